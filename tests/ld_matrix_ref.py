"""The expected answer of an LD-matrix query (vs_query_ld_matrix), worked out from a genotype matrix through ld_band_ref: the uint8
cells that genotype_matrix_ref.matrix derives from the oracle's type-6 text, or the engine's own matrix.  A block is the full
symmetric square of a region's rows, diagonal included; integer arithmetic in int64 up to the one division of the r^2."""
import numpy as np

from ld_band_ref import format_value, gram, moments, r2_values


def block(m, stat):
    """The block of the rows of matrix m (rows x columns of genotype cells): int32 D @ D.T under "dot", float32 r^2 under "r2"."""
    m = np.asarray(m, np.uint8)
    g = gram(m)
    if stat == "dot":
        return g.astype(np.int32)
    return block_r2(m)[0]


def block_r2(m):
    """(float32 (rows, rows) r^2, bool mask of the cells that must be exactly 0: vx vy == 0 -- a monomorphic or dropped row, n = 1)."""
    m = np.asarray(m, np.uint8)
    a = m.shape[0]
    if a == 0:
        return np.zeros((0, 0), np.float32), np.zeros((0, 0), bool)
    sx, sxx = moments(m)
    return r2_values(gram(m), sx[:, None], sxx[:, None], sx[None, :], sxx[None, :], m.shape[1])


def block_begin(row_count):
    """uint64 (Q + 1): the exclusive scan of m_q^2."""
    m = np.asarray(row_count, np.uint64)
    out = np.zeros(m.shape[0] + 1, np.uint64)
    np.cumsum(m * m, out=out[1:])
    return out


def blocks(cells, row_begin, row_count, stat):
    """(flat cells, block_begin) of a batch from the whole table's matrix `cells` and the per-region row ranges: block after block,
    each row-major."""
    dtype = np.int32 if stat == "dot" else np.float32
    parts = [block(cells[int(b):int(b) + int(c)], stat).reshape(-1) for b, c in zip(row_begin, row_count)]
    flat = np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)
    return flat, block_begin(row_count)


def ld_matrix_text(parsed, q, m, stat):
    """The text vs_result_format_region gives for region q of an LD-matrix result: m is genotype_matrix_ref.matrix(parsed, names)
    over the query's columns, whose rows are the reported, non-dropped rows -- the only ones the text holds."""
    a0, n = int(parsed.row_begin[q]), int(parsed.row_count[q])
    b = block(m[a0:a0 + n], stat)
    head = "Pos\tRef\tAlt" + "".join("\t" + parsed.heads[a0 + k].replace("\t", ":") for k in range(n)) + "\n"
    return head + "".join(parsed.heads[a0 + x] + "".join("\t" + format_value(b[x, y], stat) for y in range(n)) + "\n" for x in range(n))
