"""The expected answer of a banded LD query (vs_query_ld_band), worked out from a genotype matrix: the uint8 cells that
genotype_matrix_ref.matrix derives from the oracle's type-6 text, or any matrix of such cells.  Everything is integer arithmetic in
int64 up to the one division of the r^2, which is taken in float64 and cast to float32, as the interface defines it."""
import numpy as np


def dosage(m):
    """int64 (rows, C): popcount(cell & 6) of every cell -- 0, 1 or 2."""
    m = np.asarray(m, np.uint8)
    return (((m >> 1) & 1) + ((m >> 2) & 1)).astype(np.int64)


def gram(m):
    """int64 (rows, rows): D @ D.T of the dosages."""
    d = dosage(m)
    return d @ d.T


def moments(m):
    """(Sx, Sxx) per row, int64: the sums of the dosages and of their squares (alt_alleles, alt_alleles + 2 hom_alt)."""
    d = dosage(m)
    return d.sum(axis=1), (d * d).sum(axis=1)


def r2_values(sxy, sx, sxx, sy, syy, n):
    """float32 r^2 of pairs from their exact sums: cov = n Sxy - Sx Sy, vx = n Sxx - Sx^2, vy = n Syy - Sy^2 in int64, then
    (float)((double)cov * (double)cov / ((double)vx * (double)vy)), and 0 where vx or vy is 0.  Also returns that zero mask."""
    sxy, sx, sxx, sy, syy = (np.asarray(a, np.int64) for a in (sxy, sx, sxx, sy, syy))
    n = np.int64(n)
    cov = n * sxy - sx * sy
    vx = n * sxx - sx * sx
    vy = n * syy - sy * sy
    flat = (vx == 0) | (vy == 0)
    c = cov.astype(np.float64)
    den = vx.astype(np.float64) * vy.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = np.where(flat, 0.0, (c * c) / np.where(flat, 1.0, den))
    return r2.astype(np.float32), flat


def pair_values(m, ia, ib, stat):
    """The statistic of the row pairs (ia[k], ib[k]) of matrix m: int32 dot products ("dot") or float32 r^2 ("r2")."""
    d = dosage(m)
    ia, ib = np.asarray(ia, np.int64), np.asarray(ib, np.int64)
    sxy = (d[ia] * d[ib]).sum(axis=1) if ia.size else np.zeros(0, np.int64)
    if stat == "dot":
        return sxy.astype(np.int32)
    sx, sxx = d.sum(axis=1), (d * d).sum(axis=1)
    return r2_values(sxy, sx[ia], sxx[ia], sx[ib], sxx[ib], m.shape[1])[0]


def pair_flat(m, ia, ib):
    """bool per pair: vx * vy == 0 -- the pairs whose r^2 is 0 by definition (a monomorphic or dropped row, n = 1)."""
    sx, sxx = moments(m)
    n = np.int64(np.asarray(m).shape[1])
    v = n * sxx - sx * sx
    return (v[np.asarray(ia, np.int64)] == 0) | (v[np.asarray(ib, np.int64)] == 0)


def dot_band(m, window):
    """int32 (rows, window): band[i, k] = G[i, i + 1 + k] of G = D @ D.T, 0 where i + 1 + k is past the last row."""
    d = dosage(m)
    a = d.shape[0]
    band = np.zeros((a, window), np.int64)
    for k in range(min(window, max(a - 1, 0))):
        band[:a - 1 - k, k] = (d[:a - 1 - k] * d[1 + k:]).sum(axis=1)
    return band.astype(np.int32)


def r2_band(m, window):
    """(float32 (rows, window) r^2 band, bool mask of the cells that must be exactly 0: vx vy == 0 or past the last row)."""
    m = np.asarray(m, np.uint8)
    a = m.shape[0]
    sxy = dot_band(m, window).astype(np.int64)
    sx, sxx = moments(m)
    j = np.arange(a)[:, None] + 1 + np.arange(window)[None, :]
    past = j >= a
    jj = np.minimum(j, max(a - 1, 0))
    if a == 0:
        return np.zeros((0, window), np.float32), np.zeros((0, window), bool)
    r2, flat = r2_values(sxy, sx[:, None], sxx[:, None], sx[jj], sxx[jj], m.shape[1])
    r2 = np.where(past, np.float32(0), r2).astype(np.float32)
    return r2, flat | past


def format_value(v, stat):
    """A band cell as vs_result_format_region prints it: %d or %.6g."""
    return "%d" % int(v) if stat == "dot" else "%.6g" % float(v)


def ld_text(parsed, q, m, window, stat, table_index=None):
    """The text vs_result_format_region gives for region q of an LD result: m is genotype_matrix_ref.matrix(parsed, names) over the
    query's columns; table_index[i]: the table row of reference row i (None: region q's rows are consecutive in the table -- no
    row of it was dropped)."""
    head = "PosA\tRefA\tAltA\tPosB\tRefB\tAltB\t" + ("Dot" if stat == "dot" else "R2") + "\n"
    a0, n = int(parsed.row_begin[q]), int(parsed.row_count[q])
    rows = np.arange(a0, a0 + n)
    at = rows if table_index is None else np.asarray(table_index, np.int64)[rows]
    ia, ib = [], []
    for x in range(n):
        for y in range(x + 1, n):
            if at[y] - at[x] > window:
                break
            ia.append(rows[x])
            ib.append(rows[y])
    vals = pair_values(m, ia, ib, stat)
    return head + "".join(f"{parsed.heads[i]}\t{parsed.heads[j]}\t{format_value(v, stat)}\n" for i, j, v in zip(ia, ib, vals))
