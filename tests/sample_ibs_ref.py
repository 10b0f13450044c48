"""The expected answer of a pairwise IBS query (vs_query_sample_ibs), worked out from a genotype matrix: the uint8 cells that
genotype_matrix_ref.matrix derives from the oracle's type-6 text, or any matrix of such cells (rows x columns), and a mask of the
rows the duplicate rule dropped.  Everything is int64.  sample_ibs computes the answer two ways -- the indicator products and the
two identities the interface defines, and a brute-force count of the nine (d_i, d_j) state pairs -- and asserts that they agree."""
import numpy as np

from ld_band_ref import dosage


def _products(x):
    """X^T X of a 0/1 matrix as int64; through float64 where it is large (exact: every sum is far below 2^53)."""
    if x.shape[0] * x.shape[1] * x.shape[1] < 1 << 28:
        return x.T @ x
    f = x.astype(np.float64)
    return (f.T @ f).astype(np.int64)


def sample_ibs(cells, dropped=None):
    """A dict of het_het, hom_hom, carrier_both, ibs0, ibs1, ibs2 ((n, n) int64) and n_used (a Python int) of a rows x n matrix of
    cells.  `dropped`: a boolean mask of the rows the duplicate rule dropped -- their cells must be 0; they are no sites."""
    d = dosage(np.asarray(cells, np.uint8)).astype(np.int64)
    a, n = d.shape
    dropped = np.zeros(a, bool) if dropped is None else np.asarray(dropped, bool)
    assert dropped.shape == (a,) and not d[dropped].any(), "a dropped row has an all-zero matrix row"
    n_used = int(a - dropped.sum())
    # 1. the interface's definition: three indicator products, the rest from them and their diagonals
    h, hom, c = (d == 1).astype(np.int64), (d == 2).astype(np.int64), (d > 0).astype(np.int64)
    hh, aa, cc = _products(h), _products(hom), _products(c)
    na, nc = np.diagonal(aa), np.diagonal(cc)
    ibs0 = na[:, None] + na[None, :] - 2 * aa - (cc - hh - aa)
    ibs2 = n_used - nc[:, None] - nc[None, :] + cc + hh + aa
    ibs1 = n_used - ibs0 - ibs2
    # 2. brute force: the nine state pairs counted over the kept rows
    k = d[~dropped]
    state = [(k == s).astype(np.int64) for s in (0, 1, 2)]
    pair = [[_products_ab(state[x], state[y]) for y in range(3)] for x in range(3)]
    assert np.array_equal(hh, pair[1][1]) and np.array_equal(aa, pair[2][2])
    assert np.array_equal(cc, pair[1][1] + pair[1][2] + pair[2][1] + pair[2][2])
    assert np.array_equal(ibs0, pair[0][2] + pair[2][0]), "ibs0: the opposite homozygotes"
    assert np.array_equal(ibs2, pair[0][0] + pair[1][1] + pair[2][2]), "ibs2: equal dosage"
    assert np.array_equal(ibs1, pair[0][1] + pair[1][0] + pair[1][2] + pair[2][1]), "ibs1: one allele apart"
    return {"het_het": hh, "hom_hom": aa, "carrier_both": cc, "ibs0": ibs0, "ibs1": ibs1, "ibs2": ibs2, "n_used": n_used}


def _products_ab(x, y):
    if x.shape[0] * x.shape[1] * x.shape[1] < 1 << 28:
        return x.T @ y
    return (x.T.astype(np.float64) @ y.astype(np.float64)).astype(np.int64)


def king(het_het, ibs0):
    """float64 (n, n): float(het_het - 2 ibs0) / float(nh_i + nh_j), nh the diagonal of het_het, and 0.0 where nh_i + nh_j == 0.
    Both integers lie below 2^53: each converts exactly and one division follows."""
    hh, i0 = np.asarray(het_het, np.int64), np.asarray(ibs0, np.int64)
    nh = np.diagonal(hh)
    den = nh[:, None] + nh[None, :]
    num = hh - 2 * i0
    out = np.zeros(hh.shape, np.float64)
    nz = den != 0
    out[nz] = num[nz].astype(np.float64) / den[nz].astype(np.float64)
    return out


def ibs_text(names, got, stat, min_kinship=None):
    """What `variantstore ibs` writes from a result's arrays (QueryResult.sample_ibs or sample_ibs above, with `king` under stat
    "king"): a header line, then a line per pair i < j in column order -- integers as %lld, the kinship as %.17g; under
    `min_kinship` (which implies "king") only the pairs with king >= min_kinship."""
    with_king = stat == "king" or min_kinship is not None
    out = "ID1\tID2\tN\tHetHet\tIBS0\tIBS1\tIBS2" + ("\tKinship" if with_king else "") + "\n"
    n = len(names)
    for i in range(n):
        for j in range(i + 1, n):
            if min_kinship is not None and not float(got["king"][i, j]) >= min_kinship:
                continue
            out += "%s\t%s\t%d\t%d\t%d\t%d\t%d" % (names[i], names[j], int(got["n_used"]), int(got["het_het"][i, j]), int(got["ibs0"][i, j]),
                                                   int(got["ibs1"][i, j]), int(got["ibs2"][i, j]))
            if with_king:
                out += "\t%.17g" % float(got["king"][i, j])
            out += "\n"
    return out
