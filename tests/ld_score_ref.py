"""The expected answer of an LD-score query (vs_query_ld_scores), worked out from a genotype-matrix cell array (the uint8 cells of
genotype_matrix_ref.matrix or of the engine's own genotype_matrix()) in PYTHON INTEGERS: every summed value is
(cov * cov << 32) // (va * vb), no floating-point value takes part.  Eligibility is ld_prune_ref.eligible."""
import numpy as np

from ld_band_ref import dosage
from ld_prune_ref import eligible, row_counts

ONE = 1 << 32   # the value of r2 = 1
SCORED, INELIGIBLE, DROPPED = 1, 2, 3
STATE_WORD = {SCORED: "scored", INELIGIBLE: "skip"}


def q32(cov, va, vb):
    """floor(cov^2 2^32 / (va vb)) of an eligible pair, a Python integer."""
    return ((int(cov) * int(cov)) << 32) // (int(va) * int(vb))


def moments(cells):
    """(d int64 [rows, n], ac int64, v int64) of the cells: dosages, alt_alleles and n Sxx - Sx^2 per row."""
    d = dosage(cells).astype(np.int64)
    n = d.shape[1]
    ac, hom = row_counts(cells)
    return d, ac.astype(np.int64), np.int64(n) * (ac + 2 * hom) - ac * ac


def ld_scores(cells, dropped, pos, row_begin, row_count, window=0, max_bp=0, min_ac=0, max_ac=0xFFFFFFFF, detail=None):
    """(sums uint64, n_pairs uint32, state uint8 -- each [sum(row_count)] --, keep_begin uint64 [Q + 1], n_scored uint64 [Q]) by the
    definition: for an eligible row a of region q the sum of q32(a, b) over the eligible rows b of the same region, b = a included,
    with |a - b| <= window (window 0: no limit) and |pos_a - pos_b| <= max_bp (max_bp 0: no limit).
    `detail`: a dict that receives what the tests ask of their inputs -- `cut_window` and `cut_bp`, the eligible pairs of one region
    (ordered, b != a) beyond the row limit / beyond the position limit (a pair beyond both counts in both), and `max_num`, the
    largest cov^2 2^32 summed."""
    cells = np.asarray(cells, np.uint8)
    dropped = np.asarray(dropped, bool)
    pos = np.asarray(pos, np.int64)
    ok = eligible(cells, dropped, min_ac, max_ac)
    d, ac, v = moments(cells)
    n = d.shape[1]
    row_begin, row_count = np.asarray(row_begin, np.int64), np.asarray(row_count, np.int64)
    Q = row_begin.shape[0]
    keep_begin = np.zeros(Q + 1, np.uint64)
    keep_begin[1:] = np.cumsum(row_count)
    total = int(keep_begin[-1])
    sums, n_pairs, state = np.zeros(total, np.uint64), np.zeros(total, np.uint32), np.zeros(total, np.uint8)
    n_scored = np.zeros(Q, np.uint64)
    cut_window = cut_bp = max_num = 0
    vo = v.astype(object)
    for q in range(Q):
        a0, m, o = int(row_begin[q]), int(row_count[q]), int(keep_begin[q])
        rows = np.arange(a0, a0 + m)
        state[o:o + m] = np.where(dropped[rows], DROPPED, np.where(ok[rows], SCORED, INELIGIBLE))
        e = rows[ok[rows]]
        n_scored[q] = e.shape[0]
        if not e.shape[0]:
            continue
        sxy = d[e] @ d[e].T
        cov = (np.int64(n) * sxy - np.outer(ac[e], ac[e])).astype(object)
        num = cov * cov * ONE
        quo = num // np.outer(vo[e], vo[e])
        in_rows = np.ones((e.shape[0], e.shape[0]), bool) if not window else np.abs(e[:, None] - e[None, :]) <= window
        in_bp = np.ones_like(in_rows) if not max_bp else np.abs(pos[e][:, None] - pos[e][None, :]) <= max_bp
        use = in_rows & in_bp
        cut_window += int((~in_rows).sum())
        cut_bp += int((~in_bp).sum())
        if use.any():
            max_num = max(max_num, int(max(num[use])))
        s = np.where(use, quo, 0).sum(axis=1)
        sums[o + e - a0] = np.asarray([int(x) for x in s], np.uint64)
        n_pairs[o + e - a0] = use.sum(axis=1).astype(np.uint32)
    if detail is not None:
        detail.update(cut_window=cut_window, cut_bp=cut_bp, max_num=max_num)
    return sums, n_pairs, state, keep_begin, n_scored


def score_text(heads, ac, n_pairs, sums, state):
    """The text vs_result_format_region gives for one region of an LD-score result: heads, ac, n_pairs, sums and state of the
    region's table rows in order (heads[i] = "Pos\\tRef\\tAlt"; dropped rows are left out).  L2 is sums / 2^32 as %.6f: the
    division by a power of two is exact in a double up to sums of 2^53, far above any region a test forms."""
    head = "Pos\tRef\tAlt\tAC\tPairs\tL2\tState\n"
    return head + "".join(f"{h}\t{int(c)}\t{int(p)}\t{int(s) / ONE:.6f}\t{STATE_WORD[int(t)]}\n"
                          for h, c, p, s, t in zip(heads, ac, n_pairs, sums, state) if int(t) != DROPPED)
