"""The expected answer of a score-matrix query (vs_query_score_matrix), worked out from query type 6's text through
genotype_matrix_ref exactly as sample_scores_ref does it: the rows the texts list, region after region, are the reports the weights
are keyed by, and the dosage of a (report, sample) pair is popc(cell & 6).  The quantisation is the trait quantiser's, restated with
numpy: frexp of the column's largest |w|, f = 30 - e, rint of w 2^f in float64, int64 sums, astype(float64) and ldexp.  `totals` and
`limbs_needed` restate what the kernel multiplies with: the sum of a column's fixed-point weights over the reports of one table row,
and the balanced base-256 digits that hold the largest of them."""
import numpy as np

import sample_scores_ref as _ss

SHIFT = 30
MAX4 = 127 * (256 ** 4 - 1) // 255   # 2,139,062,143: the largest |T| four digits in [-128, 127] hold
MAX5 = 127 * (256 ** 5 - 1) // 255   # 547,599,908,735
MAX_TOTAL = 1 << 38

fsum = _ss.fsum
scores = _ss.scores
reported_rows = _ss.reported_rows


def shifts(w):
    """int32 (K,): f_k = 30 - e with max |w[:, k]| = m 2^e, 0.5 <= m < 1; 0 for a column of zeros (or without rows)."""
    w = np.asarray(w, np.float32)
    if w.ndim == 1:
        w = w.reshape(-1, 1)
    f = np.zeros(w.shape[1], np.int32)
    if w.shape[0]:
        m = np.abs(w.astype(np.float64)).max(axis=0)
        nz = m != 0.0
        f[nz] = SHIFT - np.frexp(m[nz])[1]
    return f


def quantise(w, f=None):
    """int64 (N, K): rint(w 2^f_k), ties to even, from the float32 values widened to float64 (the scaling is exact)."""
    w = np.asarray(w, np.float32)
    if w.ndim == 1:
        w = w.reshape(-1, 1)
    f = shifts(w) if f is None else np.asarray(f, np.int32)
    return np.rint(np.ldexp(w.astype(np.float64), f[None, :].astype(np.int32))).astype(np.int64)


def sums(parsed, columns_by_name, w):
    """(int64 (n_cols, K) sums, int32 (K,) shifts): the exact fixed-point sums over the reports (the rows of Parsed, which w follows)."""
    p, row, col, d = _ss._cells(parsed, columns_by_name)
    w = np.asarray(w, np.float32)
    if w.ndim == 1:
        w = w.reshape(-1, 1)
    assert w.shape[0] == p.n_rows, "a row of weights per reported row"
    f = shifts(w)
    q = quantise(w, f)
    out = np.zeros((len(columns_by_name), w.shape[1]), np.int64)
    for k in range(w.shape[1]):
        np.add.at(out[:, k], col, d * q[row, k])
    return out, f


def totals(w, rows, n_table):
    """int64 (n_table, K): T[row][k], the sum of q_k over the reports of table row `row`; rows[i] is the table row of report i."""
    q = quantise(w)
    t = np.zeros((n_table, q.shape[1]), np.int64)
    np.add.at(t, np.asarray(rows, np.int64), q)
    return t


def limbs_needed(t):
    """4 or 5: the balanced base-256 digits that hold the largest |T| (which must not pass 2^38)."""
    m = int(np.abs(np.asarray(t, np.int64)).max(initial=0))
    assert m <= MAX_TOTAL, "the engine refuses such a batch"
    return 4 if m <= MAX4 else 5
