"""The expected answer of a per-sample score query (vs_query_sample_scores), worked out from query type 6's text through
genotype_matrix_ref: the rows the texts list, region after region, ARE the reports the weights are keyed by (Parsed numbers them in
exactly that order), and the dosage of a (report, sample) pair is popc(cell & 6).  The quantisation is the header's, restated with
numpy: frexp of the column's largest |w|, rint of w 2^f in float64, int64 sums, astype(float64) and ldexp.  `fsum` is the same sum
without the quantisation, in exact arithmetic rounded once."""
import math

import numpy as np

from genotype_matrix_ref import Parsed, matrix_sparse

SHIFT = 36


def shifts(w):
    """int32 (K,): f_k = 36 - e with max |w[:, k]| = m 2^e, 0.5 <= m < 1; 0 for a column of zeros (or without rows)."""
    w = np.asarray(w, np.float32)
    if w.ndim == 1:
        w = w.reshape(-1, 1)
    f = np.zeros(w.shape[1], np.int32)
    for k in range(w.shape[1]):
        m = float(np.abs(w[:, k].astype(np.float64)).max()) if w.shape[0] else 0.0
        if m != 0.0:
            f[k] = SHIFT - int(np.frexp(m)[1])
    return f


def quantise(w, f=None):
    """int64 (N, K): rint(w 2^f_k), ties to even, from the float32 values widened to float64 (the scaling is exact)."""
    w = np.asarray(w, np.float32)
    if w.ndim == 1:
        w = w.reshape(-1, 1)
    f = shifts(w) if f is None else np.asarray(f, np.int32)
    return np.rint(np.ldexp(w.astype(np.float64), f[None, :].astype(np.int32))).astype(np.int64)


def _cells(parsed, columns_by_name):
    p = parsed if isinstance(parsed, Parsed) else Parsed(parsed)
    row, col, val = matrix_sparse(p, columns_by_name)
    d = ((val >> 1) & 1).astype(np.int64) + ((val >> 2) & 1)
    return p, row, col, d


def sums(parsed, columns_by_name, w):
    """(int64 (n_cols, K) sums, int32 (K,) shifts): the exact fixed-point sums over the reports (the rows of Parsed, which w follows)."""
    p, row, col, d = _cells(parsed, columns_by_name)
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


def scores(s, f):
    """float64 (n_cols, K): ldexp((double)sums, -f_k)."""
    return np.ldexp(np.asarray(s, np.int64).astype(np.float64), -np.asarray(f, np.int32)[None, :])


def fsum(parsed, columns_by_name, w):
    """(float64 (n_cols, K): math.fsum of dosage x weight per cell, the weights unquantised; int64 (n_cols,): the reports each column
    carries) -- the products are exact in float64."""
    p, row, col, d = _cells(parsed, columns_by_name)
    w64 = np.asarray(w, np.float32).astype(np.float64)
    if w64.ndim == 1:
        w64 = w64.reshape(-1, 1)
    n, k = len(columns_by_name), w64.shape[1]
    out = np.zeros((n, k))
    carried = np.bincount(col, minlength=n).astype(np.int64)
    order = np.argsort(col, kind="stable")
    prod = d[order, None].astype(np.float64) * w64[row[order]]
    bounds = np.concatenate([[0], np.cumsum(carried)])
    for c in np.nonzero(carried)[0]:
        seg = prod[bounds[c]:bounds[c + 1]]
        for j in range(k):
            out[c, j] = math.fsum(seg[:, j])
    return out, carried


def pairs(parsed, columns_by_name, w):
    """vs_result_totals' n_carriers: the (report, carrier in the columns) pairs whose report has a weight that is not 0 once quantised."""
    p, row, _col, _d = _cells(parsed, columns_by_name)
    nz = quantise(w).any(axis=1)
    return int(nz[row].sum())


def reported_rows(row_begin, row_count, dropped):
    """The table row of every report, in report order: region after region as given, within a region its slots row_begin[q] .. +
    row_count[q] without the dropped ones; and per report its slot within its region (which a dropped row in front shifts away from
    the report's index within the region)."""
    rows, slots = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for b, n in zip(np.asarray(row_begin, np.int64), np.asarray(row_count, np.int64)):
        a = np.arange(b, b + n)
        keep = ~np.asarray(dropped, bool)[a]
        rows.append(a[keep])
        slots.append(np.nonzero(keep)[0])
    return np.concatenate(rows), np.concatenate(slots)
