"""The expected answer of an association scan (vs_query_assoc_scan), worked out from query type 6's text through
genotype_matrix_ref: the dosage matrix of the rows the texts list (popc(cell & 6) per carrier) times the phenotypes Y -- the oracle
has no such function of its own.  Integer-valued Y is summed in int64 (exact), real Y in float64 with math.fsum per cell; the score
test is formed in float64 in the order the header states."""
import math

import numpy as np

from genotype_matrix_ref import Parsed, matrix_sparse

COUNT_HEADER = "Pos\tRef\tAlt\tCarriers\tAC\tHomAlt\tPhased"


def dosages(parsed, columns_by_name):
    """The nonzero cells of the dosage matrix: (row, column, dosage 0 .. 2, genotype byte), rows as in Parsed, sorted by (row, column)."""
    p = parsed if isinstance(parsed, Parsed) else Parsed(parsed)
    row, col, val = matrix_sparse(p, columns_by_name)
    d = ((val >> 1) & 1).astype(np.int64) + ((val >> 2) & 1)
    return row, col, d, val


def counts(parsed, columns_by_name):
    """int64 (n_rows, 4): carriers, alt_alleles, hom_alt, phased of every row over the columns."""
    p = parsed if isinstance(parsed, Parsed) else Parsed(parsed)
    row, _col, d, val = dosages(p, columns_by_name)
    out = np.zeros((p.n_rows, 4), np.int64)
    for f, w in enumerate((np.ones_like(d), d, (d == 2).astype(np.int64), (val & 1).astype(np.int64))):
        out[:, f] = np.bincount(row, weights=w, minlength=p.n_rows).astype(np.int64)
    return out


def dot_int(parsed, columns_by_name, y):
    """int64 (n_rows, K): sum of dosage x value for integer-valued y (n_cols, K)."""
    p = parsed if isinstance(parsed, Parsed) else Parsed(parsed)
    yi = np.asarray(y).astype(np.int64)
    assert np.array_equal(yi, np.asarray(y)), "dot_int takes integer-valued phenotypes"
    row, col, d, _val = dosages(p, columns_by_name)
    out = np.zeros((p.n_rows, yi.shape[1]), np.int64)
    for k in range(yi.shape[1]):   # (integer sums far below 2^53: exact as float64 weights)
        out[:, k] = np.rint(np.bincount(row, weights=(d * yi[col, k]).astype(np.float64), minlength=p.n_rows)).astype(np.int64)
    return out


def dot_fsum(parsed, columns_by_name, y):
    """(float64 (n_rows, K) of math.fsum per cell, float64 (n_rows, K) of sum |d y|, int64 (n_rows,) carriers in the columns) for
    real y (n_cols, K) float32: the products are exact in float64."""
    p = parsed if isinstance(parsed, Parsed) else Parsed(parsed)
    y64 = np.asarray(y, np.float32).astype(np.float64)
    row, col, d, _val = dosages(p, columns_by_name)
    k = y64.shape[1]
    out, mag = np.zeros((p.n_rows, k)), np.zeros((p.n_rows, k))
    m = np.bincount(row, minlength=p.n_rows).astype(np.int64)
    prod = d[:, None].astype(np.float64) * y64[col]
    bounds = np.concatenate([[0], np.cumsum(m)])
    for i in np.nonzero(m)[0]:
        seg = prod[bounds[i]:bounds[i + 1]]
        for j in range(k):
            out[i, j] = math.fsum(seg[:, j])
            mag[i, j] = math.fsum(np.abs(seg[:, j]))
    return out, mag, m


def trait_sums(y):
    """(Sy, Syy) per trait as the engine forms them: left to right in column order, in float64 from the float32 values."""
    y64 = np.asarray(y, np.float32).astype(np.float64)
    sy, syy = np.zeros(y64.shape[1]), np.zeros(y64.shape[1])
    for r in y64:
        sy = sy + r
        syy = syy + r * r
    return sy, syy


def pivots(y):
    """The pivot of every trait as the engine chooses it: the trait VALUE nearest Sy / n (float64, Sy as trait_sums forms it), of
    equally near ones the first in column order -- a value of the trait's own grid, so integer-valued traits keep integer sums."""
    y64 = np.asarray(y, np.float32).astype(np.float64)
    mean = trait_sums(y)[0] / np.float64(y64.shape[0])
    return y64[np.argmin(np.abs(y64 - mean[None, :]), axis=0), np.arange(y64.shape[1])]


def trait_sums_about(y, c):
    """(Sy~, Syy~) per trait about the pivots c (K,): y~ = y - c in float64, then left to right in column order as trait_sums."""
    yt = np.asarray(y, np.float32).astype(np.float64) - np.asarray(c, np.float64)[None, :]
    sy, syy = np.zeros(yt.shape[1]), np.zeros(yt.shape[1])
    for r in yt:
        sy = sy + r
        syy = syy + r * r
    return sy, syy


def dot_sequential(dosage, y, c=None):
    """float64 (A, K): sum of dosage x (y - c) over a dense dosage matrix (A, n), the carriers added left to right in column order
    (c None: 0).  The kernel adds the same terms in a tree fixed by the table's layout; this is the plainest order."""
    y64 = np.asarray(y, np.float32).astype(np.float64)
    if c is not None:
        y64 = y64 - np.asarray(c, np.float64)[None, :]
    d = np.asarray(dosage, np.float64)
    out = np.zeros((d.shape[0], y64.shape[1]))
    for j in range(d.shape[1]):   # (a sample that does not carry the row adds 0.0: the sum stays as it is)
        out = out + d[:, j, None] * y64[None, j, :]
    return out


def chi2_uncentred(n, alt_alleles, hom_alt, dosage, y):
    """The score test as the engine formed it before the sums were taken about a pivot: chi2() over the raw Sy, Syy and Sxy.  cov and
    vy cancel at the scale of the trait's mean; tests/test_assoc_exact_host.py keeps this to show that the exact check rejects it."""
    sy, syy = trait_sums(y)
    return chi2(n, alt_alleles, hom_alt, sy, syy, dot_sequential(dosage, y))


def chi2_centred(n, alt_alleles, hom_alt, dosage, y):
    """The score test in the engine's order: the pivots, Sy~ / Syy~ and Sxy~ about them, then chi2() (the statistic does not change
    when a constant is taken off the trait)."""
    c = pivots(y)
    sy, syy = trait_sums_about(y, c)
    return chi2(n, alt_alleles, hom_alt, sy, syy, dot_sequential(dosage, y, c))


def chi2(n, alt_alleles, hom_alt, sy, syy, sxy):
    """The score test in float64, every operation rounded on its own in the stated order: sxy (A, K), alt_alleles / hom_alt (A,)
    integers, sy / syy (K,) -- for VS_ASSOC_CHI2 the three sums about the traits' pivots.  0.0 where vx == 0 or vy <= 0."""
    sx = np.asarray(alt_alleles).astype(np.int64)
    sxx = sx + 2 * np.asarray(hom_alt).astype(np.int64)
    vx = (np.int64(n) * sxx - sx * sx)[:, None]
    dn = np.float64(n)
    sxy = np.asarray(sxy, np.float64)
    cov = dn * sxy - sx.astype(np.float64)[:, None] * np.asarray(sy, np.float64)[None, :]
    vy = (dn * np.asarray(syy, np.float64) - np.asarray(sy, np.float64) * np.asarray(sy, np.float64))[None, :]
    ok = (vx != 0) & (vy > 0.0)
    den = np.where(ok, vx.astype(np.float64) * vy, 1.0)
    return np.where(ok, (dn * cov) * cov / den, 0.0)


def assoc_text(parsed, q, cnt, scores, trait_names=None):
    """The text vs_result_format_region gives for region q: cnt = counts(...), scores (n_rows, K) over the rows of Parsed."""
    k = scores.shape[1]
    names = [str(i) for i in range(k)] if trait_names is None else list(trait_names)
    out = [COUNT_HEADER + "".join("\t" + n for n in names) + "\n"]
    a0 = int(parsed.row_begin[q])
    for i in range(a0, a0 + int(parsed.row_count[q])):
        out.append(parsed.heads[i] + "".join(f"\t{int(v)}" for v in cnt[i]) + "".join("\t%.17g" % float(v) for v in scores[i]) + "\n")
    return "".join(out)
