"""The score statistic of an association scan, exactly: chi2 = n cov^2 / (vx vy) per (row, trait) in Python integers from a dosage
matrix (rows x columns of 0 / 1 / 2) and the float32 trait values as given, and how far the engine's float64 formula
(k_assoc.hip.h: assoc_chi2 over sums taken about a per-trait pivot) may be from it.  Nothing here reads an output of the engine.

A float32 is a dyadic rational: a trait column is scaled to integers once (scaled), so a table costs integer dot products -- split
into 26-bit limbs that numpy's int64 holds exactly -- and one Fraction per cell.  The statistic does not change when a constant is
added to the trait, so the value is formed from the raw integers and the bound from the integers about the pivot."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53   # the unit roundoff of float64: one correctly rounded operation errs by at most U, relatively
LIMB = 26


def scaled(y):
    """([Python int], s) with y[j] == ints[j] / 2^s exactly, for one float32 column."""
    y = np.asarray(y, np.float32)
    assert y.ndim == 1 and np.isfinite(y).all()
    m, e = np.frexp(y.astype(np.float64))                 # y = m 2^e, 0.5 <= |m| < 1: m 2^24 is an integer (24 significant bits)
    mant = np.ldexp(m, 24)
    assert np.array_equal(mant, np.rint(mant))
    ex = e.astype(np.int64) - 24
    nz = mant != 0
    s = int(-ex[nz].min()) if nz.any() else 0
    ints = [int(a) << (int(b) + s) if a else 0 for a, b in zip(mant.astype(np.int64).tolist(), ex.tolist())]
    low = 0
    for v in ints:
        low |= v
    spare = (low & -low).bit_length() - 1 if low else 0      # zeros every value ends in: the grid is coarser than the smallest ulp
    return [v >> spare for v in ints], s - spare


def int_dot(d, ints):
    """[Python int] per row: d (A, n) int64 of small non-negative integers times a column of Python integers, exactly."""
    d = np.asarray(d, np.int64)
    out = [0] * d.shape[0]
    sign = np.array([-1 if v < 0 else 1 for v in ints], np.int64)
    mag = [abs(v) for v in ints]
    shift = 0
    while any(mag):
        limb = np.array([v & ((1 << LIMB) - 1) for v in mag], np.int64) * sign
        assert int(d.max(initial=0)) * d.shape[1] < 1 << (62 - LIMB)
        for i, v in enumerate((d @ limb).tolist()):
            out[i] += v << shift
        mag = [v >> LIMB for v in mag]
        shift += LIMB
    return out


def pivot(ints):
    """The index of the trait value nearest the exact mean; of equally near ones the first in column order."""
    n, total = len(ints), sum(ints)
    return min(range(n), key=lambda j: (abs(n * ints[j] - total), j))


def row_moments(d):
    """Per row, as Python integers: (carriers m, Sx, vx = n Sxx - Sx^2)."""
    d = np.asarray(d, np.int64)
    n = d.shape[1]
    m, sx, sxx = (d != 0).sum(axis=1).tolist(), d.sum(axis=1).tolist(), (d * d).sum(axis=1).tolist()
    return m, sx, [n * b - a * a for a, b in zip(sx, sxx)]


def table(d, y):
    """(chi2 float64 (A, K), bound float64 (A, K)) of the dosage matrix d (A, n) and the float32 traits y (n, K).

    chi2 is the exact statistic rounded once to float64 (0 where vx == 0 or vy == 0).  bound is the absolute distance the engine's
    value may have from the exact one (so from chi2 by U chi2 more): a first-order count of its correctly rounded operations with
    the exact magnitudes, x 1.001 for the second-order terms, in the style of window_stats_ref.exact_tajima.

    What keeps the bound small is the grid.  The values of a float32 trait are whole multiples of g = 2^-s (scaled), and so are the
    pivot, every y~ = y - c and every sum of terms d y~.  A whole multiple of g below 2^53 g is a float64, so an operation whose
    exact result is one does not round -- in whatever order a sum is taken.  Below, "(1)" is a rounding that is counted only where
    the exact result, in units of g (g^2 for squares), reaches 2^53; m is the row's carriers, every magnitude the exact one:
      y~           one subtraction (1): U |y~|
      Sxy~         m terms d y~ (exact products) added in ANY order; every partial sum is at most A = sum d |y~|: nothing where
                   A < 2^53 g, else m U A with the subtractions
      Sy~, Syy~    n terms left to right on the host, B = sum |y~|, Q = sum y~^2: nothing where B < 2^53 g (Q < 2^53 g^2), else
                   n U B ((n + 2) U Q: the square of a rounded y~ is off by 3 U)
      cov          p1 = n Sxy~ (1), p2 = Sx Sy~ (1), p1 - p2 (1): n dSxy + Sx dSy + U (|p1| + |p2| + |cov|)
      vy           q1 = n Syy~ (1), q2 = Sy~^2 (1), q1 - q2 (1): n dSyy + 2 |Sy~| dSy + U (q1 + q2 + vy)
      chi2         (n cov) cov (2), vx vy (1; vx is an exact integer below 2^53), the division (1):
                   chi2 (dvy / vy + 4 U) + n (2 |cov| dcov + dcov^2) / (vx vy)
    The bound is infinite where dvy reaches vy / 2: the engine could then see no variance at all, and such a trait is no test case.
    """
    d = np.asarray(d, np.int64)
    y = np.asarray(y, np.float32)
    a, n = d.shape
    assert y.shape[0] == n and set(np.unique(d).tolist()) <= {0, 1, 2}
    m, sx, vx = row_moments(d)
    val, bound = np.zeros((a, y.shape[1])), np.zeros((a, y.shape[1]))
    for k in range(y.shape[1]):
        raw, _s = scaled(y[:, k])
        sy, syy = sum(raw), sum(v * v for v in raw)
        vy = n * syy - sy * sy
        if vy == 0:
            continue   # every value equal: y~ = 0 exactly, the engine's vy is 0
        sxy = int_dot(d, raw)
        c = raw[pivot(raw)]
        ct = [v - c for v in raw]
        st, b, q = sum(ct), sum(abs(v) for v in ct), sum(v * v for v in ct)
        assert n * q - st * st == vy
        sxy_t, a_abs = int_dot(d, ct), int_dot(d, [abs(v) for v in ct])
        big = 1 << 53
        r = lambda v: U * abs(v) if abs(v) >= big else 0.0          # a rounding that happens only off the grid's exact range
        d_sy, d_syy = (n * U * b if b >= big else 0.0), ((n + 2) * U * q if q >= big else 0.0)
        d_vy = n * d_syy + 2 * abs(st) * d_sy + r(n * q) + r(st * st) + r(vy)
        for i in range(a):
            if vx[i] == 0:
                continue
            cov = n * sxy[i] - sx[i] * sy
            assert cov == n * sxy_t[i] - sx[i] * st
            chi = Fraction(n * cov * cov, vx[i] * vy)
            val[i, k] = float(chi)
            if 2 * d_vy >= vy:
                bound[i, k] = np.inf
                continue
            d_sxy = m[i] * U * a_abs[i] if a_abs[i] >= big else 0.0
            d_cov = n * d_sxy + sx[i] * d_sy + r(n * sxy_t[i]) + r(sx[i] * st) + r(cov)
            first = float(chi) * (d_vy / vy + 4 * U) + float(Fraction(n, vx[i] * vy)) * (2 * abs(cov) * d_cov + d_cov * d_cov)
            bound[i, k] = 1.001 * first / (1 - 2 * d_vy / vy)
    return val, bound


def cap(n, chi2):
    """What a bound may be at most for its case to count as a test: 8 n 2^-53 max(chi2, 1)."""
    return 8 * n * U * np.maximum(chi2, 1.0)


def trend(n_case, n_ctrl, case_ac, case_hom, case_car, ctrl_ac, ctrl_hom, ctrl_car):
    """The Cochran-Armitage trend statistic of one row, as a Fraction, from the count records of cases and controls (carriers,
    alt_alleles and hom_alt of each: carriers - hom_alt heterozygotes), with the dosages 0, 1, 2 as weights w_i:
    N (N sum_i w_i r_i - R sum_i w_i n_i)^2 / (R (N - R) (N sum_i w_i^2 n_i - (sum_i w_i n_i)^2)), r_i the cases and n_i everybody
    with genotype i, R the cases, N everybody.  None where a factor of the denominator is 0."""
    big_n, r = n_case + n_ctrl, n_case
    assert case_ac == (case_car - case_hom) + 2 * case_hom and ctrl_ac == (ctrl_car - ctrl_hom) + 2 * ctrl_hom
    wr = case_ac                                               # sum w_i r_i
    wn = case_ac + ctrl_ac                                     # sum w_i n_i
    w2n = (case_car - case_hom) + (ctrl_car - ctrl_hom) + 4 * (case_hom + ctrl_hom)
    den = r * (big_n - r) * (big_n * w2n - wn * wn)
    return Fraction(big_n * (big_n * wr - r * wn) ** 2, den) if den else None


# ---- the trait ladder both test files use ------------------------------------------------------------------------------------
LADDER = ("normal", "170+-7", "1e4+-1", "1e6+-100", "1e6+-1", "-3e7+-50", "1e-3+-1e-6", "label", "int+1e6", "int", "0.1f",
          "near_constant", "correlated")
SHIFTED = (("int", "int+1e6", 1_000_000.0),)   # (base, shifted, the float32-representable constant between them)


def snap(col):
    """The column on the grid vs_query_assoc_matrix quantises it to (assoc_matrix_ref.quantise: 30 bits below the largest value's
    exponent), so that both queries answer about the same numbers.  Only values 2^6 times smaller than the largest one move."""
    import assoc_matrix_ref
    q, f = assoc_matrix_ref.quantise(np.asarray(col, np.float32))
    out = np.ldexp(q[:, 0].astype(np.float64), -int(f[0])).astype(np.float32)
    q2, f2 = assoc_matrix_ref.quantise(out)
    assert np.array_equal(q, q2) and np.array_equal(f, f2) and np.array_equal(np.ldexp(q[:, 0].astype(np.float64), -int(f[0])), out)
    return out


def ladder(rng, n, dosage_row):
    """{name: float32 (n,)}: traits from zero mean to a mean 10^6 standard deviations away, exact-sum traits, a constant that is no
    dyadic fraction, a constant with one sample one unit off, and a trait that follows `dosage_row` (chi2 of the order of n)."""
    z = lambda: rng.standard_normal(n)
    ints = rng.integers(-8, 9, size=n).astype(np.float64)
    near = np.full(n, np.float32(1e6 + 0.3), np.float32)
    near[n // 3] += np.float32(1.0)
    out = {"normal": z(), "170+-7": 170 + 7 * z(), "1e4+-1": 1e4 + z(), "1e6+-100": 1e6 + 100 * z(), "1e6+-1": 1e6 + z(),
           "-3e7+-50": -3e7 + 50 * z(), "1e-3+-1e-6": 1e-3 + 1e-6 * z(), "label": rng.integers(0, 2, size=n).astype(np.float64),
           "int+1e6": ints + 1_000_000.0, "int": ints, "0.1f": np.full(n, np.float32(0.1)), "near_constant": near,
           "correlated": np.asarray(dosage_row, np.float64) + 0.25 * z()}
    assert tuple(out) == LADDER
    return {k: snap(np.asarray(v, np.float32)) for k, v in out.items()}
