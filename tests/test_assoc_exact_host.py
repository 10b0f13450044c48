"""The association scan's score statistic on the CPU: the restated float64 formulas (assoc_scan_ref) and assoc_matrix_ref.chi2
against the exact rational statistic (assoc_exact_ref) on the trait ladder -- from a zero-mean trait to one whose mean lies 10^6
standard deviations from zero -- at 63, 300, 2,504 and 8,255 samples (4,159 as well where the near-constant trait is concerned).

  (a) the formula over the RAW sums (assoc_scan_ref.chi2_uncentred, what the engine computed before it took its sums about a pivot)
      is REJECTED by the exact check: off by more than 1e-4 at mean / sd = 10^6, and 0.0 in every cell of the near-constant trait
  (b) the formula about the pivot (chi2_centred: the engine's order, the carriers added left to right) stays within the derived
      bound, and the bound within 8 n 2^-53 max(chi2, 1) on every case of the ladder
  (c) assoc_matrix_ref.chi2_table, formed from exact integers with four roundings, stays within 8 * 2^-53 relative
and the reference against itself: the Cochran-Armitage trend statistic of the 0/1 label, a shifted trait, the brute-force Fraction
statistic of a small table, the pivot rule in float64 against the exact one."""
from fractions import Fraction

import numpy as np
import pytest

import assoc_exact_ref as ex
import assoc_matrix_ref
import assoc_scan_ref as ref

U = ex.U
SIZES = (63, 300, 2504, 8255)


def dosages(rng, n, a=20):
    """(a, n) int64 of 0 / 1 / 2: rare to saturated rows; row 0 everybody hom-alt (no variance), row 1 everybody but the first
    sample, row 2 everybody but the last with mixed calls, row 3 everybody heterozygous (no variance)."""
    p = rng.choice([0.004, 0.03, 0.2, 0.5, 0.9], size=a)
    d = (rng.random((a, n)) < p[:, None]).astype(np.int64) + (rng.random((a, n)) < p[:, None])
    d[0] = 2
    d[1] = 2
    d[1, 0] = 0
    d[2] = rng.integers(1, 3, size=n)
    d[2, n - 1] = 0
    d[3] = 1
    return d


_CASES = {}


def case(n):
    """(dosage, traits (n, 13) in ex.LADDER's order, exact chi2, bound) of the cohort of n samples, computed once."""
    if n not in _CASES:
        rng = np.random.default_rng(n)
        d = dosages(rng, n)
        lad = ex.ladder(rng, n, d[5])
        y = np.stack([lad[k] for k in ex.LADDER], axis=1)
        _CASES[n] = (d, y) + ex.table(d, y)
    return _CASES[n]


def col(name):
    return ex.LADDER.index(name)


def counts(d):
    return d.sum(axis=1), (d == 2).sum(axis=1)


def test_exact_reference_against_brute_force():
    """The integer route (scaling, limbs, one Fraction per cell) against Fractions of the float32 values themselves."""
    d, y, val, _bound = case(63)
    n = 63
    for k in (col("normal"), col("1e6+-1"), col("1e-3+-1e-6"), col("0.1f")):
        yk = [Fraction(float(v)) for v in y[:, k]]
        sy, syy = sum(yk), sum(v * v for v in yk)
        for i in range(d.shape[0]):
            x = [int(v) for v in d[i]]
            sx, sxx, sxy = sum(x), sum(v * v for v in x), sum(a * b for a, b in zip(x, yk))
            vx, vy = n * sxx - sx * sx, n * syy - sy * sy
            want = float(n * (n * sxy - sx * sy) ** 2 / (vx * vy)) if vx and vy else 0.0
            assert val[i, k] == want, (i, k)
    assert not val[[0, 3]].any() and not val[:, col("0.1f")].any() and val[1].any() and val[2].any()
    ints, s = ex.scaled(y[:, col("1e6+-1")])
    assert [Fraction(v, 2 ** s) for v in ints] == [Fraction(float(v)) for v in y[:, col("1e6+-1")]]


@pytest.mark.parametrize("n", SIZES)
def test_shift_and_label(n):
    """A trait and the same trait 1,000,000 higher have the same exact statistic; the 0/1 label's is the trend statistic."""
    d, y, val, _bound = case(n)
    for base, shifted, by in ex.SHIFTED:
        assert np.array_equal(y[:, col(base)] + np.float32(by), y[:, col(shifted)])
        assert np.array_equal(val[:, col(base)], val[:, col(shifted)]) and val[:, col(base)].any()
    lab = y[:, col("label")] == 1
    for i in range(d.shape[0]):
        ca, co = d[i, lab], d[i, ~lab]
        t = ex.trend(int(lab.sum()), int((~lab).sum()), int(ca.sum()), int((ca == 2).sum()), int((ca != 0).sum()),
                     int(co.sum()), int((co == 2).sum()), int((co != 0).sum()))
        assert val[i, col("label")] == (float(t) if t is not None else 0.0), i


@pytest.mark.parametrize("n", SIZES + (4159,))
def test_pivot_rule(n):
    """The float64 rule (the value nearest Sy / n) picks the value the exact rule picks on every trait of the ladder: none of them
    sits on a near-tie, so the bound, which is formed about the exact pivot, is the bound of what the engine computes."""
    _d, y, _val, _bound = case(n)
    c = ref.pivots(y)
    for k in range(y.shape[1]):
        assert c[k] == np.float64(y[ex.pivot(ex.scaled(y[:, k])[0]), k]), ex.LADDER[k]
    assert c[col("label")] in (0.0, 1.0) and c[col("int")] == np.rint(c[col("int")]) and c[col("0.1f")] == np.float64(np.float32(0.1))


@pytest.mark.parametrize("n", SIZES + (4159,))
def test_uncentred_formula_is_rejected(n):
    """(a) The check has teeth: the formula over the raw sums fails it where the trait's mean is far from zero."""
    d, y, val, bound = case(n)
    ac, hom = counts(d)
    unc = ref.chi2_uncentred(n, ac, hom, d, y)
    err = np.abs(unc - val)
    rel = err / np.maximum(val, 1.0)
    print(f"n = {n}: the raw-sum formula's error relative to max(chi2, 1): " + ", ".join(f"{name} {rel[:, k].max():.1e}" for k, name in enumerate(ex.LADDER)))
    assert rel[:, col("normal")].max() < 1e-12, "a zero-mean trait is no trouble for either formula"
    if n >= 300:
        k = col("1e6+-1")
        assert rel[:, k].max() > 1e-4 and (err[:, k] > bound[:, k] + U * val[:, k]).any()
    if n >= 2504:   # rounding leaves the raw vy negative or 0: every cell 0.0 where the exact statistic reaches well above 1
        k = col("near_constant")
        assert not unc[:, k].any() and val[:, k].max() > 1.0


@pytest.mark.parametrize("n", SIZES + (4159,))
def test_centred_formula_within_the_bound(n):
    """(b) The engine's order of operations about the pivot, and the bound itself under the cap on every case."""
    d, y, val, bound = case(n)
    ac, hom = counts(d)
    got = ref.chi2_centred(n, ac, hom, d, y)
    err = np.abs(got - val)
    print(f"n = {n}: |centred - exact| / (n 2^-53 max(chi2, 1)) at most {(err / (n * U * np.maximum(val, 1.0))).max():.3f}, "
          f"bound / cap at most {(bound / ex.cap(n, val)).max():.3f}")
    assert np.all(np.isfinite(bound)) and np.all(bound <= ex.cap(n, val))
    assert np.all(err <= bound + U * val), [(ex.LADDER[k], i) for i, k in np.argwhere(err > bound + U * val)]
    assert not got[:, col("0.1f")].any() and not got[[0, 3]].any()


@pytest.mark.parametrize("n", SIZES)
def test_assoc_matrix_reference_within_four_roundings(n):
    """(c) assoc_matrix_ref's CHI2 from exact integers; the ladder's values survive its quantiser as they are."""
    d, y, val, _bound = case(n)
    q, f = assoc_matrix_ref.quantise(y)
    assert np.array_equal(np.ldexp(q.astype(np.float64), -f[None, :]).astype(np.float32), y)
    ac, hom = counts(d)
    got = assoc_matrix_ref.chi2_table(n, ac, hom, assoc_matrix_ref.dot(d, q), q)
    assert np.all(np.abs(got - val) <= 8 * U * val)
    assert got[1].any() and not got[:, col("0.1f")].any()


def test_bound_without_the_grid():
    """A trait whose values span 40 binary places leaves the grid's exact range: the bound falls back on m - 1 rounded additions
    in any order, the sequential sum stays within it, and it says so by passing the cap (such a trait is no case of the ladder)."""
    n = 2504
    d = case(n)[0]
    rng = np.random.default_rng(5)
    y = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, size=n))).astype(np.float32).reshape(-1, 1)
    val, bound = ex.table(d, y)
    ac, hom = counts(d)
    got = ref.chi2_centred(n, ac, hom, d, y)
    assert np.all(np.abs(got - val) <= bound + U * val) and np.all(np.isfinite(bound))
    assert (bound > ex.cap(n, val)).any()
