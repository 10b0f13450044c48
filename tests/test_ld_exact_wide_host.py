"""The inputs of tests/test_gpu_ld_exact_wide.py are not vacuous -- checked from the writers' output alone, on the CPU, with the
reference's Python integers: no GPU, no constructor, no engine.

  the tie cohort           every pair of ld_prune_ref.TIE_PAIRS satisfies cov^2 2^20 == T v_i v_j exactly at n = 32,760 and over the
                           16,392 columns of the subset, is a hit at T - 1 and none at T and T + 1; at n = 32,760 both sides need
                           more than 64 bits; and a kernel that multiplied in 64-bit integers (hit_band_wrapped64) would get some
                           of the T - 1 verdicts wrong
  the wide LD-block cohort 8,192 samples: every pair inside a window of 16 rows has a side of 2^64 or more at T =
                           quantise_r2(0.2), and the wrapped comparison differs from the exact one on many of them

hit_band_wrapped64 is never an expected value here or anywhere: it only says that the input can tell the two kernels apart.

The numbers these seeds give (printed by the tests, asserted with room):
  tie cohort, n = 32,760   sides of 72 .. 78 bits; wrapped != exact at T - 1 for 5 of the 11 pairs (r^2 = 1/16, 1/8, 3/16, 3/8, 5/8
                           and 3/4 wrap to a hit all the same; 1/4, 1/2, 9/16 and the two r^2 = 1 pairs do not)
  tie cohort, 16,392       sides of 68 .. 75 bits; wrapped != exact at T - 1 for 4 of the 11 pairs (1/8, 3/16, 3/8, 9/16)
  LD-block cohort, seed 31 97 rows, 1,416 pairs inside the window, 1,416 of them beyond 2^64, 203 differing verdicts"""
import numpy as np
import pytest

import vcf_truth as vt
from genotype_matrix_ref import Parsed, matrix
from ld_prune_ref import (KEPT, ONE, PRUNED, TIE_PAIRS, hit_band, hit_band_wrapped64, prune_states, side_band, tie_threshold,
                          write_ld_block_cohort, write_tie_cohort)
from test_ld_prune_host import _cells
from variantstore_amd import quantise_r2

# what the GPU file runs: the widths, the seeds, the thresholds and the windows
TIE_SAMPLES, TIE_SUBSET, TIE_SEED = 32_760, 16_392, 5
WIDE_SAMPLES, WIDE_SITES, WIDE_SEED, WIDE_SUBSET = 8_192, 96, 31, 4_099
WIDE_THRESHOLDS = (quantise_r2(0.2), quantise_r2(0.9))
WIDE_WINDOWS = (16, 64)
TWO64 = 1 << 64


@pytest.fixture(scope="module")
def tie(tmp_path_factory):
    return write_tie_cohort(str(tmp_path_factory.mktemp("tie")), TIE_SAMPLES, TIE_SEED)


def tie_subset_columns(source):
    """The columns that came from the first TIE_SUBSET positions in front of the permutation: whole patterns again."""
    return np.nonzero(np.asarray(source) < TIE_SUBSET)[0]


def _pair_sides(d, k, T):
    lhs, rhs = side_band(_cells(d[2 * k:2 * k + 2]), 1, T)
    return int(lhs[0, 0]), int(rhs[0, 0])


def _pair_hit(d, k, T, band=hit_band):
    return bool(band(_cells(d[2 * k:2 * k + 2]), 1, T)[0, 0])


def test_tie_cohort_is_what_its_writer_says(tie):
    _fasta, vcf, names, pos, fractions, d, source = tie
    assert d.shape == (22, TIE_SAMPLES) and d.dtype == np.uint8 and int(d.max()) == 2 and len(fractions) == len(TIE_PAIRS) == 11
    assert names == sorted(names) and sorted(source.tolist()) == list(range(TIE_SAMPLES)) and source.tolist() != list(range(TIE_SAMPLES))
    assert np.all(np.diff(pos) == 100)
    for k, (_f, x, y) in enumerate(TIE_PAIRS):   # every row is its pattern, repeated, behind the one permutation
        for row, pat in ((2 * k, x), (2 * k + 1, y)):
            back = np.empty(TIE_SAMPLES, np.uint8)
            back[source] = d[row]
            assert np.array_equal(back, np.tile(np.asarray(pat, np.uint8), TIE_SAMPLES // len(pat))), (k, row)
    # the VCF holds that matrix: single-ALT SNPs, 0|0 / 0|1 or 1|0 / 1|1, both spellings of dosage 1 in use
    got_names, recs = vt.read_vcf(vcf)
    assert got_names == names and [r[0] for r in recs] == pos.tolist()
    lut = {"0|0": 0, "0|1": 1, "1|0": 1, "1|1": 2}
    seen = set()
    for i, (_p, ref, alts, gts) in enumerate(recs):
        assert len(ref) == 1 and len(alts) == 1 and len(alts[0]) == 1 and alts[0] != ref
        assert np.array_equal(np.asarray([lut[g] for g in gts], np.uint8), d[i]), i
        seen |= set(gts)
    assert seen == set(lut)
    sub = tie_subset_columns(source)
    assert sub.shape == (TIE_SUBSET,) and TIE_SUBSET % 12 == 0 and TIE_SAMPLES % 12 == 0


@pytest.mark.parametrize("width", [TIE_SAMPLES, TIE_SUBSET])
def test_tie_identity_and_its_neighbours(tie, width):
    _fasta, _vcf, _names, _pos, fractions, d, source = tie
    if width != TIE_SAMPLES:
        d = d[:, tie_subset_columns(source)]
    assert d.shape[1] == width
    bits, wrapped_differs = [], []
    for k, f in enumerate(fractions):
        t = tie_threshold(f)
        assert 0 < t <= ONE
        lhs, rhs = _pair_sides(d, k, t)
        assert lhs == rhs and lhs > 0, (k, f, lhs, rhs)   # the tie, in Python integers
        assert _pair_hit(d, k, t - 1) and not _pair_hit(d, k, t) and (t == ONE or not _pair_hit(d, k, t + 1)), (k, f)
        bits.append(lhs.bit_length())
        if width == TIE_SAMPLES:
            assert lhs >= TWO64 and _pair_sides(d, k, t - 1)[1] >= TWO64, (k, f, lhs.bit_length())
        if _pair_hit(d, k, t - 1, hit_band_wrapped64) != _pair_hit(d, k, t - 1):
            wrapped_differs.append(f)
    print(f"n = {width}: sides of {min(bits)} .. {max(bits)} bits; wrapped != exact at T - 1 for {len(wrapped_differs)} pairs: {wrapped_differs}")
    assert len(wrapped_differs) >= 3
    # cov < 0 and r^2 = 1: pair 9, the case the kernel's negation of cov is there for
    x, y = d[18].astype(np.int64), d[19].astype(np.int64)
    assert fractions[9] == (1, 1) and width * int((x * y).sum()) - int(x.sum()) * int(y.sum()) < 0
    x, y = d[20].astype(np.int64), d[21].astype(np.int64)
    assert fractions[10] == (1, 1) and width * int((x * y).sum()) - int(x.sum()) * int(y.sum()) > 0


def test_wide_block_cohort_leaves_64_bits(tmp_path):
    fasta, vcf, names, last = write_ld_block_cohort(str(tmp_path), WIDE_SEED, n_sites=WIDE_SITES, n_samples=WIDE_SAMPLES, p_two_alt=0)
    assert len(names) == WIDE_SAMPLES and names == sorted(names)   # columns in name order: the text says what a row holds
    tx = vt.TextOracle(vcf)   # every record is isolated and predicted from the text: p_two_alt = 0
    n, _early, text = tx.get_var_in_ref(1, last + 50)
    assert WIDE_SITES <= n == len(tx.rows) <= WIDE_SITES + 8 and "/" in text and "|" in text
    m = matrix(Parsed([text]), sorted(names))
    a = m.shape[0]
    window, T = WIDE_WINDOWS[0], WIDE_THRESHOLDS[0]
    inside = np.arange(a)[:, None] + 1 + np.arange(window)[None, :] < a
    lhs, rhs = side_band(m, window, T)
    beyond = np.asarray([[max(int(x), int(y)) >= TWO64 for x, y in zip(lr, rr)] for lr, rr in zip(lhs, rhs)], bool)
    differs = hit_band(m, window, T) != hit_band_wrapped64(m, window, T)
    print(f"{a} rows, {int(inside.sum())} pairs inside the window, {int((beyond & inside).sum())} beyond 2^64, {int(differs.sum())} differing verdicts")
    assert np.all(beyond[inside]) and not differs[~inside].any() and int(differs.sum()) >= 50
    # every threshold and window of the GPU test keeps some rows and prunes some
    none = np.zeros(a, bool)
    for T in WIDE_THRESHOLDS:
        for window in WIDE_WINDOWS:
            state, _kb, _nk = prune_states(m, none, np.arange(a), [0], [a], window, T)
            assert (state == KEPT).sum() >= 10 and (state == PRUNED).sum() >= 10, (T, window)


def test_write_ld_block_cohort_default_bytes_are_unchanged(tmp_path):
    """p_two_alt is a threshold on a draw that is made anyway: naming the default changes nothing, 0 leaves no two-ALT record, and
    up to the first two-ALT record the two cohorts are the same positions, bases and calls."""
    fasta, vcf, names, last = write_ld_block_cohort(str(tmp_path), 31)
    again = write_ld_block_cohort(str(tmp_path), 31, p_two_alt=0.06)
    assert again[3] == last and len(names) == 40
    _n, recs = vt.read_vcf(vcf)
    assert any(len(r[2]) == 2 for r in recs) and 300 <= len(recs) <= 308
    sub = tmp_path / "zero"
    sub.mkdir()
    _n, recs0 = vt.read_vcf(write_ld_block_cohort(str(sub), 31, p_two_alt=0)[1])
    assert all(len(r[2]) == 1 for r in recs0)
    first_two = next(i for i, r in enumerate(recs) if len(r[2]) == 2)
    assert [r[:2] + (r[3],) for r in recs0[:first_two]] == [r[:2] + (r[3],) for r in recs[:first_two]]   # the same bytes up to there
