"""LD pruning and clumping where the exact comparison cov^2 2^20 > T v_i v_j leaves 64 bits, and the three other gaps of the same
kernels (prune_hit and k_prune_scan in k_prune.hip.h, k_clump_class / k_clump_blockers, ld_moments / ld_r2 and k_ld_block_scan):

  1. random verdicts at width   the LD-block cohort with 8,192 samples (and a subset of 4,099 ids: a pitch tail of the k loop) against
                                vcf_truth.TextOracle -- the VCF text alone -- through the pruning and the clumping file's oracle
                                checkers: every side of every comparison needs more than 64 bits
  2. exact ties at width        ld_prune_ref.write_tie_cohort with 32,760 samples: pairs with cov^2 2^20 == T v_i v_j exactly, at T - 1,
                                T and T + 1 (`>` against `>=`, a float detour), one of them with cov < 0 and r^2 = 1; again over the
                                16,392 columns of a subset (n is the subset's); the band's and the block's r^2 of the same pairs
  3. 32-bit intermediates       a synthetic cohort of 98,304 samples: Sx Sy and n Sxx of 2^32 and more, against the reference over
                                the engine's own genotype matrix in Python integers
  4. the scans' carry           batches of 4,097 and 2 x 4,096 + 5 short regions: keep_begin and block_begin behind the first 4,096
                                regions, which k_prune_scan and k_ld_block_scan write with a carried total

The comparisons are the other LD files' own (test_gpu_ld_prune._check_oracle / _check_full / _same, the clumping file's, the band's
_check_full and _r2_close, test_gpu_ld_matrix._check_result, ld_matrix_ref.blocks): every verdict byte for byte, no tolerance
anywhere.  tests/test_ld_exact_wide_host.py shows on the CPU that the inputs of 1 and 2 can tell a 64-bit kernel from the exact one."""
import time

import numpy as np
import pytest

import test_gpu_ld_band as tb
import test_gpu_ld_clump as tc
import test_gpu_ld_matrix as tm
import test_gpu_ld_prune as tp
import vcf_truth as vt
from ld_band_ref import dosage, dot_band, r2_band
from ld_clump_ref import INDEX, MEMBER, clump_states, key_of, keys_of, pvalue_families
from ld_matrix_ref import block_begin, blocks
from ld_prune_ref import (KEPT, ONE, PRUNED, TIE_REF_LEN, hit_band, hit_band_wrapped64, prune_states, side_band, tie_threshold,
                          write_ld_block_cohort, write_tie_cohort)
from test_ld_exact_wide_host import (TIE_SAMPLES, TIE_SEED, TIE_SUBSET, TWO64, WIDE_SAMPLES, WIDE_SEED, WIDE_SITES, WIDE_SUBSET,
                                     WIDE_THRESHOLDS, WIDE_WINDOWS, tie_subset_columns)
from test_ld_prune_host import _cells
from variantstore_amd import VariantStore, quantise_r2

pytestmark = pytest.mark.gpu
COUNT_FIELDS = ("carriers", "alt_alleles", "hom_alt", "phased")


# ------------------------------------------------------------------------ 1. random verdicts at width: 8,192 samples, VCF text
class _Wide:
    """The wide LD-block cohort, written and opened once; the expected rows of the batch from the VCF text alone."""

    def __init__(self, tmp):
        fasta, vcf, self.names, last = write_ld_block_cohort(str(tmp), WIDE_SEED, n_sites=WIDE_SITES, n_samples=WIDE_SAMPLES, p_two_alt=0)
        self.vs = VariantStore.from_vcf(fasta, vcf, device=0)
        assert self.vs.info().num_samples - 1 == WIDE_SAMPLES and self.names == sorted(self.names)
        tx = vt.TextOracle(vcf)   # asserts that every record is isolated and predicted
        n_rows = len(tx.rows)
        # region ends: the midpoints of the gaps wide enough to lie TextOracle.MARGIN bases from both neighbours
        mid = vt.gap_midpoints(tx.recs, last + 49)
        mid[0] = 1
        clear = [k for k, p in enumerate(mid) if all(p <= lo - tx.MARGIN or p >= hi + tx.MARGIN for lo, hi in tx.spans)]
        assert clear[0] == 0 and clear[-1] == n_rows and len(clear) > 20
        rng = np.random.default_rng(8)
        subs = []
        for width in (1, 2, 3, 5, 8, 12):   # a dozen sub-regions of one row to some dozens, overlapping
            for _ in range(2):
                i = int(rng.integers(0, len(clear) - width))
                subs.append((mid[clear[i]], mid[clear[i + width]]))
        self.whole = (1, last + 50)
        self.regions = [subs[i] for i in rng.permutation(len(subs))]
        self.regions.insert(5, self.whole)   # unsorted, the whole reference in the middle
        self.parsed, self.valid = tp._parse(tx, self.regions)
        assert self.valid.tolist() == list(range(len(self.regions))) and int(self.parsed.row_count[5]) == n_rows
        assert int(self.parsed.row_count.min()) >= 1 and int(np.sort(self.parsed.row_count)[-2]) > 16
        self.subset = sorted(int(i) for i in np.random.default_rng(9).choice(np.arange(1, WIDE_SAMPLES + 1), size=WIDE_SUBSET, replace=False))
        self.table_rows = tc._table_rows(self.vs, self.regions)
        assert self.table_rows == n_rows
        self.cache = {}


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    w = _Wide(tmp_path_factory.mktemp("wide"))
    yield w
    w.vs.close()


def _beyond_64_bits(cells, window, T):
    """(pairs inside the window, those with a side of the comparison at 2^64 or above, those a 64-bit kernel would get wrong)."""
    a = cells.shape[0]
    inside = np.arange(a)[:, None] + 1 + np.arange(window)[None, :] < a
    lhs, rhs = side_band(cells, window, T)
    beyond = np.asarray([[max(int(x), int(y)) >= TWO64 for x, y in zip(lr, rr)] for lr, rr in zip(lhs, rhs)], bool)
    return int(inside.sum()), int((beyond & inside).sum()), int((hit_band(cells, window, T) != hit_band_wrapped64(cells, window, T)).sum())


@pytest.mark.parametrize("columns", ["whole", "subset"])
def test_wide_cohort_prune_against_the_vcf_text(wide, columns):
    """Windows 16 and 64 at T = quantise_r2(0.2) and quantise_r2(0.9).  4,099 columns are no multiple of 16: the k loop has a pitch
    tail, and the hits' sides still need more than 64 bits."""
    w = wide
    sub = None if columns == "whole" else w.subset
    for T in WIDE_THRESHOLDS:
        for window in WIDE_WINDOWS:
            got, cells, band = tp._check_oracle(w.vs, w.regions, w.parsed, w.valid, sub, window, T, text_every=4)
            assert cells.shape == (w.table_rows, WIDE_SAMPLES if sub is None else WIDE_SUBSET)
            q = w.regions.index(w.whole)
            want = prune_states(cells, np.zeros(w.table_rows, bool), got["rows"]["pos"], [0], [w.table_rows], window, T, band=band)[0]
            assert (want == KEPT).sum() >= 10 and (want == PRUNED).sum() >= 10, (T, window)   # from the reference
            assert np.array_equal(got["state"][int(got["keep_begin"][q]):int(got["keep_begin"][q + 1])], want)
        pairs, beyond, differs = _beyond_64_bits(cells, WIDE_WINDOWS[0], T)
        print(f"{columns}, T = {T}: {pairs} pairs inside window {WIDE_WINDOWS[0]}, {beyond} beyond 2^64, {differs} verdicts a 64-bit kernel misses")
        if sub is None:
            assert beyond == pairs and differs >= 50
        else:   # (a near-copy's cov^2 2^20 is about 2^20 v^2 with v of the order 0.4 n^2 = 2^22.7: most hits are beyond, not all pairs)
            assert beyond >= 50 and differs >= 50


@pytest.mark.parametrize("columns", ["whole", "subset"])
def test_wide_cohort_clump_against_the_vcf_text(wide, columns):
    """Window 64 at the same two thresholds, two p-value families."""
    w = wide
    sub = None if columns == "whole" else w.subset
    families = pvalue_families(w.table_rows, 77)
    for T in WIDE_THRESHOLDS:
        for name, p, p1, p2 in families[:2]:
            got, _cells_, _band, _want = tc._check_oracle(w.vs, w.regions, w.parsed, w.valid, sub, p, 64, T, p1, p2, text_every=4, cache=w.cache)
            assert (got["state"] == INDEX).any() and (got["state"] == MEMBER).any(), (T, name)


# -------------------------------------------------------------------------------------- 2. exact ties at width: 32,760 samples
class _Tie:
    def __init__(self, tmp):
        fasta, vcf, self.names, self.pos, self.fractions, self.d, source = write_tie_cohort(str(tmp), TIE_SAMPLES, TIE_SEED)
        self.vs = VariantStore.from_vcf(fasta, vcf, device=0)
        assert self.vs.info().num_samples - 1 == TIE_SAMPLES
        assert self.vs.sample_name(1) == self.names[0] and self.vs.sample_name(TIE_SAMPLES) == self.names[-1]   # column c is id c + 1
        self.t = [tie_threshold(f) for f in self.fractions]
        pos = self.pos
        # one region per pair, its ends on the midpoints of the gaps; the whole reference; an empty region
        self.regions = [(int(pos[2 * k]) - 50, int(pos[2 * k + 1]) + 50) for k in range(len(self.t))] + [(1, TIE_REF_LEN + 1), (1, 40)]
        self.row_count = [2] * len(self.t) + [22, 0]
        res = self.vs.allele_counts(self.regions)   # (where an empty region "begins" is the engine's business: taken from the table)
        self.row_begin = res.allele_counts()["row_begin"].tolist()
        res.close()
        assert self.row_begin[:12] == [2 * k for k in range(len(self.t))] + [0]
        cols = tie_subset_columns(source)
        self.column_sets = {"whole": (None, self.d), "subset": ((cols + 1).tolist(), np.ascontiguousarray(self.d[:, cols]))}
        self.thresholds = sorted({t + dt for t in self.t for dt in (-1, 0, 1) if 0 <= t + dt <= ONE})
        assert ONE in self.thresholds and ONE - 1 in self.thresholds and len(self.thresholds) == 29


@pytest.fixture(scope="module")
def tie(tmp_path_factory):
    t = _Tie(tmp_path_factory.mktemp("tie"))
    yield t
    t.vs.close()


@pytest.mark.parametrize("columns", ["whole", "subset"])
def test_tie_cohort_matrix_is_the_written_one(tie, columns):
    samples, d = tie.column_sets[columns]
    m, cells, dropped = tp._matrix_of(tie.vs, tie.regions, samples)
    assert cells.shape == d.shape and not dropped.any() and np.array_equal(dosage(cells).astype(np.uint8), d)
    assert m["row_begin"].tolist() == tie.row_begin and m["row_count"].tolist() == tie.row_count
    assert np.array_equal(m["rows"]["pos"].astype(np.int64), tie.pos)
    assert m["columns"].tolist() == (list(range(1, TIE_SAMPLES + 1)) if samples is None else samples)
    assert d.shape[1] == (TIE_SAMPLES if samples is None else TIE_SUBSET)


@pytest.mark.parametrize("columns", ["whole", "subset"])
def test_ties_prune(tie, columns):
    """Window 1: the second row of a pair's region is PRUNED exactly when T is below the pair's tie threshold -- at T = t the two
    sides are EQUAL and the strict comparison keeps it.  The subset's n is the subset's: the ties hold there as well."""
    samples, d = tie.column_sets[columns]
    cells, none = _cells(d), np.zeros(22, bool)
    for T in tie.thresholds:
        res = tie.vs.ld_prune(tie.regions, samples, window=1, r2=T / ONE)
        got = res.ld_prune()
        res.close()
        assert got["threshold_q20"] == T and got["row_begin"].tolist() == tie.row_begin and got["row_count"].tolist() == tie.row_count
        tp._same(got, prune_states(cells, none, tie.pos, tie.row_begin, tie.row_count, 1, T), (columns, T))
        for k, t in enumerate(tie.t):   # the per-pair expectation, stated outright
            o = int(got["keep_begin"][k])
            assert got["state"][o:o + 2].tolist() == [KEPT, KEPT if T >= t else PRUNED], (columns, T, k, tie.fractions[k])
            assert int(got["n_kept"][k]) == (2 if T >= t else 1)


@pytest.mark.parametrize("columns", ["whole", "subset"])
def test_ties_clump(tie, columns):
    """The second row of every pair has the smaller p-value: it is the INDEX of its region, and the first row is its MEMBER exactly
    when the pair is a hit, an INDEX of its own otherwise."""
    samples, d = tie.column_sets[columns]
    cells, none = _cells(d), np.zeros(22, bool)
    p = np.empty(22)
    p[0::2], p[1::2] = 1e-3 * (1 + np.arange(11)), 1e-6 * (1 + np.arange(11))
    keys = keys_of(p)
    for T in tie.thresholds:
        res = tie.vs.ld_clump(tie.regions, p, samples, window=1, r2=T / ONE, max_bp=0, p1=0.5, p2=0.5)
        got = res.ld_clump()
        res.close()
        assert got["threshold_q20"] == T and got["row_begin"].tolist() == tie.row_begin and got["row_count"].tolist() == tie.row_count
        tc._same(got, clump_states(cells, none, tie.pos, tie.row_begin, tie.row_count, keys, 1, T, key_of(0.5), key_of(0.5)), (columns, T))
        for k, t in enumerate(tie.t):
            o = int(got["keep_begin"][k])
            hit = T < t
            assert got["state"][o:o + 2].tolist() == [MEMBER if hit else INDEX, INDEX], (columns, T, k, tie.fractions[k])
            assert got["owner"][o:o + 2].tolist() == [1 if hit else 0, 1] and int(got["n_index"][k]) == (1 if hit else 2)


@pytest.mark.parametrize("columns", ["whole", "subset"])
def test_ties_band_and_matrix(tie, columns):
    """dot exact, r2 within the band tests' bound of r2_values; the diagonal of a block exactly 1.0 and the off-diagonal cell of the
    two r^2 = 1 pairs as well: cov^2 and v_i v_j are the same integer there, so the double quotient is exactly 1."""
    samples, d = tie.column_sets[columns]
    cells = _cells(d)
    m, _engine_cells, _dropped = tp._matrix_of(tie.vs, tie.regions, samples)
    for stat in ("dot", "r2"):
        res = tie.vs.ld_band(tie.regions, samples, window=1, stat=stat)
        band = res.ld_band()["band"]
        res.close()
        if stat == "dot":
            assert band.dtype == np.int32 and np.array_equal(band, dot_band(cells, 1))
        else:
            tb._r2_close(band, *r2_band(cells, 1), (columns, "band"))
            assert band[18, 0] == np.float32(1) and band[20, 0] == np.float32(1)
        res = tie.vs.ld_matrix(tie.regions, samples, stat=stat)
        got = res.ld_matrix()
        tm._check_result(got, dict(m, cells=cells), stat, (columns, stat))   # (every cell, the symmetry, the diagonal exactly 1.0f)
        if stat == "r2":
            bb = got["block_begin"]
            for k in (9, 10):
                assert tie.fractions[k] == (1, 1) and np.all(got["cells"][int(bb[k]):int(bb[k + 1])] == np.float32(1)), k
            for k in range(9):
                assert float(got["cells"][int(bb[k]) + 1]) == tie.fractions[k][0] / tie.fractions[k][1], k   # (dyadic: exact as well)
        res.close()


# --------------------------------------------------------------------------- 3. 32-bit intermediates: 98,304 synthetic samples
SYNTH_SAMPLES = 98_304
SYNTH_KW = dict(ref_length=60_000, num_variants=300, num_samples=SYNTH_SAMPLES, seed=77, first_pos=100, frac_ins=0.06, frac_del=0.06,
                frac_multi=0.03, max_indel=4, af_exponent=1.0)
SYNTH_THRESHOLDS = (quantise_r2(1.0 / SYNTH_SAMPLES), quantise_r2(0.2))
TWO32 = 1 << 32


class _Synth:
    def __init__(self):
        t0 = time.perf_counter()
        self.vs = VariantStore.synthetic(device=0, **SYNTH_KW)
        self.open_seconds = time.perf_counter() - t0
        print(f"VariantStore.synthetic with {SYNTH_SAMPLES} samples and {SYNTH_KW['num_variants']} variants: {self.open_seconds:.2f} s")
        L = self.vs.info().ref_length
        rng = np.random.default_rng(6)
        starts = rng.integers(1, L - 20_000, size=5)
        self.regions = [(int(s), int(s) + int(rng.integers(2_000, 20_000))) for s in starts] + [(1, L), (L - 9_000, L + 5)]   # unsorted
        self.matrix_of = tp._matrix_of(self.vs, self.regions)
        self.a = self.matrix_of[1].shape[0]
        assert self.matrix_of[1].shape[1] == SYNTH_SAMPLES and self.a > 2 * 64 + 16   # more than two workgroups of the band plus halo


@pytest.fixture(scope="module")
def synth():
    s = _Synth()
    yield s
    s.vs.close()


def test_synthetic_width_reaches_32_bit_products(synth):
    """From the allele_counts record: rows with n Sxx >= 2^32 and pairs inside a window of 16 rows with Sx Sy >= 2^32; and the count
    records of the pruning and the clumping result are that query's."""
    res = synth.vs.allele_counts(synth.regions)
    ac = res.allele_counts()
    res.close()
    sx = ac["counts"]["alt_alleles"].astype(np.int64)
    sxx = sx + 2 * ac["counts"]["hom_alt"].astype(np.int64)
    assert sx.shape[0] == synth.a
    rows = int((SYNTH_SAMPLES * sxx >= TWO32).sum())
    pairs = sum(int((sx[:-k] * sx[k:] >= TWO32).sum()) for k in range(1, 17))
    print(f"{synth.a} rows, {rows} with n Sxx >= 2^32, {pairs} pairs inside window 16 with Sx Sy >= 2^32")
    assert rows >= 20 and pairs >= 20
    pres = synth.vs.ld_prune(synth.regions, window=16, r2=0.2)
    cres = synth.vs.ld_clump(synth.regions, np.full(synth.a, 0.5), window=16, r2=0.2, max_bp=0, p1=1.0, p2=1.0)
    for got in (pres.ld_prune(), cres.ld_clump()):
        assert np.array_equal(got["rows"]["pos"], ac["rows"]["pos"])
        for f in COUNT_FIELDS:
            assert np.array_equal(got["counts"][f], ac["counts"][f]), f
    pres.close(); cres.close()


@pytest.mark.parametrize("T", SYNTH_THRESHOLDS)
def test_synthetic_width_prune(synth, T):
    m, cells, dropped, out, band = tp._check_full(synth.vs, synth.regions, None, (16, 64), T, "98,304 columns")
    assert np.array_equal(cells, synth.matrix_of[1])
    if T == SYNTH_THRESHOLDS[0]:
        assert all((g["state"] == KEPT).any() and (g["state"] == PRUNED).any() for g in out.values())


@pytest.mark.parametrize("T", SYNTH_THRESHOLDS)
def test_synthetic_width_clump(synth, T):
    families = pvalue_families(synth.a, 41)
    _m, _cells_, _dropped, out, _band = tc._check_full(synth.vs, synth.regions, None, [(16, families[0]), (64, families[1])], T, "98,304 columns",
                                                     matrix_of=synth.matrix_of)
    if T == SYNTH_THRESHOLDS[0]:
        assert all((g["state"] == INDEX).any() and (g["state"] == MEMBER).any() for g in out)


def test_synthetic_width_band(synth):
    m = tb._check_full(synth.vs, synth.regions, None, (16,), "98,304 columns")
    assert m["cells"].shape == (synth.a, SYNTH_SAMPLES)


# ------------------------------------------------------------------------------------- 4. the scans' carry: > 4,096 regions
SCAN_TILE = 4096   # regions one iteration of k_prune_scan / k_ld_block_scan takes


def _short_regions(n, seed, empties=()):
    """n sorted regions of 50 .. 300 bases (about three rows each); those at `empties` are of length 0."""
    rng = np.random.default_rng(seed)
    s = np.sort(rng.integers(1_000, 7_990_000, size=n))
    length = rng.integers(50, 301, size=n)
    length[list(empties)] = 0
    return np.stack([s, s + length], axis=1).astype(np.uint64)


@pytest.fixture(scope="module")
def scan_store():
    vs = VariantStore.synthetic(device=0, **tp.T6_KW)
    n2 = 2 * SCAN_TILE + 5
    empties = (7, SCAN_TILE - 1, SCAN_TILE, 2 * SCAN_TILE, n2 - 1)
    batches = {"4097": (_short_regions(SCAN_TILE + 1, 21), ()), "8197": (_short_regions(n2, 22, empties), empties)}
    yield vs, batches
    vs.close()


def _scan_batch(scan_store, which):
    vs, batches = scan_store
    regions, empties = batches[which]
    return vs, regions, empties, tp._matrix_of(vs, regions)


def _exclusive_scan(row_count):
    out = np.zeros(row_count.shape[0] + 1, np.uint64)
    np.cumsum(np.asarray(row_count, np.uint64), out=out[1:])
    return out


def _carried(begin, want, row_count, empties):
    """The entries behind the first 4,096 regions are nonzero and the reference's; the empty regions are empty."""
    assert begin.shape[0] == row_count.shape[0] + 1 > SCAN_TILE + 1
    assert int(begin[SCAN_TILE]) != 0 and np.array_equal(begin[SCAN_TILE:], want[SCAN_TILE:])
    assert not row_count[list(empties)].any() and int(np.count_nonzero(row_count)) > row_count.shape[0] // 2
    assert 2 <= row_count.mean() <= 5


@pytest.mark.parametrize("which", ["4097", "8197"])
def test_scan_carry_prune(scan_store, which):
    vs, regions, empties, _mo = _scan_batch(scan_store, which)
    T = quantise_r2(1.0 / 300)
    m, cells, dropped, out, band = tp._check_full(vs, regions, None, (8,), T, which)
    got = out[8]
    _carried(got["keep_begin"], _exclusive_scan(m["row_count"]), m["row_count"], empties)
    assert (got["state"] == KEPT).any() and (got["state"] == PRUNED).any()


@pytest.mark.parametrize("which", ["4097", "8197"])
def test_scan_carry_clump(scan_store, which):
    vs, regions, empties, mo = _scan_batch(scan_store, which)
    T = quantise_r2(1.0 / 300)
    families = pvalue_families(mo[1].shape[0], 5)
    m, cells, dropped, out, band = tc._check_full(vs, regions, None, [(8, families[0]), (8, families[1])], T, which, matrix_of=mo)
    for got in out:
        _carried(got["keep_begin"], _exclusive_scan(m["row_count"]), m["row_count"], empties)
        assert (got["state"] == INDEX).any() and (got["state"] == MEMBER).any()


@pytest.mark.parametrize("which", ["4097", "8197"])
def test_scan_carry_ld_matrix(scan_store, which):
    vs, regions, empties, (m, cells, _dropped) = _scan_batch(scan_store, which)
    res = vs.ld_matrix(regions, stat="dot")
    got = res.ld_matrix()
    assert np.array_equal(got["row_begin"], m["row_begin"]) and np.array_equal(got["row_count"], m["row_count"])
    flat, bb = blocks(cells, m["row_begin"], m["row_count"], "dot")
    assert np.array_equal(bb, block_begin(m["row_count"]))
    assert got["block_begin"].dtype == np.uint64 and np.array_equal(got["block_begin"], bb)
    _carried(got["block_begin"], bb, m["row_count"], empties)
    assert got["cells"].dtype == np.int32 and np.array_equal(got["cells"], flat) and flat.any()
    res.close()
