"""Pairwise IBS queries on the GPU (vs_query_sample_ibs): every cell of the three indicator products, of ibs0 / ibs1 / ibs2 and of
the KING kinship against the engine's own genotype matrix (every subtile, quadrant, tile and tile-pair edge -- 16, 64 and 128 columns,
the kernel's own widths --, every pitch residue, the default row chunk and several chunks plus a remainder), small and empty tables,
column subsets, the storage forms of the genotype bits, saturated cohorts against the VCF text, the oracle's type-6 text, tables
with rows the duplicate rule dropped, determinism, interleaving with type-6 batches, the temporary matrix, the size limit, the
refused accessors, the device pointers and the CLI.

Every integer is compared bit for bit.  king is compared bit for bit too: both sides convert two exact integers below 2^53 to
float64 and divide once."""
import os
import subprocess

import numpy as np
import pytest

from genotype_matrix_ref import Parsed, matrix
from helpers import oracle_texts, random_regions, write_random_cohort
from ld_band_ref import dosage
from oracle.oracle import Oracle
from sample_ibs_ref import ibs_text, king, sample_ibs
from test_gpu_genotype_matrix import _columns, _oracle, _read_device as _read_device_bytes, _ref_len
from test_gpu_saturated_columns import _Cohort, _table_matrix
from variantstore_amd import VariantStore
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_ARG, VS_ERR_UNSUPPORTED = -5, -7
INT_FIELDS = ("het_het", "hom_hom", "carrier_both", "ibs0", "ibs1", "ibs2")


def _compare(got, want, stat, what=None):
    """A result's arrays against the reference's dict: every integer, the invariants, and under "king" every kinship bit."""
    n = want["het_het"].shape[0]
    assert got["stat"] == stat and got["n_used"] == want["n_used"], (what, got["n_used"], want["n_used"])
    for f in INT_FIELDS:
        assert got[f].shape == (n, n) and got[f].dtype == np.int64, f
        bad = np.argwhere(got[f] != want[f])
        assert bad.shape[0] == 0, (what, stat, f, n, bad[:8].tolist())
        assert np.array_equal(got[f], got[f].T), f
    assert np.array_equal(got["ibs0"] + got["ibs1"] + got["ibs2"], np.full((n, n), got["n_used"], np.int64))
    assert np.array_equal(got["het"], np.diagonal(want["het_het"])) and got["het"].dtype == np.int64
    if stat == "king":
        wk = king(want["het_het"], want["ibs0"])
        assert got["king"].dtype == np.float64 and got["king"].shape == (n, n)
        assert got["king"].tobytes() == wk.tobytes(), (what, float(np.abs(got["king"] - wk).max()))
        assert np.array_equal(got["king"], got["king"].T)
        assert (np.diagonal(got["king"])[got["het"] > 0] == 0.5).all() and not np.diagonal(got["king"])[got["het"] == 0].any()
        den0 = (got["het"][:, None] + got["het"][None, :]) == 0
        assert not got["king"][den0].any() and not np.signbit(got["king"][den0]).any(), "0.0, not -0.0, where the denominator is 0"
    else:
        assert got["king"] is None


def _check_full(vs, regions, samples, stats=("counts",), what=None, ordered=True):
    """Every matrix of every stat against sample_ibs_ref over genotype_matrix() of the same regions and samples (the dropped rows
    from the table's count_flags).  `ordered`: the table's rows come in the same order in both calls (not so for the private rows
    of regions under the duplicate rule; the sums do not depend on the order).  Returns the matrix's arrays, the expected dict and
    the last result's arrays."""
    mres = vs.genotype_matrix(regions, samples)
    m = mres.genotype_matrix()
    mres.close()
    cells = np.ascontiguousarray(m["cells"])
    a, n = cells.shape
    dropped = (m["rows"]["count_flags"] >> 31) != 0
    want = sample_ibs(cells, dropped)
    same = np.array_equal if ordered else (lambda x, y: np.array_equal(np.sort(x), np.sort(y)))
    got = None
    for stat in stats:
        res = vs.sample_ibs(regions, samples, stat=stat)
        got = res.sample_ibs()
        assert got["columns"].dtype == np.uint32 and got["columns"].tolist() == m["columns"].tolist()
        assert got["counts"].shape == (a,) and same(got["rows"]["pos"], m["rows"]["pos"])
        assert same(got["rows"]["count_flags"], m["rows"]["count_flags"])
        assert (not ordered or np.array_equal(got["row_begin"], m["row_begin"])) and np.array_equal(got["row_count"], m["row_count"])
        _compare(got, want, stat, what)
        assert same(got["counts"]["alt_alleles"].astype(np.int64), dosage(cells).sum(axis=1))
        assert res.totals()[2] == int(np.count_nonzero(cells))
        res.close()
    return m, want, got


def _distinct(want):
    """The preconditions that keep a swapped product or a wrong lane map from hiding: hom_hom, het_het and ibs0 each non-zero
    somewhere off the diagonal, the three primitives pairwise different."""
    n = want["het_het"].shape[0]
    off = ~np.eye(n, dtype=bool)
    for f in ("hom_hom", "het_het", "ibs0"):
        assert want[f][off].any(), f
    hh, aa, cc = want["het_het"], want["hom_hom"], want["carrier_both"]
    assert not np.array_equal(hh, aa) and not np.array_equal(hh, cc) and not np.array_equal(aa, cc)


def _pitch_cohort(n_cols):   # (num_samples counts the samples of the cohort; info().num_samples adds "ref")
    return VariantStore.synthetic(device=0, ref_length=60_000, num_variants=1500, num_samples=n_cols, seed=900 + n_cols, first_pos=100,
                                  frac_ins=0.06, frac_del=0.06, frac_multi=0.03, max_indel=4, af_exponent=1.0)


def _pitch_regions(vs, rng):
    L = vs.info().ref_length
    starts = rng.integers(1, L - 4000, size=60)
    return [(int(s), int(s) + int(rng.integers(1, 4000))) for s in starts] + [(1, 3000), (L - 2000, L + 5)]


# ------------------------------------------------------------------- 1. against the engine's own matrix, every cell
@pytest.mark.parametrize("n_cols", [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257])
def test_every_cell_against_the_matrix(n_cols):
    """The subtile (16), quadrant (64), tile (128) and tile-pair edges of k_sample_ibs -- k_sample_gram's widths --, an odd number
    of tiles (257: three), every pitch residue class; the default row chunk and ibs_chunk = 64: several chunks plus a remainder.
    The batch is unsorted: the device sorts it."""
    vs = _pitch_cohort(n_cols)
    rng = np.random.default_rng(n_cols)
    regions = _pitch_regions(vs, rng)
    m, want, _ = _check_full(vs, regions, None, ("counts", "king"), n_cols)
    cells = m["cells"]
    a = cells.shape[0]
    assert cells.shape[1] == n_cols and m["row_pitch"] == (n_cols + 15) // 16 * 16
    assert a > 3 * 64 and a % 64 != 0, "more than three row chunks and a remainder"
    if n_cols > 1:
        _distinct(want)
    if n_cols >= 63:   # rows with distinct carrier sets: a wrong lane map cannot hide behind uniform data
        assert np.unique(cells, axis=0).shape[0] > a // 4, (np.unique(cells, axis=0).shape[0], a)
        assert np.unique(dosage(cells), axis=1).shape[1] > n_cols // 2
    vs.set_option("ibs_chunk", 64)
    _check_full(vs, regions, None, ("counts", "king"), (n_cols, "chunk 64"))
    vs.set_option("ibs_chunk", 0)
    vs.close()


def test_small_tables_and_the_empty_one():
    """Tables of 0, 1, 15, 16, 17, 64 and 65 rows, under the default chunk and chunks of 64 rows."""
    vs = _pitch_cohort(65)
    L = vs.info().ref_length
    probe = vs.allele_counts([(1, L)])
    pos = np.unique(probe.allele_counts()["rows"]["pos"].astype(np.int64))
    probe.close()
    # regions (pos[k], pos[k + m]) for a sweep of k and m: whatever a row's exact extent, some of them report each wanted number of rows
    spans = [(int(pos[k]), int(pos[k + m])) for m in (0, 1, 2, 13, 14, 15, 16, 17, 62, 63, 64, 65, 66) for k in range(0, 60, 3)]
    cres = vs.allele_counts(spans)
    n_rows = cres.allele_counts()["row_count"].astype(np.int64)
    cres.close()
    for chunk in (0, 64):
        vs.set_option("ibs_chunk", chunk)
        for want in (1, 15, 16, 17, 64, 65):
            hit = np.nonzero(n_rows == want)[0]
            assert hit.size, (want, sorted(set(n_rows.tolist())))
            m, _w, _g = _check_full(vs, [spans[int(hit[0])]], None, ("counts", "king"), (want, chunk))
            assert m["cells"].shape[0] == want
        first = int(pos[0])
        assert first > 2
        for stat in ("counts", "king"):   # a table without rows: all-zero n x n matrices and n_used = 0, not an error
            res = vs.sample_ibs([(1, first - 2)], stat=stat)
            got = res.sample_ibs()
            assert got["n_used"] == 0 and all(got[f].shape == (65, 65) and not got[f].any() for f in INT_FIELDS)
            assert got["counts"].shape == (0,) and got["rows"].shape == (0,) and not got["het"].any()
            if stat == "king":
                assert got["king"].shape == (65, 65) and not got["king"].any() and not np.signbit(got["king"]).any()
            assert res.totals()[1:3] == (0, 0)
            assert res.sample_ibs_device()[3:] == (0, 65, stat)
            res.close()
    vs.set_option("ibs_chunk", 0)
    vs.close()


def test_column_subset_with_repeated_ids():
    vs = _pitch_cohort(129)
    rng = np.random.default_rng(8)
    sub = [int(i) for i in rng.choice(np.arange(1, 130), size=37, replace=False)]
    regions = _pitch_regions(vs, rng)
    for batch in (sorted(regions), regions):   # (the device sorts the unsorted one)
        m, want, got = _check_full(vs, batch, sub + sub[:5], ("counts", "king"), "subset")
        assert got["columns"].tolist() == sorted(sub) and m["cells"].shape[1] == 37
        _distinct(want)
    m, _w, got = _check_full(vs, regions, [vs.sample_name(sub[0])], ("counts", "king"), "one name")   # n = 1
    assert got["het_het"].shape == (1, 1) and got["het_het"][0, 0] > 0 and got["ibs2"][0, 0] == got["n_used"] and got["king"][0, 0] == 0.5
    vs.close()


# ------------------------------------------------------------------------------------------------------ 2. the storage forms
@pytest.mark.parametrize("list_max", [0, 3, 64])
def test_listed_and_dense_classes(list_max, monkeypatch):
    monkeypatch.setenv("VS_LIST_MAX", str(list_max))
    vs = VariantStore.synthetic(device=0, ref_length=60_000, num_variants=1500, num_samples=150, seed=650, first_pos=100,
                                frac_ins=0.06, frac_del=0.06, frac_multi=0.03, max_indel=4, af_exponent=2.5)
    assert vs.info().list_max == list_max
    rng = np.random.default_rng(list_max)
    regions = _pitch_regions(vs, rng)
    subset = [int(i) for i in rng.choice(np.arange(1, 150), size=50, replace=False)]
    _check_full(vs, regions, None, ("king",), list_max)
    _check_full(vs, regions, subset, ("counts",), list_max)
    vs.close()


def test_explicit_ids_many_columns():
    """An explicit-id cohort above 4,096 samples: several column tiles of the matrix kernel, 34 tiles and 595 tile pairs here."""
    vs = VariantStore.synthetic(device=0, ref_length=100_000, num_variants=400, num_samples=4_300, seed=9, first_pos=2_000, frac_ins=0.05,
                                frac_del=0.05, frac_multi=0.01, max_indel=6, af_exponent=2.0, max_af=0.002)
    info = vs.info()
    assert not info.use_bit_vector and info.num_samples - 1 > 4_096
    regions = [(1, 40_000), (30_000, 70_000), (60_000, 100_000), (2_500, 2_600)]
    m, _want, got = _check_full(vs, regions, None, ("counts",), "explicit")
    assert m["cells"][:, 4_096:].any(), "no column beyond the matrix kernel's first tile is set"
    assert m["cells"].shape[0] > 200 and got["carrier_both"][4_096:, :128].any()
    vs.close()


# ----------------------------------------------------------------------------- 3. against the VCF text and the oracle
def _check_texts(vs, regions, parsed, samples, stats):
    """Against sample_ibs_ref of the matrix the EXPECTED texts give -- not of the engine's own genotype matrix."""
    _ids, names = _columns(vs, samples)
    want_m = matrix(parsed, names)
    got = want = None
    for stat in stats:
        res = vs.sample_ibs(regions, samples, stat=stat)
        got = res.sample_ibs()
        res.close()
        dropped = (got["rows"]["count_flags"] >> 31) != 0
        want = sample_ibs(_table_matrix(got, parsed, want_m), dropped)
        _compare(got, want, stat, samples if samples is None else len(samples))
    return got, want


@pytest.mark.parametrize("n", [63, 4159])
def test_saturated_cohort_against_the_vcf_text(n, tmp_path):
    """Rows carried by 75 - 100 % of the samples -- everybody 1/1, everybody 0|1, all but one sample --: hom x hom in (nearly) every
    cell of the products.  The expected answer comes from the VCF TEXT alone (vcf_truth.TextOracle)."""
    c = _Cohort(n, None, "text", tmp_path)
    regions, parsed = c.batch["sorted"], c.mparsed("sorted")
    if n <= 64:
        got, want = _check_texts(c.vs, regions, parsed, None, ("counts", "king"))
        _distinct(want)
        a = c.table_rows(got, "sorted", [1, 3])      # everybody 1/1, everybody 0|1
        assert got["hom_hom"].min() >= 2 and got["het_het"].min() >= 2 and got["counts"]["hom_alt"][a].tolist() == [n, 0]
    rng = np.random.default_rng(19 * n)
    sub = sorted(set(c.subset) | {int(i) for i in rng.choice(np.arange(1, n + 1), size=min(260, n // 2), replace=False)})
    _got, want = _check_texts(c.vs, regions, parsed, sub, ("counts", "king"))
    _distinct(want)
    _check_texts(c.vs, c.batch["shuffled"], c.mparsed("shuffled"), c.subset, ("king",))
    c.close()


@pytest.mark.parametrize("stem", ["x", "x.small"])
def test_golden_disjoint_regions_against_the_oracle(stem, golden_dir, tmp_path):
    """Disjoint regions, so that each site is reported once: the counts of the matrix the oracle's type-6 text gives; n_used is the
    number of rows the text lists -- the rows the duplicate rule dropped are no sites."""
    fasta, vcf = os.path.join(golden_dir, stem + ".fa"), os.path.join(golden_dir, stem + ".vcf")
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    plain = os.path.join(tmp_path, "plain.bin")
    vs.export_plain(plain)
    orc = Oracle(plain)
    L = _ref_len(fasta)
    step = max(40, L // 50)
    regions = [(x, min(L, x + step - 12)) for x in range(1, L, step)]   # gaps of 12 bases between them
    want_t = oracle_texts(orc, regions)
    parsed = Parsed([t if n >= 0 else None for n, _e, t in want_t])
    assert parsed.n_rows > 0
    ids = list(range(1, vs.info().num_samples))
    for samples in (None, ids[:1], ids[::2] + ids[:1]):
        cols = ids if samples is None else sorted(set(samples))
        wm = matrix(parsed, [vs.sample_name(i) for i in cols])
        want = sample_ibs(wm)
        for stat in ("counts", "king"):
            res = vs.sample_ibs(regions, samples, stat=stat)
            got = res.sample_ibs()
            res.close()
            dropped = (got["rows"]["count_flags"] >> 31) != 0
            assert int(got["row_count"].sum()) - int(dropped.sum()) == parsed.n_rows == wm.shape[0], "a site is reported twice"
            assert got["n_used"] == parsed.n_rows == got["rows"].shape[0] - int(dropped.sum())
            assert got["columns"].tolist() == cols
            _compare(got, want, stat, (stem, samples))
    vs.close()


@pytest.mark.parametrize("seed", [701, 703])
def test_random_cohorts_with_duplicate_rule(seed, tmp_path):
    """Near and equal records: the duplicate rule drops rows of the table.  They add nothing and are excluded from n_used.  (The
    regions under the rule report private copies of their rows, so the table holds rows no region reports: the expected answer is
    formed over the engine's own matrix, whose every reported row test_gpu_genotype_matrix holds to the oracle on these cohorts.)"""
    fasta, vcf, _names = write_random_cohort(str(tmp_path), seed, ref_len=6000, n_rows=400, n_samples=9, p_near=0.6, p_multi=0.3,
                                             p_same=0.3, unphased_p=0.4 if seed % 2 else 0.05, haploid_p=0.1 if seed == 703 else 0.0)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    rng = np.random.default_rng(seed)
    texts = oracle_texts(_oracle(vs, tmp_path), random_regions(rng, 6000, 300, max_len=900))
    regions = [r for r, (n, _e, _t) in zip(random_regions(np.random.default_rng(seed), 6000, 300, max_len=900), texts) if n >= 0]
    assert len(regions) > 200   # (only the regions the reference's walk terminates on: the rows of the others are not defined)
    for samples in (None, [2, 3, 5, 9]):
        for chunk in (0, 64):
            vs.set_option("ibs_chunk", chunk)
            _m, want, got = _check_full(vs, regions, samples, ("counts", "king"), ("duplicate rule", samples, chunk), ordered=False)
            dropped = (got["rows"]["count_flags"] >> 31) != 0
            assert dropped.any(), "no row of the batch was dropped by the duplicate rule"
            assert got["n_used"] == got["rows"].shape[0] - int(dropped.sum()) < got["rows"].shape[0]
            assert (np.diagonal(got["ibs2"]) == got["n_used"]).all() and not got["counts"]["carriers"][dropped].any()
            _distinct(want)
    vs.set_option("ibs_chunk", 0)
    vs.close()


# ------------------------------------------------------------------------------------------------------ 4. determinism
T6_KW = dict(ref_length=8_000_000, num_variants=150_000, num_samples=300, seed=5, first_pos=1_000, frac_ins=0.05, frac_del=0.05,
             frac_multi=0.02, max_indel=6, af_exponent=2.0)


@pytest.fixture(scope="module")
def t6_store():
    vs = VariantStore.synthetic(device=0, **T6_KW)
    rng = np.random.default_rng(12)
    s = np.sort(rng.integers(1_000, 7_990_000, size=3_000))
    regions = np.stack([s, s + rng.integers(50, 3_000, size=3_000)], axis=1).astype(np.uint64)
    yield vs, regions
    vs.close()


def test_two_calls_give_the_same_bytes(t6_store):
    vs, regions = t6_store
    outs = []
    for _ in range(2):
        r = vs.sample_ibs(regions, stat="king")
        g = r.sample_ibs()
        outs.append(tuple(g[f].tobytes() for f in INT_FIELDS) + (g["king"].tobytes(), g["n_used"]))
        assert r.fill_ms() > 0 and r.layout()[2] == 0
        r.close()
    assert outs[0] == outs[1] and all(any(b) for b in outs[0][:7])
    cres = vs.allele_counts(regions)
    ac = cres.allele_counts()
    r = vs.sample_ibs(regions)
    got = r.sample_ibs()
    for f in ("carriers", "alt_alleles", "hom_alt", "phased"):
        assert np.array_equal(got["counts"][f], ac["counts"][f]), f
    assert r.totals()[:2] == cres.totals()[:2] and tuple(got[f].tobytes() for f in INT_FIELDS) == outs[0][:6]
    # the diagonals are the rows' counts summed the other way: het calls = carriers - hom_alt, per sample through the burden query
    assert int(np.diagonal(got["carrier_both"]).sum()) == int(ac["counts"]["carriers"].astype(np.int64).sum())
    assert int(np.diagonal(got["hom_hom"]).sum()) == int(ac["counts"]["hom_alt"].astype(np.int64).sum())
    r.close(); cres.close()


# ------------------------------------------------------------------------------------------------------- 5. housekeeping
def test_interleaving_leaves_type6_alone():
    rng = np.random.default_rng(12)
    batches = []
    for k in range(6):
        n = 3_000 + 200 * k + (4_000 if k == 4 else 0)   # like batches (speculated), one larger (refused / re-sized)
        s = np.sort(rng.integers(1_000, 7_990_000, size=n))
        batches.append(np.stack([s, s + rng.integers(50, 3_000, size=n)], axis=1).astype(np.uint64))
    shuffled = batches[3][rng.permutation(batches[3].shape[0])]

    def run(with_ibs):
        vs = VariantStore.synthetic(device=0, **T6_KW)
        digests = []
        for k, b in enumerate(batches):
            r = vs.get_var_in_ref(b)
            if with_ibs:   # IBS batches in between: sorted, unsorted, with a subset
                g1 = vs.sample_ibs(b, stat="king")
                g2 = vs.sample_ibs(shuffled, stat="counts")
                g3 = vs.sample_ibs(shuffled, [1, 5, 7, 200])
                for g in (g1, g2, g3):
                    g.totals()
                    g.close()
            digests.append(r.digest())
            r.close()
        info = vs.info()
        out = (digests, info.t6_speculated, info.t6_refused)
        vs.close()
        return out

    plain, mixed = run(False), run(True)
    assert plain[1] > 0, "the type-6 batches were not speculated"
    assert plain == mixed


def test_temporary_matrix_leaves_an_open_result():
    """The temporary genotype matrix is not part of the result: once a result has been read (its kernels have finished) the matrix
    is back in the handle's pool while the result is still open, and a second whole-cohort batch beside it takes that buffer.
    64 columns and more than 5,120 rows: the matrix (rows x 64 bytes) is larger than every other buffer of the batch -- the table
    takes 32 bytes a row, the five IBS matrices 160 KiB, no more than a table --, so nothing else in the pool can stand in for
    it.  Five 16-sample batches open side by side first leave the pool every smaller buffer two more batches take (a table's
    buffer holds the whole cohort's IBS matrices)."""
    vs = VariantStore.synthetic(device=0, ref_length=60_000, num_variants=5400, num_samples=64, seed=77, first_pos=100, frac_ins=0.06,
                                frac_del=0.06, frac_multi=0.03, max_indel=4, af_exponent=2.5)
    regions = [(1, 30_000), (20_000, 60_000), (100, 200)]
    warm = [vs.sample_ibs(regions, list(range(1, 17))) for _ in range(5)]
    for w in warm:
        w.sample_ibs()
    for w in warm:
        w.close()
    m0 = vs.info().pool_mallocs
    first = vs.sample_ibs(regions)
    got = first.sample_ibs()   # (waits for the batch)
    a = got["rows"].shape[0]
    assert a >= 5400 and a * 32 >= 64 * 64 * 40 + 24 and vs.info().pool_mallocs > m0, "the whole-cohort matrix must have been a new buffer"
    m1 = vs.info().pool_mallocs
    second = vs.sample_ibs(regions)   # beside the open result
    got2 = second.sample_ibs()
    assert vs.info().pool_mallocs == m1, "the open result still holds its temporary matrix"
    # both results are whole and their own: the second batch ran in the first's matrix buffer, not in anything the first still reads
    mres = vs.genotype_matrix(regions)
    mm = mres.genotype_matrix()
    mres.close()
    want = sample_ibs(np.ascontiguousarray(mm["cells"]), (mm["rows"]["count_flags"] >> 31) != 0)
    for g in (got, got2, first.sample_ibs(), second.sample_ibs()):
        _compare(g, want, "counts")
    assert want["het_het"].any() and first.sample_ibs_device()[3:] == (a, 64, "counts")
    first.close(); second.close()
    vs.close()


def test_size_limit(t6_store):
    vs, regions = t6_store
    warm = vs.allele_counts(regions)   # the plan's temporaries, the table and the counts of this batch are in the handle's pool afterwards
    a = warm.allele_counts()["rows"].shape[0]
    warm.close()
    c = vs.info().num_samples - 1
    pitch = (c + 15) // 16 * 16
    matrix_bytes, cell_bytes, king_bytes = a * pitch, c * c * 40, c * c * 48
    assert matrix_bytes > 4 << 20 and king_bytes > 4 << 20 > cell_bytes + 64 * pitch
    vs.set_option("matrix_max_mib", 4)
    try:
        before = vs.info().pool_mallocs
        with pytest.raises(VariantStoreError) as e:
            vs.sample_ibs(regions)
        assert e.value.code == VS_ERR_ARG
        msg = str(e.value)
        for number in (a, c, matrix_bytes + cell_bytes, matrix_bytes, cell_bytes):
            assert str(number) in msg, (number, msg)
        assert "matrix_max_mib" in msg, msg
        with pytest.raises(VariantStoreError) as e:   # 48 bytes a cell under KING: the cells alone are beyond the limit
            vs.sample_ibs(regions[:1], stat="king")
        assert e.value.code == VS_ERR_ARG and str(king_bytes) in str(e.value)
        assert vs.info().pool_mallocs == before, "a refused batch allocated"
        few = vs.sample_ibs(regions[:20], [1, 2, 3], stat="king")   # below the limit
        assert few.sample_ibs()["king"].shape == (3, 3)
        few.close()
        one = vs.sample_ibs(regions[:1])   # 40 bytes a cell: fits
        assert one.sample_ibs()["ibs2"].shape == (c, c)
        one.close()
    finally:
        vs.set_option("matrix_max_mib", 0)
    again = vs.sample_ibs(regions, stat="king")
    assert again.sample_ibs()["king"].shape == (c, c)
    again.close()


def test_refused_accessors(t6_store):
    vs, regions = t6_store
    r = vs.sample_ibs(regions[:1_000], stat="king")
    for call in (lambda: r.raw(with_carriers=True), lambda: r.view(with_carriers=True), r.digest, r.num_header_records,
                 r.num_region_records, lambda: r.region_text(0)):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_UNSUPPORTED
    for call in (r.allele_counts, r.sample_burden, r.sample_burden_device, r.genotype_matrix, r.genotype_matrix_device, r.ld_band,
                 r.ld_band_device, r.sample_scores, r.sample_scores_device, r.sample_gram, r.sample_gram_device, r.assoc_scan,
                 r.group_counts):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_ARG
    r.view(with_carriers=False)
    raw = r.raw(with_carriers=False)
    t6 = vs.get_var_in_ref(regions[:1_000])
    raw6 = t6.raw(with_carriers=False)
    for f in ("pos", "ref_off", "ref_len", "alt_off", "alt_len", "count_flags"):
        assert np.array_equal(raw["rows"][f], raw6["rows"][f]), f
    assert np.array_equal(raw["region_flags"], raw6["region_flags"]) and np.array_equal(raw["row_count"], raw6["row_count"])
    assert r.totals()[:2] == t6.totals()[:2] and r.fill_ms() > 0
    r.close()
    for res in (t6, vs.allele_counts(regions[:10]), vs.sample_burden(regions[:10]), vs.genotype_matrix(regions[:10]),
                vs.ld_band(regions[:10], window=4), vs.sample_gram(regions[:10], stat="grm")):
        with pytest.raises(VariantStoreError) as e:
            res.sample_ibs()   # not an IBS result
        assert e.value.code == VS_ERR_ARG
        with pytest.raises(VariantStoreError) as e:
            res.sample_ibs_device()
        assert e.value.code == VS_ERR_ARG
        res.close()


def test_device_pointers(t6_store):
    torch = pytest.importorskip("torch")
    vs, regions = t6_store
    sub = [3, 17, 40, 200, 250]
    r = vs.sample_ibs(regions[:2_500], sub, stat="king")
    got = r.sample_ibs()
    pm, pk, pc, a, n, stat = r.sample_ibs_device()
    assert (a, n, stat) == (got["rows"].shape[0], 5, "king") and pm and pk and pc
    later = vs.sample_ibs(regions[2_500:2_900])   # a later batch on the same handle leaves the result alone
    later.totals()
    words = _read_device_bytes(torch, pm, 5 * n * n + 1, 8).view(np.int64).reshape(5 * n * n + 1)
    for k, f in enumerate(("het_het", "hom_hom", "carrier_both", "ibs0", "ibs2")):
        assert np.array_equal(words[k * n * n:(k + 1) * n * n].reshape(n, n), got[f]) and got[f].any(), f
    assert int(words[5 * n * n]) == got["n_used"] > 0
    assert _read_device_bytes(torch, pk, n * n, 8).tobytes() == got["king"].tobytes()
    assert np.array_equal(_read_device_bytes(torch, pc, a, 16).view(np.uint32).reshape(a, 4), got["counts"].view(np.uint32).reshape(a, 4))
    later.close(); r.close()
    d = vs.sample_ibs(regions[:100], sub)
    assert d.sample_ibs_device()[1] == 0 and d.sample_ibs()["king"] is None   # no kinship under "counts"
    d.close()


# ------------------------------------------------------------------------------------------------------------- 6. the CLI
def test_cli_ibs(tmp_path):
    """A cohort of nine samples (the golden files hold one: no pair): the pair table with and without -S, --king and --min-kinship."""
    exe = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    fasta, vcf, _names = write_random_cohort(str(tmp_path), 702, ref_len=6000, n_rows=400, n_samples=9)
    subprocess.run([exe, "construct", "-r", fasta, "-v", vcf, "-p", prefix], check=True, capture_output=True)
    vs = VariantStore.open(prefix, device=0)
    assert vs.info().num_samples - 1 == 9
    regions = [(x, x + 250) for x in range(1, 5900, 300)] + [(1000, 3000)]
    rfile = os.path.join(tmp_path, "regions.txt")
    with open(rfile, "w") as f:
        f.write("".join(f"{x}:{y}\n" for x, y in regions))
    names = [vs.sample_name(i) for i in (7, 2, 4, 9)]
    sfile = os.path.join(tmp_path, "samples.txt")
    with open(sfile, "w") as f:
        f.write("\n".join(names) + "\n")
    out = os.path.join(tmp_path, "ibs.txt")

    def run(flags):
        p = subprocess.run([exe, "ibs", "-p", prefix, "-r", "@" + rfile, "-o", out] + flags, check=True, capture_output=True)
        assert p.stdout == b""
        with open(out, "rb") as f:
            return f.read().decode("latin-1")

    for samples, extra in ((None, []), (names, ["-S", sfile])):
        res = vs.sample_ibs(regions, samples, stat="king")
        got = res.sample_ibs()
        res.close()
        cols = [vs.sample_name(int(i)) for i in got["columns"]]
        pairs = got["king"][np.triu_indices(len(cols), 1)]
        assert got["het_het"].any() and got["ibs0"].any() and pairs.size == len(cols) * (len(cols) - 1) // 2 and pairs.min() < pairs.max()
        if samples is None:
            assert run(extra) == ibs_text(cols, got, "counts")
            thr = float(np.median(pairs))     # keeps some pairs and leaves some out
        else:
            assert cols == sorted(names) and run(extra + ["--king"]) == ibs_text(cols, got, "king")
            thr = float(pairs.max()) + 1.0    # keeps none: the header alone
        text = run(extra + ["--min-kinship", "%.17g" % thr])
        assert text == ibs_text(cols, got, "counts", min_kinship=thr), (samples, thr)
        assert text.count("\n") == 1 + int((pairs >= thr).sum()) and (samples is not None or 1 < text.count("\n") < 1 + pairs.size)
    vs.close()
