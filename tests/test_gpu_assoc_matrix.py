"""Trait-matrix association scans on the GPU (vs_query_assoc_matrix): every cell against the dosages of the engine's own genotype
matrix times the reference's quantised traits -- the MFMA k-step, the staged chunk and every pitch residue, the trait-tile edges,
several 64-row tiles and a remainder --, small and empty tables, a saturated column set whose limb sums reach 2 * 128 * n, assoc_scan
where both are exact, the oracle's type-6 text, column subsets, the storage forms of the genotype bits, determinism, the size limit,
interleaving with type-6 batches, the temporary matrix, the refused accessors, the device pointers and the CLI.

DOT scores are compared bit for bit with np.ldexp of the int64 product and `sums` as integers; CHI2 bit for bit with the reference
formed from exact integers (assoc_matrix_ref)."""
import os
import subprocess

import numpy as np
import pytest

import assoc_matrix_ref as ref
import assoc_scan_ref
from genotype_matrix_ref import Parsed, matrix
from helpers import oracle_texts, write_saturated_cohort
from ld_band_ref import dosage
from oracle.oracle import Oracle
from test_gpu_genotype_matrix import _read_device as _read_device_bytes, _reported
from variantstore_amd import VariantStore
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_ARG, VS_ERR_UNSUPPORTED = -5, -7


def _panel(n, K, rng):
    """(n, K) float32 in three forms: the chosen-q columns (limb extremes reach the matrix cores), one column of zeros, random
    normals of mixed scales."""
    chosen, _q = ref.chosen_traits(n)
    cols = [chosen[:, 0], chosen[:, 1], np.zeros(n, np.float32)]
    while len(cols) < K:
        cols.append((rng.standard_normal(n) * 10.0 ** int(rng.integers(-4, 5))).astype(np.float32))
    order = [0, 3, 1, 2] + list(range(4, len(cols))) if K >= 4 else list(range(K))   # (a normal column between the chosen ones)
    return np.ascontiguousarray(np.stack([cols[i] for i in order[:K]], axis=1), np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _query(vs, regions, ycol, samples, stat, rng=None, names=None):
    """The query with `ycol` (rows in column order); a subset's ids are given shuffled, their rows with them."""
    if samples is None:
        return vs.assoc_matrix(regions, ycol, None, stat, names)
    ids = sorted({vs.sample_id(i) if isinstance(i, str) else int(i) for i in samples})
    perm = np.arange(len(ids)) if rng is None else rng.permutation(len(ids))
    given = [vs.sample_name(ids[i]) if isinstance(samples[0], str) else ids[i] for i in perm]
    return vs.assoc_matrix(regions, ycol[perm], given, stat, names)


def _check_full(vs, regions, samples, ycol, what=None, rng=None, stats=("dot", "chi2")):
    """Every cell of both statistics against the genotype matrix over the same regions and samples.  Returns (matrix arrays, the
    DOT result's arrays)."""
    mres = vs.genotype_matrix(regions, samples)
    m = mres.genotype_matrix()
    mres.close()
    cells = np.ascontiguousarray(m["cells"])
    a, n = cells.shape
    d = dosage(cells).astype(np.int64)
    K = ycol.shape[1]
    assert ycol.shape[0] == n
    q, f = ref.quantise(ycol)
    S = ref.dot(d, q)
    out = None
    for stat in stats:
        res = _query(vs, regions, ycol, samples, stat, rng)
        got = res.assoc_matrix()
        print(f"assoc_matrix {what}: {a} rows x {n} columns x {K} traits, {stat}: {int(np.count_nonzero(got['scores']))} nonzero cells, "
              f"{int(np.count_nonzero(d))} nonzero dosages, fill {res.fill_ms():.3f} ms")
        assert got["stat"] == stat and got["col_ids"].dtype == np.uint32 and got["col_ids"].tolist() == m["columns"].tolist()
        assert got["scores"].dtype == np.float64 and got["scores"].shape == (a, K) and got["counts"].shape == (a,)
        assert np.array_equal(got["rows"]["pos"], m["rows"]["pos"])
        assert np.array_equal(got["row_begin"], m["row_begin"]) and np.array_equal(got["row_count"], m["row_count"])
        assert got["shift"].dtype == np.int32 and got["shift"].tolist() == f.tolist()
        sy, syy = ref.trait_sums(q, f)
        assert _bits(got["trait_sum"]).tolist() == _bits(sy).tolist() and _bits(got["trait_sumsq"]).tolist() == _bits(syy).tolist()
        assert np.array_equal(got["counts"]["alt_alleles"].astype(np.int64), d.sum(axis=1))
        assert np.array_equal(got["counts"]["hom_alt"].astype(np.int64), (d == 2).sum(axis=1))
        if stat == "dot":
            want = ref.scores_dot(S, f)
            bad = np.argwhere(_bits(got["scores"]) != _bits(want))
            assert bad.shape[0] == 0, (what, stat, a, n, K, bad[:8].tolist())
            assert got["sums"].dtype == np.int64 and np.array_equal(got["sums"], S), (what, "sums")
            out = got
        else:
            want = ref.chi2_table(n, d.sum(axis=1), (d == 2).sum(axis=1), S, q)
            bad = np.argwhere(_bits(got["scores"]) != _bits(want))
            assert bad.shape[0] == 0, (what, stat, a, n, K, bad[:8].tolist(), [(got["scores"][i, k], want[i, k]) for i, k in bad[:4]])
            assert got["sums"] is None and (got["scores"] >= 0).all()
            head = slice(0, min(a, 40))   # the table form of the reference against the Python integers, on the table's head
            assert ref.chi2(n, d.sum(axis=1)[head], (d == 2).sum(axis=1)[head], S[head], q).tobytes() == want[head].tobytes()
        dropped = (got["rows"]["count_flags"] >> 31) != 0
        assert not got["scores"][dropped].any() and not np.signbit(got["scores"][dropped]).any()
        res.close()
    return m, out


def _pitch_cohort(n_cols):   # (test_gpu_sample_gram's sizes)
    return VariantStore.synthetic(device=0, ref_length=60_000, num_variants=1500, num_samples=n_cols, seed=900 + n_cols, first_pos=100,
                                  frac_ins=0.06, frac_del=0.06, frac_multi=0.03, max_indel=4, af_exponent=1.0)


def _pitch_regions(vs, rng):
    L = vs.info().ref_length
    starts = rng.integers(1, L - 4000, size=60)
    return [(int(s), int(s) + int(rng.integers(1, 4000))) for s in starts] + [(1, 3000), (L - 2000, L + 5)]


# ------------------------------------------------------------------- 1. against the engine's own matrix, every cell
@pytest.mark.parametrize("n_cols", [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300])
def test_every_cell_against_the_matrix(n_cols):
    """The MFMA k-step (64), the staged chunk (256) and every pitch residue class; per cohort the trait-tile edges K = 1, 15, 16,
    17, 33 and 100; more than three 64-row tiles and a remainder.  The batch is unsorted: the device sorts it."""
    vs = _pitch_cohort(n_cols)
    rng = np.random.default_rng(n_cols)
    regions = _pitch_regions(vs, rng)
    probe = vs.allele_counts(regions)
    while probe.allele_counts()["rows"].shape[0] % 64 == 0:   # (a remainder of the 64-row tile, whatever the cohort)
        probe.close()
        regions = regions[:-1]
        probe = vs.allele_counts(regions)
    probe.close()
    for K in (1, 15, 16, 17, 33, 100):
        y = _panel(n_cols, K, rng)
        m, got = _check_full(vs, regions, None, y, (n_cols, K))
        cells = m["cells"]
        a = cells.shape[0]
        assert cells.shape[1] == n_cols and m["row_pitch"] == (n_cols + 15) // 16 * 16
        assert a > 3 * 64 and a % 64 != 0, "several row tiles and a remainder"
        if n_cols >= 63:   # distinct rows and distinct trait columns: a wrong lane map cannot hide behind uniform data
            assert np.unique(cells, axis=0).shape[0] > a // 4, (np.unique(cells, axis=0).shape[0], a)
            assert np.unique(y, axis=1).shape[1] == K
            if K >= 16:
                assert np.unique(got["scores"], axis=0).shape[0] > a // 4
                assert np.unique(got["scores"], axis=1).shape[1] >= K - 1
    vs.close()


def test_small_tables_and_the_empty_one():
    """Tables of 0, 1, 15, 16, 17, 63, 64 and 65 rows."""
    vs = _pitch_cohort(65)
    rng = np.random.default_rng(3)
    L = vs.info().ref_length
    probe = vs.allele_counts([(1, L)])
    pos = np.unique(probe.allele_counts()["rows"]["pos"].astype(np.int64))
    probe.close()
    spans = [(int(pos[k]), int(pos[k + m])) for m in (0, 1, 2, 13, 14, 15, 16, 17, 61, 62, 63, 64, 65, 66) for k in range(0, 60, 3)]
    cres = vs.allele_counts(spans)
    n_rows = cres.allele_counts()["row_count"].astype(np.int64)
    cres.close()
    y = _panel(65, 17, rng)
    for want in (1, 15, 16, 17, 63, 64, 65):
        hit = np.nonzero(n_rows == want)[0]
        assert hit.size, (want, sorted(set(n_rows.tolist())))
        m, _ = _check_full(vs, [spans[int(hit[0])]], None, y, want)
        assert m["cells"].shape[0] == want
    first = int(pos[0])
    assert first > 2
    for stat in ("dot", "chi2"):   # a table without rows: a 0 x K result, not an error
        res = vs.assoc_matrix([(1, first - 2)], y, stat=stat, trait_names=[f"t{k}" for k in range(17)])
        got = res.assoc_matrix()
        assert got["scores"].shape == (0, 17) and got["counts"].shape == (0,) and got["rows"].shape == (0,)
        assert got["shift"].shape == (17,) and got["trait_names"] == [f"t{k}" for k in range(17)]
        assert res.totals()[1:3] == (0, 0)
        assert res.assoc_matrix_device()[2:] == (0, 65, 17, stat)
        res.close()
    vs.close()


def test_saturated_columns(tmp_path):
    """Rows on which all 300 samples are hom-alt (a VCF written here: the synthetic generator caps an allele's frequency) against
    trait columns at +-M_k: a limb sum reaches 2 * 128 * n, S = 2 n (2^30 - 64) is the largest for this n."""
    n = 300
    fasta, vcf = write_saturated_cohort(str(tmp_path), n, 4700, rows=150, two_alt=False, extremes=True)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    assert vs.info().num_samples - 1 == n
    top = float(2 ** 30 - 64)
    half = np.where(np.arange(n) < n // 2, top, -top)
    y = np.stack([np.full(n, top), np.full(n, float(0x20800000)), np.where(np.arange(n) % 2 == 0, top, -top), half,
                  np.full(n, -top), np.where(np.arange(n) % 3 == 0, float(-(128 << 16)), float(127 << 16))], axis=1).astype(np.float32)
    y[0, 5] = float(2 ** 30 - 64)   # (the column's M_k, so that the chosen values come back as q)
    q, f = ref.quantise(y)
    assert not f.any() and ref.limbs(q)[:, 1, 2].tolist() == [-128] * n and set(ref.limbs(q)[1:, 5, 2].tolist()) == {-128, 127}
    regions = [(1, 20_001)]
    m, got = _check_full(vs, regions, None, y, "saturated")
    d = dosage(np.ascontiguousarray(m["cells"])).astype(np.int64)
    full = np.nonzero((d == 2).all(axis=1))[0]
    assert full.size >= 2, "no row on which every sample is hom-alt"
    assert (got["sums"][full, 0] == 2 * n * (2 ** 30 - 64)).all() and (got["sums"][full, 4] == -2 * n * (2 ** 30 - 64)).all()
    assert (d[full] @ ref.limbs(q)[:, 1, 2] == -2 * 128 * n).all()
    sub = list(range(1, n + 1, 2))   # ... and on a subset: the alternating column is constant there, the halves are not
    _check_full(vs, regions, sub, y[::2], "saturated subset", np.random.default_rng(1))
    vs.close()


# ------------------------------------------------------------------------------------------------ 2. cross-checks
def test_dot_equals_assoc_scan_on_small_integers():
    """K <= 8 small integer-valued traits: both queries are exact, so their DOT cells are the same bytes."""
    vs = _pitch_cohort(257)
    rng = np.random.default_rng(21)
    regions = _pitch_regions(vs, rng)
    for K, samples in ((1, None), (3, None), (8, None), (8, [int(i) for i in rng.choice(np.arange(1, 258), size=70, replace=False)])):
        n = 257 if samples is None else len(samples)
        y = rng.integers(-8, 9, size=(n, K)).astype(np.float32)
        a = vs.assoc_scan(regions, y, samples, "dot")
        b = vs.assoc_matrix(regions, y, samples, "dot")
        ga, gb = a.assoc_scan(), b.assoc_matrix()
        assert ga["scores"].shape == gb["scores"].shape and ga["scores"].any()
        assert _bits(ga["scores"]).tolist() == _bits(gb["scores"]).tolist(), (K, samples is None)
        for field in ("carriers", "alt_alleles", "hom_alt", "phased"):
            assert np.array_equal(ga["counts"][field], gb["counts"][field])
        assert ga["col_ids"].tolist() == gb["col_ids"].tolist()
        a.close(); b.close()
    vs.close()


def _ref_len(fasta):
    with open(fasta) as f:
        return sum(len(line.strip()) for line in f if not line.startswith(">"))


@pytest.mark.parametrize("stem", ["x", "x.small"])
def test_golden_disjoint_regions_against_the_oracle(stem, golden_dir, tmp_path):
    """Disjoint regions, so that each site is reported once: the cells and the region text from the oracle's type-6 text."""
    fasta, vcf = os.path.join(golden_dir, stem + ".fa"), os.path.join(golden_dir, stem + ".vcf")
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    plain = os.path.join(tmp_path, "plain.bin")
    vs.export_plain(plain)
    orc = Oracle(plain)
    L = _ref_len(fasta)
    step = max(40, L // 50)
    regions = [(x, min(L, x + step - 12)) for x in range(1, L, step)]   # gaps of 12 bases between them
    want = oracle_texts(orc, regions)
    assert all(n >= 0 for n, _e, _t in want)
    parsed = Parsed([t for _n, _e, t in want])
    assert parsed.n_rows > 0
    ids = list(range(1, vs.info().num_samples))
    rng = np.random.default_rng(4)
    K = 12
    tn = [f"gene{k}" for k in range(K)]
    for samples in (None, ids[:1], ids[::2]):
        cols = ids if samples is None else sorted(set(samples))
        names = [vs.sample_name(i) for i in cols]
        wm = matrix(parsed, names)
        d = dosage(wm).astype(np.int64)
        y = _panel(len(cols), K, rng)
        q, f = ref.quantise(y)
        S = ref.dot(d, q)
        cnt = assoc_scan_ref.counts(parsed, names)
        for stat in ("dot", "chi2"):
            exp = ref.scores_dot(S, f) if stat == "dot" else ref.chi2(len(cols), cnt[:, 1], cnt[:, 2], S, q)
            res = _query(vs, regions, y, samples, stat, rng, tn)
            got = res.assoc_matrix()
            mine, n_mine = _reported(got, range(len(regions)))
            assert mine.shape[0] == parsed.n_rows == wm.shape[0] and np.array_equal(n_mine, parsed.row_count), "a site is reported twice"
            assert _bits(got["scores"][mine]).tolist() == _bits(exp).tolist(), (samples, stat)
            assert got["trait_names"] == tn and got["col_ids"].tolist() == cols
            for qi in range(len(regions)):
                assert res.region_text(qi) == assoc_scan_ref.assoc_text(parsed, qi, cnt, exp, tn), (qi, stat)
            rows = res.region_assoc_matrix(0)
            assert len(rows) == int(parsed.row_count[0]) and all(set(r["scores"]) == set(tn) for r in rows)
            res.close()
    vs.close()


# ------------------------------------------------------------------------------------------ 3. subsets and storage forms
def test_column_subsets_by_id_and_by_name():
    """A subset given shuffled, by id and by name: the engine permutes the phenotype rows into column order.  A repeated id is
    refused as vs_query_assoc_scan refuses it (a sample has one row of phenotypes), and so is an unknown one."""
    vs = _pitch_cohort(129)
    rng = np.random.default_rng(8)
    sub = [int(i) for i in rng.choice(np.arange(1, 130), size=37, replace=False)]
    regions = _pitch_regions(vs, rng)
    y = _panel(37, 20, rng)
    for batch in (sorted(regions), regions):   # (the device sorts the unsorted one)
        m, got = _check_full(vs, batch, sub, y, "subset", rng)
        assert got["col_ids"].tolist() == sorted(sub) and m["cells"].shape[1] == 37
    _check_full(vs, regions, [vs.sample_name(i) for i in sub], y, "names", rng)
    m, got = _check_full(vs, regions, [vs.sample_name(sub[0])], y[:1], "one name")   # n = 1: vy = 0, every CHI2 cell 0
    assert got["scores"].shape[1] == 20 and got["scores"].any()
    with pytest.raises(VariantStoreError) as e:
        vs.assoc_matrix(regions, np.concatenate([y, y[:5]]), sub + sub[:5])
    assert e.value.code == VS_ERR_ARG and "twice" in str(e.value)
    with pytest.raises(VariantStoreError):
        vs.assoc_matrix(regions, y[:1], [130])
    vs.close()


@pytest.mark.parametrize("list_max", [0, 3, 64])
def test_listed_and_dense_classes(list_max, monkeypatch):
    monkeypatch.setenv("VS_LIST_MAX", str(list_max))
    vs = VariantStore.synthetic(device=0, ref_length=60_000, num_variants=1500, num_samples=150, seed=650, first_pos=100,
                                frac_ins=0.06, frac_del=0.06, frac_multi=0.03, max_indel=4, af_exponent=2.5)
    assert vs.info().list_max == list_max
    rng = np.random.default_rng(list_max)
    regions = _pitch_regions(vs, rng)
    subset = [int(i) for i in rng.choice(np.arange(1, 150), size=50, replace=False)]
    _check_full(vs, regions, None, _panel(150, 20, rng), list_max)
    _check_full(vs, regions, subset, _panel(50, 5, rng), list_max, rng)
    vs.close()


def test_explicit_ids_many_columns():
    """An explicit-id cohort above 4,096 samples: several column tiles of the matrix kernel, 17 staged chunks."""
    vs = VariantStore.synthetic(device=0, ref_length=100_000, num_variants=400, num_samples=4_300, seed=9, first_pos=2_000, frac_ins=0.05,
                                frac_del=0.05, frac_multi=0.01, max_indel=6, af_exponent=2.0, max_af=0.002)
    info = vs.info()
    assert not info.use_bit_vector and info.num_samples - 1 > 4_096
    regions = [(1, 40_000), (30_000, 70_000), (60_000, 100_000), (2_500, 2_600)]
    m, got = _check_full(vs, regions, None, _panel(4_300, 19, np.random.default_rng(2)), "explicit")
    assert m["cells"][:, 4_096:].any(), "no column beyond the matrix kernel's first tile is set"
    assert m["cells"].shape[0] > 200 and got["scores"].any()
    vs.close()


# ------------------------------------------------------------------------------------ 4. determinism, limits, housekeeping
T6_KW = dict(ref_length=8_000_000, num_variants=150_000, num_samples=300, seed=5, first_pos=1_000, frac_ins=0.05, frac_del=0.05,
             frac_multi=0.02, max_indel=6, af_exponent=2.0)


@pytest.fixture(scope="module")
def t6_store():
    vs = VariantStore.synthetic(device=0, **T6_KW)
    rng = np.random.default_rng(12)
    s = np.sort(rng.integers(1_000, 7_990_000, size=3_000))
    regions = np.stack([s, s + rng.integers(50, 3_000, size=3_000)], axis=1).astype(np.uint64)
    yield vs, regions, _panel(300, 40, rng)
    vs.close()


def test_two_calls_give_the_same_bytes(t6_store):
    vs, regions, y = t6_store
    for stat in ("dot", "chi2"):
        outs = []
        for _ in range(2):
            r = vs.assoc_matrix(regions, y, stat=stat)
            g = r.assoc_matrix()
            outs.append((g["scores"].tobytes(), g["counts"].tobytes(), g["trait_sum"].tobytes(), g["trait_sumsq"].tobytes(), g["shift"].tobytes()))
            assert r.fill_ms() > 0 and r.layout()[2] == 0
            r.close()
        assert outs[0] == outs[1] and any(outs[0][0])
    cres = vs.allele_counts(regions)
    ac = cres.allele_counts()
    r = vs.assoc_matrix(regions, y)
    got = r.assoc_matrix()
    for f in ("carriers", "alt_alleles", "hom_alt", "phased"):
        assert np.array_equal(got["counts"][f], ac["counts"][f]), f
    assert r.totals() == cres.totals()
    r.close(); cres.close()


def test_size_limit(t6_store):
    vs, regions, y = t6_store
    warm = vs.allele_counts(regions)   # the plan's temporaries, the table and the counts of this batch are in the handle's pool afterwards
    a = warm.allele_counts()["rows"].shape[0]
    warm.close()
    c = vs.info().num_samples - 1
    pitch = (c + 15) // 16 * 16
    K = y.shape[1]
    matrix_bytes, cell_bytes, count_bytes, panel_bytes = a * pitch, a * K * 8, a * 16, (K + 15) // 16 * 64 * pitch
    assert matrix_bytes + cell_bytes > 1 << 20 > panel_bytes
    vs.set_option("matrix_max_mib", 1)
    try:
        before = vs.info().pool_mallocs
        with pytest.raises(VariantStoreError) as e:
            vs.assoc_matrix(regions, y)
        assert e.value.code == VS_ERR_ARG
        msg = str(e.value)
        for number in (a, c, K, matrix_bytes + cell_bytes + count_bytes + panel_bytes, matrix_bytes, cell_bytes, count_bytes, panel_bytes):
            assert str(number) in msg, (number, msg)
        assert "matrix_max_mib" in msg, msg
        wide = np.zeros((c, 1024), np.float32)   # the limb panel alone is beyond the limit: 64 tiles x 64 rows x 304 bytes
        with pytest.raises(VariantStoreError) as e:
            vs.assoc_matrix(regions[:1], wide)
        assert e.value.code == VS_ERR_ARG and str(64 * 64 * pitch) in str(e.value)
        assert vs.info().pool_mallocs == before, "a refused batch allocated"
        few = vs.assoc_matrix(regions[:20], y[:3, :2], [1, 2, 3], stat="chi2")   # below the limit
        assert few.assoc_matrix()["scores"].shape[1] == 2
        few.close()
    finally:
        vs.set_option("matrix_max_mib", 0)
    again = vs.assoc_matrix(regions, y)
    assert again.assoc_matrix()["scores"].shape == (a, K)
    again.close()


def test_interleaving_leaves_type6_alone():
    rng = np.random.default_rng(12)
    batches = []
    for k in range(6):
        n = 3_000 + 200 * k + (4_000 if k == 4 else 0)   # like batches (speculated), one larger (refused / re-sized)
        s = np.sort(rng.integers(1_000, 7_990_000, size=n))
        batches.append(np.stack([s, s + rng.integers(50, 3_000, size=n)], axis=1).astype(np.uint64))
    shuffled = batches[3][rng.permutation(batches[3].shape[0])]
    y = _panel(300, 20, rng)

    def run(with_assoc):
        vs = VariantStore.synthetic(device=0, **T6_KW)
        digests = []
        for k, b in enumerate(batches):
            r = vs.get_var_in_ref(b)
            if with_assoc:   # trait-matrix batches in between: sorted, unsorted, with a subset
                g1 = vs.assoc_matrix(b, y, stat="chi2")
                g2 = vs.assoc_matrix(shuffled, y, stat="dot")
                g3 = vs.assoc_matrix(shuffled, y[:4], [1, 5, 7, 200])
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
    K = 1 and 64 columns: the matrix (rows x 64 bytes) is larger than every other buffer of the batch (the table takes 32 bytes a
    row, counts 16, cells 8, the limb panel 4 KiB).  Five 16-sample batches open side by side first leave the pool every smaller
    buffer two more batches take."""
    vs = VariantStore.synthetic(device=0, ref_length=60_000, num_variants=1500, num_samples=64, seed=77, first_pos=100, frac_ins=0.06,
                                frac_del=0.06, frac_multi=0.03, max_indel=4, af_exponent=2.5)
    regions = [(1, 30_000), (20_000, 60_000), (100, 200)]
    y = _panel(64, 1, np.random.default_rng(0))
    warm = [vs.assoc_matrix(regions, y[:16], list(range(1, 17))) for _ in range(5)]
    for w in warm:
        w.assoc_matrix()
    for w in warm:
        w.close()
    m0 = vs.info().pool_mallocs
    first = vs.assoc_matrix(regions, y)
    got = first.assoc_matrix()   # (waits for the batch)
    a = got["rows"].shape[0]
    assert a >= 1500 and vs.info().pool_mallocs > m0, "the whole-cohort matrix must have been a new buffer"
    m1 = vs.info().pool_mallocs
    second = vs.assoc_matrix(regions, y)   # beside the open result
    got2 = second.assoc_matrix()
    assert vs.info().pool_mallocs == m1, "the open result still holds its temporary matrix"
    mres = vs.genotype_matrix(regions)
    d = dosage(np.ascontiguousarray(mres.genotype_matrix()["cells"])).astype(np.int64)
    mres.close()
    q, f = ref.quantise(y)
    want = ref.scores_dot(ref.dot(d, q), f)
    for g in (got, got2, first.assoc_matrix(), second.assoc_matrix()):
        assert _bits(g["scores"]).tolist() == _bits(want).tolist() and want.any()
    assert first.assoc_matrix_device()[2:] == (a, 64, 1, "dot")
    first.close(); second.close()
    vs.close()


def test_refused_accessors(t6_store):
    vs, regions, y = t6_store
    r = vs.assoc_matrix(regions[:1_000], y, stat="chi2")
    for call in (lambda: r.raw(with_carriers=True), lambda: r.view(with_carriers=True), r.digest, r.num_header_records,
                 r.num_region_records):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_UNSUPPORTED
    for call in (r.allele_counts, r.sample_burden, r.sample_burden_device, r.genotype_matrix, r.genotype_matrix_device, r.ld_band,
                 r.ld_band_device, r.sample_scores, r.sample_scores_device, r.assoc_scan, r.assoc_scan_device, r.sample_gram,
                 r.sample_gram_device, r.ld_matrix, r.ld_matrix_device):
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
    for res in (t6, vs.allele_counts(regions[:10]), vs.assoc_scan(regions[:10], y[:, :2]), vs.genotype_matrix(regions[:10]),
                vs.sample_gram(regions[:10]), vs.ld_band(regions[:10], window=4)):
        with pytest.raises(VariantStoreError) as e:
            res.assoc_matrix()   # not a trait-matrix result
        assert e.value.code == VS_ERR_ARG
        with pytest.raises(VariantStoreError) as e:
            res.assoc_matrix_device()
        assert e.value.code == VS_ERR_ARG
        res.close()


def test_device_pointers(t6_store):
    torch = pytest.importorskip("torch")
    vs, regions, y = t6_store
    sub = [3, 17, 40, 200, 250]
    r = vs.assoc_matrix(regions[:2_500], y[:5], sub, stat="chi2")
    got = r.assoc_matrix()
    ps, pc, a, n, K, stat = r.assoc_matrix_device()
    assert (a, n, K, stat) == (got["rows"].shape[0], 5, 40, "chi2") and ps and pc
    later = vs.assoc_matrix(regions[2_500:2_900], y)   # a later batch on the same handle leaves the result alone
    later.totals()
    assert _read_device_bytes(torch, ps, a * K, 8).tobytes() == got["scores"].tobytes() and got["scores"].any()
    assert np.array_equal(_read_device_bytes(torch, pc, a, 16).view(np.uint32).reshape(a, 4), got["counts"].view(np.uint32).reshape(a, 4))
    later.close(); r.close()


# ------------------------------------------------------------------------------------------------------------- 5. the CLI
def test_cli_assocmatrix(golden_dir, tmp_path):
    """`variantstore assocmatrix` on the golden x with K = 12: the text against assoc_text over the oracle's type-6 text."""
    exe = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    fasta = os.path.join(golden_dir, "x.fa")
    subprocess.run([exe, "construct", "-r", fasta, "-v", os.path.join(golden_dir, "x.vcf"), "-p", prefix], check=True, capture_output=True)
    vs = VariantStore.open(prefix, device=0)
    plain = os.path.join(tmp_path, "plain.bin")
    vs.export_plain(plain)
    orc = Oracle(plain)
    L = _ref_len(fasta)
    step = max(40, L // 50)
    regions = [(x, min(L, x + step - 12)) for x in range(1, L, step)]
    want = oracle_texts(orc, regions)
    parsed = Parsed([t for _n, _e, t in want])
    rfile = os.path.join(tmp_path, "regions.txt")
    with open(rfile, "w") as f:
        f.write("".join(f"{x}:{y}\n" for x, y in regions))
    ids = list(range(1, vs.info().num_samples))
    names = [vs.sample_name(i) for i in ids]
    rng = np.random.default_rng(6)
    K = 12
    y = _panel(len(ids), K, rng)
    tn = [f"g{k}" for k in range(K)]
    order = rng.permutation(len(ids))
    pfile = os.path.join(tmp_path, "pheno.txt")
    with open(pfile, "w") as f:   # float32 values written so that they read back as they are
        f.write("#sample " + " ".join(tn) + "\n" + "".join(names[i] + "\t" + " ".join(repr(float(v)) for v in y[i]) + "\n" for i in order))
    q, fk = ref.quantise(y)
    d = dosage(matrix(parsed, names)).astype(np.int64)
    S = ref.dot(d, q)
    cnt = assoc_scan_ref.counts(parsed, names)
    some = False
    for flags, exp in (([], ref.scores_dot(S, fk)), (["--chi2"], ref.chi2(len(ids), cnt[:, 1], cnt[:, 2], S, q))):
        out = os.path.join(tmp_path, "am.txt")
        subprocess.run([exe, "assocmatrix", "-p", prefix, "-r", "@" + rfile, "-P", pfile, "-o", out] + flags, check=True, capture_output=True)
        with open(out) as f:
            parts = f.read().split("#region ")[1:]
        assert len(parts) == len(regions)
        for qi, part in enumerate(parts):
            head, text = part.split("\n", 1)
            assert head == f"{qi} {regions[qi][0]}:{regions[qi][1]}"
            assert text == assoc_scan_ref.assoc_text(parsed, qi, cnt, exp, tn), (qi, flags)
        some |= bool(exp.any())
    assert some
    vs.close()
