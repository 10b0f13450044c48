"""Banded LD queries on the GPU (vs_query_ld_band): the band of dot products and of r^2 against what the oracle's type-6 text gives,
against the engine's own genotype matrix cell by cell (every pitch residue of the k loop, every window class, tables around the
row-block size), the storage forms of the genotype bits, the count records, a band buffer that comes from the pool, interleaving
with type-6 batches, regions in device memory, the device pointers, the size limit, the refused accessors and the CLI.

DOT is compared bit for bit.  R2 is compared with rtol = 2**-22 and atol = 0, and must be exactly 0 where the reference's vx * vy is
0: both sides round every double operation correctly, the four float32 ulps cover another association of the double products in
front of the final cast and nothing else."""
import os
import subprocess

import numpy as np
import pytest

from genotype_matrix_ref import Parsed, matrix
from helpers import oracle_texts, random_regions, write_random_cohort
from test_gpu_genotype_matrix import _read_device as _read_device_bytes
from ld_band_ref import dot_band, ld_text, pair_flat, pair_values, r2_band
from oracle.oracle import Oracle
from variantstore_amd import DeviceArray, VariantStore
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_ARG, VS_ERR_UNSUPPORTED = -5, -7
RTOL = 2.0 ** -22
WINDOWS = (1, 15, 16, 17, 64, 100, 256)


def _oracle(vs, tmp_path, name="plain.bin"):
    plain = os.path.join(tmp_path, name)
    vs.export_plain(plain)
    return Oracle(plain)


def _ref_len(fasta):
    with open(fasta) as f:
        return sum(len(line.strip()) for line in f if not line.startswith(">"))


def _parse(orc, regions):
    want = oracle_texts(orc, regions)
    valid = [q for q, (n, _e, _t) in enumerate(want) if n >= 0]
    assert valid
    return Parsed([t if n >= 0 else None for n, _e, t in want]), np.asarray(valid)


def _columns(vs, samples):
    ids = (list(range(1, vs.info().num_samples)) if samples is None
           else sorted({vs.sample_id(i) if isinstance(i, str) else int(i) for i in samples}))
    return ids, [vs.sample_name(i) for i in ids]


def _r2_close(got, want, zero, what=None):
    """got against the reference's float32 r^2: within 2**-22 relative, exactly 0 where `zero`."""
    assert got.dtype == np.float32 and got.shape == want.shape, what
    assert not got[zero].any(), what
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.all(err <= RTOL * np.abs(want.astype(np.float64))), (what, float(err.max()))
    assert np.all(np.isfinite(got)), what


def _shape_checks(got, ids, window, stat):
    a = got["rows"].shape[0]
    assert got["window"] == window and got["stat"] == stat
    assert got["columns"].dtype == np.uint32 and got["columns"].tolist() == ids
    assert got["band"].shape == (a, window) and got["band"].dtype == (np.int32 if stat == "dot" else np.float32)
    assert got["counts"].shape == (a,)


# ------------------------------------------------------------------------------------------------ 1. against the oracle
def _check_oracle(vs, regions, parsed, valid, samples, window, text_every=1):
    """Every pair of a region's reported rows at most `window` apart by table index, both statistics, and the text of every
    text_every-th region."""
    ids, names = _columns(vs, samples)
    want_m = matrix(parsed, names)
    out = None
    for stat in ("dot", "r2"):
        res = vs.ld_band(regions, samples, window=window, stat=stat)
        got = res.ld_band()
        _shape_checks(got, ids, window, stat)
        dropped = (got["rows"]["count_flags"] >> 31) != 0
        table_index = np.full(parsed.n_rows, -1, np.int64)
        pairs = 0
        for q in valid:
            a = np.arange(int(got["row_begin"][q]), int(got["row_begin"][q]) + int(got["row_count"][q]))
            a = a[~dropped[a]]
            r0 = int(parsed.row_begin[q])
            assert a.shape[0] == int(parsed.row_count[q]), (q, regions[q])
            table_index[r0:r0 + a.shape[0]] = a
            x, y = np.nonzero((a[None, :] - a[:, None] >= 1) & (a[None, :] - a[:, None] <= window))
            mine = got["band"][a[x], a[y] - a[x] - 1]
            want = pair_values(want_m, r0 + x, r0 + y, stat)
            pairs += x.shape[0]
            if stat == "dot":
                assert np.array_equal(mine, want), (q, regions[q], samples, window)
            else:
                _r2_close(mine, want, pair_flat(want_m, r0 + x, r0 + y), (q, regions[q], samples, window))
        assert pairs > 0
        assert not got["band"][dropped].any(), "a dropped row has a dosage"
        if text_every:
            for q in valid[::text_every]:
                assert res.region_text(int(q)) == ld_text(parsed, int(q), want_m, window, stat, table_index), (q, regions[q], stat)
        res.close()
        out = got
    return out


@pytest.mark.parametrize("stem", ["x", "x.small"])
def test_golden_region_sweeps(stem, golden_dir, tmp_path):
    fasta, vcf = os.path.join(golden_dir, stem + ".fa"), os.path.join(golden_dir, stem + ".vcf")
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    n_samples = vs.info().num_samples - 1
    rng = np.random.default_rng(11)
    regions = random_regions(rng, _ref_len(fasta), 200)   # unsorted: the device sorts the batch
    parsed, valid = _parse(orc, regions)
    _check_oracle(vs, regions, parsed, valid, None, 64)
    _check_oracle(vs, regions, parsed, valid, None, 3)
    srt = sorted(regions)
    _check_oracle(vs, srt, *_parse(orc, srt), None, 17)
    for sid in range(1, n_samples + 1):
        _check_oracle(vs, regions, parsed, valid, [sid], 16)   # n = 1: every r^2 is 0
    _check_oracle(vs, regions, parsed, valid, [vs.sample_name(1)], 5)   # by name
    for k in range(3):
        ids = rng.choice(np.arange(1, n_samples + 1), size=int(rng.integers(1, n_samples + 1)), replace=False)
        ids = [int(i) for i in ids] + [int(i) for i in ids[:2]]   # duplicates collapse
        _check_oracle(vs, regions, parsed, valid, ids, (2, 64, 256)[k])
    vs.close()


@pytest.mark.parametrize("seed", [701, 702, 703])
def test_random_cohorts_with_duplicate_rule(seed, tmp_path):
    fasta, vcf, names = write_random_cohort(str(tmp_path), seed, ref_len=6000, n_rows=400, n_samples=9, p_near=0.6, p_multi=0.3,
                                            p_same=0.3, unphased_p=0.4 if seed % 2 else 0.05, haploid_p=0.1 if seed == 703 else 0.0)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(seed)
    regions = random_regions(rng, 6000, 300, max_len=900)
    parsed, valid = _parse(orc, regions)
    subsets = [None] + [[vs.sample_id(s) for s in rng.choice(names, size=int(rng.integers(2, len(names))), replace=False)] for _ in range(2)]
    for sub, window in zip(subsets, (64, 7, 256)):
        got = _check_oracle(vs, regions, parsed, valid, sub, window, text_every=6)
        assert np.any(got["rows"]["count_flags"] >> 31), "no region of the batch falls under the duplicate rule"
    vs.close()


# ------------------------------------------------------------------- 2. against the engine's own matrix, every cell of the band
def _check_full(vs, regions, samples, windows, what=None):
    """The whole band, zeros included, of both statistics and every window against D D^T of genotype_matrix() over the same regions
    and samples.  Returns the matrix's arrays."""
    mres = vs.genotype_matrix(regions, samples)
    m = mres.genotype_matrix()
    mres.close()
    cells = np.ascontiguousarray(m["cells"])
    a = cells.shape[0]
    for window in windows:
        want_dot = dot_band(cells, window)
        want_r2, zero = r2_band(cells, window)
        for stat in ("dot", "r2"):
            res = vs.ld_band(regions, samples, window=window, stat=stat)
            got = res.ld_band()
            _shape_checks(got, m["columns"].tolist(), window, stat)
            assert got["band"].shape[0] == a and np.array_equal(got["rows"]["pos"], m["rows"]["pos"])
            assert np.array_equal(got["row_begin"], m["row_begin"]) and np.array_equal(got["row_count"], m["row_count"])
            if stat == "dot":
                bad = np.argwhere(got["band"] != want_dot)
                assert bad.shape[0] == 0, (what, window, a, cells.shape[1], bad[:8].tolist())
            else:
                _r2_close(got["band"], want_r2, zero, (what, window, a, cells.shape[1]))
            assert res.totals()[2] == int(np.count_nonzero(cells))
            res.close()
    return m


def _pitch_cohort(n_cols):   # (num_samples counts the samples of the cohort; info().num_samples adds "ref")
    return VariantStore.synthetic(device=0, ref_length=60_000, num_variants=1500, num_samples=n_cols, seed=900 + n_cols, first_pos=100,
                                  frac_ins=0.06, frac_del=0.06, frac_multi=0.03, max_indel=4, af_exponent=1.0)


def _pitch_regions(vs, rng):
    L = vs.info().ref_length
    starts = rng.integers(1, L - 4000, size=60)
    return [(int(s), int(s) + int(rng.integers(1, 4000))) for s in starts] + [(1, 3000), (L - 2000, L + 5)]


@pytest.mark.parametrize("n_cols,pitch", [(1, 16), (47, 48), (64, 64), (65, 80), (255, 256), (257, 272)])
def test_every_cell_against_the_matrix(n_cols, pitch):
    """The k-step tail in all four residues of 64 and one full chunk plus a remainder, every window class (one column tile more at
    16 -> 17, the 5-tile and the 17-tile kernel), cross-region pairs, the shared / private boundary and the zeros at the table's
    end.  The batch is unsorted: the device sorts it."""
    vs = _pitch_cohort(n_cols)
    rng = np.random.default_rng(n_cols)
    regions = _pitch_regions(vs, rng)
    m = _check_full(vs, regions, None, WINDOWS, n_cols)
    cells = m["cells"]
    a = cells.shape[0]
    assert m["row_pitch"] == pitch and cells.shape[1] == n_cols
    assert a > 3 * 64, "at least three row blocks"
    if n_cols >= 47:   # rows with distinct carrier sets: a transposed tile write would show
        assert np.unique(cells, axis=0).shape[0] > a // 4, (np.unique(cells, axis=0).shape[0], a)
    vs.close()


def test_small_tables_and_windows_beyond_them():
    """Tables of 1, 2, 17, 64 and 65 rows (W > A included), one of three row blocks and a remainder, and an empty one."""
    vs = _pitch_cohort(65)
    L = vs.info().ref_length
    probe = vs.allele_counts([(1, L)])
    pos = np.unique(probe.allele_counts()["rows"]["pos"].astype(np.int64))
    probe.close()
    # regions (pos[k], pos[k + m]) for a sweep of k and m: whatever a row's exact extent, some of them report each wanted number of rows
    spans = [(int(pos[k]), int(pos[k + m])) for m in (0, 1, 2, 15, 16, 17, 62, 63, 64, 65, 66, 200, 210, 220, 230) for k in range(0, 60, 3)]
    cres = vs.allele_counts(spans)
    n_rows = cres.allele_counts()["row_count"].astype(np.int64)
    cres.close()
    blocks = np.nonzero((n_rows > 3 * 64) & (n_rows % 64 != 0))[0]   # at least three row blocks and a remainder
    assert blocks.size
    for want, windows in ((1, (1, 16, 256)), (2, (1, 64)), (17, (16, 17, 256)), (64, (15, 64)), (65, (1, 64, 256)), (int(n_rows[blocks[0]]), (15, 64, 256))):
        hit = np.nonzero(n_rows == want)[0]
        assert hit.size, (want, sorted(set(n_rows.tolist())))
        m = _check_full(vs, [spans[int(hit[0])]], None, windows, want)   # (W > A included)
        assert m["cells"].shape[0] == want
    first = int(pos[0])
    assert first > 2
    for stat in ("dot", "r2"):   # a table without rows
        res = vs.ld_band([(1, first - 2)], window=16, stat=stat)
        got = res.ld_band()
        assert got["band"].shape == (0, 16) and got["counts"].shape == (0,) and got["rows"].shape == (0,)
        assert res.region_ld(0) == [] and res.totals()[1:3] == (0, 0)
        pb, pc, na, nc, w, st = res.ld_band_device()
        assert (na, nc, w, st) == (0, 65, 16, stat)
        res.close()
    # a subset of the columns, a sorted batch
    rng = np.random.default_rng(8)
    sub = [int(i) for i in rng.choice(np.arange(1, 66), size=23, replace=False)]
    _check_full(vs, sorted(_pitch_regions(vs, rng)), sub + sub[:3], (16, 100), "subset")
    vs.close()


# ------------------------------------------------------------------------------------------------------ 3. the storage forms
@pytest.mark.parametrize("list_max", [0, 3, 64])
def test_listed_and_dense_classes(list_max, monkeypatch):
    monkeypatch.setenv("VS_LIST_MAX", str(list_max))
    vs = VariantStore.synthetic(device=0, ref_length=60_000, num_variants=1500, num_samples=150, seed=650, first_pos=100,
                                frac_ins=0.06, frac_del=0.06, frac_multi=0.03, max_indel=4, af_exponent=2.5)
    assert vs.info().list_max == list_max
    rng = np.random.default_rng(list_max)
    regions = _pitch_regions(vs, rng)
    if list_max * 4 < 150:
        cc = vs.get_var_in_ref(regions).view(False)["car_count"]
        assert (cc > list_max).sum() > 20, "the row path must be exercised"
    subset = [int(i) for i in rng.choice(np.arange(1, 150), size=50, replace=False)]
    _check_full(vs, regions, None, (64,), list_max)
    _check_full(vs, regions, subset, (17,), list_max)
    vs.close()


def test_explicit_ids_many_columns():
    """An explicit-id cohort above 4,032 samples: several column tiles of the matrix kernel, a long k loop of the band kernel."""
    vs = VariantStore.synthetic(device=0, ref_length=100_000, num_variants=400, num_samples=4_300, seed=9, first_pos=2_000, frac_ins=0.05,
                                frac_del=0.05, frac_multi=0.01, max_indel=6, af_exponent=2.0, max_af=0.002)
    info = vs.info()
    assert not info.use_bit_vector and info.num_samples - 1 > 4_096
    regions = [(1, 40_000), (30_000, 70_000), (60_000, 100_000), (2_500, 2_600)]
    m = _check_full(vs, regions, None, (16, 256), "explicit")
    assert m["cells"][:, 4_096:].any(), "no column beyond the matrix kernel's first tile is set"
    assert m["cells"].shape[0] > 200
    vs.close()


# -------------------------------------------------------------------------------- 4 .. 7: one larger cohort, shared by the tests
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


def test_counts_are_the_count_query_rows(t6_store):
    vs, regions = t6_store
    for sub in (None, [2, 3, 150, 151, 299]):
        res = vs.ld_band(regions[:2_000], sub, window=16, stat="r2")
        got = res.ld_band()
        cres = vs.allele_counts(regions[:2_000], sub)
        ac = cres.allele_counts()
        assert np.array_equal(ac["rows"]["pos"], got["rows"]["pos"]) and got["counts"].shape[0] > 2_000
        for f in ("carriers", "alt_alleles", "hom_alt", "phased"):
            assert np.array_equal(got["counts"][f], ac["counts"][f]), (sub, f)
        assert got["counts"]["alt_alleles"].any()
        lay = res.layout()
        assert lay[1] == got["band"].shape[0] and lay[2] == 0 and lay[3] == 0 and res.fill_ms() > 0
        assert res.totals()[:2] == cres.totals()[:2]
        res.close(); cres.close()


def test_band_buffer_from_the_pool():
    """A large batch is closed, then a small one on the same handle takes its band's buffer: every cell must be written, the zeros of
    monomorphic pairs and of the table's end included."""
    vs = VariantStore.synthetic(device=0, **T6_KW)
    rng = np.random.default_rng(4)
    s = np.sort(rng.integers(1_000, 7_990_000, size=1_500))
    regions = np.stack([s, s + rng.integers(50, 3_000, size=1_500)], axis=1).astype(np.uint64)
    for stat in ("r2", "dot"):
        big = vs.ld_band(regions, window=64, stat=stat)
        assert np.count_nonzero(big.ld_band()["band"]) > 10_000
        big.close()
        _check_full(vs, np.ascontiguousarray(regions[:40]), [5, 9, 11, 200, 250], (64,), "pool")
        _check_full(vs, np.ascontiguousarray(regions[:3]), None, (64,), "pool")
    vs.close()


def test_temporary_matrix_leaves_an_open_result():
    """The temporary genotype matrix is not part of the result: once a result has been read (its kernels have finished) the matrix
    is back in the handle's pool while the result is still open, and a second whole-cohort batch beside it takes that buffer.
    3,000 columns: the matrix (rows x 3,008 bytes) is far larger than any other buffer of the batch, so nothing else in the pool
    can stand in for it.  Three single-sample batches open side by side first leave the pool every small buffer two more take."""
    vs = VariantStore.synthetic(device=0, ref_length=60_000, num_variants=1500, num_samples=3_000, seed=77, first_pos=100, frac_ins=0.06,
                                frac_del=0.06, frac_multi=0.03, max_indel=4, af_exponent=2.5)
    regions = [(1, 30_000), (20_000, 60_000), (100, 200)]
    warm = [vs.ld_band(regions, [1], window=1) for _ in range(3)]
    for w in warm:
        w.ld_band()
        w.close()
    m0 = vs.info().pool_mallocs
    first = vs.ld_band(regions, window=1)
    got = first.ld_band()   # (waits for the batch)
    a = got["band"].shape[0]
    assert a >= 1500 and vs.info().pool_mallocs > m0, "the whole-cohort matrix must have been a new buffer"
    m1 = vs.info().pool_mallocs
    second = vs.ld_band(regions, window=1, stat="dot")   # beside the open result
    dot = second.ld_band()
    assert vs.info().pool_mallocs == m1, "the open result still holds its temporary matrix"
    # both results are whole and their own: the second batch ran in the first's matrix buffer, not in anything the first still reads
    mres = vs.genotype_matrix(regions)
    cells = np.ascontiguousarray(mres.genotype_matrix()["cells"])
    mres.close()
    assert np.array_equal(dot["band"], dot_band(cells, 1))
    want, zero = r2_band(cells, 1)
    _r2_close(first.ld_band()["band"], want, zero)
    pb, pc, na, nc, w, st = first.ld_band_device()
    assert (na, nc, w, st) == (a, 3_000, 1, "r2")
    first.close(); second.close()
    vs.close()


def test_interleaving_leaves_type6_alone():
    rng = np.random.default_rng(12)
    batches = []
    for k in range(6):
        n = 3_000 + 200 * k + (4_000 if k == 4 else 0)   # like batches (speculated), one larger (refused / re-sized)
        s = np.sort(rng.integers(1_000, 7_990_000, size=n))
        batches.append(np.stack([s, s + rng.integers(50, 3_000, size=n)], axis=1).astype(np.uint64))
    shuffled = batches[3][rng.permutation(batches[3].shape[0])]

    def run(with_ld):
        vs = VariantStore.synthetic(device=0, **T6_KW)
        digests = []
        for k, b in enumerate(batches):
            r = vs.get_var_in_ref(b)
            if with_ld:   # LD batches in between: sorted, unsorted, with a subset
                l1 = vs.ld_band(b, window=16, stat="r2")
                l2 = vs.ld_band(shuffled, window=64, stat="dot")
                l3 = vs.ld_band(shuffled, [1, 5, 7, 200], window=100)
                for ld in (l1, l2, l3):
                    ld.totals()
                    ld.close()
            digests.append(r.digest())
            r.close()
        info = vs.info()
        out = (digests, info.t6_speculated, info.t6_refused)
        vs.close()
        return out

    plain, mixed = run(False), run(True)
    assert plain[1] > 0, "the type-6 batches were not speculated"
    assert plain == mixed


def _read_device(torch, ptr, n):
    """(n,) 32-bit words in device memory, read through the matrix tests' helper as n x 4 bytes."""
    return _read_device_bytes(torch, ptr, n, 4).view(np.uint32).reshape(n).copy()


def test_device_regions_and_device_pointers(t6_store):
    torch = pytest.importorskip("torch")
    vs, regions = t6_store
    sub = [3, 17, 40, 200]
    batch = np.ascontiguousarray(regions[:2_500])
    for stat, dtype in (("dot", np.int32), ("r2", np.float32)):
        host = vs.ld_band(batch, sub, window=32, stat=stat)
        hgot = host.ld_band()
        t = torch.from_numpy(batch.astype(np.int64)).cuda()
        torch.cuda.synchronize()
        dev = vs.ld_band(DeviceArray(t.data_ptr(), batch.shape[0]), sub, window=32, stat=stat)
        dgot = dev.ld_band()
        for k in ("columns", "row_begin", "row_count", "counts"):
            assert np.array_equal(hgot[k], dgot[k]), k
        assert np.array_equal(hgot["band"].view(np.uint32), dgot["band"].view(np.uint32)) and hgot["band"].any()
        pb, pc, a, c, w, st = dev.ld_band_device()
        assert (a, c, w, st) == (hgot["band"].shape[0], 4, 32, stat) and pb and pc
        first = _read_device(torch, pb, a * w)
        later = vs.ld_band(regions[2_500:2_900], window=8)   # a later batch on the same handle leaves the band alone
        later.totals()
        assert np.array_equal(first.view(dtype).reshape(a, w).view(np.uint32), dgot["band"].view(np.uint32))
        assert np.array_equal(_read_device(torch, pb, a * w), first)
        assert np.array_equal(_read_device(torch, pc, a * 4).reshape(a, 4), dgot["counts"].view(np.uint32).reshape(a, 4))
        later.close(); host.close(); dev.close()


def test_size_limit(t6_store):
    vs, regions = t6_store
    warm = vs.allele_counts(regions)   # the plan's temporaries, the table and the counts of this batch are in the handle's pool afterwards
    a = warm.allele_counts()["rows"].shape[0]
    warm.close()
    c = vs.info().num_samples - 1
    pitch = (c + 15) // 16 * 16
    matrix_bytes, band_bytes = a * pitch, a * 4 * 256
    assert matrix_bytes > 1 << 20
    vs.set_option("matrix_max_mib", 1)
    try:
        before = vs.info().pool_mallocs
        with pytest.raises(VariantStoreError) as e:
            vs.ld_band(regions, window=256)
        assert e.value.code == VS_ERR_ARG
        msg = str(e.value)
        for number in (a, c, matrix_bytes + band_bytes, matrix_bytes, band_bytes):
            assert str(number) in msg, (number, msg)
        assert "window 256" in msg and "matrix_max_mib" in msg, msg
        assert vs.info().pool_mallocs == before, "the refused batch allocated"
        few = vs.ld_band(regions[:20], [1, 2, 3], window=2)   # (16 + 8) bytes a row: below the limit
        assert few.ld_band()["band"].shape[1] == 2
        few.close()
        if a * 16 <= 1 << 20 < a * (16 + 4 * 256):   # the band counts: the matrix alone would fit
            with pytest.raises(VariantStoreError) as e:
                vs.ld_band(regions, [1, 2, 3], window=256)
            assert e.value.code == VS_ERR_ARG
        before = vs.info().pool_mallocs
    finally:
        vs.set_option("matrix_max_mib", 0)
    again = vs.ld_band(regions, window=256)   # (matrix and band are larger than anything this handle has allocated so far)
    assert again.ld_band()["band"].shape == (a, 256)
    assert vs.info().pool_mallocs > before
    again.close()


def test_refused_accessors(t6_store):
    vs, regions = t6_store
    r = vs.ld_band(regions[:1_000], window=8)
    for call in (lambda: r.raw(with_carriers=True), lambda: r.view(with_carriers=True), r.digest, r.num_header_records,
                 r.num_region_records):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_UNSUPPORTED
    for call in (r.allele_counts, r.sample_burden, r.sample_burden_device, r.genotype_matrix, r.genotype_matrix_device):
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
    assert r.totals()[:2] == t6.totals()[:2]
    r.close()
    for res in (t6, vs.allele_counts(regions[:10]), vs.sample_burden(regions[:10]), vs.genotype_matrix(regions[:10])):
        with pytest.raises(VariantStoreError) as e:
            res.ld_band()   # not an LD result
        assert e.value.code == VS_ERR_ARG
        with pytest.raises(VariantStoreError) as e:
            res.ld_band_device()
        assert e.value.code == VS_ERR_ARG
        res.close()


# ------------------------------------------------------------------------------------------------------------- 8. the CLI
def test_cli_ld(golden_dir, tmp_path):
    exe = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    subprocess.run([exe, "construct", "-r", os.path.join(golden_dir, "x.fa"), "-v", os.path.join(golden_dir, "x.vcf"), "-p", prefix],
                   check=True, capture_output=True)
    vs = VariantStore.open(prefix, device=0)
    rng = np.random.default_rng(2)
    regions = sorted(random_regions(rng, _ref_len(os.path.join(golden_dir, "x.fa")), 80))
    regions = [(x, y) for x, y in regions if x >= 1]
    rfile = os.path.join(tmp_path, "regions.txt")
    with open(rfile, "w") as f:
        f.write("".join(f"{x}:{y}\n" for x, y in regions))
    names = [vs.sample_name(i) for i in range(1, min(3, vs.info().num_samples))]
    sfile = os.path.join(tmp_path, "samples.txt")
    with open(sfile, "w") as f:
        f.write("\n".join(names) + "\n")
    some = False
    for samples, extra in ((None, []), (names, ["-S", sfile])):
        for stat, window, flags in (("r2", 64, []), ("dot", 64, ["--dot"]), ("r2", 3, ["-w", "3"]), ("dot", 5, ["--dot", "-w", "5"])):
            out = os.path.join(tmp_path, "ld.txt")
            subprocess.run([exe, "ld", "-p", prefix, "-r", "@" + rfile, "-o", out] + extra + flags, check=True, capture_output=True)
            with open(out, "rb") as f:
                parts = f.read().decode("latin-1").split("#region ")[1:]
            res = vs.ld_band(regions, samples, window=window, stat=stat)
            assert len(parts) == len(regions)
            for q, part in enumerate(parts):
                head, text = part.split("\n", 1)
                assert head == f"{q} {regions[q][0]}:{regions[q][1]}"
                assert text == res.region_text(q), (q, stat, window)
                some |= text.count("\n") > 1
            pairs = res.region_ld(int(np.argmax([p.count("\n") for p in parts])))
            assert pairs and all(len(p["a"]) == 3 and len(p["b"]) == 3 for p in pairs)
            res.close()
    assert some
    p = subprocess.run([exe, "ld", "-p", prefix, "-r", "@" + rfile, "-w", "300"], capture_output=True, text=True)
    assert p.returncode != 0
    vs.close()
