"""LD-matrix queries on the GPU (vs_query_ld_matrix): every cell of every block against D D^T of the engine's own genotype matrix (all
tile edges of the 64-row panels, every pitch residue of the k loop), ragged batches whose cells come from the pool, the band query's
cells bit for bit, the oracle's type-6 text, the count records, the temporary matrix, interleaving with type-6 batches, regions in
device memory, the device pointers, the size limit, the refused accessors and the CLI.

DOT is compared bit for bit.  R2 is compared with the band tests' rtol = 2**-22 and atol = 0, and must be exactly 0 where the
reference's vx * vy is 0 (test_gpu_ld_band._r2_close)."""
import os
import subprocess

import numpy as np
import pytest

from genotype_matrix_ref import Parsed, matrix
from helpers import oracle_texts, random_regions, write_random_cohort
from ld_matrix_ref import block, block_begin, block_r2, ld_matrix_text
from oracle.oracle import Oracle
from test_gpu_ld_band import RTOL, T6_KW, _pitch_cohort, _r2_close, _read_device
from variantstore_amd import DeviceArray, VariantStore
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_ARG, VS_ERR_UNSUPPORTED = -5, -7
assert RTOL == 2.0 ** -22
TILE_EDGES = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 193)


def _engine_matrix(vs, regions, samples=None):
    mres = vs.genotype_matrix(regions, samples)
    m = mres.genotype_matrix()
    mres.close()
    return m


def _check_result(got, m, stat, what=None):
    """An ld_matrix() dict against the genotype matrix `m` of the same regions and samples: shapes, block_begin, every cell of every
    block, the symmetry and the diagonal.  Returns the number of cells."""
    cells = np.ascontiguousarray(m["cells"])
    nq = m["row_count"].shape[0]
    assert got["stat"] == stat and got["col_ids"].dtype == np.uint32 and got["col_ids"].tolist() == m["columns"].tolist()
    assert np.array_equal(got["row_begin"], m["row_begin"]) and np.array_equal(got["row_count"], m["row_count"])
    assert np.array_equal(got["rows"]["pos"], m["rows"]["pos"]) and got["counts"].shape == (cells.shape[0],)
    bb = block_begin(m["row_count"])
    assert got["block_begin"].dtype == np.uint64 and np.array_equal(got["block_begin"], bb), what
    assert got["cells"].dtype == (np.int32 if stat == "dot" else np.float32) and got["cells"].shape == (int(bb[nq]),)
    sxx = got["counts"]["alt_alleles"].astype(np.int64) + 2 * got["counts"]["hom_alt"].astype(np.int64)
    for q in range(nq):
        r0, mq = int(m["row_begin"][q]), int(m["row_count"][q])
        mine = got["cells"][int(bb[q]):int(bb[q + 1])].reshape(mq, mq)
        sub = cells[r0:r0 + mq]
        if stat == "dot":
            bad = np.argwhere(mine != block(sub, "dot"))
            assert bad.shape[0] == 0, (what, q, mq, cells.shape[1], bad[:8].tolist())
            assert np.array_equal(np.diag(mine), sxx[r0:r0 + mq]), (what, q)   # the diagonal is Sxx
        else:
            want, zero = block_r2(sub)
            _r2_close(mine, want, zero, (what, q, mq, cells.shape[1]))
            flat = np.diag(zero)
            assert np.array_equal(np.diag(mine), np.where(flat, np.float32(0), np.float32(1))), (what, q)   # exactly 1.0f or 0.0f
        assert np.array_equal(mine.view(np.uint32), mine.T.view(np.uint32)), (what, q)
    return int(bb[nq])


def _check_blocks(vs, regions, samples=None, what=None):
    """Both statistics of a batch against the engine's own matrix.  Returns (the matrix's arrays, {stat: copy of the cells})."""
    m = _engine_matrix(vs, regions, samples)
    out = {}
    for stat in ("dot", "r2"):
        res = vs.ld_matrix(regions, samples, stat=stat)
        got = res.ld_matrix()
        _check_result(got, m, stat, what)
        for q in range(len(regions)):
            v = res.region_ld_matrix(q)
            mq = int(m["row_count"][q])
            assert v.shape == (mq, mq)
            if mq:
                assert np.shares_memory(v, got["cells"]) and np.array_equal(v.view(np.uint32), got["cells"][int(got["block_begin"][q]):int(got["block_begin"][q + 1])].reshape(mq, mq).view(np.uint32))
        assert res.totals()[2] == int(np.count_nonzero(m["cells"]))
        out[stat] = got["cells"].copy()
        res.close()
    return m, out


def _spans_by_rows(vs, wanted):
    """{rows: a region that reports exactly that many table rows} for every wanted count, from a sweep of (pos[k], pos[k + m])."""
    L = vs.info().ref_length
    probe = vs.allele_counts([(1, L)])
    pos = np.unique(probe.allele_counts()["rows"]["pos"].astype(np.int64))
    probe.close()
    spans = [(int(pos[k]), int(pos[k + w - 1 + d])) for w in wanted if w for d in range(-(w // 8) - 2, 3) for k in range(0, 40, 3) if w - 1 + d >= 0]
    cres = vs.allele_counts(spans)
    n_rows = cres.allele_counts()["row_count"].astype(np.int64)
    cres.close()
    out = {}
    for w in wanted:
        if w == 0:
            assert int(pos[0]) > 2
            out[0] = (1, int(pos[0]) - 2)
            continue
        hit = np.nonzero(n_rows == w)[0]
        assert hit.size, (w, sorted(set(n_rows.tolist())))
        out[w] = spans[int(hit[0])]
    out["long"] = (int(pos[2]), int(pos[382]))   # some 400 rows: pairs further apart than the band's widest window
    return out


@pytest.fixture(scope="module")
def edge_store():
    vs = _pitch_cohort(65)
    spans = _spans_by_rows(vs, TILE_EDGES)
    yield vs, spans
    vs.close()


# ---------------------------------------------------------------------------------------------------- 1. tile and pitch edges
@pytest.mark.parametrize("rows", TILE_EDGES)
def test_tile_edges(edge_store, rows):
    """One region of 0 .. 193 rows: one to four 64-row tiles, with 129 and 193 the off-diagonal pairs that are not neighbours."""
    vs, spans = edge_store
    m, _ = _check_blocks(vs, [spans[rows]], None, rows)
    assert m["cells"].shape[0] == rows
    if rows >= 63:   # rows with distinct carrier sets: a transposed tile write would show
        assert np.unique(m["cells"], axis=0).shape[0] > rows // 4
    if rows == 0:
        res = vs.ld_matrix([spans[0]])
        assert res.region_text(0) == "Pos\tRef\tAlt\n" and res.totals()[1:3] == (0, 0)
        pcells, pbb, pcounts, nq, na, nc, st = res.ld_matrix_device()
        assert (nq, na, nc, st) == (1, 0, 65, "r2") and pbb
        res.close()


@pytest.mark.parametrize("n_cols,pitch", [(1, 16), (47, 48), (64, 64), (65, 80), (255, 256), (257, 272)])
def test_pitch_and_chunk_edges(n_cols, pitch):
    """The k-step tail in all four residues of 64 and one full 256-byte chunk plus a remainder, at two tiles and a remainder."""
    vs = _pitch_cohort(n_cols)
    spans = _spans_by_rows(vs, (70, 9))
    m, _ = _check_blocks(vs, [spans[70], spans[9]], None, n_cols)
    assert m["row_pitch"] == pitch and m["cells"].shape[1] == n_cols and m["row_count"].tolist() == [70, 9]
    sub = [int(i) for i in np.random.default_rng(n_cols).choice(np.arange(1, n_cols + 1), size=max(1, n_cols // 3), replace=False)]
    _check_blocks(vs, [spans[70]], sub + sub[:2], ("subset", n_cols))
    vs.close()


# ------------------------------------------------------------------------------------------------------------ 2. ragged batches
def _ragged(spans):
    x129, y129 = spans[129]
    return [spans[193], spans[0], spans[1], spans[17], spans[129], (x129 + 40, y129 + 300), spans[65], spans[65], spans[0], spans[15]]


def test_ragged_batch_from_the_pool(edge_store):
    """Empty, 1-row, sub-tile and multi-tile regions, two that overlap and two identical ones in one unsorted batch (the device sorts
    it): block_begin is the scan, every block is the single-region answer, and nothing bleeds -- with the cells in a buffer that a
    larger, freed result has left in the pool."""
    vs, spans = edge_store
    regions = _ragged(spans)
    single = {}
    for stat in ("dot", "r2"):
        for reg in set(regions):
            res = vs.ld_matrix([reg], stat=stat)
            single[stat, reg] = res.ld_matrix()["cells"].copy()
            res.close()
    for stat in ("r2", "dot"):
        big = vs.ld_matrix(regions + [spans[64]], stat=stat)   # a little larger: its cells' buffer is the best fit afterwards
        assert np.count_nonzero(big.ld_matrix()["cells"]) > 10_000
        big.close()
        before = vs.info().pool_mallocs
        res = vs.ld_matrix(regions, stat=stat)
        got = res.ld_matrix()
        assert vs.info().pool_mallocs == before, "the cells were not taken from the pool"
        mq = got["row_count"].astype(np.int64)
        assert mq.tolist()[:5] == [193, 0, 1, 17, 129] and mq[6] == mq[7] == 65 and mq[8] == 0 and mq[9] == 15 and mq[5] > 64
        assert np.array_equal(got["block_begin"], block_begin(mq))
        for q, reg in enumerate(regions):
            mine = got["cells"][int(got["block_begin"][q]):int(got["block_begin"][q + 1])]
            assert np.array_equal(mine.view(np.uint32), single[stat, reg].view(np.uint32)), (stat, q, reg)
        res.close()
    _check_blocks(vs, regions, [3, 4, 9, 33, 60], "ragged subset")   # monomorphic rows under a subset: zeros that must be written


def test_against_the_band(edge_store):
    """block[a, b] with 1 <= b - a <= 256 is the band query's cell of the same pair, bit for bit: one formula from the same integers."""
    vs, spans = edge_store
    regions = _ragged(spans) + [spans["long"]]
    for samples in (None, [2, 5, 7, 11, 40, 41, 64]):
        for stat in ("dot", "r2"):
            res = vs.ld_matrix(regions, samples, stat=stat)
            got = res.ld_matrix()
            bres = vs.ld_band(regions, samples, window=256, stat=stat)
            band = bres.ld_band()["band"]
            bres.close()
            pairs = 0
            for q in range(len(regions)):
                r0, mq = int(got["row_begin"][q]), int(got["row_count"][q])
                mine = res.region_ld_matrix(q)
                a, b = np.nonzero((np.arange(mq)[None, :] - np.arange(mq)[:, None] >= 1) & (np.arange(mq)[None, :] - np.arange(mq)[:, None] <= 256))
                assert np.array_equal(mine[a, b].view(np.uint32), band[r0 + a, b - a - 1].view(np.uint32)), (samples, stat, q)
                assert np.array_equal(mine.view(np.uint32), mine.T.view(np.uint32))
                pairs += a.shape[0]
            assert pairs > 90_000 and got["row_count"].max() > 350
            res.close()


def test_identical_calls_give_identical_bytes(edge_store):
    vs, spans = edge_store
    regions = _ragged(spans)
    for stat in ("dot", "r2"):
        a, b = vs.ld_matrix(regions, stat=stat), vs.ld_matrix(regions, stat=stat)
        ga, gb = a.ld_matrix(), b.ld_matrix()
        assert ga["cells"].any() and np.array_equal(ga["cells"].view(np.uint32), gb["cells"].view(np.uint32))
        assert np.array_equal(ga["block_begin"], gb["block_begin"]) and np.array_equal(ga["counts"], gb["counts"])
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------- 3. against the oracle
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


def _check_oracle(vs, regions, parsed, valid, samples, text_every=1):
    """Every block without its dropped rows against the block of the oracle's rows, the dropped rows' cells zero, and the text."""
    ids = (list(range(1, vs.info().num_samples)) if samples is None
           else sorted({vs.sample_id(i) if isinstance(i, str) else int(i) for i in samples}))
    want_m = matrix(parsed, [vs.sample_name(i) for i in ids])
    any_dropped = False
    for stat in ("dot", "r2"):
        res = vs.ld_matrix(regions, samples, stat=stat)
        got = res.ld_matrix()
        assert got["col_ids"].tolist() == ids and got["stat"] == stat
        dropped = (got["rows"]["count_flags"] >> 31) != 0
        any_dropped |= bool(dropped.any())
        cells = 0
        for q in valid:
            r0, mq = int(got["row_begin"][q]), int(got["row_count"][q])
            mine = res.region_ld_matrix(int(q))
            drop = dropped[r0:r0 + mq]
            assert not mine[drop].any() and not mine[:, drop].any(), "a dropped row has a dosage"
            kept = mine[~drop][:, ~drop]
            p0, n = int(parsed.row_begin[q]), int(parsed.row_count[q])
            assert kept.shape == (n, n), (q, regions[q])
            sub = want_m[p0:p0 + n]
            if stat == "dot":
                assert np.array_equal(kept, block(sub, "dot")), (q, regions[q], samples)
            else:
                _r2_close(np.ascontiguousarray(kept), *block_r2(sub), (q, regions[q], samples))
            cells += n * n
        assert cells > 0
        if text_every:
            for q in valid[::text_every]:
                assert res.region_text(int(q)) == ld_matrix_text(parsed, int(q), want_m, stat), (q, regions[q], stat)
        res.close()
    return any_dropped


@pytest.mark.parametrize("stem", ["x", "x.small"])
def test_golden_region_sweeps(stem, golden_dir, tmp_path):
    fasta, vcf = os.path.join(golden_dir, stem + ".fa"), os.path.join(golden_dir, stem + ".vcf")
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    n_samples = vs.info().num_samples - 1
    rng = np.random.default_rng(11)
    regions = random_regions(rng, _ref_len(fasta), 200)   # unsorted: the device sorts the batch
    parsed, valid = _parse(orc, regions)
    _check_oracle(vs, regions, parsed, valid, None)
    srt = sorted(regions)
    _check_oracle(vs, srt, *_parse(orc, srt), None, text_every=3)
    _check_oracle(vs, regions, parsed, valid, [1], text_every=5)   # n = 1: every r^2 is 0
    _check_oracle(vs, regions, parsed, valid, [vs.sample_name(n_samples)], text_every=5)   # by name
    for k in range(2):
        ids = rng.choice(np.arange(1, n_samples + 1), size=int(rng.integers(1, n_samples + 1)), replace=False)
        ids = [int(i) for i in ids] + [int(i) for i in ids[:2]]   # duplicates collapse
        _check_oracle(vs, regions, parsed, valid, ids, text_every=4)
    vs.close()


@pytest.mark.parametrize("seed", [711, 712])
def test_random_cohorts_with_duplicate_rule(seed, tmp_path):
    fasta, vcf, names = write_random_cohort(str(tmp_path), seed, ref_len=6000, n_rows=400, n_samples=9, p_near=0.6, p_multi=0.3,
                                            p_same=0.3, unphased_p=0.4 if seed % 2 else 0.05, haploid_p=0.1 if seed == 712 else 0.0)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(seed)
    regions = random_regions(rng, 6000, 300, max_len=900)
    parsed, valid = _parse(orc, regions)
    subsets = [None] + [[vs.sample_id(s) for s in rng.choice(names, size=int(rng.integers(2, len(names))), replace=False)] for _ in range(2)]
    for sub in subsets:
        assert _check_oracle(vs, regions, parsed, valid, sub, text_every=6), "no region of the batch falls under the duplicate rule"
    vs.close()


# -------------------------------------------------------------------------------- 4 .. 7: one larger cohort, shared by the tests
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
        res = vs.ld_matrix(regions[:2_000], sub, stat="r2")
        got = res.ld_matrix()
        cres = vs.allele_counts(regions[:2_000], sub)
        ac = cres.allele_counts()
        assert np.array_equal(ac["rows"]["pos"], got["rows"]["pos"]) and got["counts"].shape[0] > 2_000
        for f in ("carriers", "alt_alleles", "hom_alt", "phased"):
            assert np.array_equal(got["counts"][f], ac["counts"][f]), (sub, f)
        assert got["counts"]["alt_alleles"].any()
        lay = res.layout()
        assert lay[1] == got["rows"].shape[0] and lay[2] == 0 and lay[3] == 0 and res.fill_ms() > 0
        assert res.totals()[:2] == cres.totals()[:2]
        assert np.array_equal(got["block_begin"], block_begin(got["row_count"]))
        res.close(); cres.close()


def test_temporary_matrix_leaves_an_open_result():
    """The temporary genotype matrix is not part of the result: once a result has been read (its kernels have finished) the matrix
    is back in the handle's pool while the result is still open, and a second whole-cohort batch beside it takes that buffer.
    3,000 columns and 150 regions of about ten rows: the matrix (rows x 3,008 bytes) is far larger than any other buffer of the
    batch -- the cells are some tens of KiB --, so nothing else in the pool can stand in for it.  Three single-sample batches open
    side by side first leave the pool every small buffer two more take."""
    vs = VariantStore.synthetic(device=0, ref_length=60_000, num_variants=1500, num_samples=3_000, seed=77, first_pos=100, frac_ins=0.06,
                                frac_del=0.06, frac_multi=0.03, max_indel=4, af_exponent=2.5)
    regions = [(1 + 400 * k, 400 * (k + 1)) for k in range(150)]
    warm = [vs.ld_matrix(regions, [1]) for _ in range(3)]
    for w in warm:
        w.ld_matrix()
        w.close()
    m0 = vs.info().pool_mallocs
    first = vs.ld_matrix(regions)
    got = first.ld_matrix()   # (waits for the batch)
    a = got["rows"].shape[0]
    assert a >= 1400 and got["cells"].nbytes < 1 << 20 and vs.info().pool_mallocs > m0, "the whole-cohort matrix must have been a new buffer"
    m1 = vs.info().pool_mallocs
    second = vs.ld_matrix(regions, stat="dot")   # beside the open result
    dot = second.ld_matrix()
    assert vs.info().pool_mallocs == m1, "the open result still holds its temporary matrix"
    # both results are whole and their own: the second batch ran in the first's matrix buffer, not in anything the first still reads
    m = _engine_matrix(vs, regions)
    _check_result(dot, m, "dot")
    _check_result(first.ld_matrix(), m, "r2")
    pcells, pbb, pcounts, nq, na, nc, st = first.ld_matrix_device()
    assert (nq, na, nc, st) == (150, a, 3_000, "r2") and pcells and pbb and pcounts
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
            if with_ld:   # LD-matrix batches in between: sorted, unsorted, with a subset
                l1 = vs.ld_matrix(b, stat="r2")
                l2 = vs.ld_matrix(shuffled, stat="dot")
                l3 = vs.ld_matrix(shuffled, [1, 5, 7, 200])
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


def test_device_regions_and_device_pointers(t6_store):
    """Regions in device memory and the device accessor.  Sample ids in device memory are accepted by neither LD query: the C ABI
    builds the subset's mask and ranks from them on the host (sample_columns), and VariantStore.ld_matrix takes `samples` through
    _sample_set exactly as ld_band does -- so the ids here are a host list, as in the band's test of the same name."""
    torch = pytest.importorskip("torch")
    vs, regions = t6_store
    sub = [3, 17, 40, 200]
    batch = np.ascontiguousarray(regions[:2_500])
    for stat, dtype in (("dot", np.int32), ("r2", np.float32)):
        host = vs.ld_matrix(batch, sub, stat=stat)
        hgot = host.ld_matrix()
        t = torch.from_numpy(batch.astype(np.int64)).cuda()
        torch.cuda.synchronize()
        dev = vs.ld_matrix(DeviceArray(t.data_ptr(), batch.shape[0]), sub, stat=stat)
        dgot = dev.ld_matrix()
        for k in ("col_ids", "row_begin", "row_count", "counts", "block_begin"):
            assert np.array_equal(hgot[k], dgot[k]), k
        assert np.array_equal(hgot["cells"].view(np.uint32), dgot["cells"].view(np.uint32)) and hgot["cells"].any()
        pcells, pbb, pcounts, nq, a, c, st = dev.ld_matrix_device()
        total = dgot["cells"].shape[0]
        assert (nq, a, c, st) == (2_500, dgot["rows"].shape[0], 4, stat) and pcells and pbb and pcounts
        first = _read_device(torch, pcells, total)
        later = vs.ld_matrix(regions[2_500:2_900])   # a later batch on the same handle leaves the cells alone
        later.totals()
        assert np.array_equal(first, dgot["cells"].view(np.uint32))
        assert np.array_equal(_read_device(torch, pcells, total), first)
        assert np.array_equal(_read_device(torch, pbb, 2 * (nq + 1)).view(np.uint64), dgot["block_begin"])
        assert np.array_equal(_read_device(torch, pcounts, a * 4).reshape(a, 4), dgot["counts"].view(np.uint32).reshape(a, 4))
        later.close(); host.close(); dev.close()


def test_size_limit(t6_store):
    vs, regions = t6_store
    warm = vs.ld_matrix(regions)   # what the refused batch takes before it is refused -- table, counts, offsets -- is in the handle's pool afterwards
    wgot = warm.ld_matrix()
    a, mq, wcells = wgot["rows"].shape[0], wgot["row_count"].astype(np.int64), wgot["cells"].view(np.uint32).copy()
    warm.close()
    c = vs.info().num_samples - 1
    pitch = (c + 15) // 16 * 16
    matrix_bytes, cell_bytes = a * pitch, 4 * int((mq * mq).sum())
    assert matrix_bytes > 1 << 20
    vs.set_option("matrix_max_mib", 1)
    try:
        before = vs.info().pool_mallocs
        with pytest.raises(VariantStoreError) as e:
            vs.ld_matrix(regions)
        assert e.value.code == VS_ERR_ARG
        msg = str(e.value)
        for what in (f"{regions.shape[0]} regions", f"{a} rows", f"{c} columns", f"largest block {mq.max()} x {mq.max()}",
                     f"{matrix_bytes + cell_bytes} bytes", str(matrix_bytes), str(cell_bytes), "matrix_max_mib"):
            assert what in msg, (what, msg)
        assert vs.info().pool_mallocs == before, "the refused batch allocated"
        few = vs.ld_matrix(regions[:20], [1, 2, 3])   # 16 bytes a row and a few small blocks: below the limit
        assert few.ld_matrix()["block_begin"].shape == (21,)
        few.close()
        if a * 16 <= 1 << 20 < a * 16 + cell_bytes:   # the cells count: the matrix alone would fit
            with pytest.raises(VariantStoreError) as e:
                vs.ld_matrix(regions, [1, 2, 3])
            assert e.value.code == VS_ERR_ARG
    finally:
        vs.set_option("matrix_max_mib", 0)
    again = vs.ld_matrix(regions)   # the handle stays usable
    assert np.array_equal(again.ld_matrix()["cells"].view(np.uint32), wcells) and wcells.any()
    again.close()


def test_refused_accessors(t6_store):
    vs, regions = t6_store
    r = vs.ld_matrix(regions[:1_000])
    for call in (lambda: r.raw(with_carriers=True), lambda: r.view(with_carriers=True), r.digest, r.num_header_records,
                 r.num_region_records):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_UNSUPPORTED
    for call in (r.allele_counts, r.sample_burden, r.sample_burden_device, r.genotype_matrix, r.genotype_matrix_device, r.ld_band,
                 r.ld_band_device):
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
    for res in (t6, vs.allele_counts(regions[:10]), vs.sample_burden(regions[:10]), vs.genotype_matrix(regions[:10]),
                vs.ld_band(regions[:10], window=4)):
        for call in (res.ld_matrix, res.ld_matrix_device, lambda: res.region_ld_matrix(0)):
            with pytest.raises(VariantStoreError) as e:
                call()   # not an LD-matrix result
            assert e.value.code == VS_ERR_ARG
        res.close()


# ------------------------------------------------------------------------------------------------------------- 8. the CLI
def test_cli_ldmatrix(golden_dir, tmp_path):
    exe = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    subprocess.run([exe, "construct", "-r", os.path.join(golden_dir, "x.fa"), "-v", os.path.join(golden_dir, "x.vcf"), "-p", prefix],
                   check=True, capture_output=True)
    vs = VariantStore.open(prefix, device=0)
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(2)
    regions = sorted(random_regions(rng, _ref_len(os.path.join(golden_dir, "x.fa")), 80))
    regions = [(x, y) for x, y in regions if x >= 1]
    parsed, valid = _parse(orc, regions)
    rfile = os.path.join(tmp_path, "regions.txt")
    with open(rfile, "w") as f:
        f.write("".join(f"{x}:{y}\n" for x, y in regions))
    names = [vs.sample_name(i) for i in range(1, min(3, vs.info().num_samples))]
    all_names = [vs.sample_name(i) for i in range(1, vs.info().num_samples)]
    sfile = os.path.join(tmp_path, "samples.txt")
    with open(sfile, "w") as f:
        f.write("\n".join(names) + "\n")
    some = False
    for samples, extra in ((None, []), (names, ["-S", sfile])):
        want_m = matrix(parsed, all_names if samples is None else names)
        for stat, flags in (("r2", []), ("dot", ["--dot"])):
            out = os.path.join(tmp_path, "ldm.txt")
            subprocess.run([exe, "ldmatrix", "-p", prefix, "-r", "@" + rfile, "-o", out] + extra + flags, check=True, capture_output=True)
            with open(out, "rb") as f:
                parts = f.read().decode("latin-1").split("#region ")[1:]
            assert len(parts) == len(regions)
            for q, part in enumerate(parts):
                head, text = part.split("\n", 1)
                assert head == f"{q} {regions[q][0]}:{regions[q][1]}"
                if q in valid:
                    assert text == ld_matrix_text(parsed, q, want_m, stat), (q, stat, samples)
                    some |= text.count("\n") > 2
    assert some
    vs.close()
