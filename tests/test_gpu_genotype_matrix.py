"""Genotype-matrix queries on the GPU (vs_query_genotype_matrix): the table rows x samples byte matrix against what the oracle's
type-6 text gives (carriers by name), against type 6's own carrier lists, the count and the burden query, the duplicate rule, the
list threshold, column tiles, the three storage forms of the genotype bits, the edges of the row blocks, a buffer that comes from
the pool, the device pointer, interleaving with type-6 batches, the size limit, the refused accessors, regions in device memory
and the CLI.  Every comparison with the reference is exact and runs over region q's non-dropped table rows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from genotype_matrix_ref import Parsed, matrix, matrix_sparse, matrix_text
from helpers import oracle_texts, random_regions, write_random_cohort
from oracle.oracle import Oracle
from variantstore_amd import DeviceArray, VariantStore
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_ARG, VS_ERR_UNSUPPORTED = -5, -7


def _oracle(vs, tmp_path, name="plain.bin"):
    plain = os.path.join(tmp_path, name)
    vs.export_plain(plain)
    return Oracle(plain)


def _ref_len(fasta):
    with open(fasta) as f:
        return sum(len(line.strip()) for line in f if not line.startswith(">"))


def _parse(orc, regions):
    """(Parsed texts of the regions the reference terminates on, the numbers of those regions)."""
    want = oracle_texts(orc, regions)
    valid = [q for q, (n, _e, _t) in enumerate(want) if n >= 0]
    assert valid
    return Parsed([t if n >= 0 else None for n, _e, t in want]), np.asarray(valid)


def _columns(vs, samples):
    """(ids, names) of the columns a query over `samples` (ids or names; None: the whole cohort) has."""
    ids = (list(range(1, vs.info().num_samples)) if samples is None
           else sorted({vs.sample_id(i) if isinstance(i, str) else int(i) for i in samples}))
    return ids, [vs.sample_name(i) for i in ids]


def _reported(got, qs):
    """(the table rows the regions qs report, dropped ones left out, region after region; how many each region has)."""
    dropped = (got["rows"]["count_flags"] >> 31) != 0
    idx, cnt = [np.zeros(0, np.int64)], []
    for q in qs:
        a = np.arange(int(got["row_begin"][q]), int(got["row_begin"][q]) + int(got["row_count"][q]))
        a = a[~dropped[a]]
        idx.append(a)
        cnt.append(a.shape[0])
    return np.concatenate(idx), np.asarray(cnt, np.int64)


def _ref_rows(parsed, qs):
    idx = [np.zeros(0, np.int64)] + [np.arange(int(parsed.row_begin[q]), int(parsed.row_begin[q] + parsed.row_count[q])) for q in qs]
    return np.concatenate(idx), parsed.row_count[np.asarray(qs, np.int64)]


def _pitched(got):
    """The whole buffer of a result, padding included: (A, row_pitch)."""
    cells = got["cells"]
    assert cells.shape[0] == 0 or cells.strides == (got["row_pitch"], 1)
    return np.lib.stride_tricks.as_strided(cells, shape=(cells.shape[0], got["row_pitch"]), strides=(got["row_pitch"], 1))


def _shape_checks(got, ids):
    assert got["columns"].dtype == np.uint32 and got["columns"].tolist() == ids
    cells = got["cells"]
    assert cells.dtype == np.uint8 and cells.shape == (got["rows"].shape[0], len(ids))
    assert got["row_pitch"] % 16 == 0 and len(ids) <= got["row_pitch"] < len(ids) + 16
    assert not _pitched(got)[:, len(ids):].any(), "padding bytes are not zero"
    dropped = (got["rows"]["count_flags"] >> 31) != 0
    assert not cells[dropped].any(), "a dropped row has carriers"


def _check(vs, regions, parsed, valid, samples=None, texts=False):
    """The matrix of a query (and every region's text) against the reference helper; returns the result's arrays."""
    ids, names = _columns(vs, samples)
    res = vs.genotype_matrix(regions, samples)
    got = res.genotype_matrix()
    _shape_checks(got, ids)
    want = matrix(parsed, names)
    mine, n_mine = _reported(got, valid)
    ref, n_ref = _ref_rows(parsed, valid)
    assert np.array_equal(n_mine, n_ref), samples
    assert np.array_equal(got["cells"][mine], want[ref]), samples
    if texts:
        for q in valid:
            assert res.region_text(int(q)) == matrix_text(parsed, int(q), want, names), (q, regions[q])
    assert res.totals()[2] == int(np.count_nonzero(got["cells"]))
    res.close()
    return got


@pytest.mark.parametrize("stem", ["x", "x.small"])
def test_golden_region_sweeps(stem, golden_dir, tmp_path):
    fasta, vcf = os.path.join(golden_dir, stem + ".fa"), os.path.join(golden_dir, stem + ".vcf")
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    n_samples = vs.info().num_samples - 1
    rng = np.random.default_rng(11)
    regions = random_regions(rng, _ref_len(fasta), 200)   # unsorted: the device sorts the batch
    parsed, valid = _parse(orc, regions)
    _check(vs, regions, parsed, valid, texts=True)
    srt = sorted(regions)
    _check(vs, srt, *_parse(orc, srt), texts=True)
    for sid in range(1, n_samples + 1):
        _check(vs, regions, parsed, valid, [sid], texts=True)
    _check(vs, regions, parsed, valid, [vs.sample_name(1)], texts=True)   # by name
    for k in range(4):
        ids = rng.choice(np.arange(1, n_samples + 1), size=int(rng.integers(1, n_samples + 1)), replace=False)
        ids = [int(i) for i in ids] + [int(i) for i in ids[:2]]   # duplicates collapse
        _check(vs, regions, parsed, valid, ids, texts=True)
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
    subsets = [None] + [[vs.sample_id(s) for s in rng.choice(names, size=int(rng.integers(1, len(names))), replace=False)] for _ in range(3)]
    for sub in subsets:
        got = _check(vs, regions, parsed, valid, sub, texts=True)   # (dropped rows: all zero -- _shape_checks -- and absent from the text)
        assert np.any(got["rows"]["count_flags"] >> 31), "no region of the batch falls under the duplicate rule"
    vs.close()


def _small_cohort(n_samples):
    return VariantStore.synthetic(device=0, ref_length=60_000, num_variants=1500, num_samples=n_samples, seed=500 + n_samples, first_pos=100,
                                  frac_ins=0.06, frac_del=0.06, frac_multi=0.03, max_indel=4, af_exponent=2.5)


def _small_regions(vs, rng):
    L = vs.info().ref_length
    starts = rng.integers(1, L - 4000, size=60)
    return [(int(s), int(s) + int(rng.integers(1, 4000))) for s in starts] + [(1, 3000), (L - 2000, L + 5)]


@pytest.mark.parametrize("list_max", [0, 3, 64])
@pytest.mark.parametrize("n_samples", [70, 150])
def test_list_threshold(list_max, n_samples, tmp_path, monkeypatch):
    """Small cohorts take the class-row path only under a lowered threshold (VS_LIST_MAX is read when an index is opened): row
    widths of 2 and 3 words, both paths, the whole cohort and a third of it."""
    monkeypatch.setenv("VS_LIST_MAX", str(list_max))
    vs = _small_cohort(n_samples)
    assert vs.info().list_max == list_max
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(list_max * 31 + n_samples)
    regions = _small_regions(vs, rng)
    cc = vs.get_var_in_ref(regions).view(False)["car_count"]
    if list_max * 4 < n_samples:
        assert (cc > list_max).sum() > 20, "the row path must be exercised"
    parsed, valid = _parse(orc, regions)
    subset = [int(i) for i in rng.choice(np.arange(1, n_samples + 1), size=n_samples // 3, replace=False)]
    got = _check(vs, regions, parsed, valid, None, texts=True)
    assert got["row_pitch"] == {70: 80, 150: 160}[n_samples]   # C = 69 and 149
    _check(vs, regions, parsed, valid, subset, texts=True)
    vs.close()


@pytest.mark.parametrize("tile", [16, 64])
def test_column_tiles(tile, tmp_path, monkeypatch):
    """149 columns in tiles of 16 and 64 (tile boundaries inside a row, the last tile partial, lists and class rows) and a subset
    of 17 columns: the matrices of the default tiling (one tile), and the reference's."""
    monkeypatch.setenv("VS_LIST_MAX", "3")
    vs = _small_cohort(150)
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(tile)
    regions = _small_regions(vs, rng)
    parsed, valid = _parse(orc, regions)
    sub17 = [int(i) for i in rng.choice(np.arange(1, 150), size=17, replace=False)]
    subsets = (None, sub17, list(range(1, 150)))
    default = [_check(vs, regions, parsed, valid, sub) for sub in subsets]
    vs.set_option("matrix_tile_cols", tile)
    try:
        for sub, d in zip(subsets, default):
            got = _check(vs, regions, parsed, valid, sub, texts=sub is not None and len(sub) == 17)
            assert np.array_equal(_pitched(got), _pitched(d)), sub
            if got["cells"].shape[1] > 2 * tile:
                assert got["cells"][:, tile:].any(), "no column beyond the first tile is set"
    finally:
        vs.set_option("matrix_tile_cols", 0)
    vs.close()


def _check_sparse(vs, regions, parsed, valid, samples):
    """As _check for matrices too large to build twice: the nonzero cells against the reference's."""
    ids, names = _columns(vs, samples)
    res = vs.genotype_matrix(regions, samples)
    got = res.genotype_matrix()
    _shape_checks(got, ids)
    mine, n_mine = _reported(got, valid)
    ref, n_ref = _ref_rows(parsed, valid)
    assert np.array_equal(n_mine, n_ref)
    place = np.full(parsed.n_rows + 1, -1, np.int64)   # reference row -> its place among the compared rows
    place[ref] = np.arange(ref.shape[0])
    row, col, val = matrix_sparse(parsed, names)
    keep = place[row] >= 0
    sub = got["cells"][mine]
    r_mine, c_mine = np.nonzero(sub)
    assert np.array_equal(r_mine, place[row[keep]]) and np.array_equal(c_mine, col[keep])
    assert np.array_equal(sub[r_mine, c_mine], val[keep])
    assert res.totals()[2] == int(np.count_nonzero(got["cells"]))
    res.close()
    return got


@pytest.mark.parametrize("shape", ["narrow_dense", "wide", "explicit"])
def test_storage_forms(shape, tmp_path):
    """gt_groups with dense rows, gt_nibbles of a 4,100-sample class-row cohort (4,099 columns: a tile boundary inside the row) and
    the unpadded pool of a 10,000-sample explicit-id cohort -- short scattered regions and long overlapping ones, sorted and
    shuffled, the whole cohort and a third of it."""
    kw = dict(ref_length=1_500_000, num_variants=30_000, seed=9, first_pos=2_000, frac_ins=0.05, frac_del=0.05, frac_multi=0.01, max_indel=6)
    if shape == "wide":
        kw.update(num_samples=4_100, af_exponent=3.0)
    elif shape == "explicit":
        kw.update(num_samples=10_000, af_exponent=2.0, max_af=0.0004)
    else:
        kw.update(num_samples=1_500, af_exponent=0.8)
    vs = VariantStore.synthetic(device=0, **kw)
    info = vs.info()
    assert bool(info.use_bit_vector) == (shape != "explicit")
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(6)
    starts = np.sort(rng.integers(3_000, 1_495_000, size=300))
    short = [(int(x), int(x) + 25) for x in starts]
    long_ = sorted((int(x), int(x) + int(rng.integers(5_000, 30_000))) for x in rng.integers(3_000, 1_450_000, size=20))
    ns = info.num_samples - 1
    subset = [int(i) for i in rng.choice(np.arange(1, ns + 1), size=ns // 3, replace=False)]
    for regions in (short, long_):
        parsed, valid = _parse(orc, regions)
        perm = rng.permutation(len(regions))
        shuffled = [regions[i] for i in perm]
        for sub in (None, subset):
            got = _check_sparse(vs, regions, parsed, valid, sub)
            assert got["cells"].nbytes < 120 << 20
            res = vs.genotype_matrix(shuffled, sub)       # the device sorts the batch: every region keeps its rows
            again = res.genotype_matrix()
            a, na = _reported(again, range(len(regions)))
            b, nb = _reported(got, perm)
            assert np.array_equal(na, nb) and np.array_equal(again["cells"][a], got["cells"][b])
            res.close()
            if shape == "wide" and sub is None and regions is long_:
                assert got["cells"].shape[1] == ns > 4_096 and got["cells"][:, 4_096:].any(), "no column beyond the first tile is set"
    vs.close()


T6_KW = dict(ref_length=8_000_000, num_variants=150_000, num_samples=300, seed=5, first_pos=1_000, frac_ins=0.05, frac_del=0.05,
             frac_multi=0.02, max_indel=6, af_exponent=2.0)


@pytest.fixture(scope="module")
def t6_store():
    vs = VariantStore.synthetic(device=0, **T6_KW)
    rng = np.random.default_rng(12)
    s = np.sort(rng.integers(1_000, 7_990_000, size=3_000))
    regions = np.stack([s, s + rng.integers(50, 3_000, size=3_000)], axis=1).astype(np.uint64)
    regions = np.concatenate([regions, np.array([[1, 7_999_000]], np.uint64)])   # a region that reports most of the table
    yield vs, regions
    vs.close()


def _from_type6(vs, regions, n_cols):
    """(uint8 (rows, n_cols) over the whole cohort, rows per region): the rows every region reports, region after region, from
    type 6's own carrier lists -- arena entries sample_id | gt << 13."""
    t6 = vs.get_var_in_ref(regions)
    raw = t6.raw(with_carriers=True)
    assert raw["carrier_bytes"] == 2
    got = {"rows": raw["rows"], "row_begin": raw["row_begin"], "row_count": raw["row_count"]}
    a, n = _reported(got, range(len(regions)))
    cnt = (raw["rows"]["count_flags"][a] & 0x7FFFFFFF).astype(np.int64)
    at = np.repeat(raw["rows"]["car_begin"][a].astype(np.int64), cnt) + np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    w = raw["arena"][at].astype(np.int64)
    out = np.zeros((a.shape[0], n_cols), np.uint8)
    out[np.repeat(np.arange(a.shape[0]), cnt), (w & 0x1FFF) - 1] = 0x08 | (w >> 13)
    t6.close()
    return out, n


def test_against_type6_lists_counts_and_burden(t6_store):
    vs, regions = t6_store
    ns = vs.info().num_samples - 1
    want, n_want = _from_type6(vs, regions, ns)
    assert n_want[-1] > 100_000
    res = vs.genotype_matrix(regions)
    got = res.genotype_matrix()
    _shape_checks(got, list(range(1, ns + 1)))
    cells = got["cells"]
    mine, n_mine = _reported(got, range(len(regions)))
    assert np.array_equal(n_mine, n_want)
    assert np.array_equal(cells[mine], want)
    # the count query's rows: the same table, the sums along a row
    cres = vs.allele_counts(regions)
    ac = cres.allele_counts()
    assert np.array_equal(ac["rows"]["pos"], got["rows"]["pos"]) and np.array_equal(ac["row_count"], got["row_count"])
    counts = ac["counts"]
    assert np.array_equal(np.count_nonzero(cells, axis=1), counts["carriers"])
    assert np.array_equal((((cells >> 1) & 1) + ((cells >> 2) & 1)).sum(axis=1, dtype=np.int64), counts["alt_alleles"])   # sum popc(M & 6)
    assert np.array_equal(((cells & 6) == 6).sum(axis=1), counts["hom_alt"])
    assert np.array_equal((cells & 1).sum(axis=1, dtype=np.int64), counts["phased"])
    assert not (cells[cells != 0] & 0xF0).any() and ((cells[cells != 0] & 0x08) != 0).all()
    assert res.totals()[:2] == cres.totals()[:2]
    assert res.totals()[2] == int(np.count_nonzero(cells))   # (every table row once; the count result adds a row once per region reporting it)
    lay = res.layout()
    assert lay[1] == cells.shape[0] and lay[2] == 0 and lay[3] == 0 and res.fill_ms() > 0
    res.close(); cres.close()
    # a subset: the burden query's cells are the column sums over every region's reported rows
    sub = [2, 3, 150, 151, 299]
    sres = vs.genotype_matrix(regions, sub)
    sgot = sres.genotype_matrix()
    assert np.array_equal(sgot["cells"], cells[:, np.asarray(sub) - 1])
    bres = vs.sample_burden(regions, sub)
    burden = bres.sample_burden()["cells"]
    sc = sgot["cells"]
    for q in (0, 1, 17, 1_500, 2_999, 3_000):
        a, _n = _reported(sgot, [q])
        m = sc[a]
        assert np.array_equal(np.count_nonzero(m, axis=0), burden["variants"][q]), q
        assert np.array_equal((((m >> 1) & 1) + ((m >> 2) & 1)).sum(axis=0, dtype=np.int64), burden["alt_alleles"][q]), q
        assert np.array_equal(((m & 6) == 6).sum(axis=0), burden["hom_alt"][q]), q
        assert np.array_equal((m & 1).sum(axis=0, dtype=np.int64), burden["phased"][q]), q
    assert sres.totals()[2] == int(np.count_nonzero(sc))
    sres.close(); bres.close()
    # regions that share no row: every table row is reported once, and the totals are the count result's
    apart = np.ascontiguousarray(regions[:3_000]).copy()
    apart[:-1, 1] = np.minimum(apart[:-1, 1], np.maximum(apart[1:, 0] - 1, apart[:-1, 0]))
    apart = apart[np.concatenate([apart[1:, 0] > apart[:-1, 0], [True]])]
    assert apart.shape[0] > 2_500
    for s in (None, sub):
        m, c = vs.genotype_matrix(apart, s), vs.allele_counts(apart, s)
        assert m.totals() == c.totals() and m.totals()[2] > 0
        m.close(); c.close()


def test_row_block_edges(t6_store):
    vs, regions = t6_store
    sub = [3, 17, 40, 200]
    batch = np.ascontiguousarray(regions[:2_000])
    big = vs.genotype_matrix(batch, sub)
    whole = big.genotype_matrix()
    tables = set()
    for n in (1, 7, 64, 100, 101, 103):   # (of tables whose rows differ by less than a block at most one is a whole number of blocks)
        small = vs.genotype_matrix(np.ascontiguousarray(batch[:n]), sub)
        got = small.genotype_matrix()
        _shape_checks(got, sub)
        a, na = _reported(got, range(n))
        b, nb = _reported(whole, range(n))
        assert np.array_equal(na, nb) and np.array_equal(got["cells"][a], whole["cells"][b]), n
        for q in range(min(n, 7)):
            assert small.region_text(q) == big.region_text(q), (n, q)
        tables.add(got["cells"].shape[0])
        small.close()
    assert len(tables) >= 5
    # a table of one row, and of none
    rc = whole["row_count"]
    full = vs.genotype_matrix(batch)
    gf = full.genotype_matrix()
    lone = np.nonzero(rc == 1)[0]
    one = int(lone[gf["cells"][gf["row_begin"][lone].astype(np.int64)].any(axis=1)][0])
    none = int(np.nonzero(rc == 0)[0][0])
    r1 = vs.genotype_matrix(np.ascontiguousarray(batch[one:one + 1]))
    g1 = r1.genotype_matrix()
    assert g1["cells"].shape == (1, vs.info().num_samples - 1)
    assert np.array_equal(g1["cells"][0], gf["cells"][int(gf["row_begin"][one])]) and g1["cells"].any()
    assert r1.totals()[2] == int(np.count_nonzero(g1["cells"]))
    r1.close(); full.close()
    for s in (None, sub):
        r0 = vs.genotype_matrix(np.ascontiguousarray(batch[none:none + 1]), s)
        g0 = r0.genotype_matrix()
        nc = vs.info().num_samples - 1 if s is None else len(s)
        assert g0["cells"].shape == (0, nc) and g0["columns"].shape == (nc,) and g0["rows"].shape == (0,)
        assert r0.totals()[1:3] == (0, 0)
        assert r0.region_text(0) == "Pos\tRef\tAlt" + "".join("\t" + vs.sample_name(int(i)) for i in g0["columns"]) + "\n"
        assert r0.region_genotypes(0) == []
        ptr, a, c, pitch = r0.genotype_matrix_device()
        assert (a, c) == (0, nc) and pitch % 16 == 0
        r0.close()
    rows = big.region_genotypes(int(np.nonzero(rc > 1)[0][0]))
    assert len(rows) > 1 and all(len(v["calls"]) == len(sub) and v["ref"] and v["alt"] for v in rows)
    big.close()


def test_written_once_no_stale_bytes():
    """A matrix whose buffer comes back from the handle's pool: the bytes the earlier batch left in it must all be overwritten."""
    vs = VariantStore.synthetic(device=0, **T6_KW)
    rng = np.random.default_rng(4)
    s = np.sort(rng.integers(1_000, 7_990_000, size=1_500))
    regions = np.stack([s, s + rng.integers(50, 3_000, size=1_500)], axis=1).astype(np.uint64)
    whole = vs.genotype_matrix(regions)
    full = whole.genotype_matrix()["cells"]
    whole.close()
    order = rng.permutation(299) + 1
    dense = sorted(int(i) for i in order[:130])      # two disjoint sample sets of one size: the same A x C, other bytes
    other = sorted(int(i) for i in order[130:260])
    first = vs.genotype_matrix(regions, dense)
    g1 = first.genotype_matrix()
    assert np.array_equal(g1["cells"], full[:, np.asarray(dense) - 1]) and g1["cells"].any()
    first.close()
    second = vs.genotype_matrix(regions, other)
    g2 = second.genotype_matrix()
    assert g2["cells"].shape == g1["cells"].shape
    assert np.array_equal(g2["cells"], full[:, np.asarray(other) - 1])
    assert not _pitched(g2)[:, 130:].any()
    second.close()
    # other regions with a table of about the same size
    s2 = np.sort(rng.integers(1_000, 7_990_000, size=1_500))
    regions2 = np.stack([s2, s2 + rng.integers(50, 3_000, size=1_500)], axis=1).astype(np.uint64)
    third = vs.genotype_matrix(regions2, [7])
    g3 = third.genotype_matrix()
    whole2 = vs.genotype_matrix(regions2)
    assert np.array_equal(g3["cells"][:, 0], whole2.genotype_matrix()["cells"][:, 6])
    assert not _pitched(g3)[:, 1:].any()
    third.close(); whole2.close()
    vs.close()


class _DeviceBytes:
    """(A, pitch) uint8 in device memory, for torch.as_tensor."""

    def __init__(self, ptr, a, pitch):
        self.__cuda_array_interface__ = {"shape": (a, pitch), "typestr": "|u1", "data": (ptr, True), "version": 3, "strides": None}


def _read_device(torch, ptr, a, pitch):
    try:
        return torch.as_tensor(_DeviceBytes(ptr, a, pitch), device="cuda").cpu().numpy().copy()
    except (TypeError, RuntimeError, ValueError):   # this torch does not take the interface: a plain copy through the runtime it loaded
        hip = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    hip = C.CDLL(line.split()[-1])
                    break
        assert hip is not None, "no HIP runtime is loaded"
        out = np.zeros((a, pitch), np.uint8)
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0   # hipMemcpyDeviceToHost
        return out


def test_device_pointer(t6_store):
    torch = pytest.importorskip("torch")
    vs, regions = t6_store
    res = vs.genotype_matrix(regions[:2_000])
    ptr, a, c, pitch = res.genotype_matrix_device()
    assert c == vs.info().num_samples - 1 and pitch == 304 and a > 2_000 and ptr
    first = _read_device(torch, ptr, a, pitch)
    later = vs.genotype_matrix(regions[2_000:2_900])   # a later batch on the same handle leaves the matrix alone
    later.totals()
    got = res.genotype_matrix()
    assert got["row_pitch"] == pitch and got["cells"].shape == (a, c)
    assert np.array_equal(first, _pitched(got)) and first.any()
    assert np.array_equal(_read_device(torch, ptr, a, pitch), first)
    later.close(); res.close()


def test_interleaving_leaves_type6_alone():
    rng = np.random.default_rng(12)
    batches = []
    for k in range(10):
        n = 3_000 + 200 * k + (4_000 if k == 6 else 0)   # like batches (speculated), one larger (refused / re-sized)
        s = np.sort(rng.integers(1_000, 7_990_000, size=n))
        batches.append(np.stack([s, s + rng.integers(50, 3_000, size=n)], axis=1).astype(np.uint64))
    shuffled = batches[3][rng.permutation(batches[3].shape[0])]

    def run(with_matrix):
        vs = VariantStore.synthetic(device=0, **T6_KW)
        digests = []
        for k, b in enumerate(batches):
            r = vs.get_var_in_ref(b)
            if with_matrix:   # matrix batches in between: sorted, unsorted, with a subset
                m1 = vs.genotype_matrix(b)
                m2 = vs.genotype_matrix(shuffled)
                m3 = vs.genotype_matrix(shuffled, [1, 5, 7, 200])
                for m in (m1, m2, m3):
                    m.totals()
                    m.close()
            digests.append(r.digest())
            r.close()
        info = vs.info()
        out = (digests, info.t6_speculated, info.t6_refused)
        vs.close()
        return out

    plain, mixed = run(False), run(True)
    assert plain[1] > 0, "the type-6 batches were not speculated"
    assert plain == mixed


def test_size_limit(t6_store):
    vs, regions = t6_store
    batch = np.ascontiguousarray(regions[:2_000])
    ok = vs.genotype_matrix(batch)
    ptr, a, c, pitch = ok.genotype_matrix_device()
    ok.close()
    assert a * pitch > 1 << 20
    vs.set_option("matrix_max_mib", 1)
    try:
        with pytest.raises(VariantStoreError) as e:
            vs.genotype_matrix(batch)
        assert e.value.code == VS_ERR_ARG
        msg = str(e.value)
        assert str(a) in msg and str(c) in msg and str(a * pitch) in msg, msg
        few = vs.genotype_matrix(batch, [1, 2, 3])   # 16 bytes a row: below the limit
        assert few.genotype_matrix()["cells"].shape == (a, 3)
        few.close()
    finally:
        vs.set_option("matrix_max_mib", 0)
    again = vs.genotype_matrix(batch)
    assert again.genotype_matrix()["cells"].shape == (a, c)
    again.close()


def test_refused_accessors(t6_store):
    vs, regions = t6_store
    r = vs.genotype_matrix(regions[:1_000])
    for call in (lambda: r.raw(with_carriers=True), lambda: r.view(with_carriers=True), r.digest, r.num_header_records,
                 r.num_region_records):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_UNSUPPORTED
    for call in (r.allele_counts, r.sample_burden, r.sample_burden_device):   # not a count result, not a burden result
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_ARG
    r.view(with_carriers=False)
    raw = r.raw(with_carriers=False)
    t6 = vs.get_var_in_ref(regions[:1_000])
    raw6 = t6.raw(with_carriers=False)
    for f in ("pos", "ref_off", "ref_len", "alt_off", "alt_len", "count_flags"):
        assert np.array_equal(raw["rows"][f], raw6["rows"][f]), f
    assert np.array_equal(raw["region_flags"], raw6["region_flags"])
    assert np.array_equal(raw["row_count"], raw6["row_count"]) and np.array_equal(raw["var_count"], raw6["var_count"])
    some = raw["row_count"] > 0
    assert some.any() and not some.all()
    assert np.array_equal(raw["row_begin"][some], raw6["row_begin"][some])
    assert r.totals()[:2] == t6.totals()[:2]
    r.close()
    for res in (t6, vs.allele_counts(regions[:10]), vs.sample_burden(regions[:10])):
        with pytest.raises(VariantStoreError) as e:
            res.genotype_matrix()   # not a matrix result
        assert e.value.code == VS_ERR_ARG
        with pytest.raises(VariantStoreError) as e:
            res.genotype_matrix_device()
        assert e.value.code == VS_ERR_ARG
        res.close()


def test_device_regions(t6_store):
    torch = pytest.importorskip("torch")
    vs, regions = t6_store
    sub = [3, 17, 40, 200]
    rng = np.random.default_rng(3)
    s = np.sort(rng.integers(1_000, 7_990_000, size=5_000))
    batch = np.stack([s, s + rng.integers(50, 3_000, size=5_000)], axis=1).astype(np.uint64)
    host = vs.genotype_matrix(batch, sub).genotype_matrix()
    t = torch.from_numpy(batch.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    dev = vs.genotype_matrix(DeviceArray(t.data_ptr(), batch.shape[0]), sub).genotype_matrix()
    for k in ("columns", "cells", "row_begin", "row_count", "flags"):
        assert np.array_equal(host[k], dev[k]), k
    assert host["cells"].any() and host["row_pitch"] == dev["row_pitch"] == 16


def test_cli_genotypes(golden_dir, tmp_path):
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
        out = os.path.join(tmp_path, "genotypes.txt")
        subprocess.run([exe, "genotypes", "-p", prefix, "-r", "@" + rfile, "-o", out] + extra, check=True, capture_output=True)
        with open(out) as f:
            parts = f.read().split("#region ")[1:]
        res = vs.genotype_matrix(regions, samples)
        assert len(parts) == len(regions)
        for q, part in enumerate(parts):
            head, text = part.split("\n", 1)
            assert head == f"{q} {regions[q][0]}:{regions[q][1]}"
            assert text == res.region_text(q), q
            some |= text.count("\n") > 1
        res.close()
    assert some
    with open(sfile, "w") as f:
        f.write(names[0] + "\nnobody-of-that-name\n")
    p = subprocess.run([exe, "genotypes", "-p", prefix, "-r", "@" + rfile, "-S", sfile], capture_output=True, text=True)
    assert p.returncode != 0 and "Sample not found: nobody-of-that-name" in (p.stdout + p.stderr)
    vs.close()
