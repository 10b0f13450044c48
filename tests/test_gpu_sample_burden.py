"""Burden queries on the GPU (vs_query_sample_burden): the regions x samples matrix against what the oracle's type-6 text gives
(carriers by name, rows filtered by their allele count over the subset), against type 6's own carrier lists and the count
query, the duplicate rule, the list threshold, the three storage forms of the genotype bits (a column tile boundary inside the
row), a region split between workgroups, subset identities, interleaving with type-6 batches, regions in device memory, small
batches, the device pointer, the refused accessors and the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import oracle_texts, random_regions, write_random_cohort
from oracle.oracle import Oracle
from sample_burden_ref import FIELDS, NO_MAX, Parsed, burden_matrix, burden_sparse, burden_text, cells_array
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


def _check(vs, regions, parsed, valid, samples=None, min_ac=0, max_ac=None, texts=False):
    """The matrix of a burden query (and every region's text) against the reference helper; returns the cells as int64."""
    ids, names = _columns(vs, samples)
    res = vs.sample_burden(regions, samples, min_ac, max_ac)
    got = res.sample_burden()
    assert got["columns"].tolist() == ids
    cells = cells_array(got["cells"])
    want = burden_matrix(parsed, names, min_ac, NO_MAX if max_ac is None else max_ac)
    assert cells.shape == want.shape
    assert np.array_equal(cells[valid], want[valid]), (samples, min_ac, max_ac)
    if texts:
        for q in valid:
            assert res.region_text(int(q)) == burden_text(want[q], names), (q, regions[q])
    assert res.totals()[2] == int(cells[..., 0].sum())
    res.close()
    return cells


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
    t6 = vs.get_var_in_ref(regions).raw(with_carriers=False)
    assert np.any(t6["rows"]["count_flags"] >> 31), "no region of the batch falls under the duplicate rule"
    parsed, valid = _parse(orc, regions)
    subsets = [None] + [[vs.sample_id(s) for s in rng.choice(names, size=int(rng.integers(1, len(names))), replace=False)] for _ in range(3)]
    for sub in subsets:
        for lo, hi in ((0, None), (2, None), (0, 1), (1, 3)):
            _check(vs, regions, parsed, valid, sub, lo, hi, texts=(lo, hi) == (0, None))
    vs.close()


@pytest.mark.parametrize("list_max", [0, 3, 64])
@pytest.mark.parametrize("n_samples", [70, 150])
def test_list_threshold(list_max, n_samples, tmp_path, monkeypatch):
    """Small cohorts take the class-row path only under a lowered threshold (VS_LIST_MAX is read when an index is opened): row
    widths of 2 and 3 words, both paths, the whole cohort (the row path serves it too) and a subset."""
    monkeypatch.setenv("VS_LIST_MAX", str(list_max))
    vs = VariantStore.synthetic(device=0, ref_length=60_000, num_variants=1500, num_samples=n_samples, seed=500 + n_samples, first_pos=100,
                                frac_ins=0.06, frac_del=0.06, frac_multi=0.03, max_indel=4, af_exponent=2.5)
    assert vs.info().list_max == list_max
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(list_max * 31 + n_samples)
    L = vs.info().ref_length
    starts = rng.integers(1, L - 4000, size=60)
    regions = [(int(s), int(s) + int(rng.integers(1, 4000))) for s in starts] + [(1, 3000), (L - 2000, L + 5)]
    cc = vs.get_var_in_ref(regions).view(False)["car_count"]
    if list_max * 4 < n_samples:
        assert (cc > list_max).sum() > 20, "the row path must be exercised"
    parsed, valid = _parse(orc, regions)
    subset = [int(i) for i in rng.choice(np.arange(1, n_samples + 1), size=n_samples // 3, replace=False)]
    for sub in (None, subset):
        _check(vs, regions, parsed, valid, sub, texts=True)
        _check(vs, regions, parsed, valid, sub, 2, 9)
    vs.close()


def _check_sparse(vs, regions, parsed, valid, samples):
    """As _check for matrices too large to build twice: the nonzero cells against the reference's."""
    ids, names = _columns(vs, samples)
    res = vs.sample_burden(regions, samples)
    got = res.sample_burden()
    assert got["columns"].tolist() == ids
    cells = got["cells"]
    assert cells.shape == (len(regions), len(ids))
    keep = np.zeros(len(regions), bool)
    keep[valid] = True
    flat, vals = burden_sparse(parsed, names)
    sel = keep[flat // len(ids)]
    flat, vals = flat[sel], vals[sel]
    mine = cells[keep].reshape(-1)
    at = np.searchsorted(np.nonzero(keep)[0], flat // len(ids)) * len(ids) + flat % len(ids)
    for k, f in enumerate(FIELDS):
        assert np.array_equal(mine[f][at].astype(np.int64), vals[:, k]), f
    assert int(np.count_nonzero(mine["variants"])) == flat.shape[0]
    assert not mine["alt_alleles"][mine["variants"] == 0].any()
    res.close()
    return cells


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
    starts = np.sort(rng.integers(3_000, 1_495_000, size=2_500))
    short = [(int(x), int(x) + 25) for x in starts]
    long_ = sorted((int(x), int(x) + int(rng.integers(5_000, 40_000))) for x in rng.integers(3_000, 1_450_000, size=120))
    ns = info.num_samples - 1
    subset = [int(i) for i in rng.choice(np.arange(1, ns + 1), size=ns // 3, replace=False)]
    for regions in (short, long_):
        parsed, valid = _parse(orc, regions)
        perm = rng.permutation(len(regions))
        shuffled = [regions[i] for i in perm]
        for sub in (None, subset):
            cells = _check_sparse(vs, regions, parsed, valid, sub)
            res = vs.sample_burden(shuffled, sub)       # the device sorts the batch: the matrix's rows stay the caller's
            assert np.array_equal(res.sample_burden()["cells"], cells[perm])
            res.close()
            if shape == "wide" and sub is None:
                assert cells.shape[1] == ns > 4_096 and cells["variants"][:, 4_096:].any(), "no column beyond the first tile is set"
    vs.close()


T6_KW = dict(ref_length=8_000_000, num_variants=150_000, num_samples=300, seed=5, first_pos=1_000, frac_ins=0.05, frac_del=0.05,
             frac_multi=0.02, max_indel=6, af_exponent=2.0)


@pytest.fixture(scope="module")
def t6_store():
    vs = VariantStore.synthetic(device=0, **T6_KW)
    rng = np.random.default_rng(12)
    s = np.sort(rng.integers(1_000, 7_990_000, size=3_000))
    regions = np.stack([s, s + rng.integers(50, 3_000, size=3_000)], axis=1).astype(np.uint64)
    regions = np.concatenate([regions, np.array([[1, 7_999_000]], np.uint64)])   # far more rows than any chunk
    yield vs, regions
    vs.close()


def _from_type6(vs, regions, n_cols):
    """(matrix int64 (Q, n_cols, 4) over the whole cohort with every reported row counting, per region the table rows it
    reports) from type 6's own carrier lists: arena entries sample_id | gt << 13."""
    t6 = vs.get_var_in_ref(regions)
    raw = t6.raw(with_carriers=True)
    assert raw["carrier_bytes"] == 2
    rows, arena = raw["rows"], raw["arena"]
    cnt = (rows["count_flags"] & 0x7FFFFFFF).astype(np.int64)
    cnt[(rows["count_flags"] >> 31) != 0] = 0
    out = np.zeros((len(regions), n_cols, 4), np.int64)
    reported = []
    for q in range(len(regions)):
        a = np.arange(int(raw["row_begin"][q]), int(raw["row_begin"][q]) + int(raw["row_count"][q]))
        a = a[(rows["count_flags"][a] >> 31) == 0]
        reported.append(a)
        c = cnt[a]
        at = np.repeat(rows["car_begin"][a].astype(np.int64), c) + np.arange(c.sum()) - np.repeat(np.cumsum(c) - c, c)
        w = arena[at].astype(np.int64)
        sid, gt = w & 0x1FFF, w >> 13
        g1, g2, ph = (gt >> 1) & 1, (gt >> 2) & 1, gt & 1
        for k, v in enumerate((np.ones_like(sid), g1 + g2, g1 & g2, ph)):
            out[q, :, k] = np.bincount(sid - 1, weights=v, minlength=n_cols).astype(np.int64)
    t6.close()
    return out, reported


def test_against_type6_lists_counts_and_a_split_region(t6_store):
    vs, regions = t6_store
    ns = vs.info().num_samples - 1
    want, reported = _from_type6(vs, regions, ns)
    assert len(reported[-1]) > 100_000
    res = vs.sample_burden(regions)
    got = res.sample_burden()
    cells = cells_array(got["cells"])
    assert got["columns"].tolist() == list(range(1, ns + 1))
    assert np.array_equal(cells, want)
    # the same sums along the other axis: the count query's rows
    cres = vs.allele_counts(regions)
    counts = cres.allele_counts()["counts"]
    per_row = np.stack([counts[f].astype(np.int64) for f in ("carriers", "alt_alleles", "hom_alt", "phased")], axis=-1)
    for q in (0, 1, 17, 1_500, 2_999, 3_000):
        assert np.array_equal(cells[q].sum(axis=0), per_row[reported[q]].sum(axis=0)), q
    assert np.array_equal(cells.sum(axis=1), np.stack([per_row[a].sum(axis=0) for a in reported]))
    assert res.totals() == cres.totals()
    assert res.totals()[2] == int(cells[..., 0].sum())
    lay = res.layout()
    assert lay[2] == 0 and lay[3] == 0 and res.fill_ms() > 0
    res.close()
    # the window [1, 5]: the rows filtered by their alt_alleles
    wres = vs.sample_burden(regions, None, 1, 5)
    wcells = cells_array(wres.sample_burden()["cells"])
    ok = (per_row[:, 1] >= 1) & (per_row[:, 1] <= 5)
    assert np.array_equal(wcells.sum(axis=1), np.stack([per_row[a[ok[a]]].sum(axis=0) for a in reported]))
    assert wres.totals()[2] == int(wcells[..., 0].sum()) and wcells[..., 0].sum() < cells[..., 0].sum()
    assert np.all(wcells <= cells)
    wres.close(); cres.close()
    # smaller chunks (the long region and many of the others are split) give the same matrices
    r0 = vs.sample_burden(regions, [2, 3, 150, 299], 1, 5)
    c0 = r0.sample_burden()["cells"]
    r0.close()
    vs.set_option("burden_chunk", 64)
    try:
        for sub, lo, hi, same in ((None, 0, None, cells), ([2, 3, 150, 299], 1, 5, cells_array(c0))):
            r64 = vs.sample_burden(regions, sub, lo, hi)
            assert np.array_equal(cells_array(r64.sample_burden()["cells"]), same), sub
            assert r64.totals()[2] == int(same[..., 0].sum())
            r64.close()
    finally:
        vs.set_option("burden_chunk", 0)


def test_subset_identities(t6_store):
    vs, regions = t6_store
    ns = vs.info().num_samples - 1
    whole = vs.sample_burden(regions).sample_burden()
    everyone = vs.sample_burden(regions, list(range(1, ns + 1))).sample_burden()
    assert np.array_equal(whole["cells"], everyone["cells"]) and np.array_equal(whole["columns"], everyone["columns"])
    rng = np.random.default_rng(8)
    part = rng.integers(0, 4, size=ns)
    joined = np.zeros_like(whole["cells"])
    for k in range(4):
        ids = [int(i) + 1 for i in np.nonzero(part == k)[0]]
        got = vs.sample_burden(regions, ids).sample_burden()
        assert got["columns"].tolist() == ids
        joined[:, np.asarray(ids) - 1] = got["cells"]
    assert np.array_equal(joined, whole["cells"])


def test_interleaving_leaves_type6_alone():
    rng = np.random.default_rng(12)
    batches = []
    for k in range(10):
        n = 3_000 + 200 * k + (4_000 if k == 6 else 0)   # like batches (speculated), one larger (refused / re-sized)
        s = np.sort(rng.integers(1_000, 7_990_000, size=n))
        batches.append(np.stack([s, s + rng.integers(50, 3_000, size=n)], axis=1).astype(np.uint64))
    shuffled = batches[3][rng.permutation(batches[3].shape[0])]

    def run(with_burden):
        vs = VariantStore.synthetic(device=0, **T6_KW)
        digests = []
        for k, b in enumerate(batches):
            r = vs.get_var_in_ref(b)
            if with_burden:   # burden batches in between: sorted, unsorted, with a subset and a window
                b1 = vs.sample_burden(b)
                b2 = vs.sample_burden(shuffled, [1, 5, 7, 200], 1, 4)
                b1.totals(); b2.totals()
                b1.close(); b2.close()
            digests.append(r.digest())
            r.close()
        info = vs.info()
        out = (digests, info.t6_speculated, info.t6_refused)
        vs.close()
        return out

    plain, mixed = run(False), run(True)
    assert plain[1] > 0, "the type-6 batches were not speculated"
    assert plain == mixed


def test_device_regions_and_small_batches(t6_store):
    torch = pytest.importorskip("torch")
    vs, regions = t6_store
    sub = [3, 17, 40, 200]
    rng = np.random.default_rng(3)
    s = np.sort(rng.integers(1_000, 7_990_000, size=5_000))
    batch = np.stack([s, s + rng.integers(50, 3_000, size=5_000)], axis=1).astype(np.uint64)
    host = vs.sample_burden(batch, sub, 0, 40).sample_burden()
    t = torch.from_numpy(batch.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    dev = vs.sample_burden(DeviceArray(t.data_ptr(), batch.shape[0]), sub, 0, 40).sample_burden()
    for k in ("columns", "cells", "flags"):
        assert np.array_equal(host[k], dev[k]), k
    big = vs.sample_burden(batch, sub, 0, 40)
    for n in (1, 7, 64):
        small = vs.sample_burden(np.ascontiguousarray(batch[:n]), sub, 0, 40)
        assert np.array_equal(small.sample_burden()["cells"], host["cells"][:n]), n
        for q in range(n):
            assert small.region_text(q) == big.region_text(q), (n, q)
        small.close()
    big.close()


class _DeviceCells:
    """(Q, C, 4) int32 in device memory, for torch.as_tensor."""

    def __init__(self, ptr, q, c):
        self.__cuda_array_interface__ = {"shape": (q, c, 4), "typestr": "<i4", "data": (ptr, True), "version": 3, "strides": None}


def _read_device(torch, ptr, q, c):
    try:
        return torch.as_tensor(_DeviceCells(ptr, q, c), device="cuda").cpu().numpy().copy()
    except (TypeError, RuntimeError, ValueError):   # this torch does not take the interface: a plain copy through the runtime it loaded
        hip = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    hip = C.CDLL(line.split()[-1])
                    break
        assert hip is not None, "no HIP runtime is loaded"
        out = np.zeros((q, c, 4), np.int32)
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0   # hipMemcpyDeviceToHost
        return out


def test_device_pointer(t6_store):
    torch = pytest.importorskip("torch")
    vs, regions = t6_store
    res = vs.sample_burden(regions[:2_000], None, 1, 30)
    ptr, q, c = res.sample_burden_device()
    assert (q, c) == (2_000, vs.info().num_samples - 1) and ptr
    first = _read_device(torch, ptr, q, c)
    later = vs.sample_burden(regions[2_000:2_900])   # a later batch on the same handle leaves the matrix alone
    later.totals()
    host = cells_array(res.sample_burden()["cells"])
    assert np.array_equal(first.astype(np.int64), host) and host.any()
    assert np.array_equal(_read_device(torch, ptr, q, c), first)
    later.close(); res.close()


def test_refused_accessors(t6_store):
    vs, regions = t6_store
    r = vs.sample_burden(regions[:1_000])
    for call in (lambda: r.raw(with_carriers=True), lambda: r.view(with_carriers=True), r.digest, r.num_header_records,
                 r.num_region_records):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_UNSUPPORTED
    with pytest.raises(VariantStoreError) as e:
        r.allele_counts()   # not a count result
    assert e.value.code == VS_ERR_ARG
    r.view(with_carriers=False)
    raw = r.raw(with_carriers=False)
    t6 = vs.get_var_in_ref(regions[:1_000])
    raw6 = t6.raw(with_carriers=False)
    for f in ("pos", "ref_off", "ref_len", "alt_off", "alt_len", "count_flags"):
        assert np.array_equal(raw["rows"][f], raw6["rows"][f]), f
    assert np.array_equal(raw["region_flags"], raw6["region_flags"])
    assert np.array_equal(raw["row_count"], raw6["row_count"]) and np.array_equal(raw["var_count"], raw6["var_count"])
    # (where a region without rows points is not part of the answer: a type-6 batch on a handle that sorts first -- the fixture's
    #  unsorted batches left it so -- places it elsewhere in the table than a batch worked in the order given)
    some = raw["row_count"] > 0
    assert some.any() and not some.all()
    assert np.array_equal(raw["row_begin"][some], raw6["row_begin"][some])
    assert r.totals()[:2] == t6.totals()[:2]
    r.close()
    for res in (t6, vs.allele_counts(regions[:10])):
        with pytest.raises(VariantStoreError) as e:
            res.sample_burden()   # not a burden result
        assert e.value.code == VS_ERR_ARG
        with pytest.raises(VariantStoreError) as e:
            res.sample_burden_device()
        assert e.value.code == VS_ERR_ARG
        res.close()


def test_cli_burden(golden_dir, tmp_path):
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
    for samples, max_ac, extra in ((None, None, []), (names, None, ["-S", sfile]), (None, 1, ["--max-ac", "1"]),
                                   (names, 2, ["-S", sfile, "--min-ac", "1", "--max-ac", "2"])):
        out = os.path.join(tmp_path, "burden.txt")
        subprocess.run([exe, "burden", "-p", prefix, "-r", "@" + rfile, "-o", out] + extra, check=True, capture_output=True)
        with open(out) as f:
            parts = f.read().split("#region ")[1:]
        res = vs.sample_burden(regions, samples, 1 if "--min-ac" in extra else 0, max_ac)
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
    p = subprocess.run([exe, "burden", "-p", prefix, "-r", "@" + rfile, "-S", sfile], capture_output=True, text=True)
    assert p.returncode != 0 and "Sample not found: nobody-of-that-name" in (p.stdout + p.stderr)
    vs.close()
