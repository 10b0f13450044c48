"""Association scans on the GPU (vs_query_assoc_scan).  Integer-valued phenotypes: every DOT cell equals the int64 reference worked
out from the oracle's type-6 text exactly -- golden sweeps, the duplicate rule, the three storage forms, the class-row widths of 63
and 64 words, K = 1, 3 and 8, the whole cohort and a subset, ids given shuffled.  The flat pass's segments (a listed row longer than
a wave's step, rows of 1 .. 8 carriers, a table that ends inside a wave's rows), real-valued phenotypes within the bound of m - 1
rounded additions, the score test, determinism (twice, LDS against global table, a dirty pool), cross-checks against the count,
grouped-count and genotype-matrix queries, and the plumbing: interleaving, device regions and pointers, refused accessors, the size
limit, the CLI."""
import math
import os
import subprocess

import numpy as np
import pytest

import assoc_exact_ref
import assoc_scan_ref as ref
from helpers import random_regions, write_random_cohort
from test_gpu_genotype_matrix import _columns, _oracle, _parse, _read_device, _ref_len, _ref_rows, _reported
from test_gpu_row_width_edges import SPREAD_KW, SPREAD_SEED
from variantstore_amd import DeviceArray, VariantStore
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_ARG, VS_ERR_UNSUPPORTED = -5, -7
EPS = 2.0 ** -53
FIELDS = ("carriers", "alt_alleles", "hom_alt", "phased")


def _int_traits(rng, n, k):
    """Integer-valued float32 (n, k): trait 0 case-control labels 0/1, the others integers in -8 .. 8."""
    y = rng.integers(-8, 9, size=(n, k)).astype(np.float32)
    y[:, 0] = rng.integers(0, 2, size=n)
    return y


def _real_traits(rng, n):
    """float32 (n, 3): standard normal, one trait of magnitude 1e6 beside one of 1e-3."""
    y = rng.standard_normal(size=(n, 3)).astype(np.float32)
    y[:, 1] *= np.float32(1e6)
    y[:, 2] *= np.float32(1e-3)
    return y


def _query(vs, regions, ycol, samples, rng, stat="dot", names=None):
    """The query with `ycol` (rows in column order); a subset's ids are given shuffled, their rows with them."""
    if samples is None:
        return vs.assoc_scan(regions, ycol, None, stat, names)
    ids, _names = _columns(vs, samples)
    perm = rng.permutation(len(ids))
    return vs.assoc_scan(regions, ycol[perm], [ids[i] for i in perm], stat, names)


def _check_rows(vs, got, parsed, valid, samples, ycol):
    """What every result is held to, whatever the phenotypes: the columns, the counts, the traits' sums, zeros on dropped rows.
    Returns (the table rows the regions report, the reference's rows for them)."""
    ids, names = _columns(vs, samples)
    assert got["col_ids"].dtype == np.uint32 and got["col_ids"].tolist() == ids
    assert got["scores"].dtype == np.float64 and got["scores"].shape == (got["rows"].shape[0], ycol.shape[1])
    mine, n_mine = _reported(got, valid)
    rows, n_ref = _ref_rows(parsed, valid)
    assert np.array_equal(n_mine, n_ref)
    cnt = ref.counts(parsed, names)
    for f, field in enumerate(FIELDS):
        assert np.array_equal(got["counts"][field][mine].astype(np.int64), cnt[rows, f]), field
    dropped = (got["rows"]["count_flags"] >> 31) != 0
    assert not got["scores"][dropped].any() and not got["counts"]["carriers"][dropped].any(), "a dropped row has carriers"
    sy, syy = ref.trait_sums(ycol)
    assert np.array_equal(got["trait_sum"], sy) and np.array_equal(got["trait_sumsq"], syy)
    return mine, rows, names


def _check_int(vs, regions, parsed, valid, samples, ycol, rng, chi2=True):
    """DOT over integer-valued phenotypes: exact; CHI2: within 8 * 2^-53 relative of the reference formed from the exact sums."""
    res = _query(vs, regions, ycol, samples, rng)
    got = res.assoc_scan()
    mine, rows, names = _check_rows(vs, got, parsed, valid, samples, ycol)
    want = ref.dot_int(parsed, names, ycol)
    assert np.array_equal(got["scores"][mine], want[rows].astype(np.float64)), (samples is None, ycol.shape)
    res.close()
    if chi2:
        cres = _query(vs, regions, ycol, samples, rng, "chi2")
        c = cres.assoc_scan()
        cres.close()
        assert c["stat"] == "chi2"
        mine_c, _rows, _names = _check_rows(vs, c, parsed, valid, samples, ycol)   # (the private rows of two batches need not lie alike)
        cnt = ref.counts(parsed, names)
        sy, syy = ref.trait_sums(ycol)
        exp = ref.chi2(len(names), cnt[:, 1], cnt[:, 2], sy, syy, want.astype(np.float64))[rows]
        assert np.all(np.abs(c["scores"][mine_c] - exp) <= 8 * EPS * np.abs(exp))
        assert np.all(c["scores"] >= 0)
    return got


def _check_real(vs, regions, parsed, valid, samples, ycol, rng):
    """Real-valued phenotypes: |got - fsum| <= m 2^-53 sum |d y| per cell, m the row's carriers in S (m - 1 rounded additions of exact
    terms); the sums of the traits within n 2^-53 sum |y| and n 2^-53 sum y^2 of fsum; CHI2 against the formula applied on the host
    to the engine's own DOT cells, counts and sums within 8 * 2^-53 relative -- for the traits taken about their pivots, where
    the score is formed from exactly those cells (below); the traits as given give the same bytes where y - c is exact, and stay
    within the bound of the exact statistic that assoc_exact_ref derives from the text and the trait values alone."""
    res = _query(vs, regions, ycol, samples, rng)
    got = res.assoc_scan()
    res.close()
    mine, rows, names = _check_rows(vs, got, parsed, valid, samples, ycol)
    want, mag, m = ref.dot_fsum(parsed, names, ycol)
    err = np.abs(got["scores"][mine] - want[rows])
    assert np.all(err <= (m[rows, None] * EPS) * mag[rows]), float((err / np.maximum(mag[rows], 1e-300)).max())
    n = len(names)
    y64 = ycol.astype(np.float64)
    for k in range(ycol.shape[1]):
        assert abs(got["trait_sum"][k] - math.fsum(y64[:, k])) <= n * EPS * math.fsum(np.abs(y64[:, k]))
        assert abs(got["trait_sumsq"][k] - math.fsum(y64[:, k] ** 2)) <= n * EPS * math.fsum(y64[:, k] ** 2)
    cres = _query(vs, regions, ycol, samples, rng, "chi2")
    c = cres.assoc_scan()
    cres.close()
    mine_c, _rows, _names = _check_rows(vs, c, parsed, valid, samples, ycol)
    # the formula's order of operations: y2 = float32(y - c) holds 0.0 where y holds its pivot, and 0.0 is y2's own pivot, so the
    # CHI2 query over y2 adds the numbers its DOT query adds, in the same order, and forms the score from y2's raw sums
    piv = ref.pivots(ycol)
    y2 = (y64 - piv[None, :]).astype(np.float32)
    assert not ref.pivots(y2).any(), "a near-tie of the pivot"
    dres, c2res = _query(vs, regions, y2, samples, rng), _query(vs, regions, y2, samples, rng, "chi2")
    about, c2 = dres.assoc_scan(), c2res.assoc_scan()
    dres.close(); c2res.close()
    mine_d, mine_2 = _reported(about, valid)[0], _reported(c2, valid)[0]
    exp = ref.chi2(n, about["counts"]["alt_alleles"][mine_d], about["counts"]["hom_alt"][mine_d], about["trait_sum"], about["trait_sumsq"], about["scores"][mine_d])
    assert np.all(np.abs(c2["scores"][mine_2] - exp) <= 8 * EPS * np.abs(exp))
    exact_diff = (y2.astype(np.float64) == y64 - piv[None, :]).all(axis=0)
    # where every y - c is a float32 as it is, y and y2 are the same numbers to the kernel: the same bytes
    assert c["scores"][mine_c][:, exact_diff].tobytes() == c2["scores"][mine_2][:, exact_diff].tobytes()
    dense = np.zeros((parsed.n_rows, n), np.int64)
    r_, c_, d_, _val = ref.dosages(parsed, names)
    dense[r_, c_] = d_
    val, bound = assoc_exact_ref.table(dense, ycol)
    err = np.abs(c["scores"][mine_c] - val[rows])
    assert np.all(err <= bound[rows] + EPS * val[rows]), float((err / np.maximum(bound[rows] + EPS * val[rows], 1e-300)).max())
    return got


def _subset(rng, ns):
    """A subset that straddles the mask-word boundaries at ids 64 and 128 and contains the last sample (small cohorts: what fits)."""
    ids = set(int(i) for i in rng.choice(np.arange(1, ns + 1), size=max(1, ns // 3), replace=False))
    ids.update(i for i in range(40, 151) if i <= ns)
    ids.add(ns)
    return sorted(ids)


def _sweep(vs, regions, parsed, valid, rng, real=False):
    """K = 1, 3 and 8 over the whole cohort and a subset."""
    ns = vs.info().num_samples - 1
    sub = _subset(rng, ns)
    for samples, n in ((None, ns), (sub, len(sub))):
        for k in (1, 3, 8):
            got = _check_int(vs, regions, parsed, valid, samples, _int_traits(rng, n, k), rng)
        if real:
            _check_real(vs, regions, parsed, valid, samples, _real_traits(rng, n), rng)
    # the whole cohort by explicit ids, shuffled: the same columns
    y = _int_traits(rng, ns, 3)
    _check_int(vs, regions, parsed, valid, list(range(1, ns + 1)), y, rng, chi2=False)
    return got


@pytest.mark.parametrize("stem", ["x", "x.small"])
def test_golden_region_sweeps(stem, golden_dir, tmp_path):
    fasta, vcf = os.path.join(golden_dir, stem + ".fa"), os.path.join(golden_dir, stem + ".vcf")
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(11)
    regions = random_regions(rng, _ref_len(fasta), 200)   # unsorted: the device sorts the batch
    parsed, valid = _parse(orc, regions)
    _sweep(vs, regions, parsed, valid, rng, real=True)
    srt = sorted(regions)
    _sweep(vs, srt, *_parse(orc, srt), rng)
    # the text, with names and without; n = 1: vy = 0, every CHI2 cell is 0
    y = _int_traits(rng, 1, 3)
    names = _columns(vs, None)[1]
    want, cnt = ref.dot_int(parsed, names, y).astype(np.float64), ref.counts(parsed, names)
    for tn in (None, ["case", "q 1", "q2"]):
        res = vs.assoc_scan(regions, y, trait_names=tn)
        for q in valid:
            assert res.region_text(int(q)) == ref.assoc_text(parsed, int(q), cnt, want, tn), (q, regions[q])
        assert res.assoc_scan()["trait_names"] == (tn or ["0", "1", "2"])
        res.close()
    c = vs.assoc_scan(regions, y, stat="chi2")
    assert not c.assoc_scan()["scores"].any() and want.any()
    c.close()
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
    got = _sweep(vs, regions, parsed, valid, rng, real=True)
    assert np.any(got["rows"]["count_flags"] >> 31), "no row of the batch was dropped by the duplicate rule"
    # region_assoc: the text as dicts
    res = vs.assoc_scan(regions, _int_traits(rng, 9, 2), trait_names=["cc", "q"])
    arr = res.assoc_scan()
    q = int(valid[np.argmax(parsed.row_count[valid])])
    rows = res.region_assoc(q)
    mine, _n = _reported(arr, [q])
    assert len(rows) == mine.shape[0] > 1
    for r, a in zip(rows, mine):
        assert r["scores"] == {"cc": arr["scores"][a, 0], "q": arr["scores"][a, 1]} and r["alt_alleles"] == arr["counts"]["alt_alleles"][a]
    res.close()
    vs.close()


@pytest.mark.parametrize("shape", ["narrow_dense", "wide", "explicit"])
def test_storage_forms(shape, tmp_path):
    """gt_groups (1,500 samples, dense rows: the staged row path), gt_nibbles of a 4,100-sample class-row cohort, and the unpadded
    pool of a 10,000-sample explicit-id cohort, whose K = 8 table (320 KB) can only take the global form: short scattered regions
    and long overlapping ones, the long ones shuffled as well."""
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
    n_long = 24 if shape == "explicit" else 6   # (the class-row cohorts: some hundred carriers a row, every one parsed from the oracle's text)
    base = int(rng.integers(3_000, 1_400_000))
    long_ = sorted((int(x), int(x) + int(rng.integers(5_000, 20_000))) for x in base + rng.integers(0, 15_000, size=n_long))
    dense_seen = 0
    for regions in (short, long_):
        parsed, valid = _parse(orc, regions)
        got = _sweep(vs, regions, parsed, valid, rng, real=True)
        dense_seen = max(dense_seen, int((got["rows"]["count_flags"] & 0x7FFFFFFF).max()))
    perm = rng.permutation(len(long_))
    shuffled = [long_[i] for i in perm]
    _sweep(vs, shuffled, *_parse(orc, shuffled), rng)
    if shape == "narrow_dense":   # the dense path ran: rows with more carriers than a decoded list holds
        assert dense_seen > info.list_max
    if shape == "explicit":       # rows of 1 .. 8 carriers, one group each: a wave's 64 rows whose step holds 32 segments or more
        cnt = got["rows"]["count_flags"] & 0x7FFFFFFF
        few = ((cnt >= 1) & (cnt <= 8))[: cnt.shape[0] // 64 * 64].reshape(-1, 64)
        assert few.shape[0] > 4 and few.sum(axis=1).max() >= 32 and set(range(1, 9)) <= set(cnt.tolist())
    vs.close()


@pytest.mark.parametrize("n_samples", [4031, 4032])
def test_row_width_edges(n_samples, tmp_path, monkeypatch):
    """Class rows of 63 and 64 words (gt_groups' widest, gt_nibbles' narrowest), listed and dense rows together."""
    monkeypatch.setenv("VS_LIST_MAX", "64")
    vs = VariantStore.synthetic(device=0, num_samples=n_samples, seed=SPREAD_SEED[n_samples], **SPREAD_KW)
    info = vs.info()
    assert (info.num_samples + 63) // 64 == (63 if n_samples == 4031 else 64) and info.list_max == 64
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(n_samples)
    starts = np.sort(rng.integers(1, info.ref_length - 1500, size=30))
    regions = [(int(s), int(s) + int(rng.integers(750, 1500))) for s in starts]
    parsed, valid = _parse(orc, regions)
    got = _sweep(vs, regions, parsed, valid, rng, real=True)
    cnt = got["rows"]["count_flags"] & 0x7FFFFFFF
    assert (cnt > 64).sum() > 10 and ((cnt > 0) & (cnt <= 64)).sum() > 10, "both paths"
    vs.close()


T6_KW = dict(ref_length=8_000_000, num_variants=150_000, num_samples=300, seed=5, first_pos=1_000, frac_ins=0.05, frac_del=0.05,
             frac_multi=0.02, max_indel=6, af_exponent=2.0)


@pytest.fixture(scope="module")
def t6_store():
    vs = VariantStore.synthetic(device=0, **T6_KW)
    rng = np.random.default_rng(31)
    s = np.sort(rng.integers(1_000, 7_990_000, size=4_000))
    regions = np.stack([s, s + rng.integers(50, 3_000, size=s.shape[0])], axis=1).astype(np.uint64)
    yield vs, regions
    vs.close()


def _dosage_times(vs, regions, samples, ycol):
    """dosage(genotype_matrix) @ Y in int64: the route the scan replaces."""
    m = vs.genotype_matrix(regions, samples)
    cells = m.genotype_matrix()["cells"]
    m.close()
    d = ((cells >> 1) & 1).astype(np.int64) + ((cells >> 2) & 1)
    return d @ ycol.astype(np.int64)


def test_dot_equals_the_matrix_route(t6_store):
    """The 300-sample cohort: DOT == dosage(genotype_matrix) @ Y in int64; rows of one group beside rows of many in the same steps."""
    vs, regions = t6_store
    rng = np.random.default_rng(8)
    sub = _subset(rng, 300)
    for samples, n in ((None, 300), (sub, len(sub))):
        for k in (1, 3, 8):
            y = _int_traits(rng, n, k)
            res = _query(vs, regions, y, samples, rng)
            got = res.assoc_scan()
            assert np.array_equal(got["scores"], _dosage_times(vs, regions, samples, y).astype(np.float64)), (n, k)
            assert res.fill_ms() > 0
            res.close()
    cnt = got["rows"]["count_flags"] & 0x7FFFFFFF
    few = (cnt >= 1) & (cnt <= 8)
    assert few.sum() > 1_000 and (cnt > 64).sum() > 1_000 and got["scores"][few].any(), "short and long segments share the steps"


def test_listed_row_longer_than_a_step(monkeypatch):
    """VS_LIST_MAX = 1,499 on the 1,500-sample cohort: every row is listed, the flat pass walks rows of more than 512 carriers -- more
    than the 64 groups of one step -- whose sums continue in the next step.  Against the matrix route, and against the same cohort
    under the default threshold, where those rows take the dense pass."""
    kw = dict(ref_length=1_500_000, num_variants=30_000, seed=9, first_pos=2_000, frac_ins=0.05, frac_del=0.05, frac_multi=0.01, max_indel=6,
              num_samples=1_500, af_exponent=0.8)
    rng = np.random.default_rng(3)
    starts = np.sort(rng.integers(3_000, 1_495_000, size=200))
    regions = [(int(x), int(x) + 400) for x in starts]
    sub = _subset(rng, 1_500)
    ys = {None: _int_traits(rng, 1_500, 8), "sub": _int_traits(rng, len(sub), 3)}
    out = {}
    for list_max in ("1499", None):
        if list_max:
            monkeypatch.setenv("VS_LIST_MAX", list_max)
        else:
            monkeypatch.delenv("VS_LIST_MAX")
        vs = VariantStore.synthetic(device=0, **kw)
        info = vs.info()
        for key, samples in ((None, None), ("sub", sub)):
            res = vs.assoc_scan(regions, ys[key], samples)
            got = res.assoc_scan()
            res.close()
            cnt = got["rows"]["count_flags"] & 0x7FFFFFFF
            if list_max:
                assert info.list_max == 1_499 and (cnt > 512).sum() > 20 and cnt.max() <= info.list_max, "no listed row spans two steps"
                assert np.array_equal(got["scores"], _dosage_times(vs, regions, samples, ys[key]).astype(np.float64))
            else:
                assert (cnt > info.list_max).sum() > 20
            out[(list_max, key)] = got
        vs.close()
    for key in (None, "sub"):
        a, b = out[("1499", key)], out[(None, key)]
        assert np.array_equal(a["scores"], b["scores"]) and np.array_equal(a["counts"], b["counts"]) and a["scores"].any()


def test_table_ends_inside_a_wave(t6_store):
    vs, regions = t6_store
    rng = np.random.default_rng(5)
    y = _int_traits(rng, 300, 3)
    for n in range(900, 1_000):   # a batch whose table ends inside a wave's 64 rows
        big = vs.assoc_scan(regions[:n], y)
        a = big.layout()[1]
        if a % 64:
            break
        big.close()
    assert a % 64 != 0 and a > 4 * 64
    got = big.assoc_scan()
    assert got["scores"].shape == (a, 3)
    assert np.array_equal(got["scores"], _dosage_times(vs, regions[:n], None, y).astype(np.float64))
    for k in (1, 7, 64):
        small = vs.assoc_scan(regions[:k], y)
        for q in range(k):
            assert small.region_text(q) == big.region_text(q), (k, q)
        small.close()
    big.close()


def test_chi2_degenerate_cases(t6_store):
    """A constant trait (vy = 0), monomorphic rows over the subset (vx = 0) and n = 1: 0.0, never a NaN."""
    vs, regions = t6_store
    rng = np.random.default_rng(17)
    y = _int_traits(rng, 300, 3)
    y[:, 1] = 5.0
    res = vs.assoc_scan(regions[:1_500], y, stat="chi2")
    got = res.assoc_scan()
    res.close()
    assert not got["scores"][:, 1].any() and got["scores"][:, 0].any() and np.all(np.isfinite(got["scores"]))
    sub = [7, 90, 201]
    res = vs.assoc_scan(regions[:1_500], _real_traits(rng, 3), sub, stat="chi2")
    got = res.assoc_scan()
    res.close()
    sx, hom = got["counts"]["alt_alleles"].astype(np.int64), got["counts"]["hom_alt"].astype(np.int64)
    mono = 3 * (sx + 2 * hom) - sx * sx == 0
    assert mono.sum() > 100 and (~mono).sum() > 10
    assert not got["scores"][mono].any() and got["scores"][~mono].any() and np.all(np.isfinite(got["scores"]))
    res = vs.assoc_scan(regions[:1_500], [[2.5, -1.0]], [299], stat="chi2")
    got = res.assoc_scan()
    res.close()
    assert got["counts"]["alt_alleles"].any() and not got["scores"].any()


def test_same_bytes_every_time(t6_store):
    """The same call twice, and the LDS form of the phenotype table against the global form (assoc_lds_max_kib = 1: 300 x 8 x 4 bytes
    do not fit 1 KiB), whole cohort and subset, DOT and CHI2."""
    vs, regions = t6_store
    rng = np.random.default_rng(23)
    sub = _subset(rng, 300)
    for samples, n in ((None, 300), (sub, len(sub))):
        y = np.concatenate([_real_traits(rng, n), _real_traits(rng, n), _real_traits(rng, n)[:, :2]], axis=1)
        for stat in ("dot", "chi2"):
            outs = []
            for kib in (0, 0, 1):
                vs.set_option("assoc_lds_max_kib", kib)
                try:
                    res = vs.assoc_scan(regions, y, samples, stat)
                    outs.append(res.assoc_scan()["scores"])
                    res.close()
                finally:
                    vs.set_option("assoc_lds_max_kib", 0)
            assert outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes() and outs[0].any()


def test_recycled_buffer_does_not_show_through():
    """The cells land in a buffer the handle's pool hands back dirty: a genotype matrix of at least their size was there before."""
    rng = np.random.default_rng(4)
    s = np.sort(rng.integers(1_000, 7_990_000, size=1_500))
    batch = np.stack([s, s + rng.integers(50, 3_000, size=s.shape[0])], axis=1).astype(np.uint64)
    y = np.concatenate([_real_traits(rng, 300), _int_traits(rng, 300, 5)], axis=1)
    fresh_vs = VariantStore.synthetic(device=0, **T6_KW)
    fresh = fresh_vs.assoc_scan(batch, y)
    want = fresh.assoc_scan()
    fresh.close(); fresh_vs.close()
    vs = VariantStore.synthetic(device=0, **T6_KW)
    m = vs.genotype_matrix(batch)
    _ptr, a, _c, pitch = m.genotype_matrix_device()
    assert a * pitch >= want["scores"].nbytes and m.totals()[2] > 0
    m.close()
    res = vs.assoc_scan(batch, y)
    got = res.assoc_scan()
    assert got["scores"].tobytes() == want["scores"].tobytes() and np.array_equal(got["counts"], want["counts"])
    assert np.array_equal(got["rows"], want["rows"])
    res.close(); vs.close()


def test_cross_checks_inside_the_engine(t6_store):
    """An all-ones trait is the row's alt_alleles over S; the 0/1 indicator of group g is group_counts' alt_alleles[:, g]; totals."""
    vs, regions = t6_store
    rng = np.random.default_rng(29)
    sub = _subset(rng, 300)
    for samples, n in ((None, 300), (sub, len(sub))):
        res = vs.assoc_scan(regions, np.ones(n, np.float32), samples)
        got = res.assoc_scan()
        cres = vs.allele_counts(regions, samples)
        cc = cres.allele_counts()["counts"]
        assert np.array_equal(got["scores"][:, 0], cc["alt_alleles"].astype(np.float64)) and np.array_equal(got["counts"], cc)
        assert res.totals()[:3] == cres.totals()[:3]
        lay = res.layout()
        assert lay[2] == 0 and lay[3] == 0 and lay[1] == got["rows"].shape[0]
        res.close(); cres.close()
    label = rng.integers(0, 5, size=301)
    members = [[int(i) for i in np.nonzero(label[1:] == g)[0] + 1] for g in range(5)]
    gres = vs.group_counts(regions, members)
    gc = gres.group_counts()["counts"]
    gres.close()
    y = (label[1:, None] == np.arange(5)[None, :]).astype(np.float32)
    res = vs.assoc_scan(regions, y)
    assert np.array_equal(res.assoc_scan()["scores"], gc["alt_alleles"].astype(np.float64))
    res.close()


def test_interleaving_leaves_type6_alone():
    rng = np.random.default_rng(12)
    batches = []
    for k in range(10):
        n = 3_000 + 200 * k + (4_000 if k == 6 else 0)   # like batches (speculated), one larger (refused / re-sized)
        s = np.sort(rng.integers(1_000, 7_990_000, size=n))
        batches.append(np.stack([s, s + rng.integers(50, 3_000, size=n)], axis=1).astype(np.uint64))
    shuffled = batches[3][rng.permutation(batches[3].shape[0])]
    y = _real_traits(rng, 300)

    def run(with_assoc):
        vs = VariantStore.synthetic(device=0, **T6_KW)
        digests = []
        for k, b in enumerate(batches):
            r = vs.get_var_in_ref(b)
            if with_assoc:   # association batches in between: sorted, unsorted
                c1 = vs.assoc_scan(b, y)
                c2 = vs.assoc_scan(shuffled, y[:3, :1], [1, 5, 200], "chi2")
                c1.totals(); c2.totals()
                c1.close(); c2.close()
            digests.append(r.digest())
            r.close()
        info = vs.info()
        out = (digests, info.t6_speculated, info.t6_refused)
        vs.close()
        return out

    plain, mixed = run(False), run(True)
    assert plain[1] > 0, "the type-6 batches were not speculated"
    assert plain == mixed


def test_device_regions_and_device_pointer(t6_store):
    torch = pytest.importorskip("torch")
    vs, regions = t6_store
    y = _real_traits(np.random.default_rng(2), 300)
    hres = vs.assoc_scan(regions, y, stat="chi2")
    host = hres.assoc_scan()
    t = torch.from_numpy(regions.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    dres = vs.assoc_scan(DeviceArray(t.data_ptr(), regions.shape[0]), y, stat="chi2")
    dev = dres.assoc_scan()
    for k in ("rows", "counts", "scores", "col_ids", "trait_sum", "trait_sumsq", "row_begin", "row_count", "flags"):
        assert np.array_equal(host[k], dev[k]), k
    dres.close()
    ps, pc, a, c, k, stat = hres.assoc_scan_device()
    assert (a, k) == host["scores"].shape and c == 300 and stat == "chi2" and ps and pc
    later = vs.assoc_scan(regions[:500], y)   # a later batch on the same handle leaves the cells alone
    later.totals()
    cells = _read_device(torch, ps, a, k * 8).view(np.float64).reshape(a, k)
    assert cells.tobytes() == host["scores"].tobytes() and cells.any()
    words = _read_device(torch, pc, a, 16).view(np.uint32).reshape(a, 4)
    for i, f in enumerate(FIELDS):
        assert np.array_equal(words[:, i], host["counts"][f]), f
    later.close(); hres.close()


def test_refused_accessors(t6_store):
    vs, regions = t6_store
    r = vs.assoc_scan(regions[:1_000], np.ones(300, np.float32))
    for call in (lambda: r.raw(with_carriers=True), lambda: r.view(with_carriers=True), r.digest, r.num_header_records,
                 r.num_region_records):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_UNSUPPORTED
    for call in (r.allele_counts, r.group_counts, r.group_counts_device, r.sample_burden, r.sample_burden_device, r.genotype_matrix,
                 r.genotype_matrix_device, r.ld_band, r.ld_band_device):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_ARG
    r.view(with_carriers=False)
    r.close()
    others = (vs.get_var_in_ref(regions[:1_000]), vs.allele_counts(regions[:1_000]), vs.genotype_matrix(regions[:100], [1, 2]),
              vs.group_counts(regions[:100], [[1], [2]]), vs.ld_band(regions[:100], window=4))
    for res in others:
        for call in (res.assoc_scan, res.assoc_scan_device):
            with pytest.raises(VariantStoreError) as e:
                call()
            assert e.value.code == VS_ERR_ARG
        res.close()


def test_size_limit(t6_store):
    vs, regions = t6_store
    y = _int_traits(np.random.default_rng(2), 300, 8)
    ok = vs.assoc_scan(regions, y)
    a = ok.layout()[1]
    ok.close()
    assert a * (8 * 8 + 16) > 1 << 20
    vs.set_option("matrix_max_mib", 1)
    try:
        with pytest.raises(VariantStoreError) as e:
            vs.assoc_scan(regions, y)
        assert e.value.code == VS_ERR_ARG
        msg = str(e.value)
        assert f"{a} rows" in msg and "8 traits" in msg and str(a * (8 * 8 + 16)) in msg, msg
        few = vs.assoc_scan(regions[:200], y[:, :2])   # a request below the limit is answered meanwhile
        got = few.assoc_scan()["scores"]
        assert got.shape[1] == 2 and 0 < got.nbytes < 1 << 20
        few.close()
    finally:
        vs.set_option("matrix_max_mib", 0)
    again = vs.assoc_scan(regions, y)
    assert again.assoc_scan()["scores"].shape == (a, 8)
    again.close()


def test_cli_assoc(tmp_path):
    exe = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
    fasta, vcf, names = write_random_cohort(str(tmp_path), 77, ref_len=6000, n_rows=300, n_samples=70)
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    subprocess.run([exe, "construct", "-r", fasta, "-v", vcf, "-p", prefix], check=True, capture_output=True)
    vs = VariantStore.open(prefix, device=0)
    rng = np.random.default_rng(2)
    regions = [(x, y) for x, y in sorted(random_regions(rng, 6000, 80)) if x >= 1]
    rfile = os.path.join(tmp_path, "regions.txt")
    with open(rfile, "w") as f:
        f.write("".join(f"{x}:{y}\n" for x, y in regions))
    who = [names[i] for i in rng.permutation(70)[:40]]
    y = np.stack([rng.integers(0, 2, size=40).astype(np.float32), rng.standard_normal(40).astype(np.float32)], axis=1)
    pfile = os.path.join(tmp_path, "pheno.txt")
    for header, tn in (("#sample\tcase bmi\n", ["case", "bmi"]), ("", None)):
        with open(pfile, "w") as f:   # tab or space; a blank line; float32 values written so that they read back as they are
            f.write(header + "\n".join(f"{n}\t{int(a)} {float(b)!r}" for n, (a, b) in zip(who, y)) + "\n\n")
        for flag, stat in (((), "dot"), (("--chi2",), "chi2")):
            out = os.path.join(tmp_path, "assoc_out.txt")
            subprocess.run([exe, "assoc", "-p", prefix, "-r", "@" + rfile, "-P", pfile, "-o", out, *flag], check=True, capture_output=True)
            with open(out) as f:
                parts = f.read().split("#region ")[1:]
            res = vs.assoc_scan(regions, y, who, stat, tn)
            assert len(parts) == len(regions)
            for q, part in enumerate(parts):
                head, text = part.split("\n", 1)
                assert head == f"{q} {regions[q][0]}:{regions[q][1]}"
                assert text == res.region_text(q), q
            assert res.assoc_scan()["scores"].any()
            res.close()
    vs.close()
