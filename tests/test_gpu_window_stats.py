"""Window statistics on the GPU (vs_query_window_stats): every region's text against records worked out in Python integers from the
oracle's type-6 text (tests/window_stats_ref.py), the arrays against the same reduction done in numpy over vs.group_counts() of the
same call, the duplicate rule's dropped rows, the group counts at which the group kernel's padding and the new kernel's lane mapping
change, regions split between workgroups on a recycled pool, sums beyond 32 bits, regions in device memory, the device pointers,
interleaving with type-6 and group-count batches, the refused accessors, the size limit and the command line."""
import math
import os
import subprocess

import numpy as np
import pytest

import vcf_truth as vt
import window_stats_ref as ws
from group_counts_ref import parse_region
from helpers import SAT_REF_LEN, oracle_texts, random_regions, write_random_cohort, write_saturated_cohort
from test_gpu_genotype_matrix import _read_device
from test_gpu_group_counts import T6_KW, _members, _oracle, _partition, _ref_len, _small_groupings, rows_per_wave
from variantstore_amd import DeviceArray, QueryResult, VariantStore
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_ARG, VS_ERR_UNSUPPORTED = -5, -7


def reduce_numpy(gc, pairs=True):
    """The records of a window-statistics result from QueryResult.group_counts() of the same regions and groups, in numpy: what a
    caller does on the host without the query.  -> structured (Q, G) and (Q, P) arrays."""
    counts, sizes = gc["counts"], gc["group_sizes"].astype(np.int64)
    live_all = (gc["rows"]["count_flags"] >> 31) == 0
    nq, ng = gc["row_begin"].shape[0], counts.shape[1]
    pl = ws.pair_list(ng) if pairs else []
    stats, prs = np.zeros((nq, ng), QueryResult.WINDOW_DTYPE), np.zeros((nq, len(pl)), QueryResult.WINDOW_PAIR_DTYPE)
    cn = 2 * sizes
    gi, hi = (np.array([p[k] for p in pl], np.int64) for k in (0, 1)) if pl else (None, None)
    for q in range(nq):
        a0, nv = int(gc["row_begin"][q]), int(gc["row_count"][q])
        live = live_all[a0:a0 + nv]
        ac = counts["alt_alleles"][a0:a0 + nv].astype(np.int64)[live]
        het = (counts["carriers"][a0:a0 + nv].astype(np.int64) - counts["hom_alt"][a0:a0 + nv].astype(np.int64))[live]
        total = ac.sum(axis=1, keepdims=True)
        s = stats[q]
        s["rows"] = ac.shape[0]
        s["seg"] = ((ac > 0) & (ac < cn)).sum(axis=0)
        s["singletons"] = (ac == 1).sum(axis=0)
        s["doubletons"] = (ac == 2).sum(axis=0)
        s["private"] = ((ac > 0) & (ac == total)).sum(axis=0)
        s["fixed"] = ((cn > 0) & (ac == cn)).sum(axis=0)
        s["sum_ac"] = ac.sum(axis=0)
        s["sum_ac2"] = (ac * ac).sum(axis=0)
        s["obs_het"] = het.sum(axis=0)
        if pl:   # every pair at once: rows x P
            a, b = ac[:, gi], ac[:, hi]
            prs["sum_cross"][q] = (a * b).sum(axis=0)
            prs["seg_union"][q] = ((a + b > 0) & (a + b < cn[gi] + cn[hi])).sum(axis=0)
            prs["fixed_diff"][q] = ((cn[gi] > 0) & (cn[hi] > 0) & (((a == 0) & (b == cn[hi])) | ((a == cn[gi]) & (b == 0)))).sum(axis=0)
    return stats, prs


def _groups_arg(members, names):
    return dict(zip(names, members)) if names is not None else members


def _check_arrays(vs, regions, members, got, pairs):
    gres = vs.group_counts(regions, members)
    want_stats, want_pairs = reduce_numpy(gres.group_counts(), pairs)
    gres.close()
    assert np.array_equal(got["stats"], want_stats)
    assert np.array_equal(got["pairs"], want_pairs) and got["pairs"].shape == want_pairs.shape


def _check_small(vs, regions, want, members, names, pairs, arrays=True):
    """Every region's text against the reference's text of the oracle's type-6 text, and the arrays against the numpy reduction of
    group_counts of the same call.  -> (the accessor's dict, the reference's records per region or None)."""
    group_of = {vs.sample_name(i): g for g, m in enumerate(members) for i in m}
    res = vs.window_stats(regions, _groups_arg(members, names), pairs=pairs)
    got = res.window_stats(lengths=[max(1, y - x) for x, y in regions])
    got["dropped"] = (res.raw(with_carriers=False)["rows"]["count_flags"] >> 31).astype(bool)   # per table row of THIS result
    refs, checked = [], 0
    for q, (n, _early, text) in enumerate(want):
        if n < 0:
            refs.append(None)   # the reference does not terminate on this region
            continue
        recs, prs, sizes = ws.region_records(text, group_of, len(members), pairs)
        refs.append((recs, prs))
        assert res.region_text(q) == ws.text(recs, prs, sizes, names), (q, regions[q])
        assert tuple(got["stats"][q, 0]) == tuple(recs[0][f] for f in ws.FIELDS)
        checked += 1
    assert checked > 0
    assert list(got["group_sizes"]) == [len(set(m)) for m in members]
    assert got["group_names"] == (names if names is not None else [str(g) for g in range(len(members))])
    npair = len(members) * (len(members) - 1) // 2 if pairs else 0
    assert got["stats"].shape == (len(regions), len(members)) and got["pairs"].shape == (len(regions), npair)
    assert got["pair_index"].tolist() == ([list(p) for p in ws.pair_list(len(members))] if npair else [])
    if arrays:
        _check_arrays(vs, regions, members, got, pairs)
    res.close()
    return got, refs


@pytest.mark.parametrize("stem", ["x", "x.small"])
def test_golden_region_sweeps(stem, golden_dir, tmp_path):
    fasta, vcf = os.path.join(golden_dir, stem + ".fa"), os.path.join(golden_dir, stem + ".vcf")
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(11)
    regions = random_regions(rng, _ref_len(fasta), 200)   # unsorted: the device sorts the batch
    want = oracle_texts(orc, regions)
    order = sorted(range(len(regions)), key=lambda i: regions[i])
    srt, want_srt = [regions[i] for i in order], [want[i] for i in order]
    ns = vs.info().num_samples - 1
    for k, members in enumerate(_small_groupings(rng, ns)):
        names = [f"grp {g}" for g in range(len(members))]
        for nm in (names, None):
            for pairs in (True, False):
                _check_small(vs, regions, want, members, nm, pairs, arrays=nm is None)
                _check_small(vs, srt, want_srt, members, nm, pairs, arrays=nm is None)
    # groups=None: the whole cohort as one group
    listed = vs.window_stats(regions, [list(range(1, ns + 1))])
    everyone = listed.window_stats()
    listed.close()
    res = vs.window_stats(regions)
    whole = res.window_stats()
    assert np.array_equal(whole["stats"], everyone["stats"]) and whole["pairs"].shape == (len(regions), 0)
    assert list(whole["group_sizes"]) == [ns] and whole["group_names"] == ["0"]
    assert res.region_text(3).startswith(ws.HEADER + f"0\t{ns}\t")
    view = res.region_window_stats(3, whole)
    assert np.array_equal(view["stats"], whole["stats"][3]) and view["pi"].shape == (1,)
    res.close()
    vs.close()


@pytest.mark.parametrize("seed", [701, 702, 703])
def test_random_cohorts_with_duplicate_rule(seed, tmp_path):
    fasta, vcf, names = write_random_cohort(str(tmp_path), seed, ref_len=6000, n_rows=400, n_samples=9, p_near=0.6, p_multi=0.3,
                                            p_same=0.3, unphased_p=0.4 if seed % 2 else 0.05, haploid_p=0.1 if seed == 703 else 0.0)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(seed)
    regions = random_regions(rng, 6000, 200, max_len=900)
    regions += [regions[7], regions[7]]                                                   # a region given twice (three times in all)
    regions += [(x, x + 1500) for x in range(40, 2400, 23)]                               # heavily overlapping
    regions += [(x, x + 4) for x in range(3000, 3400, 9)]                                 # a handful of bases: no row, or one
    want = oracle_texts(orc, regions)   # (dropped rows are not in the oracle's text: they must add to nothing, `rows` included)
    assert any(n == 0 for n, _e, _t in want) and any(n == 1 for n, _e, _t in want), "no region of 0 rows / of 1 row"
    t6 = vs.get_var_in_ref(regions).raw(with_carriers=False)
    dropped = (t6["rows"]["count_flags"] >> 31).astype(bool)
    assert dropped.any(), "no region of the batch falls under the duplicate rule"
    for k, members in enumerate(_small_groupings(rng, len(names))):
        got, refs = _check_small(vs, regions, want, members, [f"g{g}" for g in range(len(members))], True)
        if k == 0:   # `rows` leaves the dropped rows out: fewer than the region's slots where one was dropped
            nd = np.array([int(got["dropped"][int(a):int(a) + int(c)].sum()) for a, c in zip(got["row_begin"], got["row_count"])])
            assert nd.any() and np.array_equal(got["stats"]["rows"][:, 0].astype(np.int64), got["row_count"].astype(np.int64) - nd)
        if k in (1, 3):   # the accessor's float64 values: against Fractions within the derived bounds, and against counted pairs
            live = [q for q, r in enumerate(refs) if r is not None]
            sub = {key: got[key][live] for key in ("pi", "theta_w", "tajima_d", "het_obs", "dxy", "fst_hudson")}
            sizes = [len(set(m)) for m in members]
            ws.check_derived(sub, [refs[q][0] for q in live], [refs[q][1] for q in live], sizes)
            sets = [{vs.sample_name(i) for i in m} for m in members]
            for q in live[:40]:
                pi, dxy, fst = ws.brute_force(want[q][2], sets)
                for g, v in enumerate(pi):
                    assert (math.isnan(got["pi"][q, g]) if v is None else abs(got["pi"][q, g] - float(v)) <= 4 * ws.U * float(v)), (q, g)
                for p, (d, f) in enumerate(zip(dxy, fst)):
                    assert (math.isnan(got["dxy"][q, p]) if d is None else abs(got["dxy"][q, p] - float(d)) <= 4 * ws.U * float(d)), (q, p)
                    assert (math.isnan(got["fst_hudson"][q, p]) if f is None
                            else abs(got["fst_hudson"][q, p] - float(f)) <= 8 * ws.U * (1 + abs(1 - float(f)))), (q, p)
    _check_small(vs, regions, want, _small_groupings(rng, len(names))[1], None, False)
    vs.close()


@pytest.fixture(scope="module")
def t6_store():
    vs = VariantStore.synthetic(device=0, **T6_KW)
    rng = np.random.default_rng(31)
    s = np.sort(rng.integers(1_000, 7_990_000, size=4_000))
    regions = np.stack([s, s + rng.integers(50, 3_000, size=s.shape[0])], axis=1).astype(np.uint64)
    yield vs, regions
    vs.close()


@pytest.mark.parametrize("n_groups", [1, 2, 3, 8, 9, 33, 64])
def test_group_counts_around_the_padding_edges(t6_store, n_groups, tmp_path):
    """300 samples.  The group kernel pads the groups to 1, 2, 4, 8, 16 and 64; the reduction's lanes own floor(64 / G) row slices and
    min(P, 64) pairs a pass: P = 0, 1, 3, 28 and 36 (below 64: row slices of pairs), 528 and 2,016 (16 and 32 pairs a lane)."""
    vs, regions = t6_store
    rng = np.random.default_rng(n_groups)
    label = _partition(rng, vs.info().num_samples - 1, n_groups, unlisted=0.0 if n_groups == 1 else 0.2)
    members = _members(label, n_groups)
    per_wave = rows_per_wave(n_groups)
    for n in range(400, 500):   # a batch whose table ends inside a wave's rows of the group kernel
        res = vs.window_stats(regions[:n], members)
        a = res.layout()[1]
        if a % per_wave and a % 64:
            break
        res.close()
    assert a % per_wave != 0 and a % 64 != 0 and a > 4 * per_wave
    got = res.window_stats()
    assert got["pairs"].shape == (n, n_groups * (n_groups - 1) // 2)
    _check_arrays(vs, regions[:n], members, got, True)
    assert got["stats"]["seg"].any() and got["stats"]["private"].any() and (n_groups == 1 or got["pairs"]["sum_cross"].any())
    # a few regions against the oracle's text as well, and the same regions as a batch of their own
    orc = _oracle(vs, tmp_path)
    ids_of = {vs.sample_name(i): i for i in range(1, vs.info().num_samples)}
    few = [tuple(int(v) for v in r) for r in regions[:12]]
    small = vs.window_stats(few, members)
    for q, (cnt, _e, text) in enumerate(oracle_texts(orc, few)):
        if cnt >= 0:
            recs, prs, sizes = ws.parsed_records(parse_region(text, ids_of), label, n_groups)
            assert res.region_text(q) == small.region_text(q) == ws.text(recs, prs, sizes), (q, n_groups)
    nop = vs.window_stats(regions[:n], members, pairs=False)
    plain = nop.window_stats()
    assert np.array_equal(plain["stats"], got["stats"]) and plain["pairs"].shape == (n, 0)
    nop.close(); small.close(); res.close()


def _regions_of_row_counts(vs, targets, rng):
    """Regions of the synthetic store that report exactly the wanted numbers of rows, found by asking."""
    table = vs.get_var_in_ref([(1_000, 400_000)])
    pos = np.unique(table.raw(with_carriers=False)["rows"]["pos"].astype(np.int64))
    table.close()
    cand = [(int(pos[i]), int(pos[i + k - 1 + d]) + 1, k) for k in targets for i in rng.integers(10, pos.shape[0] - 450, size=12)
            for d in (-1, 0, 1)]   # (two rows at one position, a deletion reaching in: a span of k positions need not report k rows)
    res = vs.allele_counts([(x, y) for x, y, _k in cand])
    rc = res.allele_counts()["row_count"]
    res.close()
    out = {}
    for (x, y, k), c in zip(cand, rc):
        if int(c) == k:
            out.setdefault(k, (x, y))
    assert sorted(out) == sorted(targets), (sorted(out), targets)
    return out


@pytest.mark.parametrize("n_groups", [3, 26])
def test_split_regions_give_the_same_bytes(n_groups):
    """window_chunk = 64: regions of 63 and 64 rows stay whole, 65, 128, 129 and 400 rows are split into 2, 2, 3 and 7 chunks whose
    workgroups add with atomics -- the same bytes as with the default chunk, twice on a recycled pool, between short regions."""
    vs = VariantStore.synthetic(device=0, **T6_KW)
    rng = np.random.default_rng(5)
    long_ = _regions_of_row_counts(vs, (63, 64, 65, 128, 129, 400), rng)
    s = np.sort(rng.integers(1_000, 7_990_000, size=300))
    short = [(int(x), int(x) + int(rng.integers(50, 3_000))) for x in s]
    regions = sorted(short + list(long_.values()) + [long_[400], long_[65]])   # (two of the long ones twice)
    members = _members(_partition(rng, T6_KW["num_samples"], n_groups, unlisted=0.1), n_groups)
    base = vs.window_stats(regions, members)
    want = base.window_stats()
    base.close()
    assert {63, 64, 65, 128, 129, 400} <= set(int(c) for c in want["row_count"])
    _check_arrays(vs, regions, members, want, True)
    vs.set_option("window_chunk", 64)
    try:
        for _round in range(2):
            res = vs.window_stats(regions, members)
            got = res.window_stats()
            assert np.array_equal(got["stats"], want["stats"]) and np.array_equal(got["pairs"], want["pairs"])
            res.close()
            other = vs.genotype_matrix(regions[:150])   # a result of another shape in between: the pool hands its buffer back dirty
            assert other.totals()[2] > 0
            other.close()
        shuffled = [regions[i] for i in rng.permutation(len(regions))]
        res = vs.window_stats(shuffled, members, pairs=False)
        got = res.window_stats()
        back = {r: i for i, r in enumerate(regions)}
        assert np.array_equal(got["stats"], want["stats"][[back[r] for r in shuffled]])
        res.close()
    finally:
        vs.set_option("window_chunk", 0)
    for bad in (1, 63, 65537):
        with pytest.raises(VariantStoreError) as e:
            vs.set_option("window_chunk", bad)
        assert e.value.code == VS_ERR_ARG
    vs.close()


@pytest.fixture(scope="module", params=[(8255, 150), (12000, 150)], ids=["8255", "12000"])
def saturated(request, tmp_path_factory):
    n, rows = request.param
    tmp = tmp_path_factory.mktemp(f"winsat{n}")
    fasta, vcf = write_saturated_cohort(str(tmp), n, 5100 + n, rows=rows, two_alt=False)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = vt.TextOracle(vcf)
    ids_of = {nm: i + 1 for i, nm in enumerate(orc.names)}
    cnt, _e, text = orc.get_var_in_ref(1, SAT_REF_LEN + 1)
    assert cnt == rows
    yield vs, n, parse_region(text, ids_of)
    vs.close()


def test_sums_beyond_32_bits(saturated):
    """One region over all 150 rows of a saturated cohort, as one group and as two halves.  At 8,255 samples the reference gives
    sum_ac2 = 1.4e10 (one group) but sum_cross = 3.5e9, below 2^32 -- the rows are carried by hets mostly, ac is near 9,500, not
    14,000 -- and the helper's 20,000-base reference holds no more than 158 rows; so the assertion on sum_cross is made on a second
    cohort of 12,000 samples (7.4e9), and on sum_ac2 on both."""
    vs, n, parsed = saturated
    region = [(1, SAT_REF_LEN + 1)]
    one = np.zeros(n + 1, np.int64)
    one[0] = -1
    halves = (np.arange(n + 1) > n // 2).astype(np.int64)
    halves[0] = -1
    for label, n_groups in ((one, 1), (halves, 2)):
        recs, prs, sizes = ws.parsed_records(parsed, label, n_groups)
        print(n, n_groups, [r["sum_ac2"] for r in recs], [p["sum_cross"] for p in prs])
        if n_groups == 1:
            assert recs[0]["sum_ac2"] > 1 << 32
        elif n >= 12000:
            assert prs[0]["sum_cross"] > 1 << 32 and min(r["sum_ac2"] for r in recs) > 1 << 32
        res = vs.window_stats(region, _members(label, n_groups))
        assert res.region_text(0) == ws.text(recs, prs, sizes)
        got = res.window_stats()
        assert [int(got["stats"]["sum_ac2"][0, g]) for g in range(n_groups)] == [r["sum_ac2"] for r in recs]
        assert [int(v) for v in got["pairs"]["sum_cross"][0]] == [p["sum_cross"] for p in prs]
        for g in range(n_groups):   # (N sum_ac - sum_ac2 leaves 2^53 here and is still formed exactly: uint64)
            pi = float(ws.exact_pi(recs[g], sizes[g]))
            assert abs(got["pi"][0, g] - pi) <= 3 * ws.U * pi
        res.close()
    whole = vs.window_stats(region)
    assert whole.region_text(0) == ws.text(*ws.parsed_records(parsed, one, 1))
    whole.close()


def test_device_regions_and_device_pointers(t6_store):
    torch = pytest.importorskip("torch")
    vs, regions = t6_store
    members = [[3, 17, 40], [200, 201, 202, 299], list(range(60, 70))]
    hres = vs.window_stats(regions, members)
    host = hres.window_stats()
    t = torch.from_numpy(regions.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    dres = vs.window_stats(DeviceArray(t.data_ptr(), regions.shape[0]), members)
    dev = dres.window_stats()
    for k in ("stats", "pairs", "group_sizes", "row_begin", "row_count", "flags"):
        assert np.array_equal(host[k], dev[k]), k
    dres.close()
    d = hres.window_stats_device()
    assert (d["n_regions"], d["n_groups"], d["n_pairs"]) == (regions.shape[0], 3, 3) and d["stats"] and d["pairs"]
    later = vs.window_stats(regions[:500], members)   # a later batch on the same handle leaves the records alone
    later.totals()
    stats = _read_device(torch, d["stats"], regions.shape[0], 3 * 48).view(QueryResult.WINDOW_DTYPE).reshape(-1, 3)
    prs = _read_device(torch, d["pairs"], regions.shape[0], 3 * 16).view(QueryResult.WINDOW_PAIR_DTYPE).reshape(-1, 3)
    assert np.array_equal(stats, host["stats"]) and np.array_equal(prs, host["pairs"]) and host["stats"]["sum_ac"].any()
    nop = vs.window_stats(regions[:500], members, pairs=False)
    assert nop.window_stats_device()["pairs"] == 0 and nop.window_stats_device()["n_pairs"] == 0
    nop.close(); later.close(); hres.close()


def test_totals_layout_view_and_refused_accessors(t6_store):
    vs, regions = t6_store
    members = [[1, 2, 9], [3], list(range(100, 200))]
    r = vs.window_stats(regions[:1_000], members)
    g = vs.group_counts(regions[:1_000], members)
    t6 = vs.get_var_in_ref(regions[:1_000])
    assert r.totals() == g.totals() and r.totals()[:2] == t6.totals()[:2]
    assert r.layout() == g.layout() and r.layout()[2] == 0 and r.layout()[3] == 0
    assert r.fill_ms() > 0
    raw, graw = r.raw(with_carriers=False), g.raw(with_carriers=False)
    for f in raw["rows"].dtype.names:
        assert np.array_equal(raw["rows"][f], graw["rows"][f]), f
    r.view(with_carriers=False)
    for call in (lambda: r.raw(with_carriers=True), lambda: r.view(with_carriers=True), r.digest, r.num_header_records,
                 r.num_region_records):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_UNSUPPORTED
    for call in (r.allele_counts, r.group_counts, r.group_counts_device, r.sample_burden, r.genotype_matrix, r.ld_band, r.ld_scores):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_ARG
    for other in (g, t6):
        for call in (other.window_stats, other.window_stats_device):
            with pytest.raises(VariantStoreError) as e:
                call()
            assert e.value.code == VS_ERR_ARG
    r.close(); g.close(); t6.close()


def test_interleaving_leaves_type6_and_group_counts_alone():
    rng = np.random.default_rng(12)
    batches = []
    for k in range(8):
        n = 3_000 + 200 * k + (4_000 if k == 5 else 0)   # like batches (speculated), one larger (refused / re-sized)
        s = np.sort(rng.integers(1_000, 7_990_000, size=n))
        batches.append(np.stack([s, s + rng.integers(50, 3_000, size=n)], axis=1).astype(np.uint64))
    shuffled = batches[3][rng.permutation(batches[3].shape[0])]
    groups = {"a": range(1, 150), "b": range(150, 301)}

    def run(with_windows):
        vs = VariantStore.synthetic(device=0, **T6_KW)
        answers = []
        for k, b in enumerate(batches):
            r = vs.get_var_in_ref(b)
            g = vs.group_counts(b[:500], groups)
            if with_windows:   # window batches in between: sorted, unsorted, without pairs
                w1 = vs.window_stats(b, groups)
                w2 = vs.window_stats(shuffled, [[1, 5, 7], [200], []], pairs=False)
                w1.totals(); w2.totals()
                w1.close(); w2.close()
            answers.append((r.digest(), g.group_counts()["counts"].tobytes()))
            r.close(); g.close()
        info = vs.info()
        out = (answers, info.t6_speculated, info.t6_refused)
        vs.close()
        return out

    plain, mixed = run(False), run(True)
    assert plain[1] > 0, "the type-6 batches were not speculated"
    assert plain == mixed


def test_size_limit_comes_before_allocation(t6_store):
    vs, regions = t6_store
    members = _members(_partition(np.random.default_rng(2), 300, 40), 40)
    ok = vs.window_stats(regions, members)
    a = ok.layout()[1]
    ok.close()
    q, g, p = regions.shape[0], 40, 40 * 39 // 2
    tmp_bytes, out_bytes = a * g * 16, q * (48 * g + 16 * p)
    assert tmp_bytes > 1 << 20 and out_bytes > 1 << 20
    vs.set_option("matrix_max_mib", 1)
    try:
        with pytest.raises(VariantStoreError) as e:
            vs.window_stats(regions, members)
        assert e.value.code == VS_ERR_ARG
        msg = str(e.value)
        assert f"{a} rows" in msg and "40 groups" in msg and str(tmp_bytes + out_bytes) in msg and "matrix_max_mib" in msg, msg
        with pytest.raises(VariantStoreError) as e:   # the records alone are too many as well
            vs.window_stats(regions, members[:1] + [[] for _ in range(39)])
        assert e.value.code == VS_ERR_ARG
        few = vs.window_stats(regions[:200], members[:2])   # a request below the limit is answered meanwhile
        got = few.window_stats()
        assert got["stats"].shape == (200, 2) and got["stats"]["rows"].any()
        few.close()
    finally:
        vs.set_option("matrix_max_mib", 0)
    again = vs.window_stats(regions, members)
    assert again.window_stats()["pairs"].shape == (q, p)
    again.close()


def test_cli_windows(tmp_path):
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
    groups = {"controls": names[5:9], "cases": names[:4], "other pop": names[10:11]}   # (names[4], [9], [11] ...: in no group)
    gfile = os.path.join(tmp_path, "groups.txt")
    with open(gfile, "w") as f:   # groups in order of first appearance; tab or space; a blank line; a pair given twice
        f.write(f"{names[5]}\tcontrols\n{names[0]} cases\n\n{names[10]}\tother pop\n{names[0]}\tcases\n")
        f.write("".join(f"{n}\tcontrols\n" for n in names[6:9]) + "".join(f"{n} cases\n" for n in names[1:4]))

    def run(*more):
        out = os.path.join(tmp_path, "windows_out.txt")
        subprocess.run([exe, "windows", "-p", prefix, "-r", "@" + rfile, "-o", out, *more], check=True, capture_output=True)
        with open(out) as f:
            parts = f.read().split("#region ")[1:]
        assert len(parts) == len(regions)
        texts = []
        for q, part in enumerate(parts):
            head, text = part.split("\n", 1)
            assert head == f"{q} {regions[q][0]}:{regions[q][1]}"
            texts.append(text)
        return texts

    for kw, args in ((dict(groups=groups), ("-G", gfile)), (dict(groups=groups, pairs=False), ("-G", gfile, "--no-pairs")), (dict(), ())):
        res = vs.window_stats(regions, **kw)
        for q, text in enumerate(run(*args)):
            assert text == res.region_text(q), (q, args)
        res.close()
    # --derived: the same lines with Pi ThetaW TajimaD per group and Dxy Fst per pair, ten digits: 5e-10 relative
    res = vs.window_stats(regions, groups)
    got = res.window_stats()
    seen = 0
    for q, text in enumerate(run("-G", gfile, "--derived")):
        lines, plain = text.split("\n"), res.region_text(q).split("\n")
        assert len(lines) == len(plain) == 1 + 3 + 1 + 3 + 1
        assert lines[0] == plain[0] + "\tPi\tThetaW\tTajimaD" and lines[4] == plain[4] + "\tDxy\tFst"
        for row, base in ((1, 0), (5, 0)):
            for k in range(3):
                fields = lines[row + k].split("\t")
                n_int = len(plain[row + k].split("\t"))
                assert "\t".join(fields[:n_int]) == plain[row + k]
                want = ([got[key][q, k] for key in ("pi", "theta_w", "tajima_d")] if row == 1 else [got[key][q, k] for key in ("dxy", "fst_hudson")])
                assert len(fields) == n_int + len(want)
                for s, w in zip(fields[n_int:], want):
                    if math.isnan(w):
                        assert s == "nan", (q, row, k)
                    else:
                        assert abs(float(s) - w) <= 5e-10 * abs(w) + 1e-300, (q, row, k, s, w)
                        seen += 1
    assert seen > 200
    res.close()
    vs.close()
