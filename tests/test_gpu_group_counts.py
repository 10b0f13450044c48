"""Grouped allele counts on the GPU (vs_query_group_counts): every region's text against counts worked out from the oracle's
type-6 text, column g against the existing count query with group g as the subset, the three storage forms of the genotype bits,
the class-row widths of 63 and 64 words, tables that end inside a wave's rows for every rows-per-wave the kernel chooses, a recycled
buffer, interleaving with type-6 batches, regions in device memory, the device pointer, the refused accessors, the size limit and
the CLI."""
import os
import subprocess

import numpy as np
import pytest

from group_counts_ref import groups_text, parse_region, parsed_groups_text
from helpers import oracle_texts, random_regions, write_random_cohort
from oracle.oracle import Oracle
from test_gpu_genotype_matrix import _read_device
from test_gpu_row_width_edges import SPREAD_KW, SPREAD_SEED
from variantstore_amd import DeviceArray, VariantStore
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_ARG, VS_ERR_UNSUPPORTED = -5, -7
FIELDS = ("carriers", "alt_alleles", "hom_alt", "phased")


def rows_per_wave(n_groups):
    """What k_group_counts chooses: 512 accumulator cells a wave, the groups padded to a power of two, at most 64 rows."""
    gp = 1
    while gp < n_groups:
        gp *= 2
    return min(64, 512 // gp)


def _oracle(vs, tmp_path, name="plain.bin"):
    plain = os.path.join(tmp_path, name)
    vs.export_plain(plain)
    return Oracle(plain)


def _ref_len(fasta):
    with open(fasta) as f:
        return sum(len(line.strip()) for line in f if not line.startswith(">"))


def _partition(rng, ns, n_groups, unlisted=0.0):
    """label[id] for id 0 .. ns: a random group per sample, -1 for "ref" and for a share `unlisted` of the samples."""
    label = rng.integers(0, n_groups, size=ns + 1)
    label[rng.random(ns + 1) < unlisted] = -1
    label[0] = -1
    return label


def _members(label, n_groups):
    return [[int(i) for i in np.nonzero(label == g)[0]] for g in range(n_groups)]


def _check_small(vs, regions, want, members, names):
    """Every region's text against groups_text of the oracle's type-6 text; `members`: sample ids per group, names: the groups'
    names or None (then the query is made without names)."""
    group_of = {vs.sample_name(i): g for g, m in enumerate(members) for i in m}
    res = vs.group_counts(regions, dict(zip(names, members)) if names is not None else members)
    checked = 0
    for q, (n, _early, text) in enumerate(want):
        if n < 0:
            continue   # the reference does not terminate on this region
        assert res.region_text(q) == groups_text(text, group_of, len(members), names), (q, regions[q])
        checked += 1
    assert checked > 0
    got = res.group_counts()
    assert list(got["group_sizes"]) == [len(set(m)) for m in members]
    assert got["group_names"] == (names if names is not None else [str(g) for g in range(len(members))])
    res.close()


def _small_groupings(rng, n_samples):
    """G = 1 (everyone), G = 2 with samples unlisted, a group per sample, a grouping with an empty group, duplicate pairs."""
    ids = list(range(1, n_samples + 1))
    half = [i for i in ids if rng.random() < 0.4]
    rest = [i for i in ids if i not in half and rng.random() < 0.7]
    out = [[ids], [half or ids[:1], rest], [[i] for i in ids], [ids[: (n_samples + 1) // 2], [], ids[(n_samples + 1) // 2:]],
           [ids[:1] + ids[:1], ids[1:] + ids[1:2]]]
    return out


@pytest.mark.parametrize("stem", ["x", "x.small"])
def test_golden_region_sweeps(stem, golden_dir, tmp_path):
    fasta, vcf = os.path.join(golden_dir, stem + ".fa"), os.path.join(golden_dir, stem + ".vcf")
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(11)
    regions = random_regions(rng, _ref_len(fasta), 200)   # unsorted: the device sorts the batch
    want = oracle_texts(orc, regions)
    order = sorted(range(len(regions)), key=lambda i: regions[i])
    for members in _small_groupings(rng, vs.info().num_samples - 1):
        names = [f"grp {g}" for g in range(len(members))]
        for nm in (names, None):
            _check_small(vs, regions, want, members, nm)
            _check_small(vs, [regions[i] for i in order], [want[i] for i in order], members, nm)
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
    want = oracle_texts(orc, regions)   # (dropped rows are not in the oracle's text: they must print nothing)
    for members in _small_groupings(rng, len(names)):
        _check_small(vs, regions, want, members, [f"g{g}" for g in range(len(members))])
    _check_small(vs, regions, want, _small_groupings(rng, len(names))[1], None)
    vs.close()


def _check_parsed(vs, regions, parsed, label, n_groups, names=None):
    members = _members(label, n_groups)
    res = vs.group_counts(regions, dict(zip(names, members)) if names is not None else members)
    for q, p in enumerate(parsed):
        if p is not None:
            assert res.region_text(q) == parsed_groups_text(p, label, n_groups, names), (q, regions[q], n_groups)
    out = res.group_counts()
    res.close()
    return out


@pytest.mark.parametrize("shape", ["narrow_dense", "wide", "explicit"])
def test_storage_forms(shape, tmp_path):
    """gt_groups (1,500 samples, dense rows: the staged row path), gt_nibbles of a 4,100-sample class-row cohort, and the unpadded
    pool of a 10,000-sample explicit-id cohort: short scattered regions and long overlapping ones, sorted and shuffled, G = 3 with a
    third of the samples unlisted and G = 64."""
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
    ns = info.num_samples - 1
    orc = _oracle(vs, tmp_path)
    ids_of = {vs.sample_name(i): i for i in range(1, ns + 1)}
    rng = np.random.default_rng(6)
    starts = np.sort(rng.integers(3_000, 1_495_000, size=600))
    short = [(int(x), int(x) + 25) for x in starts]
    n_long = 24 if shape == "explicit" else 6   # (the class-row cohorts: some hundred carriers a row, every one parsed from the oracle's text)
    base = int(rng.integers(3_000, 1_400_000))
    long_ = sorted((int(x), int(x) + int(rng.integers(5_000, 20_000))) for x in base + rng.integers(0, 15_000, size=n_long))
    # G = 3: group 0 the contiguous ids 40 .. 150 (it straddles the word boundaries at 64 and 128), the rest at random, a third unlisted,
    # the last sample in group 2; G = 64: a random partition, the last sample in group 63, ids 100 .. 140 in group 7
    lab3 = _partition(rng, ns, 3, unlisted=1 / 3)
    lab3[40:151] = 0
    lab3[ns] = 2
    lab64 = _partition(rng, ns, 64)
    lab64[100:141] = 7
    lab64[ns] = 63
    names3 = ["cases", "controls", "other"]
    dense_seen = 0
    for regions in (short, long_):
        parsed = [parse_region(text, ids_of) if n >= 0 else None for n, _e, text in oracle_texts(orc, regions)]
        perm = rng.permutation(len(regions))
        for rr, pp in ((regions, parsed), ([regions[i] for i in perm], [parsed[i] for i in perm])):
            got = _check_parsed(vs, rr, pp, lab3, 3, names3)
            _check_parsed(vs, rr, pp, lab64, 64)
            dense_seen = max(dense_seen, int((got["rows"]["count_flags"] & 0x7FFFFFFF).max()))
    if shape == "narrow_dense":   # the dense path ran: rows with more carriers than a decoded list holds
        assert dense_seen > info.list_max
    vs.close()


@pytest.fixture(scope="module")
def mid_store():
    vs = VariantStore.synthetic(device=0, ref_length=40_000_000, num_variants=1_000_000, num_samples=2_504, seed=21, first_pos=1_000,
                                frac_ins=0.05, frac_del=0.05, frac_multi=0.02, max_indel=6, af_exponent=2.5)
    rng = np.random.default_rng(4)
    starts = np.sort(rng.integers(1_000, 39_990_000, size=20_000))
    regions = np.stack([starts, starts + rng.integers(100, 5_000, size=starts.shape[0])], axis=1).astype(np.uint64)
    yield vs, regions
    vs.close()


def _column_equals_subset(vs, regions, counts, members, groups):
    """counts[:, g] == allele_counts(regions, group g) field by field, for the groups asked for."""
    for g in groups:
        r = vs.allele_counts(regions, members[g])
        cc = r.allele_counts()["counts"]
        r.close()
        for f in FIELDS:
            assert np.array_equal(counts[f][:, g], cc[f]), (g, f)


@pytest.mark.parametrize("n_groups", [5, 26, 64])
def test_columns_equal_the_subset_counts(mid_store, n_groups):
    vs, regions = mid_store
    ns = vs.info().num_samples - 1
    rng = np.random.default_rng(100 + n_groups)
    label = _partition(rng, ns, n_groups, unlisted=0.1)
    members = _members(label, n_groups)
    res = vs.group_counts(regions, members)
    got = res.group_counts()
    counts = got["counts"]
    assert counts.shape[1] == n_groups and counts.shape[0] > 200_000
    assert list(got["group_sizes"]) == [len(m) for m in members]
    _column_equals_subset(vs, regions, counts, members, range(n_groups) if n_groups < 64 else range(3, 64, 8))
    listed = vs.allele_counts(regions, [i for m in members for i in m])
    whole = listed.allele_counts()["counts"]
    listed.close()
    for f in FIELDS:   # the groups are disjoint: they add up to the count over all listed samples
        assert np.array_equal(counts[f].astype(np.int64).sum(axis=1), whole[f].astype(np.int64)), f
    # totals: the carriers of the rows every region reports, over all groups
    car = counts["carriers"].astype(np.int64).sum(axis=1)
    pre = np.concatenate([[0], np.cumsum(car)])
    rb, rc = got["row_begin"].astype(np.int64), got["row_count"].astype(np.int64)
    t6 = vs.get_var_in_ref(regions)
    assert res.totals()[:3] == (regions.shape[0], t6.totals()[1], int((pre[rb + rc] - pre[rb]).sum()))
    t6.close()
    res.close()


def test_full_partition_rows_and_accessors(mid_store):
    vs, regions = mid_store
    ns = vs.info().num_samples - 1
    label = _partition(np.random.default_rng(9), ns, 7)
    res = vs.group_counts(regions, _members(label, 7))
    got = res.group_counts()
    cres = vs.allele_counts(regions)
    whole = cres.allele_counts()["counts"]
    for f in FIELDS:   # a full partition: the groups add up to the whole cohort
        assert np.array_equal(got["counts"][f].astype(np.int64).sum(axis=1), whole[f].astype(np.int64)), f
    t6 = vs.get_var_in_ref(regions)
    raw6 = t6.raw(with_carriers=False)
    for f in raw6["rows"].dtype.names:
        if f != "car_begin":
            assert np.array_equal(raw6["rows"][f], got["rows"][f]), f
    assert np.array_equal(raw6["region_flags"], got["flags"])
    assert np.array_equal(raw6["row_begin"], got["row_begin"]) and np.array_equal(raw6["row_count"], got["row_count"])
    assert res.totals()[:3] == cres.totals()[:3] == t6.totals()[:3]
    lay = res.layout()
    assert lay[2] == 0 and lay[3] == 0 and lay[1] == raw6["rows"].shape[0]
    assert res.fill_ms() > 0
    q = int(np.nonzero(got["row_count"] > 1)[0][0])
    rows = res.region_group_counts(q)
    assert len(rows) == int(raw6["var_count"][q]) and list(rows[0]["groups"]) == [str(g) for g in range(7)]
    a = int(got["row_begin"][q])
    for g in range(7):
        cell = rows[0]["groups"][str(g)]
        assert cell["n"] == int((label == g).sum()) and cell["alt_alleles"] == int(got["counts"]["alt_alleles"][a, g])
        assert cell["af"] == cell["alt_alleles"] / (2.0 * cell["n"])
    res.close(); cres.close(); t6.close()


@pytest.mark.parametrize("n_samples", [4031, 4032])
def test_row_width_edges(n_samples, tmp_path, monkeypatch):
    """Class rows of 63 and 64 words (gt_groups' widest, gt_nibbles' narrowest), listed and dense rows together."""
    monkeypatch.setenv("VS_LIST_MAX", "64")
    vs = VariantStore.synthetic(device=0, num_samples=n_samples, seed=SPREAD_SEED[n_samples], **SPREAD_KW)
    info = vs.info()
    assert (info.num_samples + 63) // 64 == (63 if n_samples == 4031 else 64) and info.list_max == 64
    orc = _oracle(vs, tmp_path)
    ids_of = {vs.sample_name(i): i for i in range(1, n_samples + 1)}
    rng = np.random.default_rng(n_samples)
    starts = np.sort(rng.integers(1, info.ref_length - 1500, size=70))
    regions = [(int(s), int(s) + int(rng.integers(750, 1500))) for s in starts]
    parsed = [parse_region(text, ids_of) if n >= 0 else None for n, _e, text in oracle_texts(orc, regions[:30])]
    for n_groups in (4, 64):
        label = _partition(rng, n_samples, n_groups, unlisted=0.1)
        label[n_samples] = n_groups - 1                      # the last bit of the last row word
        label[60:70] = 0                                     # across the first word boundary
        members = _members(label, n_groups)
        got = _check_parsed(vs, regions[:30], parsed, label, n_groups)
        res = vs.group_counts(regions, members)
        got = res.group_counts()
        res.close()
        cnt = got["rows"]["count_flags"] & 0x7FFFFFFF
        assert (cnt > 64).sum() > 20 and ((cnt > 0) & (cnt <= 64)).sum() > 20, "both paths"
        _column_equals_subset(vs, regions, got["counts"], members, range(n_groups) if n_groups == 4 else (0, 31, 63))
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


@pytest.mark.parametrize("n_groups", [3, 16, 26, 64])   # 64, 32, 16 and 8 rows a wave
def test_table_ends_inside_a_wave(t6_store, n_groups):
    vs, regions = t6_store
    label = _partition(np.random.default_rng(n_groups), vs.info().num_samples - 1, n_groups, unlisted=0.2)
    members = _members(label, n_groups)
    per_wave = rows_per_wave(n_groups)
    assert per_wave == {3: 64, 16: 32, 26: 16, 64: 8}[n_groups]
    for n in range(900, 1_000):   # a batch whose table ends inside a wave's rows
        big = vs.group_counts(regions[:n], members)
        a = big.layout()[1]
        if a % per_wave:
            break
        big.close()
    assert a % per_wave != 0 and a > 4 * per_wave
    got = big.group_counts()
    _column_equals_subset(vs, regions[:n], got["counts"], members, (0, n_groups - 1))
    for k in (1, 7, 64):
        small = vs.group_counts(regions[:k], members)
        for q in range(k):
            assert small.region_text(q) == big.region_text(q), (k, q)
        small.close()
    big.close()


def test_recycled_buffer_does_not_show_through():
    """The records land in a buffer the handle's pool hands back dirty: a genotype matrix of at least their size was there before."""
    rng = np.random.default_rng(4)
    s = np.sort(rng.integers(1_000, 7_990_000, size=1_500))
    batch = np.stack([s, s + rng.integers(50, 3_000, size=s.shape[0])], axis=1).astype(np.uint64)
    label = _partition(rng, T6_KW["num_samples"], 19, unlisted=0.5)   # 19 x 16 = 304 bytes a row: the matrix's pitch for 300 samples
    members = _members(label, 19)
    fresh_vs = VariantStore.synthetic(device=0, **T6_KW)
    fresh = fresh_vs.group_counts(batch, members)
    want = fresh.group_counts()
    fresh.close(); fresh_vs.close()
    vs = VariantStore.synthetic(device=0, **T6_KW)
    m = vs.genotype_matrix(batch)
    _ptr, a, _c, pitch = m.genotype_matrix_device()
    assert a * pitch >= want["counts"].nbytes and m.totals()[2] > 0
    m.close()
    res = vs.group_counts(batch, members)
    got = res.group_counts()
    assert np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["rows"], want["rows"])
    res.close(); vs.close()


def test_interleaving_leaves_type6_alone():
    rng = np.random.default_rng(12)
    batches = []
    for k in range(10):
        n = 3_000 + 200 * k + (4_000 if k == 6 else 0)   # like batches (speculated), one larger (refused / re-sized)
        s = np.sort(rng.integers(1_000, 7_990_000, size=n))
        batches.append(np.stack([s, s + rng.integers(50, 3_000, size=n)], axis=1).astype(np.uint64))
    shuffled = batches[3][rng.permutation(batches[3].shape[0])]

    def run(with_groups):
        vs = VariantStore.synthetic(device=0, **T6_KW)
        digests = []
        for k, b in enumerate(batches):
            r = vs.get_var_in_ref(b)
            if with_groups:   # grouped batches in between: sorted, unsorted
                c1 = vs.group_counts(b, {"a": range(1, 150), "b": range(150, 301)})
                c2 = vs.group_counts(shuffled, [[1, 5, 7], [200], []])
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
    members = [[3, 17, 40], [200, 201, 202, 299], list(range(60, 70))]
    hres = vs.group_counts(regions, members)
    host = hres.group_counts()
    t = torch.from_numpy(regions.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    dres = vs.group_counts(DeviceArray(t.data_ptr(), regions.shape[0]), members)
    dev = dres.group_counts()
    for k in ("rows", "counts", "group_sizes", "row_begin", "row_count", "flags"):
        assert np.array_equal(host[k], dev[k]), k
    dres.close()
    ptr, a, g = hres.group_counts_device()
    assert (a, g) == host["counts"].shape and ptr
    later = vs.group_counts(regions[:500], members)   # a later batch on the same handle leaves the records alone
    later.totals()
    words = _read_device(torch, ptr, a, g * 16).view(np.uint32).reshape(a, g, 4)
    for i, f in enumerate(FIELDS):
        assert np.array_equal(words[:, :, i], host["counts"][f]), f
    assert words.any()
    later.close(); hres.close()


def test_refused_accessors(t6_store):
    vs, regions = t6_store
    r = vs.group_counts(regions[:1_000], [[1, 2], [3]])
    for call in (lambda: r.raw(with_carriers=True), lambda: r.view(with_carriers=True), r.digest, r.num_header_records,
                 r.num_region_records):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_UNSUPPORTED
    for call in (r.allele_counts, r.sample_burden, r.sample_burden_device, r.genotype_matrix, r.genotype_matrix_device, r.ld_band):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_ARG
    r.view(with_carriers=False)
    r.close()
    others = (vs.get_var_in_ref(regions[:1_000]), vs.allele_counts(regions[:1_000]), vs.genotype_matrix(regions[:100], [1, 2]))
    for res in others:
        for call in (res.group_counts, res.group_counts_device):
            with pytest.raises(VariantStoreError) as e:
                call()
            assert e.value.code == VS_ERR_ARG
        res.close()


def test_size_limit(t6_store):
    vs, regions = t6_store
    members = _members(_partition(np.random.default_rng(2), 300, 40), 40)
    ok = vs.group_counts(regions, members)
    a = ok.layout()[1]
    ok.close()
    assert a * 40 * 16 > 1 << 20
    vs.set_option("matrix_max_mib", 1)
    try:
        with pytest.raises(VariantStoreError) as e:
            vs.group_counts(regions, members)
        assert e.value.code == VS_ERR_ARG
        msg = str(e.value)
        assert f"{a} rows" in msg and "40 groups" in msg and str(a * 40 * 16) in msg, msg
        few = vs.group_counts(regions[:200], members[:2])   # a request below the limit is answered meanwhile
        got = few.group_counts()["counts"]
        assert got.shape[1] == 2 and 0 < got.nbytes < 1 << 20
        few.close()
    finally:
        vs.set_option("matrix_max_mib", 0)
    again = vs.group_counts(regions, members)
    assert again.group_counts()["counts"].shape == (a, 40)
    again.close()


def test_cli_groups(golden_dir, tmp_path):
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
    groups = {"controls": names[5:9], "cases": names[:4], "other pop": names[10:11]}   # (names[4], [9], [11]: in no group)
    gfile = os.path.join(tmp_path, "groups.txt")
    with open(gfile, "w") as f:   # groups in order of first appearance; tab or space; a blank line; a pair given twice
        f.write(f"{names[5]}\tcontrols\n{names[0]} cases\n\n{names[10]}\tother pop\n{names[0]}\tcases\n")
        f.write("".join(f"{n}\tcontrols\n" for n in names[6:9]) + "".join(f"{n} cases\n" for n in names[1:4]))
    out = os.path.join(tmp_path, "groups_out.txt")
    subprocess.run([exe, "groups", "-p", prefix, "-r", "@" + rfile, "-G", gfile, "-o", out], check=True, capture_output=True)
    with open(out) as f:
        parts = f.read().split("#region ")[1:]
    res = vs.group_counts(regions, groups)
    assert len(parts) == len(regions)
    for q, part in enumerate(parts):
        head, text = part.split("\n", 1)
        assert head == f"{q} {regions[q][0]}:{regions[q][1]}"
        assert text == res.region_text(q), q
    assert any("\tother pop\t1\t" in res.region_text(q) for q in range(len(regions)))
    res.close()
    vs.close()

    def run_bad(text):
        with open(gfile, "w") as f:
            f.write(text)
        p = subprocess.run([exe, "groups", "-p", prefix, "-r", "@" + rfile, "-G", gfile], capture_output=True, text=True)
        assert p.returncode != 0
        return p.stdout + p.stderr

    assert "Sample not found: nobody-of-that-name" in run_bad(f"{names[0]}\ta\nnobody-of-that-name\tb\n")
    assert "two groups" in run_bad(f"{names[0]}\ta\n{names[1]}\tb\n{names[0]}\tb\n")
    assert "more than 64 groups" in run_bad("".join(f"{names[i]}\tg{i}\n" for i in range(65)))
    p = subprocess.run([exe, "groups", "-p", prefix, "-r", "@" + rfile, "-G", gfile, "--nprocs", "2"], capture_output=True, text=True)
    q = subprocess.run([exe, "counts", "-p", prefix, "-r", "@" + rfile, "--nprocs", "2"], capture_output=True, text=True)
    assert p.returncode == q.returncode != 0 and "unknown option --nprocs" in p.stdout + p.stderr   # as `counts` handles it
