"""Allele-count queries on the GPU (vs_query_allele_counts): every region's text against counts worked out from the oracle's
type-6 text (carriers filtered by name), the rows against type 6's, subset identities, the three storage forms of the genotype
bits, interleaving with type-6 batches, regions in device memory, small batches, the refused accessors and the CLI."""
import os
import subprocess

import numpy as np
import pytest

from allele_counts_ref import counts_text
from helpers import oracle_texts, random_regions, write_random_cohort
from oracle.oracle import Oracle
from variantstore_amd import DeviceArray, VariantStore
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_UNSUPPORTED = -7


def _oracle(vs, tmp_path, name="plain.bin"):
    plain = os.path.join(tmp_path, name)
    vs.export_plain(plain)
    return Oracle(plain)


def _names(vs, ids):
    return {vs.sample_name(int(i)) for i in ids}


def _check_texts(vs, regions, want, samples=None, subset_names=None):
    """Every region's count text against the oracle's type-6 text `want` ([(n, early, text)]) filtered to the subset."""
    res = vs.allele_counts(regions, samples)
    checked = 0
    for q, (n, _early, text) in enumerate(want):
        if n < 0:
            continue   # the reference does not terminate on this region
        assert res.region_text(q) == counts_text(text, subset_names), (q, regions[q], samples)
        checked += 1
    assert checked > 0
    res.close()
    return checked


def _ref_len(fasta):
    with open(fasta) as f:
        return sum(len(line.strip()) for line in f if not line.startswith(">"))


@pytest.mark.parametrize("stem", ["x", "x.small"])
def test_golden_region_sweeps(stem, golden_dir, tmp_path):
    fasta, vcf = os.path.join(golden_dir, stem + ".fa"), os.path.join(golden_dir, stem + ".vcf")
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    n_samples = vs.info().num_samples - 1
    rng = np.random.default_rng(11)
    regions = random_regions(rng, _ref_len(fasta), 200)   # unsorted: the device sorts the batch
    want = oracle_texts(orc, regions)
    _check_texts(vs, regions, want)
    _check_texts(vs, sorted(regions), oracle_texts(orc, sorted(regions)))
    for sid in range(1, n_samples + 1):
        _check_texts(vs, regions, want, [vs.sample_name(sid)], {vs.sample_name(sid)})
    for k in range(4):
        ids = rng.choice(np.arange(1, n_samples + 1), size=int(rng.integers(1, n_samples + 1)), replace=False)
        ids = list(ids) + list(ids[:2])   # duplicates count once
        _check_texts(vs, regions, want, [int(i) for i in ids], _names(vs, ids))
    vs.close()


@pytest.mark.parametrize("seed", [701, 702, 703])
def test_random_cohorts_with_duplicate_rule(seed, tmp_path):
    fasta, vcf, names = write_random_cohort(str(tmp_path), seed, ref_len=6000, n_rows=400, n_samples=9, p_near=0.6, p_multi=0.3,
                                            p_same=0.3, unphased_p=0.4 if seed % 2 else 0.05, haploid_p=0.1 if seed == 703 else 0.0)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(seed)
    regions = random_regions(rng, 6000, 300, max_len=900)
    # the plan took the duplicate rule's path: type 6 drops rows in this batch
    t6 = vs.get_var_in_ref(regions).raw(with_carriers=False)
    assert np.any(t6["rows"]["count_flags"] >> 31), "no region of the batch falls under the duplicate rule"
    want = oracle_texts(orc, regions)
    _check_texts(vs, regions, want)
    for k in range(3):
        sub = list(rng.choice(names, size=int(rng.integers(1, len(names))), replace=False))
        _check_texts(vs, regions, want, sub, set(sub))
    vs.close()


@pytest.mark.parametrize("shape", ["narrow_dense", "wide", "explicit"])
def test_storage_forms(shape, tmp_path):
    """gt_groups (<= 4032 samples, dense rows: the subset's row path), gt_nibbles of a 4,100-sample class-row cohort, and the
    unpadded pool of a 10,000-sample explicit-id cohort -- 2,500 short scattered regions (hundreds of runs, carrier runs at every
    offset modulo 8) and long overlapping ones, sorted and shuffled, with and without a subset."""
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
    names = _names(vs, subset)
    if shape == "explicit":   # offsets of the carrier runs modulo 8 that the short batch reaches
        res = vs.get_var_in_ref(short).raw(with_carriers=False)
        assert res["rows"].shape[0] > 200
    for regions in (short, long_):
        want = oracle_texts(orc, regions)
        perm = rng.permutation(len(regions))
        shuffled = [regions[i] for i in perm]
        want_sh = [want[i] for i in perm]
        for rr, ww in ((regions, want), (shuffled, want_sh)):
            _check_texts(vs, rr, ww)
            _check_texts(vs, rr, ww, subset, names)
    if shape == "narrow_dense":   # the subset's row path is taken: rows with more carriers than a decoded list holds
        res = vs.allele_counts(long_).allele_counts()
        assert int(res["counts"]["carriers"].max()) > info.list_max
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


def test_rows_equal_type6_and_counts_from_genotype_bits(mid_store):
    vs, regions = mid_store
    t6 = vs.get_var_in_ref(regions)
    raw6 = t6.raw(with_carriers=True)
    cres = vs.allele_counts(regions)
    c = cres.allele_counts()
    rows6, rowsc = raw6["rows"], c["rows"]
    assert rows6.shape == rowsc.shape and rows6.shape[0] > 200_000
    for f in rows6.dtype.names:
        if f != "car_begin":
            assert np.array_equal(rows6[f], rowsc[f]), f
    assert np.array_equal(raw6["region_flags"], c["flags"])
    assert np.array_equal(raw6["row_begin"], c["row_begin"]) and np.array_equal(raw6["row_count"], c["row_count"])
    cnt = (rows6["count_flags"] & 0x7FFFFFFF).astype(np.int64)
    assert np.array_equal(c["counts"]["carriers"].astype(np.int64), cnt)
    # alt / hom / phased from the type-6 arena's genotype bits (16-bit words: gt << 13)
    arena = raw6["arena"]
    assert raw6["carrier_bytes"] == 2
    starts = np.repeat(rows6["car_begin"].astype(np.int64), cnt)
    within = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    gt = (arena[starts + within].astype(np.uint32) >> 13) & 7
    row_of = np.repeat(np.arange(cnt.shape[0]), cnt)
    g1, g2, ph = (gt >> 1) & 1, (gt >> 2) & 1, gt & 1
    alt = np.bincount(row_of, weights=g1 + g2, minlength=cnt.shape[0]).astype(np.int64)
    hom = np.bincount(row_of, weights=g1 & g2, minlength=cnt.shape[0]).astype(np.int64)
    phs = np.bincount(row_of, weights=ph, minlength=cnt.shape[0]).astype(np.int64)
    assert np.array_equal(c["counts"]["alt_alleles"].astype(np.int64), alt)
    assert np.array_equal(c["counts"]["hom_alt"].astype(np.int64), hom)
    assert np.array_equal(c["counts"]["phased"].astype(np.int64), phs)
    # totals, layout and fill_ms of a count result
    n_regions, n_var, n_car, _ = cres.totals()
    assert (n_regions, n_var, n_car) == t6.totals()[:3]
    lay = cres.layout()
    assert lay[2] == 0 and lay[3] == 0 and lay[1] == rows6.shape[0]
    assert cres.fill_ms() > 0
    cres.close(); t6.close()


def test_subset_identities(mid_store):
    vs, regions = mid_store
    ns = vs.info().num_samples - 1
    whole = vs.allele_counts(regions).allele_counts()["counts"]
    everyone = vs.allele_counts(regions, list(range(1, ns + 1))).allele_counts()["counts"]
    assert np.array_equal(whole, everyone)
    rng = np.random.default_rng(8)
    part = rng.integers(0, 4, size=ns)
    acc = {f: np.zeros(whole.shape[0], np.int64) for f in whole.dtype.names}
    for k in range(4):
        ids = [int(i) + 1 for i in np.nonzero(part == k)[0]]
        r = vs.allele_counts(regions, ids)
        cc = r.allele_counts()["counts"]
        for f in whole.dtype.names:
            acc[f] += cc[f]
        r.close()
    for f in whole.dtype.names:
        assert np.array_equal(acc[f], whole[f].astype(np.int64)), f


def test_interleaving_leaves_type6_alone():
    kw = dict(ref_length=8_000_000, num_variants=150_000, num_samples=300, seed=5, first_pos=1_000, frac_ins=0.05, frac_del=0.05,
              frac_multi=0.02, max_indel=6, af_exponent=2.0)
    rng = np.random.default_rng(12)
    batches = []
    for k in range(10):
        n = 3_000 + 200 * k + (4_000 if k == 6 else 0)   # like batches (speculated), one larger (refused / re-sized)
        s = np.sort(rng.integers(1_000, 7_990_000, size=n))
        batches.append(np.stack([s, s + rng.integers(50, 3_000, size=n)], axis=1).astype(np.uint64))
    shuffled = batches[3][rng.permutation(batches[3].shape[0])]

    def run(with_counts):
        vs = VariantStore.synthetic(device=0, **kw)
        digests = []
        for k, b in enumerate(batches):
            r = vs.get_var_in_ref(b)
            if with_counts:   # count batches in between: sorted, unsorted, with a subset
                c1 = vs.allele_counts(b)
                c2 = vs.allele_counts(shuffled, [1, 5, 7, 200])
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


def test_device_regions_and_small_batches(mid_store):
    torch = pytest.importorskip("torch")
    vs, regions = mid_store
    sub = [3, 17, 400, 2_000]
    host = vs.allele_counts(regions[:5_000], sub).allele_counts()
    t = torch.from_numpy(regions[:5_000].astype(np.int64)).cuda()
    torch.cuda.synchronize()
    dev = vs.allele_counts(DeviceArray(t.data_ptr(), 5_000), sub).allele_counts()
    for k in ("rows", "counts", "row_begin", "row_count", "flags"):
        assert np.array_equal(host[k], dev[k]), k
    big = vs.allele_counts(regions[:5_000], sub)
    for n in (1, 7, 64):
        small = vs.allele_counts(regions[:n], sub)
        for q in range(n):
            assert small.region_text(q) == big.region_text(q), (n, q)
        small.close()
    big.close()


def test_unsupported_accessors(mid_store):
    vs, regions = mid_store
    r = vs.allele_counts(regions[:1_000])
    for call in (lambda: r.raw(with_carriers=True), lambda: r.view(with_carriers=True), r.digest, r.num_header_records,
                 r.num_region_records):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_UNSUPPORTED
    r.view(with_carriers=False)
    r.close()
    t6 = vs.get_var_in_ref(regions[:1_000])
    with pytest.raises(VariantStoreError):
        t6.allele_counts()   # not a count result
    t6.close()


def test_cli_counts(golden_dir, tmp_path):
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
    for samples, extra in ((None, []), (names, ["-S", sfile])):
        out = os.path.join(tmp_path, "counts.txt")
        subprocess.run([exe, "counts", "-p", prefix, "-r", "@" + rfile, "-o", out] + extra, check=True, capture_output=True)
        with open(out) as f:
            parts = f.read().split("#region ")[1:]
        res = vs.allele_counts(regions, samples)
        assert len(parts) == len(regions)
        for q, part in enumerate(parts):
            head, text = part.split("\n", 1)
            assert head == f"{q} {regions[q][0]}:{regions[q][1]}"
            assert text == res.region_text(q), q
        res.close()
    with open(sfile, "w") as f:
        f.write(names[0] + "\nnobody-of-that-name\n")
    p = subprocess.run([exe, "counts", "-p", prefix, "-r", "@" + rfile, "-S", sfile], capture_output=True, text=True)
    assert p.returncode != 0 and "Sample not found: nobody-of-that-name" in (p.stdout + p.stderr)
    vs.close()
