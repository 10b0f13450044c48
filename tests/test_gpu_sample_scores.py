"""Per-sample scores on the GPU (vs_query_sample_scores).  `sums`, `shift` and `scores` equal the reference worked out from the
oracle's type-6 text EXACTLY -- integer weights and real ones, K = 1, 3 and 8, the whole cohort, a subset and ids given shuffled;
golden sweeps, the duplicate rule (a dropped row shifts the report index), the three storage forms, class rows of 63 and 64 words.
Real weights also within the contract's bound of math.fsum.  Tile and chunk boundaries, overlapping regions with a weight per
report, cross-checks against the burden and genotype-matrix queries, determinism, and the plumbing: device regions and weights, the
device accessor, interleaving, refused accessors, refusals on the device, the mapping form, the CLI."""
import os
import subprocess

import numpy as np
import pytest

import sample_scores_ref as ref
from helpers import random_regions, write_random_cohort
from test_gpu_genotype_matrix import _columns, _oracle, _parse, _read_device, _ref_len, _reported
from test_gpu_row_width_edges import SPREAD_KW, SPREAD_SEED
from variantstore_amd import DeviceArray, VariantStore
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_ARG, VS_ERR_UNSUPPORTED = -5, -7
EPS = 2.0 ** -53


def _int_weights(rng, n, k):
    """Integer-valued float32 (n, k) in -8 .. 8."""
    return rng.integers(-8, 9, size=(n, k)).astype(np.float32)


def _real_weights(rng, n):
    """float32 (n, 5): standard normal, one column x 1e6 beside one x 1e-3, one all-zero column, one holding 1.0 beside 2^-30."""
    w = rng.standard_normal(size=(n, 5)).astype(np.float32)
    w[:, 1] *= np.float32(1e6)
    w[:, 2] *= np.float32(1e-3)
    w[:, 3] = 0
    w[:, 4] = np.where(rng.integers(0, 2, size=n) == 1, np.float32(1.0), np.float32(2.0 ** -30))
    return w


def _subset(rng, ns):
    """A subset that straddles the mask-word boundaries at ids 64 and 128 and contains the last sample (small cohorts: what fits)."""
    ids = set(int(i) for i in rng.choice(np.arange(1, ns + 1), size=max(1, ns // 3), replace=False))
    ids.update(i for i in range(40, 151) if i <= ns)
    ids.add(ns)
    return sorted(ids)


def _query(vs, regions, w, samples, rng, names=None):
    """The query; a subset's ids are given shuffled (the columns are the distinct ids ascending whatever the order)."""
    if samples is not None:
        samples = [samples[i] for i in rng.permutation(len(samples))]
    return vs.sample_scores(regions, w, samples, names)


def _check(vs, regions, parsed, samples, w, rng, real=False):
    """Equality with the reference, the pair count, and for real weights the bound against math.fsum."""
    ids, names = _columns(vs, samples)
    res = _query(vs, regions, w, samples, rng)
    got = res.sample_scores()
    k = w.shape[1]
    assert got["col_ids"].dtype == np.uint32 and got["col_ids"].tolist() == ids and got["names"] == names
    assert got["sums"].dtype == np.int64 and got["scores"].dtype == np.float64 and got["shift"].dtype == np.int32
    assert got["sums"].shape == got["scores"].shape == (len(ids), k) and got["score_names"] == [str(i) for i in range(k)]
    # the reports are the rows of the texts, region after region (a region the reference does not terminate on reports nothing)
    _mine, n_mine = _reported(got, range(len(regions)))
    assert np.array_equal(n_mine, parsed.row_count)
    want, f = ref.sums(parsed, names, w)
    assert np.array_equal(got["shift"], f), (got["shift"], f)
    assert np.array_equal(got["sums"], want), (samples is None, w.shape)
    assert got["scores"].tobytes() == ref.scores(want, f).tobytes()
    assert res.totals()[2] == ref.pairs(parsed, names, w)
    if real:
        exact, carried = ref.fsum(parsed, names, w)
        e = 36 - f.astype(np.int64)
        bound = carried[:, None] * np.ldexp(1.0, e - 36)[None, :] + EPS * np.abs(got["scores"])
        err = np.abs(got["scores"] - exact)
        print("real weights: max |score - fsum| / bound per column:", (err / np.maximum(bound, 1e-300)).max(axis=0))
        assert np.all(err <= bound)
    res.close()
    return got


def _sweep(vs, regions, parsed, rng, real=True):
    """Integer weights at K = 1, 3 and 8 and real ones over the whole cohort and a subset; then the whole cohort by explicit ids."""
    ns = vs.info().num_samples - 1
    n = parsed.n_rows
    sub = _subset(rng, ns)
    for samples in (None, sub):
        for k in (1, 3, 8):
            got = _check(vs, regions, parsed, samples, _int_weights(rng, n, k), rng)
        if real:
            _check(vs, regions, parsed, samples, _real_weights(rng, n), rng, real=True)
    _check(vs, regions, parsed, list(range(1, ns + 1)), _int_weights(rng, n, 3), rng)
    return got


@pytest.mark.parametrize("stem", ["x", "x.small"])
def test_golden_region_sweeps(stem, golden_dir, tmp_path):
    fasta, vcf = os.path.join(golden_dir, stem + ".fa"), os.path.join(golden_dir, stem + ".vcf")
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(11)
    regions = random_regions(rng, _ref_len(fasta), 200)   # unsorted: the device sorts the batch
    parsed, valid = _parse(orc, regions)
    _sweep(vs, regions, parsed, rng)
    srt = sorted(regions)
    _sweep(vs, srt, _parse(orc, srt)[0], rng, real=False)
    # the text: the reported rows the weights are keyed by; names
    res = vs.sample_scores(regions, _int_weights(rng, parsed.n_rows, 2), score_names=["prs", "pc 1"])
    for q in valid:
        a0 = int(parsed.row_begin[q])
        assert res.region_text(int(q)) == "Pos\tRef\tAlt\n" + "".join(h + "\n" for h in parsed.heads[a0:a0 + int(parsed.row_count[q])])
    assert res.sample_scores()["score_names"] == ["prs", "pc 1"]
    res.close()
    vs.close()


def test_mapping_form_on_golden_x(golden_dir):
    """x.vcf by hand: sample id 1 carries 10 C>T as 1|1 and 14 G>A as 1|0.  (1, 20) reports both; (5, 12) reports 10 C>T again."""
    vs = VariantStore.from_vcf(os.path.join(golden_dir, "x.fa"), os.path.join(golden_dir, "x.vcf"), device=0)
    weights = {(10, "C", "T"): [1.5, 1], (14, "G", "A"): [-0.5, 0], (999, "A", "T"): [1, 1]}
    res = vs.sample_scores([(1, 20)], weights, samples=[1], score_names=["prs", "n"])
    got = res.sample_scores()
    assert got["scores"].tolist() == [[1.5 * 2 - 0.5, 2.0]] and res.unmatched == [(999, "A", "T")]
    assert got["names"] == [vs.sample_name(1)] and got["score_names"] == ["prs", "n"]
    res.close()
    res = vs.sample_scores([(1, 20), (5, 12)], weights, samples=[vs.sample_name(1)])
    assert res.sample_scores()["scores"].tolist() == [[1.5 * 2 * 2 - 0.5, 4.0]]
    res.close()
    res = vs.sample_scores([(1, 20)], {(10, "C", "T"): 2})
    got = res.sample_scores()
    assert got["scores"].shape == (vs.info().num_samples - 1, 1) and got["scores"][0, 0] == 4.0 and res.unmatched == []
    res.close()
    vs.close()


@pytest.mark.parametrize("seed", [701, 702, 703])
def test_random_cohorts_with_duplicate_rule(seed, tmp_path):
    fasta, vcf, names = write_random_cohort(str(tmp_path), seed, ref_len=6000, n_rows=400, n_samples=9, p_near=0.6, p_multi=0.3,
                                            p_same=0.3, unphased_p=0.4 if seed % 2 else 0.05, haploid_p=0.1 if seed == 703 else 0.0)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(seed)
    regions = random_regions(rng, 6000, 300, max_len=900)
    parsed, _valid = _parse(orc, regions)
    got = _sweep(vs, regions, parsed, rng)
    dropped = (got["rows"]["count_flags"] >> 31) != 0
    assert dropped.any(), "no row of the batch was dropped by the duplicate rule"
    _rows, slots = ref.reported_rows(got["row_begin"], got["row_count"], dropped)
    n_rep = np.asarray([int((~dropped[int(b):int(b) + int(n)]).sum()) for b, n in zip(got["row_begin"], got["row_count"])], np.int64)
    index = np.concatenate([np.arange(n) for n in n_rep])
    assert (slots != index).any(), "no report's index differs from its slot"
    vs.close()


@pytest.mark.parametrize("shape", ["narrow_dense", "wide", "explicit"])
def test_storage_forms(shape, tmp_path):
    """gt_groups (1,500 samples, dense rows), gt_nibbles of a 4,100-sample class-row cohort (five column tiles at K = 8), and the
    unpadded pool of a 10,000-sample explicit-id cohort: short scattered regions and long overlapping ones, the long ones shuffled."""
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
        got = _sweep(vs, regions, _parse(orc, regions)[0], rng)
        dense_seen = max(dense_seen, int((got["rows"]["count_flags"] & 0x7FFFFFFF).max()))
    perm = rng.permutation(len(long_))
    shuffled = [long_[i] for i in perm]
    _sweep(vs, shuffled, _parse(orc, shuffled)[0], rng, real=False)
    if shape == "narrow_dense":   # the dense path ran: rows with more carriers than a decoded list holds
        assert dense_seen > info.list_max
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
    parsed, _valid = _parse(orc, regions)
    got = _sweep(vs, regions, parsed, rng)
    cnt = got["rows"]["count_flags"] & 0x7FFFFFFF
    assert (cnt > 64).sum() > 10 and ((cnt > 0) & (cnt <= 64)).sum() > 10, "both passes"
    # both passes ran with a weight: all-ones weights make every carrier of every reported row count
    res = vs.sample_scores(regions, np.ones(parsed.n_rows, np.float32))
    dropped = (got["rows"]["count_flags"] >> 31) != 0
    rows, _slots = ref.reported_rows(got["row_begin"], got["row_count"], dropped)
    assert (cnt[rows] > 64).any() and (cnt[rows] <= 64).any() and res.totals()[2] == int(cnt[rows].sum())
    res.close()
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


def _n_reports(vs, regions):
    """(N, the count result's arrays) of a batch: the rows its regions report."""
    c = vs.allele_counts(regions)
    got = c.allele_counts()
    c.close()
    dropped = (got["rows"]["count_flags"] >> 31) != 0
    rows, _slots = ref.reported_rows(got["row_begin"], got["row_count"], dropped)
    return rows.shape[0], got


class _MatrixRoute:
    """The route the query replaces: the genotype matrix of the batch (taken once per sample set), the reports' quantised weights
    scattered to the rows of THAT batch's table (the report order is the same in every batch, the private rows need not lie alike),
    then dosage^T @ W in int64."""

    def __init__(self, vs, regions, samples):
        m = vs.genotype_matrix(regions, samples)
        got = m.genotype_matrix()
        m.close()
        dropped = (got["rows"]["count_flags"] >> 31) != 0
        self.rows, _slots = ref.reported_rows(got["row_begin"], got["row_count"], dropped)
        self.n_table = got["rows"].shape[0]
        self.dt = np.ascontiguousarray((((got["cells"] >> 1) & 1) + ((got["cells"] >> 2) & 1)).T).astype(np.float64)

    def sums(self, w):
        """(int64 sums, shifts).  The product runs in float64 on the weights' low 20 bits and on the rest apart: every partial sum stays below 2^53."""
        f = ref.shifts(w)
        q = ref.quantise(w, f)
        table = np.zeros((self.n_table, q.shape[1]), np.int64)
        np.add.at(table, self.rows, q)
        lo, hi = table & ((1 << 20) - 1), table >> 20
        assert np.abs(hi).max(initial=0) * 2 * self.n_table < 2 ** 53
        return (np.rint(self.dt @ hi.astype(np.float64)).astype(np.int64) << 20) + np.rint(self.dt @ lo.astype(np.float64)).astype(np.int64), f


def _matrix_route(vs, regions, samples, w):
    return _MatrixRoute(vs, regions, samples).sums(w)


def test_matrix_route_tiles_and_chunks(t6_store):
    """The 300-sample cohort: sums == dosage(genotype_matrix)^T @ W in int64, under the defaults and with tiles of 64 columns and chunks
    of 64 rows (five tiles, the last of 44 columns; a subset whose columns end inside a tile), the same integers every time."""
    vs, regions = t6_store
    regions = regions[:1_500]
    rng = np.random.default_rng(8)
    n, _c = _n_reports(vs, regions)
    sub = _subset(rng, 300)
    for samples in (None, sub):
        route = _MatrixRoute(vs, regions, samples)
        for w in (_int_weights(rng, n, 1), _int_weights(rng, n, 3), _real_weights(rng, n), _int_weights(rng, n, 8)):
            want, f = route.sums(w)
            outs = []
            for tile, chunk in ((0, 0), (64, 64), (16, 0), (0, 64)):
                vs.set_option("score_tile_cols", tile)
                vs.set_option("score_chunk", chunk)
                try:
                    res = _query(vs, regions, w, samples, rng)
                    got = res.sample_scores()
                    assert res.fill_ms() > 0
                    res.close()
                finally:
                    vs.set_option("score_tile_cols", 0)
                    vs.set_option("score_chunk", 0)
                assert np.array_equal(got["shift"], f) and np.array_equal(got["sums"], want), (samples is None, w.shape, tile, chunk)
                outs.append(got["sums"].tobytes() + got["scores"].tobytes())
            assert len(set(outs)) == 1 and want.any()


def test_table_ends_inside_a_chunk(t6_store):
    vs, regions = t6_store
    rng = np.random.default_rng(5)
    for n in range(900, 1_000):   # a batch whose table ends inside a chunk of 64 rows and inside a wave's rows
        c = vs.allele_counts(regions[:n])
        a = c.layout()[1]
        c.close()
        if a % 64:
            break
    assert a % 64 != 0 and a > 4 * 64
    nrep, _c = _n_reports(vs, regions[:n])
    w = _int_weights(rng, nrep, 3)
    want, _f = _matrix_route(vs, regions[:n], None, w)
    for chunk in (0, 64, 4096):
        vs.set_option("score_chunk", chunk)
        try:
            res = vs.sample_scores(regions[:n], w)
            assert np.array_equal(res.sample_scores()["sums"], want) and res.layout()[1] == a
            res.close()
        finally:
            vs.set_option("score_chunk", 0)


def test_overlapping_regions_weigh_every_report(t6_store):
    """Long overlapping regions: a table row is reported by up to ten regions, every report with a weight of its own."""
    vs, _regions = t6_store
    rng = np.random.default_rng(41)
    x = np.arange(2_000_000, 2_400_000, 5_000)
    regions = np.stack([x, x + 50_000], axis=1).astype(np.uint64)
    regions = regions[rng.permutation(regions.shape[0])]
    n, c = _n_reports(vs, regions)
    assert n > 3 * c["rows"].shape[0], "the regions do not overlap"
    for samples in (None, _subset(rng, 300)):
        route = _MatrixRoute(vs, regions, samples)
        for w in (_int_weights(rng, n, 3), _real_weights(rng, n)):
            want, f = route.sums(w)
            res = vs.sample_scores(regions, w, samples)
            got = res.sample_scores()
            res.close()
            assert np.array_equal(got["sums"], want) and np.array_equal(got["shift"], f) and want.any()
            assert got["scores"].tobytes() == ref.scores(want, f).tobytes()


def test_all_ones_is_the_burden(t6_store):
    """All weights 1 at K = 1: scores[c] == the sum over the regions of sample_burden[q, c].alt_alleles; the pair count is the sum of
    its `variants`."""
    vs, regions = t6_store
    rng = np.random.default_rng(29)
    n, _c = _n_reports(vs, regions)
    for samples in (None, _subset(rng, 300)):
        res = vs.sample_scores(regions, np.ones(n, np.float32), samples)
        got = res.sample_scores()
        b = vs.sample_burden(regions, samples)
        cells = b.sample_burden()["cells"]
        assert got["shift"].tolist() == [35]
        assert np.array_equal(got["scores"][:, 0], cells["alt_alleles"].astype(np.int64).sum(axis=0).astype(np.float64)) and got["scores"].any()
        assert res.totals()[2] == int(cells["variants"].astype(np.int64).sum()) == b.totals()[2]
        assert res.totals()[:2] == b.totals()[:2]
        lay = res.layout()
        assert lay[2] == 0 and lay[3] == 0 and lay[1] == got["rows"].shape[0]
        res.close(); b.close()


def test_sparse_weights_and_an_empty_table(t6_store):
    """Weights on 1 % of the reports (the other rows are skipped), no weight at all, and a batch without rows."""
    vs, regions = t6_store
    rng = np.random.default_rng(3)
    n, _c = _n_reports(vs, regions)
    w = _real_weights(rng, n)
    w[rng.random(n) >= 0.01] = 0
    want, f = _matrix_route(vs, regions, None, w)
    res = vs.sample_scores(regions, w)
    got = res.sample_scores()
    assert np.array_equal(got["sums"], want) and np.array_equal(got["shift"], f) and want.any()
    res.close()
    res = vs.sample_scores(regions, np.zeros((n, 2), np.float32))
    got = res.sample_scores()
    assert got["shift"].tolist() == [0, 0] and not got["sums"].any() and not got["scores"].any() and res.totals()[2] == 0
    res.close()
    empty = [(2, 900), (9_000_000, 9_000_010)]   # in front of the first variant; beyond the reference
    n0, c0 = _n_reports(vs, empty)
    assert n0 == 0 and c0["rows"].shape[0] == 0
    for w0 in (np.zeros((0, 3), np.float32), np.zeros(0, np.float32)):
        res = vs.sample_scores(empty, w0, [5, 200])
        got = res.sample_scores()
        assert got["scores"].shape == (2, w0.shape[1] if w0.ndim == 2 else 1) and not got["scores"].any() and not got["sums"].any()
        assert got["col_ids"].tolist() == [5, 200] and res.totals()[2] == 0
        res.close()


def test_same_bytes_every_time(t6_store):
    """The same call twice on the shared handle, and on a fresh handle whose pool hands the buffers back dirty."""
    vs, regions = t6_store
    rng = np.random.default_rng(23)
    batch = regions[:1_500]
    n, _c = _n_reports(vs, batch)
    w = np.concatenate([_real_weights(rng, n), _int_weights(rng, n, 3)], axis=1)
    sub = _subset(rng, 300)
    outs = {}
    for samples in (None, sub):
        res = [vs.sample_scores(batch, w, samples) for _ in range(2)]
        got = [r.sample_scores() for r in res]
        for r in res:
            r.close()
        assert got[0]["sums"].tobytes() == got[1]["sums"].tobytes() and got[0]["scores"].tobytes() == got[1]["scores"].tobytes()
        assert got[0]["sums"].any()
        outs[samples is None] = got[0]
    fresh = VariantStore.synthetic(device=0, **T6_KW)
    m = fresh.genotype_matrix(batch)   # a genotype matrix larger than every buffer of the score batch was there before
    _ptr, a, _cols, pitch = m.genotype_matrix_device()
    assert a * pitch >= a * 8 * 8 + 4 * a and m.totals()[2] > 0
    m.close()
    for samples in (None, sub):
        res = fresh.sample_scores(batch, w, samples)
        got = res.sample_scores()
        res.close()
        assert got["sums"].tobytes() == outs[samples is None]["sums"].tobytes()
        assert got["scores"].tobytes() == outs[samples is None]["scores"].tobytes()
    fresh.close()


def test_interleaving_leaves_type6_alone():
    rng = np.random.default_rng(12)
    batches = []
    for k in range(10):
        n = 3_000 + 200 * k + (4_000 if k == 6 else 0)   # like batches (speculated), one larger (refused / re-sized)
        s = np.sort(rng.integers(1_000, 7_990_000, size=n))
        batches.append(np.stack([s, s + rng.integers(50, 3_000, size=n)], axis=1).astype(np.uint64))
    shuffled = batches[3][rng.permutation(batches[3].shape[0])]

    def run(with_scores):
        vs = VariantStore.synthetic(device=0, **T6_KW)
        digests = []
        n_shuffled = _n_reports(vs, shuffled)[0] if with_scores else 0
        for k, b in enumerate(batches):
            n_b = _n_reports(vs, b)[0] if with_scores else 0
            r = vs.get_var_in_ref(b)
            if with_scores:   # score batches in between: sorted, unsorted
                c1 = vs.sample_scores(b, np.ones(n_b, np.float32))
                c2 = vs.sample_scores(shuffled, np.ones((n_shuffled, 2), np.float32), [1, 5, 200])
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


def test_device_regions_weights_and_pointer(t6_store):
    torch = pytest.importorskip("torch")
    vs, regions = t6_store
    n, _c = _n_reports(vs, regions)
    w = _real_weights(np.random.default_rng(2), n)
    names = ["a", "b", "c", "d", "e"]
    hres = vs.sample_scores(regions, w, score_names=names)
    host = hres.sample_scores()
    t = torch.from_numpy(regions.astype(np.int64)).cuda()
    tw = torch.from_numpy(w).cuda()
    torch.cuda.synchronize()
    dres = vs.sample_scores(DeviceArray(t.data_ptr(), regions.shape[0]), DeviceArray(tw.data_ptr(), w.size), score_names=names)
    dev = dres.sample_scores()
    for k in ("rows", "sums", "scores", "shift", "col_ids", "row_begin", "row_count", "flags"):
        assert np.array_equal(host[k], dev[k]), k
    assert dres.totals() == hres.totals()
    dres.close()
    ps, pu, c, k = hres.sample_scores_device()
    assert (c, k) == host["scores"].shape and ps and pu
    later = vs.sample_scores(regions[:500], np.ones(_n_reports(vs, regions[:500])[0], np.float32))   # a later batch leaves the cells alone
    later.totals()
    cells = _read_device(torch, ps, c, k * 8).view(np.float64).reshape(c, k)
    assert cells.tobytes() == host["scores"].tobytes() and cells.any()
    ints = _read_device(torch, pu, c, k * 8).view(np.int64).reshape(c, k)
    assert np.array_equal(ints, host["sums"])
    later.close(); hres.close()
    # a NaN in device weights: the scale kernel finds it, the message names the column
    bad = w.copy()
    bad[n // 2, 3] = np.nan
    tb = torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()
    with pytest.raises(VariantStoreError) as e:
        vs.sample_scores(regions, DeviceArray(tb.data_ptr(), bad.size), score_names=names)
    assert e.value.code == VS_ERR_ARG and "column 3" in str(e.value) and "not finite" in str(e.value)
    ok = vs.sample_scores(regions, DeviceArray(tw.data_ptr(), w.size), score_names=names)   # the handle answers afterwards
    assert np.array_equal(ok.sample_scores()["sums"], host["sums"])
    ok.close()


def test_refusals_on_the_device(t6_store):
    """Wrong n_weights (the message names both numbers) and the size limit; the handle goes on answering."""
    vs, regions = t6_store
    n, c = _n_reports(vs, regions)
    for wrong in (n - 1, n + 1, 0):
        with pytest.raises(VariantStoreError) as e:
            vs.sample_scores(regions, np.ones((wrong, 2), np.float32))
        assert e.value.code == VS_ERR_ARG and str(wrong) in str(e.value) and str(n) in str(e.value), str(e.value)
    a = c["rows"].shape[0]
    w = np.ones((n, 8), np.float32)
    need = n * 8 * 4 + a * (8 * 8 + 4) + 300 * 8 * 16
    assert need > 1 << 20
    vs.set_option("matrix_max_mib", 1)
    try:
        with pytest.raises(VariantStoreError) as e:
            vs.sample_scores(regions, w)
        assert e.value.code == VS_ERR_ARG
        msg = str(e.value)
        assert f"{n} reports" in msg and "8 scores" in msg and str(need) in msg and "matrix_max_mib" in msg, msg
        m0 = _n_reports(vs, regions[:50])[0]
        few = vs.sample_scores(regions[:50], np.ones(m0, np.float32), [3])   # a request below the limit is answered meanwhile
        assert few.sample_scores()["scores"].shape == (1, 1)
        few.close()
    finally:
        vs.set_option("matrix_max_mib", 0)
    again = vs.sample_scores(regions, w)
    assert again.sample_scores()["scores"].shape == (300, 8)
    again.close()


def test_refused_accessors(t6_store):
    vs, regions = t6_store
    n = _n_reports(vs, regions[:1_000])[0]
    r = vs.sample_scores(regions[:1_000], np.ones(n, np.float32))
    for call in (lambda: r.raw(with_carriers=True), lambda: r.view(with_carriers=True), r.digest, r.num_header_records,
                 r.num_region_records):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_UNSUPPORTED
    for call in (r.allele_counts, r.group_counts, r.group_counts_device, r.sample_burden, r.sample_burden_device, r.genotype_matrix,
                 r.genotype_matrix_device, r.ld_band, r.ld_band_device, r.assoc_scan, r.assoc_scan_device):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_ARG
    r.view(with_carriers=False)
    r.close()
    others = (vs.get_var_in_ref(regions[:1_000]), vs.allele_counts(regions[:1_000]), vs.genotype_matrix(regions[:100], [1, 2]),
              vs.group_counts(regions[:100], [[1], [2]]), vs.ld_band(regions[:100], window=4), vs.sample_burden(regions[:100], [1, 2]),
              vs.assoc_scan(regions[:100], np.ones(300, np.float32)))
    for res in others:
        for call in (res.sample_scores, res.sample_scores_device):
            with pytest.raises(VariantStoreError) as e:
                call()
            assert e.value.code == VS_ERR_ARG
        res.close()


def test_cli_score_on_golden_x(golden_dir, tmp_path):
    exe = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    subprocess.run([exe, "construct", "-r", os.path.join(golden_dir, "x.fa"), "-v", os.path.join(golden_dir, "x.vcf"), "-p", prefix], check=True, capture_output=True)
    vs = VariantStore.open(prefix, device=0)
    regions = [(1, 20), (5, 12), (1, _ref_len(os.path.join(golden_dir, "x.fa")))]
    rfile, wfile, sfile = (os.path.join(tmp_path, f) for f in ("regions.txt", "weights.txt", "samples.txt"))
    with open(rfile, "w") as f:
        f.write("".join(f"{x}:{y}\n" for x, y in regions))
    weights = {(10, "C", "T"): [1.5, -3.0], (14, "G", "A"): [-0.5, 0.001], (999, "A", "T"): [1.0, 1.0]}
    for header, names in (("#pos ref alt prs pc1\n", ["prs", "pc1"]), ("", None)):
        with open(wfile, "w") as f:
            f.write(header + "".join(f"{p}\t{r} {a}\t" + " ".join(repr(float(np.float32(v))) for v in vals) + "\n" for (p, r, a), vals in weights.items()) + "\n")
        for who in (None, [vs.sample_name(1)]):
            out = os.path.join(tmp_path, "score_out.txt")
            cmd = [exe, "score", "-p", prefix, "-r", "@" + rfile, "-W", wfile, "-o", out]
            if who:
                with open(sfile, "w") as f:
                    f.write("\n".join(who) + "\n")
                cmd += ["-S", sfile]
            p = subprocess.run(cmd, check=True, capture_output=True, text=True)
            assert "warning: 1 of 3 variants" in p.stderr
            res = vs.sample_scores(regions, weights, who, names)
            got = res.sample_scores()
            assert res.unmatched == [(999, "A", "T")] and got["scores"].any()
            res.close()
            with open(out) as f:
                lines = f.read().split("\n")
            assert lines[0] == "Sample\t" + "\t".join(names or ["0", "1"]) and lines[-1] == "" and len(lines) == len(got["names"]) + 2
            for name, row, line in zip(got["names"], got["scores"], lines[1:]):
                assert line == name + "".join("\t%.17g" % v for v in row)
    vs.close()
