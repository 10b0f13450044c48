"""Score-matrix queries on the GPU (vs_query_score_matrix).  `sums`, `shift` and `scores` equal the reference worked out from the
oracle's type-6 text EXACTLY (golden sweeps with the mapping form, random cohorts under the duplicate rule), and the route the query
replaces -- genotype_matrix dosages^T @ T in int64 -- at every edge the kernel has: column tiles of 127, 128 and 129 columns, 300
columns in three tiles and a subset, score tiles at K = 1, 15, 16, 17 and 33, row chunks of 128 and 4096, a table that ends inside
the first and inside the second 64-row k-step, row totals that need four limbs and five.  Agreement with vs_query_sample_scores on
integer weights, the contract's bound against math.fsum on real ones, zeros, an empty table, interleaving, the device accessor,
refused accessors, refusals on the device (the row total beyond 2^38 among them), and the CLI."""
import os
import subprocess

import numpy as np
import pytest

import score_matrix_ref as ref
from helpers import random_regions, write_random_cohort
from test_gpu_genotype_matrix import _columns, _oracle, _parse, _read_device, _ref_len, _reported
from test_gpu_sample_scores import T6_KW, _MatrixRoute, _int_weights, _n_reports, _real_weights, _subset, t6_store  # noqa: F401 (t6_store: a fixture)
from variantstore_amd import VariantStore
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_ARG, VS_ERR_UNSUPPORTED = -5, -7
EPS = 2.0 ** -53


def _route_sums(route, w):
    """(int64 sums, shifts, T) by the route the query replaces: the reports' fixed-point weights added up per table row of the
    genotype-matrix batch, then dosage^T @ T -- in float64 on T's low 20 bits and on the rest apart, so that every partial sum
    stays below 2^53 and the product is exact."""
    f = ref.shifts(w)
    t = ref.totals(w, route.rows, route.n_table)
    lo, hi = t & ((1 << 20) - 1), t >> 20
    assert np.abs(hi).max(initial=0) * 2 * route.n_table < 2 ** 53
    s = (np.rint(route.dt @ hi.astype(np.float64)).astype(np.int64) << 20) + np.rint(route.dt @ lo.astype(np.float64)).astype(np.int64)
    return s, f, t


def _get(vs, regions, w, samples=None, names=None):
    res = vs.score_matrix(regions, w, samples, names)
    got = res.score_matrix()
    assert res.fill_ms() > 0
    res.close()
    return got


def _same(got, want, f, limbs=None):
    assert got["sums"].dtype == np.int64 and got["scores"].dtype == np.float64 and got["shift"].dtype == np.int32
    assert got["sums"].shape == got["scores"].shape == want.shape
    assert np.array_equal(got["shift"], f), (got["shift"], f)
    assert np.array_equal(got["sums"], want)
    assert got["scores"].tobytes() == ref.scores(want, f).tobytes()
    if limbs is not None:
        assert got["limbs"] == limbs


def _check_text(vs, regions, parsed, samples, w, rng, real=False):
    """Equality with the reference from the oracle's text, and for real weights the bound against math.fsum."""
    ids, names = _columns(vs, samples)
    given = None if samples is None else [samples[i] for i in rng.permutation(len(samples))]   # (a subset's ids shuffled)
    got = _get(vs, regions, w, given)
    assert got["col_ids"].dtype == np.uint32 and got["col_ids"].tolist() == ids and got["names"] == names
    assert got["score_names"] == [str(i) for i in range(w.shape[1])]
    _mine, n_mine = _reported(got, range(len(regions)))
    assert np.array_equal(n_mine, parsed.row_count)
    want, f = ref.sums(parsed, names, w)
    _same(got, want, f)
    if real:
        exact, carried = ref.fsum(parsed, names, w)
        e = 30 - f.astype(np.int64)
        # each term is off by at most d 2^(e - 31) with d <= 2: carried 2^(e - 30); then one conversion rounding
        bound = carried[:, None] * np.ldexp(1.0, e - 30)[None, :] + EPS * np.abs(got["scores"])
        err = np.abs(got["scores"] - exact)
        print("real weights: max |score - fsum| / bound per column:", (err / np.maximum(bound, 1e-300)).max(axis=0))
        assert np.all(err <= bound)
    return got


def _sweep_text(vs, regions, parsed, rng):
    ns = vs.info().num_samples - 1
    n = parsed.n_rows
    for samples in (None, _subset(rng, ns)):
        for k in (1, 17):
            got = _check_text(vs, regions, parsed, samples, _int_weights(rng, n, k), rng)
        _check_text(vs, regions, parsed, samples, _real_weights(rng, n), rng, real=True)
    return got


@pytest.mark.parametrize("stem", ["x", "x.small"])
def test_golden_region_sweeps(stem, golden_dir, tmp_path):
    fasta, vcf = os.path.join(golden_dir, stem + ".fa"), os.path.join(golden_dir, stem + ".vcf")
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(11)
    regions = random_regions(rng, _ref_len(fasta), 200)   # unsorted: the device sorts the batch
    parsed, valid = _parse(orc, regions)
    _sweep_text(vs, regions, parsed, rng)
    res = vs.score_matrix(regions, _int_weights(rng, parsed.n_rows, 2), score_names=["prs", "pc 1"])
    for q in valid:
        a0 = int(parsed.row_begin[q])
        assert res.region_text(int(q)) == "Pos\tRef\tAlt\n" + "".join(h + "\n" for h in parsed.heads[a0:a0 + int(parsed.row_count[q])])
    assert res.score_matrix()["score_names"] == ["prs", "pc 1"]
    res.close()
    vs.close()


def test_mapping_form_on_golden_x(golden_dir):
    """x.vcf by hand: sample id 1 carries 10 C>T as 1|1 and 14 G>A as 1|0.  (1, 20) reports both; (5, 12) reports 10 C>T again."""
    vs = VariantStore.from_vcf(os.path.join(golden_dir, "x.fa"), os.path.join(golden_dir, "x.vcf"), device=0)
    weights = {(10, "C", "T"): [1.5, 1], (14, "G", "A"): [-0.5, 0], (999, "A", "T"): [1, 1]}
    res = vs.score_matrix([(1, 20)], weights, samples=[1], score_names=["prs", "n"])
    got = res.score_matrix()
    assert got["scores"].tolist() == [[1.5 * 2 - 0.5, 2.0]] and res.unmatched == [(999, "A", "T")] and got["limbs"] == 4
    assert got["names"] == [vs.sample_name(1)] and got["score_names"] == ["prs", "n"]
    res.close()
    res = vs.score_matrix([(1, 20), (5, 12)], weights, samples=[vs.sample_name(1)])
    assert res.score_matrix()["scores"].tolist() == [[1.5 * 2 * 2 - 0.5, 4.0]]
    res.close()
    wide = {(10, "C", "T"): np.arange(1, 41), (14, "G", "A"): -np.arange(1, 41)}   # 40 columns: beyond sample_scores' 8
    res = vs.score_matrix([(1, 20)], wide)
    got = res.score_matrix()
    assert got["scores"].shape == (vs.info().num_samples - 1, 40) and got["scores"][0].tolist() == [float(k) for k in range(1, 41)] and res.unmatched == []
    res.close()
    vs.close()


@pytest.mark.parametrize("seed", [701, 703])
def test_random_cohorts_with_duplicate_rule(seed, tmp_path):
    fasta, vcf, names = write_random_cohort(str(tmp_path), seed, ref_len=6000, n_rows=400, n_samples=9, p_near=0.6, p_multi=0.3,
                                            p_same=0.3, unphased_p=0.4 if seed % 2 else 0.05, haploid_p=0.1 if seed == 703 else 0.0)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(seed)
    regions = random_regions(rng, 6000, 300, max_len=900)
    parsed, _valid = _parse(orc, regions)
    got = _sweep_text(vs, regions, parsed, rng)
    dropped = (got["rows"]["count_flags"] >> 31) != 0
    assert dropped.any(), "no row of the batch was dropped by the duplicate rule"
    _rows, slots = ref.reported_rows(got["row_begin"], got["row_count"], dropped)
    n_rep = np.asarray([int((~dropped[int(b):int(b) + int(n)]).sum()) for b, n in zip(got["row_begin"], got["row_count"])], np.int64)
    assert (slots != np.concatenate([np.arange(n) for n in n_rep])).any(), "no report's index differs from its slot: no dropped row in front of a report"
    vs.close()


@pytest.mark.parametrize("num_samples", [127, 128, 129])
def test_column_tile_edges(num_samples):
    """127, 128 and 129 columns (a synthetic cohort's num_samples does not count the reference's column): one tile short of full, one
    full tile, and a second tile that holds one column."""
    vs = VariantStore.synthetic(device=0, ref_length=200_000, num_variants=4_000, num_samples=num_samples, seed=900 + num_samples, first_pos=100,
                                frac_ins=0.05, frac_del=0.05, frac_multi=0.02, max_indel=4, af_exponent=1.5)
    rng = np.random.default_rng(num_samples)
    x = np.arange(100, 195_000, 1_300)
    apart = np.stack([x, x + 1_299], axis=1).astype(np.uint64)   # windows side by side: every row reported once, four limbs
    s = np.sort(rng.integers(100, 195_000, size=150))
    over = np.stack([s, s + rng.integers(50, 3_000, size=s.shape[0])], axis=1).astype(np.uint64)
    seen = set()
    for regions in (apart, over):
        n, _c = _n_reports(vs, regions)
        route = _MatrixRoute(vs, regions, None)
        assert route.dt.shape[0] == num_samples and route.n_table > 256
        for w in (_int_weights(rng, n, 17), _real_weights(rng, n)):
            want, f, t = _route_sums(route, w)
            got = _get(vs, regions, w)
            _same(got, want, f, limbs=ref.limbs_needed(t))
            seen.add(got["limbs"])
            assert want[-1].any() and want[0].any(), "the last column carries nothing: the edge is not exercised"
        assert regions is not apart or seen == {4}
    vs.close()


def test_tiles_score_tiles_and_chunks(t6_store):
    """The 300-sample cohort -- three column tiles, the last of 43 columns; a subset whose columns end inside a tile --, K at the
    score-tile edges (1, 15, 16, 17, 33: the last tile holds one score), row chunks by the batch's shape, of one step and of 32:
    the route's integers and the same bytes under every chunk; n_carriers is the matrix's."""
    vs, regions = t6_store
    regions = regions[:1_500]
    rng = np.random.default_rng(8)
    n, _c = _n_reports(vs, regions)
    sub = _subset(rng, 300)
    assert len(sub) % 128 != 0
    for samples in (None, sub):
        route = _MatrixRoute(vs, regions, samples)
        m = vs.genotype_matrix(regions, samples)
        cells = m.totals()[2]
        m.close()
        for k in (1, 15, 16, 17, 33):
            w = _real_weights(rng, n)[:, :1] if k == 1 else np.concatenate([_int_weights(rng, n, k - 5), _real_weights(rng, n)], axis=1)
            want, f, t = _route_sums(route, w)
            outs = []
            for chunk in (0, 128, 4096):
                vs.set_option("score_matrix_chunk", chunk)
                try:
                    res = vs.score_matrix(regions, w, samples)
                    got = res.score_matrix()
                    assert res.totals()[2] == cells and res.layout()[2] == 0 and res.layout()[3] == 0
                    res.close()
                finally:
                    vs.set_option("score_matrix_chunk", 0)
                _same(got, want, f, limbs=ref.limbs_needed(t))   # (the batch's regions overlap here and there: some K need five)
                outs.append(got["sums"].tobytes() + got["scores"].tobytes())
            assert len(set(outs)) == 1 and want.any() and want[:, -1].any()


def test_table_ends_inside_a_step(t6_store):
    """One batch whose table ends inside the first 64-row k-step of its last 128-row step, one that ends inside the second."""
    vs, regions = t6_store
    rng = np.random.default_rng(5)
    found = {}
    for n in range(900, 1_100):
        c = vs.allele_counts(regions[:n])
        a = c.layout()[1]
        c.close()
        half = 0 if 1 <= a % 128 <= 63 else 1 if 65 <= a % 128 <= 127 else None
        if half is not None and half not in found:
            found[half] = (n, a)
        if len(found) == 2:
            break
    assert len(found) == 2
    for half, (n, a) in found.items():
        nrep, _c = _n_reports(vs, regions[:n])
        w = _int_weights(rng, nrep, 17)
        want, f, t = _route_sums(_MatrixRoute(vs, regions[:n], None), w)
        for chunk in (0, 128, 4096):
            vs.set_option("score_matrix_chunk", chunk)
            try:
                res = vs.score_matrix(regions[:n], w)
                assert res.layout()[1] == a
                _same(res.score_matrix(), want, f, limbs=ref.limbs_needed(t))
                res.close()
            finally:
                vs.set_option("score_matrix_chunk", 0)


def test_overlapping_regions_four_and_five_limbs(t6_store):
    """Long overlapping regions: a table row is reported by up to ten regions, every report with a weight of its own.  With every
    weight of a column at the column's largest the totals of such rows pass 2,139,062,143 and the kernel runs five limbs; the same
    regions laid side by side report every row once and run four."""
    vs, _regions = t6_store
    rng = np.random.default_rng(41)
    x = np.arange(2_000_000, 2_400_000, 5_000)
    over = np.stack([x, x + 50_000], axis=1).astype(np.uint64)
    over = over[rng.permutation(over.shape[0])]
    apart = np.stack([x, x + 4_999], axis=1).astype(np.uint64)
    n, c = _n_reports(vs, over)
    assert n > 3 * c["rows"].shape[0], "the regions do not overlap"
    n1, c1 = _n_reports(vs, apart)
    assert n1 == int((~((c1["rows"]["count_flags"] >> 31) != 0)).sum()), "a row is reported twice"
    for samples in (None, _subset(rng, 300)):
        route = _MatrixRoute(vs, over, samples)
        # random weights, integer and real: whether ten of them pass the four-limb bound is the reference's to say
        for w in (_int_weights(rng, n, 3), _real_weights(rng, n)):
            want, f, t = _route_sums(route, w)
            _same(_get(vs, over, w, samples), want, f, limbs=ref.limbs_needed(t))
        # every weight of column 0 at the column's largest (3.0: q = 3 x 2^28); beside it integer weights in -1 .. 1 under a largest
        # of 64 (q = w 2^23: ten of them stay far below the four-limb bound)
        w = rng.integers(-1, 2, size=(n, 18)).astype(np.float32)
        w[0, :] = 64.0
        w[:, 0] = 3.0
        want, f, t = _route_sums(route, w)
        assert ref.limbs_needed(t) == 5 and int(np.abs(t).max()) > ref.MAX4
        got5 = _get(vs, over, w, samples)
        _same(got5, want, f, limbs=5)
        # the same integer columns without column 0 run four limbs and agree with the five-limb run where the inputs coincide
        want4, f4, t4 = _route_sums(route, w[:, 1:])
        assert ref.limbs_needed(t4) == 4
        got4 = _get(vs, over, np.ascontiguousarray(w[:, 1:]), samples)
        _same(got4, want4, f4, limbs=4)
        assert np.array_equal(got4["sums"], got5["sums"][:, 1:]) and got4["scores"].tobytes() == np.ascontiguousarray(got5["scores"][:, 1:]).tobytes()
        # side by side: the largest weight everywhere, every row reported once: four limbs
        route1 = _MatrixRoute(vs, apart, samples)
        w1 = np.full((n1, 2), 3.0, np.float32)
        want1, f1, t1 = _route_sums(route1, w1)
        assert ref.limbs_needed(t1) == 4
        _same(_get(vs, apart, w1, samples), want1, f1, limbs=4)


def test_agrees_with_sample_scores_on_integer_weights(t6_store):
    """Integer weights are exact at both scales, and f differs by exactly 6 (36 - e against 30 - e)."""
    vs, regions = t6_store
    rng = np.random.default_rng(17)
    batch = regions[:1_500]
    n, _c = _n_reports(vs, batch)
    for samples in (None, _subset(rng, 300)):
        for k in (1, 3, 8):
            w = _int_weights(rng, n, k)
            old = vs.sample_scores(batch, w, samples)
            a = old.sample_scores()
            old.close()
            b = _get(vs, batch, w, samples)
            assert np.array_equal(a["shift"], b["shift"] + 6)
            assert np.array_equal(a["sums"], b["sums"] << 6) and a["sums"].any()
            assert a["scores"].tobytes() == b["scores"].tobytes()
            assert np.array_equal(a["col_ids"], b["col_ids"]) and np.array_equal(a["rows"], b["rows"])


def test_zeros_and_an_empty_table(t6_store):
    vs, regions = t6_store
    rng = np.random.default_rng(3)
    batch = regions[:1_000]
    n, _c = _n_reports(vs, batch)
    got = _get(vs, batch, np.zeros((n, 20), np.float32))
    assert got["shift"].tolist() == [0] * 20 and not got["sums"].any() and not got["scores"].any() and got["limbs"] == 4
    assert not np.signbit(got["scores"]).any()
    w = np.zeros((n, 18), np.float32)
    w[:, 16] = _real_weights(rng, n)[:, 0]   # a column of zeros beside a nonzero one, in the second score tile
    want, f, t = _route_sums(_MatrixRoute(vs, batch, None), w)
    got = _get(vs, batch, w)
    _same(got, want, f, limbs=ref.limbs_needed(t))
    assert got["sums"][:, 16].any() and not got["sums"][:, 17].any() and not got["sums"][:, :16].any() and f[17] == 0
    empty = [(2, 900), (9_000_000, 9_000_010)]   # in front of the first variant; beyond the reference
    n0, c0 = _n_reports(vs, empty)
    assert n0 == 0 and c0["rows"].shape[0] == 0
    for w0 in (np.zeros((0, 33), np.float32), np.zeros(0, np.float32)):
        res = vs.score_matrix(empty, w0, [5, 200])
        got = res.score_matrix()
        assert got["scores"].shape == (2, w0.shape[1] if w0.ndim == 2 else 1) and not got["scores"].any() and not got["sums"].any()
        assert got["col_ids"].tolist() == [5, 200] and res.totals()[2] == 0
        res.close()


def test_interleaving_leaves_type6_alone():
    rng = np.random.default_rng(12)
    batches = []
    for k in range(6):
        n = 3_000 + 200 * k + (4_000 if k == 4 else 0)   # like batches (speculated), one larger (refused / re-sized)
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
            if with_scores:   # score-matrix batches in between: sorted, unsorted
                c1 = vs.score_matrix(b, np.ones((n_b, 17), np.float32))
                c2 = vs.score_matrix(shuffled, np.ones((n_shuffled, 2), np.float32), [1, 5, 200])
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


def test_device_accessor(t6_store):
    torch = pytest.importorskip("torch")
    vs, regions = t6_store
    n, _c = _n_reports(vs, regions)
    w = np.concatenate([_real_weights(np.random.default_rng(2), n), _int_weights(np.random.default_rng(4), n, 15)], axis=1)
    res = vs.score_matrix(regions, w)
    host = res.score_matrix()
    ps, pu, c, k = res.score_matrix_device()
    assert (c, k) == host["scores"].shape == (300, 20) and ps and pu
    later = vs.score_matrix(regions[:500], np.ones(_n_reports(vs, regions[:500])[0], np.float32))   # a later batch leaves the cells alone
    later.totals()
    ints = _read_device(torch, pu, c, k * 8).view(np.int64).reshape(c, k)
    assert np.array_equal(ints, host["sums"]) and ints.any()
    cells = _read_device(torch, ps, c, k * 8).view(np.float64).reshape(c, k)
    assert cells.tobytes() == host["scores"].tobytes()
    later.close(); res.close()


def test_refused_accessors(t6_store):
    vs, regions = t6_store
    n = _n_reports(vs, regions[:1_000])[0]
    r = vs.score_matrix(regions[:1_000], np.ones((n, 9), np.float32))
    for call in (lambda: r.raw(with_carriers=True), lambda: r.view(with_carriers=True), r.digest, r.num_header_records, r.num_region_records):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_UNSUPPORTED
    for call in (r.sample_scores, r.sample_scores_device, r.allele_counts, r.group_counts, r.group_counts_device, r.sample_burden, r.sample_burden_device,
                 r.genotype_matrix, r.genotype_matrix_device, r.ld_band, r.ld_band_device, r.ld_matrix, r.assoc_scan, r.assoc_scan_device, r.assoc_matrix,
                 r.assoc_matrix_device, r.sample_gram, r.sample_gram_device, r.sample_ibs, r.sample_ibs_device):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_ARG
    r.view(with_carriers=False)
    r.close()
    others = (vs.get_var_in_ref(regions[:1_000]), vs.allele_counts(regions[:1_000]), vs.genotype_matrix(regions[:100], [1, 2]),
              vs.sample_scores(regions[:1_000], np.ones(n, np.float32)), vs.sample_gram(regions[:100], [1, 2]),
              vs.assoc_matrix(regions[:100], np.ones((300, 9), np.float32)))
    for res in others:
        for call in (res.score_matrix, res.score_matrix_device):
            with pytest.raises(VariantStoreError) as e:
                call()
            assert e.value.code == VS_ERR_ARG
        res.close()


def test_refusals_on_the_device(t6_store):
    """Wrong n_weights (the message gives both numbers) and the size limit (the message names the parts); the
    handle goes on answering."""
    vs, regions = t6_store
    n, c = _n_reports(vs, regions)
    for wrong in (n - 1, n + 1, 0):
        with pytest.raises(VariantStoreError) as e:
            vs.score_matrix(regions, np.ones((wrong, 20), np.float32))
        assert e.value.code == VS_ERR_ARG and str(wrong) in str(e.value) and str(n) in str(e.value), str(e.value)
    a, K = c["rows"].shape[0], 20
    w = np.ones((n, K), np.float32)
    parts = (a * 304, n * K * 4, a * K * 8, 2 * 16 * 5 * ((a + 127) // 128 * 128), 300 * K * 16)   # matrix (pitch 304), weights, totals, limb panel, sums and scores
    assert sum(parts) > 1 << 20
    vs.set_option("matrix_max_mib", 1)
    try:
        with pytest.raises(VariantStoreError) as e:
            vs.score_matrix(regions, w)
        assert e.value.code == VS_ERR_ARG
        msg = str(e.value)
        assert f"{n} reports" in msg and "20 scores" in msg and str(sum(parts)) in msg and "matrix_max_mib" in msg, msg
        for part, name in zip(parts, ("genotype matrix", "weights", "rows' totals", "limb panel", "sums and scores")):
            assert f"{part} of the {name}" in msg, (name, msg)
        m0 = _n_reports(vs, regions[:20])[0]
        few = vs.score_matrix(regions[:20], np.ones(m0, np.float32), [3])   # a request below the limit is answered meanwhile
        assert few.score_matrix()["scores"].shape == (1, 1)
        few.close()
    finally:
        vs.set_option("matrix_max_mib", 0)
    again = _get(vs, regions, w)
    assert again["scores"].shape == (300, K) and again["scores"].any()


def test_row_total_beyond_2_38_is_refused(golden_dir):
    """300 identical regions report one row 300 times; with every weight just below a power of two (q = 2^30 - 64) its total passes
    2^38 and the call is refused; 256 such reports stay below (256 (2^30 - 64) < 2^38) and run five limbs."""
    vs = VariantStore.from_vcf(os.path.join(golden_dir, "x.fa"), os.path.join(golden_dir, "x.vcf"), device=0)
    big = np.nextafter(np.float32(1.0), np.float32(0.0))
    for reps, refused in ((300, True), (256, False)):
        regions = [(9, 11)] * reps
        n, c = _n_reports(vs, regions)
        assert n == reps * int((~((c["rows"]["count_flags"] >> 31) != 0)).sum()) and n >= reps
        w = np.full((n, 1), big, np.float32)
        if refused:
            with pytest.raises(VariantStoreError) as e:
                vs.score_matrix(regions, w)
            assert e.value.code == VS_ERR_UNSUPPORTED and "2^38" in str(e.value) and "split the batch" in str(e.value)
        else:
            route = _MatrixRoute(vs, regions, None)
            want, f, t = _route_sums(route, w)
            assert int(np.abs(t).max()) == 256 * (2 ** 30 - 64)
            _same(_get(vs, regions, w), want, f, limbs=5)
    vs.close()


def test_cli_scorematrix_on_golden_x(golden_dir, tmp_path):
    exe = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    subprocess.run([exe, "construct", "-r", os.path.join(golden_dir, "x.fa"), "-v", os.path.join(golden_dir, "x.vcf"), "-p", prefix], check=True, capture_output=True)
    vs = VariantStore.open(prefix, device=0)
    regions = [(1, 20), (5, 12), (1, _ref_len(os.path.join(golden_dir, "x.fa")))]
    rfile, wfile, sfile = (os.path.join(tmp_path, f) for f in ("regions.txt", "weights.txt", "samples.txt"))
    with open(rfile, "w") as f:
        f.write("".join(f"{x}:{y}\n" for x, y in regions))
    K = 12
    rng = np.random.default_rng(1)
    weights = {(10, "C", "T"): rng.standard_normal(K).astype(np.float32), (14, "G", "A"): rng.standard_normal(K).astype(np.float32),
               (999, "A", "T"): np.ones(K, np.float32)}
    all_names = [f"s{k}" for k in range(K)]
    for header, names in (("#pos ref alt " + " ".join(all_names) + "\n", all_names), ("", None)):
        with open(wfile, "w") as f:
            f.write(header + "".join(f"{p}\t{r} {a}\t" + " ".join(repr(float(v)) for v in vals) + "\n" for (p, r, a), vals in weights.items()) + "\n")
        for who in (None, [vs.sample_name(1)]):
            out = os.path.join(tmp_path, "score_out.txt")
            cmd = [exe, "scorematrix", "-p", prefix, "-r", "@" + rfile, "-W", wfile, "-o", out]
            if who:
                with open(sfile, "w") as f:
                    f.write("\n".join(who) + "\n")
                cmd += ["-S", sfile]
            p = subprocess.run(cmd, check=True, capture_output=True, text=True)
            assert "warning: 1 of 3 variants" in p.stderr
            res = vs.score_matrix(regions, weights, who, names)
            got = res.score_matrix()
            assert res.unmatched == [(999, "A", "T")] and got["scores"].any()
            res.close()
            with open(out) as f:
                lines = f.read().split("\n")
            assert lines[0] == "Sample\t" + "\t".join(names or [str(k) for k in range(K)]) and lines[-1] == "" and len(lines) == len(got["names"]) + 2
            for name, row, line in zip(got["names"], got["scores"], lines[1:]):
                assert line == name + "".join("\t%.17g" % v for v in row)
    vs.close()
