"""ROH queries on the GPU (vs_query_roh): summary, segments, seg_begin and n_sites bit for bit against roh_ref over the engine's own
genotype matrix of the same regions and samples -- column-tile edges (1, 63, 64, 65, 255, 256, 257 and 513 columns, explicit
subsets and the whole cohort), row-block edges (regions of 0, 1, 63, 64, 65, 128 and 129 rows, a region whose only sites sit in its
last block, a whole block of non-sites in the middle, hundreds of short regions, overlapping regions), the parameters, tables with
dropped rows, saturated rows, segments=False, determinism, interleaving with type-6 batches, the device pointers, both size
refusals, the refused accessors, the CLI, and a cohort written as VCF text with planted stretches whose truth is the text alone."""
import os
import subprocess

import numpy as np
import pytest

from helpers import oracle_texts, random_regions, write_random_cohort, write_saturated_cohort
from roh_cohort import (COHORT_KW, PARAM_SETS, REGION_ROWS, conditions_met, dosages_of_vcf, regions_of_rows, write_planted_cohort, write_roh_cohort)
from roh_ref import (SEGMENT_DTYPE, SUMMARY_DTYPE, check_invariants, cli_segments_text, cli_summary_text, derived, dosage, new_stats, params, region_text,
                     roh_region, runs_column, site_mask)
from test_gpu_genotype_matrix import _oracle, _read_device as _read_device_bytes
from variantstore_amd import VariantStore
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_ARG, VS_ERR_UNSUPPORTED = -5, -7
KEY = ("pos", "ref_off", "ref_len", "alt_off", "alt_len", "count_flags")


def _expected(m, got, p, stats=None, check_columns=24):
    """The expected answer from the matrix result `m` for the table order of the ROH result `got`.  The two calls may place the
    private rows of regions under the duplicate rule elsewhere in the table, so every region is taken through its own row_begin and
    its rows are held to be the same rows in the same order.  Also runs the second formulation (max_het == 0) or the invariant
    checker (max_het > 0) on the first `check_columns` columns of every region."""
    cells_all = np.ascontiguousarray(m["cells"])
    Q, S = got["summary"].shape
    assert np.array_equal(got["row_count"], m["row_count"]) and cells_all.shape[1] == S
    summary = np.zeros((Q, S), SUMMARY_DTYPE)
    n_sites = np.zeros(Q, np.uint32)
    segs = []
    for q in range(Q):
        k, a0, b0 = int(m["row_count"][q]), int(m["row_begin"][q]), int(got["row_begin"][q])
        rm, rg = m["rows"][a0:a0 + k], got["rows"][b0:b0 + k]
        for f in KEY:
            assert np.array_equal(rm[f], rg[f]), ("the region's rows differ between the two calls", q, f)
        cells = cells_all[a0:a0 + k]
        dropped = (rm["count_flags"] >> 31) != 0
        assert not cells[dropped].any()
        assert np.array_equal(got["counts"]["alt_alleles"][b0:b0 + k].astype(np.int64), dosage(cells).sum(axis=1))
        site = site_mask(cells, dropped, p["min_ac"], p["max_ac"])
        pos = rm["pos"].astype(np.int64)
        summary[q], sq, n_sites[q] = roh_region(cells, pos, site, p, q, stats)
        segs += sq
        idx = np.nonzero(site)[0]
        sub = cells[:, :check_columns]
        if p["max_het"] == 0:
            s2, g2, _n = roh_region(sub, pos, site, p, q, walker=runs_column)
            assert g2 == [g for g in sq if g[1] < check_columns] and s2.tobytes() == summary[q, :check_columns].tobytes()
        else:
            d = dosage(sub[idx])
            for c in range(sub.shape[1]):
                check_invariants(summary[q, c], [g[2:] for g in sq if g[1] == c], d[:, c] == 1, pos[idx], idx, p)
    segments = np.zeros(len(segs), SEGMENT_DTYPE)
    for i, g in enumerate(segs):
        segments[i] = g
    seg_begin = np.zeros(Q * S + 1, np.uint64)
    seg_begin[1:] = np.cumsum(summary["n_segments"].reshape(-1).astype(np.uint64))
    return {"summary": summary, "segments": segments, "seg_begin": seg_begin, "n_sites": n_sites}


def _check_full(vs, regions, samples, kw, what=None, stats=None, texts=0, m=None):
    """summary, segments, seg_begin and n_sites of vs.roh(regions, samples, **kw) against roh_ref over genotype_matrix() of the same
    regions and samples.  Returns (matrix arrays, expected, result arrays)."""
    if m is None:
        mres = vs.genotype_matrix(regions, samples)
        m = mres.genotype_matrix()
        mres.close()
    p = params(**kw)
    res = vs.roh(regions, samples, **kw)
    got = res.roh()
    want = _expected(m, got, p, stats)
    assert np.array_equal(got["columns"], m["columns"]) and got["columns"].dtype == np.uint32
    assert got["summary"].dtype == SUMMARY_DTYPE and got["segments"].dtype == SEGMENT_DTYPE and got["seg_begin"].dtype == np.uint64
    assert got["n_sites"].dtype == np.uint32 and np.array_equal(got["n_sites"], want["n_sites"]), (what, got["n_sites"].tolist(), want["n_sites"].tolist())
    for f in SUMMARY_DTYPE.names:
        bad = np.argwhere(got["summary"][f] != want["summary"][f])
        assert bad.shape[0] == 0, (what, f, bad[:6].tolist(), [int(got["summary"][f][tuple(b)]) for b in bad[:6]], [int(want["summary"][f][tuple(b)]) for b in bad[:6]])
    assert got["summary"].tobytes() == want["summary"].tobytes()
    assert np.array_equal(got["seg_begin"], want["seg_begin"]), what
    assert got["segments"].shape == want["segments"].shape and got["segments"].tobytes() == want["segments"].tobytes(), what
    assert {k: got["params"][k] for k in p} == p and got["params"]["segments"] == 1
    want_f = derived(got["summary"])
    assert got["kb"].tobytes() == want_f["kb"].tobytes() and got["kb_avg"].tobytes() == want_f["kb_avg"].tobytes()
    assert res.totals()[2] == int(np.count_nonzero(m["cells"]))
    if texts:
        names = [vs.sample_name(int(i)) for i in got["columns"]]
        S = len(names)
        for q in range(0, len(regions), texts):
            mine = want["segments"][int(want["seg_begin"][q * S]):int(want["seg_begin"][(q + 1) * S])]
            assert res.region_text(q) == region_text(mine, names), (what, q)
            sub = res.region_roh(q, got)
            assert sub["segments"].tobytes() == mine.tobytes() and sub["summary"].tobytes() == want["summary"][q].tobytes() and sub["n_sites"] == int(want["n_sites"][q])
    res.close()
    return m, want, got


# ----------------------------------------------------------------------------------------------------- the ROH cohort
@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("roh_cohort"))
    fasta, vcf, names, positions, dos = write_roh_cohort(d, **COHORT_KW)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    yield vs, names, positions, dos
    vs.close()


def test_parameter_sets_over_the_whole_cohort(cohort):
    """samples=None: 520 columns, three column tiles and a last one of 8 columns; overlapping regions that share rows; every parameter
    set -- max_het 0, 1 and 3, max_gap 0 and 200 (the cohort has two stretches of 400 bases without a record), min_sites 1 and values
    that reject runs, min_bp likewise, an [min_ac, max_ac] window, min_ac = 2 under which 150 consecutive rows are no sites (the
    skip path).  The conditions that keep the comparison from being vacuous are asserted on the expected values."""
    vs, _names, positions, dos = cohort
    regions = regions_of_rows(positions)
    stats, outs, m = new_stats(), [], None
    for kw in PARAM_SETS:
        m, want, got = _check_full(vs, regions, None, kw, kw, stats, texts=2, m=m)
        outs.append((params(**kw), want))
    assert m["row_count"].tolist() == [b - a + 1 for a, b in REGION_ROWS]
    a0 = int(m["row_begin"][0])
    assert np.array_equal(dosage(m["cells"][a0:a0 + 420]), dos), "the engine's matrix is not the writer's"
    conditions_met(stats, outs)
    under_min_ac = outs[1][1]["n_sites"]
    assert int(under_min_ac[3]) == 0 and int(outs[0][1]["n_sites"][3]) == 140   # a region of ineligible rows only


@pytest.mark.parametrize("n_cols", [1, 63, 64, 65, 255, 256, 257, 513])
def test_column_tile_edges(n_cols, cohort):
    """Explicit subsets: one lane, a wave less one, a wave, a wave and one, a tile less one, a tile, a tile and one, two tiles and one."""
    vs, _names, positions, _dos = cohort
    rng = np.random.default_rng(n_cols)
    samples = np.sort(rng.choice(np.arange(1, 521), size=n_cols, replace=False)).astype(np.uint32)
    regions = regions_of_rows(positions, [(0, 419), (290, 419), (100, 200)])
    m = None
    for kw in (PARAM_SETS[0], PARAM_SETS[1 + n_cols % 3]):
        if "max_ac" in kw:   # the cohort's allele-count window, scaled from its 520 columns to this subset
            kw = dict(kw, min_ac=kw["min_ac"] * n_cols // 520, max_ac=kw["max_ac"] * n_cols // 520)
        m, want, got = _check_full(vs, regions, samples, kw, (n_cols, kw), texts=1, m=m)
        assert got["summary"].shape == (3, n_cols) and m["row_pitch"] == (n_cols + 15) // 16 * 16
        if n_cols > 1:
            assert (want["summary"]["n_segments"] > 0).any() and want["segments"].shape[0] > 0
            assert want["summary"][0, 0].tobytes() != want["summary"][0, n_cols - 1].tobytes()
        else:   # one column: a site is a row at which it is het (ac == 1), so there is no run -- and under min_ac = 2 no site at all
            assert not want["summary"]["n_segments"].any()
            if kw.get("min_ac", 0) <= 1:
                assert want["summary"]["n_het"].any() and np.array_equal(want["n_sites"], want["summary"]["n_het"][:, 0])
            else:
                assert not want["n_sites"].any() and not want["summary"]["n_het"].any()


def test_row_block_edges(cohort):
    """Regions reporting 0, 1, 63, 64, 65, 128 and 129 rows; a region whose only sites (under min_ac = 2) sit in its last block; a
    region with a whole block of non-sites in the middle; 300 short regions in one batch."""
    vs, _names, positions, _dos = cohort
    samples = np.arange(5, 5 + 70, dtype=np.uint32)   # two waves
    pos = positions
    by_rows = {k: (int(pos[20]) - 2, int(pos[20 + k - 1]) + 2) for k in (1, 63, 64, 65, 128, 129)}
    empty = (int(pos[69]) + 100, int(pos[69]) + 200)            # inside the first stretch without a record (rows 69 | 70)
    assert int(pos[70]) - int(pos[69]) == 400
    last_block = (int(pos[150]) - 2, int(pos[310]) + 2)         # rows 150 .. 299 are singletons: offsets 0 .. 149, two whole blocks and 22 rows
    hole = (int(pos[60]) - 2, int(pos[349]) + 2)                # offsets 90 .. 239 are singletons: block 2 (128 .. 191) holds no site
    regions = [empty] + list(by_rows.values()) + [last_block, hole]
    for kw in (PARAM_SETS[1], PARAM_SETS[0], PARAM_SETS[2]):
        m, want, got = _check_full(vs, regions, samples, kw, kw, texts=1)
        assert m["row_count"].tolist() == [0, 1, 63, 64, 65, 128, 129, 161, 290]
        assert not got["summary"][0].view(np.uint8).any() and int(got["n_sites"][0]) == 0
        if kw.get("min_ac") == 2:
            a0 = int(m["row_begin"][7])
            site = site_mask(m["cells"][a0:a0 + 161], np.zeros(161, bool), 2)
            assert not site[:150].any() and site[150:].any() and (want["summary"]["n_segments"][7] > 0).any()
            a0 = int(m["row_begin"][8])
            site = site_mask(m["cells"][a0:a0 + 290], np.zeros(290, bool), 2)
            assert site[:64].all() and not site[128:192].any() and site[256:].any() and (want["summary"]["n_segments"][8] > 1).any()
    rng = np.random.default_rng(3)
    starts = rng.integers(0, 400, size=300)
    short = [(int(pos[s]) - 2, int(pos[min(s + int(k), 419)]) + 2) for s, k in zip(starts, rng.integers(0, 20, size=300))]
    m, want, _got = _check_full(vs, short, samples, dict(min_sites=2, max_het=1), "short regions", texts=50)
    assert len(short) == 300 and want["segments"].shape[0] > 1000 and m["row_count"].max() <= 20


# ------------------------------------------------------------------------------------------------ other tables
def test_rows_the_duplicate_rule_dropped(tmp_path):
    """Near and equal records: the duplicate rule drops rows of the table; a dropped row is no site.  The regions under the rule
    report private copies of their rows: every region is compared through its own row_begin."""
    fasta, vcf, _names = write_random_cohort(str(tmp_path), 701, ref_len=6000, n_rows=400, n_samples=9, p_near=0.6, p_multi=0.3, p_same=0.3,
                                             unphased_p=0.4, carrier_p=0.5)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    all_regions = random_regions(np.random.default_rng(701), 6000, 300, max_len=900)
    texts = oracle_texts(_oracle(vs, tmp_path), all_regions)
    regions = [r for r, (n, _e, _t) in zip(all_regions, texts) if n >= 0]
    assert len(regions) > 200   # (only the regions the reference's walk terminates on: the rows of the others are not defined)
    m = None
    for kw in (dict(min_sites=1), dict(min_sites=2, max_het=1, max_gap=40), dict(min_sites=1, max_het=3, min_ac=2, max_ac=12)):
        m, want, got = _check_full(vs, regions, None, kw, ("duplicate rule", kw), texts=40, m=m)
        dropped = (got["rows"]["count_flags"] >> 31) != 0
        assert dropped.any(), "no row of the batch was dropped by the duplicate rule"
        assert want["segments"].shape[0] > 100 and (np.diff(got["rows"]["pos"].astype(np.int64)) == 0).any()   # same-position rows
    vs.close()


def test_saturated_rows(tmp_path):
    """Rows carried by 75 - 100 % of the samples, dense in hets and hom-alt calls; rows carried by every sample 1|1 are no sites."""
    fasta, vcf = write_saturated_cohort(str(tmp_path), 130, 515)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    regions = [(1, 7000), (6000, 14000), (13000, 20001), (500, 900)]
    m = None
    for kw in (dict(min_sites=1), dict(min_sites=3, max_het=3), dict(min_sites=2, max_het=1, min_ac=140, max_ac=170)):   # (the rows' ac lies in 71 .. 189 of 260: the window admits about half of them)
        m, want, got = _check_full(vs, regions, None, kw, ("saturated", kw), texts=1, m=m)
        assert want["segments"].shape[0] > 0 and (want["summary"]["n_het"] > 0).any()
    d = dosage(m["cells"])
    assert (d == 2).sum() > 1000 and (d == 1).sum() > 1000
    vs.close()


def test_planted_stretches_from_the_vcf_text(tmp_path):
    """No engine matrix in the loop: 40 samples, 300 records written as VCF text, seven stretches of 20 or more homozygous calls
    planted in chosen samples and a het at least every seventh record elsewhere.  The truth is read back from the text."""
    fasta, vcf, names, _positions, planted = write_planted_cohort(str(tmp_path))
    pos, names2, d = dosages_of_vcf(vcf)
    assert names2 == names
    truth = []
    for c in range(d.shape[1]):          # from the text: the maximal stretches of 20 or more calls that are not het
        hom = np.concatenate([[False], d[:, c] != 1, [False]])
        edges = np.nonzero(np.diff(hom.astype(np.int64)))[0]
        truth += [(c, int(a), int(b) - 1) for a, b in zip(edges[::2], edges[1::2]) if b - a >= 20]
    assert sorted(truth) == sorted(planted) and len(planted) == 7
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    res = vs.roh([(1, int(pos[-1]) + 50)], min_sites=20)
    got = res.roh(lengths=[int(pos[-1]) + 50])
    assert got["columns"].tolist() == list(range(1, 41)) and [vs.sample_name(i) for i in range(1, 41)] == names
    assert got["rows"]["pos"].tolist() == pos.tolist() and int(got["n_sites"][0]) == 300
    seg = got["segments"]
    assert [(int(g["column"]), int(g["row_first"]), int(g["row_last"])) for g in seg] == sorted(planted)
    for g in seg:
        a, b = int(g["row_first"]), int(g["row_last"])
        assert (int(g["pos_first"]), int(g["pos_last"]), int(g["n_sites"]), int(g["n_het"]), int(g["region"])) == (int(pos[a]), int(pos[b]), b - a + 1, 0, 0)
    per_col = {c: [(a, b) for cc, a, b in planted if cc == c] for c in range(40)}
    for c in range(40):
        s = got["summary"][0, c]
        bps = [int(pos[b] - pos[a]) + 1 for a, b in per_col[c]]
        assert (int(s["n_segments"]), int(s["total_bp"]), int(s["longest_bp"])) == (len(bps), sum(bps), max(bps, default=0))
        assert int(s["n_het"]) == int((d[:, c] == 1).sum())
        assert got["froh"][0, c] == sum(bps) / float(int(pos[-1]) + 50)
    res.close()
    vs.close()


# ---------------------------------------------------------------------------------- a type-6 sized cohort
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


def test_two_calls_give_the_same_bytes_and_segments_false_the_same_summaries(t6_store):
    vs, regions = t6_store
    kw = dict(min_sites=3, max_het=1, max_gap=2_000)
    outs = []
    for _ in range(2):
        r = vs.roh(regions, **kw)
        g = r.roh()
        outs.append((g["summary"].tobytes(), g["segments"].tobytes(), g["seg_begin"].tobytes(), g["n_sites"].tobytes(), g["counts"].tobytes()))
        assert r.fill_ms() > 0 and r.layout()[2] == 0
        r.close()
    assert outs[0] == outs[1] and any(outs[0][1]) and any(outs[0][0])
    r = vs.roh(regions, segments=False, **kw)
    g = r.roh()
    assert g["segments"] is None and g["seg_begin"] is None and g["params"]["segments"] == 0
    assert (g["summary"].tobytes(), g["n_sites"].tobytes(), g["counts"].tobytes()) == (outs[0][0], outs[0][3], outs[0][4])
    dev = r.roh_device()
    assert dev["segments"] == 0 and dev["seg_begin"] == 0 and dev["n_segments"] == 0 and dev["summary"]
    with pytest.raises(VariantStoreError) as e:
        r.region_text(0)
    assert e.value.code == VS_ERR_ARG
    assert r.region_roh(0, g)["segments"] is None
    r.close()
    m, want, _got = _check_full(vs, regions[:150], None, kw, "t6", texts=30)
    assert m["cells"].shape[0] > 1_000 and want["segments"].shape[0] > 1_000


def test_interleaving_leaves_type6_alone():
    rng = np.random.default_rng(12)
    batches = []
    for k in range(6):
        n = 3_000 + 200 * k + (4_000 if k == 4 else 0)   # like batches (speculated), one larger (refused / re-sized)
        s = np.sort(rng.integers(1_000, 7_990_000, size=n))
        batches.append(np.stack([s, s + rng.integers(50, 3_000, size=n)], axis=1).astype(np.uint64))
    shuffled = batches[3][rng.permutation(batches[3].shape[0])]

    def run(with_roh):
        vs = VariantStore.synthetic(device=0, **T6_KW)
        digests = []
        for b in batches:
            r = vs.get_var_in_ref(b)
            if with_roh:   # ROH batches in between: sorted, unsorted with a subset, summaries only
                for g in (vs.roh(b, min_sites=2), vs.roh(shuffled, [7, 200, 1, 64], min_sites=1, max_het=2), vs.roh(shuffled[:500], segments=False)):
                    g.totals()
                    g.close()
            digests.append(r.digest())
            r.close()
        info = vs.info()
        out = (digests, info.t6_speculated, info.t6_refused)
        vs.close()
        return out

    plain, mixed = run(False), run(True)
    assert plain[1] > 0, "the type-6 batches were not speculated"
    assert plain == mixed


def test_device_pointers(t6_store):
    torch = pytest.importorskip("torch")
    vs, regions = t6_store
    r = vs.roh(regions[:1_000], np.arange(1, 131), min_sites=2, max_het=1)
    got = r.roh()
    dev = r.roh_device()
    Q, S = got["summary"].shape
    n = got["segments"].shape[0]
    assert (dev["n_regions"], dev["n_cols"], dev["n_rows"], dev["n_segments"]) == (Q, S, got["rows"].shape[0], n) and n > 0 and (Q, S) == (1_000, 130)
    assert dev["n_sites"] == dev["summary"] + 32 * Q * S
    later = vs.roh(regions[1_000:1_400], min_sites=1)   # a later batch on the same handle leaves the result alone
    later.totals()
    assert _read_device_bytes(torch, dev["summary"], Q * S, 32).tobytes() == got["summary"].tobytes() and got["summary"].view(np.uint8).any()
    assert _read_device_bytes(torch, dev["n_sites"], Q, 4).tobytes() == got["n_sites"].tobytes() and got["n_sites"].any()
    assert _read_device_bytes(torch, dev["seg_begin"], Q * S + 1, 8).tobytes() == got["seg_begin"].tobytes()
    assert _read_device_bytes(torch, dev["segments"], n, 32).tobytes() == got["segments"].tobytes()
    assert _read_device_bytes(torch, dev["counts"], got["rows"].shape[0], 16).tobytes() == got["counts"].tobytes()
    later.close(); r.close()


def test_size_limits(t6_store):
    """The batch's own bytes are refused before anything is allocated; the segments' bytes after the first pass."""
    vs, regions = t6_store
    kw = dict(min_sites=1, max_het=1)
    first = vs.roh(regions, **kw)
    g = first.roh()
    a, (q, s), n = g["rows"].shape[0], g["summary"].shape, g["segments"].shape[0]
    first.close()
    pitch = (s + 15) // 16 * 16
    base = a * (pitch + 24) + q * s * 44 + q * 4 + 64
    assert base > 4 << 20 and n * 32 > 4 << 20
    warm = vs.allele_counts(regions)   # the plan's temporaries, the table and the counts of this batch are in the handle's pool afterwards
    warm.close()
    try:
        vs.set_option("matrix_max_mib", 4)
        before = vs.info().pool_mallocs
        with pytest.raises(VariantStoreError) as e:
            vs.roh(regions, **kw)
        assert e.value.code == VS_ERR_ARG
        msg = str(e.value)
        for number in (q, s, a, base, a * pitch, a * 24):
            assert str(number) in msg, (number, msg)
        assert "regions" in msg and "columns" in msg and " 0 segments" in msg and "bytes" in msg and "matrix_max_mib" in msg, msg
        assert vs.info().pool_mallocs == before, "a refused batch allocated"
        # room for everything but the segments: refused once pass 1 has counted them
        vs.set_option("matrix_max_mib", (base >> 20) + 2)
        with pytest.raises(VariantStoreError) as e:
            vs.roh(regions, **kw)
        assert e.value.code == VS_ERR_ARG
        msg = str(e.value)
        for number in (q, s, a, n, base + 32 * n, 32 * n):
            assert str(number) in msg, (number, msg)
        assert f" {n} segments" in msg and "matrix_max_mib" in msg, msg
        summaries = vs.roh(regions, segments=False, **kw)   # the same batch without segments fits
        assert summaries.roh()["summary"].tobytes() == g["summary"].tobytes()
        summaries.close()
    finally:
        vs.set_option("matrix_max_mib", 0)
    again = vs.roh(regions, **kw)
    assert again.roh()["segments"].tobytes() == g["segments"].tobytes()
    again.close()


def test_refused_accessors(t6_store):
    vs, regions = t6_store
    r = vs.roh(regions[:1_000], min_sites=2)
    for call in (lambda: r.raw(with_carriers=True), lambda: r.view(with_carriers=True), r.digest, r.num_header_records, r.num_region_records):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_UNSUPPORTED
    for call in (r.allele_counts, r.sample_burden, r.sample_burden_device, r.genotype_matrix, r.genotype_matrix_device, r.ld_band, r.ld_band_device,
                 r.sample_scores, r.sample_gram, r.sample_ibs, r.sample_ibs_device, r.assoc_scan, r.group_counts, r.ld_scores, r.trio_scan, r.trio_scan_device):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_ARG
    r.view(with_carriers=False)
    raw = r.raw(with_carriers=False)
    t6 = vs.get_var_in_ref(regions[:1_000])
    raw6 = t6.raw(with_carriers=False)
    for f in KEY:
        assert np.array_equal(raw["rows"][f], raw6["rows"][f]), f
    assert np.array_equal(raw["region_flags"], raw6["region_flags"]) and np.array_equal(raw["row_count"], raw6["row_count"])
    assert r.totals()[:2] == t6.totals()[:2] and r.fill_ms() > 0 and r.region_text(0).startswith("Sample\tPos1\tPos2\tKB\tNSites\tNHet\n")
    r.close()
    for res in (t6, vs.allele_counts(regions[:10]), vs.genotype_matrix(regions[:10]), vs.trio_scan(regions[:10], [(1, 2, 3)])):
        with pytest.raises(VariantStoreError) as e:
            res.roh()   # not a ROH result
        assert e.value.code == VS_ERR_ARG
        with pytest.raises(VariantStoreError) as e:
            res.roh_device()
        assert e.value.code == VS_ERR_ARG
        res.close()


# ------------------------------------------------------------------------------------------------------------ the CLI
def test_cli_roh(tmp_path):
    exe = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    fasta, vcf, names, positions, _dos = write_roh_cohort(str(tmp_path), seed=11, n_samples=40, n_rows=200, single_from=80, single_to=100, regular_from=150)
    subprocess.run([exe, "construct", "-r", fasta, "-v", vcf, "-p", prefix], check=True, capture_output=True)
    vs = VariantStore.open(prefix, device=0)
    regions = sorted(regions_of_rows(positions, [(0, 199), (50, 120), (140, 199)]))   # (the command line sorts its regions)
    rfile, sfile, out = os.path.join(tmp_path, "regions.txt"), os.path.join(tmp_path, "samples.txt"), os.path.join(tmp_path, "roh.txt")
    with open(rfile, "w") as f:
        f.write("".join(f"{x}:{y}\n" for x, y in regions))
    chosen = [names[k] for k in (3, 4, 9, 20, 21, 22, 39)]
    with open(sfile, "w") as f:
        f.write("".join(n + "\n" for n in chosen))
    flags = ["--min-sites", "3", "--max-het", "1", "--max-gap", "300", "--min-bp", "20", "--min-ac", "2", "--max-ac", "70"]
    kw = dict(min_sites=3, max_het=1, max_gap=300, min_bp=20, min_ac=2, max_ac=70)

    def run(more):
        p = subprocess.run([exe, "roh", "-p", prefix, "-r", "@" + rfile, "-S", sfile, "-o", out] + flags + more, check=True, capture_output=True)
        assert p.stdout == b""
        with open(out, "rb") as f:
            return f.read().decode("latin-1")

    _m, want, got = _check_full(vs, regions, chosen, kw, "cli", texts=1)
    assert want["segments"].shape[0] > 10 and (want["segments"]["n_het"] > 0).any()
    text = run([])
    assert text == cli_segments_text(want["segments"], chosen, regions)
    res = vs.roh(regions, chosen, **kw)
    body = "".join("".join(f"{ln.split(chr(9), 1)[0]}\t{x}:{y}\t{ln.split(chr(9), 1)[1]}\n" for ln in res.region_text(q).split("\n")[1:] if ln)
                   for q, (x, y) in enumerate(regions))
    assert text == "Sample\tRegion\tPos1\tPos2\tKB\tNSites\tNHet\n" + body
    res.close()
    assert run(["--summary"]) == cli_summary_text(want["summary"], chosen, regions)
    vs.close()
