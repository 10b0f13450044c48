"""ROH queries without a GPU: the reference's state machine against its second formulation (max_het == 0) and against the invariants
(max_het > 0) on random columns, hand-written cases with the answer written out, the derived floats, the conditions the GPU test's
cohort must meet (from the writer's own dosages), the argument checks of vs_query_roh (made on the host, before the handle's device
is asked for) in their order, the Python wrapper's codes, and the CLI's argument parsing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import write_random_cohort
from roh_cohort import COHORT_KW, PARAM_SETS, REGION_ROWS, conditions_met, dosages_of_vcf, write_planted_cohort, write_roh_cohort
from roh_ref import (SEGMENT_DTYPE, SUMMARY_DTYPE, check_invariants, cli_segments_text, cli_summary_text, derived, dosage, fold, new_stats, params,
                     region_text, roh_batch, roh_region, runs_column, site_mask, walk_column)
from variantstore_amd import VariantStore, _lib, roh_derived
from variantstore_amd.api import QueryResult, VariantStoreError

VS_ERR_NO_DEVICE, VS_ERR_ARG, VS_ERR_UNKNOWN_SAMPLE = -3, -5, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
CELL_OF_DOSAGE = np.asarray([0, 0x0A, 0x0F], np.uint8)   # 0, 1|0 unphased-bit clear, 1|1 phased


def _column(states, pos=None, **kw):
    """One column given as a string: 'o' hom, 'x' het, '.' a row that is no site.  Returns (segments, summary, n_sites)."""
    n = len(states)
    pos = list(range(100, 100 + 10 * n, 10)) if pos is None else pos
    d = np.asarray([[1 if ch == "x" else 0] for ch in states])
    site = np.asarray([ch != "." for ch in states])
    summary, segs, n_sites = roh_region(CELL_OF_DOSAGE[d], pos, site, params(**kw))
    return [s[2:] for s in segs], summary[0], n_sites


# ------------------------------------------------------------------------------------------------ hand-written cases
def test_het_overflow_closes_and_restarts_the_run():
    #         rows 0123456789
    segs, s, n = _column("ooxooxxoo", min_sites=1, max_het=1)
    # run 1: rows 0-4 absorbs the het at 2; the het at 5 is pending (1 < 1 is false: n_het 1 + pend 0 >= max_het) -> it closes the run
    # at once; the het at 6 finds no run; run 2: rows 7-8
    assert segs == [(100, 140, 0, 4, 5, 1), (170, 180, 7, 8, 2, 0)]
    assert (int(s["n_segments"]), int(s["seg_sites"]), int(s["total_bp"]), int(s["seg_hets"]), int(s["n_het"])) == (2, 7, 41 + 11, 1, 3) and n == 9
    assert (int(s["longest_bp"]), int(s["longest_sites"])) == (41, 5)
    # the hets a closed run had absorbed are not revisited: with max_het = 1 "oxoxo" is ONE run up to row 2, then a new one from row 4
    segs, _s, _n = _column("oxoxo", min_sites=1, max_het=1)
    assert segs == [(100, 120, 0, 2, 3, 1), (140, 140, 4, 4, 1, 0)]
    # max_het = 0: every het closes
    segs, _s, _n = _column("ooxoo", min_sites=1)
    assert segs == [(100, 110, 0, 1, 2, 0), (130, 140, 3, 4, 2, 0)]


def test_trailing_hets_are_trimmed():
    segs, s, _n = _column("oooxx", min_sites=1, max_het=3)
    assert segs == [(100, 120, 0, 2, 3, 0)] and int(s["seg_hets"]) == 0 and int(s["n_het"]) == 2
    segs, _s, _n = _column("xxooxoxx", min_sites=1, max_het=3)      # leading hets open nothing, trailing ones are dropped
    assert segs == [(120, 150, 2, 5, 4, 1)]
    # a pending het counts against max_het while it is pending: "ooxx" + "x" with max_het 2 closes at the third het
    segs, _s, _n = _column("ooxxxoo", min_sites=1, max_het=2)
    assert segs == [(100, 110, 0, 1, 2, 0), (150, 160, 5, 6, 2, 0)]


def test_the_gap_is_measured_to_a_pending_het():
    # sites at 100 110 120(het) 500 510: the gap 120 -> 500 closes the run although the run's last hom site is 110; and the gap
    # 110 -> 120 is none.  Were the gap measured from the last hom site the answer would be the same here, so a second case: het at
    # 300, hom at 500 with max_gap 250: 110 -> 300 and 300 -> 500 are both within it, 110 -> 500 is not -- ONE run.
    segs, _s, _n = _column("ooxoo", pos=[100, 110, 120, 500, 510], min_sites=1, max_het=2, max_gap=100)
    assert segs == [(100, 110, 0, 1, 2, 0), (500, 510, 3, 4, 2, 0)]
    segs, _s, _n = _column("ooxoo", pos=[100, 110, 300, 500, 510], min_sites=1, max_het=2, max_gap=250)
    assert segs == [(100, 510, 0, 4, 5, 1)]
    # rows that are no sites neither break nor extend, and the gap is between SITES: 100 .(200) .(300) 400 with max_gap 250 closes
    segs, _s, n = _column("o..o", pos=[100, 200, 300, 400], min_sites=1, max_gap=250)
    assert segs == [(100, 100, 0, 0, 1, 0), (400, 400, 3, 3, 1, 0)] and n == 2
    segs, _s, _n = _column("o..o", pos=[100, 200, 300, 400], min_sites=1, max_gap=300)
    assert segs == [(100, 400, 0, 3, 2, 0)]
    # max_gap = 0: no gap rule
    segs, _s, _n = _column("oo", pos=[100, 4_000_000_000], min_sites=1)
    assert segs == [(100, 4_000_000_000, 0, 1, 2, 0)]


def test_same_position_multi_allelic_rows():
    # two ALT rows of one record share a position; a 1|2 call is het on both.  A difference that would be negative counts as 0.
    segs, s, _n = _column("ooxxoo", pos=[100, 110, 120, 120, 130, 130], min_sites=1, max_het=2, max_gap=10)
    assert segs == [(100, 130, 0, 5, 6, 2)] and int(s["total_bp"]) == 31
    segs, _s, _n = _column("ooo", pos=[100, 90, 95], min_sites=1, max_gap=5)    # 100 -> 90 counts as 0; 90 -> 95 is 5
    assert segs == [(100, 95, 0, 2, 3, 0)]
    _segs, s, _n = _column("ooo", pos=[100, 90, 95], min_sites=1)
    assert int(s["total_bp"]) == 1 and int(s["longest_bp"]) == 1             # bp = max(95 - 100, 0) + 1
    segs, _s, _n = _column("oo", pos=[100, 100], min_sites=2, min_bp=1)
    assert segs == [(100, 100, 0, 1, 2, 0)]


def test_min_sites_and_min_bp_each_reject_a_run():
    stats = new_stats()
    d = np.asarray([[0], [0], [1], [0], [0], [0], [1], [0]])
    pos = [100, 105, 110, 200, 300, 400, 410, 500]
    summary, segs, _n = roh_region(CELL_OF_DOSAGE[d], pos, np.ones(8, bool), params(min_sites=2, min_bp=50), stats=stats)
    # runs: rows 0-1 (2 sites, 6 bp: min_bp rejects), rows 3-5 (3 sites, 201 bp: kept), row 7 (1 site: min_sites rejects)
    assert [s[2:] for s in segs] == [(200, 400, 3, 5, 3, 0)]
    assert stats == {"closed_gap": 0, "closed_het": 2, "closed_end": 1, "rejected_min_sites": 1, "rejected_min_bp": 1}
    assert int(summary[0]["n_segments"]) == 1 and int(summary[0]["n_het"]) == 2


def test_longest_tie_goes_to_the_earlier_segment():
    segs, s, _n = _column("oooxooo" + "x" + "oo", pos=[100, 110, 120, 130, 140, 145, 160, 170, 180, 200], min_sites=1)
    assert [g[4] for g in segs] == [3, 3, 2] and (int(s["longest_bp"]), int(s["longest_sites"])) == (21, 3)
    segs, s, _n = _column("ooxooo", pos=[100, 120, 130, 140, 150, 160], min_sites=1)     # 21 bp with 2 sites, then 21 bp with 3
    assert (int(s["longest_bp"]), int(s["longest_sites"])) == (21, 2)


def test_an_empty_region_and_a_region_of_ineligible_rows():
    p = params(min_sites=1)
    out = roh_batch(np.zeros((0, 3), np.uint8), np.zeros(0), np.zeros(0, bool), [0], [0], p)
    assert out["summary"].shape == (1, 3) and not out["summary"].view(np.uint8).any() and out["n_sites"].tolist() == [0]
    assert out["segments"].shape == (0,) and out["seg_begin"].tolist() == [0, 0, 0, 0]
    # ineligible rows only: monomorphic (nobody carries it / everybody 1|1), dropped, outside the ac window
    d = np.asarray([[0, 0, 0], [2, 2, 2], [1, 0, 0], [0, 1, 1]])
    cells = CELL_OF_DOSAGE[d]
    dropped = np.asarray([0, 0, 1, 0], bool)
    cells[2] = 0
    site = site_mask(cells, dropped, min_ac=3, max_ac=5)
    assert site.tolist() == [False, False, False, False]
    assert site_mask(cells, dropped).tolist() == [False, False, False, True]
    assert site_mask(CELL_OF_DOSAGE[np.asarray([[1, 1, 1]])], [False]).tolist() == [True]   # every column het: ac = n, a site
    out = roh_batch(cells, [10, 20, 30, 40], site, [0], [4], p)
    assert not out["summary"].view(np.uint8).any() and out["n_sites"].tolist() == [0] and out["segments"].shape == (0,)


# ------------------------------------------------------------------------------------ the two formulations, the invariants
def _random_columns(rng, n_rows, n_cols, het_p):
    d = (rng.random((n_rows, n_cols)) < het_p).astype(np.int64)
    d[(d == 0) & (rng.random((n_rows, n_cols)) < 0.3)] = 2
    pos = 50 + np.cumsum(rng.choice([0, 1, 3, 10, 40, 300], size=n_rows, p=[0.05, 0.2, 0.3, 0.3, 0.1, 0.05]))
    site = rng.random(n_rows) < 0.8
    return CELL_OF_DOSAGE[d], pos, site


@pytest.mark.parametrize("seed", range(6))
def test_the_two_formulations_agree_on_random_columns(seed):
    rng = np.random.default_rng(seed)
    cells, pos, site = _random_columns(rng, 300, 12, het_p=(0.05, 0.15, 0.4)[seed % 3])
    n_segments = 0
    for kw in (dict(min_sites=1), dict(min_sites=3), dict(min_sites=1, max_gap=30), dict(min_sites=2, min_bp=25, max_gap=9), dict(min_sites=4, min_bp=100)):
        p = params(**kw)
        s1, g1, n1 = roh_region(cells, pos, site, p)
        s2, g2, n2 = roh_region(cells, pos, site, p, walker=runs_column)
        assert g1 == g2 and s1.tobytes() == s2.tobytes() and n1 == n2 == int(site.sum()), kw
        n_segments += len(g1)
    assert n_segments > 100


@pytest.mark.parametrize("seed", range(6))
def test_invariants_hold_with_hets_allowed(seed):
    rng = np.random.default_rng(100 + seed)
    cells, pos, site = _random_columns(rng, 300, 10, het_p=(0.1, 0.3)[seed % 2])
    idx = np.nonzero(site)[0]
    d = dosage(cells[idx])
    with_hets = 0
    for kw in (dict(min_sites=1, max_het=1), dict(min_sites=5, max_het=3), dict(min_sites=2, max_het=2, max_gap=30), dict(min_sites=3, max_het=255, min_bp=40)):
        p = params(**kw)
        summary, segs, _n = roh_region(cells, pos, site, p)
        for c in range(cells.shape[1]):
            mine = [g[2:] for g in segs if g[1] == c]
            check_invariants(summary[c], mine, d[:, c] == 1, pos[idx], idx, p)
            with_hets += sum(g[5] > 0 for g in mine)
        # max_het = 255 and no other rule: one run from the first hom site to the last
        if kw.get("max_het") == 255:
            assert all(int(summary[c]["n_segments"]) <= 1 for c in range(cells.shape[1]))
    assert with_hets > 20
    # max_het = 0 through the machine equals max_het = 0 through the runs, and more hets never give more segments of one site
    assert roh_region(cells, pos, site, params(min_sites=1))[1] == roh_region(cells, pos, site, params(min_sites=1), walker=runs_column)[1]


# ------------------------------------------------------------------------------------------------------ the derived floats
def test_derived_floats():
    s = np.zeros((2, 3), SUMMARY_DTYPE)
    s["total_bp"] = [[0, 1500, 3_000_000_001], [10, 999, 20]]
    s["n_segments"] = [[0, 2, 3], [1, 4, 1]]
    got = roh_derived(s, lengths=[1_000_000, 0])
    assert got["kb"].tolist() == [[0.0, 1.5, 3000000.001], [0.01, 0.999, 0.02]]
    assert np.isnan(got["kb_avg"][0, 0]) and got["kb_avg"][0, 1:].tolist() == [1500 / 2000.0, 3_000_000_001 / 3000.0] and got["kb_avg"][1].tolist() == [0.01, 999 / 4000.0, 0.02]
    assert got["froh"][0].tolist() == [0.0, 0.0015, 3_000_000_001 / 1_000_000.0] and np.isnan(got["froh"][1]).all()
    want = derived(s, [1_000_000, 0])
    for k in ("kb", "kb_avg", "froh"):
        assert got[k].dtype == np.float64 and got[k].tobytes() == want[k].tobytes(), k
    assert "froh" not in roh_derived(s)
    with pytest.raises(ValueError):
        roh_derived(s, lengths=[1, 2, 3])
    assert QueryResult.ROH_SUMMARY_DTYPE == SUMMARY_DTYPE and QueryResult.ROH_SEGMENT_DTYPE == SEGMENT_DTYPE and SUMMARY_DTYPE.itemsize == SEGMENT_DTYPE.itemsize == 32


def test_texts():
    seg = np.zeros(2, SEGMENT_DTYPE)
    seg[0] = (0, 1, 100, 2099, 0, 40, 41, 2)
    seg[1] = (1, 0, 5, 5, 3, 3, 1, 0)
    assert region_text(seg[:1], ["a", "b"]) == "Sample\tPos1\tPos2\tKB\tNSites\tNHet\nb\t100\t2099\t2.000\t41\t2\n"
    assert cli_segments_text(seg, ["a", "b"], [(1, 3000), (4, 9)]) == ("Sample\tRegion\tPos1\tPos2\tKB\tNSites\tNHet\nb\t1:3000\t100\t2099\t2.000\t41\t2\n"
                                                                     "a\t4:9\t5\t5\t0.001\t1\t0\n")
    s = np.zeros((1, 2), SUMMARY_DTYPE)
    s[0, 1] = fold([(100, 2099, 0, 40, 41, 2), (3000, 3000, 50, 50, 1, 0)], 7)
    assert cli_summary_text(s, ["a", "b"], [(1, 3000)]) == ("Sample\tRegion\tNSeg\tKB\tKBAvg\tLongestKB\tNHet\na\t1:3000\t0\t0.000\tNA\t0.000\t0\n"
                                                           "b\t1:3000\t2\t2.001\t1.000\t2.000\t7\n")


# --------------------------------------------------------------------------- the GPU test's cohorts, from the writer's arrays
def test_the_gpu_cohort_meets_its_conditions(tmp_path):
    """What tests/test_gpu_roh.py asserts on the expected values it forms on the GPU box, checked here from the writer's own dosages
    (every record a well-separated SNP: the table is the VCF's records in order) under the same parameter sets."""
    _fa, vcf, names, positions, d = write_roh_cohort(str(tmp_path), **COHORT_KW)
    pos2, names2, d2 = dosages_of_vcf(vcf)
    assert np.array_equal(pos2, positions) and names2 == names and np.array_equal(d2, d)
    cells = CELL_OF_DOSAGE[d]
    n_rows = cells.shape[0]
    row_begin, row_count = [a for a, _b in REGION_ROWS], [b - a + 1 for a, b in REGION_ROWS]
    stats, outs = new_stats(), []
    for kw in PARAM_SETS:
        p = params(**kw)
        site = site_mask(cells, np.zeros(n_rows, bool), p["min_ac"], p["max_ac"])
        outs.append((p, roh_batch(cells, positions, site, row_begin, row_count, p, stats)))
    conditions_met(stats, outs)


def test_the_planted_cohort_has_exactly_its_planted_stretches(tmp_path):
    _fa, vcf, names, positions, planted = write_planted_cohort(str(tmp_path))
    pos, names2, d = dosages_of_vcf(vcf)
    assert names2 == names and np.array_equal(pos, positions)
    site = site_mask(CELL_OF_DOSAGE[d], np.zeros(d.shape[0], bool))
    assert site.all()
    _s, segs, _n = roh_region(CELL_OF_DOSAGE[d], pos, site, params(min_sites=20))
    assert sorted((g[1], g[4], g[5]) for g in segs) == sorted(planted)
    _s, segs2, _n = roh_region(CELL_OF_DOSAGE[d], pos, site, params(min_sites=20), walker=runs_column)
    assert segs == segs2


# ------------------------------------------------------------------------------------------------------ the C ABI on the host
@pytest.fixture(scope="module")
def host_store(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("roh_host"))
    fasta, vcf, _names = write_random_cohort(d, 4101, ref_len=6000, n_samples=9, carrier_p=0.5)
    vs = VariantStore.from_vcf(fasta, vcf, device=-1)
    yield vs
    vs.close()


def _call(vs, ids=None, n=1, n_ids=None, null_params=False, **kw):
    lib = _lib.load()
    regions = (_lib.Region * 1)(_lib.Region(1, 100))
    h = C.c_void_p()
    ptr = None if ids is None else (C.c_uint32 * max(len(ids), 1))(*ids)
    n_ids = (0 if ids is None else len(ids)) if n_ids is None else n_ids
    vals = dict(min_sites=50, min_bp=0, max_gap=0, max_het=0, min_ac=0, max_ac=0xFFFFFFFF, segments=1)
    vals.update(kw)
    prm = _lib.RohParams(**vals)
    return lib.vs_query_roh(vs._h, regions, n, ptr, n_ids, None if null_params else C.byref(prm), C.byref(h))


def _err():
    return _lib.load().vs_last_error().decode()


def test_entry_points_are_declared():
    lib = _lib.load()
    for name in ("vs_query_roh", "vs_result_get_roh", "vs_result_roh_device"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "variantstore_hip.h")).read()
    assert "typedef struct { uint32_t n_segments, seg_sites; uint64_t total_bp; uint32_t longest_bp, longest_sites, seg_hets, n_het; } vs_roh_summary;" in header
    assert "typedef struct { uint32_t region, column, pos_first, pos_last, row_first, row_last, n_sites, n_het; } vs_roh_segment;" in header
    assert C.sizeof(_lib.RohParams) == 28


def test_argument_errors_and_their_order(host_store):
    ns = host_store.info().num_samples
    assert _call(host_store, n=0) == VS_ERR_ARG and "region" in _err()
    assert _call(host_store, [], n_ids=0) == VS_ERR_ARG and "empty sample subset" in _err()
    assert _call(host_store, None, n_ids=3) == VS_ERR_ARG and "null" in _err()
    assert _call(host_store, null_params=True) == VS_ERR_ARG and "params" in _err()
    assert _call(host_store, min_sites=0) == VS_ERR_ARG and "min_sites" in _err()
    assert _call(host_store, max_het=256) == VS_ERR_ARG and "256" in _err()
    assert _call(host_store, max_het=255) == VS_ERR_NO_DEVICE
    assert _call(host_store, min_ac=5, max_ac=4) == VS_ERR_ARG and "[5, 4]" in _err()
    assert _call(host_store, min_ac=4, max_ac=4) == VS_ERR_NO_DEVICE
    for bad in ([0], [1, ns], [0xFFFFFFFF, 2]):
        assert _call(host_store, bad) == VS_ERR_UNKNOWN_SAMPLE, bad
    # the order: regions < params < min_sites < max_het < the ac window < the sample ids < the device
    assert _call(host_store, [0], n=0, null_params=True) == VS_ERR_ARG and "region" in _err()
    assert _call(host_store, [0], null_params=True) == VS_ERR_ARG and "params" in _err()
    assert _call(host_store, [0], min_sites=0, max_het=300, min_ac=2, max_ac=1) == VS_ERR_ARG and "min_sites" in _err()
    assert _call(host_store, [0], max_het=300, min_ac=2, max_ac=1) == VS_ERR_ARG and "300" in _err()
    assert _call(host_store, [0], min_ac=2, max_ac=1) == VS_ERR_ARG and "[2, 1]" in _err()
    assert _call(host_store, [0]) == VS_ERR_UNKNOWN_SAMPLE
    assert _call(host_store, [1, 2, 2, 9]) == VS_ERR_NO_DEVICE
    assert _call(host_store) == VS_ERR_NO_DEVICE


def test_wrapper_raises_the_same_codes(host_store):
    name = host_store.sample_name(3)
    cases = ((dict(), VS_ERR_NO_DEVICE), (dict(samples=[name, 2]), VS_ERR_NO_DEVICE), (dict(min_sites=0), VS_ERR_ARG), (dict(max_het=256), VS_ERR_ARG),
             (dict(min_ac=3, max_ac=2), VS_ERR_ARG), (dict(samples=[0]), VS_ERR_UNKNOWN_SAMPLE), (dict(samples=[]), VS_ERR_ARG),
             (dict(segments=False, max_ac=None, max_gap=0xFFFFFFFF), VS_ERR_NO_DEVICE))
    for kw, code in cases:
        with pytest.raises(VariantStoreError) as e:
            host_store.roh([(1, 100)], **kw)
        assert e.value.code == code, kw
    with pytest.raises(VariantStoreError) as e:
        host_store.roh([])
    assert e.value.code == VS_ERR_ARG
    for kw in (dict(min_bp=-1), dict(max_gap=1 << 32), dict(min_sites=1 << 40)):
        with pytest.raises(ValueError):
            host_store.roh([(1, 100)], **kw)


# ------------------------------------------------------------------------------------------------------------------ the CLI
def test_cli_argument_parsing(tmp_path):
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    fasta, vcf, names = write_random_cohort(str(tmp_path), 4101, ref_len=6000, n_samples=9, carrier_p=0.5)
    subprocess.run([CLI, "construct", "-r", fasta, "-v", vcf, "-p", prefix], check=True, capture_output=True)

    def run(*argv):
        p = subprocess.run([CLI, "roh", *argv], capture_output=True, text=True)
        return p.returncode, p.stdout + p.stderr

    for argv in (["-p", prefix], ["-r", "1:100"], []):   # something is missing: the usage
        rc, out = run(*argv)
        assert rc != 0 and "variantstore roh" in out and "--min-sites" in out and "--summary" in out, argv
    base = ["-p", prefix, "-r", "1:100", "--device", "-1"]
    rc, out = run(*base, "--king")
    assert rc != 0 and "unknown option" in out
    for flag in ("--min-sites", "--min-bp", "--max-gap", "--max-het", "--min-ac", "--max-ac"):
        for bad in ("abc", "-1", "1.5", "4294967296", "", "12x"):
            rc, out = run(*base, flag, bad)
            assert rc != 0 and f"{flag} takes a whole number" in out and "variantstore roh" in out, (flag, bad, out)
    rc, out = run(*base, "--min-sites", "0")
    assert rc != 0 and "--min-sites takes at least 1" in out
    rc, out = run(*base, "--max-het", "256")
    assert rc != 0 and "--max-het takes at most 255" in out
    rc, out = run(*base, "--min-ac", "5", "--max-ac", "4")
    assert rc != 0 and "--min-ac 5 is above --max-ac 4" in out
    # well-formed command lines fail only for want of a device
    sfile = os.path.join(tmp_path, "samples.txt")
    with open(sfile, "w") as f:
        f.write(f"{names[0]}\n{names[4]}\n")
    for more in ([], ["--summary"], ["--min-sites", "1", "--min-bp", "4294967295", "--max-gap", "1000", "--max-het", "255", "--min-ac", "2", "--max-ac", "9"],
                 ["-S", sfile, "--summary", "-o", os.path.join(tmp_path, "out.txt")]):
        rc, out = run(*base, *more)
        assert rc != 0 and "device" in out.lower() and "variantstore roh" not in out and "takes" not in out, (more, out)
    with open(sfile, "w") as f:
        f.write("nobody-of-that-name\n")
    rc, out = run(*base, "-S", sfile)
    assert rc != 0 and "nobody-of-that-name" in out
