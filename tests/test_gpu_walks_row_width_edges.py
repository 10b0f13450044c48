"""The walking queries -- types 2, 3 and 5 (sample coordinates), 1 and 7 (points) -- on the cohorts whose class rows are as wide or as
full as rows get: tests/test_gpu_row_width_edges.py holds types 6 and 4 to the oracle there, tests/test_gpu_saturated_columns.py the
column queries.  What is width-dependent in the walks themselves is sample_entry_rec (k_sample_coords.hip.h): the rank of the
sample's bit in its class row -- the ones below it in its word, plus the 16-bit prefix table class_cum, minus the ref bit -- indexes
car_index, and a rank that is off by one hands the sample another carrier's coordinate: types 3 and 5 answer wrongly while types 6
and 4 stay right.

  saturated  helpers.write_saturated_cohort(n, 4400 + n, rows=150, two_alt=False, extremes=True) at 63, 64, 4031, 4032, 4095 and
             4159 samples: 1, 2, 63, 64, 64 and 65 row words, rows carried by 75 - 100 % of the samples.
  switch     the same with 40 rows at 65,534 samples (info().num_samples 65,535: the table exists and its entries reach 65,472, above
             32,767) and at 65,535 (65,536: no table, sample_entry_rec loops over the row's 1,024 words).
  spread     VariantStore.synthetic(sample_coordinates=True) of test_gpu_row_width_edges at 4031 and 4095 samples: listed, medium
             and dense classes, ranks of every size.

Samples: ids 1, 63, 64, the first id of the last row word, n, and "ref" -- each with a batch of its own, and one batch with one sample
per region, cycling through them, so that the lanes of a wave read different row words.  Regions: five records each on the midpoints
of the gaps between records (38 of 150 rows, 10 of 40).  Every check is text-exact or flag-exact against the oracle; type 2 also
against vcf_truth.sample_sequence, which never passes through the constructor.  Every check runs in each kernel form: the cooperative
walk, one lane per region, the count-then-emit fallbacks, and without the per-sample rows (record_has_sample then reads the class
rows).  tests/test_dense_explicit_host.py asserts the conditions on these inputs on the CPU; the ones a pass depends on are
asserted again here, from the oracle's answers."""
import numpy as np
import pytest

import vcf_truth as vt
from helpers import SAT_REF_LEN
from test_dense_explicit_host import (SAT_WIDTHS, SWITCH_SEED, Memo, edge_ids, flagged, fully_carried_lines, neighbour_differences,
                                      open_cohort, predicted_sequences, sample_name, walk_regions)
from test_gpu_parity import _parse_rows, _sc_regions
from test_gpu_row_width_edges import SPREAD_KW, SPREAD_SEED
from oracle.oracle import Oracle
from variantstore_amd import VariantStore

pytestmark = pytest.mark.gpu

FORMS = {                      # name -> (option, value for the form, value that puts it back)
    "cooperative": ("t4_walk", 2, 2),
    "one_lane": ("t4_walk", 1, 2),
    "fallbacks": ("force_fallbacks", 1, 0),
    "no_rows": ("t4_rows_max_mb", 0, 1 << 20),
}


def _check_seq(vs, orc, regions, samples, coords):
    """query_sample_seq of one batch (`samples`: one name, or one per region) against the oracle: flags, sequences, region_text, the
    total length.  Returns (answered, flagged)."""
    per = samples if isinstance(samples, list) else [samples] * len(regions)
    res = vs.query_sample_seq(regions, samples, sample_coordinates=bool(coords))
    flags, seqs = res.sequences()
    ok = bad = 0
    for q, (x, y) in enumerate(regions):
        n, seq = (orc.query_sample_from_sample if coords else orc.query_sample_from_ref)(x, y, per[q])
        if n == -1:
            assert flags[q] & 8, (per[q], coords, x, y)
        elif n == -3:
            assert flags[q] & 2, (per[q], coords, x, y)
        else:
            assert n == len(seq) and not flags[q] and seqs[q] == seq, (per[q], coords, x, y)
            assert res.region_text(q) == seq + "\n"
            ok += 1
        bad += flagged(n)
    assert res.totals()[3] == sum(len(s) for s in seqs)
    res.close()
    return ok, bad


def _check_t5(vs, orc, regions, samples):
    """get_sample_var_in_sample of one batch against the oracle: text (with the full carrier lists), var_count, flags."""
    per = samples if isinstance(samples, list) else [samples] * len(regions)
    res = vs.get_sample_var_in_sample(regions, samples)
    view = res.view(False)
    ok = bad = 0
    for q, (x, y) in enumerate(regions):
        n, text = orc.get_sample_var_in_sample(x, y, per[q])
        if n == -1:
            assert view["region_flags"][q] & 8, (per[q], x, y)
            bad += 1
            continue
        assert n >= 0 and not view["region_flags"][q] and res.region_text(q) == text, (per[q], x, y)
        assert int(view["var_count"][q]) == n
        ok += 1
    res.close()
    return ok, bad


def _walks(vs, orc, regions, names, forms, max_flagged):
    """Types 2, 3 and 5 for every sample of `names` and for the batch that cycles through them, under every kernel form."""
    mixed = [names[q % len(names)] for q in range(len(regions))]
    for form in forms:
        option, on, off = FORMS[form]
        vs.set_option(option, on)
        try:
            if form == "no_rows":
                assert vs.info().t4_rows_bytes == 0
            for smp in names + [mixed]:
                for coords in (0, 1):
                    ok, bad = _check_seq(vs, orc, regions, smp, coords)
                    assert ok + bad == len(regions) and bad <= max_flagged, (form, smp, coords, bad)
                ok, bad = _check_t5(vs, orc, regions, smp)
                assert ok + bad == len(regions) and bad <= max_flagged, (form, smp, bad)
        finally:
            vs.set_option(option, off)
        if form == "no_rows":
            assert vs.info().t4_rows_bytes > 0, "the per-sample rows did not come back"


def _check_text_sequences(vs, fasta, names, recs, regions, sids):
    """Type 2 against the VCF and FASTA text (no constructor, no oracle) wherever vcf_truth.sample_sequence predicts: at least half
    of each sample's regions."""
    for sid in sids:
        want = predicted_sequences(fasta, names, recs, regions, sid)
        assert len(want) >= len(regions) // 2, (sid, len(want))
        qs = sorted(want)
        res = vs.query_sample_seq([regions[q] for q in qs], sample_name(sid))
        flags, seqs = res.sequences()
        assert not flags.any() and seqs == [want[q] for q in qs], sid
        res.close()


def _check_points(vs, orc, n, min_hits, every_offset=True):
    """Type 1 at every 37th position of the reference and past its end; type 7 for every row type 6 reports, at pos - 2 .. pos + 1 and
    with a wrong ALT -- compared as tests/test_gpu_parity.py compares them."""
    positions = list(range(0, SAT_REF_LEN + 1, 37)) + [SAT_REF_LEN + 40, 2 ** 31 + 5, 2 ** 32 + 7] if every_offset else []
    if positions:
        res = vs.closest_var(positions)
        fl = res.view(False)["region_flags"]
        for q, p in enumerate(positions):
            cnt, text = orc.closest_var(p)
            if cnt < 0:
                assert fl[q] & 4 and res.region_text(q) == "", p
            else:
                assert not (fl[q] & 4) and res.region_text(q) == text, p
        res.close()
    rows = _parse_rows(orc.get_var_in_ref(1, SAT_REF_LEN + 1)[2])
    qs = []
    for pos, ref, alt in rows:
        qs += [(pos + d, ref, alt) for d in ((-2, -1, 0, 1) if every_offset else (0,))]
        qs.append((pos, ref, alt + "C"))
    res = vs.samples_has_var([q[0] for q in qs], [q[1] for q in qs], [q[2] for q in qs])
    fl = res.view(False)["region_flags"]
    hits = 0
    for q, (pos, ref, alt) in enumerate(qs):
        want = orc.samples_has_var(pos, ref, alt)
        if want is None:
            assert fl[q] & 4 and res.region_text(q) == "", qs[q]
        else:
            assert not (fl[q] & 4) and res.region_text(q) == want, qs[q]
            hits += want.count("|") + want.count("/") >= 0.75 * n      # (one `name a|b` or `name a/b` per carrier)
    res.close()
    assert hits >= min_hits, hits


@pytest.mark.parametrize("n", SAT_WIDTHS)
def test_walks_on_saturated_rows_at_the_width_edges(n, tmp_path):
    vs, orc, names, recs, (fasta, _vcf, _plain) = open_cohort(tmp_path, n, 0, rows=150, extremes=True)
    info = vs.info()
    wpc = (n + 1 + 63) // 64
    assert info.num_samples - 1 == n and info.use_bit_vector and (info.num_samples + 63) // 64 == wpc
    assert wpc == {63: 1, 64: 2, 4031: 63, 4032: 64, 4095: 64, 4159: 65}[n]
    regions = walk_regions(vt.gap_midpoints(recs, SAT_REF_LEN))
    assert len(regions) == 38
    sids = edge_ids(n)
    for sid in sids:     # a rank off by one is visible: the id neighbours' answers differ on at least half of the regions
        diff = neighbour_differences(orc, regions, n, sid)
        assert diff and min(diff.values()) >= len(regions) // 2, (sid, diff)
    _walks(vs, orc, regions, [sample_name(i) for i in sids] + ["ref"], list(FORMS), len(regions) // 10)
    _check_text_sequences(vs, fasta, names, recs, regions, sids)
    _check_points(vs, orc, n, 2)
    vs.close()


@pytest.mark.parametrize("n", sorted(SWITCH_SEED))
def test_walks_on_both_sides_of_the_class_cum_switch(n, tmp_path):
    """65,534 samples: class_cum exists, its entries pass 32,767 and reach 65,472.  65,535 samples: no table, the word loop.  Sample n
    carries a row that everybody carries -- a rank above 65,000 -- and reports it in sample coordinates.
    (The oracle takes 0.1 s per region here and a second per type-1 call: ids 1, 65,472 and n, ten regions, the cooperative walk and the
    dropped rows, type 7 at every row's own position and with a wrong ALT, no type 1.)"""
    vs, orc, names, recs, (fasta, _vcf, _plain) = open_cohort(tmp_path, n, 0, rows=40, extremes=True)
    info = vs.info()
    assert info.num_samples == n + 1 == {65534: 65535, 65535: 65536}[n] and info.use_bit_vector and (info.num_samples + 63) // 64 == 1024
    regions = walk_regions(vt.gap_midpoints(recs, SAT_REF_LEN))
    sids = edge_ids(n)
    assert len(regions) == 10 and sids == [1, 65472, n]
    for sid in sids:
        diff = neighbour_differences(orc, regions, n, sid, enough=2)
        assert diff and min(diff.values()) >= 2, (sid, diff)
    top = [orc.get_sample_var_in_sample(x, y, sample_name(n)) for x, y in regions]
    assert any(fully_carried_lines(t, n) for c, t in top if c >= 0), "no row carried by everybody among sample n's reports"
    _walks(vs, orc, regions, [sample_name(i) for i in sids], ["cooperative", "no_rows"], 1)
    _check_text_sequences(vs, fasta, names, recs, regions, sids)
    _check_points(vs, orc, n, 2, every_offset=False)
    vs.close()


@pytest.mark.parametrize("n", [4031, 4095])
def test_walks_on_spread_cohorts_at_the_width_edges(n, tmp_path):
    """Listed, medium and dense classes at 63 and 64 row words: ranks of every size, random and edge-shaped regions."""
    vs = VariantStore.synthetic(device=0, num_samples=n, sample_coordinates=True, seed=SPREAD_SEED[n], **SPREAD_KW)
    info = vs.info()
    assert info.num_samples - 1 == n and info.use_bit_vector and (info.num_samples + 63) // 64 == (63 if n == 4031 else 64)
    plain = str(tmp_path / "plain.bin")
    vs.export_plain(plain)
    orc = Memo(Oracle(plain))
    regions = _sc_regions(np.random.default_rng(n), info.ref_length)
    names = [vs.sample_name(i) for i in edge_ids(n)] + ["ref"]
    assert names[:-1] == [sample_name(i) for i in edge_ids(n)]
    _walks(vs, orc, regions, names, list(FORMS), len(regions))
    vs.close()
