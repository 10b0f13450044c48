"""Explicit-id cohorts with LONG carrier lists.  The constructor picks explicit sample ids when the carrier density of the first 99
records is at most 0.05; every other explicit-id cohort of the suite is somatic-like, with lists of about 9.  A VCF that opens with
100 rare records and goes on with common ones opens in explicit-id mode too (helpers.write_saturated_cohort, sparse_head=100), and
then the explicit branch of expand_task (lane per group over car_sid, the unaligned nibble window, 16-bit and 32-bit carrier
words), BitRow::holds_explicit and the explicit branch of sample_entry_rec (eight records per round trip, the `m > k` masks) and
both forms of the per-sample rows run on lists hundreds of groups long.

Cohorts: 63, 300 and 4031 samples (16-bit carrier words; 4031: id 4031 is the top of 13 bits) and 4159 (32-bit words); at 300 and
4159 with the coarse per-sample rows and with the exact ones (VS_T4_EXACT_ROWS).  Type 6 against vcf_truth.TextOracle (the VCF text
alone) through every form of the expansion; types 4, 2, 3 and 5 against the oracle for the 1st, 8th, 9th and last carrier of a dense
row and for a sample that does not carry it.  The column queries on these cohorts are the `explicit` cells of
tests/test_gpu_saturated_columns.py; tests/test_dense_explicit_host.py holds TextOracle to the oracle here and asserts the inputs'
conditions on the CPU."""
import numpy as np
import pytest

import vcf_truth as vt
from helpers import SAT_REF_LEN
from test_dense_explicit_host import SPARSE_HEAD, explicit_preconditions, explicit_walk_cases, open_cohort, sample_name
from test_gpu_parity import _compare_t4, _compare_t6
from test_gpu_walks_row_width_edges import _walks

pytestmark = pytest.mark.gpu

CASES = [(63, False), (300, False), (300, True), (4031, False), (4159, False), (4159, True)]


@pytest.mark.parametrize("n,exact", CASES, ids=lambda v: {True: "exact", False: "coarse"}.get(v, str(v)))
def test_type6_and_the_walks_on_long_explicit_lists(n, exact, tmp_path, monkeypatch):
    if exact:
        monkeypatch.setenv("VS_T4_EXACT_ROWS", "1")
    else:
        monkeypatch.delenv("VS_T4_EXACT_ROWS", raising=False)
    vs, orc, names, recs, (_fasta, vcf, plain) = open_cohort(tmp_path, n, 0, rows=150, sparse_head=SPARSE_HEAD)
    info = vs.info()
    assert not info.use_bit_vector and info.num_samples == n + 1
    exact_bytes = info.num_samples * ((info.ref_path_nodes + 63) // 64 + 1 + (info.num_vertices + 63) // 64 + 1) * 8
    assert (info.t4_rows_bytes == exact_bytes) == exact, (info.t4_rows_bytes, exact_bytes)
    car = explicit_preconditions(n, recs, plain)
    tx = vt.TextOracle(vcf)
    edges = tx.midpoints(SAT_REF_LEN)

    # ---- type 6 against the VCF text, through every form of the expansion
    rng = np.random.default_rng(n)
    starts = np.sort(rng.integers(0, 150, size=70))
    regions = sorted([(edges[i], edges[min(150, i + int(rng.integers(1, 4)))]) for i in starts] + [(1, SAT_REF_LEN + 1), (edges[3], edges[3])])
    assert _compare_t6(vs, tx, regions) == len(regions)                                    # shared rows and lists
    assert _compare_t6(vs, tx, [regions[i] for i in rng.permutation(len(regions))]) == len(regions)
    vs.set_option("share_lists", 0)
    try:
        assert _compare_t6(vs, tx, regions) == len(regions)                                # private rows
    finally:
        vs.set_option("share_lists", 1)
    vs.set_option("latency_server", 0)                                                      # one launch per small batch
    try:
        assert _compare_t6(vs, tx, regions[:3]) == 3
        assert _compare_t6(vs, tx, regions[-20:]) == 20                                    # (the last 20: dense rows; [:3] holds the whole reference)
    finally:
        vs.set_option("latency_server", 1)
    plain_res = vs.get_var_in_ref(regions)
    digest, totals = plain_res.digest(), plain_res.totals()
    plain_res.close()
    vs.set_option("resident_lists", 1)
    try:
        res = vs.get_var_in_ref(regions)
        assert res.layout()[2] == 0 and (res.digest(), res.totals()) == (digest, totals), "resident carrier lists change the answers"
        res.close()
        assert _compare_t6(vs, tx, regions) == len(regions)
    finally:
        vs.set_option("resident_lists", 0)

    # ---- the walks: samples by their place in a dense row's carrier list, read from the type-6 answer checked above
    k0, walk_regions_, want_sids, outsider = explicit_walk_cases(car, edges)
    res = vs.get_var_in_ref([(edges[k0], edges[k0 + 1])])
    assert res.region_text(0) == tx.get_var_in_ref(edges[k0], edges[k0 + 1])[2]
    view = res.view(with_carriers=True)
    assert view["pos"].shape[0] == 1 and int(view["car_count"][0]) == int(car[k0].sum()) >= 0.7 * n
    b = int(view["car_begin"][0])
    ids = (view["carriers"][b:b + int(view["car_count"][0])] & 0x1FFFFFFF).astype(np.int64)
    res.close()
    sids = [int(ids[0]), int(ids[7]), int(ids[8]), int(ids[-1])]
    assert sids == want_sids and outsider not in set(ids.tolist())
    assert int(car[100:, np.array(sids) - 1].sum()) > 100                                   # they carry most dense rows
    for sid in sids + [outsider]:
        name = sample_name(sid)
        assert vs.sample_name(sid) == name
        for walk in (2, 1, 0):
            vs.set_option("t4_walk", walk)
            try:
                assert _compare_t4(vs, orc, walk_regions_, name) == len(walk_regions_), (sid, walk)
            finally:
                vs.set_option("t4_walk", 2)
    _walks(vs, orc, walk_regions_, [sample_name(i) for i in sids + [outsider]], ["cooperative", "one_lane", "fallbacks"],
           len(walk_regions_) // 10)
    vs.close()
