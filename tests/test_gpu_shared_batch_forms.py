"""The forms of a shared batch (more than 64 regions: shared rows and carrier lists, and every count, burden and genotype-matrix
batch) give one answer: the default form -- enqueued, the plan on a stream of its own, speculative sizes -- against the synchronous
finish (async_submit = 0), the expansion on a second stream (async_fill), resident carrier lists and a handle that never
speculates.  Three batches: sorted, the same regions shuffled (the device sorts them) and one just above the 64-region boundary;
then the sorted one again, on a handle that by now sorts first.  Every form runs on a handle of its own over the same synthetic
index (the size smoke() uses), so that each meets the three ways of planning -- as given, sorted after the plan's verdict, sorted
first -- from the same start.  Comparisons are within a batch only: a shuffled batch may place its rows elsewhere in the table
than its sorted twin."""
import os

import numpy as np
import pytest

from oracle.oracle import Oracle
from variantstore_amd import VariantStore

pytestmark = pytest.mark.gpu

KW = dict(ref_length=200_000, num_variants=4000, num_samples=40, seed=7, first_pos=100, frac_ins=0.08, frac_del=0.08,
          frac_multi=0.05, max_indel=4, af_exponent=2.0)
SUBSET = [1, 5, 7, 33]
WINDOW = (1, 4)
DEFAULT = {"async_submit": 1, "async_fill": 0, "resident_lists": 0, "t6_speculate": 1}
FORMS = [{"async_submit": 0}, {"async_fill": 1}, {"async_fill": 1, "async_submit": 0}, {"resident_lists": 1},
         {"resident_lists": 1, "async_submit": 0}, {"t6_speculate": 0}]
ROW_FIELDS = ("pos", "ref_off", "ref_len", "alt_off", "alt_len", "count_flags")   # (a count batch has no arena: car_begin is not written)


def _batches():
    rng = np.random.default_rng(3)
    rng.integers(1, 199_000, size=64)   # (the draws smoke() makes in front of its sorted batch)
    [rng.integers(1, 3000) for _ in range(64)]
    srt = sorted((int(s), int(s) + 2500) for s in rng.integers(1, 197_000, size=300))
    shuffled = [srt[i] for i in np.random.default_rng(17).permutation(len(srt))]
    assert shuffled != srt
    return {"sorted": srt, "small": srt[100:170], "shuffled": shuffled, "sorted_again": srt}


BATCHES = _batches()


def _store():
    return VariantStore.synthetic(device=0, **KW)


def _flat(prefix, arrays):
    """The arrays of a count, burden or matrix result under one name each; of the table's rows the fields a count batch writes."""
    out = {}
    for k, v in arrays.items():
        if k == "rows":
            for f in ROW_FIELDS:
                out[f"{prefix}.rows.{f}"] = np.ascontiguousarray(v[f])
        else:
            out[f"{prefix}.{k}"] = np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v
    return out


def _type6(vs, regions, resident):
    res = vs.get_var_in_ref(regions)
    out = {"totals": res.totals(), "digest": res.digest(), "shared": res.layout()[4]}
    if resident:
        assert res.layout()[2] == 0, "a result over resident lists owns no arena"
    else:
        assert res.layout()[2] > 0
        assert res.fill_ms() > 0, "the result's own event pair around the expansion"
        assert vs.last_timing().ms_total > 0
    return out, res


def _columns(vs, regions):
    """Every count, burden and matrix array of a batch: the whole cohort, a subset, and the burden under a window."""
    out = {}
    for name, samples in (("all", None), ("subset", SUBSET)):
        queries = [("counts", lambda: vs.allele_counts(regions, samples), lambda r: r.allele_counts()),
                   ("burden", lambda: vs.sample_burden(regions, samples), lambda r: r.sample_burden()),
                   ("matrix", lambda: vs.genotype_matrix(regions, samples), lambda r: r.genotype_matrix())]
        if samples is None:
            queries.append(("burden_window", lambda: vs.sample_burden(regions, None, *WINDOW), lambda r: r.sample_burden()))
        for kind, query, arrays in queries:
            res = query()
            out.update(_flat(f"{kind}.{name}", arrays(res)))
            out[f"{kind}.{name}.totals"] = res.totals()
            assert res.fill_ms() >= 0, (kind, name)
            res.close()
    return out


def _run(form):
    """Every batch under `form` on a fresh handle: {batch: (type-6 outcome, column arrays)}."""
    vs = _store()
    for k, v in form.items():
        vs.set_option(k, v)
    out = {}
    try:
        for name, regions in BATCHES.items():
            t6, res = _type6(vs, regions, bool(form.get("resident_lists")))
            res.close()
            out[name] = (t6, _columns(vs, regions))
    finally:
        for k in form:
            vs.set_option(k, DEFAULT[k])
    again, res = _type6(vs, BATCHES["sorted"], False)   # the default form is back
    res.close()
    assert again == out["sorted"][0]
    vs.close()
    return out


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    out = _run({})
    for name in BATCHES:
        assert out[name][0]["shared"], name
        assert out[name][1]["matrix.all.cells"].any() and out[name][1]["counts.all.counts"]["carriers"].any(), name
        assert out[name][1]["burden.all.cells"]["variants"].any() and out[name][1]["burden_window.all.cells"]["variants"].any(), name
        assert not np.array_equal(out[name][1]["burden.all.cells"], out[name][1]["burden_window.all.cells"]), name
    # the baseline is itself right: the sorted batch against the oracle, region by region
    vs = _store()
    plain = os.path.join(tmp_path_factory.mktemp("forms"), "plain.bin")
    vs.export_plain(plain)
    orc = Oracle(plain)
    res = vs.get_var_in_ref(BATCHES["sorted"])
    assert res.digest() == out["sorted"][0]["digest"]
    for q, (x, y) in enumerate(BATCHES["sorted"]):
        assert res.region_text(q) == orc.get_var_in_ref(x, y)[2], f"region {q} {x}:{y} differs from the oracle"
    res.close()
    vs.close()
    assert out["sorted"][0] == out["sorted_again"][0]
    assert out["sorted"][0]["totals"] != out["small"][0]["totals"]
    return out


@pytest.mark.parametrize("form", FORMS, ids=lambda f: "-".join(f"{k}={v}" for k, v in f.items()))
def test_form_answers_as_the_default(form, baseline):
    got = _run(form)
    for name in BATCHES:
        t6, cols = got[name]
        want6, want_cols = baseline[name]
        assert t6 == want6, (name, t6, want6)
        assert cols.keys() == want_cols.keys()
        for k, v in cols.items():
            w = want_cols[k]
            if isinstance(v, np.ndarray):
                assert v.dtype == w.dtype and v.shape == w.shape and v.tobytes() == w.tobytes(), (name, k)
            else:
                assert v == w, (name, k)


def _counters(vs):
    info = vs.info()
    return info.t6_speculated, info.t6_refused


def test_speculation_and_interleaving(baseline):
    regions = BATCHES["sorted"]
    want = baseline["sorted"][0]["digest"]

    def run(interleave):
        vs = _store()
        first = vs.get_var_in_ref(regions)
        assert first.digest() == want
        before = _counters(vs)
        if interleave:
            for r in (vs.allele_counts(regions), vs.sample_burden(regions, SUBSET), vs.genotype_matrix(regions),
                      vs.allele_counts(BATCHES["shuffled"], SUBSET), vs.sample_burden(BATCHES["shuffled"], None, *WINDOW),
                      vs.genotype_matrix(BATCHES["shuffled"], SUBSET)):
                r.totals()
                r.close()
            assert _counters(vs) == before
        second = vs.get_var_in_ref(regions)
        assert second.digest() == want
        after = _counters(vs)
        first.close(); second.close()
        vs.close()
        return before, after

    before, after = run(False)
    assert after[0] == before[0] + 1, "the second of two like batches is submitted without waiting for its sizes"
    assert run(True) == (before, after)
