"""The CPU side of tests/test_gpu_walks_row_width_edges.py and tests/test_gpu_dense_explicit.py: the cohorts those files open, their
regions and samples, and every condition on the INPUTS that makes a pass on the GPU prove something -- checked here from the VCF
text and the oracle alone, so that a seed that misses a condition shows up in the CPU suite and not on the GPU.

  helpers.write_saturated_cohort(sparse_head=H)  draws nothing from the writer's generator: H = 0 is the default's bytes, and the
      records from H on are the unthinned file's.  The first 100 records thinned to n // 50 carriers make the constructor choose
      EXPLICIT sample ids (it looks at the first 99 records) for a cohort whose later records are carried by 70 - 100 % of the
      samples: carrier lists as long as the cohort, where every other explicit-id cohort of the suite has lists of about 9.
  dense explicit-id cohorts (63, 300, 4031, 4159 samples)  open with use_bit_vector == 0, and vcf_truth.TextOracle equals the oracle
      on the whole reference and on every region of three records.
  saturated class-row cohorts at the row-width edges (wpc 1, 2, 63, 64, 64, 65) and on both sides of the class_cum switch
      (info().num_samples 65,535: the 16-bit prefix table; 65,536: the word loop)  the walking queries' regions are mostly
      unflagged, mostly predicted from the text, and every edge sample's type-5 answers differ from its id neighbours' -- a rank
      that is off by one in sample_entry_rec cannot hide."""
import os

import numpy as np
import pytest

import vcf_truth as vt
from helpers import SAT_REF_LEN, read_plain, write_saturated_cohort
from oracle.oracle import Oracle
from variantstore_amd import VariantStore

SAT_WIDTHS = (63, 64, 4031, 4032, 4095, 4159)           # wpc 1, 2, 63, 64, 64, 65
SWITCH_SEED = {65534: 4400 + 65534, 65535: 4400 + 65535}   # samples -> seed, around the class_cum switch (40 rows)
EXPLICIT_WIDTHS = (63, 300, 4031, 4159)                 # 16-bit carrier words up to info().num_samples == 4032, 32-bit above
SPARSE_HEAD = 100


class Memo:
    """Any oracle with every answer kept (the GPU files run the same regions through several kernel forms); `calls` counts the
    answers that were computed."""

    def __init__(self, orc):
        self._orc, self._kept, self.calls = orc, {}, 0

    def __getattr__(self, name):
        fn = getattr(self._orc, name)

        def call(*args):
            if (name,) + args not in self._kept:
                self._kept[(name,) + args] = fn(*args)
                self.calls += 1
            return self._kept[(name,) + args]
        return call


def sample_name(sid):
    return "ref" if sid == 0 else f"S{sid:05d}"


def seed_of(n):
    return SWITCH_SEED.get(n, 4400 + n)


def edge_ids(n):
    """The ids at the row words' edges: 1, 63 and 64, the first id of the last row word, n (at the 65k cohorts: 1, 65,472, n)."""
    last_word = ((n + 1 + 63) // 64 - 1) * 64
    ids = {1, last_word, n} if n > 65000 else {1, 63, 64, last_word, n}
    return sorted(i for i in ids if 1 <= i <= n)


def walk_regions(edges):
    """[edges[i], edges[i + 5]) for every fourth i: five records each, neighbours overlap in one (38 regions of 150 rows, 10 of 40)."""
    rows = len(edges) - 1
    return [(edges[i], edges[min(i + 5, rows)]) for i in range(0, rows, 4)]


def open_cohort(tmp, n, device, **kw):
    """(store, oracle over its plain dump, names, records, plain path) of write_saturated_cohort(n, seed_of(n), two_alt=False, **kw)."""
    fasta, vcf = write_saturated_cohort(str(tmp), n, seed_of(n), two_alt=False, **kw)
    vs = VariantStore.from_vcf(fasta, vcf, device=device)
    plain = os.path.join(tmp, "plain.bin")
    vs.export_plain(plain)
    names, recs = vt.read_vcf(vcf)
    assert names == [sample_name(i) for i in range(1, n + 1)]
    return vs, Memo(Oracle(plain)), names, recs, (fasta, vcf, plain)


def flagged(code):
    """The oracle's codes for an input the reference does not answer: -1 it never returns, -3 it throws."""
    return code in (-1, -3)


def neighbour_differences(orc, regions, n, sid, enough=None):
    """{neighbour id: on how many regions the oracle's type-5 answer for `sid` differs from the neighbour's} for sid - 1 and
    sid + 1 where they are samples; counting stops at `enough`."""
    out = {}
    for other in (sid - 1, sid + 1):
        if not 1 <= other <= n:
            continue
        out[other] = 0
        for x, y in regions:
            out[other] += orc.get_sample_var_in_sample(x, y, sample_name(sid)) != orc.get_sample_var_in_sample(x, y, sample_name(other))
            if enough is not None and out[other] >= enough:
                break
    return out


def predicted_sequences(fasta, names, recs, regions, sid):
    """{region index: the sample's sequence worked out from the VCF and FASTA text} where vcf_truth.sample_sequence predicts."""
    _name, ref = vt.read_fasta(fasta)
    out = {}
    for q, (x, y) in enumerate(regions):
        want = vt.sample_sequence(ref, names, recs, sample_name(sid), x, y)
        if want is not None:
            out[q] = want
    return out


def fully_carried_lines(text, n):
    """The lines of a print_var text whose carrier list names all n samples."""
    return [line for line in text.split("\n")[1:] if line and line.split("\t")[3].count("(") == n]


def carriers_of(recs):
    """[records x samples] bool from the VCF text."""
    return np.array([[g not in ("0|0", "0/0") for g in r[3]] for r in recs])


def explicit_preconditions(n, recs, plain):
    """What a dense explicit-id cohort must hold, from the VCF text and the plain dump.  Returns the carrier matrix."""
    car = carriers_of(recs)
    cnt = car.sum(axis=1)
    assert cnt[:SPARSE_HEAD].max() <= max(1, n // 50) and cnt[:SPARSE_HEAD].min() >= 1
    for k in range(SPARSE_HEAD, len(recs)):
        assert cnt[k] >= 0.7 * n or (k % 16 == 4 and not car[k, 2015:].any() and cnt[k] >= 1500), (k, int(cnt[k]))
    assert cnt[144] == n
    tail = cnt[SPARSE_HEAD:]
    assert (tail % 8 == 0).any() and (tail % 8 != 0).any(), "list lengths: both a multiple of 8 and not"
    g = read_plain(plain)
    assert g["use_bit_vector"] == 0 and g["car_sid"].shape[0] == g["car_begin"][-1]
    lens = np.diff(g["car_begin"].astype(np.int64))
    dense = np.nonzero(lens >= min(0.7 * n, 1500))[0]
    assert sorted(lens[dense].tolist()) == sorted(tail.tolist()), "the dense vertices are the records from 100 on"
    assert (g["car_begin"][dense] % 8 != 0).any(), "no dense row starts at a pool offset that is not a multiple of 8"
    if n == 4031:
        assert any((g["car_sid"][int(g["car_begin"][v]):int(g["car_begin"][v + 1])] == 4031).any() for v in dense), "id 4031: the top of 13 bits"
    return car


def explicit_walk_cases(car, edges):
    """(k0, regions, [ids], outsider) for the walks on a dense explicit-id cohort: k0 is the first dense record that somebody does not
    carry, the ids are its 1st, 8th, 9th (the second round trip of holds_explicit and of sample_entry_rec's explicit branch) and
    last carrier in id order, the outsider is the first sample that does not carry it; the regions are walk_regions plus four
    regions of one dense record each, k0's among them (there the outsider carries none of the region's dense rows)."""
    n = car.shape[1]
    k0 = next(k for k in range(SPARSE_HEAD, car.shape[0]) if k % 16 != 4 and car[k].sum() < n)
    ids = np.nonzero(car[k0])[0] + 1
    outsider = int(np.nonzero(~car[k0])[0][0]) + 1
    regions = walk_regions(edges) + [(edges[k], edges[k + 1]) for k in (k0, 116, 132, 144)]
    return k0, regions, [int(ids[0]), int(ids[7]), int(ids[8]), int(ids[-1])], outsider


# ------------------------------------------------------------------------------------ A: the writer's option
def test_sparse_head_draws_nothing_from_the_writers_generator(tmp_path):
    """sparse_head=0 and no option: identical files.  sparse_head=100: the records from 100 on are the unthinned file's bytes, the
    first 100 keep at most n // 50 carriers, each with the call it had; extremes=True with sparse_head > 6 is refused."""
    text = {}
    for key, kw in (("none", {}), ("zero", dict(sparse_head=0)), ("head", dict(sparse_head=SPARSE_HEAD)),
                    ("snp", dict(two_alt=False)), ("snp_head", dict(two_alt=False, sparse_head=SPARSE_HEAD))):
        d = os.path.join(tmp_path, key)
        os.makedirs(d)
        fasta, vcf = write_saturated_cohort(d, 300, 4700, **kw)
        with open(vcf) as f, open(fasta) as g:
            text[key] = (f.read().split("\n"), g.read())
    assert text["none"] == text["zero"]
    first = next(i for i, l in enumerate(text["none"][0]) if l.startswith("c1"))
    for plain, thinned in (("none", "head"), ("snp", "snp_head")):
        a, b = text[plain], text[thinned]
        assert a[1] == b[1] and len(a[0]) == len(b[0]) and a[0][:first] == b[0][:first]
        assert a[0][first + SPARSE_HEAD:] == b[0][first + SPARSE_HEAD:]
        for la, lb in zip(a[0][first:first + SPARSE_HEAD], b[0][first:first + SPARSE_HEAD]):
            ta, tb = la.split("\t"), lb.split("\t")
            assert ta[:9] == tb[:9]
            kept = [(x, y) for x, y in zip(ta[9:], tb[9:]) if y != "0|0"]
            assert 1 <= len(kept) <= 300 // 50
            assert all(x == y for x, y in kept) or (len(kept) == 1 and kept[0][1] in ("0|1", "0|2"))
    with pytest.raises(AssertionError):
        write_saturated_cohort(str(tmp_path), 64, 1, extremes=True, sparse_head=7)


# ------------------------------------------------------------------------------------ D: dense explicit-id cohorts
@pytest.mark.parametrize("n", EXPLICIT_WIDTHS)
def test_a_sparse_head_opens_explicit_ids_and_the_text_equals_the_oracle(n, tmp_path):
    vs, orc, names, recs, (_fasta, vcf, plain) = open_cohort(tmp_path, n, -1, rows=150, sparse_head=SPARSE_HEAD)
    info = vs.info()
    assert info.use_bit_vector == 0 and info.num_samples == n + 1
    tx = vt.TextOracle(vcf)
    assert len(tx.rows) == 150
    edges = tx.midpoints(SAT_REF_LEN)
    assert edges == vt.gap_midpoints(recs, SAT_REF_LEN)
    for x, y in [(1, SAT_REF_LEN + 1)] + [(edges[i], edges[i + 3]) for i in range(len(edges) - 3)]:
        assert tx.get_var_in_ref(x, y) == orc.get_var_in_ref(x, y), (x, y)
    car = explicit_preconditions(n, recs, plain)
    # the samples the GPU file picks by their place in a dense row's list exist: every dense row has more than nine carriers, and
    # some region of one dense record has a sample that does not carry it
    assert car[SPARSE_HEAD:].sum(axis=1).min() > 9 and not car[SPARSE_HEAD:].all(axis=1).all()
    # the walks: the samples picked by their place in a dense list are distinct, the list's order is the ids', the oracle flags few of
    # their regions, and where it answers type 4 the outsider reports nothing of record k0
    k0, regions, sids, outsider = explicit_walk_cases(car, edges)
    assert len(set(sids + [outsider])) == 5 and len(regions) == 42
    g = read_plain(plain)
    lists = [g["car_sid"][int(a):int(b)] for a, b in zip(g["car_begin"][:-1], g["car_begin"][1:]) if b - a == car[k0].sum()]
    assert any(np.array_equal(l, np.nonzero(car[k0])[0] + 1) for l in lists), "record k0's carrier records are not in id order"
    for sid in sids + [outsider]:
        for call in (orc.query_sample_from_ref, orc.query_sample_from_sample, orc.get_sample_var_in_sample):
            assert sum(flagged(call(x, y, sample_name(sid))[0]) for x, y in regions) <= len(regions) // 10, (sid, call)
        assert all(orc.get_sample_var_in_ref(x, y, sample_name(sid))[0] >= 0 for x, y in regions)
    assert orc.get_sample_var_in_ref(edges[k0], edges[k0 + 1], sample_name(outsider))[0] == 0
    assert orc.get_sample_var_in_ref(edges[k0], edges[k0 + 1], sample_name(sids[2]))[0] == 1
    vs.close()


# ------------------------------------------------------------------------------------ C: the walks at the row-width edges
@pytest.mark.parametrize("n", SAT_WIDTHS)
def test_walk_preconditions_at_the_row_width_edges(n, tmp_path):
    """38 regions; for every edge sample at most a tenth flagged (per query type), at least half predicted from the text (type 2),
    and type-5 answers that differ from both id neighbours' on at least half of the regions."""
    vs, orc, names, recs, (fasta, _vcf, _plain) = open_cohort(tmp_path, n, -1, rows=150, extremes=True)
    info = vs.info()
    assert info.use_bit_vector and info.num_samples == n + 1
    regions = walk_regions(vt.gap_midpoints(recs, SAT_REF_LEN))
    assert len(regions) == 38
    for sid in [0] + edge_ids(n):
        for call in (orc.query_sample_from_ref, orc.query_sample_from_sample, orc.get_sample_var_in_sample):
            assert sum(flagged(call(x, y, sample_name(sid))[0]) for x, y in regions) <= len(regions) // 10, (sid, call)
        if sid:
            want = predicted_sequences(fasta, names, recs, regions, sid)
            assert len(want) >= len(regions) // 2, (sid, len(want))
            for q, seq in want.items():
                assert orc.query_sample_from_ref(*regions[q], sample_name(sid)) == (len(seq), seq), (sid, q)
            diff = neighbour_differences(orc, regions, n, sid)
            assert diff and min(diff.values()) >= len(regions) // 2, (sid, diff)
    vs.close()


@pytest.mark.parametrize("n", sorted(SWITCH_SEED))
def test_walk_preconditions_around_the_class_cum_switch(n, tmp_path):
    """40 rows, 10 regions: info().num_samples is 65,535 / 65,536; ids 1, 65,472 and n differ from their id neighbours on at least two
    regions; a row carried by all n samples is among sample n's type-5 reports (a rank above 65,000)."""
    vs, orc, names, recs, _paths = open_cohort(tmp_path, n, -1, rows=40, extremes=True)
    info = vs.info()
    assert info.use_bit_vector and info.num_samples == n + 1 and (info.num_samples + 63) // 64 == 1024
    regions = walk_regions(vt.gap_midpoints(recs, SAT_REF_LEN))
    assert len(regions) == 10 and edge_ids(n) == [1, 65472, n]
    for sid in edge_ids(n):
        diff = neighbour_differences(orc, regions, n, sid, enough=2)
        assert diff and min(diff.values()) >= 2, (sid, diff)
    texts = [orc.get_sample_var_in_sample(x, y, sample_name(n)) for x, y in regions]
    assert sum(flagged(c) for c, _t in texts) <= 1
    assert any(fully_carried_lines(t, n) for c, t in texts if c >= 0), "no row carried by everybody in sample n's answers"
    vs.close()
