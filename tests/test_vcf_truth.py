"""Constructor evidence that does not pass through the product: expected type-6 rows and type-2 sequences are derived
in Python from the VCF / FASTA TEXT (tests/vcf_truth.py) and compared with

  * the CPU oracle reading the graph the product's constructor built   (this file's CPU tests), and
  * the HIP path on the same cohorts                                    (the -m gpu tests below).

A constructor fault on an isolated SNP / MNP / insertion / deletion -- wrong vertex, wrong carrier set, wrong genotype
bits, wrong sequence offsets -- is invisible to oracle-vs-GPU parity (both read the same graph) and visible here."""
import os
import random

import pytest

import vcf_truth as vt
from helpers import SAT_REF_LEN, write_random_cohort, write_saturated_cohort
from oracle.oracle import Oracle
from variantstore_amd import VariantStore

COHORTS = [
    (200, dict(n_samples=5, p_near=0.0, carrier_p=0.3)),
    (201, dict(n_samples=40, p_near=0.3, carrier_p=0.3)),
    (202, dict(n_samples=70, p_near=0.0, carrier_p=0.02)),      # class rows wider than one word
    (203, dict(n_samples=130, p_near=0.3, carrier_p=0.02)),
    (204, dict(n_samples=130, p_near=0.0, carrier_p=0.004)),    # sparse: explicit sample ids
]


def _cohort(tmp_path, seed, kw):
    fasta, vcf, _ = write_random_cohort(str(tmp_path), seed, ref_len=6000, n_rows=150, p_multi=0.05, p_mnp=0.08,
                                        unphased_p=0.2, missing_p=0.05, haploid_p=0.03, **kw)
    _name, ref = vt.read_fasta(fasta)
    names, recs = vt.read_vcf(vcf)
    assert names == sorted(names)          # (sample ids then follow the columns: no name-order permutation in play)
    return fasta, vcf, ref, names, recs


def _sequence_cases(ref, names, recs, seed, n=250):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        x = rng.randint(1, len(ref) - 50)
        y = min(len(ref), x + rng.randint(1, 300))
        smp = rng.choice(names)
        want = vt.sample_sequence(ref, names, recs, smp, x, y)
        if want is not None:
            out.append((x, y, smp, want))
    return out


def test_x_vcf_rows_follow_from_the_vcf_text(golden_dir, survey_vectors, tmp_path):
    """The reference's own data set: all 75 records of x.vcf are simple and their rows follow from the VCF lines; the
    count and the fragments the reference publishes (G2, README) are a subset of that."""
    fasta, vcf = os.path.join(golden_dir, "x.fa"), os.path.join(golden_dir, "x.vcf")
    _n, ref = vt.read_fasta(fasta)
    names, recs = vt.read_vcf(vcf)
    want = "Pos\tRef\tAlt\tSamples\n" + "".join(t for _i, t in vt.expected_type6_rows(names, recs, only=range(len(recs))))
    assert want.count("\n") == 76
    g2 = survey_vectors["G2"]
    assert want.split("\n")[-2] == g2["last_row"] and all(any(l.startswith(f) for l in want.split("\n")) for f in g2["contains"])
    vs = VariantStore.from_vcf(fasta, vcf, device=-1)
    plain = os.path.join(tmp_path, "x.plain")
    vs.export_plain(plain)
    orc = Oracle(plain)
    assert orc.get_var_in_ref(1, len(ref) + 1)[2] == want
    g1 = survey_vectors["G1"]
    in_g1 = [t for _i, t in vt.expected_type6_rows(names, recs, only=range(len(recs))) if g1["region"][0] <= int(t.split("\t")[0]) < g1["region"][1]]
    assert "Pos\tRef\tAlt\tSamples\n" + "".join(in_g1) == g1["text"]      # the reference's published 8 rows, from the VCF alone


@pytest.mark.parametrize("seed,kw", COHORTS)
def test_oracle_on_the_constructed_graph_matches_the_vcf_text(seed, kw, tmp_path):
    fasta, vcf, ref, names, recs = _cohort(tmp_path, seed, kw)
    vs = VariantStore.from_vcf(fasta, vcf, device=-1)
    plain = os.path.join(tmp_path, "c.plain")
    vs.export_plain(plain)
    orc = Oracle(plain)
    rows = set(orc.get_var_in_ref(1, len(ref) + 1)[2].split("\n")[1:-1])
    exp = vt.expected_type6_rows(names, recs)
    assert len(exp) > 40
    for i, text in exp:
        assert text[:-1] in rows, (i, recs[i][:3], text)
        pos = int(text.split("\t")[0])       # and a small region around the row reports it
        assert text in orc.get_var_in_ref(max(1, pos - 3), pos + 4)[2]
    cases = _sequence_cases(ref, names, recs, seed)
    assert len(cases) > 30
    for x, y, smp, want in cases:
        assert orc.query_sample_from_ref(x, y, smp)[1] == want, (x, y, smp)
    if seed == 204:
        assert vs.info().use_bit_vector == 0


def _text_oracle_regions(tx, seed):
    """About 80 regions whose ends are midpoints between records: random spans of 1 .. 12 gaps, the whole reference, a region
    between two neighbouring records, one before the first record, one behind the last, empty ones."""
    edges = tx.midpoints(SAT_REF_LEN)
    rng = random.Random(seed)
    out = [(1, SAT_REF_LEN + 1), (edges[10], edges[11]), (1, edges[0]), (edges[-2] + 40, SAT_REF_LEN + 1), (edges[5], edges[5]),
           (edges[7] - 3, edges[7] + 3)]
    while len(out) < 80:
        a = rng.randrange(len(edges) - 1)
        out.append((edges[a], edges[min(len(edges) - 1, a + rng.randint(1, 12))]))
    return out


@pytest.mark.parametrize("n_samples", [63, 64, 200])
def test_text_oracle_equals_the_oracle_on_a_saturated_cohort(n_samples, tmp_path):
    """TextOracle (the VCF text alone) and Oracle (the graph the constructor built) return equal (n, early_out, text) on every
    region the text answers; a region that ends inside a record's span is refused.  When a GPU test against TextOracle fails,
    this test says which side is wrong."""
    fasta, vcf = write_saturated_cohort(str(tmp_path), n_samples, 4400 + n_samples, two_alt=False, extremes=True)
    tx = vt.TextOracle(vcf)
    assert len(tx.rows) == len(tx.recs) == 150
    ns = n_samples
    assert tx.rows[1].count("(1/1) ") == ns and tx.rows[2].count("(1|1) ") == ns and tx.rows[3].count("(0|1) ") == ns
    assert tx.rows[4].count("(1/0) ") == ns and tx.rows[5].count(") ") == ns - 1 and tx.rows[6].count(") ") == ns - 1
    assert "S00001(" not in tx.rows[5] and f"S{ns:05d}(" not in tx.rows[6] and f"S{ns:05d}(" in tx.rows[5]
    vs = VariantStore.from_vcf(fasta, vcf, device=-1)
    plain = os.path.join(tmp_path, "sat.plain")
    vs.export_plain(plain)
    orc = Oracle(plain)
    regions = _text_oracle_regions(tx, n_samples)
    seen = set()
    for x, y in regions:
        want = orc.get_var_in_ref(x, y)
        assert tx.get_var_in_ref(x, y) == want, (x, y)
        seen.add((want[0] > 0, want[1]))
    assert seen == {(True, False), (False, True)}     # regions with rows and early-outs, and nothing else
    assert tx.get_var_in_ref(1, SAT_REF_LEN + 1)[0] == 150
    pos, ref = tx.recs[20][0], tx.recs[20][1]
    for bad in (pos, pos + len(ref), pos - 1 - 7, pos + len(ref) + 7):
        with pytest.raises(ValueError):
            tx.get_var_in_ref(1, bad)
        with pytest.raises(ValueError):
            tx.get_var_in_ref(bad, SAT_REF_LEN + 1)
    tx.get_var_in_ref(1, pos - 1 - 8)                  # the nearest ends that are answered
    tx.get_var_in_ref(pos + len(ref) + 8, SAT_REF_LEN + 1)
    vs.close()


def test_saturated_writer_options_leave_the_other_rows_alone(tmp_path):
    """two_alt and extremes draw no random number: every line they do not rewrite is the default's, byte for byte."""
    lines = {}
    for key, kw in (("default", {}), ("snp", dict(two_alt=False)), ("both", dict(two_alt=False, extremes=True)), ("ext", dict(extremes=True))):
        d = os.path.join(tmp_path, key)
        os.makedirs(d)
        _fa, vcf = write_saturated_cohort(d, 64, 4464, **kw)
        with open(vcf) as f:
            lines[key] = f.read().split("\n")
    multi = [i for i, l in enumerate(lines["default"]) if not l.startswith("#") and l and "," in l.split("\t")[4]]
    assert multi and not any("," in l.split("\t")[4] for l in lines["snp"] if l and not l.startswith("#"))
    first = next(i for i, l in enumerate(lines["default"]) if l.startswith("c1"))
    extreme = set(range(first + 1, first + 7))
    for i, l in enumerate(lines["default"]):
        if i not in multi:
            assert lines["snp"][i] == l
        if i not in extreme:
            assert lines["ext"][i] == l and lines["both"][i] == lines["snp"][i]
    short = os.path.join(tmp_path, "short")
    os.makedirs(short)
    with open(write_saturated_cohort(short, 64, 4464, rows=12)[1]) as f:
        assert f.read().split("\n")[:-1] == lines["default"][:first + 12]


@pytest.mark.gpu
def test_gpu_x_vcf_rows_follow_from_the_vcf_text(golden_dir):
    fasta, vcf = os.path.join(golden_dir, "x.fa"), os.path.join(golden_dir, "x.vcf")
    _n, ref = vt.read_fasta(fasta)
    names, recs = vt.read_vcf(vcf)
    want = "Pos\tRef\tAlt\tSamples\n" + "".join(t for _i, t in vt.expected_type6_rows(names, recs, only=range(len(recs))))
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    res = vs.get_var_in_ref([(1, len(ref) + 1), (10, 105)])
    assert res.region_text(0) == want                       # all 75 rows of G2, row by row, from the VCF text
    assert res.region_text(1).count("\n") == 9              # README: 8 variants for 10:105
    # the sample's whole sequence (type 2) is the reference with its alleles applied
    cases = _sequence_cases(ref, names, recs, 5, n=300)
    assert len(cases) > 25
    rs = vs.query_sample_seq([(x, y) for x, y, _s, _w in cases], [s for _x, _y, s, _w in cases])
    flags, seqs = rs.sequences()
    assert [s for s in seqs] == [w for _x, _y, _s, w in cases] and not flags.any()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,kw", COHORTS)
def test_gpu_matches_the_vcf_text(seed, kw, tmp_path):
    fasta, vcf, ref, names, recs = _cohort(tmp_path, seed, kw)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    exp = vt.expected_type6_rows(names, recs)
    regions = [(1, len(ref) + 1)] + [(max(1, int(t.split("\t")[0]) - 3), int(t.split("\t")[0]) + 4) for _i, t in exp]
    res = vs.get_var_in_ref(regions)
    rows = set(res.region_text(0).split("\n")[1:-1])
    for k, (i, text) in enumerate(exp):
        assert text[:-1] in rows, (i, recs[i][:3])
        assert text in res.region_text(k + 1)
    # type 4: a carrier's rows include the record's row (substitutions: type 4 reports indels by its own rule, query.h:682-698);
    # type 2: its sequence is the reference with its alleles applied
    rng = random.Random(seed)
    subs = [(i, t) for i, t in exp if len(recs[i][1]) == len(recs[i][2][0])]
    for i, text in rng.sample(subs, 25):
        carrier = text.split("\t")[3].split("(")[0]
        pos = int(text.split("\t")[0])
        r4 = vs.get_sample_var_in_ref([(max(1, pos - 3), pos + 4)], carrier)
        assert text in r4.region_text(0), (i, carrier)
    cases = _sequence_cases(ref, names, recs, seed)
    rs = vs.query_sample_seq([(x, y) for x, y, _s, _w in cases], [s for _x, _y, s, _w in cases])
    flags, seqs = rs.sequences()
    assert seqs == [w for _x, _y, _s, w in cases] and not flags.any()
