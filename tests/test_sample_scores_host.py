"""Per-sample scores without a GPU (vs_query_sample_scores on a handle opened host-only): the reference helper on the golden VCFs
and on a hand-written text with the scores worked out by hand, the quantisation's corner cases, every argument error the host can
raise with its message where one is promised, VS_ERR_NO_DEVICE for a valid call, the wrapper's mapping form against a stubbed count
result and the CLI's weight-file errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sample_scores_ref as ref
from genotype_matrix_ref import Parsed
from oracle.oracle import Oracle
from variantstore_amd import VariantStore, _lib
from variantstore_amd.api import VariantStoreError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
VS_ERR_NO_DEVICE, VS_ERR_ARG, VS_ERR_UNKNOWN_SAMPLE = -3, -5, -6


@pytest.fixture(scope="module")
def host_store(golden_dir):
    vs = VariantStore.from_vcf(os.path.join(golden_dir, "x.small.fa"), os.path.join(golden_dir, "x.small.vcf"), device=-1)
    yield vs
    vs.close()


def test_reference_on_the_golden_vcfs(golden_dir, tmp_path):
    """x.small.vcf by hand: sample `1` carries 9 G>A as 1|0 (dosage 1) and the deletion printed as `55 C -` as 1|1 (dosage 2);
    x.vcf: 10 C>T 1|1, 14 G>A 1|0.  Weights (0.5, 3) and (-1.25, 0) on the two rows, 0 on every other."""
    for stem, region, hand in (("x.small", (1, 60), {"9\tG\tA": 1, "55\tC\t": 2}), ("x", (1, 20), {"10\tC\tT": 2, "14\tG\tA": 1})):
        vs = VariantStore.from_vcf(os.path.join(golden_dir, stem + ".fa"), os.path.join(golden_dir, stem + ".vcf"), device=-1)
        plain = os.path.join(tmp_path, stem + ".bin")
        vs.export_plain(plain)
        name = vs.sample_name(1)
        vs.close()
        n, _early, text = Oracle(plain).get_var_in_ref(*region)
        assert n >= 0
        p = Parsed([text])
        heads = list(hand)
        w = np.zeros((p.n_rows, 2), np.float32)
        w[p.heads.index(heads[0])] = (0.5, 3)
        w[p.heads.index(heads[1])] = (-1.25, 0)
        s, f = ref.sums(p, [name], w)
        d0, d1 = hand[heads[0]], hand[heads[1]]
        assert f.tolist() == [35, 34]                    # 1.25 = 0.625 x 2^1, 3 = 0.75 x 2^2
        assert s.tolist() == [[int((0.5 * d0 - 1.25 * d1) * 2 ** 35), 3 * d0 * 2 ** 34]]
        assert ref.scores(s, f).tolist() == [[0.5 * d0 - 1.25 * d1, 3.0 * d0]]
        real, carried = ref.fsum(p, [name], w)
        assert real.tolist() == [[0.5 * d0 - 1.25 * d1, 3.0 * d0]] and carried[0] >= 2
        assert ref.pairs(p, [name], w) == 2
        assert not ref.sums(p, ["nobody"], w)[0].any()


TEXTS = ["Pos\tRef\tAlt\tSamples\n"
         "10\tA\tC\tS1(1|1) S2(0/1) S3(1/0) \n"
         "20\tG\tT\tS4(1|0) S1(0|1) \n",
         "Pos\tRef\tAlt\tSamples\n"
         "20\tG\tT\tS4(1|0) S1(0|1) \n"
         "40\tT\tG\tS2(1|1) \n"]


def test_reference_on_a_hand_written_text():
    """Two regions; the row 20 G>T is reported by both, with different weights.  Reports in order: 10 (r0), 20 (r0), 20 (r1), 40 (r1)."""
    cols = ["S1", "S2", "S4", "S5"]                       # S3 is outside the subset, S5 carries nothing
    p = Parsed(TEXTS)
    assert p.n_rows == 4
    w = np.array([[1.0, 0.25], [2.0, 0.0], [-4.0, 0.5], [0.5, -0.125]], np.float32)
    s, f = ref.sums(p, cols, w)
    assert f.tolist() == [33, 36]                          # 4 = 0.5 x 2^3, 0.5 = 0.5 x 2^0
    # S1: 2 x 1 + 1 x 2 + 1 x -4 = 0 | 2 x 0.25 + 0 + 0.5 = 1;  S2: 1 x 1 + 2 x 0.5 = 2 | 0.25 - 0.25 = 0;  S4: 2 - 4 = -2 | 0.5
    assert ref.scores(s, f).tolist() == [[0.0, 1.0], [2.0, 0.0], [-2.0, 0.5], [0.0, 0.0]]
    assert s[:, 0].tolist() == [0, 2 << 33, -(2 << 33), 0] and s[1, 1] == 0 and s[2, 1] == 1 << 35
    real, carried = ref.fsum(p, cols, w)
    assert np.array_equal(real, ref.scores(s, f)) and carried.tolist() == [3, 2, 2, 0]
    assert ref.pairs(p, cols, w) == 7
    assert ref.pairs(p, cols, w * np.float32([[1], [0], [1], [1]])) == 5   # the report without a weight does not count
    # one column of weights, given flat
    assert ref.scores(*ref.sums(p, cols, w[:, 0])).ravel().tolist() == [0.0, 2.0, -2.0, 0.0]


def test_a_dropped_row_shifts_the_report_index():
    """A table of 6 rows, two regions: region 0 owns slots 0 .. 3 of which slot 1 was dropped, region 1 the rows 2 .. 5 (two shared
    with region 0) of which row 4 was dropped.  Reports: rows 0, 2, 3 | 2, 3, 5 -- the third report is slot 3's, not slot 2's."""
    dropped = np.array([0, 1, 0, 0, 1, 0], bool)
    rows, slots = ref.reported_rows([0, 2], [4, 4], dropped)
    assert rows.tolist() == [0, 2, 3, 2, 3, 5] and slots.tolist() == [0, 2, 3, 0, 1, 3]
    in_region = np.concatenate([np.arange(3), np.arange(3)])
    assert (slots != in_region).sum() == 3
    # the weights of the reports land on the table rows: a shared row collects both reports'
    w = np.array([1, 2, 3, 10, 20, 30], np.int64)
    table = np.zeros(6, np.int64)
    np.add.at(table, rows, w)
    assert table.tolist() == [1, 0, 12, 23, 0, 30]


def test_quantisation_cases():
    one = np.float32(1.0)
    # M_k a power of two: 1 = 0.5 x 2^1, f = 35, and the largest weight becomes 2^35 (|q| <= 2^36 holds with room)
    w = np.array([[one, 0, 2.0 ** -36, 2.0 ** -40], [-one, 0, 3 * 2.0 ** -36, -(2.0 ** -40)], [0.5, 0, 5 * 2.0 ** -36, 2.0 ** -38]], np.float32)
    w[:, 2] += np.float32([1, 0, 0])       # column 2: M = 1 + 2^-36 rounds to 1 in float32; ties 0.5, 1.5, 2.5 -> 0, 2, 2
    w[:, 3] += np.float32([0, 0, 1])       # column 3: below 2^-37 M: 2^-40 x 2^35 = 2^-5 -> 0
    f = ref.shifts(w)
    assert f.tolist() == [35, 0, 35, 35]
    q = ref.quantise(w)
    assert q[:, 0].tolist() == [2 ** 35, -(2 ** 35), 2 ** 34]
    assert q[:, 1].tolist() == [0, 0, 0]
    assert q[1:, 2].tolist() == [2, 2] and q[0, 2] == 2 ** 35
    assert q[:2, 3].tolist() == [0, 0] and q[2, 3] == 2 ** 35
    assert ref.quantise(np.float32([2.0 ** -36, 1]))[0, 0] == 0             # the tie 0.5 goes to the even 0
    # just below a power of two: 0.99999994 = m 2^0, f = 36, |q| < 2^36; the smallest subnormal scales without underflow
    assert ref.shifts(np.float32([np.nextafter(one, np.float32(0))])).tolist() == [36]
    tiny = np.float32(2.0 ** -149)
    assert ref.shifts([tiny]).tolist() == [36 + 148] and ref.quantise([tiny]).tolist() == [[2 ** 35]]
    big = np.float32(3.0e38)
    assert ref.shifts([big]).tolist() == [36 - 128] and abs(int(ref.quantise([big])[0, 0])) <= 2 ** 36
    # weights at or above 2^-12 M are exact: a float32 has 24 bits, 36 - 12 = 24
    w = np.float32([1.9999999, 2.0 ** -12 * 1.0000001])
    assert np.array_equal(np.ldexp(ref.quantise(w).astype(np.float64), -ref.shifts(w)[0]).ravel(), w.astype(np.float64))


def _call(vs, n=1, ids=(1,), weights=((0.5,),), n_scores=None, names=None, n_ids=None, null_ids=False, null_weights=False, n_weights=None):
    """vs_query_sample_scores through ctypes: (code, message)."""
    lib = _lib.load()
    regions = (_lib.Region * max(n, 1))(*[_lib.Region(1, 100)] * max(n, 1))
    a = np.ascontiguousarray(ids, dtype=np.uint32)
    w = np.ascontiguousarray(weights, dtype=np.float32)
    pa = None if null_ids else a.ctypes.data_as(C.POINTER(C.c_uint32))
    pw = None if null_weights else C.c_void_p(w.ctypes.data)
    pn = (C.c_char_p * len(names))(*[s.encode() for s in names]) if names is not None else None
    h = C.c_void_p()
    rc = lib.vs_query_sample_scores(vs._h, regions, n, pa, len(a) if n_ids is None else n_ids, pw, w.shape[0] if n_weights is None else n_weights,
                                    w.shape[1] if n_scores is None else n_scores, pn, C.byref(h))
    assert rc != 0 and not h.value
    return rc, lib.vs_last_error().decode()


def test_argument_errors(host_store):
    vs = host_store
    ns = vs.info().num_samples
    assert ns == 2                                                          # x.small: "ref" and one sample, id 1
    assert _call(vs, n=0)[0] == VS_ERR_ARG
    assert _call(vs, null_weights=True)[0] == VS_ERR_ARG
    rc, msg = _call(vs, n_scores=0)
    assert rc == VS_ERR_ARG and "0 scores" in msg
    rc, msg = _call(vs, weights=[[0.0] * 9])
    assert rc == VS_ERR_ARG and "9 scores" in msg
    assert _call(vs, n_ids=0)[0] == VS_ERR_ARG
    assert _call(vs, null_ids=True, n_ids=0)[0] == VS_ERR_ARG
    assert _call(vs, null_ids=True, n_ids=2)[0] == VS_ERR_ARG             # NULL ids: the whole cohort, one sample
    assert _call(vs, ids=(ns + 5,), n_scores=9)[0] == VS_ERR_ARG            # before the unknown sample
    assert _call(vs, ids=(0,))[0] == VS_ERR_UNKNOWN_SAMPLE
    assert _call(vs, ids=(ns,))[0] == VS_ERR_UNKNOWN_SAMPLE
    rc, msg = _call(vs, ids=(1, 1))
    assert rc == VS_ERR_ARG and "sample id 1" in msg and "twice" in msg
    # a weight that is not finite: the message names the column
    for bad in (np.nan, np.inf, -np.inf):
        rc, msg = _call(vs, weights=[[1.0, 2.0, 3.0], [1.0, 2.0, bad]])
        assert rc == VS_ERR_ARG and "column 2" in msg and "not finite" in msg, msg
    rc, msg = _call(vs, null_ids=True, n_ids=1, weights=[[np.nan]])
    assert rc == VS_ERR_ARG and "column 0" in msg
    # 2^26 reports or more: refused from n_weights alone, the weights are not read
    rc, msg = _call(vs, n_weights=1 << 26)
    assert rc == VS_ERR_ARG and "2^26" in msg
    # a name with a tab or a newline
    assert _call(vs, names=["a\tb"])[0] == VS_ERR_ARG
    assert _call(vs, weights=[[1.0, 2.0]], names=["ok", "two\nlines"])[0] == VS_ERR_ARG
    # the options
    for key, bad, ok in (("score_chunk", (-1, 63, 65537), (64, 65536, 0)), ("score_tile_cols", (-16, 8, 24, 65552), (16, 64, 65536, 0))):
        for v in bad:
            with pytest.raises(VariantStoreError) as e:
                vs.set_option(key, v)
            assert e.value.code == VS_ERR_ARG
        for v in ok:
            vs.set_option(key, v)


def test_valid_call_on_a_host_only_handle_has_no_device(host_store):
    vs = host_store
    assert _call(vs)[0] == VS_ERR_NO_DEVICE
    assert _call(vs, null_ids=True, n_ids=1, weights=[[1.0] * 8] * 3, names=[f"s{k}" for k in range(8)])[0] == VS_ERR_NO_DEVICE
    assert _call(vs, null_weights=True, n_weights=0, n_scores=2)[0] == VS_ERR_NO_DEVICE     # no reports announced: no weights needed
    for kw in (dict(), dict(samples=[1]), dict(samples=[vs.sample_name(1)], score_names=["prs"])):
        with pytest.raises(VariantStoreError) as e:
            vs.sample_scores([(1, 100)], [0.25, 0.5], **kw)
        assert e.value.code == VS_ERR_NO_DEVICE
    with pytest.raises(VariantStoreError) as e:
        vs.sample_scores([(1, 100)], [1.0], samples=[1, 1])
    assert e.value.code == VS_ERR_ARG
    for bad in (lambda: vs.sample_scores([(1, 100)], [[1.0, 2.0]], score_names=["one"]), lambda: vs.sample_scores([(1, 100)], np.zeros((1, 1, 1))),
                lambda: vs.sample_scores([(1, 100)], {}), lambda: vs.sample_scores([(1, 100)], {(9, "G", "A"): [1, 2], (10, "C", "T"): 1})):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(VariantStoreError):
        vs.sample_scores([(1, 100)], [1.0], samples=["nobody-of-that-name"])


class _StubCounts:
    """What the mapping form reads of a count result: the number of regions and every region's text."""

    def __init__(self, texts):
        self.texts = texts
        self.closed = False

    def totals(self):
        return (len(self.texts), 0, 0, 0)

    def region_text(self, q):
        return self.texts[q]

    def close(self):
        self.closed = True


def test_mapping_form_against_a_stubbed_count_result(host_store, monkeypatch):
    head = "Pos\tRef\tAlt\tCarriers\tAC\tHomAlt\tPhased\n"
    stub = _StubCounts([head + "10\tA\tC\t3\t4\t1\t1\n20\tG\tT\t2\t2\t0\t2\n", head, head + "20\tG\tT\t2\t2\t0\t2\n55\tC\t\t1\t2\t1\t1\n"])
    monkeypatch.setattr(host_store, "allele_counts", lambda regions: stub)
    w, unmatched = host_store._weights_from_mapping([(1, 30), (31, 32), (15, 60)], {(20, "G", "T"): [1.5, -2], (55, "C", ""): [0.25, 4], (99, "A", "G"): [7, 7]})
    assert w.dtype == np.float32 and w.tolist() == [[0, 0], [1.5, -2], [1.5, -2], [0.25, 4]]
    assert unmatched == [(99, "A", "G")] and stub.closed
    w, unmatched = host_store._weights_from_mapping([(1, 30), (31, 32), (15, 60)], {(10, "A", "C"): 3})
    assert w.tolist() == [[3], [0], [0], [0]] and unmatched == []


def test_cli_weight_file_errors(golden_dir, tmp_path):
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    subprocess.run([CLI, "construct", "-r", os.path.join(golden_dir, "x.small.fa"), "-v", os.path.join(golden_dir, "x.small.vcf"), "-p", prefix],
                   check=True, capture_output=True)
    wfile = os.path.join(tmp_path, "weights.txt")

    def run(text, *more):
        with open(wfile, "w") as f:
            f.write(text)
        p = subprocess.run([CLI, "score", "-p", prefix, "-r", "1:100", "-W", wfile, "--device", "-1", *more], capture_output=True, text=True)
        assert p.returncode != 0
        return p.stdout + p.stderr

    out = run("9 G A 0.5\n\n55 C\n")
    assert "line 3" in out and "malformed line" in out
    out = run("nine G A 0.5\n")
    assert "line 1" in out and "malformed line" in out
    out = run("9 G A 0.5 1\n55 C - 2\n")
    assert "line 2" in out and "1 values, 2 expected" in out
    out = run("#pos ref alt prs\n9 G A 0.5 1\n")
    assert "line 2" in out and "2 values, 1 expected" in out
    out = run("9 G A 0.5x\n")
    assert "line 1" in out and "not a number: 0.5x" in out
    assert "more than 8 values" in run("9 G A 1 2 3 4 5 6 7 8 9\n")
    out = run("#pos ref alt a b c d e f g h i\n")
    assert "line 1" in out and "more than 8 values" in out
    assert "line 2" in run("9 G A 1\n#pos ref alt late\n")
    out = run("9 G A 1\n9 G A 2\n")
    assert "line 2" in out and "twice" in out
    assert "no variants" in run("\n\n")
    valid = run("#pos ref alt prs pc1\n9\tG\tA\t0.5\t1e-3\n55 C - 2 3\n")          # a good file: the handle has no device
    assert "line" not in valid and "malformed" not in valid
    assert subprocess.run([CLI, "score", "-p", prefix, "-r", "1:100"], capture_output=True).returncode != 0   # no -W: the usage
    p = subprocess.run([CLI, "score", "-p", prefix, "-r", "1:100", "-W", os.path.join(tmp_path, "missing.txt"), "--device", "-1"],
                       capture_output=True, text=True)
    assert p.returncode != 0 and "cannot open weights file" in p.stdout + p.stderr
