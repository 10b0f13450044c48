"""Association scans without a GPU (vs_query_assoc_scan on a handle opened host-only): the reference helper on the golden VCFs
against hand-counted rows and on a hand-written text, every argument error the header states with its message where one is promised,
VS_ERR_NO_DEVICE for a valid call, the Python wrapper's own checks and the CLI's phenotype-file errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import assoc_scan_ref as ref
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
    """x.small.vcf by hand: sample `1` carries 9 G>A as 1|0 (dosage 1) and the deletion 54 CC>C, printed as `55 C -`, as 1|1 (dosage 2); x.vcf: 10 C>T 1|1, 14 G>A 1|0."""
    for stem, region, hand in (("x.small", (1, 60), {"9\tG\tA": 1, "55\tC\t": 2}), ("x", (1, 20), {"10\tC\tT": 2, "14\tG\tA": 1})):
        vs = VariantStore.from_vcf(os.path.join(golden_dir, stem + ".fa"), os.path.join(golden_dir, stem + ".vcf"), device=-1)
        plain = os.path.join(tmp_path, stem + ".bin")
        vs.export_plain(plain)
        name = vs.sample_name(1)
        vs.close()
        n, _early, text = Oracle(plain).get_var_in_ref(*region)
        assert n >= 0
        p = Parsed([text])
        y = np.array([[3, -2]], np.float32)
        got = ref.dot_int(p, [name], y)
        cnt = ref.counts(p, [name])
        real, mag, m = ref.dot_fsum(p, [name], y)
        for head, d in hand.items():
            i = p.heads.index(head)
            assert got[i].tolist() == [3 * d, -2 * d] and real[i].tolist() == [3.0 * d, -2.0 * d] and mag[i].tolist() == [3.0 * d, 2.0 * d]
            assert cnt[i].tolist() == [1, d, int(d == 2), 1] and m[i] == 1
        # one sample: vx = 1 * Sxx - Sx^2 is 0 for dosage 1 and not for dosage 2, but vy = 1 * y^2 - y^2 = 0: every cell is 0
        sy, syy = ref.trait_sums(y)
        assert sy.tolist() == [3.0, -2.0] and syy.tolist() == [9.0, 4.0]
        assert not ref.chi2(1, cnt[:, 1], cnt[:, 2], sy, syy, got).any()
        assert not ref.dot_int(p, ["nobody"], y).any()


def test_reference_on_a_hand_written_text():
    text = ("Pos\tRef\tAlt\tSamples\n"
            "10\tA\tC\tS1(1|1) S2(0/1) S3(1/0) \n"
            "20\tG\tT\tS4(1|0) \n"
            "40\tT\tG\t\n")
    cols = ["S1", "S2", "S4", "S5"]                     # S3 is outside the subset, S5 carries nothing
    y = np.array([[1, 0.5], [0, -1.25], [1, 4.0], [0, 2.0]], np.float32)
    p = Parsed([text])
    assert ref.dot_int(p, cols, y[:, :1]).tolist() == [[2], [1], [0]]
    real, mag, m = ref.dot_fsum(p, cols, y)
    assert real.tolist() == [[2.0, 2 * 0.5 - 1.25], [1.0, 4.0], [0.0, 0.0]] and mag[0].tolist() == [2.0, 2.25] and m.tolist() == [2, 1, 0]
    cnt = ref.counts(p, cols)
    assert cnt.tolist() == [[2, 3, 1, 1], [1, 1, 0, 1], [0, 0, 0, 0]]
    # the trend test by hand, trait 0 (0/1): n = 4, row 0: Sx = 3, Sxx = 5, vx = 20 - 9 = 11; Sy = 2, Syy = 2, vy = 8 - 4 = 4;
    # cov = 4 * 2 - 3 * 2 = 2; chi2 = 4 * 2 * 2 / (11 * 4)
    sy, syy = ref.trait_sums(y)
    c = ref.chi2(4, cnt[:, 1], cnt[:, 2], sy, syy, real)
    assert c[0, 0] == (4.0 * 2.0) * 2.0 / (11.0 * 4.0) and c[2].tolist() == [0.0, 0.0]
    assert c[1, 0] == (4.0 * 2.0) * 2.0 / (3.0 * 4.0)   # row 1: Sx = Sxx = 1, vx = 3, cov = 4 - 2
    assert not ref.chi2(4, cnt[:, 1], cnt[:, 2], [4.0], [4.0], real[:, :1]).any()   # a constant trait: vy = 0
    lines = ref.assoc_text(p, 0, cnt, real, ["cc", "q t"]).split("\n")
    assert lines[0] == "Pos\tRef\tAlt\tCarriers\tAC\tHomAlt\tPhased\tcc\tq t"
    assert lines[1] == "10\tA\tC\t2\t3\t1\t1\t2\t-0.25" and lines[3] == "40\tT\tG\t0\t0\t0\t0\t0\t0"
    assert ref.assoc_text(p, 0, cnt, real).split("\n")[0].endswith("Phased\t0\t1")


def _call(vs, n=1, ids=(1,), traits=((0.5,),), n_traits=None, stat=0, names=None, n_ids=None, null_ids=False, null_traits=False):
    """vs_query_assoc_scan through ctypes: (code, message)."""
    lib = _lib.load()
    regions = (_lib.Region * max(n, 1))(*[_lib.Region(1, 100)] * max(n, 1))
    a = np.ascontiguousarray(ids, dtype=np.uint32)
    y = np.ascontiguousarray(traits, dtype=np.float32)
    pa = None if null_ids else a.ctypes.data_as(C.POINTER(C.c_uint32))
    py = None if null_traits else y.ctypes.data_as(C.POINTER(C.c_float))
    pn = (C.c_char_p * len(names))(*[s.encode() for s in names]) if names is not None else None
    h = C.c_void_p()
    rc = lib.vs_query_assoc_scan(vs._h, regions, n, pa, len(a) if n_ids is None else n_ids, py, y.shape[1] if n_traits is None else n_traits,
                                 stat, pn, C.byref(h))
    assert rc != 0 and not h.value
    return rc, lib.vs_last_error().decode()


def test_argument_errors(host_store):
    vs = host_store
    ns = vs.info().num_samples
    assert ns == 2                                                          # x.small: "ref" and one sample, id 1
    assert _call(vs, n=0)[0] == VS_ERR_ARG
    assert _call(vs, null_traits=True)[0] == VS_ERR_ARG
    assert _call(vs, n_traits=0)[0] == VS_ERR_ARG
    assert _call(vs, traits=[[0.0] * 9])[0] == VS_ERR_ARG
    assert _call(vs, stat=2)[0] == VS_ERR_ARG
    assert _call(vs, n_ids=0)[0] == VS_ERR_ARG
    assert _call(vs, null_ids=True, n_ids=0)[0] == VS_ERR_ARG
    assert _call(vs, ids=(ns + 5,), stat=7)[0] == VS_ERR_ARG               # before the unknown sample
    # NULL ids: the phenotypes are the whole cohort's
    assert _call(vs, null_ids=True, n_ids=2, traits=[[1.0], [2.0]])[0] == VS_ERR_ARG
    # "ref" or an id beyond the cohort
    assert _call(vs, ids=(0,))[0] == VS_ERR_UNKNOWN_SAMPLE
    assert _call(vs, ids=(ns,))[0] == VS_ERR_UNKNOWN_SAMPLE
    assert _call(vs, ids=(1, ns), traits=[[1.0], [2.0]])[0] == VS_ERR_UNKNOWN_SAMPLE
    # a sample listed twice: the message names the id
    rc, msg = _call(vs, ids=(1, 1), traits=[[1.0], [2.0]])
    assert rc == VS_ERR_ARG and "sample id 1" in msg and "twice" in msg
    # a value that is not finite: the message names the sample id and the trait
    for bad in (np.nan, np.inf, -np.inf):
        rc, msg = _call(vs, traits=[[1.0, 2.0, bad]])
        assert rc == VS_ERR_ARG and "sample id 1" in msg and "trait 2" in msg, msg
    rc, msg = _call(vs, null_ids=True, n_ids=1, traits=[[np.nan]])
    assert rc == VS_ERR_ARG and "sample id 1" in msg and "trait 0" in msg
    # a name with a tab or a newline
    assert _call(vs, names=["a\tb"])[0] == VS_ERR_ARG
    assert _call(vs, traits=[[1.0, 2.0]], names=["ok", "two\nlines"])[0] == VS_ERR_ARG
    # the option
    for bad in (-1, 129):
        with pytest.raises(VariantStoreError) as e:
            vs.set_option("assoc_lds_max_kib", bad)
        assert e.value.code == VS_ERR_ARG
    for ok in (1, 128, 0):
        vs.set_option("assoc_lds_max_kib", ok)


def test_valid_call_on_a_host_only_handle_has_no_device(host_store):
    vs = host_store
    assert _call(vs)[0] == VS_ERR_NO_DEVICE
    assert _call(vs, null_ids=True, n_ids=1, traits=[[1.0] * 8], stat=1, names=[f"t{k}" for k in range(8)])[0] == VS_ERR_NO_DEVICE
    for kw in (dict(), dict(samples=[1]), dict(samples=[vs.sample_name(1)], stat="chi2", trait_names=["bmi"])):
        with pytest.raises(VariantStoreError) as e:
            vs.assoc_scan([(1, 100)], [0.25], **kw)
        assert e.value.code == VS_ERR_NO_DEVICE
    with pytest.raises(VariantStoreError) as e:
        vs.assoc_scan([(1, 100)], [1.0, 2.0], samples=[1, 1])
    assert e.value.code == VS_ERR_ARG
    with pytest.raises(VariantStoreError) as e:
        vs.assoc_scan([(1, 100)], [1.0, 2.0])               # two rows for a cohort of one
    assert e.value.code == VS_ERR_ARG
    for bad in (lambda: vs.assoc_scan([(1, 100)], [1.0], stat="r2"), lambda: vs.assoc_scan([(1, 100)], [1.0, 2.0], samples=[1]),
                lambda: vs.assoc_scan([(1, 100)], [[1.0, 2.0]], trait_names=["one"]), lambda: vs.assoc_scan([(1, 100)], np.zeros((1, 1, 1)))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(VariantStoreError):
        vs.assoc_scan([(1, 100)], [1.0], samples=["nobody-of-that-name"])


def test_cli_phenotype_file_errors(golden_dir, tmp_path):
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    subprocess.run([CLI, "construct", "-r", os.path.join(golden_dir, "x.small.fa"), "-v", os.path.join(golden_dir, "x.small.vcf"), "-p", prefix],
                   check=True, capture_output=True)
    pfile = os.path.join(tmp_path, "pheno.txt")

    def run(text, *more):
        with open(pfile, "w") as f:
            f.write(text)
        p = subprocess.run([CLI, "assoc", "-p", prefix, "-r", "1:100", "-P", pfile, "--device", "-1", *more], capture_output=True, text=True)
        assert p.returncode != 0
        return p.stdout + p.stderr

    out = run("#sample bmi ldl\n1\t0.5\t1\n\nnobody-of-that-name 1 2\n")
    assert "line 4" in out and "Sample not found: nobody-of-that-name" in out
    out = run("1 0.5 1\n1 2\n")
    assert "line 2" in out and "1 values, 2 expected" in out
    out = run("#sample bmi\n1 0.5 1\n")
    assert "line 2" in out and "2 values, 1 expected" in out
    out = run("1 0.5 1x\n")
    assert "line 1" in out and "not a number: 1x" in out
    assert "line 1" in run("1\n")
    assert "line 2" in run("1 2\n#sample late\n")
    assert "more than 8 traits" in run("1 1 2 3 4 5 6 7 8 9\n")
    out = run("#sample a b c d e f g h i\n")
    assert "line 1" in out and "more than 8 traits" in out
    assert "Sample not found: #foo" in run("#foo a b\n1 1 2\n")       # only `#sample` names traits
    assert "no samples" in run("\n\n")
    valid = run("#sample bmi ldl\n1\t0.5\t1e-3\n", "--chi2")       # a good file: the handle has no device
    assert "line" not in valid and "Sample not found" not in valid
    assert subprocess.run([CLI, "assoc", "-p", prefix, "-r", "1:100"], capture_output=True).returncode != 0   # no -P: the usage
    p = subprocess.run([CLI, "assoc", "-p", prefix, "-r", "1:100", "-P", os.path.join(tmp_path, "missing.txt"), "--device", "-1"],
                       capture_output=True, text=True)
    assert p.returncode != 0 and "cannot open phenotype file" in p.stdout + p.stderr
