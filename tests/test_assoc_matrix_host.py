"""Trait-matrix association scans without a GPU (vs_query_assoc_matrix on a handle opened host-only): the reference on a hand-worked
example, the engine's quantiser (vs_assoc_matrix_quantise) against the reference bit for bit, every argument error of
vs_query_assoc_scan restated for the new call, VS_ERR_NO_DEVICE for a valid call with 9 and 300 traits, the Python wrapper's own
checks, the CLI's phenotype reader without the 8-trait limit, and the host code under AddressSanitizer + UBSan as a stand-alone
program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import assoc_matrix_ref as ref
from variantstore_amd import VariantStore, _lib, quantise_traits
from variantstore_amd.api import VariantStoreError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
VS_ERR_NO_DEVICE, VS_ERR_ARG, VS_ERR_UNKNOWN_SAMPLE = -3, -5, -6


@pytest.fixture(scope="module")
def host_store(golden_dir):
    vs = VariantStore.from_vcf(os.path.join(golden_dir, "x.small.fa"), os.path.join(golden_dir, "x.small.vcf"), device=-1)
    yield vs
    vs.close()


def test_reference_on_a_hand_worked_example():
    """3 rows x 4 samples x 2 traits, every number written out."""
    D = np.array([[2, 1, 0, 0],      # Sx = 3, Sxx = 5
                  [0, 0, 1, 0],      # Sx = 1, Sxx = 1
                  [0, 0, 0, 0]])     # a carrier-free row
    y = np.array([[1.0, 0.75], [0.0, -1.5], [1.0, 3.0], [0.0, 0.0]], np.float32)
    q, f = ref.quantise(y)
    # trait 0: max 1 = 0.5 * 2^1, f = 29, q = y * 2^29; trait 1: max 3 = 0.75 * 2^2, f = 28, q = y * 2^28
    assert f.tolist() == [29, 28]
    assert q.tolist() == [[2 ** 29, 3 * 2 ** 26], [0, -3 * 2 ** 27], [2 ** 29, 3 * 2 ** 28], [0, 0]]
    # the limbs of 2^29 = 32 * 2^24: (0, 0, 0, 32); of 3 * 2^26 = 12 * 2^24: (0, 0, 0, 12); of -3 * 2^27 = -24 * 2^24
    assert ref.limbs(q)[:2].tolist() == [[[0, 0, 0, 32], [0, 0, 0, 12]], [[0, 0, 0, 0], [0, 0, 0, -24]]]
    S = ref.dot(D, q)
    assert S.tolist() == [[2 ** 30, 6 * 2 ** 26 - 3 * 2 ** 27], [2 ** 29, 3 * 2 ** 28], [0, 0]]
    assert (ref.dot_by_limbs(D, q) == S).all()
    assert ref.scores_dot(S, f).tolist() == [[2.0, 0.0], [1.0, 3.0], [0.0, 0.0]]
    # CHI2, trait 0 in units of 2^29 (the scale cancels): n = 4, Sy = 2, Syy = 2, vy = 8 - 4 = 4
    #   row 0: vx = 4 * 5 - 9 = 11, cov = 4 * 2 - 3 * 2 = 2, chi2 = 4 * 2 * 2 / (11 * 4)
    #   row 1: vx = 4 * 1 - 1 = 3,  cov = 4 * 1 - 1 * 2 = 2, chi2 = 4 * 2 * 2 / (3 * 4)
    c = ref.chi2(4, [3, 1, 0], [1, 0, 0], S, q)
    assert c[0, 0] == 16.0 / 44.0 and c[1, 0] == 16.0 / 12.0 and c[2].tolist() == [0.0, 0.0]
    # trait 1 in units of 2^26: q = (3, -6, 12, 0): Sy = 9, Syy = 189, vy = 756 - 81 = 675; row 0: S = 0, cov = -27;
    # row 1: S = 12, cov = 48 - 9 = 39
    assert c[0, 1] == (4.0 * 27.0) * 27.0 / (11.0 * 675.0) and c[1, 1] == (4.0 * 39.0) * 39.0 / (3.0 * 675.0)
    sy, syy = ref.trait_sums(q, f)
    assert sy.tolist() == [2.0, 2.25] and syy.tolist() == [2.0, 0.75 ** 2 + 1.5 ** 2 + 9.0]


def _same(y):
    y = np.ascontiguousarray(y, np.float32)
    q, f = quantise_traits(y)
    rq, rf = ref.quantise(y)
    assert q.dtype == np.int32 and f.dtype == np.int32
    assert (f == rf).all(), (f, rf)
    assert (q == rq).all()
    return q, f


def test_quantiser_equals_the_reference():
    rng = np.random.default_rng(11)
    _same(rng.normal(0, 3, size=(300, 33)))
    _same(rng.normal(0, 1e-3, size=(17, 1)))
    q, f = _same(np.zeros((5, 3)))                                           # columns of zeros: f = 0, q = 0
    assert not q.any() and not f.any()
    y = rng.normal(0, 1, size=(40, 4)).astype(np.float32)
    y[:, 1] = 0
    y[3, 2] = 8.0                                                            # the largest value a power of two: e = 4
    y[:, 2] = np.clip(y[:, 2], -8, 8)
    y[5, 3] = np.nextafter(np.float32(8.0), np.float32(0))                   # ... and just below one: e = 3, q = 2^30 - 64
    y[:, 3] = np.clip(y[:, 3], -7, y[5, 3])
    q, f = _same(y)
    assert f.tolist()[1:] == [0, 26, 27] and q[3, 2] == 2 ** 29 and q[5, 3] == 2 ** 30 - 64
    # ties at .5: with the largest value 2^29 (f = 0) the values k + 0.5 are exact in float32 and round to even
    t = np.array([2.0 ** 29, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 1023.5, 1024.5], np.float32).reshape(-1, 1)
    q, f = _same(t)
    assert f.tolist() == [0] and q[:, 0].tolist() == [2 ** 29, 0, 2, 2, 0, -2, -2, 1024, 1024]
    # denormals: a column of denormals alone (its largest 3 * 2^-149: f = 177), and denormals beside a normal value (they round to 0)
    q, f = _same(np.array([[2.0 ** -149, 1.0], [-(2.0 ** -149), 2.0 ** -140], [3 * 2.0 ** -149, 0.0]], np.float32))
    assert f.tolist() == [177, 29] and q[:, 0].tolist() == [2 ** 28, -(2 ** 28), 3 * 2 ** 28] and q[:, 1].tolist() == [2 ** 29, 0, 0]
    _same(np.array([[3.0e38, -1.0e-30]], np.float32))                        # the other end of the range: f = -98


def test_quantiser_on_chosen_limbs():
    """Traits built by ldexp from chosen q come back as chosen, and the limbs the values were chosen for are hit."""
    y, want = ref.chosen_traits(64)
    q, f = _same(y)
    assert f.tolist() == [0, 20] and (q == want).all()
    b = ref.limbs(want)
    assert set(ref.CHOSEN_Q) <= set(want[:, 0].tolist())
    for l in range(3):                                                       # both extremes in the three low limbs
        assert b[..., l].min() == -128 and b[..., l].max() == 127, l
    assert b[..., 3].min() == -64 and b[..., 3].max() == 64                  # |q| < 2^30 bounds the top limb
    hand = {127: (127, 0, 0, 0), 128: (-128, 1, 0, 0), 129: (-127, 1, 0, 0), 255: (-1, 1, 0, 0), 256: (0, 1, 0, 0), -128: (-128, 0, 0, 0),
            -129: (127, -1, 0, 0), 0x7F7F7F: (127, 127, 127, 0), 0x808080: (-128, -127, -127, 1), 2 ** 30 - 64: (-64, 0, 0, 64),
            -(2 ** 30 - 64): (64, 0, 0, -64)}
    for v, digits in hand.items():
        assert tuple(ref.limbs(np.array([v]))[0].tolist()) == digits, v
        assert sum(d * 256 ** l for l, d in enumerate(digits)) == v


def test_quantiser_argument_errors():
    lib = _lib.load()
    y = np.ones((2, 2), np.float32)
    q, f = np.zeros((2, 2), np.int32), np.zeros(2, np.int32)
    py, pq, pf = y.ctypes.data_as(C.POINTER(C.c_float)), q.ctypes.data_as(C.POINTER(C.c_int32)), f.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.vs_assoc_matrix_quantise(py, 2, 2, pq, pf) == 0
    for args in ((None, 2, 2, pq, pf), (py, 2, 2, None, pf), (py, 2, 2, pq, None), (py, 0, 2, pq, pf), (py, 2, 0, pq, pf)):
        assert lib.vs_assoc_matrix_quantise(*args) == VS_ERR_ARG
    for bad in (np.nan, np.inf, -np.inf):
        y[1, 0] = bad
        assert lib.vs_assoc_matrix_quantise(py, 2, 2, pq, pf) == VS_ERR_ARG
        with pytest.raises(VariantStoreError):
            quantise_traits(y)
    for shape in ((0, 2), (2, 0), (1, 1, 1)):
        with pytest.raises(ValueError):
            quantise_traits(np.zeros(shape, np.float32))


def _call(vs, n=1, ids=(1,), traits=((0.5,),), n_traits=None, stat=0, names=None, n_ids=None, null_ids=False, null_traits=False):
    """vs_query_assoc_matrix through ctypes: (code, message)."""
    lib = _lib.load()
    regions = (_lib.Region * max(n, 1))(*[_lib.Region(1, 100)] * max(n, 1))
    a = np.ascontiguousarray(ids, dtype=np.uint32)
    y = np.ascontiguousarray(traits, dtype=np.float32)
    pa = None if null_ids else a.ctypes.data_as(C.POINTER(C.c_uint32))
    py = None if null_traits else y.ctypes.data_as(C.POINTER(C.c_float))
    pn = (C.c_char_p * len(names))(*[s.encode() for s in names]) if names is not None else None
    h = C.c_void_p()
    rc = lib.vs_query_assoc_matrix(vs._h, regions, n, pa, len(a) if n_ids is None else n_ids, py, y.shape[1] if n_traits is None else n_traits,
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
    assert _call(vs, traits=[[0.0] * 65537])[0] == VS_ERR_ARG              # VS_TRAIT_MATRIX_MAX + 1
    assert _call(vs, stat=2)[0] == VS_ERR_ARG
    assert _call(vs, n_ids=0)[0] == VS_ERR_ARG
    assert _call(vs, null_ids=True, n_ids=0)[0] == VS_ERR_ARG
    assert _call(vs, ids=(ns + 5,), stat=7)[0] == VS_ERR_ARG               # before the unknown sample
    assert _call(vs, ids=(ns + 5,), traits=[[0.0] * 65537])[0] == VS_ERR_ARG
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
        rc, msg = _call(vs, traits=[[1.0] * 20 + [bad] + [0.0] * 19])
        assert rc == VS_ERR_ARG and "sample id 1" in msg and "trait 20" in msg, msg
    rc, msg = _call(vs, null_ids=True, n_ids=1, traits=[[np.nan]])
    assert rc == VS_ERR_ARG and "sample id 1" in msg and "trait 0" in msg
    # a name with a tab or a newline
    assert _call(vs, names=["a\tb"])[0] == VS_ERR_ARG
    assert _call(vs, traits=[[1.0, 2.0]], names=["ok", "two\nlines"])[0] == VS_ERR_ARG


def test_valid_call_on_a_host_only_handle_has_no_device(host_store):
    vs = host_store
    assert _call(vs)[0] == VS_ERR_NO_DEVICE
    for K in (8, 9, 300, 65536):                                            # no limit of 8 here
        assert _call(vs, traits=[[1.0] * K])[0] == VS_ERR_NO_DEVICE
    assert _call(vs, null_ids=True, n_ids=1, traits=[[1.0] * 9], stat=1, names=[f"t{k}" for k in range(9)])[0] == VS_ERR_NO_DEVICE
    for kw in (dict(), dict(samples=[1]), dict(samples=[vs.sample_name(1)], stat="chi2", trait_names=["bmi"])):
        with pytest.raises(VariantStoreError) as e:
            vs.assoc_matrix([(1, 100)], [0.25], **kw)
        assert e.value.code == VS_ERR_NO_DEVICE
    with pytest.raises(VariantStoreError) as e:
        vs.assoc_matrix([(1, 100)], np.ones((1, 40)))
    assert e.value.code == VS_ERR_NO_DEVICE
    with pytest.raises(VariantStoreError) as e:
        vs.assoc_matrix([(1, 100)], [1.0, 2.0], samples=[1, 1])
    assert e.value.code == VS_ERR_ARG
    with pytest.raises(VariantStoreError) as e:
        vs.assoc_matrix([(1, 100)], [1.0, 2.0])               # two rows for a cohort of one
    assert e.value.code == VS_ERR_ARG
    for bad in (lambda: vs.assoc_matrix([(1, 100)], [1.0], stat="r2"), lambda: vs.assoc_matrix([(1, 100)], [1.0, 2.0], samples=[1]),
                lambda: vs.assoc_matrix([(1, 100)], [[1.0, 2.0]], trait_names=["one"]), lambda: vs.assoc_matrix([(1, 100)], np.zeros((1, 1, 1)))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(VariantStoreError):
        vs.assoc_matrix([(1, 100)], [1.0], samples=["nobody-of-that-name"])
    # assoc_scan keeps its limit
    with pytest.raises(VariantStoreError) as e:
        vs.assoc_scan([(1, 100)], np.ones((1, 9)))
    assert e.value.code == VS_ERR_ARG


def test_cli_phenotype_file(golden_dir, tmp_path):
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    subprocess.run([CLI, "construct", "-r", os.path.join(golden_dir, "x.small.fa"), "-v", os.path.join(golden_dir, "x.small.vcf"), "-p", prefix],
                   check=True, capture_output=True)
    pfile = os.path.join(tmp_path, "pheno.txt")

    def run(text, *more, cmd="assocmatrix"):
        with open(pfile, "w") as f:
            f.write(text)
        p = subprocess.run([CLI, cmd, "-p", prefix, "-r", "1:100", "-P", pfile, "--device", "-1", *more], capture_output=True, text=True)
        assert p.returncode != 0
        return p.stdout + p.stderr

    out = run("#sample bmi ldl\n1\t0.5\t1\n\nnobody-of-that-name 1 2\n")
    assert "line 4" in out and "Sample not found: nobody-of-that-name" in out
    out = run("1 0.5 1\n1 2\n")
    assert "line 2" in out and "1 values, 2 expected" in out
    out = run("1 0.5 1x\n")
    assert "line 1" in out and "not a number: 1x" in out
    assert "line 1" in run("1\n")
    assert "line 2" in run("1 2\n#sample late\n")
    assert "no samples" in run("\n\n")
    for K in (9, 40):                                            # accepted up to the missing device, with and without names
        values = " ".join(str(0.25 * k) for k in range(K))
        for text in (f"1 {values}\n", "#sample " + " ".join(f"t{k}" for k in range(K)) + f"\n1 {values}\n"):
            valid = run(text, "--chi2")
            assert "line" not in valid and "Sample not found" not in valid and "more than" not in valid, valid
            assert "more than 8 traits" in run(text, cmd="assoc")          # `assoc` keeps its limit and its message
    assert subprocess.run([CLI, "assocmatrix", "-p", prefix, "-r", "1:100"], capture_output=True).returncode != 0   # no -P: the usage
    p = subprocess.run([CLI, "assocmatrix", "-p", prefix, "-r", "1:100"], capture_output=True, text=True)
    assert "SYNOPSIS" in p.stdout and "assocmatrix" in p.stdout
    p = subprocess.run([CLI, "assocmatrix", "-p", prefix, "-r", "1:100", "-P", os.path.join(tmp_path, "missing.txt"), "--device", "-1"],
                       capture_output=True, text=True)
    assert p.returncode != 0 and "cannot open phenotype file" in p.stdout + p.stderr


def test_host_code_under_sanitizers_standalone(tmp_path):
    """The quantiser and the panel writer (assoc_matrix_host.hpp) in a stand-alone program with AddressSanitizer + UBSan (CPU only)."""
    exe = os.path.join(tmp_path, "assoc_matrix_host_check")
    src = os.path.join(ROOT, "tests", "native", "assoc_matrix_host_check.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok ") and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def test_table_form_of_the_reference_equals_the_python_integers():
    rng = np.random.default_rng(5)
    n = 300
    D = rng.integers(0, 3, size=(40, n))
    D[3] = 0
    D[4] = 2
    y = rng.normal(0, 2, size=(n, 7)).astype(np.float32)
    y[:, 2] = 0
    y[:, 3] = 1.5
    q, _f = ref.quantise(y)
    S = ref.dot(D, q)
    ac, hom = D.sum(axis=1), (D == 2).sum(axis=1)
    a, b = ref.chi2(n, ac, hom, S, q), ref.chi2_table(n, ac, hom, S, q)
    assert a.tobytes() == b.tobytes() and a.any() and not a[3].any() and not a[4].any() and not a[:, 2].any() and not a[:, 3].any()
