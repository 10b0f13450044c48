"""Score-matrix queries without a GPU (vs_query_score_matrix on a handle opened host-only): the reference's quantiser against the
engine's (vs_assoc_matrix_quantise) bit for bit, the reference's row totals and limb counts on hand-worked numbers, every host
refusal in the contract's order and with its code, then VS_ERR_NO_DEVICE -- up to 65,536 weight columns, 65,537 refused --, option
score_matrix_chunk, the Python wrapper's own checks, the CLI without -W, and the digit split as a stand-alone program, plain and
under AddressSanitizer + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import score_matrix_ref as ref
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


def test_reference_quantiser_is_the_engines():
    rng = np.random.default_rng(3)
    w = rng.normal(0, 2, size=(200, 7)).astype(np.float32)
    w[:, 1] = 0
    w[:, 2] *= np.float32(1e-20)
    w[:, 3] *= np.float32(1e6)
    w[:, 4] = np.where(rng.integers(0, 2, size=200) == 1, np.float32(1.0), np.float32(2.0 ** -30))
    q, f = quantise_traits(w)
    assert np.array_equal(f, ref.shifts(w)) and np.array_equal(q.astype(np.int64), ref.quantise(w))
    assert f[1] == 0 and f[4] == 29 and np.abs(q).max() < 2 ** 30
    assert ref.shifts(np.zeros((0, 3), np.float32)).tolist() == [0, 0, 0]


def test_reference_totals_and_limbs_by_hand():
    """Three reports, two of them of table row 1: T adds their fixed-point weights.  The limb count flips between 2,139,062,143 and
    2,139,062,144."""
    w = np.array([[1.0, 0.5], [1.0, -1.0], [0.5, 1.0]], np.float32)   # f = 29 for both columns: q = w 2^29
    t = ref.totals(w, [0, 1, 1], 3)
    assert t.tolist() == [[2 ** 29, 2 ** 28], [2 ** 29 + 2 ** 28, 0], [0, 0]]
    assert ref.limbs_needed(t) == 4
    assert ref.MAX4 == 2139062143 and ref.MAX5 == 547599908735
    assert ref.limbs_needed(np.array([ref.MAX4, -ref.MAX4])) == 4 and ref.limbs_needed(np.array([ref.MAX4 + 1])) == 5
    assert ref.limbs_needed(np.array([-(ref.MAX4 + 1)])) == 5 and ref.limbs_needed(np.array([1 << 38])) == 5
    # ten reports of one row at the column's largest weight: 10 (2^30 - 2^29) > MAX4
    assert ref.limbs_needed(ref.totals(np.ones((10, 1), np.float32), [0] * 10, 1)) == 5
    with pytest.raises(AssertionError):
        ref.limbs_needed(np.array([(1 << 38) + 1]))


def _call(vs, n=1, ids=(1,), weights=((0.5,),), n_scores=None, n_weights=None, names=None, n_ids=None, null_ids=False, null_weights=False):
    """vs_query_score_matrix through ctypes: (code, message)."""
    lib = _lib.load()
    regions = (_lib.Region * max(n, 1))(*[_lib.Region(1, 100)] * max(n, 1))
    a = np.ascontiguousarray(ids, dtype=np.uint32)
    w = np.ascontiguousarray(weights, dtype=np.float32)
    pa = None if null_ids else a.ctypes.data_as(C.POINTER(C.c_uint32))
    pw = None if null_weights else w.ctypes.data_as(C.POINTER(C.c_float))
    pn = (C.c_char_p * len(names))(*[s.encode() for s in names]) if names is not None else None
    h = C.c_void_p()
    rc = lib.vs_query_score_matrix(vs._h, regions, n, pa, len(a) if n_ids is None else n_ids, pw, w.shape[0] if n_weights is None else n_weights,
                                   w.shape[1] if n_scores is None else n_scores, pn, C.byref(h))
    assert rc != 0 and not h.value
    return rc, lib.vs_last_error().decode()


def test_host_refusals_in_order_then_no_device(host_store):
    vs = host_store
    ns = vs.info().num_samples
    assert ns == 2                                                          # x.small: "ref" and one sample, id 1
    nan = [[1.0, np.nan]]
    # each refusal alone
    assert _call(vs, n=0)[0] == VS_ERR_ARG
    rc, msg = _call(vs, n_scores=0)
    assert rc == VS_ERR_ARG and "0 scores" in msg
    rc, msg = _call(vs, weights=[[0.0] * 65537])                            # VS_SCORE_MATRIX_MAX + 1
    assert rc == VS_ERR_ARG and "65537 scores" in msg and "65536" in msg
    assert _call(vs, null_weights=True)[0] == VS_ERR_ARG
    for bad in (np.nan, np.inf, -np.inf):
        rc, msg = _call(vs, weights=[[1.0] * 20 + [bad] + [0.0] * 19])
        assert rc == VS_ERR_ARG and "column 20" in msg and "not finite" in msg, msg
    rc, msg = _call(vs, weights=[[1.0, 2.0]], names=["ok", "two\nlines"])
    assert rc == VS_ERR_ARG and "score 1" in msg
    assert _call(vs, names=["a\tb"])[0] == VS_ERR_ARG
    assert _call(vs, n_ids=0)[0] == VS_ERR_ARG
    assert _call(vs, null_ids=True, n_ids=2)[0] == VS_ERR_ARG               # without ids the columns are the whole cohort's
    assert _call(vs, ids=(0,))[0] == VS_ERR_UNKNOWN_SAMPLE
    assert _call(vs, ids=(ns,))[0] == VS_ERR_UNKNOWN_SAMPLE
    rc, msg = _call(vs, ids=(1, 1))
    assert rc == VS_ERR_ARG and "sample id 1" in msg and "twice" in msg
    rc, msg = _call(vs, weights=np.zeros((1 << 26, 1), np.float32))         # N >= 2^26, already by the rows of weights
    assert rc == VS_ERR_ARG and "2^26" in msg
    # the order: the number of scores, a weight that is not finite, a name, the ids
    assert "scores" in _call(vs, n_scores=0, weights=nan, names=["a\tb", "c"], ids=(0,))[1]
    assert "not finite" in _call(vs, weights=nan, names=["a\tb", "c"], ids=(0,))[1]
    rc, msg = _call(vs, weights=[[1.0, 2.0]], names=["a\tb", "c"], ids=(0,))
    assert rc == VS_ERR_ARG and "name of score 0" in msg
    assert _call(vs, weights=[[1.0, 2.0]], names=["a", "c"], ids=(0,))[0] == VS_ERR_UNKNOWN_SAMPLE
    assert _call(vs, weights=[[1.0, 2.0]], names=["a", "c"], ids=(1, 1))[0] == VS_ERR_ARG
    # nothing left to refuse on the host: the device is asked for
    assert _call(vs)[0] == VS_ERR_NO_DEVICE
    assert _call(vs, null_ids=True, n_ids=1, weights=[[1.0] * 9], names=[f"s{k}" for k in range(9)])[0] == VS_ERR_NO_DEVICE
    for K in (8, 9, 300, 65536):                                            # no limit of 8 here; 65,536 passes the host's checks
        assert _call(vs, weights=np.ones((3, K), np.float32))[0] == VS_ERR_NO_DEVICE
    assert _call(vs, weights=np.zeros((0, 4), np.float32))[0] == VS_ERR_NO_DEVICE   # no rows of weights: for the plan to judge
    # ... while sample_scores keeps its limit of 8
    with pytest.raises(VariantStoreError) as e:
        vs.sample_scores([(1, 100)], np.ones((1, 9), np.float32))
    assert e.value.code == VS_ERR_ARG


def test_python_wrapper(host_store):
    vs = host_store
    for kw in (dict(), dict(samples=[1]), dict(samples=[vs.sample_name(1)], score_names=["prs"])):
        with pytest.raises(VariantStoreError) as e:
            vs.score_matrix([(1, 100)], [0.25], **kw)
        assert e.value.code == VS_ERR_NO_DEVICE
    with pytest.raises(VariantStoreError) as e:
        vs.score_matrix([(1, 100)], np.ones((5, 40)))
    assert e.value.code == VS_ERR_NO_DEVICE
    with pytest.raises(VariantStoreError) as e:
        vs.score_matrix([(1, 100)], np.ones((5, 40)), samples=[1, 1])
    assert e.value.code == VS_ERR_ARG
    with pytest.raises(VariantStoreError) as e:
        vs.score_matrix([(1, 100)], np.array([[1.0, np.inf]]))
    assert e.value.code == VS_ERR_ARG and "column 1" in str(e.value)
    for bad in (lambda: vs.score_matrix([(1, 100)], [[1.0, 2.0]], score_names=["one"]), lambda: vs.score_matrix([(1, 100)], np.zeros((1, 1, 1))),
                lambda: vs.score_matrix([(1, 100)], {})):
        with pytest.raises(ValueError):
            bad()


def test_score_matrix_chunk_option(host_store):
    vs = host_store
    for ok in (0, 128, 256, 4096, 65536, 0):
        vs.set_option("score_matrix_chunk", ok)
    for bad in (-1, 1, 64, 127, 129, 200, 65536 + 128, 1 << 20):
        with pytest.raises(VariantStoreError) as e:
            vs.set_option("score_matrix_chunk", bad)
        assert e.value.code == VS_ERR_ARG and "score_matrix_chunk" in str(e.value)


def test_cli_without_weights_prints_the_usage(golden_dir, tmp_path):
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    subprocess.run([CLI, "construct", "-r", os.path.join(golden_dir, "x.small.fa"), "-v", os.path.join(golden_dir, "x.small.vcf"), "-p", prefix],
                   check=True, capture_output=True)
    p = subprocess.run([CLI, "scorematrix", "-p", prefix, "-r", "1:100"], capture_output=True, text=True)
    assert p.returncode != 0 and "SYNOPSIS" in p.stdout and "scorematrix" in p.stdout
    wfile = os.path.join(tmp_path, "weights.txt")

    def run(text, cmd="scorematrix"):
        with open(wfile, "w") as f:
            f.write(text)
        p = subprocess.run([CLI, cmd, "-p", prefix, "-r", "1:100", "-W", wfile, "--device", "-1"], capture_output=True, text=True)
        assert p.returncode != 0
        return p.stdout + p.stderr

    assert "2 values, 3 expected" in run("10 C T 1 2 3\n14 G A 1 2\n")
    values = " ".join(str(0.25 * k) for k in range(12))
    for text in (f"10 C T {values}\n", "#pos ref alt " + " ".join(f"s{k}" for k in range(12)) + f"\n10 C T {values}\n"):
        out = run(text)                                                      # 12 columns are read; what stops the run is the missing device
        assert "more than" not in out and "line" not in out, out
        assert "more than 8 values" in run(text, cmd="score")               # `score` keeps its limit and its message
    p = subprocess.run([CLI, "scorematrix", "-p", prefix, "-r", "1:100", "-W", os.path.join(tmp_path, "missing.txt"), "--device", "-1"],
                       capture_output=True, text=True)
    assert p.returncode != 0 and "cannot open weights file" in p.stdout + p.stderr


def test_digit_split_standalone_and_under_sanitizers(tmp_path):
    """score_matrix_host.hpp in a stand-alone program: built plainly, and once more with AddressSanitizer + UBSan (CPU only)."""
    src = os.path.join(ROOT, "tests", "native", "score_matrix_host_check.cpp")
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])):
        exe = os.path.join(tmp_path, "score_matrix_host_check_" + name)
        subprocess.check_call(["g++", "-std=c++17", *flags, "-o", exe, src])
        out = subprocess.run([exe], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.startswith("ok ") and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
        assert int(out.stdout.split()[1]) > 1_000_000
