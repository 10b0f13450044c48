"""LD-matrix queries without a GPU: the helper that derives the expected blocks and text from a genotype matrix against a hand-worked
example, the argument checks of vs_query_ld_matrix (made on the host, before the handle's device is asked for) and their order, the
Python wrapper's statistic names and codes, and the CLI's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from genotype_matrix_ref import Parsed, matrix
from ld_matrix_ref import block, block_begin, block_r2, blocks, ld_matrix_text
from variantstore_amd import VariantStore, _lib
from variantstore_amd.api import QueryResult, VariantStoreError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
VS_ERR_NO_DEVICE, VS_ERR_ARG, VS_ERR_UNKNOWN_SAMPLE = -3, -5, -6
DOT, R2 = 0, 1


@pytest.fixture(scope="module")
def host_store(golden_dir):
    vs = VariantStore.from_vcf(os.path.join(golden_dir, "x.small.fa"), os.path.join(golden_dir, "x.small.vcf"), device=-1)
    yield vs
    vs.close()


# S4 has a 1|2 call (a carrier of both ALT rows at 10), S3 a haploid 1 (gt_1 alone); the row at 12 has no carrier
TEXTS = [("Pos\tRef\tAlt\tSamples\n"
          "10\tA\tC\tS1(1|1) S2(0/1) S3(1/0) S4(1|1) \n"
          "10\tA\tG\tS4(1|1) \n"
          "12\tT\tTA\t\n"
          "15\tG\tT\tS2(0|1) S1(1|1) \n"),
         "Pos\tRef\tAlt\tSamples\n",
         None]
NAMES = ["S1", "S2", "S3", "S4", "S5"]


def test_helper_blocks_of_the_worked_example():
    """Dosages [[2 1 1 2 0] [0 0 0 2 0] [0 0 0 0 0] [2 1 0 0 0]], n = 5: Sx = 6, 2, 0, 3, Sxx = 10, 4, 0, 5, n Sxx - Sx^2 = 14, 16, 0, 16."""
    m = matrix(Parsed(TEXTS), NAMES)
    dot = block(m, "dot")
    assert dot.dtype == np.int32 and dot.tolist() == [[10, 4, 0, 5], [4, 4, 0, 0], [0, 0, 0, 0], [5, 0, 0, 5]]   # the diagonal is Sxx
    r2, zero = block_r2(m)
    assert r2.dtype == np.float32 and r2.shape == (4, 4) and np.array_equal(r2, block(m, "r2"))
    assert r2[0, 1] == np.float32(64.0 / (14.0 * 16.0))    # cov = 5 * 4 - 6 * 2 = 8
    assert r2[0, 3] == np.float32(49.0 / (14.0 * 16.0))    # cov = 5 * 5 - 6 * 3 = 7
    assert r2[1, 3] == np.float32(36.0 / (16.0 * 16.0))    # cov = 0 - 2 * 3 = -6
    assert np.array_equal(r2, r2.T)
    # the diagonal of a polymorphic row is exactly 1, the monomorphic row's 0 like its whole row and column
    assert np.diag(r2).tolist() == [1.0, 1.0, 0.0, 1.0]
    assert zero.tolist() == [[False, False, True, False], [False, False, True, False], [True] * 4, [False, False, True, False]]
    assert not r2[zero].any()
    # a row the duplicate rule dropped is a row of zero cells: it stays in the block as a row and a column of zeros
    with_dropped = np.insert(m, 1, 0, axis=0)
    d5 = block(with_dropped, "dot")
    assert d5.shape == (5, 5) and not d5[1].any() and not d5[:, 1].any() and np.array_equal(np.delete(np.delete(d5, 1, 0), 1, 1), dot)
    r5, z5 = block_r2(with_dropped)
    assert z5[1].all() and z5[:, 1].all() and np.array_equal(np.delete(np.delete(r5, 1, 0), 1, 1), r2)
    # n = 1: one column, every variance is 0
    one, z1 = block_r2(m[:, :1])
    assert z1.all() and not one.any() and block(m[:, :1], "dot").tolist() == [[4, 0, 0, 4], [0, 0, 0, 0], [0, 0, 0, 0], [4, 0, 0, 4]]
    # no rows
    assert block(m[:0], "dot").shape == (0, 0) and block(m[:0], "r2").shape == (0, 0)


def test_helper_batch_layout():
    m = matrix(Parsed(TEXTS), NAMES)
    bb = block_begin([4, 0, 1, 3])
    assert bb.dtype == np.uint64 and bb.tolist() == [0, 16, 16, 17, 26]
    flat, bb2 = blocks(m, [0, 4, 3, 1], [4, 0, 1, 3], "dot")   # overlapping ranges: each region its own block over the shared rows
    assert np.array_equal(bb, bb2) and flat.dtype == np.int32 and flat.shape == (26,)
    assert flat[:16].reshape(4, 4).tolist() == block(m, "dot").tolist()
    assert flat[16:17].tolist() == [5] and flat[17:].reshape(3, 3).tolist() == [[4, 0, 0], [0, 0, 0], [0, 0, 5]]
    assert block_begin([]).tolist() == [0] and block_begin([70_000]).tolist() == [0, 4_900_000_000]
    rf, _ = blocks(m, [0], [4], "r2")
    assert rf.dtype == np.float32 and np.array_equal(rf.reshape(4, 4), block(m, "r2"))


def test_helper_text():
    p = Parsed(TEXTS)
    m = matrix(p, NAMES)
    head = "Pos\tRef\tAlt\t10:A:C\t10:A:G\t12:T:TA\t15:G:T\n"
    assert ld_matrix_text(p, 0, m, "dot") == (head + "10\tA\tC\t10\t4\t0\t5\n" "10\tA\tG\t4\t4\t0\t0\n" "12\tT\tTA\t0\t0\t0\t0\n"
                                              "15\tG\tT\t5\t0\t0\t5\n")
    assert ld_matrix_text(p, 0, m, "r2") == (head + "10\tA\tC\t1\t0.285714\t0\t0.21875\n" "10\tA\tG\t0.285714\t1\t0\t0.140625\n"
                                             "12\tT\tTA\t0\t0\t0\t0\n" "15\tG\tT\t0.21875\t0.140625\t0\t1\n")
    assert ld_matrix_text(p, 1, m, "dot") == "Pos\tRef\tAlt\n" and ld_matrix_text(p, 1, m, "r2") == "Pos\tRef\tAlt\n"


def _call(vs, ids, n_ids, n=1, stat=R2):
    lib = _lib.load()
    regions = (_lib.Region * 1)(_lib.Region(1, 100))
    h = C.c_void_p()
    ptr = None if ids is None else (C.c_uint32 * max(len(ids), 1))(*ids)
    return lib.vs_query_ld_matrix(vs._h, regions, n, ptr, n_ids, stat, C.byref(h))


def test_entry_points_are_declared():
    lib = _lib.load()
    for name in ("vs_query_ld_matrix", "vs_result_get_ld_matrix", "vs_result_ld_matrix_device"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def test_host_only_handle_refuses_ld_matrix(host_store):
    for stat in (DOT, R2):
        assert _call(host_store, None, 0, stat=stat) == VS_ERR_NO_DEVICE
    assert _call(host_store, [1], 1) == VS_ERR_NO_DEVICE
    assert _call(host_store, [1, 1], 2) == VS_ERR_NO_DEVICE
    for kw in (dict(), dict(samples=[1]), dict(stat="dot"), dict(stat="R2")):
        with pytest.raises(VariantStoreError) as e:
            host_store.ld_matrix([(1, 100)], **kw)
        assert e.value.code == VS_ERR_NO_DEVICE, kw


def test_argument_errors_and_their_order(host_store):
    ns = host_store.info().num_samples
    err = lambda: _lib.load().vs_last_error().decode()
    # the band query's checks of the batch and the subset, in its order
    assert _call(host_store, [1], 1, n=0) == VS_ERR_ARG             # no regions
    assert "region" in err()
    assert _call(host_store, None, 3) == VS_ERR_ARG                 # NULL ids with n_ids set
    assert _call(host_store, [1], 0) == VS_ERR_ARG                  # an empty subset
    assert "subset" in err()
    for stat in (2, 7, 0xFFFFFFFF):
        assert _call(host_store, None, 0, stat=stat) == VS_ERR_ARG, stat
        assert "statistic" in err()
    # ... come before the ids are looked at, the ids before the device
    assert _call(host_store, [0], 1, stat=2) == VS_ERR_ARG
    assert _call(host_store, [ns], 1, stat=9) == VS_ERR_ARG
    assert _call(host_store, [0], 1) == VS_ERR_UNKNOWN_SAMPLE       # "ref"
    assert _call(host_store, [1, ns], 2) == VS_ERR_UNKNOWN_SAMPLE   # out of range
    assert _call(host_store, [1, 0xFFFFFFFF], 2) == VS_ERR_UNKNOWN_SAMPLE
    assert _call(host_store, [1], 1, stat=DOT) == VS_ERR_NO_DEVICE
    # a batch without regions is reported before a bad statistic, an empty subset before it too
    assert _call(host_store, None, 0, n=0, stat=5) == VS_ERR_ARG
    assert "region" in err()
    assert _call(host_store, [1], 0, stat=5) == VS_ERR_ARG
    assert "subset" in err()


def test_wrapper_stat_names_and_codes(host_store):
    assert QueryResult.LD_STATS == {"dot": 0, "r2": 1}
    ns = host_store.info().num_samples
    cases = ((dict(samples=[]), VS_ERR_ARG), (dict(samples=[0]), VS_ERR_UNKNOWN_SAMPLE), (dict(samples=[ns]), VS_ERR_UNKNOWN_SAMPLE),
             (dict(stat=2), VS_ERR_ARG), (dict(stat=-1), VS_ERR_ARG), (dict(stat=2, samples=[0]), VS_ERR_ARG))
    for kw, code in cases:
        with pytest.raises(VariantStoreError) as e:
            host_store.ld_matrix([(1, 100)], **kw)
        assert e.value.code == code, kw
    for name in ("r2", "R2", "dot", "Dot", 0, 1):   # the names and the ABI's numbers pass the wrapper: the device is what is missing
        with pytest.raises(VariantStoreError) as e:
            host_store.ld_matrix([(1, 100)], stat=name)
        assert e.value.code == VS_ERR_NO_DEVICE, name
    with pytest.raises(VariantStoreError):
        host_store.ld_matrix([(1, 100)], samples=["no-such-sample"])
    for bad in ("d-prime", "r", ""):
        with pytest.raises(ValueError):
            host_store.ld_matrix([(1, 100)], stat=bad)
    with pytest.raises(VariantStoreError) as e:
        host_store.ld_matrix([])
    assert e.value.code == VS_ERR_ARG


def test_cli_usage_errors(golden_dir, tmp_path):
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    subprocess.run([CLI, "construct", "-r", os.path.join(golden_dir, "x.small.fa"), "-v", os.path.join(golden_dir, "x.small.vcf"), "-p", prefix],
                   check=True, capture_output=True)
    p = subprocess.run([CLI, "ldmatrix", "-p", prefix], capture_output=True, text=True)   # no region: the usage
    assert p.returncode != 0 and "variantstore ldmatrix" in p.stdout and "--dot" in p.stdout
    p = subprocess.run([CLI, "ldmatrix", "-r", "1:100"], capture_output=True, text=True)   # no prefix
    assert p.returncode != 0 and "variantstore ldmatrix" in p.stdout
    p = subprocess.run([CLI, "ldmatrix", "-p", prefix, "-r", "1:100", "-w", "8"], capture_output=True, text=True)   # the band's flag
    assert p.returncode != 0 and "unknown option" in p.stdout + p.stderr
    p = subprocess.run([CLI, "ld", "-p", prefix], capture_output=True, text=True)   # `ld` still parses as it did
    assert p.returncode != 0 and "variantstore ld " in p.stdout and "--window" not in p.stderr
