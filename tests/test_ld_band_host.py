"""Banded LD queries without a GPU: the argument checks of vs_query_ld_band (made on the host, before the handle's device is asked
for), the host-only refusal, the Python wrapper's codes, and the helper that derives the expected band and text from a genotype
matrix."""
import ctypes as C
import os

import numpy as np
import pytest

from genotype_matrix_ref import Parsed, matrix
from ld_band_ref import dosage, dot_band, format_value, gram, ld_text, moments, pair_values, r2_band, r2_values
from variantstore_amd import VariantStore, _lib
from variantstore_amd.api import VariantStoreError

VS_ERR_NO_DEVICE, VS_ERR_ARG, VS_ERR_UNKNOWN_SAMPLE = -3, -5, -6
DOT, R2 = 0, 1


@pytest.fixture(scope="module")
def host_store(golden_dir):
    vs = VariantStore.from_vcf(os.path.join(golden_dir, "x.small.fa"), os.path.join(golden_dir, "x.small.vcf"), device=-1)
    yield vs
    vs.close()


def _call(vs, ids, n_ids, n=1, window=64, stat=R2):
    lib = _lib.load()
    regions = (_lib.Region * 1)(_lib.Region(1, 100))
    h = C.c_void_p()
    ptr = None if ids is None else (C.c_uint32 * max(len(ids), 1))(*ids)
    return lib.vs_query_ld_band(vs._h, regions, n, ptr, n_ids, window, stat, C.byref(h))


def test_entry_points_are_declared():
    lib = _lib.load()
    for name in ("vs_query_ld_band", "vs_result_get_ld_band", "vs_result_ld_band_device"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def test_host_only_handle_refuses_ld(host_store):
    for stat in (DOT, R2):
        for window in (1, 64, 256):
            assert _call(host_store, None, 0, window=window, stat=stat) == VS_ERR_NO_DEVICE
    assert _call(host_store, [1], 1) == VS_ERR_NO_DEVICE
    assert _call(host_store, [1, 1], 2) == VS_ERR_NO_DEVICE
    for kw in (dict(), dict(samples=[1]), dict(window=1, stat="dot"), dict(window=256, stat="R2")):
        with pytest.raises(VariantStoreError) as e:
            host_store.ld_band([(1, 100)], **kw)
        assert e.value.code == VS_ERR_NO_DEVICE, kw


def test_argument_errors_and_their_order(host_store):
    ns = host_store.info().num_samples
    # the matrix query's checks of the batch and the subset
    assert _call(host_store, [1], 1, n=0) == VS_ERR_ARG             # no regions
    assert _call(host_store, None, 3) == VS_ERR_ARG                 # NULL ids with n_ids set
    assert _call(host_store, [1], 0) == VS_ERR_ARG                  # an empty subset
    # the window and the statistic
    for window in (0, 257, 0xFFFFFFFF):
        assert _call(host_store, None, 0, window=window) == VS_ERR_ARG, window
        assert "window" in _lib.load().vs_last_error().decode()
    for stat in (2, 7, 0xFFFFFFFF):
        assert _call(host_store, None, 0, stat=stat) == VS_ERR_ARG, stat
        assert "statistic" in _lib.load().vs_last_error().decode()
    # ... come before the ids are looked at, the ids before the device
    assert _call(host_store, [0], 1, window=0) == VS_ERR_ARG
    assert _call(host_store, [ns], 1, window=257) == VS_ERR_ARG
    assert _call(host_store, [0], 1, stat=2) == VS_ERR_ARG
    assert _call(host_store, [0], 1) == VS_ERR_UNKNOWN_SAMPLE       # "ref"
    assert _call(host_store, [1, ns], 2) == VS_ERR_UNKNOWN_SAMPLE   # out of range
    assert _call(host_store, [1, 0xFFFFFFFF], 2) == VS_ERR_UNKNOWN_SAMPLE
    assert _call(host_store, [1], 1, window=256, stat=DOT) == VS_ERR_NO_DEVICE
    # a batch without regions is reported before a bad window
    assert _call(host_store, None, 0, n=0, window=0) == VS_ERR_ARG
    assert "region" in _lib.load().vs_last_error().decode()


def test_wrapper_raises_the_same_codes(host_store):
    ns = host_store.info().num_samples
    cases = ((dict(samples=[]), VS_ERR_ARG), (dict(samples=[0]), VS_ERR_UNKNOWN_SAMPLE), (dict(samples=[ns]), VS_ERR_UNKNOWN_SAMPLE),
             (dict(window=0), VS_ERR_ARG), (dict(window=257), VS_ERR_ARG), (dict(window=-1), VS_ERR_ARG), (dict(window=1 << 32), VS_ERR_ARG),
             (dict(stat=2), VS_ERR_ARG), (dict(window=0, samples=[0]), VS_ERR_ARG))
    for kw, code in cases:
        with pytest.raises(VariantStoreError) as e:
            host_store.ld_band([(1, 100)], **kw)
        assert e.value.code == code, kw
    with pytest.raises(VariantStoreError):
        host_store.ld_band([(1, 100)], samples=["no-such-sample"])
    with pytest.raises(ValueError):
        host_store.ld_band([(1, 100)], stat="d-prime")
    with pytest.raises(VariantStoreError) as e:
        host_store.ld_band([])
    assert e.value.code == VS_ERR_ARG


# S4 has a 1|2 call (a carrier of both ALT rows at 10), S3 a haploid 1 (gt_1 alone); the row at 12 has no carrier
TEXTS = [("Pos\tRef\tAlt\tSamples\n"
          "10\tA\tC\tS1(1|1) S2(0/1) S3(1/0) S4(1|1) \n"
          "10\tA\tG\tS4(1|1) \n"
          "12\tT\tTA\t\n"
          "15\tG\tT\tS2(0|1) S1(1|1) \n"),
         "Pos\tRef\tAlt\tSamples\n",
         None]
NAMES = ["S1", "S2", "S3", "S4", "S5"]


def test_helper_dosages_and_dot_band():
    m = matrix(Parsed(TEXTS), NAMES)
    d = dosage(m)
    assert d.dtype == np.int64 and d.tolist() == [[2, 1, 1, 2, 0], [0, 0, 0, 2, 0], [0, 0, 0, 0, 0], [2, 1, 0, 0, 0]]
    g = gram(m)
    assert g.dtype == np.int64 and g.tolist() == [[10, 4, 0, 5], [4, 4, 0, 0], [0, 0, 0, 0], [5, 0, 0, 5]]
    sx, sxx = moments(m)
    assert sx.tolist() == [6, 2, 0, 3] and sxx.tolist() == [10, 4, 0, 5]
    for w, want in ((1, [[4], [0], [0], [0]]), (2, [[4, 0], [0, 0], [0, 0], [0, 0]]),
                    (3, [[4, 0, 5], [0, 0, 0], [0, 0, 0], [0, 0, 0]]), (5, [[4, 0, 5, 0, 0]] + [[0] * 5] * 3)):
        b = dot_band(m, w)
        assert b.dtype == np.int32 and b.tolist() == want, w
    assert pair_values(m, [0, 0, 1], [1, 3, 3], "dot").tolist() == [4, 5, 0]
    assert dot_band(m[:0], 4).shape == (0, 4) and dot_band(m[:1], 4).tolist() == [[0, 0, 0, 0]]


def test_helper_r2():
    m = matrix(Parsed(TEXTS), NAMES)
    n = 5
    r2, zero = r2_band(m, 3)
    assert r2.dtype == np.float32 and r2.shape == (4, 3)
    # rows 0 and 1: cov = 5 * 4 - 6 * 2 = 8, vx = 5 * 10 - 36 = 14, vy = 5 * 4 - 4 = 16
    assert r2[0, 0] == np.float32(64.0 / (14.0 * 16.0))
    # rows 0 and 3: cov = 5 * 5 - 6 * 3 = 7, vy = 5 * 5 - 9 = 16
    assert r2[0, 2] == np.float32(49.0 / (14.0 * 16.0))
    # rows 1 and 3: cov = 0 - 2 * 3 = -6
    assert r2[1, 1] == np.float32(36.0 / (16.0 * 16.0))
    # the empty row is monomorphic: every pair with it is exactly 0, and so is everything past the table's end
    assert zero.tolist() == [[False, True, False], [True, False, True], [True, True, True], [True, True, True]]
    assert not r2[zero].any()
    assert np.array_equal(pair_values(m, [0, 0, 1, 2], [1, 3, 3, 3], "r2"), np.asarray([r2[0, 0], r2[0, 2], r2[1, 1], 0], np.float32))
    # n = 1: one column, every variance is 0
    one, z1 = r2_band(m[:, :1], 2)
    assert z1.all() and not one.any()
    # a perfectly correlated pair
    v, flat = r2_values([4], [2], [4], [2], [4], 3)
    assert v.tolist() == [1.0] and not flat.any()
    assert n == m.shape[1]


def test_helper_text():
    p = Parsed(TEXTS)
    m = matrix(p, NAMES)
    hd, hr = "PosA\tRefA\tAltA\tPosB\tRefB\tAltB\tDot\n", "PosA\tRefA\tAltA\tPosB\tRefB\tAltB\tR2\n"
    assert ld_text(p, 0, m, 1, "dot") == hd + "10\tA\tC\t10\tA\tG\t4\n" "10\tA\tG\t12\tT\tTA\t0\n" "12\tT\tTA\t15\tG\tT\t0\n"
    assert ld_text(p, 0, m, 3, "dot") == (hd + "10\tA\tC\t10\tA\tG\t4\n" "10\tA\tC\t12\tT\tTA\t0\n" "10\tA\tC\t15\tG\tT\t5\n"
                                          "10\tA\tG\t12\tT\tTA\t0\n" "10\tA\tG\t15\tG\tT\t0\n" "12\tT\tTA\t15\tG\tT\t0\n")
    assert ld_text(p, 0, m, 2, "r2") == (hr + "10\tA\tC\t10\tA\tG\t0.285714\n" "10\tA\tC\t12\tT\tTA\t0\n"
                                         "10\tA\tG\t12\tT\tTA\t0\n" "10\tA\tG\t15\tG\tT\t0.140625\n" "12\tT\tTA\t15\tG\tT\t0\n")
    assert ld_text(p, 1, m, 64, "dot") == hd and ld_text(p, 1, m, 64, "r2") == hr
    # a dropped row between reference rows 1 and 2 of the table moves the later rows one further away
    assert ld_text(p, 0, m, 1, "dot", table_index=[0, 1, 3, 4]) == hd + "10\tA\tC\t10\tA\tG\t4\n" "12\tT\tTA\t15\tG\tT\t0\n"
    assert format_value(np.float32(1.0), "r2") == "1" and format_value(np.int32(-3), "dot") == "-3"
