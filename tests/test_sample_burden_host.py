"""Burden queries without a GPU: the argument checks of vs_query_sample_burden (made on the host, before the handle's device is
asked for), the host-only refusal, and the helper that derives the expected matrix from type-6 text."""
import ctypes as C
import os

import numpy as np
import pytest

from sample_burden_ref import HEADER, NO_MAX, burden_matrix, burden_text
from variantstore_amd import VariantStore, _lib
from variantstore_amd.api import VariantStoreError

VS_ERR_NO_DEVICE, VS_ERR_ARG, VS_ERR_UNKNOWN_SAMPLE = -3, -5, -6


@pytest.fixture(scope="module")
def host_store(golden_dir):
    vs = VariantStore.from_vcf(os.path.join(golden_dir, "x.small.fa"), os.path.join(golden_dir, "x.small.vcf"), device=-1)
    yield vs
    vs.close()


def _call(vs, ids, n_ids, n=1, min_ac=0, max_ac=NO_MAX):
    lib = _lib.load()
    regions = (_lib.Region * 1)(_lib.Region(1, 100))
    h = C.c_void_p()
    ptr = None if ids is None else (C.c_uint32 * max(len(ids), 1))(*ids)
    return lib.vs_query_sample_burden(vs._h, regions, n, ptr, n_ids, min_ac, max_ac, C.byref(h))


def test_host_only_handle_refuses_burden(host_store):
    assert _call(host_store, None, 0) == VS_ERR_NO_DEVICE
    assert _call(host_store, [1], 1) == VS_ERR_NO_DEVICE
    assert _call(host_store, [1, 1], 2, min_ac=1, max_ac=1) == VS_ERR_NO_DEVICE
    with pytest.raises(VariantStoreError) as e:
        host_store.sample_burden([(1, 100)])
    assert e.value.code == VS_ERR_NO_DEVICE
    with pytest.raises(VariantStoreError) as e:
        host_store.sample_burden([(1, 100)], samples=[1], min_ac=0, max_ac=3)
    assert e.value.code == VS_ERR_NO_DEVICE


def test_argument_errors(host_store):
    ns = host_store.info().num_samples
    assert _call(host_store, [1], 1, n=0) == VS_ERR_ARG             # no regions
    assert _call(host_store, None, 3) == VS_ERR_ARG                 # NULL ids with n_ids set
    assert _call(host_store, [1], 0) == VS_ERR_ARG                  # an empty subset
    assert _call(host_store, None, 0, min_ac=3, max_ac=2) == VS_ERR_ARG   # an empty window
    assert _call(host_store, [1], 1, min_ac=1, max_ac=0) == VS_ERR_ARG
    assert _call(host_store, [0], 1) == VS_ERR_UNKNOWN_SAMPLE       # "ref"
    assert _call(host_store, [1, ns], 2) == VS_ERR_UNKNOWN_SAMPLE   # out of range
    assert _call(host_store, [0], 1, min_ac=3, max_ac=2) == VS_ERR_ARG    # the window is checked before the ids
    # the Python wrapper raises with the same codes
    for kw, code in ((dict(samples=[]), VS_ERR_ARG), (dict(min_ac=2, max_ac=1), VS_ERR_ARG), (dict(samples=[0]), VS_ERR_UNKNOWN_SAMPLE),
                     (dict(samples=[ns]), VS_ERR_UNKNOWN_SAMPLE)):
        with pytest.raises(VariantStoreError) as e:
            host_store.sample_burden([(1, 100)], **kw)
        assert e.value.code == code, kw
    with pytest.raises(VariantStoreError):
        host_store.sample_burden([(1, 100)], samples=["no-such-sample"])
    with pytest.raises(VariantStoreError) as e:
        host_store.sample_burden([])
    assert e.value.code == VS_ERR_ARG


def test_cell_cap(host_store):
    # 2^31 + 1 regions declared over a one-region array: the cap is checked before anything reads the regions
    lib = _lib.load()
    assert _call(host_store, [1], 1, n=(1 << 31) + 1) == VS_ERR_ARG
    msg = lib.vs_last_error().decode()
    assert str((1 << 31) + 1) in msg and "2^31" in msg, msg
    assert _call(host_store, [1, 1], 2, n=(1 << 31) + 1) == VS_ERR_ARG    # duplicates collapse: still one column
    assert _call(host_store, [1], 1, n=1 << 31) == VS_ERR_NO_DEVICE       # exactly 2^31 cells pass the check
    ns = host_store.info().num_samples
    if ns > 2:
        assert _call(host_store, None, 0, n=(1 << 31) // (ns - 1) + 1) == VS_ERR_ARG
        assert _call(host_store, None, 0, n=(1 << 31) // (ns - 1)) == VS_ERR_NO_DEVICE


TEXTS = [("Pos\tRef\tAlt\tSamples\n"
          "10\tA\tC\tS1(1|1) S2(0/1) S3(1/0) S4(1|1) \n"     # 1|1, 0/1, a haploid 1 (gt_1 alone), S4's 1|2 call ...
          "10\tA\tG\tS4(1|1) \n"                             # ... on both of its ALT rows
          "12\tT\tTA\t\n"                                    # an empty row
          "15\tG\tT\tS2(0|1) \n"),
         "Pos\tRef\tAlt\tSamples\n",
         None]
NAMES = ["S1", "S2", "S3", "S4", "S5"]


def test_matrix_from_print_var_text():
    m = burden_matrix(TEXTS, NAMES)
    assert m.shape == (3, 5, 4)
    assert m[0].tolist() == [[1, 2, 1, 1], [2, 2, 0, 1], [1, 1, 0, 0], [2, 4, 2, 2], [0, 0, 0, 0]]
    assert not m[1].any() and not m[2].any()
    # a subset: the columns are its names, and a row's allele count is taken over them alone
    sub = burden_matrix(TEXTS, ["S2", "S4"])
    assert sub[0].tolist() == [[2, 2, 0, 1], [2, 4, 2, 2]]
    # windows: [2, max] drops the singleton row at 15; [0, 1] keeps it alone (and the empty row, which has no carriers)
    assert burden_matrix(TEXTS, NAMES, 2, NO_MAX)[0].tolist() == [[1, 2, 1, 1], [1, 1, 0, 0], [1, 1, 0, 0], [2, 4, 2, 2], [0, 0, 0, 0]]
    assert burden_matrix(TEXTS, NAMES, 0, 1)[0].tolist() == [[0, 0, 0, 0], [1, 1, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    # over {S2, S3} the first row has 2 alternate alleles, the last 1
    assert burden_matrix(TEXTS, ["S2", "S3"], 2, NO_MAX)[0].tolist() == [[1, 1, 0, 0], [1, 1, 0, 0]]
    assert burden_matrix(TEXTS, ["S2", "S3"], 0, 1)[0].tolist() == [[1, 1, 0, 1], [0, 0, 0, 0]]
    # a window no row's count lies in
    assert not burden_matrix(TEXTS, NAMES, 7, 9).any()
    assert not burden_matrix(TEXTS, ["S5"], 1, NO_MAX).any()


def test_text_from_matrix():
    m = burden_matrix(TEXTS, NAMES)
    assert burden_text(m[0], NAMES) == HEADER + "S1\t1\t2\t1\t1\nS2\t2\t2\t0\t1\nS3\t1\t1\t0\t0\nS4\t2\t4\t2\t2\n"
    assert burden_text(m[1], NAMES) == HEADER
    assert burden_text(np.zeros((0, 4), np.int64), []) == HEADER
