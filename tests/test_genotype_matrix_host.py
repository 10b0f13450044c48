"""Genotype-matrix queries without a GPU: the argument checks of vs_query_genotype_matrix (made on the host, before the handle's
device is asked for), the host-only refusal, and the helper that derives the expected matrix and text from type-6 text."""
import ctypes as C
import os

import numpy as np
import pytest

from genotype_matrix_ref import Parsed, call_text, cell, matrix, matrix_sparse, matrix_text
from variantstore_amd import VariantStore, _lib
from variantstore_amd.api import VariantStoreError

VS_ERR_NO_DEVICE, VS_ERR_ARG, VS_ERR_UNKNOWN_SAMPLE = -3, -5, -6


@pytest.fixture(scope="module")
def host_store(golden_dir):
    vs = VariantStore.from_vcf(os.path.join(golden_dir, "x.small.fa"), os.path.join(golden_dir, "x.small.vcf"), device=-1)
    yield vs
    vs.close()


def _call(vs, ids, n_ids, n=1):
    lib = _lib.load()
    regions = (_lib.Region * 1)(_lib.Region(1, 100))
    h = C.c_void_p()
    ptr = None if ids is None else (C.c_uint32 * max(len(ids), 1))(*ids)
    return lib.vs_query_genotype_matrix(vs._h, regions, n, ptr, n_ids, C.byref(h))


def test_host_only_handle_refuses_matrix(host_store):
    assert _call(host_store, None, 0) == VS_ERR_NO_DEVICE
    assert _call(host_store, [1], 1) == VS_ERR_NO_DEVICE
    assert _call(host_store, [1, 1], 2) == VS_ERR_NO_DEVICE
    with pytest.raises(VariantStoreError) as e:
        host_store.genotype_matrix([(1, 100)])
    assert e.value.code == VS_ERR_NO_DEVICE
    with pytest.raises(VariantStoreError) as e:
        host_store.genotype_matrix([(1, 100)], samples=[1])
    assert e.value.code == VS_ERR_NO_DEVICE


def test_argument_errors(host_store):
    ns = host_store.info().num_samples
    assert _call(host_store, [1], 1, n=0) == VS_ERR_ARG             # no regions
    assert _call(host_store, None, 3) == VS_ERR_ARG                 # NULL ids with n_ids set
    assert _call(host_store, [1], 0) == VS_ERR_ARG                  # an empty subset
    assert _call(host_store, [0], 1) == VS_ERR_UNKNOWN_SAMPLE       # "ref"
    assert _call(host_store, [1, ns], 2) == VS_ERR_UNKNOWN_SAMPLE   # out of range
    assert _call(host_store, [1, 0xFFFFFFFF], 2) == VS_ERR_UNKNOWN_SAMPLE
    # the Python wrapper raises with the same codes
    for kw, code in ((dict(samples=[]), VS_ERR_ARG), (dict(samples=[0]), VS_ERR_UNKNOWN_SAMPLE), (dict(samples=[ns]), VS_ERR_UNKNOWN_SAMPLE)):
        with pytest.raises(VariantStoreError) as e:
            host_store.genotype_matrix([(1, 100)], **kw)
        assert e.value.code == code, kw
    with pytest.raises(VariantStoreError):
        host_store.genotype_matrix([(1, 100)], samples=["no-such-sample"])
    with pytest.raises(VariantStoreError) as e:
        host_store.genotype_matrix([])
    assert e.value.code == VS_ERR_ARG


def test_options(host_store):
    for key, bad in (("matrix_tile_cols", (8, 17, 65552, -16)), ("matrix_max_mib", (-1,))):
        for v in bad:
            with pytest.raises(VariantStoreError) as e:
                host_store.set_option(key, v)
            assert e.value.code == VS_ERR_ARG, (key, v)
    for key, good in (("matrix_tile_cols", (16, 4096, 65536, 0)), ("matrix_max_mib", (1, 1 << 20, 0))):
        for v in good:
            host_store.set_option(key, v)


TEXTS = [("Pos\tRef\tAlt\tSamples\n"
          "10\tA\tC\tS1(1|1) S2(0/1) S3(1/0) S4(1|1) \n"     # 1|1, 0/1, a haploid 1 (gt_1 alone), S4's 1|2 call ...
          "10\tA\tG\tS4(1|1) \n"                             # ... on both of its ALT rows
          "12\tT\tTA\t\n"                                    # an empty row
          "15\tG\tT\tS2(0|1) \n"),
         "Pos\tRef\tAlt\tSamples\n",
         None]
NAMES = ["S1", "S2", "S3", "S4", "S5"]   # nobody carries S5's column


def test_cell_bytes():
    assert cell(1, 1, True) == 0x0F and cell(0, 1, False) == 0x0C and cell(1, 0, False) == 0x0A and cell(0, 1, True) == 0x0D
    assert [call_text(v) for v in (0, 0x0F, 0x0C, 0x0A, 0x0D, 0x0E)] == ["0", "1|1", "0/1", "1/0", "0|1", "1/1"]
    for v in (0x0F, 0x0C, 0x0A, 0x0D):
        assert bin(v & 6).count("1") == int(call_text(v)[0]) + int(call_text(v)[2])   # the dosage


def test_matrix_from_print_var_text():
    p = Parsed(TEXTS)
    assert p.n_rows == 4 and p.row_begin.tolist() == [0, 4, 4] and p.row_count.tolist() == [4, 0, 0]
    m = matrix(p, NAMES)
    assert m.dtype == np.uint8 and m.shape == (4, 5)
    assert m.tolist() == [[0x0F, 0x0C, 0x0A, 0x0F, 0], [0, 0, 0, 0x0F, 0], [0, 0, 0, 0, 0], [0, 0x0D, 0, 0, 0]]
    assert np.array_equal(m, matrix(TEXTS, NAMES))
    # a subset: its names are the columns
    sub = matrix(p, ["S2", "S4"])
    assert sub.tolist() == [[0x0C, 0x0F], [0, 0x0F], [0, 0], [0x0D, 0]]
    assert not matrix(p, ["S5"]).any()
    row, col, val = matrix_sparse(p, NAMES)
    assert row.tolist() == [0, 0, 0, 0, 1, 3] and col.tolist() == [0, 1, 2, 3, 3, 1]
    assert val.tolist() == [0x0F, 0x0C, 0x0A, 0x0F, 0x0F, 0x0D]
    empty = Parsed([None, "Pos\tRef\tAlt\tSamples\n"])
    assert empty.n_rows == 0 and matrix(empty, NAMES).shape == (0, 5)


def test_text_from_matrix():
    p = Parsed(TEXTS)
    m = matrix(p, NAMES)
    head = "Pos\tRef\tAlt\tS1\tS2\tS3\tS4\tS5\n"
    assert matrix_text(p, 0, m, NAMES) == (head + "10\tA\tC\t1|1\t0/1\t1/0\t1|1\t0\n" "10\tA\tG\t0\t0\t0\t1|1\t0\n"
                                           "12\tT\tTA\t0\t0\t0\t0\t0\n" "15\tG\tT\t0\t0|1\t0\t0\t0\n")
    assert matrix_text(p, 1, m, NAMES) == head
    sub = matrix(p, ["S2", "S4"])
    assert matrix_text(p, 0, sub, ["S2", "S4"]) == ("Pos\tRef\tAlt\tS2\tS4\n" "10\tA\tC\t0/1\t1|1\n" "10\tA\tG\t0\t1|1\n"
                                                     "12\tT\tTA\t0\t0\n" "15\tG\tT\t0|1\t0\n")
