"""Allele-count queries without a GPU: argument checks of vs_query_allele_counts (made on the host, before the handle's
device is asked for), the host-only refusal, and the helper that derives expected counts from type-6 text."""
import ctypes as C
import os

import pytest

from allele_counts_ref import HEADER, count_rows, counts_text
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
    return lib.vs_query_allele_counts(vs._h, regions, n, ptr, n_ids, C.byref(h))


def test_host_only_handle_refuses_counts(host_store):
    assert _call(host_store, None, 0) == VS_ERR_NO_DEVICE
    assert _call(host_store, [1], 1) == VS_ERR_NO_DEVICE
    with pytest.raises(VariantStoreError) as e:
        host_store.allele_counts([(1, 100)])
    assert e.value.code == VS_ERR_NO_DEVICE


def test_argument_errors(host_store):
    ns = host_store.info().num_samples
    assert _call(host_store, None, 3) == VS_ERR_ARG                 # NULL ids with n_ids set
    assert _call(host_store, [1], 0) == VS_ERR_ARG                  # an empty subset
    assert _call(host_store, [0], 1) == VS_ERR_UNKNOWN_SAMPLE       # "ref"
    assert _call(host_store, [1, ns], 2) == VS_ERR_UNKNOWN_SAMPLE   # out of range
    assert _call(host_store, [1], 1, n=0) == VS_ERR_ARG             # no regions
    with pytest.raises(VariantStoreError) as e:
        host_store.allele_counts([(1, 100)], samples=["no-such-sample"])


def test_counts_from_print_var_text():
    # 1|1, 0/1, a haploid 1 (gt_1 alone), a 1|2 call (both gt bits set: the index's bits, not the allele indexes) on each ALT row
    text = ("Pos\tRef\tAlt\tSamples\n"
            "10\tA\tC\tS1(1|1) S2(0/1) S3(1/0) S4(1|1) \n"
            "10\tA\tG\tS4(1|1) \n"
            "12\tT\tTA\t\n")
    assert count_rows(text) == [(10, "A", "C", 4, 6, 2, 2), (10, "A", "G", 1, 2, 1, 1), (12, "T", "TA", 0, 0, 0, 0)]
    assert count_rows(text, {"S2", "S3"}) == [(10, "A", "C", 2, 2, 0, 0), (10, "A", "G", 0, 0, 0, 0), (12, "T", "TA", 0, 0, 0, 0)]
    assert count_rows(text, {"S4"})[0] == (10, "A", "C", 1, 2, 1, 1)
    assert counts_text(text, {"S1"}) == HEADER + "10\tA\tC\t1\t2\t1\t1\n10\tA\tG\t0\t0\t0\t0\n12\tT\tTA\t0\t0\t0\t0\n"
    assert counts_text("Pos\tRef\tAlt\tSamples\n") == HEADER
