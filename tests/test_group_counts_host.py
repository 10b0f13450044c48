"""Grouped allele counts without a GPU (vs_query_group_counts on a handle opened host-only): the argument checks in the order the
header states them, VS_ERR_NO_DEVICE for a valid call, the Python wrapper's unknown name, and the reference helper on a
hand-written type-6 text."""
import ctypes as C
import os

import numpy as np
import pytest

from group_counts_ref import HEADER, group_rows, groups_text, parse_region, parsed_groups_text
from variantstore_amd import VariantStore, _lib
from variantstore_amd.api import VariantStoreError

VS_ERR_NO_DEVICE, VS_ERR_ARG, VS_ERR_UNKNOWN_SAMPLE = -3, -5, -6


@pytest.fixture(scope="module")
def host_store(golden_dir):
    vs = VariantStore.from_vcf(os.path.join(golden_dir, "x.small.fa"), os.path.join(golden_dir, "x.small.vcf"), device=-1)
    yield vs
    vs.close()


def _call(vs, n=1, ids=(1,), gof=(0,), n_groups=1, names=None, n_ids=None, null_ids=False, null_gof=False):
    """vs_query_group_counts through ctypes: (code, message)."""
    lib = _lib.load()
    regions = (_lib.Region * max(n, 1))(*[_lib.Region(1, 100)] * max(n, 1))
    a = np.ascontiguousarray(ids, dtype=np.uint32)
    b = np.ascontiguousarray(gof, dtype=np.uint32)
    pa = None if null_ids else a.ctypes.data_as(C.POINTER(C.c_uint32))
    pb = None if null_gof else b.ctypes.data_as(C.POINTER(C.c_uint32))
    pn = (C.c_char_p * len(names))(*[s.encode() for s in names]) if names is not None else None
    h = C.c_void_p()
    rc = lib.vs_query_group_counts(vs._h, regions, n, pa, pb, len(a) if n_ids is None else n_ids, n_groups, pn, C.byref(h))
    assert rc != 0 and not h.value
    return rc, lib.vs_last_error().decode()


def test_argument_errors_in_the_stated_order(host_store):
    vs = host_store
    ns = vs.info().num_samples
    assert ns == 2                                                          # x.small: "ref" and one sample, id 1
    # 1. the plain argument errors
    assert _call(vs, n=0)[0] == VS_ERR_ARG
    assert _call(vs, null_ids=True)[0] == VS_ERR_ARG
    assert _call(vs, null_gof=True)[0] == VS_ERR_ARG
    assert _call(vs, n_ids=0)[0] == VS_ERR_ARG
    assert _call(vs, n_groups=0)[0] == VS_ERR_ARG
    assert _call(vs, n_groups=65)[0] == VS_ERR_ARG
    assert _call(vs, ids=(ns + 5,), n_groups=65)[0] == VS_ERR_ARG          # before the unknown sample
    # 2. a group out of range -- before an unknown sample
    assert _call(vs, ids=(1, 1), gof=(0, 2), n_groups=2)[0] == VS_ERR_ARG
    assert _call(vs, ids=(ns + 5, 1), gof=(0, 2), n_groups=2)[0] == VS_ERR_ARG
    assert _call(vs, ids=(0, 1), gof=(0, 7), n_groups=2)[0] == VS_ERR_ARG
    # 3. "ref" or an id beyond the cohort -- before a conflicting membership
    assert _call(vs, ids=(0,), gof=(0,))[0] == VS_ERR_UNKNOWN_SAMPLE
    assert _call(vs, ids=(ns,), gof=(0,))[0] == VS_ERR_UNKNOWN_SAMPLE
    assert _call(vs, ids=(1, 1, ns), gof=(0, 1, 0), n_groups=2)[0] == VS_ERR_UNKNOWN_SAMPLE
    # 4. a sample in two groups: the message names the sample and both groups
    rc, msg = _call(vs, ids=(1, 1, 1), gof=(1, 1, 4), n_groups=5)
    assert rc == VS_ERR_ARG and "sample id 1" in msg and "group 1" in msg and "group 4" in msg
    # a name with a tab or a newline
    assert _call(vs, names=["a\tb"])[0] == VS_ERR_ARG
    assert _call(vs, ids=(1, 1), gof=(0, 0), n_groups=2, names=["ok", "two\nlines"])[0] == VS_ERR_ARG


def test_valid_call_on_a_host_only_handle_has_no_device(host_store):
    vs = host_store
    assert _call(vs, ids=(1, 1), gof=(63, 63), n_groups=64)[0] == VS_ERR_NO_DEVICE      # a duplicate pair, empty groups
    assert _call(vs, ids=(1,), gof=(1,), n_groups=2, names=["cases", "controls"])[0] == VS_ERR_NO_DEVICE
    with pytest.raises(VariantStoreError) as e:
        vs.group_counts([(1, 100)], {"a": [1], "b": []})
    assert e.value.code == VS_ERR_NO_DEVICE
    with pytest.raises(VariantStoreError) as e:
        vs.group_counts([(1, 100)], [[1], [1]])
    assert e.value.code == VS_ERR_ARG


def test_python_wrapper_raises_for_an_unknown_name(host_store):
    vs = host_store
    with pytest.raises(VariantStoreError) as a:
        vs.allele_counts([(1, 100)], ["nobody-of-that-name"])
    with pytest.raises(VariantStoreError) as g:
        vs.group_counts([(1, 100)], {"a": [vs.sample_name(1)], "b": ["nobody-of-that-name"]})
    assert type(g.value) is type(a.value) and g.value.code == a.value.code


def test_reference_helper_on_a_hand_written_text():
    text = ("Pos\tRef\tAlt\tSamples\n"
            "10\tA\tC\tS1(1|1) S2(0/1) S3(1/0) \n"         # hom phased, two unphased hets
            "20\tG\tT\tS4(1|0) \n"                          # a haploid `1` is stored as gt_1 alone: prints 1|0
            "30\tC\tA\tS1(1|1) S5(1|0) \n"                  # a `1|2` call shows with both bits on both ALT rows
            "30\tC\tG\tS1(1|1) \n"
            "40\tT\tG\t\n")                                 # a row with no carriers
    group_of = {"S1": 0, "S2": 0, "S3": 2, "S4": 2, "S9": 2}   # group 1 empty, S5 unlisted, S9 carries nothing
    rows = group_rows(text, group_of, 3)
    assert rows == [(10, "A", "C", [(2, 3, 1, 1), (0, 0, 0, 0), (1, 1, 0, 0)]),
                    (20, "G", "T", [(0, 0, 0, 0), (0, 0, 0, 0), (1, 1, 0, 1)]),
                    (30, "C", "A", [(1, 2, 1, 1), (0, 0, 0, 0), (0, 0, 0, 0)]),
                    (30, "C", "G", [(1, 2, 1, 1), (0, 0, 0, 0), (0, 0, 0, 0)]),
                    (40, "T", "G", [(0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)])]
    got = groups_text(text, group_of, 3, ["cases", "none", "controls"])
    lines = got.split("\n")
    assert got.startswith(HEADER) and len(lines) == 1 + 5 * 3 + 1
    assert lines[1] == "10\tA\tC\tcases\t2\t2\t3\t1\t1"
    assert lines[2] == "10\tA\tC\tnone\t0\t0\t0\t0\t0"
    assert lines[3] == "10\tA\tC\tcontrols\t3\t1\t1\t0\t0"
    assert groups_text(text, group_of, 3).split("\n")[3] == "10\tA\tC\t2\t3\t1\t1\t0\t0"
    assert groups_text("Pos\tRef\tAlt\tSamples\n", group_of, 3) == HEADER
    # the one-pass form the large cohorts are checked with gives the same text
    ids_of = {f"S{i}": i for i in range(1, 10)}
    label = np.full(10, -1)
    for name, g in group_of.items():
        label[ids_of[name]] = g
    for names in (None, ["cases", "none", "controls"]):
        assert parsed_groups_text(parse_region(text, ids_of), label, 3, names) == groups_text(text, group_of, 3, names)
    assert parsed_groups_text(parse_region("Pos\tRef\tAlt\tSamples\n", ids_of), label, 3) == HEADER
