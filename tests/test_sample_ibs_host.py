"""Pairwise IBS queries without a GPU: the reference that derives the expected matrices from a genotype matrix -- its two forms
against each other and against a hand-worked example --, the argument checks of vs_query_sample_ibs (made on the host, before the
handle's device is asked for) and their order, the host-only refusal, the Python wrapper's codes and the CLI's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from sample_ibs_ref import ibs_text, king, sample_ibs
from variantstore_amd import VariantStore, _lib
from variantstore_amd.api import VariantStoreError

VS_ERR_NO_DEVICE, VS_ERR_ARG, VS_ERR_UNKNOWN_SAMPLE = -3, -5, -6
COUNTS, KING = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")


@pytest.fixture(scope="module")
def host_store(golden_dir):
    vs = VariantStore.from_vcf(os.path.join(golden_dir, "x.small.fa"), os.path.join(golden_dir, "x.small.vcf"), device=-1)
    yield vs
    vs.close()


def _call(vs, ids, n_ids, n=1, stat=COUNTS):
    lib = _lib.load()
    regions = (_lib.Region * 1)(_lib.Region(1, 100))
    h = C.c_void_p()
    ptr = None if ids is None else (C.c_uint32 * max(len(ids), 1))(*ids)
    return lib.vs_query_sample_ibs(vs._h, regions, n, ptr, n_ids, stat, C.byref(h))


# cells: 2 = gt_1 alone (dosage 1), 4 = gt_2 alone (dosage 1), 6 / 7 = both (dosage 2), 0 = not a carrier.  Samples A B C D:
#   row 0   dosages 1 1 0 2
#   row 1   dosages 0 0 0 0   nobody carries it: a site all the same, IBS2 for every pair
#   row 2   dosages 2 2 2 2   everybody 1/1
#   row 3   dropped by the duplicate rule: no site
#   row 4   dosages 1 0 2 0
#   row 5   dosages 2 1 0 0
# C and D are never heterozygous: nh_C + nh_D == 0.
HAND = np.asarray([[2, 4, 0, 7], [0, 0, 0, 0], [7, 6, 7, 6], [0, 0, 0, 0], [4, 0, 6, 0], [7, 2, 0, 0]], np.uint8)
HAND_DROPPED = np.asarray([0, 0, 0, 1, 0, 0], bool)


def test_reference_against_a_hand_worked_example():
    w = sample_ibs(HAND, HAND_DROPPED)
    assert w["n_used"] == 5 and all(w[k].dtype == np.int64 and w[k].shape == (4, 4) for k in ("het_het", "hom_hom", "carrier_both", "ibs0", "ibs1", "ibs2"))
    # het: A in rows 0, 4; B in rows 0, 5.  hom-alt: A 2, 5; B 2; C 2, 4; D 0, 2.  carriers: A 0, 2, 4, 5; B 0, 2, 5; C 2, 4; D 0, 2
    assert w["het_het"].tolist() == [[2, 1, 0, 0], [1, 2, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert w["hom_hom"].tolist() == [[2, 1, 1, 1], [1, 1, 1, 1], [1, 1, 2, 1], [1, 1, 1, 2]]
    assert w["carrier_both"].tolist() == [[4, 3, 2, 2], [3, 3, 1, 2], [2, 1, 2, 1], [2, 2, 1, 2]]
    # opposite homozygotes: A-C row 5, A-D row 0, B-C row 4, C-D rows 0 and 4
    assert w["ibs0"].tolist() == [[0, 0, 1, 1], [0, 0, 1, 0], [1, 1, 0, 2], [1, 0, 2, 0]]
    # equal dosage: rows 1 and 2 for every pair; A-B row 0 too, B-D row 4, C-D row 5
    assert w["ibs2"].tolist() == [[5, 3, 2, 2], [3, 5, 2, 3], [2, 2, 5, 3], [2, 3, 3, 5]]
    assert w["ibs1"].tolist() == [[0, 2, 2, 2], [2, 0, 2, 2], [2, 2, 0, 0], [2, 2, 0, 0]]
    k = king(w["het_het"], w["ibs0"])
    assert k.dtype == np.float64
    # (het_het - 2 ibs0) / (nh_i + nh_j), nh = 2 2 0 0
    assert k.tolist() == [[0.5, 0.25, -1.0, -1.0], [0.25, 0.5, -1.0, 0.0], [-1.0, -1.0, 0.0, 0.0], [-1.0, 0.0, 0.0, 0.0]]
    assert not np.signbit(k[2:, 2:]).any(), "0.0, not -0.0, where the denominator is 0 (C-D: the numerator is -4)"
    # without the mask the dropped row would be a site nobody carries: IBS2 and n_used one larger, nothing else moves
    w6 = sample_ibs(HAND)
    assert w6["n_used"] == 6 and np.array_equal(w6["ibs2"], w["ibs2"] + 1) and np.array_equal(w6["ibs0"], w["ibs0"])
    assert np.array_equal(w6["het_het"], w["het_het"]) and np.array_equal(w6["ibs1"], w["ibs1"])
    # a dropped row with a set cell is a contradiction
    with pytest.raises(AssertionError):
        sample_ibs(HAND, np.asarray([1, 0, 0, 0, 0, 0], bool))
    # n = 1 and an empty table
    w1 = sample_ibs(HAND[:, :1], HAND_DROPPED)
    assert (w1["het_het"].tolist(), w1["hom_hom"].tolist(), w1["ibs0"].tolist(), w1["ibs2"].tolist()) == ([[2]], [[2]], [[0]], [[5]])
    we = sample_ibs(HAND[:0])
    assert we["n_used"] == 0 and all(we[f].shape == (4, 4) and not we[f].any() for f in ("het_het", "hom_hom", "carrier_both", "ibs0", "ibs1", "ibs2"))
    assert not king(we["het_het"], we["ibs0"]).any()
    # the pair table
    w["king"] = k
    names = ["A", "B", "C", "D"]
    assert ibs_text(names, w, "counts") == ("ID1\tID2\tN\tHetHet\tIBS0\tIBS1\tIBS2\n"
                                            "A\tB\t5\t1\t0\t2\t3\nA\tC\t5\t0\t1\t2\t2\nA\tD\t5\t0\t1\t2\t2\n"
                                            "B\tC\t5\t0\t1\t2\t2\nB\tD\t5\t0\t0\t2\t3\nC\tD\t5\t0\t2\t0\t3\n")
    assert ibs_text(names, w, "king").split("\n")[:2] == ["ID1\tID2\tN\tHetHet\tIBS0\tIBS1\tIBS2\tKinship", "A\tB\t5\t1\t0\t2\t3\t0.25"]
    assert ibs_text(names, w, "counts", min_kinship=0.0) == ("ID1\tID2\tN\tHetHet\tIBS0\tIBS1\tIBS2\tKinship\n"
                                                            "A\tB\t5\t1\t0\t2\t3\t0.25\nB\tD\t5\t0\t0\t2\t3\t0\nC\tD\t5\t0\t2\t0\t3\t0\n")
    assert ibs_text(names[:1], w, "king") == "ID1\tID2\tN\tHetHet\tIBS0\tIBS1\tIBS2\tKinship\n"


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_two_forms_agree_on_random_matrices(seed):
    """sample_ibs asserts its indicator-product form against the brute-force count of the nine state pairs; here on random cells of
    every storage pattern, with dropped rows, and the invariants that follow."""
    rng = np.random.default_rng(seed)
    n = (23, 64, 7)[seed - 1]
    m = rng.choice(np.asarray([0, 2, 4, 6, 7, 3, 5], np.uint8), size=(300, n), p=[0.5, 0.12, 0.12, 0.1, 0.1, 0.03, 0.03])
    dropped = rng.random(300) < 0.05
    m[dropped] = 0
    w = sample_ibs(m, dropped)
    assert w["n_used"] == 300 - int(dropped.sum()) and dropped.any()
    for f in ("het_het", "hom_hom", "carrier_both", "ibs0", "ibs1", "ibs2"):
        assert np.array_equal(w[f], w[f].T) and (w[f] >= 0).all(), f
    assert np.array_equal(w["ibs0"] + w["ibs1"] + w["ibs2"], np.full((n, n), w["n_used"]))
    assert not np.diagonal(w["ibs0"]).any() and (np.diagonal(w["ibs2"]) == w["n_used"]).all()
    assert w["ibs0"].any() and w["het_het"].any() and w["hom_hom"].any()
    k = king(w["het_het"], w["ibs0"])
    assert np.array_equal(k, k.T) and (np.diagonal(k)[np.diagonal(w["het_het"]) > 0] == 0.5).all() and (k <= 0.5).all()


def test_entry_points_are_declared():
    lib = _lib.load()
    for name in ("vs_query_sample_ibs", "vs_result_get_sample_ibs", "vs_result_sample_ibs_device"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def test_host_only_handle_refuses_ibs(host_store):
    for stat in (COUNTS, KING):
        assert _call(host_store, None, 0, stat=stat) == VS_ERR_NO_DEVICE
        assert _call(host_store, [1], 1, stat=stat) == VS_ERR_NO_DEVICE
        assert _call(host_store, [1, 1], 2, stat=stat) == VS_ERR_NO_DEVICE
    for kw in (dict(), dict(samples=[1]), dict(stat="king"), dict(stat="COUNTS", samples=[1, 1])):
        with pytest.raises(VariantStoreError) as e:
            host_store.sample_ibs([(1, 100)], **kw)
        assert e.value.code == VS_ERR_NO_DEVICE, kw


def test_argument_errors_and_their_order(host_store):
    ns = host_store.info().num_samples
    err = lambda: _lib.load().vs_last_error().decode()
    # the matrix query's checks of the batch and the subset
    assert _call(host_store, [1], 1, n=0) == VS_ERR_ARG             # no regions
    assert "region" in err()
    assert _call(host_store, None, 3) == VS_ERR_ARG                 # NULL ids with n_ids set
    assert _call(host_store, [1], 0) == VS_ERR_ARG                  # an empty subset
    # the statistic
    for stat in (2, 7, 0xFFFFFFFF):
        assert _call(host_store, None, 0, stat=stat) == VS_ERR_ARG, stat
        assert "statistic" in err()
    # ... comes before the ids are looked at, the ids before the device
    assert _call(host_store, [0], 1, stat=2) == VS_ERR_ARG
    assert _call(host_store, [ns], 1, stat=9) == VS_ERR_ARG
    assert _call(host_store, [0], 1) == VS_ERR_UNKNOWN_SAMPLE       # "ref"
    assert _call(host_store, [1, ns], 2, stat=KING) == VS_ERR_UNKNOWN_SAMPLE   # out of range
    assert _call(host_store, [1, 0xFFFFFFFF], 2) == VS_ERR_UNKNOWN_SAMPLE
    assert _call(host_store, [1], 1, stat=KING) == VS_ERR_NO_DEVICE
    # a batch without regions is reported before a bad statistic, an empty subset before it too
    assert _call(host_store, None, 0, n=0, stat=5) == VS_ERR_ARG
    assert "region" in err()
    assert _call(host_store, [1], 0, stat=5) == VS_ERR_ARG
    assert "statistic" not in err()


def test_wrapper_raises_the_same_codes(host_store):
    ns = host_store.info().num_samples
    cases = ((dict(samples=[]), VS_ERR_ARG), (dict(samples=[0]), VS_ERR_UNKNOWN_SAMPLE), (dict(samples=[ns]), VS_ERR_UNKNOWN_SAMPLE),
             (dict(stat=2), VS_ERR_ARG), (dict(stat=-1), VS_ERR_ARG), (dict(stat=2, samples=[0]), VS_ERR_ARG))
    for kw, code in cases:
        with pytest.raises(VariantStoreError) as e:
            host_store.sample_ibs([(1, 100)], **kw)
        assert e.value.code == code, kw
    with pytest.raises(VariantStoreError):
        host_store.sample_ibs([(1, 100)], samples=["no-such-sample"])
    with pytest.raises(ValueError):
        host_store.sample_ibs([(1, 100)], stat="grm")
    with pytest.raises(VariantStoreError) as e:
        host_store.sample_ibs([])
    assert e.value.code == VS_ERR_ARG
    for bad in (63, 65537, -1):
        with pytest.raises(VariantStoreError) as e:
            host_store.set_option("ibs_chunk", bad)
        assert e.value.code == VS_ERR_ARG
    for ok in (64, 65536, 0):
        host_store.set_option("ibs_chunk", ok)


def test_cli_usage_errors(golden_dir, tmp_path):
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    subprocess.run([CLI, "construct", "-r", os.path.join(golden_dir, "x.small.fa"), "-v", os.path.join(golden_dir, "x.small.vcf"), "-p", prefix],
                   check=True, capture_output=True)
    p = subprocess.run([CLI, "ibs", "-p", prefix], capture_output=True, text=True)   # no region: the usage
    assert p.returncode != 0 and "variantstore ibs" in p.stdout and "--king" in p.stdout and "--min-kinship" in p.stdout
    p = subprocess.run([CLI, "ibs", "-r", "1:100"], capture_output=True, text=True)   # no prefix
    assert p.returncode != 0 and "variantstore ibs" in p.stdout
    p = subprocess.run([CLI, "ibs", "-p", prefix, "-r", "1:100", "--grm"], capture_output=True, text=True)   # another command's flag
    assert p.returncode != 0 and "unknown option" in p.stdout + p.stderr
    for bad in ("high", "0.1x", "", "nan"):   # --min-kinship with a non-number: a usage error
        p = subprocess.run([CLI, "ibs", "-p", prefix, "-r", "1:100", "--min-kinship", bad, "--device", "-1"], capture_output=True, text=True)
        assert p.returncode != 0 and "--min-kinship takes a number" in p.stderr and "variantstore ibs" in p.stdout, bad
    p = subprocess.run([CLI, "ibs", "-p", prefix, "-r", "1:100", "-S", os.path.join(tmp_path, "missing.txt"), "--device", "-1"],
                       capture_output=True, text=True)
    assert p.returncode != 0 and "cannot open sample file" in p.stdout + p.stderr
    sfile = os.path.join(tmp_path, "samples.txt")
    with open(sfile, "w") as f:
        f.write("no-such-sample\n")
    p = subprocess.run([CLI, "ibs", "-p", prefix, "-r", "1:100", "-S", sfile, "--device", "-1"], capture_output=True, text=True)
    assert p.returncode != 0 and "Sample not found" in p.stdout + p.stderr
    for flags in (["--king"], ["--min-kinship", "0.177"], ["--min-kinship", "-1e-3"]):   # well-formed: fails only for want of a device
        p = subprocess.run([CLI, "ibs", "-p", prefix, "-r", "1:100", "--device", "-1"] + flags, capture_output=True, text=True)
        assert p.returncode != 0 and "--min-kinship takes a number" not in p.stderr and "variantstore ibs" not in p.stdout, flags
