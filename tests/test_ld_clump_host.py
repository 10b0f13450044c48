"""LD clumping queries without a GPU: the argument checks of vs_query_ld_clump (made on the host, before the handle's device is asked
for) and their order, the host-only refusal, the key conversion, the mapping route, the reference's own definition on hand cases,
and -- through the oracle, on the CPU -- that on the "LD-block" cohort the sequential procedure and the round formulation give the
same bytes for every p-value family, that the table-order family reproduces the pruning reference's KEPT set, and that the cohort
is not a vacuous input: with uniform p-values a tenth of the candidates is INDEX, a tenth MEMBER, some row is INDEX although a
MEMBER of higher priority hits it, and some MEMBER's owner is not the nearest INDEX that hits it.

T = 2**20 can never hit: there every index-eligible candidate is INDEX and nothing is MEMBER."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from genotype_matrix_ref import Parsed, cell, matrix
from ld_clump_ref import (DROPPED, INDEX, INELIGIBLE, MEMBER, NO_KEY, NO_OWNER, UNCLUMPED, classes, clump_states, clump_states_by_rounds,
                          clump_text, first_maximal_independent_set, index_despite_member_hit, key_of, keys_of,
                          members_not_with_the_nearest_index, pvalue_families, region_hits, window_hits)
from ld_prune_ref import KEPT, ONE, eligible, hit_band, prune_states, write_ld_block_cohort
from oracle.oracle import Oracle
from variantstore_amd import VariantStore, _lib, pvalue_keys, quantise_r2
from variantstore_amd.api import VariantStoreError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_NO_DEVICE, VS_ERR_ARG, VS_ERR_UNKNOWN_SAMPLE = -3, -5, -6
UMAX = 0xFFFFFFFF
NAN = float("nan")

# what the GPU test of the LD-block cohort runs as well: the seeds, the thresholds and the windows
BLOCK_SEED = 31
P_SEED = 77
CONDITION_THRESHOLDS = (quantise_r2(0.2), quantise_r2(0.5), quantise_r2(0.8))
BLOCK_WINDOWS = (4, 8)


@pytest.fixture(scope="module")
def host_store(golden_dir):
    vs = VariantStore.from_vcf(os.path.join(golden_dir, "x.small.fa"), os.path.join(golden_dir, "x.small.vcf"), device=-1)
    yield vs
    vs.close()


def _call(vs, ids, n_ids, n=1, pvalues=(0.5,), n_pvalues=None, window=64, max_bp=0, threshold=1 << 19, p1=1e-4, p2=1e-2):
    lib = _lib.load()
    regions = (_lib.Region * 1)(_lib.Region(1, 100))
    h = C.c_void_p()
    ptr = None if ids is None else (C.c_uint32 * max(len(ids), 1))(*ids)
    pv = None if pvalues is None else (C.c_double * max(len(pvalues), 1))(*pvalues)
    n_pv = (0 if pvalues is None else len(pvalues)) if n_pvalues is None else n_pvalues
    return lib.vs_query_ld_clump(vs._h, regions, n, ptr, n_ids, pv, n_pv, window, max_bp, threshold, p1, p2, C.byref(h))


def _last_error():
    return _lib.load().vs_last_error().decode()


def test_entry_points_are_declared():
    lib = _lib.load()
    for name in ("vs_query_ld_clump", "vs_result_get_ld_clump", "vs_result_ld_clump_device"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "variantstore_hip.h")).read()
    for word, value in (("VS_CLUMP_MEMBER", MEMBER), ("VS_CLUMP_INDEX", INDEX), ("VS_CLUMP_INELIGIBLE", INELIGIBLE), ("VS_CLUMP_DROPPED", DROPPED),
                        ("VS_CLUMP_UNCLUMPED", UNCLUMPED)):
        assert f"#define {word} {value}u" in header
    assert "#define VS_CLUMP_NO_OWNER 0xFFFFFFFFu" in header


def test_host_only_handle_refuses_clumping(host_store):
    for window in (1, 64, 256):
        for threshold in (0, 1 << 19, ONE):
            assert _call(host_store, None, 0, window=window, threshold=threshold) == VS_ERR_NO_DEVICE
    assert _call(host_store, [1], 1) == VS_ERR_NO_DEVICE
    assert _call(host_store, [1, 1], 2, pvalues=(0.0, -0.0, 1.0, NAN, 5e-324), max_bp=500, p1=0.0, p2=0.0) == VS_ERR_NO_DEVICE
    assert _call(host_store, None, 0, p1=1.0, p2=1.0) == VS_ERR_NO_DEVICE and _call(host_store, None, 0, p1=-0.0, p2=0.0) == VS_ERR_NO_DEVICE
    for kw in (dict(), dict(samples=[1]), dict(window=1, r2=0.0), dict(window=256, r2=1.0, max_bp=9, p1=0.5, p2=0.5)):
        with pytest.raises(VariantStoreError) as e:
            host_store.ld_clump([(1, 100)], np.asarray([0.1, NAN]), **kw)
        assert e.value.code == VS_ERR_NO_DEVICE, kw


def test_argument_errors_and_their_order(host_store):
    ns = host_store.info().num_samples
    # 1. the batch and the subset
    assert _call(host_store, [1], 1, n=0) == VS_ERR_ARG
    assert "region" in _last_error()
    assert _call(host_store, None, 3) == VS_ERR_ARG
    assert _call(host_store, [1], 0) == VS_ERR_ARG
    # 2. the window
    for window in (0, 257, UMAX):
        assert _call(host_store, None, 0, window=window) == VS_ERR_ARG, window
        assert "window" in _last_error()
    # 3. the threshold
    for threshold in (ONE + 1, 1 << 21, UMAX):
        assert _call(host_store, None, 0, threshold=threshold) == VS_ERR_ARG, threshold
        assert "threshold" in _last_error()
    # 4. the p-values' pointer
    assert _call(host_store, None, 0, pvalues=None) == VS_ERR_ARG
    assert "pvalues" in _last_error()
    assert _call(host_store, None, 0, pvalues=None, n_pvalues=4) == VS_ERR_ARG
    # 5. p1 and p2, 6. their order
    for bad in (-1e-9, 1.0000001, NAN, float("inf"), -float("inf")):
        assert _call(host_store, None, 0, p1=bad, p2=1.0) == VS_ERR_ARG, bad
        assert "p1" in _last_error()
        assert _call(host_store, None, 0, p1=0.0, p2=bad) == VS_ERR_ARG, bad
        assert "p2" in _last_error()
    assert _call(host_store, None, 0, p1=0.02, p2=0.01) == VS_ERR_ARG
    assert "above" in _last_error()
    assert _call(host_store, None, 0, p1=5e-324, p2=0.0) == VS_ERR_ARG   # the smallest subnormal is above 0
    # 7. the p-values: the message names the row
    for bad in (-1e-300, 1.0000001, 2.0, float("inf"), -float("inf"), -5e-324):
        assert _call(host_store, None, 0, pvalues=(0.5, NAN, 1.0, bad, 3.0)) == VS_ERR_ARG, bad
        assert "row 3" in _last_error()
    # the order: batch < window < threshold < pvalues < p1 < p2 < p1 > p2 < the values < ids < device
    assert _call(host_store, None, 0, n=0, window=0) == VS_ERR_ARG
    assert "region" in _last_error()
    assert _call(host_store, None, 0, window=0, threshold=ONE + 1) == VS_ERR_ARG
    assert "window" in _last_error()
    assert _call(host_store, None, 0, threshold=ONE + 1, pvalues=None) == VS_ERR_ARG
    assert "threshold" in _last_error()
    assert _call(host_store, None, 0, pvalues=None, p1=2.0) == VS_ERR_ARG
    assert "pvalues" in _last_error()
    assert _call(host_store, None, 0, p1=2.0, p2=3.0) == VS_ERR_ARG
    assert "p1" in _last_error()
    assert _call(host_store, None, 0, p1=0.5, p2=3.0, pvalues=(7.0,)) == VS_ERR_ARG
    assert "p2" in _last_error()
    assert _call(host_store, None, 0, p1=0.5, p2=0.25, pvalues=(7.0,)) == VS_ERR_ARG
    assert "above" in _last_error()
    assert _call(host_store, [0], 1, pvalues=(7.0,)) == VS_ERR_ARG
    assert "row 0" in _last_error()
    assert _call(host_store, [0], 1, window=257) == VS_ERR_ARG
    assert _call(host_store, [ns], 1, p1=0.5, p2=0.25) == VS_ERR_ARG
    # 8. the ids, 9. the device
    assert _call(host_store, [0], 1) == VS_ERR_UNKNOWN_SAMPLE
    assert _call(host_store, [1, ns], 2) == VS_ERR_UNKNOWN_SAMPLE
    assert _call(host_store, [1, UMAX], 2) == VS_ERR_UNKNOWN_SAMPLE
    assert _call(host_store, [1], 1, window=256, threshold=ONE, p1=0.0, p2=1.0) == VS_ERR_NO_DEVICE
    assert _call(host_store, None, 0, pvalues=(), n_pvalues=0) == VS_ERR_NO_DEVICE   # (a non-NULL pointer to no p-values)


def test_wrapper_raises_the_same_codes(host_store):
    ns = host_store.info().num_samples
    pv = np.asarray([0.5, 0.25])
    cases = ((dict(samples=[]), VS_ERR_ARG), (dict(samples=[0]), VS_ERR_UNKNOWN_SAMPLE), (dict(samples=[ns]), VS_ERR_UNKNOWN_SAMPLE),
             (dict(window=0), VS_ERR_ARG), (dict(window=257), VS_ERR_ARG), (dict(window=-1), VS_ERR_ARG), (dict(window=1 << 32), VS_ERR_ARG),
             (dict(p1=0.5, p2=0.1), VS_ERR_ARG), (dict(p1=-1.0), VS_ERR_ARG), (dict(p2=NAN), VS_ERR_ARG), (dict(window=0, samples=[0]), VS_ERR_ARG))
    for kw, code in cases:
        with pytest.raises(VariantStoreError) as e:
            host_store.ld_clump([(1, 100)], pv, **kw)
        assert e.value.code == code, kw
    for r2 in (-0.01, 1.5, NAN, float("inf")):
        with pytest.raises(ValueError):
            host_store.ld_clump([(1, 100)], pv, r2=r2)
    with pytest.raises(VariantStoreError) as e:
        host_store.ld_clump([(1, 100)], np.asarray([0.5, 1.5]))
    assert e.value.code == VS_ERR_ARG and "row 1" in str(e.value)
    with pytest.raises(ValueError):
        host_store.ld_clump([(1, 100)], np.zeros((2, 2)))
    with pytest.raises(VariantStoreError) as e:
        host_store.ld_clump([], pv)
    assert e.value.code == VS_ERR_ARG
    with pytest.raises(VariantStoreError) as e:
        host_store.ld_clump([(1, 100)], np.zeros(0))   # no p-values: not NULL, the device is asked for
    assert e.value.code == VS_ERR_NO_DEVICE


def test_keys_are_monotone():
    tiny = 5e-324   # the smallest subnormal
    ladder = [0.0, tiny, 2 * tiny, 2.2250738585072014e-308 / 2, 2.2250738585072014e-308, 1e-300, 1e-10, 1e-4, 0.01, 0.5, np.nextafter(1.0, 0.0), 1.0]
    keys = [key_of(p) for p in ladder]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert keys[0] == 0 and keys[1] == 1 and keys[2] == 2 and keys[-1] == 0x3FF0000000000000
    assert key_of(-0.0) == 0 and key_of(NAN) == NO_KEY and NO_KEY > keys[-1]
    rng = np.random.default_rng(1)
    p = np.concatenate([rng.random(2000), rng.random(2000) ** 40, 10.0 ** -rng.uniform(0, 320, 2000), np.asarray(ladder), [-0.0]])
    k = keys_of(p)
    order = np.argsort(p, kind="stable")
    assert np.all(np.diff(k[order].astype(np.float64)) >= 0)   # (a first, coarse look)
    ks = [int(x) for x in k[order]]
    assert ks == sorted(ks)
    assert all((p[a] < p[b]) == (int(k[a]) < int(k[b])) and (p[a] == p[b]) == (int(k[a]) == int(k[b])) for a, b in rng.integers(0, p.shape[0], (5000, 2)))
    # the package's conversion is the reference's
    mixed = np.concatenate([p, [NAN, NAN]])
    got = pvalue_keys(mixed)
    assert got.dtype == np.uint64 and got.shape == mixed.shape and np.array_equal(got, keys_of(mixed)) and int(got[-1]) == NO_KEY
    assert pvalue_keys(np.zeros((2, 3))).shape == (2, 3) and int(pvalue_keys(-0.0)) == 0 and int(pvalue_keys(1.0)) == 0x3FF0000000000000
    for bad in (-1e-300, -tiny, 1.0000001, float("inf")):
        with pytest.raises(ValueError):
            pvalue_keys([0.5, bad])
        with pytest.raises(ValueError):
            key_of(bad)


def test_mapping_route(host_store, monkeypatch):
    """A mapping is laid out in table order; rows without a key get NaN (dropped rows have no key at all) and keys that match no row
    come back.  (The rows come from an allele_counts batch: here its answer is given; the GPU test goes through the device.)"""
    keys = [(10, "A", "C"), (10, "A", "G"), None, (12, "T", "TA"), (15, "G", "T")]
    monkeypatch.setattr(host_store, "_table_keys", lambda regions: keys)
    pv, unmatched = host_store._pvalues_from_mapping([(1, 100)], {(10, "A", "G"): 0.25, (15, "G", "T"): 1e-9, (15, "G", "A"): 0.5, (99, "C", "T"): 0.1,
                                                                   (np.int64(12), "T", "TA"): np.float32(0.5)})
    assert pv.dtype == np.float64 and np.array_equal(pv, np.asarray([NAN, 0.25, NAN, 0.5, 1e-9]), equal_nan=True)
    assert unmatched == [(15, "G", "A"), (99, "C", "T")]
    with pytest.raises(VariantStoreError) as e:   # the call itself goes on to the C ABI with these p-values
        host_store.ld_clump([(1, 100)], {(10, "A", "G"): 0.25})
    assert e.value.code == VS_ERR_NO_DEVICE
    with pytest.raises(VariantStoreError) as e:
        host_store.ld_clump([(1, 100)], {(10, "A", "G"): 1.25})
    assert e.value.code == VS_ERR_ARG and "row 1" in str(e.value)


def test_cli_refuses_bad_values(tmp_path):
    """Bad bounds are refused by the command line itself, before an index is opened."""
    exe = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
    pfile = os.path.join(tmp_path, "p.txt")
    with open(pfile, "w") as f:
        f.write("10 A C 0.5\n")
    for flag, word in ((["--r2", "1.5"], "--r2"), (["--p1", "2"], "--p1"), (["--p2", "-0.1"], "--p2"), (["--p1", "x"], "--p1"), (["--p2", "nan"], "--p2")):
        p = subprocess.run([exe, "clump", "-p", str(tmp_path), "-r", "1:100", "-A", pfile] + flag, capture_output=True, text=True)
        assert p.returncode != 0 and word in p.stderr, flag
    p = subprocess.run([exe, "clump"], capture_output=True, text=True)
    assert p.returncode != 0 and "variantstore clump " in p.stdout
    p = subprocess.run([exe, "clump", "-p", str(tmp_path), "-r", "1:100"], capture_output=True, text=True)   # no -A
    assert p.returncode != 0 and "variantstore clump " in p.stdout


# ------------------------------------------------------------------------------------------- the reference's own definition
def _cells(dosages):
    """uint8 cells of a dosage table: 1 -> 1|0, 2 -> 1|1."""
    lut = np.asarray([0, cell(1, 0, True), cell(1, 1, True)], np.uint8)
    return lut[np.asarray(dosages, np.int64)]


def _both(cells, p, window, T, p1=1.0, p2=1.0, regions=None, **kw):
    """The sequential answer of one region over all rows (or `regions`), after checking that the rounds give the same bytes."""
    a = cells.shape[0]
    dropped = kw.pop("dropped", np.zeros(a, bool))
    pos = kw.pop("pos", np.arange(a) * 10 + 1)
    rb, rc = ([0], [a]) if regions is None else regions
    args = (cells, dropped, pos, rb, rc, keys_of(p), window, T, key_of(p1), key_of(p2))
    seq = clump_states(*args, **kw)
    rnd = clump_states_by_rounds(*args, **kw)
    for x, y in zip(seq, rnd[:4]):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    return seq + (rnd[4],)


A8 = [1, 1, 0, 0, 1, 1, 0, 0]
B8 = [1, 0, 1, 0, 1, 0, 1, 0]
C8 = [1, 1, 1, 1, 0, 0, 0, 0]


def test_reference_clumps_runs_of_copies():
    # runs of identical rows whose patterns are uncorrelated between runs (cov = 0 exactly): one clump per run, led by its best row
    m = _cells([A8, A8, A8, B8, B8, C8, C8, C8, C8])
    p = [0.3, 0.1, 0.2, 0.5, 0.4, 0.9, 0.8, 0.01, 0.7]
    state, owner, kb, ni, _r = _both(m, p, 8, 0)
    assert state.tolist() == [MEMBER, INDEX, MEMBER, MEMBER, INDEX, MEMBER, MEMBER, INDEX, MEMBER]
    assert owner.tolist() == [1, 1, 1, 4, 4, 7, 7, 7, 7] and kb.tolist() == [0, 9] and ni.tolist() == [3]
    # the window reaches both ways, one row each way: row 5 is out of row 7's reach
    state, owner, _kb, ni, _r = _both(m, p, 1, 0)
    assert state.tolist() == [MEMBER, INDEX, MEMBER, MEMBER, INDEX, INDEX, MEMBER, INDEX, MEMBER]
    assert owner.tolist() == [1, 1, 1, 4, 4, 5, 7, 7, 7] and ni.tolist() == [4]
    # ties go to the earlier row; -0.0 is 0
    state, owner, _kb, _ni, _r = _both(m, [0.5, 0.5, 0.5, 0.0, -0.0, 1.0, 1.0, 1.0, 1.0], 8, 0)
    assert state.tolist() == [INDEX, MEMBER, MEMBER, INDEX, MEMBER, INDEX, MEMBER, MEMBER, MEMBER] and owner.tolist() == [0, 0, 0, 3, 3, 5, 5, 5, 5]
    # T = 2^20: nothing hits
    state, owner, _kb, ni, _r = _both(m, p, 8, ONE)
    assert np.all(state == INDEX) and owner.tolist() == list(range(9)) and ni.tolist() == [9]


def test_reference_thresholds_and_missing_p_values():
    m = _cells([A8, A8, A8, B8, B8, C8, C8, C8, C8])
    m[2] = 0   # monomorphic
    dropped = np.zeros(9, bool)
    dropped[8] = True
    p = [0.3, 0.001, 0.2, 0.004, 0.05, NAN, 0.8, 0.002, 0.7]
    state, owner, _kb, ni, _r = _both(m, p, 8, 0, p1=0.003, p2=0.3, dropped=dropped)
    # row 0 joins row 1; row 3 (p between p1 and p2) cannot lead and nothing leads its run: it and row 4 stay unclumped; row 5 has no
    # p-value, row 6 lies above p2, row 7 leads alone
    assert state.tolist() == [MEMBER, INDEX, INELIGIBLE, UNCLUMPED, UNCLUMPED, INELIGIBLE, INELIGIBLE, INDEX, DROPPED]
    assert owner.tolist() == [1, 1, NO_OWNER, NO_OWNER, NO_OWNER, NO_OWNER, NO_OWNER, 7, NO_OWNER] and ni.tolist() == [2]
    # p1 = p2 = 0: only the rows with p = 0 take part
    state, owner, _kb, ni, _r = _both(m, [0.0, 1e-320, 0.0, 0.0, -0.0, 0.0, 5e-324, 0.0, 0.0], 8, 0, p1=0.0, p2=0.0, dropped=dropped)
    assert state.tolist() == [INDEX, INELIGIBLE, INELIGIBLE, INDEX, MEMBER, INDEX, INELIGIBLE, MEMBER, DROPPED] and ni.tolist() == [3]
    assert owner.tolist() == [0, NO_OWNER, NO_OWNER, 3, 3, 5, NO_OWNER, 5, NO_OWNER]


def test_reference_members_block_nothing_and_owners_go_by_priority():
    """A - B - C with r2(A, B) = r2(B, C) = 0.4 and r2(A, C) = 0.04 at T = q(0.3) (the pruning reference's case)."""
    a = [2] * 4 + [0] * 20
    b = [2] * 8 + [0] * 16
    c = [0] * 4 + [2] * 4 + [0] * 16
    m = _cells([a, b, c])
    T = quantise_r2(0.3)
    # A leads and takes B; C, hit by the member B only, leads as well: an INDEX despite a higher-priority MEMBER that hits it
    state, owner, _kb, _ni, rounds = _both(m, [0.1, 0.2, 0.3], 2, T)
    assert state.tolist() == [INDEX, MEMBER, INDEX] and owner.tolist() == [0, 0, 2] and rounds.tolist() == [3]   # (A; then B; then C)
    hits = region_hits(window_hits(hit_band(m, 2, T), [1, 11, 21], 2), 0, 3, 2)
    assert index_despite_member_hit(state, keys_of([0.1, 0.2, 0.3]), hits) == [2]
    # B leads and takes both
    state, owner, _kb, _ni, rounds = _both(m, [0.2, 0.1, 0.3], 2, T)
    assert state.tolist() == [MEMBER, INDEX, MEMBER] and owner.tolist() == [1, 1, 1] and rounds.tolist() == [2]
    # A and the last C lead; B, hit by both, goes to C: the higher priority, although A is nearer
    m5 = _cells([a, b, [0] * 24, c, c])
    m5[2, 20:] = _cells([2] * 4)   # unrelated to the others (cov < 0: r2 = 0.04 with A and C, 0.1 with B)
    state, owner, _kb, _ni, _r = _both(m5, [0.2, 0.5, 0.9, 0.3, 0.1], 4, T)
    assert state.tolist() == [INDEX, MEMBER, INDEX, MEMBER, INDEX] and owner.tolist() == [0, 4, 2, 4, 4]
    hits = region_hits(window_hits(hit_band(m5, 4, T), np.arange(5), 4), 0, 5, 4)
    assert hits[1].tolist() == [True, False, False, True, True]
    assert members_not_with_the_nearest_index(state, owner, hits) == [1]
    # max_bp cuts the pair of B and the last C: B goes to A
    state, owner, _kb, _ni, _r = _both(m5, [0.2, 0.5, 0.9, 0.3, 0.1], 4, T, pos=[1, 5, 9, 13, 30], max_bp=20)
    assert state.tolist() == [INDEX, MEMBER, INDEX, MEMBER, INDEX] and owner.tolist() == [0, 0, 2, 4, 4]


def test_reference_regions_are_independent():
    m = _cells([A8, A8, A8, B8, B8, C8, C8, C8, C8])
    p = [0.1, 0.2, 0.3, 0.5, 0.4, 0.9, 0.8, 0.01, 0.7]
    state, owner, kb, ni, _r = _both(m, p, 8, 0, regions=([0, 1, 5, 0, 2], [9, 2, 3, 0, 1]))
    assert kb.tolist() == [0, 9, 11, 14, 14, 15] and ni.tolist() == [3, 1, 1, 0, 1]
    # row 1 is a MEMBER of row 0 in the whole table and leads the region that begins with it; owners are region-relative
    assert state[:9].tolist() == [INDEX, MEMBER, MEMBER, MEMBER, INDEX, MEMBER, MEMBER, INDEX, MEMBER] and owner[:9].tolist() == [0, 0, 0, 4, 4, 7, 7, 7, 7]
    assert state[9:11].tolist() == [INDEX, MEMBER] and owner[9:11].tolist() == [0, 0]
    assert state[11:14].tolist() == [MEMBER, MEMBER, INDEX] and owner[11:14].tolist() == [2, 2, 2]
    assert state[14:].tolist() == [INDEX] and owner[14:].tolist() == [0]


def test_reference_text():
    heads = ["10\tA\tC", "10\tA\tG", "12\tT\tTA", "15\tG\tT", "17\tC\tA", "19\tG\tC"]
    text = clump_text(heads, [6, 2, 0, 3, 4, 9], [1e-9, 0.25, NAN, 0.5, 0.001234567, -0.0], [INDEX, MEMBER, INELIGIBLE, DROPPED, UNCLUMPED, MEMBER],
                      [0, 0, NO_OWNER, NO_OWNER, NO_OWNER, 0])
    assert text == ("Pos\tRef\tAlt\tAC\tP\tState\tIndex\n" "10\tA\tC\t6\t1e-09\tindex\t10:A:C\n" "10\tA\tG\t2\t0.25\tclumped\t10:A:C\n"
                    "12\tT\tTA\t0\t.\tskip\t.\n" "17\tC\tA\t4\t0.00123457\tunclumped\t.\n" "19\tG\tC\t9\t0\tclumped\t10:A:C\n")
    assert clump_text([], [], [], [], []) == "Pos\tRef\tAlt\tAC\tP\tState\tIndex\n"


# ------------------------------------------------- the LD-block cohort: both formulations, pruning, the conditions (oracle, CPU)
def clump_conditions(state, owner, keys, lead, hits, T, what):
    """What both the CPU and the GPU test assert of a whole-cohort clumping of the LD-block cohort with uniform p, p1 = p2 = 1."""
    n = int(lead.sum())
    index, member = int((state == INDEX).sum()), int((state == MEMBER).sum())
    assert n >= 250 and index + member == n and not (state == UNCLUMPED).any(), what
    if T == ONE:
        assert member == 0, what
        return
    assert 10 * index >= n and 10 * member >= n, (what, n, index, member)
    assert index_despite_member_hit(state, keys, hits), what
    assert members_not_with_the_nearest_index(state, owner, hits), what


@pytest.fixture(scope="module")
def block_cohort(tmp_path_factory):
    """(cells by the oracle, positions, heads) of the LD-block cohort over all of its samples."""
    tmp = str(tmp_path_factory.mktemp("ldblock"))
    fasta, vcf, names, last = write_ld_block_cohort(tmp, BLOCK_SEED)
    vs = VariantStore.from_vcf(fasta, vcf, device=-1)
    plain = os.path.join(tmp, "plain.bin")
    vs.export_plain(plain)
    vs.close()
    n, _early, text = Oracle(plain).get_var_in_ref(1, last + 50)
    assert n >= 0
    parsed = Parsed([text])
    assert parsed.n_rows == 316 and len(names) == 40
    return matrix(parsed, names), np.asarray([int(h.split("\t")[0]) for h in parsed.heads]), parsed.heads


def test_formulations_agree_on_the_block_cohort(block_cohort):
    cells, pos, _heads = block_cohort
    a = cells.shape[0]
    none = np.zeros(a, bool)
    rng = np.random.default_rng(3)
    starts = rng.integers(0, a - 1, size=12)
    rb = np.concatenate([[0], starts, [5]])
    rc = np.concatenate([[a], np.minimum(rng.integers(1, 120, size=12), a - starts), [0]])
    deepest = 0
    for T in (0, quantise_r2(0.2), quantise_r2(0.5), quantise_r2(0.8), ONE):
        band = hit_band(cells, max(BLOCK_WINDOWS), T)
        for window in BLOCK_WINDOWS:
            for max_bp in (0, 40):
                hits = region_hits(window_hits(band, pos, window, max_bp), 0, a, window)
                for name, p, p1, p2 in pvalue_families(a, P_SEED):
                    keys = keys_of(p)
                    args = (cells, none, pos, rb, rc, keys, window, T, key_of(p1), key_of(p2))
                    seq = clump_states(*args, max_bp=max_bp, band=band)
                    rnd = clump_states_by_rounds(*args, max_bp=max_bp, band=band)
                    for x, y in zip(seq, rnd[:4]):
                        assert x.dtype == y.dtype and np.array_equal(x, y), (name, T, window, max_bp)
                    deepest = max(deepest, int(rnd[4].max()))
                    # the third statement: the INDEX rows of the whole table are the first maximal independent set of the leads
                    cand, lead = classes(cells, none, keys, key_of(p1), key_of(p2))
                    rank = np.empty(a, np.int64)
                    rank[np.lexsort((np.arange(a), keys))] = np.arange(a)
                    assert np.array_equal(seq[0][:a] == INDEX, first_maximal_independent_set(hits, lead, rank)), (name, T, window)
                    assert np.all(seq[0][:a][cand & ~lead] != INDEX)
                    if name == "holes":
                        assert np.all(seq[0][:a][np.isnan(p)] == INELIGIBLE) and np.isnan(p).sum() > 15
                    if name == "ordered":   # table order, p1 = p2 = 1: the forward greedy of the pruning query
                        kept = prune_states(cells, none, pos, rb, rc, window, T, max_bp, band=band)
                        assert np.array_equal(seq[0] == INDEX, kept[0] == KEPT), (T, window, max_bp)
                        assert np.array_equal(seq[3], kept[2]) and np.array_equal(seq[2], kept[1])
                    if name == "uniform" and T in CONDITION_THRESHOLDS + (ONE,) and not max_bp:
                        clump_conditions(seq[0][:a], seq[1][:a], keys, lead, hits, T, (T, window))
    assert deepest >= 100   # the deep chain the GPU test runs: table order at T = 0


def test_table_order_needs_many_rounds(block_cohort):
    """At T = 0 and window 4 the table-order family is one long chain: the rounds of the synchronous formulation."""
    cells, pos, _heads = block_cohort
    a = cells.shape[0]
    p = (np.arange(a) + 1.0) / (a + 1.0)
    rnd = clump_states_by_rounds(cells, np.zeros(a, bool), pos, [0], [a], keys_of(p), 4, 0, key_of(1.0), key_of(1.0))
    assert 100 <= int(rnd[4][0]) <= a
    uniform = pvalue_families(a, P_SEED)[0][1]
    rnd = clump_states_by_rounds(cells, np.zeros(a, bool), pos, [0], [a], keys_of(uniform), 4, 0, key_of(1.0), key_of(1.0))
    assert int(rnd[4][0]) <= 12
