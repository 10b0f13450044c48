"""LD pruning queries without a GPU: the argument checks of vs_query_ld_prune (made on the host, before the handle's device is asked
for) and their order, the host-only refusal, quantise_r2, the reference's own definition on hand cases, and -- through the oracle,
on the CPU -- that the "LD-block" cohort the GPU tests prune is not a vacuous input: at every threshold they use a tenth of the
eligible rows is kept, a tenth is pruned, and some row is kept although a pruned row inside the window hits it.

T = 2**20 can never hit (cov^2 <= v_i v_j): for that threshold the condition is that every eligible row is kept."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from genotype_matrix_ref import Parsed, cell, matrix
from ld_prune_ref import (DROPPED, INELIGIBLE, KEPT, ONE, PRUNED, eligible, hit, hit_band, kept_despite_pruned_hit, prune_states,
                          prune_text, row_counts, write_ld_block_cohort)
from oracle.oracle import Oracle
from variantstore_amd import VariantStore, _lib, quantise_r2
from variantstore_amd.api import VariantStoreError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_NO_DEVICE, VS_ERR_ARG, VS_ERR_UNKNOWN_SAMPLE = -3, -5, -6
UMAX = 0xFFFFFFFF

# what the GPU test of the LD-block cohort runs: the seed, the thresholds, the windows and the column subsets
BLOCK_SEED = 31
BLOCK_THRESHOLDS = (0, quantise_r2(0.2), quantise_r2(0.8), ONE - 1, ONE)
BLOCK_WINDOWS = (4, 8)


def block_subsets(names):
    return (None, names[:17], names[5:40:3])


@pytest.fixture(scope="module")
def host_store(golden_dir):
    vs = VariantStore.from_vcf(os.path.join(golden_dir, "x.small.fa"), os.path.join(golden_dir, "x.small.vcf"), device=-1)
    yield vs
    vs.close()


def _call(vs, ids, n_ids, n=1, window=64, max_bp=0, threshold=209715, min_ac=0, max_ac=UMAX):
    lib = _lib.load()
    regions = (_lib.Region * 1)(_lib.Region(1, 100))
    h = C.c_void_p()
    ptr = None if ids is None else (C.c_uint32 * max(len(ids), 1))(*ids)
    return lib.vs_query_ld_prune(vs._h, regions, n, ptr, n_ids, window, max_bp, threshold, min_ac, max_ac, C.byref(h))


def _last_error():
    return _lib.load().vs_last_error().decode()


def test_entry_points_are_declared():
    lib = _lib.load()
    for name in ("vs_query_ld_prune", "vs_result_get_ld_prune", "vs_result_ld_prune_device"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "variantstore_hip.h")).read()
    for word, value in (("VS_PRUNE_PRUNED", PRUNED), ("VS_PRUNE_KEPT", KEPT), ("VS_PRUNE_INELIGIBLE", INELIGIBLE), ("VS_PRUNE_DROPPED", DROPPED)):
        assert f"#define {word} {value}u" in header


def test_host_only_handle_refuses_pruning(host_store):
    for window in (1, 64, 256):
        for threshold in (0, 209715, ONE):
            assert _call(host_store, None, 0, window=window, threshold=threshold) == VS_ERR_NO_DEVICE
    assert _call(host_store, [1], 1) == VS_ERR_NO_DEVICE
    assert _call(host_store, [1, 1], 2, max_bp=500, min_ac=2, max_ac=2) == VS_ERR_NO_DEVICE
    for kw in (dict(), dict(samples=[1]), dict(window=1, r2=0.0), dict(window=256, r2=1.0, max_bp=9, min_ac=1, max_ac=5)):
        with pytest.raises(VariantStoreError) as e:
            host_store.ld_prune([(1, 100)], **kw)
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
    # 4. the allele-count window
    assert _call(host_store, None, 0, min_ac=3, max_ac=2) == VS_ERR_ARG
    assert "allele-count" in _last_error()
    # the order: batch < window < threshold < allele counts < ids < device
    assert _call(host_store, None, 0, n=0, window=0) == VS_ERR_ARG
    assert "region" in _last_error()
    assert _call(host_store, None, 0, window=0, threshold=ONE + 1) == VS_ERR_ARG
    assert "window" in _last_error()
    assert _call(host_store, None, 0, threshold=ONE + 1, min_ac=3, max_ac=2) == VS_ERR_ARG
    assert "threshold" in _last_error()
    assert _call(host_store, [0], 1, min_ac=3, max_ac=2) == VS_ERR_ARG
    assert _call(host_store, [0], 1, window=257) == VS_ERR_ARG
    assert _call(host_store, [ns], 1, threshold=ONE + 1) == VS_ERR_ARG
    # 5. the ids, 6. the device
    assert _call(host_store, [0], 1) == VS_ERR_UNKNOWN_SAMPLE
    assert _call(host_store, [1, ns], 2) == VS_ERR_UNKNOWN_SAMPLE
    assert _call(host_store, [1, UMAX], 2) == VS_ERR_UNKNOWN_SAMPLE
    assert _call(host_store, [1], 1, window=256, threshold=ONE, min_ac=2, max_ac=2) == VS_ERR_NO_DEVICE
    assert _call(host_store, None, 0, min_ac=0, max_ac=0) == VS_ERR_NO_DEVICE


def test_wrapper_raises_the_same_codes(host_store):
    ns = host_store.info().num_samples
    cases = ((dict(samples=[]), VS_ERR_ARG), (dict(samples=[0]), VS_ERR_UNKNOWN_SAMPLE), (dict(samples=[ns]), VS_ERR_UNKNOWN_SAMPLE),
             (dict(window=0), VS_ERR_ARG), (dict(window=257), VS_ERR_ARG), (dict(window=-1), VS_ERR_ARG), (dict(window=1 << 32), VS_ERR_ARG),
             (dict(min_ac=5, max_ac=4), VS_ERR_ARG), (dict(window=0, samples=[0]), VS_ERR_ARG))
    for kw, code in cases:
        with pytest.raises(VariantStoreError) as e:
            host_store.ld_prune([(1, 100)], **kw)
        assert e.value.code == code, kw
    for r2 in (-0.01, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            host_store.ld_prune([(1, 100)], r2=r2)
    with pytest.raises(VariantStoreError) as e:
        host_store.ld_prune([])
    assert e.value.code == VS_ERR_ARG


def test_quantise_r2():
    assert quantise_r2(0) == 0 and quantise_r2(1) == ONE == 1 << 20
    assert quantise_r2(0.2) == 209715 and quantise_r2(0.8) == 838861 and quantise_r2(0.5) == 1 << 19
    assert quantise_r2(0.5 / ONE) == 1 and quantise_r2(0.49 / ONE) == 0   # floor(x + 0.5)
    for k in (1, 7, 209715, ONE - 1):
        assert quantise_r2(k / ONE) == k
    for bad in (-1e-9, 1.0000001, float("nan")):
        with pytest.raises(ValueError):
            quantise_r2(bad)


def test_cli_refuses_bad_window_and_bound(tmp_path):
    """`--r2 1.5` is refused by the command line itself, before an index is opened (`-w 300` reaches the C ABI's check: the GPU test)."""
    exe = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
    p = subprocess.run([exe, "prune", "-p", str(tmp_path), "-r", "1:100", "--r2", "1.5"], capture_output=True, text=True)
    assert p.returncode != 0 and "--r2" in p.stderr
    p = subprocess.run([exe, "prune"], capture_output=True, text=True)
    assert p.returncode != 0 and "variantstore prune " in p.stdout


# ------------------------------------------------------------------------------------------- the reference's own definition
def _cells(dosages):
    """uint8 cells of a dosage table: 1 -> 1|0, 2 -> 1|1."""
    lut = np.asarray([0, cell(1, 0, True), cell(1, 1, True)], np.uint8)
    return lut[np.asarray(dosages, np.int64)]


def _walk(cells, window, T, **kw):
    a = cells.shape[0]
    kw.setdefault("dropped", np.zeros(a, bool))
    kw.setdefault("pos", np.arange(a) * 10 + 1)
    dropped, pos = kw.pop("dropped"), kw.pop("pos")
    return prune_states(cells, dropped, pos, [0], [a], window, T, **kw)


def test_reference_hit_is_the_integer_comparison():
    # rows (2,1,1,2,0) and (0,0,0,2,0): n = 5, Sxy = 4, cov = 5 * 4 - 6 * 2 = 8, vx = 5 * 10 - 36 = 14, vy = 5 * 4 - 4 = 16
    ci, cj = (6, 2), (2, 1)
    # r2 = 64 / 224 = 2/7: the hit flips between floor(2^20 * 2 / 7) and the next integer
    t = (64 * ONE) // 224
    assert hit(4, ci, cj, 5, t) and not hit(4, ci, cj, 5, t + 1) and hit(4, ci, cj, 5, 0) and not hit(4, ci, cj, 5, ONE)
    assert not hit(0, (0, 0), cj, 5, 0) and not hit(4, ci, (10, 5), 5, 0)   # a flat row never hits
    m = _cells([[2, 1, 1, 2, 0], [0, 0, 0, 2, 0]])
    assert row_counts(m)[0].tolist() == [6, 2] and row_counts(m)[1].tolist() == [2, 1]
    assert hit_band(m, 3, t).tolist() == [[True, False, False], [False, False, False]]
    assert not hit_band(m, 3, t + 1).any()
    # the largest operands: n = 2^21 - 1 columns of perfectly correlated rows stay exact beyond 64 bits
    n = (1 << 21) - 1
    assert hit(4 * (n // 2), (2 * (n // 2), n // 2), (2 * (n // 2), n // 2), n, ONE - 1) and not hit(4 * (n // 2), (2 * (n // 2), n // 2), (2 * (n // 2), n // 2), n, ONE)


def test_reference_threshold_one_keeps_every_eligible_row():
    rng = np.random.default_rng(1)
    m = _cells(rng.integers(0, 3, size=(80, 12)))
    m[7] = 0                      # monomorphic: ineligible
    m[9] = m[8]                   # a perfect copy: r2 = 1 is not above 1
    dropped = np.zeros(80, bool)
    dropped[20] = True
    state, kb, nk = _walk(m, 64, ONE, dropped=dropped)
    assert state[7] == INELIGIBLE and state[20] == DROPPED and kb.tolist() == [0, 80]
    assert np.all(np.delete(state, [7, 20]) == KEPT) and nk.tolist() == [78]
    assert _walk(m, 64, ONE - 1, dropped=dropped)[0][9] == PRUNED


def test_reference_threshold_zero_keeps_one_row_per_run():
    # runs of identical rows whose patterns are uncorrelated between runs (cov = 0 exactly): one kept row per run
    a = [1, 1, 0, 0, 1, 1, 0, 0]
    b = [1, 0, 1, 0, 1, 0, 1, 0]
    c = [1, 1, 1, 1, 0, 0, 0, 0]
    m = _cells([a, a, a, b, b, c, c, c, c])
    state, _kb, nk = _walk(m, 8, 0)
    assert state.tolist() == [KEPT, PRUNED, PRUNED, KEPT, PRUNED, KEPT, PRUNED, PRUNED, PRUNED] and nk.tolist() == [3]


def test_reference_pruned_rows_block_nothing():
    """A kept, B pruned by A, C hits B only -> C kept."""
    # n = 24: r2(A, B) = r2(B, C) = 256^2 / (320 * 512) = 0.4, r2(A, C) = 64^2 / 320^2 = 0.04
    a = [2] * 4 + [0] * 20
    b = [2] * 8 + [0] * 16
    c = [0] * 4 + [2] * 4 + [0] * 16
    m = _cells([a, b, c])
    T = quantise_r2(0.3)
    band = hit_band(m, 2, T)
    assert band[0, 0] and band[1, 0] and not band[0, 1]   # A-B and B-C hit, A-C does not
    state, _kb, _nk = _walk(m, 2, T)
    assert state.tolist() == [KEPT, PRUNED, KEPT]
    assert kept_despite_pruned_hit(state, 0, band, 2) == [2]
    # an ineligible B blocks nothing either; min_ac / max_ac make it so
    state, _kb, _nk = _walk(m, 2, T, min_ac=0, max_ac=15)   # ac(B) = 16
    assert state.tolist() == [KEPT, INELIGIBLE, KEPT]


def test_reference_window_and_distance():
    """A window of 1 against one of 2, and max_bp cutting inside the window."""
    a = [2, 2, 2, 0, 0, 0, 0, 0]
    x = [0, 0, 0, 0, 2, 0, 2, 0]
    m = _cells([a, x, a])
    T = quantise_r2(0.5)
    assert not hit_band(m, 2, T)[0, 0] and hit_band(m, 2, T)[0, 1]
    assert _walk(m, 1, T)[0].tolist() == [KEPT, KEPT, KEPT]
    assert _walk(m, 2, T)[0].tolist() == [KEPT, KEPT, PRUNED]
    assert _walk(m, 2, T, pos=[1, 11, 21], max_bp=19)[0].tolist() == [KEPT, KEPT, KEPT]
    assert _walk(m, 2, T, pos=[1, 11, 21], max_bp=20)[0].tolist() == [KEPT, KEPT, PRUNED]
    # regions are independent: a walk that begins at the third row has nothing in front of it
    state, kb, nk = prune_states(m, np.zeros(3, bool), [1, 11, 21], [0, 2, 1, 0], [3, 1, 2, 0], 2, T)
    assert state.tolist() == [KEPT, KEPT, PRUNED, KEPT, KEPT, KEPT] and kb.tolist() == [0, 3, 4, 6, 6] and nk.tolist() == [2, 1, 2, 0]


def test_reference_text():
    heads = ["10\tA\tC", "10\tA\tG", "12\tT\tTA", "15\tG\tT"]
    assert prune_text(heads, [6, 2, 0, 3], [KEPT, PRUNED, INELIGIBLE, DROPPED]) == ("Pos\tRef\tAlt\tAC\tState\n" "10\tA\tC\t6\tkeep\n"
                                                                                  "10\tA\tG\t2\tpruned\n" "12\tT\tTA\t0\tskip\n")
    assert prune_text([], [], []) == "Pos\tRef\tAlt\tAC\tState\n"


# ------------------------------------------------------------------------ the LD-block cohort is not a vacuous input (oracle, CPU)
def block_conditions(state, elig, band, window, T, what):
    """What both the CPU and the GPU test assert of a whole-cohort walk over the LD-block cohort."""
    ne = int(elig.sum())
    kept, pruned = int((state == KEPT).sum()), int((state == PRUNED).sum())
    assert ne >= 250 and kept + pruned == ne, what
    if T == ONE:
        assert pruned == 0, what
        return
    assert 10 * kept >= ne and 10 * pruned >= ne, (what, ne, kept, pruned)
    assert kept_despite_pruned_hit(state, 0, band, window), what


def test_block_cohort_is_not_vacuous(tmp_path):
    fasta, vcf, names, last = write_ld_block_cohort(str(tmp_path), BLOCK_SEED)
    vs = VariantStore.from_vcf(fasta, vcf, device=-1)
    plain = os.path.join(tmp_path, "plain.bin")
    vs.export_plain(plain)
    vs.close()
    n, _early, text = Oracle(plain).get_var_in_ref(1, last + 50)
    assert n >= 0
    parsed = Parsed([text])
    assert 280 <= parsed.n_rows <= 360
    pos = [int(h.split("\t")[0]) for h in parsed.heads]
    assert len(set(pos)) < len(pos), "no multi-allelic site"
    assert "/" in text and "|" in text
    none = np.zeros(parsed.n_rows, bool)
    for sub in block_subsets(names):
        m = matrix(parsed, sub if sub is not None else names)
        elig = eligible(m, none)
        for T in BLOCK_THRESHOLDS:
            band = hit_band(m, max(BLOCK_WINDOWS), T)
            for window in BLOCK_WINDOWS:
                state, kb, nk = prune_states(m, none, pos, [0], [parsed.n_rows], window, T, band=band)
                assert kb.tolist() == [0, parsed.n_rows] and int(nk[0]) == int((state == KEPT).sum())
                block_conditions(state, elig, band, window, T, (sub is None or len(sub), T, window))
