"""LD-score queries without a GPU: the quotient function of the kernel, compiled for the host and held against a 128-bit division
(plainly and under the sanitizers), the argument checks of vs_query_ld_scores and their order, the host-only refusal, the
reference's own definition on hand cases, and -- through the oracle, on the CPU -- that the "LD-block" cohort the GPU tests score
is not a vacuous input: for every window, distance limit and subset they use, a tenth of the scored rows has a sum above 2 * 2^32
(real LD beyond the row itself), some row is ineligible, and the row limit and the position limit each cut a pair."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from genotype_matrix_ref import Parsed, matrix
from ld_prune_ref import eligible, write_ld_block_cohort
from ld_score_ref import DROPPED, INELIGIBLE, ONE, SCORED, ld_scores, q32, score_text
from oracle.oracle import Oracle
from test_ld_prune_host import _cells, block_subsets
from variantstore_amd import VariantStore, _lib
from variantstore_amd.api import QueryResult, VariantStoreError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_NO_DEVICE, VS_ERR_ARG, VS_ERR_UNKNOWN_SAMPLE = -3, -5, -6
UMAX = 0xFFFFFFFF

# what the GPU test of the LD-block cohort runs: the seed, the row windows and the distance limits (the allele-count window: block_ac_window)
BLOCK_SEED = 31
BLOCK_WINDOWS = (0, 5, 70)
BLOCK_MAX_BP = (0, 40)   # (sites are 4 .. 24 bases apart: 40 bases cut inside a window of 5 rows)


@pytest.fixture(scope="module")
def host_store(golden_dir):
    vs = VariantStore.from_vcf(os.path.join(golden_dir, "x.small.fa"), os.path.join(golden_dir, "x.small.vcf"), device=-1)
    yield vs
    vs.close()


def _call(vs, ids, n_ids, n=1, window=0, max_bp=0, min_ac=0, max_ac=UMAX):
    lib = _lib.load()
    regions = (_lib.Region * 1)(_lib.Region(1, 100))
    h = C.c_void_p()
    ptr = None if ids is None else (C.c_uint32 * max(len(ids), 1))(*ids)
    return lib.vs_query_ld_scores(vs._h, regions, n, ptr, n_ids, window, max_bp, min_ac, max_ac, C.byref(h))


def _last_error():
    return _lib.load().vs_last_error().decode()


# ------------------------------------------------------------------------------------------------------ the quotient function
def test_quotient_standalone_and_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "ld_score_host_check.cpp")
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])):
        exe = os.path.join(tmp_path, "ld_score_host_check_" + name)
        subprocess.check_call(["g++", "-std=c++17", *flags, "-o", exe, src])
        out = subprocess.run([exe], capture_output=True, text=True)
        assert out.returncode == 0, (name, out.stdout[-2000:], out.stderr[-2000:])
        assert out.stdout.startswith("ok ") and int(out.stdout.split()[1]) > 1_000_000 and "runtime error" not in out.stderr, (name, out.stderr[-2000:])


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared():
    lib = _lib.load()
    for name in ("vs_query_ld_scores", "vs_result_get_ld_scores", "vs_result_ld_scores_device"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "variantstore_hip.h")).read()
    for word, value in (("VS_LDSCORE_SCORED", SCORED), ("VS_LDSCORE_INELIGIBLE", INELIGIBLE), ("VS_LDSCORE_DROPPED", DROPPED)):
        assert f"#define {word} {value}u" in header
    assert QueryResult.LDSCORE_STATES == {"scored": SCORED, "ineligible": INELIGIBLE, "dropped": DROPPED} and QueryResult.LDSCORE_ONE == ONE


def test_host_only_handle_refuses(host_store):
    for window in (0, 1, 64, 257, 100_000, UMAX):
        for max_bp in (0, 1_000_000, UMAX):
            assert _call(host_store, None, 0, window=window, max_bp=max_bp) == VS_ERR_NO_DEVICE
    assert _call(host_store, [1], 1) == VS_ERR_NO_DEVICE
    assert _call(host_store, [1, 1], 2, max_bp=500, min_ac=2, max_ac=2) == VS_ERR_NO_DEVICE
    for kw in (dict(), dict(samples=[1]), dict(window=1, max_bp=0), dict(window=5000, max_bp=9, min_ac=1, max_ac=5)):
        with pytest.raises(VariantStoreError) as e:
            host_store.ld_scores([(1, 100)], **kw)
        assert e.value.code == VS_ERR_NO_DEVICE, kw


def test_argument_errors_and_their_order(host_store):
    ns = host_store.info().num_samples
    # 1. the batch and the subset
    assert _call(host_store, [1], 1, n=0) == VS_ERR_ARG
    assert "region" in _last_error()
    assert _call(host_store, None, 3) == VS_ERR_ARG
    assert _call(host_store, [1], 0) == VS_ERR_ARG
    # 2. the allele-count window
    assert _call(host_store, None, 0, min_ac=3, max_ac=2) == VS_ERR_ARG
    assert "allele-count" in _last_error()
    # the order: batch < allele counts < ids < device
    assert _call(host_store, None, 0, n=0, min_ac=3, max_ac=2) == VS_ERR_ARG
    assert "region" in _last_error()
    assert _call(host_store, [0], 1, min_ac=3, max_ac=2) == VS_ERR_ARG
    assert "allele-count" in _last_error()
    # 3. the ids, 4. the device
    assert _call(host_store, [0], 1) == VS_ERR_UNKNOWN_SAMPLE
    assert _call(host_store, [1, ns], 2) == VS_ERR_UNKNOWN_SAMPLE
    assert _call(host_store, [1, UMAX], 2) == VS_ERR_UNKNOWN_SAMPLE
    assert _call(host_store, [1], 1, window=256, min_ac=2, max_ac=2) == VS_ERR_NO_DEVICE
    assert _call(host_store, None, 0, min_ac=0, max_ac=0) == VS_ERR_NO_DEVICE


def test_wrapper_raises_the_same_codes(host_store):
    ns = host_store.info().num_samples
    cases = ((dict(samples=[]), VS_ERR_ARG), (dict(samples=[0]), VS_ERR_UNKNOWN_SAMPLE), (dict(samples=[ns]), VS_ERR_UNKNOWN_SAMPLE),
             (dict(min_ac=5, max_ac=4), VS_ERR_ARG), (dict(min_ac=5, max_ac=4, samples=[0]), VS_ERR_ARG))
    for kw, code in cases:
        with pytest.raises(VariantStoreError) as e:
            host_store.ld_scores([(1, 100)], **kw)
        assert e.value.code == code, kw
    for kw in (dict(window=-1), dict(window=1 << 32), dict(max_bp=-1), dict(max_bp=1 << 32)):
        with pytest.raises(ValueError):
            host_store.ld_scores([(1, 100)], **kw)
    with pytest.raises(VariantStoreError) as e:
        host_store.ld_scores([])
    assert e.value.code == VS_ERR_ARG


def test_cli_usage_and_host_only_refusal(golden_dir, tmp_path):
    exe = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
    p = subprocess.run([exe, "ldscore"], capture_output=True, text=True)
    assert p.returncode != 0 and "variantstore ldscore " in p.stdout
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    subprocess.run([exe, "construct", "-r", os.path.join(golden_dir, "x.small.fa"), "-v", os.path.join(golden_dir, "x.small.vcf"), "-p", prefix],
                   check=True, capture_output=True)
    p = subprocess.run([exe, "ldscore", "-p", prefix], capture_output=True, text=True)
    assert p.returncode != 0 and "variantstore ldscore " in p.stdout
    p = subprocess.run([exe, "ldscore", "-p", prefix, "-r", "1:100", "--device", "-1"], capture_output=True, text=True)
    q = subprocess.run([exe, "prune", "-p", prefix, "-r", "1:100", "--device", "-1"], capture_output=True, text=True)
    assert p.returncode != 0 and p.returncode == q.returncode
    said, prune_said = (r.stdout + r.stderr for r in (p, q))   # (the log line begins with a time stamp)
    assert "ldscore: no GPU device" in said and said.split("ldscore: ", 1)[1] == prune_said.split("prune: ", 1)[1]


# ------------------------------------------------------------------------------------------- the reference's own definition
def _score(cells, window=0, **kw):
    a = cells.shape[0]
    dropped, pos = kw.pop("dropped", np.zeros(a, bool)), kw.pop("pos", np.arange(a) * 10 + 1)
    return ld_scores(cells, dropped, pos, [0], [a], window, **kw)


def test_reference_quotient():
    # rows (2,1,1,2,0) and (0,0,0,2,0): n = 5, cov = 8, vx = 14, vy = 16: r2 = 64 / 224 = 2 / 7
    assert q32(8, 14, 16) == (2 << 32) // 7 and q32(-8, 14, 16) == q32(8, 14, 16) and q32(0, 14, 16) == 0 and q32(14, 14, 14) == ONE
    m = _cells([[2, 1, 1, 2, 0], [0, 0, 0, 2, 0]])
    sums, n_pairs, state, kb, ns = _score(m)
    assert sums.tolist() == [ONE + (2 << 32) // 7] * 2 and n_pairs.tolist() == [2, 2] and state.tolist() == [SCORED, SCORED]
    assert kb.tolist() == [0, 2] and ns.tolist() == [2] and sums.dtype == np.uint64 and n_pairs.dtype == np.uint32 and state.dtype == np.uint8
    # the largest operands: n = 2^21 - 1 columns stay exact
    n = (1 << 21) - 1
    v = n * (2 * (n // 2) + 2 * (n // 2)) - (2 * (n // 2)) ** 2
    assert q32(v, v, v) == ONE and q32(v - 1, v, v) == ((v - 1) * (v - 1) << 32) // (v * v) < ONE


def test_reference_identical_rows_and_a_monomorphic_row():
    a = [2, 1, 0, 0, 1, 0, 2, 0]
    m = _cells([a, [1] * 8, a, [0] * 8])
    dropped = np.zeros(4, bool)
    sums, n_pairs, state, _kb, ns = _score(m, dropped=dropped)
    # two identical rows: both sums are 2 * 2^32; the monomorphic rows ([1] * 8 has Sxx n = Sx^2) are ineligible and add nothing
    assert sums.tolist() == [2 * ONE, 0, 2 * ONE, 0] and n_pairs.tolist() == [2, 0, 2, 0]
    assert state.tolist() == [SCORED, INELIGIBLE, SCORED, INELIGIBLE] and ns.tolist() == [2]
    dropped[2] = True
    sums, n_pairs, state, _kb, ns = _score(m, dropped=dropped)
    assert sums.tolist() == [ONE, 0, 0, 0] and n_pairs.tolist() == [1, 0, 0, 0] and state.tolist() == [SCORED, INELIGIBLE, DROPPED, INELIGIBLE]
    # the allele-count window makes a row ineligible: ac(a) = 6
    sums, n_pairs, state, _kb, ns = _score(m, min_ac=7)
    assert not sums.any() and not n_pairs.any() and state.tolist() == [INELIGIBLE] * 4 and ns.tolist() == [0]


def test_reference_window_and_distance():
    a = [2, 2, 2, 0, 0, 0, 0, 0]
    x = [0, 0, 0, 0, 2, 0, 2, 0]
    m = _cells([a, x, a])
    rax = q32(8 * 0 - 6 * 4, 8 * 12 - 36, 8 * 8 - 16)
    assert 0 < rax < ONE
    detail = {}
    assert ld_scores(m, np.zeros(3, bool), [1, 11, 21], [0], [3], 0, detail=detail)[0].tolist() == [2 * ONE + rax, ONE + 2 * rax, 2 * ONE + rax]
    assert detail == dict(cut_window=0, cut_bp=0, max_num=(60 * 60) << 32)
    s1 = ld_scores(m, np.zeros(3, bool), [1, 11, 21], [0], [3], 1, detail=detail)
    assert s1[0].tolist() == [ONE + rax, ONE + 2 * rax, ONE + rax] and s1[1].tolist() == [2, 3, 2] and detail["cut_window"] == 2
    assert _score(m, 2)[0].tolist() == _score(m, 0)[0].tolist() == _score(m, 300)[0].tolist()
    s = ld_scores(m, np.zeros(3, bool), [1, 11, 21], [0], [3], 0, 19, detail=detail)
    assert s[0].tolist() == s1[0].tolist() and detail["cut_bp"] == 2 and detail["cut_window"] == 0
    assert ld_scores(m, np.zeros(3, bool), [1, 11, 21], [0], [3], 0, 20)[0].tolist() == [2 * ONE + rax, ONE + 2 * rax, 2 * ONE + rax]
    assert ld_scores(m, np.zeros(3, bool), [1, 11, 21], [0], [3], 0, 9)[0].tolist() == [ONE, ONE, ONE]
    # regions are independent and each gets its own slots: the third row alone, rows 1 .. 2, an empty region
    sums, n_pairs, state, kb, ns = ld_scores(m, np.zeros(3, bool), [1, 11, 21], [0, 2, 1, 0], [3, 1, 2, 0], 0)
    assert kb.tolist() == [0, 3, 4, 6, 6] and ns.tolist() == [3, 1, 2, 0]
    assert sums.tolist() == [2 * ONE + rax, ONE + 2 * rax, 2 * ONE + rax, ONE, ONE + rax, ONE + rax] and n_pairs.tolist() == [3, 3, 3, 1, 2, 2]


def test_reference_text():
    heads = ["10\tA\tC", "10\tA\tG", "12\tT\tTA", "15\tG\tT"]
    text = score_text(heads, [6, 2, 0, 3], [3, 2, 0, 0], [2 * ONE + ONE // 3, ONE + 1, 0, 0], [SCORED, SCORED, INELIGIBLE, DROPPED])
    assert text == ("Pos\tRef\tAlt\tAC\tPairs\tL2\tState\n" "10\tA\tC\t6\t3\t2.333333\tscored\n" "10\tA\tG\t2\t2\t1.000000\tscored\n"
                    "12\tT\tTA\t0\t0\t0.000000\tskip\n")
    assert score_text([], [], [], [], []) == "Pos\tRef\tAlt\tAC\tPairs\tL2\tState\n"


# ------------------------------------------------------------------------ the LD-block cohort is not a vacuous input (oracle, CPU)
def block_ac_window(n_cols):
    """The allele-count window of the LD-block queries: a quarter of the columns up to all of them (of 2 n alleles).  In every
    subset some rows lie below it and some above."""
    return max(1, n_cols // 4), n_cols


def block_cases(names):
    """(subset, window, max_bp, min_ac, max_ac) of every query the GPU test of the LD-block cohort makes."""
    out = []
    for sub in block_subsets(names):
        for window in BLOCK_WINDOWS:
            for max_bp in BLOCK_MAX_BP:
                out.append((sub, window, max_bp, *block_ac_window(len(sub) if sub is not None else len(names))))
    return out


def block_conditions(sums, state, detail, window, max_bp, what):
    """What both the CPU and the GPU test assert of a whole-cohort query over the LD-block cohort."""
    scored = state == SCORED
    ns = int(scored.sum())
    assert ns >= 100, (what, ns)
    assert 10 * int((sums[scored] > 2 * ONE).sum()) >= ns, (what, ns, int((sums[scored] > 2 * ONE).sum()))
    assert (state == INELIGIBLE).any(), what
    if window:
        assert detail["cut_window"] > 0, what
    if max_bp:
        assert detail["cut_bp"] > 0, what


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
    none = np.zeros(parsed.n_rows, bool)
    some_window = some_bp = False
    for sub, window, max_bp, min_ac, max_ac in block_cases(names):
        m = matrix(parsed, sub if sub is not None else names)
        detail = {}
        sums, n_pairs, state, kb, ns = ld_scores(m, none, pos, [0], [parsed.n_rows], window, max_bp, min_ac, max_ac, detail=detail)
        assert kb.tolist() == [0, parsed.n_rows] and int(ns[0]) == int((state == SCORED).sum()) == int(eligible(m, none, min_ac, max_ac).sum())
        assert np.all(n_pairs[state == SCORED] >= 1) and not n_pairs[state != SCORED].any()
        block_conditions(sums, state, detail, window, max_bp, (sub is None or len(sub), window, max_bp, min_ac, max_ac))
        some_window |= bool(window)
        some_bp |= bool(max_bp)
    assert some_window and some_bp
