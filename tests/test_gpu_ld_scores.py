"""LD-score queries on the GPU (vs_query_ld_scores): sums, n_pairs, state, keep_begin and n_scored against tests/ld_score_ref.py --
Python integers -- over the engine's own genotype matrix and over the cells the oracle's type-6 text gives, BIT FOR BIT: there is
no tolerance anywhere but in the one comparison with ld_matrix's float r2 (test_agrees_with_the_ld_matrix, where it is derived).

  1. tile edges          one region of 0 .. 193 rows x every tile-distance cutoff of the window
  2. pitch and k-tail    1 .. 257 columns at about 150 rows
  3. LD-block cohort     three column subsets x windows x max_bp x an allele-count window, in a ragged batch
  4. the family          ld_prune's states and keep_begin, the count query's rows, ld_matrix's r2
  5. beyond 64 bits      8,192 columns: cov^2 2^32 beyond 2^64; 98,304 columns: 2^96 and more
  6. the oracle          golden sweeps and random cohorts under the duplicate rule, with the region text
  7. the engine          repeats, device inputs and pointers, the size limit, interleaving, the temporary matrix, refused accessors,
                         the scan's carry behind 4,096 regions
  8. the CLI"""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_ld_matrix as tm
import test_gpu_ld_prune as tp
from genotype_matrix_ref import matrix
from helpers import random_regions, write_random_cohort
from ld_prune_ref import KEPT, PRUNED, TIE_REF_LEN, row_counts, write_ld_block_cohort, write_tie_cohort
from ld_score_ref import DROPPED, INELIGIBLE, ONE, SCORED, ld_scores, score_text
from test_gpu_ld_band import RTOL, T6_KW
from test_ld_exact_wide_host import WIDE_SAMPLES, WIDE_SEED, WIDE_SITES, WIDE_SUBSET
from test_ld_prune_host import block_subsets
from test_ld_scores_host import BLOCK_MAX_BP, BLOCK_SEED, BLOCK_WINDOWS, block_ac_window, block_cases, block_conditions
from variantstore_amd import DeviceArray, VariantStore
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_ARG, VS_ERR_UNSUPPORTED = -5, -7
UMAX = 0xFFFFFFFF
EDGE_WINDOWS = (0, 1, 63, 64, 65, 128, 300)   # every tile-distance cutoff, and a window wider than any region of the edge test
FIELDS = ("sums", "n_pairs", "state", "keep_begin", "n_scored")


def _same(got, want, what=None):
    sums, n_pairs, state, keep_begin, n_scored = want
    assert got["sums"].dtype == np.uint64 and got["n_pairs"].dtype == np.uint32 and got["state"].dtype == np.uint8, what
    assert got["keep_begin"].dtype == np.uint64 and got["n_scored"].dtype == np.uint64, what
    assert np.array_equal(got["keep_begin"], keep_begin), what
    assert got["state"].shape == state.shape and got["sums"].shape == sums.shape and got["n_pairs"].shape == n_pairs.shape, what
    for name, mine, theirs in (("state", got["state"], state), ("n_pairs", got["n_pairs"], n_pairs), ("sums", got["sums"], sums)):
        bad = np.nonzero(mine != theirs)[0]
        assert bad.size == 0, (what, name, bad[:8].tolist(), mine[bad[:8]].tolist(), theirs[bad[:8]].tolist())
    assert np.array_equal(got["n_scored"], n_scored), what
    assert np.array_equal(got["scores"], got["sums"].astype(np.float64) / ONE), what


def _params(got, ids, window, max_bp, min_ac, max_ac):
    assert got["col_ids"].dtype == np.uint32 and got["col_ids"].tolist() == ids
    assert got["params"] == dict(window=window, max_bp=max_bp, min_ac=min_ac, max_ac=max_ac)
    assert got["counts"].shape == got["rows"].shape


def _check_full(vs, regions, samples, queries, what=None, m=None):
    """Every query (window, max_bp, min_ac, max_ac) of `queries` against the reference over the cells of genotype_matrix() for the
    same regions and samples, every byte.  Returns (the matrix's arrays, cells, dropped, [result dict per query], [detail per query])."""
    if m is None:
        m = tp._matrix_of(vs, regions, samples)
    marr, cells, dropped = m
    outs, details = [], []
    for window, max_bp, min_ac, max_ac in queries:
        res = vs.ld_scores(regions, samples, window=window, max_bp=max_bp, min_ac=min_ac, max_ac=None if max_ac == UMAX else max_ac)
        got = res.ld_scores()
        _params(got, marr["columns"].tolist(), window, max_bp, min_ac, max_ac)
        assert np.array_equal(got["rows"]["pos"], marr["rows"]["pos"])
        some = marr["row_count"] > 0   # (where an empty region "begins" is the engine's business)
        assert np.array_equal(got["row_begin"][some], marr["row_begin"][some]) and np.array_equal(got["row_count"], marr["row_count"])
        detail = {}
        want = ld_scores(cells, dropped, marr["rows"]["pos"], marr["row_begin"], marr["row_count"], window, max_bp, min_ac, max_ac, detail=detail)
        _same(got, want, (what, window, max_bp, min_ac, max_ac, cells.shape))
        assert res.totals()[2] == int(np.count_nonzero(cells))
        for q in range(0, len(regions), max(1, len(regions) // 7)):
            view = res.region_ld_scores(q, got)
            o, e = int(got["keep_begin"][q]), int(got["keep_begin"][q + 1])
            assert view["sums"].shape == (e - o,) and (e == o or np.shares_memory(view["sums"], got["sums"]))
            assert np.array_equal(view["sums"], got["sums"][o:e]) and np.array_equal(view["state"], got["state"][o:e])
        res.close()
        outs.append(got)
        details.append(detail)
    return marr, cells, dropped, outs, details


# ------------------------------------------------------------------------------------------------------------ 1. tile edges
@pytest.fixture(scope="module")
def edge_store():
    vs = tp._pitch_cohort(65)
    spans = tm._spans_by_rows(vs, tm.TILE_EDGES)
    yield vs, spans
    vs.close()


@pytest.mark.parametrize("rows", tm.TILE_EDGES)
def test_tile_edges(edge_store, rows):
    """One region of 0 .. 193 rows -- one to four 64-row tiles, ragged last tiles, 129 and 193 with tile pairs that are not
    neighbours -- under every window in EDGE_WINDOWS: 1 (the diagonal pair and its neighbour only), 63 / 64 / 65 (a tile distance of
    one, with the second tile just reached or not), 128 (two), 300 (wider than the region) and 0 (no limit)."""
    vs, spans = edge_store
    marr, cells, _dropped, outs, details = _check_full(vs, [spans[rows]], None, [(w, 0, 0, UMAX) for w in EDGE_WINDOWS], rows)
    assert cells.shape[0] == rows
    by = dict(zip(EDGE_WINDOWS, outs))
    if rows == 0:
        for got in outs:
            assert got["sums"].shape == (0,) and got["keep_begin"].tolist() == [0, 0] and got["n_scored"].tolist() == [0]
        res = vs.ld_scores([spans[0]])
        assert res.region_text(0) == "Pos\tRef\tAlt\tAC\tPairs\tL2\tState\n" and res.totals()[1:3] == (0, 0)
        dev = res.ld_scores_device()
        assert (dev["n_regions"], dev["n_rows"], dev["n_cols"], dev["n_slots"]) == (1, 0, 65, 0) and dev["keep_begin"]
        res.close()
    else:
        ns = int(by[0]["n_scored"][0])
        assert ns >= rows // 4 and np.array_equal(by[300]["sums"], by[0]["sums"])
        scored = by[0]["state"] == SCORED
        assert np.all(by[0]["n_pairs"][scored] == ns) and np.all(by[0]["sums"][scored] >= ONE)
        if rows >= 15:   # (from the reference's own count: the windows do cut)
            assert dict(zip(EDGE_WINDOWS, details))[1]["cut_window"] > 0 and not np.array_equal(by[1]["sums"], by[0]["sums"])
        if rows >= 129:   # pairs exactly 65 rows apart; from 130 rows on, pairs more than 128 apart
            assert not np.array_equal(by[64]["sums"], by[65]["sums"])
            assert np.array_equal(by[128]["sums"], by[0]["sums"]) == (rows == 129)


# ------------------------------------------------------------------------------------------------------ 2. pitch and k-tail
@pytest.mark.parametrize("n_cols,pitch", [(1, 16), (47, 48), (64, 64), (65, 80), (255, 256), (257, 272)])
def test_pitch_and_k_tail(n_cols, pitch):
    """The k-step tail in all four residues of 64 and one full 256-byte chunk plus a remainder, at three tiles of which the last is
    ragged, and a small region beside it; the whole cohort and a third of it."""
    vs = tp._pitch_cohort(n_cols)
    spans = tm._spans_by_rows(vs, (150, 9))
    regions = [spans[150], spans[9]]
    typical = 40   # bases: about a row per 40 bases in this cohort
    queries = [(0, 0, 0, UMAX), (70, 0, 0, UMAX), (0, 50 * typical, 1, UMAX)]
    marr, cells, _dropped, outs, _details = _check_full(vs, regions, None, queries, n_cols)
    assert marr["row_pitch"] == pitch and cells.shape[1] == n_cols and marr["row_count"].tolist() == [150, 9]
    if n_cols == 1:   # n = 1: no row has a variance
        assert all(not g["sums"].any() and not (g["state"] == SCORED).any() for g in outs)
    else:
        assert int(outs[0]["n_scored"][0]) > 30 and (outs[0]["sums"] > ONE).sum() > 30
    sub = [int(i) for i in np.random.default_rng(n_cols).choice(np.arange(1, n_cols + 1), size=max(1, n_cols // 3), replace=False)]
    _check_full(vs, regions, sub + sub[:2], queries[:2], ("subset", n_cols))
    vs.close()


# -------------------------------------------------------------------------------------------------------- 3. LD-block cohort
def test_ld_block_cohort(tmp_path):
    """The cohort tests/test_ld_scores_host.py shows to be no vacuous input, in a ragged batch: the whole cohort, overlapping regions,
    two identical ones, a region between two sites and a region in front of the first site (empty).  Every subset x window x max_bp of
    block_cases, each with the allele-count window."""
    fasta, vcf, names, last = write_ld_block_cohort(str(tmp_path), BLOCK_SEED)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    rng = np.random.default_rng(5)
    probe = vs.allele_counts([(1, last + 50)])
    pos = np.unique(probe.allele_counts()["rows"]["pos"].astype(np.int64))
    probe.close()
    gap = int(np.argmax(np.diff(pos)))
    assert pos[gap + 1] - pos[gap] > 4 and pos[0] > 3
    overlapping = random_regions(rng, last + 50, 24, max_len=1500)
    regions = [(1, last + 50)] + overlapping[:12] + [(int(pos[gap]) + 1, int(pos[gap + 1]) - 1), (1, int(pos[0]) - 2)] + overlapping[12:] + [overlapping[3]]
    seen = set()
    for sub in block_subsets(names):
        m = tp._matrix_of(vs, regions, sub)
        cases = [c[1:] for c in block_cases(names) if c[0] == sub]
        assert len(cases) == len(BLOCK_WINDOWS) * len(BLOCK_MAX_BP) and all(c[2:] == block_ac_window(m[1].shape[1]) for c in cases)
        marr, cells, dropped, outs, _details = _check_full(vs, regions, sub, cases, ("block", sub is None or len(sub)), m=m)
        assert not dropped.any() and marr["row_count"][14] == 0 and marr["row_count"][0] == cells.shape[0]
        assert np.sum(marr["row_count"]) > cells.shape[0] + 100, "the regions do not overlap"
        for (window, max_bp, min_ac, max_ac), got in zip(cases, outs):
            kb = got["keep_begin"].astype(np.int64)
            n0 = int(marr["row_count"][0])
            # region 0 is the whole cohort: the conditions of the CPU test, on the GPU's own answer
            detail = {}
            ld_scores(cells, dropped, marr["rows"]["pos"], [0], [n0], window, max_bp, min_ac, max_ac, detail=detail)
            block_conditions(got["sums"][:n0], got["state"][:n0], detail, window, max_bp, (sub is None or len(sub), window, max_bp))
            # identical regions have identical slots; an empty region has none
            a, b = 1 + 3, len(regions) - 1
            for f in ("sums", "n_pairs", "state"):
                assert np.array_equal(got[f][kb[a]:kb[a + 1]], got[f][kb[b]:kb[b + 1]]), f
            assert kb[14] == kb[15] and got["n_scored"][14] == 0
            seen.add((window, max_bp))
    assert len(seen) == len(BLOCK_WINDOWS) * len(BLOCK_MAX_BP)
    vs.close()


# ----------------------------------------------------------------------------------------- 4. agreement with the rest of the family
def test_agrees_with_prune_and_counts(edge_store):
    """state == SCORED exactly where ld_prune with the same allele-count window says kept or pruned, DROPPED and INELIGIBLE where it
    does, the same keep_begin; the counts are the count query's rows."""
    vs, spans = edge_store
    regions = tm._ragged(spans) + [spans["long"]]
    for samples in (None, [2, 5, 7, 11, 40, 41, 64]):
        probe = vs.allele_counts(regions, samples)
        ac = probe.allele_counts()
        probe.close()
        alt = ac["counts"]["alt_alleles"]
        lo, hi = int(np.percentile(alt[alt > 0], 30)), int(np.percentile(alt, 90))
        assert 0 < lo < hi
        for kw in (dict(), dict(min_ac=lo, max_ac=hi)):
            res = vs.ld_scores(regions, samples, window=100, max_bp=0, **kw)
            got = res.ld_scores()
            pres = vs.ld_prune(regions, samples, window=64, r2=0.5, **kw)
            pr = pres.ld_prune()
            pres.close()
            assert np.array_equal(got["keep_begin"], pr["keep_begin"]) and got["state"].shape == pr["state"].shape
            assert np.array_equal(got["state"] == SCORED, (pr["state"] == KEPT) | (pr["state"] == PRUNED))
            assert np.array_equal(got["state"] == DROPPED, pr["state"] == tp.DROPPED)
            assert np.array_equal(got["state"] == INELIGIBLE, pr["state"] == tp.INELIGIBLE)
            assert (got["state"] == SCORED).sum() > 50 and (not kw or (got["state"] == INELIGIBLE).any())
            assert np.array_equal(ac["rows"]["pos"], got["rows"]["pos"])
            for f in ("carriers", "alt_alleles", "hom_alt", "phased"):
                assert np.array_equal(got["counts"][f], ac["counts"][f]), (samples, f)
            lay = res.layout()
            assert lay[1] == got["rows"].shape[0] and lay[2] == 0 and lay[3] == 0 and res.fill_ms() > 0
            assert int(got["keep_begin"][-1]) == int(got["row_count"].sum()) == got["sums"].shape[0]
            res.close()


def test_agrees_with_the_ld_matrix(edge_store):
    """sums / 2^32 against the masked row sums of ld_matrix's float r2 of the same regions.  The tolerance is derived, not measured:
    a cell of the matrix is within RTOL = 2^-22 (relative, the band tests' bound) of r2 <= 1, the integer value is below r2 by less
    than 2^-32 (the truncation): n_pairs (2^-22 + 2^-32) per row, the row sums taken in float64."""
    vs, spans = edge_store
    regions = tm._ragged(spans) + [spans["long"]]
    assert RTOL == 2.0 ** -22
    for samples, window, max_bp, kw in ((None, 0, 0, {}), (None, 100, 4000, dict(min_ac=3)), ([2, 5, 7, 11, 40, 41, 64], 70, 0, {})):
        res = vs.ld_scores(regions, samples, window=window, max_bp=max_bp, **kw)
        got = res.ld_scores()
        res.close()
        mres = vs.ld_matrix(regions, samples, stat="r2")
        pos = got["rows"]["pos"].astype(np.int64)
        rows = 0
        for q in range(len(regions)):
            a0, mq, o = int(got["row_begin"][q]), int(got["row_count"][q]), int(got["keep_begin"][q])
            ok = got["state"][o:o + mq] == SCORED
            mask = ok[:, None] & ok[None, :]
            idx = np.arange(mq)
            if window:
                mask &= np.abs(idx[:, None] - idx[None, :]) <= window
            if max_bp:
                mask &= np.abs(pos[a0:a0 + mq, None] - pos[None, a0:a0 + mq]) <= max_bp
            r2 = mres.region_ld_matrix(q).astype(np.float64)
            want = np.where(mask, r2, 0.0).sum(axis=1)
            pairs = mask.sum(axis=1)
            assert np.array_equal(pairs, got["n_pairs"][o:o + mq]), (q, window, max_bp)
            err = np.abs(got["scores"][o:o + mq] - want)
            print(f"region {q}: {mq} rows, largest difference {err.max() if mq else 0:.3e}, bound {(pairs.max() if mq else 0) * (RTOL + 2.0 ** -32):.3e}")
            assert np.all(err <= pairs * (RTOL + 2.0 ** -32)), (q, window, max_bp, float(err.max()))
            rows += int(ok.sum())
        mres.close()
        assert rows > 100
        # the adjusted score is formed from the two exact outputs
        n = len(got["col_ids"])
        assert np.array_equal(got["scores_adj"], got["scores"] - (got["n_pairs"].astype(np.float64) - got["scores"]) / (n - 2))
    one = vs.ld_scores(regions, [3, 9])   # n = 2: no adjusted score
    got = one.ld_scores()
    one.close()
    assert np.isnan(got["scores_adj"]).all() and got["scores_adj"].shape == got["sums"].shape and (got["state"] == SCORED).any()


# ------------------------------------------------------------------------------------------------------ 5. beyond 64 bits
def test_wide_cohort_beyond_64_bits(tmp_path):
    """The wide LD-block cohort of test_gpu_ld_exact_wide.py: 8,192 samples, and a subset of 4,099 ids (a pitch tail of the k loop).
    v is at most n^2 = 2^26 there, so cov^2 2^32 reaches 2^84 -- far beyond 64 bits, asserted from the reference -- but never 2^96:
    that takes v of 2^32, 92,682 columns or more (test_tie_cohort_reaches_2_to_the_96)."""
    fasta, vcf, _names, last = write_ld_block_cohort(str(tmp_path), WIDE_SEED, n_sites=WIDE_SITES, n_samples=WIDE_SAMPLES, p_two_alt=0)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    assert vs.info().num_samples - 1 == WIDE_SAMPLES
    subset = sorted(int(i) for i in np.random.default_rng(9).choice(np.arange(1, WIDE_SAMPLES + 1), size=WIDE_SUBSET, replace=False))
    regions = [(1, last + 50), (last // 3, 2 * last // 3), (1, last // 2)]
    for sub, queries in ((None, [(0, 0, 0, UMAX), (16, 0, 0, UMAX)]), (subset, [(0, 200, 0, UMAX)])):
        marr, cells, _dropped, outs, details = _check_full(vs, regions, sub, queries, ("wide", sub is None))
        assert cells.shape[0] >= WIDE_SITES and cells.shape[1] == (WIDE_SAMPLES if sub is None else WIDE_SUBSET)
        for got, detail in zip(outs, details):
            assert detail["max_num"] >= 1 << 72, detail["max_num"].bit_length()
            assert (got["sums"] > 2 * ONE).sum() > 50
    vs.close()


def test_tie_cohort_reaches_2_to_the_96(tmp_path):
    """Some summed pair has cov^2 2^32 >= 2^96 -- asserted here, from the reference.  That takes v >= 2^32 and so more columns than
    8,192: the tie cohort (ld_prune_ref.write_tie_cohort, the other wide builder of test_gpu_ld_exact_wide.py) at 98,304 samples,
    where the rows of the pattern (0, 1, 1, 2) have v = n^2 / 2 = 2^32.17.  Its pairs have r2 = 1/16 .. 1 exactly, with both signs of
    cov: the quotients are exact multiples, where an estimate that is off by one shows.  The whole reference, every pair alone, an
    empty region; then 49,152 of the columns, in whole patterns."""
    n = 98_304
    fasta, vcf, _names, pos, _fractions, d, source = write_tie_cohort(str(tmp_path), n, 5)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    assert vs.info().num_samples - 1 == n
    regions = [(1, TIE_REF_LEN + 1)] + [(int(pos[2 * k]) - 50, int(pos[2 * k + 1]) + 50) for k in range(d.shape[0] // 2)] + [(1, 40)]
    subset = [int(c) + 1 for c in np.nonzero(np.asarray(source) < n // 2)[0]]   # column c is id c + 1
    for sub, queries in ((None, [(0, 0, 0, UMAX), (3, 250, 0, UMAX)]), (subset, [(0, 0, 0, UMAX)])):
        marr, cells, dropped, outs, details = _check_full(vs, regions, sub, queries, ("tie", sub is None))
        assert cells.shape == (d.shape[0], n if sub is None else n // 2) and not dropped.any()
        if sub is None:
            assert np.array_equal(cells != 0, d != 0)
            assert all(detail["max_num"] >= 1 << 96 for detail in details), [detail["max_num"].bit_length() for detail in details]
        got = outs[0]
        assert got["n_scored"].tolist() == [d.shape[0]] + [2] * (d.shape[0] // 2) + [0]
        kb = got["keep_begin"].astype(np.int64)
        two = [got["sums"][kb[1 + k]:kb[2 + k]].tolist() for k in range(d.shape[0] // 2)]
        assert two[-1] == [2 * ONE, 2 * ONE] and two[-2] == [2 * ONE, 2 * ONE]           # r2 = 1, cov > 0 and cov < 0
        assert two[3] == [ONE + ONE // 4, ONE + ONE // 4] and two[0] == [ONE + ONE // 16, ONE + ONE // 16]
    vs.close()


# ---------------------------------------------------------------------------------------------------------- 6. against the oracle
def _check_oracle(vs, regions, parsed, valid, samples, window, max_bp, text_every=1, **kw):
    """The slots of every region the oracle answers, from the cells its type-6 text gives, and the text of every text_every-th
    region.  Returns the result dict."""
    ids, names = tp._columns(vs, samples)
    want_m = matrix(parsed, names)
    res = vs.ld_scores(regions, samples, window=window, max_bp=max_bp, **kw)
    got = res.ld_scores()
    min_ac, max_ac = kw.get("min_ac", 0), UMAX if kw.get("max_ac") is None else kw["max_ac"]
    _params(got, ids, window, max_bp, min_ac, max_ac)
    rows = got["rows"]
    a_all = rows.shape[0]
    dropped = (rows["count_flags"] >> 31) != 0
    cells = np.zeros((a_all, len(names)), np.uint8)
    heads = [None] * a_all
    for q in valid:
        a = np.arange(int(got["row_begin"][q]), int(got["row_begin"][q]) + int(got["row_count"][q]))
        a = a[~dropped[a]]
        r0 = int(parsed.row_begin[q])
        assert a.shape[0] == int(parsed.row_count[q]), (q, regions[q])
        cells[a] = want_m[r0:r0 + a.shape[0]]
        for k, i in enumerate(a):
            heads[i] = parsed.heads[r0 + k]
            assert int(heads[i].split("\t")[0]) == int(rows["pos"][i])
    want = ld_scores(cells, dropped, rows["pos"], got["row_begin"], got["row_count"], window, max_bp, min_ac, max_ac)
    assert np.array_equal(got["keep_begin"], want[3])
    ac = row_counts(cells)[0]
    for q in valid:
        o0, o1 = int(want[3][q]), int(want[3][q + 1])
        for k, f in enumerate(("sums", "n_pairs", "state")):
            assert np.array_equal(got[f][o0:o1], want[k][o0:o1]), (f, q, regions[q], samples, window, max_bp)
        assert int(got["n_scored"][q]) == int(want[4][q]), (q, regions[q])
    for q in valid[::text_every] if text_every else ():
        a0, m = int(got["row_begin"][q]), int(got["row_count"][q])
        o0 = int(want[3][q])
        text = score_text(heads[a0:a0 + m], ac[a0:a0 + m], want[1][o0:o0 + m], want[0][o0:o0 + m], want[2][o0:o0 + m])
        assert res.region_text(int(q)) == text, (q, regions[q])
    res.close()
    return got


@pytest.mark.parametrize("stem", ["x", "x.small"])
def test_golden_region_sweeps(stem, golden_dir, tmp_path):
    fasta, vcf = os.path.join(golden_dir, stem + ".fa"), os.path.join(golden_dir, stem + ".vcf")
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = tp._oracle(vs, tmp_path)
    n_samples = vs.info().num_samples - 1
    rng = np.random.default_rng(11)
    regions = random_regions(rng, tp._ref_len(fasta), 200)   # unsorted: the device sorts the batch
    parsed, valid = tp._parse(orc, regions)
    _check_oracle(vs, regions, parsed, valid, None, 0, 1_000_000)
    _check_oracle(vs, regions, parsed, valid, None, 3, 0, text_every=3)
    srt = sorted(regions)
    _check_oracle(vs, srt, *tp._parse(orc, srt), None, 70, 500, text_every=3)
    _check_oracle(vs, regions, parsed, valid, [vs.sample_name(1)], 0, 0, text_every=5, min_ac=1)   # by name
    for k in range(2):
        ids = rng.choice(np.arange(1, n_samples + 1), size=int(rng.integers(1, n_samples + 1)), replace=False)
        ids = [int(i) for i in ids] + [int(i) for i in ids[:2]]   # duplicates collapse
        _check_oracle(vs, regions, parsed, valid, ids, (2, 0)[k], (0, 40)[k], text_every=4, min_ac=k)
    vs.close()


@pytest.mark.parametrize("seed", [721, 722])
def test_random_cohorts_with_duplicate_rule(seed, tmp_path):
    fasta, vcf, names = write_random_cohort(str(tmp_path), seed, ref_len=6000, n_rows=400, n_samples=9, p_near=0.6, p_multi=0.3,
                                            p_same=0.3, unphased_p=0.4 if seed % 2 else 0.05)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = tp._oracle(vs, tmp_path)
    rng = np.random.default_rng(seed)
    regions = random_regions(rng, 6000, 300, max_len=900)
    parsed, valid = tp._parse(orc, regions)
    subsets = [None] + [[vs.sample_id(s) for s in rng.choice(names, size=int(rng.integers(3, len(names))), replace=False)] for _ in range(2)]
    for sub, window, max_bp in zip(subsets, (0, 7, 0), (0, 0, 150)):
        got = _check_oracle(vs, regions, parsed, valid, sub, window, max_bp, text_every=6)
        assert (got["state"] == DROPPED).any(), "no region of the batch falls under the duplicate rule"
        assert (got["state"] == SCORED).any() and (got["sums"] > ONE).any()
    vs.close()


# ------------------------------------------------------------------------------------------------------ 7. engine behaviour
@pytest.fixture(scope="module")
def t6_store():
    vs = VariantStore.synthetic(device=0, **T6_KW)
    rng = np.random.default_rng(12)
    s = np.sort(rng.integers(1_000, 7_990_000, size=3_000))
    regions = np.stack([s, s + rng.integers(50, 3_000, size=3_000)], axis=1).astype(np.uint64)
    yield vs, regions
    vs.close()


def test_identical_calls_give_identical_bytes(t6_store):
    vs, regions = t6_store
    batch = np.ascontiguousarray(regions[:1_500])
    first = None
    for _ in range(3):
        res = vs.ld_scores(batch, window=100, max_bp=20_000, min_ac=3)
        got = res.ld_scores()
        res.close()
        if first is None:
            first = got
            assert (got["sums"] > ONE).sum() > 1_000
        for k in FIELDS:
            assert got[k].tobytes() == first[k].tobytes(), k
    # and they are the reference's bytes, over the engine's own matrix (a sixth of the batch: the reference is Python integers)
    _check_full(vs, np.ascontiguousarray(regions[:250]), None, [(100, 20_000, 3, UMAX)], "t6")
    _check_full(vs, np.ascontiguousarray(regions[:250]), [2, 3, 150, 151, 299], [(0, 1_000_000, 0, UMAX)], "t6 subset")


def test_device_regions_and_device_pointers(t6_store):
    """Regions in device memory and the device accessor.  Sample ids are a host list, as for the other LD queries."""
    torch = pytest.importorskip("torch")
    vs, regions = t6_store
    sub = [3, 17, 40, 200, 250, 251]
    batch = np.ascontiguousarray(regions[:2_500])
    host = vs.ld_scores(batch, sub, window=32)
    hgot = host.ld_scores()
    t = torch.from_numpy(batch.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    dev = vs.ld_scores(DeviceArray(t.data_ptr(), batch.shape[0]), sub, window=32)
    dgot = dev.ld_scores()
    for k in ("col_ids", "row_begin", "row_count", "counts") + FIELDS:
        assert np.array_equal(hgot[k], dgot[k]), k
    assert (hgot["sums"] > ONE).any() and (hgot["state"] == INELIGIBLE).any()
    p = dev.ld_scores_device()
    total = dgot["state"].shape[0]
    nq, a = p["n_regions"], p["n_rows"]
    assert (nq, a, p["n_cols"], p["n_slots"]) == (2_500, dgot["rows"].shape[0], 6, total)
    assert all(p[k] for k in ("sums", "n_pairs", "state", "keep_begin", "n_scored", "counts"))
    first = tp._read_device(torch, p["sums"], 8 * total)
    later = vs.ld_scores(regions[2_500:2_900], window=8)   # a later batch on the same handle leaves the sums alone
    later.totals()
    assert np.array_equal(first.view(np.uint64), dgot["sums"])
    assert np.array_equal(tp._read_device(torch, p["sums"], 8 * total), first)
    assert np.array_equal(tp._read_device(torch, p["n_pairs"], 4 * total).view(np.uint32), dgot["n_pairs"])
    assert np.array_equal(tp._read_device(torch, p["state"], total), dgot["state"])
    assert np.array_equal(tp._read_device(torch, p["keep_begin"], 8 * (nq + 1)).view(np.uint64), dgot["keep_begin"])
    assert np.array_equal(tp._read_device(torch, p["n_scored"], 8 * nq).view(np.uint64), dgot["n_scored"])
    assert np.array_equal(tp._read_device(torch, p["counts"], a * 16).view(np.uint32).reshape(a, 4), dgot["counts"].view(np.uint32).reshape(a, 4))
    later.close(); host.close(); dev.close()


def test_size_limit(t6_store):
    vs, regions = t6_store
    warm = vs.allele_counts(regions)   # the plan's temporaries, the table and the counts of this batch are in the handle's pool afterwards
    wgot = warm.allele_counts()
    a, slots = wgot["rows"].shape[0], int(wgot["row_count"].sum())
    warm.close()
    c = vs.info().num_samples - 1
    pitch = (c + 15) // 16 * 16
    matrix_bytes = a * pitch
    assert matrix_bytes > 1 << 20
    vs.set_option("matrix_max_mib", 1)
    try:
        before = vs.info().pool_mallocs
        with pytest.raises(VariantStoreError) as e:
            vs.ld_scores(regions)
        assert e.value.code == VS_ERR_ARG
        msg = str(e.value)
        for what in ("LD scores", f"{regions.shape[0]} regions", f"{a} rows", f"{c} columns", str(matrix_bytes), " bytes", "matrix_max_mib"):
            assert what in msg, (what, msg)
        assert vs.info().pool_mallocs == before, "the refused batch allocated"
        few = vs.ld_scores(regions[:20], [1, 2, 3], window=2)   # 16 bytes a row and 13 a slot: below the limit
        assert few.ld_scores()["keep_begin"].shape == (21,)
        few.close()
        # 16 bytes of matrix a row: the matrix alone fits, with 13 bytes a slot and 24 a region the whole does not -- known only
        # once the scan has counted the slots
        part = np.ascontiguousarray(regions[:2_000])
        vs.set_option("matrix_max_mib", 0)
        warm = vs.allele_counts(part)
        wgot = warm.allele_counts()
        pa, pslots = wgot["rows"].shape[0], int(wgot["row_count"].sum())
        warm.close()
        vs.set_option("matrix_max_mib", 1)
        region_bytes = 8 * (3 * (part.shape[0] + 1) + 6)
        assert pa * 16 + region_bytes <= 1 << 20 < pa * 16 + 13 * pslots + region_bytes, (pa, pslots)
        with pytest.raises(VariantStoreError) as e:
            vs.ld_scores(part, [1, 2, 3])
        assert e.value.code == VS_ERR_ARG and f"{pa} rows" in str(e.value) and str(13 * pslots) in str(e.value) and str(pa * 16) in str(e.value)
    finally:
        vs.set_option("matrix_max_mib", 0)
    again = vs.ld_scores(regions)   # the handle stays usable
    got = again.ld_scores()
    assert got["state"].shape == (slots,) and (got["sums"] > ONE).any()
    again.close()


def test_interleaving_leaves_type6_alone():
    rng = np.random.default_rng(12)
    batches = []
    for k in range(6):
        n = 3_000 + 200 * k + (4_000 if k == 4 else 0)   # like batches (speculated), one larger (refused / re-sized)
        s = np.sort(rng.integers(1_000, 7_990_000, size=n))
        batches.append(np.stack([s, s + rng.integers(50, 3_000, size=n)], axis=1).astype(np.uint64))
    shuffled = batches[3][rng.permutation(batches[3].shape[0])]

    def run(with_scores):
        vs = VariantStore.synthetic(device=0, **T6_KW)
        digests = []
        for k, b in enumerate(batches):
            r = vs.get_var_in_ref(b)
            if with_scores:   # LD-score batches in between: sorted, unsorted, with a subset
                l1 = vs.ld_scores(b, window=16)
                l2 = vs.ld_scores(shuffled)
                l3 = vs.ld_scores(shuffled, [1, 5, 7, 200], window=100, max_bp=5_000)
                for ld in (l1, l2, l3):
                    ld.totals()
                    ld.close()
            digests.append(r.digest())
            r.close()
        info = vs.info()
        out = (digests, info.t6_speculated, info.t6_refused)
        vs.close()
        return out

    plain, mixed = run(False), run(True)
    assert plain[1] > 0, "the type-6 batches were not speculated"
    assert plain == mixed


def test_temporary_matrix_leaves_an_open_result():
    """The temporary genotype matrix is not part of the result: once a result has been read (its kernels have finished) the matrix
    is back in the handle's pool while the result is still open, and a second whole-cohort batch beside it takes that buffer.  The
    shape of test_gpu_ld_matrix's test: 3,000 columns, 150 regions of about ten rows, so the matrix is far larger than any other
    buffer of the batch."""
    vs = VariantStore.synthetic(device=0, ref_length=60_000, num_variants=1500, num_samples=3_000, seed=77, first_pos=100, frac_ins=0.06,
                                frac_del=0.06, frac_multi=0.03, max_indel=4, af_exponent=2.5)
    regions = [(1 + 400 * k, 400 * (k + 1)) for k in range(150)]
    warm = [vs.ld_scores(regions, [1]) for _ in range(3)]
    for w in warm:
        w.ld_scores()
        w.close()
    m0 = vs.info().pool_mallocs
    first = vs.ld_scores(regions)
    got = first.ld_scores()   # (waits for the batch)
    a = got["rows"].shape[0]
    assert a >= 1400 and vs.info().pool_mallocs > m0, "the whole-cohort matrix must have been a new buffer"
    m1 = vs.info().pool_mallocs
    second = vs.ld_scores(regions, window=3)   # beside the open result
    other = second.ld_scores()
    assert vs.info().pool_mallocs == m1, "the open result still holds its temporary matrix"
    # both results are whole and their own: the second batch ran in the first's matrix buffer, not in anything the first still reads
    m = tp._matrix_of(vs, regions)
    for mine, window in ((first.ld_scores(), 0), (other, 3)):
        _same(mine, ld_scores(m[1], m[2], m[0]["rows"]["pos"], m[0]["row_begin"], m[0]["row_count"], window, 1_000_000), window)
    dev = first.ld_scores_device()
    assert (dev["n_regions"], dev["n_rows"], dev["n_cols"]) == (150, a, 3_000) and dev["sums"]
    first.close(); second.close()
    vs.close()


def test_refused_accessors(t6_store):
    vs, regions = t6_store
    r = vs.ld_scores(regions[:1_000], window=8)
    for call in (lambda: r.raw(with_carriers=True), lambda: r.view(with_carriers=True), r.digest, r.num_header_records,
                 r.num_region_records):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_UNSUPPORTED
    for call in (r.allele_counts, r.sample_burden, r.sample_burden_device, r.genotype_matrix, r.genotype_matrix_device, r.ld_band,
                 r.ld_band_device, r.ld_matrix, r.ld_matrix_device, r.ld_prune, r.ld_prune_device, r.ld_clump, r.ld_clump_device,
                 r.sample_gram, r.sample_ibs):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_ARG
    r.view(with_carriers=False)
    raw = r.raw(with_carriers=False)
    t6 = vs.get_var_in_ref(regions[:1_000])
    raw6 = t6.raw(with_carriers=False)
    for f in ("pos", "ref_off", "ref_len", "alt_off", "alt_len", "count_flags"):
        assert np.array_equal(raw["rows"][f], raw6["rows"][f]), f
    assert np.array_equal(raw["region_flags"], raw6["region_flags"]) and np.array_equal(raw["row_count"], raw6["row_count"])
    assert r.totals()[:2] == t6.totals()[:2]
    r.close()
    for res in (t6, vs.allele_counts(regions[:10]), vs.sample_burden(regions[:10]), vs.genotype_matrix(regions[:10]),
                vs.ld_band(regions[:10], window=4), vs.ld_matrix(regions[:10]), vs.ld_prune(regions[:10]), vs.sample_gram(regions[:10])):
        for call in (res.ld_scores, res.ld_scores_device, lambda: res.region_ld_scores(0)):
            with pytest.raises(VariantStoreError) as e:
                call()   # not an LD-score result
            assert e.value.code == VS_ERR_ARG
        res.close()


def test_scan_carry_behind_4096_regions(edge_store):
    """4,096 + 204 short regions and a 193-row region behind them: keep_begin and the workgroups' prefix behind the first 4,096
    regions, which the scan writes with a carried total."""
    vs, spans = edge_store
    rng = np.random.default_rng(41)
    L = vs.info().ref_length
    s = rng.integers(1, L - 400, size=4_300)
    regions = [(int(x), int(x) + int(w)) for x, w in zip(s, rng.integers(1, 300, size=4_300))] + [spans[193], spans[0], spans[65]]
    marr, _cells, _dropped, outs, _details = _check_full(vs, regions, None, [(0, 0, 0, UMAX), (64, 3_000, 0, UMAX)], "carry")
    assert marr["row_count"][4_300] == 193 and marr["row_count"][:4_300].sum() > 10_000 and (marr["row_count"][:4_300] == 0).any()
    assert int(outs[0]["keep_begin"][4_096]) > 0 and (outs[0]["sums"][int(outs[0]["keep_begin"][4_300]):] > ONE).any()


# ------------------------------------------------------------------------------------------------------------------ 8. the CLI
def test_cli_ldscore(tmp_path):
    """The LD-block cohort through `variantstore construct` and `variantstore ldscore`: the text is the reference's text over the
    engine's own matrix, and the library's."""
    exe = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    fasta, vcf, _names, last = write_ld_block_cohort(str(tmp_path), BLOCK_SEED)
    subprocess.run([exe, "construct", "-r", fasta, "-v", vcf, "-p", prefix], check=True, capture_output=True)
    vs = VariantStore.open(prefix, device=0)
    rng = np.random.default_rng(2)
    regions = sorted(random_regions(rng, last + 50, 60, max_len=1500))
    regions = [(x, y) for x, y in regions if x >= 1]
    rfile = os.path.join(tmp_path, "regions.txt")
    with open(rfile, "w") as f:
        f.write("".join(f"{x}:{y}\n" for x, y in regions))
    names = [vs.sample_name(i) for i in range(1, min(8, vs.info().num_samples))]
    sfile = os.path.join(tmp_path, "samples.txt")
    with open(sfile, "w") as f:
        f.write("\n".join(names) + "\n")
    some = False
    for samples, extra in ((None, []), (names, ["-S", sfile])):
        marr, cells, dropped = tp._matrix_of(vs, regions, samples)
        ac = row_counts(cells)[0]
        heads = [f"{int(v['pos'])}\t{ref}\t{alt}" for v, (ref, alt) in zip(marr["rows"], _alleles(vs, regions))]
        for kw, flags in ((dict(), []), (dict(window=3, max_bp=0), ["-w", "3", "--bp", "0"]), (dict(max_bp=40), ["--bp", "40"]),
                          (dict(window=256, min_ac=1, max_ac=3), ["--window", "256", "--min-ac", "1", "--max-ac", "3"])):
            out = os.path.join(tmp_path, "ldscore.txt")
            subprocess.run([exe, "ldscore", "-p", prefix, "-r", "@" + rfile, "-o", out] + extra + flags, check=True, capture_output=True)
            with open(out, "rb") as f:
                parts = f.read().decode("latin-1").split("#region ")[1:]
            res = vs.ld_scores(regions, samples, **kw)
            want = ld_scores(cells, dropped, marr["rows"]["pos"], marr["row_begin"], marr["row_count"], kw.get("window", 0),
                             kw.get("max_bp", 1_000_000), kw.get("min_ac", 0), kw.get("max_ac", UMAX))
            assert len(parts) == len(regions)
            for q, part in enumerate(parts):
                head, text = part.split("\n", 1)
                assert head == f"{q} {regions[q][0]}:{regions[q][1]}"
                a0, m, o = int(marr["row_begin"][q]), int(marr["row_count"][q]), int(want[3][q])
                assert text == score_text(heads[a0:a0 + m], ac[a0:a0 + m], want[1][o:o + m], want[0][o:o + m], want[2][o:o + m]), (q, kw)
                assert text == res.region_text(q), (q, kw)
                some |= "\tscored\n" in text and "\tskip\n" in text
            res.close()
    assert some
    p = subprocess.run([exe, "ldscore", "-p", prefix, "-r", "@" + rfile, "--min-ac", "3", "--max-ac", "2"], capture_output=True, text=True)
    assert p.returncode != 0
    vs.close()


def _alleles(vs, regions):
    """(ref, alt) of every table row of the batch, from the count query's region text (dropped rows have no line: the LD-block cohort
    has none)."""
    res = vs.allele_counts(regions)
    got = res.allele_counts()
    out = [None] * got["rows"].shape[0]
    for q in range(len(regions)):
        a0 = int(got["row_begin"][q])
        lines = [ln for ln in res.region_text(q).split("\n")[1:] if ln]
        assert len(lines) == int(got["row_count"][q])
        for k, ln in enumerate(lines):
            f = ln.split("\t")
            assert int(f[0]) == int(got["rows"]["pos"][a0 + k])
            out[a0 + k] = (f[1], f[2])
    res.close()
    assert all(x is not None for x in out)
    return out
