"""LD clumping queries on the GPU (vs_query_ld_clump): the verdicts and owners against what the oracle's type-6 text gives, against
the engine's own genotype matrix byte for byte (every mask-word and column-tile edge of the window, on both sides of a row; regions
around 64 rows and beyond the workgroup's 1024 threads), the table-order family against vs.ld_prune on the device (also the deep
chain: many rounds), the independence of the regions, the thresholds, repeated calls, buffers that come from the pool, interleaving
with type-6 batches, regions in device memory, the device pointers, the size limit, the number of p-values, the refused accessors
and the CLI.

state, owner, keep_begin and n_index are compared byte for byte with tests/ld_clump_ref.py: there is no tolerance anywhere.  The
kernel has one path for every region size (states and masks in HBM), so there is no size threshold to straddle; the region sizes
are chosen around the 64 rows of a wave and the 1024 threads of the workgroup."""
import os
import subprocess

import numpy as np
import pytest

from genotype_matrix_ref import Parsed, matrix
from helpers import oracle_texts, random_regions, write_random_cohort
from ld_clump_ref import (DROPPED, INDEX, INELIGIBLE, MEMBER, NO_OWNER, UNCLUMPED, classes, clump_states, clump_text, key_of, keys_of,
                          pvalue_families, region_hits, window_hits)
from ld_prune_ref import KEPT, ONE, hit_band, row_counts, write_ld_block_cohort
from oracle.oracle import Oracle
from test_gpu_genotype_matrix import _read_device as _read_device_bytes
from test_ld_clump_host import BLOCK_SEED, BLOCK_WINDOWS, CONDITION_THRESHOLDS, P_SEED, clump_conditions
from variantstore_amd import DeviceArray, VariantStore, pvalue_keys, quantise_r2
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_ARG, VS_ERR_UNSUPPORTED = -5, -7
WINDOWS = (1, 16, 17, 31, 32, 33, 64, 100, 256)
NAN = float("nan")


def _oracle(vs, tmp_path, name="plain.bin"):
    plain = os.path.join(tmp_path, name)
    vs.export_plain(plain)
    return Oracle(plain)


def _ref_len(fasta):
    with open(fasta) as f:
        return sum(len(line.strip()) for line in f if not line.startswith(">"))


def _parse(orc, regions):
    want = oracle_texts(orc, regions)
    valid = [q for q, (n, _e, _t) in enumerate(want) if n >= 0]
    assert valid
    return Parsed([t if n >= 0 else None for n, _e, t in want]), np.asarray(valid)


def _columns(vs, samples):
    ids = (list(range(1, vs.info().num_samples)) if samples is None
           else sorted({vs.sample_id(i) if isinstance(i, str) else int(i) for i in samples}))
    return ids, [vs.sample_name(i) for i in ids]


def _table_rows(vs, regions):
    """The number of table rows of a batch: what the p-values are laid out over."""
    res = vs.allele_counts(regions)
    a = res.allele_counts()["rows"].shape[0]
    res.close()
    return a


def _same(got, want, what=None):
    state, owner, keep_begin, n_index = want
    assert got["state"].dtype == np.uint8 and got["owner"].dtype == np.uint32, what
    assert got["keep_begin"].dtype == np.uint64 and got["n_index"].dtype == np.uint64, what
    assert np.array_equal(got["keep_begin"], keep_begin), what
    for k, w in (("state", state), ("owner", owner)):
        bad = np.nonzero(got[k] != w)[0] if got[k].shape == w.shape else None
        assert bad is not None and bad.size == 0, (what, k, None if bad is None else [(int(i), int(got[k][i]), int(w[i])) for i in bad[:8]])
    assert np.array_equal(got["n_index"], n_index), what
    assert got["rounds"].shape == n_index.shape and np.all((got["rounds"] > 0) == (got["row_count"] > 0)), what


def _params(got, ids, p, window, T, p1, p2, max_bp=0):
    assert got["columns"].dtype == np.uint32 and got["columns"].tolist() == ids
    assert (got["window"], got["threshold_q20"], got["max_bp"]) == (window, T, max_bp)
    assert got["threshold"] == T / ONE and got["counts"].shape == got["rows"].shape
    assert (got["p1"], got["p2"], got["p1_key"], got["p2_key"]) == (abs(p1), abs(p2), key_of(p1), key_of(p2))
    assert np.array_equal(got["pvalues"], np.asarray(p, np.float64), equal_nan=True)


def _clumps_of(heads, p, keys, state_q, owner_q, a0):
    """region_clumps by the definition: ((pos, ref, alt), p, [members in table order]) per index row, in priority order."""
    def name(x):
        pos, ref, alt = heads[a0 + x].split("\t")
        return (int(pos), ref, alt)
    index = np.nonzero(state_q == INDEX)[0]
    order = index[np.lexsort((index, keys[a0 + index]))]
    return [(name(x), float(p[a0 + x]), [name(y) for y in np.nonzero((state_q == MEMBER) & (owner_q == x))[0]]) for x in order]


# ------------------------------------------------------------------------------------------------ 1. against the oracle
def _check_oracle(vs, regions, parsed, valid, samples, p, window, T, p1, p2, text_every=1, max_bp=0, cache=None):
    """The verdicts of every region the oracle answers, from the cells its type-6 text gives, and the text and the clumps of every
    text_every-th region.  `cache`: a dict that keeps the oracle's cells per column set between calls over the same `parsed`.
    Returns (result dict, the table's cells by the oracle, the hit band, the expected answer)."""
    ids, names = _columns(vs, samples)
    cache = {} if cache is None else cache
    if tuple(names) not in cache:
        cache[tuple(names)] = matrix(parsed, names)
    want_m = cache[tuple(names)]
    res = vs.ld_clump(regions, p, samples, window=window, r2=T / ONE, max_bp=max_bp, p1=p1, p2=p2)
    got = res.ld_clump()
    _params(got, ids, p, window, T, p1, p2, max_bp)
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
    band = hit_band(cells, window, T)
    keys = keys_of(p)
    want = clump_states(cells, dropped, rows["pos"], got["row_begin"], got["row_count"], keys, window, T, key_of(p1), key_of(p2), max_bp, band=band)
    assert np.array_equal(got["keep_begin"], want[2])
    ac = row_counts(cells)[0]
    for q in valid:
        o0, o1 = int(want[2][q]), int(want[2][q + 1])
        assert np.array_equal(got["state"][o0:o1], want[0][o0:o1]), (q, regions[q], samples, window, T)
        assert np.array_equal(got["owner"][o0:o1], want[1][o0:o1]), (q, regions[q], samples, window, T)
        assert int(got["n_index"][q]) == int(want[3][q]), (q, regions[q])
    for q in valid[::text_every] if text_every else ():
        a0, m = int(got["row_begin"][q]), int(got["row_count"][q])
        o0 = int(want[2][q])
        text = clump_text(heads[a0:a0 + m], ac[a0:a0 + m], p[a0:a0 + m], want[0][o0:o0 + m], want[1][o0:o0 + m])
        assert res.region_text(int(q)) == text, (q, regions[q])
        assert res.region_clumps(int(q)) == _clumps_of(heads, p, keys, want[0][o0:o0 + m], want[1][o0:o0 + m], a0), (q, regions[q])
    res.close()
    return got, cells, band, want


def block_subsets(names):
    return (None, names[:17], names[5:40:3])


def test_ld_block_cohort_against_the_oracle(tmp_path):
    fasta, vcf, names, last = write_ld_block_cohort(str(tmp_path), BLOCK_SEED)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(5)
    regions = [(1, last + 50)] + random_regions(rng, last + 50, 40, max_len=1500)
    parsed, valid = _parse(orc, regions)
    assert 0 in valid
    a = _table_rows(vs, regions)
    assert a == 316
    families = pvalue_families(a, P_SEED)
    some_unclumped = False
    cache = {}
    for sub in block_subsets(names):
        for T in ((0,) + CONDITION_THRESHOLDS + (ONE,)) if sub is None else (0, CONDITION_THRESHOLDS[1]):
            for window in BLOCK_WINDOWS:
                # every family at window 4 (the subsets: at one threshold), the uniform one everywhere
                for name, p, p1, p2 in families if window == 4 and (sub is None or T) else families[:1]:
                    got, cells, band, want = _check_oracle(vs, regions, parsed, valid, sub, p, window, T, p1, p2, text_every=7, cache=cache)
                    some_unclumped |= bool((got["state"] == UNCLUMPED).any())
                    if name != "uniform" or sub is not None or T == 0:
                        continue
                    m = int(got["row_count"][0])   # region 0 is the whole cohort: the conditions of the CPU test, on the GPU's verdicts
                    assert int(got["row_begin"][0]) == 0 and m == a
                    dropped = (got["rows"]["count_flags"] >> 31) != 0
                    assert not dropped.any(), "the LD-block cohort has no row under the duplicate rule"
                    keys = keys_of(p)
                    _cand, lead = classes(cells, dropped, keys, key_of(p1), key_of(p2))
                    hits = region_hits(window_hits(band, got["rows"]["pos"], window), 0, a, window)
                    clump_conditions(got["state"][:m], got["owner"][:m], keys, lead, hits, T, (T, window))
    assert some_unclumped
    vs.close()


@pytest.mark.parametrize("stem", ["x", "x.small"])
def test_golden_region_sweeps(stem, golden_dir, tmp_path):
    fasta, vcf = os.path.join(golden_dir, stem + ".fa"), os.path.join(golden_dir, stem + ".vcf")
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(11)
    regions = random_regions(rng, _ref_len(fasta), 200)   # unsorted: the device sorts the batch
    parsed, valid = _parse(orc, regions)
    a = _table_rows(vs, regions)
    p = rng.random(a)
    cache = {}
    for samples, window, T in ((None, 64, quantise_r2(0.2)), ([1], 3, 0), ([vs.sample_name(1)], 256, ONE)):
        got, _c, _b, _w = _check_oracle(vs, regions, parsed, valid, samples, p, window, T, 1.0, 1.0, text_every=9, cache=cache)
        assert np.all((got["state"] == INELIGIBLE) | (got["state"] == DROPPED)) and not got["n_index"].any()   # n = 1: no row has a variance
        assert np.all(got["owner"] == NO_OWNER)
    srt = sorted(regions)
    assert _table_rows(vs, srt) == a
    _check_oracle(vs, srt, *_parse(orc, srt), None, p, 17, quantise_r2(0.5), 0.3, 0.6, text_every=9)
    vs.close()


@pytest.mark.parametrize("seed", [701, 702])
def test_random_cohorts_with_duplicate_rule(seed, tmp_path):
    fasta, vcf, names = write_random_cohort(str(tmp_path), seed, ref_len=6000, n_rows=400, n_samples=9, p_near=0.6, p_multi=0.3,
                                            p_same=0.3, unphased_p=0.4 if seed % 2 else 0.05)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(seed)
    regions = random_regions(rng, 6000, 300, max_len=900)
    parsed, valid = _parse(orc, regions)
    subsets = [None] + [[vs.sample_id(s) for s in rng.choice(names, size=int(rng.integers(2, len(names))), replace=False)] for _ in range(2)]
    families = pvalue_families(_table_rows(vs, regions), seed)
    for sub, window, T, fam in zip(subsets, (64, 7, 256), (quantise_r2(0.2), 0, quantise_r2(0.05)), (0, 1, 4)):
        _name, p, p1, p2 = families[fam]
        got, _cells, _band, _want = _check_oracle(vs, regions, parsed, valid, sub, p, window, T, p1, p2, text_every=6)
        assert (got["state"] == DROPPED).any(), "no region of the batch falls under the duplicate rule"
        assert (got["state"] == INDEX).any() and (got["state"] == MEMBER).any()
    vs.close()


# ------------------------------------------------------------- 2. against the engine's own matrix, every byte of the verdicts
def _matrix_of(vs, regions, samples=None):
    mres = vs.genotype_matrix(regions, samples)
    m = mres.genotype_matrix()
    mres.close()
    return m, np.ascontiguousarray(m["cells"]), (m["rows"]["count_flags"] >> 31) != 0


def _check_full(vs, regions, samples, runs, T, what=None, max_bp=0, matrix_of=None):
    """Every verdict byte, owner, keep_begin and n_index of every run -- (window, (name, p, p1, p2)) -- against the reference over
    the cells of genotype_matrix() for the same regions and samples.  Returns (the matrix's arrays, cells, dropped, [result dict
    per run], the hit band of the widest window)."""
    m, cells, dropped = matrix_of if matrix_of is not None else _matrix_of(vs, regions, samples)
    band = hit_band(cells, max(w for w, _f in runs), T)
    out = []
    for window, (name, p, p1, p2) in runs:
        res = vs.ld_clump(regions, p, samples, window=window, r2=T / ONE, max_bp=max_bp, p1=p1, p2=p2)
        got = res.ld_clump()
        _params(got, m["columns"].tolist(), p, window, T, p1, p2, max_bp)
        assert np.array_equal(got["rows"]["pos"], m["rows"]["pos"])
        assert np.array_equal(got["row_begin"], m["row_begin"]) and np.array_equal(got["row_count"], m["row_count"])
        want = clump_states(cells, dropped, m["rows"]["pos"], m["row_begin"], m["row_count"], keys_of(p), window, T, key_of(p1), key_of(p2), max_bp,
                            band=band)
        _same(got, want, (what, window, name, T, cells.shape))
        assert res.totals()[2] == int(np.count_nonzero(cells))
        res.close()
        out.append(got)
    return m, cells, dropped, out, band


def _pitch_cohort(n_cols):   # (num_samples counts the samples of the cohort; info().num_samples adds "ref")
    return VariantStore.synthetic(device=0, ref_length=60_000, num_variants=1500, num_samples=n_cols, seed=900 + n_cols, first_pos=100,
                                  frac_ins=0.06, frac_del=0.06, frac_multi=0.03, max_indel=4, af_exponent=1.0)


def _pitch_regions(vs, rng):
    L = vs.info().ref_length
    starts = rng.integers(1, L - 4000, size=60)
    return [(int(s), int(s) + int(rng.integers(1, 4000))) for s in starts] + [(1, 3000), (L - 2000, L + 5), (1, L)]


@pytest.mark.parametrize("n_cols", [1, 47, 65, 257])
def test_every_byte_against_the_matrix(n_cols):
    """Windows on both sides of a mask word (31, 32, 33) and of a column tile (16, 17), the 5-tile and the 17-tile mask kernel; an
    unsorted batch of overlapping regions, one of them the whole table (more rows than the workgroup has threads); every family at
    window 64 and one family, in turn, at each other window.  T is about 1 / n: among random genotypes the hits are dense."""
    vs = _pitch_cohort(n_cols)
    rng = np.random.default_rng(n_cols)
    regions = _pitch_regions(vs, rng)
    T = quantise_r2(1.0 / n_cols)
    mo = _matrix_of(vs, regions)
    a = mo[1].shape[0]
    assert a > 1024
    families = pvalue_families(a, 100 + n_cols)
    runs = [(w, families[k % 5]) for k, w in enumerate(WINDOWS)] + [(64, f) for f in families] + [(256, families[0])]
    m, cells, dropped, out, band = _check_full(vs, regions, None, runs, T, n_cols, matrix_of=mo)
    assert cells.shape == (a, n_cols) and int(m["row_count"].max()) == a
    if n_cols == 1:   # n = 1: no row has a variance
        assert all(not ((g["state"] == INDEX) | (g["state"] == MEMBER) | (g["state"] == UNCLUMPED)).any() for g in out)
    else:
        assert band.mean() > 0.1, "the hits are not dense"
        for (window, (name, _p, _p1, _p2)), g in zip(runs, out):
            if window >= 16 and name in ("uniform", "ordered"):
                s = g["state"]
                n, index, member = int((s != INELIGIBLE).sum() - (s == DROPPED).sum()), int((s == INDEX).sum()), int((s == MEMBER).sum())
                assert n > 1000 and index > 0 and 10 * member >= n, (window, name, n, index, member)
        assert any((g["state"] == UNCLUMPED).any() for g in out)
    vs.close()


def test_region_sizes_around_a_wave_and_the_workgroup():
    """Regions of 1, 2, 63, 64, 65, more than 3 x 64 and more than 1024 rows, each alone (its table is the region) and all in one
    batch with an empty region; a batch whose table is empty; a region that begins inside another one, behind a row that leads there
    and hits its first row; the region that ends at the table's last row."""
    vs = _pitch_cohort(65)
    L = vs.info().ref_length
    probe = vs.allele_counts([(1, L)])
    pos = np.unique(probe.allele_counts()["rows"]["pos"].astype(np.int64))
    probe.close()
    spans = [(int(pos[k]), int(pos[k + m])) for m in (0, 1, 2, 61, 62, 63, 64, 65, 66, 200, 210, 220, 230, 1100) for k in range(0, 60, 3)]
    cres = vs.allele_counts(spans)
    n_rows = cres.allele_counts()["row_count"].astype(np.int64)
    cres.close()
    blocks = np.nonzero((n_rows > 3 * 64) & (n_rows < 1024) & (n_rows % 64 != 0))[0]
    large = np.nonzero(n_rows > 1024)[0]
    assert blocks.size and large.size
    T = quantise_r2(1.0 / 65)
    first = int(pos[0])
    assert first > 2
    chosen = []
    for want, windows in ((1, (1, 256)), (2, (1, 64)), (63, (16, 100)), (64, (33, 64)), (65, (1, 64, 256)), (int(n_rows[blocks[0]]), (17, 64, 256)),
                          (int(n_rows[large[0]]), (32, 256))):
        hit = np.nonzero(n_rows == want)[0]
        assert hit.size, (want, sorted(set(n_rows.tolist())))
        span = spans[int(hit[0])]
        families = pvalue_families(want, want)
        runs = [(w, families[(k + want) % 5]) for k, w in enumerate(windows)] + [(windows[-1], families[0])]
        m, _cells, _dropped, out, _band = _check_full(vs, [span], None, runs, T, want)
        assert m["cells"].shape[0] == want and all(g["keep_begin"].tolist() == [0, want] for g in out)
        chosen.append(span)
    # all of them in one unsorted batch, an empty region among them and the whole table behind them
    batch = chosen[::-1] + [(1, first - 2)] + chosen[:2] + [(1, L)]
    a = _table_rows(vs, batch)
    families = pvalue_families(a, 9)
    m, cells, dropped, out, band = _check_full(vs, batch, None, [(16, families[1]), (64, families[0]), (256, families[4]), (64, families[3])], T, "batch")
    e = len(chosen)
    for got in out:
        assert int(got["row_count"][e]) == 0 and int(got["n_index"][e]) == 0 and got["keep_begin"][e] == got["keep_begin"][e + 1]
        assert int(got["rounds"][e]) == 0
        last = len(batch) - 1
        assert int(got["row_begin"][last]) + int(got["row_count"][last]) == cells.shape[0]   # ends at the table's last row
    # a batch whose table is empty
    res = vs.ld_clump([(1, first - 2), (1, 1)], np.zeros(0), window=16)
    got = res.ld_clump()
    assert got["state"].shape == (0,) and got["owner"].shape == (0,) and got["keep_begin"].tolist() == [0, 0, 0] and got["n_index"].tolist() == [0, 0]
    assert got["rows"].shape == (0,) and got["counts"].shape == (0,) and res.region_clumps(0) == [] and res.totals()[1:3] == (0, 0)
    assert res.region_text(1) == "Pos\tRef\tAlt\tAC\tP\tState\tIndex\n"
    ps, po, pb, pn, pc, nq, na, nc = res.ld_clump_device()
    assert (nq, na, nc) == (2, 0, 65)
    res.close()
    vs.close()


# ------------------------------------------------------------------------- 3. the table-order family is the pruning query
def test_table_order_is_ld_prune():
    """p increasing in table order, p1 = p2 = 1: every region's INDEX set is vs.ld_prune's KEPT set -- both on the device."""
    vs = _pitch_cohort(47)
    rng = np.random.default_rng(8)
    regions = _pitch_regions(vs, rng)
    a = _table_rows(vs, regions)
    p = (np.arange(a) + 1.0) / (a + 1.0)
    gaps = np.diff(np.unique(vs.allele_counts(regions).allele_counts()["rows"]["pos"].astype(np.int64)))
    for window in (1, 33, 256):
        for max_bp in (0, 20 * int(np.median(gaps))):
            for r2 in (1.0 / 47, 0.3):
                cres = vs.ld_clump(regions, p, window=window, r2=r2, max_bp=max_bp, p1=1.0, p2=1.0)
                pres = vs.ld_prune(regions, window=window, r2=r2, max_bp=max_bp)
                c, k = cres.ld_clump(), pres.ld_prune()
                cres.close(); pres.close()
                assert np.array_equal(c["keep_begin"], k["keep_begin"]) and np.array_equal(c["n_index"], k["n_kept"]), (window, max_bp, r2)
                assert np.array_equal(c["state"] == INDEX, k["state"] == KEPT), (window, max_bp, r2)
                assert np.array_equal((c["state"] == INELIGIBLE) | (c["state"] == DROPPED), k["state"] >= 2)
                assert (c["state"] == INDEX).any() and (c["state"] == MEMBER).any() and not (c["state"] == UNCLUMPED).any()
    vs.close()


def test_deep_chain_on_the_block_cohort(tmp_path):
    """Table order at T = 0 and window 4 on the LD-block cohort is one long chain (the synchronous reference takes more than 100
    rounds for its 316 rows): the loop ends and the bytes are the pruning query's and the reference's."""
    fasta, vcf, _names, last = write_ld_block_cohort(str(tmp_path), BLOCK_SEED)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    regions = [(1, last + 50), (200, 3000), (1, last + 50)]
    a = _table_rows(vs, regions)
    p = (np.arange(a) + 1.0) / (a + 1.0)
    _m, _cells, _dropped, out, _band = _check_full(vs, regions, None, [(4, ("ordered", p, 1.0, 1.0)), (8, ("ordered", p, 1.0, 1.0))], 0, "chain")
    pres = vs.ld_prune(regions, window=4, r2=0.0)
    k = pres.ld_prune()
    pres.close()
    assert np.array_equal(out[0]["state"] == INDEX, k["state"] == KEPT) and np.array_equal(out[0]["n_index"], k["n_kept"])
    assert 1 <= int(out[0]["rounds"][0]) <= a and int(out[0]["n_index"][0]) >= 30
    vs.close()


# ------------------------------------------------------------------------------------------------------ 4. independence
def test_regions_are_independent():
    vs = _pitch_cohort(47)
    rng = np.random.default_rng(3)
    regions = _pitch_regions(vs, rng)[:58]
    regions += [regions[4], regions[4], regions[17], (1, vs.info().ref_length)]   # identical regions, and the whole table
    T = quantise_r2(1.0 / 47)
    mo = _matrix_of(vs, regions)
    a = mo[1].shape[0]
    fam = pvalue_families(a, 21)[0]
    m, cells, dropped, out, _band = _check_full(vs, regions, None, [(64, fam)], T, "independence", matrix_of=mo)
    assert not dropped.any(), "the cohort has rows under the duplicate rule"
    got = out[0]
    kb = got["keep_begin"].astype(np.int64)
    per = [got["state"][kb[q]:kb[q + 1]] for q in range(len(regions))]
    own = [got["owner"][kb[q]:kb[q + 1]] for q in range(len(regions))]
    assert sum(x.shape[0] for x in per) > cells.shape[0], "the regions do not overlap"
    for q, region in enumerate(regions):
        # the region alone: its table is a part of the batch's, so its p-values are that part of the batch's
        a0, mq = int(got["row_begin"][q]), int(got["row_count"][q])
        res = vs.ld_clump([region], fam[1][a0:a0 + mq], window=64, r2=T / ONE, max_bp=0, p1=fam[2], p2=fam[3])
        alone = res.ld_clump()
        res.close()
        assert np.array_equal(alone["state"], per[q]) and np.array_equal(alone["owner"], own[q]), (q, region)
        assert int(alone["n_index"][0]) == int(got["n_index"][q])
        # no owner points outside its region, and every owner is an INDEX row
        has = own[q] != NO_OWNER
        assert np.array_equal(has, (per[q] == INDEX) | (per[q] == MEMBER)) and np.all(own[q][has] < mq) and np.all(per[q][own[q][has]] == INDEX)
    assert np.array_equal(per[58], per[4]) and np.array_equal(per[59], per[4]) and np.array_equal(per[60], per[17])
    assert np.array_equal(own[58], own[4]) and np.array_equal(own[60], own[17]) and per[4].shape[0] > 0
    # a region that begins behind a row that leads in the whole table and hits its first row: INDEX there, MEMBER in the whole table
    whole = len(regions) - 1
    w0, wb = int(got["row_begin"][whole]), int(kb[whole])
    seen = False
    for q in range(whole):
        a0, mq = int(got["row_begin"][q]), int(got["row_count"][q])
        if mq and a0 > w0 and per[q][0] == INDEX and got["state"][wb + a0 - w0] == MEMBER and int(got["owner"][wb + a0 - w0]) < a0 - w0:
            seen = True
    assert seen, "no region begins behind the index row of its first row"
    vs.close()


# ------------------------------------------------------------------------------------------------------- 5. thresholds
def test_thresholds_ties_and_missing_p_values():
    vs = _pitch_cohort(65)
    rng = np.random.default_rng(9)
    regions = _pitch_regions(vs, rng)
    T = quantise_r2(1.0 / 65)
    mo = _matrix_of(vs, regions)
    m, cells, dropped = mo
    a = cells.shape[0]
    # p1 = p2 = 0: only the rows with p = 0 (or -0.0) take part; the smallest subnormal does not
    p = rng.choice(np.asarray([0.0, -0.0, 5e-324, 1e-300, 0.5]), size=a)
    _m, _c, _d, out, _b = _check_full(vs, regions, None, [(64, ("zeros", p, 0.0, 0.0)), (17, ("zeros", p, -0.0, 0.0))], T, "p = 0", matrix_of=mo)
    rows_of = np.concatenate([np.arange(int(b), int(b) + int(n)) for b, n in zip(out[0]["row_begin"], out[0]["row_count"])])
    s = out[0]["state"]
    assert np.all(s[(p[rows_of] != 0.0) & ~dropped[rows_of]] == INELIGIBLE) and (s == INDEX).any() and (s == MEMBER).any()
    # rows between p1 and p2 are never INDEX; some join, some stay unclumped
    fam = pvalue_families(a, 31)[1]
    _m, _c, _d, out, _b = _check_full(vs, regions, None, [(33, fam), (256, fam)], T, "p1 < p2", matrix_of=mo)
    for got in out:
        s, between = got["state"], (fam[1][rows_of] > fam[2]) & (fam[1][rows_of] <= fam[3])
        assert between.any() and not (s[between] == INDEX).any() and (s[between] == MEMBER).any() and (s[between] == UNCLUMPED).any()
        assert np.all(s[fam[1][rows_of] > fam[3]] >= INELIGIBLE) and not (s[~between] == UNCLUMPED).any()
    # ties go to the earlier row: with one p-value for every row the priority is the table's order
    flat = np.full(a, 0.125)
    _m, _c, _d, out, _b = _check_full(vs, regions, None, [(64, ("flat", flat, 1.0, 1.0))], T, "ties", matrix_of=mo)
    pres = vs.ld_prune(regions, window=64, r2=T / ONE)
    assert np.array_equal(out[0]["state"] == INDEX, pres.ld_prune()["state"] == KEPT)
    pres.close()
    # NaN rows are skipped
    fam = pvalue_families(a, 32)[4]
    _m, _c, _d, out, _b = _check_full(vs, regions, None, [(100, fam)], T, "NaN", matrix_of=mo)
    nan = np.isnan(fam[1][rows_of])
    assert nan.sum() > 100 and np.all(out[0]["state"][nan & ~dropped[rows_of]] == INELIGIBLE) and np.all(out[0]["owner"][nan] == NO_OWNER)
    # max_bp cuts inside a window and changes the answer
    gaps = np.diff(np.unique(m["rows"]["pos"].astype(np.int64)))
    typical = int(np.median(gaps))
    fam = pvalue_families(a, 33)[0]
    _m, _c, _d, base, _b = _check_full(vs, regions, None, [(16, fam), (64, fam)], T, "base", matrix_of=mo)
    for max_bp in (1, typical, 5 * typical, 40 * typical):   # 5 and 40 typical gaps cut inside windows of 16 and 64 rows
        _m, _c, _d, out, _b = _check_full(vs, regions, None, [(16, fam), (64, fam)], T, ("bp", max_bp), max_bp=max_bp, matrix_of=mo)
        if max_bp == 5 * typical:
            assert not np.array_equal(out[0]["state"], base[0]["state"]) and int(out[0]["n_index"].sum()) != int(base[0]["n_index"].sum())
    vs.close()


# ------------------------------------------------------------------------------------------------- 6. engine behaviour
T6_KW = dict(ref_length=8_000_000, num_variants=150_000, num_samples=300, seed=5, first_pos=1_000, frac_ins=0.05, frac_del=0.05,
             frac_multi=0.02, max_indel=6, af_exponent=2.0)


@pytest.fixture(scope="module")
def t6_store():
    vs = VariantStore.synthetic(device=0, **T6_KW)
    rng = np.random.default_rng(12)
    s = np.sort(rng.integers(1_000, 7_990_000, size=3_000))
    regions = np.stack([s, s + rng.integers(50, 3_000, size=3_000)], axis=1).astype(np.uint64)
    yield vs, regions
    vs.close()


def _uniform(vs, regions, seed, power=1.0):
    return np.random.default_rng(seed).random(_table_rows(vs, regions)) ** power


def test_identical_calls_give_identical_bytes(t6_store):
    vs, regions = t6_store
    batch = np.ascontiguousarray(regions[:1_500])
    p = _uniform(vs, batch, 1, 3.0)
    first = None
    for _ in range(3):
        res = vs.ld_clump(batch, p, window=100, r2=0.1, max_bp=20_000, p1=0.05, p2=0.3)
        got = res.ld_clump()
        res.close()
        if first is None:
            first = got
            assert all((got["state"] == s).any() for s in (INDEX, MEMBER, INELIGIBLE, UNCLUMPED))
        for k in ("state", "owner", "keep_begin", "n_index", "counts"):
            assert np.array_equal(got[k], first[k]), k
    cres = vs.allele_counts(batch)   # the counts are the count query's rows
    ac = cres.allele_counts()
    for f in ("carriers", "alt_alleles", "hom_alt", "phased"):
        assert np.array_equal(first["counts"][f], ac["counts"][f]), f
    lay = cres.layout()
    cres.close()
    res = vs.ld_clump(batch, p, window=16)
    assert res.layout()[1] == lay[1] and res.fill_ms() > 0 and int(res.ld_clump()["keep_begin"][-1]) == int(first["row_count"].sum())
    res.close()


def test_buffers_from_the_pool():
    """A large batch is closed, then small ones on the same handle take its buffers -- state, owners, masks, blocker masks, classes,
    keys, matrix: every byte of the answer must be written, and with T = 2^20 every mask word is a written 0."""
    vs = VariantStore.synthetic(device=0, **T6_KW)
    rng = np.random.default_rng(4)
    s = np.sort(rng.integers(1_000, 7_990_000, size=1_500))
    regions = np.stack([s, s + rng.integers(50, 3_000, size=1_500)], axis=1).astype(np.uint64)
    p = _uniform(vs, regions, 2)
    small = np.ascontiguousarray(regions[:40])
    fam = pvalue_families(_table_rows(vs, small), 5)
    few = np.ascontiguousarray(regions[:3])
    ffam = pvalue_families(_table_rows(vs, few), 6)
    for T in (0, quantise_r2(0.02)):
        big = vs.ld_clump(regions, p, window=256, r2=T / ONE, max_bp=0, p1=1.0, p2=1.0)
        assert (big.ld_clump()["state"] == MEMBER).sum() > 500
        big.close()
        _check_full(vs, small, [5, 9, 11, 200, 250], [(33, fam[0]), (33, fam[1])], ONE, "pool")   # nothing hits: every mask word is 0
        _check_full(vs, small, None, [(64, fam[0]), (64, fam[4])], T, "pool")
        _check_full(vs, few, None, [(256, ffam[0])], T, "pool")
    vs.close()


def test_interleaving_leaves_type6_alone():
    rng = np.random.default_rng(12)
    batches = []
    for k in range(6):
        n = 3_000 + 200 * k + (4_000 if k == 4 else 0)   # like batches (speculated), one larger (refused / re-sized)
        s = np.sort(rng.integers(1_000, 7_990_000, size=n))
        batches.append(np.stack([s, s + rng.integers(50, 3_000, size=n)], axis=1).astype(np.uint64))
    shuffled = batches[3][rng.permutation(batches[3].shape[0])]

    def run(with_clump):
        vs = VariantStore.synthetic(device=0, **T6_KW)
        ps = _uniform(vs, shuffled, 3) if with_clump else None
        digests = []
        for k, b in enumerate(batches):
            r = vs.get_var_in_ref(b)
            if with_clump:   # clumping batches in between: sorted, unsorted, with a subset
                l1 = vs.ld_clump(b, _uniform(vs, b, k), window=16, p1=0.5, p2=0.9)
                l2 = vs.ld_clump(shuffled, ps, window=64, r2=0.5, p1=1.0, p2=1.0)
                l3 = vs.ld_clump(shuffled, ps, [1, 5, 7, 200], window=100, max_bp=5_000)
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


def _read_device(torch, ptr, n_bytes):
    return _read_device_bytes(torch, ptr, 1, n_bytes).reshape(n_bytes).copy()


def test_device_regions_and_device_pointers(t6_store):
    """Regions in device memory and the device accessor.  Sample ids and p-values are host arrays."""
    torch = pytest.importorskip("torch")
    vs, regions = t6_store
    sub = [3, 17, 40, 200, 250, 251]
    batch = np.ascontiguousarray(regions[:2_500])
    p = _uniform(vs, batch, 7)
    host = vs.ld_clump(batch, p, sub, window=32, r2=0.0, p1=0.5, p2=0.8)
    hgot = host.ld_clump()
    t = torch.from_numpy(batch.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    dev = vs.ld_clump(DeviceArray(t.data_ptr(), batch.shape[0]), p, sub, window=32, r2=0.0, p1=0.5, p2=0.8)
    dgot = dev.ld_clump()
    for k in ("columns", "row_begin", "row_count", "counts", "state", "owner", "keep_begin", "n_index"):
        assert np.array_equal(hgot[k], dgot[k]), k
    assert all((hgot["state"] == s).any() for s in (INDEX, MEMBER, UNCLUMPED))
    ps, po, pb, pn, pc, nq, a, c = dev.ld_clump_device()
    total = dgot["state"].shape[0]
    assert (nq, a, c) == (2_500, dgot["rows"].shape[0], 6) and ps and po and pb and pn and pc
    first = _read_device(torch, ps, total)
    later = vs.ld_clump(regions[2_500:2_900], _uniform(vs, regions[2_500:2_900], 8), window=8)   # a later batch leaves the verdicts alone
    later.totals()
    assert np.array_equal(first, dgot["state"])
    assert np.array_equal(_read_device(torch, ps, total), first)
    assert np.array_equal(_read_device(torch, po, 4 * total).view(np.uint32), dgot["owner"])
    assert np.array_equal(_read_device(torch, pb, 8 * (nq + 1)).view(np.uint64), dgot["keep_begin"])
    assert np.array_equal(_read_device(torch, pn, 8 * nq).view(np.uint64), dgot["n_index"])
    assert np.array_equal(_read_device(torch, pc, a * 16).view(np.uint32).reshape(a, 4), dgot["counts"].view(np.uint32).reshape(a, 4))
    later.close(); host.close(); dev.close()


def test_size_limit_and_the_number_of_p_values(t6_store):
    vs, regions = t6_store
    warm = vs.allele_counts(regions)   # the plan's temporaries, the table and the counts of this batch are in the handle's pool afterwards
    wgot = warm.allele_counts()
    a, states = wgot["rows"].shape[0], int(wgot["row_count"].sum())
    warm.close()
    p = np.random.default_rng(5).random(a)
    # one p-value per table row: both numbers are in the message
    for n in (a - 1, a + 1, 0, states if states != a else a + 2):
        with pytest.raises(VariantStoreError) as e:
            vs.ld_clump(regions, np.resize(p, n), window=16)
        assert e.value.code == VS_ERR_ARG and f"{n} p-values" in str(e.value) and f"{a} rows" in str(e.value), (n, str(e.value))
    c = vs.info().num_samples - 1
    pitch = (c + 15) // 16 * 16
    parts = (a * pitch, a * 4 * 8, a * 9, states * 2 * 4 * 8, states * 5, 8 * (3 * (regions.shape[0] + 1) + 4))
    assert parts[0] > 1 << 20
    vs.set_option("matrix_max_mib", 1)
    try:
        before = vs.info().pool_mallocs
        with pytest.raises(VariantStoreError) as e:
            vs.ld_clump(regions, p, window=256)
        assert e.value.code == VS_ERR_ARG
        msg = str(e.value)
        for what in (f"{regions.shape[0]} regions", f"{a} rows", f"{c} columns", "window 256", " bytes", "matrix_max_mib") + tuple(str(x) for x in parts[:2]):
            assert what in msg, (what, msg)
        assert vs.info().pool_mallocs == before, "the refused batch allocated"
        few = vs.ld_clump(regions[:20], _uniform(vs, regions[:20], 1), [1, 2, 3], window=2)   # a few bytes a row: below the limit
        assert few.ld_clump()["keep_begin"].shape == (21,)
        few.close()
        # with three columns the matrix alone would fit; the whole does not, and now the verdicts are known: every part is named
        if a * 16 <= 1 << 20 < a * (16 + 32 + 9) + states * (5 + 64):
            with pytest.raises(VariantStoreError) as e:
                vs.ld_clump(regions, p, [1, 2, 3], window=256)
            assert e.value.code == VS_ERR_ARG
            for x in (a * 16,) + parts[1:]:
                assert f"{x} of" in str(e.value) or f"{x} bytes" in str(e.value), (x, str(e.value))
            assert str(a * (16 + 32 + 9) + sum(parts[3:])) + " bytes" in str(e.value)
    finally:
        vs.set_option("matrix_max_mib", 0)
    again = vs.ld_clump(regions, p, window=256, p1=0.5, p2=0.9)   # the handle stays usable
    got = again.ld_clump()
    assert got["state"].shape == (states,) and (got["state"] == INDEX).any()
    again.close()


def test_refused_accessors(t6_store):
    vs, regions = t6_store
    batch = regions[:1_000]
    r = vs.ld_clump(batch, _uniform(vs, batch, 2), window=8)
    for call in (lambda: r.raw(with_carriers=True), lambda: r.view(with_carriers=True), r.digest, r.num_header_records,
                 r.num_region_records):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_UNSUPPORTED
    for call in (r.allele_counts, r.sample_burden, r.sample_burden_device, r.genotype_matrix, r.genotype_matrix_device, r.ld_band,
                 r.ld_band_device, r.ld_matrix, r.ld_matrix_device, r.ld_prune, r.ld_prune_device, r.sample_gram, r.sample_ibs):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_ARG
    r.view(with_carriers=False)
    raw = r.raw(with_carriers=False)
    t6 = vs.get_var_in_ref(batch)
    raw6 = t6.raw(with_carriers=False)
    for f in ("pos", "ref_off", "ref_len", "alt_off", "alt_len", "count_flags"):
        assert np.array_equal(raw["rows"][f], raw6["rows"][f]), f
    assert np.array_equal(raw["region_flags"], raw6["region_flags"]) and np.array_equal(raw["row_count"], raw6["row_count"])
    assert r.totals()[:2] == t6.totals()[:2]
    r.close()
    for res in (t6, vs.allele_counts(regions[:10]), vs.sample_burden(regions[:10]), vs.genotype_matrix(regions[:10]),
                vs.ld_band(regions[:10], window=4), vs.ld_matrix(regions[:10]), vs.ld_prune(regions[:10]), vs.sample_gram(regions[:10])):
        for call in (res.ld_clump, res.ld_clump_device):
            with pytest.raises(VariantStoreError) as e:
                call()   # not a clumping result
            assert e.value.code == VS_ERR_ARG
        res.close()


def test_mapping_route_and_cli(tmp_path):
    """The LD-block cohort through `variantstore construct` and `variantstore clump`, against VariantStore.ld_clump with the same
    mapping: a p-value for most variants, one key that matches nothing."""
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
    keys = vs._table_keys(regions)
    assert len(keys) > 200 and all(k is not None for k in keys)
    pv = rng.random(len(keys)) ** 6
    mapping = {k: float(x) for k, x in zip(keys, pv) if rng.random() < 0.9}
    mapping[(last + 7, "A", "C")] = 0.5   # matches nothing
    afile = os.path.join(tmp_path, "p.txt")
    with open(afile, "w") as f:
        f.write("# pos ref alt p\n" + "".join(f"{k[0]} {k[1] or '-'}\t{k[2] or '.'} {x!r}\n" for k, x in mapping.items()))   # (- or .: an empty allele)
    assert any(not k[1] for k in mapping)
    # the mapping lands in table order, rows without a key have no p-value
    res = vs.ld_clump(regions, mapping)
    got = res.ld_clump()
    want_p = np.asarray([mapping.get(k, NAN) for k in keys])
    assert np.array_equal(got["pvalues"], want_p, equal_nan=True) and res.unmatched == [(last + 7, "A", "C")]
    arr = vs.ld_clump(regions, want_p)
    for k in ("state", "owner", "n_index"):
        assert np.array_equal(got[k], arr.ld_clump()[k]), k
    assert arr.unmatched is None and np.array_equal(pvalue_keys(want_p)[~np.isnan(want_p)], keys_of(want_p)[~np.isnan(want_p)])
    arr.close(); res.close()
    names = [vs.sample_name(i) for i in range(1, min(4, vs.info().num_samples))]
    sfile = os.path.join(tmp_path, "samples.txt")
    with open(sfile, "w") as f:
        f.write("\n".join(names) + "\n")
    words = set()
    for samples, extra in ((None, []), (names, ["-S", sfile])):
        for kw, flags in ((dict(), []), (dict(window=3, r2=0.0, p1=0.01, p2=0.5), ["-w", "3", "--r2", "0", "--p1", "0.01", "--p2", "0.5"]),
                          (dict(r2=0.75, max_bp=40, p1=1.0, p2=1.0), ["--r2", "0.75", "--bp", "40", "--p1", "1", "--p2", "1"]),
                          (dict(window=256, max_bp=0, p1=0.0, p2=0.2), ["--window", "256", "--bp", "0", "--p1", "0", "--p2", "0.2"])):
            out = os.path.join(tmp_path, "clump.txt")
            run = subprocess.run([exe, "clump", "-p", prefix, "-r", "@" + rfile, "-A", afile, "-o", out] + extra + flags, check=True, capture_output=True,
                                 text=True)
            assert "warning" in run.stderr and "1 line" in run.stderr
            with open(out, "rb") as f:
                parts = f.read().decode("latin-1").split("#region ")[1:]
            res = vs.ld_clump(regions, mapping, samples, **kw)
            assert len(parts) == len(regions)
            for q, part in enumerate(parts):
                head, text = part.split("\n", 1)
                assert head == f"{q} {regions[q][0]}:{regions[q][1]}"
                assert text == res.region_text(q), (q, kw)
                assert text.startswith("Pos\tRef\tAlt\tAC\tP\tState\tIndex\n")
                words |= {line.split("\t")[5] for line in text.split("\n")[1:] if line}
            res.close()
    assert words == {"index", "clumped", "unclumped", "skip"}
    for bad in (["-w", "300"], ["--r2", "1.5"], ["--p1", "0.5", "--p2", "0.1"], ["--p2", "7"]):
        run = subprocess.run([exe, "clump", "-p", prefix, "-r", "@" + rfile, "-A", afile] + bad, capture_output=True, text=True)
        assert run.returncode != 0, bad
    bfile = os.path.join(tmp_path, "bad.txt")
    with open(bfile, "w") as f:
        f.write(f"{keys[0][0]} {keys[0][1]} {keys[0][2]} 1.5\n")
    run = subprocess.run([exe, "clump", "-p", prefix, "-r", "@" + rfile, "-A", bfile], capture_output=True, text=True)
    assert run.returncode != 0 and "p-value" in run.stdout + run.stderr and "line 1" in run.stdout + run.stderr
    vs.close()
