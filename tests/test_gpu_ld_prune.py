"""LD pruning queries on the GPU (vs_query_ld_prune): the verdicts against what the oracle's type-6 text gives, against the engine's
own genotype matrix byte for byte (every pitch residue of the k loop, every mask-word and column-tile edge of the window, regions
around the walk's batch of 64 rows), the independence of the regions, the other parameters, repeated calls, buffers that come from
the pool, interleaving with type-6 batches, regions in device memory, the device pointers, the size limit, the refused accessors
and the CLI.

state, keep_begin and n_kept are compared byte for byte with tests/ld_prune_ref.py: there is no tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

from genotype_matrix_ref import Parsed, matrix
from helpers import oracle_texts, random_regions, write_random_cohort
from ld_prune_ref import (DROPPED, INELIGIBLE, KEPT, ONE, PRUNED, eligible, hit_band, prune_states, prune_text, row_counts,
                          write_ld_block_cohort)
from oracle.oracle import Oracle
from test_gpu_genotype_matrix import _read_device as _read_device_bytes
from test_ld_prune_host import BLOCK_SEED, BLOCK_THRESHOLDS, BLOCK_WINDOWS, block_conditions, block_subsets
from variantstore_amd import DeviceArray, VariantStore, quantise_r2
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_ARG, VS_ERR_UNSUPPORTED = -5, -7
WINDOWS = (1, 16, 17, 31, 32, 33, 64, 100, 256)
UMAX = 0xFFFFFFFF


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


def _same(got, want, what=None):
    state, keep_begin, n_kept = want
    assert got["state"].dtype == np.uint8 and got["keep_begin"].dtype == np.uint64 and got["n_kept"].dtype == np.uint64, what
    assert np.array_equal(got["keep_begin"], keep_begin), what
    bad = np.nonzero(got["state"] != state)[0] if got["state"].shape == state.shape else None
    assert bad is not None and bad.size == 0, (what, None if bad is None else bad[:8].tolist())
    assert np.array_equal(got["n_kept"], n_kept), what


def _params(got, ids, window, T, max_bp=0, min_ac=0, max_ac=UMAX):
    assert got["columns"].dtype == np.uint32 and got["columns"].tolist() == ids
    assert (got["window"], got["threshold_q20"], got["max_bp"], got["min_ac"], got["max_ac"]) == (window, T, max_bp, min_ac, max_ac)
    assert got["threshold"] == T / ONE and got["counts"].shape == got["rows"].shape


# ------------------------------------------------------------------------------------------------ 1. against the oracle
def _check_oracle(vs, regions, parsed, valid, samples, window, T, text_every=1, **kw):
    """The verdicts of every region the oracle answers, from the cells its type-6 text gives, and the text of every text_every-th
    region.  Returns (result dict, the table's cells by the oracle, the hit band)."""
    ids, names = _columns(vs, samples)
    want_m = matrix(parsed, names)
    res = vs.ld_prune(regions, samples, window=window, r2=T / ONE, **kw)
    got = res.ld_prune()
    _params(got, ids, window, T, kw.get("max_bp", 0), kw.get("min_ac", 0), UMAX if kw.get("max_ac") is None else kw["max_ac"])
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
    want = prune_states(cells, dropped, rows["pos"], got["row_begin"], got["row_count"], window, T, kw.get("max_bp", 0), kw.get("min_ac", 0),
                        UMAX if kw.get("max_ac") is None else kw["max_ac"], band=band)
    assert np.array_equal(got["keep_begin"], want[1])
    ac = row_counts(cells)[0]
    for q in valid:
        o0, o1 = int(want[1][q]), int(want[1][q + 1])
        assert np.array_equal(got["state"][o0:o1], want[0][o0:o1]), (q, regions[q], samples, window, T)
        assert int(got["n_kept"][q]) == int(want[2][q]), (q, regions[q])
    for q in valid[::text_every] if text_every else ():
        a0, m = int(got["row_begin"][q]), int(got["row_count"][q])
        o0 = int(want[1][q])
        text = prune_text(heads[a0:a0 + m], ac[a0:a0 + m], want[0][o0:o0 + m])
        assert res.region_text(int(q)) == text, (q, regions[q])
        kept = [tuple(line.split("\t")[:3]) for line in text.split("\n")[1:] if line.endswith("\tkeep")]
        assert res.region_kept(int(q)) == [(int(p), r, alt) for p, r, alt in kept]
    res.close()
    return got, cells, band


def test_ld_block_cohort_against_the_oracle(tmp_path):
    fasta, vcf, names, last = write_ld_block_cohort(str(tmp_path), BLOCK_SEED)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    rng = np.random.default_rng(5)
    regions = [(1, last + 50)] + random_regions(rng, last + 50, 40, max_len=1500)
    parsed, valid = _parse(orc, regions)
    assert 0 in valid
    for sub in block_subsets(names):
        for T in BLOCK_THRESHOLDS:
            for window in BLOCK_WINDOWS:
                got, cells, band = _check_oracle(vs, regions, parsed, valid, sub, window, T, text_every=5)
                m = int(got["row_count"][0])   # region 0 is the whole cohort: the conditions of the CPU test, on the GPU's verdicts
                assert int(got["row_begin"][0]) == 0 and m == got["rows"].shape[0]
                dropped = (got["rows"]["count_flags"] >> 31) != 0
                assert not dropped.any(), "the LD-block cohort has no row under the duplicate rule"
                block_conditions(got["state"][:m], eligible(cells, dropped), band, window, T, (sub is None or len(sub), T, window))
    vs.close()


@pytest.mark.parametrize("stem", ["x", "x.small"])
def test_golden_region_sweeps(stem, golden_dir, tmp_path):
    fasta, vcf = os.path.join(golden_dir, stem + ".fa"), os.path.join(golden_dir, stem + ".vcf")
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    orc = _oracle(vs, tmp_path)
    n_samples = vs.info().num_samples - 1
    rng = np.random.default_rng(11)
    regions = random_regions(rng, _ref_len(fasta), 200)   # unsorted: the device sorts the batch
    parsed, valid = _parse(orc, regions)
    _check_oracle(vs, regions, parsed, valid, None, 64, quantise_r2(0.2))
    _check_oracle(vs, regions, parsed, valid, None, 3, 0)
    srt = sorted(regions)
    _check_oracle(vs, srt, *_parse(orc, srt), None, 17, quantise_r2(0.5))
    _check_oracle(vs, regions, parsed, valid, [1], 16, 0)   # n = 1: every row is ineligible
    _check_oracle(vs, regions, parsed, valid, [vs.sample_name(1)], 5, ONE)   # by name
    for k in range(3):
        ids = rng.choice(np.arange(1, n_samples + 1), size=int(rng.integers(1, n_samples + 1)), replace=False)
        ids = [int(i) for i in ids] + [int(i) for i in ids[:2]]   # duplicates collapse
        _check_oracle(vs, regions, parsed, valid, ids, (2, 64, 256)[k], (0, quantise_r2(0.1), ONE - 1)[k], min_ac=(0, 1, 2)[k])
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
    for sub, window, T in zip(subsets, (64, 7, 256), (quantise_r2(0.2), 0, quantise_r2(0.05))):
        got, _cells, _band = _check_oracle(vs, regions, parsed, valid, sub, window, T, text_every=6)
        assert (got["state"] == DROPPED).any(), "no region of the batch falls under the duplicate rule"
        assert (got["state"] == KEPT).any() and (got["state"] == PRUNED).any()
    vs.close()


# ------------------------------------------------------------- 2. against the engine's own matrix, every byte of the verdicts
def _matrix_of(vs, regions, samples=None):
    mres = vs.genotype_matrix(regions, samples)
    m = mres.genotype_matrix()
    mres.close()
    return m, np.ascontiguousarray(m["cells"]), (m["rows"]["count_flags"] >> 31) != 0


def _check_full(vs, regions, samples, windows, T, what=None, **kw):
    """Every verdict byte, keep_begin and n_kept of every window against the reference over the cells of genotype_matrix() for the
    same regions and samples.  Returns (the matrix's arrays, cells, dropped, {window: result dict}, the hit band of the widest)."""
    m, cells, dropped = _matrix_of(vs, regions, samples)
    band = hit_band(cells, max(windows), T)
    out = {}
    for window in windows:
        res = vs.ld_prune(regions, samples, window=window, r2=T / ONE, **kw)
        got = res.ld_prune()
        _params(got, m["columns"].tolist(), window, T, kw.get("max_bp", 0), kw.get("min_ac", 0), UMAX if kw.get("max_ac") is None else kw["max_ac"])
        assert np.array_equal(got["rows"]["pos"], m["rows"]["pos"])
        assert np.array_equal(got["row_begin"], m["row_begin"]) and np.array_equal(got["row_count"], m["row_count"])
        want = prune_states(cells, dropped, m["rows"]["pos"], m["row_begin"], m["row_count"], window, T, kw.get("max_bp", 0), kw.get("min_ac", 0),
                            UMAX if kw.get("max_ac") is None else kw["max_ac"], band=band)
        _same(got, want, (what, window, T, cells.shape))
        assert res.totals()[2] == int(np.count_nonzero(cells))
        res.close()
        out[window] = got
    return m, cells, dropped, out, band


def _pitch_cohort(n_cols):   # (num_samples counts the samples of the cohort; info().num_samples adds "ref")
    return VariantStore.synthetic(device=0, ref_length=60_000, num_variants=1500, num_samples=n_cols, seed=900 + n_cols, first_pos=100,
                                  frac_ins=0.06, frac_del=0.06, frac_multi=0.03, max_indel=4, af_exponent=1.0)


def _pitch_regions(vs, rng):
    L = vs.info().ref_length
    starts = rng.integers(1, L - 4000, size=60)
    return [(int(s), int(s) + int(rng.integers(1, 4000))) for s in starts] + [(1, 3000), (L - 2000, L + 5), (1, L)]


def _shares(got, cells, dropped):
    """(eligible, kept, pruned) over all verdicts of a result."""
    s = got["state"]
    return int(((s == KEPT) | (s == PRUNED)).sum()), int((s == KEPT).sum()), int((s == PRUNED).sum())


@pytest.mark.parametrize("n_cols,pitch", [(1, 16), (47, 48), (65, 80), (257, 272)])
def test_every_byte_against_the_matrix(n_cols, pitch):
    """The k-step tail in its residues of 64 and one full chunk plus a remainder; windows on both sides of a mask word (31, 32, 33)
    and of a column tile (16, 17), the 5-tile and the 17-tile kernel; an unsorted batch of overlapping regions, one of them the whole
    table.  T is about 1 / n: among random genotypes the hits are dense."""
    vs = _pitch_cohort(n_cols)
    rng = np.random.default_rng(n_cols)
    regions = _pitch_regions(vs, rng)
    T = quantise_r2(1.0 / n_cols)
    m, cells, dropped, out, band = _check_full(vs, regions, None, WINDOWS, T, n_cols)
    assert m["row_pitch"] == pitch and cells.shape == (m["rows"].shape[0], n_cols) and cells.shape[0] > 3 * 64
    if n_cols == 1:   # n = 1: no row has a variance
        assert all(not ((g["state"] == KEPT) | (g["state"] == PRUNED)).any() for g in out.values())
    else:
        assert band.mean() > 0.1, "the hits are not dense"
        for window in (16, 64, 256):
            ne, kept, pruned = _shares(out[window], cells, dropped)
            assert ne > 1000 and 10 * kept >= ne and 10 * pruned >= ne, (window, ne, kept, pruned)
    vs.close()


def test_region_sizes_around_the_batch_of_64_rows():
    """Regions of 1, 2, 63, 64, 65 and more than 3 x 64 rows, each alone (its table is the region) and all in one batch with an empty
    region; a batch whose table is empty; a region that begins inside another one, behind a row that one keeps; the region that ends
    at the table's last row."""
    vs = _pitch_cohort(65)
    L = vs.info().ref_length
    probe = vs.allele_counts([(1, L)])
    pos = np.unique(probe.allele_counts()["rows"]["pos"].astype(np.int64))
    probe.close()
    spans = [(int(pos[k]), int(pos[k + m])) for m in (0, 1, 2, 61, 62, 63, 64, 65, 66, 200, 210, 220, 230) for k in range(0, 60, 3)]
    cres = vs.allele_counts(spans)
    n_rows = cres.allele_counts()["row_count"].astype(np.int64)
    cres.close()
    blocks = np.nonzero((n_rows > 3 * 64) & (n_rows % 64 != 0))[0]
    assert blocks.size
    T = quantise_r2(1.0 / 65)
    first = int(pos[0])
    assert first > 2
    chosen = []
    for want, windows in ((1, (1, 256)), (2, (1, 64)), (63, (16, 100)), (64, (33, 64)), (65, (1, 64, 256)), (int(n_rows[blocks[0]]), (17, 64, 256))):
        hit = np.nonzero(n_rows == want)[0]
        assert hit.size, (want, sorted(set(n_rows.tolist())))
        span = spans[int(hit[0])]
        m, _cells, _dropped, out, _band = _check_full(vs, [span], None, windows, T, want)
        assert m["cells"].shape[0] == want and all(g["keep_begin"].tolist() == [0, want] for g in out.values())
        chosen.append(span)
    # all of them in one unsorted batch, an empty region among them and the whole table behind them
    batch = chosen[::-1] + [(1, first - 2)] + chosen[:2] + [(1, L)]
    m, cells, dropped, out, band = _check_full(vs, batch, None, (16, 64, 256), T, "batch")
    e = len(chosen)
    for got in out.values():
        assert int(got["row_count"][e]) == 0 and int(got["n_kept"][e]) == 0 and got["keep_begin"][e] == got["keep_begin"][e + 1]
        last = len(batch) - 1
        assert int(got["row_begin"][last]) + int(got["row_count"][last]) == cells.shape[0]   # ends at the table's last row
    # a region that begins mid-block: its first row is kept in its own walk and pruned in the walk of the whole table
    got = out[64]
    whole = len(batch) - 1
    w0, wb = int(got["row_begin"][whole]), int(got["keep_begin"][whole])
    seen = False
    for q in range(len(batch) - 1):
        a0, m_q, o = int(got["row_begin"][q]), int(got["row_count"][q]), int(got["keep_begin"][q])
        if m_q and a0 > w0 and got["state"][o] == KEPT and got["state"][wb + a0 - w0] == PRUNED:
            seen = True
    assert seen, "no region begins behind a row that blocks its first row in the whole table's walk"
    # a batch whose table is empty
    res = vs.ld_prune([(1, first - 2), (1, 1)], window=16)
    got = res.ld_prune()
    assert got["state"].shape == (0,) and got["keep_begin"].tolist() == [0, 0, 0] and got["n_kept"].tolist() == [0, 0]
    assert got["rows"].shape == (0,) and got["counts"].shape == (0,) and res.region_kept(0) == [] and res.totals()[1:3] == (0, 0)
    ps, pb, pn, pc, nq, na, nc = res.ld_prune_device()
    assert (nq, na, nc) == (2, 0, 65)
    res.close()
    vs.close()


# ------------------------------------------------------------------------------------------------------ 3. independence
def test_regions_are_independent():
    vs = _pitch_cohort(47)
    rng = np.random.default_rng(3)
    regions = _pitch_regions(vs, rng)[:58]
    regions += [regions[4], regions[4], regions[17]]   # identical regions
    T = quantise_r2(1.0 / 47)
    m, cells, dropped, out, _band = _check_full(vs, regions, None, (64,), T, "independence")
    assert not dropped.any(), "the cohort has rows under the duplicate rule"
    got = out[64]
    kb = got["keep_begin"].astype(np.int64)
    per = [got["state"][kb[q]:kb[q + 1]] for q in range(len(regions))]
    assert sum(p.shape[0] for p in per) > cells.shape[0], "the regions do not overlap"
    for q, region in enumerate(regions):
        res = vs.ld_prune([region], window=64, r2=T / ONE)
        alone = res.ld_prune()
        res.close()
        assert np.array_equal(alone["state"], per[q]) and int(alone["n_kept"][0]) == int(got["n_kept"][q]), (q, region)
    assert np.array_equal(per[58], per[4]) and np.array_equal(per[59], per[4]) and np.array_equal(per[60], per[17])
    assert per[4].shape[0] > 0
    vs.close()


# ------------------------------------------------------------------------------------------------ 4. the other parameters
def test_distance_and_allele_count_limits():
    vs = _pitch_cohort(65)
    rng = np.random.default_rng(9)
    regions = _pitch_regions(vs, rng)
    T = quantise_r2(1.0 / 65)
    m, cells, dropped, base, band = _check_full(vs, regions, None, (16, 64), T, "base")
    gaps = np.diff(np.unique(m["rows"]["pos"].astype(np.int64)))
    typical = int(np.median(gaps))
    for max_bp in (1, typical, 5 * typical, 40 * typical):   # 5 and 40 typical gaps cut inside windows of 16 and 64 rows
        _m, _c, _d, out, _b = _check_full(vs, regions, None, (16, 64), T, ("bp", max_bp), max_bp=max_bp)
        if max_bp == 5 * typical:
            assert not np.array_equal(out[16]["state"], base[16]["state"]) and int(out[16]["n_kept"].sum()) != int(base[16]["n_kept"].sum())
    ac = row_counts(cells)[0]
    lo, hi = int(np.percentile(ac[ac > 0], 30)), int(np.percentile(ac, 80))
    assert 0 < lo < hi
    for kw in (dict(min_ac=lo), dict(max_ac=hi), dict(min_ac=lo, max_ac=hi), dict(min_ac=hi, max_ac=hi), dict(min_ac=0, max_ac=0)):
        _m, _c, _d, out, _b = _check_full(vs, regions, None, (64,), T, kw, **kw)
        got = out[64]
        # every verdict of a row outside the limits is "ineligible"; the rows inside them are judged among themselves only
        a = np.concatenate([np.arange(int(b), int(b) + int(n)) for b, n in zip(got["row_begin"], got["row_count"])])
        outside = (ac[a] < kw.get("min_ac", 0)) | (ac[a] > kw.get("max_ac", UMAX))
        assert outside.any() and np.all(got["state"][outside & ~dropped[a]] == INELIGIBLE)
    _m, _c, _d, out, _b = _check_full(vs, regions, None, (64,), T, "limits", min_ac=lo, max_ac=hi)
    assert int(out[64]["n_kept"].sum()) != int(base[64]["n_kept"].sum())
    vs.close()


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


def test_counts_are_the_count_query_rows(t6_store):
    vs, regions = t6_store
    for sub in (None, [2, 3, 150, 151, 299]):
        res = vs.ld_prune(regions[:2_000], sub, window=16)
        got = res.ld_prune()
        cres = vs.allele_counts(regions[:2_000], sub)
        ac = cres.allele_counts()
        assert np.array_equal(ac["rows"]["pos"], got["rows"]["pos"]) and got["counts"].shape[0] > 2_000
        for f in ("carriers", "alt_alleles", "hom_alt", "phased"):
            assert np.array_equal(got["counts"][f], ac["counts"][f]), (sub, f)
        assert got["counts"]["alt_alleles"].any()
        lay = res.layout()
        assert lay[1] == got["rows"].shape[0] and lay[2] == 0 and lay[3] == 0 and res.fill_ms() > 0
        assert res.totals()[:2] == cres.totals()[:2]
        assert int(got["keep_begin"][-1]) == int(got["row_count"].sum()) == got["state"].shape[0]
        res.close(); cres.close()


# ------------------------------------------------------------------------------------------------ 5, 6. repeats and the pool
def test_identical_calls_give_identical_bytes(t6_store):
    vs, regions = t6_store
    batch = np.ascontiguousarray(regions[:1_500])
    first = None
    for _ in range(3):
        res = vs.ld_prune(batch, window=100, r2=0.1, max_bp=20_000, min_ac=1)
        got = res.ld_prune()
        res.close()
        if first is None:
            first = got
            assert (got["state"] == KEPT).any() and (got["state"] == PRUNED).any()
        for k in ("state", "keep_begin", "n_kept"):
            assert np.array_equal(got[k], first[k]), k


def test_buffers_from_the_pool():
    """A large batch is closed, then small ones on the same handle take its buffers -- state, masks, matrix: every byte of the state
    and every mask word must be written, the zeros included."""
    vs = VariantStore.synthetic(device=0, **T6_KW)
    rng = np.random.default_rng(4)
    s = np.sort(rng.integers(1_000, 7_990_000, size=1_500))
    regions = np.stack([s, s + rng.integers(50, 3_000, size=1_500)], axis=1).astype(np.uint64)
    for T in (0, quantise_r2(0.02)):
        big = vs.ld_prune(regions, window=256, r2=T / ONE)
        assert (big.ld_prune()["state"] == PRUNED).sum() > 500
        big.close()
        _check_full(vs, np.ascontiguousarray(regions[:40]), [5, 9, 11, 200, 250], (33,), ONE, "pool")   # nothing hits: every mask word is 0
        _check_full(vs, np.ascontiguousarray(regions[:40]), None, (64,), T, "pool")
        _check_full(vs, np.ascontiguousarray(regions[:3]), None, (256,), T, "pool")
    vs.close()


# ------------------------------------------------------------------------------------------------ 7. type-6 isolation
def test_interleaving_leaves_type6_alone():
    rng = np.random.default_rng(12)
    batches = []
    for k in range(6):
        n = 3_000 + 200 * k + (4_000 if k == 4 else 0)   # like batches (speculated), one larger (refused / re-sized)
        s = np.sort(rng.integers(1_000, 7_990_000, size=n))
        batches.append(np.stack([s, s + rng.integers(50, 3_000, size=n)], axis=1).astype(np.uint64))
    shuffled = batches[3][rng.permutation(batches[3].shape[0])]

    def run(with_prune):
        vs = VariantStore.synthetic(device=0, **T6_KW)
        digests = []
        for k, b in enumerate(batches):
            r = vs.get_var_in_ref(b)
            if with_prune:   # pruning batches in between: sorted, unsorted, with a subset
                l1 = vs.ld_prune(b, window=16)
                l2 = vs.ld_prune(shuffled, window=64, r2=0.5)
                l3 = vs.ld_prune(shuffled, [1, 5, 7, 200], window=100, max_bp=5_000)
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


# ------------------------------------------------------------------------------------------------ 8. device inputs
def _read_device(torch, ptr, n_bytes):
    return _read_device_bytes(torch, ptr, 1, n_bytes).reshape(n_bytes).copy()


def test_device_regions_and_device_pointers(t6_store):
    """Regions in device memory and the device accessor.  Sample ids are a host list, as for the other LD queries: the C ABI builds
    the subset's mask and ranks from them on the host."""
    torch = pytest.importorskip("torch")
    vs, regions = t6_store
    sub = [3, 17, 40, 200, 250, 251]
    batch = np.ascontiguousarray(regions[:2_500])
    host = vs.ld_prune(batch, sub, window=32, r2=0.0)
    hgot = host.ld_prune()
    t = torch.from_numpy(batch.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    dev = vs.ld_prune(DeviceArray(t.data_ptr(), batch.shape[0]), sub, window=32, r2=0.0)
    dgot = dev.ld_prune()
    for k in ("columns", "row_begin", "row_count", "counts", "state", "keep_begin", "n_kept"):
        assert np.array_equal(hgot[k], dgot[k]), k
    assert (hgot["state"] == KEPT).any() and (hgot["state"] == PRUNED).any()
    ps, pb, pn, pc, nq, a, c = dev.ld_prune_device()
    total = dgot["state"].shape[0]
    assert (nq, a, c) == (2_500, dgot["rows"].shape[0], 6) and ps and pb and pn and pc
    first = _read_device(torch, ps, total)
    later = vs.ld_prune(regions[2_500:2_900], window=8)   # a later batch on the same handle leaves the verdicts alone
    later.totals()
    assert np.array_equal(first, dgot["state"])
    assert np.array_equal(_read_device(torch, ps, total), first)
    assert np.array_equal(_read_device(torch, pb, 8 * (nq + 1)).view(np.uint64), dgot["keep_begin"])
    assert np.array_equal(_read_device(torch, pn, 8 * nq).view(np.uint64), dgot["n_kept"])
    assert np.array_equal(_read_device(torch, pc, a * 16).view(np.uint32).reshape(a, 4), dgot["counts"].view(np.uint32).reshape(a, 4))
    later.close(); host.close(); dev.close()


# ------------------------------------------------------------------------------------------------ 9. the size limit
def test_size_limit(t6_store):
    vs, regions = t6_store
    warm = vs.allele_counts(regions)   # the plan's temporaries, the table and the counts of this batch are in the handle's pool afterwards
    wgot = warm.allele_counts()
    a, states = wgot["rows"].shape[0], int(wgot["row_count"].sum())
    warm.close()
    c = vs.info().num_samples - 1
    pitch = (c + 15) // 16 * 16
    matrix_bytes, mask_bytes = a * pitch, a * 4 * 8
    assert matrix_bytes > 1 << 20
    vs.set_option("matrix_max_mib", 1)
    try:
        before = vs.info().pool_mallocs
        with pytest.raises(VariantStoreError) as e:
            vs.ld_prune(regions, window=256)
        assert e.value.code == VS_ERR_ARG
        msg = str(e.value)
        for what in (f"{regions.shape[0]} regions", f"{a} rows", f"{c} columns", "window 256", str(matrix_bytes), str(mask_bytes), " bytes",
                     "matrix_max_mib"):
            assert what in msg, (what, msg)
        assert vs.info().pool_mallocs == before, "the refused batch allocated"
        few = vs.ld_prune(regions[:20], [1, 2, 3], window=2)   # (16 + 4) bytes a row: below the limit
        assert few.ld_prune()["keep_begin"].shape == (21,)
        few.close()
        # 16 bytes of matrix, 32 of masks and a verdict a row and 16 a region: the matrix alone would fit, the whole does not
        if a * 16 <= 1 << 20 < a * (16 + 32) + states + 16 * regions.shape[0]:
            with pytest.raises(VariantStoreError) as e:
                vs.ld_prune(regions, [1, 2, 3], window=256)
            assert e.value.code == VS_ERR_ARG and f"{a} rows" in str(e.value)
    finally:
        vs.set_option("matrix_max_mib", 0)
    again = vs.ld_prune(regions, window=256)   # the handle stays usable
    got = again.ld_prune()
    assert got["state"].shape == (states,) and (got["state"] == KEPT).any()
    again.close()


# ------------------------------------------------------------------------------------------------ 10. the refused accessors
def test_refused_accessors(t6_store):
    vs, regions = t6_store
    r = vs.ld_prune(regions[:1_000], window=8)
    for call in (lambda: r.raw(with_carriers=True), lambda: r.view(with_carriers=True), r.digest, r.num_header_records,
                 r.num_region_records):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_UNSUPPORTED
    for call in (r.allele_counts, r.sample_burden, r.sample_burden_device, r.genotype_matrix, r.genotype_matrix_device, r.ld_band,
                 r.ld_band_device, r.ld_matrix, r.ld_matrix_device, r.sample_gram, r.sample_ibs):
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
                vs.ld_band(regions[:10], window=4), vs.ld_matrix(regions[:10]), vs.sample_gram(regions[:10])):
        for call in (res.ld_prune, res.ld_prune_device):
            with pytest.raises(VariantStoreError) as e:
                call()   # not a pruning result
            assert e.value.code == VS_ERR_ARG
        res.close()


# ------------------------------------------------------------------------------------------------------------- 11. the CLI
def test_cli_prune(tmp_path):
    """The LD-block cohort through `variantstore construct` and `variantstore prune` (the goldens have one sample: nothing to prune)."""
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
    names = [vs.sample_name(i) for i in range(1, min(4, vs.info().num_samples))]
    sfile = os.path.join(tmp_path, "samples.txt")
    with open(sfile, "w") as f:
        f.write("\n".join(names) + "\n")
    some = False
    for samples, extra in ((None, []), (names, ["-S", sfile])):
        for kw, flags in ((dict(), []), (dict(window=3, r2=0.0), ["-w", "3", "--r2", "0"]), (dict(r2=0.75, max_bp=40), ["--r2", "0.75", "--bp", "40"]),
                          (dict(window=256, min_ac=1, max_ac=3), ["--window", "256", "--min-ac", "1", "--max-ac", "3"])):
            out = os.path.join(tmp_path, "prune.txt")
            subprocess.run([exe, "prune", "-p", prefix, "-r", "@" + rfile, "-o", out] + extra + flags, check=True, capture_output=True)
            with open(out, "rb") as f:
                parts = f.read().decode("latin-1").split("#region ")[1:]
            res = vs.ld_prune(regions, samples, **kw)
            assert len(parts) == len(regions)
            for q, part in enumerate(parts):
                head, text = part.split("\n", 1)
                assert head == f"{q} {regions[q][0]}:{regions[q][1]}"
                assert text == res.region_text(q), (q, kw)
                assert text.startswith("Pos\tRef\tAlt\tAC\tState\n")
                some |= "\tkeep\n" in text and "\tpruned\n" in text
            res.close()
    assert some
    for bad in (["-w", "300"], ["--r2", "1.5"]):
        p = subprocess.run([exe, "prune", "-p", prefix, "-r", "@" + rfile] + bad, capture_output=True, text=True)
        assert p.returncode != 0, bad
    vs.close()
