"""Trio queries on the GPU (vs_query_trio_scan): every record per row and per trio against trio_ref over the engine's own genotype
matrix of the same regions and members -- lane, chunk and pitch edges (1, 63, 64, 65 and 257 trios over 3, 16, 17 and 129 member
columns, the default chunk and chunks of 64 trios), row-block edges and the empty table, a Mendel-consistent pedigree written as VCF
text with planted violations, tables with rows the duplicate rule dropped, saturated rows, determinism, interleaving with type-6
batches, the device pointers, the derived float64 quantities, the size limit, the refused accessors and the CLI.

Every integer is compared bit for bit.  tdt_chi2 and error_rate are compared bit for bit too: both sides convert exact integers to
float64 once, multiply once and divide once."""
import os
import subprocess

import numpy as np
import pytest

from helpers import oracle_texts, random_regions, write_random_cohort, write_saturated_cohort
from test_gpu_genotype_matrix import _oracle, _read_device as _read_device_bytes
from trio_ref import FIELDS, TRIO_DTYPE, dosage, error_rate, states, tdt_chi2, trio_scan, trio_table_text, trio_text
from variantstore_amd import VariantStore
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_ARG, VS_ERR_UNSUPPORTED = -5, -7


def make_trios(members, n_trios, rng):
    """(n_trios, 3) sample ids -- child, father, mother -- over `members` (three or more ids), every member in some trio: members are
    drawn with reuse, a sample is a child in one trio and a parent in another, one father has three children, the order is shuffled."""
    members = [int(i) for i in members]
    n = len(members)
    assert n >= 3 and 3 * n_trios >= n
    perm = rng.permutation(n)
    out = [[int(perm[k]), int(perm[(k + 1) % n]), int(perm[(k + 2) % n])] for k in range(0, n, 3)]   # every member once
    if n >= 5 and n_trios >= len(out) + 4:
        a, b, c, d, e = (int(x) for x in rng.choice(n, size=5, replace=False))
        out += [[c, a, b], [d, a, b], [e, a, c], [a, d, e]]   # a: father of c, d and e, and a child of d and e; c: a child, then a mother
    while len(out) < n_trios:
        out.append([int(x) for x in rng.choice(n, size=3, replace=False)])
    out = np.asarray(out[:n_trios])
    assert out.shape[0] == n_trios and np.unique(out).shape[0] == n
    return np.asarray(members, np.uint32)[out[rng.permutation(n_trios)]]


def _row_keys(rows, stats):
    """The table's rows with their records as sorted tuples: what two calls must agree on whatever the order of private rows."""
    cols = [rows["pos"].astype(np.int64), rows["alt_off"].astype(np.int64), rows["alt_len"].astype(np.int64), rows["count_flags"].astype(np.int64)]
    cols += [stats[f].astype(np.int64) for f in FIELDS]
    return sorted(zip(*[c.tolist() for c in cols]))


def _heads(vs, regions, members):
    """"Pos\\tRef\\tAlt" of the rows every region reports, dropped rows left out: from the count query's text."""
    res = vs.allele_counts(regions, members)
    out = [["\t".join(ln.split("\t")[:3]) for ln in res.region_text(q).split("\n")[1:] if ln] for q in range(len(regions))]
    res.close()
    return out


def _check_full(vs, regions, trios, what=None, texts=0, conditions=True):
    """Both record arrays, n_used and the derived quantities against trio_ref over genotype_matrix() of the same regions and the
    trios' members (the dropped rows from the table's count_flags).  The table's rows may come in another order in the two calls
    (the private rows of regions under the duplicate rule): rows are compared as sorted (row, record) tuples, and in place when the
    order is the same.  `texts`: region_text of every texts-th region too.  Returns (matrix arrays, expected dict, result arrays)."""
    trios = np.asarray(trios, np.uint32).reshape(-1, 3)
    members = sorted({int(i) for i in trios.ravel()})
    mres = vs.genotype_matrix(regions, members)
    m = mres.genotype_matrix()
    mres.close()
    cells = np.ascontiguousarray(m["cells"])
    a, n = cells.shape
    assert m["columns"].tolist() == members and n == len(members)
    col_of = {s: k for k, s in enumerate(members)}
    tcols = np.asarray([[col_of[int(s)] for s in t] for t in trios], np.uint32)
    dropped = (m["rows"]["count_flags"] >> 31) != 0
    want = trio_scan(cells, tcols, dropped)
    res = vs.trio_scan(regions, trios)
    got = res.trio_scan()
    assert got["columns"].dtype == np.uint32 and got["columns"].tolist() == members
    assert got["trio_cols"].dtype == np.uint32 and np.array_equal(got["trio_cols"], tcols) and np.array_equal(got["trio_ids"], trios)
    assert got["row_stats"].dtype == TRIO_DTYPE and got["row_stats"].shape == (a,) and got["counts"].shape == (a,)
    assert got["trio_stats"].dtype == TRIO_DTYPE and got["trio_stats"].shape == (trios.shape[0],)
    assert got["n_used"] == want["n_used"] == a - int(dropped.sum()), (what, got["n_used"], want["n_used"])
    for f in FIELDS:
        bad = np.nonzero(got["trio_stats"][f] != want["trio_stats"][f])[0]
        assert bad.shape[0] == 0, (what, "trio", f, bad[:8].tolist(), got["trio_stats"][f][bad[:8]].tolist(), want["trio_stats"][f][bad[:8]].tolist())
    assert _row_keys(got["rows"], got["row_stats"]) == _row_keys(m["rows"], want["row_stats"]), what
    same_order = np.array_equal(got["rows"]["pos"], m["rows"]["pos"]) and np.array_equal(got["rows"]["alt_off"], m["rows"]["alt_off"]) and \
        np.array_equal(got["rows"]["count_flags"], m["rows"]["count_flags"])
    if same_order:
        for f in FIELDS:
            bad = np.nonzero(got["row_stats"][f] != want["row_stats"][f])[0]
            assert bad.shape[0] == 0, (what, "row", f, bad[:8].tolist())
        assert np.array_equal(got["row_begin"], m["row_begin"])
        assert np.array_equal(got["counts"]["alt_alleles"].astype(np.int64), dosage(cells).sum(axis=1))
    assert np.array_equal(got["row_count"], m["row_count"])
    assert not got["row_stats"].view(np.uint32).reshape(a, 4)[(got["rows"]["count_flags"] >> 31) != 0].any(), "a dropped row's record is zero"
    # the derived quantities, bit for bit, from the result's own integers
    assert got["tdt_chi2"].dtype == np.float64 and got["tdt_chi2"].tobytes() == tdt_chi2(got["row_stats"]).tobytes()
    assert got["error_rate"].dtype == np.float64 and got["error_rate"].tobytes() == error_rate(got["trio_stats"], got["n_used"]).tobytes()
    assert res.totals()[2] == int(np.count_nonzero(cells))
    if conditions and trios.shape[0] >= 3:   # a wrong table or lane map cannot hide
        assert np.unique(states(cells, tcols)).shape[0] == 27, (what, np.unique(states(cells, tcols)).tolist())
        for axis in ("row_stats", "trio_stats"):
            arrays = [want[axis][f] for f in FIELDS]
            assert all(not np.array_equal(arrays[i], arrays[j]) for i in range(4) for j in range(i)), (what, axis)
        assert np.unique(want["trio_stats"]).shape[0] > 1, "every trio has the same record"
    if texts and same_order:
        heads = _heads(vs, regions, members)
        ac = dosage(cells).sum(axis=1)
        for q in range(0, len(regions), texts):
            a0, k = int(m["row_begin"][q]), int(m["row_count"][q])
            gone = dropped[a0:a0 + k]
            it = iter(heads[q])
            hq = [None if g else next(it) for g in gone]
            assert res.region_text(q) == trio_text(hq, ac[a0:a0 + k], want["row_stats"][a0:a0 + k], gone), (what, q)
            sub = res.region_trio_stats(q, got)
            assert np.array_equal(sub["row_stats"], got["row_stats"][a0:a0 + k]) and sub["rows"].shape == (k,)
    res.close()
    return m, want, got


# ------------------------------------------------------------------------------------- 1. lane, chunk and pitch edges
# member columns -> (seed, samples of the cohort).  Three columns of a cohort of nine: in a cohort of three every row has a carrier
# among the three, and the state "nobody carries it" would never occur.
COHORTS = {3: (4101, 9), 16: (4103, 66), 17: (4103, 66), 129: (4104, 130)}
_open = {}


@pytest.fixture(scope="module")
def cohorts(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("trio_cohorts"))

    def get(seed, n_samples):
        if seed not in _open:
            fasta, vcf, _names = write_random_cohort(d, seed, ref_len=6000, n_rows=400, n_samples=n_samples, carrier_p=0.5)
            _open[seed] = VariantStore.from_vcf(fasta, vcf, device=0)
        return _open[seed]
    yield get
    for vs in _open.values():
        vs.close()
    _open.clear()


def _regions(rng):
    return [(int(s), int(s) + int(rng.integers(1, 900))) for s in rng.integers(1, 5900, size=40)] + [(1, 6001), (5000, 6100)]


@pytest.mark.parametrize("n_trios,n_cols", [(1, 3)] + [(t, c) for t in (63, 64, 65, 257) for c in (3, 16, 17, 129)])
def test_every_record_against_the_matrix(n_trios, n_cols, cohorts):
    """One lane, a wave less one, a full wave, a wave and one, several slabs and a remainder (257 = 4 x 64 + 1) x pitches of 16, 16,
    32 and 144 bytes with 3, 16, 17 and 129 columns in use; under the default chunk (one chunk: plain stores for the rows) and under
    trio_chunk = 64 (several chunks plus a remainder: the atomic path).  The batch is unsorted: the device sorts it."""
    seed, n_samples = COHORTS[n_cols]
    vs = cohorts(seed, n_samples)
    rng = np.random.default_rng(1000 * n_trios + n_cols)
    members = np.sort(rng.choice(np.arange(1, n_samples + 1), size=n_cols, replace=False))
    trios = make_trios(members, n_trios, rng)
    if n_trios >= 63 and n_cols >= 16:
        assert (trios[:, 0] < trios[:, 1:].min(axis=1)).any() and (trios[:, 0] > trios[:, 1:].max(axis=1)).any()
        children, parents = set(trios[:, 0].tolist()), set(trios[:, 1:].ravel().tolist())
        assert children & parents and np.unique(trios[:, 1], return_counts=True)[1].max() >= 3
    regions = _regions(rng)
    outs = []
    for chunk in (0, 64):
        vs.set_option("trio_chunk", chunk)
        m, _want, got = _check_full(vs, regions, trios, (n_trios, n_cols, chunk), texts=7 if chunk == 0 else 0)
        assert m["cells"].shape[1] == n_cols and m["row_pitch"] == (n_cols + 15) // 16 * 16 and m["cells"].shape[0] > 400
        outs.append((got["row_stats"].tobytes(), got["trio_stats"].tobytes(), got["n_used"]))
    vs.set_option("trio_chunk", 0)
    assert outs[0] == outs[1]


# ------------------------------------------------------------------------------------------------- 2. row-block edges
def test_small_tables_and_the_empty_one(cohorts):
    """Tables of 0, 1, 15, 16, 17 and 33 rows: less than a block of 16 rows, exactly one, one and a row, two and a row."""
    vs = cohorts(4103, 66)
    trios = np.arange(1, 67, dtype=np.uint32).reshape(22, 3)
    probe = vs.allele_counts([(1, 6001)])
    pos = np.unique(probe.allele_counts()["rows"]["pos"].astype(np.int64))
    probe.close()
    spans = [(int(pos[k]), int(pos[k + m])) for m in (0, 1, 2, 13, 14, 15, 16, 17, 30, 31, 32, 33, 34) for k in range(0, 60, 3)]
    cres = vs.allele_counts(spans)
    n_rows = cres.allele_counts()["row_count"].astype(np.int64)
    cres.close()
    for chunk in (0, 64):
        vs.set_option("trio_chunk", chunk)
        for want in (1, 15, 16, 17, 33):
            hit = np.nonzero(n_rows == want)[0]
            assert hit.size, (want, sorted(set(n_rows.tolist())))
            m, _w, _g = _check_full(vs, [spans[int(hit[0])]], trios, (want, chunk), texts=1, conditions=False)
            assert m["cells"].shape[0] == want
        gap = int(pos[np.argmax(np.diff(pos))])   # the widest stretch without a record: no row's extent (at most 5 bases) reaches its middle
        assert int(np.diff(pos).max()) >= 14
        res = vs.trio_scan([(gap + 7, gap + 8)], trios)   # a table without rows: all-zero records and n_used = 0, not an error
        got = res.trio_scan()
        assert got["n_used"] == 0 and got["row_stats"].shape == (0,) and got["rows"].shape == (0,) and got["tdt_chi2"].shape == (0,)
        assert got["trio_stats"].shape == (22,) and not got["trio_stats"].view(np.uint32).any() and np.isnan(got["error_rate"]).all()
        assert res.totals()[1:3] == (0, 0) and res.region_text(0) == "Pos\tRef\tAlt\tAC\tErrors\tDeNovo\tT\tU\n"
        dev = res.trio_scan_device()
        assert (dev["n_rows"], dev["n_cols"], dev["n_trios"]) == (0, 66, 22)
        res.close()
    vs.set_option("trio_chunk", 0)


# --------------------------------------------------------------------------------- 3. a pedigree written as VCF text
def write_pedigree(dirpath, seed=77, n_rows=100, n_trios=20, ref_len=6000, n_planted=12):
    """FASTA + VCF of a Mendel-consistent pedigree: n_trios trios over 2 n_trios founders, n_rows single-ALT rows; founders random and
    phased, each child takes one gamete from each parent; n_planted violations at recorded (row, child) cells.  Returns (fasta, vcf,
    positions, planted, expected records per row, per trio) -- the records from the construction alone."""
    rng = np.random.default_rng(seed)
    bases = "ACGT"
    ref = "".join(bases[i] for i in rng.integers(0, 4, size=ref_len))
    # (fathers, mothers, children; the names ascend in the order of the VCF's columns, as in every cohort of this suite)
    names = [f"A{t:02d}f" for t in range(n_trios)] + [f"B{t:02d}m" for t in range(n_trios)] + [f"C{t:02d}c" for t in range(n_trios)]
    hap = (rng.random((n_rows, 2 * n_trios, 2)) < 0.35).astype(np.int64)          # founders' haplotypes: [row, founder, slot]
    pick = rng.integers(0, 2, size=(n_rows, n_trios, 2))                         # which slot the father / the mother gave
    fa, mo = hap[:, :n_trios], hap[:, n_trios:]
    g_f = np.take_along_axis(fa, pick[:, :, :1], axis=2)[:, :, 0]                # the gametes: [row, trio]
    g_m = np.take_along_axis(mo, pick[:, :, 1:], axis=2)[:, :, 0]
    child = np.stack([g_f, g_m], axis=2)                                         # the child's call, father's gamete first
    df, dm = fa.sum(axis=2), mo.sum(axis=2)
    planted = {}
    while len(planted) < n_planted:
        r, t = int(rng.integers(0, n_rows)), int(rng.integers(0, n_trios))
        f, m = int(df[r, t]), int(dm[r, t])
        allowed = {a + b for a in ((0,), (0, 1), (1,))[f] for b in ((0,), (0, 1), (1,))[m]}
        wrong = [c for c in (0, 1, 2) if c not in allowed]
        if (r, t) in planted or not wrong:
            continue
        planted[(r, t)] = int(rng.choice(wrong))
    for (r, t), c in planted.items():
        child[r, t] = ((0, 0), (1, 0), (1, 1))[c]
    assert any(df[r, t] == 0 and dm[r, t] == 0 for r, t in planted), "no planted cell has both parents 0|0"
    assert any(df[r, t] + dm[r, t] > 0 for r, t in planted)
    positions = [50 + 55 * r for r in range(n_rows)]
    fasta, vcf = os.path.join(dirpath, "ped.fa"), os.path.join(dirpath, "ped.vcf")
    with open(fasta, "w") as f:
        f.write(">c1 pedigree\n" + "".join(ref[i:i + 60] + "\n" for i in range(0, ref_len, 60)))
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.1\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n")
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n")
        for r, p in enumerate(positions):
            r0 = ref[p - 1]
            calls = [f"{a}|{b}" for a, b in hap[r]] + [f"{a}|{b}" for a, b in child[r]]
            assert any(c != "0|0" for c in calls)
            f.write(f"c1\t{p}\t.\t{r0}\t{bases[(bases.index(r0) + 1) % 4]}\t99\t.\t.\tGT\t" + "\t".join(calls) + "\n")
    # the expected records, from the construction
    is_err = np.zeros((n_rows, n_trios), bool)
    for r, t in planted:
        is_err[r, t] = True
    ok = ~is_err
    want_rows, want_trios = np.zeros(n_rows, TRIO_DTYPE), np.zeros(n_trios, TRIO_DTYPE)
    cells4 = np.stack([is_err, is_err & (df == 0) & (dm == 0),
                       ok * ((df == 1) * g_f + (dm == 1) * g_m), ok * ((df == 1) * (1 - g_f) + (dm == 1) * (1 - g_m))]).astype(np.int64)
    for k, name in enumerate(FIELDS):
        want_rows[name], want_trios[name] = cells4[k].sum(axis=1), cells4[k].sum(axis=0)
    assert int(want_rows["errors"].sum()) == n_planted and 0 < int(want_rows["denovo"].sum()) < n_planted
    het_parents = (ok * ((df == 1).astype(np.int64) + (dm == 1))).sum(axis=1)
    assert np.array_equal(want_rows["transmitted"].astype(np.int64) + want_rows["untransmitted"], het_parents)
    return fasta, vcf, positions, planted, want_rows, want_trios


def test_mendel_consistent_pedigree_with_planted_violations(tmp_path):
    """20 trios over 40 founders, 100 single-ALT rows: founders random and phased, each child takes one gamete from each parent, about
    12 violations planted at recorded (row, child) cells.  The expected records follow from the construction alone -- no constructor,
    no oracle, no closed form: errors exactly at the planted cells, de novo exactly where both parents are 0|0, T and U from the
    gametes the heterozygous parents of the consistent cells actually gave."""
    n_rows, n_trios, ref_len = 100, 20, 6000
    fasta, vcf, positions, planted, want_rows, want_trios = write_pedigree(str(tmp_path))
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    trios = [(f"C{t:02d}c", f"A{t:02d}f", f"B{t:02d}m") for t in range(n_trios)]
    for chunk in (0, 64):
        vs.set_option("trio_chunk", chunk)
        res = vs.trio_scan([(1, ref_len)], trios)
        got = res.trio_scan()
        assert got["rows"]["pos"].tolist() == positions and got["n_used"] == n_rows
        for name in FIELDS:
            assert np.array_equal(got["row_stats"][name], want_rows[name]), (name, chunk)
            assert np.array_equal(got["trio_stats"][name], want_trios[name]), (name, chunk)
        assert np.array_equal(np.nonzero(got["row_stats"]["errors"])[0], np.unique([r for r, _t in planted]))
        res.close()
    _check_full(vs, [(1, 3000), (2500, ref_len)], np.asarray([[vs.sample_id(x) for x in t] for t in trios], np.uint32), "pedigree", texts=1, conditions=False)
    vs.close()


# --------------------------------------------------------------------------------------------------- 4. dropped rows
def test_rows_the_duplicate_rule_dropped(tmp_path):
    """Near and equal records: the duplicate rule drops rows of the table.  They add nothing, their record is zero, and they are
    excluded from n_used.  The regions under the rule report private copies of their rows, whose order is not fixed: the sums are
    compared irrespective of the order of the rows."""
    fasta, vcf, _names = write_random_cohort(str(tmp_path), 701, ref_len=6000, n_rows=400, n_samples=9, p_near=0.6, p_multi=0.3, p_same=0.3,
                                             unphased_p=0.4, carrier_p=0.5)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    texts = oracle_texts(_oracle(vs, tmp_path), random_regions(np.random.default_rng(701), 6000, 300, max_len=900))
    regions = [r for r, (n, _e, _t) in zip(random_regions(np.random.default_rng(701), 6000, 300, max_len=900), texts) if n >= 0]
    assert len(regions) > 200   # (only the regions the reference's walk terminates on: the rows of the others are not defined)
    trios = np.asarray([(1, 2, 3), (4, 5, 6), (7, 8, 9), (2, 9, 4), (5, 1, 7)], np.uint32)
    for chunk in (0, 64):
        vs.set_option("trio_chunk", chunk)
        _m, _want, got = _check_full(vs, regions, trios, ("duplicate rule", chunk))
        dropped = (got["rows"]["count_flags"] >> 31) != 0
        assert dropped.any(), "no row of the batch was dropped by the duplicate rule"
        assert got["n_used"] == got["rows"].shape[0] - int(dropped.sum()) < got["rows"].shape[0]
        assert not got["row_stats"].view(np.uint32).reshape(-1, 4)[dropped].any() and not got["counts"]["carriers"][dropped].any()
    vs.set_option("trio_chunk", 0)
    vs.close()


# ------------------------------------------------------------------------------------------------- 5. saturated rows
def test_saturated_rows(tmp_path):
    """Rows carried by 75 - 100 % of the samples: child, father and mother are all carriers in most cells and all 1/1 in hundreds, a
    state the random cohorts barely reach; a cohort of 130 samples, 40 trios."""
    fasta, vcf = write_saturated_cohort(str(tmp_path), 130, 515)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    rng = np.random.default_rng(5)
    trios = make_trios(np.arange(1, 131), 44, rng)[:40]
    regions = [(1, 7000), (6000, 14000), (13000, 20001), (500, 900)]
    for chunk in (0, 64):
        vs.set_option("trio_chunk", chunk)
        m, want, got = _check_full(vs, regions, trios, ("saturated", chunk), texts=1, conditions=False)
        members = sorted({int(i) for i in trios.ravel()})
        col_of = {s: k for k, s in enumerate(members)}
        s = states(m["cells"], [[col_of[int(x)] for x in t] for t in trios])
        count = np.bincount(s.ravel(), minlength=27)
        all_carriers = [9 * f + 3 * m_ + c for f in (1, 2) for m_ in (1, 2) for c in (1, 2)]
        assert 2 * int(count[all_carriers].sum()) > s.size and count[26] >= 100 and count.min() > 0, count.tolist()
        assert want["row_stats"]["errors"].any() and want["trio_stats"]["transmitted"].any() and got["n_used"] >= 150
    vs.set_option("trio_chunk", 0)
    vs.close()


# ---------------------------------------------------------------------------------- 6. - 10. a type-6 sized cohort
T6_KW = dict(ref_length=8_000_000, num_variants=150_000, num_samples=300, seed=5, first_pos=1_000, frac_ins=0.05, frac_del=0.05,
             frac_multi=0.02, max_indel=6, af_exponent=2.0)


@pytest.fixture(scope="module")
def t6_store():
    vs = VariantStore.synthetic(device=0, **T6_KW)
    rng = np.random.default_rng(12)
    s = np.sort(rng.integers(1_000, 7_990_000, size=3_000))
    regions = np.stack([s, s + rng.integers(50, 3_000, size=3_000)], axis=1).astype(np.uint64)
    trios = make_trios(np.arange(1, 301), 257, rng)
    yield vs, regions, trios
    vs.close()


def test_two_calls_and_every_chunk_give_the_same_bytes(t6_store):
    vs, regions, trios = t6_store
    outs = []
    for chunk in (0, 0, 64, 128, 16384):
        vs.set_option("trio_chunk", chunk)
        r = vs.trio_scan(regions, trios)
        g = r.trio_scan()
        outs.append((g["row_stats"].tobytes(), g["trio_stats"].tobytes(), g["n_used"], g["counts"].tobytes()))
        assert r.fill_ms() > 0 and r.layout()[2] == 0
        r.close()
    vs.set_option("trio_chunk", 0)
    assert all(o == outs[0] for o in outs) and any(outs[0][0]) and any(outs[0][1]) and outs[0][2] > 0
    m, _want, _got = _check_full(vs, regions[:400], trios, "t6")   # (the reference over a part: 257 trios x every row is large)
    assert m["cells"].shape[0] > 3_000
    cres = vs.allele_counts(regions, sorted({int(i) for i in trios.ravel()}))
    assert cres.allele_counts()["counts"].tobytes() == outs[0][3]
    cres.close()


def test_interleaving_leaves_type6_alone():
    rng = np.random.default_rng(12)
    batches = []
    for k in range(6):
        n = 3_000 + 200 * k + (4_000 if k == 4 else 0)   # like batches (speculated), one larger (refused / re-sized)
        s = np.sort(rng.integers(1_000, 7_990_000, size=n))
        batches.append(np.stack([s, s + rng.integers(50, 3_000, size=n)], axis=1).astype(np.uint64))
    shuffled = batches[3][rng.permutation(batches[3].shape[0])]
    trios = make_trios(np.arange(1, 301), 100, rng)

    def run(with_trios):
        vs = VariantStore.synthetic(device=0, **T6_KW)
        digests = []
        for b in batches:
            r = vs.get_var_in_ref(b)
            if with_trios:   # trio batches in between: sorted, unsorted, a single trio
                for g in (vs.trio_scan(b, trios), vs.trio_scan(shuffled, trios[:65]), vs.trio_scan(shuffled, [(7, 200, 1)])):
                    g.totals()
                    g.close()
            digests.append(r.digest())
            r.close()
        info = vs.info()
        out = (digests, info.t6_speculated, info.t6_refused)
        vs.close()
        return out

    plain, mixed = run(False), run(True)
    assert plain[1] > 0, "the type-6 batches were not speculated"
    assert plain == mixed


def test_device_pointers(t6_store):
    torch = pytest.importorskip("torch")
    vs, regions, trios = t6_store
    r = vs.trio_scan(regions[:2_500], trios[:70])
    got = r.trio_scan()
    dev = r.trio_scan_device()
    a, t = got["rows"].shape[0], 70
    assert (dev["n_rows"], dev["n_cols"], dev["n_trios"]) == (a, got["columns"].shape[0], t) and dev["rows"] and dev["counts"]
    assert dev["trios"] == dev["rows"] + 16 * a and dev["n_used"] == dev["trios"] + 16 * t
    later = vs.trio_scan(regions[2_500:2_900], trios)   # a later batch on the same handle leaves the result alone
    later.totals()
    assert _read_device_bytes(torch, dev["rows"], a, 16).tobytes() == got["row_stats"].tobytes() and got["row_stats"].view(np.uint32).any()
    assert _read_device_bytes(torch, dev["trios"], t, 16).tobytes() == got["trio_stats"].tobytes() and got["trio_stats"].view(np.uint32).any()
    assert int(_read_device_bytes(torch, dev["n_used"], 1, 8).view(np.uint64)[0, 0]) == got["n_used"] > 0
    assert _read_device_bytes(torch, dev["counts"], a, 16).tobytes() == got["counts"].tobytes()
    later.close(); r.close()


def test_size_limit(t6_store):
    vs, regions, trios = t6_store
    warm = vs.allele_counts(regions, np.unique(trios))   # the plan's temporaries, the table and the counts of this batch are in the handle's pool afterwards
    a = warm.allele_counts()["rows"].shape[0]
    warm.close()
    c, t = np.unique(trios).shape[0], trios.shape[0]
    pitch = (c + 15) // 16 * 16
    total = a * (pitch + 32) + t * 28
    assert a * pitch > 4 << 20
    vs.set_option("matrix_max_mib", 4)
    try:
        before = vs.info().pool_mallocs
        with pytest.raises(VariantStoreError) as e:
            vs.trio_scan(regions, trios)
        assert e.value.code == VS_ERR_ARG
        msg = str(e.value)
        for number in (a, c, t, total, a * pitch, a * 16, t * 16, t * 12):
            assert str(number) in msg, (number, msg)
        assert "matrix_max_mib" in msg and "bytes" in msg, msg
        assert vs.info().pool_mallocs == before, "a refused batch allocated"
        few = vs.trio_scan(regions[:20], trios)   # below the limit
        assert few.trio_scan()["trio_stats"].shape == (t,)
        few.close()
    finally:
        vs.set_option("matrix_max_mib", 0)
    again = vs.trio_scan(regions, trios)
    assert again.trio_scan()["row_stats"].shape == (a,)
    again.close()


def test_refused_accessors(t6_store):
    vs, regions, trios = t6_store
    r = vs.trio_scan(regions[:1_000], trios)
    for call in (lambda: r.raw(with_carriers=True), lambda: r.view(with_carriers=True), r.digest, r.num_header_records, r.num_region_records):
        with pytest.raises(VariantStoreError) as e:
            call()
        assert e.value.code == VS_ERR_UNSUPPORTED
    for call in (r.allele_counts, r.sample_burden, r.sample_burden_device, r.genotype_matrix, r.genotype_matrix_device, r.ld_band,
                 r.ld_band_device, r.sample_scores, r.sample_gram, r.sample_ibs, r.sample_ibs_device, r.assoc_scan, r.group_counts, r.ld_scores):
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
    assert r.totals()[:2] == t6.totals()[:2] and r.fill_ms() > 0 and r.region_text(0).startswith("Pos\tRef\tAlt\tAC\tErrors\tDeNovo\tT\tU\n")
    r.close()
    for res in (t6, vs.allele_counts(regions[:10]), vs.genotype_matrix(regions[:10]), vs.sample_ibs(regions[:10], [1, 2, 3])):
        with pytest.raises(VariantStoreError) as e:
            res.trio_scan()   # not a trio result
        assert e.value.code == VS_ERR_ARG
        with pytest.raises(VariantStoreError) as e:
            res.trio_scan_device()
        assert e.value.code == VS_ERR_ARG
        res.close()


# ------------------------------------------------------------------------------------------------------------ 11. the CLI
def test_cli_trios(tmp_path):
    """Nine samples, a trio file of three-field lines and PED lines with founders: the regions' text and the per-trio table."""
    exe = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    fasta, vcf, names = write_random_cohort(str(tmp_path), 4101, ref_len=6000, n_samples=9, carrier_p=0.5)
    subprocess.run([exe, "construct", "-r", fasta, "-v", vcf, "-p", prefix], check=True, capture_output=True)
    vs = VariantStore.open(prefix, device=0)
    regions = sorted([(x, x + 250) for x in range(1, 5900, 300)] + [(1000, 3000)])   # (the command line sorts its regions, as the reference's driver does)
    rfile = os.path.join(tmp_path, "regions.txt")
    with open(rfile, "w") as f:
        f.write("".join(f"{x}:{y}\n" for x, y in regions))
    tnames = [(names[6], names[7], names[8]), (names[0], names[1], names[2]), (names[3], names[4], names[5]), (names[1], names[6], names[3])]
    tfile = os.path.join(tmp_path, "trios.ped")
    with open(tfile, "w") as f:
        f.write(f"{tnames[0][0]} {tnames[0][1]} {tnames[0][2]}\n# a comment\nfam1 {tnames[1][0]} {tnames[1][1]} {tnames[1][2]} 1 2\n")
        f.write(f"fam1 {names[1]} 0 0 1 1\nfam1 {names[2]} 0 0 2 1\n\n{tnames[2][0]}\t{tnames[2][1]}\t{tnames[2][2]}\nfam2 {tnames[3][0]} {tnames[3][1]} {tnames[3][2]} 2 2 x y\n")
    out = os.path.join(tmp_path, "trios.txt")

    def run(flags):
        p = subprocess.run([exe, "trios", "-p", prefix, "-r", "@" + rfile, "-T", tfile, "-o", out] + flags, check=True, capture_output=True)
        assert p.stdout == b"" and b"skipped 2 line(s)" in p.stderr
        with open(out, "rb") as f:
            return f.read().decode("latin-1")

    trios = np.asarray([[vs.sample_id(x) for x in t] for t in tnames], np.uint32)
    m, want, got = _check_full(vs, regions, trios, "cli")
    res = vs.trio_scan(regions, tnames)
    assert res.trio_scan()["trio_stats"].tobytes() == got["trio_stats"].tobytes()
    assert run(["--per-trio"]) == trio_table_text(tnames, want["trio_stats"], want["n_used"])
    text = run([])
    parts = text.split("#region ")[1:]
    assert len(parts) == len(regions)
    heads = _heads(vs, regions, sorted({int(i) for i in trios.ravel()}))
    dropped = (m["rows"]["count_flags"] >> 31) != 0
    ac = dosage(m["cells"]).sum(axis=1)
    for q, part in enumerate(parts):
        head, body = part.split("\n", 1)
        assert head == f"{q} {regions[q][0]}:{regions[q][1]}"
        a0, k = int(got["row_begin"][q]), int(got["row_count"][q])
        it = iter(heads[q])
        hq = [None if g else next(it) for g in dropped[a0:a0 + k]]
        assert body == trio_text(hq, ac[a0:a0 + k], got["row_stats"][a0:a0 + k], dropped[a0:a0 + k]) == res.region_text(q), q
    assert want["trio_stats"]["errors"].any() and want["trio_stats"]["transmitted"].any()
    res.close()
    vs.close()
