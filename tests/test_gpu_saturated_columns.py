"""The column queries -- allele_counts, group_counts, assoc_scan, sample_scores, sample_burden, genotype_matrix, ld_band, sample_gram
and its GRM -- on SATURATED rows: rows carried by 75 - 100 % of the samples, which VariantStore.synthetic cannot produce (it caps an
allele's frequency at 0.5) and which only helpers.write_saturated_cohort writes.  They all read a row's carriers through
k_carriers.hip.h (class_chunk, group_load, column_of), a decoder of its own beside the expansion kernels'.

Two legs per (cohort width, VS_LIST_MAX):
  text     two_alt=False, extremes=True against vcf_truth.TextOracle: the expected answer comes from the VCF TEXT alone, no
           constructor and no graph in the loop (tests/test_vcf_truth.py holds TextOracle to the oracle on the CPU)
  oracle   two_alt=True, extremes=True against the oracle, for the two-ALT rows the text does not fix (64, 4095, 4159 samples)
and a third at 63, 300 and 4159 samples with VS_LIST_MAX unset:
  explicit two_alt=False, sparse_head=100 against vcf_truth.TextOracle: the cohort opens with EXPLICIT sample ids (the constructor
           looks at the first 99 records) and its records from 100 on are carried by 70 - 100 % of the samples -- the explicit side
           of k_carriers.hip.h on lists hundreds of groups long.  No extreme rows: the checks that read them are left out.

Widths (samples -> words per class row): 63 -> 1 (one full word, the ref bit included), 64 -> 2 (one bit in the second),
4031 -> 63 (the widest non-WIDE row, its last word full), 4095 -> 64 (the 64-word form, full), 4159 -> 65 (a second round of the
dense loop: lane 0 full, `before` = 4095 carried over), 8255 -> 129 (a full middle chunk whose first carrier record is not a
multiple of 8: k_group_counts stages 513 genotype words).  VS_LIST_MAX unset (63 and 64 samples: the saturated rows are LISTED, 63
of 63), 0 (everything dense, at one and two words too) and, at the three middle widths, 64.

Every family goes through its own file's checker and reference module; the batch is 70 sorted overlapping regions with ends on
the midpoints of the gaps between records, the whole reference and an empty region, sorted -- and the same regions shuffled.
The extreme rows (helpers.write_saturated_cohort: everybody 1/1, 1|1, 0|1, 1/0, all but sample 1, all but the last sample) lie in
the first wave's rows beside ordinary ones; the preconditions that make a cell prove anything are asserted from the VCF text.

Then the 16-bit packed fields of k_group_counts at the admitted maximum of 32,767 samples (alt_alleles = 65,534 in one group: one
more would carry into hom_alt) and the refusal one sample above it."""
import os

import numpy as np
import pytest

import sample_gram_ref
import vcf_truth as vt
from genotype_matrix_ref import Parsed as MatrixParsed, matrix
from group_counts_ref import parse_region
from helpers import SAT_REF_LEN, write_saturated_cohort
from oracle.oracle import Oracle
from sample_burden_ref import Parsed as BurdenParsed
from test_gpu_allele_counts import _check_texts
from test_gpu_assoc_scan import _check_int, _int_traits
from test_gpu_genotype_matrix import _check as _check_matrix, _columns
from test_gpu_group_counts import FIELDS, _check_parsed, _members, _partition
from test_gpu_ld_band import _check_oracle as _check_ld
from test_gpu_row_width_edges import _Memo
from test_gpu_sample_burden import _check as _check_burden
from test_gpu_sample_gram import _want as _gram_want
from test_gpu_sample_scores import _check as _check_scores, _int_weights
from variantstore_amd import VariantStore
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
VS_ERR_UNSUPPORTED = -7
ROWS = {63: 150, 64: 150, 4031: 150, 4095: 150, 4159: 150, 8255: 70}   # (never below 65: one wave's rows plus one)
CELLS = [(n, lm, leg) for n in ROWS for lm in ((None, 0, 64) if n in (4031, 4095, 4159) else (None, 0))
         for leg in (("text", "oracle") if n in (64, 4095, 4159) else ("text",))]
# dense EXPLICIT-ID cohorts (sparse_head=100: the constructor chooses explicit sample ids from the first 99 records, the records from
# 100 on are carried by 70 - 100 % of the samples): the explicit side of k_carriers.hip.h on lists hundreds of groups long, with
# 16-bit (63, 300) and 32-bit (4159) carrier words
CELLS += [(n, None, "explicit") for n in (63, 300, 4159)]


def _open_with_list_max(fasta, vcf, list_max):
    """from_vcf with VS_LIST_MAX set (None: unset) while the index is opened; the variable is put back afterwards."""
    old = os.environ.pop("VS_LIST_MAX", None)
    if list_max is not None:
        os.environ["VS_LIST_MAX"] = str(list_max)
    try:
        return VariantStore.from_vcf(fasta, vcf, device=0)
    finally:
        os.environ.pop("VS_LIST_MAX", None)
        if old is not None:
            os.environ["VS_LIST_MAX"] = old


class _Cohort:
    """One saturated cohort, written and opened once: the store, the expected-answer source (`orc`: TextOracle or the memoised
    oracle), the two batches, and the parsed expected texts every family's checker takes, each parsed at first use."""

    def __init__(self, n, list_max, leg, tmp, rows=None):
        self.n, self.leg, self.rows = n, leg, ROWS.get(n, 150) if rows is None else rows
        kw = dict(sparse_head=100, extremes=False) if leg == "explicit" else dict(extremes=True)
        fasta, vcf = write_saturated_cohort(str(tmp), n, 4400 + n, rows=self.rows, two_alt=leg == "oracle", **kw)
        self.vs = _open_with_list_max(fasta, vcf, list_max)
        info = self.vs.info()
        self.list_max = 640 if list_max is None else list_max
        self.wpc = (n + 1 + 63) // 64
        assert info.num_samples - 1 == n and bool(info.use_bit_vector) == (leg != "explicit")
        assert info.list_max == self.list_max or leg == "explicit"
        assert (info.num_samples + 63) // 64 == self.wpc and info.ref_length == SAT_REF_LEN
        self.names, self.recs = vt.read_vcf(vcf)
        assert self.names == sorted(self.names) and len(self.recs) == self.rows
        assert self.vs.sample_name(1) == self.names[0] and self.vs.sample_name(n) == self.names[-1]
        self.ids_of = {nm: i + 1 for i, nm in enumerate(self.names)}
        if leg in ("text", "explicit"):
            self.orc = vt.TextOracle(vcf)
            assert len(self.orc.rows) == self.rows                 # the text leg leaves out no row
        else:
            plain = os.path.join(tmp, "plain.bin")
            self.vs.export_plain(plain)
            self.orc = _Memo(Oracle(plain))
        self.edges = vt.gap_midpoints(self.recs, SAT_REF_LEN)
        rng = np.random.default_rng(n)
        starts = np.sort(rng.integers(0, self.rows, size=70))
        picks = [(self.edges[i], self.edges[min(self.rows, i + int(rng.integers(1, 4)))]) for i in starts]
        self.whole = (1, SAT_REF_LEN + 1)
        srt = sorted(picks + [self.whole, (self.edges[3], self.edges[3])])
        self.batch = {"sorted": srt, "shuffled": [srt[i] for i in rng.permutation(len(srt))]}
        sub = {1, 63, 64, (self.wpc - 1) * 64, n} | {int(i) for i in rng.choice(np.arange(1, n + 1), size=40, replace=False)}
        self.subset = sorted(i for i in sub if 1 <= i <= n)      # (63 samples: no id 64, and id 0 is "ref")
        self.subset_names = {self.vs.sample_name(i) for i in self.subset}
        self._cache = {}
        self._preconditions()

    def _preconditions(self):
        """From the VCF text: what the cohort must hold for its cell to exercise the case it is there for."""
        n = self.n
        car = np.array([[g not in ("0|0", "0/0") for g in r[3]] for r in self.recs])
        self.carriers = car.sum(axis=1)
        if self.leg == "explicit":    # (no extreme rows: the head is sparse, the tail dense, record 144 is carried by everybody)
            assert self.carriers[:100].max() <= max(1, n // 50) and self.carriers[144] == n
            assert (self.carriers[100:] >= (0.7 * n if n <= 2015 else 1500)).all()
            return
        assert (self.carriers == n).sum() >= 2, "fewer than two rows carried by every sample"
        for k, call in ((1, "1/1"), (2, "1|1"), (3, "0|1"), (4, "1/0")):
            assert len(self.recs[k][2]) == 1 and set(self.recs[k][3]) == {call}, k
        assert self.carriers[5] == n - 1 and not car[5, 0] and self.carriers[6] == n - 1 and not car[6, n - 1]
        dense = self.carriers > self.list_max
        if n == 4159:
            assert (dense & car[:, :4095].all(axis=1) & (car[:, 4095:].sum(axis=1) >= 60)).any(), "no row whose second round starts at 4095"
        if n == 8255:    # ids 4096 .. 8191 are the second chunk: full, behind a first chunk whose carriers are no multiple of 8
            assert (dense & car[:, 4095:8191].all(axis=1) & (car[:, :4095].sum(axis=1) % 8 != 0)).any(), "no chunk of 513 staged words"
        if n == 63 and self.list_max == 0:
            assert (self.carriers == 63).any() and dense.all()
        if n <= 64 and self.list_max == 640:
            assert not dense.any()                                  # 63 of 63 carriers as a LIST

    def close(self):
        self.vs.close()

    def _cached(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def want(self, kind):
        """[(n, early_out, text)] of the batch's regions."""
        def make():
            out = [self.orc.get_var_in_ref(x, y) for x, y in self.batch[kind]]
            assert all(n >= 0 for n, _e, _t in out)
            assert out[self.batch[kind].index(self.whole)][0] >= self.rows    # (two-ALT records report two rows)
            return out
        return self._cached(("want", kind), make)

    def valid(self, kind):
        return np.arange(len(self.batch[kind]))

    def mparsed(self, kind):
        return self._cached(("m", kind), lambda: MatrixParsed([t for _n, _e, t in self.want(kind)]))

    def bparsed(self, kind):
        return self._cached(("b", kind), lambda: BurdenParsed([t for _n, _e, t in self.want(kind)]))

    def gparsed(self, kind):
        by_region = self._cached("g", lambda: {r: parse_region(t, self.ids_of) for r, (_n, _e, t) in zip(self.batch["sorted"], self.want("sorted"))})
        return [by_region[r] for r in self.batch[kind]]

    def table_rows(self, got, kind, records):
        """The table rows of `records` (indexes of VCF records; the text leg: record k is row k of the whole reference)."""
        q = self.batch[kind].index(self.whole)
        assert int(got["row_count"][q]) == self.rows and self.leg == "text"
        return int(got["row_begin"][q]) + np.asarray(records, np.int64)


@pytest.fixture(scope="module", params=CELLS, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def cohort(request, tmp_path_factory):
    n, list_max, leg = request.param
    c = _Cohort(n, list_max, leg, tmp_path_factory.mktemp(f"sat{n}"))
    yield c
    c.close()


def test_allele_counts(cohort):
    c = cohort
    for kind in ("sorted", "shuffled"):
        regions, want = c.batch[kind], c.want(kind)
        assert _check_texts(c.vs, regions, want) == len(regions)
        assert _check_texts(c.vs, regions, want, c.subset, c.subset_names) == len(regions)
    if c.leg == "text":     # the extreme rows, from the answer checked above
        res = c.vs.allele_counts(c.batch["sorted"])
        got = res.allele_counts()
        res.close()
        a, n = c.table_rows(got, "sorted", range(7)), c.n
        cnt = np.stack([got["counts"][f][a].astype(np.int64) for f in FIELDS], axis=1)
        assert cnt[1:5].tolist() == [[n, 2 * n, n, 0], [n, 2 * n, n, n], [n, n, 0, n], [n, n, 0, 0]]
        assert cnt[0, 0] == n and cnt[5, 0] == cnt[6, 0] == n - 1
        assert ((got["counts"]["carriers"] == n).sum() >= 2)


def test_group_counts(cohort):
    """One group of everybody (8 copies per row, summed packed), a partition into 64 groups, 3 groups that leave a third out."""
    c, n = cohort, cohort.n
    rng = np.random.default_rng(7 * n)
    everybody = np.zeros(n + 1, np.int64)
    everybody[0] = -1
    lab64 = _partition(rng, n, 64)
    lab64[n] = 63                        # the last bit of the last row word
    lab64[60:min(70, n + 1)] = 7         # across the first word boundary
    lab3 = _partition(rng, n, 3, unlisted=1 / 3)
    for kind in ("sorted", "shuffled"):
        regions, parsed = c.batch[kind], c.gparsed(kind)
        for label, g in ((everybody, 1), (lab64, 64), (lab3, 3)):
            got = _check_parsed(c.vs, regions, parsed, label, g)
            assert list(got["group_sizes"]) == [len(m) for m in _members(label, g)]
        if c.leg == "text" and kind == "sorted":
            got = _check_parsed(c.vs, regions, parsed, everybody, 1)
            a = c.table_rows(got, kind, [1, 2])
            assert [tuple(int(got["counts"][f][i, 0]) for f in FIELDS) for i in a] == [(n, 2 * n, n, 0), (n, 2 * n, n, n)]


def test_assoc_scan(cohort):
    """Integer traits at K = 1, 3 and 8: DOT exact, CHI2 within 8 * 2^-53 relative (test_gpu_assoc_scan._check_int: kernel and
    reference round the same operations in the same order, every input exact) and exactly 0 on the rows without variance."""
    c = cohort
    rng = np.random.default_rng(11 * c.n)
    regions, parsed, valid = c.batch["sorted"], c.mparsed("sorted"), c.valid("sorted")
    for k in (1, 3, 8):
        _check_int(c.vs, regions, parsed, valid, None, _int_traits(rng, c.n, k), rng)
    _check_int(c.vs, regions, parsed, valid, c.subset, _int_traits(rng, len(c.subset), 3), rng)
    _check_int(c.vs, c.batch["shuffled"], c.mparsed("shuffled"), c.valid("shuffled"), None, _int_traits(rng, c.n, 3), rng)
    if c.leg == "text":
        res = c.vs.assoc_scan(regions, _int_traits(rng, c.n, 3), None, "chi2")
        got = res.assoc_scan()
        res.close()
        flat = c.table_rows(got, "sorted", [1, 2, 3, 4])             # everybody 1/1, 1|1, 0|1, 1/0: n Sxx - Sx^2 = 0
        assert not got["scores"][flat].any() and got["scores"][c.table_rows(got, "sorted", [5, 6])].any(axis=1).all()


def test_sample_scores(cohort):
    """Integer weights at K = 1 and 8, whole cohort and subset: sums, shift and scores equal sample_scores_ref; all-ones weights are
    the burden's alt_alleles summed over the regions."""
    c = cohort
    rng = np.random.default_rng(13 * c.n)
    regions, parsed = c.batch["sorted"], c.mparsed("sorted")
    for samples in (None, c.subset):
        for k in (1, 8):
            _check_scores(c.vs, regions, parsed, samples, _int_weights(rng, parsed.n_rows, k), rng)
    sh = c.mparsed("shuffled")
    _check_scores(c.vs, c.batch["shuffled"], sh, None, _int_weights(rng, sh.n_rows, 1), rng)
    for samples in (None, c.subset):
        got = _check_scores(c.vs, regions, parsed, samples, np.ones((parsed.n_rows, 1), np.float32), rng)
        b = c.vs.sample_burden(regions, samples)
        cells = b.sample_burden()["cells"]
        b.close()
        assert np.array_equal(got["scores"][:, 0], cells["alt_alleles"].astype(np.int64).sum(axis=0).astype(np.float64)) and got["scores"].all()


def test_sample_burden(cohort):
    """Whole cohort and subset; the window max_ac = 2 n - 1 drops exactly the rows everybody is hom-alt on, min_ac = 2 n keeps only
    them (the ends of the burden's allele-count window, reachable only when a row is carried twice by everyone)."""
    c, n = cohort, cohort.n
    for kind in ("sorted", "shuffled"):
        regions, parsed, valid = c.batch[kind], c.bparsed(kind), c.valid(kind)
        full = _check_burden(c.vs, regions, parsed, valid, None, texts=n <= 64)
        _check_burden(c.vs, regions, parsed, valid, c.subset, texts=True)
        if kind == "shuffled":
            continue
        below = _check_burden(c.vs, regions, parsed, valid, None, 0, 2 * n - 1)
        only = _check_burden(c.vs, regions, parsed, valid, None, 2 * n)
        assert np.array_equal(below + only, full)
        if c.leg == "explicit":      # (no row everybody is hom-alt on)
            assert not only.any()
            continue
        q = regions.index(c.whole)
        assert (only[q] == [2, 4, 2, 1]).all(), "the whole reference: the all-1/1 and the all-1|1 row, for every sample"
        m = len(c.subset)
        sub_only = _check_burden(c.vs, regions, parsed, valid, c.subset, 2 * m)
        assert (sub_only[q, :, 0] >= 2).all()


def test_genotype_matrix(cohort):
    """Every cell, the last column, the pitch; a subset's columns."""
    c, n = cohort, cohort.n
    for kind in ("sorted", "shuffled"):
        regions, parsed, valid = c.batch[kind], c.mparsed(kind), c.valid(kind)
        got = _check_matrix(c.vs, regions, parsed, valid, None, texts=n <= 64)
        assert got["cells"][:, -1].any(), "the last column is set nowhere"
        assert got["row_pitch"] == (n + 15) // 16 * 16 and got["cells"].shape[1] == n
        _check_matrix(c.vs, regions, parsed, valid, c.subset, texts=kind == "sorted")
    if c.leg == "text":
        a = c.table_rows(got, "shuffled", range(7))
        cells = got["cells"][a]
        assert [set(np.unique(cells[k]).tolist()) for k in (1, 2, 3, 4)] == [{0x0E}, {0x0F}, {0x0D}, {0x0A}]   # 1/1, 1|1, 0|1, 1/0
        assert cells[5, 0] == 0 and cells[5, 1:].all() and cells[6, -1] == 0 and cells[6, :-1].all() and cells[0].all()


def test_ld_band(cohort):
    """Windows 16 and 100: DOT exact, R2 within 2**-22 relative and exactly 0 wherever a row has no variance (test_gpu_ld_band's
    _r2_close); rows carried by all but one sample leave n Sxx - Sx^2 a small integer behind a large cancellation."""
    c = cohort
    regions, parsed, valid = c.batch["sorted"], c.mparsed("sorted"), c.valid("sorted")
    for window in (16, 100):
        got = _check_ld(c.vs, regions, parsed, valid, None, window, text_every=9 if c.n <= 64 else 0)
    _check_ld(c.vs, c.batch["shuffled"], c.mparsed("shuffled"), c.valid("shuffled"), c.subset, 16, text_every=0)
    if c.leg == "text":       # (got: the r2 band at window 100)
        a = c.table_rows(got, "sorted", range(8))
        band = got["band"]
        assert got["stat"] == "r2" and not band[a[1:5]].any() and not band[a[0], :4].any()
        assert band[a[5], :2].any()                            # rows 5, 6, 7: carried by all but one, all but one, a share of the samples


def _table_matrix(got, parsed, want_m):
    """The expected cells of every table row, from the expected matrix over the rows the regions report."""
    dropped = (got["rows"]["count_flags"] >> 31) != 0
    out = np.zeros((got["rows"].shape[0], want_m.shape[1]), np.uint8)
    seen = np.zeros(out.shape[0], bool)
    for q in range(parsed.n_regions):
        a = np.arange(int(got["row_begin"][q]), int(got["row_begin"][q]) + int(got["row_count"][q]))
        a = a[~dropped[a]]
        r0 = int(parsed.row_begin[q])
        assert a.shape[0] == int(parsed.row_count[q]), q
        out[a] = want_m[r0:r0 + a.shape[0]]
        seen[a] = True
    assert seen[~dropped].all(), "a table row that no region reports"
    return out


def _check_gram(c, regions, parsed, samples, stats):
    """gram, col_weighted, C, H (and grm, bit for bit) against sample_gram_ref of the matrix the EXPECTED texts give -- not of the
    engine's own genotype matrix."""
    _ids, names = _columns(c.vs, samples)
    want_m = matrix(parsed, names)
    got = None
    for stat in stats:
        res = c.vs.sample_gram(regions, samples, stat=stat)
        got = res.sample_gram()
        res.close()
        wg, ws, wc, wh = _gram_want(_table_matrix(got, parsed, want_m))
        assert np.array_equal(got["gram"], wg) and np.array_equal(got["col_weighted"], ws) and (got["C"], got["H"]) == (wc, wh), stat
        if stat == "grm":
            want, _num = sample_gram_ref.grm(wg, ws, wc, wh)
            assert got["grm"].dtype == np.float64 and np.array_equal(got["grm"], want), float(np.abs(got["grm"] - want).max())
    return got


def test_sample_gram(cohort):
    """Dosage 2 in every cell of the i8 MFMA products, H = sum ac (2 n - ac) with ac = 2 n, the GRM's 128-bit numerators."""
    c, n = cohort, cohort.n
    regions, parsed = c.batch["sorted"], c.mparsed("sorted")
    if n <= 64:
        _check_gram(c, regions, parsed, None, ("dot", "grm"))
    elif n < 8255:
        _check_gram(c, regions, parsed, None, ("dot",))
    rng = np.random.default_rng(17 * n)
    sub = sorted(set(c.subset) | {int(i) for i in rng.choice(np.arange(1, n + 1), size=min(260, n // 2), replace=False)})
    got = _check_gram(c, regions, parsed, sub, ("dot", "grm"))
    assert got["H"] > 0 and got["grm"].any()
    _check_gram(c, c.batch["shuffled"], c.mparsed("shuffled"), c.subset, ("grm",))
    if c.leg == "explicit":
        return
    # only the rows everybody is 1/1 and 1|1 on: no variance anywhere, H = 0 and every GRM cell 0.0
    e = c.edges
    flat = [(e[1], e[2]), (e[2], e[3]), (e[1], e[3])]
    fp = MatrixParsed([c.orc.get_var_in_ref(x, y)[2] for x, y in flat])
    assert fp.n_rows == 4
    for samples in ((None, sub) if n < 8255 else (sub,)):
        got = _check_gram(c, flat, fp, samples, ("grm",))
        m = n if samples is None else len(samples)
        assert got["H"] == 0 and not got["grm"].any() and not np.signbit(got["grm"]).any()
        assert got["gram"].min() == got["gram"].max() == 4 * got["rows"].shape[0] and got["C"] == got["rows"].shape[0] * (2 * m) ** 2


# ------------------------------------------------------------------------------------ the group-count field limit
@pytest.fixture(scope="module")
def max_cohort(tmp_path_factory):
    """32,767 samples -- 32,768 sample ids, the largest label table k_group_counts admits -- and 12 rows."""
    c = _Cohort(32767, None, "text", tmp_path_factory.mktemp("sat32767"), rows=12)
    e = c.edges
    srt = sorted([c.whole, (e[3], e[3])] + [(e[i], e[i + 2]) for i in (0, 1, 2, 5, 8, 10)])
    c.batch = {"sorted": srt, "shuffled": srt[::-1]}
    yield c
    c.close()


def test_group_count_fields_at_the_admitted_maximum(max_cohort):
    """alt_alleles = 65,534 = 2^16 - 2 in one group, summed packed over the 8 copies G = 1 keeps per row; two groups with everybody
    in the first (4 copies); a 64-way partition (none).  Eight full rounds of the dense loop."""
    c, n = max_cohort, 32767
    assert c.wpc == 512 and c.vs.info().use_bit_vector
    regions, parsed = c.batch["sorted"], c.gparsed("sorted")
    everybody = np.zeros(n + 1, np.int64)
    everybody[0] = -1
    lab64 = _partition(np.random.default_rng(5), n, 64)
    lab64[n] = 63
    for label, g in ((everybody, 1), (everybody, 2), (lab64, 64)):
        got = _check_parsed(c.vs, regions, parsed, label, g)
        if g <= 2:
            a = c.table_rows(got, "sorted", [1, 2])
            assert [tuple(int(got["counts"][f][i, 0]) for f in FIELDS) for i in a] == [(n, 2 * n, n, 0), (n, 2 * n, n, n)]
            assert 2 * n == 65534 and not any(got["counts"][f][:, 1:].any() for f in FIELDS)
    _check_parsed(c.vs, c.batch["shuffled"], c.gparsed("shuffled"), everybody, 1)


def test_other_columns_at_the_admitted_maximum(max_cohort):
    """The same handle: allele_counts, sample_scores (K = 1, all-ones weights) and genotype_matrix over rows of 512 words."""
    c = max_cohort
    regions, want, parsed = c.batch["sorted"], c.want("sorted"), c.mparsed("sorted")
    assert _check_texts(c.vs, regions, want) == len(regions)
    rng = np.random.default_rng(3)
    got = _check_scores(c.vs, regions, parsed, None, np.ones((parsed.n_rows, 1), np.float32), rng)
    assert got["scores"].all()
    m = _check_matrix(c.vs, regions, parsed, c.valid("sorted"), None)
    assert m["cells"][:, -1].any() and m["row_pitch"] == 32768


def test_group_counts_refuses_one_sample_more(tmp_path):
    """32,768 samples are 32,769 sample ids: the label table does not fit, the query says so; allele_counts has no such limit."""
    fasta, vcf = write_saturated_cohort(str(tmp_path), 32768, 4400 + 32768, rows=3, two_alt=False, extremes=True)
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    assert vs.info().num_samples == 32769
    tx = vt.TextOracle(vcf)
    e = tx.midpoints(SAT_REF_LEN)
    regions = [(1, SAT_REF_LEN + 1), (e[1], e[3]), (e[0], e[0])]
    for groups in ([list(range(1, 32769))], [[1, 2], [32768]]):
        with pytest.raises(VariantStoreError) as err:
            vs.group_counts(regions, groups)
        assert err.value.code == VS_ERR_UNSUPPORTED and "at most 32768 sample ids" in str(err.value), str(err.value)
    assert _check_texts(vs, regions, [tx.get_var_in_ref(x, y) for x, y in regions]) == len(regions)
    vs.close()
