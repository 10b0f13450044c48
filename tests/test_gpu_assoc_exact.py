"""assoc_scan's CHI2 on the GPU against the EXACT score statistic (assoc_exact_ref: Python integers from the oracle's type-6 text and
the float32 trait values, nothing of the engine in it), on traits that have an offset -- the one float-valued answer of the engine
that is summed and cancelled in floating point, and that the other files compare with a restatement of its own formula only.

Cohorts: synthetic ones of 300 and 2,504 samples (listed and dense rows), a sparse explicit-id cohort (the flat pass alone), and the
saturated cohort of 4,159 samples, whose dense pass takes a second round of row words and whose rows are carried by everybody, by
everybody but one sample and by all-heterozygous callers (Sx Sy at its largest).  Traits: assoc_exact_ref.LADDER, from zero mean to
a mean 10^6 standard deviations away, in tables of K = 8, 3, 2 and 1 (every Kp instantiation).  Forms: the whole cohort and a subset
that straddles ids 64 and 128 and holds the last sample, the phenotype table in LDS and in global memory, regions sorted and shuffled.

Held on EVERY row of every table:
  * assoc_scan's chi2 within the derived bound of the exact value, the bound itself at most 8 n 2^-53 max(chi2, 1)
  * assoc_matrix's chi2 of the same call within 8 * 2^-53 relative of it, and the two queries within the sum of both bounds
  * the LDS and the global form, and the same call twice: the same bytes
  * the 0/1 label: the Cochran-Armitage trend statistic, in Fraction from group_counts of cases and controls on the same regions
  * a trait and the same trait 1,000,000 higher: no chi2 moves by more than the two bounds together
  * the constant 0.1f: exactly 0.0 in every cell
  * DOT cells, trait_sum and trait_sumsq under test_gpu_assoc_scan._check_real's bounds: they stay the raw sums
and one CLI case: `variantstore assoc --chi2` with the 1e6 +- 1 trait prints the values the accessor returns."""
import os
import subprocess

import numpy as np
import pytest

import assoc_exact_ref as ex
import assoc_matrix_ref
import assoc_scan_ref as ref
from helpers import random_regions, write_random_cohort
from test_gpu_assoc_scan import _check_real, _check_rows, _subset
from test_gpu_genotype_matrix import _columns, _oracle, _parse, _reported
from variantstore_amd import VariantStore

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = ex.U
TABLES = (("normal", "170+-7", "1e4+-1", "1e6+-100", "1e6+-1", "-3e7+-50", "1e-3+-1e-6", "label"),   # Kp = 8
          ("int+1e6", "int", "0.1f"),                                                                   # Kp = 4
          ("near_constant", "correlated"),                                                              # Kp = 2
          ("1e6+-1",))                                                                                  # Kp = 1
assert {t for tab in TABLES for t in tab} == set(ex.LADDER)


class _Synthetic:
    """A synthetic cohort of n samples with about 150 table rows, listed rows beside dense ones where the cohort has both."""

    def __init__(self, n, tmp):
        self.vs = VariantStore.synthetic(device=0, ref_length=200_000, num_variants=3_000, num_samples=n, seed=40 + n, first_pos=500,
                                         frac_ins=0.05, frac_del=0.05, frac_multi=0.02, max_indel=4, af_exponent=1.0 if n > 1000 else 2.0)
        self.orc = _oracle(self.vs, str(tmp))
        rng = np.random.default_rng(n)
        starts = np.sort(rng.integers(600, 195_000, size=12))
        srt = [(int(s), int(s) + int(rng.integers(500, 1_100))) for s in starts]
        self.batch = {"sorted": srt, "shuffled": [srt[i] for i in rng.permutation(len(srt))]}
        self._parsed = {}

    def parsed(self, kind):
        if kind not in self._parsed:
            self._parsed[kind] = _parse(self.orc, self.batch[kind])
        return self._parsed[kind]

    def close(self):
        self.vs.close()


class _Explicit(_Synthetic):
    """130 samples, a carrier in 250: the cohort opens with explicit sample ids, every row is a short list (the flat pass)."""

    def __init__(self, tmp):
        fasta, vcf, _names = write_random_cohort(str(tmp), 703, n_rows=300, ref_len=5000, n_samples=130, carrier_p=0.004)
        self.vs = VariantStore.from_vcf(fasta, vcf, device=0)
        assert not self.vs.info().use_bit_vector
        self.orc = _oracle(self.vs, str(tmp))
        rng = np.random.default_rng(703)
        srt = sorted(r for r in random_regions(rng, 5000, 30, max_len=400) if r[0] >= 1)
        self.batch = {"sorted": srt, "shuffled": [srt[i] for i in rng.permutation(len(srt))]}
        self._parsed = {}


class _Saturated(_Synthetic):
    """test_gpu_saturated_columns' cohort of 4,159 samples (65 row words: two rounds of the dense pass), against the VCF text."""

    def __init__(self, tmp):
        from test_gpu_saturated_columns import _Cohort
        self.c = _Cohort(4159, None, "text", tmp)
        self.vs, self.batch = self.c.vs, self.c.batch

    def parsed(self, kind):
        return self.c.mparsed(kind), self.c.valid(kind)


@pytest.fixture(scope="module", params=["syn300", "syn2504", "explicit", "saturated"])
def cohort(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp(request.param)
    c = {"syn300": lambda: _Synthetic(300, tmp), "syn2504": lambda: _Synthetic(2504, tmp), "explicit": lambda: _Explicit(tmp),
         "saturated": lambda: _Saturated(tmp)}[request.param]()
    c.name = request.param
    yield c
    c.close()


def _dense(parsed, names):
    """int64 (n_rows, n): the dosage matrix of Parsed's rows over the columns, from the type-6 text (genotype_matrix_ref)."""
    row, col, d, _val = ref.dosages(parsed, names)
    out = np.zeros((parsed.n_rows, len(names)), np.int64)
    out[row, col] = d
    return out


def _scan(vs, regions, y, samples, stat, kib=0):
    vs.set_option("assoc_lds_max_kib", kib)
    try:
        res = vs.assoc_scan(regions, y, samples, stat)
        got = res.assoc_scan()
        res.close()
    finally:
        vs.set_option("assoc_lds_max_kib", 0)
    return got


def _trend(vs, regions, valid, ids, label):
    """float64 per reported row: the Cochran-Armitage trend statistic in Fraction from group_counts of cases and controls."""
    cases, ctrls = [i for i, l in zip(ids, label) if l == 1], [i for i, l in zip(ids, label) if l == 0]
    res = vs.group_counts(regions, [cases, ctrls])
    got = res.group_counts()
    res.close()
    mine, _n = _reported(got, valid)
    out = np.zeros(mine.shape[0])
    for j, a in enumerate(mine):
        c = got["counts"][a]
        t = ex.trend(len(cases), len(ctrls), int(c["alt_alleles"][0]), int(c["hom_alt"][0]), int(c["carriers"][0]),
                     int(c["alt_alleles"][1]), int(c["hom_alt"][1]), int(c["carriers"][1]))
        out[j] = float(t) if t is not None else 0.0
    return mine, out


@pytest.mark.parametrize("kind", ["sorted", "shuffled"])
@pytest.mark.parametrize("who", ["whole", "subset"])
def test_chi2_against_the_exact_statistic(cohort, who, kind):
    vs, regions = cohort.vs, cohort.batch[kind]
    parsed, valid = cohort.parsed(kind)
    ns = vs.info().num_samples - 1
    rng = np.random.default_rng(ns + (who == "subset") + 2 * (kind == "sorted"))
    samples = None if who == "whole" else _subset(rng, ns)
    ids, names = _columns(vs, samples)
    n = len(ids)
    d = _dense(parsed, names)
    var = n * (d * d).sum(axis=1) - d.sum(axis=1) ** 2
    lad = ex.ladder(rng, n, d[int(np.argmax(var))])
    failures, seen_dense = [], False
    for tab in TABLES:
        y = np.ascontiguousarray(np.stack([lad[t] for t in tab], axis=1))
        assert np.array_equal(ref.pivots(y), [np.float64(y[ex.pivot(ex.scaled(y[:, k])[0]), k]) for k in range(len(tab))]), "a near-tie of the pivot"
        val, bound = ex.table(d, y)
        got = _scan(vs, regions, y, samples, "chi2")
        mine, rows, _names = _check_rows(vs, got, parsed, valid, samples, y)
        # the same bytes: twice, and the global form of the phenotype table
        assert got["scores"].tobytes() == _scan(vs, regions, y, samples, "chi2")["scores"].tobytes()
        assert got["scores"].tobytes() == _scan(vs, regions, y, samples, "chi2", kib=1)["scores"].tobytes()
        cnt = got["rows"]["count_flags"] & 0x7FFFFFFF
        seen_dense |= bool((cnt > vs.info().list_max).any())
        want, lim = val[rows], bound[rows]
        mres = vs.assoc_matrix(regions, y, samples, "chi2")
        mgot = mres.assoc_matrix()
        mres.close()
        mmine, _n = _reported(mgot, valid)
        assert mmine.shape == mine.shape and np.array_equal(mgot["shift"], assoc_matrix_ref.shifts(y))
        scan, mat = got["scores"][mine], mgot["scores"][mmine]
        err, merr = np.abs(scan - want), np.abs(mat - want)
        for k, t in enumerate(tab):
            unit = n * U * np.maximum(want[:, k], 1.0)
            print(f"{cohort.name} {who} {kind} n = {n} {t}: chi2 up to {want[:, k].max():.4g}; |scan - exact| <= {(err[:, k] / unit).max():.3g} n 2^-53 "
                  f"max(chi2, 1), bound <= {(lim[:, k] / unit).max():.3g}; |matrix - exact| <= {(merr[:, k] / np.maximum(U * want[:, k], 1e-300)).max():.3g} 2^-53 chi2; "
                  f"{int((err[:, k] > lim[:, k] + U * want[:, k]).sum())} of {want.shape[0]} rows beyond the bound")
            if not (np.all(np.isfinite(lim[:, k])) and np.all(lim[:, k] <= ex.cap(n, want[:, k]))):
                failures.append((t, "the bound passes the cap: no test case"))
            if not np.all(err[:, k] <= lim[:, k] + U * want[:, k]):
                failures.append((t, "scan beyond the bound", float((err[:, k] / unit).max())))
            if not np.all(merr[:, k] <= 8 * U * want[:, k]):
                failures.append((t, "matrix beyond 8 * 2^-53"))
            if not np.all(np.abs(scan[:, k] - mat[:, k]) <= lim[:, k] + 9 * U * want[:, k]):
                failures.append((t, "the two queries disagree"))
            if t == "0.1f" and (scan[:, k].any() or mat[:, k].any() or np.signbit(scan[:, k]).any()):
                failures.append((t, "a constant trait scores"))
            if t == "label":
                gmine, trend = _trend(vs, regions, valid, ids, y[:, k])
                assert gmine.shape == mine.shape
                assert np.array_equal(trend, want[:, k]), "the exact statistic of a 0/1 trait is the trend statistic"
                if not np.all(np.abs(scan[:, k] - trend) <= lim[:, k] + U * trend):
                    failures.append((t, "not the trend statistic"))
        for base, shifted, by in ex.SHIFTED:
            if base in tab and shifted in tab:
                a, b = tab.index(base), tab.index(shifted)
                assert np.array_equal(y[:, a] + np.float32(by), y[:, b]) and np.array_equal(want[:, a], want[:, b])
                if not np.all(np.abs(scan[:, a] - scan[:, b]) <= lim[:, a] + lim[:, b] + 2 * U * want[:, a]):
                    failures.append((shifted, "a shift moves chi2"))
        assert np.all(scan >= 0) and np.all(np.isfinite(scan)) and want.any()
        # DOT, trait_sum, trait_sumsq (the raw sums) and CHI2 once more, as test_gpu_assoc_scan holds real-valued traits
        try:
            _check_real(vs, regions, parsed, valid, samples, y, rng)
        except AssertionError as e:
            failures.append((tab, "_check_real", str(e)[:200]))
    if cohort.name in ("syn2504", "saturated") and who == "whole":
        assert seen_dense, "no dense row: the wave-per-row pass did not run"
    assert not failures, failures


def test_cli_prints_what_the_accessor_returns(tmp_path):
    exe = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
    fasta, vcf, names = write_random_cohort(str(tmp_path), 79, ref_len=6000, n_rows=300, n_samples=70)
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    subprocess.run([exe, "construct", "-r", fasta, "-v", vcf, "-p", prefix], check=True, capture_output=True)
    vs = VariantStore.open(prefix, device=0)
    rng = np.random.default_rng(5)
    regions = [(x, y) for x, y in sorted(random_regions(rng, 6000, 40)) if x >= 1]
    rfile, pfile, out = (os.path.join(tmp_path, f) for f in ("regions.txt", "pheno.txt", "out.txt"))
    with open(rfile, "w") as f:
        f.write("".join(f"{x}:{y}\n" for x, y in regions))
    who = [names[i] for i in rng.permutation(70)[:50]]
    y = (1e6 + rng.standard_normal(50)).astype(np.float32)
    with open(pfile, "w") as f:   # float32 values written so that they read back as they are
        f.write("#sample\theight\n" + "".join(f"{nm}\t{float(v)!r}\n" for nm, v in zip(who, y)))
    subprocess.run([exe, "assoc", "-p", prefix, "-r", "@" + rfile, "-P", pfile, "-o", out, "--chi2"], check=True, capture_output=True)
    with open(out) as f:
        parts = f.read().split("#region ")[1:]
    res = vs.assoc_scan(regions, y, who, "chi2", ["height"])
    got = res.assoc_scan()
    assert len(parts) == len(regions)
    printed = []
    for q, part in enumerate(parts):
        head, text = part.split("\n", 1)
        assert head == f"{q} {regions[q][0]}:{regions[q][1]}" and text == res.region_text(q), q
        printed += [float(line.rsplit("\t", 1)[1]) for line in text.split("\n")[1:] if line]
    mine, _n = _reported(got, range(len(regions)))
    assert np.array_equal(np.asarray(printed), got["scores"][mine, 0]) and got["scores"].any()
    # ... and they are the statistic: the text of the same regions through the oracle, the exact reference
    orc = _oracle(vs, str(tmp_path))
    parsed, valid = _parse(orc, regions)
    ids, cols = _columns(vs, who)
    ycol = np.zeros((len(ids), 1), np.float32)
    for nm, v in zip(who, y):
        ycol[cols.index(nm), 0] = v
    val, bound = ex.table(_dense(parsed, cols), ycol)
    vmine, _n = _reported(got, valid)
    rows = np.concatenate([np.arange(int(parsed.row_begin[q]), int(parsed.row_begin[q] + parsed.row_count[q])) for q in valid])
    assert np.all(np.abs(got["scores"][vmine] - val[rows]) <= bound[rows] + U * val[rows]) and np.all(bound <= ex.cap(len(ids), val))
    res.close()
    vs.close()
