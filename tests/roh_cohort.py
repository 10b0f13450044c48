"""Cohorts for the ROH tests, written as FASTA + VCF text of well-separated SNPs, so that the table a batch reports is the VCF's
records in order and the expected dosages are the writer's own arrays (the CPU test checks the conditions the GPU test relies on
from them; the GPU test compares against the engine's own genotype matrix and asserts the same conditions again).

write_roh_cohort: every sample's column is a chain that alternates between an autozygous state (homozygous for the allele a
hidden haplotype carries) and an outbred state (a het with probability het_p); rows [single_from, single_to) are singletons
(ac == 1: no site under min_ac = 2 -- a stretch longer than two row blocks, so that some block of 64 rows holds no site), and two
stretches of the reference carry no record (gaps of gap_bp bases for the gap rule); from row regular_from on the rows are 10 bases
apart and a quarter of them are singletons too, so that two segments of one column can span the same bases with different numbers
of sites (the tie of longest_bp).

write_planted_cohort: a background in which no sample stays homozygous for min_sites sites, and planted stretches of known
coordinates."""
import os

import numpy as np

BASES = "ACGT"


def _write(dirpath, stem, ref, names, positions, calls):
    fasta, vcf = os.path.join(dirpath, stem + ".fa"), os.path.join(dirpath, stem + ".vcf")
    with open(fasta, "w") as f:
        f.write(">c1 roh\n" + "".join(ref[i:i + 60] + "\n" for i in range(0, len(ref), 60)))
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.1\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n")
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n")
        text = np.asarray(["0|0", "1|0", "0|1", "1|1"])
        for r, p in enumerate(positions):
            r0 = ref[p - 1]
            f.write(f"c1\t{p}\t.\t{r0}\t{BASES[(BASES.index(r0) + 1) % 4]}\t99\t.\t.\tGT\t" + "\t".join(text[calls[r]].tolist()) + "\n")
    return fasta, vcf


def write_roh_cohort(dirpath, seed, n_samples=520, n_rows=420, single_from=150, single_to=300, regular_from=300, gap_bp=400, het_p=0.45, stay_p=0.93):
    """Returns (fasta, vcf, names, positions, dosage[rows, samples]).  Names ascend with the column, as in every cohort here."""
    rng = np.random.default_rng(seed)
    step = rng.integers(8, 16, size=n_rows)
    step[regular_from:] = 10                            # evenly spaced rows: segments of equal length in bases occur
    step[[n_rows // 6, n_rows - 60]] = gap_bp           # two stretches without a record
    positions = (40 + np.cumsum(step)).astype(np.int64)
    ref_len = int(positions[-1]) + 200
    ref = "".join(BASES[i] for i in rng.integers(0, 4, size=ref_len))
    names = [f"S{k:04d}" for k in range(n_samples)]
    af = rng.uniform(0.15, 0.6, size=n_rows)
    calls = np.zeros((n_rows, n_samples), np.int64)     # 0: 0|0, 1: 1|0, 2: 0|1, 3: 1|1
    auto = rng.random(n_samples) < 0.5
    for r in range(n_rows):
        flip = rng.random(n_samples) > stay_p
        auto = np.where(flip, ~auto, auto)
        hom_alt = rng.random(n_samples) < af[r]
        het = (~auto) & (rng.random(n_samples) < het_p)
        calls[r] = np.where(het, rng.integers(1, 3, size=n_samples), np.where(hom_alt, 3, 0))
    sprinkled = [r for r in range(regular_from, n_rows) if rng.random() < 0.25]   # ... with different numbers of sites under min_ac = 2
    for r in list(range(single_from, single_to)) + sprinkled:   # singletons: one het carrier
        calls[r] = 0
        calls[r, int(rng.integers(0, n_samples))] = 1
    dosage = np.asarray([0, 1, 1, 2])[calls]
    assert ((dosage.sum(axis=1) > 0) & (dosage.sum(axis=1) < 2 * n_samples)).all()
    fasta, vcf = _write(dirpath, f"roh{seed}", ref, names, positions.tolist(), calls)
    return fasta, vcf, names, positions, dosage


def write_planted_cohort(dirpath, seed=31, n_samples=40, n_rows=300, min_sites=20):
    """Returns (fasta, vcf, names, positions, planted): planted = [(sample column, first row, last row)], the only stretches of
    min_sites or more consecutive homozygous calls in the cohort.  Background: sample s is het at every row r with (r + 3 s) % 7 ==
    0 -- at most six homozygous rows in a row; a planted stretch is made homozygous and bounded by a het on either side."""
    rng = np.random.default_rng(seed)
    positions = (100 + np.cumsum(rng.integers(30, 90, size=n_rows))).astype(np.int64)
    ref = "".join(BASES[i] for i in rng.integers(0, 4, size=int(positions[-1]) + 200))
    names = [f"P{k:02d}" for k in range(n_samples)]
    calls = np.where(rng.random((n_rows, n_samples)) < 0.3, 3, 0)
    r_idx, s_idx = np.meshgrid(np.arange(n_rows), np.arange(n_samples), indexing="ij")
    calls[(r_idx + 3 * s_idx) % 7 == 0] = 1
    planted = [(3, 10, 45), (3, 120, 139), (17, 0, 30), (17, 200, 299), (28, 60, 150), (39, 250, 280), (0, 150, 169)]
    for s, a, b in planted:
        assert b - a + 1 >= min_sites
        calls[a:b + 1, s] = np.where(rng.random(b - a + 1) < 0.3, 3, 0)
        if a > 0:
            calls[a - 1, s] = 2
        if b + 1 < n_rows:
            calls[b + 1, s] = 1
    fasta, vcf = _write(dirpath, "planted", ref, names, positions.tolist(), calls)
    return fasta, vcf, names, positions, planted


def dosages_of_vcf(vcf):
    """(positions, names, dosage[rows, samples]) read back from the VCF TEXT of single-ALT records: the count of '1' alleles per call."""
    pos, rows, names = [], [], None
    for line in open(vcf):
        if line.startswith("##"):
            continue
        f = line.rstrip("\n").split("\t")
        if line.startswith("#"):
            names = f[9:]
            continue
        assert "," not in f[4]
        pos.append(int(f[1]))
        rows.append([g.replace("|", "/").split("/").count("1") for g in f[9:]])
    return np.asarray(pos, np.int64), names, np.asarray(rows, np.int64)


# ------------------------------------------------------------- the cohort, regions and parameter sets of tests/test_gpu_roh.py
COHORT_KW = dict(seed=7, n_samples=520, n_rows=420)
REGION_ROWS = [(0, 419), (100, 349), (350, 419), (160, 299), (0, 62), (290, 419)]   # first and last table row of a region
PARAM_SETS = [dict(min_sites=1),
              dict(min_sites=5, max_het=1, max_gap=200, min_ac=2),
              dict(min_sites=3, max_het=3, min_bp=60, min_ac=2),
              dict(min_sites=1, min_bp=25, min_ac=100, max_ac=400),
              dict(min_sites=50)]


def regions_of_rows(positions, region_rows=REGION_ROWS):
    """Regions that report the records first .. last (the records are 8 bases or more apart)."""
    return [(int(positions[a]) - 2, int(positions[b]) + 2) for a, b in region_rows]


def tie_resolved_to_the_earlier(out):
    """Some cell whose largest span is reached by two segments with different numbers of sites, and whose longest_sites is the
    earlier one's."""
    seg, sb = out["segments"], out["seg_begin"]
    summary = out["summary"].reshape(-1)
    for cell in np.nonzero(summary["n_segments"] >= 2)[0]:
        mine = seg[int(sb[cell]):int(sb[cell + 1])]
        bp = np.maximum(mine["pos_last"].astype(np.int64) - mine["pos_first"], 0) + 1
        top = np.nonzero(bp == bp.max())[0]
        if top.size >= 2 and np.unique(mine["n_sites"][top]).size >= 2 and int(mine["n_sites"][top[0]]) != int(mine["n_sites"][top[1]]):
            assert int(summary["longest_sites"][cell]) == int(mine["n_sites"][top[0]]) and int(summary["longest_bp"][cell]) == int(bp.max())
            return True
    return False


def conditions_met(stats, outs):
    """The conditions that keep a comparison from being vacuous, asserted on EXPECTED values: `stats` roh_ref's counters over all
    parameter sets, `outs` [(params, expected answer)]."""
    assert stats["closed_het"] > 0 and stats["closed_gap"] > 0 and stats["closed_end"] > 0, stats
    assert stats["rejected_min_sites"] > 0 and stats["rejected_min_bp"] > 0, stats
    assert any((o["segments"]["n_het"] > 0).any() for _p, o in outs), "no segment absorbed a het"
    assert any((o["summary"]["n_segments"] >= 3).any() for _p, o in outs), "no column has three segments"
    assert any(tie_resolved_to_the_earlier(o) for _p, o in outs), "no tie of longest_bp between segments of different n_sites"
    assert any(((o["summary"]["n_het"] > 0) & (o["summary"]["n_segments"] == 0)).any() for _p, o in outs), "no cell with hets and no segment"
    for _p, o in outs:
        s = o["summary"]
        if s.shape[1] >= 513 and (s["n_segments"] > 0).any():
            rows = [s[:, c].tobytes() for c in (3, 70, 300, 512)]   # two waves of tile 0, tile 1, tile 2
            assert len(set(rows)) == 4, "columns of different waves and tiles have the same summaries"
