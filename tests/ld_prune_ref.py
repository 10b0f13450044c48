"""The expected answer of an LD pruning query (vs_query_ld_prune), worked out from a genotype-matrix cell array (the uint8 cells of
genotype_matrix_ref.matrix or of the engine's own genotype_matrix()) in Python integers and numpy int64: no floating-point value
takes part in a verdict.  Also the writer of the "LD-block" VCF cohort the pruning tests share."""
import os

import numpy as np

from ld_band_ref import dosage

ONE = 1 << 20   # the threshold of r2 = 1
PRUNED, KEPT, INELIGIBLE, DROPPED = 0, 1, 2, 3
STATE_WORD = {PRUNED: "pruned", KEPT: "keep", INELIGIBLE: "skip"}


def variance(counts, n):
    """v = n Sxx - Sx^2 of a row from its count record (alt_alleles, hom_alt), a Python integer."""
    ac, hom = int(counts[0]), int(counts[1])
    return int(n) * (ac + 2 * hom) - ac * ac


def hit(sxy, counts_i, counts_j, n, T):
    """The pair is a hit exactly when v_i > 0, v_j > 0 and cov^2 2^20 > T v_i v_j, in Python integers; counts = (alt_alleles,
    hom_alt) of a row over the n columns, sxy the dot product of the two rows' dosages."""
    vi, vj = variance(counts_i, n), variance(counts_j, n)
    if vi <= 0 or vj <= 0:
        return False
    cov = int(n) * int(sxy) - int(counts_i[0]) * int(counts_j[0])
    return cov * cov * ONE > int(T) * vi * vj


def row_counts(cells):
    """(alt_alleles, hom_alt) per row, int64, from the cells."""
    d = dosage(cells)
    return d.sum(axis=1), (d == 2).sum(axis=1)


def _band_sides(cells, window, T):
    """For k = 0 .. window - 1: (k, m, cov^2 2^20, T v_i v_j, v_i > 0 and v_j > 0) of the pairs (i, i + 1 + k), i < m.  The sums in
    int64 (exact: |cov|, v <= 4 n^2 < 2^63 for every n the engine admits), the two sides in Python integers from n = 800 on."""
    d = dosage(cells)
    a, n = d.shape
    ac, hom = row_counts(cells)
    # |cov|, v <= 4 n^2: below n = 800 both sides of the comparison stay under 2^20 * 16 n^4 < 2^63 and int64 is exact as well
    wide = np.int64 if n < 800 else object
    v = (np.int64(n) * (ac + 2 * hom) - ac * ac).astype(wide)
    d8 = d.astype(np.int8)   # (the products of the dosages, summed in int64: the same integers from an eighth of the memory)
    for k in range(min(window, max(a - 1, 0))):
        m = a - 1 - k
        sxy = np.einsum("ij,ij->i", d8[:m], d8[1 + k:], dtype=np.int64)
        cov = (np.int64(n) * sxy - ac[:m] * ac[1 + k:]).astype(wide)
        vi, vj = v[:m], v[1 + k:]
        yield k, m, cov * cov * ONE, vi * vj * int(T), np.asarray(vi > 0, bool) & np.asarray(vj > 0, bool)


def hit_band(cells, window, T):
    """bool (rows, window): [i, k] = hit(i, i + 1 + k), False past the last row.  The sums in int64, the comparison in Python
    integers (object arrays): exact."""
    out = np.zeros((np.asarray(cells).shape[0], window), bool)
    for k, m, lhs, rhs, live in _band_sides(cells, window, T):
        out[:m, k] = np.asarray(lhs > rhs, bool) & live
    return out


def side_band(cells, window, T):
    """(lhs, rhs), object (rows, window): the two sides cov^2 2^20 and T v_i v_j of hit_band's comparison as Python integers, 0
    past the last row -- for the conditions the tests put on their inputs (how many bits a pair needs, whether it is a tie)."""
    a = np.asarray(cells).shape[0]
    lhs, rhs = np.zeros((a, window), object), np.zeros((a, window), object)
    for k, m, left, right, _live in _band_sides(cells, window, T):
        lhs[:m, k], rhs[:m, k] = left.astype(object), right.astype(object)
    return lhs, rhs


def hit_band_wrapped64(cells, window, T):
    """hit_band with both sides of the comparison reduced mod 2^64 before they are compared: what a kernel that multiplied in
    64-bit integers would give.  NEVER an expected value: it only states that an input can tell such a kernel from the exact one."""
    out = np.zeros((np.asarray(cells).shape[0], window), bool)
    mask = (1 << 64) - 1
    for k, m, lhs, rhs, live in _band_sides(cells, window, T):
        out[:m, k] = np.asarray((lhs.astype(object) & mask) > (rhs.astype(object) & mask), bool) & live
    return out


def eligible(cells, dropped, min_ac=0, max_ac=0xFFFFFFFF):
    d = dosage(cells)
    n = d.shape[1]
    ac, hom = row_counts(cells)
    v = np.int64(n) * (ac + 2 * hom) - ac * ac
    return ~np.asarray(dropped, bool) & (v > 0) & (ac >= min_ac) & (ac <= max_ac)


def prune_states(cells, dropped, pos, row_begin, row_count, window, T, max_bp=0, min_ac=0, max_ac=0xFFFFFFFF, band=None):
    """(state uint8 [sum(row_count)], keep_begin uint64 [Q + 1], n_kept uint64 [Q]) by the definition: every region's walk over its
    table rows in ascending order, a row kept when it is eligible and no kept row j of the same walk with 1 <= i - j <= window and
    |pos_i - pos_j| <= max_bp (max_bp 0: no limit) hits it.  `band`: hit_band(cells, W, T) of any W >= window, to share it."""
    cells = np.asarray(cells, np.uint8)
    dropped = np.asarray(dropped, bool)
    pos = np.asarray(pos, np.int64)
    if band is None:
        band = hit_band(cells, window, T)
    assert band.shape[1] >= window
    ok = eligible(cells, dropped, min_ac, max_ac)
    row_begin, row_count = np.asarray(row_begin, np.int64), np.asarray(row_count, np.int64)
    keep_begin = np.zeros(row_begin.shape[0] + 1, np.uint64)
    keep_begin[1:] = np.cumsum(row_count)
    state = np.zeros(int(keep_begin[-1]), np.uint8)
    n_kept = np.zeros(row_begin.shape[0], np.uint64)
    kept = np.zeros(cells.shape[0], bool)
    for q in range(row_begin.shape[0]):
        a0, m, o = int(row_begin[q]), int(row_count[q]), int(keep_begin[q])
        kept[a0:a0 + m] = False
        for i in range(a0, a0 + m):
            if dropped[i]:
                state[o + i - a0] = DROPPED
                continue
            if not ok[i]:
                state[o + i - a0] = INELIGIBLE
                continue
            j = np.arange(max(a0, i - window), i)
            block = kept[j] & band[j, i - j - 1]
            if max_bp:
                block &= np.abs(pos[j] - pos[i]) <= max_bp
            if not block.any():
                kept[i] = True
                state[o + i - a0] = KEPT
        n_kept[q] = int(kept[a0:a0 + m].sum())
    return state, keep_begin, n_kept


def kept_despite_pruned_hit(state_q, a0, band, window):
    """Rows of one region (its verdicts state_q, its first table row a0) that are kept although a PRUNED row inside the window hits
    them: what tells the forward greedy from "drop everything that hits anything"."""
    out = []
    for x in np.nonzero(state_q == KEPT)[0]:
        for y in range(max(0, x - window), x):
            if state_q[y] == PRUNED and band[a0 + y, x - y - 1]:
                out.append(int(x))
                break
    return out


def prune_text(heads, ac, state):
    """The text vs_result_format_region gives for one region of a pruning result: heads, ac and state of the region's table rows in
    order (heads[i] = "Pos\\tRef\\tAlt"; dropped rows are left out)."""
    return "Pos\tRef\tAlt\tAC\tState\n" + "".join(f"{h}\t{int(c)}\t{STATE_WORD[int(s)]}\n" for h, c, s in zip(heads, ac, state) if int(s) != DROPPED)


BASES = "ACGT"


def write_ld_block_cohort(dirpath, seed, n_sites=300, n_samples=40, ref_len=6000, p_two_alt=0.06):
    """FASTA + VCF of an "LD-block" cohort: runs of 2 .. 9 sites that are near-copies of one base genotype pattern -- a third of
    them exact copies, the others with one to four flipped calls --, about a tenth of the calls unphased and a few two-ALT records
    (a share p_two_alt of the sites: the draw is made whatever it is, so the default writes the bytes it always wrote, and with 0
    every record is a single-ALT SNP that vcf_truth.TextOracle predicts).  Sites are 4 .. 24 bases apart.  The sample names are
    zero-padded to the width of the largest (three digits up to 999 samples, as ever), so the columns are in name order at every
    width: where they are not, the reference permutes the genotype strings among a site's carriers and the VCF
    text alone no longer says what a row holds.  Returns (fasta, vcf, names, the last site's position)."""
    rng = np.random.default_rng(seed)
    ref = "".join(BASES[i] for i in rng.integers(0, 4, size=ref_len))
    digits = max(3, len(str(n_samples)))
    names = [f"B{i + 1:0{digits}d}" for i in range(n_samples)]
    fasta, vcf = os.path.join(dirpath, f"ldblock{seed}.fa"), os.path.join(dirpath, f"ldblock{seed}.vcf")
    with open(fasta, "w") as f:
        f.write(">c1 ldblock\n")
        for i in range(0, ref_len, 60):
            f.write(ref[i:i + 60] + "\n")
    lines = []
    p = 10
    while len(lines) < n_sites:
        base = np.where(rng.random((n_samples, 2)) < rng.uniform(0.15, 0.5), 1, 0)
        for k in range(int(rng.integers(2, 10))):
            p += int(rng.integers(4, 25))
            assert p < ref_len - 4
            g = base.copy()
            if k and rng.random() > 1 / 3:
                for _ in range(int(rng.integers(1, 5))):
                    g[int(rng.integers(0, n_samples)), int(rng.integers(0, 2))] ^= 1
            if not g.any():
                g[0, 0] = 1
            r0 = ref[p - 1]
            others = [b for b in BASES if b != r0]
            alt = others[int(rng.integers(0, 3))]
            two = rng.random() < p_two_alt
            if two:
                alt += "," + [b for b in others if b != alt][0]
                g = np.where((g == 1) & (rng.random(g.shape) < 0.3), 2, g)
            calls = [f"{a}{'/' if rng.random() < 0.1 else '|'}{b}" for a, b in g]
            lines.append(f"c1\t{p}\t.\t{r0}\t{alt}\t99\t.\t.\tGT\t" + "\t".join(calls) + "\n")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.1\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n")
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n")
        f.write("".join(lines))
    return fasta, vcf, names, p


# Pairs of short dosage patterns whose r^2 is the fraction (num, den) exactly, found by brute force over patterns of length 4 and 6.
# Repeating a pattern c times multiplies cov, v_i and v_j by c^2 each, so cov^2 2^20 == T v_i v_j holds for T = 2^20 num / den at
# every number of columns that is a multiple of the pattern's length.
TIE_PAIRS = (
    ((1, 16), (0, 0, 0, 0, 1, 1), (0, 0, 0, 1, 0, 1)),
    ((1, 8), (0, 0, 1, 1, 2, 2), (0, 1, 1, 2, 1, 1)),
    ((3, 16), (0, 0, 0, 0, 1, 1), (0, 0, 1, 2, 1, 2)),
    ((1, 4), (0, 1, 1, 2), (0, 1, 2, 1)),
    ((3, 8), (0, 0, 0, 0, 1, 1), (0, 1, 1, 1, 1, 2)),
    ((1, 2), (0, 0, 1, 1), (0, 1, 1, 2)),
    ((9, 16), (0, 0, 1, 1, 2, 2), (0, 0, 1, 2, 1, 2)),
    ((5, 8), (0, 0, 0, 0, 1, 1), (0, 0, 0, 1, 1, 2)),
    ((3, 4), (0, 0, 0, 0, 1, 1), (0, 0, 1, 1, 2, 2)),
    ((1, 1), (0, 1, 1, 2), (2, 1, 1, 0)),   # cov < 0
    ((1, 1), (0, 1, 1, 2), (0, 1, 1, 2)),   # cov > 0
)
TIE_REF_LEN = 2400


def tie_threshold(fraction):
    """T = 2^20 num / den of a TIE_PAIRS fraction, an integer."""
    num, den = fraction
    assert (ONE * num) % den == 0
    return ONE * num // den


def write_tie_cohort(dirpath, n_samples, seed):
    """FASTA + VCF (tie.fa, tie.vcf) of the TIE_PAIRS: rows 2 k and 2 k + 1 are pair k, single-ALT SNPs 100 bases apart, each
    pattern repeated across the n_samples columns (a multiple of 12), then ONE seeded permutation of the columns applied to every
    row, which leaves every moment as it was.  Dosage 1 is written as 0|1 or 1|0, 2 as 1|1.  Returns (fasta, vcf, names (sorted: the
    column order is the engine's id order), pos int64 [22], the fractions [11], the dosage matrix written uint8 (22, n_samples),
    source int64 [n_samples]: the position column c had before the permutation -- the columns with source < m, m a multiple of
    12, are m columns of whole patterns again)."""
    assert n_samples % 12 == 0
    rng = np.random.default_rng(seed)
    ref = "".join(BASES[i] for i in rng.integers(0, 4, size=TIE_REF_LEN))
    names = [f"T{i + 1:06d}" for i in range(n_samples)]
    source = rng.permutation(n_samples).astype(np.int64)
    rows = [np.tile(np.asarray(pat, np.uint8), n_samples // len(pat)) for _f, x, y in TIE_PAIRS for pat in (x, y)]
    d = np.stack(rows)[:, source]
    pos = 100 + 100 * np.arange(d.shape[0], dtype=np.int64)
    fasta, vcf = os.path.join(dirpath, "tie.fa"), os.path.join(dirpath, "tie.vcf")
    with open(fasta, "w") as f:
        f.write(">c1 ties\n")
        for i in range(0, TIE_REF_LEN, 60):
            f.write(ref[i:i + 60] + "\n")
    calls = np.array(["0|0", "0|1", "1|1", "1|0"])
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.1\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n")
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n")
        for i, p in enumerate(pos):
            r0 = ref[int(p) - 1]
            alt = [b for b in BASES if b != r0][int(rng.integers(0, 3))]
            which = np.where((d[i] == 1) & (rng.random(n_samples) < 0.5), 3, d[i])
            f.write(f"c1\t{int(p)}\t.\t{r0}\t{alt}\t99\t.\t.\tGT\t" + "\t".join(calls[which]) + "\n")
    return fasta, vcf, names, pos, [f for f, _x, _y in TIE_PAIRS], d, source
