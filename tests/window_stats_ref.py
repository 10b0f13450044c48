"""The expected answer of a window-statistics query (vs_query_window_stats), worked out in Python integers from query type 6's text
through group_counts_ref (group_rows for small cohorts, parse_region's arrays for large ones) -- the oracle has no function for it --,
the derived quantities in fractions.Fraction with the rounding-error bounds of the accessor's float64 formulas, and an independent
brute-force check of those formulas that counts differing pairs of allele copies site by site."""
import math
from fractions import Fraction

import numpy as np

from group_counts_ref import group_members, group_rows

HEADER = "Group\tN\tRows\tSeg\tSingletons\tDoubletons\tPrivate\tFixed\tSumAC\tSumAC2\tObsHet\n"
PAIR_HEADER = "GroupA\tGroupB\tSumCross\tSegUnion\tFixedDiff\n"
FIELDS = ("rows", "seg", "singletons", "doubletons", "private", "fixed", "sum_ac", "sum_ac2", "obs_het")
PAIR_FIELDS = ("sum_cross", "seg_union", "fixed_diff")
U = 2.0 ** -53   # the unit roundoff of float64: one correctly rounded operation errs by at most U, relatively


def pair_list(n_groups):
    return [(g, h) for g in range(n_groups) for h in range(g + 1, n_groups)]


def records(ac, het, sizes, pairs=True):
    """The records of one region from ac[row][g] and het[row][g] (sequences of Python integers over the region's reported,
    non-dropped rows) and the groups' sizes in samples: ([dict per group], [dict per pair g < h])."""
    n_groups = len(sizes)
    cn = [2 * int(s) for s in sizes]
    recs = [dict.fromkeys(FIELDS, 0) for _ in range(n_groups)]
    prs = [dict.fromkeys(PAIR_FIELDS, 0) for _ in pair_list(n_groups)] if pairs else []
    for row_ac, row_het in zip(ac, het):
        row_ac = [int(v) for v in row_ac]
        total = sum(row_ac)
        for g in range(n_groups):
            a, r = row_ac[g], recs[g]
            assert 0 <= a <= cn[g]
            r["rows"] += 1
            r["seg"] += 0 < a < cn[g]
            r["singletons"] += a == 1
            r["doubletons"] += a == 2
            r["private"] += a > 0 and total == a
            r["fixed"] += cn[g] > 0 and a == cn[g]
            r["sum_ac"] += a
            r["sum_ac2"] += a * a
            r["obs_het"] += int(row_het[g])
        if pairs:
            for p, (g, h) in enumerate(pair_list(n_groups)):
                a, b = row_ac[g], row_ac[h]
                prs[p]["sum_cross"] += a * b
                prs[p]["seg_union"] += 0 < a + b < cn[g] + cn[h]
                prs[p]["fixed_diff"] += cn[g] > 0 and cn[h] > 0 and ((a == 0 and b == cn[h]) or (a == cn[g] and b == 0))
    return recs, prs


def region_records(text, group_of, n_groups, pairs=True):
    """records of a type-6 region text and a {sample name -> group index} map, with the groups' sizes."""
    sizes = [len(m) for m in group_members(group_of, n_groups)]
    rows = group_rows(text, group_of, n_groups)
    ac = [[c[1] for c in counts] for _p, _r, _a, counts in rows]
    het = [[c[0] - c[2] for c in counts] for _p, _r, _a, counts in rows]
    return records(ac, het, sizes, pairs) + (sizes,)


def parsed_records(parsed, label, n_groups, pairs=True):
    """The same from group_counts_ref.parse_region's arrays, for cohorts too large for a pass per group; `label`: integer array over
    the sample ids, the group of each or -1."""
    heads, ids, row_of, ac, hom, _ph = parsed
    sizes = [int(v) for v in np.bincount(label[label >= 0], minlength=n_groups)]
    lab = label[ids] if ids.shape[0] else ids
    keep = lab >= 0
    key = row_of[keep] * n_groups + lab[keep]
    cells = len(heads) * n_groups
    car = np.bincount(key, minlength=cells)
    acs = np.bincount(key, weights=ac[keep], minlength=cells).astype(np.int64)
    homs = np.bincount(key, weights=hom[keep], minlength=cells).astype(np.int64)
    return records(acs.reshape(-1, n_groups).tolist(), (car - homs).reshape(-1, n_groups).tolist(), sizes, pairs) + (sizes,)


def text(recs, prs, sizes, names=None):
    """The text vs_result_format_region gives for a window-statistics region; `names`: the groups' names (None: decimal indices)."""
    label = (lambda g: str(g)) if names is None else (lambda g: names[g])
    out = [HEADER]
    for g, r in enumerate(recs):
        out.append("\t".join([label(g), str(sizes[g])] + [str(r[f]) for f in FIELDS]) + "\n")
    if prs:
        out.append(PAIR_HEADER)
        for (g, h), r in zip(pair_list(len(recs)), prs):
            out.append("\t".join([label(g), label(h)] + [str(r[f]) for f in PAIR_FIELDS]) + "\n")
    return "".join(out)


def arrays(all_recs, all_prs, stat_dtype, pair_dtype):
    """Structured (Q, G) and (Q, P) arrays of the accessor's dtypes from per-region records."""
    q = len(all_recs)
    g = len(all_recs[0]) if q else 0
    p = len(all_prs[0]) if q else 0
    stats, prs = np.zeros((q, g), stat_dtype), np.zeros((q, p), pair_dtype)
    for i in range(q):
        for j, r in enumerate(all_recs[i]):
            stats[i, j] = tuple(r[f] for f in FIELDS)
        for j, r in enumerate(all_prs[i]):
            prs[i, j] = tuple(r[f] for f in PAIR_FIELDS)
    return stats, prs


# ---- the derived quantities, exactly, and how far the accessor's float64 may be from them ------------------------------------
# Every bound is first order in U and counts the correctly rounded operations of window_stats_derived's formula; an integer below
# 2^53 and a product or sum of such integers that stays below 2^53 are exact.  The test cohorts keep every integer far below that.
def exact_pi(r, n):
    """pi = 2 (N sum_ac - sum_ac2) / (N (N - 1)).  Accessor: the numerator exact in uint64, its conversion (1 rounding -- exact
    below 2^53), x 2 exact, the divisor exact, the division (1): at most 2 U relative."""
    cn = 2 * n
    return Fraction(2 * (cn * r["sum_ac"] - r["sum_ac2"]), cn * (cn - 1)) if cn >= 2 else None


def harmonic(cn, power=1):
    return sum(Fraction(1, i ** power) for i in range(1, cn))


def exact_theta(r, n):
    """theta_w = S / a1.  Accessor: every 1 / i rounded (U each, so the sum of the rounded terms is within U a1), math.fsum (1), the
    division (1): at most 3 U relative."""
    cn = 2 * n
    return Fraction(r["seg"]) / harmonic(cn) if cn >= 2 else None


def exact_het(r, n):
    """het_obs = obs_het / (rows n): the product (1) and the division (1): at most 2 U relative."""
    return Fraction(r["obs_het"], r["rows"] * n) if r["rows"] * n else None


def exact_dxy(rg, rh, pr, ng, nh):
    """dxy = (N_h sum_ac_g + N_g sum_ac_h - 2 sum_cross) / (N_g N_h): numerator exact, its conversion and the division: 2 U relative."""
    cg, ch = 2 * ng, 2 * nh
    return Fraction(ch * rg["sum_ac"] + cg * rh["sum_ac"] - 2 * pr["sum_cross"], cg * ch) if cg and ch else None


def exact_fst(pi_g, pi_h, dxy):
    """fst = 1 - ((pi_g + pi_h) / 2) / dxy.  Accessor: pi_g + pi_h from two values within 2 U each, the sum (1): 3 U of the sum;
    / 2 exact; the division by a dxy within 2 U (1): the ratio r within 6 U r; 1 - r (1): absolute error at most 6 U r + U |1 - r|.
    Returns (value, absolute bound)."""
    if pi_g is None or pi_h is None or dxy is None or dxy == 0:
        return None, 0.0
    ratio = (pi_g + pi_h) / 2 / dxy
    return 1 - ratio, 6 * U * float(ratio) + U * abs(float(1 - ratio))


def exact_tajima(r, n):
    """Tajima's D with its variance in Fraction and one square root, and the absolute bound of the accessor's value: a running
    first-order error analysis of window_stats_derived's operations, the cancellation in pi - S / a1, in c1 = b1 - 1 / a1 and in c2
    carried as absolute errors.  Returns (value, bound), (None, 0) where D is undefined (S = 0, N < 4)."""
    cn, s = 2 * n, r["seg"]
    if cn < 4 or s == 0:
        return None, 0.0
    a1, a2 = harmonic(cn), harmonic(cn, 2)
    b1, b2 = Fraction(cn + 1, 3 * (cn - 1)), Fraction(2 * (cn * cn + cn + 3), 9 * cn * (cn - 1))
    c1, c2 = b1 - 1 / a1, b2 - Fraction(cn + 2) / (a1 * cn) + a2 / (a1 * a1)
    e1, e2 = c1 / a1, c2 / (a1 * a1 + a2)
    var = e1 * s + e2 * s * (s - 1)
    pi, theta = exact_pi(r, n), exact_theta(r, n)
    num = pi - theta
    if var <= 0:
        return None, 0.0
    value = float(num) / math.sqrt(float(var))           # (three more roundings of its own: 3 U relative)
    f = lambda x: abs(float(x))
    # a1, a2: 2 U relative (the rounded terms, fsum).  b1, b2: integers and their products exact, one division each.
    d_inv = 3 * U * f(1 / a1)                             # 1 / a1: a1's 2 U and the division
    d_c1 = U * f(b1) + d_inv + U * f(c1)                  # b1 - 1 / a1
    d_t1 = 4 * U * f(Fraction(cn + 2) / (a1 * cn))        # (N + 2) / (a1 N): a1's 2 U, the product, the division
    d_t2 = 8 * U * f(a2 / (a1 * a1))                      # a2 / (a1 a1): 2 U, a1 a1 within 4 U + 1, the division
    d_c2 = U * f(b2) + d_t1 + U * f(b2 - Fraction(cn + 2) / (a1 * cn)) + d_t2 + U * f(c2)
    d_e1 = d_c1 / f(a1) + 3 * U * f(e1)                   # c1 / a1
    den = a1 * a1 + a2                                    # a1 a1 (5 U) + a2 (2 U), the sum: 6 U relative
    d_e2 = d_c2 / f(den) + 7 * U * f(e2)
    d_var = (d_e1 + U * f(e1)) * s + (d_e2 + 2 * U * f(e2)) * s * (s - 1) + U * f(var)
    sq = math.sqrt(float(var))
    rel_sq = d_var / (2 * float(var)) + U                 # the square root halves the relative error, and rounds once
    d_num = 2 * U * f(pi) + 3 * U * f(theta) + U * f(num)   # pi - S / a1
    bound = d_num / sq + abs(value) * (rel_sq + U) + 3 * U * abs(value)
    return value, bound


def check_derived(got, all_recs, all_prs, sizes):
    """window_stats_derived's arrays (`got`) against the exact values, region by region, within the bounds derived above (x 1.001
    for the second-order terms: they are smaller than the first-order ones by factors of U times the condition numbers above);
    a quantity that is undefined must be NaN and a defined one must not."""
    def close(value, exact, bound, what):
        if exact is None:
            assert math.isnan(value), what
        else:
            assert not math.isnan(value) and abs(value - float(exact)) <= 1.001 * bound + U * abs(float(exact)), (what, value, float(exact), bound)

    n_groups = len(sizes)
    for q, (recs, prs) in enumerate(zip(all_recs, all_prs)):
        pis = []
        for g in range(n_groups):
            pi = exact_pi(recs[g], sizes[g])
            pis.append(pi)
            close(got["pi"][q, g], pi, 2 * U * abs(float(pi or 0)), ("pi", q, g))
            th = exact_theta(recs[g], sizes[g])
            close(got["theta_w"][q, g], th, 3 * U * abs(float(th or 0)), ("theta_w", q, g))
            he = exact_het(recs[g], sizes[g])
            close(got["het_obs"][q, g], he, 2 * U * abs(float(he or 0)), ("het_obs", q, g))
            d, bound = exact_tajima(recs[g], sizes[g])
            close(got["tajima_d"][q, g], d, bound, ("tajima_d", q, g))
        for p, (g, h) in enumerate(pair_list(n_groups) if prs else []):
            dxy = exact_dxy(recs[g], recs[h], prs[p], sizes[g], sizes[h])
            close(got["dxy"][q, p], dxy, 2 * U * abs(float(dxy or 0)), ("dxy", q, p))
            fst, bound = exact_fst(pis[g], pis[h], dxy)
            close(got["fst_hudson"][q, p], fst, bound, ("fst_hudson", q, p))


# ---- brute force: the allele copies themselves --------------------------------------------------------------------------------
def site_copies(text, members):
    """Per reported row of a type-6 region text and per group (members: [set of sample names]) the list of its N = 2 n allele
    copies, 0 or 1: a sample that the row does not list carries two reference copies."""
    out = []
    for line in text.split("\n")[1:]:
        if not line:
            continue
        calls = {}
        for tok in line.split("\t")[3].split(" "):
            if tok:
                name, gt = tok[:-1].rsplit("(", 1)
                calls[name] = (int(gt[0] == "1"), int(gt[2] == "1"))
        out.append([[c for name in sorted(m) for c in calls.get(name, (0, 0))] for m in members])
    return out


def brute_force(text, members):
    """(pi per group, dxy per pair, fst per pair) of a region as Fractions (None where undefined), by counting, site by site, the
    pairs of allele copies that differ: within a group over its C(N, 2) pairs, between two groups over their N_g N_h pairs."""
    sites = site_copies(text, members)
    n_groups = len(members)
    pi = []
    for g in range(n_groups):
        cn = 2 * len(members[g])
        if cn < 2:
            pi.append(None)
            continue
        total = Fraction(0)
        for site in sites:
            c = site[g]
            total += Fraction(sum(c[i] != c[j] for i in range(cn) for j in range(i + 1, cn)), cn * (cn - 1) // 2)
        pi.append(total)
    dxy, fst = [], []
    for g, h in pair_list(n_groups):
        cg, ch = 2 * len(members[g]), 2 * len(members[h])
        if not cg or not ch:
            dxy.append(None); fst.append(None)
            continue
        d = sum((Fraction(sum(x != y for x in site[g] for y in site[h]), cg * ch) for site in sites), Fraction(0))
        dxy.append(d)
        fst.append(1 - (pi[g] + pi[h]) / 2 / d if pi[g] is not None and pi[h] is not None and d != 0 else None)
    return pi, dxy, fst
