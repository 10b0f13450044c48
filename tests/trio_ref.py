"""Reference for trio queries (vs_query_trio_scan): Mendelian errors and transmission counts of (child, father, mother) column
triples of a genotype matrix, computed two ways that must agree.

With f, m, c the dosages popcount(cell & 6) of father, mother and child in one table row, and the gametes a parent of dosage d can
give g(0) = {0}, g(1) = {0, 1}, g(2) = {1}:
  error         c is no sum a + b, a in g(f), b in g(m)
  denovo        f == 0 and m == 0 and c > 0                  (a subset of the errors)
  transmitted   T = c - [f == 2] - [m == 2]                  (consistent cells only; an error cell adds nothing)
  untransmitted U = [f == 1] + [m == 1] - T
A row the duplicate rule dropped is all zeros and adds nothing; it is no site: n_used = rows - dropped rows.

Way 1, the closed forms above, vectorised.  Way 2, brute force: for every cell the gamete pairs (a, b) of its parents' dosages are
enumerated; the cell is consistent when some pair sums to the child's dosage, and then every such pair must tell the same story --
T the ALT gametes heterozygous parents gave, U the REF gametes they gave (a homozygous parent has no choice and counts nowhere).
The enumeration runs once per distinct state (f, m, c) that occurs, never through the closed forms."""
import numpy as np

TRIO_DTYPE = np.dtype([("errors", "<u4"), ("denovo", "<u4"), ("transmitted", "<u4"), ("untransmitted", "<u4")])
FIELDS = ("errors", "denovo", "transmitted", "untransmitted")
GAMETES = {0: (0,), 1: (0, 1), 2: (1,)}


def dosage(cells):
    c = np.asarray(cells).astype(np.int64)
    return ((c >> 1) & 1) + ((c >> 2) & 1)


def state_by_enumeration(f, m, c):
    """(error, denovo, T, U) of one cell from the gamete pairs themselves."""
    stories = set()
    for a in GAMETES[f]:
        for b in GAMETES[m]:
            if a + b != c:
                continue
            t = (a if f == 1 else 0) + (b if m == 1 else 0)
            u = ((1 - a) if f == 1 else 0) + ((1 - b) if m == 1 else 0)
            stories.add((t, u))
    if not stories:
        return 1, int(f == 0 and m == 0 and c > 0), 0, 0
    assert len(stories) == 1, (f, m, c, stories)
    t, u = stories.pop()
    return 0, 0, t, u


def state_closed_form(f, m, c):
    """The same from the closed forms."""
    lo, hi = int(f == 2) + int(m == 2), int(f >= 1) + int(m >= 1)
    if c < lo or c > hi:
        return 1, int(f == 0 and m == 0 and c > 0), 0, 0
    t = c - lo
    return 0, 0, t, int(f == 1) + int(m == 1) - t


def states(cells, trio_cols):
    """(rows, trios) int64 of 9 f + 3 m + c."""
    d = dosage(cells)
    tc = np.asarray(trio_cols, np.int64).reshape(-1, 3)
    return 9 * d[:, tc[:, 1]] + 3 * d[:, tc[:, 2]] + d[:, tc[:, 0]]


def trio_scan(cells, trio_cols, dropped=None):
    """{"row_stats": TRIO_DTYPE[rows], "trio_stats": TRIO_DTYPE[trios], "n_used": int} of a genotype matrix `cells` (rows x columns,
    uint8) and `trio_cols` ((trios, 3): the columns of child, father, mother); `dropped`: the rows the duplicate rule dropped (their
    cells must be zero).  Both ways are computed and asserted equal."""
    cells = np.asarray(cells, np.uint8)
    a = cells.shape[0]
    tc = np.asarray(trio_cols, np.int64).reshape(-1, 3)
    t_n = tc.shape[0]
    dropped = np.zeros(a, bool) if dropped is None else np.asarray(dropped, bool)
    assert dropped.shape == (a,) and not cells[dropped].any(), "a dropped row with a set cell"
    assert (tc >= 0).all() and (tc < max(cells.shape[1], 1)).all()
    d = dosage(cells)
    c, f, m = d[:, tc[:, 0]], d[:, tc[:, 1]], d[:, tc[:, 2]]
    # way 1: closed forms
    lo, hi = (f == 2).astype(np.int64) + (m == 2), (f >= 1).astype(np.int64) + (m >= 1)
    err = (c < lo) | (c > hi)
    den = (f == 0) & (m == 0) & (c > 0)
    tr = np.where(err, 0, c - lo)
    un = np.where(err, 0, (f == 1).astype(np.int64) + (m == 1) - tr)
    assert not (den & ~err).any() and (tr >= 0).all() and (un >= 0).all()
    way1 = np.stack([err.astype(np.int64), den.astype(np.int64), tr, un])           # (4, rows, trios)
    # way 2: the gamete pairs of every state that occurs
    s = 9 * f + 3 * m + c
    way2 = np.zeros_like(way1)
    for st in np.unique(s):
        rec = state_by_enumeration(int(st) // 9, int(st) // 3 % 3, int(st) % 3)
        hit = s == st
        for k in range(4):
            way2[k][hit] = rec[k]
    assert np.array_equal(way1, way2)
    row_stats, trio_stats = np.zeros(a, TRIO_DTYPE), np.zeros(t_n, TRIO_DTYPE)
    for k, name in enumerate(FIELDS):
        row_stats[name] = way1[k].sum(axis=1)
        trio_stats[name] = way1[k].sum(axis=0)
    return {"row_stats": row_stats, "trio_stats": trio_stats, "n_used": int(a - dropped.sum())}


def tdt_chi2(row_stats):
    """(T - U)^2 / (T + U) per row as float64: each integer converted once, one multiplication, one division; NaN where T + U == 0."""
    out = np.full(row_stats.shape[0], np.nan)
    for i, r in enumerate(row_stats):
        t, u = int(r["transmitted"]), int(r["untransmitted"])
        if t + u:
            diff = float(t - u)
            out[i] = diff * diff / float(t + u)
    return out


def error_rate(trio_stats, n_used):
    """errors / n_used per trio as float64; NaN at n_used == 0."""
    if not n_used:
        return np.full(trio_stats.shape[0], np.nan)
    return np.asarray([float(int(e)) / float(n_used) for e in trio_stats["errors"]], np.float64).reshape(trio_stats.shape[0])


def trio_text(heads, ac, row_stats, dropped):
    """The text vs_result_format_region gives for one region of a trio result: heads, ac, row_stats and dropped of the region's table
    rows in order (heads[i] = "Pos\\tRef\\tAlt"; dropped rows are left out)."""
    head = "Pos\tRef\tAlt\tAC\tErrors\tDeNovo\tT\tU\n"
    return head + "".join(f"{h}\t{int(c)}\t{int(r['errors'])}\t{int(r['denovo'])}\t{int(r['transmitted'])}\t{int(r['untransmitted'])}\n"
                          for h, c, r, gone in zip(heads, ac, row_stats, dropped) if not gone)


def trio_table_text(names, trio_stats, n_used):
    """What `variantstore trios --per-trio` writes: names[t] = (child, father, mother) of trio t, in the trio file's order."""
    head = "Child\tFather\tMother\tN\tErrors\tDeNovo\tT\tU\n"
    return head + "".join(f"{c}\t{f}\t{m}\t{int(n_used)}\t{int(r['errors'])}\t{int(r['denovo'])}\t{int(r['transmitted'])}\t{int(r['untransmitted'])}\n"
                          for (c, f, m), r in zip(names, trio_stats))
