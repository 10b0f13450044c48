"""Reference for vs_query_roh: the header's state machine in plain Python over (cells, pos, site mask, params), a second, independent
formulation for max_het == 0 (numpy: every column's string of sites split at hets and at gaps, then run lengths), an invariant
checker for max_het > 0, the fold of segments into summaries, and the texts of the result and of the command line.  Integers only;
the derived floats are formed the way QueryResult.roh documents them."""
import numpy as np

SUMMARY_DTYPE = np.dtype([("n_segments", "<u4"), ("seg_sites", "<u4"), ("total_bp", "<u8"), ("longest_bp", "<u4"), ("longest_sites", "<u4"),
                          ("seg_hets", "<u4"), ("n_het", "<u4")])
SEGMENT_DTYPE = np.dtype([("region", "<u4"), ("column", "<u4"), ("pos_first", "<u4"), ("pos_last", "<u4"), ("row_first", "<u4"), ("row_last", "<u4"),
                          ("n_sites", "<u4"), ("n_het", "<u4")])
DEFAULTS = dict(min_sites=50, min_bp=0, max_gap=0, max_het=0, min_ac=0, max_ac=0xFFFFFFFF)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    if p["max_ac"] is None:
        p["max_ac"] = 0xFFFFFFFF
    return p


def dosage(cells):
    c = np.asarray(cells).astype(np.int64)
    return ((c >> 1) & 1) + ((c >> 2) & 1)


def site_mask(cells, dropped, min_ac=0, max_ac=0xFFFFFFFF):
    """The rows that are sites: kept by the duplicate rule, 0 < ac < 2 n over the columns, min_ac <= ac <= max_ac."""
    cells = np.asarray(cells)
    ac = dosage(cells).sum(axis=1)
    n = cells.shape[1]
    return (~np.asarray(dropped, bool)) & (ac > 0) & (ac < 2 * n) & (ac >= min_ac) & (ac <= max_ac)


def span(p_first, p_last):
    return max(int(p_last) - int(p_first), 0) + 1


def walk_column(het, pos, rows, p, stats=None):
    """The state machine over one column: het[i], pos[i], rows[i] (the row offset in the region) of site i.  Returns the accepted
    segments as (pos_first, pos_last, row_first, row_last, n_sites, n_het); `stats` counts why runs were closed and rejected."""
    out = []
    run = None   # [first, last, n_sites, n_het, pend]

    def close(why):
        nonlocal run
        first, last, n_sites, n_het, _pend = run
        bp = span(pos[first], pos[last])
        ok_sites, ok_bp = n_sites >= p["min_sites"], bp >= p["min_bp"]
        if stats is not None:
            stats["closed_" + why] += 1
            stats["rejected_min_sites"] += not ok_sites
            stats["rejected_min_bp"] += ok_sites and not ok_bp
        if ok_sites and ok_bp:
            out.append((int(pos[first]), int(pos[last]), int(rows[first]), int(rows[last]), n_sites, n_het))
        run = None

    for i in range(len(pos)):
        if run is not None and p["max_gap"] > 0 and max(int(pos[i]) - int(pos[i - 1]), 0) > p["max_gap"]:
            close("gap")
        if not het[i]:
            if run is None:
                run = [i, i, 1, 0, 0]
            else:
                run[2] += run[4] + 1
                run[3] += run[4]
                run[4] = 0
                run[1] = i
        elif run is not None:
            if run[3] + run[4] < p["max_het"]:
                run[4] += 1
            else:
                close("het")
    if run is not None:
        close("end")
    return out


def new_stats():
    return {k: 0 for k in ("closed_gap", "closed_het", "closed_end", "rejected_min_sites", "rejected_min_bp")}


def fold(segs, n_het):
    """The summary of one cell from its segments (in order of occurrence) and the column's het sites."""
    s = np.zeros((), SUMMARY_DTYPE)
    s["n_het"] = n_het
    for p1, p2, _r1, _r2, n_sites, hets in segs:
        bp = span(p1, p2)
        s["n_segments"] += 1
        s["seg_sites"] += n_sites
        s["total_bp"] += bp
        s["seg_hets"] += hets
        if min(bp, 0xFFFFFFFF) > int(s["longest_bp"]):
            s["longest_bp"], s["longest_sites"] = min(bp, 0xFFFFFFFF), n_sites
    return s


def roh_region(cells, pos, site, p, q=0, stats=None, walker=walk_column):
    """Region q from its rows: cells (rows x columns), pos per row, the site mask.  Returns (summary[columns], segments, n_sites)."""
    cells = np.asarray(cells)
    idx = np.nonzero(np.asarray(site, bool))[0]
    d = dosage(cells[idx]) if idx.size else np.zeros((0, cells.shape[1]), np.int64)
    spos = np.asarray(pos, np.int64)[idx]
    summary = np.zeros(cells.shape[1], SUMMARY_DTYPE)
    segs = []
    for c in range(cells.shape[1]):
        het = d[:, c] == 1
        got = walker(het, spos, idx, p, stats) if walker is walk_column else walker(het, spos, idx, p)
        summary[c] = fold(got, int(het.sum()))
        segs += [(q, c) + g for g in got]
    return summary, segs, int(idx.size)


def roh_batch(cells, pos, site, row_begin, row_count, p, stats=None):
    """The whole answer: summary (Q, S), segments, seg_begin [Q S + 1], n_sites [Q] from the table's cells, positions and site mask
    and the regions' row ranges."""
    cells = np.asarray(cells)
    Q, S = len(row_begin), cells.shape[1]
    summary = np.zeros((Q, S), SUMMARY_DTYPE)
    n_sites = np.zeros(Q, np.uint32)
    all_segs = []
    for q in range(Q):
        a0, k = int(row_begin[q]), int(row_count[q])
        summary[q], segs, n_sites[q] = roh_region(cells[a0:a0 + k], np.asarray(pos)[a0:a0 + k], np.asarray(site)[a0:a0 + k], p, q, stats)
        all_segs += segs
    segments = np.zeros(len(all_segs), SEGMENT_DTYPE)
    for k, g in enumerate(all_segs):
        segments[k] = g
    seg_begin = np.zeros(Q * S + 1, np.uint64)
    seg_begin[1:] = np.cumsum(summary["n_segments"].reshape(-1).astype(np.uint64))
    return {"summary": summary, "segments": segments, "seg_begin": seg_begin, "n_sites": n_sites}


# ---------------------------------------------------------------------------- the second formulation, max_het == 0
def runs_column(het, pos, rows, p):
    """max_het == 0 only, with numpy and no state: a run is a maximal stretch of consecutive hom sites with no break in front of
    any but its first -- a break in front of site i being a het at i - 1 or a gap p_i - p_(i-1) > max_gap.  (A het closes the run
    in front of it and opens none; the gap rule is measured between consecutive sites whatever their state.)"""
    assert p["max_het"] == 0
    het = np.asarray(het, bool)
    n = het.shape[0]
    if n == 0:
        return []
    pos = np.asarray(pos, np.int64)
    brk = np.zeros(n, bool)
    brk[0] = True
    brk[1:] = het[:-1]
    if p["max_gap"] > 0:
        brk[1:] |= np.maximum(pos[1:] - pos[:-1], 0) > p["max_gap"]
    hom = ~het
    start = hom & brk                      # a run's first site
    run_id = np.cumsum(start | het)        # hets get ids of their own, so that they belong to nobody
    out = []
    ids, first, counts = np.unique(run_id[hom], return_index=True, return_counts=True)
    hom_at = np.nonzero(hom)[0]
    for f, cnt in zip(first, counts):
        a, b = int(hom_at[f]), int(hom_at[f + cnt - 1])
        assert b - a + 1 == cnt
        bp = span(pos[a], pos[b])
        if cnt >= p["min_sites"] and bp >= p["min_bp"]:
            out.append((int(pos[a]), int(pos[b]), int(rows[a]), int(rows[b]), int(cnt), 0))
    return out


# ---------------------------------------------------------------------------- invariants, max_het > 0
def check_invariants(summary, segs, het, pos, rows, p):
    """One column's segments against what any answer must satisfy: disjoint and in order, first and last site hom, n_het and n_sites
    the hets and sites inside, n_het <= max_het, no gap inside beyond max_gap, the thresholds met, and the summary their fold."""
    het = np.asarray(het, bool)
    pos = np.asarray(pos, np.int64)
    at = {int(r): i for i, r in enumerate(rows)}
    last_end = -1
    for p1, p2, r1, r2, n_sites, n_het in segs:
        a, b = at[r1], at[r2]
        assert last_end < a <= b, "segments overlap or are out of order"
        last_end = b
        assert not het[a] and not het[b] and int(pos[a]) == p1 and int(pos[b]) == p2
        assert n_sites == b - a + 1 and n_het == int(het[a:b + 1].sum()) <= p["max_het"]
        if p["max_gap"] > 0 and b > a:
            assert int(np.maximum(pos[a + 1:b + 1] - pos[a:b], 0).max()) <= p["max_gap"]
        assert n_sites >= p["min_sites"] and span(p1, p2) >= p["min_bp"]
    want = fold(segs, int(het.sum()))
    assert summary.tobytes() == want.tobytes(), (summary, want)


# ---------------------------------------------------------------------------------------------- floats and texts
def derived(summary, lengths=None):
    total, nseg = summary["total_bp"].astype(np.float64), summary["n_segments"].astype(np.float64)
    out = {"kb": total / 1000.0}
    with np.errstate(divide="ignore", invalid="ignore"):
        out["kb_avg"] = np.where(nseg > 0.0, total / (1000.0 * nseg), np.nan)
        if lengths is not None:
            ln = np.asarray(lengths, np.float64)[:, None]
            out["froh"] = np.where(ln > 0.0, total / ln, np.nan)
    return out


def kb_text(bp):
    return f"{int(bp) // 1000}.{int(bp) % 1000:03d}"


def region_text(segments, names):
    """vs_result_format_region of a ROH result: `segments` the region's, `names[c]` the sample name of column c."""
    out = "Sample\tPos1\tPos2\tKB\tNSites\tNHet\n"
    for g in segments:
        out += f"{names[int(g['column'])]}\t{int(g['pos_first'])}\t{int(g['pos_last'])}\t{kb_text(span(g['pos_first'], g['pos_last']))}\t{int(g['n_sites'])}\t{int(g['n_het'])}\n"
    return out


def cli_segments_text(segments, names, regions):
    out = "Sample\tRegion\tPos1\tPos2\tKB\tNSites\tNHet\n"
    for g in segments:
        x, y = regions[int(g["region"])]
        out += (f"{names[int(g['column'])]}\t{x}:{y}\t{int(g['pos_first'])}\t{int(g['pos_last'])}\t{kb_text(span(g['pos_first'], g['pos_last']))}\t"
                f"{int(g['n_sites'])}\t{int(g['n_het'])}\n")
    return out


def cli_summary_text(summary, names, regions):
    out = "Sample\tRegion\tNSeg\tKB\tKBAvg\tLongestKB\tNHet\n"
    for q, (x, y) in enumerate(regions):
        for c, name in enumerate(names):
            s = summary[q, c]
            n, total = int(s["n_segments"]), int(s["total_bp"])
            out += f"{name}\t{x}:{y}\t{n}\t{kb_text(total)}\t{kb_text(total // n) if n else 'NA'}\t{kb_text(s['longest_bp'])}\t{int(s['n_het'])}\n"
    return out
