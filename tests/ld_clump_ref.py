"""The expected answer of an LD clumping query (vs_query_ld_clump), worked out from a genotype-matrix cell array in Python integers
and numpy integers: the key conversion, the sequential procedure of the definition, the round formulation the kernel may use
instead (the tests show the two equal), the region text, and what the tests ask of an input so that a trivial answer cannot pass.
No floating-point value takes part in a verdict: p-values are compared as the bit patterns of the non-negative doubles."""
import struct

import numpy as np

from ld_prune_ref import eligible, hit_band

MEMBER, INDEX, INELIGIBLE, DROPPED, UNCLUMPED = 0, 1, 2, 3, 4
NO_OWNER = 0xFFFFFFFF
NO_KEY = 0xFFFFFFFFFFFFFFFF
STATE_WORD = {MEMBER: "clumped", INDEX: "index", INELIGIBLE: "skip", UNCLUMPED: "unclumped"}
HEADER = "Pos\tRef\tAlt\tAC\tP\tState\tIndex\n"


def key_of(p):
    """The key of one p-value, a Python integer: the bit pattern of the non-negative double; NaN: NO_KEY.  ValueError outside [0, 1]."""
    p = float(p)
    if p != p:
        return NO_KEY
    if not 0.0 <= p <= 1.0:
        raise ValueError(p)
    return struct.unpack("<Q", struct.pack("<d", p))[0] & ((1 << 63) - 1)   # (-0.0 counts as 0)


def keys_of(pvalues):
    return np.asarray([key_of(p) for p in np.asarray(pvalues, np.float64).ravel()], np.uint64)


def classes(cells, dropped, keys, key1, key2):
    """(candidate, index-eligible) per table row: not dropped, v > 0, a p-value with key <= key2; and key <= key1."""
    keys = np.asarray(keys, np.uint64)
    cand = eligible(cells, dropped) & (keys <= np.uint64(key2))
    return cand, cand & (keys <= np.uint64(key1))


def window_hits(band, pos, window, max_bp=0):
    """bool (rows, window): [i, k] = the pair (i, i + 1 + k) hits and lies at most max_bp positions apart (0: no limit).  The pair
    relation is symmetric: row j < i is read at [j, i - j - 1]."""
    assert band.shape[1] >= window
    b = band[:, :window].copy()
    a = b.shape[0]
    if max_bp:
        pos = np.asarray(pos, np.int64)
        for k in range(min(window, max(a - 1, 0))):
            b[:a - 1 - k, k] &= (pos[1 + k:] - pos[:a - 1 - k]) <= max_bp
    return b


def _setup(cells, dropped, pos, row_begin, row_count, keys, window, T, key1, key2, max_bp, band):
    cells = np.asarray(cells, np.uint8)
    dropped = np.asarray(dropped, bool)
    keys = np.asarray(keys, np.uint64)
    assert keys.shape[0] == cells.shape[0]
    if band is None:
        band = hit_band(cells, window, T)
    wh = window_hits(band, pos, window, max_bp)
    cand, lead = classes(cells, dropped, keys, key1, key2)
    row_begin, row_count = np.asarray(row_begin, np.int64), np.asarray(row_count, np.int64)
    keep_begin = np.zeros(row_begin.shape[0] + 1, np.uint64)
    keep_begin[1:] = np.cumsum(row_count)
    total = int(keep_begin[-1])
    return (dropped, keys, wh, cand, lead, row_begin, row_count, keep_begin, np.zeros(total, np.uint8), np.full(total, NO_OWNER, np.uint32),
            np.zeros(row_begin.shape[0], np.uint64))


def clump_states(cells, dropped, pos, row_begin, row_count, keys, window, T, key1, key2, max_bp=0, band=None):
    """(state uint8, owner uint32, keep_begin uint64 [Q + 1], n_index uint64 [Q]) by the sequential procedure: every region walks
    its index-eligible candidates in (key, row) order; an unassigned one becomes an INDEX and takes every unassigned candidate of
    the region within the window (both ways) and max_bp that it hits.  `band`: hit_band(cells, W, T) of any W >= window."""
    dropped, keys, wh, cand, lead, row_begin, row_count, keep_begin, state, owner, n_index = _setup(
        cells, dropped, pos, row_begin, row_count, keys, window, T, key1, key2, max_bp, band)
    for q in range(row_begin.shape[0]):
        a0, m, o = int(row_begin[q]), int(row_count[q]), int(keep_begin[q])
        st, own = state[o:o + m], owner[o:o + m]
        st[:] = INELIGIBLE
        st[dropped[a0:a0 + m]] = DROPPED
        free = cand[a0:a0 + m].copy()   # the candidates not yet assigned
        leads = np.nonzero(lead[a0:a0 + m])[0]
        for x in leads[np.lexsort((leads, keys[a0 + leads]))]:
            x = int(x)
            if not free[x]:
                continue
            st[x], own[x], free[x] = INDEX, x, False
            n_index[q] += 1
            hi = min(m, x + 1 + window)
            fwd = x + 1 + np.nonzero(wh[a0 + x, :hi - x - 1] & free[x + 1:hi])[0]
            j = np.arange(max(0, x - window), x)
            back = j[wh[a0 + j, x - j - 1] & free[j]]
            for got in (fwd, back):
                st[got], own[got], free[got] = MEMBER, x, False
        st[free] = UNCLUMPED
    return state, owner, keep_begin, n_index


def region_hits(wh, a0, m, window):
    """The symmetric bool (m, m) hit relation of one region's rows from the banded form."""
    h = np.zeros((m, m), bool)
    for k in range(min(window, max(m - 1, 0))):
        d = wh[a0:a0 + m - 1 - k, k]
        i = np.arange(m - 1 - k)
        h[i, i + 1 + k] = d
        h[i + 1 + k, i] = d
    return h


def clump_states_by_rounds(cells, dropped, pos, row_begin, row_count, keys, window, T, key1, key2, max_bp=0, band=None):
    """The same answer by rounds, and the rounds each region takes: a row's BLOCKERS are the index-eligible candidates of its
    region that hit it inside the window and outrank it.  All undecided rows look at once (synchronous rounds): one blocker INDEX
    -> MEMBER; every blocker decided and none INDEX -> INDEX.  Then every candidate that is no INDEX takes the INDEX blocker of the
    highest priority as its owner, or is UNCLUMPED."""
    dropped, keys, wh, cand, lead, row_begin, row_count, keep_begin, state, owner, n_index = _setup(
        cells, dropped, pos, row_begin, row_count, keys, window, T, key1, key2, max_bp, band)
    rounds = np.zeros(row_begin.shape[0], np.uint64)
    for q in range(row_begin.shape[0]):
        a0, m, o = int(row_begin[q]), int(row_count[q]), int(keep_begin[q])
        if not m:
            continue
        st, own = state[o:o + m], owner[o:o + m]
        st[:] = INELIGIBLE
        st[dropped[a0:a0 + m]] = DROPPED
        rank = np.empty(m, np.int64)
        rank[np.lexsort((np.arange(m), keys[a0:a0 + m]))] = np.arange(m)
        c, l = cand[a0:a0 + m], lead[a0:a0 + m]
        blockers = region_hits(wh, a0, m, window) & l[None, :] & (rank[None, :] < rank[:, None]) & c[:, None]
        und, index = l.copy(), np.zeros(m, bool)
        while True:
            rounds[q] += 1
            member = und & (blockers & index[None, :]).any(axis=1)
            wait = (blockers & und[None, :]).any(axis=1)
            new_index = und & ~member & ~wait
            index |= new_index
            und &= ~(member | new_index)
            if not und.any():
                break
            assert rounds[q] <= m
        st[index] = INDEX
        own[index] = np.nonzero(index)[0]
        n_index[q] = int(index.sum())
        for x in np.nonzero(c & ~index)[0]:
            by = np.nonzero(blockers[x] & index)[0]
            if by.size:
                st[x], own[x] = MEMBER, by[np.argmin(rank[by])]
            else:
                assert not l[x]
                st[x] = UNCLUMPED
    return state, owner, keep_begin, n_index, rounds


def first_maximal_independent_set(hits, lead, rank):
    """The lexicographically first maximal independent set of the rows `lead` under the symmetric relation `hits`, in rank order."""
    chosen = np.zeros(lead.shape[0], bool)
    for x in np.argsort(rank):
        if lead[x] and not (hits[x] & chosen).any():
            chosen[x] = True
    return chosen


def index_despite_member_hit(state_q, keys_q, hits):
    """Rows of one region that are INDEX although a MEMBER of higher priority hits them inside the window: what tells the greedy
    from "every local minimum of p is an index"."""
    m = state_q.shape[0]
    rank = np.empty(m, np.int64)
    rank[np.lexsort((np.arange(m), keys_q))] = np.arange(m)
    return [int(x) for x in np.nonzero(state_q == INDEX)[0] if (hits[x] & (state_q == MEMBER) & (rank < rank[x])).any()]


def members_not_with_the_nearest_index(state_q, owner_q, hits):
    """MEMBER rows of one region whose owner is not the nearest INDEX row that hits them."""
    out = []
    index = state_q == INDEX
    for x in np.nonzero(state_q == MEMBER)[0]:
        by = np.nonzero(hits[x] & index)[0]
        nearest = by[np.argmin(np.abs(by - x))]
        if abs(int(owner_q[x]) - int(x)) > abs(int(nearest) - int(x)):
            out.append(int(x))
    return out


def clump_text(heads, ac, pvalues, state, owner):
    """The text vs_result_format_region gives for one region of a clumping result: heads ("Pos\\tRef\\tAlt"), ac, p-values, state and
    owner (region-relative) of the region's table rows in order; dropped rows are left out."""
    out = [HEADER]
    for h, c, p, s, o in zip(heads, ac, pvalues, state, owner):
        if int(s) == DROPPED:
            continue
        ptxt = "." if p != p else "%.6g" % (abs(float(p)) if p == 0 else float(p))
        itxt = "." if int(o) == NO_OWNER else heads[int(o)].replace("\t", ":")
        out.append(f"{h}\t{int(c)}\t{ptxt}\t{STATE_WORD[int(s)]}\t{itxt}\n")
    return "".join(out)


def pvalue_families(n, seed):
    """The five p-value families of the tests, each (name, p float64 [n], p1, p2)."""
    rng = np.random.default_rng(seed)
    uniform = rng.random(n)
    skewed = rng.random(n) ** 4
    tied = rng.choice(np.asarray([0.0, 1e-6, 0.003, 0.2, 1.0]), size=n)
    ordered = (np.arange(n) + 1.0) / (n + 1.0)
    holes = rng.random(n)
    holes[rng.random(n) < 0.1] = np.nan
    return [("uniform", uniform, 1.0, 1.0), ("skewed", skewed, 0.05, 0.3), ("tied", tied, 0.003, 0.2), ("ordered", ordered, 1.0, 1.0),
            ("holes", holes, 0.5, 0.9)]
