"""Host-side mirror of the reference's query interface, over the C ABI.

The reference's driver (src/commands.cc:114-215) builds `Index idx(prefix)` and
`VariantGraph vg(prefix, mode)` and calls `get_var_in_ref(&vg, &idx, x, y, ...)`
(include/query.h:736) or `get_sample_var_in_ref(..., sample, ...)` (query.h:618)
per region.  Here one `VariantStore` object plays the (vg, idx) pair and the two
query methods take a whole batch of regions; each returns a `QueryResult` whose
per-region content is what the reference's `std::vector<Variant>` would hold.
All computation happens in the HIP engine.
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import ConstructStats, IndexInfo, Region, ResultRaw, ResultView, SynthParams, Timing

REGION_EMPTY = 1
REGION_INVALID = 2
VAR_DROPPED = 1


class VariantStoreError(RuntimeError):
    def __init__(self, code, where):
        lib = _lib.load()
        msg = lib.vs_last_error().decode() or lib.vs_strerror(code).decode()
        super().__init__(f"{where}: {msg} (code {code})")
        self.code = code


def _check(code, where):
    if code != 0:
        raise VariantStoreError(code, where)


@dataclass
class Variant:  # reference include/query.h:30-36
    var_pos: int
    ref: str
    alt: str
    samples: List[Tuple[str, str]]


class DeviceArray:
    """An array that already lies in device memory: `ptr` (an integer address, e.g. a torch tensor's data_ptr()) and its
    number of elements -- regions ({u64 beg, u64 end} pairs) or sample ids (u32).  The walking query types
    (get_sample_var_in_ref with one sample per region, query_sample_seq, get_sample_var_in_sample) take it wherever they
    take a host array; the engine then neither reads the array on the host nor copies it over the link."""

    def __init__(self, ptr, n):
        self.ptr = int(ptr)
        self.n = int(n)


def quantise_traits(y):
    """The engine's own quantiser (vs_assoc_matrix_quantise, host-only): `y` array-like of shape (n,) or (n, K), float32, finite.
    Returns (q, shift): q ((n, K) int32) = rint(y * 2**shift[k]) per column, ties to even, |q| < 2**30; shift int32[K]."""
    y = np.asarray(y, dtype=np.float32)
    if y.ndim == 1:
        y = y.reshape(-1, 1)
    if y.ndim != 2 or y.shape[0] == 0 or y.shape[1] == 0:
        raise ValueError("traits: a non-empty array of shape (n,) or (n, K)")
    y = np.ascontiguousarray(y)
    q = np.zeros(y.shape, np.int32)
    shift = np.zeros(y.shape[1], np.int32)
    _check(_lib.load().vs_assoc_matrix_quantise(y.ctypes.data_as(C.POINTER(C.c_float)), y.shape[0], y.shape[1],
                                                q.ctypes.data_as(C.POINTER(C.c_int32)), shift.ctypes.data_as(C.POINTER(C.c_int32))),
           "vs_assoc_matrix_quantise")
    return q, shift


PRUNE_THRESHOLD_ONE = 1 << 20   # VS_PRUNE_THRESHOLD_ONE: the integer threshold of r2 = 1


def quantise_r2(r2):
    """The integer threshold T of an r2 bound for VariantStore.ld_prune: floor(r2 * 2**20 + 0.5), 0 .. 2**20.  The pruning decides
    r2 > T / 2**20 in exact integers.  ValueError outside [0, 1]."""
    r2 = float(r2)
    if not 0.0 <= r2 <= 1.0:   # (a NaN fails both comparisons)
        raise ValueError(f"r2 {r2!r}: a bound between 0 and 1")
    return int(math.floor(r2 * PRUNE_THRESHOLD_ONE + 0.5))


CLUMP_NO_KEY = 0xFFFFFFFFFFFFFFFF   # the key of "no p-value" (NaN): above the key of every p-value


def pvalue_keys(p):
    """The 64-bit keys VariantStore.ld_clump orders p-values by: the bit pattern of each non-negative double (-0.0 counts as 0),
    which is monotone in p; NaN ("no p-value") gives CLUMP_NO_KEY.  uint64, of p's shape.  ValueError for any other value outside
    [0, 1]."""
    p = np.asarray(p, dtype=np.float64)
    nan = np.isnan(p)
    if not np.all(nan | ((p >= 0.0) & (p <= 1.0))):
        raise ValueError("p-values lie between 0 and 1 (NaN: none)")
    keys = np.where(nan, 0.0, np.abs(p)).astype(np.float64).view(np.uint64).copy()   # (abs: -0.0)
    keys[nan] = CLUMP_NO_KEY
    return keys


def trio_tdt_chi2(row_stats):
    """The transmission disequilibrium statistic of every row of a trio result: (T - U)**2 / (T + U) as float64 from the row's exact
    transmitted and untransmitted counts -- each integer (T - U and T + U, formed in int64) converted once, one multiplication, one
    division.  NaN where T + U == 0."""
    t, u = row_stats["transmitted"].astype(np.int64), row_stats["untransmitted"].astype(np.int64)
    diff, total = (t - u).astype(np.float64), (t + u).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(total > 0.0, diff * diff / total, np.nan)


def trio_error_rate(trio_stats, n_used):
    """The Mendelian error rate of every trio of a trio result: errors / n_used as float64, NaN at n_used == 0."""
    if not n_used:
        return np.full(trio_stats.shape[0], np.nan)
    return trio_stats["errors"].astype(np.float64) / float(n_used)


def roh_derived(summary, lengths=None):
    """The derived figures of a ROH result, formed in float64 from its exact integers alone (QueryResult.roh calls this; `summary`
    is its (Q, S) structured array): `kb` = total_bp / 1000, `kb_avg` = total_bp / (1000 n_segments), NaN in a cell without
    segments, and -- with `lengths`, one length in bases per region -- `froh` = total_bp / lengths[q] (NaN where the length is 0).
    Each integer is converted once and each figure is one division."""
    total = summary["total_bp"].astype(np.float64)
    nseg = summary["n_segments"].astype(np.float64)
    out = {"kb": total / 1000.0}
    with np.errstate(divide="ignore", invalid="ignore"):
        out["kb_avg"] = np.where(nseg > 0.0, total / (1000.0 * nseg), np.nan)
        if lengths is not None:
            ln = np.asarray(lengths, dtype=np.float64).reshape(-1)
            if ln.shape[0] != summary.shape[0]:
                raise ValueError(f"{ln.shape[0]} lengths for {summary.shape[0]} regions")
            out["froh"] = np.where(ln[:, None] > 0.0, total / ln[:, None], np.nan)
    return out


def window_stats_derived(stats, pairs, group_sizes, lengths=None):
    """The diversity statistics of a window-statistics result, formed in float64 from its exact integers (QueryResult.window_stats
    calls this; `stats` (Q, G) and `pairs` (Q, P) are its structured arrays, `group_sizes` the G sizes in samples).  With n a
    group's size, N = 2 n its allele copies (two per sample whatever the ploidy), S = seg, and per region:

      pi          = 2 (N sum_ac - sum_ac2) / (N (N - 1))      the mean number of differences between two of the N copies, summed
                                                              over the window's sites (sum over sites of 2 ac (N - ac) / (N (N - 1)));
                                                              N sum_ac - sum_ac2 is formed exactly in uint64; NaN for N < 2
      pi_per_bp   = pi / lengths[q]                           only with `lengths`
      theta_w     = S / a1,  a1 = sum_{i=1}^{N-1} 1/i         Watterson's estimator; NaN for N < 2
      tajima_d    = (pi - S / a1) / sqrt(e1 S + e2 S (S - 1)) Tajima 1989: a2 = sum 1/i^2, b1 = (N + 1) / (3 (N - 1)),
                                                              b2 = 2 (N^2 + N + 3) / (9 N (N - 1)), c1 = b1 - 1 / a1,
                                                              c2 = b2 - (N + 2) / (a1 N) + a2 / a1^2, e1 = c1 / a1,
                                                              e2 = c2 / (a1^2 + a2); NaN for S = 0 and for N < 4 (the variance
                                                              is identically zero at N = 2 and 3)
      het_obs     = obs_het / (rows n)                        observed heterozygosity per site and sample; NaN for rows n = 0
      dxy         = (N_h sum_ac_g + N_g sum_ac_h - 2 sum_cross) / (N_g N_h)
                                                              the mean number of differences between a copy of g and a copy of h,
                                                              summed over the window's sites; the numerator exact in uint64; NaN
                                                              when either group is empty
      fst_hudson  = 1 - ((pi_g + pi_h) / 2) / dxy             Hudson's Fst as the ratio of the window's sums (scikit-allel's
                                                              hudson_fst); NaN where pi_g, pi_h or dxy is NaN or dxy = 0

    An undefined quantity is NaN, never an exception.  Returns a dict with those arrays ((Q, G) and (Q, P)) and `pair_index`
    ((P, 2): the groups g < h of pair p, in the order (0,1), (0,2), ..., (G-2,G-1))."""
    stats, pairs = np.asarray(stats), np.asarray(pairs)
    q, ng = stats.shape
    n = [int(x) for x in np.asarray(group_sizes).reshape(-1)]
    nan = np.full((q, ng), np.nan)
    pi, theta, taj, het = nan.copy(), nan.copy(), nan.copy(), nan.copy()
    big = q > 0 and int(stats["rows"].max()) >= 1 << 31   # (only then can a numerator leave 64 bits: Python integers instead)
    wide = (lambda a: a.astype(object)) if big else (lambda a: a.astype(np.uint64))
    sum_ac, sum_ac2 = wide(stats["sum_ac"]), wide(stats["sum_ac2"])
    with np.errstate(divide="ignore", invalid="ignore"):
        for g in range(ng):
            cn = 2 * n[g]
            rows = stats["rows"][:, g].astype(np.float64)
            if n[g]:
                het[:, g] = np.where(rows > 0, stats["obs_het"][:, g].astype(np.float64) / (rows * float(n[g])), np.nan)
            if cn < 2:
                continue
            num = (int(cn) if big else np.uint64(cn)) * sum_ac[:, g] - sum_ac2[:, g]
            pi[:, g] = 2.0 * num.astype(np.float64) / float(cn * (cn - 1))
            a1 = math.fsum(1.0 / i for i in range(1, cn))
            s = stats["seg"][:, g].astype(np.float64)
            theta[:, g] = s / a1
            if cn < 4:
                continue
            a2 = math.fsum(1.0 / (i * i) for i in range(1, cn))
            b1 = (cn + 1) / (3.0 * (cn - 1))
            b2 = 2.0 * (cn * cn + cn + 3) / (9.0 * cn * (cn - 1))
            c1 = b1 - 1.0 / a1
            c2 = b2 - (cn + 2) / (a1 * cn) + a2 / (a1 * a1)
            e1 = c1 / a1
            e2 = c2 / (a1 * a1 + a2)
            var = e1 * s + e2 * s * (s - 1.0)
            taj[:, g] = np.where((s > 0) & (var > 0), (pi[:, g] - theta[:, g]) / np.sqrt(var), np.nan)
        pair_index = np.array([(g, h) for g in range(ng) for h in range(g + 1, ng)], dtype=np.uint32).reshape(-1, 2)
        npair = pairs.shape[1] if pairs.ndim == 2 else 0
        dxy, fst = np.full((q, npair), np.nan), np.full((q, npair), np.nan)
        if npair:
            cross = wide(pairs["sum_cross"])
            for p, (g, h) in enumerate(pair_index.tolist()):
                ng_, nh_ = 2 * n[g], 2 * n[h]
                if not ng_ or not nh_:
                    continue
                cg, ch = (int(nh_), int(ng_)) if big else (np.uint64(nh_), np.uint64(ng_))
                num = cg * sum_ac[:, g] + ch * sum_ac[:, h] - (2 if big else np.uint64(2)) * cross[:, p]
                dxy[:, p] = num.astype(np.float64) / float(ng_ * nh_)
                fst[:, p] = np.where(dxy[:, p] > 0, 1.0 - ((pi[:, g] + pi[:, h]) / 2.0) / dxy[:, p], np.nan)
    out = {"pi": pi, "theta_w": theta, "tajima_d": taj, "het_obs": het, "dxy": dxy, "fst_hudson": fst,
           "pair_index": pair_index if npair else np.zeros((0, 2), np.uint32)}
    if lengths is not None:
        ln = np.asarray(lengths, dtype=np.float64).reshape(-1)
        if ln.shape[0] != q:
            raise ValueError(f"{ln.shape[0]} window lengths for {q} regions")
        with np.errstate(divide="ignore", invalid="ignore"):
            out["pi_per_bp"] = pi / ln[:, None]
    return out


def _regions_array(regions):
    if isinstance(regions, DeviceArray):
        return regions, C.cast(C.c_void_p(regions.ptr), C.POINTER(Region)), regions.n
    arr = np.ascontiguousarray(np.asarray(regions, dtype=np.uint64).reshape(-1, 2))
    return arr, arr.ctypes.data_as(C.POINTER(Region)), arr.shape[0]


def _u32_ptr(ids):
    if isinstance(ids, DeviceArray):
        return C.cast(C.c_void_p(ids.ptr), C.POINTER(C.c_uint32))
    return ids.ctypes.data_as(C.POINTER(C.c_uint32))


class QueryResult:
    def __init__(self, store, handle):
        self._store = store
        self._h = handle
        self._lib = store._lib
        self.subset_size = 0   # allele-count results: |S|, the samples the counts are over (region_counts' af)

    def close(self):
        if self._h:
            self._lib.vs_result_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def totals(self):
        """(n_regions, n_variants, n_carriers, n_bases) over the whole batch."""
        v = [C.c_uint64() for _ in range(4)]
        _check(self._lib.vs_result_totals(self._h, *[C.byref(x) for x in v]), "vs_result_totals")
        return tuple(int(x.value) for x in v)

    def sequences(self):
        """(region_flags, list of str) of a sequence result (query types 2 and 3)."""
        n = C.c_uint64()
        fl = C.POINTER(C.c_uint8)()
        beg = C.POINTER(C.c_uint64)()
        chars = C.c_char_p()
        _check(self._lib.vs_result_get_sequences(self._h, C.byref(n), C.byref(fl), C.byref(beg), C.byref(chars)),
               "vs_result_get_sequences")
        q = int(n.value)
        flags = np.ctypeslib.as_array(fl, shape=(q,)).copy() if q else np.zeros(0, np.uint8)
        b = np.ctypeslib.as_array(beg, shape=(q + 1,)).copy() if q else np.zeros(1, np.uint64)
        raw = C.string_at(C.cast(chars, C.c_void_p).value, int(b[q])) if q else b""
        return flags, [raw[int(b[i]):int(b[i + 1])].decode("latin-1") for i in range(q)]

    def layout(self):
        """(rows reported over all regions, rows of the variant table, arena entries, carrier lists expanded, rows and lists
        shared between regions?) of the result in HBM."""
        n, t, s, u, sh = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
        _check(self._lib.vs_result_layout(self._h, C.byref(n), C.byref(t), C.byref(s), C.byref(u), C.byref(sh)), "vs_result_layout")
        return int(n.value), int(t.value), int(s.value), int(u.value), bool(sh.value)

    def fill_ms(self):
        """Duration of the carrier expansion when it ran asynchronously (option "async_fill"; waits for it), else -1."""
        ms = C.c_float()
        _check(self._lib.vs_result_fill_ms(self._h, C.byref(ms)), "vs_result_fill_ms")
        return float(ms.value)

    def digest(self):
        d = C.c_uint64()
        _check(self._lib.vs_result_digest(self._h, C.byref(d)), "vs_result_digest")
        return int(d.value)

    def view(self, with_carriers=True):
        """Host copy of the result as numpy arrays (dict)."""
        rv = ResultView()
        _check(self._lib.vs_result_get_view(self._h, 1 if with_carriers else 0, C.byref(rv)), "vs_result_get_view")
        q, a, s = int(rv.n_regions), int(rv.n_slots), int(rv.n_carriers)

        def arr(ptr, n, dt):
            if n == 0 or not ptr:
                return np.zeros(0, dtype=dt)
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy()

        return {
            "region_flags": arr(rv.region_flags, q, np.uint8),
            "var_begin": arr(rv.var_begin, q + 1, np.uint64),
            "var_count": arr(rv.var_count, q, np.uint64),
            "pos": arr(rv.pos, a, np.uint64),
            "ref_off": arr(rv.ref_off, a, np.uint32), "ref_len": arr(rv.ref_len, a, np.uint32),
            "alt_off": arr(rv.alt_off, a, np.uint32), "alt_len": arr(rv.alt_len, a, np.uint32),
            "var_flags": arr(rv.var_flags, a, np.uint32),
            "car_begin": arr(rv.car_begin, a, np.uint64), "car_count": arr(rv.car_count, a, np.uint32),
            "carriers": arr(rv.carriers, s, np.uint32) if with_carriers else None,
        }

    ROW_DTYPE = np.dtype([("pos", "<u4"), ("ref_off", "<u4"), ("ref_len", "<u4"), ("alt_off", "<u4"), ("alt_len", "<u4"),
                          ("count_flags", "<u4"), ("car_begin", "<u8")])

    def raw(self, with_carriers=True):
        """The result as it lies in HBM, copied once into page-locked memory (vs_result_get_raw): numpy VIEWS (no copy; valid
        until the result is closed) of the per-region arrays, the variant table (structured rows) and the carrier arena
        (uint16 words id | gt << 13 for cohorts of at most 4032 samples, else uint32 id | gt << 29)."""
        rr = ResultRaw()
        _check(self._lib.vs_result_get_raw(self._h, 1 if with_carriers else 0, C.byref(rr)), "vs_result_get_raw")
        q, a, s = int(rr.n_regions), int(rr.n_rows), int(rr.arena_entries)

        def arr(ptr, n, dt):
            if n == 0 or not ptr:
                return np.zeros(0, dtype=dt)
            return np.ctypeslib.as_array(ptr, shape=(n,))

        rows = (np.ctypeslib.as_array(C.cast(rr.rows, C.POINTER(C.c_uint8)), shape=(a * 32,)).view(self.ROW_DTYPE)
                if a else np.zeros(0, self.ROW_DTYPE))
        arena = None
        if with_carriers and rr.arena:
            ct = C.c_uint16 if rr.carrier_bytes == 2 else C.c_uint32
            arena = np.ctypeslib.as_array(C.cast(rr.arena, C.POINTER(ct)), shape=(s,)) if s else np.zeros(0, np.uint16)
        return {"region_flags": arr(rr.region_flags, q, np.uint8), "row_begin": arr(rr.row_begin, q, np.uint64),
                "row_count": arr(rr.row_count, q, np.uint64), "var_count": arr(rr.var_count, q, np.uint64),
                "car_base": arr(rr.car_base, q, np.uint64), "car_len": arr(rr.car_len, q, np.uint64),
                "rows": rows, "arena": arena, "carrier_bytes": int(rr.carrier_bytes), "shared": bool(rr.shared & 1),
                "resident": bool(rr.shared & 2), "scattered": bool(rr.shared & 4)}

    def num_header_records(self):
        n = C.c_uint64()
        _check(self._lib.vs_result_pack_headers(self._h, None, 0, 0, C.byref(n)), "vs_result_pack_headers")
        return int(n.value)

    def pack_headers_into(self, device_ptr, capacity_records, region_base=0):
        """Write the hit-list records (4 x uint64 per variant slot) into device memory at `device_ptr`
        (e.g. a torch CUDA tensor's data_ptr()) for a collective over the shards of a batch."""
        n = C.c_uint64()
        _check(self._lib.vs_result_pack_headers(self._h, C.c_void_p(device_ptr), capacity_records, region_base,
                                                C.byref(n)), "vs_result_pack_headers")
        return int(n.value)

    def num_region_records(self):
        n = C.c_uint64()
        _check(self._lib.vs_result_pack_regions(self._h, None, 0, 0, C.byref(n)), "vs_result_pack_regions")
        return int(n.value)

    def pack_regions_into(self, device_ptr, capacity_records, region_base=0):
        """Compact hit lists: one 4 x uint64 record per region (site range of the replicated index)."""
        n = C.c_uint64()
        _check(self._lib.vs_result_pack_regions(self._h, C.c_void_p(device_ptr), capacity_records, region_base,
                                                C.byref(n)), "vs_result_pack_regions")
        return int(n.value)

    def region_text(self, q):
        """The `-o` file the reference writes for region q (query.h:38-50, 774-781)."""
        txt = C.c_char_p()
        n = C.c_uint64()
        _check(self._lib.vs_result_format_region(self._h, q, C.byref(txt), C.byref(n)), "vs_result_format_region")
        return C.string_at(txt, n.value).decode("latin-1")

    COUNT_DTYPE = np.dtype([("carriers", "<u4"), ("alt_alleles", "<u4"), ("hom_alt", "<u4"), ("phased", "<u4")])

    def allele_counts(self):
        """An allele-count result (VariantStore.allele_counts) as numpy arrays: the variant table's `rows` and their `counts`
        (structured: carriers, alt_alleles, hom_alt, phased; counts[i] belongs to rows[i]), and per region `row_begin`,
        `row_count` and `flags` -- region q reports rows[row_begin[q] : row_begin[q] + row_count[q]].  Copies, valid after
        the result is closed."""
        raw = self.raw(with_carriers=False)
        n = C.c_uint64()
        p = C.POINTER(_lib.AlleleCounts)()
        _check(self._lib.vs_result_get_allele_counts(self._h, C.byref(n), C.byref(p)), "vs_result_get_allele_counts")
        a = int(n.value)
        counts = (np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(a * 16,)).view(self.COUNT_DTYPE).copy()
                  if a else np.zeros(0, self.COUNT_DTYPE))
        return {"rows": raw["rows"].copy(), "counts": counts, "row_begin": raw["row_begin"].copy(),
                "row_count": raw["row_count"].copy(), "flags": raw["region_flags"].copy()}

    def region_counts(self, q):
        """The rows region q reports (dropped ones left out) with their counts: a list of dicts with pos, ref, alt, carriers,
        alt_alleles, hom_alt, phased and af = alt_alleles / (2 |S|), S the subset the query was made for."""
        out = []
        for line in self.region_text(q).split("\n")[1:]:
            if not line:
                continue
            pos, ref, alt, car, ac, hom, ph = line.split("\t")
            ac = int(ac)
            out.append({"pos": int(pos), "ref": ref, "alt": alt, "carriers": int(car), "alt_alleles": ac, "hom_alt": int(hom),
                        "phased": int(ph), "af": ac / (2.0 * self.subset_size) if self.subset_size else 0.0})
        return out

    def group_counts(self):
        """A grouped-count result (VariantStore.group_counts) as numpy arrays: the variant table's `rows`, `counts` (structured
        as for allele_counts, shape (A, G): counts[i, g] is row i over the samples of group g), `group_sizes` (uint32[G]),
        `group_names` (list of G strings) and per region `row_begin`, `row_count` and `flags`.  Copies, valid after the result
        is closed."""
        n, g = C.c_uint64(), C.c_uint32()
        sizes = C.POINTER(C.c_uint32)()
        p = C.POINTER(_lib.AlleleCounts)()
        _check(self._lib.vs_result_get_group_counts(self._h, C.byref(n), C.byref(g), C.byref(sizes), C.byref(p)),
               "vs_result_get_group_counts")
        a, ng = int(n.value), int(g.value)
        counts = (np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(a * ng * 16,)).view(self.COUNT_DTYPE).copy()
                  if a else np.zeros(0, self.COUNT_DTYPE)).reshape(a, ng)
        raw = self.raw(with_carriers=False)
        names = getattr(self, "group_names", None) or [str(i) for i in range(ng)]
        return {"rows": raw["rows"].copy(), "counts": counts, "group_sizes": np.ctypeslib.as_array(sizes, shape=(ng,)).copy(),
                "group_names": list(names), "row_begin": raw["row_begin"].copy(), "row_count": raw["row_count"].copy(),
                "flags": raw["region_flags"].copy()}

    def region_group_counts(self, q):
        """The rows region q of a grouped-count result reports (dropped ones left out): a list of dicts with pos, ref, alt and
        `groups`, which maps each group's name to carriers, alt_alleles, hom_alt, phased, n (the group's size) and
        af = alt_alleles / (2 n) -- 0.0 for an empty group."""
        out = []
        for line in self.region_text(q).split("\n")[1:]:
            if not line:
                continue
            pos, ref, alt, name, n, car, ac, hom, ph = line.split("\t")
            if not out or (out[-1]["pos"], out[-1]["ref"], out[-1]["alt"]) != (int(pos), ref, alt) or name in out[-1]["groups"]:
                out.append({"pos": int(pos), "ref": ref, "alt": alt, "groups": {}})
            n, ac = int(n), int(ac)
            out[-1]["groups"][name] = {"carriers": int(car), "alt_alleles": ac, "hom_alt": int(hom), "phased": int(ph), "n": n,
                                       "af": ac / (2.0 * n) if n else 0.0}
        return out

    def group_counts_device(self):
        """(address, A, G) of a grouped-count result's records as they lie in this GPU's memory: A x G records of four uint32
        (carriers, alt_alleles, hom_alt, phased), row-major, complete when this returns and valid until the result is closed."""
        n, g = C.c_uint64(), C.c_uint32()
        p = C.c_void_p()
        _check(self._lib.vs_result_group_counts_device(self._h, C.byref(n), C.byref(g), C.byref(p)), "vs_result_group_counts_device")
        return int(p.value or 0), int(n.value), int(g.value)

    WINDOW_DTYPE = np.dtype([("rows", "<u4"), ("seg", "<u4"), ("singletons", "<u4"), ("doubletons", "<u4"), ("private", "<u4"),
                             ("fixed", "<u4"), ("sum_ac", "<u8"), ("sum_ac2", "<u8"), ("obs_het", "<u8")])   # vs_window_stats
    WINDOW_PAIR_DTYPE = np.dtype([("sum_cross", "<u8"), ("seg_union", "<u4"), ("fixed_diff", "<u4")])     # vs_window_pair_stats

    def window_stats(self, lengths=None):
        """A window-statistics result (VariantStore.window_stats) as numpy arrays: `stats` (structured WINDOW_DTYPE, shape (Q, G):
        stats[q, g] is region q over group g -- rows, seg, singletons, doubletons, private, fixed, sum_ac, sum_ac2, obs_het),
        `pairs` (structured WINDOW_PAIR_DTYPE, shape (Q, P): sum_cross, seg_union, fixed_diff; P = 0 without pair records),
        `pair_index` ((P, 2): the groups g < h of pair p), `group_sizes` (uint32[G], samples), `group_names` (list of G strings),
        the regions' `flags`, `row_begin` and `row_count`, and the quantities window_stats_derived forms from the exact integers in
        float64 -- `pi`, `theta_w`, `tajima_d`, `het_obs` (each (Q, G)), `dxy`, `fst_hudson` (each (Q, P)) and, with `lengths` (Q
        window lengths in bp), `pi_per_bp`: the formulas are written out there.  Copies, valid after the result is closed."""
        nq, g, p = C.c_uint64(), C.c_uint32(), C.c_uint32()
        sizes = C.POINTER(C.c_uint32)()
        names = C.POINTER(C.c_char_p)()
        ps, pp = C.c_void_p(), C.c_void_p()
        _check(self._lib.vs_result_get_window_stats(self._h, C.byref(nq), C.byref(g), C.byref(p), C.byref(sizes), C.byref(names), C.byref(ps),
                                                    C.byref(pp)), "vs_result_get_window_stats")
        q, ng, npair = int(nq.value), int(g.value), int(p.value)
        stats = np.ctypeslib.as_array(C.cast(ps, C.POINTER(C.c_uint8)), shape=(q * ng * 48,)).view(self.WINDOW_DTYPE).copy().reshape(q, ng)
        pairs = (np.ctypeslib.as_array(C.cast(pp, C.POINTER(C.c_uint8)), shape=(q * npair * 16,)).view(self.WINDOW_PAIR_DTYPE).copy()
                 if npair else np.zeros(0, self.WINDOW_PAIR_DTYPE)).reshape(q, npair)
        group_sizes = np.ctypeslib.as_array(sizes, shape=(ng,)).copy()
        raw = self.raw(with_carriers=False)
        out = {"stats": stats, "pairs": pairs, "group_sizes": group_sizes,
               "group_names": [names[i].decode() for i in range(ng)] if names else [str(i) for i in range(ng)],
               "flags": raw["region_flags"].copy(), "row_begin": raw["row_begin"].copy(), "row_count": raw["row_count"].copy()}
        out.update(window_stats_derived(stats, pairs, group_sizes, lengths))
        return out

    def region_window_stats(self, q, stats=None):
        """Region q of a window-statistics result: a dict of views into `stats` (window_stats() of this result; taken now when
        None) -- `stats` (G records), `pairs` (P records) and the region's row of every derived quantity."""
        got = self.window_stats() if stats is None else stats
        q = int(q)
        if not 0 <= q < got["stats"].shape[0]:
            raise IndexError(f"region {q} of {got['stats'].shape[0]}")
        keys = ("stats", "pairs", "pi", "pi_per_bp", "theta_w", "tajima_d", "het_obs", "dxy", "fst_hudson")
        out = {k: got[k][q] for k in keys if k in got}
        out["pair_index"], out["group_sizes"], out["group_names"] = got["pair_index"], got["group_sizes"], got["group_names"]
        return out

    def window_stats_device(self):
        """A window-statistics result as it lies in this GPU's memory: a dict of the addresses `stats` (n_regions x n_groups records
        of 48 bytes) and `pairs` (n_regions x n_pairs records of 16 bytes; 0 without), with `n_regions`, `n_groups` and `n_pairs`;
        complete when this returns and valid until the result is closed."""
        nq, g, p = C.c_uint64(), C.c_uint32(), C.c_uint32()
        ps, pp = C.c_void_p(), C.c_void_p()
        _check(self._lib.vs_result_window_stats_device(self._h, C.byref(nq), C.byref(g), C.byref(p), C.byref(ps), C.byref(pp)),
               "vs_result_window_stats_device")
        return {"stats": int(ps.value or 0), "pairs": int(pp.value or 0), "n_regions": int(nq.value), "n_groups": int(g.value),
                "n_pairs": int(p.value)}

    ASSOC_STATS = {"dot": 0, "chi2": 1}   # VS_ASSOC_DOT, VS_ASSOC_CHI2

    def assoc_scan(self):
        """An association-scan result (VariantStore.assoc_scan) as numpy arrays: `scores` ((A, K) float64: scores[i, k] is table row
        i against trait k -- the sum of dosage x value under stat "dot", the score test under "chi2"), `counts` (structured as for
        allele_counts: the count record of every table row over the query's samples), `col_ids` (uint32[n], the sample ids the
        sums run over, ascending), `trait_sum` and `trait_sumsq` (float64[K]: Sy and Syy over those samples), `trait_names`
        (list of K strings), `stat`, the table's `rows` and per region `row_begin`, `row_count` and `flags` -- region q's rows are
        rows[row_begin[q] : row_begin[q] + row_count[q]].  Copies, valid after the result is closed."""
        a, c = C.c_uint64(), C.c_uint64()
        k, st = C.c_uint32(), C.c_uint32()
        cols = C.POINTER(C.c_uint32)()
        sy, syy, sc = C.POINTER(C.c_double)(), C.POINTER(C.c_double)(), C.POINTER(C.c_double)()
        cnt = C.POINTER(_lib.AlleleCounts)()
        _check(self._lib.vs_result_get_assoc_scan(self._h, C.byref(a), C.byref(c), C.byref(k), C.byref(st), C.byref(cols), C.byref(sy),
                                                  C.byref(syy), C.byref(cnt), C.byref(sc)), "vs_result_get_assoc_scan")
        na, nc, nk = int(a.value), int(c.value), int(k.value)
        if na:
            scores = np.ctypeslib.as_array(sc, shape=(na * nk,)).reshape(na, nk).copy()
            counts = np.ctypeslib.as_array(C.cast(cnt, C.POINTER(C.c_uint8)), shape=(na * 16,)).view(self.COUNT_DTYPE).copy()
        else:
            scores, counts = np.zeros((0, nk), np.float64), np.zeros(0, self.COUNT_DTYPE)
        raw = self.raw(with_carriers=False)
        names = self.region_text(0).split("\n")[0].split("\t")[7:]   # (the result's own: the header of every region's text)
        return {"rows": raw["rows"].copy(), "row_begin": raw["row_begin"].copy(), "row_count": raw["row_count"].copy(),
                "flags": raw["region_flags"].copy(), "scores": scores, "counts": counts,
                "col_ids": np.ctypeslib.as_array(cols, shape=(nc,)).copy(), "trait_sum": np.ctypeslib.as_array(sy, shape=(nk,)).copy(),
                "trait_sumsq": np.ctypeslib.as_array(syy, shape=(nk,)).copy(), "trait_names": list(names),
                "stat": "chi2" if st.value == self.ASSOC_STATS["chi2"] else "dot"}

    def region_assoc(self, q):
        """The rows region q of an association-scan result reports (dropped ones left out): a list of dicts with pos, ref, alt,
        carriers, alt_alleles, hom_alt, phased and `scores`, which maps each trait's name to its float."""
        lines = self.region_text(q).split("\n")
        names = lines[0].split("\t")[7:]
        out = []
        for line in lines[1:]:
            if not line:
                continue
            f = line.split("\t")
            out.append({"pos": int(f[0]), "ref": f[1], "alt": f[2], "carriers": int(f[3]), "alt_alleles": int(f[4]), "hom_alt": int(f[5]),
                        "phased": int(f[6]), "scores": {n: float(v) for n, v in zip(names, f[7:])}})
        return out

    def assoc_scan_device(self):
        """(scores address, counts address, n_rows, n_cols, n_traits, stat) of an association-scan result as it lies in this GPU's
        memory: n_rows x n_traits float64 cells, row-major, and n_rows count records of four uint32, complete when this returns and
        valid until the result is closed."""
        a, c = C.c_uint64(), C.c_uint64()
        k, st = C.c_uint32(), C.c_uint32()
        pc, ps = C.c_void_p(), C.c_void_p()
        _check(self._lib.vs_result_assoc_scan_device(self._h, C.byref(a), C.byref(c), C.byref(k), C.byref(st), C.byref(pc), C.byref(ps)),
               "vs_result_assoc_scan_device")
        return (int(ps.value or 0), int(pc.value or 0), int(a.value), int(c.value), int(k.value),
                "chi2" if st.value == self.ASSOC_STATS["chi2"] else "dot")

    def assoc_matrix(self):
        """A trait-matrix association result (VariantStore.assoc_matrix) as numpy arrays: what assoc_scan() gives -- `scores`
        ((A, K) float64), `counts`, `col_ids`, `trait_sum`, `trait_sumsq`, `trait_names`, `stat`, `rows`, `row_begin`, `row_count`,
        `flags` -- plus `shift` (int32[K]: trait k was quantised as q = rint(y * 2**shift[k])) and, under stat "dot", `sums`
        ((A, K) int64: the exact integers sum of dosage x q, scores = ldexp(sums, -shift); None under "chi2").  trait_sum and
        trait_sumsq are the exact sums of q and q*q scaled back.  Copies, valid after the result is closed."""
        a, c = C.c_uint64(), C.c_uint64()
        k, st = C.c_uint32(), C.c_uint32()
        cols = C.POINTER(C.c_uint32)()
        sh = C.POINTER(C.c_int32)()
        sy, syy, sc = C.POINTER(C.c_double)(), C.POINTER(C.c_double)(), C.POINTER(C.c_double)()
        cnt = C.POINTER(_lib.AlleleCounts)()
        _check(self._lib.vs_result_get_assoc_matrix(self._h, C.byref(a), C.byref(c), C.byref(k), C.byref(st), C.byref(cols), C.byref(sh),
                                                    C.byref(sy), C.byref(syy), C.byref(cnt), C.byref(sc)), "vs_result_get_assoc_matrix")
        na, nc, nk = int(a.value), int(c.value), int(k.value)
        if na:
            scores = np.ctypeslib.as_array(sc, shape=(na * nk,)).reshape(na, nk).copy()
            counts = np.ctypeslib.as_array(C.cast(cnt, C.POINTER(C.c_uint8)), shape=(na * 16,)).view(self.COUNT_DTYPE).copy()
        else:
            scores, counts = np.zeros((0, nk), np.float64), np.zeros(0, self.COUNT_DTYPE)
        shift = np.ctypeslib.as_array(sh, shape=(nk,)).copy()
        stat = "chi2" if st.value == self.ASSOC_STATS["chi2"] else "dot"
        sums = np.ldexp(scores, shift[None, :]).astype(np.int64) if stat == "dot" else None   # (exact: |sum| <= 2^53)
        raw = self.raw(with_carriers=False)
        names = self.region_text(0).split("\n")[0].split("\t")[7:]   # (the result's own: the header of every region's text)
        return {"rows": raw["rows"].copy(), "row_begin": raw["row_begin"].copy(), "row_count": raw["row_count"].copy(),
                "flags": raw["region_flags"].copy(), "scores": scores, "sums": sums, "shift": shift, "counts": counts,
                "col_ids": np.ctypeslib.as_array(cols, shape=(nc,)).copy(), "trait_sum": np.ctypeslib.as_array(sy, shape=(nk,)).copy(),
                "trait_sumsq": np.ctypeslib.as_array(syy, shape=(nk,)).copy(), "trait_names": list(names), "stat": stat}

    def region_assoc_matrix(self, q):
        """The rows region q of a trait-matrix association result reports, as region_assoc gives them."""
        return self.region_assoc(q)

    def assoc_matrix_device(self):
        """(scores address, counts address, n_rows, n_cols, n_traits, stat) of a trait-matrix association result as it lies in this
        GPU's memory: n_rows x n_traits float64 cells, row-major, and n_rows count records of four uint32, complete when this
        returns and valid until the result is closed."""
        a, c = C.c_uint64(), C.c_uint64()
        k, st = C.c_uint32(), C.c_uint32()
        pc, ps = C.c_void_p(), C.c_void_p()
        _check(self._lib.vs_result_assoc_matrix_device(self._h, C.byref(a), C.byref(c), C.byref(k), C.byref(st), C.byref(pc), C.byref(ps)),
               "vs_result_assoc_matrix_device")
        return (int(ps.value or 0), int(pc.value or 0), int(a.value), int(c.value), int(k.value),
                "chi2" if st.value == self.ASSOC_STATS["chi2"] else "dot")

    def sample_scores(self):
        """A per-sample score result (VariantStore.sample_scores) as numpy arrays: `scores` ((n, K) float64: scores[c, k] is the
        sum over the reported rows of dosage x weight k for the sample of column c), `sums` ((n, K) int64: the same sums in fixed
        point, exact) and `shift` (int32[K]: scores = ldexp(sums, -shift)), `col_ids` (uint32[n], the sample ids of the columns,
        ascending) and their `names`, `score_names` (list of K strings), the table's `rows` and per region `row_begin`,
        `row_count` and `flags`.  Copies, valid after the result is closed."""
        c, k = C.c_uint64(), C.c_uint32()
        cols = C.POINTER(C.c_uint32)()
        sh = C.POINTER(C.c_int32)()
        su = C.POINTER(C.c_int64)()
        sc = C.POINTER(C.c_double)()
        _check(self._lib.vs_result_get_sample_scores(self._h, C.byref(c), C.byref(k), C.byref(cols), C.byref(sh), C.byref(su), C.byref(sc)),
               "vs_result_get_sample_scores")
        nc, nk = int(c.value), int(k.value)
        raw = self.raw(with_carriers=False)
        col_ids = np.ctypeslib.as_array(cols, shape=(nc,)).copy()
        given = getattr(self, "score_names", None)
        return {"rows": raw["rows"].copy(), "row_begin": raw["row_begin"].copy(), "row_count": raw["row_count"].copy(),
                "flags": raw["region_flags"].copy(), "col_ids": col_ids, "names": [self._store.sample_name(int(i)) for i in col_ids],
                "shift": np.ctypeslib.as_array(sh, shape=(nk,)).copy(),
                "sums": np.ctypeslib.as_array(su, shape=(nc * nk,)).reshape(nc, nk).copy(),
                "scores": np.ctypeslib.as_array(sc, shape=(nc * nk,)).reshape(nc, nk).copy(),
                "score_names": list(given) if given else [str(i) for i in range(nk)]}

    def sample_scores_device(self):
        """(scores address, sums address, n_cols, n_scores) of a per-sample score result as it lies in this GPU's memory:
        n_cols x n_scores float64 scores and int64 sums, row-major, complete when this returns and valid until the result is closed."""
        c, k = C.c_uint64(), C.c_uint32()
        pu, ps = C.c_void_p(), C.c_void_p()
        _check(self._lib.vs_result_sample_scores_device(self._h, C.byref(c), C.byref(k), C.byref(pu), C.byref(ps)),
               "vs_result_sample_scores_device")
        return int(ps.value or 0), int(pu.value or 0), int(c.value), int(k.value)

    def score_matrix(self):
        """A score-matrix result (VariantStore.score_matrix) as numpy arrays: `scores` ((n, K) float64), `sums` ((n, K) int64: the
        same sums in fixed point, exact), `shift` (int32[K]: scores = ldexp(sums, -shift)) and `limbs` (4 or 5: the int8 limbs the
        kernel split the rows' weight totals into), `col_ids` (uint32[n], the sample ids of the columns, ascending) and their
        `names`, `score_names` (list of K strings), the table's `rows` and per region `row_begin`, `row_count` and `flags`.
        Copies, valid after the result is closed."""
        c, k, lb = C.c_uint64(), C.c_uint32(), C.c_uint32()
        cols = C.POINTER(C.c_uint32)()
        sh = C.POINTER(C.c_int32)()
        su = C.POINTER(C.c_int64)()
        sc = C.POINTER(C.c_double)()
        _check(self._lib.vs_result_get_score_matrix(self._h, C.byref(c), C.byref(k), C.byref(cols), C.byref(sh), C.byref(lb), C.byref(su),
                                                    C.byref(sc)), "vs_result_get_score_matrix")
        nc, nk = int(c.value), int(k.value)
        raw = self.raw(with_carriers=False)
        col_ids = np.ctypeslib.as_array(cols, shape=(nc,)).copy()
        given = getattr(self, "score_names", None)
        return {"rows": raw["rows"].copy(), "row_begin": raw["row_begin"].copy(), "row_count": raw["row_count"].copy(),
                "flags": raw["region_flags"].copy(), "col_ids": col_ids, "names": [self._store.sample_name(int(i)) for i in col_ids],
                "shift": np.ctypeslib.as_array(sh, shape=(nk,)).copy(), "limbs": int(lb.value),
                "sums": np.ctypeslib.as_array(su, shape=(nc * nk,)).reshape(nc, nk).copy(),
                "scores": np.ctypeslib.as_array(sc, shape=(nc * nk,)).reshape(nc, nk).copy(),
                "score_names": list(given) if given else [str(i) for i in range(nk)]}

    def score_matrix_device(self):
        """(scores address, sums address, n_cols, n_scores) of a score-matrix result as it lies in this GPU's memory:
        n_cols x n_scores float64 scores and int64 sums, row-major, complete when this returns and valid until the result is closed."""
        c, k = C.c_uint64(), C.c_uint32()
        pu, ps = C.c_void_p(), C.c_void_p()
        _check(self._lib.vs_result_score_matrix_device(self._h, C.byref(c), C.byref(k), C.byref(pu), C.byref(ps)),
               "vs_result_score_matrix_device")
        return int(ps.value or 0), int(pu.value or 0), int(c.value), int(k.value)

    BURDEN_DTYPE = np.dtype([("variants", "<u4"), ("alt_alleles", "<u4"), ("hom_alt", "<u4"), ("phased", "<u4")])

    def sample_burden(self):
        """A burden result (VariantStore.sample_burden) as numpy arrays: `columns` (uint32[C], the sample id of each column,
        ascending), `cells` (structured (Q, C): variants, alt_alleles, hom_alt, phased; row q is region q of the batch as it
        was given) and per region `flags`.  Copies, valid after the result is closed."""
        q, c = C.c_uint64(), C.c_uint64()
        cols = C.POINTER(C.c_uint32)()
        p = C.POINTER(_lib.SampleBurden)()
        _check(self._lib.vs_result_get_sample_burden(self._h, C.byref(q), C.byref(c), C.byref(cols), C.byref(p)),
               "vs_result_get_sample_burden")
        nq, nc = int(q.value), int(c.value)
        cells = (np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nq * nc * 16,)).view(self.BURDEN_DTYPE)
                 .reshape(nq, nc).copy())
        return {"columns": np.ctypeslib.as_array(cols, shape=(nc,)).copy(), "cells": cells,
                "flags": self.raw(with_carriers=False)["region_flags"].copy()}

    def sample_burden_device(self):
        """(address, Q, C) of a burden result's matrix as it lies in this GPU's memory: Q x C cells of four uint32, row-major,
        complete when this returns and valid until the result is closed."""
        q, c = C.c_uint64(), C.c_uint64()
        p = C.c_void_p()
        _check(self._lib.vs_result_sample_burden_device(self._h, C.byref(q), C.byref(c), C.byref(p)),
               "vs_result_sample_burden_device")
        return int(p.value or 0), int(q.value), int(c.value)

    def genotype_matrix(self):
        """A genotype-matrix result (VariantStore.genotype_matrix) as numpy arrays: `columns` (uint32[C], the sample id of each
        column, ascending), `cells` (uint8 (A, C): row i belongs to row i of the variant table, 0 = not a carrier, else
        0x08 | genotype bits; a view of the pitched buffer: cells.strides[0] == row_pitch), `row_pitch`, the table's
        `rows` and per region `row_begin`, `row_count` and `flags` -- region q's rows are
        cells[row_begin[q] : row_begin[q] + row_count[q]].  Copies, valid after the result is closed."""
        a, c, pitch = C.c_uint64(), C.c_uint64(), C.c_uint64()
        cols = C.POINTER(C.c_uint32)()
        p = C.POINTER(C.c_uint8)()
        _check(self._lib.vs_result_get_genotype_matrix(self._h, C.byref(a), C.byref(c), C.byref(pitch), C.byref(cols), C.byref(p)),
               "vs_result_get_genotype_matrix")
        na, nc, np_ = int(a.value), int(c.value), int(pitch.value)
        buf = (np.ctypeslib.as_array(p, shape=(na * np_,)).copy() if na else np.zeros(0, np.uint8)).reshape(na, np_)
        raw = self.raw(with_carriers=False)
        return {"columns": np.ctypeslib.as_array(cols, shape=(nc,)).copy(), "cells": buf[:, :nc], "row_pitch": np_,
                "rows": raw["rows"].copy(), "row_begin": raw["row_begin"].copy(), "row_count": raw["row_count"].copy(),
                "flags": raw["region_flags"].copy()}

    def genotype_matrix_device(self):
        """(address, n_rows, n_cols, row_pitch) of a genotype-matrix result's matrix as it lies in this GPU's memory: n_rows rows
        of row_pitch bytes, complete when this returns and valid until the result is closed."""
        a, c, pitch = C.c_uint64(), C.c_uint64(), C.c_uint64()
        p = C.c_void_p()
        _check(self._lib.vs_result_genotype_matrix_device(self._h, C.byref(a), C.byref(c), C.byref(pitch), C.byref(p)),
               "vs_result_genotype_matrix_device")
        return int(p.value or 0), int(a.value), int(c.value), int(pitch.value)

    def region_genotypes(self, q):
        """The rows region q of a genotype-matrix result reports (dropped ones left out): a list of dicts with pos, ref, alt and
        `calls`, per column `0` for a non-carrier or the call as type 6 prints it (`1|1`, `0/1`, ...)."""
        out = []
        for line in self.region_text(q).split("\n")[1:]:
            if not line:
                continue
            pos, ref, alt, *calls = line.split("\t")
            out.append({"pos": int(pos), "ref": ref, "alt": alt, "calls": calls})
        return out

    LD_STATS = {"dot": 0, "r2": 1}   # VS_LD_DOT, VS_LD_R2

    def ld_band(self):
        """An LD result (VariantStore.ld_band) as numpy arrays: `band` ((A, W): band[i, k] belongs to the pair of table rows
        (i, i + 1 + k); int32 dot products of the dosages under stat "dot", float32 squared correlations under "r2"; 0 where
        i + 1 + k >= A), `counts` (structured as for allele_counts: the count record of every table row over the query's
        samples), `columns` (uint32[C], the sample ids the statistics run over), `window`, `stat`, the table's `rows` and per
        region `row_begin` and `row_count` -- region q's pairs are those inside rows[row_begin[q] : row_begin[q] + row_count[q]].
        Copies, valid after the result is closed."""
        a, c = C.c_uint64(), C.c_uint64()
        w, st = C.c_uint32(), C.c_uint32()
        cols = C.POINTER(C.c_uint32)()
        cnt = C.POINTER(_lib.AlleleCounts)()
        p = C.c_void_p()
        _check(self._lib.vs_result_get_ld_band(self._h, C.byref(a), C.byref(c), C.byref(w), C.byref(st), C.byref(cols), C.byref(cnt),
                                               C.byref(p)), "vs_result_get_ld_band")
        na, nc, nw = int(a.value), int(c.value), int(w.value)
        stat = "r2" if st.value == self.LD_STATS["r2"] else "dot"
        dtype = np.float32 if stat == "r2" else np.int32
        if na:
            band = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(na * nw * 4,)).view(dtype).reshape(na, nw).copy()
            counts = np.ctypeslib.as_array(C.cast(cnt, C.POINTER(C.c_uint8)), shape=(na * 16,)).view(self.COUNT_DTYPE).copy()
        else:
            band, counts = np.zeros((0, nw), dtype), np.zeros(0, self.COUNT_DTYPE)
        raw = self.raw(with_carriers=False)
        return {"rows": raw["rows"].copy(), "row_begin": raw["row_begin"].copy(), "row_count": raw["row_count"].copy(),
                "columns": np.ctypeslib.as_array(cols, shape=(nc,)).copy(), "window": nw, "stat": stat, "counts": counts,
                "band": band}

    def ld_band_device(self):
        """(band address, counts address, n_rows, n_cols, window, stat) of an LD result as it lies in this GPU's memory: n_rows x
        window cells of 4 bytes (int32 under "dot", float32 under "r2") and n_rows count records of four uint32, complete when
        this returns and valid until the result is closed."""
        a, c = C.c_uint64(), C.c_uint64()
        w, st = C.c_uint32(), C.c_uint32()
        pc, pb = C.c_void_p(), C.c_void_p()
        _check(self._lib.vs_result_ld_band_device(self._h, C.byref(a), C.byref(c), C.byref(w), C.byref(st), C.byref(pc), C.byref(pb)),
               "vs_result_ld_band_device")
        return (int(pb.value or 0), int(pc.value or 0), int(a.value), int(c.value), int(w.value),
                "r2" if st.value == self.LD_STATS["r2"] else "dot")

    PRUNE_STATES = {"pruned": 0, "kept": 1, "ineligible": 2, "dropped": 3}   # VS_PRUNE_*

    def ld_prune(self):
        """A pruning result (VariantStore.ld_prune) as numpy arrays: `state` (uint8, a verdict per reported row: PRUNE_STATES),
        `keep_begin` (uint64[Q + 1], the exclusive scan of row_count: region q's verdicts are state[keep_begin[q] :
        keep_begin[q + 1]], for the table rows row_begin[q] .. + row_count[q]), `n_kept` (uint64[Q]), `threshold` (the exact
        T / 2**20 the walk used), `threshold_q20` (T), `window`, `max_bp`, `min_ac`, `max_ac`, `counts` (structured as for
        allele_counts: the count record of every table row over the query's samples), `columns` (uint32[C], the sample ids), the
        table's `rows` and per region `row_begin` and `row_count`.  Copies, valid after the result is closed."""
        nq, a, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        params = (C.c_uint32 * 5)()
        cols = C.POINTER(C.c_uint32)()
        cnt = C.POINTER(_lib.AlleleCounts)()
        kb, nk = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        p = C.POINTER(C.c_uint8)()
        _check(self._lib.vs_result_get_ld_prune(self._h, C.byref(nq), C.byref(a), C.byref(c), params, C.byref(cols), C.byref(cnt),
                                                C.byref(kb), C.byref(nk), C.byref(p)), "vs_result_get_ld_prune")
        q, na, nc = int(nq.value), int(a.value), int(c.value)
        keep_begin = np.ctypeslib.as_array(kb, shape=(q + 1,)).copy()
        n_kept = np.ctypeslib.as_array(nk, shape=(q,)).copy() if q else np.zeros(0, np.uint64)
        total = int(keep_begin[q])
        state = np.ctypeslib.as_array(p, shape=(total,)).copy() if total else np.zeros(0, np.uint8)
        counts = (np.ctypeslib.as_array(C.cast(cnt, C.POINTER(C.c_uint8)), shape=(na * 16,)).view(self.COUNT_DTYPE).copy() if na
                  else np.zeros(0, self.COUNT_DTYPE))
        raw = self.raw(with_carriers=False)
        return {"rows": raw["rows"].copy(), "row_begin": raw["row_begin"].copy(), "row_count": raw["row_count"].copy(),
                "columns": np.ctypeslib.as_array(cols, shape=(nc,)).copy(), "counts": counts, "state": state, "keep_begin": keep_begin,
                "n_kept": n_kept, "threshold": int(params[2]) / PRUNE_THRESHOLD_ONE, "threshold_q20": int(params[2]),
                "window": int(params[0]), "max_bp": int(params[1]), "min_ac": int(params[3]), "max_ac": int(params[4])}

    def ld_prune_device(self):
        """(state address, keep_begin address, n_kept address, counts address, n_regions, n_rows, n_cols) of a pruning result as it
        lies in this GPU's memory: keep_begin[n_regions] verdict bytes, n_regions + 1 and n_regions uint64 words and n_rows count
        records of four uint32, complete when this returns and valid until the result is closed."""
        nq, a, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        pc, pb, pn, ps = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(self._lib.vs_result_ld_prune_device(self._h, C.byref(nq), C.byref(a), C.byref(c), C.byref(pc), C.byref(pb), C.byref(pn),
                                                   C.byref(ps)), "vs_result_ld_prune_device")
        return (int(ps.value or 0), int(pb.value or 0), int(pn.value or 0), int(pc.value or 0), int(nq.value), int(a.value),
                int(c.value))

    def region_kept(self, q):
        """The rows region q of a pruning result keeps: a list of (pos, ref, alt), in the table's order."""
        out = []
        for line in self.region_text(q).split("\n")[1:]:
            if not line:
                continue
            pos, ref, alt, _ac, state = line.split("\t")
            if state == "keep":
                out.append((int(pos), ref, alt))
        return out

    CLUMP_STATES = {"member": 0, "index": 1, "ineligible": 2, "dropped": 3, "unclumped": 4}   # VS_CLUMP_*
    CLUMP_NO_OWNER = 0xFFFFFFFF   # VS_CLUMP_NO_OWNER

    def ld_clump(self):
        """A clumping result (VariantStore.ld_clump) as numpy arrays: `state` (uint8, a verdict per reported row: CLUMP_STATES),
        `owner` (uint32, the region-relative row of the verdict's index row, CLUMP_NO_OWNER for a row that is neither index nor
        member), `keep_begin` (uint64[Q + 1]: region q's verdicts are state[keep_begin[q] : keep_begin[q + 1]], for the table rows
        row_begin[q] .. + row_count[q]), `n_index` (uint64[Q]), `rounds` (uint64[Q], a diagnostic: the parallel rounds each region
        took; not part of the answer), `pvalues` (float64 per table row, as the query took them), `threshold` / `threshold_q20`,
        `window`, `max_bp`, `p1`, `p2`, `p1_key`, `p2_key`, `counts`, `columns`, the table's `rows` and per region `row_begin` and
        `row_count`.  Copies, valid after the result is closed."""
        nq, a, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        params = (C.c_uint32 * 3)()
        pkeys, pb = (C.c_uint64 * 2)(), (C.c_double * 2)()
        cols = C.POINTER(C.c_uint32)()
        cnt = C.POINTER(_lib.AlleleCounts)()
        kb, ni, rd = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        p, o = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint32)()
        _check(self._lib.vs_result_get_ld_clump(self._h, C.byref(nq), C.byref(a), C.byref(c), params, pkeys, pb, C.byref(cols), C.byref(cnt),
                                                C.byref(kb), C.byref(ni), C.byref(rd), C.byref(p), C.byref(o)), "vs_result_get_ld_clump")
        q, na, nc = int(nq.value), int(a.value), int(c.value)
        keep_begin = np.ctypeslib.as_array(kb, shape=(q + 1,)).copy()
        n_index = np.ctypeslib.as_array(ni, shape=(q,)).copy() if q else np.zeros(0, np.uint64)
        rounds = np.ctypeslib.as_array(rd, shape=(q,)).copy() if q else np.zeros(0, np.uint64)
        total = int(keep_begin[q])
        state = np.ctypeslib.as_array(p, shape=(total,)).copy() if total else np.zeros(0, np.uint8)
        owner = np.ctypeslib.as_array(o, shape=(total,)).copy() if total else np.zeros(0, np.uint32)
        counts = (np.ctypeslib.as_array(C.cast(cnt, C.POINTER(C.c_uint8)), shape=(na * 16,)).view(self.COUNT_DTYPE).copy() if na
                  else np.zeros(0, self.COUNT_DTYPE))
        raw = self.raw(with_carriers=False)
        return {"rows": raw["rows"].copy(), "row_begin": raw["row_begin"].copy(), "row_count": raw["row_count"].copy(),
                "columns": np.ctypeslib.as_array(cols, shape=(nc,)).copy(), "counts": counts, "state": state, "owner": owner,
                "keep_begin": keep_begin, "n_index": n_index, "rounds": rounds, "pvalues": getattr(self, "_clump_pvalues", None),
                "threshold": int(params[2]) / PRUNE_THRESHOLD_ONE, "threshold_q20": int(params[2]), "window": int(params[0]),
                "max_bp": int(params[1]), "p1": float(pb[0]), "p2": float(pb[1]), "p1_key": int(pkeys[0]), "p2_key": int(pkeys[1])}

    def ld_clump_device(self):
        """(state address, owner address, keep_begin address, n_index address, counts address, n_regions, n_rows, n_cols) of a
        clumping result as it lies in this GPU's memory: keep_begin[n_regions] verdict bytes and as many uint32 owners, n_regions + 1
        and n_regions uint64 words and n_rows count records of four uint32, complete when this returns and valid until the result
        is closed."""
        nq, a, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        pc, pb, pn, ps, po = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(self._lib.vs_result_ld_clump_device(self._h, C.byref(nq), C.byref(a), C.byref(c), C.byref(pc), C.byref(pb), C.byref(pn),
                                                   C.byref(ps), C.byref(po)), "vs_result_ld_clump_device")
        return (int(ps.value or 0), int(po.value or 0), int(pb.value or 0), int(pn.value or 0), int(pc.value or 0), int(nq.value),
                int(a.value), int(c.value))

    def region_clumps(self, q):
        """The clumps of region q of a clumping result: a list of ((pos, ref, alt), p, [member keys in table order]), one per index
        row, in priority order (p ascending, ties by table order)."""
        clumps, order = {}, []
        for k, line in enumerate(self.region_text(q).split("\n")[1:]):
            if not line:
                continue
            pos, ref, alt, _ac, p, state, index = line.split("\t")
            key = (int(pos), ref, alt)
            if state == "index":
                clumps.setdefault(key, [None, []])[0] = float(p)
                order.append((float(p), k, key))
            elif state == "clumped":
                ipos, iref, ialt = index.split(":")
                clumps.setdefault((int(ipos), iref, ialt), [None, []])[1].append(key)
        if not order:
            return []
        # (the text prints p with six digits: the order comes from the p-values the query took)
        got = self.ld_clump()
        a0, m, o = int(got["row_begin"][q]), int(got["row_count"][q]), int(got["keep_begin"][q])
        live = [a for a in range(a0, a0 + m) if got["state"][o + a - a0] != self.CLUMP_STATES["dropped"]]
        exact = pvalue_keys(got["pvalues"][live]) if got["pvalues"] is not None else None
        ranked = sorted(order, key=lambda t: ((int(exact[t[1]]) if exact is not None else t[0]), t[1]))
        pv = got["pvalues"]
        return [(key, float(pv[live[k]]) if pv is not None else clumps[key][0], clumps[key][1]) for _p, k, key in ranked]

    LDSCORE_STATES = {"scored": 1, "ineligible": 2, "dropped": 3}   # VS_LDSCORE_*
    LDSCORE_ONE = 1 << 32                                            # VS_LDSCORE_ONE: the integer value of r2 = 1

    def ld_scores(self):
        """An LD-score result (VariantStore.ld_scores) as numpy arrays, one entry per slot -- region q's slots are keep_begin[q] :
        keep_begin[q + 1], for the table rows row_begin[q] .. + row_count[q]: `sums` (uint64, the exact sum of floor(r2 * 2**32)
        over the rows summed), `n_pairs` (uint32, how many were summed, the row itself included), `state` (uint8: LDSCORE_STATES),
        `scores` (float64, sums / 2**32) and `scores_adj` (float64, the small-sample-adjusted score L - (n_pairs - L) / (n - 2):
        r2 - (1 - r2) / (n - 2) summed; NaN for n <= 2; formed here from the two exact outputs).  `keep_begin` (uint64[Q + 1]),
        `n_scored` (uint64[Q]), `counts` (structured as for allele_counts: the count record of every table row over the query's
        samples), `col_ids` (uint32[C], the sample ids), `params` (dict: window, max_bp, min_ac, max_ac), the table's `rows` and per
        region `row_begin` and `row_count`.  Copies, valid after the result is closed."""
        nq, a, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        params = (C.c_uint32 * 4)()
        cols = C.POINTER(C.c_uint32)()
        cnt = C.POINTER(_lib.AlleleCounts)()
        kb, ns, ps = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        pp = C.POINTER(C.c_uint32)()
        pst = C.POINTER(C.c_uint8)()
        _check(self._lib.vs_result_get_ld_scores(self._h, C.byref(nq), C.byref(a), C.byref(c), params, C.byref(cols), C.byref(cnt),
                                                 C.byref(kb), C.byref(ns), C.byref(ps), C.byref(pp), C.byref(pst)), "vs_result_get_ld_scores")
        q, na, nc = int(nq.value), int(a.value), int(c.value)
        keep_begin = np.ctypeslib.as_array(kb, shape=(q + 1,)).copy()
        n_scored = np.ctypeslib.as_array(ns, shape=(q,)).copy() if q else np.zeros(0, np.uint64)
        total = int(keep_begin[q])
        sums = np.ctypeslib.as_array(ps, shape=(total,)).copy() if total else np.zeros(0, np.uint64)
        n_pairs = np.ctypeslib.as_array(pp, shape=(total,)).copy() if total else np.zeros(0, np.uint32)
        state = np.ctypeslib.as_array(pst, shape=(total,)).copy() if total else np.zeros(0, np.uint8)
        counts = (np.ctypeslib.as_array(C.cast(cnt, C.POINTER(C.c_uint8)), shape=(na * 16,)).view(self.COUNT_DTYPE).copy() if na
                  else np.zeros(0, self.COUNT_DTYPE))
        scores = sums.astype(np.float64) / float(self.LDSCORE_ONE)
        if nc > 2:
            scores_adj = scores - (n_pairs.astype(np.float64) - scores) / float(nc - 2)
        else:
            scores_adj = np.full(total, np.nan)
        raw = self.raw(with_carriers=False)
        return {"rows": raw["rows"].copy(), "row_begin": raw["row_begin"].copy(), "row_count": raw["row_count"].copy(),
                "col_ids": np.ctypeslib.as_array(cols, shape=(nc,)).copy(), "counts": counts, "sums": sums, "n_pairs": n_pairs,
                "state": state, "scores": scores, "scores_adj": scores_adj, "keep_begin": keep_begin, "n_scored": n_scored,
                "params": {"window": int(params[0]), "max_bp": int(params[1]), "min_ac": int(params[2]), "max_ac": int(params[3])}}

    def region_ld_scores(self, q, scores=None):
        """Region q of an LD-score result: a dict of views into `scores` (ld_scores() of this result; taken now when None) --
        `sums`, `n_pairs`, `state`, `scores`, `scores_adj` of the region's slots, and `rows` and `counts` of its table rows."""
        got = self.ld_scores() if scores is None else scores
        q = int(q)
        if not 0 <= q < got["row_begin"].shape[0]:
            raise IndexError(f"region {q} of {got['row_begin'].shape[0]}")
        o, e = int(got["keep_begin"][q]), int(got["keep_begin"][q + 1])
        a0 = int(got["row_begin"][q])
        out = {k: got[k][o:e] for k in ("sums", "n_pairs", "state", "scores", "scores_adj")}
        out["rows"], out["counts"] = got["rows"][a0:a0 + e - o], got["counts"][a0:a0 + e - o]
        return out

    def ld_scores_device(self):
        """An LD-score result as it lies in this GPU's memory: a dict of the addresses `sums` (n_slots uint64), `n_pairs` (n_slots
        uint32), `state` (n_slots bytes), `keep_begin` (n_regions + 1 uint64), `n_scored` (n_regions uint64) and `counts` (n_rows
        records of four uint32), with `n_regions`, `n_rows`, `n_cols` and `n_slots`; complete when this returns and valid until
        the result is closed."""
        nq, a, c, s = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        pc, pb, pn, psum, pp, pst = (C.c_void_p() for _ in range(6))
        _check(self._lib.vs_result_ld_scores_device(self._h, C.byref(nq), C.byref(a), C.byref(c), C.byref(s), C.byref(pc), C.byref(pb),
                                                    C.byref(pn), C.byref(psum), C.byref(pp), C.byref(pst)), "vs_result_ld_scores_device")
        return {"sums": int(psum.value or 0), "n_pairs": int(pp.value or 0), "state": int(pst.value or 0), "keep_begin": int(pb.value or 0),
                "n_scored": int(pn.value or 0), "counts": int(pc.value or 0), "n_regions": int(nq.value), "n_rows": int(a.value),
                "n_cols": int(c.value), "n_slots": int(s.value)}

    def region_ld(self, q):
        """The pairs region q of an LD result reports: a list of dicts with `a` and `b` (each (pos, ref, alt)) and `value` (int under
        "dot", float under "r2") for every pair of the region's reported rows at most the window apart in the table."""
        lines = self.region_text(q).split("\n")
        dot = lines[0].endswith("Dot")
        out = []
        for line in lines[1:]:
            if not line:
                continue
            pa, ra, aa, pb, rb, ab, v = line.split("\t")
            out.append({"a": (int(pa), ra, aa), "b": (int(pb), rb, ab), "value": int(v) if dot else float(v)})
        return out

    def ld_matrix(self):
        """An LD-matrix result (VariantStore.ld_matrix) as numpy arrays: `cells` (flat; int32 dot products of the dosages under stat
        "dot", float32 squared correlations under "r2"), `block_begin` (uint64[Q + 1]: region q's block is the row_count[q] x
        row_count[q] cells from block_begin[q] on, row-major, for the table rows row_begin[q] .. + row_count[q]), `counts`
        (structured as for allele_counts: the count record of every table row over the query's samples), `col_ids` (uint32[C], the
        sample ids the statistics run over), `stat`, the table's `rows` and per region `row_begin` and `row_count`.  `cells`,
        `block_begin` and `counts` are views of memory the result owns, valid until it is closed; the rest are copies."""
        nq, a, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        st = C.c_uint32()
        cols = C.POINTER(C.c_uint32)()
        cnt = C.POINTER(_lib.AlleleCounts)()
        bb = C.POINTER(C.c_uint64)()
        p = C.c_void_p()
        _check(self._lib.vs_result_get_ld_matrix(self._h, C.byref(nq), C.byref(a), C.byref(c), C.byref(st), C.byref(cols), C.byref(cnt),
                                                 C.byref(bb), C.byref(p)), "vs_result_get_ld_matrix")
        q, na, nc = int(nq.value), int(a.value), int(c.value)
        stat = "r2" if st.value == self.LD_STATS["r2"] else "dot"
        dtype = np.float32 if stat == "r2" else np.int32
        block_begin = np.ctypeslib.as_array(bb, shape=(q + 1,))
        total = int(block_begin[q])
        cells = (np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(total * 4,)).view(dtype) if total else np.zeros(0, dtype))
        counts = (np.ctypeslib.as_array(C.cast(cnt, C.POINTER(C.c_uint8)), shape=(na * 16,)).view(self.COUNT_DTYPE) if na
                  else np.zeros(0, self.COUNT_DTYPE))
        raw = self.raw(with_carriers=False)
        return {"rows": raw["rows"].copy(), "row_begin": raw["row_begin"].copy(), "row_count": raw["row_count"].copy(),
                "col_ids": np.ctypeslib.as_array(cols, shape=(nc,)).copy(), "stat": stat, "counts": counts, "block_begin": block_begin,
                "cells": cells}

    def region_ld_matrix(self, q):
        """Region q's block of an LD-matrix result as an (m, m) array, m = the region's rows in the table: a view of the result's
        cells, not a copy, valid until the result is closed."""
        nq = C.c_uint64()
        st = C.c_uint32()
        bb = C.POINTER(C.c_uint64)()
        p = C.c_void_p()
        _check(self._lib.vs_result_get_ld_matrix(self._h, C.byref(nq), None, None, C.byref(st), None, None, C.byref(bb), C.byref(p)),
               "vs_result_get_ld_matrix")
        q = int(q)
        if not 0 <= q < int(nq.value):
            raise IndexError(f"region {q} of {int(nq.value)}")
        b0, b1 = int(bb[q]), int(bb[q + 1])
        m = math.isqrt(b1 - b0)
        dtype = np.float32 if st.value == self.LD_STATS["r2"] else np.int32
        if not m:
            return np.zeros((0, 0), dtype)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(b1 * 4,)).view(dtype)[b0:b1].reshape(m, m)

    def ld_matrix_device(self):
        """(cells address, block_begin address, counts address, n_regions, n_rows, n_cols, stat) of an LD-matrix result as it lies in
        this GPU's memory: the blocks' cells of 4 bytes (int32 under "dot", float32 under "r2"), n_regions + 1 uint64 offsets and
        n_rows count records of four uint32, complete when this returns and valid until the result is closed."""
        nq, a, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        st = C.c_uint32()
        pc, pb, pcells = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(self._lib.vs_result_ld_matrix_device(self._h, C.byref(nq), C.byref(a), C.byref(c), C.byref(st), C.byref(pc), C.byref(pb),
                                                    C.byref(pcells)), "vs_result_ld_matrix_device")
        return (int(pcells.value or 0), int(pb.value or 0), int(pc.value or 0), int(nq.value), int(a.value), int(c.value),
                "r2" if st.value == self.LD_STATS["r2"] else "dot")

    GRAM_STATS = {"dot": 0, "grm": 1}   # VS_GRAM_DOT, VS_GRAM_GRM

    def sample_gram(self):
        """A Gram result (VariantStore.sample_gram) as numpy arrays: `gram` ((n, n) int64: gram[i, j] = the sum over the table rows of
        the dosage products of columns i and j; symmetric, the diagonal the sum of squares), `grm` ((n, n) float64 under stat "grm":
        VanRaden's first GRM formed from exact integers; None under "dot"), `col_weighted` (int64[n]: s_i = the sum of a row's
        alt_alleles over the samples times the row's dosage in column i), `C` and `H` (Python ints: the sums of ac^2 and of
        ac (2 n - ac) over the rows), `counts` (structured as for allele_counts: the count record of every table row over the
        query's samples), `columns` (uint32[n], the sample ids), `stat`, the table's `rows` and per region `row_begin` and
        `row_count`.  Copies, valid after the result is closed."""
        a, c = C.c_uint64(), C.c_uint64()
        st = C.c_uint32()
        cols = C.POINTER(C.c_uint32)()
        cnt = C.POINTER(_lib.AlleleCounts)()
        pg, ps = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)()
        pd = C.POINTER(C.c_double)()
        cc, hh = C.c_int64(), C.c_int64()
        _check(self._lib.vs_result_get_sample_gram(self._h, C.byref(a), C.byref(c), C.byref(st), C.byref(cols), C.byref(cnt), C.byref(pg),
                                                   C.byref(pd), C.byref(ps), C.byref(cc), C.byref(hh)), "vs_result_get_sample_gram")
        na, nc = int(a.value), int(c.value)
        stat = "grm" if st.value == self.GRAM_STATS["grm"] else "dot"
        gram = np.ctypeslib.as_array(pg, shape=(nc, nc)).copy()
        grm = np.ctypeslib.as_array(pd, shape=(nc, nc)).copy() if stat == "grm" else None
        colw = np.ctypeslib.as_array(ps, shape=(nc,)).copy()
        if na:
            counts = np.ctypeslib.as_array(C.cast(cnt, C.POINTER(C.c_uint8)), shape=(na * 16,)).view(self.COUNT_DTYPE).copy()
        else:
            counts = np.zeros(0, self.COUNT_DTYPE)
        raw = self.raw(with_carriers=False)
        return {"rows": raw["rows"].copy(), "row_begin": raw["row_begin"].copy(), "row_count": raw["row_count"].copy(),
                "columns": np.ctypeslib.as_array(cols, shape=(nc,)).copy(), "stat": stat, "counts": counts, "gram": gram, "grm": grm,
                "col_weighted": colw, "C": int(cc.value), "H": int(hh.value)}

    def sample_gram_device(self):
        """(gram address, grm address, col_weighted address, counts address, n_rows, n_cols, stat) of a Gram result as it lies in
        this GPU's memory: n_cols x n_cols int64, n_cols x n_cols float64 (0 under "dot"), n_cols int64 with C and H right behind
        them, n_rows count records of four uint32; complete when this returns and valid until the result is closed."""
        a, c = C.c_uint64(), C.c_uint64()
        st = C.c_uint32()
        pc, pg, pd, ps = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(self._lib.vs_result_sample_gram_device(self._h, C.byref(a), C.byref(c), C.byref(st), C.byref(pc), C.byref(pg), C.byref(pd),
                                                      C.byref(ps)), "vs_result_sample_gram_device")
        return (int(pg.value or 0), int(pd.value or 0), int(ps.value or 0), int(pc.value or 0), int(a.value), int(c.value),
                "grm" if st.value == self.GRAM_STATS["grm"] else "dot")

    IBS_STATS = {"counts": 0, "king": 1}   # VS_IBS_COUNTS, VS_IBS_KING

    def sample_ibs(self):
        """An IBS result (VariantStore.sample_ibs) as numpy arrays.  (n, n) int64, symmetric, counted over the table rows the
        duplicate rule kept: `het_het` (both heterozygous), `hom_hom` (both hom-alt), `carrier_both` (both carriers), `ibs0`
        (opposite homozygotes), `ibs2` (equal dosage, 0/0 included) and `ibs1` = n_used - ibs0 - ibs2, derived here; `n_used` (a
        Python int: the table's rows minus those the duplicate rule dropped), `het` (int64[n]: the diagonal of het_het, a sample's
        heterozygous calls), `king` ((n, n) float64 under stat "king": (het_het - 2 ibs0) / (het_i + het_j), 0.0 where the
        denominator is 0; None under "counts"), `counts` (structured as for allele_counts: the count record of every table row over
        the query's samples), `columns` (uint32[n], the sample ids), `stat`, the table's `rows` and per region `row_begin` and
        `row_count`.  Copies, valid after the result is closed."""
        a, c = C.c_uint64(), C.c_uint64()
        st = C.c_uint32()
        cols = C.POINTER(C.c_uint32)()
        cnt = C.POINTER(_lib.AlleleCounts)()
        pm = [C.POINTER(C.c_int64)() for _ in range(5)]
        pk = C.POINTER(C.c_double)()
        nu = C.c_int64()
        _check(self._lib.vs_result_get_sample_ibs(self._h, C.byref(a), C.byref(c), C.byref(st), C.byref(cols), C.byref(cnt), C.byref(pm[0]),
                                                  C.byref(pm[1]), C.byref(pm[2]), C.byref(pm[3]), C.byref(pm[4]), C.byref(pk), C.byref(nu)),
               "vs_result_get_sample_ibs")
        na, nc = int(a.value), int(c.value)
        stat = "king" if st.value == self.IBS_STATS["king"] else "counts"
        hh, aa, cb, ibs0, ibs2 = (np.ctypeslib.as_array(p, shape=(nc, nc)).copy() for p in pm)
        king = np.ctypeslib.as_array(pk, shape=(nc, nc)).copy() if stat == "king" else None
        if na:
            counts = np.ctypeslib.as_array(C.cast(cnt, C.POINTER(C.c_uint8)), shape=(na * 16,)).view(self.COUNT_DTYPE).copy()
        else:
            counts = np.zeros(0, self.COUNT_DTYPE)
        raw = self.raw(with_carriers=False)
        n_used = int(nu.value)
        return {"rows": raw["rows"].copy(), "row_begin": raw["row_begin"].copy(), "row_count": raw["row_count"].copy(),
                "columns": np.ctypeslib.as_array(cols, shape=(nc,)).copy(), "stat": stat, "counts": counts, "het_het": hh, "hom_hom": aa,
                "carrier_both": cb, "ibs0": ibs0, "ibs1": n_used - ibs0 - ibs2, "ibs2": ibs2, "n_used": n_used, "het": np.diagonal(hh).copy(),
                "king": king}

    def sample_ibs_device(self):
        """(matrices address, king address, counts address, n_rows, n_cols, stat) of an IBS result as it lies in this GPU's memory:
        five n_cols x n_cols int64 matrices one behind the other -- het_het, hom_hom, carrier_both, ibs0, ibs2 -- with n_used (one
        int64) right behind them, n_cols x n_cols float64 (0 under "counts"), n_rows count records of four uint32; complete when
        this returns and valid until the result is closed."""
        a, c = C.c_uint64(), C.c_uint64()
        st = C.c_uint32()
        pc, pm, pk = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(self._lib.vs_result_sample_ibs_device(self._h, C.byref(a), C.byref(c), C.byref(st), C.byref(pc), C.byref(pm), C.byref(pk)),
               "vs_result_sample_ibs_device")
        return (int(pm.value or 0), int(pk.value or 0), int(pc.value or 0), int(a.value), int(c.value),
                "king" if st.value == self.IBS_STATS["king"] else "counts")

    TRIO_DTYPE = np.dtype([("errors", "<u4"), ("denovo", "<u4"), ("transmitted", "<u4"), ("untransmitted", "<u4")])   # vs_trio_counts

    def trio_scan(self):
        """A trio result (VariantStore.trio_scan) as numpy arrays.  `row_stats` (structured: errors, denovo, transmitted,
        untransmitted, uint32; row_stats[i] belongs to rows[i] and sums over all trios), `trio_stats` (the same per trio, summed
        over every table row once), `n_used` (a Python int: the table's rows minus those the duplicate rule dropped), `tdt_chi2`
        (float64 per row, (T - U)**2 / (T + U) of the row's transmitted and untransmitted counts: each integer converted once, one
        multiplication, one division; NaN where T + U == 0), `error_rate` (float64 per trio, errors / n_used; NaN at n_used == 0),
        `columns` (uint32[n], the distinct member ids, ascending), `trio_cols` ((n_trios, 3) uint32: the columns of child, father,
        mother), `trio_ids` (the same as sample ids), `counts` (structured as for allele_counts: the count record of every table row
        over the members), the table's `rows` and per region `row_begin` and `row_count`.  Copies, valid after the result is
        closed."""
        a, c, t, nu = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        cols, tc = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
        cnt = C.POINTER(_lib.AlleleCounts)()
        pr, pt = C.c_void_p(), C.c_void_p()
        _check(self._lib.vs_result_get_trio_scan(self._h, C.byref(a), C.byref(c), C.byref(t), C.byref(nu), C.byref(cols), C.byref(tc),
                                                 C.byref(cnt), C.byref(pr), C.byref(pt)), "vs_result_get_trio_scan")
        na, nc, nt, n_used = int(a.value), int(c.value), int(t.value), int(nu.value)

        def records(p, n):
            if not n:
                return np.zeros(0, self.TRIO_DTYPE)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n * 16,)).view(self.TRIO_DTYPE).copy()
        row_stats, trio_stats = records(pr, na), records(pt, nt)
        counts = records(cnt, na).view(self.COUNT_DTYPE)
        columns = np.ctypeslib.as_array(cols, shape=(nc,)).copy()
        trio_cols = np.ctypeslib.as_array(tc, shape=(nt, 3)).copy()
        raw = self.raw(with_carriers=False)
        return {"rows": raw["rows"].copy(), "row_begin": raw["row_begin"].copy(), "row_count": raw["row_count"].copy(),
                "columns": columns, "trio_cols": trio_cols, "trio_ids": columns[trio_cols], "counts": counts, "row_stats": row_stats,
                "trio_stats": trio_stats, "n_used": n_used, "tdt_chi2": trio_tdt_chi2(row_stats), "error_rate": trio_error_rate(trio_stats, n_used)}

    def region_trio_stats(self, q, scan=None):
        """Region q of a trio result: a dict of views into `scan` (trio_scan() of this result; taken now when None) -- `row_stats`,
        `tdt_chi2`, `rows` and `counts` of the region's table rows."""
        got = self.trio_scan() if scan is None else scan
        q = int(q)
        if not 0 <= q < got["row_begin"].shape[0]:
            raise IndexError(f"region {q} of {got['row_begin'].shape[0]}")
        a0, m = int(got["row_begin"][q]), int(got["row_count"][q])
        return {k: got[k][a0:a0 + m] for k in ("row_stats", "tdt_chi2", "rows", "counts")}

    def trio_scan_device(self):
        """A trio result as it lies in this GPU's memory: a dict of the addresses `rows` (n_rows records of four uint32), `trios`
        (n_trios records, right behind them), `n_used` (one uint64) and `counts` (n_rows records of four uint32), with `n_rows`,
        `n_cols` and `n_trios`; complete when this returns and valid until the result is closed."""
        a, c, t = C.c_uint64(), C.c_uint64(), C.c_uint64()
        pc, pr, pt, pu = (C.c_void_p() for _ in range(4))
        _check(self._lib.vs_result_trio_scan_device(self._h, C.byref(a), C.byref(c), C.byref(t), C.byref(pc), C.byref(pr), C.byref(pt),
                                                    C.byref(pu)), "vs_result_trio_scan_device")
        return {"rows": int(pr.value or 0), "trios": int(pt.value or 0), "n_used": int(pu.value or 0), "counts": int(pc.value or 0),
                "n_rows": int(a.value), "n_cols": int(c.value), "n_trios": int(t.value)}

    ROH_SUMMARY_DTYPE = np.dtype([("n_segments", "<u4"), ("seg_sites", "<u4"), ("total_bp", "<u8"), ("longest_bp", "<u4"),
                                  ("longest_sites", "<u4"), ("seg_hets", "<u4"), ("n_het", "<u4")])   # vs_roh_summary
    ROH_SEGMENT_DTYPE = np.dtype([("region", "<u4"), ("column", "<u4"), ("pos_first", "<u4"), ("pos_last", "<u4"), ("row_first", "<u4"),
                                  ("row_last", "<u4"), ("n_sites", "<u4"), ("n_het", "<u4")])   # vs_roh_segment

    def roh(self, lengths=None):
        """A ROH result (VariantStore.roh) as numpy arrays.  `summary` (structured, shape (Q, S): n_segments, seg_sites, total_bp,
        longest_bp, longest_sites, seg_hets, n_het -- summary[q, c] belongs to region q and columns[c]), `n_sites` (uint32[Q]: the
        sites of every region), `segments` (structured: region, column, pos_first, pos_last, row_first, row_last, n_sites, n_het;
        ordered by region, column, occurrence) and `seg_begin` (uint64[Q S + 1]: cell (q, c) owns segments[seg_begin[q S + c] ..
        seg_begin[q S + c + 1])) -- both None when the batch ran with segments=False --, `columns` (uint32[S], the sample ids,
        ascending), `params` (the batch's own, a dict), `counts` (structured as for allele_counts: the count record of every
        table row over the columns), the table's `rows` and per region `row_begin` and `row_count`; and, in float64 from the
        integers only (roh_derived), `kb` = total_bp / 1000, `kb_avg` (NaN without segments) and -- with `lengths`, one per
        region -- `froh` = total_bp / lengths[q].  Copies, valid after the result is closed."""
        nq, nc, na, ns = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        prm = _lib.RohParams()
        cols, nsites, sb = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint64)()
        cnt = C.POINTER(_lib.AlleleCounts)()
        psum, pseg = C.c_void_p(), C.c_void_p()
        _check(self._lib.vs_result_get_roh(self._h, C.byref(nq), C.byref(nc), C.byref(na), C.byref(ns), C.byref(prm), C.byref(cols), C.byref(cnt),
                                           C.byref(psum), C.byref(nsites), C.byref(sb), C.byref(pseg)), "vs_result_get_roh")
        Q, S, A, N = int(nq.value), int(nc.value), int(na.value), int(ns.value)

        def records(p, n, dtype):
            if not n:
                return np.zeros(0, dtype)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n * dtype.itemsize,)).view(dtype).copy()
        summary = records(psum, Q * S, self.ROH_SUMMARY_DTYPE).reshape(Q, S)
        counts = records(cnt, A, self.COUNT_DTYPE)
        has_segments = bool(prm.segments)
        segments = records(pseg, N, self.ROH_SEGMENT_DTYPE) if has_segments else None
        seg_begin = np.ctypeslib.as_array(sb, shape=(Q * S + 1,)).copy() if has_segments else None
        raw = self.raw(with_carriers=False)
        out = {"rows": raw["rows"].copy(), "row_begin": raw["row_begin"].copy(), "row_count": raw["row_count"].copy(),
               "columns": np.ctypeslib.as_array(cols, shape=(S,)).copy(), "counts": counts, "summary": summary,
               "n_sites": np.ctypeslib.as_array(nsites, shape=(Q,)).copy(), "segments": segments, "seg_begin": seg_begin,
               "params": {k: int(getattr(prm, k)) for k, _ in _lib.RohParams._fields_}}
        out.update(roh_derived(summary, lengths))
        return out

    def region_roh(self, q, roh=None):
        """Region q of a ROH result: a dict of views into `roh` (roh() of this result; taken now when None) -- `summary` (the
        region's row, one record per column), `segments` (the region's, None without segments), `n_sites`, `kb`, `kb_avg`."""
        got = self.roh() if roh is None else roh
        q = int(q)
        Q, S = got["summary"].shape
        if not 0 <= q < Q:
            raise IndexError(f"region {q} of {Q}")
        seg = None
        if got["segments"] is not None:
            seg = got["segments"][int(got["seg_begin"][q * S]):int(got["seg_begin"][(q + 1) * S])]
        return {"summary": got["summary"][q], "segments": seg, "n_sites": int(got["n_sites"][q]), "kb": got["kb"][q], "kb_avg": got["kb_avg"][q]}

    def roh_device(self):
        """A ROH result as it lies in this GPU's memory: a dict of the addresses `summary` (n_regions x n_cols records of 32
        bytes), `n_sites` (n_regions uint32), `seg_begin` (n_regions x n_cols + 1 uint64) and `segments` (n_segments records of 32
        bytes; both 0 without segments) and `counts` (n_rows records of four uint32), with `n_regions`, `n_cols`, `n_rows` and
        `n_segments`; complete when this returns and valid until the result is closed."""
        nq, nc, na, ns = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        pc, psum, pn, pb, pseg = (C.c_void_p() for _ in range(5))
        _check(self._lib.vs_result_roh_device(self._h, C.byref(nq), C.byref(nc), C.byref(na), C.byref(ns), C.byref(pc), C.byref(psum), C.byref(pn),
                                              C.byref(pb), C.byref(pseg)), "vs_result_roh_device")
        return {"summary": int(psum.value or 0), "n_sites": int(pn.value or 0), "seg_begin": int(pb.value or 0), "segments": int(pseg.value or 0),
                "counts": int(pc.value or 0), "n_regions": int(nq.value), "n_cols": int(nc.value), "n_rows": int(na.value), "n_segments": int(ns.value)}

    def region_variants(self, q) -> List[Variant]:
        out = []
        for line in self.region_text(q).split("\n")[1:]:
            if not line:
                continue
            pos, ref, alt, samples = line.split("\t")
            pairs = []
            for tok in samples.split(" "):
                if tok:
                    name, gt = tok[:-1].rsplit("(", 1)
                    pairs.append((name, gt))
            out.append(Variant(int(pos), ref, alt, pairs))
        return out


class Comm:
    """The hit-list collective of one rank (vs_comm_*: RCCL called directly by the engine, no torch.distributed).
    `Comm.unique_id()` on rank 0, the 128 bytes handed to every rank by whatever means the host program has, then
    `Comm(store, rank, world, uid)` on every rank."""

    def __init__(self, store, rank, world, uid):
        self._lib = store._lib
        self._store = store     # (keeps the index handle alive)
        self.rank, self.world = int(rank), int(world)
        buf = C.create_string_buffer(bytes(uid), 128)
        h = C.c_void_p()
        _check(self._lib.vs_comm_init(store._h, self.rank, self.world, C.cast(buf, C.c_void_p), C.byref(h)), "vs_comm_init")
        self._h = h

    @staticmethod
    def unique_id():
        lib = _lib.load()
        buf = C.create_string_buffer(128)
        _check(lib.vs_comm_unique_id(C.cast(buf, C.c_void_p)), "vs_comm_unique_id")
        return bytes(buf.raw)

    def allgather_regions(self, result, region_base, max_count, device_dst, async_op=False):
        """Pack `result`'s per-region records and all-gather them, padded to max_count per rank, into device memory at
        `device_dst` (world x max_count x 32 bytes; rank k's records start at record k * max_count)."""
        _check(self._lib.vs_comm_allgather_regions(self._h, result._h, int(region_base), int(max_count), C.c_void_p(int(device_dst)),
                                                   1 if async_op else 0), "vs_comm_allgather_regions")

    def wait(self):
        _check(self._lib.vs_comm_wait(self._h), "vs_comm_wait")

    def info(self):
        """(rank, world, ranks RCCL reports for the communicator: ncclCommCount)."""
        r, w, n = C.c_int(), C.c_int(), C.c_int()
        _check(self._lib.vs_comm_info(self._h, C.byref(r), C.byref(w), C.byref(n)), "vs_comm_info")
        return r.value, w.value, n.value

    def close(self):
        if self._h:
            self._lib.vs_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VariantStore:
    """An opened index: the reference's (VariantGraph, Index) pair on one GPU."""

    def __init__(self, handle, stats=None):
        self._h = handle
        self._lib = _lib.load()
        # same symbol, raw-address prototype: passing a numpy buffer's address as an int skips ctypes' pointer objects
        self._q6 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)(("vs_query_var_in_ref", self._lib))
        self.construct_stats = stats

    # ---- constructors -------------------------------------------------------
    @classmethod
    def from_vcf(cls, fasta, vcf, device=0):
        lib = _lib.load()
        h = C.c_void_p()
        st = ConstructStats()
        _check(lib.vs_index_from_vcf(str(fasta).encode(), str(vcf).encode(), device, C.byref(st), C.byref(h)),
               "vs_index_from_vcf")
        return cls(h, st)

    @classmethod
    def synthetic(cls, device=0, **kw):
        lib = _lib.load()
        p = SynthParams(ref_length=kw.get("ref_length", 1_000_000), num_variants=kw.get("num_variants", 10_000),
                        num_samples=kw.get("num_samples", 100), seed=kw.get("seed", 1),
                        first_pos=kw.get("first_pos", 1000), frac_ins=kw.get("frac_ins", 0.0),
                        frac_del=kw.get("frac_del", 0.0), frac_multi=kw.get("frac_multi", 0.0),
                        max_indel=kw.get("max_indel", 6), af_exponent=kw.get("af_exponent", 3.0),
                        sample_coordinates=1 if kw.get("sample_coordinates") else 0,
                        max_af=float(kw.get("max_af", 0.0)))
        h = C.c_void_p()
        st = ConstructStats()
        _check(lib.vs_index_synthetic(C.byref(p), device, C.byref(st), C.byref(h)), "vs_index_synthetic")
        return cls(h, st)

    @classmethod
    def open(cls, prefix, device=0):
        lib = _lib.load()
        h = C.c_void_p()
        _check(lib.vs_index_open(str(prefix).encode(), device, C.byref(h)), "vs_index_open")
        return cls(h)

    def save(self, prefix):
        _check(self._lib.vs_index_save(self._h, str(prefix).encode()), "vs_index_save")

    def close(self):
        if self._h:
            self._lib.vs_index_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- inspection ---------------------------------------------------------
    def info(self) -> IndexInfo:
        info = IndexInfo()
        _check(self._lib.vs_index_get_info(self._h, C.byref(info)), "vs_index_get_info")
        return info

    def chr(self):
        return self._lib.vs_index_chr(self._h).decode()

    def sample_id(self, name):
        sid = C.c_uint32()
        _check(self._lib.vs_index_sample_id(self._h, name.encode(), C.byref(sid)), "vs_index_sample_id")
        return int(sid.value)

    def sample_name(self, sid):
        s = self._lib.vs_index_sample_name(self._h, sid)
        return s.decode() if s is not None else None

    def export_plain(self, path):
        _check(self._lib.vs_index_export_plain(self._h, str(path).encode()), "vs_index_export_plain")

    def out_neighbors(self, v):
        buf = (C.c_uint32 * 4096)()
        n = self._lib.vs_index_out_neighbors(self._h, v, buf, 4096)
        if n < 0:
            raise IndexError(v)
        return [int(buf[i]) for i in range(min(n, 4096))]

    def last_timing(self) -> Timing:
        t = Timing()
        _check(self._lib.vs_index_last_timing(self._h, C.byref(t)), "vs_index_last_timing")
        return t

    def set_option(self, key, value):
        """Test / tuning switches of this handle (include/variantstore_hip.h: vs_index_set_option)."""
        _check(self._lib.vs_index_set_option(self._h, key.encode(), int(value)), "vs_index_set_option")

    # ---- queries ------------------------------------------------------------
    def find(self, positions: Sequence[int]):
        """Index::find for a batch of positions (index.h:119-133)."""
        pos = np.ascontiguousarray(np.asarray(positions, dtype=np.uint64))
        out = np.zeros(pos.shape[0], dtype=np.uint32)
        _check(self._lib.vs_index_find(self._h, pos.ctypes.data_as(C.POINTER(C.c_uint64)), pos.shape[0],
                                       out.ctypes.data_as(C.POINTER(C.c_uint32))), "vs_index_find")
        return out

    def get_var_in_ref(self, regions) -> QueryResult:
        """Query type 6 over a batch of (pos_x, pos_y) regions (query.h:736-784)."""
        # (this is the call whose single-region latency the bench reports: a ready uint64 array is passed on as it is,
        #  without the ctypes pointer objects of the general helper)
        if (type(regions) is np.ndarray and regions.dtype == np.uint64 and regions.flags.c_contiguous and regions.ndim == 2
                and regions.shape[1] == 2):
            arr = regions
        else:
            arr = np.ascontiguousarray(np.asarray(regions, dtype=np.uint64).reshape(-1, 2))
        h = C.c_void_p()
        rc = self._q6(self._h, arr.__array_interface__["data"][0], arr.shape[0], C.byref(h))
        if rc != 0:
            raise VariantStoreError(rc, "vs_query_var_in_ref")
        return QueryResult(self, h)

    def stream_var_in_ref(self, regions, chunk_regions, on_chunk, with_carriers=True):
        """Query type 6 with delivery (vs_query_var_in_ref_stream): `on_chunk(first_region, raw)` is called per chunk with the
        ctypes ResultRaw of that chunk (valid during the call) while the next chunk is being computed."""
        arr, ptr, n = _regions_array(regions)

        def tramp(_user, first, raw):
            on_chunk(int(first), raw.contents)
            return 0

        cb = _lib.CHUNK_FN(tramp)
        _check(self._lib.vs_query_var_in_ref_stream(self._h, ptr, n, int(chunk_regions), 1 if with_carriers else 0,
                                                    C.cast(cb, C.c_void_p), None), "vs_query_var_in_ref_stream")

    def get_var_in_ref_device(self, device_ptr, n) -> QueryResult:
        """Query type 6 over n (pos_x, pos_y) uint64 pairs that already live in this GPU's memory (`device_ptr`: an
        address, e.g. `tensor.data_ptr()` of a contiguous int64/uint64 CUDA tensor of shape (n, 2))."""
        h = C.c_void_p()
        _check(self._lib.vs_query_var_in_ref_device(self._h, C.c_void_p(int(device_ptr)), int(n), C.byref(h)),
               "vs_query_var_in_ref_device")
        return QueryResult(self, h)

    def expand_site_ranges(self, device_ptr, n) -> QueryResult:
        """The receiving side of the hit-list collective: n compact region records (QueryResult.pack_regions_into, own or
        gathered from ranks holding the same index) in this GPU's memory -> the full type-6 result they describe."""
        h = C.c_void_p()
        _check(self._lib.vs_query_expand_site_ranges(self._h, C.c_void_p(int(device_ptr)), int(n), C.byref(h)),
               "vs_query_expand_site_ranges")
        return QueryResult(self, h)

    def allele_counts(self, regions, samples=None) -> QueryResult:
        """Allele counts over regions (vs_query_allele_counts): the rows type 6 reports, each with carriers, alt_alleles,
        hom_alt and phased over the samples in `samples` (names or ids, taken as a set; None: the whole cohort).  `regions`:
        (pos_x, pos_y) pairs as a list or an array, or a DeviceArray of them in this GPU's memory.  Read the result with
        QueryResult.allele_counts / region_counts / region_text."""
        arr, ptr, n = _regions_array(regions)
        h = C.c_void_p()
        if samples is None:
            ids, ids_ptr, n_ids = None, None, 0
            if getattr(self, "_cohort", None) is None:   # (vs_index_get_info asks the device for its free memory: once per handle)
                self._cohort = self.info().num_samples - 1
            subset = self._cohort
        else:
            if isinstance(samples, (str, bytes)):
                samples = [samples]
            ids = np.ascontiguousarray([self.sample_id(x) if isinstance(x, str) else int(x) for x in samples], dtype=np.uint32)
            ids_ptr, n_ids = ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.shape[0]
            if n_ids == 0:   # (the C ABI's NULL-or-non-empty rule: an empty list is not the whole cohort)
                ids_ptr = (C.c_uint32 * 1)()
            subset = len(set(ids.tolist()))
        _check(self._lib.vs_query_allele_counts(self._h, ptr, n, ids_ptr, n_ids, C.byref(h)), "vs_query_allele_counts")
        res = QueryResult(self, h)
        res.subset_size = subset
        return res

    def group_counts(self, regions, groups) -> QueryResult:
        """Grouped allele counts over regions (vs_query_group_counts): the rows type 6 reports, each with carriers, alt_alleles,
        hom_alt and phased over every one of several disjoint groups of samples -- one pass instead of one allele_counts call per
        group.  `groups`: a dict name -> iterable of samples (names or ids; dict order is group order), or a sequence of such
        iterables, named "0", "1", ...  A sample that is listed nowhere belongs to no group; a group may be empty.  `regions` as
        for allele_counts.  Read the result with QueryResult.group_counts / region_group_counts / group_counts_device / region_text."""
        names, members, ids, gof = self._groups_arg(groups)
        arr, ptr, n = _regions_array(regions)
        name_arr = (C.c_char_p * len(names))(*[s.encode() for s in names]) if names is not None else None
        h = C.c_void_p()
        _check(self._lib.vs_query_group_counts(self._h, ptr, n, ids.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               gof.ctypes.data_as(C.POINTER(C.c_uint32)), ids.shape[0], len(members), name_arr,
                                               C.byref(h)), "vs_query_group_counts")
        res = QueryResult(self, h)
        res.group_names = names if names is not None else [str(i) for i in range(len(members))]
        return res

    def _groups_arg(self, groups):
        """(names or None, members, ids, group_of) of a grouped query's `groups`: a dict name -> samples or a sequence of sample lists."""
        if isinstance(groups, dict):
            names, members = [str(k) for k in groups], list(groups.values())
        else:
            members = list(groups)
            names = None
        ids, gof = [], []
        for g, m in enumerate(members):
            if isinstance(m, (str, bytes)):
                m = [m]
            for x in m:
                ids.append(self.sample_id(x) if isinstance(x, str) else int(x))
                gof.append(g)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        gof = np.ascontiguousarray(gof, dtype=np.uint32)
        return names, members, ids, gof

    def window_stats(self, regions, groups=None, pairs=True) -> QueryResult:
        """Windowed diversity statistics over regions (vs_query_window_stats): per region and group the exact integers nucleotide
        diversity pi, segregating sites, Watterson's theta, Tajima's D, private alleles and fixed sites are formed from, and with
        `pairs` per pair of groups those of dxy, Hudson's Fst, shared segregating sites and fixed differences -- the reduction of
        group_counts' records done on the GPU, a few dozen bytes per window and group instead of 16 bytes per row and group.
        `groups` as for group_counts, or None: the whole cohort as one group.  `regions` as for allele_counts (a list, an array or
        a DeviceArray).  Read the result with QueryResult.window_stats (which also forms pi, theta_w, tajima_d, het_obs, dxy and
        fst_hudson) / region_window_stats / window_stats_device / region_text."""
        arr, ptr, n = _regions_array(regions)
        h = C.c_void_p()
        if groups is None:
            names, n_groups, ids_ptr, gof_ptr, n_ids, name_arr = None, 1, None, None, 0, None
        else:
            names, members, ids, gof = self._groups_arg(groups)
            n_groups, n_ids = len(members), ids.shape[0]
            ids_ptr, gof_ptr = ids.ctypes.data_as(C.POINTER(C.c_uint32)), gof.ctypes.data_as(C.POINTER(C.c_uint32))
            name_arr = (C.c_char_p * len(names))(*[s.encode() for s in names]) if names is not None else None
        _check(self._lib.vs_query_window_stats(self._h, ptr, n, ids_ptr, gof_ptr, n_ids, n_groups, name_arr, 1 if pairs else 0, C.byref(h)),
               "vs_query_window_stats")
        res = QueryResult(self, h)
        res.group_names = names if names is not None else [str(i) for i in range(n_groups)]
        return res

    def _sample_set(self, samples):
        """(the id array or None, its pointer, its length) of a column request's `samples`: names or ids, None for the whole cohort."""
        if samples is None:
            return None, None, 0
        if isinstance(samples, (str, bytes)):
            samples = [samples]
        ids = np.ascontiguousarray([self.sample_id(x) if isinstance(x, str) else int(x) for x in samples], dtype=np.uint32)
        ids_ptr, n_ids = ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.shape[0]
        if n_ids == 0:   # (the C ABI's NULL-or-non-empty rule: an empty list is not the whole cohort)
            ids_ptr = (C.c_uint32 * 1)()
        return ids, ids_ptr, n_ids

    def sample_burden(self, regions, samples=None, min_ac=0, max_ac=None) -> QueryResult:
        """Per-sample burden over regions (vs_query_sample_burden): a regions x samples matrix -- for every region and every
        sample of `samples` (names or ids, taken as a set; None: the whole cohort) the variants of the region the sample
        carries, with alt_alleles, hom_alt and phased.  Only the rows whose alternate-allele count over the same samples lies
        in [min_ac, max_ac] count (max_ac None: no upper limit).  `regions` as for allele_counts.  Read the result with
        QueryResult.sample_burden / sample_burden_device / region_text."""
        arr, ptr, n = _regions_array(regions)
        h = C.c_void_p()
        ids, ids_ptr, n_ids = self._sample_set(samples)   # (ids keeps the array alive over the call)
        _check(self._lib.vs_query_sample_burden(self._h, ptr, n, ids_ptr, n_ids, int(min_ac),
                                                0xFFFFFFFF if max_ac is None else int(max_ac), C.byref(h)), "vs_query_sample_burden")
        return QueryResult(self, h)

    def genotype_matrix(self, regions, samples=None) -> QueryResult:
        """The genotype matrix over regions (vs_query_genotype_matrix): one row per row of the variant table a type-6 batch over
        `regions` produces, one column per sample of `samples` (names or ids, taken as a set; None: the whole cohort), a byte
        per call.  `regions` as for allele_counts.  Read the result with QueryResult.genotype_matrix /
        genotype_matrix_device / region_genotypes / region_text."""
        arr, ptr, n = _regions_array(regions)
        h = C.c_void_p()
        ids, ids_ptr, n_ids = self._sample_set(samples)   # (ids keeps the array alive over the call)
        _check(self._lib.vs_query_genotype_matrix(self._h, ptr, n, ids_ptr, n_ids, C.byref(h)), "vs_query_genotype_matrix")
        return QueryResult(self, h)

    def ld_band(self, regions, samples=None, window=64, stat="r2") -> QueryResult:
        """Banded LD over regions (vs_query_ld_band): every row of the variant table a type-6 batch over `regions` produces against
        the next `window` rows (1 .. 256), over the dosages of `samples` (names or ids, taken as a set; None: the whole cohort).
        `stat`: "r2" (squared dosage correlation, float32) or "dot" (sum of dosage products, int32, exact).  `regions` as for
        allele_counts.  Read the result with QueryResult.ld_band / ld_band_device / region_ld / region_text."""
        arr, ptr, n = _regions_array(regions)
        h = C.c_void_p()
        if isinstance(stat, str):
            if stat.lower() not in QueryResult.LD_STATS:
                raise ValueError(f"stat {stat!r}: 'r2' or 'dot'")
            stat = QueryResult.LD_STATS[stat.lower()]
        ids, ids_ptr, n_ids = self._sample_set(samples)   # (ids keeps the array alive over the call)
        window = int(window)
        if not 0 <= window <= 0xFFFFFFFF:   # (ctypes would wrap it: 0 is refused by the C ABI like any window outside 1 .. 256)
            window = 0
        _check(self._lib.vs_query_ld_band(self._h, ptr, n, ids_ptr, n_ids, window, int(stat) & 0xFFFFFFFF, C.byref(h)),
               "vs_query_ld_band")
        return QueryResult(self, h)

    def ld_prune(self, regions, samples=None, window=64, r2=0.2, max_bp=0, min_ac=0, max_ac=None) -> QueryResult:
        """LD pruning over regions (vs_query_ld_prune): for every region the forward greedy pruning of its table rows, in table
        order -- a row is kept when it is polymorphic over `samples` (names or ids, taken as a set; None: the whole cohort), its
        alternate-allele count lies in [min_ac, max_ac] (max_ac None: no upper limit), and no kept row among the `window`
        (1 .. 256) rows before it (at most `max_bp` positions away; 0: no limit) has a squared dosage correlation with it above
        `r2`.  `r2` is quantised to T = quantise_r2(r2) and r2 > T / 2**20 is decided in exact integers: the verdicts do not
        depend on rounding.  Regions are independent.  `regions` as for allele_counts.  Read the result with
        QueryResult.ld_prune / ld_prune_device / region_kept / region_text."""
        threshold = quantise_r2(r2)
        arr, ptr, n = _regions_array(regions)
        h = C.c_void_p()
        ids, ids_ptr, n_ids = self._sample_set(samples)   # (ids keeps the array alive over the call)
        window = int(window)
        if not 0 <= window <= 0xFFFFFFFF:   # (ctypes would wrap it: 0 is refused by the C ABI like any window outside 1 .. 256)
            window = 0
        _check(self._lib.vs_query_ld_prune(self._h, ptr, n, ids_ptr, n_ids, window, int(max_bp) & 0xFFFFFFFF, threshold, int(min_ac),
                                           0xFFFFFFFF if max_ac is None else int(max_ac), C.byref(h)), "vs_query_ld_prune")
        return QueryResult(self, h)

    def ld_scores(self, regions, samples=None, window=0, max_bp=1_000_000, min_ac=0, max_ac=None) -> QueryResult:
        """LD scores over regions (vs_query_ld_scores): for every table row of every region the sum of its squared dosage
        correlation with the rows of the same region at most `window` table rows (0: no limit; there is no 256-row ceiling) and at
        most `max_bp` positions (0: no limit) away, the row itself included, over `samples` (names or ids, taken as a set; None:
        the whole cohort).  A row is scored when it is polymorphic there and its alternate-allele count lies in [min_ac, max_ac]
        (max_ac None: no upper limit); the others are skipped and add to no sum.  Every r2 is floor(r2 * 2**32) in exact integers
        and the sums are integers: the same call gives the same bytes.  Regions are independent.  `regions` as for
        allele_counts.  Read the result with QueryResult.ld_scores / region_ld_scores / ld_scores_device / region_text."""
        arr, ptr, n = _regions_array(regions)
        h = C.c_void_p()
        ids, ids_ptr, n_ids = self._sample_set(samples)   # (ids keeps the array alive over the call)
        window, max_bp = int(window), int(max_bp)
        if not 0 <= window <= 0xFFFFFFFF or not 0 <= max_bp <= 0xFFFFFFFF:
            raise ValueError(f"window {window} / max_bp {max_bp}: 0 .. 2**32 - 1")
        _check(self._lib.vs_query_ld_scores(self._h, ptr, n, ids_ptr, n_ids, window, max_bp, int(min_ac),
                                            0xFFFFFFFF if max_ac is None else int(max_ac), C.byref(h)), "vs_query_ld_scores")
        return QueryResult(self, h)

    def ld_matrix(self, regions, samples=None, stat="r2") -> QueryResult:
        """LD matrices over regions (vs_query_ld_matrix): for every region the full square block of its table rows against each
        other, diagonal included, over the dosages of `samples` (names or ids, taken as a set; None: the whole cohort).  `stat`:
        "r2" (squared dosage correlation, float32) or "dot" (sum of dosage products, int32, exact).  `regions` as for
        allele_counts.  Read the result with QueryResult.ld_matrix / region_ld_matrix / ld_matrix_device / region_text."""
        arr, ptr, n = _regions_array(regions)
        h = C.c_void_p()
        if isinstance(stat, str):
            if stat.lower() not in QueryResult.LD_STATS:
                raise ValueError(f"stat {stat!r}: 'r2' or 'dot'")
            stat = QueryResult.LD_STATS[stat.lower()]
        ids, ids_ptr, n_ids = self._sample_set(samples)   # (ids keeps the array alive over the call)
        _check(self._lib.vs_query_ld_matrix(self._h, ptr, n, ids_ptr, n_ids, int(stat) & 0xFFFFFFFF, C.byref(h)), "vs_query_ld_matrix")
        return QueryResult(self, h)

    def sample_gram(self, regions, samples=None, stat="dot") -> QueryResult:
        """Sample Gram matrix over regions (vs_query_sample_gram): D^T D, the samples x samples products of the dosages over every
        row of the variant table a type-6 batch over `regions` produces, for `samples` (names or ids, taken as a set; None: the
        whole cohort).  `stat`: "dot" (the exact int64 products) or "grm" (the same and VanRaden's first GRM as float64, formed
        from exact integers).  `regions` as for allele_counts.  Read the result with QueryResult.sample_gram / sample_gram_device."""
        arr, ptr, n = _regions_array(regions)
        h = C.c_void_p()
        if isinstance(stat, str):
            if stat.lower() not in QueryResult.GRAM_STATS:
                raise ValueError(f"stat {stat!r}: 'dot' or 'grm'")
            stat = QueryResult.GRAM_STATS[stat.lower()]
        ids, ids_ptr, n_ids = self._sample_set(samples)   # (ids keeps the array alive over the call)
        _check(self._lib.vs_query_sample_gram(self._h, ptr, n, ids_ptr, n_ids, int(stat) & 0xFFFFFFFF, C.byref(h)), "vs_query_sample_gram")
        return QueryResult(self, h)

    def sample_ibs(self, regions, samples=None, stat="counts") -> QueryResult:
        """Pairwise IBS counts over regions (vs_query_sample_ibs): for every pair of `samples` (names or ids, taken as a set; None:
        the whole cohort) how often, over the rows of the variant table a type-6 batch over `regions` produces, both are
        heterozygous, both hom-alt, both carriers, opposite homozygotes (IBS0) and equal (IBS2) -- exact int64.  `stat`: "counts"
        or "king" (the same and the KING-robust kinship as float64, formed from exact integers).  `regions` as for allele_counts.
        Read the result with QueryResult.sample_ibs / sample_ibs_device."""
        arr, ptr, n = _regions_array(regions)
        h = C.c_void_p()
        if isinstance(stat, str):
            if stat.lower() not in QueryResult.IBS_STATS:
                raise ValueError(f"stat {stat!r}: 'counts' or 'king'")
            stat = QueryResult.IBS_STATS[stat.lower()]
        ids, ids_ptr, n_ids = self._sample_set(samples)   # (ids keeps the array alive over the call)
        _check(self._lib.vs_query_sample_ibs(self._h, ptr, n, ids_ptr, n_ids, int(stat) & 0xFFFFFFFF, C.byref(h)), "vs_query_sample_ibs")
        return QueryResult(self, h)

    def trio_ids(self, trios):
        """`trios` -- a sequence of (child, father, mother), each a name or an id, or an (n, 3) integer array -- as the contiguous
        (n, 3) uint32 array of sample ids the C ABI takes."""
        if isinstance(trios, np.ndarray) and trios.dtype.kind in "ui":
            ids = np.ascontiguousarray(trios, dtype=np.uint32)
        else:
            ids = np.ascontiguousarray([[self.sample_id(x) if isinstance(x, str) else int(x) for x in t] for t in trios], dtype=np.uint32)
        if ids.size == 0:
            return ids.reshape(0, 3)
        if ids.ndim != 2 or ids.shape[1] != 3:
            raise ValueError("trios: (child, father, mother) triples expected")
        return ids

    def trio_scan(self, regions, trios) -> QueryResult:
        """Trio scan over regions (vs_query_trio_scan): for every row of the variant table a type-6 batch over `regions` produces
        and every trio, whether the three dosages obey Mendel's laws and which alleles heterozygous parents transmitted -- summed
        per row over the trios and per trio over the rows, exact uint32: errors, de novo calls, transmitted and untransmitted
        alleles.  `trios`: a sequence of (child, father, mother), each a name or an id, or an (n, 3) integer array; a sample may
        appear in any number of trios and in any role.  Meant for diploid calls (only the dosage takes part).  `regions` as for
        allele_counts.  Read the result with QueryResult.trio_scan / region_trio_stats / trio_scan_device."""
        arr, ptr, n = _regions_array(regions)
        ids = self.trio_ids(trios)
        h = C.c_void_p()
        _check(self._lib.vs_query_trio_scan(self._h, ptr, n, _u32_ptr(ids) if ids.size else None, ids.shape[0], C.byref(h)),
               "vs_query_trio_scan")
        return QueryResult(self, h)

    def roh(self, regions, samples=None, min_sites=50, min_bp=0, max_gap=0, max_het=0, min_ac=0, max_ac=None, segments=True) -> QueryResult:
        """Runs of homozygosity over regions (vs_query_roh): for every region and every column of `samples` (names or ids, taken
        as a set; None: the whole cohort) the stretches of consecutive sites at which the sample is homozygous.  A site is a
        table row that is polymorphic over the columns with its alternate-allele count in [min_ac, max_ac] (max_ac None: no upper
        limit); other rows are invisible.  A run may absorb up to `max_het` (0 .. 255) heterozygous sites between homozygous
        ones, is cut where two consecutive sites lie more than `max_gap` bases apart (0: never), and is a segment when it has at
        least `min_sites` sites and spans at least `min_bp` bases.  Integers throughout: the same call gives the same bytes.
        segments=False leaves the segment list out (summaries only, one pass).  Regions are independent.  `regions` as for
        allele_counts.  Read the result with QueryResult.roh / region_roh / roh_device / region_text."""
        arr, ptr, n = _regions_array(regions)
        h = C.c_void_p()
        ids, ids_ptr, n_ids = self._sample_set(samples)   # (ids keeps the array alive over the call)
        vals = {"min_sites": min_sites, "min_bp": min_bp, "max_gap": max_gap, "max_het": max_het, "min_ac": min_ac,
                "max_ac": 0xFFFFFFFF if max_ac is None else max_ac}
        for k, v in vals.items():
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError(f"{k} {v}: 0 .. 2**32 - 1")
        prm = _lib.RohParams(**{k: int(v) for k, v in vals.items()}, segments=1 if segments else 0)
        _check(self._lib.vs_query_roh(self._h, ptr, n, ids_ptr, n_ids, C.byref(prm), C.byref(h)), "vs_query_roh")
        return QueryResult(self, h)

    def assoc_scan(self, regions, traits, samples=None, stat="dot", trait_names=None) -> QueryResult:
        """Association scan over regions (vs_query_assoc_scan): every row of the variant table a type-6 batch over `regions`
        produces against K phenotypes (1 .. 8) in one pass over its carriers, no genotype matrix in between.  `traits`: array-like
        of shape (n,) or (n, K), float32; row i belongs to samples[i] (names or ids, in any order, each once), or with samples
        None to sample id i + 1 of the whole cohort.  `stat`: "dot" (the sum of dosage x value, float64) or "chi2" (the score test
        of a regression of the value on the dosage; for a 0/1 trait the Cochran-Armitage trend test).  Pass residuals to adjust
        for covariates, and the subset of samples that have a value.  `regions` as for allele_counts.  Read the result with
        QueryResult.assoc_scan / assoc_scan_device / region_assoc / region_text."""
        y = np.asarray(traits, dtype=np.float32)
        if y.ndim == 1:
            y = y.reshape(-1, 1)
        if y.ndim != 2:
            raise ValueError("traits: an array of shape (n,) or (n, K)")
        y = np.ascontiguousarray(y)
        if isinstance(stat, str):
            if stat.lower() not in QueryResult.ASSOC_STATS:
                raise ValueError(f"stat {stat!r}: 'dot' or 'chi2'")
            stat = QueryResult.ASSOC_STATS[stat.lower()]
        arr, ptr, n = _regions_array(regions)
        ids, ids_ptr, n_ids = self._sample_set(samples)   # (ids keeps the array alive over the call)
        if samples is None:
            n_ids = y.shape[0]
        elif n_ids != y.shape[0]:
            raise ValueError(f"traits has {y.shape[0]} rows for {n_ids} samples")
        names = [str(s) for s in trait_names] if trait_names is not None else None
        if names is not None and len(names) != y.shape[1]:
            raise ValueError(f"{len(names)} trait names for {y.shape[1]} traits")
        name_arr = (C.c_char_p * len(names))(*[s.encode() for s in names]) if names else None
        h = C.c_void_p()
        _check(self._lib.vs_query_assoc_scan(self._h, ptr, n, ids_ptr, n_ids, y.ctypes.data_as(C.POINTER(C.c_float)), y.shape[1],
                                             int(stat) & 0xFFFFFFFF, name_arr, C.byref(h)), "vs_query_assoc_scan")
        return QueryResult(self, h)

    def assoc_matrix(self, regions, traits, samples=None, stat="dot", trait_names=None) -> QueryResult:
        """Trait-matrix association scan over regions (vs_query_assoc_matrix): every row of the variant table a type-6 batch over
        `regions` produces against a wide panel of K traits (1 .. 65,536) -- the product of the dosage matrix with the panel on
        the matrix cores.  `traits`, `samples`, `stat` and `trait_names` as for assoc_scan.  Each trait is quantised to 31-bit
        fixed point (quantise_traits gives the integers); every sum is an exact integer, so the same call gives the same bytes.
        Read the result with QueryResult.assoc_matrix / assoc_matrix_device / region_assoc_matrix / region_text."""
        y = np.asarray(traits, dtype=np.float32)
        if y.ndim == 1:
            y = y.reshape(-1, 1)
        if y.ndim != 2:
            raise ValueError("traits: an array of shape (n,) or (n, K)")
        y = np.ascontiguousarray(y)
        if isinstance(stat, str):
            if stat.lower() not in QueryResult.ASSOC_STATS:
                raise ValueError(f"stat {stat!r}: 'dot' or 'chi2'")
            stat = QueryResult.ASSOC_STATS[stat.lower()]
        arr, ptr, n = _regions_array(regions)
        ids, ids_ptr, n_ids = self._sample_set(samples)   # (ids keeps the array alive over the call)
        if samples is None:
            n_ids = y.shape[0]
        elif n_ids != y.shape[0]:
            raise ValueError(f"traits has {y.shape[0]} rows for {n_ids} samples")
        names = [str(s) for s in trait_names] if trait_names is not None else None
        if names is not None and len(names) != y.shape[1]:
            raise ValueError(f"{len(names)} trait names for {y.shape[1]} traits")
        name_arr = (C.c_char_p * len(names))(*[s.encode() for s in names]) if names else None
        h = C.c_void_p()
        _check(self._lib.vs_query_assoc_matrix(self._h, ptr, n, ids_ptr, n_ids, y.ctypes.data_as(C.POINTER(C.c_float)), y.shape[1],
                                               int(stat) & 0xFFFFFFFF, name_arr, C.byref(h)), "vs_query_assoc_matrix")
        return QueryResult(self, h)

    def sample_scores(self, regions, weights, samples=None, score_names=None) -> QueryResult:
        """Per-sample scores over regions (vs_query_sample_scores): for every sample of `samples` (names or ids, each once; None:
        the whole cohort) K weighted sums of its dosages over the rows a type-6 batch over `regions` reports -- a polygenic score
        per weight column, no genotype matrix in between.  `weights` is either an array-like of shape (N,) or (N, K), float32
        (or a DeviceArray of N x K float32 in this GPU's memory, with `score_names` or K = 1), in REPORT order: region after region
        as given, within a region the rows it reports (the data lines of region_text), a row of weights per reported row; or a
        mapping {(pos, ref, alt): value or K values} with ref / alt as the texts print them.  For a mapping an allele_counts batch
        over the regions is run first to learn the reported rows; rows without a key weigh 0, and the keys that matched no row
        come back as `result.unmatched`.  The sums are taken in 64-bit fixed point (the weights of a column are quantised to
        2^-36 of the column's largest): the same call gives the same bytes.  Read the result with QueryResult.sample_scores /
        sample_scores_device."""
        names = [str(s) for s in score_names] if score_names is not None else None
        unmatched = None
        keep = None
        if isinstance(weights, dict):
            weights, unmatched = self._weights_from_mapping(regions, weights)
        if isinstance(weights, DeviceArray):
            k = len(names) if names is not None else 1
            if weights.n % k:
                raise ValueError(f"{weights.n} device weights are no whole number of rows of {k}")
            w_ptr, n_w = C.c_void_p(weights.ptr), weights.n // k
        else:
            w = np.asarray(weights, dtype=np.float32)
            if w.ndim == 1:
                w = w.reshape(-1, 1)
            if w.ndim != 2:
                raise ValueError("weights: an array of shape (N,) or (N, K), or a mapping")
            keep = w = np.ascontiguousarray(w)
            k = w.shape[1]
            w_ptr, n_w = C.c_void_p(w.ctypes.data if w.size else None), w.shape[0]
        if names is not None and len(names) != k:
            raise ValueError(f"{len(names)} score names for {k} weight columns")
        arr, ptr, n = _regions_array(regions)
        ids, ids_ptr, n_ids = self._sample_set(samples)   # (ids keeps the array alive over the call)
        if samples is None:
            if getattr(self, "_cohort", None) is None:
                self._cohort = self.info().num_samples - 1
            n_ids = self._cohort
        name_arr = (C.c_char_p * len(names))(*[s.encode() for s in names]) if names else None
        h = C.c_void_p()
        _check(self._lib.vs_query_sample_scores(self._h, ptr, n, ids_ptr, n_ids, w_ptr, n_w, k, name_arr, C.byref(h)), "vs_query_sample_scores")
        del keep
        res = QueryResult(self, h)
        res.score_names = names
        res.unmatched = unmatched
        return res

    def score_matrix(self, regions, weights, samples=None, score_names=None) -> QueryResult:
        """Score matrix over regions (vs_query_score_matrix): sample_scores for a wide panel of weight columns, 1 .. 65,536, as a
        product with the temporary genotype matrix on the matrix cores.  `regions`, `samples`, `score_names` and `weights` -- an
        array-like of shape (N,) or (N, K), float32, in report order, or a mapping {(pos, ref, alt): value or K values}, with
        `result.unmatched` -- are sample_scores'; the weights are host memory.  The sums are taken in fixed point (the weights of a
        column are quantised to 2^-30 of the column's largest): the same call gives the same bytes.  Read the result with
        QueryResult.score_matrix / score_matrix_device."""
        names = [str(s) for s in score_names] if score_names is not None else None
        unmatched = None
        if isinstance(weights, dict):
            weights, unmatched = self._weights_from_mapping(regions, weights)
        if isinstance(weights, DeviceArray):
            raise ValueError("score_matrix takes its weights from host memory")
        w = np.asarray(weights, dtype=np.float32)
        if w.ndim == 1:
            w = w.reshape(-1, 1)
        if w.ndim != 2:
            raise ValueError("weights: an array of shape (N,) or (N, K), or a mapping")
        w = np.ascontiguousarray(w)
        k = w.shape[1]
        if names is not None and len(names) != k:
            raise ValueError(f"{len(names)} score names for {k} weight columns")
        arr, ptr, n = _regions_array(regions)
        ids, ids_ptr, n_ids = self._sample_set(samples)   # (ids keeps the array alive over the call)
        if samples is None:
            if getattr(self, "_cohort", None) is None:
                self._cohort = self.info().num_samples - 1
            n_ids = self._cohort
        name_arr = (C.c_char_p * len(names))(*[s.encode() for s in names]) if names else None
        h = C.c_void_p()
        w_ptr = w.ctypes.data_as(C.POINTER(C.c_float)) if w.size else None
        _check(self._lib.vs_query_score_matrix(self._h, ptr, n, ids_ptr, n_ids, w_ptr, w.shape[0], k, name_arr, C.byref(h)), "vs_query_score_matrix")
        res = QueryResult(self, h)
        res.score_names = names
        res.unmatched = unmatched
        return res

    def _weights_from_mapping(self, regions, mapping):
        """The (N, K) float32 array in report order of a {(pos, ref, alt): value(s)} mapping, and the keys that matched no row."""
        table, k = {}, None
        for key, v in mapping.items():
            vals = np.atleast_1d(np.asarray(v, dtype=np.float32))
            if vals.ndim != 1 or (k is not None and vals.shape[0] != k):
                raise ValueError(f"weights of {key!r}: every key takes the same number of values")
            k = vals.shape[0]
            table[(int(key[0]), str(key[1]), str(key[2]))] = vals
        if k is None:
            raise ValueError("an empty mapping of weights")
        counts = self.allele_counts(regions)
        try:
            n_regions = counts.totals()[0]
            rows, seen = [], set()
            for q in range(n_regions):
                for line in counts.region_text(q).split("\n")[1:]:
                    if not line:
                        continue
                    f = line.split("\t")
                    key = (int(f[0]), f[1], f[2])
                    rows.append(key)
        finally:
            counts.close()
        w = np.zeros((len(rows), k), np.float32)
        for i, key in enumerate(rows):
            v = table.get(key)
            if v is not None:
                w[i] = v
                seen.add(key)
        return w, [key for key in table if key not in seen]

    def _table_keys(self, regions):
        """The (pos, ref, alt) of every table row of a batch, in table order (None for a row under the duplicate rule, which no
        region reports), through an allele_counts batch over the same regions."""
        counts = self.allele_counts(regions)
        try:
            got = counts.allele_counts()
            dropped = (got["rows"]["count_flags"] >> 31) != 0
            keys = [None] * got["rows"].shape[0]
            for q in range(got["row_begin"].shape[0]):
                a0, m = int(got["row_begin"][q]), int(got["row_count"][q])
                live = [a for a in range(a0, a0 + m) if not dropped[a]]
                if all(keys[a] is not None for a in live):
                    continue
                lines = [line for line in counts.region_text(q).split("\n")[1:] if line]
                assert len(lines) == len(live)
                for a, line in zip(live, lines):
                    f = line.split("\t")
                    keys[a] = (int(f[0]), f[1], f[2])
        finally:
            counts.close()
        return keys

    def _pvalues_from_mapping(self, regions, mapping):
        """The float64 array in table order of a {(pos, ref, alt): p} mapping (NaN for a row without a key), and the keys that
        matched no row."""
        table = {(int(k[0]), str(k[1]), str(k[2])): float(v) for k, v in mapping.items()}
        keys = self._table_keys(regions)
        seen = set()
        pv = np.full(len(keys), np.nan, np.float64)
        for i, key in enumerate(keys):
            if key in table:
                pv[i] = table[key]
                seen.add(key)
        return pv, [key for key in table if key not in seen]

    def ld_clump(self, regions, pvalues, samples=None, window=256, r2=0.5, max_bp=250_000, p1=1e-4, p2=1e-2) -> QueryResult:
        """LD clumping over regions (vs_query_ld_clump), as `plink --clump`: for every region its rows are taken in order of
        significance; the best one with p <= `p1` becomes an index row, every row with p <= `p2` among the `window` (1 .. 256) rows
        on either side of it (at most `max_bp` positions away; 0: no limit) whose squared dosage correlation with it over `samples`
        is above `r2` joins its clump; the next best row that is still unclaimed starts the next clump.  `pvalues`: an array of A
        float64 in table order (the rows an allele_counts batch over the same regions returns; NaN: no p-value), or a mapping
        {(pos, ref, alt): p}, resolved through an allele_counts batch: rows without a key get NaN, keys that matched no row come
        back as `result.unmatched`.  The p-values become 64-bit keys (pvalue_keys) and r2 the integer T = quantise_r2(r2): the
        device compares integers only, ties go to the earlier row.  Regions are independent.  Read the result with
        QueryResult.ld_clump / ld_clump_device / region_clumps / region_text."""
        threshold = quantise_r2(r2)
        unmatched = None
        if isinstance(pvalues, dict):
            pv, unmatched = self._pvalues_from_mapping(regions, pvalues)
        else:
            pv = np.ascontiguousarray(np.asarray(pvalues, dtype=np.float64))
            if pv.ndim != 1:
                raise ValueError("pvalues: one float64 per table row")
        arr, ptr, n = _regions_array(regions)
        h = C.c_void_p()
        ids, ids_ptr, n_ids = self._sample_set(samples)   # (ids keeps the array alive over the call)
        window = int(window)
        if not 0 <= window <= 0xFFFFFFFF:   # (ctypes would wrap it: 0 is refused by the C ABI like any window outside 1 .. 256)
            window = 0
        buf = pv if pv.shape[0] else np.zeros(1, np.float64)   # (the C ABI refuses NULL)
        _check(self._lib.vs_query_ld_clump(self._h, ptr, n, ids_ptr, n_ids, buf.ctypes.data_as(C.POINTER(C.c_double)), pv.shape[0], window,
                                           int(max_bp) & 0xFFFFFFFF, threshold, float(p1), float(p2), C.byref(h)), "vs_query_ld_clump")
        res = QueryResult(self, h)
        res.unmatched = unmatched
        res._clump_pvalues = pv.copy()
        return res

    def get_sample_var_in_ref(self, regions, sample) -> QueryResult:
        """Query type 4 for one sample over a batch of regions (query.h:618-729)."""
        arr, ptr, n = _regions_array(regions)
        h = C.c_void_p()
        if isinstance(sample, (list, tuple, np.ndarray, DeviceArray)):  # one sample per region
            sids = self._sample_ids(sample, n)
            _check(self._lib.vs_query_samples_var_in_ref(self._h, ptr, n, _u32_ptr(sids),
                                                         C.byref(h)), "vs_query_samples_var_in_ref")
            return QueryResult(self, h)
        sid = self.sample_id(sample) if isinstance(sample, str) else int(sample)
        _check(self._lib.vs_query_sample_var_in_ref(self._h, ptr, n, sid, C.byref(h)), "vs_query_sample_var_in_ref")
        return QueryResult(self, h)

    def closest_var(self, positions) -> QueryResult:
        """Query type 1 (query.h:441-483) for a batch of positions: one result "region" per position;
        `region_flags & 4` marks the calls for which the reference returns false."""
        pos = np.ascontiguousarray(positions, dtype=np.uint64)
        h = C.c_void_p()
        _check(self._lib.vs_query_closest_var(self._h, pos.ctypes.data_as(C.POINTER(C.c_uint64)), pos.shape[0],
                                              C.byref(h)), "vs_query_closest_var")
        return QueryResult(self, h)

    def samples_has_var(self, positions, refs, alts) -> QueryResult:
        """Query type 7 (query.h:792-823) for a batch of (pos, ref, alt): region_text(q) is the reference's
        output line, `region_flags & 4` means "There is no such variant!"."""
        pos = np.ascontiguousarray(positions, dtype=np.uint64)
        n = pos.shape[0]
        if len(refs) != n or len(alts) != n:
            raise ValueError("one ref and one alt per position expected")
        r = refs if isinstance(refs, C.Array) else self.c_strings(refs)      # (a caller that asks again and again builds the arrays once)
        a = alts if isinstance(alts, C.Array) else self.c_strings(alts)
        h = C.c_void_p()
        _check(self._lib.vs_query_samples_has_var(self._h, pos.ctypes.data_as(C.POINTER(C.c_uint64)), r, a, n,
                                                  C.byref(h)), "vs_query_samples_has_var")
        return QueryResult(self, h)

    @staticmethod
    def c_strings(strings):
        """`strings` as the char*[] the C ABI takes (samples_has_var accepts the result in place of a list)."""
        return (C.c_char_p * max(len(strings), 1))(*[x.encode("latin-1") for x in strings])

    def _sample_ids(self, sample, n):
        if isinstance(sample, DeviceArray):
            if sample.n != n:
                raise ValueError("one sample per region expected")
            return sample
        if isinstance(sample, np.ndarray) and sample.dtype.kind in "ui":   # ids already: no per-element Python
            sids = np.ascontiguousarray(sample, dtype=np.uint32)
            if sids.shape[0] != n:
                raise ValueError("one sample per region expected")
            return sids
        if isinstance(sample, (list, tuple, np.ndarray)):
            sids = np.ascontiguousarray([self.sample_id(x) if isinstance(x, str) else int(x) for x in sample], dtype=np.uint32)
            if sids.shape[0] != n:
                raise ValueError("one sample per region expected")
            return sids
        sid = self.sample_id(sample) if isinstance(sample, str) else int(sample)
        return np.full(max(n, 1), sid, dtype=np.uint32)

    def query_sample_seq(self, regions, sample, sample_coordinates=False) -> QueryResult:
        """Query type 2 (query_sample_from_ref, query.h:118-190) or, with sample_coordinates, type 3
        (query_sample_from_sample, query.h:196-261).  `sample` is one name/id or one per region."""
        arr, ptr, n = _regions_array(regions)
        sids = self._sample_ids(sample, n)
        h = C.c_void_p()
        _check(self._lib.vs_query_sample_seq(self._h, ptr, n, _u32_ptr(sids),
                                             1 if sample_coordinates else 0, C.byref(h)), "vs_query_sample_seq")
        return QueryResult(self, h)

    def get_sample_var_in_sample(self, regions, sample) -> QueryResult:
        """Query type 5 (query.h:490-612)."""
        arr, ptr, n = _regions_array(regions)
        sids = self._sample_ids(sample, n)
        h = C.c_void_p()
        _check(self._lib.vs_query_sample_var_in_sample(self._h, ptr, n, _u32_ptr(sids),
                                                       C.byref(h)), "vs_query_sample_var_in_sample")
        return QueryResult(self, h)

    def draw_subgraph(self, pos, radius, outfile, sample=None):
        """`variantstore draw` (query.h:825-842, dot_graph.h:71-132): Graphviz file of the neighbourhood of the
        vertex at `pos`.  Host-only."""
        _check(self._lib.vs_index_draw_subgraph(self._h, int(pos), int(radius), sample.encode() if sample else None,
                                                str(outfile).encode()), "vs_index_draw_subgraph")
