// k_window_stats.hip.h -- windowed diversity statistics (vs_query_window_stats): k_group_counts' records reduced per region and
// sample group (and per pair of groups) to the exact integers pi, Watterson's theta, Tajima's D, dxy and Hudson's Fst are formed from.
// Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_group_counts.hip.h"

namespace vsamd {

// Input: gc[row * G + g] = {carriers, alt_alleles, hom_alt, phased} of table row `row` over group g (k_group_counts over the whole
// table, into a temporary).  Region q reports the contiguous rows var_begin[q] .. + q_nvar[q] of the table; regions overlap, so a
// table row is read by every region that reports it (4.08 on the bench) -- from L2 / Infinity Cache where neighbouring regions run
// side by side, as they do in a sorted batch: the four regions of a workgroup are consecutive.  A private row (behind the U shared
// rows) that the duplicate rule dropped is no site: its counts are zero in every group and it is left out of `rows`.
//
// Output per (region, group), 48 bytes: rows, seg, singletons, doubletons, private, fixed (uint32), sum_ac, sum_ac2, obs_het (uint64);
// per (region, pair g < h), 16 bytes: sum_cross (uint64), seg_union, fixed_diff (uint32).  With ac a row's alt_alleles in g and
// N_g = 2 x group_size[g] (two allele copies per sample whatever the call's ploidy, as the GRM's 2n; a multi-allelic site's ALT rows are
// separate sites with the index's genotype bits).  Integers only; no floating-point value is formed here.
//
// Overflow: the label table admits at most 32,767 samples, so ac <= 65,534 < 2^16, ac^2 and ac_g ac_h < 2^32, het <= 32,767 < 2^15.
// A region has fewer than 2^32 rows (the table's rows are counted in 32 bits per region: `rows` is a uint32), so sum_ac < 2^48,
// obs_het < 2^47 and sum_ac2, sum_cross < 2^32 x 2^32 = 2^64: no 64-bit sum can overflow for any table the engine admits.
//
// Mapping.  A region of the headline shape has ~203 rows and G is 1 .. 26: too few rows for a workgroup, too few groups for a wave.
// So a WAVE owns a region (four regions a workgroup) and walks it in tiles of T = min(64, 2048 / G) rows:
//   staging   the tile's T x G records are contiguous in gc: 16-byte loads, consecutive lanes consecutive records, each packed to
//             one LDS word  ac | het << 16 | (ac == N_g) << 31  at cell[r * G + g] -- the index of the load, no division
//   totals    lane r sums the ac of row r over the groups (its reads rotated by r, so that the lanes of a half-wave fall on
//             different banks even where G is a multiple of 32): `private` is ac > 0 and ac == the row's total
//   groups    lane l owns (row slice l / G, group l % G), floor(64 / G) slices: G = 2 keeps all 64 lanes busy, G = 26 keeps 52.  A
//             lane reads one cell per row of its slice: the lanes of a slice read G consecutive words, slices consecutive rows
//   pairs     P = G (G - 1) / 2 pairs.  P < 64: lane l owns (row slice l / P, pair l % P).  P >= 64: a lane owns the pairs
//             l, l + 64, ... -- NPB of them (template: 1, 2, 4, 8, 16, 32 for P <= 64 .. 2,048), their sums in registers, the loop
//             over them unrolled so that no register array is indexed by a variable: (g, h) of a pair sits in one register, read
//             once from a table in LDS; a row costs two LDS reads and one 32 x 32 -> 64-bit multiply-add per pair (sum_cross).
//             seg_union and fixed_diff come from two 64-bit row masks per group (rows with ac == 0, rows with ac == N_g, by ballot
//             once a tile): four ANDs and population counts per pair and TILE instead of compares per pair and row
//   the end   slices are summed through shuffles (stride G or P, a tree over the slices), then one lane per record stores it
// LDS per workgroup: cells 4 x 4 x min(2048, 64 G) B (dynamic: 1 KiB at G = 1, 26 KiB at G = 26, 32 KiB from G = 32 on), totals 1 KiB,
// N_g 256 B, with pairs the pair table 4 KiB and the row masks 4 KiB: 35.2 KiB at G = 26 (four workgroups, 16 waves, per CU),
// 41.2 KiB from G = 32 on (three).  Registers limit the waves further from NPB = 8 on (DESIGN 5q has the compiler's counts): NPB = 32
// (G = 46 .. 64) holds 4 x 32 accumulator and 32 pair registers and takes 356 in all, one wave per SIMD; no variant uses scratch.
//
// A region of more than chunk_rows rows is SPLIT (k_burden.hip.h's scheme): the wave above writes zeros for it, k_burden_split_plan
// lists its chunks, and a second launch (SPLIT) gives a chunk to a workgroup whose four waves take every fourth tile and add
// their nonzero sums with integer atomics -- exact, so the order does not matter.  A batch without such a region launches neither.
// Every record is stored whatever the buffer held: zeros of empty regions, empty groups and dropped rows included.
constexpr uint32_t kWinCells = 2048;       // packed cells of a wave's tile
constexpr uint32_t kWinChunkRows = 4096;   // rows a wave walks before a region is split (option window_chunk)
constexpr uint32_t kWinRecWords = 12;      // a 48-byte record
constexpr uint32_t kWinPairsMax = 2016;    // 64 x 63 / 2

__host__ __device__ inline uint32_t window_cells(uint32_t G) { return 64 * G < kWinCells ? 64 * G : kWinCells; }

struct WindowArgs {
  const uint4* gc;             // k_group_counts' records [A x G]
  const VariantRow* rows;      // the table
  uint64_t U;                  // shared rows: the rows behind them are private and may be dropped
  const uint64_t* var_begin;   // per region, in the caller's order
  const uint64_t* q_nvar;
  uint64_t Q;
  uint32_t G, P, chunk_rows;   // P: 0 without pair records
  const uint2* work;           // SPLIT: {region, chunk}
  const uint32_t* n_work;
  uint32_t* rec;               // [Q x G] records of kWinRecWords words
  uint4* pair;                 // [Q x P]
  uint16_t gsize[64];          // samples of every group
};

// the sum over the `n` slices of a value held by the lanes (slice s, item i) = lane s * stride + i: lanes of slice 0 get the total
template <typename T>
__device__ __forceinline__ T slice_sum(T v, uint32_t lane, uint32_t slice, uint32_t n, uint32_t stride) {
  uint32_t p = 1;
  while (p < n) p <<= 1;
  for (uint32_t off = p >> 1; off; off >>= 1) {
    const T t = __shfl(v, (int)((lane + off * stride) & 63u));
    if (slice + off < n) v += t;
  }
  return v;
}

template <uint32_t NPB, bool SPLIT>
__global__ void __launch_bounds__(256) k_window_stats(WindowArgs a) {
  extern __shared__ uint32_t s_cell[];   // 4 x window_cells(G)
  __shared__ uint32_t s_tot[4][64];
  __shared__ uint32_t s_n[64];
  __shared__ uint16_t s_gh[NPB ? kWinPairsMax : 1];
  __shared__ unsigned long long s_zm[NPB ? 4 : 1][64], s_fm[NPB ? 4 : 1][64];   // per group: the tile's rows with ac == 0, with ac == N_g
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint32_t G = a.G, P = NPB ? a.P : 0;
  if (threadIdx.x < 64) s_n[threadIdx.x] = threadIdx.x < G ? 2u * a.gsize[threadIdx.x] : 0u;
  if (NPB && threadIdx.x + 1 < G) {   // pair p = (g, h), g < h, in the order (0,1), (0,2), ..., (G-2,G-1)
    const uint32_t g = threadIdx.x;
    uint32_t p = g * (2 * G - g - 1) / 2;
    for (uint32_t h = g + 1; h < G; ++h) s_gh[p++] = (uint16_t)(g | (h << 8));
  }
  __syncthreads();
  // ---- the wave's rows ----
  uint64_t q, r_begin, r_end;
  uint32_t t0 = 0, tstep = 1;
  if (SPLIT) {
    if (blockIdx.x >= *a.n_work) return;
    q = a.work[blockIdx.x].x;
    const uint64_t a0 = a.var_begin[q];
    r_begin = a0 + (uint64_t)a.work[blockIdx.x].y * a.chunk_rows;
    r_end = a0 + a.q_nvar[q];
    if (r_end > r_begin + a.chunk_rows) r_end = r_begin + a.chunk_rows;
    t0 = wid; tstep = 4;
  } else {
    q = (uint64_t)blockIdx.x * 4 + wid;
    if (q >= a.Q) return;
    const uint64_t nv = a.q_nvar[q];
    r_begin = a.var_begin[q];
    r_end = nv > a.chunk_rows ? r_begin : r_begin + nv;   // a split region: zeros here, its chunks add to them
  }
  const uint32_t T = kWinCells / G < 64 ? kWinCells / G : 64u;
  uint32_t* cell = s_cell + wid * window_cells(G);
  uint32_t* tot = s_tot[wid];
  // ---- the lane's parts ----
  const uint32_t S = 64 / G, gg = lane % G, gs = lane / G;
  const bool gact = gs < S;
  const uint32_t n_g = s_n[gg];
  const uint32_t PW = P < 64 ? (P ? P : 1u) : 64u, SP = 64 / PW, pl = lane % PW, ps = lane / PW;
  uint32_t gh[NPB ? NPB : 1];   // g | h << 8 | both groups have members << 16 | the lane owns the pair << 17 | neither has << 18
#pragma unroll
  for (uint32_t b = 0; b < NPB; ++b) {
    const uint32_t p = b * 64 + pl;
    const bool own = p < P && ps < SP;
    const uint32_t e = own ? s_gh[p] : 0u;
    gh[b] = e | ((own && s_n[e & 0xFF] && s_n[e >> 8]) ? 1u << 16 : 0u) | (own ? 1u << 17 : 0u) | ((own && !s_n[e & 0xFF] && !s_n[e >> 8]) ? 1u << 18 : 0u);
  }
  uint32_t nrows = 0, seg = 0, sing = 0, doub = 0, priv = 0, fixd = 0;
  unsigned long long sum_ac = 0, sum_ac2 = 0, sum_het = 0;
  unsigned long long cross[NPB ? NPB : 1];
  uint32_t su[NPB ? NPB : 1], fd[NPB ? NPB : 1];
#pragma unroll
  for (uint32_t b = 0; b < NPB; ++b) { cross[b] = 0; su[b] = 0; fd[b] = 0; }
  const uint32_t gstep = 64 % G;
  for (uint64_t base = r_begin + (uint64_t)t0 * T; base < r_end; base += (uint64_t)tstep * T) {
    const uint32_t n = r_end - base < T ? (uint32_t)(r_end - base) : T;
    const uint64_t row = base + lane;
    bool live = lane < n;
    if (live && row >= a.U && (a.rows[row].count_flags & kRowDropped)) live = false;
    nrows += (uint32_t)__popcll(__ballot(live));
    wave_lds_sync();   // (the tile before this one has been read)
    // ---- staging: n x G records, contiguous ----
    {
      const uint4* __restrict__ src = a.gc + base * G;
      const uint32_t ncell = n * G;
      uint32_t g = gg;   // the group of record j = lane + 64 i
      for (uint32_t j0 = 0; j0 < ncell; j0 += 256) {
        uint4 k[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
          const uint32_t j = j0 + 64 * u + lane;
          k[u] = j < ncell ? src[j] : uint4{0, 0, 0, 0};
        }
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
          const uint32_t j = j0 + 64 * u + lane;
          if (j < ncell) cell[j] = (k[u].y & 0xFFFFu) | (((k[u].x - k[u].z) & 0x7FFFu) << 16) | (k[u].y == s_n[g] ? 0x80000000u : 0u);
          g += gstep;
          if (g >= G) g -= G;
        }
      }
    }
    wave_lds_sync();
    if (G > 1) {   // ---- the rows' totals over all groups ----
      uint32_t t = 0;
      if (lane < n) {
        const uint32_t* cr = cell + lane * G;
        uint32_t k = lane % G;
        for (uint32_t i = 0; i < G; ++i) {
          t += cr[k] & 0xFFFFu;
          if (++k == G) k = 0;
        }
      }
      tot[lane] = t;
      wave_lds_sync();
    }
    // ---- groups ----
    if (gact)
      for (uint32_t r = gs; r < n; r += S) {
        const uint32_t c = cell[r * G + gg], ac = c & 0xFFFFu, full = c >> 31;
        seg += (ac != 0) & (full ^ 1u);
        sing += ac == 1;
        doub += ac == 2;
        priv += ac != 0 && (G == 1 || tot[r] == ac);
        fixd += full & (n_g != 0);
        sum_ac += ac;
        sum_ac2 += (unsigned long long)ac * ac;
        sum_het += (c >> 16) & 0x7FFFu;
      }
    // ---- pairs ----
    if (NPB) {
      // seg_union and fixed_diff from row masks, 64 rows an operation: Z_g the tile's rows with ac_g == 0, F_g those with ac_g == N_g.
      // A row is NOT in seg_union when ac_g + ac_h is 0 (Z_g & Z_h) or N_g + N_h (F_g & F_h) -- disjoint unless neither group has a
      // member, and then no row counts --; a fixed difference is Z_g & F_h or F_g & Z_h, disjoint when both groups have members.
      unsigned long long* zm = s_zm[wid];
      unsigned long long* fm = s_fm[wid];
      for (uint32_t g = 0; g < G; ++g) {
        const uint32_t c = lane < n ? cell[lane * G + g] : 1u;   // (beyond the tile: neither)
        const unsigned long long z = __ballot((c & 0xFFFFu) == 0), f = __ballot((c >> 31) != 0);
        if (lane == 0) { zm[g] = z; fm[g] = f; }
      }
      wave_lds_sync();
#pragma unroll
      for (uint32_t b = 0; b < NPB; ++b) {
        const uint32_t e = gh[b], g = e & 0xFF, h = (e >> 8) & 0xFF;
        if (!((e >> 17) & 1u) || ps) continue;   // (slice 0 of a pair's lanes adds the tile's counts)
        const unsigned long long zg = zm[g], zh = zm[h], fg = fm[g], fh = fm[h];
        if (!((e >> 18) & 1u)) su[b] += n - (uint32_t)__popcll(zg & zh) - (uint32_t)__popcll(fg & fh);
        if ((e >> 16) & 1u) fd[b] += (uint32_t)__popcll(zg & fh) + (uint32_t)__popcll(fg & zh);
        __builtin_amdgcn_sched_barrier(0);   // (the masks of ONE pair in registers at a time: hoisted, the loads of 32 pairs take 256)
      }
      // sum_cross: the one per-row term.  (A lane that owns no pair, or slices beyond the last, sums what nobody reads.  The asm keeps
      // the compiler from hoisting the 2 x NPB cell offsets out of the row loop: 64 more registers at NPB = 32.)
#pragma unroll 1
      for (uint32_t r = ps; r < n; r += SP) {
        const uint16_t* cr = reinterpret_cast<const uint16_t*>(cell + r * G);   // (the low half of a cell: ac)
#pragma unroll
        for (uint32_t b = 0; b < NPB; ++b) {
          uint32_t e = gh[b];
          asm volatile("" : "+v"(e));
          cross[b] += (unsigned long long)((uint32_t)cr[2 * (e & 0xFF)] * (uint32_t)cr[2 * ((e >> 8) & 0xFF)]);
        }
      }
    }
  }
  // ---- the slices' sums; one lane per record ----
  seg = slice_sum(seg, lane, gs, S, G); sing = slice_sum(sing, lane, gs, S, G); doub = slice_sum(doub, lane, gs, S, G);
  priv = slice_sum(priv, lane, gs, S, G); fixd = slice_sum(fixd, lane, gs, S, G);
  sum_ac = slice_sum(sum_ac, lane, gs, S, G); sum_ac2 = slice_sum(sum_ac2, lane, gs, S, G); sum_het = slice_sum(sum_het, lane, gs, S, G);
  if (lane < G) {
    uint32_t* dst = a.rec + (q * G + lane) * kWinRecWords;
    if (!SPLIT) {
      uint4* d4 = reinterpret_cast<uint4*>(dst);
      d4[0] = uint4{nrows, seg, sing, doub};
      d4[1] = uint4{priv, fixd, (uint32_t)sum_ac, (uint32_t)(sum_ac >> 32)};
      d4[2] = uint4{(uint32_t)sum_ac2, (uint32_t)(sum_ac2 >> 32), (uint32_t)sum_het, (uint32_t)(sum_het >> 32)};
    } else {
      if (nrows) atomicAdd(dst, nrows);
      if (seg) atomicAdd(dst + 1, seg);
      if (sing) atomicAdd(dst + 2, sing);
      if (doub) atomicAdd(dst + 3, doub);
      if (priv) atomicAdd(dst + 4, priv);
      if (fixd) atomicAdd(dst + 5, fixd);
      unsigned long long* d8 = reinterpret_cast<unsigned long long*>(dst + 6);
      if (sum_ac) atomicAdd(d8, sum_ac);
      if (sum_ac2) atomicAdd(d8 + 1, sum_ac2);
      if (sum_het) atomicAdd(d8 + 2, sum_het);
    }
  }
  if (NPB) {
    if (P < 64) {   // (NPB == 1 covers it: the slices of the one pair per lane)
      cross[0] = slice_sum(cross[0], lane, ps, SP, PW); su[0] = slice_sum(su[0], lane, ps, SP, PW); fd[0] = slice_sum(fd[0], lane, ps, SP, PW);
    }
#pragma unroll
    for (uint32_t b = 0; b < NPB; ++b) {
      const uint32_t p = b * 64 + lane;
      if (p >= P || (P < 64 && b)) continue;
      uint4* dst = a.pair + q * P + p;
      if (!SPLIT) *dst = uint4{(uint32_t)cross[b], (uint32_t)(cross[b] >> 32), su[b], fd[b]};
      else {
        if (cross[b]) atomicAdd(reinterpret_cast<unsigned long long*>(dst), cross[b]);
        if (su[b]) atomicAdd(reinterpret_cast<uint32_t*>(dst) + 2, su[b]);
        if (fd[b]) atomicAdd(reinterpret_cast<uint32_t*>(dst) + 3, fd[b]);
      }
    }
  }
}

}  // namespace vsamd
