// k_ld_score.hip.h -- the LD score of every table row of every region over the genotype matrix of a type-6 plan
// (vs_query_ld_scores): k_ld_block's products with an epilogue that reduces the cells instead of storing them.
// Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_ld_block.hip.h"
#include "../host/ld_score_host.hpp"

namespace vsamd {

// Region q owns the table rows row_begin[q] + a, a < m_q, and the slots keep_begin[q] + a (keep_begin: the exclusive scan of the row
// counts, as for a pruning batch).  A row is ELIGIBLE when the duplicate rule did not drop it, v = n Sxx - Sx^2 > 0 (ld_moments) and
// min_ac <= alt_alleles <= max_ac.  For an eligible pair q32(a, b) = floor(cov^2 2^32 / (v_a v_b)), cov = n Sxy - Sx Sy
// (ld_score_q32: exact integers, 0 .. 2^32, exactly 2^32 for a = b).  sums[slot of a] = the sum of q32(a, b) over the eligible b of
// the region, b = a included, with |a - b| <= window (window 0: no limit) and |pos_a - pos_b| <= max_bp (max_bp 0: no limit);
// n_pairs[slot] = the number of b summed.  The other rows keep sums = 0, n_pairs = 0.  No floating-point value is summed or decides.
//
// k_ld_score_scan (one workgroup, ld_region_scans) gives keep_begin and wg_begin, the exclusive scan of the workgroups a region
// takes: with t = ceil(m / 64) tiles and B = window ? min(t - 1, (window + 63) / 64) : t - 1 tile distances, t (B + 1) of them.
//
// k_ld_score_init: a workgroup per region writes every slot's state byte (kLdScoreScored / Ineligible / Dropped), sums = 0 and
// n_pairs = 0, and n_scored[q]: after it no memset is needed.
//
// k_ld_score: a workgroup of four waves per (region, ti, d); the region by bisection over wg_begin as in k_ld_block, ti = p / (B + 1),
// d = p % (B + 1), tj = ti + d; it leaves at once when tj >= t.  Under max_bp it also leaves, before anything is staged, when the
// positions LOADED for the rows of the two panels say that every pair of them is further apart (the smallest of one panel above the
// largest of the other by more than max_bp): no order of the table is assumed.  Products: ld_block_products, the staging, fragments
// and v_mfma_i32_16x16x64_i8 loop of k_ld_block.  Epilogue: register g of lane l in accumulator t is the pair (row ai + 16 wid +
// 4 (l >> 4) + g, row bj + 16 t + (l & 15)).  The lane forms q32 of its 16 cells; the sums per row of panel ti are reduced over the
// four accumulators in the lane and over the 16 lanes of a row group with shuffles; off the diagonal the sums per row of panel tj
// are reduced over the lane's four registers, the four row groups (shuffles) and the four waves (64-bit LDS adds into the staging
// buffer, free by then).  Then one 64-bit integer atomic add per row and panel into sums and one 32-bit add into n_pairs (none for
// a row that summed nothing).  A diagonal pair holds both triangles of its 64 x 64 tile and adds the row sums only.  Integer adds
// commute: the bytes do not depend on the order the workgroups run in.  Every accumulator is indexed statically: no scratch.
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage): DESIGN 5p.
constexpr uint8_t kLdScoreScored = 1, kLdScoreIneligible = 2, kLdScoreDropped = 3;   // VS_LDSCORE_*

struct LdScoreArgs {
  const uint8_t* cells;          // the genotype matrix [A x pitch]
  uint32_t pitch;                // a multiple of 16
  uint32_t n_cols;               // n of the correlation
  uint64_t Q;
  const uint64_t* row_begin;     // per region, in the caller's order
  const uint64_t* row_count;
  const uint64_t* keep_begin;    // [Q + 1]
  const uint64_t* wg_begin;      // [Q + 1]
  const VariantRow* rows;        // the table: positions, the duplicate rule's flag
  const uint4* counts;           // {carriers, alt_alleles, hom_alt, phased} per table row
  uint32_t window, max_bp;       // 0: no limit
  uint32_t min_ac, max_ac;
  unsigned long long* sums;      // [keep_begin[Q]]
  uint32_t* n_pairs;             // [keep_begin[Q]]
  uint8_t* state;                // [keep_begin[Q]]
  uint64_t* n_scored;            // [Q]
};

// tile distances a tile pairs with (itself included) less one, and the workgroups of a region of m rows
__host__ __device__ __forceinline__ uint64_t ld_score_reach(uint64_t t, uint32_t window) {
  const uint64_t w = ((uint64_t)window + kLdBlockTile - 1) / kLdBlockTile;
  return window && w < t - 1 ? w : t - 1;   // (t >= 1)
}
__host__ __device__ __forceinline__ uint64_t ld_score_wgs(uint64_t m, uint32_t window) {
  const uint64_t t = (m + kLdBlockTile - 1) / kLdBlockTile;
  return t ? t * (ld_score_reach(t, window) + 1) : 0;
}

// The state of a table row and, for a scored row, its moments.
__device__ __forceinline__ uint8_t ld_score_row(const LdScoreArgs& a, uint64_t row, int64_t& sx, int64_t& v) {
  const uint4 c = a.counts[row];
  ld_moments(c, (int64_t)a.n_cols, sx, v);
  if (a.rows[row].count_flags & kRowDropped) return kLdScoreDropped;
  return v > 0 && c.y >= a.min_ac && c.y <= a.max_ac ? kLdScoreScored : kLdScoreIneligible;
}

// keep_begin[q], wg_begin[q] = the sums of m and of the workgroups over the regions in front of q; [Q]: the totals.
// summary = {slots, workgroups, largest m, 0}.
__global__ void __launch_bounds__(kLdBlockScanThreads) k_ld_score_scan(const uint64_t* __restrict__ row_count, uint64_t Q, uint64_t* __restrict__ keep_begin,
                                                                        uint64_t* __restrict__ wg_begin, uint64_t* __restrict__ summary, uint32_t window) {
  ld_region_scans(row_count, Q, keep_begin, wg_begin, summary, [](uint64_t m) { return m; }, [window](uint64_t m) { return ld_score_wgs(m, window); });
}

__global__ void __launch_bounds__(256) k_ld_score_init(LdScoreArgs a) {
  __shared__ uint32_t s_n[4];
  const uint64_t q = blockIdx.x;
  const uint64_t m = a.row_count[q], r0 = a.row_begin[q], kb = a.keep_begin[q];
  uint32_t scored = 0;
  for (uint64_t i = threadIdx.x; i < m; i += 256) {
    int64_t sx, v;
    const uint8_t st = ld_score_row(a, r0 + i, sx, v);
    a.state[kb + i] = st;
    a.sums[kb + i] = 0ull;
    a.n_pairs[kb + i] = 0u;
    scored += st == kLdScoreScored;
  }
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) scored += __shfl_xor(scored, d, 64);
  if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = scored;
  __syncthreads();
  if (threadIdx.x == 0) a.n_scored[q] = (uint64_t)s_n[0] + s_n[1] + s_n[2] + s_n[3];
}

__global__ void __launch_bounds__(256) k_ld_score(LdScoreArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_ld[kLdBlockLds];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  // ---- the region: the last q with wg_begin[q] <= blockIdx.x (the launch has wg_begin[Q] workgroups) ----
  const uint64_t wg = blockIdx.x;
  uint64_t lo = 0, hi = a.Q;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (a.wg_begin[mid] <= wg) lo = mid; else hi = mid;
  }
  const uint64_t q = lo;
  const uint64_t m = a.row_count[q], r0 = a.row_begin[q], kb = a.keep_begin[q];
  // ---- the tile pair: ti = p / (B + 1), tj = ti + p % (B + 1) ----
  const uint64_t t_region = (m + kLdBlockTile - 1) / kLdBlockTile;
  if (!t_region) return;   // (never: an empty region has no workgroup)
  const uint64_t reach = ld_score_reach(t_region, a.window) + 1;
  const uint64_t p = wg - a.wg_begin[q];
  const uint64_t ti = p / reach, tj = ti + p % reach;
  if (ti >= t_region || tj >= t_region) return;
  const bool diag = ti == tj;
  const uint64_t ai = ti * kLdBlockTile, bj = tj * kLdBlockTile;   // the panels' first rows within the region
  const uint32_t W = a.window, max_bp = a.max_bp;
  // ---- under max_bp: the two panels' actual position ranges (wave 0: panel ti, wave 1: panel tj) ----
  if (max_bp && !diag) {
    uint32_t* const s_range = reinterpret_cast<uint32_t*>(s_ld);
    if (wid < 2) {
      const uint64_t local = (wid ? bj : ai) + lane;
      uint32_t pmin = 0xFFFFFFFFu, pmax = 0u;
      if (local < m) pmin = pmax = a.rows[r0 + local].pos;
#pragma unroll
      for (uint32_t d = 32; d; d >>= 1) {
        const uint32_t omin = __shfl_xor(pmin, d, 64), omax = __shfl_xor(pmax, d, 64);
        pmin = omin < pmin ? omin : pmin;
        pmax = omax > pmax ? omax : pmax;
      }
      if (lane == 0) { s_range[2 * wid] = pmin; s_range[2 * wid + 1] = pmax; }
    }
    __syncthreads();
    const uint32_t imin = s_range[0], imax = s_range[1], jmin = s_range[2], jmax = s_range[3];
    __syncthreads();   // (the staging writes over them)
    // (both panels hold a row of the region: min <= max in each)
    if ((jmin > imax && jmin - imax > max_bp) || (imin > jmax && imin - jmax > max_bp)) return;
  }
  ld_i32x4 acc[4];
  ld_block_products(a.cells, a.pitch, r0, m, ai, bj, diag, s_ld, acc);
  // ---- the sums per row of panel tj in LDS, in the staging buffer once every wave has read its fragments ----
  unsigned long long* const s_csum = reinterpret_cast<unsigned long long*>(s_ld);
  uint32_t* const s_ccnt = reinterpret_cast<uint32_t*>(s_ld + 8 * kLdBlockTile);
  if (!diag) {
    __syncthreads();
    if (threadIdx.x < kLdBlockTile) { s_csum[threadIdx.x] = 0ull; s_ccnt[threadIdx.x] = 0u; }
    __syncthreads();
  }
  // ---- epilogue: register g of the lane is the pair (a_first + g, b) ----
  const uint64_t a_first = ai + 16 * wid + 4 * (lane >> 4);
  const int64_t n = (int64_t)a.n_cols;
  int64_t sx[4] = {0, 0, 0, 0}, vx[4] = {0, 0, 0, 0};
  uint32_t px[4] = {0, 0, 0, 0};
  bool ex[4] = {false, false, false, false};
#pragma unroll
  for (int g = 0; g < 4; ++g)
    if (a_first + g < m) {
      ex[g] = ld_score_row(a, r0 + a_first + g, sx[g], vx[g]) == kLdScoreScored;
      if (max_bp) px[g] = a.rows[r0 + a_first + g].pos;
    }
  unsigned long long rsum[4] = {0, 0, 0, 0};
  uint32_t rcnt[4] = {0, 0, 0, 0};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint64_t b = bj + 16 * (uint32_t)t + (lane & 15);
    int64_t sy = 0, vy = 0;
    uint32_t py = 0;
    bool ey = false;
    if (b < m) {
      ey = ld_score_row(a, r0 + b, sy, vy) == kLdScoreScored;
      if (max_bp) py = a.rows[r0 + b].pos;
    }
    unsigned long long csum = 0;
    uint32_t ccnt = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const uint64_t ar = a_first + g;
      if (!ex[g] || !ey) continue;
      if (W && (ar > b ? ar - b : b - ar) > W) continue;
      if (max_bp && (px[g] > py ? px[g] - py : py - px[g]) > max_bp) continue;
      const int64_t cov = n * (int64_t)acc[t][g] - sx[g] * sy;
      const uint64_t mag = cov < 0 ? (uint64_t)0 - (uint64_t)cov : (uint64_t)cov;
      const uint64_t v = ld_score_q32(mag, (uint64_t)vx[g], (uint64_t)vy);
      rsum[g] += v; rcnt[g] += 1u;
      csum += v; ccnt += 1u;
    }
    if (!diag) {   // (workgroup-uniform)
#pragma unroll
      for (uint32_t d = 16; d < 64; d <<= 1) {
        csum += __shfl_xor(csum, d, 64);
        ccnt += __shfl_xor(ccnt, d, 64);
      }
      if (lane < 16 && ccnt) {
        atomicAdd(&s_csum[16 * (uint32_t)t + lane], csum);
        atomicAdd(&s_ccnt[16 * (uint32_t)t + lane], ccnt);
      }
    }
  }
  // ---- the rows of panel ti: over the 16 lanes of the row group, then one add per row ----
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (uint32_t d = 1; d < 16; d <<= 1) {
      rsum[g] += __shfl_xor(rsum[g], d, 64);
      rcnt[g] += __shfl_xor(rcnt[g], d, 64);
    }
    if ((lane & 15) == 0 && rcnt[g]) {   // (rcnt > 0: the row is eligible, so a_first + g < m)
      atomicAdd(&a.sums[kb + a_first + g], rsum[g]);
      atomicAdd(&a.n_pairs[kb + a_first + g], rcnt[g]);
    }
  }
  // ---- the rows of panel tj ----
  if (!diag) {
    __syncthreads();
    if (threadIdx.x < kLdBlockTile && s_ccnt[threadIdx.x]) {   // (a count > 0: the row is eligible, so bj + threadIdx.x < m)
      atomicAdd(&a.sums[kb + bj + threadIdx.x], s_csum[threadIdx.x]);
      atomicAdd(&a.n_pairs[kb + bj + threadIdx.x], s_ccnt[threadIdx.x]);
    }
  }
}

}  // namespace vsamd
