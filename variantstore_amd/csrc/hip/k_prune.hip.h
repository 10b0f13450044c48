// k_prune.hip.h -- greedy LD pruning of every region over the genotype matrix of a type-6 plan (vs_query_ld_prune): the band's
// products turned into exact hit masks, then one sequential walk per region.
// Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_ld.hip.h"

namespace vsamd {

// The pair of table rows (i, j) is a HIT when v_i > 0, v_j > 0 and cov^2 2^20 > T v_i v_j, cov = n Sxy - Sx Sy, v = n Sxx - Sx^2
// (ld_moments), T the threshold in 0 .. 2^20: r^2 > T / 2^20 decided in unsigned 128-bit integers, no floating-point value takes
// part.  With n < 2^21: |cov| < 2^44, v < 2^44, both sides below 2^108.
//
// k_prune_hits is k_ld_band with a third epilogue: the same 64-row workgroups, halo, staging and MFMAs (ld_band_products).  Where
// the band stores a four-byte cell, a pair yields one bit: hits[i * words + (k >> 5)] bit k & 31 for the pair (i, i + 1 + k),
// k < window, words = ceil(window / 32); 0 for i + 1 + k >= A and in the padding bits.  max_bp (nonzero) clears the pairs whose
// positions are further apart; eligibility is not applied here.  The workgroup's 64 mask rows are assembled in LDS -- the staging
// buffer, free once the products are done -- with ds_or, then every word is stored once with plain vector stores: no HBM atomic,
// no memset.
//
// k_prune_scan (one workgroup) turns the per-region row counts into keep_begin, their exclusive scan, and leaves the total for the
// host, which holds it against the size limit before the state bytes are allocated.
//
// k_prune_greedy: one wave per region, all regions in one launch.  The walk's state is a 256-bit register `blocked`, wave-uniform
// (eight SGPRs): bit d = table row i + d is blocked by a kept row.  At row i: the row is kept when it is eligible and bit 0 is
// clear; the register moves on by one bit; a kept row ORs its mask in (bit k of hits[i] is row i + 1 + k).  The 64 lanes load the
// masks and the eligibility of 64 rows at a time, the next batch in front of the chain over this one, and the chain takes them with
// v_readlane: it never waits on memory.  A batch's 64 state bytes are written together, a byte per lane.  The walk starts with an
// empty register at the region's first row, so rows in front of it never block; the bits of rows past its end are never looked at.
// An empty region writes n_kept = 0 and nothing else.  Every byte of `state` is stored exactly once.
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage): DESIGN 5n.
constexpr uint32_t kPruneMaxWords = kLdMaxWindow / 32;   // mask words of a row at the largest window
constexpr uint32_t kPruneScanThreads = 1024, kPruneScanItems = 4;
constexpr uint32_t kPruneThresholdOne = 1u << 20;        // T of r^2 = 1
constexpr uint8_t kPrunePruned = 0, kPruneKept = 1, kPruneIneligible = 2, kPruneDropped = 3;   // VS_PRUNE_*

struct PruneHitArgs {
  LdArgs ld;                // cells, A, pitch, n_cols, window, n_tiles, counts as for the band (band unused)
  const VariantRow* rows;   // the table: positions (max_bp)
  uint32_t* hits;           // [A x words]
  uint32_t words;           // ceil(window / 32)
  uint32_t max_bp;          // 0: no limit
  uint32_t threshold;       // T, 0 .. 2^20
};

struct PruneGreedyArgs {
  uint64_t Q;
  const uint64_t* row_begin;    // per region, in the caller's order
  const uint64_t* row_count;
  const uint64_t* keep_begin;   // [Q + 1]
  const VariantRow* rows;       // the table: the duplicate rule's flag
  const uint4* counts;          // {carriers, alt_alleles, hom_alt, phased} per table row
  const uint32_t* hits;         // [A x words]
  uint32_t words;
  uint32_t n_cols;
  uint32_t min_ac, max_ac;
  uint8_t* state;               // [keep_begin[Q]]
  uint64_t* n_kept;             // [Q]
};

__device__ __forceinline__ bool prune_hit(int64_t n, int32_t sxy, int64_t sx, int64_t sy, int64_t vx, int64_t vy, uint32_t T) {
  if (vx <= 0 || vy <= 0) return false;
  const int64_t cov = n * (int64_t)sxy - sx * sy;
  const uint64_t mag = cov < 0 ? (uint64_t)0 - (uint64_t)cov : (uint64_t)cov;
  const unsigned __int128 lhs = ((unsigned __int128)mag * mag) << 20;
  const unsigned __int128 rhs = (unsigned __int128)(uint64_t)vx * (uint64_t)vy * T;
  return lhs > rhs;
}

template <int MAXT>
__global__ void __launch_bounds__(256) k_prune_hits(PruneHitArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_ld[];
  const LdArgs& a = p.ld;
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t row0 = (uint64_t)blockIdx.x * kLdRows;
  if (row0 >= a.A) return;
  const uint32_t W = a.window;
  const uint64_t iw = row0 + 16 * wid;               // the wave's row tile
  ld_i32x4 acc[MAXT];
  const uint32_t ntw = ld_band_products<MAXT>(a, s_ld, acc);
  // ---- the workgroup's mask rows in LDS: [kLdRows][kPruneMaxWords], in the staging buffer once every wave has read its fragments ----
  uint32_t* const s_mask = reinterpret_cast<uint32_t*>(s_ld);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < kLdRows * kPruneMaxWords; i += 256) s_mask[i] = 0u;
  __syncthreads();
  // ---- epilogue: register g of the lane is the pair (row iw + 4 (lane >> 4) + g, column tile row lane & 15) ----
  const uint32_t r_first = 16 * wid + 4 * (lane >> 4);   // the row within the block
  const uint64_t i_first = row0 + r_first;
  const int64_t n = (int64_t)a.n_cols;
  int64_t sx[4] = {0, 0, 0, 0}, vx[4] = {0, 0, 0, 0};
  uint32_t px[4] = {0, 0, 0, 0};
#pragma unroll
  for (int g = 0; g < 4; ++g)
    if (i_first + g < a.A) {
      ld_moments(a.counts[i_first + g], n, sx[g], vx[g]);
      if (p.max_bp) px[g] = p.rows[i_first + g].pos;
    }
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    if ((uint32_t)t >= ntw) continue;
    const uint64_t j = iw + 16 * (uint32_t)t + (lane & 15);
    if (j >= a.A) continue;
    int64_t sy = 0, vy = 0;
    ld_moments(a.counts[j], n, sy, vy);
    const uint32_t py = p.max_bp ? p.rows[j].pos : 0u;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const uint64_t i = i_first + g;
      if (j <= i || j - i > W) continue;   // (j < A and i < j: row i is a row of the table)
      if (p.max_bp && (px[g] > py ? px[g] - py : py - px[g]) > p.max_bp) continue;
      if (!prune_hit(n, acc[t][g], sx[g], sy, vx[g], vy, p.threshold)) continue;
      const uint32_t k = (uint32_t)(j - i - 1);
      atomicOr(&s_mask[(r_first + g) * kPruneMaxWords + (k >> 5)], 1u << (k & 31));
    }
  }
  __syncthreads();
  // ---- every word of the block's rows, once ----
  const uint32_t words = p.words;
  for (uint32_t i = threadIdx.x; i < kLdRows * words; i += 256) {
    const uint32_t r = i / words, w = i - r * words;
    if (row0 + r < a.A) p.hits[(row0 + r) * words + w] = s_mask[r * kPruneMaxWords + w];
  }
}

// keep_begin[q] = the sum of row_count over the regions in front of q; keep_begin[Q] and summary[0]: the total.
__global__ void __launch_bounds__(kPruneScanThreads) k_prune_scan(const uint64_t* __restrict__ row_count, uint64_t Q, uint64_t* __restrict__ keep_begin,
                                                                  uint64_t* __restrict__ summary) {
  __shared__ uint64_t s_sum[kPruneScanThreads / 64];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint64_t carry = 0;
  for (uint64_t base = 0; base < Q; base += (uint64_t)kPruneScanThreads * kPruneScanItems) {
    const uint64_t q0 = base + (uint64_t)threadIdx.x * kPruneScanItems;
    uint64_t m[kPruneScanItems], s = 0;
#pragma unroll
    for (uint32_t i = 0; i < kPruneScanItems; ++i) {
      m[i] = q0 + i < Q ? row_count[q0 + i] : 0;
      s += m[i];
    }
    uint64_t inc = s;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint64_t t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    if (lane == 63) s_sum[wid] = inc;
    __syncthreads();
    uint64_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kPruneScanThreads / 64; ++w) {
      if (w < wid) before += s_sum[w];
      total += s_sum[w];
    }
    __syncthreads();
    uint64_t e = carry + before + inc - s;
#pragma unroll
    for (uint32_t i = 0; i < kPruneScanItems; ++i) {
      if (q0 + i < Q) keep_begin[q0 + i] = e;
      e += m[i];
    }
    carry += total;
  }
  if (threadIdx.x == 0) { keep_begin[Q] = carry; summary[0] = carry; summary[1] = 0; }
}

// The masks and the verdict a row starts with, for the lane's row of a batch: 0 (a candidate: kept or pruned by the walk),
// kPruneIneligible or kPruneDropped.  Lanes past the region's end: zeros and kPruneIneligible (never looked at).
__device__ __forceinline__ void prune_load(const PruneGreedyArgs& a, uint64_t r0, uint64_t m, uint64_t local, uint32_t (&h)[kPruneMaxWords], uint32_t& code) {
#pragma unroll
  for (uint32_t w = 0; w < kPruneMaxWords; ++w) h[w] = 0u;
  code = kPruneIneligible;
  if (local >= m) return;
  const uint64_t row = r0 + local;
#pragma unroll
  for (uint32_t w = 0; w < kPruneMaxWords; ++w)
    if (w < a.words) h[w] = a.hits[row * a.words + w];
  const uint4 c = a.counts[row];
  int64_t sx, v;
  ld_moments(c, (int64_t)a.n_cols, sx, v);
  if (a.rows[row].count_flags & kRowDropped) code = kPruneDropped;
  else if (v > 0 && c.y >= a.min_ac && c.y <= a.max_ac) code = 0u;
}

__global__ void __launch_bounds__(64) k_prune_greedy(PruneGreedyArgs a) {
  const uint64_t q = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  const uint64_t m = a.row_count[q], r0 = a.row_begin[q];
  uint8_t* const out = a.state + a.keep_begin[q];
  uint32_t blocked[kPruneMaxWords];
#pragma unroll
  for (uint32_t w = 0; w < kPruneMaxWords; ++w) blocked[w] = 0u;
  uint64_t total = 0;
  uint32_t h[kPruneMaxWords], code;
  prune_load(a, r0, m, lane, h, code);
  for (uint64_t base = 0; base < m; base += 64) {
    uint32_t hn[kPruneMaxWords], coden;
    prune_load(a, r0, m, base + 64 + lane, hn, coden);   // the next batch, in front of the chain over this one
    const uint32_t cnt = m - base < 64 ? (uint32_t)(m - base) : 64u;
    uint64_t kept_mask = 0;
    for (uint32_t d = 0; d < cnt; ++d) {
      const bool kept = __builtin_amdgcn_readlane((int)code, (int)d) == 0 && !(blocked[0] & 1u);
#pragma unroll
      for (uint32_t w = 0; w + 1 < kPruneMaxWords; ++w) blocked[w] = (blocked[w] >> 1) | (blocked[w + 1] << 31);
      blocked[kPruneMaxWords - 1] >>= 1;
      if (kept) {
        kept_mask |= 1ull << d;
#pragma unroll
        for (uint32_t w = 0; w < kPruneMaxWords; ++w) blocked[w] |= (uint32_t)__builtin_amdgcn_readlane((int)h[w], (int)d);
      }
    }
    if (lane < cnt) out[base + lane] = code ? (uint8_t)code : (uint8_t)((kept_mask >> lane) & 1ull);
    total += (uint64_t)__builtin_popcountll(kept_mask);
#pragma unroll
    for (uint32_t w = 0; w < kPruneMaxWords; ++w) h[w] = hn[w];
    code = coden;
  }
  if (lane == 0) a.n_kept[q] = total;
}

}  // namespace vsamd
