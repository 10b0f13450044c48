// k_ld_block.hip.h -- the full LD block of every region over the genotype matrix of a type-6 plan (vs_query_ld_matrix): D D^T per
// region, square, where k_ld_band gives the band of the whole table.
// Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_ld.hip.h"

namespace vsamd {

// Region q owns the table rows row_begin[q] .. + m_q (m_q = row_count[q], dropped rows included) and the block of m_q x m_q
// four-byte cells at out[block_begin[q] + a * m_q + b] for the rows (row_begin[q] + a, row_begin[q] + b): Sxy as int32 (DOT) or the
// squared dosage correlation as float (R2), formed exactly as k_ld_band forms a band cell (ld_r2) -- the full symmetric square,
// diagonal included.
//
// k_ld_block_scan (one workgroup) turns the per-region row counts into block_begin (the exclusive scan of m_q^2) and wg_begin (the
// exclusive scan of the workgroups a region takes: t (t + 1) / 2 pairs of 64-row tiles, t = ceil(m_q / 64)) and leaves the two totals
// and the largest m_q for the host, which holds them against the size limit before it allocates the cells.
//
// k_ld_block: a workgroup of four waves owns one tile pair (ti <= tj) of one region.  It finds the region by bisection over wg_begin
// (an empty region has no workgroup: the last q with wg_begin[q] <= blockIdx.x is the owner) and the pair from the index p within the
// region: pairs are numbered by tj, p = tj (tj + 1) / 2 + ti.  It walks the columns in chunks of kLdChunk bytes; the 64 rows of
// panel ti and -- off the diagonal -- the 64 rows of panel tj are staged as in k_ld_band (16-byte loads, dosages on the way in, zeros
// for the rows past m_q and the words past the pitch, LDS rows kLdStride apart): 128 x 272 = 34,816 bytes.  Wave w owns the row
// tile 16 w of panel ti and four i32x4 accumulators, one per 16-row tile of panel tj: per 64-column step one A read, four B reads,
// four v_mfma_i32_16x16x64_i8.  Fragment reads and the C/D map are k_ld_band's: register g of lane l is the cell (row 4 (l >> 4) + g
// of the wave's row tile, row l & 15 of the column tile).  Every accumulator is indexed statically: no scratch.
//
// Epilogue: the lane forms its cells with a, b < m_q and stores (a, b); off the diagonal it stores the same word at (b, a) as well,
// four consecutive cells of block row b.  A diagonal pair holds the whole 64 x 64 tile, both triangles, and stores each cell once.
// Every cell of every block is stored exactly once with plain vector stores: no memset, no atomic.
//
// The prologue (bisection, row_count, row_begin, block_begin) depends on blockIdx.x alone and comes in front of every store of the
// kernel: the compiler keeps it in SGPRs and reads with scalar loads, once per workgroup, not per lane.
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage): DESIGN 5k.
constexpr uint32_t kLdBlockTile = 64;                                  // rows of a panel: a 16-row tile per wave
constexpr uint32_t kLdBlockLds = 2 * kLdBlockTile * kLdStride;         // both panels
constexpr uint32_t kLdBlockScanThreads = 1024, kLdBlockScanItems = 4;

struct LdBlockArgs {
  const uint8_t* cells;          // the genotype matrix [A x pitch]
  uint32_t pitch;                // a multiple of 16
  uint32_t n_cols;               // n of the correlation
  uint64_t Q;
  const uint64_t* row_begin;     // per region, in the caller's order
  const uint64_t* row_count;
  const uint64_t* block_begin;   // [Q + 1]
  const uint64_t* wg_begin;      // [Q + 1]
  const uint4* counts;           // {carriers, alt_alleles, hom_alt, phased} per table row (R2)
  uint32_t* out;                 // the blocks: int32 (DOT) or float (R2)
};

__host__ __device__ __forceinline__ uint64_t ld_block_pairs(uint64_t m) {
  const uint64_t t = (m + kLdBlockTile - 1) / kLdBlockTile;
  return t * (t + 1) / 2;
}

// The two exclusive scans of a batch's per-region row counts by one workgroup of kLdBlockScanThreads threads: first[q], second[q] =
// the sums of fa(m) and fb(m) over the regions in front of q; [Q]: the totals.  summary = {total of fa, total of fb, largest m, 0}.
// k_ld_block_scan and k_ld_score_scan (k_ld_score.hip.h) share it.
template <class FA, class FB>
__device__ __forceinline__ void ld_region_scans(const uint64_t* __restrict__ row_count, uint64_t Q, uint64_t* __restrict__ first, uint64_t* __restrict__ second,
                                                uint64_t* __restrict__ summary, FA fa, FB fb) {
  __shared__ uint64_t s_cells[kLdBlockScanThreads / 64], s_wgs[kLdBlockScanThreads / 64], s_max[kLdBlockScanThreads / 64];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint64_t carry_c = 0, carry_w = 0, largest = 0;
  for (uint64_t base = 0; base < Q; base += (uint64_t)kLdBlockScanThreads * kLdBlockScanItems) {
    const uint64_t q0 = base + (uint64_t)threadIdx.x * kLdBlockScanItems;
    uint64_t m[kLdBlockScanItems], sc = 0, sw = 0;
#pragma unroll
    for (uint32_t i = 0; i < kLdBlockScanItems; ++i) {
      m[i] = q0 + i < Q ? row_count[q0 + i] : 0;
      sc += fa(m[i]); sw += fb(m[i]);
      largest = m[i] > largest ? m[i] : largest;
    }
    uint64_t ic = sc, iw = sw;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint64_t tc = __shfl_up(ic, d, 64), tw = __shfl_up(iw, d, 64);
      if (lane >= d) { ic += tc; iw += tw; }
    }
    if (lane == 63) { s_cells[wid] = ic; s_wgs[wid] = iw; }
    __syncthreads();
    uint64_t before_c = 0, before_w = 0, total_c = 0, total_w = 0;
#pragma unroll
    for (uint32_t w = 0; w < kLdBlockScanThreads / 64; ++w) {
      if (w < wid) { before_c += s_cells[w]; before_w += s_wgs[w]; }
      total_c += s_cells[w]; total_w += s_wgs[w];
    }
    __syncthreads();
    uint64_t ec = carry_c + before_c + ic - sc, ew = carry_w + before_w + iw - sw;
#pragma unroll
    for (uint32_t i = 0; i < kLdBlockScanItems; ++i) {
      if (q0 + i < Q) { first[q0 + i] = ec; second[q0 + i] = ew; }
      ec += fa(m[i]); ew += fb(m[i]);
    }
    carry_c += total_c; carry_w += total_w;
  }
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) {
    const uint64_t o = __shfl_xor(largest, d, 64);
    largest = o > largest ? o : largest;
  }
  if (lane == 0) s_max[wid] = largest;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < kLdBlockScanThreads / 64; ++w) largest = s_max[w] > largest ? s_max[w] : largest;
    first[Q] = carry_c; second[Q] = carry_w;
    summary[0] = carry_c; summary[1] = carry_w; summary[2] = largest; summary[3] = 0;
  }
}

// block_begin[q], wg_begin[q] = the sums of m^2 and of the tile pairs over the regions in front of q; [Q]: the totals.
// summary = {cells, workgroups, largest m, 0}.
__global__ void __launch_bounds__(kLdBlockScanThreads) k_ld_block_scan(const uint64_t* __restrict__ row_count, uint64_t Q, uint64_t* __restrict__ block_begin,
                                                                        uint64_t* __restrict__ wg_begin, uint64_t* __restrict__ summary) {
  ld_region_scans(row_count, Q, block_begin, wg_begin, summary, [](uint64_t m) { return m * m; }, [](uint64_t m) { return ld_block_pairs(m); });
}

// The products of a workgroup's tile pair: acc[t] = the wave's 16-row tile of panel ti (first row ai within the region) against the
// 16-row tile t of panel tj (first row bj), summed over all columns.  k_ld_block and k_ld_score (k_ld_score.hip.h) share it:
// staging, fragments and MFMAs are one piece of code, the epilogues differ.
__device__ __forceinline__ void ld_block_products(const uint8_t* __restrict__ cells, uint32_t pitch, uint64_t r0, uint64_t m, uint64_t ai, uint64_t bj, bool diag,
                                                  uint8_t* s_ld, ld_i32x4 (&acc)[4]) {
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint32_t words = (diag ? kLdBlockTile : 2 * kLdBlockTile) * (kLdChunk / 16);
  const uint32_t b_base = diag ? 0u : kLdBlockTile * kLdStride;    // panel tj in LDS
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = ld_i32x4{0, 0, 0, 0};
  const uint32_t frag = (lane & 15) * kLdStride + 16 * (lane >> 4);   // the lane's fragment of k-step 0 within a 16-row tile
  for (uint32_t c0 = 0; c0 < pitch; c0 += kLdChunk) {
    if (c0) __syncthreads();   // (the chunk before this one has been read)
    // ---- staging: 16 bytes per thread and step, dosages on the way in ----
#pragma unroll 4
    for (uint32_t i = threadIdx.x; i < words; i += 256) {
      const uint32_t r = i >> 4, col = c0 + 16 * (i & 15);
      const uint64_t local = (r < kLdBlockTile ? ai : bj - kLdBlockTile) + r;   // the row within the region
      uint4 v{0u, 0u, 0u, 0u};
      if (local < m && col < pitch) v = ld_load_dosages(cells + (r0 + local) * pitch + col);
      *reinterpret_cast<uint4*>(s_ld + r * kLdStride + 16 * (i & 15)) = v;
    }
    __syncthreads();
    // ---- products: four MFMAs per 64-column step ----
    const uint32_t left = pitch - c0;
    const uint32_t ksteps = left >= kLdChunk ? kLdChunk / 64 : (left + 63) / 64;
    for (uint32_t ks = 0; ks < ksteps; ++ks) {
      const ld_i32x4 fa = *reinterpret_cast<const ld_i32x4*>(s_ld + 16 * wid * kLdStride + frag + 64 * ks);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const ld_i32x4 fb = *reinterpret_cast<const ld_i32x4*>(s_ld + b_base + (uint32_t)t * 16 * kLdStride + frag + 64 * ks);
        acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa, fb, acc[t], 0, 0, 0);
      }
    }
  }
}

template <bool R2>
__global__ void __launch_bounds__(256) k_ld_block(LdBlockArgs a) {
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
  const uint64_t m = a.row_count[q], r0 = a.row_begin[q];
  // ---- the tile pair: p = tj (tj + 1) / 2 + ti, ti <= tj ----
  const uint64_t p = wg - a.wg_begin[q];
  if (p >= ld_block_pairs(m)) return;   // (never: wg_begin is the scan of exactly these counts)
  uint64_t tj = (uint64_t)((__builtin_sqrt((double)(8 * p + 1)) - 1.0) * 0.5);
  while (tj * (tj + 1) / 2 > p) --tj;
  while ((tj + 1) * (tj + 2) / 2 <= p) ++tj;
  const uint64_t ti = p - tj * (tj + 1) / 2;
  const bool diag = ti == tj;
  const uint64_t ai = ti * kLdBlockTile, bj = tj * kLdBlockTile;   // the panels' first rows within the region
  ld_i32x4 acc[4];
  ld_block_products(a.cells, a.pitch, r0, m, ai, bj, diag, s_ld, acc);
  // ---- epilogue: register g of the lane is the cell (a_first + g, b) ----
  const uint64_t a_first = ai + 16 * wid + 4 * (lane >> 4);
  const int64_t n = (int64_t)a.n_cols;
  int64_t sx[4] = {0, 0, 0, 0}, vx[4] = {0, 0, 0, 0};
  if (R2) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
      if (a_first + g < m) ld_moments(a.counts[r0 + a_first + g], n, sx[g], vx[g]);
  }
  uint32_t* const block = a.out + a.block_begin[q];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint64_t b = bj + 16 * (uint32_t)t + (lane & 15);
    if (b >= m) continue;
    int64_t sy = 0, vy = 0;
    if (R2) ld_moments(a.counts[r0 + b], n, sy, vy);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const uint64_t ar = a_first + g;
      if (ar >= m) continue;
      const uint32_t out = R2 ? __float_as_uint(ld_r2(n, acc[t][g], sx[g], sy, vx[g], vy)) : (uint32_t)acc[t][g];
      block[ar * m + b] = out;
      if (!diag) block[b * m + ar] = out;
    }
  }
}

}  // namespace vsamd
