// k_assoc_matrix.hip.h -- trait-matrix association scan over the genotype matrix of a type-6 plan (vs_query_assoc_matrix): D Y, every
// table row against a wide panel of K traits, on the matrix cores.  Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_ld.hip.h"
#include "k_int128.hip.h"
#include "../host/assoc_matrix_host.hpp"

namespace vsamd {

// out[row * K + k] belongs to table row `row` and trait k.  The traits come as fixed-point integers q_k(s) = rint(y 2^f_k),
// |q| < 2^30, split on the host into four balanced base-256 digits (int8 "limbs": assoc_matrix_host.hpp), so
//   S = sum over the columns s of d(s) q_k(s) = acc0 + 2^8 acc1 + 2^16 acc2 + 2^24 acc3
// with acc_l = sum d(s) b_l(s) an int32 from v_mfma_i32_16x16x64_i8: |acc_l| <= 2 * 128 * n < 2^31 for n < 2^22, and
// |S| <= 2 * 2^30 * n <= 2^53 converts to double exactly.  No floating-point value is ever summed.
//   DOT   out = ldexp((double)S, -f_k)
//   CHI2  the score test of k_assoc.hip.h from exact integers: vx = n Sxx - Sx^2 (int64, the row's count record), cov = n S - Sx Sy_k
//         (128 bits, converted once: gram_to_double), vy_k = (double)(n Syy_k - Sy_k^2) from the host,
//         chi2 = (((double)n * cov) * cov) / ((double)vx * vy), no contraction; 0 when vx == 0 or vy <= 0.  2^f_k cancels.
//
// The shape is k_ld_block's with the second panel replaced.  A workgroup of four waves owns 64 table rows x one tile of 16 traits.
// It walks the columns in chunks of kLdChunk bytes: the 64 matrix rows are staged as in k_ld_band (16-byte loads, dosages on the
// way in, zeros for the rows past the table and the words past the pitch, LDS rows kLdStride apart), the tile's 4 x 16 limb rows
// -- [trait tile][limb][trait within the tile][pitch], 64 contiguous rows of the panel -- with plain 16-byte loads behind them:
// 128 x 272 = 34,816 bytes.  Wave w owns the row tile 16 w and four i32x4 accumulators, one per limb: per 64-column step one A
// read, four B reads, four MFMAs.  Fragment reads and the C/D map are k_ld_band's: register g of lane l is the cell (row
// 4 (l >> 4) + g of the wave's row tile, trait l & 15 of the tile).  Every accumulator is indexed statically: no scratch.
//
// Grid: one dimension, the trait tile fastest.  The workgroups in flight at one time then share a few 64-row panels of the matrix
// and all of the limb panel: the matrix -- rows x pitch bytes, the large operand -- streams from HBM once, the limb panel
// (ceil(K / 16) x 64 x pitch bytes) is re-read per row tile from L2 / the memory-side cache.  Measured against the row tile
// fastest: 3 to 17 % faster.
//
// Epilogue: every cell of the rows x K array is stored once with a plain 8-byte store, 16 consecutive cells per 16 lanes; a dropped or
// carrier-free row has an all-zero matrix row and an all-zero count record, so S = 0, vx = 0 and its cells are zeros: no memset, no
// atomic.  Guards: row < A, trait < K.
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage): <DOT> 61 VGPRs + 16 AGPRs, 52 SGPRs; <CHI2> 61
// VGPRs + 16 AGPRs, 51 SGPRs; both 34,816 bytes of static LDS, scratch 0, no spills, 4 waves a SIMD (four workgroups a CU by LDS).
constexpr uint32_t kAmRows = 64;                             // table rows of a workgroup: a 16-row tile per wave
constexpr uint32_t kAmPanelRows = kAmTileRows;               // limb rows of a trait tile: 4 limbs x 16 traits
constexpr uint32_t kAmLds = (kAmRows + kAmPanelRows) * kLdStride;

struct AssocMatrixArgs {
  const uint8_t* cells;      // the genotype matrix [A x pitch]
  const int8_t* panel;       // [tiles x 64 x pitch]
  uint64_t A;
  uint32_t pitch;            // a multiple of 16
  uint32_t n_cols;           // n of the statistic
  uint32_t K, tiles;         // tiles = ceil(K / 16)
  const int64_t* sy;         // [K] sum of q (CHI2)
  const double* vy;          // [K] (double)(n Syy - Sy^2) (CHI2)
  const int32_t* shift;      // [K] f_k (DOT)
  const uint4* counts;       // {carriers, alt_alleles, hom_alt, phased} per table row (CHI2)
  double* out;               // [A x K]
};

__device__ __forceinline__ double am_chi2(int64_t n, int64_t S, const uint4 rec, int64_t sy, double vy) {
#pragma clang fp contract(off)
  const int64_t sx = (int64_t)rec.y, sxx = (int64_t)rec.y + 2ll * (int64_t)rec.z;
  const int64_t vx = n * sxx - sx * sx;
  if (vx == 0 || !(vy > 0.0)) return 0.0;
  const double cov = gram_to_double((__int128)n * S - (__int128)sx * sy);
  return (((double)n * cov) * cov) / ((double)vx * vy);
}

template <bool CHI2>
__global__ void __launch_bounds__(256) k_assoc_matrix(AssocMatrixArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_am[kAmLds];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint32_t tile = blockIdx.x % a.tiles;
  const uint64_t row0 = (uint64_t)(blockIdx.x / a.tiles) * kAmRows;
  const int8_t* const ptile = a.panel + (uint64_t)tile * kAmPanelRows * a.pitch;
  constexpr uint32_t words = (kAmRows + kAmPanelRows) * (kLdChunk / 16);
  constexpr uint32_t b_base = kAmRows * kLdStride;
  ld_i32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = ld_i32x4{0, 0, 0, 0};
  const uint32_t frag = (lane & 15) * kLdStride + 16 * (lane >> 4);   // the lane's fragment of k-step 0 within a 16-row tile
  for (uint32_t c0 = 0; c0 < a.pitch; c0 += kLdChunk) {
    if (c0) __syncthreads();   // (the chunk before this one has been read)
    // ---- staging: 16 bytes per thread and step; the matrix rows as dosages, the limb rows as they are ----
#pragma unroll 4
    for (uint32_t i = threadIdx.x; i < words; i += 256) {
      const uint32_t r = i >> 4, col = c0 + 16 * (i & 15);
      uint4 v{0u, 0u, 0u, 0u};
      if (col < a.pitch) {
        if (r < kAmRows) {
          if (row0 + r < a.A) v = ld_load_dosages(a.cells + (row0 + r) * a.pitch + col);
        } else v = *reinterpret_cast<const uint4*>(ptile + (uint64_t)(r - kAmRows) * a.pitch + col);
      }
      *reinterpret_cast<uint4*>(s_am + r * kLdStride + 16 * (i & 15)) = v;
    }
    __syncthreads();
    // ---- products: four MFMAs per 64-column step, one per limb ----
    const uint32_t left = a.pitch - c0;
    const uint32_t ksteps = left >= kLdChunk ? kLdChunk / 64 : (left + 63) / 64;
    for (uint32_t ks = 0; ks < ksteps; ++ks) {
      const ld_i32x4 fa = *reinterpret_cast<const ld_i32x4*>(s_am + 16 * wid * kLdStride + frag + 64 * ks);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const ld_i32x4 fb = *reinterpret_cast<const ld_i32x4*>(s_am + b_base + (uint32_t)t * 16 * kLdStride + frag + 64 * ks);
        acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa, fb, acc[t], 0, 0, 0);
      }
    }
  }
  // ---- epilogue: register g of the lane is the cell (row_first + g, trait) ----
  const uint32_t trait = tile * kAmTraitTile + (lane & 15);
  if (trait >= a.K) return;
  const uint64_t row_first = row0 + 16 * wid + 4 * (lane >> 4);
  const int64_t n = (int64_t)a.n_cols;
  const int64_t sy = CHI2 ? a.sy[trait] : 0;
  const double vy = CHI2 ? a.vy[trait] : 0.0;
  const int f = CHI2 ? 0 : a.shift[trait];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const uint64_t row = row_first + g;
    if (row >= a.A) continue;
    const int64_t S = (int64_t)acc[0][g] + (int64_t)acc[1][g] * 256 + (int64_t)acc[2][g] * 65536 + (int64_t)acc[3][g] * 16777216;
    a.out[row * a.K + trait] = CHI2 ? am_chi2(n, S, a.counts[row], sy, vy) : ldexp((double)S, -f);
  }
}

}  // namespace vsamd
