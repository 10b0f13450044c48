// k_ld.hip.h -- banded LD over the genotype matrix of a type-6 plan (vs_query_ld_band): every table row against the next W rows.
// Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_matrix.hip.h"

namespace vsamd {

// band[i * W + k] belongs to the pair of table rows (i, j = i + 1 + k): Sxy = sum over the columns of d_i * d_j, d = the dosage
// popcount(cell & 6) of a genotype-matrix cell (0, 1 or 2) -- the band of the Gram matrix D D^T.  Dosages are bytes and the
// products are summed in int32 on the matrix cores (v_mfma_i32_16x16x64_i8): exact.  DOT stores Sxy; R2 forms the squared dosage
// correlation from it and the two rows' count records (Sx = alt_alleles, Sxx = alt_alleles + 2 hom_alt) in 64-bit integers and
// doubles, cast to float at the end.
//
// A workgroup of four waves owns kLdRows consecutive table rows i0 .. and reads the halo of W rows behind them (rounded up to whole
// 16-row tiles).  It walks the columns in chunks of kLdChunk bytes: the chunk of all its rows is staged into LDS with 16-byte
// loads, a row's 16 words side by side, converted to dosages on the way in; rows beyond A and the words beyond the pitch are zeros
// (the matrix's own padding bytes are 0 already).  LDS rows are kLdStride = kLdChunk + 16 bytes apart: the 16-byte fragment reads
// of 16 consecutive rows start 4 banks apart and cover all 64 banks once.
//
// Wave w owns the 16-row tile i0 + 16 w and keeps one i32x4 accumulator per 16 x 16 column tile that meets the band: tile offsets
// t = 0 .. (W + 15) / 16, the rows i0 + 16 (w + t) ...  Per 64-column step it reads its A fragment once -- lane l: the 16 bytes at
// [row l & 15][16 (l >> 4) ..] of the row tile -- and per column tile the same read of that tile's rows as B.  Both operands index
// k alike and a dot product does not care about the order of k, so the product holds whatever the instruction's own k map is;
// the C/D map does matter: register g of lane l is row 4 (l >> 4) + g of the row tile, column l & 15 of the column tile.
// MAXT bounds the accumulators at compile time (5: windows up to 64, 17: up to 256); the loops over them are unrolled, every
// accumulator is indexed statically and the kernel uses no scratch.
//
// Every cell of the band is stored exactly once, with plain vector stores: the pairs with j < A by the lane that holds them, the
// cells with i + 1 + k >= A as zeros by the workgroup that owns row i.  No memset, no atomic.
constexpr uint32_t kLdRows = 64;                   // rows a workgroup owns: a 16-row tile per wave
constexpr uint32_t kLdChunk = 256;                 // column bytes staged per step: four MFMA k-steps
constexpr uint32_t kLdStride = kLdChunk + 16;      // bytes from an LDS row to the next
constexpr uint32_t kLdMaxWindow = 256;
constexpr uint32_t kLdSmallTiles = 5, kLdMaxTiles = kLdMaxWindow / 16 + 1;   // column tiles of a row tile: W <= 64, W <= 256

struct LdArgs {
  const uint8_t* cells;   // the genotype matrix [A x pitch]
  uint64_t A;
  uint32_t pitch;         // a multiple of 16
  uint32_t n_cols;        // n of the correlation
  uint32_t window;        // 1 .. kLdMaxWindow
  uint32_t n_tiles;       // (window + 15) / 16 + 1
  const uint4* counts;    // {carriers, alt_alleles, hom_alt, phased} per table row (R2)
  uint32_t* band;         // [A x window] int32 (DOT) or float (R2)
};

typedef int ld_i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t ld_dosage4(uint32_t w) { return ((w >> 1) & 0x01010101u) + ((w >> 2) & 0x01010101u); }

// 16 cells of a matrix row as dosages (p: 16-byte aligned)
__device__ __forceinline__ uint4 ld_load_dosages(const uint8_t* p) {
  uint4 v = *reinterpret_cast<const uint4*>(p);
  v.x = ld_dosage4(v.x); v.y = ld_dosage4(v.y); v.z = ld_dosage4(v.z); v.w = ld_dosage4(v.w);
  return v;
}

// n Sxx - Sx^2 of a row from its count record
__device__ __forceinline__ void ld_moments(const uint4 c, int64_t n, int64_t& sx, int64_t& v) {
  sx = (int64_t)c.y;
  v = n * (int64_t)(c.y + 2ull * c.z) - sx * sx;
}

// r^2 of a pair from Sxy and the two rows' moments: exact 64-bit integers, three double operations, one cast; 0 beside a flat row
__device__ __forceinline__ float ld_r2(int64_t n, int32_t sxy, int64_t sx, int64_t sy, int64_t vx, int64_t vy) {
  if (vx == 0 || vy == 0) return 0.0f;
  const double cov = (double)(n * (int64_t)sxy - sx * sy);
  return (float)(cov * cov / ((double)vx * (double)vy));
}

// The products of a workgroup of the band: acc[t] = the wave's 16-row tile against column tile t, summed over all columns.  Returns
// the column tiles of this wave that hold a row of the table at all (wave-uniform).  k_ld_band and k_prune_hits (k_prune.hip.h)
// share it: staging, fragments and MFMAs are one piece of code, the epilogues differ.
template <int MAXT>
__device__ __forceinline__ uint32_t ld_band_products(const LdArgs& a, uint8_t* s_ld, ld_i32x4 (&acc)[MAXT]) {
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t row0 = (uint64_t)blockIdx.x * kLdRows;
  const uint32_t nt = a.n_tiles;
  const uint32_t n_rows = kLdRows + 16 * (nt - 1);   // LDS rows: the block's and the halo's
  const uint32_t words = n_rows * (kLdChunk / 16);
  const uint64_t iw = row0 + 16 * wid;               // the wave's row tile
  // column tiles of this wave that hold a row of the table at all (wave-uniform)
  const uint32_t ntw = iw >= a.A ? 0u : (uint32_t)((a.A - iw + 15) / 16 < nt ? (a.A - iw + 15) / 16 : nt);
#pragma unroll
  for (int t = 0; t < MAXT; ++t) acc[t] = ld_i32x4{0, 0, 0, 0};
  const uint32_t frag = (16 * wid + (lane & 15)) * kLdStride + 16 * (lane >> 4);   // the lane's A fragment of k-step 0
  for (uint32_t c0 = 0; c0 < a.pitch; c0 += kLdChunk) {
    if (c0) __syncthreads();   // (the chunk before this one has been read)
    // ---- staging: 16 bytes per thread and step, dosages on the way in ----
#pragma unroll 4
    for (uint32_t i = threadIdx.x; i < words; i += 256) {
      const uint32_t r = i >> 4, col = c0 + 16 * (i & 15);
      const uint64_t g = row0 + r;
      uint4 v{0u, 0u, 0u, 0u};
      if (g < a.A && col < a.pitch) v = ld_load_dosages(a.cells + g * a.pitch + col);
      *reinterpret_cast<uint4*>(s_ld + r * kLdStride + 16 * (i & 15)) = v;
    }
    __syncthreads();
    // ---- products: one MFMA per column tile and 64-column step ----
    const uint32_t left = a.pitch - c0;
    const uint32_t ksteps = left >= kLdChunk ? kLdChunk / 64 : (left + 63) / 64;
    for (uint32_t ks = 0; ks < ksteps; ++ks) {
      const ld_i32x4 fa = *reinterpret_cast<const ld_i32x4*>(s_ld + frag + 64 * ks);
#pragma unroll
      for (int t = 0; t < MAXT; ++t)
        if ((uint32_t)t < ntw) {
          const ld_i32x4 fb = *reinterpret_cast<const ld_i32x4*>(s_ld + frag + 64 * ks + (uint32_t)t * 16 * kLdStride);
          acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa, fb, acc[t], 0, 0, 0);
        }
    }
  }
  return ntw;
}

template <int MAXT, bool R2>
__global__ void __launch_bounds__(256) k_ld_band(LdArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_ld[];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t row0 = (uint64_t)blockIdx.x * kLdRows;
  if (row0 >= a.A) return;
  const uint32_t W = a.window;
  const uint64_t iw = row0 + 16 * wid;               // the wave's row tile
  ld_i32x4 acc[MAXT];
  const uint32_t ntw = ld_band_products<MAXT>(a, s_ld, acc);
  // ---- epilogue: register g of the lane is the pair (row iw + 4 (lane >> 4) + g, column tile row lane & 15) ----
  const uint64_t i_first = iw + 4 * (lane >> 4);
  const int64_t n = (int64_t)a.n_cols;
  int64_t sx[4] = {0, 0, 0, 0}, vx[4] = {0, 0, 0, 0};
  if (R2) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
      if (i_first + g < a.A) ld_moments(a.counts[i_first + g], n, sx[g], vx[g]);
  }
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    if ((uint32_t)t >= ntw) continue;
    const uint64_t j = iw + 16 * (uint32_t)t + (lane & 15);
    if (j >= a.A) continue;
    int64_t sy = 0, vy = 0;
    if (R2) ld_moments(a.counts[j], n, sy, vy);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const uint64_t i = i_first + g;
      if (j <= i || j - i > W) continue;   // (j < A and i < j: row i is a row of the table)
      uint32_t out;
      if (R2) out = __float_as_uint(ld_r2(n, acc[t][g], sx[g], sy, vx[g], vy));
      else out = (uint32_t)acc[t][g];
      a.band[i * W + (j - i - 1)] = out;
    }
  }
  // ---- the pairs that reach beyond the table's end: zeros, by the block that owns row i ----
  if (row0 + kLdRows + W > a.A)
    for (uint32_t r = wid; r < kLdRows; r += 4) {
      const uint64_t i = row0 + r;
      if (i >= a.A) break;
      const uint64_t k0 = a.A - 1 - i;   // the first k with i + 1 + k >= A
      for (uint64_t k = k0 + lane; k < W; k += 64) a.band[i * W + k] = 0u;
    }
}

}  // namespace vsamd
