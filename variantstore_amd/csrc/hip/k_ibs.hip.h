// k_ibs.hip.h -- pairwise IBS counts and KING kinship over the genotype matrix of a type-6 plan (vs_query_sample_ibs): three
// samples x samples matrices of genotype-STATE co-occurrences from one staging of the dosages.  Part of kernels.hip.h (the kernel
// index is there).
#pragma once
#include "k_gram.hip.h"

namespace vsamd {

// With d = the dosage popcount(cell & 6) of a genotype-matrix cell (0, 1 or 2), h = [d == 1], a = [d == 2], c = [d > 0]:
//   het_het[i * n + j] = sum over the table rows v of h_v(i) h_v(j), hom_hom the same of a, carrier_both of c: int64, full and
//   symmetric; their diagonals are the per-sample totals nh, na and nc = nh + na.  A row the duplicate rule dropped has an all-zero
//   matrix row (k_genotype_matrix) and adds nothing; it is not a site: n_used = A - dropped rows.
// None of the three can be read off D^T D, whose cell mixes them as HH + 2 (HA + AH) + 4 AA.
//
// k_sample_ibs: k_sample_gram's structure -- a workgroup of four waves owns one pair (I, J), I <= J, of column tiles of kGramTile =
//   128 samples (the upper triangle only) and one chunk of `chunk` consecutive table rows (option ibs_chunk); a wave owns a 64 x 64
//   quadrant -- and k_sample_gram's staging as it stands: gram_load / gram_store put kGramK = 128 table rows of both tiles into LDS
//   as [column][row dosage bytes], transposed in registers, the next step's loads in flight behind the barrier.
//   The dosage panel is staged ONCE and feeds all three products.  A fragment read is k_sample_gram's (lane l: column l & 15 of a
//   16-column subtile, bytes 16 (l >> 4) .. of the 64-row k-step); the four dosage dwords of a fragment become three indicator
//   fragments in registers -- het = f & 0x01010101, hom = (f >> 1) & 0x01010101, car = het | hom (a dosage byte is 0, 1 or 2) -- and
//   three v_mfma_i32_16x16x64_i8 per pair of subtiles accumulate into three sets of 16 i32x4 accumulators.  Per k-step a wave reads
//   8 fragments and issues 48 MFMAs: three times k_sample_gram's arithmetic on the same L2 reads and the same LDS transposes, which
//   DESIGN 5i names as what bounds the large case.
//   Tile shape.  gram_load / gram_store fix the panel at 128 columns x 128 rows and the workgroup at 256 threads.  Three sets of
//   16 accumulators are 192 registers a lane: beside the staging registers that is more than the 256 of two waves a SIMD, so the
//   kernel runs ONE wave a SIMD (a workgroup a CU).  The alternatives keep two: a 64 x 32 quadrant needs eight waves on the same
//   panels (the staging helpers are written for 256 threads) and 64-column tiles double the re-reads of every matrix byte (41
//   instead of 21 at 2504 samples), which is what the one staging is there to save.  One wave a SIMD costs the overlap of one
//   workgroup's staging with another's products; within a wave the 48 MFMAs of a k-step are independent of each other (16
//   accumulators x 3) and of the loads in flight, so the matrix pipe stays fed between barriers: per 128-row step a wave issues 96
//   MFMAs of 8 passes (about 3,100 cycles) against 8 dword loads, 8 dword LDS stores and 16 fragment reads.  (Measured, DESIGN 5j:
//   the three products cost 1.0 to 1.9 of k_sample_gram's stage.)
//   Accumulators are int32: an indicator sum over a chunk is at most kIbsChunkMax = 65,536.  All 48 are statically indexed.
//   Epilogue: k_sample_gram's, three times -- 64-bit integer global atomics into the three matrices (cleared by the engine), zeros
//   skipped; an off-diagonal pair adds its cell to (i, j) and (j, i), a diagonal pair adds each once.  Integer adds are exact and
//   order-free: the same call gives the same bytes.  The atomics are what a launch of many row chunks pays for (DESIGN 5j's
//   sweep: three matrices' worth, and they bound the kernel long before the MFMAs do); when the table is ONE chunk a tile pair
//   has one workgroup and the cells are plain stores.
//   LDS: kGramLds = 36,864 bytes (dynamic; the second panel is idle on the diagonal).
//   Resources (-Rpass-analysis=kernel-resource-usage, gfx950): 256 VGPRs + 203 AGPRs (the 192 accumulators stay in AGPRs in
//   place), 65 SGPRs, scratch 0, no spills: 1 wave a SIMD, one workgroup a CU.  (The k-step loop is kept rolled: unrolled by two
//   the compiler spilled 20 registers.)  k_ibs_n_used: 10 VGPRs, 24 SGPRs, 2 KiB of static LDS; k_ibs_finish: 29 VGPRs, 29 SGPRs,
//   no LDS; both scratch 0 and 8 waves a SIMD.
//
// k_ibs_n_used: the rows the duplicate rule kept, A - |{v >= U : count_flags bit 31}| (only private rows are ever dropped:
//   row_site of k_carriers.hip.h), counted per thread, summed per block in LDS, one 64-bit atomic a block into the result's word.
//
// k_ibs_finish: a thread per cell.  From the three diagonals and n_used, in int64:
//     ibs0 = na_i + na_j - 2 hom_hom - (carrier_both - het_het - hom_hom)          opposite homozygotes, {0, 2}
//     ibs2 = n_used - nc_i - nc_j + carrier_both + het_het + hom_hom               equal dosage, 0/0 included
//   and under VS_IBS_KING king = (double)(het_het - 2 ibs0) / (double)(nh_i + nh_j), 0.0 where nh_i + nh_j == 0: both integers lie
//   below 2^53, each converts exactly, one division follows; nothing floating-point is summed.
constexpr uint32_t kIbsChunkMax = 65536;       // an indicator sum over a chunk fits int32 by a wide margin
constexpr uint32_t kIbsBlocksWanted = 128;     // the default chunk aims at this many workgroups: fewer, longer chunks -- every chunk adds three tiles of atomics (DESIGN 5j's sweep)

struct IbsArgs {
  GramArgs m;                  // cells, A, pitch, n_cols, n_tiles, n_pairs, chunk as for k_sample_gram (gram_load / gram_store read it)
  const VariantRow* rows;      // the table's rows (k_ibs_n_used)
  uint64_t U;                  // shared rows: the rows behind them are private and may be dropped
  unsigned long long* het_het; // [n x n] int64, hom_hom and carrier_both right behind it
  long long* ibs0;             // [n x n] int64, ibs2 right behind it
  unsigned long long* n_used;  // one word
  double* king;                // [n x n] (KING), else NULL
};

// the 4 x 4 subtile products of one indicator: 16 independent MFMAs
__device__ __forceinline__ void ibs_mfma16(const ld_i32x4 (&ui)[4], const ld_i32x4 (&uj)[4], ld_i32x4 (&acc)[4][4]) {
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) acc[x][y] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ui[x], uj[y], acc[x][y], 0, 0, 0);
}

// a wave's quadrant of one product into its matrix: register g of acc[x][y] is the cell (i0 + 16 x + g, j0 + 16 y)
__device__ __forceinline__ void ibs_flush(const ld_i32x4 (&acc)[4][4], unsigned long long* dst, uint64_t n, uint64_t i0, uint64_t j0, bool diag, bool single) {
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const uint64_t j = j0 + 16 * (uint32_t)y;
      if (j >= n) continue;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const uint64_t i = i0 + 16 * (uint32_t)x + (uint32_t)g;
        const int v = acc[x][y][g];
        if (i >= n || v == 0) continue;
        if (single) {   // (block-uniform) the only workgroup of its tile pair: nobody else adds to these cells
          dst[i * n + j] = (unsigned long long)v;
          if (!diag) dst[j * n + i] = (unsigned long long)v;
        } else {
          atomicAdd(dst + i * n + j, (unsigned long long)v);
          if (!diag) atomicAdd(dst + j * n + i, (unsigned long long)v);
        }
      }
    }
}

__global__ void __launch_bounds__(256) k_sample_ibs(IbsArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_ibs[];
  const GramArgs& m = a.m;
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  // the block's tile pair (I <= J) and row chunk
  uint32_t p = blockIdx.x % m.n_pairs, I = 0;
  while (p >= m.n_tiles - I) { p -= m.n_tiles - I; ++I; }
  const uint32_t J = I + p;
  const uint64_t row_begin = (uint64_t)(blockIdx.x / m.n_pairs) * m.chunk;
  if (row_begin >= m.A) return;
  const uint64_t row_end = row_begin + m.chunk < m.A ? row_begin + m.chunk : m.A;
  const bool diag = I == J;
  uint8_t* const panel_i = s_ibs;
  uint8_t* const panel_j = diag ? s_ibs : s_ibs + kGramPanel;
  ld_i32x4 acc_h[4][4], acc_a[4][4], acc_c[4][4];
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) acc_h[x][y] = acc_a[x][y] = acc_c[x][y] = ld_i32x4{0, 0, 0, 0};
  const uint32_t wr = wid >> 1, wc = wid & 1;   // the wave's quadrant: rows 64 wr .. of tile I, columns 64 wc .. of tile J
  const uint32_t frag_i = (64 * wr + (lane & 15)) * kGramStride + 16 * (lane >> 4);
  const uint32_t frag_j = (64 * wc + (lane & 15)) * kGramStride + 16 * (lane >> 4);
  // the loads of the next step are in flight while this step's products run
  GramItem ri[kGramItems], rj[kGramItems];
  gram_load(m, ri, row_begin, row_end, I * kGramTile);
  if (!diag) gram_load(m, rj, row_begin, row_end, J * kGramTile);
  for (uint64_t r0 = row_begin; r0 < row_end; r0 += kGramK) {
    if (r0 != row_begin) __syncthreads();   // (the step before this one has been read)
    gram_store(m, panel_i, ri, r0, row_end, I * kGramTile);
    if (!diag) gram_store(m, panel_j, rj, r0, row_end, J * kGramTile);
    __syncthreads();
    if (r0 + kGramK < row_end) {   // (block-uniform)
      gram_load(m, ri, r0 + kGramK, row_end, I * kGramTile);
      if (!diag) gram_load(m, rj, r0 + kGramK, row_end, J * kGramTile);
    }
    const uint32_t ksteps = row_end - r0 > 64 ? 2u : 1u;
#pragma unroll 1
    for (uint32_t ks = 0; ks < ksteps; ++ks) {
      ld_i32x4 fi[4], fj[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        fi[x] = *reinterpret_cast<const ld_i32x4*>(panel_i + frag_i + 64 * ks + (uint32_t)x * 16 * kGramStride);
        fj[x] = *reinterpret_cast<const ld_i32x4*>(panel_j + frag_j + 64 * ks + (uint32_t)x * 16 * kGramStride);
      }
      // one product after the other: only one pair of indicator fragment sets is live beside the dosages
      ld_i32x4 ui[4], uj[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) { ui[x] = fi[x] & 0x01010101; uj[x] = fj[x] & 0x01010101; }
      ibs_mfma16(ui, uj, acc_h);
#pragma unroll
      for (int x = 0; x < 4; ++x) { ui[x] = (fi[x] >> 1) & 0x01010101; uj[x] = (fj[x] >> 1) & 0x01010101; }
      ibs_mfma16(ui, uj, acc_a);
#pragma unroll
      for (int x = 0; x < 4; ++x) { ui[x] = (fi[x] | (fi[x] >> 1)) & 0x01010101; uj[x] = (fj[x] | (fj[x] >> 1)) & 0x01010101; }
      ibs_mfma16(ui, uj, acc_c);
    }
  }
  // ---- epilogue ----
  const uint64_t n = m.n_cols;
  const uint64_t i0 = (uint64_t)I * kGramTile + 64 * wr + 4 * (lane >> 4);
  const uint64_t j0 = (uint64_t)J * kGramTile + 64 * wc + (lane & 15);
  const bool single = gridDim.x == m.n_pairs;   // one row chunk: plain stores
  ibs_flush(acc_h, a.het_het, n, i0, j0, diag, single);
  ibs_flush(acc_a, a.het_het + n * n, n, i0, j0, diag, single);
  ibs_flush(acc_c, a.het_het + 2 * n * n, n, i0, j0, diag, single);
}

// n_used.  grid: blocks of 256 threads striding over the table's rows; the word is cleared by the engine.
__global__ void __launch_bounds__(256) k_ibs_n_used(IbsArgs a) {
  __shared__ unsigned long long s_kept[256];
  unsigned long long kept = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < a.m.A; r += (uint64_t)gridDim.x * 256)
    kept += r >= a.U && (a.rows[r].count_flags & kRowDropped) ? 0u : 1u;
  s_kept[threadIdx.x] = kept;
  __syncthreads();
  for (uint32_t w = 128; w; w >>= 1) {
    if (threadIdx.x < w) s_kept[threadIdx.x] += s_kept[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0 && s_kept[0]) atomicAdd(a.n_used, s_kept[0]);
}

__global__ void __launch_bounds__(256) k_ibs_finish(IbsArgs a) {
  const uint64_t n = a.m.n_cols, nn = n * n, cell = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= nn) return;
  const uint64_t i = cell / n, j = cell - i * n;
  const long long* hh = reinterpret_cast<const long long*>(a.het_het);
  const long long* aa = hh + nn;
  const long long* cc = aa + nn;
  const long long nh_i = hh[i * n + i], nh_j = hh[j * n + j];
  const long long na_i = aa[i * n + i], na_j = aa[j * n + j];
  const long long nc_i = cc[i * n + i], nc_j = cc[j * n + j];
  const long long h = hh[cell], q = aa[cell], c = cc[cell];
  const long long ibs0 = na_i + na_j - 2 * q - (c - h - q);
  a.ibs0[cell] = ibs0;
  a.ibs0[nn + cell] = (long long)*a.n_used - nc_i - nc_j + c + h + q;
  if (a.king) {
    const long long den = nh_i + nh_j;
    a.king[cell] = den ? (double)(h - 2 * ibs0) / (double)den : 0.0;
  }
}

}  // namespace vsamd
