// k_gram.hip.h -- the samples x samples Gram matrix D^T D over the genotype matrix of a type-6 plan, and the GRM formed from it
// (vs_query_sample_gram).  Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_ld.hip.h"
#include "k_int128.hip.h"

namespace vsamd {

// gram[i * n + j] = sum over the table rows v of d_v(i) * d_v(j), d = the dosage popcount(cell & 6) of a genotype-matrix cell (0, 1
// or 2): int64, the full symmetric matrix, the diagonal sum d^2.  A row the duplicate rule dropped has an all-zero matrix row
// (k_genotype_matrix) and an all-zero count record (row_span of k_carriers.hip.h gives such a row no carriers, and k_allele_counts
// walks its rows with it), so it adds nothing to any sum below.
//
// k_sample_gram: D^T D on the matrix cores (v_mfma_i32_16x16x64_i8; bytes in, int32 sums: exact).
//   A workgroup of four waves owns one pair (I, J), I <= J, of column tiles of kGramTile = 128 samples -- only the upper triangle
//   of tile pairs is launched -- and one chunk of `chunk` consecutive table rows (option gram_chunk).  Both operands are tiles of
//   the same matrix; on the diagonal (I == J) one panel is staged and read as both.
//   Tile size.  With 64-column tiles a cohort of 2504 samples has 40 tiles, 820 pairs, and every matrix byte is read 41 times
//   (2 x 820 x 64 / 2504); the MFMAs of a 64 x 64 x 64 step (16, 4 per wave) then stand against 8 KiB staged -- the re-reads and
//   the LDS traffic dominate by an order of magnitude.  128-column tiles: 20 tiles, 210 pairs, 21 reads of every byte, and a
//   wave's 64 x 64 quadrant (4 x 4 subtiles of 16 x 16) runs 16 MFMAs per 8 fragment reads of 16 bytes.  256-column tiles would
//   halve the re-reads again but take 256 accumulator registers per lane at four waves, or eight waves; 128 it is.
//   The summed index is the table row, but the matrix is row-major with the samples along the pitch: the staging transposes.
//   Per step kGramK = 128 table rows of the workgroup's columns go into LDS as [column][row bytes], dosages on the way in
//   (ld_dosage4).  A thread loads one dword (4 columns) from each of 4 consecutive rows, transposes the 4 x 4 bytes in registers
//   (__byte_perm) and stores 4 dwords, one per column; the loads of a step are issued together, with clamped addresses and no
//   branch between them, and those of the next step right behind this step's barrier, so they are in flight during the products.
//   LDS rows (columns of the matrix) are kGramStride = kGramK + 16 bytes apart: 36 dwords, 4 mod 8 -- the 16-byte fragment reads of 16 consecutive LDS rows start 4 banks apart and cover all 64
//   banks once (kLdStride's argument), and a 32-lane group of the dword stores covers the 32 banks of a store once: its lanes
//   hold 8 column quads x 4 row quads, and store t of a lane writes column (t + (quad >> 1)) & 3 of its quad, so the 8 columns
//   of one store differ mod 8.  (The rotation is two rounds of selects: no register is indexed dynamically.)
//   A fragment read is k_ld_band's: lane l reads column l & 15 of a 16-column subtile, bytes 16 (l >> 4) .. of the 64-row k-step.
//   Both operands index k alike, so the instruction's own k map does not matter; the C/D map does: register g of lane l is row
//   4 (l >> 4) + g (a column of tile I), column l & 15 (a column of tile J).  Rows beyond the chunk's end, columns beyond the
//   pitch are zeros in LDS; the pitch's own padding bytes are zeros in the matrix.
//   Accumulators are int32: a chunk adds at most 4 x 65536 to a cell.  All 16 are statically indexed.
//   Epilogue: 64-bit integer global atomics into gram (cleared by the engine), zeros skipped; an off-diagonal pair adds its cell
//   to (i, j) and (j, i), a diagonal pair -- whose four waves hold the whole 128 x 128 block, both triangles -- adds each once.
//   Integer adds are exact and order-free: the same call gives the same bytes.
//   LDS: 2 panels x 128 columns x 144 bytes = 36,864 bytes (dynamic; the second panel is idle on the diagonal).
//   Resources (-Rpass-analysis=kernel-resource-usage, gfx950; one instantiation): 176 VGPRs + 64 AGPRs, 73 SGPRs, scratch 0, no
//   spills: 2 waves a SIMD, two workgroups a CU -- the registers bind, LDS would allow four.
//
// k_gram_moments: s_i = sum over v of ac_v d_v(i), ac_v = the row's alt_alleles over S from its count record; C = sum ac_v^2 and
//   H = sum ac_v (2 n - ac_v).  Blocks are (row chunk of kGramMomentRows) x (column group of 256 samples): lane l of a wave owns
//   the dword (4 columns) l of the group, the four waves take every fourth row; the loads along the pitch are coalesced, the sums
//   int64 per thread, added to s with 64-bit integer atomics.  The blocks of column group 0 also sum C and H over their rows.
//   21 VGPRs, 32 SGPRs, 4 KiB of static LDS, scratch 0: 8 waves a SIMD.
//
// k_gram_finish: num_ij = n^2 G_ij - n (s_i + s_j) + C in 128-bit integers, grm_ij = (double)(2 num_ij) / (double)H, 0.0 when
//   H == 0.  Each of the two conversions rounds once (gram_to_double: round to nearest even from 128 bits), one division
//   follows; nothing floating-point is ever summed.  24 VGPRs, 31 SGPRs, no LDS, scratch 0: 8 waves a SIMD.
constexpr uint32_t kGramTile = 128;                 // columns of a tile: a 64 x 64 quadrant per wave
constexpr uint32_t kGramK = 128;                    // table rows staged per step: two MFMA k-steps
constexpr uint32_t kGramStride = kGramK + 16;       // bytes from an LDS row (a column of the matrix) to the next
constexpr uint32_t kGramPanel = kGramTile * kGramStride;
constexpr uint32_t kGramLds = 2 * kGramPanel;
constexpr uint32_t kGramChunkMax = 65536;           // 4 x chunk < 2^31 by a wide margin
constexpr uint32_t kGramBlocksWanted = 256;         // the default chunk aims at this many workgroups: one a CU (more only add atomics: DESIGN 5i's sweep)
constexpr uint32_t kGramMomentRows = 1024;          // table rows per block of k_gram_moments
constexpr uint32_t kGramMomentCols = 256;           // columns per block of k_gram_moments: a dword per lane

struct GramArgs {
  const uint8_t* cells;   // the genotype matrix [A x pitch]
  uint64_t A;
  uint32_t pitch;         // a multiple of 16
  uint32_t n_cols;        // n
  uint32_t n_tiles;       // (n + kGramTile - 1) / kGramTile
  uint32_t n_pairs;       // n_tiles (n_tiles + 1) / 2
  uint32_t chunk;         // table rows per workgroup
  const uint4* counts;    // {carriers, alt_alleles, hom_alt, phased} per table row
  unsigned long long* gram;   // [n x n] int64
  unsigned long long* colw;   // [n] int64: s
  unsigned long long* ch;     // C, H
  double* grm;            // [n x n] (GRM)
};

// A thread's share of one panel step -- kGramK rows from `row0` (rows at `row_end` and beyond are zeros) of the kGramTile columns from
// byte `c0` --: item k of the thread is column quad cq, row quad rq, a dword (4 columns) of each of 4 consecutive rows.
struct GramItem { uint32_t d[4]; };
__device__ __forceinline__ uint32_t gram_cq(uint32_t it) { return (it & 7u) | ((it >> 2) & 24u); }          // column quad 0 .. 31
__device__ __forceinline__ uint32_t gram_rq(uint32_t it) { return ((it >> 3) & 3u) | ((it >> 7) << 2); }    // row quad 0 .. 31
constexpr uint32_t kGramItems = kGramTile * kGramK / 16 / 256;   // per thread and panel

// The loads of a panel step, all issued before any is used: the addresses are clamped into the matrix (row_end >= 1, pitch >= 16)
// and what lies outside is zeroed afterwards, so no load waits for a branch.
__device__ __forceinline__ void gram_load(const GramArgs& a, GramItem (&regs)[kGramItems], uint64_t row0, uint64_t row_end, uint32_t c0) {
#pragma unroll
  for (uint32_t k = 0; k < kGramItems; ++k) {
    const uint32_t it = threadIdx.x + 256 * k;
    const uint32_t col = c0 + 4 * gram_cq(it);
    const uint32_t colc = col < a.pitch ? col : a.pitch - 4;
    const uint64_t g = row0 + 4 * gram_rq(it);
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      const uint64_t gi = g + i < row_end ? g + i : row_end - 1;
      regs[k].d[i] = *reinterpret_cast<const uint32_t*>(a.cells + gi * a.pitch + colc);
    }
  }
}

// Dosages, the 4 x 4 byte transpose and the four dword stores of every item.
__device__ __forceinline__ void gram_store(const GramArgs& a, uint8_t* panel, const GramItem (&regs)[kGramItems], uint64_t row0, uint64_t row_end, uint32_t c0) {
#pragma unroll
  for (uint32_t k = 0; k < kGramItems; ++k) {
    const uint32_t it = threadIdx.x + 256 * k;
    const uint32_t cq = gram_cq(it), rq = gram_rq(it);
    const bool col_in = c0 + 4 * cq < a.pitch;
    const uint64_t g = row0 + 4 * rq;
    const uint32_t d0 = col_in && g + 0 < row_end ? ld_dosage4(regs[k].d[0]) : 0u;
    const uint32_t d1 = col_in && g + 1 < row_end ? ld_dosage4(regs[k].d[1]) : 0u;
    const uint32_t d2 = col_in && g + 2 < row_end ? ld_dosage4(regs[k].d[2]) : 0u;
    const uint32_t d3 = col_in && g + 3 < row_end ? ld_dosage4(regs[k].d[3]) : 0u;
    // 4 x 4 byte transpose: o_j = byte j of d0 .. d3 (the rows side by side, lowest row in the lowest byte)
    const uint32_t t0 = __byte_perm(d0, d1, 0x5140), t1 = __byte_perm(d0, d1, 0x7362);
    const uint32_t t2 = __byte_perm(d2, d3, 0x5140), t3 = __byte_perm(d2, d3, 0x7362);
    const uint32_t o0 = __byte_perm(t0, t2, 0x5410), o1 = __byte_perm(t0, t2, 0x7632);
    const uint32_t o2 = __byte_perm(t1, t3, 0x5410), o3 = __byte_perm(t1, t3, 0x7632);
    // store t writes column (t + s) & 3 of the quad: rotate the four words by s
    const uint32_t s = (cq >> 1) & 3u;
    const bool s1 = s & 1u, s2 = s & 2u;
    const uint32_t p0 = s1 ? o1 : o0, p1 = s1 ? o2 : o1, p2 = s1 ? o3 : o2, p3 = s1 ? o0 : o3;
    const uint32_t q0 = s2 ? p2 : p0, q1 = s2 ? p3 : p1, q2 = s2 ? p0 : p2, q3 = s2 ? p1 : p3;
    uint8_t* base = panel + 4 * cq * kGramStride + 4 * rq;
    *reinterpret_cast<uint32_t*>(base + ((0 + s) & 3u) * kGramStride) = q0;
    *reinterpret_cast<uint32_t*>(base + ((1 + s) & 3u) * kGramStride) = q1;
    *reinterpret_cast<uint32_t*>(base + ((2 + s) & 3u) * kGramStride) = q2;
    *reinterpret_cast<uint32_t*>(base + ((3 + s) & 3u) * kGramStride) = q3;
  }
}

__global__ void __launch_bounds__(256) k_sample_gram(GramArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_gram[];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  // the block's tile pair (I <= J) and row chunk
  uint32_t p = blockIdx.x % a.n_pairs, I = 0;
  while (p >= a.n_tiles - I) { p -= a.n_tiles - I; ++I; }
  const uint32_t J = I + p;
  const uint64_t row_begin = (uint64_t)(blockIdx.x / a.n_pairs) * a.chunk;
  if (row_begin >= a.A) return;
  const uint64_t row_end = row_begin + a.chunk < a.A ? row_begin + a.chunk : a.A;
  const bool diag = I == J;
  uint8_t* const panel_i = s_gram;
  uint8_t* const panel_j = diag ? s_gram : s_gram + kGramPanel;
  ld_i32x4 acc[4][4];
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) acc[x][y] = ld_i32x4{0, 0, 0, 0};
  const uint32_t wr = wid >> 1, wc = wid & 1;   // the wave's quadrant: rows 64 wr .. of tile I, columns 64 wc .. of tile J
  const uint32_t frag_i = (64 * wr + (lane & 15)) * kGramStride + 16 * (lane >> 4);
  const uint32_t frag_j = (64 * wc + (lane & 15)) * kGramStride + 16 * (lane >> 4);
  // the loads of the next step are in flight while this step's products run
  GramItem ri[kGramItems], rj[kGramItems];
  gram_load(a, ri, row_begin, row_end, I * kGramTile);
  if (!diag) gram_load(a, rj, row_begin, row_end, J * kGramTile);
  for (uint64_t r0 = row_begin; r0 < row_end; r0 += kGramK) {
    if (r0 != row_begin) __syncthreads();   // (the step before this one has been read)
    gram_store(a, panel_i, ri, r0, row_end, I * kGramTile);
    if (!diag) gram_store(a, panel_j, rj, r0, row_end, J * kGramTile);
    __syncthreads();
    if (r0 + kGramK < row_end) {   // (block-uniform)
      gram_load(a, ri, r0 + kGramK, row_end, I * kGramTile);
      if (!diag) gram_load(a, rj, r0 + kGramK, row_end, J * kGramTile);
    }
    const uint32_t ksteps = row_end - r0 > 64 ? 2u : 1u;
    for (uint32_t ks = 0; ks < ksteps; ++ks) {
      ld_i32x4 fi[4], fj[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        fi[x] = *reinterpret_cast<const ld_i32x4*>(panel_i + frag_i + 64 * ks + (uint32_t)x * 16 * kGramStride);
        fj[x] = *reinterpret_cast<const ld_i32x4*>(panel_j + frag_j + 64 * ks + (uint32_t)x * 16 * kGramStride);
      }
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fi[x], fj[y], acc[x][y], 0, 0, 0);
    }
  }
  // ---- epilogue: register g of acc[x][y] is the cell (i0 + 16 x + g, j0 + 16 y) ----
  const uint64_t n = a.n_cols;
  const uint64_t i0 = (uint64_t)I * kGramTile + 64 * wr + 4 * (lane >> 4);
  const uint64_t j0 = (uint64_t)J * kGramTile + 64 * wc + (lane & 15);
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
        atomicAdd(a.gram + i * n + j, (unsigned long long)v);
        if (!diag) atomicAdd(a.gram + j * n + i, (unsigned long long)v);
      }
    }
}

// s, C and H.  grid: x = row chunk, y = column group.
__global__ void __launch_bounds__(256) k_gram_moments(GramArgs a) {
  __shared__ unsigned long long s_c[256], s_h[256];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t row_begin = (uint64_t)blockIdx.x * kGramMomentRows;
  const uint64_t row_end = row_begin + kGramMomentRows < a.A ? row_begin + kGramMomentRows : a.A;
  const uint32_t col = blockIdx.y * kGramMomentCols + 4 * lane;
  if (col < a.pitch) {
    unsigned long long s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (uint64_t r = row_begin + wid; r < row_end; r += 4) {
      const unsigned long long ac = a.counts[r].y;
      const uint32_t d = ld_dosage4(*reinterpret_cast<const uint32_t*>(a.cells + r * a.pitch + col));
      s0 += ac * (d & 3u); s1 += ac * ((d >> 8) & 3u); s2 += ac * ((d >> 16) & 3u); s3 += ac * (d >> 24);
    }
    if (s0 && col + 0 < a.n_cols) atomicAdd(a.colw + col + 0, s0);
    if (s1 && col + 1 < a.n_cols) atomicAdd(a.colw + col + 1, s1);
    if (s2 && col + 2 < a.n_cols) atomicAdd(a.colw + col + 2, s2);
    if (s3 && col + 3 < a.n_cols) atomicAdd(a.colw + col + 3, s3);
  }
  if (blockIdx.y != 0) return;   // (block-uniform)
  unsigned long long c = 0, h = 0;
  const unsigned long long n2 = 2ull * a.n_cols;
  for (uint64_t r = row_begin + threadIdx.x; r < row_end; r += 256) {
    const unsigned long long ac = a.counts[r].y;
    c += ac * ac;
    h += ac * (n2 - ac);
  }
  s_c[threadIdx.x] = c; s_h[threadIdx.x] = h;
  __syncthreads();
  for (uint32_t w = 128; w; w >>= 1) {
    if (threadIdx.x < w) { s_c[threadIdx.x] += s_c[threadIdx.x + w]; s_h[threadIdx.x] += s_h[threadIdx.x + w]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (s_c[0]) atomicAdd(a.ch + 0, s_c[0]);
    if (s_h[0]) atomicAdd(a.ch + 1, s_h[0]);
  }
}

// (gram_to_double: k_int128.hip.h)
__global__ void __launch_bounds__(256) k_gram_finish(GramArgs a) {
  const uint64_t n = a.n_cols, cell = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= n * n) return;
  const uint64_t i = cell / n, j = cell - i * n;
  const unsigned long long H = a.ch[1];
  double out = 0.0;
  if (H != 0) {
    const __int128 num = (__int128)(n * n) * (__int128)(long long)a.gram[cell]
                         - (__int128)n * ((__int128)(long long)a.colw[i] + (__int128)(long long)a.colw[j]) + (__int128)(long long)a.ch[0];
    out = gram_to_double(2 * num) / (double)H;
  }
  a.grm[cell] = out;
}

}  // namespace vsamd
