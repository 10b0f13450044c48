// k_trio.hip.h -- Mendelian errors and transmission counts per table row and per trio over the genotype matrix of a type-6 plan
// (vs_query_trio_scan).  Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_ibs.hip.h"

namespace vsamd {

// A trio is three columns (child, father, mother) of the temporary genotype matrix over the members S.  With f, m, c the dosages
// popcount(cell & 6) of father, mother and child in one table row (0, 1 or 2; a row the duplicate rule dropped is all zeros) and
// the gamete sets g(0) = {0}, g(1) = {0, 1}, g(2) = {1}:
//   error         c is no sum a + b, a in g(f), b in g(m)
//   denovo        f == 0 && m == 0 && c > 0                      (a subset of the errors)
//   transmitted   T = c - [f == 2] - [m == 2]                    (consistent cells only; an error cell adds nothing)
//   untransmitted U = [f == 1] + [m == 1] - T
// 27 states s = 9 f + 3 m + c, four small numbers each: err, denovo in {0, 1}, T, U in {0, 1, 2}.  The table is built at compile
// time by ENUMERATING the gamete pairs (trio_table below; the closed forms above are what the tests hold it against) and lives in
// three 64-bit constants of two bits a state -- kTrioT, kTrioU, kTrioED (bit 0 err, bit 1 denovo) -- which the compiler keeps in
// scalar registers: a look-up is three 64-bit shifts by 2 s, no memory and no branch.
//
// k_trio_scan: a workgroup of four waves owns (a block of R consecutive table rows) x (a chunk of `chunk` trios, a multiple of
//   64; option trio_chunk).  R = the largest power of two up to min(16, 64 KiB / pitch), at least 1 -- a staged row must fit the
//   64 KiB tile, hence the query's bound of 65,536 members.
//   Skip.  A block whose rows all have carriers == 0 in the count records over S returns at once (its records were cleared by the
//   engine): most rows of a sparse cohort.
//   Staging.  The block's rows are R * pitch CONTIGUOUS bytes of the matrix (pitch is a multiple of 16): 16-byte loads, the four
//   dwords turned into DOSAGE bytes on the way -- ((w >> 1) & 0x01010101) + ((w >> 2) & 0x01010101) -- and stored with 16-byte LDS
//   writes; the rows a last block lacks are staged as zeros, so that the row loop below is unrolled R times without a bound.
//   Hot loop.  Wave w takes the chunk's slabs of 64 trios w, w + 4, ..; lane l owns trio slab * 64 + l and reads its column triple
//   from the trio table in L2 (12 bytes a lane, consecutive lanes consecutive; the next slab's triple is loaded while this one is
//   worked).  A lane beyond the chunk or the table reads columns (0, 0, 0) and its look-up is replaced by 0 with a select: every
//   loop bound is wave-uniform, no lane leaves early.  Per row: three LDS byte reads through the triple, s, the look-up packed as
//   4 x 8 bits (err | denovo << 8 | T << 16 | U << 24), one add into the lane's per-trio sum and one into its per-row sum.  No
//   branch on data.
//   Per-trio sums stay in the lane: one register, 4 x 8 bits (at most 2 R = 32 a field).  At the end of a slab the lane adds each
//   non-zero field with one 32-bit integer atomic to trios[t] -- so a block adds to a trio once -- or stores the four fields
//   when the launch has ONE row block.
//   Per-row sums: R registers of 4 x 8 bits a lane over the wave's slabs (at most 2 per slab and field: kTrioChunkMax keeps a wave
//   to 64 slabs, 128 < 256).  Behind the slabs they are widened to 4 x 16 bits in one 64-bit value (64 lanes x 128 < 65,536) and
//   reduced over the wave by a halving butterfly: at distance 1, 2, 4, 8 a lane keeps one half of its values and adds the
//   partner's copies of that half, then holds ONE row's sum over its 16 lanes; distances 16 and 32 finish it.  R - 1 + 6 - log2 R
//   64-bit shuffles instead of 6 R, all under wave-uniform control flow.  Lane l < R then holds row bitrev(l); the four waves'
//   values meet in LDS and threads 0 .. R - 1 add each non-zero field to rows[v] with a 32-bit integer atomic -- or store the four
//   when the launch has ONE trio chunk.
//   Only integer adds: the same call gives the same bytes under every trio_chunk.
//   LDS: R * pitch bytes dynamic (at most 64 KiB) + 528 bytes static.
//   Resources (-Rpass-analysis=kernel-resource-usage, gfx950), R = 16 / 8 / 4 / 2 / 1: VGPRs 56 / 40 / 30 / 22 / 21, SGPRs 76 / 50 /
//   46 / 44 / 42, no AGPRs, scratch 0, no spills, occupancy 8 waves a SIMD by registers in every form (the LDS tile, not the
//   registers, bounds the resident workgroups: 160 KiB / (R * pitch)).
//
// n_used is k_ibs_n_used's (the rows the duplicate rule kept), through an IbsArgs of its four fields.
constexpr uint32_t kTrioRowsMax = 16;          // table rows a workgroup stages at most
constexpr uint32_t kTrioTileBytes = 64 << 10;  // ... and the bytes of its tile
constexpr uint32_t kTrioChunkMax = 16384;      // trios a workgroup takes at most: 64 slabs a wave, a lane's per-row field stays below 256
                                               // (tests/test_gpu_trio_scan_wide.py runs 16,384 trios that all add 2 to one field of one row:
                                               // 128 a lane, 8,192 a wave, 32,768 a workgroup, and holds that a larger trio_chunk is refused)
constexpr uint32_t kTrioBlocksWanted = 2048;   // the default chunk splits the trios only while the launch has fewer workgroups than this

struct TrioEntry { uint32_t err, denovo, t, u; };
// the state's record from the gamete pairs themselves
constexpr TrioEntry trio_entry(uint32_t f, uint32_t m, uint32_t c) {
  const uint32_t g_lo[3] = {0, 0, 1}, g_hi[3] = {0, 1, 1};   // g(d) = {g_lo[d] .. g_hi[d]}
  bool consistent = false;
  for (uint32_t a = g_lo[f]; a <= g_hi[f]; ++a)
    for (uint32_t b = g_lo[m]; b <= g_hi[m]; ++b) consistent = consistent || a + b == c;
  if (!consistent) return TrioEntry{1u, f == 0 && m == 0 && c > 0 ? 1u : 0u, 0u, 0u};
  // a heterozygous parent transmits ALT or not; a homozygous one has no choice and counts nowhere
  const uint32_t forced = g_lo[f] + g_lo[m], het = (f == 1 ? 1u : 0u) + (m == 1 ? 1u : 0u), t = c - forced;
  return TrioEntry{0u, 0u, t, het - t};
}
constexpr uint64_t trio_table(int field) {
  uint64_t w = 0;
  for (uint32_t s = 0; s < 27; ++s) {
    const TrioEntry e = trio_entry(s / 9, s / 3 % 3, s % 3);
    const uint64_t v = field == 0 ? e.t : field == 1 ? e.u : (e.err | e.denovo << 1);
    w |= v << (2 * s);
  }
  return w;
}
constexpr uint64_t kTrioT = trio_table(0), kTrioU = trio_table(1), kTrioED = trio_table(2);

struct TrioArgs {
  const uint8_t* cells;        // the temporary genotype matrix over S, rows `pitch` bytes apart
  uint64_t A;                  // table rows
  uint32_t pitch, n_cols;
  const uint4* counts;         // the count record of every table row over S (x: carriers)
  const uint32_t* trio_cols;   // 3 per trio: the columns of child, father, mother
  uint32_t n_trios, chunk, n_chunks;
  uint32_t* rows;              // 4 per table row: errors, denovo, transmitted, untransmitted
  uint32_t* trios;             // 4 per trio, the same
};

__device__ __forceinline__ uint32_t trio_dosage4(uint32_t w) { return ((w >> 1) & 0x01010101u) + ((w >> 2) & 0x01010101u); }

// 4 x 8 bits -> 4 x 16 bits
__device__ __forceinline__ uint64_t trio_widen(uint32_t x) {
  const uint32_t lo = (x & 0xFFu) | ((x & 0xFF00u) << 8), hi = ((x >> 16) & 0xFFu) | ((x >> 24) << 16);
  return (uint64_t)lo | (uint64_t)hi << 32;
}

// The wave's sums of v[0 .. R - 1]: afterwards v[0] of lane l is the sum over all 64 lanes of row trio_row_of_lane<R>(l).
template <uint32_t R>
__device__ __forceinline__ void trio_wave_rows(uint64_t (&v)[R], uint32_t lane) {
#pragma unroll
  for (uint32_t step = 0; step < 6; ++step) {
    const uint32_t d = 1u << step, n = R >> step;   // n: the values a lane still holds
    if (n > 1) {
      const bool up = (lane & d) != 0;
#pragma unroll
      for (uint32_t i = 0; i < n / 2; ++i) {
        const uint64_t send = up ? v[i] : v[i + n / 2], keep = up ? v[i + n / 2] : v[i];
        v[i] = keep + __shfl_xor(send, (int)d, 64);
      }
    } else v[0] += __shfl_xor(v[0], (int)d, 64);
  }
}
template <uint32_t R>
__device__ __forceinline__ uint32_t trio_row_of_lane(uint32_t lane) {
  uint32_t row = 0;
#pragma unroll
  for (uint32_t step = 0; (R >> step) > 1; ++step) row += (lane >> step & 1u) * (R >> (step + 1));
  return row;
}

// grid: row blocks x trio chunks (blockIdx.x = row block * n_chunks + chunk), 256 threads, R * pitch bytes of dynamic LDS; rows
// and trios cleared by the engine.
template <uint32_t R>
__global__ void __launch_bounds__(256) k_trio_scan(TrioArgs a) {
  extern __shared__ uint4 s_tile4[];
  __shared__ uint64_t s_part[4][kTrioRowsMax];
  __shared__ uint32_t s_live;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t chunk_i = blockIdx.x % a.n_chunks;
  const uint64_t row0 = (uint64_t)(blockIdx.x / a.n_chunks) * R;
  const uint32_t n_rows = (uint32_t)(a.A - row0 < R ? a.A - row0 : R);
  if (tid == 0) s_live = 0;
  __syncthreads();
  if (tid < n_rows && a.counts[row0 + tid].x) s_live = 1;
  __syncthreads();
  if (!s_live) return;   // (the same word in every thread)
  {   // the block's rows as dosage bytes, the rows it lacks as zeros
    const uint4* src = reinterpret_cast<const uint4*>(a.cells + row0 * a.pitch);
    const uint32_t have = n_rows * (a.pitch / 16), all = R * (a.pitch / 16);
    for (uint32_t i = tid; i < all; i += 256) {
      uint4 w = make_uint4(0, 0, 0, 0);
      if (i < have) {
        w = src[i];
        w.x = trio_dosage4(w.x); w.y = trio_dosage4(w.y); w.z = trio_dosage4(w.z); w.w = trio_dosage4(w.w);
      }
      s_tile4[i] = w;
    }
  }
  __syncthreads();
  const uint8_t* tile = reinterpret_cast<const uint8_t*>(s_tile4);
  const uint32_t t_begin = chunk_i * a.chunk;
  const uint32_t t_end = a.n_trios - t_begin < a.chunk ? a.n_trios : t_begin + a.chunk;
  const uint32_t n_slabs = (t_end - t_begin + 63) / 64;
  const bool one_block = gridDim.x == a.n_chunks, one_chunk = a.n_chunks == 1;
  uint32_t racc[R];
#pragma unroll
  for (uint32_t r = 0; r < R; ++r) racc[r] = 0;
  auto triple = [&](uint32_t slab, uint32_t& cc, uint32_t& cf, uint32_t& cm) {
    const uint32_t t = t_begin + slab * 64 + lane;
    cc = cf = cm = 0;
    if (slab < n_slabs && t < t_end) { cc = a.trio_cols[3 * (size_t)t]; cf = a.trio_cols[3 * (size_t)t + 1]; cm = a.trio_cols[3 * (size_t)t + 2]; }
  };
  uint32_t cc, cf, cm;
  triple(wave, cc, cf, cm);
  for (uint32_t slab = wave; slab < n_slabs; slab += 4) {   // (wave-uniform bounds)
    const uint32_t t = t_begin + slab * 64 + lane;
    const bool valid = t < t_end;
    uint32_t ncc, ncf, ncm;
    triple(slab + 4, ncc, ncf, ncm);
    uint32_t tacc = 0;
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
      const uint8_t* row = tile + r * a.pitch;
      const uint32_t c = row[cc], f = row[cf], m = row[cm];
      const uint32_t sh = 2 * (9 * f + 3 * m + c);
      const uint32_t ed = (uint32_t)(kTrioED >> sh) & 3u, tt = (uint32_t)(kTrioT >> sh) & 3u, uu = (uint32_t)(kTrioU >> sh) & 3u;
      const uint32_t packed = (ed & 1u) | (ed & 2u) << 7 | tt << 16 | uu << 24;
      const uint32_t add = valid ? packed : 0u;
      tacc += add;
      racc[r] += add;
    }
    if (valid) {
      uint32_t* dst = a.trios + 4 * (size_t)t;
      if (one_block) *reinterpret_cast<uint4*>(dst) = make_uint4(tacc & 0xFFu, tacc >> 8 & 0xFFu, tacc >> 16 & 0xFFu, tacc >> 24);
      else {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
          const uint32_t v = tacc >> (8 * k) & 0xFFu;
          if (v) atomicAdd(dst + k, v);
        }
      }
    }
    cc = ncc; cf = ncf; cm = ncm;
  }
  uint64_t wide[R];
#pragma unroll
  for (uint32_t r = 0; r < R; ++r) wide[r] = trio_widen(racc[r]);
  trio_wave_rows<R>(wide, lane);
  if (lane < R) s_part[wave][trio_row_of_lane<R>(lane)] = wide[0];
  __syncthreads();
  if (tid < n_rows) {
    const uint64_t s = s_part[0][tid] + s_part[1][tid] + s_part[2][tid] + s_part[3][tid];   // (4 x 8,192 a field at most)
    uint32_t* dst = a.rows + 4 * (row0 + tid);
    const uint32_t v[4] = {(uint32_t)s & 0xFFFFu, (uint32_t)s >> 16, (uint32_t)(s >> 32) & 0xFFFFu, (uint32_t)(s >> 48)};
    if (one_chunk) *reinterpret_cast<uint4*>(dst) = make_uint4(v[0], v[1], v[2], v[3]);
    else {
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k)
        if (v[k]) atomicAdd(dst + k, v[k]);
    }
  }
}

}  // namespace vsamd
