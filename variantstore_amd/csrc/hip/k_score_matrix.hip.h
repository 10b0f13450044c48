// k_score_matrix.hip.h -- score-matrix queries (vs_query_score_matrix): D^T W, samples x K weighted dosage sums over the rows a batch
// reports, for a WIDE panel of K weight columns, on the matrix cores.  The transpose of k_assoc_matrix's product and the wide form
// of k_sample_scores'.  Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_gram.hip.h"
#include "k_scores.hip.h"
#include "../host/score_matrix_host.hpp"

namespace vsamd {

// sums[c * K + k] = sum over the reports of d(row(report), c) q_k(report): column c of the subset, weight column k, d the dosage
// popcount(cell & 6) of the temporary genotype matrix, q_k = rint(w 2^f_k) the trait quantiser's fixed point (|q| < 2^30, f_k = 30 - e
// from the host).  The weights are keyed by REPORT, the matrix by table row, and several regions may report one shared row; so the
// product runs over the table rows with the row totals T[row][k] = the sum of q_k over the row's reports:
//   k_score_matrix_weights  a wave per region: slot j of region q is report off[q] + j - (dropped slots in front of j), found from one
//                           ballot over the kept slots of a round of 64 (k_score_weights' rule).  A report's K weights are contiguous
//                           and K is wide, so the lanes run along k: a group of G lanes (K rounded up to a power of two, at most 64)
//                           takes one slot, 64 / G slots a pass; every lane forms slot, row and report from the wave-uniform ballot
//                           word alone.  q = rint(ldexp((double)w, f_k)), f_k from a device array; nonzero q goes into T[row][k]
//                           (cleared) with a 64-bit integer global atomic.
//   k_score_matrix_limbs    T to the limb panel, [score tile of 16][limb of 5][score in tile][row] int8, rows `apad` (A rounded up
//                           to 128) apart: the balanced base-256 digits of score_matrix_host.hpp.  A workgroup owns 128 rows x 32
//                           columns of T: the waves read T two rows of 256 contiguous bytes at a time into LDS ([row slot][36] int64,
//                           row 16 g + i in slot 8 i + g: the write of a half-wave and the read below both cover the banks once), then
//                           thread (k, g) splits rows 16 g .. 16 g + 15 of its k and stores 16 bytes per limb, eight lanes a 128-byte
//                           run of a panel row.  Rows past the table and scores past K are written as zeros: the panel needs no
//                           memset.  The largest |T| leaves through a wave reduction and one 64-bit atomicMax per wave into `meta`.
//   k_score_matrix          below
//   k_score_matrix_finish   scores = ldexp((double)sums, -f_k), f_k from the device array
//
// k_score_matrix<LIMBS, TS>: a workgroup of four waves owns 128 columns (k_sample_gram's tile) x TS score tiles of 16 x one chunk
// of table rows (option score_matrix_chunk).  Per step of kGramK = 128 rows the dosage operand goes into LDS as [column][row bytes]
// through gram_load / gram_store (k_gram.hip.h: a GramArgs with `cells` and `pitch` set is all they read), the limb operand -- TS x
// LIMBS x 16 panel rows of 128 bytes, contiguous runs of the panel, in bounds and zero past the table because its rows are padded to
// 128 -- with plain 16-byte loads into LDS rows kGramStride apart; the loads of the next step are issued right behind this step's
// barrier.  Wave w owns the column subtiles 2 w and 2 w + 1: per 64-row k-step 2 dosage fragment reads, TS x LIMBS panel reads and
// 2 x TS x LIMBS v_mfma_i32_16x16x64_i8, the dosage as the first operand: register g of lane l is then (column 4 (l >> 4) + g of the
// subtile, score l & 15 of the tile), 16 consecutive lanes on 16 consecutive scores of one sample, a 128-byte run of `sums`.
// Accumulators: 2 x TS x LIMBS i32x4, all statically indexed; a chunk of at most 65,536 rows adds at most 2 x 128 x 65536 = 2^24 to
// one.  LIMBS is a template parameter: the engine reads the largest |T| back before this kernel (it has to -- a batch beyond 2^38 is
// refused by the call), so the four-limb kernel carries no fifth accumulator and no branch.
// Epilogue: S = sum acc_l 256^l in int64; nonzero cells leave with 64-bit integer global atomics into `sums` (cleared), guarded by
// column < n and score < K.  Integer adds are exact and order-free: the same call gives the same bytes under every chunk.
// Grid: one dimension, the score tile fastest (then the column tile, then the chunk): the workgroups in flight share the chunk's
// matrix panel in L2.  Measured against the column tile fastest: the same to 0.3 % at K = 64, 1.3 % slower at K = 512.
// LDS (static): (128 + 16 TS LIMBS) x 144 bytes: 27,648 / 29,952 at TS = 1, 36,864 / 41,472 at TS = 2.
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage), k_score_matrix<LIMBS, TS>: VGPRs + AGPRs, waves a
// SIMD; scratch 0 and no spills in every instantiation:
//   <4,1> 120 + 32, 3   <5,1> 135 + 40, 2   <4,2> 166 + 64, 2   <5,2> 189 + 80, 1
// The engine runs <4,2> (42 SGPRs, 36,864 bytes of LDS) and <5,1> (45 SGPRs, 29,952 bytes): on the chr1-2504 bench batch at K = 64 the
// four-limb kernel takes 0.94 ms with two score tiles a workgroup against 1.49 ms with one (the dosage stage is shared by twice the
// MFMAs); <5,2> would run one wave a SIMD.  The limb operand's prefetch registers are the native vector type (ld_i32x4): as an
// array of uint4 they went to scratch.
// k_score_matrix_weights 28 VGPRs, 51 SGPRs; k_score_matrix_limbs 76 VGPRs, 28 SGPRs, 36,864 bytes of LDS, 4 waves a SIMD;
// k_score_matrix_finish 12 VGPRs, 23 SGPRs: scratch 0, no spills.
constexpr uint32_t kSmTilesPerWg = 2;                 // TS: score tiles of a workgroup (16 against 32 scores)
constexpr uint32_t kSmTilesPerWg5 = 1;                // ... of the five-limb kernel: two tiles take 189 VGPRs + 80 AGPRs, one wave a SIMD
constexpr uint32_t kSmChunkMax = 65536;               // an int32 accumulator stays below 2^24
constexpr uint32_t kSmBlocksWanted = 1024;            // the default chunk aims at this many workgroups
constexpr uint32_t kSmLimbRows = 128, kSmLimbCols = 32, kSmLimbPitch = 36;   // k_score_matrix_limbs: T rows x columns of a workgroup; LDS row pitch in words of 8 bytes (4 mod 32)

struct ScoreMatrixWeightArgs {
  const VariantRow* rows;
  const uint64_t* var_begin;   // per region, in the caller's order
  const uint64_t* q_nvar;
  const uint64_t* off;         // k_score_offsets
  uint64_t Q, N;
  const float* w;              // [N][K], report order
  const int32_t* shift;        // [K] f_k
  uint32_t K, G;               // G: lanes per slot, a power of two in 1 .. 64, >= min(K, 64)
  long long* T;                // [A][K], cleared
};
__global__ void __launch_bounds__(256) k_score_matrix_weights(ScoreMatrixWeightArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const uint32_t per_pass = 64 / a.G, sub = lane / a.G, k_first = lane % a.G;
  for (uint64_t q = wave; q < a.Q; q += nwaves) {
    const uint64_t a0 = a.var_begin[q], nv = a.q_nvar[q];
    uint64_t report = a.off[q];   // of the first kept slot of this round
    for (uint64_t j0 = 0; j0 < nv; j0 += 64) {
      const bool kept = j0 + lane < nv && !(a.rows[a0 + j0 + lane].count_flags & kRowDropped);
      const uint64_t keep = __ballot(kept);   // (wave-uniform: every lane derives its slot from it)
      const uint32_t slots = nv - j0 < 64 ? (uint32_t)(nv - j0) : 64u;
      for (uint32_t s0 = 0; s0 < slots; s0 += per_pass) {
        const uint32_t s = s0 + sub;
        if (s >= slots || !((keep >> s) & 1ull)) continue;
        const uint64_t ri = report + __popcll(keep & ((1ull << s) - 1ull));
        if (ri >= a.N) continue;
        const uint64_t row = a0 + j0 + s;
        for (uint32_t k = k_first; k < a.K; k += a.G) {
          const long long v = (long long)__builtin_rint(ldexp((double)a.w[ri * a.K + k], a.shift[k]));   // ties to even
          if (v) atomicAdd(reinterpret_cast<unsigned long long*>(a.T + row * a.K + k), (unsigned long long)v);
        }
      }
      report += __popcll(keep);
    }
  }
}

struct ScoreMatrixLimbArgs {
  const long long* T;          // [A][K]
  uint64_t A, apad;            // apad: A rounded up to 128
  uint32_t K, tiles;           // tiles = ceil(K / 16)
  int8_t* panel;               // [tiles][5][16][apad]
  unsigned long long* meta;    // the largest |T| (cleared)
};
// grid: x = block of 128 rows, y = group of 32 columns of T
__global__ void __launch_bounds__(256) k_score_matrix_limbs(ScoreMatrixLimbArgs a) {
  __shared__ long long s_t[kSmLimbRows * kSmLimbPitch];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t row0 = (uint64_t)blockIdx.x * kSmLimbRows;
  const uint32_t k0 = blockIdx.y * kSmLimbCols;
  // ---- T into LDS: a wave reads two rows x 32 columns a round ----
  unsigned long long mx = 0;
  const uint32_t kk = lane & 31;
  for (uint32_t r = 2 * wid + (lane >> 5); r < kSmLimbRows; r += 8) {
    long long v = 0;
    if (row0 + r < a.A && k0 + kk < a.K) v = a.T[(row0 + r) * a.K + k0 + kk];
    const unsigned long long m = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
    mx = m > mx ? m : mx;
    s_t[((r & 15u) * 8 + (r >> 4)) * kSmLimbPitch + kk] = v;
  }
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) {
    const unsigned long long o = __shfl_xor(mx, d, 64);
    mx = o > mx ? o : mx;
  }
  if (lane == 0 && mx) atomicMax(a.meta, mx);
  __syncthreads();
  // ---- thread (k, g): the five digits of rows 16 g .. 16 g + 15, 16 bytes a limb ----
  const uint32_t g = threadIdx.x & 7, k = threadIdx.x >> 3;
  const uint32_t tile = (k0 + k) / kSmScoreTile, j = (k0 + k) % kSmScoreTile;
  if (tile >= a.tiles) return;
  uint32_t out[kSmLimbsMax][4];
#pragma unroll
  for (uint32_t l = 0; l < kSmLimbsMax; ++l)
#pragma unroll
    for (uint32_t x = 0; x < 4; ++x) out[l][x] = 0;
#pragma unroll
  for (uint32_t i = 0; i < 16; ++i) {
    int8_t b[kSmLimbsMax];
    (void)sm_limbs(s_t[(i * 8 + g) * kSmLimbPitch + k], b);
#pragma unroll
    for (uint32_t l = 0; l < kSmLimbsMax; ++l) out[l][i >> 2] |= (uint32_t)(uint8_t)b[l] << (8 * (i & 3));
  }
  int8_t* const dst = a.panel + ((uint64_t)tile * kSmLimbsMax * kSmScoreTile + j) * a.apad + row0 + 16 * g;
#pragma unroll
  for (uint32_t l = 0; l < kSmLimbsMax; ++l)
    *reinterpret_cast<uint4*>(dst + (uint64_t)l * kSmScoreTile * a.apad) = uint4{out[l][0], out[l][1], out[l][2], out[l][3]};
}

struct ScoreMatrixArgs {
  const uint8_t* cells;        // the genotype matrix [A x pitch]
  const int8_t* panel;         // [tiles][5][16][apad]
  uint64_t A, apad;
  uint32_t pitch;              // a multiple of 16
  uint32_t n_cols, K;
  uint32_t tiles;              // ceil(K / 16)
  uint32_t tile_groups;        // ceil(tiles / TS)
  uint32_t col_tiles;          // ceil(n / 128)
  uint32_t chunk;              // table rows per workgroup: a multiple of 128
  unsigned long long* sums;    // [n][K] int64, cleared
};

template <uint32_t LIMBS, uint32_t TS>
__global__ void __launch_bounds__(256) k_score_matrix(ScoreMatrixArgs a) {
  constexpr uint32_t kRowsB = TS * LIMBS * 16;                  // limb rows in LDS
  constexpr uint32_t kWordsB = kRowsB * (kGramK / 16);          // their 16-byte words a step
  constexpr uint32_t kItemsB = (kWordsB + 255) / 256;
  __shared__ __attribute__((aligned(16))) uint8_t s_sm[(kGramTile + kRowsB) * kGramStride];
  uint8_t* const panel_d = s_sm;
  uint8_t* const panel_b = s_sm + kGramPanel;
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  // the score tile group fastest, then the column tile, then the chunk
  const uint32_t tg = blockIdx.x % a.tile_groups, rest = blockIdx.x / a.tile_groups;
  const uint32_t ct = rest % a.col_tiles;
  const uint64_t ch = rest / a.col_tiles;
  const uint64_t row_begin = ch * a.chunk;
  if (row_begin >= a.A) return;
  const uint64_t row_end = row_begin + a.chunk < a.A ? row_begin + a.chunk : a.A;
  const uint32_t c0 = ct * kGramTile;
  GramArgs ga{};
  ga.cells = a.cells; ga.pitch = a.pitch;
  // the limb operand: word i of a step is 16 bytes of limb row i >> 3 -- score tile (i >> 3) / (16 LIMBS) of the group, limb and score
  // within it --, rows 16 (i & 7) .. of the step.  A score tile past the last one reads the last one's rows; its cells are not stored.
  const int8_t* bsrc[kItemsB];
  uint32_t bdst[kItemsB];
#pragma unroll
  for (uint32_t x = 0; x < kItemsB; ++x) {
    const uint32_t i = threadIdx.x + 256 * x, lr = (i >> 3) % kRowsB, t = lr / (LIMBS * 16), within = lr % (LIMBS * 16);
    const uint32_t tile = tg * TS + t < a.tiles ? tg * TS + t : a.tiles - 1;
    bsrc[x] = a.panel + ((uint64_t)tile * kSmLimbsMax * kSmScoreTile + within) * a.apad + 16 * (i & 7);
    bdst[x] = lr * kGramStride + 16 * (i & 7);
  }
  ld_i32x4 acc[2][TS][LIMBS];
#pragma unroll
  for (uint32_t s = 0; s < 2; ++s)
#pragma unroll
    for (uint32_t t = 0; t < TS; ++t)
#pragma unroll
      for (uint32_t l = 0; l < LIMBS; ++l) acc[s][t][l] = ld_i32x4{0, 0, 0, 0};
  const uint32_t frag = (lane & 15) * kGramStride + 16 * (lane >> 4);   // the lane's fragment of k-step 0 within 16 LDS rows
  // the loads of the next step are in flight while this step's products run
  GramItem rd[kGramItems];
  ld_i32x4 rb[kItemsB];
  gram_load(ga, rd, row_begin, row_end, c0);
#pragma unroll
  for (uint32_t x = 0; x < kItemsB; ++x) rb[x] = *reinterpret_cast<const ld_i32x4*>(bsrc[x] + row_begin);
  for (uint64_t r0 = row_begin; r0 < row_end; r0 += kGramK) {
    if (r0 != row_begin) __syncthreads();   // (the step before this one has been read)
    gram_store(ga, panel_d, rd, r0, row_end, c0);
#pragma unroll
    for (uint32_t x = 0; x < kItemsB; ++x)
      if (kWordsB % 256 == 0 || threadIdx.x + 256 * x < kWordsB) *reinterpret_cast<ld_i32x4*>(panel_b + bdst[x]) = rb[x];
    __syncthreads();
    if (r0 + kGramK < row_end) {   // (block-uniform; r0 is a multiple of 128 -- the chunk is one -- and apad is A rounded up to 128, so r0 + 2 kGramK <= apad: the panel's rows are there)
      gram_load(ga, rd, r0 + kGramK, row_end, c0);
#pragma unroll
      for (uint32_t x = 0; x < kItemsB; ++x) rb[x] = *reinterpret_cast<const ld_i32x4*>(bsrc[x] + r0 + kGramK);
    }
    const uint32_t ksteps = row_end - r0 > 64 ? 2u : 1u;
    for (uint32_t ks = 0; ks < ksteps; ++ks) {
      const ld_i32x4 fa0 = *reinterpret_cast<const ld_i32x4*>(panel_d + (32 * wid) * kGramStride + frag + 64 * ks);
      const ld_i32x4 fa1 = *reinterpret_cast<const ld_i32x4*>(panel_d + (32 * wid + 16) * kGramStride + frag + 64 * ks);
#pragma unroll
      for (uint32_t t = 0; t < TS; ++t)
#pragma unroll
        for (uint32_t l = 0; l < LIMBS; ++l) {
          const ld_i32x4 fb = *reinterpret_cast<const ld_i32x4*>(panel_b + ((t * LIMBS + l) * 16) * kGramStride + frag + 64 * ks);
          acc[0][t][l] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa0, fb, acc[0][t][l], 0, 0, 0);
          acc[1][t][l] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa1, fb, acc[1][t][l], 0, 0, 0);
        }
    }
  }
  // ---- epilogue: register g of acc[s][t][.] is the cell (column col0 + 16 s + g, score 16 (tg TS + t) + (l & 15)) ----
  const uint64_t col0 = (uint64_t)c0 + 32 * wid + 4 * (lane >> 4);
#pragma unroll
  for (uint32_t t = 0; t < TS; ++t) {
    const uint32_t score = (tg * TS + t) * kSmScoreTile + (lane & 15);
    if (score >= a.K) continue;
#pragma unroll
    for (uint32_t s = 0; s < 2; ++s)
#pragma unroll
      for (uint32_t g = 0; g < 4; ++g) {
        const uint64_t col = col0 + 16 * s + g;
        long long S = 0;
#pragma unroll
        for (uint32_t l = 0; l < LIMBS; ++l) S += (long long)acc[s][t][l][g] * (1ll << (8 * l));
        if (col < a.n_cols && S != 0) atomicAdd(a.sums + col * a.K + score, (unsigned long long)S);
      }
  }
}

__global__ void __launch_bounds__(256) k_score_matrix_finish(const long long* __restrict__ sums, uint64_t n_cells, uint32_t K, const int32_t* __restrict__ shift,
                                                             double* __restrict__ scores) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cells) return;
  scores[i] = ldexp((double)sums[i], -shift[i % K]);
}

}  // namespace vsamd
