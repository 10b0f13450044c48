// k_scores.hip.h -- per-sample scores (vs_query_sample_scores): samples x K weighted dosage sums over the rows a batch reports, the
// transpose of the association scan's product.  No matrix is built and no floating-point number is ever added: the weights are
// quantised to 64-bit integers once per column, so every sum is exact and the order of its additions does not matter.
// Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_carriers.hip.h"

namespace vsamd {

// The four steps of a score batch (the contract is in include/variantstore_hip.h):
//   k_score_scale     per column k the largest |w| as a max over the float bit patterns with the sign cleared (for finite floats the
//                     order of the patterns is the order of the magnitudes) and a bit per column that holds a non-finite value.  The
//                     host forms f_k = 36 - e from it (M_k = m 2^e, 0.5 <= m < 1)
//   k_score_offsets   off[q] = exclusive prefix sum over the caller's region order of rep[q], the rows region q reports (the plan's
//                     var_count); off[Q] = N, which the host holds against n_weights
//   k_score_weights   a wave per region: slot j of region q is report off[q] + j - (dropped slots in front of j); its K weights are
//                     quantised, q = rint(w 2^f_k), and added to Wq[row][k] with 64-bit integer global atomics -- a shared row that
//                     several regions report collects every report's weight; Wn[row] counts the reports whose weights are not all 0
//   k_sample_scores   below
//   k_score_finish    scores = ldexp((double)sums, -f_k)
//
// k_sample_scores: a workgroup of four waves owns (chunk_rows consecutive table rows) x (a column tile).  The tile is [column][Kp]
// int64 in LDS (Kp: K rounded up to 1, 2, 4 or 8; the padding weights are zero).  The waves walk the chunk 256 rows at a time, lane l
// of wave w takes row 4 l + w, as k_sample_burden does.  A row without a report that carries a nonzero weight (Wn[row] == 0 -- most
// rows under a score file) is dropped from the walk before any of its carriers is touched.  The walk is k_carriers.hip.h's: listed and
// explicit-id rows as the flat list of 8-carrier groups, a lane per group and step (the row's Kp integer weights are loaded once per
// group); denser class rows a row at a time, a lane per class-row word.  Per carrier in the tile: column_of<SUBSET>, then up to Kp
// 64-bit integer LDS adds of d x Wq[row][k], d = popc(gt & 6).  The tile's nonzero cells leave with 64-bit integer global atomics into
// `sums`, which the engine has cleared.  Integer sums: the same call gives the same bytes whatever chunk and tile it runs with.
//
// LDS per workgroup, from MI355X_MICROARCH.md (160 KiB per CU):
//   static   the wave state (FlatRows) 5136 B + Wn of the waves' rows 1024 B + the pair count 8 B = 6168 B
//   dynamic  the tile, tile_cols x Kp x 8 B, at most 64 KiB (tile_cols <= 65536 / (8 Kp): 8192 / 4096 / 2048 / 1024 columns at
//            Kp = 1 / 2 / 4 / 8); SUBSET: the mask, 8 B a word, and its ranks, 4 B a word (2504 samples: 480 B)
//   whole cohort, full tile: 70.0 KiB -> two workgroups per CU, as in k_sample_burden; 2504 columns at Kp = 1: 25.6 KiB -> six
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage), k_sample_scores<Kp, SUBSET>: VGPRs / SGPRs
// (SGPRs spilled to VGPR lanes), waves per SIMD by registers; scratch 0 bytes per lane and no VGPR spill in every instantiation:
//   <1,0> 54/96 (0) 8   <1,1> 54/102 (0) 7   <2,0> 54/102 (0) 7   <2,1> 55/106 (2) 7
//   <4,0> 58/106 (0) 7  <4,1> 59/106 (6) 7   <8,0> 67/106 (6) 7   <8,1> 67/106 (18) 7
// k_score_scale 19/42, k_score_offsets 68/78 (128 B of LDS), k_score_weights 28/60, k_score_finish 12/23: scratch 0, no spills.
// Registers allow 7 waves per SIMD and more: LDS (two workgroups = 8 waves per CU at a full tile) bounds the occupancy.
constexpr uint32_t kScoresMax = 8;
constexpr uint32_t kScoreChunkRows = 4096;         // rows one workgroup walks
constexpr uint32_t kScoreTileBytes = 64 << 10;     // a second workgroup fits a CU's 160 KiB
constexpr uint32_t kScoreShift = 36;               // |q| <= 2^36
constexpr uint64_t kScoreMaxReports = 1ull << 26;  // |sum| <= 2 N 2^36 < 2^63
__host__ __device__ constexpr uint32_t score_pow2(uint32_t k) { return k <= 1 ? 1u : k <= 2 ? 2u : k <= 4 ? 4u : 8u; }

// the words the scale kernel and the offsets leave for the host, and the sum the walk leaves
struct ScoreMeta {
  uint32_t max_bits[kScoresMax];   // per column: the largest float pattern with the sign cleared
  uint32_t nonfinite;              // bit k: column k holds an infinity or a NaN
  uint32_t pad_;
  unsigned long long n_pairs;      // (report, carrier in S) pairs whose report has a nonzero weight
};

__global__ void __launch_bounds__(256) k_score_scale(const float* __restrict__ w, uint64_t n_reports, uint32_t K, ScoreMeta* meta) {
  uint32_t m[kScoresMax];
#pragma unroll
  for (uint32_t k = 0; k < kScoresMax; ++k) m[k] = 0;
  uint32_t bad = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_reports; i += stride) {
#pragma unroll
    for (uint32_t k = 0; k < kScoresMax; ++k) {
      if (k >= K) break;
      const uint32_t b = __float_as_uint(w[i * K + k]) & 0x7FFFFFFFu;
      if (b >= 0x7F800000u) bad |= 1u << k;
      else if (b > m[k]) m[k] = b;
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < kScoresMax; ++k) {
    if (k >= K) break;
    uint32_t v = m[k];
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64);
      v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0 && v) atomicMax(&meta->max_bits[k], v);
  }
  if (bad) atomicOr(&meta->nonfinite, bad);
}

// One workgroup: off[q] = sum of rep[0 .. q), off[Q] = the total.  8 regions per thread and round.
constexpr uint32_t kScoreOffBlock = 1024, kScoreOffItems = 8;
__global__ void __launch_bounds__(kScoreOffBlock) k_score_offsets(const uint64_t* __restrict__ rep, uint64_t Q, uint64_t* __restrict__ off) {
  __shared__ uint64_t s_wave[kScoreOffBlock / 64];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint64_t carry = 0;
  for (uint64_t base = 0; base < Q; base += (uint64_t)kScoreOffBlock * kScoreOffItems) {
    const uint64_t q0 = base + (uint64_t)threadIdx.x * kScoreOffItems;
    uint64_t v[kScoreOffItems], s = 0;
#pragma unroll
    for (uint32_t i = 0; i < kScoreOffItems; ++i) { v[i] = q0 + i < Q ? rep[q0 + i] : 0; s += v[i]; }
    uint64_t incl = s;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint64_t t = __shfl_up(incl, d, 64);
      if (lane >= d) incl += t;
    }
    if (lane == 63) s_wave[wid] = incl;
    __syncthreads();
    uint64_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kScoreOffBlock / 64; ++w) { if (w < wid) before += s_wave[w]; total += s_wave[w]; }
    __syncthreads();
    uint64_t ex = carry + before + incl - s;
#pragma unroll
    for (uint32_t i = 0; i < kScoreOffItems; ++i) { if (q0 + i < Q) off[q0 + i] = ex; ex += v[i]; }
    carry += total;
  }
  if (threadIdx.x == 0) off[Q] = carry;
}

struct ScoreShift { int32_t f[kScoresMax]; };   // f_k per column
struct ScoreWeightArgs {
  const VariantRow* rows;
  const uint64_t* var_begin;   // per region, in the caller's order
  const uint64_t* q_nvar;
  const uint64_t* off;         // k_score_offsets
  uint64_t Q, N;
  const float* w;              // [N][K], report order
  uint32_t K, KP;
  ScoreShift shift;
  long long* wq;               // [A][KP], cleared
  uint32_t* wn;                // [A], cleared
};
__global__ void __launch_bounds__(256) k_score_weights(ScoreWeightArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  for (uint64_t q = wave; q < a.Q; q += nwaves) {
    const uint64_t a0 = a.var_begin[q], nv = a.q_nvar[q];
    uint64_t report = a.off[q];   // of the first kept slot of this round
    for (uint64_t j0 = 0; j0 < nv; j0 += 64) {
      const uint64_t row = a0 + j0 + lane;
      const bool kept = j0 + lane < nv && !(a.rows[row].count_flags & kRowDropped);
      const uint64_t keep = __ballot(kept);
      const uint64_t ri = report + __popcll(keep & ((1ull << lane) - 1ull));
      if (kept && ri < a.N) {
        bool any = false;
        for (uint32_t k = 0; k < a.K; ++k) {
          const long long v = (long long)__builtin_rint(ldexp((double)a.w[ri * a.K + k], a.shift.f[k]));   // ties to even
          if (v) { atomicAdd(reinterpret_cast<unsigned long long*>(a.wq + row * a.KP + k), (unsigned long long)v); any = true; }
        }
        if (any) atomicAdd(a.wn + row, 1u);
      }
      report += __popcll(keep);
    }
  }
}

struct ScoreArgs {
  const VariantRow* rows;       // the table
  const uint32_t* u_site;       // the site of every table row
  uint64_t A, U;
  const uint64_t* S;            // SUBSET: the mask and the columns in front of each of its words
  const uint32_t* S_rank;
  uint32_t s_words;
  uint32_t n_cols, K, tile_cols, n_tiles, chunk_rows;
  const long long* wq;          // [A][Kp]
  const uint32_t* wn;           // [A]
  unsigned long long* sums;     // [n_cols][K] int64, cleared
  ScoreMeta* meta;
};

struct ScoreTile : ColumnTile { unsigned long long* cell; };

// one carrier (sample id, dosage d) of a row with the integer weights w into its Kp cells, if the tile holds its column
template <uint32_t KP, bool SUBSET>
__device__ __forceinline__ uint32_t score_add(const ScoreTile& t, uint32_t id, uint32_t d, const long long (&w)[KP]) {
  uint32_t col;
  if (!column_of<SUBSET>(t, id, col)) return 0u;
  if (d) {
#pragma unroll
    for (uint32_t k = 0; k < KP; ++k)
      if (w[k]) atomicAdd(&t.cell[(size_t)col * KP + k], (unsigned long long)((long long)d * w[k]));
  }
  return 1u;
}
template <uint32_t KP>
__device__ __forceinline__ void score_weights_of(const long long* __restrict__ wq, uint64_t row, long long (&w)[KP]) {
  const long long* p = wq + row * KP;
  if constexpr (KP == 1) w[0] = p[0];
  else {
#pragma unroll
    for (uint32_t i = 0; i < KP / 2; ++i) {
      const longlong2 v = reinterpret_cast<const longlong2*>(p)[i];
      w[2 * i] = v.x; w[2 * i + 1] = v.y;
    }
  }
}

template <uint32_t KP, bool SUBSET>
__global__ void __launch_bounds__(256) k_sample_scores(DevImage im, ScoreArgs a) {
  extern __shared__ unsigned long long s_score[];   // tile_cols x KP cells | SUBSET: s_words mask words | s_words ranks
  __shared__ FlatRows s_rows;
  __shared__ uint32_t s_wn[4][64];
  __shared__ unsigned long long s_pairs;
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t chunk = blockIdx.x / a.n_tiles;
  const uint32_t tile = blockIdx.x % a.n_tiles;
  const uint64_t r_begin = chunk * a.chunk_rows;
  const uint64_t r_end = a.A - r_begin < a.chunk_rows ? a.A : r_begin + a.chunk_rows;   // (the table may end inside the chunk)
  ScoreTile t;
  t.cell = s_score;
  t.mask = reinterpret_cast<const uint64_t*>(s_score + (size_t)a.tile_cols * KP);
  t.rank = reinterpret_cast<const uint32_t*>(t.mask + a.s_words);
  t.tile0 = tile * a.tile_cols;
  t.tn = a.n_cols - t.tile0 < a.tile_cols ? a.n_cols - t.tile0 : a.tile_cols;
  t.num_samples = im.num_samples;
  for (uint32_t i = threadIdx.x; i < t.tn * KP; i += 256) s_score[i] = 0;
  if (SUBSET)
    for (uint32_t i = threadIdx.x; i < a.s_words; i += 256) {
      const_cast<uint64_t*>(t.mask)[i] = a.S[i];
      const_cast<uint32_t*>(t.rank)[i] = a.S_rank[i];
    }
  if (threadIdx.x == 0) s_pairs = 0;
  __syncthreads();
  const CarrierForm f = carrier_form(im);
  const uint32_t* off = s_rows.off[wid];
  unsigned long long pairs = 0;
  for (uint64_t base = r_begin; base < r_end; base += 256) {
    // ---- the parameters of this wave's 64 rows; a row no report weights has no carriers here ----
    const uint64_t row = base + 4 * lane + wid;
    RowSite rs{0, 0, 0};
    uint32_t wn = 0;
    if (row < r_end) {
      wn = a.wn[row];
      if (wn) rs = row_site(im, a.rows, a.u_site, row, a.U);
    }
    s_wn[wid][lane] = wn;
    const bool dense = is_dense(im, f, rs.cnt);
    const uint32_t total = flat_publish(s_rows, wid, lane, dense, rs);
    // ---- the flat pass: one group of 8 carriers per lane and step ----
    for (uint32_t e = lane; e < total; e += 64) {
      const uint32_t L = flat_find<64>(off, e);
      const uint32_t k8 = e - off[L], nsel = group_nsel(s_rows.cnt[wid][L], k8);
      long long w[KP];
      score_weights_of<KP>(a.wq, base + 4 * L + wid, w);
      uint32_t id[8];
      const uint32_t gw = group_load(im, f, s_rows.gt0[wid][L] + 8ull * k8, s_rows.src[wid][L], k8, id);
      uint32_t hit = 0;
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j)
        if (j < nsel) hit += score_add<KP, SUBSET>(t, id[j], __popc(gt_of_slot(gw, j, f.groups) & 6u), w);
      pairs += (unsigned long long)hit * s_wn[wid][L];
    }
    // ---- denser classes: a row at a time, a lane per word of the class row ----
    uint64_t dmask = __ballot(dense);
    while (dmask) {
      const int r = __builtin_ctzll(dmask);
      dmask &= dmask - 1;
      const uint32_t c_r = __builtin_amdgcn_readlane(rs.cls, r);
      const uint64_t gt0_r = wave_bcast64(rs.gt0, r);
      const uint32_t wn_r = __builtin_amdgcn_readlane(wn, r);
      long long w[KP];
      score_weights_of<KP>(a.wq, base + 4 * (uint64_t)r + wid, w);
      uint32_t before = 0, hit = 0;   // carriers in the row words before this round of 64
      for (uint32_t wb = 0; wb < im.wpc; wb += 64) {
        const uint32_t wi = wb + lane;
        const ClassChunk ch = class_chunk(im, c_r, wi);
        uint64_t m = ch.rw;
        if (SUBSET) m = wi < a.s_words ? ch.rw & t.mask[wi] : 0ull;
        while (m) {
          const int b = __builtin_ctzll(m);
          m &= m - 1;
          const uint64_t kc = gt0_r + before + (ch.incl - ch.pc) + __popcll(ch.rw & ((1ull << b) - 1ull));   // carrier record of sample wi * 64 + b
          hit += score_add<KP, SUBSET>(t, wi * 64 + (uint32_t)b, __popc(gt_of_record(gt_word(im, f, kc >> 3), kc, f.groups) & 6u), w);
        }
        before += __builtin_amdgcn_readlane(ch.incl, 63);
      }
      pairs += (unsigned long long)hit * wn_r;
    }
    wave_lds_sync();   // (the rows are read before the next 256 overwrite them)
  }
  if (pairs) atomicAdd(&s_pairs, pairs);
  __syncthreads();
  // ---- the tile's nonzero cells leave LDS ----
  for (uint32_t i = threadIdx.x; i < t.tn * KP; i += 256) {
    const unsigned long long v = t.cell[i];
    const uint32_t col = i / KP, k = i % KP;
    if (v && k < a.K) atomicAdd(&a.sums[(size_t)(t.tile0 + col) * a.K + k], v);
  }
  if (threadIdx.x == 0 && s_pairs) atomicAdd(&a.meta->n_pairs, s_pairs);
}

__global__ void __launch_bounds__(256) k_score_finish(const long long* __restrict__ sums, uint64_t n_cells, uint32_t K, ScoreShift sh, double* __restrict__ scores) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cells) return;
  scores[i] = ldexp((double)sums[i], -sh.f[i % K]);
}

}  // namespace vsamd
