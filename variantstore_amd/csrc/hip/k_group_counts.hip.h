// k_group_counts.hip.h -- allele counts per row of a type-6 plan and per sample GROUP (vs_query_group_counts): every carrier of a
// row visited once, looked up in a label-per-sample table and added to the accumulator of its (row, group).
// Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_counts.hip.h"

namespace vsamd {

// out[row * G + g] = {carriers, alt_alleles, hom_alt, phased} of table row `row` over the samples whose label is g: the record
// k_allele_counts gives with group g as the subset, for all G groups in ONE pass over the row's carriers.
//
// One wave owns R consecutive rows (R from G, below).  Every lane gathers a row's site parameters as in k_allele_counts; then
//   flat pass   explicit-id rows and the rows of listed classes (at most list_max carriers): the FLAT list of 8-carrier groups of the
//               wave's rows (DPP prefix sum over the group counts, a lane finds its row by bisection over the offsets in LDS), a lane
//               per group: one genotype word (gt_groups | gt_nibbles | an unaligned window of the unpadded explicit-id pool, the run's
//               end masked by the entry count) and the group's 8 ids (cls_list16 | cls_list_ids | car_sid)
//   dense pass  a denser class row: the WAVE per row, a lane per 64-bit word of the class row, 64 words a chunk.  A sample's id is its
//               bit position, its carrier index the prefix popcount -- and a lane's carriers are consecutive, so the index is a counter.
//               The chunk's genotype words (at most 4096 carriers = 512 words + 1 for the unaligned start) are staged in LDS ONCE with
//               coalesced loads and read from there per carrier: no dependent global load per carrier (DESIGN 5b's cost of the subset path)
// A carrier costs one LDS byte load (its label) and, when the label is a group, ONE 64-bit LDS atomic: the four counts travel packed,
// 16 bits a field -- carriers | alt << 16 | hom << 32 | phased << 48.  No field overflows: the label table admits cohorts of at most
// kGroupLabelMaxBytes = 32768 sample ids (ref included), so carriers, hom_alt and phased stay below 2^15 and alt_alleles
// (2 x samples) below 2^16.
//
// Accumulators: kGroupCells = 512 packed cells per wave, [row][group, padded to the power of two Gp][copy]:
//   Gp        1   2   4   8  16  32  64
//   R (rows) 64  64  64  64  32  16   8
//   copies    8   4   2   1   1   1   1      a lane adds to copy (lane & (copies - 1)): with few groups the lanes of a wave would
//                                            otherwise serialise on a handful of addresses
// LDS per workgroup (4 waves), from MI355X_MICROARCH.md (160 KiB per CU, workgroups per CU <= 160 KiB / LDS per workgroup, 64 KiB per
// workgroup without an attribute): label table <= 32768 B (dynamic) + accumulators 4 x 512 x 8 = 16384 B + staged genotype words
// 4 x 520 x 4 = 8320 B + wave state 4 x (65 + 64 + 64) x 4 + 4 x 64 x 8 = 5136 B = 62608 B at the largest table, whatever G: two
// workgroups (8 waves) per CU by LDS there, and it stays below the 64 KiB a launch gets without asking.  A 2504-sample cohort: 32348 B,
// five workgroups per CU.
//
// Output: when a wave's rows are counted, its lanes sum the copies and store the R x G records -- contiguous in `out` -- with one
// 16-byte vector store per record, consecutive lanes consecutive records; every cell of `out` is stored exactly once, zeros of empty
// groups and dropped rows included (no memset, nothing of a recycled buffer shows through).
constexpr uint32_t kGroupCells = 512;
constexpr uint32_t kGroupStageWords = 520;           // 4096 carriers of a 64-word chunk = 512 words, + 1 (unaligned start), rounded up
constexpr size_t kGroupLabelMaxBytes = 32 << 10;     // a label byte per sample id; also what keeps the 16-bit fields from overflowing
constexpr uint32_t kGroupNone = 0xFFu;               // label of a sample in no group

__host__ __device__ inline uint32_t group_pow2(uint32_t n_groups) { uint32_t p = 1; while (p < n_groups) p <<= 1; return p; }
__host__ __device__ inline uint32_t group_rows_per_wave(uint32_t n_groups) { const uint32_t r = kGroupCells / group_pow2(n_groups); return r < 64 ? r : 64u; }

// one carrier's packed contribution from its three genotype bits (bit 0 phase, bit 1 gt_1, bit 2 gt_2)
__device__ __forceinline__ unsigned long long group_packed(uint32_t gt) {
  const uint32_t lo = 1u | ((((gt >> 1) & 1u) + ((gt >> 2) & 1u)) << 16);
  const uint32_t hi = ((gt >> 1) & (gt >> 2) & 1u) | ((gt & 1u) << 16);
  return (unsigned long long)lo | ((unsigned long long)hi << 32);
}

__global__ void __launch_bounds__(256) k_group_counts(DevImage im, const VariantRow* __restrict__ rows, const uint32_t* __restrict__ u_site, uint64_t A,
                                                      uint64_t U, const uint64_t* __restrict__ labels, uint32_t label_words, uint32_t G,
                                                      uint4* __restrict__ out) {
  extern __shared__ uint64_t s_label64[];   // label_words words: a label byte per sample id, shared by the block's waves
  __shared__ uint32_t s_off[4][64 + 1];
  __shared__ uint32_t s_src[4][64];
  __shared__ uint32_t s_cnt[4][64];
  __shared__ uint64_t s_gt0[4][64];
  __shared__ unsigned long long s_acc[4][kGroupCells];
  __shared__ uint32_t s_stage[4][kGroupStageWords];
  for (uint32_t i = threadIdx.x; i < label_words; i += blockDim.x) s_label64[i] = labels[i];
  __syncthreads();
  const uint8_t* s_label = reinterpret_cast<const uint8_t*>(s_label64);
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint32_t Gp = group_pow2(G), R = group_rows_per_wave(G), copies = kGroupCells / (R * Gp);
  const uint32_t gshift = 31 - __clz(Gp), cshift = 31 - __clz(copies), mycopy = lane & (copies - 1);
  const uint64_t r0 = (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * R;
  if (r0 >= A) return;
  const uint64_t row = r0 + lane;
  const bool valid = lane < R && row < A;
  const bool groups = im.use_bv && im.wpc <= 63;
  const bool explicit_ids = !im.use_bv;
  const uint32_t ns = im.num_samples;
  // ---- the row's parameters ----
  uint32_t cnt = 0, cls = 0;
  uint64_t gt0 = 0;
  if (valid) {
    const uint32_t g = u_site[row];
    cnt = im.s_ncar[g];
    if (row >= U && (rows[row].count_flags & kRowDropped)) cnt = 0;   // dropped by the duplicate rule: counts 0 in every group
    cls = im.s_class[g];
    gt0 = im.s_gt0[g];
  }
  const bool dense = !explicit_ids && cnt > im.list_max;   // counted by the wave-per-row pass below
  const uint32_t ng = dense ? 0u : (cnt + 7) / 8;
  const uint32_t incl = wave_inclusive_scan(ng);
  const uint32_t total = __builtin_amdgcn_readlane(incl, 63);
  uint32_t* off = s_off[wid];
  unsigned long long* acc = s_acc[wid];
  off[lane] = incl - ng;                // (lanes beyond R: no groups, their offsets equal the total)
  if (lane == 0) off[64] = total;
  s_src[wid][lane] = cls;
  s_cnt[wid][lane] = cnt;
  s_gt0[wid][lane] = gt0;
#pragma unroll
  for (uint32_t i = 0; i < kGroupCells / 64; ++i) acc[lane + 64 * i] = 0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  const uint32_t* __restrict__ gt32 = reinterpret_cast<const uint32_t*>(im.gt_nibbles);
  // ---- the flat pass: one group of 8 carriers per lane and step ----
  for (uint32_t e0 = 0; e0 < total; e0 += 64) {
    const uint32_t e = e0 + lane;
    if (e >= total) continue;
    uint32_t L = 0;
#pragma unroll
    for (uint32_t step = 32; step; step >>= 1)
      if (off[L + step] <= e) L += step;
    const uint32_t k = e - off[L], rcnt = s_cnt[wid][L], src = s_src[wid][L];
    const uint32_t rem = rcnt - 8 * k, nsel = rem < 8 ? rem : 8u;    // entries of the group that belong to the row
    const uint64_t g = s_gt0[wid][L] + 8ull * k;                      // carrier record of the group's first entry
    uint32_t w, id[8];
    if (explicit_ids) {                                               // unpadded pool: a window of the nibble stream, ids beside it
      uint2 nw;
      __builtin_memcpy(&nw, gt32 + (g >> 3), 8);
      w = __builtin_amdgcn_alignbit(nw.y, nw.x, ((uint32_t)g & 7u) * 4);
      uint4 ia, ib;
      __builtin_memcpy(&ia, im.car_sid + g, 16);
      __builtin_memcpy(&ib, im.car_sid + g + 4, 16);
      id[0] = ia.x; id[1] = ia.y; id[2] = ia.z; id[3] = ia.w; id[4] = ib.x; id[5] = ib.y; id[6] = ib.z; id[7] = ib.w;
    } else if (groups) {                                              // (g is a multiple of 8 in class-row pools)
      w = im.gt_groups[g >> 3];
      const uint4 iw = reinterpret_cast<const uint4*>(im.cls_list16)[(uint64_t)src + k];
      id[0] = iw.x & 0xFFFFu; id[1] = iw.x >> 16; id[2] = iw.y & 0xFFFFu; id[3] = iw.y >> 16;
      id[4] = iw.z & 0xFFFFu; id[5] = iw.z >> 16; id[6] = iw.w & 0xFFFFu; id[7] = iw.w >> 16;
    } else {
      w = gt32[g >> 3];
      const uint4* lg = reinterpret_cast<const uint4*>(im.cls_list_ids) + 2 * ((uint64_t)src + k);
      const uint4 ia = lg[0], ib = lg[1];
      id[0] = ia.x; id[1] = ia.y; id[2] = ia.z; id[3] = ia.w; id[4] = ib.x; id[5] = ib.y; id[6] = ib.z; id[7] = ib.w;
    }
    unsigned long long* racc = acc + ((size_t)L << (gshift + cshift)) + mycopy;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      if (j >= nsel || id[j] >= ns) continue;                         // (beyond the run's end: the next run's records, or padding)
      const uint32_t lab = s_label[id[j]];
      if (lab >= G) continue;
      const uint32_t gt = (w >> (groups ? 3 * (j >> 1) + 16 * (j & 1) : 4 * j)) & 7u;
      atomicAdd(racc + ((size_t)lab << cshift), group_packed(gt));
    }
  }
  // ---- denser classes: the wave per row, a lane per word of the class row, the chunk's genotype words staged in LDS ----
  uint64_t dmask = __ballot(dense);
  uint32_t* stage = s_stage[wid];
  const uint32_t wpc = im.wpc;
  while (dmask) {
    const int t = __builtin_ctzll(dmask);
    dmask &= dmask - 1;
    const uint32_t c_t = __builtin_amdgcn_readlane(cls, t);
    const uint64_t gt0_t = wave_bcast64(gt0, t);
    unsigned long long* racc = acc + ((size_t)t << (gshift + cshift)) + mycopy;
    uint64_t first = gt0_t;             // carrier record of the chunk's first carrier
    for (uint32_t wb = 0; wb < wpc; wb += 64) {
      const uint32_t wi = wb + lane;
      uint64_t rw = wi < wpc ? im.class_rows[(uint64_t)c_t * wpc + wi] : 0ull;
      if (wi == 0) rw &= ~1ull;         // bit 0 of the first word is the reference, never a carrier
      const uint32_t pc = __popcll(rw);
      const uint32_t pin = wave_inclusive_scan(pc);
      const uint32_t chunk = __builtin_amdgcn_readlane(pin, 63);   // <= 4096
      // stage words [first >> 3, (first + chunk + 7) >> 3): at most 513
      const uint64_t w0 = first >> 3;
      const uint32_t nw = (uint32_t)(((first + chunk + 7) >> 3) - w0);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");       // (the previous chunk's reads are over before it is overwritten)
      __builtin_amdgcn_wave_barrier();
      for (uint32_t i = lane; i < nw && i < kGroupStageWords; i += 64) stage[i] = groups ? im.gt_groups[w0 + i] : gt32[w0 + i];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      uint32_t kc = (uint32_t)(first - (w0 << 3)) + (pin - pc);    // the lane's first carrier, relative to the staged words
      while (rw) {                                                 // four carriers a round: their label loads are in flight together
        uint32_t lab[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
          const bool on = rw != 0;
          const uint32_t sid = wi * 64 + (on ? (uint32_t)__builtin_ctzll(rw) : 0u);
          rw &= rw - 1;
          lab[u] = on && sid < ns ? s_label[sid] : kGroupNone;
        }
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
          if (lab[u] >= G) continue;
          const uint32_t k = kc + u;
          const uint32_t sw = stage[k >> 3];
          const uint32_t gt = (sw >> (groups ? 3 * ((k & 7) >> 1) + 16 * (k & 1) : 4 * (k & 7))) & 7u;
          atomicAdd(racc + ((size_t)lab[u] << cshift), group_packed(gt));
        }
        kc += 4;
      }
      first += chunk;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  // ---- the wave's R x G records, contiguous in `out`: a 16-byte store per record, consecutive lanes consecutive records ----
  const uint64_t nrow = A - r0 < R ? A - r0 : R;
  const uint32_t ncell = (uint32_t)nrow * G;
  uint4* __restrict__ dst = out + r0 * G;
  for (uint32_t j = lane; j < ncell; j += 64) {
    const uint32_t rr = j / G, g = j - rr * G;
    const unsigned long long* cell = acc + ((((size_t)rr << gshift) + g) << cshift);
    unsigned long long s = 0;
    for (uint32_t c = 0; c < copies; ++c) s += cell[c];
    dst[j] = uint4{(uint32_t)s & 0xFFFFu, ((uint32_t)s >> 16) & 0xFFFFu, (uint32_t)(s >> 32) & 0xFFFFu, (uint32_t)(s >> 48)};
  }
}

}  // namespace vsamd
