// k_group_counts.hip.h -- allele counts per row of a type-6 plan and per sample GROUP (vs_query_group_counts): every carrier of a
// row visited once, looked up in a label-per-sample table and added to the accumulator of its (row, group).
// Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_counts.hip.h"

namespace vsamd {

// out[row * G + g] = {carriers, alt_alleles, hom_alt, phased} of table row `row` over the samples whose label is g: the record
// k_allele_counts gives with group g as the subset, for all G groups in ONE pass over the row's carriers.
//
// One wave owns R consecutive rows (R from G, below).  Every lane gathers a row's site parameters (row_site; the pieces named here
// are k_carriers.hip.h's); then
//   flat pass   explicit-id rows and the rows of listed classes (at most list_max carriers): the FLAT list of 8-carrier groups of the
//               wave's rows (flat_publish, a lane finds its row with flat_find), a lane per group: one genotype word and the group's
//               8 ids (group_load), the run's end cut by the entry count (group_nsel)
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
  __shared__ FlatRows s_rows;
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
  const CarrierForm f = carrier_form(im);
  const uint32_t ns = im.num_samples;
  // ---- the row's parameters ----
  RowSite rs{0, 0, 0};
  if (valid) rs = row_site(im, rows, u_site, row, U);   // (a dropped row counts 0 in every group)
  const bool dense = is_dense(im, f, rs.cnt);           // counted by the wave-per-row pass below
  unsigned long long* acc = s_acc[wid];
#pragma unroll
  for (uint32_t i = 0; i < kGroupCells / 64; ++i) acc[lane + 64 * i] = 0;
  const uint32_t total = flat_publish(s_rows, wid, lane, dense, rs);   // (lanes beyond R: no groups, their offsets equal the total)
  const uint32_t* off = s_rows.off[wid];
  // ---- the flat pass: one group of 8 carriers per lane and step ----
  for (uint32_t e0 = 0; e0 < total; e0 += 64) {
    const uint32_t e = e0 + lane;
    if (e >= total) continue;
    const uint32_t L = flat_find<64>(off, e);
    const uint32_t k = e - off[L], nsel = group_nsel(s_rows.cnt[wid][L], k);
    const uint64_t g = s_rows.gt0[wid][L] + 8ull * k;                 // carrier record of the group's first entry
    uint32_t id[8];
    const uint32_t w = group_load(im, f, g, s_rows.src[wid][L], k, id);
    unsigned long long* racc = acc + ((size_t)L << (gshift + cshift)) + mycopy;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      if (j >= nsel || id[j] >= ns) continue;                         // (beyond the run's end: the next run's records, or padding)
      const uint32_t lab = s_label[id[j]];
      if (lab >= G) continue;
      atomicAdd(racc + ((size_t)lab << cshift), group_packed(gt_of_slot(w, j, f.groups)));
    }
  }
  // ---- denser classes: the wave per row, a lane per word of the class row, the chunk's genotype words staged in LDS ----
  uint64_t dmask = __ballot(dense);
  uint32_t* stage = s_stage[wid];
  while (dmask) {
    const int t = __builtin_ctzll(dmask);
    dmask &= dmask - 1;
    const uint32_t c_t = __builtin_amdgcn_readlane(rs.cls, t);
    const uint64_t gt0_t = wave_bcast64(rs.gt0, t);
    unsigned long long* racc = acc + ((size_t)t << (gshift + cshift)) + mycopy;
    uint64_t first = gt0_t;             // carrier record of the chunk's first carrier
    for (uint32_t wb = 0; wb < im.wpc; wb += 64) {
      const uint32_t wi = wb + lane;
      const ClassChunk ch = class_chunk(im, c_t, wi);
      uint64_t rw = ch.rw;
      const uint32_t chunk = __builtin_amdgcn_readlane(ch.incl, 63);   // <= 4096
      // stage words [first >> 3, (first + chunk + 7) >> 3): at most 513
      const uint64_t w0 = first >> 3;
      const uint32_t nw = (uint32_t)(((first + chunk + 7) >> 3) - w0);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");       // (the previous chunk's reads are over before it is overwritten)
      __builtin_amdgcn_wave_barrier();
      for (uint32_t i = lane; i < nw && i < kGroupStageWords; i += 64) stage[i] = gt_word(im, f, w0 + i);
      wave_lds_sync();
      uint32_t kc = (uint32_t)(first - (w0 << 3)) + (ch.incl - ch.pc);   // the lane's first carrier, relative to the staged words
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
          atomicAdd(racc + ((size_t)lab[u] << cshift), group_packed(gt_of_record(stage[k >> 3], k, f.groups)));
        }
        kc += 4;
      }
      first += chunk;
    }
  }
  wave_lds_sync();
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
