// k_counts.hip.h -- allele counts per row of a type-6 plan (vs_query_allele_counts): the carrier expansion replaced by a count.
// Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_carriers.hip.h"

namespace vsamd {

// Every row of the table gets {carriers, alt_alleles, hom_alt, phased} over the carriers that lie in the sample subset S
// (16 bytes).  The counts come from the genotype bits the index stores per carrier (bit 0 phase, bit 1 gt_1, bit 2 gt_2).
//
// One wave owns kCountRows consecutive rows; every lane gathers its row's site parameters, then the wave works through the
// FLAT list of 8-carrier groups of all its rows (a DPP prefix sum over the group counts, a lane finds its row by bisection over
// the 64 offsets in LDS), as the list path of the expansion does.  A group is one genotype word: gt_groups (class-row cohorts of
// at most 4032 samples: genotype j at bit 3 (j / 2) + 16 (j & 1)) or eight nibbles of gt_nibbles.  Per group the counts are
// popcounts of the word under masks; the groups of one pass are summed per row by a wave prefix sum of the packed counts whose
// segment boundaries add into the row's LDS accumulator (the lane that ends a segment adds its prefix to its row and takes it
// off the next one): at most two LDS atomics per lane and pass, none of them on a contended address.
//
// With a subset S (a bit per sample, in LDS):
//   explicit-id cohorts   the group's 8 ids from car_sid, tested against S
//   listed classes        (at most list_max carriers) the group's 8 ids from the class's decoded list, tested against S
//   denser classes        a WAVE per row after the flat pass: a lane per word of the class row, m = row & S, the carrier index
//                         of a bit is the prefix popcount of the row; the genotype of each selected carrier is read by index
// Without S every carrier counts: carriers = s_ncar, and the groups are read whole.  Class-row pools are padded with zeros (a
// vertex's records start on a multiple of 8); explicit-id pools are not, so a group there is an unaligned window of the nibble
// stream whose nibbles beyond the run are masked off.
constexpr uint32_t kCountRows = 64;
constexpr uint32_t kCountDepth = 4;   // flat-pass steps whose loads are issued together (the pass is latency-bound: a dependent load per step)
constexpr size_t kCountMaskMaxBytes = 48 << 10;   // the subset's bit mask in LDS (dynamic, beside ~10 KiB of the waves' own)
constexpr uint32_t kGroupM0 = 0x02490249u;   // the phase bit of each genotype of a gt_groups word
constexpr uint32_t kNibM0 = 0x11111111u;     // the phase bit of each nibble

// packed per-group counts: lo = carriers | hom << 16, hi = alt | phased << 16 (a pass of 64 groups stays below 2^16 per field)
struct GroupCounts { uint32_t lo, hi; };
__device__ __forceinline__ GroupCounts counts_of(uint32_t w, uint32_t m0, uint32_t carriers) {
  const uint32_t alt = __popc(w & (m0 << 1)) + __popc(w & (m0 << 2));
  const uint32_t hom = __popc((w >> 1) & (w >> 2) & m0);
  const uint32_t ph = __popc(w & m0);
  return GroupCounts{carriers | (hom << 16), alt | (ph << 16)};
}
// the genotype-field mask of the selected entries j (bit j of sel) of a group word
__device__ __forceinline__ uint32_t sel_mask(uint32_t sel, bool groups) {
  uint32_t m = 0;
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j)
    if ((sel >> j) & 1u) m |= 7u << gt_shift(j, groups);
  return m;
}
__device__ __forceinline__ bool in_set(const uint64_t* s_mask, uint32_t sid) { return (s_mask[sid >> 6] >> (sid & 63)) & 1ull; }
// a packed 32-bit pair of 16-bit fields as a 64-bit pair of 32-bit fields (the accumulators add whole rows: up to 2 x samples)
__device__ __forceinline__ unsigned long long widen(uint32_t v) { return (unsigned long long)(v & 0xFFFFu) | ((unsigned long long)(v >> 16) << 32); }

// group k of a row (count rcnt, first carrier record gt0, list group / class src): its packed counts
template <bool SUBSET>
__device__ __forceinline__ GroupCounts group_counts(const DevImage& im, const CarrierForm& f, const uint64_t* s_mask, uint32_t k, uint32_t rcnt, uint64_t gt0,
                                                    uint32_t src) {
  const uint32_t nsel_all = group_nsel(rcnt, k);
  const uint64_t g = gt0 + 8ull * k;                                      // carrier record of the group's first entry
  const uint32_t m0 = f.groups ? kGroupM0 : kNibM0;
  if (!SUBSET) {   // no ids: the word alone
    uint32_t w = group_word(im, f, g);
    if (f.explicit_ids && nsel_all < 8) w &= (1u << (4 * nsel_all)) - 1u;   // the run ends inside the window
    return counts_of(w, m0, 0);
  }
  uint32_t id[8];
  const uint32_t w = group_load(im, f, g, src, k, id);
  uint32_t sel = 0;
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j)
    if (j < nsel_all && id[j] < im.num_samples && in_set(s_mask, id[j])) sel |= 1u << j;
  return counts_of(w & sel_mask(sel, f.groups), m0, __popc(sel));
}

// u_site: the site of every row of the table (row_site).  S == NULL: the whole cohort.
template <bool SUBSET>
__global__ void __launch_bounds__(256) k_allele_counts(DevImage im, const VariantRow* __restrict__ rows, const uint32_t* __restrict__ u_site, uint64_t A,
                                                       uint64_t U, const uint64_t* __restrict__ S, uint32_t s_words, uint4* __restrict__ out) {
  extern __shared__ uint64_t s_mask[];   // SUBSET: S, s_words words, shared by the block's waves
  __shared__ FlatRows s_rows;
  __shared__ unsigned long long s_acc[4][2][kCountRows];
  if (SUBSET) {
    for (uint32_t i = threadIdx.x; i < s_words; i += blockDim.x) s_mask[i] = S[i];
    __syncthreads();
  }
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t r0 = (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * kCountRows;
  if (r0 >= A) return;
  const uint64_t row = r0 + lane;
  const bool valid = row < A;
  const CarrierForm f = carrier_form(im);
  // ---- the row's parameters ----
  RowSite rs{0, 0, 0};
  if (valid) rs = row_site(im, rows, u_site, row, U);
  const bool dense = SUBSET && is_dense(im, f, rs.cnt);   // counted by the wave-per-row pass below
  s_acc[wid][0][lane] = 0;
  s_acc[wid][1][lane] = 0;
  const uint32_t total = flat_publish(s_rows, wid, lane, dense, rs);
  const uint32_t* off = s_rows.off[wid];
  // ---- the flat pass: one group of 8 carriers per lane and step, kCountDepth steps' loads in flight at a time ----
  for (uint32_t e00 = 0; e00 < total; e00 += 64 * kCountDepth) {
    GroupCounts c[kCountDepth];
    uint32_t Ls[kCountDepth];
#pragma unroll
    for (uint32_t d = 0; d < kCountDepth; ++d) {
      const uint32_t e = e00 + 64 * d + lane;
      const uint32_t L = Ls[d] = flat_find<kCountRows>(off, e);
      c[d] = GroupCounts{0, 0};
      if (e < total) c[d] = group_counts<SUBSET>(im, f, s_mask, e - off[L], s_rows.cnt[wid][L], s_rows.gt0[wid][L], s_rows.src[wid][L]);
    }
    // sum per row: segments of equal L are contiguous in a step
#pragma unroll
    for (uint32_t d = 0; d < kCountDepth; ++d) {
      const uint32_t e = e00 + 64 * d + lane, L = Ls[d];
      const uint32_t plo = wave_inclusive_scan(c[d].lo), phi = wave_inclusive_scan(c[d].hi);
      const uint32_t L_next = (uint32_t)__shfl_down((int)L, 1, 64);
      const bool last = lane == 63 || e + 1 >= total;
      if (e < total && (last || L_next != L)) {
        atomicAdd(&s_acc[wid][0][L], widen(plo));
        atomicAdd(&s_acc[wid][1][L], widen(phi));
        if (!last) {   // the next segment's prefix starts with ours: take it off its row
          atomicAdd(&s_acc[wid][0][L_next], 0ull - widen(plo));
          atomicAdd(&s_acc[wid][1][L_next], 0ull - widen(phi));
        }
      }
    }
  }
  // ---- denser classes with a subset: a wave per row, a lane per word of the class row ----
  uint64_t dmask = SUBSET ? __ballot(dense) : 0ull;
  while (dmask) {
    const int t = __builtin_ctzll(dmask);
    dmask &= dmask - 1;
    const uint32_t c_t = __builtin_amdgcn_readlane(rs.cls, t);
    const uint64_t gt0_t = wave_bcast64(rs.gt0, t);
    uint32_t base = 0;                 // carriers in the row words before this chunk
    uint32_t a_car = 0, a_hom = 0, a_alt = 0, a_ph = 0;
    for (uint32_t wb = 0; wb < im.wpc; wb += 64) {
      const uint32_t wi = wb + lane;
      const ClassChunk ch = class_chunk(im, c_t, wi);
      uint64_t m = wi < s_words ? ch.rw & s_mask[wi] : 0ull;
      while (m) {
        const int b = __builtin_ctzll(m);
        m &= m - 1;
        const uint64_t kc = gt0_t + base + (ch.incl - ch.pc) + __popcll(ch.rw & ((1ull << b) - 1ull));   // carrier record of sample wi * 64 + b
        const uint32_t gt = gt_of_record(gt_word(im, f, kc >> 3), kc, f.groups);
        a_car += 1;
        a_ph += gt & 1u;
        a_alt += ((gt >> 1) & 1u) + ((gt >> 2) & 1u);
        a_hom += (gt >> 1) & (gt >> 2) & 1u;
      }
      base += __builtin_amdgcn_readlane(ch.incl, 63);
    }
    a_car = wave_inclusive_scan(a_car); a_hom = wave_inclusive_scan(a_hom); a_alt = wave_inclusive_scan(a_alt); a_ph = wave_inclusive_scan(a_ph);
    if (lane == 63) {
      s_acc[wid][0][t] = (unsigned long long)a_car | ((unsigned long long)a_hom << 32);
      s_acc[wid][1][t] = (unsigned long long)a_alt | ((unsigned long long)a_ph << 32);
    }
  }
  wave_lds_sync();
  if (!valid) return;
  const unsigned long long a0 = s_acc[wid][0][lane], a1 = s_acc[wid][1][lane];
  const uint32_t carriers = SUBSET ? (uint32_t)a0 : rs.cnt;
  out[row] = uint4{carriers, (uint32_t)a1, (uint32_t)(a0 >> 32), (uint32_t)(a1 >> 32)};
}

// The site of every private row of the regions under the duplicate rule (k_t6_slow's copies: region q's rows
// [var_begin[q], var_begin[q] + q_nvar[q]) are its sites q_g0[q] ...).  One wave per such region.
__global__ void __launch_bounds__(256) k_count_slow_sites(DevResult r, const uint32_t* slow_list, uint64_t n, uint32_t* u_site) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  for (uint64_t i = wave; i < n; i += nwaves) {
    const uint64_t q = slow_list[i];
    const uint64_t a0 = r.var_begin[q], nv = r.q_nvar[q];
    const uint32_t g0 = r.q_g0[q];
    for (uint64_t j = lane; j < nv; j += 64) u_site[a0 + j] = g0 + (uint32_t)j;
  }
}

}  // namespace vsamd
