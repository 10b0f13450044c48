// k_assoc.hip.h -- association scan (vs_query_assoc_scan): every row of a type-6 table scored against K phenotypes, every carrier of
// a row visited once, its K phenotype values looked up and dosage x value added to the row's K sums.  No matrix is built.
// Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_carriers.hip.h"

namespace vsamd {

// out[row * K + k] = Sxy = sum over the samples s of S of d(s) * y_k(s), d = popc(gt & 6) the dosage (VS_ASSOC_DOT), or the score
// test (VS_ASSOC_CHI2, assoc_chi2 below) formed from the row's count record over S and three sums taken about the trait's pivot c_k:
// Sxy~ = sum d(s) * (y_k(s) - c_k) here, Sy~ and Syy~ by the host.  The pivot is the trait value nearest the trait's mean over S (the
// host chooses it); the statistic does not change with it, but the cancellations in it then happen at the scale of the trait's
// spread instead of its mean.  DOT (the kernel's CHI2 parameter false) takes no pivot and no subtraction: the instructions it ran before.
//
// The shape is k_group_counts': one wave owns kAssocRows = 64 consecutive rows and 64 x Kp double accumulators in LDS (Kp: K rounded
// up to 1, 2, 4 or 8; the padding columns of the phenotype table are zero).  The pieces named here are k_carriers.hip.h's.
//   flat pass   explicit-id rows and the rows of listed classes: the flat list of 8-carrier groups of the wave's rows (flat_publish /
//               flat_find), a lane per group and step: the genotype word and 8 ids (group_load, group_nsel), per carrier column_of,
//               one vector load of the carrier's Kp floats and Kp multiply-adds into the lane's registers, carriers in slot order
//   dense pass  a denser class row: the wave per row, a lane per 64-bit word of the class row, 64 words a chunk (class_chunk), the
//               chunk's genotype words staged in LDS once; a lane sums its word's carriers in bit order, chunk after chunk
// The phenotype table is [column][Kp] float32 in column order (column_of<SUBSET>, one tile over all columns), either staged in LDS by
// the workgroup (LDSTAB) or read through global memory, where a table of tens of KB sits in L2.  Both forms add the same numbers in
// the same order: their scores are the same bytes.
//
// NO floating-point atomic, in LDS or global memory: the order of a row's additions is fixed by the table's layout alone, so the same
// call gives the same bytes every time.
//   flat   the lanes of a step that hold groups of one row are consecutive: a segmented inclusive scan across the lanes keyed by
//          the row (6 shuffle steps per double), then ONE plain LDS read-add-write of acc[row][k] by the segment's last lane.  A row
//          has one segment per step, the steps of a wave are sequential and no other wave owns the row.
//   dense  lane-private sums, a butterfly over the wave (6 steps, the same tree every time), lane 0 adds.
// y - c is taken in double (exact unless the two lie 29 binary places apart; c sits in scalar registers: a uniform load of the kernel's
// arguments).  A product d * (y - c) is exact in double (d is 0, 1 or 2), so a fused multiply-add rounds as multiply-then-add does.
//
// LDS per workgroup (4 waves), from MI355X_MICROARCH.md (160 KiB per CU, workgroups per CU <= 160 KiB / LDS per workgroup, 64 KiB per
// workgroup unless the launch asks for more):
//   static   accumulators 4 x 64 x Kp x 8 = 2048 Kp B + staged genotype words 4 x 520 x 4 = 8320 B + wave state (FlatRows) 5136 B
//            + Sy / Syy 128 B:  Kp = 1: 15632 B   2: 17680 B   4: 21776 B   8: 29968 B
//   dynamic  SUBSET: the mask, 8 B a word, and its ranks, 4 B a word, each rounded up to 16 B (2504 samples: 320 + 160 B; at most
//            kCountMaskMaxBytes = 48 KiB + 24 KiB, the limit k_allele_counts sets for the counts of the same batch)
//            LDSTAB: the table, n x Kp x 4 B, at most option assoc_lds_max_kib (default 32 KiB, at most 128 KiB)
//   global form, whole cohort:        15.3 .. 29.3 KiB  -> 10 .. 5 workgroups per CU by LDS (at most 8 by the 32 waves a CU holds)
//   LDS form, 2504 samples, Kp = 8:   29968 + 80128 B = 107.5 KiB (above the 32 KiB default: only on request)  -> 1 workgroup per CU
//   LDS form, 2504 samples, Kp = 1:   15632 + 10016 B = 25.0 KiB  -> 6 per CU
//   LDS form at the default limit:    Kp = 8: 29968 + 32768 B = 61.3 KiB (+ mask and ranks)  -> 2 per CU
// The engine takes the global form when static + dynamic would pass 160 KiB.
//
// Output: the K cells of a wave's rows are contiguous in `out`: consecutive lanes store consecutive cells with plain 8-byte stores,
// every cell exactly once -- zeros of dropped and empty rows and the cells of a table that ends inside a wave's rows included.  No
// memset; nothing of a recycled buffer shows through.
//
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage): VGPRs / SGPRs, then waves per SIMD by registers;
// scratch 0 bytes per lane, no SGPR or VGPR spill in any instantiation; <Kp, SUBSET, LDSTAB> under DOT, then under CHI2:
//   <1,0,0> 46/76 8   <1,0,1> 48/74 8   <1,1,0> 48/79 8   <1,1,1> 48/78 8      <2,0,0> 48/76 8   <2,0,1> 48/74 8   <2,1,0> 48/79 8   <2,1,1> 48/78 8
//   <4,0,0> 56/76 7   <4,0,1> 54/74 7   <4,1,0> 56/79 7   <4,1,1> 54/78 7      <8,0,0> 74/76 5   <8,0,1> 68/74 5   <8,1,0> 72/79 5   <8,1,1> 68/78 5
//   <1,0,0> 46/78 8   <1,0,1> 48/76 8   <1,1,0> 48/81 8   <1,1,1> 48/80 8      <2,0,0> 48/80 8   <2,0,1> 48/78 8   <2,1,0> 48/83 8   <2,1,1> 48/82 8
//   <4,0,0> 56/84 7   <4,0,1> 54/82 7   <4,1,0> 56/87 7   <4,1,1> 54/86 7      <8,0,0> 74/92 5   <8,0,1> 68/90 5   <8,1,0> 72/95 5   <8,1,1> 68/94 5
// At Kp = 8 the registers allow 5 waves per SIMD = 5 workgroups per CU, which is what the static LDS allows as well.  CHI2's pivots
// are the 2 Kp scalar registers it holds more than DOT.  The template parameter CHI2 governs the pivot alone and the epilogue reads the
// statistic from the arguments, as it did before there was a pivot: a DOT instantiation is that kernel, instruction for instruction.
constexpr uint32_t kAssocRows = 64;
constexpr uint32_t kAssocStageWords = 520;        // 4096 carriers of a 64-word chunk = 512 words, + 1 (unaligned start), rounded up
constexpr uint32_t kAssocTraitsMax = 8;
constexpr size_t kAssocLdsPerCu = 160 << 10;
constexpr size_t kAssocHeadWords = 3 * kAssocTraitsMax;   // the doubles in front of the phenotype table in the upload (AssocArgs::sums)
__host__ __device__ constexpr uint32_t assoc_pow2(uint32_t k) { return k <= 1 ? 1u : k <= 2 ? 2u : k <= 4 ? 4u : 8u; }
__host__ __device__ constexpr size_t assoc_static_lds(uint32_t kp) { return 4ull * kAssocRows * kp * 8 + 4ull * kAssocStageWords * 4 + 5136 + 128; }

struct AssocArgs {
  const VariantRow* rows; const uint32_t* u_site; uint64_t A, U;
  const uint64_t* S; const uint32_t* S_rank; uint32_t s_words;   // the subset's mask and the columns in front of each word (SUBSET)
  uint32_t n_cols, K, chi2;
  const double* sums;      // Sy~[8], Syy~[8] about the pivots, then the pivots c[8] (read under CHI2 only)
  const float* table;      // [n_cols][Kp]
  const uint4* counts;     // the rows' count records over S (k_allele_counts, the launch before this one)
  double* out;
};

// the Kp floats of a column: one vector load of 4 to 16 bytes, two of 16 at Kp = 8
template <uint32_t KP>
__device__ __forceinline__ void pheno_load(const float* __restrict__ tab, uint32_t col, float (&y)[KP]) {
  const float* p = tab + (size_t)col * KP;
  if constexpr (KP == 1) y[0] = p[0];
  else if constexpr (KP == 2) { const float2 v = *reinterpret_cast<const float2*>(p); y[0] = v.x; y[1] = v.y; }
  else {
#pragma unroll
    for (uint32_t q = 0; q < KP / 4; ++q) {
      const float4 v = reinterpret_cast<const float4*>(p)[q];
      y[4 * q] = v.x; y[4 * q + 1] = v.y; y[4 * q + 2] = v.z; y[4 * q + 3] = v.w;
    }
  }
}

// y~ = y - c in double under CHI2; y under DOT, whose cells are the sums of d * y and cost no subtraction
template <bool CHI2>
__device__ __forceinline__ double about(float y, double c) {
  if constexpr (CHI2) return (double)y - c;
  else return (double)y;
}

// The score test of a regression of y on the dosage without covariates, n cov^2 / (vx vy), from the row's record over S
// (Sx = alt_alleles, Sxx = alt_alleles + 2 hom_alt) and the trait's Sy~ / Syy~ and the cell's Sxy~ about the pivot -- in exactly this
// order of operations, each rounded on its own (no contraction: cov and vy cancel, and a fused product would move them by more than
// the last bit).  About the pivot Sy~ is of the order of one standard deviation, so p2 is small beside p1 and q2 beside q1: what
// cancels is what the data cancel.  A constant trait has every y~ = 0: vy = 0 exactly.
__device__ __forceinline__ double assoc_chi2(uint32_t n, const uint4 rec, double sy, double syy, double sxy) {
#pragma clang fp contract(off)
  const long long sx = rec.y, sxx = (long long)rec.y + 2ll * rec.z;
  const long long vx = (long long)n * sxx - sx * sx;
  const double dn = (double)n;
  const double p1 = dn * sxy, p2 = (double)sx * sy;
  const double cov = p1 - p2;
  const double q1 = dn * syy, q2 = sy * sy;
  const double vy = q1 - q2;
  if (vx == 0 || !(vy > 0.0)) return 0.0;
  const double num = (dn * cov) * cov, den = (double)vx * vy;
  return num / den;
}

template <uint32_t KP, bool SUBSET, bool LDSTAB, bool CHI2>
__global__ void __launch_bounds__(256) k_assoc_scan(DevImage im, AssocArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_assoc[];   // SUBSET: mask, ranks; LDSTAB: the table
  __shared__ FlatRows s_rows;
  __shared__ double s_acc[4][kAssocRows * KP];
  __shared__ uint32_t s_stage[4][kAssocStageWords];
  __shared__ double s_sums[2 * kAssocTraitsMax];
  uint8_t* p = s_assoc;
  uint64_t* s_mask = reinterpret_cast<uint64_t*>(p);
  if (SUBSET) p += ((size_t)a.s_words * 8 + 15) / 16 * 16;
  uint32_t* s_rank = reinterpret_cast<uint32_t*>(p);
  if (SUBSET) p += ((size_t)a.s_words * 4 + 15) / 16 * 16;
  float* s_tab = reinterpret_cast<float*>(p);
  if (SUBSET)
    for (uint32_t i = threadIdx.x; i < a.s_words; i += blockDim.x) { s_mask[i] = a.S[i]; s_rank[i] = a.S_rank[i]; }
  if (LDSTAB) {   // n_cols x KP floats: a multiple of 4 bytes, whole 16-byte words first
    const uint32_t nf = a.n_cols * KP;
    for (uint32_t i = threadIdx.x; i < nf / 4; i += blockDim.x) reinterpret_cast<float4*>(s_tab)[i] = reinterpret_cast<const float4*>(a.table)[i];
    for (uint32_t i = (nf & ~3u) + threadIdx.x; i < nf; i += blockDim.x) s_tab[i] = a.table[i];
  }
  if (threadIdx.x < 2 * kAssocTraitsMax) s_sums[threadIdx.x] = a.sums[threadIdx.x];
  __syncthreads();
  const float* __restrict__ tab = LDSTAB ? s_tab : a.table;
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t r0 = (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * kAssocRows;
  if (r0 >= a.A) return;
  const uint64_t row = r0 + lane;
  const bool valid = row < a.A;
  double piv[KP];            // CHI2 only; uniform: scalar loads, scalar registers
#pragma unroll
  for (uint32_t k = 0; k < KP; ++k) piv[k] = CHI2 ? a.sums[2 * kAssocTraitsMax + k] : 0.0;
  const CarrierForm f = carrier_form(im);
  const ColumnTile t{s_mask, s_rank, 0u, a.n_cols, im.num_samples};   // one tile over all columns
  // ---- the row's parameters ----
  RowSite rs{0, 0, 0};
  if (valid) rs = row_site(im, a.rows, a.u_site, row, a.U);   // (a dropped row has no carriers: its cells are 0)
  const bool dense = is_dense(im, f, rs.cnt);                 // summed by the wave-per-row pass below
  double* acc = s_acc[wid];
#pragma unroll
  for (uint32_t i = 0; i < KP; ++i) acc[lane + 64 * i] = 0.0;
  const uint32_t total = flat_publish(s_rows, wid, lane, dense, rs);
  const uint32_t* off = s_rows.off[wid];
  // ---- the flat pass: one group of 8 carriers per lane and step ----
  for (uint32_t e0 = 0; e0 < total; e0 += 64) {
    const uint32_t e = e0 + lane;
    const bool on = e < total;
    uint32_t L = kAssocRows;   // a lane without a group: a segment of its own behind the step's last row
    double s[KP];
#pragma unroll
    for (uint32_t k = 0; k < KP; ++k) s[k] = 0.0;
    if (on) {
      L = flat_find<kAssocRows>(off, e);
      const uint32_t k8 = e - off[L], nsel = group_nsel(s_rows.cnt[wid][L], k8);
      const uint64_t g = s_rows.gt0[wid][L] + 8ull * k8;               // carrier record of the group's first entry
      uint32_t id[8];
      const uint32_t w = group_load(im, f, g, s_rows.src[wid][L], k8, id);
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) {
        uint32_t col;
        if (j >= nsel || !column_of<SUBSET>(t, id[j], col)) continue;   // beyond the run's end; padding, "ref", outside S
        float y[KP];
        pheno_load<KP>(tab, col, y);
        const double d = (double)__popc(gt_of_slot(w, j, f.groups) & 6u);
#pragma unroll
        for (uint32_t k = 0; k < KP; ++k) s[k] = __builtin_fma(d, about<CHI2>(y[k], piv[k]), s[k]);
      }
    }
    // the groups of a row are consecutive lanes: inclusive scan within the segments of equal L
#pragma unroll
    for (uint32_t dist = 1; dist < 64; dist <<= 1) {
      const uint32_t Lu = (uint32_t)__shfl_up((int)L, dist, 64);
      const bool take = lane >= dist && Lu == L;
#pragma unroll
      for (uint32_t k = 0; k < KP; ++k) {
        const double v = __shfl_up(s[k], dist, 64);
        if (take) s[k] += v;
      }
    }
    const uint32_t Ln = (uint32_t)__shfl_down((int)L, 1, 64);
    if (on && (lane == 63 || Ln != L)) {
#pragma unroll
      for (uint32_t k = 0; k < KP; ++k) acc[L * KP + k] += s[k];
    }
    wave_lds_sync();   // (the next step's segment of the same row adds behind this one)
  }
  // ---- denser classes: the wave per row, a lane per word of the class row, the chunk's genotype words staged in LDS ----
  uint64_t dmask = __ballot(dense);
  uint32_t* stage = s_stage[wid];
  while (dmask) {
    const int tl = __builtin_ctzll(dmask);
    dmask &= dmask - 1;
    const uint32_t c_t = __builtin_amdgcn_readlane(rs.cls, tl);
    const uint64_t gt0_t = wave_bcast64(rs.gt0, tl);
    double s[KP];
#pragma unroll
    for (uint32_t k = 0; k < KP; ++k) s[k] = 0.0;
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
      for (uint32_t i = lane; i < nw && i < kAssocStageWords; i += 64) stage[i] = gt_word(im, f, w0 + i);
      wave_lds_sync();
      uint32_t kc = (uint32_t)(first - (w0 << 3)) + (ch.incl - ch.pc);   // the lane's first carrier, relative to the staged words
      while (rw) {                                                 // the lane's carriers in bit order; their records are consecutive
        const uint32_t sid = wi * 64 + (uint32_t)__builtin_ctzll(rw);
        rw &= rw - 1;
        uint32_t col;
        if (column_of<SUBSET>(t, sid, col)) {
          float y[KP];
          pheno_load<KP>(tab, col, y);
          const double d = (double)__popc(gt_of_record(stage[kc >> 3], kc, f.groups) & 6u);
#pragma unroll
          for (uint32_t k = 0; k < KP; ++k) s[k] = __builtin_fma(d, about<CHI2>(y[k], piv[k]), s[k]);
        }
        kc += 1;
      }
      first += chunk;
    }
    // the wave's sum: the same butterfly every time, every lane ends with the same bits
#pragma unroll
    for (uint32_t m = 32; m; m >>= 1) {
#pragma unroll
      for (uint32_t k = 0; k < KP; ++k) s[k] += __shfl_xor(s[k], m, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (uint32_t k = 0; k < KP; ++k) acc[(uint32_t)tl * KP + k] += s[k];
    }
  }
  wave_lds_sync();
  // ---- the wave's rows x K cells, contiguous in `out`: consecutive lanes consecutive cells ----
  const uint64_t nrow = a.A - r0 < kAssocRows ? a.A - r0 : kAssocRows;
  const uint32_t K = a.K, ncell = (uint32_t)nrow * K;
  double* __restrict__ dst = a.out + r0 * K;
  for (uint32_t j = lane; j < ncell; j += 64) {
    const uint32_t rr = j / K, k = j - rr * K;
    double v = acc[rr * KP + k];
    if (a.chi2) v = assoc_chi2(a.n_cols, a.counts[r0 + rr], s_sums[k], s_sums[kAssocTraitsMax + k], v);
    dst[j] = v;
  }
}

}  // namespace vsamd
