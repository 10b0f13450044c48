// k_burden.hip.h -- per-sample burden of a type-6 plan (vs_query_sample_burden): a regions x samples matrix of counts.
// Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_counts.hip.h"

namespace vsamd {

// Cell (q, c) of the matrix is {variants, alt_alleles, hom_alt, phased} (16 bytes) over the rows region q reports of which column
// c's sample is a carrier -- the same genotype bits, per carrier, that k_allele_counts sums per row.  With a window the rows whose
// alt_alleles (k_allele_counts over the same subset, run first) lie outside [min_ac, max_ac] are skipped.
//
// A workgroup owns ONE (region, column tile) pair: the tile's cells live in LDS as two 64-bit words per column (variants | alt << 32,
// hom | phased << 32: a carrier is one or two LDS atomics, and no field can carry into its neighbour -- each stays below the
// region's row count x 2), the four waves walk the region's rows 256 at a time (lane l of wave w takes row 4 l + w, so a region of
// thirty rows still occupies every wave), and the tile is written with plain 16-byte stores, zeros included: the matrix needs no
// memset.  Per 64 rows a wave works as k_allele_counts does: the listed rows and the rows of explicit-id cohorts as a FLAT list of
// 8-carrier groups (ids from cls_list16 / cls_list_ids / car_sid, the genotype word from gt_groups / gt_nibbles), then the classes
// denser than list_max a row at a time, a lane per word of the class row (the carrier index of a bit is the prefix popcount).
//
// The column of sample id: id - 1 without a subset; with one, the rank of id in S -- per-word prefix popcounts of the mask
// (s_rank) sit in LDS behind the mask.
//
// A region of more than chunk_rows rows is SPLIT: the workgroup above writes zeros for it, k_burden_split_plan lists its chunks
// (region, chunk) on the device, and a second launch (SPLIT) walks one chunk per workgroup and adds its nonzero cells to the
// matrix with 64-bit global atomics.  A batch without such a region launches neither.
constexpr uint32_t kBurdenTileCols = 4096;         // 64 KiB of cells: a second workgroup fits a CU's 160 KiB
constexpr uint32_t kBurdenChunkRows = 4096;        // rows one workgroup walks before a region is split
constexpr size_t kBurdenMaskMaxBytes = 40 << 10;   // the subset's bit mask in LDS (its ranks take half as much again)

struct BurdenArgs {
  const VariantRow* rows;       // the table
  const uint32_t* u_site;       // the site of every table row
  uint64_t U;                   // shared rows: the rows behind them are private and may be dropped
  const uint64_t* var_begin;    // per region, in the caller's order
  const uint64_t* q_nvar;
  const uint64_t* S;            // SUBSET: the mask and the columns in front of each of its words
  const uint32_t* S_rank;
  uint32_t s_words;
  const uint4* ac;              // WINDOW: k_allele_counts' output per table row
  uint32_t min_ac, max_ac;
  uint32_t n_cols, tile_cols, n_tiles, chunk_rows;
  const uint2* work;            // SPLIT: {region, chunk}
  const uint32_t* n_work;
  uint4* cells;                 // [Q x n_cols]
  unsigned long long* total;    // sum of `variants` over the matrix
};

struct BurdenTile { unsigned long long* cell; const uint64_t* mask; const uint32_t* rank; uint32_t tile0, tn, num_samples; };

// one carrier (sample id, 3 genotype bits) into its cell, if the tile holds its column
template <bool SUBSET>
__device__ __forceinline__ void burden_add(const BurdenTile& t, uint32_t id, uint32_t gt) {
  if (id - 1u >= t.num_samples - 1u) return;   // "ref" (id 0) and the padding of a list
  uint32_t col = id - 1u;
  if (SUBSET) {
    const uint64_t mw = t.mask[id >> 6], bit = 1ull << (id & 63);
    if (!(mw & bit)) return;
    col = t.rank[id >> 6] + __popcll(mw & (bit - 1ull));
  }
  col -= t.tile0;
  if (col >= t.tn) return;
  const uint32_t g1 = (gt >> 1) & 1u, g2 = (gt >> 2) & 1u, ph = gt & 1u;
  atomicAdd(&t.cell[2 * col], 1ull | ((unsigned long long)(g1 + g2) << 32));
  if ((g1 & g2) | ph) atomicAdd(&t.cell[2 * col + 1], (unsigned long long)(g1 & g2) | ((unsigned long long)ph << 32));
}

// group k of a row (count rcnt, first carrier record gt0, list group src): its up to 8 carriers
template <bool SUBSET>
__device__ __forceinline__ void burden_group(const DevImage& im, const BurdenTile& t, uint32_t k, uint32_t rcnt, uint64_t gt0, uint32_t src, bool groups,
                                             bool explicit_ids, const uint32_t* __restrict__ gt32) {
  const uint32_t rem = rcnt - 8 * k;
  const uint32_t nsel = rem < 8 ? rem : 8u;
  const uint64_t g = gt0 + 8ull * k;
  uint32_t w;
  uint32_t id[8];
  if (explicit_ids) {   // unpadded pool: a window of the nibble stream, entries beyond the run belong to the next one
    uint2 nw;
    __builtin_memcpy(&nw, gt32 + (g >> 3), 8);
    w = __builtin_amdgcn_alignbit(nw.y, nw.x, ((uint32_t)g & 7u) * 4);
    uint4 ia, ib;
    __builtin_memcpy(&ia, im.car_sid + g, 16);
    __builtin_memcpy(&ib, im.car_sid + g + 4, 16);
    id[0] = ia.x; id[1] = ia.y; id[2] = ia.z; id[3] = ia.w; id[4] = ib.x; id[5] = ib.y; id[6] = ib.z; id[7] = ib.w;
  } else if (groups) {
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
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j)
    if (j < nsel) burden_add<SUBSET>(t, id[j], (w >> (groups ? 3 * (j >> 1) + 16 * (j & 1) : 4 * j)) & 7u);
}

template <bool SUBSET, bool WINDOW, bool SPLIT>
__global__ void __launch_bounds__(256) k_sample_burden(DevImage im, BurdenArgs a) {
  extern __shared__ unsigned long long s_dyn[];   // tile_cols x 2 cell words | SUBSET: s_words mask words | s_words ranks
  __shared__ uint32_t s_off[4][65];
  __shared__ uint32_t s_src[4][64];
  __shared__ uint32_t s_cnt[4][64];
  __shared__ uint64_t s_gt0[4][64];
  __shared__ unsigned long long s_sum;
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t item = blockIdx.x / a.n_tiles;
  const uint32_t tile = blockIdx.x % a.n_tiles;
  if (SPLIT && item >= *a.n_work) return;
  const uint64_t q = SPLIT ? a.work[item].x : item;
  const uint64_t a0 = a.var_begin[q], nv = a.q_nvar[q];
  uint64_t r_begin = a0, r_end = a0 + nv;
  if (SPLIT) {
    r_begin = a0 + (uint64_t)a.work[item].y * a.chunk_rows;
    if (r_end > r_begin + a.chunk_rows) r_end = r_begin + a.chunk_rows;
  } else if (nv > a.chunk_rows) r_end = r_begin;   // a split region: zeros here, its chunks add to them
  BurdenTile t;
  t.cell = s_dyn;
  t.mask = reinterpret_cast<const uint64_t*>(s_dyn + 2 * (size_t)a.tile_cols);
  t.rank = reinterpret_cast<const uint32_t*>(t.mask + a.s_words);
  t.tile0 = tile * a.tile_cols;
  t.tn = a.n_cols - t.tile0 < a.tile_cols ? a.n_cols - t.tile0 : a.tile_cols;
  t.num_samples = im.num_samples;
  for (uint32_t i = threadIdx.x; i < 2 * t.tn; i += 256) s_dyn[i] = 0;
  if (SUBSET)
    for (uint32_t i = threadIdx.x; i < a.s_words; i += 256) {
      const_cast<uint64_t*>(t.mask)[i] = a.S[i];
      const_cast<uint32_t*>(t.rank)[i] = a.S_rank[i];
    }
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  const bool groups = im.use_bv && im.wpc <= 63;
  const bool explicit_ids = !im.use_bv;
  const uint32_t* __restrict__ gt32 = reinterpret_cast<const uint32_t*>(im.gt_nibbles);
  uint32_t* off = s_off[wid];
  for (uint64_t base = r_begin; base < r_end; base += 256) {
    // ---- the parameters of this wave's 64 rows ----
    const uint64_t row = base + 4 * lane + wid;
    uint32_t cnt = 0, cls = 0;
    uint64_t gt0 = 0;
    if (row < r_end) {
      const uint32_t g = a.u_site[row];
      cnt = im.s_ncar[g];
      if (row >= a.U && (a.rows[row].count_flags & kRowDropped)) cnt = 0;   // dropped by the duplicate rule: reports nothing
      if (WINDOW) {
        const uint32_t ac = a.ac[row].y;
        if (ac < a.min_ac || ac > a.max_ac) cnt = 0;
      }
      cls = im.s_class[g];
      gt0 = im.s_gt0[g];
    }
    const bool dense = !explicit_ids && cnt > im.list_max;
    const uint32_t ng = dense ? 0u : (cnt + 7) / 8;
    const uint32_t incl = wave_inclusive_scan(ng);
    const uint32_t total = __builtin_amdgcn_readlane(incl, 63);
    off[lane] = incl - ng;
    if (lane == 0) off[64] = total;
    s_src[wid][lane] = cls;
    s_cnt[wid][lane] = cnt;
    s_gt0[wid][lane] = gt0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // ---- the flat pass: one group of 8 carriers per lane and step ----
    for (uint32_t e = lane; e < total; e += 64) {
      uint32_t L = 0;
#pragma unroll
      for (uint32_t step = 32; step; step >>= 1)
        if (off[L + step] <= e) L += step;
      burden_group<SUBSET>(im, t, e - off[L], s_cnt[wid][L], s_gt0[wid][L], s_src[wid][L], groups, explicit_ids, gt32);
    }
    // ---- denser classes: a row at a time, a lane per word of the class row ----
    uint64_t dmask = __ballot(dense);
    while (dmask) {
      const int r = __builtin_ctzll(dmask);
      dmask &= dmask - 1;
      const uint32_t c_r = __builtin_amdgcn_readlane(cls, r);
      const uint64_t gt0_r = wave_bcast64(gt0, r);
      const uint32_t wpc = im.wpc;
      uint32_t before = 0;   // carriers in the row words before this round of 64
      for (uint32_t wb = 0; wb < wpc; wb += 64) {
        const uint32_t wi = wb + lane;
        uint64_t rw = wi < wpc ? im.class_rows[(uint64_t)c_r * wpc + wi] : 0ull;
        if (wi == 0) rw &= ~1ull;   // bit 0 of the first word is the reference, never a carrier
        const uint32_t pc = __popcll(rw);
        const uint32_t inc = wave_inclusive_scan(pc);
        uint64_t m = rw;
        if (SUBSET) m = wi < a.s_words ? rw & t.mask[wi] : 0ull;
        while (m) {
          const int b = __builtin_ctzll(m);
          m &= m - 1;
          const uint64_t kc = gt0_r + before + (inc - pc) + __popcll(rw & ((1ull << b) - 1ull));   // carrier record of sample wi * 64 + b
          const uint32_t gt = groups ? (im.gt_groups[kc >> 3] >> (3 * ((kc & 7) >> 1) + 16 * (kc & 1))) & 7u
                                     : (gt32[kc >> 3] >> (4 * (kc & 7))) & 7u;
          burden_add<SUBSET>(t, wi * 64 + (uint32_t)b, gt);
        }
        before += __builtin_amdgcn_readlane(inc, 63);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  __syncthreads();
  // ---- the tile leaves LDS ----
  const uint64_t out0 = q * a.n_cols + t.tile0;
  uint32_t nvars = 0;   // (a workgroup walks at most chunk_rows rows: the sum of a tile stays far below 2^32)
  for (uint32_t i = threadIdx.x; i < t.tn; i += 256) {
    const unsigned long long c0 = t.cell[2 * i], c1 = t.cell[2 * i + 1];
    nvars += (uint32_t)c0;
    if (!SPLIT) a.cells[out0 + i] = uint4{(uint32_t)c0, (uint32_t)(c0 >> 32), (uint32_t)c1, (uint32_t)(c1 >> 32)};
    else {
      unsigned long long* dst = reinterpret_cast<unsigned long long*>(a.cells + out0 + i);
      if (c0) atomicAdd(dst, c0);
      if (c1) atomicAdd(dst + 1, c1);
    }
  }
  nvars = wave_inclusive_scan(nvars);
  if (lane == 63 && nvars) atomicAdd(&s_sum, (unsigned long long)nvars);
  __syncthreads();
  if (threadIdx.x == 0 && s_sum) atomicAdd(a.total, s_sum);
}

// The chunks of the regions of more than chunk_rows rows, as {region, chunk} records (in no particular order: their sums do not
// depend on it).  cap bounds the list; the host sizes it from the rows all regions report, which no list can exceed.
__global__ void __launch_bounds__(256) k_burden_split_plan(const uint64_t* q_nvar, uint64_t Q, uint32_t chunk_rows, uint2* work, uint32_t* n_work, uint32_t cap) {
  const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= Q) return;
  const uint64_t nv = q_nvar[q];
  if (nv <= chunk_rows) return;
  const uint32_t nc = (uint32_t)((nv + chunk_rows - 1) / chunk_rows);
  const uint32_t at = atomicAdd(n_work, nc);
  for (uint32_t c = 0; c < nc; ++c)
    if (at + c < cap) work[at + c] = uint2{(uint32_t)q, c};
}

}  // namespace vsamd
