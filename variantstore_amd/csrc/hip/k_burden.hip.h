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
// memset.  Per 64 rows a wave works over k_carriers.hip.h: the listed rows and the rows of explicit-id cohorts as a FLAT list of
// 8-carrier groups (group_load), then the classes denser than list_max a row at a time, a lane per word of the class
// row (class_chunk: the carrier index of a bit is the prefix popcount).
//
// The column of a sample id: column_of (k_carriers.hip.h); with a subset the ranks (s_rank) sit in LDS behind the mask.
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

struct BurdenTile : ColumnTile { unsigned long long* cell; };

// one carrier (sample id, 3 genotype bits) into its cell, if the tile holds its column
template <bool SUBSET>
__device__ __forceinline__ void burden_add(const BurdenTile& t, uint32_t id, uint32_t gt) {
  uint32_t col;
  if (!column_of<SUBSET>(t, id, col)) return;
  const uint32_t g1 = (gt >> 1) & 1u, g2 = (gt >> 2) & 1u, ph = gt & 1u;
  atomicAdd(&t.cell[2 * col], 1ull | ((unsigned long long)(g1 + g2) << 32));
  if ((g1 & g2) | ph) atomicAdd(&t.cell[2 * col + 1], (unsigned long long)(g1 & g2) | ((unsigned long long)ph << 32));
}

// group k of a row (count rcnt, first carrier record gt0, list group src): its up to 8 carriers
template <bool SUBSET>
__device__ __forceinline__ void burden_group(const DevImage& im, const CarrierForm& f, const BurdenTile& t, uint32_t k, uint32_t rcnt, uint64_t gt0, uint32_t src) {
  const uint32_t nsel = group_nsel(rcnt, k);
  const uint64_t g = gt0 + 8ull * k;
  uint32_t id[8];
  const uint32_t w = group_load(im, f, g, src, k, id);
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j)
    if (j < nsel) burden_add<SUBSET>(t, id[j], gt_of_slot(w, j, f.groups));
}

template <bool SUBSET, bool WINDOW, bool SPLIT>
__global__ void __launch_bounds__(256) k_sample_burden(DevImage im, BurdenArgs a) {
  extern __shared__ unsigned long long s_dyn[];   // tile_cols x 2 cell words | SUBSET: s_words mask words | s_words ranks
  __shared__ FlatRows s_rows;
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
  const CarrierForm f = carrier_form(im);
  const uint32_t* off = s_rows.off[wid];
  for (uint64_t base = r_begin; base < r_end; base += 256) {
    // ---- the parameters of this wave's 64 rows ----
    const uint64_t row = base + 4 * lane + wid;
    RowSite rs{0, 0, 0};
    if (row < r_end) {
      rs = row_site(im, a.rows, a.u_site, row, a.U);
      if (WINDOW) {
        const uint32_t ac = a.ac[row].y;
        if (ac < a.min_ac || ac > a.max_ac) rs.cnt = 0;
      }
    }
    const bool dense = is_dense(im, f, rs.cnt);
    const uint32_t total = flat_publish(s_rows, wid, lane, dense, rs);
    // ---- the flat pass: one group of 8 carriers per lane and step ----
    for (uint32_t e = lane; e < total; e += 64) {
      const uint32_t L = flat_find<64>(off, e);
      burden_group<SUBSET>(im, f, t, e - off[L], s_rows.cnt[wid][L], s_rows.gt0[wid][L], s_rows.src[wid][L]);
    }
    // ---- denser classes: a row at a time, a lane per word of the class row ----
    uint64_t dmask = __ballot(dense);
    while (dmask) {
      const int r = __builtin_ctzll(dmask);
      dmask &= dmask - 1;
      const uint32_t c_r = __builtin_amdgcn_readlane(rs.cls, r);
      const uint64_t gt0_r = wave_bcast64(rs.gt0, r);
      uint32_t before = 0;   // carriers in the row words before this round of 64
      for (uint32_t wb = 0; wb < im.wpc; wb += 64) {
        const uint32_t wi = wb + lane;
        const ClassChunk ch = class_chunk(im, c_r, wi);
        uint64_t m = ch.rw;
        if (SUBSET) m = wi < a.s_words ? ch.rw & t.mask[wi] : 0ull;
        while (m) {
          const int b = __builtin_ctzll(m);
          m &= m - 1;
          const uint64_t kc = gt0_r + before + (ch.incl - ch.pc) + __popcll(ch.rw & ((1ull << b) - 1ull));   // carrier record of sample wi * 64 + b
          burden_add<SUBSET>(t, wi * 64 + (uint32_t)b, gt_of_record(gt_word(im, f, kc >> 3), kc, f.groups));
        }
        before += __builtin_amdgcn_readlane(ch.incl, 63);
      }
    }
    wave_lds_sync();   // (the rows are read before the next 256 overwrite them)
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
