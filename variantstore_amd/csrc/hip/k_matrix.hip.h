// k_matrix.hip.h -- the genotype matrix of a type-6 plan (vs_query_genotype_matrix): table rows x samples, one byte per call.
// Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_counts.hip.h"

namespace vsamd {

// Cell (i, c) of the matrix is 0 when column c's sample is not a carrier of table row i (or the row was dropped by the duplicate
// rule), else 0x08 | gt with the three genotype bits the index stores per carrier (bit 0 phase, bit 1 gt_1, bit 2 gt_2: what
// k_allele_counts and k_sample_burden sum).  Rows are `pitch` bytes apart (the columns rounded up to 16), padding bytes are 0.
//
// A workgroup owns rows_per_block consecutive table rows times ONE column tile.  The tile lives in LDS as it will lie in memory
// (row after row, a tile row of tb bytes, at most 64 KiB): the workgroup zeroes it, scatters its rows' carriers into it with
// plain LDS byte stores (a sample occurs once in a site's carriers: no two stores meet) and, behind a barrier, streams it out
// with 16-byte stores -- every byte of the matrix, zeros and padding included, is stored exactly once, by one workgroup; there
// is no memset of the matrix and no atomic on it.  The nonzero cells are counted from the same 16-byte words on their way out
// (bit 3 of a byte says it is a carrier) and added to the batch's total once per workgroup.
//
// The rows take their parameters and are decoded over k_carriers.hip.h (row_site, group_load, class_chunk), here by
// the whole workgroup: the listed rows and the rows of explicit-id cohorts as ONE flat list of 8-carrier groups over the block's
// rows (a prefix sum over the group counts, a thread finds its row by bisection), then the classes denser than list_max a row
// per wave, a lane per word of the class row.  There a lane's carriers are consecutive genotype records: the word of eight is
// loaded once and kept while the record index stays inside it.
//
// The column of a sample id: column_of; with a subset the ranks sit in LDS behind the mask.
// All LDS is dynamic and carved on 16-byte bounds: tile | SUBSET: mask, ranks | the block's row parameters.
constexpr uint32_t kMatrixTileCols = 4096;         // default column tile: 16 rows of it are the 64 KiB below
constexpr uint32_t kMatrixTileBytes = 64 << 10;    // the tile in LDS: with the row parameters a second workgroup fits a CU's 160 KiB
constexpr uint32_t kMatrixMaxRows = 256;           // rows of a block: a thread loads one row's parameters
constexpr size_t kMatrixMaskMaxBytes = 40 << 10;   // the subset's bit mask in LDS (its ranks take half as much again)
constexpr size_t kMatrixParamBytes = (kMatrixMaxRows + 8) * 4 + 3 * kMatrixMaxRows * 4 + kMatrixMaxRows * 8 + 32;

struct MatrixArgs {
  const VariantRow* rows;       // the table
  const uint32_t* u_site;       // the site of every table row
  uint64_t A, U;                // rows of the table; the shared ones: the rows behind them are private and may be dropped
  const uint64_t* S;            // SUBSET: the mask and the columns in front of each of its words
  const uint32_t* S_rank;
  uint32_t s_words;
  uint32_t n_cols, pitch;       // columns; bytes from a row to the next (a multiple of 16)
  uint32_t tile_cols, n_tiles;  // a multiple of 16, at most the pitch; tiles per row
  uint32_t rows_per_block;      // 1 .. kMatrixMaxRows, rows_per_block x tile_cols <= kMatrixTileBytes
  uint8_t* cells;               // [A x pitch]
  unsigned long long* total;    // nonzero cells of the matrix
};

struct MatrixTile : ColumnTile { uint8_t* cell; uint32_t tb; };   // tb: bytes of a tile row

// one carrier (sample id, 3 genotype bits) of block row r into its byte, if the tile holds its column
template <bool SUBSET>
__device__ __forceinline__ void matrix_put(const MatrixTile& t, uint32_t r, uint32_t id, uint32_t gt) {
  uint32_t col;
  if (column_of<SUBSET>(t, id, col)) t.cell[r * t.tb + col] = (uint8_t)(0x08u | gt);
}

// group k of block row r (count rcnt, first carrier record gt0, list group src): its up to 8 carriers
template <bool SUBSET>
__device__ __forceinline__ void matrix_group(const DevImage& im, const CarrierForm& f, const MatrixTile& t, uint32_t r, uint32_t k, uint32_t rcnt, uint64_t gt0,
                                             uint32_t src) {
  const uint32_t nsel = group_nsel(rcnt, k);
  const uint64_t g = gt0 + 8ull * k;
  uint32_t id[8];
  const uint32_t w = group_load(im, f, g, src, k, id);
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j)
    if (j < nsel) matrix_put<SUBSET>(t, r, id[j], gt_of_slot(w, j, f.groups));
}

template <bool SUBSET>
__global__ void __launch_bounds__(256) k_genotype_matrix(DevImage im, MatrixArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_mx[];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t blk = blockIdx.x / a.n_tiles;
  const uint32_t tile = blockIdx.x % a.n_tiles;
  const uint64_t row0 = blk * a.rows_per_block;
  if (row0 >= a.A) return;
  const uint32_t nr = a.A - row0 < a.rows_per_block ? (uint32_t)(a.A - row0) : a.rows_per_block;
  // ---- the carve ----
  const uint32_t mask_bytes = SUBSET ? (a.s_words * 8 + 15) & ~15u : 0u, rank_bytes = SUBSET ? (a.s_words * 4 + 15) & ~15u : 0u;
  uint8_t* p = s_mx + (size_t)a.rows_per_block * a.tile_cols;
  uint64_t* s_mask = reinterpret_cast<uint64_t*>(p); p += mask_bytes;
  uint32_t* s_rank = reinterpret_cast<uint32_t*>(p); p += rank_bytes;
  uint64_t* s_gt0 = reinterpret_cast<uint64_t*>(p); p += kMatrixMaxRows * 8;
  uint32_t* s_off = reinterpret_cast<uint32_t*>(p); p += (kMatrixMaxRows + 8) * 4;   // [kMatrixMaxRows + 1]
  uint32_t* s_src = reinterpret_cast<uint32_t*>(p); p += kMatrixMaxRows * 4;
  uint32_t* s_cnt = reinterpret_cast<uint32_t*>(p); p += kMatrixMaxRows * 4;
  uint32_t* s_dense = reinterpret_cast<uint32_t*>(p); p += kMatrixMaxRows * 4;
  uint32_t* s_wsum = reinterpret_cast<uint32_t*>(p);        // [4] group counts of the waves
  uint32_t* s_nd = s_wsum + 4;                              // dense rows of the block
  unsigned long long* s_sum = reinterpret_cast<unsigned long long*>(s_wsum + 6);   // (8-byte aligned: 24 bytes in)
  MatrixTile t;
  t.cell = s_mx;
  t.mask = s_mask;
  t.rank = s_rank;
  t.tile0 = tile * a.tile_cols;
  t.tb = a.pitch - t.tile0 < a.tile_cols ? a.pitch - t.tile0 : a.tile_cols;
  t.tn = a.n_cols - t.tile0 < a.tile_cols ? a.n_cols - t.tile0 : a.tile_cols;
  t.num_samples = im.num_samples;
  const uint32_t n16 = t.tb >> 4;            // 16-byte words of a tile row
  const uint32_t words = nr * n16;           // ... of the tile: at most 4096
  uint4* tile16 = reinterpret_cast<uint4*>(s_mx);
  for (uint32_t i = threadIdx.x; i < words; i += 256) tile16[i] = uint4{0u, 0u, 0u, 0u};
  if (SUBSET)
    for (uint32_t i = threadIdx.x; i < a.s_words; i += 256) {
      s_mask[i] = a.S[i];
      s_rank[i] = a.S_rank[i];
    }
  if (threadIdx.x == 0) { *s_nd = 0; *s_sum = 0; }
  const CarrierForm f = carrier_form(im);
  // ---- the parameters of the block's rows: a row per thread ----
  RowSite rs{0, 0, 0};
  if (threadIdx.x < nr) rs = row_site(im, a.rows, a.u_site, row0 + threadIdx.x, a.U);
  const bool dense = is_dense(im, f, rs.cnt);
  const uint32_t ng = flat_groups(dense, rs.cnt);
  const uint32_t incl = wave_inclusive_scan(ng);
  if (lane == 63) s_wsum[wid] = incl;
  s_src[threadIdx.x] = rs.cls;
  s_cnt[threadIdx.x] = rs.cnt;
  s_gt0[threadIdx.x] = rs.gt0;
  __syncthreads();   // (the tile's zeros, the mask, the waves' sums and s_nd = 0 are in place)
  uint32_t before = 0, total = 0;
#pragma unroll
  for (uint32_t w = 0; w < 4; ++w) {
    const uint32_t s = s_wsum[w];
    if (w < wid) before += s;
    total += s;
  }
  s_off[threadIdx.x] = before + incl - ng;
  if (threadIdx.x == 0) s_off[kMatrixMaxRows] = total;
  if (dense) s_dense[atomicAdd(s_nd, 1u)] = threadIdx.x;
  __syncthreads();
  // ---- the flat pass: one group of 8 carriers per thread and step ----
  for (uint32_t e = threadIdx.x; e < total; e += 256) {
    const uint32_t L = flat_find<kMatrixMaxRows>(s_off, e);
    matrix_group<SUBSET>(im, f, t, L, e - s_off[L], s_cnt[L], s_gt0[L], s_src[L]);
  }
  // ---- denser classes: a row per wave, a lane per word of the class row ----
  const uint32_t nd = *s_nd;
  for (uint32_t k = wid; k < nd; k += 4) {
    const uint32_t r = s_dense[k];
    const uint32_t c_r = s_src[r];
    const uint64_t gt0_r = s_gt0[r];
    uint32_t seen = 0;   // carriers in the row words before this round of 64
    for (uint32_t wb = 0; wb < im.wpc; wb += 64) {
      const uint32_t wi = wb + lane;
      const ClassChunk ch = class_chunk(im, c_r, wi);
      uint64_t m = ch.rw;
      if (SUBSET) {   // the word's columns are rank .. rank + popc(mask): none of them in this tile -> nothing to scatter
        const uint64_t mw = wi < a.s_words ? s_mask[wi] : 0ull;
        m = ch.rw & mw;
        if (m) {
          const uint32_t c0 = s_rank[wi];
          if (c0 >= t.tile0 + t.tn || c0 + __popcll(mw) <= t.tile0) m = 0;
        }
      } else if ((uint64_t)wi * 64 + 62 < t.tile0 || (uint64_t)wi * 64 > (uint64_t)t.tile0 + t.tn) m = 0;   // columns wi * 64 - 1 .. wi * 64 + 62
      uint64_t have = ~0ull;   // the genotype word in hand: its record index / 8
      uint32_t w = 0;
      while (m) {
        const int b = __builtin_ctzll(m);
        m &= m - 1;
        const uint64_t kc = gt0_r + seen + (ch.incl - ch.pc) + __popcll(ch.rw & ((1ull << b) - 1ull));   // carrier record of sample wi * 64 + b
        if ((kc >> 3) != have) {
          have = kc >> 3;
          w = gt_word(im, f, have);
        }
        matrix_put<SUBSET>(t, r, wi * 64 + (uint32_t)b, gt_of_record(w, kc, f.groups));
      }
      seen += __builtin_amdgcn_readlane(ch.incl, 63);
    }
  }
  __syncthreads();
  // ---- the tile leaves LDS: 16 bytes per thread and step, a tile row's words side by side ----
  uint8_t* out = a.cells + row0 * a.pitch + t.tile0;
  const bool whole_rows = t.tb == a.pitch;   // one tile per row: the block's rows are one run of bytes
  uint32_t nz = 0;
  for (uint32_t i = threadIdx.x; i < words; i += 256) {
    const uint4 v = tile16[i];
    nz += __popc(v.x & 0x08080808u) + __popc(v.y & 0x08080808u) + __popc(v.z & 0x08080808u) + __popc(v.w & 0x08080808u);
    size_t at = (size_t)i * 16;
    if (!whole_rows) {
      const uint32_t r = i / n16;
      at = (size_t)r * a.pitch + (size_t)(i - r * n16) * 16;
    }
    *reinterpret_cast<uint4*>(out + at) = v;
  }
  nz = wave_inclusive_scan(nz);
  if (lane == 63 && nz) atomicAdd(s_sum, (unsigned long long)nz);
  __syncthreads();
  if (threadIdx.x == 0 && *s_sum) atomicAdd(a.total, *s_sum);
}

}  // namespace vsamd
