// k_roh.hip.h -- runs of homozygosity per region and column over the genotype matrix of a type-6 plan (vs_query_roh): the first
// consumer that walks a COLUMN of the matrix in row order.  Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_matrix.hip.h"

namespace vsamd {

// The definition is the C header's (vs_query_roh): a table row is a SITE when the duplicate rule kept it, 0 < ac < 2 n over the
// columns and min_ac <= ac <= max_ac; at a site a column is het (dosage popcount(cell & 6) == 1) or hom; a run opens at a hom site,
// absorbs up to max_het hets that a later hom site confirms, and is closed by the gap rule, by a het beyond max_het or by the
// region's end.
//
// k_roh_sites: a thread per table row writes {pos, site ? 1 : 0} (8 bytes) from rows[] and counts[] -- the walk then reads 8 bytes
//   a row instead of 48, and it reads them once per wave and column tile.
//
// k_roh_walk<EMIT>: a workgroup of four waves owns (one region) x (a tile of 256 columns); blockIdx.x = region * n_tiles + tile.
//   It goes through the region's rows in blocks of 64.
//   Site mask.  Lane l of EVERY wave loads the 8 bytes of block row l (the next block's while this one is walked); one ballot turns
//   the flags into a 64-bit mask in scalar registers, the same in all four waves.  A block without a site is skipped before anything
//   is staged -- a workgroup-uniform decision --, and inside a block the walk visits the set bits only: a row that is no site costs
//   nothing.  A site's position comes out of the lane that loaded it with v_readlane: positions never touch LDS.
//   Staging.  The block's 64 x 256 cells go from the matrix to LDS as they lie (a tile row of 256 bytes): thread t loads four 16-byte
//   words -- 16 threads a row, 256 contiguous bytes --, holds them in registers while the block before is walked, and stores them
//   with 16-byte LDS writes into the other of two buffers.  The buffer alternates per STAGED block, so one barrier a staged block
//   orders everything: whoever writes staged block k has passed the barrier of k - 1, which nobody passes before walking k - 2.
//   Words past the region's last row or past `pitch` are staged as zeros (never read from memory).
//   Walk.  Lane t of wave w owns column tile * 256 + 64 w + t and reads ITS byte of a site row: 64 lanes, 64 consecutive bytes, no
//   bank conflict.  The machine's state (open, first / last row and position, n_sites, n_het, pend) and the cell's summary stay in
//   registers across blocks; the loop bounds (the mask's bits) are wave-uniform; the transition is written with selects; the one
//   branch is the close (gap rule: uniform; het overflow: per lane), taken by the wave when any lane closes.
//   Pass 1 (EMIT = false) stores each cell's 32-byte summary with two 16-byte stores -- a lane owns its cell, no atomic -- and, when
//   segments are wanted, n_segments again into a dense uint32 array for the engine's exclusive scan.  Tile 0's thread 0 stores
//   n_sites[region], the sum of the masks' popcounts.  Pass 2 (EMIT = true) repeats the walk and stores accepted segment k of a cell
//   at seg_begin[cell] + k, 32 bytes, two 16-byte stores.  Lanes at or past n_cols store nothing.
//   LDS: 2 x 16 KiB static: five workgroups fit a CU's 160 KiB, and that, not the registers, sets the occupancy.
//   Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage):
//     k_roh_walk<false>: 54 VGPRs, 56 SGPRs, no AGPRs, scratch 0, no spills, LDS 32,768 bytes, occupancy 5 waves a SIMD
//     k_roh_walk<true>:  54 VGPRs, 54 SGPRs, no AGPRs, scratch 0, no spills, LDS 32,768 bytes, occupancy 5 waves a SIMD
//     k_roh_sites:       10 VGPRs, 20 SGPRs, no AGPRs, scratch 0, no spills, no LDS, occupancy 8 waves a SIMD
constexpr uint32_t kRohBlockRows = 64;    // rows of a block: a lane of the mask each
constexpr uint32_t kRohTileCols = 256;    // columns of a workgroup: a thread each
constexpr uint32_t kRohMaxHet = 255;      // vs_roh_params::max_het at most

struct RohSummary {   // vs_roh_summary
  uint32_t n_segments, seg_sites;
  uint64_t total_bp;
  uint32_t longest_bp, longest_sites, seg_hets, n_het;
};
static_assert(sizeof(RohSummary) == 32, "record layout of the ABI");

struct RohArgs {
  const uint8_t* cells;          // the temporary genotype matrix, rows `pitch` bytes apart
  const uint2* sites;            // {pos, site} per table row (k_roh_sites)
  const uint64_t* row_begin;     // per region, in the caller's order
  const uint64_t* row_count;
  uint64_t Q;
  uint32_t pitch, n_cols, n_tiles;
  uint32_t min_sites, min_bp, max_gap, max_het;
  RohSummary* summary;           // [Q x n_cols]
  uint32_t* n_sites;             // [Q]
  uint32_t* seg_count;           // [Q x n_cols] n_segments again, dense, for the scan; NULL: no segments wanted
  const uint64_t* seg_begin;     // EMIT: [Q x n_cols + 1]
  uint4* segments;               // EMIT: two words a segment
};

struct RohSiteArgs {
  const VariantRow* rows;
  const uint4* counts;           // {carriers, alt_alleles, hom_alt, phased} per table row over the columns
  uint64_t A;
  uint32_t n_cols, min_ac, max_ac;
  uint2* sites;
};

__global__ void __launch_bounds__(256) k_roh_sites(RohSiteArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.A) return;
  const uint4 r0 = reinterpret_cast<const uint4*>(a.rows + i)[0], r1 = reinterpret_cast<const uint4*>(a.rows + i)[1];   // pos .. alt_off | alt_len, count_flags, ..
  const uint32_t ac = a.counts[i].y;
  const bool site = !(r1.y & kRowDropped) && ac > 0 && (uint64_t)ac < 2ull * a.n_cols && ac >= a.min_ac && ac <= a.max_ac;
  a.sites[i] = make_uint2(r0.x, site ? 1u : 0u);
}

template <bool EMIT>
__global__ void __launch_bounds__(256) k_roh_walk(RohArgs a) {
  __shared__ uint4 s_tile[2][kRohBlockRows * kRohTileCols / 16];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint64_t q = blockIdx.x / a.n_tiles;
  const uint32_t tile = blockIdx.x % a.n_tiles;
  const uint32_t col0 = tile * kRohTileCols, col = col0 + tid;
  const uint64_t m = a.row_count[q], r0 = a.row_begin[q];
  const uint64_t n_blocks = (m + kRohBlockRows - 1) / kRohBlockRows;
  const uint64_t cell = q * a.n_cols + col;

  // the machine and the summary of this lane's cell
  bool open = false;
  uint32_t first_row = 0, first_pos = 0, last_row = 0, last_pos = 0, run_sites = 0, run_het = 0, pend = 0;
  uint32_t n_seg = 0, seg_sites = 0, longest_bp = 0, longest_sites = 0, seg_hets = 0, n_het = 0;
  uint64_t total_bp = 0;
  uint64_t seg_at = 0;
  if (EMIT) seg_at = col < a.n_cols ? a.seg_begin[cell] : 0;
  auto close = [&](bool mine) {   // the lanes with `mine` close their run
    if (mine) {
      const uint64_t bp = (uint64_t)(last_pos > first_pos ? last_pos - first_pos : 0u) + 1u;
      if (run_sites >= a.min_sites && bp >= a.min_bp) {
        const uint32_t bp32 = bp > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)bp;
        if (EMIT) {
          if (col < a.n_cols) {
            uint4* dst = a.segments + 2 * (seg_at + n_seg);
            dst[0] = make_uint4((uint32_t)q, col, first_pos, last_pos);
            dst[1] = make_uint4(first_row, last_row, run_sites, run_het);
          }
        }
        n_seg += 1; seg_sites += run_sites; total_bp += bp; seg_hets += run_het;
        if (bp32 > longest_bp) { longest_bp = bp32; longest_sites = run_sites; }
      }
      open = false;
    }
  };

  // the lane's row of a block: {pos, site}; zeros past the region's end
  auto load_meta = [&](uint64_t b) {
    const uint64_t local = b * kRohBlockRows + lane;
    return b < n_blocks && local < m ? a.sites[r0 + local] : make_uint2(0u, 0u);
  };
  // the thread's four 16-byte words of a block's 64 x 256 cells; zeros past the region's end and past the pitch
  auto load_cells = [&](uint64_t b, uint4 (&w)[4]) {
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      const uint32_t idx = tid + 256 * i, row = idx >> 4, at = col0 + ((idx & 15u) << 4);
      const uint64_t local = b * kRohBlockRows + row;
      w[i] = make_uint4(0, 0, 0, 0);
      if (local < m && at < a.pitch) w[i] = *reinterpret_cast<const uint4*>(a.cells + (r0 + local) * a.pitch + at);
    }
  };

  uint32_t prev_pos = 0, sites_seen = 0;   // wave-uniform: the site before, and how many there were (n_sites; 0: no site before)
  uint32_t staged = 0;                     // staged blocks so far: the buffer alternates with it
  uint2 mt = load_meta(0);
  uint64_t mask = __ballot(mt.y != 0u);
  uint4 w[4];
  if (mask) load_cells(0, w);
  for (uint64_t b = 0; b < n_blocks; ++b) {
    const uint32_t buf = staged & 1u;
    if (mask) {
#pragma unroll
      for (uint32_t i = 0; i < 4; ++i) s_tile[buf][tid + 256 * i] = w[i];
    }
    const uint2 mtn = load_meta(b + 1);   // the next block, in front of the walk over this one
    const uint64_t maskn = __ballot(mtn.y != 0u);
    if (maskn) load_cells(b + 1, w);
    if (mask) {
      __syncthreads();
      staged += 1;
      const uint8_t* tile_bytes = reinterpret_cast<const uint8_t*>(s_tile[buf]) + tid;
      const uint32_t row_base = (uint32_t)(b * kRohBlockRows);
      for (uint64_t left = mask; left; left &= left - 1) {
        const uint32_t r = (uint32_t)__builtin_ctzll(left);
        const uint32_t pos = (uint32_t)__builtin_amdgcn_readlane((int)mt.x, (int)r);
        const uint32_t cellv = tile_bytes[r * kRohTileCols];
        const uint32_t dosage = (cellv >> 1 & 1u) + (cellv >> 2 & 1u);
        const bool het = dosage == 1u;
        const bool gap = a.max_gap != 0u && sites_seen != 0u && pos > prev_pos && pos - prev_pos > a.max_gap;   // (uniform)
        const bool closing = open && (gap || (het && run_het + pend >= a.max_het));
        if (__ballot(closing)) close(closing);
        const bool hom = !het;
        const uint32_t row = row_base + r;
        // hom: open a run or extend it over the pending hets; het on an open run (it has room, or the run was closed): pend
        const bool start = hom && !open;
        first_row = start ? row : first_row;
        first_pos = start ? pos : first_pos;
        run_sites = hom ? (open ? run_sites + pend + 1u : 1u) : run_sites;
        run_het = hom ? (open ? run_het + pend : 0u) : run_het;
        last_row = hom ? row : last_row;
        last_pos = hom ? pos : last_pos;
        pend = hom ? 0u : pend + (open ? 1u : 0u);
        open = open || hom;
        n_het += het ? 1u : 0u;
        prev_pos = pos;
        sites_seen += 1;
      }
    }
    mt = mtn; mask = maskn;
  }
  close(open);   // the region's end
  if (!EMIT) {
    if (col < a.n_cols) {
      uint4* dst = reinterpret_cast<uint4*>(a.summary + cell);
      dst[0] = make_uint4(n_seg, seg_sites, (uint32_t)total_bp, (uint32_t)(total_bp >> 32));
      dst[1] = make_uint4(longest_bp, longest_sites, seg_hets, n_het);
      if (a.seg_count) a.seg_count[cell] = n_seg;
    }
    if (tile == 0 && tid == 0) a.n_sites[q] = sites_seen;
  }
}

}  // namespace vsamd
