// k_carriers.hip.h -- how a column kernel (k_counts, k_group_counts, k_assoc, k_scores, k_burden, k_matrix) reads the carriers of the rows of a type-6
// table: the one place, next to the expansion kernels, that knows how a carrier is stored.  No kernels here.
// Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_rows.hip.h"

namespace vsamd {

// ---- the three storage forms of an image ----
//   explicit ids            ids in car_sid, genotypes as nibbles of gt_nibbles; the pool is NOT padded: a group of 8 is an unaligned
//                           window of both, and the entries beyond a row's run belong to the next one
//   class rows, wpc <= 63   one word of gt_groups per 8 carrier records, genotype j at bit 3 (j / 2) + 16 (j & 1); the ids of a listed
//                           class (at most list_max carriers) as 16-bit entries of the class's decoded list
//   class rows of 64 words  eight nibbles of gt_nibbles per group, the decoded lists hold 32-bit ids
// Class-row pools are padded with zeros (a vertex's records start on a multiple of 8), and so are the lists.
struct CarrierForm { bool groups, explicit_ids; const uint32_t* __restrict__ gt32; };
__device__ __forceinline__ CarrierForm carrier_form(const DevImage& im) {
  return CarrierForm{im.use_bv && im.wpc <= 63, !im.use_bv, reinterpret_cast<const uint32_t*>(im.gt_nibbles)};
}

// the bit of genotype j (0 .. 7) in a word of eight; the three bits there: bit 0 phase, bit 1 gt_1, bit 2 gt_2
__device__ __forceinline__ uint32_t gt_shift(uint32_t j, bool groups) { return groups ? 3 * (j >> 1) + 16 * (j & 1) : 4 * j; }
__device__ __forceinline__ uint32_t gt_of_slot(uint32_t w, uint32_t j, bool groups) { return (w >> gt_shift(j, groups)) & 7u; }
// ... of carrier record kc, given the word that holds it (gt_word(kc >> 3), or a copy of it)
__device__ __forceinline__ uint32_t gt_of_record(uint32_t word, uint64_t kc, bool groups) { return gt_of_slot(word, (uint32_t)kc & 7u, groups); }
// word i of the genotype pool: carrier records 8 i .. 8 i + 7
__device__ __forceinline__ uint32_t gt_word(const DevImage& im, const CarrierForm& f, uint64_t i) { return f.groups ? im.gt_groups[i] : f.gt32[i]; }

// ---- one group of 8 carriers: group k of a row whose first carrier record is gt0; g = gt0 + 8 k is the group's first record ----
__device__ __forceinline__ uint32_t group_nsel(uint32_t rcnt, uint32_t k) {   // entries of the group that belong to the row (count rcnt)
  const uint32_t rem = rcnt - 8 * k;
  return rem < 8 ? rem : 8u;
}
// the group's genotype word alone: eight fields, gt_shift apart
__device__ __forceinline__ uint32_t window_word(const CarrierForm& f, uint64_t g) {   // unpadded pool: a window of the nibble stream
  uint2 nw;
  __builtin_memcpy(&nw, f.gt32 + (g >> 3), 8);
  return __builtin_amdgcn_alignbit(nw.y, nw.x, ((uint32_t)g & 7u) * 4);
}
__device__ __forceinline__ uint32_t group_word(const DevImage& im, const CarrierForm& f, uint64_t g) {
  return f.explicit_ids ? window_word(f, g) : gt_word(im, f, g >> 3);   // (g is a multiple of 8 in class-row pools)
}
// the word and the group's 8 sample ids (src: the row's list group); entries beyond group_nsel are the next run's or a list's padding.
// ONE branch per storage form with the word's and the ids' loads side by side: as two functions, each with its own branch, the loads
// of a group wait for one another (measured: 4 to 8 % of k_genotype_matrix).
__device__ __forceinline__ uint32_t group_load(const DevImage& im, const CarrierForm& f, uint64_t g, uint32_t src, uint32_t k, uint32_t (&id)[8]) {
  uint4 ia, ib;
  uint32_t w;
  if (f.explicit_ids) {
    w = window_word(f, g);
    __builtin_memcpy(&ia, im.car_sid + g, 16);
    __builtin_memcpy(&ib, im.car_sid + g + 4, 16);
  } else if (f.groups) {
    w = gt_word(im, f, g >> 3);
    const uint4 iw = reinterpret_cast<const uint4*>(im.cls_list16)[(uint64_t)src + k];
    ia = uint4{iw.x & 0xFFFFu, iw.x >> 16, iw.y & 0xFFFFu, iw.y >> 16};
    ib = uint4{iw.z & 0xFFFFu, iw.z >> 16, iw.w & 0xFFFFu, iw.w >> 16};
  } else {
    w = gt_word(im, f, g >> 3);
    const uint4* lg = reinterpret_cast<const uint4*>(im.cls_list_ids) + 2 * ((uint64_t)src + k);
    ia = lg[0]; ib = lg[1];
  }
  id[0] = ia.x; id[1] = ia.y; id[2] = ia.z; id[3] = ia.w; id[4] = ib.x; id[5] = ib.y; id[6] = ib.z; id[7] = ib.w;
  return w;
}

// ---- a table row's site parameters ----
// u_site: the site of every row of the table (k_share_rows2 for the shared rows, k_count_slow_sites for the private rows of the
// regions under the duplicate rule, which may have dropped some: those rows' own counts say so, and such a row has no carriers).
struct RowSite { uint32_t cnt, cls; uint64_t gt0; };   // carriers; class (or list group); first carrier record
__device__ __forceinline__ RowSite row_site(const DevImage& im, const VariantRow* __restrict__ rows, const uint32_t* __restrict__ u_site, uint64_t row, uint64_t U) {
  const uint32_t g = u_site[row];
  RowSite s{im.s_ncar[g], im.s_class[g], im.s_gt0[g]};
  if (row >= U && (rows[row].count_flags & kRowDropped)) s.cnt = 0;   // dropped by the duplicate rule: reports nothing
  return s;
}
// a class denser than list_max has no id list: its carriers are the bits of its class row (class_chunk below), not groups of a flat list
__device__ __forceinline__ bool is_dense(const DevImage& im, const CarrierForm& f, uint32_t cnt) { return !f.explicit_ids && cnt > im.list_max; }
__device__ __forceinline__ uint32_t flat_groups(bool dense, uint32_t cnt) { return dense ? 0u : (cnt + 7) / 8; }

// ---- the flat list of 8-carrier groups of 64 (a wave's) or 256 (a workgroup's) rows ----
// LDS written by one wave and read by the same wave's other lanes
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// the row of flat entry e: the last of N rows whose offset is at most e (off: exclusive prefix of the rows' group counts)
template <uint32_t N>
__device__ __forceinline__ uint32_t flat_find(const uint32_t* off, uint32_t e) {
  uint32_t L = 0;
#pragma unroll
  for (uint32_t step = N / 2; step; step >>= 1)
    if (off[L + step] <= e) L += step;
  return L;
}
// the rows of a workgroup's four waves in LDS, wave w's 64 at [w]: 5136 bytes
struct FlatRows {
  uint64_t gt0[4][64];
  uint32_t off[4][64 + 1], src[4][64], cnt[4][64];
};
// lane `lane` of wave `wid` publishes its row (dense: no groups in the list); returns the groups of the wave's rows
__device__ __forceinline__ uint32_t flat_publish(FlatRows& fr, uint32_t wid, uint32_t lane, bool dense, const RowSite& s) {
  const uint32_t ng = flat_groups(dense, s.cnt);
  const uint32_t incl = wave_inclusive_scan(ng);
  const uint32_t total = __builtin_amdgcn_readlane(incl, 63);
  fr.off[wid][lane] = incl - ng;
  if (lane == 0) fr.off[wid][64] = total;
  fr.src[wid][lane] = s.cls;
  fr.cnt[wid][lane] = s.cnt;
  fr.gt0[wid][lane] = s.gt0;
  wave_lds_sync();
  return total;
}

// ---- a dense class row: a lane per 64-bit word, 64 words a chunk; a sample's id is its bit position, its carrier index the number
// of bits below it in the row ----
__device__ __forceinline__ uint64_t class_row_word(const DevImage& im, uint32_t c, uint32_t wi) {
  uint64_t rw = wi < im.wpc ? im.class_rows[(uint64_t)c * im.wpc + wi] : 0ull;
  if (wi == 0) rw &= ~1ull;   // bit 0 of the first word is the reference, never a carrier
  return rw;
}
struct ClassChunk { uint64_t rw; uint32_t pc, incl; };   // the lane's word, its carriers, the carriers of the chunk's lanes up to and with it
__device__ __forceinline__ ClassChunk class_chunk(const DevImage& im, uint32_t c, uint32_t wi) {
  const uint64_t rw = class_row_word(im, c, wi);
  const uint32_t pc = __popcll(rw);
  return ClassChunk{rw, pc, wave_inclusive_scan(pc)};
}

// ---- sample id -> column of a column tile ----
// The column of sample id: id - 1 without a subset; with one, the rank of id in S -- per-word prefix popcounts of the mask (rank).
struct ColumnTile { const uint64_t* mask; const uint32_t* rank; uint32_t tile0, tn, num_samples; };   // columns tile0 .. tile0 + tn
template <bool SUBSET>
__device__ __forceinline__ bool column_of(const ColumnTile& t, uint32_t id, uint32_t& col) {   // col: relative to the tile; false: not in it
  if (id - 1u >= t.num_samples - 1u) return false;   // "ref" (id 0) and the padding of a list
  col = id - 1u;
  if (SUBSET) {
    const uint64_t mw = t.mask[id >> 6], bit = 1ull << (id & 63);
    if (!(mw & bit)) return false;
    col = t.rank[id >> 6] + __popcll(mw & (bit - 1ull));
  }
  col -= t.tile0;
  return col < t.tn;
}

}  // namespace vsamd
