// k_clump.hip.h -- p-value clumping of every region over the hit masks of a pruning batch (vs_query_ld_clump): the greedy in priority
// order, decided in parallel rounds instead of one sequential chain.
// Part of kernels.hip.h (the kernel index is there).
#pragma once
#include "k_prune.hip.h"

namespace vsamd {

// The masks are k_prune_hits' (bit k of hits[i] is the pair (i, i + 1 + k), max_bp applied).  A table row has a 64-bit KEY, the bit
// pattern of its non-negative p-value (kClumpNoKey: no p-value, above every key of a p-value); priority is (key, table row)
// ascending.  No floating-point value takes part.
//
// k_clump_class, a thread per table row: the row's class, region-independent -- kClassLead (a candidate with key <= key(p1)),
// kClassJoin (a candidate with key(p1) < key <= key(p2)), kClassIneligible, kClassDropped.
//
// k_clump_blockers, a thread per verdict slot and mask word: the slot's BLOCKER mask, 2 * words words -- the first `words` are the
// forward bits (bit k: row i + 1 + k), the others the backward bits (bit d: row i - 1 - d, read from bit d of hits[i - 1 - d]).  A
// blocker of row i is a row j that hits it, lies inside the slot's region, is of class kClassLead and outranks i.  (For a row of
// class kClassJoin every hitting lead row outranks it.)  The slot's region is found by bisection over keep_begin.  The thread of
// word 0 also stores the slot's first state -- the final one for an ineligible or dropped row, kClumpLead / kClumpJoin otherwise --
// and owner = none.
//
// k_clump_rounds, one workgroup per region, all regions in one launch, no host wait: every undecided lead row looks at the states
// of its blockers.  One INDEX among them: the row is a MEMBER.  All decided and none INDEX: the row is an INDEX.  Otherwise it waits
// for the next round.  States move from undecided to final only, and a final state is never changed by the loop, so the updates are
// made in place: a stale "undecided" costs a round, never a verdict.  The states are read and written as relaxed atomics of
// workgroup scope, and the barrier between two rounds (__syncthreads_or: it also tells whether a row is still undecided) makes a
// round's stores visible to the next.  The undecided row of the highest priority is decided in every round, so the loop ends
// after at most m rounds for m rows; it is bounded by that as well.  The last pass gives every MEMBER and every row of class
// kClassJoin its owner, the INDEX blocker with the smallest (key, row) -- none: UNCLUMPED --, and sums n_index.
// There is one path for every region size: the states live in HBM (the caches hold them), the masks are read from HBM each round.
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage): DESIGN 5o.
constexpr uint32_t kClumpThreads = 1024;       // k_clump_rounds' workgroup
constexpr uint32_t kClumpBuildThreads = 256;   // k_clump_class, k_clump_blockers
constexpr uint8_t kClumpMember = 0, kClumpIndex = 1, kClumpIneligible = 2, kClumpDropped = 3, kClumpUnclumped = 4;   // VS_CLUMP_*
constexpr uint8_t kClumpLead = 0xFF, kClumpJoin = 0xFE;   // undecided: never left in the answer
constexpr uint8_t kClassLead = 0, kClassJoin = 1, kClassIneligible = 2, kClassDropped = 3;
constexpr uint64_t kClumpNoKey = ~0ull;
constexpr uint32_t kClumpNoOwner = 0xFFFFFFFFu;

struct ClumpArgs {
  uint64_t Q, A, states;
  const uint64_t* row_begin;    // per region, in the caller's order
  const uint64_t* row_count;
  const uint64_t* keep_begin;   // [Q + 1]
  const VariantRow* rows;       // the table: the duplicate rule's flag
  const uint4* counts;          // {carriers, alt_alleles, hom_alt, phased} per table row
  const uint64_t* keys;         // [A]
  const uint32_t* hits;         // [A x words]
  uint8_t* cls;                 // [A]
  uint32_t* blockers;           // [states x 2 words]
  uint32_t words, window, n_cols;
  uint64_t key1, key2;          // of p1 and p2
  uint8_t* state;               // [states]
  uint32_t* owner;              // [states]
  uint64_t* n_index;            // [Q]
  uint64_t* rounds;             // [Q], a diagnostic
};

__global__ void __launch_bounds__(kClumpBuildThreads) k_clump_class(ClumpArgs a) {
  for (uint64_t i = (uint64_t)blockIdx.x * kClumpBuildThreads + threadIdx.x; i < a.A; i += (uint64_t)gridDim.x * kClumpBuildThreads) {
    uint8_t c = kClassDropped;
    if (!(a.rows[i].count_flags & kRowDropped)) {
      int64_t sx, v;
      ld_moments(a.counts[i], (int64_t)a.n_cols, sx, v);
      const uint64_t key = a.keys[i];
      c = v > 0 && key <= a.key2 ? (key <= a.key1 ? kClassLead : kClassJoin) : kClassIneligible;
    }
    a.cls[i] = c;
  }
}

__global__ void __launch_bounds__(kClumpBuildThreads) k_clump_blockers(ClumpArgs a) {
  const uint32_t words = a.words, per_slot = 2 * words;
  const uint64_t t = (uint64_t)blockIdx.x * kClumpBuildThreads + threadIdx.x;
  const uint64_t slot = t / per_slot;
  const uint32_t w2 = (uint32_t)(t - slot * per_slot);
  if (slot >= a.states) return;
  uint64_t lo = 0, hi = a.Q - 1;   // the last region whose keep_begin is at most the slot: it is not empty
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (a.keep_begin[mid] <= slot) lo = mid;
    else hi = mid - 1;
  }
  const uint64_t r0 = a.row_begin[lo], r1 = r0 + a.row_count[lo], i = r0 + (slot - a.keep_begin[lo]);
  const uint8_t ci = a.cls[i];
  uint32_t mask = 0u;
  if (ci <= kClassJoin) {
    const uint64_t key = a.keys[i];
    if (w2 < words) {   // forward: row j = i + 1 + k outranks i when its key is smaller (a tie goes to i, the earlier row)
      for (uint32_t word = a.hits[i * words + w2]; word; word &= word - 1) {
        const uint32_t b = (uint32_t)__builtin_ctz(word);
        const uint64_t j = i + 1 + 32 * w2 + b;
        if (j >= r1) break;
        if (a.cls[j] == kClassLead && a.keys[j] < key) mask |= 1u << b;
      }
    } else {            // backward: row j = i - 1 - d outranks i when its key is not larger
      const uint32_t w = w2 - words;
      for (uint32_t b = 0; b < 32; ++b) {
        const uint64_t d = 32ull * w + b;
        if (d >= a.window || i < r0 + 1 + d) break;
        const uint64_t j = i - 1 - d;
        if (((a.hits[j * words + w] >> b) & 1u) && a.cls[j] == kClassLead && a.keys[j] <= key) mask |= 1u << b;
      }
    }
  }
  a.blockers[slot * per_slot + w2] = mask;
  if (w2 == 0) {
    a.state[slot] = ci == kClassLead ? kClumpLead : ci == kClassJoin ? kClumpJoin : ci == kClassIneligible ? kClumpIneligible : kClumpDropped;
    a.owner[slot] = kClumpNoOwner;
  }
}

__device__ __forceinline__ uint8_t clump_state(const uint8_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void clump_set(uint8_t* p, uint8_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__global__ void __launch_bounds__(kClumpThreads) k_clump_rounds(ClumpArgs a) {
  __shared__ uint32_t s_index;
  const uint64_t q = blockIdx.x;
  const uint64_t m = a.row_count[q], r0 = a.row_begin[q], o = a.keep_begin[q];
  if (m == 0) {
    if (threadIdx.x == 0) { a.n_index[q] = 0; a.rounds[q] = 0; }
    return;
  }
  const uint32_t words = a.words;
  uint8_t* const st = a.state + o;
  const uint32_t* const bl = a.blockers + o * 2 * words;
  if (threadIdx.x == 0) s_index = 0u;
  uint64_t rounds = 0;
  for (;;) {
    int pending = 0;
    for (uint64_t x = threadIdx.x; x < m; x += kClumpThreads) {
      if (clump_state(st + x) != kClumpLead) continue;
      const uint32_t* const row = bl + x * 2 * words;
      bool wait = false, member = false;
      for (uint32_t w = 0; w < 2 * words && !member; ++w)
        for (uint32_t word = row[w]; word; word &= word - 1) {
          const uint64_t d = 1 + 32ull * (w < words ? w : w - words) + (uint32_t)__builtin_ctz(word);
          const uint8_t s = clump_state(st + (w < words ? x + d : x - d));   // (a blocker lies inside the region)
          if (s == kClumpIndex) { member = true; break; }
          wait |= s == kClumpLead;
        }
      if (member) clump_set(st + x, kClumpMember);
      else if (!wait) clump_set(st + x, kClumpIndex);
      else pending = 1;
    }
    ++rounds;
    if (!__syncthreads_or(pending) || rounds > m) break;
  }
  // ---- owners: the INDEX blocker of the highest priority; a joining row without one is unclumped ----
  uint32_t n_index = 0;
  for (uint64_t x = threadIdx.x; x < m; x += kClumpThreads) {
    const uint8_t s = clump_state(st + x);
    if (s == kClumpIndex) {
      a.owner[o + x] = (uint32_t)x;
      ++n_index;
      continue;
    }
    if (s != kClumpMember && s != kClumpJoin) continue;
    const uint32_t* const row = bl + x * 2 * words;
    uint64_t best_key = 0, best = m;
    for (uint32_t w = 0; w < 2 * words; ++w)
      for (uint32_t word = row[w]; word; word &= word - 1) {
        const uint64_t d = 1 + 32ull * (w < words ? w : w - words) + (uint32_t)__builtin_ctz(word);
        const uint64_t y = w < words ? x + d : x - d;
        if (clump_state(st + y) != kClumpIndex) continue;
        const uint64_t key = a.keys[r0 + y];
        if (best == m || key < best_key || (key == best_key && y < best)) { best_key = key; best = y; }
      }
    if (best != m) a.owner[o + x] = (uint32_t)best;
    if (s == kClumpJoin) clump_set(st + x, best != m ? kClumpMember : kClumpUnclumped);
  }
  if (n_index) atomicAdd(&s_index, n_index);
  __syncthreads();
  if (threadIdx.x == 0) { a.n_index[q] = s_index; a.rounds[q] = rounds; }
}

}  // namespace vsamd
