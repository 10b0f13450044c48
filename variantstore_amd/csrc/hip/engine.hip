// engine.hip -- host side of the C ABI (include/variantstore_hip.h).
//
// Owns the decoded index (HostGraph), its flattened image (HostImage), the HBM
// copy (DevImage), one HIP stream per handle and a small device-buffer pool so
// that steady-state batches do no hipMalloc.  Mirrors the reference's seam
// between query_main and query.h (reference src/commands.cc:114-215).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../../include/variantstore_hip.h"
#include "../host/host_graph.hpp"
#include "../host/builder.hpp"
#include "../host/vcf.hpp"
#include "../host/synth.hpp"
#include "../host/device_image.hpp"
#include "../host/index_files.hpp"
#include "../host/dot_graph.hpp"
#include "kernels.hip.h"

using namespace vsamd;

static thread_local std::string g_last_error;
static int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}
#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return fail(VS_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)
#define VS_TRY(expr)          \
  do {                        \
    int rc_ = (expr);         \
    if (rc_ != VS_OK) return rc_; \
  } while (0)

struct DevBuf { void* p; size_t cap; };

// Switches of one handle.  The environment is read ONCE, when the handle is opened (read_env_opts); afterwards only
// vs_index_set_option changes them -- no getenv on any query path.
struct EngineOpts {
  // ---- the production switches (vs_index_set_option; eight keys) ----
  int server = 1;               // "latency_server": 0 never use the resident server, 1 start it for a back-to-back streak of small queries
                                // only (default), 2 start it with the first small query
  unsigned srv_blocks = 16;     // "server_blocks": grid of the resident server (>= 1)
  bool share_lists = true;      // "share_lists": type-6 batches of more than 64 regions hold one row and one carrier list per covered site, shared
                                // by the regions that report it; type-4 / 5 batches one list per reported vertex
  bool resident_lists = false;  // "resident_lists": carrier lists expanded once into an arena that stays with the index (build_resident_lists)
  bool async_submit = true;     // "async_submit": a type-6 batch of more than 64 regions returns once it is ENQUEUED (its sizes are known -- or speculated: t6_speculate --, its
                                // buffers allocated, its last kernel launched); everything that reads the result is ordered behind it on the
                                // handle's stream, so callers see no difference except that the host is free while the GPU works
  bool async_fill = false;      // "async_fill": the carrier expansion of a type-6 batch runs on a second stream and the call returns while it
                                // is in flight (every accessor of the result waits for it): the next batch's plan and rows run beside it
  int t4_walk = 2;              // "t4_walk": the walk of query type 4 -- 2 cooperative (8 lanes per region, episodes in parallel; default),
                                // 1 one lane per region jumping over uneventful ref-path runs, 0 literal (every vertex of the sample's path)
  bool t6_speculate = true;     // "t6_speculate": a type-6 batch that returns when it is enqueued does not wait for its plan's totals either -- table and
                                // arena are sized from the handle's previous batch (+ 1/8), the kernels read the totals on the device, and a batch
                                // that does not fit is refused there and redone with the exact sizes when its result is first asked for anything
  bool force_fallbacks = false; // "force_fallbacks": the count-then-emit pairs of walks that query types 2 - 5 fall back to when a region
                                // outgrows the capacity of its recording walk (tests of those paths)
  // ---- read from the environment when the handle is opened ----
  bool phase_events = false;    // walking batches record all five phase events (vs_index_last_timing's phases); default: first and last only
  bool no_t4_events = false;    // VS_T4_NO_EVENTS: do not build the event bitmaps at all
  int plan_stream_priority = 0; // VS_PLAN_STREAM_PRIORITY: high (+1) / low (-1): the priority of the stream the plan of a type-6 batch and the part of a walking
                                // batch in front of its host wait run on (0: default priority)
  uint32_t plan_items = 1;      // VS_PLAN_ITEMS: regions per thread of the plan's kernels for batches of 64 k regions and more (fewer, longer waves beside
                                // the previous batch's expansion: what the plan costs the expansion is the wave slots its waves hold)
  bool t4_exact_rows = false;   // VS_T4_EXACT_ROWS: an explicit-id cohort gets exact per-sample rows (a bit per slot and a hold row) instead of round 4's
                                // coarse event rows (a bit per 8 slots, hold tests from the carrier lists) when they fit the budget
  // ---- tuning builds only (VS_TUNING: VS_BUILD_TUNING=1 python -m variantstore_amd.build --force) ----
  bool lat_debug = false;       // device-clock stamps of the latency kernels on stderr
  bool fill_fused = true;       // shared batches: the expansion writes the shared rows as well (k_fill_sites2); false: k_share_rows2 + k_fill_sites
  uint32_t fill_chunk = 0;      // rows per task of the expansion: 0 = by the batch's shape, else 8 / 16 / 32 / 64
  uint32_t burden_chunk = 0;    // rows one workgroup of the burden kernel walks before a region is split: 0 = kBurdenChunkRows
  uint32_t window_chunk = 0;    // rows one wave of the window-statistics kernel walks before a region is split: 0 = kWinChunkRows
  uint32_t matrix_max_mib = 0;  // largest genotype matrix a batch may ask for, MiB: 0 = 32 GiB
  uint32_t assoc_lds_max_kib = 0;   // largest phenotype table k_assoc_scan stages in LDS, KiB: 0 = 32; a larger one is read through global memory
  uint32_t score_chunk = 0;     // table rows one workgroup of k_sample_scores walks: 0 = kScoreChunkRows, else 64..65536
  uint32_t score_tile_cols = 0; // column tile of k_sample_scores: 0 = all a 64 KiB tile holds, 65536 / (8 Kp); else a multiple of 16, held to that
  uint32_t gram_chunk = 0;      // table rows one workgroup of k_sample_gram sums: 0 = by the batch's shape (gram_chunk_rows), else 64..65536
  uint32_t score_matrix_chunk = 0;   // table rows one workgroup of k_score_matrix sums: 0 = by the batch's shape (score_matrix_chunk_rows), else a multiple of 128 in 128..65536
  uint32_t ibs_chunk = 0;       // table rows one workgroup of k_sample_ibs sums: 0 = by the batch's shape (ibs_chunk_rows), else 64..65536
  uint32_t trio_chunk = 0;      // trios one workgroup of k_trio_scan takes: 0 = by the batch's shape (trio_chunk_trios), else a multiple of 64 in 64..16384
  uint32_t matrix_tile_cols = 0;   // column tile of the matrix kernel: 0 = kMatrixTileCols, else a multiple of 16 in 16..65536
  int fill_mode = 0;            // shared expansion: 0 one launch, 2 split (lists + rows, then the dense sites: what a profiler wants to see apart)
  uint32_t fill_dense_k = 16;   // dense sites per wave of k_fill_dense: 8 / 16 / 32 / 64
  bool fill_stats = false;      // device-clock ticks per phase of the expansion's tasks (k_fill_sites2)
  int sc_group = 1;             // lanes per region of the walks of query types 2 / 3 / 5: 1, or 8 lanes running the same chain
  bool walk_stats = false;      // iteration counts and device-clock ticks of k_sample_walk
  uint32_t fill_ablate = 0;     // skip a regime of the expansion
  size_t fill_lds_pad = 0;      // pad the fill kernel's LDS block (occupancy experiments)
};


struct vs_index {
  HostGraph g;
  HostImage im;
  DevImage d{};
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  std::vector<void*> image_allocs;
  uint64_t device_bytes = 0;
  uint64_t t4_rows_bytes = 0;   // of which: the per-sample event and hold rows of query type 4
  uint64_t t4_alloc_bytes = 0;   // what build_t4_rows added to device_bytes (drop_t4_rows takes it off again)
  uint64_t pool_mallocs = 0, pool_frees = 0;   // hipMalloc / hipFree calls of the batch-buffer pool (vs_index_info)
  std::string seq_chars;
  std::unordered_map<std::string, uint32_t> sample_ids;
  std::vector<DevBuf> pool;
  // [V] list claims of the walking query types (kernels.hip.h: k_t4_claim), generation-stamped.  TWO tables, taken in turn: the claims of
  // a batch are made in front of its host wait on the second stream while the emitter of the batch before may still be reading its own
  // on the handle's stream; a table's next user (two batches on) waits for the completion event of its last (t4_claim_done).
  unsigned long long* t4_claim[2] = {nullptr, nullptr};
  hipEvent_t t4_claim_done[2] = {nullptr, nullptr};
  uint64_t t4_gen = 0;
  hipStream_t plan_stream = nullptr;        // the plan of an async_submit batch runs here, beside the previous batch's expansion on `stream`
  hipStream_t fill_stream = nullptr;        // second stream: the expansion of an async_fill batch
  hipEvent_t fill_ev[2] = {nullptr, nullptr};
  bool sort_hint = false;                   // the last shared batch arrived unsorted and was sorted on the device
  uint32_t sort_probe_in = 0;
  uint64_t seq_cap_hint[2] = {0, 0};        // the same for the piece lists of query types 2 / 3
  uint64_t walk_cap_hint[2] = {0, 0};       // scratch entries the last type-4 / type-5 batch's recording walk needed (+ 1/8): the next batch's allocation
  // A hint shrinks only after kHintShrinkAfter CONSECUTIVE batches that needed less than a quarter of it, and then to the largest of
  // those: a handle that alternates large and small batches keeps the large scratch (one host wait per batch) instead of having every
  // large batch refused on the device and redone.  [0 / 1]: walk hints, [2 / 3]: sequence hints.
  uint32_t hint_small_runs[4] = {0, 0, 0, 0};
  uint64_t hint_small_max[4] = {0, 0, 0, 0};
  // speculative type-6 batches (run_type6_shared, result_sizes): what the last shared batch needed (+ 1/8) and how many regions it had;
  // a ring of totals mailboxes in mapped host memory (kPinPlanRing), one per batch in flight, and who is still to read which
  uint64_t t6_hint_rows = 0, t6_hint_arena = 0, t6_hint_n = 0;
  uint32_t t6_small_runs = 0;
  uint64_t t6_small_rows = 0, t6_small_arena = 0;
  static constexpr int kPlanSlots = 8;
  vs_result* plan_slot_owner[kPlanSlots] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  uint32_t plan_slot_next = 0;
  uint32_t assoc_lds_raised = 0;   // k_assoc_scan instantiations whose dynamic-LDS limit this handle's device has raised (launch_assoc_form), a bit each
  uint64_t t6_speculated = 0, t6_refused = 0;   // batches submitted without a host wait / of those, refused on the device and redone (vs_index_info)
  uint64_t share_seq = 0;                   // sequence number of the plan's totals mailbox
  uint64_t done_seq = 0;                    // sequence number of the batch completion word
  uint64_t* walk_words = nullptr;           // the flag words of the walking batches (batch_words): zero between batches
  bool walk_words_dirty = true;
  hipStream_t pre = nullptr;                // the stream the part of a walking batch IN FRONT of its host wait is on (PreStream below); NULL: the handle's
  bool batch_in_flight = false;             // a batch returned when it was enqueued (async_submit) and nothing has synchronised the stream since
  hipEvent_t tev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // the events collect_timing reads: the handle's own (ev[]) or, for a
                                            // lean batch, the result's pair around its expansion (timing_owner)
  vs_result* timing_owner = nullptr;
  bool timing_total_only = false;           // ... and recorded only its first and last event (query types 2 / 3)
  bool timing_pending = false;              // the last batch returned before its kernels had finished: vs_index_last_timing reads the events then
  uint64_t timing_fill_launches = 0;
  std::vector<hipEvent_t> ev_pool;          // timing events of results (two per shared batch), reused between results
  // resident carrier lists (DevImage::v_abegin): the arena, its length in entries, and -- once a caller has asked for
  // carriers on the host -- its page-locked host mirror, shared by every result of the handle
  void* res_arena = nullptr;
  uint64_t res_entries = 0, res_site_entries = 0;
  void* res_mirror = nullptr;
  std::vector<DevBuf> pin_pool;        // page-locked host buffers of raw result copies (vs_result_get_raw), reused between results
  hipStream_t copy_stream = nullptr;   // device-to-host copies of the streamed form run here, beside the next chunk's kernels
  vs_timing timing{};
  vs_construct_stats cstats{};
  uint64_t live_results = 0;
  uint64_t live_comms = 0;     // communicators (vs_comm) made on this handle: they keep its device and stream in use
  bool close_pending = false;  // vs_index_close was called while results or communicators were alive
  unsigned long long* done_counter = nullptr;   // device word of the latency path's completion mailbox
  uint64_t lat_seq = 0;
  // resident query server of the latency path (kernels.hip.h: k_query_server)
  hipStream_t srv_stream = nullptr;
  bool srv_alive = false;
  std::chrono::steady_clock::time_point srv_started{}, srv_last{};
  uint64_t srv_seq = 1;                          // sequence number of the next request
  unsigned long long* srv_counter = nullptr;     // device word: blocks done with the current request
  std::vector<uint64_t> h_carpre;   // host copy of DevImage::s_carpre (arena prefix): sizes of the latency path's results
  EngineOpts opts;
  // back-to-back detection for opts.server == 1: small queries that followed the previous one within kSrvStreakGap
  uint32_t small_streak = 0;
  std::chrono::steady_clock::time_point last_small_done{};
  uint64_t* pinned = nullptr;  // 16 KiB of mapped host memory (uint64 words): latency-path mailboxes, server request, batch totals
  static constexpr size_t kPinTotals = 0;     // [0..2] latency path, lat_debug only: device-clock durations (kernel, bounds, tasks)
  static constexpr size_t kPinFlag = 6;       // latency path: completion sequence number
  static constexpr size_t kPinSrvResp = 16;   // [16..20] resident server: sequence number of the last request answered (+ debug stamps)
  static constexpr size_t kPinSrvReq = 256;   // [256 .. 256 + 136) resident server: the request (ServerRequest, 64-byte aligned)
  static constexpr size_t kPinBatch = 1040;   // [1040..1041] throughput path, private rows: slots and arena entries of the batch
  static constexpr size_t kPinPlan = 1056;    // [1056..1063] throughput path, shared rows: PlanTotals of the batch (k_t6_apply), sequence word last
  static constexpr size_t kPinDone = 1072;    // completion word of a batch (k_post_done)
  static constexpr size_t kPinWords = 1080;   // [1080..1083] three device words + sequence (k_post_words: read_device_words)
  static constexpr size_t kPinPlanRing = 1104;   // [1104 .. 1104 + 8 x 8) PlanTotals of the speculative batches in flight (kPlanSlots mailboxes)
};

struct vs_result {
  vs_index* idx = nullptr;
  DevResult d{};
  std::vector<DevBuf> bufs;
  std::vector<DevBuf> call_temps;   // temporaries of the call that an enqueued batch's kernels still use and no accessor reads (an LD batch's
                                    // genotype matrix): back to the pool as soon as the batch is known to have finished (result_ready)
  // host copies
  bool have_headers = false, have_carriers = false;
  std::vector<uint8_t> h_flags;
  std::vector<uint64_t> h_var_begin, h_nvar, h_var_count, h_car_base;   // per region: first table row, rows, variants reported, arena offset
  std::vector<VariantRow> h_rows;           // the variant table as it lies in HBM (rows may be shared between regions)
  // the host VIEW: every region's rows expanded back to back (slot = region-major row), carrier lists back to back
  std::vector<uint64_t> h_view_begin, h_pos, h_car_begin, h_car_begin_view;   // h_car_begin: arena offsets per slot
  std::vector<uint32_t> h_ref_off, h_ref_len, h_alt_off, h_alt_len, h_vflags, h_car_count, h_carriers;
  uint64_t n_variants = 0, n_carriers_kept = 0, n_bases = 0, n_view_carriers = 0;
  bool have_totals = false;
  std::string text;
  std::vector<uint32_t> slice_carriers;
  // per-region arrays alone (flags, slot and arena offsets, counts): all that totals and single-region formatting need
  bool have_meta = false;
  bool shared_lists = false;          // rows and carrier lists shared between the regions of the batch (DevResult::q_car_len valid)
  uint64_t n_unique_sites = 0;        // lists actually expanded: unique covered sites when shared, else the rows
  uint64_t n_rows_reported = 0;       // rows over all regions (shared rows counted once per region that reports them)
  // async_fill: the expansion of this result is (or was) in flight on the handle's second stream
  bool pending = false;
  hipEvent_t ev_fill[2] = {nullptr, nullptr};   // around the expansion, on the stream it runs on
  hipEvent_t ev_done = nullptr;       // behind the LAST kernel of a batch that returned when it was enqueued (async_submit): nothing of the result
                                      // -- its buffers, the call's temporaries it keeps -- goes back to the pool before this has happened
  float fill_ms = -1.0f;
  // a SPECULATIVE type-6 batch: d.A / d.S hold what was ALLOCATED until somebody asks for the result's sizes (result_sizes)
  bool sizes_pending = false, totals_captured = false;
  int redo_rc = VS_OK;                // the redo of a refused batch failed with this code: the result is torn, every accessor returns it (result_enter)
  int plan_slot = -1;
  uint64_t plan_seq = 0, cap_rows = 0, cap_arena = 0;
  PlanTotals plan_copy{};
  bool resident = false;              // the carrier arena is the index's (vs_index::res_arena), not this result's
  bool scattered_lists = false;       // lists shared per vertex (walking query types): a region's carriers are not one arena range
  std::vector<uint64_t> h_car_len;
  // the rows of ONE region, fetched when the whole table is not on the host (vs_result_format_region)
  std::vector<VariantRow> sl_rows;
  // the RAW host copy (vs_result_get_raw): variant table and arena exactly as they lie in HBM, in page-locked memory
  DevBuf raw_pin{nullptr, 0};
  std::vector<DevBuf> old_pins;   // earlier raw copies of this result (rows only, then rows + carriers): pointers handed out stay valid until it is freed
  const VariantRow* raw_rows = nullptr;
  const uint8_t* raw_arena = nullptr;   // NULL: carriers not copied
  int kind = 0;  // 7: samples_has_var result (vs_result_format_region writes the sample line); 2 / 3: sequences; kKindCounts: allele counts;
                 // kKindBurden: per-sample burden; kKindMatrix: genotype matrix; kKindLd: banded LD; kKindGroups: grouped allele counts; kKindAssoc: association scan;
                 // kKindScores: per-sample scores; kKindGram: sample Gram matrix / GRM; kKindIbs: pairwise IBS counts / KING kinship;
                 // kKindLdMatrix: the full LD block of every region; kKindAssocMatrix: trait-matrix association scan;
                 // kKindScoreMatrix: score matrix; kKindPrune: LD pruning verdicts; kKindClump: p-value clumping verdicts; kKindLdScore: LD scores;
                 // kKindWindowStats: windowed diversity statistics; kKindTrio: Mendelian errors and transmission counts per row and trio;
                 // kKindRoh: runs of homozygosity per region and column
  // allele-count results (vs_query_allele_counts): 16 bytes per table row in HBM, and their page-locked host copy
  uint4* d_counts = nullptr;
  DevBuf counts_pin{nullptr, 0};
  // grouped-count results (vs_query_group_counts): n_groups records per table row in d_counts / counts_pin (row-major), the groups'
  // sizes and -- when the caller gave them -- names (else the decimal index stands for a group)
  uint32_t n_groups = 0;
  std::vector<uint32_t> group_sizes;
  std::vector<std::string> group_names;
  // association-scan results (vs_query_assoc_scan): table rows x n_traits float64 cells in HBM (row-major) and their page-locked host
  // copy in cells_pin, the count record of every table row over the subset in d_counts / counts_pin as for a count result, the column
  // ids h_cols, per trait Sy and Syy over the columns, and the traits' names (empty: the decimal index stands for a trait)
  double* d_scores = nullptr;
  uint32_t n_traits = 0, assoc_stat = 0;
  std::vector<double> trait_sum, trait_sumsq;
  std::vector<std::string> trait_names;
  // trait-matrix association results (vs_query_assoc_matrix): the same fields (n_traits up to VS_TRAIT_MATRIX_MAX; trait_sum and
  // trait_sumsq from the exact integer sums) and f_k per trait; d_cell_total, two words of their own, is the matrix kernel's
  std::vector<int32_t> trait_shift;
  // score results (vs_query_sample_scores): columns x n_scores int64 sums in HBM (row-major) with the float64 scores formed from
  // them right behind (d_score_out), both copied to cells_pin in one piece; the kernels' words (largest |w| per column, the
  // pair count of vs_result_totals); f_k per column and the scores' names (empty: the decimal index stands for a score)
  long long* d_sums = nullptr;
  double* d_score_out = nullptr;
  ScoreMeta* d_score_meta = nullptr;
  uint32_t n_scores = 0;
  std::vector<int32_t> score_shift;
  std::vector<std::string> score_names;
  // score-matrix results (vs_query_score_matrix): d_sums / d_score_out, h_cols, n_scores (up to VS_SCORE_MATRIX_MAX), score_shift and
  // score_names as for a score result; the limbs the kernel ran with (4 or 5); the nonzero cells of the (temporary) genotype matrix
  // in d_cell_total (two words of their own); the count record of every table row in d_counts as for a Gram result
  uint32_t sm_limbs = 0;
  // burden results (vs_query_sample_burden): the regions x columns matrix in HBM (16 bytes per cell, row-major), the sum of its
  // `variants` (a device word the kernels add to), the column ids, and the matrix's page-locked host copy
  uint4* d_cells = nullptr;
  unsigned long long* d_cell_total = nullptr;
  std::vector<uint32_t> h_cols;
  DevBuf cells_pin{nullptr, 0};
  std::vector<uint4> sl_cells;   // the cells of ONE region, fetched when the matrix is not on the host (vs_result_format_region)
  // genotype-matrix results (vs_query_genotype_matrix): table rows x columns bytes in HBM, rows mx_pitch bytes apart; the nonzero
  // total is d_cell_total, the column ids h_cols and the page-locked host copy cells_pin, as for a burden result
  uint8_t* d_matrix = nullptr;
  uint64_t mx_pitch = 0;
  std::vector<uint8_t> sl_matrix;   // the rows of ONE region, fetched when the matrix is not on the host (vs_result_format_region)
  // LD results (vs_query_ld_band): table rows x window cells of four bytes in HBM (int32 under VS_LD_DOT, float under VS_LD_R2), the
  // count record of every table row in d_counts / counts_pin as for a count result, the column ids h_cols, the nonzero cells of the
  // (temporary) genotype matrix in d_cell_total; the band's page-locked host copy is cells_pin
  uint32_t* d_band = nullptr;
  uint32_t ld_window = 0, ld_stat = 0;
  std::vector<uint32_t> sl_band;   // the band rows of ONE region (vs_result_format_region)
  // LD-matrix results (vs_query_ld_matrix): per region a square block of four-byte cells in HBM (d_ldm, ldm_cells of them in all;
  // ld_stat says which), one buffer of 8-byte words beside it -- block_begin [Q + 1], the workgroup prefix [Q + 1], the scan's summary
  // (four words), the nonzero cells of the (temporary) genotype matrix (d_cell_total, two words) --, counts and column ids as for an
  // LD result; the cells' page-locked host copy is cells_pin, block_begin's host copy h_block_begin, sl_band the block of ONE region
  uint32_t* d_ldm = nullptr;
  uint64_t* d_ldm_meta = nullptr;
  uint64_t ldm_cells = 0, ldm_wgs = 0;
  std::vector<uint64_t> h_block_begin;
  // pruning results (vs_query_ld_prune): a verdict byte per reported row in HBM (d_state, prune_states of them), one buffer of 8-byte
  // words beside it -- keep_begin [Q + 1], n_kept [Q + 1, the last unused], the scan's summary (two words), the nonzero cells of the
  // (temporary) genotype matrix (d_cell_total, two words) --, counts and column ids as for an LD result, ld_window and the other
  // parameters of the walk; the state's page-locked host copy is cells_pin, the per-region words' host copy h_prune_meta
  uint8_t* d_state = nullptr;
  uint64_t* d_prune_meta = nullptr;
  uint64_t prune_states = 0;
  uint32_t prune_max_bp = 0, prune_T = 0, prune_min_ac = 0, prune_max_ac = UINT32_MAX;
  std::vector<uint64_t> h_prune_meta;
  // LD-score results (vs_query_ld_scores): one buffer in HBM (d_ldscore) of prune_states slots -- sums [uint64], then n_pairs
  // [uint32], then state [uint8], 13 bytes a slot --, copied to cells_pin in one piece; the 8-byte words beside it in d_prune_meta:
  // keep_begin [Q + 1], wg_begin [Q + 1], n_scored [Q + 1, the last unused], the scan's summary (four words), the nonzero cells of
  // the (temporary) genotype matrix (d_cell_total, two words); counts, column ids, ld_window (0: no limit), prune_max_bp,
  // prune_min_ac and prune_max_ac as for a pruning result; ldscore_wgs: the score kernel's workgroups
  uint8_t* d_ldscore = nullptr;
  uint64_t ldscore_wgs = 0;
  // window-statistics results (vs_query_window_stats): one buffer in HBM (d_wstats) -- Q x n_groups records of 48 bytes, then
  // Q x ws_pairs pair records of 16 bytes (ws_pairs: n_groups (n_groups - 1) / 2, or 0 without pairs) --, copied to cells_pin in one
  // piece; n_groups, group_sizes and group_names as for a grouped-count result; the chunks of the split regions in d_cell_total's
  // second word.  The grouped counts the records are reduced from are a temporary of the call
  uint8_t* d_wstats = nullptr;
  uint32_t ws_pairs = 0;
  std::vector<const char*> ws_name_ptrs;   // group_names as the array of C strings vs_result_get_window_stats hands out
  // clumping results (vs_query_ld_clump): d_state, d_prune_meta, prune_states, ld_window, prune_max_bp and prune_T as for a pruning
  // result -- the words are keep_begin [Q + 1], n_index [Q + 1, the last unused], the scan's summary, d_cell_total, then the rounds
  // every region took [Q + 1, the last unused] --, an owner per verdict beside the state (d_owner, its page-locked copy owner_pin),
  // the keys of the table rows as the caller's p-values gave them (h_clump_keys: the batch uploads them, the text prints them), p1
  // and p2 with their keys
  uint32_t* d_owner = nullptr;
  DevBuf owner_pin{nullptr, 0};
  std::vector<uint64_t> h_clump_keys;
  double clump_p[2] = {0.0, 0.0};
  uint64_t clump_key[2] = {0, 0};
  // Gram results (vs_query_sample_gram): one buffer of 8-byte words in HBM -- gram [n x n] int64, col_weighted [n] int64, C, H, the
  // nonzero cells of the (temporary) genotype matrix (d_cell_total, two words), then from gram_grm_off on grm [n x n] float64 under
  // VS_GRAM_GRM -- copied to cells_pin in one piece; the count record of every table row in d_counts / counts_pin, the column ids h_cols
  long long* d_gram = nullptr;
  size_t gram_grm_off = 0, gram_words = 0;
  uint32_t gram_stat = 0;
  // IBS results (vs_query_sample_ibs): one buffer of 8-byte words in HBM -- het_het, hom_hom, carrier_both, ibs0, ibs2 ([n x n] int64
  // each), n_used, the nonzero cells of the (temporary) genotype matrix (d_cell_total, two words), then from ibs_king_off on king
  // [n x n] float64 under VS_IBS_KING -- copied to cells_pin in one piece; counts and column ids as for a Gram result
  long long* d_ibs = nullptr;
  size_t ibs_king_off = 0, ibs_words = 0;
  uint32_t ibs_stat = 0;
  // trio results (vs_query_trio_scan): one buffer in HBM (d_trio) -- a record of 16 bytes per table row, one per trio, n_used (8 bytes),
  // the nonzero cells of the (temporary) genotype matrix (d_cell_total, two words), then from trio_table_off on the trio table, three
  // column indices of four bytes per trio -- copied to cells_pin in one piece (trio_bytes); the count record of every table row in
  // d_counts / counts_pin, the member ids h_cols
  uint8_t* d_trio = nullptr;
  uint64_t n_trios = 0;
  size_t trio_table_off = 0, trio_bytes = 0;
  std::vector<uint32_t> h_trio_cols;   // the table as the batch uploads it
  // ROH results (vs_query_roh): one buffer in HBM (d_roh) -- Q x n_cols summaries of 32 bytes, n_sites (4 bytes a region, rounded up
  // to 16), the nonzero cells of the (temporary) genotype matrix (d_cell_total, two words), then from roh_begin_off on seg_begin
  // (Q x n_cols + 1 words of 8 bytes; with segments only) -- copied to cells_pin in one piece (roh_bytes); the segments (32 bytes
  // each, roh_segs of them) in d_roh_seg / owner_pin; the count record of every table row in d_counts / counts_pin, the column ids h_cols
  uint8_t* d_roh = nullptr;
  uint4* d_roh_seg = nullptr;
  size_t roh_sites_off = 0, roh_begin_off = 0, roh_bytes = 0;
  uint64_t roh_segs = 0;
  vs_roh_params roh{};
  // sequence results (query types 2 and 3)
  DevSeqResult sq{};
  uint64_t seq_bytes = 0;
  bool have_seq = false;
  std::vector<uint64_t> h_byte_begin;
  std::vector<uint8_t> h_chars;
};

constexpr int kKindCounts = 8;   // vs_result::kind of an allele-count result: the rows of type 6, counts instead of carrier lists
static int refuse_counts(const char* what) {
  return fail(VS_ERR_UNSUPPORTED, "%s: an allele-count result holds counts per row, no carrier lists (vs_result_get_allele_counts)", what);
}
constexpr int kKindBurden = 9;   // ... of a burden result: the rows of type 6, a regions x samples matrix instead of carrier lists
constexpr int kKindMatrix = 10;  // ... of a genotype-matrix result: the rows of type 6, a table rows x samples byte matrix instead of carrier lists
constexpr int kKindLd = 11;      // ... of an LD result: the rows of type 6, a table rows x window band of pair statistics instead of carrier lists
constexpr int kKindGroups = 12;  // ... of a grouped-count result: the rows of type 6, a count record per row and sample group instead of carrier lists
constexpr int kKindAssoc = 13;   // ... of an association-scan result: the rows of type 6, a score per row and trait instead of carrier lists
constexpr int kKindScores = 14;  // ... of a per-sample score result: the rows of type 6, a columns x scores matrix of weighted dosage sums instead of carrier lists
constexpr int kKindGram = 15;    // ... of a Gram result: the rows of type 6, a samples x samples matrix of dosage products instead of carrier lists
constexpr int kKindIbs = 16;     // ... of an IBS result: the rows of type 6, samples x samples matrices of genotype-state counts instead of carrier lists
constexpr int kKindLdMatrix = 17;   // ... of an LD-matrix result: the rows of type 6, a square block of pair statistics per region instead of carrier lists
constexpr int kKindAssocMatrix = 18;   // ... of a trait-matrix association result: the rows of type 6, a score per row and trait (up to VS_TRAIT_MATRIX_MAX traits) instead of carrier lists
constexpr int kKindScoreMatrix = 19;   // ... of a score-matrix result: the rows of type 6, a columns x scores matrix of weighted dosage sums (up to VS_SCORE_MATRIX_MAX scores) instead of carrier lists
constexpr int kKindPrune = 20;   // ... of a pruning result: the rows of type 6, a verdict byte per reported row instead of carrier lists
constexpr int kKindLdScore = 22;   // ... of an LD-score result: the rows of type 6, a sum, a pair count and a state byte per reported row instead of carrier lists
constexpr int kKindWindowStats = 23;   // ... of a window-statistics result: the rows of type 6, a record per region and sample group (and pair of groups) instead of carrier lists
constexpr int kKindTrio = 24;    // ... of a trio result: the rows of type 6, a record of Mendelian errors and transmission counts per row and per trio instead of carrier lists
constexpr int kKindRoh = 25;     // ... of a ROH result: the rows of type 6, a summary per region and column and the segments instead of carrier lists
constexpr int kKindClump = 21;   // ... of a clumping result: the rows of type 6, a verdict byte and an owner per reported row instead of carrier lists
static bool no_lists(const vs_result* r) {
  return r->kind == kKindRoh || r->kind == kKindTrio || r->kind == kKindWindowStats || r->kind == kKindLdScore || r->kind == kKindClump || r->kind == kKindPrune || r->kind == kKindScoreMatrix || r->kind == kKindAssocMatrix || r->kind == kKindLdMatrix || r->kind == kKindIbs || r->kind == kKindGram || r->kind == kKindCounts || r->kind == kKindBurden || r->kind == kKindMatrix || r->kind == kKindLd || r->kind == kKindGroups || r->kind == kKindAssoc ||
         r->kind == kKindScores;
}
static int refuse_no_lists(const vs_result* r, const char* what) {
  if (r->kind == kKindCounts) return refuse_counts(what);
  if (r->kind == kKindGroups)
    return fail(VS_ERR_UNSUPPORTED, "%s: a grouped-count result holds counts per row and group, no carrier lists (vs_result_get_group_counts)", what);
  if (r->kind == kKindAssoc)
    return fail(VS_ERR_UNSUPPORTED, "%s: an association-scan result holds a score per row and trait, no carrier lists (vs_result_get_assoc_scan)", what);
  if (r->kind == kKindAssocMatrix)
    return fail(VS_ERR_UNSUPPORTED, "%s: a trait-matrix association result holds a score per row and trait, no carrier lists (vs_result_get_assoc_matrix)", what);
  if (r->kind == kKindScores)
    return fail(VS_ERR_UNSUPPORTED, "%s: a per-sample score result holds a score per sample and weight column, no carrier lists (vs_result_get_sample_scores)", what);
  if (r->kind == kKindScoreMatrix)
    return fail(VS_ERR_UNSUPPORTED, "%s: a score-matrix result holds a score per sample and weight column, no carrier lists (vs_result_get_score_matrix)", what);
  if (r->kind == kKindGram)
    return fail(VS_ERR_UNSUPPORTED, "%s: a Gram result holds a samples x samples matrix of dosage products, no carrier lists (vs_result_get_sample_gram)", what);
  if (r->kind == kKindIbs)
    return fail(VS_ERR_UNSUPPORTED, "%s: an IBS result holds samples x samples matrices of genotype-state counts, no carrier lists (vs_result_get_sample_ibs)", what);
  if (r->kind == kKindTrio)
    return fail(VS_ERR_UNSUPPORTED, "%s: a trio result holds a record of Mendelian errors and transmission counts per row and per trio, no carrier lists (vs_result_get_trio_scan)", what);
  if (r->kind == kKindRoh)
    return fail(VS_ERR_UNSUPPORTED, "%s: a ROH result holds a summary per region and column and the segments, no carrier lists (vs_result_get_roh)", what);
  if (r->kind == kKindLdMatrix)
    return fail(VS_ERR_UNSUPPORTED, "%s: an LD-matrix result holds a square block of pair statistics per region, no carrier lists (vs_result_get_ld_matrix)", what);
  if (r->kind == kKindClump)
    return fail(VS_ERR_UNSUPPORTED, "%s: a clumping result holds a verdict and an owner per reported row, no carrier lists (vs_result_get_ld_clump)", what);
  if (r->kind == kKindWindowStats)
    return fail(VS_ERR_UNSUPPORTED, "%s: a window-statistics result holds a record per region and group, no carrier lists (vs_result_get_window_stats)", what);
  if (r->kind == kKindLdScore)
    return fail(VS_ERR_UNSUPPORTED, "%s: an LD-score result holds a sum of r2 per reported row, no carrier lists (vs_result_get_ld_scores)", what);
  if (r->kind == kKindPrune)
    return fail(VS_ERR_UNSUPPORTED, "%s: a pruning result holds a verdict per reported row, no carrier lists (vs_result_get_ld_prune)", what);
  if (r->kind == kKindLd)
    return fail(VS_ERR_UNSUPPORTED, "%s: an LD result holds a rows x window band of pair statistics, no carrier lists (vs_result_get_ld_band)", what);
  if (r->kind == kKindMatrix)
    return fail(VS_ERR_UNSUPPORTED, "%s: a genotype-matrix result holds a rows x samples matrix, no carrier lists (vs_result_get_genotype_matrix)", what);
  return fail(VS_ERR_UNSUPPORTED, "%s: a burden result holds a regions x samples matrix, no carrier lists (vs_result_get_sample_burden)", what);
}

// ------------------------------------------------------------------ helpers
static int server_stop(vs_index* idx);   // the resident latency server must be gone before anything that synchronises the
                                         // whole device (hipFree does): it would otherwise wait for the server's idle clock

static int dev_alloc(vs_index* idx, size_t bytes, void** out, std::vector<DevBuf>* owner) {
  if (bytes == 0) bytes = 8;
  bytes = (bytes + 255) & ~(size_t)255;
  // best fit from the pool
  int best = -1;
  for (size_t i = 0; i < idx->pool.size(); ++i)
    if (idx->pool[i].cap >= bytes && (best < 0 || idx->pool[i].cap < idx->pool[best].cap)) best = (int)i;
  if (best >= 0 && idx->pool[best].cap <= 2 * bytes + (256 << 10)) {   // never more than twice (+256 KiB) what was asked for
    DevBuf b = idx->pool[best];
    idx->pool.erase(idx->pool.begin() + best);
    *out = b.p;
    if (owner) owner->push_back(b);
    return VS_OK;
  }
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  idx->pool_mallocs++;
  if (e != hipSuccess) {
    // release the pool and retry once
    (void)server_stop(idx);
    for (auto& b : idx->pool) { (void)hipFree(b.p); idx->pool_frees++; }
    idx->pool.clear();
    e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return fail(VS_ERR_HIP, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  }
  *out = p;
  if (owner) owner->push_back(DevBuf{p, bytes});
  return VS_OK;
}

template <typename T>
static int upload_image(vs_index* idx, const std::vector<T>& v, const T** dptr) {
  size_t bytes = v.size() * sizeof(T);
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, bytes + 64));   // (slack: k_copy_segments reads 16 bytes at a time, up to 15 beyond a piece)
  idx->image_allocs.push_back(p);
  idx->device_bytes += bytes;
  if (bytes) HIP_TRY(hipMemcpyAsync(p, v.data(), bytes, hipMemcpyHostToDevice, idx->stream));
  *dptr = (const T*)p;
  return VS_OK;
}
template <typename T>
static int alloc_image(vs_index* idx, size_t n, T** dptr) {
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, n ? n * sizeof(T) : 8));
  idx->image_allocs.push_back(p);
  idx->device_bytes += n * sizeof(T);
  *dptr = (T*)p;
  return VS_OK;
}

// Walking batches (query types 4, 5, 2, 3) under async_submit run everything in front of their one host wait -- copies, capacities,
// scans, the recording walk, the claims -- on the handle's SECOND stream (vs_index::plan_stream), beside the rows and the carrier
// expansion of the batch before, which are on the handle's stream; the host has seen that part's last kernel post its words before
// it enqueues the rest, so no event links the two.  What the part reads is the caller's input and the index, what it writes is the
// batch's own (a batch that returned when it was enqueued keeps its temporaries until its completion event) -- but for the claim
// tables of the type-4 lists, which belong to the handle: two, taken in turn (vs_index::t4_claim).
// The helpers below launch on work_stream(idx): the second stream while a PreStream guard is alive, else the handle's.
static inline hipStream_t work_stream(const vs_index* idx) { return idx->pre ? idx->pre : idx->stream; }
struct PreStream {
  vs_index* idx;
  PreStream(vs_index* i, hipStream_t s) : idx(i) { i->pre = s; }
  // (left without done(): an error on the way -- whatever was launched has to be over before the caller releases the result's buffers,
  //  which nothing on the handle's own stream is ordered behind)
  ~PreStream() { if (idx->pre) (void)hipStreamSynchronize(idx->pre); idx->pre = nullptr; }
  void done() { idx->pre = nullptr; }
};

// out[0..n) = exclusive prefix of in, out[n] = total
template <typename T>
static int exclusive_scan(vs_index* idx, const T* in, uint64_t n, uint64_t* out, std::vector<DevBuf>* scratch_owner) {
  if (n == 0) {
    HIP_TRY(hipMemsetAsync(out, 0, 8, work_stream(idx)));
    return VS_OK;
  }
  if (n <= kScanSmallMax && (const void*)in != (const void*)out) {   // one launch instead of three
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_small<T>), dim3((unsigned)((n + kScanSmallTile - 1) / kScanSmallTile)), dim3(kScanSmallBlock), 0, work_stream(idx), in, (uint32_t)n, out);
    HIP_TRY(hipGetLastError());
    return VS_OK;
  }
  const uint64_t ntiles = (n + kScanTile - 1) / kScanTile;
  void* ts = nullptr;
  VS_TRY(dev_alloc(idx, ntiles * 8, &ts, scratch_owner));
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_tile_sums<T>), dim3((unsigned)ntiles), dim3(kScanBlock), 0, work_stream(idx), in, n, (uint64_t*)ts);
  hipLaunchKernelGGL(k_scan_spine, dim3(1), dim3(kScanBlock), 0, work_stream(idx), (uint64_t*)ts, ntiles, out + n);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_apply<T>), dim3((unsigned)ntiles), dim3(kScanBlock), 0, work_stream(idx), in, n, (const uint64_t*)ts, out);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}

// var_begin / car_base of a batch in one pass (k_scan2_*): out[0..n) = exclusive prefixes, out[n] = totals, which the
// spine kernel also writes to `host_totals` (mapped host memory; NULL = not wanted) -- no staged device-to-host copy.
static int scan_offsets(vs_index* idx, const uint64_t* nvar, const uint64_t* ncar, uint64_t n, uint64_t* var_begin, uint64_t* car_base,
                        uint64_t* host_totals, std::vector<DevBuf>* scratch_owner) {
  if (n <= kScanSmallMax) {   // one launch instead of three
    hipLaunchKernelGGL(k_scan2_small, dim3((unsigned)std::max<uint64_t>(1, (n + kScanSmallTile - 1) / kScanSmallTile)), dim3(kScanSmallBlock), 0, work_stream(idx), nvar, ncar,
                       (uint32_t)n, var_begin, car_base, host_totals);
    HIP_TRY(hipGetLastError());
    return VS_OK;
  }
  const uint64_t ntiles = n ? (n + kScanTile - 1) / kScanTile : 0;
  void* ts = nullptr;
  VS_TRY(dev_alloc(idx, (ntiles + 1) * sizeof(Scan2), &ts, scratch_owner));
  if (ntiles) hipLaunchKernelGGL(k_scan2_tile_sums, dim3((unsigned)ntiles), dim3(kScanBlock), 0, work_stream(idx), nvar, ncar, n, (Scan2*)ts);
  hipLaunchKernelGGL(k_scan2_spine, dim3(1), dim3(kScanBlock), 0, work_stream(idx), (Scan2*)ts, ntiles, var_begin + n, car_base + n, host_totals);
  if (ntiles) hipLaunchKernelGGL(k_scan2_apply, dim3((unsigned)ntiles), dim3(kScanBlock), 0, work_stream(idx), nvar, ncar, n, (const Scan2*)ts, var_begin, car_base);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}

static void release_bufs(vs_index* idx, std::vector<DevBuf>& bufs) {
  for (auto& b : bufs) idx->pool.push_back(b);
  bufs.clear();
  // keep the pool bounded: drop the smallest buffers beyond kPoolEntries.  (hipFree waits for the whole device: the bound
  // has to sit well above what a loop of batches in flight cycles through -- a type-6 batch that returned when it was
  // enqueued holds ~20 buffers until it is freed, two of them are alive at a time, and buffers of other batch shapes stay
  // around -- or every step frees and re-allocates its small buffers and stalls on the expansion in flight: 64 entries
  // made the bench loop take 2.1 ms per step instead of 0.61 on some runs.)
  constexpr size_t kPoolEntries = 320;
  if (idx->pool.size() > kPoolEntries) (void)server_stop(idx);
  while (idx->pool.size() > kPoolEntries) {
    size_t k = 0;
    for (size_t i = 1; i < idx->pool.size(); ++i)
      if (idx->pool[i].cap < idx->pool[k].cap) k = i;
    (void)hipFree(idx->pool[k].p);
    idx->pool_frees++;
    idx->pool.erase(idx->pool.begin() + k);
  }
}

// Page-locked host memory for raw result copies: allocating it costs as much as copying into it, so buffers go back to a
// small per-handle pool when their result is freed.
static int pin_alloc(vs_index* idx, size_t bytes, DevBuf* out) {
  bytes = (bytes + 4095) & ~(size_t)4095;
  int best = -1;
  for (size_t i = 0; i < idx->pin_pool.size(); ++i)
    if (idx->pin_pool[i].cap >= bytes && (best < 0 || idx->pin_pool[i].cap < idx->pin_pool[best].cap)) best = (int)i;
  if (best >= 0) { *out = idx->pin_pool[best]; idx->pin_pool.erase(idx->pin_pool.begin() + best); return VS_OK; }
  void* p = nullptr;
  HIP_TRY(hipHostMalloc(&p, bytes, hipHostMallocDefault));
  *out = DevBuf{p, bytes};
  return VS_OK;
}
static void pin_release(vs_index* idx, DevBuf b) {
  if (!b.p) return;
  idx->pin_pool.push_back(b);
  while (idx->pin_pool.size() > 4) {   // keep the largest few
    size_t k = 0;
    for (size_t i = 1; i < idx->pin_pool.size(); ++i)
      if (idx->pin_pool[i].cap < idx->pin_pool[k].cap) k = i;
    (void)hipHostFree(idx->pin_pool[k].p);
    idx->pin_pool.erase(idx->pin_pool.begin() + k);
  }
}

// Temporaries of one call.  Every early return (VS_TRY / HIP_TRY) runs the destructor: the stream is drained first
// -- queued kernels may still be using the buffers -- and then they go back to the pool, so a failing call on a
// long-lived handle neither leaks HBM nor recycles memory that is still in flight.  The success path calls
// release() itself after its own synchronisation.
struct ScratchBufs {
  vs_index* idx;
  std::vector<DevBuf> bufs;
  explicit ScratchBufs(vs_index* i) : idx(i) {}
  ScratchBufs(const ScratchBufs&) = delete;
  ScratchBufs& operator=(const ScratchBufs&) = delete;
  void release() { release_bufs(idx, bufs); }
  void hand_to(std::vector<DevBuf>& owner) { owner.insert(owner.end(), bufs.begin(), bufs.end()); bufs.clear(); }   // (a result that outlives the call)
  ~ScratchBufs() {
    if (bufs.empty()) return;
    if (idx->plan_stream) (void)hipStreamSynchronize(idx->plan_stream);
    if (idx->stream) (void)hipStreamSynchronize(idx->stream);
    release_bufs(idx, bufs);
  }
};

// ----------------------------------------------------------- image on device
// ---- event bitmaps of query type 4: one row of P bits per sample (3 GB for 2504 samples x 9.6 M ref-path slots; HBM is
//      what this part has plenty of).  Skipped when they would take more than half of the free memory or `cap` bytes; dropped
//      and rebuilt on an open handle by option t4_rows_max_mb (several handles on one GPU: the caller decides who gets them --
//      without the rows type 4 walks one lane per region). ----
static void free_image_alloc(vs_index* idx, const void* p) {
  if (!p) return;
  auto it = std::find(idx->image_allocs.begin(), idx->image_allocs.end(), const_cast<void*>(p));
  if (it != idx->image_allocs.end()) idx->image_allocs.erase(it);
  (void)hipFree(const_cast<void*>(p));
}
constexpr uint32_t kHintShrinkAfter = 8;
static void hint_after_batch(vs_index* idx, int which, uint64_t& hint, uint64_t cap_seen) {
  if (cap_seen >= hint / 4) { idx->hint_small_runs[which] = 0; idx->hint_small_max[which] = 0; return; }
  idx->hint_small_max[which] = std::max(idx->hint_small_max[which], cap_seen);
  if (++idx->hint_small_runs[which] >= kHintShrinkAfter) {
    const uint64_t m = idx->hint_small_max[which];
    hint = m + m / 8 + 1024;
    idx->hint_small_runs[which] = 0; idx->hint_small_max[which] = 0;
  }
}
static int drop_t4_rows(vs_index* idx) {
  DevImage& d = idx->d;
  if (!d.t4_events) return VS_OK;
  HIP_TRY(hipDeviceSynchronize());   // (batches that returned when they were enqueued may still be walking over the rows)
  free_image_alloc(idx, d.t4_events); free_image_alloc(idx, d.t4_hold); free_image_alloc(idx, d.t4_irr);
  idx->device_bytes -= idx->t4_alloc_bytes;
  idx->t4_alloc_bytes = 0; idx->t4_rows_bytes = 0;
  d.t4_events = nullptr; d.t4_stride = 0; d.t4_hold = nullptr; d.t4_hold_stride = 0; d.t4_irr = nullptr; d.t4_ev_shift = 0; d.t4_irr_reach = 1;
  return VS_OK;
}
static int build_t4_rows(vs_index* idx, uint64_t cap) {
  const HostImage& im = idx->im;
  DevImage& d = idx->d;
  if (d.t4_events) return VS_OK;
  if (im.slots_follow_ranks && im.P && d.num_samples > 1) {
    // Class-row cohorts: a bit per slot and sample, a bit per vertex and sample (3.0 + 4.6 GB at 2504 samples).  Explicit-id
    // cohorts (thousands of samples, a handful of carriers per variant): one bit per EIGHT slots -- any superset of the
    // events is exact, a coarse bit costs a few literal steps where the sample does have an event, and those are rare -- and
    // no hold rows at all: "does v hold the sample" is read from v's carrier list (k_walk.hip.h: BitRow).  10,000 samples x
    // 20 M variants: 6.3 GB instead of round 3's 125 GB.
    const uint64_t istride = (im.P + 63) / 64 + 1;                                   // the global irregular row: a bit per slot
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    // Round 6, opt-in (VS_T4_EXACT_ROWS=1 when the handle is opened): an explicit-id cohort takes the EXACT rows too when they fit the
    // budget (10,000 samples x 20 M variants: 48 + 73 GB of the part's 288): hold tests become one bit, the spill-free type-4 walk and the
    // cooperative kernels of types 2 / 3 / 5 apply.  Measured on that cohort: type 4 160 -> 172 M regions/s, types 2 / 3 / 5 unchanged
    // (82 / 83 / 101 -> 84 / 84 / 109) for 116 GB more image -- not the default.
    const uint64_t exact_bytes = (uint64_t)d.num_samples * (istride + (im.V + 63) / 64 + 1) * 8;
    const bool exact = d.use_bv || (idx->opts.t4_exact_rows && exact_bytes <= cap && exact_bytes <= free_b / 2);
    const uint32_t shift = exact ? 0u : 3u;
    const uint64_t stride = exact ? istride : ((im.P >> shift) + 64) / 64 + 1, hstride = exact ? (im.V + 63) / 64 + 1 : 0;
    const uint64_t bytes = (uint64_t)d.num_samples * stride * 8, hbytes = (uint64_t)d.num_samples * hstride * 8;
    if (bytes + hbytes <= cap && bytes + hbytes <= free_b / 2) {
      const uint64_t bytes_before = idx->device_bytes;
      uint64_t *events = nullptr, *hold = nullptr, *irr = nullptr;
      // every allocation and launch first, the handle's fields last: a failure half way (the check against the free memory is not atomic with
      // the allocations) gives back what it took and leaves the handle without rows, as if none had been asked for
      auto build = [&]() -> int {
        VS_TRY(alloc_image(idx, (size_t)istride, &irr));
        HIP_TRY(hipMemsetAsync(irr, 0, istride * 8, idx->stream));
        VS_TRY(alloc_image(idx, (size_t)d.num_samples * stride, &events));
        HIP_TRY(hipMemsetAsync(events, 0, bytes, idx->stream));
        if (hstride) {
          VS_TRY(alloc_image(idx, (size_t)d.num_samples * hstride, &hold));
          HIP_TRY(hipMemsetAsync(hold, 0, hbytes, idx->stream));
        }
        DevImage dd = d;   // (the build kernels read the strides from their copy of the image)
        dd.t4_stride = stride; dd.t4_hold_stride = hstride; dd.t4_ev_shift = shift;
        const unsigned tiles = (unsigned)((im.P + 63) / 64), vtiles = (unsigned)((im.V + 63) / 64);
        if (d.use_bv) {
          hipLaunchKernelGGL(k_build_events, dim3((tiles + 3) / 4), dim3(256), 0, idx->stream, dd, events, irr);
          hipLaunchKernelGGL(k_build_hold, dim3((vtiles + 3) / 4), dim3(256), 0, idx->stream, dd, hold);
        } else {
          hipLaunchKernelGGL(k_events_irregular_rows, dim3((tiles + 3) / 4), dim3(256), 0, idx->stream, dd, irr);
          hipLaunchKernelGGL(k_events_explicit, dim3((unsigned)((im.P + 255) / 256)), dim3(256), 0, idx->stream, dd, events);
          if (hstride) hipLaunchKernelGGL(k_hold_explicit, dim3((unsigned)((im.V + 255) / 256)), dim3(256), 0, idx->stream, dd, hold);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(idx->stream));
        return VS_OK;
      };
      const int rc = build();
      if (rc != VS_OK) {
        (void)hipStreamSynchronize(idx->stream);
        free_image_alloc(idx, events); free_image_alloc(idx, hold); free_image_alloc(idx, irr);
        idx->device_bytes = bytes_before;
        return rc;
      }
      d.t4_stride = stride; d.t4_hold_stride = hstride; d.t4_ev_shift = shift;
      d.t4_events = events; d.t4_hold = hold; d.t4_irr = irr; d.t4_irr_reach = im.irr_reach;
      idx->t4_rows_bytes = bytes + hbytes;
      idx->t4_alloc_bytes = idx->device_bytes - bytes_before;
    }
  }
  HIP_TRY(hipStreamSynchronize(idx->stream));
  return VS_OK;
}

static int build_device_image(vs_index* idx) {
  HostImage& im = idx->im;
  DevImage& d = idx->d;
  HIP_TRY(hipSetDevice(idx->device));
  HIP_TRY(hipStreamCreate(&idx->stream));
  for (auto& e : idx->ev) HIP_TRY(hipEventCreate(&e));
  HIP_TRY(hipHostMalloc((void**)&idx->pinned, 16384, hipHostMallocCoherent | hipHostMallocMapped));
  memset(idx->pinned, 0, 16384);
  HIP_TRY(hipMalloc((void**)&idx->done_counter, 32));   // [0] blocks finished, [1..3] device time stamps of the latency kernel
  idx->image_allocs.push_back(idx->done_counter);
  HIP_TRY(hipMemsetAsync(idx->done_counter, 0, 32, idx->stream));
  d.ref_length = im.ref_length;
  d.nbits = (uint64_t)im.bits.size() * 64;
  d.num_samples = im.num_samples; d.wpc = im.wpc; d.use_bv = im.use_bit_vector;
  d.V = im.V; d.E = im.E; d.P = im.P; d.R = im.R; d.C = im.C;
  d.G = im.rp_cand_prefix[im.P];
  VS_TRY(upload_image(idx, im.bits, &d.bits));
  VS_TRY(upload_image(idx, im.blk_rank, &d.blk_rank));
  VS_TRY(upload_image(idx, im.idx_pos, &d.idx_pos));
  VS_TRY(upload_image(idx, im.rank_to_slot, &d.rank_to_slot));
  VS_TRY(upload_image(idx, im.rp_vid, &d.rp_vid));
  VS_TRY(upload_image(idx, im.rp_cand_prefix, &d.rp_cand_prefix));
  VS_TRY(upload_image(idx, im.row_ptr, &d.row_ptr));
  VS_TRY(upload_image(idx, im.col, &d.col));
  VS_TRY(upload_image(idx, im.v_off, &d.v_off));
  VS_TRY(upload_image(idx, im.v_len, &d.v_len));
  VS_TRY(upload_image(idx, im.v_ridx, &d.v_ridx));
  VS_TRY(upload_image(idx, im.v_class, &d.v_class));
  VS_TRY(upload_image(idx, im.v_src, &d.v_src));
  {
    const uint32_t *wv = nullptr, *we = nullptr;
    VS_TRY(upload_image(idx, im.w_vertex, &wv));
    VS_TRY(upload_image(idx, im.w_edge, &we));
    d.w_vertex = reinterpret_cast<const uint4*>(wv);
    d.w_edge = reinterpret_cast<const uint4*>(we);
    const uint32_t *wb = nullptr, *rb = nullptr;
    VS_TRY(upload_image(idx, im.wblob, &wb));
    VS_TRY(upload_image(idx, im.blob_of_slot, &d.blob_of_slot));
    VS_TRY(upload_image(idx, im.blob_row, &d.blob_row));
    VS_TRY(upload_image(idx, im.rk_back, &rb));
    VS_TRY(upload_image(idx, im.seq_breaks, &d.seq_breaks));
    const uint32_t* ra = nullptr;
    VS_TRY(upload_image(idx, im.rk_anc, &ra));
    d.rk_anc = reinterpret_cast<const uint2*>(ra);
    VS_TRY(upload_image(idx, im.slot_rank, &d.slot_rank));
    d.wblob = reinterpret_cast<const uint4*>(wb);
    d.rk_back = reinterpret_cast<const uint2*>(rb);
  }
  VS_TRY(upload_image(idx, im.v_ncar, &d.v_ncar));
  VS_TRY(upload_image(idx, im.v_nri, &d.v_nri));
  VS_TRY(upload_image(idx, im.v_car_begin, &d.v_car_begin));
  VS_TRY(upload_image(idx, im.class_rows, &d.class_rows));
  VS_TRY(upload_image(idx, im.cls_list_begin, &d.cls_list_begin));
  VS_TRY(upload_image(idx, im.cls_list_ids, &d.cls_list_ids));
  VS_TRY(upload_image(idx, im.cls_list16, &d.cls_list16));
  d.list_max = im.list_max;
  VS_TRY(upload_image(idx, im.gt_nibbles, &d.gt_nibbles));
  VS_TRY(upload_image(idx, im.gt_groups, &d.gt_groups));
  VS_TRY(upload_image(idx, im.car_sid, &d.car_sid));
  VS_TRY(upload_image(idx, im.car_index, &d.car_index));
  d.has_car_index = im.car_index.empty() ? 0u : 1u;
  d.class_cum = nullptr;
  if (d.has_car_index && d.use_bv && im.wpc && im.num_samples < 65536) {   // rank of a sample's bit in its class row without a pass over the row
    const uint64_t n_rows = im.class_rows.size() / im.wpc;
    uint16_t* cum = nullptr;
    VS_TRY(alloc_image(idx, n_rows * im.wpc, &cum));
    if (n_rows) hipLaunchKernelGGL(k_class_cum, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, idx->stream, d.class_rows, n_rows, (uint32_t)im.wpc, cum);
    HIP_TRY(hipGetLastError());
    d.class_cum = cum;
  }
  VS_TRY(upload_image(idx, im.seq_codes, &d.seq_codes));
  const uint64_t G = d.G;
  VS_TRY(alloc_image(idx, G, &d.s_pos));
  VS_TRY(alloc_image(idx, G, &d.s_ref_off));
  VS_TRY(alloc_image(idx, G, &d.s_ref_len));
  VS_TRY(alloc_image(idx, G, &d.s_alt_off));
  VS_TRY(alloc_image(idx, G, &d.s_alt_len));
  VS_TRY(alloc_image(idx, G, &d.s_vid));
  VS_TRY(alloc_image(idx, G, &d.s_ncar));
  VS_TRY(alloc_image(idx, G, &d.s_flags));
  VS_TRY(alloc_image(idx, G, &d.s_dup_prev));
  VS_TRY(alloc_image(idx, G + 1, &d.s_carpre));
  VS_TRY(alloc_image(idx, G + 1, &d.s_kpre));
  VS_TRY(alloc_image(idx, G, &d.s_class));
  VS_TRY(alloc_image(idx, G, &d.s_gt0));
  d.sus_g = nullptr; d.sus_prev = nullptr; d.n_sus = 0;

  // site table: the reference's per-node classification, once for the whole ref path
  if (im.P) {
    const uint64_t chunk = 1ull << 24;
    for (uint64_t s = 0; s < im.P; s += chunk) {
      uint64_t e = std::min<uint64_t>(im.P, s + chunk);
      hipLaunchKernelGGL(k_build_sites, dim3((unsigned)((e - s + 255) / 256)), dim3(256), 0, idx->stream, d, s, e);
    }
    HIP_TRY(hipGetLastError());
  }
  ScratchBufs scratch(idx);
  {  // arena offsets: prefix of the counts rounded up to the carrier alignment (kernels.hip.h: pad_car)
    void* padded = nullptr;
    VS_TRY(dev_alloc(idx, (G + 1) * 4, &padded, &scratch.bufs));
    if (G) hipLaunchKernelGGL(k_pad_counts, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, idx->stream, (const uint32_t*)d.s_ncar, (uint32_t*)padded, G);
    VS_TRY(exclusive_scan<uint32_t>(idx, (const uint32_t*)padded, G, d.s_carpre, &scratch.bufs));
    VS_TRY(exclusive_scan<uint32_t>(idx, (const uint32_t*)d.s_ncar, G, d.s_kpre, &scratch.bufs));
    {
      uint64_t *rc = nullptr, *rk = nullptr;
      VS_TRY(alloc_image(idx, im.P + 1, &rc));
      VS_TRY(alloc_image(idx, im.P + 1, &rk));
      hipLaunchKernelGGL(k_slot_prefixes, dim3((unsigned)((im.P + 256) / 256)), dim3(256), 0, idx->stream, d, rc, rk);
      HIP_TRY(hipGetLastError());
      d.rp_carpre = rc; d.rp_kpre = rk;
    }
    {
      VariantRow* rows = nullptr;
      VS_TRY(alloc_image(idx, G, &rows));
      if (G) hipLaunchKernelGGL(k_build_site_rows, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, idx->stream, d, rows);
      HIP_TRY(hipGetLastError());
      d.s_row = rows;
    }
    idx->h_carpre.resize(G + 1);
    HIP_TRY(hipMemcpyAsync(idx->h_carpre.data(), d.s_carpre, (G + 1) * 8, hipMemcpyDeviceToHost, idx->stream));
  }
  std::vector<uint32_t> h_dup(G), h_fl(G), h_ncar(G);
  if (G) {
    hipLaunchKernelGGL(k_mark_dups, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, idx->stream, d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_dup.data(), d.s_dup_prev, G * 4, hipMemcpyDeviceToHost, idx->stream));
    HIP_TRY(hipMemcpyAsync(h_fl.data(), d.s_flags, G * 4, hipMemcpyDeviceToHost, idx->stream));
    HIP_TRY(hipMemcpyAsync(h_ncar.data(), d.s_ncar, G * 4, hipMemcpyDeviceToHost, idx->stream));
  }
  HIP_TRY(hipStreamSynchronize(idx->stream));
  scratch.release();
  {  // the dense sites (k_fill_dense)
    std::vector<uint32_t> dense;
    if (d.use_bv)
      for (uint64_t g = 0; g < G; ++g)
        if (h_ncar[g] > d.list_max) dense.push_back((uint32_t)g);
    d.n_dense = dense.size();
    VS_TRY(upload_image(idx, dense, &d.dense_site));
  }
  std::vector<uint32_t> sus_g, sus_prev;
  for (uint64_t g = 0; g < G; ++g) {
    if (h_fl[g] & kSiteAlwaysDrop) { sus_g.push_back((uint32_t)g); sus_prev.push_back(kNone); }
    else if (h_dup[g] != kNone) { sus_g.push_back((uint32_t)g); sus_prev.push_back(h_dup[g]); }
  }
  d.n_sus = (uint32_t)sus_g.size();
  {  // suspicious sites before each ref-path slot's first site
    std::vector<uint32_t> pre(im.P + 1, 0);
    size_t k = 0;
    for (uint64_t s = 0; s <= im.P; ++s) {
      while (k < sus_g.size() && sus_g[k] < im.rp_cand_prefix[s]) ++k;
      pre[s] = (uint32_t)k;
    }
    VS_TRY(upload_image(idx, pre, &d.rp_sus_prefix));
  }
  {  // the bounds' per-slot and per-rank records
    uint4* rp = nullptr; uint2* rk = nullptr;
    VS_TRY(alloc_image(idx, 2 * (im.P + 1), &rp));
    VS_TRY(alloc_image(idx, im.R + 1, &rk));
    hipLaunchKernelGGL(k_slot_records, dim3((unsigned)((im.P + 256) / 256)), dim3(256), 0, idx->stream, d, rp);
    hipLaunchKernelGGL(k_rank_records, dim3((unsigned)((im.R + 256) / 256)), dim3(256), 0, idx->stream, d, rk);
    HIP_TRY(hipGetLastError());
    d.rp_rec = rp; d.rk_rec = rk;
  }
  VS_TRY(upload_image(idx, sus_g, &d.sus_g));
  VS_TRY(upload_image(idx, sus_prev, &d.sus_prev));
  // ---- the per-sample rows of query type 4 (build_t4_rows below) ----
  d.t4_events = nullptr; d.t4_stride = 0; d.t4_hold = nullptr; d.t4_hold_stride = 0; d.t4_irr = nullptr; d.t4_ev_shift = 0; d.t4_irr_reach = 1;
  if (!idx->opts.no_t4_events) {
    // Budget: half of the free memory, at most 176 GB -- or VS_T4_ROWS_MAX_GB from the environment, or option t4_rows_max_mb
    // on the open handle; vs_index_get_info reports what was taken (t4_rows_bytes).
    uint64_t cap = 176ull << 30;
    if (const char* gb = getenv("VS_T4_ROWS_MAX_GB")) cap = (uint64_t)(std::max(0.0, atof(gb)) * (double)(1ull << 30));
    VS_TRY(build_t4_rows(idx, cap));
  }
  HIP_TRY(hipStreamSynchronize(idx->stream));
  return VS_OK;
}

// The environment switches of DESIGN.md section 7a, read once per handle.
static void read_env_opts(vs_index* idx) {
  EngineOpts& o = idx->opts;
  if (getenv("VS_NO_SERVER")) o.server = 0;
  else if (const char* sv = getenv("VS_SERVER")) o.server = std::max(0, std::min(2, atoi(sv)));
  if (const char* sb = getenv("VS_SRV_BLOCKS")) o.srv_blocks = (unsigned)std::max(1, std::min(64, atoi(sb)));
  if (getenv("VS_NO_SHARED_LISTS")) o.share_lists = false;
  o.async_fill = getenv("VS_ASYNC_FILL") != nullptr;
  if (getenv("VS_SYNC_SUBMIT")) o.async_submit = false;
  o.resident_lists = getenv("VS_RESIDENT_LISTS") != nullptr;   // (the arena itself is built at the end of finish_open)
  o.no_t4_events = getenv("VS_T4_NO_EVENTS") != nullptr;
  o.t4_exact_rows = getenv("VS_T4_EXACT_ROWS") != nullptr;
  if (const char* pp = getenv("VS_PLAN_STREAM_PRIORITY")) o.plan_stream_priority = !strcmp(pp, "high") ? 1 : (!strcmp(pp, "low") ? -1 : 0);
  if (const char* pi = getenv("VS_PLAN_ITEMS")) o.plan_items = (uint32_t)std::max(1, std::min(64, atoi(pi)));
  if (const char* lm = getenv("VS_LIST_MAX")) idx->im.list_max = (uint32_t)atoi(lm);   // tuning aid (default: kListMaxDefault)
#ifdef VS_TUNING
  o.lat_debug = getenv("VS_LAT_DEBUG") != nullptr;
#endif
}

static int build_resident_lists(vs_index* idx);
static int finish_open(vs_index* idx, int device) {
  try {
    read_env_opts(idx);
    build_host_image(idx->g, idx->im);
  } catch (const std::exception& e) {
    return fail(VS_ERR_FORMAT, "%s", e.what());
  }
  idx->seq_chars.resize(idx->g.seq.size());
  for (size_t i = 0; i < idx->g.seq.size(); ++i) idx->seq_chars[i] = map_int(idx->g.seq[i]);
  for (uint32_t i = 0; i < idx->g.sample_names.size(); ++i) idx->sample_ids.emplace(idx->g.sample_names[i], i);
  idx->device = device;
  if (device < 0) return VS_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VS_ERR_NO_DEVICE, "no HIP device is visible");
  if (device >= ndev) return fail(VS_ERR_NO_DEVICE, "device %d requested, %d visible", device, ndev);
  VS_TRY(build_device_image(idx));
  if (idx->opts.resident_lists) {   // VS_RESIDENT_LISTS: over budget is not an error at open, the lists are then expanded per batch
    idx->opts.resident_lists = false;
    if (build_resident_lists(idx) == VS_OK) idx->opts.resident_lists = true;
  }
  return VS_OK;
}

template <typename T>
static int ralloc(vs_result* r, size_t n, T** p) {
  void* q = nullptr;
  VS_TRY(dev_alloc(r->idx, n * sizeof(T), &q, &r->bufs));
  *p = (T*)q;
  return VS_OK;
}

// Several arrays out of ONE pooled buffer (every allocation is a search of the handle's pool, and a batch of a tenth of a
// millisecond makes sixteen of them): want() registers an array -- its pointer, its elements -- and adds up the sizes, the buffer of
// `bytes` is taken once into `base`, carve() then points every registered array into it, in that order, on 256-byte bounds.
struct Slab {
  struct Part { void* ptr; size_t off; void (*set)(void* ptr, uint8_t* at); };
  size_t bytes = 0;
  uint8_t* base = nullptr;
  Part parts[16];   // (a shared batch registers twelve)
  int n_parts = 0;
  template <typename T> void want(T*& p, size_t count) {
    parts[n_parts++] = Part{&p, bytes, [](void* ptr, uint8_t* at) { *static_cast<T**>(ptr) = reinterpret_cast<T*>(at); }};
    bytes += (count * sizeof(T) + 255) & ~(size_t)255;
  }
  void carve() const { for (int i = 0; i < n_parts; ++i) parts[i].set(parts[i].ptr, base + parts[i].off); }
};

// Strings of a type-7 batch (ref, alt per query) as one byte pool + [2n+1] offsets.
struct PointStrings {
  const std::vector<uint8_t>* chars;
  const std::vector<uint64_t>* off;
};

// Fill-kernel launch shared by every path: LDS per wave from the cohort width, WIDE from the row width.
static uint32_t fill_gt_words(const vs_index* idx) {
  uint32_t gt_words = ((std::min<uint32_t>(idx->d.num_samples, 4064) + 32 + 255) / 256) * 64;
  return gt_words < 448 ? 448 : gt_words;   // the medium path keeps 640 ids at word 256..
}
static size_t fill_lds_bytes(const vs_index* idx) {
  return 4 * (size_t)(idx->d.wpc <= 63 ? slice_lds_words(idx->d.num_samples) : fill_gt_words(idx) + kRingWords) * 4;
}

// one launch of the carrier expansion: over the rows of a private-row result or over the shared rows of a sorted batch
template <bool WIDE, uint32_t CH, bool TUNE>
static void launch_fill(vs_index* idx, const DevResult& d, bool share, const uint32_t* u_site, uint64_t n_fill, unsigned blocks, size_t lds_bytes,
                        uint32_t ablate, uint32_t gt_words, hipStream_t stream = nullptr) {
  if (!stream) stream = idx->stream;
  if (share) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fill_sites<WIDE, CH, TUNE>), dim3(blocks), dim3(256), lds_bytes, stream, idx->d, d, u_site, n_fill, ablate, gt_words);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fill_carriers<WIDE, CH, TUNE>), dim3(blocks), dim3(256), lds_bytes, stream, idx->d, d, ablate, gt_words);
}

static int ensure_fill_stream(vs_index* idx) {
  if (idx->fill_stream) return VS_OK;
  HIP_TRY(hipStreamCreateWithFlags(&idx->fill_stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&idx->fill_ev[0], hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&idx->fill_ev[1], hipEventDisableTiming));
  return VS_OK;
}
static int result_events(vs_result* r) {   // the result's own pair of timing events around its expansion, from the handle's pool
  vs_index* idx = r->idx;
  for (auto& e : r->ev_fill) {
    if (e) continue;
    if (!idx->ev_pool.empty()) { e = idx->ev_pool.back(); idx->ev_pool.pop_back(); }
    else HIP_TRY(hipEventCreate(&e));
  }
  return VS_OK;
}
static int pooled_event(vs_index* idx, hipEvent_t* e) {
  if (*e) return VS_OK;
  if (!idx->ev_pool.empty()) { *e = idx->ev_pool.back(); idx->ev_pool.pop_back(); return VS_OK; }
  HIP_TRY(hipEventCreate(e));
  return VS_OK;
}
static int ensure_plan_stream(vs_index* idx) {
  if (idx->plan_stream) return VS_OK;
  // (stream priorities, lowest and highest, were measured: the expansion beside a plan takes 0.031 ms longer than alone
  //  whatever the plan's priority -- the plan's 137 MB of scattered lines are what it shares, not wave slots)
  if (idx->opts.plan_stream_priority) {   // (tuning aid, VS_PLAN_STREAM_PRIORITY = high | low when the handle is opened)
    int lo = 0, hi = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));   // (numerically: hi <= lo)
    HIP_TRY(hipStreamCreateWithPriority(&idx->plan_stream, hipStreamNonBlocking, idx->opts.plan_stream_priority > 0 ? hi : lo));
    return VS_OK;
  }
  HIP_TRY(hipStreamCreateWithFlags(&idx->plan_stream, hipStreamNonBlocking));
  return VS_OK;
}
// Regions and sample ids of the walking query types may be handed over in device memory (the copies below are
// hipMemcpyDefault: the runtime reads the direction off the pointers).
static bool is_device_ptr(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // (plain host memory: not known to the runtime)
  return a.type == hipMemoryTypeDevice;
}
// The phase times of a batch from the handle's events (the batch's last event has completed or is waited for here).
static int collect_timing(vs_index* idx) {
  if (!idx->timing_pending) return VS_OK;
  idx->timing_pending = false;
  vs_timing& t = idx->timing;
  hipEvent_t* e = idx->timing_owner ? idx->tev : idx->ev;
  idx->timing_owner = nullptr;
  HIP_TRY(hipEventSynchronize(e[4]));
  HIP_TRY(hipEventElapsedTime(&t.ms_total, e[0], e[4]));
  if (idx->timing_total_only) {   // (a sequence batch records its first and last event only)
    idx->timing_total_only = false;
    t.ms_bounds = t.ms_scan = t.ms_emit = t.ms_fill = 0.f;
    t.fill_launches = 0;
    return VS_OK;
  }
  HIP_TRY(hipEventElapsedTime(&t.ms_bounds, e[0], e[1]));
  HIP_TRY(hipEventElapsedTime(&t.ms_scan, e[1], e[2]));
  HIP_TRY(hipEventElapsedTime(&t.ms_emit, e[2], e[3]));
  HIP_TRY(hipEventElapsedTime(&t.ms_fill, e[3], e[4]));
  t.fill_launches = idx->timing_fill_launches;
  return VS_OK;
}
// An asynchronous expansion (option "async_fill") must have finished before anything reads the result or returns its
// buffers to the pool.
static int result_ready(vs_result* r) {
  if (!r->pending) return VS_OK;
  r->pending = false;
  if (r->ev_done) HIP_TRY(hipEventSynchronize(r->ev_done));
  if (r->ev_fill[1]) {
    HIP_TRY(hipEventSynchronize(r->ev_fill[1]));
    HIP_TRY(hipEventElapsedTime(&r->fill_ms, r->ev_fill[0], r->ev_fill[1]));
  }
  release_bufs(r->idx, r->call_temps);   // (the batch has finished: nothing in flight reads them, the result never does)
  return VS_OK;
}

// Every throughput batch starts here: a throughput batch does not share the GPU with a polling server, and the handle's timing
// state is this batch's from now on (an earlier lean batch's event pair is not).
static int begin_batch(vs_index* idx) {
  if (idx->srv_alive) VS_TRY(server_stop(idx));
  idx->timing_pending = false; idx->timing_owner = nullptr; idx->timing_total_only = false;
  return VS_OK;
}
// A batch that returns ENQUEUED (async_submit): everything that reads the result is ordered behind it on the handle's stream, and
// the call's temporaries stay with the result until its completion event (vs_result_free, result_ready) -- a buffer in the pool is
// never referenced by work in flight, whatever stream takes it next.  record_done = false: the caller's last event is the batch's
// completion already (a lean type-6 batch's last kernel is its expansion: the result's own event behind that is it).
static int batch_enqueued(vs_result* r, ScratchBufs& scratch, bool record_done = true) {
  vs_index* idx = r->idx;
  if (record_done) {
    VS_TRY(pooled_event(idx, &r->ev_done));
    HIP_TRY(hipEventRecord(r->ev_done, idx->stream));
  }
  r->pending = true;
  idx->batch_in_flight = true;
  scratch.hand_to(r->bufs);
  return VS_OK;
}

// The carrier expansion of one result (or of the resident arena): one launch over n_fill rows.
static int fill_lists(vs_index* idx, const DevResult& d, bool share, const uint32_t* u_site, uint64_t n_fill, hipStream_t on = nullptr) {
  if (n_fill) {
    {
      // one task per wave, no grid-stride loop: task costs vary tenfold with the number of dense variants, and the
      // hardware's block scheduler balances that better than a static round-robin (8192-block grid: +8 % kernel time).
      // A task is 64 consecutive slots; batches of few, carrier-heavy variants (a type-4 batch: ~1 M variants of ~1300
      // carriers) take 16-slot tasks -- 17 k tasks of 64 would be two rounds of waves with a long tail.
      uint32_t chunk = idx->opts.fill_chunk;
      // (8-slot tasks for the carrier-heavy shape: 0.36 ms against 0.40 with 16 on the bench's type-4 leg, tools/run_t4.py)
      if (chunk == 0) chunk = share ? 16 : ((n_fill < 64ull * 8192 * 8 && d.S / n_fill >= 256) ? 8 : 64);
      const uint64_t nchunks = (n_fill + chunk - 1) / chunk;
      const uint64_t blocks = (nchunks + 3) / 4;
      if (blocks > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu variant slots)", (unsigned long long)d.A);
      // per-wave LDS: one genotype byte per carrier of the widest variant the staged paths take, plus the ring
      const uint32_t gt_words = fill_gt_words(idx);
#ifdef VS_TUNING   // tuning builds: one regime of the kernel can be skipped, the LDS block padded (tools/exp_fill.py)
      const size_t lds_bytes = fill_lds_bytes(idx) + std::min<size_t>(idx->opts.fill_lds_pad, 96 << 10);
      const uint32_t ablate = idx->opts.fill_ablate;
      constexpr bool kTune = true;
#else
      const size_t lds_bytes = fill_lds_bytes(idx);
      const uint32_t ablate = 0;
      constexpr bool kTune = false;
#endif
      const bool wide = idx->d.wpc > 63;
      switch (chunk) {
        case 8:  wide ? launch_fill<true, 8, kTune>(idx, d, share, u_site, n_fill, (unsigned)blocks, lds_bytes, ablate, gt_words, on)
                      : launch_fill<false, 8, kTune>(idx, d, share, u_site, n_fill, (unsigned)blocks, lds_bytes, ablate, gt_words, on); break;
        case 16: wide ? launch_fill<true, 16, kTune>(idx, d, share, u_site, n_fill, (unsigned)blocks, lds_bytes, ablate, gt_words, on)
                      : launch_fill<false, 16, kTune>(idx, d, share, u_site, n_fill, (unsigned)blocks, lds_bytes, ablate, gt_words, on); break;
        case 32: wide ? launch_fill<true, 32, kTune>(idx, d, share, u_site, n_fill, (unsigned)blocks, lds_bytes, ablate, gt_words, on)
                      : launch_fill<false, 32, kTune>(idx, d, share, u_site, n_fill, (unsigned)blocks, lds_bytes, ablate, gt_words, on); break;
        default: wide ? launch_fill<true, 64, kTune>(idx, d, share, u_site, n_fill, (unsigned)blocks, lds_bytes, ablate, gt_words, on)
                      : launch_fill<false, 64, kTune>(idx, d, share, u_site, n_fill, (unsigned)blocks, lds_bytes, ablate, gt_words, on); break;
      }
    }
    HIP_TRY(hipGetLastError());
  }
  return VS_OK;
}

// Resident carrier lists (option "resident_lists"): every carrier list a query can report is a function of the index
// alone -- a site's list is its vertex's -- so it can be expanded ONCE, with the kernel the queries would run, into an
// arena that stays with the handle: 2 (4) bytes per carrier record of HBM bought back as the whole expansion of every
// later batch, and as 9/10 of what a result sends across PCIe (rows only; the host keeps one mirror of the arena).
// Layout: the sites' lists in site-table order at s_carpre[g] -- a region's lists stay ONE range, everything downstream
// of car_base is unchanged -- followed by the lists of vertices that only the walking query types report (no site, or
// a site the reference never reports).
static int build_resident_lists(vs_index* idx) {
  if (idx->res_arena) return VS_OK;
  if (idx->device < 0) return fail(VS_ERR_NO_DEVICE, "index handle was opened without a device");
  HIP_TRY(hipSetDevice(idx->device));
  if (idx->srv_alive) VS_TRY(server_stop(idx));
  const HostImage& im = idx->im;
  const uint64_t G = idx->d.G, V = idx->d.V;
  std::vector<uint32_t> s_vid(G), s_ncar(G);
  if (G) {
    HIP_TRY(hipMemcpyAsync(s_vid.data(), idx->d.s_vid, G * 4, hipMemcpyDeviceToHost, idx->stream));
    HIP_TRY(hipMemcpyAsync(s_ncar.data(), idx->d.s_ncar, G * 4, hipMemcpyDeviceToHost, idx->stream));
    HIP_TRY(hipStreamSynchronize(idx->stream));
  }
  std::vector<uint64_t> v_abegin(V, ~0ull), x_begin;
  std::vector<uint32_t> x_vid;
  for (uint64_t g = 0; g < G; ++g) {
    const uint32_t v = s_vid[g];
    if (s_ncar[g] && s_ncar[g] == im.v_ncar[v] && v_abegin[v] == ~0ull) v_abegin[v] = idx->h_carpre[g];
  }
  uint64_t total = idx->h_carpre[G];
  idx->res_site_entries = total;
  for (uint64_t v = 0; v < V; ++v)
    if (im.v_ncar[v] && v_abegin[v] == ~0ull) {
      v_abegin[v] = total; x_vid.push_back((uint32_t)v); x_begin.push_back(total);
      total += pad_car(im.v_ncar[v]);
    }
  const uint64_t X = x_vid.size(), A = G + X;
  const uint32_t width = idx->d.wpc <= 63 ? 2 : 4;
  const uint64_t arena_bytes = total * width + 16, temp_bytes = A * (sizeof(VariantRow) + 12) + X * 12;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (arena_bytes + temp_bytes + V * 8 > free_b / 2)
    return fail(VS_ERR_UNSUPPORTED, "resident carrier lists need %.1f GB of HBM, %.1f GB are free", (arena_bytes + temp_bytes + V * 8) / 1e9, free_b / 1e9);
  void* arena = nullptr;
  HIP_TRY(hipMalloc(&arena, arena_bytes));
  idx->image_allocs.push_back(arena);
  const uint64_t* d_abegin = nullptr;
  VS_TRY(upload_image(idx, v_abegin, &d_abegin));
  if (A) {
    ScratchBufs tmp(idx);
    DevResult d{};
    uint32_t* dx_vid = nullptr; uint64_t* dx_begin = nullptr;
    VS_TRY(dev_alloc(idx, A * sizeof(VariantRow), (void**)&d.rows, &tmp.bufs));
    VS_TRY(dev_alloc(idx, A * 4, (void**)&d.r_class, &tmp.bufs));
    VS_TRY(dev_alloc(idx, A * 8, (void**)&d.r_gt0, &tmp.bufs));
    VS_TRY(dev_alloc(idx, X * 4, (void**)&dx_vid, &tmp.bufs));
    VS_TRY(dev_alloc(idx, X * 8, (void**)&dx_begin, &tmp.bufs));
    if (X) {
      HIP_TRY(hipMemcpyAsync(dx_vid, x_vid.data(), X * 4, hipMemcpyHostToDevice, idx->stream));
      HIP_TRY(hipMemcpyAsync(dx_begin, x_begin.data(), X * 8, hipMemcpyHostToDevice, idx->stream));
    }
    d.A = A; d.S = total; d.carriers = arena; d.car_width = width;
    hipLaunchKernelGGL(k_resident_params, dim3((unsigned)((A + 255) / 256)), dim3(256), 0, idx->stream, idx->d, (const uint32_t*)dx_vid, (const uint64_t*)dx_begin, X,
                       d.rows, d.r_class, d.r_gt0);
    HIP_TRY(hipGetLastError());
    VS_TRY(fill_lists(idx, d, false, nullptr, A));
    HIP_TRY(hipStreamSynchronize(idx->stream));
    tmp.release();
  }
  idx->device_bytes += arena_bytes;
  idx->d.v_abegin = d_abegin;
  idx->res_entries = total;
  idx->res_arena = arena;
  return VS_OK;
}
// the arena's host mirror: page-locked, copied over once, shared by the handle's results
static int ensure_resident_mirror(vs_index* idx) {
  if (idx->res_mirror) return VS_OK;
  const uint32_t width = idx->d.wpc <= 63 ? 2 : 4;
  void* p = nullptr;
  HIP_TRY(hipHostMalloc(&p, idx->res_entries * width + 16, hipHostMallocDefault));
  const hipError_t e = hipMemcpy(p, idx->res_arena, idx->res_entries * width, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { (void)hipHostFree(p); return fail(VS_ERR_HIP, "copy of the resident carrier lists failed: %s", hipGetErrorString(e)); }
  idx->res_mirror = p;
  return VS_OK;
}

// Spin on a word in mapped host memory until the device has posted `seq` (the runtime's completion wait costs tens of
// microseconds more); a kernel that never posts -- a fault -- is caught by the synchronisation after the deadline.
static int wait_posted(vs_index* idx, volatile uint64_t* word, uint64_t seq, int deadline_ms) {
  const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(deadline_ms);
  bool posted = false;
  uint32_t spins = 0;
  while (!(posted = (*word == seq))) {
    __builtin_ia32_pause();
    if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() > deadline) break;
  }
  if (!posted) {
    if (idx->plan_stream) HIP_TRY(hipStreamSynchronize(idx->plan_stream));
    HIP_TRY(hipStreamSynchronize(idx->stream));
    if (*word != seq) return fail(VS_ERR_INTERNAL, "a batch kernel finished without posting its sequence word");
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return VS_OK;
}

// Up to three 64-bit device words for the host, behind everything queued on the handle's stream: a one-thread kernel
// copies them into mapped host memory and posts a sequence word the host spins on (a staged hipMemcpyAsync into pageable
// memory + hipStreamSynchronize costs 20 - 30 us more, and the walking query types do it two or three times per batch).
static int read_device_words(vs_index* idx, const uint64_t* a, uint64_t* va, const uint64_t* b = nullptr, uint64_t* vb = nullptr,
                             const uint64_t* c = nullptr, uint64_t* vc = nullptr) {
  uint64_t* dst = idx->pinned + vs_index::kPinWords;
  const uint64_t seq = ++idx->done_seq;
  hipLaunchKernelGGL(k_post_words, dim3(1), dim3(1), 0, work_stream(idx), dst, a, b, c, seq);
  HIP_TRY(hipGetLastError());
  VS_TRY(wait_posted(idx, dst + 3, seq, 2000));
  if (!idx->pre) idx->batch_in_flight = false;   // (the handle's own stream has drained)
  if (va) *va = ((volatile uint64_t*)dst)[0];
  if (vb) *vb = ((volatile uint64_t*)dst)[1];
  if (vc) *vc = ((volatile uint64_t*)dst)[2];
  return VS_OK;
}

// ---- speculative type-6 batches: hints, the totals mailbox, the result's sizes on first use ----
static void t6_hint_update(vs_index* idx, uint64_t n, uint64_t rows, uint64_t arena) {
  const uint64_t need_rows = rows + rows / 8 + 1024, need_arena = arena + arena / 8 + 4096;
  idx->t6_hint_n = n;
  if (need_rows > idx->t6_hint_rows || need_arena > idx->t6_hint_arena || idx->t6_hint_rows == 0) {   // grows at once (both: they belong to one shape of batch)
    idx->t6_hint_rows = std::max(idx->t6_hint_rows, need_rows); idx->t6_hint_arena = std::max(idx->t6_hint_arena, need_arena);
    idx->t6_small_runs = 0; idx->t6_small_rows = idx->t6_small_arena = 0;
    return;
  }
  if (need_rows >= idx->t6_hint_rows / 2 && need_arena >= idx->t6_hint_arena / 2) { idx->t6_small_runs = 0; idx->t6_small_rows = idx->t6_small_arena = 0; return; }
  // shrinks after kHintShrinkAfter consecutive batches that needed less than half of it, to the largest of those
  idx->t6_small_rows = std::max(idx->t6_small_rows, need_rows); idx->t6_small_arena = std::max(idx->t6_small_arena, need_arena);
  if (++idx->t6_small_runs >= kHintShrinkAfter) {
    idx->t6_hint_rows = idx->t6_small_rows; idx->t6_hint_arena = idx->t6_small_arena;
    idx->t6_small_runs = 0; idx->t6_small_rows = idx->t6_small_arena = 0;
  }
}
// The totals of a speculative batch move from its mailbox into the result (and the handle's hints follow them).  The plan is four short
// kernels in front of everything else of the batch: by the time anybody asks, the word is there.
static int capture_totals(vs_result* r) {
  if (!r->sizes_pending || r->totals_captured) return VS_OK;
  vs_index* idx = r->idx;
  volatile PlanTotals* pt = reinterpret_cast<volatile PlanTotals*>(idx->pinned + vs_index::kPinPlanRing + (size_t)r->plan_slot * 8);
  VS_TRY(wait_posted(idx, &pt->seq, r->plan_seq, 2000));
  r->plan_copy.rows = pt->rows; r->plan_copy.arena = pt->arena; r->plan_copy.shared_rows = pt->shared_rows; r->plan_copy.not_sorted = pt->not_sorted;
  r->plan_copy.reported = pt->reported; r->plan_copy.n_slow = pt->n_slow; r->plan_copy.n_runs = pt->n_runs; r->plan_copy.seq = r->plan_seq;
  r->totals_captured = true;
  if (idx->plan_slot_owner[r->plan_slot] == r) idx->plan_slot_owner[r->plan_slot] = nullptr;
  if (!r->plan_copy.not_sorted) t6_hint_update(idx, r->d.Q, r->plan_copy.rows, r->plan_copy.arena);
  else { idx->sort_hint = true; idx->sort_probe_in = 32; }   // (as after a batch that was sorted on the device: the next ones sort first -- also when nobody reads this one)
  return VS_OK;
}
// What a shared batch (run_type6_shared) is for: the type-6 expansion of carrier lists, or one of the three column requests over
// the same rows -- allele counts, the burden matrix, the genotype matrix.  The columns: the subset's bit mask in host memory (NULL:
// the whole cohort) and its words; for burden and matrix the columns in front of each word of the mask (NULL with the mask) and
// their number; for burden the window (0 .. UINT32_MAX: every reported row counts, k_allele_counts is not run); for LD the band's
// window and statistic.  Groups: `mask` is the label table (a byte per sample id, eight to a word), n_cols the number of groups.
// Assoc: mask, rank and n_cols as for the matrix; `pheno` is the upload that travels with them -- Sy~[8], Syy~[8] and the pivots c[8] as doubles, then the
// phenotype table in column order, [column][Kp] float32 -- of pheno_words 8-byte words; the traits and the statistic.
// Scores: mask, rank and n_cols as for the matrix; `weights` (host or device memory, weights_on_device) are n_weights x n_scores
// float32 in report order; score_max_bits: per column the largest |w| as a float pattern, formed on the host from host weights.
// Gram, Ibs: mask, rank and n_cols as for the matrix; the statistic.  LdMatrix: as LD without a window (ld_stat).
// AssocMatrix: mask, rank and n_cols as for the matrix; `am` is the host's limb panel with the traits' shifts and sums (it goes to
// the device once the batch has passed the size limit: assoc_matrix_upload); the traits and the statistic.
// ScoreMatrix: mask, rank and n_cols as for the matrix; `weights` (host memory), n_weights and n_scores as for Scores; `sm_shift`: f_k
// per weight column, formed on the host.
// Prune: as LD (ld_window) with the walk's parameters: prune_max_bp, prune_T (0 .. 2^20), prune_min_ac, prune_max_ac.
// Clump: as Prune without the allele-count window; `clump_keys` (host memory, owned by the result), n_pvalues of them, held against
// the number of table rows once the plan has given it; clump_key: the keys of p1 and p2.
// LdScore: as Prune without the threshold; ld_window = 0 stands for no row limit.
// WindowStats: mask and n_cols as for Groups; ws_sizes: the groups' sizes (n_cols of them), ws_pairs: the pair records (0: none).
// Trio: mask, rank and n_cols as for the matrix (the members); trio_cols (host memory, owned by the result): three column indices
// per trio -- child, father, mother --, n_trios of them.
// Roh: mask, rank and n_cols as for the matrix; roh: the walk's parameters (min_ac / max_ac: the site window, as Prune's).
enum class ReqKind { Lists, Counts, Burden, Matrix, LD, Groups, Assoc, Scores, Gram, Ibs, LdMatrix, AssocMatrix, ScoreMatrix, Prune, Clump, LdScore, WindowStats, Trio, Roh };
struct SharedReq {
  ReqKind kind = ReqKind::Lists;
  const uint64_t* mask = nullptr;
  uint32_t words = 0;
  const uint32_t* rank = nullptr;
  uint32_t n_cols = 0, min_ac = 0, max_ac = UINT32_MAX;
  uint32_t ld_window = 0, ld_stat = 0, gram_stat = 0, ibs_stat = 0;
  uint32_t prune_max_bp = 0, prune_T = 0, prune_min_ac = 0, prune_max_ac = UINT32_MAX;
  const uint64_t* clump_keys = nullptr;
  uint64_t n_pvalues = 0, clump_key[2] = {0, 0};
  const uint64_t* pheno = nullptr;
  size_t pheno_words = 0;
  uint32_t n_traits = 0, assoc_stat = 0;
  const AmPanel* am = nullptr;
  const float* weights = nullptr;
  uint64_t n_weights = 0;
  uint32_t n_scores = 0, score_max_bits[kScoresMax] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool weights_on_device = false;
  const std::vector<int32_t>* sm_shift = nullptr;
  const uint32_t* ws_sizes = nullptr;
  uint32_t ws_pairs = 0;
  const uint32_t* trio_cols = nullptr;
  uint64_t n_trios = 0;
  vs_roh_params roh{};
  bool window() const { return min_ac != 0 || max_ac != UINT32_MAX; }
};
static int run_type6_shared(vs_index* idx, const vs_region* regions, uint64_t n, vs_result* r, bool regions_on_device, const uint64_t* site_records,
                            bool allow_async, bool may_speculate = true, const SharedReq& req = SharedReq{});
// A speculative batch's sizes become the plan's totals here -- or, when the plan refused the batch on the device (more rows or arena
// entries than were allocated, or regions that were not sorted), the batch is run again from the result's own copy of the regions,
// with the exact sizes, before anything is read.  A redo that fails leaves the result torn: its code sticks (vs_result::redo_rc).
static int result_sizes(vs_result* r) {
  if (!r->sizes_pending) return VS_OK;
  vs_index* idx = r->idx;
  VS_TRY(capture_totals(r));
  r->sizes_pending = false;
  const PlanTotals& t = r->plan_copy;
  if (!t.not_sorted && t.rows <= r->cap_rows && t.arena <= r->cap_arena) {
    r->d.A = t.rows; r->d.S = t.arena;
    r->n_rows_reported = t.reported; r->n_unique_sites = t.shared_rows;
    return VS_OK;
  }
  idx->t6_refused++;
  int rc = result_ready(r);                        // (its kernels returned at once; nothing was written behind the plan)
  if (rc == VS_OK) {
    if (idx->timing_owner == r) { idx->timing_owner = nullptr; idx->timing_pending = false; }
    std::vector<DevBuf> old;
    old.swap(r->bufs);                             // (the result's copy of the regions lives in there: released when the redo has read it)
    const uint64_t n = r->d.Q;
    const vs_region* dreg = reinterpret_cast<const vs_region*>(r->d.regions);
    r->d = DevResult{};
    rc = run_type6_shared(idx, dreg, n, r, /*regions_on_device=*/true, nullptr, /*allow_async=*/false, /*may_speculate=*/false);
    release_bufs(idx, old);
  }
  r->redo_rc = rc;
  return rc;
}

// THE entry of every exported accessor of a result, in this order: the result exists and is of the kind asked for, no redo of it has
// failed (vs_result::redo_rc), its handle's device is current -- and, with `sizes`, a speculative batch's sizes are known (result_sizes:
// a refused batch is redone here, on its own handle's device).  The helpers below that take a result (fetch_*, raw_copy_begin,
// launch_pack_regions) assume that the caller has passed this gate; they neither set the device nor resolve sizes.
enum class Want { Variants, Sequences, Any };
static hipError_t result_device(const vs_result* r) { return hipSetDevice(r->idx->device); }   // (vs_result_free's too: it tears down any state)
static int result_enter(vs_result* r, Want want, bool sizes) {
  if (!r) return fail(VS_ERR_ARG, "null argument");
  const bool seq = r->kind == 2 || r->kind == 3;
  if (want == Want::Variants && seq) return fail(VS_ERR_ARG, "a sequence result (query types 2/3) has no variant table; use vs_result_get_sequences");
  if (want == Want::Sequences && !seq) return fail(VS_ERR_ARG, "not a sequence result");
  if (r->redo_rc != VS_OK) return fail(r->redo_rc, "the batch was refused on the device and its redo failed (%s): the result holds nothing; free it", vs_strerror(r->redo_rc));
  HIP_TRY(result_device(r));
  return sizes ? result_sizes(r) : VS_OK;
}

// The expansion of a shared batch that writes the shared rows as well (k_fill_sites2).  mode 2 (tuning builds): split -- rows +
// listed variants here, the dense sites of the index the batch covers in k_fill_dense behind it.
template <bool WIDE, bool TUNE>
static void launch_fill2(vs_index* idx, const DevResult& d, const RunRec* runs, const uint32_t* coarse, uint64_t n_runs, uint64_t U, uint32_t chunk,
                         size_t lds_bytes, uint32_t ablate, uint32_t gt_words, unsigned long long* tstat, int mode, const PlanDev* pd = nullptr) {
  const unsigned blocks = (unsigned)(((U + chunk - 1) / chunk + 3) / 4);
#ifdef VS_TUNING
  if (mode == 2) {
    switch (chunk) {
      case 16: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fill_sites2<WIDE, 16, TUNE, false>), dim3(blocks), dim3(256), lds_bytes, idx->stream, idx->d, d, runs, coarse, n_runs, U, ablate, gt_words, tstat, (const PlanDev*)nullptr); break;
      case 32: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fill_sites2<WIDE, 32, TUNE, false>), dim3(blocks), dim3(256), lds_bytes, idx->stream, idx->d, d, runs, coarse, n_runs, U, ablate, gt_words, tstat, (const PlanDev*)nullptr); break;
      default: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fill_sites2<WIDE, 64, TUNE, false>), dim3(blocks), dim3(256), lds_bytes, idx->stream, idx->d, d, runs, coarse, n_runs, U, ablate, gt_words, tstat, (const PlanDev*)nullptr); break;
    }
    const uint64_t nd = idx->d.n_dense;
    if (nd) {
      const uint32_t k = idx->opts.fill_dense_k;
      const unsigned db = (unsigned)(((nd + k - 1) / k + 3) / 4);
      switch (k) {
        case 8:  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fill_dense<WIDE, 8>), dim3(db), dim3(256), lds_bytes, idx->stream, idx->d, d, runs, n_runs, U, gt_words); break;
        case 32: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fill_dense<WIDE, 32>), dim3(db), dim3(256), lds_bytes, idx->stream, idx->d, d, runs, n_runs, U, gt_words); break;
        case 64: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fill_dense<WIDE, 64>), dim3(db), dim3(256), lds_bytes, idx->stream, idx->d, d, runs, n_runs, U, gt_words); break;
        default: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fill_dense<WIDE, 16>), dim3(db), dim3(256), lds_bytes, idx->stream, idx->d, d, runs, n_runs, U, gt_words); break;
      }
    }
    return;
  }
#endif
  switch (chunk) {
    case 8:  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fill_sites2<WIDE, 8, TUNE>), dim3(blocks), dim3(256), lds_bytes, idx->stream, idx->d, d, runs, coarse, n_runs, U, ablate, gt_words, tstat, pd); break;
    case 32: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fill_sites2<WIDE, 32, TUNE>), dim3(blocks), dim3(256), lds_bytes, idx->stream, idx->d, d, runs, coarse, n_runs, U, ablate, gt_words, tstat, pd); break;
    case 64: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fill_sites2<WIDE, 64, TUNE>), dim3(blocks), dim3(256), lds_bytes, idx->stream, idx->d, d, runs, coarse, n_runs, U, ablate, gt_words, tstat, pd); break;
    default: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fill_sites2<WIDE, 16, TUNE>), dim3(blocks), dim3(256), lds_bytes, idx->stream, idx->d, d, runs, coarse, n_runs, U, ablate, gt_words, tstat, pd); break;
  }
}

// k_allele_counts over the whole table of a count batch (u_site: the site of every row; d_mask NULL: the whole cohort)
static void launch_allele_counts(vs_index* idx, const DevResult& d, const uint32_t* u_site, uint64_t U, const uint64_t* d_mask, uint32_t words, uint4* out) {
  const unsigned blocks = (unsigned)((d.A + 4 * kCountRows - 1) / (4 * kCountRows));
  if (d_mask) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_allele_counts<true>), dim3(blocks), dim3(256), (size_t)words * 8, idx->stream, idx->d,
                                 (const VariantRow*)d.rows, u_site, d.A, U, d_mask, words, out);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_allele_counts<false>), dim3(blocks), dim3(256), 0, idx->stream, idx->d,
                          (const VariantRow*)d.rows, u_site, d.A, U, (const uint64_t*)nullptr, 0u, out);
}

// k_group_counts over the whole table of a grouped-count batch (d_labels: the label table, `words` words of eight label bytes)
static void launch_group_counts(vs_index* idx, const DevResult& d, const uint32_t* u_site, uint64_t U, const uint64_t* d_labels, uint32_t words, uint32_t n_groups,
                                uint4* out) {
  const uint64_t per_block = 4ull * group_rows_per_wave(n_groups);
  const unsigned blocks = (unsigned)((d.A + per_block - 1) / per_block);
  hipLaunchKernelGGL(k_group_counts, dim3(blocks), dim3(256), (size_t)words * 8, idx->stream, idx->d, (const VariantRow*)d.rows, u_site, d.A, U, d_labels, words,
                     n_groups, out);
}

// k_assoc_scan over the whole table of an association batch, behind k_allele_counts over the same table (d_pheno: SharedReq::pheno on
// the device).  The table form: in LDS when it is at most option assoc_lds_max_kib and the workgroup's LDS stays within a CU's.
template <uint32_t KP, bool SUBSET, bool CHI2>
static int launch_assoc_form(vs_index* idx, const AssocArgs& a, unsigned blocks, bool lds_table, size_t lds) {
  const void* fn = lds_table ? reinterpret_cast<const void*>(&k_assoc_scan<KP, SUBSET, true, CHI2>) : reinterpret_cast<const void*>(&k_assoc_scan<KP, SUBSET, false, CHI2>);
  // more than the default LDS of a launch: the limit is raised once per instantiation, to all a CU has beside the static part
  const uint32_t bit = 1u << (16 * CHI2 + 4 * (KP == 1 ? 0 : KP == 2 ? 1 : KP == 4 ? 2 : 3) + 2 * SUBSET + lds_table);
  if (lds + assoc_static_lds(KP) > (48 << 10) && !(idx->assoc_lds_raised & bit)) {
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kAssocLdsPerCu - assoc_static_lds(KP))));
    idx->assoc_lds_raised |= bit;
  }
  if (lds_table) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_assoc_scan<KP, SUBSET, true, CHI2>), dim3(blocks), dim3(256), lds, idx->stream, idx->d, a);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_assoc_scan<KP, SUBSET, false, CHI2>), dim3(blocks), dim3(256), lds, idx->stream, idx->d, a);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}
template <uint32_t KP>
static int launch_assoc_kp(vs_index* idx, const AssocArgs& a, bool subset, bool chi2, unsigned blocks, bool lds_table, size_t lds) {
  if (chi2) return subset ? launch_assoc_form<KP, true, true>(idx, a, blocks, lds_table, lds) : launch_assoc_form<KP, false, true>(idx, a, blocks, lds_table, lds);
  return subset ? launch_assoc_form<KP, true, false>(idx, a, blocks, lds_table, lds) : launch_assoc_form<KP, false, false>(idx, a, blocks, lds_table, lds);
}
static int launch_assoc(vs_index* idx, vs_result* r, const uint32_t* u_site, uint64_t U, const uint64_t* d_mask, const uint32_t* d_rank, const uint64_t* d_pheno,
                        const SharedReq& q) {
  const DevResult& d = r->d;
  const uint32_t kp = assoc_pow2(q.n_traits);
  AssocArgs a{};
  a.rows = (const VariantRow*)d.rows; a.u_site = u_site; a.A = d.A; a.U = U;
  a.S = d_mask; a.S_rank = d_rank; a.s_words = d_mask ? q.words : 0;
  a.n_cols = q.n_cols; a.K = q.n_traits; a.chi2 = q.assoc_stat == VS_ASSOC_CHI2;
  const bool chi2 = a.chi2 != 0;
  a.sums = reinterpret_cast<const double*>(d_pheno);
  a.table = reinterpret_cast<const float*>(d_pheno + kAssocHeadWords);
  a.counts = r->d_counts; a.out = r->d_scores;
  const size_t sub = d_mask ? ((size_t)q.words * 8 + 15) / 16 * 16 + ((size_t)q.words * 4 + 15) / 16 * 16 : 0;
  const size_t table = (size_t)q.n_cols * kp * 4;
  const size_t cap = (size_t)(idx->opts.assoc_lds_max_kib ? idx->opts.assoc_lds_max_kib : 32) << 10;
  const bool lds_table = table <= cap && assoc_static_lds(kp) + sub + table <= kAssocLdsPerCu;
  const size_t lds = sub + (lds_table ? table : 0);
  const unsigned blocks = (unsigned)((d.A + 4 * kAssocRows - 1) / (4 * kAssocRows));
  switch (kp) {
    case 1: return launch_assoc_kp<1>(idx, a, d_mask != nullptr, chi2, blocks, lds_table, lds);
    case 2: return launch_assoc_kp<2>(idx, a, d_mask != nullptr, chi2, blocks, lds_table, lds);
    case 4: return launch_assoc_kp<4>(idx, a, d_mask != nullptr, chi2, blocks, lds_table, lds);
    default: return launch_assoc_kp<8>(idx, a, d_mask != nullptr, chi2, blocks, lds_table, lds);
  }
}

// The burden matrix of a count batch whose per-region arrays are in the caller's order: one workgroup per (region, column tile), and
// -- only when the rows all regions report could hold a region longer than a chunk -- the device-built list of such regions' chunks
// and the launch that adds them (its workgroups beyond the list return at once).
template <bool SUBSET, bool WINDOW>
static int launch_burden_kernels(vs_index* idx, const BurdenArgs& a, uint64_t Q, uint32_t cap, size_t lds) {
  auto big_lds = [&](const void* fn) -> int {   // (more than 64 KiB of dynamic LDS is asked for per kernel)
    if (lds > (64 << 10)) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return VS_OK;
  };
  VS_TRY(big_lds(reinterpret_cast<const void*>(&k_sample_burden<SUBSET, WINDOW, false>)));
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sample_burden<SUBSET, WINDOW, false>), dim3((unsigned)(Q * a.n_tiles)), dim3(256), lds, idx->stream, idx->d, a);
  if (cap) {
    VS_TRY(big_lds(reinterpret_cast<const void*>(&k_sample_burden<SUBSET, WINDOW, true>)));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sample_burden<SUBSET, WINDOW, true>), dim3((unsigned)((uint64_t)cap * a.n_tiles)), dim3(256), lds, idx->stream, idx->d, a);
  }
  HIP_TRY(hipGetLastError());
  return VS_OK;
}
static int launch_burden(vs_index* idx, vs_result* r, const uint32_t* u_site, uint64_t U, const uint64_t* d_mask, const uint32_t* d_rank, const SharedReq& bq,
                         ScratchBufs& scratch) {
  const DevResult& d = r->d;
  BurdenArgs a{};
  a.rows = d.rows; a.u_site = u_site; a.U = U; a.var_begin = d.var_begin; a.q_nvar = d.q_nvar;
  a.S = d_mask; a.S_rank = d_rank; a.s_words = d_mask ? bq.words : 0;
  a.ac = r->d_counts; a.min_ac = bq.min_ac; a.max_ac = bq.max_ac;
  a.n_cols = bq.n_cols;
  a.tile_cols = std::min<uint32_t>(bq.n_cols, kBurdenTileCols);
  a.n_tiles = (bq.n_cols + a.tile_cols - 1) / a.tile_cols;
  a.chunk_rows = idx->opts.burden_chunk ? idx->opts.burden_chunk : kBurdenChunkRows;
  a.cells = r->d_cells; a.total = r->d_cell_total;
  uint32_t* n_work = reinterpret_cast<uint32_t*>(r->d_cell_total + 1);
  a.n_work = n_work;
  if (d.Q * a.n_tiles > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu regions x %u column tiles)", (unsigned long long)d.Q, a.n_tiles);
  HIP_TRY(hipMemsetAsync(r->d_cell_total, 0, 16, idx->stream));
  // every split region has more than chunk_rows rows, so its chunks number less than twice its rows / chunk_rows
  const uint64_t cap64 = r->n_rows_reported > a.chunk_rows ? 2 * r->n_rows_reported / a.chunk_rows : 0;
  if (cap64 * a.n_tiles > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu row chunks x %u column tiles)", (unsigned long long)cap64, a.n_tiles);
  const uint32_t cap = (uint32_t)cap64;
  if (cap) {
    uint2* work = nullptr;
    VS_TRY(dev_alloc(idx, (size_t)cap * sizeof(uint2), (void**)&work, &scratch.bufs));
    a.work = work;
    hipLaunchKernelGGL(k_burden_split_plan, dim3((unsigned)((d.Q + 255) / 256)), dim3(256), 0, idx->stream, (const uint64_t*)d.q_nvar, d.Q, a.chunk_rows, work, n_work, cap);
  }
  const size_t lds = (size_t)a.tile_cols * 16 + (size_t)a.s_words * 12;
  const bool window = r->d_counts != nullptr;
  if (d_mask) return window ? launch_burden_kernels<true, true>(idx, a, d.Q, cap, lds) : launch_burden_kernels<true, false>(idx, a, d.Q, cap, lds);
  return window ? launch_burden_kernels<false, true>(idx, a, d.Q, cap, lds) : launch_burden_kernels<false, false>(idx, a, d.Q, cap, lds);
}

// The genotype matrix of a count batch: one workgroup per (block of table rows, column tile).  The tile is at most the pitch and
// at most kMatrixTileBytes; a block takes as many rows as fit beside it, up to one per thread.  `cells`: the result's matrix, or
// the temporary one of an LD batch.
static int launch_matrix(vs_index* idx, vs_result* r, uint8_t* cells, const uint32_t* u_site, uint64_t U, const uint64_t* d_mask, const uint32_t* d_rank,
                         const SharedReq& mq) {
  const DevResult& d = r->d;
  const uint32_t words = mq.words;
  HIP_TRY(hipMemsetAsync(r->d_cell_total, 0, 16, idx->stream));
  if (!d.A) return VS_OK;
  MatrixArgs a{};
  a.rows = d.rows; a.u_site = u_site; a.A = d.A; a.U = U;
  a.S = d_mask; a.S_rank = d_rank; a.s_words = d_mask ? words : 0;
  a.n_cols = mq.n_cols; a.pitch = (uint32_t)r->mx_pitch;
  a.tile_cols = std::min<uint32_t>(a.pitch, idx->opts.matrix_tile_cols ? idx->opts.matrix_tile_cols : kMatrixTileCols);
  a.n_tiles = (a.pitch + a.tile_cols - 1) / a.tile_cols;
  a.rows_per_block = std::max<uint32_t>(1, std::min<uint32_t>(kMatrixMaxRows, kMatrixTileBytes / a.tile_cols));
  a.cells = cells; a.total = r->d_cell_total;
  const uint64_t blocks = (d.A + a.rows_per_block - 1) / a.rows_per_block * a.n_tiles;
  if (blocks > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu row blocks x %u column tiles)",
                                           (unsigned long long)(blocks / a.n_tiles), a.n_tiles);
  const size_t lds = (size_t)a.rows_per_block * a.tile_cols + (d_mask ? ((size_t)words * 8 + 15) / 16 * 16 + ((size_t)words * 4 + 15) / 16 * 16 : 0) + kMatrixParamBytes;
  const void* fn = d_mask ? reinterpret_cast<const void*>(&k_genotype_matrix<true>) : reinterpret_cast<const void*>(&k_genotype_matrix<false>);
  if (lds > (48 << 10)) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (d_mask) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_genotype_matrix<true>), dim3((unsigned)blocks), dim3(256), lds, idx->stream, idx->d, a);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_genotype_matrix<false>), dim3((unsigned)blocks), dim3(256), lds, idx->stream, idx->d, a);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}

// The band of an LD batch from its temporary genotype matrix and the table's counts: one workgroup per kLdRows table rows.
static int launch_ld(vs_index* idx, vs_result* r, const uint8_t* cells, const SharedReq& lq) {
  const DevResult& d = r->d;
  if (!d.A) return VS_OK;
  LdArgs a{};
  a.cells = cells; a.A = d.A; a.pitch = (uint32_t)r->mx_pitch; a.n_cols = lq.n_cols;
  a.window = lq.ld_window; a.n_tiles = (lq.ld_window + 15) / 16 + 1;
  a.counts = r->d_counts; a.band = r->d_band;
  const uint64_t blocks = (d.A + kLdRows - 1) / kLdRows;
  if (blocks > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu row blocks)", (unsigned long long)blocks);
  const size_t lds = (size_t)(kLdRows + 16 * (a.n_tiles - 1)) * kLdStride;
  const bool small = a.n_tiles <= kLdSmallTiles, r2 = lq.ld_stat == VS_LD_R2;
  const void* fn = small ? (r2 ? reinterpret_cast<const void*>(&k_ld_band<kLdSmallTiles, true>) : reinterpret_cast<const void*>(&k_ld_band<kLdSmallTiles, false>))
                         : (r2 ? reinterpret_cast<const void*>(&k_ld_band<kLdMaxTiles, true>) : reinterpret_cast<const void*>(&k_ld_band<kLdMaxTiles, false>));
  if (lds > (48 << 10)) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const dim3 grid((unsigned)blocks), block(256);
  if (small) {
    if (r2) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ld_band<kLdSmallTiles, true>), grid, block, lds, idx->stream, a);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ld_band<kLdSmallTiles, false>), grid, block, lds, idx->stream, a);
  } else {
    if (r2) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ld_band<kLdMaxTiles, true>), grid, block, lds, idx->stream, a);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ld_band<kLdMaxTiles, false>), grid, block, lds, idx->stream, a);
  }
  HIP_TRY(hipGetLastError());
  return VS_OK;
}

// Table rows per workgroup of k_sample_gram.  Option gram_chunk, or by the batch's shape: the chunk that gives about
// kGramBlocksWanted workgroups over all tile pairs, a multiple of kGramK, at least 2 kGramK (fewer rows per workgroup only add
// atomics) and at most kGramChunkMax.
static uint32_t gram_chunk_rows(const vs_index* idx, uint64_t A, uint32_t n_pairs) {
  if (idx->opts.gram_chunk) return idx->opts.gram_chunk;
  const uint64_t per = (A * n_pairs + kGramBlocksWanted - 1) / kGramBlocksWanted;
  const uint64_t rows = (per + kGramK - 1) / kGramK * kGramK;
  return (uint32_t)std::min<uint64_t>(kGramChunkMax, std::max<uint64_t>(2 * kGramK, rows));
}

// The Gram matrix of a batch from its temporary genotype matrix and the table's counts: the result's words cleared, k_sample_gram
// over (tile pair, row chunk), k_gram_moments over (row chunk, column group) and -- under VS_GRAM_GRM -- k_gram_finish over the
// cells.  (launch_matrix, in front of this, has cleared and filled d_cell_total.)
static int launch_gram(vs_index* idx, vs_result* r, const uint8_t* cells, const SharedReq& gq) {
  const DevResult& d = r->d;
  const uint64_t n = gq.n_cols;
  const size_t head = (size_t)(n * n + n + 2);   // gram, col_weighted, C, H
  HIP_TRY(hipMemsetAsync(r->d_gram, 0, head * 8, idx->stream));
  const bool grm = gq.gram_stat == VS_GRAM_GRM;
  if (!d.A) {   // an empty table: an all-zero matrix, H = 0
    if (grm) HIP_TRY(hipMemsetAsync(r->d_gram + r->gram_grm_off, 0, (size_t)(n * n) * 8, idx->stream));
    return VS_OK;
  }
  GramArgs a{};
  a.cells = cells; a.A = d.A; a.pitch = (uint32_t)r->mx_pitch; a.n_cols = gq.n_cols;
  a.n_tiles = (gq.n_cols + kGramTile - 1) / kGramTile;
  const uint64_t pairs = (uint64_t)a.n_tiles * (a.n_tiles + 1) / 2;
  if (pairs > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu tile pairs)", (unsigned long long)pairs);
  a.n_pairs = (uint32_t)pairs;
  a.chunk = gram_chunk_rows(idx, d.A, a.n_pairs);
  a.counts = r->d_counts;
  a.gram = reinterpret_cast<unsigned long long*>(r->d_gram);
  a.colw = a.gram + n * n; a.ch = a.colw + n;
  a.grm = grm ? reinterpret_cast<double*>(r->d_gram + r->gram_grm_off) : nullptr;
  const uint64_t chunks = (d.A + a.chunk - 1) / a.chunk, blocks = chunks * pairs;
  const uint64_t mrows = (d.A + kGramMomentRows - 1) / kGramMomentRows, mcols = (a.pitch + kGramMomentCols - 1) / kGramMomentCols;
  const uint64_t fblocks = (n * n + 255) / 256;
  if (blocks > 0x7FFFFFFFull || mrows > 0x7FFFFFFFull || mcols > 65535 || fblocks > 0x7FFFFFFFull)
    return fail(VS_ERR_ARG, "batch too large for one launch (%llu row chunks x %llu tile pairs)", (unsigned long long)chunks, (unsigned long long)pairs);
  hipLaunchKernelGGL(k_sample_gram, dim3((unsigned)blocks), dim3(256), kGramLds, idx->stream, a);
  hipLaunchKernelGGL(k_gram_moments, dim3((unsigned)mrows, (unsigned)mcols), dim3(256), 0, idx->stream, a);
  if (grm) hipLaunchKernelGGL(k_gram_finish, dim3((unsigned)fblocks), dim3(256), 0, idx->stream, a);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}

// Table rows per workgroup of k_sample_ibs.  Option ibs_chunk, or by the batch's shape as gram_chunk_rows: the chunk that gives about
// kIbsBlocksWanted workgroups over all tile pairs, a multiple of kGramK, at least 2 kGramK and at most kIbsChunkMax -- and then the
// table's rows spread evenly over that number of chunks, so that the last chunk is not a short one the others wait for.
static uint32_t ibs_chunk_rows(const vs_index* idx, uint64_t A, uint32_t n_pairs) {
  if (idx->opts.ibs_chunk) return idx->opts.ibs_chunk;
  const uint64_t per = (A * n_pairs + kIbsBlocksWanted - 1) / kIbsBlocksWanted;
  const uint64_t rows = std::min<uint64_t>(kIbsChunkMax, std::max<uint64_t>(2 * kGramK, (per + kGramK - 1) / kGramK * kGramK));
  const uint64_t chunks = (A + rows - 1) / rows;
  return (uint32_t)std::max<uint64_t>(2 * kGramK, ((A + chunks - 1) / chunks + kGramK - 1) / kGramK * kGramK);
}

// The IBS matrices of a batch from its temporary genotype matrix: the three primitives and n_used cleared, k_ibs_n_used over the
// table's rows, k_sample_ibs over (tile pair, row chunk), k_ibs_finish over the cells.  (launch_matrix, in front of this, has
// cleared and filled d_cell_total.)
static int launch_ibs(vs_index* idx, vs_result* r, const uint8_t* cells, uint64_t U, const SharedReq& iq) {
  const DevResult& d = r->d;
  const uint64_t n = iq.n_cols, nn = n * n;
  const bool king = iq.ibs_stat == VS_IBS_KING;
  if (!d.A) {   // an empty table: all-zero matrices, n_used = 0
    HIP_TRY(hipMemsetAsync(r->d_ibs, 0, (size_t)(5 * nn + 1) * 8, idx->stream));
    if (king) HIP_TRY(hipMemsetAsync(r->d_ibs + r->ibs_king_off, 0, (size_t)nn * 8, idx->stream));
    return VS_OK;
  }
  HIP_TRY(hipMemsetAsync(r->d_ibs, 0, (size_t)(3 * nn) * 8, idx->stream));
  HIP_TRY(hipMemsetAsync(r->d_ibs + 5 * nn, 0, 8, idx->stream));
  IbsArgs a{};
  a.m.cells = cells; a.m.A = d.A; a.m.pitch = (uint32_t)r->mx_pitch; a.m.n_cols = iq.n_cols;
  a.m.n_tiles = (iq.n_cols + kGramTile - 1) / kGramTile;
  const uint64_t pairs = (uint64_t)a.m.n_tiles * (a.m.n_tiles + 1) / 2;
  if (pairs > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu tile pairs)", (unsigned long long)pairs);
  a.m.n_pairs = (uint32_t)pairs;
  a.m.chunk = ibs_chunk_rows(idx, d.A, a.m.n_pairs);
  a.rows = (const VariantRow*)d.rows; a.U = U;
  a.het_het = reinterpret_cast<unsigned long long*>(r->d_ibs);
  a.ibs0 = r->d_ibs + 3 * nn;
  a.n_used = reinterpret_cast<unsigned long long*>(r->d_ibs + 5 * nn);
  a.king = king ? reinterpret_cast<double*>(r->d_ibs + r->ibs_king_off) : nullptr;
  const uint64_t chunks = (d.A + a.m.chunk - 1) / a.m.chunk, blocks = chunks * pairs;
  const uint64_t ublocks = std::min<uint64_t>((d.A + 1023) / 1024, 1024), fblocks = (nn + 255) / 256;
  if (blocks > 0x7FFFFFFFull || fblocks > 0x7FFFFFFFull)
    return fail(VS_ERR_ARG, "batch too large for one launch (%llu row chunks x %llu tile pairs)", (unsigned long long)chunks, (unsigned long long)pairs);
  hipLaunchKernelGGL(k_ibs_n_used, dim3((unsigned)ublocks), dim3(256), 0, idx->stream, a);
  hipLaunchKernelGGL(k_sample_ibs, dim3((unsigned)blocks), dim3(256), kGramLds, idx->stream, a);
  hipLaunchKernelGGL(k_ibs_finish, dim3((unsigned)fblocks), dim3(256), 0, idx->stream, a);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}

// Trios one workgroup of k_trio_scan takes.  Option trio_chunk, or by the batch's shape: all of them -- every chunk stages the block's
// rows again -- unless the row blocks alone give fewer than kTrioBlocksWanted workgroups; then as many chunks as reach that number,
// of at least four slabs of 64 (one per wave).  At most kTrioChunkMax, a multiple of 64.
static uint32_t trio_chunk_trios(const vs_index* idx, uint64_t row_blocks, uint64_t n_trios) {
  if (idx->opts.trio_chunk) return idx->opts.trio_chunk;
  const uint64_t slabs = (n_trios + 63) / 64;
  const uint64_t want = std::max<uint64_t>(1, (kTrioBlocksWanted + row_blocks - 1) / std::max<uint64_t>(row_blocks, 1));
  const uint64_t per = std::min<uint64_t>(kTrioChunkMax / 64, std::max<uint64_t>(4, (slabs + want - 1) / want));
  return (uint32_t)(std::min(per, slabs) * 64);
}
template <uint32_t R>
static int launch_trio_r(vs_index* idx, const TrioArgs& a, unsigned blocks) {
  const size_t lds = (size_t)R * a.pitch;
  if (lds > (48 << 10)) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_trio_scan<R>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_trio_scan<R>), dim3(blocks), dim3(256), lds, idx->stream, a);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}
// The records of a trio batch from its temporary genotype matrix and the table's counts: both record arrays and n_used cleared, the
// trio table uploaded (trio_upload, in front of the pair of events), k_ibs_n_used over the table's rows, k_trio_scan over (row block,
// trio chunk).  (launch_matrix, in front of this, has cleared and filled d_cell_total.)
static int launch_trio(vs_index* idx, vs_result* r, const uint8_t* cells, uint64_t U, const SharedReq& tq) {
  const DevResult& d = r->d;
  HIP_TRY(hipMemsetAsync(r->d_trio, 0, (size_t)(d.A + tq.n_trios) * 16 + 8, idx->stream));
  if (!d.A) return VS_OK;   // an empty table: all-zero records, n_used = 0
  IbsArgs u{};
  u.m.A = d.A; u.rows = (const VariantRow*)d.rows; u.U = U;
  u.n_used = reinterpret_cast<unsigned long long*>(r->d_trio + (size_t)(d.A + tq.n_trios) * 16);
  hipLaunchKernelGGL(k_ibs_n_used, dim3((unsigned)std::min<uint64_t>((d.A + 1023) / 1024, 1024)), dim3(256), 0, idx->stream, u);
  TrioArgs a{};
  a.cells = cells; a.A = d.A; a.pitch = (uint32_t)r->mx_pitch; a.n_cols = tq.n_cols;
  a.counts = r->d_counts;
  a.trio_cols = reinterpret_cast<const uint32_t*>(r->d_trio + r->trio_table_off);
  a.n_trios = (uint32_t)tq.n_trios;
  a.rows = reinterpret_cast<uint32_t*>(r->d_trio);
  a.trios = a.rows + 4 * d.A;
  uint32_t R = kTrioRowsMax;   // the largest power of two up to min(kTrioRowsMax, kTrioTileBytes / pitch), at least 1
  while (R > 1 && (uint64_t)R * a.pitch > kTrioTileBytes) R >>= 1;
  const uint64_t row_blocks = (d.A + R - 1) / R;
  a.chunk = trio_chunk_trios(idx, row_blocks, tq.n_trios);
  a.n_chunks = (uint32_t)((tq.n_trios + a.chunk - 1) / a.chunk);
  const uint64_t blocks = row_blocks * a.n_chunks;
  if (blocks > 0x7FFFFFFFull)
    return fail(VS_ERR_ARG, "batch too large for one launch (%llu row blocks x %u trio chunks)", (unsigned long long)row_blocks, a.n_chunks);
  switch (R) {
    case 16: return launch_trio_r<16>(idx, a, (unsigned)blocks);
    case 8: return launch_trio_r<8>(idx, a, (unsigned)blocks);
    case 4: return launch_trio_r<4>(idx, a, (unsigned)blocks);
    case 2: return launch_trio_r<2>(idx, a, (unsigned)blocks);
    default: return launch_trio_r<1>(idx, a, (unsigned)blocks);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Query type 6 over a batch whose regions SHARE rows and carrier lists (every batch of more than 64 regions unless option
// share_lists is 0), and every count, grouped-count, burden, genotype-matrix, LD, Gram and IBS batch: the same plan and rows, another consumer (SharedReq).
// Like the private-row batches further down it runs as stages over a context, each a function that reads only what the
// stages before it left in the SharedCtx:
//   shared_setup       per-region arrays, regions / mask / ranks on the device, the decisions taken up front, the plan's temporaries
//   shared_plan_batch  shared_plan = k_t6_bounds / _mid / _totals / _apply: bounds, E_prev, the per-region arrays, the row deltas, the
//                      slow-region list; the totals arrive in mapped host memory and the host spins on their sequence word (the one
//                      host wait of a batch; a speculative batch does not wait).  A batch that turns out not to be sorted by first
//                      site is sorted on the device (shared_sort) and planned again; a handle whose last batch was, sorts first
//   shared_tables      sizes from the totals or the speculation; the table and, by the request's kind, arena | counts | burden cells
//                      (counts only under a window) | the matrix, refused beyond option matrix_max_mib before anything is allocated |
//                      LD: counts, the band and -- with the call's temporaries -- the matrix it is formed from, under the same limit
//   shared_rows        k_t6_slow (private copies + the literal duplicate rule, only when the plan counted such regions), k_share_rows2
//                      unless the expansion writes the rows itself; a column request: the site of every row (k_count_slow_sites)
//   shared_expand      Lists: k_fill_sites2, the shared rows AND their carrier lists in one launch -- with async_fill k_fill_sites on
//                      the second stream, with resident lists nothing | shared_columns  Counts: k_allele_counts over the table,
//                      Groups: k_group_counts over the table, Assoc: k_allele_counts, then k_assoc_scan over the table
//   shared_permute_out an unsorted batch's per-region arrays back in the caller's order
//   shared_columns     Burden, Matrix, LD, Scores, behind the permutation -- the matrix's rows are the regions in the caller's order: k_allele_counts
//                      only under a window, k_sample_burden over (region, column tile) pairs and for regions longer than a chunk
//                      k_burden_split_plan + the SPLIT launch | k_genotype_matrix over (block of table rows, column tile) pairs |
//                      LD: k_allele_counts over the table, k_genotype_matrix into the temporary, k_ld_band over blocks of table rows |
//                      Gram: the same two, then k_sample_gram, k_gram_moments and (GRM) k_gram_finish (launch_gram) |
//                      Ibs: the same two, then k_ibs_n_used, k_sample_ibs and k_ibs_finish (launch_ibs) |
//                      Trio: the same two, then k_ibs_n_used and k_trio_scan (launch_trio); the trio table goes up in front of them |
//                      Roh: the same two, then k_roh_sites and k_roh_walk; with segments a scan, one host wait and the walk again (launch_roh) |
//                      LdMatrix: in front of them k_ld_block_scan over the per-region row counts and one host wait for its totals
//                      (ld_matrix_tables: the size limit, the temporary matrix, the cells); behind them k_ld_block (launch_ld_block)
//                      Prune: in front of them k_prune_scan over the per-region row counts and one host wait for its total
//                      (prune_tables: the size limit, the temporary matrix and masks, the state); behind them k_prune_hits and
//                      k_prune_greedy (launch_prune)
//                      Clump: as Prune up to k_prune_hits (clump_tables also uploads the keys); behind it k_clump_class,
//                      k_clump_blockers and k_clump_rounds (launch_clump)
//   shared_finish      enqueued: the completion event | synchronous: k_post_done, a word in mapped host memory, the host spins on it
// A column request is never speculative, has no arena, and leaves the handle's type-6 state (size hints, sort hint) as it found
// it: count batches interleaved with type-6 batches change none of theirs.
// ---------------------------------------------------------------------------------------------------------------------
struct SharedCtx {
  vs_index* idx;
  vs_result* r;
  uint64_t n;
  const SharedReq& req;
  ScratchBufs scratch;
  ScratchBufs ld_tmp;   // an LD, LD-matrix, Gram, IBS or trait-matrix batch's temporary genotype matrix (the last one's limb panel too), apart from the rest: an enqueued batch keeps it only until it has finished
  // the consumer, asked once: Lists -- carrier lists in an arena (the result's or the resident one), may speculate, owns the handle's
  // type-6 hints; else a column request -- no arena, never speculative, hints untouched, the site of EVERY row (u_site).  Burden,
  // Matrix, LD and Scores are consumed behind k_permute_out, Lists, Counts, Groups and Assoc in front of it
  const bool lists, behind_perm;
  // shared_setup: the decisions taken up front
  bool allow_async = false, async_submit = false, sort_first = false, plan_aside = false, resident = false, spec = false;
  hipStream_t ps = nullptr;                // the plan's stream: the handle's own unless plan_aside
  const uint64_t* regions_dev = nullptr;   // regions already in device memory are copied by the kernel that reads them first: k_t6_bounds
  const uint64_t* site_records = nullptr;
  int slot = -1;                           // speculative: the batch's mailbox in the ring
  PlanTotals* pt = nullptr;
  uint64_t want_rows = 0, want_arena = 0;
  uint64_t* d_mask = nullptr;   // a column request over a subset: its bit mask, copied with the regions
  uint32_t* d_rank = nullptr;   // (burden, matrix) the columns in front of each mask word
  uint64_t* d_pheno = nullptr;  // (assoc) the traits' sums and the phenotype table, copied with them
  // the plan's temporaries (e_prev_c: the arena prefix at E_prev, carried by the same scan -- k_rows.hip.h: ShareMax)
  uint32_t items = 0, ntiles = 0, *e_prev = nullptr, *status = nullptr, *slow_list = nullptr, *coarse = nullptr;
  uint64_t* e_prev_c = nullptr;
  ShareMax* tile_max = nullptr;
  Scan5* tile_sums = nullptr;
  RunRec* runs = nullptr;
  PlanDev* plan_dev = nullptr;
  DevResult d_user{};        // shared_sort: the caller's per-region arrays while an unsorted batch works on sorted copies
  uint32_t* perm = nullptr;  // sorted position -> region of the caller's batch (NULL: the batch is worked in the order given)
  bool plan_end_enqueued = false;   // ev[1] recorded behind the (last) plan and waited for by the handle's stream
  uint64_t plan_seq = 0, U = 0, n_slow = 0, n_runs = 0;   // what the plan produced
  uint64_t n_fill = 0;          // shared_tables: carrier lists to expand, and the form of the rows and the expansion
  bool async_fill = false, fused = false, lean = false;
  uint32_t* u_site = nullptr;   // shared_rows: the site of every shared row (a column request: of every row)
  uint8_t* ld_matrix = nullptr; // shared_tables: the temporary genotype matrix of an LD batch (ld_tmp); an LD-matrix batch: ld_matrix_tables
  uint4* ws_counts = nullptr;   // shared_tables: a window-statistics batch's temporary grouped counts (ld_tmp)
  uint32_t* prune_hits = nullptr;   // prune_tables: a pruning batch's hit masks (ld_tmp)
  uint64_t* clump_keys = nullptr;   // clump_tables: a clumping batch's keys, classes and blocker masks (ld_tmp)
  uint8_t* clump_cls = nullptr;
  uint32_t* clump_blockers = nullptr;
  uint64_t* am_dev = nullptr;   // shared_tables: a trait-matrix batch's Sy, vy, shifts and limb panel on the device (ld_tmp)
  uint32_t fill_launches = 0;   // the consumer's, for the phase times
  SharedCtx(vs_index* i, vs_result* res, uint64_t nn, const SharedReq& q)
      : idx(i), r(res), n(nn), req(q), scratch(i), ld_tmp(i), lists(q.kind == ReqKind::Lists), behind_perm(q.kind == ReqKind::Burden || q.kind == ReqKind::Matrix || q.kind == ReqKind::LD || q.kind == ReqKind::Scores || q.kind == ReqKind::Gram || q.kind == ReqKind::Ibs || q.kind == ReqKind::LdMatrix || q.kind == ReqKind::AssocMatrix || q.kind == ReqKind::ScoreMatrix || q.kind == ReqKind::Prune || q.kind == ReqKind::Clump || q.kind == ReqKind::LdScore || q.kind == ReqKind::WindowStats || q.kind == ReqKind::Trio || q.kind == ReqKind::Roh) {}
};

// The nine per-region arrays of a shared batch, f(array, elements) for each: shared_setup carves them out of one buffer of the
// result, shared_sort takes the sorted copies from the pool.
template <typename F>
static int region_arrays(DevResult& d, uint64_t** regions, uint64_t n, F&& f) {
  VS_TRY(f(regions, 2 * n)); VS_TRY(f(&d.q_flags, n)); VS_TRY(f(&d.q_g0, n)); VS_TRY(f(&d.q_nvar, n)); VS_TRY(f(&d.q_ncar, n));
  VS_TRY(f(&d.var_begin, n + 1)); VS_TRY(f(&d.car_base, n + 1)); VS_TRY(f(&d.var_count, n)); VS_TRY(f(&d.q_car_len, n));
  return VS_OK;
}
// The table and the arena of a list batch, of the sizes in d.A / d.S (resident lists: the index's arena).
static int shared_list_tables(SharedCtx& c) {
  DevResult& d = c.r->d;
  VS_TRY(ralloc(c.r, d.A, &d.rows));
  if (c.resident) { d.carriers = c.idx->res_arena; return VS_OK; }
  uint8_t* arena = nullptr;
  VS_TRY(ralloc(c.r, d.S * d.car_width + 16, &arena));
  d.carriers = arena;
  return VS_OK;
}

// Leaves: the result's per-region arrays, regions (mask, ranks) on their way to the device behind ev[0], every decision of the
// context's first block, the plan's temporaries -- and a speculative batch's slot, table and arena.
static int shared_setup(SharedCtx& c, const vs_region* regions, bool regions_on_device, bool may_speculate) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const uint64_t n = c.n;
  const SharedReq& q = c.req;
  VS_TRY(begin_batch(idx));
  DevResult& d = r->d;
  d.Q = n;
  uint64_t* dreg = nullptr;
  {   // the per-region arrays of the result: one buffer
    Slab sl;
    (void)region_arrays(d, &dreg, n, [&](auto** p, uint64_t k) { sl.want(*p, k); return VS_OK; });
    if (q.mask) sl.want(c.d_mask, q.words);
    if (q.rank) sl.want(c.d_rank, q.words);
    if (q.pheno) sl.want(c.d_pheno, q.pheno_words);
    VS_TRY(ralloc(r, sl.bytes, &sl.base));
    sl.carve();
  }
  d.regions = dreg;
  // async_submit: the PLAN of this batch runs on a stream of its own -- beside the expansion of the batch before it, which
  // is still on the handle's stream when the caller submits back to back.  The plan reads the regions and the index and
  // writes this batch's own arrays; nothing in the pool is referenced by work in flight (a batch that returned when it
  // was enqueued keeps its temporaries until its completion event, vs_result::ev_done), so its buffers are its own.  The
  // rest of the batch (rows, expansion) goes to the handle's stream behind an event.  Not for a handle that sorts first,
  // not with async_fill (whose second stream plays the opposite game).
  c.async_submit = c.allow_async && idx->opts.async_submit && !idx->opts.async_fill && !idx->opts.lat_debug;
  c.sort_first = c.lists && idx->sort_hint && idx->sort_probe_in > 0;
  c.plan_aside = c.async_submit && !c.sort_first;
  if (c.plan_aside) VS_TRY(ensure_plan_stream(idx));
  c.ps = c.plan_aside ? idx->plan_stream : idx->stream;
  c.regions_dev = regions && regions_on_device && !c.site_records && (reinterpret_cast<uintptr_t>(regions) & 15) == 0
                      ? reinterpret_cast<const uint64_t*>(regions) : nullptr;
  if (c.regions_dev) {}
  else if (regions) HIP_TRY(hipMemcpyAsync(dreg, regions, n * 16, regions_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c.ps));
  else HIP_TRY(hipMemsetAsync(dreg, 0, n * 16, c.ps));
  if (c.d_mask) HIP_TRY(hipMemcpyAsync(c.d_mask, q.mask, (size_t)q.words * 8, hipMemcpyHostToDevice, c.ps));
  if (c.d_rank) HIP_TRY(hipMemcpyAsync(c.d_rank, q.rank, (size_t)q.words * 4, hipMemcpyHostToDevice, c.ps));
  if (c.d_pheno) HIP_TRY(hipMemcpyAsync(c.d_pheno, q.pheno, q.pheno_words * 8, hipMemcpyHostToDevice, c.ps));
  HIP_TRY(hipEventRecord(idx->ev[0], c.ps));
  c.resident = c.lists && idx->opts.resident_lists && idx->res_arena;
  c.items = (uint32_t)((n + (uint64_t)kPlanBlock * kPlanMaxTiles - 1) / ((uint64_t)kPlanBlock * kPlanMaxTiles));
  if (n >= 65536 && c.items < idx->opts.plan_items) c.items = idx->opts.plan_items;   // (regions per thread of the plan's kernels: see EngineOpts::plan_items)
  c.ntiles = (uint32_t)((n + (uint64_t)kPlanBlock * c.items - 1) / ((uint64_t)kPlanBlock * c.items));
  {   // the plan's temporaries: one buffer
    Slab sl;
    sl.want(c.coarse, idx->d.G / kCoarseRows + 2); sl.want(c.tile_max, c.ntiles);
    sl.want(c.tile_sums, c.ntiles + 1);   // (+ the totals: k_t6_totals)
    sl.want(c.e_prev, n); sl.want(c.status, 1); sl.want(c.slow_list, n); sl.want(c.runs, n + 1); sl.want(c.plan_dev, 1); sl.want(c.e_prev_c, n);
    VS_TRY(dev_alloc(idx, sl.bytes, (void**)&sl.base, &c.scratch.bufs));
    sl.carve();
  }
  // SPECULATIVE (round 6, option t6_speculate): the default batch -- async_submit, rows and lists in one launch, regions given as regions --
  // on a handle whose previous shared batch was about this size does not wait for the plan's totals: table and arena are sized from that
  // batch (+ 1/8), k_t6_totals leaves the totals and its verdict in device memory for the kernels behind it (PlanDev) and in this batch's
  // own mailbox for the host, which reads it when the result is first asked for anything (result_sizes) -- and redoes a refused batch.
  c.want_rows = idx->t6_hint_rows; c.want_arena = idx->t6_hint_arena;
  c.spec = may_speculate && c.lists && idx->opts.t6_speculate && c.plan_aside && regions && !c.site_records && !c.resident && idx->opts.fill_fused && !idx->opts.fill_mode &&
           !idx->opts.fill_stats && !idx->opts.lat_debug && c.want_rows > 0 && idx->t6_hint_n > 0 && n * 4 <= idx->t6_hint_n * 5 && n * 5 >= idx->t6_hint_n * 4;
  if (c.spec) {
    c.slot = (int)(idx->plan_slot_next++ % vs_index::kPlanSlots);
    if (idx->plan_slot_owner[c.slot]) VS_TRY(capture_totals(idx->plan_slot_owner[c.slot]));   // (eight batches back: long done; its totals move into the result)
  }
  c.pt = reinterpret_cast<PlanTotals*>(idx->pinned + (c.spec ? vs_index::kPinPlanRing + (size_t)c.slot * 8 : vs_index::kPinPlan));
  d.car_width = idx->d.wpc <= 63 ? 2 : 4;
  if (c.spec) {   // table and arena BEFORE the plan: the rows of the regions under the duplicate rule are written on the plan's stream (shared_plan)
    d.A = c.want_rows; d.S = c.want_arena;
    VS_TRY(shared_list_tables(c));
  }
  return VS_OK;
}

// The first kernel of a plan.  src 0: the regions (regions_dev, or the copy in `d`), 1: site records, 2: the sorted copy in `d`.
static void shared_bounds(SharedCtx& c, int src) {
  const dim3 grid(c.ntiles), block(kPlanBlock);
  if (src == 0) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_t6_bounds<0>), grid, block, 0, c.ps, c.idx->d, c.r->d, c.regions_dev, c.items, c.tile_max, c.status);
  else if (src == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_t6_bounds<1>), grid, block, 0, c.ps, c.idx->d, c.r->d, c.site_records, c.items, c.tile_max, c.status);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_t6_bounds<2>), grid, block, 0, c.ps, c.idx->d, c.r->d, (const uint64_t*)nullptr, c.items, c.tile_max, c.status);
}
// One plan pass over the regions as they stand in `d`, on the plan's stream.  Leaves the per-region arrays, runs, coarse and
// slow_list, plan_seq, and the totals in *pt -- waited for here unless the batch is speculative (PlanDev has them for the device).
static int shared_plan(SharedCtx& c, int src) {
  vs_index* idx = c.idx;
  const DevResult& d = c.r->d;
  const dim3 grid(c.ntiles), block(kPlanBlock);
  c.plan_end_enqueued = false;
  shared_bounds(c, src);   // (block 0 clears `status`)
  hipLaunchKernelGGL(k_t6_mid, grid, block, 0, c.ps, idx->d, d, (const ShareMax*)c.tile_max, c.items, c.e_prev, c.e_prev_c, c.tile_sums, c.status);
  const uint64_t seq = ++idx->share_seq;
  hipLaunchKernelGGL(k_t6_totals, dim3(1), block, 0, c.ps, c.tile_sums, c.ntiles, (const uint32_t*)c.status, c.pt, seq, idx->res_entries, c.resident ? 1u : 0u,
                     c.spec ? c.plan_dev : (PlanDev*)nullptr, c.want_rows, c.want_arena);
  c.plan_seq = seq;
  if (c.resident) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_t6_apply<true>), grid, block, 0, c.ps, idx->d, d, (const uint32_t*)c.e_prev, (const uint64_t*)c.e_prev_c, (const Scan5*)c.tile_sums,
                                     c.ntiles, c.items, c.runs, c.coarse, c.slow_list, (const uint32_t*)c.status, idx->res_entries);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_t6_apply<false>), grid, block, 0, c.ps, idx->d, d, (const uint32_t*)c.e_prev, (const uint64_t*)c.e_prev_c, (const Scan5*)c.tile_sums,
                          c.ntiles, c.items, c.runs, c.coarse, c.slow_list, (const uint32_t*)c.status, (uint64_t)0);
  // speculative: the private rows of the regions under the duplicate rule (count and verdict from the plan's record) on the PLAN's stream,
  // beside the previous batch's expansion like the rest of the plan -- the handle's stream then carries the expansion alone
  if (c.spec) hipLaunchKernelGGL(k_t6_slow, dim3((unsigned)((std::min<uint64_t>(c.n, 1024) + 3) / 4)), dim3(256), 0, c.ps, idx->d, d, (const uint32_t*)c.slow_list, (uint64_t)0,
                                 (const PlanDev*)c.plan_dev);
  HIP_TRY(hipGetLastError());
  // the plan's end event, and the handle's stream waiting for it, are enqueued while the plan is still on its way to the totals:
  // two calls less between "the totals are here" and "the expansion is launched" (a batch of a tenth of a millisecond is the host's)
  if (c.plan_aside) {
    HIP_TRY(hipEventRecord(idx->ev[1], c.ps));
    HIP_TRY(hipStreamWaitEvent(idx->stream, idx->ev[1], 0));
    c.plan_end_enqueued = true;
  }
  return c.spec ? VS_OK : wait_posted(idx, &c.pt->seq, seq, 200);   // (a speculative batch: nobody waits here)
}
// A batch that is not sorted by first site: counting sort of the regions over the site index (k_sort_*) on the handle's stream,
// behind a k_t6_bounds that left every region's first site.  Leaves perm, d_user (the caller's arrays) and `d` pointing at sorted
// copies of its per-region arrays; shared_permute_out hands the outcome back at the end.
static int shared_sort(SharedCtx& c) {
  vs_index* idx = c.idx;
  DevResult& d = c.r->d;
  const uint64_t n = c.n, G = idx->d.G;
  uint32_t* count = nullptr;
  unsigned long long* cursor = nullptr;
  VS_TRY(dev_alloc(idx, (G + 2) * 4, (void**)&count, &c.scratch.bufs));
  VS_TRY(dev_alloc(idx, (G + 2) * 8, (void**)&cursor, &c.scratch.bufs));
  VS_TRY(dev_alloc(idx, n * 4, (void**)&c.perm, &c.scratch.bufs));
  HIP_TRY(hipMemsetAsync(count, 0, (G + 1) * 4, idx->stream));
  hipLaunchKernelGGL(k_sort_hist, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, idx->stream, d, count);
  VS_TRY(exclusive_scan<uint32_t>(idx, (const uint32_t*)count, G + 1, (uint64_t*)cursor, &c.scratch.bufs));
  hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, idx->stream, d, cursor, c.perm);
  c.d_user = d;
  uint64_t* sregions = nullptr;
  VS_TRY(region_arrays(d, &sregions, n, [&](auto** p, uint64_t k) { return dev_alloc(idx, k * sizeof(**p), (void**)p, &c.scratch.bufs); }));
  hipLaunchKernelGGL(k_permute_in, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, idx->stream, c.d_user, d, (const uint32_t*)c.perm, sregions);
  d.regions = sregions;
  HIP_TRY(hipGetLastError());
  return VS_OK;
}
// The policy around the two: a handle whose last batch needed sorting sorts first (it looks at the order as given again every
// 32nd batch); a speculative batch leaves the verdict to the device; every other batch waits for its totals and sorts when they
// say so.  Leaves a planned batch, ev[1] behind the plan, the handle's sort hint (list batches only).
static int shared_plan_batch(SharedCtx& c) {
  vs_index* idx = c.idx;
  const int src = c.site_records ? 1 : 0;
  if (c.sort_first) {
    --idx->sort_probe_in;
    shared_bounds(c, src);
    VS_TRY(shared_sort(c));
    VS_TRY(shared_plan(c, 2));
  } else if (c.spec) {
    VS_TRY(shared_plan(c, src));   // (sorted or not is the device's verdict)
  } else {
    VS_TRY(shared_plan(c, src));
    if (c.pt->not_sorted) {
      if (c.plan_aside) {   // the sort and the second plan run on the handle's stream (behind the plan stream's work so far)
        HIP_TRY(hipStreamSynchronize(c.ps));
        c.plan_aside = false; c.ps = idx->stream;
      }
      VS_TRY(shared_sort(c));
      VS_TRY(shared_plan(c, 2));
      if (c.lists) { idx->sort_hint = true; idx->sort_probe_in = 32; }
    } else if (c.lists) idx->sort_hint = false;
  }
  if (!c.spec && c.pt->not_sorted) return fail(VS_ERR_INTERNAL, "the batch is not sorted by first site after the device-side sort");
  if (!c.plan_end_enqueued) HIP_TRY(hipEventRecord(idx->ev[1], c.ps));   // (a plan on the handle's own stream: the phase boundary only)
  return VS_OK;
}

// The plan's rows are known: grouped counts beyond the limit (rows x groups records of 16 bytes) are refused here, before they or the
// table are allocated.
static int group_counts_fit(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const uint64_t cap = idx->opts.matrix_max_mib ? (uint64_t)idx->opts.matrix_max_mib << 20 : 32ull << 30;
  const uint64_t row_bytes = 16ull * c.req.n_cols;
  if (r->d.A <= cap / row_bytes) return VS_OK;
  (void)hipStreamSynchronize(c.ps);   // (the plan's last kernels still read the call's temporaries: they go back to the pool on return)
  (void)hipStreamSynchronize(idx->stream);
  return fail(VS_ERR_ARG, "grouped counts of %llu rows x %u groups take %llu bytes, more than the limit of %llu MiB (option matrix_max_mib): split the batch",
              (unsigned long long)r->d.A, c.req.n_cols, (unsigned long long)(r->d.A * row_bytes), (unsigned long long)(cap >> 20));
}
// A window-statistics batch: the temporary grouped counts (rows x groups x 16 bytes) and the answer (regions x (48 groups + 16 pairs)
// bytes) together, under the same limit, before either or the table is allocated.
static int window_stats_fit(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const uint64_t cap = idx->opts.matrix_max_mib ? (uint64_t)idx->opts.matrix_max_mib << 20 : 32ull << 30;
  const uint64_t row_bytes = 16ull * c.req.n_cols, region_bytes = 48ull * c.req.n_cols + 16ull * c.req.ws_pairs;   // (at most 1 KiB and 35 KiB)
  if (r->d.Q <= cap / region_bytes && r->d.A <= (cap - r->d.Q * region_bytes) / row_bytes) return VS_OK;
  (void)hipStreamSynchronize(c.ps);   // (the plan's last kernels still read the call's temporaries: they go back to the pool on return)
  (void)hipStreamSynchronize(idx->stream);
  return fail(VS_ERR_ARG, "the window statistics of %llu regions over %llu rows x %u groups take %llu bytes (%llu of the grouped counts they are reduced from, "
              "%llu of the records), more than the limit of %llu MiB (option matrix_max_mib): split the batch", (unsigned long long)r->d.Q, (unsigned long long)r->d.A,
              c.req.n_cols, (unsigned long long)(r->d.A * row_bytes + r->d.Q * region_bytes), (unsigned long long)(r->d.A * row_bytes),
              (unsigned long long)(r->d.Q * region_bytes), (unsigned long long)(cap >> 20));
}
// The plan's rows are known: an association scan beyond the limit (rows x traits cells of 8 bytes and the rows' count records) is
// refused here, before they or the table are allocated.
static int assoc_fits(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const uint64_t cap = idx->opts.matrix_max_mib ? (uint64_t)idx->opts.matrix_max_mib << 20 : 32ull << 30;
  const uint64_t row_bytes = 8ull * c.req.n_traits + 16;
  if (r->d.A <= cap / row_bytes) return VS_OK;
  (void)hipStreamSynchronize(c.ps);   // (the plan's last kernels still read the call's temporaries: they go back to the pool on return)
  (void)hipStreamSynchronize(idx->stream);
  return fail(VS_ERR_ARG, "an association scan of %llu rows x %u traits takes %llu bytes, more than the limit of %llu MiB (option matrix_max_mib): split the batch",
              (unsigned long long)r->d.A, c.req.n_traits, (unsigned long long)(r->d.A * row_bytes), (unsigned long long)(cap >> 20));
}
// The plan's rows are known: a genotype matrix beyond the limit is refused here, before it or the table is allocated.
// An LD batch: the temporary matrix and the band together, under the same limit.
static int matrix_fits(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const uint64_t cap = idx->opts.matrix_max_mib ? (uint64_t)idx->opts.matrix_max_mib << 20 : 32ull << 30;
  r->mx_pitch = ((uint64_t)c.req.n_cols + 15) & ~15ull;
  const uint64_t row_bytes = r->mx_pitch + (c.req.kind == ReqKind::LD ? 4ull * c.req.ld_window : 0);
  if (r->d.A <= cap / row_bytes) return VS_OK;
  (void)hipStreamSynchronize(c.ps);   // (the plan's last kernels still read the call's temporaries: they go back to the pool on return)
  (void)hipStreamSynchronize(idx->stream);
  if (c.req.kind == ReqKind::LD)
    return fail(VS_ERR_ARG, "an LD band of %llu rows x %u columns with window %u takes %llu bytes (%llu of the genotype matrix it is formed from, %llu of the band), "
                "more than the limit of %llu MiB (option matrix_max_mib): split the batch", (unsigned long long)r->d.A, c.req.n_cols, c.req.ld_window,
                (unsigned long long)(r->d.A * row_bytes), (unsigned long long)(r->d.A * r->mx_pitch), (unsigned long long)(r->d.A * 4 * c.req.ld_window),
                (unsigned long long)(cap >> 20));
  return fail(VS_ERR_ARG, "a genotype matrix of %llu rows x %u columns takes %llu bytes (rows %llu bytes apart), more than the limit of %llu MiB "
              "(option matrix_max_mib): split the batch", (unsigned long long)r->d.A, c.req.n_cols, (unsigned long long)(r->d.A * r->mx_pitch),
              (unsigned long long)r->mx_pitch, (unsigned long long)(cap >> 20));
}
// A Gram batch: the temporary matrix and the n x n cells -- 8 bytes each, 16 under VS_GRAM_GRM -- together, under the same limit.
static int gram_fits(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const uint64_t cap = idx->opts.matrix_max_mib ? (uint64_t)idx->opts.matrix_max_mib << 20 : 32ull << 30;
  r->mx_pitch = ((uint64_t)c.req.n_cols + 15) & ~15ull;
  const uint64_t n = c.req.n_cols, cell_bytes = n * n * (c.req.gram_stat == VS_GRAM_GRM ? 16ull : 8ull);
  if (cell_bytes <= cap && r->d.A <= (cap - cell_bytes) / r->mx_pitch) return VS_OK;
  (void)hipStreamSynchronize(c.ps);   // (the plan's last kernels still read the call's temporaries: they go back to the pool on return)
  (void)hipStreamSynchronize(idx->stream);
  return fail(VS_ERR_ARG, "a Gram matrix of %llu rows x %u columns takes %llu bytes (%llu of the genotype matrix it is formed from, %llu of the %u x %u cells), "
              "more than the limit of %llu MiB (option matrix_max_mib): split the batch or the samples", (unsigned long long)r->d.A, c.req.n_cols,
              (unsigned long long)(r->d.A * r->mx_pitch + cell_bytes), (unsigned long long)(r->d.A * r->mx_pitch), (unsigned long long)cell_bytes, c.req.n_cols,
              c.req.n_cols, (unsigned long long)(cap >> 20));
}
// An IBS batch: the temporary matrix and the n x n cells -- five int64 matrices, 40 bytes a cell, 48 under VS_IBS_KING -- together,
// under the same limit.
static int ibs_fits(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const uint64_t cap = idx->opts.matrix_max_mib ? (uint64_t)idx->opts.matrix_max_mib << 20 : 32ull << 30;
  r->mx_pitch = ((uint64_t)c.req.n_cols + 15) & ~15ull;
  const uint64_t n = c.req.n_cols, cell_bytes = n * n * (c.req.ibs_stat == VS_IBS_KING ? 48ull : 40ull);
  if (cell_bytes <= cap && r->d.A <= (cap - cell_bytes) / r->mx_pitch) return VS_OK;
  (void)hipStreamSynchronize(c.ps);   // (the plan's last kernels still read the call's temporaries: they go back to the pool on return)
  (void)hipStreamSynchronize(idx->stream);
  return fail(VS_ERR_ARG, "IBS matrices of %llu rows x %u columns take %llu bytes (%llu of the genotype matrix they are formed from, %llu of the %u x %u cells), "
              "more than the limit of %llu MiB (option matrix_max_mib): split the batch or the samples", (unsigned long long)r->d.A, c.req.n_cols,
              (unsigned long long)(r->d.A * r->mx_pitch + cell_bytes), (unsigned long long)(r->d.A * r->mx_pitch), (unsigned long long)cell_bytes, c.req.n_cols,
              c.req.n_cols, (unsigned long long)(cap >> 20));
}
// A trait-matrix association batch: the temporary matrix, the rows x K cells of 8 bytes, the rows' count records and the limb panel
// together, under the same limit.
static uint64_t am_meta_words(uint32_t K) { return (3ull * K + 1) & ~1ull; }   // Sy, vy and the shifts (8 bytes each), the panel behind them 16-byte aligned
static int assoc_matrix_fits(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const uint64_t cap = idx->opts.matrix_max_mib ? (uint64_t)idx->opts.matrix_max_mib << 20 : 32ull << 30;
  r->mx_pitch = ((uint64_t)c.req.n_cols + 15) & ~15ull;
  const uint64_t K = c.req.n_traits, panel_bytes = (uint64_t)c.req.am->tiles * kAmTileRows * r->mx_pitch;
  const uint64_t row_bytes = r->mx_pitch + 8 * K + 16;   // (at most 16 + 2^22 + 2^19: no overflow below)
  if (panel_bytes <= cap && r->d.A <= (cap - panel_bytes) / row_bytes) return VS_OK;
  (void)hipStreamSynchronize(c.ps);   // (the plan's last kernels still read the call's temporaries: they go back to the pool on return)
  (void)hipStreamSynchronize(idx->stream);
  return fail(VS_ERR_ARG, "a trait-matrix association scan of %llu rows x %u columns x %u traits takes %llu bytes (%llu of the genotype matrix it is formed from, "
              "%llu of the cells, %llu of the count records, %llu of the limb panel), more than the limit of %llu MiB (option matrix_max_mib): split the batch or the traits",
              (unsigned long long)r->d.A, c.req.n_cols, c.req.n_traits, (unsigned long long)(r->d.A * row_bytes + panel_bytes), (unsigned long long)(r->d.A * r->mx_pitch),
              (unsigned long long)(r->d.A * 8 * K), (unsigned long long)(r->d.A * 16), (unsigned long long)panel_bytes, (unsigned long long)(cap >> 20));
}
// A pruning batch: the temporary matrix, the hit masks, the state bytes and the per-region words together, under the same limit.
// `states`: the number of verdicts, 0 while the scan has not given it (shared_tables: what is known by then already decides most
// refusals, before anything is allocated).
static int prune_fits(SharedCtx& c, uint64_t states) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const uint64_t cap = idx->opts.matrix_max_mib ? (uint64_t)idx->opts.matrix_max_mib << 20 : 32ull << 30;
  r->mx_pitch = ((uint64_t)c.req.n_cols + 15) & ~15ull;
  const uint64_t mask_row = 4ull * ((c.req.ld_window + 31) / 32), row_bytes = r->mx_pitch + mask_row;
  const uint64_t region_bytes = 8 * (2 * (r->d.Q + 1) + 4);   // (Q < 2^32)
  if (region_bytes <= cap && states <= cap - region_bytes && r->d.A <= (cap - region_bytes - states) / row_bytes) return VS_OK;
  (void)hipStreamSynchronize(c.ps);   // (the plan's last kernels still read the call's temporaries: they go back to the pool on return)
  (void)hipStreamSynchronize(idx->stream);
  return fail(VS_ERR_ARG, "an LD pruning of %llu regions over %llu rows x %u columns with window %u takes %llu bytes (%llu of the genotype matrix it is formed from, "
              "%llu of the hit masks, %llu of the verdicts, %llu of the per-region arrays), more than the limit of %llu MiB (option matrix_max_mib): split the batch",
              (unsigned long long)r->d.Q, (unsigned long long)r->d.A, c.req.n_cols, c.req.ld_window, (unsigned long long)(r->d.A * row_bytes + states + region_bytes),
              (unsigned long long)(r->d.A * r->mx_pitch), (unsigned long long)(r->d.A * mask_row), (unsigned long long)states, (unsigned long long)region_bytes,
              (unsigned long long)(cap >> 20));
}
// A clumping batch: per table row the temporary matrix, the hit masks, the key (8 bytes) and the class (1 byte); per verdict the
// state (1 byte), the owner (4 bytes) and the blocker masks (two masks); the per-region words.  All together under the same limit,
// `states` as for prune_fits.
static int clump_fits(SharedCtx& c, uint64_t states) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const uint64_t cap = idx->opts.matrix_max_mib ? (uint64_t)idx->opts.matrix_max_mib << 20 : 32ull << 30;
  r->mx_pitch = ((uint64_t)c.req.n_cols + 15) & ~15ull;
  const uint64_t mask_row = 4ull * ((c.req.ld_window + 31) / 32), row_bytes = r->mx_pitch + mask_row + 9, slot_bytes = 5 + 2 * mask_row;
  const uint64_t region_bytes = 8 * (3 * (r->d.Q + 1) + 4);   // (Q < 2^32)
  if (region_bytes <= cap && states <= (cap - region_bytes) / slot_bytes && r->d.A <= (cap - region_bytes - states * slot_bytes) / row_bytes) return VS_OK;
  (void)hipStreamSynchronize(c.ps);   // (the plan's last kernels still read the call's temporaries: they go back to the pool on return)
  (void)hipStreamSynchronize(idx->stream);
  return fail(VS_ERR_ARG, "an LD clumping of %llu regions over %llu rows x %u columns with window %u takes %llu bytes (%llu of the genotype matrix it is formed from, "
              "%llu of the hit masks, %llu of the keys and classes, %llu of the blocker masks, %llu of the verdicts and owners, %llu of the per-region arrays), more than "
              "the limit of %llu MiB (option matrix_max_mib): split the batch",
              (unsigned long long)r->d.Q, (unsigned long long)r->d.A, c.req.n_cols, c.req.ld_window,
              (unsigned long long)(r->d.A * row_bytes + states * slot_bytes + region_bytes), (unsigned long long)(r->d.A * r->mx_pitch),
              (unsigned long long)(r->d.A * mask_row), (unsigned long long)(r->d.A * 9), (unsigned long long)(states * 2 * mask_row), (unsigned long long)(states * 5),
              (unsigned long long)region_bytes, (unsigned long long)(cap >> 20));
}
// An LD-score batch: the temporary matrix, 13 bytes per slot (8 of the sum, 4 of the pair count, 1 of the state) and the per-region
// words together, under the same limit.  `slots` as prune_fits' `states`.
static int ldscore_fits(SharedCtx& c, uint64_t slots) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const uint64_t cap = idx->opts.matrix_max_mib ? (uint64_t)idx->opts.matrix_max_mib << 20 : 32ull << 30;
  r->mx_pitch = ((uint64_t)c.req.n_cols + 15) & ~15ull;
  const uint64_t region_bytes = 8 * (3 * (r->d.Q + 1) + 6);   // (Q < 2^32)
  if (region_bytes <= cap && slots <= (cap - region_bytes) / 13 && r->d.A <= (cap - region_bytes - slots * 13) / r->mx_pitch) return VS_OK;
  (void)hipStreamSynchronize(c.ps);   // (the plan's last kernels still read the call's temporaries: they go back to the pool on return)
  (void)hipStreamSynchronize(idx->stream);
  return fail(VS_ERR_ARG, "the LD scores of %llu regions over %llu rows x %u columns take %llu bytes (%llu of the genotype matrix they are formed from, "
              "%llu of the sums, pair counts and states, %llu of the per-region arrays), more than the limit of %llu MiB (option matrix_max_mib): split the batch",
              (unsigned long long)r->d.Q, (unsigned long long)r->d.A, c.req.n_cols, (unsigned long long)(r->d.A * r->mx_pitch + slots * 13 + region_bytes),
              (unsigned long long)(r->d.A * r->mx_pitch), (unsigned long long)(slots * 13), (unsigned long long)region_bytes, (unsigned long long)(cap >> 20));
}
// A trio batch: the temporary matrix, the count records, both record arrays and the trio table together, under the same limit; and
// a table of 2^31 rows or more is refused, because a per-trio sum (at most 2 a row) must fit uint32.
static int trio_fits(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const uint64_t cap = idx->opts.matrix_max_mib ? (uint64_t)idx->opts.matrix_max_mib << 20 : 32ull << 30;
  r->mx_pitch = ((uint64_t)c.req.n_cols + 15) & ~15ull;
  const uint64_t trio_part = c.req.n_trios * 28, row_bytes = r->mx_pitch + 32;   // (at most 2^20 trios)
  const bool rows_fit = r->d.A < (1ull << 31);
  if (rows_fit && trio_part <= cap && r->d.A <= (cap - trio_part) / row_bytes) return VS_OK;
  (void)hipStreamSynchronize(c.ps);   // (the plan's last kernels still read the call's temporaries: they go back to the pool on return)
  (void)hipStreamSynchronize(idx->stream);
  if (!rows_fit)
    return fail(VS_ERR_ARG, "a trio scan over %llu rows: a trio's sums are 32-bit, the table may have at most 2^31 - 1 rows: split the batch", (unsigned long long)r->d.A);
  return fail(VS_ERR_ARG, "a trio scan of %llu rows x %u columns x %llu trios takes %llu bytes (%llu of the genotype matrix it is formed from, %llu of the count "
              "records, %llu of the records per row, %llu of the records per trio, %llu of the trio table), more than the limit of %llu MiB (option matrix_max_mib): "
              "split the batch or the trios", (unsigned long long)r->d.A, c.req.n_cols, (unsigned long long)c.req.n_trios,
              (unsigned long long)(r->d.A * row_bytes + trio_part), (unsigned long long)(r->d.A * r->mx_pitch), (unsigned long long)(r->d.A * 16),
              (unsigned long long)(r->d.A * 16), (unsigned long long)(c.req.n_trios * 16), (unsigned long long)(c.req.n_trios * 12), (unsigned long long)(cap >> 20));
}
// A ROH batch: the temporary matrix, the count records and the walk's 8 bytes a row; per (region, column) the summary (32 bytes) and
// -- with segments -- seg_begin (8) and the scan's input (4); n_sites; the segments (32 bytes each; `segs` is 0 until pass 1 has
// counted them).  All together under the same limit; and a table of 2^31 rows or more is refused (row offsets and site counts are 32-bit).
static int roh_fits(SharedCtx& c, uint64_t segs) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const uint64_t cap = idx->opts.matrix_max_mib ? (uint64_t)idx->opts.matrix_max_mib << 20 : 32ull << 30;
  r->mx_pitch = ((uint64_t)c.req.n_cols + 15) & ~15ull;
  const bool rows_fit = r->d.A < (1ull << 31);
  const unsigned __int128 cells = (unsigned __int128)r->d.Q * c.req.n_cols;
  const unsigned __int128 row_part = (unsigned __int128)r->d.A * (r->mx_pitch + 24), cell_part = cells * (c.req.roh.segments ? 44u : 32u) + (unsigned __int128)r->d.Q * 4 + 64,
                          seg_part = (unsigned __int128)segs * 32, need = row_part + cell_part + seg_part;
  if (rows_fit && need <= cap) return VS_OK;
  (void)hipStreamSynchronize(c.ps);   // (the plan's last kernels still read the call's temporaries: they go back to the pool on return)
  (void)hipStreamSynchronize(idx->stream);
  if (!rows_fit)
    return fail(VS_ERR_ARG, "a ROH batch over %llu rows: row offsets and site counts are 32-bit, the table may have at most 2^31 - 1 rows: split the batch", (unsigned long long)r->d.A);
  auto sat = [](unsigned __int128 v) { return v > ~0ull ? ~0ull : (unsigned long long)v; };
  return fail(VS_ERR_ARG, "a ROH batch of %llu regions x %u columns over %llu rows with %llu segments takes %llu bytes (%llu of the genotype matrix it walks, %llu of the "
              "count records and site words, %llu of the summaries and per-cell words, %llu of the segments), more than the limit of %llu MiB (option matrix_max_mib): "
              "split the batch or the samples", (unsigned long long)r->d.Q, c.req.n_cols, (unsigned long long)r->d.A, (unsigned long long)segs, sat(need),
              sat((unsigned __int128)r->d.A * r->mx_pitch), sat((unsigned __int128)r->d.A * 24), sat(cell_part), sat(seg_part), (unsigned long long)(cap >> 20));
}
// Reads the totals (*pt) or the speculation.  Leaves U / n_slow / n_runs, the result's sizes and bookkeeping, a speculative batch
// registered with its slot, what the request's kind allocates, and the form of the rows and the expansion (n_fill .. lean).
static int shared_tables(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  DevResult& d = r->d;
  const SharedReq& q = c.req;
  const PlanTotals* pt = c.pt;
  // (speculative: every size below is what was ALLOCATED -- an upper bound the launches are made for; the kernels take the real ones from PlanDev)
  c.U = c.spec ? c.want_rows : pt->shared_rows; c.n_slow = c.spec ? 0 : pt->n_slow; c.n_runs = c.spec ? 0 : pt->n_runs;
  if (!c.spec) { d.A = pt->rows; d.S = c.lists ? pt->arena : 0; }
  r->n_rows_reported = c.spec ? 0 : pt->reported;
  if (c.spec) {
    r->sizes_pending = true; r->totals_captured = false; r->plan_slot = c.slot; r->plan_seq = c.plan_seq; r->cap_rows = c.want_rows; r->cap_arena = c.want_arena;
    idx->plan_slot_owner[c.slot] = r;
    idx->t6_speculated++;
  } else if (c.lists) t6_hint_update(idx, c.n, pt->rows, pt->arena);
  c.n_fill = c.lists && !c.resident ? c.U : 0;
  r->shared_lists = true;
  r->resident = c.resident;
  r->scattered_lists = false;
  r->n_unique_sites = c.n_fill;
  switch (q.kind) {
    case ReqKind::Lists:
      if (!c.spec) VS_TRY(shared_list_tables(c));   // (speculative: taken in front of the plan)
      break;
    case ReqKind::Counts:
      VS_TRY(ralloc(r, d.A, &d.rows));
      VS_TRY(ralloc(r, d.A, &r->d_counts));
      break;
    case ReqKind::Groups:
      VS_TRY(group_counts_fit(c));
      VS_TRY(ralloc(r, d.A, &d.rows));
      VS_TRY(ralloc(r, (size_t)(d.A * q.n_cols), &r->d_counts));
      break;
    case ReqKind::WindowStats:   // (the grouped counts are a temporary like an LD batch's matrix: the reduction alone reads them)
      VS_TRY(window_stats_fit(c));
      VS_TRY(ralloc(r, d.A, &d.rows));
      VS_TRY(dev_alloc(idx, (size_t)(d.A * q.n_cols) * sizeof(uint4), (void**)&c.ws_counts, &c.ld_tmp.bufs));
      VS_TRY(ralloc(r, (size_t)d.Q * (48 * (size_t)q.n_cols + 16 * (size_t)q.ws_pairs), &r->d_wstats));
      VS_TRY(ralloc(r, 2, &r->d_cell_total));   // (the second word: the number of chunks of the split regions)
      r->ws_pairs = q.ws_pairs;
      break;
    case ReqKind::Assoc:
      VS_TRY(assoc_fits(c));
      VS_TRY(ralloc(r, d.A, &d.rows));
      VS_TRY(ralloc(r, d.A, &r->d_counts));
      VS_TRY(ralloc(r, (size_t)(d.A * q.n_traits), &r->d_scores));
      break;
    case ReqKind::Scores:   // (the sums and what they are formed from wait for the number of reports: launch_scores)
      VS_TRY(ralloc(r, d.A, &d.rows));
      VS_TRY(ralloc(r, 1, &r->d_score_meta));
      break;
    case ReqKind::Burden:
      VS_TRY(ralloc(r, d.A, &d.rows));
      if (q.window()) VS_TRY(ralloc(r, d.A, &r->d_counts));   // (the filter's input, made only under a window)
      VS_TRY(ralloc(r, (size_t)c.n * q.n_cols, &r->d_cells));
      VS_TRY(ralloc(r, 2, &r->d_cell_total));   // (+ the number of chunks of the split regions)
      break;
    case ReqKind::Matrix:
      VS_TRY(matrix_fits(c));
      VS_TRY(ralloc(r, d.A, &d.rows));
      VS_TRY(ralloc(r, (size_t)(d.A * r->mx_pitch), &r->d_matrix));
      VS_TRY(ralloc(r, 2, &r->d_cell_total));
      break;
    case ReqKind::LD: {   // (the matrix kernel's count of nonzero cells lives in the band's buffer, behind the band)
      VS_TRY(matrix_fits(c));
      VS_TRY(ralloc(r, d.A, &d.rows));
      VS_TRY(dev_alloc(idx, (size_t)(d.A * r->mx_pitch), (void**)&c.ld_matrix, &c.ld_tmp.bufs));
      VS_TRY(ralloc(r, d.A, &r->d_counts));
      const size_t band_words = ((size_t)d.A * q.ld_window + 3) & ~(size_t)3;
      VS_TRY(ralloc(r, band_words + 4, &r->d_band));
      r->d_cell_total = reinterpret_cast<unsigned long long*>(r->d_band + band_words);
      r->ld_window = q.ld_window; r->ld_stat = q.ld_stat;
      break;
    }
    case ReqKind::Gram: {   // (the matrix kernel's count of nonzero cells lives behind C and H)
      VS_TRY(gram_fits(c));
      VS_TRY(ralloc(r, d.A, &d.rows));
      VS_TRY(dev_alloc(idx, (size_t)(d.A * r->mx_pitch), (void**)&c.ld_matrix, &c.ld_tmp.bufs));
      VS_TRY(ralloc(r, d.A, &r->d_counts));
      const size_t nn = (size_t)q.n_cols * q.n_cols, head = nn + q.n_cols + 2;
      r->gram_grm_off = head + 2;
      r->gram_words = r->gram_grm_off + (q.gram_stat == VS_GRAM_GRM ? nn : 0);
      VS_TRY(ralloc(r, r->gram_words, &r->d_gram));
      r->d_cell_total = reinterpret_cast<unsigned long long*>(r->d_gram + head);
      r->gram_stat = q.gram_stat;
      break;
    }
    case ReqKind::Ibs: {   // (the matrix kernel's count of nonzero cells lives behind n_used)
      VS_TRY(ibs_fits(c));
      VS_TRY(ralloc(r, d.A, &d.rows));
      VS_TRY(dev_alloc(idx, (size_t)(d.A * r->mx_pitch), (void**)&c.ld_matrix, &c.ld_tmp.bufs));
      VS_TRY(ralloc(r, d.A, &r->d_counts));
      const size_t nn = (size_t)q.n_cols * q.n_cols, head = 5 * nn + 1;
      r->ibs_king_off = head + 2;
      r->ibs_words = r->ibs_king_off + (q.ibs_stat == VS_IBS_KING ? nn : 0);
      VS_TRY(ralloc(r, r->ibs_words, &r->d_ibs));
      r->d_cell_total = reinterpret_cast<unsigned long long*>(r->d_ibs + head);
      r->ibs_stat = q.ibs_stat;
      break;
    }
    case ReqKind::Trio: {   // (n_used and the matrix kernel's count of nonzero cells live behind the records, the trio table behind them)
      VS_TRY(trio_fits(c));
      VS_TRY(ralloc(r, d.A, &d.rows));
      VS_TRY(dev_alloc(idx, (size_t)(d.A * r->mx_pitch), (void**)&c.ld_matrix, &c.ld_tmp.bufs));
      VS_TRY(ralloc(r, d.A, &r->d_counts));
      const size_t head = (size_t)(d.A + q.n_trios) * 16 + 8;
      r->trio_table_off = (head + 16 + 15) & ~(size_t)15;
      r->trio_bytes = r->trio_table_off + (size_t)q.n_trios * 12;
      VS_TRY(ralloc(r, r->trio_bytes, &r->d_trio));
      r->d_cell_total = reinterpret_cast<unsigned long long*>(r->d_trio + head);
      r->n_trios = q.n_trios;
      break;
    }
    case ReqKind::Roh: {   // (n_sites and the matrix kernel's count of nonzero cells live behind the summaries, seg_begin behind them; the segments wait for pass 1: launch_roh)
      VS_TRY(roh_fits(c, 0));
      VS_TRY(ralloc(r, d.A, &d.rows));
      VS_TRY(dev_alloc(idx, (size_t)(d.A * r->mx_pitch), (void**)&c.ld_matrix, &c.ld_tmp.bufs));
      VS_TRY(ralloc(r, d.A, &r->d_counts));
      const size_t cells = (size_t)d.Q * q.n_cols;
      r->roh_sites_off = cells * 32;
      const size_t head = r->roh_sites_off + (((size_t)d.Q * 4 + 15) & ~(size_t)15);
      r->roh_begin_off = head + 16;
      r->roh_bytes = r->roh_begin_off + (q.roh.segments ? (cells + 1) * 8 : 0);
      VS_TRY(ralloc(r, r->roh_bytes, &r->d_roh));
      r->d_cell_total = reinterpret_cast<unsigned long long*>(r->d_roh + head);
      r->roh = q.roh;
      break;
    }
    case ReqKind::AssocMatrix: {   // (the traits' words and the limb panel are temporaries like the matrix: the kernel alone reads them)
      VS_TRY(assoc_matrix_fits(c));
      VS_TRY(ralloc(r, d.A, &d.rows));
      VS_TRY(dev_alloc(idx, (size_t)(d.A * r->mx_pitch), (void**)&c.ld_matrix, &c.ld_tmp.bufs));
      VS_TRY(dev_alloc(idx, (size_t)(am_meta_words(q.n_traits) * 8 + q.am->n_bytes()), (void**)&c.am_dev, &c.ld_tmp.bufs));
      VS_TRY(ralloc(r, d.A, &r->d_counts));
      VS_TRY(ralloc(r, (size_t)(d.A * q.n_traits), &r->d_scores));
      VS_TRY(ralloc(r, 2, &r->d_cell_total));
      break;
    }
    case ReqKind::ScoreMatrix:   // (the temporary matrix, the sums and what they are formed from wait for the number of reports: launch_score_matrix)
      r->mx_pitch = ((uint64_t)q.n_cols + 15) & ~15ull;
      VS_TRY(ralloc(r, d.A, &d.rows));
      VS_TRY(ralloc(r, d.A, &r->d_counts));
      VS_TRY(ralloc(r, 2, &r->d_cell_total));
      break;
    case ReqKind::LdMatrix:   // (the temporary matrix and the cells wait for the blocks' sizes: ld_matrix_tables, behind the permutation)
      r->mx_pitch = ((uint64_t)q.n_cols + 15) & ~15ull;
      VS_TRY(ralloc(r, d.A, &d.rows));
      VS_TRY(ralloc(r, d.A, &r->d_counts));
      VS_TRY(ralloc(r, 2 * (size_t)(d.Q + 1) + 6, &r->d_ldm_meta));
      r->d_cell_total = reinterpret_cast<unsigned long long*>(r->d_ldm_meta + 2 * (d.Q + 1) + 4);
      r->ld_stat = q.ld_stat;
      break;
    case ReqKind::Prune:   // (the temporary matrix, the masks and the state wait for the number of verdicts: prune_tables, behind the permutation)
      VS_TRY(prune_fits(c, 0));
      VS_TRY(ralloc(r, d.A, &d.rows));
      VS_TRY(ralloc(r, d.A, &r->d_counts));
      VS_TRY(ralloc(r, 2 * (size_t)(d.Q + 1) + 4, &r->d_prune_meta));
      r->d_cell_total = reinterpret_cast<unsigned long long*>(r->d_prune_meta + 2 * (d.Q + 1) + 2);
      r->ld_window = q.ld_window;
      r->prune_max_bp = q.prune_max_bp; r->prune_T = q.prune_T; r->prune_min_ac = q.prune_min_ac; r->prune_max_ac = q.prune_max_ac;
      break;
    case ReqKind::Clump:   // (as Prune: the keys, the temporaries, the state and the owners wait for clump_tables, behind the permutation)
      VS_TRY(clump_fits(c, 0));
      VS_TRY(ralloc(r, d.A, &d.rows));
      VS_TRY(ralloc(r, d.A, &r->d_counts));
      VS_TRY(ralloc(r, 3 * (size_t)(d.Q + 1) + 4, &r->d_prune_meta));
      r->d_cell_total = reinterpret_cast<unsigned long long*>(r->d_prune_meta + 2 * (d.Q + 1) + 2);
      r->ld_window = q.ld_window;
      r->prune_max_bp = q.prune_max_bp; r->prune_T = q.prune_T;
      break;
    case ReqKind::LdScore:   // (as Prune: the temporary matrix and the slots wait for ldscore_tables, behind the permutation)
      VS_TRY(ldscore_fits(c, 0));
      VS_TRY(ralloc(r, d.A, &d.rows));
      VS_TRY(ralloc(r, d.A, &r->d_counts));
      VS_TRY(ralloc(r, 3 * (size_t)(d.Q + 1) + 6, &r->d_prune_meta));
      r->d_cell_total = reinterpret_cast<unsigned long long*>(r->d_prune_meta + 3 * (d.Q + 1) + 4);
      r->ld_window = q.ld_window;
      r->prune_max_bp = q.prune_max_bp; r->prune_min_ac = q.prune_min_ac; r->prune_max_ac = q.prune_max_ac;
      break;
  }
  c.async_fill = c.allow_async && idx->opts.async_fill && c.n_fill > 0;
  c.fused = idx->opts.fill_fused && c.lists && !c.resident && !c.async_fill;
  // Every event on a stream is a packet the GPU works through (~3 us each): the default batch -- async_submit, rows and lists in one
  // launch, no permutation -- records TWO on the handle's stream, the result's own pair around the expansion, and its phase
  // times are read from those (round 3 recorded five per batch, and this round's completion event would have made it eight).
  c.lean = c.async_submit && c.fused && c.n_fill > 0 && !c.perm;
  return VS_OK;
}

// Leaves the table's rows -- the private ones of the regions under the duplicate rule, the shared ones unless the expansion
// writes them (fused) -- and u_site; ev[2] / ev[3] around them unless lean.
static int shared_rows(SharedCtx& c) {
  vs_index* idx = c.idx;
  const DevResult& d = c.r->d;
  if (!c.lean) HIP_TRY(hipEventRecord(idx->ev[2], idx->stream));
  const unsigned slow_blocks = (unsigned)((std::min<uint64_t>(c.n_slow, 16384) + 3) / 4);
  if (c.n_slow)   // (a speculative batch launched the kernel behind its plan, with the count from the plan's record)
    hipLaunchKernelGGL(k_t6_slow, dim3(slow_blocks), dim3(256), 0, idx->stream, idx->d, d, (const uint32_t*)c.slow_list, c.n_slow, (const PlanDev*)nullptr);
  if (!c.lists && d.A) VS_TRY(dev_alloc(idx, d.A * 4 + 8, (void**)&c.u_site, &c.scratch.bufs));   // (a column request: the private rows' sites too)
  if (c.U && !c.fused) {
    if (c.n_fill) VS_TRY(dev_alloc(idx, c.U * 4 + 8, (void**)&c.u_site, &c.scratch.bufs));
    hipLaunchKernelGGL(k_share_rows2, dim3((unsigned)((c.U + 255) / 256)), dim3(256), 0, idx->stream, idx->d, d, (const RunRec*)c.runs, (const uint32_t*)c.coarse, c.n_runs, c.U, c.u_site);
  }
  HIP_TRY(hipGetLastError());
  if (!c.lean) HIP_TRY(hipEventRecord(idx->ev[3], idx->stream));
  if (!c.lists && d.A && c.n_slow)   // the private rows' sites behind the shared ones
    hipLaunchKernelGGL(k_count_slow_sites, dim3(slow_blocks), dim3(256), 0, idx->stream, d, (const uint32_t*)c.slow_list, c.n_slow, c.u_site);
  return VS_OK;
}

#ifdef VS_TUNING
// option fill_stats: the per-task clocks k_fill_sites2 left in tstat, read back and summed up on stderr
static int print_fill_stats(vs_index* idx, const unsigned long long* tstat, uint64_t nt, uint32_t chunk) {
  std::vector<uint32_t> h(nt * 4);
  HIP_TRY(hipMemcpyAsync(h.data(), tstat, nt * 16, hipMemcpyDeviceToHost, idx->stream));
  HIP_TRY(hipStreamSynchronize(idx->stream));
  double sp = 0, sl = 0, sd = 0, st = 0, nd = 0; uint32_t mx = 0;
  for (uint64_t t = 0; t < nt; ++t) {
    const uint32_t tot = h[4 * t + 3] & 0xFFFFFFu;
    sp += h[4 * t]; sl += h[4 * t + 1]; sd += h[4 * t + 2]; st += tot; nd += h[4 * t + 3] >> 24; mx = std::max(mx, tot);
  }
  fprintf(stderr, "fill stats: %llu tasks of %u rows | mean ticks (10 ns) per task: parameters + rows %.1f, list phase %.1f, dense phase %.1f, whole task %.1f (max %u) | "
          "dense variants per task %.2f\n", (unsigned long long)nt, chunk, sp / nt, sl / nt, sd / nt, st / nt, mx, nd / nt);
  return VS_OK;
}
#endif
// The fused expansion: k_fill_sites2 writes the shared rows AND their carrier lists, between the result's own pair of events.
static int shared_expand_fused(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const uint64_t U = c.U;
  // rows per wave task: 32 (one look-up of the run records and one round of parameter loads per 32 rows; 16-row tasks -- round 3's
  // choice for the kernel that did not write rows -- measure the same to 5 % slower, 64 and 8 slower: tools/ab_t6.py)
  const uint32_t chunk = idx->opts.fill_chunk ? idx->opts.fill_chunk : 32;
  const uint32_t gt_words = fill_gt_words(idx);
  size_t lds_bytes = fill_lds_bytes(idx);
  uint32_t ablate = 0;
  unsigned long long* tstat = nullptr;
  if ((U + chunk - 1) / chunk / 4 > 0x7FFFFFF0ull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu shared rows)", (unsigned long long)U);
#ifdef VS_TUNING
  constexpr bool kTune = true;
  lds_bytes += std::min<size_t>(idx->opts.fill_lds_pad, 96 << 10);
  ablate = idx->opts.fill_ablate;
  if (idx->opts.fill_stats) {
    VS_TRY(dev_alloc(idx, ((U + chunk - 1) / chunk + 4) * 16, (void**)&tstat, &c.scratch.bufs));
    HIP_TRY(hipMemsetAsync(tstat, 0, ((U + chunk - 1) / chunk + 4) * 16, idx->stream));
  }
#else
  constexpr bool kTune = false;
#endif
  const int mode = idx->opts.fill_mode;
  VS_TRY(result_events(r));   // the kernel's own duration, whenever the result is asked for it (vs_result_fill_ms)
  HIP_TRY(hipEventRecord(r->ev_fill[0], idx->stream));
  const PlanDev* pd = c.spec ? c.plan_dev : nullptr;
  if (idx->d.wpc > 63) launch_fill2<true, kTune>(idx, r->d, c.runs, c.coarse, c.n_runs, U, chunk, lds_bytes, ablate, gt_words, tstat, mode, pd);
  else launch_fill2<false, kTune>(idx, r->d, c.runs, c.coarse, c.n_runs, U, chunk, lds_bytes, ablate, gt_words, tstat, mode, pd);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(r->ev_fill[1], idx->stream));
  r->pending = true;
#ifdef VS_TUNING
  if (tstat) VS_TRY(print_fill_stats(idx, tstat, (U + chunk - 1) / chunk, chunk));
#endif
  return VS_OK;
}
// Lists: the carrier lists of the n_fill shared rows, in one of three forms (resident lists: none, the rows point into the index's arena).
static int shared_expand(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  c.fill_launches = c.n_fill ? 1 : 0;   // (async_fill: ms_fill is what the first stream saw of it, ~0; vs_result_fill_ms has the kernel's time)
  if (c.async_fill) {
    // the expansion goes to the handle's second stream behind an event and the call returns once the FIRST stream is done
    // (rows, per-region arrays); the next batch's plan and rows then run beside it.  The call's temporaries (the site
    // index the expansion reads) stay with the result until it is freed.
    VS_TRY(ensure_fill_stream(idx));
    VS_TRY(result_events(r));
    HIP_TRY(hipEventRecord(idx->fill_ev[0], idx->stream));
    HIP_TRY(hipStreamWaitEvent(idx->fill_stream, idx->fill_ev[0], 0));
    HIP_TRY(hipEventRecord(r->ev_fill[0], idx->fill_stream));
    VS_TRY(fill_lists(idx, r->d, true, c.u_site, c.n_fill, idx->fill_stream));
    HIP_TRY(hipEventRecord(r->ev_fill[1], idx->fill_stream));
    r->pending = true;
    return VS_OK;
  }
  if (!c.n_fill) return VS_OK;
  return c.fused ? shared_expand_fused(c) : fill_lists(idx, r->d, true, c.u_site, c.n_fill);
}
// A column request's kernels between the result's own pair of events (vs_result_fill_ms).  Counts, Groups: one launch over the whole
// table.  Assoc: k_allele_counts over the table, then k_assoc_scan.  Burden, Matrix, LD (behind the permutation): a burden filter's counts are inside the pair, and so are the three launches of
// an LD batch: counts, temporary matrix, band.  Scores (behind the permutation): launch_scores, with its one host wait inside the pair.
static int launch_scores(SharedCtx& c);
static int launch_score_matrix(SharedCtx& c);
static int ld_matrix_tables(SharedCtx& c);
static int assoc_matrix_upload(SharedCtx& c);
static int launch_assoc_matrix(SharedCtx& c);
static int launch_ld_block(vs_index* idx, vs_result* r, const uint8_t* cells, const SharedReq& lq);
static int prune_tables(SharedCtx& c);
static int launch_prune(SharedCtx& c);
static int clump_tables(SharedCtx& c);
static int launch_clump(SharedCtx& c);
static int ldscore_tables(SharedCtx& c);
static int launch_ldscore(SharedCtx& c);
static int launch_window_stats(SharedCtx& c);
static int launch_roh(SharedCtx& c);
static int shared_columns(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  if (!c.behind_perm && !r->d.A) return VS_OK;
  if (c.req.kind == ReqKind::LdMatrix) VS_TRY(ld_matrix_tables(c));   // (its one host wait in front of the pair of events: they time kernels only)
  if (c.req.kind == ReqKind::AssocMatrix) VS_TRY(assoc_matrix_upload(c));   // (in front of the pair of events as well)
  if (c.req.kind == ReqKind::Prune) VS_TRY(prune_tables(c));   // (its one host wait in front of the pair of events as well)
  if (c.req.kind == ReqKind::Clump) VS_TRY(clump_tables(c));   // (the same wait, and the upload of the keys)
  if (c.req.kind == ReqKind::LdScore) VS_TRY(ldscore_tables(c));   // (the same wait)
  if (c.req.kind == ReqKind::Trio)   // (the trio table's upload in front of the pair of events as well)
    HIP_TRY(hipMemcpyAsync(r->d_trio + r->trio_table_off, c.req.trio_cols, (size_t)c.req.n_trios * 12, hipMemcpyHostToDevice, idx->stream));
  VS_TRY(result_events(r));
  HIP_TRY(hipEventRecord(r->ev_fill[0], idx->stream));
  if (c.req.kind == ReqKind::Groups) launch_group_counts(idx, r->d, c.u_site, c.U, c.d_mask, c.req.words, c.req.n_cols, r->d_counts);
  else if (c.req.kind == ReqKind::WindowStats) {   // (a table without rows: no group kernel, the records are zeros all the same)
    if (r->d.A) launch_group_counts(idx, r->d, c.u_site, c.U, c.d_mask, c.req.words, c.req.n_cols, c.ws_counts);
    VS_TRY(launch_window_stats(c));
  } else if (c.req.kind != ReqKind::Matrix && r->d_counts && r->d.A)   // (Counts, LD, Gram, Ibs, Trio, Roh, ScoreMatrix; Burden only under a window: shared_tables gives it counts)
    launch_allele_counts(idx, r->d, c.u_site, c.U, c.d_mask, c.req.words, r->d_counts);
  HIP_TRY(hipGetLastError());
  if (c.req.kind == ReqKind::Assoc) VS_TRY(launch_assoc(idx, r, c.u_site, c.U, c.d_mask, c.d_rank, c.d_pheno, c.req));
  if (c.req.kind == ReqKind::Scores) VS_TRY(launch_scores(c));
  if (c.req.kind == ReqKind::ScoreMatrix) VS_TRY(launch_score_matrix(c));
  if (c.req.kind == ReqKind::Burden) VS_TRY(launch_burden(idx, r, c.u_site, c.U, c.d_mask, c.d_rank, c.req, c.scratch));
  if (c.req.kind == ReqKind::LD) {
    VS_TRY(launch_matrix(idx, r, c.ld_matrix, c.u_site, c.U, c.d_mask, c.d_rank, c.req));
    VS_TRY(launch_ld(idx, r, c.ld_matrix, c.req));
  } else if (c.req.kind == ReqKind::LdMatrix) {
    VS_TRY(launch_matrix(idx, r, c.ld_matrix, c.u_site, c.U, c.d_mask, c.d_rank, c.req));
    VS_TRY(launch_ld_block(idx, r, c.ld_matrix, c.req));
  } else if (c.req.kind == ReqKind::Prune) {
    VS_TRY(launch_matrix(idx, r, c.ld_matrix, c.u_site, c.U, c.d_mask, c.d_rank, c.req));
    VS_TRY(launch_prune(c));
  } else if (c.req.kind == ReqKind::Clump) {
    VS_TRY(launch_matrix(idx, r, c.ld_matrix, c.u_site, c.U, c.d_mask, c.d_rank, c.req));
    VS_TRY(launch_clump(c));
  } else if (c.req.kind == ReqKind::LdScore) {
    VS_TRY(launch_matrix(idx, r, c.ld_matrix, c.u_site, c.U, c.d_mask, c.d_rank, c.req));
    VS_TRY(launch_ldscore(c));
  } else if (c.req.kind == ReqKind::AssocMatrix) {
    VS_TRY(launch_matrix(idx, r, c.ld_matrix, c.u_site, c.U, c.d_mask, c.d_rank, c.req));
    VS_TRY(launch_assoc_matrix(c));
  } else if (c.req.kind == ReqKind::Gram) {
    VS_TRY(launch_matrix(idx, r, c.ld_matrix, c.u_site, c.U, c.d_mask, c.d_rank, c.req));
    VS_TRY(launch_gram(idx, r, c.ld_matrix, c.req));
  } else if (c.req.kind == ReqKind::Ibs) {
    VS_TRY(launch_matrix(idx, r, c.ld_matrix, c.u_site, c.U, c.d_mask, c.d_rank, c.req));
    VS_TRY(launch_ibs(idx, r, c.ld_matrix, c.U, c.req));
  } else if (c.req.kind == ReqKind::Trio) {
    VS_TRY(launch_matrix(idx, r, c.ld_matrix, c.u_site, c.U, c.d_mask, c.d_rank, c.req));
    VS_TRY(launch_trio(idx, r, c.ld_matrix, c.U, c.req));
  } else if (c.req.kind == ReqKind::Roh) {
    VS_TRY(launch_matrix(idx, r, c.ld_matrix, c.u_site, c.U, c.d_mask, c.d_rank, c.req));
    VS_TRY(launch_roh(c));
  } else if (c.req.kind == ReqKind::Matrix) VS_TRY(launch_matrix(idx, r, r->d_matrix, c.u_site, c.U, c.d_mask, c.d_rank, c.req));
  HIP_TRY(hipEventRecord(r->ev_fill[1], idx->stream));
  r->pending = true;
  c.fill_launches = 1;
  return VS_OK;
}

// The summaries and segments of a ROH batch behind the permutation (the per-region arrays are in the caller's order) from its temporary
// genotype matrix and the table's counts: k_roh_sites over the table, k_roh_walk<false> over (region, column tile).  With segments:
// the engine's exclusive scan over the cells' n_segments, ONE host wait for the total (inside the pair of events, as launch_scores'),
// the segment bytes held against option matrix_max_mib before they are allocated, then k_roh_walk<true>.
static int launch_roh(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const DevResult& d = r->d;
  const SharedReq& q = c.req;
  const uint64_t cells = d.Q * q.n_cols;
  RohArgs a{};
  a.cells = c.ld_matrix; a.row_begin = (const uint64_t*)d.var_begin; a.row_count = (const uint64_t*)d.q_nvar; a.Q = d.Q;
  a.pitch = (uint32_t)r->mx_pitch; a.n_cols = q.n_cols; a.n_tiles = (q.n_cols + kRohTileCols - 1) / kRohTileCols;
  a.min_sites = q.roh.min_sites; a.min_bp = q.roh.min_bp; a.max_gap = q.roh.max_gap; a.max_het = q.roh.max_het;
  a.summary = reinterpret_cast<RohSummary*>(r->d_roh);
  a.n_sites = reinterpret_cast<uint32_t*>(r->d_roh + r->roh_sites_off);
  if (d.Q * a.n_tiles > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu regions x %u column tiles)", (unsigned long long)d.Q, a.n_tiles);
  uint2* sites = nullptr;
  VS_TRY(dev_alloc(idx, (size_t)d.A * 8, (void**)&sites, &c.ld_tmp.bufs));
  a.sites = sites;
  if (d.A) {
    RohSiteArgs s{};
    s.rows = (const VariantRow*)d.rows; s.counts = r->d_counts; s.A = d.A; s.n_cols = q.n_cols; s.min_ac = q.roh.min_ac; s.max_ac = q.roh.max_ac; s.sites = sites;
    hipLaunchKernelGGL(k_roh_sites, dim3((unsigned)((d.A + 255) / 256)), dim3(256), 0, idx->stream, s);
  }
  uint64_t* seg_begin = reinterpret_cast<uint64_t*>(r->d_roh + r->roh_begin_off);
  if (q.roh.segments) VS_TRY(dev_alloc(idx, (size_t)cells * 4, (void**)&a.seg_count, &c.ld_tmp.bufs));
  const unsigned blocks = (unsigned)(d.Q * a.n_tiles);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_roh_walk<false>), dim3(blocks), dim3(256), 0, idx->stream, a);
  HIP_TRY(hipGetLastError());
  if (!q.roh.segments) return VS_OK;
  VS_TRY(exclusive_scan(idx, (const uint32_t*)a.seg_count, cells, seg_begin, &c.ld_tmp.bufs));
  uint64_t segs = 0;
  HIP_TRY(hipMemcpyAsync(&segs, seg_begin + cells, 8, hipMemcpyDeviceToHost, idx->stream));
  HIP_TRY(hipStreamSynchronize(idx->stream));
  VS_TRY(roh_fits(c, segs));
  r->roh_segs = segs;
  VS_TRY(ralloc(r, (size_t)segs * 2, &r->d_roh_seg));
  if (!segs) return VS_OK;
  a.seg_begin = seg_begin; a.segments = r->d_roh_seg;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_roh_walk<true>), dim3(blocks), dim3(256), 0, idx->stream, a);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}

// The records of a window-statistics batch behind the permutation (the per-region arrays are in the caller's order) from the temporary
// grouped counts: k_window_stats, a wave per region, and -- only when the rows all regions report could hold a region longer than a
// chunk -- the device-built list of such regions' chunks (k_burden_split_plan) and the SPLIT launch that adds them.
template <uint32_t NPB>
static void launch_window_kernels(vs_index* idx, const WindowArgs& a, uint32_t cap, size_t lds) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_window_stats<NPB, false>), dim3((unsigned)((a.Q + 3) / 4)), dim3(256), lds, idx->stream, a);
  if (cap) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_window_stats<NPB, true>), dim3(cap), dim3(256), lds, idx->stream, a);
}
static int launch_window_stats(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const DevResult& d = r->d;
  const SharedReq& q = c.req;
  WindowArgs a{};
  a.gc = c.ws_counts; a.rows = (const VariantRow*)d.rows; a.U = c.U; a.var_begin = d.var_begin; a.q_nvar = d.q_nvar; a.Q = d.Q;
  a.G = q.n_cols; a.P = q.ws_pairs;
  a.chunk_rows = idx->opts.window_chunk ? idx->opts.window_chunk : kWinChunkRows;
  a.rec = reinterpret_cast<uint32_t*>(r->d_wstats);
  a.pair = reinterpret_cast<uint4*>(r->d_wstats + (size_t)d.Q * 48 * q.n_cols);
  for (uint32_t g = 0; g < q.n_cols; ++g) a.gsize[g] = (uint16_t)q.ws_sizes[g];   // (at most 32,767 samples in all)
  uint32_t* n_work = reinterpret_cast<uint32_t*>(r->d_cell_total + 1);
  a.n_work = n_work;
  if (d.Q > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu regions)", (unsigned long long)d.Q);
  HIP_TRY(hipMemsetAsync(r->d_cell_total, 0, 16, idx->stream));
  // every split region has more than chunk_rows rows, so its chunks number less than twice its rows / chunk_rows
  const uint64_t cap64 = r->n_rows_reported > a.chunk_rows ? 2 * r->n_rows_reported / a.chunk_rows : 0;
  if (cap64 > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu row chunks)", (unsigned long long)cap64);
  const uint32_t cap = (uint32_t)cap64;
  if (cap) {
    uint2* work = nullptr;
    VS_TRY(dev_alloc(idx, (size_t)cap * sizeof(uint2), (void**)&work, &c.scratch.bufs));
    a.work = work;
    hipLaunchKernelGGL(k_burden_split_plan, dim3((unsigned)((d.Q + 255) / 256)), dim3(256), 0, idx->stream, (const uint64_t*)d.q_nvar, d.Q, a.chunk_rows, work, n_work, cap);
  }
  const size_t lds = 4 * sizeof(uint32_t) * (size_t)window_cells(a.G);
  const uint32_t batches = (a.P + 63) / 64;   // pairs a lane owns
  if (batches == 0) launch_window_kernels<0>(idx, a, cap, lds);
  else if (batches <= 1) launch_window_kernels<1>(idx, a, cap, lds);
  else if (batches <= 2) launch_window_kernels<2>(idx, a, cap, lds);
  else if (batches <= 4) launch_window_kernels<4>(idx, a, cap, lds);
  else if (batches <= 8) launch_window_kernels<8>(idx, a, cap, lds);
  else if (batches <= 16) launch_window_kernels<16>(idx, a, cap, lds);
  else launch_window_kernels<32>(idx, a, cap, lds);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}

// A score batch behind the permutation (the per-region arrays are in the caller's order).  The reports' offsets and -- for weights in
// device memory -- their scale come back in ONE host wait (the batch is never speculative); the number of reports is held against
// n_weights before anything else is allocated.  Then the integer weights per table row, the walk, the scores.
template <uint32_t KP>
static int launch_score_walk(vs_index* idx, const ScoreArgs& a, unsigned blocks, size_t lds) {
  const bool sub = a.S != nullptr;
  const void* fn = sub ? reinterpret_cast<const void*>(&k_sample_scores<KP, true>) : reinterpret_cast<const void*>(&k_sample_scores<KP, false>);
  if (lds > (40 << 10)) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   // (beside 6 KiB of static LDS)
  if (sub) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sample_scores<KP, true>), dim3(blocks), dim3(256), lds, idx->stream, idx->d, a);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sample_scores<KP, false>), dim3(blocks), dim3(256), lds, idx->stream, idx->d, a);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}
static int launch_scores(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const DevResult& d = r->d;
  const SharedReq& q = c.req;
  const uint32_t K = q.n_scores, kp = score_pow2(K);
  uint64_t* off = nullptr;
  VS_TRY(dev_alloc(idx, (d.Q + 1) * 8, (void**)&off, &c.scratch.bufs));
  HIP_TRY(hipMemsetAsync(r->d_score_meta, 0, sizeof(ScoreMeta), idx->stream));
  hipLaunchKernelGGL(k_score_offsets, dim3(1), dim3(kScoreOffBlock), 0, idx->stream, (const uint64_t*)d.var_count, d.Q, off);
  if (q.weights_on_device && q.n_weights)
    hipLaunchKernelGGL(k_score_scale, dim3((unsigned)std::min<uint64_t>((q.n_weights + 255) / 256, 1024)), dim3(256), 0, idx->stream, q.weights, q.n_weights, K,
                       r->d_score_meta);
  HIP_TRY(hipGetLastError());
  uint64_t N = 0;
  ScoreMeta hm{};
  HIP_TRY(hipMemcpyAsync(&N, off + d.Q, 8, hipMemcpyDeviceToHost, idx->stream));
  HIP_TRY(hipMemcpyAsync(&hm, r->d_score_meta, sizeof(ScoreMeta), hipMemcpyDeviceToHost, idx->stream));
  HIP_TRY(hipStreamSynchronize(idx->stream));
  if (N != q.n_weights)
    return fail(VS_ERR_ARG, "%llu rows of weights for the %llu rows the regions report: one row of weights per reported row, in report order",
                (unsigned long long)q.n_weights, (unsigned long long)N);
  if (N >= kScoreMaxReports)
    return fail(VS_ERR_ARG, "%llu reported rows: a score batch takes fewer than 2^26 (the 64-bit sums could overflow beyond): split the batch", (unsigned long long)N);
  if (hm.nonfinite) return fail(VS_ERR_ARG, "weight column %d holds a value that is not finite", __builtin_ctz(hm.nonfinite));
  ScoreShift sh{};
  r->score_shift.assign(K, 0);
  for (uint32_t k = 0; k < K; ++k) {
    const uint32_t bits = q.weights_on_device ? hm.max_bits[k] : q.score_max_bits[k];
    float m;
    memcpy(&m, &bits, 4);
    int e = 0;
    if (bits) { (void)std::frexp((double)m, &e); sh.f[k] = (int32_t)kScoreShift - e; }
    r->score_shift[k] = sh.f[k];
  }
  const uint64_t cap = idx->opts.matrix_max_mib ? (uint64_t)idx->opts.matrix_max_mib << 20 : 32ull << 30;
  const uint64_t cells = (uint64_t)q.n_cols * K;
  const uint64_t need = (q.weights_on_device ? 0 : N * K * 4) + d.A * (8ull * kp + 4) + cells * 16;
  if (need > cap)
    return fail(VS_ERR_ARG, "a score batch of %llu reports x %u scores over %llu rows and %u columns takes %llu bytes, more than the limit of %llu MiB (option matrix_max_mib): split the batch",
                (unsigned long long)N, K, (unsigned long long)d.A, q.n_cols, (unsigned long long)need, (unsigned long long)(cap >> 20));
  VS_TRY(ralloc(r, (size_t)cells * 2, &r->d_sums));
  r->d_score_out = reinterpret_cast<double*>(r->d_sums + cells);
  HIP_TRY(hipMemsetAsync(r->d_sums, 0, cells * 8, idx->stream));
  if (N && d.A) {
    const float* dw = q.weights;
    if (!q.weights_on_device) {
      float* up = nullptr;
      VS_TRY(dev_alloc(idx, N * K * 4, (void**)&up, &c.scratch.bufs));
      HIP_TRY(hipMemcpyAsync(up, q.weights, N * K * 4, hipMemcpyHostToDevice, idx->stream));
      dw = up;
    }
    long long* wq = nullptr;
    const size_t wq_bytes = (size_t)d.A * kp * 8;
    VS_TRY(dev_alloc(idx, wq_bytes + (size_t)d.A * 4, (void**)&wq, &c.scratch.bufs));
    HIP_TRY(hipMemsetAsync(wq, 0, wq_bytes + (size_t)d.A * 4, idx->stream));
    uint32_t* wn = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(wq) + wq_bytes);
    ScoreWeightArgs wa{};
    wa.rows = (const VariantRow*)d.rows; wa.var_begin = d.var_begin; wa.q_nvar = d.q_nvar; wa.off = off; wa.Q = d.Q; wa.N = N;
    wa.w = dw; wa.K = K; wa.KP = kp; wa.shift = sh; wa.wq = wq; wa.wn = wn;
    hipLaunchKernelGGL(k_score_weights, dim3((unsigned)std::min<uint64_t>((d.Q + 3) / 4, 8192)), dim3(256), 0, idx->stream, wa);
    HIP_TRY(hipGetLastError());
    ScoreArgs a{};
    a.rows = (const VariantRow*)d.rows; a.u_site = c.u_site; a.A = d.A; a.U = c.U;
    a.S = c.d_mask; a.S_rank = c.d_rank; a.s_words = c.d_mask ? q.words : 0;
    a.n_cols = q.n_cols; a.K = K;
    const uint32_t tile_max = kScoreTileBytes / (8 * kp);
    a.tile_cols = std::min<uint32_t>(q.n_cols, idx->opts.score_tile_cols ? std::min(idx->opts.score_tile_cols, tile_max) : tile_max);
    a.n_tiles = (q.n_cols + a.tile_cols - 1) / a.tile_cols;
    a.chunk_rows = idx->opts.score_chunk ? idx->opts.score_chunk : kScoreChunkRows;
    a.wq = wq; a.wn = wn; a.sums = reinterpret_cast<unsigned long long*>(r->d_sums); a.meta = r->d_score_meta;
    const uint64_t chunks = (d.A + a.chunk_rows - 1) / a.chunk_rows;
    if (chunks * a.n_tiles > 0x7FFFFFFFull)
      return fail(VS_ERR_ARG, "batch too large for one launch (%llu row chunks x %u column tiles)", (unsigned long long)chunks, a.n_tiles);
    const size_t lds = (size_t)a.tile_cols * kp * 8 + (size_t)a.s_words * 12;
    const unsigned blocks = (unsigned)(chunks * a.n_tiles);
    switch (kp) {
      case 1: VS_TRY(launch_score_walk<1>(idx, a, blocks, lds)); break;
      case 2: VS_TRY(launch_score_walk<2>(idx, a, blocks, lds)); break;
      case 4: VS_TRY(launch_score_walk<4>(idx, a, blocks, lds)); break;
      default: VS_TRY(launch_score_walk<8>(idx, a, blocks, lds)); break;
    }
  }
  hipLaunchKernelGGL(k_score_finish, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, idx->stream, (const long long*)r->d_sums, cells, K, sh, r->d_score_out);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}

// Table rows per workgroup of k_score_matrix.  Option score_matrix_chunk, or by the batch's shape as gram_chunk_rows: the chunk that
// gives about kSmBlocksWanted workgroups over all (score tile group, column tile) pairs, a multiple of kGramK, at least 2 kGramK
// (fewer rows per workgroup only add atomics) and at most kSmChunkMax.
static uint32_t score_matrix_chunk_rows(const vs_index* idx, uint64_t A, uint64_t n_pairs) {
  if (idx->opts.score_matrix_chunk) return idx->opts.score_matrix_chunk;
  const uint64_t per = (A * n_pairs + kSmBlocksWanted - 1) / kSmBlocksWanted;
  const uint64_t rows = (per + kGramK - 1) / kGramK * kGramK;
  return (uint32_t)std::min<uint64_t>(kSmChunkMax, std::max<uint64_t>(2 * kGramK, rows));
}
// A score-matrix batch behind the permutation (the per-region arrays are in the caller's order).  The reports' offsets come back in a
// first host wait (the batch is never speculative) and the number of reports is held against n_weights, then the whole batch against
// option matrix_max_mib, before anything of it is allocated.  Then the temporary matrix, the weights' row totals T and the limb
// panel; the largest |T| comes back in a second wait -- the call refuses a batch beyond 2^38, so the host has to see it, and the
// matrix kernel is then picked by the limbs the batch needs --; the product and the scores.
static int launch_score_matrix(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const DevResult& d = r->d;
  const SharedReq& q = c.req;
  const uint32_t K = q.n_scores;
  uint64_t* off = nullptr;
  VS_TRY(dev_alloc(idx, (d.Q + 1) * 8, (void**)&off, &c.scratch.bufs));
  hipLaunchKernelGGL(k_score_offsets, dim3(1), dim3(kScoreOffBlock), 0, idx->stream, (const uint64_t*)d.var_count, d.Q, off);
  HIP_TRY(hipGetLastError());
  uint64_t N = 0;
  HIP_TRY(hipMemcpyAsync(&N, off + d.Q, 8, hipMemcpyDeviceToHost, idx->stream));
  HIP_TRY(hipStreamSynchronize(idx->stream));
  if (N != q.n_weights)
    return fail(VS_ERR_ARG, "%llu rows of weights for the %llu rows the regions report: one row of weights per reported row, in report order",
                (unsigned long long)q.n_weights, (unsigned long long)N);
  if (N >= kSmMaxReports)
    return fail(VS_ERR_ARG, "%llu reported rows: a score-matrix batch takes fewer than 2^26 (the 64-bit sums could overflow beyond): split the batch", (unsigned long long)N);
  const uint64_t cap = idx->opts.matrix_max_mib ? (uint64_t)idx->opts.matrix_max_mib << 20 : 32ull << 30;
  const uint64_t cells = (uint64_t)q.n_cols * K, apad = (d.A + 127) & ~127ull, tiles = (K + kSmScoreTile - 1) / kSmScoreTile;
  // (the table's rows are slots of the regions, N of them and the dropped ones: with N < 2^26, K <= 2^16 and a pitch below 2^32 every part stays far below 2^63)
  const uint64_t b_matrix = d.A * r->mx_pitch, b_weights = N * K * 4, b_totals = d.A * K * 8, b_panel = tiles * kSmScoreTile * kSmLimbsMax * apad, b_cells = cells * 16;
  const uint64_t need = b_matrix + b_weights + b_totals + b_panel + b_cells;
  if (need > cap)
    return fail(VS_ERR_ARG, "a score-matrix batch of %llu reports x %u scores over %llu rows and %u columns takes %llu bytes (%llu of the genotype matrix it is formed from, "
                "%llu of the weights, %llu of the rows' totals, %llu of the limb panel, %llu of the sums and scores), more than the limit of %llu MiB (option matrix_max_mib): "
                "split the batch or the scores", (unsigned long long)N, K, (unsigned long long)d.A, q.n_cols, (unsigned long long)need, (unsigned long long)b_matrix,
                (unsigned long long)b_weights, (unsigned long long)b_totals, (unsigned long long)b_panel, (unsigned long long)b_cells, (unsigned long long)(cap >> 20));
  VS_TRY(ralloc(r, (size_t)cells * 2, &r->d_sums));
  r->d_score_out = reinterpret_cast<double*>(r->d_sums + cells);
  HIP_TRY(hipMemsetAsync(r->d_sums, 0, cells * 16, idx->stream));   // (the scores of an all-zero batch are +0.0: the same bytes)
  r->sm_limbs = 4;
  VS_TRY(dev_alloc(idx, (size_t)b_matrix, (void**)&c.ld_matrix, &c.ld_tmp.bufs));
  VS_TRY(launch_matrix(idx, r, c.ld_matrix, c.u_site, c.U, c.d_mask, c.d_rank, q));
  if (!N || !d.A) return VS_OK;
  // ---- the weights and their shifts to the device, the rows' totals, the limb panel ----
  int32_t* shift = nullptr;
  float* dw = nullptr;
  long long* T = nullptr;
  int8_t* panel = nullptr;
  unsigned long long* meta = nullptr;
  const uint64_t lrows = apad / kSmLimbRows, lcols = (tiles * kSmScoreTile + kSmLimbCols - 1) / kSmLimbCols;
  if (lrows > 0x7FFFFFFFull || lcols > 65535) return fail(VS_ERR_ARG, "batch too large for one launch (%llu row blocks of the limb panel)", (unsigned long long)lrows);
  VS_TRY(dev_alloc(idx, (size_t)K * 4 + 16, (void**)&shift, &c.ld_tmp.bufs));
  VS_TRY(dev_alloc(idx, (size_t)b_weights, (void**)&dw, &c.ld_tmp.bufs));
  VS_TRY(dev_alloc(idx, (size_t)b_totals + 8, (void**)&T, &c.ld_tmp.bufs));
  VS_TRY(dev_alloc(idx, (size_t)b_panel, (void**)&panel, &c.ld_tmp.bufs));
  meta = reinterpret_cast<unsigned long long*>(T + d.A * K);
  HIP_TRY(hipMemcpyAsync(shift, r->score_shift.data(), (size_t)K * 4, hipMemcpyHostToDevice, idx->stream));
  // From here on the runtime may be reading the caller's weights: nothing returns before the stream has been waited for.
  uint64_t max_abs = 0;
  const int enq = [&]() -> int {
    HIP_TRY(hipMemcpyAsync(dw, q.weights, (size_t)b_weights, hipMemcpyHostToDevice, idx->stream));
    HIP_TRY(hipMemsetAsync(T, 0, (size_t)b_totals + 8, idx->stream));
    ScoreMatrixWeightArgs wa{};
    wa.rows = (const VariantRow*)d.rows; wa.var_begin = d.var_begin; wa.q_nvar = d.q_nvar; wa.off = off; wa.Q = d.Q; wa.N = N;
    wa.w = dw; wa.shift = shift; wa.K = K; wa.T = T;
    wa.G = 1;
    while (wa.G < 64 && wa.G < K) wa.G *= 2;
    hipLaunchKernelGGL(k_score_matrix_weights, dim3((unsigned)std::min<uint64_t>((d.Q + 3) / 4, 8192)), dim3(256), 0, idx->stream, wa);
    ScoreMatrixLimbArgs la{};
    la.T = T; la.A = d.A; la.apad = apad; la.K = K; la.tiles = (uint32_t)tiles; la.panel = panel; la.meta = meta;
    hipLaunchKernelGGL(k_score_matrix_limbs, dim3((unsigned)lrows, (unsigned)lcols), dim3(256), 0, idx->stream, la);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&max_abs, meta, 8, hipMemcpyDeviceToHost, idx->stream));
    return VS_OK;
  }();
  const hipError_t waited = hipStreamSynchronize(idx->stream);   // (the weights have left the caller's memory as well, whatever failed above)
  VS_TRY(enq);
  HIP_TRY(waited);
  if (max_abs > (uint64_t)kSmMaxTotal)
    return fail(VS_ERR_UNSUPPORTED, "the weights of the reports of one table row add up to %llu in fixed point, more than 2^38 (more than 256 regions report the row): split the batch",
                (unsigned long long)max_abs);
  r->sm_limbs = sm_limbs_needed(max_abs);
  // ---- the product ----
  const uint32_t ts = r->sm_limbs == 4 ? kSmTilesPerWg : kSmTilesPerWg5;   // score tiles per workgroup
  ScoreMatrixArgs a{};
  a.cells = c.ld_matrix; a.panel = panel; a.A = d.A; a.apad = apad; a.pitch = (uint32_t)r->mx_pitch; a.n_cols = q.n_cols; a.K = K;
  a.tiles = (uint32_t)tiles; a.tile_groups = (a.tiles + ts - 1) / ts; a.col_tiles = (q.n_cols + kGramTile - 1) / kGramTile;
  a.sums = reinterpret_cast<unsigned long long*>(r->d_sums);
  const uint64_t pairs = (uint64_t)a.tile_groups * a.col_tiles;
  a.chunk = score_matrix_chunk_rows(idx, d.A, pairs);
  const uint64_t blocks = (d.A + a.chunk - 1) / a.chunk * pairs, fblocks = (cells + 255) / 256;
  if (blocks > 0x7FFFFFFFull || fblocks > 0x7FFFFFFFull)
    return fail(VS_ERR_ARG, "batch too large for one launch (%llu row chunks x %llu tiles)", (unsigned long long)(blocks / pairs), (unsigned long long)pairs);
  if (r->sm_limbs == 4) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_score_matrix<4, kSmTilesPerWg>), dim3((unsigned)blocks), dim3(256), 0, idx->stream, a);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_score_matrix<5, kSmTilesPerWg5>), dim3((unsigned)blocks), dim3(256), 0, idx->stream, a);
  hipLaunchKernelGGL(k_score_matrix_finish, dim3((unsigned)fblocks), dim3(256), 0, idx->stream, (const long long*)r->d_sums, cells, K, (const int32_t*)shift, r->d_score_out);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}

// An LD-matrix batch behind the permutation (the per-region arrays are in the caller's order): the blocks' offsets and the workgroups'
// prefix from the per-region row counts by one small scan; the two totals and the largest block come back in ONE host wait (the
// batch is never speculative).  The temporary matrix and the cells together are held against option matrix_max_mib here, before
// either is allocated.
static int ld_matrix_tables(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const DevResult& d = r->d;
  uint64_t* meta = r->d_ldm_meta;
  hipLaunchKernelGGL(k_ld_block_scan, dim3(1), dim3(kLdBlockScanThreads), 0, idx->stream, (const uint64_t*)d.q_nvar, d.Q, meta, meta + (d.Q + 1), meta + 2 * (d.Q + 1));
  HIP_TRY(hipGetLastError());
  uint64_t sum[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(sum, meta + 2 * (d.Q + 1), sizeof sum, hipMemcpyDeviceToHost, idx->stream));
  HIP_TRY(hipStreamSynchronize(idx->stream));
  const uint64_t cap = idx->opts.matrix_max_mib ? (uint64_t)idx->opts.matrix_max_mib << 20 : 32ull << 30;
  const uint64_t cells = sum[0], matrix_bytes = d.A * r->mx_pitch;
  if (cells > cap / 4 || matrix_bytes > cap - 4 * cells) {
    // (the handle's stream, waited for above, runs behind the plan's last event, so the plan's kernels have finished with the call's
    //  temporaries that go back to the pool on return; the plan stream is waited for all the same, as matrix_fits does)
    (void)hipStreamSynchronize(c.ps);
    return fail(VS_ERR_ARG, "the LD blocks of %llu regions over %llu rows x %u columns (largest block %llu x %llu) take %llu bytes (%llu of the genotype matrix they are "
                "formed from, %llu of the cells), more than the limit of %llu MiB (option matrix_max_mib): split the batch or the regions",
                (unsigned long long)d.Q, (unsigned long long)d.A, c.req.n_cols, (unsigned long long)sum[2], (unsigned long long)sum[2],
                (unsigned long long)(matrix_bytes + 4 * cells), (unsigned long long)matrix_bytes, (unsigned long long)(4 * cells), (unsigned long long)(cap >> 20));
  }
  if (sum[1] > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu tile pairs)", (unsigned long long)sum[1]);
  r->ldm_cells = cells; r->ldm_wgs = sum[1];
  VS_TRY(dev_alloc(idx, (size_t)matrix_bytes, (void**)&c.ld_matrix, &c.ld_tmp.bufs));
  VS_TRY(ralloc(r, (size_t)cells, &r->d_ldm));
  return VS_OK;
}

// The blocks of an LD-matrix batch from its temporary genotype matrix and the table's counts: one workgroup per (region, pair of
// 64-row tiles), all regions in one launch.
static int launch_ld_block(vs_index* idx, vs_result* r, const uint8_t* cells, const SharedReq& lq) {
  const DevResult& d = r->d;
  if (!r->ldm_cells) return VS_OK;
  LdBlockArgs a{};
  a.cells = cells; a.pitch = (uint32_t)r->mx_pitch; a.n_cols = lq.n_cols; a.Q = d.Q;
  a.row_begin = (const uint64_t*)d.var_begin; a.row_count = (const uint64_t*)d.q_nvar;
  a.block_begin = r->d_ldm_meta; a.wg_begin = r->d_ldm_meta + (d.Q + 1);
  a.counts = r->d_counts; a.out = r->d_ldm;
  if (lq.ld_stat == VS_LD_R2) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ld_block<true>), dim3((unsigned)r->ldm_wgs), dim3(256), 0, idx->stream, a);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ld_block<false>), dim3((unsigned)r->ldm_wgs), dim3(256), 0, idx->stream, a);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}

// An LD-score batch behind the permutation (the per-region arrays are in the caller's order): keep_begin and the workgroups' prefix
// from the per-region row counts by one small scan; the two totals come back in ONE host wait (the batch is never speculative).
// The temporary matrix, the slots and the per-region words together are held against option matrix_max_mib here, before the first
// two are allocated.
static int ldscore_tables(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const DevResult& d = r->d;
  uint64_t* meta = r->d_prune_meta;
  hipLaunchKernelGGL(k_ld_score_scan, dim3(1), dim3(kLdBlockScanThreads), 0, idx->stream, (const uint64_t*)d.q_nvar, d.Q, meta, meta + (d.Q + 1), meta + 3 * (d.Q + 1),
                     c.req.ld_window);
  HIP_TRY(hipGetLastError());
  uint64_t sum[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(sum, meta + 3 * (d.Q + 1), sizeof sum, hipMemcpyDeviceToHost, idx->stream));
  HIP_TRY(hipStreamSynchronize(idx->stream));
  VS_TRY(ldscore_fits(c, sum[0]));
  if (sum[1] > 0x7FFFFFFFull) {
    (void)hipStreamSynchronize(c.ps);
    return fail(VS_ERR_ARG, "batch too large for one launch (%llu tile pairs)", (unsigned long long)sum[1]);
  }
  r->prune_states = sum[0]; r->ldscore_wgs = sum[1];
  VS_TRY(dev_alloc(idx, (size_t)(d.A * r->mx_pitch), (void**)&c.ld_matrix, &c.ld_tmp.bufs));
  VS_TRY(ralloc(r, (size_t)sum[0] * 13, &r->d_ldscore));
  return VS_OK;
}

// The scores of an LD-score batch from its temporary genotype matrix and the table's counts: k_ld_score_init, a workgroup per
// region, then k_ld_score, one workgroup per (region, tile, tile distance), all regions in one launch.
static int launch_ldscore(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const DevResult& d = r->d;
  const SharedReq& q = c.req;
  LdScoreArgs a{};
  a.cells = c.ld_matrix; a.pitch = (uint32_t)r->mx_pitch; a.n_cols = q.n_cols; a.Q = d.Q;
  a.row_begin = (const uint64_t*)d.var_begin; a.row_count = (const uint64_t*)d.q_nvar;
  a.keep_begin = r->d_prune_meta; a.wg_begin = r->d_prune_meta + (d.Q + 1);
  a.rows = (const VariantRow*)d.rows; a.counts = r->d_counts;
  a.window = q.ld_window; a.max_bp = q.prune_max_bp; a.min_ac = q.prune_min_ac; a.max_ac = q.prune_max_ac;
  a.sums = reinterpret_cast<unsigned long long*>(r->d_ldscore);
  a.n_pairs = reinterpret_cast<uint32_t*>(r->d_ldscore + 8 * r->prune_states);
  a.state = r->d_ldscore + 12 * r->prune_states;
  a.n_scored = r->d_prune_meta + 2 * (d.Q + 1);
  if (d.Q > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu regions)", (unsigned long long)d.Q);
  hipLaunchKernelGGL(k_ld_score_init, dim3((unsigned)d.Q), dim3(256), 0, idx->stream, a);
  if (r->ldscore_wgs) hipLaunchKernelGGL(k_ld_score, dim3((unsigned)r->ldscore_wgs), dim3(256), 0, idx->stream, a);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}

// A pruning batch behind the permutation (the per-region arrays are in the caller's order): keep_begin from the per-region row counts
// by one small scan; the number of verdicts comes back in ONE host wait (the batch is never speculative).  The temporary matrix,
// the masks, the state and the per-region words together are held against option matrix_max_mib here, before the first three are
// allocated.
static int prune_tables(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const DevResult& d = r->d;
  uint64_t* meta = r->d_prune_meta;
  hipLaunchKernelGGL(k_prune_scan, dim3(1), dim3(kPruneScanThreads), 0, idx->stream, (const uint64_t*)d.q_nvar, d.Q, meta, meta + 2 * (d.Q + 1));
  HIP_TRY(hipGetLastError());
  uint64_t sum[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(sum, meta + 2 * (d.Q + 1), sizeof sum, hipMemcpyDeviceToHost, idx->stream));
  HIP_TRY(hipStreamSynchronize(idx->stream));
  VS_TRY(prune_fits(c, sum[0]));
  r->prune_states = sum[0];
  const uint32_t words = (c.req.ld_window + 31) / 32;
  VS_TRY(dev_alloc(idx, (size_t)(d.A * r->mx_pitch), (void**)&c.ld_matrix, &c.ld_tmp.bufs));
  VS_TRY(dev_alloc(idx, (size_t)(d.A * words) * 4, (void**)&c.prune_hits, &c.ld_tmp.bufs));
  VS_TRY(ralloc(r, (size_t)sum[0], &r->d_state));
  return VS_OK;
}

// The verdicts of a pruning batch from its temporary genotype matrix and the table's counts: k_prune_hits over blocks of kLdRows
// table rows, as the band kernel, then k_prune_greedy, one wave per region, all regions in one launch.
template <int MAXT>
static int launch_prune_hits(vs_index* idx, const PruneHitArgs& p, unsigned blocks, size_t lds) {
  if (lds > (48 << 10)) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_prune_hits<MAXT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_prune_hits<MAXT>), dim3(blocks), dim3(256), lds, idx->stream, p);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}
static int launch_prune(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const DevResult& d = r->d;
  const SharedReq& q = c.req;
  const uint32_t words = (q.ld_window + 31) / 32;
  if (d.A) {
    PruneHitArgs p{};
    p.ld.cells = c.ld_matrix; p.ld.A = d.A; p.ld.pitch = (uint32_t)r->mx_pitch; p.ld.n_cols = q.n_cols;
    p.ld.window = q.ld_window; p.ld.n_tiles = (q.ld_window + 15) / 16 + 1;
    p.ld.counts = r->d_counts; p.ld.band = nullptr;
    p.rows = (const VariantRow*)d.rows; p.hits = c.prune_hits; p.words = words; p.max_bp = q.prune_max_bp; p.threshold = q.prune_T;
    const uint64_t blocks = (d.A + kLdRows - 1) / kLdRows;
    if (blocks > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu row blocks)", (unsigned long long)blocks);
    const size_t lds = (size_t)(kLdRows + 16 * (p.ld.n_tiles - 1)) * kLdStride;
    if (p.ld.n_tiles <= kLdSmallTiles) VS_TRY(launch_prune_hits<(int)kLdSmallTiles>(idx, p, (unsigned)blocks, lds));
    else VS_TRY(launch_prune_hits<(int)kLdMaxTiles>(idx, p, (unsigned)blocks, lds));
  }
  PruneGreedyArgs g{};
  g.Q = d.Q; g.row_begin = (const uint64_t*)d.var_begin; g.row_count = (const uint64_t*)d.q_nvar;
  g.keep_begin = r->d_prune_meta; g.rows = (const VariantRow*)d.rows; g.counts = r->d_counts; g.hits = c.prune_hits;
  g.words = words; g.n_cols = q.n_cols; g.min_ac = q.prune_min_ac; g.max_ac = q.prune_max_ac;
  g.state = r->d_state; g.n_kept = r->d_prune_meta + (d.Q + 1);
  if (d.Q > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu regions)", (unsigned long long)d.Q);
  hipLaunchKernelGGL(k_prune_greedy, dim3((unsigned)d.Q), dim3(64), 0, idx->stream, g);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}

// A clumping batch behind the permutation: prune_tables' scan and its ONE host wait; then the number of p-values is held against
// the table's rows and everything the batch takes against option matrix_max_mib, before any of it is allocated.  The keys go up
// from the result's own copy.
static int clump_tables(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const DevResult& d = r->d;
  uint64_t* meta = r->d_prune_meta;
  hipLaunchKernelGGL(k_prune_scan, dim3(1), dim3(kPruneScanThreads), 0, idx->stream, (const uint64_t*)d.q_nvar, d.Q, meta, meta + 2 * (d.Q + 1));
  HIP_TRY(hipGetLastError());
  uint64_t sum[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(sum, meta + 2 * (d.Q + 1), sizeof sum, hipMemcpyDeviceToHost, idx->stream));
  HIP_TRY(hipStreamSynchronize(idx->stream));
  if (c.req.n_pvalues != d.A) {
    (void)hipStreamSynchronize(c.ps);   // (as prune_fits: the plan's last kernels still read the call's temporaries)
    return fail(VS_ERR_ARG, "%llu p-values for the %llu rows of the regions' table: one p-value per table row, in table order",
                (unsigned long long)c.req.n_pvalues, (unsigned long long)d.A);
  }
  VS_TRY(clump_fits(c, sum[0]));
  r->prune_states = sum[0];
  const uint32_t words = (c.req.ld_window + 31) / 32;
  VS_TRY(dev_alloc(idx, (size_t)(d.A * r->mx_pitch), (void**)&c.ld_matrix, &c.ld_tmp.bufs));
  VS_TRY(dev_alloc(idx, (size_t)(d.A * words) * 4, (void**)&c.prune_hits, &c.ld_tmp.bufs));
  VS_TRY(dev_alloc(idx, (size_t)d.A * 8, (void**)&c.clump_keys, &c.ld_tmp.bufs));
  VS_TRY(dev_alloc(idx, (size_t)d.A, (void**)&c.clump_cls, &c.ld_tmp.bufs));
  VS_TRY(dev_alloc(idx, (size_t)(sum[0] * words) * 8, (void**)&c.clump_blockers, &c.ld_tmp.bufs));
  VS_TRY(ralloc(r, (size_t)sum[0], &r->d_state));
  VS_TRY(ralloc(r, (size_t)sum[0], &r->d_owner));
  if (d.A) {
    HIP_TRY(hipMemcpyAsync(c.clump_keys, c.req.clump_keys, (size_t)d.A * 8, hipMemcpyHostToDevice, idx->stream));
    HIP_TRY(hipStreamSynchronize(idx->stream));   // (in front of the pair of events: they time kernels only)
  }
  return VS_OK;
}

// The verdicts of a clumping batch: k_prune_hits as for a pruning batch, then the classes of the table rows, the blocker masks of
// the verdict slots and the rounds, one workgroup per region, all regions in one launch.
static int launch_clump(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const DevResult& d = r->d;
  const SharedReq& q = c.req;
  const uint32_t words = (q.ld_window + 31) / 32;
  ClumpArgs g{};
  g.Q = d.Q; g.A = d.A; g.states = r->prune_states;
  g.row_begin = (const uint64_t*)d.var_begin; g.row_count = (const uint64_t*)d.q_nvar; g.keep_begin = r->d_prune_meta;
  g.rows = (const VariantRow*)d.rows; g.counts = r->d_counts; g.keys = c.clump_keys; g.hits = c.prune_hits;
  g.cls = c.clump_cls; g.blockers = c.clump_blockers;
  g.words = words; g.window = q.ld_window; g.n_cols = q.n_cols; g.key1 = q.clump_key[0]; g.key2 = q.clump_key[1];
  g.state = r->d_state; g.owner = r->d_owner; g.n_index = r->d_prune_meta + (d.Q + 1); g.rounds = r->d_prune_meta + 2 * (d.Q + 1) + 4;
  if (d.A) {
    PruneHitArgs p{};
    p.ld.cells = c.ld_matrix; p.ld.A = d.A; p.ld.pitch = (uint32_t)r->mx_pitch; p.ld.n_cols = q.n_cols;
    p.ld.window = q.ld_window; p.ld.n_tiles = (q.ld_window + 15) / 16 + 1;
    p.ld.counts = r->d_counts; p.ld.band = nullptr;
    p.rows = (const VariantRow*)d.rows; p.hits = c.prune_hits; p.words = words; p.max_bp = q.prune_max_bp; p.threshold = q.prune_T;
    const uint64_t blocks = (d.A + kLdRows - 1) / kLdRows;
    if (blocks > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu row blocks)", (unsigned long long)blocks);
    const size_t lds = (size_t)(kLdRows + 16 * (p.ld.n_tiles - 1)) * kLdStride;
    if (p.ld.n_tiles <= kLdSmallTiles) VS_TRY(launch_prune_hits<(int)kLdSmallTiles>(idx, p, (unsigned)blocks, lds));
    else VS_TRY(launch_prune_hits<(int)kLdMaxTiles>(idx, p, (unsigned)blocks, lds));
    hipLaunchKernelGGL(k_clump_class, dim3((unsigned)std::min<uint64_t>((d.A + kClumpBuildThreads - 1) / kClumpBuildThreads, 1u << 20)), dim3(kClumpBuildThreads), 0,
                       idx->stream, g);
    HIP_TRY(hipGetLastError());
  }
  if (g.states) {
    const uint64_t blocks = (g.states * 2 * words + kClumpBuildThreads - 1) / kClumpBuildThreads;
    if (blocks > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu blocks of verdict words)", (unsigned long long)blocks);
    hipLaunchKernelGGL(k_clump_blockers, dim3((unsigned)blocks), dim3(kClumpBuildThreads), 0, idx->stream, g);
    HIP_TRY(hipGetLastError());
  }
  if (d.Q > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu regions)", (unsigned long long)d.Q);
  hipLaunchKernelGGL(k_clump_rounds, dim3((unsigned)d.Q), dim3(kClumpThreads), 0, idx->stream, g);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}

// A trait-matrix association batch: Sy, vy and the shifts of the K traits and the limb panel, from the host's memory to the buffer
// shared_tables took from the pool.  The host's copy lives in the entry point's frame and an enqueued batch outlives that, so the
// copy is waited for here.
static int assoc_matrix_upload(SharedCtx& c) {
  vs_index* idx = c.idx;
  const AmPanel& p = *c.req.am;
  const uint32_t K = c.req.n_traits;
  if (!c.r->d.A) return VS_OK;
  std::vector<uint64_t> meta(am_meta_words(K), 0);
  memcpy(meta.data(), p.sy.data(), (size_t)K * 8);
  memcpy(meta.data() + K, p.vy.data(), (size_t)K * 8);
  memcpy(meta.data() + 2 * (size_t)K, p.shift.data(), (size_t)K * 4);
  HIP_TRY(hipMemcpyAsync(c.am_dev, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, idx->stream));
  HIP_TRY(hipMemcpyAsync(c.am_dev + meta.size(), p.bytes(), p.n_bytes(), hipMemcpyHostToDevice, idx->stream));
  HIP_TRY(hipStreamSynchronize(idx->stream));
  return VS_OK;
}

// The cells of a trait-matrix association batch from its temporary genotype matrix, the limb panel and the table's counts: one
// workgroup per (64 table rows, 16 traits), the trait tile fastest, all in one launch.
static int launch_assoc_matrix(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  const DevResult& d = r->d;
  const SharedReq& q = c.req;
  if (!d.A) return VS_OK;
  const uint32_t K = q.n_traits;
  AssocMatrixArgs a{};
  a.cells = c.ld_matrix; a.A = d.A; a.pitch = (uint32_t)r->mx_pitch; a.n_cols = q.n_cols; a.K = K; a.tiles = q.am->tiles;
  a.sy = reinterpret_cast<const int64_t*>(c.am_dev); a.vy = reinterpret_cast<const double*>(c.am_dev + K);
  a.shift = reinterpret_cast<const int32_t*>(c.am_dev + 2 * (size_t)K);
  a.panel = reinterpret_cast<const int8_t*>(c.am_dev + am_meta_words(K));
  a.counts = r->d_counts; a.out = r->d_scores;
  const uint64_t wgs = (d.A + kAmRows - 1) / kAmRows * a.tiles;
  if (wgs > 0x7FFFFFFFull) return fail(VS_ERR_ARG, "batch too large for one launch (%llu workgroups): split the batch or the traits", (unsigned long long)wgs);
  if (q.assoc_stat == VS_ASSOC_CHI2) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_assoc_matrix<true>), dim3((unsigned)wgs), dim3(256), 0, idx->stream, a);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_assoc_matrix<false>), dim3((unsigned)wgs), dim3(256), 0, idx->stream, a);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}

// An unsorted batch: every region's outcome back to its place in the caller's order (rows and lists are shared: nothing else
// moves).  Leaves `d` pointing at the caller's per-region arrays again.
static int shared_permute_out(SharedCtx& c) {
  if (!c.perm) return VS_OK;
  DevResult& d = c.r->d;
  const DevResult ds = d, &du = c.d_user;
  d.regions = du.regions; d.q_flags = du.q_flags; d.q_g0 = du.q_g0; d.q_nvar = du.q_nvar; d.q_ncar = du.q_ncar;
  d.var_begin = du.var_begin; d.car_base = du.car_base; d.q_car_len = du.q_car_len; d.var_count = du.var_count;
  hipLaunchKernelGGL(k_permute_out, dim3((unsigned)((c.n + 256) / 256)), dim3(256), 0, c.idx->stream, ds, d, (const uint32_t*)c.perm);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}

// The batch's last event and the handle's timing state; then the batch is ENQUEUED (async_submit: its sizes are known -- the
// plan's totals; a speculative batch: result_sizes --, its buffers are the result's, the timing events are read when asked) or
// waited for: k_post_done, temporaries back to the pool (async_fill: to the result), the phase times.
static int shared_finish(SharedCtx& c) {
  vs_index* idx = c.idx; vs_result* r = c.r;
  if (!c.lean) HIP_TRY(hipEventRecord(idx->ev[4], idx->stream));
  else {   // plan: the handle's two events on the plan stream; the rest: the result's pair (no separate rows kernel: ms_emit = 0)
    idx->tev[0] = idx->ev[0]; idx->tev[1] = idx->ev[1]; idx->tev[2] = r->ev_fill[0]; idx->tev[3] = r->ev_fill[0]; idx->tev[4] = r->ev_fill[1];
    idx->timing_owner = r;
  }
  idx->timing_pending = true;
  idx->timing_fill_launches = c.fill_launches;
  if (c.async_submit) {
    VS_TRY(batch_enqueued(r, c.scratch, /*record_done=*/!c.lean));
    c.ld_tmp.hand_to(r->call_temps);   // (until the completion event has passed: result_ready)
    return VS_OK;
  }
  uint64_t* done = idx->pinned + vs_index::kPinDone;
  const uint64_t seq = ++idx->done_seq;
  hipLaunchKernelGGL(k_post_done, dim3(1), dim3(1), 0, idx->stream, done, seq);
  HIP_TRY(hipGetLastError());
  VS_TRY(wait_posted(idx, done, seq, 2000));
  idx->batch_in_flight = false;
  if (c.async_fill) c.scratch.hand_to(r->bufs);
  c.scratch.release();
  c.ld_tmp.release();
  return collect_timing(idx);
}

static int run_type6_shared(vs_index* idx, const vs_region* regions, uint64_t n, vs_result* r, bool regions_on_device, const uint64_t* site_records,
                            bool allow_async, bool may_speculate, const SharedReq& req) {
  SharedCtx c(idx, r, n, req);
  c.allow_async = allow_async;
  c.site_records = site_records;
  VS_TRY(shared_setup(c, regions, regions_on_device, may_speculate));
  VS_TRY(shared_plan_batch(c));
  VS_TRY(shared_tables(c));
  VS_TRY(shared_rows(c));
  if (!c.behind_perm) VS_TRY(c.lists ? shared_expand(c) : shared_columns(c));
  VS_TRY(shared_permute_out(c));
  if (c.behind_perm) VS_TRY(shared_columns(c));
  return shared_finish(c);
}

// ---------------------------------------------------------------------------------------------------------------------
// The batches whose regions own PRIVATE rows (query types 4 and 5, the point queries, type 6 with share_lists = 0 or from
// a handful of regions' records) run through the same four stages, each a function that reads only what the stage
// before it left in the batch's context -- a mode cannot reach into another mode's temporaries:
//   batch_setup       per-region arrays of the result, regions (and sample ids) on the device
//   <mode>: bounds    k_region_bounds / k_bounds_from_records / k_point_bounds -- or the recording walk of types 4 / 5
//   batch_sizes       offsets of rows and arena by one scan; the totals cross in mapped host memory
//   batch_tables      rows (+ the expansion's per-row parameters) and arena of exactly that size
//   <mode>: rows      k_emit_headers + k_dedup_slow (+ k_has_var_filter) -- or k_emit_from_walk / the emitting walk
//   batch_fill        k_fill_carriers over the rows (async_fill: on the handle's second stream)
//   batch_finish      synchronise, temporaries back to the pool, phase times from the handle's events
// (A type-6 batch of more than 64 regions shares rows and lists between its regions: run_type6_shared above.)
// ---------------------------------------------------------------------------------------------------------------------
struct BatchCtx {
  vs_index* idx;
  vs_result* r;
  uint64_t n;
  ScratchBufs scratch;
  uint32_t* dsids = nullptr;     // one sample per region (types 4 / 5), on the device
  uint64_t* bad_ids = nullptr;   // ids that arrived in device memory: set by k_walk_setup / k_check_sample_ids, read with the batch's first sizes
  uint64_t* words = nullptr;     // a walking batch's flag words (the handle's, zero when the batch starts: batch_words): [0] bad_ids, [1] the walk's overflow word
  bool caps_done = false;        // the capacities of the recording walk were written by the batch's first kernel (k_walk_setup)
  bool lean_events = false;      // first and last event only (every event is a packet between two kernels of a string of dependent launches)
  bool resident = false;         // rows point into the index's resident arena: nothing is expanded
  bool async_fill = false;
  BatchCtx(vs_index* i, vs_result* res, uint64_t nn) : idx(i), r(res), n(nn), scratch(i) {}
};

// (`bad`: a word the batch's memset has cleared)
static int check_device_ids(vs_index* idx, const uint32_t* dsids, uint64_t n, uint64_t* bad) {
  hipLaunchKernelGGL(k_check_sample_ids, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, work_stream(idx), dsids, n, idx->g.num_samples, bad);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}
// The flag words of a walking batch (BatchCtx::words: ids out of range, the walk's overflow word).  They belong to the HANDLE and
// are zero between batches: only the part of a batch in front of its host wait writes them, the host reads them in that wait, and
// a batch that read anything but zeros (or did not get that far) leaves them marked for the one memset the next batch then pays --
// a stream of healthy batches pays none.
static int batch_words(vs_index* idx, uint64_t** words) {
  if (!idx->walk_words) {
    HIP_TRY(hipMalloc((void**)&idx->walk_words, 32));
    idx->image_allocs.push_back(idx->walk_words);
    idx->walk_words_dirty = true;
  }
  if (idx->walk_words_dirty) HIP_TRY(hipMemsetAsync(idx->walk_words, 0, 32, work_stream(idx)));
  idx->walk_words_dirty = true;   // (until this batch's host wait has read zeros: words_read_clean)
  *words = idx->walk_words;
  return VS_OK;
}
static void words_read_clean(vs_index* idx, uint64_t overflow_seen) { if (!overflow_seen) idx->walk_words_dirty = false; }
static int bad_ids_error(vs_index* idx) {
  return fail(VS_ERR_UNKNOWN_SAMPLE, "a sample id of the batch is out of range (%u samples)", idx->g.num_samples);
}

// walk_caps: -1 none; 0 / 1: the batch is a recording walk of query type 4 / 5 -- when its regions and sample ids are in device
// memory the capacities come from the same kernel that takes the copies (k_walk_setup: BatchCtx::caps_done).
static int batch_setup(BatchCtx& c, const vs_region* regions, bool regions_on_device, const uint32_t* sample_ids, int walk_caps = -1) {
  vs_index* idx = c.idx;
  vs_result* r = c.r;
  const uint64_t n = c.n;
  VS_TRY(begin_batch(idx));
  DevResult& d = r->d;
  d.Q = n;
  uint64_t* dreg = nullptr;
  VS_TRY(ralloc(r, 2 * n, &dreg));
  d.regions = dreg;
  VS_TRY(ralloc(r, n, &d.q_flags));
  VS_TRY(ralloc(r, n, &d.q_g0));
  VS_TRY(ralloc(r, n, &d.q_nvar));
  VS_TRY(ralloc(r, n, &d.q_ncar));
  VS_TRY(ralloc(r, n + 1, &d.var_begin));
  VS_TRY(ralloc(r, n + 1, &d.car_base));
  VS_TRY(ralloc(r, n, &d.var_count));
  static_assert(sizeof(vs_region) == 16, "vs_region layout");
  if (c.lean_events) HIP_TRY(hipEventRecord(idx->ev[0], work_stream(idx)));   // (in front of the first kernel, not between two)
  const bool ids_on_device = sample_ids && n && is_device_ptr(sample_ids);
  if (n && (walk_caps >= 0 || ids_on_device)) {
    VS_TRY(batch_words(idx, &c.words));
    if (ids_on_device) c.bad_ids = c.words;
  }
  if (sample_ids && n) VS_TRY(ralloc(r, n, &c.dsids));
  if (n && walk_caps >= 0 && regions && (ids_on_device || !sample_ids) && is_device_ptr(regions)) {
    const dim3 grid((unsigned)((n + 255) / 256));
    if (walk_caps == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_walk_setup<true>), grid, dim3(256), 0, work_stream(idx), idx->d, d, reinterpret_cast<const uint64_t*>(regions), sample_ids,
                                           c.dsids, idx->g.num_samples, c.words);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_walk_setup<false>), grid, dim3(256), 0, work_stream(idx), idx->d, d, reinterpret_cast<const uint64_t*>(regions), sample_ids,
                            c.dsids, idx->g.num_samples, c.words);
    HIP_TRY(hipGetLastError());
    c.caps_done = true;
  } else {
    if (n && regions) HIP_TRY(hipMemcpyAsync(dreg, regions, n * 16, regions_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDefault, work_stream(idx)));
    else if (n) HIP_TRY(hipMemsetAsync(dreg, 0, n * 16, work_stream(idx)));
    if (sample_ids && n) {
      HIP_TRY(hipMemcpyAsync(c.dsids, sample_ids, n * 4, hipMemcpyDefault, work_stream(idx)));
      if (ids_on_device) VS_TRY(check_device_ids(idx, c.dsids, n, c.bad_ids));
    }
  }
  if (!c.lean_events) HIP_TRY(hipEventRecord(idx->ev[0], work_stream(idx)));
  return VS_OK;
}

// Offsets of the rows and of the arena from the per-region counts the bounds / the walk left (q_nvar, q_ncar); the totals
// arrive in mapped host memory (read after the caller's synchronisation: batch_totals).
static int batch_sizes(BatchCtx& c) {
  DevResult& d = c.r->d;
  return scan_offsets(c.idx, d.q_nvar, d.q_ncar, c.n, d.var_begin, d.car_base, c.idx->pinned + vs_index::kPinBatch, &c.scratch.bufs);
}
static void batch_totals(const BatchCtx& c, uint64_t* rows, uint64_t* arena) {
  const volatile uint64_t* pin = c.idx->pinned + vs_index::kPinBatch;
  *rows = pin[0]; *arena = pin[1];
}

// The variant table (+ the per-row parameters of k_fill_carriers) and the arena, of exactly the sizes the scan found.
static int batch_tables(BatchCtx& c, uint64_t rows, uint64_t arena, bool shared_per_vertex, bool walking) {
  vs_index* idx = c.idx;
  vs_result* r = c.r;
  DevResult& d = r->d;
  d.A = rows;
  d.S = arena;
  VS_TRY(ralloc(r, d.A, &d.rows));
  if (!c.resident) {
    VS_TRY(ralloc(r, d.A, &d.r_class));
    VS_TRY(ralloc(r, d.A, &d.r_gt0));
  }
  r->n_rows_reported = d.A;
  r->shared_lists = shared_per_vertex;
  r->resident = c.resident;
  r->scattered_lists = shared_per_vertex || (c.resident && walking);   // a region's lists are not one arena range: texts come from a raw copy
  r->n_unique_sites = c.resident ? 0 : d.A;
  d.car_width = idx->d.wpc <= 63 ? 2 : 4;
  if (c.resident) d.carriers = idx->res_arena;
  else {
    uint8_t* a = nullptr;
    VS_TRY(ralloc(r, d.S * d.car_width + 16, &a));
    d.carriers = a;
  }
  if (!c.lean_events) HIP_TRY(hipEventRecord(idx->ev[2], idx->stream));
  return VS_OK;
}

// The carrier expansion over the rows; async_fill: on the handle's second stream behind an event, the call then returns
// once the FIRST stream is done and the call's temporaries stay with the result until it is freed.
static int batch_fill(BatchCtx& c, bool allow_async) {
  vs_index* idx = c.idx;
  vs_result* r = c.r;
  if (!c.lean_events) HIP_TRY(hipEventRecord(idx->ev[3], idx->stream));
  const uint64_t n_fill = c.resident ? 0 : r->d.A;
  c.async_fill = allow_async && idx->opts.async_fill && n_fill > 0;
  if (c.async_fill) {
    VS_TRY(ensure_fill_stream(idx));
    VS_TRY(result_events(r));
    HIP_TRY(hipEventRecord(idx->fill_ev[0], idx->stream));
    HIP_TRY(hipStreamWaitEvent(idx->fill_stream, idx->fill_ev[0], 0));
    HIP_TRY(hipEventRecord(r->ev_fill[0], idx->fill_stream));
    VS_TRY(fill_lists(idx, r->d, false, nullptr, n_fill, idx->fill_stream));
    HIP_TRY(hipEventRecord(r->ev_fill[1], idx->fill_stream));
    r->pending = true;
  } else VS_TRY(fill_lists(idx, r->d, false, nullptr, n_fill));
  idx->timing_fill_launches = n_fill ? 1 : 0;   // (async_fill: ms_fill is what the first stream saw of it, ~0; vs_result_fill_ms has the kernel's time)
  return VS_OK;
}

// enqueued: the batch returns when its last kernel is launched (the walking query types under async_submit: batch_enqueued), and the
// phase times are read from the handle's events when somebody asks (vs_index_last_timing)
static int batch_finish(BatchCtx& c, bool enqueued = false) {
  vs_index* idx = c.idx;
  HIP_TRY(hipEventRecord(idx->ev[4], idx->stream));
  if (c.lean_events) idx->timing_total_only = true;
  if (enqueued) {
    VS_TRY(batch_enqueued(c.r, c.scratch));
    idx->timing_pending = true;
    return VS_OK;
  }
  HIP_TRY(hipStreamSynchronize(idx->stream));
  idx->batch_in_flight = false;
  if (c.async_fill) c.scratch.hand_to(c.r->bufs);
  c.scratch.release();
  idx->timing_pending = true;
  return collect_timing(idx);
}

// Query type 6 with private rows (share_lists = 0, or few regions' records), and the point queries (point_mode 1 / 7: one
// next_variant_in_ref call per position -- closest_var / samples_has_var).
static int run_private_batch(vs_index* idx, const vs_region* regions, uint64_t n, vs_result* r, bool regions_on_device, const uint64_t* site_records,
                             uint32_t point_mode, const PointStrings* strings, bool allow_async) {
  BatchCtx c(idx, r, n);
  VS_TRY(batch_setup(c, regions, regions_on_device, nullptr));
  DevResult& d = r->d;
  if (n) {   // ---- bounds ----
    if (point_mode) hipLaunchKernelGGL(k_point_bounds, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, idx->stream, idx->d, d, point_mode);
    else if (site_records) hipLaunchKernelGGL(k_bounds_from_records, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, idx->stream, idx->d, d, site_records);
    else hipLaunchKernelGGL(k_region_bounds, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, idx->stream, idx->d, d);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(idx->ev[1], idx->stream));
  c.resident = idx->opts.resident_lists && idx->res_arena && !point_mode;
  VS_TRY(batch_sizes(c));
  if (c.resident) {   // the rows point into the index's arena; a region's lists ARE the arena range of its sites
    VS_TRY(ralloc(r, n, &d.q_car_len));   // (before the header kernels overwrite q_ncar with the reported carriers)
    hipLaunchKernelGGL(k_resident_bases, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, idx->stream, idx->d, d, idx->res_entries);
  }
  HIP_TRY(hipStreamSynchronize(idx->stream));
  uint64_t rows = 0, arena = 0;
  batch_totals(c, &rows, &arena);
  if (c.resident) arena = idx->res_entries;
  VS_TRY(batch_tables(c, rows, arena, false, false));
  if (n) {   // ---- rows ----
    if (c.resident) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_emit_headers<false>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, idx->stream, idx->d, d);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_emit_headers<true>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, idx->stream, idx->d, d);
    hipLaunchKernelGGL(k_dedup_slow, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, idx->stream, idx->d, d);
    if (strings) {
      uint8_t* dchars = nullptr;
      uint64_t* doff = nullptr;
      VS_TRY(ralloc(r, strings->chars->size() + 8, &dchars));
      VS_TRY(ralloc(r, strings->off->size(), &doff));
      if (!strings->chars->empty())
        HIP_TRY(hipMemcpyAsync(dchars, strings->chars->data(), strings->chars->size(), hipMemcpyHostToDevice, idx->stream));
      HIP_TRY(hipMemcpyAsync(doff, strings->off->data(), strings->off->size() * 8, hipMemcpyHostToDevice, idx->stream));
      hipLaunchKernelGGL(k_has_var_filter, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, idx->stream, idx->d, d,
                         (const uint8_t*)dchars, (const uint64_t*)doff);
    }
    HIP_TRY(hipGetLastError());
  }
  VS_TRY(batch_fill(c, allow_async && !point_mode));
  return batch_finish(c);
}

// Query type 6: more than 64 regions share rows and carrier lists (unless share_lists is 0).
static int run_type6(vs_index* idx, const vs_region* regions, uint64_t n, vs_result* r, bool regions_on_device, const uint64_t* site_records, bool allow_async) {
  if (idx->opts.share_lists && n > 64) return run_type6_shared(idx, regions, n, r, regions_on_device, site_records, allow_async);
  return run_private_batch(idx, regions, n, r, regions_on_device, site_records, 0, nullptr, allow_async);
}

// A column request (allele counts, grouped counts, association scan, burden, genotype matrix, LD band): the plan and the shared rows of type 6, then the request's own kernels
// over the rows instead of the expansion -- every batch size, never speculative, no arena (SharedCtx::lists).
static int run_column_batch(vs_index* idx, const vs_region* regions, uint64_t n, vs_result* r, const SharedReq& req) {
  return run_type6_shared(idx, regions, n, r, is_device_ptr(regions), nullptr, /*allow_async=*/true, /*may_speculate=*/false, req);
}

// lanes per region of the one-chain walks of query types 2, 3 and 5 (k_sample_walk_sc, k_sample_seq): 1, or kScGroup running the same chain
template <int MODE>
static void launch_walk_sc(vs_index* idx, const DevResult& d, uint64_t n, const uint32_t* dsids, const WalkScratch& ws) {
  // the recording walk: cooperative (eight lanes per region, episodes in parallel) where the samples' event rows name slots
  if (MODE == 2 && idx->opts.t4_walk >= 2 && idx->d.t4_events && idx->d.seq_breaks && idx->d.t4_ev_shift == 0 && idx->opts.sc_group <= 1) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sample_walk_sc_coop<8>), dim3((unsigned)((n * 8 + 255) / 256)), dim3(256), 0, work_stream(idx), idx->d, d, dsids, ws);
    return;
  }
  if (idx->opts.sc_group > 1)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sample_walk_sc<MODE, kScGroup>), dim3((unsigned)((n * kScGroup + 255) / 256)), dim3(256), 0, work_stream(idx), idx->d, d, dsids, ws);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sample_walk_sc<MODE, 1>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, work_stream(idx), idx->d, d, dsids, ws);
}
template <int MODE, int PASS>
static void launch_sample_seq(vs_index* idx, const DevSeqResult& q, uint64_t n) {
  // the single walk: cooperative (eight lanes per region, episodes in parallel) where the samples' event rows name slots
  if (PASS == 2 && idx->opts.t4_walk >= 2 && idx->d.t4_events && idx->d.seq_breaks && idx->d.t4_ev_shift == 0 && idx->opts.sc_group <= 1) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sample_seq_coop<MODE, 8>), dim3((unsigned)((n * 8 + 255) / 256)), dim3(256), 0, work_stream(idx), idx->d, q);
    return;
  }
  if (idx->opts.sc_group > 1)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sample_seq<MODE, PASS, kScGroup>), dim3((unsigned)((n * kScGroup + 255) / 256)), dim3(256), 0, work_stream(idx), idx->d, q);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sample_seq<MODE, PASS, 1>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, work_stream(idx), idx->d, q);
}

// Query types 4 (walk_mode 4: get_sample_var_in_ref, one sample's path in reference coordinates) and 5 (walk_mode 5:
// get_sample_var_in_sample).  sample_id: the one sample of the batch, or kNone with one sample per region in sample_ids.
//   walk   capacities from the type-6 bounds of the same regions (k_walk_caps_sc for type 5), ONE recording walk
//          (cooperative, serial with jumps, or literal: option t4_walk); a region that outgrows its capacity -- not seen
//          in practice; option force_fallbacks -- sends the batch down the count-then-emit pair of walks
//   claims one carrier list per reported VERTEX, shared by the rows that report it (k_t4_claim)
// ONE host wait per batch (round 5): the recording walk's scratch is sized from the handle's previous batch of the kind; a batch
// that does not fit is refused on the device (WalkAdmit: the walk's first look) and redone with the exact size (run_with_redo) -- the
// first batch of a handle and a batch 12 % bigger than any before it pay the second wait, a steady stream of batches never does.
template <typename Once>   // once(bool speculate, bool* refused)
static int run_with_redo(Once&& once) {
  bool refused = false;
  VS_TRY(once(true, &refused));
  return refused ? once(false, &refused) : VS_OK;
}
static int run_walk_batch_once(vs_index* idx, const vs_region* regions, uint64_t n, vs_result* r, uint32_t sample_id, const uint32_t* sample_ids, int walk_mode,
                               bool speculate, bool* refused) {
  BatchCtx c(idx, r, n);
  // everything in front of the host wait on the handle's second stream, beside the previous batch's rows and expansion (PreStream)
  const bool aside = idx->opts.async_submit && speculate && n > 0 && !idx->opts.force_fallbacks && !idx->opts.walk_stats && !idx->opts.lat_debug;
  if (aside) VS_TRY(ensure_plan_stream(idx));
  PreStream pre(idx, aside ? idx->plan_stream : nullptr);
  c.lean_events = aside && !idx->opts.phase_events;
  VS_TRY(batch_setup(c, regions, false, sample_ids, idx->opts.force_fallbacks ? -1 : (walk_mode == 5 ? 1 : 0)));
  DevResult& d = r->d;
  ScratchBufs& scratch = c.scratch;
  const uint32_t* dsids = c.dsids;
  WalkScratch ws{};
  uint64_t ws_capacity = 0;
  bool single_walk = false, speculative = false;
  const uint64_t* cap_total_dev = nullptr;
  DevImage dwalk = idx->d;   // what the type-4 walk sees: with or without the event bitmaps
  if (idx->opts.t4_walk == 0) dwalk.t4_events = nullptr;
  auto counting_walk = [&]() {
    if (walk_mode == 5) launch_walk_sc<0>(idx, d, n, dsids, WalkScratch{});
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sample_walk<0>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, work_stream(idx), dwalk, d, sample_id, dsids, WalkScratch{});
  };
  if (c.bad_ids && idx->opts.force_fallbacks) {   // (otherwise read with the capacities' total below: nothing before that looks at an id)
    uint64_t bad = 0;
    VS_TRY(read_device_words(idx, c.bad_ids, &bad));
    if (bad) return bad_ids_error(idx);
  }
  if (n && !idx->opts.force_fallbacks) {
    if (c.caps_done) {}   // (k_walk_setup)
    else if (walk_mode == 5) hipLaunchKernelGGL(k_walk_caps_sc, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, work_stream(idx), idx->d, d);
    else hipLaunchKernelGGL(k_region_bounds, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, work_stream(idx), idx->d, d);
    uint64_t* cap_begin = nullptr;
    VS_TRY(dev_alloc(idx, (n + 1) * 8, (void**)&cap_begin, &scratch.bufs));
    VS_TRY(exclusive_scan<uint64_t>(idx, d.q_nvar, n, cap_begin, &scratch.bufs));
    uint64_t cap_total = 0, bad = 0;
    uint64_t& hint = idx->walk_cap_hint[walk_mode == 5 ? 1 : 0];
    speculative = speculate && hint > 0 && idx->opts.async_submit;
    if (speculative) cap_total = hint;   // (the walk itself holds the batch to it: WalkAdmit)
    else {
      VS_TRY(read_device_words(idx, cap_begin + n, &cap_total, c.bad_ids, &bad));
      if (bad) return bad_ids_error(idx);
      hint = cap_total + cap_total / 8 + 1024;
    }
    cap_total_dev = cap_begin + n;
    ws_capacity = cap_total;
    ws.cap_begin = cap_begin;
    VS_TRY(dev_alloc(idx, cap_total * 8 + 8, (void**)&ws.pos, &scratch.bufs));
    VS_TRY(dev_alloc(idx, cap_total * 4 + 8, (void**)&ws.cur, &scratch.bufs));
    VS_TRY(dev_alloc(idx, cap_total * 4 + 8, (void**)&ws.ro, &scratch.bufs));
    VS_TRY(dev_alloc(idx, cap_total * 4 + 8, (void**)&ws.rl, &scratch.bufs));
    VS_TRY(dev_alloc(idx, cap_total * 4 + 8, (void**)&ws.ao, &scratch.bufs));
    VS_TRY(dev_alloc(idx, cap_total * 4 + 8, (void**)&ws.al, &scratch.bufs));
    ws.overflow = c.words + 1;   // (zero: batch_words)
    if (speculative) ws.admit = WalkAdmit{cap_total_dev, cap_total, c.bad_ids};
#ifdef VS_TUNING
    if (idx->opts.walk_stats) {
      VS_TRY(dev_alloc(idx, 128, (void**)&ws.stats, &scratch.bufs));
      HIP_TRY(hipMemsetAsync(ws.stats, 0, 128, work_stream(idx)));
    }
#endif
    if (walk_mode == 5) launch_walk_sc<2>(idx, d, n, dsids, ws);
    else if (dwalk.t4_events && idx->opts.t4_walk == 2)   // 8 lanes per region: the episodes of a region run in parallel
    {
      if (dwalk.t4_hold) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sample_walk_coop<8, false>), dim3((unsigned)((n + 31) / 32)), dim3(256), 0, work_stream(idx), dwalk, d, sample_id, dsids, ws);
      else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sample_walk_coop<8, true>), dim3((unsigned)((n + 31) / 32)), dim3(256), 0, work_stream(idx), dwalk, d, sample_id, dsids, ws);   // explicit ids
    }
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sample_walk<2>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, work_stream(idx), dwalk, d, sample_id, dsids, ws);
    HIP_TRY(hipGetLastError());
    single_walk = true;
  }
  uint64_t walk_overflow = 0;
#ifdef VS_TUNING
  if (single_walk && ws.stats) {
    unsigned long long h[16];
    HIP_TRY(hipMemcpyAsync(h, ws.stats, 128, hipMemcpyDeviceToHost, work_stream(idx)));
    HIP_TRY(hipStreamSynchronize(work_stream(idx)));
    const double nr = h[0] ? (double)h[0] : 1.0;
    fprintf(stderr, "walk stats: %llu regions | per region: search iterations %.1f (literal %.2f), jumps %.1f, steps %.1f, variants %.1f | "
            "mean ticks(10ns): search %.0f walk %.0f head %.0f | max: search iters %llu steps %llu search ticks %llu walk ticks %llu\n",
            h[0], h[1] / nr, h[2] / nr, h[3] / nr, h[4] / nr, h[7] / nr, h[5] / nr, h[6] / nr, h[12] / nr, h[8], h[9], h[10], h[11]);
  }
#endif
  if (!single_walk && n) { counting_walk(); HIP_TRY(hipGetLastError()); }
  if (!c.lean_events) HIP_TRY(hipEventRecord(idx->ev[1], work_stream(idx)));
  c.resident = idx->opts.resident_lists && idx->res_arena && single_walk;
  ListClaims lc{};
  bool share_t4 = false;   // one carrier list per reported VERTEX, shared by the rows that report it
  int claim_tab = -1;      // which of the handle's two claim tables the batch took
  uint64_t t4_arena = 0;
  VS_TRY(batch_sizes(c));

  if (single_walk && idx->opts.share_lists && n > 64 && !c.resident) {
    // (rows <= the scratch capacity the walk was given: the claim arrays can be sized before the row count is known)
    const uint64_t cap_rows = ws_capacity;
    const uint64_t gen = ++idx->t4_gen;
    const int tab = (int)(gen & 1);
    if (!idx->t4_claim[tab]) {
      HIP_TRY(hipMalloc((void**)&idx->t4_claim[tab], (idx->d.V + 1) * 8));
      idx->image_allocs.push_back(idx->t4_claim[tab]);
      HIP_TRY(hipMemsetAsync(idx->t4_claim[tab], 0, (idx->d.V + 1) * 8, work_stream(idx)));
    }
    // the table's last user (two batches back) has to be through with it: its completion event, if it returned when it was enqueued
    // (the event is the result's, pooled: should it have been recorded again since, this waits for something later -- never for less)
    if (idx->pre && idx->t4_claim_done[tab]) HIP_TRY(hipStreamWaitEvent(idx->pre, idx->t4_claim_done[tab], 0));
    idx->t4_claim_done[tab] = nullptr;
    claim_tab = tab;
    uint64_t* own_base = nullptr;
    VS_TRY(dev_alloc(idx, (cap_rows + 1) * 4, (void**)&lc.own_pad, &scratch.bufs));
    VS_TRY(dev_alloc(idx, (cap_rows + 1) * 8, (void**)&lc.own_off, &scratch.bufs));
    VS_TRY(dev_alloc(idx, (n + 1) * 8, (void**)&lc.q_own, &scratch.bufs));
    VS_TRY(dev_alloc(idx, (n + 2) * 8, (void**)&own_base, &scratch.bufs));
    lc.claim = idx->t4_claim[tab]; lc.gen = gen; lc.own_base = own_base; lc.rows_cap = cap_rows;
    hipLaunchKernelGGL(k_t4_claim, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, work_stream(idx), idx->d, d, ws, lc);
    if (n <= kScanSmallMax)   // the scan and the offsets in one launch
      hipLaunchKernelGGL(k_t4_offsets_small, dim3((unsigned)((n + kScanSmallTile - 1) / kScanSmallTile)), dim3(kScanSmallBlock), 0, work_stream(idx), d, lc, own_base);
    else {
      VS_TRY(exclusive_scan<uint64_t>(idx, (const uint64_t*)lc.q_own, n, own_base, &scratch.bufs));
      hipLaunchKernelGGL(k_t4_offsets, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, work_stream(idx), d, lc);
    }
    share_t4 = true;
  }
  // the walk's overflow flag, the claims' arena total and what the capacities added up to (the scan's totals are in mapped memory
  // already): THE host wait of a batch whose scratch was sized from the one before
  uint64_t cap_seen = 0;
  VS_TRY(read_device_words(idx, single_walk ? ws.overflow : nullptr, &walk_overflow, share_t4 ? lc.own_base + n : nullptr, &t4_arena,
                           speculative ? cap_total_dev : nullptr, &cap_seen));
  pre.done();   // (that part is over: the host has seen its last kernel's words; the rest goes on the handle's stream)
  if (c.words) words_read_clean(idx, walk_overflow);   // (ids out of range: verdict 3 in the same word, or the early return above)
  if (speculative) {
    uint64_t& hint = idx->walk_cap_hint[walk_mode == 5 ? 1 : 0];
    if (walk_overflow == 3) return bad_ids_error(idx);
    if (walk_overflow == 2) {   // refused: the caller redoes the batch with the exact size (and the next batches get the bigger scratch)
      hint = cap_seen + cap_seen / 8 + 1024;
      *refused = true;
      return VS_OK;
    }
    hint_after_batch(idx, walk_mode == 5 ? 1 : 0, hint, cap_seen);   // (batches that have become much smaller for a while: so does the scratch)
  }
  uint64_t rows = 0, arena = 0;
  batch_totals(c, &rows, &arena);
  if (share_t4 && !walk_overflow) arena = t4_arena;
  if (c.resident && !walk_overflow) arena = idx->res_entries;
  if (single_walk && walk_overflow) {   // redo the sizes with a counting walk; the emitting walk follows below
    single_walk = false;
    share_t4 = false;
    c.resident = false;
    counting_walk();
    VS_TRY(batch_sizes(c));
    HIP_TRY(hipStreamSynchronize(idx->stream));
    batch_totals(c, &rows, &arena);
  }
  VS_TRY(batch_tables(c, rows, arena, share_t4, true));
  if (n) {   // ---- rows ----
    const dim3 g16((unsigned)((n + 15) / 16)), g64((unsigned)((n + 63) / 64));
    if (single_walk && walk_mode == 5 && c.resident) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_emit_from_walk<false, 2>), g16, dim3(256), 0, idx->stream, idx->d, d, ws, lc);
    else if (single_walk && walk_mode == 5 && share_t4) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_emit_from_walk<false, 1>), g16, dim3(256), 0, idx->stream, idx->d, d, ws, lc);
    else if (single_walk && walk_mode == 5) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_emit_from_walk<false, 0>), g16, dim3(256), 0, idx->stream, idx->d, d, ws, lc);
    else if (single_walk && c.resident) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_emit_from_walk<true, 2>), g16, dim3(256), 0, idx->stream, idx->d, d, ws, lc);
    else if (single_walk && share_t4) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_emit_from_walk<true, 1>), g16, dim3(256), 0, idx->stream, idx->d, d, ws, lc);
    else if (single_walk) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_emit_from_walk<true, 0>), g16, dim3(256), 0, idx->stream, idx->d, d, ws, lc);
    else if (walk_mode == 5) launch_walk_sc<1>(idx, d, n, dsids, WalkScratch{});
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sample_walk<1>), g64, dim3(64), 0, idx->stream, dwalk, d, sample_id, dsids, WalkScratch{});
    HIP_TRY(hipGetLastError());
  }
  VS_TRY(batch_fill(c, false));
  // the batch is enqueued: return (async_submit), unless a tuning aid wants the host in the loop
  const bool enqueued = idx->opts.async_submit && single_walk && !idx->opts.walk_stats && !idx->opts.lat_debug;
  VS_TRY(batch_finish(c, enqueued));
  if (claim_tab >= 0 && enqueued) idx->t4_claim_done[claim_tab] = r->ev_done;   // (not enqueued: the stream has been synchronised)
  return VS_OK;
}
static int run_walk_batch(vs_index* idx, const vs_region* regions, uint64_t n, vs_result* r, uint32_t sample_id, const uint32_t* sample_ids, int walk_mode) {
  return run_with_redo([&](bool speculate, bool* refused) { return run_walk_batch_once(idx, regions, n, r, sample_id, sample_ids, walk_mode, speculate, refused); });
}

template <typename T>
static int fetch(vs_index* idx, std::vector<T>& h, const T* dptr, size_t n) {
  h.resize(n);
  if (n) HIP_TRY(hipMemcpyAsync(h.data(), dptr, n * sizeof(T), hipMemcpyDeviceToHost, idx->stream));
  return VS_OK;
}

// The host copies of a result.  The caller has passed the gate (result_enter): the handle's device is current and the sizes are known.
// carriers [first, first + n) of the arena as 32-bit words (id | gt << 29), whatever the arena's width
static int fetch_carriers(vs_result* r, uint64_t first, uint64_t n, std::vector<uint32_t>& out) {
  vs_index* idx = r->idx;
  VS_TRY(result_ready(r));
  out.resize(n);
  if (n == 0) return VS_OK;
  if (r->d.car_width == 4) {
    HIP_TRY(hipMemcpyAsync(out.data(), (const uint32_t*)r->d.carriers + first, n * 4, hipMemcpyDeviceToHost, idx->stream));
    HIP_TRY(hipStreamSynchronize(idx->stream));
    return VS_OK;
  }
  // 16-bit arena: copy into the upper half of the output buffer, widen in place from the front
  uint16_t* narrow = reinterpret_cast<uint16_t*>(out.data()) + n;
  HIP_TRY(hipMemcpyAsync(narrow, (const uint16_t*)r->d.carriers + first, n * 2, hipMemcpyDeviceToHost, idx->stream));
  HIP_TRY(hipStreamSynchronize(idx->stream));
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t c = narrow[i];
    out[i] = (c & 0x1FFFu) | ((c >> 13) << 29);
  }
  return VS_OK;
}

// the per-region arrays (Q-sized: a few MB for the largest batches)
static int fetch_region_meta(vs_result* r) {
  if (r->have_meta) return VS_OK;
  vs_index* idx = r->idx;
  const DevResult& d = r->d;
  VS_TRY(fetch(idx, r->h_flags, (const uint8_t*)d.q_flags, d.Q));
  VS_TRY(fetch(idx, r->h_var_begin, (const uint64_t*)d.var_begin, d.Q + 1));
  VS_TRY(fetch(idx, r->h_car_base, (const uint64_t*)d.car_base, d.Q + 1));
  VS_TRY(fetch(idx, r->h_var_count, (const uint64_t*)d.var_count, d.Q));
  VS_TRY(fetch(idx, r->h_nvar, (const uint64_t*)d.q_nvar, d.Q));
  if (d.q_car_len) VS_TRY(fetch(idx, r->h_car_len, (const uint64_t*)d.q_car_len, d.Q));
  HIP_TRY(hipStreamSynchronize(idx->stream));
  if (!d.q_car_len) {
    r->h_car_len.resize(d.Q);
    for (uint64_t q = 0; q < d.Q; ++q) r->h_car_len[q] = r->h_car_base[q + 1] - r->h_car_base[q];
  }
  for (auto& f : r->h_flags) f &= (uint8_t)~kRegionSlow;
  r->have_meta = true;
  return VS_OK;
}

// The whole variant table on the host, and the VIEW built from it: every region's rows expanded back to back (shared
// rows once per region that reports them) as the structure-of-arrays vs_result_view promises.
static int fetch_headers(vs_result* r) {
  if (r->have_headers) return VS_OK;
  vs_index* idx = r->idx;
  VS_TRY(fetch_region_meta(r));
  const DevResult& d = r->d;
  VS_TRY(fetch(idx, r->h_rows, (const VariantRow*)d.rows, d.A));
  HIP_TRY(hipStreamSynchronize(idx->stream));
  r->h_view_begin.assign(d.Q + 1, 0);
  for (uint64_t q = 0; q < d.Q; ++q) r->h_view_begin[q + 1] = r->h_view_begin[q] + r->h_nvar[q];
  const uint64_t ns = r->h_view_begin[d.Q];
  r->h_pos.resize(ns); r->h_car_begin.resize(ns); r->h_car_begin_view.resize(ns);
  r->h_ref_off.resize(ns); r->h_ref_len.resize(ns); r->h_alt_off.resize(ns); r->h_alt_len.resize(ns);
  r->h_vflags.resize(ns); r->h_car_count.resize(ns);
  uint64_t acc = 0;
  for (uint64_t q = 0; q < d.Q; ++q) {
    const VariantRow* src = r->h_rows.data() + r->h_var_begin[q];
    for (uint64_t j = 0, a = r->h_view_begin[q]; j < r->h_nvar[q]; ++j, ++a) {
      const VariantRow& v = src[j];
      const uint32_t cnt = v.count_flags & ~kRowDropped;
      r->h_pos[a] = v.pos; r->h_ref_off[a] = v.ref_off; r->h_ref_len[a] = v.ref_len; r->h_alt_off[a] = v.alt_off; r->h_alt_len[a] = v.alt_len;
      r->h_vflags[a] = (v.count_flags & kRowDropped) ? VS_VAR_DROPPED : 0u;
      r->h_car_count[a] = cnt; r->h_car_begin[a] = v.car_begin;
      r->h_car_begin_view[a] = acc; acc += cnt;
    }
  }
  r->n_view_carriers = acc;
  r->have_headers = true;
  return VS_OK;
}

// Query types 2 and 3: count pieces and bytes per region, scan, emit the piece list, decode it.  ONE host wait per batch
// (the byte total): the piece list is sized from the handle's previous batch of the type, as the walking types' scratch is (run_with_redo).
static int run_sample_seq_once(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, int mode, vs_result* r, bool speculate, bool* refused) {
  DevSeqResult& q = r->sq;
  // everything in front of the host wait on the handle's second stream, beside the previous batch's k_copy_segments (PreStream)
  const bool aside = idx->opts.async_submit && speculate && n > 0 && !idx->opts.force_fallbacks && !idx->opts.lat_debug;
  if (aside) VS_TRY(ensure_plan_stream(idx));
  PreStream pre(idx, aside ? idx->plan_stream : nullptr);
  VS_TRY(begin_batch(idx));
  q.Q = n;
  r->d.Q = n;
  uint64_t* dreg = nullptr;
  uint32_t* dsids = nullptr;
  VS_TRY(ralloc(r, 2 * n, &dreg));
  VS_TRY(ralloc(r, n, &dsids));
  q.regions = dreg; q.sids = dsids;
  VS_TRY(ralloc(r, n, &q.q_flags));
  VS_TRY(ralloc(r, n, &q.q_nseg));
  VS_TRY(ralloc(r, n, &q.q_nbytes));
  VS_TRY(ralloc(r, n + 1, &q.seg_begin));
  VS_TRY(ralloc(r, n + 1, &q.byte_begin));
  HIP_TRY(hipEventRecord(idx->ev[0], work_stream(idx)));   // (in front of the first kernel, not between two)
  uint64_t *bad_ids = nullptr, *words = nullptr;   // (the batch's flag words, batch_words: [0] ids out of range, [1] the walk's overflow word)
  bool caps_done = false;
  if (n) {
    const bool ids_on_device = is_device_ptr(sample_ids);
    VS_TRY(batch_words(idx, &words));
    if (ids_on_device) bad_ids = words;
    if (ids_on_device && !idx->opts.force_fallbacks && is_device_ptr(regions)) {   // copies, id check and piece capacities in one launch
      hipLaunchKernelGGL(k_seq_setup, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, work_stream(idx), idx->d, q, reinterpret_cast<const uint64_t*>(regions), sample_ids,
                         idx->g.num_samples, words, (uint32_t)(mode == 3));
      HIP_TRY(hipGetLastError());
      caps_done = true;
    } else {
      HIP_TRY(hipMemcpyAsync(dreg, regions, n * 16, hipMemcpyDefault, work_stream(idx)));
      HIP_TRY(hipMemcpyAsync(dsids, sample_ids, n * 4, hipMemcpyDefault, work_stream(idx)));
      if (ids_on_device) VS_TRY(check_device_ids(idx, dsids, n, bad_ids));
    }
  }
  ScratchBufs scratch(idx);
  uint64_t totals[2] = {0, 0};
  if (bad_ids && idx->opts.force_fallbacks) {
    uint64_t bad = 0;
    VS_TRY(read_device_words(idx, bad_ids, &bad));
    if (bad) return bad_ids_error(idx);
  }
  // Single walk: piece capacities from the reference range of each region, one recording walk, then the byte
  // offsets.  A region that outgrows its capacity sends the batch down the count-then-emit path.
  bool single_walk = n > 0 && !idx->opts.force_fallbacks;
  if (single_walk) {
    q.overflow = words + 1;
    q.admit = WalkAdmit{};   // (a batch that is redone with the exact size keeps its result: nothing to admit then)
    if (!caps_done) hipLaunchKernelGGL(k_seq_caps, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, work_stream(idx), idx->d, q, (uint32_t)(mode == 3));
    VS_TRY(exclusive_scan<uint64_t>(idx, q.q_nseg, n, q.seg_begin, &scratch.bufs));
    uint64_t bad = 0;
    uint64_t& hint = idx->seq_cap_hint[mode == 3 ? 1 : 0];
    const bool speculative = speculate && hint > 0 && idx->opts.async_submit;
    if (speculative) {
      totals[0] = hint;
      q.admit = WalkAdmit{q.seg_begin + n, hint, bad_ids};   // (the walk's first look: seq_void)
    } else {
      VS_TRY(read_device_words(idx, q.seg_begin + n, &totals[0], bad_ids, &bad));
      if (bad) return bad_ids_error(idx);
      hint = totals[0] + totals[0] / 8 + 1024;
    }
    VS_TRY(ralloc(r, totals[0], &q.seg_src));
    VS_TRY(ralloc(r, totals[0], &q.seg_len));
    VS_TRY(ralloc(r, totals[0], &q.seg_dst));
    q.relative = 1;
    if (mode == 2) launch_sample_seq<2, 2>(idx, q, n);
    else launch_sample_seq<3, 2>(idx, q, n);
    HIP_TRY(hipGetLastError());
    VS_TRY(exclusive_scan<uint64_t>(idx, q.q_nbytes, n, q.byte_begin, &scratch.bufs));
    uint64_t over = 0, cap_seen = 0;
    VS_TRY(read_device_words(idx, q.byte_begin + n, &totals[1], q.overflow, &over, speculative ? q.seg_begin + n : nullptr, &cap_seen));
    pre.done();   // (the rest goes on the handle's stream)
    words_read_clean(idx, over);
    if (speculative) {
      if (over == 3) return bad_ids_error(idx);
      if (over == 2) { hint = cap_seen + cap_seen / 8 + 1024; *refused = true; return VS_OK; }
      hint_after_batch(idx, mode == 3 ? 3 : 2, hint, cap_seen);
    }
    if (over) { single_walk = false; q.relative = 0; }
    else {
      VS_TRY(ralloc(r, totals[1], &q.chars));
      r->seq_bytes = totals[1];
      hipLaunchKernelGGL(k_copy_segments, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, idx->stream, idx->d, q);
      HIP_TRY(hipGetLastError());
    }
  }
  if (!single_walk) {
    if (n) {
      if (mode == 2) launch_sample_seq<2, 0>(idx, q, n);
      else launch_sample_seq<3, 0>(idx, q, n);
      HIP_TRY(hipGetLastError());
    }
    VS_TRY(exclusive_scan<uint64_t>(idx, q.q_nseg, n, q.seg_begin, &scratch.bufs));
    VS_TRY(exclusive_scan<uint64_t>(idx, q.q_nbytes, n, q.byte_begin, &scratch.bufs));
    VS_TRY(read_device_words(idx, q.seg_begin + n, &totals[0], q.byte_begin + n, &totals[1]));
    VS_TRY(ralloc(r, totals[0], &q.seg_src));
    VS_TRY(ralloc(r, totals[0], &q.seg_len));
    VS_TRY(ralloc(r, totals[0], &q.seg_dst));
    VS_TRY(ralloc(r, totals[1], &q.chars));
    r->seq_bytes = totals[1];
    if (n) {
      if (mode == 2) launch_sample_seq<2, 1>(idx, q, n);
      else launch_sample_seq<3, 1>(idx, q, n);
      hipLaunchKernelGGL(k_copy_segments, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, idx->stream, idx->d, q);
      HIP_TRY(hipGetLastError());
    }
  }
  HIP_TRY(hipEventRecord(idx->ev[4], idx->stream));
  if (idx->opts.async_submit && single_walk) {   // the batch is enqueued: return
    VS_TRY(batch_enqueued(r, scratch));
    idx->timing_pending = true; idx->timing_total_only = true;
    return VS_OK;
  }
  HIP_TRY(hipStreamSynchronize(idx->stream));
  scratch.release();
  vs_timing& t = idx->timing;
  t.ms_bounds = t.ms_scan = t.ms_emit = t.ms_fill = 0.f;
  HIP_TRY(hipEventElapsedTime(&t.ms_total, idx->ev[0], idx->ev[4]));
  t.fill_launches = 0;
  return VS_OK;
}
static int run_sample_seq(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, int mode, vs_result* r) {
  return run_with_redo([&](bool speculate, bool* refused) { return run_sample_seq_once(idx, regions, n, sample_ids, mode, r, speculate, refused); });
}

// the per-region records of any result on the handle's stream: site ranges + counts (k_pack_regions: query types 6, 4, 5, 1, 7)
// or pieces + bytes (k_pack_seq_regions: types 2, 3).  The caller has passed the gate (result_enter).
static int launch_pack_regions(vs_result* r, uint64_t* dst, uint64_t region_base) {
  vs_index* idx = r->idx;
  const uint64_t n = r->d.Q;
  if (!n) return VS_OK;
  if (r->kind == 2 || r->kind == 3) hipLaunchKernelGGL(k_pack_seq_regions, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, idx->stream, r->sq, dst, region_base);
  else hipLaunchKernelGGL(k_pack_regions, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, idx->stream, r->d, dst, region_base);
  HIP_TRY(hipGetLastError());
  return VS_OK;
}

static int fetch_sequences(vs_result* r) {   // (the caller has passed the gate)
  if (r->have_seq) return VS_OK;
  vs_index* idx = r->idx;
  VS_TRY(fetch(idx, r->h_flags, (const uint8_t*)r->sq.q_flags, r->sq.Q));
  VS_TRY(fetch(idx, r->h_byte_begin, (const uint64_t*)r->sq.byte_begin, r->sq.Q + 1));
  VS_TRY(fetch(idx, r->h_chars, (const uint8_t*)r->sq.chars, r->seq_bytes));
  HIP_TRY(hipStreamSynchronize(idx->stream));
  r->h_chars.push_back(0);
  r->have_seq = true;
  return VS_OK;
}

// Host-side SIZES of a region's answer: the arithmetic of k_region_bounds (kernels.hip.h: region_bounds_of) on the
// host copies of the rank structure, the ref-path tables and the arena prefix -- slot count and padded carrier count,
// nothing else.  The latency path allocates exactly this much and launches exactly the waves it needs; the device
// works the bounds out again for itself and refuses to write if it ever disagrees.
static uint32_t host_rank1(const HostImage& im, uint64_t p) {
  const uint64_t nbits = (uint64_t)im.bits.size() * 64;
  if (p > nbits) p = nbits;
  const uint64_t blk = p >> 9, w1 = p >> 6;
  uint32_t r = im.blk_rank[blk];
  for (uint64_t w = blk << 3; w < w1; ++w) r += (uint32_t)__builtin_popcountll(im.bits[w]);
  const uint32_t rem = (uint32_t)(p & 63);
  if (rem) r += (uint32_t)__builtin_popcountll(im.bits[w1] & ((1ULL << rem) - 1));
  return r;
}
static void host_region_size(const vs_index* idx, uint64_t x, uint64_t y, uint64_t* slots, uint64_t* arena_entries) {
  const HostImage& im = idx->im;
  *slots = 0; *arena_entries = 0;
  if (x < 1 || x > im.ref_length || !(x < y)) return;
  const uint32_t rx = host_rank1(im, x);
  if (rx >= im.R || !((uint64_t)im.idx_pos[rx] - 1 <= y)) return;   // Index::is_empty
  const uint64_t rf = (x >= im.ref_length) ? im.R - 1 : (uint64_t)rx - 1;
  const uint32_t s0 = im.rank_to_slot[rf];
  uint32_t s1 = im.rank_to_slot[host_rank1(im, y - 1)] - 1;
  if (s1 < s0) s1 = s0;
  const uint32_t g0 = im.rp_cand_prefix[s0], g1 = im.rp_cand_prefix[s1];
  *slots = g1 - g0;
  *arena_entries = idx->h_carpre[g1] - idx->h_carpre[g0];
}

// ---- resident query server (kernels.hip.h: k_query_server) ----
constexpr uint64_t kSrvMaxTasks = 2 * 16 * 4;       // (16 blocks = 64 waves share a request's 4-slot tasks) larger requests are better
                                                    // off with a launch sized for them
constexpr uint32_t kSrvStreak = 4;                  // opts.server == 1: this many small queries back to back start the server
constexpr auto kSrvStreakGap = std::chrono::microseconds(150);   // "back to back": the caller came back within this of the last answer
constexpr uint64_t kSrvLifeTicks = 2000000;         // device clock, 100 MHz: 20 ms, then the kernel leaves by itself
constexpr uint64_t kSrvIdleTicks = 100000;          // ... or 1 ms after the last request
constexpr auto kSrvHostLife = std::chrono::milliseconds(14);     // the host replaces a server older than this
constexpr auto kSrvHostIdle = std::chrono::microseconds(600);    // ... and does not trust one that has been idle this long

static ServerRequest* srv_request(vs_index* idx) { return reinterpret_cast<ServerRequest*>(idx->pinned + vs_index::kPinSrvReq); }

static int server_stop(vs_index* idx) {
  if (!idx->srv_stream) return VS_OK;
  if (idx->srv_alive) {
    volatile uint64_t* head = &srv_request(idx)->head;
    *head = ~0ULL;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    idx->srv_alive = false;
  }
  HIP_TRY(hipStreamSynchronize(idx->srv_stream));   // bounded: the kernel leaves on the exit word, or by its own clock
  return VS_OK;
}

static int server_ensure(vs_index* idx) {
  const auto now = std::chrono::steady_clock::now();
  if (idx->srv_alive && now - idx->srv_started < kSrvHostLife && now - idx->srv_last < kSrvHostIdle) return VS_OK;
  if (!idx->srv_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&idx->srv_stream, hipStreamNonBlocking));
    HIP_TRY(hipMalloc((void**)&idx->srv_counter, 8));
    idx->image_allocs.push_back(idx->srv_counter);
  }
  VS_TRY(server_stop(idx));
  ServerRequest* rq = srv_request(idx);
  memset(rq, 0, 64);
  std::atomic_thread_fence(std::memory_order_seq_cst);
  HIP_TRY(hipMemsetAsync(idx->srv_counter, 0, 8, idx->srv_stream));
  const uint32_t gt_words = fill_gt_words(idx);
  const size_t lds_bytes = fill_lds_bytes(idx);
  volatile uint64_t* resp = idx->pinned + vs_index::kPinSrvResp;
  const unsigned srv_blocks = std::max(1u, idx->opts.srv_blocks);
  if (idx->d.wpc <= 63)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_query_server<false>), dim3(srv_blocks), dim3(256), lds_bytes, idx->srv_stream, idx->d,
                       (const ServerRequest*)rq, idx->srv_counter, resp, idx->srv_seq, gt_words, kSrvLifeTicks, kSrvIdleTicks);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_query_server<true>), dim3(srv_blocks), dim3(256), lds_bytes, idx->srv_stream, idx->d,
                       (const ServerRequest*)rq, idx->srv_counter, resp, idx->srv_seq, gt_words, kSrvLifeTicks, kSrvIdleTicks);
  HIP_TRY(hipGetLastError());
  idx->srv_alive = true;
  idx->srv_started = idx->srv_last = std::chrono::steady_clock::now();
  return VS_OK;
}

// Latency path for type-6 batches of at most 64 regions: ONE launch (k_query_small), regions in the kernel arguments,
// one exact-size pooled slab for the whole result, completion through a mailbox in mapped host memory the caller
// spins on.  Returns 1 if the device found the slab too small (cannot happen unless host and device disagree; the
// caller then takes the general path).
static int run_small_type6(vs_index* idx, const vs_region* regions, uint64_t n, vs_result* r) {
  if (idx->batch_in_flight) {   // the latency path's server runs on a stream of its own and takes its slab from the pool a batch in
    idx->batch_in_flight = false;   // flight has already returned its temporaries to: that batch first
    HIP_TRY(hipStreamSynchronize(idx->stream));
  }
  const auto host_enter = std::chrono::steady_clock::now();
  idx->timing_pending = false; idx->timing_owner = nullptr; idx->timing_total_only = false;
  DevResult& d = r->d;
  uint64_t capA = 0, capS = 0, ntasks = 0;
  for (uint64_t q = 0; q < n; ++q) {
    uint64_t a = 0, c = 0;
    host_region_size(idx, regions[q].x, regions[q].y, &a, &c);
    capA += a; capS += c; ntasks += (a + kFillChunkSmall - 1) / kFillChunkSmall;
  }
  const uint32_t car_width = idx->d.wpc <= 63 ? 2 : 4;
  uint8_t* slab = nullptr;
  {  // one pooled slab for everything (two dozen pool look-ups cost microseconds at this scale)
    DevResult probe{};
    const size_t bytes = small_result_layout(probe, nullptr, n, capA, capS, car_width);
    VS_TRY(ralloc(r, bytes, &slab));
    small_result_layout(d, slab, n, capA, capS, car_width);
  }
  r->n_rows_reported = capA; r->n_unique_sites = capA; r->shared_lists = false;
  const bool lat_debug = idx->opts.lat_debug;
  vs_timing& t = idx->timing;
  const auto host_prep = std::chrono::steady_clock::now();
  // The resident server pays off for a client that asks again the moment it has its answer, and costs everybody else
  // (it holds CUs for up to 1 ms after a request; a caller slower than its idle clock pays stop + restart).  So by
  // default (opts.server == 1) it is started only once kSrvStreak small queries have arrived back to back, and a
  // caller that pauses for longer than kSrvStreakGap goes back to the single launch.
  if (idx->small_streak && host_enter - idx->last_small_done > kSrvStreakGap) idx->small_streak = 0;
  idx->small_streak++;
  const bool use_server = idx->opts.server == 2 || (idx->opts.server == 1 && idx->small_streak > kSrvStreak);
  struct StreakStamp {   // every exit of this function is "the last small query was answered now"
    vs_index* i;
    ~StreakStamp() { i->last_small_done = std::chrono::steady_clock::now(); }
  } streak_stamp{idx};
  if (!use_server && idx->srv_alive) VS_TRY(server_stop(idx));

  // ---- resident server: no launch at all (requests small enough for its 64 waves) ----
  if (use_server && ntasks <= kSrvMaxTasks) {
    VS_TRY(server_ensure(idx));
    ServerRequest* rq = srv_request(idx);
    const uint64_t seq = idx->srv_seq;
    volatile uint64_t* w = reinterpret_cast<volatile uint64_t*>(rq);
    if (n > 1) memcpy((void*)rq->xy, regions, n * 16);
    const uint64_t body[6] = {(uint64_t)slab, capA, capS, n | (lat_debug ? 1ull << 16 : 0ull) | ((uint64_t)car_width << 32),
                              regions[0].x, regions[0].y};
    for (int i = 0; i < 6; ++i) w[1 + i] = body[i];
    std::atomic_thread_fence(std::memory_order_release);
    w[7] = server_request_tail(seq, body);        // the tail seals the body (sequence number ^ checksum): a reader that
    std::atomic_thread_fence(std::memory_order_release);   // caught a half-written line sees a tail that does not match
    w[0] = seq;
    const auto posted_at = std::chrono::steady_clock::now();
    volatile uint64_t* resp = idx->pinned + vs_index::kPinSrvResp;
    const auto deadline = posted_at + std::chrono::microseconds(400);
    bool answered = false;
    while (!(answered = ((*resp & 0x3FFFFFFFFFFFFFFFull) == seq))) {
      __builtin_ia32_pause();
      if (std::chrono::steady_clock::now() > deadline) break;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (answered) {
      idx->srv_seq = seq + 1;
      const auto host_done = std::chrono::steady_clock::now();
      idx->srv_last = host_done;
      if (*resp >> 63) return 1;   // the device wanted more than the host computed: nothing was written
      if (lat_debug)
        fprintf(stderr, "server request: seen -> tasks done %.2f us, release fence %.2f us, -> last block posts %.2f us (wait on host %.2f us)\n",
                (resp[2] - resp[1]) * 0.01, (resp[3] - resp[2]) * 0.01, (double)(int64_t)(resp[4] - resp[3]) * 0.01,
                std::chrono::duration<double, std::micro>(host_done - posted_at).count());
      t.ms_bounds = std::chrono::duration<float, std::milli>(host_prep - host_enter).count();
      t.ms_scan = std::chrono::duration<float, std::milli>(posted_at - host_prep).count();
      t.ms_emit = std::chrono::duration<float, std::milli>(host_done - posted_at).count();
      t.ms_fill = 0.f;
      t.ms_total = std::chrono::duration<float, std::milli>(host_done - host_enter).count();
      t.fill_launches = 0;
      return VS_OK;
    }
    // Not answered in time: the server left between the host's check and the request (its own clock), or some of its
    // blocks did.  Whatever a block wrote is what the launch below writes again; make sure the server is gone first.
    VS_TRY(server_stop(idx));
    idx->srv_seq = seq + 1;   // a sequence number is never reused
  }

  // ---- one launch ----
  d.done_counter = idx->done_counter;
  d.done_flag = idx->pinned + vs_index::kPinFlag;
  d.done_seq = ++idx->lat_seq;
  d.host_totals = lat_debug ? idx->pinned + vs_index::kPinTotals : nullptr;
  const auto host_t0 = std::chrono::steady_clock::now();   // no HIP events here: each one is a packet on the critical path
  {
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, (ntasks + 3) / 4);
    const uint32_t gt_words = fill_gt_words(idx);
    const size_t lds_bytes = fill_lds_bytes(idx);
    const bool wide = idx->d.wpc > 63;
    if (n <= 8) {
      SmallRegions<8> regs;
      memset(&regs, 0, sizeof(regs));
      memcpy(regs.xy, regions, n * 16);
      if (!wide) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_query_small<false, 8>), dim3(blocks), dim3(256), lds_bytes, idx->stream, idx->d, d, regs, gt_words, capA, capS);
      else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_query_small<true, 8>), dim3(blocks), dim3(256), lds_bytes, idx->stream, idx->d, d, regs, gt_words, capA, capS);
    } else {
      SmallRegions<64> regs;
      memset(&regs, 0, sizeof(regs));
      memcpy(regs.xy, regions, n * 16);
      if (!wide) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_query_small<false, 64>), dim3(blocks), dim3(256), lds_bytes, idx->stream, idx->d, d, regs, gt_words, capA, capS);
      else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_query_small<true, 64>), dim3(blocks), dim3(256), lds_bytes, idx->stream, idx->d, d, regs, gt_words, capA, capS);
    }
  }
  HIP_TRY(hipGetLastError());
  const auto host_launched = std::chrono::steady_clock::now();
  {  // spin on the mailbox (the runtime's completion wait costs several microseconds more); a kernel that never posts
     // -- a fault -- is caught by the stream synchronisation after the deadline
    volatile uint64_t* flag = idx->pinned + vs_index::kPinFlag;
    const auto deadline = host_t0 + std::chrono::microseconds(300);
    bool posted = false;
    while (!(posted = ((*flag & 0x3FFFFFFFFFFFFFFFull) == d.done_seq))) {
      __builtin_ia32_pause();
      if (std::chrono::steady_clock::now() > deadline) break;
    }
    if (!posted) HIP_TRY(hipStreamSynchronize(idx->stream));
    std::atomic_thread_fence(std::memory_order_acquire);
  }
  d.done_flag = nullptr;
  d.host_totals = nullptr;
  const uint64_t posted_word = *(volatile uint64_t*)(idx->pinned + vs_index::kPinFlag);
  if ((posted_word & 0x3FFFFFFFFFFFFFFFull) != d.done_seq) return fail(VS_ERR_INTERNAL, "the latency kernel finished without posting its completion word");
  if (posted_word >> 63) return 1;  // the device wanted more than the host computed: nothing was written
  // d.A / d.S keep the host's figures: the device arrived at the same ones or it would have said so
  const volatile uint64_t* tot = idx->pinned + vs_index::kPinTotals;
  // latency path: host clock.  ms_bounds = sizing + slab, ms_scan = the launch call (or posting the request), ms_emit =
  // waiting for the mailbox, ms_fill = the kernel's own duration by the device clock (VS_LAT_DEBUG only)
  const auto host_done = std::chrono::steady_clock::now();
  t.ms_bounds = std::chrono::duration<float, std::milli>(host_prep - host_enter).count();
  t.ms_scan = std::chrono::duration<float, std::milli>(host_launched - host_t0).count();
  t.ms_emit = std::chrono::duration<float, std::milli>(host_done - host_launched).count();
  t.ms_fill = lat_debug ? (float)tot[0] * 1e-5f : 0.f;
  if (lat_debug) fprintf(stderr, "latency kernel: %.2f us total, bounds %.2f us, tasks %.2f us\n", tot[0] * 0.01, tot[1] * 0.01, tot[2] * 0.01);
  t.ms_total = std::chrono::duration<float, std::milli>(host_done - host_enter).count();   // call -> completion
  t.fill_launches = 1;
  return VS_OK;
}

// A failed call: kernels of the attempt may still be queued, so the stream is drained before the result's buffers
// go back to the pool.
static int drop_result(vs_result* r, int rc) {
  if (r->idx && r->idx->plan_stream) (void)hipStreamSynchronize(r->idx->plan_stream);
  if (r->idx && r->idx->stream) (void)hipStreamSynchronize(r->idx->stream);
  vs_result_free(r);
  return rc;
}

// The arguments every column query checks first, on the host -- also on a handle opened without a device; `batch`: its name in the message.
static int column_query_args(const vs_index* idx, const void* out, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, const char* batch) {
  if (!idx || !out || (n && !regions) || (!sample_ids && n_ids)) return fail(VS_ERR_ARG, "null argument");
  if (n == 0) return fail(VS_ERR_ARG, "%s batch needs at least one region", batch);
  if (sample_ids && n_ids == 0) return fail(VS_ERR_ARG, "an empty sample subset (pass NULL for the whole cohort)");
  return VS_OK;
}
// A sample subset as a bit per sample (id 0, "ref", is never a carrier).
static int sample_mask(const vs_index* idx, const uint32_t* sample_ids, uint64_t n_ids, std::vector<uint64_t>& mask) {
  const uint32_t ns = idx->g.num_samples;
  mask.assign((ns + 63) / 64, 0);
  for (uint64_t i = 0; i < n_ids; ++i) {
    const uint32_t id = sample_ids[i];
    if (id == 0 || id >= ns) return fail(VS_ERR_UNKNOWN_SAMPLE, "sample id %u is not a sample of the cohort (1 .. %u)", id, ns - 1);
    mask[id >> 6] |= 1ull << (id & 63);
  }
  return VS_OK;
}
// The columns of a samples-wide answer (burden, genotype matrix): the subset's mask, the columns in front of each word of it,
// and the distinct ids, ascending.  sample_ids NULL: the whole cohort, mask and rank stay empty.
static int sample_columns(const vs_index* idx, const uint32_t* sample_ids, uint64_t n_ids, std::vector<uint64_t>& mask, std::vector<uint32_t>& rank,
                          std::vector<uint32_t>& cols) {
  const uint32_t ns = idx->g.num_samples;
  if (sample_ids) {
    VS_TRY(sample_mask(idx, sample_ids, n_ids, mask));
    rank.resize(mask.size());
    for (size_t w = 0; w < mask.size(); ++w) {
      rank[w] = (uint32_t)cols.size();
      for (uint64_t m = mask[w]; m; m &= m - 1) cols.push_back((uint32_t)(w * 64 + __builtin_ctzll(m)));
    }
  } else {
    if (ns < 2) return fail(VS_ERR_ARG, "the cohort has no samples");
    cols.resize(ns - 1);
    for (uint32_t i = 0; i + 1 < ns; ++i) cols[i] = i + 1;
  }
  return VS_OK;
}

// The handle of a query: present and opened with a device.
static int query_handle(const vs_index* idx) {
  if (!idx) return fail(VS_ERR_ARG, "null argument");
  if (idx->device < 0) return fail(VS_ERR_NO_DEVICE, "index handle was opened without a device; queries run on the GPU only");
  return VS_OK;
}
static vs_result* new_result(vs_index* idx, int kind) {
  vs_result* r = new vs_result();
  r->idx = idx;
  r->kind = kind;
  idx->live_results++;
  return r;
}
// THE way a query makes its result (after its own argument checks): the handle's device is current, a live result of `kind` is
// handed to run(r); a failed run drops it (drop_result), a successful one goes to the caller.
template <typename Run>
static int make_result(vs_index* idx, int kind, vs_result** out, Run&& run) {
  VS_TRY(query_handle(idx));
  if (!out) return fail(VS_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(idx->device));
  vs_result* r = new_result(idx, kind);
  const int rc = run(r);
  if (rc != VS_OK) return drop_result(r, rc);
  *out = r;
  return VS_OK;
}

extern "C" {

const char* vs_strerror(int code) {
  switch (code) {
    case VS_OK: return "ok";
    case VS_ERR_IO: return "i/o error";
    case VS_ERR_FORMAT: return "malformed index";
    case VS_ERR_NO_DEVICE: return "no GPU device (the query path has no CPU fallback)";
    case VS_ERR_HIP: return "HIP runtime error";
    case VS_ERR_ARG: return "bad argument";
    case VS_ERR_UNKNOWN_SAMPLE: return "unknown sample";
    case VS_ERR_UNSUPPORTED: return "unsupported";
    case VS_ERR_INTERNAL: return "internal error";
    default: return "unknown error code";
  }
}
const char* vs_last_error(void) { return g_last_error.c_str(); }

void vs_index_close(vs_index* idx) {
  if (!idx) return;
  if (idx->live_results > 0 || idx->live_comms > 0) {  // results / communicators still use this handle: the last vs_result_free / vs_comm_destroy closes it
    idx->close_pending = true;
    return;
  }
  if (idx->device >= 0) {
    (void)hipSetDevice(idx->device);
    (void)server_stop(idx);
    if (idx->srv_stream) (void)hipStreamDestroy(idx->srv_stream);
    if (idx->stream) (void)hipStreamSynchronize(idx->stream);
    for (auto p : idx->image_allocs) (void)hipFree(p);
    for (auto& b : idx->pool) (void)hipFree(b.p);
    for (auto& b : idx->pin_pool) (void)hipHostFree(b.p);
    if (idx->res_mirror) (void)hipHostFree(idx->res_mirror);
    if (idx->copy_stream) (void)hipStreamDestroy(idx->copy_stream);
    if (idx->fill_stream) (void)hipStreamDestroy(idx->fill_stream);
    if (idx->plan_stream) (void)hipStreamDestroy(idx->plan_stream);
    for (auto& e : idx->fill_ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : idx->ev_pool) if (e) (void)hipEventDestroy(e);
    for (auto& e : idx->ev) if (e) (void)hipEventDestroy(e);
    if (idx->pinned) (void)hipHostFree(idx->pinned);
    if (idx->stream) (void)hipStreamDestroy(idx->stream);
  }
  delete idx;
}

int vs_index_from_vcf(const char* fasta, const char* vcf, int device, vs_construct_stats* stats, vs_index** out) {
  if (!fasta || !vcf || !out) return fail(VS_ERR_ARG, "null argument");
  vs_index* idx = new vs_index();
  try {
    uint64_t nk = 0, ne = 0, sl = 0;
    ConstructStats st = construct_from_files(fasta, vcf, idx->g, &nk, &ne, &sl);
    idx->cstats = vs_construct_stats{st.num_vars, st.num_mutations, st.num_mutations_samples, nk, ne, sl,
                                     idx->g.num_classes, (uint32_t)st.use_bit_vector};
  } catch (const std::exception& e) {
    delete idx;
    return fail(VS_ERR_IO, "%s", e.what());
  }
  if (stats) *stats = idx->cstats;
  int rc = finish_open(idx, device);
  if (rc != VS_OK) { vs_index_close(idx); return rc; }
  *out = idx;
  return VS_OK;
}

int vs_index_synthetic(const vs_synth_params* p, int device, vs_construct_stats* stats, vs_index** out) {
  if (!p || !out) return fail(VS_ERR_ARG, "null argument");
  vs_index* idx = new vs_index();
  try {
    SynthParams sp;
    sp.ref_length = p->ref_length; sp.num_variants = p->num_variants; sp.num_samples = p->num_samples;
    sp.seed = p->seed; sp.first_pos = p->first_pos; sp.frac_ins = p->frac_ins; sp.frac_del = p->frac_del;
    sp.frac_multi = p->frac_multi; sp.max_indel = p->max_indel ? p->max_indel : 1; sp.af_exponent = p->af_exponent;
    sp.sample_coordinates = p->sample_coordinates != 0;
    sp.max_af = (p->max_af > 0 && p->max_af < 0.5) ? p->max_af : 0.5;
    uint64_t nk = 0, ne = 0, sl = 0;
    SynthStats st = construct_synthetic(sp, idx->g, &nk, &ne, &sl);
    idx->cstats = vs_construct_stats{st.num_vars, st.num_mutations, st.num_mutations_samples, nk, ne, sl,
                                     idx->g.num_classes, (uint32_t)st.use_bit_vector};
  } catch (const std::exception& e) {
    delete idx;
    return fail(VS_ERR_INTERNAL, "%s", e.what());
  }
  if (stats) *stats = idx->cstats;
  int rc = finish_open(idx, device);
  if (rc != VS_OK) { vs_index_close(idx); return rc; }
  *out = idx;
  return VS_OK;
}

int vs_index_open(const char* prefix, int device, vs_index** out) {
  if (!prefix || !out) return fail(VS_ERR_ARG, "null argument");
  vs_index* idx = new vs_index();
  try {
    load_index_dir(prefix, idx->g);
  } catch (const std::exception& e) {
    delete idx;
    return fail(VS_ERR_IO, "%s", e.what());
  }
  int rc = finish_open(idx, device);
  if (rc != VS_OK) { vs_index_close(idx); return rc; }
  *out = idx;
  return VS_OK;
}

int vs_index_save(const vs_index* idx, const char* prefix) {
  if (!idx || !prefix) return fail(VS_ERR_ARG, "null argument");
  try {
    save_index_dir(idx->g, prefix);
  } catch (const std::exception& e) {
    return fail(VS_ERR_IO, "%s", e.what());
  }
  return VS_OK;
}

int vs_index_get_info(const vs_index* idx, vs_index_info* info) {
  if (!idx || !info) return fail(VS_ERR_ARG, "null argument");
  info->ref_length = idx->g.ref_length;
  info->num_vertices = idx->im.V;
  info->num_edges_csr = idx->im.E;
  info->ref_path_nodes = idx->im.P;
  info->index_nodes = idx->im.R;
  info->num_classes = idx->im.C;
  info->num_sites = idx->im.rp_cand_prefix.empty() ? 0 : idx->im.rp_cand_prefix[idx->im.P];
  info->num_carriers = idx->g.car_flags.size();
  info->seq_length = idx->g.seq.size();
  info->num_samples = idx->g.num_samples;
  info->use_bit_vector = idx->g.use_bit_vector;
  info->device_bytes = idx->device_bytes;
  info->device = idx->device;
  info->num_topology_keys = 0;
  for (uint32_t v : idx->g.topo_val) info->num_topology_keys += v != 0;
  info->list_max = idx->im.use_bit_vector ? idx->im.list_max : 0;
  info->reserved_ = 0;
  info->t4_rows_bytes = idx->t4_rows_bytes;
  info->pool_mallocs = idx->pool_mallocs;
  info->pool_frees = idx->pool_frees;
  info->t6_speculated = idx->t6_speculated;
  info->t6_refused = idx->t6_refused;
  return VS_OK;
}

int vs_index_sample_id(const vs_index* idx, const char* name, uint32_t* id) {
  if (!idx || !name || !id) return fail(VS_ERR_ARG, "null argument");
  auto it = idx->sample_ids.find(name);
  if (it == idx->sample_ids.end()) return fail(VS_ERR_UNKNOWN_SAMPLE, "Sample not found: %s", name);
  *id = it->second;
  return VS_OK;
}
const char* vs_index_sample_name(const vs_index* idx, uint32_t id) {
  if (!idx || id >= idx->g.sample_names.size()) return nullptr;
  return idx->g.sample_names[id].c_str();
}
const char* vs_index_chr(const vs_index* idx) { return idx ? idx->g.chr.c_str() : nullptr; }

int vs_index_export_plain(const vs_index* idx, const char* path) {
  if (!idx || !path) return fail(VS_ERR_ARG, "null argument");
  try {
    idx->g.write_plain(path);
  } catch (const std::exception& e) {
    return fail(VS_ERR_IO, "%s", e.what());
  }
  return VS_OK;
}

int64_t vs_index_out_neighbors(const vs_index* idx, uint32_t v, uint32_t* out, uint64_t cap) {
  if (!idx || v >= idx->im.V) return -1;
  uint32_t b = idx->im.row_ptr[v], e = idx->im.row_ptr[v + 1];
  for (uint32_t i = b; i < e && (uint64_t)(i - b) < cap; ++i) out[i - b] = idx->im.col[i];
  return (int64_t)(e - b);
}

int vs_index_set_option(vs_index* idx, const char* key, int64_t value) {
  if (!idx || !key) return fail(VS_ERR_ARG, "null argument");
  EngineOpts& o = idx->opts;
  const std::string k(key);
  if (k == "latency_server") {
    if (value < 0 || value > 2) return fail(VS_ERR_ARG, "latency_server takes 0 (never), 1 (back-to-back streaks) or 2 (always)");
    if (idx->device >= 0 && idx->srv_alive) { HIP_TRY(hipSetDevice(idx->device)); VS_TRY(server_stop(idx)); }
    o.server = (int)value; idx->small_streak = 0;
  } else if (k == "server_blocks") {
    if (value < 1 || value > 64) return fail(VS_ERR_ARG, "server_blocks takes 1..64");
    if (idx->device >= 0 && idx->srv_alive) { HIP_TRY(hipSetDevice(idx->device)); VS_TRY(server_stop(idx)); }
    o.srv_blocks = (unsigned)value;
  } else if (k == "share_lists") {
    if (value < 0 || value > 1) return fail(VS_ERR_ARG, "share_lists takes 0 (private rows and lists per region) or 1 (shared, default)");
    o.share_lists = value != 0;
  } else if (k == "resident_lists") {
    if (value != 0 && value != 1) return fail(VS_ERR_ARG, "resident_lists takes 0 or 1");
    if (value) VS_TRY(build_resident_lists(idx));   // (kept once built: switching back to 0 only stops results from using it)
    o.resident_lists = value != 0;
  } else if (k == "async_fill") o.async_fill = value != 0;
  else if (k == "async_submit") o.async_submit = value != 0;
  else if (k == "t4_walk") {
    if (value < 0 || value > 2) return fail(VS_ERR_ARG, "t4_walk takes 0 (literal), 1 (one lane per region, jumping) or 2 (cooperative, default)");
    o.t4_walk = (int)value;
  } else if (k == "t4_rows_max_mb") {
    // the per-sample rows of query type 4 on an open handle: dropped when they take more than `value` MiB (0: always), built
    // when they are absent and fit it (and half of the free memory); vs_index_get_info().t4_rows_bytes says what is there.
    // An explicit request on the open handle overrides VS_T4_NO_EVENTS of the environment (that switch only decides what open builds).
    if (value < 0) return fail(VS_ERR_ARG, "t4_rows_max_mb takes a size in MiB (0: drop the rows)");
    if (idx->device < 0) return fail(VS_ERR_ARG, "the handle has no device image");
    HIP_TRY(hipSetDevice(idx->device));
    const uint64_t cap = (uint64_t)value << 20;
    if (idx->d.t4_events && idx->t4_rows_bytes > cap) VS_TRY(drop_t4_rows(idx));
    else if (!idx->d.t4_events && cap) VS_TRY(build_t4_rows(idx, cap));
  } else if (k == "phase_events") o.phase_events = value != 0;
  else if (k == "force_fallbacks") o.force_fallbacks = value != 0;
  else if (k == "t6_speculate") o.t6_speculate = value != 0;
  else if (k == "window_chunk") {
    if (value != 0 && (value < 64 || value > 65536)) return fail(VS_ERR_ARG, "window_chunk takes 0 (default) or 64..65536 rows");
    o.window_chunk = (uint32_t)value;
  }
  else if (k == "burden_chunk") {
    if (value != 0 && (value < 64 || value > 65536)) return fail(VS_ERR_ARG, "burden_chunk takes 0 (default) or 64..65536 rows");
    o.burden_chunk = (uint32_t)value;
  } else if (k == "matrix_max_mib") {
    if (value < 0 || value > 0xFFFFFFFFll) return fail(VS_ERR_ARG, "matrix_max_mib takes 0 (default: 32 GiB) or a number of MiB");
    o.matrix_max_mib = (uint32_t)value;
  } else if (k == "assoc_lds_max_kib") {
    if (value < 0 || value > 128) return fail(VS_ERR_ARG, "assoc_lds_max_kib takes 0 (default: 32) or 1..128 KiB");
    o.assoc_lds_max_kib = (uint32_t)value;
  } else if (k == "score_chunk") {
    if (value != 0 && (value < 64 || value > 65536)) return fail(VS_ERR_ARG, "score_chunk takes 0 (default: %u) or 64..65536 rows", kScoreChunkRows);
    o.score_chunk = (uint32_t)value;
  } else if (k == "gram_chunk") {
    if (value != 0 && (value < 64 || value > kGramChunkMax)) return fail(VS_ERR_ARG, "gram_chunk takes 0 (default: by the batch's shape) or 64..%u rows", kGramChunkMax);
    o.gram_chunk = (uint32_t)value;
  } else if (k == "score_matrix_chunk") {
    if (value != 0 && (value < 128 || value > kSmChunkMax || value % 128))
      return fail(VS_ERR_ARG, "score_matrix_chunk takes 0 (default: by the batch's shape) or a multiple of 128 in 128..%u rows", kSmChunkMax);
    o.score_matrix_chunk = (uint32_t)value;
  } else if (k == "ibs_chunk") {
    if (value != 0 && (value < 64 || value > kIbsChunkMax)) return fail(VS_ERR_ARG, "ibs_chunk takes 0 (default: by the batch's shape) or 64..%u rows", kIbsChunkMax);
    o.ibs_chunk = (uint32_t)value;
  } else if (k == "trio_chunk") {
    if (value != 0 && (value < 64 || value > kTrioChunkMax || value % 64))
      return fail(VS_ERR_ARG, "trio_chunk takes 0 (default: by the batch's shape) or a multiple of 64 in 64..%u trios", kTrioChunkMax);
    o.trio_chunk = (uint32_t)value;
  } else if (k == "score_tile_cols") {
    if (value != 0 && (value < 16 || value > 65536 || value % 16)) return fail(VS_ERR_ARG, "score_tile_cols takes 0 (default) or a multiple of 16 in 16..65536");
    o.score_tile_cols = (uint32_t)value;
  } else if (k == "matrix_tile_cols") {
    if (value != 0 && (value < 16 || value > 65536 || value % 16)) return fail(VS_ERR_ARG, "matrix_tile_cols takes 0 (default) or a multiple of 16 in 16..65536");
    o.matrix_tile_cols = (uint32_t)value;
  }
  else if (k == "lat_debug" || k == "sc_group" || k == "fill_fused" || k == "fill_chunk" || k == "fill_mode" || k == "fill_dense_k" || k == "fill_stats" || k == "walk_stats" || k == "fill_ablate" ||
           k == "fill_lds_pad") {
#ifdef VS_TUNING
    if (value < 0) return fail(VS_ERR_ARG, "%s takes a non-negative value", key);
    if (k == "lat_debug") o.lat_debug = value != 0;
    else if (k == "fill_fused") o.fill_fused = value != 0;
    else if (k == "sc_group") o.sc_group = value > 1 ? 8 : 1;
    else if (k == "fill_chunk") {
      if (value != 0 && value != 8 && value != 16 && value != 32 && value != 64) return fail(VS_ERR_ARG, "fill_chunk takes 0 (by the batch's shape), 8, 16, 32 or 64");
      o.fill_chunk = (uint32_t)value;
    }
    else if (k == "fill_mode") { if (value != 0 && value != 2) return fail(VS_ERR_ARG, "fill_mode takes 0 or 2"); o.fill_mode = (int)value; }
    else if (k == "fill_dense_k") { if (value != 8 && value != 16 && value != 32 && value != 64) return fail(VS_ERR_ARG, "fill_dense_k takes 8, 16, 32 or 64"); o.fill_dense_k = (uint32_t)value; }
    else if (k == "fill_stats") o.fill_stats = value != 0;
    else if (k == "walk_stats") o.walk_stats = value != 0;
    else if (k == "fill_ablate") o.fill_ablate = (uint32_t)value & 7u;
    else o.fill_lds_pad = (size_t)value;
#else
    return fail(VS_ERR_UNSUPPORTED, "%s exists in tuning builds only (VS_BUILD_TUNING=1 python -m variantstore_amd.build --force)", key);
#endif
  } else return fail(VS_ERR_ARG, "unknown option %s", key);
  return VS_OK;
}

int vs_index_last_timing(const vs_index* cidx, vs_timing* t) {
  vs_index* idx = const_cast<vs_index*>(cidx);
  if (!idx || !t) return fail(VS_ERR_ARG, "null argument");
  if (idx->timing_pending) {   // (the last batch returned when it was enqueued: its events are read -- waited for -- here)
    HIP_TRY(hipSetDevice(idx->device));
    VS_TRY(collect_timing(idx));
  }
  *t = idx->timing;
  return VS_OK;
}

// --------------------------------------------------------------------- queries
void vs_result_free(vs_result* r) {
  if (!r) return;
  if (r->idx) {
    (void)result_device(r);
    (void)result_ready(r);
    if (r->sizes_pending) {   // a speculative batch nobody asked anything of: its totals still feed the handle's hints, its mailbox goes back
      (void)capture_totals(r);
      if (r->idx->plan_slot_owner[r->plan_slot] == r) r->idx->plan_slot_owner[r->plan_slot] = nullptr;
      r->sizes_pending = false;
    }
    if (r->idx->timing_owner == r) (void)collect_timing(r->idx);   // (its events go back to the pool below)
    for (auto& e : r->ev_fill) if (e) { r->idx->ev_pool.push_back(e); e = nullptr; }
    if (r->ev_done) { r->idx->ev_pool.push_back(r->ev_done); r->ev_done = nullptr; }
    release_bufs(r->idx, r->call_temps);   // (only where result_ready failed)
    release_bufs(r->idx, r->bufs);
    pin_release(r->idx, r->raw_pin);
    pin_release(r->idx, r->counts_pin);
    pin_release(r->idx, r->cells_pin);
    pin_release(r->idx, r->owner_pin);
    for (auto& b : r->old_pins) pin_release(r->idx, b);
    r->idx->live_results--;
    if (r->idx->close_pending && r->idx->live_results == 0 && r->idx->live_comms == 0) vs_index_close(r->idx);
  }
  delete r;
}

// ids in host memory are checked before anything is launched (ids in device memory: k_check_sample_ids, inside the batch)
static int check_host_ids(vs_index* idx, const uint32_t* sample_ids, uint64_t n) {
  if (!n || is_device_ptr(sample_ids)) return VS_OK;
  uint32_t top = 0;
  for (uint64_t i = 0; i < n; ++i) top = sample_ids[i] > top ? sample_ids[i] : top;
  if (top < idx->g.num_samples) return VS_OK;
  for (uint64_t i = 0; i < n; ++i)
    if (sample_ids[i] >= idx->g.num_samples) return fail(VS_ERR_UNKNOWN_SAMPLE, "sample id %u out of range (%u samples)", sample_ids[i], idx->g.num_samples);
  return VS_OK;
}

int vs_query_var_in_ref(vs_index* idx, const vs_region* regions, uint64_t n, vs_result** out) {
  if (n && !regions) return fail(VS_ERR_ARG, "null argument");
  return make_result(idx, 0, out, [&](vs_result* r) {
    if (n > 0 && n <= 64) {
      const int rc = run_small_type6(idx, regions, n, r);
      if (rc != 1) return rc;
      release_bufs(idx, r->bufs);   // the device asked for more than the host had sized (host and device disagree: should not happen)
      r->d = DevResult{};
    }
    return run_type6(idx, regions, n, r, false, nullptr, /*allow_async=*/true);
  });
}

int vs_query_var_in_ref_device(vs_index* idx, const vs_region* device_regions, uint64_t n, vs_result** out) {
  if (n && !device_regions) return fail(VS_ERR_ARG, "null argument");
  return make_result(idx, 0, out, [&](vs_result* r) {
    return run_type6(idx, device_regions, n, r, /*regions_on_device=*/true, nullptr, /*allow_async=*/true);
  });
}

int vs_query_expand_site_ranges(vs_index* idx, const void* device_records, uint64_t n, vs_result** out) {
  if (n && !device_records) return fail(VS_ERR_ARG, "null argument");
  return make_result(idx, 0, out, [&](vs_result* r) {
    return run_type6(idx, nullptr, n, r, false, (const uint64_t*)device_records, /*allow_async=*/false);
  });
}

// The request of a column query from the host vectors of its entry point (they outlive the batch's submission).
static SharedReq column_request(ReqKind kind, const std::vector<uint64_t>& mask, const std::vector<uint32_t>& rank, uint64_t n_cols) {
  SharedReq q;
  q.kind = kind; q.mask = mask.empty() ? nullptr : mask.data(); q.words = (uint32_t)mask.size();
  q.rank = rank.empty() ? nullptr : rank.data(); q.n_cols = (uint32_t)n_cols;
  return q;
}

int vs_query_allele_counts(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, vs_result** out) {
  VS_TRY(column_query_args(idx, out, regions, n, sample_ids, n_ids, "an allele-count"));
  std::vector<uint64_t> mask;   // (NULL: the whole cohort -- also of a cohort without samples, which the samples-wide answers refuse)
  if (sample_ids) {
    VS_TRY(sample_mask(idx, sample_ids, n_ids, mask));
    if (mask.size() * 8 > kCountMaskMaxBytes)
      return fail(VS_ERR_UNSUPPORTED, "a sample subset of a cohort of %u samples does not fit the counting kernel's LDS", idx->g.num_samples);
  }
  const SharedReq req = column_request(ReqKind::Counts, mask, {}, 0);
  return make_result(idx, kKindCounts, out, [&](vs_result* r) { return run_column_batch(idx, regions, n, r, req); });
}

// The host's checks of a grouped batch, in the documented order, and what they leave: the label table (a byte per sample id), the
// groups' sizes and names.  `whole` (window statistics): sample_ids == NULL with one group stands for the whole cohort; `pairs`: that
// query's with_pairs, which may be 0 or 1.
static int group_query_args(const vs_index* idx, const void* out, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, const uint32_t* group_of,
                            uint64_t n_ids, uint32_t n_groups, const char* const* group_names, const char* batch, bool whole, uint32_t pairs,
                            std::vector<uint64_t>& labels, std::vector<uint32_t>& sizes, std::vector<std::string>& names) {
  if (!idx || !out || (n && !regions)) return fail(VS_ERR_ARG, "null argument");
  if (n == 0) return fail(VS_ERR_ARG, "%s batch needs at least one region", batch);
  whole = whole && !sample_ids && n_groups == 1;
  if (!whole) {
    if (!sample_ids || !group_of) return fail(VS_ERR_ARG, "null argument: %s batch takes sample ids and the group of each", batch);
    if (n_ids == 0) return fail(VS_ERR_ARG, "an empty list of samples: no group has a member");
  }
  if (n_groups == 0 || n_groups > VS_GROUPS_MAX) return fail(VS_ERR_ARG, "%u groups (1 .. %u)", n_groups, VS_GROUPS_MAX);
  if (pairs > 1) return fail(VS_ERR_ARG, "with_pairs is %u: 0 (no pair records) or 1", pairs);
  const uint32_t ns = idx->g.num_samples;
  labels.assign(((size_t)ns + 7) / 8, ~0ull);   // a byte per sample id: kGroupNone = in no group
  uint8_t* lab = reinterpret_cast<uint8_t*>(labels.data());
  sizes.assign(n_groups, 0);
  if (whole) {
    for (uint32_t id = 1; id < ns; ++id) lab[id] = 0;
    sizes[0] = ns ? ns - 1 : 0;
  } else {
    for (uint64_t i = 0; i < n_ids; ++i)
      if (group_of[i] >= n_groups) return fail(VS_ERR_ARG, "group %u of sample id %u is out of range (%u groups)", group_of[i], sample_ids[i], n_groups);
    for (uint64_t i = 0; i < n_ids; ++i)
      if (sample_ids[i] == 0 || sample_ids[i] >= ns)
        return fail(VS_ERR_UNKNOWN_SAMPLE, "sample id %u is not a sample of the cohort (1 .. %u)", sample_ids[i], ns - 1);
    for (uint64_t i = 0; i < n_ids; ++i) {
      const uint32_t id = sample_ids[i], g = group_of[i];
      if (lab[id] == kGroupNone) { lab[id] = (uint8_t)g; sizes[g]++; }
      else if (lab[id] != g) return fail(VS_ERR_ARG, "sample id %u is listed in group %u and in group %u: a sample belongs to at most one group", id, (uint32_t)lab[id], g);
    }
  }
  if (group_names)
    for (uint32_t g = 0; g < n_groups; ++g) {
      if (!group_names[g]) return fail(VS_ERR_ARG, "null name of group %u", g);
      names.emplace_back(group_names[g]);
      if (names.back().find_first_of("\t\n") != std::string::npos) return fail(VS_ERR_ARG, "the name of group %u holds a tab or a newline", g);
    }
  if (labels.size() * 8 > kGroupLabelMaxBytes)
    return fail(VS_ERR_UNSUPPORTED, "the label table of a cohort of %u samples does not fit the group-count kernel's LDS (at most %zu sample ids)", ns, kGroupLabelMaxBytes);
  return VS_OK;
}

int vs_query_group_counts(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, const uint32_t* group_of, uint64_t n_ids,
                          uint32_t n_groups, const char* const* group_names, vs_result** out) {
  std::vector<uint64_t> labels;
  std::vector<uint32_t> sizes;
  std::vector<std::string> names;
  VS_TRY(group_query_args(idx, out, regions, n, sample_ids, group_of, n_ids, n_groups, group_names, "a grouped-count", false, 0, labels, sizes, names));
  const SharedReq req = column_request(ReqKind::Groups, labels, {}, n_groups);
  return make_result(idx, kKindGroups, out, [&](vs_result* r) {
    r->n_groups = n_groups;
    r->group_sizes = sizes;
    r->group_names = names;
    return run_column_batch(idx, regions, n, r, req);
  });
}

int vs_query_window_stats(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, const uint32_t* group_of, uint64_t n_ids,
                          uint32_t n_groups, const char* const* group_names, uint32_t with_pairs, vs_result** out) {
  std::vector<uint64_t> labels;
  std::vector<uint32_t> sizes;
  std::vector<std::string> names;
  VS_TRY(group_query_args(idx, out, regions, n, sample_ids, group_of, n_ids, n_groups, group_names, "a window-statistics", true, with_pairs, labels, sizes, names));
  SharedReq req = column_request(ReqKind::WindowStats, labels, {}, n_groups);
  req.ws_sizes = sizes.data();
  req.ws_pairs = with_pairs ? n_groups * (n_groups - 1) / 2 : 0;
  return make_result(idx, kKindWindowStats, out, [&](vs_result* r) {
    r->n_groups = n_groups;
    r->group_sizes = sizes;
    r->group_names = names;
    return run_column_batch(idx, regions, n, r, req);
  });
}

int vs_query_assoc_scan(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, const float* traits, uint32_t n_traits,
                        uint32_t stat, const char* const* trait_names, vs_result** out) {
  if (!idx || !out || (n && !regions)) return fail(VS_ERR_ARG, "null argument");
  if (n == 0) return fail(VS_ERR_ARG, "an association batch needs at least one region");
  if (!traits) return fail(VS_ERR_ARG, "null argument: an association batch takes the samples' phenotype values");
  if (n_traits == 0 || n_traits > VS_TRAITS_MAX) return fail(VS_ERR_ARG, "%u traits (1 .. %u)", n_traits, VS_TRAITS_MAX);
  if (stat != VS_ASSOC_DOT && stat != VS_ASSOC_CHI2) return fail(VS_ERR_ARG, "association statistic %u is neither VS_ASSOC_DOT nor VS_ASSOC_CHI2", stat);
  if (n_ids == 0) return fail(VS_ERR_ARG, "an empty list of samples: phenotypes of nobody");
  const uint32_t ns = idx->g.num_samples;
  if (!sample_ids && n_ids != (uint64_t)ns - 1)
    return fail(VS_ERR_ARG, "without sample ids the phenotypes are the whole cohort's: %llu rows given, %u samples", (unsigned long long)n_ids, ns - 1);
  std::vector<uint64_t> mask;
  std::vector<uint32_t> rank, cols;
  VS_TRY(sample_columns(idx, sample_ids, n_ids, mask, rank, cols));   // (VS_ERR_UNKNOWN_SAMPLE: id 0 or an id beyond the cohort)
  if (sample_ids && cols.size() != n_ids) {   // a sample listed twice: which of its phenotype rows would count?
    std::vector<uint64_t> seen(mask.size(), 0);
    for (uint64_t i = 0; i < n_ids; ++i) {
      const uint32_t id = sample_ids[i];
      if (seen[id >> 6] >> (id & 63) & 1) return fail(VS_ERR_ARG, "sample id %u is listed twice: a sample has one row of phenotypes", id);
      seen[id >> 6] |= 1ull << (id & 63);
    }
  }
  for (uint64_t i = 0; i < n_ids; ++i)
    for (uint32_t k = 0; k < n_traits; ++k)
      if (!std::isfinite(traits[i * n_traits + k]))
        return fail(VS_ERR_ARG, "trait %u of sample id %u is not finite: pass the subset of samples that have a value", k, sample_ids ? sample_ids[i] : (uint32_t)i + 1);
  std::vector<std::string> names;
  if (trait_names)
    for (uint32_t k = 0; k < n_traits; ++k) {
      if (!trait_names[k]) return fail(VS_ERR_ARG, "null name of trait %u", k);
      names.emplace_back(trait_names[k]);
      if (names.back().find_first_of("\t\n") != std::string::npos) return fail(VS_ERR_ARG, "the name of trait %u holds a tab or a newline", k);
    }
  if (mask.size() * 8 > kCountMaskMaxBytes)
    return fail(VS_ERR_UNSUPPORTED, "a sample subset of a cohort of %u samples does not fit the counting kernel's LDS (the whole cohort has no such limit)", ns);
  // the upload: Sy~[8], Syy~[8] and the pivots c[8] (below), then the table in column order, [column][Kp] float32 with the padding zero
  const uint32_t kp = assoc_pow2(n_traits);
  const size_t n_cols = cols.size();
  std::vector<uint64_t> pheno(kAssocHeadWords + (n_cols * kp * 4 + 7) / 8, 0);
  float* table = reinterpret_cast<float*>(pheno.data() + kAssocHeadWords);
  for (uint64_t i = 0; i < n_ids; ++i) {
    size_t col = i;
    if (sample_ids) {
      const uint32_t id = sample_ids[i];
      col = rank[id >> 6] + (size_t)__builtin_popcountll(mask[id >> 6] & ((1ull << (id & 63)) - 1ull));
    }
    for (uint32_t k = 0; k < n_traits; ++k) table[col * kp + k] = traits[i * n_traits + k];
  }
  std::vector<double> sy(n_traits, 0.0), syy(n_traits, 0.0);   // left to right in column order, from the float32 values
  for (size_t c = 0; c < n_cols; ++c)
    for (uint32_t k = 0; k < n_traits; ++k) {
      const double y = (double)table[c * kp + k];
      sy[k] += y;
      syy[k] += y * y;   // (the product of two float32 values is exact in double)
    }
  // CHI2 cancels n Sxy - Sx Sy and n Syy - Sy^2: at the scale of the trait's mean those differences lose what the statistic is made
  // of (a trait of 1e6 +- 1 keeps 3 digits of it).  The statistic does not change when a constant is taken off the trait, so the
  // three sums are taken about a pivot c_k instead: the trait VALUE nearest Sy / n (the first of equally near ones), a function of
  // the columns asked for alone.  A value of the trait's own grid keeps integer-valued traits' sums integers, and y - c, taken in
  // double, is exact unless the two lie 29 binary places apart.  DOT takes no pivot (the kernel's CHI2 parameter): its cells are
  // the bytes they were.  trait_sum / trait_sumsq stay the raw sums above.
  double* sums = reinterpret_cast<double*>(pheno.data());
  for (uint32_t k = 0; k < n_traits; ++k) {
    double c = 0.0;
    if (stat == VS_ASSOC_CHI2) {
      const double mean = sy[k] / (double)n_cols;
      double best = INFINITY;
      for (size_t j = 0; j < n_cols; ++j) {
        const double y = (double)table[j * kp + k], dist = std::fabs(y - mean);
        if (dist < best) { best = dist; c = y; }
      }
    }
    double st = 0.0, stt = 0.0;
    for (size_t j = 0; j < n_cols; ++j) {
      const double y = (double)table[j * kp + k] - c;
      st += y;
      stt += y * y;
    }
    sums[k] = st; sums[kAssocTraitsMax + k] = stt; sums[2 * kAssocTraitsMax + k] = c;
  }
  SharedReq req = column_request(ReqKind::Assoc, mask, rank, n_cols);
  req.pheno = pheno.data(); req.pheno_words = pheno.size(); req.n_traits = n_traits; req.assoc_stat = stat;
  return make_result(idx, kKindAssoc, out, [&](vs_result* r) {
    r->h_cols = cols;
    r->n_traits = n_traits; r->assoc_stat = stat;
    r->trait_sum = sy; r->trait_sumsq = syy;
    r->trait_names = names;
    return run_column_batch(idx, regions, n, r, req);
  });
}

int vs_assoc_matrix_quantise(const float* traits, uint64_t n, uint32_t n_traits, int32_t* q_out, int32_t* shift_out) {
  if (!traits || !q_out || !shift_out) return fail(VS_ERR_ARG, "null argument");
  if (n == 0 || n_traits == 0) return fail(VS_ERR_ARG, "an empty trait matrix (%llu rows x %u traits)", (unsigned long long)n, n_traits);
  if (!am_quantise(traits, (size_t)n, n_traits, q_out, shift_out)) return fail(VS_ERR_ARG, "a trait value is not finite");
  return VS_OK;
}

int vs_query_assoc_matrix(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, const float* traits, uint32_t n_traits,
                          uint32_t stat, const char* const* trait_names, vs_result** out) {
  if (!idx || !out || (n && !regions)) return fail(VS_ERR_ARG, "null argument");
  if (n == 0) return fail(VS_ERR_ARG, "an association batch needs at least one region");
  if (!traits) return fail(VS_ERR_ARG, "null argument: an association batch takes the samples' phenotype values");
  if (n_traits == 0 || n_traits > VS_TRAIT_MATRIX_MAX) return fail(VS_ERR_ARG, "%u traits (1 .. %u)", n_traits, VS_TRAIT_MATRIX_MAX);
  if (stat != VS_ASSOC_DOT && stat != VS_ASSOC_CHI2) return fail(VS_ERR_ARG, "association statistic %u is neither VS_ASSOC_DOT nor VS_ASSOC_CHI2", stat);
  if (n_ids == 0) return fail(VS_ERR_ARG, "an empty list of samples: phenotypes of nobody");
  const uint32_t ns = idx->g.num_samples;
  if (!sample_ids && n_ids != (uint64_t)ns - 1)
    return fail(VS_ERR_ARG, "without sample ids the phenotypes are the whole cohort's: %llu rows given, %u samples", (unsigned long long)n_ids, ns - 1);
  std::vector<uint64_t> mask;
  std::vector<uint32_t> rank, cols;
  VS_TRY(sample_columns(idx, sample_ids, n_ids, mask, rank, cols));   // (VS_ERR_UNKNOWN_SAMPLE: id 0 or an id beyond the cohort)
  if (sample_ids && cols.size() != n_ids) {   // a sample listed twice: which of its phenotype rows would count?
    std::vector<uint64_t> seen(mask.size(), 0);
    for (uint64_t i = 0; i < n_ids; ++i) {
      const uint32_t id = sample_ids[i];
      if (seen[id >> 6] >> (id & 63) & 1) return fail(VS_ERR_ARG, "sample id %u is listed twice: a sample has one row of phenotypes", id);
      seen[id >> 6] |= 1ull << (id & 63);
    }
  }
  AmPanel panel;
  {
    const size_t bad = am_shifts(traits, (size_t)n_ids, n_traits, panel.shift);
    if (bad != (size_t)n_ids * n_traits) {
      const size_t i = bad / n_traits;
      return fail(VS_ERR_ARG, "trait %u of sample id %u is not finite: pass the subset of samples that have a value", (uint32_t)(bad % n_traits),
                  sample_ids ? sample_ids[i] : (uint32_t)i + 1);
    }
  }
  std::vector<std::string> names;
  if (trait_names)
    for (uint32_t k = 0; k < n_traits; ++k) {
      if (!trait_names[k]) return fail(VS_ERR_ARG, "null name of trait %u", k);
      names.emplace_back(trait_names[k]);
      if (names.back().find_first_of("\t\n") != std::string::npos) return fail(VS_ERR_ARG, "the name of trait %u holds a tab or a newline", k);
    }
  const size_t n_cols = cols.size();
  if (n_cols >= kAmMaxCols)
    return fail(VS_ERR_UNSUPPORTED, "%zu columns: a trait-matrix association scan takes fewer than 2^22 samples (a 32-bit limb sum could overflow beyond)", n_cols);
  if (mask.size() * 8 > kMatrixMaskMaxBytes)
    return fail(VS_ERR_UNSUPPORTED, "a sample subset of a cohort of %u samples does not fit the matrix kernel's LDS", ns);
  // the fixed-point traits as int8 limbs in column order, and their exact sums
  std::vector<uint32_t> col_of;
  if (sample_ids) {
    col_of.resize(n_ids);
    for (uint64_t i = 0; i < n_ids; ++i) {
      const uint32_t id = sample_ids[i];
      col_of[i] = rank[id >> 6] + (uint32_t)__builtin_popcountll(mask[id >> 6] & ((1ull << (id & 63)) - 1ull));
    }
  }
  am_write_panel(traits, (size_t)n_ids, n_traits, sample_ids ? col_of.data() : nullptr, (n_cols + 15) & ~(size_t)15, panel);
  std::vector<double> sum(n_traits), sumsq(n_traits);
  for (uint32_t k = 0; k < n_traits; ++k) {
    sum[k] = std::ldexp((double)panel.sy[k], -panel.shift[k]);
    sumsq[k] = std::ldexp((double)panel.syy[k], -2 * panel.shift[k]);
  }
  SharedReq req = column_request(ReqKind::AssocMatrix, mask, rank, n_cols);
  req.am = &panel; req.n_traits = n_traits; req.assoc_stat = stat;
  return make_result(idx, kKindAssocMatrix, out, [&](vs_result* r) {
    r->h_cols = cols;
    r->n_traits = n_traits; r->assoc_stat = stat;
    r->trait_sum = sum; r->trait_sumsq = sumsq; r->trait_shift = panel.shift;
    r->trait_names = names;
    return run_column_batch(idx, regions, n, r, req);
  });
}

int vs_query_sample_scores(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, const float* weights, uint64_t n_weights,
                           uint32_t n_scores, const char* const* score_names, vs_result** out) {
  if (!idx || !out || (n && !regions)) return fail(VS_ERR_ARG, "null argument");
  if (n == 0) return fail(VS_ERR_ARG, "a score batch needs at least one region");
  if (n_scores == 0 || n_scores > VS_SCORES_MAX) return fail(VS_ERR_ARG, "%u scores (1 .. %u)", n_scores, VS_SCORES_MAX);
  if (!weights && n_weights) return fail(VS_ERR_ARG, "null argument: a score batch takes a row of weights per reported row");
  if (n_ids == 0) return fail(VS_ERR_ARG, "an empty list of samples: scores of nobody");
  const uint32_t ns = idx->g.num_samples;
  if (!sample_ids && n_ids != (uint64_t)ns - 1)
    return fail(VS_ERR_ARG, "without sample ids the scores are the whole cohort's: %llu ids announced, %u samples", (unsigned long long)n_ids, ns - 1);
  std::vector<uint64_t> mask;
  std::vector<uint32_t> rank, cols;
  VS_TRY(sample_columns(idx, sample_ids, n_ids, mask, rank, cols));   // (VS_ERR_UNKNOWN_SAMPLE: id 0 or an id beyond the cohort)
  if (sample_ids && cols.size() != n_ids) {
    std::vector<uint64_t> seen(mask.size(), 0);
    for (uint64_t i = 0; i < n_ids; ++i) {
      const uint32_t id = sample_ids[i];
      if (seen[id >> 6] >> (id & 63) & 1) return fail(VS_ERR_ARG, "sample id %u is listed twice: a sample has one row of scores", id);
      seen[id >> 6] |= 1ull << (id & 63);
    }
  }
  std::vector<std::string> names;
  if (score_names)
    for (uint32_t k = 0; k < n_scores; ++k) {
      if (!score_names[k]) return fail(VS_ERR_ARG, "null name of score %u", k);
      names.emplace_back(score_names[k]);
      if (names.back().find_first_of("\t\n") != std::string::npos) return fail(VS_ERR_ARG, "the name of score %u holds a tab or a newline", k);
    }
  if (n_weights >= kScoreMaxReports)
    return fail(VS_ERR_ARG, "%llu rows of weights: a score batch takes fewer than 2^26 reported rows (the 64-bit sums could overflow beyond): split the batch",
                (unsigned long long)n_weights);
  SharedReq req = column_request(ReqKind::Scores, mask, rank, cols.size());
  req.weights = weights; req.n_weights = n_weights; req.n_scores = n_scores;
  req.weights_on_device = weights && is_device_ptr(weights);
  if (!req.weights_on_device)   // host weights: finite, and the largest |w| per column, before the device is asked
    for (uint64_t i = 0; i < n_weights; ++i)
      for (uint32_t k = 0; k < n_scores; ++k) {
        uint32_t b;
        memcpy(&b, weights + i * n_scores + k, 4);
        b &= 0x7FFFFFFFu;
        if (b >= 0x7F800000u) return fail(VS_ERR_ARG, "weight column %u holds a value that is not finite (row %llu)", k, (unsigned long long)i);
        if (b > req.score_max_bits[k]) req.score_max_bits[k] = b;
      }
  if (mask.size() * 8 > kCountMaskMaxBytes)
    return fail(VS_ERR_UNSUPPORTED, "a sample subset of a cohort of %u samples does not fit the score kernel's LDS (the whole cohort has no such limit)", ns);
  return make_result(idx, kKindScores, out, [&](vs_result* r) {
    r->h_cols = cols;
    r->n_scores = n_scores;
    r->score_names = names;
    return run_column_batch(idx, regions, n, r, req);
  });
}

int vs_query_score_matrix(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, const float* weights, uint64_t n_weights,
                          uint32_t n_scores, const char* const* score_names, vs_result** out) {
  if (!idx || !out || (n && !regions)) return fail(VS_ERR_ARG, "null argument");
  if (n == 0) return fail(VS_ERR_ARG, "a score-matrix batch needs at least one region");
  if (n_scores == 0 || n_scores > VS_SCORE_MATRIX_MAX) return fail(VS_ERR_ARG, "%u scores (1 .. %u)", n_scores, VS_SCORE_MATRIX_MAX);
  if (!weights && n_weights) return fail(VS_ERR_ARG, "null argument: a score-matrix batch takes a row of weights per reported row");
  // the weights: finite, and f_k from the largest |w| of every column, before the device is asked
  std::vector<int32_t> shift;
  {
    const size_t bad = am_shifts(weights, (size_t)n_weights, n_scores, shift);
    if (bad != (size_t)n_weights * n_scores)
      return fail(VS_ERR_ARG, "weight column %u holds a value that is not finite (row %llu)", (uint32_t)(bad % n_scores), (unsigned long long)(bad / n_scores));
  }
  std::vector<std::string> names;
  if (score_names)
    for (uint32_t k = 0; k < n_scores; ++k) {
      if (!score_names[k]) return fail(VS_ERR_ARG, "null name of score %u", k);
      names.emplace_back(score_names[k]);
      if (names.back().find_first_of("\t\n") != std::string::npos) return fail(VS_ERR_ARG, "the name of score %u holds a tab or a newline", k);
    }
  if (n_ids == 0) return fail(VS_ERR_ARG, "an empty list of samples: scores of nobody");
  const uint32_t ns = idx->g.num_samples;
  if (!sample_ids && n_ids != (uint64_t)ns - 1)
    return fail(VS_ERR_ARG, "without sample ids the scores are the whole cohort's: %llu ids announced, %u samples", (unsigned long long)n_ids, ns - 1);
  std::vector<uint64_t> mask;
  std::vector<uint32_t> rank, cols;
  VS_TRY(sample_columns(idx, sample_ids, n_ids, mask, rank, cols));   // (VS_ERR_UNKNOWN_SAMPLE: id 0 or an id beyond the cohort)
  if (sample_ids && cols.size() != n_ids) {
    std::vector<uint64_t> seen(mask.size(), 0);
    for (uint64_t i = 0; i < n_ids; ++i) {
      const uint32_t id = sample_ids[i];
      if (seen[id >> 6] >> (id & 63) & 1) return fail(VS_ERR_ARG, "sample id %u is listed twice: a sample has one row of scores", id);
      seen[id >> 6] |= 1ull << (id & 63);
    }
  }
  if (n_weights >= kSmMaxReports)
    return fail(VS_ERR_ARG, "%llu rows of weights: a score-matrix batch takes fewer than 2^26 reported rows (the 64-bit sums could overflow beyond): split the batch",
                (unsigned long long)n_weights);
  if (mask.size() * 8 > kMatrixMaskMaxBytes)
    return fail(VS_ERR_UNSUPPORTED, "a sample subset of a cohort of %u samples does not fit the matrix kernel's LDS", ns);
  SharedReq req = column_request(ReqKind::ScoreMatrix, mask, rank, cols.size());
  req.weights = weights; req.n_weights = n_weights; req.n_scores = n_scores;
  return make_result(idx, kKindScoreMatrix, out, [&](vs_result* r) {
    r->h_cols = cols;
    r->n_scores = n_scores;
    r->score_names = names;
    r->score_shift = shift;
    return run_column_batch(idx, regions, n, r, req);
  });
}

int vs_query_sample_burden(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, uint32_t min_ac, uint32_t max_ac,
                           vs_result** out) {
  VS_TRY(column_query_args(idx, out, regions, n, sample_ids, n_ids, "a burden"));
  if (min_ac > max_ac) return fail(VS_ERR_ARG, "an empty allele-count window [%u, %u]", min_ac, max_ac);
  const uint32_t ns = idx->g.num_samples;
  std::vector<uint64_t> mask;
  std::vector<uint32_t> rank, cols;
  VS_TRY(sample_columns(idx, sample_ids, n_ids, mask, rank, cols));
  const uint64_t n_cols = cols.size();
  if (n > (1ull << 31) / n_cols)
    return fail(VS_ERR_ARG, "a burden matrix of %llu regions x %llu columns exceeds 2^31 cells (%llu GiB at 16 bytes a cell): split the batch",
                (unsigned long long)n, (unsigned long long)n_cols, (unsigned long long)((n >> 26) * n_cols));
  if (mask.size() * 8 > kBurdenMaskMaxBytes) return fail(VS_ERR_UNSUPPORTED, "a sample subset of a cohort of %u samples does not fit the burden kernel's LDS", ns);
  SharedReq req = column_request(ReqKind::Burden, mask, rank, n_cols);
  req.min_ac = min_ac; req.max_ac = max_ac;
  return make_result(idx, kKindBurden, out, [&](vs_result* r) {
    r->h_cols = cols;
    return run_column_batch(idx, regions, n, r, req);
  });
}

int vs_query_genotype_matrix(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, vs_result** out) {
  VS_TRY(column_query_args(idx, out, regions, n, sample_ids, n_ids, "a genotype-matrix"));
  std::vector<uint64_t> mask;
  std::vector<uint32_t> rank, cols;
  VS_TRY(sample_columns(idx, sample_ids, n_ids, mask, rank, cols));
  if (mask.size() * 8 > kMatrixMaskMaxBytes)
    return fail(VS_ERR_UNSUPPORTED, "a sample subset of a cohort of %u samples does not fit the matrix kernel's LDS", idx->g.num_samples);
  const SharedReq req = column_request(ReqKind::Matrix, mask, rank, cols.size());
  return make_result(idx, kKindMatrix, out, [&](vs_result* r) {
    r->h_cols = cols;
    return run_column_batch(idx, regions, n, r, req);
  });
}

int vs_query_ld_band(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, uint32_t window, uint32_t stat,
                     vs_result** out) {
  VS_TRY(column_query_args(idx, out, regions, n, sample_ids, n_ids, "an LD"));
  if (window == 0 || window > kLdMaxWindow) return fail(VS_ERR_ARG, "an LD window of %u rows (1 .. %u)", window, kLdMaxWindow);
  if (stat != VS_LD_DOT && stat != VS_LD_R2) return fail(VS_ERR_ARG, "LD statistic %u is neither VS_LD_DOT nor VS_LD_R2", stat);
  std::vector<uint64_t> mask;
  std::vector<uint32_t> rank, cols;
  VS_TRY(sample_columns(idx, sample_ids, n_ids, mask, rank, cols));
  if (mask.size() * 8 > kMatrixMaskMaxBytes)
    return fail(VS_ERR_UNSUPPORTED, "a sample subset of a cohort of %u samples does not fit the matrix kernel's LDS", idx->g.num_samples);
  SharedReq req = column_request(ReqKind::LD, mask, rank, cols.size());
  req.ld_window = window; req.ld_stat = stat;
  return make_result(idx, kKindLd, out, [&](vs_result* r) {
    r->h_cols = cols;
    return run_column_batch(idx, regions, n, r, req);
  });
}

int vs_query_ld_matrix(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, uint32_t stat, vs_result** out) {
  VS_TRY(column_query_args(idx, out, regions, n, sample_ids, n_ids, "an LD-matrix"));
  if (stat != VS_LD_DOT && stat != VS_LD_R2) return fail(VS_ERR_ARG, "LD statistic %u is neither VS_LD_DOT nor VS_LD_R2", stat);
  std::vector<uint64_t> mask;
  std::vector<uint32_t> rank, cols;
  VS_TRY(sample_columns(idx, sample_ids, n_ids, mask, rank, cols));
  if (mask.size() * 8 > kMatrixMaskMaxBytes)
    return fail(VS_ERR_UNSUPPORTED, "a sample subset of a cohort of %u samples does not fit the matrix kernel's LDS", idx->g.num_samples);
  SharedReq req = column_request(ReqKind::LdMatrix, mask, rank, cols.size());
  req.ld_stat = stat;
  return make_result(idx, kKindLdMatrix, out, [&](vs_result* r) {
    r->h_cols = cols;
    return run_column_batch(idx, regions, n, r, req);
  });
}

int vs_query_ld_prune(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, uint32_t window, uint32_t max_bp,
                      uint32_t threshold_q20, uint32_t min_ac, uint32_t max_ac, vs_result** out) {
  VS_TRY(column_query_args(idx, out, regions, n, sample_ids, n_ids, "an LD-pruning"));
  if (window == 0 || window > kLdMaxWindow) return fail(VS_ERR_ARG, "an LD-pruning window of %u rows (1 .. %u)", window, kLdMaxWindow);
  if (threshold_q20 > kPruneThresholdOne)
    return fail(VS_ERR_ARG, "an LD-pruning threshold of %u / 2^20 (0 .. %u: r2 between 0 and 1)", threshold_q20, kPruneThresholdOne);
  if (min_ac > max_ac) return fail(VS_ERR_ARG, "an empty allele-count window [%u, %u]", min_ac, max_ac);
  std::vector<uint64_t> mask;
  std::vector<uint32_t> rank, cols;
  VS_TRY(sample_columns(idx, sample_ids, n_ids, mask, rank, cols));
  if (cols.size() >= (1ull << 21))
    return fail(VS_ERR_UNSUPPORTED, "an LD pruning over %llu columns: the exact comparison takes fewer than 2^21", (unsigned long long)cols.size());
  if (mask.size() * 8 > kMatrixMaskMaxBytes)
    return fail(VS_ERR_UNSUPPORTED, "a sample subset of a cohort of %u samples does not fit the matrix kernel's LDS", idx->g.num_samples);
  SharedReq req = column_request(ReqKind::Prune, mask, rank, cols.size());
  req.ld_window = window;
  req.prune_max_bp = max_bp; req.prune_T = threshold_q20; req.prune_min_ac = min_ac; req.prune_max_ac = max_ac;
  return make_result(idx, kKindPrune, out, [&](vs_result* r) {
    r->h_cols = cols;
    return run_column_batch(idx, regions, n, r, req);
  });
}

int vs_query_ld_scores(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, uint32_t window, uint32_t max_bp,
                       uint32_t min_ac, uint32_t max_ac, vs_result** out) {
  VS_TRY(column_query_args(idx, out, regions, n, sample_ids, n_ids, "an LD-score"));
  if (min_ac > max_ac) return fail(VS_ERR_ARG, "an empty allele-count window [%u, %u]", min_ac, max_ac);
  std::vector<uint64_t> mask;
  std::vector<uint32_t> rank, cols;
  VS_TRY(sample_columns(idx, sample_ids, n_ids, mask, rank, cols));
  if (cols.size() >= (1ull << 21))
    return fail(VS_ERR_UNSUPPORTED, "LD scores over %llu columns: the exact quotient takes fewer than 2^21", (unsigned long long)cols.size());
  if (mask.size() * 8 > kMatrixMaskMaxBytes)
    return fail(VS_ERR_UNSUPPORTED, "a sample subset of a cohort of %u samples does not fit the matrix kernel's LDS", idx->g.num_samples);
  SharedReq req = column_request(ReqKind::LdScore, mask, rank, cols.size());
  req.ld_window = window;
  req.prune_max_bp = max_bp; req.prune_min_ac = min_ac; req.prune_max_ac = max_ac;
  return make_result(idx, kKindLdScore, out, [&](vs_result* r) {
    r->h_cols = cols;
    return run_column_batch(idx, regions, n, r, req);
  });
}

// The key of a p-value in [0, 1]: the bit pattern of the non-negative double (-0.0 counts as 0), monotone in p.  False outside
// [0, 1] and for a NaN.
static bool clump_key(double p, uint64_t* key) {
  if (!(p >= 0.0 && p <= 1.0)) return false;
  memcpy(key, &p, 8);
  *key &= ~(1ull << 63);   // (-0.0)
  return true;
}

int vs_query_ld_clump(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, const double* pvalues, uint64_t n_pvalues,
                      uint32_t window, uint32_t max_bp, uint32_t threshold_q20, double p1, double p2, vs_result** out) {
  VS_TRY(column_query_args(idx, out, regions, n, sample_ids, n_ids, "an LD-clumping"));
  if (window == 0 || window > kLdMaxWindow) return fail(VS_ERR_ARG, "an LD-clumping window of %u rows (1 .. %u)", window, kLdMaxWindow);
  if (threshold_q20 > kPruneThresholdOne)
    return fail(VS_ERR_ARG, "an LD-clumping threshold of %u / 2^20 (0 .. %u: r2 between 0 and 1)", threshold_q20, kPruneThresholdOne);
  if (!pvalues) return fail(VS_ERR_ARG, "null argument: a clumping batch takes a p-value per table row (pvalues)");
  uint64_t key1 = 0, key2 = 0;
  if (!clump_key(p1, &key1)) return fail(VS_ERR_ARG, "an index p-value bound p1 of %g (0 .. 1)", p1);
  if (!clump_key(p2, &key2)) return fail(VS_ERR_ARG, "a clump p-value bound p2 of %g (0 .. 1)", p2);
  if (key1 > key2) return fail(VS_ERR_ARG, "p1 = %g above p2 = %g: the bound of the index rows may not exceed the bound of the clumped rows", p1, p2);
  std::vector<uint64_t> keys((size_t)n_pvalues);
  for (uint64_t i = 0; i < n_pvalues; ++i) {
    const double p = pvalues[i];
    if (p != p) keys[i] = kClumpNoKey;
    else if (!clump_key(p, &keys[i])) return fail(VS_ERR_ARG, "the p-value of table row %llu is %g: a p-value lies in 0 .. 1 (NaN: none)", (unsigned long long)i, p);
  }
  std::vector<uint64_t> mask;
  std::vector<uint32_t> rank, cols;
  VS_TRY(sample_columns(idx, sample_ids, n_ids, mask, rank, cols));
  if (cols.size() >= (1ull << 21))
    return fail(VS_ERR_UNSUPPORTED, "an LD clumping over %llu columns: the exact comparison takes fewer than 2^21", (unsigned long long)cols.size());
  if (mask.size() * 8 > kMatrixMaskMaxBytes)
    return fail(VS_ERR_UNSUPPORTED, "a sample subset of a cohort of %u samples does not fit the matrix kernel's LDS", idx->g.num_samples);
  SharedReq req = column_request(ReqKind::Clump, mask, rank, cols.size());
  req.ld_window = window;
  req.prune_max_bp = max_bp; req.prune_T = threshold_q20;
  req.n_pvalues = n_pvalues; req.clump_key[0] = key1; req.clump_key[1] = key2;
  return make_result(idx, kKindClump, out, [&](vs_result* r) {
    r->h_cols = cols;
    r->h_clump_keys = std::move(keys);
    r->clump_key[0] = key1; r->clump_key[1] = key2;
    memcpy(r->clump_p, r->clump_key, 16);
    req.clump_keys = r->h_clump_keys.data();
    return run_column_batch(idx, regions, n, r, req);
  });
}

int vs_query_sample_gram(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, uint32_t stat, vs_result** out) {
  VS_TRY(column_query_args(idx, out, regions, n, sample_ids, n_ids, "a Gram"));
  if (stat != VS_GRAM_DOT && stat != VS_GRAM_GRM) return fail(VS_ERR_ARG, "Gram statistic %u is neither VS_GRAM_DOT nor VS_GRAM_GRM", stat);
  std::vector<uint64_t> mask;
  std::vector<uint32_t> rank, cols;
  VS_TRY(sample_columns(idx, sample_ids, n_ids, mask, rank, cols));
  if (mask.size() * 8 > kMatrixMaskMaxBytes)
    return fail(VS_ERR_UNSUPPORTED, "a sample subset of a cohort of %u samples does not fit the matrix kernel's LDS", idx->g.num_samples);
  SharedReq req = column_request(ReqKind::Gram, mask, rank, cols.size());
  req.gram_stat = stat;
  return make_result(idx, kKindGram, out, [&](vs_result* r) {
    r->h_cols = cols;
    return run_column_batch(idx, regions, n, r, req);
  });
}

int vs_query_sample_ibs(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, uint32_t stat, vs_result** out) {
  VS_TRY(column_query_args(idx, out, regions, n, sample_ids, n_ids, "an IBS"));
  if (stat != VS_IBS_COUNTS && stat != VS_IBS_KING) return fail(VS_ERR_ARG, "IBS statistic %u is neither VS_IBS_COUNTS nor VS_IBS_KING", stat);
  std::vector<uint64_t> mask;
  std::vector<uint32_t> rank, cols;
  VS_TRY(sample_columns(idx, sample_ids, n_ids, mask, rank, cols));
  if (mask.size() * 8 > kMatrixMaskMaxBytes)
    return fail(VS_ERR_UNSUPPORTED, "a sample subset of a cohort of %u samples does not fit the matrix kernel's LDS", idx->g.num_samples);
  SharedReq req = column_request(ReqKind::Ibs, mask, rank, cols.size());
  req.ibs_stat = stat;
  return make_result(idx, kKindIbs, out, [&](vs_result* r) {
    r->h_cols = cols;
    return run_column_batch(idx, regions, n, r, req);
  });
}

int vs_query_trio_scan(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* trios, uint64_t n_trios, vs_result** out) {
  VS_TRY(column_query_args(idx, out, regions, n, nullptr, 0, "a trio"));
  if (!trios) return fail(VS_ERR_ARG, "null argument: a trio batch takes three sample ids per trio (trios)");
  if (n_trios == 0 || n_trios > VS_TRIOS_MAX) return fail(VS_ERR_ARG, "a trio batch of %llu trios (1 .. %u)", (unsigned long long)n_trios, VS_TRIOS_MAX);
  const uint32_t ns = idx->g.num_samples;
  for (uint64_t t = 0; t < n_trios; ++t) {
    const uint32_t c = trios[3 * t], f = trios[3 * t + 1], m = trios[3 * t + 2];
    if (c == f || c == m || f == m)
      return fail(VS_ERR_ARG, "trio %llu names a sample twice (child %u, father %u, mother %u): its three members are distinct", (unsigned long long)t, c, f, m);
    for (uint32_t id : {c, f, m})
      if (id == 0 || id >= ns) return fail(VS_ERR_UNKNOWN_SAMPLE, "sample id %u of trio %llu is not a sample of the cohort (1 .. %u)", id, (unsigned long long)t, ns - 1);
  }
  std::vector<uint64_t> mask;
  std::vector<uint32_t> rank, cols;
  VS_TRY(sample_columns(idx, trios, 3 * n_trios, mask, rank, cols));
  if (cols.size() > kTrioTileBytes)
    return fail(VS_ERR_UNSUPPORTED, "a trio scan over %llu distinct members: a staged row must fit the kernel's LDS tile, at most %u", (unsigned long long)cols.size(), kTrioTileBytes);
  if (mask.size() * 8 > kMatrixMaskMaxBytes)
    return fail(VS_ERR_UNSUPPORTED, "a sample subset of a cohort of %u samples does not fit the matrix kernel's LDS", idx->g.num_samples);
  std::vector<uint32_t> tcols((size_t)(3 * n_trios));   // id -> column: the members in front of the id's mask word and inside it
  for (size_t i = 0; i < tcols.size(); ++i) {
    const uint32_t id = trios[i];
    tcols[i] = rank[id >> 6] + (uint32_t)__builtin_popcountll(mask[id >> 6] & ((1ull << (id & 63)) - 1));
  }
  SharedReq req = column_request(ReqKind::Trio, mask, rank, cols.size());
  req.n_trios = n_trios;
  return make_result(idx, kKindTrio, out, [&](vs_result* r) {
    r->h_cols = cols;
    r->h_trio_cols = std::move(tcols);
    req.trio_cols = r->h_trio_cols.data();
    return run_column_batch(idx, regions, n, r, req);
  });
}

int vs_query_roh(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, const vs_roh_params* params, vs_result** out) {
  VS_TRY(column_query_args(idx, out, regions, n, sample_ids, n_ids, "a ROH"));
  if (!params) return fail(VS_ERR_ARG, "null argument: a ROH batch takes its parameters (params)");
  if (params->min_sites == 0) return fail(VS_ERR_ARG, "a ROH segment of at least 0 sites (min_sites is 1 or more)");
  if (params->max_het > kRohMaxHet) return fail(VS_ERR_ARG, "a ROH run absorbing %u heterozygous sites (max_het is 0 .. %u)", params->max_het, kRohMaxHet);
  if (params->min_ac > params->max_ac) return fail(VS_ERR_ARG, "an empty allele-count window [%u, %u]", params->min_ac, params->max_ac);
  std::vector<uint64_t> mask;
  std::vector<uint32_t> rank, cols;
  VS_TRY(sample_columns(idx, sample_ids, n_ids, mask, rank, cols));
  if (mask.size() * 8 > kMatrixMaskMaxBytes)
    return fail(VS_ERR_UNSUPPORTED, "a sample subset of a cohort of %u samples does not fit the matrix kernel's LDS", idx->g.num_samples);
  SharedReq req = column_request(ReqKind::Roh, mask, rank, cols.size());
  req.roh = *params;
  req.roh.segments = params->segments ? 1u : 0u;
  return make_result(idx, kKindRoh, out, [&](vs_result* r) {
    r->h_cols = cols;
    return run_column_batch(idx, regions, n, r, req);
  });
}

int vs_query_sample_var_in_ref(vs_index* idx, const vs_region* regions, uint64_t n, uint32_t sample_id, vs_result** out) {
  if (!out || (n && !regions)) return fail(VS_ERR_ARG, "null argument");
  VS_TRY(query_handle(idx));
  if (sample_id >= idx->g.num_samples) return fail(VS_ERR_UNKNOWN_SAMPLE, "sample id %u out of range (%u samples)", sample_id, idx->g.num_samples);
  return make_result(idx, 0, out, [&](vs_result* r) { return run_walk_batch(idx, regions, n, r, sample_id, nullptr, 4); });
}

// the argument checks of a batch with one sample per region
static int check_sample_batch(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, vs_result** out,
                              bool need_index) {
  if (!out || (n && (!regions || !sample_ids))) return fail(VS_ERR_ARG, "null argument");
  VS_TRY(query_handle(idx));
  VS_TRY(check_host_ids(idx, sample_ids, n));
  if (need_index && !idx->d.has_car_index)
    return fail(VS_ERR_ARG, "this index holds no sample coordinates (built without them); query types 2, 3 and 5 need them");
  return VS_OK;
}

int vs_query_samples_var_in_ref(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids,
                                vs_result** out) {
  VS_TRY(check_sample_batch(idx, regions, n, sample_ids, out, false));
  return make_result(idx, 0, out, [&](vs_result* r) { return run_walk_batch(idx, regions, n, r, kNone, sample_ids, 4); });
}

static int run_point_batch(vs_index* idx, const uint64_t* positions, uint64_t n, uint32_t mode, const PointStrings* strings,
                           vs_result** out) {
  return make_result(idx, mode == 7 ? 7 : 0, out, [&](vs_result* r) {
    std::vector<vs_region> regions(n);
    for (uint64_t i = 0; i < n; ++i) regions[i] = vs_region{positions[i], 0};
    return run_private_batch(idx, regions.data(), n, r, false, nullptr, mode, strings, false);
  });
}

int vs_query_closest_var(vs_index* idx, const uint64_t* positions, uint64_t n, vs_result** out) {
  if (!idx || !out || (n && !positions)) return fail(VS_ERR_ARG, "null argument");
  return run_point_batch(idx, positions, n, 1, nullptr, out);
}

int vs_query_samples_has_var(vs_index* idx, const uint64_t* positions, const char* const* refs, const char* const* alts,
                             uint64_t n, vs_result** out) {
  if (!idx || !out || (n && (!positions || !refs || !alts))) return fail(VS_ERR_ARG, "null argument");
  std::vector<uint8_t> chars;
  std::vector<uint64_t> off(2 * n + 1, 0);
  for (uint64_t i = 0; i < n; ++i) {
    if (!refs[i] || !alts[i]) return fail(VS_ERR_ARG, "null ref/alt string at query %llu", (unsigned long long)i);
    off[2 * i] = chars.size();
    chars.insert(chars.end(), (const uint8_t*)refs[i], (const uint8_t*)refs[i] + strlen(refs[i]));
    off[2 * i + 1] = chars.size();
    chars.insert(chars.end(), (const uint8_t*)alts[i], (const uint8_t*)alts[i] + strlen(alts[i]));
  }
  off[2 * n] = chars.size();
  PointStrings ps{&chars, &off};
  return run_point_batch(idx, positions, n, 7, &ps, out);
}

int vs_query_sample_seq(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, int sample_coordinates,
                        vs_result** out) {
  VS_TRY(check_sample_batch(idx, regions, n, sample_ids, out, true));
  const int kind = sample_coordinates ? 3 : 2;
  return make_result(idx, kind, out, [&](vs_result* r) { return run_sample_seq(idx, regions, n, sample_ids, kind, r); });
}

int vs_query_sample_var_in_sample(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, vs_result** out) {
  VS_TRY(check_sample_batch(idx, regions, n, sample_ids, out, true));
  static const uint32_t none = 0;
  return make_result(idx, 0, out, [&](vs_result* r) { return run_walk_batch(idx, regions, n, r, kNone, n ? sample_ids : &none, 5); });
}

int vs_result_get_sequences(vs_result* r, uint64_t* n_regions, const uint8_t** region_flags, const uint64_t** seq_begin,
                            const char** chars) {
  VS_TRY(result_enter(r, Want::Sequences, true));
  VS_TRY(fetch_sequences(r));
  if (n_regions) *n_regions = r->sq.Q;
  if (region_flags) *region_flags = r->h_flags.data();
  if (seq_begin) *seq_begin = r->h_byte_begin.data();
  if (chars) *chars = (const char*)r->h_chars.data();
  return VS_OK;
}

int vs_index_draw_subgraph(const vs_index* idx, uint64_t pos, uint64_t radius, const char* sample, const char* outfile) {
  if (!idx || !outfile) return fail(VS_ERR_ARG, "null argument");
  uint32_t sid = 0;
  if (sample && *sample && std::string(sample) != "ref") {
    auto it = idx->sample_ids.find(sample);
    if (it == idx->sample_ids.end()) return fail(VS_ERR_UNKNOWN_SAMPLE, "Sample not found: %s", sample);
    sid = it->second;
  }
  try {
    const std::string text = dot_text(idx->g, draw_start_vertex(idx->g, pos, sid), radius);
    FILE* f = fopen(outfile, "wb");
    if (!f) return fail(VS_ERR_IO, "Can't open the file graph output: %s", outfile);
    fwrite(text.data(), 1, text.size(), f);
    fclose(f);
  } catch (const std::exception& e) {
    return fail(VS_ERR_INTERNAL, "%s", e.what());
  }
  return VS_OK;
}

int vs_index_find(vs_index* idx, const uint64_t* pos, uint64_t n, uint32_t* vertex_out) {
  if (!idx || (n && (!pos || !vertex_out))) return fail(VS_ERR_ARG, "null argument");
  if (idx->device < 0) return fail(VS_ERR_NO_DEVICE, "index handle was opened without a device");
  HIP_TRY(hipSetDevice(idx->device));
  if (n == 0) return VS_OK;
  ScratchBufs tmp(idx);
  void *dp = nullptr, *dout = nullptr;
  VS_TRY(dev_alloc(idx, n * 8, &dp, &tmp.bufs));
  VS_TRY(dev_alloc(idx, n * 4, &dout, &tmp.bufs));
  HIP_TRY(hipMemcpyAsync(dp, pos, n * 8, hipMemcpyHostToDevice, idx->stream));
  hipLaunchKernelGGL(k_find, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, idx->stream, idx->d, (const uint64_t*)dp, n, (uint32_t*)dout);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(vertex_out, dout, n * 4, hipMemcpyDeviceToHost, idx->stream));
  HIP_TRY(hipStreamSynchronize(idx->stream));
  tmp.release();
  return VS_OK;
}

// ---------------------------------------------------------------- result access
// `bytes` of a result's array in device memory into page-locked memory owned by the result (`pin`), once; `what`: its name in the
// error text.  An empty array: no copy, the (16-byte) buffer is there all the same.  (The caller has passed the gate.)
static int array_to_host(vs_result* r, const void* dev, size_t bytes, DevBuf* pin, const char* what) {
  if (pin->p) return VS_OK;
  vs_index* idx = r->idx;
  VS_TRY(result_ready(r));
  DevBuf b{nullptr, 0};
  VS_TRY(pin_alloc(idx, bytes + 16, &b));
  if (bytes) {
    const hipError_t e = hipMemcpyAsync(b.p, dev, bytes, hipMemcpyDeviceToHost, idx->stream);
    const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(idx->stream) : e;
    if (e2 != hipSuccess) { pin_release(idx, b); return fail(VS_ERR_HIP, "copy of the %s failed: %s", what, hipGetErrorString(e2)); }
  }
  *pin = b;
  return VS_OK;
}
// block_begin of an LD-matrix result ([Q + 1]; the scan that wrote it was waited for when the batch was sized)
static int ld_block_begin_to_host(vs_result* r) {
  if (!r->h_block_begin.empty()) return VS_OK;
  VS_TRY(fetch(r->idx, r->h_block_begin, (const uint64_t*)r->d_ldm_meta, (size_t)r->d.Q + 1));
  HIP_TRY(hipStreamSynchronize(r->idx->stream));
  return VS_OK;
}
// keep_begin [Q + 1] and n_kept of a pruning result (the walk writes n_kept: the batch must have finished)
static int prune_meta_to_host(vs_result* r) {
  if (!r->h_prune_meta.empty()) return VS_OK;
  VS_TRY(result_ready(r));
  // (a clumping result: n_index in n_kept's place, and behind the scan's summary and the cell total the rounds of every region)
  VS_TRY(fetch(r->idx, r->h_prune_meta, (const uint64_t*)r->d_prune_meta, r->kind == kKindClump ? 3 * ((size_t)r->d.Q + 1) + 4 : r->kind == kKindLdScore ? 3 * ((size_t)r->d.Q + 1) : 2 * ((size_t)r->d.Q + 1)));
  HIP_TRY(hipStreamSynchronize(r->idx->stream));
  return VS_OK;
}
static int counts_to_host(vs_result* r) {   // (a grouped-count result: n_groups records per row)
  const size_t per_row = r->kind == kKindGroups ? r->n_groups : 1;
  return array_to_host(r, r->d_counts, (size_t)r->d.A * per_row * sizeof(uint4), &r->counts_pin, "allele counts");
}
// the records and pair records of a window-statistics result, one piece
static size_t window_stats_bytes(const vs_result* r) { return (size_t)r->d.Q * (48 * (size_t)r->n_groups + 16 * (size_t)r->ws_pairs); }
// Start (stream) the raw copy of a result: rows and -- on request -- the arena go into one page-locked block.  (The caller has passed
// the gate.)
static int raw_copy_begin(vs_result* r, bool with_carriers, hipStream_t stream) {
  vs_index* idx = r->idx;
  const DevResult& d = r->d;
  const size_t row_bytes = (size_t)d.A * sizeof(VariantRow), arena_bytes = with_carriers && !r->resident ? (size_t)d.S * d.car_width : 0;
  if (r->raw_rows && (r->raw_arena || !with_carriers)) return VS_OK;
  if (with_carriers) VS_TRY(result_ready(r));
  if (with_carriers && r->resident) VS_TRY(ensure_resident_mirror(idx));   // the rows point into the handle's mirror of the resident arena
  if (r->raw_pin.p) { r->old_pins.push_back(r->raw_pin); r->raw_pin = DevBuf{nullptr, 0}; r->raw_rows = nullptr; r->raw_arena = nullptr; }
  VS_TRY(pin_alloc(idx, row_bytes + arena_bytes + 64, &r->raw_pin));
  uint8_t* base = (uint8_t*)r->raw_pin.p;
  if (row_bytes) HIP_TRY(hipMemcpyAsync(base, d.rows, row_bytes, hipMemcpyDeviceToHost, stream));
  const size_t arena_at = (row_bytes + 63) & ~(size_t)63;
  if (arena_bytes) HIP_TRY(hipMemcpyAsync(base + arena_at, d.carriers, arena_bytes, hipMemcpyDeviceToHost, stream));
  r->raw_rows = (const VariantRow*)base;
  r->raw_arena = !with_carriers ? nullptr : r->resident ? (const uint8_t*)idx->res_mirror : base + arena_at;
  return VS_OK;
}
static void fill_raw(vs_result* r, vs_result_raw* raw) {
  raw->n_regions = r->d.Q;
  raw->region_flags = r->h_flags.data();
  raw->row_begin = r->h_var_begin.data();
  raw->row_count = r->h_nvar.data();
  raw->var_count = r->h_var_count.data();
  raw->car_base = r->h_car_base.data();
  raw->car_len = r->h_car_len.data();
  raw->n_rows = r->d.A;
  raw->rows = (const vs_variant_row*)r->raw_rows;
  raw->arena_entries = r->d.S;
  raw->carrier_bytes = r->d.car_width;
  raw->arena = r->raw_arena;
  raw->seq_pool = r->idx->seq_chars.data();
  raw->shared = (r->shared_lists ? 1 : 0) | (r->resident ? 2 : 0) | (r->scattered_lists ? 4 : 0);
  if (r->scattered_lists) { raw->car_base = nullptr; raw->car_len = nullptr; }   // a region's lists are not one arena range: rows[].car_begin alone addresses them
}

int vs_result_get_raw(vs_result* r, int with_carriers, vs_result_raw* raw) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!raw) return fail(VS_ERR_ARG, "null argument");
  if (no_lists(r) && with_carriers) return refuse_no_lists(r, "vs_result_get_raw with carriers");
  static_assert(sizeof(vs_variant_row) == sizeof(VariantRow), "row layout of the ABI");
  vs_index* idx = r->idx;
  VS_TRY(raw_copy_begin(r, with_carriers != 0, idx->stream));
  VS_TRY(fetch_region_meta(r));   // (synchronises the stream)
  HIP_TRY(hipStreamSynchronize(idx->stream));
  fill_raw(r, raw);
  return VS_OK;
}

// Type 6 over a large batch with the results leaving the GPU as they are produced: the batch is cut into chunks of
// `chunk_regions`; while chunk k + 1 is computed, the raw copy of chunk k (rows + carrier arena) crosses PCIe on a
// second stream into one of two page-locked buffers, and `fn` is called with it.  The regions must be sorted for the
// chunks to share rows and lists (each chunk is a batch of its own).
int vs_query_var_in_ref_stream(vs_index* idx, const vs_region* regions, uint64_t n, uint64_t chunk_regions, int with_carriers,
                               vs_chunk_fn fn, void* user) {
  if ((n && !regions) || !fn) return fail(VS_ERR_ARG, "null argument");
  VS_TRY(query_handle(idx));
  if (chunk_regions == 0) return fail(VS_ERR_ARG, "chunk_regions must be positive");
  HIP_TRY(hipSetDevice(idx->device));
  if (!idx->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&idx->copy_stream, hipStreamNonBlocking));
  vs_result* in_flight = nullptr;   // chunk whose copy is under way
  uint64_t in_flight_first = 0;
  int rc = VS_OK;
  auto deliver = [&]() -> int {
    if (!in_flight) return VS_OK;
    int rcd = VS_OK;
    if (hipStreamSynchronize(idx->copy_stream) != hipSuccess) rcd = fail(VS_ERR_HIP, "copy of a result chunk failed");
    if (rcd == VS_OK) {
      vs_result_raw raw;
      fill_raw(in_flight, &raw);
      if (fn(user, in_flight_first, &raw) != 0) rcd = fail(VS_ERR_ARG, "the chunk callback asked to stop");
    }
    vs_result_free(in_flight);
    in_flight = nullptr;
    return rcd;
  };
  for (uint64_t first = 0; first < n && rc == VS_OK; first += chunk_regions) {
    const uint64_t cn = std::min<uint64_t>(chunk_regions, n - first);
    vs_result* r = new_result(idx, 0);   // (never speculative, and on the handle's device: the chunk's helpers below need no gate)
    rc = run_type6(idx, regions + first, cn, r, false, nullptr, /*allow_async=*/false);   // (returns with the chunk's kernels complete; the previous chunk's copy ran beside them)
    if (rc == VS_OK) rc = fetch_region_meta(r);
    if (rc != VS_OK) { drop_result(r, rc); break; }
    const int rcd = deliver();                           // the previous chunk
    if (rcd != VS_OK) { vs_result_free(r); rc = rcd; break; }
    rc = raw_copy_begin(r, with_carriers != 0, idx->copy_stream);
    if (rc != VS_OK) { vs_result_free(r); break; }
    in_flight = r;
    in_flight_first = first;
  }
  const int rcd = deliver();
  return rc != VS_OK ? rc : rcd;
}

int vs_result_get_view(vs_result* r, int with_carriers, vs_result_view* view) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!view) return fail(VS_ERR_ARG, "null argument");
  if (no_lists(r) && with_carriers) return refuse_no_lists(r, "vs_result_get_view with carriers");
  VS_TRY(fetch_headers(r));
  if (with_carriers && !r->have_carriers) {
    // the arena pads every variant's range; the view packs the lists back to back
    r->h_carriers.resize(r->n_view_carriers);
    const uint64_t ns = r->h_view_begin[r->d.Q];
    if (r->resident) {   // from the handle's mirror of the resident arena
      VS_TRY(ensure_resident_mirror(r->idx));
      const uint16_t* m16 = (const uint16_t*)r->idx->res_mirror;
      const uint32_t* m32 = (const uint32_t*)r->idx->res_mirror;
      for (uint64_t a = 0; a < ns; ++a) {
        uint32_t* dst = r->h_carriers.data() + r->h_car_begin_view[a];
        const uint64_t src = r->h_car_begin[a];
        if (r->d.car_width == 4) { if (r->h_car_count[a]) memcpy(dst, m32 + src, (size_t)r->h_car_count[a] * 4); }
        else for (uint32_t k = 0; k < r->h_car_count[a]; ++k) { const uint32_t c = m16[src + k]; dst[k] = (c & 0x1FFFu) | ((c >> 13) << 29); }
      }
    } else {
    std::vector<uint32_t> arena;
    VS_TRY(fetch_carriers(r, 0, r->d.S, arena));
    for (uint64_t a = 0; a < ns; ++a)
      if (r->h_car_count[a])
        memcpy(r->h_carriers.data() + r->h_car_begin_view[a], arena.data() + r->h_car_begin[a], (size_t)r->h_car_count[a] * 4);
    }
    r->have_carriers = true;
  }
  view->n_regions = r->d.Q;
  view->region_flags = r->h_flags.data();
  view->var_begin = r->h_view_begin.data();
  view->var_count = r->h_var_count.data();
  view->n_slots = r->h_view_begin[r->d.Q];
  view->pos = r->h_pos.data();
  view->ref_off = r->h_ref_off.data(); view->ref_len = r->h_ref_len.data();
  view->alt_off = r->h_alt_off.data(); view->alt_len = r->h_alt_len.data();
  view->var_flags = r->h_vflags.data();
  view->car_begin = r->h_car_begin_view.data();
  view->car_count = r->h_car_count.data();
  view->n_carriers = r->n_view_carriers;
  view->carriers = (with_carriers || r->have_carriers) ? r->h_carriers.data() : nullptr;
  view->seq_pool = r->idx->seq_chars.data();
  return VS_OK;
}

int vs_result_totals(const vs_result* cr, uint64_t* n_regions, uint64_t* n_variants, uint64_t* n_carriers, uint64_t* n_bases) {
  vs_result* r = const_cast<vs_result*>(cr);
  VS_TRY(result_enter(r, Want::Any, true));
  if (r->kind == 2 || r->kind == 3) {  // sequences: only regions and bases
    if (n_regions) *n_regions = r->sq.Q;
    if (n_variants) *n_variants = 0;
    if (n_carriers) *n_carriers = 0;
    if (n_bases) *n_bases = r->seq_bytes;
    return VS_OK;
  }
  if (!r->have_totals) {   // reduced on the device: nothing but three words crosses PCIe
    vs_index* idx = r->idx;
    ScratchBufs tmp(idx);
    void* dt = nullptr;
    VS_TRY(dev_alloc(idx, 24, &dt, &tmp.bufs));
    HIP_TRY(hipMemsetAsync(dt, 0, 24, idx->stream));
    if (r->d.Q) {
      hipLaunchKernelGGL(k_result_totals, dim3((unsigned)((r->d.Q + 3) / 4)), dim3(256), 0, idx->stream, r->d, (unsigned long long*)dt);
      HIP_TRY(hipGetLastError());
    }
    uint64_t h[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, dt, 24, hipMemcpyDeviceToHost, idx->stream));
    HIP_TRY(hipStreamSynchronize(idx->stream));
    tmp.release();
    r->n_variants = h[0]; r->n_carriers_kept = h[1]; r->n_bases = h[2];
    if (r->kind == kKindCounts || r->kind == kKindAssoc || r->kind == kKindAssocMatrix) {   // the carriers that lie in the subset: the counts of the rows every region reports (dropped rows count 0)
      VS_TRY(fetch_region_meta(r));
      VS_TRY(counts_to_host(r));
      const uint4* c = (const uint4*)r->counts_pin.p;
      uint64_t nc = 0;
      for (uint64_t q = 0; q < r->d.Q; ++q)
        for (uint64_t a = r->h_var_begin[q], e = a + r->h_nvar[q]; a < e; ++a) nc += c[a].x;
      r->n_carriers_kept = nc;
    }
    if (r->kind == kKindScores) {   // the (report, carrier in S) pairs whose report has a nonzero weight: the walk's own word
      VS_TRY(result_ready(r));
      uint64_t nc = 0;
      HIP_TRY(hipMemcpyAsync(&nc, &r->d_score_meta->n_pairs, 8, hipMemcpyDeviceToHost, idx->stream));
      HIP_TRY(hipStreamSynchronize(idx->stream));
      r->n_carriers_kept = nc;
    }
    if (r->kind == kKindGroups) {   // the same over every group: a carrier in no group counts nowhere
      VS_TRY(fetch_region_meta(r));
      VS_TRY(counts_to_host(r));
      const uint4* c = (const uint4*)r->counts_pin.p;
      const uint64_t G = r->n_groups;
      uint64_t nc = 0;
      for (uint64_t q = 0; q < r->d.Q; ++q)
        for (uint64_t a = r->h_var_begin[q] * G, e = a + r->h_nvar[q] * G; a < e; ++a) nc += c[a].x;
      r->n_carriers_kept = nc;
    }
    if (r->kind == kKindWindowStats) {   // as a grouped-count result's: carriers = (alt_alleles + heterozygotes) / 2, summed over regions and groups
      VS_TRY(array_to_host(r, r->d_wstats, window_stats_bytes(r), &r->cells_pin, "window statistics"));
      const vs_window_stats* w = (const vs_window_stats*)r->cells_pin.p;
      uint64_t nc = 0;
      for (uint64_t i = 0, e = r->d.Q * r->n_groups; i < e; ++i) nc += (w[i].sum_ac + w[i].obs_het) / 2;
      r->n_carriers_kept = nc;
    }
    if (r->kind == kKindBurden || r->kind == kKindMatrix || r->kind == kKindLd || r->kind == kKindLdMatrix || r->kind == kKindPrune || r->kind == kKindClump || r->kind == kKindLdScore || r->kind == kKindGram || r->kind == kKindIbs || r->kind == kKindTrio || r->kind == kKindRoh || r->kind == kKindScoreMatrix) {   // (LD, LD matrix, Gram, IBS, trio, ROH: of the matrix the band / the products were formed from) the sum of `variants` over the burden matrix, the nonzero cells of the genotype matrix: the kernels' own word
      VS_TRY(result_ready(r));
      uint64_t nc = 0;
      HIP_TRY(hipMemcpyAsync(&nc, r->d_cell_total, 8, hipMemcpyDeviceToHost, idx->stream));
      HIP_TRY(hipStreamSynchronize(idx->stream));
      r->n_carriers_kept = nc;
    }
    r->have_totals = true;
  }
  if (n_regions) *n_regions = r->d.Q;
  if (n_variants) *n_variants = r->n_variants;
  if (n_carriers) *n_carriers = r->n_carriers_kept;
  if (n_bases) *n_bases = r->n_bases;
  return VS_OK;
}

int vs_result_format_region(vs_result* r, uint64_t q, const char** text, uint64_t* len) {
  VS_TRY(result_enter(r, Want::Any, true));
  if (!text) return fail(VS_ERR_ARG, "null argument");
  if (r->kind == 2 || r->kind == 3) {  // `out << seq << std::endl`, query.h:182-187 / :252-257
    VS_TRY(fetch_sequences(r));
    if (q >= r->sq.Q) return fail(VS_ERR_ARG, "region %llu out of range", (unsigned long long)q);
    r->text.clear();
    if (!(r->h_flags[q] & (VS_REGION_INVALID | VS_REGION_ENDLESS))) {
      r->text.assign((const char*)r->h_chars.data() + r->h_byte_begin[q], r->h_byte_begin[q + 1] - r->h_byte_begin[q]);
      r->text += '\n';
    }
    *text = r->text.c_str();
    if (len) *len = r->text.size();
    return VS_OK;
  }
  if (r->kind == kKindGram)
    return fail(VS_ERR_UNSUPPORTED, "a Gram result holds one samples x samples matrix over the whole batch, no text per region (vs_result_get_sample_gram)");
  if (r->kind == kKindIbs)
    return fail(VS_ERR_UNSUPPORTED, "an IBS result holds samples x samples matrices over the whole batch, no text per region (vs_result_get_sample_ibs)");
  VS_TRY(fetch_region_meta(r));
  if (q >= r->d.Q) return fail(VS_ERR_ARG, "region %llu out of range", (unsigned long long)q);
  vs_index* idx = r->idx;
  const uint64_t a0 = r->h_var_begin[q], a1 = a0 + r->h_nvar[q];
  if (r->kind == kKindBurden) {   // the region's row of the matrix: the columns whose sample carries any counting row
    const size_t nc = r->h_cols.size();
    const uint4* c;
    if (r->cells_pin.p) c = (const uint4*)r->cells_pin.p + q * nc;
    else {
      VS_TRY(result_ready(r));
      VS_TRY(fetch(idx, r->sl_cells, (const uint4*)r->d_cells + q * nc, nc));
      HIP_TRY(hipStreamSynchronize(idx->stream));
      c = r->sl_cells.data();
    }
    std::string& out = r->text;
    out = "Sample\tVariants\tAC\tHomAlt\tPhased\n";
    for (size_t k = 0; k < nc; ++k) {
      if (!c[k].x) continue;
      const uint32_t id = r->h_cols[k];
      out += id < idx->g.sample_names.size() ? idx->g.sample_names[id] : std::string("?");
      for (uint32_t f : {c[k].x, c[k].y, c[k].z, c[k].w}) { out += '\t'; out += std::to_string(f); }
      out += '\n';
    }
    *text = out.c_str();
    if (len) *len = out.size();
    return VS_OK;
  }
  if (r->kind == kKindMatrix) {   // the region's reported rows, a genotype per column
    const size_t nc = r->h_cols.size(), pitch = (size_t)r->mx_pitch;
    const VariantRow* rows;
    if (r->have_headers) rows = r->h_rows.data() + a0;
    else if (r->raw_rows) rows = r->raw_rows + a0;
    else {
      VS_TRY(fetch(idx, r->sl_rows, (const VariantRow*)r->d.rows + a0, (size_t)(a1 - a0)));
      rows = r->sl_rows.data();
    }
    const uint8_t* c;
    if (r->cells_pin.p) c = (const uint8_t*)r->cells_pin.p + a0 * pitch;
    else {
      VS_TRY(result_ready(r));
      VS_TRY(fetch(idx, r->sl_matrix, (const uint8_t*)r->d_matrix + a0 * pitch, (size_t)(a1 - a0) * pitch));
      c = r->sl_matrix.data();
    }
    HIP_TRY(hipStreamSynchronize(idx->stream));
    std::string& out = r->text;
    out = "Pos\tRef\tAlt";
    for (size_t k = 0; k < nc; ++k) {
      const uint32_t id = r->h_cols[k];
      out += '\t';
      out += id < idx->g.sample_names.size() ? idx->g.sample_names[id] : std::string("?");
    }
    out += '\n';
    for (uint64_t a = a0; a < a1; ++a) {
      const VariantRow& v = rows[a - a0];
      if (v.count_flags & kRowDropped) continue;
      out += std::to_string(v.pos);
      out += '\t';
      out.append(idx->seq_chars, v.ref_off, v.ref_len);
      out += '\t';
      out.append(idx->seq_chars, v.alt_off, v.alt_len);
      const uint8_t* m = c + (a - a0) * pitch;
      for (size_t k = 0; k < nc; ++k) {
        out += '\t';
        const uint32_t gt = m[k];
        if (!gt) { out += '0'; continue; }
        out += (gt & GT_1) ? '1' : '0';   // the characters of print_var
        out += (gt & GT_PHASE) ? '|' : '/';
        out += (gt & GT_2) ? '1' : '0';
      }
      out += '\n';
    }
    *text = out.c_str();
    if (len) *len = out.size();
    return VS_OK;
  }
  if (r->kind == kKindLd) {   // the pairs a < b of the region's reported rows whose table indices are at most the window apart
    const uint64_t W = r->ld_window;
    const VariantRow* rows;
    if (r->have_headers) rows = r->h_rows.data() + a0;
    else if (r->raw_rows) rows = r->raw_rows + a0;
    else {
      VS_TRY(fetch(idx, r->sl_rows, (const VariantRow*)r->d.rows + a0, (size_t)(a1 - a0)));
      rows = r->sl_rows.data();
    }
    const uint32_t* b;
    if (r->cells_pin.p) b = (const uint32_t*)r->cells_pin.p + a0 * W;
    else {
      VS_TRY(result_ready(r));
      VS_TRY(fetch(idx, r->sl_band, (const uint32_t*)r->d_band + a0 * W, (size_t)((a1 - a0) * W)));
      b = r->sl_band.data();
    }
    HIP_TRY(hipStreamSynchronize(idx->stream));
    std::string& out = r->text;
    out = "PosA\tRefA\tAltA\tPosB\tRefB\tAltB\t";
    out += r->ld_stat == VS_LD_R2 ? "R2\n" : "Dot\n";
    auto site = [&](const VariantRow& v) {
      out += std::to_string(v.pos);
      out += '\t';
      out.append(idx->seq_chars, v.ref_off, v.ref_len);
      out += '\t';
      out.append(idx->seq_chars, v.alt_off, v.alt_len);
      out += '\t';
    };
    char num[48];
    for (uint64_t a = a0; a < a1; ++a) {
      if (rows[a - a0].count_flags & kRowDropped) continue;
      for (uint64_t k = 0; k < W && a + 1 + k < a1; ++k) {
        if (rows[a + 1 + k - a0].count_flags & kRowDropped) continue;
        site(rows[a - a0]);
        site(rows[a + 1 + k - a0]);
        const uint32_t cell = b[(a - a0) * W + k];
        if (r->ld_stat == VS_LD_R2) {
          float f;
          memcpy(&f, &cell, 4);
          snprintf(num, sizeof num, "%.6g\n", (double)f);
        } else snprintf(num, sizeof num, "%d\n", (int)cell);
        out += num;
      }
    }
    *text = out.c_str();
    if (len) *len = out.size();
    return VS_OK;
  }
  if (r->kind == kKindTrio) {   // the region's reported rows with their alternate-allele count over the members and their four sums over the trios
    const VariantRow* rows;
    if (r->have_headers) rows = r->h_rows.data() + a0;
    else if (r->raw_rows) rows = r->raw_rows + a0;
    else {
      VS_TRY(fetch(idx, r->sl_rows, (const VariantRow*)r->d.rows + a0, (size_t)(a1 - a0)));
      rows = r->sl_rows.data();
    }
    VS_TRY(array_to_host(r, r->d_trio, r->trio_bytes, &r->cells_pin, "trio records"));
    VS_TRY(counts_to_host(r));
    HIP_TRY(hipStreamSynchronize(idx->stream));
    const vs_trio_counts* rec = (const vs_trio_counts*)r->cells_pin.p + a0;
    const uint4* cnt = (const uint4*)r->counts_pin.p + a0;
    std::string& out = r->text;
    out = "Pos\tRef\tAlt\tAC\tErrors\tDeNovo\tT\tU\n";
    for (uint64_t a = a0; a < a1; ++a) {
      const VariantRow& v = rows[a - a0];
      if (v.count_flags & kRowDropped) continue;
      out += std::to_string(v.pos);
      out += '\t';
      out.append(idx->seq_chars, v.ref_off, v.ref_len);
      out += '\t';
      out.append(idx->seq_chars, v.alt_off, v.alt_len);
      const vs_trio_counts& t = rec[a - a0];
      for (uint32_t f : {cnt[a - a0].y, t.errors, t.denovo, t.transmitted, t.untransmitted}) { out += '\t'; out += std::to_string(f); }
      out += '\n';
    }
    *text = out.c_str();
    if (len) *len = out.size();
    return VS_OK;
  }
  if (r->kind == kKindRoh) {   // the region's segments, a line each, in column order: integers only (KB from bp with three fixed decimals)
    if (!r->roh.segments) return fail(VS_ERR_ARG, "the ROH batch was run without segments (vs_roh_params::segments): its summaries are vs_result_get_roh's");
    VS_TRY(array_to_host(r, r->d_roh, r->roh_bytes, &r->cells_pin, "ROH summaries"));
    VS_TRY(array_to_host(r, r->d_roh_seg, (size_t)r->roh_segs * 32, &r->owner_pin, "ROH segments"));
    const size_t nc = r->h_cols.size();
    const uint64_t* sb = (const uint64_t*)((const uint8_t*)r->cells_pin.p + r->roh_begin_off) + q * nc;
    const vs_roh_segment* seg = (const vs_roh_segment*)r->owner_pin.p;
    std::string& out = r->text;
    out = "Sample\tPos1\tPos2\tKB\tNSites\tNHet\n";
    char kb[40];
    for (uint64_t s = sb[0]; s < sb[nc]; ++s) {
      const vs_roh_segment& g = seg[s];
      const uint32_t id = r->h_cols[g.column];
      const uint64_t bp = (uint64_t)(g.pos_last > g.pos_first ? g.pos_last - g.pos_first : 0u) + 1u;
      snprintf(kb, sizeof kb, "%llu.%03u", (unsigned long long)(bp / 1000), (unsigned)(bp % 1000));
      out += id < idx->g.sample_names.size() ? idx->g.sample_names[id] : std::string("?");
      for (uint32_t f : {g.pos_first, g.pos_last}) { out += '\t'; out += std::to_string(f); }
      out += '\t'; out += kb;
      for (uint32_t f : {g.n_sites, g.n_het}) { out += '\t'; out += std::to_string(f); }
      out += '\n';
    }
    *text = out.c_str();
    if (len) *len = out.size();
    return VS_OK;
  }
  if (r->kind == kKindPrune) {   // the region's reported rows with their verdicts
    const VariantRow* rows;
    if (r->have_headers) rows = r->h_rows.data() + a0;
    else if (r->raw_rows) rows = r->raw_rows + a0;
    else {
      VS_TRY(fetch(idx, r->sl_rows, (const VariantRow*)r->d.rows + a0, (size_t)(a1 - a0)));
      rows = r->sl_rows.data();
    }
    VS_TRY(array_to_host(r, r->d_state, (size_t)r->prune_states, &r->cells_pin, "pruning verdicts"));
    VS_TRY(counts_to_host(r));
    VS_TRY(prune_meta_to_host(r));
    HIP_TRY(hipStreamSynchronize(idx->stream));
    const uint8_t* st = (const uint8_t*)r->cells_pin.p + r->h_prune_meta[q];
    const uint4* cnt = (const uint4*)r->counts_pin.p + a0;
    std::string& out = r->text;
    out = "Pos\tRef\tAlt\tAC\tState\n";
    for (uint64_t a = a0; a < a1; ++a) {
      const VariantRow& v = rows[a - a0];
      if (v.count_flags & kRowDropped) continue;
      out += std::to_string(v.pos);
      out += '\t';
      out.append(idx->seq_chars, v.ref_off, v.ref_len);
      out += '\t';
      out.append(idx->seq_chars, v.alt_off, v.alt_len);
      out += '\t';
      out += std::to_string(cnt[a - a0].y);
      const uint8_t verdict = st[a - a0];
      out += verdict == kPruneKept ? "\tkeep\n" : verdict == kPrunePruned ? "\tpruned\n" : "\tskip\n";
    }
    *text = out.c_str();
    if (len) *len = out.size();
    return VS_OK;
  }
  if (r->kind == kKindLdScore) {   // the region's reported rows with their pair counts and scores
    const VariantRow* rows;
    if (r->have_headers) rows = r->h_rows.data() + a0;
    else if (r->raw_rows) rows = r->raw_rows + a0;
    else {
      VS_TRY(fetch(idx, r->sl_rows, (const VariantRow*)r->d.rows + a0, (size_t)(a1 - a0)));
      rows = r->sl_rows.data();
    }
    VS_TRY(array_to_host(r, r->d_ldscore, (size_t)r->prune_states * 13, &r->cells_pin, "LD scores"));
    VS_TRY(counts_to_host(r));
    VS_TRY(prune_meta_to_host(r));
    HIP_TRY(hipStreamSynchronize(idx->stream));
    const uint8_t* base = (const uint8_t*)r->cells_pin.p;
    const uint64_t kb = r->h_prune_meta[q];
    const uint64_t* sums = (const uint64_t*)base + kb;
    const uint32_t* pairs = (const uint32_t*)(base + 8 * r->prune_states) + kb;
    const uint8_t* st = base + 12 * r->prune_states + kb;
    const uint4* cnt = (const uint4*)r->counts_pin.p + a0;
    std::string& out = r->text;
    out = "Pos\tRef\tAlt\tAC\tPairs\tL2\tState\n";
    char num[64];
    for (uint64_t a = a0; a < a1; ++a) {
      const VariantRow& v = rows[a - a0];
      if (v.count_flags & kRowDropped) continue;
      out += std::to_string(v.pos);
      out += '\t';
      out.append(idx->seq_chars, v.ref_off, v.ref_len);
      out += '\t';
      out.append(idx->seq_chars, v.alt_off, v.alt_len);
      out += '\t';
      out += std::to_string(cnt[a - a0].y);
      out += '\t';
      out += std::to_string(pairs[a - a0]);
      snprintf(num, sizeof num, "\t%.6f", (double)sums[a - a0] / 4294967296.0);
      out += num;
      out += st[a - a0] == kLdScoreScored ? "\tscored\n" : "\tskip\n";
    }
    *text = out.c_str();
    if (len) *len = out.size();
    return VS_OK;
  }
  if (r->kind == kKindClump) {   // the region's reported rows with their p-values, verdicts and index rows
    const VariantRow* rows;
    if (r->have_headers) rows = r->h_rows.data() + a0;
    else if (r->raw_rows) rows = r->raw_rows + a0;
    else {
      VS_TRY(fetch(idx, r->sl_rows, (const VariantRow*)r->d.rows + a0, (size_t)(a1 - a0)));
      rows = r->sl_rows.data();
    }
    VS_TRY(array_to_host(r, r->d_state, (size_t)r->prune_states, &r->cells_pin, "clumping verdicts"));
    VS_TRY(array_to_host(r, r->d_owner, (size_t)r->prune_states * 4, &r->owner_pin, "clump owners"));
    VS_TRY(counts_to_host(r));
    VS_TRY(prune_meta_to_host(r));
    HIP_TRY(hipStreamSynchronize(idx->stream));
    const uint8_t* st = (const uint8_t*)r->cells_pin.p + r->h_prune_meta[q];
    const uint32_t* own = (const uint32_t*)r->owner_pin.p + r->h_prune_meta[q];
    const uint4* cnt = (const uint4*)r->counts_pin.p + a0;
    const auto name = [&](std::string& out, const VariantRow& v, char sep) {
      out += std::to_string(v.pos);
      out += sep;
      out.append(idx->seq_chars, v.ref_off, v.ref_len);
      out += sep;
      out.append(idx->seq_chars, v.alt_off, v.alt_len);
    };
    std::string& out = r->text;
    out = "Pos\tRef\tAlt\tAC\tP\tState\tIndex\n";
    char num[40];
    for (uint64_t a = a0; a < a1; ++a) {
      const VariantRow& v = rows[a - a0];
      if (v.count_flags & kRowDropped) continue;
      name(out, v, '\t');
      out += '\t';
      out += std::to_string(cnt[a - a0].y);
      out += '\t';
      const uint64_t key = r->h_clump_keys[a];
      if (key == kClumpNoKey) out += '.';
      else {
        double p;
        memcpy(&p, &key, 8);
        snprintf(num, sizeof num, "%.6g", p);
        out += num;
      }
      const uint8_t verdict = st[a - a0];
      out += verdict == kClumpIndex ? "\tindex\t" : verdict == kClumpMember ? "\tclumped\t" : verdict == kClumpUnclumped ? "\tunclumped\t" : "\tskip\t";
      const uint32_t o = own[a - a0];
      if (o == kClumpNoOwner || o >= a1 - a0) out += '.';
      else name(out, rows[o], ':');
      out += '\n';
    }
    *text = out.c_str();
    if (len) *len = out.size();
    return VS_OK;
  }
  if (r->kind == kKindLdMatrix) {   // the region's block without the rows and columns of dropped rows, a header of the rows' names
    const uint64_t m = a1 - a0;
    const VariantRow* rows;
    if (r->have_headers) rows = r->h_rows.data() + a0;
    else if (r->raw_rows) rows = r->raw_rows + a0;
    else {
      VS_TRY(fetch(idx, r->sl_rows, (const VariantRow*)r->d.rows + a0, (size_t)m));
      rows = r->sl_rows.data();
    }
    VS_TRY(ld_block_begin_to_host(r));
    const uint32_t* b;
    if (r->cells_pin.p) b = (const uint32_t*)r->cells_pin.p + r->h_block_begin[q];
    else {
      VS_TRY(result_ready(r));
      VS_TRY(fetch(idx, r->sl_band, (const uint32_t*)r->d_ldm + r->h_block_begin[q], (size_t)(m * m)));
      b = r->sl_band.data();
    }
    HIP_TRY(hipStreamSynchronize(idx->stream));
    std::string& out = r->text;
    out = "Pos\tRef\tAlt";
    for (uint64_t k = 0; k < m; ++k) {
      const VariantRow& v = rows[k];
      if (v.count_flags & kRowDropped) continue;
      out += '\t';
      out += std::to_string(v.pos);
      out += ':';
      out.append(idx->seq_chars, v.ref_off, v.ref_len);
      out += ':';
      out.append(idx->seq_chars, v.alt_off, v.alt_len);
    }
    out += '\n';
    char num[48];
    for (uint64_t x = 0; x < m; ++x) {
      const VariantRow& v = rows[x];
      if (v.count_flags & kRowDropped) continue;
      out += std::to_string(v.pos);
      out += '\t';
      out.append(idx->seq_chars, v.ref_off, v.ref_len);
      out += '\t';
      out.append(idx->seq_chars, v.alt_off, v.alt_len);
      for (uint64_t y = 0; y < m; ++y) {
        if (rows[y].count_flags & kRowDropped) continue;
        const uint32_t cell = b[x * m + y];
        if (r->ld_stat == VS_LD_R2) {
          float f;
          memcpy(&f, &cell, 4);
          snprintf(num, sizeof num, "\t%.6g", (double)f);
        } else snprintf(num, sizeof num, "\t%d", (int)cell);
        out += num;
      }
      out += '\n';
    }
    *text = out.c_str();
    if (len) *len = out.size();
    return VS_OK;
  }
  if (r->kind == kKindWindowStats) {   // the region's records, a line per group, then a line per pair: integers only
    VS_TRY(array_to_host(r, r->d_wstats, window_stats_bytes(r), &r->cells_pin, "window statistics"));
    const uint32_t G = r->n_groups, P = r->ws_pairs;
    const vs_window_stats* w = (const vs_window_stats*)r->cells_pin.p + q * G;
    const vs_window_pair_stats* wp = (const vs_window_pair_stats*)((const uint8_t*)r->cells_pin.p + (size_t)r->d.Q * 48 * G) + q * P;
    auto name = [&](uint32_t g) { return r->group_names.empty() ? std::to_string(g) : r->group_names[g]; };
    std::string& out = r->text;
    out = "Group\tN\tRows\tSeg\tSingletons\tDoubletons\tPrivate\tFixed\tSumAC\tSumAC2\tObsHet\n";
    for (uint32_t g = 0; g < G; ++g) {
      out += name(g);
      for (uint64_t f : {(uint64_t)r->group_sizes[g], (uint64_t)w[g].rows, (uint64_t)w[g].seg, (uint64_t)w[g].singletons, (uint64_t)w[g].doubletons,
                         (uint64_t)w[g].private_alleles, (uint64_t)w[g].fixed, w[g].sum_ac, w[g].sum_ac2, w[g].obs_het}) {
        out += '\t';
        out += std::to_string(f);
      }
      out += '\n';
    }
    if (P) {
      out += "GroupA\tGroupB\tSumCross\tSegUnion\tFixedDiff\n";
      uint32_t p = 0;
      for (uint32_t g = 0; g < G; ++g)
        for (uint32_t h = g + 1; h < G; ++h, ++p) {
          out += name(g);
          out += '\t';
          out += name(h);
          for (uint64_t f : {wp[p].sum_cross, (uint64_t)wp[p].seg_union, (uint64_t)wp[p].fixed_diff}) { out += '\t'; out += std::to_string(f); }
          out += '\n';
        }
    }
    *text = out.c_str();
    if (len) *len = out.size();
    return VS_OK;
  }
  if (r->kind == kKindGroups) {   // the region's reported rows, a line per row and group
    VS_TRY(counts_to_host(r));
    const VariantRow* rows;
    if (r->have_headers) rows = r->h_rows.data() + a0;
    else if (r->raw_rows) rows = r->raw_rows + a0;
    else {
      VS_TRY(fetch(idx, r->sl_rows, (const VariantRow*)r->d.rows + a0, (size_t)(a1 - a0)));
      HIP_TRY(hipStreamSynchronize(idx->stream));
      rows = r->sl_rows.data();
    }
    const uint4* c = (const uint4*)r->counts_pin.p;
    const uint32_t G = r->n_groups;
    std::string& out = r->text;
    out = "Pos\tRef\tAlt\tGroup\tN\tCarriers\tAC\tHomAlt\tPhased\n";
    std::string head;
    for (uint64_t a = a0; a < a1; ++a) {
      const VariantRow& v = rows[a - a0];
      if (v.count_flags & kRowDropped) continue;
      head = std::to_string(v.pos);
      head += '\t';
      head.append(idx->seq_chars, v.ref_off, v.ref_len);
      head += '\t';
      head.append(idx->seq_chars, v.alt_off, v.alt_len);
      head += '\t';
      for (uint32_t g = 0; g < G; ++g) {
        const uint4 k = c[a * G + g];
        out += head;
        out += r->group_names.empty() ? std::to_string(g) : r->group_names[g];
        for (uint32_t f : {r->group_sizes[g], k.x, k.y, k.z, k.w}) { out += '\t'; out += std::to_string(f); }
        out += '\n';
      }
    }
    *text = out.c_str();
    if (len) *len = out.size();
    return VS_OK;
  }
  if (r->kind == kKindAssoc || r->kind == kKindAssocMatrix) {   // the region's reported rows: the count text's columns, then the K cells
    VS_TRY(array_to_host(r, r->d_scores, (size_t)(r->d.A * r->n_traits) * sizeof(double), &r->cells_pin, "association scores"));
    VS_TRY(counts_to_host(r));
    const VariantRow* rows;
    if (r->have_headers) rows = r->h_rows.data() + a0;
    else if (r->raw_rows) rows = r->raw_rows + a0;
    else {
      VS_TRY(fetch(idx, r->sl_rows, (const VariantRow*)r->d.rows + a0, (size_t)(a1 - a0)));
      HIP_TRY(hipStreamSynchronize(idx->stream));
      rows = r->sl_rows.data();
    }
    const uint4* c = (const uint4*)r->counts_pin.p;
    const double* sc = (const double*)r->cells_pin.p;
    const uint32_t K = r->n_traits;
    std::string& out = r->text;
    out = "Pos\tRef\tAlt\tCarriers\tAC\tHomAlt\tPhased";
    for (uint32_t k = 0; k < K; ++k) { out += '\t'; out += r->trait_names.empty() ? std::to_string(k) : r->trait_names[k]; }
    out += '\n';
    char num[48];
    for (uint64_t a = a0; a < a1; ++a) {
      const VariantRow& v = rows[a - a0];
      if (v.count_flags & kRowDropped) continue;
      out += std::to_string(v.pos);
      out += '\t';
      out.append(idx->seq_chars, v.ref_off, v.ref_len);
      out += '\t';
      out.append(idx->seq_chars, v.alt_off, v.alt_len);
      for (uint32_t f : {c[a].x, c[a].y, c[a].z, c[a].w}) { out += '\t'; out += std::to_string(f); }
      for (uint32_t k = 0; k < K; ++k) { snprintf(num, sizeof num, "\t%.17g", sc[a * K + k]); out += num; }
      out += '\n';
    }
    *text = out.c_str();
    if (len) *len = out.size();
    return VS_OK;
  }
  if (r->kind == kKindScores || r->kind == kKindScoreMatrix) {   // the region's reported rows -- the rows the weights are keyed by, in report order
    const VariantRow* rows;
    if (r->have_headers) rows = r->h_rows.data() + a0;
    else if (r->raw_rows) rows = r->raw_rows + a0;
    else {
      VS_TRY(fetch(idx, r->sl_rows, (const VariantRow*)r->d.rows + a0, (size_t)(a1 - a0)));
      HIP_TRY(hipStreamSynchronize(idx->stream));
      rows = r->sl_rows.data();
    }
    std::string& out = r->text;
    out = "Pos\tRef\tAlt\n";
    for (uint64_t a = a0; a < a1; ++a) {
      const VariantRow& v = rows[a - a0];
      if (v.count_flags & kRowDropped) continue;
      out += std::to_string(v.pos);
      out += '\t';
      out.append(idx->seq_chars, v.ref_off, v.ref_len);
      out += '\t';
      out.append(idx->seq_chars, v.alt_off, v.alt_len);
      out += '\n';
    }
    *text = out.c_str();
    if (len) *len = out.size();
    return VS_OK;
  }
  if (r->kind == kKindCounts) {   // the region's reported rows with their counts
    VS_TRY(counts_to_host(r));
    const VariantRow* rows;
    if (r->have_headers) rows = r->h_rows.data() + a0;
    else if (r->raw_rows) rows = r->raw_rows + a0;
    else {
      VS_TRY(fetch(idx, r->sl_rows, (const VariantRow*)r->d.rows + a0, (size_t)(a1 - a0)));
      HIP_TRY(hipStreamSynchronize(idx->stream));
      rows = r->sl_rows.data();
    }
    const uint4* c = (const uint4*)r->counts_pin.p;
    std::string& out = r->text;
    out = "Pos\tRef\tAlt\tCarriers\tAC\tHomAlt\tPhased\n";
    for (uint64_t a = a0; a < a1; ++a) {
      const VariantRow& v = rows[a - a0];
      if (v.count_flags & kRowDropped) continue;
      out += std::to_string(v.pos);
      out += '\t';
      out.append(idx->seq_chars, v.ref_off, v.ref_len);
      out += '\t';
      out.append(idx->seq_chars, v.alt_off, v.alt_len);
      for (uint32_t f : {c[a].x, c[a].y, c[a].z, c[a].w}) { out += '\t'; out += std::to_string(f); }
      out += '\n';
    }
    *text = out.c_str();
    if (len) *len = out.size();
    return VS_OK;
  }
  const uint64_t c0 = r->h_car_base[q], c1 = c0 + r->h_car_len[q];
  const uint32_t* car = nullptr;
  const bool from_view = r->have_carriers;
  if (!from_view && r->scattered_lists && !(r->raw_rows && r->raw_arena)) {   // lists all over the arena: bring it over once
    VS_TRY(raw_copy_begin(r, true, idx->stream));
    HIP_TRY(hipStreamSynchronize(idx->stream));
  }
  const bool from_raw = !from_view && r->raw_rows && r->raw_arena;   // a raw copy holds rows and arena: nothing to fetch
  // the rows: the whole table when a view or a raw copy has already brought it over, otherwise this region's slice of it
  const VariantRow* rows;
  if (r->have_headers) rows = r->h_rows.data() + a0;
  else if (r->raw_rows) rows = r->raw_rows + a0;
  else {
    VS_TRY(fetch(idx, r->sl_rows, (const VariantRow*)r->d.rows + a0, (size_t)(a1 - a0)));
    HIP_TRY(hipStreamSynchronize(idx->stream));   // the rows are read below whether or not any carrier is fetched
    rows = r->sl_rows.data();
  }
  const uint64_t vbase = r->have_headers ? r->h_view_begin[q] : 0;   // slot of the region's first row in the view
  if (!from_view && !from_raw) {
    VS_TRY(fetch_carriers(r, c0, c1 - c0, r->slice_carriers));
    car = r->slice_carriers.data();
  }
  const uint16_t* raw16 = reinterpret_cast<const uint16_t*>(r->raw_arena);
  const uint32_t* raw32 = reinterpret_cast<const uint32_t*>(r->raw_arena);
  const bool narrow = r->d.car_width == 2;
  // carrier k of row v as id | gt << 29, from whichever host copy there is
  auto carrier = [&](const VariantRow& v, uint64_t slot, uint32_t k) -> uint32_t {
    if (from_view) return r->h_carriers[r->h_car_begin_view[slot] + k];
    if (from_raw) {
      if (!narrow) return raw32[v.car_begin + k];
      const uint32_t c = raw16[v.car_begin + k];
      return (c & 0x1FFFu) | ((c >> 13) << 29);
    }
    return car[(v.car_begin - c0) + k];
  };
  std::string& out = r->text;
  out.clear();
  if (r->kind == 7) {  // samples_has_var's output line, query.h:811-816: `name gt` pairs with nothing between them
    for (uint64_t a = a0; a < a1; ++a) {
      const VariantRow& v = rows[a - a0];
      if (v.count_flags & kRowDropped) continue;
      for (uint32_t k = 0; k < v.count_flags; ++k) {
        const uint32_t cw = carrier(v, vbase + (a - a0), k);
        const uint32_t id = VS_CARRIER_ID(cw), gt = VS_CARRIER_GT(cw);
        out += id < idx->g.sample_names.size() ? idx->g.sample_names[id] : std::string("?");
        out += ' ';
        out += (gt & GT_1) ? '1' : '0';
        out += (gt & GT_PHASE) ? '|' : '/';
        out += (gt & GT_2) ? '1' : '0';
      }
      out += '\n';
    }
    *text = out.c_str();
    if (len) *len = out.size();
    return VS_OK;
  }
  if (r->h_flags[q] & VS_REGION_NOT_FOUND) {  // closest_var returned false: the reference writes no file
    *text = out.c_str();
    if (len) *len = 0;
    return VS_OK;
  }
  out += "Pos\tRef\tAlt\tSamples\n";  // print_header, query.h:38-41
  for (uint64_t a = a0; a < a1; ++a) {
    const VariantRow& v = rows[a - a0];
    if (v.count_flags & kRowDropped) continue;
    out += std::to_string(v.pos);  // print_var, query.h:43-50
    out += '\t';
    out.append(idx->seq_chars, v.ref_off, v.ref_len);
    out += '\t';
    out.append(idx->seq_chars, v.alt_off, v.alt_len);
    out += '\t';
    for (uint32_t k = 0; k < v.count_flags; ++k) {
      const uint32_t cw = carrier(v, vbase + (a - a0), k);
      const uint32_t id = VS_CARRIER_ID(cw), gt = VS_CARRIER_GT(cw);
      out += id < idx->g.sample_names.size() ? idx->g.sample_names[id] : std::string("?");
      out += '(';
      out += (gt & GT_1) ? '1' : '0';   // get_sample_phasing, variant_graph.h:882-900
      out += (gt & GT_PHASE) ? '|' : '/';
      out += (gt & GT_2) ? '1' : '0';
      out += ") ";
    }
    out += '\n';
  }
  *text = out.c_str();
  if (len) *len = out.size();
  return VS_OK;
}

/* Duration of the result's carrier expansion by HIP events on the stream it ran on, when it ran asynchronously (option
 * "async_fill"; waits for it); -1 otherwise (vs_index_last_timing().ms_fill has it then). */
int vs_result_get_allele_counts(vs_result* r, uint64_t* n_rows, const vs_allele_counts** counts) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!counts) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindCounts) return fail(VS_ERR_ARG, "not an allele-count result (vs_query_allele_counts)");
  static_assert(sizeof(vs_allele_counts) == sizeof(uint4), "count layout of the ABI");
  VS_TRY(counts_to_host(r));
  *counts = (const vs_allele_counts*)r->counts_pin.p;
  if (n_rows) *n_rows = r->d.A;
  return VS_OK;
}

int vs_result_get_group_counts(vs_result* r, uint64_t* n_rows, uint32_t* n_groups, const uint32_t** group_sizes, const vs_allele_counts** counts) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!counts) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindGroups) return fail(VS_ERR_ARG, "not a grouped-count result (vs_query_group_counts)");
  VS_TRY(counts_to_host(r));
  *counts = (const vs_allele_counts*)r->counts_pin.p;
  if (n_rows) *n_rows = r->d.A;
  if (n_groups) *n_groups = r->n_groups;
  if (group_sizes) *group_sizes = r->group_sizes.data();
  return VS_OK;
}

int vs_result_get_assoc_scan(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* n_traits, uint32_t* stat, const uint32_t** col_ids, const double** trait_sum,
                             const double** trait_sumsq, const vs_allele_counts** counts, const double** scores) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!scores) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindAssoc) return fail(VS_ERR_ARG, "not an association-scan result (vs_query_assoc_scan)");
  VS_TRY(array_to_host(r, r->d_scores, (size_t)(r->d.A * r->n_traits) * sizeof(double), &r->cells_pin, "association scores"));
  VS_TRY(counts_to_host(r));
  *scores = (const double*)r->cells_pin.p;
  if (counts) *counts = (const vs_allele_counts*)r->counts_pin.p;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  if (n_traits) *n_traits = r->n_traits;
  if (stat) *stat = r->assoc_stat;
  if (col_ids) *col_ids = r->h_cols.data();
  if (trait_sum) *trait_sum = r->trait_sum.data();
  if (trait_sumsq) *trait_sumsq = r->trait_sumsq.data();
  return VS_OK;
}

int vs_result_get_assoc_matrix(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* n_traits, uint32_t* stat, const uint32_t** col_ids, const int32_t** shift,
                               const double** trait_sum, const double** trait_sumsq, const vs_allele_counts** counts, const double** scores) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!scores) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindAssocMatrix) return fail(VS_ERR_ARG, "not a trait-matrix association result (vs_query_assoc_matrix)");
  VS_TRY(array_to_host(r, r->d_scores, (size_t)(r->d.A * r->n_traits) * sizeof(double), &r->cells_pin, "association scores"));
  VS_TRY(counts_to_host(r));
  *scores = (const double*)r->cells_pin.p;
  if (counts) *counts = (const vs_allele_counts*)r->counts_pin.p;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  if (n_traits) *n_traits = r->n_traits;
  if (stat) *stat = r->assoc_stat;
  if (col_ids) *col_ids = r->h_cols.data();
  if (shift) *shift = r->trait_shift.data();
  if (trait_sum) *trait_sum = r->trait_sum.data();
  if (trait_sumsq) *trait_sumsq = r->trait_sumsq.data();
  return VS_OK;
}

int vs_result_get_sample_scores(vs_result* r, uint64_t* n_cols, uint32_t* n_scores, const uint32_t** col_ids, const int32_t** shift, const int64_t** sums,
                                const double** scores) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!sums && !scores) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindScores) return fail(VS_ERR_ARG, "not a per-sample score result (vs_query_sample_scores)");
  const size_t cells = r->h_cols.size() * r->n_scores;
  VS_TRY(array_to_host(r, r->d_sums, cells * 16, &r->cells_pin, "per-sample scores"));
  if (sums) *sums = (const int64_t*)r->cells_pin.p;
  if (scores) *scores = (const double*)((const int64_t*)r->cells_pin.p + cells);
  if (n_cols) *n_cols = r->h_cols.size();
  if (n_scores) *n_scores = r->n_scores;
  if (col_ids) *col_ids = r->h_cols.data();
  if (shift) *shift = r->score_shift.data();
  return VS_OK;
}

int vs_result_get_score_matrix(vs_result* r, uint64_t* n_cols, uint32_t* n_scores, const uint32_t** col_ids, const int32_t** shift, uint32_t* limbs,
                               const int64_t** sums, const double** scores) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!sums && !scores) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindScoreMatrix) return fail(VS_ERR_ARG, "not a score-matrix result (vs_query_score_matrix)");
  const size_t cells = r->h_cols.size() * r->n_scores;
  VS_TRY(array_to_host(r, r->d_sums, cells * 16, &r->cells_pin, "score matrix"));
  if (sums) *sums = (const int64_t*)r->cells_pin.p;
  if (scores) *scores = (const double*)((const int64_t*)r->cells_pin.p + cells);
  if (n_cols) *n_cols = r->h_cols.size();
  if (n_scores) *n_scores = r->n_scores;
  if (col_ids) *col_ids = r->h_cols.data();
  if (shift) *shift = r->score_shift.data();
  if (limbs) *limbs = r->sm_limbs;
  return VS_OK;
}

int vs_result_get_sample_burden(vs_result* r, uint64_t* n_regions, uint64_t* n_cols, const uint32_t** col_ids, const vs_sample_burden** cells) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!cells) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindBurden) return fail(VS_ERR_ARG, "not a burden result (vs_query_sample_burden)");
  static_assert(sizeof(vs_sample_burden) == sizeof(uint4), "cell layout of the ABI");
  VS_TRY(array_to_host(r, r->d_cells, (size_t)r->d.Q * r->h_cols.size() * sizeof(uint4), &r->cells_pin, "burden matrix"));
  *cells = (const vs_sample_burden*)r->cells_pin.p;
  if (n_regions) *n_regions = r->d.Q;
  if (n_cols) *n_cols = r->h_cols.size();
  if (col_ids) *col_ids = r->h_cols.data();
  return VS_OK;
}

// The *_device accessors: the gate, a result of `kind` (else the text `not_kind`), and the matrix complete when its pointer is
// handed out -- the caller needs no event.
static int device_matrix_ready(vs_result* r, const void* out, int kind, const char* not_kind) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!out) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kind) return fail(VS_ERR_ARG, "%s", not_kind);
  VS_TRY(result_ready(r));
  HIP_TRY(hipStreamSynchronize(r->idx->stream));
  return VS_OK;
}

int vs_result_sample_burden_device(vs_result* r, uint64_t* n_regions, uint64_t* n_cols, const void** dev_cells) {
  VS_TRY(device_matrix_ready(r, dev_cells, kKindBurden, "not a burden result (vs_query_sample_burden)"));
  *dev_cells = r->d_cells;
  if (n_regions) *n_regions = r->d.Q;
  if (n_cols) *n_cols = r->h_cols.size();
  return VS_OK;
}

int vs_result_group_counts_device(vs_result* r, uint64_t* n_rows, uint32_t* n_groups, const void** dev_counts) {
  VS_TRY(device_matrix_ready(r, dev_counts, kKindGroups, "not a grouped-count result (vs_query_group_counts)"));
  *dev_counts = r->d_counts;
  if (n_rows) *n_rows = r->d.A;
  if (n_groups) *n_groups = r->n_groups;
  return VS_OK;
}

int vs_result_get_window_stats(vs_result* r, uint64_t* n_regions, uint32_t* n_groups, uint32_t* n_pairs, const uint32_t** group_sizes, const char* const** group_names,
                               const vs_window_stats** stats, const vs_window_pair_stats** pair_stats) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!stats) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindWindowStats) return fail(VS_ERR_ARG, "not a window-statistics result (vs_query_window_stats)");
  static_assert(sizeof(vs_window_stats) == 48 && sizeof(vs_window_pair_stats) == 16, "record layout of the ABI");
  VS_TRY(array_to_host(r, r->d_wstats, window_stats_bytes(r), &r->cells_pin, "window statistics"));
  if (r->ws_name_ptrs.empty())
    for (const std::string& s : r->group_names) r->ws_name_ptrs.push_back(s.c_str());
  *stats = (const vs_window_stats*)r->cells_pin.p;
  if (pair_stats) *pair_stats = r->ws_pairs ? (const vs_window_pair_stats*)((const uint8_t*)r->cells_pin.p + (size_t)r->d.Q * 48 * r->n_groups) : nullptr;
  if (n_regions) *n_regions = r->d.Q;
  if (n_groups) *n_groups = r->n_groups;
  if (n_pairs) *n_pairs = r->ws_pairs;
  if (group_sizes) *group_sizes = r->group_sizes.data();
  if (group_names) *group_names = r->ws_name_ptrs.empty() ? nullptr : r->ws_name_ptrs.data();
  return VS_OK;
}

int vs_result_window_stats_device(vs_result* r, uint64_t* n_regions, uint32_t* n_groups, uint32_t* n_pairs, const void** dev_stats, const void** dev_pair_stats) {
  VS_TRY(device_matrix_ready(r, dev_stats, kKindWindowStats, "not a window-statistics result (vs_query_window_stats)"));
  *dev_stats = r->d_wstats;
  if (dev_pair_stats) *dev_pair_stats = r->ws_pairs ? r->d_wstats + (size_t)r->d.Q * 48 * r->n_groups : nullptr;
  if (n_regions) *n_regions = r->d.Q;
  if (n_groups) *n_groups = r->n_groups;
  if (n_pairs) *n_pairs = r->ws_pairs;
  return VS_OK;
}

int vs_result_get_genotype_matrix(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint64_t* row_pitch, const uint32_t** col_ids, const uint8_t** cells) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!cells) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindMatrix) return fail(VS_ERR_ARG, "not a genotype-matrix result (vs_query_genotype_matrix)");
  VS_TRY(array_to_host(r, r->d_matrix, (size_t)(r->d.A * r->mx_pitch), &r->cells_pin, "genotype matrix"));   // (pitch and all)
  *cells = (const uint8_t*)r->cells_pin.p;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  if (row_pitch) *row_pitch = r->mx_pitch;
  if (col_ids) *col_ids = r->h_cols.data();
  return VS_OK;
}

int vs_result_genotype_matrix_device(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint64_t* row_pitch, const void** dev_cells) {
  VS_TRY(device_matrix_ready(r, dev_cells, kKindMatrix, "not a genotype-matrix result (vs_query_genotype_matrix)"));
  *dev_cells = r->d_matrix;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  if (row_pitch) *row_pitch = r->mx_pitch;
  return VS_OK;
}

int vs_result_get_ld_band(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* window, uint32_t* stat, const uint32_t** col_ids,
                          const vs_allele_counts** counts, const void** band) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!band) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindLd) return fail(VS_ERR_ARG, "not an LD result (vs_query_ld_band)");
  VS_TRY(array_to_host(r, r->d_band, (size_t)(r->d.A * r->ld_window) * 4, &r->cells_pin, "LD band"));
  VS_TRY(counts_to_host(r));
  *band = r->cells_pin.p;
  if (counts) *counts = (const vs_allele_counts*)r->counts_pin.p;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  if (window) *window = r->ld_window;
  if (stat) *stat = r->ld_stat;
  if (col_ids) *col_ids = r->h_cols.data();
  return VS_OK;
}

int vs_result_ld_band_device(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* window, uint32_t* stat, const void** dev_counts,
                             const void** dev_band) {
  VS_TRY(device_matrix_ready(r, dev_band, kKindLd, "not an LD result (vs_query_ld_band)"));
  *dev_band = r->d_band;
  if (dev_counts) *dev_counts = r->d_counts;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  if (window) *window = r->ld_window;
  if (stat) *stat = r->ld_stat;
  return VS_OK;
}

int vs_result_get_ld_matrix(vs_result* r, uint64_t* n_regions, uint64_t* n_rows, uint64_t* n_cols, uint32_t* stat, const uint32_t** col_ids,
                            const vs_allele_counts** counts, const uint64_t** block_begin, const void** cells) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!cells) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindLdMatrix) return fail(VS_ERR_ARG, "not an LD-matrix result (vs_query_ld_matrix)");
  VS_TRY(array_to_host(r, r->d_ldm, (size_t)r->ldm_cells * 4, &r->cells_pin, "LD blocks"));
  VS_TRY(counts_to_host(r));
  VS_TRY(ld_block_begin_to_host(r));
  *cells = r->cells_pin.p;
  if (counts) *counts = (const vs_allele_counts*)r->counts_pin.p;
  if (block_begin) *block_begin = r->h_block_begin.data();
  if (n_regions) *n_regions = r->d.Q;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  if (stat) *stat = r->ld_stat;
  if (col_ids) *col_ids = r->h_cols.data();
  return VS_OK;
}

int vs_result_ld_matrix_device(vs_result* r, uint64_t* n_regions, uint64_t* n_rows, uint64_t* n_cols, uint32_t* stat, const void** dev_counts,
                               const void** dev_block_begin, const void** dev_cells) {
  VS_TRY(device_matrix_ready(r, dev_cells, kKindLdMatrix, "not an LD-matrix result (vs_query_ld_matrix)"));
  *dev_cells = r->d_ldm;
  if (dev_counts) *dev_counts = r->d_counts;
  if (dev_block_begin) *dev_block_begin = r->d_ldm_meta;
  if (n_regions) *n_regions = r->d.Q;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  if (stat) *stat = r->ld_stat;
  return VS_OK;
}

int vs_result_get_ld_prune(vs_result* r, uint64_t* n_regions, uint64_t* n_rows, uint64_t* n_cols, uint32_t* params, const uint32_t** col_ids,
                           const vs_allele_counts** counts, const uint64_t** keep_begin, const uint64_t** n_kept, const uint8_t** state) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!state) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindPrune) return fail(VS_ERR_ARG, "not a pruning result (vs_query_ld_prune)");
  VS_TRY(array_to_host(r, r->d_state, (size_t)r->prune_states, &r->cells_pin, "pruning verdicts"));
  VS_TRY(counts_to_host(r));
  VS_TRY(prune_meta_to_host(r));
  *state = (const uint8_t*)r->cells_pin.p;
  if (counts) *counts = (const vs_allele_counts*)r->counts_pin.p;
  if (keep_begin) *keep_begin = r->h_prune_meta.data();
  if (n_kept) *n_kept = r->h_prune_meta.data() + (r->d.Q + 1);
  if (n_regions) *n_regions = r->d.Q;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  if (params) { params[0] = r->ld_window; params[1] = r->prune_max_bp; params[2] = r->prune_T; params[3] = r->prune_min_ac; params[4] = r->prune_max_ac; }
  if (col_ids) *col_ids = r->h_cols.data();
  return VS_OK;
}

int vs_result_ld_prune_device(vs_result* r, uint64_t* n_regions, uint64_t* n_rows, uint64_t* n_cols, const void** dev_counts, const void** dev_keep_begin,
                              const void** dev_n_kept, const void** dev_state) {
  VS_TRY(device_matrix_ready(r, dev_state, kKindPrune, "not a pruning result (vs_query_ld_prune)"));
  *dev_state = r->d_state;
  if (dev_counts) *dev_counts = r->d_counts;
  if (dev_keep_begin) *dev_keep_begin = r->d_prune_meta;
  if (dev_n_kept) *dev_n_kept = r->d_prune_meta + (r->d.Q + 1);
  if (n_regions) *n_regions = r->d.Q;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  return VS_OK;
}

int vs_result_get_ld_scores(vs_result* r, uint64_t* n_regions, uint64_t* n_rows, uint64_t* n_cols, uint32_t* params, const uint32_t** col_ids,
                            const vs_allele_counts** counts, const uint64_t** keep_begin, const uint64_t** n_scored, const uint64_t** sums, const uint32_t** n_pairs,
                            const uint8_t** state) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!sums) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindLdScore) return fail(VS_ERR_ARG, "not an LD-score result (vs_query_ld_scores)");
  VS_TRY(array_to_host(r, r->d_ldscore, (size_t)r->prune_states * 13, &r->cells_pin, "LD scores"));
  VS_TRY(counts_to_host(r));
  VS_TRY(prune_meta_to_host(r));
  const uint8_t* base = (const uint8_t*)r->cells_pin.p;
  *sums = (const uint64_t*)base;
  if (n_pairs) *n_pairs = (const uint32_t*)(base + 8 * r->prune_states);
  if (state) *state = base + 12 * r->prune_states;
  if (counts) *counts = (const vs_allele_counts*)r->counts_pin.p;
  if (keep_begin) *keep_begin = r->h_prune_meta.data();
  if (n_scored) *n_scored = r->h_prune_meta.data() + 2 * (r->d.Q + 1);
  if (n_regions) *n_regions = r->d.Q;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  if (params) { params[0] = r->ld_window; params[1] = r->prune_max_bp; params[2] = r->prune_min_ac; params[3] = r->prune_max_ac; }
  if (col_ids) *col_ids = r->h_cols.data();
  return VS_OK;
}

int vs_result_ld_scores_device(vs_result* r, uint64_t* n_regions, uint64_t* n_rows, uint64_t* n_cols, uint64_t* n_slots, const void** dev_counts,
                               const void** dev_keep_begin, const void** dev_n_scored, const void** dev_sums, const void** dev_n_pairs, const void** dev_state) {
  VS_TRY(device_matrix_ready(r, dev_sums, kKindLdScore, "not an LD-score result (vs_query_ld_scores)"));
  *dev_sums = r->d_ldscore;
  if (dev_n_pairs) *dev_n_pairs = r->d_ldscore + 8 * r->prune_states;
  if (dev_state) *dev_state = r->d_ldscore + 12 * r->prune_states;
  if (dev_counts) *dev_counts = r->d_counts;
  if (dev_keep_begin) *dev_keep_begin = r->d_prune_meta;
  if (dev_n_scored) *dev_n_scored = r->d_prune_meta + 2 * (r->d.Q + 1);
  if (n_regions) *n_regions = r->d.Q;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  if (n_slots) *n_slots = r->prune_states;
  return VS_OK;
}

int vs_result_get_ld_clump(vs_result* r, uint64_t* n_regions, uint64_t* n_rows, uint64_t* n_cols, uint32_t* params, uint64_t* p_keys, double* p_bounds,
                           const uint32_t** col_ids, const vs_allele_counts** counts, const uint64_t** keep_begin, const uint64_t** n_index, const uint64_t** rounds,
                           const uint8_t** state, const uint32_t** owner) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!state || !owner) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindClump) return fail(VS_ERR_ARG, "not a clumping result (vs_query_ld_clump)");
  VS_TRY(array_to_host(r, r->d_state, (size_t)r->prune_states, &r->cells_pin, "clumping verdicts"));
  VS_TRY(array_to_host(r, r->d_owner, (size_t)r->prune_states * 4, &r->owner_pin, "clump owners"));
  VS_TRY(counts_to_host(r));
  VS_TRY(prune_meta_to_host(r));
  *state = (const uint8_t*)r->cells_pin.p;
  *owner = (const uint32_t*)r->owner_pin.p;
  if (counts) *counts = (const vs_allele_counts*)r->counts_pin.p;
  if (keep_begin) *keep_begin = r->h_prune_meta.data();
  if (n_index) *n_index = r->h_prune_meta.data() + (r->d.Q + 1);
  if (rounds) *rounds = r->h_prune_meta.data() + 2 * (r->d.Q + 1) + 4;
  if (n_regions) *n_regions = r->d.Q;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  if (params) { params[0] = r->ld_window; params[1] = r->prune_max_bp; params[2] = r->prune_T; }
  if (p_keys) { p_keys[0] = r->clump_key[0]; p_keys[1] = r->clump_key[1]; }
  if (p_bounds) { p_bounds[0] = r->clump_p[0]; p_bounds[1] = r->clump_p[1]; }
  if (col_ids) *col_ids = r->h_cols.data();
  return VS_OK;
}

int vs_result_ld_clump_device(vs_result* r, uint64_t* n_regions, uint64_t* n_rows, uint64_t* n_cols, const void** dev_counts, const void** dev_keep_begin,
                              const void** dev_n_index, const void** dev_state, const void** dev_owner) {
  VS_TRY(device_matrix_ready(r, dev_state, kKindClump, "not a clumping result (vs_query_ld_clump)"));
  *dev_state = r->d_state;
  if (dev_owner) *dev_owner = r->d_owner;
  if (dev_counts) *dev_counts = r->d_counts;
  if (dev_keep_begin) *dev_keep_begin = r->d_prune_meta;
  if (dev_n_index) *dev_n_index = r->d_prune_meta + (r->d.Q + 1);
  if (n_regions) *n_regions = r->d.Q;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  return VS_OK;
}

int vs_result_get_sample_gram(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* stat, const uint32_t** col_ids, const vs_allele_counts** counts,
                              const int64_t** gram, const double** grm, const int64_t** col_weighted, int64_t* C, int64_t* H) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!gram) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindGram) return fail(VS_ERR_ARG, "not a Gram result (vs_query_sample_gram)");
  VS_TRY(array_to_host(r, r->d_gram, r->gram_words * 8, &r->cells_pin, "Gram matrix"));
  VS_TRY(counts_to_host(r));
  const int64_t* w = (const int64_t*)r->cells_pin.p;
  const size_t nc = r->h_cols.size();
  *gram = w;
  if (grm) *grm = r->gram_stat == VS_GRAM_GRM ? (const double*)(w + r->gram_grm_off) : nullptr;
  if (col_weighted) *col_weighted = w + nc * nc;
  if (C) *C = w[nc * nc + nc];
  if (H) *H = w[nc * nc + nc + 1];
  if (counts) *counts = (const vs_allele_counts*)r->counts_pin.p;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = nc;
  if (stat) *stat = r->gram_stat;
  if (col_ids) *col_ids = r->h_cols.data();
  return VS_OK;
}

int vs_result_sample_gram_device(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* stat, const void** dev_counts, const void** dev_gram,
                                 const void** dev_grm, const void** dev_col_weighted) {
  VS_TRY(device_matrix_ready(r, dev_gram, kKindGram, "not a Gram result (vs_query_sample_gram)"));
  const size_t nc = r->h_cols.size();
  *dev_gram = r->d_gram;
  if (dev_grm) *dev_grm = r->gram_stat == VS_GRAM_GRM ? (const void*)(r->d_gram + r->gram_grm_off) : nullptr;
  if (dev_col_weighted) *dev_col_weighted = r->d_gram + nc * nc;   // (C and H follow the n sums)
  if (dev_counts) *dev_counts = r->d_counts;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = nc;
  if (stat) *stat = r->gram_stat;
  return VS_OK;
}

int vs_result_get_sample_ibs(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* stat, const uint32_t** col_ids, const vs_allele_counts** counts,
                             const int64_t** het_het, const int64_t** hom_hom, const int64_t** carrier_both, const int64_t** ibs0, const int64_t** ibs2,
                             const double** king, int64_t* n_used) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!het_het) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindIbs) return fail(VS_ERR_ARG, "not an IBS result (vs_query_sample_ibs)");
  VS_TRY(array_to_host(r, r->d_ibs, r->ibs_words * 8, &r->cells_pin, "IBS matrices"));
  VS_TRY(counts_to_host(r));
  const int64_t* w = (const int64_t*)r->cells_pin.p;
  const size_t nc = r->h_cols.size(), nn = nc * nc;
  *het_het = w;
  if (hom_hom) *hom_hom = w + nn;
  if (carrier_both) *carrier_both = w + 2 * nn;
  if (ibs0) *ibs0 = w + 3 * nn;
  if (ibs2) *ibs2 = w + 4 * nn;
  if (n_used) *n_used = w[5 * nn];
  if (king) *king = r->ibs_stat == VS_IBS_KING ? (const double*)(w + r->ibs_king_off) : nullptr;
  if (counts) *counts = (const vs_allele_counts*)r->counts_pin.p;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = nc;
  if (stat) *stat = r->ibs_stat;
  if (col_ids) *col_ids = r->h_cols.data();
  return VS_OK;
}

int vs_result_sample_ibs_device(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* stat, const void** dev_counts, const void** dev_matrices,
                                const void** dev_king) {
  VS_TRY(device_matrix_ready(r, dev_matrices, kKindIbs, "not an IBS result (vs_query_sample_ibs)"));
  *dev_matrices = r->d_ibs;
  if (dev_king) *dev_king = r->ibs_stat == VS_IBS_KING ? (const void*)(r->d_ibs + r->ibs_king_off) : nullptr;
  if (dev_counts) *dev_counts = r->d_counts;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  if (stat) *stat = r->ibs_stat;
  return VS_OK;
}

int vs_result_get_trio_scan(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint64_t* n_trios, uint64_t* n_used, const uint32_t** col_ids,
                            const uint32_t** trio_cols, const vs_allele_counts** counts, const vs_trio_counts** rows, const vs_trio_counts** trios) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!rows) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindTrio) return fail(VS_ERR_ARG, "not a trio result (vs_query_trio_scan)");
  static_assert(sizeof(vs_trio_counts) == 16, "record layout of the ABI");
  VS_TRY(array_to_host(r, r->d_trio, r->trio_bytes, &r->cells_pin, "trio records"));
  VS_TRY(counts_to_host(r));
  const uint8_t* base = (const uint8_t*)r->cells_pin.p;
  *rows = (const vs_trio_counts*)base;
  if (trios) *trios = (const vs_trio_counts*)base + r->d.A;
  if (n_used) memcpy(n_used, base + (size_t)(r->d.A + r->n_trios) * 16, 8);
  if (trio_cols) *trio_cols = r->h_trio_cols.data();
  if (counts) *counts = (const vs_allele_counts*)r->counts_pin.p;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  if (n_trios) *n_trios = r->n_trios;
  if (col_ids) *col_ids = r->h_cols.data();
  return VS_OK;
}

int vs_result_trio_scan_device(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint64_t* n_trios, const void** dev_counts, const void** dev_rows,
                               const void** dev_trios, const void** dev_n_used) {
  VS_TRY(device_matrix_ready(r, dev_rows, kKindTrio, "not a trio result (vs_query_trio_scan)"));
  *dev_rows = r->d_trio;
  if (dev_trios) *dev_trios = r->d_trio + (size_t)r->d.A * 16;
  if (dev_n_used) *dev_n_used = r->d_trio + (size_t)(r->d.A + r->n_trios) * 16;
  if (dev_counts) *dev_counts = r->d_counts;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  if (n_trios) *n_trios = r->n_trios;
  return VS_OK;
}

int vs_result_get_roh(vs_result* r, uint64_t* n_regions, uint64_t* n_cols, uint64_t* n_rows, uint64_t* n_segments, vs_roh_params* params,
                      const uint32_t** col_ids, const vs_allele_counts** counts, const vs_roh_summary** summary, const uint32_t** n_sites,
                      const uint64_t** seg_begin, const vs_roh_segment** segments) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (!summary) return fail(VS_ERR_ARG, "null argument");
  if (r->kind != kKindRoh) return fail(VS_ERR_ARG, "not a ROH result (vs_query_roh)");
  static_assert(sizeof(vs_roh_summary) == 32 && sizeof(vs_roh_segment) == 32, "record layout of the ABI");
  VS_TRY(array_to_host(r, r->d_roh, r->roh_bytes, &r->cells_pin, "ROH summaries"));
  if (counts) VS_TRY(counts_to_host(r));
  if (r->roh.segments && segments) VS_TRY(array_to_host(r, r->d_roh_seg, (size_t)r->roh_segs * 32, &r->owner_pin, "ROH segments"));
  const uint8_t* base = (const uint8_t*)r->cells_pin.p;
  *summary = (const vs_roh_summary*)base;
  if (n_sites) *n_sites = (const uint32_t*)(base + r->roh_sites_off);
  if (seg_begin) *seg_begin = r->roh.segments ? (const uint64_t*)(base + r->roh_begin_off) : nullptr;
  if (segments) *segments = r->roh.segments ? (const vs_roh_segment*)r->owner_pin.p : nullptr;
  if (counts) *counts = (const vs_allele_counts*)r->counts_pin.p;
  if (n_regions) *n_regions = r->d.Q;
  if (n_cols) *n_cols = r->h_cols.size();
  if (n_rows) *n_rows = r->d.A;
  if (n_segments) *n_segments = r->roh_segs;
  if (params) *params = r->roh;
  if (col_ids) *col_ids = r->h_cols.data();
  return VS_OK;
}

int vs_result_roh_device(vs_result* r, uint64_t* n_regions, uint64_t* n_cols, uint64_t* n_rows, uint64_t* n_segments, const void** dev_counts,
                         const void** dev_summary, const void** dev_n_sites, const void** dev_seg_begin, const void** dev_segments) {
  VS_TRY(device_matrix_ready(r, dev_summary, kKindRoh, "not a ROH result (vs_query_roh)"));
  *dev_summary = r->d_roh;
  if (dev_n_sites) *dev_n_sites = r->d_roh + r->roh_sites_off;
  if (dev_seg_begin) *dev_seg_begin = r->roh.segments ? r->d_roh + r->roh_begin_off : nullptr;
  if (dev_segments) *dev_segments = r->roh.segments ? r->d_roh_seg : nullptr;
  if (dev_counts) *dev_counts = r->d_counts;
  if (n_regions) *n_regions = r->d.Q;
  if (n_cols) *n_cols = r->h_cols.size();
  if (n_rows) *n_rows = r->d.A;
  if (n_segments) *n_segments = r->roh_segs;
  return VS_OK;
}

int vs_result_assoc_scan_device(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* n_traits, uint32_t* stat, const void** dev_counts,
                                const void** dev_scores) {
  VS_TRY(device_matrix_ready(r, dev_scores, kKindAssoc, "not an association-scan result (vs_query_assoc_scan)"));
  *dev_scores = r->d_scores;
  if (dev_counts) *dev_counts = r->d_counts;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  if (n_traits) *n_traits = r->n_traits;
  if (stat) *stat = r->assoc_stat;
  return VS_OK;
}

int vs_result_assoc_matrix_device(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* n_traits, uint32_t* stat, const void** dev_counts,
                                  const void** dev_scores) {
  VS_TRY(device_matrix_ready(r, dev_scores, kKindAssocMatrix, "not a trait-matrix association result (vs_query_assoc_matrix)"));
  *dev_scores = r->d_scores;
  if (dev_counts) *dev_counts = r->d_counts;
  if (n_rows) *n_rows = r->d.A;
  if (n_cols) *n_cols = r->h_cols.size();
  if (n_traits) *n_traits = r->n_traits;
  if (stat) *stat = r->assoc_stat;
  return VS_OK;
}

int vs_result_sample_scores_device(vs_result* r, uint64_t* n_cols, uint32_t* n_scores, const void** dev_sums, const void** dev_scores) {
  VS_TRY(device_matrix_ready(r, dev_scores, kKindScores, "not a per-sample score result (vs_query_sample_scores)"));
  *dev_scores = r->d_score_out;
  if (dev_sums) *dev_sums = r->d_sums;
  if (n_cols) *n_cols = r->h_cols.size();
  if (n_scores) *n_scores = r->n_scores;
  return VS_OK;
}

int vs_result_score_matrix_device(vs_result* r, uint64_t* n_cols, uint32_t* n_scores, const void** dev_sums, const void** dev_scores) {
  VS_TRY(device_matrix_ready(r, dev_scores, kKindScoreMatrix, "not a score-matrix result (vs_query_score_matrix)"));
  *dev_scores = r->d_score_out;
  if (dev_sums) *dev_sums = r->d_sums;
  if (n_cols) *n_cols = r->h_cols.size();
  if (n_scores) *n_scores = r->n_scores;
  return VS_OK;
}

int vs_result_fill_ms(vs_result* r, float* ms) {
  VS_TRY(result_enter(r, Want::Any, true));   // (a refused speculative batch is run now: the time asked for is that of the expansion that produced the result)
  if (!ms) return fail(VS_ERR_ARG, "null argument");
  VS_TRY(result_ready(r));
  *ms = r->fill_ms;
  return VS_OK;
}

int vs_result_layout(const vs_result* r, uint64_t* n_slots, uint64_t* table_rows, uint64_t* arena_entries, uint64_t* lists_expanded, int* shared) {
  VS_TRY(result_enter(const_cast<vs_result*>(r), Want::Variants, true));
  if (n_slots) *n_slots = r->n_rows_reported;
  if (table_rows) *table_rows = r->d.A;
  if (arena_entries) *arena_entries = r->resident ? 0 : r->d.S;   // (a result over resident lists owns no arena)
  if (lists_expanded) *lists_expanded = r->n_unique_sites;
  if (shared) *shared = r->shared_lists ? 1 : 0;
  return VS_OK;
}

int vs_result_digest(vs_result* r, uint64_t* digest) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (no_lists(r)) return refuse_no_lists(r, "vs_result_digest");
  if (!digest) return fail(VS_ERR_ARG, "null argument");
  vs_index* idx = r->idx;
  VS_TRY(result_ready(r));
  ScratchBufs tmp(idx);
  void* dd = nullptr;
  VS_TRY(dev_alloc(idx, 8, &dd, &tmp.bufs));
  HIP_TRY(hipMemsetAsync(dd, 0, 8, idx->stream));
  if (r->d.A && r->d.Q) {   // the carrier part of every table row once, then every (region, row) pair
    void* rh = nullptr;
    VS_TRY(dev_alloc(idx, r->d.A * 8, &rh, &tmp.bufs));
    const uint64_t blocks = std::min<uint64_t>((r->d.A + 3) / 4, 8192);
    hipLaunchKernelGGL(k_digest_rows, dim3((unsigned)blocks), dim3(256), 0, idx->stream, r->d, (uint64_t*)rh);
    hipLaunchKernelGGL(k_digest, dim3((unsigned)((r->d.Q + 3) / 4)), dim3(256), 0, idx->stream, idx->d, r->d, (const uint64_t*)rh, (uint64_t*)dd);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(digest, dd, 8, hipMemcpyDeviceToHost, idx->stream));
  HIP_TRY(hipStreamSynchronize(idx->stream));
  tmp.release();
  return VS_OK;
}

int vs_result_pack_headers(vs_result* r, void* device_dst, uint64_t capacity_records, uint64_t region_base,
                           uint64_t* n_records) {
  VS_TRY(result_enter(r, Want::Variants, true));
  if (no_lists(r)) return refuse_no_lists(r, "vs_result_pack_headers");
  if (n_records) *n_records = r->n_rows_reported;   // rows over all regions (a shared row once per region reporting it)
  if (!device_dst) return VS_OK;  // size query
  if (capacity_records < r->n_rows_reported) return fail(VS_ERR_ARG, "destination holds %llu records, %llu needed",
                                                        (unsigned long long)capacity_records, (unsigned long long)r->n_rows_reported);
  vs_index* idx = r->idx;
  if (r->d.Q) {
    ScratchBufs tmp(idx);
    uint64_t* slot_begin = nullptr;
    VS_TRY(dev_alloc(idx, (r->d.Q + 1) * 8, (void**)&slot_begin, &tmp.bufs));
    VS_TRY(exclusive_scan<uint64_t>(idx, r->d.q_nvar, r->d.Q, slot_begin, &tmp.bufs));
    hipLaunchKernelGGL(k_pack_headers, dim3((unsigned)((r->d.Q + 3) / 4)), dim3(256), 0, idx->stream, r->d,
                       (uint64_t*)device_dst, (const uint64_t*)slot_begin, region_base);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(idx->stream));
    tmp.release();
  }
  HIP_TRY(hipStreamSynchronize(idx->stream));
  return VS_OK;
}

int vs_result_pack_regions(vs_result* r, void* device_dst, uint64_t capacity_records, uint64_t region_base,
                           uint64_t* n_records) {
  // (a size query: the region count is known -- a refused batch is redone before its records travel, not before)
  VS_TRY(result_enter(r, Want::Any, /*sizes=*/device_dst != nullptr));
  if (no_lists(r)) return refuse_no_lists(r, "vs_result_pack_regions");
  if (n_records) *n_records = r->d.Q;
  if (!device_dst) return VS_OK;
  if (capacity_records < r->d.Q) return fail(VS_ERR_ARG, "destination holds %llu records, %llu needed",
                                             (unsigned long long)capacity_records, (unsigned long long)r->d.Q);
  vs_index* idx = r->idx;
  VS_TRY(launch_pack_regions(r, (uint64_t*)device_dst, region_base));
  HIP_TRY(hipStreamSynchronize(idx->stream));
  return VS_OK;
}

}  // extern "C"

#include "comm.hip.h"
