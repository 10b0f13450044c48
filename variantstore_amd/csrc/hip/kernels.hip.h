// kernels.hip.h -- gfx950 device code of the region-query path.
//
// All integer / index work: the roofline that bounds these kernels is HBM
// bandwidth (and memory latency for the gather phases), never MFMA.
// Wavefront width is 64 throughout; one workgroup = 256 threads = 4 waves.
//
// Kernel                replaces (reference file:line)
// --------------------  ------------------------------------------------------
// k_build_sites         next_variant_in_ref's per-node branch classification
//                       (include/query.h:308-393) + the radius-1 neighbour walk
//                       (include/graph.h:394-431), run ONCE over the whole ref
//                       path when an index is opened (the "site table")
// k_mark_dups           the candidates the "already seen" rule can ever hit
//                       (include/query.h:397-414)
// k_region_bounds       Index::is_empty / Index::find (include/index.h:119-166)
//                       + the stop rule ref_index+length >= end (query.h:312)
// k_emit_headers        building std::vector<Variant> (query.h:736-771)
// k_dedup_slow          the literal "already seen" rule for the rare regions
//                       that contain a repeated (pos, alt)
// k_t6_bounds / _mid /  the plan of a SORTED type-6 batch whose regions share rows and carrier lists (the reference's
//  _totals / _apply     driver sorts its regions, src/commands.cc:91): is_empty / find / stop rule per region, the sites each
//                       region is the first to cover, run records, totals for the host (k_rows.hip.h)
// k_t6_slow             private rows + the literal "already seen" rule for the regions under it
// k_fill_sites2         the shared rows AND their carrier lists: get_samples -> get_sample_id / get_sample_phasing
//                       (query.h:268-285, variant_graph.h:875-1006) once per covered site.  THE DOMINANT KERNEL
//                       (DESIGN.md section 6); k_fill_dense: its dense variants alone (tuning builds, for profilers)
// k_fill_carriers       the same expansion over private rows (share_lists = 0, point queries, the walking types' lists):
//                       decoded class id lists / class bit rows + genotype bits into carrier lists
// k_query_small         a whole get_var_in_ref batch of <= 64 regions in one launch
//                       (bounds, offsets, headers, carriers, dedup): the latency path
// k_query_server        the same, resident: polls requests in mapped host memory
// k_point_bounds        one next_variant_in_ref call from a position (query.h:297-436)
//                       as used by closest_var (query.h:441-483, type 1) and
//                       samples_has_var (query.h:792-823, type 7)
// k_has_var_filter      the (pos, ref, alt) match of samples_has_var (query.h:802-803)
// k_sample_walk_sc      get_sample_var_in_sample (query.h:490-612, type 5), one lane per region;
// k_sample_walk_sc_coop  eight lanes per region, the sample's events walked as episodes in parallel
// k_sample_seq          query_sample_from_ref / query_sample_from_sample
//                       (query.h:118-261, types 2 and 3): the walk emits (offset, length)
//                       pieces of the sequence pool; k_copy_segments decodes them;
// k_sample_seq_coop      the cooperative form (window logic of query.h:160-177 / :236-247 at the hand-over)
// k_sample_walk_coop    get_prev_vertex_with_sample + get_sample_var_in_ref (query.h:618-729, type 4), eight lanes per region;
//  (k_sample_walk)       WalkAdmit holds a batch to the scratch its predecessor needed; k_t4_claim / _offsets(_small): one carrier
//                       list per reported vertex; k_emit_from_walk: the rows (query.h:680-704)
// k_walk_setup /        the first kernel of a walking batch whose regions and sample ids are in device memory: the result's
//  k_seq_setup           copies, the range check of the ids, the capacities of the recording walk (no reference counterpart:
//                       the reference reads its regions from a file, src/commands.cc:100-140)
// k_scan_*, k_scan2_*,  offsets of rows, arena and scratch (exclusive scans over the regions of a batch; up to 16 k regions: one launch)
//  k_scan_small
// k_pack_regions /      what a sharded run gathers per region (the reference's loop, src/commands.cc:145-193, prints counts and
//  k_pack_seq_regions    flags per region): site range + counts, or pieces + bytes of a sequence; k_bounds_from_records: the
//                       receiving side (vs_query_expand_site_ranges)
// k_find                Index::find batched
// (k_carriers.hip.h)    no kernel: how the six column kernels below read the carriers of a table row -- the three storage forms of a
//                       group of 8 carriers, a row's site parameters, the flat list of groups, the head of a dense class-row chunk,
//                       sample id -> column; next to the expansion kernels the one place that knows how a carrier is stored
// k_allele_counts       allele counts per row of a type-6 plan over a sample subset (vs_query_allele_counts: no reference
//  k_count_slow_sites    counterpart; what a caller of type 6 would count on the host from the carrier lists)
// k_group_counts        the same counts per sample GROUP in one pass over a row's carriers: a label byte per sample in LDS, one packed
//                       LDS atomic per carrier, rows x groups records stored once (vs_query_group_counts: no reference counterpart)
// k_window_stats        those records reduced per region and group, and per pair of groups, to the integers of the windowed diversity
//                       statistics (rows, seg, singletons, private, fixed, sums of ac, ac^2, het, ac_g ac_h): a wave per region, 64-row
//                       tiles packed into LDS, lanes owning (row slice, group) and (row slice, pair); regions longer than a chunk split
//                       through k_burden_split_plan and added with integer atomics (vs_query_window_stats: no reference counterpart;
//                       DESIGN 5q)
// k_assoc_scan          every row scored against K phenotypes in one pass over its carriers: the carrier's K float32 values from a table
//                       in LDS or L2, dosage x value summed in float64 in an order the table's layout fixes (segmented lane scans, no
//                       floating-point atomic), rows x K cells stored once (vs_query_assoc_scan: no reference counterpart)
// k_sample_scores       the transpose of that product: samples x K weighted dosage sums over the rows a batch reports, the weights
//  k_score_scale         keyed by report order and quantised to 64-bit integers once per column (k_score_scale, k_score_offsets,
//  k_score_offsets       k_score_weights), a (row chunk, column tile) per workgroup with the tile as int64 in LDS, integer atomics only:
//  k_score_weights       every sum exact and order-free; k_score_finish forms the float64 scores (vs_query_sample_scores: no reference
//  k_score_finish        counterpart)
// k_sample_burden       the same counts along the other axis: a regions x samples matrix over each region's reported rows
//  k_burden_split_plan   (vs_query_sample_burden: no reference counterpart); the chunks of the regions too long for one workgroup
// k_genotype_matrix     what both reduce: table rows x samples, a byte per call, each (row block, column tile) built in LDS and
//                       stored once (vs_query_genotype_matrix: no reference counterpart)
// k_ld_band             the band of D D^T over that matrix's dosages -- every table row against the next W rows -- on the matrix
//                       cores (v_mfma_i32_16x16x64_i8, exact), as dot products or r^2 (vs_query_ld_band: no reference counterpart;
//                       with k_sample_gram the kernels here on the matrix cores; by DESIGN 5e's count its reads of the matrix bound it, not the MFMAs)
// k_ld_block            D D^T in full per region: the m x m block of every region of a batch, a pair of 64-row tiles per workgroup,
//  k_ld_block_scan       found by bisection over the scan of the regions' workgroups; k_ld_band's staging, fragments and r^2, both
//                       triangles stored once with plain stores (vs_query_ld_matrix: no reference counterpart)
// k_prune_hits          greedy LD pruning of every region: k_ld_band's products (ld_band_products) with a third epilogue -- a bit per
//  k_prune_scan          pair, r^2 > T / 2^20 decided in unsigned 128-bit integers, the mask rows assembled in LDS and stored once --,
//  k_prune_greedy        the scan of the regions' row counts, and the walk: a wave per region, a 256-bit wave-uniform register of
//                       blocked rows, the masks of 64 rows loaded ahead and taken with v_readlane, a state byte per row
//                       (vs_query_ld_prune: no reference counterpart)
// k_clump_class         p-value clumping of every region over k_prune_hits' masks: the greedy in priority order -- (key of the
//  k_clump_blockers      p-value, table row) ascending, unsigned integers only -- decided in parallel rounds.  A class per table row,
//  k_clump_rounds        per verdict slot the mask of the hitting rows that outrank it (both directions of the window), then one
//                       workgroup per region: a row is a member once a blocker is an index, an index once every blocker is
//                       decided and none is; in-place updates, no host wait between rounds; owners and n_index in a last pass
//                       (vs_query_ld_clump: no reference counterpart)
// k_ld_score            the LD score of every row of every region: k_ld_block's products (ld_block_products) with an epilogue that
//  k_ld_score_scan       reduces the cells instead of storing them -- floor(cov^2 2^32 / (v_a v_b)) per eligible pair from 128-bit
//  k_ld_score_init       integers (ld_score_q32), summed per row over a window of rows and positions with no 256-row ceiling, one
//                       64-bit integer atomic per row and tile pair: exact and order-free; the scan of the regions' slots and
//                       workgroups, and the state bytes (vs_query_ld_scores: no reference counterpart)
// k_assoc_matrix        D Y over the same dosages: table rows x K traits (K up to 65,536) given as four int8 limbs of a fixed-point
//                       value, 64 rows x 16 traits per workgroup, k_ld_band's staging and fragments, four MFMAs per 64-column step,
//                       the limb sums combined in int64: exact dot products or the score test from 128-bit integers
//                       (vs_query_assoc_matrix: no reference counterpart)
// k_sample_gram         D^T D over the same dosages, the samples x samples Gram matrix: a pair of 128-column tiles and a chunk of
//  k_gram_moments       table rows per workgroup, the tiles transposed into LDS, v_mfma_i32_16x16x64_i8, 64-bit integer atomics;
//  k_gram_finish        the count-weighted column sums s, C and H; the GRM cells from 128-bit integers (vs_query_sample_gram: no
//                       reference counterpart)
// k_sample_ibs          the same staging once, three indicator products (het x het, hom x hom, carrier x carrier) into three sets of
//  k_ibs_n_used         int32 accumulators: the pairwise genotype-state counts D^T D cannot give; the rows the duplicate rule kept;
//  k_ibs_finish         IBS0 / IBS2 and the KING-robust kinship from exact integers (vs_query_sample_ibs: no reference counterpart;
//                       DESIGN 5j)
// k_trio_scan           Mendel's laws over the same dosages: per (child, father, mother) column triple and table row a 27-state look-up
//                       -- error, de novo, transmitted, untransmitted -- from three LDS byte reads, a block of rows staged per
//                       workgroup, a lane per trio; per-trio sums in the lane, per-row sums by one halving butterfly a wave,
//                       32-bit integer atomics: exact and order-free; n_used is k_ibs_n_used's (vs_query_trio_scan: no reference
//                       counterpart)
// k_roh_sites           Runs of homozygosity: per table row {pos, site} from the count records (eligible as for pruning: kept,
//  k_roh_walk           polymorphic, inside the allele-count window); then a COLUMN walk of the temporary matrix -- a workgroup per
//                       (region, 256 columns), blocks of 64 rows staged in LDS through registers, double-buffered, a block without
//                       a site skipped, a lane per column, the run machine in registers, selects but for the close; pass 1 the
//                       32-byte summaries, the engine's scan over n_segments, pass 2 the segments.  Integers only (vs_query_roh:
//                       no reference counterpart)
// k_score_matrix        D^T W over the same dosages: samples x K weighted sums (K up to 65,536) over the rows a batch reports, the
//  k_score_matrix_weights  wide form of k_sample_scores.  The report-keyed weights become per-row totals of fixed-point integers
//  k_score_matrix_limbs    (64-bit atomics), the totals a panel of four or five int8 limbs; 128 columns x 16 or 32 scores x a chunk
//  k_score_matrix_finish   of rows per workgroup, k_sample_gram's transposing stage, the limb sums combined in int64 and added to
//                       the sums with 64-bit integer atomics: exact and order-free (vs_query_score_matrix: no reference counterpart;
//                       DESIGN 5m)
#pragma once
#include "k_image.hip.h"
#include "k_sites.hip.h"
#include "k_scan.hip.h"
#include "k_rows.hip.h"
#include "k_expand.hip.h"
#include "k_latency.hip.h"
#include "k_walk.hip.h"
#include "k_points.hip.h"
#include "k_sample_coords.hip.h"
#include "k_digest.hip.h"
#include "k_carriers.hip.h"
#include "k_counts.hip.h"
#include "k_group_counts.hip.h"
#include "k_assoc.hip.h"
#include "k_scores.hip.h"
#include "k_burden.hip.h"
#include "k_window_stats.hip.h"
#include "k_matrix.hip.h"
#include "k_ld.hip.h"
#include "k_ld_block.hip.h"
#include "k_prune.hip.h"
#include "k_clump.hip.h"
#include "k_ld_score.hip.h"
#include "k_int128.hip.h"
#include "k_gram.hip.h"
#include "k_assoc_matrix.hip.h"
#include "k_ibs.hip.h"
#include "k_trio.hip.h"
#include "k_roh.hip.h"
#include "k_score_matrix.hip.h"
