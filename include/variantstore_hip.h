/* variantstore_hip.h -- C ABI of the MI355X variant-query engine.
 *
 * The reference (Kingsford-Group/variantstore) has no plugin / FFI interface;
 * its query path is entered from `query_main` (reference src/commands.cc:114-215)
 * through two C++ calls on two objects built from an index directory:
 *
 *   Index idx(prefix);                         include/index.h:108-117
 *   VariantGraph vg(prefix, mode);             include/variant_graph.h:366-446
 *   get_var_in_ref(&vg,&idx,x,y,print,file)    include/query.h:736-784   (query type 6)
 *   get_sample_var_in_ref(...,sample,...)      include/query.h:618-729   (query type 4)
 *
 * This header is that seam as a C ABI: plain pointers and sizes, int error
 * codes, no exceptions, no C++ or torch types.  One vs_index per device; calls on
 * one handle must be serialised by the caller; different handles may be used
 * from different host threads.  Every entry point that computes runs on the GPU:
 * there is no CPU fallback, and a handle opened without a device refuses queries
 * with VS_ERR_NO_DEVICE.
 */
#ifndef VARIANTSTORE_HIP_H
#define VARIANTSTORE_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct vs_index vs_index;   /* replaces the (Index, VariantGraph) pair: host copy + HBM image */
typedef struct vs_result vs_result; /* replaces std::vector<Variant> per region (query.h:30-36), batched */

enum {
  VS_OK = 0,
  VS_ERR_IO = -1,          /* index directory / file unreadable or malformed   */
  VS_ERR_FORMAT = -2,      /* on-disk structure violates the layout contract   */
  VS_ERR_NO_DEVICE = -3,   /* no usable GPU / handle opened host-only          */
  VS_ERR_HIP = -4,         /* a HIP runtime call failed                        */
  VS_ERR_ARG = -5,         /* bad argument                                     */
  VS_ERR_UNKNOWN_SAMPLE = -6,
  VS_ERR_UNSUPPORTED = -7,
  VS_ERR_INTERNAL = -8
};
const char* vs_strerror(int code);
/* message of the last failure on the calling thread (empty string if none) */
const char* vs_last_error(void);

/* ---- region ------------------------------------------------------------ */
typedef struct { uint64_t x, y; } vs_region; /* [pos_x, pos_y), 1-based: std::get<0>/<1> of commands.cc:64-93 */

/* ---- construction: `variantstore construct` (commands.cc:33-60) ---------- */
typedef struct {
  uint64_t num_vars, num_mutations, num_mutations_samples;  /* the "Num mutations" log line */
  uint64_t num_vertices, num_edges, seq_length;              /* the "Graph stats" log line  */
  uint64_t num_classes;                                       /* "Number of sample vector classes" */
  uint32_t use_bit_vector;
} vs_construct_stats;

/* Build a graph from FASTA + VCF entirely in memory and open it on `device`
 * (device < 0: host-only handle, for inspection/export; queries are refused). */
int vs_index_from_vcf(const char* fasta, const char* vcf, int device, vs_construct_stats* stats, vs_index** out);

/* Deterministic synthetic cohort (bench / scale tests): a random reference of
 * `ref_length` bases, `num_variants` sites (SNP / insertion / deletion mix, some
 * multi-allelic), `num_samples` samples with a skewed allele-frequency spectrum,
 * fed record by record through the same constructor as a VCF would be. */
typedef struct {
  uint64_t ref_length;
  uint64_t num_variants;
  uint32_t num_samples;
  uint64_t seed;
  uint64_t first_pos;        /* variants are placed in [first_pos, ref_length) */
  double frac_ins, frac_del; /* remaining fraction are SNPs                    */
  double frac_multi;         /* fraction of SNP sites with a second ALT        */
  uint32_t max_indel;        /* indel length 1..max_indel                      */
  double af_exponent;        /* AF = min(0.5, 10^(-af_exponent * U))           */
  uint32_t sample_coordinates; /* != 0: also compute the per-carrier sample-coordinate indexes (the reference's
                                * "Fixing sample indexes" pass, variant_graph.h:1919-1997) that query types 2, 3 and 5
                                * read; 4 bytes per carrier record                                                      */
  double max_af;             /* cap of the allele frequency; 0 = 0.5.  Small caps give somatic-like cohorts that the
                              * constructor stores with explicit sample ids instead of class bit vectors          */
} vs_synth_params;
int vs_index_synthetic(const vs_synth_params* p, int device, vs_construct_stats* stats, vs_index** out);

/* Open an index directory written by `variantstore construct` (Index(prefix) +
 * VariantGraph(prefix, mode): index.h:108-117, variant_graph.h:366-446). */
int vs_index_open(const char* prefix, int device, vs_index** out);
/* Write the index directory (VariantGraph::serialize + Index::serialize). */
int vs_index_save(const vs_index* idx, const char* prefix);
/* Releases the handle.  If results of this handle are still alive the release is deferred to the vs_result_free of
 * the last one (their arrays live in the handle's HBM pool); the handle must not be used for new calls meanwhile. */
void vs_index_close(vs_index* idx);

typedef struct {
  uint64_t ref_length, num_vertices, num_edges_csr, ref_path_nodes, index_nodes;
  uint64_t num_classes, num_sites, num_carriers, seq_length;
  uint32_t num_samples;      /* includes "ref" */
  uint32_t use_bit_vector;
  uint64_t device_bytes;     /* HBM held by the image */
  int device;
  uint64_t num_topology_keys; /* Graph::get_num_vertices(): vertices with an adjacency entry (graph.h:318-320) */
  uint32_t list_max;         /* classes of at most this many carriers are expanded from decoded id lists (16-bit entries up
                              * to 4032 samples, else 32-bit), denser ones from their bit row; 0: explicit-id cohort   */
  uint32_t reserved_;
  uint64_t t4_rows_bytes;    /* of device_bytes: the per-sample event and hold rows of query type 4 (O(samples x ref-path slots):
                              * taken when they fit half of the free HBM and 176 GB -- VS_T4_ROWS_MAX_GB in the environment
                              * lowers the cap, option "t4_rows_max_mb" drops / rebuilds them on the open handle; 0: not built, the walks
                              * then visit every vertex).  Explicit-id cohorts keep coarse event rows (a bit per 8 slots) and no hold rows;
                              * VS_T4_EXACT_ROWS=1 in the environment gives them the exact form when it fits the same budget */
  uint64_t pool_mallocs;     /* hipMalloc / hipFree calls the handle's pool of batch buffers has made since it was opened: a loop */
  uint64_t pool_frees;       /* of like batches makes none once it is warm (hipFree waits for the whole device)                  */
  uint64_t t6_speculated;    /* type-6 batches submitted without waiting for their plan's totals (option "t6_speculate") ...       */
  uint64_t t6_refused;       /* ... and those of them the device refused (did not fit what was allocated, or unsorted) and the host  */
                             /* ran again with the exact sizes when the result was first asked for anything                          */
} vs_index_info;
int vs_index_get_info(const vs_index* idx, vs_index_info* info);
/* sampleid_map / idsample_map lookups (variant_graph.h:1230-1236, 1327-1339) */
int vs_index_sample_id(const vs_index* idx, const char* name, uint32_t* id);
const char* vs_index_sample_name(const vs_index* idx, uint32_t id);
const char* vs_index_chr(const vs_index* idx);
/* Dump the decoded index content in the flat format the test oracle reads. */
int vs_index_export_plain(const vs_index* idx, const char* path);
/* Host-side inspection used by structure tests (no GPU needed):
 * out-neighbours of v in the reference's iteration order; returns the degree. */
int64_t vs_index_out_neighbors(const vs_index* idx, uint32_t v, uint32_t* out, uint64_t cap);

/* ---- queries ------------------------------------------------------------ */
/* type 6: get_var_in_ref for each of the n regions (query.h:736-784).  Batches of at most 64 regions take the latency
 * path: one kernel for the whole query, or -- while the handle's resident query server is alive -- no launch at all
 * (by default only for back-to-back streaks of small queries -- vs_index_set_option
 * "latency_server"; VS_NO_SERVER=1 in the environment when the handle is opened keeps it to one launch per call). */
int vs_query_var_in_ref(vs_index* idx, const vs_region* regions, uint64_t n, vs_result** out);
/* The same with the regions already in DEVICE memory of the handle's GPU (e.g. produced there, or uploaded once and
 * queried repeatedly): no host buffer crosses PCIe inside the call.  Always the batch pipeline, whatever n. */
int vs_query_var_in_ref_device(vs_index* idx, const vs_region* device_regions, uint64_t n, vs_result** out);
/* The receiving side of the hit-list collective (vs_result_pack_regions below): n compact region records in DEVICE
 * memory -- this rank's own or gathered from other ranks holding the same index -- expanded into a full type-6 result
 * (variant rows + carrier lists), exactly what the producing rank holds.  Records whose site range does not fit this
 * index come back as VS_REGION_INVALID. */
int vs_query_expand_site_ranges(vs_index* idx, const void* device_records, uint64_t n, vs_result** out);
/* type 4: get_sample_var_in_ref for one sample over n regions (query.h:618-729) */
int vs_query_sample_var_in_ref(vs_index* idx, const vs_region* regions, uint64_t n, uint32_t sample_id,
                               vs_result** out);
/* type 4 with one sample id per region (a batch mixing samples, e.g. the cohort round-robin of the bench).
 * Here and in vs_query_sample_seq / vs_query_sample_var_in_sample, `regions` and `sample_ids` may each lie in host
 * memory or in DEVICE memory of the handle's GPU (the engine asks the runtime which): device arrays are neither read
 * on the host nor copied over the link, and an id out of range is found by the batch's first kernel instead of the
 * host loop -- the call fails with VS_ERR_UNKNOWN_SAMPLE either way. */
int vs_query_samples_var_in_ref(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids,
                                vs_result** out);
/* Query type 1, closest_var (include/query.h:441-483; called from src/commands.cc:151-155): the variants of the
 * site nearest to each position, found exactly as the reference does (one next_variant_in_ref call forwards, one
 * mirrored call backwards, or the one-position-at-a-time step back when nothing lies ahead).  Each position gives one
 * "region" of the result; VS_REGION_NOT_FOUND marks a call for which the reference returns false (it then writes
 * no output file and vs_result_format_region gives an empty text). */
int vs_query_closest_var(vs_index* idx, const uint64_t* positions, uint64_t n, vs_result** out);
/* Query type 7, samples_has_var (include/query.h:792-823; src/commands.cc:181-189): the carriers of the variant
 * (positions[i], refs[i], alts[i]) among the variants ONE next_variant_in_ref(positions[i]) call reports.
 * refs/alts are NUL-terminated strings compared byte for byte with the index's sequences.  A region of the result
 * holds one variant when found (vs_result_format_region then gives the reference's output line: `name gt` pairs
 * with no separator, then a newline) and carries VS_REGION_NOT_FOUND otherwise ("There is no such variant!"). */
int vs_query_samples_has_var(vs_index* idx, const uint64_t* positions, const char* const* refs, const char* const* alts,
                             uint64_t n, vs_result** out);
/* Query types 2 and 3, query_sample_from_ref / query_sample_from_sample (include/query.h:118-190, :196-261;
 * src/commands.cc:156-165): the sequence of sample sample_ids[i] over regions[i] = [x, y) in reference coordinates
 * (sample_coordinates == 0) or in the sample's own coordinates (!= 0).  The result is a SEQUENCE result: read it with
 * vs_result_get_sequences or vs_result_format_region (sequence + '\n', the reference's output file).  Regions on
 * which the reference dies of an uncaught std::out_of_range carry VS_REGION_INVALID, regions on which its backward
 * search never ends carry VS_REGION_ENDLESS; both give an empty sequence.  Needs an index with sample coordinates
 * (every index built from a VCF or loaded from disk has them). */
int vs_query_sample_seq(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, int sample_coordinates,
                        vs_result** out);
/* Query type 5, get_sample_var_in_sample (include/query.h:490-612; src/commands.cc:171-175): the variants on the path
 * of sample_ids[i] over regions[i] in the SAMPLE's coordinates; an ordinary variant-table result.  var_pos follows the
 * reference: the sample-coordinate index for substitutions and deletions, the reference index for insertions. */
int vs_query_sample_var_in_sample(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, vs_result** out);
/* Allele counts over regions, optionally for a subset S of the samples (no reference counterpart: what a caller of type 6
 * would count on the host from the carrier lists).  Each region reports the rows type 6 reports -- same positions, REF / ALT,
 * order, duplicate rule (dropped rows flagged as in vs_result_raw) and region flags -- and each row carries, instead of a
 * carrier list, four counts over its carriers c that lie in S.  They come from the genotype bits the index stores per carrier
 * (VS_CARRIER_GT: bit 0 phase, bit 1 gt_1, bit 2 gt_2), not from the VCF's allele indices: the constructor sets gt_1 / gt_2 for
 * ANY allele > 0, so a `1|2` call counts 2 alternate alleles on both of its ALT rows, and a haploid `1` counts as gt_1 alone.
 *   carriers    = |{c in S}|
 *   alt_alleles = sum over c in S of gt_1 + gt_2
 *   hom_alt     = |{c in S : gt_1 && gt_2}|
 *   phased      = |{c in S : phase}|
 * A dropped row counts 0. */
typedef struct { uint32_t carriers, alt_alleles, hom_alt, phased; } vs_allele_counts;
/* `regions` may lie in host memory or in DEVICE memory of the handle's GPU (the engine asks the runtime which); n >= 1.
 * sample_ids == NULL: the whole cohort (every sample but "ref"); else a HOST array of n_ids >= 1 index sample ids, taken as a set
 * (duplicates count once) -- id 0 ("ref") or an id >= num_samples fails with VS_ERR_UNKNOWN_SAMPLE, n_ids == 0 with VS_ERR_ARG.
 * Every batch size takes the batch pipeline: the type-6 plan and shared rows, then one counting kernel instead of the carrier
 * expansion (never speculative; the handle's type-6 state -- vs_index_info.t6_speculated / t6_refused, size and sort hints -- is
 * left as it was).  The result has the variant table of type 6 and no carrier arena: vs_result_get_raw / vs_result_get_view
 * with with_carriers = 0, vs_result_totals (n_carriers = the sum of `carriers` over the reported rows), vs_result_layout (arena
 * and lists 0), vs_result_fill_ms (the counting kernel) and vs_result_format_region
 * ("Pos\tRef\tAlt\tCarriers\tAC\tHomAlt\tPhased\n", then one line per reported row) work; with_carriers = 1, vs_result_digest,
 * vs_result_pack_headers / _pack_regions and vs_comm_allgather_regions* fail with VS_ERR_UNSUPPORTED. */
int vs_query_allele_counts(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids,
                           vs_result** out);
/* The counts of an allele-count result, copied into page-locked memory owned by the result: counts[i] belongs to
 * vs_result_raw.rows[i] (table order), so region q's are counts[row_begin[q] .. row_begin[q] + row_count[q]). */
int vs_result_get_allele_counts(vs_result* r, uint64_t* n_rows, const vs_allele_counts** counts);
/* Grouped allele counts: the counts above for each of several disjoint GROUPS of samples in one pass -- cases and controls, the
 * populations of a cohort, batches (no reference counterpart: what a caller would get from one vs_query_allele_counts call per group).
 * sample_ids[i] belongs to group group_of[i] in 0 .. n_groups - 1 (both HOST arrays of n_ids entries); a sample that is not listed
 * belongs to no group, the same (sample, group) pair given twice counts once, a group may be empty (size 0, all counts 0).
 * counts[i * n_groups + g] is the vs_allele_counts record of table row i over the samples of group g, with exactly the semantics of
 * vs_query_allele_counts with that group as the subset (index genotype bits: a `1|2` call counts 2 on both ALT rows, a haploid `1` is
 * gt_1 alone; a row dropped by the duplicate rule counts 0 in every group).  A batch whose table is empty gives 0 rows and is no error.
 * `regions` as for vs_query_allele_counts (host or device memory, n >= 1).  Checked on the host, in this order, before the handle's
 * device is asked for (a handle opened without a device reports them first and VS_ERR_NO_DEVICE otherwise): n == 0, NULL sample_ids,
 * NULL group_of, n_ids == 0, n_groups == 0 or n_groups > VS_GROUPS_MAX -> VS_ERR_ARG; some group_of[i] >= n_groups -> VS_ERR_ARG; id 0
 * ("ref") or an id >= num_samples -> VS_ERR_UNKNOWN_SAMPLE; a sample listed in two different groups -> VS_ERR_ARG (the message names
 * the sample id and both groups); a group name (group_names: NULL, or n_groups strings that are copied into the result) with a tab
 * or a newline -> VS_ERR_ARG.  The kernel keeps one label byte per sample id in LDS, 32 KiB of it (beside 29 KiB of accumulators,
 * staged genotype words and wave state: two workgroups per CU), and its packed 16-bit count fields hold 2 x samples: a cohort of more
 * than 32768 sample ids ("ref" included) is refused with VS_ERR_UNSUPPORTED.
 * rows x n_groups x 16 bytes are held to option "matrix_max_mib" (default 32 GiB): a larger request is refused with VS_ERR_ARG once
 * the plan has given the rows and before anything is allocated; the message names rows, groups and bytes.
 * Every batch size takes the batch pipeline; a grouped-count batch is never speculative and leaves the handle's type-6 state as it
 * was.  The result holds the type-6 per-region arrays and variant table, no carrier arena, and the records: vs_result_get_raw /
 * vs_result_get_view with with_carriers = 0, vs_result_layout (arena and lists 0), vs_result_fill_ms (the group kernel),
 * vs_result_totals (n_carriers = the sum of `carriers` over the rows every region reports and all groups) and
 * vs_result_format_region ("Pos\tRef\tAlt\tGroup\tN\tCarriers\tAC\tHomAlt\tPhased\n", then one line per reported, non-dropped row
 * and per group in group order; Group is the group's name, or its decimal index without names; N its size) work; with_carriers = 1,
 * vs_result_digest, vs_result_pack_headers / _pack_regions and vs_comm_allgather_regions* fail with VS_ERR_UNSUPPORTED, the other
 * kinds' getters with VS_ERR_ARG. */
#define VS_GROUPS_MAX 64u
int vs_query_group_counts(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, const uint32_t* group_of,
                          uint64_t n_ids, uint32_t n_groups, const char* const* group_names, vs_result** out);
/* The records of a grouped-count result copied into page-locked memory owned by the result: counts[i * n_groups + g];
 * group_sizes[g] the number of distinct samples of group g (either may be NULL but `counts`).  VS_ERR_ARG on any other result. */
int vs_result_get_group_counts(vs_result* r, uint64_t* n_rows, uint32_t* n_groups, const uint32_t** group_sizes,
                               const vs_allele_counts** counts);
/* The records as they lie in HBM: n_rows x n_groups records of 16 bytes, row-major, valid until vs_result_free.  The engine has
 * synchronised its stream when this returns: the caller needs no event. */
int vs_result_group_counts_device(vs_result* r, uint64_t* n_rows, uint32_t* n_groups, const void** dev_counts);
/* Window statistics: the grouped counts above reduced on the GPU per REGION and group, and per pair of groups, to the exact integers
 * that nucleotide diversity pi, segregating sites, Watterson's theta, Tajima's D, dxy, Hudson's Fst, private alleles and fixed
 * differences are formed from -- what `vcftools --window-pi / --TajimaD / --weir-fst-pop` or scikit-allel's windowed_* compute per
 * window (no reference counterpart: what a caller would reduce on the host from vs_query_group_counts' rows x n_groups x 16 bytes).
 * The arguments, their checks and the order of the checks are vs_query_group_counts's (the cohort limit of 32768 sample ids and
 * argument errors before VS_ERR_NO_DEVICE included), with two additions: sample_ids == NULL with n_groups == 1 stands for the whole
 * cohort as one group (group_of and n_ids are then ignored), and with_pairs may be 0 or 1 only (VS_ERR_ARG, checked right behind the
 * range of n_groups).
 * For every region q, in the caller's order, and every group g there is one vs_window_stats record, stats[q * n_groups + g], over
 * the rows region q reports; a row the duplicate rule dropped is not a site and adds to nothing, `rows` included.  With `ac` a row's
 * alt_alleles in g, N_g = 2 x group_size[g] and het = carriers - hom_alt in g: rows (reported, non-dropped rows, the same for every
 * group), seg (0 < ac < N_g), singletons (ac == 1), doubletons (ac == 2), private_alleles (ac > 0 and no alternate allele in any
 * other group; one group: ac > 0), fixed (N_g > 0 and ac == N_g), sum_ac, sum_ac2 (the sums of ac and ac^2) and obs_het (the sum of
 * het).  With with_pairs every pair g < h adds one vs_window_pair_stats record, pair_stats[q * n_pairs + p], the pairs in the order
 * (0,1), (0,2), ..., (n_groups-2, n_groups-1), n_pairs = n_groups (n_groups - 1) / 2 (at most 2016): sum_cross (the sum of
 * ac_g x ac_h), seg_union (0 < ac_g + ac_h < N_g + N_h) and fixed_diff (both groups have members and one has ac == 0 while the
 * other has ac == N).
 * N_g is two allele copies per sample whatever the call's ploidy, as the GRM's 2n is; a multi-allelic site's ALT rows are separate
 * sites with the index's genotype bits (a `1|2` call counts on both ALT rows), as in every column query here.
 * The device sums integers only (ac <= 65534, so every product is below 2^32 and no 64-bit sum can overflow): the same call gives
 * the same bytes.  pi, theta, Tajima's D, dxy and Fst are the caller's to form from them (the Python accessor and the command line do).
 * The temporary rows x n_groups x 16 bytes and the n x (48 n_groups + 16 n_pairs) bytes of the answer together are held to option
 * "matrix_max_mib": a larger request is refused with VS_ERR_ARG once the plan has given the rows and before anything is allocated.
 * A region of more than option "window_chunk" rows is split between workgroups that add with integer atomics (same bytes).
 * Every batch size takes the batch pipeline; the batch is never speculative and leaves the handle's type-6 state as it was.  The
 * result holds the type-6 per-region arrays and variant table, no carrier arena, and the records: vs_result_get_raw /
 * vs_result_get_view with with_carriers = 0, vs_result_layout (arena and lists 0), vs_result_fill_ms (the group kernel and the
 * reduction, between the result's own pair of events), vs_result_totals (n_carriers as for a grouped-count result) and
 * vs_result_format_region work -- integers only: "Group\tN\tRows\tSeg\tSingletons\tDoubletons\tPrivate\tFixed\tSumAC\tSumAC2\tObsHet\n",
 * one line per group (Group is the group's name, or its decimal index without names; N its size in samples), then, when there are
 * pair records, "GroupA\tGroupB\tSumCross\tSegUnion\tFixedDiff\n" and one line per pair --; with_carriers = 1, vs_result_digest,
 * vs_result_pack_headers / _pack_regions and vs_comm_allgather_regions* fail with VS_ERR_UNSUPPORTED, the other kinds' getters with
 * VS_ERR_ARG. */
typedef struct vs_window_stats {
  uint32_t rows, seg, singletons, doubletons, private_alleles, fixed;
  uint64_t sum_ac, sum_ac2, obs_het;
} vs_window_stats;
typedef struct vs_window_pair_stats {
  uint64_t sum_cross;
  uint32_t seg_union, fixed_diff;
} vs_window_pair_stats;
int vs_query_window_stats(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, const uint32_t* group_of,
                          uint64_t n_ids, uint32_t n_groups, const char* const* group_names, uint32_t with_pairs, vs_result** out);
/* The records of a window-statistics result copied into page-locked memory owned by the result: stats[q * n_groups + g],
 * pair_stats[q * n_pairs + p] (NULL without pair records), group_sizes[g] the number of distinct samples of group g, group_names the
 * n_groups names (NULL when none were given).  Any may be NULL but `stats`.  VS_ERR_ARG on any other result. */
int vs_result_get_window_stats(vs_result* r, uint64_t* n_regions, uint32_t* n_groups, uint32_t* n_pairs, const uint32_t** group_sizes,
                               const char* const** group_names, const vs_window_stats** stats, const vs_window_pair_stats** pair_stats);
/* The records as they lie in HBM: n_regions x n_groups records of 48 bytes, and n_regions x n_pairs pair records of 16 bytes (NULL
 * without), valid until vs_result_free.  The engine has synchronised its stream when this returns: the caller needs no event. */
int vs_result_window_stats_device(vs_result* r, uint64_t* n_regions, uint32_t* n_groups, uint32_t* n_pairs, const void** dev_stats,
                                  const void** dev_pair_stats);
/* Association scan: every row of the type-6 variant table scored against K phenotypes in one pass over its carriers -- "for the
 * variants in these regions, how does each one go with this trait?" (no reference counterpart: what a caller would get from
 * vs_query_genotype_matrix, a conversion of the cells to dosages and a matrix product, without the matrix).
 * The subset S and its n_cols = n columns are the genotype matrix's: the distinct sample ids ascending; sample_ids == NULL: the whole
 * cohort, ids 1 .. num_samples - 1, and n_ids must be num_samples - 1.  traits[i * n_traits + k] (HOST float32, n_ids x n_traits) is
 * trait k of sample_ids[i], in whatever order the ids come (NULL ids: of id i + 1); the engine permutes the rows into column order.
 * d_i(s) = popc(gt & 6) is the dosage of sample s on table row i: 0 for a non-carrier and on a row dropped by the duplicate rule.
 * scores[i * n_traits + k], a float64, is
 *   VS_ASSOC_DOT   Sxy = sum over s in S of d_i(s) * y_k(s), accumulated in float64 (every product is exact);
 *   VS_ASSOC_CHI2  the score test of a linear regression of y_k on the dosage without covariates (for a 0/1 trait the
 *                  Cochran-Armitage trend test): with the row's own count record over S, Sx = alt_alleles, Sxx = alt_alleles +
 *                  2 hom_alt, vx = n Sxx - Sx^2 in 64-bit integers, cov = n Sxy - Sx Sy and vy = n Syy - Sy^2 in double,
 *                  chi2 = ((double)n * cov) * cov / ((double)vx * vy), each operation rounded on its own in this order; 0.0 when
 *                  vx == 0 or vy <= 0 (a monomorphic or dropped row, a constant trait, n = 1).  Sxy, Sy and Syy of this formula
 *                  are taken about a pivot, over y_k(s) - c_k in double: c_k is the value of trait k nearest its mean over S (the
 *                  first of equally near ones).  The statistic does not change with c_k; the cancellations in cov and vy then
 *                  happen at the scale of the trait's spread, not of its mean, and integer-valued traits keep integer sums.
 * The order of a row's additions is fixed by the table's layout, not by the run: the same call gives the same bytes every time,
 * whichever form the phenotype table takes on the device (option "assoc_lds_max_kib").  The result also holds the count record of
 * every table row over S (vs_allele_counts, as an LD result does), per trait Sy and Syy as doubles -- summed on the host left to right
 * in column order from the float32 values --, and the columns' ids.  A batch whose table is empty gives 0 rows and is no error.
 * `regions` as for vs_query_allele_counts (host or device memory, n >= 1).  Checked on the host before the handle's device is asked
 * for (a handle opened without a device reports them first and VS_ERR_NO_DEVICE otherwise): n == 0, NULL traits, n_traits == 0 or
 * n_traits > VS_TRAITS_MAX, an unknown stat, n_ids == 0, NULL sample_ids with n_ids != num_samples - 1 -> VS_ERR_ARG; id 0 ("ref") or
 * an id >= num_samples -> VS_ERR_UNKNOWN_SAMPLE; a sample listed twice -> VS_ERR_ARG (the message names the id); a value that is not
 * finite -> VS_ERR_ARG (the message names the sample id and the trait: pass the subset of samples that have a value); a trait name
 * (trait_names: NULL, or n_traits strings that are copied into the result) with a tab or a newline -> VS_ERR_ARG.  The whole cohort
 * has no size limit; a subset's bit mask lies in the counting kernel's LDS as for vs_query_allele_counts (more than 393216 sample
 * ids: VS_ERR_UNSUPPORTED).
 * rows x n_traits x 8 + rows x 16 bytes are held to option "matrix_max_mib" (default 32 GiB): a larger request is refused with
 * VS_ERR_ARG once the plan has given the rows and before anything is allocated; the message names rows, traits and bytes.
 * Every batch size takes the batch pipeline; an association batch is never speculative and leaves the handle's type-6 state as it
 * was.  The result holds the type-6 per-region arrays and variant table, no carrier arena: vs_result_get_raw / vs_result_get_view
 * with with_carriers = 0, vs_result_layout (arena and lists 0), vs_result_fill_ms (the count kernel and the scan), vs_result_totals
 * (n_carriers = the sum of `carriers` over the rows every region reports) and vs_result_format_region
 * ("Pos\tRef\tAlt\tCarriers\tAC\tHomAlt\tPhased", then a column per trait under its name, or its decimal index without names; one
 * line per reported, non-dropped row, the cells printed with %.17g) work; with_carriers = 1, vs_result_digest, vs_result_pack_headers /
 * _pack_regions and vs_comm_allgather_regions* fail with VS_ERR_UNSUPPORTED, the other kinds' getters with VS_ERR_ARG. */
#define VS_TRAITS_MAX 8u
#define VS_ASSOC_DOT 0u
#define VS_ASSOC_CHI2 1u
int vs_query_assoc_scan(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids,
                        const float* traits, uint32_t n_traits, uint32_t stat, const char* const* trait_names, vs_result** out);
/* The cells of an association-scan result copied into page-locked memory owned by the result: scores[i * n_traits + k] of table row
 * i (vs_result_raw.rows[i]; region q's rows are row_begin[q] .. + row_count[q]); counts[i] its record over S; trait_sum / trait_sumsq
 * n_traits doubles each; col_ids the n_cols column ids (any but `scores` may be NULL).  VS_ERR_ARG on any other result. */
int vs_result_get_assoc_scan(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* n_traits, uint32_t* stat,
                             const uint32_t** col_ids, const double** trait_sum, const double** trait_sumsq,
                             const vs_allele_counts** counts, const double** scores);
/* The cells as they lie in HBM: n_rows x n_traits float64, row-major, and the n_rows count records of 16 bytes (dev_counts may be
 * NULL), valid until vs_result_free.  The engine has synchronised its stream when this returns: the caller needs no event. */
int vs_result_assoc_scan_device(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* n_traits, uint32_t* stat,
                                const void** dev_counts, const void** dev_scores);
/* Trait-matrix association scan: every row of the type-6 variant table against a WIDE panel of K traits, 1 <= K <=
 * VS_TRAIT_MATRIX_MAX -- eQTL windows against every expressed gene, a variant set against every phenotype of a biobank, K shuffled
 * copies of one trait -- as the product of the dosage matrix with the panel on the matrix cores (no reference counterpart).
 * regions, sample_ids / n_ids, traits (HOST float32, n_ids x n_traits, in the order of the ids), the subset S, its n columns, the
 * dosage, dropped rows, trait_names, the argument rules and their error codes are vs_query_assoc_scan's, with VS_TRAIT_MATRIX_MAX in
 * place of VS_TRAITS_MAX; the checks come in that call's order and before the handle's device is asked for.  n must stay below 2^22
 * (VS_ERR_UNSUPPORTED).
 * Fixed point: per trait k, M_k = max |y| = m 2^e (frexp, 0.5 <= m < 1), f_k = 30 - e (0 for a column of zeros), q_k(s) =
 * rint(y 2^f_k), ties to even: |q| < 2^30.  (vs_assoc_matrix_quantise gives q and f.)  scores[i * n_traits + k], a float64, is
 *   VS_ASSOC_DOT   ldexp((double)S, -f_k), S = sum over s in S of d_i(s) q_k(s), an exact integer with |S| <= 2^53: the caller
 *                  gets it back as ldexp(score, f_k);
 *   VS_ASSOC_CHI2  the score test of vs_query_assoc_scan from exact integers: vx = n Sxx - Sx^2 (64 bits), Sy = sum q, Syy = sum q^2,
 *                  vy = n Syy - Sy^2 and cov = n S - Sx Sy in 128 bits, each converted to double once, chi2 = (((double)n * cov) *
 *                  cov) / ((double)vx * vy) in this order without contraction; 0.0 when vx == 0 or vy <= 0.  2^f_k cancels.
 * No floating-point value is ever summed: the same call gives the same bytes.  The result also holds f_k (shift), the exact trait
 * sums as doubles (trait_sum = ldexp(Sy, -f_k), trait_sumsq = ldexp(Syy, -2 f_k)), the rows' count records over S and the column ids.
 * The temporary genotype matrix (rows x pitch, pitch = n rounded up to 16), the cells (rows x n_traits x 8), the count records
 * (rows x 16) and the limb panel (ceil(n_traits / 16) x 64 x pitch) together are held to option "matrix_max_mib": a larger request
 * is refused with VS_ERR_ARG before anything is allocated; the message gives rows, columns, traits, the total and the parts in bytes.
 * Never speculative; the handle's type-6 state stays as it was.  What works on the result and what is refused is an
 * association-scan result's (vs_result_format_region gives its text with K score columns), with the accessors below in place of
 * vs_result_get_assoc_scan / _device; those two and the other kinds' getters answer VS_ERR_ARG here, these two on any other result. */
#define VS_TRAIT_MATRIX_MAX 65536u
int vs_query_assoc_matrix(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids,
                          const float* traits, uint32_t n_traits, uint32_t stat, const char* const* trait_names, vs_result** out);
/* Host copies, owned by the result: scores[i * n_traits + k], counts[i], col_ids, shift / trait_sum / trait_sumsq (n_traits each);
 * any but `scores` may be NULL. */
int vs_result_get_assoc_matrix(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* n_traits, uint32_t* stat,
                               const uint32_t** col_ids, const int32_t** shift, const double** trait_sum, const double** trait_sumsq,
                               const vs_allele_counts** counts, const double** scores);
/* The cells as they lie in HBM: n_rows x n_traits float64, row-major, and the n_rows count records of 16 bytes (dev_counts may be
 * NULL), valid until vs_result_free.  The engine has synchronised its stream when this returns. */
int vs_result_assoc_matrix_device(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* n_traits, uint32_t* stat,
                                  const void** dev_counts, const void** dev_scores);
/* The engine's own quantiser, the one vs_query_assoc_matrix calls; host-only, needs no handle.  traits: n x n_traits float32,
 * row-major; q_out: n x n_traits int32; shift_out: n_traits int32.  VS_ERR_ARG on NULL, n == 0, n_traits == 0 or a value that is
 * not finite. */
int vs_assoc_matrix_quantise(const float* traits, uint64_t n, uint32_t n_traits, int32_t* q_out, int32_t* shift_out);
/* Per-sample scores: samples x K weighted dosage sums over the rows a batch reports -- "what is each sample's polygenic score under
 * this score file?", the projection of the samples onto K loadings, the second half of a matrix-free iteration on the genotype matrix
 * (vs_query_assoc_scan gives G Y: every row against K per-sample vectors; this gives G^T W: every sample against K per-variant
 * weights).  No reference counterpart: what a caller would get from vs_query_genotype_matrix and a matrix product, without the matrix.
 * `regions`, the subset S, its n_cols = n columns (the distinct ids ascending; sample_ids == NULL: the whole cohort, ids 1 ..
 * num_samples - 1, and n_ids must be num_samples - 1) and the dosage d = popc(gt & 6) are vs_query_assoc_scan's.
 * Weights are keyed by REPORT ORDER.  rep[q] is the number of rows region q reports: the table rows row_begin[q] .. + row_count[q]
 * whose dropped flag is clear -- the data lines of vs_result_format_region(q), and of the reference's type-6 text.  off[q] is the
 * exclusive prefix sum of rep in the caller's region order, N the sum of rep.  `weights` is N x n_scores float32, row-major,
 * 1 <= n_scores <= VS_SCORES_MAX, in host or device memory (told apart as the regions are); entry off[q] + j belongs to the j-th row
 * region q reports.  A row that several regions report takes part once per report, with that report's weight (the burden's rule).
 * (Weights cannot be keyed by table row: the private rows of two batches over the same regions need not lie alike.)
 * The sums are taken in 64-bit fixed point, so that the same call gives the same bytes.  Per column k: M_k = max |w| over its N values;
 * M_k == 0: f_k = 0; else M_k = m 2^e with 0.5 <= m < 1 (frexp) and f_k = 36 - e.  q = rint((double)w 2^f_k), ties to even, so
 * |q| <= 2^36.  sums[c * n_scores + k] = the sum over the reports of d(row, column c) q, an int64, exact whatever the order.
 * scores[c * n_scores + k] = ldexp((double)sums[c * n_scores + k], -f_k).  Weights with |w| >= 2^-12 M_k are represented exactly; any
 * term is off by at most d 2^(e - 37).
 * Refused, beside everything vs_query_assoc_scan refuses about regions and ids: n_scores outside 1 .. VS_SCORES_MAX -> VS_ERR_ARG; a
 * weight that is not finite -> VS_ERR_ARG, the message names the column (host weights are checked on the host before the device is
 * asked for, device weights by the scale kernel); n_weights != N -> VS_ERR_ARG, the message names both numbers, once the plan has
 * given rep and before anything further is allocated; N >= 2^26 -> VS_ERR_ARG (below that |sum| <= 2 N 2^36 < 2^63); a score name
 * (score_names: NULL, or n_scores strings that are copied) with a tab or a newline -> VS_ERR_ARG.  The uploaded weights, the integer
 * weights per table row (rows x Kp x 8 bytes, Kp = n_scores rounded up to 1, 2, 4 or 8, + 4 bytes a row) and the sums and scores are
 * held to option "matrix_max_mib": VS_ERR_ARG.  A handle opened without a device reports the host's checks first and
 * VS_ERR_NO_DEVICE otherwise.  A batch whose table is empty gives all-zero scores over the n columns and is no error.
 * Every batch size takes the batch pipeline; a score batch is never speculative and leaves the handle's type-6 state as it was.  The
 * result holds the type-6 per-region arrays and variant table, no carrier arena, as an association result does: vs_result_fill_ms is
 * the new kernels' own pair of events, vs_result_totals' n_carriers the number of (report, carrier in S) pairs whose report has a
 * weight that is not zero after quantisation, vs_result_format_region the region's reported rows ("Pos\tRef\tAlt", a line per row:
 * the rows of the type-6 text without their carriers, which no arena holds).  The other kinds' getters fail with VS_ERR_ARG. */
#define VS_SCORES_MAX 8u
int vs_query_sample_scores(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids,
                           const float* weights, uint64_t n_weights, uint32_t n_scores, const char* const* score_names, vs_result** out);
/* The cells of a score result copied into page-locked memory owned by the result: sums and scores [n_cols x n_scores], shift the
 * n_scores values f_k, col_ids the n_cols column ids (any may be NULL but not both sums and scores).  VS_ERR_ARG on any other result. */
int vs_result_get_sample_scores(vs_result* r, uint64_t* n_cols, uint32_t* n_scores, const uint32_t** col_ids, const int32_t** shift,
                                const int64_t** sums, const double** scores);
/* The cells as they lie in HBM: n_cols x n_scores int64 sums and float64 scores, row-major (dev_sums may be NULL), valid until
 * vs_result_free.  The engine has synchronised its stream when this returns: the caller needs no event. */
int vs_result_sample_scores_device(vs_result* r, uint64_t* n_cols, uint32_t* n_scores, const void** dev_sums, const void** dev_scores);
/* Score matrix: vs_query_sample_scores for a WIDE panel of weight columns, 1 <= n_scores <= VS_SCORE_MATRIX_MAX -- a cohort against
 * dozens of polygenic score files, a projection onto PCA loadings, the second half of a randomised-SVD step on the vectors
 * vs_query_assoc_matrix produced -- as the product D^T W of the dosage matrix with the weights on the matrix cores (no reference
 * counterpart).  regions, the subset S and its n columns, the dosage, dropped rows, score_names and the report-keyed `weights`
 * (n_weights x n_scores float32, row-major, entry off[q] + j for the j-th row region q reports; a shared row takes part once per
 * report with that report's weight) are vs_query_sample_scores'.  The weights are in HOST memory.
 * Fixed point is the trait quantiser's (vs_assoc_matrix_quantise over the N x n_scores weights gives q and f): per column k, M_k =
 * max |w| = m 2^e (frexp), f_k = 30 - e (0 for a column of zeros), q = rint((double)w 2^f_k), ties to even, |q| < 2^30.
 * sums[c * n_scores + k] = the sum over the reports of d(row(report), column c) q_k(report), an exact int64 (|sum| <= 2 x 2^30 x N
 * < 2^57); scores[c * n_scores + k] = ldexp((double)sums, -f_k), one rounding.  No floating-point value is summed: the same call
 * gives the same bytes under every option setting, with or without share_lists.  Any term is off by at most d 2^(e - 31).
 * The kernel multiplies by the per-row totals T[row][k] = the sum of q_k over the row's reports, split into balanced base-256 int8
 * limbs: four hold |T| <= 2,139,062,143 (every batch in which no row is reported twice), five up to 547,599,908,735; the engine
 * runs four where the batch's largest |T| allows it, else five, and the result records which (limbs).  |T| > 2^38 -- more than 256
 * regions reporting one row -- is refused with VS_ERR_UNSUPPORTED: split the batch.
 * Refused on the host, in this order, before the handle's device is asked for: n_scores outside 1 .. VS_SCORE_MATRIX_MAX ->
 * VS_ERR_ARG; a weight that is not finite -> VS_ERR_ARG, the message names the column; a score name with a tab or a newline ->
 * VS_ERR_ARG; ids as vs_query_sample_scores refuses them (none, an id twice -> VS_ERR_ARG; id 0 or beyond the cohort ->
 * VS_ERR_UNKNOWN_SAMPLE); n_weights >= 2^26 -> VS_ERR_ARG.  A handle opened without a device reports these first and
 * VS_ERR_NO_DEVICE otherwise.  Then, after the plan's one host wait: n_weights != N -> VS_ERR_ARG, the message gives both numbers;
 * N >= 2^26 -> VS_ERR_ARG; and the batch's buffers -- the temporary genotype matrix (rows x pitch, pitch = n rounded up to 16), the
 * uploaded weights (N x n_scores x 4), T (rows x n_scores x 8), the limb panel (ceil(n_scores / 16) x 16 x 5 x rows rounded up to
 * 128: it is laid out for five limbs) and the sums and scores (n x n_scores x 16) -- together are held to option "matrix_max_mib":
 * a larger request is refused with VS_ERR_ARG before anything of it is allocated; the message gives the parts in bytes.
 * A batch whose table is empty gives all-zero cells and is no error.  Never speculative; the handle's type-6 state stays as it
 * was.  The result is a score result in everything else (per-region arrays and variant table, no arena, vs_result_format_region's
 * "Pos\tRef\tAlt" lines, vs_result_fill_ms its own pair of events), but vs_result_totals' n_carriers is what a Gram result
 * reports: the nonzero cells of the temporary matrix.  The two accessors below answer VS_ERR_ARG on every other kind of result;
 * every other kind's getter, vs_result_get_sample_scores included, answers VS_ERR_ARG on this one. */
#define VS_SCORE_MATRIX_MAX 65536u
int vs_query_score_matrix(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids,
                          const float* weights, uint64_t n_weights, uint32_t n_scores, const char* const* score_names, vs_result** out);
/* Host copies in page-locked memory owned by the result: sums and scores [n_cols x n_scores], shift the n_scores values f_k, limbs
 * (4 or 5), col_ids the n_cols column ids (any may be NULL but not both sums and scores). */
int vs_result_get_score_matrix(vs_result* r, uint64_t* n_cols, uint32_t* n_scores, const uint32_t** col_ids, const int32_t** shift,
                               uint32_t* limbs, const int64_t** sums, const double** scores);
/* The cells as they lie in HBM: n_cols x n_scores int64 sums and float64 scores, row-major (dev_sums may be NULL), valid until
 * vs_result_free.  The engine has synchronised its stream when this returns: the caller needs no event. */
int vs_result_score_matrix_device(vs_result* r, uint64_t* n_cols, uint32_t* n_scores, const void** dev_sums, const void** dev_scores);
/* Per-sample burden over regions: the counts above along the other axis -- a regions x samples matrix, the input of gene-burden
 * and collapsing tests and of per-sample QC counts (no reference counterpart: what a caller of type 6 would reduce on the host
 * from every carrier list).  Let R(q) be the rows type 6 reports for region q (same order, duplicate rule and region flags; a
 * dropped row is not in R(q)) and ac_S(row) the alt_alleles vs_query_allele_counts reports for the row over the same S.  A row
 * COUNTS iff min_ac <= ac_S(row) <= max_ac (0 and UINT32_MAX: every reported row counts).  Cell (q, c), over the counting rows
 * of R(q) of which column c's sample is a carrier (genotype bits as for vs_allele_counts: a `1|2` call gives 2 on both of its
 * ALT rows, a haploid `1` is gt_1 alone):
 *   variants    = number of such rows
 *   alt_alleles = sum of gt_1 + gt_2
 *   hom_alt     = number with gt_1 && gt_2
 *   phased      = number with the phase bit */
typedef struct { uint32_t variants, alt_alleles, hom_alt, phased; } vs_sample_burden;   /* 16 bytes, one cell */
/* `regions` as for vs_query_allele_counts (host or device memory, n >= 1); `sample_ids` NULL (the whole cohort) or a HOST array of
 * n_ids >= 1 ids.  The COLUMNS are the distinct ids of S in ascending id order (duplicates collapse); with S == NULL they are the
 * ids 1 .. num_samples - 1 ("ref", id 0, is never a column).  The matrix's rows are the regions in the caller's order, whether or
 * not the device sorted the batch.  Checked on the host, in this order, before the handle's device is asked for (a handle opened
 * without a device reports them first and VS_ERR_NO_DEVICE otherwise): n == 0, sample_ids == NULL with n_ids != 0, non-NULL
 * sample_ids with n_ids == 0, min_ac > max_ac -> VS_ERR_ARG; id 0 or id >= num_samples -> VS_ERR_UNKNOWN_SAMPLE; a matrix of more
 * than 2^31 cells (n x columns; 32 GiB) -> VS_ERR_ARG: a condition of this interface, callers split larger batches.  An
 * allocation failure below that limit is VS_ERR_HIP.
 * Every batch size takes the batch pipeline, as count batches do; a burden batch is never speculative and leaves the handle's
 * type-6 state as it was.  The result holds the type-6 per-region arrays and variant table, no carrier arena, and the matrix:
 * vs_result_get_raw / vs_result_get_view with with_carriers = 0, vs_result_layout (arena and lists 0), vs_result_fill_ms (the
 * burden kernels, the window's count kernel included), vs_result_totals (n_regions, n_var as for type 6; n_carriers = the sum
 * of `variants` over the matrix, reduced on the device: with the default window the count result's n_carriers for the same S)
 * and vs_result_format_region ("Sample\tVariants\tAC\tHomAlt\tPhased\n", then one line per column with variants > 0, in column
 * order, by sample name) work; with_carriers = 1, vs_result_digest, vs_result_pack_headers / _pack_regions and
 * vs_comm_allgather_regions* fail with VS_ERR_UNSUPPORTED, vs_result_get_allele_counts with VS_ERR_ARG.
 * Option "burden_chunk" (vs_index_set_option; 0 = default, 64..65536): the rows of a region one workgroup walks before the region
 * is split between several. */
int vs_query_sample_burden(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids,
                           uint32_t min_ac, uint32_t max_ac, vs_result** out);
/* The matrix of a burden result copied into page-locked memory owned by the result: cells[q * n_cols + c], col_ids[c] the sample
 * id of column c.  VS_ERR_ARG on any other result. */
int vs_result_get_sample_burden(vs_result* r, uint64_t* n_regions, uint64_t* n_cols, const uint32_t** col_ids,
                                const vs_sample_burden** cells);
/* The matrix as it lies in HBM: n_regions x n_cols cells of 16 bytes, row-major, valid until vs_result_free.  The engine has
 * synchronised its stream when this returns: the caller needs no event. */
int vs_result_sample_burden_device(vs_result* r, uint64_t* n_regions, uint64_t* n_cols, const void** dev_cells);
/* The genotype matrix over regions: the object the two queries above reduce -- for the variants of a set of regions every sample's
 * call as a dense byte matrix, the input of LD / r^2, PCA / GRM and association tests (no reference counterpart: what a caller of
 * type 6 would scatter on the host from every carrier list).  Let T be the variant table a type-6 batch over `regions` produces
 * (the shared rows in site order, behind them the private rows of the regions under the duplicate rule; region q's rows are
 * row_begin[q] .. row_begin[q] + row_count[q] of vs_result_get_raw).  The matrix has one ROW per row of T and one COLUMN per
 * sample of S: the distinct ids of `sample_ids` in ascending order (a HOST array of n_ids >= 1 ids, duplicates collapse), or with
 * sample_ids == NULL the ids 1 .. num_samples - 1 ("ref", id 0, is never a column).  Cell (i, c):
 *   0           column c's sample is not a carrier of row i, or row i was dropped by the duplicate rule
 *   0x08 | gt   it is a carrier; gt = the index's three genotype bits as type 6's arena holds them (bit 0 phase, bit 1 gt_1,
 *               bit 2 gt_2: what vs_allele_counts and vs_sample_burden sum).  The dosage is popcount(cell & 6); a `1|2` call shows
 *               on both of its ALT rows, a haploid `1` is gt_1 alone.
 * The matrix is row-major, rows row_pitch bytes apart: the columns rounded up to a multiple of 16; padding bytes are 0.  A batch
 * whose table is empty gives 0 rows and is no error.
 * `regions` as for vs_query_allele_counts (host or device memory, n >= 1).  Checked on the host, in this order, before the handle's
 * device is asked for (a handle opened without a device reports them first and VS_ERR_NO_DEVICE otherwise): n == 0, sample_ids ==
 * NULL with n_ids != 0, non-NULL sample_ids with n_ids == 0 -> VS_ERR_ARG; id 0 or id >= num_samples -> VS_ERR_UNKNOWN_SAMPLE.
 * A matrix (rows x row_pitch) of more than option "matrix_max_mib" MiB (default 32 GiB) is refused with VS_ERR_ARG once the plan
 * has given the rows and before anything is allocated for it; the message names rows, columns and bytes.  An allocation failure
 * below the limit is VS_ERR_HIP.
 * Every batch size takes the batch pipeline, as count batches do; a matrix batch is never speculative and leaves the handle's
 * type-6 state as it was.  The result holds the type-6 per-region arrays and variant table, no carrier arena, and the matrix:
 * vs_result_get_raw / vs_result_get_view with with_carriers = 0, vs_result_layout (arena and lists 0), vs_result_fill_ms (the
 * matrix kernel), vs_result_totals (n_regions, n_var as for type 6; n_carriers = the nonzero cells of the matrix, counted on the
 * device: every table row once -- the count result's n_carriers for the same S when no two regions report the same row) and vs_result_format_region ("Pos\tRef\tAlt" and "\t<sample name>" per
 * column, then per reported row of the region -- dropped rows left out -- Pos, Ref, Alt as type 6 prints them and per column `0`
 * for a non-carrier, else gt_1, `|` under the phase bit or `/`, gt_2) work; with_carriers = 1, vs_result_digest,
 * vs_result_pack_headers / _pack_regions and vs_comm_allgather_regions* fail with VS_ERR_UNSUPPORTED, vs_result_get_allele_counts
 * and vs_result_get_sample_burden with VS_ERR_ARG. */
int vs_query_genotype_matrix(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids,
                             vs_result** out);
/* The matrix of a genotype-matrix result copied into page-locked memory owned by the result: cells[i * row_pitch + c], col_ids[c]
 * the sample id of column c.  VS_ERR_ARG on any other result. */
int vs_result_get_genotype_matrix(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint64_t* row_pitch, const uint32_t** col_ids,
                                  const uint8_t** cells);
/* The matrix as it lies in HBM: n_rows rows of row_pitch bytes, valid until vs_result_free.  The engine has synchronised its
 * stream when this returns: the caller needs no event. */
int vs_result_genotype_matrix_device(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint64_t* row_pitch, const void** dev_cells);
/* Banded LD over regions: the step behind the genotype matrix -- every row of the variant table against the next `window` rows, the
 * input of pruning, clumping, fine-mapping windows and haplotype-block calls (no reference counterpart).  T, its rows, S and its
 * n columns are those of vs_query_genotype_matrix over the same regions and sample_ids; A is the number of rows of T.  The dosage
 * of a cell is d = popcount(cell & 6) of the genotype-matrix cell: 0 for a non-carrier and everywhere on a row the duplicate rule
 * dropped.  The answer is a band of A x window four-byte cells, band[i * window + k] for the pair of table rows (i, j = i + 1 + k):
 *   VS_LD_DOT   int32   Sxy = sum over the columns s of d_i(s) * d_j(s), exact
 *   VS_LD_R2    float   the squared dosage correlation from exact integers: with Sx = sum d = the row's alt_alleles over S and
 *                       Sxx = sum d^2 = alt_alleles + 2 hom_alt, in 64-bit integers cov = n Sxy - Sx Sy, vx = n Sxx - Sx^2,
 *                       vy = n Syy - Sy^2, then r2 = (float)((double)cov * (double)cov / ((double)vx * (double)vy)), and 0.0f when
 *                       vx == 0 or vy == 0 (a monomorphic row, a dropped row, n = 1)
 * Pairs are taken by table index and nothing else: a pair with i + 1 + k >= A is 0, a pair that straddles the end of the shared
 * rows is computed like any other; region q's pairs are those inside row_begin[q] .. row_begin[q] + row_count[q].  Every cell of
 * the band is stored exactly once by the kernel, zeros included.  The result also carries the count record of every table row over
 * S (vs_allele_counts, what vs_query_allele_counts reports): the r2 was formed from it, and it turns a DOT band into covariance, D
 * or r.
 * `regions` and `sample_ids` as for vs_query_genotype_matrix.  Checked on the host, in this order, before the handle's device is
 * asked for (a handle opened without a device reports them first and VS_ERR_NO_DEVICE otherwise): n == 0, sample_ids == NULL with
 * n_ids != 0, non-NULL sample_ids with n_ids == 0, window == 0 or window > 256, stat neither VS_LD_DOT nor VS_LD_R2 -> VS_ERR_ARG;
 * id 0 or id >= num_samples -> VS_ERR_UNKNOWN_SAMPLE.  The band is formed from a temporary genotype matrix (rows x row_pitch
 * bytes; it is not part of the result: it goes back to the handle's pool at the end of the call or, where the call returns with
 * its kernels enqueued -- option "async_submit", the default --, as soon as an accessor or vs_result_free has waited for them, the
 * result still open); matrix and band together may not exceed option
 * "matrix_max_mib" MiB (default 32 GiB): beyond it the call is refused with VS_ERR_ARG once the plan has given the rows and before
 * anything is allocated; the message names rows, columns, window and bytes.
 * Every batch size takes the batch pipeline; an LD batch is never speculative and leaves the handle's type-6 state as it was.  The
 * result holds the type-6 per-region arrays and variant table, no carrier arena, the counts and the band: vs_result_get_raw /
 * vs_result_get_view with with_carriers = 0, vs_result_layout (arena and lists 0), vs_result_fill_ms (the batch's own kernels: the
 * counts, the temporary matrix and the band kernel), vs_result_totals (n_carriers = the nonzero cells of the matrix, as for the
 * matrix query) and vs_result_format_region ("PosA\tRefA\tAltA\tPosB\tRefB\tAltB\t" + "Dot" or "R2", then one line for every pair
 * a < b of the region's reported, non-dropped rows whose table indices are at most `window` apart, the value as %d or %.6g) work;
 * with_carriers = 1, vs_result_digest, vs_result_pack_headers / _pack_regions and vs_comm_allgather_regions* fail with
 * VS_ERR_UNSUPPORTED, vs_result_get_allele_counts, vs_result_get_sample_burden and vs_result_get_genotype_matrix with VS_ERR_ARG. */
#define VS_LD_DOT 0u
#define VS_LD_R2 1u
int vs_query_ld_band(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, uint32_t window,
                     uint32_t stat, vs_result** out);
/* The band of an LD result copied into page-locked memory owned by the result: band[i * window + k] (int32 under VS_LD_DOT, float
 * under VS_LD_R2: `stat` says which), counts[i] the count record of table row i over S, col_ids[c] the sample id of column c.
 * Every out-pointer but `band` may be NULL.  VS_ERR_ARG on any other result. */
int vs_result_get_ld_band(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* window, uint32_t* stat, const uint32_t** col_ids,
                          const vs_allele_counts** counts, const void** band);
/* Band and counts as they lie in HBM (n_rows x window cells of 4 bytes; n_rows records of 16 bytes), valid until vs_result_free.
 * The engine has synchronised its stream when this returns: the caller needs no event. */
int vs_result_ld_band_device(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* window, uint32_t* stat, const void** dev_counts,
                             const void** dev_band);
/* LD matrices over regions: the complete square block of every region where vs_query_ld_band gives a band of the whole table -- the
 * input of fine-mapping, conditional analysis, LD scores and "LD with the lead variant" plots (no reference counterpart).  T, its A
 * rows, S and its n columns are those of vs_query_genotype_matrix over the same regions and sample_ids.  Region q owns the table
 * rows row_begin[q] .. row_begin[q] + m_q, m_q = row_count[q] (vs_result_get_raw); its block is m_q x m_q four-byte cells,
 * cells[block_begin[q] + a * m_q + b] for the pair of table rows (row_begin[q] + a, row_begin[q] + b): the full symmetric square,
 * diagonal included.  block_begin is the exclusive scan of m_q^2 in uint64, block_begin[n] the number of cells.  Blocks go by table
 * index and nothing else: overlapping or identical regions each get their own block over the shared rows, a row the duplicate rule
 * dropped stays in the block as a row and a column of zeros, an empty region has an empty block.  The cells are the band's, by the
 * same definition: VS_LD_DOT stores int32 Sxy (the diagonal is Sxx), VS_LD_R2 the float r2 formed from the count records in 64-bit
 * integers, 0.0f where vx == 0 or vy == 0 (the diagonal of a polymorphic row is exactly 1.0f).  Every cell of every block is stored
 * exactly once by the kernel.  The result carries the count record of every table row over S, as an LD result does.
 * Checked on the host, in this order, before the handle's device is asked for: n == 0, sample_ids == NULL with n_ids != 0, non-NULL
 * sample_ids with n_ids == 0, stat neither VS_LD_DOT nor VS_LD_R2 -> VS_ERR_ARG; id 0 or id >= num_samples ->
 * VS_ERR_UNKNOWN_SAMPLE.  The blocks are formed from a temporary genotype matrix, which leaves the result as an LD batch's does;
 * the matrix and the 4 sum(m_q^2) bytes of cells together may not exceed option "matrix_max_mib" MiB (default 32 GiB): beyond it
 * the call is refused with VS_ERR_ARG once the plan has given the rows and before the matrix or the cells are allocated; the
 * message names regions, rows, the largest block, columns and bytes.  The block sizes are known on the device only: the call waits
 * once for a small scan over the per-region row counts, in front of the kernels vs_result_fill_ms times (the counts, the
 * temporary matrix and the block kernel).  The batch is never speculative and leaves the handle's type-6 state as it was.
 * vs_result_get_raw / vs_result_get_view with with_carriers = 0, vs_result_layout, vs_result_totals (n_carriers = the nonzero cells
 * of the matrix) work as for an LD result; vs_result_format_region gives "Pos\tRef\tAlt" and "\t<Pos>:<Ref>:<Alt>" for every reported,
 * non-dropped row of the region, then one line per such row: Pos, Ref, Alt and its values against the same rows, as %d or %.6g.
 * What an LD result refuses this result refuses with the same codes; vs_result_get_ld_band refuses it with VS_ERR_ARG. */
int vs_query_ld_matrix(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, uint32_t stat,
                       vs_result** out);
/* The blocks of an LD-matrix result copied into page-locked memory owned by the result (int32 under VS_LD_DOT, float under
 * VS_LD_R2: `stat` says which), block_begin[n_regions + 1], counts[i] the count record of table row i over S, col_ids[c] the sample
 * id of column c.  Every out-pointer but `cells` may be NULL.  VS_ERR_ARG on any other result. */
int vs_result_get_ld_matrix(vs_result* r, uint64_t* n_regions, uint64_t* n_rows, uint64_t* n_cols, uint32_t* stat, const uint32_t** col_ids,
                            const vs_allele_counts** counts, const uint64_t** block_begin, const void** cells);
/* Cells, block_begin (n_regions + 1 uint64) and counts (n_rows records of 16 bytes) as they lie in HBM, valid until vs_result_free.
 * The engine has synchronised its stream when this returns: the caller needs no event. */
int vs_result_ld_matrix_device(vs_result* r, uint64_t* n_regions, uint64_t* n_rows, uint64_t* n_cols, uint32_t* stat, const void** dev_counts,
                               const void** dev_block_begin, const void** dev_cells);
/* LD pruning over regions: the forward greedy r2 pruning of every region on the device -- the step in front of a GRM, a PCA or a
 * kinship table, which are meaningful on an LD-pruned variant set only (no reference counterpart).  The table T, its A rows,
 * row_begin / row_count, the column set S with n columns and the count records are those of vs_query_ld_band over the same regions
 * and ids.
 * For a table row i: ac_i = alt_alleles, Sx = ac_i, Sxx = ac_i + 2 hom_alt_i, v_i = n Sxx - Sx^2 in int64.  For a pair of rows: Sxy
 * the exact dosage dot product, cov = n Sxy - Sx Sy.
 * Threshold: an integer T in 0 .. 2^20 (threshold_q20); the r2 bound is T / 2^20.
 * Hit: the pair is a hit exactly when v_i > 0, v_j > 0 and cov^2 2^20 > T v_i v_j.  The comparison is evaluated in unsigned 128-bit
 * integers; no floating-point value takes part.  With n < 2^21 both sides stay below 2^108; a column set of 2^21 or more is refused
 * with VS_ERR_UNSUPPORTED.  T = 2^20 can never hit.
 * Eligible: a row is eligible when the duplicate rule did not drop it, v_i > 0 and min_ac <= ac_i <= max_ac (0 and UINT32_MAX admit
 * every row, as for vs_query_sample_burden).
 * Greedy: for region q, walk its table rows i = row_begin[q] .. row_begin[q] + row_count[q] - 1 in ascending order.  Row i is kept
 * when it is eligible and no already kept row j of the same walk satisfies all of 1 <= i - j <= window, max_bp == 0 or
 * |pos_i - pos_j| <= max_bp, and hit(j, i).  A pruned or ineligible row blocks nothing: the forward greedy with a sliding window of
 * SNPRelate's LD pruning, "the later row loses".  (MAF-priority removal and p-value clumping are other procedures.)
 * Regions are independent: each walk starts with an empty kept set at its own first row; overlapping or identical regions each get
 * their own verdicts over the shared rows, as vs_query_ld_matrix gives each region its own block.
 * Result: keep_begin[n + 1] (uint64), the exclusive scan of row_count; state[keep_begin[q] + a] (uint8), the verdict for table row
 * row_begin[q] + a: VS_PRUNE_PRUNED, VS_PRUNE_KEPT, VS_PRUNE_INELIGIBLE or VS_PRUNE_DROPPED; n_kept[q] (uint64) per region; the count
 * record of every table row over S, the column ids, and window, max_bp, T, min_ac, max_ac.  Every byte of `state` is stored exactly
 * once by a kernel.
 * Checked on the host, in this order, before the handle's device is asked for (a handle opened without a device reports them first
 * and VS_ERR_NO_DEVICE otherwise): n == 0, sample_ids == NULL with n_ids != 0, non-NULL sample_ids with n_ids == 0 -> VS_ERR_ARG;
 * window == 0 or window > 256 -> VS_ERR_ARG ("window" in the message); threshold_q20 > 2^20 -> VS_ERR_ARG ("threshold" in the
 * message); min_ac > max_ac -> VS_ERR_ARG; id 0 or id >= num_samples -> VS_ERR_UNKNOWN_SAMPLE.
 * The verdicts are formed from a temporary genotype matrix and temporary hit masks (ceil(window / 32) words of 4 bytes per table
 * row), which leave the result as an LD batch's matrix does; the matrix, the masks, `state` and the per-region arrays together may
 * not exceed option "matrix_max_mib" MiB (default 32 GiB): beyond it the call is refused with VS_ERR_ARG before anything is
 * allocated for them; the message names rows, columns, window and bytes.  The size of `state` is known on the device only: the
 * call may wait once for a small scan over the per-region row counts, in front of the kernels vs_result_fill_ms times (the counts,
 * the temporary matrix, the mask kernel and the walk).  The batch is never speculative and leaves the handle's type-6 state as it
 * was.  vs_result_get_raw / vs_result_get_view with with_carriers = 0, vs_result_layout, vs_result_totals (n_carriers = the nonzero
 * cells of the matrix) and vs_result_fill_ms work as for an LD result; vs_result_format_region gives "Pos\tRef\tAlt\tAC\tState\n",
 * then one line per reported, non-dropped row of the region, State one of keep, pruned, skip.  What an LD result refuses this
 * result refuses with the same codes; the other results' getters refuse it with VS_ERR_ARG. */
#define VS_PRUNE_PRUNED 0u
#define VS_PRUNE_KEPT 1u
#define VS_PRUNE_INELIGIBLE 2u
#define VS_PRUNE_DROPPED 3u
#define VS_PRUNE_THRESHOLD_ONE (1u << 20)
int vs_query_ld_prune(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, uint32_t window,
                      uint32_t max_bp, uint32_t threshold_q20, uint32_t min_ac, uint32_t max_ac, vs_result** out);
/* The verdicts of a pruning result copied into page-locked memory owned by the result: state[keep_begin[q] + a], keep_begin[n_regions
 * + 1], n_kept[n_regions], counts[i] the count record of table row i over S, col_ids[c] the sample id of column c, and params[5] =
 * {window, max_bp, threshold_q20, min_ac, max_ac}.  Every out-pointer but `state` may be NULL.  VS_ERR_ARG on any other result. */
int vs_result_get_ld_prune(vs_result* r, uint64_t* n_regions, uint64_t* n_rows, uint64_t* n_cols, uint32_t* params, const uint32_t** col_ids,
                           const vs_allele_counts** counts, const uint64_t** keep_begin, const uint64_t** n_kept, const uint8_t** state);
/* State (keep_begin[n_regions] bytes), keep_begin (n_regions + 1 uint64), n_kept (n_regions uint64) and counts (n_rows records of 16
 * bytes) as they lie in HBM, valid until vs_result_free.  The engine has synchronised its stream when this returns: the caller
 * needs no event. */
int vs_result_ld_prune_device(vs_result* r, uint64_t* n_regions, uint64_t* n_rows, uint64_t* n_cols, const void** dev_counts,
                              const void** dev_keep_begin, const void** dev_n_kept, const void** dev_state);
/* LD clumping over regions: p-value-ordered greedy clumps of every region on the device, as `plink --clump` forms them -- how a
 * scan becomes a list of independent loci, and how variants are chosen for a polygenic score (no reference counterpart).  The table
 * T, its A rows, row_begin / row_count, the column set S with n columns, the count records, hit(i, j) with the threshold T / 2^20
 * and keep_begin are exactly those of vs_query_ld_prune over the same regions and ids; hit is symmetric.
 * P-values: pvalues[i] (float64) belongs to table row i, in table order -- the rows a vs_query_allele_counts batch over the same
 * regions returns; there are A of them.  A p-value belongs to the variant: regions that share a row share it.  NaN: the row has no
 * p-value.  The host turns each p-value into a 64-bit key, the bit pattern of the non-negative double (-0.0 counts as 0), which is
 * monotone in p; p1 and p2 become keys the same way.  Priority is the pair (key, table row), ascending: ties go to the earlier row.
 * The device compares unsigned integers only; no floating-point value takes part in any verdict.
 * Candidates: row i is a candidate when it is not dropped, v_i > 0, it has a p-value and key_i <= key(p2); index-eligible when also
 * key_i <= key(p1).
 * Procedure, for every region on its own rows: walk the index-eligible candidates in priority order.  A row not yet assigned
 * becomes an INDEX and owns itself; every not yet assigned candidate j of the region with 1 <= |i - j| <= window, max_bp == 0 or
 * |pos_i - pos_j| <= max_bp, and hit(i, j) becomes a MEMBER with owner i (the window reaches both ways).  A candidate between p1 and
 * p2 can only join.  Candidates left at the end are UNCLUMPED.  Equivalently: the INDEX rows are the lexicographically first maximal
 * independent set of the index-eligible candidates under hit, in priority order, and the owner of any other candidate is the INDEX
 * row of the highest priority that hits it inside the window.  Regions are independent, as for vs_query_ld_prune.
 * Result: keep_begin[n + 1]; state[keep_begin[q] + a] (uint8): VS_CLUMP_MEMBER, VS_CLUMP_INDEX, VS_CLUMP_INELIGIBLE (no variance, no
 * p-value, or a p-value above p2), VS_CLUMP_DROPPED or VS_CLUMP_UNCLUMPED; owner[keep_begin[q] + a] (uint32): the region-relative
 * row of the index, VS_CLUMP_NO_OWNER for a row that is neither INDEX nor MEMBER; n_index[q] (uint64); the count records, the column
 * ids and the parameters.  rounds[q] (uint64) is a diagnostic: the parallel rounds the region's greedy took; it is no part of the
 * answer and may differ between runs.
 * Checked on the host, in this order, before the handle's device is asked for (a handle opened without a device reports them first
 * and VS_ERR_NO_DEVICE otherwise): n == 0, sample_ids == NULL with n_ids != 0, non-NULL sample_ids with n_ids == 0 -> VS_ERR_ARG;
 * window == 0 or window > 256 -> VS_ERR_ARG ("window" in the message); threshold_q20 > 2^20 -> VS_ERR_ARG ("threshold"); pvalues ==
 * NULL -> VS_ERR_ARG ("pvalues"); p1, then p2, NaN or outside [0, 1] -> VS_ERR_ARG ("p1" / "p2"); p1 > p2 -> VS_ERR_ARG ("above");
 * a p-value that is neither NaN nor in [0, 1] -> VS_ERR_ARG (the message names the table row); id 0 or id >= num_samples ->
 * VS_ERR_UNKNOWN_SAMPLE.  A is known on the device only: after the call's one host wait, n_pvalues != A -> VS_ERR_ARG with both
 * numbers in the message.
 * The uploaded keys (8 A bytes), the classes (A bytes), the temporary genotype matrix, the hit masks, the blocker masks (two masks of
 * ceil(window / 32) words per verdict), `state`, `owner` and the per-region words together may not exceed option "matrix_max_mib"
 * MiB: beyond it the call is refused with VS_ERR_ARG before anything is allocated for them; the message names regions, rows,
 * columns, window and the parts in bytes.  The batch is never speculative and leaves the handle's type-6 state as it was.  What works
 * on a pruning result works here; vs_result_format_region gives "Pos\tRef\tAlt\tAC\tP\tState\tIndex\n", then one line per reported,
 * non-dropped row of the region: P as %.6g or "." without a p-value, State one of index, clumped, unclumped, skip, Index the owner
 * as Pos:Ref:Alt or ".".  What a pruning result refuses this result refuses with the same codes; the other results' getters refuse
 * it, and its getters refuse the others, with VS_ERR_ARG. */
#define VS_CLUMP_MEMBER 0u
#define VS_CLUMP_INDEX 1u
#define VS_CLUMP_INELIGIBLE 2u
#define VS_CLUMP_DROPPED 3u
#define VS_CLUMP_UNCLUMPED 4u
#define VS_CLUMP_NO_OWNER 0xFFFFFFFFu
int vs_query_ld_clump(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, const double* pvalues,
                      uint64_t n_pvalues, uint32_t window, uint32_t max_bp, uint32_t threshold_q20, double p1, double p2, vs_result** out);
/* The verdicts of a clumping result copied into page-locked memory owned by the result: state and owner [keep_begin[n_regions]],
 * keep_begin[n_regions + 1], n_index[n_regions], rounds[n_regions], counts[i] the count record of table row i over S, col_ids[c] the
 * sample id of column c, params[3] = {window, max_bp, threshold_q20}, p_keys[2] the keys of p1 and p2 and p_bounds[2] the doubles.
 * Every out-pointer but `state` and `owner` may be NULL.  VS_ERR_ARG on any other result. */
int vs_result_get_ld_clump(vs_result* r, uint64_t* n_regions, uint64_t* n_rows, uint64_t* n_cols, uint32_t* params, uint64_t* p_keys, double* p_bounds,
                           const uint32_t** col_ids, const vs_allele_counts** counts, const uint64_t** keep_begin, const uint64_t** n_index,
                           const uint64_t** rounds, const uint8_t** state, const uint32_t** owner);
/* State (keep_begin[n_regions] bytes), owner (as many uint32), keep_begin (n_regions + 1 uint64), n_index (n_regions uint64) and
 * counts (n_rows records of 16 bytes) as they lie in HBM, valid until vs_result_free.  The engine has synchronised its stream when
 * this returns: the caller needs no event. */
int vs_result_ld_clump_device(vs_result* r, uint64_t* n_regions, uint64_t* n_rows, uint64_t* n_cols, const void** dev_counts,
                              const void** dev_keep_begin, const void** dev_n_index, const void** dev_state, const void** dev_owner);
/* LD scores over regions: for every table row of every region the sum of r2 with the rows of the same region within a distance of
 * it -- the input of LD-score regression, of LDAK-style variant weights and of LD-aware annotation --, reduced on the device from
 * the products an LD matrix is formed from, without the matrix: the window has no 256-row ceiling (no reference counterpart).  The
 * table T, its A rows, row_begin / row_count, the column set S with n columns, the count records, v_i and cov are those of
 * vs_query_ld_prune over the same regions and ids.  All arithmetic is integer: no floating-point value decides or is summed.
 * Region q owns the table rows row_begin[q] + a, a < m_q = row_count[q], and the slots keep_begin[q] + a, keep_begin exactly
 * vs_query_ld_prune's scan of the row counts; overlapping regions each get their own slots, regions are independent.
 * Eligible: as for vs_query_ld_prune -- the duplicate rule did not drop the row, v = n Sxx - Sx^2 > 0 and min_ac <= alt_alleles <=
 * max_ac.
 * Per pair: for an eligible pair (a, b), q32(a, b) = floor(cov^2 2^32 / (v_a v_b)); 0 .. 2^32 by Cauchy-Schwarz, exactly 2^32 for
 * a = b.
 * Sum: for an eligible row a, sums[slot] = the sum of q32(a, b) over all eligible b of the same region, b = a INCLUDED (the LDSC
 * convention), with |a - b| <= window in table rows (window = 0: no row limit) and, if max_bp is nonzero, |pos_a - pos_b| <=
 * max_bp.  n_pairs[slot] = the number of b summed, self included.  Ineligible and dropped rows: sums = 0, n_pairs = 0.
 * State: a byte per slot, VS_LDSCORE_SCORED, VS_LDSCORE_INELIGIBLE or VS_LDSCORE_DROPPED; n_scored[q] counts the scored rows.
 * The score is sums / 2^32.  With n < 2^21: cov^2 2^32 < 2^120 and q v_a v_b < 2^121; a column set of 2^21 or more is refused with
 * VS_ERR_UNSUPPORTED.  The sums are added with integer atomics: the same call gives the same bytes.
 * Checked on the host, in this order, before the handle's device is asked for (a handle opened without a device reports them first
 * and VS_ERR_NO_DEVICE otherwise): n == 0, sample_ids == NULL with n_ids != 0, non-NULL sample_ids with n_ids == 0 -> VS_ERR_ARG;
 * min_ac > max_ac -> VS_ERR_ARG; id 0 or id >= num_samples -> VS_ERR_UNKNOWN_SAMPLE; 2^21 columns or more -> VS_ERR_UNSUPPORTED.
 * The sums are formed from a temporary genotype matrix, which leaves the result as an LD batch's matrix does; the matrix, 13 bytes
 * per slot (8 of the sum, 4 of the pair count, 1 of the state) and the per-region arrays together may not exceed option
 * "matrix_max_mib" MiB (default 32 GiB): beyond it the call is refused with VS_ERR_ARG before anything is allocated for them; the
 * message names rows, columns and bytes.  The number of slots is known on the device only: the call may wait once for a small scan
 * over the per-region row counts, in front of the kernels vs_result_fill_ms times.  More than 2^31 - 1 workgroups (a region of t
 * tiles of 64 rows takes t (B + 1), B = the tile distances the window reaches) are refused with VS_ERR_ARG.  The batch is never
 * speculative and leaves the handle's type-6 state as it was.  vs_result_get_raw / vs_result_get_view with with_carriers = 0,
 * vs_result_layout, vs_result_totals and vs_result_fill_ms work as for a pruning result; vs_result_format_region gives
 * "Pos\tRef\tAlt\tAC\tPairs\tL2\tState\n", then one line per reported, non-dropped row of the region: L2 = sums / 2^32 as %.6f,
 * State one of scored, skip.  What a pruning result refuses this result refuses with the same codes; the other results' getters
 * refuse it, and its getters refuse the others, with VS_ERR_ARG. */
#define VS_LDSCORE_SCORED 1u
#define VS_LDSCORE_INELIGIBLE 2u
#define VS_LDSCORE_DROPPED 3u
#define VS_LDSCORE_ONE (1ull << 32)
int vs_query_ld_scores(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, uint32_t window, uint32_t max_bp,
                       uint32_t min_ac, uint32_t max_ac, vs_result** out);
/* The scores of an LD-score result copied into page-locked memory owned by the result: sums (uint64), n_pairs (uint32) and state
 * (uint8), keep_begin[n_regions] of each, keep_begin[n_regions + 1], n_scored[n_regions], counts[i] the count record of table row i
 * over S, col_ids[c] the sample id of column c, and params[4] = {window, max_bp, min_ac, max_ac}.  Every out-pointer but `sums` may
 * be NULL.  VS_ERR_ARG on any other result. */
int vs_result_get_ld_scores(vs_result* r, uint64_t* n_regions, uint64_t* n_rows, uint64_t* n_cols, uint32_t* params, const uint32_t** col_ids,
                            const vs_allele_counts** counts, const uint64_t** keep_begin, const uint64_t** n_scored, const uint64_t** sums,
                            const uint32_t** n_pairs, const uint8_t** state);
/* Sums (n_slots uint64), n_pairs (n_slots uint32), state (n_slots bytes), keep_begin (n_regions + 1 uint64), n_scored (n_regions
 * uint64) and counts (n_rows records of 16 bytes) as they lie in HBM, valid until vs_result_free; n_slots = keep_begin[n_regions].
 * The engine has synchronised its stream when this returns: the caller needs no event. */
int vs_result_ld_scores_device(vs_result* r, uint64_t* n_regions, uint64_t* n_rows, uint64_t* n_cols, uint64_t* n_slots, const void** dev_counts,
                               const void** dev_keep_begin, const void** dev_n_scored, const void** dev_sums, const void** dev_n_pairs,
                               const void** dev_state);
/* Sample Gram matrix / GRM over regions: D^T D, the samples x samples product of the dosages -- what a GRM, kinship, IBS-type sharing
 * and the PCA of a cohort start from, and the one product of the dosage matrix the other column queries leave out (D Y:
 * vs_query_assoc_scan, D^T W: vs_query_sample_scores, the band of D D^T: vs_query_ld_band; no reference counterpart).  T, its rows, S
 * and its n columns are those of vs_query_genotype_matrix over the same regions and sample_ids; A is the number of rows of T and
 * d_v(s) = popcount(cell & 6) the dosage of table row v in column s.  Each table row counts once, however many regions report it;
 * a row the duplicate rule dropped has an all-zero matrix row and an all-zero count record and adds nothing to any sum.
 *   VS_GRAM_DOT   gram[i * n + j] = sum over v of d_v(i) * d_v(j), int64, exact: the full symmetric matrix, the diagonal sum d^2;
 *                 and from the rows' count records over S (ac_v = alt_alleles of row v): col_weighted[i] = s_i = sum ac_v d_v(i)
 *                 (int64), C = sum ac_v^2, H = sum ac_v (2 n - ac_v)
 *   VS_GRAM_GRM   the same and VanRaden's first GRM, Z Z^T / 2 sum p (1 - p) with Z = D - 2 p and p_v = ac_v / 2 n, from exact
 *                 integers: num_ij = n^2 gram_ij - n (s_i + s_j) + C in 128-bit integers, grm[i * n + j] = (double)(2 num_ij) /
 *                 (double)H as float64 -- each conversion rounds once, to nearest even, one division follows -- and 0.0 when
 *                 H == 0 (every row monomorphic in S, no rows, n = 1 gives num = 0 everywhere)
 * Nothing floating-point is ever summed, and the integer sums are formed with integer atomics: the same call gives the same bytes.
 * C and H are 64-bit sums: 4 A n^2 must stay below 2^63.
 * `regions` and `sample_ids` as for vs_query_genotype_matrix.  Checked on the host, in this order, before the handle's device is
 * asked for (a handle opened without a device reports them first and VS_ERR_NO_DEVICE otherwise): n == 0, sample_ids == NULL with
 * n_ids != 0, non-NULL sample_ids with n_ids == 0, stat neither VS_GRAM_DOT nor VS_GRAM_GRM -> VS_ERR_ARG; id 0 or id >=
 * num_samples -> VS_ERR_UNKNOWN_SAMPLE.  The products are formed from a temporary genotype matrix (rows x row_pitch bytes, not part
 * of the result: it goes back to the handle's pool as an LD batch's does); the matrix and the n x n cells -- 8 bytes each, 16
 * under VS_GRAM_GRM -- together may not exceed option "matrix_max_mib" MiB (default 32 GiB): beyond it the call is refused with
 * VS_ERR_ARG once the plan has given the rows and before anything is allocated; the message names rows, columns and bytes.
 * Option "gram_chunk": the table rows one workgroup of the product kernel sums before it adds its partial sums to the matrix,
 * 64 .. 65536; 0 (default): by the batch's shape -- the multiple of 128 rows that gives about 256 workgroups over all pairs of
 * 128-column tiles, at least 256 rows.  The sums are the same integers under every setting.
 * Every batch size takes the batch pipeline; a Gram batch is never speculative and leaves the handle's type-6 state as it was.  The
 * result holds the type-6 per-region arrays and variant table, no carrier arena, the counts and the matrices: vs_result_get_raw /
 * vs_result_get_view with with_carriers = 0, vs_result_layout (arena and lists 0), vs_result_fill_ms (the batch's own kernels) and
 * vs_result_totals (n_carriers = the nonzero cells of the temporary matrix) work; vs_result_format_region fails with
 * VS_ERR_UNSUPPORTED (one matrix over the whole batch: there is no text per region), and so do with_carriers = 1, vs_result_digest,
 * vs_result_pack_headers / _pack_regions and vs_comm_allgather_regions*; the other vs_result_get_* accessors fail with VS_ERR_ARG. */
#define VS_GRAM_DOT 0u
#define VS_GRAM_GRM 1u
int vs_query_sample_gram(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, uint32_t stat,
                         vs_result** out);
/* A Gram result copied into page-locked memory owned by the result: gram[i * n_cols + j], grm[i * n_cols + j] (NULL under
 * VS_GRAM_DOT), col_weighted[i], C and H, counts[v] the count record of table row v over S, col_ids[c] the sample id of column c.
 * Every out-pointer but `gram` may be NULL.  VS_ERR_ARG on any other result. */
int vs_result_get_sample_gram(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* stat, const uint32_t** col_ids,
                              const vs_allele_counts** counts, const int64_t** gram, const double** grm, const int64_t** col_weighted,
                              int64_t* C, int64_t* H);
/* The same as it lies in HBM, valid until vs_result_free: n_cols x n_cols int64, n_cols x n_cols float64 (NULL under VS_GRAM_DOT),
 * n_cols int64 with C and H right behind them, n_rows count records of 16 bytes.  The engine has synchronised its stream when this
 * returns: the caller needs no event. */
int vs_result_sample_gram_device(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* stat, const void** dev_counts,
                                 const void** dev_gram, const void** dev_grm, const void** dev_col_weighted);
/* Pairwise IBS counts and KING kinship over regions: for every pair of samples how often both are heterozygous, how often they are
 * opposite homozygotes (IBS0) and how often they agree (IBS2) -- what KING and `plink2 --make-king-table` start from to say who is
 * related to whom and which samples are duplicates (no reference counterpart).  These are counts of genotype STATES: they cannot be
 * recovered from the Gram matrix of vs_query_sample_gram, one cell of which mixes het x het, het x hom and hom x hom.
 * T, its A rows, the column set S and its n columns are those of vs_query_genotype_matrix over the same regions and sample_ids.
 * The dosage is d_v(s) = popcount(cell & 6).  Each table row counts once, however many regions report it.  For a row v let
 *   h_v(s) = [d_v(s) == 1],   a_v(s) = [d_v(s) == 2],   c_v(s) = [d_v(s) > 0].
 * Three primitive matrices are accumulated; they are int64, n x n, full and symmetric:
 *   het_het[i * n + j]      = sum over v of h_v(i) h_v(j)
 *   hom_hom[i * n + j]      = sum over v of a_v(i) a_v(j)
 *   carrier_both[i * n + j] = sum over v of c_v(i) c_v(j)
 * Their diagonals are the per-sample totals nh_i, na_i and nc_i = nh_i + na_i.
 * A row the duplicate rule dropped (bit 31 of its count_flags) has an all-zero matrix row: it adds nothing to the primitives and is
 * not a site.  n_used = A - dropped rows.
 * From the primitives, in exact int64:
 *   ibs0[i * n + j] = na_i + na_j - 2 hom_hom - (carrier_both - het_het - hom_hom)     the opposite homozygotes, {0, 2}
 *   ibs2[i * n + j] = n_used - nc_i - nc_j + carrier_both + het_het + hom_hom           equal dosage, 0/0 included
 *   ibs1            = n_used - ibs0 - ibs2                                               not stored
 *   VS_IBS_COUNTS   the five matrices above and n_used
 *   VS_IBS_KING     the same and king[i * n + j] = (double)(het_het - 2 ibs0) / (double)(nh_i + nh_j) as float64, 0.0 where
 *                   nh_i + nh_j == 0: the KING-robust between-family estimator, in the form with the sum of the two het counts in
 *                   the denominator; the diagonal is 0.5 wherever nh_i > 0.  Numerator and denominator are integers below 2^53:
 *                   each converts exactly and one division follows
 * Nothing floating-point is ever summed, and the integer sums are formed with integer atomics: the same call gives the same bytes.
 * `regions` and `sample_ids` as for vs_query_genotype_matrix.  Checked on the host, in this order, before the handle's device is
 * asked for (a handle opened without a device reports them first and VS_ERR_NO_DEVICE otherwise): n == 0, sample_ids == NULL with
 * n_ids != 0, non-NULL sample_ids with n_ids == 0, stat neither VS_IBS_COUNTS nor VS_IBS_KING -> VS_ERR_ARG; id 0 or id >=
 * num_samples -> VS_ERR_UNKNOWN_SAMPLE.  The products are formed from a temporary genotype matrix (rows x row_pitch bytes, not part
 * of the result: it goes back to the handle's pool as an LD or Gram batch's does); the matrix and the n x n cells -- 40 bytes each,
 * 48 under VS_IBS_KING -- together may not exceed option "matrix_max_mib" MiB (default 32 GiB): beyond it the call is refused with
 * VS_ERR_ARG once the plan has given the rows and before anything is allocated; the message names rows, columns and bytes.
 * Option "ibs_chunk": the table rows one workgroup of the product kernel sums before it adds its partial sums to the matrices,
 * 64 .. 65536; 0 (default): by the batch's shape -- the multiple of 128 rows that gives about 128 workgroups over all pairs of
 * 128-column tiles, at least 256 rows, the table's rows spread evenly over the chunks.  The sums are the same integers under every
 * setting.
 * Every batch size takes the batch pipeline; an IBS batch is never speculative and leaves the handle's type-6 state as it was.  The
 * result holds the type-6 per-region arrays and variant table, no carrier arena, the counts and the matrices: vs_result_get_raw /
 * vs_result_get_view with with_carriers = 0, vs_result_layout (arena and lists 0), vs_result_fill_ms (the batch's own kernels) and
 * vs_result_totals (n_carriers = the nonzero cells of the temporary matrix) work; vs_result_format_region fails with
 * VS_ERR_UNSUPPORTED (matrices over the whole batch: there is no text per region), and so do with_carriers = 1, vs_result_digest,
 * vs_result_pack_headers / _pack_regions and vs_comm_allgather_regions*; the other vs_result_get_* accessors fail with VS_ERR_ARG. */
#define VS_IBS_COUNTS 0u
#define VS_IBS_KING 1u
int vs_query_sample_ibs(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, uint32_t stat,
                        vs_result** out);
/* An IBS result copied into page-locked memory owned by the result: the five matrices [i * n_cols + j], king (NULL under
 * VS_IBS_COUNTS), n_used, counts[v] the count record of table row v over S, col_ids[c] the sample id of column c.
 * Every out-pointer but `het_het` may be NULL.  VS_ERR_ARG on any other result. */
int vs_result_get_sample_ibs(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* stat, const uint32_t** col_ids,
                             const vs_allele_counts** counts, const int64_t** het_het, const int64_t** hom_hom, const int64_t** carrier_both,
                             const int64_t** ibs0, const int64_t** ibs2, const double** king, int64_t* n_used);
/* The same as it lies in HBM, valid until vs_result_free: dev_matrices is five n_cols x n_cols int64 matrices one behind the other
 * -- het_het, hom_hom, carrier_both, ibs0, ibs2 -- with n_used (one int64) right behind them; dev_king n_cols x n_cols float64 (NULL
 * under VS_IBS_COUNTS); n_rows count records of 16 bytes.  The engine has synchronised its stream when this returns: the caller
 * needs no event. */
int vs_result_sample_ibs_device(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint32_t* stat, const void** dev_counts,
                                const void** dev_matrices, const void** dev_king);

/* Trio scan over regions: Mendelian errors and allele transmissions per table row and per trio -- what `plink --mendel`, `plink --tdt`
 * and `bcftools +mendelian` start from once parents and children are known -- counted on the GPU without the genotype matrix ever
 * reaching the host.  The variant table, its rows and which of them the duplicate rule dropped are those of
 * vs_query_genotype_matrix over the same regions.  `trios`: 3 * n_trios sample ids, per trio child, father, mother -- pairwise
 * distinct, none of them 0.  A sample may appear in any number of trios and in any role; the same triple given twice counts twice.
 * The columns S are the distinct ids over all trios, ascending.
 * For a table row v and a trio t let f, m, c be the dosages popcount(cell & 6) of father, mother and child (0, 1 or 2; a dropped
 * row is all zeros), and g(0) = {0}, g(1) = {0, 1}, g(2) = {1} the gametes a parent of that dosage can give:
 *   error         c is no sum a + b with a in g(f), b in g(m)
 *   denovo        f == 0 && m == 0 && c > 0, a subset of the errors
 *   transmitted   T = c - [f == 2] - [m == 2]            consistent cells only: an error cell adds nothing to T or U
 *   untransmitted U = [f == 1] + [m == 1] - T            a cell with no heterozygous parent has T = U = 0; both parents and the
 *                                                        child heterozygous: T = U = 1
 * Only the dosage takes part: the query is meant for diploid calls, a haploid `1` counts as dosage 1.  A `1|2` call shows dosage 1
 * on both of its ALT rows, as everywhere here: the rule per row is then a necessary condition per allele.
 *   rows[v]   the four sums over all trios
 *   trios[t]  the four sums over every table row once (rows that several regions report count once, as for vs_query_sample_ibs)
 *   n_used    the table's rows minus those the duplicate rule dropped
 *   counts[v] the count record of table row v over S
 * All sums are integers formed with integer adds: the same call gives the same bytes.
 * `regions` as for vs_query_genotype_matrix.  Checked on the host, in this order, before the handle's device is asked for (a handle
 * opened without a device reports them first and VS_ERR_NO_DEVICE otherwise): n == 0, trios == NULL, n_trios == 0 or n_trios >
 * VS_TRIOS_MAX -> VS_ERR_ARG; then trio by trio: two equal ids inside the triple -> VS_ERR_ARG (the message names the trio's index),
 * id 0 or id >= num_samples -> VS_ERR_UNKNOWN_SAMPLE; more than 65,536 distinct members -> VS_ERR_UNSUPPORTED (a staged row must
 * fit the kernel's LDS tile).  Once the plan has given the rows and before anything is allocated: a table of 2^31 rows or more ->
 * VS_ERR_ARG (a per-trio sum must fit uint32); the temporary genotype matrix (rows x row_pitch bytes, not part of the result), the
 * count records, both record arrays and the trio table together may not exceed option "matrix_max_mib" MiB (default 32 GiB):
 * beyond it VS_ERR_ARG, and the message names rows, columns, trios and bytes.
 * Option "trio_chunk": the trios one workgroup of the scan takes, a multiple of 64 in 64 .. 16384; 0 (default): by the batch's
 * shape -- all of them unless the table's row blocks alone give fewer than 2048 workgroups.  The sums are the same integers under
 * every setting.
 * Every batch size takes the batch pipeline; a trio batch is never speculative and leaves the handle's type-6 state as it was.  The
 * result holds the type-6 per-region arrays and variant table, no carrier arena, the counts and the records: vs_result_get_raw /
 * vs_result_get_view with with_carriers = 0, vs_result_layout (arena and lists 0), vs_result_fill_ms (the batch's own kernels) and
 * vs_result_totals (n_carriers = the nonzero cells of the temporary matrix) work; vs_result_format_region returns per reported row
 * "Pos Ref Alt AC Errors DeNovo T U" (tab-separated, under that header; AC over S; dropped rows left out); with_carriers = 1,
 * vs_result_digest, vs_result_pack_headers / _pack_regions and vs_comm_allgather_regions* fail with VS_ERR_UNSUPPORTED; the other
 * vs_result_get_* accessors fail with VS_ERR_ARG. */
#define VS_TRIOS_MAX (1u << 20)
typedef struct { uint32_t errors, denovo, transmitted, untransmitted; } vs_trio_counts;
int vs_query_trio_scan(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* trios /* 3 * n_trios: child, father, mother */,
                       uint64_t n_trios, vs_result** out);
/* A trio result copied into page-locked memory owned by the result: rows[v], trios[t], n_used, counts[v], col_ids[c] the sample id
 * of column c, trio_cols three column indices per trio (child, father, mother: col_ids[trio_cols[3 t]] is trio t's child).
 * Every out-pointer but `rows` may be NULL.  VS_ERR_ARG on any other result. */
int vs_result_get_trio_scan(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint64_t* n_trios, uint64_t* n_used, const uint32_t** col_ids,
                            const uint32_t** trio_cols /* 3 per trio: column indices */, const vs_allele_counts** counts,
                            const vs_trio_counts** rows, const vs_trio_counts** trios);
/* The same as it lies in HBM, valid until vs_result_free: dev_rows n_rows records of 16 bytes, dev_trios n_trios records right behind
 * them, dev_n_used one uint64 right behind those; n_rows count records of 16 bytes.  The engine has synchronised its stream when
 * this returns: the caller needs no event. */
int vs_result_trio_scan_device(vs_result* r, uint64_t* n_rows, uint64_t* n_cols, uint64_t* n_trios, const void** dev_counts,
                               const void** dev_rows, const void** dev_trios, const void** dev_n_used);

/* Runs of homozygosity over regions: per region and per sample the autozygous stretches, their number and their total length --
 * what `plink --homozyg` reports and F_ROH is formed from -- found on the GPU by walking every column of the batch's genotype matrix
 * in row order, without that matrix ever reaching the host.  Everything is an integer.
 * The variant table, its rows, which of them the duplicate rule dropped and the columns are those of vs_query_genotype_matrix over
 * the same regions and sample ids: the columns S are the distinct ids ascending, or every sample when sample_ids == NULL.
 * Site: a table row is a site when the duplicate rule did not drop it, it is polymorphic over the columns -- 0 < ac < 2 n, ac the
 * row's alt_alleles over S, n the number of columns -- and min_ac <= ac <= max_ac (0 and UINT32_MAX admit every count): the rows
 * vs_query_ld_prune calls eligible, and a row on which EVERY column is heterozygous besides (its variance is 0, it is a site
 * here).  Any other row is invisible: it neither extends nor breaks a run.
 * State: at a site column c is het when its dosage popcount(cell & 6) is 1 and hom when it is 0 or 2.  Only the dosage takes part:
 * a `1|2` call is dosage 1 on both of its ALT rows, as everywhere here, so it is het on both.
 * Walk: for region q and column c the sites of q in table order, site i at position p_i, with the run's first, last, n_sites,
 * n_het and pend:
 *   gap rule             before site i is looked at: a run is open, max_gap > 0 and p_i - p_(i-1) > max_gap -> close.  p_(i-1) is the
 *                        previous SITE whatever its state; a difference that would be negative counts as 0
 *   hom, no run open     open: first = last = i, n_sites = 1, n_het = 0, pend = 0
 *   hom, run open        n_sites += pend + 1, n_het += pend, pend = 0, last = i
 *   het, run open        n_het + pend < max_het: pend += 1; otherwise close -- the next run opens at the next hom site, the hets the
 *                        closed run had absorbed are not looked at again
 *   het, no run open     nothing
 *   end of the region    close
 *   close                pending hets behind `last` are not part of the run.  With bp = max(p_last - p_first, 0) + 1 the run is a
 *                        SEGMENT when n_sites >= min_sites and bp >= min_bp; otherwise it is discarded
 * Answer: per (region, column), region-major, a vs_roh_summary -- n_segments; seg_sites, total_bp and seg_hets, the sums of the
 * segments' n_sites, bp and n_het; longest_bp (saturating at 2^32 - 1) and longest_sites, of the segment of largest bp, the EARLIEST
 * such on a tie; n_het, the column's het sites in the region, inside segments or not.  Per region n_sites[q].  With segments != 0
 * also seg_begin [Q S + 1] and the segments: cell (q, c) owns segments[seg_begin[q S + c] .. seg_begin[q S + c + 1]), in order of
 * occurrence -- so the segments are ordered by region, then column, then occurrence; row_first and row_last are offsets into the
 * region's row_count rows.  No floating-point value anywhere: the same call gives the same bytes.
 * `regions` as for vs_query_genotype_matrix.  Checked on the host, in this order, before the handle's device is asked for (a handle
 * opened without a device reports them first and VS_ERR_NO_DEVICE otherwise): n == 0 -> VS_ERR_ARG; an empty subset -> VS_ERR_ARG;
 * params == NULL, min_sites == 0, max_het > 255, min_ac > max_ac -> VS_ERR_ARG; then the sample ids as for vs_query_ld_prune (id 0
 * or id >= num_samples -> VS_ERR_UNKNOWN_SAMPLE).  Once the plan has given the rows and before anything is allocated: a table of
 * 2^31 rows or more -> VS_ERR_ARG; the temporary genotype matrix (rows x row_pitch bytes, not part of the result), the count records,
 * the walk's site words, the summaries, the per-cell words and n_sites together may not exceed option "matrix_max_mib" MiB (default
 * 32 GiB); once the first pass has counted the segments, their 32 bytes each are held to it too.  Beyond it VS_ERR_ARG, and the
 * message names regions, columns, segments and bytes.
 * Every batch size takes the batch pipeline; a ROH batch is never speculative and leaves the handle's type-6 state as it was.  The
 * result holds the type-6 per-region arrays and variant table, no carrier arena, the counts, the summaries and the segments:
 * vs_result_get_raw / vs_result_get_view with with_carriers = 0, vs_result_layout (arena and lists 0), vs_result_fill_ms (the batch's
 * own kernels, its one host wait between the passes included) and vs_result_totals (n_carriers = the nonzero cells of the temporary
 * matrix) work; vs_result_format_region returns region q's segments, a line each, "Sample Pos1 Pos2 KB NSites NHet" (tab-separated,
 * under that header; KB = bp / 1000 printed from the integer with three decimals) and fails with VS_ERR_ARG when segments == 0;
 * with_carriers = 1, vs_result_digest, vs_result_pack_headers / _pack_regions and vs_comm_allgather_regions* fail with
 * VS_ERR_UNSUPPORTED; the other vs_result_get_* accessors fail with VS_ERR_ARG. */
typedef struct {
  uint32_t min_sites;   /* a segment has at least this many sites (>= 1) */
  uint32_t min_bp;      /* ... and spans at least this many bases (0: any) */
  uint32_t max_gap;     /* two consecutive sites further apart than this close the run (0: no gap rule) */
  uint32_t max_het;     /* het sites a run may absorb (0 .. 255) */
  uint32_t min_ac, max_ac;   /* the site window over ac (0 and UINT32_MAX: every count) */
  uint32_t segments;    /* nonzero: the answer also holds seg_begin and the segments */
} vs_roh_params;
typedef struct { uint32_t n_segments, seg_sites; uint64_t total_bp; uint32_t longest_bp, longest_sites, seg_hets, n_het; } vs_roh_summary;
typedef struct { uint32_t region, column, pos_first, pos_last, row_first, row_last, n_sites, n_het; } vs_roh_segment;
int vs_query_roh(vs_index* idx, const vs_region* regions, uint64_t n, const uint32_t* sample_ids, uint64_t n_ids, const vs_roh_params* params,
                 vs_result** out);
/* A ROH result copied into page-locked memory owned by the result: summary[q * n_cols + c], n_sites[q], col_ids[c] the sample id of
 * column c, counts[v] the count record of table row v over S, params the batch's own; with segments seg_begin [n_regions * n_cols + 1]
 * and segments [n_segments], else both NULL and n_segments 0.  Every out-pointer but `summary` may be NULL.  VS_ERR_ARG on any other
 * result. */
int vs_result_get_roh(vs_result* r, uint64_t* n_regions, uint64_t* n_cols, uint64_t* n_rows, uint64_t* n_segments, vs_roh_params* params,
                      const uint32_t** col_ids, const vs_allele_counts** counts, const vs_roh_summary** summary, const uint32_t** n_sites,
                      const uint64_t** seg_begin, const vs_roh_segment** segments);
/* The same as it lies in HBM, valid until vs_result_free: dev_summary n_regions * n_cols records of 32 bytes, dev_n_sites n_regions
 * uint32 behind them, dev_seg_begin n_regions * n_cols + 1 uint64 and dev_segments n_segments records of 32 bytes (both NULL without
 * segments), dev_counts n_rows count records of 16 bytes.  The engine has synchronised its stream when this returns: the caller
 * needs no event. */
int vs_result_roh_device(vs_result* r, uint64_t* n_regions, uint64_t* n_cols, uint64_t* n_rows, uint64_t* n_segments, const void** dev_counts,
                         const void** dev_summary, const void** dev_n_sites, const void** dev_seg_begin, const void** dev_segments);

/* host view of a sequence result: region i is chars[seq_begin[i] .. seq_begin[i+1]) */
int vs_result_get_sequences(vs_result* r, uint64_t* n_regions, const uint8_t** region_flags, const uint64_t** seq_begin,
                            const char** chars);
/* `variantstore draw` (src/commands.cc:217-242 -> draw_subgraph, include/query.h:825-842 -> createDotGraph,
 * include/dot_graph.h:71-132): the vertices within `radius` hops of the vertex at `pos` (on the path of `sample`;
 * NULL or "ref" = the reference) as a Graphviz file.  Host-only; works on handles opened without a device. */
int vs_index_draw_subgraph(const vs_index* idx, uint64_t pos, uint64_t radius, const char* sample, const char* outfile);
/* batched Index::find (index.h:119-133): vertex id of the ref node covering each position */
int vs_index_find(vs_index* idx, const uint64_t* pos, uint64_t n, uint32_t* vertex_out);

/* Result of one batch.  Arrays live in HBM until a view is requested. */
enum { VS_REGION_EMPTY = 1,   /* Index::is_empty early-out fired (query.h:745-756 prints the other label) */
       VS_REGION_INVALID = 2, /* pos_x < 1: the reference aborts (index.h:151-154) */
       VS_REGION_NOT_FOUND = 4, /* types 1 and 7: closest_var returned false / "There is no such variant!" */
       VS_REGION_ENDLESS = 8   /* types 3 and 5: the reference's backward search (query.h:213-218) never terminates */ };
enum { VS_VAR_DROPPED = 1 };  /* suppressed by the reference's "already seen" rule, query.h:397-414 */
#define VS_CARRIER_ID(c) ((c) & 0x1FFFFFFFu)
#define VS_CARRIER_GT(c) ((c) >> 29)         /* bit0 phase ('|'), bit1 gt_1, bit2 gt_2 */

typedef struct {
  uint64_t n_regions;
  const uint8_t* region_flags;   /* [n_regions] */
  const uint64_t* var_begin;     /* [n_regions+1] slot range of each region */
  const uint64_t* var_count;     /* [n_regions]   variants the reference reports (slots minus dropped) */
  uint64_t n_slots;
  const uint64_t* pos;           /* [n_slots] Variant::var_pos */
  const uint32_t* ref_off;       /* [n_slots] Variant::ref = seq_pool[ref_off, ref_off+ref_len) */
  const uint32_t* ref_len;
  const uint32_t* alt_off;       /* Variant::alt likewise */
  const uint32_t* alt_len;
  const uint32_t* var_flags;     /* VS_VAR_* */
  const uint64_t* car_begin;     /* [n_slots] first carrier of the slot */
  const uint32_t* car_count;     /* [n_slots] Variant::samples.size() */
  uint64_t n_carriers;
  const uint32_t* carriers;      /* sample id | gt << 29, s_info order; NULL when carriers were not fetched.  (In HBM the
                                  * arena holds 16-bit words for cohorts of at most 4032 samples; the copy widens them.) */
  const char* seq_pool;          /* index-owned: one character per base */
} vs_result_view;

/* The RAW host copy: the result exactly as it lies in HBM -- per-region arrays, the variant table (32-byte rows) and, on
 * request, the carrier arena -- copied with two transfers into page-locked memory owned by the result.  No repacking:
 * region q reports rows [row_begin[q], row_begin[q] + row_count[q]) of the table (ranges of different regions overlap
 * when `shared`), a row's carriers are arena[car_begin .. car_begin + VS_ROW_COUNT) in units of carrier_bytes
 * (2: id | gt << 13, VS_CARRIER16_*; 4: id | gt << 29, VS_CARRIER_*).  This is the form to use when results leave the GPU
 * in bulk; vs_result_get_view below expands it per region into the structure-of-arrays of round 1. */
typedef struct {
  uint32_t pos;                 /* Variant::var_pos */
  uint32_t ref_off, ref_len;    /* Variant::ref = seq_pool[ref_off, ref_off + ref_len) */
  uint32_t alt_off, alt_len;    /* Variant::alt likewise */
  uint32_t count_flags;         /* VS_ROW_COUNT carriers | VS_ROW_DROPPED */
  uint64_t car_begin;           /* first carrier of the row in the arena */
} vs_variant_row;
#define VS_ROW_COUNT(row) ((row).count_flags & 0x7FFFFFFFu)
#define VS_ROW_DROPPED(row) ((row).count_flags >> 31)
#define VS_CARRIER16_ID(c) ((uint32_t)(c) & 0x1FFFu)
#define VS_CARRIER16_GT(c) ((uint32_t)(c) >> 13)
typedef struct {
  uint64_t n_regions;
  const uint8_t* region_flags;   /* [n_regions] */
  const uint64_t* row_begin;     /* [n_regions] first table row of each region */
  const uint64_t* row_count;     /* [n_regions] rows it reports (including dropped ones) */
  const uint64_t* var_count;     /* [n_regions] variants the reference reports */
  const uint64_t* car_base;      /* [n_regions] arena offset of the region's first row (NULL: shared bit 2) */
  const uint64_t* car_len;       /* [n_regions] arena extent of the region's rows (NULL: shared bit 2) */
  uint64_t n_rows;
  const vs_variant_row* rows;    /* [n_rows], page-locked */
  uint64_t arena_entries;
  uint32_t carrier_bytes;        /* 2 or 4 */
  const void* arena;             /* [arena_entries], page-locked; NULL when carriers were not copied */
  const char* seq_pool;
  int shared;                    /* bit 2: lists shared per VERTEX (query types 4 / 5): a region's carriers are not one arena
                                  * range -- car_base / car_len are NULL, rows[].car_begin alone addresses the lists;
                                  * bit 0: rows and lists shared between regions (vs_result_layout); bit 1: `arena` is the
                                  * handle's host mirror of the index's RESIDENT carrier lists ("resident_lists"): nothing
                                  * but the rows was copied for this result, and the pointer stays valid until the index
                                  * is closed */
} vs_result_raw;
int vs_result_get_raw(vs_result* r, int with_carriers, vs_result_raw* raw);

/* Duration of the result's carrier expansion by its OWN pair of HIP events on the stream the kernel ran on (waits for the
 * kernel): every type-6 batch that shares rows and lists carries one, as does every "async_fill" batch; -1 for the other
 * result forms (vs_index_last_timing().ms_fill has it then).
 * "async_submit" (default 1): a type-6 batch of more than 64 regions returns when it is ENQUEUED -- sizes known (or, option "t6_speculate", taken from the handle's previous batch and settled when the result is first asked for anything), buffers
 * allocated, last kernel launched.  Everything that reads the result is ordered behind the batch on the handle's stream
 * (copies, digests, packs, the collective) or waits for it (this call, vs_index_last_timing); freeing it early is safe.
 * "async_fill" (default 0): the call returns as soon as rows and per-region arrays are in HBM while the expansion runs
 * on the handle's second stream beside the next batch's plan and rows; accessors that read carriers wait by themselves. */
int vs_result_fill_ms(vs_result* r, float* ms);

/* Type 6 with delivery: the (sorted) batch is answered in chunks of `chunk_regions`, and while one chunk is computed the
 * raw copy of the previous one crosses PCIe on a second stream into page-locked memory; `fn(user, first_region, raw)` is
 * called once per chunk, in order, with a raw view that is valid during the call (return non-zero to stop). */
typedef int (*vs_chunk_fn)(void* user, uint64_t first_region, const vs_result_raw* chunk);
int vs_query_var_in_ref_stream(vs_index* idx, const vs_region* regions, uint64_t n, uint64_t chunk_regions, int with_carriers,
                               vs_chunk_fn fn, void* user);

/* Copy the result to host memory (owned by the vs_result).  with_carriers = 0
 * leaves the carrier lists in HBM (view->carriers == NULL). */
int vs_result_get_view(vs_result* r, int with_carriers, vs_result_view* view);
/* Totals without any copy of the arrays. */
int vs_result_totals(const vs_result* r, uint64_t* n_regions, uint64_t* n_variants, uint64_t* n_carriers,
                     uint64_t* n_bases);
/* How the result lies in HBM: rows the regions report in total, rows of the variant table, arena entries in use (lists
 * padded to groups of 8), carrier lists actually expanded, and whether rows and lists are SHARED: a type-6 batch of
 * overlapping regions holds one row and one carrier list per site it covers, and every region reporting the site
 * refers to them (its rows are a range of the shared table) -- the way REF / ALT are references into the sequence
 * pool.  (A batch that is not sorted by start is sorted on the device for this and answered in the caller's order.)
 * Views, texts, digests and totals are per region and unaffected.  With resident carrier lists ("resident_lists") a
 * result owns no arena: arena_entries and lists_expanded are 0. */
int vs_result_layout(const vs_result* r, uint64_t* n_slots, uint64_t* table_rows, uint64_t* arena_entries, uint64_t* lists_expanded,
                     int* shared);
/* The `-o` file of region q (print_header + print_var, query.h:38-50) as text owned by the result. */
int vs_result_format_region(vs_result* r, uint64_t q, const char** text, uint64_t* len);
/* Order-independent 64-bit digest of (region, pos, ref, alt, carriers) computed
 * on the device -- the "checksum of checksums" used by full-size property tests. */
int vs_result_digest(vs_result* r, uint64_t* digest);
/* Hit-list records for a collective over the shards of a batch (all-gatherv):
 * writes n_slots records of 4 x uint64 into DEVICE memory at device_dst
 *   {pos | dropped<<63, ref_off | ref_len<<32, alt_off | alt_len<<32, (region_base+region) | car_count<<32}.
 * device_dst == NULL only reports the record count. */
int vs_result_pack_headers(vs_result* r, void* device_dst, uint64_t capacity_records, uint64_t region_base,
                           uint64_t* n_records);
/* Compact hit lists (query type 6): because every rank holds the same index, a region's variant list is
 * its range of the position-ordered site table.  n_regions records of 4 x uint64 in DEVICE memory:
 *   {region_base+q, first_site | region_flags<<32 | has_dropped<<40, sites | variants reported<<32, carriers}.
 * (A region with has_dropped set lost entries to the reference's duplicate rule: fewer variants reported than
 * sites; vs_query_expand_site_ranges applies the rule again.)  device_dst == NULL only reports the record count.
 * Results of the other query types pack per-region SUMMARIES in the same 32 bytes -- what the reference's driver prints
 * per region (src/commands.cc:150-193) and what a sharded run gathers: types 4, 5, 1, 7 the same fields (flags incl.
 * VS_REGION_NOT_FOUND of the point queries, variants reported, carriers; the site fields mean nothing there); types 2, 3
 *   {region_base+q, region_flags<<32, pieces, bytes of the sequence}. */
int vs_result_pack_regions(vs_result* r, void* device_dst, uint64_t capacity_records, uint64_t region_base,
                           uint64_t* n_records);
void vs_result_free(vs_result* r);

/* ---- multi-GPU: the hit-list collective (one process per GPU, RCCL over xGMI) ----
 * north_star: "a batch of thousands of independent region queries shards trivially across the 8 GPUs of one node with
 * an RCCL all-gatherv of hit lists over xGMI".  The reference's loop over the regions is serial and single-process
 * (src/commands.cc:145); these entry points are what its query_main would call once per batch after sharding the sorted
 * region list into contiguous pieces.  RCCL is loaded at run time: VS_ERR_UNSUPPORTED when
 * no librccl.so can be found.
 *   vs_comm_unique_id   rank 0 makes the id (VS_COMM_ID_BYTES bytes) and hands it to the other ranks by whatever means
 *                       the host program has (a file, a pipe, MPI, a torch broadcast)
 *   vs_comm_init        every rank, with the handle whose device it computes on (ncclCommInitRank: collective)
 *   vs_comm_allgather_regions   packs the result's per-region records (vs_result_pack_regions' format) and all-gathers
 *                       them, padded to max_count records per rank: device_dst receives world x max_count records, rank k's
 *                       at record k * max_count, of which the first (regions of rank k) are valid.  async_op != 0: returns
 *                       once the collective is enqueued (on the communicator's own stream, behind the result's kernels);
 *                       vs_comm_wait -- or the next vs_comm_allgather_regions -- waits for it.
 *   Any rank can then rebuild rows and carrier lists of the whole batch from the records: vs_query_expand_site_ranges. */
#define VS_COMM_ID_BYTES 128
typedef struct vs_comm vs_comm;
int vs_comm_unique_id(void* id_out);
int vs_comm_init(vs_index* idx, int rank, int world, const void* id, vs_comm** out);
int vs_comm_allgather_regions(vs_comm* c, vs_result* r, uint64_t region_base, uint64_t max_count, void* device_dst, int async_op);
/* the same into HOST memory (world x max_count records; synchronous) for callers that hold no device memory of their own */
int vs_comm_allgather_regions_host(vs_comm* c, vs_result* r, uint64_t region_base, uint64_t max_count, void* host_dst);
int vs_comm_wait(vs_comm* c);
/* what the communicator is: the rank and world size it was made with and the number of ranks RCCL itself reports for it
 * (ncclCommCount) -- a self-check for launchers: the three agree or the ranks did not all join the same communicator */
int vs_comm_info(vs_comm* c, int* rank, int* world, int* rccl_ranks);
void vs_comm_destroy(vs_comm* c);

/* ---- switches of one handle ----
 * The environment is read once when a handle is opened; afterwards only this call changes a
 * switch.  The production library has ELEVEN keys:
 *   "latency_server"  0 never / 1 for back-to-back streaks of small queries (default) / 2 from the first small query
 *   "server_blocks"   1..64 blocks of the resident server
 *   "share_lists"     1 (default): a type-6 batch of more than 64 regions holds one row and one carrier list per covered
 *                     site, shared by the regions that report it (type 4 / 5: one list per reported vertex); 0: private rows
 *                     and lists per region
 *   "resident_lists"  1 = expand every carrier list of the index ONCE into an arena that stays in HBM with the handle (2 or
 *                     4 bytes per carrier record; VS_ERR_UNSUPPORTED when that does not fit): batches of query types 6 and 4
 *                     then emit rows that point into it, expand nothing and own no arena, and a raw copy moves the rows only
 *                     (default 0; VS_RESIDENT_LISTS=1 in the environment builds it when the handle is opened)
 *   "async_submit"    see vs_result_fill_ms (default 1)
 *   "async_fill"      see vs_result_fill_ms (default 0)
 *   "t6_speculate"    1 (default): a type-6 batch that returns when it is enqueued (async_submit) does not wait for its plan's totals
 *                     either when the handle's previous shared batch had about as many regions (4/5 .. 5/4): variant table and arena
 *                     are sized from that batch (+ 1/8), the kernels behind the plan read the totals in device memory, and a batch
 *                     that does not fit (or whose regions are not sorted) is refused on the device and run again with the exact
 *                     sizes the first time its result is asked for anything -- vs_index_info.t6_speculated / t6_refused count
 *                     them.  Same answers; the host never waits between two batches of a stream of like batches.  0: every batch
 *                     waits for its totals (rounds 1-5)
 *   "t4_walk"         the walk of the query types that follow one sample's path: 2 cooperative (8 lanes per region, a region's
 *                     events walked in parallel: types 4, 2 and 3; default), 1 one lane per region jumping over uneventful
 *                     ref-path runs, 0 literal (type 4: every vertex of the sample's path; types 2 / 3 / 5 as 1)
 *   "t4_rows_max_mb"  the per-sample event and hold rows of query type 4 (vs_index_info.t4_rows_bytes: 7.6 GB for 2504
 *                     samples over chr1) on an OPEN handle: rows larger than the value in MiB are dropped (0: always -- the walks
 *                     then visit every vertex, same answers), absent rows are built when they fit it and half of the free
 *                     memory.  Several handles on one GPU: the caller decides which of them keeps its rows.  Waits for the
 *                     device before it frees anything.
 *   "phase_events"    1 = batches of query types 4 and 5 record all five phase events, so that vs_index_last_timing reports their
 *                     phases (walk, sizes, rows, expansion); default 0: first and last event only -- ms_total, phases 0 -- because
 *                     every event is a packet between two kernels of a string of dependent launches (~3 us each)
 *   "force_fallbacks" 1 = query types 2 - 5 take the count-then-emit pair of walks they fall back to when a region outgrows
 *                     the capacity of its recording walk (tests of that path)
 *   "burden_chunk"    rows of a region one workgroup of the burden kernel walks (vs_query_sample_burden): a region with more is
 *                     split between several, which add to its cells with atomics.  0 (default): 4096; else 64..65536
 *   "window_chunk"    rows of a region one wave of the window-statistics kernel walks (vs_query_window_stats): a region with more is
 *                     split between workgroups, which add to its records with integer atomics.  0 (default): 4096; else 64..65536
 *   "matrix_max_mib"  the largest genotype matrix (vs_query_genotype_matrix; also an LD batch's matrix + band, the records of
 *                     vs_query_group_counts, the temporary counts + records of vs_query_window_stats, the cells + records of vs_query_assoc_scan and the buffers of vs_query_sample_scores), in MiB, a batch may ask for.  0 (default): 32 GiB
 *   "assoc_lds_max_kib" the largest phenotype table (columns x traits rounded up to 1, 2, 4 or 8, x 4 bytes) the kernel of
 *                     vs_query_assoc_scan stages in LDS, in KiB; a larger one is read through global memory.  0 (default): 32; else
 *                     1..128 (small cohorts reach the global form with 1).  The scores are the same bytes in either form
 *   "score_chunk"     table rows one workgroup of the score kernel walks (vs_query_sample_scores).  0 (default): 4096; else 64..65536
 *   "gram_chunk"      table rows one workgroup of the Gram kernel sums (vs_query_sample_gram).  0 (default): by the batch's shape,
 *                     about 256 workgroups; else 64..65536.  The sums are the same integers under every setting
 *   "score_matrix_chunk" table rows one workgroup of the score-matrix kernel sums (vs_query_score_matrix).  0 (default): by the
 *                     batch's shape, about 1024 workgroups; else a multiple of 128 in 128..65536.  The sums are the same integers
 *                     under every setting
 *   "ibs_chunk"       table rows one workgroup of the IBS kernel sums (vs_query_sample_ibs).  0 (default): by the batch's shape,
 *                     about 128 workgroups; else 64..65536.  The sums are the same integers under every setting
 *   "trio_chunk"      trios one workgroup of the trio kernel takes (vs_query_trio_scan).  0 (default): by the batch's shape, all of
 *                     them unless the row blocks give fewer than 2048 workgroups; else a multiple of 64 in 64..16384.  The sums are
 *                     the same integers under every setting
 *   "score_tile_cols" columns of a workgroup's tile of the score kernel: 0 (default): all that 64 KiB of int64 cells hold,
 *                     65536 / (8 Kp); else a multiple of 16 in 16..65536, held to that (small cohorts reach tile boundaries with it).
 *                     The sums are the same integers under every setting of the two
 *   "matrix_tile_cols" columns of a workgroup's tile of the matrix kernel: 0 (default): 4096; else a multiple of 16 in 16..65536
 *                     (small cohorts reach tile boundaries with it)
 * Tuning builds (VS_BUILD_TUNING=1 python -m variantstore_amd.build --force) add "lat_debug", "fill_fused", "fill_chunk",
 * "fill_stats", "walk_stats", "fill_ablate", "fill_lds_pad"; VS_ERR_UNSUPPORTED in the production library, whose kernels
 * do not carry the code. */
int vs_index_set_option(vs_index* idx, const char* key, int64_t value);

/* ---- timing of the last batch on this handle ----
 * Batches of more than 64 regions and every other query type: HIP events on the engine's stream.
 * Type-6 batches of at most 64 regions (latency path: no events on the critical path): host clock --
 *   ms_total call -> result resident, ms_bounds sizing + result slab, ms_scan posting the request / the launch call,
 *   ms_emit waiting for the completion word, ms_fill 0 (the kernel's duration by the device clock under VS_LAT_DEBUG),
 *   fill_launches 0 when the resident query server answered, 1 when a kernel was launched for the call. */
typedef struct {
  float ms_total;    /* first launch to last kernel completion */
  float ms_bounds;   /* rank / region-bounds kernel            */
  float ms_scan;     /* offset scan (+ the host round trip for the sizes) */
  float ms_emit;     /* variant-header kernel                  */
  float ms_fill;     /* carrier-expansion kernel (dominant)    */
  uint64_t fill_launches;
} vs_timing;
int vs_index_last_timing(const vs_index* idx, vs_timing* t);

#ifdef __cplusplus
}
#endif
#endif
