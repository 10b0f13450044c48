// variantstore -- drop-in command line for the query path, on top of the C ABI.
//
// Same sub-commands, flags, log lines and output files as the reference driver
// (reference src/variantstore.cc:81-156 clipp grammar, src/commands.cc:33-60 construct_main,
// :64-93 read_regions, :114-215 query_main, src/util.cc:67-80 print_time_elapsed; log lines in
// spdlog's default pattern "[Y-m-d H:M:S.ms] [level] msg").  All seven query types run on the GPU
// through include/variantstore_hip.h.
//
// Extensions for batches that do not fit a command line:
//   -r @FILE            one "<start>:<end>" (or "<start>") per line instead of a comma list
//   --batch-out FILE    rows of ALL regions ("#region <i> <x>:<y>" before each), since the
//                       reference's -o file only ever holds the last region (query.h:774-781)
//   --device N          GPU ordinal (default 0)
//   --resident-lists    expand every carrier list of the index once, when it is opened, into an arena that stays in
//                       HBM (vs_index_set_option "resident_lists"): batches then copy rows only across PCIe
//   --nprocs N          any query type (1 - 7: the dispatch of src/commands.cc:150-193) as N PROCESSES, one per GPU (device ..
//                       device + N - 1): the parent forks before anything touches a GPU, every rank answers its contiguous shard
//                       of the sorted region list, the ranks all-gather the per-region records (counts and flags: what the
//                       reference prints per region) through the C ABI's collective (vs_comm_*: RCCL over xGMI; the unique id
//                       travels through a file) and rank 0 prints the log lines of ALL regions from the gathered records;
//                       --batch-out text is written per rank and concatenated in rank order, -o holds the last region's
//                       text (the last FOUND position's for types 1 and 7).  A rank that fails ends the others.  --ngpus
//                       (threads in one process, no collective) remains the fallback.
//   --nprocs-same-device  TEST-ONLY: every rank of --nprocs opens GPU `--device` (real RCCL refuses two ranks on one device:
//                       tests load tests/native/fake_rccl.cpp through VS_RCCL_LIB to run the multi-rank code on a one-GPU box)
//   --ngpus N           shard the sorted region list over GPUs device .. device + N - 1 (query types 4, 5, 6): one handle
//                       and one host thread per GPU, contiguous shards (the reference's serial loop, commands.cc:145,
//                       carries no state between regions), results printed in region order
#include <sys/stat.h>
#include <sys/time.h>
#include <sys/wait.h>
#include <signal.h>
#include <unistd.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <thread>
#include <tuple>
#include <unordered_map>
#include <vector>
#include "variantstore_hip.h"

namespace {

void log_line(const char* level, const std::string& msg) {
  struct timeval tv;
  gettimeofday(&tv, nullptr);
  struct tm tm;
  localtime_r(&tv.tv_sec, &tm);
  char ts[64];
  strftime(ts, sizeof(ts), "%Y-%m-%d %H:%M:%S", &tm);
  printf("[%s.%03d] [%s] %s\n", ts, (int)(tv.tv_usec / 1000), level, msg.c_str());
  fflush(stdout);
}
void info(const std::string& m) { log_line("info", m); }
void error(const std::string& m) { log_line("error", m); }

[[noreturn]] void die(int rc, const char* what) {
  error(std::string(what) + ": " + vs_strerror(rc) + ": " + vs_last_error());
  abort();
}

// std::stoi semantics of read_regions (commands.cc:64-93): throws std::invalid_argument on garbage
uint64_t stoi_like(const std::string& s) { return (uint64_t)std::stoi(s); }

std::vector<std::tuple<uint64_t, uint64_t>> read_regions(std::string region) {
  std::vector<std::tuple<uint64_t, uint64_t>> regions;
  if (!region.empty() && region[0] == '@') {
    std::ifstream in(region.substr(1));
    if (!in) throw std::runtime_error("cannot open region file " + region.substr(1));
    std::string line;
    while (std::getline(in, line)) {
      if (line.empty()) continue;
      auto p = line.find(':');
      if (p == std::string::npos) regions.emplace_back(stoi_like(line), 0);
      else regions.emplace_back(stoi_like(line.substr(0, p)), stoi_like(line.substr(p + 1)));
    }
  } else {
    auto pos = region.find(',');
    while (true) {
      std::string token = region.substr(0, pos);
      auto pos2 = token.find(':');
      uint64_t beg = 0, end = 0;
      if (pos2 == std::string::npos) beg = stoi_like(token);
      else { end = stoi_like(token.substr(pos2 + 1)); beg = stoi_like(token.substr(0, pos2)); }
      regions.emplace_back(beg, end);
      if (pos == std::string::npos) break;
      region = region.substr(pos + 1);
      pos = region.find(',');
    }
  }
  std::sort(regions.begin(), regions.end());
  return regions;
}

void print_time_elapsed(const std::string& desc, const timeval& start, timeval end) {  // util.cc:67-80
  if (start.tv_usec > end.tv_usec) { end.tv_usec += 1000000; end.tv_sec--; }
  float t = ((end.tv_sec - start.tv_sec) * 1000000 + (end.tv_usec - start.tv_usec)) / 1000000.f;
  std::cout << desc << "Total Time Elapsed: " << std::to_string(t) << "seconds" << std::endl;
}

bool dir_exists(const std::string& p) {
  struct stat st;
  return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}

struct Args {
  std::string cmd, ref, vcf, prefix, region, outfile, sample, alt, refseq, batch_out, samples_file, groups_file, pheno_file, weights_file, trios_file;
  uint32_t min_ac = 0, max_ac = UINT32_MAX;   // `burden`: the alternate-allele-count window of the rows that count
  uint32_t ld_window = 64;   // `ld`: every row against the next ld_window rows; --dot: dot products instead of r^2
  bool ld_dot = false;
  uint32_t prune_max_bp = 0, prune_threshold = 209715;   // `prune`: --bp, and --r2 as floor(r2 * 2^20 + 0.5) (0.2 by default)
  std::string pvalues_file;   // `clump`: -A, lines of "pos ref alt p"; --p1, --p2: the bounds of the index rows and of the clumped rows
  double clump_p1 = 1e-4, clump_p2 = 1e-2;
  bool gram_grm = false;      // `gram`: the GRM (float64) instead of the dosage products (int64)
  bool ibs_king = false;      // `ibs`: the kinship column beside the counts; --min-kinship X: only pairs with kinship >= X (implies --king)
  bool ibs_have_min = false;
  bool trios_per_trio = false;   // `trios`: one table over the batch, a line per trio, instead of the regions' rows
  uint32_t roh_min_sites = 50, roh_min_bp = 0, roh_max_gap = 0, roh_max_het = 0;   // `roh`: the walk's parameters (--min-ac / --max-ac: the site window)
  bool roh_summary = false;      // `roh`: a line per sample and region instead of a line per segment
  double ibs_min_kinship = 0.0;
  bool assoc_chi2 = false;   // `assoc`: the score test instead of the dot products
  bool windows_no_pairs = false, windows_derived = false;   // `windows`: no pair records; pi, theta, Tajima's D, dxy and Fst beside the integers
  uint32_t type = 0, mode = 0;
  uint64_t hops = 0;
  bool have_hops = false;
  bool have_type = false, have_mode = false, verbose = false;
  int device = 0, ngpus = 1, nprocs = 0;
  bool resident_lists = false;
  bool nprocs_same_device = false;   // test-only (--nprocs-same-device): every rank of --nprocs opens GPU `device`
};

int usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore construct -r <reference-file> -v <vcf-file> -p <output-prefix>\n"
               "        variantstore query -p <output-prefix> -t <query-type> -r <region> -m <mode> [-o <outfile>]\n"
               "                     [-s <sample-name>] [-a <alt-seq>] [-b <ref-seq>] [-v]\n"
               "                     [--batch-out <file>] [--device <n>] [--ngpus <n>] [--nprocs <n>] [--resident-lists]\n"
               "        variantstore draw -p <output-prefix> -r <region> -h <hops> [-s <sample-name>]\n"
               "        variantstore help\n\n"
               "OPTIONS\n"
               "        <query-type>  1  Return closest variant in reference coordinates.\n"
               "                      2  Get sample's sequence in reference coordinates.\n"
               "                      3  Get sample's sequence in sample coordinates.\n"
               "                      4  Get sample's variants in reference coordinates.\n"
               "                      5  Get sample's variants in sample coordinates.\n"
               "                      6  Get variants in reference coordinates.\n"
               "                      7  Return samples with a given mutation.\n"
               "        <region>      <start>:<end>[,<start>:<end>...] or @file with one region per line\n"
               "        <mode>        READ_INDEX_ONLY: 0, READ_COMPLETE_GRAPH: 1 (the index is always resident here)\n";
  return EXIT_FAILURE;
}

int construct_main(const Args& a) {
  info("Creating variant graph");
  vs_construct_stats st;
  vs_index* idx = nullptr;
  // stdout lines of the VariantGraph constructor (variant_graph.h:342-344, 625-626, 729-731, 1919)
  int rc = vs_index_from_vcf(a.ref.c_str(), a.vcf.c_str(), -1, &st, &idx);
  if (rc != VS_OK) die(rc, "construct");
  if (st.use_bit_vector) info("Building sample vector based variant graph.");
  vs_index_info inf;
  vs_index_get_info(idx, &inf);
  info("Adding mutations from: " + a.vcf + " #Samples: " + std::to_string(inf.num_samples - 1));
  info("Num mutations: " + std::to_string(st.num_mutations) + " num mutations-sample: " + std::to_string(st.num_mutations_samples));
  info("Num vars: " + std::to_string(st.num_vars));
  info("Fixing sample indexes in the graph");
  info("Graph stats:");
  info(std::string("Chromosome: ") + vs_index_chr(idx) + " #Vertices: " + std::to_string(st.num_vertices) +
       " #Edges: " + std::to_string(st.num_edges) + " Seq length: " + std::to_string(st.seq_length));
  info("Serializing variant graph to disk");
  info("Number of sample vector classes: " + std::to_string(st.num_classes));
  info("Creating Index");
  info("Serializing index to disk");
  rc = vs_index_save(idx, a.prefix.c_str());
  if (rc != VS_OK) die(rc, "serialize");
  vs_index_close(idx);
  return EXIT_SUCCESS;
}

// read_sequences, commands.cc:96-111
std::vector<std::string> read_sequences(std::string s) {
  std::vector<std::string> seqs;
  auto pos = s.find(',');
  while (true) {
    seqs.push_back(s.substr(0, pos));
    if (pos == std::string::npos) break;
    s = s.substr(pos + 1);
    pos = s.find(',');
  }
  return seqs;
}

// Query types 2 (query_sample_from_ref) and 3 (query_sample_from_sample): commands.cc:156-165.
int sequence_query_main(const Args& a, vs_index* idx, const std::vector<vs_region>& batch) {
  struct timeval start, end;
  gettimeofday(&start, nullptr);
  uint32_t sid = 0;
  if (vs_index_sample_id(idx, a.sample.c_str(), &sid) != VS_OK) { error("Sample not found"); abort(); }  // variant_graph.h:2010-2013
  std::vector<uint32_t> sids(batch.size(), sid);
  vs_result* res = nullptr;
  int rc = vs_query_sample_seq(idx, batch.data(), batch.size(), sids.data(), a.type == 3 ? 1 : 0, &res);
  if (rc != VS_OK) die(rc, "query");
  uint64_t nq = 0;
  const uint8_t* flags = nullptr;
  rc = vs_result_get_sequences(res, &nq, &flags, nullptr, nullptr);
  if (rc != VS_OK) die(rc, "result");
  gettimeofday(&end, nullptr);
  std::ofstream batch_out;
  if (!a.batch_out.empty()) batch_out.open(a.batch_out);
  uint32_t query_num = 0;
  for (uint64_t i = 0; i < nq; ++i) {
    if (a.type == 2) info("2. Get sample's sequence in ref coordinate. " + std::to_string(i));
    else info("3. Get sample's sequence in sample's coordinate. " + std::to_string(i));
    if (flags[i] & VS_REGION_INVALID) {  // an uncaught exception of std::string::substr in the reference
      std::cerr << "terminate called after throwing an instance of 'std::out_of_range'\n";
      abort();
    }
    if (flags[i] & VS_REGION_ENDLESS) {
      error("the reference's backward search does not terminate on region " + std::to_string(batch[i].x) + ":" + std::to_string(batch[i].y));
      return EXIT_FAILURE;
    }
    const char* text = nullptr; uint64_t len = 0;
    if (batch_out.is_open() || a.verbose) {
      rc = vs_result_format_region(res, i, &text, &len);
      if (rc != VS_OK) die(rc, "result");
    }
    if (batch_out.is_open()) {
      batch_out << "#region " << i << " " << batch[i].x << ":" << batch[i].y << "\n";
      batch_out.write(text, len);
    }
    if (a.verbose && i + 1 == nq) {
      std::ofstream out;
      out.open(a.outfile);
      out.write(text, len);
    }
    query_num += 1;
    if (query_num == 10 || query_num == 100 || query_num == 1000) {
      gettimeofday(&end, nullptr);   // cumulative up to this line, as in the reference's loop (commands.cc:196-211)
      print_time_elapsed("Query" + std::to_string(query_num) + ": ", start, end);
    }
  }
  gettimeofday(&end, nullptr);
  print_time_elapsed("Query" + std::to_string(query_num) + ": ", start, end);
  vs_result_free(res);
  vs_index_close(idx);
  return EXIT_SUCCESS;
}

// Query types 1 (closest_var) and 7 (samples_has_var): commands.cc:151-155, 181-189.
int point_query_main(const Args& a, vs_index* idx, const std::vector<vs_region>& batch) {
  struct timeval start, end;
  gettimeofday(&start, nullptr);
  std::vector<uint64_t> positions;
  for (auto& b : batch) positions.push_back(b.x);
  std::vector<std::string> refs, alts;
  std::vector<const char*> refp, altp;
  vs_result* res = nullptr;
  int rc;
  if (a.type == 7) {
    alts = read_sequences(a.alt);
    refs = read_sequences(a.refseq);
    // the reference indexes refs[i]/alts[i] with the position of the region in the SORTED list and does not
    // check the lengths (commands.cc:185); a shorter list is out of bounds there and refused here
    if (refs.size() < batch.size() || alts.size() < batch.size()) {
      error("-a/-b must list one sequence per region");
      vs_index_close(idx);
      return EXIT_FAILURE;
    }
    for (size_t i = 0; i < batch.size(); ++i) { refp.push_back(refs[i].c_str()); altp.push_back(alts[i].c_str()); }
    rc = vs_query_samples_has_var(idx, positions.data(), refp.data(), altp.data(), positions.size(), &res);
  } else {
    rc = vs_query_closest_var(idx, positions.data(), positions.size(), &res);
  }
  if (rc != VS_OK) die(rc, "query");
  vs_result_view v;
  rc = vs_result_get_view(res, 0, &v);
  if (rc != VS_OK) die(rc, "result");
  gettimeofday(&end, nullptr);
  std::ofstream batch_out;
  if (!a.batch_out.empty()) batch_out.open(a.batch_out);
  uint32_t query_num = 0;
  for (uint64_t i = 0; i < v.n_regions; ++i) {
    const bool found = !(v.region_flags[i] & VS_REGION_NOT_FOUND);
    if (a.type == 1) info("1. return closest mutation in ref coordinate. " + std::to_string(i));
    else {
      info("7. Get samples have given variant. " + std::to_string(i));
      info("Looking for variant POS: " + std::to_string(positions[i]) + ", REF: " + refs[i] + ", ALT: " + alts[i]);
      if (!found) error("There is no such variant!");
    }
    const char* text = nullptr; uint64_t len = 0;
    if (found && (batch_out.is_open() || a.verbose)) {
      rc = vs_result_format_region(res, i, &text, &len);
      if (rc != VS_OK) die(rc, "result");
    }
    if (batch_out.is_open()) {
      batch_out << "#region " << i << " " << positions[i] << (found ? "" : " not-found") << "\n";
      if (found) batch_out.write(text, len);
    }
    if (a.verbose && found) {  // rewritten by every call that finds something: the last one stays
      std::ofstream out;
      out.open(a.outfile);
      out.write(text, len);
    }
    query_num += 1;
    if (query_num == 10 || query_num == 100 || query_num == 1000) {
      gettimeofday(&end, nullptr);   // cumulative up to this line, as in the reference's loop (commands.cc:196-211)
      print_time_elapsed("Query" + std::to_string(query_num) + ": ", start, end);
    }
  }
  gettimeofday(&end, nullptr);
  print_time_elapsed("Query" + std::to_string(query_num) + ": ", start, end);
  vs_result_free(res);
  vs_index_close(idx);
  return EXIT_SUCCESS;
}

// `variantstore draw` (commands.cc:217-242): <prefix>/graph.dot for the neighbourhood of the vertex at the region's
// start.  The reference's option grammar stores -s into the QUERY options (variantstore.cc:146-150), so its draw
// always starts from the reference path; the same here.
int draw_main(const Args& a) {
  info("Loading Index ...");
  info("Loading variant graph ...");
  info("Read complete graph ..");
  vs_index* idx = nullptr;
  int rc = vs_index_open(a.prefix.c_str(), -1, &idx);   // host-only: nothing here runs on the GPU
  if (rc != VS_OK) die(rc, "load");
  vs_index_info inf;
  vs_index_get_info(idx, &inf);
  info("Graph stats:");
  info(std::string("Chromosome: ") + vs_index_chr(idx) + " #Vertices: " + std::to_string(inf.num_topology_keys) +
       " #Edges: 0 Seq length: " + std::to_string(inf.seq_length));
  auto regions = read_regions(a.region);
  info("Looking up vertex corresponding to the queried region");
  rc = vs_index_draw_subgraph(idx, std::get<0>(regions[0]), a.hops, "ref", (a.prefix + "/graph.dot").c_str());
  if (rc != VS_OK) die(rc, "draw");
  vs_index_close(idx);
  return EXIT_SUCCESS;
}

// `--nprocs N`: one process per GPU and the collective of the C ABI (see the header comment), for every query type the
// reference's loop dispatches (src/commands.cc:150-193).  The sorted region list is cut into contiguous shards, every rank
// answers its shard with the type's own entry point, the per-region records (vs_result_pack_regions: counts and flags --
// all the reference prints per region) are all-gathered through vs_comm_*, rank 0 prints the log lines of EVERY region from
// the gathered records, and the ranks' shards of the --batch-out text are put together by the parent.
int query_multiproc_main(const Args& a) {
  auto regions = read_regions(a.region);
  if (a.type < 1 || a.type > 7) {
    for (size_t i = 0; i < regions.size(); ++i) error("Unsupported query type");  // commands.cc:191
    return EXIT_SUCCESS;
  }
  std::vector<vs_region> batch;
  for (auto& r : regions) batch.push_back(vs_region{std::get<0>(r), std::get<1>(r)});
  std::vector<std::string> refs, alts;
  if (a.type == 7) {
    alts = read_sequences(a.alt);
    refs = read_sequences(a.refseq);
    if (refs.size() < batch.size() || alts.size() < batch.size()) { error("-a/-b must list one sequence per region"); return EXIT_FAILURE; }
  }
  const int world = (int)std::min<size_t>((size_t)a.nprocs, std::max<size_t>(batch.size(), 1));
  char tmpl[] = "/tmp/vs_nprocs_XXXXXX";
  if (!mkdtemp(tmpl)) { error("cannot create a temporary directory"); return EXIT_FAILURE; }
  const std::string dir = tmpl, uid_file = dir + "/uid";
  auto shard = [&](int k, size_t* lo, size_t* hi) {
    const size_t base = batch.size() / world, rem = batch.size() % world;
    *lo = k * base + std::min<size_t>(k, rem);
    *hi = *lo + base + ((size_t)k < rem ? 1 : 0);
  };
  size_t max_count = 0;
  for (int k = 0; k < world; ++k) { size_t lo, hi; shard(k, &lo, &hi); max_count = std::max(max_count, hi - lo); }
  std::vector<pid_t> kids;
  fflush(stdout);
  for (int rank = 0; rank < world; ++rank) {
    const pid_t pid = fork();   // (nothing in this process has touched a GPU)
    if (pid < 0) { error("fork failed"); return EXIT_FAILURE; }
    if (pid > 0) { kids.push_back(pid); continue; }
    // ---- rank `rank` ----
    struct timeval start, end;
    if (rank == 0) { info("Loading Index ..."); info("Loading variant graph ..."); info(a.mode == 0 ? "Read index only .." : "Read complete graph .."); }
    vs_index* idx = nullptr;
    int rc = vs_index_open(a.prefix.c_str(), a.nprocs_same_device ? a.device : a.device + rank, &idx);
    if (rc != VS_OK) die(rc, "load");
    if (const char* k = getenv("VS_NPROCS_TEST_KILL_RANK"))   // TEST-ONLY: this rank dies the hard way before it joins the communicator
      if (*k && atoi(k) == rank) raise(SIGKILL);
    if (rank == 0) {
      vs_index_info inf;
      vs_index_get_info(idx, &inf);
      info("Graph stats:");
      info(std::string("Chromosome: ") + vs_index_chr(idx) + " #Vertices: " + std::to_string(inf.num_topology_keys) +
           " #Edges: 0 Seq length: " + std::to_string(inf.seq_length));
    }
    if (a.resident_lists && vs_index_set_option(idx, "resident_lists", 1) != VS_OK)
      log_line("warning", std::string("--resident-lists: ") + vs_last_error() + " (lists are expanded per batch)");
    uint32_t sid = 0;
    if (a.type >= 2 && a.type <= 5 && vs_index_sample_id(idx, a.sample.c_str(), &sid) != VS_OK) {   // variant_graph.h:2010-2013
      if (rank == 0) error("Sample not found");
      _exit(EXIT_FAILURE);
    }
    // the communicator: rank 0 makes the unique id, the others wait for its file
    unsigned char uid[VS_COMM_ID_BYTES];
    if (rank == 0) {
      rc = vs_comm_unique_id(uid);
      if (rc != VS_OK) die(rc, "vs_comm_unique_id");
      std::ofstream f(uid_file + ".tmp", std::ios::binary);
      f.write((const char*)uid, sizeof(uid));
      f.close();
      rename((uid_file + ".tmp").c_str(), uid_file.c_str());
    } else {
      for (int tries = 0;; ++tries) {
        std::ifstream f(uid_file, std::ios::binary);
        if (f && f.read((char*)uid, sizeof(uid))) break;
        if (tries > 60000) { error("no unique id from rank 0"); _exit(EXIT_FAILURE); }
        usleep(2000);
      }
    }
    vs_comm* comm = nullptr;
    {   // RCCL prints a version banner through C stdio when a communicator is made: stdout is the reference's log, so file
        // descriptor 1 points at stderr for the duration of the call
      fflush(stdout);
      const int saved = dup(1);
      dup2(2, 1);
      rc = vs_comm_init(idx, rank, world, uid, &comm);
      fflush(stdout);
      dup2(saved, 1);
      close(saved);
    }
    if (rc != VS_OK) die(rc, "vs_comm_init");
    size_t lo, hi;
    shard(rank, &lo, &hi);
    const uint64_t n = hi - lo;
    gettimeofday(&start, nullptr);
    vs_result* res = nullptr;
    if (a.type == 6) rc = vs_query_var_in_ref(idx, batch.data() + lo, n, &res);
    else if (a.type == 4) rc = vs_query_sample_var_in_ref(idx, batch.data() + lo, n, sid, &res);
    else if (a.type == 5) { std::vector<uint32_t> sids(n, sid); rc = vs_query_sample_var_in_sample(idx, batch.data() + lo, n, sids.data(), &res); }
    else if (a.type == 2 || a.type == 3) { std::vector<uint32_t> sids(n, sid); rc = vs_query_sample_seq(idx, batch.data() + lo, n, sids.data(), a.type == 3 ? 1 : 0, &res); }
    else {
      std::vector<uint64_t> positions;
      for (size_t i = lo; i < hi; ++i) positions.push_back(batch[i].x);
      if (a.type == 7) {
        std::vector<const char*> refp, altp;
        for (size_t i = lo; i < hi; ++i) { refp.push_back(refs[i].c_str()); altp.push_back(alts[i].c_str()); }
        rc = vs_query_samples_has_var(idx, positions.data(), refp.data(), altp.data(), n, &res);
      } else rc = vs_query_closest_var(idx, positions.data(), n, &res);
    }
    if (rc != VS_OK) die(rc, "query");
    std::vector<uint64_t> recs((size_t)world * max_count * 4);
    rc = vs_comm_allgather_regions_host(comm, res, lo, max_count, recs.data());
    if (rc != VS_OK) die(rc, "vs_comm_allgather_regions_host");
    const bool point = a.type == 1 || a.type == 7;
    auto own_flags = [&](size_t k) { return (recs[((size_t)rank * max_count + k) * 4 + 1] >> 32) & 0xFF; };
    if (!a.batch_out.empty()) {   // this rank's shard of the text
      std::ofstream out(dir + "/out." + std::to_string(rank));
      for (size_t k = 0; k < n; ++k) {
        const bool found = !(own_flags(k) & VS_REGION_NOT_FOUND);
        if (point) out << "#region " << (lo + k) << " " << batch[lo + k].x << (found ? "" : " not-found") << "\n";
        else out << "#region " << (lo + k) << " " << batch[lo + k].x << ":" << batch[lo + k].y << "\n";
        const char* text; uint64_t len;
        if ((!point || found) && vs_result_format_region(res, k, &text, &len) == VS_OK) out.write(text, len);
      }
    }
    if (a.verbose) {   // the -o file: the last region's text (query.h:774-781) -- the last FOUND one for the point queries; a rank that
                       // holds a candidate leaves it for the parent, which keeps the highest rank's
      size_t last = n;
      for (size_t k = n; k-- > 0;)
        if (!point || !(own_flags(k) & VS_REGION_NOT_FOUND)) { last = k; break; }
      const char* text; uint64_t len;
      if (last < n && (point || hi == batch.size()) && vs_result_format_region(res, last, &text, &len) == VS_OK) {
        std::ofstream out(dir + "/last." + std::to_string(rank));
        out.write(text, len);
      }
    }
    int status = EXIT_SUCCESS;
    if (rank == 0) {   // the log lines of every region, from the gathered records
      uint32_t query_num = 0;
      for (int k = 0; k < world && status == EXIT_SUCCESS; ++k) {
        size_t klo, khi;
        shard(k, &klo, &khi);
        for (size_t j = 0; j < khi - klo && status == EXIT_SUCCESS; ++j) {
          const uint64_t* rec = &recs[((size_t)k * max_count + j) * 4];
          const uint64_t i = rec[0], flags = (rec[1] >> 32) & 0xFF, nvar = rec[2] >> 32;
          switch (a.type) {
            case 1: info("1. return closest mutation in ref coordinate. " + std::to_string(i)); break;
            case 2: info("2. Get sample's sequence in ref coordinate. " + std::to_string(i)); break;
            case 3: info("3. Get sample's sequence in sample's coordinate. " + std::to_string(i)); break;
            case 4: info("4. Get sample's variants in ref coordinate. " + std::to_string(i)); break;
            case 5: info("5. Get sample's variants in sample coordinate. " + std::to_string(i)); break;
            case 6: info("6. Get variants in ref coordinate. " + std::to_string(i)); break;
            default:
              info("7. Get samples have given variant. " + std::to_string(i));
              info("Looking for variant POS: " + std::to_string(batch[i].x) + ", REF: " + refs[i] + ", ALT: " + alts[i]);
              if (flags & VS_REGION_NOT_FOUND) error("There is no such variant!");
          }
          if (!point && (flags & VS_REGION_ENDLESS)) {
            error("the reference's backward search does not terminate on region " + std::to_string(batch[i].x) + ":" + std::to_string(batch[i].y));
            status = EXIT_FAILURE; break;
          }
          if (!point && (flags & VS_REGION_INVALID)) {
            if (a.type == 2 || a.type == 3) std::cerr << "terminate called after throwing an instance of 'std::out_of_range'\n";
            else error("Can't find node corresponding to pos " + std::to_string(batch[i].x));   // index.h:151-154
            status = EXIT_FAILURE; break;
          }
          if (a.type >= 4 && a.type <= 6) {
            const char* label = (a.type == 6 && !(flags & VS_REGION_EMPTY)) ? "get_var_in_ref" : "get_sample_var_in_ref";   // query.h:746
            if (a.type == 5) label = "get_sample_var_in_sample";  // query.h:599
            std::cout << "Number of variants " << label << ": " << nvar << '\n';
          }
          query_num += 1;
          if (query_num == 10 || query_num == 100 || query_num == 1000) {
            gettimeofday(&end, nullptr);
            print_time_elapsed("Query" + std::to_string(query_num) + ": ", start, end);
          }
        }
      }
      gettimeofday(&end, nullptr);
      print_time_elapsed("Query" + std::to_string(query_num) + ": " + (a.type == 6 ? "(query_var_in_ref) " : ""), start, end);
    }
    fflush(stdout);
    vs_result_free(res);
    vs_comm_destroy(comm);
    vs_index_close(idx);
    _exit(status);
  }
  // Whichever rank ends first is reaped first; a rank that fails (no such device, an RCCL error) leaves the others inside
  // ncclCommInitRank or the all-gather for good, so the first abnormal exit ends them all (fresh forks: nothing to save).
  int failed = 0;
  for (size_t left = kids.size(); left > 0; --left) {
    int st = 0;
    const pid_t pid = waitpid(-1, &st, 0);
    if (pid < 0) { failed = 1; break; }
    auto it = std::find(kids.begin(), kids.end(), pid);
    if (it == kids.end()) { ++left; continue; }   // (not one of the ranks)
    *it = -1;
    if (!WIFEXITED(st) || WEXITSTATUS(st) != EXIT_SUCCESS) {
      if (!failed) {
        error("a rank of --nprocs failed; stopping the others");
        for (pid_t other : kids) if (other > 0) kill(other, SIGKILL);
      }
      failed = 1;
    }
  }
  if (!failed && !a.batch_out.empty()) {
    std::ofstream out(a.batch_out, std::ios::binary);
    for (int k = 0; k < world; ++k) {
      std::ifstream in(dir + "/out." + std::to_string(k), std::ios::binary);
      out << in.rdbuf();
    }
  }
  if (!failed && a.verbose)
    for (int k = world; k-- > 0;) {
      std::ifstream in(dir + "/last." + std::to_string(k), std::ios::binary);
      if (!in) continue;
      std::ofstream out(a.outfile, std::ios::binary);
      out << in.rdbuf();
      break;
    }
  for (int k = 0; k < world; ++k) { remove((dir + "/out." + std::to_string(k)).c_str()); remove((dir + "/last." + std::to_string(k)).c_str()); }
  remove(uid_file.c_str());
  rmdir(dir.c_str());
  return failed ? EXIT_FAILURE : EXIT_SUCCESS;
}

int query_main(const Args& a) {
  if (a.nprocs >= 1) return query_multiproc_main(a);
  info("Loading Index ...");
  info("Loading variant graph ...");
  info(a.mode == 0 ? "Read index only .." : "Read complete graph ..");
  vs_index* idx = nullptr;
  int rc = vs_index_open(a.prefix.c_str(), a.device, &idx);
  if (rc != VS_OK) die(rc, "load");
  vs_index_info inf;
  vs_index_get_info(idx, &inf);
  info("Graph stats:");
  info(std::string("Chromosome: ") + vs_index_chr(idx) + " #Vertices: " + std::to_string(inf.num_topology_keys) +
       " #Edges: 0 Seq length: " + std::to_string(inf.seq_length));

  auto regions = read_regions(a.region);
  struct timeval start, end;
  gettimeofday(&start, nullptr);
  if (a.type < 1 || a.type > 7) {
    for (size_t i = 0; i < regions.size(); ++i) error("Unsupported query type");  // commands.cc:191
    vs_index_close(idx);
    return EXIT_SUCCESS;
  }
  std::vector<vs_region> batch;
  for (auto& r : regions) batch.push_back(vs_region{std::get<0>(r), std::get<1>(r)});
  if (a.type == 1 || a.type == 7) return point_query_main(a, idx, batch);
  if (a.type == 2 || a.type == 3) return sequence_query_main(a, idx, batch);
  uint32_t sid = 0;
  if (a.type != 6 && vs_index_sample_id(idx, a.sample.c_str(), &sid) != VS_OK) { error("Sample not found"); abort(); }  // variant_graph.h:2010-2013
  // ---- shards: one per GPU (--ngpus), contiguous pieces of the sorted list ----
  const int ng = (int)std::min<size_t>((size_t)a.ngpus, std::max<size_t>(batch.size(), 1));
  struct Shard { vs_index* idx = nullptr; size_t lo = 0, hi = 0; vs_result* res = nullptr; vs_result_raw v{}; int rc = VS_OK; std::string err; };
  std::vector<Shard> shards(ng);
  shards[0].idx = idx;
  for (int g = 0; g < ng; ++g) {
    const size_t base = batch.size() / ng, rem = batch.size() % ng;
    shards[g].lo = g * base + std::min<size_t>(g, rem);
    shards[g].hi = shards[g].lo + base + ((size_t)g < rem ? 1 : 0);
  }
  auto run_shard = [&](Shard& sh, int g) {
    if (!sh.idx) {
      sh.rc = vs_index_open(a.prefix.c_str(), a.device + g, &sh.idx);
      if (sh.rc != VS_OK) { sh.err = vs_last_error(); return; }
    }
    if (a.resident_lists && vs_index_set_option(sh.idx, "resident_lists", 1) != VS_OK)
      log_line("warning", std::string("--resident-lists: ") + vs_last_error() + " (lists are expanded per batch)");
    const vs_region* rg = batch.data() + sh.lo;
    const uint64_t n = sh.hi - sh.lo;
    if (a.type == 6) sh.rc = vs_query_var_in_ref(sh.idx, rg, n, &sh.res);
    else if (a.type == 4) sh.rc = vs_query_sample_var_in_ref(sh.idx, rg, n, sid, &sh.res);
    else {
      std::vector<uint32_t> sids(n, sid);
      sh.rc = vs_query_sample_var_in_sample(sh.idx, rg, n, sids.data(), &sh.res);
    }
    // the per-region counts and flags are all the log lines need (the raw form: no per-region expansion on the host); when
    // the text of every region is wanted, rows and carriers come over in ONE raw copy (not one copy per region)
    if (sh.rc == VS_OK) sh.rc = vs_result_get_raw(sh.res, a.batch_out.empty() ? 0 : 1, &sh.v);
    if (sh.rc != VS_OK) sh.err = vs_last_error();
  };
  if (ng == 1) run_shard(shards[0], 0);
  else {
    std::vector<std::thread> th;
    for (int g = 0; g < ng; ++g) th.emplace_back(run_shard, std::ref(shards[g]), g);
    for (auto& t : th) t.join();
  }
  for (auto& sh : shards)
    if (sh.rc != VS_OK) { error(std::string("query: ") + vs_strerror(sh.rc) + ": " + sh.err); abort(); }
  gettimeofday(&end, nullptr);

  std::ofstream batch_out;
  if (!a.batch_out.empty()) batch_out.open(a.batch_out);
  uint32_t query_num = 0;
  for (auto& sh : shards) {
    const vs_result_raw& v = sh.v;
    for (uint64_t k = 0; k < v.n_regions; ++k) {
      const uint64_t i = sh.lo + k;
      if (a.type == 6) info("6. Get variants in ref coordinate. " + std::to_string(i));
      else if (a.type == 5) info("5. Get sample's variants in sample coordinate. " + std::to_string(i));
      else info("4. Get sample's variants in ref coordinate. " + std::to_string(i));
      if (v.region_flags[k] & VS_REGION_ENDLESS) {
        error("the reference's backward search does not terminate on region " + std::to_string(batch[i].x) + ":" + std::to_string(batch[i].y));
        return EXIT_FAILURE;
      }
      if (v.region_flags[k] & VS_REGION_INVALID) {  // index.h:151-154
        error("Can't find node corresponding to pos " + std::to_string(batch[i].x));
        abort();
      }
      // query.h:746 prints the type-4 label on the early-out of type 6 as well
      const char* label = (a.type == 6 && !(v.region_flags[k] & VS_REGION_EMPTY)) ? "get_var_in_ref" : "get_sample_var_in_ref";
      if (a.type == 5) label = "get_sample_var_in_sample";  // query.h:599
      std::cout << "Number of variants " << label << ": " << v.var_count[k] << '\n';
      if (batch_out.is_open()) {
        const char* text; uint64_t len;
        if (vs_result_format_region(sh.res, k, &text, &len) == VS_OK) {
          batch_out << "#region " << i << " " << batch[i].x << ":" << batch[i].y << "\n";
          batch_out.write(text, len);
        }
      }
      if (a.verbose && i + 1 == batch.size()) {  // the -o file is reopened (truncated) per region: the last one stays
        const char* text; uint64_t len;
        if (vs_result_format_region(sh.res, k, &text, &len) == VS_OK) {
          std::ofstream out;
          out.open(a.outfile);
          out.write(text, len);
        }
      }
      query_num += 1;
      if (query_num == 10 || query_num == 100 || query_num == 1000) {
        gettimeofday(&end, nullptr);   // cumulative up to this line, as in the reference's loop (commands.cc:196-211)
        print_time_elapsed("Query" + std::to_string(query_num) + ": ", start, end);
      }
    }
  }
  std::string dsc = "Query" + std::to_string(query_num) + ": ";
  if (a.type == 6) dsc.append("(query_var_in_ref) ");
  gettimeofday(&end, nullptr);   // the whole loop, output included: what the reference's last line measures
  print_time_elapsed(dsc, start, end);
  for (auto& sh : shards) {
    vs_result_free(sh.res);
    vs_index_close(sh.idx);
  }
  return EXIT_SUCCESS;
}

// `variantstore counts`: allele counts over the regions (vs_query_allele_counts), for the whole cohort or the samples named in
// the -S file (one name per line).  Every region's text ("Pos Ref Alt Carriers AC HomAlt Phased") goes to -o (stdout without it),
// with a "#region <i> <x>:<y>" line before it, as --batch-out writes type 6.
int counts_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore counts -p <output-prefix> -r <region> [-S <sample-name-file>] [-o <outfile>] [--device <n>]\n\n"
               "        Allele counts (carriers, alternate alleles, homozygous-alternate and phased carriers) of the variants\n"
               "        query type 6 reports in each region, over the whole cohort or over the samples named in the file.\n";
  return EXIT_FAILURE;
}

// `variantstore burden`: the per-sample burden of the regions (vs_query_sample_burden) over the same samples, restricted to the
// rows whose alternate-allele count lies in [--min-ac, --max-ac].  Output as `counts`: "#region <i> <x>:<y>", then the region's
// text ("Sample Variants AC HomAlt Phased", one line per sample that carries a counting variant of the region).
int burden_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore burden -p <output-prefix> -r <region> [-S <sample-name-file>] [--min-ac <n>] [--max-ac <n>]\n"
               "                            [-o <outfile>] [--device <n>]\n\n"
               "        For every region and every sample (of the whole cohort or of those named in the file): the variants of the\n"
               "        region the sample carries, their alternate alleles, homozygous-alternate and phased calls.  Only variants whose\n"
               "        alternate-allele count over those samples lies within --min-ac .. --max-ac count (rare-variant burden).\n";
  return EXIT_FAILURE;
}

// `variantstore genotypes`: the genotype matrix of the regions (vs_query_genotype_matrix) over the same samples.  Output as `counts`:
// "#region <i> <x>:<y>", then the region's text ("Pos Ref Alt" and a column per sample; per reported row `0` or the call).
int genotypes_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore genotypes -p <output-prefix> -r <region> [-S <sample-name-file>] [-o <outfile>] [--device <n>]\n\n"
               "        For every variant query type 6 reports in each region, every sample's call (of the whole cohort or of the\n"
               "        samples named in the file): 0 for a non-carrier, else the genotype as type 6 prints it (1|1, 0/1, ...).\n";
  return EXIT_FAILURE;
}

// `variantstore ld`: banded LD of the regions (vs_query_ld_band) over the same samples.  Output as `counts`: "#region <i> <x>:<y>",
// then the region's text ("PosA RefA AltA PosB RefB AltB R2|Dot", one line per pair of its reported rows at most -w rows apart).
int ld_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore ld -p <output-prefix> -r <region> [-S <sample-name-file>] [-w <window>] [--dot] [-o <outfile>]\n"
               "                        [--device <n>]\n\n"
               "        For every pair of variants query type 6 reports in a region that lie at most <window> rows (default 64, at\n"
               "        most 256) apart: the squared correlation of the samples' alternate-allele dosages (of the whole cohort or of\n"
               "        the samples named in the file), or with --dot the sum of the dosage products.\n";
  return EXIT_FAILURE;
}

// `variantstore groups`: allele counts per sample group (vs_query_group_counts).  The -G file holds one `sample<TAB or space>group` per
// line; the groups are numbered in order of first appearance.  Output as `counts`: "#region <i> <x>:<y>", then the region's text
// ("Pos Ref Alt Group N Carriers AC HomAlt Phased", one line per reported row and group).
int groups_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore groups -p <output-prefix> -r <region> -G <sample-group-file> [-o <outfile>] [--device <n>]\n\n"
               "        Allele counts of the variants query type 6 reports in each region, separately for every group of samples\n"
               "        (cases / controls, populations, batches): the file holds one `sample group` pair per line, at most 64 groups,\n"
               "        a sample in at most one of them; samples that are not listed are counted nowhere.\n";
  return EXIT_FAILURE;
}

// `variantstore windows`: the diversity statistics of every region (vs_query_window_stats) per sample group and pair of groups.  The -G
// file is `groups`'s; without it the whole cohort is one group.  Output as `counts`: "#region <i> <x>:<y>", then the region's text
// ("Group N Rows Seg Singletons Doubletons Private Fixed SumAC SumAC2 ObsHet", a line per group, then "GroupA GroupB SumCross SegUnion
// FixedDiff", a line per pair).  --derived: each group line gains Pi ThetaW TajimaD and each pair line Dxy Fst.
int windows_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore windows -p <output-prefix> -r <region> [-G <sample-group-file>] [--no-pairs] [--derived] [-o <outfile>]\n"
               "                             [--device <n>]\n\n"
               "        For every region (window) and every group of samples -- the file holds one `sample group` pair per line as\n"
               "        for `groups`; without it the whole cohort is one group -- the integers of the windowed diversity statistics:\n"
               "        sites, segregating sites, singletons, doubletons, private and fixed alleles, the sums of the alternate-allele\n"
               "        counts and of their squares, heterozygous calls; and for every pair of groups (unless --no-pairs) the sum of\n"
               "        the products of their counts, sites segregating in either, fixed differences.  --derived adds nucleotide\n"
               "        diversity pi, Watterson's theta and Tajima's D per group and dxy and Hudson's Fst per pair (nan: undefined).\n";
  return EXIT_FAILURE;
}

// pi, theta_w and Tajima's D of a record over a group of n samples (N = 2 n allele copies), and dxy of a pair: the formulas of the
// Python accessor (window_stats_derived), in double from exact integers.
struct WindowDerived { double pi, theta, tajima; };
WindowDerived window_derived(const vs_window_stats& w, uint32_t n) {
  const double nan = std::nan("");
  WindowDerived d{nan, nan, nan};
  const uint64_t N = 2ull * n;
  if (N < 2) return d;
  const unsigned __int128 num = (unsigned __int128)N * w.sum_ac - w.sum_ac2;
  d.pi = 2.0 * (double)num / (double)(N * (N - 1));
  double a1 = 0.0, a2 = 0.0;
  for (uint64_t i = 1; i < N; ++i) { a1 += 1.0 / (double)i; a2 += 1.0 / ((double)i * (double)i); }
  const double S = (double)w.seg;
  d.theta = S / a1;
  if (N < 4 || w.seg == 0) return d;
  const double dn = (double)N;
  const double b1 = (dn + 1) / (3.0 * (dn - 1)), b2 = 2.0 * (dn * dn + dn + 3) / (9.0 * dn * (dn - 1));
  const double c1 = b1 - 1.0 / a1, c2 = b2 - (dn + 2) / (a1 * dn) + a2 / (a1 * a1);
  const double e1 = c1 / a1, e2 = c2 / (a1 * a1 + a2);
  const double var = e1 * S + e2 * S * (S - 1.0);
  if (var > 0) d.tajima = (d.pi - d.theta) / std::sqrt(var);
  return d;
}
double window_dxy(const vs_window_stats& g, const vs_window_stats& h, const vs_window_pair_stats& p, uint32_t n_g, uint32_t n_h) {
  const uint64_t Ng = 2ull * n_g, Nh = 2ull * n_h;
  if (!Ng || !Nh) return std::nan("");
  const unsigned __int128 num = (unsigned __int128)Nh * g.sum_ac + (unsigned __int128)Ng * h.sum_ac - 2 * (unsigned __int128)p.sum_cross;
  return (double)num / (double)(Ng * Nh);
}
std::string g10(double v) {
  if (std::isnan(v)) return "nan";
  char buf[48];
  snprintf(buf, sizeof buf, "%.10g", v);
  return buf;
}

int groups_main(const Args& a, bool windows = false) {
  vs_index* idx = nullptr;
  int rc = vs_index_open(a.prefix.c_str(), a.device, &idx);
  if (rc != VS_OK) die(rc, "load");
  auto fail_with = [&](const std::string& msg) { error(msg); vs_index_close(idx); return EXIT_FAILURE; };
  std::ifstream in;
  if (!windows || !a.groups_file.empty()) {
    in.open(a.groups_file);
    if (!in) return fail_with("cannot open group file " + a.groups_file);
  }
  std::vector<uint32_t> ids, group_of;
  std::vector<std::string> names;
  std::map<uint32_t, uint32_t> seen;   // sample id -> its group
  std::string line;
  while (std::getline(in, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.find_first_not_of(" \t") == std::string::npos) continue;
    const size_t s0 = line.find_first_not_of(" \t"), s1 = line.find_first_of(" \t", s0);
    const size_t g0 = s1 == std::string::npos ? s1 : line.find_first_not_of(" \t", s1);
    if (g0 == std::string::npos) return fail_with("no group on the line: " + line);
    const std::string sample = line.substr(s0, s1 - s0);
    std::string group = line.substr(g0);
    group.erase(group.find_last_not_of(" \t") + 1);
    uint32_t sid = 0;
    if (vs_index_sample_id(idx, sample.c_str(), &sid) != VS_OK || sid == 0) return fail_with("Sample not found: " + sample);
    uint32_t g = (uint32_t)(std::find(names.begin(), names.end(), group) - names.begin());
    if (g == names.size()) {
      if (names.size() == VS_GROUPS_MAX) return fail_with("more than " + std::to_string(VS_GROUPS_MAX) + " groups in " + a.groups_file);
      names.push_back(group);
    }
    const auto it = seen.find(sid);
    if (it != seen.end() && it->second != g) return fail_with("sample " + sample + " is in two groups: " + names[it->second] + " and " + group);
    seen[sid] = g;
    ids.push_back(sid);
    group_of.push_back(g);
  }
  if (ids.empty() && (!windows || !a.groups_file.empty())) return fail_with("no sample-group pairs in " + a.groups_file);
  std::vector<const char*> name_ptrs;
  for (auto& n : names) name_ptrs.push_back(n.c_str());
  std::vector<vs_region> batch;
  for (auto& r : read_regions(a.region)) batch.push_back(vs_region{std::get<0>(r), std::get<1>(r)});
  vs_result* res = nullptr;
  if (!windows) rc = vs_query_group_counts(idx, batch.data(), batch.size(), ids.data(), group_of.data(), ids.size(), (uint32_t)names.size(), name_ptrs.data(), &res);
  else if (ids.empty()) rc = vs_query_window_stats(idx, batch.data(), batch.size(), nullptr, nullptr, 0, 1, nullptr, a.windows_no_pairs ? 0 : 1, &res);
  else rc = vs_query_window_stats(idx, batch.data(), batch.size(), ids.data(), group_of.data(), ids.size(), (uint32_t)names.size(), name_ptrs.data(), a.windows_no_pairs ? 0 : 1, &res);
  if (rc != VS_OK) die(rc, windows ? "windows" : "groups");
  uint32_t G = 0, P = 0;
  const uint32_t* sizes = nullptr;
  const vs_window_stats* ws = nullptr;
  const vs_window_pair_stats* wp = nullptr;
  if (windows && a.windows_derived) {
    rc = vs_result_get_window_stats(res, nullptr, &G, &P, &sizes, nullptr, &ws, &wp);
    if (rc != VS_OK) die(rc, "result");
  }
  std::ofstream file;
  if (!a.outfile.empty()) file.open(a.outfile, std::ios::binary);
  std::ostream& out = a.outfile.empty() ? std::cout : file;
  for (size_t i = 0; i < batch.size(); ++i) {
    const char* text = nullptr;
    uint64_t len = 0;
    rc = vs_result_format_region(res, i, &text, &len);
    if (rc != VS_OK) die(rc, "result");
    out << "#region " << i << " " << batch[i].x << ":" << batch[i].y << "\n";
    if (!ws) { out.write(text, len); continue; }
    // --derived: the same lines, each with its columns appended (line 0: the group header, then G groups, the pair header, P pairs)
    const std::string body(text, len);
    std::vector<WindowDerived> d(G);
    for (uint32_t g = 0; g < G; ++g) d[g] = window_derived(ws[i * G + g], sizes[g]);
    std::vector<std::pair<uint32_t, uint32_t>> gh;
    for (uint32_t g = 0; g < G; ++g)
      for (uint32_t h = g + 1; h < G; ++h) gh.emplace_back(g, h);
    size_t at = 0;
    for (uint32_t ln = 0; at < body.size(); ++ln) {
      const size_t nl = body.find('\n', at);
      out.write(body.data() + at, nl - at);
      if (ln == 0) out << "\tPi\tThetaW\tTajimaD";
      else if (ln <= G) out << '\t' << g10(d[ln - 1].pi) << '\t' << g10(d[ln - 1].theta) << '\t' << g10(d[ln - 1].tajima);
      else if (ln == G + 1) out << "\tDxy\tFst";
      else {
        const uint32_t p = ln - G - 2, g = gh[p].first, h = gh[p].second;
        const double dxy = window_dxy(ws[i * G + g], ws[i * G + h], wp[i * P + p], sizes[g], sizes[h]);
        const double fst = dxy > 0 ? 1.0 - ((d[g].pi + d[h].pi) / 2.0) / dxy : std::nan("");
        out << '\t' << g10(dxy) << '\t' << g10(fst);
      }
      out << '\n';
      at = nl + 1;
    }
  }
  out.flush();
  vs_result_free(res);
  vs_index_close(idx);
  return EXIT_SUCCESS;
}

// `variantstore assoc`: every variant the regions report scored against the phenotypes of a file (vs_query_assoc_scan).  The -P file
// holds one `sample value [value ...]` line per sample, fields separated by tabs or spaces; its samples are the subset.  A first line
// `#sample name1 name2 ...` names the traits.  Output as `counts`: "#region <i> <x>:<y>", then the region's text.
int assoc_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore assoc -p <output-prefix> -r <region> -P <phenotype-file> [--chi2] [-o <outfile>] [--device <n>]\n\n"
               "        Every variant query type 6 reports in each region against up to 8 phenotypes: the sum of dosage x value over\n"
               "        the file's samples, or with --chi2 the score test of a regression of the value on the dosage.  The file holds\n"
               "        one `sample value [value ...]` line per sample; a first line `#sample name1 name2 ...` names the traits.\n";
  return EXIT_FAILURE;
}

// `variantstore assocmatrix`: the same file without the limit of 8 traits (up to 65,536), through vs_query_assoc_matrix.  Output as `assoc`.
int assocmatrix_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore assocmatrix -p <output-prefix> -r <region> -P <phenotype-file> [--chi2] [-o <outfile>] [--device <n>]\n\n"
               "        Every variant query type 6 reports in each region against a wide panel of phenotypes (up to 65536): the sum of\n"
               "        dosage x value over the file's samples from exact fixed-point integers, or with --chi2 the score test.  The file\n"
               "        is `assoc`'s: one `sample value [value ...]` line per sample; a first line `#sample name1 name2 ...` names the traits.\n";
  return EXIT_FAILURE;
}

// (max_traits: VS_TRAITS_MAX for `assoc`, VS_TRAIT_MATRIX_MAX for `assocmatrix`, which also picks the query)
int assoc_main(const Args& a, const size_t max_traits = VS_TRAITS_MAX) {
  vs_index* idx = nullptr;
  int rc = vs_index_open(a.prefix.c_str(), a.device, &idx);
  if (rc != VS_OK) die(rc, "load");
  auto fail_with = [&](const std::string& msg) { error(msg); vs_index_close(idx); return EXIT_FAILURE; };
  std::ifstream in(a.pheno_file);
  if (!in) return fail_with("cannot open phenotype file " + a.pheno_file);
  auto fields_of = [](const std::string& line) {
    std::vector<std::string> f;
    for (size_t p = line.find_first_not_of(" \t"); p != std::string::npos;) {
      const size_t e = line.find_first_of(" \t", p);
      f.push_back(line.substr(p, e == std::string::npos ? e : e - p));
      p = e == std::string::npos ? e : line.find_first_not_of(" \t", e);
    }
    return f;
  };
  std::vector<uint32_t> ids;
  std::vector<float> traits;
  std::vector<std::string> names;
  size_t n_traits = 0, lineno = 0;
  std::string line;
  while (std::getline(in, line)) {
    ++lineno;
    const std::string at = a.pheno_file + " line " + std::to_string(lineno);
    if (!line.empty() && line.back() == '\r') line.pop_back();
    const std::vector<std::string> f = fields_of(line);
    if (f.empty()) continue;
    if (f[0] == "#sample") {
      if (!ids.empty() || !names.empty() || f.size() < 2) return fail_with(at + ": a `#sample name ...` line comes first and once");
      if (f.size() - 1 > max_traits) return fail_with(at + ": more than " + std::to_string(max_traits) + " traits");
      names.assign(f.begin() + 1, f.end());
      n_traits = names.size();
      continue;
    }
    if (f.size() < 2) return fail_with(at + ": no value behind the sample");
    if (!n_traits) n_traits = f.size() - 1;
    if (f.size() - 1 != n_traits) return fail_with(at + ": " + std::to_string(f.size() - 1) + " values, " + std::to_string(n_traits) + " expected");
    if (n_traits > max_traits) return fail_with(at + ": more than " + std::to_string(max_traits) + " traits");
    uint32_t sid = 0;
    if (vs_index_sample_id(idx, f[0].c_str(), &sid) != VS_OK || sid == 0) return fail_with(at + ": Sample not found: " + f[0]);
    ids.push_back(sid);
    for (size_t k = 1; k < f.size(); ++k) {
      char* end = nullptr;
      const float v = strtof(f[k].c_str(), &end);
      if (end == f[k].c_str() || *end) return fail_with(at + ": not a number: " + f[k]);
      traits.push_back(v);
    }
  }
  if (ids.empty()) return fail_with("no samples in " + a.pheno_file);
  std::vector<const char*> name_ptrs;
  for (auto& n : names) name_ptrs.push_back(n.c_str());
  std::vector<vs_region> batch;
  for (auto& r : read_regions(a.region)) batch.push_back(vs_region{std::get<0>(r), std::get<1>(r)});
  vs_result* res = nullptr;
  const bool wide = max_traits != VS_TRAITS_MAX;
  rc = (wide ? vs_query_assoc_matrix : vs_query_assoc_scan)(idx, batch.data(), batch.size(), ids.data(), ids.size(), traits.data(), (uint32_t)n_traits,
                                                            a.assoc_chi2 ? VS_ASSOC_CHI2 : VS_ASSOC_DOT, names.empty() ? nullptr : name_ptrs.data(), &res);
  if (rc != VS_OK) die(rc, wide ? "assocmatrix" : "assoc");
  std::ofstream file;
  if (!a.outfile.empty()) file.open(a.outfile, std::ios::binary);
  std::ostream& out = a.outfile.empty() ? std::cout : file;
  for (size_t i = 0; i < batch.size(); ++i) {
    const char* text = nullptr;
    uint64_t len = 0;
    rc = vs_result_format_region(res, i, &text, &len);
    if (rc != VS_OK) die(rc, "result");
    out << "#region " << i << " " << batch[i].x << ":" << batch[i].y << "\n";
    out.write(text, len);
  }
  out.flush();
  vs_result_free(res);
  vs_index_close(idx);
  return EXIT_SUCCESS;
}

// `variantstore score`: per-sample scores of the variants the regions report under the weights of a file (vs_query_sample_scores).  The
// -W file holds one `pos ref alt weight [weight ...]` line per variant, fields separated by tabs or spaces, pos / ref / alt as query type
// 6 prints them; a first line `#pos ref alt name1 name2 ...` names the scores.  A count batch over the regions gives the reported rows,
// every one takes the weights of its key (none: 0), then the score batch runs over the same regions.  Output: `Sample\t<names>`, then a
// line per sample.
int score_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore score -p <output-prefix> -r <region> -W <weights-file> [-S <samples-file>] [-o <outfile>] [--device <n>]\n\n"
               "        For every sample (of the file: one name per line; default: the whole cohort) up to 8 weighted sums of its dosages\n"
               "        over the variants query type 6 reports in the regions.  The weights file holds one `pos ref alt weight [weight ...]`\n"
               "        line per variant; a first line `#pos ref alt name1 name2 ...` names the scores.\n";
  return EXIT_FAILURE;
}

// `variantstore scorematrix`: the same over any number of weight columns up to VS_SCORE_MATRIX_MAX, as a product on the matrix cores
// (vs_query_score_matrix); the weights file, its header line, the warning about unmatched variants and the output are `score`'s.
int scorematrix_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore scorematrix -p <output-prefix> -r <region> -W <weights-file> [-S <samples-file>] [-o <outfile>] [--device <n>]\n\n"
               "        For every sample (of the file: one name per line; default: the whole cohort) any number of weighted sums of its\n"
               "        dosages over the variants query type 6 reports in the regions, as one matrix product.  The weights file holds one\n"
               "        `pos ref alt weight [weight ...]` line per variant; a first line `#pos ref alt name1 name2 ...` names the scores.\n";
  return EXIT_FAILURE;
}

int score_main(const Args& a, bool matrix = false) {
  const size_t max_scores = matrix ? VS_SCORE_MATRIX_MAX : VS_SCORES_MAX;
  const char* const what = matrix ? "scorematrix" : "score";
  vs_index* idx = nullptr;
  int rc = vs_index_open(a.prefix.c_str(), a.device, &idx);
  if (rc != VS_OK) die(rc, "load");
  auto fail_with = [&](const std::string& msg) { error(msg); vs_index_close(idx); return EXIT_FAILURE; };
  std::ifstream in(a.weights_file);
  if (!in) return fail_with("cannot open weights file " + a.weights_file);
  auto fields_of = [](const std::string& line) {
    std::vector<std::string> f;
    for (size_t p = line.find_first_not_of(" \t"); p != std::string::npos;) {
      const size_t e = line.find_first_of(" \t", p);
      f.push_back(line.substr(p, e == std::string::npos ? e : e - p));
      p = e == std::string::npos ? e : line.find_first_not_of(" \t", e);
    }
    return f;
  };
  std::unordered_map<std::string, size_t> key_row;   // "pos\tref\talt" -> its row of `table`
  std::vector<float> table;
  std::vector<std::string> names;
  size_t K = 0, lineno = 0;
  std::string line;
  while (std::getline(in, line)) {
    ++lineno;
    const std::string at = a.weights_file + " line " + std::to_string(lineno);
    if (!line.empty() && line.back() == '\r') line.pop_back();
    const std::vector<std::string> f = fields_of(line);
    if (f.empty()) continue;
    if (f[0] == "#pos") {
      if (!key_row.empty() || !names.empty() || f.size() < 4) return fail_with(at + ": a `#pos ref alt name ...` line comes first and once");
      if (f.size() - 3 > max_scores) return fail_with(at + ": more than " + std::to_string(max_scores) + " values");
      names.assign(f.begin() + 3, f.end());
      K = names.size();
      continue;
    }
    if (f.size() < 4) return fail_with(at + ": malformed line, `pos ref alt weight [weight ...]` expected");
    char* end = nullptr;
    const unsigned long long pos = strtoull(f[0].c_str(), &end, 10);
    if (end == f[0].c_str() || *end) return fail_with(at + ": malformed line, not a position: " + f[0]);
    if (!K) K = f.size() - 3;
    if (f.size() - 3 != K) return fail_with(at + ": " + std::to_string(f.size() - 3) + " values, " + std::to_string(K) + " expected");
    if (K > max_scores) return fail_with(at + ": more than " + std::to_string(max_scores) + " values");
    auto allele = [](const std::string& x) { return x == "-" || x == "." ? std::string() : x; };   // (an empty allele, as the texts print a deletion's)
    const std::string key = std::to_string(pos) + "\t" + allele(f[1]) + "\t" + allele(f[2]);
    if (!key_row.emplace(key, table.size() / K).second) return fail_with(at + ": the variant is listed twice: " + f[0] + " " + f[1] + " " + f[2]);
    for (size_t k = 3; k < f.size(); ++k) {
      end = nullptr;
      const float v = strtof(f[k].c_str(), &end);
      if (end == f[k].c_str() || *end) return fail_with(at + ": not a number: " + f[k]);
      table.push_back(v);
    }
  }
  if (key_row.empty()) return fail_with("no variants in " + a.weights_file);
  std::vector<uint32_t> ids;
  if (!a.samples_file.empty()) {
    std::ifstream sin(a.samples_file);
    if (!sin) return fail_with("cannot open sample file " + a.samples_file);
    while (std::getline(sin, line)) {
      if (!line.empty() && line.back() == '\r') line.pop_back();
      if (line.empty()) continue;
      uint32_t sid = 0;
      if (vs_index_sample_id(idx, line.c_str(), &sid) != VS_OK || sid == 0) return fail_with("Sample not found: " + line);
      ids.push_back(sid);
    }
    if (ids.empty()) return fail_with("no sample names in " + a.samples_file);
  }
  vs_index_info info{};
  rc = vs_index_get_info(idx, &info);
  if (rc != VS_OK) die(rc, "info");
  std::vector<vs_region> batch;
  for (auto& r : read_regions(a.region)) batch.push_back(vs_region{std::get<0>(r), std::get<1>(r)});
  // the reported rows, region after region: a count batch's text
  vs_result* cres = nullptr;
  rc = vs_query_allele_counts(idx, batch.data(), batch.size(), nullptr, 0, &cres);
  if (rc != VS_OK) die(rc, what);
  std::vector<float> weights;
  std::vector<uint8_t> matched(key_row.size(), 0);
  for (size_t i = 0; i < batch.size(); ++i) {
    const char* text = nullptr;
    uint64_t len = 0;
    rc = vs_result_format_region(cres, i, &text, &len);
    if (rc != VS_OK) die(rc, "result");
    const std::string t(text, len);
    for (size_t p = t.find('\n'); p != std::string::npos && p + 1 < t.size();) {   // (the first line is the header)
      const size_t b = p + 1, e = t.find('\n', b);
      size_t tab = b;
      for (int k = 0; k < 3 && tab != std::string::npos; ++k) tab = t.find('\t', tab + (k ? 1 : 0));
      const auto it = key_row.find(t.substr(b, (tab == std::string::npos || tab > e ? e : tab) - b));
      if (it == key_row.end()) weights.insert(weights.end(), K, 0.0f);
      else {
        weights.insert(weights.end(), table.begin() + it->second * K, table.begin() + (it->second + 1) * K);
        matched[it->second] = 1;
      }
      p = e;
    }
  }
  vs_result_free(cres);
  size_t unmatched = 0;
  for (uint8_t m : matched) unmatched += !m;
  if (unmatched) std::cerr << "warning: " << unmatched << " of " << matched.size() << " variants of " << a.weights_file << " matched no reported row\n";
  std::vector<const char*> name_ptrs;
  for (auto& n : names) name_ptrs.push_back(n.c_str());
  vs_result* res = nullptr;
  rc = (matrix ? vs_query_score_matrix : vs_query_sample_scores)(idx, batch.data(), batch.size(), ids.empty() ? nullptr : ids.data(),
                                                                 ids.empty() ? info.num_samples - 1 : ids.size(), weights.data(), weights.size() / K, (uint32_t)K,
                                                                 names.empty() ? nullptr : name_ptrs.data(), &res);
  if (rc != VS_OK) die(rc, what);
  uint64_t n_cols = 0;
  uint32_t n_scores = 0;
  const uint32_t* cols = nullptr;
  const double* sc = nullptr;
  rc = matrix ? vs_result_get_score_matrix(res, &n_cols, &n_scores, &cols, nullptr, nullptr, nullptr, &sc)
              : vs_result_get_sample_scores(res, &n_cols, &n_scores, &cols, nullptr, nullptr, &sc);
  if (rc != VS_OK) die(rc, "result");
  std::ofstream file;
  if (!a.outfile.empty()) file.open(a.outfile, std::ios::binary);
  std::ostream& out = a.outfile.empty() ? std::cout : file;
  out << "Sample";
  for (uint32_t k = 0; k < n_scores; ++k) out << '\t' << (names.empty() ? std::to_string(k) : names[k]);
  out << '\n';
  char num[48];
  for (uint64_t c = 0; c < n_cols; ++c) {
    const char* nm = vs_index_sample_name(idx, cols[c]);
    out << (nm ? nm : "?");
    for (uint32_t k = 0; k < n_scores; ++k) { snprintf(num, sizeof num, "\t%.17g", sc[c * n_scores + k]); out << num; }
    out << '\n';
  }
  out.flush();
  vs_result_free(res);
  vs_index_close(idx);
  return EXIT_SUCCESS;
}

// The ids of the samples named in a file, one name a line (`gram`, `ibs`): false, with the error reported, when the file cannot be
// read, names nobody or names a sample the index does not have.
bool read_sample_ids(vs_index* idx, const std::string& path, std::vector<uint32_t>& ids) {
  std::ifstream in(path);
  if (!in) { error("cannot open sample file " + path); return false; }
  std::string line;
  while (std::getline(in, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty()) continue;
    uint32_t sid = 0;
    if (vs_index_sample_id(idx, line.c_str(), &sid) != VS_OK || sid == 0) { error("Sample not found: " + line); return false; }
    ids.push_back(sid);
  }
  if (ids.empty()) { error("no sample names in " + path); return false; }
  return true;
}

// `variantstore gram`: the samples x samples Gram matrix of the regions' variant table (vs_query_sample_gram), or with --grm the GRM
// formed from it.  Output: a header line of the sample names, then one line per sample -- its name and its row of the matrix.
int gram_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore gram -p <output-prefix> -r <region> [-S <sample-name-file>] [--grm] [-o <outfile>] [--device <n>]\n\n"
               "        For every pair of samples (of the whole cohort or of those named in the file) the sum, over the variants query\n"
               "        type 6 reports in the regions (each once), of the product of their alternate-allele dosages; with --grm the\n"
               "        genomic relationship matrix (VanRaden's first form) computed from those sums.\n";
  return EXIT_FAILURE;
}

int gram_main(const Args& a) {
  vs_index* idx = nullptr;
  int rc = vs_index_open(a.prefix.c_str(), a.device, &idx);
  if (rc != VS_OK) die(rc, "load");
  std::vector<uint32_t> ids;
  if (!a.samples_file.empty() && !read_sample_ids(idx, a.samples_file, ids)) { vs_index_close(idx); return EXIT_FAILURE; }
  std::vector<vs_region> batch;
  for (auto& r : read_regions(a.region)) batch.push_back(vs_region{std::get<0>(r), std::get<1>(r)});
  vs_result* res = nullptr;
  rc = vs_query_sample_gram(idx, batch.data(), batch.size(), ids.empty() ? nullptr : ids.data(), ids.size(), a.gram_grm ? VS_GRAM_GRM : VS_GRAM_DOT, &res);
  if (rc != VS_OK) die(rc, "gram");
  uint64_t n_cols = 0;
  const uint32_t* cols = nullptr;
  const int64_t* gram = nullptr;
  const double* grm = nullptr;
  rc = vs_result_get_sample_gram(res, nullptr, &n_cols, nullptr, &cols, nullptr, &gram, &grm, nullptr, nullptr, nullptr);
  if (rc != VS_OK) die(rc, "gram");
  std::ofstream file;
  if (!a.outfile.empty()) file.open(a.outfile, std::ios::binary);
  std::ostream& out = a.outfile.empty() ? std::cout : file;
  out << "Sample";
  for (uint64_t c = 0; c < n_cols; ++c) {
    const char* nm = vs_index_sample_name(idx, cols[c]);
    out << '\t' << (nm ? nm : "?");
  }
  out << '\n';
  char num[48];
  for (uint64_t i = 0; i < n_cols; ++i) {
    const char* nm = vs_index_sample_name(idx, cols[i]);
    out << (nm ? nm : "?");
    for (uint64_t j = 0; j < n_cols; ++j) {
      if (a.gram_grm) snprintf(num, sizeof num, "\t%.17g", grm[i * n_cols + j]);
      else snprintf(num, sizeof num, "\t%lld", (long long)gram[i * n_cols + j]);
      out << num;
    }
    out << '\n';
  }
  out.flush();
  vs_result_free(res);
  vs_index_close(idx);
  return EXIT_SUCCESS;
}

// `variantstore ibs`: the pairwise genotype-state counts of the regions' variant table (vs_query_sample_ibs) as a pair table, what
// users of KING's .kin0 expect: a header line, then one line per pair i < j in column order.
int ibs_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore ibs -p <output-prefix> -r <region> [-S <sample-name-file>] [--king] [--min-kinship <x>] [-o <outfile>] [--device <n>]\n\n"
               "        For every pair of samples (of the whole cohort or of those named in the file), over the variants query type 6\n"
               "        reports in the regions (each once): N, the variants counted; HetHet, both heterozygous; IBS0, opposite\n"
               "        homozygotes; IBS1; IBS2, equal genotypes.  With --king the KING-robust kinship as a last column; with\n"
               "        --min-kinship <x> (implies --king) only the pairs whose kinship is at least x.\n";
  return EXIT_FAILURE;
}

int ibs_main(const Args& a) {
  vs_index* idx = nullptr;
  int rc = vs_index_open(a.prefix.c_str(), a.device, &idx);
  if (rc != VS_OK) die(rc, "load");
  std::vector<uint32_t> ids;
  if (!a.samples_file.empty() && !read_sample_ids(idx, a.samples_file, ids)) { vs_index_close(idx); return EXIT_FAILURE; }
  std::vector<vs_region> batch;
  for (auto& r : read_regions(a.region)) batch.push_back(vs_region{std::get<0>(r), std::get<1>(r)});
  const bool king = a.ibs_king || a.ibs_have_min;
  vs_result* res = nullptr;
  rc = vs_query_sample_ibs(idx, batch.data(), batch.size(), ids.empty() ? nullptr : ids.data(), ids.size(), king ? VS_IBS_KING : VS_IBS_COUNTS, &res);
  if (rc != VS_OK) die(rc, "ibs");
  uint64_t n = 0;
  const uint32_t* cols = nullptr;
  const int64_t *hh = nullptr, *ibs0 = nullptr, *ibs2 = nullptr;
  const double* kin = nullptr;
  int64_t n_used = 0;
  rc = vs_result_get_sample_ibs(res, nullptr, &n, nullptr, &cols, nullptr, &hh, nullptr, nullptr, &ibs0, &ibs2, &kin, &n_used);
  if (rc != VS_OK) die(rc, "ibs");
  std::ofstream file;
  if (!a.outfile.empty()) file.open(a.outfile, std::ios::binary);
  std::ostream& out = a.outfile.empty() ? std::cout : file;
  out << "ID1\tID2\tN\tHetHet\tIBS0\tIBS1\tIBS2" << (king ? "\tKinship" : "") << '\n';
  char num[160];
  for (uint64_t i = 0; i < n; ++i) {
    const char* ni = vs_index_sample_name(idx, cols[i]);
    for (uint64_t j = i + 1; j < n; ++j) {
      const uint64_t c = i * n + j;
      if (a.ibs_have_min && !(kin[c] >= a.ibs_min_kinship)) continue;
      const char* nj = vs_index_sample_name(idx, cols[j]);
      snprintf(num, sizeof num, "\t%lld\t%lld\t%lld\t%lld\t%lld", (long long)n_used, (long long)hh[c], (long long)ibs0[c],
               (long long)(n_used - ibs0[c] - ibs2[c]), (long long)ibs2[c]);
      out << (ni ? ni : "?") << '\t' << (nj ? nj : "?") << num;
      if (king) { snprintf(num, sizeof num, "\t%.17g", kin[c]); out << num; }
      out << '\n';
    }
  }
  out.flush();
  vs_result_free(res);
  vs_index_close(idx);
  return EXIT_SUCCESS;
}

// `variantstore trios`: Mendelian errors and transmission counts of the regions' variant table (vs_query_trio_scan).  Output as
// `counts`: "#region <i> <x>:<y>", then the region's text ("Pos Ref Alt AC Errors DeNovo T U", a line per reported row); with
// --per-trio instead one table over the whole batch, "Child Father Mother N Errors DeNovo T U", a line per trio in the file's order.
int trios_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore trios -p <output-prefix> -r <region> -T <trio-file> [--per-trio] [-o <outfile>] [--device <n>]\n\n"
               "        For every variant query type 6 reports in the regions, over the trios of the file: Errors, the trios whose\n"
               "        three genotypes break Mendel's laws; DeNovo, those of them whose parents both lack the allele; T and U, the\n"
               "        alleles heterozygous parents transmitted and did not transmit (the counts of the transmission disequilibrium\n"
               "        test).  With --per-trio the same four per trio, summed over the variants (each once; N of them).  The file\n"
               "        has a line per trio: three names, child father mother, or a PED/FAM line of six or more fields (FID IID PAT\n"
               "        MAT ...), where lines whose PAT or MAT is 0 are skipped.  Meant for diploid calls.\n";
  return EXIT_FAILURE;
}

// The trios of a file as sample ids, three per trio: false, with the error reported, when the file cannot be read, a line has
// neither three nor six or more fields, a name is not a sample of the index, or no trio is left.  `founders`: the PED lines skipped
// (their number goes to stderr).
bool read_trios(vs_index* idx, const std::string& path, std::vector<uint32_t>& ids, size_t& founders) {
  std::ifstream in(path);
  if (!in) { error("cannot open trio file " + path); return false; }
  std::string line;
  size_t lineno = 0;
  while (std::getline(in, line)) {
    ++lineno;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    std::istringstream ls(line);
    std::vector<std::string> f;
    for (std::string w; ls >> w;) f.push_back(w);
    if (f.empty() || f[0][0] == '#') continue;
    if (f.size() != 3 && f.size() < 6) {
      error("trio file line " + std::to_string(lineno) + ": expected \"child father mother\" or a PED line \"FID IID PAT MAT ...\" of six or more fields");
      return false;
    }
    const bool ped = f.size() >= 6;
    if (ped && (f[2] == "0" || f[3] == "0")) { ++founders; continue; }
    for (const std::string& name : {f[ped ? 1 : 0], f[ped ? 2 : 1], f[ped ? 3 : 2]}) {
      uint32_t sid = 0;
      if (vs_index_sample_id(idx, name.c_str(), &sid) != VS_OK || sid == 0) { error("Sample not found: " + name); return false; }
      ids.push_back(sid);
    }
  }
  if (founders) std::cerr << "skipped " << founders << " line(s) of " << path << " without both parents\n";
  if (ids.empty()) { error("no trios in " + path); return false; }
  return true;
}

int trios_main(const Args& a) {
  vs_index* idx = nullptr;
  int rc = vs_index_open(a.prefix.c_str(), a.device, &idx);
  if (rc != VS_OK) die(rc, "load");
  std::vector<uint32_t> ids;
  size_t founders = 0;
  if (!read_trios(idx, a.trios_file, ids, founders)) { vs_index_close(idx); return EXIT_FAILURE; }
  std::vector<vs_region> batch;
  for (auto& r : read_regions(a.region)) batch.push_back(vs_region{std::get<0>(r), std::get<1>(r)});
  vs_result* res = nullptr;
  rc = vs_query_trio_scan(idx, batch.data(), batch.size(), ids.data(), ids.size() / 3, &res);
  if (rc != VS_OK) die(rc, "trios");
  std::ofstream file;
  if (!a.outfile.empty()) file.open(a.outfile, std::ios::binary);
  std::ostream& out = a.outfile.empty() ? std::cout : file;
  if (a.trios_per_trio) {
    uint64_t n_trios = 0, n_used = 0;
    const vs_trio_counts *rows = nullptr, *trios = nullptr;
    rc = vs_result_get_trio_scan(res, nullptr, nullptr, &n_trios, &n_used, nullptr, nullptr, nullptr, &rows, &trios);
    if (rc != VS_OK) die(rc, "trios");
    out << "Child\tFather\tMother\tN\tErrors\tDeNovo\tT\tU\n";
    for (uint64_t t = 0; t < n_trios; ++t) {
      for (int k = 0; k < 3; ++k) {
        const char* nm = vs_index_sample_name(idx, ids[3 * t + k]);
        out << (nm ? nm : "?") << '\t';
      }
      out << n_used << '\t' << trios[t].errors << '\t' << trios[t].denovo << '\t' << trios[t].transmitted << '\t' << trios[t].untransmitted << '\n';
    }
  } else {
    for (size_t i = 0; i < batch.size(); ++i) {
      const char* text = nullptr;
      uint64_t len = 0;
      rc = vs_result_format_region(res, i, &text, &len);
      if (rc != VS_OK) die(rc, "result");
      out << "#region " << i << " " << batch[i].x << ":" << batch[i].y << "\n";
      out.write(text, len);
    }
  }
  out.flush();
  vs_result_free(res);
  vs_index_close(idx);
  return EXIT_SUCCESS;
}

// `variantstore roh`: runs of homozygosity per sample and region (vs_query_roh).  One table over the batch, tab-separated: by default
// "Sample Region Pos1 Pos2 KB NSites NHet", a line per segment, ordered by region, then sample column, then occurrence; with
// --summary "Sample Region NSeg KB KBAvg LongestKB NHet", a line per region and sample.  Region is <x>:<y>; KB figures are printed
// from the integer base counts with three fixed decimals (KBAvg: floor(total_bp / NSeg) bases; NA without segments).
int roh_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore roh -p <output-prefix> -r <region> [-S <sample-file>] [--min-sites <n>] [--min-bp <n>] [--max-gap <n>]\n"
               "                         [--max-het <n>] [--min-ac <n>] [--max-ac <n>] [--summary] [-o <outfile>] [--device <n>]\n\n"
               "        Runs of homozygosity of every sample (or of the samples of the file) in every region: stretches of consecutive\n"
               "        polymorphic sites (alternate-allele count within --min-ac .. --max-ac) at which the sample is homozygous.  A run\n"
               "        absorbs up to --max-het (0 .. 255, default 0) heterozygous sites, is cut where two consecutive sites lie more\n"
               "        than --max-gap bases apart (default 0: never) and is reported when it has at least --min-sites sites (default\n"
               "        50, at least 1) and spans at least --min-bp bases (default 0).  --summary: per sample and region the number of\n"
               "        segments, their total and mean length, the longest one and the sample's heterozygous sites.\n";
  return EXIT_FAILURE;
}

// a decimal uint32 and nothing else
bool parse_u32(const std::string& v, uint32_t& out) {
  if (v.empty() || v.size() > 10) return false;
  uint64_t x = 0;
  for (char ch : v) {
    if (ch < '0' || ch > '9') return false;
    x = x * 10 + (uint64_t)(ch - '0');
  }
  if (x > UINT32_MAX) return false;
  out = (uint32_t)x;
  return true;
}

std::string roh_kb(uint64_t bp) {
  char buf[40];
  snprintf(buf, sizeof buf, "%llu.%03u", (unsigned long long)(bp / 1000), (unsigned)(bp % 1000));
  return buf;
}

int roh_main(const Args& a) {
  vs_index* idx = nullptr;
  int rc = vs_index_open(a.prefix.c_str(), a.device, &idx);
  if (rc != VS_OK) die(rc, "load");
  std::vector<uint32_t> ids;
  if (!a.samples_file.empty() && !read_sample_ids(idx, a.samples_file, ids)) { vs_index_close(idx); return EXIT_FAILURE; }
  std::vector<vs_region> batch;
  for (auto& r : read_regions(a.region)) batch.push_back(vs_region{std::get<0>(r), std::get<1>(r)});
  vs_roh_params prm{};
  prm.min_sites = a.roh_min_sites; prm.min_bp = a.roh_min_bp; prm.max_gap = a.roh_max_gap; prm.max_het = a.roh_max_het;
  prm.min_ac = a.min_ac; prm.max_ac = a.max_ac; prm.segments = a.roh_summary ? 0u : 1u;
  vs_result* res = nullptr;
  rc = vs_query_roh(idx, batch.data(), batch.size(), ids.empty() ? nullptr : ids.data(), ids.size(), &prm, &res);
  if (rc != VS_OK) die(rc, "roh");
  uint64_t n_cols = 0, n_segments = 0;
  const uint32_t* cols = nullptr;
  const vs_roh_summary* sum = nullptr;
  const vs_roh_segment* seg = nullptr;
  rc = vs_result_get_roh(res, nullptr, &n_cols, nullptr, &n_segments, nullptr, &cols, nullptr, &sum, nullptr, nullptr, &seg);
  if (rc != VS_OK) die(rc, "roh");
  std::ofstream file;
  if (!a.outfile.empty()) file.open(a.outfile, std::ios::binary);
  std::ostream& out = a.outfile.empty() ? std::cout : file;
  auto name = [&](uint32_t c) { const char* nm = vs_index_sample_name(idx, cols[c]); return nm ? nm : "?"; };
  if (a.roh_summary) {
    out << "Sample\tRegion\tNSeg\tKB\tKBAvg\tLongestKB\tNHet\n";
    for (size_t q = 0; q < batch.size(); ++q)
      for (uint64_t c = 0; c < n_cols; ++c) {
        const vs_roh_summary& s = sum[q * n_cols + c];
        out << name((uint32_t)c) << '\t' << batch[q].x << ':' << batch[q].y << '\t' << s.n_segments << '\t' << roh_kb(s.total_bp) << '\t'
            << (s.n_segments ? roh_kb(s.total_bp / s.n_segments) : std::string("NA")) << '\t' << roh_kb(s.longest_bp) << '\t' << s.n_het << '\n';
      }
  } else {
    out << "Sample\tRegion\tPos1\tPos2\tKB\tNSites\tNHet\n";
    for (uint64_t k = 0; k < n_segments; ++k) {
      const vs_roh_segment& g = seg[k];
      const uint64_t bp = (uint64_t)(g.pos_last > g.pos_first ? g.pos_last - g.pos_first : 0u) + 1u;
      out << name(g.column) << '\t' << batch[g.region].x << ':' << batch[g.region].y << '\t' << g.pos_first << '\t' << g.pos_last << '\t' << roh_kb(bp) << '\t'
          << g.n_sites << '\t' << g.n_het << '\n';
    }
  }
  out.flush();
  vs_result_free(res);
  vs_index_close(idx);
  return EXIT_SUCCESS;
}

// `variantstore ldmatrix`: the full LD block of every region (vs_query_ld_matrix) over the same samples.  Output as `counts`:
// "#region <i> <x>:<y>", then the region's text (a header of the reported rows' <Pos>:<Ref>:<Alt>, then one line per row with its
// r^2 -- or with --dot its dot product -- against every one of them).
int ldmatrix_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore ldmatrix -p <output-prefix> -r <region> [-S <sample-name-file>] [--dot] [-o <outfile>] [--device <n>]\n\n"
               "        For every region the square matrix of its variants (as query type 6 reports them) against each other: the\n"
               "        squared correlation of the samples' alternate-allele dosages (of the whole cohort or of the samples named in\n"
               "        the file), or with --dot the sum of the dosage products.\n";
  return EXIT_FAILURE;
}

// `variantstore prune`: greedy LD pruning of every region (vs_query_ld_prune) over the same samples.  Output as `counts`:
// "#region <i> <x>:<y>", then the region's text ("Pos Ref Alt AC State", a line per reported row: keep, pruned or skip).
int prune_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore prune -p <output-prefix> -r <region> [-S <sample-name-file>] [-w <window>] [--r2 <bound>] [--bp <n>]\n"
               "                           [--min-ac <n>] [--max-ac <n>] [-o <outfile>] [--device <n>]\n\n"
               "        For every region the forward greedy LD pruning of its variants (as query type 6 reports them), in order: a\n"
               "        variant is kept unless a kept variant among the <window> rows before it (1 .. 256, 64 by default; at most --bp\n"
               "        positions away) has a squared dosage correlation with it above --r2 (0 .. 1, 0.2 by default), over the whole\n"
               "        cohort or the samples named in the file.  Variants that are monomorphic there or whose alternate-allele\n"
               "        count lies outside [--min-ac, --max-ac] are skipped.\n";
  return EXIT_FAILURE;
}

// `variantstore clump`: p-value clumping of every region (vs_query_ld_clump) over the same samples.  Output as `prune`: "#region
// <i> <x>:<y>", then the region's text ("Pos Ref Alt AC P State Index", a line per reported row: index, clumped, unclumped or skip).
int clump_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore clump -p <output-prefix> -r <region> -A <p-value-file> [-S <sample-name-file>] [-w <window>] [--r2 <bound>]\n"
               "                           [--bp <n>] [--p1 <bound>] [--p2 <bound>] [-o <outfile>] [--device <n>]\n\n"
               "        For every region the clumps of its variants (as query type 6 reports them), as `plink --clump` forms them: the\n"
               "        variants are taken in order of their p-values (lines of \"pos ref alt p\" in the file, an empty allele written as\n"
               "        - or .; variants without a line have no p-value and are skipped); the best one with p <=\n"
               "        --p1 (0.0001 by default) becomes an index variant, every variant with p <= --p2 (0.01 by default) among the\n"
               "        <window> rows on either side of it (1 .. 256, 256 by default; at most --bp positions away, 250000 by default, 0:\n"
               "        no limit) whose squared dosage correlation with it is above --r2 (0 .. 1, 0.5 by default) joins its clump; the\n"
               "        next best unclaimed variant starts the next clump.  Over the whole cohort or the samples named in the file.\n";
  return EXIT_FAILURE;
}

// The p-value of every table row of the batch, in table order, from the lines of "pos ref alt p" (NaN: no line names the row); the
// rows through a count batch over the same regions.  Lines that matched no row are counted for the warning.
int clump_pvalues(vs_index* idx, const std::vector<vs_region>& batch, const std::string& path, std::vector<double>& pvalues, size_t& unmatched) {
  std::ifstream in(path);
  if (!in) { error("cannot open p-value file " + path); return EXIT_FAILURE; }
  std::map<std::string, std::pair<double, bool>> table;   // "pos\tref\talt" -> (p, matched)
  std::string line;
  size_t lineno = 0;
  while (std::getline(in, line)) {
    ++lineno;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty() || line[0] == '#') continue;
    std::istringstream ls(line);
    std::string pos, ref, alt, pv;
    if (!(ls >> pos >> ref >> alt >> pv)) { error("p-value file line " + std::to_string(lineno) + ": expected \"pos ref alt p\""); return EXIT_FAILURE; }
    char* end = nullptr;
    const double p = strtod(pv.c_str(), &end);
    if (*end != '\0' || !(std::isnan(p) || (p >= 0.0 && p <= 1.0))) { error("p-value file line " + std::to_string(lineno) + ": '" + pv + "' is no p-value between 0 and 1"); return EXIT_FAILURE; }
    const auto allele = [](const std::string& x) { return x == "-" || x == "." ? std::string() : x; };   // (an empty allele, as for `score`)
    table[pos + "\t" + allele(ref) + "\t" + allele(alt)] = {p, false};
  }
  vs_result* res = nullptr;
  int rc = vs_query_allele_counts(idx, batch.data(), batch.size(), nullptr, 0, &res);
  if (rc != VS_OK) die(rc, "clump");
  vs_result_raw raw;
  rc = vs_result_get_raw(res, 0, &raw);
  if (rc != VS_OK) die(rc, "clump");
  pvalues.assign(raw.n_rows, std::nan(""));
  for (uint64_t i = 0; i < raw.n_rows; ++i) {
    const vs_variant_row& v = raw.rows[i];
    if (VS_ROW_DROPPED(v)) continue;
    const auto it = table.find(std::to_string(v.pos) + "\t" + std::string(raw.seq_pool + v.ref_off, v.ref_len) + "\t" + std::string(raw.seq_pool + v.alt_off, v.alt_len));
    if (it == table.end()) continue;
    pvalues[i] = it->second.first;
    it->second.second = true;
  }
  vs_result_free(res);
  unmatched = 0;
  for (const auto& kv : table) unmatched += !kv.second.second;
  return EXIT_SUCCESS;
}

// `variantstore ldscore`: the LD score of every variant of every region (vs_query_ld_scores) over the same samples.  Output as
// `prune`: "#region <i> <x>:<y>", then the region's text ("Pos Ref Alt AC Pairs L2 State", a line per reported row: scored or skip).
int ldscore_usage() {
  std::cout << "SYNOPSIS\n"
               "        variantstore ldscore -p <output-prefix> -r <region> [-S <sample-name-file>] [-w <window>] [--bp <n>]\n"
               "                             [--min-ac <n>] [--max-ac <n>] [-o <outfile>] [--device <n>]\n\n"
               "        For every region the LD score of its variants (as query type 6 reports them): the sum of the squared dosage\n"
               "        correlation of a variant with every variant of the region at most <window> rows (0, the default: no limit)\n"
               "        and at most --bp positions (1000000 by default; 0: no limit) away, itself included, over the whole cohort or\n"
               "        the samples named in the file.  Pairs: the variants summed.  Variants that are monomorphic there or whose\n"
               "        alternate-allele count lies outside [--min-ac, --max-ac] are skipped and add to no sum.\n";
  return EXIT_FAILURE;
}

int counts_main(const Args& a, bool burden = false, bool genotypes = false, bool ld = false, bool ldmatrix = false, bool prune = false, bool clump = false,
                bool ldscore = false) {
  vs_index* idx = nullptr;
  int rc = vs_index_open(a.prefix.c_str(), a.device, &idx);
  if (rc != VS_OK) die(rc, "load");
  std::vector<uint32_t> ids;
  if (!a.samples_file.empty()) {
    std::ifstream in(a.samples_file);
    if (!in) { error("cannot open sample file " + a.samples_file); vs_index_close(idx); return EXIT_FAILURE; }
    std::string line;
    while (std::getline(in, line)) {
      if (!line.empty() && line.back() == '\r') line.pop_back();
      if (line.empty()) continue;
      uint32_t sid = 0;
      if (vs_index_sample_id(idx, line.c_str(), &sid) != VS_OK || sid == 0) {
        error("Sample not found: " + line);
        vs_index_close(idx);
        return EXIT_FAILURE;
      }
      ids.push_back(sid);
    }
    if (ids.empty()) { error("no sample names in " + a.samples_file); vs_index_close(idx); return EXIT_FAILURE; }
  }
  std::vector<vs_region> batch;
  for (auto& r : read_regions(a.region)) batch.push_back(vs_region{std::get<0>(r), std::get<1>(r)});
  vs_result* res = nullptr;
  if (clump) {
    std::vector<double> pvalues;
    size_t unmatched = 0;
    if (clump_pvalues(idx, batch, a.pvalues_file, pvalues, unmatched) != EXIT_SUCCESS) { vs_index_close(idx); return EXIT_FAILURE; }
    if (unmatched) std::cerr << "warning: " << unmatched << " line(s) of " << a.pvalues_file << " name no variant of the regions\n";
    const double none = 0.0;   // (an empty table: the C ABI takes no NULL)
    rc = vs_query_ld_clump(idx, batch.data(), batch.size(), ids.empty() ? nullptr : ids.data(), ids.size(), pvalues.empty() ? &none : pvalues.data(), pvalues.size(),
                           a.ld_window, a.prune_max_bp, a.prune_threshold, a.clump_p1, a.clump_p2, &res);
  }
  else if (ldscore) rc = vs_query_ld_scores(idx, batch.data(), batch.size(), ids.empty() ? nullptr : ids.data(), ids.size(), a.ld_window, a.prune_max_bp, a.min_ac, a.max_ac, &res);
  else if (prune) rc = vs_query_ld_prune(idx, batch.data(), batch.size(), ids.empty() ? nullptr : ids.data(), ids.size(), a.ld_window, a.prune_max_bp, a.prune_threshold, a.min_ac, a.max_ac, &res);
  else if (ldmatrix) rc = vs_query_ld_matrix(idx, batch.data(), batch.size(), ids.empty() ? nullptr : ids.data(), ids.size(), a.ld_dot ? VS_LD_DOT : VS_LD_R2, &res);
  else if (ld) rc = vs_query_ld_band(idx, batch.data(), batch.size(), ids.empty() ? nullptr : ids.data(), ids.size(), a.ld_window, a.ld_dot ? VS_LD_DOT : VS_LD_R2, &res);
  else if (genotypes) rc = vs_query_genotype_matrix(idx, batch.data(), batch.size(), ids.empty() ? nullptr : ids.data(), ids.size(), &res);
  else if (burden) rc = vs_query_sample_burden(idx, batch.data(), batch.size(), ids.empty() ? nullptr : ids.data(), ids.size(), a.min_ac, a.max_ac, &res);
  else rc = vs_query_allele_counts(idx, batch.data(), batch.size(), ids.empty() ? nullptr : ids.data(), ids.size(), &res);
  if (rc != VS_OK) die(rc, ldscore ? "ldscore" : clump ? "clump" : prune ? "prune" : ldmatrix ? "ldmatrix" : ld ? "ld" : genotypes ? "genotypes" : burden ? "burden" : "counts");
  std::ofstream file;
  if (!a.outfile.empty()) file.open(a.outfile, std::ios::binary);
  std::ostream& out = a.outfile.empty() ? std::cout : file;
  for (size_t i = 0; i < batch.size(); ++i) {
    const char* text = nullptr;
    uint64_t len = 0;
    rc = vs_result_format_region(res, i, &text, &len);
    if (rc != VS_OK) die(rc, "result");
    out << "#region " << i << " " << batch[i].x << ":" << batch[i].y << "\n";
    out.write(text, len);
  }
  out.flush();
  vs_result_free(res);
  vs_index_close(idx);
  return EXIT_SUCCESS;
}

}  // namespace

int main(int argc, char** argv) {
  Args a;
  if (argc < 2) return usage();
  a.cmd = argv[1];
  auto need = [&](int& i) -> std::string {
    if (i + 1 >= argc) { std::cerr << "missing value for " << argv[i] << "\n"; exit(EXIT_FAILURE); }
    return argv[++i];
  };
  if (a.cmd == "ldscore") { a.ld_window = 0; a.prune_max_bp = 1000000; }   // no row limit, 1 Mb
  if (a.cmd == "clump") { a.ld_window = 256; a.prune_max_bp = 250000; a.prune_threshold = 524288; }   // plink's defaults: 250 kb, r2 0.5
  for (int i = 2; i < argc; ++i) {
    std::string f = argv[i];
    if (a.cmd == "construct") {
      if (f == "-r" || f == "--reference") a.ref = need(i);
      else if (f == "-v" || f == "--vcf") a.vcf = need(i);
      else if (f == "-p" || f == "--output-prefix") a.prefix = need(i);
      else { std::cerr << "unknown option " << f << "\n"; return EXIT_FAILURE; }
    } else if (a.cmd == "draw") {
      if (f == "-p" || f == "--output-prefix") a.prefix = need(i);
      else if (f == "-r" || f == "--region") a.region = need(i);
      else if (f == "-h" || f == "--hops") { a.hops = (uint64_t)atoll(need(i).c_str()); a.have_hops = true; }
      else if (f == "-s" || f == "--sample-name") a.sample = need(i);
      else { std::cerr << "unknown option " << f << "\n"; return EXIT_FAILURE; }
    } else if (a.cmd == "query") {
      if (f == "-p" || f == "--output-prefix") a.prefix = need(i);
      else if (f == "-t" || f == "--type") { a.type = (uint32_t)atoi(need(i).c_str()); a.have_type = true; }
      else if (f == "-r" || f == "--region") a.region = need(i);
      else if (f == "-m" || f == "--mode") { a.mode = (uint32_t)atoi(need(i).c_str()); a.have_mode = true; }
      else if (f == "-o" || f == "--output_file") a.outfile = need(i);
      else if (f == "-s" || f == "--sample-name") a.sample = need(i);
      else if (f == "-a" || f == "--alt-seq") a.alt = need(i);
      else if (f == "-b" || f == "--ref-seq") a.refseq = need(i);
      else if (f == "-v" || f == "--verbose") a.verbose = true;
      else if (f == "--batch-out") a.batch_out = need(i);
      else if (f == "--device") a.device = atoi(need(i).c_str());
      else if (f == "--ngpus") a.ngpus = std::max(1, atoi(need(i).c_str()));
      else if (f == "--nprocs") a.nprocs = std::max(1, atoi(need(i).c_str()));
      else if (f == "--nprocs-same-device") a.nprocs_same_device = true;
      else if (f == "--resident-lists") a.resident_lists = true;
      else { std::cerr << "unknown option " << f << "\n"; return EXIT_FAILURE; }
    } else if (a.cmd == "counts" || a.cmd == "burden" || a.cmd == "genotypes" || a.cmd == "ld" || a.cmd == "ldmatrix" || a.cmd == "prune" || a.cmd == "clump" || a.cmd == "ldscore" || a.cmd == "groups" || a.cmd == "windows" || a.cmd == "assoc" || a.cmd == "assocmatrix" || a.cmd == "score" || a.cmd == "scorematrix" || a.cmd == "gram" || a.cmd == "ibs" || a.cmd == "trios" || a.cmd == "roh") {
      if (f == "-p" || f == "--output-prefix") a.prefix = need(i);
      else if (a.cmd == "roh" && (f == "--min-sites" || f == "--min-bp" || f == "--max-gap" || f == "--max-het" || f == "--min-ac" || f == "--max-ac")) {
        const std::string v = need(i);
        uint32_t x = 0;
        if (!parse_u32(v, x)) { std::cerr << f << " takes a whole number between 0 and 4294967295, not '" << v << "'\n"; return roh_usage(); }
        if (f == "--min-sites" && x == 0) { std::cerr << "--min-sites takes at least 1\n"; return roh_usage(); }
        if (f == "--max-het" && x > 255) { std::cerr << "--max-het takes at most 255, not " << x << "\n"; return roh_usage(); }
        (f == "--min-sites" ? a.roh_min_sites : f == "--min-bp" ? a.roh_min_bp : f == "--max-gap" ? a.roh_max_gap : f == "--max-het" ? a.roh_max_het
         : f == "--min-ac" ? a.min_ac : a.max_ac) = x;
      }
      else if (a.cmd == "roh" && f == "--summary") a.roh_summary = true;
      else if ((a.cmd == "burden" || a.cmd == "prune" || a.cmd == "ldscore") && f == "--min-ac") a.min_ac = (uint32_t)strtoul(need(i).c_str(), nullptr, 10);
      else if ((a.cmd == "burden" || a.cmd == "prune" || a.cmd == "ldscore") && f == "--max-ac") a.max_ac = (uint32_t)strtoul(need(i).c_str(), nullptr, 10);
      else if ((a.cmd == "ld" || a.cmd == "prune" || a.cmd == "clump" || a.cmd == "ldscore") && (f == "-w" || f == "--window")) a.ld_window = (uint32_t)strtoul(need(i).c_str(), nullptr, 10);
      else if ((a.cmd == "ld" || a.cmd == "ldmatrix") && f == "--dot") a.ld_dot = true;
      else if ((a.cmd == "prune" || a.cmd == "clump" || a.cmd == "ldscore") && f == "--bp") a.prune_max_bp = (uint32_t)strtoul(need(i).c_str(), nullptr, 10);
      else if (a.cmd == "clump" && (f == "-A" || f == "--pvalues")) a.pvalues_file = need(i);
      else if (a.cmd == "clump" && (f == "--p1" || f == "--p2")) {
        const std::string v = need(i);
        char* end = nullptr;
        const double p = strtod(v.c_str(), &end);
        if (v.empty() || *end != '\0' || !(p >= 0.0 && p <= 1.0)) { std::cerr << f << " takes a bound between 0 and 1, not '" << v << "'\n"; return clump_usage(); }
        (f == "--p1" ? a.clump_p1 : a.clump_p2) = p;
      }
      else if ((a.cmd == "prune" || a.cmd == "clump") && f == "--r2") {
        const std::string v = need(i);
        char* end = nullptr;
        const double r2 = strtod(v.c_str(), &end);
        if (v.empty() || *end != '\0' || !(r2 >= 0.0 && r2 <= 1.0)) { std::cerr << "--r2 takes a bound between 0 and 1, not '" << v << "'\n"; return a.cmd == "clump" ? clump_usage() : prune_usage(); }
        a.prune_threshold = (uint32_t)std::floor(r2 * 1048576.0 + 0.5);
      }
      else if (a.cmd == "gram" && f == "--grm") a.gram_grm = true;
      else if (a.cmd == "trios" && (f == "-T" || f == "--trios")) a.trios_file = need(i);
      else if (a.cmd == "trios" && f == "--per-trio") a.trios_per_trio = true;
      else if (a.cmd == "ibs" && f == "--king") a.ibs_king = true;
      else if (a.cmd == "ibs" && f == "--min-kinship") {
        const std::string v = need(i);
        char* end = nullptr;
        a.ibs_min_kinship = strtod(v.c_str(), &end);
        if (v.empty() || *end != '\0' || std::isnan(a.ibs_min_kinship)) { std::cerr << "--min-kinship takes a number, not '" << v << "'\n"; return ibs_usage(); }
        a.ibs_have_min = true;
      }
      else if (f == "-r" || f == "--region") a.region = need(i);
      else if ((a.cmd == "groups" || a.cmd == "windows") && (f == "-G" || f == "--groups")) a.groups_file = need(i);
      else if (a.cmd == "windows" && f == "--no-pairs") a.windows_no_pairs = true;
      else if (a.cmd == "windows" && f == "--derived") a.windows_derived = true;
      else if ((a.cmd == "assoc" || a.cmd == "assocmatrix") && (f == "-P" || f == "--phenotypes")) a.pheno_file = need(i);
      else if ((a.cmd == "assoc" || a.cmd == "assocmatrix") && f == "--chi2") a.assoc_chi2 = true;
      else if ((a.cmd == "score" || a.cmd == "scorematrix") && (f == "-W" || f == "--weights")) a.weights_file = need(i);
      else if (a.cmd != "groups" && a.cmd != "windows" && a.cmd != "assoc" && a.cmd != "assocmatrix" && a.cmd != "trios" && (f == "-S" || f == "--samples")) a.samples_file = need(i);
      else if (f == "-o" || f == "--output_file") a.outfile = need(i);
      else if (f == "--device") a.device = atoi(need(i).c_str());
      else { std::cerr << "unknown option " << f << "\n"; return EXIT_FAILURE; }
    }
  }
  if (a.cmd == "counts") {
    if (a.prefix.empty() || a.region.empty()) return counts_usage();
    return counts_main(a);
  }
  if (a.cmd == "groups") {
    if (a.prefix.empty() || a.region.empty() || a.groups_file.empty()) return groups_usage();
    return groups_main(a);
  }
  if (a.cmd == "windows") {
    if (a.prefix.empty() || a.region.empty()) return windows_usage();
    return groups_main(a, /*windows=*/true);
  }
  if (a.cmd == "assocmatrix") {
    if (a.prefix.empty() || a.region.empty() || a.pheno_file.empty()) return assocmatrix_usage();
    return assoc_main(a, VS_TRAIT_MATRIX_MAX);
  }
  if (a.cmd == "assoc") {
    if (a.prefix.empty() || a.region.empty() || a.pheno_file.empty()) return assoc_usage();
    return assoc_main(a);
  }
  if (a.cmd == "scorematrix") {
    if (a.prefix.empty() || a.region.empty() || a.weights_file.empty()) return scorematrix_usage();
    return score_main(a, true);
  }
  if (a.cmd == "score") {
    if (a.prefix.empty() || a.region.empty() || a.weights_file.empty()) return score_usage();
    return score_main(a);
  }
  if (a.cmd == "burden") {
    if (a.prefix.empty() || a.region.empty()) return burden_usage();
    return counts_main(a, /*burden=*/true);
  }
  if (a.cmd == "genotypes") {
    if (a.prefix.empty() || a.region.empty()) return genotypes_usage();
    return counts_main(a, /*burden=*/false, /*genotypes=*/true);
  }
  if (a.cmd == "prune") {
    if (a.prefix.empty() || a.region.empty()) return prune_usage();
    return counts_main(a, /*burden=*/false, /*genotypes=*/false, /*ld=*/false, /*ldmatrix=*/false, /*prune=*/true);
  }
  if (a.cmd == "ldscore") {
    if (a.prefix.empty() || a.region.empty()) return ldscore_usage();
    return counts_main(a, /*burden=*/false, /*genotypes=*/false, /*ld=*/false, /*ldmatrix=*/false, /*prune=*/false, /*clump=*/false, /*ldscore=*/true);
  }
  if (a.cmd == "clump") {
    if (a.prefix.empty() || a.region.empty() || a.pvalues_file.empty()) return clump_usage();
    return counts_main(a, /*burden=*/false, /*genotypes=*/false, /*ld=*/false, /*ldmatrix=*/false, /*prune=*/false, /*clump=*/true);
  }
  if (a.cmd == "ldmatrix") {
    if (a.prefix.empty() || a.region.empty()) return ldmatrix_usage();
    return counts_main(a, /*burden=*/false, /*genotypes=*/false, /*ld=*/false, /*ldmatrix=*/true);
  }
  if (a.cmd == "ld") {
    if (a.prefix.empty() || a.region.empty()) return ld_usage();
    return counts_main(a, /*burden=*/false, /*genotypes=*/false, /*ld=*/true);
  }
  if (a.cmd == "gram") {
    if (a.prefix.empty() || a.region.empty()) return gram_usage();
    return gram_main(a);
  }
  if (a.cmd == "ibs") {
    if (a.prefix.empty() || a.region.empty()) return ibs_usage();
    return ibs_main(a);
  }
  if (a.cmd == "trios") {
    if (a.prefix.empty() || a.region.empty() || a.trios_file.empty()) return trios_usage();
    return trios_main(a);
  }
  if (a.cmd == "roh") {
    if (a.prefix.empty() || a.region.empty()) return roh_usage();
    if (a.min_ac > a.max_ac) { std::cerr << "--min-ac " << a.min_ac << " is above --max-ac " << a.max_ac << "\n"; return roh_usage(); }
    return roh_main(a);
  }
  if (a.cmd == "construct") {
    if (a.ref.empty() || a.vcf.empty() || a.prefix.empty()) return usage();
    if (!dir_exists(a.prefix)) {
      std::cerr << "The required input directory " << a.prefix << " does not seem to exist.\n";
      return EXIT_FAILURE;
    }
    return construct_main(a);
  }
  if (a.cmd == "query") {
    if (a.prefix.empty() || !a.have_type || a.region.empty() || !a.have_mode) return usage();
    return query_main(a);
  }
  if (a.cmd == "draw") {
    if (a.prefix.empty() || a.region.empty() || !a.have_hops) return usage();
    return draw_main(a);
  }
  return usage();
}
