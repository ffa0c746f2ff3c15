// kmcp-search — `kmcp search` on MI355X: same flags, same 15-column TSV, same trailer (kmcp/cmd/search.go),
// with the per-query work done by libkmcpgpu.so (include/kmcp_gpu.h) instead of the Go search engine.
//
// Mirrors: flags search.go:1031-1107 + root.go:62-82; input handling :793-1000 (single-end, -1/-2 paired-end,
// -g whole file incl. the k-1 N's appended after records 2..m, :899-914); output :436-438 (header), :448-588
// (rows), :1022-1025 (trailer); fatal errors as checkError (util-cli.go:35-40: message + exit status 255).
// Threads: one reader (FASTA/Q, gz via zlib; it runs up to 8 parser threads on a plain FASTQ file, a second reader for the mates of -1/-2,
// up to 8 file parsers for -g) -> two searchers that keep GPU batches in flight (one for a paged index) -> the main thread as the ordered
// writer, with its pool of -j formatter threads and a flusher thread that writes the file.  What they share is struct Pipeline below.
#include <errno.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <optional>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include <dirent.h>
#include <fcntl.h>
#include <sched.h>
#include <unistd.h>
#include <sys/stat.h>

#include "../include/kmcp_gpu.h"

static const char* VERSION = "0.9.5-mi355x";
static bool g_quiet = false;
static FILE* g_log = nullptr;

static void logf(const char* level, const char* fmt, va_list ap) {
  char buf[2048];
  vsnprintf(buf, sizeof buf, fmt, ap);
  time_t t = time(nullptr);
  struct tm tmv;
  localtime_r(&t, &tmv);
  char ts[32];
  strftime(ts, sizeof ts, "%H:%M:%S.000", &tmv);
  fprintf(stderr, "%s [%s] %s\n", ts, level, buf);
  if (g_log) fprintf(g_log, "%s [%s] %s\n", ts, level, buf);
}
static void info(const char* fmt, ...) {
  if (g_quiet && !g_log) return;
  va_list ap;
  va_start(ap, fmt);
  logf("INFO", fmt, ap);
  va_end(ap);
}
static void warn(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  logf("WARN", fmt, ap);
  va_end(ap);
}
[[noreturn]] void die(const char* fmt, ...) {  // checkError: log + os.Exit(-1)
  va_list ap;
  va_start(ap, fmt);
  logf("ERRO", fmt, ap);
  va_end(ap);
  exit(255);
}

// ------------------------------------------------------------------------------------------------
// options
// ------------------------------------------------------------------------------------------------
struct Options {
  std::string db_dir, out_file = "-", read1, read2, query_id, sort_by = "qcov", infile_list, log_file;
  std::vector<std::string> name_maps, files;
  // --specific-level / --taxid-map / --taxdump: only the queries whose matches point at one target (strain, assembly) or one species are
  // written — what `kmcp-filter -f 1 -t 0 --level L -T ... -X ...` makes of the plain output (K4 of the library, kmcpg_set_specific)
  std::string specific_level, taxdump;
  std::vector<std::string> taxid_maps;
  // --ref-stats FILE [--ref-stats-*]: stage 1/4 of `kmcp profile` counted on the GPU while the search runs — the file is what
  // `kmcp-refstats -f 1 -t 0 -m N --level L ...` writes from this run's unfiltered TSV (K6 of the library, kmcpg_set_refstats)
  std::string ref_stats, ref_stats_level;
  int ref_stats_mode = 3;
  double ref_stats_h = 0.75, ref_stats_p = 0.8;
  bool ref_stats_h_given = false, ref_stats_p_given = false;
  const char* ref_stats_flag = nullptr;  // the first --ref-stats-* flag other than --ref-stats that was given
  // --ref-stats-cooccur FILE [--ref-stats-cooccur-slots N]: stage 2/4 beside it — the reads shared by every pair of kept references; the
  // file is what `kmcp-refstats -f 1 -t 0 ... --cooccur FILE` writes from this run's TSV (K7 of the library, kmcpg_set_cooccur)
  std::string ref_stats_cooccur;
  long long ref_stats_cooccur_slots = 0;  // the pair table's slots, a power of two; 0: the library's default
  // --ref-stats-recount FILE [--ref-stats-no-amb-corr] [--ref-stats-min-dreads-prop D] [--ref-stats-max-mismatch-err R]
  // [--ref-stats-recount-log-mb N]: stage 3/4 behind the two — the recount with ambiguity correction; the file is what
  // kmcp-refstats --recount writes from the search result
  std::string ref_stats_recount;
  bool ref_stats_no_amb_corr = false;
  double ref_stats_d = 0.05, ref_stats_r = 0.05;
  long long ref_stats_recount_log_mb = -1;  // the read log in device memory; -1: the library's default
  const char* recount_flag = nullptr;       // the first of the four optional flags that was given
  // --ref-stats-profile FILE [--ref-stats-abund-max-iters I] [--ref-stats-abund-pct-threshold X] [--ref-stats-filter-low-pct F]: stage 4/4
  // behind the three — the abundances by EM over the logs stage 3 keeps; the file is what kmcp-refstats --profile writes from the search result
  std::string ref_stats_profile;
  // --ref-stats-only: the same files, and no search result — the batches go through kmcpg_submit_stats / kmcpg_wait_stats, no match leaves
  // the GPU but those of the reads the counting stages left to the host
  bool ref_stats_only = false;
  // --binning FILE --binning-refs LIST --taxid-map ... --taxdump ... [--binning-sample-id S]: the binning file of `kmcp profile -B` and no
  // search result — the batches go through kmcpg_submit_bins / kmcpg_wait_bins (K11 of the library, kmcpg_set_binning), four bytes per read
  // leave the GPU; the file is what `kmcp-refstats -f 1 -t 0 ... --profile P --binning FILE` writes from this search's TSV when LIST = P
  std::string binning, binning_refs, binning_sample_id;
  const char* binning_flag = nullptr;  // the first --binning-* flag other than --binning that was given
  long long ref_stats_iters = 10;
  double ref_stats_pct = 0.01, ref_stats_filter = 0;
  const char* profile_flag = nullptr;       // the first of the three optional flags that was given
  std::vector<std::string> also_dbs;  // --also-db: further databases searched in the same pass, the output merged as kmcp-merge would
  bool gpus_given = false;
  int min_qlen = 30, min_kmers = 10, dedup = 256, top_scores = 0, threads = 0, device = 0, batch = 131072, gpus = 1, gpu_passes = -1;
  bool batch_given = false;
  // --sliding-step / --sliding-window / --sliding-greedy: every record searched as the windows `seqkit sliding -s S -W W [-g]` would cut
  // --regions-bed FILE [--regions-*]: with --specific-level and --sliding-*, the specific windows merged into regions (BED6) — what
  // kmcp-filter and kmcp-regions make of the sliding search's TSV, without the TSV (K5 of the library, kmcpg_submit_windows_summary)
  std::string regions_bed, regions_name_species = "species-specific", regions_name_assembly = "assembly-specific";
  long long regions_min_overlap = 1, regions_max_gap = 0;
  bool regions_ignore_type = false, out_file_given = false;
  const char* regions_flag = nullptr;  // the first --regions-* flag other than --regions-bed that was given
  long long sliding_step = 0, sliding_window = 0;
  bool sliding_step_given = false, sliding_window_given = false, sliding_greedy = false;
  std::vector<int32_t> gpu_ids;
  double min_qcov = 0.55, min_tcov = 0, max_fpr = 0.01;
  bool load_whole = false, low_mem = false, whole_file = false, use_filename = false, keep_unmatched = false, no_header = false,
       do_not_sort = false, default_name_map = false, try_se = false, quiet = false, parse_only = false;
};

static void usage() {
  fputs(
      "kmcp-search: search sequences against a kmcp database on an AMD MI355X GPU\n\n"
      "Usage:\n  kmcp-search [-w] -d <kmcp db> [-t <min-query-cov>] [read1.fq.gz] [read2.fq.gz] [unpaired.fq.gz] [-o read.tsv.gz]\n\n"
      "Flags (identical to `kmcp search`, kmcp/cmd/search.go:1031-1107):\n"
      "  -d, --db-dir string            database directory created by \"kmcp index\"\n"
      "  -1, --read1 / -2, --read2      paired-end files;   --try-se   retry unmatched pairs with read1, then read2\n"
      "  -o, --out-file string          out file, \".gz\" supported (default \"-\")\n"
      "  -t, --min-query-cov float      (default 0.55)      -T, --min-target-cov float (default 0)\n"
      "  -c, --min-kmers int            (default 10)        -m, --min-query-len int    (default 30)\n"
      "  -f, --max-fpr float            (default 0.01)      -u, --kmer-dedup-threshold int (default 256)\n"
      "  -s, --sort-by qcov|tcov|jacc   -S, --do-not-sort   -n, --keep-top-scores int  -K, --keep-unmatched  -H, --no-header-row\n"
      "  -g, --query-whole-file         -G, --use-filename  --query-id string\n"
      "  -N, --name-map file(s)         -D, --default-name-map\n"
      "  -w, --load-whole-db / --low-mem  accepted for compatibility (the index is always resident in HBM)\n"
      "  -j, --threads int  -i, --infile-list file  -q, --quiet  --log file\n"
      "GPU flags: --gpu int (device, default 0)  --gpus int (use devices 0..N-1, index blocks partitioned over them)\n"
      "           --gpu-ids a,b,c (explicit device list)  --gpu-batch int (queries per GPU call, default 131072)\n"
      "           --gpu-passes int (an index larger than the GPU's memory is searched in this many passes per batch, one part\n"
      "                             resident at a time; 0 = as few as fit; default: only when the index does not fit)\n"
      "           --also-db dir (repeatable, up to 15) search these databases too, in the same pass: all of them resident on the one GPU, the\n"
      "                             reads parsed once, and the output is what `kmcp-merge -s <the same -s>` makes of one kmcp-search run per\n"
      "                             database (-d first, then every --also-db in order).  The databases must agree in k, sketching, number of\n"
      "                             hashes and FPR.  Not with -K, --try-se, -S, -n, -g/-G, --sliding-*, --gpus/--gpu-ids, --gpu-passes.\n"
      "           --specific-level species|strain|assembly [--taxid-map file(s) --taxdump dir]\n"
      "                             write only the queries whose matches point at one target (strain, assembly) or lie under one species:\n"
      "                             the output is what `kmcp-filter -f 1 -t 0 --level L -T ... -X ...` makes of this command's output\n"
      "                             without these flags, followed by the trailer; the decision is made on the GPU.  Targets are the printed\n"
      "                             ones (after -N / -D); at level species every target of the database needs a TaxId.\n"
      "                             Not with -K, --try-se, -n, --sliding-* (except for --regions-bed), --gpus/--gpu-ids, --gpu-passes.\n"
      "           --ref-stats file [--ref-stats-mode int (3)] [--ref-stats-min-hic-ureads-qcov float] [--ref-stats-min-chunks-fraction float]\n"
      "                             [--ref-stats-level species|strain|assembly] [--taxid-map file(s) --taxdump dir]\n"
      "                             [--ref-stats-cooccur file [--ref-stats-cooccur-slots int]]\n"
      "                             [--ref-stats-recount file [--ref-stats-no-amb-corr] [--ref-stats-min-dreads-prop float (0.05)]\n"
      "                              [--ref-stats-max-mismatch-err float (0.05)] [--ref-stats-recount-log-mb int]\n"
      "                              [--ref-stats-profile file [--ref-stats-abund-max-iters int (10)] [--ref-stats-abund-pct-threshold float (0.01)]\n"
      "                               [--ref-stats-filter-low-pct float (0)]]] [--ref-stats-only]\n"
      "                             count, on the GPU while the search runs, what stage 1/4 of `kmcp profile` counts per reference (reads,\n"
      "                             uniquely matched reads, high-confidence ones, chunks covered) and judge which references are in the\n"
      "                             sample: the file is what `kmcp-refstats -f 1 -t 0 -m N --level L ...` writes from this command's\n"
      "                             unfiltered output, which is written as before.  Modes 1-5 are kmcp profile's presets (mode 0 cuts\n"
      "                             rows: use kmcp-refstats).  The level defaults to species with --taxid-map and --taxdump, else strain.\n"
      "                             Not with what --specific-level refuses.\n"
      "                             --ref-stats-recount (with --ref-stats and --ref-stats-cooccur): stage 3/4 as well — the reads recounted\n"
      "                             with ambiguity correction and the references judged with the mode's thresholds; the file is what\n"
      "                             `kmcp-refstats ... --recount` writes from this command's output.\n"
      "                             --ref-stats-profile (with --ref-stats-recount): stage 4/4 as well — the abundances estimated by EM on the\n"
      "                             GPU, one pass per iteration over the reads stage 3 kept; the table `kmcp-refstats ... --profile` writes.\n"
      "                             --ref-stats-only: write the --ref-stats* files and NO search result — byte for byte the files of the\n"
      "                             same command without it, but no match leaves the GPU except those of the reads its counting kernels\n"
      "                             leave to the host, and no row is formatted.  Not with -o, --specific-level, --regions-bed, --also-db, -g.\n"
      "           --binning file --binning-refs file --taxid-map file[,file...] --taxdump dir [--binning-sample-id string]\n"
      "                             write the binning result of `kmcp profile -B` (CAMI format: one TaxId per read — that of its reference,\n"
      "                             or the lowest common ancestor of its references) and NO search result: the reads are searched and\n"
      "                             binned on the GPU, four bytes per read leave it.  --binning-refs lists the references to bin over, the\n"
      "                             first column of every line that does not start with '#': a profile of --ref-stats-profile or\n"
      "                             kmcp-refstats --profile as it is.  The file is what `kmcp-refstats -f 1 -t 0 ... --profile P --binning`\n"
      "                             writes from the search result; \".binning.gz\" is appended unless the name ends in \".binning[.gz]\".\n"
      "                             Not with -o, any --ref-stats* flag, or what --ref-stats-only refuses.\n"
      "           --parse-only (read the inputs and print records / bases / checksum per file; no database, no GPU)\n"
      "           --regions-bed file [--regions-min-overlap int (1)] [--regions-max-gap int (0)] [--regions-ignore-type]\n"
      "                             [--regions-name-species string] [--regions-name-assembly string]\n"
      "                             with --specific-level AND --sliding-step/--sliding-window: merge the specific windows of every\n"
      "                             record into regions (BED6; .gz honoured) — what kmcp-filter -f 1 -t 0 and kmcp-regions -f 1 -t 0 make\n"
      "                             of the sliding search's output, in one pass.  No search result is written: not with -o.\n"
      "Long reads and contigs (the reference's advice: split them with `seqkit sliding -s 100 -W 300`, search the pieces):\n"
      "           --sliding-step int --sliding-window int [--sliding-greedy]\n"
      "                             search every window of every record, as `seqkit sliding -s S -W W [-g] | kmcp search` would,\n"
      "                             without the window text: queries are named <id>_sliding:<start>-<end> (1-based, inclusive),\n"
      "                             queryIdx and \"# input queries\" count windows.  Both values are needed (>= 1); single-end input\n"
      "                             only, not with -g/-G or --query-id.  --sliding-greedy keeps the last windows, cut at the end.\n",
      stderr);
}

static double to_f(const std::string& flag, const std::string& v) {
  char* e = nullptr;
  double d = strtod(v.c_str(), &e);
  if (!e || *e || v.empty()) die("invalid argument \"%s\" for \"%s\" flag", v.c_str(), flag.c_str());
  return d;
}
static int to_i(const std::string& flag, const std::string& v) {
  char* e = nullptr;
  long d = strtol(v.c_str(), &e, 10);
  if (!e || *e || v.empty()) die("invalid argument \"%s\" for \"%s\" flag", v.c_str(), flag.c_str());
  return (int)d;
}

static Options parse_args(int argc, char** argv) {
  Options o;
  struct Spec { const char* lng; char sht; int kind; };  // kind 0 bool, 1 value
  static const Spec specs[] = {
      {"db-dir", 'd', 1}, {"out-file", 'o', 1}, {"read1", '1', 1}, {"read2", '2', 1}, {"try-se", 0, 0}, {"load-whole-db", 'w', 0},
      {"low-mem", 0, 0}, {"kmer-dedup-threshold", 'u', 1}, {"query-whole-file", 'g', 0}, {"use-filename", 'G', 0}, {"query-id", 0, 1},
      {"min-kmers", 'c', 1}, {"min-query-len", 'm', 1}, {"min-query-cov", 't', 1}, {"min-target-cov", 'T', 1}, {"max-fpr", 'f', 1},
      {"name-map", 'N', 1}, {"default-name-map", 'D', 0}, {"keep-unmatched", 'K', 0}, {"keep-top-scores", 'n', 1}, {"no-header-row", 'H', 0},
      {"sort-by", 's', 1}, {"do-not-sort", 'S', 0}, {"threads", 'j', 1}, {"quiet", 'q', 0}, {"infile-list", 'i', 1}, {"log", 0, 1},
      {"gpu", 0, 1}, {"gpu-batch", 0, 1}, {"gpus", 0, 1}, {"gpu-ids", 0, 1}, {"gpu-passes", 0, 1}, {"parse-only", 0, 0}, {"help", 'h', 0}, {"version", 'V', 0},
      {"sliding-step", 0, 1}, {"sliding-window", 0, 1}, {"sliding-greedy", 0, 0}, {"also-db", 0, 1},
      {"specific-level", 0, 1}, {"taxid-map", 0, 1}, {"taxdump", 0, 1},
      {"ref-stats", 0, 1}, {"ref-stats-mode", 0, 1}, {"ref-stats-min-hic-ureads-qcov", 0, 1}, {"ref-stats-min-chunks-fraction", 0, 1}, {"ref-stats-level", 0, 1}, {"ref-stats-cooccur", 0, 1}, {"ref-stats-cooccur-slots", 0, 1},
      {"ref-stats-recount", 0, 1}, {"ref-stats-no-amb-corr", 0, 0}, {"ref-stats-min-dreads-prop", 0, 1}, {"ref-stats-max-mismatch-err", 0, 1}, {"ref-stats-recount-log-mb", 0, 1},
      {"ref-stats-only", 0, 0}, {"ref-stats-profile", 0, 1}, {"ref-stats-abund-max-iters", 0, 1}, {"ref-stats-abund-pct-threshold", 0, 1}, {"ref-stats-filter-low-pct", 0, 1},
      {"binning", 0, 1}, {"binning-refs", 0, 1}, {"binning-sample-id", 0, 1},
      {"regions-bed", 0, 1}, {"regions-min-overlap", 0, 1}, {"regions-max-gap", 0, 1}, {"regions-ignore-type", 0, 0},
      {"regions-name-species", 0, 1}, {"regions-name-assembly", 0, 1}};
  auto regions_flag = [&](const char* flag) {
    if (!o.regions_flag) o.regions_flag = flag;
  };
  auto apply = [&](const std::string& name, const std::string& v) {
    if (name == "db-dir") o.db_dir = v;
    else if (name == "out-file") { o.out_file = v; o.out_file_given = true; }
    else if (name == "regions-bed") o.regions_bed = v;
    else if (name == "regions-min-overlap") { o.regions_min_overlap = to_i(name, v); regions_flag("--regions-min-overlap"); }
    else if (name == "regions-max-gap") { o.regions_max_gap = to_i(name, v); regions_flag("--regions-max-gap"); }
    else if (name == "regions-ignore-type") { o.regions_ignore_type = true; regions_flag("--regions-ignore-type"); }
    else if (name == "regions-name-species") { o.regions_name_species = v; regions_flag("--regions-name-species"); }
    else if (name == "regions-name-assembly") { o.regions_name_assembly = v; regions_flag("--regions-name-assembly"); }
    else if (name == "read1") o.read1 = v;
    else if (name == "read2") o.read2 = v;
    else if (name == "try-se") o.try_se = true;
    else if (name == "load-whole-db") o.load_whole = true;
    else if (name == "low-mem") o.low_mem = true;
    else if (name == "kmer-dedup-threshold") o.dedup = to_i(name, v);
    else if (name == "query-whole-file") o.whole_file = true;
    else if (name == "use-filename") o.use_filename = true;
    else if (name == "query-id") o.query_id = v;
    else if (name == "min-kmers") o.min_kmers = to_i(name, v);
    else if (name == "min-query-len") o.min_qlen = to_i(name, v);
    else if (name == "min-query-cov") o.min_qcov = to_f(name, v);
    else if (name == "min-target-cov") o.min_tcov = to_f(name, v);
    else if (name == "max-fpr") o.max_fpr = to_f(name, v);
    else if (name == "name-map") {
      size_t b = 0;  // StringSlice: comma separated and repeatable
      while (b <= v.size()) {
        size_t e = v.find(',', b);
        if (e == std::string::npos) e = v.size();
        if (e > b) o.name_maps.push_back(v.substr(b, e - b));
        b = e + 1;
      }
    } else if (name == "default-name-map") o.default_name_map = true;
    else if (name == "keep-unmatched") o.keep_unmatched = true;
    else if (name == "keep-top-scores") o.top_scores = to_i(name, v);
    else if (name == "no-header-row") o.no_header = true;
    else if (name == "sort-by") o.sort_by = v;
    else if (name == "do-not-sort") o.do_not_sort = true;
    else if (name == "threads") o.threads = to_i(name, v);
    else if (name == "quiet") o.quiet = true;
    else if (name == "infile-list") o.infile_list = v;
    else if (name == "log") o.log_file = v;
    else if (name == "gpu") o.device = to_i(name, v);
    else if (name == "gpu-batch") { o.batch = to_i(name, v); o.batch_given = true; }
    else if (name == "gpu-passes") o.gpu_passes = to_i(name, v);
    else if (name == "parse-only") o.parse_only = true;
    else if (name == "sliding-step") { o.sliding_step = to_i(name, v); o.sliding_step_given = true; }
    else if (name == "sliding-window") { o.sliding_window = to_i(name, v); o.sliding_window_given = true; }
    else if (name == "sliding-greedy") o.sliding_greedy = true;
    else if (name == "also-db") o.also_dbs.push_back(v);
    else if (name == "ref-stats") o.ref_stats = v;
    else if (name == "ref-stats-mode") { o.ref_stats_mode = to_i(name, v); if (!o.ref_stats_flag) o.ref_stats_flag = "--ref-stats-mode"; }
    else if (name == "ref-stats-min-hic-ureads-qcov") { o.ref_stats_h = to_f(name, v); o.ref_stats_h_given = true; if (!o.ref_stats_flag) o.ref_stats_flag = "--ref-stats-min-hic-ureads-qcov"; }
    else if (name == "ref-stats-min-chunks-fraction") { o.ref_stats_p = to_f(name, v); o.ref_stats_p_given = true; if (!o.ref_stats_flag) o.ref_stats_flag = "--ref-stats-min-chunks-fraction"; }
    else if (name == "ref-stats-cooccur") { o.ref_stats_cooccur = v; if (!o.ref_stats_flag) o.ref_stats_flag = "--ref-stats-cooccur"; }
    else if (name == "ref-stats-recount") { o.ref_stats_recount = v; if (!o.ref_stats_flag) o.ref_stats_flag = "--ref-stats-recount"; }
    else if (name == "ref-stats-no-amb-corr") { o.ref_stats_no_amb_corr = true; if (!o.recount_flag) o.recount_flag = "--ref-stats-no-amb-corr"; }
    else if (name == "ref-stats-min-dreads-prop") { o.ref_stats_d = to_f(name, v); if (!o.recount_flag) o.recount_flag = "--ref-stats-min-dreads-prop"; }
    else if (name == "ref-stats-max-mismatch-err") { o.ref_stats_r = to_f(name, v); if (!o.recount_flag) o.recount_flag = "--ref-stats-max-mismatch-err"; }
    else if (name == "ref-stats-recount-log-mb") { o.ref_stats_recount_log_mb = to_i(name, v); if (o.ref_stats_recount_log_mb < 0) o.ref_stats_recount_log_mb = 0; if (!o.recount_flag) o.recount_flag = "--ref-stats-recount-log-mb"; }
    else if (name == "ref-stats-profile") o.ref_stats_profile = v;
    else if (name == "ref-stats-only") o.ref_stats_only = true;
    else if (name == "binning") o.binning = v;
    else if (name == "binning-refs") { o.binning_refs = v; if (!o.binning_flag) o.binning_flag = "--binning-refs"; }
    else if (name == "binning-sample-id") { o.binning_sample_id = v; if (!o.binning_flag) o.binning_flag = "--binning-sample-id"; }
    else if (name == "ref-stats-abund-max-iters") { o.ref_stats_iters = to_i(name, v); if (!o.profile_flag) o.profile_flag = "--ref-stats-abund-max-iters"; }
    else if (name == "ref-stats-abund-pct-threshold") { o.ref_stats_pct = to_f(name, v); if (!o.profile_flag) o.profile_flag = "--ref-stats-abund-pct-threshold"; }
    else if (name == "ref-stats-filter-low-pct") { o.ref_stats_filter = to_f(name, v); if (!o.profile_flag) o.profile_flag = "--ref-stats-filter-low-pct"; }
    else if (name == "ref-stats-cooccur-slots") { o.ref_stats_cooccur_slots = to_i(name, v); if (!o.ref_stats_flag) o.ref_stats_flag = "--ref-stats-cooccur-slots"; }
    else if (name == "ref-stats-level") { o.ref_stats_level = v; for (char& c : o.ref_stats_level) c = (char)tolower((unsigned char)c); if (!o.ref_stats_flag) o.ref_stats_flag = "--ref-stats-level"; }
    else if (name == "specific-level") { o.specific_level = v; for (char& c : o.specific_level) c = (char)tolower((unsigned char)c); }
    else if (name == "taxdump") o.taxdump = v;
    else if (name == "taxid-map") {
      size_t b = 0;  // StringSlice: comma separated and repeatable
      while (b <= v.size()) {
        size_t e = v.find(',', b);
        if (e == std::string::npos) e = v.size();
        if (e > b) o.taxid_maps.push_back(v.substr(b, e - b));
        b = e + 1;
      }
    }
    else if (name == "gpus") { o.gpus = to_i(name, v); o.gpus_given = true; }
    else if (name == "gpu-ids") {
      o.gpus_given = true;
      size_t b = 0;
      while (b <= v.size()) {
        size_t e = v.find(',', b);
        if (e == std::string::npos) e = v.size();
        if (e > b) o.gpu_ids.push_back(to_i(name, v.substr(b, e - b)));
        b = e + 1;
      }
    }
    else if (name == "help") { usage(); exit(0); }
    else if (name == "version") { printf("kmcp-search v%s\n", VERSION); exit(0); }
  };
  bool only_pos = false;
  int first = 1;
  // `kmcp-search search ...` = `kmcp search ...`: cobra's sub-command word, accepted (only) as the first argument
  if (argc > 1 && strcmp(argv[1], "search") == 0) first = 2;
  for (int i = first; i < argc; i++) {
    std::string a = argv[i];
    if (only_pos || a == "-" || a.empty() || a[0] != '-') { o.files.push_back(a); continue; }
    if (a == "--") { only_pos = true; continue; }
    if (a[1] == '-') {
      std::string name = a.substr(2), val;
      bool has = false;
      size_t eq = name.find('=');
      if (eq != std::string::npos) { val = name.substr(eq + 1); name = name.substr(0, eq); has = true; }
      const Spec* sp = nullptr;
      for (const auto& s : specs) if (name == s.lng) sp = &s;
      if (!sp) die("unknown flag: --%s", name.c_str());
      if (sp->kind == 1 && !has) {
        if (i + 1 >= argc) die("flag needs an argument: --%s", name.c_str());
        val = argv[++i];
      }
      apply(sp->lng, val);
    } else {
      for (size_t p = 1; p < a.size(); p++) {
        const Spec* sp = nullptr;
        for (const auto& s : specs) if (s.sht && a[p] == s.sht) sp = &s;
        if (!sp) die("unknown shorthand flag: '%c' in %s", a[p], a.c_str());
        if (sp->kind == 0) { apply(sp->lng, ""); continue; }
        std::string val = a.substr(p + 1);
        if (!val.empty() && val[0] == '=') val = val.substr(1);
        if (val.empty()) {
          if (i + 1 >= argc) die("flag needs an argument: '%c' in %s", a[p], a.c_str());
          val = argv[++i];
        }
        apply(sp->lng, val);
        break;
      }
    }
  }
  return o;
}

#include "../kmcp_amd/csrc/taxonomy.hpp"
#include "../kmcp_amd/csrc/regions_rule.hpp"
#include "../kmcp_amd/csrc/refstats_rule.hpp"
#include "../kmcp_amd/csrc/bin_rule.hpp"
#include "binning_format.hpp"
#include "recount_format.hpp"
#include "profile_format.hpp"
#include "search_batch.hpp"
#include "row_format.hpp"

using Clock = std::chrono::steady_clock;
static inline double seconds_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// one 64-bit word per (query, column, count) tuple, summed mod 2^64 over a run: bench.py's hits_checksum (kmcp_amd/dist.py) in C++
static inline uint64_t tuple_mix(uint64_t query, uint32_t col, uint32_t count) {
  uint64_t x = query * 0x9E3779B97F4A7C15ULL + (uint64_t)col * 0xC2B2AE3D27D4EB4FULL + (uint64_t)count * 0x165667B19E3779F9ULL;
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ULL;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBULL;
  x ^= x >> 31;
  return x;
}

// On a two-socket host the threads of this process — parsers, searchers, formatters, the flusher — pass every batch from one to the next;
// spread over both sockets each hand-over crosses the interconnect (formatting cost 1.5-2x the thread-seconds, profiles/r06_cli_e2e.txt).
// When the affinity mask spans several NUMA nodes and one node has the cores the CPU quota grants anyway, the process keeps to the node it
// was started on (KMCP_SEARCH_NUMA=<node> picks another, KMCP_SEARCH_NUMA=off leaves the mask alone).  Called before any thread exists.
static void keep_to_one_numa_node() {
  const char* env = getenv("KMCP_SEARCH_NUMA");
  if (env && (!strcmp(env, "off") || !strcmp(env, "no"))) return;
  cpu_set_t mask;
  if (sched_getaffinity(0, sizeof mask, &mask) != 0) return;
  std::vector<cpu_set_t> nodes;
  for (int n = 0; n < 64; n++) {
    char path[96];
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", n);
    FILE* f = fopen(path, "r");
    if (!f) break;
    char buf[4096];
    cpu_set_t cs;
    CPU_ZERO(&cs);
    if (fgets(buf, sizeof buf, f))
      for (char* tok = strtok(buf, ",\n"); tok; tok = strtok(nullptr, ",\n")) {
        int a = 0, b = 0;
        const int got = sscanf(tok, "%d-%d", &a, &b);
        if (got == 1) b = a;
        if (got >= 1)
          for (int c = a; c <= b && c < CPU_SETSIZE; c++) CPU_SET(c, &cs);
      }
    fclose(f);
    cpu_set_t both;
    CPU_AND(&both, &cs, &mask);
    nodes.push_back(both);
  }
  int spanned = 0;
  for (const auto& n : nodes) spanned += CPU_COUNT(&n) > 0;
  if (spanned < 2) return;
  int want = -1;
  if (env && *env >= '0' && *env <= '9') want = atoi(env);
  else {
    const int cpu = sched_getcpu();
    for (size_t n = 0; n < nodes.size(); n++)
      if (cpu >= 0 && CPU_ISSET(cpu, &nodes[n])) want = (int)n;
  }
  if (want < 0 || want >= (int)nodes.size() || (unsigned)CPU_COUNT(&nodes[(size_t)want]) < std::min(usable_cpus(), 4u)) return;
  (void)sched_setaffinity(0, sizeof(cpu_set_t), &nodes[(size_t)want]);
}

static std::unordered_map<std::string, std::string> read_kvs(const std::string& file) {  // cliutil.ReadKVs
  std::unordered_map<std::string, std::string> m;
  gzFile g = gzopen(file.c_str(), "rb");
  if (!g) die("%s: %s", file.c_str(), strerror(errno));
  char buf[1 << 16];
  while (gzgets(g, buf, sizeof buf)) {
    size_t n = strlen(buf);
    while (n && (buf[n - 1] == '\n' || buf[n - 1] == '\r')) buf[--n] = 0;
    if (!n || buf[0] == '#') continue;
    char* tab = strchr(buf, '\t');
    if (!tab) continue;
    *tab = 0;
    m[buf] = tab + 1;
  }
  gzclose(g);
  return m;
}

static std::string trim_ext(const std::string& path) {  // filepathTrimExtension: basename without (.gz/.xz/..)+ext
  size_t s = path.find_last_of('/');
  std::string b = s == std::string::npos ? path : path.substr(s + 1);
  for (const char* z : {".gz", ".xz", ".zst", ".bz2"}) {
    size_t l = strlen(z);
    if (b.size() > l && b.compare(b.size() - l, l, z) == 0) { b.resize(b.size() - l); break; }
  }
  size_t d = b.find_last_of('.');
  if (d != std::string::npos && d > 0) b.resize(d);
  return b;
}

// ---- --parse-only: reader check, no database and no GPU: one summary line per input file
// checksum = sum over records i (0-based, in file order) of fnv1a("id\tseq\n") * (2 i + 1) mod 2^64: order-sensitive, yet
// every batch can be summed on its own thread
// (pairs, -1/-2: "id\tseq1\tseq2\n")
struct ParseTotals {
  std::mutex mu;
  uint64_t n = 0, bases = 0, id_bytes = 0, sum = 0;
};

static void parse_only_worker(Queue<std::unique_ptr<Batch>>& q, ParseTotals& tot) {
  std::unique_ptr<Batch> b;
  uint64_t my_sum = 0, my_bases = 0, my_ids = 0, my_n = 0;
  while (q.pop(&b)) {
    for (size_t i = 0; i < b->size(); i++) {
      uint64_t h = 1469598103934665603ULL;
      auto mix = [&](const char* p, size_t len) {
        for (size_t j = 0; j < len; j++) h = (h ^ (uint8_t)p[j]) * 1099511628211ULL;
      };
      mix(b->id_buf.data() + b->id_offs[i], (size_t)(b->id_offs[i + 1] - b->id_offs[i]));
      mix("\t", 1);
      mix((const char*)b->seqs.data() + b->offs[i], (size_t)(b->offs[i + 1] - b->offs[i]));
      if (b->paired) {
        mix("\t", 1);
        mix((const char*)b->seqs2.data() + b->offs2[i], (size_t)(b->offs2[i + 1] - b->offs2[i]));
      }
      mix("\n", 1);
      my_sum += h * (2 * (b->first_idx + i) + 1);
    }
    my_n += b->size();
    my_bases += b->seqs.size() + b->seqs2.size();
    my_ids += b->id_buf.size();
  }
  std::lock_guard<std::mutex> g(tot.mu);
  tot.sum += my_sum;
  tot.n += my_n;
  tot.bases += my_bases;
  tot.id_bytes += my_ids;
}

static int run_parse_only(const Options& o) {
  const bool pe = !o.read1.empty() && !o.read2.empty();
  std::vector<std::string> inputs = pe ? std::vector<std::string>{o.read1 + "," + o.read2} : o.files;
  for (const auto& file : inputs) {
    const auto t0 = Clock::now();
    Queue<std::unique_ptr<Batch>> q(8);
    ParseTotals tot;
    std::vector<std::thread> th;
    for (int t = 0; t < 4; t++) th.emplace_back(parse_only_worker, std::ref(q), std::ref(tot));
    uint64_t idx = 0;
    auto emit = [&](std::unique_ptr<Batch> b) {
      b->first_idx = idx;
      idx += b->size();
      q.push(std::move(b));
    };
    if (pe) read_paired(o.read1, o.read2, (size_t)o.batch, 64u << 20, emit);
    else read_single_end(file, (size_t)o.batch, 64u << 20, emit);
    q.close();
    for (auto& t : th) t.join();
    const double dt = seconds_since(t0);
    printf("%s\trecords=%llu\tbases=%llu\tid_bytes=%llu\tfnv1a=%016llx\n", file.c_str(), (unsigned long long)tot.n, (unsigned long long)tot.bases,
           (unsigned long long)tot.id_bytes, (unsigned long long)tot.sum);
    if (!o.quiet) fprintf(stderr, "%s: %.3f s, %.2f M records/s\n", file.c_str(), dt, tot.n / dt / 1e6);
  }
  return 0;
}

// ---- stages before the pipeline runs: flags, input files, databases, name maps
// Dies with the first complaint — the ORDER of the checks is what a user with two mistakes sees (tests/test_sliding_cpu.py pins it) — and
// returns kmcpg_params::sort_by.
static int validate_flags(const Options& o, bool sliding) {
  // --specific-level: what would judge something else than a query's final matches, and the handles that do not hold them in one place,
  // are refused here, before a file or a GPU is touched (the words of kmcp utils filter where it has them, filter.go:93-114)
  if (o.specific_level.empty() && o.ref_stats.empty() && o.binning.empty() && (!o.taxid_maps.empty() || !o.taxdump.empty()))
    die("flags --taxid-map and --taxdump are only used with --specific-level");
  // --binning: no search result is written and no counting stage runs; what --ref-stats-only refuses is refused here, for its reasons
  if (o.binning.empty() && o.binning_flag) die("flag %s is only used with --binning", o.binning_flag);
  if (!o.binning.empty()) {
    const char* stats = !o.ref_stats.empty() ? "--ref-stats" : o.ref_stats_flag ? o.ref_stats_flag : o.recount_flag ? o.recount_flag : !o.ref_stats_profile.empty() ? "--ref-stats-profile"
                        : o.profile_flag ? o.profile_flag : o.ref_stats_only ? "--ref-stats-only" : nullptr;
    if (stats) die("flag %s cannot be combined with --binning: the reads are binned over references a profile of an earlier run lists (--binning-refs)", stats);
    const char* clash = o.out_file_given ? "-o/--out-file" : !o.specific_level.empty() ? "--specific-level" : !o.regions_bed.empty() ? "--regions-bed"
                        : !o.also_dbs.empty() ? "--also-db" : o.whole_file ? "-g/--query-whole-file" : nullptr;
    if (clash) die("flag %s cannot be combined with --binning: no search result is written, the reads are only binned", clash);
    const char* bad = o.keep_unmatched ? "-K/--keep-unmatched" : o.try_se ? "--try-se" : o.top_scores != 0 ? "-n/--keep-top-scores"
                      : sliding ? "--sliding-step/--sliding-window/--sliding-greedy" : o.gpus_given ? "--gpus/--gpu-ids" : o.gpu_passes >= 0 ? "--gpu-passes" : nullptr;
    if (bad) die("flag %s cannot be combined with --binning", bad);
    if (o.binning_refs.empty()) die("flag --binning needs --binning-refs: the list of the references to bin over (a profile of kmcp-refstats --profile or --ref-stats-profile as it is)");
    if (o.taxid_maps.empty() || o.taxdump.empty()) die("TaxID mapping files (--taxid-map) and taxonomy dump files (--taxdump) are needed for --binning");
  }
  if (!o.specific_level.empty()) {
    const bool species = o.specific_level == "species";
    if (!species && o.specific_level != "strain" && o.specific_level != "assembly")
      die("invalid value for --specific-level, available values: species, strain/assembly");
    const char* bad = o.keep_unmatched ? "-K/--keep-unmatched" : o.try_se ? "--try-se" : o.top_scores != 0 ? "-n/--keep-top-scores"
                      : sliding && o.regions_bed.empty() ? "--sliding-step/--sliding-window/--sliding-greedy"  // (with --regions-bed: the windows' summaries, below)
                      : o.gpus_given ? "--gpus/--gpu-ids" : o.gpu_passes >= 0 ? "--gpu-passes" : nullptr;
    if (bad) die("flag %s cannot be combined with --specific-level", bad);
    if (!o.taxid_maps.empty() && o.taxdump.empty()) die("flag --taxdump is needed when --taxid-map given");
    if (o.taxid_maps.empty() && !o.taxdump.empty()) die("flag --taxid-map is needed when --taxdump given");
    if ((o.taxid_maps.empty() || o.taxdump.empty()) && species) die("TaxID mapping files (--taxid-map) and taxonomy dump files (--taxdump) are needed for --specific-level species");
  }
  // --ref-stats: the same refusals as --specific-level, for the same reason (what is counted must be every query's final matches, counted
  // once); mode 0 cuts rows of a query, which only the TSV route can do
  if (o.ref_stats_profile.empty() && o.profile_flag) die("flag %s is only used with --ref-stats-profile", o.profile_flag);
  if (!o.ref_stats_profile.empty() && o.ref_stats_recount.empty())
    die("flag --ref-stats-profile is only used with --ref-stats-recount (stage 4 starts from the references stage 3 lists and from the reads it kept)");
  if (o.ref_stats_recount.empty() && o.recount_flag) die("flag %s is only used with --ref-stats-recount", o.recount_flag);
  if (!o.ref_stats_recount.empty() && (o.ref_stats.empty() || o.ref_stats_cooccur.empty()))
    die("flag --ref-stats-recount is only used with --ref-stats and --ref-stats-cooccur (stage 3 starts from the tables of stages 1 and 2)");
  if (o.ref_stats.empty() && o.ref_stats_flag) die("flag %s is only used with --ref-stats", o.ref_stats_flag);
  if (o.ref_stats.empty() && o.ref_stats_only) die("flag --ref-stats-only is only used with --ref-stats");
  if (!o.ref_stats.empty()) {
    const char* bad = o.keep_unmatched ? "-K/--keep-unmatched" : o.try_se ? "--try-se" : o.top_scores != 0 ? "-n/--keep-top-scores"
                      : sliding ? "--sliding-step/--sliding-window/--sliding-greedy" : o.gpus_given ? "--gpus/--gpu-ids" : o.gpu_passes >= 0 ? "--gpu-passes" : nullptr;
    if (bad) die("flag %s cannot be combined with --ref-stats", bad);
    if (o.ref_stats_only) {  // no search result: nothing that writes one, filters one, or merges several
      const char* clash = o.out_file_given ? "-o/--out-file" : !o.specific_level.empty() ? "--specific-level" : !o.regions_bed.empty() ? "--regions-bed"
                          : !o.also_dbs.empty() ? "--also-db" : o.whole_file ? "-g/--query-whole-file" : nullptr;
      if (clash) die("flag %s cannot be combined with --ref-stats-only: no search result is written, the reads are only counted", clash);
    }
    if (o.ref_stats_mode < 0 || o.ref_stats_mode >= kmcpg::REFSTATS_MODES) die("invalid profiling mode: %d", o.ref_stats_mode);
    if (o.ref_stats_mode == 0)
      die("flag --ref-stats-mode 0 is not supported: its main-match cut (--keep-main-matches) drops rows of a query before they are counted; run kmcp-refstats -m 0 on the search result");
    if (o.ref_stats_p < 0 || o.ref_stats_p > 1) die("the value of --ref-stats-min-chunks-fraction (%f) should be in range of [0, 1]", o.ref_stats_p);
    if (!(o.ref_stats_h > 0) || o.ref_stats_h > 1) die("the value of --ref-stats-min-hic-ureads-qcov (%f) should be in range of (0, 1]", o.ref_stats_h);
    const bool both = !o.taxid_maps.empty() && !o.taxdump.empty();
    const std::string& lv = o.ref_stats_level;
    if (!lv.empty() && lv != "species" && lv != "strain" && lv != "assembly") die("invalid value for --ref-stats-level, available values: species, strain/assembly");
    if (!o.taxid_maps.empty() && o.taxdump.empty()) die("flag --taxdump is needed when --taxid-map given");
    if (o.taxid_maps.empty() && !o.taxdump.empty()) die("flag --taxid-map is needed when --taxdump given");
    if (lv == "species" && !both) die("TaxID mapping files (--taxid-map) and taxonomy dump files (--taxdump) are needed for --ref-stats-level species");
    if (o.ref_stats == o.out_file) die("flag --ref-stats: the statistics file must not be the search result's file");
    if (o.ref_stats_cooccur.empty() && o.ref_stats_cooccur_slots != 0) die("flag --ref-stats-cooccur-slots is only used with --ref-stats-cooccur");
    if (!o.ref_stats_cooccur.empty()) {
      if (o.ref_stats_cooccur == o.out_file) die("flag --ref-stats-cooccur: the pairs' file must not be the search result's file");
      if (o.ref_stats_cooccur == o.ref_stats) die("flag --ref-stats-cooccur: the pairs' file must not be the statistics file (--ref-stats)");
      const long long n = o.ref_stats_cooccur_slots;
      if (n < 0 || (n & (n - 1)) || n > (1ll << 30)) die("the value of --ref-stats-cooccur-slots (%lld) should be a power of two, at most 2^30", n);
    }
    if (!o.ref_stats_recount.empty()) {
      if (o.ref_stats_recount == o.out_file) die("flag --ref-stats-recount: the file must not be the search result's file");
      if (o.ref_stats_recount == o.ref_stats) die("flag --ref-stats-recount: the file must not be the statistics file (--ref-stats)");
      if (o.ref_stats_recount == o.ref_stats_cooccur) die("flag --ref-stats-recount: the file must not be the pairs' file (--ref-stats-cooccur)");
      if (o.ref_stats_recount_log_mb == 0 || o.ref_stats_recount_log_mb > 4096) die("the value of --ref-stats-recount-log-mb (%lld) should be in range of [1, 4096]", o.ref_stats_recount_log_mb);
      if (!(o.ref_stats_d > 0) || o.ref_stats_d > 1) die("the value of --ref-stats-min-dreads-prop (%f) should be in range of (0, 1]", o.ref_stats_d);
      if (!(o.ref_stats_r > 0) || !(o.ref_stats_r < 1)) die("the value of --ref-stats-max-mismatch-err (%f) should be in range of (0, 1)", o.ref_stats_r);
    }
    if (!o.ref_stats_profile.empty()) {
      if (o.ref_stats_profile == o.out_file) die("flag --ref-stats-profile: the file must not be the search result's file");
      if (o.ref_stats_profile == o.ref_stats) die("flag --ref-stats-profile: the file must not be the statistics file (--ref-stats)");
      if (o.ref_stats_profile == o.ref_stats_cooccur) die("flag --ref-stats-profile: the file must not be the pairs' file (--ref-stats-cooccur)");
      if (o.ref_stats_profile == o.ref_stats_recount) die("flag --ref-stats-profile: the file must not be the recount's file (--ref-stats-recount)");
      if (o.ref_stats_iters <= 0 || o.ref_stats_iters > 1000000) die("the value of --ref-stats-abund-max-iters (%lld) should be in range of [1, 1000000]", o.ref_stats_iters);
      if (!(o.ref_stats_pct > 0)) die("the value of --ref-stats-abund-pct-threshold (%f) should be greater than 0", o.ref_stats_pct);
      if (!(o.ref_stats_filter >= 0) || !(o.ref_stats_filter < 100)) die("the value of --ref-stats-filter-low-pct (%f) should be in range of [0, 100)", o.ref_stats_filter);
    }
  }
  // sliding windows: seqkit sliding has no meaning for pairs, whole files as queries or one ID for everything
  if (sliding) {
    if (!o.sliding_step_given || !o.sliding_window_given) die("flags --sliding-step and --sliding-window are needed together");
    if (o.sliding_step < 1 || o.sliding_window < 1) die("values of flags --sliding-step and --sliding-window should be positive");
    if (!o.read1.empty() && !o.read2.empty()) die("flags --sliding-step/--sliding-window are not supported for paired-end input (-1/-2)");
    if (o.whole_file || o.use_filename) die("flags --sliding-step/--sliding-window cannot be combined with -g/--query-whole-file or -G/--use-filename");
    if (!o.query_id.empty()) die("flags --sliding-step/--sliding-window cannot be combined with --query-id");
  }
  // --also-db: whatever acts per database in separate runs and would act per query on the union is refused here, before a file is
  // opened or a GPU touched (the library refuses the same through its parameters)
  if (!o.also_dbs.empty()) {
    const char* clash = o.keep_unmatched ? "-K/--keep-unmatched" : o.try_se ? "--try-se" : o.do_not_sort ? "-S/--do-not-sort" : o.top_scores != 0 ? "-n/--keep-top-scores"
                      : o.whole_file ? "-g/--query-whole-file" : o.use_filename ? "-G/--use-filename" : sliding ? "--sliding-step/--sliding-window/--sliding-greedy"
                      : o.gpus_given ? "--gpus/--gpu-ids" : o.gpu_passes >= 0 ? "--gpu-passes" : nullptr;
    if (clash)
      die("flag %s cannot be combined with --also-db: in separate searches it acts per database, on databases searched together it would act per query; "
          "search the databases one by one and merge the results with kmcp-merge", clash);
    if (o.also_dbs.size() > 15) die("flag --also-db: at most 15 further databases (%zu given)", o.also_dbs.size());
  }
  if (o.db_dir.empty()) die("flag -d/--db-dir needed");
  if (o.min_kmers < 1) die("value of flag --min-kmers should be positive: %d", o.min_kmers);
  if (o.dedup < 1) die("value of flag --kmer-dedup-threshold should be positive: %d", o.dedup);
  if (!(o.max_fpr > 0)) die("value of flag --max-fpr should be positive: %f", o.max_fpr);
  if (o.min_qlen < 0 || o.top_scores < 0) die("value of flag --min-query-len/--keep-top-scores should not be negative");
  if (o.do_not_sort && o.top_scores > 0) warn("flag -n/--keep-top-scores ignored when -S/--do-not-sort given");
  int sort_by = 0;
  if (o.sort_by == "qcov") sort_by = 0;
  else if (o.sort_by == "tcov") sort_by = 1;
  else if (o.sort_by == "jacc") sort_by = 2;
  else die("invalid value for flag -s/--sort-by: %s. Available: qcov/tsov/jacc", o.sort_by.c_str());
  if (o.min_qcov < 0 || o.min_qcov > 1) die("value of -t/--min-query-cov should be in range [0, 1]");
  if (o.min_tcov < 0 || o.min_tcov > 1) die("value of -T/-target-cov should be in range [0, 1]");
  // --regions-bed: the windows of --sliding-* judged by --specific-level, merged into regions; no search result is written
  if (o.regions_bed.empty() && o.regions_flag) die("flag %s is only used with --regions-bed", o.regions_flag);
  if (!o.regions_bed.empty()) {
    if (o.specific_level.empty()) die("flag --regions-bed needs --specific-level: regions are merged from species- or assembly-specific windows");
    if (!sliding) die("flag --regions-bed needs --sliding-step and --sliding-window: regions are merged from the windows of the input");
    if (o.out_file_given) die("flag -o/--out-file cannot be combined with --regions-bed: no search result is written, the regions go to the BED file");
    if (o.regions_min_overlap < 1) die("value of flag --regions-min-overlap should be positive");
    if (o.regions_max_gap < 0) die("value of flag --regions-max-gap should not be negative");
  }
  if (!o.quiet) {
    info("kmcp-search v%s (MI355X build of the kmcp search hot path)", VERSION);
    info("  https://github.com/shenwei356/kmcp");
    info("");
    info("checking input files ...");
  }
  return sort_by;
}

// input files (search.go:219-290): the single-end files to read, or none and *paired set for -1/-2
static std::vector<std::string> resolve_inputs(Options& o, bool* paired) {
  const bool verbose = !o.quiet;
  std::vector<std::string> files;
  *paired = false;
  if (o.read1.empty()) {
    if (!o.read2.empty()) { warn("only flag -2/--read2 given, it's treated as single-end"); files.push_back(o.read2); }
  } else if (o.read2.empty()) {
    warn("only flag -1/--read1 given, it's treated as single-end");
    files.push_back(o.read1);
  } else {
    *paired = true;
    if (verbose) { info("paired end files given: %s, %s", o.read1.c_str(), o.read2.c_str()); info("other input files via positional arguments are ignored"); }
  }
  if (o.try_se && !*paired) { warn("flag --try-se ignored for single-end input(s)"); o.try_se = false; }
  if (*paired) return files;
  std::vector<std::string> f1 = o.files;
  if (!o.infile_list.empty()) {
    gzFile g = gzopen(o.infile_list.c_str(), "rb");
    if (!g) die("%s: %s", o.infile_list.c_str(), strerror(errno));
    char buf[1 << 14];
    while (gzgets(g, buf, sizeof buf)) {
      size_t n = strlen(buf);
      while (n && (buf[n - 1] == '\n' || buf[n - 1] == '\r')) buf[--n] = 0;
      if (n) f1.push_back(buf);
    }
    gzclose(g);
  }
  if (f1.empty() && files.empty()) f1.push_back("-");
  for (const auto& f : f1) {
    if ((!o.read1.empty() || !o.read2.empty()) && f == "-") continue;
    files.push_back(f);
  }
  for (const auto& f : files) {
    struct stat st;
    if (f != "-" && stat(f.c_str(), &st) != 0) die("%s: %s", f.c_str(), strerror(errno));
    if (f != "-" && f == o.out_file) die("out file should not be one of the input file");
  }
  if (verbose) {
    if (files.size() == 1 && files[0] == "-") info("  no files given, reading from stdin");
    else info("  %zu input file(s) given", files.size());
  }
  return files;
}

// one database: the sub-directory of `root` holding __db.yml (search.go:299-324)
static std::string resolve_db(const std::string& root, bool verbose) {
  if (verbose) info("checking the database: %s", root.c_str());
  std::vector<std::string> found;
  DIR* d = opendir(root.c_str());
  if (!d) die("read database error: open %s: %s", root.c_str(), strerror(errno));
  std::vector<std::string> subs;
  while (struct dirent* e = readdir(d)) {
    std::string n = e->d_name;
    if (n == "." || n == "..") continue;
    subs.push_back(n);
  }
  closedir(d);
  std::sort(subs.begin(), subs.end());
  for (const auto& n : subs) {
    struct stat st;
    std::string p = root + "/" + n;
    if (stat(p.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) continue;
    if (stat((p + "/__db.yml").c_str(), &st) == 0) found.push_back(p);
  }
  if (found.empty()) die("invalid kmcp database: %s", root.c_str());
  if (found.size() > 1) die("databases with several repeats (R001, R002, ...) are not supported: `kmcp index` only writes R001");
  return found[0];
}

// the R001 directory of -d, then of every --also-db
static std::vector<std::string> resolve_databases(const Options& o) {
  std::vector<std::string> db_dirs{resolve_db(o.db_dir, !o.quiet)};
  for (const auto& a : o.also_dbs) db_dirs.push_back(resolve_db(a, !o.quiet));
  return db_dirs;
}

struct NameMaps {
  std::unordered_map<std::string, std::string> given;                  // -N: all files in one map
  std::vector<std::unordered_map<std::string, std::string>> defaults;  // -D: every database's own mapping, for its own columns
};

static NameMaps load_name_maps(const Options& o, const std::vector<std::string>& db_dirs) {
  const bool verbose = !o.quiet;
  NameMaps nm;
  if (!o.name_maps.empty()) {
    if (verbose) info("loading name mapping file ...");
    for (const auto& f : o.name_maps)
      for (auto& kv : read_kvs(f)) nm.given[kv.first] = kv.second;
    if (verbose) info("  %zu pairs of name mapping values from %zu file(s) loaded", nm.given.size(), o.name_maps.size());
  }
  nm.defaults.resize(db_dirs.size());
  if (o.default_name_map)
    for (size_t m = 0; m < db_dirs.size(); m++) {
      struct stat st;
      std::string f = db_dirs[m] + "/__name_mapping.tsv";
      if (stat(f.c_str(), &st) == 0) nm.defaults[m] = read_kvs(f);
    }
  return nm;
}

// ---- the pipeline's shared state: reader -> q_in -> searchers -> q_out -> writer (main thread)
// The reader starts before the database is open and cuts its first batches by the default limits.  What only the open database tells —
// its k, the batch limits that fit beside the resident index — is published here, once, by main; a thread that cannot go on without it waits.
class OpenGate {
 public:
  std::atomic<size_t> max_bases{(size_t)64 << 20}, batch_reads;  // a batch closes at this many bases / queries: the defaults until open()
  std::atomic<int> k{0};  // the database's k (-g may have it before open(): read_k_early)
  explicit OpenGate(size_t reads) : batch_reads(reads) {}
  void wait() {
    std::unique_lock<std::mutex> l(mu_);
    cv_.wait(l, [&] { return ready_.load(); });
  }
  void open(size_t bases, size_t reads, int db_k) {
    max_bases.store(bases);
    batch_reads.store(reads);
    k.store(db_k);
    ready_.store(true);
    { std::lock_guard<std::mutex> g(mu_); }
    cv_.notify_all();
  }

 private:
  std::atomic<bool> ready_{false};
  std::mutex mu_;
  std::condition_variable cv_;
};

struct Pipeline {
  Pipeline(const Options& opts, bool paired_, bool sliding_, const kmcpg_window_spec& w)
      : o(opts), paired(paired_), sliding(sliding_), wspec(w), gate((size_t)opts.batch) {}

  // ---- constant context: nothing below is written while a thread that reads it runs
  const Options& o;  // (main goes on writing o.batch and o.gpu_ids while it opens the database: no thread reads those two)
  const bool paired, sliding;
  bool regions() const { return !o.regions_bed.empty(); }
  bool stats_only() const { return o.ref_stats_only; }
  bool bins_only() const { return !o.binning.empty(); }
  const kmcpg_window_spec wspec;
  // set by main after the database open and before the searchers start; the reader never looks at them
  kmcpg_db* db = nullptr;
  int32_t paged_passes = 0;  // > 1: a paged index, searched in this many passes per batch
  kmcpg_params params{};
  std::vector<std::string> target;  // target names after mapping, by column
  kmcpg::BinPlan bin_plan;          // --binning: the pruned tree of the listed references ...
  std::vector<uint32_t> bin_node;   // ... and the node of every column (kmcpg::BIN_NO_NODE: not listed)

  // ---- the queues and the gate
  Queue<std::unique_ptr<Batch>> q_in{24};  // reader -> searchers
  Queue<std::unique_ptr<Batch>> q_out{3};  // searchers -> writer, which puts the batches back in order; closed by the last searcher to leave
  OpenGate gate;

  // ---- counters and timers (seconds) of the run, for the summary lines
  Clock::time_point t_start, t_search;  // main: the process start / right before the gate opens, where the speed lines count from
  // the reader thread writes these two (blocked: while it runs; total: as it ends); main reads them after reader.join()
  double t_reader_blocked = 0, t_reader_total = 0;  // waiting for a free slot of q_in / its whole life
  // every searcher adds its own sums under t_mu as it ends; main reads them after the searchers are joined
  std::mutex t_mu;
  double t_gpu = 0, t_read_wait = 0;        // inside libkmcpgpu / waiting for input
  uint64_t sum_matches = 0, sum_check = 0;  // matches of the run and their order-independent checksum
  std::atomic<int> live{0};                 // searchers still running
  // the writer loop alone (the main thread), read by print_summary and the trailer after it
  uint64_t total = 0, matched = 0;
  kmcpg_result_stats stats{};  // --ref-stats-only: the tickets' sums
  kmcpg_result_bins bins{};    // --binning: the tickets' sums
  int fmt_threads = 0;
  double t_fmt = 0;                                       // formatting + writing, all of an iteration
  double t_fmt_busy = 0;                                  // summed over the formatter threads: time inside the parts
  double t_fmt_pool = 0, t_fmt_push = 0, t_fmt_wait = 0;  // rows being formatted / waiting for the flusher / waiting for a searched batch
};

// --binning: the listed references (--binning-refs: the first tab-separated column of every line that does not start with '#', so that a
// profile can be passed as it is) and the plan over their TaxIds (kmcp_amd/csrc/bin_rule.hpp).  `target`: the database's printed target
// names by column, from a metadata-only handle — a listed name the database does not have and a listed reference without a TaxId are
// refused here, before the GPU is touched or a file is written
static void plan_binning(const Options& o, Pipeline& p, const std::vector<std::string>& target, const kmcpg::Taxonomy& tax, const kmcpg::TaxidMap& map) {
  std::vector<std::string> refs;
  {
    gzFile f = gzopen(o.binning_refs.c_str(), "rb");  // (reads plain files as they are)
    if (!f) die("%s: %s", o.binning_refs.c_str(), strerror(errno));
    std::string text;
    char buf[1 << 16];
    int n;
    while ((n = gzread(f, buf, sizeof buf)) > 0) text.append(buf, (size_t)n);
    if (n < 0) die("%s: read error", o.binning_refs.c_str());
    gzclose(f);
    std::set<std::string> seen;
    for (size_t at = 0; at < text.size();) {
      size_t end = text.find('\n', at);
      if (end == std::string::npos) end = text.size();
      std::string line = text.substr(at, end - at);
      at = end + 1;
      if (!line.empty() && line.back() == '\r') line.pop_back();
      if (line.empty() || line[0] == '#') continue;
      line.resize(std::min(line.size(), line.find('\t')));
      if (seen.insert(line).second) refs.push_back(line);
    }
  }
  std::sort(refs.begin(), refs.end());  // (the refusals name the first in byte order)
  const std::set<std::string> have(target.begin(), target.end());
  for (const std::string& r : refs)
    if (!have.count(r)) die("flag --binning-refs: the database has no reference %s", r.c_str());
  std::string missing;
  if (!kmcpg::bin_plan_build(tax, map, refs, &p.bin_plan, &missing)) die("unknown taxid for %s, please check taxid mapping file(s)", missing.c_str());
  if (p.bin_plan.unknown_taxids)
    warn("%llu TaxId(s) of the listed references are deleted or not in nodes.dmp: a read that matches one of them and any other reference is binned at 0", (unsigned long long)p.bin_plan.unknown_taxids);
  if (!o.quiet) info("  binning over %zu references, %zu nodes of the taxonomy", refs.size(), p.bin_plan.parent.size());
}
// ... and the library's stage, once the database is open
static void set_binning(Pipeline& p) {
  p.bin_node.resize(p.target.size());
  for (size_t c = 0; c < p.target.size(); c++) p.bin_node[c] = p.bin_plan.node_of(p.target[c]);
  if (kmcpg_set_binning(p.db, p.bin_node.data(), (uint32_t)p.bin_node.size(), p.bin_plan.parent.data(), p.bin_plan.last.data(), p.bin_plan.taxid.data(),
                        (uint32_t)p.bin_plan.parent.size()) != 0)
    die("%s", kmcpg_last_error());
}

// ---- reader thread

// -g, one query per file (search.go:885-935): the records of the file back to back, records 2..m each followed by k - 1 N's
// (search.go:899-914) — packed to 2-bit codes as they are read (the file's bases are touched once, the batch is a quarter of the text and the
// library takes it as it is).  The files are parsed by several threads, a file each (a 4-Mbp assembly is ~4 ms of line joining and packing:
// one reader thread fed 250 genomes/s to a GPU that searches 40 000), and handed to the reader in the order of the command line.
struct FileQuery {
  Batch q;  // the file's one query, packed from base 0
  std::string qid;
  bool empty = true;
};

class WholeFileParsers {
 public:
  WholeFileParsers(const Options& o, const std::vector<std::string>& files, const std::string& gap) : o_(o), files_(files), gap_(gap), slots_(files.size()) {
    const size_t n_workers = std::max<size_t>(1, std::min<size_t>({(size_t)8, (size_t)usable_cpus() / 2, files.size()}));
    ahead_ = 4 * n_workers;
    for (size_t wi = 0; wi < n_workers; wi++) workers_.emplace_back(&WholeFileParsers::work, this);
  }
  // file fi's query; the reader asks for every file, in order
  std::unique_ptr<FileQuery> take(size_t fi) {
    std::unique_lock<std::mutex> l(m_);
    cv_.wait(l, [&] { return slots_[fi] != nullptr; });
    std::unique_ptr<FileQuery> fq = std::move(slots_[fi]);
    consumed_ = fi + 1;
    cv_.notify_all();
    return fq;
  }
  void join() {
    for (auto& t : workers_) t.join();
  }

 private:
  void work() {
    std::string wid, ws;
    for (;;) {
      const size_t fi = next_file_.fetch_add(1);
      if (fi >= files_.size()) return;
      {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return fi < consumed_ + ahead_; });
      }
      std::unique_ptr<FileQuery> fq(new FileQuery());
      fq->q.packed = true;
      FastxReader r(files_[fi]);
      while (r.next(&wid, &ws)) {
        if (fq->empty) {
          fq->qid = o_.use_filename ? trim_ext(files_[fi]) : (!o_.query_id.empty() ? o_.query_id : wid);
          fq->empty = false;
          fq->q.pack_append(ws.data(), ws.size());
        } else {
          fq->q.pack_append(ws.data(), ws.size());
          fq->q.pack_append(gap_.data(), gap_.size());
        }
      }
      std::lock_guard<std::mutex> l(m_);
      slots_[fi] = std::move(fq);
      cv_.notify_all();
    }
  }
  const Options& o_;
  const std::vector<std::string>& files_;
  const std::string gap_;
  std::vector<std::unique_ptr<FileQuery>> slots_;
  std::mutex m_;
  std::condition_variable cv_;
  std::atomic<size_t> next_file_{0};
  size_t consumed_ = 0;  // under m_: files the reader has taken (workers stay at most `ahead_` files in front of it)
  size_t ahead_ = 0;
  std::vector<std::thread> workers_;
};

// The reader thread's own state: the batch being filled and how far the input has been numbered.  Every input mode ends a batch through flush().
struct Reader {
  Pipeline& p;
  const std::vector<std::string>& files;
  uint64_t id = 0, seq = 0;  // queries numbered / batches handed on so far
  std::unique_ptr<Batch> b;  // the batch being filled

  void flush() {
    if (b->size() == 0) return;
    b->seq = seq++;
    const auto tp = Clock::now();
    p.q_in.push(std::move(b));
    p.t_reader_blocked += seconds_since(tp);
    b.reset(new Batch());
    b->paired = p.paired;
    b->first_idx = id;
  }
  // a batch that read_single_end / read_paired cut: numbered and handed on as it is
  void take(std::unique_ptr<Batch> nb) {
    nb->first_idx = id;
    id += nb->size();
    b = std::move(nb);
    flush();
  }

  void read_pairs() {
    const Options& o = p.o;
    if (!p.o.quiet) info("reading from paired-end files: %s, %s", o.read1.c_str(), o.read2.c_str());
    flush();
    read_paired(o.read1, o.read2, p.gate.batch_reads.load(), p.gate.max_bases.load(), [&](std::unique_ptr<Batch> nb) { take(std::move(nb)); });
    if (id == 0) warn("no valid sequences in files: %s, %s", o.read1.c_str(), o.read2.c_str());
  }

  void read_whole_files() {
    // the gap between records is k - 1 N's: the database's k is needed first
    if (p.gate.k.load() <= 0) p.gate.wait();  // (normally known already: read from the headers before the GPU was touched, read_k_early)
    const std::string nnn((size_t)std::max(0, p.gate.k.load() - 1), 'N');
    WholeFileParsers parsers(p.o, files, nnn);
    for (size_t fi = 0; fi < files.size(); fi++) {
      if (!p.o.quiet) info("reading sequence file: %s", files[fi].c_str());
      std::unique_ptr<FileQuery> fq = parsers.take(fi);
      if (fq->empty) { warn("no valid sequences in file: %s", files[fi].c_str()); continue; }
      b->packed = true;
      b->append_packed(fq->q.codes.data(), fq->q.n_bases, fq->q.exc.data(), fq->q.n_exc);
      b->id_buf.insert(b->id_buf.end(), fq->qid.begin(), fq->qid.end());
      b->id_offs.push_back(b->id_buf.size());
      b->offs.push_back(b->n_bases);
      id++;
      if (b->size() >= p.gate.batch_reads.load() || b->bases() >= p.gate.max_bases.load()) flush();
    }
    parsers.join();
  }

  // records as they are (one upload of their bases); the library cuts the windows.  A batch closes at `batch_reads` windows or
  // `max_bases` bases of records; a record with more windows than that is a batch of its own (the library cuts it into pieces).
  void read_sliding() {
    for (const auto& file : files) {
      if (!p.o.quiet) info("reading sequence file: %s", file.c_str());
      FastxReader r(file);
      std::string rid, rs;
      uint64_t got = 0;
      while (r.next(&rid, &rs)) {
        got++;
        const uint64_t L = rs.size(), nw = window_count(L, p.wspec);
        if (nw == 0) continue;  // (seqkit sliding emits nothing for it: no query)
        if (b->size() && (b->wpre.back() + nw > p.gate.batch_reads.load() || b->seqs.size() + L > p.gate.max_bases.load())) flush();
        b->windows = true;
        b->id_buf.insert(b->id_buf.end(), rid.begin(), rid.end());
        b->id_offs.push_back(b->id_buf.size());
        b->seqs.insert(b->seqs.end(), (const uint8_t*)rs.data(), (const uint8_t*)rs.data() + L);
        b->offs.push_back(b->seqs.size());
        b->wpre.push_back(b->wpre.back() + nw);
        id += nw;
      }
      if (got == 0) warn("no valid sequences in file: %s", file.c_str());
    }
  }

  void read_plain() {
    for (const auto& file : files) {
      if (!p.o.quiet) info("reading sequence file: %s", file.c_str());
      flush();  // batches do not span input files on this path
      const uint64_t got = read_single_end(file, p.gate.batch_reads.load(), p.gate.max_bases.load(), [&](std::unique_ptr<Batch> nb) { take(std::move(nb)); });
      if (got == 0) warn("no valid sequences in file: %s", file.c_str());
    }
  }

  void run() {
    if (p.o.gpu_passes >= 0) p.gate.wait();
    const auto tr0 = Clock::now();
    b.reset(new Batch());
    b->paired = p.paired;
    if (p.paired) read_pairs();
    else if (p.o.whole_file) read_whole_files();
    else if (p.sliding) read_sliding();
    else read_plain();
    flush();
    p.q_in.close();
    p.t_reader_total = seconds_since(tr0);
  }
};

// -g needs the database's k before the first file can be joined (k - 1 N's between records): a metadata-only handle reads it from
// __db.yml and the block headers in a millisecond, without the GPU runtime, so that the files are parsed while the index is loaded
static void read_k_early(Pipeline& p, const std::string& db_dir) {
  kmcpg_db* meta = nullptr;
  kmcpg_opts mo{-1, 0, 1, 0};
  if (kmcpg_open(db_dir.c_str(), &mo, &meta) != 0) return;
  kmcpg_info mi;
  if (kmcpg_db_info(meta, &mi) == 0) p.gate.k.store(mi.k);
  kmcpg_close(meta);
}

// ---- the database: open, notes to the user, target names, batch limits
// One of three ways to open (several databases as a set / one database over several GPUs / one database on one GPU, paged if it has to be);
// *paged_passes > 1 says the last.  Fills o.gpu_ids from --gpus and, for a paged index, raises o.batch.
static kmcpg_db* open_database(Options& o, const std::vector<std::string>& db_dirs, int32_t* paged_passes) {
  const bool verbose = !o.quiet;
  if (verbose) info("loading database into GPU memory ...");
  kmcpg_db* db = nullptr;
  *paged_passes = 0;
  if (o.gpu_ids.empty() && o.gpus > 1)
    for (int i = 0; i < o.gpus; i++) o.gpu_ids.push_back(i);
  if (db_dirs.size() > 1) {  // --also-db: one handle over all the databases (kmcp_gpu.h kmcpg_open_set)
    std::vector<const char*> dirs;
    for (const auto& d : db_dirs) dirs.push_back(d.c_str());
    kmcpg_opts gopts{o.device, 0, 1, 0};
    if (kmcpg_open_set(dirs.data(), (uint32_t)dirs.size(), &gopts, &db) != 0) die("open kmcp dbs: %s", kmcpg_last_error());
    if (verbose) info("  %zu databases searched together, results merged as kmcp-merge would", db_dirs.size());
  } else if (!o.gpu_ids.empty()) {  // one process, several GPUs: blocks partitioned over the devices, hits merged on the host
    if (kmcpg_open_devices(db_dirs[0].c_str(), o.gpu_ids.data(), (int32_t)o.gpu_ids.size(), &db) != 0)
      die("open kmcp db: %s: %s", db_dirs[0].c_str(), kmcpg_last_error());
    if (verbose) info("  %zu GPUs, exchange of the hit lists: %s", o.gpu_ids.size(), kmcpg_exchange_info(db));
  } else {
    kmcpg_opts gopts{o.device, 0, 1, 0};
    int rc = o.gpu_passes >= 0 ? KMCPG_ENOMEM : kmcpg_open(db_dirs[0].c_str(), &gopts, &db);
    if (rc == KMCPG_ENOMEM) {
      // the index is larger than the GPU's memory (or --gpu-passes asks for it): one part of it resident at a time, every batch
      // searched against all parts in turn (the reference's counterpart: mmap / --low-mem, search.go:80)
      if (o.gpu_passes < 0) warn("%s", kmcpg_last_error());
      if (kmcpg_open_paged(db_dirs[0].c_str(), o.device, std::max(0, o.gpu_passes), &db) != 0) die("open kmcp db: %s: %s", db_dirs[0].c_str(), kmcpg_last_error());
      int32_t passes = 0;
      kmcpg_paged_info(db, &passes, nullptr);
      *paged_passes = passes;
      if (passes > 1) {
        if (!o.batch_given) o.batch = 4 << 20;  // a batch costs passes - 1 uploads of index parts: large batches keep their share small
        warn("the index is searched in %d passes per batch of %d queries (one part resident in GPU memory at a time); more GPUs (--gpus) avoid this", passes, o.batch);
      }
    } else if (rc != 0) die("open kmcp db: %s: %s", db_dirs[0].c_str(), kmcpg_last_error());
  }
  return db;
}

// Narrow blocks (rows of up to 64 bytes: what `kmcp index -j 32` makes of a small database) cost one memory request per (k-mer,
// block) whatever their width; blocks that share NumSigs are laid side by side in GPU memory and served by ONE request.  Blocks
// with a NumSigs of their own cannot be: say so once, with the remedy (profiles/r04_narrow_rows.txt: ~3x).
static void warn_narrow_blocks(kmcpg_db* db, const kmcpg_info& dbi) {
  std::set<uint64_t> sigs;
  int narrow = 0;
  for (int32_t b = 0; b < dbi.n_blocks; b++) {
    uint64_t ns = 0;
    uint32_t nc = 0, rb = 0, st = 0, cb = 0;
    int32_t loc = 0;
    if (kmcpg_block_info(db, (uint32_t)b, &ns, &nc, &rb, &st, &loc, &cb) == 0 && rb <= 64) {
      narrow++;
      sigs.insert(ns);
    }
  }
  if (narrow > 1 && sigs.size() > 1)
    info("  note: %zu distinct NumSigs over %d narrow blocks (rows <= 64 bytes): every k-mer costs %zu gathers; a database built with fewer, wider "
         "blocks (`kmcp index -b`) or with equal NumSigs (kmcpg_build_db uniform_sigs = 1) is searched ~3x faster",
         sigs.size(), narrow, sigs.size());
}

// target names after mapping (util-db-search.go:317-332), resolved once per column
static std::vector<std::string> resolve_targets(const Options& o, kmcpg_db* db, const kmcpg_info& dbi, const NameMaps& nm) {
  std::vector<std::string> target(dbi.n_cols);
  uint32_t member_base[16] = {0}, n_members = 0;
  if (kmcpg_set_info(db, &n_members, member_base, 16) != 0) die("%s", kmcpg_last_error());
  for (uint32_t c = 0, member = 0; c < dbi.n_cols; c++) {
    while (member + 1 < n_members && member + 1 < 16 && c >= member_base[member + 1]) member++;
    const auto& default_map = nm.defaults[std::min<size_t>(member, nm.defaults.size() - 1)];
    const char* name = nullptr;
    kmcpg_col_info(db, c, &name, nullptr, nullptr, nullptr);
    target[c] = name;
    if (!o.name_maps.empty() || o.default_name_map) {
      auto it = nm.given.find(target[c]);
      if (it != nm.given.end()) target[c] = it->second;
      else if (o.default_name_map) {
        auto it2 = default_map.find(target[c]);
        if (it2 != default_map.end()) target[c] = it2->second;
      }
    }
  }
  return target;
}

// --specific-level: the TaxId maps and the taxdump (filter.go:158-205)
static void load_taxonomy(const Options& o, std::unique_ptr<kmcpg::Taxonomy>& tax, std::unique_ptr<kmcpg::TaxidMap>& map) {
  std::string err;
  map.reset(new kmcpg::TaxidMap());
  for (const auto& f : o.taxid_maps)
    if (!map->load(f, &err)) die("%s", err.c_str());
  if (map->ids.empty()) die("no valid TaxIds found in TaxId mapping file");
  tax.reset(new kmcpg::Taxonomy());
  if (!tax->load(o.taxdump, &err)) die("%s", err.c_str());
  if (!o.quiet) info("  %zu pairs of TaxId mapping values from %zu file(s) loaded, %zu taxonomy nodes", map->ids.size(), o.taxid_maps.size(), tax->nodes.size());
}

// ... and the two integers per column the library judges with (kmcp_amd/csrc/specific_rule.hpp), from the PRINTED target of every
// column — after -N / -D, as kmcp-filter sees it in the TSV.  At level species every column's target needs a TaxId: the reference dies
// when such a target is matched, this command before anything is searched.
static void set_specific(const Options& o, kmcpg_db* db, const std::vector<std::string>& target, const kmcpg::Taxonomy* tax, const kmcpg::TaxidMap* map) {
  const bool species = o.specific_level == "species";
  std::vector<uint32_t> cls, sp;
  uint64_t unknown = 0;
  std::string missing;
  if (!kmcpg::specific_classes(target, species ? map : nullptr, species ? tax : nullptr, &cls, species ? &sp : nullptr, &unknown, &missing))
    die("unknown taxid for %s, please check taxid mapping file(s)", missing.c_str());
  if (unknown) warn("%llu TaxId(s) of the database's targets are deleted or not in nodes.dmp: they belong to no species", (unsigned long long)unknown);
  if (kmcpg_set_specific(db, cls.data(), species ? sp.data() : nullptr, (uint32_t)cls.size()) != 0) die("%s", kmcpg_last_error());
}

// --ref-stats: the level (species by default where there is a taxonomy), the preset, and the library's stage with tables of its own
static bool ref_stats_species(const Options& o) { return o.ref_stats_level.empty() ? !o.taxid_maps.empty() && !o.taxdump.empty() : o.ref_stats_level == "species"; }
static void set_ref_stats(const Options& o, kmcpg_db* db, const std::vector<std::string>& target, const kmcpg::Taxonomy* tax, const kmcpg::TaxidMap* map) {
  const bool species = ref_stats_species(o);
  std::vector<uint32_t> cls, sp;
  uint64_t unknown = 0;
  std::string missing;
  if (!kmcpg::specific_classes(target, species ? map : nullptr, species ? tax : nullptr, &cls, species ? &sp : nullptr, &unknown, &missing))
    die("unknown taxid for %s, please check taxid mapping file(s)", missing.c_str());
  if (unknown && o.specific_level.empty()) warn("%llu TaxId(s) of the database's targets are deleted or not in nodes.dmp: they belong to no species", (unsigned long long)unknown);
  const double H = o.ref_stats_h_given ? o.ref_stats_h : kmcpg::refstats_mode(o.ref_stats_mode).hic_min_qcov;
  if (kmcpg_set_refstats(db, cls.data(), species ? sp.data() : nullptr, (uint32_t)cls.size(), H) != 0) die("%s", kmcpg_last_error());
}

// ... and the file, once every batch has been waited for: kmcp-refstats' format (cli/kmcp_refstats.cpp), the references by name, each from
// the counters of its columns (kmcp_amd/csrc/refstats_rule.hpp); returns the references written
static void write_file(const std::string& path, const std::string& s) {
  if (path.size() > 3 && path.compare(path.size() - 3, 3, ".gz") == 0) {
    gzFile f = gzopen(path.c_str(), "wb");
    if (!f || (!s.empty() && gzwrite(f, s.data(), (unsigned)s.size()) != (int)s.size()) || gzclose(f) != Z_OK) die("%s: write error", path.c_str());
  } else {
    FILE* f = path == "-" ? stdout : fopen(path.c_str(), "wb");
    if (!f || fwrite(s.data(), 1, s.size(), f) != s.size() || (f == stdout ? fflush(f) : fclose(f)) != 0) die("%s: write error", path.c_str());
  }
}
// what stage 1 leaves of a reference for stage 3
struct Stage1Ref {
  uint64_t chunks, tlen, reads, ureads;
  bool ok;
};
// kept: the references with the verdict ok (what stage 2 looks at); stage1: every reference with rows
static uint64_t write_ref_stats(const Options& o, kmcpg_db* db, const std::vector<std::string>& target, uint64_t* reruns, std::set<std::string>* kept,
                                std::map<std::string, Stage1Ref>* stage1) {
  const uint32_t n_cols = (uint32_t)target.size();
  std::vector<kmcpg_col_stats> cols(n_cols);
  kmcpg_refstats_totals tot;
  if (kmcpg_refstats_read(db, cols.data(), n_cols, &tot) != 0) die("%s", kmcpg_last_error());
  *reruns = tot.skipped_launches;
  struct Ref {
    uint64_t chunks = 0, tlen = 0;
    std::vector<uint64_t> w;  // [chunks][4]
  };
  std::map<std::string, Ref> refs;  // ascending byte order of the name
  for (uint32_t c = 0; c < n_cols; c++) {
    if (cols[c].rows == 0) continue;
    uint32_t tidx = 0;
    uint64_t gsize = 0;
    kmcpg_col_info(db, c, nullptr, &tidx, &gsize, nullptr);
    Ref& r = refs[target[c]];
    if (r.w.empty()) {  // chunks and tLen: the reference's first column with rows
      r.chunks = tidx >> 16;
      r.tlen = gsize;
      r.w.assign((size_t)r.chunks * kmcpg::REFSTATS_WORDS, 0);
    }
    const uint64_t chunk = (uint16_t)tidx;
    if (chunk >= r.chunks) die("--ref-stats: chunk %llu of %s is outside its %llu chunks", (unsigned long long)chunk, target[c].c_str(), (unsigned long long)r.chunks);
    const uint64_t v[kmcpg::REFSTATS_WORDS] = {cols[c].rows, cols[c].firsts, cols[c].ureads, cols[c].hic_ureads};
    for (int j = 0; j < kmcpg::REFSTATS_WORDS; j++) r.w[chunk * kmcpg::REFSTATS_WORDS + j] += v[j];
  }
  const double min_frac = o.ref_stats_p_given ? o.ref_stats_p : kmcpg::refstats_mode(o.ref_stats_mode).min_chunks_fraction;
  std::string s;
  char line[256];
  s.append(line, (size_t)snprintf(line, sizeof line, "# matched reads: %llu\n# unique reads: %llu\n", (unsigned long long)tot.matched_reads, (unsigned long long)tot.unique_reads));
  s += "#ref\tchunks\ttLen\treads\tureads\thicUreads\tchunksFrac\tverdict\tchunkReads\tchunkFirsts\tchunkUreads\tchunkHicUreads\n";
  for (const auto& kv : refs) {
    const Ref& r = kv.second;
    const kmcpg::RefstatsRef t = kmcpg::refstats_rollup(r.chunks, min_frac, [&](uint64_t c) { return r.w.data() + c * kmcpg::REFSTATS_WORDS; });
    s += kv.first;
    s.append(line, (size_t)snprintf(line, sizeof line, "\t%llu\t%llu\t%llu\t%llu\t%llu\t%.4f\t%s", (unsigned long long)r.chunks, (unsigned long long)r.tlen,
                                    (unsigned long long)t.reads, (unsigned long long)t.ureads, (unsigned long long)t.hic_ureads, t.chunks_frac,
                                    kmcpg::refstats_verdict_name(t.verdict)));
    if (t.verdict == kmcpg::REFSTATS_OK) kept->insert(kv.first);
    (*stage1)[kv.first] = Stage1Ref{r.chunks, r.tlen, t.reads, t.ureads, t.verdict == kmcpg::REFSTATS_OK};
    for (int j = 0; j < kmcpg::REFSTATS_WORDS; j++)
      for (uint64_t c = 0; c < r.chunks; c++) {
        s.push_back(c ? ',' : '\t');
        s += std::to_string(r.w[c * kmcpg::REFSTATS_WORDS + j]);
      }
    s.push_back('\n');
  }
  write_file(o.ref_stats, s);
  return refs.size();
}

// --ref-stats-cooccur: the library's stage — a class per printed target, whatever the level (a pair is a pair of references) ...
static std::vector<std::string> set_cooccur(const Options& o, kmcpg_db* db, const std::vector<std::string>& target) {
  std::vector<uint32_t> cls;
  uint64_t unknown = 0;
  std::string missing;
  kmcpg::specific_classes(target, nullptr, nullptr, &cls, nullptr, &unknown, &missing);
  std::vector<std::string> name_of;  // by class
  for (size_t c = 0; c < cls.size(); c++) {
    if (cls[c] >= name_of.size()) name_of.resize((size_t)cls[c] + 1);
    name_of[cls[c]] = target[c];
  }
  if (kmcpg_set_cooccur(db, cls.data(), (uint32_t)cls.size(), (uint64_t)o.ref_stats_cooccur_slots) != 0) die("%s", kmcpg_last_error());
  return name_of;
}
// ... and the file, once every batch has been waited for and the verdicts are known: kmcp-refstats --cooccur's format; every pair was
// counted in the one pass, and the pairs of two kept references are written (with -f 1 -t 0 and no cuts that equals the two passes of the
// TSV route: skipping a dropped target's rows only takes the target out of a query's set).  Returns the pairs written
static uint64_t write_cooccur(const Options& o, kmcpg_db* db, const std::vector<std::string>& name_of, const std::set<std::string>& kept, kmcpg_cooccur_totals* tot) {
  uint64_t n = 0;
  if (kmcpg_cooccur_read(db, nullptr, 0, &n, tot) != 0) die("%s", kmcpg_last_error());
  std::vector<kmcpg_cooccur_pair> pairs(n);
  if (kmcpg_cooccur_read(db, pairs.data(), n, &n, tot) != 0) die("%s", kmcpg_last_error());
  std::vector<std::pair<std::pair<const std::string*, const std::string*>, uint64_t>> rows;
  for (const kmcpg_cooccur_pair& pr : pairs) {
    const std::string *a = &name_of[pr.class_a], *b = &name_of[pr.class_b];
    if (!kept.count(*a) || !kept.count(*b)) continue;
    if (*b < *a) std::swap(a, b);
    rows.push_back({{a, b}, pr.reads});
  }
  std::sort(rows.begin(), rows.end(), [](const auto& x, const auto& y) { return *x.first.first != *y.first.first ? *x.first.first < *y.first.first : *x.first.second < *y.first.second; });
  std::string s = "# pairs: " + std::to_string(rows.size()) + "\n#refA\trefB\treads\n";
  for (const auto& r : rows) s += *r.first.first + "\t" + *r.first.second + "\t" + std::to_string(r.second) + "\n";
  write_file(o.ref_stats_cooccur, s);
  return rows.size();
}

// --ref-stats-recount: the library's stage — the classes of --ref-stats-cooccur (a class per printed target) and the species of --ref-stats ...
static std::vector<uint32_t> set_recount(const Options& o, kmcpg_db* db, const std::vector<std::string>& target, const kmcpg::Taxonomy* tax, const kmcpg::TaxidMap* map) {
  const bool species = ref_stats_species(o);
  std::vector<uint32_t> cls, cls2, sp;
  uint64_t unknown = 0;
  std::string missing;
  kmcpg::specific_classes(target, nullptr, nullptr, &cls, nullptr, &unknown, &missing);
  if (species && !kmcpg::specific_classes(target, map, tax, &cls2, &sp, &unknown, &missing)) die("unknown taxid for %s, please check taxid mapping file(s)", missing.c_str());
  const double H = o.ref_stats_h_given ? o.ref_stats_h : kmcpg::refstats_mode(o.ref_stats_mode).hic_min_qcov;
  const uint64_t log_bytes = o.ref_stats_recount_log_mb < 0 ? 0 : (uint64_t)o.ref_stats_recount_log_mb << 20;
  if (kmcpg_set_recount(db, cls.data(), species ? sp.data() : nullptr, (uint32_t)cls.size(), H, log_bytes) != 0) die("%s", kmcpg_last_error());
  return cls;
}
// ... and the file, once stage 1 is rolled up and the pair table is read: the logs are replayed with both, and the references are written
// by the formatter kmcp-refstats --recount uses.  All pairs go in: the rows of a reference stage 1 dropped are skipped at replay, so its
// pairs are never asked for — with no row cut that equals the TSV route's skip
typedef std::map<std::string, std::vector<uint64_t>> RecountCounters;  // per listed reference: RECOUNT_WORDS per chunk
static void write_recount(const Options& o, kmcpg_db* db, const std::vector<std::string>& target, const std::vector<uint32_t>& cls,
                          const std::map<std::string, Stage1Ref>& stage1, kmcpg_recount_totals* tot, RecountCounters* listed, kmcpg::RecountThresholds* thresholds) {
  uint32_t n_classes = 0;
  for (uint32_t c : cls) n_classes = std::max(n_classes, c + 1);
  std::vector<kmcpg_recount_class> classes(n_classes);
  for (size_t c = 0; c < cls.size(); c++) {
    const auto it = stage1.find(target[c]);
    classes[cls[c]] = it == stage1.end() ? kmcpg_recount_class{0, 0, 0, 0} : kmcpg_recount_class{it->second.ok ? 1u : 0u, 0, it->second.reads, it->second.ureads};
  }
  uint64_t n = 0;
  if (kmcpg_cooccur_read(db, nullptr, 0, &n, nullptr) != 0) die("%s", kmcpg_last_error());
  std::vector<kmcpg_cooccur_pair> pairs(n);
  if (kmcpg_cooccur_read(db, pairs.data(), n, &n, nullptr) != 0) die("%s", kmcpg_last_error());
  kmcpg_recount_params rp{1 - o.ref_stats_d, o.ref_stats_r, o.ref_stats_no_amb_corr ? 1u : 0u, ref_stats_species(o) ? 1u : 0u};
  if (kmcpg_recount_run(db, classes.data(), n_classes, pairs.data(), n, &rp) != 0) die("%s", kmcpg_last_error());
  const uint32_t n_cols = (uint32_t)target.size();
  std::vector<kmcpg_recount_col> cols(n_cols);
  if (kmcpg_recount_read(db, cols.data(), n_cols, tot) != 0) die("%s", kmcpg_last_error());
  RecountCounters& counters = *listed;
  for (uint32_t c = 0; c < n_cols; c++) {
    if (!cols[c].match && !cols[c].uniq && !cols[c].hic && !cols[c].bases) continue;
    const auto it = stage1.find(target[c]);
    if (it == stage1.end()) die("--ref-stats-recount: %s was recounted but has no row in stage 1", target[c].c_str());
    uint32_t tidx = 0;
    kmcpg_col_info(db, c, nullptr, &tidx, nullptr, nullptr);
    const uint64_t chunk = (uint16_t)tidx;
    if (chunk >= it->second.chunks) die("--ref-stats-recount: chunk %llu of %s is outside its %llu chunks", (unsigned long long)chunk, target[c].c_str(), (unsigned long long)it->second.chunks);
    std::vector<uint64_t>& w = counters[target[c]];
    if (w.empty()) w.assign((size_t)it->second.chunks * kmcpg::RECOUNT_WORDS, 0);
    const uint64_t v[kmcpg::RECOUNT_WORDS] = {cols[c].match, cols[c].uniq, cols[c].hic, cols[c].bases};
    for (int j = 0; j < kmcpg::RECOUNT_WORDS; j++) w[chunk * kmcpg::RECOUNT_WORDS + j] += v[j];
  }
  std::vector<recount_format::Ref> list;
  for (const auto& kv : counters) list.push_back(recount_format::Ref{&kv.first, stage1.at(kv.first).chunks, stage1.at(kv.first).tlen, kv.second.data()});
  const kmcpg::RefstatsMode preset = kmcpg::refstats_mode(o.ref_stats_mode);
  kmcpg::RecountThresholds th;
  th.min_chunks_reads = preset.min_chunks_reads, th.min_uniq_reads = preset.min_uniq_reads, th.min_hic_ureads = preset.min_hic_ureads;
  th.min_hic_ureads_prop = preset.min_hic_ureads_prop, th.max_depth_stdev = preset.max_chunks_depth_stdev;
  th.min_chunks_fraction = o.ref_stats_p_given ? o.ref_stats_p : preset.min_chunks_fraction;
  tsv_out::Out out(o.ref_stats_recount, -1);
  recount_format::write(out, list, tot->recounted_reads, tot->unique_reads, tot->corrected_reads, th);
  out.close();
  *thresholds = th;
}

// --ref-stats-profile: stage 4/4 — em_run (kmcp_amd/csrc/em_rule.hpp) with kmcpg_em_pass as the pass, from the references stage 3 lists
// (`listed`: their stage-3 counters) to the table kmcp-refstats --profile writes.  A reference's chunk is the sum of its columns of that
// chunk, as in the files of the earlier stages
static void write_profile(const Options& o, kmcpg_db* db, const std::vector<std::string>& target, const std::vector<uint32_t>& cls,
                          const std::map<std::string, Stage1Ref>& stage1, const RecountCounters& listed, const kmcpg::RecountThresholds& th, kmcpg::EmResult* res,
                          kmcpg_em_totals* tot) {
  const uint32_t n_cols = (uint32_t)target.size();
  uint32_t n_classes = 0;
  for (uint32_t c : cls) n_classes = std::max(n_classes, c + 1);
  std::vector<kmcpg::EmClass> classes(n_classes);
  std::vector<uint8_t> est(n_classes, 0);
  std::vector<double> cov(n_classes, 0.0);
  std::vector<uint64_t> chunk_of(n_cols, UINT64_MAX);  // a column's place in the chunk table: its reference's first chunk + its own
  uint64_t n_chunks = 0;
  for (uint32_t c = 0; c < n_cols; c++) {
    const auto it = listed.find(target[c]);
    if (it == listed.end()) continue;
    const Stage1Ref& s1 = stage1.at(target[c]);
    kmcpg::EmClass& k = classes[cls[c]];
    if (k.columns.empty()) {
      k.name = target[c], k.tlen = s1.tlen;
      for (uint64_t i = 0; i < s1.chunks; i++) k.columns.push_back(n_chunks++);
      const uint64_t* w = it->second.data();
      est[cls[c]] = kmcpg::em_start(kmcpg::recount_rollup(s1.chunks, s1.tlen, th, [&](uint64_t i) { return w + i * kmcpg::RECOUNT_WORDS; }), &cov[cls[c]]) ? 1 : 0;
    }
    uint32_t tidx = 0;
    kmcpg_col_info(db, c, nullptr, &tidx, nullptr, nullptr);
    if ((uint16_t)tidx < s1.chunks) chunk_of[c] = k.columns[(uint16_t)tidx];
  }
  std::vector<kmcpg_em_class> pass_classes(n_classes);
  std::vector<kmcpg_em_col> cols(n_cols);
  const uint32_t level_species = ref_stats_species(o) ? 1u : 0u;
  const auto pass = [&](const std::vector<uint8_t>& e, const std::vector<double>& cv, std::vector<kmcpg::EmChunk>* chunks, uint64_t* assigned) {
    for (uint32_t k = 0; k < n_classes; k++) pass_classes[k] = kmcpg_em_class{e[k] ? 1u : 0u, 0, cv[k]};
    if (kmcpg_em_pass(db, pass_classes.data(), n_classes, level_species) != 0) return -1;
    if (kmcpg_em_read(db, cols.data(), n_cols, tot) != 0) return -1;
    chunks->assign(n_chunks, kmcpg::EmChunk());
    for (uint32_t c = 0; c < n_cols; c++) {
      if (chunk_of[c] == UINT64_MAX) continue;
      kmcpg::EmChunk& w = (*chunks)[chunk_of[c]];
      w.match += cols[c].match, w.uniq += cols[c].uniq, w.hic += cols[c].hic;
      w.single_bases += cols[c].single_bases, w.bases_lo += cols[c].bases_lo, w.bases_hi += cols[c].bases_hi;
    }
    *assigned = tot->assigned_reads;
    return 0;
  };
  kmcpg::EmParams ep;
  ep.th = th, ep.max_iters = (int)o.ref_stats_iters, ep.pct_threshold = o.ref_stats_pct;
  memset(tot, 0, sizeof *tot);
  if (kmcpg::em_run(classes, est, cov, ep, pass, res) != 0) die("%s", kmcpg_last_error());
  const std::vector<uint32_t> order = kmcpg::em_finish(classes, o.ref_stats_filter, res);
  tsv_out::Out out(o.ref_stats_profile, -1);
  profile_format::write(out, classes, *res, order);
  out.close();
}

static kmcpg_params make_params(const Options& o, int sort_by, bool paired) {
  kmcpg_params params{};
  params.min_qlen = o.min_qlen;
  params.min_matched = o.min_kmers;
  params.min_qcov = o.min_qcov;
  params.min_tcov = o.min_tcov;
  params.max_fpr = o.max_fpr;
  params.dedup_threshold = o.dedup;
  params.try_se = o.try_se;
  params.sort_by = sort_by;
  params.do_not_sort = o.do_not_sort;
  params.top_n_scores = o.top_scores;
  params.fpr_buf_size = paired ? 499 : 249;
  return params;
}

// The batch limits now that the database is open.  A batch also closes at 64 Mbases (long queries); paged indexes want the largest batches
// the host can hold (a batch's device workspace is up to 24 B per base: the library says how many bases fit beside the resident index).
// (-g: whole genomes as queries, packed 4 bases to a byte on the host — 256 Mbases per batch, 64 assemblies of 4 Mbp: the GPU needs
// ~2 ms for them while the readers need ~100, and the device workspace of a batch is 24 bytes per base — a gigabase batch made the
// process allocate, and the driver reclaim after it, 25 GB for nothing: profiles/r06_cli_e2e.txt)
static void open_gate(Pipeline& p, int k) {
  const Options& o = p.o;
  size_t mb = p.paged_passes > 1 ? std::min<size_t>((size_t)o.batch * 512, (size_t)2 << 30) : (o.whole_file ? (size_t)256 << 20 : (size_t)64 << 20);
  uint64_t hint = 0;
  if (kmcpg_batch_hint(p.db, &hint) == 0 && hint > 0) mb = std::max<size_t>((size_t)1 << 20, std::min<size_t>(mb, (size_t)hint));
  p.gate.open(mb, (size_t)o.batch, k);
}

// ---- searcher threads
// Two searchers: libkmcpgpu serialises their GPU halves and runs the host half (thresholds, FPR, sorting) outside that lock,
// so one batch is finalized while the next one's kernels run.
// (A paged index searches one batch at a time inside the library and wants the largest batches: one searcher, which joins the
// batches the reader cut before the database was open — consecutive ones, so the order of the output is untouched.)
// Each searcher keeps `depth` batches in flight through kmcpg_submit / kmcpg_wait_pairs (round 6; one synchronous
// kmcpg_search_batch_pairs call per batch before): a submit returns once the batch is staged, so the upload and the kernels of
// the next batch queue up behind this one's instead of waiting for this thread to come back from the host half.
struct Searcher {
  Pipeline& p;
  const size_t depth;
  std::deque<std::pair<kmcpg_ticket*, std::unique_ptr<Batch>>> fl;  // submitted, not yet waited for: oldest first
  double my_gpu = 0, my_wait = 0;
  uint64_t my_sum = 0, my_matches = 0;

  explicit Searcher(Pipeline& pl) : p(pl), depth(pl.paged_passes > 1 ? 1 : 2) {}

  // the one-call form: it also halves a batch whose workspace does not fit (kmcp_gpu.h kmcpg_batch_hint)
  void search_sync(Batch& bb) {
    if (bb.windows) {  // (the window route failed for memory: its windows as text, what `seqkit sliding | kmcp search` would hand over)
      std::vector<uint8_t> wt;
      std::vector<uint64_t> wo{0};
      for (size_t r = 0; r + 1 < bb.offs.size(); r++) {
        const uint64_t L = bb.offs[r + 1] - bb.offs[r];
        for (uint64_t j = 0; j < bb.wpre[r + 1] - bb.wpre[r]; j++) {
          const WindowSpan w = window_span(L, j, p.wspec);
          wt.insert(wt.end(), bb.seqs.begin() + (ptrdiff_t)(bb.offs[r] + w.start), bb.seqs.begin() + (ptrdiff_t)(bb.offs[r] + w.end));
          wo.push_back(wt.size());
        }
      }
      if (kmcpg_search_batch_pairs(p.db, wt.data(), wo.data(), nullptr, nullptr, (uint32_t)(wo.size() - 1), &p.params, &bb.res) != 0) die("%s", kmcpg_last_error());
      return;
    }
    if (bb.packed) {  // (a rare path: the text again, the one-call form reads text)
      bb.seqs.resize((size_t)bb.n_bases + 16);
      if (kmcpg_unpack2(bb.codes.data(), bb.n_bases, bb.exc.data(), bb.n_exc, bb.seqs.data()) != 0) die("%s", kmcpg_last_error());
    }
    if (kmcpg_search_batch_pairs(p.db, bb.seqs.data(), bb.offs.data(), bb.paired ? bb.seqs2.data() : nullptr, bb.paired ? bb.offs2.data() : nullptr,
                                 (uint32_t)bb.size(), &p.params, &bb.res) != 0)
      die("%s", kmcpg_last_error());
  }

  // --ref-stats-only, a batch the ticket route could not take for memory: the one-call form counts it all the same (and halves it if it
  // must); what came to the host is then its whole result
  void search_sync_stats(Batch& bb) {
    static std::atomic<bool> said{false};
    if (!said.exchange(true))
      warn("--ref-stats-only: a batch did not fit the statistics-only route (%s); it is counted through the route that brings all its matches to the host, "
           "which the summary line counts as left to the host", kmcpg_last_error());
    search_sync(bb);
    const kmcpg_result_pairs& r = bb.res;
    kmcpg_result_stats& st = bb.stats;
    st = kmcpg_result_stats{};
    st.n_reads = r.n_reads;
    for (uint32_t i = 0; i < r.n_reads; i++) st.matched_reads += r.match_offs[i + 1] > r.match_offs[i] ? 1 : 0;
    st.kept_pairs = r.n_reads ? r.match_offs[r.n_reads] : 0;
    st.left_reads = st.matched_reads, st.left_pairs = st.kept_pairs;  // (all of them came to the host)
    st.bytes_d2h = st.kept_pairs * sizeof(kmcpg_pair) + st.n_reads * (sizeof(uint64_t) + 2 * sizeof(int32_t));
    kmcpg_result_pairs_free(&bb.res);
  }

  // --binning, a batch the ticket route could not take for memory: the one-call form brings all its matches to the host (and halves the
  // batch if it must), and the bins come from the rule itself (kmcp_amd/csrc/bin_rule.hpp) over the plan the library was given
  void search_sync_bins(Batch& bb) {
    static std::atomic<bool> said{false};
    if (!said.exchange(true))
      warn("--binning: a batch did not fit the binning route (%s); it is binned through the route that brings all its matches to the host", kmcpg_last_error());
    search_sync(bb);
    const kmcpg_result_pairs& r = bb.res;
    bb.bres = kmcpg_result_bins{};
    bb.bres.n_reads = r.n_reads;
    bb.bins.assign(r.n_reads, kmcpg::BIN_NONE);
    for (uint32_t i = 0; i < r.n_reads; i++) {
      kmcpg::BinRange range;
      for (uint64_t j = r.match_offs[i]; j < r.match_offs[i + 1]; j++) range.add(p.bin_node[r.pairs[j].col]);
      bb.bins[i] = range.bin(p.bin_plan);
      bb.bres.binned_reads += range.none() ? 0 : 1;
    }
    bb.bres.kept_pairs = r.n_reads ? r.match_offs[r.n_reads] : 0;
    bb.bres.host_reads = r.n_reads, bb.bres.left_pairs = bb.bres.kept_pairs;  // (all of them came to the host)
    bb.bres.bytes_d2h = bb.bres.kept_pairs * sizeof(kmcpg_pair) + bb.bres.n_reads * (sizeof(uint64_t) + 2 * sizeof(int32_t));
    kmcpg_result_pairs_free(&bb.res);
  }

  void publish(std::unique_ptr<Batch> bb) {
    if (!p.o.quiet && !p.stats_only() && !p.bins_only()) {  // order-independent checksum of the (query, column, mKmers) tuples: the same on 1, 2, 4, 8 GPUs
      const kmcpg_result_pairs& r = bb->res;
      for (uint32_t i = 0; i < r.n_reads; i++)
        for (uint64_t j = r.match_offs[i]; j < r.match_offs[i + 1]; j++)
          my_sum += tuple_mix(bb->first_idx + i, r.pairs[j].col, r.pairs[j].count);
      if (r.n_reads) my_matches += r.match_offs[r.n_reads];
    }
    p.q_out.push(std::move(bb));
  }

  void finish_oldest() {
    kmcpg_ticket* t = fl.front().first;
    std::unique_ptr<Batch> bb = std::move(fl.front().second);
    fl.pop_front();
    const auto t0 = Clock::now();
    if (p.bins_only()) bb->bins.resize(bb->size());
    const int rc = p.bins_only()    ? kmcpg_wait_bins(t, bb->bins.data(), &bb->bres)
                   : p.stats_only() ? kmcpg_wait_stats(t, &bb->stats)
                   : p.regions()    ? kmcpg_wait_summaries(t, &bb->sres)
                                    : kmcpg_wait_pairs(t, &bb->res);
    // (a statistics-only batch may have been counted by the time its wait runs out of memory: searching it again would count it twice)
    if (rc != 0 && p.stats_only()) die("--ref-stats-only: %s", kmcpg_last_error());
    else if (rc == KMCPG_ENOMEM && p.bins_only()) search_sync_bins(*bb);  // (binning a batch changes nothing on the handle: it may be searched again)
    else if (rc == KMCPG_ENOMEM && !p.regions()) search_sync(*bb);  // (kmcpg_wait consumed the ticket; the batch's buffers are still ours)
    else if (rc != 0) die("%s", kmcpg_last_error());
    my_gpu += seconds_since(t0);
    publish(std::move(bb));
  }

  // the asynchronous form that takes the batch as the reader left it: the records' windows, packed codes, or text
  int submit(Batch& b, kmcpg_ticket** t) {
    if (p.bins_only())  // (reads as text, single or paired: validate_flags refused the rest)
      return kmcpg_submit_bins(p.db, b.seqs.data(), b.offs.data(), b.paired ? b.seqs2.data() : nullptr, b.paired ? b.offs2.data() : nullptr, (uint32_t)b.size(), &p.params, t);
    if (p.stats_only())
      return kmcpg_submit_stats(p.db, b.seqs.data(), b.offs.data(), b.paired ? b.seqs2.data() : nullptr, b.paired ? b.offs2.data() : nullptr, (uint32_t)b.size(), &p.params, t);
    if (b.windows && p.regions()) return kmcpg_submit_windows_summary(p.db, b.seqs.data(), b.offs.data(), (uint32_t)(b.offs.size() - 1), &p.wspec, &p.params, t);
    if (b.windows) return kmcpg_submit_windows(p.db, b.seqs.data(), b.offs.data(), (uint32_t)(b.offs.size() - 1), &p.wspec, &p.params, t);
    if (b.packed) return kmcpg_submit_packed(p.db, b.codes.data(), b.offs.data(), b.exc.data(), b.n_exc, (uint32_t)b.size(), &p.params, t);
    return kmcpg_submit(p.db, b.seqs.data(), b.offs.data(), b.paired ? b.seqs2.data() : nullptr, b.paired ? b.offs2.data() : nullptr, (uint32_t)b.size(),
                        &p.params, t);
  }

  void run() {
    std::unique_ptr<Batch> b;
    for (;;) {
      const auto tw = Clock::now();
      // (with batches of its own in flight a searcher does not sleep on an empty input queue: it brings its oldest batch home first)
      if (!fl.empty() ? !p.q_in.try_pop(&b) : !p.q_in.pop(&b)) {
        if (fl.empty()) break;
        finish_oldest();
        continue;
      }
      if (p.paged_passes > 1 && !b->packed && !b->windows) {
        std::unique_ptr<Batch> nb;
        while (b->size() < p.gate.batch_reads.load() && b->seqs.size() + b->seqs2.size() < p.gate.max_bases.load() && p.q_in.try_pop(&nb)) b->append(*nb);
      }
      const auto t0 = Clock::now();
      my_wait += std::chrono::duration<double>(t0 - tw).count();
      kmcpg_ticket* t = nullptr;
      int rc;
      while ((rc = submit(*b, &t)) == KMCPG_EBUSY) {
        if (!fl.empty()) {  // every lane of the handle is taken: one of this thread's own comes back first
          finish_oldest();
          continue;
        }
        // The lanes are all the other searcher's.  The one place where windows and reads differ: a batch of reads goes to the one-call form
        // below; windows have none that takes them as they are (it would mean cutting their text), so they wait for a lane to come back.
        // (a statistics-only or binning batch waits as well: the one-call form would bring all its matches down)
        if (!b->windows && !p.stats_only() && !p.bins_only()) break;
        std::this_thread::sleep_for(std::chrono::microseconds(200));
      }
      if (rc == KMCPG_ENOMEM && p.regions()) die("%s", kmcpg_last_error());  // (summaries have no one-call form)
      if (rc == KMCPG_EBUSY || rc == KMCPG_ENOMEM) {  // no lane / a batch that must be halved: the one-call form
        if (p.bins_only()) search_sync_bins(*b);
        else if (p.stats_only()) search_sync_stats(*b);
        else search_sync(*b);
        my_gpu += seconds_since(t0);
        publish(std::move(b));
        continue;
      }
      if (rc != 0) die("%s", kmcpg_last_error());
      my_gpu += seconds_since(t0);
      fl.emplace_back(t, std::move(b));
      if (fl.size() >= depth) finish_oldest();
    }
    {
      std::lock_guard<std::mutex> g(p.t_mu);
      p.sum_matches += my_matches;
      p.sum_check += my_sum;
      p.t_gpu += my_gpu;
      p.t_read_wait += my_wait;
    }
    if (p.live.fetch_sub(1) == 1) p.q_out.close();
  }
};

// ---- writer (the main thread): rows exactly as search.go:517-575 / :458-512.  A batch is formatted by several threads (contiguous ranges of
// queries, concatenated in order); with -o *.gz each range becomes its own gzip member, compressed in the same thread
// (a multi-member .gz is what pgzip/gzip readers, `kmcp profile` included, accept).
// One batch's text: the parts in order, each with the formatter that wrote it.  Text buffers go round — a match-heavy batch is hundreds
// of megabytes of rows, fresh strings would be page-faulted in (and grown by doubling) for every batch — and they go back to the
// THREAD that wrote them: a buffer another core filled last costs a cache-line transfer per line written (measured: formatting
// took 2-4x the thread-seconds of the same loop on thread-owned buffers, profiles/r06_cli_e2e.txt).
struct Text {
  std::vector<std::string> part;
  std::vector<RowFormatter*> owner;
};

// the formatted text of a batch goes to the file on a thread of its own, while the next batch is being formatted
static void run_flusher(Queue<std::unique_ptr<Text>>& q_flush, Out& out) {
  std::unique_ptr<Text> t;
  while (q_flush.pop(&t)) {
    for (size_t i = 0; i < t->part.size(); i++) {
      out.write_raw(t->part[i]);
      if (RowFormatter* F = t->owner[i]) F->give_back(std::move(t->part[i]));
    }
  }
}

// the next batch in input order; the searchers finish them in any order
static std::unique_ptr<Batch> next_in_order(Pipeline& p, std::map<uint64_t, std::unique_ptr<Batch>>& pending, uint64_t next_seq) {
  for (;;) {
    auto it = pending.find(next_seq);
    if (it != pending.end()) {
      std::unique_ptr<Batch> b = std::move(it->second);
      pending.erase(it);
      return b;
    }
    std::unique_ptr<Batch> got;
    const auto tp0 = Clock::now();
    const bool more = p.q_out.pop(&got);
    p.t_fmt_wait += seconds_since(tp0);
    if (!more) return nullptr;
    if (got->seq == next_seq) return got;
    pending.emplace(got->seq, std::move(got));  // finished ahead of its turn
  }
}

// parts of about equal work: a query costs one unit, a row one more (reads of a family database carry hundreds of rows);
// part pi = queries cut[pi] .. cut[pi + 1] - 1
static std::vector<uint32_t> cut_parts(const kmcpg_result_pairs& r, int nfmt) {
  const uint32_t n = r.n_reads;
  const uint64_t rows = n ? r.match_offs[n] : 0;
  // (up to four parts per thread, taken in turn: a thread that is descheduled for a while holds up a small part, not an eighth of the batch)
  const int parts = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)nfmt * 4, std::max<uint64_t>((n + 2047) / 2048, rows / 16384)));
  std::vector<uint32_t> cut((size_t)parts + 1, n);
  cut[0] = 0;
  for (int pi = 1; pi < parts; pi++) {
    const uint64_t want = (rows + n) * (uint64_t)pi / (uint64_t)parts;
    uint32_t a = cut[(size_t)pi - 1], z = n;  // first query i with match_offs[i] + i >= want
    while (a < z) {
      const uint32_t mid = a + (z - a) / 2;
      if (r.match_offs[mid] + mid < want) a = mid + 1; else z = mid;
    }
    cut[(size_t)pi] = a;
  }
  return cut;
}

// the rows of queries lo .. hi - 1 of `b` into `buf` (one gzip member of them for -o *.gz); returns how many of the queries matched
static uint64_t format_part(const Pipeline& p, const Batch& b, uint32_t lo, uint32_t hi, bool gz, RowFormatter& F, std::string& buf) {
  const kmcpg_result_pairs& r = b.res;
  uint64_t matched = 0;
  buf.reserve((size_t)(r.match_offs[hi] - r.match_offs[lo]) * 112 + (size_t)(hi - lo) * (p.o.keep_unmatched ? 64 : 8) + 256);
  // sliding windows: query i is window j of record wr, named as `seqkit sliding` names it: <id>_sliding:<start>-<end> (1-based)
  size_t wr = b.windows ? (size_t)(std::upper_bound(b.wpre.begin(), b.wpre.end(), (uint64_t)lo) - b.wpre.begin()) - 1 : 0;
  std::string wname;
  auto qname = [&](uint32_t i) -> std::string_view {
    if (!b.windows) return b.id(i);
    while (b.wpre[wr + 1] <= i) wr++;
    const WindowSpan w = window_span(b.offs[wr + 1] - b.offs[wr], i - b.wpre[wr], p.wspec);
    const std::string_view rid = b.id(wr);
    char tail[64];
    const int tn = snprintf(tail, sizeof tail, "_sliding:%llu-%llu", (unsigned long long)(w.start + 1), (unsigned long long)w.end);
    wname.assign(rid.data(), rid.size());
    wname.append(tail, (size_t)tn);
    return wname;
  };
  for (uint32_t i = lo; i < hi; i++) {
    const uint64_t qidx = b.first_idx + i;
    const uint64_t m0 = r.match_offs[i], m1 = r.match_offs[i + 1];
    if (m0 == m1) {
      if (p.o.keep_unmatched) F.unmatched(buf, qname(i), r.qlen[i], r.qkmers[i], r.ksize[i], qidx);
      continue;
    }
    matched++;
    // the query's Match records (float64 qCov / tCov / jacc, the FPR column, tLen ...) from its pairs, into a scratch array that
    // stays in this thread's cache: the batch's records never exist as a whole (1.5 GB per 131 072 reads of a family database)
    if (F.scratch.size() < m1 - m0) F.scratch.resize((size_t)(m1 - m0));
    if (kmcpg_expand_pairs(p.db, r.qkmers[i], r.pairs + m0, m1 - m0, F.scratch.data()) != 0) die("%s", kmcpg_last_error());
    F.rows(buf, qname(i), r.qlen[i], r.qkmers[i], F.scratch.data(), m1 - m0, p.target, r.ksize[i], qidx);
  }
  if (gz) buf = gzip_member(buf);
  return matched;
}

// the batch's vectors go back to the reader (fastx_reader.hpp ChunkPool)
static void recycle(Batch& b) {
  kmcpg_result_pairs_free(&b.res);
  kmcpg_result_summaries_free(&b.sres);
  ChunkPool::get().give(b.id_buf, b.id_offs, b.seqs, b.offs);
  if (b.paired) {
    std::vector<char> no_ids;
    std::vector<uint64_t> no_offs{0};
    ChunkPool::get().give(no_ids, no_offs, b.seqs2, b.offs2);
  }
}

static void write_results(Pipeline& p, Out& out) {
  const Options& o = p.o;
  // -j formatter threads; by default three quarters of the cores this process may use (the rest: two searchers, the reader's
  // parsers, the library's workers, the flusher) — on the 16-core grant of a GPU box 12 threads were the knee, profiles/r06_cli_e2e.txt
  const int nfmt = o.threads > 0 ? std::max(1, std::min(o.threads, 64)) : (int)std::max(4u, std::min(32u, usable_cpus() * 3 / 4));
  p.fmt_threads = nfmt;
  FormatPool pool(nfmt);
  Queue<std::unique_ptr<Text>> q_flush(4);
  std::thread flusher(run_flusher, std::ref(q_flush), std::ref(out));
  std::map<uint64_t, std::unique_ptr<Batch>> pending;  // batches that finished ahead of their turn
  uint64_t next_seq = 0;
  while (std::unique_ptr<Batch> b = next_in_order(p, pending, next_seq)) {
    next_seq += b->n_seq;
    const auto tf0 = Clock::now();
    const uint32_t n = b->res.n_reads;
    const std::vector<uint32_t> cut = cut_parts(b->res, nfmt);
    const int parts = (int)cut.size() - 1;
    std::unique_ptr<Text> text(new Text());
    text->part.resize((size_t)parts);
    text->owner.assign((size_t)parts, nullptr);
    std::vector<uint64_t> part_matched((size_t)parts, 0);
    std::vector<double> part_busy((size_t)parts, 0);
    const std::function<void(int, RowFormatter&)> work = [&](int pi, RowFormatter& F) {
      const auto tb0 = Clock::now();
      std::string& buf = text->part[(size_t)pi];
      F.take(buf);  // one of this thread's own buffers, if one has come back from the flusher
      text->owner[(size_t)pi] = &F;
      part_matched[(size_t)pi] = format_part(p, *b, cut[(size_t)pi], cut[(size_t)pi + 1], out.gz(), F, buf);
      part_busy[(size_t)pi] = seconds_since(tb0);
    };
    const auto tq0 = Clock::now();
    pool.run(parts, work);
    const auto tq1 = Clock::now();
    for (int pi = 0; pi < parts; pi++) {
      p.matched += part_matched[(size_t)pi];
      p.t_fmt_busy += part_busy[(size_t)pi];
    }
    q_flush.push(std::move(text));
    p.t_fmt_pool += std::chrono::duration<double>(tq1 - tq0).count();
    p.t_fmt_push += seconds_since(tq1);
    p.total += n;
    recycle(*b);
    p.t_fmt += seconds_since(tf0);
    if (!o.quiet) {
      double min = seconds_since(p.t_search) / 60.0;
      fprintf(stderr, "processed queries: %llu, speed: %.3f million queries per minute\r", (unsigned long long)p.total, p.total / 1e6 / min);
    }
  }
  q_flush.close();
  flusher.join();
}

// --regions-bed: the batches in input order through ONE streaming merger (kmcp_amd/csrc/regions_rule.hpp); a window with a summary is a
// query of the filtered TSV, named <record>_sliding:<start + 1>-<end>: the record's name is the region's reference
static void write_regions(Pipeline& p, Out& out, kmcpg::RegionMerger& merger) {
  std::map<uint64_t, std::unique_ptr<Batch>> pending;
  uint64_t next_seq = 0;
  std::string bed;
  while (std::unique_ptr<Batch> b = next_in_order(p, pending, next_seq)) {
    next_seq += b->n_seq;
    const auto tf0 = Clock::now();
    const kmcpg_result_summaries& r = b->sres;
    size_t wr = 0;
    for (uint32_t i = 0; i < r.n_windows; i++) {
      if (r.s[i].n_targets == 0) continue;
      while (b->wpre[wr + 1] <= i) wr++;
      const WindowSpan w = window_span(b->offs[wr + 1] - b->offs[wr], i - b->wpre[wr], p.wspec);
      const std::string_view rid = b->id(wr);
      merger.add(rid.data(), rid.size(), (int64_t)w.start + 1, (int64_t)w.end, r.s[i].n_targets, r.s[i].score, &bed);
      p.matched++;
    }
    out.write(bed);
    bed.clear();
    p.total += r.n_windows;
    recycle(*b);
    p.t_fmt += seconds_since(tf0);
  }
  merger.finish(&bed);
  out.write(bed);
}

// --ref-stats-only: nothing to format, nothing to write — the batches' counts are added up and their buffers go back to the reader
static void drain_stats(Pipeline& p) {
  std::unique_ptr<Batch> b;
  while (p.q_out.pop(&b)) {
    const kmcpg_result_stats& s = b->stats;
    p.stats.n_reads += s.n_reads, p.stats.matched_reads += s.matched_reads, p.stats.kept_pairs += s.kept_pairs;
    p.stats.left_reads += s.left_reads, p.stats.left_pairs += s.left_pairs, p.stats.bytes_d2h += s.bytes_d2h;
    p.total += s.n_reads;
    recycle(*b);
    if (!p.o.quiet) {
      double min = seconds_since(p.t_search) / 60.0;
      fprintf(stderr, "processed queries: %llu, speed: %.3f million queries per minute\r", (unsigned long long)p.total, p.total / 1e6 / min);
    }
  }
}

// --binning: one line per binned read, the batches in input order; nothing else is formatted
static void write_bins(Pipeline& p, tsv_out::Out& out) {
  std::map<uint64_t, std::unique_ptr<Batch>> pending;
  uint64_t next_seq = 0;
  while (std::unique_ptr<Batch> b = next_in_order(p, pending, next_seq)) {
    next_seq += b->n_seq;
    const auto tf0 = Clock::now();
    const size_t n = b->size();
    for (size_t i = 0; i < n; i++) {
      if (b->bins[i] == kmcpg::BIN_NONE) continue;
      const std::string_view id = b->id(i);
      binning_format::write_line(out, id.data(), id.size(), b->bins[i]);
      p.matched++;
    }
    const kmcpg_result_bins& s = b->bres;
    p.bins.n_reads += s.n_reads, p.bins.binned_reads += s.binned_reads, p.bins.kept_pairs += s.kept_pairs;
    p.bins.host_reads += s.host_reads, p.bins.left_pairs += s.left_pairs, p.bins.bytes_d2h += s.bytes_d2h;
    p.total += n;
    recycle(*b);
    p.t_fmt += seconds_since(tf0);
    if (!p.o.quiet) {
      double min = seconds_since(p.t_search) / 60.0;
      fprintf(stderr, "processed queries: %llu, speed: %.3f million queries per minute\r", (unsigned long long)p.total, p.total / 1e6 / min);
    }
  }
}

// ---- the end of a run
static void print_summary(const Pipeline& p) {
  fprintf(stderr, "\n");
  double min = seconds_since(p.t_search) / 60.0;
  const unsigned long long total = p.total, matched = p.matched;
  info("");
  info("processed queries: %llu, speed: %.3f million queries per minute", total, total / 1e6 / min);
  info("%.4f%% (%llu/%llu) queries matched", total ? (double)matched / (double)total * 100 : NAN, matched, total);
  info("done searching (pipeline: %.3f s in the GPU library, %.3f s formatting/writing, %.3f s waiting for the reader; reader: %.3f s parsing, %.3f s "
       "blocked; %.3f s before the search started)",
       p.t_gpu, p.t_fmt, p.t_read_wait, p.t_reader_total - p.t_reader_blocked, p.t_reader_blocked, std::chrono::duration<double>(p.t_search - p.t_start).count());
  info("writer loop: %.3f s formatting rows on %d threads (%.3f thread-seconds inside the parts), %.3f s waiting for the flusher, %.3f s waiting for searched batches",
       p.t_fmt_pool, p.fmt_threads, p.t_fmt_busy, p.t_fmt_push, p.t_fmt_wait);
  info("matches: %llu, checksum %016llx (order-independent over (queryIdx, column, mKmers): the same on any number of GPUs)", (unsigned long long)p.sum_matches,
       (unsigned long long)p.sum_check);
  if (p.o.out_file != "-") info("search results saved to: %s", p.o.out_file.c_str());
}

// trailer read by `kmcp profile` (profile.go:1945-1951)
static void write_trailer(const Pipeline& p, Out& out) {
  char tr[256];
  int n = snprintf(tr, sizeof tr, "# input queries: %llu\n# matched queries: %llu\n", (unsigned long long)p.total, (unsigned long long)p.matched);
  std::string trailer(tr, (size_t)n);
  if (p.total) n = snprintf(tr, sizeof tr, "# matched percentage: %.4f%%\n", (double)p.matched / (double)p.total * 100);
  else n = snprintf(tr, sizeof tr, "# matched percentage: NaN%%\n");
  trailer.append(tr, (size_t)n);
  out.write(trailer);
  out.close();
}

int main(int argc, char** argv) {
  Options o = parse_args(argc, argv);
  g_quiet = o.quiet;
  if (!o.log_file.empty()) {
    g_log = fopen(o.log_file.c_str(), "w");
    if (!g_log) die("%s: %s", o.log_file.c_str(), strerror(errno));
  }
  const auto t_start = Clock::now();
  keep_to_one_numa_node();
  if (o.parse_only) return run_parse_only(o);

  const bool sliding = o.sliding_step_given || o.sliding_window_given || o.sliding_greedy;
  const int sort_by = validate_flags(o, sliding);
  bool paired = false;
  const std::vector<std::string> files = resolve_inputs(o, &paired);
  const std::vector<std::string> db_dirs = resolve_databases(o);
  const NameMaps name_maps = load_name_maps(o, db_dirs);
  std::unique_ptr<kmcpg::Taxonomy> taxonomy;
  std::unique_ptr<kmcpg::TaxidMap> taxid_map;
  if (!o.taxid_maps.empty()) load_taxonomy(o, taxonomy, taxid_map);

  const kmcpg_window_spec wspec{(uint64_t)std::max(0ll, o.sliding_step), (uint64_t)std::max(0ll, o.sliding_window), o.sliding_greedy ? 1 : 0, 0};
  Pipeline p(o, paired, sliding, wspec);
  p.t_start = t_start;

  // The reader starts NOW, before the database is opened: parsing the input needs neither the GPU nor the index, and the HIP
  // runtime alone takes 0.2 s to come up (tools/ubench_init.cpp) — by the time the index is resident the first batches (up to
  // q_in's capacity) are waiting.  Batch limits are the defaults until the open has finished; should the index turn out to be
  // paged (larger than the GPU's memory: a batch then costs passes - 1 uploads), the early batches are joined into large ones
  // before they are searched (Batch::append).
  if (p.bins_only()) {  // the database's names from a metadata-only handle: what the list cannot give is refused before the GPU is touched
    kmcpg_db* meta = nullptr;
    kmcpg_opts mo{-1, 0, 1, 0};
    kmcpg_info mi;
    if (kmcpg_open(db_dirs[0].c_str(), &mo, &meta) != 0 || kmcpg_db_info(meta, &mi) != 0) die("%s", kmcpg_last_error());
    plan_binning(o, p, resolve_targets(o, meta, mi, name_maps), *taxonomy, *taxid_map);
    kmcpg_close(meta);
  }
  if (o.whole_file && o.gpu_passes < 0) read_k_early(p, db_dirs[0]);
  Reader the_reader{p, files};
  std::thread reader(&Reader::run, &the_reader);

  p.db = open_database(o, db_dirs, &p.paged_passes);
  kmcpg_info dbi;
  kmcpg_db_info(p.db, &dbi);
  if (dbi.minimizer && !dbi.syncmer)
    warn("this is a minimizer database: the reference publishes no result for minimizer sketches to check against, so this mode is "
         "verified against a restatement of bio/sketches only (DESIGN.md section 2)");
  if (!o.quiet) warn_narrow_blocks(p.db, dbi);
  if (o.min_qcov <= dbi.fpr)  // search.go:405-409
    die("query coverage threshold (%f) should not be smaller than FPR of single bloom filter of index database (%f)", o.min_qcov, dbi.fpr);
  if (!o.quiet) {
    info("database loaded: %s", o.db_dir.c_str());
    info("");
    info("-------------------- [main parameters] --------------------");
    info("  minimum    query length: %d", o.min_qlen);
    info("  minimum  matched k-mers: %d", o.min_kmers);
    info("  minimum  query coverage: %f", o.min_qcov);
    info("  minimum target coverage: %f", o.min_tcov);
    info("-------------------- [main parameters] --------------------");
    info("");
    info("searching ...");
  }
  p.target = resolve_targets(o, p.db, dbi, name_maps);
  p.params = make_params(o, sort_by, paired);
  if (!o.specific_level.empty()) set_specific(o, p.db, p.target, taxonomy.get(), taxid_map.get());
  if (!o.ref_stats.empty()) set_ref_stats(o, p.db, p.target, taxonomy.get(), taxid_map.get());
  std::vector<std::string> cooccur_names;
  if (!o.ref_stats_cooccur.empty()) cooccur_names = set_cooccur(o, p.db, p.target);
  std::vector<uint32_t> recount_classes;
  if (!o.ref_stats_recount.empty()) recount_classes = set_recount(o, p.db, p.target, taxonomy.get(), taxid_map.get());
  if (p.bins_only()) set_binning(p);

  p.t_search = Clock::now();
  std::optional<Out> out_file;  // (--ref-stats-only: no search result, no file)
  if (!p.stats_only() && !p.bins_only()) out_file.emplace(p.regions() ? o.regions_bed : o.out_file);
  std::optional<tsv_out::Out> bin_file;  // --binning: the binning file instead
  if (p.bins_only()) {
    bin_file.emplace(binning_format::file_name(o.binning), -1);
    binning_format::write_header(*bin_file, o.binning_sample_id);
  }
  if (!o.no_header && !p.regions() && !p.stats_only() && !p.bins_only()) out_file->write("#query\tqLen\tqKmers\tFPR\thits\ttarget\tchunkIdx\tchunks\ttLen\tkSize\tmKmers\tqCov\ttCov\tjacc\tqueryIdx\n");
  open_gate(p, dbi.k);

  const int n_search = p.paged_passes > 1 ? 1 : 2;  // (see Searcher)
  p.live.store(n_search);
  std::deque<Searcher> searcher_state;
  std::vector<std::thread> searchers;
  for (int si = 0; si < n_search; si++) searchers.emplace_back(&Searcher::run, &searcher_state.emplace_back(p));

  kmcpg::RegionParams region_params;
  region_params.min_overlap = o.regions_min_overlap;
  region_params.max_gap = o.regions_max_gap;
  region_params.ignore_type = o.regions_ignore_type;
  region_params.name_species = o.regions_name_species;
  region_params.name_assembly = o.regions_name_assembly;
  kmcpg::RegionMerger merger(region_params);
  if (p.bins_only()) write_bins(p, *bin_file);
  else if (p.stats_only()) drain_stats(p);
  else if (p.regions()) write_regions(p, *out_file, merger);
  else write_results(p, *out_file);
  reader.join();
  for (auto& t : searchers) t.join();

  if (p.bins_only()) {
    bin_file->close();
    if (!o.quiet) {
      fprintf(stderr, "\n");
      info("done searching (%.3f s in the GPU library, %.3f s waiting for the reader; no search result is written)", p.t_gpu, p.t_read_wait);
      info("binning result of %llu reads saved to: %s", (unsigned long long)p.matched, binning_format::file_name(o.binning).c_str());
    }
    // (one line of its own, whatever -q says: the tests read it)
    fprintf(stderr, "%llu reads searched, %llu binned; %llu reads (%llu pairs) left to the host, %llu bytes from the device\n", (unsigned long long)p.bins.n_reads,
            (unsigned long long)p.bins.binned_reads, (unsigned long long)p.bins.host_reads, (unsigned long long)p.bins.left_pairs, (unsigned long long)p.bins.bytes_d2h);
  } else if (p.stats_only()) {
    if (!o.quiet) {
      fprintf(stderr, "\n");
      info("done searching (%.3f s in the GPU library, %.3f s waiting for the reader; no search result is written)", p.t_gpu, p.t_read_wait);
    }
    // (one line of its own, whatever -q says: the tests read it)
    fprintf(stderr, "%llu reads searched, %llu matched; %llu reads (%llu pairs) left to the host, %llu bytes from the device\n", (unsigned long long)p.stats.n_reads,
            (unsigned long long)p.stats.matched_reads, (unsigned long long)p.stats.left_reads, (unsigned long long)p.stats.left_pairs, (unsigned long long)p.stats.bytes_d2h);
  } else if (p.regions()) {
    if (!o.quiet) {
      fprintf(stderr, "\n");
      info("specific regions: %llu windows, %llu with a summary (species- or assembly-specific), %llu regions saved to: %s", (unsigned long long)p.total,
           (unsigned long long)p.matched, (unsigned long long)merger.n_regions, o.regions_bed.c_str());
    }
    out_file->close();
  } else {
    if (!o.quiet) print_summary(p);
    write_trailer(p, *out_file);
  }
  if (!o.ref_stats.empty()) {
    uint64_t reruns = 0;
    std::set<std::string> kept;
    std::map<std::string, Stage1Ref> stage1;
    const uint64_t n_refs = write_ref_stats(o, p.db, p.target, &reruns, &kept, &stage1);
    if (!o.quiet)
      info("reference statistics (mode %d, level %s): %llu references saved to: %s (%llu batches counted by their rerun after a hit-buffer overflow)", o.ref_stats_mode,
           ref_stats_species(o) ? "species" : "strain", (unsigned long long)n_refs, o.ref_stats.c_str(), (unsigned long long)reruns);
    if (!o.ref_stats_cooccur.empty()) {
      kmcpg_cooccur_totals tot;
      const uint64_t n_pairs = write_cooccur(o, p.db, cooccur_names, kept, &tot);
      if (!o.quiet)
        info("shared reads of reference pairs: %llu pairs of kept references saved to: %s (%llu reads with several targets, %llu of them counted on the host, %llu for want of room in the table)",
             (unsigned long long)n_pairs, o.ref_stats_cooccur.c_str(), (unsigned long long)tot.multi_reads, (unsigned long long)tot.host_reads, (unsigned long long)tot.left_full);
    }
    if (!o.ref_stats_recount.empty()) {
      kmcpg_recount_totals tot;
      RecountCounters listed;
      kmcpg::RecountThresholds th;
      write_recount(o, p.db, p.target, recount_classes, stage1, &tot, &listed, &th);
      // (one line of its own, whatever -q says: the tests read it)
      fprintf(stderr, "%llu reads recounted, %llu of them replayed (%llu on the host, %llu for want of log room), %llu corrected\n", (unsigned long long)tot.recounted_reads,
              (unsigned long long)(tot.recounted_reads - tot.single_reads), (unsigned long long)tot.host_reads, (unsigned long long)tot.left_full,
              (unsigned long long)tot.corrected_reads);
      if (!o.ref_stats_profile.empty()) {
        kmcpg::EmResult res;
        kmcpg_em_totals et;
        write_profile(o, p.db, p.target, recount_classes, stage1, listed, th, &res, &et);
        // (one line of its own, whatever -q says: the tests read it)
        fprintf(stderr, "%d EM passes (%s), %llu reads assigned in the last, %llu of them split (%llu from the host log)\n", res.passes, res.converged ? "converged" : "not converged",
                (unsigned long long)et.assigned_reads, (unsigned long long)et.split_reads, (unsigned long long)et.host_reads);
      }
    }
  }
  // Everything the user asked for is on disk.  Giving back pinned staging buffers, streams and a resident index one by one takes
  // ~0.1 s and the runtime's own exit handlers as long again (profiles/r06_cli_e2e.txt) — a short-lived process leaves that to the
  // kernel driver, which reclaims a dead process's GPU memory anyway (the Go reference exits the same way: search.go:1027).
  // KMCP_SEARCH_FULL_TEARDOWN=1 closes the handle and returns through the runtime's handlers (leak checks, sanitizers).
  // (The handle itself IS closed: device memory a process leaves behind is reclaimed by the driver while the NEXT process is starting —
  // three back-to-back runs that each left 25 GB took 0.69, 0.90, 1.74 s.)
  const bool full_teardown = getenv("KMCP_SEARCH_FULL_TEARDOWN") != nullptr;
  if (kmcpg_close(p.db) != 0) die("%s", kmcpg_last_error());
  if (!o.quiet) {
    info("");
    info("elapsed time: %.3fs", seconds_since(p.t_start));
    info("");
  }
  if (g_log) fclose(g_log);
  fflush(stdout);
  fflush(stderr);
  if (!full_teardown) _exit(0);
  return 0;
}
