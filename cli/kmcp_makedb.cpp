// kmcp-makedb: `kmcp compute` followed by `kmcp index` (kmcp/cmd/compute.go, index.go) in one command above the C ABI of libkmcpgpu.so —
// genome files in, a searchable database out, no .unik files in between.
//
//   kmcp-makedb -O out.kmcp -k 21 [-n 10 -l 150 -m 1000] [-D scale | -W w | -S s] [-B regexp ...] [-N regexp]
//               [--num-hash 1 -f 0.3 -b 0 -j 16 -x 10M -X 256 -8 20M -1 200M -a alias --force] [--two-pass [--matrix-budget BYTES]]
//               {genome.fa[.gz] ... | -i list.txt | -I dir [-r regexp]}
//
// One file is one reference: the records whose header no -B expression matches are joined with kMax-1 N's (compute.go:569-627), the
// joined sequence is cut into chunks (kmcpg_split_bounds restates :675-744), every chunk is sketched on the GPU (kmcpg_sketch_genomes)
// and the lists go to kmcpg_build_db.  Files are read and inflated by a few threads while the GPU sketches the batch before.
// Where this command differs from the reference's two — all listed in INTEGRATION.md, "Building a database":
//   * -n is --split-number (compute); the number of hash functions of `kmcp index` has its long form --num-hash only;
//   * --circular, --by-seq and -s/--split-size are refused; one k-mer size per database;
//   * files are always joined, also with -n 1 (the reference joins in --split-number / --split-size mode only);
//   * regular expressions are std::regex (ECMAScript), not RE2; a leading "(?i)" is understood, and matching ignores case as it does there.
// --dry-run prints "name <tab> joined length <tab> chunks" per reference and touches no GPU.
//
// --two-pass builds a database larger than host memory ("Building a database"): pass 1 sketches every file and keeps
// only the k-mer count of every chunk; the block layout needs no more (kmcpg_builder_plan).  Pass 2 sketches the files again and ORs the
// lists, which never leave the GPU, into block matrices that stay in HBM (kmcpg_sketch_genomes_to -> kmcpg_builder_scatter_device); when
// the matrices exceed --matrix-budget together the blocks are built in rounds, each reading only the files it has columns of.  The
// database is the same bytes; the input is read and inflated twice (or more).
#include <dirent.h>
#include <errno.h>
#include <ftw.h>
#include <sched.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <fstream>
#include <functional>
#include <mutex>
#include <regex>
#include <string>
#include <thread>
#include <vector>

#include "../include/kmcp_gpu.h"
#include "fastx_reader.hpp"

[[noreturn]] void die(const char* fmt, ...) {  // checkError: "[ERRO] message", exit status 255
  va_list ap;
  va_start(ap, fmt);
  fputs("[ERRO] ", stderr);
  vfprintf(stderr, fmt, ap);
  fputc('\n', stderr);
  va_end(ap);
  fflush(stderr);
  _exit(255);  // reader threads may be running
}
static std::mutex g_log_mu;
static void logf(const char* level, const char* fmt, ...) {
  std::lock_guard<std::mutex> g(g_log_mu);
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "[%s] ", level);
  vfprintf(stderr, fmt, ap);
  fputc('\n', stderr);
  va_end(ap);
}
#define CK(expr)                                    \
  do {                                              \
    if ((expr) != 0) die("%s", kmcpg_last_error()); \
  } while (0)

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Args {
  std::vector<std::string> files;
  std::string out_dir, in_dir, infile_list, alias;
  std::string file_re = "\\.(f[aq](st[aq])?|fna)(.gz)?$", name_re = "(?i)(.+)\\.(f[aq](st[aq])?|fna)(.gz)?$";
  std::vector<std::string> filters;
  std::vector<int> ks;
  long scale = 1, minimizer_w = 0, syncmer_s = 0, split_number = 0, split_overlap = -1, split_min_ref = 1000;
  long num_hash = 1, block_size = 0, threads = 16, block_size_x = 256, device = 0;
  double fpr = 0.3;
  uint64_t kmers_x = 10ull << 20, kmers_8 = 20ull << 20, kmers_1 = 200ull << 20;
  uint64_t batch_bases = 1ull << 28;
  uint64_t matrix_budget = 0;  // --two-pass: 0 = the free HBM minus the sketcher's needs
  bool force = false, dry_run = false, verbose = false, two_pass = false;
};

static long parse_int(const std::string& flag, const std::string& v) {
  char* end = nullptr;
  errno = 0;
  const long x = strtol(v.c_str(), &end, 10);
  if (v.empty() || *end || errno) die("invalid argument \"%s\" for \"%s\" flag", v.c_str(), flag.c_str());
  return x;
}
static long nonneg_int(const std::string& flag, const std::string& v) {  // getFlagNonNegativeInt
  const long x = parse_int(flag, v);
  if (x < 0) die("value of flag --%s should be greater than or equal to 0", flag.c_str());
  return x;
}
static long pos_int(const std::string& flag, const std::string& v) {  // getFlagPositiveInt
  const long x = parse_int(flag, v);
  if (x <= 0) die("value of flag --%s should be greater than 0", flag.c_str());
  return x;
}
static uint64_t byte_size(const std::string& flag, const std::string& v) {  // bytesize.ParseByteSize: K, M, G are powers of 1024
  char* end = nullptr;
  const double x = strtod(v.c_str(), &end);
  if (v.empty() || end == v.c_str()) die("invalid size: %s", v.c_str());
  double m = 1;
  std::string u = end;
  for (auto& c : u) c = (char)toupper((unsigned char)c);
  if (u == "K" || u == "KB") m = 1024.0;
  else if (u == "M" || u == "MB") m = 1048576.0;
  else if (u == "G" || u == "GB") m = 1073741824.0;
  else if (!(u.empty() || u == "B")) die("invalid size: %s", v.c_str());
  if (x * m <= 0) die("value of flag --%s should be positive: %s", flag.c_str(), v.c_str());
  return (uint64_t)(x * m);
}

static const char* USAGE =
    "kmcp-makedb: genome files -> a kmcp database (`kmcp compute` + `kmcp index` on the GPU)\n\n"
    "  kmcp-makedb -O <out dir> -k <k> [compute flags] [index flags] {<genome files> | -i <list> | -I <dir>}\n\n"
    "compute: -k/--kmer  -D/--scale  -W/--minimizer-w  -S/--syncmer-s  -n/--split-number  -l/--split-overlap  -m/--split-min-ref\n"
    "         -N/--ref-name-regexp  -B/--seq-name-filter  -i/--infile-list  -I/--in-dir  -r/--file-regexp\n"
    "index:   --num-hash  -f/--false-positive-rate  -b/--block-size  -j/--threads  -x -X -8 -1 (big-genome blocks)  -a/--alias  --force\n"
    "other:   --device N  --batch-bases N  --dry-run  --verbose\n"
    "         --two-pass (sketch twice, keep no k-mer list in host memory)  --matrix-budget BYTES (HBM for block matrices per round; k/M/G)\n"
    "refused: --circular  --by-seq  -s/--split-size  (and -n here is --split-number, not the number of hash functions)\n";

static Args parse(int argc, char** argv) {
  struct Flag {
    const char* lng;
    char sht;
    bool takes;
  };
  static const Flag flags[] = {
      {"out-dir", 'O', true},      {"kmer", 'k', true},          {"scale", 'D', true},           {"minimizer-w", 'W', true},
      {"syncmer-s", 'S', true},    {"split-number", 'n', true},  {"split-overlap", 'l', true},   {"split-min-ref", 'm', true},
      {"split-size", 's', true},   {"ref-name-regexp", 'N', true}, {"seq-name-filter", 'B', true}, {"infile-list", 'i', true},
      {"in-dir", 'I', true},       {"file-regexp", 'r', true},   {"num-hash", 0, true},          {"false-positive-rate", 'f', true},
      {"block-size", 'b', true},   {"threads", 'j', true},       {"block-sizeX-kmers-t", 'x', true}, {"block-sizeX", 'X', true},
      {"block-size8-kmers-t", '8', true}, {"block-size1-kmers-t", '1', true}, {"alias", 'a', true}, {"force", 0, false},
      {"circular", 0, false},      {"by-seq", 0, false},         {"device", 0, true},            {"batch-bases", 0, true},
      {"dry-run", 0, false},       {"verbose", 0, false},        {"help", 'h', false},           {"compress", 'c', false},
      {"quiet", 'q', false},         {"two-pass", 0, false},       {"matrix-budget", 0, true},
  };
  Args a;
  bool circular = false, by_seq = false, split_size = false, budget_given = false;
  for (int i = 1; i < argc; i++) {
    std::string w = argv[i], v;
    const Flag* f = nullptr;
    bool has_v = false;
    if (w == "--") {
      for (i++; i < argc; i++) a.files.push_back(argv[i]);
      break;
    }
    if (w.size() > 2 && w[0] == '-' && w[1] == '-') {
      const size_t eq = w.find('=');
      const std::string name = w.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
      for (const Flag& c : flags)
        if (name == c.lng) f = &c;
      if (!f) die("unknown flag: %s", w.substr(0, eq).c_str());
      if (eq != std::string::npos) {
        v = w.substr(eq + 1);
        has_v = true;
      }
    } else if (w.size() >= 2 && w[0] == '-' && w != "-") {
      for (const Flag& c : flags)
        if (c.sht && w[1] == c.sht) f = &c;
      if (!f) die("unknown shorthand flag: '%c' in %s", w[1], w.c_str());
      if (w.size() > 2) {
        if (!f->takes) die("unknown shorthand flag in %s", w.c_str());
        v = w.substr(w[2] == '=' ? 3 : 2);
        has_v = true;
      }
    } else {
      a.files.push_back(w);
      continue;
    }
    const std::string n = f->lng;
    if (f->takes && !has_v) {
      if (i + 1 >= argc) die("flag needs an argument: --%s", f->lng);
      v = argv[++i];
    }
    if (n == "help") {
      fputs(USAGE, stdout);
      exit(0);
    } else if (n == "out-dir") a.out_dir = v;
    else if (n == "kmer") {
      size_t at = 0;
      while (at <= v.size()) {
        const size_t c = v.find(',', at);
        a.ks.push_back((int)parse_int(n, v.substr(at, c == std::string::npos ? std::string::npos : c - at)));
        if (c == std::string::npos) break;
        at = c + 1;
      }
    } else if (n == "scale") a.scale = pos_int(n, v);
    else if (n == "minimizer-w") a.minimizer_w = nonneg_int(n, v);
    else if (n == "syncmer-s") a.syncmer_s = nonneg_int(n, v);
    else if (n == "split-number") a.split_number = nonneg_int(n, v);
    else if (n == "split-overlap") a.split_overlap = nonneg_int(n, v);
    else if (n == "split-min-ref") a.split_min_ref = nonneg_int(n, v);
    else if (n == "split-size") split_size = true;
    else if (n == "ref-name-regexp") a.name_re = v;
    else if (n == "seq-name-filter") a.filters.push_back(v);
    else if (n == "infile-list") a.infile_list = v;
    else if (n == "in-dir") a.in_dir = v;
    else if (n == "file-regexp") a.file_re = v;
    else if (n == "num-hash") a.num_hash = parse_int(n, v);
    else if (n == "false-positive-rate") {
      char* end = nullptr;
      a.fpr = strtod(v.c_str(), &end);
      if (v.empty() || *end) die("invalid argument \"%s\" for \"-f, --false-positive-rate\" flag", v.c_str());
    } else if (n == "block-size") a.block_size = parse_int(n, v);
    else if (n == "threads") a.threads = pos_int(n, v);
    else if (n == "block-sizeX-kmers-t") a.kmers_x = byte_size(n, v);
    else if (n == "block-sizeX") a.block_size_x = pos_int(n, v);
    else if (n == "block-size8-kmers-t") a.kmers_8 = byte_size(n, v);
    else if (n == "block-size1-kmers-t") a.kmers_1 = byte_size(n, v);
    else if (n == "alias") a.alias = v;
    else if (n == "force") a.force = true;
    else if (n == "circular") circular = true;
    else if (n == "by-seq") by_seq = true;
    else if (n == "device") a.device = nonneg_int(n, v);
    else if (n == "batch-bases") a.batch_bases = (uint64_t)pos_int(n, v);
    else if (n == "dry-run") a.dry_run = true;
    else if (n == "verbose") a.verbose = true;
    else if (n == "two-pass") a.two_pass = true;
    else if (n == "matrix-budget") {
      a.matrix_budget = byte_size(n, v);
      budget_given = true;
    }
    // --compress, --quiet: nothing to do (no .unik files; warnings always go to stderr)
  }
  // what this command does not do, by the flag's name
  if (circular) die("flag --circular is not supported by kmcp-makedb (chunks of a split genome are linear, compute.go:305)");
  if (by_seq) die("flag --by-seq is not supported by kmcp-makedb: one file is one reference");
  if (split_size) die("flag -s/--split-size is not supported by kmcp-makedb: use -n/--split-number");
  if (budget_given && !a.two_pass) die("flag --matrix-budget needs --two-pass: only the two-pass build keeps block matrices in HBM");
  // compute.go:172-181
  if (a.ks.empty()) die("flag -k/--kmer needed");
  for (int k : a.ks) {
    if (k < 1) die("invalid k: %d", k);
    if (k > 64) die("k-mer size (%d) should be <=64", k);
  }
  std::sort(a.ks.begin(), a.ks.end());
  a.ks.erase(std::unique(a.ks.begin(), a.ks.end()), a.ks.end());
  if (a.ks.size() > 1) die("flag -k/--kmer: kmcp-makedb builds a database of one k-mer size (%zu given); build one database per size", a.ks.size());
  if (a.out_dir.empty()) die("flag -O/--out-dir is needed");
  if (a.split_number > 65535) die("value of flag -n/--split-number should not be greater than 65535");  // :295
  if (a.minimizer_w && a.syncmer_s) die("flag --minimizer-w and --syncmer-s can not be given simultaneously");  // :331
  if (a.syncmer_s > a.ks.back()) die("value of flag --syncmer-s is too big");                                  // :325
  // index.go:191-198, :224-259
  if (!(a.fpr > 0)) die("value of flag --false-positive-rate should be greater than 0");
  if (a.fpr >= 1) die("value of -f/--false-positive-rate too big: %f", a.fpr);
  if (a.num_hash <= 0) die("value of flag --num-hash should be greater than 0");
  if (a.num_hash > 4) die("value of --num-hash too big: %ld", a.num_hash);
  if (a.block_size_x <= 8) die("value of flag -X/--block-sizeX should be greater than 8: %ld", a.block_size_x);
  if (a.block_size_x % 8) die("value of flag -X/--block-sizeX should be a multiple of 8: %ld", a.block_size_x);
  if (a.kmers_x >= a.kmers_8) die("value of flag -x/--block-sizeX-kmers-t (%llu) should be small than -8/--block-size8-kmers-t (%llu)", (unsigned long long)a.kmers_x, (unsigned long long)a.kmers_8);
  if (a.kmers_8 >= a.kmers_1) die("value of flag -8/--block-size8-kmers-t (%llu) should be small than -1/--block-size1-kmers-t (%llu)", (unsigned long long)a.kmers_8, (unsigned long long)a.kmers_1);
  if (a.split_number == 0) a.split_number = 1;          // :272
  if (a.split_overlap < 0) a.split_overlap = a.ks.back() - 1;  // :268-270
  return a;
}

// the reference prefixes (?i) to every expression (compute.go:223, :237, :251); std::regex has no inline flags: icase instead
static std::regex compile_re(std::string s, const char* what) {
  if (s.compare(0, 4, "(?i)") == 0) s = s.substr(4);
  try {
    return std::regex(s, std::regex::ECMAScript | std::regex::icase | std::regex::optimize);
  } catch (const std::regex_error& e) {
    die("failed to parse regular expression for %s: %s (%s)", what, s.c_str(), e.what());
  }
}

static bool has_suffix(const std::string& s, const char* suf) {
  const size_t n = strlen(suf);
  return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}
static std::string base_name(const std::string& p) {
  const size_t s = p.find_last_of('/');
  return s == std::string::npos ? p : p.substr(s + 1);
}
static std::string trim_extension(std::string f) {  // filepathTrimExtension (util.go:145-180)
  if (has_suffix(f, ".gz") || has_suffix(f, ".GZ")) f.resize(f.size() - 3);
  const size_t dot = f.find_last_of('.');
  return dot == std::string::npos || dot == 0 ? f : f.substr(0, dot);
}

static void walk_dir(const std::string& dir, const std::regex& re, std::vector<std::string>* out) {  // directory symlinks are followed (stat)
  DIR* d = opendir(dir.c_str());
  if (!d) die("walking dir: %s: %s", dir.c_str(), strerror(errno));
  std::vector<std::string> names;
  while (dirent* e = readdir(d))
    if (strcmp(e->d_name, ".") && strcmp(e->d_name, "..")) names.push_back(e->d_name);
  closedir(d);
  std::sort(names.begin(), names.end());
  for (const auto& n : names) {
    const std::string p = dir + "/" + n;
    struct stat sb;
    if (stat(p.c_str(), &sb) != 0) continue;
    if (S_ISDIR(sb.st_mode)) walk_dir(p, re, out);
    else if (std::regex_search(n, re)) out->push_back(p);
  }
}

static int rm_entry(const char* p, const struct stat*, int, struct FTW*) { return remove(p); }
static void make_out_dir(const std::string& out_dir, bool force) {  // makeOutDir (util.go:92-113)
  struct stat sb;
  if (stat(out_dir.c_str(), &sb) == 0) {
    if (!S_ISDIR(sb.st_mode)) die("%s: not a directory", out_dir.c_str());
    bool empty = true;
    if (DIR* d = opendir(out_dir.c_str())) {
      while (dirent* e = readdir(d))
        if (strcmp(e->d_name, ".") && strcmp(e->d_name, "..")) empty = false;
      closedir(d);
    }
    if (!empty) {
      if (!force) die("out-dir not empty: %s, use --force to overwrite", out_dir.c_str());
      logf("INFO", "removing old output directory: %s", out_dir.c_str());
    }
    if (nftw(out_dir.c_str(), rm_entry, 32, FTW_DEPTH | FTW_PHYS) != 0) die("%s: %s", out_dir.c_str(), strerror(errno));
  }
}

struct Genome {
  std::string name, seq;
  bool done = false, skipped = false;
};

// the records of one file that no filter matches, joined with k_max - 1 N's (compute.go:569-627)
static void read_genome(const std::string& path, const std::vector<std::regex>& filters, int k_max, Genome* g) {
  FastxReader rd(path);
  FastxRec r;
  bool first = true;
  while (rd.next(&r)) {
    bool ignore = false;
    for (const auto& re : filters)
      if (std::regex_search(r.id, r.id + r.name_len, re)) {
        ignore = true;
        break;
      }
    if (ignore) continue;
    if (!first) g->seq.append((size_t)k_max - 1, 'N');
    g->seq.append(r.seq, r.seq_len);
    first = false;
  }
  // lenSum == 0 (:606-610): kept records that are all empty leave nothing but the N's between them
  if (g->seq.find_first_not_of('N') == std::string::npos) g->seq.clear();
}

// A few threads read, inflate and join the files which[0], which[1], ... ahead of the consumer, at most `window` files ahead; body(i) is
// called for every one in order, on the calling thread, with genomes[i] read (seq empty and skipped set when it holds nothing); the
// sequence is released after it.
template <class Body>
static void for_each_genome(const std::vector<std::string>& files, const std::vector<size_t>& which, const std::vector<std::regex>& filters, int k_max,
                            int n_readers, std::atomic<uint64_t>* read_us, std::vector<Genome>* genomes, Body&& body) {
  const size_t window = (size_t)n_readers * 4;
  std::mutex mu;
  std::condition_variable cv;
  size_t next_file = 0, consumed = 0;
  for (size_t i : which) {
    Genome& g = (*genomes)[i];
    g.done = g.skipped = false;
    std::string().swap(g.seq);
  }
  std::vector<std::thread> readers;
  for (int t = 0; t < n_readers; t++)
    readers.emplace_back([&] {
      for (;;) {
        size_t i;
        {
          std::unique_lock<std::mutex> l(mu);
          cv.wait(l, [&] { return next_file >= which.size() || next_file < consumed + window; });
          if (next_file >= which.size()) return;
          i = which[next_file++];
        }
        Genome& g = (*genomes)[i];
        const double t0 = now_s();
        read_genome(files[i], filters, k_max, &g);
        *read_us += (uint64_t)((now_s() - t0) * 1e6);
        if (g.seq.empty()) {
          g.skipped = true;
          logf("WARN", "skipping %s: no valid sequences", files[i].c_str());
        }
        std::lock_guard<std::mutex> l(mu);
        g.done = true;
        cv.notify_all();
      }
    });
  for (size_t p = 0; p < which.size(); p++) {
    Genome& g = (*genomes)[which[p]];
    {
      std::unique_lock<std::mutex> l(mu);
      cv.wait(l, [&] { return g.done; });
    }
    body(which[p]);
    std::string().swap(g.seq);
    std::lock_guard<std::mutex> l(mu);
    consumed = p + 1;
    cv.notify_all();
  }
  for (auto& t : readers) t.join();
}

static int granted_cpus() {
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) return std::max(1, CPU_COUNT(&set));
  return 1;
}

// ---- --two-pass
typedef std::function<void(const std::vector<size_t>&, const std::function<void(size_t)>&)> EachFn;

// one batch of joined genomes on its way through kmcpg_sketch_genomes_to
struct SinkBatch {
  std::string seqs;
  std::vector<uint64_t> offs{0};
  std::vector<size_t> file;  // genome (file) index of every sequence
};

struct FilePlace {
  uint32_t first_col = 0, n_cols = 0;  // the file's chunks are columns first_col .. first_col + n_cols - 1
  bool sketched = false;
};

struct TwoPass {
  const std::vector<std::string>* files;
  const std::vector<Genome>* genomes;
  std::vector<FilePlace> place;
  std::vector<kmcpg_build_colmeta> cols;  // pass 1: all that is kept of a chunk
  kmcpg_builder* builder = nullptr;
  const SinkBatch* batch = nullptr;  // the one in flight
  std::vector<uint32_t> col_ids;
  std::string err;
};

// pass 1: the counts alone.  The lists stay where the sort left them
static int count_sink(void* user, const kmcpg_sketch_piece* p) {
  TwoPass* tp = (TwoPass*)user;
  for (uint32_t c = 0; c < p->n_chunks; c++) {
    const size_t fi = tp->batch->file[p->genome[c]];
    FilePlace& fp = tp->place[fi];
    if (!fp.sketched) {
      fp.sketched = true;
      fp.first_col = (uint32_t)tp->cols.size();
      fp.n_cols = p->chunks[c];
    }
    kmcpg_build_colmeta m;
    memset(&m, 0, sizeof m);
    m.name = (*tp->genomes)[fi].name.c_str();
    m.gsize = tp->batch->offs[p->genome[c] + 1] - tp->batch->offs[p->genome[c]];
    m.chunk_idx = p->chunk_idx[c];
    m.chunks = p->chunks[c];
    m.n_hashes = p->koff[c + 1] - p->koff[c];
    tp->cols.push_back(m);
  }
  return 0;
}

// pass 2: every list into its column's block matrix, on the sketcher's stream behind the sort
static int scatter_sink(void* user, const kmcpg_sketch_piece* p) {
  TwoPass* tp = (TwoPass*)user;
  tp->col_ids.resize(p->n_chunks);
  for (uint32_t c = 0; c < p->n_chunks; c++) {
    const size_t fi = tp->batch->file[p->genome[c]];
    const FilePlace& fp = tp->place[fi];
    if (!fp.sketched || p->chunks[c] != fp.n_cols) {
      char msg[64];
      snprintf(msg, sizeof msg, ": %u chunk(s) now, %u in pass 1", p->chunks[c], fp.sketched ? fp.n_cols : 0);
      tp->err = (*tp->files)[fi] + msg + ": the input changed between the passes";
      return KMCPG_EINVAL;
    }
    tp->col_ids[c] = fp.first_col + p->chunk_idx[c];
  }
  return kmcpg_builder_scatter_device(tp->builder, p->d_hashes, p->koff, tp->col_ids.data(), p->n_chunks, p->stream);
}

static void two_pass(const Args& a, const std::vector<std::string>& files, const std::vector<Genome>& genomes, const kmcpg_split_spec& spec,
                     kmcpg_sketcher* sk, const kmcpg_build_cfg& bc, int n_readers, const std::atomic<uint64_t>& read_us, const EachFn& each) {
  const double t_start = now_s();
  TwoPass tp;
  tp.files = &files;
  tp.genomes = &genomes;
  tp.place.resize(files.size());
  double sketch_s = 0;
  // the files `which` through the sketcher in batches, one sketched while the next is read; every piece goes to `sink`
  auto run = [&](const std::vector<size_t>& which, kmcpg_sketch_sink sink) {
    std::thread worker;
    SinkBatch* in_flight = nullptr;
    int rc = 0;
    std::string err;
    auto finish = [&] {
      if (!in_flight) return;
      worker.join();
      if (rc) die("%s", err.c_str());
      delete in_flight;
      in_flight = nullptr;
    };
    auto launch = [&](SinkBatch* b) {
      finish();
      in_flight = b;
      worker = std::thread([&, b] {
        const double t0 = now_s();
        tp.batch = b;
        tp.err.clear();
        rc = kmcpg_sketch_genomes_to(sk, (const uint8_t*)b->seqs.data(), b->offs.data(), (uint32_t)b->file.size(), &spec, sink, &tp);
        if (rc) err = tp.err.empty() ? kmcpg_last_error() : tp.err;
        sketch_s += now_s() - t0;
      });
    };
    SinkBatch* cur = new SinkBatch();
    each(which, [&](size_t i) {
      if (genomes[i].skipped) return;
      if (!cur->file.empty() && cur->seqs.size() + genomes[i].seq.size() > a.batch_bases) {
        launch(cur);
        cur = new SinkBatch();
      }
      cur->seqs += genomes[i].seq;
      cur->offs.push_back(cur->seqs.size());
      cur->file.push_back(i);
    });
    if (!cur->file.empty()) launch(cur);
    else delete cur;
    finish();
  };

  // ---- pass 1: per file its columns, per column its count
  std::vector<size_t> all_files(files.size());
  for (size_t i = 0; i < files.size(); i++) all_files[i] = i;
  run(all_files, count_sink);
  for (size_t i = 0; i < files.size(); i++)
    if (!genomes[i].skipped && !tp.place[i].sketched)  // compute.go:720-723
      logf("WARN", "sequence is too short to split into %ld chunks with an overlap of %ld: %s", a.split_number, a.split_overlap, files[i].c_str());
  if (tp.cols.empty()) die("no k-mers to index: every input file was skipped");
  uint64_t total_hashes = 0;
  for (const auto& c : tp.cols) total_hashes += c.n_hashes;
  const double t_pass1 = now_s();

  // ---- plan: blocks from the counts, rounds from the budget
  kmcpg_builder_cfg cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.build = bc;
  uint64_t piece_bases = 1ull << 28;
  if (const char* e = getenv("KMCPG_SKETCH_PIECE_BASES")) piece_bases = std::max<uint64_t>(1, strtoull(e, nullptr, 10));
  cfg.hbm_reserve = 2 * a.batch_bases + 25 * piece_bases;  // the sketcher's workspace ("Building a database")
  CK(kmcpg_builder_open(&cfg, (int32_t)a.device, &tp.builder));
  CK(kmcpg_builder_add_cols(tp.builder, tp.cols.data(), (uint32_t)tp.cols.size()));
  uint32_t n_blocks = 0, n_rounds = 0;
  CK(kmcpg_builder_plan(tp.builder, a.matrix_budget, &n_blocks, &n_rounds));
  std::vector<uint32_t> col_round(tp.cols.size());
  for (uint32_t c = 0; c < tp.cols.size(); c++) CK(kmcpg_builder_col_place(tp.builder, c, nullptr, nullptr, &col_round[c]));

  // ---- pass 2: per round, the files that have a column in one of its blocks
  size_t files_pass2 = 0;
  for (uint32_t r = 0; r < n_rounds; r++) {
    std::vector<size_t> which;
    for (size_t i = 0; i < files.size(); i++) {
      bool in = false;
      for (uint32_t c = 0; c < tp.place[i].n_cols && tp.place[i].sketched && !in; c++) in = col_round[tp.place[i].first_col + c] == r;
      if (in) which.push_back(i);
    }
    CK(kmcpg_builder_begin_round(tp.builder, r));
    run(which, scatter_sink);
    CK(kmcpg_builder_end_round(tp.builder, a.out_dir.c_str()));
    logf("INFO", "round %u of %u: %zu of %zu file(s) read", r + 1, n_rounds, which.size(), files.size());
    files_pass2 += which.size();
  }
  CK(kmcpg_builder_finish(tp.builder, a.out_dir.c_str()));
  kmcpg_builder_stats st;
  memset(&st, 0, sizeof st);
  CK(kmcpg_builder_info(tp.builder, &st));
  const double t_end = now_s();
  logf("INFO", "%zu file(s), %zu column(s), %llu k-mers -> %s", files.size(), tp.cols.size(), (unsigned long long)total_hashes, a.out_dir.c_str());
  logf("INFO", "two-pass: %u block(s) in %u round(s); files read: pass 1 %zu, pass 2 %zu; %llu keys scattered in %.3f ms (%llu launch(es)); peak matrix bytes %llu",
       n_blocks, n_rounds, files.size(), files_pass2, (unsigned long long)st.keys_scattered, st.scatter_ms, (unsigned long long)st.scatter_launches,
       (unsigned long long)st.matrix_bytes_peak);
  logf("INFO", "no k-mer list was held in host memory: the lists went from the sort into the block matrices on the GPU");
  logf("INFO", "elapsed %.3f s: read + gunzip %.3f s on %d thread(s) (beside the GPU), sketch + scatter %.3f s, pass 1 wall %.3f s, plan + pass 2 wall %.3f s",
       t_end - t_start, (double)read_us.load() / 1e6, n_readers, sketch_s, t_pass1 - t_start, t_end - t_pass1);
  kmcpg_builder_close(tp.builder);
}

int main(int argc, char** argv) {
  const Args a = parse(argc, argv);
  const int k = a.ks[0], k_max = a.ks.back();
  // input files (compute.go:353-372)
  std::vector<std::string> files;
  if (!a.in_dir.empty()) {
    struct stat sb;
    if (stat(a.in_dir.c_str(), &sb) != 0) die("checking -I/--in-dir: %s: %s", a.in_dir.c_str(), strerror(errno));
    if (!S_ISDIR(sb.st_mode)) die("value of -I/--in-dir should be a directory: %s", a.in_dir.c_str());
    walk_dir(a.in_dir, compile_re(a.file_re, "matching file"), &files);
    if (files.empty()) logf("WARN", "  no files matching regular expression: %s", a.file_re.c_str());
  } else {
    files = a.files;
    if (!a.infile_list.empty()) {
      std::ifstream in(a.infile_list);
      if (!in) die("%s: %s", a.infile_list.c_str(), strerror(errno));
      std::string line;
      size_t n = 0;
      while (std::getline(in, line)) {
        while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
        if (line.empty()) continue;
        files.push_back(line);
        n++;
      }
      if (!n) logf("WARN", "no files found in file list: %s", a.infile_list.c_str());
    }
    for (const auto& f : files)
      if (access(f.c_str(), R_OK) != 0) die("%s: %s", f.c_str(), strerror(errno));
  }
  if (files.empty()) die("FASTA/Q files needed");
  if (a.name_re.find('(') == std::string::npos || a.name_re.find(')') == std::string::npos || a.name_re.find(')') < a.name_re.find('(') + 2)
    if (!a.name_re.empty()) die("value of --ref-name-regexp must contains \"(\" and \")\" to capture the ref name from file name");
  std::vector<std::regex> filters;
  for (const auto& f : a.filters) filters.push_back(compile_re(f, "matching sequence header"));
  std::vector<Genome> genomes(files.size());
  {
    const bool extract = !a.name_re.empty();
    std::regex re_name;
    if (extract) re_name = compile_re(a.name_re, "extracting the reference name");
    for (size_t i = 0; i < files.size(); i++) {
      const std::string base = base_name(files[i]);
      std::smatch m;
      if (extract && std::regex_search(base, m, re_name) && m.size() > 1) genomes[i].name = m[1].str();
      else genomes[i].name = trim_extension(base);
    }
  }
  kmcpg_split_spec spec;
  memset(&spec, 0, sizeof spec);
  spec.split_number = (uint32_t)a.split_number;
  spec.split_overlap = (uint32_t)a.split_overlap;
  spec.split_min_ref = (uint64_t)a.split_min_ref;
  spec.k_min = k;
  spec.k_max = k_max;

  // ---- readers: a few threads read, inflate and join files ahead of the consumer (for_each_genome)
  const int n_readers = std::max(1, std::min({(int)a.threads, granted_cpus(), 8, (int)files.size()}));
  std::atomic<uint64_t> read_us{0};
  std::vector<size_t> all_files(files.size());
  for (size_t i = 0; i < files.size(); i++) all_files[i] = i;
  auto each = [&](const std::vector<size_t>& which, auto&& body) { for_each_genome(files, which, filters, k_max, n_readers, &read_us, &genomes, body); };

  if (a.dry_run) {
    each(all_files, [&](size_t i) {  // nothing about a two-pass plan is known without sketching: --two-pass changes nothing here
      if (genomes[i].skipped) return;
      uint64_t n = 0;
      CK(kmcpg_split_bounds(genomes[i].seq.size(), &spec, nullptr, nullptr, 0, &n));
      if (n == 0) logf("WARN", "sequence is too short to split into %ld chunks with an overlap of %ld: %s", a.split_number, a.split_overlap, files[i].c_str());
      printf("%s\t%zu\t%llu\n", genomes[i].name.c_str(), genomes[i].seq.size(), (unsigned long long)n);
    });
    return 0;
  }

  make_out_dir(a.out_dir, a.force);
  const double t_start = now_s();
  kmcpg_sketch_cfg cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.ks[0] = k;
  cfg.n_k = 1;
  cfg.scale = (uint32_t)a.scale;
  cfg.minimizer_w = (uint32_t)a.minimizer_w;
  cfg.syncmer_s = (uint32_t)a.syncmer_s;
  kmcpg_sketcher* sk = nullptr;
  CK(kmcpg_sketcher_open(&cfg, (int32_t)a.device, &sk));
  kmcpg_build_cfg bc;
  memset(&bc, 0, sizeof bc);
  bc.k = k;
  bc.canonical = 1;
  bc.num_hashes = (int32_t)a.num_hash;
  bc.fpr = a.fpr;
  bc.threads = (int32_t)a.threads;
  bc.block_size = (int32_t)a.block_size;
  bc.scale = (uint32_t)a.scale;
  bc.minimizer_w = (uint32_t)a.minimizer_w;
  bc.syncmer_s = (uint32_t)a.syncmer_s;
  bc.split_seq = a.split_number > 1;
  bc.split_num = a.split_number > 1 ? (int32_t)a.split_number : 0;
  bc.split_overlap = a.split_number > 1 ? (int32_t)a.split_overlap : 0;
  std::string alias = a.alias;
  if (alias.empty()) {  // index.go:294-296
    std::string o = a.out_dir;
    while (o.size() > 1 && o.back() == '/') o.pop_back();
    alias = base_name(o);
  }
  bc.alias = alias.c_str();
  bc.kmers_x = a.kmers_x;
  bc.block_size_x = (int32_t)a.block_size_x;
  bc.kmers_8 = a.kmers_8;
  bc.kmers_1 = a.kmers_1;
  if (a.two_pass) {
    two_pass(a, files, genomes, spec, sk, bc, n_readers, read_us, [&](const std::vector<size_t>& which, const std::function<void(size_t)>& body) { each(which, body); });
    kmcpg_sketcher_close(sk);
    return 0;
  }

  // ---- batches: one is filled from the readers while the GPU sketches the one before it
  struct Batch {
    std::string seqs;
    std::vector<uint64_t> offs{0};
    std::vector<size_t> file;  // genome (file) index of every sequence
    kmcpg_sketch_result res{};
    int rc = 0;
    std::string err;
  };
  std::vector<Batch*> done;
  std::thread worker;
  Batch* in_flight = nullptr;
  double sketch_s = 0;
  auto finish = [&] {
    if (!in_flight) return;
    worker.join();
    if (in_flight->rc) die("%s", in_flight->err.c_str());
    std::string().swap(in_flight->seqs);
    done.push_back(in_flight);
    in_flight = nullptr;
  };
  auto launch = [&](Batch* b) {
    finish();
    in_flight = b;
    worker = std::thread([&, b] {
      const double t0 = now_s();
      b->rc = kmcpg_sketch_genomes(sk, (const uint8_t*)b->seqs.data(), b->offs.data(), (uint32_t)b->file.size(), &spec, &b->res);
      if (b->rc) b->err = kmcpg_last_error();
      sketch_s += now_s() - t0;
    });
  };
  Batch* cur = new Batch();
  each(all_files, [&](size_t i) {
    if (genomes[i].skipped) return;
    if (!cur->file.empty() && cur->seqs.size() + genomes[i].seq.size() > a.batch_bases) {
      launch(cur);
      cur = new Batch();
    }
    cur->seqs += genomes[i].seq;
    cur->offs.push_back(cur->seqs.size());
    cur->file.push_back(i);
  });
  if (!cur->file.empty()) launch(cur);
  else delete cur;
  finish();
  const double t_sketched = now_s();

  // ---- index: every list is in host memory until the layout is known (block sizing needs every column's k-mer count)
  std::vector<kmcpg_build_col> cols;
  uint64_t total_hashes = 0;
  for (Batch* b : done) {
    std::vector<uint32_t> seen(b->file.size(), 0);
    for (uint32_t c = 0; c < b->res.n_chunks; c++) {
      const uint32_t gi = b->res.genome[c];
      seen[gi]++;
      kmcpg_build_col col;
      memset(&col, 0, sizeof col);
      col.name = genomes[b->file[gi]].name.c_str();
      col.gsize = b->offs[gi + 1] - b->offs[gi];
      col.chunk_idx = b->res.chunk_idx[c];
      col.chunks = b->res.chunks[c];
      col.hashes = b->res.hashes + b->res.koff[c];
      col.n_hashes = b->res.koff[c + 1] - b->res.koff[c];
      total_hashes += col.n_hashes;
      cols.push_back(col);
    }
    for (size_t gi = 0; gi < seen.size(); gi++)
      if (!seen[gi])  // compute.go:720-723
        logf("WARN", "sequence is too short to split into %ld chunks with an overlap of %ld: %s", a.split_number, a.split_overlap, files[b->file[gi]].c_str());
  }
  if (cols.empty()) die("no k-mers to index: every input file was skipped");
  CK(kmcpg_build_db(a.out_dir.c_str(), &bc, cols.data(), (uint32_t)cols.size(), (int32_t)a.device));
  const double t_end = now_s();
  logf("INFO", "%zu file(s), %zu column(s), %llu k-mers -> %s", files.size(), cols.size(), (unsigned long long)total_hashes, a.out_dir.c_str());
  logf("INFO", "elapsed %.3f s: read + gunzip %.3f s on %d thread(s) (beside the GPU), sketch %.3f s, read + sketch wall %.3f s, index %.3f s", t_end - t_start,
       (double)read_us.load() / 1e6, n_readers, sketch_s, t_sketched - t_start, t_end - t_sketched);
  for (Batch* b : done) {
    kmcpg_sketch_result_free(&b->res);
    delete b;
  }
  kmcpg_sketcher_close(sk);
  return 0;
}
