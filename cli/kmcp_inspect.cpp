// kmcp-inspect: `kmcp utils index-density` and `kmcp utils ref-info` of the reference (kmcp/cmd/index-density.go, ref-info.go) above the
// C ABI of libkmcpgpu.so.  The TSV of both is the reference's, line for line; the positional popcount of index-density runs on the GPU
// (kmcpg_block_density on a kmcpg_open_files handle), ref-info reads the headers alone unless --measured asks for the columns' set bits
// (kmcpg_col_ones).
//
//   kmcp-inspect index-density [-b/--bins 1024] [-s/--bin-size 0] [-o out.tsv[.gz]] [--out-img x.pgm] [--device N] [--verbose] <file.uniki>
//   kmcp-inspect ref-info -d <db> [-o out.tsv[.gz]] [-H/--no-header-row] [--measured [--device N]]
//
// Differences from the reference, all refusals: where index-density.go would panic or never fill a bin (bin size 0, a bin larger than
// the file's NumSigs, stdin as input) this command fails with a message; the image is a binary PGM (P5) with the reference's pixel
// values (:263-268), JPEG is not offered.  The persistent flags the `kmcp` dispatcher hands on (-j, -q, -i, --log) are accepted.
#include <dirent.h>
#include <errno.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <zlib.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "../include/kmcp_gpu.h"
#include "../kmcp_amd/csrc/dbformat.hpp"

using kmcpg::DbYml;
using kmcpg::UnikiHeader;

[[noreturn]] static void die(const char* fmt, ...) {  // checkError: "[ERRO] message", exit status 255
  va_list ap;
  va_start(ap, fmt);
  fputs("[ERRO] ", stderr);
  vfprintf(stderr, fmt, ap);
  fputc('\n', stderr);
  va_end(ap);
  exit(255);
}
static void info(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  fputs("[INFO] ", stderr);
  vfprintf(stderr, fmt, ap);
  fputc('\n', stderr);
  va_end(ap);
}
#define CK(expr)                                  \
  do {                                            \
    if ((expr) != 0) die("%s", kmcpg_last_error()); \
  } while (0)

static bool ends_with(const std::string& s, const char* suf) {
  const size_t n = strlen(suf);
  return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}
static std::string lower(std::string s) {
  for (auto& c : s) c = (char)tolower((unsigned char)c);
  return s;
}

// the reference's outStream: "-" = stdout, a ".gz" suffix (any case) = gzip
class Out {
 public:
  explicit Out(const std::string& path) {
    if (ends_with(lower(path), ".gz")) {
      g_ = path == "-" ? gzdopen(1, "wb") : gzopen(path.c_str(), "wb");
      if (!g_) die("%s: %s", path.c_str(), strerror(errno));
    } else {
      f_ = path == "-" ? stdout : fopen(path.c_str(), "wb");
      if (!f_) die("%s: %s", path.c_str(), strerror(errno));
    }
  }
  void write(const std::string& s) {
    if (s.empty()) return;
    if (g_) {
      for (size_t at = 0; at < s.size();) {
        const unsigned n = (unsigned)std::min<size_t>(s.size() - at, 1u << 30);
        if (gzwrite(g_, s.data() + at, n) != (int)n) die("write failed");
        at += n;
      }
    } else if (fwrite(s.data(), 1, s.size(), f_) != s.size()) {
      die("write failed: %s", strerror(errno));
    }
  }
  void close() {
    if (g_ && gzclose(g_) != Z_OK) die("write failed");
    if (f_ && (f_ == stdout ? fflush(f_) : fclose(f_)) != 0) die("write failed: %s", strerror(errno));
    g_ = nullptr;
    f_ = nullptr;
  }

 private:
  gzFile g_ = nullptr;
  FILE* f_ = nullptr;
};

static void append_u64(std::string& s, uint64_t v) {
  char t[24];
  int n = 0;
  do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v);
  while (n) s.push_back(t[--n]);
}

struct Args {
  std::vector<std::string> pos;
  std::string out_file = "-", out_img, db_dir;
  long bins = 1024, bin_size = 0;
  int device = 0;
  bool verbose = false, no_header = false, measured = false;
};

static long nonneg_int(const std::string& flag, const std::string& v) {  // getFlagNonNegativeInt
  char* end = nullptr;
  errno = 0;
  const long x = strtol(v.c_str(), &end, 10);
  if (v.empty() || *end || errno) die("invalid argument \"%s\" for \"%s\" flag", v.c_str(), flag.c_str());
  if (x < 0) die("value of flag --%s should be greater than or equal to 0", flag.c_str());
  return x;
}

static Args parse(int argc, char** argv, int from) {
  Args a;
  for (int i = from; i < argc; i++) {
    std::string w = argv[i], v;
    bool has_v = false;
    if (w.size() > 2 && w[0] == '-' && w[1] == '-') {
      const size_t eq = w.find('=');
      if (eq != std::string::npos) {
        v = w.substr(eq + 1);
        w = w.substr(0, eq);
        has_v = true;
      }
    }
    auto value = [&]() -> std::string {
      if (has_v) return v;
      if (i + 1 >= argc) die("flag needs an argument: %s", w.c_str());
      return argv[++i];
    };
    if (w == "-b" || w == "--bins") a.bins = nonneg_int("bins", value());
    else if (w == "-s" || w == "--bin-size") a.bin_size = nonneg_int("bin-size", value());
    else if (w == "-o" || w == "--out-file") a.out_file = value();
    else if (w == "--out-img") a.out_img = value();
    else if (w == "--device") a.device = (int)nonneg_int("device", value());
    else if (w == "-d" || w == "--db-dir") a.db_dir = value();
    else if (w == "-H" || w == "--no-header-row") a.no_header = true;
    else if (w == "--measured") a.measured = true;
    else if (w == "--verbose") a.verbose = true;
    else if (w == "-q" || w == "--quiet") a.verbose = false;
    else if (w == "-j" || w == "--threads" || w == "-i" || w == "--infile-list" || w == "--log") (void)value();  // the root command's flags: nothing here uses them
    else if (w == "-" || w.empty() || w[0] != '-') a.pos.push_back(w);
    else die("unknown flag: %s", w.c_str());
  }
  return a;
}

// ---- index-density (index-density.go:71-282) -----------------------------------------------------------------------------------------------
static int index_density(const Args& a) {
  if (a.pos.empty() || (a.pos.size() == 1 && a.pos[0] == "-")) die("stdin not supported, a .uniki file is needed");
  const std::string file = a.pos[0];  // the reference reads files[0] only (:115)
  if (!ends_with(file, ".uniki")) die("input should be stdin or %s file: %s", ".uniki", file.c_str());
  if (a.out_file == file || a.out_img == file) die("intput and output paths should not be the same: %s", file.c_str());
  if (!a.out_img.empty() && !ends_with(lower(a.out_img), ".pgm"))
    die("--out-img %s: JPEG is not offered by this build, the image is a binary PGM (P5): give a name that ends in .pgm", a.out_img.c_str());
  UnikiHeader h;
  const std::string e = kmcpg::read_uniki_header(file, &h);
  if (!e.empty()) die("%s", e.c_str());
  const uint64_t num_sigs = h.num_sigs, n_names = h.names.size();
  // :150-155
  uint64_t bins, bin_size = (uint64_t)a.bin_size;
  if (bin_size > 0) {
    bins = num_sigs / bin_size + 1;
  } else {
    if (a.bins == 0) die("the value of --bins should be greater than 0 when --bin-size is not given");
    bins = (uint64_t)a.bins;
    bin_size = num_sigs / bins;
  }
  if (bin_size == 0) die("bin size is 0: %llu bins for the %llu rows (#sigs) of %s; give fewer --bins or a --bin-size", (unsigned long long)bins,
                         (unsigned long long)num_sigs, file.c_str());
  if (bin_size > num_sigs) die("bin size %llu is larger than the %llu rows (#sigs) of %s: no bin would be filled", (unsigned long long)bin_size,
                               (unsigned long long)num_sigs, file.c_str());
  if (!a.out_img.empty() && bins >= 65536) die("the number of bins is too large for plotting: %llu (generating an image needs fewer than 65536)", (unsigned long long)bins);
  if (a.verbose) {
    info("#names: %llu, #sigs: %llu", (unsigned long long)n_names, (unsigned long long)num_sigs);
    info("#bins: %llu, bin size: %llu", (unsigned long long)bins, (unsigned long long)bin_size);
  }
  // The reference collects floor(NumSigs / binSize) full bins plus one trailing partial bin per column (:189-212; the trailing one
  // may be empty) and prints all but the trailing one (:232); the image shows the first `bins` of all of them (:264-268).
  const uint64_t n_full = num_sigs / bin_size;
  const bool tail_rows = num_sigs % bin_size != 0;
  const uint64_t n_counted = n_full + (tail_rows ? 1 : 0);
  if (n_names && n_counted > (~(size_t)0 / sizeof(uint32_t)) / n_names) die("the count matrix of %llu x %llu bins does not fit in memory", (unsigned long long)n_names, (unsigned long long)n_counted);
  uint32_t* counts = n_names ? new (std::nothrow) uint32_t[n_names * n_counted] : nullptr;
  if (n_names && !counts)
    die("cannot allocate the count matrix: %llu names x %llu bins x 4 bytes = %llu bytes", (unsigned long long)n_names, (unsigned long long)n_counted,
        (unsigned long long)(n_names * n_counted * 4));
  kmcpg_db* db = nullptr;
  const char* paths[1] = {file.c_str()};
  CK(kmcpg_open_files(paths, 1, a.device, &db));
  if (n_names) {
    kmcpg_density_spec spec{bin_size, 0, 0, 0};
    uint64_t nb = 0;
    CK(kmcpg_density_bins(db, 0, &spec, &nb));
    if (nb != n_counted) die("internal error: %llu bins counted, %llu expected", (unsigned long long)nb, (unsigned long long)n_counted);
    CK(kmcpg_block_density(db, 0, &spec, counts, n_names * n_counted));
  }
  CK(kmcpg_close(db));

  Out out(a.out_file);
  std::string text = "target\tchunkIdx\tbins\tbinSize\tcounts\n";
  uint64_t m = bin_size << 1, M = 0;
  for (uint64_t i = 0; i < n_names; i++) {
    text += h.names[i];
    text.push_back('\t');
    append_u64(text, h.indices[i] & 65535u);
    text.push_back('\t');
    append_u64(text, bins);
    text.push_back('\t');
    append_u64(text, bin_size);
    const uint32_t* c = counts + i * n_counted;
    for (uint64_t j = 0; j < n_full; j++) {
      text.push_back(j ? ',' : '\t');
      append_u64(text, c[j]);
      m = std::min<uint64_t>(m, c[j]);
      M = std::max<uint64_t>(M, c[j]);
    }
    text.push_back('\n');
    if (text.size() > (8u << 20)) {
      out.write(text);
      text.clear();
    }
  }
  out.write(text);
  out.close();
  if (a.verbose) {
    info("minimum count in bins of %llu: %llu (%f)", (unsigned long long)bin_size, (unsigned long long)m, (double)m / (double)bin_size);
    info("maximum count in bins of %llu: %llu (%f)", (unsigned long long)bin_size, (unsigned long long)M, (double)M / (double)bin_size);
  }
  if (!a.out_img.empty()) {
    const double r = 255.0 / (double)bin_size;  // :263
    FILE* f = fopen(a.out_img.c_str(), "wb");
    if (!f) die("%s: %s", a.out_img.c_str(), strerror(errno));
    fprintf(f, "P5\n%llu %llu\n255\n", (unsigned long long)bins, (unsigned long long)n_names);
    std::vector<uint8_t> line(bins);
    for (uint64_t i = 0; i < n_names; i++) {
      for (uint64_t j = 0; j < bins; j++) {
        // pixels the reference never sets stay 0; its trailing bin is an entry of its own, empty (count 0) when NumSigs is a multiple of binSize
        uint8_t px = 0;
        if (j <= n_full) {
          const uint32_t c = j < n_counted ? counts[i * n_counted + j] : 0u;
          px = (uint8_t)(255 - (uint8_t)((double)c * r));
        }
        line[j] = px;
      }
      if (fwrite(line.data(), 1, line.size(), f) != line.size()) die("write failed: %s", strerror(errno));
    }
    if (fclose(f) != 0) die("write failed: %s", strerror(errno));
    if (a.verbose) info("out image saved to: %s", a.out_img.c_str());
  }
  delete[] counts;
  return 0;
}

// ---- ref-info (ref-info.go:51-157) -----------------------------------------------------------------------------------------------------------
// CalcFPR (util-hash.go:55)
static double calc_fpr(uint64_t n, int num_hashes, uint64_t num_sigs) {
  return pow(1.0 - pow(M_E, (double)(-num_hashes) * (double)n / (double)num_sigs), (double)num_hashes);
}

static int ref_info(const Args& a) {
  if (a.db_dir.empty()) die("flag -d/--db-dir needed");
  DIR* d = opendir(a.db_dir.c_str());
  if (!d) die("read database error: open %s: %s", a.db_dir.c_str(), strerror(errno));
  std::vector<std::string> subs;
  while (struct dirent* de = readdir(d)) {
    const std::string name = de->d_name;
    if (name == "." || name == "..") continue;
    const std::string p = a.db_dir + "/" + name;
    struct stat st;
    if (stat(p.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) continue;
    if (stat((p + "/__db.yml").c_str(), &st) == 0) subs.push_back(p);
  }
  closedir(d);
  std::sort(subs.begin(), subs.end());  // os.ReadDir returns the entries sorted by file name
  if (subs.empty()) die("invalid kmcp database: %s", a.db_dir.c_str());
  Out out(a.out_file);
  std::string text;
  if (!a.no_header) text = a.measured ? "file\ti\ttarget\tchunkIdx\tchunks\tkmers\tfpr\tones\tfprMeasured\n" : "file\ti\ttarget\tchunkIdx\tchunks\tkmers\tfpr\n";
  char num[64];
  for (const std::string& sub : subs) {
    DbYml y;
    std::string e = kmcpg::read_db_yml(sub + "/__db.yml", &y);
    if (!e.empty()) die("%s", e.c_str());
    if (y.files.empty()) die("no index files");
    std::vector<uint64_t> ones;
    if (a.measured) {
      kmcpg_db* db = nullptr;
      kmcpg_opts o{a.device, 0, 1, 0};
      CK(kmcpg_open(sub.c_str(), &o, &db));
      kmcpg_info I;
      CK(kmcpg_db_info(db, &I));
      ones.assign(I.n_cols, 0);
      CK(kmcpg_col_ones(db, ones.data(), ones.size()));
      CK(kmcpg_close(db));
    }
    uint64_t col = 0;
    for (const std::string& fn : y.files) {
      UnikiHeader h;
      e = kmcpg::read_uniki_header(sub + "/" + fn, &h);
      if (!e.empty()) die("%s: %s", fn.c_str(), e.c_str());
      for (size_t i = 0; i < h.sizes.size(); i++, col++) {
        const uint32_t idx = h.indices[i];
        text += fn;
        text.push_back('\t');
        append_u64(text, i + 1);
        text.push_back('\t');
        text += h.names[i];
        text.push_back('\t');
        append_u64(text, idx & 65535u);
        text.push_back('\t');
        append_u64(text, idx >> 16);
        text.push_back('\t');
        append_u64(text, h.sizes[i]);
        snprintf(num, sizeof num, "\t%f", calc_fpr(h.sizes[i], h.num_hashes, h.num_sigs));
        text += num;
        if (a.measured) {
          if (col >= ones.size()) die("internal error: %s has more columns than the database handle", fn.c_str());
          text.push_back('\t');
          append_u64(text, ones[col]);
          // the rate at which a random k-mer hits this column of this file: every one of its numHashes bits is set
          snprintf(num, sizeof num, "\t%f", pow((double)ones[col] / (double)h.num_sigs, (double)h.num_hashes));
          text += num;
        }
        text.push_back('\n');
      }
      if (text.size() > (8u << 20)) {
        out.write(text);
        text.clear();
      }
    }
  }
  out.write(text);
  out.close();
  return 0;
}

static void usage(FILE* f) {
  fputs("kmcp-inspect: index inspection of the MI355X build of kmcp\n\nUsage:\n"
        "  kmcp-inspect index-density [flags] <file.uniki>   (kmcp utils index-density)\n"
        "      -b, --bins int        number of bins for counting the number of 1s (default 1024)\n"
        "      -s, --bin-size int    bin size/width; when given, bins = #sigs / bin-size + 1\n"
        "      -o, --out-file string out file, \".gz\" supported (default \"-\")\n"
        "          --out-img string  out density image, a binary PGM (.pgm); JPEG is not offered\n"
        "          --device int      GPU to count on (default 0)\n"
        "          --verbose         print #names, #sigs, #bins and the minimum / maximum count\n"
        "  kmcp-inspect ref-info -d <db> [flags]             (kmcp utils ref-info)\n"
        "      -d, --db-dir string   database directory created by \"kmcp index\"\n"
        "      -o, --out-file string out file, \".gz\" supported (default \"-\")\n"
        "      -H, --no-header-row   do not print the header row\n"
        "          --measured        add the columns ones (set bits of the column in the file, counted on the GPU) and\n"
        "                            fprMeasured = (ones / #sigs) ^ #hashes\n"
        "          --device int      GPU for --measured (default 0)\n", f);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    usage(stderr);
    return 255;
  }
  const std::string cmd = argv[1];
  if (cmd == "-h" || cmd == "--help") {
    usage(stdout);
    return 0;
  }
  for (int i = 2; i < argc; i++)
    if (!strcmp(argv[i], "-h") || !strcmp(argv[i], "--help")) {
      usage(stdout);
      return 0;
    }
  if (cmd == "index-density") return index_density(parse(argc, argv, 2));
  if (cmd == "ref-info") return ref_info(parse(argc, argv, 2));
  die("unknown command \"%s\" for \"kmcp-inspect\" (index-density, ref-info)", cmd.c_str());
}
