// kmcp-refstats: which references are in the sample — host-side mirror of stage 1/4 of `kmcp profile` ("counting matches and unique
// matches for filtering out low-confidence references", kmcp/cmd/profile.go:761-1099; row parser util-profile.go:94-182) and, with
// --cooccur, of stage 2/4 ("counting ambiguous matches for correcting matches", profile.go:1117-1279).  Host only, no GPU.
//
//   kmcp-refstats [-o out.tsv[.gz]] [--cooccur pairs.tsv[.gz]] [-f 0.01] [-t 0.55] [-n 0] [--keep-perfect-matches] [--keep-main-matches] [--max-qcov-gap 0.4]
//                 [-m 3] [-p frac] [-H qcov] [--level species|strain|assembly] [-T map.tsv[,more.tsv]]... [-X taxdump/] [-i list.txt]
//                 [--recount recount.tsv[.gz]] [-r n] [-u n] [-U n] [-P prop] [-d stdev] [-D 0.05] [-R 0.05] [--no-amb-corr] [--norm-abund mean|min|max]
//                 [--profile profile.tsv[.gz]] [-I 10] [--abund-pct-threshold 0.01] [-F 0] [--binning out[.binning[.gz]]] [--sample-id S]
//                 [a.tsv[.gz] ...]
//
// Semantics restated from the reference (the counting rule, the verdict and the presets are kmcp_amd/csrc/refstats_rule.hpp):
//   * blank lines and every line that starts with '#' are dropped;
//   * a row is cut at its first 12 tabs (fewer than 13 fields is fatal); qCov (field 12) is parsed and the row dropped when it is below
//     -t, THEN FPR (field 4) is parsed and the row dropped when it is above -f; then the integer fields are parsed (a bad one is fatal);
//   * the remaining rows of consecutive equal query names form a query (per input file; counters accumulate across files); within a query
//     --keep-perfect-matches, --keep-main-matches / --max-qcov-gap and -n cut later rows;
//   * a reference's chunks and tLen are those of its first row; at --level species a target without a TaxId is fatal;
//   * -m picks H and p (mode 0 also --keep-main-matches); -H / -p override the preset only when given; the VALUE of -H (0.75 when not
//     given) must lie in [-t, 1], as in the reference, whatever the mode.
//   * --recount FILE: stage 3/4 ("recounting matches and unique matches", profile.go:1282-1888) after stages 1 and 2 — the rule, the
//     reference's quirk and our tie order are kmcp_amd/csrc/recount_rule.hpp, the file's format is cli/recount_format.hpp; -r -u -U -P -d
//     come from -m and are overridden only when given, -D -R --no-amb-corr --norm-abund are the reference's.
//   * --profile FILE: stage 4/4 ("estimating abundance using EM algorithm", profile.go:1907-2570, its end :2786-2853) after stages 1-3,
//     whether or not their files are asked for — the rule, the loop and our tie orders are kmcp_amd/csrc/em_rule.hpp, the table's format
//     is cli/profile_format.hpp; -I --abund-pct-threshold -F are the reference's.  The rows are kept in memory after stage 3 (about 56 bytes
//     per row of a reference stage 3 judged ok, and the distinct query names of one input at a time) and every
//     pass applies the row cuts after the skip of the rows outside ITS whitelist, as profile.go:2039-2226 does.  -m 0 is refused: its
//     final order rests on the score column, which this tool does not compute.
//   * --binning FILE: the binning pass of `kmcp profile -B` (profile.go:2591-2784) after stage 4 — one line `query<TAB>TaxId` per read
//     with a row of a reference the EM ended with (its whitelist after the last pass, before -F).  The rule, the pruned tree and what is
//     done with unknown TaxIds are kmcp_amd/csrc/bin_rule.hpp, the file's name and format cli/binning_format.hpp.  Needs --profile, -T, -X.
// The reference prints none of this (it goes on to stages 2-4); the output format is this tool's:
//   # matched reads: N
//   # unique reads: U
//   #ref chunks tLen reads ureads hicUreads chunksFrac verdict chunkReads chunkFirsts chunkUreads chunkHicUreads
// one line per reference with at least one row, in ascending byte order of the name; the four per-chunk lists are comma-joined.
// --cooccur FILE: a second pass over the inputs (stdin is refused) counts, for every pair of references that stage 1 kept (verdict ok),
// the queries whose kept rows name both — the rule and the reference's quirks are kmcp_amd/csrc/cooccur_rule.hpp:
//   # pairs: N
//   #refA refB reads
// one line per pair with refA < refB bytewise, in ascending order of (refA, refB).  The stage-1 output is what it is without the flag.
#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <fstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../kmcp_amd/csrc/cooccur_rule.hpp"
#include "../kmcp_amd/csrc/recount_rule.hpp"
#include "../kmcp_amd/csrc/refstats_rule.hpp"
#include "../kmcp_amd/csrc/taxonomy.hpp"
#include "../kmcp_amd/csrc/em_rule.hpp"
#include "../kmcp_amd/csrc/bin_rule.hpp"
#include "binning_format.hpp"
#include "profile_format.hpp"
#include "recount_format.hpp"
#include "tsv_in.hpp"
#include "tsv_out.hpp"

namespace {

using tsv_in::parse_float;
using tsv_in::RawLines;
using tsv_out::die;
using tsv_out::Out;

void usage() {
  fputs(
      "Count matches and unique matches per reference and judge which references are in the sample (stage 1/4 of kmcp profile)\n\n"
      "Usage:\n  kmcp-refstats [flags] [<search results> ...]\n\n"
      "Flags:\n"
      "  -o, --out-file string             Out file, supports a \".gz\" suffix (\"-\" for stdout). (default \"-\")\n"
      "  -f, --max-fpr float               Maximum false positive rate of a read in search result. (default 0.01)\n"
      "  -t, --min-query-cov float         Minimum query coverage of a read in search result. (default 0.55)\n"
      "  -n, --keep-top-qcovs int          Keep matches with the top N qCovs for a query, 0 for all.\n"
      "      --keep-perfect-matches        Only keep the perfect matches (qCov == 1) if there are.\n"
      "      --keep-main-matches           Only keep main matches, abandon matches with sharply decreased qCov (> --max-qcov-gap).\n"
      "      --max-qcov-gap float          Max qCov gap between adjacent matches. (default 0.4)\n"
      "  -m, --mode int                    Profiling mode, 0-5. (default 3)\n"
      "  -p, --min-chunks-fraction float   Minimum fraction of matched reference chunks with reads. (default 0.8)\n"
      "  -H, --min-hic-ureads-qcov float   Minimum query coverage of high-confidence uniquely matched reads. (default 0.75)\n"
      "  -T, --taxid-map strings           Tabular two-column file(s) mapping reference IDs to TaxIds.\n"
      "  -X, --taxdump string              Directory of NCBI taxonomy dump files: nodes.dmp, optional with merged.dmp and delnodes.dmp.\n"
      "      --level string                Level to estimate abundance at. available values: species, strain/assembly. (default \"species\")\n"
      "      --line-chunk-size int         Accepted for command-line compatibility. (default 5000)\n"
      "  -i, --infile-list string          File of input files list (one file per line).\n"
      "      --cooccur string              Also count the reads shared by every pair of kept references (stage 2/4 of kmcp profile) into\n"
      "                                    this file, supports a \".gz\" suffix. A second pass over the inputs: stdin is not supported.\n"
      "      --recount string              Also recount the reads with ambiguity correction and judge the references again (stage 3/4 of\n"
      "                                    kmcp profile) into this file, supports a \".gz\" suffix. Stdin is not supported.\n"
      "  -r, --min-chunks-reads int        Minimum number of reads for a reference chunk. (default 50)\n"
      "  -u, --min-uniq-reads int          Minimum number of uniquely matched reads for a reference. (default 20)\n"
      "  -U, --min-hic-ureads int          Minimum number of high-confidence uniquely matched reads for a reference. (default 5)\n"
      "  -P, --min-hic-ureads-prop float   Minimum proportion of high-confidence uniquely matched reads. (default 0.1)\n"
      "  -d, --max-chunks-depth-stdev float  Maximum standard deviation of relative depths of all chunks. (default 2)\n"
      "  -D, --min-dreads-prop float       Minimum proportion of distinct reads, for determing the right reference for ambiguous reads. (default 0.05)\n"
      "  -R, --max-mismatch-err float      Maximum error rate of a read being matched to a wrong reference. (default 0.05)\n"
      "      --no-amb-corr                 Do not correct ambiguous reads.\n"
      "      --norm-abund string           Method for normalizing abundance of a reference by the mean/min/max abundance in all chunks. (default \"mean\")\n"
      "      --profile string              Also estimate the abundances by EM (stage 4/4 of kmcp profile) and write the table of references\n"
      "                                    into this file, supports a \".gz\" suffix. Stdin and -m 0 are not supported.\n"
      "                                    The rows of the references stage 3 keeps stay in memory for the passes: about 56 bytes per row.\n"
      "  -I, --abund-max-iters int         Maximum iteration of abundance estimation. (default 10)\n"
      "      --abund-pct-threshold float   If the percentage change of the predominant target is smaller than this threshold, stop the iteration. (default 0.01)\n"
      "  -F, --filter-low-pct float        Filter out predictions with the smallest relative abundances summing up X%. Range: [0,100). (default 0)\n"
      "  -B, --binning string              Also save the binning result (one TaxId per read: that of its reference, or the lowest common\n"
      "                                    ancestor of its references) in CAMI format; \".binning.gz\" is appended unless the name ends in\n"
      "                                    \".binning\" or \".binning.gz\". Needs --profile, -T and -X. Stdin is not supported.\n"
      "  -s, --sample-id string            Sample ID in the binning result.\n",
      stderr);
}

// strconv.Atoi / ParseUint of a whole field
bool parse_int(const char* p, size_t n, bool sign_ok, uint64_t* v, bool* neg) {
  size_t i = 0;
  *neg = false;
  if (sign_ok && n && (p[0] == '-' || p[0] == '+')) *neg = p[0] == '-', i = 1;
  if (i == n) return false;
  uint64_t x = 0;
  for (; i < n; i++) {
    if (p[i] < '0' || p[i] > '9') return false;
    const uint64_t d = (uint64_t)(p[i] - '0');
    if (x > (UINT64_MAX - d) / 10) return false;
    x = x * 10 + d;
  }
  if (sign_ok && x > (uint64_t)INT64_MAX) return false;
  *v = x;
  return true;
}

struct Ref {
  uint32_t target_class, species_class;
  uint64_t chunks, tlen, base;  // its counters: 4 words per chunk from counters[4 * base]
  bool ok = false;              // stage 1 kept it (set once every row is counted)
  uint64_t reads = 0, ureads = 0;  // stage 1's sums (what stage 3 compares)
};

// a row cut at its first 12 tabs: field k = 1..12 (the 13th keeps the rest of the line)
struct Fields {
  const char* p;
  size_t tab[13];
  size_t get(int k, const char** fp) const {
    *fp = k == 1 ? p : p + tab[k - 2] + 1;
    return tab[k - 1] - (size_t)(*fp - p);
  }
};
// a line of a search result through the tests every stage makes when it parses a row: false = not a row (blank, comment) or dropped by -t / -f
bool parse_row(const char* p, size_t n, double min_qcov, double max_fpr, Fields* f, double* qcov) {
  size_t len = n;  // without the end of line
  if (len && p[len - 1] == '\n') len--;
  if (len && p[len - 1] == '\r') len--;
  if (len == 0 || p[0] == '#') return false;
  f->p = p;
  int nt = 0;
  for (size_t i = 0; i < len && nt < 12; i++)
    if (p[i] == '\t') f->tab[nt++] = i;
  if (nt < 12) die("invalid kmcp search result format");
  const char* fp;
  double fpr = 0;
  size_t fn = f->get(12, &fp);
  if (!parse_float(fp, fn, qcov)) die("failed to parse qCov: %.*s", (int)fn, fp);
  if (*qcov < min_qcov) return false;
  fn = f->get(4, &fp);
  if (!parse_float(fp, fn, &fpr)) die("failed to parse FPR: %.*s", (int)fn, fp);
  return !(fpr > max_fpr);
}

}  // namespace

int main(int argc, char** argv) {
  std::string out_file = "-", level = "species", taxdump, infile_list, cooccur_file, recount_file, norm_abund = "mean", profile_file, binning_file, sample_id;
  long max_iters = 10;
  double pct_threshold = 0.01, filter_low_pct = 0;
  long flag_r = 50, flag_u = 20, flag_U = 5;
  double flag_P = 0.1, flag_d = 2, flag_D = 0.05, flag_R = 0.05;
  bool given_r = false, given_u = false, given_U = false, given_P = false, given_d = false, no_amb_corr = false;
  std::vector<std::string> map_files, files;
  double max_fpr = 0.01, min_qcov = 0.55, flag_h = 0.75, flag_p = 0.8, max_gap = 0.4;
  bool given_h = false, given_p = false, keep_perfect = false, keep_main = false;
  long chunk = 5000, top_n = 0, mode = kmcpg::REFSTATS_DEFAULT_MODE;
  auto need = [&](int& i) -> const char* {
    if (i + 1 >= argc) die("flag needs an argument: %s", argv[i]);
    return argv[++i];
  };
  auto num = [&](const char* flag, const char* v) {
    double x = 0;
    if (!parse_float(v, strlen(v), &x)) die("invalid argument \"%s\" for \"%s\" flag", v, flag);
    return x;
  };
  auto integer = [&](const char* flag, const char* v) {
    uint64_t x = 0;
    bool neg = false;
    if (!parse_int(v, strlen(v), true, &x, &neg)) die("invalid argument \"%s\" for \"%s\" flag", v, flag);
    return neg ? -(long)x : (long)x;
  };
  // `kmcp-refstats ref-stats ...` = `kmcp utils ref-stats ...`: the sub-command word, accepted (only) as the first argument
  for (int i = (argc > 1 && strcmp(argv[1], "ref-stats") == 0) ? 2 : 1; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "-o" || a == "--out-file") out_file = need(i);
    else if (a == "-f" || a == "--max-fpr") max_fpr = num("-f, --max-fpr", need(i));
    else if (a == "-t" || a == "--min-query-cov") min_qcov = num("-t, --min-query-cov", need(i));
    else if (a == "-n" || a == "--keep-top-qcovs") top_n = integer("-n, --keep-top-qcovs", need(i));
    else if (a == "--keep-perfect-matches") keep_perfect = true;
    else if (a == "--keep-main-matches") keep_main = true;
    else if (a == "--max-qcov-gap") max_gap = num("--max-qcov-gap", need(i));
    else if (a == "-m" || a == "--mode") mode = integer("-m, --mode", need(i));
    else if (a == "-p" || a == "--min-chunks-fraction") flag_p = num("-p, --min-chunks-fraction", need(i)), given_p = true;
    else if (a == "-H" || a == "--min-hic-ureads-qcov") flag_h = num("-H, --min-hic-ureads-qcov", need(i)), given_h = true;
    else if (a == "-T" || a == "--taxid-map") {
      std::string v = need(i);  // a StringSlice flag: repeatable, each value a comma list
      size_t at = 0;
      for (;;) {
        const size_t c = v.find(',', at);
        const std::string one = v.substr(at, c == std::string::npos ? std::string::npos : c - at);
        if (!one.empty()) map_files.push_back(one);
        if (c == std::string::npos) break;
        at = c + 1;
      }
    } else if (a == "-X" || a == "--taxdump") taxdump = need(i);
    else if (a == "--level") level = need(i);
    else if (a == "--line-chunk-size") chunk = integer("--line-chunk-size", need(i));
    else if (a == "-i" || a == "--infile-list") infile_list = need(i);
    else if (a == "--cooccur") cooccur_file = need(i);
    else if (a == "--recount") recount_file = need(i);
    else if (a == "-r" || a == "--min-chunks-reads") flag_r = integer("-r, --min-chunks-reads", need(i)), given_r = true;
    else if (a == "-u" || a == "--min-uniq-reads") flag_u = integer("-u, --min-uniq-reads", need(i)), given_u = true;
    else if (a == "-U" || a == "--min-hic-ureads") flag_U = integer("-U, --min-hic-ureads", need(i)), given_U = true;
    else if (a == "-P" || a == "--min-hic-ureads-prop") flag_P = num("-P, --min-hic-ureads-prop", need(i)), given_P = true;
    else if (a == "-d" || a == "--max-chunks-depth-stdev") flag_d = num("-d, --max-chunks-depth-stdev", need(i)), given_d = true;
    else if (a == "-D" || a == "--min-dreads-prop") flag_D = num("-D, --min-dreads-prop", need(i));
    else if (a == "-R" || a == "--max-mismatch-err") flag_R = num("-R, --max-mismatch-err", need(i));
    else if (a == "--no-amb-corr") no_amb_corr = true;
    else if (a == "--norm-abund") norm_abund = need(i);
    else if (a == "--profile") profile_file = need(i);
    else if (a == "-B" || a == "--binning" || a == "--binning-result") binning_file = need(i);
    else if (a == "-s" || a == "--sample-id") sample_id = need(i);
    else if (a == "-I" || a == "--abund-max-iters") max_iters = integer("-I, --abund-max-iters", need(i));
    else if (a == "--abund-pct-threshold") pct_threshold = num("--abund-pct-threshold", need(i));
    else if (a == "-F" || a == "--filter-low-pct") filter_low_pct = num("-F, --filter-low-pct", need(i));
    else if (a == "-j" || a == "--threads" || a == "--log") need(i);  // accepted for command-line compatibility
    else if (a == "-q" || a == "--quiet") {
    } else if (a == "-h" || a == "--help") {
      usage();
      return 0;
    } else if (a.size() > 1 && a[0] == '-') die("unknown flag: %s", a.c_str());
    else files.push_back(a);
  }
  // profile.go:315-485, in its order
  if (mode < 0) die("value of flag --mode should be greater than or equal to 0");
  if (mode >= kmcpg::REFSTATS_MODES) die("invalid profiling mode: %ld", mode);
  if (max_fpr <= 0) die("value of flag --max-fpr should be greater than 0");
  if (min_qcov < 0) die("value of flag --min-query-cov should be greater than or equal to 0");
  if (top_n < 0) die("value of flag --keep-top-qcovs should be greater than or equal to 0");
  if (flag_p < 0) die("value of flag --min-chunks-fraction should be greater than or equal to 0");
  if (flag_p > 1) die("the value of -p/--min-chunks-fraction (%f) should be in range of [0, 1]", flag_p);
  if (flag_h <= 0) die("value of flag --min-hic-ureads-qcov should be greater than 0");
  if (flag_h > 1 || flag_h < min_qcov) die("the value of -H/--min-hic-ureads-qcov (%f) should be in range of [<-t/--min-query-cov>, 1]", flag_h);
  if (flag_r <= 0) die("value of flag --min-chunks-reads should be greater than 0");
  if (flag_d <= 0) die("value of flag --max-chunks-depth-stdev should be greater than 0");
  if (flag_u <= 0) die("value of flag --min-uniq-reads should be greater than 0");
  if (flag_U <= 0) die("value of flag --min-hic-ureads should be greater than 0");
  if (flag_P <= 0) die("value of flag --min-hic-ureads-prop should be greater than 0");
  if (flag_P > 1) die("the value of -P/--min-hic-ureads-prop (%f) should be in range of (0, 1]", flag_P);
  if (flag_D <= 0) die("value of flag --min-dreads-prop should be greater than 0");
  if (flag_D > 1) die("the value of -D/--min-dreads-prop (%f) should be in range of (0, 1]", flag_D);
  if (flag_R <= 0) die("value of flag --max-mismatch-err should be greater than 0");
  if (flag_R >= 1) die("the value of -R/--max-mismatch-err (%f) should be in range of (0, 1)", flag_R);
  if (max_iters <= 0) die("value of flag --abund-max-iters should be greater than 0");
  if (pct_threshold <= 0) die("value of flag --abund-pct-threshold should be greater than 0");
  if (filter_low_pct < 0 || filter_low_pct >= 100) die("the value of -F/--filter-low-pct (%f) should be in range of [0, 100)", filter_low_pct);
  if (!profile_file.empty() && mode == 0) die("flag --profile: -m 0 is not supported (its final order rests on the score column)");
  for (char& c : norm_abund) c = (char)tolower((unsigned char)c);
  if (norm_abund != "mean" && norm_abund != "min" && norm_abund != "max") die("invalid value of --norm-abund: %s. available: mean, min, max", norm_abund.c_str());
  kmcpg::RefstatsMode preset = kmcpg::refstats_mode((int)mode);
  kmcpg::RecountThresholds th;
  th.min_chunks_reads = given_r ? (uint64_t)flag_r : preset.min_chunks_reads;
  th.min_uniq_reads = given_u ? (uint64_t)flag_u : preset.min_uniq_reads;
  th.min_hic_ureads = given_U ? (uint64_t)flag_U : preset.min_hic_ureads;
  th.min_hic_ureads_prop = given_P ? flag_P : preset.min_hic_ureads_prop;
  th.max_depth_stdev = given_d ? flag_d : preset.max_chunks_depth_stdev;
  th.norm = norm_abund == "mean" ? kmcpg::RECOUNT_NORM_MEAN : norm_abund == "min" ? kmcpg::RECOUNT_NORM_MIN : kmcpg::RECOUNT_NORM_MAX;
  const double H = given_h ? flag_h : preset.hic_min_qcov, min_frac = given_p ? flag_p : preset.min_chunks_fraction;
  keep_main = keep_main || preset.keep_main;
  for (char& c : level) c = (char)tolower((unsigned char)c);
  bool level_species = false;
  if (level == "species") level_species = true;
  else if (level != "strain" && level != "assembly") die("invalid value for --level, available values: species, strain/assembly");
  if (!map_files.empty() && taxdump.empty()) die("flag -X/--taxdump is needed when -T/--taxid-map given");
  if (map_files.empty() && !taxdump.empty()) die("flag -T/--taxid-map is needed when -X/--taxdump given");
  if (level_species && map_files.empty()) die("-T/--taxid-map needed for --level species");
  if (chunk <= 0) die("value of flag --line-chunk-size should be greater than 0");

  for (const std::string& f : files)
    if (f != "-" && access(f.c_str(), F_OK) != 0) die("%s: stat %s: %s", f.c_str(), f.c_str(), strerror(errno));
  if (!infile_list.empty()) {
    std::ifstream fh(infile_list);
    if (!fh) die("read file list from '%s': %s", infile_list.c_str(), strerror(errno));
    std::string l;
    while (std::getline(fh, l)) {
      if (l.find_first_not_of(" \t\r\n") == std::string::npos) continue;
      if (!l.empty() && l.back() == '\r') l.pop_back();
      if (l != "-" && access(l.c_str(), F_OK) != 0) die("check file '%s': stat %s: %s", l.c_str(), l.c_str(), strerror(errno));
      files.push_back(l);
    }
  }
  if (files.empty()) files.push_back("-");
  for (const std::string& f : files)
    if (f != "-" && tsv_in::clean_path(f) == tsv_in::clean_path(out_file)) die("out file should not be one of the input file");
  if (!cooccur_file.empty()) {  // before anything is read
    for (const std::string& f : files) {
      if (f == "-") die("flag --cooccur: stdin is not supported (the search results are read twice)");
      if (tsv_in::clean_path(f) == tsv_in::clean_path(cooccur_file)) die("flag --cooccur: the file should not be one of the input file");
    }
    if (cooccur_file == "-" ? out_file == "-" : tsv_in::clean_path(cooccur_file) == tsv_in::clean_path(out_file)) die("flag --cooccur: the file must not be the out file (-o)");
  }

  if (!recount_file.empty()) {  // before anything is read
    for (const std::string& f : files) {
      if (f == "-") die("flag --recount: stdin is not supported (the search results are read three times)");
      if (tsv_in::clean_path(f) == tsv_in::clean_path(recount_file)) die("flag --recount: the file should not be one of the input file");
    }
    if (recount_file == "-" ? out_file == "-" : tsv_in::clean_path(recount_file) == tsv_in::clean_path(out_file)) die("flag --recount: the file must not be the out file (-o)");
    if (!cooccur_file.empty() && (recount_file == "-" ? cooccur_file == "-" : tsv_in::clean_path(recount_file) == tsv_in::clean_path(cooccur_file)))
      die("flag --recount: the file must not be the --cooccur file");
  }
  if (!profile_file.empty()) {  // before anything is read
    for (const std::string& f : files) {
      if (f == "-") die("flag --profile: stdin is not supported (the search results are read four times)");
      if (tsv_in::clean_path(f) == tsv_in::clean_path(profile_file)) die("flag --profile: the file should not be one of the input file");
    }
    const auto same = [&](const std::string& other) { return profile_file == "-" ? other == "-" : tsv_in::clean_path(profile_file) == tsv_in::clean_path(other); };
    if (same(out_file)) die("flag --profile: the file must not be the out file (-o)");
    if (!cooccur_file.empty() && same(cooccur_file)) die("flag --profile: the file must not be the --cooccur file");
    if (!recount_file.empty() && same(recount_file)) die("flag --profile: the file must not be the --recount file");
  }
  if (!binning_file.empty()) {  // before anything is read
    if (profile_file.empty()) die("flag --binning: --profile is needed (the reads are binned over the references the EM ends with)");
    if (map_files.empty() || taxdump.empty()) die("flag -T/--taxid-map and -X/--taxdump needed when -B/--binning-result given");
    binning_file = binning_format::file_name(binning_file);
    const auto same = [&](const std::string& other) { return tsv_in::clean_path(binning_file) == tsv_in::clean_path(other); };
    for (const std::string& f : files) {
      if (f == "-") die("flag --binning: stdin is not supported (the search results are read five times)");
      if (same(f)) die("flag --binning: the file should not be one of the input file");
    }
    if (same(out_file) || same(profile_file) || (!cooccur_file.empty() && same(cooccur_file)) || (!recount_file.empty() && same(recount_file)))
      die("flag --binning: the file must not be one of the other out files");
  }
  const bool stage3 = !recount_file.empty() || !profile_file.empty();
  th.min_chunks_fraction = min_frac;

  kmcpg::TaxidMap tmap;
  kmcpg::Taxonomy tax;
  if (!map_files.empty()) {
    std::string err;
    for (const std::string& f : map_files)
      if (!tmap.load(f, &err)) die("%s", err.c_str());
    if (tmap.ids.empty()) {
      std::string all;
      for (const std::string& f : map_files) all += (all.empty() ? "" : ", ") + f;
      die("no valid TaxIds found in TaxId mapping file: %s", all.c_str());
    }
    if (!tax.load(taxdump, &err)) die("%s", err.c_str());
  }

  // target name -> its classes and counters, filled as targets are met (chunks and tLen: the first row's)
  std::unordered_map<std::string, Ref> refs;
  std::vector<uint64_t> counters;
  std::string name;
  auto ref_of = [&](const char* p, size_t n, uint64_t chunks, uint64_t tlen) -> const Ref& {
    name.assign(p, n);
    auto it = refs.find(name);
    if (it != refs.end()) return it->second;
    if (chunks > 65535) die("%s: %llu chunks (IdxNum); an index holds at most 65535 per reference", name.c_str(), (unsigned long long)chunks);
    Ref r{(uint32_t)refs.size(), 0, chunks, tlen, counters.size() / kmcpg::REFSTATS_WORDS};
    if (level_species) {
      auto t = tmap.ids.find(name);
      if (t == tmap.ids.end()) die("unknown taxid for %s, please check taxid mapping file(s)", name.c_str());
      r.species_class = tax.species_of(t->second);
    }
    counters.resize(counters.size() + (size_t)chunks * kmcpg::REFSTATS_WORDS, 0);
    return refs.emplace(name, r).first->second;
  };

  uint64_t matched = 0, unique = 0;
  kmcpg::RefstatsCut cut;
  cut.keep_perfect = keep_perfect, cut.keep_main = keep_main, cut.max_gap = max_gap, cut.top_n = (int)std::min<long>(top_n, INT32_MAX);
  for (const std::string& file : files) {
    RawLines in(file);
    std::string query;  // the name of the previous row that passed -t / -f
    bool any = false;
    std::vector<kmcpg::RefstatsRow> rows;  // the current query's kept rows
    auto flush = [&] {
      if (rows.empty()) return;
      matched++;
      if (kmcpg::refstats_count_query(rows.data(), rows.size(), level_species, H, [&](uint64_t col, int w) { counters[col * kmcpg::REFSTATS_WORDS + w]++; })) unique++;
      rows.clear();
    };
    const char* p = nullptr;
    size_t n = 0;
    while (in.next(&p, &n)) {
      Fields fl;
      double qcov = 0;
      if (!parse_row(p, n, min_qcov, max_fpr, &fl, &qcov)) continue;
      const size_t* tab = fl.tab;
      auto field = [&](int k, const char** fp) { return fl.get(k, fp); };
      const char* fp;
      size_t fn;
      uint64_t v[12] = {};
      bool neg[12] = {};
      static const struct {
        int k;
        const char* what;
      } ints[] = {{2, "qLen"}, {3, "qKmers"}, {5, "hits"}, {7, "chunkIdx"}, {8, "IdxNum"}, {9, "genomeSize"}, {10, "K"}, {11, "mKmers"}};
      for (const auto& f : ints) {
        fn = field(f.k, &fp);
        if (!parse_int(fp, fn, f.k != 9, &v[f.k], &neg[f.k])) die("failed to parse %s: %.*s", f.what, (int)fn, fp);
      }
      const bool first = !any || query.size() != tab[0] || memcmp(query.data(), p, tab[0]) != 0;
      if (first) {
        flush();
        query.assign(p, tab[0]);
        any = true;
      }
      if (!cut.keep(first, qcov)) continue;
      fn = field(6, &fp);
      const uint64_t chunks = neg[8] ? 0 : v[8];
      const Ref& r = ref_of(fp, fn, chunks, v[9]);
      if (neg[7] || v[7] >= r.chunks) die("chunkIdx %s%llu of %.*s is outside its %llu chunks", neg[7] ? "-" : "", (unsigned long long)v[7], (int)fn, fp, (unsigned long long)r.chunks);
      rows.push_back(kmcpg::RefstatsRow{r.target_class, r.species_class, r.base + v[7], qcov});
    }
    flush();
  }

  // the verdicts: what the output prints, and stage 2's set of kept references
  for (auto& kv : refs) {
    Ref& r = kv.second;
    const uint64_t* w = counters.data() + r.base * kmcpg::REFSTATS_WORDS;
    const kmcpg::RefstatsRef t = kmcpg::refstats_rollup(r.chunks, min_frac, [&](uint64_t c) { return w + c * kmcpg::REFSTATS_WORDS; });
    r.ok = t.verdict == kmcpg::REFSTATS_OK, r.reads = t.reads, r.ureads = t.ureads;
  }

  // stage 2/4 (profile.go:1117-1279): the inputs once more; a query's targets are a set (chunks of one reference are one target)
  std::unordered_map<uint64_t, uint64_t> shared;  // cooccur_key of two target classes -> queries
  if (!cooccur_file.empty() || stage3) {
    kmcpg::CooccurCut cut2;
    cut2.cut = cut;
    for (const std::string& file : files) {
      RawLines in(file);
      std::string query;  // the name of the previous row that was not skipped
      bool any = false;
      std::vector<uint32_t> cls;  // the current query's targets
      auto flush = [&] {
        kmcpg::cooccur_query_pairs(cls.data(), cls.size(), [&](uint64_t key) { shared[key]++; });
        cls.clear();
      };
      const char* p = nullptr;
      size_t n = 0;
      while (in.next(&p, &n)) {
        Fields fl;
        double qcov = 0;
        if (!parse_row(p, n, min_qcov, max_fpr, &fl, &qcov)) continue;
        const char* fp;
        const size_t fn = fl.get(6, &fp);
        name.assign(fp, fn);
        const auto it = refs.find(name);
        const bool kept = it != refs.end() && it->second.ok;
        const bool new_name = !any || query.size() != fl.tab[0] || memcmp(query.data(), p, fl.tab[0]) != 0;
        bool opens = false;
        const bool take = cut2.row(kept, new_name, qcov, &opens);
        if (!kept) continue;
        if (opens) flush();
        query.assign(p, fl.tab[0]);
        any = true;
        if (take) cls.push_back(it->second.target_class);
      }
      flush();
    }
  }

  // stage 3/4 (profile.go:1282-1888): the inputs a third time; the kept rows are stage 2's, the rest is recount_rule.hpp
  std::vector<uint64_t> recounted;  // RECOUNT_WORDS per column, laid out as `counters`
  uint64_t n_recounted = 0, n_unique3 = 0, n_corrected = 0;
  if (stage3) {
    recounted.assign(counters.size() / kmcpg::REFSTATS_WORDS * kmcpg::RECOUNT_WORDS, 0);
    std::vector<kmcpg::RecountClass> classes(refs.size());
    for (const auto& kv : refs) classes[kv.second.target_class] = kmcpg::RecountClass{kv.second.ok ? 1u : 0u, kv.second.reads, kv.second.ureads};
    kmcpg::RecountParams rp;
    rp.one_minus_d = 1 - flag_D, rp.r_err = flag_R, rp.hic_min_qcov = H, rp.no_amb_corr = no_amb_corr, rp.level_species = level_species;
    kmcpg::CooccurCut cut3;
    cut3.cut = cut;
    for (const std::string& file : files) {
      RawLines in(file);
      std::string query;  // the name of the previous row that was not skipped
      bool any = false;
      std::vector<kmcpg::RecountRow> rows;  // the current query's kept rows
      auto flush = [&] {
        if (rows.empty()) return;
        bool lost = false;
        const size_t ns = kmcpg::recount_query(
            rows.data(), rows.size(), classes.data(), rp,
            [&](uint32_t a, uint32_t b) {
              const auto it = shared.find(kmcpg::cooccur_key(a, b));
              return it == shared.end() ? (uint64_t)0 : it->second;
            },
            [&](uint64_t col, int w, uint64_t n) { recounted[col * kmcpg::RECOUNT_WORDS + w] += n; }, &lost);
        n_recounted++;
        if (ns == 1) n_unique3++;
        if (lost) n_corrected++;
        rows.clear();
      };
      const char* p = nullptr;
      size_t n = 0;
      while (in.next(&p, &n)) {
        Fields fl;
        double qcov = 0;
        if (!parse_row(p, n, min_qcov, max_fpr, &fl, &qcov)) continue;
        const char* fp;
        size_t fn = fl.get(6, &fp);
        name.assign(fp, fn);
        const auto it = refs.find(name);
        const bool kept = it != refs.end() && it->second.ok;
        const bool new_name = !any || query.size() != fl.tab[0] || memcmp(query.data(), p, fl.tab[0]) != 0;
        bool opens = false;
        const bool take = cut3.row(kept, new_name, qcov, &opens);
        if (!kept) continue;
        if (opens) flush();
        query.assign(p, fl.tab[0]);
        any = true;
        if (!take) continue;
        uint64_t qlen = 0, chunk_idx = 0;  // (both parsed and range-checked by stage 1: a kept target's rows all passed it)
        bool neg = false;
        fn = fl.get(2, &fp);
        if (!parse_int(fp, fn, true, &qlen, &neg) || neg) qlen = 0;
        fn = fl.get(7, &fp);
        if (!parse_int(fp, fn, true, &chunk_idx, &neg) || neg || chunk_idx >= it->second.chunks) die("chunkIdx of %s is outside its chunks", name.c_str());
        rows.push_back(kmcpg::RecountRow{it->second.target_class, it->second.species_class, it->second.base + chunk_idx, qcov, qlen});
      }
      flush();
    }
  }

  // stage 4/4 (profile.go:1907-2570): the rows of the references stage 3 lists as ok, kept in memory; a pass is em_rule.hpp over them
  std::vector<kmcpg::EmClass> em_classes;
  kmcpg::EmResult em_res;
  std::vector<uint32_t> em_order;
  if (!profile_file.empty()) {
    const size_t n_cols = counters.size() / kmcpg::REFSTATS_WORDS;
    em_classes.resize(refs.size());
    std::vector<uint8_t> est(refs.size(), 0);
    std::vector<double> cov(refs.size(), 0.0);
    for (const auto& kv : refs) {
      const Ref& r = kv.second;
      kmcpg::EmClass& c = em_classes[r.target_class];
      c.name = kv.first, c.tlen = r.tlen;
      for (uint64_t k = 0; k < r.chunks; k++) c.columns.push_back(r.base + k);
      const uint64_t* w = recounted.data() + r.base * kmcpg::RECOUNT_WORDS;
      const kmcpg::RecountRef t = kmcpg::recount_rollup(r.chunks, r.tlen, th, [&](uint64_t k) { return w + k * kmcpg::RECOUNT_WORDS; });
      est[r.target_class] = kmcpg::em_start(t, &cov[r.target_class]) ? 1 : 0;
    }
    // the log: every row of a reference on the first whitelist that passed -t / -f, with the name of its query (per file) and whether the
    // rows of its run of equal query names — all of them, whatever their reference — name ONE target (em_rule.hpp: such a read is
    // counted by K8's single rule)
    struct LogRow {
      kmcpg::RecountRow row;
      uint32_t file, query;
      bool run_single;
    };
    std::vector<LogRow> log;
    {
      std::unordered_map<std::string, uint32_t> query_ids;
      std::string qname, first_target;
      for (size_t fi = 0; fi < files.size(); fi++) {
        RawLines in(files[fi]);
        query_ids.clear();
        std::string run;  // the query name of the previous row that passed -t / -f
        bool any = false, single = true;
        size_t run_from = log.size();
        auto end_run = [&] {
          for (size_t i = run_from; i < log.size(); i++) log[i].run_single = single;
          run_from = log.size(), single = true;
        };
        const char* p = nullptr;
        size_t n = 0;
        while (in.next(&p, &n)) {
          Fields fl;
          double qcov = 0;
          if (!parse_row(p, n, min_qcov, max_fpr, &fl, &qcov)) continue;
          const char* fp;
          size_t fn = fl.get(6, &fp);
          name.assign(fp, fn);
          if (!any || run.size() != fl.tab[0] || memcmp(run.data(), p, fl.tab[0]) != 0) {
            end_run();
            run.assign(p, fl.tab[0]), any = true, first_target = name;
          } else if (name != first_target) single = false;
          const auto it = refs.find(name);
          if (it == refs.end() || !est[it->second.target_class]) continue;
          uint64_t qlen = 0, chunk_idx = 0;
          bool neg = false;
          fn = fl.get(2, &fp);
          if (!parse_int(fp, fn, true, &qlen, &neg) || neg) qlen = 0;
          fn = fl.get(7, &fp);
          if (!parse_int(fp, fn, true, &chunk_idx, &neg) || neg || chunk_idx >= it->second.chunks) die("chunkIdx of %s is outside its chunks", name.c_str());
          const uint32_t q = query_ids.emplace(run, (uint32_t)query_ids.size()).first->second;
          log.push_back(LogRow{kmcpg::RecountRow{it->second.target_class, it->second.species_class, it->second.base + chunk_idx, qcov, qlen}, (uint32_t)fi, q, false});
        }
        end_run();
      }
    }
    kmcpg::EmParams ep;
    ep.th = th, ep.max_iters = (int)std::min<long>(max_iters, INT32_MAX - 1), ep.pct_threshold = pct_threshold;
    const auto pass = [&](const std::vector<uint8_t>& e, const std::vector<double>& cv, std::vector<kmcpg::EmChunk>* cols, uint64_t* assigned) {
      cols->assign(n_cols, kmcpg::EmChunk());
      *assigned = 0;
      kmcpg::CooccurCut cut4;
      cut4.cut = cut;
      std::vector<kmcpg::RecountRow> rows;
      bool single = true, any = false;
      uint32_t file = 0, query = 0;
      auto flush = [&] {
        if (rows.empty()) return;
        (*assigned)++;
        if (single) {  // one target in the whole table: K8's single rule, in its units
          const uint64_t m = rows.size();
          for (size_t i = 0; i < rows.size(); i++) {
            kmcpg::EmChunk& w = (*cols)[rows[i].column];
            const uint64_t u = i == 0 ? kmcpg::EM_UNIT : 0;
            w.match += kmcpg::em_single_share(m, i == 0), w.uniq += u, w.hic += rows[i].qcov >= H ? u : 0;
            w.single_bases += kmcpg::recount_bases(rows[i].qlen, 1, m);
          }
        } else {
          kmcpg::em_query(rows.data(), rows.size(), cv.data(), H, level_species, [&](uint64_t col, int w, uint64_t x) {
            kmcpg::EmChunk& c = (*cols)[col];
            (w == kmcpg::EM_MATCH ? c.match : w == kmcpg::EM_UNIQ ? c.uniq : w == kmcpg::EM_HIC ? c.hic : w == kmcpg::EM_BASES_LO ? c.bases_lo : c.bases_hi) += x;
          });
        }
        rows.clear();
      };
      for (const LogRow& l : log) {
        const bool kept = e[l.row.target_class] != 0;
        const bool new_name = !any || l.file != file || l.query != query;
        if (any && l.file != file) flush(), any = false, cut4 = kmcpg::CooccurCut{cut};  // (a file ends its last query)
        bool opens = false;
        const bool take = cut4.row(kept, new_name, l.row.qcov, &opens);
        if (!kept) continue;
        if (opens) flush(), single = true;
        file = l.file, query = l.query, any = true;
        if (!take) continue;
        single = single && l.run_single;
        rows.push_back(l.row);
      }
      flush();
      return 0;
    };
    if (kmcpg::em_run(em_classes, est, cov, ep, pass, &em_res) != 0) die("the EM loop failed");
    em_order = kmcpg::em_finish(em_classes, filter_low_pct, &em_res);
  }

  // the binning pass (profile.go:2591-2784): the inputs once more, over the references the EM ended with — refused before a file is written
  kmcpg::BinPlan bin_plan;
  if (!binning_file.empty()) {
    std::vector<std::string> whitelist;
    for (size_t c = 0; c < em_classes.size(); c++)
      if (c < em_res.est.size() && em_res.est[c]) whitelist.push_back(em_classes[c].name);
    std::sort(whitelist.begin(), whitelist.end());  // (the refusal names the first in byte order, whatever numbered the references)
    std::string missing;
    if (!kmcpg::bin_plan_build(tax, tmap, whitelist, &bin_plan, &missing)) die("unknown taxid for %s, please check taxid mapping file(s)", missing.c_str());
  }

  Out out(out_file, -1);
  char line[256];
  out.write(line, (size_t)snprintf(line, sizeof line, "# matched reads: %llu\n# unique reads: %llu\n", (unsigned long long)matched, (unsigned long long)unique));
  out.write("#ref\tchunks\ttLen\treads\tureads\thicUreads\tchunksFrac\tverdict\tchunkReads\tchunkFirsts\tchunkUreads\tchunkHicUreads\n");
  std::vector<const std::pair<const std::string, Ref>*> order;
  for (const auto& kv : refs) order.push_back(&kv);
  std::sort(order.begin(), order.end(), [](auto* a, auto* b) { return a->first < b->first; });
  std::string s;
  for (const auto* kv : order) {
    const Ref& r = kv->second;
    const uint64_t* w = counters.data() + r.base * kmcpg::REFSTATS_WORDS;
    const kmcpg::RefstatsRef t = kmcpg::refstats_rollup(r.chunks, min_frac, [&](uint64_t c) { return w + c * kmcpg::REFSTATS_WORDS; });
    s = kv->first;
    s.append(line, (size_t)snprintf(line, sizeof line, "\t%llu\t%llu\t%llu\t%llu\t%llu\t%.4f\t%s", (unsigned long long)r.chunks, (unsigned long long)r.tlen,
                                    (unsigned long long)t.reads, (unsigned long long)t.ureads, (unsigned long long)t.hic_ureads, t.chunks_frac,
                                    kmcpg::refstats_verdict_name(t.verdict)));
    for (int j = 0; j < kmcpg::REFSTATS_WORDS; j++)
      for (uint64_t c = 0; c < r.chunks; c++) {
        s.push_back(c ? ',' : '\t');
        s += std::to_string(w[c * kmcpg::REFSTATS_WORDS + j]);
      }
    s.push_back('\n');
    out.write(s);
  }
  out.close();

  if (!recount_file.empty()) {
    std::vector<recount_format::Ref> list;
    for (const auto& kv : refs) list.push_back(recount_format::Ref{&kv.first, kv.second.chunks, kv.second.tlen, recounted.data() + kv.second.base * kmcpg::RECOUNT_WORDS});
    Out rc(recount_file, -1);
    recount_format::write(rc, list, n_recounted, n_unique3, n_corrected, th);
    rc.close();
  }

  if (!profile_file.empty()) {
    Out pf(profile_file, -1);
    profile_format::write(pf, em_classes, em_res, em_order);
    pf.close();
  }

  if (!binning_file.empty()) {
    Out bf(binning_file, -1);
    binning_format::write_header(bf, sample_id);
    kmcpg::BinAcc acc;
    acc.cut = cut;
    for (const std::string& file : files) {
      RawLines in(file);
      std::string query;  // the name of the previous whitelisted row that passed -t / -f
      bool any = false;
      auto flush = [&] {
        const uint32_t bin = any ? acc.bin(bin_plan) : kmcpg::BIN_NONE;
        if (bin != kmcpg::BIN_NONE) binning_format::write_line(bf, query.data(), query.size(), bin);
      };
      const char* p = nullptr;
      size_t n = 0;
      while (in.next(&p, &n)) {
        Fields fl;
        double qcov = 0;
        if (!parse_row(p, n, min_qcov, max_fpr, &fl, &qcov)) continue;
        const char* fp;
        const size_t fn = fl.get(6, &fp);
        name.assign(fp, fn);
        const uint32_t node = bin_plan.node_of(name);
        if (node == kmcpg::BIN_NO_NODE) continue;  // skipped before anything else: it neither opens a query nor is its first row
        if (!any || query.size() != fl.tab[0] || memcmp(query.data(), p, fl.tab[0]) != 0) {
          flush();
          query.assign(p, fl.tab[0]);
          any = true;
          acc.begin();
        }
        acc.row(node, qcov);
      }
      flush();
    }
    bf.close();
  }

  if (!cooccur_file.empty()) {
    std::vector<const std::string*> name_of(refs.size());
    for (const auto& kv : refs) name_of[kv.second.target_class] = &kv.first;
    std::vector<std::pair<std::pair<const std::string*, const std::string*>, uint64_t>> rows;
    for (const auto& kv : shared) {
      const std::string *a = name_of[kmcpg::cooccur_key_a(kv.first)], *b = name_of[kmcpg::cooccur_key_b(kv.first)];
      if (*b < *a) std::swap(a, b);
      rows.push_back({{a, b}, kv.second});
    }
    std::sort(rows.begin(), rows.end(), [](const auto& x, const auto& y) { return *x.first.first != *y.first.first ? *x.first.first < *y.first.first : *x.first.second < *y.first.second; });
    Out co(cooccur_file, -1);
    co.write(line, (size_t)snprintf(line, sizeof line, "# pairs: %zu\n", rows.size()));
    co.write("#refA\trefB\treads\n");
    for (const auto& r : rows) {
      s = *r.first.first + "\t" + *r.first.second + "\t" + std::to_string(r.second) + "\n";
      co.write(s);
    }
    co.close();
  }
  return 0;
}
