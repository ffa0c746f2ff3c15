// kmcp-regions: merge the species- / assembly-specific windows of a genome into regions, BED6 out — host-side mirror of
// `kmcp utils merge-regions` (kmcp/cmd/merge-regions.go, row parser util-regions.go).  Host only, no GPU.
//
//   kmcp-regions [-o out.bed[.gz]] [-f 0.05] [-t 0.55] [-l 1] [-g 0] [-I] [-r regexp] [-s species-specific] [-a assembly-specific]
//                [-i list.txt] [filtered.tsv[.gz] ...]
//
// The input is what kmcp-filter leaves of a search of sliding windows (queries named REF_sliding:BEGIN-END).  The rule — rows, queries,
// a window's summary, merging, and the three deliberate differences to the reference — is kmcp_amd/csrc/regions_rule.hpp.  The state is
// reset per input file and the outputs are concatenated.
//
// -r: the default pattern is matched by a hand-written parser; any other pattern goes through std::regex, whose grammar is ECMAScript,
// not the reference's RE2 (the common subset — classes, groups, greedy and lazy repeats, anchors — reads the same; RE2-only syntax such
// as (?P<name>...) or \pL is refused or read differently).  The first match's groups 1, 2 and 3 are the reference name, begin and end.
#include <unistd.h>

#include <cstdint>
#include <fstream>
#include <regex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../kmcp_amd/csrc/regions_rule.hpp"
#include "tsv_in.hpp"
#include "tsv_out.hpp"

namespace {

using tsv_in::parse_float;
using tsv_in::RawLines;
using tsv_out::die;
using tsv_out::Out;

const char DEFAULT_PATTERN[] = "^(.+)_sliding:(\\d+)\\-(\\d+)$";

void usage() {
  fputs(
      "Merge species/assembly-specific regions\n\n"
      "Usage:\n  kmcp-regions [flags] [<filtered search results> ...]\n\n"
      "Flags:\n"
      "  -o, --out-file string        Out file (BED6), supports a \".gz\" suffix (\"-\" for stdout). (default \"-\")\n"
      "  -f, --max-fpr float          Maximum false positive rate of a read in search result. (default 0.05)\n"
      "  -t, --min-query-cov float    Minimum query coverage of a read in search result. (default 0.55)\n"
      "  -g, --max-gap int            Maximum distance of starting positions of two adjacent regions, 0 for no limitation, 1 for no merging.\n"
      "  -l, --min-overlap int        Minimum overlap of two adjacent regions, recommend K-1. (default 1)\n"
      "  -I, --ignore-type            Merge species and assembly-specific regions.\n"
      "  -r, --regexp string          Regular expression (ECMAScript grammar) for extract reference name and query locations.\n"
      "                               (default \"^(.+)_sliding:(\\d+)\\-(\\d+)$\")\n"
      "  -s, --name-species string    Name of species-specific regions. (default \"species-specific\")\n"
      "  -a, --name-assembly string   Name of assembly-specific regions. (default \"assembly-specific\")\n"
      "      --line-chunk-size int    Accepted for command-line compatibility. (default 5000)\n"
      "  -i, --infile-list string     File of input files list (one file per line).\n",
      stderr);
}

// strconv.Atoi with its error thrown away, as the reference does: digits with an optional sign, else 0; out of range saturates
int64_t atoi_go(const std::string& s) {
  if (s.empty()) return 0;
  size_t i = s[0] == '-' || s[0] == '+' ? 1 : 0;
  if (i == s.size()) return 0;
  uint64_t x = 0;
  bool sat = false;
  for (; i < s.size(); i++) {
    if (s[i] < '0' || s[i] > '9') return 0;
    if (x > (0x7fffffffffffffffULL - 9) / 10) sat = true;
    else x = x * 10 + (uint64_t)(s[i] - '0');
  }
  if (sat) return s[0] == '-' ? INT64_MIN : INT64_MAX;
  return s[0] == '-' ? -(int64_t)x : (int64_t)x;
}

}  // namespace

int main(int argc, char** argv) {
  std::string out_file = "-", infile_list, pattern = DEFAULT_PATTERN;
  std::vector<std::string> files;
  double max_fpr = 0.05, min_qcov = 0.55;
  long chunk = 5000;
  kmcpg::RegionParams rp;
  auto need = [&](int& i) -> const char* {
    if (i + 1 >= argc) die("flag needs an argument: %s", argv[i]);
    return argv[++i];
  };
  auto num = [&](const char* flag, const char* v) {
    double x = 0;
    if (!parse_float(v, strlen(v), &x)) die("invalid argument \"%s\" for \"%s\" flag", v, flag);
    return x;
  };
  auto whole = [&](const char* flag, const char* v) {
    char* e = nullptr;
    errno = 0;
    const long long x = strtoll(v, &e, 10);
    if (e == v || *e || errno) die("invalid argument \"%s\" for \"%s\" flag", v, flag);
    return (int64_t)x;
  };
  // `kmcp-regions merge-regions ...` = `kmcp utils merge-regions ...`: cobra's sub-command word, accepted (only) as the first argument
  for (int i = (argc > 1 && strcmp(argv[1], "merge-regions") == 0) ? 2 : 1; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "-o" || a == "--out-file") out_file = need(i);
    else if (a == "-f" || a == "--max-fpr") max_fpr = num("-f, --max-fpr", need(i));
    else if (a == "-t" || a == "--min-query-cov") min_qcov = num("-t, --min-query-cov", need(i));
    else if (a == "-g" || a == "--max-gap") rp.max_gap = whole("-g, --max-gap", need(i));
    else if (a == "-l" || a == "--min-overlap") rp.min_overlap = whole("-l, --min-overlap", need(i));
    else if (a == "-I" || a == "--ignore-type") rp.ignore_type = true;
    else if (a == "-r" || a == "--regexp") pattern = need(i);
    else if (a == "-s" || a == "--name-species") rp.name_species = need(i);
    else if (a == "-a" || a == "--name-assembly") rp.name_assembly = need(i);
    else if (a == "--line-chunk-size") chunk = (long)whole("--line-chunk-size", need(i));
    else if (a == "-i" || a == "--infile-list") infile_list = need(i);
    else if (a == "-j" || a == "--threads" || a == "--log") need(i);  // accepted for command-line compatibility
    else if (a == "-q" || a == "--quiet") {
    } else if (a == "-h" || a == "--help") {
      usage();
      return 0;
    } else if (a.size() > 1 && a[0] == '-') die("unknown flag: %s", a.c_str());
    else files.push_back(a);
  }
  // merge-regions.go:98-118, in its order
  if (max_fpr <= 0) die("value of flag --max-fpr should be greater than 0");
  if (min_qcov < 0) die("value of flag --min-query-cov should be greater than or equal to ");
  if (chunk <= 0) die("value of flag --line-chunk-size should be greater than 0");
  if (rp.max_gap < 0) die("value of flag --max-gap should be greater than or equal to 0");
  if (rp.min_overlap <= 0) die("value of flag --min-overlap should be greater than 0");
  if (rp.min_overlap == 1) fputs("[WARN] you may set -l/--min-overlap as k-1, where k is the k-mer size\n", stderr);
  const bool by_hand = pattern == DEFAULT_PATTERN;
  std::regex re;
  if (!by_hand) {
    try {
      re.assign(pattern, std::regex::ECMAScript);
    } catch (const std::regex_error& e) {
      die("error parsing regexp: %s: `%s`", e.what(), pattern.c_str());
    }
    if (re.mark_count() < 3) die("the regular expression needs three groups (reference name, begin, end): `%s`", pattern.c_str());
  }

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

  Out out(out_file, -1);
  kmcpg::RegionMerger merger(rp);
  std::string bed;
  std::unordered_map<std::string, uint32_t> target_ids;  // target name -> its class: equal strings, equal class
  std::string key;
  for (const std::string& file : files) {
    RawLines in(file);
    // the current query: its name, where the pattern found it, and its summary so far
    std::string query, ref;
    int64_t begin = 0, end = 0;
    kmcpg::WindowSummaryAcc acc;
    auto flush = [&] {
      if (acc.n == 0) return;
      merger.add(ref.data(), ref.size(), begin, end, acc.n, acc.score(), &bed);
      acc.clear();
      if (bed.size() > (1u << 16)) {
        out.write(bed);
        bed.clear();
      }
    };
    const char* p = nullptr;
    size_t n = 0;
    while (in.next(&p, &n)) {
      kmcpg::RegionRowFields f{};
      switch (kmcpg::region_row(p, n, max_fpr, min_qcov, parse_float, &f)) {
        case kmcpg::REGION_ROW_SKIP:
        case kmcpg::REGION_ROW_DROPPED: continue;
        case kmcpg::REGION_ROW_FEW_FIELDS: die("invalid kmcp search result format");
        case kmcpg::REGION_ROW_BAD_FPR: die("failed to parse FPR: %.*s", (int)f.bad_n, f.bad);
        case kmcpg::REGION_ROW_BAD_QCOV: die("failed to parse qCov: %.*s", (int)f.bad_n, f.bad);
        case kmcpg::REGION_ROW_KEPT: break;
      }
      // (the reference matches every kept row's name; the rows of one query share the name, so once per query decides the same)
      if (acc.n == 0 || query.size() != f.query_n || memcmp(query.data(), f.query, f.query_n) != 0) {
        flush();
        query.assign(f.query, f.query_n);
        if (by_hand) {
          size_t ref_n = 0;
          if (!kmcpg::region_default_name(f.query, f.query_n, &ref_n, &begin, &end)) die("no reference and location found in the query name");
          ref.assign(f.query, ref_n);
        } else {
          std::smatch m;
          if (!std::regex_search(query, m, re)) die("no reference and location found in the query name");
          ref = m[1].str();
          begin = atoi_go(m[2].str());
          end = atoi_go(m[3].str());
        }
      }
      key.assign(f.target, f.target_n);
      const uint32_t cls = target_ids.emplace(key, (uint32_t)target_ids.size()).first->second;
      acc.add(cls, f.qcov);
    }
    flush();
    merger.finish(&bed);
    out.write(bed);
    bed.clear();
  }
  out.close();
  return 0;
}
