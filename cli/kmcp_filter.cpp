// kmcp-filter: keep the queries of a search result whose matches point at one target or one species — host-side mirror of
// `kmcp utils filter` (kmcp/cmd/filter.go:57-399, row parser util-filter.go:46-82).  Host only, no GPU.
//
//   kmcp-filter [-o out.tsv[.gz]] [-H] [-f 0.05] [-t 0.55] [--level species|strain|assembly] [-T map.tsv[,more.tsv]]... [-X taxdump/]
//               [-i list.txt] [a.tsv[.gz] ...]
//
// Semantics restated from the reference:
//   * blank lines and every line that starts with '#' are dropped; the header row is written anew unless -H;
//   * a row is cut at its first 12 tabs (fewer than 13 fields is fatal); FPR (field 4) is parsed and the row dropped when it is above
//     -f, THEN qCov (field 12) is parsed and the row dropped when it is below -t;
//   * the remaining rows of consecutive equal query names form a query (per input file); it is kept when its rows name one target, or,
//     at --level species, when its targets lie under one species (kmcp_amd/csrc/specific_rule.hpp: the rule and why it equals the
//     reference's "LCA at or below rank species"); kept rows are written verbatim;
//   * at --level species a target without a TaxId is fatal.
// Where the reference is nondeterministic (it walks a Go map of the query's targets) this tool is deterministic: kept rows stay in
// input order.
#include <unistd.h>
#include <zlib.h>

#include <cstdint>
#include <fstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../kmcp_amd/csrc/specific_rule.hpp"
#include "../kmcp_amd/csrc/taxonomy.hpp"
#include "tsv_in.hpp"
#include "tsv_out.hpp"

namespace {

using tsv_in::parse_float;
using tsv_in::RawLines;
using tsv_out::die;
using tsv_out::Out;

void usage() {
  fputs(
      "Filter search results and find species/assembly-specific queries\n\n"
      "Usage:\n  kmcp-filter [flags] [<search results> ...]\n\n"
      "Flags:\n"
      "  -H, --no-header-row         Do not print header row.\n"
      "  -o, --out-file string       Out file, supports a \".gz\" suffix (\"-\" for stdout). (default \"-\")\n"
      "  -f, --max-fpr float         Maximum false positive rate of a read in search result. (default 0.05)\n"
      "  -t, --min-query-cov float   Minimum query coverage of a read in search result. (default 0.55)\n"
      "  -T, --taxid-map strings     Tabular two-column file(s) mapping reference IDs to TaxIds.\n"
      "  -X, --taxdump string        Directory of NCBI taxonomy dump files: nodes.dmp, optional with merged.dmp and delnodes.dmp.\n"
      "      --level string          Level to filter. available values: species, strain/assembly. (default \"species\")\n"
      "      --line-chunk-size int   Accepted for command-line compatibility. (default 5000)\n"
      "  -i, --infile-list string    File of input files list (one file per line).\n",
      stderr);
}

}  // namespace

int main(int argc, char** argv) {
  std::string out_file = "-", level = "species", taxdump, infile_list;
  std::vector<std::string> map_files, files;
  double max_fpr = 0.05, min_qcov = 0.55;
  long chunk = 5000;
  bool no_header = false;
  auto need = [&](int& i) -> const char* {
    if (i + 1 >= argc) die("flag needs an argument: %s", argv[i]);
    return argv[++i];
  };
  auto num = [&](const char* flag, const char* v) {
    double x = 0;
    if (!parse_float(v, strlen(v), &x)) die("invalid argument \"%s\" for \"%s\" flag", v, flag);
    return x;
  };
  // `kmcp-filter filter ...` = `kmcp utils filter ...`: cobra's sub-command word, accepted (only) as the first argument
  for (int i = (argc > 1 && strcmp(argv[1], "filter") == 0) ? 2 : 1; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "-o" || a == "--out-file") out_file = need(i);
    else if (a == "-H" || a == "--no-header-row") no_header = true;
    else if (a == "-f" || a == "--max-fpr") max_fpr = num("-f, --max-fpr", need(i));
    else if (a == "-t" || a == "--min-query-cov") min_qcov = num("-t, --min-query-cov", need(i));
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
    else if (a == "--line-chunk-size") chunk = (long)num("--line-chunk-size", need(i));
    else if (a == "-i" || a == "--infile-list") infile_list = need(i);
    else if (a == "-j" || a == "--threads" || a == "--log") need(i);  // accepted for command-line compatibility
    else if (a == "-q" || a == "--quiet") {
    } else if (a == "-h" || a == "--help") {
      usage();
      return 0;
    } else if (a.size() > 1 && a[0] == '-') die("unknown flag: %s", a.c_str());
    else files.push_back(a);
  }
  // filter.go:82-114, in its order
  if (max_fpr <= 0) die("value of flag --max-fpr should be greater than 0");
  if (min_qcov < 0) die("value of flag --min-query-cov should be greater than or equal to ");
  for (char& c : level) c = (char)tolower((unsigned char)c);
  bool level_species = false;
  if (level == "species") level_species = true;
  else if (level != "strain" && level != "assembly") die("invalid value for --level, available values: species, strain/assembly");
  if (!map_files.empty() && taxdump.empty()) die("flag -X/--taxdump is needed when -T/--taxid-map given");
  if (map_files.empty() && !taxdump.empty()) die("flag -T/--taxid-map is needed when -X/--taxdump given");
  if ((map_files.empty() || taxdump.empty()) && level_species) die("TaxID mapping files (-T/--taxid-map) and taxonomy dump files are needed for --level species");
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

  kmcpg::TaxidMap tmap;
  kmcpg::Taxonomy tax;
  const bool mapping = !map_files.empty();
  if (mapping) {
    std::string err;
    for (const std::string& f : map_files)
      if (!tmap.load(f, &err)) die("%s", err.c_str());
    if (tmap.ids.empty()) {
      std::string all;
      for (const std::string& f : map_files) all += (all.empty() ? "" : ", ") + f;
      die("no valid TaxIds found in TaxId mapping file: %s", all.c_str());
    }
    if (!tax.load(taxdump, &err)) die("%s", err.c_str());
    uint64_t unknown = 0;
    std::unordered_map<uint32_t, bool> seen;
    for (const auto& kv : tmap.ids)
      if (seen.emplace(kv.second, true).second && !tax.known(kv.second)) unknown++;
    if (unknown) fprintf(stderr, "[WARN] %llu TaxId(s) of the mapping file(s) are deleted or not in nodes.dmp: they belong to no species\n", (unsigned long long)unknown);
  }

  Out out(out_file, -1);
  if (!no_header) out.write("#query\tqLen\tqKmers\tFPR\thits\ttarget\tchunkIdx\tchunks\ttLen\tkSize\tmKmers\tqCov\ttCov\tjacc\tqueryIdx\n");

  // target name -> (target_class, species_class), filled as targets are met
  struct Classes {
    uint32_t target, species;
  };
  std::unordered_map<std::string, Classes> classes;
  std::string name;
  auto classes_of = [&](const char* p, size_t n) -> const Classes& {
    name.assign(p, n);
    auto it = classes.find(name);
    if (it != classes.end()) return it->second;
    Classes c{(uint32_t)classes.size(), 0};
    if (level_species) {
      auto t = tmap.ids.find(name);
      if (t == tmap.ids.end()) die("unknown taxid for %s, please check taxid mapping file(s)", name.c_str());
      c.species = tax.species_of(t->second);
    }
    return classes.emplace(name, c).first->second;
  };

  for (const std::string& file : files) {
    RawLines in(file);
    std::string query, rows;  // the current query: its name and its surviving rows, verbatim
    kmcpg::SpecificAcc acc;
    auto flush = [&] {
      if (acc.n == 0) return;
      if (kmcpg::specific_keep(acc, level_species)) out.write(rows);
      rows.clear();
      acc = kmcpg::SpecificAcc();
    };
    const char* p = nullptr;
    size_t n = 0;
    while (in.next(&p, &n)) {
      size_t len = n;  // without the end of line
      if (len && p[len - 1] == '\n') len--;
      if (len && p[len - 1] == '\r') len--;
      if (len == 0 || p[0] == '#') continue;
      size_t tab[12];
      int nt = 0;
      for (size_t i = 0; i < len && nt < 12; i++)
        if (p[i] == '\t') tab[nt++] = i;
      if (nt < 12) die("invalid kmcp search result format");
      double fpr = 0, qcov = 0;
      if (!parse_float(p + tab[2] + 1, tab[3] - tab[2] - 1, &fpr)) die("failed to parse FPR: %.*s", (int)(tab[3] - tab[2] - 1), p + tab[2] + 1);
      if (fpr > max_fpr) continue;
      if (!parse_float(p + tab[10] + 1, tab[11] - tab[10] - 1, &qcov)) die("failed to parse qCov: %.*s", (int)(tab[11] - tab[10] - 1), p + tab[10] + 1);
      if (qcov < min_qcov) continue;
      if (acc.n == 0 || query.size() != tab[0] || memcmp(query.data(), p, tab[0]) != 0) {
        flush();
        query.assign(p, tab[0]);
      }
      const Classes& c = classes_of(p + tab[4] + 1, tab[5] - tab[4] - 1);
      acc.add(c.target, c.species);
      rows.append(p, n);
    }
    flush();
  }
  out.close();
  return 0;
}
