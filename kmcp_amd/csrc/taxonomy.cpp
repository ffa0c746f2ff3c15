// taxonomy.cpp — see taxonomy.hpp.  Host only: no HIP, no library state; compiled into libkmcpgpu.so and into kmcp-filter / kmcp-search.
#include "taxonomy.hpp"

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

namespace kmcpg {

namespace {

// the fields of a .dmp line ("a\t|\tb\t|\tc\t|"): cut at '|', tabs and blanks around a field dropped
void dmp_fields(const std::string& line, std::vector<std::string>* out, size_t want) {
  out->clear();
  size_t at = 0;
  while (out->size() < want && at <= line.size()) {
    size_t bar = line.find('|', at);
    if (bar == std::string::npos) bar = line.size();
    size_t lo = at, hi = bar;
    while (lo < hi && (line[lo] == '\t' || line[lo] == ' ')) lo++;
    while (hi > lo && (line[hi - 1] == '\t' || line[hi - 1] == ' ' || line[hi - 1] == '\r')) hi--;
    out->push_back(line.substr(lo, hi - lo));
    at = bar + 1;
  }
}

bool parse_u32(const std::string& s, uint32_t* v) {
  if (s.empty() || s[0] < '0' || s[0] > '9') return false;  // strconv.ParseUint: digits only, no sign, no blanks
  char* e = nullptr;
  errno = 0;
  const unsigned long long x = strtoull(s.c_str(), &e, 10);
  if (errno || *e || x > 0xffffffffull) return false;
  *v = (uint32_t)x;
  return true;
}

}  // namespace

bool Taxonomy::load(const std::string& dir, std::string* err) {
  nodes.clear();
  merged.clear();
  deleted.clear();
  std::vector<std::string> f;
  std::string line;
  {
    const std::string path = dir + "/nodes.dmp";
    std::ifstream in(path);
    if (!in) {
      *err = "err on loading Taxonomy nodes: open " + path + ": " + strerror(errno);
      return false;
    }
    while (std::getline(in, line)) {
      if (line.empty()) continue;
      dmp_fields(line, &f, 3);
      uint32_t t = 0, p = 0;
      if (f.size() < 3 || !parse_u32(f[0], &t) || !parse_u32(f[1], &p)) {
        *err = "err on loading Taxonomy nodes: invalid line in " + path + ": " + line;
        return false;
      }
      nodes[t] = Node{p, f[2] == "species"};
    }
  }
  {
    std::ifstream in(dir + "/merged.dmp");
    while (in && std::getline(in, line)) {
      dmp_fields(line, &f, 2);
      uint32_t a = 0, b = 0;
      if (f.size() >= 2 && parse_u32(f[0], &a) && parse_u32(f[1], &b)) merged[a] = b;
    }
  }
  {
    std::ifstream in(dir + "/delnodes.dmp");
    while (in && std::getline(in, line)) {
      dmp_fields(line, &f, 1);
      uint32_t a = 0;
      if (!f.empty() && parse_u32(f[0], &a)) deleted.insert(a);
    }
  }
  return true;
}

uint32_t Taxonomy::resolve(uint32_t taxid) const {
  for (int hop = 0; hop < 64; hop++) {  // (a chain longer than that is a loop)
    auto it = merged.find(taxid);
    if (it == merged.end() || it->second == taxid) break;
    taxid = it->second;
  }
  return taxid;
}

bool Taxonomy::known(uint32_t taxid) const {
  taxid = resolve(taxid);
  return !deleted.count(taxid) && nodes.count(taxid);
}

uint32_t Taxonomy::species_of(uint32_t taxid) const {
  taxid = resolve(taxid);
  if (deleted.count(taxid)) return 0;
  for (size_t step = 0; step <= nodes.size(); step++) {  // (more steps than nodes is a loop)
    auto it = nodes.find(taxid);
    if (it == nodes.end()) return 0;
    if (it->second.species) return taxid;
    if (it->second.parent == taxid) return 0;  // the root
    taxid = it->second.parent;
  }
  return 0;
}

bool TaxidMap::load(const std::string& path, std::string* err) {
  std::ifstream in(path);
  if (!in) {
    *err = path + ": " + strerror(errno);
    return false;
  }
  std::string line;
  while (std::getline(in, line)) {
    while (!line.empty() && (line.back() == '\r' || line.back() == '\n')) line.pop_back();
    if (line.empty()) continue;
    const size_t t1 = line.find('\t');
    if (t1 == std::string::npos) continue;
    size_t t2 = line.find('\t', t1 + 1);
    if (t2 == std::string::npos) t2 = line.size();
    const std::string val = line.substr(t1 + 1, t2 - t1 - 1);
    uint32_t v = 0;
    if (!parse_u32(val, &v)) {
      *err = "invalid TaxId: " + val;
      return false;
    }
    ids[line.substr(0, t1)] = v;
  }
  return true;
}

bool specific_classes(const std::vector<std::string>& names, const TaxidMap* map, const Taxonomy* tax, std::vector<uint32_t>* classes,
                      std::vector<uint32_t>* species, uint64_t* unknown_taxids, std::string* missing) {
  std::unordered_map<std::string, uint32_t> cls;
  std::unordered_set<uint32_t> unknown;
  classes->assign(names.size(), 0);
  if (species) species->assign(names.size(), 0);
  for (size_t i = 0; i < names.size(); i++) {
    auto ins = cls.emplace(names[i], (uint32_t)cls.size());
    (*classes)[i] = ins.first->second;
    if (!species || !map || !tax) continue;
    auto it = map->ids.find(names[i]);
    if (it == map->ids.end()) {
      if (missing) *missing = names[i];
      return false;
    }
    if (!tax->known(it->second)) unknown.insert(it->second);
    (*species)[i] = tax->species_of(it->second);
  }
  if (unknown_taxids) *unknown_taxids = unknown.size();
  return true;
}

}  // namespace kmcpg
