// specific_rule_check — the class shortcut of kmcp_amd/csrc/specific_rule.hpp (minimum and maximum of target_class / species_class)
// against the literal rule of `kmcp utils filter` (one target, or the LCA of the targets' TaxIds — found by walking parents — at or
// below rank species), over every assignment of TaxIds to up to 4 targets on the crafted tree of tests/filter_cases.py, and over
// random segments of columns (several chunks per target).  The tables come from taxonomy.cpp (files written here, read back), so
// the loader runs under the sanitizers too.
//
//   g++ -std=c++17 -fsanitize=address,undefined tests/specific_rule_check.cpp kmcp_amd/csrc/taxonomy.cpp && ./a.out <scratch dir>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../kmcp_amd/csrc/specific_rule.hpp"
#include "../kmcp_amd/csrc/taxonomy.hpp"

namespace {

struct N {
  uint32_t t, p;
  const char* rank;
};
const N NODES[] = {
    {1, 1, "no rank"}, {2, 1, "superkingdom"}, {10, 2, "phylum"}, {20, 10, "class"}, {30, 20, "order"}, {40, 30, "family"},
    {100, 40, "genus"}, {110, 100, "species"}, {111, 110, "strain"}, {112, 110, "strain"}, {113, 111, "no rank"},
    {120, 100, "species"}, {121, 120, "strain"},
    {500, 100, "species group"}, {510, 500, "species"}, {511, 510, "strain"},
    {200, 40, "genus"}, {210, 200, "species"}, {211, 210, "subspecies"}, {212, 211, "strain"},
    {300, 40, "genus"}, {301, 300, "no rank"},
    {50, 30, "family"}, {400, 50, "genus"}, {410, 400, "species"},
};
// every node, the merged TaxId 999 (-> 111), the deleted 888 and 777, which no file knows
std::vector<uint32_t> all_taxids() {
  std::vector<uint32_t> v;
  for (const N& n : NODES) v.push_back(n.t);
  v.push_back(999);
  v.push_back(888);
  v.push_back(777);
  return v;
}

// ---- the literal rule, from the arrays above and nothing else ----
std::map<uint32_t, N> by_id() {
  std::map<uint32_t, N> m;
  for (const N& n : NODES) m[n.t] = n;
  return m;
}
const std::map<uint32_t, N> TREE = by_id();

std::vector<uint32_t> lineage(uint32_t t) {
  if (t == 999) t = 111;
  std::vector<uint32_t> out;
  if (t == 888 || !TREE.count(t)) return out;
  for (;;) {
    out.push_back(t);
    const N& n = TREE.at(t);
    if (n.p == t) break;
    t = n.p;
  }
  return out;
}
uint32_t lca(uint32_t a, uint32_t b) {  // 0: none
  if (a == 0 || b == 0) return 0;
  const std::vector<uint32_t> la = lineage(a), lb = lineage(b);
  for (uint32_t x : lb)
    for (uint32_t y : la)
      if (x == y) return x;
  return 0;
}
bool at_or_below_species(uint32_t t) {
  if (t == 0) return false;
  for (uint32_t x : lineage(t))
    if (std::string(TREE.at(x).rank) == "species") return true;
  return false;
}
// targets: (name, TaxId) of every row of the query
bool literal_keep(const std::vector<std::pair<std::string, uint32_t>>& rows, bool level_species) {
  std::vector<std::pair<std::string, uint32_t>> distinct;
  for (const auto& r : rows) {
    bool seen = false;
    for (const auto& d : distinct) seen |= d.first == r.first;
    if (!seen) distinct.push_back(r);
  }
  bool same = false;
  if (level_species) {
    uint32_t node = lineage(distinct[0].second).empty() ? 0 : lineage(distinct[0].second)[0];
    for (size_t i = 1; i < distinct.size(); i++) node = lca(node, distinct[i].second);
    same = at_or_below_species(node);
  }
  return distinct.size() == 1 || same;
}

long wrong = 0, checked = 0;
void expect(bool ok, const char* what) {
  checked++;
  if (!ok) {
    wrong++;
    if (wrong < 20) printf("WRONG: %s\n", what);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  {
    std::ofstream n(dir + "/nodes.dmp"), m(dir + "/merged.dmp"), d(dir + "/delnodes.dmp");
    for (const N& x : NODES) n << x.t << "\t|\t" << x.p << "\t|\t" << x.rank << "\t|\tXX\t|\t0\t|\n";
    m << "999\t|\t111\t|\n";
    d << "888\t|\n";
  }
  kmcpg::Taxonomy tax;
  std::string err;
  if (!tax.load(dir, &err)) {
    printf("load: %s\n", err.c_str());
    return 1;
  }
  const std::vector<uint32_t> ids = all_taxids();
  // species_of against the literal walk
  for (uint32_t t : ids) {
    uint32_t want = 0;
    for (uint32_t x : lineage(t))
      if (!want && std::string(TREE.at(x).rank) == "species") want = x;
    expect(tax.species_of(t) == want, "species_of");
    expect(tax.known(t) == !lineage(t).empty(), "known");
  }
  expect(tax.resolve(999) == 111 && tax.resolve(111) == 111, "resolve");

  // every assignment of TaxIds to 1 .. 3 distinct targets over every TaxId, to 4 targets over one of every kind (a species, its strains,
  // the node below a strain, the merged TaxId, a sister species and its strain, the genus, the species-group strain, the no-rank node,
  // another genus' strain, the deleted and the absent TaxId); both levels
  const std::vector<uint32_t> every = ids, kinds = {110, 111, 112, 113, 999, 120, 121, 100, 511, 301, 212, 888, 777};
  for (int k = 1; k <= 4; k++) {
    const std::vector<uint32_t>& ids = k == 4 ? kinds : every;
    const size_t T = ids.size();
    size_t total = 1;
    for (int i = 0; i < k; i++) total *= T;
    for (size_t code = 0; code < total; code++) {
      std::vector<std::string> names;
      kmcpg::TaxidMap map;
      std::vector<std::pair<std::string, uint32_t>> rows;
      size_t c = code;
      for (int i = 0; i < k; i++) {
        names.push_back("t" + std::to_string(i));
        map.ids[names.back()] = ids[c % T];
        rows.emplace_back(names.back(), ids[c % T]);
        c /= T;
      }
      std::vector<uint32_t> cls, sp;
      uint64_t unknown = 0;
      std::string missing;
      if (!kmcpg::specific_classes(names, &map, &tax, &cls, &sp, &unknown, &missing)) {
        expect(false, "specific_classes refused");
        continue;
      }
      kmcpg::SpecificAcc acc;
      for (int i = 0; i < k; i++) acc.add(cls[(size_t)i], sp[(size_t)i]);
      expect(kmcpg::specific_keep(acc, true) == literal_keep(rows, true), "assignment, level species");
      expect(kmcpg::specific_keep(acc, false) == (k == 1), "assignment, level strain");
    }
  }

  // random segments over columns: 40 columns, chunks of 14 targets
  const size_t T = ids.size();
  std::mt19937_64 rng(12345);
  for (int round = 0; round < 6000; round++) {
    const int n_targets = 2 + (int)(rng() % 13);
    std::vector<std::string> col_name;
    kmcpg::TaxidMap map;
    for (int c = 0; c < 40; c++) {
      const int t = (int)(rng() % (uint64_t)n_targets);
      col_name.push_back("ref" + std::to_string(t));
    }
    // most rounds draw the TaxIds from one species' subtree or one genus, so that KEEP is common
    const uint32_t pool_a[] = {110, 111, 112, 113, 999}, pool_b[] = {110, 111, 120, 121, 100, 511};
    for (int t = 0; t < n_targets; t++) {
      const int how = round % 3;
      map.ids["ref" + std::to_string(t)] = how == 0 ? pool_a[rng() % 5] : (how == 1 ? pool_b[rng() % 6] : ids[rng() % T]);
    }
    std::vector<uint32_t> cls, sp;
    if (!kmcpg::specific_classes(col_name, &map, &tax, &cls, &sp, nullptr, nullptr)) {
      expect(false, "specific_classes refused");
      continue;
    }
    for (int c = 0; c < 40 && round % 40 == 0; c++)
      for (int d = 0; d < 40; d++) expect((cls[(size_t)c] == cls[(size_t)d]) == (col_name[(size_t)c] == col_name[(size_t)d]), "target_class");
    const int len = 1 + (int)(rng() % 12);
    kmcpg::SpecificAcc acc;
    std::vector<std::pair<std::string, uint32_t>> rows;
    for (int i = 0; i < len; i++) {
      const size_t c = (size_t)(rng() % 40);
      acc.add(cls[c], sp[c]);
      rows.emplace_back(col_name[c], map.ids[col_name[c]]);
    }
    expect(kmcpg::specific_keep(acc, true) == literal_keep(rows, true), "segment, level species");
    std::set<std::string> distinct;
    for (const auto& r : rows) distinct.insert(r.first);
    expect(kmcpg::specific_keep(acc, false) == (distinct.size() == 1), "segment, level strain");
  }
  expect(!kmcpg::specific_keep(kmcpg::SpecificAcc(), true), "a query without matches has no verdict");
  // a target without a TaxId is reported
  {
    kmcpg::TaxidMap map;
    map.ids["a"] = 111;
    std::vector<uint32_t> cls, sp;
    std::string missing;
    expect(!kmcpg::specific_classes({"a", "b"}, &map, &tax, &cls, &sp, nullptr, &missing) && missing == "b", "missing TaxId");
    expect(kmcpg::specific_classes({"a", "b", "a"}, nullptr, nullptr, &cls, nullptr, nullptr, nullptr) && cls[0] == cls[2] && cls[0] != cls[1], "strain level");
  }
  printf("%ld checked, %ld wrong\n", checked, wrong);
  return wrong ? 1 : 0;
}
