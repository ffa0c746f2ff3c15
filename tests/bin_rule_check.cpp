// bin_rule_check.cpp — kmcp_amd/csrc/bin_rule.hpp alone: the pre-order tables of the pruned tree and bin_lca(min, max) against a brute-force
// LCA by ancestor sets taken from the taxonomy itself, over random forests (several roots, unknown, deleted and merged ids, references
// mapped to leaves and to inner nodes) and chains deeper than 40; the missing-TaxId refusal; the per-query accumulator (whitelist skip
// before the cuts).  Built with taxonomy.cpp; prints "<checks> checks, <n> wrong".
#include <cstdio>
#include <random>
#include <set>

#include "../kmcp_amd/csrc/bin_rule.hpp"

using namespace kmcpg;

static uint64_t checks = 0, wrong = 0;
#define CHECK(c, ...)                                     \
  do {                                                    \
    checks++;                                             \
    if (!(c)) {                                           \
      if (++wrong <= 20) printf("line %d: ", __LINE__), printf(__VA_ARGS__), printf("\n"); \
    }                                                     \
  } while (0)

// the chain of a TaxId in the taxonomy itself: self, parents, then the virtual root 0; an unknown id: itself, then 0
static std::vector<uint32_t> chain(const Taxonomy& tax, uint32_t t) {
  t = tax.resolve(t);
  std::vector<uint32_t> c;
  if (!tax.known(t)) return {t, 0};
  for (;;) {
    c.push_back(t);
    const uint32_t p = tax.nodes.at(t).parent;
    if (p == t || !tax.nodes.count(p)) break;
    t = p;
  }
  c.push_back(0);
  return c;
}
static uint32_t brute_lca(const Taxonomy& tax, const std::vector<uint32_t>& ids) {
  std::vector<std::set<uint32_t>> sets;
  for (uint32_t t : ids) {
    auto c = chain(tax, t);
    sets.emplace_back(c.begin(), c.end());
  }
  for (uint32_t a : chain(tax, ids[0])) {  // deepest first
    bool all = true;
    for (auto& s : sets) all = all && s.count(a);
    if (all) return a;
  }
  return 0;
}

static void check_tables(const Taxonomy& tax, const BinPlan& p, int it) {
  const size_t n = p.parent.size();
  CHECK(n >= 1 && p.last.size() == n && p.taxid.size() == n, "case %d: sizes", it);
  CHECK(p.parent[0] == 0 && p.taxid[0] == 0 && p.last[0] == n - 1, "case %d: node 0", it);
  std::set<uint32_t> seen;
  for (uint32_t v = 1; v < n; v++) {
    CHECK(p.parent[v] < v, "case %d: parent[%u] = %u is not before it", it, v, p.parent[v]);
    CHECK(seen.insert(p.taxid[v]).second, "case %d: TaxId %u twice", it, p.taxid[v]);
    // the parent in the plan is the parent in the taxonomy (0 above a root or an unknown id)
    auto c = chain(tax, p.taxid[v]);
    CHECK(c.size() >= 2 && c[0] == p.taxid[v] && c[1] == p.taxid[p.parent[v]], "case %d: node %u (TaxId %u) hangs under TaxId %u", it, v, p.taxid[v], p.taxid[p.parent[v]]);
  }
  // pre-order: the descendants of v are exactly (v, last[v]]
  for (uint32_t v = 0; v < n; v++) {
    CHECK(p.last[v] >= v && p.last[v] < n, "case %d: last[%u] = %u", it, v, p.last[v]);
    for (uint32_t w = 0; w < n; w++) {
      bool below = false;
      for (uint32_t x = w; !below; x = p.parent[x]) {
        below = x == v;
        if (x == 0) break;
      }
      CHECK(below == (w >= v && w <= p.last[v]), "case %d: node %u %s below %u, last[%u] = %u", it, w, below ? "is" : "is not", v, v, p.last[v]);
    }
  }
}

static void check_subsets(const Taxonomy& tax, const TaxidMap& map, const std::vector<std::string>& names, const BinPlan& p, int it) {
  const size_t k = names.size();
  auto one = [&](std::vector<size_t> pick) {
    std::vector<uint32_t> ids;
    uint32_t lo = BIN_NO_NODE, hi = 0;
    for (size_t i : pick) {
      ids.push_back(map.ids.at(names[i]));
      const uint32_t v = p.node_of(names[i]);
      CHECK(v != BIN_NO_NODE && v < p.parent.size() && v != 0, "case %d: %s has node %u", it, names[i].c_str(), v);
      if (v == BIN_NO_NODE || v >= p.parent.size()) return;
      CHECK(p.taxid[v] == tax.resolve(ids.back()), "case %d: %s prints as %u", it, names[i].c_str(), p.taxid[v]);
      lo = std::min(lo, v), hi = std::max(hi, v);
    }
    const uint32_t got = p.taxid[bin_lca(p, lo, hi)], want = brute_lca(tax, ids);
    CHECK(got == want, "case %d: LCA of %zu references is %u, brute force says %u", it, pick.size(), got, want);
  };
  for (size_t a = 0; a < k; a++) {
    one({a});
    for (size_t b = a + 1; b < k; b++) {
      one({a, b});
      for (size_t c = b + 1; c < k; c++) one({a, b, c});
    }
  }
}

int main() {
  std::mt19937 rng(20240611);
  auto rnd = [&](uint32_t n) { return (uint32_t)(rng() % n); };
  int it = 0;
  for (; it < 400; it++) {
    Taxonomy tax;
    TaxidMap map;
    const uint32_t n = 1 + rnd(30), roots = 1 + rnd(std::min(n, 3u));
    std::vector<uint32_t> ids;
    for (uint32_t i = 0; i < n; i++) ids.push_back(10 + i * 7 + rnd(7));  // distinct; shuffled: a child may have the smaller TaxId
    std::shuffle(ids.begin(), ids.end(), rng);
    for (uint32_t i = 0; i < n; i++) tax.nodes[ids[i]] = Taxonomy::Node{i < roots ? ids[i] : ids[rnd(i)], false};
    if (it % 5 == 0 && n > roots) tax.nodes[ids[roots]].parent = 5;  // a parent that nodes.dmp does not have: a root as well
    // merged ids (one through a chain of two); 5000 is absent from nodes.dmp, 5001 is deleted as well
    tax.merged[1000] = ids[rnd(n)];
    tax.merged[1001] = 1000;
    tax.deleted.insert(5001);
    std::vector<std::string> names;
    const uint32_t k = 1 + rnd(9);
    for (uint32_t i = 0; i < k; i++) {
      names.push_back("ref" + std::to_string(i));
      const uint32_t how = rnd(10);
      map.ids[names.back()] = how == 0 ? 5000 + rnd(2) : how == 1 ? 1000 + rnd(2) : ids[rnd(n)];  // absent; merged; a leaf or an inner node
    }
    BinPlan p;
    std::string missing;
    CHECK(bin_plan_build(tax, map, names, &p, &missing), "case %d: refused (%s)", it, missing.c_str());
    check_tables(tax, p, it);
    check_subsets(tax, map, names, p, it);
    // a non-whitelisted name has no node
    CHECK(p.node_of("nobody") == BIN_NO_NODE, "case %d: a name off the whitelist has a node", it);
  }
  // chains deeper than 40, with references along them and on a side branch
  for (uint32_t depth : {41u, 48u, 100u}) {
    Taxonomy tax;
    TaxidMap map;
    tax.nodes[1] = Taxonomy::Node{1, false};
    for (uint32_t i = 2; i <= depth; i++) tax.nodes[i] = Taxonomy::Node{i - 1, false};
    tax.nodes[900] = Taxonomy::Node{depth / 2, false};
    std::vector<std::string> names = {"bottom", "middle", "top", "side", "near"};
    map.ids["bottom"] = depth, map.ids["middle"] = depth / 2, map.ids["top"] = 1, map.ids["side"] = 900, map.ids["near"] = depth - 1;
    BinPlan p;
    std::string missing;
    CHECK(bin_plan_build(tax, map, names, &p, &missing), "chain %u: refused", depth);
    CHECK(p.parent.size() == depth + 2, "chain %u: %zu nodes", depth, p.parent.size());
    check_tables(tax, p, (int)depth);
    check_subsets(tax, map, names, p, (int)depth);
    uint64_t steps = 0;
    const uint32_t lo = std::min(p.node_of("bottom"), p.node_of("side")), hi = std::max(p.node_of("bottom"), p.node_of("side"));
    CHECK(p.taxid[bin_lca(p.parent.data(), p.last.data(), lo, hi, &steps)] == depth / 2 && steps >= 1, "chain %u: bottom and side", depth);
    it++;
  }
  {  // the refusal names the FIRST whitelisted reference without a TaxId
    Taxonomy tax;
    TaxidMap map;
    tax.nodes[1] = Taxonomy::Node{1, false};
    map.ids["a"] = 1;
    BinPlan p;
    std::string missing;
    CHECK(!bin_plan_build(tax, map, {"a", "x", "y"}, &p, &missing) && missing == "x", "the refusal names '%s'", missing.c_str());
    // an empty whitelist: the virtual root alone
    CHECK(bin_plan_build(tax, map, {}, &p, &missing) && p.parent.size() == 1 && p.last[0] == 0, "empty whitelist");
  }
  {  // the per-query accumulator: tree 1 -> (2 -> (3, 4), 5); references r3, r4, r5, and r2 on the inner node
    Taxonomy tax;
    TaxidMap map;
    tax.nodes[1] = Taxonomy::Node{1, false};
    tax.nodes[2] = Taxonomy::Node{1, false}, tax.nodes[5] = Taxonomy::Node{1, false};
    tax.nodes[3] = Taxonomy::Node{2, true}, tax.nodes[4] = Taxonomy::Node{2, true};
    map.ids["r2"] = 2, map.ids["r3"] = 3, map.ids["r4"] = 4, map.ids["r5"] = 5, map.ids["off"] = 5;
    BinPlan p;
    std::string missing;
    CHECK(bin_plan_build(tax, map, {"r3", "r4", "r5", "r2"}, &p, &missing), "refused");
    const uint32_t n3 = p.node_of("r3"), n4 = p.node_of("r4"), n5 = p.node_of("r5"), n2 = p.node_of("r2"), off = p.node_of("off");
    CHECK(off == BIN_NO_NODE, "off is whitelisted");
    BinAcc a;
    a.begin();
    CHECK(a.bin(p) == BIN_NONE, "no row");
    a.row(off, 1.0);
    CHECK(a.bin(p) == BIN_NONE, "only a row off the whitelist");
    a.row(n3, 0.9);
    CHECK(a.bin(p) == 3, "one target");
    a.row(n3, 0.9), a.row(n4, 0.8);
    CHECK(a.bin(p) == 2, "siblings");
    a.row(n2, 0.8);
    CHECK(a.bin(p) == 2, "ancestor with descendants");
    a.row(n5, 0.8);
    CHECK(a.bin(p) == 1, "across the root's children");
    // --keep-perfect-matches: a perfect first row cuts the rest; a perfect row OFF the whitelist is no first row and cuts nothing
    BinAcc b;
    b.cut.keep_perfect = true;
    b.begin(), b.row(n3, 1.0), b.row(n5, 0.9);
    CHECK(b.bin(p) == 3, "keep-perfect cuts the second row");
    b.begin(), b.row(off, 1.0), b.row(n3, 0.9), b.row(n5, 0.9);
    CHECK(b.bin(p) == 1, "the skipped row changes which row is first");
    // --keep-main-matches with gap 0.4, and -n 1
    BinAcc c;
    c.cut.keep_main = true;
    c.begin(), c.row(n3, 0.95), c.row(n4, 0.9), c.row(n5, 0.45), c.row(n5, 0.9);
    CHECK(c.bin(p) == 2, "keep-main cuts at the gap, and everything behind it");
    BinAcc d;
    d.cut.top_n = 1;
    d.begin(), d.row(n3, 0.9), d.row(n4, 0.9), d.row(n5, 0.8);
    CHECK(d.bin(p) == 2, "-n 1 keeps the rows of the best score");
  }
  printf("%d cases, %llu checks, %llu wrong\n", it, (unsigned long long)checks, (unsigned long long)wrong);
  return wrong ? 1 : 0;
}
