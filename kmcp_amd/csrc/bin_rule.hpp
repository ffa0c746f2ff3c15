// bin_rule.hpp — taxonomic binning: which TaxId a read gets from the references it matches.  The one rule behind kmcp-refstats --binning
// (cli/kmcp_refstats.cpp), the library's host half (binning.cpp) and the tests' stand-alone check (tests/bin_rule_check.cpp).  Host only,
// plain C++17; k11_bin.hip restates the per-read part.
//
// Reference counterpart: the binning pass of `kmcp profile -B` (kmcp/cmd/profile.go:2591-2784), a second pass over the search result once
// the EM has ended and the whitelist of references is final.
//
// Rows and targets.  Rows of a query whose target is not on the whitelist are skipped before anything else.  The row cuts (RefstatsCut of
// refstats_rule.hpp) apply after that skip: a query's "first row" is its first WHITELISTED row.  The kept rows name a set of targets: an
// empty set gives no line, one target gives its TaxId, several give the lowest common ancestor (LCA) of their TaxIds.
//
// The pruned tree (BinPlan).  Only the nodes on the paths from the whitelisted references' TaxIds to the root are held.  TaxIds are resolved
// through merged.dmp first.  Node 0 is a virtual root that prints as TaxId 0, above the real root(s).  A TaxId that is deleted or absent from
// nodes.dmp becomes its own child of node 0: alone it prints as it is mapped (after merged.dmp), beside any other target the bin is 0 — the
// reference's LCA for such ids lives in a third-party module and cannot be pinned.  Nodes are numbered in PRE-ORDER; parent[] is a node's
// parent, last[] the largest pre-order number in its subtree (so the subtree of v is exactly [v, last[v]]), taxid[] what it prints as.
//
// The property the device kernel rests on: in a rooted tree numbered in pre-order, the LCA of a set of nodes is the LCA of the member
// with the smallest number and the member with the largest.  (An ancestor a of both lo and hi has lo, hi in [a, last[a]], hence every
// member, whose number lies between them; and an ancestor of all members is an ancestor of lo and hi in particular.)  A read therefore needs only a min and a max
// over its whitelisted rows, then ONE climb: bin_lca goes up from lo until the subtree reaches hi.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "refstats_rule.hpp"
#include "taxonomy.hpp"

namespace kmcpg {

constexpr uint32_t BIN_NO_NODE = 0xffffffffu;  // node_of_column of a column whose target is not whitelisted (= NO_CLASS of seg_walk.hpp)
constexpr uint32_t BIN_NONE = 0xffffffffu;     // a read's bin: no whitelisted row, no line
constexpr uint32_t BIN_LEFT = 0xfffffffeu;     // a read's bin on the device: left to the host

struct BinPlan {
  std::vector<uint32_t> parent, last, taxid;  // by pre-order number; node 0: the virtual root (parent 0, TaxId 0)
  std::unordered_map<std::string, uint32_t> node_of_name;  // the whitelisted references
  uint64_t unknown_taxids = 0;  // distinct resolved TaxIds that are deleted or absent from nodes.dmp
  uint32_t node_of(const std::string& name) const {
    auto it = node_of_name.find(name);
    return it == node_of_name.end() ? BIN_NO_NODE : it->second;
  }
};

// The plan of a whitelist.  false: *missing = the first whitelisted reference without a TaxId in the map (refused: the reference aborts on
// such a target in a multi-target read and prints 0 for a single one).
inline bool bin_plan_build(const Taxonomy& tax, const TaxidMap& map, const std::vector<std::string>& whitelist, BinPlan* plan, std::string* missing) {
  *plan = BinPlan{};
  // the pruned tree by TaxId: parent 0 = under the virtual root
  std::unordered_map<uint32_t, uint32_t> up;
  std::vector<uint32_t> leaf(whitelist.size());
  for (size_t i = 0; i < whitelist.size(); i++) {
    auto it = map.ids.find(whitelist[i]);
    if (it == map.ids.end()) {
      if (missing) *missing = whitelist[i];
      return false;
    }
    uint32_t t = tax.resolve(it->second);
    leaf[i] = t;
    if (up.count(t)) continue;
    if (!tax.known(t)) {
      up[t] = 0;
      plan->unknown_taxids++;
      continue;
    }
    for (size_t step = 0; step <= tax.nodes.size() && !up.count(t); step++) {  // (more steps than nodes is a loop: it ends at a node seen)
      const uint32_t p = tax.nodes.find(t)->second.parent;
      if (p == t || !tax.nodes.count(p)) {  // a root
        up[t] = 0;
        break;
      }
      up[t] = p;
      t = p;
    }
  }
  // children in TaxId order, then pre-order without recursion (chains are deep)
  std::vector<std::pair<uint32_t, uint32_t>> edges;  // (parent TaxId, TaxId)
  edges.reserve(up.size());
  for (auto& e : up) edges.emplace_back(e.second, e.first);
  std::sort(edges.begin(), edges.end());
  auto kids = [&](uint32_t t) { return std::equal_range(edges.begin(), edges.end(), std::make_pair(t, 0u), [](auto& a, auto& b) { return a.first < b.first; }); };
  const size_t n = up.size() + 1;
  plan->parent.assign(n, 0), plan->last.assign(n, 0), plan->taxid.assign(n, 0);
  std::unordered_map<uint32_t, uint32_t> number;
  struct Frame {
    uint32_t node;
    decltype(edges.begin()) at, end;
  };
  std::vector<Frame> stack;
  uint32_t next = 1;
  {
    auto r = kids(0);
    stack.push_back({0, r.first, r.second});
  }
  while (!stack.empty()) {
    Frame& f = stack.back();
    if (f.at == f.end) {
      plan->last[f.node] = next - 1;
      stack.pop_back();
      continue;
    }
    const uint32_t t = (f.at++)->second, p = f.node;
    if (t == 0 || number.count(t)) continue;  // (TaxId 0 is the virtual root's; a loop in nodes.dmp)
    const uint32_t v = next++;
    number[t] = v;
    plan->parent[v] = p, plan->taxid[v] = t;
    auto r = kids(t);
    stack.push_back({v, r.first, r.second});
  }
  plan->parent.resize(next), plan->last.resize(next), plan->taxid.resize(next);
  for (size_t i = 0; i < whitelist.size(); i++) {
    auto it = number.find(leaf[i]);
    plan->node_of_name[whitelist[i]] = it == number.end() ? 0u : it->second;
  }
  return true;
}

// The LCA of the nodes lo <= hi: climb from lo until the subtree reaches hi (node 0's reaches every node)
inline uint32_t bin_lca(const uint32_t* parent, const uint32_t* last, uint32_t lo, uint32_t hi, uint64_t* steps = nullptr) {
  uint32_t v = lo;
  while (last[v] < hi) {
    v = parent[v];
    if (steps) ++*steps;
  }
  return v;
}
inline uint32_t bin_lca(const BinPlan& plan, uint32_t lo, uint32_t hi) { return bin_lca(plan.parent.data(), plan.last.data(), lo, hi); }

// The kept targets of one query as the range of their nodes, and its bin: what every host-side caller folds a query's nodes into (the
// TSV tool below, the library's host half, a caller that holds a query's final pairs).  Nodes off the whitelist are not added.
struct BinRange {
  uint32_t lo = BIN_NO_NODE, hi = 0;
  void add(uint32_t node) {
    if (node != BIN_NO_NODE) lo = std::min(lo, node), hi = std::max(hi, node);
  }
  bool none() const { return lo == BIN_NO_NODE; }
  // the TaxId of the query's line, or BIN_NONE: no line
  uint32_t bin(const uint32_t* parent, const uint32_t* last, const uint32_t* taxid) const { return none() ? BIN_NONE : taxid[bin_lca(parent, last, lo, hi)]; }
  uint32_t bin(const BinPlan& plan) const { return bin(plan.parent.data(), plan.last.data(), plan.taxid.data()); }
};

// One query, row by row in the order of the search result: node = the row's target's node (BIN_NO_NODE: not whitelisted).
struct BinAcc {
  RefstatsCut cut;
  BinRange range;
  bool first = true;
  void begin() { range = BinRange(), first = true; }
  void row(uint32_t node, double qcov) {
    if (node == BIN_NO_NODE) return;  // skipped before anything else: it is no "first row" either
    const bool keep = cut.keep(first, qcov);
    first = false;
    if (keep) range.add(node);
  }
  uint32_t bin(const BinPlan& plan) const { return range.bin(plan); }
};

}  // namespace kmcpg
