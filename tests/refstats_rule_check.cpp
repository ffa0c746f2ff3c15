// refstats_rule_check — kmcp_amd/csrc/refstats_rule.hpp alone, on the host: the per-query counting against a literal dict-of-lists
// count, the row cuts, the roll-up and the verdict at its boundaries (chunksFrac exactly p), and the mode table.
// Prints "<n> checks, <w> wrong"; the exit status is 0 only with 0 wrong.
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../kmcp_amd/csrc/k3_set_order.hpp"
#include "../kmcp_amd/csrc/refstats_rule.hpp"

using namespace kmcpg;

static int checks = 0, wrong = 0;
#define CHECK(c)                                             \
  do {                                                       \
    checks++;                                                \
    if (!(c)) wrong++, printf("line %d: %s\n", __LINE__, #c); \
  } while (0)

using Counters = std::map<uint64_t, std::vector<uint64_t>>;

static bool count(const std::vector<RefstatsRow>& r, bool species, double H, Counters* c) {
  return refstats_count_query(r.data(), r.size(), species, H, [&](uint64_t col, int w) {
    auto& v = (*c)[col];
    v.resize(REFSTATS_WORDS);
    v[w]++;
  });
}

// the reference's way: target -> its rows in order; the first of each list is counted once
static bool count_literal(const std::vector<RefstatsRow>& r, bool species, double H, Counters* c) {
  std::map<uint32_t, std::vector<RefstatsRow>> by;
  for (const auto& x : r) by[x.target_class].push_back(x);
  bool same = species;
  uint32_t s0 = r[0].species_class;
  for (const auto& x : r) same = same && x.species_class == s0 && s0 != 0;
  const bool unique = by.size() == 1 || same;
  for (auto& kv : by) {
    bool first = true;
    for (const auto& m : kv.second) {
      auto& v = (*c)[m.column];
      v.resize(REFSTATS_WORDS);
      if (first) {
        v[REFSTATS_FIRSTS]++;
        if (unique) {
          v[REFSTATS_UREADS]++;
          if (m.qcov >= H) v[REFSTATS_HIC]++;
        }
        first = false;
      }
      v[REFSTATS_ROWS]++;
    }
  }
  return unique;
}

static RefstatsRef roll(const std::vector<std::vector<uint64_t>>& chunks, double p) {
  return refstats_rollup(chunks.size(), p, [&](uint64_t c) { return chunks[c].data(); });
}

int main() {
  // counting: fixed cases
  {
    Counters c;
    CHECK(count({{0, 5, 10, 0.9}, {0, 5, 12, 0.6}, {0, 5, 10, 0.56}}, false, 0.75, &c));
    CHECK((c[10] == std::vector<uint64_t>{2, 1, 1, 1}) && (c[12] == std::vector<uint64_t>{1, 0, 0, 0}));
  }
  {
    Counters c;  // the second row of target 0 has the higher chunk; two targets of one species
    CHECK(count({{0, 5, 10, 0.8}, {1, 5, 21, 0.7}, {0, 5, 12, 0.9}, {1, 5, 20, 0.9}}, true, 0.75, &c));
    CHECK((c[10] == std::vector<uint64_t>{1, 1, 1, 1}) && (c[12] == std::vector<uint64_t>{1, 0, 0, 0}));
    CHECK((c[21] == std::vector<uint64_t>{1, 1, 1, 0}) && (c[20] == std::vector<uint64_t>{1, 0, 0, 0}));
    Counters d;
    CHECK(!count({{0, 5, 10, 0.8}, {1, 5, 21, 0.7}}, false, 0.75, &d));  // strain level: two targets are not unique
    CHECK((d[10] == std::vector<uint64_t>{1, 1, 0, 0}) && (d[21] == std::vector<uint64_t>{1, 1, 0, 0}));
    Counters e;
    CHECK(!count({{0, 0, 10, 0.8}, {1, 0, 21, 0.7}}, true, 0.75, &e));  // species 0 = under no species
    CHECK(!count({{0, 5, 10, 0.8}, {1, 6, 21, 0.7}}, true, 0.75, &e));
  }
  {
    Counters c;  // qCov exactly H counts, the next double below does not
    count({{0, 0, 1, 0.75}}, false, 0.75, &c);
    count({{0, 0, 2, 0.7499}}, false, 0.75, &c);
    CHECK(c[1][REFSTATS_HIC] == 1 && c[2][REFSTATS_HIC] == 0 && c[2][REFSTATS_UREADS] == 1);
  }
  {
    Counters c;  // the qCov a row carries is the printed one: 15000 / 20001 = 0.74996... prints as 0.7500 and passes H = 0.75
    CHECK(printed_qcov(15000, 20001) == 0.75 && printed_qcov(14999, 20001) == 0.7499 && printed_qcov(75, 100) == 0.75 && printed_qcov(130, 130) == 1.0);
    count({{0, 0, 1, printed_qcov(15000, 20001)}}, false, 0.75, &c);
    count({{0, 0, 2, printed_qcov(14999, 20001)}}, false, 0.75, &c);
    CHECK(c[1][REFSTATS_HIC] == 1 && c[2][REFSTATS_HIC] == 0);
  }
  // counting: pseudo-random queries against the literal count
  uint64_t s = 88172645463325252ull;
  auto rnd = [&](uint32_t n) {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return (uint32_t)((s >> 20) % n);
  };
  for (int it = 0; it < 2000; it++) {
    std::vector<RefstatsRow> r(1 + rnd(9));
    const uint32_t nt = 1 + rnd(4);
    for (auto& x : r) {
      x.target_class = rnd(nt) * 7;
      x.species_class = it % 3 == 0 ? 3 : x.target_class / 14;  // joins neighbouring targets; class 0 is "no species"
      x.column = x.target_class * 10 + rnd(3);
      x.qcov = (double)(6000 + rnd(4000)) / 10000.0;
    }
    for (int species = 0; species < 2; species++) {
      Counters a, b;
      const bool ua = count(r, species, 0.8, &a), ub = count_literal(r, species, 0.8, &b);
      CHECK(ua == ub && a == b);
    }
  }
  // the row cuts
  {
    RefstatsCut c;
    c.keep_perfect = true;
    CHECK(c.keep(true, 1.0) && c.keep(false, 1.0) && !c.keep(false, 0.9) && !c.keep(false, 1.0));
    CHECK(c.keep(true, 0.9) && c.keep(false, 0.8));  // no perfect match: all stay
    RefstatsCut m;
    m.keep_main = true;
    CHECK(m.keep(true, 1.0) && m.keep(false, 0.61) && !m.keep(false, 0.2) && !m.keep(false, 0.6));
    CHECK(m.keep(true, 0.15) && m.keep(false, 0.1));  // a first row is never tested
    RefstatsCut n;
    n.top_n = 1;
    CHECK(n.keep(true, 0.9) && n.keep(false, 0.9) && !n.keep(false, 0.8) && !n.keep(false, 0.9));
    n.top_n = 2;
    CHECK(n.keep(true, 0.9) && n.keep(false, 0.8) && n.keep(false, 0.8) && !n.keep(false, 0.7));
    RefstatsCut pm;  // --keep-perfect-matches shadows --keep-main-matches (an else-if chain)
    pm.keep_perfect = pm.keep_main = true;
    CHECK(pm.keep(true, 0.9) && pm.keep(false, 0.1));
  }
  // roll-up and verdict
  {
    RefstatsRef t = roll({{3, 2, 1, 1}, {0, 0, 0, 0}, {1, 1, 1, 0}, {2, 0, 0, 0}}, 0.75);
    CHECK(t.reads == 3 && t.ureads == 2 && t.hic_ureads == 1 && t.covered == 3 && t.chunks_frac == 0.75 && t.verdict == REFSTATS_OK);  // exactly p
    CHECK(roll({{3, 2, 1, 1}, {0, 0, 0, 0}, {1, 1, 1, 0}, {2, 0, 0, 0}}, 0.7500000000000001).verdict == REFSTATS_LOW_CHUNKS);
    CHECK(roll({{1, 1, 1, 1}}, 1.0).verdict == REFSTATS_OK);
    // 7 of 10 chunks against p = 0.7: 7.0 / 10.0 is the double 0.7
    std::vector<std::vector<uint64_t>> ten(10, std::vector<uint64_t>{0, 0, 0, 0});
    for (int i = 0; i < 7; i++) ten[i] = {1, 1, 1, 1};
    CHECK(roll(ten, 0.7).verdict == REFSTATS_OK && roll(ten, 0.8).verdict == REFSTATS_LOW_CHUNKS);
    // the order of the tests: no unique read wins over everything, then no high-confidence one
    CHECK(roll({{5, 5, 0, 0}, {0, 0, 0, 0}}, 1.0).verdict == REFSTATS_NO_UNIQUE);
    CHECK(roll({{5, 5, 2, 0}, {0, 0, 0, 0}}, 1.0).verdict == REFSTATS_NO_HIC_UNIQUE);
    CHECK(roll({{5, 5, 2, 1}, {0, 0, 0, 0}}, 1.0).verdict == REFSTATS_LOW_CHUNKS);
    CHECK(roll({{5, 5, 2, 1}, {0, 0, 0, 0}}, 0.0).verdict == REFSTATS_OK);
    // a chunk with rows but no first row is covered
    CHECK(roll({{0, 0, 0, 0}, {4, 0, 0, 0}}, 0.5).covered == 1);
    CHECK(std::string(refstats_verdict_name(REFSTATS_OK)) == "ok" && std::string(refstats_verdict_name(REFSTATS_LOW_CHUNKS)) == "low-chunks-fraction");
    CHECK(std::string(refstats_verdict_name(REFSTATS_NO_UNIQUE)) == "no-unique" && std::string(refstats_verdict_name(REFSTATS_NO_HIC_UNIQUE)) == "no-hic-unique");
  }
  // the mode table
  {
    const double H[6] = {0.7, 0.7, 0.7, 0.75, 0.8, 0.8}, p[6] = {0.2, 0.6, 0.7, 0.8, 1, 1};
    for (int m = 0; m < REFSTATS_MODES; m++) {
      const RefstatsMode x = refstats_mode(m);
      CHECK(x.hic_min_qcov == H[m] && x.min_chunks_fraction == p[m] && x.keep_main == (m == 0));
    }
  }
  printf("%d checks, %d wrong\n", checks, wrong);
  return wrong ? 1 : 0;
}
