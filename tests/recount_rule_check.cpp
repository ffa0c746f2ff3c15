// recount_rule_check.cpp — kmcp_amd/csrc/recount_rule.hpp stand-alone on the host (tests/test_recount_rule_cpu.py builds it with the
// address and undefined-behaviour sanitizers): the elimination in bit masks against the literal double loop of the reference on random
// predicates (the three-target quirk case included), the shares of a target's rows, the tie order, a read's adds and the verdicts.
#include <cstdio>
#include <map>
#include <random>
#include <vector>

#include "../kmcp_amd/csrc/recount_rule.hpp"

using namespace kmcpg;

static int wrong = 0, checks = 0;
#define CHECK(...)                                           \
  do {                                                       \
    checks++;                                                \
    if (!(__VA_ARGS__)) {                                              \
      wrong++;                                               \
      printf("line %d: %s\n", __LINE__, #__VA_ARGS__);                 \
    }                                                        \
  } while (0)

// profile.go:1357-1382 as written: pred[i][j] for i < j
static std::vector<bool> literal_loop(const std::vector<std::vector<int>>& pred) {
  const size_t n = pred.size();
  std::vector<bool> del(n, false);
  for (size_t i = 0; i + 1 < n; i++) {
    if (del[i]) continue;
    for (size_t j = i + 1; j < n; j++) {
      if (del[j]) continue;
      if (pred[i][j] == 1) del[j] = true;
      else if (pred[i][j] == 2) del[i] = true;  // the j loop goes on
    }
  }
  return del;
}

static void mask_checks() {
  std::mt19937 rng(7);
  for (int round = 0; round < 3000; round++) {
    const size_t n = round < 200 ? (size_t)(round % 6) + 1 : (size_t)(rng() % 150) + 1;
    const unsigned density = 1 + rng() % 12;  // how rare a condition is
    std::vector<std::vector<int>> pred(n, std::vector<int>(n, 0));
    for (size_t i = 0; i < n; i++)
      for (size_t j = i + 1; j < n; j++) {
        const unsigned x = rng() % (2 * density);
        pred[i][j] = x == 0 ? 1 : x == 1 ? 2 : 0;
      }
    const std::vector<bool> want = literal_loop(pred);
    std::vector<uint64_t> del;
    recount_eliminate(n, [&](size_t i, size_t j) { return pred[i][j]; }, &del);
    bool same = del.size() == (n + 63) / 64;
    for (size_t k = 0; k < n && same; k++) same = ((del[k / 64] >> (k % 64)) & 1) == (want[k] ? 1u : 0u);
    CHECK(same);
    if (n > 64) continue;
    // the one-word form the device runs: recount_row per live row
    uint64_t d = 0;
    for (size_t i = 0; i + 1 < n; i++) {
      if (d >> i & 1) continue;
      uint64_t a = 0, b = 0;
      for (size_t j = i + 1; j < n; j++) a |= (uint64_t)(pred[i][j] == 1) << j, b |= (uint64_t)(pred[i][j] == 2) << j;
      d = recount_row(d, (uint32_t)i, a, b);
    }
    CHECK(d == del[0]);
  }
  // the quirk: b beats a, a beats c, b does not beat c — row a goes on after a was deleted and still deletes c: {b} survives
  std::vector<std::vector<int>> q(3, std::vector<int>(3, 0));
  q[0][1] = 2, q[0][2] = 1, q[1][2] = 0;
  std::vector<uint64_t> del;
  recount_eliminate(3, [&](size_t i, size_t j) { return q[i][j]; }, &del);
  CHECK(del[0] == 0b101);
  const std::vector<bool> lit = literal_loop(q);
  CHECK(lit[0] && !lit[1] && lit[2]);
  // ... and through the predicate: reads / ureads a = (100, 1), b = (100, 100), c = (100, 0), nothing shared
  CHECK(recount_pred(100, 1, 100, 100, 0, 0.95, 0.05) == 2);   // (a, b): b beats a
  CHECK(recount_pred(100, 1, 100, 0, 0, 0.95, 0.05) == 1);     // (a, c): a beats c
  CHECK(recount_pred(100, 100, 100, 5, 0, 0.95, 0.05) == 0);   // 5 < 100 * 0.05 is false
  CHECK(recount_pred(100, 100, 100, 4, 0, 0.95, 0.05) == 1);
  CHECK(recount_pred(100, 100, 100, 4, 96, 0.95, 0.05) == 0);  // 95 >= 96 is false: too many shared reads
  CHECK(recount_pred(100, 100, 100, 4, 95, 0.95, 0.05) == 1);
}

static void share_checks() {
  for (uint64_t m = 1; m <= 4096; m++) {
    CHECK(recount_share(m, true) + (m - 1) * recount_share(m, false) == RECOUNT_UNIT);
    if (RECOUNT_UNIT % m == 0) CHECK(recount_share(m, true) == RECOUNT_UNIT / m && recount_share(m, false) == RECOUNT_UNIT / m);
    CHECK(recount_share(m, true) >= recount_share(m, false));
  }
  for (uint64_t m = 1; m <= 16; m++) CHECK(RECOUNT_UNIT % m == 0);
  CHECK(recount_share(17, false) == 42395 && recount_share(17, true) == 720720 - 16 * 42395);
  CHECK(recount_bases(150, 1, 1) == 150 * 65536 && recount_bases(150, 2, 3) == 150 * 65536 / 6 && recount_bases(0xffffffffu, 64, 4096) == 0xffffffffull * 65536 / (64 * 4096));
}

static void order_checks() {
  const double q[] = {0.8, 0.9, 0.8, 0.9, 1.0, 0.8};
  std::vector<uint32_t> o;
  recount_order(q, 6, &o);
  const uint32_t want[] = {4, 1, 3, 0, 2, 5};
  for (int i = 0; i < 6; i++) CHECK(o[i] == want[i]);
  recount_order(q, 1, &o);
  CHECK(o.size() == 1 && o[0] == 0);
}

static void query_checks() {
  // classes 0 = a, 1 = b, 2 = c (the quirk's counts), 3 = d: species 7 for a and b, 9 for c, 0 for d
  const RecountClass cls[] = {{1, 100, 1}, {1, 100, 100}, {1, 100, 0}, {1, 100, 100}};
  std::map<std::pair<uint64_t, int>, uint64_t> got;
  auto add = [&](uint64_t col, int w, uint64_t n) { got[{col, w}] += n; };
  auto none = [](uint32_t, uint32_t) { return (uint64_t)0; };
  RecountParams p;
  bool lost = false;
  // the quirk read: a (two rows), b, c in qCov order -> {b}: unique, hic because 0.8 >= 0.75
  const RecountRow quirk[] = {{0, 7, 0, 0.9, 150}, {0, 7, 1, 0.9, 150}, {1, 7, 2, 0.8, 150}, {2, 9, 3, 0.7, 150}};
  // (b does not beat c: they share more reads than 95% of either's — an implementation that ends row a with a's deletion keeps {b, c})
  auto bc = [](uint32_t x, uint32_t y) { return (uint64_t)(x + y == 3 && x * y == 2 ? 96 : 0); };
  CHECK(recount_pred(100, 100, 100, 0, 96, 0.95, 0.05) == 0);
  CHECK(recount_query(quirk, 4, cls, p, bc, add, &lost) == 1 && lost);
  CHECK(got.size() == 4 && got[{2, RECOUNT_MATCH}] == RECOUNT_UNIT && got[{2, RECOUNT_UNIQ}] == RECOUNT_UNIT && got[{2, RECOUNT_HIC}] == RECOUNT_UNIT &&
        got[{2, RECOUNT_BASES}] == 150 * RECOUNT_BASE_UNIT);
  // without the correction: three survivors, not one species: no uniq; a's two rows share
  got.clear();
  p.no_amb_corr = true;
  CHECK(recount_query(quirk, 4, cls, p, none, add, &lost) == 3 && !lost);
  CHECK(got[{0, RECOUNT_MATCH}] == RECOUNT_UNIT / 2 && got[{1, RECOUNT_MATCH}] == RECOUNT_UNIT / 2 && got[{3, RECOUNT_MATCH}] == RECOUNT_UNIT);
  CHECK(got[{0, RECOUNT_BASES}] == 150 * RECOUNT_BASE_UNIT / 6 && got[{2, RECOUNT_BASES}] == 150 * RECOUNT_BASE_UNIT / 3);
  CHECK(got.count({0, RECOUNT_UNIQ}) == 0 && got.count({2, RECOUNT_UNIQ}) == 0);
  // survivors under one species: the first rows add their match share to uniq, and to hic by their own qCov
  got.clear();
  p.no_amb_corr = false;
  const RecountRow same[] = {{1, 7, 2, 0.9, 100}, {3, 7, 5, 0.7, 100}, {3, 7, 6, 0.9, 100}};
  CHECK(recount_query(same, 3, cls, p, none, add, &lost) == 2 && !lost);
  CHECK(got[{2, RECOUNT_UNIQ}] == RECOUNT_UNIT && got[{2, RECOUNT_HIC}] == RECOUNT_UNIT && got[{5, RECOUNT_UNIQ}] == RECOUNT_UNIT / 2 && got.count({5, RECOUNT_HIC}) == 0 &&
        got.count({6, RECOUNT_UNIQ}) == 0 && got[{6, RECOUNT_MATCH}] == RECOUNT_UNIT / 2);
  // ... not at level strain, and not under species 0
  got.clear();
  p.level_species = false;
  CHECK(recount_query(same, 3, cls, p, none, add, &lost) == 2 && got.count({2, RECOUNT_UNIQ}) == 0);
  got.clear();
  p.level_species = true;
  const RecountRow zero[] = {{1, 0, 2, 0.9, 100}, {3, 0, 5, 0.7, 100}};
  CHECK(recount_query(zero, 2, cls, p, none, add, &lost) == 2 && got.count({2, RECOUNT_UNIQ}) == 0);
  // a shared count above reads * (1 - D) protects the weaker target
  got.clear();
  const RecountRow two[] = {{1, 7, 2, 0.9, 100}, {2, 9, 3, 0.8, 100}};
  CHECK(recount_query(two, 2, cls, p, [](uint32_t, uint32_t) { return (uint64_t)96; }, add, &lost) == 2 && !lost);
  CHECK(recount_query(two, 2, cls, p, [](uint32_t, uint32_t) { return (uint64_t)95; }, add, &lost) == 1 && lost);
  // 17 rows of one target: the first row takes the remainder
  got.clear();
  std::vector<RecountRow> many(17, RecountRow{1, 7, 0, 0.9, 170});
  for (int i = 0; i < 17; i++) many[(size_t)i].column = (uint64_t)i;
  CHECK(recount_query(many.data(), 17, cls, p, none, add, &lost) == 1);
  uint64_t sum = 0;
  for (int i = 0; i < 17; i++) sum += got[{(uint64_t)i, RECOUNT_MATCH}];
  CHECK(sum == RECOUNT_UNIT && got[{0, RECOUNT_MATCH}] == RECOUNT_UNIT - 16 * 42395 && got[{0, RECOUNT_UNIQ}] == RECOUNT_UNIT && got[{5, RECOUNT_BASES}] == 10 * RECOUNT_BASE_UNIT);
}

static void verdict_checks() {
  RecountThresholds th;
  th.min_chunks_reads = 2, th.min_uniq_reads = 3, th.min_hic_ureads = 2, th.min_hic_ureads_prop = 0.5, th.min_chunks_fraction = 1.0, th.max_depth_stdev = 0.5;
  const uint64_t U = RECOUNT_UNIT, B = RECOUNT_BASE_UNIT;
  auto judge = [&](std::vector<uint64_t> w, uint64_t tlen = 1000) {
    return recount_rollup(w.size() / 4, tlen, th, [&](uint64_t c) { return w.data() + c * 4; });
  };
  CHECK(!judge({0, 0, 0, 0, 0, 0, 0, 0}).listed);
  CHECK(judge({2 * U, 3 * U - 1, 3 * U - 1, 100 * B, 2 * U, 0, 0, 100 * B}).verdict == RECOUNT_FEW_UNIQUE);
  CHECK(judge({2 * U, 3 * U, 2 * U - 1, 100 * B, 2 * U, 0, 0, 100 * B}).verdict == RECOUNT_FEW_HIC_UNIQUE);
  CHECK(judge({2 * U, 5 * U, 2 * U, 100 * B, 2 * U, 0, 0, 100 * B}).verdict == RECOUNT_LOW_HIC_PROP);
  CHECK(judge({2 * U, 4 * U, 2 * U, 100 * B, 2 * U - 1, 0, 0, 100 * B}).verdict == RECOUNT_LOW_CHUNKS);
  CHECK(judge({2 * U, 4 * U, 2 * U, 300 * B, 2 * U, 0, 0, 100 * B}).verdict == RECOUNT_OK);           // rel depth 1.5, 0.5: stdev 0.5, not above
  CHECK(judge({2 * U, 4 * U, 2 * U, 301 * B, 2 * U, 0, 0, 99 * B}).verdict == RECOUNT_HIGH_STDEV);
  const RecountRef r = judge({2 * U, 4 * U, 2 * U, 300 * B, 2 * U, 0, 0, 100 * B});
  CHECK(r.listed && r.match == 4 * U && r.chunks_frac == 1.0 && r.depth_stdev == 0.5 && r.coverage == 0.4);
  th.norm = RECOUNT_NORM_MIN;
  CHECK(judge({2 * U, 4 * U, 2 * U, 300 * B, 2 * U, 0, 0, 100 * B}).coverage == 0.2);
  th.norm = RECOUNT_NORM_MAX;
  CHECK(judge({2 * U, 4 * U, 2 * U, 300 * B, 2 * U, 0, 0, 100 * B}).coverage == 0.6);
  // the presets (profile.go:243-313)
  CHECK(refstats_mode(3).min_chunks_reads == 50 && refstats_mode(3).min_uniq_reads == 20 && refstats_mode(3).min_hic_ureads == 5 && refstats_mode(3).min_hic_ureads_prop == 0.1 &&
        refstats_mode(3).max_chunks_depth_stdev == 2);
  CHECK(refstats_mode(0).min_chunks_reads == 1 && refstats_mode(0).max_chunks_depth_stdev == 10 && refstats_mode(5).min_hic_ureads_prop == 0.15 &&
        refstats_mode(5).max_chunks_depth_stdev == 1.5 && refstats_mode(2).min_uniq_reads == 5 && refstats_mode(1).min_chunks_reads == 5 && refstats_mode(4).min_uniq_reads == 50);
}

int main() {
  mask_checks();
  share_checks();
  order_checks();
  query_checks();
  verdict_checks();
  printf("%d checks, %d wrong\n", checks, wrong);
  return wrong ? 1 : 0;
}
