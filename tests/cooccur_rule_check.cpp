// cooccur_rule_check.cpp — kmcp_amd/csrc/cooccur_rule.hpp stand-alone on the host (tests/test_cooccur_rule_cpu.py builds it with the
// address and undefined-behaviour sanitizers): the pair key, the probe sequence of the table, the two-phase count on a table that is too
// small, the pairs of a query and the row cuts of stage 2.
#include <cstdio>
#include <map>
#include <set>
#include <vector>

#include "../kmcp_amd/csrc/cooccur_rule.hpp"

using namespace kmcpg;

static int wrong = 0, checks = 0;
#define CHECK(c)                                             \
  do {                                                       \
    checks++;                                                \
    if (!(c)) {                                              \
      wrong++;                                               \
      printf("line %d: %s\n", __LINE__, #c);                 \
    }                                                        \
  } while (0)

static void key_checks() {
  const uint32_t v[] = {0u, 1u, 2u, 7u, 65535u, 65536u, 0x7fffffffu, 0xfffffffeu, 0xffffffffu};
  std::set<uint64_t> seen;
  for (uint32_t a : v)
    for (uint32_t b : v) {
      if (a == b) continue;
      const uint64_t k = cooccur_key(a, b);
      CHECK(k == cooccur_key(b, a));  // symmetric
      CHECK(k != COOCCUR_EMPTY);      // never the empty slot
      CHECK(cooccur_key_a(k) == (a < b ? a : b) && cooccur_key_b(k) == (a < b ? b : a));  // round trip, the smaller class first
      if (a < b) CHECK(seen.insert(k).second);  // distinct pairs, distinct keys
    }
  // the key's order is (class_a, class_b)'s
  CHECK(cooccur_key(0, 1) < cooccur_key(0, 2) && cooccur_key(0, 0xffffffffu) < cooccur_key(1, 2) && cooccur_key(3, 9) < cooccur_key(4, 5));
}

static void probe_checks() {
  for (uint64_t slots : {1ull, 2ull, 8ull, 1ull << 20}) {
    const uint32_t lg = cooccur_log2(slots), want = cooccur_probes(slots);
    CHECK((1ull << lg) == slots);
    CHECK(want == (slots < K7_PROBES ? slots : K7_PROBES));
    for (uint64_t n = 0; n < 2000; n++) {
      const uint64_t key = cooccur_key((uint32_t)(n * 2654435761u), (uint32_t)(n * 40503u + 1) | 0x80000000u);
      std::set<uint64_t> visited;
      uint64_t i = cooccur_slot0(key, lg);
      for (uint32_t p = 0; p < want; p++, i = cooccur_next(i, slots)) {
        CHECK(i < slots);
        visited.insert(i);
      }
      CHECK(visited.size() == want);  // K7_PROBES distinct slots (every slot of a smaller table)
    }
  }
  // a table of 2^20 slots: the first slots of consecutive pairs spread (no more than a handful share one)
  std::map<uint64_t, int> first;
  int worst = 0;
  for (uint32_t a = 0; a < 300; a++)
    for (uint32_t b = a + 1; b < 300; b++) worst = std::max(worst, ++first[cooccur_slot0(cooccur_key(a, b), 20)]);
  CHECK(worst <= 4);
}

// reads on an 8-slot table, one after the other: each is counted completely or not at all, and what was counted is exact
static void two_phase_checks() {
  const uint64_t slots = 8;
  std::vector<uint64_t> keys(slots, COOCCUR_EMPTY), counts(slots, 0);
  std::map<uint64_t, uint64_t> want;
  const std::vector<std::vector<uint32_t>> reads = {
      {1, 2},            // 1 pair
      {2, 1, 1, 2},      // the same, with repeats: chunks of one target
      {1, 2, 3},         // 3 pairs: 2 new keys
      {5},               // one target: nothing
      {},                // no rows
      {4, 5, 6, 7, 8},   // 10 pairs: cannot fit — LEFT whole, though some of its keys are reserved
      {1, 2, 3},         // still counted: its keys are there
      {1, 2, 3, 4},      // 6 pairs, 3 of them new: fits only if the reserved keys of the LEFT read left room
      {9, 10},           // a new key on a table that may be full
      {1, 3},
  };
  int counted = 0, left = 0;
  for (const auto& r : reads) {
    std::vector<uint32_t> cls = r, again = r;
    const std::vector<uint64_t> before = counts;
    const bool ok = cooccur_count_read(keys.data(), counts.data(), slots, cls.data(), cls.size());
    if (ok) {
      counted++;
      cooccur_query_pairs(again.data(), again.size(), [&](uint64_t k) { want[k]++; });
    } else {
      left++;
      CHECK(counts == before);  // nothing of it was counted
    }
    // after every read: the counted slots are exactly the brute force over the counted reads
    std::map<uint64_t, uint64_t> got;
    for (uint64_t i = 0; i < slots; i++) {
      CHECK(keys[i] != COOCCUR_EMPTY || counts[i] == 0);
      if (counts[i]) CHECK(got.emplace(keys[i], counts[i]).second);  // a key lives in one slot
    }
    CHECK(got == want);
  }
  CHECK(left >= 1 && counted >= 6);
  CHECK(want[cooccur_key(1, 2)] >= 3 && want[cooccur_key(2, 3)] >= 2);
  // reserve is idempotent, find finds what reserve reserved and nothing else
  for (uint64_t i = 0; i < slots; i++)
    if (keys[i] != COOCCUR_EMPTY) {
      CHECK(cooccur_reserve(keys.data(), slots, keys[i]) == (int64_t)i);
      CHECK(cooccur_find(keys.data(), slots, keys[i]) == (int64_t)i);
    }
  CHECK(cooccur_find(keys.data(), slots, cooccur_key(100, 200)) == -1);
  // a table of one slot holds one key
  uint64_t one = COOCCUR_EMPTY;
  CHECK(cooccur_reserve(&one, 1, cooccur_key(1, 2)) == 0 && cooccur_reserve(&one, 1, cooccur_key(2, 1)) == 0 && cooccur_reserve(&one, 1, cooccur_key(1, 3)) == -1);
}

static void query_checks() {
  std::vector<uint32_t> cls = {7, 3, 7, 9, 3};
  std::vector<uint64_t> got;
  CHECK(cooccur_query_pairs(cls.data(), cls.size(), [&](uint64_t k) { got.push_back(k); }) == 3);
  CHECK((got == std::vector<uint64_t>{cooccur_key(3, 7), cooccur_key(3, 9), cooccur_key(7, 9)}));
  std::vector<uint32_t> one = {4, 4, 4}, none;
  got.clear();
  CHECK(cooccur_query_pairs(one.data(), one.size(), [&](uint64_t k) { got.push_back(k); }) == 1 && got.empty());
  CHECK(cooccur_query_pairs(none.data(), 0, [&](uint64_t k) { got.push_back(k); }) == 0 && got.empty());
}

// the row cuts: (target kept, new name, qCov) -> (joins the set, opens a query)
struct Row {
  bool kept, new_name;
  double qcov;
  bool take, opens;
};
static void cut_rows(CooccurCut c, const std::vector<Row>& rows, int line) {
  for (const Row& r : rows) {
    bool opens = !r.opens;
    const bool take = c.row(r.kept, r.new_name, r.qcov, &opens);
    checks++;
    if (take != r.take || opens != r.opens) {
      wrong++;
      printf("line %d: row (%d, %d, %g): take %d opens %d\n", line, r.kept, r.new_name, r.qcov, take, opens);
    }
  }
}
static void cut_checks() {
  CooccurCut plain;
  cut_rows(plain, {{true, true, 0.9, true, true}, {false, true, 1.0, false, false}, {true, false, 0.1, true, false}, {true, true, 0.5, true, true}}, __LINE__);
  CooccurCut perfect;
  perfect.cut.keep_perfect = true;
  // a dropped first row with qCov 1 does not become the previous score; the first kept row is never tested; once cut, cut
  cut_rows(perfect, {{false, true, 1.0, false, false}, {true, true, 0.9, true, true}, {true, false, 0.9, true, false},
                     {true, true, 1.0, true, true}, {true, false, 1.0, true, false}, {true, false, 0.9, false, false}, {true, false, 1.0, false, false}}, __LINE__);
  CooccurCut main_;
  main_.cut.keep_main = true, main_.cut.max_gap = 0.4;
  // the gap is taken to the previous KEPT target's row
  cut_rows(main_, {{true, true, 1.0, true, true}, {false, false, 0.7, false, false}, {true, false, 0.58, false, false}, {true, false, 0.9, false, false},
                   {true, true, 1.0, true, true}, {true, false, 0.7, true, false}, {true, false, 0.58, true, false}}, __LINE__);
  CooccurCut top;
  top.cut.top_n = 1;
  // the first row counts as one; a tie is not a smaller score; a dropped target's smaller score is not counted
  cut_rows(top, {{true, true, 0.9, true, true}, {true, false, 0.9, true, false}, {false, false, 0.8, false, false}, {true, false, 0.9, true, false},
                 {true, false, 0.8, false, false}, {true, false, 0.9, false, false}}, __LINE__);
}

int main() {
  key_checks();
  probe_checks();
  two_phase_checks();
  query_checks();
  cut_checks();
  printf("%d checks, %d wrong\n", checks, wrong);
  return wrong ? 1 : 0;
}
