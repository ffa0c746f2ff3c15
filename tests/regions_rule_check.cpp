// regions_rule_check.cpp — the streaming merger of kmcp_amd/csrc/regions_rule.hpp keeps its state across batches: one sequence of window
// summaries, handed over in two batches cut at EVERY position (and in batches of one), must give the bytes it gives in one batch.  Also
// the hand-written parser of the default query-name pattern on names at its edges.  A program of its own (tests/test_regions_rule_cpu.py
// builds it with the address and undefined-behaviour sanitizers).
#include <stdio.h>

#include <random>
#include <string>
#include <vector>

#include "../kmcp_amd/csrc/regions_rule.hpp"

using namespace kmcpg;

struct Win {
  std::string ref;
  int64_t begin, end;
  uint32_t n;  // 0: a window without a summary (dropped or unmatched): it is not handed to the merger
  double score;
};

static std::string run(const std::vector<Win>& w, const RegionParams& p, const std::vector<size_t>& cuts) {
  RegionMerger m(p);
  std::string all;
  size_t at = 0;
  for (size_t c = 0; c <= cuts.size(); c++) {
    const size_t to = c < cuts.size() ? cuts[c] : w.size();
    std::string bed;  // a batch's lines: a buffer of its own, as a caller that writes per batch has
    for (; at < to; at++)
      if (w[at].n) m.add(w[at].ref.data(), w[at].ref.size(), w[at].begin, w[at].end, w[at].n, w[at].score, &bed);
    all += bed;
  }
  m.finish(&all);
  return all;
}

int main() {
  unsigned long wrong = 0, checked = 0;
  std::mt19937_64 rng(7);
  for (int round = 0; round < 200; round++) {
    std::vector<Win> w;
    const size_t n = 1 + rng() % 40;
    int64_t begin = 1;
    std::string ref = "chr1";
    for (size_t i = 0; i < n; i++) {
      if (rng() % 12 == 0) ref = rng() % 2 ? "chr2" : "chr1", begin = 1;
      const uint32_t nt = rng() % 5 == 0 ? 0 : (rng() % 3 == 0 ? 2 + (uint32_t)(rng() % 3) : 1);
      w.push_back({ref, begin, begin + 99, nt, (double)(5500 + rng() % 4501) / 10000.0});
      begin += 1 + (int64_t)(rng() % 150);
    }
    RegionParams p;
    p.min_overlap = rng() % 2 ? 20 : 1;
    p.max_gap = (int64_t)(rng() % 3) * 30;
    p.ignore_type = rng() % 2;
    const std::string one = run(w, p, {});
    for (size_t cut = 0; cut <= n; cut++) {
      checked++;
      if (run(w, p, {cut}) != one) wrong++;
    }
    std::vector<size_t> every;
    for (size_t i = 1; i < n; i++) every.push_back(i);
    checked++;
    if (run(w, p, every) != one) wrong++;
  }
  // a merger that finished an input starts the next one clean
  {
    RegionMerger m;
    std::string a, b;
    m.add("c", 1, 1, 100, 1, 0.8, &a);
    m.finish(&a);
    m.add("c", 1, 11, 110, 1, 0.8, &b);
    m.finish(&b);
    checked++;
    if (a != "c\t0\t100\tassembly-specific\t800\t.\n" || b != "c\t10\t110\tassembly-specific\t800\t.\n" || m.n_regions != 2) wrong++;
  }
  // the default pattern by hand
  struct Name {
    const char* q;
    bool ok;
    const char* ref;
    int64_t b, e;
  };
  const Name names[] = {{"c_sliding:1-100", true, "c", 1, 100},
                        {"a_sliding:5-9_sliding:11-110", true, "a_sliding:5-9", 11, 110},
                        {"_sliding:1-100", false, "", 0, 0},
                        {"c_sliding:1-", false, "", 0, 0},
                        {"c_sliding:-5", false, "", 0, 0},
                        {"c_sliding:1-100 ", false, "", 0, 0},
                        {"c_sliding:1-1x", false, "", 0, 0},
                        {"c_sliding:1--1", false, "", 0, 0},
                        {"c_sliding:", false, "", 0, 0},
                        {"", false, "", 0, 0},
                        {"x", false, "", 0, 0},
                        {"c_sliding:007-99999999999999999999999", true, "c", 7, INT64_MAX}};
  for (const Name& t : names) {
    // the name in a buffer of exactly its size: a read past either end is the sanitizer's to find
    std::vector<char> buf(t.q, t.q + strlen(t.q));
    size_t rn = 0;
    int64_t b = 0, e = 0;
    const bool ok = region_default_name(buf.data(), buf.size(), &rn, &b, &e);
    checked++;
    if (ok != t.ok || (ok && (std::string(buf.data(), rn) != t.ref || b != t.b || e != t.e))) {
      wrong++;
      printf("name \"%s\": ok=%d ref_n=%zu begin=%lld end=%lld\n", t.q, (int)ok, rn, (long long)b, (long long)e);
    }
  }
  // a summary: A B A -> n = 2, rows 1 and 2; and more distinct classes than the small list holds
  {
    WindowSummaryAcc acc;
    acc.add(7, 0.9), acc.add(3, 0.6), acc.add(7, 0.7);
    checked++;
    if (acc.n != 2 || acc.score() != (0.9 + 0.6) / 2) wrong++;
    acc.clear();
    double sum = 0;
    for (uint32_t i = 0; i < 100; i++) {
      acc.add(i % 50, 0.01 * (i + 1));
      if (i < 50) sum = i == 0 ? 0.01 : sum + 0.01 * (i + 1);
    }
    checked++;
    if (acc.n != 50 || acc.score() != sum / 50) wrong++;
  }
  printf("%lu checked, %lu wrong\n", checked, wrong);
  return wrong ? 1 : 0;
}
