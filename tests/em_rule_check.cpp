// em_rule_check.cpp — kmcp_amd/csrc/em_rule.hpp stand-alone on the host (tests/test_em_rule_cpu.py builds it with the address and
// undefined-behaviour sanitizers): on random reads the conservation law (every assigned read adds exactly EM_UNIT to match), a target's rows
// summing to its p, the two-word bases against unsigned __int128, the placement of the deficit, uniq and hic; the quota's edges; the
// roll-up, the loop's three ways to stop and the end's order and -F.
#include <cstdio>
#include <map>
#include <random>
#include <vector>

#include "../kmcp_amd/csrc/em_rule.hpp"

using namespace kmcpg;

static int wrong = 0, checks = 0;
#define CHECK(...)                                     \
  do {                                                 \
    checks++;                                          \
    if (!(__VA_ARGS__)) {                              \
      wrong++;                                         \
      printf("line %d: %s\n", __LINE__, #__VA_ARGS__); \
    }                                                  \
  } while (0)

typedef unsigned __int128 u128;
constexpr uint32_t N_CLASSES = 40;

static void quota_checks() {
  CHECK(EM_UNIT == 720720ull * 4096 && EM_UNIT < (1ull << 32));
  CHECK(em_quota(1.0, 1.0) == EM_UNIT && em_quota(1.0, 2.0) == EM_UNIT / 2 && em_quota(1.0, 4.0) == EM_UNIT / 4);
  CHECK(em_quota(1e-9, 1e6 + 1e-9) == 0);  // 1e-15 of 2.95e9 units
  CHECK(em_quota(1.0, INFINITY) == 0);
  CHECK(em_quota(2.0, 1.0) == EM_UNIT);  // (never: a target's coverage is part of the sum)
  CHECK(em_quota(1.0, 3.0) == (uint64_t)(1.0 / 3.0 * (double)EM_UNIT));
  for (uint64_t m = 1; m <= 64; m++)
    for (uint64_t p : {(uint64_t)0, (uint64_t)1, (uint64_t)63, (uint64_t)1000003, EM_UNIT - 1, EM_UNIT}) {
      CHECK(em_row_share(p, m, true) + (m - 1) * em_row_share(p, m, false) == p);
      CHECK(em_row_share(p, m, true) >= em_row_share(p, m, false));
    }
  for (uint64_t m = 1; m <= 4096; m++) CHECK(em_single_share(m, true) + (m - 1) * em_single_share(m, false) == EM_UNIT);
  uint64_t lo, hi;
  em_bases(0x7fffffffull, EM_UNIT, &lo, &hi);
  CHECK((((u128)hi << 32) | lo) == (u128)0x7fffffffull * EM_UNIT && hi > 0 && lo < (1ull << 32) && hi < (1ull << 32));
  em_bases(~0ull, EM_UNIT, &lo, &hi);  // clamped to 2^32 - 1: the product stays below 2^64
  CHECK((((u128)hi << 32) | lo) == (u128)0xffffffffull * EM_UNIT);
  CHECK(em_bases_value(lo, hi) == (double)0xffffffffull);
  em_bases(150, 7, &lo, &hi);
  CHECK(lo == 1050 && hi == 0);
}

static void read_checks() {
  std::mt19937_64 rng(11);
  const double covs[] = {1e-9, 1e-3, 0.5, 1.0, 3.0, 17.25, 1e6};
  uint64_t reads = 0, split = 0, zero_shares = 0, capped = 0;
  for (int round = 0; round < 20000; round++) {
    std::vector<double> cov(N_CLASSES);
    for (auto& c : cov) c = round % 3 == 0 ? covs[rng() % 7] : (double)(rng() % 100000 + 1) / 997.0;
    const size_t n = round < 100 ? (size_t)(round % 5) : (size_t)(rng() % 64) + 1;
    const uint32_t spread = (uint32_t)(rng() % 8) + 1;
    const bool one_species = rng() % 2, level_species = rng() % 4 != 0;
    std::vector<RecountRow> rows(n);
    for (size_t i = 0; i < n; i++)
      rows[i] = RecountRow{(uint32_t)(rng() % spread) * 3 % N_CLASSES, one_species ? 5u : (uint32_t)(rng() % 3), (uint64_t)i, (double)(rng() % 101) / 100.0,
                           round % 7 == 0 ? 0x7fffffffull : rng() % 300};
    std::map<uint64_t, std::vector<uint64_t>> got;
    const size_t nt = em_query(rows.data(), n, cov.data(), 0.75, level_species, [&](uint64_t col, int w, uint64_t x) {
      auto& v = got[col];
      v.resize(EM_WORDS, 0);
      v[(size_t)w] += x;
    });
    // the targets, by hand
    std::vector<uint32_t> tcls;
    std::vector<std::vector<size_t>> trows;
    for (size_t i = 0; i < n; i++) {
      size_t t = 0;
      while (t < tcls.size() && tcls[t] != rows[i].target_class) t++;
      if (t == tcls.size()) tcls.push_back(rows[i].target_class), trows.emplace_back();
      trows[t].push_back(i);
    }
    CHECK(nt == tcls.size());
    if (nt == 0) {
      CHECK(got.empty());
      continue;
    }
    reads++;
    uint64_t match = 0;
    for (auto& kv : got) match += kv.second[EM_MATCH];
    CHECK(match == EM_UNIT);  // the conservation law
    // p by hand: quotas, the cap in first-row order, the deficit to the first target
    std::vector<uint64_t> p(nt, EM_UNIT);
    bool same = true, none = false;
    if (nt > 1) {
      split++;
      double s = 0;
      for (size_t t = 0; t < nt; t++) s += cov[tcls[t]];
      uint64_t total = 0;
      for (size_t t = 0; t < nt; t++) p[t] = em_quota(cov[tcls[t]], s), total += p[t], zero_shares += p[t] == 0;
      if (total > EM_UNIT) {
        capped++;
        uint64_t room = EM_UNIT;
        for (size_t t = 0; t < nt; t++) p[t] = std::min(p[t], room), room -= p[t];
        total = EM_UNIT - room;
      }
      CHECK(EM_UNIT - total <= nt);  // every floor loses less than a unit
      p[0] += EM_UNIT - total;
      for (size_t t = 0; t < nt; t++) same = same && rows[trows[t][0]].species_class == rows[trows[0][0]].species_class, none = none || rows[trows[t][0]].species_class == 0;
    }
    const bool uniq_first = nt == 1 || (level_species && same && !none);
    for (size_t t = 0; t < nt; t++) {
      uint64_t sum = 0;
      u128 bases = 0, want = 0;
      const size_t m = trows[t].size();
      for (size_t k = 0; k < m; k++) {
        const RecountRow& r = rows[trows[t][k]];
        const auto& v = got[r.column];
        sum += v[EM_MATCH];
        bases += ((u128)v[EM_BASES_HI] << 32) + v[EM_BASES_LO];
        want += (u128)r.qlen * v[EM_MATCH];
        CHECK(v[EM_BASES_LO] < (1ull << 32) && v[EM_BASES_HI] < (1ull << 32));
        CHECK(v[EM_MATCH] == (nt == 1 ? em_single_share(m, k == 0) : em_row_share(p[t], m, k == 0)));
        const uint64_t u = k == 0 && uniq_first ? (nt == 1 ? EM_UNIT : v[EM_MATCH]) : 0;
        CHECK(v[EM_UNIQ] == u && v[EM_HIC] == (r.qcov >= 0.75 ? u : 0));
      }
      CHECK(sum == p[t]);     // a target's rows sum to its p
      CHECK(bases == want);   // nothing is rounded
    }
  }
  printf("%llu reads, %llu split, %llu zero shares, %llu capped\n", (unsigned long long)reads, (unsigned long long)split, (unsigned long long)zero_shares, (unsigned long long)capped);
  CHECK(split > 5000 && zero_shares > 100);
  // 1e-9 beside 1e6: the small target's share is 0, the deficit goes to the FIRST target — the small one when it comes first
  std::vector<double> cov(N_CLASSES, 1.0);
  cov[1] = 1e-9, cov[2] = 1e6;
  for (int swap = 0; swap < 2; swap++) {
    const RecountRow two[] = {{swap ? 2u : 1u, 0, 0, 0.9, 100}, {swap ? 1u : 2u, 0, 1, 0.9, 100}};
    uint64_t match[2] = {};
    em_query(two, 2, cov.data(), 0.75, true, [&](uint64_t col, int w, uint64_t x) { if (w == EM_MATCH) match[col] += x; });
    const uint64_t big = em_quota(1e6, swap ? 1e6 + 1e-9 : 1e-9 + 1e6), small = em_quota(1e-9, 1e6 + 1e-9);
    CHECK(small == 0 && big <= EM_UNIT && match[0] + match[1] == EM_UNIT);
    CHECK(swap ? (match[0] == EM_UNIT && match[1] == 0) : (match[0] == EM_UNIT - big && match[1] == big));
  }
}

// a pass for the loop's checks: class c has two chunks, columns 2c and 2c + 1; the reads are 1000 per class, `shared` of them split with
// class 0 by coverage (a toy model: the loop, not the rule, is under test)
static void loop_checks() {
  std::vector<EmClass> classes(3);
  for (size_t c = 0; c < 3; c++) classes[c].columns = {2 * c, 2 * c + 1}, classes[c].tlen = 1000 * (c + 1), classes[c].name = std::string(1, (char)('c' - c));
  int calls = 0;
  auto pass = [&](const std::vector<uint8_t>& est, const std::vector<double>& cov, std::vector<EmChunk>* cols, uint64_t* assigned) {
    calls++;
    cols->assign(6, EmChunk());
    *assigned = 0;
    for (size_t c = 0; c < 3; c++) {
      if (!est[c]) continue;
      uint64_t reads = 1000;
      if (c > 0 && est[0]) reads = 600 + (uint64_t)(400.0 * cov[c] / (cov[c] + cov[0]));
      for (size_t o = 1; o < 3 && c == 0; o++) {
        if (est[o]) reads += 400 - (uint64_t)(400.0 * cov[o] / (cov[o] + cov[0]));
      }
      for (size_t k = 0; k < 2; k++) {
        EmChunk& w = (*cols)[2 * c + k];
        w.match = reads / 2 * EM_UNIT, w.uniq = 300 * EM_UNIT, w.hic = c == 2 ? 0 : 200 * EM_UNIT;
        w.single_bases = reads / 2 * 150 * RECOUNT_BASE_UNIT;
      }
      *assigned += reads;
    }
    return 0;
  };
  EmParams p;
  EmResult res;
  // class 2 has no hic: it fails few-hic-unique after pass 0 and leaves for good; the loop converges
  CHECK(em_run(classes, {1, 1, 1}, {1.0, 1.0, 1.0}, p, pass, &res) == 0);
  CHECK(res.refs[2].verdict == RECOUNT_FEW_HIC_UNIQUE && !res.est[2] && res.est[0] && res.est[1]);
  CHECK(res.converged && res.passes >= 2 && res.passes == calls && res.passes <= 11);
  CHECK(std::fabs(res.refs[0].percentage + res.refs[1].percentage - 100) < 1e-9);
  CHECK(res.refs[0].chunks_frac == 1.0 && res.refs[0].depth_stdev == 0 && res.refs[0].rel_depth.size() == 2 && res.refs[0].rel_depth[0] == 1.0);
  const int free_passes = res.passes;
  // -I 1: two passes at most
  p.max_iters = 1, p.pct_threshold = 0;
  calls = 0;
  CHECK(em_run(classes, {1, 1, 1}, {1.0, 1.0, 1.0}, p, pass, &res) == 0);
  CHECK(res.passes == 2 && calls == 2 && !res.converged && free_passes >= 2);
  // nothing on the whitelist: no pass at all; every reference failing after pass 0: one pass, an empty table
  calls = 0;
  CHECK(em_run(classes, {0, 0, 0}, {1.0, 1.0, 1.0}, p, pass, &res) == 0 && res.passes == 0 && calls == 0);
  p.th.min_uniq_reads = 1000;
  CHECK(em_run(classes, {1, 1, 0}, {1.0, 1.0, 1.0}, p, pass, &res) == 0 && res.passes == 1 && !res.converged);
  CHECK(res.refs[0].verdict == RECOUNT_FEW_UNIQUE && em_finish(classes, 0, &res).empty());
  // a failing pass ends the loop with its code
  CHECK(em_run(classes, {1, 1, 0}, {1.0, 1.0, 1.0}, p, [](const std::vector<uint8_t>&, const std::vector<double>&, std::vector<EmChunk>*, uint64_t*) { return -4; }, &res) == -4);
  // the end: coverage descending, chunksFrac descending, name ascending; -F drops the tail that sums to at most X and renormalises
  res.est = {1, 1, 1};
  res.refs.assign(3, EmRef());
  res.refs[0].coverage = 1, res.refs[0].chunks_frac = 0.5, res.refs[0].percentage = 10;
  res.refs[1].coverage = 1, res.refs[1].chunks_frac = 0.5, res.refs[1].percentage = 10;  // name "b" before "c"
  res.refs[2].coverage = 8, res.refs[2].chunks_frac = 0.1, res.refs[2].percentage = 80;
  CHECK(em_finish(classes, 0, &res) == std::vector<uint32_t>({2, 1, 0}));
  res.refs[0].chunks_frac = 0.6;
  CHECK(em_finish(classes, 0, &res) == std::vector<uint32_t>({2, 0, 1}));
  CHECK(em_finish(classes, 9.9, &res) == std::vector<uint32_t>({2, 0, 1}) && res.refs[2].percentage == 80);
  EmResult one = res;
  CHECK(em_finish(classes, 10, &one) == std::vector<uint32_t>({2, 0}) && one.refs[2].percentage == 8.0 / 9.0 * 100 && one.refs[0].percentage == 1.0 / 9.0 * 100);
  one = res;
  CHECK(em_finish(classes, 99.9, &one) == std::vector<uint32_t>({2}) && one.refs[2].percentage == 100);
  one = res;
  one.est = {0, 0, 1};
  CHECK(em_finish(classes, 99.9, &one) == std::vector<uint32_t>({2}) && one.refs[2].percentage == 80);  // one reference left: -F does not act
  // the roll-up: --norm-abund and the verdicts in the reference's order
  RecountThresholds th;
  th.min_chunks_reads = 2, th.min_uniq_reads = 3, th.min_hic_ureads = 2, th.min_hic_ureads_prop = 0.5, th.min_chunks_fraction = 1.0, th.max_depth_stdev = 0.5;
  const uint64_t U = EM_UNIT, B = RECOUNT_BASE_UNIT;
  auto judge = [&](std::vector<EmChunk> w, bool j = true) { return em_rollup(w.size(), 1000, th, j, [&](uint64_t c) { return w[(size_t)c]; }); };
  CHECK(!judge({EmChunk(), EmChunk()}).listed);
  CHECK(judge({{2 * U, 3 * U - 1, 3 * U - 1, 100 * B, 0, 0}, {2 * U, 0, 0, 100 * B, 0, 0}}).verdict == RECOUNT_FEW_UNIQUE);
  CHECK(judge({{2 * U, 3 * U - 1, 3 * U - 1, 100 * B, 0, 0}, {2 * U, 0, 0, 100 * B, 0, 0}}, false).verdict == RECOUNT_OK);  // only after pass 0
  CHECK(judge({{2 * U, 3 * U, 2 * U - 1, 100 * B, 0, 0}, {2 * U, 0, 0, 100 * B, 0, 0}}).verdict == RECOUNT_FEW_HIC_UNIQUE);
  CHECK(judge({{2 * U, 5 * U, 2 * U, 100 * B, 0, 0}, {2 * U, 0, 0, 100 * B, 0, 0}}).verdict == RECOUNT_LOW_HIC_PROP);
  CHECK(judge({{2 * U, 4 * U, 2 * U, 100 * B, 0, 0}, {2 * U - 1, 0, 0, 100 * B, 0, 0}}).verdict == RECOUNT_LOW_CHUNKS);
  // 200 bases from single-target reads + 100 from the pass (100 * EM_UNIT = hi 68, lo 3157057536) against 100: rel depth 1.5, 0.5
  const uint64_t lo = (100 * U) & 0xffffffffull, hi = (100 * U) >> 32;
  const EmRef r = judge({{2 * U, 4 * U, 2 * U, 200 * B, lo, hi}, {2 * U, 0, 0, 100 * B, 0, 0}});
  CHECK(r.verdict == RECOUNT_OK && r.match == 4 * U && r.chunks_frac == 1.0 && r.depth_stdev == 0.5 && r.coverage == 0.4 && r.rel_depth[0] == 1.5);
  CHECK(judge({{2 * U, 4 * U, 2 * U, 201 * B, lo, hi}, {2 * U, 0, 0, 99 * B, 0, 0}}).verdict == RECOUNT_HIGH_STDEV);
  th.norm = RECOUNT_NORM_MIN;
  CHECK(judge({{2 * U, 4 * U, 2 * U, 200 * B, lo, hi}, {2 * U, 0, 0, 100 * B, 0, 0}}).coverage == 0.2);
  th.norm = RECOUNT_NORM_MAX;
  CHECK(judge({{2 * U, 4 * U, 2 * U, 200 * B, lo, hi}, {2 * U, 0, 0, 100 * B, 0, 0}}).coverage == 0.6);
}

int main() {
  quota_checks();
  read_checks();
  loop_checks();
  printf("%d checks, %d wrong\n", checks, wrong);
  return wrong ? 1 : 0;
}
