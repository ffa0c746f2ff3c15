// build_plan_check.cpp — kmcp_amd/csrc/build_plan.hpp compiled for the host (tests/test_build_plan_cpu.py; go_pow comes from
// kmcp_amd/csrc/fpr.cpp, compiled beside it): no HIP is needed to lay out a database.  Reads cases
//   "n_cols threads block_size kmers_x block_size_x kmers_8 kmers_1 uniform_sigs num_hashes fpr budget"
//   "count[0] ... count[n_cols - 1]"
//   "n_blocks n_rounds"                      (n_rounds -1: the budget is below a block, build_rounds must refuse and name the budget)
//   "block[0] pos[0] ... "                   (per column: block, -1 = in none, and place in the block)
//   "num_sigs[0] round[0] ..."               (per block)
// from the file named on the command line — what the test expects from the oracle's layout and its own restatement of the rounds — and
// compares build_plan / build_rounds with every one; then invariants of its own (every non-empty column in exactly one block, blocks
// ascending by count, row_bytes and matrix_bytes as defined, no round above the budget).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../kmcp_amd/csrc/build_plan.hpp"

using namespace kmcpg;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  unsigned long long cases = 0, bad = 0;
  unsigned long long n, kx, k8, k1, budget;
  int threads, bs, bsx, uni, nh;
  double fpr;
  while (fscanf(f, "%llu %d %d %llu %d %llu %llu %d %d %lf %llu", &n, &threads, &bs, &kx, &bsx, &k8, &k1, &uni, &nh, &fpr, &budget) == 11) {
    std::vector<uint64_t> counts(n);
    for (auto& c : counts) {
      unsigned long long v;
      if (fscanf(f, "%llu", &v) != 1) return 2;
      c = v;
    }
    long long want_blocks, want_rounds;
    if (fscanf(f, "%lld %lld", &want_blocks, &want_rounds) != 2) return 2;
    std::vector<long long> wb(n), wp(n), ws(want_blocks), wr(want_blocks);
    for (size_t i = 0; i < n; i++)
      if (fscanf(f, "%lld %lld", &wb[i], &wp[i]) != 2) return 2;
    for (long long b = 0; b < want_blocks; b++)
      if (fscanf(f, "%lld %lld", &ws[b], &wr[b]) != 2) return 2;
    kmcpg_build_cfg cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.k = 21;
    cfg.canonical = 1;
    cfg.num_hashes = nh;
    cfg.fpr = fpr;
    cfg.threads = threads;
    cfg.block_size = bs;
    cfg.kmers_x = kx;
    cfg.block_size_x = bsx;
    cfg.kmers_8 = k8;
    cfg.kmers_1 = k1;
    cfg.uniform_sigs = uni;
    BuildPlan plan;
    bool ok = build_cfg_error(cfg).empty() && build_plan(counts.data(), (uint32_t)n, cfg, &plan).empty();
    ok = ok && (long long)plan.blocks.size() == want_blocks;
    std::vector<long long> gb(n, -1), gp(n, -1);
    uint64_t prev = 0, total = 0;
    for (size_t b = 0; ok && b < plan.blocks.size(); b++) {
      const PlanBlock& pb = plan.blocks[b];
      ok = !pb.cols.empty() && pb.row_bytes == (pb.cols.size() + 7) / 8 && pb.matrix_bytes == pb.num_sigs * pb.row_bytes && (long long)pb.num_sigs == ws[b];
      for (size_t j = 0; ok && j < pb.cols.size(); j++) {
        const uint32_t c = pb.cols[j];
        ok = c < n && gb[c] < 0 && counts[c] > 0 && counts[c] >= prev;
        if (ok) {
          gb[c] = (long long)b;
          gp[c] = (long long)j;
          prev = counts[c];
        }
      }
    }
    for (size_t i = 0; ok && i < n; i++) {
      ok = gb[i] == wb[i] && gp[i] == wp[i] && (counts[i] == 0) == (gb[i] < 0);
      total += counts[i];
    }
    ok = ok && plan.total_kmers == total;
    if (ok) {
      std::vector<uint32_t> round;
      uint32_t nr = 0;
      const std::string err = build_rounds(plan, budget, &round, &nr);
      if (want_rounds < 0) {
        char num[32];
        snprintf(num, sizeof num, "%llu", budget);
        ok = !err.empty() && err.find(num) != std::string::npos && err.find("block ") != std::string::npos;
      } else {
        ok = err.empty() && (long long)nr == want_rounds;
        std::vector<uint64_t> used(nr, 0);
        for (size_t b = 0; ok && b < round.size(); b++) {
          ok = round[b] == wr[b] && round[b] < nr && (b == 0 || round[b] == round[b - 1] || round[b] == round[b - 1] + 1);
          if (ok) used[round[b]] += plan.blocks[b].matrix_bytes + 8;
        }
        for (uint64_t u : used) ok = ok && u > 0 && u <= budget;
      }
    }
    if (!ok && bad++ < 10) fprintf(stderr, "wrong: case %llu (%llu columns, -j %d -b %d, uniform_sigs %d, budget %llu)\n", cases, n, threads, bs, uni, budget);
    cases++;
  }
  fclose(f);
  printf("%llu cases, %llu wrong\n", cases, bad);
  return bad ? 1 : 0;
}
