// match_rule_check.cpp — kmcp_amd/csrc/match_rule.hpp behind thin C functions, built as a shared object with g++ and driven by
// tests/test_match_rule_cpu.py, which holds every answer against its own restatement of the reference's rule.  Nothing is decided here.
#include <stdint.h>

#include "../kmcp_amd/csrc/match_rule.hpp"

using namespace kmcpg;

namespace {
struct Meta {
  uint64_t size, gsize;
  uint32_t tidx;
};
}  // namespace

extern "C" void mr_values(uint32_t col, int32_t count, int32_t n, uint64_t size, uint64_t gsize, uint32_t tidx, double fpr, kmcpg_match* out) {
  *out = match_values(col, count, n, Meta{size, gsize, tidx}, fpr);
}

// the four tests; queryFPR answers `fpr`, and *fpr_asked counts how often it was asked
extern "C" int mr_accept(uint32_t col, int32_t count, int32_t n, uint64_t size, uint64_t gsize, uint32_t tidx, const kmcpg_params* p, double fpr,
                         int32_t* fpr_asked, kmcpg_match* out) {
  const auto fpr_of = [&](int, int) {
    ++*fpr_asked;
    return fpr;
  };
  return match_accept(col, count, n, Meta{size, gsize, tidx}, *p, fpr_of, out) ? 1 : 0;
}

extern "C" double mr_score(const kmcpg_match* m, int32_t sort_by) { return match_score(*m, sort_by); }
extern "C" int mr_less(const kmcpg_match* x, const kmcpg_match* y, int32_t sort_by) { return match_less(*x, *y, sort_by) ? 1 : 0; }
extern "C" void mr_sort(kmcpg_match* rec, uint64_t m, const kmcpg_params* p) { sort_matches(rec, rec + m, *p); }
extern "C" void mr_sort_indices(uint32_t* idx, uint64_t m, const kmcpg_match* rec, const kmcpg_params* p) { sort_matches(idx, idx + m, rec, *p); }
extern "C" int mr_top_on(const kmcpg_params* p) { return top_scores_on(*p) ? 1 : 0; }
extern "C" uint64_t mr_top_batch(const kmcpg_match* rec, uint64_t m, const kmcpg_params* p) { return top_scores_keep(rec, m, *p); }

// TopScores fed one record at a time, as the grouped driver feeds it while the records go out: kept until the cut
extern "C" uint64_t mr_top_stream(const kmcpg_match* rec, uint64_t m, const kmcpg_params* p) {
  TopScores top(p->top_n_scores);
  uint64_t kept = 0;
  bool cut = false;
  for (uint64_t i = 0; i < m; i++) {
    if (cut) continue;
    kept++;
    if (top_scores_on(*p) && top.last_kept(match_score(rec[i], p->sort_by))) cut = true;
  }
  return kept;
}
