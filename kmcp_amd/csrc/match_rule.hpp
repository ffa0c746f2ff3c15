// match_rule.hpp — which hits become matches, what a Match holds, how a query's matches are ordered and what --keep-top-scores keeps of
// them: the one statement of the host half's rule, used by both drivers of finalize.cpp and by kmcpg_expand_pairs, and compiled alone by
// tests/match_rule_check.cpp.  Host only, no HIP.  Reference: util-db-search.go:7467-7489 (tests and values), :105-145 (order),
// :285-311 (top-N).  k3_keys.hpp holds the device's view of the order; the two must agree bit for bit.
//
// A column's metadata is anything with .size (its k-mers), .gsize and .tidx; n is the query's NumKmers.  fpr_of(n, count) is queryFPR.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "../../include/kmcp_gpu.h"

namespace kmcpg {

// queryFPR for a query without k-mers is 1 (fpr_of is never asked); for every other query it is asked only once -T has passed
template <class FprOf>
inline double match_fpr(int n, int count, FprOf&& fpr_of) { return n > 0 ? fpr_of(n, count) : 1.0; }

// The Match of `count` shared k-mers between a query of n and column `col` (:7479-7489).  No test is applied.
template <class Meta>
inline kmcpg_match match_values(uint32_t col, int count, int n, const Meta& cm, double fpr) {
  const double c = (double)count, nh = (double)n, nt = (double)cm.size;
  kmcpg_match m{};
  m.col = col;
  m.target_idx = cm.tidx;
  m.gsize = cm.gsize;
  m.mkmers = count;
  m.fpr = fpr;
  m.qcov = c / nh;
  m.tcov = c / nt;
  m.jacc = c / (nh + nt - c);
  return m;
}

// -c, -t, -T, -f in the reference's order (:7467-7478); *out is written only for a hit that passes.  The negated forms drop a NaN;
// n <= 0 gives the threshold 0 and qcov = inf, as the reference's arithmetic would.  cm is not read unless -c and -t passed.
template <class Meta, class FprOf>
inline bool match_accept(uint32_t col, int count, int n, const Meta& cm, const kmcpg_params& p, FprOf&& fpr_of, kmcpg_match* out) {
  if (count < p.min_matched) return false;
  const double c = (double)count;
  if (!(c > (double)n * p.min_qcov)) return false;
  if (!(c / (double)cm.size >= p.min_tcov)) return false;
  const double fpr = match_fpr(n, count, fpr_of);
  if (!(fpr <= p.max_fpr)) return false;
  *out = match_values(col, count, n, cm, fpr);
  return true;
}

// the score -s sorts by: 0 qcov, 1 tcov, 2 jacc
inline double match_score(const kmcpg_match& m, int sort_by) { return sort_by == 1 ? m.tcov : (sort_by == 2 ? m.jacc : m.qcov); }

inline bool match_less(const kmcpg_match& x, const kmcpg_match& y, int sort_by) {
  double s1, s2, t1, t2;
  switch (sort_by) {  // Matches.Less / SortByTCov.Less / SortByJacc.Less (:105-145)
    case 1: s1 = x.tcov; s2 = y.tcov; t1 = x.mkmers; t2 = y.mkmers; break;
    case 2: s1 = x.jacc; s2 = y.jacc; t1 = x.mkmers; t2 = y.mkmers; break;
    default: s1 = x.qcov; s2 = y.qcov; t1 = x.tcov; t2 = y.tcov; break;
  }
  if (s1 != s2) return s1 > s2;
  if (t1 != t2) return t1 > t2;
  return x.col < y.col;  // deterministic tie-break; the reference's order among exact ties is arbitrary
}

// A query's matches in final order (:273-282): match_less under -s, column order under -S.  Records are sorted where they are, or
// 4-byte indices into a record array in their place (the records are then written once, in order).  (static: with internal linkage
// std::sort's helpers are the caller's own and the compiler inlines them as it does a sort written in place; as weak symbols they stay calls)
template <class It, class RecordOf>
static inline void sort_matches_by(It first, It last, const kmcpg_params& p, RecordOf rec) {
  if (last - first < 2) return;
  const int sb = p.sort_by;
  if (!p.do_not_sort) std::sort(first, last, [=](const auto& x, const auto& y) { return match_less(rec(x), rec(y), sb); });
  else std::sort(first, last, [=](const auto& x, const auto& y) { return rec(x).col < rec(y).col; });
}
static inline void sort_matches(kmcpg_match* first, kmcpg_match* last, const kmcpg_params& p) {
  sort_matches_by(first, last, p, [](const kmcpg_match& m) -> const kmcpg_match& { return m; });
}
static inline void sort_matches(uint32_t* first, uint32_t* last, const kmcpg_match* records, const kmcpg_params& p) {
  sort_matches_by(first, last, p, [records](uint32_t i) -> const kmcpg_match& { return records[i]; });
}

// --keep-top-scores (:285-311) acts on sorted matches only
inline bool top_scores_on(const kmcpg_params& p) { return p.top_n_scores > 0 && !p.do_not_sort; }

// The running state of the reference's loop over matches of descending score: distinct scores seen, and the last of them.
struct TopScores {
  int top_n, nn = 0;
  double pscore = 1024;
  explicit TopScores(int top_n_scores) : top_n(top_n_scores) {}
  // the next match's score -> whether this match is the last one kept: the first of the (N+1)-th distinct score, which the
  // reference keeps too (its [:i+1], :302-310)
  bool last_kept(double score) {
    if (score < pscore) {
      if (++nn > top_n) return true;
      pscore = score;
    }
    return false;
  }
};

// how many of records[0 .. m), in final order, --keep-top-scores keeps: all of them when it is off or the loop visits every one
inline uint64_t top_scores_keep(const kmcpg_match* records, uint64_t m, const kmcpg_params& p) {
  if (!top_scores_on(p)) return m;
  TopScores top(p.top_n_scores);
  for (uint64_t i = 0; i < m; i++)
    if (top.last_kept(match_score(records[i], p.sort_by))) return i + 1;
  return m;
}

}  // namespace kmcpg
