// regions_rule.hpp — the rule of `kmcp utils merge-regions`, stated once (host only).
//
// Reference counterpart: kmcp/cmd/merge-regions.go:219-388 and the row parser util-regions.go.  The windows of a genome (queries named
// REF_sliding:BEGIN-END) that survived the specific-query filter are merged into regions, BED6 out.  Users: cli/kmcp_regions.cpp (rows
// of a TSV), cli/kmcp_search.cpp --regions-bed (window summaries from the library), finalize.cpp (the summaries the device leaves to the
// host), tests/regions_rule_check.cpp.
//
//   rows     a row is cut at its first 12 tabs; FPR (field 4) is parsed and tested against -f BEFORE qCov (field 12) is parsed and tested
//            against -t; only a row that passed both has its query name matched against the pattern.
//   queries  a maximal run of consecutive KEPT rows with equal field 1; a dropped row does not end a run.
//   summary  n = distinct targets of the query; score = the qCov of the first row of each distinct target, added in order of first
//            appearance in float64, divided by n when n > 1; the window is "assembly" when n == 1, else "species".
//   merging  the state is a pending region and the previous query's (begin, end); see RegionMerger::add.
//
// Deliberate differences to the reference ("Specific regions"):
//   1. the reference adds the targets' scores in Go map order (random); here: order of first appearance, one of the orders it can take;
//   2. a file with exactly one passing query makes the reference print a line of an empty region first; here only the real one;
//   3. the reference takes begin0 > 0 for "there is a pending region"; here a flag says so (differs only for a pattern that yields 0).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <unordered_set>
#include <vector>

namespace kmcpg {

// ---- rows
enum RegionRow { REGION_ROW_SKIP, REGION_ROW_KEPT, REGION_ROW_DROPPED, REGION_ROW_FEW_FIELDS, REGION_ROW_BAD_FPR, REGION_ROW_BAD_QCOV };
struct RegionRowFields {
  const char *query, *target, *bad;  // bad: the field that did not parse
  size_t query_n, target_n, bad_n;
  double fpr, qcov;
};
// p[0 .. len): one line with or without its end of line.  parse_float(p, n, &v): the whole field as a float64.
template <class ParseFloat>
inline RegionRow region_row(const char* p, size_t len, double max_fpr, double min_qcov, ParseFloat parse_float, RegionRowFields* f) {
  if (len && p[len - 1] == '\n') len--;
  if (len && p[len - 1] == '\r') len--;
  if (len == 0 || p[0] == '#') return REGION_ROW_SKIP;
  size_t tab[12];
  int nt = 0;
  for (size_t i = 0; i < len && nt < 12; i++)
    if (p[i] == '\t') tab[nt++] = i;
  if (nt < 12) return REGION_ROW_FEW_FIELDS;
  f->bad = p + tab[2] + 1, f->bad_n = tab[3] - tab[2] - 1;
  if (!parse_float(f->bad, f->bad_n, &f->fpr)) return REGION_ROW_BAD_FPR;
  if (f->fpr > max_fpr) return REGION_ROW_DROPPED;
  f->bad = p + tab[10] + 1, f->bad_n = tab[11] - tab[10] - 1;
  if (!parse_float(f->bad, f->bad_n, &f->qcov)) return REGION_ROW_BAD_QCOV;
  if (f->qcov < min_qcov) return REGION_ROW_DROPPED;
  f->query = p, f->query_n = tab[0];
  f->target = p + tab[4] + 1, f->target_n = tab[5] - tab[4] - 1;
  return REGION_ROW_KEPT;
}

// the default pattern ^(.+)_sliding:(\d+)\-(\d+)$ by hand: the LAST "_sliding:" (what follows a match holds no other), a non-empty name
// before it, digits, '-', digits to the end.  Numbers too large for 64 bits saturate.
inline bool region_default_name(const char* q, size_t n, size_t* ref_n, int64_t* begin, int64_t* end) {
  static const char tag[] = "_sliding:";
  const size_t tn = sizeof tag - 1;
  if (n < tn + 4) return false;
  size_t at = n - tn;
  for (;; at--) {
    if (memcmp(q + at, tag, tn) == 0) break;
    if (at == 0) return false;
  }
  if (at == 0) return false;
  auto digits = [&](size_t& i, int64_t* v) {
    const size_t i0 = i;
    uint64_t x = 0;
    bool sat = false;
    for (; i < n && q[i] >= '0' && q[i] <= '9'; i++) {
      if (x > (0x7fffffffffffffffULL - 9) / 10) sat = true;
      else x = x * 10 + (uint64_t)(q[i] - '0');
    }
    *v = sat ? 0x7fffffffffffffffLL : (int64_t)x;
    return i > i0;
  };
  size_t i = at + tn;
  if (!digits(i, begin) || i >= n || q[i] != '-') return false;
  i++;
  if (!digits(i, end) || i != n) return false;
  *ref_n = at;
  return true;
}

// ---- a window's summary over target classes (equal class = equal printed target)
struct WindowSummaryAcc {
  uint32_t n = 0;
  double sum = 0;
  void clear() {
    n = 0, sum = 0;
    few_.clear();
    many_.clear();
  }
  // a row in print order: x = its qCov
  void add(uint32_t target_class, double x) {
    if (many_.empty()) {
      for (uint32_t c : few_)
        if (c == target_class) return;
      few_.push_back(target_class);
      if (few_.size() > 32) many_.insert(few_.begin(), few_.end());
    } else if (!many_.insert(target_class).second) return;
    sum = n == 0 ? x : sum + x;
    n++;
  }
  double score() const { return n > 1 ? sum / (double)n : sum; }

 private:
  std::vector<uint32_t> few_;
  std::unordered_set<uint32_t> many_;
};

// ---- merging
struct RegionParams {
  int64_t min_overlap = 1, max_gap = 0;
  bool ignore_type = false;
  std::string name_species = "species-specific", name_assembly = "assembly-specific";
};

// One input's windows in order -> BED lines appended to a string.  The state lives across calls, so a caller may hand the windows over
// in batches cut anywhere.
struct RegionMerger {
  RegionParams p;
  uint64_t n_windows = 0, n_regions = 0;
  explicit RegionMerger(const RegionParams& params = RegionParams()) : p(params) {}

  // a query with n_targets >= 1 distinct targets
  void add(const char* ref, size_t ref_n, int64_t begin, int64_t end, uint32_t n_targets, double score, std::string* out) {
    n_windows++;
    const std::string& name = n_targets == 1 ? p.name_assembly : p.name_species;
    const bool extend = pending_ && ref0_.size() == ref_n && memcmp(ref0_.data(), ref, ref_n) == 0 && begin + p.min_overlap - 1 <= end1_ &&
                        (p.ignore_type || name == name0_) && (p.max_gap == 0 || begin - begin1_ <= p.max_gap);
    if (extend) {
      end0_ = end;
      if (name0_ != name) name0_ = p.name_species;
      if (name0_ == p.name_species) score0_ = (score0_ + score) / 2;
    } else {
      print(out);
      pending_ = true;
      ref0_.assign(ref, ref_n);
      begin0_ = begin, end0_ = end, name0_ = name, score0_ = score;
    }
    begin1_ = begin, end1_ = end;
  }
  // the end of the input: the pending region is printed and the state is that of a new input
  void finish(std::string* out) {
    print(out);
    pending_ = false;
  }

 private:
  bool pending_ = false;
  std::string ref0_, name0_;
  int64_t begin0_ = 0, end0_ = 0, begin1_ = 0, end1_ = 0;
  double score0_ = 0;
  void print(std::string* out) {
    if (!pending_) return;
    n_regions++;
    char num[96];
    out->append(ref0_);
    int m = snprintf(num, sizeof num, "\t%lld\t%lld\t", (long long)(begin0_ - 1), (long long)end0_);
    out->append(num, (size_t)m);
    out->append(name0_);
    m = snprintf(num, sizeof num, "\t%.0f\t.\n", score0_ * 1000);
    out->append(num, (size_t)m);
  }
};

}  // namespace kmcpg
