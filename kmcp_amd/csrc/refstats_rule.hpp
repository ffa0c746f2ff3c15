// refstats_rule.hpp — what stage 1 of `kmcp profile` counts per reference and how it judges a reference from the counts: the one rule
// behind kmcp-refstats (cli/kmcp_refstats.cpp), the library's host half (refstats.cpp) and the tests' stand-alone check
// (tests/refstats_rule_check.cpp).  Host only; k6_refstats.hip restates the counting.
//
// Reference counterpart: kmcp/cmd/profile.go:761-1099 ("stage 1/4: counting matches and unique matches for filtering out low-confidence
// references"), presets :243-313.  Everything here is integer-exact except chunksFrac, one float64 division.
//
// A query is the run of surviving rows with one query name.  Its rows are grouped by target; the query is UNIQUE when it names one target,
// or, at --level species, when its targets lie under one species (specific_rule.hpp: specific_keep).  Every (target, chunk) is a COLUMN
// with four counters:
//   rows    every row of the column                                   (reference: Match[chunk] > 0  <=>  rows > 0)
//   firsts  the queries whose FIRST row of the target is this column  (reference: SumMatch = the sum over the target's chunks)
//   ureads  ... of them the unique queries                            (UniqMatch[chunk])
//   hic     ... of them those with that first row's qCov >= H         (UniqMatchHic[chunk])
// The reference adds 1/m per row to Match[chunk] (m = the target's rows in the query); stage 1 only asks Match > 0 and sums Match over
// the reference, which is the number of queries: both are stated in integers here.
#pragma once
#include <cstddef>
#include <cstdint>

#include "specific_rule.hpp"

namespace kmcpg {

constexpr int REFSTATS_ROWS = 0, REFSTATS_FIRSTS = 1, REFSTATS_UREADS = 2, REFSTATS_HIC = 3, REFSTATS_WORDS = 4;

// --mode 0..5: H = --min-hic-ureads-qcov, p = --min-chunks-fraction, and whether --keep-main-matches is on; then what only stage 3 asks
// (recount_rule.hpp): r = --min-chunks-reads, u = --min-uniq-reads, U = --min-hic-ureads, P = --min-hic-ureads-prop,
// d = --max-chunks-depth-stdev (mode 3: the flags' defaults)
struct RefstatsMode {
  double hic_min_qcov, min_chunks_fraction;
  bool keep_main;
  uint64_t min_chunks_reads, min_uniq_reads, min_hic_ureads;
  double min_hic_ureads_prop, max_chunks_depth_stdev;
};
constexpr int REFSTATS_MODES = 6, REFSTATS_DEFAULT_MODE = 3;
inline RefstatsMode refstats_mode(int mode) {
  constexpr RefstatsMode t[REFSTATS_MODES] = {{0.7, 0.2, true, 1, 1, 1, 0.01, 10},    {0.7, 0.6, false, 5, 2, 1, 0.1, 2},    {0.7, 0.7, false, 10, 5, 2, 0.2, 2},
                                               {0.75, 0.8, false, 50, 20, 5, 0.1, 2}, {0.8, 1.0, false, 100, 50, 10, 0.1, 2}, {0.8, 1.0, false, 100, 50, 10, 0.15, 1.5}};
  return t[mode];
}

// The rows a query keeps (profile.go:808-919): fed every row that passed -f / -t, in order; `first` = the row opens a query.  A query's
// first row is never tested by --keep-perfect-matches / --keep-main-matches; -n counts the rows whose qCov is below the previous KEPT one
// (a first row counts as one: the previous score starts at 1024).  Once a row is cut, so is the rest of the query.
struct RefstatsCut {
  bool keep_perfect = false, keep_main = false;
  double max_gap = 0.4;
  int top_n = 0;
  // state
  double prev = 1024;
  int n_score = 0;
  bool on = true;
  bool keep(bool first, double qcov) {
    if (first) {
      prev = 1024, n_score = 0, on = true;
    } else if (keep_perfect) {
      if (!on) return false;
      if (prev == 1 && qcov < 1) return on = false;
    } else if (keep_main && prev <= 1) {
      if (!on) return false;
      if (prev - qcov > max_gap) return on = false;
    }
    if (top_n > 0) {
      if (!on) return false;
      if (qcov < prev && ++n_score > top_n) return on = false;
    }
    prev = qcov;
    return true;
  }
};

struct RefstatsRow {
  uint32_t target_class, species_class;
  uint64_t column;
  double qcov;  // as printed and parsed back
};

// One finished query (n >= 1 rows, in row order): add(column, word) for every count.  Returns whether the query is unique.
template <class Add>
inline bool refstats_count_query(const RefstatsRow* r, size_t n, bool level_species, double hic_min_qcov, Add&& add) {
  SpecificAcc acc;
  for (size_t i = 0; i < n; i++) acc.add(r[i].target_class, r[i].species_class);
  const bool unique = specific_keep(acc, level_species);
  for (size_t i = 0; i < n; i++) {
    add(r[i].column, REFSTATS_ROWS);
    bool first = true;
    for (size_t j = 0; j < i && first; j++) first = r[j].target_class != r[i].target_class;
    if (!first) continue;
    add(r[i].column, REFSTATS_FIRSTS);
    if (!unique) continue;
    add(r[i].column, REFSTATS_UREADS);
    if (r[i].qcov >= hic_min_qcov) add(r[i].column, REFSTATS_HIC);
  }
  return unique;
}

// A reference from its chunks' counters (profile.go:1018-1095, the tests in its order)
enum RefstatsVerdict { REFSTATS_OK = 0, REFSTATS_NO_UNIQUE = 1, REFSTATS_NO_HIC_UNIQUE = 2, REFSTATS_LOW_CHUNKS = 3 };
inline const char* refstats_verdict_name(int v) {
  return v == REFSTATS_OK ? "ok" : v == REFSTATS_NO_UNIQUE ? "no-unique" : v == REFSTATS_NO_HIC_UNIQUE ? "no-hic-unique" : "low-chunks-fraction";
}
struct RefstatsRef {
  uint64_t reads = 0, ureads = 0, hic_ureads = 0, covered = 0;
  double chunks_frac = 0;
  int verdict = REFSTATS_OK;
};
// counters_of(c) -> const uint64_t* to the REFSTATS_WORDS counters of the reference's chunk c, c < chunks
template <class CountersOf>
inline RefstatsRef refstats_rollup(uint64_t chunks, double min_chunks_fraction, CountersOf&& counters_of) {
  RefstatsRef o;
  for (uint64_t c = 0; c < chunks; c++) {
    const uint64_t* w = counters_of(c);
    o.reads += w[REFSTATS_FIRSTS];
    o.ureads += w[REFSTATS_UREADS];
    o.hic_ureads += w[REFSTATS_HIC];
    if (w[REFSTATS_ROWS] > 0) o.covered++;
  }
  o.chunks_frac = (double)o.covered / (double)chunks;
  o.verdict = o.ureads < 1 ? REFSTATS_NO_UNIQUE : o.hic_ureads < 1 ? REFSTATS_NO_HIC_UNIQUE : o.chunks_frac < min_chunks_fraction ? REFSTATS_LOW_CHUNKS : REFSTATS_OK;
  return o;
}

}  // namespace kmcpg
