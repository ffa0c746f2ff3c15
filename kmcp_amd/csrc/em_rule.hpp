// em_rule.hpp — what stage 4 of `kmcp profile` does with the references stage 3 lists: it estimates their abundances by an EM loop.  Every
// pass shares each read out over its estimated references in proportion to their current coverage, rolls the shares up into a new coverage
// per reference, and stops when the top percentage stands still.  The one rule behind the library's pass on the host (em.cpp), the device
// code (k9_em.hip: the shares and the two-word bases are the functions below) and the tests' stand-alone check (tests/em_rule_check.cpp).
// Host-compilable; the functions marked KMCPG_HD compile for the device too.
//
// Reference counterpart: kmcp/cmd/profile.go:1907-2570 ("stage 4/4: estimating abundance using EM algorithm"), its end :2786-2853.
//
// Everything a read adds is an INTEGER, so every route gives the same bytes whatever the order of the reads.
//
// Unit.  EM_UNIT = RECOUNT_UNIT << 12 = 2 952 069 120 per read (< 2^32): K8's single-read counters convert exactly by << 12.
//
// One read in one pass — its rows as K3 left them, est[class] (the pass's whitelist), cov[class] (float64, > 0 and finite for every estimated
// class), H, level_species.  Rows of classes with est == 0 are skipped; the others are grouped by target in first-row order, m_t rows each.
//   nt == 0  nothing
//   nt == 1  the unique rule (profile.go:2127-2165): a row adds recount_share(m, first) << 12 to match, the first row EM_UNIT to uniq and —
//            printed qCov >= H — to hic
//   nt > 1   S = the sum of cov[class_t], added SEQUENTIALLY IN FIRST-ROW ORDER in float64 (the reference adds in Go's map order: it is not
//            deterministic to the last bit — this order is ours).  q_t = min(EM_UNIT, floor(cov_t / S * EM_UNIT)): one division, one
//            multiply, no contraction.  p_t = min(q_t, EM_UNIT - (p of the targets before t)), in first-row order: with exact quotients the
//            q_t sum to at most EM_UNIT and p_t = q_t; the rounding of S and of the quotients can lift the sum above it by a unit or two (S
//            rounded down by 2^-53 relative is 3e-7 units), and then the cap takes them off the last targets.  What is left,
//            EM_UNIT - sum p_t, goes to the FIRST target: every assigned read adds exactly EM_UNIT to match.
//            A row of target t adds p_t / m_t, its first row p_t - (m_t - 1) * (p_t / m_t).  uniq and hic only at level species with all
//            targets under one non-zero species (SpecificAcc, as in K8): every target's first row adds its match share to uniq, and to
//            hic if its qCov >= H.
//   bases    a row adds the exact product qlen * (its match share), in units of 1 / EM_UNIT base, into TWO 64-bit counters: the product's
//            low 32 bits and the rest.  qlen < 2^32 (it is clamped) and a share <= EM_UNIT < 2^32: the product is below 2^64, either part
//            below 2^32, so neither counter overflows below 2^32 rows per column.  Nothing is rounded.
// A column has five counters: match, uniq, hic, bases_lo, bases_hi.
//
// Reads with ONE target in the whole table (before the whitelist) never reach this rule: K8 counts them once, when they are searched, in its
// own units (recount_rule.hpp, ns == 1: recount_share and recount_bases, four counters per column), and a pass takes those counters over for
// the estimated classes — match, uniq and hic << 12, the bases apart in units of 2^-16 base (EmChunk below).  Whoever meets such a read
// later (the host half of a pass, the TSV tool) counts it by that rule too: the words do not depend on who counted.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "recount_rule.hpp"

namespace kmcpg {

constexpr int EM_SHIFT = 12;
constexpr uint64_t EM_UNIT = RECOUNT_UNIT << EM_SHIFT;
static_assert(EM_UNIT == 2952069120ull && EM_UNIT < (1ull << 32), "a share fits 32 bits");
constexpr int EM_MATCH = 0, EM_UNIQ = 1, EM_HIC = 2, EM_BASES_LO = 3, EM_BASES_HI = 4, EM_WORDS = 5;

// ---- shares
// q_t: the share of a target of coverage cov in a read whose targets' coverages sum to sum
KMCPG_HD inline uint64_t em_quota(double cov, double sum) {
  const double x = cov / sum * (double)EM_UNIT;
  return x < (double)EM_UNIT ? (uint64_t)x : EM_UNIT;  // (x >= 0; anything that does not compare below EM_UNIT is EM_UNIT)
}
// a row's part of its target's p: the first row takes the remainder
KMCPG_HD inline uint64_t em_row_share(uint64_t p, uint64_t m, bool first) { return first ? p - (m - 1) * (p / m) : p / m; }
KMCPG_HD inline uint64_t em_single_share(uint64_t m, bool first) { return recount_share(m, first) << EM_SHIFT; }
// the exact product qlen * share in two words
KMCPG_HD inline void em_bases(uint64_t qlen, uint64_t share, uint64_t* lo, uint64_t* hi) {
  const uint64_t x = (qlen < 0xffffffffull ? qlen : 0xffffffffull) * share;
  *lo = x & 0xffffffffull, *hi = x >> 32;
}
// the bases of a column's two words, in bases
inline double em_bases_value(uint64_t lo, uint64_t hi) { return ((double)hi * 4294967296.0 + (double)lo) / (double)EM_UNIT; }

// One read: its rows with an estimated class (n >= 0, in row order).  cov[class]; add(column, word, amount).  Returns the number of targets
template <class Add>
inline size_t em_query(const RecountRow* r, size_t n, const double* cov, double hic_min_qcov, bool level_species, Add&& add) {
  std::vector<uint32_t> tcls, tfirst, tm, tof(n);
  for (size_t i = 0; i < n; i++) {
    size_t t = 0;
    while (t < tcls.size() && tcls[t] != r[i].target_class) t++;
    if (t == tcls.size()) tcls.push_back(r[i].target_class), tfirst.push_back((uint32_t)i), tm.push_back(0);
    tm[t]++, tof[i] = (uint32_t)t;
  }
  const size_t nt = tcls.size();
  if (nt == 0) return 0;
  std::vector<uint64_t> p(nt, 0);
  bool uniq_first = true;
  if (nt > 1) {
    double sum = 0;
    for (size_t t = 0; t < nt; t++) sum += cov[tcls[t]];
    uint64_t room = EM_UNIT;
    for (size_t t = 0; t < nt; t++) p[t] = std::min(em_quota(cov[tcls[t]], sum), room), room -= p[t];
    p[0] += room;
    SpecificAcc acc;
    for (size_t t = 0; t < nt; t++) acc.add(tcls[t], r[tfirst[t]].species_class);
    uniq_first = level_species && acc.smin == acc.smax && acc.smin != 0;
  }
  for (size_t i = 0; i < n; i++) {
    const uint32_t t = tof[i];
    const bool first = tfirst[t] == i;
    const uint64_t share = nt == 1 ? em_single_share(tm[t], first) : em_row_share(p[t], tm[t], first);
    uint64_t lo, hi;
    em_bases(r[i].qlen, share, &lo, &hi);
    add(r[i].column, EM_MATCH, share);
    add(r[i].column, EM_BASES_LO, lo);
    add(r[i].column, EM_BASES_HI, hi);
    if (!first || !uniq_first) continue;
    const uint64_t u = nt == 1 ? EM_UNIT : share;
    add(r[i].column, EM_UNIQ, u);
    if (r[i].qcov >= hic_min_qcov) add(r[i].column, EM_HIC, u);
  }
  return nt;
}

// ---- a reference in one pass (profile.go:2372-2518).  A chunk's counters: the single-target reads' (K8's, match / uniq / hic << 12, their
// bases kept apart in units of 2^-16 base) plus the pass's
struct EmChunk {
  uint64_t match = 0, uniq = 0, hic = 0;  // EM units, single-target reads included
  uint64_t single_bases = 0;              // 2^-16 base
  uint64_t bases_lo = 0, bases_hi = 0;    // 1 / EM_UNIT base
};
inline double em_chunk_bases(const EmChunk& c) { return (double)c.single_bases / (double)RECOUNT_BASE_UNIT + em_bases_value(c.bases_lo, c.bases_hi); }
struct EmRef {
  uint64_t match = 0, uniq = 0, hic = 0;
  double chunks_frac = 0, depth_stdev = 0, coverage = 0, percentage = 0;
  std::vector<double> rel_depth;
  int verdict = RECOUNT_OK;  // judged after pass 0 only
  bool listed = false;       // a read added to it in this pass (the reference's profile3 has an entry)
};
// chunk_of(c) -> EmChunk of the reference's chunk c; judge: the five tests of pass 0, in the reference's order
template <class ChunkOf>
inline EmRef em_rollup(uint64_t chunks, uint64_t tlen, const RecountThresholds& th, bool judge, ChunkOf&& chunk_of) {
  EmRef o;
  uint64_t covered = 0;
  std::vector<double> b((size_t)chunks);
  double qlens = 0, bmin = 0, bmax = 0;
  bool any = false;
  for (uint64_t c = 0; c < chunks; c++) {
    const EmChunk w = chunk_of(c);
    o.match += w.match, o.uniq += w.uniq, o.hic += w.hic;
    if (w.match >= th.min_chunks_reads * EM_UNIT) covered++;
    const double x = em_chunk_bases(w);
    b[(size_t)c] = x, qlens += x;
    if (x != 0) bmin = any ? std::min(bmin, x) : x, bmax = any ? std::max(bmax, x) : x, any = true;
  }
  o.listed = o.match > 0;
  o.chunks_frac = chunks ? (double)covered / (double)chunks : 0;
  o.rel_depth.assign((size_t)chunks, 0);
  if (any) {
    for (uint64_t c = 0; c < chunks; c++) o.rel_depth[(size_t)c] = b[(size_t)c] / qlens * (double)chunks;
    o.depth_stdev = recount_stdev(o.rel_depth);
    o.coverage = (th.norm == RECOUNT_NORM_MEAN ? qlens : (th.norm == RECOUNT_NORM_MIN ? bmin : bmax) * (double)chunks) / (double)tlen;
  }
  if (judge)
    o.verdict = o.uniq < th.min_uniq_reads * EM_UNIT                      ? RECOUNT_FEW_UNIQUE
                : o.hic < th.min_hic_ureads * EM_UNIT                     ? RECOUNT_FEW_HIC_UNIQUE
                : (double)o.hic < th.min_hic_ureads_prop * (double)o.uniq ? RECOUNT_LOW_HIC_PROP
                : o.chunks_frac < th.min_chunks_fraction                  ? RECOUNT_LOW_CHUNKS
                : o.depth_stdev > th.max_depth_stdev                      ? RECOUNT_HIGH_STDEV
                                                                          : RECOUNT_OK;
  return o;
}

// ---- the loop.  A class (a reference): its chunks' columns and length; est / coverage are the loop's state
struct EmClass {
  std::vector<uint64_t> columns;  // the global column of chunk c
  uint64_t tlen = 0;
  std::string name;
};
struct EmParams {
  RecountThresholds th;
  int max_iters = 10;            // --abund-max-iters: at most max_iters + 1 passes
  double pct_threshold = 0.01;   // --abund-pct-threshold
};
struct EmResult {
  std::vector<EmRef> refs;     // per class, of the last pass; est[c] != 0: it is in the table
  std::vector<uint8_t> est;
  uint64_t assigned = 0;       // reads the last pass assigned
  int passes = 0;
  bool converged = false;
};
// The loop's entry from stage 3 (recount_rule.hpp: recount_rollup): a reference is estimated if stage 3 lists it with verdict ok — and
// its coverage is a positive number (a reference whose reads all have qLen 0 has none to share by: ours)
inline bool em_start(const RecountRef& t, double* cov) {
  *cov = t.coverage;
  return t.listed && t.verdict == RECOUNT_OK && std::isfinite(t.coverage) && t.coverage > 0;
}
// pass(est, cov, &cols, &assigned) -> 0 or an error code: cols[column] = the EmChunk of every column for this whitelist and these coverages.
// est / cov on entry: stage 3's ok references and their stage-3 coverage
template <class Pass>
inline int em_run(const std::vector<EmClass>& classes, std::vector<uint8_t> est, std::vector<double> cov, const EmParams& p, Pass&& pass, EmResult* out) {
  const size_t n = classes.size();
  out->refs.assign(n, EmRef());
  out->passes = 0, out->converged = false, out->assigned = 0;
  double top_before = 0;
  std::vector<EmChunk> cols;
  // the coverages are added, and the top reference is looked for, in ascending order of the NAMES: a command that numbers the references
  // by the search result's rows and one that numbers them by the database's columns then add in the same order — the same bits
  std::vector<size_t> by_name(n);
  for (size_t c = 0; c < n; c++) by_name[c] = c;
  std::sort(by_name.begin(), by_name.end(), [&](size_t a, size_t b) { return classes[a].name != classes[b].name ? classes[a].name < classes[b].name : a < b; });
  for (int iter = 0; iter <= p.max_iters; iter++) {
    if (std::none_of(est.begin(), est.end(), [](uint8_t e) { return e != 0; })) break;
    if (int rc = pass(est, cov, &cols, &out->assigned)) return rc;
    out->passes++;
    double sum = 0, top_cov = -1, top_pct = 0;
    for (const size_t c : by_name) {
      if (!est[c]) continue;
      EmRef r = em_rollup(classes[c].columns.size(), classes[c].tlen, p.th, iter == 0, [&](uint64_t k) { return cols[(size_t)classes[c].columns[(size_t)k]]; });
      if (!r.listed || r.verdict != RECOUNT_OK) est[c] = 0;  // it leaves the whitelist for good
      out->refs[c] = r;
      if (est[c]) cov[c] = r.coverage, sum += r.coverage;
    }
    size_t left = 0;
    for (const size_t c : by_name) {
      if (!est[c]) continue;
      left++;
      out->refs[c].percentage = cov[c] / sum * 100;
      if (cov[c] > top_cov) top_cov = cov[c], top_pct = out->refs[c].percentage;
    }
    if (left == 0) break;
    if (iter > 0 && std::fabs(top_pct - top_before) < p.pct_threshold) {
      out->converged = true;
      break;
    }
    top_before = top_pct;
  }
  out->est = est;
  return 0;
}

// ---- the end (profile.go:2786-2853): the order — coverage descending, chunksFrac descending, name ascending (the last is ours: the reference's
// sort is unstable) — and -F: the tail whose percentages sum to at most filter_low_pct is dropped and the rest renormalised; only with more
// than one reference left.  Returns the class indexes in table order; percentages are updated in res
inline std::vector<uint32_t> em_finish(const std::vector<EmClass>& classes, double filter_low_pct, EmResult* res) {
  std::vector<uint32_t> order;
  for (size_t c = 0; c < classes.size(); c++)
    if (c < res->est.size() && res->est[c]) order.push_back((uint32_t)c);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const EmRef &x = res->refs[a], &y = res->refs[b];
    if (x.coverage != y.coverage) return x.coverage > y.coverage;
    if (x.chunks_frac != y.chunks_frac) return x.chunks_frac > y.chunks_frac;
    return classes[a].name < classes[b].name;
  });
  if (filter_low_pct > 0 && order.size() > 1) {
    double acc = 0;
    size_t keep = order.size();
    while (keep > 0) {  // from the tail
      acc += res->refs[order[keep - 1]].percentage;
      if (acc > filter_low_pct) break;
      keep--;
    }
    if (keep < order.size()) {  // (in table order, as the reference adds)
      order.resize(keep);
      double sum = 0;
      for (uint32_t c : order) sum += res->refs[c].coverage;
      for (uint32_t c : order) res->refs[c].percentage = res->refs[c].coverage / sum * 100;
    }
  }
  return order;
}

}  // namespace kmcpg
