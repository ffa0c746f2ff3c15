// recount_rule.hpp — what stage 3 of `kmcp profile` does with the tables of stages 1 and 2: it takes the references a sample cannot support
// out of every read that names several (ambiguity correction), redistributes the read over the survivors and judges every reference again.
// The one rule behind kmcp-refstats --recount (cli/kmcp_refstats.cpp), the library's replay on the host (recount.cpp), the device code
// (k8_recount.hip: predicate, shares and masks are the functions below) and the tests' stand-alone check (tests/recount_rule_check.cpp).
// Host-compilable; the functions marked KMCPG_HD compile for the device too.
//
// Reference counterpart: kmcp/cmd/profile.go:1282-1888 ("stage 3/4: recounting matches and unique matches").
//
// A query's kept rows on the TSV route are exactly stage 2's (cooccur_rule.hpp: CooccurCut): rows of targets that stage 1 dropped are
// skipped before anything else, the cuts apply after that skip.  The kept rows are grouped by printed target: target h has m_h rows, its
// FIRST row is the first in row order.
//
// Ambiguity correction (unless no_amb_corr; only for a read with more than one target).  The targets are ordered by the printed qCov of
// their first rows, descending; ties keep the order of the first rows in the query (the reference sorts unstably over a map: it is not
// deterministic on ties — this tie rule is ours).  Then the reference's loop, quirk included:
//     for i in order: if del[i] continue
//       for j > i:   if del[j] continue
//         n = shared(i, j)                                                   stage 2's count, 0 if the pair is absent
//         if   reads[i] * (1 - D) >= n and ureads[j] < ureads[i] * R: del[j] = 1
//         elif reads[j] * (1 - D) >= n and ureads[i] < ureads[j] * R: del[i] = 1      the j loop goes ON with the deleted i
// reads / ureads: stage 1's integers of the reference (RefstatsRef); float64 compares, 1 - D computed once, one multiply each
// (-ffp-contract=off on the device: the same bits).  IN BIT MASKS: for row i let A_i be the j > i with the first condition and B_i those
// with the second and not the first; inside row i a bit j can be set only at its own visit, so the row is exactly
//     del |= (A_i & ~del) | ((B_i & ~del) ? bit(i) : 0)
// which is what host and device run (recount_row below).
//
// Shares, in integers — every route is bit-identical and order-free.  A row of a target with m rows adds UNIT / m to match[column]; the
// target's first row adds UNIT - (m - 1) * (UNIT / m) instead, so a target's rows sum to exactly UNIT = 720720 = lcm(1..16): for every m
// that divides UNIT, every m <= 16 among them, both are UNIT / m.  A row adds floor(qlen * 2^16 / (ns * m)) to bases[column], ns = the
// number of survivors.
//   ns == 1  the first row adds UNIT to uniq[column], and to hic[column] if its printed qCov >= H
//   ns > 1   at level species with all survivors under one species (specific_rule.hpp; species 0 is none) the first row of every survivor
//            adds its MATCH SHARE to uniq, and to hic if qCov >= H (the reference's 1 / floatMsSize)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "cooccur_rule.hpp"

namespace kmcpg {

constexpr uint64_t RECOUNT_UNIT = 720720, RECOUNT_BASE_UNIT = 1ull << 16;
constexpr int RECOUNT_MATCH = 0, RECOUNT_UNIQ = 1, RECOUNT_HIC = 2, RECOUNT_BASES = 3, RECOUNT_WORDS = 4;

// ---- shares
KMCPG_HD inline uint64_t recount_share(uint64_t m, bool first) { return first ? RECOUNT_UNIT - (m - 1) * (RECOUNT_UNIT / m) : RECOUNT_UNIT / m; }
KMCPG_HD inline uint64_t recount_bases(uint64_t qlen, uint64_t ns, uint64_t m) { return qlen * RECOUNT_BASE_UNIT / (ns * m); }

// ---- the predicate of (i, j), i before j in the order: 1 = j goes (A), 2 = i goes (B), 0 = neither
KMCPG_HD inline int recount_pred(uint64_t reads_i, uint64_t ureads_i, uint64_t reads_j, uint64_t ureads_j, uint64_t shared, double one_minus_d, double r_err) {
  const double n = (double)shared;
  if ((double)reads_i * one_minus_d >= n && (double)ureads_j < (double)ureads_i * r_err) return 1;
  if ((double)reads_j * one_minus_d >= n && (double)ureads_i < (double)ureads_j * r_err) return 2;
  return 0;
}
// ---- one row of the loop on a 64-bit mask (bit k = the target of rank k); a_i / b_i: bits j > i only
KMCPG_HD inline uint64_t recount_row(uint64_t del, uint32_t i, uint64_t a_i, uint64_t b_i) {
  return del | (a_i & ~del) | ((b_i & ~del) ? 1ull << i : 0ull);
}

struct RecountClass {  // a target class as stages 1 and 2 leave it
  uint32_t kept;       // stage 1's verdict is ok
  uint64_t reads, ureads;
};
struct RecountParams {
  double one_minus_d = 0.95, r_err = 0.05, hic_min_qcov = 0.75;
  bool no_amb_corr = false, level_species = true;
};
struct RecountRow {
  uint32_t target_class, species_class;
  uint64_t column;
  double qcov;  // as printed and parsed back
  uint64_t qlen;
};

// The targets of a read in elimination order: ids of the first rows, by (qcov desc, first-row index asc)
inline void recount_order(const double* first_qcov, size_t nt, std::vector<uint32_t>* order) {
  order->resize(nt);
  for (size_t i = 0; i < nt; i++) (*order)[i] = (uint32_t)i;
  std::stable_sort(order->begin(), order->end(), [&](uint32_t a, uint32_t b) { return first_qcov[a] > first_qcov[b]; });
}
// The loop over any number of targets, in masks of 64-bit words: pred(i, j) for ranks i < j as recount_pred.  del: (nt + 63) / 64 words
template <class Pred>
inline void recount_eliminate(size_t nt, Pred&& pred, std::vector<uint64_t>* del) {
  const size_t nw = (nt + 63) / 64;
  del->assign(nw, 0);
  std::vector<uint64_t> a(nw), b(nw);
  for (size_t i = 0; i + 1 < nt; i++) {
    if ((*del)[i / 64] >> (i % 64) & 1) continue;
    std::fill(a.begin(), a.end(), 0), std::fill(b.begin(), b.end(), 0);
    for (size_t j = i + 1; j < nt; j++) {
      const int p = pred(i, j);
      if (p == 1) a[j / 64] |= 1ull << (j % 64);
      else if (p == 2) b[j / 64] |= 1ull << (j % 64);
    }
    uint64_t any_b = 0;
    for (size_t w = 0; w < nw; w++) any_b |= b[w] & ~(*del)[w];
    for (size_t w = 0; w < nw; w++) (*del)[w] |= a[w] & ~(*del)[w];
    if (any_b) (*del)[i / 64] |= 1ull << (i % 64);
  }
}

// One finished query: its kept rows (n >= 1, in row order, every target kept by stage 1).  shared(class_a, class_b) -> stage 2's count;
// add(column, word, amount).  Returns the number of survivors; *lost: the correction took at least one target.
template <class Shared, class Add>
inline size_t recount_query(const RecountRow* r, size_t n, const RecountClass* cls, const RecountParams& p, Shared&& shared, Add&& add, bool* lost) {
  // the targets in order of their first rows
  std::vector<uint32_t> tcls, tfirst, tm, tof(n);
  for (size_t i = 0; i < n; i++) {
    size_t t = 0;
    while (t < tcls.size() && tcls[t] != r[i].target_class) t++;
    if (t == tcls.size()) tcls.push_back(r[i].target_class), tfirst.push_back((uint32_t)i), tm.push_back(0);
    tm[t]++, tof[i] = (uint32_t)t;
  }
  const size_t nt = tcls.size();
  std::vector<uint8_t> gone(nt, 0);
  *lost = false;
  if (nt > 1 && !p.no_amb_corr) {
    std::vector<double> q(nt);
    for (size_t t = 0; t < nt; t++) q[t] = r[tfirst[t]].qcov;
    std::vector<uint32_t> order;
    recount_order(q.data(), nt, &order);
    std::vector<uint64_t> del;
    recount_eliminate(nt, [&](size_t i, size_t j) {
      const RecountClass &ci = cls[tcls[order[i]]], &cj = cls[tcls[order[j]]];
      return recount_pred(ci.reads, ci.ureads, cj.reads, cj.ureads, shared(tcls[order[i]], tcls[order[j]]), p.one_minus_d, p.r_err);
    }, &del);
    for (size_t k = 0; k < nt; k++)
      if (del[k / 64] >> (k % 64) & 1) gone[order[k]] = 1, *lost = true;
  }
  size_t ns = 0;
  SpecificAcc acc;
  for (size_t t = 0; t < nt; t++)
    if (!gone[t]) ns++, acc.add(tcls[t], r[tfirst[t]].species_class);
  const bool uniq_first = ns == 1 || (p.level_species && acc.smin == acc.smax && acc.smin != 0);
  for (size_t i = 0; i < n; i++) {
    const uint32_t t = tof[i];
    if (gone[t]) continue;
    const bool first = tfirst[t] == i;
    const uint64_t share = recount_share(tm[t], first);
    add(r[i].column, RECOUNT_MATCH, share);
    add(r[i].column, RECOUNT_BASES, recount_bases(r[i].qlen, ns, tm[t]));
    if (!first || !uniq_first) continue;
    const uint64_t u = ns == 1 ? RECOUNT_UNIT : share;
    add(r[i].column, RECOUNT_UNIQ, u);
    if (r[i].qcov >= p.hic_min_qcov) add(r[i].column, RECOUNT_HIC, u);
  }
  return ns;
}

// ---- a reference from its chunks' counters (profile.go:1743-1888, the tests in its order)
enum RecountVerdict { RECOUNT_OK = 0, RECOUNT_FEW_UNIQUE = 1, RECOUNT_FEW_HIC_UNIQUE = 2, RECOUNT_LOW_HIC_PROP = 3, RECOUNT_LOW_CHUNKS = 4, RECOUNT_HIGH_STDEV = 5 };
inline const char* recount_verdict_name(int v) {
  static const char* const names[] = {"ok", "few-unique", "few-hic-unique", "low-hic-unique-prop", "low-chunks-fraction", "high-depth-stdev"};
  return names[v];
}
enum RecountNorm { RECOUNT_NORM_MEAN = 0, RECOUNT_NORM_MIN = 1, RECOUNT_NORM_MAX = 2 };
struct RecountThresholds {
  uint64_t min_chunks_reads = 50, min_uniq_reads = 20, min_hic_ureads = 5;             // -r -u -U
  double min_hic_ureads_prop = 0.1, min_chunks_fraction = 0.8, max_depth_stdev = 2;  // -P -p -d
  int norm = RECOUNT_NORM_MEAN;
};
struct RecountRef {
  uint64_t match = 0, uniq = 0, hic = 0, bases = 0;  // sums over the chunks, in units
  double chunks_frac = 0, depth_stdev = 0, coverage = 0;
  int verdict = RECOUNT_OK;
  bool listed = false;  // it has an add (the reference's profile2 has an entry)
};
// MeanStdev (util.go:381): the population standard deviation
inline double recount_stdev(const std::vector<double>& v) {
  const size_t n = v.size();
  if (n < 2) return 0;
  double sum = 0, var = 0;
  for (double x : v) sum += x;
  const double mean = sum / (double)n;
  for (double x : v) var += (x - mean) * (x - mean);
  return std::sqrt(var / (double)n);
}
// counters_of(c) -> const uint64_t* to the RECOUNT_WORDS counters of the reference's chunk c, c < chunks
template <class CountersOf>
inline RecountRef recount_rollup(uint64_t chunks, uint64_t tlen, const RecountThresholds& th, CountersOf&& counters_of) {
  RecountRef o;
  uint64_t covered = 0, bmin = UINT64_MAX, bmax = 0;
  for (uint64_t c = 0; c < chunks; c++) {
    const uint64_t* w = counters_of(c);
    o.match += w[RECOUNT_MATCH], o.uniq += w[RECOUNT_UNIQ], o.hic += w[RECOUNT_HIC], o.bases += w[RECOUNT_BASES];
    if (w[RECOUNT_MATCH] >= th.min_chunks_reads * RECOUNT_UNIT) covered++;
    if (w[RECOUNT_BASES]) bmin = std::min(bmin, w[RECOUNT_BASES]), bmax = std::max(bmax, w[RECOUNT_BASES]);
  }
  o.listed = o.match > 0;  // every add of a read comes with a match share
  o.chunks_frac = chunks ? (double)covered / (double)chunks : 0;
  const double unit = (double)RECOUNT_BASE_UNIT, qlens = (double)o.bases / unit;
  if (o.bases) {
    std::vector<double> rel((size_t)chunks);
    for (uint64_t c = 0; c < chunks; c++) rel[(size_t)c] = (double)counters_of(c)[RECOUNT_BASES] / unit / qlens * (double)chunks;
    o.depth_stdev = recount_stdev(rel);
    const double top = th.norm == RECOUNT_NORM_MEAN ? qlens : (double)(th.norm == RECOUNT_NORM_MIN ? bmin : bmax) / unit * (double)chunks;
    o.coverage = top / (double)tlen;
  }
  o.verdict = o.uniq < th.min_uniq_reads * RECOUNT_UNIT                      ? RECOUNT_FEW_UNIQUE
              : o.hic < th.min_hic_ureads * RECOUNT_UNIT                     ? RECOUNT_FEW_HIC_UNIQUE
              : (double)o.hic < th.min_hic_ureads_prop * (double)o.uniq      ? RECOUNT_LOW_HIC_PROP
              : o.chunks_frac < th.min_chunks_fraction                       ? RECOUNT_LOW_CHUNKS
              : o.depth_stdev > th.max_depth_stdev                           ? RECOUNT_HIGH_STDEV
                                                                             : RECOUNT_OK;
  return o;
}

}  // namespace kmcpg
