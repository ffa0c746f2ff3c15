// k5_summary.hip — K5: a window's summary for region merging, ON THE DEVICE, behind K4.
//
// Reference counterpart: what `kmcp utils merge-regions` derives from the rows of one query before it merges (merge-regions.go:256-279;
// the rule is restated in regions_rule.hpp): n = the distinct targets among the query's rows, score = the qCov of the first row of each
// distinct target added in order of first appearance (float64), divided by n when n > 1.  K4 leaves the surviving windows' matches in HBM
// as (column, count) pairs in print order; target_class (kmcpg_set_specific) says which columns are one printed target.  A row's qCov as
// the TSV route parses it back is x = fixed4(count / qkmers) / 10000 (k3_set_order.hpp: the digits "%.4f" prints; both divisions are
// correctly rounded, -ffp-contract=off, no fast-math), so the 16-byte record written here has the bits the three-command pipeline computes.
//
//   k5_summary  the walk of seg_walk.hpp (one wave per 16 consecutive windows; a window's lane group reduces segments of up to 64 pairs,
//               the whole wave the longer ones) over min / max of target_class alone.
//                 empty    no pairs, or verdict DROP                      n = 0
//                 single   min == max (ANY length; by far the common case) n = 1, score = x of the segment's first pair
//                 wave     several targets, up to K5_CAP pairs: lane i holds pair i and whether it is the first of its class
//                          (first_of_class, seg_walk.hpp); the flagged x are added in ascending lane order in float64 by every lane
//                          alike (shuffles), then divided by n
//                 LEFT     several targets above K5_CAP, and verdict HOST (the pairs still face the host's -f test): the host computes
//                          the summary from the pairs (host.cpp); the record carries the segment's length in n_targets and the HOST
//                          verdict as a flag, so a caller needs neither the LEFT offsets nor the verdict bytes; cnt[r] = that length
//   k3_scan_*   exclusive scan of cnt (k3_finalize.hip)
//   k4_compact  the LEFT segments, and only those, copied to left_pairs (k4_specific.hip)
//
// K5_CAP = 64: one pair per lane, so the distinct-class pass needs no memory and at most 64 shuffles, and the sum is one shuffle per
// distinct target.  A window of 100-150 bases that matches more than 64 chunks of several targets is rare (it is a repeat shared by a
// whole family); a larger cap would need several pairs per lane and a sum that crosses lanes in print order — exact as well, but more
// code on a path almost no window takes.  Counters (wave-aggregated: one atomic per wave and word): windows single / by the wave / LEFT /
// empty, segments outside the pair buffer (treated as empty; must be 0).
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "k3_set_order.hpp"
#include "kernels.hpp"
#include "seg_walk.hpp"

namespace kmcpg {

namespace {

static_assert(K5_CAP == 64, "the wave class holds one pair per lane");

__device__ __forceinline__ double x_of(kmcpg_pair p, int32_t qk) { return printed_qcov(p.count, qk); }  // (k3_set_order.hpp)

__global__ void __launch_bounds__(256) k5_summary(K5Args a) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t r0 = ((uint64_t)blockIdx.x * 4 + wave) * RPW;
  if (r0 >= a.n_reads) return;  // wave-uniform
  const uint64_t mine = load_offsets(a.offs, r0, lane, a.n_reads);
  OwnRead own = own_read(mine, r0, lane, a.n_reads, a.pair_cap);
  const uint8_t verdict = own.live ? a.verdict[own.r] : K4_DROP;
  if (verdict == K4_DROP) own.seg.m = 0;
  const uint64_t m = own.seg.m;
  const int32_t qk = own.live ? a.nk[own.r] : 1;
  bool left = m > 0 && verdict == K4_HOST;
  const bool judged = m > 0 && !left;
  const ClassTables c{a.target_class, nullptr, a.n_cols};
  const MinMax<false> v = walk<false>(c, a.pairs, a.pair_cap, mine, lane, own, judged).v;
  const bool single = judged && v.one_target();
  uint32_t n_targets = single ? 1u : 0u;
  double score = single ? x_of(a.pairs[own.seg.s0], qk) : 0.0;
  if (judged && !single && m > K5_CAP) left = true;
  // several targets, up to K5_CAP pairs: one segment at a time by the whole wave
  const bool by_wave = judged && !single && !left;
  uint64_t multi = __ballot(by_wave && own.sub == 0);
  while (multi) {  // wave-uniform
    const int q = pop_group(multi);
    const Segment t = segment(mine, q, a.pair_cap);  // 2 <= t.m <= K5_CAP
    const int32_t tq = __shfl(qk, q * LPR, 64);
    const bool has = lane < t.m;
    const kmcpg_pair p = has ? a.pairs[t.s0 + lane] : kmcpg_pair{0u, 0u};
    const uint32_t cls = has ? class_of(c.target, c.n_cols, p.col, NO_CLASS) : 0u;
    const double x = has ? x_of(p, tq) : 0.0;
    uint64_t flagged = __ballot(first_of_class(cls, (uint32_t)t.m, lane));
    const uint32_t n = (uint32_t)__popcll(flagged);
    double sum = 0.0;  // (0 + x = x exactly: the first term needs no case of its own)
    while (flagged) {  // wave-uniform: every lane adds the same terms in the same order
      const int b = __ffsll((long long)flagged) - 1;
      flagged &= flagged - 1;
      sum = sum + __shfl(x, b, 64);
    }
    if (own.g == q) {
      n_targets = n;
      score = n > 1 ? sum / (double)n : sum;
    }
  }
  if (own.lead) {
    kmcpg_window_summary s;
    s.n_targets = left ? (uint32_t)m : n_targets;  // LEFT: the segment's length (the host rebuilds the LEFT offsets from these)
    s.flags = left ? KMCPG_SUMMARY_LEFT | (verdict == K4_HOST ? KMCPG_SUMMARY_HOST : 0u) : 0u;
    s.score = left ? 0.0 : score;
    a.out[own.r] = s;
    a.cnt[own.r] = left ? (uint32_t)m : 0u;
  }
  if (r0 + RPW >= a.n_reads && lane == 0) a.cnt[a.n_reads] = 0;  // the scan runs over n_reads + 1 words
  wave_add(&a.stats[0], wave_count(own.lead && single), lane);
  wave_add(&a.stats[1], wave_count(own.lead && by_wave), lane);
  wave_add(&a.stats[2], wave_count(own.lead && left), lane);
  wave_add(&a.stats[3], wave_count(own.lead && m == 0), lane);
  wave_add(&a.stats[4], wave_count(own.lead && own.seg.bad), lane);
}

}  // namespace

// stats (K5_STATS words) must be zero on entry; cnt: n_reads + 1 words, sums: k3_scan_tiles_for(n_reads + 1) + 1 words
void launch_k5(const K5Args& a, hipStream_t st, K4Log* log) {
  if (a.n_reads == 0) return;
  hipLaunchKernelGGL(k5_summary, dim3(walk_grid(a.n_reads)), dim3(256), 0, st, a);
  k4_note(log, KMCPG_K5_SUMMARY, walk_grid(a.n_reads), 256);
  launch_k3_scan(a.cnt, a.left_offs, a.sums, a.n_reads + 1, st, log);
  // the LEFT segments go where the new offsets say: k4_compact reads nothing else of its arguments
  K4Args c{};
  c.pairs = a.pairs;
  c.offs = a.offs;
  c.n_reads = a.n_reads;
  c.out_pairs = a.left_pairs;
  c.out_offs = a.left_offs;
  c.out_cap = a.left_cap;
  launch_k4_compact(c, st, log, KMCPG_K5_COMPACT);
}

}  // namespace kmcpg
