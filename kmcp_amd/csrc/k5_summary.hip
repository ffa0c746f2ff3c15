// k5_summary.hip — K5: a window's summary for region merging, ON THE DEVICE, behind K4.
//
// Reference counterpart: what `kmcp utils merge-regions` derives from the rows of one query before it merges (merge-regions.go:256-279;
// the rule is restated in regions_rule.hpp): n = the distinct targets among the query's rows, score = the qCov of the first row of each
// distinct target added in order of first appearance (float64), divided by n when n > 1.  K4 leaves the surviving windows' matches in HBM
// as (column, count) pairs in print order; target_class (kmcpg_set_specific) says which columns are one printed target.  A row's qCov as
// the TSV route parses it back is x = fixed4(count / qkmers) / 10000 (k3_set_order.hpp: the digits "%.4f" prints; both divisions are
// correctly rounded, -ffp-contract=off, no fast-math), so the 16-byte record written here has the bits the three-command pipeline computes.
//
//   k5_summary  one wave per RPW = 16 consecutive windows, the walk of k4_verdict: lanes 0..16 hold the offsets; a window's lane group
//               (4 lanes) reduces min / max of target_class over segments of up to 64 pairs, the whole wave the longer ones.
//                 empty    no pairs, or verdict DROP                      n = 0
//                 single   min == max (ANY length; by far the common case) n = 1, score = x of the segment's first pair
//                 wave     several targets, up to K5_CAP pairs: lane i holds pair i; a wave-uniform loop over the pairs clears "first
//                          of its class" in the later lanes of equal class; the flagged x are added in ascending lane order in float64
//                          by every lane alike (shuffles), then divided by n
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

namespace kmcpg {

namespace {

constexpr int RPW = 16, LPR = 64 / RPW;  // windows per wave, lanes per window
constexpr uint32_t GROUP_CAP = 64;        // longest segment a lane group reduces
static_assert(K5_CAP == 64, "the wave class holds one pair per lane");

__device__ __forceinline__ uint32_t class_of(const K5Args& a, kmcpg_pair p) {
  return p.col < a.n_cols ? a.target_class[p.col] : 0xffffffffu;  // (K3 emits no such column: never out of the table)
}
__device__ __forceinline__ double x_of(kmcpg_pair p, int32_t qk) { return printed_qcov(p.count, qk); }  // (k3_set_order.hpp)

struct MinMax {
  uint32_t tmin, tmax;
};
__device__ __forceinline__ void fold(MinMax& v, int d) {
  v.tmin = min(v.tmin, (uint32_t)__shfl_xor((int)v.tmin, d, 64));
  v.tmax = max(v.tmax, (uint32_t)__shfl_xor((int)v.tmax, d, 64));
}

// the segment of window r0 + q as the wave's lanes hold the offsets (lane i: offs[r0 + i], i <= RPW); outside the buffer = empty
__device__ __forceinline__ void segment(uint64_t mine, int q, uint64_t cap, uint64_t* s0, uint64_t* m, bool* bad) {
  const uint64_t a = __shfl(mine, q, 64), b = __shfl(mine, q + 1, 64);
  *bad = b < a || b > cap;
  *s0 = a;
  *m = *bad ? 0 : b - a;
}

__global__ void __launch_bounds__(256) k5_summary(K5Args a) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t r0 = ((uint64_t)blockIdx.x * 4 + wave) * RPW;
  if (r0 >= a.n_reads) return;  // wave-uniform
  const uint64_t mine = a.offs[min(r0 + lane, (uint64_t)a.n_reads)];  // lanes 0..RPW hold offs[r0 + lane]
  const int g = (int)(lane / LPR), sub = (int)(lane % LPR);
  const uint64_t r = r0 + (uint64_t)g;
  const bool live = r < a.n_reads;
  uint64_t s0, m;
  bool bad;
  segment(mine, g, a.pair_cap, &s0, &m, &bad);
  if (!live) m = 0, bad = false;
  const uint8_t verdict = live ? a.verdict[r] : K4_DROP;
  if (verdict == K4_DROP) m = 0;
  const int32_t qk = live ? a.nk[r] : 1;
  bool left = m > 0 && verdict == K4_HOST;
  const bool judged = m > 0 && !left;
  // min / max of the class: the lane group's strided loads and two butterfly steps (every lane takes part in the shuffles: the partners
  // sub ^ 1, sub ^ 2 are lanes of the same group, and a group's lanes agree on `small`), the long segments by the whole wave in turn
  const bool small = judged && m <= GROUP_CAP;
  MinMax v{0xffffffffu, 0u};
  if (small)
    for (uint32_t i = (uint32_t)sub; i < (uint32_t)m; i += LPR) {
      const uint32_t t = class_of(a, a.pairs[s0 + i]);
      v.tmin = min(v.tmin, t), v.tmax = max(v.tmax, t);
    }
  fold(v, 1);
  fold(v, 2);
  uint64_t longs = __ballot(judged && !small && sub == 0);
  while (longs) {  // wave-uniform
    const int q = (__ffsll((long long)longs) - 1) / LPR;
    longs &= longs - 1;
    uint64_t t0, tm;
    bool tb;
    segment(mine, q, a.pair_cap, &t0, &tm, &tb);
    MinMax w{0xffffffffu, 0u};
    for (uint64_t i = lane; i < tm; i += 64) {
      const uint32_t t = class_of(a, a.pairs[t0 + i]);
      w.tmin = min(w.tmin, t), w.tmax = max(w.tmax, t);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) fold(w, d);
    if (g == q) v = w;
  }
  const bool single = judged && v.tmin == v.tmax;
  uint32_t n_targets = single ? 1u : 0u;
  double score = single ? x_of(a.pairs[s0], qk) : 0.0;
  if (judged && !single && m > K5_CAP) left = true;
  // several targets, up to K5_CAP pairs: one segment at a time by the whole wave
  uint64_t multi = __ballot(judged && !single && !left && sub == 0);
  const uint32_t n_multi = (uint32_t)__popcll(multi);
  while (multi) {  // wave-uniform
    const int q = (__ffsll((long long)multi) - 1) / LPR;
    multi &= multi - 1;
    uint64_t t0, tm;
    bool tb;
    segment(mine, q, a.pair_cap, &t0, &tm, &tb);  // 2 <= tm <= K5_CAP
    const int32_t tq = __shfl(qk, q * LPR, 64);
    const bool has = lane < tm;
    const kmcpg_pair p = has ? a.pairs[t0 + lane] : kmcpg_pair{0u, 0u};
    const uint32_t cls = has ? class_of(a, p) : 0u;
    const double x = has ? x_of(p, tq) : 0.0;
    bool first = has;
    for (uint32_t j = 0; j + 1 < (uint32_t)tm; j++) {  // wave-uniform
      const uint32_t cj = (uint32_t)__shfl((int)cls, (int)j, 64);
      if (lane > j && cls == cj) first = false;
    }
    uint64_t flagged = __ballot(first);
    const uint32_t n = (uint32_t)__popcll(flagged);
    double sum = 0.0;  // (0 + x = x exactly: the first term needs no case of its own)
    while (flagged) {  // wave-uniform: every lane adds the same terms in the same order
      const int b = __ffsll((long long)flagged) - 1;
      flagged &= flagged - 1;
      sum = sum + __shfl(x, b, 64);
    }
    if (g == q) {
      n_targets = n;
      score = n > 1 ? sum / (double)n : sum;
    }
  }
  const bool lead = live && sub == 0;
  if (lead) {
    kmcpg_window_summary s;
    s.n_targets = left ? (uint32_t)m : n_targets;  // LEFT: the segment's length (the host rebuilds the LEFT offsets from these)
    s.flags = left ? KMCPG_SUMMARY_LEFT | (verdict == K4_HOST ? KMCPG_SUMMARY_HOST : 0u) : 0u;
    s.score = left ? 0.0 : score;
    a.out[r] = s;
    a.cnt[r] = left ? (uint32_t)m : 0u;
  }
  if (r0 + RPW >= a.n_reads && lane == 0) a.cnt[a.n_reads] = 0;  // the scan runs over n_reads + 1 words
  const uint64_t singles = __ballot(lead && single), lefts = __ballot(lead && left), empties = __ballot(lead && m == 0), bads = __ballot(lead && bad);
  if (lane == 0) {
    if (singles) atomicAdd(&a.stats[0], (uint32_t)__popcll(singles));
    if (n_multi) atomicAdd(&a.stats[1], n_multi);
    if (lefts) atomicAdd(&a.stats[2], (uint32_t)__popcll(lefts));
    if (empties) atomicAdd(&a.stats[3], (uint32_t)__popcll(empties));
    if (bads) atomicAdd(&a.stats[4], (uint32_t)__popcll(bads));
  }
}

}  // namespace

// stats (K5_STATS words) must be zero on entry; cnt: n_reads + 1 words, sums: k3_scan_tiles_for(n_reads + 1) + 1 words
void launch_k5(const K5Args& a, hipStream_t st, K4Log* log) {
  if (a.n_reads == 0) return;
  const unsigned grid = (unsigned)(((uint64_t)a.n_reads + 4 * RPW - 1) / (4 * RPW));
  hipLaunchKernelGGL(k5_summary, dim3(grid), dim3(256), 0, st, a);
  k4_note(log, KMCPG_K5_SUMMARY, grid, 256);
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
