// seg_walk.hpp — the walk over K3's (column, count) segments that the stages behind K3 share: K4 (k4_specific.hip), K5 (k5_summary.hip),
// K6 (k6_refstats.hip), K10 (k10_left.hip), K11 (k11_bin.hip).  Device code, and nothing stage-specific: what a stage does with a segment's reduced classes is its own.
//
// One wave takes RPW = 16 consecutive reads (as k3_sort_wave): lanes 0..16 load the offsets with one coalesced load, and the LPR = 4 lanes
// of lane group g work for read r0 + g.  A segment of up to GROUP_CAP = 64 pairs is reduced by its lane group (strided loads, two
// __shfl_xor steps), a longer one by the whole wave, one segment after the other (stride 64, six steps); the owning group then takes the
// wave's result over.  No LDS, no atomic per pair; the order inside a segment does not matter to min / max, so the unordered segments above
// K3_WG_CAP need nothing special.
//
// Two invariants carry the walk:
//   1. Every lane takes part in every shuffle.  The lane group's steps run outside `if (small)`, their partners sub ^ 1 and sub ^ 2 are
//      lanes of the same group, and a group's lanes must agree on `small` — so `judged` and the segment handed to walk() may depend on
//      the lane's GROUP only, never on the lane.  The loops over long segments are wave-uniform (their trip counts come from a ballot).
//   2. Reads past the end read offs[n_reads] twice (load_offsets clamps the index): their segment is empty, never out of bounds, and
//      own_read() reports them as not live with no pairs.  A wave whose first read lies past the end has nothing to do at all.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace kmcpg {

constexpr int RPW = 16, LPR = 64 / RPW;  // reads per wave, lanes per read
constexpr uint32_t GROUP_CAP = 64;        // longest segment a lane group reduces
constexpr uint32_t NO_CLASS = 0xffffffffu;

// workgroups of 256 threads that give every RPW reads a wave
inline unsigned walk_grid(uint32_t n_reads) { return (unsigned)(((uint64_t)n_reads + 4 * RPW - 1) / (4 * RPW)); }

// lanes 0..RPW hold words[r0 + lane]; past the end: words[n_reads] (invariant 2)
__device__ __forceinline__ uint64_t load_offsets(const uint64_t* words, uint64_t r0, uint32_t lane, uint32_t n_reads) {
  return words[min(r0 + lane, (uint64_t)n_reads)];
}

// the segment of read r0 + q as the wave's lanes hold the offsets (`mine` of load_offsets); outside the buffer = empty and bad
struct Segment {
  uint64_t s0, m;
  bool bad;
};
__device__ __forceinline__ Segment segment(uint64_t mine, int q, uint64_t cap) {
  const uint64_t a = __shfl(mine, q, 64), b = __shfl(mine, q + 1, 64);
  const bool bad = b < a || b > cap;
  return {a, bad ? 0 : b - a, bad};
}

// this lane's read — the one of its lane group — and its segment
struct OwnRead {
  int g, sub;  // the lane group and the lane's place in it
  uint64_t r;
  bool live, lead;  // the read exists; ... and this lane speaks for it (writes its outputs, counts it)
  Segment seg;
};
__device__ __forceinline__ OwnRead own_read(uint64_t mine, uint64_t r0, uint32_t lane, uint32_t n_reads, uint64_t pair_cap) {
  OwnRead o;
  o.g = (int)(lane / LPR), o.sub = (int)(lane % LPR);
  o.r = r0 + (uint64_t)o.g;
  o.live = o.r < n_reads;
  o.lead = o.live && o.sub == 0;
  o.seg = segment(mine, o.g, pair_cap);
  if (!o.live) o.seg.m = 0, o.seg.bad = false;
  return o;
}

// the lane group that leads a ballot's lowest set lane, taken off the mask (wave-uniform)
__device__ __forceinline__ int pop_group(uint64_t& mask) {
  const int q = (__ffsll((long long)mask) - 1) / LPR;
  mask &= mask - 1;
  return q;
}

// The two per-column tables.  A column's class in `table`; outside the table (K3 emits no such column) or without a table: `none`
struct ClassTables {
  const uint32_t *target, *species;  // species: nullptr at strain level
  uint32_t n_cols;
};
__device__ __forceinline__ uint32_t class_of(const uint32_t* table, uint32_t n_cols, uint32_t col, uint32_t none) {
  return table && col < n_cols ? table[col] : none;
}

// min / max of the target classes of a segment's pairs and — SPECIES — of their species classes (all 0 without a species table: never
// "one species").  Without SPECIES the two species words are neither loaded nor reduced.
template <bool SPECIES>
struct MinMax {
  uint32_t tmin = NO_CLASS, tmax = 0u, smin = NO_CLASS, smax = 0u;
  __device__ __forceinline__ void take(const ClassTables& c, kmcpg_pair p) {
    const uint32_t t = class_of(c.target, c.n_cols, p.col, NO_CLASS);
    tmin = min(tmin, t), tmax = max(tmax, t);
    if constexpr (SPECIES) {
      const uint32_t s = class_of(c.species, c.n_cols, p.col, 0u);
      smin = min(smin, s), smax = max(smax, s);
    }
  }
  // a lane group's share of up to GROUP_CAP pairs; the wave's share of any number
  __device__ __forceinline__ void take_group(const ClassTables& c, const kmcpg_pair* seg, uint32_t m, int sub) {
    for (uint32_t i = (uint32_t)sub; i < m; i += LPR) take(c, seg[i]);
  }
  __device__ __forceinline__ void take_wave(const ClassTables& c, const kmcpg_pair* seg, uint64_t m, uint32_t lane) {
    for (uint64_t i = lane; i < m; i += 64) take(c, seg[i]);
  }
  __device__ __forceinline__ void fold(int d) {
    tmin = min(tmin, (uint32_t)__shfl_xor((int)tmin, d, 64));
    tmax = max(tmax, (uint32_t)__shfl_xor((int)tmax, d, 64));
    if constexpr (SPECIES) {
      smin = min(smin, (uint32_t)__shfl_xor((int)smin, d, 64));
      smax = max(smax, (uint32_t)__shfl_xor((int)smax, d, 64));
    }
  }
  __device__ __forceinline__ void fold_group() { fold(1), fold(2); }
  __device__ __forceinline__ void fold_wave() {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) fold(d);
  }
  __device__ __forceinline__ bool one_target() const { return tmin == tmax; }
  __device__ __forceinline__ bool one_species() const { return SPECIES && smin == smax && smin != 0; }  // (specific_rule.hpp: species 0 is none)
};

// What walk() hands every lane: the reduced value of its group's segment (of nothing, where `judged` is false), and whether the lane
// group reduced it (`small`) or the wave did (judged && !small)
template <class V>
struct WalkedAs {
  V v;
  bool small;
};
template <bool SPECIES>
using Walked = WalkedAs<MinMax<SPECIES>>;
struct NoLongSegmentWork {
  template <class V>
  __device__ __forceinline__ void operator()(int, uint64_t, uint64_t, const V&) const {}
};
// The walk over a reduced value V (MinMax above; K11's node range in k11_bin.hip) and the tables C it reads: V() is the value of no pair,
// take_group / take_wave take a lane's share of a segment, fold_group / fold_wave bring the shares together with shuffles that EVERY lane
// of the group / the wave runs (invariant 1).  `own`: own_read()'s; `judged`: the group's segment is to be reduced (invariant 1: a
// function of the lane group).  on_long(q, t0, tm, reduced) is called wave-uniformly for every long segment — read r0 + q,
// pairs[t0 .. t0 + tm) — before its group takes `reduced` over: what a stage does with the whole wave at hand.
template <class V, class C, class OnLong = NoLongSegmentWork>
__device__ __forceinline__ WalkedAs<V> walk_as(const C& c, const kmcpg_pair* pairs, uint64_t pair_cap, uint64_t mine, uint32_t lane, const OwnRead& own, bool judged,
                                               OnLong on_long = OnLong()) {
  WalkedAs<V> out;
  out.small = judged && own.seg.m <= GROUP_CAP;
  if (out.small) out.v.take_group(c, pairs + own.seg.s0, (uint32_t)own.seg.m, own.sub);
  out.v.fold_group();
  uint64_t longs = __ballot(judged && !out.small && own.sub == 0);
  while (longs) {  // wave-uniform
    const int q = pop_group(longs);
    const Segment t = segment(mine, q, pair_cap);
    V w;
    w.take_wave(c, pairs + t.s0, t.m, lane);
    w.fold_wave();
    on_long(q, t.s0, t.m, w);
    if (own.g == q) out.v = w;
  }
  return out;
}
// ... over min / max of the classes: K4, K5, K6, K7, K8
template <bool SPECIES, class OnLong = NoLongSegmentWork>
__device__ __forceinline__ Walked<SPECIES> walk(const ClassTables& c, const kmcpg_pair* pairs, uint64_t pair_cap, uint64_t mine, uint32_t lane, const OwnRead& own,
                                                 bool judged, OnLong on_long = OnLong()) {
  return walk_as<MinMax<SPECIES>>(c, pairs, pair_cap, mine, lane, own, judged, on_long);
}

// Lane i holds pair i of a segment of tm <= 64 pairs and its class: is it the first of its class?  (wave-uniform loop; at most 63 shuffles)
__device__ __forceinline__ bool first_of_class(uint32_t cls, uint32_t tm, uint32_t lane) {
  bool first = lane < tm;
  for (uint32_t j = 0; j + 1 < tm; j++) {
    const uint32_t cj = (uint32_t)__shfl((int)cls, (int)j, 64);
    if (lane > j && cls == cj) first = false;
  }
  return first;
}

// Wave-aggregated counters: the lanes for which a predicate holds, and one atomic per wave and word (32- or 64-bit) for a count that is not 0
__device__ __forceinline__ uint32_t wave_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }
template <class Word>
__device__ __forceinline__ void wave_add(Word* word, uint32_t n, uint32_t lane) {
  if (lane == 0 && n) atomicAdd(word, (Word)n);
}
// ... and the sum of a 64-bit value over the wave's lanes (every lane takes part and gets the sum; a lane without a share holds 0)
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

}  // namespace kmcpg
