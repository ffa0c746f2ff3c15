// k6_refstats.hip — K6: what stage 1/4 of `kmcp profile` counts per reference, ON THE DEVICE, behind K3.
//
// Reference counterpart: kmcp/cmd/profile.go:761-1000 (the rule is restated in refstats_rule.hpp): every (target, chunk) is a column with
// four counters — rows, first rows of a target in a query, of those the unique queries', of those the ones with qCov >= H.  K3 leaves a
// batch's matches in HBM as (column, count) pairs grouped by read, in print order; target_class / species_class (kmcpg_set_refstats) say
// which columns are one printed target and which species it lies under.  A row's qCov as the TSV route parses it back is printed_qcov
// (k3_set_order.hpp), so "first.qCov >= H" has the bits `kmcp profile` compares.
//
//   k6_refstats  persistent workgroups; a wave takes RPW = 16 consecutive reads at a time in a grid-stride loop, the walk of k4_verdict /
//                k5_summary: lanes 0..16 hold the offsets, a read's lane group (4 lanes) reduces min / max of both classes over segments
//                of up to 64 pairs, the whole wave the longer ones.
//                  empty    no pairs                                                        nothing to count
//                  single   min == max of target_class (any length up to K3_WG_CAP)         rows for every pair; the first pair is the
//                                                                                           target's first row
//                  wave     several targets, up to K6_CAP pairs: lane i holds pair i; K5's loop clears "first of its class" in the later
//                           lanes of equal class; unique from min / max of species_class
//                  LEFT     more than final_n k-mers (the pairs still face the host's -f test), more than K3_WG_CAP pairs (K3 leaves them
//                           unordered: "first row" is not known), several targets among more than K6_CAP pairs: left[r] = 1, nothing counted
//
// Contention.  A metagenome puts a large share of its reads on a few references: plain global atomics would serialise tens of thousands
// of adds on a handful of addresses.  Every workgroup keeps an open-addressed table in LDS instead — key = column, four 32-bit counters
// per slot, LDS atomics — and adds each non-zero counter to global memory ONCE when it has taken its last read (64-bit atomics; the four
// counters of a column share a 32-byte sector).  A column that finds no slot within K6_PROBES probes goes straight to global memory.
// Integer adds commute: the counters are bitwise reproducible whatever the order.  matched / unique reads and the witness words are
// aggregated per wave over the whole loop: one atomic per wave and word.
//
// A batch whose hit buffer overflowed is run again as a whole (lane.cpp collect): with the batch's hit counter above the capacity the
// kernel returns at once (workgroup-uniform, before the first barrier) and the rerun does the counting.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "k3_set_order.hpp"
#include "kernels.hpp"

namespace kmcpg {

namespace {

constexpr int RPW = 16, LPR = 64 / RPW;  // reads per wave, lanes per read
constexpr uint32_t GROUP_CAP = 64;        // longest segment a lane group reduces
constexpr uint32_t NO_KEY = 0xffffffffu;
static_assert(K6_CAP == 64, "the wave class holds one pair per lane");

struct MinMax {
  uint32_t tmin, tmax, smin, smax;
};
__device__ __forceinline__ void take(MinMax& v, const K6Args& a, kmcpg_pair p) {
  const uint32_t t = p.col < a.n_cols ? a.target_class[p.col] : 0xffffffffu;  // (K3 emits no such column: never out of the table)
  v.tmin = min(v.tmin, t);
  v.tmax = max(v.tmax, t);
  if (a.species_class) {
    const uint32_t s = p.col < a.n_cols ? a.species_class[p.col] : 0u;
    v.smin = min(v.smin, s);
    v.smax = max(v.smax, s);
  }
}
__device__ __forceinline__ void fold(MinMax& v, int d) {
  v.tmin = min(v.tmin, (uint32_t)__shfl_xor((int)v.tmin, d, 64));
  v.tmax = max(v.tmax, (uint32_t)__shfl_xor((int)v.tmax, d, 64));
  v.smin = min(v.smin, (uint32_t)__shfl_xor((int)v.smin, d, 64));
  v.smax = max(v.smax, (uint32_t)__shfl_xor((int)v.smax, d, 64));
}
// specific_rule.hpp: one target, or one species that is not 0
__device__ __forceinline__ bool unique_of(const MinMax& v, bool species) { return v.tmin == v.tmax || (species && v.smin == v.smax && v.smin != 0); }

// the segment of read r0 + q as the wave's lanes hold the offsets (lane i: offs[r0 + i], i <= RPW); outside the buffer = empty
__device__ __forceinline__ void segment(uint64_t mine, int q, uint64_t cap, uint64_t* s0, uint64_t* m, bool* bad) {
  const uint64_t a = __shfl(mine, q, 64), b = __shfl(mine, q + 1, 64);
  *bad = b < a || b > cap;
  *s0 = a;
  *m = *bad ? 0 : b - a;
}

// The workgroup's table: keys[slots], then cnt[slots][4].  `mine` counts what this lane added where (the witness).
struct Table {
  uint32_t* keys;
  uint32_t* cnt;
  uint32_t slots, shift;  // slots: a power of two, or 0
  uint32_t lds_adds, spilled;
};
// the slot of a column, claimed if need be; -1: none within K6_PROBES probes (or no table) — the column's adds go straight to global memory
__device__ __forceinline__ int slot_of(const Table& t, uint32_t col) {
  if (t.slots == 0) return -1;
  uint32_t i = t.slots > 1 ? (col * 0x9E3779B1u) >> t.shift : 0u;
  for (uint32_t probe = 0; probe < K6_PROBES && probe < t.slots; probe++) {
    const uint32_t k = atomicCAS(&t.keys[i], NO_KEY, col);
    if (k == NO_KEY || k == col) return (int)i;
    i = (i + 1) & (t.slots - 1);
  }
  return -1;
}
__device__ __forceinline__ void bump(Table& t, const K6Args& a, int slot, uint32_t col, int word) {
  if (slot >= 0) {
    atomicAdd(&t.cnt[(uint32_t)slot * 4 + (uint32_t)word], 1u);
    t.lds_adds++;
  } else {
    atomicAdd(&a.counters[(uint64_t)col * 4 + (uint32_t)word], 1ull);
    t.spilled++;
  }
}
// one row of column p.col; `first`: it is its target's first row in the query (one probe of the table serves all of the pair's adds)
__device__ __forceinline__ void add_row(Table& t, const K6Args& a, kmcpg_pair p, int32_t qk, bool first, bool unique) {
  if (p.col >= a.n_cols) return;  // (never: the counters end at 4 * n_cols)
  const int slot = slot_of(t, p.col);
  bump(t, a, slot, p.col, 0);
  if (!first) return;
  bump(t, a, slot, p.col, 1);
  if (!unique) return;
  bump(t, a, slot, p.col, 2);
  if (printed_qcov(p.count, qk) >= a.hic_min_qcov) bump(t, a, slot, p.col, 3);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
  return v;
}

__global__ void __launch_bounds__(256) k6_refstats(K6Args a) {
  extern __shared__ uint32_t lds[];
  // the batch will be run again (its hit buffer overflowed): the rerun counts.  Every thread reads the same word: workgroup-uniform
  if (a.n_hits && *a.n_hits > a.hit_cap) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      atomicAdd(&a.stats[K6_SKIPPED], 1ull);
      atomicAdd(&a.totals[2], 1ull);
    }
    return;
  }
  Table t{lds, lds + a.slots, a.slots, a.slots > 1 ? 32u - (uint32_t)__ffs((int)a.slots) + 1u : 0u, 0u, 0u};
  for (uint32_t i = threadIdx.x; i < a.slots; i += blockDim.x) {
    t.keys[i] = NO_KEY;
    t.cnt[i * 4 + 0] = t.cnt[i * 4 + 1] = t.cnt[i * 4 + 2] = t.cnt[i * 4 + 3] = 0u;
  }
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool species = a.species_class != nullptr;
  const int g = (int)(lane / LPR), sub = (int)(lane % LPR);
  uint32_t n_matched = 0, n_unique = 0, n_empty = 0, n_single = 0, n_wave = 0, n_left = 0, n_bad = 0;  // lane 0 keeps the wave's counts
  for (uint64_t r0 = ((uint64_t)blockIdx.x * 4 + wave) * RPW; r0 < a.n_reads; r0 += (uint64_t)gridDim.x * 4 * RPW) {  // wave-uniform
    const uint64_t mine = a.offs[min(r0 + lane, (uint64_t)a.n_reads)];  // lanes 0..RPW hold offs[r0 + lane]
    const uint64_t r = r0 + (uint64_t)g;
    const bool live = r < a.n_reads;
    uint64_t s0, m;
    bool bad;
    segment(mine, g, a.pair_cap, &s0, &m, &bad);
    if (!live) m = 0, bad = false;
    const int32_t qk = live ? a.nk[r] : 1;
    bool left = m > 0 && (qk > a.final_n || m > (uint64_t)K3_WG_CAP);
    const bool judged = m > 0 && !left;
    // min / max of the classes: the lane group's strided loads and two butterfly steps (every lane takes part in the shuffles: the
    // partners sub ^ 1, sub ^ 2 are lanes of the same group, and a group's lanes agree on `small`)
    const bool small = judged && m <= GROUP_CAP;
    MinMax v{0xffffffffu, 0u, 0xffffffffu, 0u};
    if (small)
      for (uint32_t i = (uint32_t)sub; i < (uint32_t)m; i += LPR) take(v, a, a.pairs[s0 + i]);
    fold(v, 1);
    fold(v, 2);
    bool single = small && v.tmin == v.tmax;
    // one target, up to GROUP_CAP pairs (by far the common case): the lane group counts its rows; the first pair is the first row
    if (single) {
      for (uint32_t i = (uint32_t)sub; i < (uint32_t)m; i += LPR) {
        add_row(t, a, a.pairs[s0 + i], qk, i == 0, true);
      }
    }
    // the long segments, one after the other, by the whole wave: one target = counted here, several = LEFT
    uint64_t longs = __ballot(judged && !small && sub == 0);
    while (longs) {  // wave-uniform
      const int q = (__ffsll((long long)longs) - 1) / LPR;
      longs &= longs - 1;
      uint64_t t0, tm;
      bool tb;
      segment(mine, q, a.pair_cap, &t0, &tm, &tb);  // GROUP_CAP < tm <= K3_WG_CAP
      MinMax w{0xffffffffu, 0u, 0xffffffffu, 0u};
      for (uint64_t i = lane; i < tm; i += 64) take(w, a, a.pairs[t0 + i]);
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) fold(w, d);
      const bool one = w.tmin == w.tmax;  // wave-uniform
      if (one) {
        const int32_t tq = __shfl(qk, q * LPR, 64);
        for (uint64_t i = lane; i < tm; i += 64) {
          add_row(t, a, a.pairs[t0 + i], tq, i == 0, true);
        }
      }
      if (g == q) single = one, left = !one, v = w;
    }
    // several targets, up to K6_CAP pairs: one segment at a time by the whole wave, a pair per lane
    uint64_t multi = __ballot(judged && !single && !left && sub == 0);
    n_wave += (uint32_t)__popcll(multi);
    while (multi) {  // wave-uniform
      const int q = (__ffsll((long long)multi) - 1) / LPR;
      multi &= multi - 1;
      uint64_t t0, tm;
      bool tb;
      segment(mine, q, a.pair_cap, &t0, &tm, &tb);  // 2 <= tm <= K6_CAP
      const int32_t tq = __shfl(qk, q * LPR, 64);
      const bool uq = species && __shfl((int)v.smin, q * LPR, 64) == __shfl((int)v.smax, q * LPR, 64) && __shfl((int)v.smin, q * LPR, 64) != 0;
      const bool has = lane < tm;
      const kmcpg_pair p = has ? a.pairs[t0 + lane] : kmcpg_pair{0u, 0u};
      const uint32_t cls = has ? (p.col < a.n_cols ? a.target_class[p.col] : 0xffffffffu) : 0u;
      bool first = has;
      for (uint32_t j = 0; j + 1 < (uint32_t)tm; j++) {  // wave-uniform
        const uint32_t cj = (uint32_t)__shfl((int)cls, (int)j, 64);
        if (lane > j && cls == cj) first = false;
      }
      if (has) add_row(t, a, p, tq, first, uq);
    }
    const bool lead = live && sub == 0;
    if (lead) a.left[r] = left ? 1 : 0;
    const bool counted = lead && m > 0 && !left;
    n_matched += (uint32_t)__popcll(__ballot(counted));
    n_unique += (uint32_t)__popcll(__ballot(counted && unique_of(v, species)));
    n_empty += (uint32_t)__popcll(__ballot(lead && m == 0));
    n_single += (uint32_t)__popcll(__ballot(lead && single));
    n_left += (uint32_t)__popcll(__ballot(lead && left));
    n_bad += (uint32_t)__popcll(__ballot(lead && bad));
  }
  __syncthreads();
  // the table goes to global memory: one 64-bit add per non-zero counter
  uint32_t flushed = 0;
  for (uint32_t i = threadIdx.x; i < a.slots; i += blockDim.x) {
    const uint32_t col = t.keys[i];
    if (col == NO_KEY) continue;
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) {
      const uint32_t c = t.cnt[i * 4 + w];
      if (c) {
        atomicAdd(&a.counters[(uint64_t)col * 4 + w], (unsigned long long)c);
        flushed++;
      }
    }
  }
  const uint32_t lds_adds = wave_sum(t.lds_adds), spilled = wave_sum(t.spilled), globals = wave_sum(flushed) + spilled;
  if (lane == 0) {
    if (n_matched) atomicAdd(&a.totals[0], (unsigned long long)n_matched);
    if (n_unique) atomicAdd(&a.totals[1], (unsigned long long)n_unique);
    if (n_empty) atomicAdd(&a.stats[K6_EMPTY], (unsigned long long)n_empty);
    if (n_single) atomicAdd(&a.stats[K6_SINGLE], (unsigned long long)n_single);
    if (n_wave) atomicAdd(&a.stats[K6_WAVE], (unsigned long long)n_wave);
    if (n_left) atomicAdd(&a.stats[K6_LEFT], (unsigned long long)n_left);
    if (lds_adds) atomicAdd(&a.stats[K6_LDS_ADDS], (unsigned long long)lds_adds);
    if (globals) atomicAdd(&a.stats[K6_GLOBAL_ADDS], (unsigned long long)globals);
    if (spilled) atomicAdd(&a.stats[K6_SPILLED], (unsigned long long)spilled);
    if (n_bad) atomicAdd(&a.stats[K6_BAD], (unsigned long long)n_bad);
  }
}

}  // namespace

// grid: as many workgroups as the reads fill, at most `max_wgs` (the chip's resident workgroups; a test may pass fewer to force grid-stride
// rounds).  stats (K6_STATS words) must be zero on entry.  Returns the grid.
unsigned launch_k6(const K6Args& a, unsigned max_wgs, hipStream_t st, K4Log* log) {
  if (a.n_reads == 0) return 0;
  const uint64_t full = ((uint64_t)a.n_reads + 4 * RPW - 1) / (4 * RPW);
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(full, max_wgs));
  hipLaunchKernelGGL(k6_refstats, dim3(grid), dim3(256), (size_t)a.slots * 20, st, a);
  k4_note(log, KMCPG_K6_REFSTATS, grid, 256);
  return grid;
}

}  // namespace kmcpg
