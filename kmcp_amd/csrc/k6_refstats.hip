// k6_refstats.hip — K6: what stage 1/4 of `kmcp profile` counts per reference, ON THE DEVICE, behind K3.
//
// Reference counterpart: kmcp/cmd/profile.go:761-1000 (the rule is restated in refstats_rule.hpp): every (target, chunk) is a column with
// four counters — rows, first rows of a target in a query, of those the unique queries', of those the ones with qCov >= H.  K3 leaves a
// batch's matches in HBM as (column, count) pairs grouped by read, in print order; target_class / species_class (kmcpg_set_refstats) say
// which columns are one printed target and which species it lies under.  A row's qCov as the TSV route parses it back is printed_qcov
// (k3_set_order.hpp), so "first.qCov >= H" has the bits `kmcp profile` compares.
//
//   k6_refstats  persistent workgroups; a wave takes 16 consecutive reads at a time in a grid-stride loop, each time the walk of
//                seg_walk.hpp (a read's lane group reduces min / max of both classes over segments of up to 64 pairs, the whole wave the
//                longer ones — and counts their rows then and there when they have one target).
//                  empty    no pairs                                                        nothing to count
//                  single   min == max of target_class (any length up to K3_WG_CAP)         rows for every pair; the first pair is the
//                                                                                           target's first row
//                  wave     several targets, up to K6_CAP pairs: lane i holds pair i and whether it is the first of its class
//                           (first_of_class, seg_walk.hpp); unique from min / max of species_class
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
#include "seg_walk.hpp"

namespace kmcpg {

namespace {

constexpr uint32_t NO_KEY = 0xffffffffu;
static_assert(K6_CAP == 64 && K6_CAP == GROUP_CAP, "the wave class holds one pair per lane, and every longer segment is the walk's long class");

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
  const ClassTables c{a.target_class, a.species_class, a.n_cols};
  uint32_t n_matched = 0, n_unique = 0, n_empty = 0, n_single = 0, n_wave = 0, n_left = 0, n_bad = 0;  // the wave's counts over its rounds
  for (uint64_t r0 = ((uint64_t)blockIdx.x * 4 + wave) * RPW; r0 < a.n_reads; r0 += (uint64_t)gridDim.x * 4 * RPW) {  // wave-uniform
    const uint64_t mine = load_offsets(a.offs, r0, lane, a.n_reads);
    const OwnRead own = own_read(mine, r0, lane, a.n_reads, a.pair_cap);
    const uint64_t m = own.seg.m;
    const int32_t qk = own.live ? a.nk[own.r] : 1;
    bool left = m > 0 && (qk > a.final_n || m > (uint64_t)K3_WG_CAP);
    const bool judged = m > 0 && !left;
    // a long segment (GROUP_CAP < tm <= K3_WG_CAP) of one target is counted while the wave has it at hand; of several, it is LEFT
    const auto w = walk<true>(c, a.pairs, a.pair_cap, mine, lane, own, judged, [&](int q, uint64_t t0, uint64_t tm, const MinMax<true>& reduced) {
      if (!reduced.one_target()) return;  // wave-uniform
      const int32_t tq = __shfl(qk, q * LPR, 64);
      for (uint64_t i = lane; i < tm; i += 64) add_row(t, a, a.pairs[t0 + i], tq, i == 0, true);
    });
    const bool single = judged && w.v.one_target();
    if (judged && !single && m > K6_CAP) left = true;
    // one target, up to GROUP_CAP pairs (by far the common case): the lane group counts its rows; the first pair is the first row
    if (single && w.small)
      for (uint32_t i = (uint32_t)own.sub; i < (uint32_t)m; i += LPR) add_row(t, a, a.pairs[own.seg.s0 + i], qk, i == 0, true);
    // several targets, up to K6_CAP pairs: one segment at a time by the whole wave, a pair per lane
    const bool by_wave = judged && !single && !left, unique = w.v.one_target() || w.v.one_species();  // (specific_rule.hpp)
    uint64_t multi = __ballot(by_wave && own.sub == 0);
    while (multi) {  // wave-uniform
      const int q = pop_group(multi);
      const Segment s = segment(mine, q, a.pair_cap);  // 2 <= s.m <= K6_CAP
      const int32_t tq = __shfl(qk, q * LPR, 64);
      const bool uq = __shfl((int)unique, q * LPR, 64) != 0;
      const bool has = lane < s.m;
      const kmcpg_pair p = has ? a.pairs[s.s0 + lane] : kmcpg_pair{0u, 0u};
      const uint32_t cls = has ? class_of(c.target, c.n_cols, p.col, NO_CLASS) : 0u;
      const bool first = first_of_class(cls, (uint32_t)s.m, lane);
      if (has) add_row(t, a, p, tq, first, uq);
    }
    if (own.lead) a.left[own.r] = left ? 1 : 0;
    const bool counted = own.lead && m > 0 && !left;
    n_matched += wave_count(counted);
    n_unique += wave_count(counted && unique);
    n_empty += wave_count(own.lead && m == 0);
    n_single += wave_count(own.lead && single);
    n_wave += wave_count(own.lead && by_wave);
    n_left += wave_count(own.lead && left);
    n_bad += wave_count(own.lead && own.seg.bad);
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
  wave_add(&a.totals[0], n_matched, lane);
  wave_add(&a.totals[1], n_unique, lane);
  wave_add(&a.stats[K6_EMPTY], n_empty, lane);
  wave_add(&a.stats[K6_SINGLE], n_single, lane);
  wave_add(&a.stats[K6_WAVE], n_wave, lane);
  wave_add(&a.stats[K6_LEFT], n_left, lane);
  wave_add(&a.stats[K6_LDS_ADDS], lds_adds, lane);
  wave_add(&a.stats[K6_GLOBAL_ADDS], globals, lane);
  wave_add(&a.stats[K6_SPILLED], spilled, lane);
  wave_add(&a.stats[K6_BAD], n_bad, lane);
}

}  // namespace

// grid: as many workgroups as the reads fill, at most `max_wgs` (the chip's resident workgroups; a test may pass fewer to force grid-stride
// rounds).  stats (K6_STATS words) must be zero on entry.  Returns the grid.
unsigned launch_k6(const K6Args& a, unsigned max_wgs, hipStream_t st, K4Log* log) {
  if (a.n_reads == 0) return 0;
  const unsigned grid = std::max(1u, std::min(walk_grid(a.n_reads), max_wgs));
  hipLaunchKernelGGL(k6_refstats, dim3(grid), dim3(256), (size_t)a.slots * 20, st, a);
  k4_note(log, KMCPG_K6_REFSTATS, grid, 256);
  return grid;
}

}  // namespace kmcpg
