// k7_cooccur.hip — K7: what stage 2/4 of `kmcp profile` counts — the reads shared by every pair of references — ON THE DEVICE, behind K3.
//
// Reference counterpart: kmcp/cmd/profile.go:1117-1279 (the rule is restated in cooccur_rule.hpp): for every query with several targets,
// every unordered pair of its targets gets one more read.  K3 leaves a batch's matches in HBM as (column, count) pairs grouped by read;
// target_class (kmcpg_set_cooccur) says which columns are one printed target.
//
//   k7_cooccur  persistent workgroups; a wave takes 16 consecutive reads at a time in a grid-stride loop, each time the walk of seg_walk.hpp
//                 empty    no pairs                                              nothing
//                 single   min == max of target_class (any length)               nothing: no pair to count
//                 wave     several targets, up to K7_CAP pairs: one read at a time by the whole wave — lane i holds pair i, the lanes that
//                          are the first of their class (first_of_class, seg_walk.hpp) are the read's m distinct targets, and the
//                          m (m - 1) / 2 pairs are dealt out to the lanes, 64 at a time
//                 LEFT     more than final_n k-mers (the pairs still face the host's -f test), more than K3_WG_CAP pairs, several targets
//                          among more than K7_CAP pairs, or no room in the table (below): left[r] = 1, nothing counted
//
// The table is open-addressed in HBM (keys claimed with a 64-bit compare-and-swap, counts beside them; cooccur_rule.hpp has the key, the
// hash and the probe sequence).  A read is counted in two phases, so that a full table never leaves a read half-counted:
//   1. reserve  every pair of the read finds or claims its key's slot (idempotent: a key that is there stays, with whatever count it has);
//   2. if any pair found none, the read is LEFT ("table full") — the decision is the wave's (one ballot), nothing of the read is counted;
//   3. count    otherwise every pair looks its key up again — it cannot fail now, keys are never removed — and adds 1.
// Keys are read with agent-scope atomic loads: the claims of workgroups on other XCDs must be visible.
//
// Contention.  Two near-identical genomes share most of their reads: plain global atomics would put tens of thousands of adds on one
// address.  Every workgroup keeps an open-addressed table in LDS — key = the pair, one 32-bit counter per slot, LDS atomics.  A key is
// put there only AFTER its global slot is reserved, so a hit in the LDS table during the reserve phase means the global slot exists.  A
// pair that gets no LDS slot adds straight to global memory.  The workgroup flushes its non-zero counters once, after its last read: one
// 64-bit atomic per slot, to a global slot that is known to exist.  Integer adds commute: the table's contents are bitwise reproducible as
// a set of (key, count).
//
// A batch whose hit buffer overflowed is run again as a whole (lane.cpp collect): with the batch's hit counter above the capacity the
// kernel returns at once (workgroup-uniform, before the first barrier) and the rerun does the counting.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "cooccur_rule.hpp"
#include "kernels.hpp"
#include "seg_walk.hpp"

namespace kmcpg {

namespace {

static_assert(K7_CAP == 64 && K7_CAP == GROUP_CAP, "the wave class holds one pair per lane, and every longer segment is the walk's long class");
typedef unsigned long long u64;

struct Tables {
  // the workgroup's: keys[slots], then cnt[slots]
  u64* lkeys;
  uint32_t* lcnt;
  uint32_t lslots, llog2;  // lslots: a power of two, or 0
  // the handle's, in HBM
  u64* keys;
  u64* counts;
  uint64_t slots;
  uint32_t log2;
  // what this lane did (the witness)
  uint32_t lds_adds, global_adds, spilled, claimed;
};

__device__ __forceinline__ u64 load_key(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// cooccur_reserve / cooccur_find (cooccur_rule.hpp) on the table in HBM
__device__ __forceinline__ bool global_reserve(Tables& t, u64 key) {
  uint64_t i = cooccur_slot0(key, t.log2);
  for (uint32_t p = 0; p < cooccur_probes(t.slots); p++, i = cooccur_next(i, t.slots)) {
    u64 k = load_key(&t.keys[i]);
    if (k == COOCCUR_EMPTY) {
      k = atomicCAS(&t.keys[i], (u64)COOCCUR_EMPTY, key);
      if (k == COOCCUR_EMPTY) {
        t.claimed++;
        return true;
      }
    }
    if (k == key) return true;
  }
  return false;
}
__device__ __forceinline__ void global_add(Tables& t, u64 key, u64 n) {
  uint64_t i = cooccur_slot0(key, t.log2);
  for (uint32_t p = 0; p < cooccur_probes(t.slots); p++, i = cooccur_next(i, t.slots))
    if (load_key(&t.keys[i]) == key) {
      atomicAdd(&t.counts[i], n);
      t.global_adds++;
      return;
    }
  // (never: the key was reserved and keys are not removed)
}
// ... and on the workgroup's table: the slot of a key; claim: taken if need be.  -1: none within the probes, or no table
__device__ __forceinline__ int lds_slot(const Tables& t, u64 key, bool claim) {
  if (t.lslots == 0) return -1;
  uint32_t i = (uint32_t)cooccur_slot0(key, t.llog2);
  for (uint32_t p = 0; p < cooccur_probes(t.lslots); p++, i = (uint32_t)cooccur_next(i, t.lslots)) {
    u64 k = __hip_atomic_load(&t.lkeys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == COOCCUR_EMPTY && claim) {
      k = atomicCAS(&t.lkeys[i], (u64)COOCCUR_EMPTY, key);
      if (k == COOCCUR_EMPTY) return (int)i;
    }
    if (k == key) return (int)i;
  }
  return -1;
}

// phase 1 for one pair: false = no slot in HBM
__device__ __forceinline__ bool reserve(Tables& t, u64 key) {
  if (lds_slot(t, key, false) >= 0) return true;  // its global slot was reserved before it came here
  if (!global_reserve(t, key)) return false;
  (void)lds_slot(t, key, true);
  return true;
}
// phase 3 for one pair
__device__ __forceinline__ void count(Tables& t, u64 key) {
  const int s = lds_slot(t, key, false);
  if (s >= 0) {
    atomicAdd(&t.lcnt[s], 1u);
    t.lds_adds++;
  } else {
    global_add(t, key, 1ull);
    if (t.lslots) t.spilled++;
  }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
  return v;
}
// the lane of a mask's k-th set bit (k below its population count)
__device__ __forceinline__ int nth_lane(uint64_t mask, uint32_t k) {
  for (uint32_t i = 0; i < k; i++) mask &= mask - 1;
  return __ffsll((long long)mask) - 1;
}
// pair t of m targets, t < m (m - 1) / 2, in the order (0,1) (0,2) (1,2) (0,3) ...: j = the largest with j (j - 1) / 2 <= t, i = the rest
__device__ __forceinline__ void pair_of(uint32_t t, uint32_t* i, uint32_t* j) {
  uint32_t b = (uint32_t)((1.0f + sqrtf(1.0f + 8.0f * (float)t)) * 0.5f);  // t <= 2015: exact to within one, mended below
  while (b * (b - 1) / 2 > t) b--;
  while ((b + 1) * b / 2 <= t) b++;
  *j = b, *i = t - b * (b - 1) / 2;
}

__global__ void __launch_bounds__(256) k7_cooccur(K7Args a) {
  extern __shared__ u64 lds[];
  // the batch will be run again (its hit buffer overflowed): the rerun counts.  Every thread reads the same word: workgroup-uniform
  if (a.n_hits && *a.n_hits > a.hit_cap) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      atomicAdd(&a.stats[K7_SKIPPED], 1ull);
      atomicAdd(&a.totals[K7_T_SKIPPED], 1ull);
    }
    return;
  }
  Tables t{lds, (uint32_t*)(lds + a.slots), a.slots, cooccur_log2(a.slots), a.keys, a.counts, a.table_slots, cooccur_log2(a.table_slots), 0u, 0u, 0u, 0u};
  for (uint32_t i = threadIdx.x; i < a.slots; i += blockDim.x) t.lkeys[i] = COOCCUR_EMPTY, t.lcnt[i] = 0u;
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const ClassTables c{a.target_class, nullptr, a.n_cols};
  uint32_t n_empty = 0, n_single = 0, n_wave = 0, n_left = 0, n_full = 0, n_bad = 0;  // the wave's counts over its rounds
  u64 n_pairs = 0;                                                                   // (wave-uniform)
  for (uint64_t r0 = ((uint64_t)blockIdx.x * 4 + wave) * RPW; r0 < a.n_reads; r0 += (uint64_t)gridDim.x * 4 * RPW) {  // wave-uniform
    const uint64_t mine = load_offsets(a.offs, r0, lane, a.n_reads);
    const OwnRead own = own_read(mine, r0, lane, a.n_reads, a.pair_cap);
    const uint64_t m = own.seg.m;
    const int32_t qk = own.live ? a.nk[own.r] : 1;
    bool left = m > 0 && (qk > a.final_n || m > (uint64_t)K3_WG_CAP);
    const bool judged = m > 0 && !left;
    const auto w = walk<false>(c, a.pairs, a.pair_cap, mine, lane, own, judged);
    const bool single = judged && w.v.one_target();
    if (judged && !single && m > K7_CAP) left = true;
    // several targets, up to K7_CAP pairs: one read at a time by the whole wave
    const bool by_wave = judged && !single && !left;
    bool full = false;
    uint64_t multi = __ballot(by_wave && own.sub == 0);
    while (multi) {  // wave-uniform
      const int q = pop_group(multi);
      const Segment s = segment(mine, q, a.pair_cap);  // 2 <= s.m <= K7_CAP
      const bool has = lane < s.m;
      const uint32_t cls = has ? class_of(c.target, c.n_cols, a.pairs[s.s0 + lane].col, NO_CLASS) : NO_CLASS;
      const uint64_t firsts = __ballot(first_of_class(cls, (uint32_t)s.m, lane) && cls != NO_CLASS);
      const uint32_t nt = (uint32_t)__popcll(firsts), np = nt * (nt - 1) / 2;  // the read's distinct targets and their pairs
      const uint32_t tcls = (uint32_t)__shfl((int)cls, lane < nt ? nth_lane(firsts, lane) : 0, 64);  // lane i < nt: target i
      // reserve, decide (the wave's ballot: uniform over every lane that shares the read's shuffles), count
      bool failed = false;
      for (int phase = 0; phase < 2; phase++) {
        for (uint32_t base = 0; base < np; base += 64) {  // wave-uniform
          uint32_t i = 0, j = 0;
          const bool live = base + lane < np;
          if (live) pair_of(base + lane, &i, &j);
          const uint32_t ca = (uint32_t)__shfl((int)tcls, (int)i, 64), cb = (uint32_t)__shfl((int)tcls, (int)j, 64);
          if (!live) continue;
          const u64 key = cooccur_key(ca, cb);
          if (phase == 0) failed |= !reserve(t, key);
          else count(t, key);
        }
        if (phase == 0 && __ballot(failed)) break;  // table full: nothing of the read is counted
      }
      const bool rfull = __ballot(failed) != 0;
      if (own.g == q) full = rfull;
      if (!rfull) n_pairs += np;
    }
    if (own.lead) a.left[own.r] = left || full ? 1 : 0;
    n_empty += wave_count(own.lead && m == 0);
    n_single += wave_count(own.lead && single);
    n_wave += wave_count(own.lead && by_wave && !full);
    n_left += wave_count(own.lead && (left || full));
    n_full += wave_count(own.lead && full);
    n_bad += wave_count(own.lead && own.seg.bad);
  }
  __syncthreads();
  // the workgroup's table goes to global memory: one 64-bit add per non-zero counter, to a slot that exists
  for (uint32_t i = threadIdx.x; i < a.slots; i += blockDim.x) {
    const uint32_t n = t.lcnt[i];
    if (n) global_add(t, t.lkeys[i], (u64)n);
  }
  const uint32_t lds_adds = wave_sum(t.lds_adds), globals = wave_sum(t.global_adds), spilled = wave_sum(t.spilled), claimed = wave_sum(t.claimed);
  wave_add(&a.totals[K7_T_MULTI], n_wave, lane);
  if (lane == 0 && n_pairs) atomicAdd(&a.totals[K7_T_PAIRS], n_pairs), atomicAdd(&a.stats[K7_PAIRS], n_pairs);
  wave_add(&a.totals[K7_T_LEFT_FULL], n_full, lane);
  wave_add(&a.stats[K7_EMPTY], n_empty, lane);
  wave_add(&a.stats[K7_SINGLE], n_single, lane);
  wave_add(&a.stats[K7_WAVE], n_wave, lane);
  wave_add(&a.stats[K7_LEFT], n_left, lane);
  wave_add(&a.stats[K7_LEFT_FULL], n_full, lane);
  wave_add(&a.stats[K7_LDS_ADDS], lds_adds, lane);
  wave_add(&a.stats[K7_GLOBAL_ADDS], globals, lane);
  wave_add(&a.stats[K7_SPILLED], spilled, lane);
  wave_add(&a.stats[K7_CLAIMED], claimed, lane);
  wave_add(&a.stats[K7_BAD], n_bad, lane);
}

}  // namespace

// grid: as many workgroups as the reads fill, at most `max_wgs` (the chip's resident workgroups; a test may pass fewer to force grid-stride
// rounds).  stats (K7_STATS words) must be zero on entry.  Returns the grid.
unsigned launch_k7(const K7Args& a, unsigned max_wgs, hipStream_t st, K4Log* log) {
  if (a.n_reads == 0) return 0;
  const unsigned grid = std::max(1u, std::min(walk_grid(a.n_reads), max_wgs));
  hipLaunchKernelGGL(k7_cooccur, dim3(grid), dim3(256), (size_t)a.slots * 12, st, a);
  k4_note(log, KMCPG_K7_COOCCUR, grid, 256);
  return grid;
}

}  // namespace kmcpg
