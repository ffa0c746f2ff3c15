// k8_recount.hip — K8: stage 3/4 of `kmcp profile` — the recount with ambiguity correction — ON THE DEVICE, in two kernels.
//
// Reference counterpart: kmcp/cmd/profile.go:1282-1733 (the rule — the order, the loop in bit masks, the integer shares — is
// recount_rule.hpp; its predicate, row step and shares are the functions this file calls).  Stage 3 needs the FINAL verdicts of stage 1
// and the FINAL pair table of stage 2, which exist only after the last read: so the search keeps what it needs of every read, and the
// correction runs afterwards.
//
//   k8_log     behind K3 (after K4, K6 and K7; all of them only read K3's pairs), persistent workgroups on the walk of seg_walk.hpp:
//                empty    no pairs                                                 nothing
//                single   min == max of target_class (any length up to K3_WG_CAP)  counted at once by the ns == 1 rule: every row its
//                                                                                   match share and bases, the first row UNIT to uniq and —
//                                                                                   printed qCov >= H — to hic.  Unconditional: if stage 1
//                                                                                   drops the reference its columns are ignored at read-out,
//                                                                                   which is exact because the read touches no other
//                logged   several targets among up to K8_CAP pairs                 the read's pairs, NumKmers and qLen are appended to the
//                                                                                   read log (common.hpp: K8LogArgs) — completely or not at
//                                                                                   all; with no room the read is LEFT
//                LEFT     more than final_n k-mers, more than K3_WG_CAP pairs, several targets among more than K8_CAP pairs, no log room:
//                         left[r] = 1, nothing counted or logged
//   k8_replay  after the last batch, over the log: one read at a time by a whole wave, lane i holds pair i.  Rows of classes stage 1 dropped
//              are skipped; first_of_class gives the targets; their ranks by (printed qCov descending, first-row index ascending) come
//              from shuffles; for every live row i of the elimination lane j evaluates the predicate of (i, j) — one binary search in the
//              sorted pair list — and two ballots give A_i and B_i (recount_row): at most 63 wave-uniform steps.  Then every surviving row
//              adds its shares.
//
// Room in the log is taken with ONE fetch-add per wave and round for all of the round's reads (a compare-and-swap per read, retried by
// every wave that lost, cost 22 ms for 8 192 reads).  The reserve word only grows, so an allocation that does not fit is followed by none
// that does: the reads that fit are a prefix in the word's order — of the round that met the end, its first reads — and their records and
// index entries are dense.  What was really taken is the largest end of a fitting allocation: one atomic max on the commit word.  A wave
// that finds the reserve word past the end adds nothing to it (the word cannot run over).
//
// Contention.  A sample puts most reads on a few columns.  Every workgroup keeps an open-addressed table in LDS — key = column, four
// counters per slot — and adds each non-zero counter to global memory once, after its last read.  The shares are multiples of up to 720720
// and the bases of 2^16: the LDS counters are 64-BIT (LDS 64-bit atomic adds), so nothing can overflow between flushes.  A column that finds
// no slot within K8_PROBES probes adds straight to global memory.  Integer adds commute: the counters are bitwise reproducible.
//
// A batch whose hit buffer overflowed is run again as a whole (lane.cpp collect): with the batch's hit counter above the capacity k8_log
// returns at once (workgroup-uniform, before the first barrier) and the rerun counts and logs.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "k3_set_order.hpp"
#include "kernels.hpp"
#include "recount_rule.hpp"
#include "seg_walk.hpp"

namespace kmcpg {

namespace {

constexpr uint32_t NO_KEY = 0xffffffffu;
static_assert(K8_CAP == 64 && K8_CAP == GROUP_CAP, "the replay holds one pair per lane, and every longer segment is the walk's long class");
typedef unsigned long long u64;

// The workgroup's table: cnt[slots][4] (64-bit), then keys[slots].  lds_adds / spilled / flushed count what this lane added where
struct Table {
  u64* cnt;
  uint32_t* keys;
  uint32_t slots, shift;  // slots: a power of two, or 0
  u64* global;            // [4 * n_cols]
  uint32_t n_cols;
  uint32_t lds_adds, spilled, flushed;
};
__device__ __forceinline__ Table table_init(u64* lds, uint32_t slots, u64* global, uint32_t n_cols) {
  Table t{lds, (uint32_t*)(lds + (size_t)slots * 4), slots, slots > 1 ? 32u - (uint32_t)__ffs((int)slots) + 1u : 0u, global, n_cols, 0u, 0u, 0u};
  for (uint32_t i = threadIdx.x; i < slots; i += blockDim.x) {
    t.keys[i] = NO_KEY;
    t.cnt[i * 4 + 0] = t.cnt[i * 4 + 1] = t.cnt[i * 4 + 2] = t.cnt[i * 4 + 3] = 0ull;
  }
  return t;
}
// the slot of a column, claimed if need be; -1: none within K8_PROBES probes (or no table)
__device__ __forceinline__ int slot_of(const Table& t, uint32_t col) {
  if (t.slots == 0) return -1;
  uint32_t i = t.slots > 1 ? (col * 0x9E3779B1u) >> t.shift : 0u;
  for (uint32_t probe = 0; probe < K8_PROBES && probe < t.slots; probe++) {
    const uint32_t k = atomicCAS(&t.keys[i], NO_KEY, col);
    if (k == NO_KEY || k == col) return (int)i;
    i = (i + 1) & (t.slots - 1);
  }
  return -1;
}
// one row's adds to the four counters of its column (one probe of the table serves all of them)
__device__ __forceinline__ void add_row(Table& t, uint32_t col, u64 match, u64 uniq, u64 hic, u64 bases) {
  if (col >= t.n_cols) return;  // (never: the counters end at 4 * n_cols)
  const int slot = slot_of(t, col);
  const u64 v[RECOUNT_WORDS] = {match, uniq, hic, bases};
#pragma unroll
  for (uint32_t w = 0; w < (uint32_t)RECOUNT_WORDS; w++) {
    if (!v[w]) continue;
    if (slot >= 0) {
      atomicAdd(&t.cnt[(uint32_t)slot * 4 + w], v[w]);
      t.lds_adds++;
    } else {
      atomicAdd(&t.global[(uint64_t)col * 4 + w], v[w]);
      t.spilled++;
    }
  }
}
// the table goes to global memory: one 64-bit add per non-zero counter (after a __syncthreads)
__device__ __forceinline__ void table_flush(Table& t) {
  for (uint32_t i = threadIdx.x; i < t.slots; i += blockDim.x) {
    const uint32_t col = t.keys[i];
    if (col == NO_KEY) continue;
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) {
      const u64 c = t.cnt[i * 4 + w];
      if (c) {
        atomicAdd(&t.global[(uint64_t)col * 4 + w], c);
        t.flushed++;
      }
    }
  }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
  return v;
}

// a row of a read with ONE target of m rows (recount_rule.hpp: ns == 1)
__device__ __forceinline__ void add_single(Table& t, const K8LogArgs& a, kmcpg_pair p, int32_t qk, int32_t ql, uint64_t m, bool first) {
  const u64 u = first ? RECOUNT_UNIT : 0ull;
  add_row(t, p.col, recount_share(m, first), u, first && printed_qcov(p.count, qk) >= a.hic_min_qcov ? u : 0ull, recount_bases((uint64_t)max(ql, 0), 1, m));
}

constexpr u64 STATE_WORDS = (1ull << K8_STATE_WORD_BITS) - 1;

__global__ void __launch_bounds__(256) k8_log(K8LogArgs a) {
  extern __shared__ u64 lds[];
  // the batch will be run again (its hit buffer overflowed): the rerun counts.  Every thread reads the same word: workgroup-uniform
  if (a.n_hits && *a.n_hits > a.hit_cap) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      atomicAdd(&a.stats[K8_SKIPPED], 1ull);
      atomicAdd(&a.totals[K8_T_SKIPPED], 1ull);
    }
    return;
  }
  Table t = table_init(lds, a.slots, a.counters, a.n_cols);
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const ClassTables c{a.target_class, nullptr, a.n_cols};
  uint32_t n_empty = 0, n_single = 0, n_logged = 0, n_left = 0, n_full = 0, n_bad = 0;  // the wave's counts over its rounds
  for (uint64_t r0 = ((uint64_t)blockIdx.x * 4 + wave) * RPW; r0 < a.n_reads; r0 += (uint64_t)gridDim.x * 4 * RPW) {  // wave-uniform
    const uint64_t mine = load_offsets(a.offs, r0, lane, a.n_reads);
    const OwnRead own = own_read(mine, r0, lane, a.n_reads, a.pair_cap);
    const uint64_t m = own.seg.m;
    const int32_t qk = own.live ? a.nk[own.r] : 1, ql = own.live ? a.qlen[own.r] : 0;
    bool left = m > 0 && (qk > a.final_n || m > (uint64_t)K3_WG_CAP);
    const bool judged = m > 0 && !left;
    // a long segment (GROUP_CAP < tm <= K3_WG_CAP) of one target is counted while the wave has it at hand; of several, it is LEFT
    const auto w = walk<false>(c, a.pairs, a.pair_cap, mine, lane, own, judged, [&](int q, uint64_t t0, uint64_t tm, const MinMax<false>& reduced) {
      if (!reduced.one_target()) return;  // wave-uniform
      const int32_t tq = __shfl(qk, q * LPR, 64), tl = __shfl(ql, q * LPR, 64);
      for (uint64_t i = lane; i < tm; i += 64) add_single(t, a, a.pairs[t0 + i], tq, tl, tm, i == 0);
    });
    const bool single = judged && w.v.one_target();
    if (judged && !single && m > K8_CAP) left = true;
    // one target, up to GROUP_CAP pairs (by far the common case): the lane group counts its rows; the first pair is the first row
    if (single && w.small)
      for (uint32_t i = (uint32_t)own.sub; i < (uint32_t)m; i += LPR) add_single(t, a, a.pairs[own.seg.s0 + i], qk, ql, m, i == 0);
    // several targets, up to K8_CAP pairs: one read at a time by the whole wave, into the log
    const bool by_wave = judged && !single && !left;
    // room for the round's reads: the leading lane of read g holds the words and reads of the round's reads up to and including its own
    const bool asks = by_wave && own.sub == 0;
    uint64_t words = asks ? m + 2 : 0;
    uint32_t nth = asks ? 1u : 0u;
#pragma unroll
    for (int d = LPR; d < 64; d <<= 1) {
      const uint64_t w2 = __shfl_up(words, d, 64);
      const uint32_t n2 = (uint32_t)__shfl_up((int)nth, d, 64);
      if ((int)lane >= d) words += w2, nth += n2;
    }
    const uint64_t all_words = __shfl(words, 63 - (LPR - 1), 64);
    const uint32_t all_reads = (uint32_t)__shfl((int)nth, 63 - (LPR - 1), 64);
    u64 state = ~0ull;  // the reserve word before this round's reads; ~0: nothing was taken
    if (lane == 0 && all_reads) {
      const u64 seen = __hip_atomic_load(a.log_state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((seen & STATE_WORDS) + (seen >> K8_STATE_WORD_BITS) <= a.log_cap) state = atomicAdd(a.log_state, ((u64)all_reads << K8_STATE_WORD_BITS) | all_words);
    }
    state = __shfl(state, 0, 64);
    const u64 base_words = state & STATE_WORDS, base_reads = state >> K8_STATE_WORD_BITS;
    const bool fits = asks && state != ~0ull && base_words + words + base_reads + nth <= a.log_cap;  // (both sums grow with g: the reads that fit are the round's first)
    const uint64_t fit = __ballot(fits);
    if (fit) {  // the end of the last read that fits: what the log really holds
      const int last = 63 - __clzll((long long)fit);
      const uint64_t w_end = __shfl(words, last, 64);
      const uint32_t n_end = (uint32_t)__shfl((int)nth, last, 64);
      if (lane == 0) atomicMax(a.log_commit, ((base_reads + n_end) << K8_STATE_WORD_BITS) | (base_words + w_end));
    }
    const bool full = by_wave && !__shfl((int)fits, (int)(lane & ~(uint32_t)(LPR - 1)), 64);
    uint64_t multi = fit;
    while (multi) {  // wave-uniform: the reads that got room, one at a time by the whole wave
      const int q = pop_group(multi);
      const Segment s = segment(mine, q, a.pair_cap);  // 2 <= s.m <= K8_CAP
      const int32_t tq = __shfl(qk, q * LPR, 64), tl = __shfl(ql, q * LPR, 64);
      const uint64_t at = base_words + __shfl(words, q * LPR, 64) - (s.m + 2), idx = base_reads + (uint32_t)__shfl((int)nth, q * LPR, 64) - 1;
      {
        if (lane < s.m) {
          const kmcpg_pair p = a.pairs[s.s0 + lane];
          a.log[at + 2 + lane] = (u64)p.col | ((u64)p.count << 32);
        }
        if (lane == 0) {
          a.log[at] = (u64)s.m | ((u64)(uint32_t)tq << 32);
          a.log[at + 1] = (u64)max(tl, 0);
          a.log[a.log_cap - 1 - idx] = at;
        }
      }
    }
    if (own.lead) a.left[own.r] = left || full ? 1 : 0;
    n_empty += wave_count(own.lead && m == 0);
    n_single += wave_count(own.lead && single);
    n_logged += wave_count(own.lead && by_wave && !full);
    n_left += wave_count(own.lead && (left || full));
    n_full += wave_count(own.lead && full);
    n_bad += wave_count(own.lead && own.seg.bad);
  }
  __syncthreads();
  table_flush(t);
  const uint32_t lds_adds = wave_sum(t.lds_adds), spilled = wave_sum(t.spilled), globals = wave_sum(t.flushed) + spilled;
  wave_add(&a.totals[K8_T_SINGLE], n_single, lane);
  wave_add(&a.totals[K8_T_LEFT_FULL], n_full, lane);
  wave_add(&a.stats[K8_EMPTY], n_empty, lane);
  wave_add(&a.stats[K8_SINGLE], n_single, lane);
  wave_add(&a.stats[K8_LOGGED], n_logged, lane);
  wave_add(&a.stats[K8_LEFT], n_left, lane);
  wave_add(&a.stats[K8_LEFT_FULL], n_full, lane);
  wave_add(&a.stats[K8_LDS_ADDS], lds_adds, lane);
  wave_add(&a.stats[K8_GLOBAL_ADDS], globals, lane);
  wave_add(&a.stats[K8_SPILLED], spilled, lane);
  wave_add(&a.stats[K8_BAD], n_bad, lane);
}

// stage 2's count of a pair of classes: binary search in the sorted keys; 0 if the pair is absent
__device__ __forceinline__ uint64_t shared_reads(const K8ReplayArgs& a, uint32_t ca, uint32_t cb) {
  const u64 key = cooccur_key(ca, cb);
  uint64_t lo = 0, hi = a.n_pairs;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (a.keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < a.n_pairs && a.keys[lo] == key ? a.counts[lo] : 0ull;
}

__global__ void __launch_bounds__(256) k8_replay(K8ReplayArgs a) {
  extern __shared__ u64 lds[];
  Table t = table_init(lds, a.slots, a.counters, a.n_cols);
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t n_reads = 0, n_recounted = 0, n_corrected = 0, n_unique = 0, lookups = 0;  // (the first four wave-uniform)
  for (uint64_t k = (uint64_t)blockIdx.x * 4 + wave; k < a.n_logged; k += (uint64_t)gridDim.x * 4) {  // wave-uniform: one read, the whole wave
    const uint64_t at = a.log[a.log_cap - 1 - k];
    if (at + 2 > a.log_cap) continue;  // (never: k8_log wrote the index)
    const u64 w0 = a.log[at];
    const uint32_t m = (uint32_t)w0;
    const int32_t qk = (int32_t)(w0 >> 32);
    const uint64_t qlen = a.log[at + 1];
    if (m == 0 || m > K8_CAP || at + 2 + m > a.log_cap) continue;  // (never)
    n_reads++;
    const bool has = lane < m;
    const u64 pw = has ? a.log[at + 2 + lane] : 0ull;
    const uint32_t col = (uint32_t)pw, count = (uint32_t)(pw >> 32);
    // rows of targets that stage 1 dropped are skipped before anything else
    uint32_t cls = has ? class_of(a.target_class, a.n_cols, col, NO_CLASS) : NO_CLASS;
    const bool kept = cls < a.n_classes && a.classes[cls].kept != 0;
    if (!kept) cls = NO_CLASS;
    const bool first = first_of_class(cls, m, lane) && kept;
    const uint64_t firsts = __ballot(first);
    const uint32_t nt = (uint32_t)__popcll(firsts);
    if (nt == 0) continue;  // no kept target: not a read of stage 3
    const double qcov = kept ? printed_qcov(count, qk) : 0.0;
    // every row: the rows of its target and the lane of its first row; every first row: its target's rank by (qCov desc, first row asc)
    uint32_t my_m = 0, my_f = 0, rank = 0;
    for (uint64_t f = firsts; f; f &= f - 1) {  // wave-uniform
      const int g = __ffsll((long long)f) - 1;
      const uint32_t cg = (uint32_t)__shfl((int)cls, g, 64);
      const double qg = __shfl(qcov, g, 64);
      const uint64_t same = __ballot(kept && cls == cg);
      if (kept && cls == cg) my_m = (uint32_t)__popcll(same), my_f = (uint32_t)g;
      if (first && (qg > qcov || (qg == qcov && (uint32_t)g < lane))) rank++;
    }
    // lane r < nt takes the target of rank r
    uint32_t src = 0;
    for (uint64_t f = firsts; f; f &= f - 1) {  // wave-uniform
      const int g = __ffsll((long long)f) - 1;
      if ((uint32_t)__shfl((int)rank, g, 64) == lane) src = (uint32_t)g;
    }
    const bool is_t = lane < nt;
    const uint32_t rc = (uint32_t)__shfl((int)cls, (int)src, 64), rcol = (uint32_t)__shfl((int)col, (int)src, 64);
    uint64_t reads = 0, ureads = 0;
    if (is_t) reads = a.classes[rc].reads, ureads = a.classes[rc].ureads;
    // the elimination, a row of the loop per live i (recount_rule.hpp)
    uint64_t del = 0;
    if (nt > 1 && !a.no_amb_corr)
      for (uint32_t i = 0; i + 1 < nt; i++) {  // wave-uniform, and so is del
        if (del >> i & 1) continue;
        const uint32_t ci = (uint32_t)__shfl((int)rc, (int)i, 64);
        const uint64_t ri = __shfl(reads, (int)i, 64), ui = __shfl(ureads, (int)i, 64);
        int p = 0;
        if (is_t && lane > i && !(del >> lane & 1)) {
          p = recount_pred(ri, ui, reads, ureads, shared_reads(a, ci, rc), a.one_minus_d, a.r_err);
          lookups++;
        }
        del = recount_row(del, i, __ballot(p == 1), __ballot(p == 2));
      }
    const uint32_t ns = nt - (uint32_t)__popcll(del);
    // the survivors under one species?
    const bool surv = is_t && !(del >> lane & 1);
    const uint32_t sp = surv ? class_of(a.species_class, a.n_cols, rcol, 0u) : 0u;
    uint32_t smin = surv ? sp : 0xffffffffu, smax = surv ? sp : 0u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      smin = min(smin, (uint32_t)__shfl_xor((int)smin, d, 64));
      smax = max(smax, (uint32_t)__shfl_xor((int)smax, d, 64));
    }
    const bool uniq_first = ns == 1 || (a.level_species && smin == smax && smin != 0);
    // every surviving row adds its shares
    const uint32_t my_rank = (uint32_t)__shfl((int)rank, (int)my_f, 64);
    if (kept && !(del >> my_rank & 1)) {
      const u64 share = recount_share(my_m, first), u = first && uniq_first ? (ns == 1 ? RECOUNT_UNIT : share) : 0ull;
      add_row(t, col, share, u, qcov >= a.hic_min_qcov ? u : 0ull, recount_bases(qlen, ns, my_m));
    }
    n_recounted++;
    n_corrected += del != 0;
    n_unique += ns == 1;
  }
  __syncthreads();
  table_flush(t);
  const uint32_t lds_adds = wave_sum(t.lds_adds), spilled = wave_sum(t.spilled), globals = wave_sum(t.flushed) + spilled, looked = wave_sum(lookups);
  wave_add(&a.stats[K8_R_READS], n_reads, lane);
  wave_add(&a.stats[K8_R_RECOUNTED], n_recounted, lane);
  wave_add(&a.stats[K8_R_CORRECTED], n_corrected, lane);
  wave_add(&a.stats[K8_R_UNIQUE], n_unique, lane);
  wave_add(&a.stats[K8_R_LOOKUPS], looked, lane);
  wave_add(&a.stats[K8_R_LDS_ADDS], lds_adds, lane);
  wave_add(&a.stats[K8_R_GLOBAL_ADDS], globals, lane);
  wave_add(&a.stats[K8_R_SPILLED], spilled, lane);
}

}  // namespace

// grid: as many workgroups as the reads fill, at most `max_wgs` (the chip's resident workgroups; a test may pass fewer to force grid-stride
// rounds).  stats (K8_STATS words) must be zero on entry.  Returns the grid.
unsigned launch_k8_log(const K8LogArgs& a, unsigned max_wgs, hipStream_t st, K4Log* log) {
  if (a.n_reads == 0) return 0;
  const unsigned grid = std::max(1u, std::min(walk_grid(a.n_reads), max_wgs));
  hipLaunchKernelGGL(k8_log, dim3(grid), dim3(256), (size_t)a.slots * 36, st, a);
  k4_note(log, KMCPG_K8_LOG, grid, 256);
  return grid;
}
// grid: a wave per 16 logged reads, at most `max_wgs` workgroups.  counters and stats (K8_R_STATS words) must be zero on entry
unsigned launch_k8_replay(const K8ReplayArgs& a, unsigned max_wgs, hipStream_t st, K4Log* log) {
  if (a.n_logged == 0) return 0;
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((a.n_logged + 63) / 64, max_wgs));
  hipLaunchKernelGGL(k8_replay, dim3(grid), dim3(256), (size_t)a.slots * 36, st, a);
  k4_note(log, KMCPG_K8_REPLAY, grid, 256);
  return grid;
}

}  // namespace kmcpg
