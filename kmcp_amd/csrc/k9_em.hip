// k9_em.hip — K9: one PASS of stage 4/4 of `kmcp profile` — abundance estimation by EM — ON THE DEVICE, over the read log K8 keeps in HBM.
//
// Reference counterpart: kmcp/cmd/profile.go:2031-2366, a full pass over the search result per EM iteration (the rule — the quotas, the cap,
// the integer shares, the two-word bases — is em_rule.hpp; its functions are what this file calls).
//
//   k9_em  persistent workgroups, a grid-stride loop over the logged reads: one read at a time by a whole wave, lane i holds pair i, exactly
//          as k8_replay reads the log.  Rows of classes outside the pass's whitelist are skipped; first_of_class gives the targets and one
//          wave-uniform loop over the ballot of first rows gives every row its target's row count and S, the sum of the targets' coverages
//          — a shuffle and an add per target, in first-row order: the host's addition order, the host's bits.  Every first-row lane
//          computes its quota; a second loop over the same ballot caps the quotas in the same order (em_rule.hpp) and leaves what no target
//          took, which the first target gets.  Then every kept row adds its five words.
//
// Contention: K8's scheme — a per-workgroup open-addressed table in LDS keyed by column, here FIVE 64-bit counters per slot (LDS 64-bit
// atomic adds; nothing can overflow between flushes), flushed once after the workgroup's last read; a column that finds no slot within
// K9_PROBES probes adds straight to global memory.  slots == 0: every add is a global 64-bit atomic.  Integer adds commute: the counters are
// bitwise reproducible whatever the grid and the table.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "em_rule.hpp"
#include "k3_set_order.hpp"
#include "kernels.hpp"
#include "seg_walk.hpp"

namespace kmcpg {

namespace {

constexpr uint32_t NO_KEY = 0xffffffffu;
constexpr uint32_t W = (uint32_t)EM_WORDS;
static_assert(K8_CAP == 64, "the pass holds one pair per lane");
static_assert((size_t)K9_MAX_SLOTS * (W * 8 + 4) * 2 <= 160 * 1024, "two workgroups' tables fit a CU's LDS");
typedef unsigned long long u64;

// The workgroup's table: cnt[slots][5] (64-bit), then keys[slots]
struct Table {
  u64* cnt;
  uint32_t* keys;
  uint32_t slots, shift;  // slots: a power of two, or 0
  u64* global;            // [5 * n_cols]
  uint32_t n_cols;
  uint32_t lds_adds, spilled, flushed;
};
__device__ __forceinline__ Table table_init(u64* lds, uint32_t slots, u64* global, uint32_t n_cols) {
  Table t{lds, (uint32_t*)(lds + (size_t)slots * W), slots, slots > 1 ? 32u - (uint32_t)__ffs((int)slots) + 1u : 0u, global, n_cols, 0u, 0u, 0u};
  for (uint32_t i = threadIdx.x; i < slots; i += blockDim.x) {
    t.keys[i] = NO_KEY;
    for (uint32_t w = 0; w < W; w++) t.cnt[i * W + w] = 0ull;
  }
  return t;
}
// the slot of a column, claimed if need be; -1: none within K9_PROBES probes (or no table)
__device__ __forceinline__ int slot_of(const Table& t, uint32_t col) {
  if (t.slots == 0) return -1;
  uint32_t i = t.slots > 1 ? (col * 0x9E3779B1u) >> t.shift : 0u;
  for (uint32_t probe = 0; probe < K9_PROBES && probe < t.slots; probe++) {
    const uint32_t k = atomicCAS(&t.keys[i], NO_KEY, col);
    if (k == NO_KEY || k == col) return (int)i;
    i = (i + 1) & (t.slots - 1);
  }
  return -1;
}
// one row's adds to the five counters of its column (one probe of the table serves all of them)
__device__ __forceinline__ void add_row(Table& t, uint32_t col, const u64 (&v)[EM_WORDS]) {
  if (col >= t.n_cols) return;  // (never: an estimated row's column has a class; the counters end at 5 * n_cols)
  const int slot = slot_of(t, col);
#pragma unroll
  for (uint32_t w = 0; w < W; w++) {
    if (!v[w]) continue;
    if (slot >= 0) {
      atomicAdd(&t.cnt[(uint32_t)slot * W + w], v[w]);
      t.lds_adds++;
    } else {
      atomicAdd(&t.global[(uint64_t)col * W + w], v[w]);
      t.spilled++;
    }
  }
}
// the table goes to global memory: one 64-bit add per non-zero counter (after a __syncthreads)
__device__ __forceinline__ void table_flush(Table& t) {
  for (uint32_t i = threadIdx.x; i < t.slots; i += blockDim.x) {
    const uint32_t col = t.keys[i];
    if (col == NO_KEY) continue;
    for (uint32_t w = 0; w < W; w++) {
      const u64 c = t.cnt[i * W + w];
      if (c) {
        atomicAdd(&t.global[(uint64_t)col * W + w], c);
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

__global__ void __launch_bounds__(256) k9_em(K9Args a) {
  extern __shared__ u64 lds[];
  Table t = table_init(lds, a.slots, a.counters, a.n_cols);
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t n_reads = 0, n_none = 0, n_one = 0, n_split = 0;  // (wave-uniform)
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
    // rows of classes outside the whitelist are skipped before anything else
    uint32_t cls = has ? class_of(a.target_class, a.n_cols, col, NO_CLASS) : NO_CLASS;
    const bool est = cls < a.n_classes && a.classes[cls].est != 0;
    if (!est) cls = NO_CLASS;
    const bool first = first_of_class(cls, m, lane) && est;
    const uint64_t firsts = __ballot(first);
    const uint32_t nt = (uint32_t)__popcll(firsts);
    if (nt == 0) {
      n_none++;
      continue;
    }
    const double qcov = est ? printed_qcov(count, qk) : 0.0;
    const double cov = first ? a.classes[cls].coverage : 0.0;
    // every row: the rows of its target and the lane of its first row; S in first-row order
    uint32_t my_m = 0, my_f = 0;
    double sum = 0;
    for (uint64_t f = firsts; f; f &= f - 1) {  // wave-uniform
      const int g = __ffsll((long long)f) - 1;
      const uint32_t cg = (uint32_t)__shfl((int)cls, g, 64);
      const uint64_t same = __ballot(est && cls == cg);
      if (est && cls == cg) my_m = (uint32_t)__popcll(same), my_f = (uint32_t)g;
      sum += __shfl(cov, g, 64);
    }
    u64 p = 0;
    bool uniq_first = true;
    if (nt > 1) {  // wave-uniform
      const u64 quota = first ? em_quota(cov, sum) : 0ull;
      u64 room = EM_UNIT;
      for (uint64_t f = firsts; f; f &= f - 1) {  // wave-uniform, and so is room
        const int g = __ffsll((long long)f) - 1;
        const u64 qg = __shfl(quota, g, 64), pg = qg < room ? qg : room;
        room -= pg;
        if ((int)lane == g) p = pg;
      }
      if ((int)lane == __ffsll((long long)firsts) - 1) p += room;
      // the targets under one species?
      const uint32_t sp = first ? class_of(a.species_class, a.n_cols, col, 0u) : 0u;
      uint32_t smin = first ? sp : 0xffffffffu, smax = first ? sp : 0u;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        smin = min(smin, (uint32_t)__shfl_xor((int)smin, d, 64));
        smax = max(smax, (uint32_t)__shfl_xor((int)smax, d, 64));
      }
      uniq_first = a.level_species && smin == smax && smin != 0;
    }
    const u64 pt = __shfl(p, (int)my_f, 64);
    if (est) {
      const u64 share = nt == 1 ? em_single_share(my_m, first) : em_row_share(pt, my_m, first);
      const u64 u = first && uniq_first ? (nt == 1 ? EM_UNIT : share) : 0ull;
      uint64_t lo, hi;
      em_bases(qlen, share, &lo, &hi);
      const u64 v[EM_WORDS] = {share, u, qcov >= a.hic_min_qcov ? u : 0ull, lo, hi};
      add_row(t, col, v);
    }
    n_one += nt == 1;
    n_split += nt > 1;
  }
  __syncthreads();
  table_flush(t);
  const uint32_t lds_adds = wave_sum(t.lds_adds), spilled = wave_sum(t.spilled), globals = wave_sum(t.flushed) + spilled;
  wave_add(&a.stats[K9_READS], n_reads, lane);
  wave_add(&a.stats[K9_NONE], n_none, lane);
  wave_add(&a.stats[K9_ONE], n_one, lane);
  wave_add(&a.stats[K9_SPLIT], n_split, lane);
  wave_add(&a.stats[K9_LDS_ADDS], lds_adds, lane);
  wave_add(&a.stats[K9_GLOBAL_ADDS], globals, lane);
  wave_add(&a.stats[K9_SPILLED], spilled, lane);
}

}  // namespace

// grid: a wave per 16 logged reads, at most `max_wgs` workgroups (a test may pass few to force grid-stride rounds).  counters and stats
// (K9_STATS words) must be zero on entry.  Returns the grid
unsigned launch_k9_em(const K9Args& a, unsigned max_wgs, hipStream_t st, K4Log* log) {
  if (a.n_logged == 0) return 0;
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((a.n_logged + 63) / 64, max_wgs));
  hipLaunchKernelGGL(k9_em, dim3(grid), dim3(256), (size_t)a.slots * (W * 8 + 4), st, a);
  k4_note(log, KMCPG_K9_EM, grid, 256);
  return grid;
}

}  // namespace kmcpg
