// k10_left.hip — K10: the pairs of the reads the counting stages LEFT, brought together ON THE DEVICE, behind K6, K7 and K8.
//
// No reference counterpart: `kmcp profile` reads every row of a search result.  Here the counting stages (engine.hpp) count almost every
// read of a batch on the device and write one byte per read for those they did not take; the host half (finalize.cpp left_reads_host) needs
// the final pairs of exactly those reads.  A statistics-only search (kmcpg_submit_stats) brings nothing else of K3's output to the host:
//   k10_left_mask  the walk of seg_walk.hpp (one wave per 16 consecutive reads; only the lane that leads a read's lane group has work:
//                  the stage reduces nothing).  mask[r] = OR over the stages given of (left[s][r] != 0) << s; cnt[r] = the length of the
//                  read's segment in K3's output where mask[r] != 0, else 0.
//   k3_scan_*      exclusive scan of cnt (k3_finalize.hip), into scratch offsets
//   k4_compact     the LEFT segments, and only those, copied to left_pairs (k4_specific.hip)
//   k10_left_offs  the scratch offsets -> left_offs
// The overflow guard of the counting kernels: a batch whose hit buffer overflowed will be run again, and none of its outputs may be taken
// for a result.  k10_left_mask then writes no mask byte and zeroes cnt, so that the scan and k4_compact behind it move nothing, and
// k10_left_offs leaves left_offs alone: mask, left_pairs and left_offs keep what they held.
// Counters (wave-aggregated: one atomic per wave and word): reads with at least one pair, LEFT reads, their pairs, segments outside the
// pair buffer (treated as empty; must be 0), launches the guard skipped.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "kernels.hpp"
#include "seg_walk.hpp"

namespace kmcpg {

namespace {

__device__ __forceinline__ bool overflowed(const unsigned long long* n_hits, uint64_t hit_cap) { return n_hits && *n_hits > hit_cap; }

__global__ void __launch_bounds__(256) k10_left_mask(K10Args a) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t r0 = ((uint64_t)blockIdx.x * 4 + wave) * RPW;
  if (r0 >= a.n_reads) return;  // wave-uniform
  const bool last = r0 + RPW >= a.n_reads;
  if (overflowed(a.n_hits, a.hit_cap)) {  // every thread reads the same word: uniform over the grid
    if (lane < RPW && r0 + lane < a.n_reads) a.cnt[r0 + lane] = 0;
    if (last && lane == 0) a.cnt[a.n_reads] = 0;
    if (r0 == 0 && lane == 0) atomicAdd(&a.stats[K10_SKIPPED], 1ull);
    return;
  }
  const uint64_t mine = load_offsets(a.offs, r0, lane, a.n_reads);
  const OwnRead own = own_read(mine, r0, lane, a.n_reads, a.pair_cap);
  uint32_t mask = 0;
  if (own.lead) {
#pragma unroll
    for (int s = 0; s < K10_STAGES; s++)
      if (a.left[s] && a.left[s][own.r] != 0) mask |= 1u << s;
  }
  const bool left = own.lead && mask != 0;
  const uint64_t m = left ? own.seg.m : 0;
  if (own.lead) {
    a.mask[own.r] = (uint8_t)mask;
    a.cnt[own.r] = (uint32_t)m;
  }
  if (last && lane == 0) a.cnt[a.n_reads] = 0;  // the scan runs over n_reads + 1 words
  wave_add(&a.stats[K10_MATCHED], wave_count(own.lead && own.seg.m > 0), lane);
  wave_add(&a.stats[K10_LEFT], wave_count(left), lane);
  const uint64_t pairs = wave_sum64(m);
  if (lane == 0 && pairs) atomicAdd(&a.stats[K10_LEFT_PAIRS], (unsigned long long)pairs);
  wave_add(&a.stats[K10_BAD], wave_count(own.lead && own.seg.bad), lane);
}

__global__ void __launch_bounds__(256) k10_left_offs(const uint64_t* __restrict__ from, uint64_t* __restrict__ to, uint32_t n, const unsigned long long* n_hits,
                                                     uint64_t hit_cap) {
  if (overflowed(n_hits, hit_cap)) return;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) to[i] = from[i];
}

}  // namespace

// stats (K10_STATS words) must be zero on entry; a.cnt: n_reads + 1 words, sums: k3_scan_tiles_for(n_reads + 1) + 1 words, offs_tmp and
// left_offs: n_reads + 1 words; left_cap >= a.pair_cap
void launch_k10(const K10Args& a, const kmcpg_pair* pairs, uint64_t* sums, uint64_t* offs_tmp, kmcpg_pair* left_pairs, uint64_t left_cap, uint64_t* left_offs,
                hipStream_t st, K4Log* log) {
  if (a.n_reads == 0) return;
  hipLaunchKernelGGL(k10_left_mask, dim3(walk_grid(a.n_reads)), dim3(256), 0, st, a);
  k4_note(log, KMCPG_K10_MASK, walk_grid(a.n_reads), 256);
  launch_k3_scan(a.cnt, offs_tmp, sums, a.n_reads + 1, st, log);
  // the LEFT segments go where the new offsets say: k4_compact reads nothing else of its arguments
  K4Args c{};
  c.pairs = pairs;
  c.offs = a.offs;
  c.n_reads = a.n_reads;
  c.out_pairs = left_pairs;
  c.out_offs = offs_tmp;
  c.out_cap = left_cap;
  launch_k4_compact(c, st, log, KMCPG_K10_COMPACT);
  const unsigned grid = (unsigned)(((uint64_t)a.n_reads + 1 + 255) / 256);
  hipLaunchKernelGGL(k10_left_offs, dim3(grid), dim3(256), 0, st, offs_tmp, left_offs, a.n_reads + 1, a.n_hits, a.hit_cap);
  k4_note(log, KMCPG_K10_OFFS, grid, 256);
}

}  // namespace kmcpg
