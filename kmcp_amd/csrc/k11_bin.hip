// k11_bin.hip — K11: one TaxId per read, the read's taxonomic bin, ON THE DEVICE, behind K3.
//
// Reference counterpart: the binning pass of `kmcp profile -B` (kmcp/cmd/profile.go:2591-2784): a read's bin is the TaxId of the one
// whitelisted reference it matches, or the lowest common ancestor (LCA) of the TaxIds of the several.  The rule is bin_rule.hpp, which this
// file restates for the form the device sees — K3's (column, count) pairs and the plan's tables:
//   node_of_column[col]  the pre-order number, in the plan's pruned tree, of the column's target; NO_CLASS: not whitelisted (skipped by both
//                        the min and the max below)
//   parent / last / taxid  per node; [v, last[v]] is exactly v's subtree; node 0 is the virtual root and prints as TaxId 0
// The LCA of a set of nodes numbered in pre-order is the LCA of its smallest and its largest member (bin_rule.hpp says why), so a read
// needs a min and a max over its pairs — the reduction of the walk of seg_walk.hpp, with NodeRange as the reduced value: a lane group
// reduces segments of up to 64 pairs, the wave the longer ones, the unordered ones above K3_WG_CAP included (min and max do not care) —
// and then ONE climb, by the lane that leads the read: from the min up until the subtree reaches the max.
//   bins[r] = taxid[lca]   the read has a whitelisted pair
//           = K11_NONE     it has none (no pair at all, or none of a whitelisted target): no line
//           = K11_LEFT     it has pairs and more than final_n k-mers: exactly the reads K4 leaves (k4_specific.hip) — their pairs may still
//                          fall to -f on the host, which bins them by bin_rule.hpp
// Persistent waves: the grid is capped and a wave takes 16 reads per round.  The three tables sit in LDS when the plan has at most
// K11_LDS_NODES nodes (the whitelist of a real sample is tens to hundreds of references), else the climb reads global memory.
// The overflow guard of the counting stages: with the batch's hit counter above capacity the launch returns at once — bins keeps what it
// held — and the rerun writes the bins.  There are no row cuts here: the GPU route has none (bin_rule.hpp's are the host tool's).
// Counters (wave-aggregated): reads without a bin / of one node / of several / LEFT, climb steps, segments outside the pair buffer (treated
// as empty; must be 0), launches the guard skipped.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "seg_walk.hpp"

namespace kmcpg {

namespace {

struct BinTables {
  const uint32_t* node;
  uint32_t n_cols, n_nodes;
};

// min / max of the nodes of a segment's WHITELISTED pairs; lo == NO_CLASS: there was none
struct NodeRange {
  uint32_t lo = NO_CLASS, hi = 0u;
  __device__ __forceinline__ void take(const BinTables& c, kmcpg_pair p) {
    const uint32_t v = class_of(c.node, c.n_cols, p.col, NO_CLASS);
    if (v < c.n_nodes) lo = min(lo, v), hi = max(hi, v);  // (NO_CLASS is no node; the host refuses a table with any other number that is none)
  }
  __device__ __forceinline__ void take_group(const BinTables& c, const kmcpg_pair* seg, uint32_t m, int sub) {
    for (uint32_t i = (uint32_t)sub; i < m; i += LPR) take(c, seg[i]);
  }
  __device__ __forceinline__ void take_wave(const BinTables& c, const kmcpg_pair* seg, uint64_t m, uint32_t lane) {
    for (uint64_t i = lane; i < m; i += 64) take(c, seg[i]);
  }
  __device__ __forceinline__ void fold(int d) {
    lo = min(lo, (uint32_t)__shfl_xor((int)lo, d, 64));
    hi = max(hi, (uint32_t)__shfl_xor((int)hi, d, 64));
  }
  __device__ __forceinline__ void fold_group() { fold(1), fold(2); }
  __device__ __forceinline__ void fold_wave() {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) fold(d);
  }
  __device__ __forceinline__ bool none() const { return lo == NO_CLASS; }
};

template <bool LDS>
__global__ void __launch_bounds__(256) k11_bin(K11Args a) {
  extern __shared__ uint32_t lds[];
  // the batch will be run again (its hit buffer overflowed): the rerun writes the bins.  Every thread reads the same word: grid-uniform
  if (a.n_hits && *a.n_hits > a.hit_cap) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&a.stats[K11_SKIPPED], 1ull);
    return;
  }
  const uint32_t *parent = a.parent, *last = a.last, *taxid = a.taxid;
  if constexpr (LDS) {
    for (uint32_t i = threadIdx.x; i < a.n_nodes; i += blockDim.x) {
      lds[i] = a.parent[i];
      lds[a.n_nodes + i] = a.last[i];
      lds[2 * a.n_nodes + i] = a.taxid[i];
    }
    __syncthreads();
    parent = lds, last = lds + a.n_nodes, taxid = lds + 2 * a.n_nodes;
  }
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const BinTables c{a.node_of_column, a.n_cols, a.n_nodes};
  uint32_t n_none = 0, n_one = 0, n_several = 0, n_left = 0, n_bad = 0;  // the wave's counts over its rounds
  uint64_t steps = 0;                                                    // this lane's climb steps
  for (uint64_t r0 = ((uint64_t)blockIdx.x * 4 + wave) * RPW; r0 < a.n_reads; r0 += (uint64_t)gridDim.x * 4 * RPW) {  // wave-uniform
    const uint64_t mine = load_offsets(a.offs, r0, lane, a.n_reads);
    const OwnRead own = own_read(mine, r0, lane, a.n_reads, a.pair_cap);
    const uint64_t m = own.seg.m;
    const bool left = m > 0 && a.nk[own.r] > a.final_n;  // (m > 0: the read exists) — K4's HOST
    const bool judged = m > 0 && !left;
    const auto w = walk_as<NodeRange>(c, a.pairs, a.pair_cap, mine, lane, own, judged);
    const bool binned = judged && !w.v.none();
    if (own.lead) {
      uint32_t bin = left ? K11_LEFT : K11_NONE;
      if (binned) {
        // bin_lca: up from the min until the subtree reaches the max.  parent[v] < v for v > 0 and last[0] = n_nodes - 1 >= hi (the host
        // checks both), so the climb ends, at the latest at node 0
        uint32_t v = w.v.lo;
        while (last[v] < w.v.hi) v = parent[v], steps++;
        bin = taxid[v];
      }
      a.bins[own.r] = bin;
      if (a.left) a.left[own.r] = left ? 1 : 0;
    }
    n_none += wave_count(own.lead && !left && !binned);
    n_one += wave_count(own.lead && binned && w.v.lo == w.v.hi);
    n_several += wave_count(own.lead && binned && w.v.lo != w.v.hi);
    n_left += wave_count(own.lead && left);
    n_bad += wave_count(own.lead && own.seg.bad);
  }
  const uint64_t all_steps = wave_sum64(steps);
  wave_add(&a.stats[K11_NO_BIN], n_none, lane);
  wave_add(&a.stats[K11_ONE], n_one, lane);
  wave_add(&a.stats[K11_SEVERAL], n_several, lane);
  wave_add(&a.stats[K11_LEFT_READS], n_left, lane);
  wave_add(&a.stats[K11_BAD], n_bad, lane);
  if (lane == 0 && all_steps) atomicAdd(&a.stats[K11_STEPS], (unsigned long long)all_steps);
}

}  // namespace

// grid: as many workgroups as the reads fill, at most `max_wgs` (a test may pass fewer to force grid-stride rounds).  stats (K11_STATS
// words) must be zero on entry.  Returns the grid; *in_lds: whether the plan's tables went to LDS.
unsigned launch_k11(const K11Args& a, unsigned max_wgs, hipStream_t st, K4Log* log, bool* in_lds) {
  const bool fits = a.n_nodes <= K11_LDS_NODES;
  if (in_lds) *in_lds = fits;
  if (a.n_reads == 0) return 0;
  const unsigned grid = std::max(1u, std::min(walk_grid(a.n_reads), max_wgs));
  if (fits) hipLaunchKernelGGL(k11_bin<true>, dim3(grid), dim3(256), (size_t)a.n_nodes * 3 * sizeof(uint32_t), st, a);
  else hipLaunchKernelGGL(k11_bin<false>, dim3(grid), dim3(256), 0, st, a);
  k4_note(log, KMCPG_K11_BIN, grid, 256);
  return grid;
}

}  // namespace kmcpg
