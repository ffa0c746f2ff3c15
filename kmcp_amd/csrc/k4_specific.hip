// k4_specific.hip — K4: keep the reads whose matches point at one target or one species, ON THE DEVICE, behind K3.
//
// Reference counterpart: the per-query decision of `kmcp utils filter` (kmcp/cmd/filter.go:306-391).  K3 leaves the matches of a batch in
// HBM as (column, count) pairs grouped by read; whether a read is specific needs only those and two integers per column
// (specific_rule.hpp, which this file restates: target_class is shared exactly by the columns of one printed target, species_class is
// the species the target lies under, or 0):
//   KEEP  if min(target_class) == max(target_class) over the read's pairs
//   KEEP  if a species table is given and min(species_class) == max(species_class) != 0
//   DROP  otherwise
// A read without pairs is KEEP with nothing to keep; a read of more than final_n k-mers is HOST: its pairs may still fall to -f on the
// host (finalize.cpp), so it keeps them all and the host judges what is left.
//   k4_verdict  one wave per RPW = 16 consecutive reads (as k3_sort_wave): the offsets come with one coalesced load; segments of up to
//               64 pairs are reduced by the 4 lanes of their read's lane group (strided loads, two __shfl_xor steps), longer ones by the
//               whole wave one after the other (stride 64, six steps).  No LDS, no atomic per pair; the order inside a segment does not
//               matter, so the unordered segments above K3_WG_CAP need nothing special.  Writes the verdict byte and the kept length.
//   k3_scan_*   exclusive scan of the kept lengths (k3_finalize.hip)
//   k4_compact  the same walk: the surviving segments are copied pair by pair (8 bytes per lane, coalesced) to their new place.
// Counters (six words, wave-aggregated: one atomic per wave and word): reads kept / dropped / left to the host among the reads WITH
// pairs, segments reduced by a lane group / by the wave, segments that do not lie inside the pair buffer (treated as empty; must be 0).
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "kernels.hpp"

namespace kmcpg {

namespace {

constexpr int RPW = 16, LPR = 64 / RPW;  // reads per wave, lanes per read
constexpr uint32_t GROUP_CAP = 64;        // longest segment a lane group reduces

struct MinMax {
  uint32_t tmin, tmax, smin, smax;
};
__device__ __forceinline__ void take(MinMax& v, const K4Args& a, kmcpg_pair p) {
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
__device__ __forceinline__ uint8_t verdict_of(const MinMax& v, bool species) {
  if (v.tmin == v.tmax) return K4_KEEP;
  return species && v.smin == v.smax && v.smin != 0 ? K4_KEEP : K4_DROP;
}

// the segment of read r0 + q as the wave's lanes hold the offsets (lane i: offs[r0 + i], i <= RPW); outside the buffer = empty
__device__ __forceinline__ void segment(uint64_t mine, int q, uint64_t cap, uint64_t* s0, uint64_t* m, bool* bad) {
  const uint64_t a = __shfl(mine, q, 64), b = __shfl(mine, q + 1, 64);
  *bad = b < a || b > cap;
  *s0 = a;
  *m = *bad ? 0 : b - a;
}

__global__ void __launch_bounds__(256) k4_verdict(K4Args a) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t r0 = ((uint64_t)blockIdx.x * 4 + wave) * RPW;
  if (r0 >= a.n_reads) return;  // wave-uniform
  const uint64_t mine = a.offs[min(r0 + lane, (uint64_t)a.n_reads)];  // lanes 0..RPW hold offs[r0 + lane]
  const bool species = a.species_class != nullptr;
  // this lane's read: the one of its lane group
  const int g = (int)(lane / LPR), sub = (int)(lane % LPR);
  const uint64_t r = r0 + (uint64_t)g;
  const bool live = r < a.n_reads;
  uint64_t s0, m;
  bool bad;
  segment(mine, g, a.pair_cap, &s0, &m, &bad);  // (reads past the end: offs[n_reads] twice, m = 0)
  if (!live) m = 0, bad = false;
  const bool host = live && m > 0 && a.nk[r] > a.final_n;
  uint8_t verdict = host ? K4_HOST : K4_KEEP;
  const bool judged = live && m > 0 && !host;
  // segments of up to GROUP_CAP pairs: the lane group's strided loads, then two butterfly steps (every lane takes part in the shuffles:
  // the partners sub ^ 1, sub ^ 2 are lanes of the same group, and a group's lanes agree on `small`)
  const bool small = judged && m <= GROUP_CAP;
  MinMax v{0xffffffffu, 0u, 0xffffffffu, 0u};
  if (small)
    for (uint32_t i = (uint32_t)sub; i < (uint32_t)m; i += LPR) take(v, a, a.pairs[s0 + i]);
  fold(v, 1);
  fold(v, 2);
  if (small) verdict = verdict_of(v, species);
  // the long segments, one after the other, by the whole wave
  uint64_t longs = __ballot(judged && m > GROUP_CAP && sub == 0);
  const uint32_t n_long = (uint32_t)__popcll(longs);
  while (longs) {  // wave-uniform
    const int q = __ffsll((long long)longs) - 1;  // the lane that leads the group = LPR * read
    longs &= longs - 1;
    uint64_t t0, tm;
    bool tb;
    segment(mine, q / LPR, a.pair_cap, &t0, &tm, &tb);
    MinMax w{0xffffffffu, 0u, 0xffffffffu, 0u};
    for (uint64_t i = lane; i < tm; i += 64) take(w, a, a.pairs[t0 + i]);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) fold(w, d);
    if (g == q / LPR) verdict = verdict_of(w, species);
  }
  if (live && sub == 0) {
    a.verdict[r] = verdict;
    a.cnt[r] = verdict == K4_DROP ? 0u : (uint32_t)m;
  }
  if (r0 + RPW >= a.n_reads && lane == 0) a.cnt[a.n_reads] = 0;  // the scan runs over n_reads + 1 words
  const bool lead = live && sub == 0;
  const uint64_t kept = __ballot(lead && m > 0 && verdict == K4_KEEP), dropped = __ballot(lead && verdict == K4_DROP), hosts = __ballot(lead && host),
                 groups = __ballot(lead && small), bads = __ballot(lead && bad);
  if (lane == 0) {
    if (kept) atomicAdd(&a.stats[0], (uint32_t)__popcll(kept));
    if (dropped) atomicAdd(&a.stats[1], (uint32_t)__popcll(dropped));
    if (hosts) atomicAdd(&a.stats[2], (uint32_t)__popcll(hosts));
    if (groups) atomicAdd(&a.stats[3], (uint32_t)__popcll(groups));
    if (n_long) atomicAdd(&a.stats[4], n_long);
    if (bads) atomicAdd(&a.stats[5], (uint32_t)__popcll(bads));
  }
}

__global__ void __launch_bounds__(256) k4_compact(K4Args a) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t r0 = ((uint64_t)blockIdx.x * 4 + wave) * RPW;
  if (r0 >= a.n_reads) return;  // wave-uniform
  const uint64_t at = min(r0 + lane, (uint64_t)a.n_reads);
  const uint64_t mine = a.offs[at], to = a.out_offs[at];  // lanes 0..RPW: where the reads' segments are and where they go
  const int g = (int)(lane / LPR), sub = (int)(lane % LPR);
  // the kept length of this lane's read: the difference of the new offsets (0 for a dropped or empty read, and past the end)
  const uint64_t d0 = __shfl(to, g, 64), d1 = __shfl(to, g + 1, 64);
  const uint64_t s0 = __shfl(mine, g, 64);
  const uint64_t m = r0 + (uint64_t)g < a.n_reads ? d1 - d0 : 0;
  const bool fits = d1 <= a.out_cap;  // (the kept pairs are a subset of the input's: always, when out_cap >= pair_cap)
  if (m <= GROUP_CAP && fits)
    for (uint32_t i = (uint32_t)sub; i < (uint32_t)m; i += LPR) a.out_pairs[d0 + i] = a.pairs[s0 + i];
  uint64_t longs = __ballot(m > GROUP_CAP && fits && sub == 0);
  while (longs) {  // wave-uniform
    const int q = (__ffsll((long long)longs) - 1) / LPR;
    longs &= longs - 1;
    const uint64_t t0 = __shfl(mine, q, 64), e0 = __shfl(to, q, 64), e1 = __shfl(to, q + 1, 64);
    for (uint64_t i = lane; i < e1 - e0; i += 64) a.out_pairs[e0 + i] = a.pairs[t0 + i];
  }
}

}  // namespace

// stats (K4_STATS words) must be zero on entry; cnt: n_reads + 1 words, sums: k3_scan_tiles_for(n_reads + 1) + 1 words
void launch_k4(const K4Args& a, hipStream_t st, K4Log* log) {
  if (a.n_reads == 0) return;
  const unsigned grid = (unsigned)(((uint64_t)a.n_reads + 4 * RPW - 1) / (4 * RPW));
  hipLaunchKernelGGL(k4_verdict, dim3(grid), dim3(256), 0, st, a);
  k4_note(log, KMCPG_K4_VERDICT, grid, 256);
  launch_k3_scan(a.cnt, a.out_offs, a.sums, a.n_reads + 1, st, log);
  launch_k4_compact(a, st, log);
}

void launch_k4_compact(const K4Args& a, hipStream_t st, K4Log* log, int kernel_id) {
  if (a.n_reads == 0) return;
  const unsigned grid = (unsigned)(((uint64_t)a.n_reads + 4 * RPW - 1) / (4 * RPW));
  hipLaunchKernelGGL(k4_compact, dim3(grid), dim3(256), 0, st, a);
  k4_note(log, kernel_id, grid, 256);
}

}  // namespace kmcpg
