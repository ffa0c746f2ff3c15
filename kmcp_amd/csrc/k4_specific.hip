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
//   k4_verdict  the walk of seg_walk.hpp (one wave per 16 consecutive reads; a read's lane group reduces segments of up to 64 pairs, the
//               whole wave the longer ones) over min / max of both classes.  Writes the verdict byte and the kept length.
//   k3_scan_*   exclusive scan of the kept lengths (k3_finalize.hip)
//   k4_compact  the same split into lane groups and wave: the surviving segments are copied pair by pair (8 bytes per lane, coalesced)
//               to their new place.
// Counters (six words, wave-aggregated: one atomic per wave and word): reads kept / dropped / left to the host among the reads WITH
// pairs, segments reduced by a lane group / by the wave, segments that do not lie inside the pair buffer (treated as empty; must be 0).
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "kernels.hpp"
#include "seg_walk.hpp"

namespace kmcpg {

namespace {

__global__ void __launch_bounds__(256) k4_verdict(K4Args a) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t r0 = ((uint64_t)blockIdx.x * 4 + wave) * RPW;
  if (r0 >= a.n_reads) return;  // wave-uniform
  const uint64_t mine = load_offsets(a.offs, r0, lane, a.n_reads);
  const OwnRead own = own_read(mine, r0, lane, a.n_reads, a.pair_cap);
  const uint64_t m = own.seg.m;
  const bool host = m > 0 && a.nk[own.r] > a.final_n;
  const bool judged = m > 0 && !host;
  const auto w = walk<true>(ClassTables{a.target_class, a.species_class, a.n_cols}, a.pairs, a.pair_cap, mine, lane, own, judged);
  // the rule (specific_rule.hpp); a read without pairs is KEEP with nothing to keep
  const uint8_t verdict = host ? K4_HOST : !judged || w.v.one_target() || w.v.one_species() ? K4_KEEP : K4_DROP;
  if (own.lead) {
    a.verdict[own.r] = verdict;
    a.cnt[own.r] = verdict == K4_DROP ? 0u : (uint32_t)m;
  }
  if (r0 + RPW >= a.n_reads && lane == 0) a.cnt[a.n_reads] = 0;  // the scan runs over n_reads + 1 words
  wave_add(&a.stats[0], wave_count(own.lead && m > 0 && verdict == K4_KEEP), lane);
  wave_add(&a.stats[1], wave_count(own.lead && verdict == K4_DROP), lane);
  wave_add(&a.stats[2], wave_count(own.lead && host), lane);
  wave_add(&a.stats[3], wave_count(own.lead && w.small), lane);
  wave_add(&a.stats[4], wave_count(own.lead && judged && !w.small), lane);
  wave_add(&a.stats[5], wave_count(own.lead && own.seg.bad), lane);
}

__global__ void __launch_bounds__(256) k4_compact(K4Args a) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t r0 = ((uint64_t)blockIdx.x * 4 + wave) * RPW;
  if (r0 >= a.n_reads) return;  // wave-uniform
  // lanes 0..RPW: where the reads' segments are and where they go
  const uint64_t mine = load_offsets(a.offs, r0, lane, a.n_reads), to = load_offsets(a.out_offs, r0, lane, a.n_reads);
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
    const int q = pop_group(longs);
    const uint64_t t0 = __shfl(mine, q, 64), e0 = __shfl(to, q, 64), e1 = __shfl(to, q + 1, 64);
    for (uint64_t i = lane; i < e1 - e0; i += 64) a.out_pairs[e0 + i] = a.pairs[t0 + i];
  }
}

}  // namespace

// stats (K4_STATS words) must be zero on entry; cnt: n_reads + 1 words, sums: k3_scan_tiles_for(n_reads + 1) + 1 words
void launch_k4(const K4Args& a, hipStream_t st, K4Log* log) {
  if (a.n_reads == 0) return;
  hipLaunchKernelGGL(k4_verdict, dim3(walk_grid(a.n_reads)), dim3(256), 0, st, a);
  k4_note(log, KMCPG_K4_VERDICT, walk_grid(a.n_reads), 256);
  launch_k3_scan(a.cnt, a.out_offs, a.sums, a.n_reads + 1, st, log);
  launch_k4_compact(a, st, log);
}

void launch_k4_compact(const K4Args& a, hipStream_t st, K4Log* log, int kernel_id) {
  if (a.n_reads == 0) return;
  hipLaunchKernelGGL(k4_compact, dim3(walk_grid(a.n_reads)), dim3(256), 0, st, a);
  k4_note(log, kernel_id, walk_grid(a.n_reads), 256);
}

}  // namespace kmcpg
