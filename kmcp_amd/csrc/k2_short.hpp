// k2_short.hpp — the short-read unit of the COBS kernel, stated once: what one wave does with one (read, slot) unit on a 1-KiB tile when
// the read is short enough for ALL its row indices to fit LDS.  Two kernels drive it (k2_cobs.hip): k2_cobs<64, 8|10, false, false, 4>
// with K2F_ bits set — one unit per launched wave (k2_cobs_body.inc, the SHORT branch) — and k2_cobs_persist, whose resident waves
// take their units from a queue.  Both do, in this order: k2_short_index; per tile the cursor loop (k2_short_tile.inc, text included at both sites) and k2_emit_tile; k2_short_account.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"
#include "csa.hpp"
#include "device_utils.hpp"

namespace kmcpg {

// the reads the path takes: the host picks NPL with n + 1 < 2^NPL (k2_plan.hpp), and this many row indices fit a wave's LDS row
template <int NPL>
constexpr int K2_SHORT_NMAX = NPL == 8 ? 256 : 1024;
// a wave's row of indices (+ 4: a group's four index reads stay inside for every cursor <= n)
template <int NPL>
constexpr int K2_SHORT_ROW = K2_SHORT_NMAX<NPL> + 4;

// what is the same in every lane, told to the compiler
__device__ __forceinline__ uint32_t k2_uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t k2_uni64(uint64_t v) { return (uint64_t)k2_uni((uint32_t)v) | ((uint64_t)k2_uni((uint32_t)(v >> 32)) << 32); }

// ---- Index phase: the row indices of read r's n hashes in a block of `ns` signatures (fastmod constant mh, row pitch s16 in 16-byte
//      units) -> s_row[0 .. n).  Four hash loads per lane in flight, then the arithmetic.  r and n are wave-uniform.
__device__ __forceinline__ void k2_short_index(const K2Args& a, uint32_t r, uint64_t ns, uint64_t mh, uint32_t s16, int n, uint32_t* s_row, int lane) {
  const uint64_t koff = a.offs[r] + (a.offs2 ? a.offs2[r] : 0);
  for (int c0 = 0; c0 < n; c0 += 256) {
    uint64_t hv[4];
#pragma unroll
    for (int it = 0; it < 4; it++) hv[it] = c0 + 64 * it + lane < n ? a.hashes[koff + (uint64_t)(c0 + 64 * it + lane)] : 0;
#pragma unroll
    for (int it = 0; it < 4; it++)
      if (c0 + 64 * it + lane < n) s_row[c0 + 64 * it + lane] = (uint32_t)fastmod_u64(hv[it], ns, mh) * s16;
  }
  wave_lds_fence();
}

// ---- Threshold of a read of n k-mers: the integer threshold (:7468-7470: count >= minMatched && float64(count) > nHashes*queryCov) and
//      the -f bound (counts below it fail the host's FPR(n, count) <= max_fpr test, :7474-7478; fpr_bound in query.cpp) ...
__device__ __forceinline__ uint32_t k2_short_cmin(const K2Args& a, int n) {
  uint32_t cmin = count_threshold(n, a.min_qcov, a.min_matched);
  if (a.cmin_fpr && n <= a.cmin_fpr_n) cmin = max(cmin, (uint32_t)a.cmin_fpr[n]);
  return cmin;
}
// ... and as the planes see it (past their range nothing passes, whatever the value); wave-uniform
template <int NPL>
__device__ __forceinline__ int k2_short_clamp(uint32_t cmin) {
  return (int)k2_uni(min(cmin, 1u << NPL));
}

// ---- Hit emission of one tile (the body's own epilogue stays where it is: the other forms keep their token stream).  Wave-aggregated as
//      there: bit-sliced compare with cmin, ONE atomic on the global counter for the wave's hits, the tuples side by side; the segment of
//      the previous hit stays in registers.  boff: the lane's first byte in the row.
template <int NPL>
__device__ __forceinline__ void k2_emit_tile(const K2Args& a, const BlockDev* __restrict__ bd, uint32_t r, uint32_t boff, uint32_t cmin, bool live,
                                             const uint32_t (&pl)[4][NPL], int lane) {
  const bool emit = live && (cmin >> NPL) == 0;  // else: nothing left alive (cmin always fits the planes: query.cpp)
  uint32_t ge[4];
  uint32_t mine = 0;
#pragma unroll
  for (int d = 0; d < 4; d++) {
    uint32_t v = emit ? 0xffffffffu : 0u;  // bit-sliced (count >= cmin), LSB to MSB
#pragma unroll
    for (int p = 0; p < NPL; p++) v = ((cmin >> p) & 1u) ? (v & pl[d][p]) : (v | pl[d][p]);
    ge[d] = v;
    mine += (uint32_t)__popc(v);
  }
  if (__ballot(mine != 0) == 0) return;  // wave-uniform: the common case
  uint32_t incl = mine;  // inclusive prefix sum over the wave
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(incl, off);
    if (lane >= off) incl += t;
  }
  const uint32_t total = __shfl(incl, 63);
  unsigned long long base_idx = 0;
  if (lane == 63) base_idx = atomicAdd(a.counter, (unsigned long long)total);
  base_idx = __shfl(base_idx, 63);
  unsigned long long idx = base_idx + (incl - mine);
  uint32_t sg_lo = 1, sg_hi = 0, sg_col = 0;  // the segment of the previous hit: bytes [sg_lo, sg_hi), column of its first bit
  const Seg* __restrict__ segs = a.segs + bd->seg0;
  const uint32_t nsegs = bd->nsegs;
#pragma unroll
  for (int d = 0; d < 4; d++) {
    uint32_t w = ge[d];
    while (w) {
      const int q = __ffs(w) - 1;
      w &= w - 1;
      uint32_t count = 0;
#pragma unroll
      for (int p = 0; p < NPL; p++) count |= ((pl[d][p] >> q) & 1u) << p;
      const uint32_t byte = boff + (uint32_t)d * 4u + (uint32_t)(q >> 3);  // bit 7 = first column of the byte (index.go:1157)
      if (byte < sg_lo || byte >= sg_hi) {
        for (uint32_t i = 0; i < nsegs; i++) {
          const Seg sg = segs[i];
          if (byte < sg.byte_end) {
            sg_lo = sg.byte_start;
            sg_hi = sg.byte_end;
            sg_col = sg.col_base;
            break;
          }
        }
      }
      if (idx < a.hit_cap) {
        kmcpg_hit hit;
        hit.read = r;
        hit.col = sg_col + (byte - sg_lo) * 8u + (7u - (uint32_t)(q & 7));
        hit.count = count;
        if (byte < sg_lo || byte >= sg_hi) hit = kmcpg_hit{0xffffffffu, 0xffffffffu, 0u};  // a tombstone, as in the body
        a.hits[idx] = hit;
      }
      idx++;
    }
  }
}

// ---- Accounting (profiling level 2): what this wave asked the memory system for — its lanes' row loads and `hashes`, every hash of a
//      read once per unit — as one atomic pair per wave, on the counters of workgroup `bid` (as at the end of the body)
__device__ __forceinline__ void k2_short_account(const K2Args& a, unsigned bid, uint32_t g_rows, uint64_t hashes, int lane) {
  if (!a.gathered) return;
  unsigned long long rows = g_rows;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) rows += __shfl_xor(rows, off);
  if (lane == 0) {
    atomicAdd(a.gathered + (size_t)(bid % K2_GATHER_SLOTS) * 16, rows);
    atomicAdd(a.gathered + (size_t)(bid % K2_GATHER_SLOTS) * 16 + 1, (unsigned long long)hashes);
  }
}

}  // namespace kmcpg
