// k1_win_once.hip — K1, sliding windows of plain / FracMinHash k-mers: every staged base hashed once, every window's list cut from its
// slice's kept hashes (k1_win_hash, k1_win_scan, k1_win_rank, k1_win_gather; form WinOnce of launch_k1, k1_kmers.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "device_utils.hpp"
#include "k1_device.hpp"
#include "k1_launch.hpp"
#include "k1_plan.hpp"
#include "kernels.hpp"
#include "nthash.hpp"

namespace kmcpg {

// ---- sliding windows of plain / FracMinHash k-mers, hash-once form (host_windows.cpp kmcpg_submit_windows; launch_k1, form WinOnce) ----------------------
// A k-mer's hash and whether it is kept do not depend on the window it is read in, so the staged slices of reads are hashed once — one wave per
// K1_WIN_CHUNK positions of a slice, the wave form of the short-read kernel (hash_mate_scan) over the chunk's bases — and every window's list is
// the run of its slice's kept hashes between the ranks of its first and one-past-last k-mer position.  Positions are numbered by the slice's
// first base in the staged text (soffs[q] + p, p < npos_q = ls_q - k + 1), so h[] / rank[] need one entry per staged base.
__device__ __forceinline__ uint32_t win_slice_of(const uint64_t* __restrict__ pre, uint32_t n, uint64_t x) {  // the last q with pre[q] <= x
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (pre[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// pass 1: hashes of a chunk's positions -> h[], how many of them are kept -> cnt[chunk]
__global__ void __launch_bounds__(256) k1_win_hash(const K1Args a, const WindowSrc w, uint64_t* __restrict__ h, uint32_t* __restrict__ cnt) {
  __shared__ uint64_t tab[256];
  tab[threadIdx.x] = seed_of(threadIdx.x);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int k = a.k;
  const bool scaled = a.scaled != 0;
  for (uint64_t c = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < w.n_chunks; c += (uint64_t)gridDim.x * 4) {
    const uint32_t q = win_slice_of(w.cpre, w.ns, c);
    const uint64_t g0 = w.soffs[q], ls = w.soffs[q + 1] - g0;
    const uint64_t p0 = (c - w.cpre[q]) * K1_WIN_CHUNK;
    const int pn = (int)min((uint64_t)K1_WIN_CHUNK, ls - (uint64_t)k + 1 - p0);  // (a slice with chunks holds >= k bases)
    const uint8_t* __restrict__ s = a.seqs + g0 + p0;
    const int len = pn + k - 1;
    uint64_t* __restrict__ out = h + g0 + p0;
    uint64_t cp = 0, cq = 0;
    int kept = 0;
    WTile cur = wave_tile(s, len, 0, tab, cp, cq, lane);
    for (int base = 0; base < pn; base += 64) {
      const WTile nxt = wave_tile(s, len, base + 64, tab, cp, cq, lane);
      const uint64_t hv = wave_hash(cur, nxt, k, lane);
      const bool v = base + lane < pn;
      if (v) out[base + lane] = hv;
      kept += __popcll(__ballot(v && hv != 0 && (!scaled || hv <= a.max_hash)));  // :1097-1103, as hash_mate_scan
      cur = nxt;
    }
    if (lane == 0) cnt[c] = (uint32_t)kept;
  }
}

// the chunks' kept counts -> exclusive prefix cbase[0 .. n] (one workgroup; a batch has at most 2^16 chunks at the default piece size)
__global__ void __launch_bounds__(1024) k1_win_scan(const uint32_t* __restrict__ cnt, uint64_t n, uint64_t* __restrict__ cbase) {
  __shared__ uint64_t sm[1024];
  const uint32_t t = threadIdx.x;
  const uint64_t per = (n + 1023) / 1024, lo = min(n, (uint64_t)t * per), hi = min(n, lo + per);
  uint64_t sum = 0;
  for (uint64_t i = lo; i < hi; i++) sum += cnt[i];
  sm[t] = sum;
  __syncthreads();
  for (uint32_t off = 1; off < 1024; off <<= 1) {
    const uint64_t v = t >= off ? sm[t - off] : 0;
    __syncthreads();
    sm[t] += v;
    __syncthreads();
  }
  uint64_t run = sm[t] - sum;
  for (uint64_t i = lo; i < hi; i++) {
    cbase[i] = run;
    run += cnt[i];
  }
  if (t == 1023) cbase[n] = sm[1023];
}

// pass 2: the kept hashes of a chunk in order -> kept[cbase[chunk] ...], every position's rank (kept positions before it) -> rank[]
__global__ void __launch_bounds__(256) k1_win_rank(const K1Args a, const WindowSrc w, const uint64_t* __restrict__ h, const uint64_t* __restrict__ cbase,
                                                   uint64_t* __restrict__ kept, uint32_t* __restrict__ rank) {
  const int lane = threadIdx.x & 63;
  const int k = a.k;
  const bool scaled = a.scaled != 0;
  for (uint64_t c = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < w.n_chunks; c += (uint64_t)gridDim.x * 4) {
    const uint32_t q = win_slice_of(w.cpre, w.ns, c);
    const uint64_t g0 = w.soffs[q], ls = w.soffs[q + 1] - g0;
    const uint64_t p0 = (c - w.cpre[q]) * K1_WIN_CHUNK;
    const int pn = (int)min((uint64_t)K1_WIN_CHUNK, ls - (uint64_t)k + 1 - p0);
    uint64_t r = cbase[c];
    for (int base = 0; base < pn; base += 64) {
      const bool v = base + lane < pn;
      const uint64_t hv = v ? h[g0 + p0 + base + lane] : 0;
      const bool keep = v && hv != 0 && (!scaled || hv <= a.max_hash);
      const uint64_t m = __ballot(keep);
      const uint64_t mine = r + __popcll(m & ((1ULL << lane) - 1ULL));
      if (v) rank[g0 + p0 + base + lane] = (uint32_t)mine;
      if (keep) kept[mine] = hv;
      r += __popcll(m);
    }
  }
}

// pass 3: one wave per window: qlen, and the run of kept hashes between its first and one-past-last k-mer position (nk_raw = nk1 = its
// length; a window shorter than -m has none, handleQuery :778-786)
__global__ void __launch_bounds__(256) k1_win_gather(const K1Args a, const WindowSrc w, const uint64_t* __restrict__ kept, const uint32_t* __restrict__ rank,
                                                     const uint64_t* __restrict__ cbase) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6); r < a.n_reads; r += gridDim.x * 4) {
    const uint32_t q = win_slice_of(w.wpre, w.ns, r);
    const uint64_t g0 = w.soffs[q], ls = w.soffs[q + 1] - g0;
    const uint64_t i = (r - w.wpre[q]) * w.step, e = min(i + w.window, ls);
    const int len = (int)(e - i);
    const int np = len - a.k + 1;
    uint64_t lo = 0, n = 0;
    if (len >= a.min_qlen && np > 0) {
      const uint64_t npos = ls - (uint64_t)a.k + 1;
      lo = rank[g0 + i];
      const uint64_t hi = i + (uint64_t)np == npos ? cbase[w.cpre[q + 1]] : rank[g0 + i + (uint64_t)np];
      n = hi - lo;
    }
    uint64_t* __restrict__ out = a.hashes + a.offs[r];
    for (uint64_t t = lane; t < n; t += 64) out[t] = kept[lo + t];
    if (lane == 0) {
      a.nk_raw[r] = (int32_t)n;
      a.nk1[r] = (int32_t)n;
      a.qlen[r] = len;
    }
  }
}

void launch_k1_win_once(const K1Args& a, const K1Plan& p, const K1WinOnce& wo, hipStream_t st, K1Log* log) {
  if (p.grid) {
    hipLaunchKernelGGL(k1_win_hash, dim3(p.grid), dim3(256), 0, st, a, wo.w, wo.h, wo.cnt);
    k1_note(log, KMCPG_K1_WIN_HASH, 0, 0, p.grid, 256, 0);
    hipLaunchKernelGGL(k1_win_scan, dim3(1), dim3(1024), 0, st, wo.cnt, wo.w.n_chunks, wo.cbase);
    k1_note(log, KMCPG_K1_WIN_SCAN, 0, 0, 1, 1024, 0);
    hipLaunchKernelGGL(k1_win_rank, dim3(p.grid), dim3(256), 0, st, a, wo.w, wo.h, wo.cbase, wo.kept, wo.rank);
    k1_note(log, KMCPG_K1_WIN_RANK, 0, 0, p.grid, 256, 0);
  } else {
    (void)hipMemsetAsync(wo.cbase, 0, sizeof(uint64_t), st);
  }
  hipLaunchKernelGGL(k1_win_gather, dim3(p.grid2), dim3(256), 0, st, a, wo.w, wo.kept, wo.rank, wo.cbase);
  k1_note(log, KMCPG_K1_WIN_GATHER, 0, 0, p.grid2, 256, 0);
}


}  // namespace kmcpg
