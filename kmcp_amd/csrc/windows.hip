// windows.hip — sliding windows of long queries (kmcpg_submit_windows, `kmcp-search --sliding-step/--sliding-window`): the window
// descriptors of a batch, built on the device from the offsets of the reads' bases.  The bases of every read are uploaded once; a window is
// (first base in the staged text, its place in the batch's window numbering) and the k-mer kernels read its bases where they are
// (K1Args::src, k1_kmers.hip) — never a copy of the window as text.
//
// Enumeration (seqkit sliding, restated in INTEGRATION.md): windows of a read of length L start at i = 0, S, 2S, ... and end at
// e = min(i + W, L); without greedy only windows with i + W <= L exist, with greedy every i < L does.  The host stages, per read, the
// bases the windows of this batch cover (a slice: a long read may be cut over several batches) and the two prefix sums below; window j
// of slice q starts j S bases into the slice and is full (W bases) up to the first one that would run over the slice's end.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace kmcpg {

// one thread per window w of the batch: its slice q (the last q with wpre[q] <= w), then
//   src[w]  = soffs[q] + j S                          (first base in the staged text)
//   offs[w] = vpre[q] + bases of windows 0 .. j-1 of the slice   (the window numbering the rest of the pipeline sees)
// and the last thread writes offs[n_win] = vpre[n_slices].
__global__ void __launch_bounds__(256) k_window_desc(const uint64_t* __restrict__ soffs, const uint64_t* __restrict__ wpre,
                                                     const uint64_t* __restrict__ vpre, uint32_t n_slices, uint64_t n_win, uint64_t S,
                                                     uint64_t W, uint64_t* __restrict__ src, uint64_t* __restrict__ offs) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_win) return;
  uint32_t lo = 0, hi = n_slices;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (wpre[mid] <= w) lo = mid;
    else hi = mid;
  }
  const uint32_t q = lo;
  const uint64_t j = w - wpre[q];
  const uint64_t ls = soffs[q + 1] - soffs[q];
  const uint64_t full = ls >= W ? (ls - W) / S + 1 : 0;  // windows of the slice that hold W bases
  uint64_t v;
  if (j <= full) v = j * W;
  else  // full windows, then the truncated ones (greedy): sum over t in [full, j) of ls - t S
    v = full * W + (j - full) * ls - S * ((j * (j - 1)) / 2 - (full * (full - (full > 0 ? 1 : 0))) / 2);
  src[w] = soffs[q] + j * S;
  offs[w] = vpre[q] + v;
  if (w == n_win - 1) offs[n_win] = vpre[n_slices];
}

void launch_window_desc(const uint64_t* soffs, const uint64_t* wpre, const uint64_t* vpre, uint32_t n_slices, uint64_t n_win, uint64_t step,
                        uint64_t window, uint64_t* src, uint64_t* offs, hipStream_t st) {
  if (n_win == 0 || n_slices == 0) return;
  hipLaunchKernelGGL(k_window_desc, dim3((unsigned)((n_win + 255) / 256)), dim3(256), 0, st, soffs, wpre, vpre, n_slices, n_win, step, window, src,
                     offs);
}

}  // namespace kmcpg
