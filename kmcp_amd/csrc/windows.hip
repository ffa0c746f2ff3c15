// windows.hip — sliding windows of long queries (kmcpg_submit_windows, `kmcp-search --sliding-step/--sliding-window`): the window
// descriptors of a batch, built on the device from the offsets of the reads' bases.  The bases of every read are uploaded once; a window is
// (first base in the staged text, its place in the batch's window numbering) and the k-mer kernels read its bases where they are
// (K1Args::src, k1_bases in k1_device.hpp) — never a copy of the window as text.
//
// Enumeration (seqkit sliding, restated in INTEGRATION.md): windows of a read of length L start at i = 0, S, 2S, ... and end at
// e = min(i + W, L); without greedy only windows with i + W <= L exist, with greedy every i < L does.  The host stages, per read, the
// bases the windows of this batch cover (a slice: a long read may be cut over several batches) and the two prefix sums below; window j
// of slice q starts j S bases into the slice and is full (W bases) up to the first one that would run over the slice's end.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "window_plan.hpp"

namespace kmcpg {

// one thread per window w of the batch: src[w] and offs[w] as window_desc_at (window_plan.hpp) states them, and the last thread writes
// offs[n_win] = vpre[n_slices].
__global__ void __launch_bounds__(256) k_window_desc(const uint64_t* __restrict__ soffs, const uint64_t* __restrict__ wpre,
                                                     const uint64_t* __restrict__ vpre, uint32_t n_slices, uint64_t n_win, uint64_t S,
                                                     uint64_t W, uint64_t* __restrict__ src, uint64_t* __restrict__ offs) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_win) return;
  uint64_t s, o;
  window_desc_at(soffs, wpre, vpre, n_slices, w, S, W, &s, &o);
  src[w] = s;
  offs[w] = o;
  if (w == n_win - 1) offs[n_win] = vpre[n_slices];
}

void launch_window_desc(const uint64_t* soffs, const uint64_t* wpre, const uint64_t* vpre, uint32_t n_slices, uint64_t n_win, uint64_t step,
                        uint64_t window, uint64_t* src, uint64_t* offs, hipStream_t st) {
  if (n_win == 0 || n_slices == 0) return;
  hipLaunchKernelGGL(k_window_desc, dim3((unsigned)((n_win + 255) / 256)), dim3(256), 0, st, soffs, wpre, vpre, n_slices, n_win, step, window, src,
                     offs);
}

}  // namespace kmcpg
