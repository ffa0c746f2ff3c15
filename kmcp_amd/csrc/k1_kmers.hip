// k1_kmers.hip — K1: ntHash canonical k-mer hashes of batched reads, FracMinHash filter, Closed-Syncmer and Minimizer selection.
// Replaces bio/sketches NextHash / NextSyncmer / NextMinimizer behind generateKmers (kmcp/cmd/util-db-search.go:1037-1107).  This file is
// the entry: launch_k1, a switch over the plan's form.  The kernels live in one file per family, each with its launchers (k1_launch.hpp):
//   k1_reads.hip     one wave per short read (k1_kmers), one 1024-thread workgroup per long read (k1_kmers_wg, k1_kmers_wg_global) or per
//                    segment of a genome on the same LDS tiles (k1_seg_hash)
//   k1_windows.hip   window sketches of long reads, a wave per segment of a read (k1_windows_wave) or rolling lanes (k1_windows_roll)
//   k1_seg.hip       whole genomes: one workgroup per 65536-position segment, rolling (k1_seg_roll / k1_seg_roll2), and the pack (k1_seg_pack)
//   k1_win_once.hip  sliding windows of plain k-mers, every staged base hashed once (k1_win_hash / scan / rank / gather)
// and the wave machinery they share is in k1_device.hpp, the hash arithmetic in nthash.hpp.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "k1_launch.hpp"
#include "k1_plan.hpp"
#include "kernels.hpp"

namespace kmcpg {

static_assert(K1_WAVE_SORT_CAP == DEDUP_WAVE_CAP, "k1_plan.hpp restates kernels.hpp");

// NumKmers when no read of the batch can exceed the dedup threshold.
__global__ void k_nk_simple(const int32_t* nk_raw, int32_t* nk_search, uint32_t n, int32_t min_matched) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    int v = nk_raw[i];
    nk_search[i] = v >= min_matched ? v : 0;  // :854-869: too few k-mers => not searched
  }
}

void k1_note(K1Log* log, int kernel, int p0, int p1, unsigned grid, unsigned block, size_t lds) {
  if (!log) return;
  kmcpg_k1_launch r{};
  r.kernel = kernel;
  r.p0 = p0;
  r.p1 = p1;
  r.grid = grid;
  r.block = block;
  r.lds_bytes = (uint32_t)lds;
  r.left_on_list = UINT32_MAX;
  log->push_back(r);
}

// the kernels of the plan's form, in order (k1_plan.hpp; the table: DESIGN.md §4).  Everything was decided there: `a` is complete, side
// buffer pointers included, and nothing here looks at the batch again.
void launch_k1(const K1Args& a, const K1Plan& p, const K1WinOnce& wo, hipStream_t st, K1Log* log) {
  switch (p.form) {
    case K1Form::None: break;
    case K1Form::WinOnce: launch_k1_win_once(a, p, wo, st, log); break;     // sliding windows, each staged base hashed once
    case K1Form::SegRoll2: launch_k1_seg_roll2(a, p, st, log); break;       // whole genomes: one workgroup per 65536-position segment, then an ordered pack
    case K1Form::SegRoll: launch_k1_seg_roll(a, p, st, log); break;
    case K1Form::SegHash:
      launch_k1_seg_hash(a, p, st, log);
      launch_k1_seg_pack(a, p, st, log);
      break;
    case K1Form::WindowsRoll: launch_k1_windows_roll(a, p, st, log); break;  // closed syncmers of long reads: the rolling kernel, k1_windows_wave behind it for the reads on its list
    case K1Form::WindowsWave: launch_k1_windows_wave(a, p, st, log); break;  // window sketches of long reads, a wave per read
    case K1Form::WgGlobal: launch_k1_wg_global(a, p, st, log); break;
    case K1Form::Wg: launch_k1_wg(a, p, st, log); break;        // long queries: a whole workgroup per read
    case K1Form::Short: launch_k1_short(a, p, st, log); break;  // four reads per workgroup, a wave each
  }
}

void launch_nk_simple(const int32_t* nk_raw, int32_t* nk_search, uint32_t n, int32_t min_matched, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_nk_simple, dim3((n + 255) / 256), dim3(256), 0, st, nk_raw, nk_search, n, min_matched);
}

}  // namespace kmcpg
