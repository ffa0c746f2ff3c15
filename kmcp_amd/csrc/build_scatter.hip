// build_scatter.hip — the Bloom-column scatter of `kmcp index` (index.go:1107-1309) for k-mer lists that are already on the device:
// sigs[h_i % NumSigs][col] = 1 for every key of every list of a call, the lists going to any number of block matrices, in one launch.
//
// Work division: a wave takes one slice of BS_SLICE_KEYS consecutive keys of ONE list.  Wave w finds its list as the last one with
// sbase[list] <= w (a binary search in the prefix table of slices per list, as sort_segments.hip finds a wave's segment in wbase), so
// the descriptor — matrix, NumSigs, magic, row width, column — is wave-uniform and no search per key is left: a lane loads a key
// (64 consecutive keys per wave-instruction), reduces it num_hashes times and ORs one bit each.
//
// Why atomics: eight columns share a byte and lists of different columns of one block run in the same launch; a plain read-modify-write
// would lose bits.  OR is order-independent, so the matrix is the same whatever order the waves run in.  The OR is 32 bits wide on the
// aligned word that holds the byte; for the last byte of a matrix that word may reach up to 3 bytes past the end, which is why every
// matrix has 8 bytes of padding behind it (build_plan.hpp counts them).  All offsets are 64-bit: a GTDB block is 1.8 GB.
#include <hip/hip_runtime.h>

#include "build_scatter.hpp"
#include "fastmod.hpp"

namespace kmcpg {

__global__ void __launch_bounds__(256) k_build_scatter_lists(const ScatterDesc* __restrict__ descs, const uint32_t* __restrict__ sbase, uint32_t n_lists,
                                                             uint32_t n_slices, int num_hashes, const uint64_t* __restrict__ hashes) {
  const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (w >= n_slices) return;
  uint32_t lo = 0, hi = n_lists;  // the last list with sbase[list] <= w (every list of the table has at least one slice)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (sbase[mid] <= w) lo = mid; else hi = mid;
  }
  lo = __builtin_amdgcn_readfirstlane(lo);
  const ScatterDesc d = descs[lo];
  const uint64_t s0 = (uint64_t)(w - sbase[lo]) * BS_SLICE_KEYS;
  const uint64_t s1 = s0 + BS_SLICE_KEYS < d.n_keys ? s0 + BS_SLICE_KEYS : d.n_keys;
  const uint32_t bit = (uint32_t)(1u << (7 - (d.col & 7)));
  const uint64_t col_byte = d.col >> 3;
  for (uint64_t i = s0 + (threadIdx.x & 63); i < s1; i += 64) {
    const uint64_t h = hashes[d.first_key + i];
    const uint32_t ha = (uint32_t)(h >> 32), hb = (uint32_t)h;
    for (int t = 0; t < num_hashes; t++) {
      const uint64_t hv = num_hashes == 1 ? h : (uint64_t)(uint32_t)(ha + hb * (uint32_t)t);
      const uint64_t byte = fastmod_u64(hv, d.num_sigs, d.magic) * d.row_bytes + col_byte;
      uint32_t* const word = reinterpret_cast<uint32_t*>(d.base + (byte & ~3ULL));
      atomicOr(word, bit << (8 * (byte & 3)));
    }
  }
}

void launch_build_scatter_lists(const ScatterDesc* descs, const uint32_t* sbase, uint32_t n_lists, uint32_t n_slices, int num_hashes,
                                const uint64_t* hashes, hipStream_t st) {
  if (n_lists == 0 || n_slices == 0) return;
  hipLaunchKernelGGL(k_build_scatter_lists, dim3((n_slices + 3) / 4), dim3(256), 0, st, descs, sbase, n_lists, n_slices, num_hashes, hashes);
}

}  // namespace kmcpg
