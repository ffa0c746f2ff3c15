// build_scatter.hpp — the launcher of build_scatter.hip: every list of one kmcpg_builder_scatter_device call in ONE launch, whatever
// number of blocks the lists go to.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kmcpg {

// keys of one list a wave takes (16 per lane); kmcpg_builder_stats.slice_keys reports it
constexpr uint32_t BS_SLICE_KEYS = 1024;

// one list with keys: where its bits go.  The table is made on the host, so a wave that has found its list reads everything it needs of
// the block from one entry
struct ScatterDesc {
  uint8_t* base;       // the block's matrix in HBM (row-major, on-disk row width, 8 bytes of padding behind it)
  uint64_t num_sigs;   // rows
  uint64_t magic;      // fastmod_magic(num_sigs)
  uint64_t first_key;  // index of the list's first key in hashes[]
  uint64_t n_keys;
  uint32_t row_bytes;
  uint32_t col;        // column in the block
};
static_assert(sizeof(ScatterDesc) == 48, "five 8-byte words and two of 4");

// sbase[i] = slices of the lists before list i (n_lists + 1 entries; every list has ceil(n_keys / BS_SLICE_KEYS) >= 1 slices)
void launch_build_scatter_lists(const ScatterDesc* descs, const uint32_t* sbase, uint32_t n_lists, uint32_t n_slices, int num_hashes,
                                const uint64_t* hashes, hipStream_t st);

}  // namespace kmcpg
