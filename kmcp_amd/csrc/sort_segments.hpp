// sort_segments.hpp — launcher of the segmented sort + unique in sort_segments.hip (the chunk lists of a batch of genomes, sketch.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/kmcp_gpu.h"

namespace kmcpg {

constexpr uint32_t SEGSORT_KEYS_PER_WAVE = 4096;  // a wave owns up to this many consecutive keys of one segment

// the raw lists: segment s is the concatenation over parts p (one per k-mer size) of keys[p * part_stride + in_off[s] .. + cnt[p * cnt_stride + s])
struct SegSortIn {
  const uint64_t* keys;
  const uint64_t* in_off;  // [n_segs]
  const int32_t* cnt;      // [parts][cnt_stride]
  uint64_t part_stride;
  uint32_t cnt_stride;
  int32_t parts;           // 1 .. 8
  uint32_t n_segs;
};

// upper bound of the waves of a batch whose segment s holds at most ub[s] keys: sum of ceil(ub[s] / SEGSORT_KEYS_PER_WAVE)
inline uint32_t seg_sort_waves_for(uint64_t ub) { return (uint32_t)((ub + SEGSORT_KEYS_PER_WAVE - 1) / SEGSORT_KEYS_PER_WAVE); }
size_t seg_sort_temp_words(uint32_t n_segs, uint32_t max_waves);
int seg_sort_passes(int key_bits);
// Sorts every segment ascending, drops duplicates, compacts: *out (a or b, each with room for all raw keys; in.keys may be a) holds
// segment s at [koff[s], koff[s + 1]); koff has n_segs + 2 words, the last one receives the number of raw keys.  key_bits: no key
// has a bit set at or above it.  All raw keys of a call together must number less than 2^32.  Enqueues only; <0 on bad arguments.
int seg_sort_unique(const SegSortIn& in, uint64_t* a, uint64_t* b, uint32_t max_waves, int key_bits, uint32_t* temp, size_t temp_words, uint64_t* koff,
                    uint64_t** out, kmcpg_sketch_launch* rec, hipStream_t st);

}  // namespace kmcpg
