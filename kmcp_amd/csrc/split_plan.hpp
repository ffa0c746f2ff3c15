// split_plan.hpp — the chunks of one joined reference sequence as `kmcp compute --split-number` cuts them (kmcp/cmd/compute.go:675-744).
// Host-only arithmetic in plain C++17 (tests/split_check.cpp compiles it with g++); sketch.cpp answers kmcpg_split_bounds from it and cuts
// every genome of a kmcpg_sketch_genomes batch with it.
//
//   a sequence shorter than split_min_ref, or split_number <= 1:  one window [0, len)                                  (:677-681, :696-700)
//   otherwise  size = (len + (n - 1) overlap + n - 1) / n,  step = size - overlap                                      (:690-692)
//              windows start at 0, step, 2 step, ... while the start is inside the sequence, each cut at the sequence's end (the slider is
//              greedy), at most n of them: an (n + 1)-th would start at n step >= len - overlap and be dropped by the rule below
//   a window with len - 1 <= overlap or len < k_min is dropped (:713, :742); the surviving count is the genome's `chunks`, and the
//   survivors are numbered 0, 1, ... in order (slidIdx, :733-745).
#pragma once
#include <stdint.h>

namespace kmcpg {

struct SplitSpec {
  uint64_t n = 1;        // -n/--split-number
  uint64_t overlap = 0;  // -l/--split-overlap
  uint64_t min_ref = 0;  // -m/--split-min-ref
  uint64_t k_min = 1;    // smallest k of the sketch
};

// writes the first min(count, cap) surviving windows to first[] / end[] (either may be null when cap is 0); returns the count
inline uint64_t split_bounds(uint64_t len, const SplitSpec& sp, uint64_t* first, uint64_t* end, uint64_t cap) {
  uint64_t size = len, step = len, max_windows = 1;
  if (sp.n > 1 && len >= sp.min_ref) {
    size = (len + (sp.n - 1) * sp.overlap + sp.n - 1) / sp.n;
    if (size <= sp.overlap) return 0;  // no window can be longer than the overlap: all dropped
    step = size - sp.overlap;
    max_windows = sp.n;
  }
  uint64_t kept = 0;
  uint64_t i = 0;
  for (uint64_t w = 0; w < max_windows && (w == 0 || i < len); w++, i += step) {
    const uint64_t e = len - i < size ? len : i + size;
    const uint64_t wl = e - i;
    if (wl <= sp.overlap + 1 || wl < sp.k_min) continue;  // len - 1 <= overlap, len < kMin
    if (kept < cap) {
      first[kept] = i;
      end[kept] = e;
    }
    kept++;
    if (step == 0) break;
  }
  return kept;
}

}  // namespace kmcpg
