// lane_plan.hpp — how large a lane's hit buffers are and how the handle learns what to expect (lane.cpp enqueue / collect).  Pure integer
// code, no HIP: tests/lane_plan_check.cpp compiles it alone.  The policy decides whether a batch runs twice, so it is stated once here.
//
// ~1 hit per read is typical for distinct references, dozens to hundreds for a database full of close relatives: the buffers follow what
// the last large batches produced (hits_hint = hits per 1024 reads).  Too small a device buffer costs a rerun of the batch (collect), too
// short an eager copy a late one on the copy stream, so the device buffer is generous (up to 512 hits = 6 KB per read, and never smaller
// than it already is) while the eager copy stays within 32 hits per read: a burst of hit-heavy queries must not make every later batch
// drag gigabytes over PCIe.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace kmcpg {

struct HitPlan {
  uint64_t base_cap;  // the plain size: what the lane falls back to when the generous one does not fit beside the index
  uint64_t want;      // what this batch should have: the recent hit rate + 50 %, within the lane's share of the handle's hit-buffer budget
  bool release;       // the lane's buffer is a leftover of a burst: give it back first
  uint64_t first;     // entries of the eager copy, given a device buffer of max(what the lane keeps, want) entries
};

// n reads, hits_hint hits per 1024 reads lately, lane_hit_budget entries a lane may grow to beyond the plain size, cap = the lane's device
// hit buffer now.  generous_eager: a piece of a large kmcpg_search_batch call — its neighbours have just shown how many matches to expect,
// so the eager copy may take all of them (1024 per read instead of 32).
inline HitPlan plan_hit_buffers(uint32_t n, uint64_t hits_hint, uint64_t lane_hit_budget, uint64_t cap, bool generous_eager) {
  HitPlan h;
  const uint64_t expect = std::min<uint64_t>(hits_hint * (uint64_t)n / 1024, (uint64_t)n * 512);
  h.base_cap = (uint64_t)n * 8 + 1024;
  h.want = std::max<uint64_t>(h.base_cap, std::min<uint64_t>(expect + expect / 2, std::max<uint64_t>(h.base_cap, lane_hit_budget)));
  // a buffer left over from a burst of hit-heavy batches goes back once the data has calmed down (hits_hint decays by 1/8 per batch): HBM
  // pinned for the life of the handle is HBM the workspace of a later, larger batch may need.  (16x, not 4x: a lane that serves whole batches
  // and quarter-batch pieces in turn must not free and reallocate its buffer every time — hipFree waits for the device)
  h.release = cap > 16 * h.want && cap > (1u << 20);
  const uint64_t have = std::max<uint64_t>(h.release ? 0 : cap, h.want);
  h.first = std::min<uint64_t>(have, std::max<uint64_t>((uint64_t)n * 2 + 1024, std::min<uint64_t>(expect + expect / 4, (uint64_t)n * (generous_eager ? 1024 : 32))));
  return h;
}

// hits_hint after a batch of n reads (n >= 1024: large enough to say something about the data) that produced cnt hits: rises at once,
// decays slowly
inline uint64_t hits_hint_after(uint64_t old, uint64_t cnt, uint32_t n) {
  const uint64_t per_k = cnt * 1024 / n + 1;
  return per_k > old ? per_k : old - old / 8 + per_k / 8;
}

}  // namespace kmcpg
