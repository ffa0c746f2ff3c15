// lane_plan_check.cpp — kmcp_amd/csrc/lane_plan.hpp compiled alone (g++, no HIP) behind two C entries for tests/test_lane_plan_cpu.py
#include <stdint.h>

#include "../kmcp_amd/csrc/lane_plan.hpp"

// out = {base_cap, want, release, first}
extern "C" void lp_plan(uint32_t n, uint64_t hits_hint, uint64_t lane_hit_budget, uint64_t cap, int generous_eager, uint64_t* out) {
  const kmcpg::HitPlan h = kmcpg::plan_hit_buffers(n, hits_hint, lane_hit_budget, cap, generous_eager != 0);
  out[0] = h.base_cap;
  out[1] = h.want;
  out[2] = h.release ? 1 : 0;
  out[3] = h.first;
}

extern "C" uint64_t lp_hint(uint64_t old, uint64_t cnt, uint32_t n) { return kmcpg::hits_hint_after(old, cnt, n); }
