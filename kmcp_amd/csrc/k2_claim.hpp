// k2_claim.hpp — the unit queue of the persistent short-read COBS kernel (k2_cobs.hip k2_cobs_persist), its arithmetic stated once.
// A launch piece owns `units` consecutive work units from `unit_base` on and one 64-bit counter, zero before the launch.  A wave that
// needs work adds K2_CLAIM_RUN to the counter; the value it gets back — its ticket — names the run of units it now owns.  Tickets
// ascend, so the waves in flight stay within one (block, tile) slice of the index as they do under the hardware dispatcher, and a
// wave whose run comes out empty knows that every later one is empty too: it stops asking.  Plain C++ for host and device
// (tests/k2_claim_check.cpp compiles it with g++).
#pragma once
#include <stdint.h>

#include "k2_plan.hpp"

#if defined(__HIPCC__)
#define K2_CLAIM_HD __host__ __device__ inline
#else
#define K2_CLAIM_HD inline
#endif

namespace kmcpg {

// Units per claim.  A claim is one atomic on one address, ~16 ns each under load.  At GTDB scale (33.5 M units of ~58 us on 4 096
// waves: one unit every 14 ns chip-wide) a run of 1 is bound by the counter (532 against 457 ms per launch), runs of 2 to 16 are within
// 0.6 % of each other and 64 loses 2 % (profiles/k2_persist_ab.txt).  8: one claim every 113 ns, 4.2 M per launch, an eighth of what
// the counter can take, which leaves room for batches of shorter units; a run is ~0.5 ms of a wave's life, so the launch's ragged end
// stays short.
constexpr uint32_t K2_CLAIM_RUN = 8;

struct K2Run {
  uint64_t first, last;  // units [first, last) of the batch; first == last: the queue is dry
};

// the run a ticket stands for: `ticket` is what the counter held before this claim's `run` was added
K2_CLAIM_HD K2Run k2_claim_run(uint64_t ticket, uint64_t unit_base, uint64_t units, uint32_t run) {
  const uint64_t lo = ticket < units ? ticket : units;
  const uint64_t hi = units - lo < run ? units : lo + run;
  return K2Run{unit_base + lo, unit_base + hi};
}

// the units of a launch piece: what its grid of one-wave units would have covered, cut at the end of the batch
K2_CLAIM_HD uint64_t k2_piece_units(uint64_t total_units, uint64_t unit_base, uint64_t piece_workgroups) {
  const uint64_t left = total_units > unit_base ? total_units - unit_base : 0;
  return left < piece_workgroups * 4 ? left : piece_workgroups * 4;
}

// the grid of a persistent launch: as many workgroups as the chip holds at once (`resident`), fewer where the piece has fewer; `asked`
// (KMCPG_K2_PERSIST_WGS, for tests) != 0: that many, whatever the piece — the kernel is correct on any grid
K2_CLAIM_HD unsigned k2_persist_grid(unsigned piece_workgroups, unsigned resident, uint32_t asked) {
  const unsigned nb = asked ? asked : (piece_workgroups < resident ? piece_workgroups : resident);
  return nb < 1 ? 1 : (nb > (unsigned)K2_MAX_BLOCKS ? (unsigned)K2_MAX_BLOCKS : nb);
}

}  // namespace kmcpg
