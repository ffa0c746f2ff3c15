// k2_claim_check.cpp — host instantiation of kmcp_amd/csrc/k2_claim.hpp, the unit queue of the persistent short-read COBS kernel: for
// every number of units, unit_base, run length and number of claimers tried, claimers that draw tickets from one counter in any
// interleaving — each keeps asking until a run comes out empty, as a wave does — produce every unit of the piece exactly once, each
// claimer's own units ascend, no run reaches past the piece, and a run handed out after an empty one is empty.  Also the pieces of a
// launch (k2_plan.hpp) as the launcher cuts them: together they cover the batch once.  Built with -fsanitize=address,undefined and run
// by tests/test_k2_claim_cpu.py.
#include <stdio.h>

#include <vector>

#include "../kmcp_amd/csrc/k2_claim.hpp"
#include "../kmcp_amd/csrc/k2_plan.hpp"

using namespace kmcpg;

static unsigned long long bad = 0, checked = 0;

#define CHECK(cond)                                           \
  do {                                                        \
    checked++;                                                \
    if (!(cond)) {                                            \
      if (bad < 20) printf("line %d: %s\n", __LINE__, #cond); \
      bad++;                                                  \
    }                                                         \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // xorshift64*: the interleavings
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545f4914f6cdd1dull;
}

// `claimers` waves on one counter; which of them claims next is drawn at random (order 0: round robin, 1: random, 2: one claimer
// takes everything before the others ask)
static void drain(uint64_t units, uint64_t unit_base, uint32_t run, unsigned claimers, int order) {
  uint64_t counter = 0;
  std::vector<uint8_t> seen(units, 0);
  std::vector<uint64_t> last(claimers, 0);
  std::vector<uint8_t> started(claimers, 0), dry(claimers, 0);
  unsigned live = claimers, turn = 0;
  uint64_t produced = 0, in_order_next = unit_base;
  bool empty_seen = false;
  while (live) {
    unsigned c;
    if (order == 0) c = turn++ % claimers;
    else if (order == 1) c = (unsigned)(rnd() % claimers);
    else for (c = 0; dry[c];) c++;
    if (dry[c]) continue;
    const uint64_t ticket = counter;  // what the atomic add returns
    counter += run;
    const K2Run r = k2_claim_run(ticket, unit_base, units, run);
    CHECK(r.first <= r.last && r.last - r.first <= run);
    CHECK(r.first >= unit_base && r.last <= unit_base + units);
    if (r.first == r.last) {
      empty_seen = true;
      dry[c] = 1;
      live--;
      continue;
    }
    CHECK(!empty_seen);  // tickets ascend: nothing comes after an empty run
    CHECK(r.first == in_order_next);  // the runs themselves are handed out in order, without gaps
    in_order_next = r.last;
    for (uint64_t u = r.first; u < r.last; u++) {
      CHECK(!seen[u - unit_base]);
      seen[u - unit_base] = 1;
      CHECK(!started[c] || u > last[c]);  // a claimer's own units ascend
      started[c] = 1;
      last[c] = u;
      produced++;
    }
  }
  CHECK(produced == units);
  for (uint64_t i = 0; i < units; i++) CHECK(seen[i]);
  CHECK(counter >= units);
}

int main() {
  const uint64_t unit_counts[] = {0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1000, 4099};
  const uint64_t bases[] = {0, 5, K2_MAX_BLOCKS * 4, (1ull << 40) + 3};
  const uint32_t runs[] = {1, 2, 3, 8, 64, K2_CLAIM_RUN};
  const unsigned claimers[] = {1, 2, 3, 4, 16, 257, 1200};  // more claimers than units among them
  for (uint64_t n : unit_counts)
    for (uint64_t b : bases)
      for (uint32_t r : runs)
        for (unsigned c : claimers)
          for (int order = 0; order < 3; order++) drain(n, b, r, c, order);
  // tickets far past the end (every wave of a large grid asks once more than it gets) and at the top of the counter's range
  {
    const K2Run r = k2_claim_run(~0ull - 7, 11, 100, 8);
    CHECK(r.first == r.last && r.first == 111);
    const K2Run s = k2_claim_run(96, 11, 100, 8);
    CHECK(s.first == 107 && s.last == 111);
    const K2Run t = k2_claim_run(0, 0, ~0ull, 8);
    CHECK(t.first == 0 && t.last == 8);
  }
  // the pieces of a launch: what the persistent launcher gives each piece's queue covers the batch once, in order
  const uint64_t totals[] = {0, 1, 3, 4, 5, K2_MAX_BLOCKS * 4 - 1, K2_MAX_BLOCKS * 4, K2_MAX_BLOCKS * 4 + 1, K2_MAX_BLOCKS * 12 + 2};
  for (uint64_t total : totals) {
    K2Launch l;
    l.lpr = 64;
    l.units = total;
    uint64_t at = 0;
    for (uint64_t i = 0; i < k2_n_pieces(l); i++) {
      const K2Piece pc = k2_piece(l, i);
      CHECK(pc.unit_base == at);
      const uint64_t n = k2_piece_units(total, pc.unit_base, pc.workgroups);
      CHECK(n > 0 && n <= (uint64_t)pc.workgroups * 4);
      at += n;
    }
    CHECK(at == total);
  }
  CHECK(k2_piece_units(10, 12, 4) == 0);  // a piece past the end of the batch owns nothing
  // the grid: the chip's fill, the piece if smaller, the number asked for whatever the piece, never none and never past a launch
  CHECK(k2_persist_grid(8388608, 1024, 0) == 1024);
  CHECK(k2_persist_grid(227, 1024, 0) == 227);
  CHECK(k2_persist_grid(227, 1024, 1) == 1);
  CHECK(k2_persist_grid(227, 1024, 4096) == 4096);
  CHECK(k2_persist_grid(0, 1024, 0) == 1);
  CHECK(k2_persist_grid(227, 1024, 0xffffffffu) == K2_MAX_BLOCKS);
  printf("k2_claim_check: %llu checked, %llu wrong\n", checked, bad);
  return bad ? 1 : 0;
}
