// window_plan_check.cpp — kmcp_amd/csrc/window_plan.hpp compiled alone (g++, no HIP): plan_windows, stage_windows and the per-window
// computation of k_window_desc (window_desc_at, run here in a host loop) against a plain walk of the enumeration rule, window by window.
//
//   window_plan_check          the whole grid of tests/test_window_plan_cpu.py, checked here; prints "ok: ..." or the first disagreement
//   window_plan_check dump     a small grid, printed: the Python test recomputes every number from tests/test_sliding_cpu.py::windows_of
//
// Built with -fsanitize=address,undefined by the test.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../kmcp_amd/csrc/window_plan.hpp"

using namespace kmcpg;

namespace {

struct Win {
  uint32_t r;
  uint64_t i, e;  // bases [i, e) of read r
};

// the rule of INTEGRATION.md, one window at a time: starts 0, S, 2S, ...; e = i + W; past the end: greedy cuts at L and goes on while i < L
std::vector<Win> walk(const std::vector<uint64_t>& offs, const kmcpg_window_spec& s) {
  std::vector<Win> out;
  for (uint32_t r = 0; r + 1 < offs.size(); r++) {
    const uint64_t L = offs[r + 1] - offs[r];
    for (uint64_t i = 0;; i += s.step) {
      uint64_t e = i + s.window;
      if (e > L) {
        if (!s.greedy || i >= L) break;
        e = L;
      }
      out.push_back({r, i, e});
    }
  }
  return out;
}

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

// 0, 1, W-1, W, W+1, W+S-1, W+S, then n_random lengths: most of a few windows, some up to `longest`
std::vector<uint64_t> lengths(uint64_t S, uint64_t W, int n_random, uint64_t longest) {
  std::vector<uint64_t> len = {0, 1, W - 1, W, W + 1, W + S - 1, W + S};
  for (int i = 0; i < n_random; i++) len.push_back(i % 8 == 7 ? rnd() % (longest + 1) : rnd() % (3 * (W + S) + 2));
  return len;
}

struct Case {
  kmcpg_window_spec s;
  uint64_t budget, max_win;
};
#define FAIL(...)                                                                                                                          \
  do {                                                                                                                                     \
    printf("S %llu W %llu greedy %d budget %llu max_win %llu: ", (unsigned long long)c.s.step, (unsigned long long)c.s.window, (int)c.s.greedy, \
           (unsigned long long)c.budget, (unsigned long long)c.max_win);                                                                   \
    printf(__VA_ARGS__);                                                                                                                   \
    printf("\n");                                                                                                                          \
    return false;                                                                                                                          \
  } while (0)

bool check(const Case& c, const std::vector<uint64_t>& offs, uint64_t k, uint64_t* n_pieces, uint64_t* n_windows, bool dump) {
  const std::vector<Win> all = walk(offs, c.s);
  const std::vector<WinPiece> plan = plan_windows(offs.data(), (uint32_t)(offs.size() - 1), c.s, c.budget, c.max_win);
  // expected partition: the window-by-window greedy walk — a piece closes when the next window would exceed either limit, a window that fits
  // nowhere goes alone
  std::vector<uint64_t> want_n;
  {
    uint64_t n = 0, b = 0;
    for (const Win& w : all) {
      if (n && (n + 1 > c.max_win || b + (w.e - w.i) > c.budget)) {
        want_n.push_back(n);
        n = b = 0;
      }
      n++;
      b += w.e - w.i;
    }
    if (n) want_n.push_back(n);
  }
  size_t at = 0;  // next window of `all`
  WinStaging ws;
  for (size_t pi = 0; pi < plan.size(); pi++) {
    const WinPiece& pc = plan[pi];
    if (pc.n_win == 0 || pc.sl.empty()) FAIL("piece %zu is empty", pi);
    if (pc.n_win > c.max_win) FAIL("piece %zu holds %llu windows", pi, (unsigned long long)pc.n_win);
    if (pc.bases > c.budget && pc.n_win != 1) FAIL("piece %zu holds %llu bases in %llu windows", pi, (unsigned long long)pc.bases, (unsigned long long)pc.n_win);
    const size_t first = at;
    uint64_t bases = 0, longest = 0;
    for (const WinSlice& x : pc.sl) {
      if (x.j1 <= x.j0) FAIL("piece %zu: an empty slice", pi);
      for (uint64_t j = x.j0; j < x.j1; j++, at++) {
        if (at >= all.size() || all[at].r != x.r || all[at].i != j * c.s.step) FAIL("piece %zu: window %zu of the batch is not (read %u, window %llu)", pi, at, x.r, (unsigned long long)j);
        bases += all[at].e - all[at].i;
        longest = std::max(longest, all[at].e - all[at].i);
      }
    }
    if (at - first != pc.n_win || bases != pc.bases) FAIL("piece %zu: n_win %llu bases %llu, recounted %zu and %llu", pi, (unsigned long long)pc.n_win, (unsigned long long)pc.bases, at - first, (unsigned long long)bases);
    // what the piece stages, and the descriptor of every window as the device computes it
    stage_windows(offs.data(), c.s, pc, k, &ws);
    const uint32_t ns = (uint32_t)ws.copies.size();
    if (ws.soffs.size() != ns + 1u || ws.wpre.size() != ns + 1u || ws.vpre.size() != ns + 1u || ws.cpre.size() != ns + 1u) FAIL("piece %zu: prefix arrays of different lengths", pi);
    if (ws.wpre[ns] != pc.n_win || ws.vpre[ns] != pc.bases) FAIL("piece %zu: wpre / vpre end at %llu / %llu", pi, (unsigned long long)ws.wpre[ns], (unsigned long long)ws.vpre[ns]);
    if (ws.wmax != longest) FAIL("piece %zu: wmax %llu, the longest window has %llu", pi, (unsigned long long)ws.wmax, (unsigned long long)longest);
    for (uint32_t q = 0; q < ns; q++) {
      const uint64_t ls = ws.copies[q].len;
      if (ws.soffs[q + 1] - ws.soffs[q] != ls) FAIL("piece %zu slice %u: soffs and the copy disagree", pi, q);
      if (ws.copies[q].at + ls > offs.back()) FAIL("piece %zu slice %u: copies text past the batch", pi, q);
      if (ws.cpre[q + 1] - ws.cpre[q] != (ls >= k ? (ls - k + 1 + K1_WIN_CHUNK - 1) / K1_WIN_CHUNK : 0)) FAIL("piece %zu slice %u: cpre", pi, q);
    }
    if (dump) {
      printf("piece %llu %llu %llu\nslices", (unsigned long long)pc.n_win, (unsigned long long)pc.bases, (unsigned long long)ws.wmax);
      for (const WinSlice& x : pc.sl) printf(" %u:%llu:%llu", x.r, (unsigned long long)x.j0, (unsigned long long)x.j1);
      printf("\ncopies");
      for (const WinStaging::Copy& y : ws.copies) printf(" %llu:%llu", (unsigned long long)y.at, (unsigned long long)y.len);
      printf("\ncpre");
      for (uint64_t v : ws.cpre) printf(" %llu", (unsigned long long)v);
      printf("\ndesc");
    }
    uint64_t prefix = 0;
    uint32_t q = 0;
    for (uint64_t w = 0; w < pc.n_win; w++) {
      uint64_t src = ~0ull, off = ~0ull;
      window_desc_at(ws.soffs.data(), ws.wpre.data(), ws.vpre.data(), ns, w, c.s.step, c.s.window, &src, &off);
      const Win& x = all[first + w];
      // brute force: the staged text is the copies one behind the other; the window lies whole in one of them, its first base at src
      while (q + 1 < ns && ws.soffs[q + 1] <= src) q++;
      if (src < ws.soffs[q] || src + (x.e - x.i) > ws.soffs[q + 1]) FAIL("piece %zu window %llu: src %llu leaves its slice", pi, (unsigned long long)w, (unsigned long long)src);
      if (ws.copies[q].at + (src - ws.soffs[q]) != offs[x.r] + x.i) FAIL("piece %zu window %llu: src %llu is not base %llu of read %u", pi, (unsigned long long)w, (unsigned long long)src, (unsigned long long)x.i, x.r);
      if (off != prefix) FAIL("piece %zu window %llu: offs %llu, the windows before it hold %llu bases", pi, (unsigned long long)w, (unsigned long long)off, (unsigned long long)prefix);
      prefix += x.e - x.i;
      if (dump) printf(" %llu:%llu", (unsigned long long)src, (unsigned long long)off);
    }
    if (dump) printf("\n");
    if (pi >= want_n.size() || want_n[pi] != pc.n_win) FAIL("walk: piece %zu holds %llu windows, the greedy walk cuts after %llu", pi, (unsigned long long)pc.n_win, (unsigned long long)(pi < want_n.size() ? want_n[pi] : 0));
  }
  if (at != all.size()) FAIL("%zu of %zu windows in the plan", at, all.size());
  if (plan.size() != want_n.size()) FAIL("walk: %zu pieces, the greedy walk makes %zu", plan.size(), want_n.size());
  *n_pieces += plan.size();
  *n_windows += all.size();
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const bool dump = argc > 1 && strcmp(argv[1], "dump") == 0;
  const uint64_t specs[6][2] = {{1, 1}, {1, 10}, {4, 10}, {10, 10}, {13, 10}, {100, 300}};
  const uint64_t k = 21;
  uint64_t n_cases = 0, n_pieces = 0, n_windows = 0;
  for (const auto& sw : specs)
    for (int greedy = 0; greedy < 2; greedy++) {
      const uint64_t S = sw[0], W = sw[1];
      const std::vector<uint64_t> len = dump ? lengths(S, W, 12, 400) : lengths(S, W, 200, 5000);
      std::vector<uint64_t> offs(1, 0);
      for (uint64_t l : len) offs.push_back(offs.back() + l);
      for (uint64_t budget : {(uint64_t)1, W, 2 * W + 1, (uint64_t)1000000000})
        for (uint64_t max_win : {(uint64_t)1, (uint64_t)3, (uint64_t)1 << 22}) {
          Case c{};
          c.s.step = S;
          c.s.window = W;
          c.s.greedy = (uint32_t)greedy;
          c.budget = budget;
          c.max_win = max_win;
          if (dump) {
            printf("case %llu %llu %d %llu %llu %llu %d\nlens", (unsigned long long)S, (unsigned long long)W, greedy, (unsigned long long)budget, (unsigned long long)max_win,
                   (unsigned long long)k, (int)K1_WIN_CHUNK);
            for (uint64_t l : len) printf(" %llu", (unsigned long long)l);
            printf("\n");
          }
          if (!check(c, offs, k, &n_pieces, &n_windows, dump)) return 1;
          n_cases++;
        }
    }
  printf("ok: %llu cases, %llu pieces, %llu windows\n", (unsigned long long)n_cases, (unsigned long long)n_pieces, (unsigned long long)n_windows);
  return 0;
}
