// window_plan.hpp — the geometry of sliding windows (kmcpg_submit_windows), stated once for the host and the device: how many windows a read
// has and how many bases they hold, how a batch's windows are cut into pieces, what a piece stages (slices of reads and their prefix sums) and
// how a window's descriptor follows from them (k_window_desc, windows.hip).  Pure integer code, no HIP runtime: tests/window_plan_check.cpp
// compiles it alone.  Enumeration (seqkit sliding, restated in INTEGRATION.md): windows of a read of L bases start at 0, S, 2S, ... and end at
// min(i + W, L); without greedy only windows with i + W <= L exist, with greedy every i < L does.
// (cli/search_batch.hpp states the enumeration a second time on purpose: the CLI sits above the ABI, tests/window_geometry_check.cpp holds
// the two against each other.)
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "common.hpp"
#include "fastmod.hpp"  // KMCPG_HD

namespace kmcpg {

// bases of windows 0 .. j-1 of a read (or a staged slice) of L bases: the full ones (W each), then — greedy — the ones cut at its end
KMCPG_HD uint64_t win_bases_before(uint64_t L, uint64_t j, uint64_t S, uint64_t W) {
  const uint64_t full = L >= W ? (L - W) / S + 1 : 0;  // windows that hold W bases
  if (j <= full) return j * W;
  // sum over t in [full, j) of L - t S
  return full * W + (j - full) * L - S * ((j * (j - 1)) / 2 - (full * (full - (full > 0 ? 1 : 0))) / 2);
}

// What one thread of k_window_desc computes for window w of a piece, from the staged slices' text offsets (soffs), window prefix (wpre) and
// window-base prefix (vpre): its slice q (the last q with wpre[q] <= w) and its number j there, then
//   *src = soffs[q] + j S                                       (first base in the staged text)
//   *off = vpre[q] + bases of windows 0 .. j-1 of the slice      (the window numbering the rest of the pipeline sees)
KMCPG_HD void window_desc_at(const uint64_t* __restrict__ soffs, const uint64_t* __restrict__ wpre, const uint64_t* __restrict__ vpre, uint32_t n_slices,
                             uint64_t w, uint64_t S, uint64_t W, uint64_t* src, uint64_t* off) {
  uint32_t lo = 0, hi = n_slices;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (wpre[mid] <= w) lo = mid;
    else hi = mid;
  }
  const uint32_t q = lo;
  const uint64_t j = w - wpre[q];
  const uint64_t v = win_bases_before(soffs[q + 1] - soffs[q], j, S, W);
  *src = soffs[q] + j * S;
  *off = vpre[q] + v;
}

// ---- host only: the windows of a batch, its pieces, and what a piece stages
#pragma GCC visibility push(hidden)  // (internal: nothing here becomes a dynamic symbol of the library)
inline uint64_t win_count(uint64_t L, const kmcpg_window_spec& s) {
  if (L == 0) return 0;
  if (s.greedy) return (L + s.step - 1) / s.step;
  return L >= s.window ? (L - s.window) / s.step + 1 : 0;
}
inline uint64_t win_bases_before(uint64_t L, uint64_t j, const kmcpg_window_spec& s) { return win_bases_before(L, j, s.step, s.window); }

struct WinSlice {
  uint32_t r;
  uint64_t j0, j1;  // windows [j0, j1) of read r
};
struct WinPiece {
  std::vector<WinSlice> sl;
  uint64_t n_win = 0, bases = 0;
};

// the batch's windows in order, cut where a piece would exceed `budget` window bases or `max_win` windows (one window always goes)
inline std::vector<WinPiece> plan_windows(const uint64_t* offs, uint32_t n, const kmcpg_window_spec& s, uint64_t budget, uint64_t max_win) {
  std::vector<WinPiece> out;
  WinPiece cur;
  for (uint32_t r = 0; r < n; r++) {
    const uint64_t L = offs[r + 1] - offs[r], c = win_count(L, s);
    uint64_t j = 0;
    while (j < c) {
      const uint64_t room = budget > cur.bases ? budget - cur.bases : 0, vj = win_bases_before(L, j, s);
      const uint64_t lim = std::min<uint64_t>(c, j + (max_win - cur.n_win));
      uint64_t j1 = lim;
      if (win_bases_before(L, lim, s) - vj > room) {  // the last j1 in [j, lim) whose windows fit
        uint64_t lo = j, hi = lim;
        while (hi - lo > 1) {
          const uint64_t mid = lo + (hi - lo) / 2;
          if (win_bases_before(L, mid, s) - vj <= room) lo = mid;
          else hi = mid;
        }
        j1 = lo;
      }
      if (j1 == j) {
        if (cur.n_win) {
          out.push_back(std::move(cur));
          cur = WinPiece();
          continue;
        }
        j1 = j + 1;
      }
      cur.sl.push_back({r, j, j1});
      cur.n_win += j1 - j;
      cur.bases += win_bases_before(L, j1, s) - vj;
      j = j1;
      if (cur.n_win >= max_win || cur.bases >= budget) {
        out.push_back(std::move(cur));
        cur = WinPiece();
      }
    }
  }
  if (cur.n_win) out.push_back(std::move(cur));
  return out;
}

// What a piece stages when its windows are read in place: the ranges of the batch's text that go up one behind the other (`copies`; their
// ends in the staged text are soffs), and per staged slice the prefix sums of its windows (wpre), of its windows' bases (vpre) and of its
// chunks of K1_WIN_CHUNK k-mer positions for k-mers of k bases (cpre); wmax = the longest window.  A slice is a run of windows of one read —
// or, where windows do not overlap (S >= W: -s 1000 -W 212), each window on its own: the bases between them stay home.
struct WinStaging {
  struct Copy {
    uint64_t at, len;  // bytes [at, at + len) of the batch's text
  };
  std::vector<Copy> copies;
  std::vector<uint64_t> soffs, wpre, vpre, cpre;
  uint64_t wmax = 0;
};

inline void stage_windows(const uint64_t* offs, const kmcpg_window_spec& s, const WinPiece& pc, uint64_t k, WinStaging* out) {
  out->copies.clear();
  out->soffs.assign(1, 0);
  out->wpre.assign(1, 0);
  out->vpre.assign(1, 0);
  out->cpre.assign(1, 0);
  out->wmax = 0;
  auto slice = [&](uint32_t r, uint64_t rlen, uint64_t j0, uint64_t j1) {
    const uint64_t a0 = j0 * s.step, a1 = std::min<uint64_t>((j1 - 1) * s.step + s.window, rlen);
    out->copies.push_back({offs[r] + a0, a1 - a0});
    out->soffs.push_back(out->soffs.back() + (a1 - a0));
    out->wpre.push_back(out->wpre.back() + (j1 - j0));
    out->vpre.push_back(out->vpre.back() + win_bases_before(rlen, j1, s) - win_bases_before(rlen, j0, s));
    out->cpre.push_back(out->cpre.back() + (a1 - a0 >= k ? (a1 - a0 - k + 1 + K1_WIN_CHUNK - 1) / K1_WIN_CHUNK : 0));
    out->wmax = std::max<uint64_t>(out->wmax, std::min<uint64_t>(s.window, a1 - a0));
  };
  for (const WinSlice& x : pc.sl) {
    const uint64_t rlen = offs[x.r + 1] - offs[x.r];
    if (s.step >= s.window)
      for (uint64_t j = x.j0; j < x.j1; j++) slice(x.r, rlen, j, j + 1);
    else
      slice(x.r, rlen, x.j0, x.j1);
  }
}
#pragma GCC visibility pop

}  // namespace kmcpg
