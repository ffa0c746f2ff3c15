// win_cases_print.cpp — kmcp_amd/csrc/window_plan.hpp compiled alone (g++, no HIP): stage_windows and window_desc_at for the pieces of
// tests/win_cases.py, printed as numbers.  tests/test_win_cases_cpu.py holds the plan's own Python staging against them.
//
// stdin, one piece per line:   <id> <k> <S> <W> <greedy> <n_reads> <len> ... <n_slices> <read> <j0> <j1> ...
// stdout per piece:            piece <id> <n_win> <bases> <wmax>, then the lines copies (at:len), soffs, wpre, vpre, cpre, src, koff
//
// Built with -fsanitize=address,undefined by the test.
#include <stdio.h>

#include <iostream>
#include <string>
#include <vector>

#include "../kmcp_amd/csrc/window_plan.hpp"

using namespace kmcpg;

static void line(const char* key, const std::vector<uint64_t>& v) {
  printf("%s", key);
  for (uint64_t x : v) printf(" %llu", (unsigned long long)x);
  printf("\n");
}

int main() {
  std::string id;
  while (std::cin >> id) {
    uint64_t k, n_reads, n_slices;
    kmcpg_window_spec s{};
    int greedy;
    if (!(std::cin >> k >> s.step >> s.window >> greedy >> n_reads)) return 1;
    s.greedy = greedy;
    std::vector<uint64_t> offs(1, 0);
    for (uint64_t i = 0, len; i < n_reads; i++) {
      if (!(std::cin >> len)) return 1;
      offs.push_back(offs.back() + len);
    }
    if (!(std::cin >> n_slices)) return 1;
    WinPiece pc;
    for (uint64_t i = 0; i < n_slices; i++) {
      WinSlice x{};
      if (!(std::cin >> x.r >> x.j0 >> x.j1) || x.r >= n_reads) return 1;
      const uint64_t L = offs[x.r + 1] - offs[x.r];
      if (x.j0 >= x.j1 || x.j1 > win_count(L, s)) return 1;
      pc.sl.push_back(x);
      pc.n_win += x.j1 - x.j0;
      pc.bases += win_bases_before(L, x.j1, s) - win_bases_before(L, x.j0, s);
    }
    WinStaging ws;
    stage_windows(offs.data(), s, pc, k, &ws);
    const uint32_t ns = (uint32_t)ws.copies.size();
    printf("piece %s %llu %llu %llu\ncopies", id.c_str(), (unsigned long long)pc.n_win, (unsigned long long)pc.bases, (unsigned long long)ws.wmax);
    for (const WinStaging::Copy& c : ws.copies) printf(" %llu:%llu", (unsigned long long)c.at, (unsigned long long)c.len);
    printf("\n");
    line("soffs", ws.soffs);
    line("wpre", ws.wpre);
    line("vpre", ws.vpre);
    line("cpre", ws.cpre);
    // what k_window_desc computes: one thread per window, and the last one closes offs with vpre's end
    std::vector<uint64_t> src(pc.n_win), koff(pc.n_win + 1, 0);
    for (uint64_t w = 0; w < pc.n_win; w++) window_desc_at(ws.soffs.data(), ws.wpre.data(), ws.vpre.data(), ns, w, s.step, s.window, &src[w], &koff[w]);
    koff[pc.n_win] = ws.vpre[ns];
    line("src", src);
    line("koff", koff);
  }
  return 0;
}
