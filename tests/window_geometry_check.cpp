// window_geometry_check.cpp — kmcp-search's sliding-window geometry (cli/search_batch.hpp window_count / window_span) against the library's
// (kmcpg_window_count / kmcpg_window_locate): the reader sizes batches by the one, the library returns one result row per window of the
// other, and the writer names row i by the first again — they must agree on every count, start and end.  CPU only; built by
// tests/test_window_geometry_cpu.py with ASan/UBSan.
#include <stdarg.h>

#include <random>

#include "../cli/search_batch.hpp"

[[noreturn]] void die(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
  exit(255);
}

int main() {
  const uint64_t pairs[][2] = {{1, 1}, {1, 10}, {4, 10}, {10, 10}, {13, 10}, {100, 300}};  // (step, window)
  std::mt19937_64 g(5);
  unsigned long long checked = 0;
  for (const auto& sw : pairs)
    for (int greedy = 0; greedy < 2; greedy++) {
      const uint64_t S = sw[0], W = sw[1];
      const kmcpg_window_spec spec{S, W, greedy, 0};
      std::vector<uint64_t> lens{0, 1, W - 1, W, W + 1, W + S - 1, W + S};
      for (int i = 0; i < 300; i++) lens.push_back(g() % 5001);
      // every length alone: the count
      std::vector<uint64_t> offs{0};
      uint64_t want_windows = 0;
      for (const uint64_t L : lens) {
        const uint64_t one[2] = {0, L};
        uint64_t nw = ~0ull;
        if (kmcpg_window_count(one, 1, &spec, &nw, nullptr) != 0) die("kmcpg_window_count: %s", kmcpg_last_error());
        if (window_count(L, spec) != nw) {
          printf("FAIL count: L %llu S %llu W %llu greedy %d: header %llu, library %llu\n", (unsigned long long)L, (unsigned long long)S,
                 (unsigned long long)W, greedy, (unsigned long long)window_count(L, spec), (unsigned long long)nw);
          return 1;
        }
        offs.push_back(offs.back() + L);
        want_windows += nw;
      }
      // all of them as one batch: every window's record and span
      const uint32_t n_reads = (uint32_t)lens.size();
      uint64_t nw = 0, nb = 0;
      if (kmcpg_window_count(offs.data(), n_reads, &spec, &nw, &nb) != 0) die("kmcpg_window_count: %s", kmcpg_last_error());
      if (nw != want_windows) { printf("FAIL batch count\n"); return 1; }
      std::vector<uint32_t> read((size_t)nw + 1);
      std::vector<uint64_t> start((size_t)nw + 1);
      if (kmcpg_window_locate(offs.data(), n_reads, &spec, 0, nw, read.data(), start.data()) != 0) die("kmcpg_window_locate: %s", kmcpg_last_error());
      uint64_t row = 0, bases = 0;
      for (uint32_t r = 0; r < n_reads; r++) {
        const uint64_t L = lens[r];
        for (uint64_t j = 0; j < window_count(L, spec); j++, row++) {
          const WindowSpan w = window_span(L, j, spec);
          // Record and first base are the library's own (kmcpg_window_locate).  It reports no end: `start + window, cut at the record's end`
          // is kmcp_gpu.h's wording restated here, the same formula window_span uses, so this line alone would not catch a shared mistake.
          // What the library does say about ends is the sum of all windows' bases (kmcpg_window_count), compared below — a total, in which
          // two wrong ends could cancel.
          if (row >= nw || read[(size_t)row] != r || start[(size_t)row] != w.start || w.end != std::min(start[(size_t)row] + W, L) || w.end <= w.start) {
            printf("FAIL span: row %llu, record %u (L %llu), window %llu, S %llu W %llu greedy %d: header %llu-%llu\n", (unsigned long long)row, r,
                   (unsigned long long)L, (unsigned long long)j, (unsigned long long)S, (unsigned long long)W, greedy, (unsigned long long)w.start,
                   (unsigned long long)w.end);
            return 1;
          }
          bases += w.end - w.start;
        }
      }
      if (row != nw || bases != nb) {
        printf("FAIL totals: S %llu W %llu greedy %d: %llu windows of %llu bases, library %llu of %llu\n", (unsigned long long)S, (unsigned long long)W, greedy,
               (unsigned long long)row, (unsigned long long)bases, (unsigned long long)nw, (unsigned long long)nb);
        return 1;
      }
      checked += nw;
    }
  printf("ok: %llu windows\n", checked);
  return 0;
}
