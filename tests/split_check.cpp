// split_check.cpp — kmcp_amd/csrc/split_plan.hpp compiled for the host (tests/test_split_cpu.py): reads cases
//   "len n overlap min_ref k_min count first0 end0 first1 end1 ..."
// from the file named on the command line — the chunks tests/synth.py split_chunks cuts and compute.go's drop rule keeps, written by the
// test — and compares split_bounds with every one; then invariants of its own over the same cases (windows in order, inside the sequence,
// longer than the overlap, at most n of them; a small cap changes the count of nothing).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../kmcp_amd/csrc/split_plan.hpp"

using namespace kmcpg;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  unsigned long long cases = 0, bad = 0;
  std::vector<uint64_t> first, end, wf, we;
  unsigned long long len, n, ov, mr, k, cnt;
  while (fscanf(f, "%llu %llu %llu %llu %llu %llu", &len, &n, &ov, &mr, &k, &cnt) == 6) {
    wf.resize(cnt);
    we.resize(cnt);
    for (unsigned long long i = 0; i < cnt; i++) {
      unsigned long long a, b;
      if (fscanf(f, "%llu %llu", &a, &b) != 2) return 2;
      wf[i] = a;
      we[i] = b;
    }
    SplitSpec sp;
    sp.n = n;
    sp.overlap = ov;
    sp.min_ref = mr;
    sp.k_min = k;
    const uint64_t got = split_bounds(len, sp, nullptr, nullptr, 0);
    first.assign(got + 1, 0);
    end.assign(got + 1, 0);
    bool ok = got == cnt && split_bounds(len, sp, first.data(), end.data(), got) == got;
    for (uint64_t i = 0; ok && i < got; i++) {
      ok = first[i] == wf[i] && end[i] == we[i];
      ok = ok && end[i] <= len && first[i] < end[i] && end[i] - first[i] > ov + 1 && end[i] - first[i] >= k;
      ok = ok && (i == 0 || (first[i] > first[i - 1] && end[i] >= end[i - 1]));
    }
    ok = ok && got <= (n > 1 ? n : 1);
    if (got > 1) {  // a cap below the count: the count stands, nothing is written past the cap
      uint64_t a[2] = {~0ull, ~0ull}, b[2] = {~0ull, ~0ull};
      ok = ok && split_bounds(len, sp, a, b, 1) == got && a[0] == wf[0] && b[0] == we[0] && a[1] == ~0ull && b[1] == ~0ull;
    }
    if (!ok && bad++ < 10) fprintf(stderr, "wrong: len %llu n %llu overlap %llu min_ref %llu k %llu: %llu chunks, %llu wanted\n", len, n, ov, mr, k, (unsigned long long)got, cnt);
    cases++;
  }
  fclose(f);
  printf("%llu cases, %llu wrong\n", cases, bad);
  return bad ? 1 : 0;
}
