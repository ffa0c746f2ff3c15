// fixed4_check.cpp — host instantiation of kmcp_amd/csrc/k3_set_order.hpp (the merge order of database sets) behind two C functions,
// built as a shared object and driven by tests/test_fixed4_cpu.py:
//   fixed4_sweep     fixed4(x) against the digits snprintf("%.4f", x) prints, over the value families the test names;
//   set_order_check  the set order of a random segment — through the device's two passes (exact keys sorted, set keys sorted, pairs read
//                    back, mixed runs counted as the kernels count them) and through the host twin (set_order_host) — against
//                    "print every score with %.4f, parse it back, stable-sort descending over (member, exact K3 order)", which is what
//                    kmcp-merge does with the members' separate results (cli/kmcp_merge.cpp).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../kmcp_amd/csrc/k3_set_order.hpp"

using namespace kmcpg;

namespace {

// the digits of "%.4f" as one integer: "0.1235" -> 1235, "1.0000" -> 10000
uint64_t printed4(double x) {
  char buf[64];
  snprintf(buf, sizeof buf, "%.4f", x);
  uint64_t v = 0;
  for (const char* p = buf; *p; p++)
    if (*p >= '0' && *p <= '9') v = v * 10 + (uint64_t)(*p - '0');
  return v;
}

struct Sweep {
  uint64_t checked = 0, bad = 0;
  double first_bad = -1;
  void one(double x) {
    checked++;
    if (fixed4(x) != printed4(x)) {
      if (!bad) first_bad = x;
      bad++;
    }
  }
};

}  // namespace

// out[0] = values checked, out[1] = mismatches; *first_bad = the first value that differed
extern "C" void fixed4_sweep(uint64_t seed, uint64_t* out, double* first_bad) {
  Sweep s;
  std::mt19937_64 rng(seed);
  // every c / n a score can be: all c <= n for small n, 1000 random c for the large ones
  for (uint64_t n = 1; n <= 300; n++)
    for (uint64_t c = 0; c <= n; c++) s.one((double)c / (double)n);
  for (uint64_t n : {9999ull, 10000ull, 10001ull, 20000ull, 131072ull})
    for (int i = 0; i < 1000; i++) s.one((double)(rng() % (n + 1)) / (double)n);
  // the half-way cases: j / 20000 and the doubles on either side of it
  for (uint64_t j = 0; j <= 20000; j++) {
    const double x = (double)j / 20000.0;
    s.one(x);
    s.one(nextafter(x, 2.0));
    if (j) s.one(nextafter(x, -1.0));
  }
  s.one(0.0);
  s.one(1.0);
  s.one(1.0 / (double)(1ull << 46));  // the smallest positive c / size of a 2^46 k-mer column
  std::uniform_real_distribution<double> u(0.0, 1.0);
  for (int i = 0; i < 1000000; i++) s.one(u(rng));
  // beyond [0, 1]: a count above the column's size (Bloom false positives) prints as any other double
  for (int i = 0; i < 10000; i++) s.one(u(rng) * 4096.0);
  out[0] = s.checked;
  out[1] = s.bad;
  *first_bad = s.first_bad;
}

// One random segment of m matches of a query with nh k-mers on a set of n_members members.  Returns 0 when both the two-pass order and
// the host twin equal the reference order and all three agree on the number of mixed runs; otherwise a bit mask (1 two-pass order,
// 2 host twin order, 4 two-pass mixed-run count, 8 host twin count).  ties[0] = adjacent pairs of the reference order with equal printed
// score, ties[1] = adjacent pairs, ties[2] = runs of equal printed score with more than one member.
extern "C" int set_order_check(int32_t sort_mode, uint32_t m, uint64_t seed, uint64_t* ties) {
  std::mt19937_64 rng(seed * 0x9e3779b97f4a7c15ull + m * 31 + (uint64_t)sort_mode);
  const uint32_t n_members = 2 + (uint32_t)(rng() % 15);  // 2 .. 16
  const uint32_t per = 320, n_cols = n_members * per;     // >= 4097 columns only with many members: columns may repeat below
  std::vector<uint32_t> base(n_members);
  for (uint32_t i = 0; i < n_members; i++) base[i] = i * per;
  // column sizes: half of the columns share a handful of sizes near 3e5 (neighbouring counts print equal tCov / jacc), the rest are
  // huge (up to 2^40: scores that print 0.0000)
  const uint64_t pool[5] = {200000, 250000, 250001, 300000, 399999};
  std::vector<uint64_t> size(n_cols);
  for (auto& z : size) z = (rng() & 1) ? pool[rng() % 5] : (1ull << 40) - (rng() % 1000);
  const double nh = 20000.0;  // qCov = c / 20000: counts step through the half-way cases of %.4f
  std::vector<kmcpg_pair> pairs(m);
  for (uint32_t i = 0; i < m; i++) {
    pairs[i].col = (uint32_t)(rng() % n_cols);
    pairs[i].count = 11000 + (uint32_t)(rng() % 41);
  }
  // (a real segment names a column once; repeats are harmless to an order that ends in the column — but keep them distinct where there is room)
  if (m <= n_cols) {
    std::vector<uint32_t> perm(n_cols);
    for (uint32_t i = 0; i < n_cols; i++) perm[i] = i;
    std::shuffle(perm.begin(), perm.end(), rng);
    for (uint32_t i = 0; i < m; i++) pairs[i].col = perm[i];
  }
  // ---- the exact K3 order
  std::vector<Key> keys(m);
  for (uint32_t i = 0; i < m; i++) keys[i] = make_key(sort_mode, size.data(), pairs[i], nh);
  std::sort(keys.begin(), keys.end(), [](const Key& x, const Key& y) { return key_less(x, y); });
  std::vector<kmcpg_pair> exact(m);
  for (uint32_t i = 0; i < m; i++) exact[i] = pair_of(sort_mode, keys[i]);
  // ---- reference: (member, exact order), then a stable sort by the parsed printed score, descending
  struct Row {
    kmcpg_pair p;
    uint32_t member;
    double parsed;
  };
  std::vector<Row> ref;
  for (uint32_t mem = 0; mem < n_members; mem++)
    for (uint32_t i = 0; i < m; i++)
      if (exact[i].col / per == mem) {
        const double c = (double)exact[i].count, nt = (double)size[exact[i].col];
        const double score = sort_mode == 0 ? c / nh : (sort_mode == 1 ? c / nt : c / (nh + nt - c));
        char buf[64];
        snprintf(buf, sizeof buf, "%.4f", score);
        ref.push_back(Row{exact[i], mem, strtod(buf, nullptr)});
      }
  std::stable_sort(ref.begin(), ref.end(), [](const Row& x, const Row& y) { return x.parsed > y.parsed; });
  uint64_t ref_mixed = 0;
  ties[0] = ties[1] = 0;
  for (uint32_t i = 0; i < m;) {
    uint32_t j = i;
    while (j + 1 < m && ref[j + 1].parsed == ref[i].parsed) j++;
    if (ref[j].member != ref[i].member) ref_mixed++;
    ties[0] += j - i;
    i = j + 1;
  }
  ties[1] = m ? m - 1 : 0;
  ties[2] = ref_mixed;
  int bad = 0;
  // ---- the device's second pass: set keys in the slots of the exact keys, sorted, pairs read back
  {
    std::vector<Key> t(m);
    for (uint32_t i = 0; i < m; i++) {
      const kmcpg_pair p = pair_of(sort_mode, keys[i]);
      double score;
      if (sort_mode == 0) score = (double)p.count / nh;
      else {
        const uint64_t b = ~keys[i].a;
        memcpy(&score, &b, sizeof score);
      }
      t[i] = set_key(fixed4(score), set_member(p.col, base.data(), n_members), i, p);
    }
    std::sort(t.begin(), t.end(), [](const Key& x, const Key& y) { return key_less(x, y); });
    uint64_t mixed = 0;
    for (uint32_t i = 0; i < m; i++) {
      const kmcpg_pair p = set_pair_of(t[i]);
      if (p.col != ref[i].p.col || p.count != ref[i].p.count) bad |= 1;
      mixed += set_mixed_run_at(t.data(), m, i) ? 1 : 0;
    }
    if (mixed != ref_mixed) bad |= 4;
  }
  // ---- the host twin
  {
    std::vector<kmcpg_pair> h = exact;
    const uint64_t* sz = size.data();
    const uint32_t* bs = base.data();
    const uint64_t mixed = set_order_host(h.data(), (uint64_t)m, [=](const kmcpg_pair& p) {
      return set_host_key(fixed4(set_score(sort_mode, p.count, sz[p.col], nh)), set_member(p.col, bs, n_members));
    });
    for (uint32_t i = 0; i < m; i++)
      if (h[i].col != ref[i].p.col || h[i].count != ref[i].p.count) bad |= 2;
    if (mixed != ref_mixed) bad |= 8;
  }
  return bad;
}
