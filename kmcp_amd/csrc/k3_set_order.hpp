// k3_set_order.hpp — the order of a query's matches on a DATABASE SET (kmcpg_open_set), as plain functions for device and host.
//
// A set's result is what `kmcp-merge` prints from the members' separate search results (cli/kmcp_merge.cpp): the rows of a query from all
// members, sorted by the PRINTED score ("%.4f" of qCov / tCov / jacc, parsed back) descending, equal printed scores in (input file, row)
// order.  A member's own row order is the exact K3 order (k3_keys.hpp) restricted to its columns, so the set order is
//   1. fixed4(score) descending   2. member ascending   3. the exact K3 order.
// Rounding is monotone: after the exact sort the matches of equal fixed4 are already side by side, and what remains is a stable
// reordering by member inside each such run — the second pass over the sorted segment whose key is set_key below (layout at the top of
// k3_finalize.hip).  Host instantiation: tests/fixed4_check.cpp (tests/test_fixed4_cpu.py); finalize.cpp uses the same functions for the
// segments the device leaves to the host.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "k3_keys.hpp"

namespace kmcpg {

constexpr int SET_MAX_MEMBERS = 16;

// round(x * 10000), half to even, of the double's EXACT binary value: the integer whose digits "%.4f" prints (glibc rounds the exact
// value in the current rounding mode).  x = M * 2^-s with a 53-bit M, so x * 10^4 = (M * 625) / 2^(s - 4), and M * 625 < 2^63: integer
// arithmetic on mantissa and exponent only.  Defined for 0 <= x < 2^32 (a score is count / something >= 1 with a 32-bit count; scores
// are at most 1 unless Bloom false positives push a count above the column's size); negative, NaN and larger values saturate.
KMCPG_K3_HD uint64_t fixed4(double x) {
  const uint64_t u = bits_of_double(x);
  if (u >> 63) return 0;  // negative (or -0)
  const int e = (int)(u >> 52);
  uint64_t m = u & ((1ull << 52) - 1);
  if (e == 0) return 0;                              // zero and subnormals: far below 0.00005
  if (e >= 1023 + 32) return (1ull << 47) - 1;       // >= 2^32, inf, NaN
  m |= 1ull << 52;
  const int sh = (1075 - e) - 4;                     // x * 10^4 = (m * 625) >> sh, sh in 16 .. 1070
  if (sh >= 64) return 0;                            // m * 625 < 2^63 = half of 2^64: rounds to 0
  const uint64_t p = m * 625u;
  const uint64_t q = p >> sh, rem = p & ((1ull << sh) - 1), half = 1ull << (sh - 1);
  return q + ((rem > half || (rem == half && (q & 1))) ? 1u : 0u);
}

// A row's qCov as a consumer of the TSV parses it back: the digits "%.4f" prints of count / qkmers, divided by 10^4 again (both divisions
// correctly rounded: -ffp-contract=off, no fast-math).  What kmcp-regions adds up (k5_summary.hip) and what `kmcp profile` compares with
// --min-hic-ureads-qcov (k6_refstats.hip, refstats.cpp).
KMCPG_K3_HD double printed_qcov(uint32_t count, int32_t qkmers) { return (double)fixed4((double)count / (double)qkmers) / 10000.0; }

// the score `-s` sorts by, with the operations (and therefore the bits) of the Match record the row is printed from
// (util-db-search.go:7487-7489; finalize.cpp kmcpg_expand_pairs)
KMCPG_K3_HD double set_score(int32_t sort_mode, uint32_t count, uint64_t size, double nh) {
  const double c = (double)count;
  if (sort_mode == 0) return c / nh;
  const double nt = (double)size;
  return sort_mode == 1 ? c / nt : c / (nh + nt - c);
}

// member of a global column: base[m] = first global column of member m, ascending, base[0] = 0
KMCPG_K3_HD uint32_t set_member(uint32_t col, const uint32_t* base, uint32_t n_members) {
  uint32_t m = 0;
  for (uint32_t i = 1; i < n_members; i++) m += col >= base[i] ? 1u : 0u;
  return m;
}

// Key of the second pass.  A = ~fixed4 (47 bits) : member (4 bits) : position after the exact sort (13 bits); B = the pair itself.
// A is unique inside a segment (the position), so B never decides: it is the payload the pair is read back from.
constexpr int SET_POS_BITS = 13, SET_MEMBER_BITS = 4;
constexpr uint64_t SET_F4_MAX = (1ull << 47) - 1;
KMCPG_K3_HD Key set_key(uint64_t f4, uint32_t member, uint32_t pos, kmcpg_pair p) {
  Key k;
  k.a = ((SET_F4_MAX - f4) << (SET_MEMBER_BITS + SET_POS_BITS)) | ((uint64_t)member << SET_POS_BITS) | pos;
  k.b = ((uint64_t)p.col << 32) | p.count;
  return k;
}
KMCPG_K3_HD kmcpg_pair set_pair_of(const Key& k) {
  kmcpg_pair p;
  p.col = (uint32_t)(k.b >> 32);
  p.count = (uint32_t)k.b;
  return p;
}
KMCPG_K3_HD uint64_t set_run_of(const Key& k) { return k.a >> (SET_MEMBER_BITS + SET_POS_BITS); }  // equal = one run of equal fixed4
KMCPG_K3_HD uint32_t set_member_of(const Key& k) { return (uint32_t)(k.a >> SET_POS_BITS) & ((1u << SET_MEMBER_BITS) - 1); }

// runs of equal fixed4 that hold more than one member, among keys t[0 .. m) in set order: the run that starts at i is found by the
// thread that looks at i (a binary search for its end: A ascends)
KMCPG_K3_HD bool set_mixed_run_at(const Key* t, uint32_t m, uint32_t i) {
  const uint64_t run = set_run_of(t[i]);
  if (i > 0 && set_run_of(t[i - 1]) == run) return false;  // not the first of its run
  uint32_t lo = i, hi = m;                                 // last index of the run: in [lo, hi)
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (set_run_of(t[mid]) == run) lo = mid;
    else hi = mid;
  }
  return set_member_of(t[lo]) != set_member_of(t[i]);  // members ascend inside a run
}

// Host twin of the second pass, for segments of any length (finalize.cpp: segments above K3_WG_CAP, lists that did not come from K3,
// KMCPG_DEVICE_FINALIZE=0): items[0 .. m) in the exact K3 order -> set order, in place.  key_of(item) = set_host_key(fixed4 of its
// score, its member).  Returns the number of runs of equal fixed4 that hold more than one member.  Positions have no field in this key:
// the sort is a stable one.
KMCPG_K3_HD uint64_t set_host_key(uint64_t f4, uint32_t member) { return ((SET_F4_MAX - f4) << SET_MEMBER_BITS) | member; }
template <class T, class KeyOf>
inline uint64_t set_order_host(T* items, uint64_t m, KeyOf key_of) {
  if (m == 0) return 0;
  static thread_local std::vector<uint64_t> key;
  static thread_local std::vector<uint32_t> ord;
  static thread_local std::vector<T> copy;
  key.resize(m);
  bool sorted = true;
  for (uint64_t i = 0; i < m; i++) {
    key[i] = key_of(items[i]);
    if (i && key[i] < key[i - 1]) sorted = false;
  }
  if (!sorted) {
    ord.resize(m);
    for (uint64_t i = 0; i < m; i++) ord[i] = (uint32_t)i;
    std::stable_sort(ord.begin(), ord.end(), [](uint32_t x, uint32_t y) { return key[x] < key[y]; });
    copy.assign(items, items + m);
    for (uint64_t i = 0; i < m; i++) items[i] = copy[ord[i]];
    std::sort(key.begin(), key.end());
  }
  uint64_t mixed = 0;
  for (uint64_t i = 0; i < m;) {
    uint64_t j = i;
    while (j + 1 < m && (key[j + 1] >> SET_MEMBER_BITS) == (key[i] >> SET_MEMBER_BITS)) j++;
    if (key[j] != key[i]) mixed++;
    i = j + 1;
  }
  return mixed;
}

}  // namespace kmcpg
