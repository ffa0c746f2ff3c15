// cooccur_rule.hpp — what stage 2 of `kmcp profile` counts: the reads shared by pairs of references.  The one rule behind kmcp-refstats
// --cooccur (cli/kmcp_refstats.cpp), the library's table and host half (cooccur.cpp, finalize.cpp), the device code (k7_cooccur.hip: key,
// slot hash and probe sequence are the functions below; its atomics restate reserve / find) and the tests' stand-alone check
// (tests/cooccur_rule_check.cpp).  Host-compilable; the functions marked KMCPG_HD compile for the device too.
//
// Reference counterpart: kmcp/cmd/profile.go:1117-1279 ("stage 2/4: counting ambiguous matches for correcting matches").  Integer-exact.
//
// A PAIR is an unordered pair of printed targets {A, B}, A != B (chunks of one genome are one target); its count is the number of queries
// whose kept rows name both.  The reference keeps ambMatch[hashA][hashB] with hashA < hashB; here a pair is oriented by class index in the
// library and by name in the files — orientation cannot change a count.
//
// The rows a query keeps on the TSV route are K6's rule (refstats_rule.hpp: RefstatsCut) with the differences the reference has:
//   * rows are tested with -t and -f when parsed (as in stage 1);
//   * rows of targets that stage 1 dropped are skipped BEFORE anything else looks at them: they do not start a query, do not move pScore
//     and do not count toward -n — so the "previous row" of --keep-main-matches' gap is the previous KEPT target's row;
//   * the first remaining row of a query is never tested by --keep-perfect-matches / --keep-main-matches, but it is tested by -n (it
//     counts as one: pScore starts at 1024);
//   * once a row is cut, the rest of the query is (a cut row still names the query: the next row of the same name does not open one).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "refstats_rule.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KMCPG_HD __host__ __device__
#else
#define KMCPG_HD
#endif

namespace kmcpg {

// ---- the key: 0 is the empty slot
constexpr uint64_t COOCCUR_EMPTY = 0;
KMCPG_HD inline uint64_t cooccur_key(uint32_t class_a, uint32_t class_b) {  // class_a != class_b
  const uint32_t lo = class_a < class_b ? class_a : class_b, hi = class_a < class_b ? class_b : class_a;
  return (((uint64_t)lo << 32) | hi) + 1;
}
KMCPG_HD inline uint32_t cooccur_key_a(uint64_t key) { return (uint32_t)((key - 1) >> 32); }
KMCPG_HD inline uint32_t cooccur_key_b(uint64_t key) { return (uint32_t)(key - 1); }

// ---- the table: open-addressed, `slots` a power of two; a key lives in one of the first cooccur_probes(slots) slots of its sequence
constexpr uint32_t K7_PROBES = 16;
KMCPG_HD inline uint32_t cooccur_probes(uint64_t slots) { return slots < K7_PROBES ? (uint32_t)slots : K7_PROBES; }
KMCPG_HD inline uint32_t cooccur_log2(uint64_t slots) {  // slots: a power of two
  uint32_t b = 0;
  while ((1ull << b) < slots) b++;
  return b;
}
// the first slot (Fibonacci hashing on the key's 64 bits) and the next one (linear: the probes of a key are distinct while probes <= slots)
KMCPG_HD inline uint64_t cooccur_slot0(uint64_t key, uint32_t log2_slots) { return log2_slots ? (key * 0x9E3779B97F4A7C15ull) >> (64 - log2_slots) : 0; }
KMCPG_HD inline uint64_t cooccur_next(uint64_t slot, uint64_t slots) { return (slot + 1) & (slots - 1); }

// The two phases, sequentially (the host's tables and the check; the device does the same with a 64-bit compare-and-swap and atomic loads).
// reserve: the key's slot, claimed if need be — idempotent; -1: none within the probes.  find: the slot of a key that was reserved; -1: none.
inline int64_t cooccur_reserve(uint64_t* keys, uint64_t slots, uint64_t key) {
  uint64_t i = cooccur_slot0(key, cooccur_log2(slots));
  for (uint32_t p = 0; p < cooccur_probes(slots); p++, i = cooccur_next(i, slots)) {
    if (keys[i] == COOCCUR_EMPTY) keys[i] = key;
    if (keys[i] == key) return (int64_t)i;
  }
  return -1;
}
inline int64_t cooccur_find(const uint64_t* keys, uint64_t slots, uint64_t key) {
  uint64_t i = cooccur_slot0(key, cooccur_log2(slots));
  for (uint32_t p = 0; p < cooccur_probes(slots); p++, i = cooccur_next(i, slots))
    if (keys[i] == key) return (int64_t)i;
  return -1;
}

// One query's targets (classes in any order, repeats allowed; the array is sorted in place): pair(key) for every unordered pair of distinct
// ones.  Returns the number of distinct targets.
template <class Pair>
inline size_t cooccur_query_pairs(uint32_t* cls, size_t n, Pair&& pair) {
  std::sort(cls, cls + n);
  const size_t m = (size_t)(std::unique(cls, cls + n) - cls);
  for (size_t i = 0; i + 1 < m; i++)
    for (size_t j = i + 1; j < m; j++) pair(cooccur_key(cls[i], cls[j]));
  return m;
}
// A read is counted completely or not at all: every pair reserves its slot first; only if all of them found one are the counts touched.
// Returns whether the read was counted (false: table full — the keys it did reserve stay with the count they had).
inline bool cooccur_count_read(uint64_t* keys, uint64_t* counts, uint64_t slots, uint32_t* cls, size_t n) {
  bool full = false;
  cooccur_query_pairs(cls, n, [&](uint64_t key) { full |= cooccur_reserve(keys, slots, key) < 0; });
  if (full) return false;
  cooccur_query_pairs(cls, n, [&](uint64_t key) { counts[cooccur_find(keys, slots, key)]++; });
  return true;
}

// ---- the row cuts of stage 2 on the TSV route.  Fed every row that passed -t / -f, in order:
//   target_kept  stage 1 kept the row's target (verdict ok)
//   new_name     the row's query name differs from that of the previous row that was NOT skipped (or there is none in this file)
// Returns whether the row's target joins the query's set; *opens: the row opens a query — the previous one is finished first.
struct CooccurCut {
  RefstatsCut cut;
  bool row(bool target_kept, bool new_name, double qcov, bool* opens) {
    *opens = false;
    if (!target_kept) return false;  // skipped: the caller does not take its name as the previous one either
    *opens = new_name;
    return cut.keep(new_name, qcov);
  }
};

}  // namespace kmcpg
