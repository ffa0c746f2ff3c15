// k2_plan.hpp — which COBS kernels (K2) a batch gets, decided once.  At open: k2_row_parts cuts a group's row into lane-form tiles
// (engine.cpp finish_open adds them as slots).  At every query: the shape of the batch and the knobs in; the planes, the rows per group,
// the chunking of long queries and the list of launches with their grids out.  query.cpp query_device_after builds the shape and fills
// K2Args from the plan; k2_cobs.hip launch_k2 / launch_k2_pair are switches over a launch record.  Host-only arithmetic in plain C++17
// (tests/k2_plan_check.cpp compiles it with g++).  The table of launches: DESIGN.md §4.
#pragma once
#include <stdint.h>

namespace kmcpg {

// ---- constants ---------------------------------------------------------------------------------------------------------------
constexpr uint64_t K2_MAX_BLOCKS = 1ull << 23;  // workgroups of one launch: x 256 threads = 2^31 (a launch holds fewer than 2^32 threads)
constexpr int K2_MAX_CLASSES = 5;               // lane forms: 4, 8, 16, 32, 64 lanes per row tile
constexpr int K2_MAX_LAUNCHES = 2 * K2_MAX_CLASSES;  // every class once for the short queries, once for the chunked long ones
// Counter planes by the largest NumKmers the plain kernel will meet: 8 for single short reads, 10 for pairs (2 x 150 bp = 260 k-mers, up
// to 2 x 500 bp), 16 for long reads, 24 above
// (one below the planes' range: the largest threshold a query of n k-mers can get is n + 1 — `-t 1`, or an FPR bound no count passes —
// and k2_cobs compares counts with it on NPL bits: n + 1 <= 2^NPL - 1 keeps that compare exact.  A threshold past the planes' range
// made the kernel's epilogue emit every column with a count above its low bits: filtered again by the host half, so no wrong
// match, but a hit list of the whole row for reads of exactly 255 / 1 023 k-mers at -t 1.)
constexpr uint64_t K2_MAX_N_8 = 254, K2_MAX_N_10 = 1022, K2_MAX_N_16 = 65534, K2_MAX_N_24 = 16777214;
// Rows gathered between two pruning tests.  4 instead of 8 saves 2.3 % of the row traffic (sectors are dropped ~2 rows sooner)
// for ~15 % more VALU work: a gain where the kernel waits for HBM (GTDB scale, 8 planes: 511 -> 488 ms per 524 k reads), a loss
// where it runs near its issue limits (16-plane kernels at 3 waves per SIMD: 248 -> 361 ms; indexes that half live in the
// Infinity Cache: 17.8 -> 19.6 ms) — profiles/r02_group_rows.txt.  4 rows from this many resident index bytes on:
constexpr uint64_t K2_GR4_MIN_BYTES = 4ull << 30;
// The read-back that lists the long queries costs a host round trip in the middle of the batch (~2.5 ms: more than the kernels of a
// batch of HiFi reads take).  It is only worth it when splitting could pay: a batch that fills the chip with its (query, slot) pairs
// anyway (more than K2_ASK_MAX_UNITS of them) and whose queries are bounded by K2_ASK_MAX_N k-mers (HiFi reads, contigs) runs the plain
// kernel on 16 planes without asking.
constexpr uint64_t K2_ASK_MAX_UNITS = 16384, K2_ASK_MAX_N = 32768;
// Splitting pays when the long queries alone would leave the chip idle (few (query, slot) pairs) or need more than 16
// counter planes; a batch of thousands of 10-kb reads already fills it and keeps the plain kernel (unless forced by env)
// (round 4, genome search with 3 hash functions, same-box A/B over batch sizes: from ~1 500 (query, slot) units on — 1.5 waves per SIMD — the
// plain kernel wins, because it prunes (a third of the row bytes are never fetched for 8 000-k-mer sketches at -t 0.4) and needs no atomics:
// 192 queries x 8 slots 5.0 vs 6.0 ms, 512 x 8 11.1 vs 16.3 ms; at 128 x 8 the chunked form still leads, 4.1 vs 4.5 ms.)
constexpr uint64_t K2_PLAIN_MIN_LONG_UNITS = 1536;
constexpr int32_t K2_SPLIT_MIN_DEFAULT = 2048;
// chunks of a long query: ~64 for the largest one, 1024..8192 k-mers each (at most 8192: the chunk's counts fit 16 planes)
constexpr int K2_CHUNK_MIN = 1024, K2_CHUNK_MAX = 8192, K2_CHUNKS_AIM = 64, K2_CHUNK_ENV_MIN = 64;  // (ENV_MIN: what KMCPG_SPLIT_CHUNK may ask for)
constexpr uint64_t K2_COUNTS_BYTES = 2ull << 30;  // count arrays of the long queries: at most ~2 GB at a time

// K2Args::k2_flags: the short-read unit (k2_short.hpp) and its two drivers read them — k2_cobs<64, 8|10, false, false, 4>
// (k2_cobs_body.inc, the SHORT branch) and k2_cobs_persist (k2_cobs.hip)
// one index phase per (read, run of tiles): `slots` is the class's block-unit list (Slot::tile carries the tile count)
constexpr int32_t K2F_BLOCK_UNITS = 1;
// every 128-byte sector steps by the rows its best column proves necessary and stops at its exact row
constexpr int32_t K2F_EXACT_STOP = 2;
// what a short-read batch gets without KMCPG_K2_BLOCK_UNITS / KMCPG_K2_EXACT_STOP in the environment
constexpr bool K2_BLOCK_UNITS_DEFAULT = false, K2_EXACT_STOP_DEFAULT = true;

// ---- at open: the lane forms of a row -------------------------------------------------------------------------------------------
struct K2OpenKnobs {
  bool lpr8 = true;      // KMCPG_LPR8=0: no 8-lane form, no 32-lane form
  bool lpr32 = true;     // KMCPG_LPR32=0: 257..512 bytes on the 64-lane form with half of its lanes idle, as before round 5
  int split_tiles = -1;  // KMCPG_SPLIT_TILES (1: multi-hash databases, 2: all; -1 = unset: the rule of k2_row_parts)
};

// lanes per row tile (16 B each): the narrowest form that covers the row, so that no lane of a wave idles (a 128-byte row on the
// 16-lane form left half of every wave without a row to load)
inline int lpr_for_stride(uint32_t stride, const K2OpenKnobs& kn) {
  if (!kn.lpr8) return stride <= 64 ? 4 : (stride <= 256 ? 16 : 64);
  // 257..512 bytes: the 32-lane form, two units per wave
  return stride <= 64 ? 4 : (stride <= 128 ? 8 : (stride <= 256 ? 16 : (stride <= 512 && kn.lpr32 ? 32 : 64)));
}

struct K2RowPart {
  int lpr;
  uint32_t byte0;  // first byte of the tile in the row: a multiple of lpr * 16
};
struct K2RowParts {
  uint32_t full = 0;  // whole 1-KiB tiles: part t < full is {64, t * 1024}
  int n_rem = 0;      // ... then the remainder's tiles
  K2RowPart rem[4];
  uint32_t size() const { return full + (uint32_t)n_rem; }
  K2RowPart operator[](uint32_t i) const { return i < full ? K2RowPart{64, i * 1024u} : rem[i - full]; }
};

// whole 1-KB tiles go to full waves (64 lanes x 16 B); what is left of the row to the narrowest lane group that covers it
inline K2RowParts k2_row_parts(uint32_t stride, int num_hashes, const K2OpenKnobs& kn) {
  K2RowParts p;
  p.full = stride / 1024u;
  const uint32_t rem = stride % 1024u;
  // EXPERIMENT, off (KMCPG_SPLIT_TILES=1: multi-hash databases, 2: all): a remainder of 257..896 bytes on the 64-lane form leaves
  // 8..47 lanes of every wave without a row to load; cut into power-of-two tiles that fill their waves — 832 = 512 (32 lanes, two
  // units per wave) + 256 (16 lanes) + 64 (4 lanes), each aligned to its own tile size — the genome search's K2 took 9.35 ms instead
  // of 4.9 ms (same bytes moved): three launches read the hashes and compute the row indices three times, and the narrow parts run
  // on the fabric's request rate.  The idle lanes were never the cost (profiles/r05_split_tiles.txt).
  // Round 6 (profiles/r06_lpr_640.txt, single-hash index, short reads, 23-27 GB): a remainder of 640 bytes as 512 (32-lane form) + 128
  // (8-lane form) is 11-17 % faster than one 64-lane tile with 40 lanes busy (385 -> 329-347 ms per 1 M reads) and is now what a
  // single-hash database gets; 576 = 512 + 64 gains 4.6 % and 768 = 512 + 256 gains 6.8 %: below the 10 % bar, left as one tile.
  const int st = kn.split_tiles;
  const bool split = rem > 256 && rem <= 896 && __builtin_popcount(rem / 64u) <= 3 &&
                     (st == 2 || (st == 1 && num_hashes > 1) || (st < 0 && rem == 640 && num_hashes == 1));
  if (rem && split) {
    uint32_t at = p.full * 1024u, left = rem;
    for (uint32_t part = 512; part >= 64 && left; part >>= 1)
      if (left >= part) {
        p.rem[p.n_rem++] = K2RowPart{(int)(part / 16u), at};
        at += part;
        left -= part;
      }
  } else if (rem) {
    p.rem[p.n_rem++] = K2RowPart{lpr_for_stride(rem, kn), p.full * 1024u};
  }
  return p;
}

// ---- at every query ------------------------------------------------------------------------------------------------------------
struct K2Knobs {
  int32_t split_min = K2_SPLIT_MIN_DEFAULT;  // KMCPG_SPLIT_MIN: queries with more k-mers may take the chunked form; 0 = none does
  bool split_min_set = false;                // ... and its presence: the chunked form for every long query, whatever the batch
  int split_chunk = 0;                       // KMCPG_SPLIT_CHUNK: k-mers per chunk (clamped to 64..8192)
  bool split_chunk_set = false;
  int nt_loads = 1;     // KMCPG_NT_LOADS
  int prune = 1;        // KMCPG_PRUNE
  int group_rows = 0;   // KMCPG_GROUP_ROWS: 4 = four rows, anything else eight
  bool group_rows_set = false;
  int prune_every = 1;  // KMCPG_PRUNE_EVERY: 2, 4 or 8; anything else 1
  int slot_major = 1;   // KMCPG_SLOT_MAJOR
  int tail_sectors = 2, tail_min = 64;  // KMCPG_TAIL_SECTORS (0..4), KMCPG_TAIL_MIN (>= 1)
  bool pair = true;     // KMCPG_PAIR
  bool block_units = K2_BLOCK_UNITS_DEFAULT, exact_stop = K2_EXACT_STOP_DEFAULT;  // KMCPG_K2_BLOCK_UNITS, KMCPG_K2_EXACT_STOP
  bool persist = true;       // KMCPG_K2_PERSIST=0: the short-read launch as launched waves, one unit each
  uint32_t persist_wgs = 0;  // KMCPG_K2_PERSIST_WGS: the persistent kernel's grid, for tests; 0 = what the chip holds at once
};

struct K2Class {  // a lane class of the database (engine.hpp SlotClass)
  int lpr = 0;
  uint32_t nslots = 0;
  uint32_t nbslots = 0;  // its block-unit list; 0: the class has none
};

// everything the choice depends on
struct K2Shape {
  uint32_t n_reads = 0;
  uint64_t max_n = 0;  // no query has more k-mers
  int num_hashes = 1;
  uint64_t matrix_bytes_local = 0;
  uint64_t n_cols = 0;
  int n_classes = 0;
  K2Class classes[K2_MAX_CLASSES];
  K2Knobs knobs;
};

enum class K2Kind : int { Plain = 0, Split = 1, Pair = 2 };  // the numbers of the witness (kmcpg_k2_launch::kind)

struct K2Launch {
  K2Kind kind = K2Kind::Plain;
  int lpr = 0, lprb = 0;  // lprb: the second half of a pair
  int npl = 0;
  bool multi = false;
  int gr = 8;             // rows per group of the kernel that runs: 4 only at 8 / 10 planes
  int cls = 0, cls_b = 0; // whose slots (cls_b: the second half of a pair)
  bool block_units = false;  // the class's block-unit list instead of its slots
  int32_t k2_flags = 0;
  bool persist = false;      // k2_cobs_persist instead of k2_cobs: resident waves take the launch's units from a queue (k2_claim.hpp)
  uint64_t units = 0;        // Split: 0 here, k2_split_launch gives it per group of long queries
  uint32_t nba = 0, nbb = 0; // Pair: workgroups of the two halves, one grid of nba + nbb
};

struct K2Piece {
  uint64_t unit_base;
  unsigned workgroups;
};

struct K2Plan {
  uint32_t n_long = 0;     // queries on the chunked form
  uint64_t max_short = 0;  // largest NumKmers the plain kernel will meet
  int npl = 0;             // 0: more k-mers than 24 planes count (unsupported)
  int group_rows = 8, prune_every = 1;
  int32_t split_min = 0;   // as the kernels get it: 0 without chunked queries
  uint32_t split_chk = 0, split_chunks = 0;  // chunked form: k-mers per chunk, chunks of the largest query
  uint32_t group = 0;      // ... and long queries per count array
  int n_launches = 0;      // plain launches or the pair first, then the chunked form's (once: the caller repeats those per count array)
  K2Launch launches[K2_MAX_LAUNCHES];
};

// a wave carries G = 64 / lpr units, a workgroup four waves
inline uint64_t k2_workgroups(uint64_t units, int lpr) {
  const uint64_t G = 64 / (uint64_t)lpr;
  return ((units + G - 1) / G + 3) / 4;
}
// units of (n, nslots): with slot_major == 2 the slots of a read are rounded up to whole waves
inline uint64_t k2_units(uint64_t n, uint32_t nslots, int lpr, int slot_major) {
  const uint64_t G = 64 / (uint64_t)lpr;
  return (G > 1 && slot_major == 2) ? n * (((uint64_t)nslots + G - 1) / G) * G : n * nslots;
}
// the grid of a plain or chunked launch: pieces of at most K2_MAX_BLOCKS workgroups, piece i from unit i * K2_MAX_BLOCKS * 4 * G on
inline uint64_t k2_n_pieces(const K2Launch& l) { return (k2_workgroups(l.units, l.lpr) + K2_MAX_BLOCKS - 1) / K2_MAX_BLOCKS; }
inline K2Piece k2_piece(const K2Launch& l, uint64_t i) {
  const uint64_t blocks = k2_workgroups(l.units, l.lpr), b0 = i * K2_MAX_BLOCKS;
  return K2Piece{b0 * 4 * (64 / (uint64_t)l.lpr), (unsigned)(blocks - b0 < K2_MAX_BLOCKS ? blocks - b0 : K2_MAX_BLOCKS)};
}
// a chunked launch of the plan for one count array's n_long queries: a unit is (long query, slot, chunk)
inline K2Launch k2_split_launch(const K2Plan& p, const K2Shape& s, const K2Launch& l, uint32_t n_long) {
  K2Launch r = l;
  r.units = (uint64_t)n_long * s.classes[l.cls].nslots * p.split_chunks;
  return r;
}

inline uint64_t k2_total_slots(const K2Shape& s) {
  uint64_t t = 0;
  for (int i = 0; i < s.n_classes; i++) t += s.classes[i].nslots;
  return t;
}

// Long queries (whole genomes, -g) are split into chunks of k-mers so that they spread over the chip; short ones keep the
// one-wave-per-(query, slot) kernel.  Which queries are long is only known on the device: whether to ask (one small D2H read).
inline bool k2_ask_long(const K2Shape& s) {
  const int32_t split_min = s.knobs.split_min;
  return split_min > 0 && s.max_n > (uint64_t)split_min &&
         (s.knobs.split_min_set || s.max_n > K2_ASK_MAX_N || (uint64_t)s.n_reads * k2_total_slots(s) <= K2_ASK_MAX_UNITS);
}

// asked: k2_ask_long said so, and the device listed n_long_listed queries above split_min, the largest of max_long k-mers
inline K2Plan k2_plan(const K2Shape& s, bool asked, uint32_t n_long_listed, uint32_t max_long) {
  K2Plan p;
  const K2Knobs& kn = s.knobs;
  p.n_long = asked ? n_long_listed : 0;
  if (p.n_long && !kn.split_min_set && (uint64_t)p.n_long * k2_total_slots(s) >= K2_PLAIN_MIN_LONG_UNITS && max_long <= K2_MAX_N_16) p.n_long = 0;
  // bounded by the read length, and exactly known once the long ones were listed
  p.max_short = s.max_n;
  if (asked) p.max_short = p.n_long ? (uint64_t)kn.split_min : (max_long > (uint64_t)kn.split_min ? max_long : (uint64_t)kn.split_min);
  p.npl = p.max_short <= K2_MAX_N_8 ? 8 : (p.max_short <= K2_MAX_N_10 ? 10 : (p.max_short <= K2_MAX_N_16 ? 16 : (p.max_short <= K2_MAX_N_24 ? 24 : 0)));
  if (!p.npl) return p;
  p.group_rows = (kn.prune && p.npl <= 10 && s.matrix_bytes_local >= K2_GR4_MIN_BYTES) ? 4 : 8;
  if (kn.group_rows_set) p.group_rows = kn.group_rows == 4 ? 4 : 8;
  // How often the test runs in the 8/10-plane kernels: after every group (they wait for HBM; KMCPG_PRUNE_EVERY = 2/4/8 for experiments).
  // The 16/24-plane kernels resolve their carries every 32 rows and test there (k2_cobs.hip): the test was a quarter of their VALU
  // work at one test per group, and they run near their issue limits — same-box A/B tools/ab/r04_call13.sh: equal-width HiFi index
  // 3.88 -> 3.55 ms per 16 384 reads, genome search 5.73 -> 5.48 ms per 256 genomes with a test every 4th group alone.
  p.prune_every = (kn.prune_every == 2 || kn.prune_every == 4 || kn.prune_every == 8) ? kn.prune_every : 1;
  p.split_min = p.n_long ? kn.split_min : 0;
  const bool multi = s.num_hashes > 1;
  const int gr = (p.npl <= 10 && p.group_rows == 4) ? 4 : 8;  // there are no 4-row kernels at 16 / 24 planes
  // Long queries on rows cut into a 64-lane tile form + one narrower form: both in one grid (k2_cobs_pair: the second form's workgroups
  // take the slots the first one's last waves free; KMCPG_PAIR=0: two launches, as before round 6).  The kernel exists at 16 planes and
  // 8 rows, for two non-empty halves that fit one grid.
  bool paired = false;
  if (p.npl == 16 && p.group_rows != 4 && s.n_classes == 2 && s.classes[0].lpr == 64 && s.classes[1].lpr < 64 && kn.pair) {
    const K2Class &ca = s.classes[0], &cb = s.classes[1];
    const uint64_t ua = k2_units(s.n_reads, ca.nslots, 64, kn.slot_major), ub = k2_units(s.n_reads, cb.nslots, cb.lpr, kn.slot_major);
    const uint64_t nba = k2_workgroups(ua, 64), nbb = k2_workgroups(ub, cb.lpr);
    if (nba != 0 && nbb != 0 && nba + nbb <= K2_MAX_BLOCKS) {
      K2Launch& l = p.launches[p.n_launches++];
      l.kind = K2Kind::Pair;
      l.lpr = 64;
      l.lprb = cb.lpr;
      l.npl = 16;
      l.multi = multi;
      l.cls_b = 1;
      l.units = ua + ub;
      l.nba = (uint32_t)nba;
      l.nbb = (uint32_t)nbb;
      paired = true;
    }
  }
  // The short-read unit (k2_short.hpp) in k2_cobs<64, 8|10, false, false, 4>: KMCPG_K2_BLOCK_UNITS=1 — one index phase per (read, block
  // group), the tiles of the row one after the other in one wave; KMCPG_K2_EXACT_STOP=1 — every sector steps by the rows its best column
  // proves necessary and stops at its exact row.  Defaults: DESIGN.md §4 (profiles/k2_exact_stop_ab.txt).
  int32_t short_flags = 0;
  if (p.npl <= 10 && p.group_rows == 4 && s.num_hashes == 1 && kn.prune && p.prune_every == 1)
    short_flags = (kn.block_units ? K2F_BLOCK_UNITS : 0) | (kn.exact_stop ? K2F_EXACT_STOP : 0);
  for (int c = 0; c < s.n_classes && !paired; c++) {
    const K2Class& k = s.classes[c];
    K2Launch& l = p.launches[p.n_launches++];
    l.lpr = k.lpr;
    l.npl = p.npl;
    l.multi = multi;
    l.gr = gr;
    l.cls = c;
    l.k2_flags = k.lpr == 64 ? short_flags : 0;
    l.block_units = (l.k2_flags & K2F_BLOCK_UNITS) && k.nbslots;
    if (!l.block_units) l.k2_flags &= ~K2F_BLOCK_UNITS;  // a class without the list: tile by tile
    l.units = k2_units(s.n_reads, l.block_units ? k.nbslots : k.nslots, k.lpr, kn.slot_major);
    // the short-read unit tile by tile on a 1-KiB tile form: the persistent kernel (there are two, k2_cobs_persist<8|10>)
    l.persist = kn.persist && k.lpr == 64 && l.gr == 4 && l.npl <= 10 && !l.multi && l.k2_flags != 0 && !(l.k2_flags & K2F_BLOCK_UNITS);
  }
  if (p.n_long) {
    int chk = K2_CHUNK_MIN;
    while (chk < K2_CHUNK_MAX && (uint64_t)chk * K2_CHUNKS_AIM < max_long) chk <<= 1;
    if (kn.split_chunk_set) chk = kn.split_chunk < K2_CHUNK_ENV_MIN ? K2_CHUNK_ENV_MIN : (kn.split_chunk > K2_CHUNK_MAX ? K2_CHUNK_MAX : kn.split_chunk);
    p.split_chk = (uint32_t)chk;
    p.split_chunks = (max_long + p.split_chk - 1) / p.split_chk;
    const uint64_t row = (uint64_t)(uint32_t)s.n_cols * 4;  // the counts of one long query
    p.group = row && row <= K2_COUNTS_BYTES ? (uint32_t)(K2_COUNTS_BYTES / row) : 1;
    for (int c = 0; c < s.n_classes; c++) {
      K2Launch& l = p.launches[p.n_launches++];
      l.kind = K2Kind::Split;
      l.lpr = s.classes[c].lpr;
      l.npl = 16;
      l.multi = multi;
      l.cls = c;
    }
  }
  return p;
}

}  // namespace kmcpg
