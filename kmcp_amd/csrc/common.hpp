// common.hpp — structures shared by the host engine and the HIP kernels of libkmcpgpu.so.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/kmcp_gpu.h"

namespace kmcpg {

// Device-side description of resident index rows (index/serialization.go:66-82 Header, re-laid-out: rows padded to `stride`
// bytes, one all-zero row appended at index num_sigs).  Two arrays of these live on the device:
//  - one entry per resident .uniki block (used by the planting / read-back helpers): `rows` points at the block's first byte
//    inside its group's rows, ncols/col_base are the block's own;
//  - one entry per GROUP (used by K2): resident blocks with the same NumSigs are laid side by side in one row — a k-mer's row
//    index h % NumSigs is the same in all of them, so one wide gather serves them all (the on-disk format is untouched).
//    row_bytes is the sum of the members' NumRowBytes; segs[seg0 .. seg0+nsegs) map a byte of the row back to columns.
struct BlockDev {
  const uint8_t* rows;  // device pointer, (num_sigs + 1) * stride bytes
  uint64_t num_sigs;    // Header.NumSigs: modulus of the row address (util-db-search.go:6811)
  uint64_t magic_hi;    // fastmod_magic(num_sigs): exact h % num_sigs with one 64-bit high multiply (fastmod.hpp; replaces fastdiv, :6611)
  uint32_t stride;      // bytes per row in HBM (multiple of 16)
  uint32_t row_bytes;   // Header.NumRowBytes = (ncols+7)/8 (group: sum over the members)
  uint32_t ncols;
  uint32_t col_base;    // global column id of column 0 (group: of the first member)
  uint32_t seg0, nsegs; // group entries: its members in the segment table
};

// One member block of a group: bytes [byte_start, byte_end) of the group's row hold its columns, MSB of a byte first
// (index.go:1157); the last byte may carry padding bits (always zero).
struct Seg {
  uint32_t byte_start, byte_end;
  uint32_t col_base;  // global column id of the member's column 0
  uint32_t ncols;
};

// 2-bit packed upload of a batch's bases (lane.cpp stage / support.hip k_unpack2): a run of bytes that are not A/C/G/T/U in either
// case, restored after unpacking (positions in bases from the start of the batch)
struct ExcRun {
  uint64_t pos;
  uint32_t len;
  uint32_t byte;
};

// One unit of COBS work per read: (local block, tile of LPR*16 bytes of the row).
// Block units (K2F_BLOCK_UNITS, the 64-lane class of short-read batches): a unit is (read, run of tiles of one group's rows), `tile` =
// first tile | number of tiles << 24.
struct Slot {
  uint32_t block;  // index into the group array
  uint32_t tile;
};
constexpr uint32_t SLOT_TILE_BITS = 24, SLOT_MAX_TILES = 255;

struct K1Args {
  const uint8_t* seqs;
  const uint64_t* offs;
  const uint8_t* seqs2;  // mates or nullptr
  const uint64_t* offs2;
  uint32_t n_reads;
  int32_t k;
  int32_t min_qlen;
  int32_t scaled;
  uint64_t max_hash;
  int32_t mode;          // 0 plain (+scaled), 1 minimizer, 2 syncmer
  uint32_t w_or_s;       // minimizer-w or syncmer-s
  uint64_t* hashes;      // read i writes at hashes[offs[i] + offs2[i] ...]
  uint64_t* scratch;     // same size as hashes: k-mer hashes of window sketches / dedup output
  uint64_t* scratch2;    // same size: s-mer hashes (syncmer mode)
  int32_t* nk_raw;       // k-mers emitted for read i (both mates)
  int32_t* nk1;          // k-mers emitted for mate 1 (for --try-se)
  int32_t* qlen;
  // K1's side buffer (K1Plan's regions; query.cpp run_kmers places all four, nullptr where the plan has none)
  int32_t* seg_cnt;      // whole genomes: kept hashes per (read, segment), n_reads * segs_max entries
  uint32_t segs_max;
  // window sketches of long reads (k1_kmers_wg<1|2>): emissions without adjacent repeats go to scratch[], their number here
  // (queries above max(dedup_threshold, 512) emissions; the others keep their raw emissions in hashes[]); nullptr = raw only
  int32_t* nk_adj;
  int32_t dedup_threshold;
  int32_t flags;         // experiments (KMCPG_K1_FLAGS, the K1F_ bits of k1_plan.hpp)
  // the list a kernel leaves to the one launched behind it, and its length: whole genomes — the (read, segment) numbers k1_seg_roll2 could
  // not take (seg_cnt == -1), for k1_seg_roll; closed syncmers of long reads — the reads k1_windows_roll could not take, for k1_windows_wave
  uint32_t* seg_list;
  uint32_t* seg_nflag;
  int32_t seg_only_flagged;  // k1_seg_roll / k1_windows_wave as that second kernel: a small grid walks the list (0: the whole batch, no list)
  // whole genomes that arrived as 2-bit codes (kmcpg_submit_packed / a batch stage() packed): k1_seg_roll2 takes its codes from the packed
  // stream as it is — base j of the batch in bits 2 (j % 4) of byte j / 4 — and only the segments a run of foreign bytes reaches are expanded
  // to text (seqs_w = the buffer `seqs` points at) for the byte kernel.  nullptr: `seqs` holds the text already.
  const uint8_t* codes;
  const ExcRun* exc;
  uint32_t n_exc;
  uint8_t* seqs_w;
  uint32_t* seg_exc;     // per (read, segment): != 0 when a foreign byte lies among the bases the segment's k-mers cover (k_mark_exc)
  // sliding windows (kmcpg_submit_windows): query r is a view of src[r] .. src[r] + offs[r+1] - offs[r] of `seqs` — the bases of the reads are
  // on the device once, offs numbers the windows' bases (hash output, lengths).  nullptr: query r is seqs[offs[r] ...] itself.
  const uint64_t* src;
};


// the packed source of a batch (DeviceBatch::packed, engine.hpp): codes + runs on the device, and the text buffer the expansion goes to
// when the k-mer kernels of this batch read text.  codes == nullptr: the batch is text already.
struct PackedSrc {
  const uint8_t* codes = nullptr;
  const ExcRun* exc = nullptr;
  uint32_t n_exc = 0;
  uint8_t* text = nullptr;
  uint64_t n_bases = 0;
};
// the windows of a batch (DeviceBatch::windows): src = each window's first base in the staged text (K1Args::src), and the staged slices of
// reads with their prefix sums (windows.hip) for the hash-once form of plain / FracMinHash k-mers.  src == nullptr: no window view.
constexpr int K1_WIN_CHUNK = 1024;  // k-mer positions of a slice one wave hashes (hash-once form)
struct WindowSrc {
  const uint64_t* src = nullptr;   // [n windows]
  const uint64_t* soffs = nullptr; // [ns + 1] the slices' bases in the staged text
  const uint64_t* wpre = nullptr;  // [ns + 1] windows of slices 0 .. q-1
  const uint64_t* cpre = nullptr;  // [ns + 1] chunks of K1_WIN_CHUNK k-mer positions of slices 0 .. q-1 (for the database's k)
  uint32_t ns = 0;
  uint64_t n_chunks = 0, sb = 0, step = 0, window = 0;
};

struct DedupArgs {
  const uint64_t* offs;
  const uint64_t* offs2;
  uint32_t n_reads;
  int32_t dedup_threshold;
  int32_t min_matched;
  int32_t lo, hi;        // this workgroup-class launch sorts queries with lo < m <= hi elements (m: after k_adj_unique)
  int32_t n_lo, n_hi;    // ... among those whose raw count n is in (n_lo, n_hi]
  int32_t pre;           // window-sketch database: k_adj_unique runs first (input of the sort = scratch, m in nk_search)
  int32_t pre_done;      // ... and the k-mer kernel has already done it (k1_kmers_wg<1|2>: fused)
  int32_t key_shift;     // leading zero bits of the largest possible hash (0, or clz(maxHash) for FracMinHash databases): k_dedup_bucket
  uint64_t* hashes;
  uint64_t* scratch;
  const int32_t* nk_raw;
  int32_t* nk_search;    // NumKmers after dedup, 0 if the read is not searched
  uint32_t* fallbacks;   // profiling only (else nullptr): k_dedup_bucket counts the queries that took its bitonic fallback here
};

constexpr int K2_GATHER_SLOTS = 256;

struct K2Args {
  const BlockDev* blocks;  // groups
  const Seg* segs;
  const Slot* slots;
  uint32_t nslots;
  uint32_t n_reads;
  const uint64_t* hashes;
  const uint64_t* offs;
  const uint64_t* offs2;
  const int32_t* nk;     // nk_search
  double min_qcov;
  int32_t min_matched;
  int32_t num_hashes;
  int32_t nt_loads;      // non-temporal row loads
  int32_t prune;         // stop loading sectors whose columns can no longer reach the threshold
  int32_t group_rows;    // rows gathered between two pruning tests: 4 or 8
  int32_t prune_every;   // the pruning test runs after every prune_every-th row group (1, 2, 4 or 8) and at the end of a chunk of 64 rows
  int32_t split_min;     // >0: queries with more k-mers are handled by the SPLIT launch
  int32_t slot_major;    // unit order: 1 = slot-major (unit u -> slot u / n_reads, read u % n_reads), 0 = read-major
  int32_t tail_sectors;  // long queries on 1-KiB tiles: with at most this many live sectors (<= 4; 0 = never) and
  int32_t tail_min;      // ... at least this many k-mers to go a wave finishes in tail mode (k2_cobs.hip)
  // long-query (SPLIT) form
  const uint32_t* long_list;  // indices of the long queries
  uint32_t n_long;
  uint32_t split_chk;         // k-mers per chunk (<= 8192: 16 counter planes)
  uint32_t split_chunks;      // chunks per long query (from the largest one)
  uint32_t* long_counts;      // [n_long][ncols_total] match counts
  uint32_t ncols_total;
  uint64_t unit_base;     // first work unit of this launch (a batch may take several launches)
  kmcpg_hit* hits;
  uint64_t hit_cap;
  unsigned long long* counter;
  unsigned long long* gathered;  // optional (profiling level 2): 16-byte row loads issued, K2_GATHER_SLOTS counters 128 B apart
  const uint16_t* cmin_fpr;      // optional: [n] = smallest count whose FPR(n, count) passes -f, n <= cmin_fpr_n (query.cpp fpr_bound)
  int32_t cmin_fpr_n;
  int32_t k2_flags;              // K2F_ bits (k2_plan.hpp): the short-read unit's (k2_short.hpp; k2_cobs<64, 8|10, false, false, 4> and k2_cobs_persist drive it)
  // a launch record with `persist` set (k2_plan.hpp; k2_cobs.hip k2_cobs_persist): resident waves take their units from a queue
  unsigned long long* unit_queue;  // one zeroed counter per launch piece, K2_QUEUE_PITCH words apart (k2_claim.hpp); nullptr: the plan has no such record
  uint32_t persist_wgs;            // its grid; 0: as many workgroups as the chip holds at once (K2Knobs::persist_wgs, for tests)
};
constexpr int K2_QUEUE_PITCH = 16;  // 128 bytes: the pieces' counters do not share a cache line
static_assert(sizeof(K2Args) == 224 && offsetof(K2Args, unit_queue) == 208, "new fields go behind k2_flags: what the other K2 forms read keeps its place in the argument block");

// K3 (k3_finalize.hip): hit list -> per-read segments of (column, count), filtered by -T, ordered as the reference orders a
// query's matches.  Segments of more than K3_WG_CAP matches are grouped but left unordered (the host sorts those).
constexpr int K3_WAVE_CAP = 512, K3_WG_CAP = 4096;
struct K3Args {
  const kmcpg_hit* hits;
  const unsigned long long* n_hits;  // device word: hits produced (may exceed hit_cap: then only hit_cap are there)
  uint64_t hit_cap;
  const int32_t* nk;        // NumKmers per read
  uint32_t n_reads;
  uint32_t n_cols;
  const uint64_t* col_size; // Header.Sizes per global column
  double min_tcov;          // -T
  int32_t sort_mode;        // 0 qcov, 1 tcov, 2 jacc (-s), 3 column order (-S)
  uint32_t* cnt;            // [n_reads + 1], zero on entry and on exit
  uint64_t* offs;           // [n_reads + 1] out: CSR offsets of the reads' segments
  uint64_t* sums;           // scan scratch, one word per 4096 reads
  kmcpg_pair* pairs;        // out: offs[n_reads] pairs
  uint32_t* bad;            // hits naming a read / column that does not exist (an internal error: the caller reports it)
};

// Database sets (kmcpg_open_set): what the sort kernels of a set handle get beside K3Args (k3_set_order.hpp; layout at the top of
// k3_finalize.hip).  stats: four device words the kernels add to — segments sorted by the wave class (2 .. K3_WAVE_CAP matches), by the
// workgroup class (.. K3_WG_CAP), segments left to the host (longer), runs of equal fixed4 holding more than one member.
constexpr int K3_SET_STATS = 4;
struct K3SetArgs {
  uint32_t n_members;   // 2 .. 16
  uint32_t base[16];    // first global column of every member, ascending
  uint32_t* stats;
};

// K4 (k4_specific.hip): K3's segments -> a verdict per read and the surviving segments, compacted.  The rule: specific_rule.hpp.
constexpr uint8_t K4_DROP = 0, K4_KEEP = 1, K4_HOST = 2;  // = KMCPG_SPECIFIC_* (include/kmcp_gpu.h)
constexpr int K4_STATS = 6;  // reads kept / dropped / left to the host (of those with pairs), lane-group / wave segments, segments outside the buffer
struct K4Args {
  const kmcpg_pair* pairs;       // K3's output
  const uint64_t* offs;          // [n_reads + 1]
  uint64_t pair_cap;             // pairs there is room for behind `pairs`: a segment that ends behind it is treated as empty
  const int32_t* nk;             // NumKmers per read
  uint32_t n_reads;
  uint32_t n_cols;
  int32_t final_n;               // reads of more k-mers are left to the host (their pairs may still fall to -f there)
  const uint32_t* target_class;  // [n_cols]
  const uint32_t* species_class; // [n_cols] or nullptr: strain / assembly level
  uint32_t* cnt;                 // [n_reads + 1] scratch: kept lengths
  uint64_t* sums;                // scan scratch, one word per 4096 reads
  uint8_t* verdict;              // out [n_reads]
  kmcpg_pair* out_pairs;         // out: out_offs[n_reads] pairs
  uint64_t* out_offs;            // out [n_reads + 1]
  uint64_t out_cap;
  uint32_t* stats;               // [K4_STATS], zero on entry
};

// K5 (k5_summary.hip): K4's surviving segments -> one 16-byte summary per window (regions_rule.hpp); the segments it cannot summarise
// exactly are LEFT to the host and compacted.
constexpr uint32_t K5_CAP = 64;  // longest segment of several targets the device summarises
constexpr int K5_STATS = 5;      // windows single-target / by the wave / LEFT / empty or dropped, segments outside the buffer
struct K5Args {
  const kmcpg_pair* pairs;       // K4's output: the surviving segments in print order
  const uint64_t* offs;          // [n_reads + 1]
  uint64_t pair_cap;             // pairs there is room for behind `pairs`: a segment that ends behind it is treated as empty
  const uint8_t* verdict;        // [n_reads] K4's bytes: DROP = no rows, HOST = LEFT
  const int32_t* nk;             // NumKmers per window
  uint32_t n_reads;
  uint32_t n_cols;
  const uint32_t* target_class;  // [n_cols]
  kmcpg_window_summary* out;     // out [n_reads]
  uint32_t* cnt;                 // [n_reads + 1] scratch: the LEFT lengths
  uint64_t* sums;                // scan scratch, one word per 4096 windows
  kmcpg_pair* left_pairs;        // out: left_offs[n_reads] pairs
  uint64_t* left_offs;           // out [n_reads + 1]
  uint64_t left_cap;
  uint32_t* stats;               // [K5_STATS], zero on entry
};

// K10 (k10_left.hip): the bytes the counting stages (K6, K7, K8) wrote for the reads they LEFT -> one mask byte per read (bit s: stage s
// left it) and the length of every LEFT read's segment in K3's output; the scan and k4_compact behind it bring those segments together.
// The witness: reads with at least one pair, LEFT reads, their pairs, segments outside the buffer, launches the overflow guard skipped
enum { K10_MATCHED = 0, K10_LEFT, K10_LEFT_PAIRS, K10_BAD, K10_SKIPPED, K10_STATS };
constexpr int K10_STAGES = 3;  // K6, K7, K8 in the order of engine.hpp
struct K10Args {
  const uint64_t* offs;                // K3's offsets [n_reads + 1]
  uint64_t pair_cap;                   // pairs there is room for in K3's output: a segment that ends behind it is treated as empty
  uint32_t n_reads;
  const uint8_t* left[K10_STAGES];     // [n_reads] each, or nullptr: the stage is not looked at
  const unsigned long long* n_hits;    // device word or nullptr: the batch's hit counter ...
  uint64_t hit_cap;                    // ... above this the batch will be run again: nothing is written now
  uint8_t* mask;                       // out [n_reads]
  uint32_t* cnt;                       // [n_reads + 1] scratch: the LEFT lengths (all 0 where the guard skipped the launch)
  unsigned long long* stats;           // [K10_STATS], zero on entry
};

// K11 (k11_bin.hip): K3's segments -> one word per read, the TaxId of the read's bin (bin_rule.hpp): the lowest common ancestor, in the
// pruned tree of the plan, of the whitelisted targets the read matches.
constexpr uint32_t K11_NONE = 0xffffffffu, K11_LEFT = 0xfffffffeu;  // = KMCPG_BIN_NONE, KMCPG_BIN_LEFT (include/kmcp_gpu.h), BIN_* (bin_rule.hpp)
constexpr uint32_t K11_LDS_NODES = 2048;  // the plan's three tables sit in LDS up to this many nodes (24 KiB per workgroup)
// the witness: reads without a bin / with one target / with several / LEFT, climb steps, segments outside the buffer, launches the overflow
// guard skipped
enum { K11_NO_BIN = 0, K11_ONE, K11_SEVERAL, K11_LEFT_READS, K11_STEPS, K11_BAD, K11_SKIPPED, K11_STATS };
struct K11Args {
  const kmcpg_pair* pairs;             // K3's output
  const uint64_t* offs;                // [n_reads + 1]
  uint64_t pair_cap;                   // pairs there is room for behind `pairs`: a segment that ends behind it is treated as empty
  const int32_t* nk;                   // NumKmers per read
  uint32_t n_reads;
  uint32_t n_cols;
  int32_t final_n;                     // reads of more k-mers are LEFT (their pairs may still fall to -f on the host), as in K4
  const uint32_t* node_of_column;      // [n_cols]: the pre-order number of the column's target, NO_CLASS = not whitelisted
  const uint32_t *parent, *last, *taxid;  // [n_nodes] the plan's tables; node 0 is the virtual root
  uint32_t n_nodes;
  const unsigned long long* n_hits;    // device word or nullptr: the batch's hit counter ...
  uint64_t hit_cap;                    // ... above this the batch will be run again: nothing is written now
  uint32_t* bins;                      // out [n_reads]: a TaxId, K11_NONE or K11_LEFT
  uint8_t* left;                       // out [n_reads] or nullptr: 1 where the bin is K11_LEFT, else 0 (the byte K10's compaction takes)
  unsigned long long* stats;           // [K11_STATS], zero on entry
};

// K6 (k6_refstats.hip): K3's segments -> four counters per column, the counts of stage 1 of `kmcp profile` (refstats_rule.hpp); the reads
// it cannot count exactly are LEFT to the host (a byte per read).
constexpr uint32_t K6_CAP = 64;  // longest segment of several targets the device counts
constexpr uint32_t K6_MAX_SLOTS = 2048, K6_DEFAULT_SLOTS = 1024, K6_PROBES = 8;  // the workgroup's table in LDS: 20 bytes per slot
// the witness: reads empty / single target / by the wave / LEFT, adds to LDS / to global memory (flushes and spills) / of those the spills,
// launches the overflow guard skipped, segments outside the buffer; then the three totals that persist beside the counters
enum { K6_EMPTY = 0, K6_SINGLE, K6_WAVE, K6_LEFT, K6_LDS_ADDS, K6_GLOBAL_ADDS, K6_SPILLED, K6_SKIPPED, K6_BAD, K6_STATS };
struct K6Args {
  const kmcpg_pair* pairs;             // K3's output, in print order
  const uint64_t* offs;                // [n_reads + 1]
  uint64_t pair_cap;                   // pairs there is room for behind `pairs`: a segment that ends behind it is treated as empty
  const int32_t* nk;                   // NumKmers per read
  uint32_t n_reads;
  uint32_t n_cols;
  int32_t final_n;                     // reads of more k-mers are LEFT (their pairs may still fall to -f on the host)
  uint32_t slots;                      // table slots per workgroup: a power of two up to K6_MAX_SLOTS, or 0 = every add goes to global memory
  const uint32_t* target_class;        // [n_cols]
  const uint32_t* species_class;       // [n_cols] or nullptr: strain / assembly level
  double hic_min_qcov;                 // H
  const unsigned long long* n_hits;    // device word or nullptr: the batch's hit counter ...
  uint64_t hit_cap;                    // ... above this the batch will be run again: nothing is counted now
  unsigned long long* counters;        // [4 * n_cols]: rows, firsts, ureads, hic of column c at 4 * c (refstats_rule.hpp)
  unsigned long long* totals;          // [3]: matched reads, unique reads (of the reads counted here), launches the guard skipped
  uint8_t* left;                       // out [n_reads]: 1 = LEFT to the host
  unsigned long long* stats;           // [K6_STATS], zero on entry
};

// K7 (k7_cooccur.hip): K3's segments -> the reads shared by every pair of targets, the counts of stage 2 of `kmcp profile` (cooccur_rule.hpp:
// the key, the table's probe sequence, the two phases); the reads it cannot count exactly are LEFT to the host (a byte per read).
constexpr uint32_t K7_CAP = 64;  // longest segment of several targets the device counts
constexpr uint32_t K7_MAX_SLOTS = 4096, K7_DEFAULT_SLOTS = 2048;  // the workgroup's table in LDS: 12 bytes per slot
constexpr uint64_t K7_DEFAULT_TABLE = 1ull << 21, K7_MAX_TABLE = 1ull << 30;  // the table in HBM: 16 bytes per slot
// the witness: reads empty / single target / by the wave (counted) / LEFT, of those LEFT because the table was full; pairs enumerated (of
// the counted reads), adds to LDS / to global memory (flushes and adds past the LDS table) / of those the ones past a full LDS table, keys
// claimed in HBM, launches the overflow guard skipped, segments outside the buffer
enum { K7_EMPTY = 0, K7_SINGLE, K7_WAVE, K7_LEFT, K7_LEFT_FULL, K7_PAIRS, K7_LDS_ADDS, K7_GLOBAL_ADDS, K7_SPILLED, K7_CLAIMED, K7_SKIPPED, K7_BAD, K7_STATS };
// the totals that persist beside the table: reads with several targets counted here, their pairs, reads LEFT because the table was full,
// launches the guard skipped
enum { K7_T_MULTI = 0, K7_T_PAIRS, K7_T_LEFT_FULL, K7_T_SKIPPED, K7_TOTALS };
struct K7Args {
  const kmcpg_pair* pairs;             // K3's output
  const uint64_t* offs;                // [n_reads + 1]
  uint64_t pair_cap;                   // pairs there is room for behind `pairs`: a segment that ends behind it is treated as empty
  const int32_t* nk;                   // NumKmers per read
  uint32_t n_reads;
  uint32_t n_cols;
  int32_t final_n;                     // reads of more k-mers are LEFT (their pairs may still fall to -f on the host)
  uint32_t slots;                      // LDS table slots per workgroup: a power of two up to K7_MAX_SLOTS, or 0 = every add goes to global memory
  const uint32_t* target_class;        // [n_cols]
  const unsigned long long* n_hits;    // device word or nullptr: the batch's hit counter ...
  uint64_t hit_cap;                    // ... above this the batch will be run again: nothing is counted now
  unsigned long long* keys;            // [table_slots] pair keys, 0 = empty (cooccur_rule.hpp)
  unsigned long long* counts;          // [table_slots]
  uint64_t table_slots;                // a power of two
  unsigned long long* totals;          // [K7_TOTALS]
  uint8_t* left;                       // out [n_reads]: 1 = LEFT to the host
  unsigned long long* stats;           // [K7_STATS], zero on entry
};

// K8 (k8_recount.hip): stage 3 of `kmcp profile` (recount_rule.hpp) in two kernels.  k8_log, behind K3: single-target reads are counted at
// once (four 64-bit counters per column, in units), reads with several targets among up to K8_CAP pairs are appended to the READ LOG; the
// others are LEFT to the host (a byte per read).  k8_replay, after the last batch: the ambiguity correction and the shares of every logged
// read, with stage 1's verdicts and stage 2's pair list.
//
// The read log: `cap` 64-bit words.  Records grow from the front — word 0: pairs m | NumKmers << 32, word 1: qLen, then the m pairs as K3
// left them (col | count << 32) —, the index from the back: the record of logged read k starts at word log[cap - 1 - k].  Two words hold both
// fill levels each (K8_STATE_*): what was asked for (fetch-add; it may run past the end) and what was taken (atomic max of the ends of the
// allocations that fit).
constexpr uint32_t K8_CAP = 64;  // longest segment of several targets the device logs
constexpr uint32_t K8_MAX_SLOTS = 1024, K8_DEFAULT_SLOTS = 1024, K8_PROBES = 8;  // the workgroup's table in LDS: 36 bytes per slot (64-bit counters)
constexpr uint64_t K8_DEFAULT_LOG_BYTES = 256ull << 20, K8_MIN_LOG_BYTES = 64, K8_MAX_LOG_BYTES = 4ull << 30;
constexpr int K8_STATE_WORD_BITS = 36;  // state = logged reads << 36 | record words used (4 GiB: 2^29 words, fewer than 2^28 reads)
// the witness of k8_log: reads empty / single target / logged / LEFT, of those LEFT for want of log room; adds to LDS / to global memory
// (flushes and spills) / of those the spills; launches the overflow guard skipped, segments outside the buffer
enum { K8_EMPTY = 0, K8_SINGLE, K8_LOGGED, K8_LEFT, K8_LEFT_FULL, K8_LDS_ADDS, K8_GLOBAL_ADDS, K8_SPILLED, K8_SKIPPED, K8_BAD, K8_STATS };
// ... and of k8_replay: reads replayed, of those with a kept target / that lost a target / that ended with one target; pair lookups, adds
enum { K8_R_READS = 0, K8_R_RECOUNTED, K8_R_CORRECTED, K8_R_UNIQUE, K8_R_LOOKUPS, K8_R_LDS_ADDS, K8_R_GLOBAL_ADDS, K8_R_SPILLED, K8_R_STATS };
// the totals that persist beside the log: single-target reads counted, reads LEFT for want of log room, launches the guard skipped
enum { K8_T_SINGLE = 0, K8_T_LEFT_FULL, K8_T_SKIPPED, K8_TOTALS };
struct K8LogArgs {
  const kmcpg_pair* pairs;             // K3's output, in print order
  const uint64_t* offs;                // [n_reads + 1]
  uint64_t pair_cap;                   // pairs there is room for behind `pairs`: a segment that ends behind it is treated as empty
  const int32_t* nk;                   // NumKmers per read
  const int32_t* qlen;                 // qLen per read
  uint32_t n_reads;
  uint32_t n_cols;
  int32_t final_n;                     // reads of more k-mers are LEFT (their pairs may still fall to -f on the host)
  uint32_t slots;                      // table slots per workgroup: a power of two up to K8_MAX_SLOTS, or 0 = every add goes to global memory
  const uint32_t* target_class;        // [n_cols]
  double hic_min_qcov;                 // H
  const unsigned long long* n_hits;    // device word or nullptr: the batch's hit counter ...
  uint64_t hit_cap;                    // ... above this the batch will be run again: nothing is counted or logged now
  unsigned long long* counters;        // [4 * n_cols]: match, uniq, hic, bases of column c at 4 * c (recount_rule.hpp), the single-target reads'
  unsigned long long* log;             // [log_cap] the read log
  uint64_t log_cap;                    // words
  unsigned long long* log_state;       // the reserve word ...
  unsigned long long* log_commit;      // ... and the commit word
  unsigned long long* totals;          // [K8_TOTALS]
  uint8_t* left;                       // out [n_reads]: 1 = LEFT to the host
  unsigned long long* stats;           // [K8_STATS], zero on entry
};
struct RecountClass;
struct K8ReplayArgs {
  const unsigned long long* log;       // the read log ...
  uint64_t log_cap;
  uint64_t n_logged;                   // ... and its reads
  uint32_t n_cols, n_classes;
  uint32_t slots;
  const uint32_t* target_class;        // [n_cols]
  const uint32_t* species_class;       // [n_cols] or nullptr: strain / assembly level
  const RecountClass* classes;         // [n_classes] stage 1's verdict and sums (recount_rule.hpp)
  const unsigned long long* keys;      // [n_pairs] stage 2's pairs, cooccur_key ascending ...
  const unsigned long long* counts;    // ... and their reads
  uint64_t n_pairs;
  double one_minus_d, r_err, hic_min_qcov;
  uint32_t no_amb_corr, level_species;
  unsigned long long* counters;        // [4 * n_cols] the replay's counters, zero on entry
  unsigned long long* stats;           // [K8_R_STATS], zero on entry
};

// K9 (k9_em.hip): one pass of stage 4 of `kmcp profile` (em_rule.hpp) over K8's read log: every logged read is shared out over its
// estimated targets in proportion to their coverage; five 64-bit counters per column (match, uniq, hic, bases_lo, bases_hi).
// The workgroup's table in LDS: 44 bytes per slot (five 64-bit counters and the key), 1024 slots = 44 KiB — two workgroups per CU take
// 88 KiB of the CU's 160 KiB.  The default is 0, plain global atomics: the table gained nothing on either sample of tools/bench_em.py
// (0.371 against 0.317 ms and 0.334 against 0.329 ms per pass)
constexpr uint32_t K9_MAX_SLOTS = 1024, K9_DEFAULT_SLOTS = 0, K9_PROBES = 8;
// the witness: logged reads, of those with no / one / several estimated targets; adds to LDS / to global memory (flushes and spills) / of
// those the spills
enum { K9_READS = 0, K9_NONE, K9_ONE, K9_SPLIT, K9_LDS_ADDS, K9_GLOBAL_ADDS, K9_SPILLED, K9_STATS };
struct K9Args {
  const unsigned long long* log;       // the read log (K8LogArgs) ...
  uint64_t log_cap;
  uint64_t n_logged;                   // ... and its reads
  uint32_t n_cols, n_classes;
  uint32_t slots;                      // table slots per workgroup: a power of two up to K9_MAX_SLOTS, or 0 = every add goes to global memory
  uint32_t level_species;
  const uint32_t* target_class;        // [n_cols]
  const uint32_t* species_class;       // [n_cols] or nullptr: strain / assembly level
  const kmcpg_em_class* classes;       // [n_classes] the pass's whitelist and coverages
  double hic_min_qcov;
  unsigned long long* counters;        // [5 * n_cols] the pass's counters, zero on entry
  unsigned long long* stats;           // [K9_STATS], zero on entry
};

}  // namespace kmcpg
