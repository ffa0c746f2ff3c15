// engine.hpp — internals shared by the host-side translation units of libkmcpgpu.so (engine.cpp: residency;
// query.cpp: GPU half; finalize.cpp: host half; lane.cpp + host*.cpp: the whole pipeline on host buffers, lane.hpp).  Not part of the ABI.
#pragma once
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/kmcp_gpu.h"
#include "common.hpp"
#include "dbformat.hpp"
#include "k1_plan.hpp"
#include "fpr.hpp"

// error sink: sets the thread-local message behind kmcpg_last_error() and returns `code`
int kmcpg_fail(int code, const char* fmt, ...);
std::string& kmcpg_err_ref();  // the calling thread's message (workers hand theirs to the caller)

#define HIPCHK(expr)                                                                               \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return kmcpg_fail(KMCPG_EDEVICE, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// search entry points: refused on a handle over bare .uniki files (kmcpg_open_files knows no __db.yml: no fpr, no k-mer sketching parameters)
#define KMCPG_NO_FILES_ONLY(db)                                                                                   \
  do {                                                                                                            \
    if ((db)->files_only) return kmcpg_fail(KMCPG_EUNSUPPORTED, "handle of kmcpg_open_files: index inspection only, open the database directory with kmcpg_open to search it"); \
  } while (0)

// GPU work on a handle: refused for metadata-only handles (opts.device == -1)
#define KMCPG_USE_DEVICE(db)                                                                                      \
  do {                                                                                                            \
    if ((db)->opts.device < 0) return kmcpg_fail(KMCPG_EDEVICE, "metadata-only handle (device -1): no GPU work possible"); \
    HIPCHK(hipSetDevice((db)->opts.device));                                                                      \
  } while (0)

namespace kmcpg {

struct BlockMeta {
  std::string path;
  UnikiHeader h;
  uint32_t col_base = 0;
  bool local = false;
  int local_idx = -1;
  uint32_t stride = 0;          // row pitch of the group the block lives in
  uint8_t* d_rows = nullptr;    // first byte of the block inside its group's rows (not an allocation of its own)
  int group = -1;
  uint32_t byte_off = 0;        // offset of the block's bytes inside the group's row
};

// Resident blocks with the same NumSigs share one set of rows (common.hpp BlockDev): the allocation belongs to the group.
struct Group {
  uint8_t* d_rows = nullptr;
  uint64_t num_sigs = 0;
  uint32_t stride = 0, row_bytes = 0;
  std::vector<int> members;  // global block indices, in __db.yml `files` order
};

struct SlotClass {
  int lpr = 0;
  std::vector<Slot> slots;
  Slot* d_slots = nullptr;
  // the same tiles as block units (64-lane class only): a group whose tiles all fall into this class is ONE slot, the tiles of any
  // other group stay one slot each (finish_open)
  std::vector<Slot> bslots;
  Slot* d_bslots = nullptr;
};

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  int ensure(size_t n) {
    if (n <= cap) return 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = n + n / 8 + 64;
    if (hipMalloc((void**)&p, want * sizeof(T)) != hipSuccess) return -1;
    cap = want;
    return 0;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

}  // namespace kmcpg

namespace kmcpg {
struct Exchange;
// smallest count whose FPR(n, count) passes -f, for n = 0..n (query.cpp fpr_bound); h = pinned source of the upload
struct FprBoundTable {
  uint64_t key = 0;  // bits of max_fpr
  int n = 0;
  uint16_t* d = nullptr;
  uint16_t* h = nullptr;
};
void release_fpr_bounds(kmcpg_db* db);  // query.cpp
int plan_passes(kmcpg_db* front, int device, uint64_t* largest_shard_bytes, uint64_t* free_bytes, uint64_t* reserve_bytes = nullptr);  // engine.cpp
int open_like(const kmcpg_db* src, const kmcpg_opts* opts, kmcpg_db** out);                           // engine.cpp
struct AsyncState;
void async_release(kmcpg_db* db);  // lane.cpp
int async_in_flight(kmcpg_db* db);
}  // namespace kmcpg

struct kmcpg_db {
  kmcpg_opts opts{};
  kmcpg_info info{};
  std::vector<kmcpg::BlockMeta> blocks;
  std::vector<int> local;  // global indices of resident blocks, in kmcpg::BlockDev order
  std::vector<kmcpg::BlockDev> h_blockdev;  // per resident block (planting / read-back helpers)
  kmcpg::BlockDev* d_blockdev = nullptr;
  std::vector<kmcpg::Group> groups;
  std::vector<kmcpg::BlockDev> h_groupdev;  // per group: what K2 gathers from
  kmcpg::BlockDev* d_groupdev = nullptr;
  std::vector<kmcpg::Seg> h_segs;
  kmcpg::Seg* d_segs = nullptr;
  std::vector<kmcpg::SlotClass> classes;
  std::vector<uint32_t> col_block;  // global column -> block index
  struct ColMeta {   // per global column, side by side for the host half (one cache line per hit instead of three)
    uint64_t size;   // Header.Sizes: k-mers of the column
    uint64_t gsize;  // Header.GSizes
    uint32_t tidx;   // Header.Indices: chunk index | #chunks << 16
    uint32_t pad;
  };
  std::vector<ColMeta> col_meta;
  std::unique_ptr<kmcpg::QueryFpr> fpr;
  std::mutex mu;      // serialises the enqueueing of GPU-half calls (kernels of one workspace slot follow each other in stream order;
                      // calls on different streams are ordered by the slot's event)
  std::vector<int> ks_desc;    // k-mer sizes of the database, descending (`ks` of __db.yml; one entry for most databases)
  kmcpg::AsyncState* async = nullptr;  // lanes + streams of kmcpg_submit/kmcpg_wait (lane.hpp), created on first use
  // The k-mer workspace of kmcpg_query_device, twice: consecutive calls take the slots in turn, so that the k-mer kernels of batch
  // i + 1 (VALU-bound) may run on another stream BESIDE the COBS kernels of batch i (memory-bound) instead of behind them.  A call
  // waits for the previous user of ITS slot only (Workspace::ev); the COBS kernels themselves stay one batch at a time (cobs_ev:
  // two of them side by side would only share the memory system, and their HIP-event durations would stop meaning anything).
  // The second slot is used only while a second workspace of the batch's size fits beside the index (query.cpp pick_slot).
  struct Workspace {
    kmcpg::DevBuf<uint64_t> w_hashes, w_scratch;
    kmcpg::DevBuf<int32_t> w_nk_raw, w_nk1, w_seg_cnt;
    kmcpg::DevBuf<uint32_t> w_long_list, w_long_meta, w_long_counts;  // long-query (split) path
    kmcpg::DevBuf<uint64_t> w_huge_info;                             // whole-genome queries: (read, n, offset)
    kmcpg::DevBuf<uint8_t> w_huge_temp;                              // histogram table of the device-wide radix sort
    kmcpg::DevBuf<uint32_t> w_dedup_fb;                              // profiling: queries per k_dedup_bucket class that took its bitonic fallback
    kmcpg::DevBuf<uint64_t> w_gathered;                              // profiling level 2: the row loads k2_cobs issued
    kmcpg::DevBuf<uint64_t> w_k2_queue;                              // k2_cobs_persist: the unit counter of every grid piece (k2_claim.hpp)
    // sliding windows, hash-once form: per-position hashes, kept hashes in order, ranks, per-chunk counts and their prefix
    kmcpg::DevBuf<uint64_t> w_win_h, w_win_kept, w_win_cbase;
    kmcpg::DevBuf<uint32_t> w_win_rank, w_win_cnt;
    hipEvent_t ev = nullptr;  // recorded at the end of every call that used the slot: the slot's next user waits for it
    bool ev_valid = false;
    hipEvent_t in_ev = nullptr, k1_ev = nullptr;  // KMCPG_K1_STREAM: inputs ready on the caller's stream / k-mers ready on k1_stream
    void release() {
      w_hashes.release(); w_scratch.release(); w_nk_raw.release(); w_nk1.release(); w_seg_cnt.release(); w_long_list.release();
      w_long_meta.release(); w_long_counts.release(); w_huge_info.release(); w_huge_temp.release(); w_gathered.release(); w_dedup_fb.release();
      w_k2_queue.release();
      w_win_h.release(); w_win_kept.release(); w_win_cbase.release(); w_win_rank.release(); w_win_cnt.release();
      if (ev) (void)hipEventDestroy(ev);
      if (in_ev) (void)hipEventDestroy(in_ev);
      if (k1_ev) (void)hipEventDestroy(k1_ev);
      ev = in_ev = k1_ev = nullptr;
      ev_valid = false;
    }
  };
  Workspace ws[2];
  uint64_t ws_calls = 0;       // kmcpg_query_device calls so far: slot = ws_calls & 1 (when the second slot may be used)
  uint64_t k1_codes_direct = 0, k1_codes_expanded = 0;  // packed batches: k-mer kernels on the codes / on text expanded first (kmcpg_k1_codes_batches)
  int ws_last = 0;             // slot of the last kmcpg_query_device call (kmcpg_last_gathered_bytes reads its counters)
  hipStream_t k1_stream = nullptr;  // experiment (KMCPG_K1_STREAM=1): the k-mer kernels on a high-priority stream of the handle's own
  hipEvent_t cobs_ev = nullptr;  // end of the last call's COBS kernels: the next call's COBS kernels wait for it
  bool cobs_ev_valid = false;
  hipEvent_t fin_ev = nullptr;   // K3's scratch (w_fin_cnt, w_fin_sums) has one user at a time, whatever the k-mer slots do
  bool fin_ev_valid = false;
  bool synthetic = false;
  bool files_only = false;  // kmcpg_open_files: .uniki files without a __db.yml — inspection and read-back only, every search entry point refuses
  float last_density_ms = -1;  // HIP-event time of that call's device work (memsets, kernels), before the copy to the host
  kmcpg_density_launch last_density{};  // what the last kmcpg_block_density / kmcpg_col_ones call launched (density_host.cpp)
  // in-process multi-GPU front handle (kmcpg_open_devices): metadata only itself, one resident shard handle per device
  std::vector<kmcpg_db*> shards;
  kmcpg::Exchange* exchange = nullptr;  // RCCL gather of the shards' hit lists (exchange.cpp); nullptr = host merge
  std::string exchange_why;             // why not, when nullptr
  // paged handle (kmcpg_open_paged): metadata only itself; every batch is searched against the index one shard at a time
  // (paged_passes shards, the same partition kmcpg_open makes for shard_count = paged_passes); the shard searched last stays
  // resident and is the first one of the next batch
  std::string db_dir;
  int paged_passes = 0, paged_device = 0, paged_rank = -1;
  kmcpg_db* paged_resident = nullptr;
  std::mutex paged_mu;
  uint64_t paged_uploads = 0;  // shards made resident so far (tests / logs)
  uint64_t paged_reserve = 0;  // HBM plan_passes() kept free beside the largest shard: what a batch's workspace may take
  // optional HIP-event timing of the last kmcpg_query_device call
  int profiling = 0;  // 1: HIP-event timing of the kernels; 2: + count the row loads k2_cobs issues
  std::vector<kmcpg_k2_launch> k2_log;  // the COBS kernels the last kmcpg_query_device call launched (profiling >= 1; kmcpg_last_k2_launches)
  // the K1 kernels the last k-mer stage launched, the plan's record first (profiling >= 1; kmcpg_last_k1_launches), and — for the two list
  // forms — the device word that holds what the first kernel left on its list (valid until the slot's next batch)
  std::vector<kmcpg_k1_launch> k1_log;
  const uint32_t* k1_left = nullptr;
  // what the last dedup stage (K1d: query.cpp run_dedup) launched (profiling >= 1; kmcpg_last_dedup_launches).  A log of its own: the K1
  // log is asserted record by record
  std::vector<kmcpg_dedup_launch> dedup_log;
  const uint32_t* dedup_fb = nullptr;  // ... and the three device words its k_dedup_bucket launches count their fallback queries in
  // K3 (device half of finalize): Header.Sizes of every global column on the device, per-read counters and scan scratch
  uint64_t* d_col_size = nullptr;
  kmcpg::DevBuf<uint32_t> w_fin_cnt;
  kmcpg::DevBuf<uint64_t> w_fin_sums;
  // database set (kmcpg_open_set): the directories of the members and the first global column of each (one entry for every handle that
  // kmcpg_open / kmcpg_open_set made; a SET in the sense of the merge order and the refusals is a handle with two members or more)
  std::vector<std::string> set_dirs;
  std::vector<uint32_t> set_col_base;
  bool is_set() const { return set_col_base.size() > 1; }
  uint32_t* d_set_stats = nullptr;  // K3SetArgs::stats of the last K3 launch (kmcpg_last_set_order)
  // what the host half ordered itself since that launch (finalize.cpp): segments, and runs of equal fixed4 with several members in them
  mutable std::atomic<uint64_t> set_host_segments{0}, set_host_mixed{0};
  // K4, the species-specific stage (kmcpg_set_specific; k4_specific.hip): the two per-column tables on the device and on the host, the
  // stage's scratch (one user at a time: it shares K3's event chain, fin_ev), its counters (K4_STATS 32-bit words, then at byte 32 the
  // pairs in and out as two 64-bit words) and what its last launch noted (profiling >= 1)
  uint32_t* d_spec_target = nullptr;
  uint32_t* d_spec_species = nullptr;
  std::vector<uint32_t> h_spec_target, h_spec_species;  // species empty: strain level
  bool spec_on() const { return !h_spec_target.empty(); }
  kmcpg::DevBuf<uint32_t> w_spec_cnt;
  kmcpg::DevBuf<uint64_t> w_spec_sums;
  uint64_t* d_spec_stats = nullptr;
  bool spec_ran = false;  // a K4 launch since the stage was set
  hipEvent_t spec_ev[2] = {};  // around the stage's kernels (profiling >= 1)
  bool spec_timed = false;
  std::vector<kmcpg_k4_launch> k4_log;
  // K5, the window summaries behind K4 (k5_summary.hip): its counters (K5_STATS 32-bit words, then at byte 32 the LEFT pairs as a 64-bit
  // word) and what its last launch noted; the scratch is K4's
  uint64_t* d_sum_stats = nullptr;
  bool sum_ran = false;
  hipEvent_t sum_ev[2] = {};
  bool sum_timed = false;
  std::vector<kmcpg_k4_launch> k5_log;
  // ... or, after kmcpg_wait_summaries, what that ticket's batches came to (all its pieces; counted on the host from the records)
  bool sum_from_ticket = false;
  kmcpg_summary_stats sum_ticket{};
  // K6, the reference statistics behind K3 (kmcpg_set_refstats; k6_refstats.hip, refstats.cpp): tables of its own (the stage does not filter
  // and is independent of K4), H, the device counters (4 words per column, then matched / unique reads), the witness words of the last
  // launch, and the host half's counters (the reads the device LEFT, and every read of a batch that did not go through K3; under rs_mu)
  uint32_t* d_rs_target = nullptr;
  uint32_t* d_rs_species = nullptr;
  std::vector<uint32_t> h_rs_target, h_rs_species;  // species empty: strain level
  bool refstats_on() const { return !h_rs_target.empty(); }
  double rs_hic = 0;
  unsigned long long* d_rs_counters = nullptr;  // [4 * n_cols + 3]
  unsigned long long* d_rs_stats = nullptr;     // [K6_STATS]
  uint32_t rs_slots = 0;                        // KMCPG_REFSTATS_SLOTS, read when the stage is set
  unsigned rs_max_wgs = 0, rs_grid = 0;         // the chip's resident workgroups (KMCPG_REFSTATS_WGS: fewer, for tests); the last launch's grid
  std::mutex rs_mu;
  std::vector<uint64_t> h_rs_counters;          // [4 * n_cols]
  uint64_t h_rs_matched = 0, h_rs_unique = 0, h_rs_reads = 0;
  bool rs_tainted = false;  // a batch failed after its reads were counted: the counters may hold reads that are searched again
  bool rs_ran = false;      // a K6 launch since the stage was set
  hipEvent_t rs_ev[2] = {};
  bool rs_timed = false;
  std::vector<kmcpg_k4_launch> k6_log;
  // K7, the shared reads of reference pairs behind K3 (kmcpg_set_cooccur; k7_cooccur.hip, cooccur.cpp): a class table of its own, the
  // open-addressed pair table in HBM (keys, counts: co_table slots each, a power of two), the totals that persist beside it, the witness
  // words of the last launch, and the host half's map (key of cooccur_rule.hpp -> reads: the reads the device LEFT, and every read of a
  // batch that did not go through K3; under co_mu)
  uint32_t* d_co_target = nullptr;
  std::vector<uint32_t> h_co_target;
  bool cooccur_on() const { return !h_co_target.empty(); }
  unsigned long long* d_co_keys = nullptr;    // [co_table]
  unsigned long long* d_co_counts = nullptr;  // [co_table]
  unsigned long long* d_co_totals = nullptr;  // [K7_TOTALS]
  unsigned long long* d_co_stats = nullptr;   // [K7_STATS]
  uint64_t co_table = 0;
  uint32_t co_slots = 0;                      // KMCPG_COOCCUR_SLOTS, read when the stage is set
  unsigned co_max_wgs = 0, co_grid = 0;
  std::mutex co_mu;
  std::unordered_map<uint64_t, uint64_t> h_co_pairs;
  uint64_t h_co_multi = 0, h_co_adds = 0;
  bool co_tainted = false;  // a batch failed after its reads were counted
  bool co_ran = false;      // a K7 launch since the stage was set
  hipEvent_t co_ev[2] = {};
  bool co_timed = false;
  std::vector<kmcpg_k4_launch> k7_log;
  // K8, the recount with ambiguity correction (kmcpg_set_recount; k8_recount.hip, recount.cpp): class tables of its own, H, the counters of
  // the single-target reads and of the last replay (4 words per column each), the read log in HBM with its state word, the totals that
  // persist beside it, the witness words of the last k8_log launch and of the last replay; and the host half's log — the reads the device
  // LEFT, and every read of a batch that did not go through K3 — in the device log's record form (common.hpp: K8LogArgs), its index
  // beside it (under rc_mu)
  uint32_t* d_rc_target = nullptr;
  uint32_t* d_rc_species = nullptr;
  std::vector<uint32_t> h_rc_target, h_rc_species;  // species empty: strain level
  bool recount_on() const { return !h_rc_target.empty(); }
  double rc_hic = 0;
  unsigned long long* d_rc_counters = nullptr;  // [4 * n_cols] single-target reads
  unsigned long long* d_rc_replay = nullptr;    // [4 * n_cols] the last replay
  unsigned long long* d_rc_log = nullptr;       // [rc_log_cap]
  unsigned long long* d_rc_words = nullptr;     // the log's state word, then K8_TOTALS, K8_STATS and K8_R_STATS words
  uint64_t rc_log_cap = 0;                      // words
  uint32_t rc_slots = 0;                        // KMCPG_RECOUNT_SLOTS, read when the stage is set
  unsigned rc_max_wgs = 0, rc_grid = 0, rc_replay_grid = 0;
  std::mutex rc_mu;
  std::vector<uint64_t> h_rc_log, h_rc_index;
  std::vector<uint64_t> h_rc_replay;            // [4 * n_cols] the last replay of the host log
  std::vector<uint8_t> rc_kept;                 // per column: its class was kept in the last kmcpg_recount_run
  uint64_t rc_run_totals[4] = {};               // of the last run: recounted / unique / corrected reads of both replays, reads replayed by the device
  bool rc_tainted = false;  // a batch failed after its reads were logged
  bool rc_ran = false, rc_replayed = false;  // a k8_log launch / a kmcpg_recount_run since the stage was set
  hipEvent_t rc_ev[2] = {}, rc_rev[2] = {};
  bool rc_timed = false, rc_rtimed = false;
  std::vector<kmcpg_k4_launch> k8_log, k8_rlog;
  // K9, an EM pass over K8's logs (kmcpg_em_pass; k9_em.hip, em.cpp): the pass counters of both halves (five words per column), the pass's
  // classes on the device, the witness words; allocated on first use, freed with the recount stage
  unsigned long long* d_em_counters = nullptr;  // [5 * n_cols]
  unsigned long long* d_em_words = nullptr;     // [K9_STATS]
  kmcpg_em_class* d_em_classes = nullptr;       // [em_classes_cap]
  uint32_t em_classes_cap = 0, em_slots = 0;
  std::vector<uint64_t> h_em_pass;              // [5 * n_cols] the last pass over the host log ...
  std::vector<uint64_t> h_em_single;            // ... [4 * n_cols] its single-target reads of estimated classes, in K8's units
  std::vector<uint8_t> em_est;                  // per column: its class was estimated in the last pass
  uint64_t em_totals[4] = {};                   // of the last pass: reads with one / several targets on the device, then on the host
  bool em_ran = false, em_timed = false;
  unsigned em_grid = 0;
  hipEvent_t em_ev[2] = {};
  std::vector<kmcpg_k4_launch> k9_log;
  // K10, the LEFT reads' pairs compacted behind the counting stages (kmcpg_submit_stats, kmcpg_left_compact_device; k10_left.hip,
  // stats.cpp): the scan's offsets before they are published, the witness words of the last launch that did not bring its own, and what
  // that launch noted; cnt and sums are K4's scratch (one user at a time: fin_ev).  All of it allocated on first use
  kmcpg::DevBuf<uint64_t> w_left_offs;
  unsigned long long* d_left_stats = nullptr;  // [K10_STATS]
  bool left_ran = false, left_timed = false;
  hipEvent_t left_ev[2] = {};
  std::vector<kmcpg_k4_launch> k10_log;
  // ... or, after kmcpg_wait_stats, what that ticket's batch came to
  bool left_from_ticket = false;
  kmcpg_stats_ticket_stats left_ticket{};
  // K11, taxonomic binning (kmcpg_set_binning, kmcpg_bin_device; k11_bin.hip, binning.cpp): the plan's tables — node_of_column [n_cols],
  // then parent, last, taxid [n_nodes] each, in ONE allocation — their host copies, the witness words and what the last launch noted
  std::vector<uint32_t> h_bin_node, h_bin_parent, h_bin_last, h_bin_taxid;
  uint32_t* d_bin_tables = nullptr;
  unsigned long long* d_bin_stats = nullptr;  // [K11_STATS]
  bool binning_on() const { return !h_bin_parent.empty(); }
  unsigned bin_max_wgs = 0, bin_grid = 0;  // the chip's resident workgroups (KMCPG_BIN_WGS: fewer, for tests); the last launch's grid
  bool bin_ran = false, bin_timed = false, bin_in_lds = false;
  hipEvent_t bin_ev[2] = {};
  std::vector<kmcpg_k4_launch> k11_log;
  // ... or, after kmcpg_wait_bins, what that ticket's batch came to
  bool bin_from_ticket = false;
  kmcpg_bin_stats bin_ticket{};
  std::vector<kmcpg::FprBoundTable> fpr_bounds;  // -f bound tables (query.cpp fpr_bound): one per (max_fpr, size), never rewritten
  hipEvent_t ev[16] = {};   // ring of 4 calls x (start, COBS start, COBS done, k-mers done)
  uint64_t ev_calls = 0;    // profiled calls so far
};


namespace kmcpg {

// Database sets: what acts per member in separate runs and would act per query on the union is refused (include/kmcp_gpu.h kmcpg_open_set)
inline int set_refuse_params(const kmcpg_db* db, const kmcpg_params& p) {
  if (!db->is_set()) return 0;
  const char* what = p.try_se ? "try_se" : (p.do_not_sort ? "do_not_sort" : (p.top_n_scores != 0 ? "top_n_scores != 0" : (p.k != 0 ? "params->k != 0" : nullptr)));
  if (!what) return 0;
  return kmcpg_fail(KMCPG_EUNSUPPORTED, "database set (%zu members): %s is not supported — it acts per member in separate searches and would act per query here; "
                    "search the databases one by one and merge the results with kmcp-merge", db->set_col_base.size(), what);
}
inline int set_refuse_entry(const kmcpg_db* db, const char* entry) {
  if (!db->is_set()) return 0;
  return kmcpg_fail(KMCPG_EUNSUPPORTED, "database set (%zu members): %s is not supported on a set handle", db->set_col_base.size(), entry);
}

// The stages behind K3 that need a query's matches from EVERY block (K4 / K5: specific.cpp, K6: refstats.cpp, K7: cooccur.cpp) refuse the handles that
// search the index in parts.  "<refused> are not supported on <the handle>: <why>"
inline int refuse_handle(const kmcpg_db* db, const char* refused, const char* why) {
  const char* what = db->paged_passes > 0 ? "a paged handle (kmcpg_open_paged)"
                     : !db->shards.empty() ? "a multi-device handle (kmcpg_open_devices)"
                     : db->opts.shard_count > 1 ? "a handle with shard_count > 1"
                                                : nullptr;
  if (!what) return 0;
  return kmcpg_fail(KMCPG_EUNSUPPORTED, "%s are not supported on %s: %s", refused, what, why);
}

// a per-handle event of its own kind (COBS kernels one batch at a time; K3's scratch one user at a time): the next user waits for it
inline int chain_begin(hipEvent_t* ev, bool valid, hipStream_t st) {
  if (!*ev) HIPCHK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
  if (valid) HIPCHK(hipStreamWaitEvent(st, *ev, 0));
  return 0;
}
// K3's scratch and K4's (one user at a time: K3's chain, K4, K5) on the chain of fin_ev: wait() orders the call behind the previous user;
// from then on every way out, error paths included, leaves the event behind for the next one — kernels that use the scratch may already
// be on the stream when a later step fails
struct FinGuard {
  kmcpg_db* db;
  hipStream_t st;
  bool armed = false;
  int wait() {
    if (int rc = chain_begin(&db->fin_ev, db->fin_ev_valid, st)) return rc;
    armed = true;
    return 0;
  }
  ~FinGuard() {
    if (armed && db->fin_ev && hipEventRecord(db->fin_ev, st) == hipSuccess) db->fin_ev_valid = true;
  }
};

// A stage's launches between its two timing events (created on first use), when the call is timed (profiling >= 1) ...
template <class Launch>
int timed_launches(hipEvent_t (&ev)[2], bool timed, hipStream_t st, Launch launch) {
  if (timed) {
    for (auto& e : ev)
      if (!e) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventRecord(ev[0], st));
  }
  launch();
  if (timed) HIPCHK(hipEventRecord(ev[1], st));
  return 0;
}
// ... and what kmcpg_last_* reports of them (the device is idle): the milliseconds between the events (*ms stays as it is where the call
// was not timed), and the launch log — its length always, its first `cap` records — at profiling >= 1
inline void timed_launches_report(const kmcpg_db* db, const hipEvent_t (&ev)[2], bool timed, const std::vector<kmcpg_k4_launch>& log, double* ms,
                                  kmcpg_k4_launch* launches, uint32_t cap, uint32_t* n_launches) {
  float f = 0;
  if (timed && ev[1] && hipEventElapsedTime(&f, ev[0], ev[1]) == hipSuccess) *ms = f;
  const size_t have = db->profiling >= 1 ? log.size() : 0;
  const size_t m = std::min<size_t>(cap, have);
  if (m) memcpy(launches, log.data(), m * sizeof(kmcpg_k4_launch));
  *n_launches = (uint32_t)have;
}

// What a stage that judges or counts a query's FINAL matches, once, refuses while it is on (K4 and the counting stages): the parameter
// that would make it see something else, or nullptr
// (the smaller-k retry of a database with several k-mer sizes looks for reads without matches, and a dropped read is not one)
inline const char* final_matches_refused(const kmcpg_db* db, const kmcpg_params& p) {
  return p.try_se ? "try_se" : (p.top_n_scores != 0 ? "top_n_scores != 0" : (p.k == 0 && db->ks_desc.size() > 1 ? "a database with several k-mer sizes searched with params->k == 0" : nullptr));
}

// The species-specific stage (kmcpg_set_specific): what would judge something else than a query's final matches is refused while it is on
inline int specific_refuse_params(const kmcpg_db* db, const kmcpg_params& p) {
  const char* what = db->spec_on() ? final_matches_refused(db, p) : nullptr;
  if (!what) return 0;
  return kmcpg_fail(KMCPG_EUNSUPPORTED, "species-specific queries (kmcpg_set_specific): %s is not supported — switch the stage off, or filter the results with kmcp-filter", what);
}
inline int specific_refuse_entry(const kmcpg_db* db, const char* entry) {
  if (!db->spec_on()) return 0;
  return kmcpg_fail(KMCPG_EUNSUPPORTED, "species-specific queries (kmcpg_set_specific): %s is not supported while the stage is on", entry);
}

// The COUNTING STAGES: K6 (the reference statistics), K7 (the shared reads of reference pairs) and K8 (the recount's log).  Each counts a
// query's final matches behind K3 — a kernel that marks the reads it LEFT, the host half for those (finalize.cpp left_reads_host) — into state
// on the handle that its *_read entry adds up.  What hangs them into a batch is stated once, over this table: the lane (lane.cpp), the
// refusals, the taint rule.
enum CountingStage { K6, K7, K8, N_COUNTING };
struct CountingStageDesc {
  bool (kmcpg_db::*on)() const;
  std::mutex kmcpg_db::*mu;
  bool kmcpg_db::*tainted;                  // under mu: a batch failed after its reads were counted; the stage's read-outs refuse until its reset
  const char *title, *setter, *instead;     // the words of its refusals
  const char* device_knob;                  // = 0 in the environment: the kernel leaves every read to the host half
};
inline const CountingStageDesc kCountingStages[N_COUNTING] = {
    {&kmcpg_db::refstats_on, &kmcpg_db::rs_mu, &kmcpg_db::rs_tainted, "reference statistics", "kmcpg_set_refstats", "count the results with kmcp-refstats", "KMCPG_REFSTATS_DEVICE"},
    {&kmcpg_db::cooccur_on, &kmcpg_db::co_mu, &kmcpg_db::co_tainted, "shared reads of reference pairs", "kmcpg_set_cooccur", "count the results with kmcp-refstats --cooccur", "KMCPG_COOCCUR_DEVICE"},
    {&kmcpg_db::recount_on, &kmcpg_db::rc_mu, &kmcpg_db::rc_tainted, "recount with ambiguity correction", "kmcpg_set_recount", "recount the results with kmcp-refstats --recount", "KMCPG_RECOUNT_DEVICE"},
};
inline bool counting_on(const kmcpg_db* db, int s) { return (db->*kCountingStages[s].on)(); }
inline unsigned counting_mask(const kmcpg_db* db) {  // bit s: stage s is on
  unsigned m = 0;
  for (int s = 0; s < N_COUNTING; s++) m |= (unsigned)counting_on(db, s) << s;
  return m;
}
// The same refusals as the species-specific stage, for the same reason — what is counted must be a query's final matches, counted once
inline int counting_refuse_params(const kmcpg_db* db, const kmcpg_params& p) {
  const char* what = final_matches_refused(db, p);
  for (int s = 0; what && s < N_COUNTING; s++)
    if (const CountingStageDesc& d = kCountingStages[s]; counting_on(db, s))
      return kmcpg_fail(KMCPG_EUNSUPPORTED, "%s (%s): %s is not supported — switch the stage off, or %s", d.title, d.setter, what, d.instead);
  return 0;
}
inline int counting_refuse_entry(const kmcpg_db* db, const char* entry) {
  for (int s = 0; s < N_COUNTING; s++)
    if (const CountingStageDesc& d = kCountingStages[s]; counting_on(db, s))
      return kmcpg_fail(KMCPG_EUNSUPPORTED, "%s (%s): %s is not supported while the stage is on", d.title, d.setter, entry);
  return 0;
}
// A batch failed after the stages in `mask` may have counted its reads, and a caller may search them again
inline void counting_taint(kmcpg_db* db, unsigned mask) {
  for (int s = 0; s < N_COUNTING; s++)
    if ((mask >> s & 1) && counting_on(db, s)) {
      std::lock_guard<std::mutex> g(db->*kCountingStages[s].mu);
      db->*kCountingStages[s].tainted = true;
    }
}

inline kmcpg_params default_params() {
  kmcpg_params p{};
  p.min_qlen = 30;
  p.min_matched = 10;
  p.min_qcov = 0.55;
  p.min_tcov = 0;
  p.max_fpr = 0.01;
  p.dedup_threshold = 256;
  return p;
}

// std::vector whose resize() leaves trivially-constructible elements uninitialised (no 60-MB memset per batch)
template <class T>
struct NoInitAlloc : std::allocator<T> {
  template <class U>
  struct rebind {
    using other = NoInitAlloc<U>;
  };
  template <class U, class... A>
  void construct(U* q, A&&... a) {
    if constexpr (sizeof...(A) == 0) ::new ((void*)q) U;
    else ::new ((void*)q) U(std::forward<A>(a)...);
  }
};
// ... and whose storage starts on a cache line.  A kmcpg_match is 56 bytes (seven 8-byte words, finalize.cpp asserts it), so
// records straddle lines; the host half writes them with 8-byte streaming stores, which only need 8-byte alignment — the
// aligned start merely keeps the first write-combining buffer of an array whole (finalize.cpp)
template <class T>
struct LineAlloc : NoInitAlloc<T> {
  template <class U>
  struct rebind {
    using other = LineAlloc<U>;
  };
  T* allocate(size_t n) {
    void* q = nullptr;
    if (posix_memalign(&q, 64, std::max<size_t>(64, n * sizeof(T))) != 0) throw std::bad_alloc();
    return (T*)q;
  }
  void deallocate(T* q, size_t) { free(q); }
};
typedef std::vector<kmcpg_match, LineAlloc<kmcpg_match>> MatchVec;

struct ResultOwner {
  std::vector<int32_t> qlen, qkmers, ksize;
  std::vector<uint64_t> offs;
  MatchVec matches;
  // compact results (kmcpg_search_batch_pairs / kmcpg_wait_pairs): the final (column, count) pairs of every read, in the order its
  // Match records would have, instead of the records themselves
  std::vector<kmcpg_pair, NoInitAlloc<kmcpg_pair>> pairs;
  bool pairs_mode = false;
};
// finalize.cpp: a result assembled piece by piece (kmcpg_search_batch cuts large batches into pieces, host.cpp)
ResultOwner* result_owner_take();
void result_owner_give(ResultOwner* o);
void result_owner_shape(ResultOwner* o, uint32_t n_reads, bool as_pairs);  // as_pairs: the result collects compact pairs, not Match records
// trusted: the list is what K2 + K3 made of this very batch with these very params (the library's own pipelines) — thresholds, -T, the
// -f bound of short queries and the order of segments up to K3_WG_CAP hold by construction
int finalize_grouped_into(const kmcpg_db* db, const kmcpg_pair* pairs, const uint64_t* read_offs, const int32_t* qkmers, const int32_t* qlen, uint32_t n_reads,
                          const kmcpg_params& p, ResultOwner* o, uint32_t read_base, uint64_t match_base, uint64_t* kept_out, bool trusted = false,
                          int32_t bound_n = 0, const uint8_t* verdicts = nullptr);
int finalize_grouped_trusted(const kmcpg_db* db, const kmcpg_pair* pairs, const uint64_t* read_offs, const int32_t* qkmers, const int32_t* qlen, uint32_t n_reads,
                             const kmcpg_params& p, kmcpg_result* out, int32_t bound_n, bool as_pairs, const uint8_t* verdicts = nullptr);
// verdicts (K4's bytes for these reads, or nullptr): a read marked SPECIFIC_HOST is judged here by the rule of specific_rule.hpp on what
// the filters above left of it, with the handle's tables; KEEP and DROP were settled on the device.
// specific_filter_result: the same rule on every read of a finished result of Match records (the paths without K3)
void specific_filter_result(const kmcpg_db* db, kmcpg_result* out);
// The host half of the counting stages (finalize.cpp), for the reads of a batch their kernels LEFT: K3's pairs (n_reads + 1 offsets), the
// host's own tests (-f among them) first, the host's order for segments above K3_WG_CAP, then each read's final rows to the stages of `mask`
// that took it — left[s][r] != 0, or left[s] == nullptr: every read — by refstats_rule.hpp into the host counters (K6), by cooccur_rule.hpp
// into the host map (K7), in final order into the host log (K8).  counting_host_result: every read of a finished result of Match records
// (the paths without K3), for the stages that are on.
int left_reads_host(kmcpg_db* db, const kmcpg_pair* pairs, const uint64_t* read_offs, const int32_t* qkmers, const int32_t* qlen, uint32_t n_reads,
                    const kmcpg_params& p, unsigned mask, const uint8_t* const left[N_COUNTING]);
void counting_host_result(kmcpg_db* db, const kmcpg_result* out);
// K6 behind K3 for a lane's batch (refstats.cpp): what kmcpg_refstats_device does, without the public entry's argument checks
int refstats_enqueue(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers, uint32_t n_reads,
                     int32_t final_n, const uint64_t* d_n_hits, uint64_t hit_cap, uint8_t* d_left, hipStream_t st);
// kmcpg_db::d_rc_words: the log's reserve word, its commit word (what the log holds: logged reads << K8_STATE_WORD_BITS | record words),
// then the totals and the two sets of witness words.  recount.cpp lays them out; em.cpp reads the commit word
constexpr size_t RC_COMMIT = 1, RC_TOTALS = 2, RC_STATS = RC_TOTALS + K8_TOTALS, RC_RSTATS = RC_STATS + K8_STATS, RC_WORDS = RC_RSTATS + K8_R_STATS;
// K9's buffers and state go with the recount stage (em.cpp); the caller holds db->mu and the device is idle
void em_release(kmcpg_db* db);
// k8_log behind K3 for a lane's batch (recount.cpp): what kmcpg_recount_log_device does, without the public entry's argument checks
int recount_enqueue(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers, const int32_t* d_qlen,
                    uint32_t n_reads, int32_t final_n, const uint64_t* d_n_hits, uint64_t hit_cap, uint8_t* d_left, unsigned max_wgs, hipStream_t st);
// K7 behind K3 for a lane's batch (cooccur.cpp): what kmcpg_cooccur_device does, without the public entry's argument checks (max_wgs 0: the handle's)
int cooccur_enqueue(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers, uint32_t n_reads,
                    int32_t final_n, const uint64_t* d_n_hits, uint64_t hit_cap, uint8_t* d_left, unsigned max_wgs, hipStream_t st);
// K10 behind the counting stages for a lane's batch (stats.cpp).  left_compact_reserve: the handle's scratch for n_reads reads — called
// before the counting kernels are enqueued, so that nothing behind them fails for want of memory.  left_compact_enqueue: what
// kmcpg_left_compact_device does, without the public entry's argument checks; d_stats = K10_STATS witness words of the caller's (a lane's:
// batches in flight keep theirs apart), zeroed here, or nullptr: the handle's
int left_compact_reserve(kmcpg_db* db, uint32_t n_reads);
int left_compact_enqueue(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, uint32_t n_reads, const uint8_t* const d_left[N_COUNTING],
                         const uint64_t* d_n_hits, uint64_t hit_cap, uint8_t* d_mask, kmcpg_pair* d_left_pairs, uint64_t left_cap, uint64_t* d_left_offs,
                         unsigned long long* d_stats, hipStream_t st);
// K11 behind K3 (binning.cpp): what kmcpg_bin_device does, without the public entry's argument checks.  d_left: nullptr, or a byte per
// read, 1 where the bin is LEFT (what K10's compaction takes); d_stats = K11_STATS witness words of the caller's (a lane's), zeroed here, or
// nullptr: the handle's.  bins_left_host (finalize.cpp): the host half — the LEFT reads of bins[] from their pairs, after the host's own
// -f test, by bin_rule.hpp on the handle's copy of the plan; *host_reads counts them
int bin_enqueue(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers, uint32_t n_reads, int32_t final_n,
                const uint64_t* d_n_hits, uint64_t hit_cap, uint32_t* d_bins, uint8_t* d_left, unsigned long long* d_stats, hipStream_t st);
void bin_stats_from_words(const unsigned long long* words, kmcpg_bin_stats* out);  // the K11_STATS witness words -> the public form
int bins_left_host(kmcpg_db* db, const kmcpg_pair* pairs, const uint64_t* read_offs, const int32_t* qkmers, uint32_t n_reads, const kmcpg_params& p, uint32_t* bins,
                   uint64_t* host_reads);
// bound_n: what the kmcpg_query_device call(s) that produced the list actually did — every query of up to bound_n k-mers had the -f bound
// applied on the device, whichever kernel form served it (0: no bound table in that call).  query_device_after reports the value of its
// call; lane.cpp keeps it with the batch (Lane::bound_n) and hands it to the finalizer, which takes a compact segment as final only for
// n <= bound_n — it does not look at the environment again.
inline int k1_mode(const kmcpg_info& I) { return I.syncmer ? 2 : (I.minimizer ? 1 : 0); }  // syncmer > minimizer > plain (util-db-search.go:1052-1058)
// batches of whole genomes (segment forms of the k-mer stage, k1_plan.hpp): the ones whose k-mer kernels run beside the previous batch's COBS
// kernel by default — second workspace slot (query.cpp pick_slot) and second kernel stream (lane.cpp enqueue; bench.py does the same with its streams)
bool whole_genome_batch(const kmcpg_db* db, uint32_t max_read_len, bool paired);  // k1_whole_genomes (k1_plan.hpp) of the handle's database
// KMCPG_FPR_BOUND (default on): K2 leaves out counts that cannot pass -f for queries of up to 512 (1024) k-mers (query.cpp fpr_bound)
inline bool fpr_bound_enabled() {
  const char* e = getenv("KMCPG_FPR_BOUND");
  return !(e && atoi(e) == 0);
}
constexpr int kFprBoundAlways = 512;  // queries of up to this many k-mers are covered by the bound table whatever the batch holds
void result_publish(ResultOwner* o, uint32_t n_reads, int k_used, kmcpg_result* out);
// A batch on the device, as the GPU half is told about it (query.cpp run_kmers, query_device_after): text, or — `packed` — 2-bit codes
// that the k-mer stage reads as they are or expands into d_seqs; its queries are the reads themselves, or — `windows` — views into them.
struct DeviceBatch {
  const uint8_t* d_seqs = nullptr;
  const uint64_t* d_offs = nullptr;
  const uint8_t* d_seqs2 = nullptr;  // mates or nullptr
  const uint64_t* d_offs2 = nullptr;
  uint32_t n_reads = 0;
  uint64_t total_bases = 0;  // of the queries, both mates
  uint32_t max_read_len = 0;
  PackedSrc packed;
  WindowSrc windows;
};
// A staged piece of sliding windows on the device (host_windows.cpp submit_window_piece_device stages it, window_plan.hpp states what it
// holds): the slices' text, their four prefix arrays, and where the descriptors k_window_desc builds from them go.  Stated once for the
// lanes (lane.cpp) and for the entry that runs the k-mer stage alone on such a piece (kmcpg_kmers_device_windows).
struct WindowPiece {
  const uint8_t* d_text = nullptr;  // the slices one behind the other, 16 readable bytes behind the last
  const uint64_t *d_soffs = nullptr, *d_wpre = nullptr, *d_vpre = nullptr, *d_cpre = nullptr;  // [ns + 1] each
  uint32_t ns = 0;
  uint64_t sb = 0, n_chunks = 0;  // staged bases (= soffs[ns]); chunks of K1_WIN_CHUNK k-mer positions (= cpre[ns])
  uint32_t n_win = 0, wmax = 0;   // windows; the longest of them
  uint64_t bases = 0;             // of all windows (= vpre[ns])
  uint64_t step = 0, window = 0;
  uint64_t* d_src = nullptr;   // [n_win]      k_window_desc: each window's first base in the staged text
  uint64_t* d_offs = nullptr;  // [n_win + 1]  ... and its place in the window numbering
  // the batch the GPU half is told about: the windows are its queries, read in place through d_src
  DeviceBatch batch() const {
    DeviceBatch b{d_text, d_offs, nullptr, nullptr, n_win, bases, wmax};
    b.windows.src = d_src;
    b.windows.soffs = d_soffs;
    b.windows.wpre = d_wpre;
    b.windows.cpre = d_cpre;
    b.windows.ns = ns;
    b.windows.n_chunks = n_chunks;
    b.windows.sb = sb;
    b.windows.step = step;
    b.windows.window = window;
    return b;
  }
};
// query.cpp: the piece's descriptors, enqueued in front of the k-mer kernels that read through them
int describe_windows(const WindowPiece& w, hipStream_t st);
// host_windows.cpp: the window specs every sliding-window entry refuses (KMCPG_EINVAL)
int window_spec_args(const kmcpg_window_spec* spec);
// where the outputs of kmcpg_query_device go
struct QueryOut {
  kmcpg_hit* d_hits;
  uint64_t hit_cap;
  uint64_t* d_counters;
  int32_t *d_qkmers, *d_qlen;
};
// query.cpp: kmcpg_query_device with a prologue run under the handle's enqueue lock, in front of the batch's first kernel.
// *bound_n (optional): see finalize_grouped_trusted
int query_device_after(kmcpg_db* db, const DeviceBatch& b, const kmcpg_params* params, const QueryOut& out, void* stream, const std::function<int()>* prologue,
                       int32_t* bound_n);
void result_records_to_pairs(ResultOwner* o);  // finalize.cpp: a result that holds records -> the pairs of a compact result

}  // namespace kmcpg
