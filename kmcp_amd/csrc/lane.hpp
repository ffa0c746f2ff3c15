// lane.hpp — internals shared by the translation units of the whole pipeline on host buffers (kmcpg_submit / kmcpg_wait / kmcpg_search_batch
// and their kin).  Not part of the ABI.
//
//   lane.cpp          a batch in flight: lanes and streams of a handle, staging and the 2-bit upload, enqueue, collect, drop_ticket
//   host.cpp          what is above a lane: submit, the host half of wait, the retry walk, the pieces of kmcpg_search_batch, the entries
//   host_windows.cpp  sliding windows: pieces of windows, their two submit paths, the join of their results, the window entries
//   host_handles.cpp  handles over several GPUs and over an index larger than HBM; the bench / parity read-back entries
//   host_pack.cpp     the 2-bit packer for hosts, pinned memory for callers, kmcpg_submit_packed
//
// A handle owns a few non-blocking streams and a few LANES; a lane is the staging of one batch in flight (pinned host input and output
// buffers, device input and output buffers, a completion event).  kmcpg_submit copies the caller's batch into a free lane, enqueues
// H2D + K1 + K2 + D2H on the streams and returns; kmcpg_wait waits for the lane's event and runs the host half (float64 thresholds, FPR,
// sort) on the calling thread, so the GPU works on the next batches meanwhile.  The number of lanes bounds the batches in flight the way
// the reference's token channel bounds its queries (util-db-search.go:243, :347-351).  Retries (--try-se, smaller k of a multi-k
// database) are rare, small and synchronous; they run on a lane of their own so that they never wait for a lane another waiter holds.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"
#include "engine.hpp"

namespace kmcpg {

template <typename T>
struct PinBuf {
  T* p = nullptr;
  size_t cap = 0;
  int ensure(size_t n) {
    if (n <= cap) return 0;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = n + n / 8 + 64;
    if (hipHostMalloc((void**)&p, want * sizeof(T), hipHostMallocPortable) != hipSuccess) return -1;
    cap = want;
    return 0;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct Lane {
  PinBuf<uint8_t> h_seqs, h_seqs2;
  PinBuf<uint64_t> h_offs, h_offs2, h_cnt;
  PinBuf<int32_t> h_qk, h_ql;
  PinBuf<kmcpg_hit> h_hits;
  DevBuf<uint8_t> d_seqs, d_seqs2;
  DevBuf<uint64_t> d_offs, d_offs2, d_cnt;
  DevBuf<int32_t> d_qk, d_ql;
  DevBuf<kmcpg_hit> d_hits;
  // K3 (device half of finalize): the batch's matches grouped by read and in final order, 8 bytes each + CSR offsets of the reads
  DevBuf<kmcpg_pair> d_pairs;
  DevBuf<uint64_t> d_roffs;
  PinBuf<kmcpg_pair> h_pairs;
  PinBuf<uint64_t> h_roffs;
  // K4 (the species-specific stage, when the handle has it on): the surviving segments go into d_hits — dead once K3 has grouped it, and
  // half again as large as the pairs need —, their offsets and the verdict bytes beside them; d_final = where the batch's final pairs are
  DevBuf<uint64_t> d_soffs4;
  DevBuf<uint8_t> d_verd;
  PinBuf<uint8_t> h_verd;
  const kmcpg_pair* d_final = nullptr;
  // K5 (window summaries, kmcpg_submit_windows_summary): the batch's result is h_sum, 16 bytes per window; the pairs of the windows LEFT
  // to the host lie in d_pairs (= d_final) one behind the other and come down on demand; of K3's offsets only the last two words do
  bool summary = false;  // the caller asked for summaries (set after lane_begin, before enqueue)
  DevBuf<kmcpg_window_summary> d_sum;
  PinBuf<kmcpg_window_summary> h_sum;
  DevBuf<uint64_t> d_loffs;
  bool summarized() const { return summary && grouped && spec; }  // K5 ran: h_sum is the result
  // The counting stages (K6, K7, K8: engine.hpp), each when the handle has it on: a byte per read — 1 = LEFT to the host half, which counts
  // it from K3's pairs at collect time; with K4 on as well, K3's own offsets come down beside K4's (h_roffs3) and K3's pairs only if a read was LEFT
  DevBuf<uint8_t> d_left[N_COUNTING];
  PinBuf<uint8_t> h_left[N_COUNTING];
  PinBuf<uint64_t> h_roffs3;
  unsigned counted = 0;  // bit s: this batch went through counting stage s
  // K10 (statistics-only batches, kmcpg_submit_stats): behind the counting stages the bytes of d_left become one mask byte per read and the
  // LEFT reads' segments are compacted into d_hits (= d_final; offsets in d_loffs) — dead once K3 has grouped it; the mask and the lane's own
  // witness words come down with the batch, the offsets and the pairs on demand (collect); of K3's offsets only the last two words do
  bool stats = false;  // the caller asked for statistics only (set after lane_begin, before enqueue)
  DevBuf<uint8_t> d_mask;
  PinBuf<uint8_t> h_mask;
  DevBuf<unsigned long long> d_lstats;
  PinBuf<unsigned long long> h_lstats;
  PinBuf<uint64_t> h_loffs;
  bool stats_only() const { return stats && grouped && counted != 0; }  // K10 ran: left_res is the result (after collect)
  kmcpg_stats_ticket_stats left_res{};
  // K11 (binning batches, kmcpg_submit_bins): behind K3 one word per read, the bin, and a byte for the reads K11 LEFT, which K10's compaction
  // takes as a stage's byte (d_mask, d_loffs, d_lstats, d_hits as above); the bins and the two witnesses come down with the batch, qkmers,
  // the offsets and the LEFT pairs on demand (collect) — no counting stage runs, and of K3's offsets only the last two words come down
  bool bins = false;  // the caller asked for bins only (set after lane_begin, before enqueue)
  DevBuf<uint32_t> d_bins;
  PinBuf<uint32_t> h_bins;
  DevBuf<uint8_t> d_bleft;
  DevBuf<unsigned long long> d_bstats;
  PinBuf<unsigned long long> h_bstats;
  bool bins_only() const { return bins && grouped; }  // K11 ran: bin_res is the result (after collect)
  kmcpg_bin_stats bin_res{};
  uint64_t bin_left_pairs = 0, bin_bytes_d2h = 0, bin_kept_pairs = 0;
  uint32_t reruns = 0;  // how often collect() ran the batch again after a hit-buffer overflow (the witness of kmcpg_result_bins)
  bool spec = false;  // this batch went through K4: h_roffs / h_pairs hold ITS output, h_verd the verdicts
  // 2-bit packed upload (stage): the batch's bases as codes + the runs of foreign bytes instead of h_seqs; unpacked on the device
  PinBuf<uint8_t> h_pack;
  PinBuf<ExcRun> h_exc;
  DevBuf<uint8_t> d_pack;
  DevBuf<ExcRun> d_exc;
  // what goes up (stage / stage_packed): up_reads reads of up_bases bases with h_offs = their offsets, as text in h_seqs or — packed — as codes
  // + n_exc runs; single reads, or — paired — their mates beside them (tb2 bases)
  uint32_t up_reads = 0;
  uint64_t up_bases = 0;
  bool packed = false;
  uint32_t n_exc = 0;
  const uint8_t* ext_pack = nullptr;  // codes that live in the CALLER's pinned memory (kmcpg_host_alloc): uploaded from there, no staging copy
  // what is searched: n queries of tb1 (+ tb2) bases, the longest of maxlen.  They are the staged reads themselves (as stage leaves it), or —
  // win, kmcpg_submit_windows — windows over them: h_wmeta = the staged slices' window prefix and window-base prefix (2 x (up_reads + 1)); the
  // device builds d_offs (the windows' numbering) and d_wsrc (each window's first base in d_seqs) from d_soffs + d_wmeta (windows.hip).
  // A third array in h_wmeta: the slices' chunks of K1_WIN_CHUNK k-mer positions (wchunks in all), for the hash-once form of K1.
  uint32_t n = 0;
  bool paired = false;
  uint64_t tb1 = 0, tb2 = 0;
  uint32_t maxlen = 0;
  bool win = false;
  uint64_t wstep = 0, wwin = 0, wchunks = 0;
  PinBuf<uint64_t> h_wmeta;
  DevBuf<uint64_t> d_soffs, d_wmeta, d_wsrc;
  int32_t bound_n = 0;   // the -f bound of the LAST kmcpg_query_device call for this batch covered queries of up to this many k-mers
  bool grouped = false;  // this batch went through K3: h_pairs / h_roffs hold its result, h_hits is not filled
  hipEvent_t k3_ev = nullptr, eager_ev = nullptr;  // K3 done on the kernel stream -> the eager copy of the pairs on the copy stream
  bool eager_aside = false;                        // ... when it was put there (pieces of a large kmcpg_search_batch call)
  hipEvent_t done = nullptr, uploaded = nullptr;
  hipStream_t st = nullptr;  // the kernel stream this batch was enqueued on (AsyncState::stream or stream2, taken in turn)
  uint64_t copied = 0;  // hits already on their way to h_hits when `done` fires
  bool busy = false;
  void release() {
    h_seqs.release(); h_seqs2.release(); h_offs.release(); h_offs2.release(); h_cnt.release(); h_qk.release(); h_ql.release(); h_hits.release();
    d_seqs.release(); d_seqs2.release(); d_offs.release(); d_offs2.release(); d_cnt.release(); d_qk.release(); d_ql.release(); d_hits.release();
    d_pairs.release(); d_roffs.release(); h_pairs.release(); h_roffs.release();
    d_soffs4.release(); d_verd.release(); h_verd.release();
    d_sum.release(); h_sum.release(); d_loffs.release();
    for (auto& b : d_left) b.release();
    for (auto& b : h_left) b.release();
    h_roffs3.release();
    d_mask.release(); h_mask.release(); d_lstats.release(); h_lstats.release(); h_loffs.release();
    d_bins.release(); h_bins.release(); d_bleft.release(); d_bstats.release(); h_bstats.release();
    h_pack.release(); h_exc.release(); d_pack.release(); d_exc.release();
    h_wmeta.release(); d_soffs.release(); d_wmeta.release(); d_wsrc.release();
    if (done) (void)hipEventDestroy(done);
    if (uploaded) (void)hipEventDestroy(uploaded);
    if (k3_ev) (void)hipEventDestroy(k3_ev);
    if (eager_ev) (void)hipEventDestroy(eager_ev);
    done = uploaded = k3_ev = eager_ev = nullptr;
  }
};

struct AsyncState {
  hipStream_t stream = nullptr;
  hipStream_t copy_stream = nullptr;  // late D2H of a finished batch's hits: must not queue behind the kernels of later batches
  // (Exactly three streams per handle beside the null stream: the runtime multiplexes HIP streams onto 4 hardware queues, and a
  // fifth stream — tried for the pieces' eager copies — made uploads and kernels share one: -8 % on the pipelined path, same-box A/B.)
  hipStream_t up_stream = nullptr;    // H2D of a batch's reads, beside the kernels of the batches before it
  // a second kernel stream: consecutive batches alternate between the two, so that the k-mer kernels of one run beside the COBS
  // kernels of the one before it (with KMCPG_WS_SLOTS=2 the handle keeps two k-mer workspaces, engine.hpp).  Off unless KMCPG_KSTREAMS=2: measured a loss on
  // four of five workloads (profiles/r05_k1_beside_k2.txt)
  hipStream_t stream2 = nullptr;
  int kstreams = 0;  // KMCPG_KSTREAMS: 2 = consecutive batches alternate between the two kernel streams, 1 = never, 0 (unset) = batches of whole genomes only
  uint64_t enqueued = 0;
  std::atomic<uint64_t> hits_hint{0};  // hits per 1024 reads seen lately: sizes the hit buffers and the eager D2H of the next batches (lane_plan.hpp)
  uint64_t lane_hit_budget = 0;        // entries a lane's device hit buffer may grow to beyond the plain size (from free HBM at first use)
  bool hits_stay_on_device = false;    // shard of a handle that gathers the hit lists over RCCL: no per-shard D2H of hits
  bool device_finalize = true;         // K3 after K2: grouping, -T and the per-query order on the GPU (KMCPG_DEVICE_FINALIZE=0: host)
  std::vector<std::unique_ptr<Lane>> lanes;
  size_t max_lanes = 4;
  std::mutex mu;
  std::condition_variable cv;
  Lane retry;
  std::mutex retry_mu;
};

// a batch in the caller's memory, as the entry points take it: n reads, seqs2 / offs2 = their mates or nullptr
struct HostBatch {
  const uint8_t* seqs;
  const uint64_t* offs;
  const uint8_t* seqs2;
  const uint64_t* offs2;
  uint32_t n;
};

// A batch that arrives as 2-bit codes + exception runs (kmcpg_submit_packed): the staging copy is a quarter of the text's; from the
// upload on the lane looks exactly like one whose text stage() packed itself.
struct PackedIn {
  const uint8_t* codes;
  const kmcpg_exc_run* exc;
  uint64_t n_exc;
};

// the summaries of a batch (or of one piece of it) with what the witness counts (kmcpg_last_summary)
struct SummaryPart {
  std::vector<int32_t> qlen, qkmers;
  std::vector<kmcpg_window_summary> s;
  uint64_t single = 0, wave = 0, left = 0, empty = 0;  // windows by who summarised them: the device (one target, several), the host, nobody (no rows)
  uint64_t left_pairs = 0, bytes_d2h = 0;
  void count(const SummaryPart& o) {
    single += o.single, wave += o.wave, left += o.left, empty += o.empty, left_pairs += o.left_pairs, bytes_d2h += o.bytes_d2h;
  }
};

}  // namespace kmcpg

// one batch in flight; single-device handles have one part, kmcpg_open_devices handles one part per GPU
struct kmcpg_ticket {
  kmcpg_db* db = nullptr;
  struct Part {
    kmcpg_db* shard;
    kmcpg::Lane* lane;
    bool retry;
  };
  std::vector<Part> parts;
  uint32_t n = 0;
  bool paired = false;
  kmcpg_params p{};
  // the batch as staged (retries re-read it): the first lane's pinned copy, or — paged handles — the ticket's own
  const uint8_t* S[2] = {nullptr, nullptr};
  const uint64_t* O[2] = {nullptr, nullptr};
  // paged handles (kmcpg_open_paged): the search ran inside kmcpg_submit, one resident shard after the other; results wait here
  bool paged = false;
  std::vector<uint8_t> seqs, seqs2;
  std::vector<uint64_t> offs, offs2;
  std::vector<kmcpg_hit, kmcpg::NoInitAlloc<kmcpg_hit>> hits;
  std::vector<int32_t> qk, ql;
  // sliding windows cut into pieces (kmcpg_submit_windows): the pieces' tickets in window order; a piece that was finished early to free a
  // lane for a later one has its result in piece_res[i] instead (pieces[i] == nullptr).  Such a ticket holds no lane itself.
  std::vector<kmcpg_ticket*> pieces;
  std::vector<kmcpg_result> piece_res;
  // kmcpg_submit_windows_summary: the ticket (and its pieces) is consumed by kmcpg_wait_summaries only; a piece finished early has its
  // summaries in piece_sum[i]
  bool summary = false;
  std::vector<kmcpg::SummaryPart> piece_sum;
  // kmcpg_submit_stats: the ticket is consumed by kmcpg_wait_stats only
  bool stats = false;
  // kmcpg_submit_bins: the ticket is consumed by kmcpg_wait_bins only
  bool bins = false;
};

namespace kmcpg {
#pragma GCC visibility push(hidden)  // (the library's dynamic symbols stay the ABI's)

// ---- rules every unit states the same way
// Is the batch's text read again after it was staged?  The smaller k of a database with several k-mer sizes searches it again (retry_unmatched).
inline bool rereads_text(const kmcpg_db* db, const kmcpg_params& p) { return p.k <= 0 && db->ks_desc.size() > 1; }
// Can a query of this batch be searched a second time (retry_unmatched: --try-se on pairs, the next smaller k)?  Such batches collect Match
// records — the sub-results are spliced in record by record —, go through whole, and keep their text as text.
inline bool may_retry(const kmcpg_db* db, const kmcpg_params& p, bool paired) { return (p.try_se && paired) || rereads_text(db, p); }

// runs a cleanup and keeps the calling thread's error text across it
template <class F>
void keeping_error(F&& cleanup) {
  const std::string keep = kmcpg_err_ref();
  cleanup();
  kmcpg_err_ref() = keep;
}
int fail_all_lanes_busy(const AsyncState* A);  // KMCPG_EBUSY

// the one way to make a handle's streams idle (the caller has made the handle's device current)
void drain(AsyncState* A);

// offsets start at 0 and never decrease; *maxlen = the longest read (either mate)
int check_offsets(const HostBatch& b, uint64_t* maxlen);
// exception runs of a packed batch of n_bases bases: the runs are written into the batch's text, they must lie inside it
int check_exc_runs(const kmcpg_exc_run* exc, uint64_t n_exc, uint64_t n_bases);

// ---- lane.cpp
int async_state(kmcpg_db* db, AsyncState** out);
// block = false: nullptr when every lane is in flight (kmcpg_submit never blocks: a caller that submits from one thread
// would otherwise wait for itself); block = true: wait for a lane (kmcpg_search_batch: whoever holds a lane through it gives
// it back without needing another one)
Lane* acquire_lane(AsyncState* A, bool retry, bool block);
void release_lane(AsyncState* A, Lane* l, bool retry);
// caller's batch -> the lane's pinned buffers (the caller may reuse its buffers as soon as kmcpg_submit returns)
int stage(Lane* L, const HostBatch& b, bool allow_pack = false);
int stage_packed(Lane* L, const PackedIn& in, const HostBatch& b);  // b: offsets and count (single reads; the bases are in.codes)
// H2D + K1 + K2 (+ K3) + D2H of one staged lane on the handle's streams; returns without waiting
int enqueue(kmcpg_db* db, AsyncState* A, Lane* L, const kmcpg_params& p, bool generous_eager = false);
// waits for the lane; afterwards h_hits[0..*n_hits), h_qk, h_ql are complete (fetch = false: the hits stay in d_hits[0..*n_hits),
// the caller gathers them on the device)
int collect(kmcpg_db* db, AsyncState* A, Lane* L, const kmcpg_params& p, uint64_t* n_hits, bool fetch = true);
void drop_ticket(kmcpg_ticket* t, bool failed = false);

// ---- host.cpp
// the submit family works on a handle that holds the whole database and can reach a GPU; *p = the caller's params or the defaults
int submit_handle(kmcpg_db* db, const kmcpg_params* params, kmcpg_params* p);
int submit_impl(kmcpg_db* db, const HostBatch& b, const kmcpg_params& p, bool retry, bool block, kmcpg_ticket** out, const PackedIn* packed = nullptr,
                bool summary = false, bool stats = false, bool bins = false);
// kmcpg_wait / kmcpg_wait_pairs: the ticket's result, as_pairs = in the compact form where the path it took collects that natively; gives the ticket back
int wait_impl(kmcpg_ticket* t, kmcpg_result* out, bool as_pairs);
// kmcpg_wait_summaries: the summaries of a ticket of kmcpg_submit_windows_summary (one batch or its pieces); gives the ticket back
int wait_summary_impl(kmcpg_ticket* t, SummaryPart* out);
// np results (of n reads together) one behind the other as one result, in the form asked for — a part that arrived in the other form is
// converted; the parts are freed
void concat_results(const kmcpg_db* db, kmcpg_result* parts, size_t np, uint32_t n, bool as_pairs, int k_used, kmcpg_result* out);

// ---- host_windows.cpp
int wait_pieces(kmcpg_ticket* t, kmcpg_result* out, bool as_pairs);

// ---- host_handles.cpp
int search_paged(kmcpg_db* front, const HostBatch& b, const kmcpg_params& p, kmcpg_ticket* t);

#pragma GCC visibility pop
}  // namespace kmcpg
