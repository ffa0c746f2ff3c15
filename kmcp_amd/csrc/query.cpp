// query.cpp — the GPU half behind the C ABI: k-mer generation (K1, K1d) and the COBS query (K2) on device pointers.
// Reference counterparts: generateKmers (util-db-search.go:1037-1107), dedup (:874-908), the UnikIndex workers (:6611-7742).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "dbformat.hpp"
#include "engine.hpp"
#include "fpr.hpp"
#include "kernels.hpp"

using namespace kmcpg;

namespace kmcpg {
void release_fpr_bounds(kmcpg_db* db) {
  for (auto& t : db->fpr_bounds) {
    if (t.d) (void)hipFree(t.d);
    if (t.h) (void)hipHostFree(t.h);
  }
  db->fpr_bounds.clear();
}
}  // namespace kmcpg

// ------------------------------------------------------------------------------------------------
// GPU half
// ------------------------------------------------------------------------------------------------
bool kmcpg::whole_genome_batch(const kmcpg_db* db, uint32_t max_read_len, bool paired) { return k1_whole_genomes(k1_mode(db->info), paired, max_read_len); }

namespace {

uint64_t max_hash_for(uint32_t scale) {
  // uint64(float64(^uint64(0)) / float64(scale))  (util-db-search.go:1040-1043)
  const double d = 18446744073709551616.0 / (double)scale;
  if (d >= 18446744073709551616.0) return ~0ULL;
  return (uint64_t)d;
}

// where the k-mer stage writes: d_scratch (optional) is two halves of scratch_half words, the counters are per read
struct KmerOut {
  uint64_t *d_hashes, *d_scratch;
  uint64_t scratch_half;
  int32_t *d_nk_raw, *d_nk1, *d_nk_search, *d_qlen;
};

// The K1 knobs.  KMCPG_K1_FLAGS, KMCPG_WR_WAVES and KMCPG_K1_DEBUG are read at every call (tests flip them inside one
// process), KMCPG_K1_CODES and KMCPG_WIN_ONCE once per process.
K1Knobs k1_knobs() {
  static const int codes_mode = getenv("KMCPG_K1_CODES") ? atoi(getenv("KMCPG_K1_CODES")) : 1;
  static const bool win_once = !getenv("KMCPG_WIN_ONCE") || atoi(getenv("KMCPG_WIN_ONCE")) != 0;
  K1Knobs kn;
  if (const char* e = getenv("KMCPG_K1_FLAGS")) kn.flags = atoi(e);
  if (const char* e = getenv("KMCPG_WR_WAVES")) kn.wr_waves = atoi(e);
  kn.codes_mode = codes_mode;
  kn.win_once = win_once;
  kn.debug = getenv("KMCPG_K1_DEBUG") != nullptr;
  return kn;
}

// The K2 knobs read per query, all of them at every call: tests flip them inside one process.  (The knobs of the lane
// cutting are read at open: engine.cpp k2_open_knobs.)
K2Knobs k2_knobs() {
  K2Knobs kn;
  if (const char* e = getenv("KMCPG_SPLIT_MIN")) kn.split_min = atoi(e), kn.split_min_set = true;
  if (const char* e = getenv("KMCPG_SPLIT_CHUNK")) kn.split_chunk = atoi(e), kn.split_chunk_set = true;
  if (const char* e = getenv("KMCPG_NT_LOADS")) kn.nt_loads = atoi(e);
  if (const char* e = getenv("KMCPG_PRUNE")) kn.prune = atoi(e);
  if (const char* e = getenv("KMCPG_GROUP_ROWS")) kn.group_rows = atoi(e), kn.group_rows_set = true;
  if (const char* e = getenv("KMCPG_PRUNE_EVERY")) kn.prune_every = atoi(e);
  // slot-major unit order: the waves in flight share one (block, tile) slice of the index, so the address range they gather
  // from is ~1/64 of the index (GTDB scale: 575 -> 510 ms per 524 k reads; profiles/r02_order_exp.txt)
  if (const char* e = getenv("KMCPG_SLOT_MAJOR")) kn.slot_major = atoi(e);
  // tail mode of the 16/24-plane kernels on 1-KiB tiles (k2_cobs.hip): KMCPG_TAIL_SECTORS=0 switches it off
  // (2, not 4: a wave that enters with 3-4 live sectors carries near misses that would have died a little later through the rest of the
  // query, unpruned — same-box A/B on the genome search: 5.05 ms without, 4.74 with 2, 4.93 with 4; profiles/r06_tail_mode.txt)
  if (const char* e = getenv("KMCPG_TAIL_SECTORS")) kn.tail_sectors = std::max(0, std::min(atoi(e), 4));
  if (const char* e = getenv("KMCPG_TAIL_MIN")) kn.tail_min = std::max(1, atoi(e));
  if (const char* e = getenv("KMCPG_PAIR")) kn.pair = atoi(e) != 0;
  if (const char* e = getenv("KMCPG_K2_BLOCK_UNITS")) kn.block_units = atoi(e) != 0;
  if (const char* e = getenv("KMCPG_K2_EXACT_STOP")) kn.exact_stop = atoi(e) != 0;
  // the short-read launch of the 64-lane class as resident waves that take their units from a queue (k2_cobs.hip k2_cobs_persist)
  if (const char* e = getenv("KMCPG_K2_PERSIST")) kn.persist = atoi(e) != 0;
  if (const char* e = getenv("KMCPG_K2_PERSIST_WGS")) kn.persist_wgs = (uint32_t)std::max(0, atoi(e));
  return kn;
}

// K1d, the dedup stage of the k-mer step: every query's list sorted + unique where its raw count is above -u, NumKmers (0 below -m, tested
// on the raw count) in d_nk_search.  Query r's list is d_hashes[d_offs[r] (+ d_offs2[r]) ...], d_nk_raw[r] long; max_n bounds every
// raw count; pre / pre_done / key_shift: DedupArgs (common.hpp).  Called by the k-mer stage and by kmcpg_dedup_device.
struct DedupLists {
  uint64_t *d_hashes, *d_scratch;
  const uint64_t *d_offs, *d_offs2;
  const int32_t* d_nk_raw;
  int32_t* d_nk_search;
};

int run_dedup(kmcpg_db* db, kmcpg_db::Workspace& W, const DedupLists& o, uint32_t n_reads, uint64_t max_n, const kmcpg_dedup_spec& s, hipStream_t st) {
  db->dedup_log.clear();
  db->dedup_fb = nullptr;
  DedupLog* const log = db->profiling >= 1 ? &db->dedup_log : nullptr;  // the launch sites write it, kmcpg_last_dedup_launches reads it
  if (max_n > (uint64_t)s.dedup_threshold) {
    dedup_note(log, KMCPG_DD_LAUNCH_DEDUP, 0, 0, 0, 0, 0, 0, 0);
    DedupArgs d{};
    d.offs = o.d_offs;
    d.offs2 = o.d_offs2;
    d.n_reads = n_reads;
    d.dedup_threshold = s.dedup_threshold;
    d.min_matched = s.min_matched;
    d.hashes = o.d_hashes;
    d.scratch = o.d_scratch;
    d.nk_raw = o.d_nk_raw;
    d.nk_search = o.d_nk_search;
    d.pre = s.pre;
    d.pre_done = s.pre_done;
    d.key_shift = s.key_shift;
    if (log) {  // the witness of the distribution classes: how many queries each sent to its fallback (read by kmcpg_last_dedup_launches)
      if (W.w_dedup_fb.ensure(4)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
      HIPCHK(hipMemsetAsync(W.w_dedup_fb.p, 0, 4 * sizeof(uint32_t), st));
      d.fallbacks = W.w_dedup_fb.p;
      db->dedup_fb = W.w_dedup_fb.p;
    }
    // KMCPG_DEDUP_BIG_BUCKET is read at every call, as the K1 knobs are: tests flip it inside one process
    const char* const bb = getenv("KMCPG_DEDUP_BIG_BUCKET");
    launch_dedup(d, max_n, !(bb && atoi(bb) == 0), st, log);
    if (max_n > HUGE_MIN) {
      // whole-genome queries: which ones they are is only known on the device -> one small read-back, then a device-wide
      // sort + unique per such query
      const int32_t thr = std::max<int32_t>((int32_t)HUGE_MIN, s.dedup_threshold);
      uint32_t meta[2] = {0, 0};
      if (W.w_long_list.ensure(n_reads + 1) || W.w_long_meta.ensure(2)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
      HIPCHK(hipMemsetAsync(W.w_long_meta.p, 0, 2 * sizeof(uint32_t), st));
      launch_list_long(o.d_nk_raw, n_reads, thr, W.w_long_list.p, W.w_long_meta.p, st);
      HIPCHK(hipMemcpyAsync(meta, W.w_long_meta.p, sizeof meta, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (meta[0]) {
        const size_t tb = huge_dedup_temp_bytes(meta[1]);
        if (W.w_huge_info.ensure(3 * (size_t)meta[0] + 1) || W.w_huge_temp.ensure(tb + 64)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
        launch_gather_huge(W.w_long_list.p, meta[0], o.d_nk_raw, o.d_offs, o.d_offs2, W.w_huge_info.p, st);
        std::vector<uint64_t> hinfo(3 * (size_t)meta[0]);
        HIPCHK(hipMemcpyAsync(hinfo.data(), W.w_huge_info.p, hinfo.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        int* d_num = (int*)W.w_huge_temp.p;  // first 64 bytes: the unique count
        for (uint32_t i = 0; i < meta[0]; i++) {
          const uint32_t r = (uint32_t)hinfo[3 * i], n = (uint32_t)hinfo[3 * i + 1];
          const uint64_t koff = hinfo[3 * i + 2];
          if (huge_dedup(o.d_hashes + koff, o.d_scratch + koff, n, d_num, W.w_huge_temp.p + 64, tb, o.d_nk_search, r, s.min_matched, st, log) != 0)
            return kmcpg_fail(KMCPG_EDEVICE, "device-wide sort of a %u-k-mer query failed", n);
        }
      }
    }
  } else {
    dedup_note(log, KMCPG_DD_NK_SIMPLE, 0, 0, 0, 0, 0, 0, 0);
    launch_nk_simple(o.d_nk_raw, o.d_nk_search, n_reads, s.min_matched, st);
  }
  return 0;
}

// K1 (+K1d): hashes of read i end up at d_hashes[offs[i] + offs2[i] ...], NumKmers in d_nk_search
int run_kmers(kmcpg_db* db, kmcpg_db::Workspace& W, const DeviceBatch& b, const kmcpg_params& p, const KmerOut& o, hipStream_t st, uint64_t* max_n_out) {
  const kmcpg_info& I = db->info;
  db->k1_log.clear();
  db->k1_left = nullptr;
  K1Log* const k1_log = db->profiling >= 1 ? &db->k1_log : nullptr;  // launch_k1 writes it, kmcpg_last_k1_launches reads it
  if (!I.canonical) return kmcpg_fail(KMCPG_EUNSUPPORTED, "non-canonical index");
  const PackedSrc& src = b.packed;   // a batch that came as 2-bit codes (host_pack.cpp kmcpg_submit_packed, or text that lane.cpp stage() packed)
  const WindowSrc& win = b.windows;  // sliding windows (host_windows.cpp kmcpg_submit_windows): every kernel reads a window's bases in place through its view
  // which kernels, on what side buffer (k1_plan.hpp)
  K1Shape s;
  s.mode = k1_mode(I);
  s.k = p.k > 0 ? p.k : I.k;
  s.w_or_s = I.syncmer ? I.syncmer_s : I.minimizer_w;
  s.paired = b.d_seqs2 != nullptr;
  s.n_reads = b.n_reads;
  s.max_read_len = b.max_read_len;
  s.have_scratch = o.d_scratch != nullptr;
  s.dedup_threshold = p.dedup_threshold;
  s.win = {win.src != nullptr, win.step, win.window, win.sb, win.n_chunks};
  s.packed = {src.codes != nullptr, src.n_exc, src.n_bases, src.text == b.d_seqs};
  s.knobs = k1_knobs();
  const K1Plan plan = k1_plan(s);
  if (W.w_seg_cnt.ensure(plan.side_words) || W.w_win_h.ensure(plan.win_words) || W.w_win_kept.ensure(plan.win_words) || W.w_win_rank.ensure(plan.win_words) ||
      W.w_win_cnt.ensure(plan.win_chunk_words) || W.w_win_cbase.ensure(plan.win_chunk_words))
    return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
  uint32_t* const side = (uint32_t*)W.w_seg_cnt.p;
  auto side_at = [side](const K1Region& r) { return r.len ? side + r.off : nullptr; };
  K1Args a{};
  a.seqs = b.d_seqs;
  a.offs = b.d_offs;
  a.seqs2 = b.d_seqs2;
  a.offs2 = b.d_offs2;
  a.n_reads = b.n_reads;
  a.k = s.k;
  a.min_qlen = p.min_qlen;
  a.scaled = I.scaled;
  a.max_hash = I.scaled ? max_hash_for(I.scale) : ~0ULL;
  a.mode = s.mode;
  a.w_or_s = s.w_or_s;
  a.hashes = o.d_hashes;
  a.scratch = o.d_scratch;
  a.scratch2 = o.d_scratch ? o.d_scratch + o.scratch_half : nullptr;
  a.nk_raw = o.d_nk_raw;
  a.nk1 = o.d_nk1;
  a.qlen = o.d_qlen;
  a.flags = s.knobs.flags;
  a.seg_cnt = (int32_t*)side_at(plan.counts);
  a.segs_max = plan.segs;
  a.seg_nflag = side_at(plan.counter);
  a.seg_list = side_at(plan.list);
  a.seg_exc = side_at(plan.marks);
  a.seg_only_flagged = plan.list_fallback;
  a.nk_adj = o.d_nk_search;
  a.dedup_threshold = p.dedup_threshold;
  a.src = win.src;
  // packed input: k1_seg_roll2 reads the codes as they are, and text exists only for the segments a foreign byte reaches; every other form
  // reads text, expanded here
  if (src.codes) {
    if (plan.codes_direct) {
      a.codes = src.codes;
      a.exc = src.exc;
      a.n_exc = src.n_exc;
      a.seqs_w = src.text;
    } else {
      launch_unpack2(src.codes, src.text, src.n_bases, src.n_exc ? src.exc : nullptr, src.n_exc, st);
    }
    (plan.codes_direct ? db->k1_codes_direct : db->k1_codes_expanded)++;
  }
  if (k1_log) {  // the plan, once per call; what a list form leaves on its list is read by whoever synchronises anyway (kmers_device)
    static_assert((int)K1Form::None == KMCPG_K1F_NONE && (int)K1Form::WinOnce == KMCPG_K1F_WIN_ONCE && (int)K1Form::SegRoll2 == KMCPG_K1F_SEG_ROLL2 &&
                      (int)K1Form::SegRoll == KMCPG_K1F_SEG_ROLL && (int)K1Form::SegHash == KMCPG_K1F_SEG_HASH &&
                      (int)K1Form::WindowsRoll == KMCPG_K1F_WINDOWS_ROLL && (int)K1Form::WindowsWave == KMCPG_K1F_WINDOWS_WAVE &&
                      (int)K1Form::WgGlobal == KMCPG_K1F_WG_GLOBAL && (int)K1Form::Wg == KMCPG_K1F_WG && (int)K1Form::Short == KMCPG_K1F_SHORT,
                  "include/kmcp_gpu.h restates K1Form");
    kmcpg_k1_launch r{};
    r.kernel = KMCPG_K1_PLAN;
    r.p0 = (int)plan.form;
    r.p1 = (plan.codes_direct ? 1 : 0) | (plan.list_fallback ? 2 : 0) | (plan.adj_done ? 4 : 0);
    r.left_on_list = UINT32_MAX;
    k1_log->push_back(r);
    if (plan.form == K1Form::SegRoll2 || plan.form == K1Form::WindowsRoll) db->k1_left = a.seg_nflag;
  }
  launch_k1(a, plan, K1WinOnce{win, W.w_win_h.p, W.w_win_kept.p, W.w_win_rank.p, W.w_win_cnt.p, W.w_win_cbase.p}, st, k1_log);
  uint64_t ub = b.max_read_len >= (uint32_t)a.k ? (uint64_t)(b.max_read_len - a.k + 1) : 0;
  if (b.d_seqs2) ub *= 2;
  *max_n_out = ub;
  kmcpg_dedup_spec ds{};
  ds.dedup_threshold = p.dedup_threshold;
  ds.min_matched = p.min_matched;
  ds.pre = a.mode != 0;
  ds.pre_done = plan.adj_done;
  ds.key_shift = (I.scaled && a.max_hash) ? __builtin_clzll(a.max_hash) : 0;
  return run_dedup(db, W, DedupLists{o.d_hashes, o.d_scratch, b.d_offs, b.d_offs2, o.d_nk_raw, o.d_nk_search}, b.n_reads, ub, ds, st);
}

// The k-mer workspace exists twice (engine.hpp Workspace): calls are enqueued under db->mu and take the slots in turn; a call waits
// for the last kernel of the previous user of ITS slot, so the k-mer kernels of a batch may run beside the COBS kernels of the
// batch before it when the two calls are on different streams.  The second slot costs a second workspace (24 bytes per base of a
// batch): it is used only while that fits into a quarter of the free HBM (or is there already).
// Which batches: by default those of WHOLE GENOMES only (kmcpg::whole_genome_batch) — their k-mer stage is one fat VALU-bound kernel that fits
// beside the memory-bound COBS kernel of the batch before (genome search 47.2 -> 51.5 k genomes/s, profiles/r06_cobs_overlap.txt); on every other
// shape the second stream costs more in cross-stream waits than it hides (-3 ... -11 %, profiles/r05_k1_beside_k2.txt and the same file).
// KMCPG_WS_SLOTS=1: never, 2: every batch.
int pick_slot(kmcpg_db* db, uint64_t total_bases, bool whole_genomes) {
  static const int env = getenv("KMCPG_WS_SLOTS") ? atoi(getenv("KMCPG_WS_SLOTS")) : -1;
  if (env >= 0 ? env < 2 : !whole_genomes) return 0;
  // (by default not before the handle's fifth batch: the second workspace of a 256-Mbase batch is 6 GB to allocate and map, more than a run of
  // `kmcp-search -g` over a few hundred assemblies — four batches — can win back: 0.38 -> 0.49 s exec to exit when it was taken at once)
  // (... and then at once, with the fifth: a caller that warms up with five batches has the allocation behind it)
  if (env < 0 && db->ws_calls < 4) return 0;
  const int slot = (int)((db->ws_calls + (env < 0 ? 1 : 0)) & 1);
  if (slot == 0) return 0;
  kmcpg_db::Workspace& W = db->ws[1];
  if (W.w_hashes.cap >= total_bases + 1 && W.w_scratch.cap >= 2 * total_bases + 2) return 1;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 0;
  uint64_t limit = free_b;
  if (const char* e = getenv("KMCPG_HBM_LIMIT_MB")) limit = std::min<uint64_t>(limit, (uint64_t)std::max(0ll, atoll(e)) << 20);
  return 24 * (total_bases + 2) <= limit / 4 ? 1 : 0;
}

int ws_begin(kmcpg_db::Workspace& W, hipStream_t st) {
  if (!W.ev) HIPCHK(hipEventCreateWithFlags(&W.ev, hipEventDisableTiming));
  if (W.ev_valid) HIPCHK(hipStreamWaitEvent(st, W.ev, 0));
  return 0;
}

int ws_end(kmcpg_db::Workspace& W, hipStream_t st) {
  HIPCHK(hipEventRecord(W.ev, st));
  W.ev_valid = true;
  return 0;
}

// Every way out of a GPU-half call that has passed ws_begin leaves the event behind, error paths included: kernels that use
// the workspace may already be on the stream when a later step fails (an allocation, the FPR table, a launch), and the next
// user of the slot — possibly on another stream — must still be ordered behind them.
struct WsGuard {
  kmcpg_db::Workspace& W;
  hipStream_t st;
  hipStream_t kst = nullptr;  // the k-mer kernels' own stream when they have one (KMCPG_K1_STREAM=1), else == st
  bool armed = true;
  ~WsGuard() {
    if (!armed || !W.ev) return;
    // work queued on kst must be covered too: st waits for it first, then the slot's event on st stands for both streams
    if (kst != st && W.k1_ev && hipEventRecord(W.k1_ev, kst) == hipSuccess) (void)hipStreamWaitEvent(st, W.k1_ev, 0);
    if (hipEventRecord(W.ev, st) == hipSuccess) W.ev_valid = true;
  }
  int finish() {  // the success path: errors of the record are reported
    armed = false;
    return ws_end(W, st);
  }
};

// The reference drops a column whose FPR(n, count) exceeds -f right where it counts it (util-db-search.go:7474-7478); here
// that test runs on the host in float64, but the GPU can already leave out every count that cannot pass it: for each
// NumKmers n <= kFprBoundMaxN the smallest count c with FPR(n, c) <= max_fpr (the very values kmcpg_finalize compares, so a
// count below it fails there by definition; nothing is assumed about monotonicity).  With the defaults the query-coverage
// threshold is the stricter one; with -t just above the database's FPR it is this bound that keeps the hit list — and, through
// the pruning test, the row traffic — from exploding (n = 130, p = 0.3, -t 0.31: 45 % of all columns would be "hits").
// The table covers n <= 512 (every short read, single or paired up to 2 x 250; 18 ms of FPR rows on first use) and grows to
// 1024 when a batch may hold longer queries (+60 ms once).  Beyond ~1 100 k-mers the reference's FPR is numerically dead
// anyway: BinomialCoeff leaves the float64 range, the running value drops below zero and is clamped (util-fpr.go:32-50), so
// FPR(n, c) = 0 long before the crossing and the bound could never be the stricter threshold.
constexpr int kFprBoundMinN = kFprBoundAlways, kFprBoundMaxN = 1024;

int fpr_bound(kmcpg_db* db, double max_fpr, uint64_t max_kmers, hipStream_t st, const uint16_t** out, int32_t* out_n) {
  *out = nullptr;
  *out_n = 0;
  if (!fpr_bound_enabled()) return 0;
  int want_n = kFprBoundMinN;
  while (want_n < kFprBoundMaxN && (uint64_t)want_n < max_kmers) want_n *= 2;
  uint64_t key;
  memcpy(&key, &max_fpr, sizeof key);
  // One immutable table per (-f value, size): kernels of earlier calls may still read theirs, so a table is never rewritten —
  // another -f value, or a batch with longer queries, gets a table of its own (uploaded from its pinned copy on the caller's
  // stream: nothing here waits for the GPU, kmcpg_submit stays non-blocking).  Tables live until kmcpg_close.
  for (const auto& t : db->fpr_bounds)
    if (t.key == key && t.n >= want_n) {
      *out = t.d;
      *out_n = t.n;
      return 0;
    }
  if (db->fpr_bounds.size() >= 64) {  // a host that sweeps -f: start over once nothing can be reading the old tables
    HIPCHK(hipDeviceSynchronize());
    release_fpr_bounds(db);
  }
  FprBoundTable t{};
  t.key = key;
  t.n = want_n;
  const size_t bytes = ((size_t)want_n + 1) * sizeof(uint16_t);
  HIPCHK(hipHostMalloc((void**)&t.h, bytes, hipHostMallocDefault));
  if (hipMalloc((void**)&t.d, bytes) != hipSuccess) {
    (void)hipHostFree(t.h);
    return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
  }
  QueryFpr* F = db->fpr.get();
  t.h[0] = 0;
  for (int n = 1; n <= want_n; n++) {
    const FprRow held = F->ensure_row(n);
    const std::vector<double>& row = *held;
    int c = 0;
    while (c <= n && !(QueryFpr::value(row, n, c) <= max_fpr)) c++;
    t.h[n] = (uint16_t)c;  // n + 1: no count passes
  }
  db->fpr_bounds.push_back(t);
  HIPCHK(hipMemcpyAsync(t.d, t.h, bytes, hipMemcpyHostToDevice, st));
  *out = t.d;
  *out_n = t.n;
  return 0;
}

}  // namespace

// the k-mer stage alone on a batch of reads, text or packed (b.d_seqs = the text, or where its expansion goes), single or paired (d_koff is
// for single reads: a pair's hashes start at offs[i] + offs2[i]); d_nk1 (optional): the first mate's raw count
// d_qlen (optional): every query's length as the kernels wrote it; prologue (optional): run under the handle's lock, in front of the first kernel
static int kmers_device(kmcpg_db* db, const DeviceBatch& b, const kmcpg_params* params, uint64_t* d_hashes, uint64_t hashes_cap, uint64_t* d_koff, int32_t* d_nk,
                        int32_t* d_nk1, void* stream, int32_t* d_qlen = nullptr, const std::function<int()>* prologue = nullptr) {
  if (!db || !b.d_seqs || !b.d_offs || !d_hashes || !d_nk) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if ((b.d_seqs2 == nullptr) != (b.d_offs2 == nullptr)) return kmcpg_fail(KMCPG_EINVAL, "seqs2 and offs2 must be given together");
  if (hashes_cap < b.total_bases) return kmcpg_fail(KMCPG_EINVAL, "hashes_cap must be >= total_bases");
  KMCPG_NO_FILES_ONLY(db);
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  const kmcpg_params p = params ? *params : default_params();
  hipStream_t st = (hipStream_t)stream;
  if (prologue)
    if (int rcp = (*prologue)()) return rcp;
  kmcpg_db::Workspace& W = db->ws[0];
  if (int rc0 = ws_begin(W, st)) return rc0;
  WsGuard wsg{W, st, st};
  if (W.w_scratch.ensure(2 * b.total_bases + 2) || W.w_nk_raw.ensure(b.n_reads + 1) || W.w_nk1.ensure(b.n_reads + 1)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
  DevBuf<int32_t> ql;
  if (!d_qlen && ql.ensure(b.n_reads + 1)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
  uint64_t maxn = 0;
  int rc = run_kmers(db, W, b, p, KmerOut{d_hashes, W.w_scratch.p, b.total_bases + 1, W.w_nk_raw.p, W.w_nk1.p, d_nk, d_qlen ? d_qlen : ql.p}, st, &maxn);
  if (rc == 0 && d_koff) HIPCHK(hipMemcpyAsync(d_koff, b.d_offs, (size_t)b.n_reads * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  if (rc == 0 && d_nk1 && b.n_reads) HIPCHK(hipMemcpyAsync(d_nk1, W.w_nk1.p, (size_t)b.n_reads * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  hipError_t e = hipStreamSynchronize(st);
  ql.release();
  if (rc) return rc;
  if (e != hipSuccess) return kmcpg_fail(KMCPG_EDEVICE, "k-mer kernel failed: %s", hipGetErrorString(e));
  // the witness of a list form: what the first kernel left to the one behind it (the stream is idle, the lock held; profiling only)
  if (db->k1_left && !db->k1_log.empty()) HIPCHK(hipMemcpy(&db->k1_log[0].left_on_list, db->k1_left, sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int kmcpg_kmers_device(kmcpg_db* db, const uint8_t* d_seqs, const uint64_t* d_offs, uint32_t n_reads, uint64_t total_bases,
                                  uint32_t max_read_len, const kmcpg_params* params, uint64_t* d_hashes, uint64_t hashes_cap, uint64_t* d_koff,
                                  int32_t* d_nk, void* stream) {
  return kmers_device(db, DeviceBatch{d_seqs, d_offs, nullptr, nullptr, n_reads, total_bases, max_read_len}, params, d_hashes, hashes_cap, d_koff, d_nk, nullptr,
                      stream);
}

extern "C" int kmcpg_kmers_device_paired(kmcpg_db* db, const uint8_t* d_seqs, const uint64_t* d_offs, const uint8_t* d_seqs2, const uint64_t* d_offs2,
                                         uint32_t n_reads, uint64_t total_bases, uint32_t max_read_len, const kmcpg_params* params, uint64_t* d_hashes,
                                         uint64_t hashes_cap, int32_t* d_nk, int32_t* d_nk1, void* stream) {
  if (!d_seqs2 || !d_offs2) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  return kmers_device(db, DeviceBatch{d_seqs, d_offs, d_seqs2, d_offs2, n_reads, total_bases, max_read_len}, params, d_hashes, hashes_cap, nullptr, d_nk, d_nk1,
                      stream);
}

extern "C" int kmcpg_kmers_device_packed(kmcpg_db* db, const uint8_t* d_codes, const kmcpg_exc_run* d_exc, uint32_t n_exc, uint8_t* d_text,
                                         const uint64_t* d_offs, uint32_t n_reads, uint64_t total_bases, uint32_t max_read_len,
                                         const kmcpg_params* params, uint64_t* d_hashes, uint64_t hashes_cap, uint64_t* d_koff, int32_t* d_nk,
                                         void* stream) {
  static_assert(sizeof(kmcpg_exc_run) == sizeof(ExcRun), "one layout");
  if (!d_codes || !d_text || (n_exc && !d_exc)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (((uintptr_t)d_codes & 3) || ((uintptr_t)d_text & 3)) return kmcpg_fail(KMCPG_EINVAL, "d_codes and d_text must be 4-byte aligned");
  DeviceBatch b{d_text, d_offs, nullptr, nullptr, n_reads, total_bases, max_read_len};
  b.packed.codes = d_codes;
  b.packed.exc = reinterpret_cast<const ExcRun*>(d_exc);
  b.packed.n_exc = n_exc;
  b.packed.text = d_text;
  b.packed.n_bases = total_bases;
  return kmers_device(db, b, params, d_hashes, hashes_cap, d_koff, d_nk, nullptr, stream);
}

int kmcpg::describe_windows(const WindowPiece& w, hipStream_t st) {
  launch_window_desc(w.d_soffs, w.d_wpre, w.d_vpre, w.ns, w.n_win, w.step, w.window, w.d_src, w.d_offs, st);
  HIPCHK(hipGetLastError());
  return 0;
}

// the k-mer stage alone on a staged piece of sliding windows: what a lane does for such a batch (lane.cpp: describe_windows in the prologue,
// WindowPiece::batch as the batch), then kmers_device
extern "C" int kmcpg_kmers_device_windows(kmcpg_db* db, const uint8_t* d_text, const uint64_t* d_soffs, const uint64_t* d_wpre, const uint64_t* d_vpre,
                                          const uint64_t* d_cpre, uint32_t n_slices, uint64_t staged_bases, uint64_t n_chunks, uint32_t n_windows,
                                          uint64_t window_bases, uint32_t max_window_len, const kmcpg_window_spec* spec, const kmcpg_params* params,
                                          uint64_t* d_hashes, uint64_t hashes_cap, uint64_t* d_koff, uint64_t* d_src, int32_t* d_nk, int32_t* d_qlen,
                                          void* stream) {
  if (!d_text || !d_soffs || !d_wpre || !d_vpre || !d_cpre || !d_koff || !d_src || !d_qlen) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (int rc = window_spec_args(spec)) return rc;
  if (n_windows && !n_slices) return kmcpg_fail(KMCPG_EINVAL, "windows without a staged slice");
  // every window lies inside one slice, so the windows hold at most n_windows times the longest one; all k-mer positions lie in the staged text
  if ((uint64_t)max_window_len > spec->window || window_bases > (uint64_t)n_windows * max_window_len || n_chunks > staged_bases)
    return kmcpg_fail(KMCPG_EINVAL, "the piece's sizes contradict each other");
  WindowPiece w;
  w.d_text = d_text;
  w.d_soffs = d_soffs;
  w.d_wpre = d_wpre;
  w.d_vpre = d_vpre;
  w.d_cpre = d_cpre;
  w.ns = n_slices;
  w.sb = staged_bases;
  w.n_chunks = n_chunks;
  w.n_win = n_windows;
  w.wmax = max_window_len;
  w.bases = window_bases;
  w.step = spec->step;
  w.window = spec->window;
  w.d_src = d_src;
  w.d_offs = d_koff;
  hipStream_t st = (hipStream_t)stream;
  const std::function<int()> desc = [&]() -> int { return describe_windows(w, st); };
  return kmers_device(db, w.batch(), params, d_hashes, hashes_cap, nullptr, d_nk, nullptr, stream, d_qlen, &desc);
}

extern "C" int kmcpg_k1_codes_batches(kmcpg_db* db, uint64_t* direct, uint64_t* expanded) {
  if (!db) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  if (direct) *direct = db->k1_codes_direct;
  if (expanded) *expanded = db->k1_codes_expanded;
  return 0;
}

extern "C" int kmcpg_query_device(kmcpg_db* db, const uint8_t* d_seqs, const uint64_t* d_offs, const uint8_t* d_seqs2, const uint64_t* d_offs2,
                                  uint32_t n_reads, uint64_t total_bases, uint32_t max_read_len, const kmcpg_params* params, kmcpg_hit* d_hits,
                                  uint64_t hit_cap, uint64_t* d_counters, int32_t* d_qkmers, int32_t* d_qlen, void* stream) {
  return kmcpg::query_device_after(db, DeviceBatch{d_seqs, d_offs, d_seqs2, d_offs2, n_reads, total_bases, max_read_len}, params,
                                   QueryOut{d_hits, hit_cap, d_counters, d_qkmers, d_qlen}, stream, nullptr, nullptr);
}

// kmcpg_query_device with a prologue that runs once the handle's enqueue lock is held, i.e. right in front of this batch's first kernel.
// lane.cpp enqueue puts "wait for this batch's upload" (+ the expansion of packed input) there: enqueued BEFORE taking the lock, that wait could
// land in the kernel stream between the k-mer kernels and the COBS kernel of the batch before — a call that reads a word back in the middle
// (whole-genome queries) releases nothing until it returns — and the earlier batch's COBS kernel then sat behind the later batch's 4.5-ms
// upload (profiles/r06_h2h.txt: 2.4 ms of idle GPU per batch of 256 assemblies).
int kmcpg::query_device_after(kmcpg_db* db, const DeviceBatch& b, const kmcpg_params* params, const QueryOut& out, void* stream,
                              const std::function<int()>* prologue, int32_t* bound_n) {
  if (!db || !b.d_seqs || !b.d_offs || !out.d_counters || !out.d_qkmers || !out.d_qlen || (!out.d_hits && out.hit_cap)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if ((b.d_seqs2 == nullptr) != (b.d_offs2 == nullptr)) return kmcpg_fail(KMCPG_EINVAL, "seqs2 and offs2 must be given together");
  KMCPG_NO_FILES_ONLY(db);
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  if (prologue)
    if (int rcp = (*prologue)()) return rcp;
  const kmcpg_params p = params ? *params : default_params();
  if (int rcs = set_refuse_params(db, p)) return rcs;
  if (p.min_matched < 1) return kmcpg_fail(KMCPG_EINVAL, "min_matched must be >= 1");  // getFlagPositiveInt (search.go:165)
  if (p.k > 0 && std::find(db->ks_desc.begin(), db->ks_desc.end(), p.k) == db->ks_desc.end())
    return kmcpg_fail(KMCPG_EINVAL, "k=%d is not a k-mer size of this database", p.k);
  const int k_used = p.k > 0 ? p.k : db->info.k;
  hipStream_t st = (hipStream_t)stream;
  // test hook: behave as if the k-mer workspace of a batch above this many bases could not be allocated (the batch-halving path
  // of kmcpg_search_batch, tests/test_gpu_paged.py)
  // (honoured only together with KMCPG_TEST_HOOKS=1: a stray variable in a production environment must not fake an ENOMEM)
  static const bool test_hooks = getenv("KMCPG_TEST_HOOKS") && atoi(getenv("KMCPG_TEST_HOOKS")) == 1;
  if (test_hooks)
    if (const char* e = getenv("KMCPG_TEST_MAX_BASES"))
      if (b.total_bases > (uint64_t)atoll(e)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed (KMCPG_TEST_MAX_BASES)");
  const int slot = pick_slot(db, b.total_bases, whole_genome_batch(db, b.max_read_len, b.d_seqs2 != nullptr));
  db->ws_calls++;
  db->ws_last = slot;
  db->k2_log.clear();
  K2Log* const k2_log = db->profiling >= 1 ? &db->k2_log : nullptr;  // the launchers write it (k2_cobs.hip), kmcpg_last_k2_launches reads it
  kmcpg_db::Workspace& W = db->ws[slot];
  // experiment (KMCPG_K1_STREAM=1): the k-mer kernels on a high-priority stream of the handle's own, so that their workgroups are
  // dispatched AHEAD of the previous batch's COBS workgroups whenever a slot frees up (on equal terms the dispatcher keeps feeding the
  // kernel that came first and the k-mer kernels only get the COBS kernel's tail: tools/ab/r05_call3.sh)
  static const bool k1_own = getenv("KMCPG_K1_STREAM") && atoi(getenv("KMCPG_K1_STREAM")) == 1;
  hipStream_t kst = st;
  if (k1_own) {
    if (!db->k1_stream) {
      int lo = 0, hi = 0;
      if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0;
      HIPCHK(hipStreamCreateWithPriority(&db->k1_stream, hipStreamNonBlocking, hi));
    }
    if (!W.in_ev) HIPCHK(hipEventCreateWithFlags(&W.in_ev, hipEventDisableTiming));
    if (!W.k1_ev) HIPCHK(hipEventCreateWithFlags(&W.k1_ev, hipEventDisableTiming));
    kst = db->k1_stream;
    HIPCHK(hipEventRecord(W.in_ev, st));  // the batch's inputs are ordered on the caller's stream
    HIPCHK(hipStreamWaitEvent(kst, W.in_ev, 0));
  }
  if (int rc0 = ws_begin(W, kst)) return rc0;
  WsGuard wsg{W, st, kst};
  if (W.w_hashes.ensure(b.total_bases + 1) || W.w_nk_raw.ensure(b.n_reads + 1) || W.w_nk1.ensure(b.n_reads + 1)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
  uint64_t ub = b.max_read_len >= (uint32_t)k_used ? (uint64_t)(b.max_read_len - k_used + 1) : 0;
  if (b.d_seqs2) ub *= 2;
  const bool window_sketch = db->info.syncmer || db->info.minimizer;
  if ((ub > (uint64_t)p.dedup_threshold || window_sketch) && W.w_scratch.ensure(2 * b.total_bases + 2)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
  uint64_t maxn = 0;
  hipEvent_t* pev = db->ev + 4 * (db->ev_calls % 4);
  if (db->profiling) {
    for (auto& ev : db->ev)
      if (!ev) HIPCHK(hipEventCreate(&ev));
    HIPCHK(hipEventRecord(pev[0], kst));
  }
  int rc = run_kmers(db, W, b, p, KmerOut{W.w_hashes.p, W.w_scratch.p, b.total_bases + 1, W.w_nk_raw.p, W.w_nk1.p, out.d_qkmers, out.d_qlen}, kst, &maxn);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(out.d_counters, 0, 2 * sizeof(uint64_t), kst));
  launch_max_nk(out.d_qkmers, b.n_reads, (unsigned long long*)out.d_counters + 1, kst);
  if (db->profiling) HIPCHK(hipEventRecord(pev[3], kst));  // k-mers done
  if (k1_own) {
    HIPCHK(hipEventRecord(W.k1_ev, kst));
    HIPCHK(hipStreamWaitEvent(st, W.k1_ev, 0));
  }
  static const int debug_rowsort = getenv("KMCPG_DEBUG_ROWSORT") ? atoi(getenv("KMCPG_DEBUG_ROWSORT")) : 0;
  if (debug_rowsort && !b.d_offs2 && !db->h_groupdev.empty())  // experiment only: profiles/r05_rowsort_gate.txt
    launch_debug_rowsort(W.w_hashes.p, b.d_offs, out.d_qkmers, b.n_reads, db->h_groupdev[0].num_sigs, db->h_groupdev[0].magic_hi, debug_rowsort, st);
  // which COBS kernels, on which grids (k2_plan.hpp)
  K2Shape s;
  s.n_reads = b.n_reads;
  s.max_n = maxn;
  s.num_hashes = db->info.num_hashes;
  s.matrix_bytes_local = db->info.matrix_bytes_local;
  s.n_cols = db->info.n_cols;
  if (db->classes.size() > (size_t)K2_MAX_CLASSES) return kmcpg_fail(KMCPG_EINVAL, "more lane classes than lane forms");
  for (const auto& c : db->classes) s.classes[s.n_classes++] = K2Class{c.lpr, (uint32_t)c.slots.size(), c.d_bslots ? (uint32_t)c.bslots.size() : 0u};
  s.knobs = k2_knobs();
  // which queries are long is only known on the device: one small D2H read, where the plan has a use for the answer
  uint32_t long_meta[2] = {0, 0};  // how many above split_min, the largest of them
  const bool ask = k2_ask_long(s);
  if (ask) {
    if (W.w_long_list.ensure(b.n_reads + 1) || W.w_long_meta.ensure(2)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
    HIPCHK(hipMemsetAsync(W.w_long_meta.p, 0, 2 * sizeof(uint32_t), st));
    launch_list_long(out.d_qkmers, b.n_reads, s.knobs.split_min, W.w_long_list.p, W.w_long_meta.p, st);
    HIPCHK(hipMemcpyAsync(long_meta, W.w_long_meta.p, sizeof long_meta, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  const K2Plan plan = k2_plan(s, ask, long_meta[0], long_meta[1]);
  if (!plan.npl) return kmcpg_fail(KMCPG_EUNSUPPORTED, "queries with more than 16777214 k-mers need KMCPG_SPLIT_MIN > 0");
  K2Args a{};
  a.blocks = db->d_groupdev;
  a.segs = db->d_segs;
  a.n_reads = b.n_reads;
  a.hashes = W.w_hashes.p;
  a.offs = b.d_offs;
  a.offs2 = b.d_offs2;
  a.nk = out.d_qkmers;
  a.min_qcov = p.min_qcov;
  a.min_matched = p.min_matched;
  a.num_hashes = db->info.num_hashes;
  a.nt_loads = s.knobs.nt_loads;
  a.prune = s.knobs.prune;
  a.group_rows = plan.group_rows;
  a.prune_every = plan.prune_every;
  a.split_min = plan.split_min;
  a.slot_major = s.knobs.slot_major;
  a.tail_sectors = s.knobs.tail_sectors;
  a.tail_min = s.knobs.tail_min;
  a.hits = out.d_hits;
  a.hit_cap = out.hit_cap;
  a.counter = (unsigned long long*)out.d_counters;
  if (db->profiling >= 2) {
    if (W.w_gathered.ensure((size_t)K2_GATHER_SLOTS * 16)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
    HIPCHK(hipMemsetAsync(W.w_gathered.p, 0, (size_t)K2_GATHER_SLOTS * 16 * sizeof(uint64_t), st));
    a.gathered = (unsigned long long*)W.w_gathered.p;
  }
  // the persistent launches of the plan (k2_cobs.hip k2_cobs_persist): one zeroed unit counter per grid piece
  uint64_t pieces = 0;
  for (int i = 0; i < plan.n_launches; i++)
    if (plan.launches[i].persist) pieces = std::max(pieces, k2_n_pieces(plan.launches[i]));
  if (pieces) {
    if (W.w_k2_queue.ensure((size_t)pieces * K2_QUEUE_PITCH)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
    HIPCHK(hipMemsetAsync(W.w_k2_queue.p, 0, (size_t)pieces * K2_QUEUE_PITCH * sizeof(uint64_t), st));
    a.unit_queue = (unsigned long long*)W.w_k2_queue.p;
    a.persist_wgs = s.knobs.persist_wgs;
  }
  if (int rcb = fpr_bound(db, p.max_fpr, plan.max_short, st, &a.cmin_fpr, &a.cmin_fpr_n)) return rcb;
  if (bound_n) *bound_n = a.cmin_fpr ? a.cmin_fpr_n : 0;  // both kernel forms apply the table to every query of up to this many k-mers
  // COBS kernels one batch at a time (the k-mer kernels above may have run beside the previous batch's)
  // (KMCPG_COBS_CHAIN=0, experiment with two kernel streams + two workspace slots: the next batch's COBS kernel may start in the previous
  // one's ragged end — nothing is shared between them but the read-only index; their HIP-event durations then overlap)
  static const bool cobs_chain = !(getenv("KMCPG_COBS_CHAIN") && atoi(getenv("KMCPG_COBS_CHAIN")) == 0);
  if (int rcc = chain_begin(&db->cobs_ev, cobs_chain && db->cobs_ev_valid, st)) return rcc;
  if (db->profiling) HIPCHK(hipEventRecord(pev[1], st));
  // a launch record's slots: its class's, or that class's block-unit list
  auto with_slots = [&](K2Args x, int cls, const K2Launch& l) {
    const SlotClass& c = db->classes[(size_t)cls];
    x.slots = l.block_units ? c.d_bslots : c.d_slots;
    x.nslots = l.block_units ? (uint32_t)c.bslots.size() : (uint32_t)c.slots.size();
    x.k2_flags = l.k2_flags;
    return x;
  };
  const char* const no_kernel = "batch too large for one launch: split it";
  for (int i = 0; i < plan.n_launches; i++) {
    const K2Launch& l = plan.launches[i];
    if (l.kind == K2Kind::Split) continue;
    const int rcl = l.kind == K2Kind::Pair ? launch_k2_pair(l, with_slots(a, l.cls, l), with_slots(a, l.cls_b, l), st, k2_log) : launch_k2(l, with_slots(a, l.cls, l), st, k2_log);
    if (rcl != 0) return kmcpg_fail(KMCPG_EINVAL, no_kernel);
  }
  if (plan.n_long) {  // the chunked form: count arrays of plan.group long queries at a time
    a.ncols_total = (uint32_t)db->info.n_cols;
    a.split_chk = plan.split_chk;
    a.split_chunks = plan.split_chunks;
    if (W.w_long_counts.ensure((size_t)std::min<uint32_t>(plan.group, plan.n_long) * a.ncols_total)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
    a.long_counts = W.w_long_counts.p;
    for (uint32_t g0 = 0; g0 < plan.n_long; g0 += plan.group) {
      a.long_list = W.w_long_list.p + g0;
      a.n_long = std::min<uint32_t>(plan.group, plan.n_long - g0);
      HIPCHK(hipMemsetAsync(a.long_counts, 0, (size_t)a.n_long * a.ncols_total * sizeof(uint32_t), st));
      for (int i = 0; i < plan.n_launches; i++) {
        const K2Launch& l = plan.launches[i];
        if (l.kind == K2Kind::Split && launch_k2(k2_split_launch(plan, s, l, a.n_long), with_slots(a, l.cls, l), st, k2_log) != 0)
          return kmcpg_fail(KMCPG_EINVAL, no_kernel);
      }
      launch_threshold_long(a, st);
    }
  }
  HIPCHK(hipEventRecord(db->cobs_ev, st));
  db->cobs_ev_valid = true;
  if (db->profiling) {
    HIPCHK(hipEventRecord(pev[2], st));
    db->ev_calls++;
  }
  if (int rc1 = wsg.finish()) return rc1;
  HIPCHK(hipGetLastError());
  return 0;
}

// K3: the device half of finalize (k3_finalize.hip) — group by read, -T, per-query order.  Enqueue only.
extern "C" int kmcpg_group_device(kmcpg_db* db, const kmcpg_hit* d_hits, const uint64_t* d_n_hits, uint64_t hit_cap, const int32_t* d_qkmers, uint32_t n_reads,
                                  const kmcpg_params* params, kmcpg_pair* d_pairs, uint64_t* d_read_offs, void* stream) {
  if (!db || !d_n_hits || !d_read_offs || (n_reads && !d_qkmers) || (hit_cap && (!d_hits || !d_pairs))) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (db->opts.device < 0 || !db->d_col_size) return kmcpg_fail(KMCPG_EDEVICE, "metadata-only handle (device -1): no GPU work possible");
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  const kmcpg_params p = params ? *params : default_params();
  if (int rcs = set_refuse_params(db, p)) return rcs;
  hipStream_t st = (hipStream_t)stream;
  FinGuard fing{db, st};  // (engine.hpp; as WsGuard)
  if (int rc0 = fing.wait()) return rc0;
  if (db->w_fin_cnt.ensure((size_t)n_reads + 2) || db->w_fin_sums.ensure((size_t)k3_scan_tiles_for(n_reads + 1) + 1)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
  // counters of the reads + the word that counts hits naming a read / column that does not exist
  HIPCHK(hipMemsetAsync(db->w_fin_cnt.p, 0, ((size_t)n_reads + 2) * sizeof(uint32_t), st));
  K3Args a{};
  a.hits = d_hits;
  a.n_hits = (const unsigned long long*)d_n_hits;
  a.hit_cap = hit_cap;
  a.nk = d_qkmers;
  a.n_reads = n_reads;
  a.n_cols = (uint32_t)db->col_meta.size();
  a.col_size = db->d_col_size;
  a.min_tcov = p.min_tcov;
  a.sort_mode = p.do_not_sort ? 3 : (p.sort_by == 1 ? 1 : (p.sort_by == 2 ? 2 : 0));
  a.cnt = db->w_fin_cnt.p;
  a.bad = db->w_fin_cnt.p + n_reads + 1;
  a.offs = d_read_offs;
  a.sums = db->w_fin_sums.p;
  a.pairs = d_pairs;
  if (n_reads == 0) HIPCHK(hipMemsetAsync(d_read_offs, 0, 2 * sizeof(uint64_t), st));
  else {
    K3SetArgs sa{};
    if (db->is_set()) {  // a database set: the merge order (k3_set_order.hpp); the counters speak of this launch (kmcpg_last_set_order)
      sa.n_members = (uint32_t)db->set_col_base.size();
      for (uint32_t i = 0; i < sa.n_members; i++) sa.base[i] = db->set_col_base[i];
      sa.stats = db->d_set_stats;
      HIPCHK(hipMemsetAsync(db->d_set_stats, 0, K3_SET_STATS * sizeof(uint32_t), st));
      db->set_host_segments.store(0);
      db->set_host_mixed.store(0);
    }
    launch_k3(a, 0, st, db->is_set() ? &sa : nullptr);
    // d_read_offs[n_reads + 1] = the bad-hit count (a 32-bit word widened on the device side of the copy: two words cleared first)
    HIPCHK(hipMemsetAsync(d_read_offs + n_reads + 1, 0, sizeof(uint64_t), st));
    HIPCHK(hipMemcpyAsync(d_read_offs + n_reads + 1, a.bad, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int kmcpg_set_profiling(kmcpg_db* db, int enable) {
  if (!db) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  db->profiling = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
  db->ev_calls = 0;
  return 0;
}

// word 0 of every counter slot: 16-byte row loads; word 1: 8-byte hash loads; word 2: waves that finished in tail mode
static int read_gather_slots(kmcpg_db* db, int word, uint64_t unit, uint64_t* bytes) {
  if (!db || !bytes) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  kmcpg_db::Workspace& W = db->ws[db->ws_last];
  if (db->profiling < 2 || !W.w_gathered.p || db->ev_calls == 0) return kmcpg_fail(KMCPG_EINVAL, "no kmcpg_query_device call at profiling level 2 yet");
  KMCPG_USE_DEVICE(db);
  hipEvent_t* pev = db->ev + 4 * ((db->ev_calls - 1) % 4);
  HIPCHK(hipEventSynchronize(pev[2]));
  std::vector<uint64_t> slots((size_t)K2_GATHER_SLOTS * 16);
  HIPCHK(hipMemcpy(slots.data(), W.w_gathered.p, slots.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  uint64_t n = 0;
  for (int i = 0; i < K2_GATHER_SLOTS; i++) n += slots[(size_t)i * 16 + (size_t)word];
  *bytes = n * unit;
  return 0;
}

extern "C" int kmcpg_last_gathered_bytes(kmcpg_db* db, uint64_t* bytes) { return read_gather_slots(db, 0, 16, bytes); }
extern "C" int kmcpg_last_hash_bytes(kmcpg_db* db, uint64_t* bytes) { return read_gather_slots(db, 1, 8, bytes); }
extern "C" int kmcpg_last_tail_waves(kmcpg_db* db, uint64_t* waves) { return read_gather_slots(db, 2, 1, waves); }

extern "C" int kmcpg_last_k2_launches(kmcpg_db* db, kmcpg_k2_launch* out, uint32_t cap, uint32_t* n) {
  static_assert(sizeof(kmcpg_k2_launch) == 32, "eight 4-byte words");
  if (!db || !n || (cap && !out)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  if (db->profiling < 1) return kmcpg_fail(KMCPG_EINVAL, "no kmcpg_query_device call at profiling level >= 1 yet");
  // the records are written while the call enqueues its kernels: nothing to wait for
  const size_t m = std::min<size_t>(cap, db->k2_log.size());
  if (m) memcpy(out, db->k2_log.data(), m * sizeof(kmcpg_k2_launch));
  *n = (uint32_t)db->k2_log.size();
  return 0;
}

extern "C" int kmcpg_last_k1_launches(kmcpg_db* db, kmcpg_k1_launch* out, uint32_t cap, uint32_t* n) {
  static_assert(sizeof(kmcpg_k1_launch) == 32, "eight 4-byte words");
  if (!db || !n || (cap && !out)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  // the records are written while the call enqueues its kernels (left_on_list: after kmers_device has synchronised): nothing to wait for;
  // without profiling there are none
  const size_t have = db->profiling >= 1 ? db->k1_log.size() : 0;
  const size_t m = std::min<size_t>(cap, have);
  if (m) memcpy(out, db->k1_log.data(), m * sizeof(kmcpg_k1_launch));
  *n = (uint32_t)have;
  return 0;
}

extern "C" int kmcpg_last_dedup_launches(kmcpg_db* db, kmcpg_dedup_launch* out, uint32_t cap, uint32_t* n) {
  static_assert(sizeof(kmcpg_dedup_launch) == 32, "eight 4-byte words");
  if (!db || !n || (cap && !out)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  // written while the stage enqueues its kernels: nothing to wait for; without profiling there are none
  const size_t have = db->profiling >= 1 ? db->dedup_log.size() : 0;
  const size_t m = std::min<size_t>(cap, have);
  if (m) memcpy(out, db->dedup_log.data(), m * sizeof(kmcpg_dedup_launch));
  if (m && db->dedup_fb && out[0].kernel == KMCPG_DD_LAUNCH_DEDUP) {  // the fallback counts, as the device holds them now
    KMCPG_USE_DEVICE(db);
    uint32_t fb[3] = {0, 0, 0};
    HIPCHK(hipMemcpy(fb, db->dedup_fb, sizeof fb, hipMemcpyDeviceToHost));
    out[0].p0 = (int32_t)fb[0];
    out[0].p1 = (int32_t)fb[1];
    out[0].p2 = (int32_t)fb[2];
  }
  *n = (uint32_t)have;
  return 0;
}

// the dedup stage alone (debug/tests): run_dedup on lists the caller laid out, on the first workspace slot as kmcpg_kmers_device.  Enqueue
// only, but for the read-backs of the whole-genome path.
extern "C" int kmcpg_dedup_device(kmcpg_db* db, uint64_t* d_hashes, uint64_t* d_scratch, const uint64_t* d_offs, const uint64_t* d_offs2,
                                  const int32_t* d_nk_raw, int32_t* d_nk_search, uint32_t n_reads, uint64_t max_n, const kmcpg_dedup_spec* spec,
                                  void* stream) {
  if (!db || !d_hashes || !d_scratch || !d_offs || !d_nk_raw || !d_nk_search || !spec) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (spec->key_shift < 0 || spec->key_shift > 63) return kmcpg_fail(KMCPG_EINVAL, "key_shift must be in 0..63");
  if (max_n > 0x7fffffffull) return kmcpg_fail(KMCPG_EINVAL, "max_n must fit a 32-bit count");
  KMCPG_NO_FILES_ONLY(db);
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  hipStream_t st = (hipStream_t)stream;
  kmcpg_db::Workspace& W = db->ws[0];
  if (int rc0 = ws_begin(W, st)) return rc0;
  WsGuard wsg{W, st, st};
  if (int rc = run_dedup(db, W, DedupLists{d_hashes, d_scratch, d_offs, d_offs2, d_nk_raw, d_nk_search}, n_reads, max_n, *spec, st)) return rc;
  if (int rc1 = wsg.finish()) return rc1;
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int kmcpg_timing_at(kmcpg_db* db, uint32_t age, float* kmers_ms, float* cobs_ms) {
  if (!db) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  if (!db->profiling || age >= 4 || db->ev_calls <= age) return kmcpg_fail(KMCPG_EINVAL, "no profiled kmcpg_query_device call of that age (the last 4 are kept)");
  KMCPG_USE_DEVICE(db);
  hipEvent_t* pev = db->ev + 4 * ((db->ev_calls - 1 - age) % 4);
  HIPCHK(hipEventSynchronize(pev[2]));
  float a = 0, b = 0;
  HIPCHK(hipEventElapsedTime(&a, pev[0], pev[3]));
  HIPCHK(hipEventElapsedTime(&b, pev[1], pev[2]));
  if (kmers_ms) *kmers_ms = a;
  if (cobs_ms) *cobs_ms = b;
  return 0;
}

extern "C" int kmcpg_last_timing(kmcpg_db* db, float* kmers_ms, float* cobs_ms) { return kmcpg_timing_at(db, 0, kmers_ms, cobs_ms); }

extern "C" int kmcpg_plant_reads_device(kmcpg_db* db, const uint8_t* d_seqs, const uint64_t* d_offs, uint32_t n_reads, uint64_t total_bases,
                                        uint32_t max_read_len, const uint32_t* d_cols, void* stream) {
  if (!db || !d_seqs || !d_offs || !d_cols) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  hipStream_t st = (hipStream_t)stream;
  kmcpg_db::Workspace& W = db->ws[0];
  if (int rc0 = ws_begin(W, st)) return rc0;
  WsGuard wsg{W, st, st};
  if (W.w_hashes.ensure(total_bases + 1) || W.w_nk_raw.ensure(n_reads + 1) || W.w_nk1.ensure(n_reads + 1)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
  DevBuf<int32_t> tmp;
  if (tmp.ensure(2 * (size_t)n_reads + 2)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
  kmcpg_params p = default_params();
  p.min_qlen = 0;
  p.min_matched = 1;
  p.dedup_threshold = 0x7fffffff;  // plant every k-mer occurrence (idempotent)
  uint64_t maxn = 0;
  if ((db->info.syncmer || db->info.minimizer) && W.w_scratch.ensure(2 * total_bases + 2)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
  int rc = run_kmers(db, W, DeviceBatch{d_seqs, d_offs, nullptr, nullptr, n_reads, total_bases, max_read_len}, p,
                     KmerOut{W.w_hashes.p, W.w_scratch.p, total_bases + 1, W.w_nk_raw.p, W.w_nk1.p, tmp.p, tmp.p + n_reads + 1}, st, &maxn);
  if (rc == 0)
    launch_plant_reads(db->d_blockdev, (uint32_t)db->h_blockdev.size(), db->info.num_hashes, W.w_hashes.p, d_offs, W.w_nk_raw.p, d_cols, n_reads, st);
  hipError_t e = hipStreamSynchronize(st);
  tmp.release();
  if (rc) return rc;
  if (e != hipSuccess) return kmcpg_fail(KMCPG_EDEVICE, "plant kernel failed: %s", hipGetErrorString(e));
  return 0;
}

