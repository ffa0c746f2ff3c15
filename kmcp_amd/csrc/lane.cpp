// lane.cpp — a batch in flight (lane.hpp): the handle's streams and lanes, the staging of a batch as text or as 2-bit codes, the enqueueing
// of upload + K1 + K2 (+ K3, K4) + the copies back, the wait for a lane's result with the rerun of a batch whose hit buffer overflowed,
// and the return of a ticket's lanes.  What is above a lane (tickets over several GPUs, retries, pieces, windows) is in host*.cpp.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <thread>

#include "kernels.hpp"
#include "lane.hpp"
#include "lane_plan.hpp"
#include "pack2.hpp"

namespace kmcpg {

// batches between kmcpg_submit and the end of kmcpg_wait on this handle (or its shards)
int async_in_flight(kmcpg_db* db) {
  int n = 0;
  for (kmcpg_db* sh : db->shards) n += async_in_flight(sh);
  if (!db->async) return n;
  std::lock_guard<std::mutex> g(db->async->mu);
  for (auto& l : db->async->lanes) n += l->busy ? 1 : 0;
  return n;
}

void drain(AsyncState* A) {
  if (A->up_stream) (void)hipStreamSynchronize(A->up_stream);
  if (A->stream) (void)hipStreamSynchronize(A->stream);
  if (A->stream2) (void)hipStreamSynchronize(A->stream2);
  if (A->copy_stream) (void)hipStreamSynchronize(A->copy_stream);
}

void async_release(kmcpg_db* db) {
  if (!db->async) return;
  if (db->opts.device >= 0) (void)hipSetDevice(db->opts.device);
  drain(db->async);
  for (auto& l : db->async->lanes) l->release();
  db->async->retry.release();
  if (db->async->stream) (void)hipStreamDestroy(db->async->stream);
  if (db->async->stream2) (void)hipStreamDestroy(db->async->stream2);
  if (db->async->copy_stream) (void)hipStreamDestroy(db->async->copy_stream);
  if (db->async->up_stream) (void)hipStreamDestroy(db->async->up_stream);
  delete db->async;
  db->async = nullptr;
}

int async_state(kmcpg_db* db, AsyncState** out) {
  static std::mutex init_mu;
  std::lock_guard<std::mutex> g(init_mu);
  if (!db->async) {
    std::unique_ptr<AsyncState> a(new AsyncState());
    HIPCHK(hipSetDevice(db->opts.device));
    HIPCHK(hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking));
    // the copies back run at the highest stream priority: where a copy is done by a blit kernel it must not queue behind the
    // chip-filling kernels of the next batch (same-box A/B: the eager copy at default priority cost the pipelined path 10 %)
    int prio_lo = 0, prio_hi = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) prio_lo = prio_hi = 0;
    HIPCHK(hipStreamCreateWithPriority(&a->copy_stream, hipStreamNonBlocking, prio_hi));
    HIPCHK(hipStreamCreateWithFlags(&a->up_stream, hipStreamNonBlocking));
    if (getenv("KMCPG_KSTREAMS")) a->kstreams = atoi(getenv("KMCPG_KSTREAMS")) >= 2 ? 2 : 1;  // 2: every batch, 1: never; unset: batches of whole genomes
    if (a->kstreams == 2) HIPCHK(hipStreamCreateWithFlags(&a->stream2, hipStreamNonBlocking));
    if (const char* e = getenv("KMCPG_INFLIGHT")) a->max_lanes = (size_t)std::max(1, std::min(atoi(e), 16));
    if (const char* e = getenv("KMCPG_DEVICE_FINALIZE")) a->device_finalize = atoi(e) != 0;
    // Hit buffers follow the data (a database full of close relatives returns hundreds of hits per read) but must never crowd
    // out the k-mer workspace next to a large index: all lanes together may take a quarter of what is free now (the index is
    // resident already), at most 16 GB.
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    uint64_t budget = std::min<uint64_t>(free_b / 4, 16ull << 30);
    if (const char* e = getenv("KMCPG_HIT_BUDGET_MB")) budget = (uint64_t)std::max(0ll, atoll(e)) << 20;
    a->lane_hit_budget = budget / (sizeof(kmcpg_hit) + sizeof(kmcpg_pair)) / (a->max_lanes + 1);  // a hit entry has its K3 pair beside it (d_pairs)
    db->async = a.release();
  }
  *out = db->async;
  return 0;
}

Lane* acquire_lane(AsyncState* A, bool retry, bool block) {
  if (retry) {
    A->retry_mu.lock();
    return &A->retry;
  }
  std::unique_lock<std::mutex> g(A->mu);
  for (;;) {
    for (auto& l : A->lanes)
      if (!l->busy) {
        l->busy = true;
        return l.get();
      }
    if (A->lanes.size() < A->max_lanes) {
      A->lanes.emplace_back(new Lane());
      A->lanes.back()->busy = true;
      return A->lanes.back().get();
    }
    if (!block) return nullptr;
    A->cv.wait(g);
  }
}

void release_lane(AsyncState* A, Lane* l, bool retry) {
  if (retry) {
    A->retry_mu.unlock();
    return;
  }
  {
    std::lock_guard<std::mutex> g(A->mu);
    l->busy = false;
  }
  A->cv.notify_one();
}

int fail_all_lanes_busy(const AsyncState* A) {
  return kmcpg_fail(KMCPG_EBUSY, "all %zu lanes of this handle are in flight: kmcpg_wait for a ticket first (KMCPG_INFLIGHT)", A->max_lanes);
}

int check_offsets(const HostBatch& b, uint64_t* maxlen) {
  *maxlen = 0;
  if (b.n == 0) return 0;
  if (b.offs[0] != 0 || (b.seqs2 && b.offs2[0] != 0)) return kmcpg_fail(KMCPG_EINVAL, "offs[0] must be 0");
  for (uint32_t i = 0; i < b.n; i++) {
    if (b.offs[i + 1] < b.offs[i] || (b.seqs2 && b.offs2[i + 1] < b.offs2[i])) return kmcpg_fail(KMCPG_EINVAL, "offsets must not decrease (read %u)", i);
    *maxlen = std::max(*maxlen, b.offs[i + 1] - b.offs[i]);
    if (b.seqs2) *maxlen = std::max(*maxlen, b.offs2[i + 1] - b.offs2[i]);
  }
  return 0;
}

int check_exc_runs(const kmcpg_exc_run* exc, uint64_t n_exc, uint64_t n_bases) {
  for (uint64_t i = 0; i < n_exc; i++) {
    const kmcpg_exc_run& e = exc[i];
    if (e.pos > n_bases || e.len > n_bases - e.pos || e.byte > 255) return kmcpg_fail(KMCPG_EINVAL, "exception run %llu lies outside the batch", (unsigned long long)i);
  }
  return 0;
}

namespace {

void par_memcpy(void* dst, const void* src, size_t n) {
  const size_t kMin = 8u << 20;
  if (n < 2 * kMin) {
    memcpy(dst, src, n);
    return;
  }
  const size_t T = std::min<size_t>(4, n / kMin);
  std::vector<std::thread> th;
  for (size_t t = 1; t < T; t++) th.emplace_back([=] { memcpy((char*)dst + n * t / T, (const char*)src + n * t / T, n * (t + 1) / T - n * t / T); });
  memcpy(dst, src, n / T);
  for (auto& t : th) t.join();
}

// Long-query batches go up as 2-bit codes (pack2.hpp): a batch of 256 genomes is 1 GB of ASCII, and at ~35 k genomes/s of kernel
// rate the 40-50 GB/s of PCIe were what bounded the host-to-host rate (9.9 k genomes/s, round 4).  The pack IS the staging copy —
// it reads the caller's buffer once and writes a quarter of it to pinned memory — and the device expands it again in ~0.3 ms per
// GB (k_unpack2); the k-mer kernels read ASCII as before.  Only where nothing re-reads the staged ASCII (retries of --try-se and
// of multi-k databases do: `allow_pack` is false there) and only for batches whose bases dominate the upload (mean query >= 1 kb:
// a batch of 150-bp reads is 150 MB and its staging copy is not what limits it).  KMCPG_PACK=0 switches it off.
bool pack_wanted(uint64_t total_bases, uint32_t n) {
  static const int env = getenv("KMCPG_PACK") ? atoi(getenv("KMCPG_PACK")) : -1;  // 0 never, 1 always (tests), default by shape
  if (env == 0) return false;
  if (env == 1) return total_bases >= 64;
  return total_bases >= (8ull << 20) && total_bases / std::max<uint32_t>(1, n) >= 1000;
}

// a lane takes a new batch: nothing of its previous one is left (a lane that served kmcpg_submit_packed from the caller's pinned codes, or
// windows, last time does not now), the offsets are checked, and what is searched are the reads as they go up
int lane_begin(Lane* L, const HostBatch& b) {
  L->up_reads = L->n = b.n;
  L->up_bases = L->tb1 = L->tb2 = 0;
  L->packed = L->win = L->summary = L->stats = L->bins = false;
  L->n_exc = 0;
  L->ext_pack = nullptr;
  L->paired = b.seqs2 != nullptr;
  L->maxlen = 0;
  L->copied = 0;
  uint64_t maxlen = 0;
  if (int rc = check_offsets(b, &maxlen)) return rc;
  if (maxlen > 0x7fffffffULL) return kmcpg_fail(KMCPG_EUNSUPPORTED, "query longer than 2^31-1 bases");
  if (b.n == 0) return 0;
  L->maxlen = (uint32_t)maxlen;
  L->up_bases = L->tb1 = b.offs[b.n];
  L->tb2 = b.seqs2 ? b.offs2[b.n] : 0;
  return 0;
}

}  // namespace

int stage(Lane* L, const HostBatch& b, bool allow_pack) {
  if (int rc = lane_begin(L, b)) return rc;
  const uint32_t n = b.n;
  if (n == 0) return 0;
  if (L->h_offs.ensure((size_t)n + 1) || (b.seqs2 && (L->h_seqs2.ensure(L->tb2 + 16) || L->h_offs2.ensure((size_t)n + 1))))
    return kmcpg_fail(KMCPG_ENOMEM, "hipHostMalloc failed");
  if (allow_pack && !b.seqs2 && pack_wanted(L->tb1, n)) {
    static thread_local std::vector<PackRun> exc;
    static_assert(sizeof(PackRun) == sizeof(ExcRun), "one layout");
    if (L->h_pack.ensure(L->tb1 / 4 + 16)) return kmcpg_fail(KMCPG_ENOMEM, "hipHostMalloc failed");
    static const unsigned pack_threads = getenv("KMCPG_PACK_THREADS") ? (unsigned)std::max(1, std::min(atoi(getenv("KMCPG_PACK_THREADS")), 64))
                                                                      : std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    // more than one foreign run per 256 bases: not nucleotide text, sent as it is
    if (pack2_parallel(b.seqs, L->tb1, L->h_pack.p, exc, std::max<size_t>(1024, L->tb1 / 256), pack_threads)) {
      if (L->h_exc.ensure(exc.size() + 1)) return kmcpg_fail(KMCPG_ENOMEM, "hipHostMalloc failed");
      if (!exc.empty()) memcpy(L->h_exc.p, exc.data(), exc.size() * sizeof(ExcRun));
      L->n_exc = (uint32_t)exc.size();
      L->packed = true;
    }
  }
  if (!L->packed) {
    if (L->h_seqs.ensure(L->tb1 + 16)) return kmcpg_fail(KMCPG_ENOMEM, "hipHostMalloc failed");
    par_memcpy(L->h_seqs.p, b.seqs, L->tb1);
  }
  par_memcpy(L->h_offs.p, b.offs, ((size_t)n + 1) * sizeof(uint64_t));
  if (b.seqs2) {
    par_memcpy(L->h_seqs2.p, b.seqs2, L->tb2);
    par_memcpy(L->h_offs2.p, b.offs2, ((size_t)n + 1) * sizeof(uint64_t));
  }
  return 0;
}

int stage_packed(Lane* L, const PackedIn& in, const HostBatch& b) {
  static_assert(sizeof(kmcpg_exc_run) == sizeof(ExcRun), "one layout");
  if (int rc = lane_begin(L, b)) return rc;
  const uint32_t n = b.n;
  if (n == 0) return 0;
  const uint64_t tb = L->tb1;
  if (in.n_exc > 0xffffffffULL) return kmcpg_fail(KMCPG_EINVAL, "too many exception runs");
  if (int rc = check_exc_runs(in.exc, in.n_exc, tb)) return rc;
  // Codes in memory from kmcpg_host_alloc are page-locked already: the DMA engine reads them where they are (the caller keeps them untouched
  // until kmcpg_wait has returned).  Staging 256 MB — a batch of 256 assemblies — took the submitting thread 15-25 ms, longer than the GPU
  // needs for the batch (profiles/r06_h2h.txt); anything else is copied to the lane's pinned buffer as before.
  bool pinned = false;
  {
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, in.codes) == hipSuccess) pinned = at.type == hipMemoryTypeHost;
    else (void)hipGetLastError();  // ordinary memory: not an error
  }
  if (L->h_offs.ensure((size_t)n + 1) || (!pinned && L->h_pack.ensure(tb / 4 + 16)) || L->h_exc.ensure(in.n_exc + 1)) return kmcpg_fail(KMCPG_ENOMEM, "hipHostMalloc failed");
  if (pinned) L->ext_pack = in.codes;
  else par_memcpy(L->h_pack.p, in.codes, (tb + 3) / 4);
  if (in.n_exc) memcpy(L->h_exc.p, in.exc, in.n_exc * sizeof(ExcRun));
  par_memcpy(L->h_offs.p, b.offs, ((size_t)n + 1) * sizeof(uint64_t));
  L->n_exc = (uint32_t)in.n_exc;
  L->packed = true;
  return 0;
}

namespace {

// the staged piece of windows a lane holds (L->win)
WindowPiece lane_windows(const Lane* L) {
  const size_t ns1 = (size_t)L->up_reads + 1;  // d_wmeta: wpre, vpre, cpre one behind the other
  WindowPiece w;
  w.d_text = L->d_seqs.p;
  w.d_soffs = L->d_soffs.p;
  w.d_wpre = L->d_wmeta.p;
  w.d_vpre = L->d_wmeta.p + ns1;
  w.d_cpre = L->d_wmeta.p + 2 * ns1;
  w.ns = (uint32_t)L->up_reads;
  w.sb = L->up_bases;
  w.n_chunks = L->wchunks;
  w.n_win = L->n;
  w.wmax = L->maxlen;
  w.bases = L->tb1;
  w.step = L->wstep;
  w.window = L->wwin;
  w.d_src = L->d_wsrc.p;
  w.d_offs = L->d_offs.p;
  return w;
}

// the lane's batch as the GPU half is told about it.  Packed input: the k-mer stage (query.cpp run_kmers) reads the codes where it can — whole
// genomes — and expands them to the text in d_seqs where it cannot.  Sliding windows: the k-mer kernels read each window's bases in place
// (d_wsrc, built by the prologue of the first attempt)
DeviceBatch lane_batch(const Lane* L) {
  DeviceBatch b = L->win ? lane_windows(L).batch()
                         : DeviceBatch{L->d_seqs.p, L->d_offs.p, L->paired ? L->d_seqs2.p : nullptr, L->paired ? L->d_offs2.p : nullptr, L->n, L->tb1 + L->tb2, L->maxlen};
  if (L->packed) {
    b.packed.codes = L->d_pack.p;
    b.packed.exc = L->n_exc ? L->d_exc.p : nullptr;
    b.packed.n_exc = L->n_exc;
    b.packed.text = L->d_seqs.p;
    b.packed.n_bases = L->up_bases;
  }
  return b;
}

// K1 + K2 (+ K3) of a staged and uploaded lane; a rerun of the batch (ENOMEM, hit-buffer overflow) does all of it again
int enqueue_query(kmcpg_db* db, AsyncState* A, Lane* L, const kmcpg_params& p, const std::function<int()>* prologue = nullptr) {
  hipStream_t st = L->st;
  int rc = query_device_after(db, lane_batch(L), &p, QueryOut{L->d_hits.p, L->d_hits.cap, L->d_cnt.p, L->d_qk.p, L->d_ql.p}, st, prologue, &L->bound_n);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(L->h_cnt.p, L->d_cnt.p, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (L->grouped) {  // K3 right behind K2 (an overflowing hit buffer makes both run again, collect())
    if (L->d_pairs.ensure(L->d_hits.cap) || L->d_roffs.ensure((size_t)L->n + 2) || L->h_roffs.ensure((size_t)L->n + 2)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
    rc = kmcpg_group_device(db, L->d_hits.p, L->d_cnt.p, L->d_hits.cap, L->d_qk.p, L->n, &p, L->d_pairs.p, L->d_roffs.p, st);
    if (rc) return rc;
    L->spec = db->spec_on();
    L->counted = 0;  // (a lane keeps its fields from batch to batch: the summary path below returns before the counting stages' turn)
    // (a batch K5 summarises, and one searched for statistics only, needs K3's last two words only: the pairs it kept, and its count of bad hits)
    const bool stats_only = L->stats && counting_mask(db) != 0;
    if (L->bins) L->spec = false;  // (kmcpg_submit_bins refuses a handle with K4 on)
    const size_t skip = L->summarized() || stats_only || L->bins ? L->n : 0;
    HIPCHK(hipMemcpyAsync(L->h_roffs.p + skip, L->d_roffs.p + skip, ((size_t)L->n + 2 - skip) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    L->d_final = L->d_pairs.p;
    if (L->bins) {
      // K11 right behind K3, and nothing else: four bytes per read leave the GPU.  K11's LEFT byte goes through K10's compaction as a
      // stage's byte would; the LEFT reads' pairs go into d_hits — dead once K3 has grouped it — and come down on demand (collect).  Every
      // buffer first, as for the counting stages.  KMCPG_BIN_DEVICE=0: every read with matches goes to the host half
      if (L->d_bins.ensure(L->n) || L->h_bins.ensure(L->n) || L->d_bleft.ensure(L->n) || L->d_bstats.ensure(K11_STATS) || L->h_bstats.ensure(K11_STATS) || L->d_mask.ensure(L->n) ||
          L->d_loffs.ensure((size_t)L->n + 1) || L->d_lstats.ensure(K10_STATS) || L->h_lstats.ensure(K10_STATS))
        return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
      if (int rc2 = left_compact_reserve(db, L->n)) return rc2;
      const char* e = getenv("KMCPG_BIN_DEVICE");
      const int32_t final_n = e && atoi(e) == 0 ? -1 : std::min<int32_t>(L->bound_n, kFprBoundAlways);
      rc = bin_enqueue(db, L->d_pairs.p, L->d_roffs.p, L->d_hits.cap, L->d_qk.p, L->n, final_n, L->d_cnt.p, L->d_hits.cap, L->d_bins.p, L->d_bleft.p, L->d_bstats.p, st);
      if (rc) return rc;
      const uint8_t* left[N_COUNTING] = {L->d_bleft.p, nullptr, nullptr};
      kmcpg_pair* out = (kmcpg_pair*)L->d_hits.p;
      rc = left_compact_enqueue(db, L->d_pairs.p, L->d_roffs.p, L->d_hits.cap, L->n, left, L->d_cnt.p, L->d_hits.cap, L->d_mask.p, out, L->d_hits.cap, L->d_loffs.p, L->d_lstats.p, st);
      if (rc) return rc;
      HIPCHK(hipMemcpyAsync(L->h_bins.p, L->d_bins.p, (size_t)L->n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(L->h_bstats.p, L->d_bstats.p, K11_STATS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(L->h_lstats.p, L->d_lstats.p, K10_STATS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      L->d_final = out;
      return 0;
    }
    if (L->spec) {  // K4 right behind K3: only the surviving reads' matches leave the GPU
      if (L->d_soffs4.ensure((size_t)L->n + 1) || L->d_verd.ensure(L->n) || L->h_verd.ensure(L->n)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
      // a segment is final on the device only where the -f bound was applied there (finalize.cpp: final_n); longer queries keep their
      // pairs and the host judges what its own -f test leaves.  KMCPG_SPECIFIC_DEVICE=0: every read goes that way
      const char* e = getenv("KMCPG_SPECIFIC_DEVICE");
      const int32_t final_n = e && atoi(e) == 0 ? -1 : std::min<int32_t>(L->bound_n, kFprBoundAlways);
      kmcpg_pair* out = (kmcpg_pair*)L->d_hits.p;  // (12 bytes per hit: room for d_hits.cap pairs and more)
      rc = kmcpg_specific_device(db, L->d_pairs.p, L->d_roffs.p, L->d_hits.cap, L->d_qk.p, L->n, final_n, out, L->d_hits.cap, L->d_soffs4.p, L->d_verd.p, st);
      if (rc) return rc;
      L->d_final = out;
      if (L->summary) {
        // K5 right behind K4: 16 bytes per window leave the GPU; the pairs of the windows LEFT to the host go into d_pairs — dead once K4
        // has compacted it — and come down on demand (collect_summary).  No offsets, no verdict bytes: the LEFT records carry both
        if (L->d_sum.ensure(L->n) || L->h_sum.ensure(L->n) || L->d_loffs.ensure((size_t)L->n + 1)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
        rc = kmcpg_summarize_device(db, out, L->d_soffs4.p, L->d_hits.cap, L->d_verd.p, L->d_qk.p, L->n, L->d_sum.p, L->d_pairs.p, L->d_hits.cap, L->d_loffs.p, st);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(L->h_sum.p, L->d_sum.p, (size_t)L->n * sizeof(kmcpg_window_summary), hipMemcpyDeviceToHost, st));
        L->d_final = L->d_pairs.p;
        return 0;
      }
      // the new offsets over the old ones (in stream order); the word behind them — K3's count of bad hits — stays
      HIPCHK(hipMemcpyAsync(L->h_roffs.p, L->d_soffs4.p, ((size_t)L->n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(L->h_verd.p, L->d_verd.p, (size_t)L->n, hipMemcpyDeviceToHost, st));
    }
    // The counting stages (engine.hpp) on K3's output, which K4 leaves where it is (it compacts into d_hits), in the order K6, K7, K8: the
    // batch's last kernels.  Every buffer first — the kernels allocate nothing, so nothing that can fail for want of memory happens once the
    // first of them is on the stream: a batch that is enqueued again after KMCPG_ENOMEM has been counted by none.  One whose hit buffer
    // overflowed is not counted either (the kernels look at the hit counter themselves): collect() runs it again.
    L->counted = counting_mask(db);
    for (int s = 0; s < N_COUNTING; s++)
      if ((L->counted >> s & 1) && (L->d_left[s].ensure(L->n) || L->h_left[s].ensure(L->n))) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
    if (L->counted && L->spec && L->h_roffs3.ensure((size_t)L->n + 1)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
    if (stats_only) {
      if (L->d_mask.ensure(L->n) || L->h_mask.ensure(L->n) || L->d_loffs.ensure((size_t)L->n + 1) || L->d_lstats.ensure(K10_STATS) || L->h_lstats.ensure(K10_STATS))
        return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
      if (int rc2 = left_compact_reserve(db, L->n)) return rc2;
    }
    for (int s = 0; s < N_COUNTING; s++) {
      if (!(L->counted >> s & 1)) continue;
      const char* e = getenv(kCountingStages[s].device_knob);  // KMCPG_*_DEVICE=0: every read goes to the host half
      const int32_t final_n = e && atoi(e) == 0 ? -1 : std::min<int32_t>(L->bound_n, kFprBoundAlways);
      uint8_t* d_left = L->d_left[s].p;
      // (K8 takes the reads' lengths from where the k-mer stage wrote them)
      rc = s == K6   ? refstats_enqueue(db, L->d_pairs.p, L->d_roffs.p, L->d_hits.cap, L->d_qk.p, L->n, final_n, L->d_cnt.p, L->d_hits.cap, d_left, st)
           : s == K7 ? cooccur_enqueue(db, L->d_pairs.p, L->d_roffs.p, L->d_hits.cap, L->d_qk.p, L->n, final_n, L->d_cnt.p, L->d_hits.cap, d_left, 0, st)
                     : recount_enqueue(db, L->d_pairs.p, L->d_roffs.p, L->d_hits.cap, L->d_qk.p, L->d_ql.p, L->n, final_n, L->d_cnt.p, L->d_hits.cap, d_left, 0, st);
      if (rc) return rc;
      if (!stats_only) HIPCHK(hipMemcpyAsync(L->h_left[s].p, d_left, (size_t)L->n, hipMemcpyDeviceToHost, st));
    }
    if (stats_only) {
      // K10 right behind the counting stages: one mask byte per read leaves the GPU instead of the stages' bytes; the pairs of the reads LEFT
      // to the host go into d_hits — dead once K3 has grouped it, and room for d_hits.cap pairs and more — and come down on demand (collect)
      const uint8_t* left[N_COUNTING];
      for (int s = 0; s < N_COUNTING; s++) left[s] = (L->counted >> s & 1) ? L->d_left[s].p : nullptr;
      kmcpg_pair* out = (kmcpg_pair*)L->d_hits.p;
      rc = left_compact_enqueue(db, L->d_pairs.p, L->d_roffs.p, L->d_hits.cap, L->n, left, L->d_cnt.p, L->d_hits.cap, L->d_mask.p, out, L->d_hits.cap, L->d_loffs.p, L->d_lstats.p, st);
      if (rc) return rc;
      HIPCHK(hipMemcpyAsync(L->h_mask.p, L->d_mask.p, (size_t)L->n, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(L->h_lstats.p, L->d_lstats.p, K10_STATS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      L->d_final = out;
    }
    if (L->counted && L->spec) HIPCHK(hipMemcpyAsync(L->h_roffs3.p, L->d_roffs.p, ((size_t)L->n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  } else L->spec = false, L->counted = 0;
  return 0;
}

}  // namespace

// generous_eager: a piece of a large kmcpg_search_batch call — its neighbours of the same batch have just shown how many matches to
// expect, so the eager copy may take all of them (it runs on the copy stream, beside the next piece's kernels)
int enqueue(kmcpg_db* db, AsyncState* A, Lane* L, const kmcpg_params& p, bool generous_eager) {
  KMCPG_USE_DEVICE(db);
  if (!L->done) HIPCHK(hipEventCreateWithFlags(&L->done, hipEventDisableTiming));
  if (!L->uploaded) HIPCHK(hipEventCreateWithFlags(&L->uploaded, hipEventDisableTiming));
  const uint32_t n = L->n;
  if (n == 0) return 0;
  {
    // two kernel streams taken in turn: for every batch (KMCPG_KSTREAMS=2) or, by default, for batches of whole genomes — their k-mer kernel runs
    // beside the COBS kernel of the batch before (query.cpp pick_slot gives such a batch the second workspace); the stream is made when first needed
    std::lock_guard<std::mutex> g(A->mu);
    const bool two = A->kstreams == 2 || (A->kstreams == 0 && whole_genome_batch(db, L->maxlen, L->paired));
    if (two && !A->stream2) HIPCHK(hipStreamCreateWithFlags(&A->stream2, hipStreamNonBlocking));
    L->st = (two && (A->enqueued++ & 1)) ? A->stream2 : A->stream;
  }
  hipStream_t st = L->st;
  // the sizes of the hit buffers and of the eager copy: lane_plan.hpp
  // (d_pairs is sized by d_hits.cap and re-ensured by enqueue_query: it goes wherever d_hits goes)
  const HitPlan hp = plan_hit_buffers(n, A->hits_hint.load(), A->lane_hit_budget, L->d_hits.cap, generous_eager);
  const uint64_t base_cap = hp.base_cap;
  if (hp.release) {
    L->d_hits.release();
    L->d_pairs.release();
  }
  uint64_t first = hp.first;
  const uint64_t up_bases = L->up_bases;  // (the batch itself, or — sliding windows — the slices of reads its windows view)
  const size_t up_reads = L->up_reads;
  if (L->d_seqs.ensure(up_bases + 16) || L->d_offs.ensure((size_t)n + 1) || L->d_cnt.ensure(2) || L->d_qk.ensure(n) || L->d_ql.ensure(n) ||
      (L->paired && (L->d_seqs2.ensure(L->tb2 + 16) || L->d_offs2.ensure((size_t)n + 1))) ||
      (L->win && (L->d_soffs.ensure(up_reads + 1) || L->d_wmeta.ensure(3 * (up_reads + 1)) || L->d_wsrc.ensure(n))))
    return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
  if (L->d_hits.ensure(std::max<uint64_t>(L->d_hits.cap, hp.want))) {  // no room for the generous size next to the index: the plain one, and a rerun if it overflows
    (void)hipGetLastError();
    if (L->d_hits.ensure(base_cap)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
    first = std::min(first, base_cap);
  }
  // K3 only where this handle holds the whole database: the lists of shards (several GPUs, passes of a paged handle) are merged first
  L->grouped = A->device_finalize && !A->hits_stay_on_device && db->opts.shard_count == 1;
  // (a batch searched for statistics or for bins only brings no pairs down but those of the reads LEFT to the host: collect sizes h_pairs for them)
  if (L->h_cnt.ensure(2) || L->h_qk.ensure(n) || L->h_ql.ensure(n) || (L->grouped ? (!L->stats && !L->bins && L->h_pairs.ensure(first)) : L->h_hits.ensure(first)))
    return kmcpg_fail(KMCPG_ENOMEM, "hipHostMalloc failed");
  // the reads go up on a stream of their own (150 MB per million reads: 4 ms of PCIe that would otherwise sit between the
  // kernels of consecutive batches); the lane's device buffers are idle, its previous batch was waited for
  hipStream_t up = A->up_stream;
  if (L->packed) {
    if (L->d_pack.ensure(up_bases / 4 + 16) || (L->n_exc && L->d_exc.ensure(L->n_exc))) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
    HIPCHK(hipMemcpyAsync(L->d_pack.p, L->ext_pack ? L->ext_pack : L->h_pack.p, (up_bases + 3) / 4, hipMemcpyHostToDevice, up));
    if (L->n_exc) HIPCHK(hipMemcpyAsync(L->d_exc.p, L->h_exc.p, (size_t)L->n_exc * sizeof(ExcRun), hipMemcpyHostToDevice, up));
  } else if (up_bases) {
    HIPCHK(hipMemcpyAsync(L->d_seqs.p, L->h_seqs.p, up_bases, hipMemcpyHostToDevice, up));
  }
  if (L->win) {
    HIPCHK(hipMemcpyAsync(L->d_soffs.p, L->h_offs.p, (up_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, up));
    HIPCHK(hipMemcpyAsync(L->d_wmeta.p, L->h_wmeta.p, 3 * (up_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, up));
  } else {
    HIPCHK(hipMemcpyAsync(L->d_offs.p, L->h_offs.p, ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, up));
  }
  if (L->paired) {
    if (L->tb2) HIPCHK(hipMemcpyAsync(L->d_seqs2.p, L->h_seqs2.p, L->tb2, hipMemcpyHostToDevice, up));
    HIPCHK(hipMemcpyAsync(L->d_offs2.p, L->h_offs2.p, ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, up));
  }
  HIPCHK(hipEventRecord(L->uploaded, up));
  // the kernel stream waits for the upload (and expands packed input) in front of THIS batch's first kernel, under the handle's enqueue
  // lock: see query.cpp query_device_after
  const std::function<int()> after_upload = [&]() -> int {
    HIPCHK(hipStreamWaitEvent(st, L->uploaded, 0));
    if (L->win) return describe_windows(lane_windows(L), st);  // the windows' descriptors, in front of the k-mer kernels that read through them
    return 0;
  };
  int rc = enqueue_query(db, A, L, p, &after_upload);
  if (rc == KMCPG_ENOMEM) {
    // the shared workspace (hashes, dedup scratch, long-query counters) did not fit: hit buffers above the plain size are the
    // one thing on this handle that can give memory back — those of the idle lanes and this lane's own — then once more
    (void)hipGetLastError();
    {
      std::lock_guard<std::mutex> g(A->mu);
      for (auto& l : A->lanes)
        if (!l->busy && l.get() != L && l->d_hits.cap > 0) {
          l->d_hits.release();
          l->d_pairs.release();
        }
    }
    if (L->d_hits.cap > base_cap + base_cap / 8 + 64) {
      HIPCHK(hipStreamSynchronize(st));  // kernels of the failed attempt may have been enqueued with the old buffer
      L->d_hits.release();
      L->d_pairs.release();
      if (L->d_hits.ensure(base_cap)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
    }
    rc = enqueue_query(db, A, L, p);
  }
  if (rc) return rc;
  if (!L->bins_only()) {  // (a batch searched for bins needs the k-mer counts only if K11 LEFT a read: collect asks for them; the lengths never)
    HIPCHK(hipMemcpyAsync(L->h_qk.p, L->d_qk.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(L->h_ql.p, L->d_ql.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  }
  L->copied = A->hits_stay_on_device ? 0 : std::min<uint64_t>(first, L->d_hits.cap);
  L->eager_aside = false;
  if (L->summarized() || L->stats_only() || L->bins_only()) L->copied = 0;  // no eager copy of pairs: what the host needs of them (the LEFT windows', the LEFT reads') it asks for by itself
  if (L->copied && L->grouped && !generous_eager) {
    // a small copy (<= 32 pairs per read), in stream order before the lane's completion event (same-box A/B: on a stream of its own it
    // cost the pipelined submit / wait path 8 %)
    HIPCHK(hipMemcpyAsync(L->h_pairs.p, L->d_final, L->copied * sizeof(kmcpg_pair), hipMemcpyDeviceToHost, st));
  } else if (L->copied && L->grouped) {
    // a piece of a large kmcpg_search_batch call: all of its ordered pairs leave on the copy stream, behind K3 only, while the
    // next piece's kernels run
    L->eager_aside = true;
    if (!L->k3_ev) HIPCHK(hipEventCreateWithFlags(&L->k3_ev, hipEventDisableTiming));
    if (!L->eager_ev) HIPCHK(hipEventCreateWithFlags(&L->eager_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(L->k3_ev, st));
    HIPCHK(hipStreamWaitEvent(A->copy_stream, L->k3_ev, 0));
    HIPCHK(hipMemcpyAsync(L->h_pairs.p, L->d_final, L->copied * sizeof(kmcpg_pair), hipMemcpyDeviceToHost, A->copy_stream));
    HIPCHK(hipEventRecord(L->eager_ev, A->copy_stream));
  } else if (L->copied) HIPCHK(hipMemcpyAsync(L->h_hits.p, L->d_hits.p, L->copied * sizeof(kmcpg_hit), hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(L->done, st));
  return 0;
}

namespace {
// the host half of the counting stages for a finished batch: the reads their kernels LEFT, from K3's pairs — which are the lane's result
// itself, or, behind K4 or where the caller did not fetch them, still in d_pairs: one download for all the stages, and none if no read was LEFT
int left_collect(kmcpg_db* db, AsyncState* A, Lane* L, const kmcpg_params& p, bool fetched) {
  const unsigned mask = L->counted & counting_mask(db);
  const uint8_t* left[N_COUNTING] = {};
  bool any = false;
  for (int s = 0; s < N_COUNTING; s++) {
    if (!(mask >> s & 1)) continue;
    left[s] = L->h_left[s].p;
    for (uint32_t r = 0; r < L->n && !any; r++) any = left[s][r] != 0;
  }
  if (!any) return 0;
  const kmcpg_pair* pairs = L->h_pairs.p;
  const uint64_t* offs = L->spec ? L->h_roffs3.p : L->h_roffs.p;
  std::vector<kmcpg_pair, NoInitAlloc<kmcpg_pair>> k3;
  if (L->spec || !fetched) {
    k3.resize(offs[L->n]);
    if (!k3.empty()) {
      HIPCHK(hipMemcpyAsync(k3.data(), L->d_pairs.p, k3.size() * sizeof(kmcpg_pair), hipMemcpyDeviceToHost, A->copy_stream));
      HIPCHK(hipStreamSynchronize(A->copy_stream));
    }
    pairs = k3.data();
  }
  return left_reads_host(db, pairs, offs, L->h_qk.p, L->h_ql.p, L->n, p, mask, left);
}

// ... of a batch searched for statistics only (Lane::stats_only): the mask bytes and the witness words are here; if a read was LEFT, K10's
// offsets and the pairs it compacted come down now — nothing else of the batch's matches ever does — and the mask is split into the
// per-stage bytes the host half takes.  Reads that were not LEFT have empty segments there.  Fills L->left_res
int stats_collect(kmcpg_db* db, AsyncState* A, Lane* L, const kmcpg_params& p) {
  const uint32_t n = L->n;
  const unsigned long long* w = L->h_lstats.p;
  kmcpg_stats_ticket_stats& r = L->left_res;
  r = kmcpg_stats_ticket_stats{};
  r.k10_ms = -1;
  r.n_reads = n;
  r.matched_reads = w[K10_MATCHED];
  r.kept_pairs = L->h_roffs.p[n];
  r.left_reads = w[K10_LEFT];
  r.left_pairs = w[K10_LEFT_PAIRS];
  r.bad_segments = w[K10_BAD];
  r.skipped = w[K10_SKIPPED];
  // the two hit counters, K3's last two words, the witness words, qkmers / qlen and the mask
  r.bytes_d2h = 4 * sizeof(uint64_t) + K10_STATS * sizeof(unsigned long long) + (uint64_t)n * (2 * sizeof(int32_t) + 1);
  if (r.skipped || r.left_pairs > r.kept_pairs || r.left_pairs > L->d_hits.cap)
    return kmcpg_fail(KMCPG_EDEVICE, "internal: K10 left %llu pairs of %llu (skipped: %llu)", (unsigned long long)r.left_pairs, (unsigned long long)r.kept_pairs,
                      (unsigned long long)r.skipped);
  if (r.left_reads == 0) return 0;
  if (L->h_loffs.ensure((size_t)n + 1) || L->h_pairs.ensure(r.left_pairs + 1)) return kmcpg_fail(KMCPG_ENOMEM, "hipHostMalloc failed");
  HIPCHK(hipMemcpyAsync(L->h_loffs.p, L->d_loffs.p, ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, A->copy_stream));
  if (r.left_pairs) HIPCHK(hipMemcpyAsync(L->h_pairs.p, L->d_final, r.left_pairs * sizeof(kmcpg_pair), hipMemcpyDeviceToHost, A->copy_stream));
  HIPCHK(hipStreamSynchronize(A->copy_stream));
  r.bytes_d2h += ((uint64_t)n + 1) * sizeof(uint64_t) + r.left_pairs * sizeof(kmcpg_pair);
  if (L->h_loffs.p[n] != r.left_pairs) return kmcpg_fail(KMCPG_EDEVICE, "internal: K10 compacted %llu pairs, counted %llu", (unsigned long long)L->h_loffs.p[n], (unsigned long long)r.left_pairs);
  const unsigned mask = L->counted & counting_mask(db);
  std::vector<uint8_t> bytes[N_COUNTING];
  const uint8_t* left[N_COUNTING] = {};
  for (int s = 0; s < N_COUNTING; s++) {
    if (!(mask >> s & 1)) continue;
    bytes[s].resize(n);
    for (uint32_t i = 0; i < n; i++) bytes[s][i] = L->h_mask.p[i] >> s & 1;
    left[s] = bytes[s].data();
  }
  return left_reads_host(db, L->h_pairs.p, L->h_loffs.p, L->h_qk.p, L->h_ql.p, n, p, mask, left);
}

// ... of a batch searched for bins only (Lane::bins_only): the bins and the two witnesses are here; if K11 LEFT a read, the k-mer counts,
// K10's offsets and the pairs it compacted come down now, and the host half (finalize.cpp bins_left_host) writes those reads' bins over
// the LEFT words.  Fills L->bin_res and the three totals beside it
int bins_collect(kmcpg_db* db, AsyncState* A, Lane* L, const kmcpg_params& p) {
  const uint32_t n = L->n;
  const unsigned long long *w = L->h_bstats.p, *lw = L->h_lstats.p;
  kmcpg_bin_stats& r = L->bin_res;
  r = kmcpg_bin_stats{};
  r.k11_ms = -1;
  bin_stats_from_words(w, &r);
  L->bin_kept_pairs = L->h_roffs.p[n];
  L->bin_left_pairs = lw[K10_LEFT_PAIRS];
  // the two hit counters, K3's last two words, the two witnesses and the bins
  L->bin_bytes_d2h = 4 * sizeof(uint64_t) + (K11_STATS + K10_STATS) * sizeof(unsigned long long) + (uint64_t)n * sizeof(uint32_t);
  if (r.skipped || lw[K10_SKIPPED] || lw[K10_LEFT] != r.left || L->bin_left_pairs > L->bin_kept_pairs || L->bin_left_pairs > L->d_hits.cap ||
      r.no_bin + r.one + r.several + r.left != n)
    return kmcpg_fail(KMCPG_EDEVICE, "internal: K11 binned %llu + %llu + %llu reads and left %llu of %u (K10: %llu reads, %llu pairs of %llu; skipped: %llu, %llu)",
                      (unsigned long long)r.no_bin, (unsigned long long)r.one, (unsigned long long)r.several, (unsigned long long)r.left, n, lw[K10_LEFT], lw[K10_LEFT_PAIRS],
                      (unsigned long long)L->bin_kept_pairs, (unsigned long long)r.skipped, lw[K10_SKIPPED]);
  if (r.left == 0) return 0;
  if (L->h_loffs.ensure((size_t)n + 1) || L->h_pairs.ensure(L->bin_left_pairs + 1)) return kmcpg_fail(KMCPG_ENOMEM, "hipHostMalloc failed");
  HIPCHK(hipMemcpyAsync(L->h_qk.p, L->d_qk.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, A->copy_stream));
  HIPCHK(hipMemcpyAsync(L->h_loffs.p, L->d_loffs.p, ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, A->copy_stream));
  if (L->bin_left_pairs) HIPCHK(hipMemcpyAsync(L->h_pairs.p, L->d_final, L->bin_left_pairs * sizeof(kmcpg_pair), hipMemcpyDeviceToHost, A->copy_stream));
  HIPCHK(hipStreamSynchronize(A->copy_stream));
  L->bin_bytes_d2h += (uint64_t)n * sizeof(int32_t) + ((uint64_t)n + 1) * sizeof(uint64_t) + L->bin_left_pairs * sizeof(kmcpg_pair);
  if (L->h_loffs.p[n] != L->bin_left_pairs)
    return kmcpg_fail(KMCPG_EDEVICE, "internal: K10 compacted %llu pairs, counted %llu", (unsigned long long)L->h_loffs.p[n], (unsigned long long)L->bin_left_pairs);
  uint64_t host_reads = 0;
  if (int rc = bins_left_host(db, L->h_pairs.p, L->h_loffs.p, L->h_qk.p, n, p, L->h_bins.p, &host_reads)) return rc;
  if (host_reads != r.left) return kmcpg_fail(KMCPG_EDEVICE, "internal: the host half binned %llu reads, K11 left %llu", (unsigned long long)host_reads, (unsigned long long)r.left);
  return 0;
}
}  // namespace

int collect(kmcpg_db* db, AsyncState* A, Lane* L, const kmcpg_params& p, uint64_t* n_hits, bool fetch) {
  *n_hits = 0;
  if (L->n == 0) return 0;
  KMCPG_USE_DEVICE(db);
  struct Taint {  // a batch that fails from here on may have been counted by the counting stages already, and a caller may search its reads again
    kmcpg_db* db;
    const Lane* L;
    bool ok = false;
    ~Taint() {
      if (ok || !L->grouped || L->h_cnt.p[0] > L->d_hits.cap) return;  // (an overflowing attempt was not counted: the kernels' guard)
      counting_taint(db, L->counted);
    }
  } taint{db, L};
  HIPCHK(hipEventSynchronize(L->done));
  uint64_t cnt = L->h_cnt.p[0];
  L->reruns = 0;
  for (int attempt = 0; cnt > L->d_hits.cap; attempt++) {  // the hit buffer was too small: rerun with room for every hit
    if (attempt == 2) return kmcpg_fail(KMCPG_ENOMEM, "hit buffer overflow");
    HIPCHK(hipStreamSynchronize(L->st));
    HIPCHK(hipStreamSynchronize(A->copy_stream));  // (the eager copy of the attempt that overflowed)
    if (L->d_hits.ensure(cnt + cnt / 4)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
    int rc = enqueue_query(db, A, L, p);
    if (rc) return rc;
    L->reruns++;
    HIPCHK(hipStreamSynchronize(L->st));
    cnt = L->h_cnt.p[0];
    L->copied = 0;
  }
  // the k-mer count the counter planes were sized for (the longest read) bounds every query's NumKmers
  const uint64_t bound = (uint64_t)L->maxlen * (L->paired ? 2 : 1);
  if (L->h_cnt.p[1] > bound) return kmcpg_fail(KMCPG_EDEVICE, "internal: a query reported %llu k-mers, more than its length allows", (unsigned long long)L->h_cnt.p[1]);
  if (fetch && L->grouped) {
    // K3 ran behind K2: what comes to the host is its output — offsets (already here) and the pairs that passed -T, in final order
    if (L->copied && L->eager_aside) HIPCHK(hipEventSynchronize(L->eager_ev));
    const uint64_t kept = L->h_roffs.p[L->n];
    if (kept > cnt) return kmcpg_fail(KMCPG_EDEVICE, "internal: K3 kept %llu of %llu hits", (unsigned long long)kept, (unsigned long long)cnt);
    if (kept > L->copied) {
      if (kept > L->h_pairs.cap) {
        if (L->h_pairs.ensure(kept)) return kmcpg_fail(KMCPG_ENOMEM, "hipHostMalloc failed");
        L->copied = 0;
      }
      HIPCHK(hipMemcpyAsync(L->h_pairs.p + L->copied, L->d_final + L->copied, (kept - L->copied) * sizeof(kmcpg_pair), hipMemcpyDeviceToHost, A->copy_stream));
      HIPCHK(hipStreamSynchronize(A->copy_stream));
      L->copied = kept;
    }
  } else if (fetch && cnt > L->copied) {
    if (cnt > L->h_hits.cap) {
      if (L->h_hits.ensure(cnt)) return kmcpg_fail(KMCPG_ENOMEM, "hipHostMalloc failed");
      L->copied = 0;
    }
    // the batch's kernels are done (event above): the rest of its hits comes over the copy stream, beside later batches' kernels
    HIPCHK(hipMemcpyAsync(L->h_hits.p + L->copied, L->d_hits.p + L->copied, (cnt - L->copied) * sizeof(kmcpg_hit), hipMemcpyDeviceToHost, A->copy_stream));
    HIPCHK(hipStreamSynchronize(A->copy_stream));
    L->copied = cnt;
  }
  if (L->counted && L->grouped) {
    int rc = L->stats_only() ? stats_collect(db, A, L, p) : left_collect(db, A, L, p, fetch);
    if (rc) return rc;
  }
  if (L->bins_only()) {
    if (int rc = bins_collect(db, A, L, p)) return rc;
  }
  // a batch large enough to say something about the data (one genome with 5 000 matches does not)
  if (L->n >= 1024) A->hits_hint.store(hits_hint_after(A->hits_hint.load(), cnt, L->n));
  *n_hits = cnt;
  taint.ok = true;
  return 0;
}

void drop_ticket(kmcpg_ticket* t, bool failed) {
  for (kmcpg_ticket* pc : t->pieces)
    if (pc) drop_ticket(pc, failed);
  for (kmcpg_result& r : t->piece_res) kmcpg_result_free(&r);
  for (auto& pt : t->parts) {
    if (pt.shard->opts.device >= 0) (void)hipSetDevice(pt.shard->opts.device);
    // the lane must be idle before someone else stages into it
    if (failed && pt.shard->async) drain(pt.shard->async);
    else if (pt.lane->done && pt.lane->n) {
      (void)hipEventSynchronize(pt.lane->done);
      if (pt.lane->grouped && pt.lane->copied && pt.lane->eager_aside && pt.lane->eager_ev) (void)hipEventSynchronize(pt.lane->eager_ev);
    }
    release_lane(pt.shard->async, pt.lane, pt.retry);
  }
  delete t;
}

}  // namespace kmcpg
