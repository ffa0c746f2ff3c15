// stats.cpp — the host side of K10 (k10_left.hip): the stage alone on device pointers, the form a lane enqueues behind the counting
// stages of a statistics-only batch (kmcpg_submit_stats: host.cpp, lane.cpp), and the witness.
#include <hip/hip_runtime.h>
#include <string.h>

#include <mutex>

#include "engine.hpp"
#include "kernels.hpp"

using namespace kmcpg;

static_assert(K10_STAGES == N_COUNTING, "a mask bit per counting stage, in the order of engine.hpp");

namespace kmcpg {

// (the caller holds db->mu and has made the handle's device current)
static int reserve_locked(kmcpg_db* db, uint32_t n_reads) {
  if (db->w_spec_cnt.ensure((size_t)n_reads + 2) || db->w_spec_sums.ensure((size_t)k3_scan_tiles_for(n_reads + 1) + 1) || db->w_left_offs.ensure((size_t)n_reads + 1))
    return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
  if (!db->d_left_stats) HIPCHK(hipMalloc((void**)&db->d_left_stats, K10_STATS * sizeof(unsigned long long)));
  return 0;
}

int left_compact_reserve(kmcpg_db* db, uint32_t n_reads) {
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  return reserve_locked(db, n_reads);
}

int left_compact_enqueue(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, uint32_t n_reads, const uint8_t* const d_left[N_COUNTING],
                         const uint64_t* d_n_hits, uint64_t hit_cap, uint8_t* d_mask, kmcpg_pair* d_left_pairs, uint64_t left_cap, uint64_t* d_left_offs,
                         unsigned long long* d_stats, hipStream_t st) {
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  FinGuard fing{db, st};  // the scratch has one user at a time: K3's chain (kmcpg_group_device), K4, K5
  if (int rc = fing.wait()) return rc;
  if (int rc = reserve_locked(db, n_reads)) return rc;
  unsigned long long* const stats = d_stats ? d_stats : db->d_left_stats;
  HIPCHK(hipMemsetAsync(stats, 0, K10_STATS * sizeof(unsigned long long), st));
  db->k10_log.clear();
  db->left_ran = true;
  if (!d_stats) db->left_from_ticket = false;  // (a lane's launch is reported with its ticket: kmcpg_wait_stats)
  db->left_timed = false;
  if (n_reads == 0) {
    HIPCHK(hipMemsetAsync(d_left_offs, 0, sizeof(uint64_t), st));
    return 0;
  }
  K10Args a{};
  a.offs = d_read_offs;
  a.pair_cap = pair_cap;
  a.n_reads = n_reads;
  for (int s = 0; s < N_COUNTING; s++) a.left[s] = d_left[s];
  a.n_hits = (const unsigned long long*)d_n_hits;
  a.hit_cap = hit_cap;
  a.mask = d_mask;
  a.cnt = db->w_spec_cnt.p;
  a.stats = stats;
  db->left_timed = db->profiling >= 1;
  if (int rc = timed_launches(db->left_ev, db->left_timed, st, [&] {
        launch_k10(a, d_pairs, db->w_spec_sums.p, db->w_left_offs.p, d_left_pairs, left_cap, d_left_offs, st, db->left_timed ? &db->k10_log : nullptr);
      }))
    return rc;
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace kmcpg

extern "C" int kmcpg_left_compact_device(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, uint32_t n_reads,
                                         const uint8_t* d_left_refstats, const uint8_t* d_left_cooccur, const uint8_t* d_left_recount, const uint64_t* d_n_hits,
                                         uint64_t hit_cap, uint8_t* d_mask, kmcpg_pair* d_left_pairs, uint64_t left_cap, uint64_t* d_left_offs, void* stream) {
  if (!db || !d_read_offs || !d_left_offs || (n_reads && !d_mask) || (pair_cap && (!d_pairs || !d_left_pairs))) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (left_cap < pair_cap) return kmcpg_fail(KMCPG_EINVAL, "left_cap (%llu) must be at least pair_cap (%llu)", (unsigned long long)left_cap, (unsigned long long)pair_cap);
  if (n_reads == 0xffffffffu) return kmcpg_fail(KMCPG_EINVAL, "too many reads");
  const uint8_t* const left[N_COUNTING] = {d_left_refstats, d_left_cooccur, d_left_recount};
  return left_compact_enqueue(db, d_pairs, d_read_offs, pair_cap, n_reads, left, d_n_hits, hit_cap, d_mask, d_left_pairs, left_cap, d_left_offs, nullptr, (hipStream_t)stream);
}

extern "C" int kmcpg_last_stats(kmcpg_db* db, kmcpg_stats_ticket_stats* out, kmcpg_k4_launch* launches, uint32_t cap, uint32_t* n_launches) {
  if (!db || !out || !n_launches || (cap && !launches)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  memset(out, 0, sizeof *out);
  out->k10_ms = -1;
  *n_launches = 0;
  std::lock_guard<std::mutex> g(db->mu);
  if (!db->left_ran || db->opts.device < 0 || !db->d_left_stats) return 0;
  KMCPG_USE_DEVICE(db);
  HIPCHK(hipDeviceSynchronize());
  if (db->left_from_ticket) *out = db->left_ticket, out->k10_ms = -1;
  else {
    unsigned long long s[K10_STATS] = {};
    HIPCHK(hipMemcpy(s, db->d_left_stats, sizeof s, hipMemcpyDeviceToHost));
    out->matched_reads = s[K10_MATCHED];
    out->left_reads = s[K10_LEFT];
    out->left_pairs = s[K10_LEFT_PAIRS];
    out->bad_segments = s[K10_BAD];
    out->skipped = s[K10_SKIPPED];
  }
  timed_launches_report(db, db->left_ev, db->left_timed, db->k10_log, &out->k10_ms, launches, cap, n_launches);
  return 0;
}
