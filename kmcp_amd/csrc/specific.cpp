// specific.cpp — the host side of K4 (k4_specific.hip) and of K5 (k5_summary.hip): the tables on the handle, each stage alone, its witness.
#include <cstring>

#include "engine.hpp"
#include "kernels.hpp"
#include "specific_rule.hpp"

using namespace kmcpg;

static_assert(K4_DROP == SPECIFIC_DROP && K4_KEEP == SPECIFIC_KEEP && K4_HOST == SPECIFIC_HOST, "one set of verdict bytes");
static_assert(K4_DROP == KMCPG_SPECIFIC_DROP && K4_KEEP == KMCPG_SPECIFIC_KEEP && K4_HOST == KMCPG_SPECIFIC_HOST, "one set of verdict bytes");

namespace {
constexpr size_t SPEC_STATS_BYTES = 64;  // K4_STATS 32-bit words, then at byte 32 the pairs in and out
static_assert(K4_STATS * sizeof(uint32_t) <= 32, "the 64-bit words start at byte 32");

int refuse(const kmcpg_db* db) { return refuse_handle(db, "species-specific queries", "a query's verdict needs its matches from every block"); }
}  // namespace

extern "C" int kmcpg_set_specific(kmcpg_db* db, const uint32_t* target_class, const uint32_t* species_class, uint32_t n_cols) {
  if (!db) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  const bool off = !target_class && !species_class && n_cols == 0;
  if (!off) {
    if (int rc = refuse(db)) return rc;
    KMCPG_NO_FILES_ONLY(db);
    if (!target_class) return kmcpg_fail(KMCPG_EINVAL, "target_class is needed (species_class alone decides nothing)");
    if (n_cols != db->col_meta.size()) return kmcpg_fail(KMCPG_EINVAL, "n_cols = %u, the handle has %zu columns", n_cols, db->col_meta.size());
  }
  std::lock_guard<std::mutex> g(db->mu);
  const bool dev = db->opts.device >= 0;
  if (dev) {
    HIPCHK(hipSetDevice(db->opts.device));
    HIPCHK(hipDeviceSynchronize());  // batches in flight still read the tables that go
  }
  if (db->d_spec_target) (void)hipFree(db->d_spec_target);
  if (db->d_spec_species) (void)hipFree(db->d_spec_species);
  db->d_spec_target = db->d_spec_species = nullptr;
  db->h_spec_target.clear();
  db->h_spec_species.clear();
  db->spec_ran = false;
  db->k4_log.clear();
  db->sum_ran = false;
  db->k5_log.clear();
  if (off || n_cols == 0) return 0;
  if (dev) {
    const size_t bytes = (size_t)n_cols * sizeof(uint32_t);
    if (hipMalloc((void**)&db->d_spec_target, bytes) != hipSuccess) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc of %zu bytes failed", bytes);
    HIPCHK(hipMemcpy(db->d_spec_target, target_class, bytes, hipMemcpyHostToDevice));
    if (species_class) {
      if (hipMalloc((void**)&db->d_spec_species, bytes) != hipSuccess) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc of %zu bytes failed", bytes);
      HIPCHK(hipMemcpy(db->d_spec_species, species_class, bytes, hipMemcpyHostToDevice));
    }
    if (!db->d_spec_stats) {
      HIPCHK(hipMalloc((void**)&db->d_spec_stats, SPEC_STATS_BYTES));
      HIPCHK(hipMemset(db->d_spec_stats, 0, SPEC_STATS_BYTES));
    }
  }
  db->h_spec_target.assign(target_class, target_class + n_cols);
  if (species_class) db->h_spec_species.assign(species_class, species_class + n_cols);
  return 0;
}

extern "C" int kmcpg_specific_device(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers,
                                     uint32_t n_reads, int32_t final_n, kmcpg_pair* d_out_pairs, uint64_t out_cap, uint64_t* d_out_offs,
                                     uint8_t* d_verdicts, void* stream) {
  if (!db || !d_read_offs || !d_out_offs || (n_reads && (!d_qkmers || !d_verdicts)) || (pair_cap && (!d_pairs || !d_out_pairs)))
    return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (out_cap < pair_cap) return kmcpg_fail(KMCPG_EINVAL, "out_cap (%llu) must be at least pair_cap (%llu)", (unsigned long long)out_cap, (unsigned long long)pair_cap);
  if (n_reads == 0xffffffffu) return kmcpg_fail(KMCPG_EINVAL, "too many reads");
  if (int rc = refuse(db)) return rc;
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  if (!db->spec_on() || !db->d_spec_target) return kmcpg_fail(KMCPG_EINVAL, "the stage is off: call kmcpg_set_specific first");
  hipStream_t st = (hipStream_t)stream;
  FinGuard fing{db, st};  // the scratch has one user at a time: K3's chain (kmcpg_group_device)
  if (int rc = fing.wait()) return rc;
  if (db->w_spec_cnt.ensure((size_t)n_reads + 2) || db->w_spec_sums.ensure((size_t)k3_scan_tiles_for(n_reads + 1) + 1)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
  HIPCHK(hipMemsetAsync(db->d_spec_stats, 0, SPEC_STATS_BYTES, st));
  db->k4_log.clear();
  db->spec_ran = true;
  if (n_reads == 0) {
    db->spec_timed = false;
    HIPCHK(hipMemsetAsync(d_out_offs, 0, sizeof(uint64_t), st));
    return 0;
  }
  K4Args a{};
  a.pairs = d_pairs;
  a.offs = d_read_offs;
  a.pair_cap = pair_cap;
  a.nk = d_qkmers;
  a.n_reads = n_reads;
  a.n_cols = (uint32_t)db->h_spec_target.size();
  a.final_n = final_n;
  a.target_class = db->d_spec_target;
  a.species_class = db->d_spec_species;
  a.cnt = db->w_spec_cnt.p;
  a.sums = db->w_spec_sums.p;
  a.verdict = d_verdicts;
  a.out_pairs = d_out_pairs;
  a.out_offs = d_out_offs;
  a.out_cap = out_cap;
  a.stats = (uint32_t*)db->d_spec_stats;
  db->spec_timed = db->profiling >= 1;
  if (int rc = timed_launches(db->spec_ev, db->spec_timed, st, [&] { launch_k4(a, st, db->spec_timed ? &db->k4_log : nullptr); })) return rc;
  // the witness's pairs in and out: the last offsets, kept where the caller's buffers need not outlive the call
  HIPCHK(hipMemcpyAsync(db->d_spec_stats + 4, d_read_offs + n_reads, sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(db->d_spec_stats + 5, d_out_offs + n_reads, sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int kmcpg_last_specific(kmcpg_db* db, kmcpg_specific_stats* out, kmcpg_k4_launch* launches, uint32_t cap, uint32_t* n_launches) {
  static_assert(sizeof(kmcpg_k4_launch) == 16, "four 4-byte words");
  if (!db || !out || !n_launches || (cap && !launches)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  memset(out, 0, sizeof *out);
  out->k4_ms = -1;
  *n_launches = 0;
  std::lock_guard<std::mutex> g(db->mu);
  if (!db->spec_ran || db->opts.device < 0 || !db->d_spec_stats) return 0;
  KMCPG_USE_DEVICE(db);
  HIPCHK(hipDeviceSynchronize());
  uint64_t w[SPEC_STATS_BYTES / 8] = {};
  HIPCHK(hipMemcpy(w, db->d_spec_stats, SPEC_STATS_BYTES, hipMemcpyDeviceToHost));
  uint32_t s[K4_STATS];
  memcpy(s, w, sizeof s);
  out->kept = s[0];
  out->dropped = s[1];
  out->host = s[2];
  out->group_segments = s[3];
  out->wave_segments = s[4];
  out->bad_segments = s[5];
  out->pairs_in = w[4];
  out->pairs_out = w[5];
  timed_launches_report(db, db->spec_ev, db->spec_timed, db->k4_log, &out->k4_ms, launches, cap, n_launches);
  return 0;
}

// ---- K5: window summaries behind K4
extern "C" int kmcpg_summarize_device(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_offs, uint64_t pair_cap, const uint8_t* d_verdicts,
                                      const int32_t* d_qkmers, uint32_t n, kmcpg_window_summary* d_out, kmcpg_pair* d_left_pairs, uint64_t left_cap,
                                      uint64_t* d_left_offs, void* stream) {
  static_assert(sizeof(kmcpg_window_summary) == 16, "two 4-byte words and a double");
  static_assert(K5_STATS * sizeof(uint32_t) <= 32, "the 64-bit word starts at byte 32");
  if (!db || !d_offs || !d_left_offs || (n && (!d_qkmers || !d_verdicts || !d_out)) || (pair_cap && (!d_pairs || !d_left_pairs)))
    return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (left_cap < pair_cap) return kmcpg_fail(KMCPG_EINVAL, "left_cap (%llu) must be at least pair_cap (%llu)", (unsigned long long)left_cap, (unsigned long long)pair_cap);
  if (n == 0xffffffffu) return kmcpg_fail(KMCPG_EINVAL, "too many windows");
  if (int rc = refuse(db)) return rc;
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  if (!db->spec_on() || !db->d_spec_target) return kmcpg_fail(KMCPG_EINVAL, "the stage is off: call kmcpg_set_specific first");
  hipStream_t st = (hipStream_t)stream;
  FinGuard fing{db, st};  // the scratch has one user at a time: K3's chain (kmcpg_group_device), K4 (kmcpg_specific_device)
  if (int rc = fing.wait()) return rc;
  if (db->w_spec_cnt.ensure((size_t)n + 2) || db->w_spec_sums.ensure((size_t)k3_scan_tiles_for(n + 1) + 1)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
  if (!db->d_sum_stats) HIPCHK(hipMalloc((void**)&db->d_sum_stats, SPEC_STATS_BYTES));
  HIPCHK(hipMemsetAsync(db->d_sum_stats, 0, SPEC_STATS_BYTES, st));
  db->k5_log.clear();
  db->sum_ran = true;
  db->sum_from_ticket = false;
  if (n == 0) {
    db->sum_timed = false;
    HIPCHK(hipMemsetAsync(d_left_offs, 0, sizeof(uint64_t), st));
    return 0;
  }
  K5Args a{};
  a.pairs = d_pairs;
  a.offs = d_offs;
  a.pair_cap = pair_cap;
  a.verdict = d_verdicts;
  a.nk = d_qkmers;
  a.n_reads = n;
  a.n_cols = (uint32_t)db->h_spec_target.size();
  a.target_class = db->d_spec_target;
  a.out = d_out;
  a.cnt = db->w_spec_cnt.p;
  a.sums = db->w_spec_sums.p;
  a.left_pairs = d_left_pairs;
  a.left_offs = d_left_offs;
  a.left_cap = left_cap;
  a.stats = (uint32_t*)db->d_sum_stats;
  db->sum_timed = db->profiling >= 1;
  if (int rc = timed_launches(db->sum_ev, db->sum_timed, st, [&] { launch_k5(a, st, db->sum_timed ? &db->k5_log : nullptr); })) return rc;
  // the witness's LEFT pairs: the last offset, kept where the caller's buffers need not outlive the call
  HIPCHK(hipMemcpyAsync(db->d_sum_stats + 4, d_left_offs + n, sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int kmcpg_last_summary(kmcpg_db* db, kmcpg_summary_stats* out, kmcpg_k4_launch* launches, uint32_t cap, uint32_t* n_launches) {
  if (!db || !out || !n_launches || (cap && !launches)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  memset(out, 0, sizeof *out);
  out->k5_ms = -1;
  *n_launches = 0;
  std::lock_guard<std::mutex> g(db->mu);
  if (!db->sum_ran || db->opts.device < 0) return 0;
  if (!db->d_sum_stats) {  // a ticket no batch of which reached K5 (KMCPG_DEVICE_FINALIZE=0)
    if (db->sum_from_ticket) *out = db->sum_ticket, out->k5_ms = -1;
    return 0;
  }
  KMCPG_USE_DEVICE(db);
  HIPCHK(hipDeviceSynchronize());
  if (db->sum_from_ticket) {
    *out = db->sum_ticket;
    out->k5_ms = -1;
  }
  uint64_t w[SPEC_STATS_BYTES / 8] = {};
  HIPCHK(hipMemcpy(w, db->d_sum_stats, SPEC_STATS_BYTES, hipMemcpyDeviceToHost));
  uint32_t s[K5_STATS];
  memcpy(s, w, sizeof s);
  out->bad_segments = s[4];
  if (!db->sum_from_ticket) {
    out->single = s[0];
    out->wave = s[1];
    out->left = s[2];
    out->empty = s[3];
    out->left_pairs = w[4];
  }
  timed_launches_report(db, db->sum_ev, db->sum_timed, db->k5_log, &out->k5_ms, launches, cap, n_launches);
  return 0;
}
