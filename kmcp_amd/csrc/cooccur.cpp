// cooccur.cpp — the host side of K7 (k7_cooccur.hip): the class table and the pair table on the handle, the stage alone, the merge of the
// device's table and the host half's map, the witness.  The host half itself (the reads the device LEFT) is beside the other users of the
// match rule, in finalize.cpp (left_reads_host, the one walk of all the counting stages, and counting_host_result).
#include <cstring>

#include "cooccur_rule.hpp"
#include "engine.hpp"
#include "kernels.hpp"

using namespace kmcpg;

namespace {

// the handles K6 refuses (refstats.cpp), for the same reason
int refuse(const kmcpg_db* db) { return refuse_handle(db, "shared reads of reference pairs", "a query's pairs need its matches from every block"); }

// KMCPG_COOCCUR_SLOTS: a power of two up to K7_MAX_SLOTS, 0 = no LDS table; false: neither
bool slots_from_env(uint32_t* slots) {
  *slots = K7_DEFAULT_SLOTS;
  const char* e = getenv("KMCPG_COOCCUR_SLOTS");
  if (!e) return true;
  char* end = nullptr;
  const long v = strtol(e, &end, 10);
  if (end == e || *end || v < 0 || v > (long)K7_MAX_SLOTS || (v & (v - 1))) return false;
  *slots = (uint32_t)v;
  return true;
}

void free_device(kmcpg_db* db) {
  for (void* q : {(void*)db->d_co_target, (void*)db->d_co_keys, (void*)db->d_co_counts, (void*)db->d_co_totals})
    if (q) (void)hipFree(q);
  db->d_co_target = nullptr;
  db->d_co_keys = db->d_co_counts = db->d_co_totals = nullptr;
}

}  // namespace

extern "C" int kmcpg_set_cooccur(kmcpg_db* db, const uint32_t* target_class, uint32_t n_cols, uint64_t table_slots) {
  if (!db) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  const bool off = !target_class && n_cols == 0;
  uint32_t slots = 0;
  if (!off) {
    if (int rc = refuse(db)) return rc;
    KMCPG_NO_FILES_ONLY(db);
    if (!target_class) return kmcpg_fail(KMCPG_EINVAL, "target_class is needed");
    if (n_cols != db->col_meta.size()) return kmcpg_fail(KMCPG_EINVAL, "n_cols = %u, the handle has %zu columns", n_cols, db->col_meta.size());
    if (table_slots == 0) table_slots = K7_DEFAULT_TABLE;
    if ((table_slots & (table_slots - 1)) || table_slots > K7_MAX_TABLE)
      return kmcpg_fail(KMCPG_EINVAL, "table_slots = %llu, must be a power of two up to %llu (0: the default, %llu)", (unsigned long long)table_slots,
                        (unsigned long long)K7_MAX_TABLE, (unsigned long long)K7_DEFAULT_TABLE);
    if (!slots_from_env(&slots)) return kmcpg_fail(KMCPG_EINVAL, "KMCPG_COOCCUR_SLOTS = %s, must be a power of two up to %u, or 0", getenv("KMCPG_COOCCUR_SLOTS"), K7_MAX_SLOTS);
  }
  std::lock_guard<std::mutex> g(db->mu);
  const bool dev = db->opts.device >= 0;
  if (dev) {
    HIPCHK(hipSetDevice(db->opts.device));
    HIPCHK(hipDeviceSynchronize());  // batches in flight still read the class table and add to the pair table that go
  }
  free_device(db);
  std::lock_guard<std::mutex> gh(db->co_mu);
  db->h_co_target.clear();
  db->h_co_pairs.clear();
  db->h_co_multi = db->h_co_adds = 0;
  db->co_tainted = db->co_ran = false;
  db->co_table = 0;
  db->k7_log.clear();
  if (off || n_cols == 0) return 0;
  db->h_co_target.assign(target_class, target_class + n_cols);
  db->co_slots = slots;
  db->co_table = table_slots;
  if (dev) {
    const size_t bytes = (size_t)n_cols * sizeof(uint32_t), tbytes = (size_t)table_slots * sizeof(unsigned long long);
    bool ok = hipMalloc((void**)&db->d_co_target, bytes) == hipSuccess && hipMalloc((void**)&db->d_co_keys, tbytes) == hipSuccess &&
              hipMalloc((void**)&db->d_co_counts, tbytes) == hipSuccess && hipMalloc((void**)&db->d_co_totals, K7_TOTALS * sizeof(unsigned long long)) == hipSuccess;
    if (ok && !db->d_co_stats) ok = hipMalloc((void**)&db->d_co_stats, K7_STATS * sizeof(unsigned long long)) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      free_device(db);
      db->h_co_target.clear();  // the stage stays off
      return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc of the pair table (%llu slots) failed", (unsigned long long)table_slots);
    }
    HIPCHK(hipMemcpy(db->d_co_target, target_class, bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(db->d_co_keys, 0, tbytes));
    HIPCHK(hipMemset(db->d_co_counts, 0, tbytes));
    HIPCHK(hipMemset(db->d_co_totals, 0, K7_TOTALS * sizeof(unsigned long long)));
    HIPCHK(hipMemset(db->d_co_stats, 0, K7_STATS * sizeof(unsigned long long)));
    // persistent workgroups: two per CU, as K6 (refstats.cpp)
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, db->opts.device));
    db->co_max_wgs = (unsigned)std::max(1, prop.multiProcessorCount) * 2;
    if (const char* e = getenv("KMCPG_COOCCUR_WGS")) db->co_max_wgs = (unsigned)std::max(1, atoi(e));
  }
  return 0;
}

namespace kmcpg {
int cooccur_enqueue(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers, uint32_t n_reads,
                    int32_t final_n, const uint64_t* d_n_hits, uint64_t hit_cap, uint8_t* d_left, unsigned max_wgs, hipStream_t st) {
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  if (!db->cooccur_on() || !db->d_co_target) return kmcpg_fail(KMCPG_EINVAL, "the stage is off: call kmcpg_set_cooccur first");
  HIPCHK(hipMemsetAsync(db->d_co_stats, 0, K7_STATS * sizeof(unsigned long long), st));
  db->k7_log.clear();
  db->co_ran = true;
  db->co_grid = 0;
  db->co_timed = false;
  if (n_reads == 0) return 0;
  K7Args a{};
  a.pairs = d_pairs;
  a.offs = d_read_offs;
  a.pair_cap = pair_cap;
  a.nk = d_qkmers;
  a.n_reads = n_reads;
  a.n_cols = (uint32_t)db->h_co_target.size();
  a.final_n = final_n;
  a.slots = db->co_slots;  // (a slot's counter is 32 bits wide: a workgroup adds at most once per read and pair, and n_reads < 2^32)
  a.target_class = db->d_co_target;
  a.n_hits = (const unsigned long long*)d_n_hits;
  a.hit_cap = hit_cap;
  a.keys = db->d_co_keys;
  a.counts = db->d_co_counts;
  a.table_slots = db->co_table;
  a.totals = db->d_co_totals;
  a.left = d_left;
  a.stats = db->d_co_stats;
  db->co_timed = db->profiling >= 1;
  const unsigned wgs = max_wgs ? std::min(max_wgs, db->co_max_wgs) : db->co_max_wgs;
  if (int rc = timed_launches(db->co_ev, db->co_timed, st, [&] { db->co_grid = launch_k7(a, wgs, st, db->co_timed ? &db->k7_log : nullptr); })) return rc;
  HIPCHK(hipGetLastError());
  return 0;
}
}  // namespace kmcpg

extern "C" int kmcpg_cooccur_device(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers,
                                    uint32_t n_reads, int32_t final_n, const uint64_t* d_n_hits, uint64_t hit_cap, uint8_t* d_left, uint32_t max_wgs, void* stream) {
  if (!db || !d_read_offs || (n_reads && (!d_qkmers || !d_left)) || (pair_cap && !d_pairs)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (n_reads == 0xffffffffu) return kmcpg_fail(KMCPG_EINVAL, "too many reads");
  if (int rc = refuse(db)) return rc;
  return cooccur_enqueue(db, d_pairs, d_read_offs, pair_cap, d_qkmers, n_reads, final_n, d_n_hits, hit_cap, d_left, max_wgs, (hipStream_t)stream);
}

extern "C" int kmcpg_cooccur_read(kmcpg_db* db, kmcpg_cooccur_pair* out_pairs, uint64_t cap, uint64_t* n_pairs, kmcpg_cooccur_totals* totals) {
  if (!db || !n_pairs || (cap && !out_pairs)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  *n_pairs = 0;
  std::lock_guard<std::mutex> g(db->mu);
  if (!db->cooccur_on()) return kmcpg_fail(KMCPG_EINVAL, "the stage is off: call kmcpg_set_cooccur first");
  std::vector<unsigned long long> keys, counts;
  unsigned long long dev[K7_TOTALS] = {};
  if (db->opts.device >= 0 && db->d_co_keys) {
    HIPCHK(hipSetDevice(db->opts.device));
    HIPCHK(hipDeviceSynchronize());
    keys.resize(db->co_table);
    counts.resize(db->co_table);
    HIPCHK(hipMemcpy(keys.data(), db->d_co_keys, keys.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(counts.data(), db->d_co_counts, counts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dev, db->d_co_totals, sizeof dev, hipMemcpyDeviceToHost));
  }
  std::lock_guard<std::mutex> gh(db->co_mu);
  if (db->co_tainted)
    return kmcpg_fail(KMCPG_EDEVICE, "shared reads of reference pairs: a batch failed after its reads had been counted — the table may hold reads twice; call kmcpg_cooccur_reset and search again");
  // the device's slots with a count (a key without one was reserved by a read that was then LEFT) and the host map, by key: the key's
  // order is (class_a, class_b)'s
  std::vector<std::pair<uint64_t, uint64_t>> all;
  uint64_t n_keys = 0;
  for (size_t i = 0; i < keys.size(); i++) {
    if (keys[i] != COOCCUR_EMPTY) n_keys++;
    if (keys[i] != COOCCUR_EMPTY && counts[i]) all.emplace_back(keys[i], counts[i]);
  }
  for (const auto& kv : db->h_co_pairs) all.emplace_back(kv.first, kv.second);
  std::sort(all.begin(), all.end());
  size_t n = 0;
  for (size_t i = 0; i < all.size(); i++) {
    if (n && all[n - 1].first == all[i].first) all[n - 1].second += all[i].second;
    else all[n++] = all[i];
  }
  *n_pairs = n;
  for (size_t i = 0; i < n && i < cap; i++) out_pairs[i] = kmcpg_cooccur_pair{cooccur_key_a(all[i].first), cooccur_key_b(all[i].first), all[i].second};
  if (totals) {
    memset(totals, 0, sizeof *totals);
    totals->multi_reads = dev[K7_T_MULTI] + db->h_co_multi;
    totals->device_adds = dev[K7_T_PAIRS];
    totals->host_adds = db->h_co_adds;
    totals->left_full = dev[K7_T_LEFT_FULL];
    totals->host_reads = db->h_co_multi;
    totals->skipped_launches = dev[K7_T_SKIPPED];
    totals->table_slots = db->co_table;
    totals->keys = n_keys;
  }
  return 0;
}

extern "C" int kmcpg_cooccur_reset(kmcpg_db* db) {
  if (!db) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  if (!db->cooccur_on()) return kmcpg_fail(KMCPG_EINVAL, "the stage is off: call kmcpg_set_cooccur first");
  if (db->opts.device >= 0 && db->d_co_keys) {
    HIPCHK(hipSetDevice(db->opts.device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemset(db->d_co_keys, 0, (size_t)db->co_table * sizeof(unsigned long long)));
    HIPCHK(hipMemset(db->d_co_counts, 0, (size_t)db->co_table * sizeof(unsigned long long)));
    HIPCHK(hipMemset(db->d_co_totals, 0, K7_TOTALS * sizeof(unsigned long long)));
  }
  std::lock_guard<std::mutex> gh(db->co_mu);
  db->h_co_pairs.clear();
  db->h_co_multi = db->h_co_adds = 0;
  db->co_tainted = false;
  return 0;
}

extern "C" int kmcpg_last_cooccur(kmcpg_db* db, kmcpg_cooccur_stats* out, kmcpg_k4_launch* launches, uint32_t cap, uint32_t* n_launches) {
  if (!db || !out || !n_launches || (cap && !launches)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  memset(out, 0, sizeof *out);
  out->k7_ms = -1;
  *n_launches = 0;
  std::lock_guard<std::mutex> g(db->mu);
  if (!db->co_ran || db->opts.device < 0 || !db->d_co_stats) return 0;
  KMCPG_USE_DEVICE(db);
  HIPCHK(hipDeviceSynchronize());
  unsigned long long s[K7_STATS] = {};
  HIPCHK(hipMemcpy(s, db->d_co_stats, sizeof s, hipMemcpyDeviceToHost));
  out->empty = s[K7_EMPTY];
  out->single = s[K7_SINGLE];
  out->wave = s[K7_WAVE];
  out->left = s[K7_LEFT];
  out->left_full = s[K7_LEFT_FULL];
  out->pairs = s[K7_PAIRS];
  out->lds_adds = s[K7_LDS_ADDS];
  out->global_adds = s[K7_GLOBAL_ADDS];
  out->spilled_adds = s[K7_SPILLED];
  out->claimed = s[K7_CLAIMED];
  out->skipped = s[K7_SKIPPED];
  out->bad_segments = s[K7_BAD];
  out->grid = db->co_grid;
  out->slots = db->co_slots;
  timed_launches_report(db, db->co_ev, db->co_timed, db->k7_log, &out->k7_ms, launches, cap, n_launches);
  return 0;
}
