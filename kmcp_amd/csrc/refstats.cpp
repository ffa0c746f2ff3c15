// refstats.cpp — the host side of K6 (k6_refstats.hip): the tables and counters on the handle, the stage alone, the sum of the device's and
// the host half's counters, the witness.  The host half itself (the reads the device LEFT) is beside the other users of the match rule, in
// finalize.cpp (left_reads_host, the one walk of all the counting stages, and counting_host_result).
#include <cstring>

#include "engine.hpp"
#include "kernels.hpp"
#include "refstats_rule.hpp"

using namespace kmcpg;

static_assert(sizeof(kmcpg_col_stats) == REFSTATS_WORDS * sizeof(uint64_t), "a column's four counters, in the order of refstats_rule.hpp");
static_assert(offsetof(kmcpg_col_stats, rows) == REFSTATS_ROWS * 8 && offsetof(kmcpg_col_stats, firsts) == REFSTATS_FIRSTS * 8 &&
                  offsetof(kmcpg_col_stats, ureads) == REFSTATS_UREADS * 8 && offsetof(kmcpg_col_stats, hic_ureads) == REFSTATS_HIC * 8,
              "a column's four counters, in the order of refstats_rule.hpp");

namespace {

// the handles K4 refuses (specific.cpp), for the same reason
int refuse(const kmcpg_db* db) { return refuse_handle(db, "reference statistics", "a query's counts need its matches from every block"); }

size_t counter_words(const kmcpg_db* db) { return db->h_rs_target.size() * REFSTATS_WORDS + 3; }  // ... then matched and unique reads and the skipped launches

// KMCPG_REFSTATS_SLOTS: rounded down to a power of two, at most K6_MAX_SLOTS; 0 = no table
uint32_t slots_from_env() {
  const char* e = getenv("KMCPG_REFSTATS_SLOTS");
  if (!e) return K6_DEFAULT_SLOTS;
  const long v = std::max(0l, std::min<long>(atol(e), K6_MAX_SLOTS));
  uint32_t s = 0;
  for (uint32_t b = 1; b <= (uint32_t)v; b <<= 1) s = b;
  return s;
}

}  // namespace

extern "C" int kmcpg_set_refstats(kmcpg_db* db, const uint32_t* target_class, const uint32_t* species_class, uint32_t n_cols, double hic_min_qcov) {
  if (!db) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  const bool off = !target_class && !species_class && n_cols == 0;
  if (!off) {
    if (int rc = refuse(db)) return rc;
    KMCPG_NO_FILES_ONLY(db);
    if (!target_class) return kmcpg_fail(KMCPG_EINVAL, "target_class is needed (species_class alone decides nothing)");
    if (n_cols != db->col_meta.size()) return kmcpg_fail(KMCPG_EINVAL, "n_cols = %u, the handle has %zu columns", n_cols, db->col_meta.size());
    if (!(hic_min_qcov >= 0 && hic_min_qcov <= 1)) return kmcpg_fail(KMCPG_EINVAL, "hic_min_qcov = %g, must lie in [0, 1]", hic_min_qcov);
  }
  std::lock_guard<std::mutex> g(db->mu);
  const bool dev = db->opts.device >= 0;
  if (dev) {
    HIPCHK(hipSetDevice(db->opts.device));
    HIPCHK(hipDeviceSynchronize());  // batches in flight still read the tables and add to the counters that go
  }
  if (db->d_rs_target) (void)hipFree(db->d_rs_target);
  if (db->d_rs_species) (void)hipFree(db->d_rs_species);
  if (db->d_rs_counters) (void)hipFree(db->d_rs_counters);
  db->d_rs_target = db->d_rs_species = nullptr;
  db->d_rs_counters = nullptr;
  std::lock_guard<std::mutex> gh(db->rs_mu);
  db->h_rs_target.clear();
  db->h_rs_species.clear();
  db->h_rs_counters.clear();
  db->h_rs_matched = db->h_rs_unique = db->h_rs_reads = 0;
  db->rs_tainted = db->rs_ran = false;
  db->k6_log.clear();
  if (off || n_cols == 0) return 0;
  db->h_rs_target.assign(target_class, target_class + n_cols);
  if (species_class) db->h_rs_species.assign(species_class, species_class + n_cols);
  db->h_rs_counters.assign((size_t)n_cols * REFSTATS_WORDS, 0);
  db->rs_hic = hic_min_qcov;
  db->rs_slots = slots_from_env();
  if (dev) {
    const size_t bytes = (size_t)n_cols * sizeof(uint32_t), cbytes = counter_words(db) * sizeof(unsigned long long);
    bool ok = hipMalloc((void**)&db->d_rs_target, bytes) == hipSuccess && hipMalloc((void**)&db->d_rs_counters, cbytes) == hipSuccess;
    if (ok && species_class) ok = hipMalloc((void**)&db->d_rs_species, bytes) == hipSuccess;
    if (ok && !db->d_rs_stats) ok = hipMalloc((void**)&db->d_rs_stats, K6_STATS * sizeof(unsigned long long)) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      db->h_rs_target.clear();  // the stage stays off
      db->h_rs_species.clear();
      db->h_rs_counters.clear();
      return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc of the reference statistics' tables and counters failed");
    }
    HIPCHK(hipMemcpy(db->d_rs_target, target_class, bytes, hipMemcpyHostToDevice));
    if (species_class) HIPCHK(hipMemcpy(db->d_rs_species, species_class, bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(db->d_rs_counters, 0, cbytes));
    HIPCHK(hipMemset(db->d_rs_stats, 0, K6_STATS * sizeof(unsigned long long)));
    // persistent workgroups: two per CU.  Measured on a batch of 2^20 reads (tools/bench_refstats.py --wgs; profiles/refstats_bench.txt):
    // 1, 2, 4, 8 per CU took 0.30, 0.30, 0.37, 0.50 ms on evenly spread hits and 0.35, 0.31, 0.35, 0.56 ms with half of them on one reference
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, db->opts.device));
    db->rs_max_wgs = (unsigned)std::max(1, prop.multiProcessorCount) * 2;
    if (const char* e = getenv("KMCPG_REFSTATS_WGS")) db->rs_max_wgs = (unsigned)std::max(1, atoi(e));
  }
  return 0;
}

namespace kmcpg {
int refstats_enqueue(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers, uint32_t n_reads,
                     int32_t final_n, const uint64_t* d_n_hits, uint64_t hit_cap, uint8_t* d_left, hipStream_t st) {
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  if (!db->refstats_on() || !db->d_rs_target) return kmcpg_fail(KMCPG_EINVAL, "the stage is off: call kmcpg_set_refstats first");
  HIPCHK(hipMemsetAsync(db->d_rs_stats, 0, K6_STATS * sizeof(unsigned long long), st));
  db->k6_log.clear();
  db->rs_ran = true;
  db->rs_grid = 0;
  db->rs_timed = false;
  if (n_reads == 0) return 0;
  K6Args a{};
  a.pairs = d_pairs;
  a.offs = d_read_offs;
  a.pair_cap = pair_cap;
  a.nk = d_qkmers;
  a.n_reads = n_reads;
  a.n_cols = (uint32_t)db->h_rs_target.size();
  a.final_n = final_n;
  // (a slot's counters are 32 bits wide: a workgroup adds at most once per pair and counter)
  a.slots = pair_cap < (1ull << 32) ? db->rs_slots : 0u;
  a.target_class = db->d_rs_target;
  a.species_class = db->d_rs_species;
  a.hic_min_qcov = db->rs_hic;
  a.n_hits = (const unsigned long long*)d_n_hits;
  a.hit_cap = hit_cap;
  a.counters = db->d_rs_counters;
  a.totals = db->d_rs_counters + (size_t)a.n_cols * REFSTATS_WORDS;
  a.left = d_left;
  a.stats = db->d_rs_stats;
  db->rs_timed = db->profiling >= 1;
  if (int rc = timed_launches(db->rs_ev, db->rs_timed, st, [&] { db->rs_grid = launch_k6(a, db->rs_max_wgs, st, db->rs_timed ? &db->k6_log : nullptr); })) return rc;
  HIPCHK(hipGetLastError());
  return 0;
}
}  // namespace kmcpg

extern "C" int kmcpg_refstats_device(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers,
                                     uint32_t n_reads, int32_t final_n, const uint64_t* d_n_hits, uint64_t hit_cap, uint8_t* d_left, void* stream) {
  if (!db || !d_read_offs || (n_reads && (!d_qkmers || !d_left)) || (pair_cap && !d_pairs)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (n_reads == 0xffffffffu) return kmcpg_fail(KMCPG_EINVAL, "too many reads");
  if (int rc = refuse(db)) return rc;
  return refstats_enqueue(db, d_pairs, d_read_offs, pair_cap, d_qkmers, n_reads, final_n, d_n_hits, hit_cap, d_left, (hipStream_t)stream);
}

extern "C" int kmcpg_refstats_read(kmcpg_db* db, kmcpg_col_stats* out, uint32_t n_cols, kmcpg_refstats_totals* totals) {
  if (!db || (n_cols && !out)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  if (!db->refstats_on()) return kmcpg_fail(KMCPG_EINVAL, "the stage is off: call kmcpg_set_refstats first");
  if (n_cols != db->h_rs_target.size()) return kmcpg_fail(KMCPG_EINVAL, "n_cols = %u, the handle has %zu columns", n_cols, db->h_rs_target.size());
  std::vector<unsigned long long> dev(counter_words(db), 0);
  if (db->opts.device >= 0 && db->d_rs_counters) {
    HIPCHK(hipSetDevice(db->opts.device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(dev.data(), db->d_rs_counters, dev.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  }
  std::lock_guard<std::mutex> gh(db->rs_mu);
  if (db->rs_tainted)
    return kmcpg_fail(KMCPG_EDEVICE, "reference statistics: a batch failed after its reads had been counted — the counters may hold reads twice; call kmcpg_refstats_reset and search again");
  uint64_t* o = (uint64_t*)out;
  for (size_t i = 0; i < (size_t)n_cols * REFSTATS_WORDS; i++) o[i] = dev[i] + db->h_rs_counters[i];
  if (totals) {
    memset(totals, 0, sizeof *totals);
    totals->matched_reads = dev[(size_t)n_cols * REFSTATS_WORDS] + db->h_rs_matched;
    totals->unique_reads = dev[(size_t)n_cols * REFSTATS_WORDS + 1] + db->h_rs_unique;
    totals->host_reads = db->h_rs_reads;
    totals->skipped_launches = dev[(size_t)n_cols * REFSTATS_WORDS + 2];
  }
  return 0;
}

extern "C" int kmcpg_refstats_reset(kmcpg_db* db) {
  if (!db) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  if (!db->refstats_on()) return kmcpg_fail(KMCPG_EINVAL, "the stage is off: call kmcpg_set_refstats first");
  if (db->opts.device >= 0 && db->d_rs_counters) {
    HIPCHK(hipSetDevice(db->opts.device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemset(db->d_rs_counters, 0, counter_words(db) * sizeof(unsigned long long)));
  }
  std::lock_guard<std::mutex> gh(db->rs_mu);
  std::fill(db->h_rs_counters.begin(), db->h_rs_counters.end(), 0);
  db->h_rs_matched = db->h_rs_unique = db->h_rs_reads = 0;
  db->rs_tainted = false;
  return 0;
}

extern "C" int kmcpg_last_refstats(kmcpg_db* db, kmcpg_refstats_stats* out, kmcpg_k4_launch* launches, uint32_t cap, uint32_t* n_launches) {
  if (!db || !out || !n_launches || (cap && !launches)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  memset(out, 0, sizeof *out);
  out->k6_ms = -1;
  *n_launches = 0;
  std::lock_guard<std::mutex> g(db->mu);
  if (!db->rs_ran || db->opts.device < 0 || !db->d_rs_stats) return 0;
  KMCPG_USE_DEVICE(db);
  HIPCHK(hipDeviceSynchronize());
  unsigned long long s[K6_STATS] = {};
  HIPCHK(hipMemcpy(s, db->d_rs_stats, sizeof s, hipMemcpyDeviceToHost));
  out->empty = s[K6_EMPTY];
  out->single = s[K6_SINGLE];
  out->wave = s[K6_WAVE];
  out->left = s[K6_LEFT];
  out->lds_adds = s[K6_LDS_ADDS];
  out->global_adds = s[K6_GLOBAL_ADDS];
  out->spilled_adds = s[K6_SPILLED];
  out->skipped = s[K6_SKIPPED];
  out->bad_segments = s[K6_BAD];
  out->grid = db->rs_grid;
  out->slots = db->rs_slots;
  timed_launches_report(db, db->rs_ev, db->rs_timed, db->k6_log, &out->k6_ms, launches, cap, n_launches);
  return 0;
}
