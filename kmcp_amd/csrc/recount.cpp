// recount.cpp — the host side of K8 (k8_recount.hip): the class tables, the counters and the read log on the handle, k8_log alone, the
// replay of both logs (k8_replay on the device's, recount_rule.hpp on the host's), the read-out, the witness.  What fills the host log
// (the reads the device LEFT) is beside the other users of the match rule, in finalize.cpp (left_reads_host, the one walk of all the counting
// stages, and counting_host_result).
#include <cstring>

#include "engine.hpp"
#include "k3_set_order.hpp"
#include "kernels.hpp"
#include "recount_rule.hpp"

using namespace kmcpg;

static_assert(sizeof(kmcpg_recount_class) == sizeof(RecountClass) && offsetof(kmcpg_recount_class, reads) == offsetof(RecountClass, reads) &&
                  offsetof(kmcpg_recount_class, ureads) == offsetof(RecountClass, ureads) && offsetof(kmcpg_recount_class, kept) == offsetof(RecountClass, kept),
              "kmcpg_recount_class is RecountClass");
static_assert(sizeof(kmcpg_recount_col) == RECOUNT_WORDS * sizeof(uint64_t), "four counters per column");

namespace {

// the handles K6 refuses (refstats.cpp), for the same reason
int refuse(const kmcpg_db* db) { return refuse_handle(db, "recounts with ambiguity correction", "a query's targets need its matches from every block"); }

// KMCPG_RECOUNT_SLOTS: a power of two up to K8_MAX_SLOTS, 0 = no LDS table; false: neither
bool slots_from_env(uint32_t* slots) {
  *slots = K8_DEFAULT_SLOTS;
  const char* e = getenv("KMCPG_RECOUNT_SLOTS");
  if (!e) return true;
  char* end = nullptr;
  const long v = strtol(e, &end, 10);
  if (end == e || *end || v < 0 || v > (long)K8_MAX_SLOTS || (v & (v - 1))) return false;
  *slots = (uint32_t)v;
  return true;
}

void free_device(kmcpg_db* db) {
  for (void* q : {(void*)db->d_rc_target, (void*)db->d_rc_species, (void*)db->d_rc_counters, (void*)db->d_rc_replay, (void*)db->d_rc_log, (void*)db->d_rc_words})
    if (q) (void)hipFree(q);
  db->d_rc_target = db->d_rc_species = nullptr;
  db->d_rc_counters = db->d_rc_replay = db->d_rc_log = db->d_rc_words = nullptr;
  em_release(db);
}

// d_rc_words (engine.hpp: RC_COMMIT .. RC_WORDS)
unsigned long long* totals_of(kmcpg_db* db) { return db->d_rc_words + RC_TOTALS; }
unsigned long long* stats_of(kmcpg_db* db) { return db->d_rc_words + RC_STATS; }
unsigned long long* rstats_of(kmcpg_db* db) { return db->d_rc_words + RC_RSTATS; }

const char* const kOff = "the stage is off: call kmcpg_set_recount first";

}  // namespace

extern "C" int kmcpg_set_recount(kmcpg_db* db, const uint32_t* target_class, const uint32_t* species_class, uint32_t n_cols, double hic_min_qcov, uint64_t log_bytes) {
  if (!db) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  const bool off = !target_class && !species_class && n_cols == 0;
  uint32_t slots = 0;
  if (!off) {
    if (int rc = refuse(db)) return rc;
    KMCPG_NO_FILES_ONLY(db);
    if (!target_class) return kmcpg_fail(KMCPG_EINVAL, "target_class is needed");
    if (n_cols != db->col_meta.size()) return kmcpg_fail(KMCPG_EINVAL, "n_cols = %u, the handle has %zu columns", n_cols, db->col_meta.size());
    if (const char* e = getenv("KMCPG_RECOUNT_LOG_BYTES")) {  // the log's size whatever the caller asks for (tests: a log that fills up)
      char* end = nullptr;
      const unsigned long long v = strtoull(e, &end, 10);
      if (end == e || *end || v == 0) return kmcpg_fail(KMCPG_EINVAL, "KMCPG_RECOUNT_LOG_BYTES = %s, must be a number of bytes", e);
      log_bytes = v;
    }
    if (log_bytes == 0) log_bytes = K8_DEFAULT_LOG_BYTES;
    if (log_bytes < K8_MIN_LOG_BYTES || log_bytes > K8_MAX_LOG_BYTES)
      return kmcpg_fail(KMCPG_EINVAL, "log_bytes = %llu, must lie in [%llu, %llu] (0: the default, %llu)", (unsigned long long)log_bytes, (unsigned long long)K8_MIN_LOG_BYTES,
                        (unsigned long long)K8_MAX_LOG_BYTES, (unsigned long long)K8_DEFAULT_LOG_BYTES);
    if (!slots_from_env(&slots)) return kmcpg_fail(KMCPG_EINVAL, "KMCPG_RECOUNT_SLOTS = %s, must be a power of two up to %u, or 0", getenv("KMCPG_RECOUNT_SLOTS"), K8_MAX_SLOTS);
  }
  std::lock_guard<std::mutex> g(db->mu);
  const bool dev = db->opts.device >= 0;
  if (dev) {
    HIPCHK(hipSetDevice(db->opts.device));
    HIPCHK(hipDeviceSynchronize());  // batches in flight still read the class table and write the log that go
  }
  free_device(db);
  std::lock_guard<std::mutex> gh(db->rc_mu);
  db->h_rc_target.clear();
  db->h_rc_species.clear();
  db->h_rc_log.clear();
  db->h_rc_index.clear();
  db->h_rc_replay.clear();
  db->rc_kept.clear();
  db->rc_tainted = db->rc_ran = db->rc_replayed = false;
  db->rc_log_cap = 0;
  db->k8_log.clear();
  db->k8_rlog.clear();
  if (off || n_cols == 0) return 0;
  db->h_rc_target.assign(target_class, target_class + n_cols);
  if (species_class) db->h_rc_species.assign(species_class, species_class + n_cols);
  db->rc_hic = hic_min_qcov;
  db->rc_slots = slots;
  db->rc_log_cap = log_bytes / sizeof(unsigned long long);
  if (dev) {
    const size_t bytes = (size_t)n_cols * sizeof(uint32_t), cbytes = (size_t)n_cols * RECOUNT_WORDS * sizeof(unsigned long long),
                 lbytes = (size_t)db->rc_log_cap * sizeof(unsigned long long);
    bool ok = hipMalloc((void**)&db->d_rc_target, bytes) == hipSuccess && (!species_class || hipMalloc((void**)&db->d_rc_species, bytes) == hipSuccess) &&
              hipMalloc((void**)&db->d_rc_counters, cbytes) == hipSuccess && hipMalloc((void**)&db->d_rc_replay, cbytes) == hipSuccess &&
              hipMalloc((void**)&db->d_rc_log, lbytes) == hipSuccess && hipMalloc((void**)&db->d_rc_words, RC_WORDS * sizeof(unsigned long long)) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      free_device(db);
      db->h_rc_target.clear();  // the stage stays off
      db->h_rc_species.clear();
      return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc of the read log (%llu bytes) failed", (unsigned long long)log_bytes);
    }
    HIPCHK(hipMemcpy(db->d_rc_target, target_class, bytes, hipMemcpyHostToDevice));
    if (species_class) HIPCHK(hipMemcpy(db->d_rc_species, species_class, bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(db->d_rc_counters, 0, cbytes));
    HIPCHK(hipMemset(db->d_rc_replay, 0, cbytes));
    HIPCHK(hipMemset(db->d_rc_words, 0, RC_WORDS * sizeof(unsigned long long)));
    // persistent workgroups: two per CU, as K6 (refstats.cpp)
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, db->opts.device));
    db->rc_max_wgs = (unsigned)std::max(1, prop.multiProcessorCount) * 2;
    if (const char* e = getenv("KMCPG_RECOUNT_WGS")) db->rc_max_wgs = (unsigned)std::max(1, atoi(e));
  }
  return 0;
}

namespace kmcpg {
int recount_enqueue(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers, const int32_t* d_qlen,
                    uint32_t n_reads, int32_t final_n, const uint64_t* d_n_hits, uint64_t hit_cap, uint8_t* d_left, unsigned max_wgs, hipStream_t st) {
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  if (!db->recount_on() || !db->d_rc_target) return kmcpg_fail(KMCPG_EINVAL, "%s", kOff);
  HIPCHK(hipMemsetAsync(stats_of(db), 0, K8_STATS * sizeof(unsigned long long), st));
  db->k8_log.clear();
  db->rc_ran = true;
  db->rc_grid = 0;
  db->rc_timed = false;
  if (n_reads == 0) return 0;
  K8LogArgs a{};
  a.pairs = d_pairs;
  a.offs = d_read_offs;
  a.pair_cap = pair_cap;
  a.nk = d_qkmers;
  a.qlen = d_qlen;
  a.n_reads = n_reads;
  a.n_cols = (uint32_t)db->h_rc_target.size();
  a.final_n = final_n;
  a.slots = db->rc_slots;
  a.target_class = db->d_rc_target;
  a.hic_min_qcov = db->rc_hic;
  a.n_hits = (const unsigned long long*)d_n_hits;
  a.hit_cap = hit_cap;
  a.counters = db->d_rc_counters;
  a.log = db->d_rc_log;
  a.log_cap = db->rc_log_cap;
  a.log_state = db->d_rc_words;
  a.log_commit = db->d_rc_words + RC_COMMIT;
  a.totals = totals_of(db);
  a.left = d_left;
  a.stats = stats_of(db);
  db->rc_timed = db->profiling >= 1;
  const unsigned wgs = max_wgs ? std::min(max_wgs, db->rc_max_wgs) : db->rc_max_wgs;
  if (int rc = timed_launches(db->rc_ev, db->rc_timed, st, [&] { db->rc_grid = launch_k8_log(a, wgs, st, db->rc_timed ? &db->k8_log : nullptr); })) return rc;
  HIPCHK(hipGetLastError());
  return 0;
}
}  // namespace kmcpg

extern "C" int kmcpg_recount_log_device(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers,
                                        const int32_t* d_qlen, uint32_t n_reads, int32_t final_n, const uint64_t* d_n_hits, uint64_t hit_cap, uint8_t* d_left,
                                        uint32_t max_wgs, void* stream) {
  if (!db || !d_read_offs || (n_reads && (!d_qkmers || !d_qlen || !d_left)) || (pair_cap && !d_pairs)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (n_reads == 0xffffffffu) return kmcpg_fail(KMCPG_EINVAL, "too many reads");
  if (int rc = refuse(db)) return rc;
  return recount_enqueue(db, d_pairs, d_read_offs, pair_cap, d_qkmers, d_qlen, n_reads, final_n, d_n_hits, hit_cap, d_left, max_wgs, (hipStream_t)stream);
}

namespace {
// the host log's reads by the rule of recount_rule.hpp -> db->h_rc_replay; totals: recounted / unique / corrected
void replay_host(kmcpg_db* db, const RecountClass* classes, uint32_t n_classes, const std::vector<unsigned long long>& keys, const std::vector<unsigned long long>& counts,
                 const RecountParams& p, uint64_t* totals) {
  const bool species = !db->h_rc_species.empty();
  const size_t n_cols = db->h_rc_target.size();
  db->h_rc_replay.assign(n_cols * RECOUNT_WORDS, 0);
  std::vector<RecountRow> rows;
  const auto shared = [&](uint32_t a, uint32_t b) -> uint64_t {
    const unsigned long long key = cooccur_key(a, b);
    const auto it = std::lower_bound(keys.begin(), keys.end(), key);
    return it != keys.end() && *it == key ? counts[(size_t)(it - keys.begin())] : 0;
  };
  for (const uint64_t at : db->h_rc_index) {
    const uint64_t w0 = db->h_rc_log[at], qlen = db->h_rc_log[at + 1];
    const uint32_t m = (uint32_t)w0;
    const int32_t qk = (int32_t)(w0 >> 32);
    rows.clear();
    for (uint32_t i = 0; i < m; i++) {
      const uint64_t pw = db->h_rc_log[at + 2 + i];
      const uint32_t col = (uint32_t)pw, cls = col < n_cols ? db->h_rc_target[col] : 0xffffffffu;
      if (cls >= n_classes || !classes[cls].kept) continue;  // rows of targets that stage 1 dropped are skipped before anything else
      rows.push_back(RecountRow{cls, species ? db->h_rc_species[col] : 0u, col, printed_qcov((uint32_t)(pw >> 32), qk), qlen});
    }
    if (rows.empty()) continue;
    bool lost = false;
    const size_t ns = recount_query(rows.data(), rows.size(), classes, p, shared, [&](uint64_t col, int w, uint64_t n) { db->h_rc_replay[col * RECOUNT_WORDS + w] += n; }, &lost);
    totals[0]++;
    if (ns == 1) totals[1]++;
    if (lost) totals[2]++;
  }
}
}  // namespace

extern "C" int kmcpg_recount_run(kmcpg_db* db, const kmcpg_recount_class* classes, uint32_t n_classes, const kmcpg_cooccur_pair* pairs, uint64_t n_pairs,
                                 const kmcpg_recount_params* params) {
  if (!db || !params || (n_classes && !classes) || (n_pairs && !pairs)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  if (!db->recount_on()) return kmcpg_fail(KMCPG_EINVAL, "%s", kOff);
  std::vector<unsigned long long> keys(n_pairs), counts(n_pairs);
  for (uint64_t i = 0; i < n_pairs; i++) {
    if (pairs[i].class_a >= pairs[i].class_b) return kmcpg_fail(KMCPG_EINVAL, "pair %llu: class_a must be below class_b", (unsigned long long)i);
    keys[i] = cooccur_key(pairs[i].class_a, pairs[i].class_b), counts[i] = pairs[i].reads;
    if (i && keys[i] <= keys[i - 1]) return kmcpg_fail(KMCPG_EINVAL, "pair %llu: the pairs must be sorted by (class_a, class_b), each once", (unsigned long long)i);
  }
  const RecountClass* cls = (const RecountClass*)classes;
  RecountParams p;
  p.one_minus_d = params->one_minus_d, p.r_err = params->r_err, p.hic_min_qcov = db->rc_hic;
  p.no_amb_corr = params->no_amb_corr != 0, p.level_species = params->level_species != 0;
  const size_t n_cols = db->h_rc_target.size();
  uint64_t dev_replayed = 0;
  db->rc_replay_grid = 0;
  db->rc_rtimed = false;
  db->k8_rlog.clear();
  if (db->opts.device >= 0 && db->d_rc_log) {
    HIPCHK(hipSetDevice(db->opts.device));
    HIPCHK(hipDeviceSynchronize());
    {
      std::lock_guard<std::mutex> gh(db->rc_mu);
      if (db->rc_tainted)
        return kmcpg_fail(KMCPG_EDEVICE, "recount with ambiguity correction: a batch failed after its reads had been logged — the log may hold reads twice; call kmcpg_recount_reset and search again");
    }
    unsigned long long state = 0;
    HIPCHK(hipMemcpy(&state, db->d_rc_words + RC_COMMIT, sizeof state, hipMemcpyDeviceToHost));
    dev_replayed = state >> K8_STATE_WORD_BITS;
    HIPCHK(hipMemset(db->d_rc_replay, 0, n_cols * RECOUNT_WORDS * sizeof(unsigned long long)));
    HIPCHK(hipMemset(rstats_of(db), 0, K8_R_STATS * sizeof(unsigned long long)));
    if (dev_replayed) {
      RecountClass* d_classes = nullptr;
      unsigned long long *d_keys = nullptr, *d_counts = nullptr;
      const size_t cb = std::max<size_t>(1, n_classes) * sizeof(RecountClass), kb = std::max<size_t>(1, n_pairs) * sizeof(unsigned long long);
      const bool ok = hipMalloc((void**)&d_classes, cb) == hipSuccess && hipMalloc((void**)&d_keys, kb) == hipSuccess && hipMalloc((void**)&d_counts, kb) == hipSuccess;
      int rc = 0;
      if (!ok) {
        (void)hipGetLastError();
        rc = kmcpg_fail(KMCPG_ENOMEM, "hipMalloc of the replay's inputs failed");
      }
      const auto up = [&](void* d, const void* h, size_t n) { return n == 0 || hipMemcpy(d, h, n, hipMemcpyHostToDevice) == hipSuccess; };
      if (!rc && !(up(d_classes, cls, (size_t)n_classes * sizeof(RecountClass)) && up(d_keys, keys.data(), n_pairs * sizeof(unsigned long long)) &&
                   up(d_counts, counts.data(), n_pairs * sizeof(unsigned long long))))
        rc = kmcpg_fail(KMCPG_EDEVICE, "hipMemcpy of the replay's inputs failed");
      if (!rc) {
        K8ReplayArgs a{};
        a.log = db->d_rc_log;
        a.log_cap = db->rc_log_cap;
        a.n_logged = dev_replayed;
        a.n_cols = (uint32_t)n_cols;
        a.n_classes = n_classes;
        a.slots = db->rc_slots;
        a.target_class = db->d_rc_target;
        a.species_class = db->d_rc_species;
        a.classes = d_classes;
        a.keys = d_keys;
        a.counts = d_counts;
        a.n_pairs = n_pairs;
        a.one_minus_d = p.one_minus_d, a.r_err = p.r_err, a.hic_min_qcov = p.hic_min_qcov;
        a.no_amb_corr = p.no_amb_corr, a.level_species = p.level_species;
        a.counters = db->d_rc_replay;
        a.stats = rstats_of(db);
        db->rc_rtimed = db->profiling >= 1;
        rc = timed_launches(db->rc_rev, db->rc_rtimed, nullptr, [&] { db->rc_replay_grid = launch_k8_replay(a, db->rc_max_wgs, nullptr, db->rc_rtimed ? &db->k8_rlog : nullptr); });
        if (!rc && hipGetLastError() != hipSuccess) rc = kmcpg_fail(KMCPG_EDEVICE, "the launch of k8_replay failed");
        if (!rc && hipDeviceSynchronize() != hipSuccess) rc = kmcpg_fail(KMCPG_EDEVICE, "k8_replay failed");
      }
      for (void* q : {(void*)d_classes, (void*)d_keys, (void*)d_counts})
        if (q) (void)hipFree(q);
      if (rc) return rc;
    }
  }
  std::lock_guard<std::mutex> gh(db->rc_mu);
  if (db->rc_tainted)
    return kmcpg_fail(KMCPG_EDEVICE, "recount with ambiguity correction: a batch failed after its reads had been logged — the log may hold reads twice; call kmcpg_recount_reset and search again");
  uint64_t host_totals[3] = {};
  replay_host(db, cls, n_classes, keys, counts, p, host_totals);
  db->rc_kept.assign(n_cols, 0);
  for (size_t c = 0; c < n_cols; c++) {
    const uint32_t t = db->h_rc_target[c];
    db->rc_kept[c] = t < n_classes && cls[t].kept ? 1 : 0;
  }
  for (int i = 0; i < 3; i++) db->rc_run_totals[i] = host_totals[i];
  db->rc_run_totals[3] = dev_replayed;
  db->rc_replayed = true;
  return 0;
}

extern "C" int kmcpg_recount_read(kmcpg_db* db, kmcpg_recount_col* out_cols, uint32_t n_cols, kmcpg_recount_totals* totals) {
  if (!db || (n_cols && !out_cols)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  if (!db->recount_on()) return kmcpg_fail(KMCPG_EINVAL, "%s", kOff);
  if (n_cols != db->h_rc_target.size()) return kmcpg_fail(KMCPG_EINVAL, "n_cols = %u, the stage has %zu columns", n_cols, db->h_rc_target.size());
  if (!db->rc_replayed) return kmcpg_fail(KMCPG_EINVAL, "nothing was replayed yet: call kmcpg_recount_run first");
  const size_t words = (size_t)n_cols * RECOUNT_WORDS;
  std::vector<unsigned long long> single(words, 0), replay(words, 0);
  unsigned long long w[RC_WORDS] = {};
  if (db->opts.device >= 0 && db->d_rc_counters) {
    HIPCHK(hipSetDevice(db->opts.device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(single.data(), db->d_rc_counters, words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(replay.data(), db->d_rc_replay, words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(w, db->d_rc_words, sizeof w, hipMemcpyDeviceToHost));
  }
  std::lock_guard<std::mutex> gh(db->rc_mu);
  if (db->rc_tainted)
    return kmcpg_fail(KMCPG_EDEVICE, "recount with ambiguity correction: a batch failed after its reads had been logged — the log may hold reads twice; call kmcpg_recount_reset and search again");
  uint64_t single_units = 0;  // every single-target read adds UNIT to uniq: the reads of the kept classes
  uint64_t* out = (uint64_t*)out_cols;
  for (size_t c = 0; c < n_cols; c++)
    for (int j = 0; j < RECOUNT_WORDS; j++) {
      const size_t i = c * RECOUNT_WORDS + (size_t)j;
      const uint64_t s = db->rc_kept[c] ? single[i] : 0;  // a dropped reference's single-target reads touch no other reference: ignored here
      if (j == RECOUNT_UNIQ) single_units += s;
      out[i] = s + replay[i] + db->h_rc_replay[i];
    }
  if (totals) {
    memset(totals, 0, sizeof *totals);
    const unsigned long long* rs = w + RC_RSTATS;
    const uint64_t singles = single_units / RECOUNT_UNIT;
    totals->single_reads = singles;
    totals->recounted_reads = singles + rs[K8_R_RECOUNTED] + db->rc_run_totals[0];
    totals->unique_reads = singles + rs[K8_R_UNIQUE] + db->rc_run_totals[1];
    totals->corrected_reads = rs[K8_R_CORRECTED] + db->rc_run_totals[2];
    totals->host_reads = db->h_rc_index.size();
    totals->replayed_reads = rs[K8_R_READS] + totals->host_reads;
    totals->left_full = w[RC_TOTALS + K8_T_LEFT_FULL];
    totals->skipped_launches = w[RC_TOTALS + K8_T_SKIPPED];
    totals->log_bytes = db->rc_log_cap * sizeof(unsigned long long);
    totals->logged_reads = w[RC_COMMIT] >> K8_STATE_WORD_BITS;
    totals->log_bytes_used = ((w[RC_COMMIT] & ((1ull << K8_STATE_WORD_BITS) - 1)) + totals->logged_reads) * sizeof(unsigned long long);
  }
  return 0;
}

extern "C" int kmcpg_recount_reset(kmcpg_db* db) {
  if (!db) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  if (!db->recount_on()) return kmcpg_fail(KMCPG_EINVAL, "%s", kOff);
  if (db->opts.device >= 0 && db->d_rc_counters) {
    HIPCHK(hipSetDevice(db->opts.device));
    HIPCHK(hipDeviceSynchronize());
    const size_t cbytes = db->h_rc_target.size() * RECOUNT_WORDS * sizeof(unsigned long long);
    HIPCHK(hipMemset(db->d_rc_counters, 0, cbytes));
    HIPCHK(hipMemset(db->d_rc_replay, 0, cbytes));
    HIPCHK(hipMemset(db->d_rc_words, 0, RC_STATS * sizeof(unsigned long long)));  // (the log itself needs no clearing: its state word says it is empty)
  }
  std::lock_guard<std::mutex> gh(db->rc_mu);
  db->h_rc_log.clear();
  db->h_rc_index.clear();
  db->h_rc_replay.clear();
  db->rc_kept.clear();
  db->rc_tainted = db->rc_replayed = false;
  db->em_ran = false;  // (a pass over the logs that went)
  return 0;
}

extern "C" int kmcpg_last_recount(kmcpg_db* db, kmcpg_recount_stats* out, kmcpg_k4_launch* launches, uint32_t cap, uint32_t* n_launches) {
  if (!db || !out || !n_launches || (cap && !launches)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  memset(out, 0, sizeof *out);
  out->log_ms = out->replay_ms = -1;
  *n_launches = 0;
  std::lock_guard<std::mutex> g(db->mu);
  if (db->opts.device < 0 || !db->d_rc_words) return 0;
  KMCPG_USE_DEVICE(db);
  HIPCHK(hipDeviceSynchronize());
  unsigned long long w[RC_WORDS] = {};
  HIPCHK(hipMemcpy(w, db->d_rc_words, sizeof w, hipMemcpyDeviceToHost));
  const unsigned long long *s = w + RC_STATS, *r = w + RC_RSTATS;
  if (db->rc_ran) {
    out->empty = s[K8_EMPTY], out->single = s[K8_SINGLE], out->logged = s[K8_LOGGED], out->left = s[K8_LEFT], out->left_full = s[K8_LEFT_FULL];
    out->lds_adds = s[K8_LDS_ADDS], out->global_adds = s[K8_GLOBAL_ADDS], out->spilled_adds = s[K8_SPILLED];
    out->skipped = s[K8_SKIPPED], out->bad_segments = s[K8_BAD];
    out->grid = db->rc_grid;
  }
  out->log_bytes_used = ((w[RC_COMMIT] & ((1ull << K8_STATE_WORD_BITS) - 1)) + (w[RC_COMMIT] >> K8_STATE_WORD_BITS)) * sizeof(unsigned long long);
  out->slots = db->rc_slots;
  if (db->rc_replayed) {
    out->replay_reads = r[K8_R_READS], out->replay_recounted = r[K8_R_RECOUNTED], out->replay_corrected = r[K8_R_CORRECTED], out->replay_unique = r[K8_R_UNIQUE];
    out->replay_lookups = r[K8_R_LOOKUPS];
    out->replay_lds_adds = r[K8_R_LDS_ADDS], out->replay_global_adds = r[K8_R_GLOBAL_ADDS], out->replay_spilled_adds = r[K8_R_SPILLED];
    out->replay_grid = db->rc_replay_grid;
  }
  // the launch records: k8_log's, then the replay's
  uint32_t n_log = 0, n_rep = 0;
  timed_launches_report(db, db->rc_ev, db->rc_ran && db->rc_timed, db->k8_log, &out->log_ms, launches, cap, &n_log);
  const uint32_t used = std::min(cap, n_log);
  timed_launches_report(db, db->rc_rev, db->rc_replayed && db->rc_rtimed, db->k8_rlog, &out->replay_ms, launches ? launches + used : nullptr, cap - used, &n_rep);
  *n_launches = n_log + n_rep;
  return 0;
}
