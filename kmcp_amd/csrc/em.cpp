// em.cpp — the host side of K9 (k9_em.hip): one EM pass over the logs the recount stage keeps (recount.cpp) — k9_em over the device's,
// em_rule.hpp over the host's —, the read-out with the single-target counters, the witness.
#include <cmath>
#include <cstring>

#include "em_rule.hpp"
#include "engine.hpp"
#include "k3_set_order.hpp"
#include "kernels.hpp"

using namespace kmcpg;

static_assert(sizeof(kmcpg_em_col) == 6 * sizeof(uint64_t) && sizeof(kmcpg_em_class) == 16 && offsetof(kmcpg_em_class, coverage) == 8, "the layouts of include/kmcp_gpu.h");
static_assert(sizeof(kmcpg_em_col) == sizeof(EmChunk) && offsetof(kmcpg_em_col, single_bases) == offsetof(EmChunk, single_bases) &&
                  offsetof(kmcpg_em_col, bases_hi) == offsetof(EmChunk, bases_hi),
              "kmcpg_em_col is EmChunk");

namespace {

const char* const kOff = "the recount stage is off: call kmcpg_set_recount first";
const char* const kTainted = "EM pass: a batch failed after its reads had been logged — the log may hold reads twice; call kmcpg_recount_reset and search again";

// KMCPG_EM_SLOTS: a power of two up to K9_MAX_SLOTS, 0 = no LDS table; false: neither
bool slots_from_env(uint32_t* slots) {
  *slots = K9_DEFAULT_SLOTS;
  const char* e = getenv("KMCPG_EM_SLOTS");
  if (!e) return true;
  char* end = nullptr;
  const long v = strtol(e, &end, 10);
  if (end == e || *end || v < 0 || v > (long)K9_MAX_SLOTS || (v & (v - 1))) return false;
  *slots = (uint32_t)v;
  return true;
}

// the host log's reads by the rule of em_rule.hpp -> db->h_em_pass, and those with ONE target in the whole table by K8's single rule ->
// db->h_em_single (what k8_log adds to its counters when it has such a read: the same words whichever half counts it);
// totals: reads with one / several estimated targets
void pass_host(kmcpg_db* db, const kmcpg_em_class* classes, uint32_t n_classes, const std::vector<double>& cov, bool level_species, uint64_t* totals) {
  const bool species = !db->h_rc_species.empty();
  const size_t n_cols = db->h_rc_target.size();
  db->h_em_pass.assign(n_cols * EM_WORDS, 0);
  db->h_em_single.assign(n_cols * RECOUNT_WORDS, 0);
  std::vector<RecountRow> rows;
  for (const uint64_t at : db->h_rc_index) {
    const uint64_t w0 = db->h_rc_log[at], qlen = db->h_rc_log[at + 1];
    const uint32_t m = (uint32_t)w0;
    const int32_t qk = (int32_t)(w0 >> 32);
    rows.clear();
    uint32_t tmin = 0xffffffffu, tmax = 0;
    for (uint32_t i = 0; i < m; i++) {
      const uint64_t pw = db->h_rc_log[at + 2 + i];
      const uint32_t col = (uint32_t)pw, cls = col < n_cols ? db->h_rc_target[col] : 0xffffffffu;
      tmin = std::min(tmin, cls), tmax = std::max(tmax, cls);
      if (cls >= n_classes || !classes[cls].est) continue;  // rows of classes outside the whitelist are skipped before anything else
      rows.push_back(RecountRow{cls, species ? db->h_rc_species[col] : 0u, col, printed_qcov((uint32_t)(pw >> 32), qk), qlen});
    }
    if (rows.empty()) continue;
    if (tmin == tmax) {  // a single-target read: rows.size() == m
      for (uint32_t i = 0; i < m; i++) {
        uint64_t* w = db->h_em_single.data() + rows[i].column * RECOUNT_WORDS;
        const uint64_t u = i == 0 ? RECOUNT_UNIT : 0;
        w[RECOUNT_MATCH] += recount_share(m, i == 0), w[RECOUNT_UNIQ] += u, w[RECOUNT_HIC] += rows[i].qcov >= db->rc_hic ? u : 0;
        w[RECOUNT_BASES] += recount_bases(qlen, 1, m);
      }
      totals[0]++;
      continue;
    }
    const size_t nt = em_query(rows.data(), rows.size(), cov.data(), db->rc_hic, level_species, [&](uint64_t col, int w, uint64_t n) { db->h_em_pass[col * EM_WORDS + w] += n; });
    if (nt == 1) totals[0]++;
    if (nt > 1) totals[1]++;
  }
}

}  // namespace

namespace kmcpg {
void em_release(kmcpg_db* db) {
  for (void* q : {(void*)db->d_em_counters, (void*)db->d_em_words, (void*)db->d_em_classes})
    if (q) (void)hipFree(q);
  db->d_em_counters = db->d_em_words = nullptr;
  db->d_em_classes = nullptr;
  db->em_classes_cap = 0;
  db->h_em_pass.clear();
  db->h_em_single.clear();
  db->em_est.clear();
  db->em_ran = false;
  db->em_grid = 0;
  db->k9_log.clear();
}
}  // namespace kmcpg

extern "C" int kmcpg_em_pass(kmcpg_db* db, const kmcpg_em_class* classes, uint32_t n_classes, uint32_t level_species) {
  if (!db || (n_classes && !classes)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  if (!db->recount_on()) return kmcpg_fail(KMCPG_EINVAL, "%s", kOff);
  std::vector<double> cov(n_classes, 0.0);
  for (uint32_t c = 0; c < n_classes; c++) {
    if (!classes[c].est) continue;
    if (!std::isfinite(classes[c].coverage) || !(classes[c].coverage > 0))
      return kmcpg_fail(KMCPG_EINVAL, "class %u is estimated and its coverage is %g: it must be finite and above 0", c, classes[c].coverage);
    cov[c] = classes[c].coverage;
  }
  uint32_t slots = 0;
  if (!slots_from_env(&slots)) return kmcpg_fail(KMCPG_EINVAL, "KMCPG_EM_SLOTS = %s, must be a power of two up to %u, or 0", getenv("KMCPG_EM_SLOTS"), K9_MAX_SLOTS);
  const size_t n_cols = db->h_rc_target.size();
  uint64_t dev_totals[2] = {};
  db->em_ran = false;  // a pass that fails part-way leaves nothing to read: set again only when both halves are done
  db->em_grid = 0;
  db->em_timed = false;
  db->em_slots = slots;
  db->k9_log.clear();
  if (db->opts.device >= 0 && db->d_rc_log) {
    HIPCHK(hipSetDevice(db->opts.device));
    HIPCHK(hipDeviceSynchronize());
    {
      std::lock_guard<std::mutex> gh(db->rc_mu);
      if (db->rc_tainted) return kmcpg_fail(KMCPG_EDEVICE, "%s", kTainted);
    }
    const size_t cbytes = n_cols * EM_WORDS * sizeof(unsigned long long), wbytes = K9_STATS * sizeof(unsigned long long);
    if (!db->d_em_counters) {
      const bool ok = hipMalloc((void**)&db->d_em_counters, cbytes) == hipSuccess && hipMalloc((void**)&db->d_em_words, wbytes) == hipSuccess;
      if (!ok) {
        (void)hipGetLastError();
        em_release(db);
        return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc of the pass counters (%zu bytes) failed", cbytes);
      }
    }
    if (n_classes > db->em_classes_cap) {
      if (db->d_em_classes) (void)hipFree(db->d_em_classes);
      db->d_em_classes = nullptr, db->em_classes_cap = 0;
      if (hipMalloc((void**)&db->d_em_classes, (size_t)n_classes * sizeof(kmcpg_em_class)) != hipSuccess) {
        (void)hipGetLastError();
        return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc of the pass's classes failed");
      }
      db->em_classes_cap = n_classes;
    }
    unsigned long long state = 0;
    HIPCHK(hipMemcpy(&state, db->d_rc_words + RC_COMMIT, sizeof state, hipMemcpyDeviceToHost));
    const uint64_t n_logged = state >> K8_STATE_WORD_BITS;
    HIPCHK(hipMemset(db->d_em_counters, 0, cbytes));
    HIPCHK(hipMemset(db->d_em_words, 0, wbytes));
    if (n_logged) {
      if (n_classes) HIPCHK(hipMemcpy(db->d_em_classes, classes, (size_t)n_classes * sizeof(kmcpg_em_class), hipMemcpyHostToDevice));
      K9Args a{};
      a.log = db->d_rc_log;
      a.log_cap = db->rc_log_cap;
      a.n_logged = n_logged;
      a.n_cols = (uint32_t)n_cols;
      a.n_classes = n_classes;
      a.slots = slots;
      a.level_species = level_species != 0;
      a.target_class = db->d_rc_target;
      a.species_class = db->d_rc_species;
      a.classes = db->d_em_classes;
      a.hic_min_qcov = db->rc_hic;
      a.counters = db->d_em_counters;
      a.stats = db->d_em_words;
      db->em_timed = db->profiling >= 1;
      if (int rc = timed_launches(db->em_ev, db->em_timed, nullptr, [&] { db->em_grid = launch_k9_em(a, db->rc_max_wgs, nullptr, db->em_timed ? &db->k9_log : nullptr); })) return rc;
      HIPCHK(hipGetLastError());
      HIPCHK(hipDeviceSynchronize());
      unsigned long long w[K9_STATS] = {};
      HIPCHK(hipMemcpy(w, db->d_em_words, sizeof w, hipMemcpyDeviceToHost));
      dev_totals[0] = w[K9_ONE], dev_totals[1] = w[K9_SPLIT];
    }
  }
  std::lock_guard<std::mutex> gh(db->rc_mu);
  if (db->rc_tainted) return kmcpg_fail(KMCPG_EDEVICE, "%s", kTainted);
  uint64_t host_totals[2] = {};
  pass_host(db, classes, n_classes, cov, level_species != 0, host_totals);
  db->em_est.assign(n_cols, 0);
  for (size_t c = 0; c < n_cols; c++) {
    const uint32_t t = db->h_rc_target[c];
    db->em_est[c] = t < n_classes && classes[t].est ? 1 : 0;
  }
  db->em_totals[0] = dev_totals[0], db->em_totals[1] = dev_totals[1], db->em_totals[2] = host_totals[0], db->em_totals[3] = host_totals[1];
  db->em_ran = true;
  return 0;
}

extern "C" int kmcpg_em_read(kmcpg_db* db, kmcpg_em_col* out_cols, uint32_t n_cols, kmcpg_em_totals* totals) {
  if (!db || (n_cols && !out_cols)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  if (!db->recount_on()) return kmcpg_fail(KMCPG_EINVAL, "%s", kOff);
  if (n_cols != db->h_rc_target.size()) return kmcpg_fail(KMCPG_EINVAL, "n_cols = %u, the stage has %zu columns", n_cols, db->h_rc_target.size());
  if (!db->em_ran) return kmcpg_fail(KMCPG_EINVAL, "no pass was run yet: call kmcpg_em_pass first");
  std::vector<unsigned long long> single((size_t)n_cols * RECOUNT_WORDS, 0), pass((size_t)n_cols * EM_WORDS, 0);
  if (db->opts.device >= 0 && db->d_rc_counters && db->d_em_counters) {
    HIPCHK(hipSetDevice(db->opts.device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(single.data(), db->d_rc_counters, single.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pass.data(), db->d_em_counters, pass.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  }
  std::lock_guard<std::mutex> gh(db->rc_mu);
  if (db->rc_tainted) return kmcpg_fail(KMCPG_EDEVICE, "%s", kTainted);
  uint64_t single_units = 0;  // every single-target read adds RECOUNT_UNIT to uniq: the reads of the estimated classes
  for (size_t c = 0; c < n_cols; c++) {
    const unsigned long long* s = single.data() + c * RECOUNT_WORDS;
    const unsigned long long* d = pass.data() + c * EM_WORDS;
    const uint64_t *h = db->h_em_pass.data() + c * EM_WORDS, *hs = db->h_em_single.data() + c * RECOUNT_WORDS;
    const bool est = db->em_est[c] != 0;  // a class outside the whitelist: its single-target reads touch no other reference
    kmcpg_em_col& o = out_cols[c];
    o.match = (((est ? s[RECOUNT_MATCH] : 0) + hs[RECOUNT_MATCH]) << EM_SHIFT) + d[EM_MATCH] + h[EM_MATCH];
    o.uniq = (((est ? s[RECOUNT_UNIQ] : 0) + hs[RECOUNT_UNIQ]) << EM_SHIFT) + d[EM_UNIQ] + h[EM_UNIQ];
    o.hic = (((est ? s[RECOUNT_HIC] : 0) + hs[RECOUNT_HIC]) << EM_SHIFT) + d[EM_HIC] + h[EM_HIC];
    o.single_bases = (est ? s[RECOUNT_BASES] : 0) + hs[RECOUNT_BASES];
    o.bases_lo = d[EM_BASES_LO] + h[EM_BASES_LO];
    o.bases_hi = d[EM_BASES_HI] + h[EM_BASES_HI];
    if (est) single_units += s[RECOUNT_UNIQ];
  }
  if (totals) {
    const uint64_t singles = single_units / RECOUNT_UNIT, *t = db->em_totals;
    totals->unique_reads = singles + t[0] + t[2];
    totals->split_reads = t[1] + t[3];
    totals->assigned_reads = totals->unique_reads + totals->split_reads;
    totals->host_reads = t[2] + t[3];
  }
  return 0;
}

extern "C" int kmcpg_last_em(kmcpg_db* db, kmcpg_em_stats* out, kmcpg_k4_launch* launches, uint32_t cap, uint32_t* n_launches) {
  if (!db || !out || !n_launches || (cap && !launches)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  memset(out, 0, sizeof *out);
  out->em_ms = -1;
  *n_launches = 0;
  std::lock_guard<std::mutex> g(db->mu);
  if (db->opts.device < 0 || !db->d_em_words || !db->em_ran) return 0;
  KMCPG_USE_DEVICE(db);
  HIPCHK(hipDeviceSynchronize());
  unsigned long long w[K9_STATS] = {};
  HIPCHK(hipMemcpy(w, db->d_em_words, sizeof w, hipMemcpyDeviceToHost));
  out->reads = w[K9_READS], out->none = w[K9_NONE], out->one = w[K9_ONE], out->split = w[K9_SPLIT];
  out->lds_adds = w[K9_LDS_ADDS], out->global_adds = w[K9_GLOBAL_ADDS], out->spilled_adds = w[K9_SPILLED];
  out->grid = db->em_grid;
  out->slots = db->em_slots;
  timed_launches_report(db, db->em_ev, db->em_timed, db->k9_log, &out->em_ms, launches, cap, n_launches);
  return 0;
}
