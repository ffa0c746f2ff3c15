// binning.cpp — the host side of K11 (k11_bin.hip): the plan's tables on the handle, the stage alone on device pointers, its witness.
// The rule and the plan are bin_rule.hpp's; what is checked here is what the kernel's climb rests on.
#include <hip/hip_runtime.h>
#include <string.h>

#include <mutex>

#include "bin_rule.hpp"
#include "engine.hpp"
#include "kernels.hpp"

using namespace kmcpg;

static_assert(K11_NONE == KMCPG_BIN_NONE && K11_LEFT == KMCPG_BIN_LEFT && K11_NONE == BIN_NONE && K11_LEFT == BIN_LEFT, "one pair of sentinels");
static_assert(KMCPG_BIN_NO_NODE == BIN_NO_NODE, "one word for a column off the whitelist");

namespace {

// the handles K4 and the counting stages refuse, for the same reason
int refuse(const kmcpg_db* db) { return refuse_handle(db, "taxonomic bins", "a query's bin needs its matches from every block"); }

// What the climb of k11_bin rests on: parent[v] < v (it ends), last[0] = n - 1 (it ends at node 0 at the latest), v <= last[v] <= last[parent[v]]
// (subtrees nest: pre-order), every column names a node or none
int check_plan(const uint32_t* node, uint32_t n_cols, const uint32_t* parent, const uint32_t* last, const uint32_t* taxid, uint32_t n) {
  for (uint32_t v = 0; v < n; v++)  // (a bin that printed as a sentinel would be read as "no line" or "left to the host")
    if (taxid[v] == BIN_NONE || taxid[v] == BIN_LEFT) return kmcpg_fail(KMCPG_EINVAL, "taxid[%u] = %u is one of the two sentinels of a read's bin", v, taxid[v]);
  if (parent[0] != 0 || last[0] != n - 1) return kmcpg_fail(KMCPG_EINVAL, "node 0 must be the root of every node: parent[0] = %u, last[0] = %u of %u nodes", parent[0], last[0], n);
  for (uint32_t v = 1; v < n; v++)
    if (parent[v] >= v || last[v] < v || last[v] > last[parent[v]])
      return kmcpg_fail(KMCPG_EINVAL, "node %u is not numbered in pre-order: parent %u, last %u (its parent's: %u)", v, parent[v], last[v], parent[v] < v ? last[parent[v]] : 0u);
  for (uint32_t c = 0; c < n_cols; c++)
    if (node[c] != BIN_NO_NODE && node[c] >= n) return kmcpg_fail(KMCPG_EINVAL, "node_of_column[%u] = %u, the plan has %u nodes", c, node[c], n);
  return 0;
}

}  // namespace

extern "C" int kmcpg_set_binning(kmcpg_db* db, const uint32_t* node_of_column, uint32_t n_cols, const uint32_t* parent, const uint32_t* last, const uint32_t* taxid,
                                 uint32_t n_nodes) {
  if (!db) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  const bool off = !node_of_column && n_cols == 0;
  if (!off) {
    if (int rc = refuse(db)) return rc;
    KMCPG_NO_FILES_ONLY(db);
    if (n_nodes == 0 || n_nodes >= BIN_LEFT) return kmcpg_fail(KMCPG_EINVAL, "n_nodes = %u: the plan holds at least the virtual root", n_nodes);
    if (!node_of_column || !parent || !last || !taxid) return kmcpg_fail(KMCPG_EINVAL, "null argument");
    if (n_cols != db->col_meta.size()) return kmcpg_fail(KMCPG_EINVAL, "n_cols = %u, the handle has %zu columns", n_cols, db->col_meta.size());
    if (int rc = check_plan(node_of_column, n_cols, parent, last, taxid, n_nodes)) return rc;
  }
  std::lock_guard<std::mutex> g(db->mu);
  const bool dev = db->opts.device >= 0;
  if (dev) {
    HIPCHK(hipSetDevice(db->opts.device));
    HIPCHK(hipDeviceSynchronize());  // batches in flight still read the tables that go
  }
  if (db->d_bin_tables) (void)hipFree(db->d_bin_tables);
  db->d_bin_tables = nullptr;
  db->h_bin_node.clear(), db->h_bin_parent.clear(), db->h_bin_last.clear(), db->h_bin_taxid.clear();
  db->bin_ran = false;
  db->k11_log.clear();
  if (off || n_cols == 0) return 0;
  if (dev) {
    const size_t words = (size_t)n_cols + 3 * (size_t)n_nodes;
    bool ok = hipMalloc((void**)&db->d_bin_tables, words * sizeof(uint32_t)) == hipSuccess;
    if (ok && !db->d_bin_stats) ok = hipMalloc((void**)&db->d_bin_stats, K11_STATS * sizeof(unsigned long long)) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      if (db->d_bin_tables) (void)hipFree(db->d_bin_tables);
      db->d_bin_tables = nullptr;
      return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc of the binning tables failed");
    }
    uint32_t* d = db->d_bin_tables;
    HIPCHK(hipMemcpy(d, node_of_column, (size_t)n_cols * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d + n_cols, parent, (size_t)n_nodes * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d + n_cols + n_nodes, last, (size_t)n_nodes * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d + n_cols + 2 * (size_t)n_nodes, taxid, (size_t)n_nodes * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(db->d_bin_stats, 0, K11_STATS * sizeof(unsigned long long)));
    // persistent workgroups, as K6: two per CU (not measured for K11)
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, db->opts.device));
    db->bin_max_wgs = (unsigned)std::max(1, prop.multiProcessorCount) * 2;
    if (const char* e = getenv("KMCPG_BIN_WGS")) db->bin_max_wgs = (unsigned)std::max(1, atoi(e));
  }
  db->h_bin_node.assign(node_of_column, node_of_column + n_cols);
  db->h_bin_parent.assign(parent, parent + n_nodes);
  db->h_bin_last.assign(last, last + n_nodes);
  db->h_bin_taxid.assign(taxid, taxid + n_nodes);
  return 0;
}

namespace kmcpg {
void bin_stats_from_words(const unsigned long long* s, kmcpg_bin_stats* out) {
  out->no_bin = s[K11_NO_BIN];
  out->one = s[K11_ONE];
  out->several = s[K11_SEVERAL];
  out->left = s[K11_LEFT_READS];
  out->climb_steps = s[K11_STEPS];
  out->bad_segments = s[K11_BAD];
  out->skipped = s[K11_SKIPPED];
}
// K11 behind K3 (kmcpg_bin_device without the public entry's argument checks)
int bin_enqueue(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers, uint32_t n_reads, int32_t final_n,
                const uint64_t* d_n_hits, uint64_t hit_cap, uint32_t* d_bins, uint8_t* d_left, unsigned long long* d_stats, hipStream_t st) {
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  if (!db->binning_on() || !db->d_bin_tables) return kmcpg_fail(KMCPG_EINVAL, "the stage is off: call kmcpg_set_binning first");
  unsigned long long* const stats = d_stats ? d_stats : db->d_bin_stats;
  HIPCHK(hipMemsetAsync(stats, 0, K11_STATS * sizeof(unsigned long long), st));
  db->k11_log.clear();
  db->bin_ran = true;
  if (!d_stats) db->bin_from_ticket = false;  // (a lane's launch is reported with its ticket: kmcpg_wait_bins)
  db->bin_grid = 0;
  db->bin_timed = false;
  const uint32_t n_cols = (uint32_t)db->h_bin_node.size(), n_nodes = (uint32_t)db->h_bin_parent.size();
  db->bin_in_lds = n_nodes <= K11_LDS_NODES;
  if (n_reads == 0) return 0;
  K11Args a{};
  a.pairs = d_pairs;
  a.offs = d_read_offs;
  a.pair_cap = pair_cap;
  a.nk = d_qkmers;
  a.n_reads = n_reads;
  a.n_cols = n_cols;
  a.final_n = final_n;
  a.node_of_column = db->d_bin_tables;
  a.parent = db->d_bin_tables + n_cols;
  a.last = a.parent + n_nodes;
  a.taxid = a.last + n_nodes;
  a.n_nodes = n_nodes;
  a.n_hits = (const unsigned long long*)d_n_hits;
  a.hit_cap = hit_cap;
  a.bins = d_bins;
  a.left = d_left;
  a.stats = stats;
  db->bin_timed = db->profiling >= 1;
  if (int rc = timed_launches(db->bin_ev, db->bin_timed, st, [&] { db->bin_grid = launch_k11(a, db->bin_max_wgs, st, db->bin_timed ? &db->k11_log : nullptr, &db->bin_in_lds); }))
    return rc;
  HIPCHK(hipGetLastError());
  return 0;
}
}  // namespace kmcpg

extern "C" int kmcpg_bin_device(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers, uint32_t n_reads,
                                int32_t final_n, const uint64_t* d_n_hits, uint64_t hit_cap, uint32_t* d_bins, void* stream) {
  if (!db || !d_read_offs || (n_reads && (!d_qkmers || !d_bins)) || (pair_cap && !d_pairs)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (n_reads == 0xffffffffu) return kmcpg_fail(KMCPG_EINVAL, "too many reads");
  if (int rc = refuse(db)) return rc;
  return bin_enqueue(db, d_pairs, d_read_offs, pair_cap, d_qkmers, n_reads, final_n, d_n_hits, hit_cap, d_bins, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int kmcpg_last_bins(kmcpg_db* db, kmcpg_bin_stats* out, kmcpg_k4_launch* launches, uint32_t cap, uint32_t* n_launches) {
  if (!db || !out || !n_launches || (cap && !launches)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  memset(out, 0, sizeof *out);
  out->k11_ms = -1;
  *n_launches = 0;
  std::lock_guard<std::mutex> g(db->mu);
  if (!db->bin_ran || db->opts.device < 0 || !db->d_bin_stats) return 0;
  KMCPG_USE_DEVICE(db);
  HIPCHK(hipDeviceSynchronize());
  if (db->bin_from_ticket) *out = db->bin_ticket, out->k11_ms = -1;
  else {
    unsigned long long s[K11_STATS] = {};
    HIPCHK(hipMemcpy(s, db->d_bin_stats, sizeof s, hipMemcpyDeviceToHost));
    bin_stats_from_words(s, out);
  }
  out->grid = db->bin_grid;
  out->in_lds = db->bin_in_lds ? 1 : 0;
  timed_launches_report(db, db->bin_ev, db->bin_timed, db->k11_log, &out->k11_ms, launches, cap, n_launches);
  return 0;
}
