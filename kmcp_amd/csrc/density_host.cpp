// density_host.cpp — host side of index inspection (include/kmcp_gpu.h: kmcpg_density_bins, kmcpg_block_density, kmcpg_col_ones,
// kmcpg_last_density_launch): what `kmcp utils index-density` and `kmcp utils ref-info` need from resident rows
// (kmcp/cmd/index-density.go:139-213; ref-info.go:128-150 prints the header's side of it).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "engine.hpp"
#include "kernels.hpp"

using namespace kmcpg;

namespace {

// the rows of a request: [first, last) of block b, or an error
int density_rows(const kmcpg_db* db, uint32_t block, const kmcpg_density_spec* s, uint64_t* first, uint64_t* last) {
  if (!db || !s) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (db->paged_passes > 0 || !db->shards.empty())
    return kmcpg_fail(KMCPG_EUNSUPPORTED, "index inspection needs a handle with resident rows of its own: open the database with kmcpg_open or kmcpg_open_files");
  if (block >= db->blocks.size()) return kmcpg_fail(KMCPG_EINVAL, "block %u out of range (%zu blocks)", block, db->blocks.size());
  const BlockMeta& b = db->blocks[block];
  if (!b.local) return kmcpg_fail(KMCPG_EINVAL, "block %u is not resident on this rank", block);
  if (s->reserved != 0) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_density_spec.reserved must be 0");
  if (s->bin_rows == 0) return kmcpg_fail(KMCPG_EINVAL, "bin_rows must be >= 1");
  if (s->first_row >= b.h.num_sigs || s->n_rows > b.h.num_sigs - s->first_row)
    return kmcpg_fail(KMCPG_EINVAL, "rows %llu + %llu outside the block's %llu rows", (unsigned long long)s->first_row, (unsigned long long)s->n_rows,
                      (unsigned long long)b.h.num_sigs);
  *first = s->first_row;
  *last = s->n_rows ? s->first_row + s->n_rows : b.h.num_sigs;
  return 0;
}

struct DevMem {  // scratch of one call: freed on every path
  void* p = nullptr;
  ~DevMem() {
    if (p) (void)hipFree(p);
  }
  int alloc(uint64_t bytes, const char* what) {
    if (hipError_t e = hipMalloc(&p, bytes); e != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();
      return kmcpg_fail(e == hipErrorOutOfMemory ? KMCPG_ENOMEM : KMCPG_EDEVICE, "hipMalloc of %llu bytes for %s failed: %s", (unsigned long long)bytes, what,
                        hipGetErrorString(e));
    }
    return 0;
  }
};

void note_launch(kmcpg_db* db, const DensityPlan& p, bool first) {
  kmcpg_density_launch& L = db->last_density;
  if (first) L = kmcpg_density_launch{};
  L.form = p.form;
  L.lpr = p.lpr;
  L.npl = p.npl;
  L.workgroups += (uint32_t)std::min<uint64_t>(p.form == 0 ? p.workgroups : 0, 0xffffffffu - L.workgroups);
  L.launches++;
}

// HIP events around the device work of one call (kmcpg_last_density_ms)
struct CallTimer {
  hipEvent_t a = nullptr, b = nullptr;
  ~CallTimer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  void start() {
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess || hipEventRecord(a, nullptr) != hipSuccess) (void)hipGetLastError();
  }
  void stop() {
    if (a && b) (void)hipEventRecord(b, nullptr);
  }
  float ms() {  // after the call's last synchronising copy
    float t = -1;
    if (!a || !b || hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&t, a, b) != hipSuccess) {
      (void)hipGetLastError();
      return -1;
    }
    return t;
  }
};

constexpr uint64_t kScratchBytes = 512ull << 20;  // bins are counted in batches whose two device arrays stay below this

}  // namespace

extern "C" int kmcpg_density_bins(const kmcpg_db* db, uint32_t block, const kmcpg_density_spec* spec, uint64_t* n_bins) {
  uint64_t first = 0, last = 0;
  if (int rc = density_rows(db, block, spec, &first, &last)) return rc;
  if (!n_bins) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  const uint64_t rows = last - first;
  *n_bins = rows / spec->bin_rows + (rows % spec->bin_rows ? 1 : 0);
  return 0;
}

extern "C" int kmcpg_block_density(kmcpg_db* db, uint32_t block, const kmcpg_density_spec* spec, uint32_t* counts, uint64_t cap) {
  uint64_t first = 0, last = 0;
  if (int rc = density_rows(db, block, spec, &first, &last)) return rc;
  const BlockMeta& b = db->blocks[block];
  const uint64_t rows = last - first, bin_rows = spec->bin_rows;
  const uint64_t n_bins = rows / bin_rows + (rows % bin_rows ? 1 : 0);
  const uint32_t ncols = (uint32_t)b.h.names.size();
  if (!counts || n_bins > ~0ull / std::max<uint32_t>(1, ncols) || cap < n_bins * ncols)
    return kmcpg_fail(KMCPG_EINVAL, "counts: room for %llu x %u elements needed, cap = %llu", (unsigned long long)n_bins, ncols, (unsigned long long)cap);
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  const Group& G = db->groups[(size_t)b.group];
  // the aligned 16-byte lanes of the group's row that overlap the block's bytes
  const uint32_t lane0 = b.byte_off / 16u, lane1 = (b.byte_off + b.h.row_bytes + 15u) / 16u;
  const uint32_t col0 = (b.byte_off - lane0 * 16u) * 8u;
  const uint64_t width = plan_density(lane1 - lane0, rows, bin_rows).width;
  const uint64_t per_bin = (width + ncols) * sizeof(uint32_t);
  const uint64_t batch = std::min<uint64_t>(n_bins, std::max<uint64_t>(1, kScratchBytes / per_bin));
  DevMem d_bins, d_out;
  if (int rc = d_bins.alloc(batch * width * sizeof(uint32_t), "the counts of a batch of bins")) return rc;
  if (int rc = d_out.alloc(batch * ncols * sizeof(uint32_t), "the counts of a batch of bins, column-major")) return rc;
  bool first_launch = true;
  float ms_sum = 0;
  for (uint64_t b0 = 0; b0 < n_bins; b0 += batch) {
    CallTimer tm;
    tm.start();
    const uint64_t nb = std::min(batch, n_bins - b0);
    DensityArgs a{};
    a.rows = G.d_rows;
    a.stride = G.stride;
    a.lane0 = lane0;
    a.nlanes = lane1 - lane0;
    a.first_row = first + b0 * bin_rows;
    a.last_row = nb * bin_rows > last - a.first_row ? last : a.first_row + nb * bin_rows;
    a.bin_rows = bin_rows;
    a.out = (uint32_t*)d_bins.p;
    const DensityPlan p = plan_density(a.nlanes, a.last_row - a.first_row, bin_rows);
    HIPCHK(hipMemsetAsync(d_bins.p, 0, nb * width * sizeof(uint32_t), nullptr));
    if (launch_density(p, a, nullptr) < 0) return kmcpg_fail(KMCPG_EINVAL, "density: no kernel for this request");
    note_launch(db, p, first_launch);
    first_launch = false;
    launch_density_transpose((const uint32_t*)d_bins.p, width, col0, ncols, nb, (uint32_t*)d_out.p, nullptr);
    tm.stop();
    if (nb == n_bins) HIPCHK(hipMemcpy(counts, d_out.p, nb * ncols * sizeof(uint32_t), hipMemcpyDeviceToHost));
    else
      HIPCHK(hipMemcpy2D(counts + b0, n_bins * sizeof(uint32_t), d_out.p, nb * sizeof(uint32_t), nb * sizeof(uint32_t), ncols, hipMemcpyDeviceToHost));
    const float t = tm.ms();
    ms_sum = t < 0 || ms_sum < 0 ? -1 : ms_sum + t;
  }
  db->last_density_ms = ms_sum;
  return 0;
}

extern "C" int kmcpg_col_ones(kmcpg_db* db, uint64_t* ones, uint64_t cap) {
  if (!db || !ones) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (db->paged_passes > 0 || !db->shards.empty())
    return kmcpg_fail(KMCPG_EUNSUPPORTED, "index inspection needs a handle with resident rows of its own: open the database with kmcpg_open or kmcpg_open_files");
  const uint64_t n_cols = db->col_block.size();
  if (cap < n_cols) return kmcpg_fail(KMCPG_EINVAL, "ones: room for %llu elements needed, cap = %llu", (unsigned long long)n_cols, (unsigned long long)cap);
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  if (n_cols == 0) return 0;
  uint64_t width_max = 0;
  for (const Group& G : db->groups)
    if (G.num_sigs) width_max = std::max<uint64_t>(width_max, plan_density((G.row_bytes + 15u) / 16u, G.num_sigs, G.num_sigs).width);
  DevMem d_ones, d_bin;
  if (int rc = d_ones.alloc(n_cols * sizeof(uint64_t), "the columns' counts")) return rc;
  CallTimer tm;
  tm.start();
  HIPCHK(hipMemsetAsync(d_ones.p, 0, n_cols * sizeof(uint64_t), nullptr));
  if (width_max)
    if (int rc = d_bin.alloc(width_max * sizeof(uint32_t), "the counts of a group's row")) return rc;
  bool first_launch = true;
  for (size_t gi = 0; gi < db->groups.size(); gi++) {
    const Group& G = db->groups[gi];
    const BlockDev& gd = db->h_groupdev[gi];
    if (G.num_sigs == 0) continue;
    DensityArgs a{};
    a.rows = G.d_rows;
    a.stride = G.stride;
    a.lane0 = 0;
    a.nlanes = (G.row_bytes + 15u) / 16u;  // the lanes that hold columns: row padding is not read
    a.first_row = 0;
    a.last_row = G.num_sigs;
    a.bin_rows = G.num_sigs;  // one bin: a column's count is below 2^32 (rows are addressed with 32 bits)
    a.out = (uint32_t*)d_bin.p;
    const DensityPlan p = plan_density(a.nlanes, G.num_sigs, G.num_sigs);
    HIPCHK(hipMemsetAsync(d_bin.p, 0, p.width * sizeof(uint32_t), nullptr));
    if (launch_density(p, a, nullptr) < 0) return kmcpg_fail(KMCPG_EINVAL, "density: no kernel for this request");
    note_launch(db, p, first_launch);
    first_launch = false;
    uint32_t max_ncols = 0;
    for (uint32_t s = 0; s < gd.nsegs; s++) max_ncols = std::max(max_ncols, db->h_segs[gd.seg0 + s].ncols);
    launch_density_cols((const uint32_t*)d_bin.p, db->d_segs + gd.seg0, gd.nsegs, max_ncols, (uint64_t*)d_ones.p, nullptr);
  }
  tm.stop();
  HIPCHK(hipMemcpy(ones, d_ones.p, n_cols * sizeof(uint64_t), hipMemcpyDeviceToHost));
  db->last_density_ms = tm.ms();
  return 0;
}

extern "C" int kmcpg_last_density_launch(kmcpg_db* db, kmcpg_density_launch* out) {
  if (!db || !out) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  *out = db->last_density;
  return 0;
}

extern "C" int kmcpg_last_density_ms(kmcpg_db* db, float* ms) {
  if (!db || !ms) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(db->mu);
  if (db->last_density_ms < 0) return kmcpg_fail(KMCPG_EINVAL, "no density call has been timed on this handle");
  *ms = db->last_density_ms;
  return 0;
}

extern "C" int kmcpg_stream_probe(kmcpg_db* db, float* ms, uint64_t* bytes) {
  if (!db || !ms || !bytes) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (db->paged_passes > 0 || !db->shards.empty()) return kmcpg_fail(KMCPG_EUNSUPPORTED, "needs a handle with resident rows of its own");
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  DevMem d_out;
  if (int rc = d_out.alloc(64, "the probe's output word")) return rc;
  CallTimer tm;
  tm.start();
  uint64_t total = 0;
  for (const Group& G : db->groups) {
    const uint64_t b = G.num_sigs * (uint64_t)G.stride;
    launch_stream_probe(G.d_rows, b, (uint32_t*)d_out.p, nullptr);
    total += b / 16u * 16u;
  }
  tm.stop();
  HIPCHK(hipDeviceSynchronize());
  *ms = tm.ms();
  *bytes = total;
  if (*ms < 0) return kmcpg_fail(KMCPG_EDEVICE, "HIP event timing failed");
  return 0;
}
