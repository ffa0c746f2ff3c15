// build.cpp — kmcpg_build_db: `kmcp index` on the GPU from lists of k-mer hashes.
// Host part: block layout (kmcp/cmd/index.go:657-682), signature size (util-hash.go:46-50), .uniki header
// (index/serialization.go:159-300), __db.yml (util-db-info.go:46-79), __name_mapping.tsv (index.go:1375-1393).
// Device part: the Bloom-column scatter (index.go:1107-1309) as one atomicOr per (k-mer, hash).
#include <errno.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <string>
#include <vector>

#include "build_plan.hpp"
#include "engine.hpp"
#include "fastmod.hpp"
#include "kernels.hpp"

using namespace kmcpg;



namespace {

void be32(FILE* f, uint32_t v) { plan_be32(f, v); }
void be64(FILE* f, uint64_t v) { plan_be64(f, v); }
int mkdirs(const std::string& d) { return plan_mkdirs(d); }

#define BHIP(expr)                                                                                        \
  do {                                                                                                    \
    hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess) {                                                                               \
      rc = kmcpg_fail(KMCPG_EDEVICE, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      goto done;                                                                                          \
    }                                                                                                     \
  } while (0)

// one block: its columns' lists up in groups, one scatter launch per group, the matrix down and behind the header
int build_block(const std::string& path, const kmcpg_build_cfg& cfg, const kmcpg_build_col* in, const PlanCol* meta, const PlanBlock& b) {
  int rc = 0;
  const uint32_t n = (uint32_t)b.cols.size();
  const uint64_t num_sigs = b.num_sigs;
  uint64_t max_elems = 0;
  for (uint32_t c : b.cols) max_elems = std::max(max_elems, in[c].n_hashes);
  const uint32_t row_bytes = b.row_bytes;
  const uint64_t bytes = b.matrix_bytes;
  uint8_t* d_sigs = nullptr;
  uint64_t *d_hashes = nullptr, *d_off = nullptr;
  std::vector<uint8_t> host;
  FILE* f = nullptr;
  const uint64_t chunk_cap = std::max<uint64_t>(max_elems, 64ull << 20);  // hashes per upload
  std::vector<uint64_t> stage, off;
  BHIP(hipMalloc((void**)&d_sigs, bytes + 8));
  BHIP(hipMemset(d_sigs, 0, bytes + 8));
  BHIP(hipMalloc((void**)&d_hashes, chunk_cap * sizeof(uint64_t)));
  BHIP(hipMalloc((void**)&d_off, ((size_t)n + 1) * sizeof(uint64_t)));
  for (uint32_t c0 = 0; c0 < n;) {  // groups of consecutive columns that fit one upload
    stage.clear();
    off.assign(1, 0);
    uint32_t c1 = c0;
    while (c1 < n && (c1 == c0 || stage.size() + in[b.cols[c1]].n_hashes <= chunk_cap)) {
      const kmcpg_build_col& c = in[b.cols[c1]];
      stage.insert(stage.end(), c.hashes, c.hashes + c.n_hashes);
      off.push_back(stage.size());
      c1++;
    }
    if (!stage.empty()) {
      BHIP(hipMemcpy(d_hashes, stage.data(), stage.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
      BHIP(hipMemcpy(d_off, off.data(), off.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
      launch_build_scatter(d_sigs, num_sigs, fastmod_magic(num_sigs), row_bytes, cfg.num_hashes, d_hashes, d_off, c0, c1 - c0, stage.size(), nullptr);
      BHIP(hipDeviceSynchronize());
    }
    c0 = c1;
  }
  host.resize(bytes);
  BHIP(hipMemcpy(host.data(), d_sigs, bytes, hipMemcpyDeviceToHost));
  f = fopen(path.c_str(), "wb");
  if (!f) {
    rc = kmcpg_fail(KMCPG_EIO, "cannot write %s: %s", path.c_str(), strerror(errno));
    goto done;
  }
  write_uniki_header(f, cfg, meta, b);
  if (fwrite(host.data(), 1, bytes, f) != bytes) rc = kmcpg_fail(KMCPG_EIO, "short write on %s", path.c_str());
done:
  if (f) fclose(f);
  if (d_sigs) (void)hipFree(d_sigs);
  if (d_hashes) (void)hipFree(d_hashes);
  if (d_off) (void)hipFree(d_off);
  return rc;
}

}  // namespace

extern "C" int kmcpg_build_db(const char* out_dir, const kmcpg_build_cfg* cfg, const kmcpg_build_col* cols, uint32_t n_cols, int32_t device) {
  if (!out_dir || !cfg || !cols || n_cols == 0) return kmcpg_fail(KMCPG_EINVAL, "bad argument");
  if (cfg->num_hashes < 1 || cfg->num_hashes > 4 || !(cfg->fpr > 0 && cfg->fpr < 1) || cfg->k < 1 || cfg->k > 255)
    return kmcpg_fail(KMCPG_EINVAL, "bad build configuration");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return kmcpg_fail(KMCPG_EDEVICE, "no HIP device available: libkmcpgpu has no CPU fallback");
  if (device < 0 || device >= ndev) return kmcpg_fail(KMCPG_EINVAL, "device %d out of range", device);
  if (hipSetDevice(device) != hipSuccess) return kmcpg_fail(KMCPG_EDEVICE, "hipSetDevice failed");
  std::vector<PlanCol> meta(n_cols);
  std::vector<uint64_t> counts(n_cols);
  for (uint32_t i = 0; i < n_cols; i++) {
    if (!cols[i].name || (!cols[i].hashes && cols[i].n_hashes)) return kmcpg_fail(KMCPG_EINVAL, "column %u: null name or hashes", i);
    meta[i] = PlanCol{cols[i].name, cols[i].gsize, cols[i].chunk_idx, cols[i].chunks, cols[i].n_hashes};
    counts[i] = cols[i].n_hashes;
  }
  const std::string dir = std::string(out_dir) + "/R001";
  if (mkdirs(dir) != 0) return kmcpg_fail(KMCPG_EIO, "cannot create %s: %s", dir.c_str(), strerror(errno));
  BuildPlan plan;  // the layout is a function of the counts alone (build_plan.hpp)
  const std::string err = build_plan(counts.data(), n_cols, *cfg, &plan);
  if (!err.empty()) return kmcpg_fail(KMCPG_EINVAL, "%s", err.c_str());
  for (size_t bi = 0; bi < plan.blocks.size(); bi++) {
    int rc = build_block(dir + "/" + block_file_name(bi), *cfg, cols, meta.data(), plan.blocks[bi]);
    if (rc) return rc;
  }
  if (!write_db_yml(dir, *cfg, n_cols, plan)) return kmcpg_fail(KMCPG_EIO, "cannot write %s/__db.yml", dir.c_str());
  write_name_mapping(dir, meta.data(), n_cols);
  return 0;
}

// The resident database back to disk in the reference's format (benchmarking support, no counterpart in the reference): a synthetic
// index generated in HBM (kmcpg_open_synthetic + kmcpg_plant_reads_device) becomes <out_dir>/R001/{_blockNNN.uniki, __db.yml,
// __name_mapping.tsv}, which kmcp-search — or `kmcp search` — opens like any database `kmcp index` wrote (index/serialization.go:159-300,
// util-db-info.go:46-79).  bench.py's end-to-end leg uses it to put BASELINE configs[1] on /dev/shm.  Every block must be resident.
extern "C" int kmcpg_save_db(kmcpg_db* db, const char* out_dir) {
  if (!db || !out_dir) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (int rc = kmcpg::set_refuse_entry(db, "kmcpg_save_db")) return rc;
  for (const auto& b : db->blocks)
    if (!b.local) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_save_db needs every block resident on this handle (one GPU, one shard)");
  const std::string dir = std::string(out_dir) + "/R001";
  if (mkdirs(dir) != 0) return kmcpg_fail(KMCPG_EIO, "cannot create %s: %s", dir.c_str(), strerror(errno));
  std::vector<std::string> files;
  std::vector<uint8_t> host;
  uint64_t total_kmers = 0;
  for (size_t bi = 0; bi < db->blocks.size(); bi++) {
    const kmcpg::UnikiHeader& h = db->blocks[bi].h;
    const uint32_t n = (uint32_t)h.names.size();
    char name[64];
    snprintf(name, sizeof name, "_block%03zu.uniki", bi + 1);
    const std::string path = dir + "/" + name;
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return kmcpg_fail(KMCPG_EIO, "cannot write %s: %s", path.c_str(), strerror(errno));
    fwrite(".kmcpidx", 1, 8, f);
    const uint8_t meta[4] = {4, (uint8_t)h.k, (uint8_t)((h.canonical ? 1 : 0) | 2), (uint8_t)h.num_hashes};
    fwrite(meta, 1, 4, f);
    be64(f, h.num_sigs);
    be32(f, n);
    for (const auto& nm : h.names) {
      be32(f, (uint32_t)nm.size() + 1);
      fwrite(nm.data(), 1, nm.size(), f);
      fputc('\n', f);
    }
    be32(f, n);
    for (uint32_t c = 0; c < n; c++) {
      be32(f, 1);
      be64(f, h.gsizes[c]);
    }
    be32(f, n);
    for (uint32_t c = 0; c < n; c++) {
      be32(f, 1);
      be32(f, h.indices[c]);
    }
    for (uint32_t c = 0; c < n; c++) {
      be64(f, h.sizes[c]);
      total_kmers += h.sizes[c];
    }
    const uint64_t chunk = std::max<uint64_t>(1, (256ull << 20) / h.row_bytes);
    host.resize((size_t)(std::min(chunk, h.num_sigs) * h.row_bytes));
    int rc = 0;
    for (uint64_t r0 = 0; r0 < h.num_sigs && rc == 0; r0 += chunk) {
      const uint64_t nr = std::min(chunk, h.num_sigs - r0);
      rc = kmcpg_read_row_range(db, (uint32_t)bi, r0, nr, host.data());
      if (rc == 0 && fwrite(host.data(), 1, (size_t)(nr * h.row_bytes), f) != (size_t)(nr * h.row_bytes)) rc = kmcpg_fail(KMCPG_EIO, "short write on %s", path.c_str());
    }
    fclose(f);
    if (rc) return rc;
    files.push_back(name);
  }
  const kmcpg_info& I = db->info;
  FILE* f = fopen((dir + "/__db.yml").c_str(), "w");
  if (!f) return kmcpg_fail(KMCPG_EIO, "cannot write %s/__db.yml", dir.c_str());
  auto b = [](int v) { return v ? "true" : "false"; };
  fprintf(f, "version: 4\nunikiVersion: 4\nalias: kmcp-gpu-saved\nk: %d\nks:\n", I.k);
  std::vector<int> ks(db->ks_desc.rbegin(), db->ks_desc.rend());  // ascending, as `kmcp index` lists them
  if (ks.empty()) ks.push_back(I.k);
  for (int k : ks) fprintf(f, "- %d\n", k);
  fprintf(f, "hashed: true\ncanonical: %s\n", b(I.canonical));
  fprintf(f, "scaled: %s\nscale: %u\nminimizer: %s\nminimizer-w: %u\nsyncmer: %s\nsyncmer-s: %u\n", b(I.scaled), I.scaled ? I.scale : 1, b(I.minimizer),
          I.minimizer_w, b(I.syncmer), I.syncmer_s);
  fprintf(f, "split-seq: false\nsplit-size: 0\nsplit-num: 0\nsplit-overlap: 0\ncompact-size: true\n");
  fprintf(f, "hashes: %d\nfpr: %.17g\nnumNameGroups: %llu\nblocksize: %u\ntotalKmers: %llu\nfiles:\n", I.num_hashes, I.fpr, (unsigned long long)I.n_cols,
          db->blocks.empty() ? 0u : (uint32_t)db->blocks[0].h.names.size(), (unsigned long long)total_kmers);
  for (const auto& fn : files) fprintf(f, "- %s\n", fn.c_str());
  fclose(f);
  f = fopen((dir + "/__name_mapping.tsv").c_str(), "w");
  if (f) {
    for (const auto& bl : db->blocks)
      for (const auto& nm : bl.h.names) fprintf(f, "%s\t%s\n", nm.c_str(), nm.c_str());
    fclose(f);
  }
  return 0;
}
