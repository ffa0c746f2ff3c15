// builder.cpp — kmcpg_builder: `kmcp index` in two passes (include/kmcp_gpu.h says what for).  Pass 1 gives the counts, build_plan.hpp
// lays out blocks and rounds from them, pass 2 ORs device-resident lists into block matrices that stay in HBM (build_scatter.hip: one
// launch per scatter call) and every matrix is written once.  Header, __db.yml and __name_mapping.tsv come from the writers kmcpg_build_db
// uses, so the files of the two paths are the same bytes.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "build_plan.hpp"
#include "build_scatter.hpp"
#include "engine.hpp"
#include "fastmod.hpp"

using namespace kmcpg;

namespace {

enum BuilderState { B_COLS = 0, B_PLANNED, B_ROUND_OPEN, B_FINISHED };

// descriptor table + prefix table of one launch: page-locked on the host, a copy on the device.  Two of them alternate, and one is
// rewritten only after the launch that read it has run (its `stop` event)
struct StageSlot {
  uint8_t* h = nullptr;
  uint8_t* d = nullptr;
  size_t cap = 0;
  hipEvent_t start = nullptr, stop = nullptr;
  bool pending = false;
};

}  // namespace

struct kmcpg_builder {
  mutable std::mutex mu;
  kmcpg_builder_cfg cfg{};
  std::string alias;
  int32_t device = -1;
  BuilderState state = B_COLS;
  std::vector<std::string> names;
  std::vector<PlanCol> cols;
  BuildPlan plan;
  std::vector<uint32_t> round_of_block, block_of_col, pos_of_col;
  uint32_t n_rounds = 0;
  std::vector<uint8_t> round_done;
  uint32_t open_round = 0;
  std::vector<uint8_t*> d_matrix;   // per block, resident in the open round only
  std::vector<uint8_t> scattered;   // per column, in the open round
  std::vector<uint32_t> seen_call;  // per column: the scatter call that last named it (a column twice in one call)
  uint32_t call_epoch = 0;
  StageSlot slot[2];
  int next_slot = 0;
  kmcpg_builder_stats st{};
};

namespace {

const char* expected(const kmcpg_builder* b) {
  switch (b->state) {
    case B_COLS: return "kmcpg_builder_add_cols or kmcpg_builder_plan";
    case B_PLANNED: {
      for (uint8_t d : b->round_done)
        if (!d) return "kmcpg_builder_begin_round";
      return "kmcpg_builder_finish";
    }
    case B_ROUND_OPEN: return "kmcpg_builder_scatter_device or kmcpg_builder_end_round";
    default: return "kmcpg_builder_close";
  }
}

int out_of_order(const kmcpg_builder* b, const char* call) { return kmcpg_fail(KMCPG_EINVAL, "%s out of order: %s expected", call, expected(b)); }

// the milliseconds of a slot's launch, once it has run
int harvest(kmcpg_builder* b, StageSlot& s) {
  if (!s.pending) return 0;
  HIPCHK(hipEventSynchronize(s.stop));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, s.start, s.stop));
  b->st.scatter_ms += (double)ms;
  s.pending = false;
  return 0;
}

void free_slot(StageSlot& s) {
  if (s.h) (void)hipHostFree(s.h);
  if (s.d) (void)hipFree(s.d);
  s.h = s.d = nullptr;
  s.cap = 0;
}

void free_matrices(kmcpg_builder* b) {
  for (auto& p : b->d_matrix)
    if (p) {
      (void)hipFree(p);
      p = nullptr;
    }
  b->st.matrix_bytes_resident = 0;
}

}  // namespace

extern "C" int kmcpg_builder_open(const kmcpg_builder_cfg* cfg, int32_t device, kmcpg_builder** out) {
  if (!cfg || !out) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  *out = nullptr;
  for (uint64_t r : cfg->reserved)
    if (r) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_builder_cfg.reserved must be 0");
  const std::string err = build_cfg_error(cfg->build);
  if (!err.empty()) return kmcpg_fail(KMCPG_EINVAL, "%s", err.c_str());
  if (device < -1) return kmcpg_fail(KMCPG_EINVAL, "device %d out of range", device);
  if (device >= 0) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return kmcpg_fail(KMCPG_EDEVICE, "no HIP device available: libkmcpgpu has no CPU fallback");
    if (device >= ndev) return kmcpg_fail(KMCPG_EINVAL, "device %d out of range", device);
    HIPCHK(hipSetDevice(device));
  }
  kmcpg_builder* b = new kmcpg_builder();
  b->cfg = *cfg;
  b->alias = cfg->build.alias ? cfg->build.alias : "kmcp-gpu-db";
  b->cfg.build.alias = b->alias.c_str();
  b->device = device;
  b->st.slice_keys = BS_SLICE_KEYS;
  if (device >= 0)
    for (auto& s : b->slot)
      if (hipEventCreate(&s.start) != hipSuccess || hipEventCreate(&s.stop) != hipSuccess) {
        kmcpg_builder_close(b);
        return kmcpg_fail(KMCPG_EDEVICE, "hipEventCreate failed");
      }
  *out = b;
  return 0;
}

extern "C" int kmcpg_builder_close(kmcpg_builder* b) {
  if (!b) return 0;
  if (b->device >= 0) {
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize();
    free_matrices(b);
    for (auto& s : b->slot) {
      free_slot(s);
      if (s.start) (void)hipEventDestroy(s.start);
      if (s.stop) (void)hipEventDestroy(s.stop);
    }
  }
  delete b;
  return 0;
}

extern "C" int kmcpg_builder_add_cols(kmcpg_builder* b, const kmcpg_build_colmeta* cols, uint32_t n) {
  if (!b || (n && !cols)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(b->mu);
  if (b->state != B_COLS) return out_of_order(b, "kmcpg_builder_add_cols");
  if ((uint64_t)b->cols.size() + n >= 0xffffffffull) return kmcpg_fail(KMCPG_EINVAL, "fewer than 2^32 - 1 columns wanted");
  for (uint32_t i = 0; i < n; i++)
    if (!cols[i].name) return kmcpg_fail(KMCPG_EINVAL, "column %zu: null name", b->cols.size() + i);
  for (uint32_t i = 0; i < n; i++) {
    b->names.emplace_back(cols[i].name);
    b->cols.push_back(PlanCol{nullptr, cols[i].gsize, cols[i].chunk_idx, cols[i].chunks, cols[i].n_hashes});
  }
  return 0;
}

extern "C" int kmcpg_builder_plan(kmcpg_builder* b, uint64_t matrix_budget, uint32_t* n_blocks, uint32_t* n_rounds) {
  if (!b) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(b->mu);
  if (b->state != B_COLS) return out_of_order(b, "kmcpg_builder_plan");
  if (b->cols.empty()) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_builder_plan out of order: kmcpg_builder_add_cols expected (no column yet)");
  if (matrix_budget == 0) {
    if (b->device < 0) return kmcpg_fail(KMCPG_EINVAL, "a planning-only builder (device -1) needs an explicit matrix_budget");
    HIPCHK(hipSetDevice(b->device));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    if ((uint64_t)free_b <= b->cfg.hbm_reserve)
      return kmcpg_fail(KMCPG_ENOMEM, "%llu bytes of HBM free, not above the reserve of %llu", (unsigned long long)free_b, (unsigned long long)b->cfg.hbm_reserve);
    matrix_budget = (uint64_t)free_b - b->cfg.hbm_reserve;
  }
  const uint32_t n = (uint32_t)b->cols.size();
  std::vector<uint64_t> counts(n);
  for (uint32_t i = 0; i < n; i++) {
    b->cols[i].name = b->names[i].c_str();  // the strings no longer move
    counts[i] = b->cols[i].n_hashes;
  }
  BuildPlan plan;
  std::string err = build_plan(counts.data(), n, b->cfg.build, &plan);
  if (!err.empty()) return kmcpg_fail(KMCPG_EINVAL, "%s", err.c_str());
  std::vector<uint32_t> round;
  uint32_t nr = 0;
  err = build_rounds(plan, matrix_budget, &round, &nr);
  if (!err.empty()) return kmcpg_fail(KMCPG_ENOMEM, "%s", err.c_str());
  b->plan = std::move(plan);
  b->round_of_block = std::move(round);
  b->n_rounds = nr;
  b->round_done.assign(nr, 0);
  b->block_of_col.assign(n, UINT32_MAX);
  b->pos_of_col.assign(n, UINT32_MAX);
  for (size_t bi = 0; bi < b->plan.blocks.size(); bi++)
    for (size_t j = 0; j < b->plan.blocks[bi].cols.size(); j++) {
      b->block_of_col[b->plan.blocks[bi].cols[j]] = (uint32_t)bi;
      b->pos_of_col[b->plan.blocks[bi].cols[j]] = (uint32_t)j;
    }
  b->d_matrix.assign(b->plan.blocks.size(), nullptr);
  b->scattered.assign(n, 0);
  b->seen_call.assign(n, 0);
  b->state = B_PLANNED;
  if (n_blocks) *n_blocks = (uint32_t)b->plan.blocks.size();
  if (n_rounds) *n_rounds = nr;
  return 0;
}

extern "C" int kmcpg_builder_col_place(const kmcpg_builder* b, uint32_t col, uint32_t* block, uint32_t* col_in_block, uint32_t* round) {
  if (!b) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(b->mu);
  if (b->state == B_COLS) return out_of_order(b, "kmcpg_builder_col_place");
  if (col >= b->cols.size()) return kmcpg_fail(KMCPG_EINVAL, "column %u out of range (%zu columns)", col, b->cols.size());
  const uint32_t bi = b->block_of_col[col];
  if (block) *block = bi;
  if (col_in_block) *col_in_block = b->pos_of_col[col];
  if (round) *round = bi == UINT32_MAX ? UINT32_MAX : b->round_of_block[bi];
  return 0;
}

extern "C" int kmcpg_builder_block_info(const kmcpg_builder* b, uint32_t block, uint64_t* num_sigs, uint32_t* n_cols, uint32_t* row_bytes, uint32_t* round) {
  if (!b) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(b->mu);
  if (b->state == B_COLS) return out_of_order(b, "kmcpg_builder_block_info");
  if (block >= b->plan.blocks.size()) return kmcpg_fail(KMCPG_EINVAL, "block %u out of range (%zu blocks)", block, b->plan.blocks.size());
  const PlanBlock& pb = b->plan.blocks[block];
  if (num_sigs) *num_sigs = pb.num_sigs;
  if (n_cols) *n_cols = (uint32_t)pb.cols.size();
  if (row_bytes) *row_bytes = pb.row_bytes;
  if (round) *round = b->round_of_block[block];
  return 0;
}

extern "C" int kmcpg_builder_begin_round(kmcpg_builder* b, uint32_t round) {
  if (!b) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(b->mu);
  if (b->state != B_PLANNED) return out_of_order(b, "kmcpg_builder_begin_round");
  if (round >= b->n_rounds) return kmcpg_fail(KMCPG_EINVAL, "round %u out of range (%u rounds)", round, b->n_rounds);
  if (b->round_done[round]) return kmcpg_fail(KMCPG_EINVAL, "round %u is built already", round);
  if (b->device < 0) return kmcpg_fail(KMCPG_EDEVICE, "planning-only builder (device -1): no GPU work possible");
  HIPCHK(hipSetDevice(b->device));
  uint64_t resident = 0;
  for (size_t bi = 0; bi < b->plan.blocks.size(); bi++) {
    if (b->round_of_block[bi] != round) continue;
    const uint64_t bytes = b->plan.blocks[bi].matrix_bytes + 8;
    if (hipMalloc((void**)&b->d_matrix[bi], bytes) != hipSuccess || hipMemset(b->d_matrix[bi], 0, bytes) != hipSuccess) {
      (void)hipGetLastError();
      b->d_matrix[bi] = nullptr;
      free_matrices(b);
      return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc of %llu bytes for the matrix of block %zu failed (round %u: lower the matrix budget)", (unsigned long long)bytes,
                        bi + 1, round);
    }
    resident += bytes;
    for (uint32_t c : b->plan.blocks[bi].cols) b->scattered[c] = 0;
  }
  HIPCHK(hipDeviceSynchronize());  // the zeroes are there before a scatter on any stream
  b->st.matrix_bytes_resident = resident;
  b->st.matrix_bytes_peak = std::max(b->st.matrix_bytes_peak, resident);
  b->open_round = round;
  b->state = B_ROUND_OPEN;
  return 0;
}

extern "C" int kmcpg_builder_scatter_device(kmcpg_builder* b, const uint64_t* d_hashes, const uint64_t* koff, const uint32_t* cols, uint32_t n_lists,
                                            void* stream) {
  if (!b || (n_lists && (!koff || !cols))) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(b->mu);
  if (b->state != B_ROUND_OPEN) return out_of_order(b, "kmcpg_builder_scatter_device");
  // every refusal comes before anything is changed or launched
  const uint32_t epoch = ++b->call_epoch;
  uint32_t n_desc = 0;
  uint64_t n_slices = 0, keys = 0;
  for (uint32_t i = 0; i < n_lists; i++) {
    if (koff[i + 1] < koff[i]) return kmcpg_fail(KMCPG_EINVAL, "koff must not decrease (list %u)", i);
    const uint32_t c = cols[i];
    if (c == UINT32_MAX) continue;
    if (c >= b->cols.size()) return kmcpg_fail(KMCPG_EINVAL, "list %u: column %u out of range (%zu columns)", i, c, b->cols.size());
    const uint64_t n = koff[i + 1] - koff[i];
    if (n != b->cols[c].n_hashes)
      return kmcpg_fail(KMCPG_EINVAL, "column %u (%s): %llu k-mers now, %llu in pass 1: the input changed between the passes", c, b->names[c].c_str(),
                        (unsigned long long)n, (unsigned long long)b->cols[c].n_hashes);
    if (b->seen_call[c] == epoch) return kmcpg_fail(KMCPG_EINVAL, "column %u (%s) given twice in one call", c, b->names[c].c_str());
    b->seen_call[c] = epoch;
    const uint32_t bi = b->block_of_col[c];
    if (bi == UINT32_MAX || b->round_of_block[bi] != b->open_round) continue;
    if (b->scattered[c]) return kmcpg_fail(KMCPG_EINVAL, "column %u (%s) given twice in round %u", c, b->names[c].c_str(), b->open_round);
    n_desc++;
    n_slices += (n + BS_SLICE_KEYS - 1) / BS_SLICE_KEYS;
    keys += n;
  }
  if (n_slices >= (1ull << 32) - 4) return kmcpg_fail(KMCPG_EUNSUPPORTED, "%llu keys in one scatter call: split the call", (unsigned long long)keys);
  if (keys && !d_hashes) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  HIPCHK(hipSetDevice(b->device));
  StageSlot* s = nullptr;
  if (n_desc) {  // the tables' room first: a failure here leaves the round as it was
    s = &b->slot[b->next_slot];
    if (int rc = harvest(b, *s)) return rc;
    const size_t need = (size_t)n_desc * sizeof(ScatterDesc) + ((size_t)n_desc + 1) * sizeof(uint32_t);
    if (need > s->cap) {
      free_slot(*s);
      const size_t cap = std::max<size_t>(need + need / 2, 1 << 16);
      if (hipHostMalloc((void**)&s->h, cap, hipHostMallocDefault) != hipSuccess || hipMalloc((void**)&s->d, cap) != hipSuccess) {
        (void)hipGetLastError();
        free_slot(*s);
        return kmcpg_fail(KMCPG_ENOMEM, "no room for the descriptor table of %u lists", n_desc);
      }
      s->cap = cap;
    }
  }
  b->st.scatter_calls++;
  uint32_t at = 0, slices = 0;
  ScatterDesc* desc = s ? (ScatterDesc*)s->h : nullptr;
  uint32_t* sbase = s ? (uint32_t*)(s->h + (size_t)n_desc * sizeof(ScatterDesc)) : nullptr;
  for (uint32_t i = 0; i < n_lists; i++) {
    const uint32_t c = cols[i];
    if (c == UINT32_MAX) {
      b->st.lists_skipped++;
      continue;
    }
    const uint32_t bi = b->block_of_col[c];
    if (bi == UINT32_MAX) continue;  // an empty column: in no block, nothing to scatter
    if (b->round_of_block[bi] != b->open_round) {
      b->st.lists_skipped++;
      continue;
    }
    b->scattered[c] = 1;
    const PlanBlock& pb = b->plan.blocks[bi];
    const uint64_t n = koff[i + 1] - koff[i];
    desc[at] = ScatterDesc{b->d_matrix[bi], pb.num_sigs, fastmod_magic(pb.num_sigs), koff[i], n, pb.row_bytes, b->pos_of_col[c]};
    sbase[at] = slices;
    slices += (uint32_t)((n + BS_SLICE_KEYS - 1) / BS_SLICE_KEYS);
    at++;
  }
  if (!n_desc) return 0;
  sbase[at] = slices;
  hipStream_t st = (hipStream_t)stream;
  const size_t bytes = (size_t)n_desc * sizeof(ScatterDesc) + ((size_t)n_desc + 1) * sizeof(uint32_t);
  HIPCHK(hipMemcpyAsync(s->d, s->h, bytes, hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(s->start, st));
  launch_build_scatter_lists((const ScatterDesc*)s->d, (const uint32_t*)(s->d + (size_t)n_desc * sizeof(ScatterDesc)), n_desc, slices,
                             b->cfg.build.num_hashes, d_hashes, st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(s->stop, st));
  s->pending = true;
  b->next_slot ^= 1;
  b->st.scatter_launches++;
  b->st.keys_scattered += keys;
  return 0;
}

extern "C" int kmcpg_builder_end_round(kmcpg_builder* b, const char* out_dir) {
  if (!b || !out_dir) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(b->mu);
  if (b->state != B_ROUND_OPEN) return out_of_order(b, "kmcpg_builder_end_round");
  const uint32_t round = b->open_round;
  uint64_t max_bytes = 0;
  for (size_t bi = 0; bi < b->plan.blocks.size(); bi++) {
    if (b->round_of_block[bi] != round) continue;
    for (uint32_t c : b->plan.blocks[bi].cols)
      if (!b->scattered[c])
        return kmcpg_fail(KMCPG_EINVAL, "column %u (%s) of block %zu was not scattered in round %u: kmcpg_builder_scatter_device expected", c,
                          b->names[c].c_str(), bi + 1, round);
    max_bytes = std::max(max_bytes, b->plan.blocks[bi].matrix_bytes);
  }
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  for (auto& s : b->slot)
    if (int rc = harvest(b, s)) return rc;
  const std::string dir = std::string(out_dir) + "/R001";
  if (plan_mkdirs(dir) != 0) return kmcpg_fail(KMCPG_EIO, "cannot create %s: %s", dir.c_str(), strerror(errno));
  // rows come down through one page-locked buffer in pieces of at most 256 MB (as kmcpg_save_db writes a resident block)
  const uint64_t piece = std::min<uint64_t>(std::max<uint64_t>(max_bytes, 1), 256ull << 20);
  uint8_t* host = nullptr;
  if (hipHostMalloc((void**)&host, piece, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return kmcpg_fail(KMCPG_ENOMEM, "no page-locked buffer of %llu bytes to write the blocks through", (unsigned long long)piece);
  }
  int rc = 0;
  for (size_t bi = 0; bi < b->plan.blocks.size() && rc == 0; bi++) {
    if (b->round_of_block[bi] != round) continue;
    const PlanBlock& pb = b->plan.blocks[bi];
    const std::string path = dir + "/" + block_file_name(bi);
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) {
      rc = kmcpg_fail(KMCPG_EIO, "cannot write %s: %s", path.c_str(), strerror(errno));
      break;
    }
    write_uniki_header(f, b->cfg.build, b->cols.data(), pb);
    for (uint64_t at = 0; at < pb.matrix_bytes && rc == 0; at += piece) {
      const uint64_t n = std::min(piece, pb.matrix_bytes - at);
      const hipError_t e = hipMemcpy(host, b->d_matrix[bi] + at, n, hipMemcpyDeviceToHost);
      if (e != hipSuccess) rc = kmcpg_fail(KMCPG_EDEVICE, "copy of block %zu to the host failed: %s", bi + 1, hipGetErrorString(e));
      else if (fwrite(host, 1, n, f) != n) rc = kmcpg_fail(KMCPG_EIO, "short write on %s", path.c_str());
    }
    if (fclose(f) != 0 && rc == 0) rc = kmcpg_fail(KMCPG_EIO, "short write on %s", path.c_str());
  }
  (void)hipHostFree(host);
  if (rc) return rc;  // the round stays open: end_round may be tried again
  free_matrices(b);
  b->round_done[round] = 1;
  b->st.rounds_done++;
  b->state = B_PLANNED;
  return 0;
}

extern "C" int kmcpg_builder_finish(kmcpg_builder* b, const char* out_dir) {
  if (!b || !out_dir) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(b->mu);
  if (b->state != B_PLANNED) return out_of_order(b, "kmcpg_builder_finish");
  for (uint32_t r = 0; r < b->n_rounds; r++)
    if (!b->round_done[r]) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_builder_finish out of order: round %u was never built, kmcpg_builder_begin_round expected", r);
  const std::string dir = std::string(out_dir) + "/R001";
  if (plan_mkdirs(dir) != 0) return kmcpg_fail(KMCPG_EIO, "cannot create %s: %s", dir.c_str(), strerror(errno));
  if (!write_db_yml(dir, b->cfg.build, (uint32_t)b->cols.size(), b->plan)) return kmcpg_fail(KMCPG_EIO, "cannot write %s/__db.yml", dir.c_str());
  write_name_mapping(dir, b->cols.data(), (uint32_t)b->cols.size());
  b->state = B_FINISHED;
  return 0;
}

extern "C" int kmcpg_builder_info(kmcpg_builder* b, kmcpg_builder_stats* out) {
  if (!b || !out) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(b->mu);
  if (b->device >= 0) {
    HIPCHK(hipSetDevice(b->device));
    for (auto& s : b->slot)
      if (int rc = harvest(b, s)) return rc;
  }
  *out = b->st;
  return 0;
}
