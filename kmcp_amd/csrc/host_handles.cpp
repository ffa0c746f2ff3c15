// host_handles.cpp — the handles that are more than one resident index: the in-process multi-GPU handle (kmcpg_open_devices: one shard per
// device, every batch to all of them) and the paged handle (kmcpg_open_paged: an index larger than HBM, searched one shard after the other
// on one GPU, search_paged).  At the end, the bench / parity entries that plant k-mers and read rows back.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "exchange.hpp"
#include "kernels.hpp"
#include "lane.hpp"

namespace kmcpg {

// A database larger than the HBM at hand (the reference reads any size through mmap / --low-mem, util-db-search.go:1238-1280,
// :6975-7335): the batch is searched against one shard of the index after the other on the same GPU — make shard r resident
// (kmcpg_open with shard r of S), K1 + K2, keep the hit tuples, drop it, next shard — and the concatenated hit lists are
// finalized once, exactly as the lists of S GPUs would be.  The shard searched last stays resident and is the first one of
// the next batch, so a batch costs S - 1 uploads: the larger the batch, the smaller their share.
int search_paged(kmcpg_db* front, const HostBatch& b, const kmcpg_params& p, kmcpg_ticket* t) {
  const uint32_t n = b.n;
  std::lock_guard<std::mutex> g(front->paged_mu);
  t->paged = true;
  t->hits.clear();
  t->qk.assign(n, 0);
  t->ql.assign(n, 0);
  if (n == 0) return 0;
  uint64_t maxlen = 0;  // (stage() below refuses a read that is too long)
  if (int rc = check_offsets(b, &maxlen)) return rc;
  // retries (--try-se, smaller k) read the batch again after kmcpg_submit has returned the caller's buffers
  t->seqs.assign(b.seqs, b.seqs + b.offs[n]);
  t->offs.assign(b.offs, b.offs + n + 1);
  if (b.seqs2) {
    t->seqs2.assign(b.seqs2, b.seqs2 + b.offs2[n]);
    t->offs2.assign(b.offs2, b.offs2 + n + 1);
  }
  t->S[0] = t->seqs.data();
  t->O[0] = t->offs.data();
  t->S[1] = b.seqs2 ? t->seqs2.data() : nullptr;
  t->O[1] = b.seqs2 ? t->offs2.data() : nullptr;
  const int S = front->paged_passes;
  const int first = front->paged_rank >= 0 ? front->paged_rank : 0;
  for (int i = 0; i < S; i++) {
    const int r = (first + i) % S;
    if (!front->paged_resident || front->paged_rank != r) {
      if (front->paged_resident) {
        int rc = kmcpg_close(front->paged_resident);
        front->paged_resident = nullptr;
        front->paged_rank = -1;
        if (rc) return rc;
      }
      kmcpg_opts so{front->paged_device, r, S, 0};
      kmcpg_db* sh = nullptr;
      int rc = open_like(front, &so, &sh);  // (the front has parsed every header already)
      if (rc) return kmcpg_fail(rc, "pass %d of %d: %s", r + 1, S, std::string(kmcpg_err_ref()).c_str());
      front->paged_resident = sh;
      front->paged_rank = r;
      front->paged_uploads++;
    }
    kmcpg_db* sh = front->paged_resident;
    if (sh->info.n_blocks_local == 0) continue;
    AsyncState* A = nullptr;
    int rc = async_state(sh, &A);
    if (rc) return rc;
    Lane* L = acquire_lane(A, false, true);
    uint64_t cnt = 0;
    rc = stage(L, b);
    if (rc == 0) rc = enqueue(sh, A, L, p);
    if (rc == 0) rc = collect(sh, A, L, p, &cnt);
    if (rc == 0) {
      t->hits.insert(t->hits.end(), L->h_hits.p, L->h_hits.p + cnt);
      if (i == 0) {  // every shard generates the same k-mers
        memcpy(t->qk.data(), L->h_qk.p, (size_t)n * sizeof(int32_t));
        memcpy(t->ql.data(), L->h_ql.p, (size_t)n * sizeof(int32_t));
      }
    } else drain(A);
    release_lane(A, L, false);
    if (rc) return kmcpg_fail(rc, "pass %d of %d: %s", r + 1, S, std::string(kmcpg_err_ref()).c_str());
  }
  return 0;
}

namespace {
// closes the half-made front handle; the error text stays that of what failed
int close_failed(kmcpg_db* front, int rc) {
  keeping_error([&] { kmcpg_close(front); });
  return rc;
}
}  // namespace

}  // namespace kmcpg

using namespace kmcpg;

extern "C" int kmcpg_open_devices(const char* db_dir, const int32_t* devices, int32_t n_devices, kmcpg_db** out) {
  if (!db_dir || !devices || !out || n_devices < 1) return kmcpg_fail(KMCPG_EINVAL, "bad argument");
  *out = nullptr;
  kmcpg_opts mo{-1, 0, 1, 0};
  kmcpg_db* front = nullptr;
  int rc = kmcpg_open(db_dir, &mo, &front);  // metadata of every block: names, sizes, FPR table
  if (rc) return rc;
  front->info.n_blocks_local = 0;
  front->info.matrix_bytes_local = 0;
  front->info.row_bytes_sum_local = 0;
  for (int32_t i = 0; i < n_devices; i++) {
    kmcpg_opts so{devices[i], i, n_devices, 0};
    kmcpg_db* sh = nullptr;
    rc = open_like(front, &so, &sh);  // (the headers were parsed once, by the front)
    if (rc) return close_failed(front, rc);
    front->shards.push_back(sh);
    front->info.n_blocks_local += sh->info.n_blocks_local;
    front->info.matrix_bytes_local += sh->info.matrix_bytes_local;
    front->info.row_bytes_sum_local += sh->info.row_bytes_sum_local;
  }
  // the exchange step: RCCL gather of the hit lists onto the first GPU when the devices allow it, host merge otherwise
  front->exchange = exchange_create(std::vector<int>(devices, devices + n_devices), &front->exchange_why);
  if (front->exchange)
    for (kmcpg_db* sh : front->shards) {
      AsyncState* A = nullptr;
      rc = async_state(sh, &A);
      if (rc) return close_failed(front, rc);
      A->hits_stay_on_device = true;
    }
  *out = front;
  return 0;
}

extern "C" const char* kmcpg_exchange_info(const kmcpg_db* db) {
  if (!db) return "";
  if (db->exchange) return exchange_note(db->exchange);
  static thread_local std::string s;
  s = db->shards.empty() ? "single device: no exchange step" : "host merge of the shards' hit lists (" + db->exchange_why + ")";
  return s.c_str();
}

extern "C" int kmcpg_open_paged(const char* db_dir, int32_t device, int32_t passes, kmcpg_db** out) {
  if (!db_dir || !out || passes < 0) return kmcpg_fail(KMCPG_EINVAL, "bad argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return kmcpg_fail(KMCPG_EDEVICE, "no HIP device available: libkmcpgpu has no CPU fallback");
  if (device < 0 || device >= ndev) return kmcpg_fail(KMCPG_EINVAL, "device %d out of range (%d devices)", device, ndev);
  kmcpg_opts mo{-1, 0, 1, 0};
  kmcpg_db* front = nullptr;
  int rc = kmcpg_open(db_dir, &mo, &front);  // metadata of every block: names, sizes, FPR table
  if (rc) return rc;
  uint64_t largest = 0, free_b = 0, reserve = 0;
  const int fit = plan_passes(front, device, &largest, &free_b, &reserve);
  if (passes == 0) passes = fit;
  if (fit == 0 || passes < fit) {
    kmcpg_close(front);
    if (fit == 0)
      return kmcpg_fail(KMCPG_ENOMEM, "index does not fit in HBM even one block at a time: the largest block needs %.2f GB, %.2f GB free on device %d", largest / 1e9,
                        free_b / 1e9, device);
    return kmcpg_fail(KMCPG_ENOMEM, "%d pass(es) do not fit in HBM (%.2f GB free on device %d): at least %d are needed", passes, free_b / 1e9, device, fit);
  }
  if (passes > (int)std::max<size_t>(1, front->blocks.size())) passes = (int)std::max<size_t>(1, front->blocks.size());
  if (passes == 1) {  // it fits after all: an ordinary resident handle
    kmcpg_close(front);
    kmcpg_opts so{device, 0, 1, 0};
    return kmcpg_open(db_dir, &so, out);
  }
  front->paged_passes = passes;
  front->paged_device = device;
  // what stays free beside the largest shard of the tightest partition that fits (>= the reserve plan_passes asked for; more
  // passes than needed leave more than this: the hint stays on the safe side)
  front->paged_reserve = std::max<uint64_t>(reserve, free_b > largest ? free_b - largest : 0);
  front->info.n_blocks_local = front->info.n_blocks;
  front->info.matrix_bytes_local = front->info.matrix_bytes;
  *out = front;
  return 0;
}

extern "C" int kmcpg_paged_info(const kmcpg_db* db, int32_t* passes, uint64_t* uploads) {
  if (!db) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (passes) *passes = db->paged_passes;
  if (uploads) *uploads = db->paged_uploads;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// bench / parity support
// ------------------------------------------------------------------------------------------------
extern "C" int kmcpg_plant(kmcpg_db* db, uint32_t col, const uint64_t* hashes, uint64_t n) {
  if (!db || (!hashes && n)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (col >= db->col_block.size()) return kmcpg_fail(KMCPG_EINVAL, "column out of range");
  const BlockMeta& b = db->blocks[db->col_block[col]];
  if (!b.local || n == 0) return 0;
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  DevBuf<uint64_t> d;  // released on every path
  if (d.ensure(n)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
  hipError_t e = hipMemcpy(d.p, hashes, n * sizeof(uint64_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    launch_plant(db->h_blockdev[(size_t)b.local_idx], col - b.col_base, db->info.num_hashes, d.p, n, nullptr);
    e = hipDeviceSynchronize();
  }
  d.release();
  if (e != hipSuccess) return kmcpg_fail(KMCPG_EDEVICE, "planting: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int kmcpg_read_rows(kmcpg_db* db, uint32_t block, const uint64_t* row_idx, uint64_t n_rows, uint8_t* out) {
  if (!db || block >= db->blocks.size() || (!row_idx && n_rows) || (!out && n_rows)) return kmcpg_fail(KMCPG_EINVAL, "bad argument");
  const BlockMeta& b = db->blocks[block];
  if (!b.local) return kmcpg_fail(KMCPG_EINVAL, "block %u is not resident on this rank", block);
  for (uint64_t i = 0; i < n_rows; i++)
    if (row_idx[i] >= b.h.num_sigs) return kmcpg_fail(KMCPG_EINVAL, "row out of range");
  if (n_rows == 0) return 0;
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  DevBuf<uint64_t> d_idx;  // released on every path
  DevBuf<uint8_t> d_out;
  if (d_idx.ensure(n_rows) || d_out.ensure(n_rows * b.h.row_bytes)) {
    d_idx.release();
    d_out.release();
    return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
  }
  hipError_t e = hipMemcpy(d_idx.p, row_idx, n_rows * sizeof(uint64_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    launch_gather_rows(b.d_rows, b.stride, b.h.row_bytes, d_idx.p, 0, n_rows, d_out.p, nullptr);
    e = hipMemcpy(out, d_out.p, n_rows * b.h.row_bytes, hipMemcpyDeviceToHost);
  }
  d_idx.release();
  d_out.release();
  if (e != hipSuccess) return kmcpg_fail(KMCPG_EDEVICE, "reading rows back: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int kmcpg_read_row_range(kmcpg_db* db, uint32_t block, uint64_t first_row, uint64_t n_rows, uint8_t* out) {
  if (!db || block >= db->blocks.size() || (!out && n_rows)) return kmcpg_fail(KMCPG_EINVAL, "bad argument");
  const BlockMeta& b = db->blocks[block];
  if (!b.local) return kmcpg_fail(KMCPG_EINVAL, "block %u is not resident on this rank", block);
  if (first_row > b.h.num_sigs || n_rows > b.h.num_sigs - first_row) return kmcpg_fail(KMCPG_EINVAL, "row out of range");
  if (n_rows == 0) return 0;
  std::lock_guard<std::mutex> g(db->mu);
  KMCPG_USE_DEVICE(db);
  if (b.h.row_bytes >= 512 && b.h.row_bytes % 16 == 0) {  // wide rows of a DMA-friendly width: one strided copy (782-byte rows took 23 s for 2.7 GB this way)
    HIPCHK(hipMemcpy2D(out, b.h.row_bytes, b.d_rows + first_row * b.stride, b.stride, b.h.row_bytes, n_rows, hipMemcpyDeviceToHost));
    return 0;
  }
  // narrow rows (a 2-D copy would move them one by one): packed on the device first
  const uint64_t chunk = std::max<uint64_t>(1, (64ull << 20) / b.h.row_bytes);
  uint8_t* d_out = nullptr;
  HIPCHK(hipMalloc((void**)&d_out, std::min(chunk, n_rows) * b.h.row_bytes));
  hipError_t e = hipSuccess;
  for (uint64_t r0 = 0; r0 < n_rows && e == hipSuccess; r0 += chunk) {
    const uint64_t nr = std::min(chunk, n_rows - r0);
    launch_gather_rows(b.d_rows, b.stride, b.h.row_bytes, nullptr, first_row + r0, nr, d_out, nullptr);
    e = hipMemcpy(out + r0 * b.h.row_bytes, d_out, nr * b.h.row_bytes, hipMemcpyDeviceToHost);
  }
  (void)hipFree(d_out);
  if (e != hipSuccess) return kmcpg_fail(KMCPG_EDEVICE, "reading rows back: %s", hipGetErrorString(e));
  return 0;
}
