// host_pack.cpp — packed queries for callers (kmcp_gpu.h): the 2-bit packer and its inverse for hosts (kmcpg_pack2 / kmcpg_unpack2),
// page-locked memory whose codes are uploaded without a staging copy (kmcpg_host_alloc / kmcpg_host_free), and the entry that takes
// codes instead of text (kmcpg_submit_packed).  The lane's side of a packed batch is stage_packed (lane.cpp).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "lane.hpp"
#include "pack2.hpp"

using namespace kmcpg;

extern "C" int kmcpg_pack2(const uint8_t* seq, uint64_t n, uint64_t pos, uint8_t* codes, kmcpg_exc_run* exc, uint64_t exc_cap, uint64_t* n_exc) {
  if ((n && (!seq || !codes)) || !n_exc || (exc_cap && !exc)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  static_assert(sizeof(kmcpg_exc_run) == sizeof(PackRun), "one layout");
  static thread_local std::vector<PackRun> runs;
  runs.clear();
  pack2_append(seq, (size_t)n, codes, pos, runs);
  const uint64_t have = *n_exc, total = have + runs.size();
  // a run that continues the caller's last one (a gap of N's across two calls) is joined with it
  size_t first = 0;
  bool join = false;
  if (have && have <= exc_cap && !runs.empty()) {
    const kmcpg_exc_run& l = exc[have - 1];
    join = l.byte == runs[0].byte && l.pos + l.len == runs[0].pos && (uint64_t)l.len + runs[0].len <= 0xffffffffu;
  }
  if (join) first = 1;
  const uint64_t need = have + (runs.size() - first);
  if (need > exc_cap) {  // nothing of the caller's list has been touched: the call can be repeated with more room
    *n_exc = total;
    return kmcpg_fail(KMCPG_ENOMEM, "kmcpg_pack2: room for %llu exception runs, %llu needed", (unsigned long long)exc_cap, (unsigned long long)total);
  }
  if (join) exc[have - 1].len += runs[0].len;
  for (size_t i = first; i < runs.size(); i++) exc[have + (i - first)] = kmcpg_exc_run{runs[i].pos, runs[i].len, runs[i].byte};
  *n_exc = need;
  return 0;
}

extern "C" int kmcpg_host_alloc(uint64_t bytes, void** out) {
  if (!out) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return kmcpg_fail(KMCPG_EDEVICE, "no HIP device available: libkmcpgpu has no CPU fallback");
  if (hipHostMalloc(out, (size_t)std::max<uint64_t>(bytes, 64), hipHostMallocPortable) != hipSuccess) {
    (void)hipGetLastError();
    *out = nullptr;
    return kmcpg_fail(KMCPG_ENOMEM, "hipHostMalloc of %llu bytes failed", (unsigned long long)bytes);
  }
  return 0;
}

extern "C" int kmcpg_host_free(void* p) {
  if (p && hipHostFree(p) != hipSuccess) {
    (void)hipGetLastError();
    return kmcpg_fail(KMCPG_EINVAL, "not a pointer from kmcpg_host_alloc");
  }
  return 0;
}

extern "C" int kmcpg_unpack2(const uint8_t* codes, uint64_t n_bases, const kmcpg_exc_run* exc, uint64_t n_exc, uint8_t* out) {
  if ((n_bases && (!codes || !out)) || (n_exc && !exc)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  static const char lut[4] = {'A', 'C', 'T', 'G'};
  for (uint64_t j = 0; j < n_bases; j++) out[j] = (uint8_t)lut[(codes[j >> 2] >> (2 * (j & 3))) & 3];
  if (int rc = check_exc_runs(exc, n_exc, n_bases)) return rc;
  for (uint64_t i = 0; i < n_exc; i++) memset(out + exc[i].pos, (int)exc[i].byte, exc[i].len);
  return 0;
}

extern "C" int kmcpg_submit_packed(kmcpg_db* db, const uint8_t* codes, const uint64_t* offs, const kmcpg_exc_run* exc, uint64_t n_exc, uint32_t n_reads,
                                   const kmcpg_params* params, kmcpg_ticket** out) {
  if (!db || !out || (n_reads && (!codes || !offs)) || (n_exc && !exc)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  *out = nullptr;
  if (int rc = set_refuse_entry(db, "kmcpg_submit_packed")) return rc;
  kmcpg_params p;
  if (int rc = submit_handle(db, params, &p)) return rc;
  // handles that read the batch's text again (rereads_text, the passes of a paged index) get text
  if (db->paged_passes > 0 || rereads_text(db, p)) {
    const uint64_t tb = n_reads ? offs[n_reads] : 0;
    std::vector<uint8_t, NoInitAlloc<uint8_t>> text((size_t)tb + 16);
    if (int rc = kmcpg_unpack2(codes, tb, exc, n_exc, text.data())) return rc;
    return submit_impl(db, HostBatch{text.data(), offs, nullptr, nullptr, n_reads}, p, false, false, out);
  }
  const PackedIn in{codes, exc, n_exc};
  return submit_impl(db, HostBatch{nullptr, offs, nullptr, nullptr, n_reads}, p, false, false, out, &in);
}
