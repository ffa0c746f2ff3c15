// sort_segments.hip — sort + unique of MANY k-mer lists at once: the chunk lists of a batch of reference genomes (`kmcp compute`,
// kmcp/cmd/compute.go:809-826: sortutil.Uint64s, then duplicates removed), for kmcpg_sketch_genomes (sketch.cpp).
//
// k1_dedup.hip sorts a list on one workgroup and sort_huge.hip sorts ONE long list device-wide, called once per list; a batch of genomes
// cut into chunks is thousands of lists of 10^4 .. 10^6 hashes, and a device-wide sort per list is ~26 launches that each fill a fraction
// of the chip.  Here the whole batch goes through one set of launches whose number depends on the key width alone:
//
//   * a segmented LSD radix sort, 8 bits per pass.  Segments are kept apart by the LAYOUT of the histogram table, not by a wider key: a
//     wave owns up to 4096 consecutive keys of ONE segment (segment s has ceil(n_s / 4096) waves, numbered from wbase[s]), writes its
//     256 digit counts to table[256 wbase[s] + digit * waves_s + wave in segment], and ONE exclusive scan over the table in that order —
//     segment, then digit, then wave — gives every (wave, digit) its destination in a compact buffer where segment s starts at the sum of
//     the sizes of the segments before it.  A pass is stable inside a segment and never moves a key out of it; no key carries a segment
//     id, no pass is spent on one.  (The alternative, the id as leading digits of a wider key, costs 12-byte keys and ceil(log2(chunks)
//     / 8) more passes, and the launch count would depend on the number of chunks.)
//   * hashes of a FracMinHash sketch are <= maxHash: only the passes below its highest set bit run (DedupArgs::key_shift, k1_dedup.hip).
//   * the first pass reads the lists where the k-mer kernels left them (with gaps, one part per k-mer size) and writes them compact.
//   * unique: heads per wave -> scan -> ordered scatter; a segment's first key is a head whatever precedes it.  koff[s] is the scanned
//     head count at the segment's first wave.
//
// Nothing is read back between the launches: the waves of the grid (an upper bound the host derives from the chunk lengths) look up
// their segment in wbase[] with a binary search, and waves past the last one leave at once.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_utils.hpp"
#include "sort_segments.hpp"

namespace kmcpg {

namespace {
constexpr uint32_t SS_KEYS = SEGSORT_KEYS_PER_WAVE;
constexpr int SS_ROUNDS = SS_KEYS / 64;
constexpr uint32_t SS_SCAN_TILE = 4096;

// what a wave works on: its segment, its place in it, where the segment's keys are
struct WaveJob {
  uint32_t seg, wl, nw_s;  // segment, wave in segment, waves of the segment
  uint32_t n_s;            // keys of the segment
  uint32_t c0;             // first key of the segment in the compact buffers
  uint32_t wb;             // first wave of the segment
};

__device__ __forceinline__ bool wave_job(const uint32_t* __restrict__ wbase, const uint32_t* __restrict__ cbase, uint32_t n_segs, uint32_t w, WaveJob* j) {
  if (w >= wbase[n_segs]) return false;
  uint32_t lo = 0, hi = n_segs;  // the last segment with wbase[s] <= w (segments without keys have no waves and are never found)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (wbase[mid] <= w) lo = mid;
    else hi = mid;
  }
  j->seg = lo;
  j->wb = wbase[lo];
  j->wl = w - j->wb;
  j->nw_s = wbase[lo + 1] - j->wb;
  j->c0 = cbase[lo];
  j->n_s = cbase[lo + 1] - j->c0;
  return true;
}

// key i of segment s as the k-mer kernels left it: part p (one per k-mer size) holds cnt[p][s] keys at in[p * part_stride + in_off[s] ...]
__device__ __forceinline__ uint64_t raw_key(const SegSortIn& in, uint32_t s, uint32_t i) {
  uint32_t p = 0;
  for (; p + 1 < (uint32_t)in.parts; p++) {
    const uint32_t c = (uint32_t)in.cnt[(size_t)p * in.cnt_stride + s];
    if (i < c) break;
    i -= c;
  }
  return in.keys[(size_t)p * in.part_stride + in.in_off[s] + i];
}

// sizes of the segments (all parts together) and their waves, one thread per segment; entry n_segs = 0 for the exclusive scans
__global__ void __launch_bounds__(256) k_ss_sizes(const SegSortIn in, uint32_t* __restrict__ cbase, uint32_t* __restrict__ wbase) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > in.n_segs) return;
  uint32_t n = 0;
  if (s < in.n_segs)
    for (int p = 0; p < in.parts; p++) n += (uint32_t)in.cnt[(size_t)p * in.cnt_stride + s];
  cbase[s] = n;
  wbase[s] = (n + SS_KEYS - 1) / SS_KEYS;
}

// ---- exclusive scans of u32 arrays in place ----
__device__ __forceinline__ uint32_t wg_exclusive_scan_256(uint32_t v, uint32_t* lds /*[4]*/, uint32_t* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t u = __shfl_up(inc, off);
    if (lane >= off) inc += u;
  }
  if (lane == 63) lds[wv] = inc;
  __syncthreads();
  uint32_t base = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 4; w++) {
    const uint32_t t = lds[w];
    if (w < wv) base += t;
    all += t;
  }
  __syncthreads();
  if (total) *total = all;
  return base + inc - v;
}

__global__ void __launch_bounds__(256) k_ss_tile_sums(const uint32_t* __restrict__ data, uint64_t total, uint32_t* __restrict__ tile_sum) {
  __shared__ uint32_t lds[4];
  const uint64_t base = (uint64_t)blockIdx.x * SS_SCAN_TILE + (uint64_t)threadIdx.x * 16;
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < 16; i++)
    if (base + i < total) s += data[base + i];
  uint32_t all = 0;
  (void)wg_exclusive_scan_256(s, lds, &all);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
}

// one workgroup: the tile sums, and the two per-segment arrays (both in one launch: blockIdx.x picks the array)
struct ScanOne {
  uint32_t* data[2];
  uint32_t total[2];
};
__global__ void __launch_bounds__(1024) k_ss_scan_one(const ScanOne a) {
  __shared__ uint32_t part[1024];
  uint32_t* __restrict__ data = a.data[blockIdx.x];
  const uint32_t total = a.total[blockIdx.x];
  const uint32_t t = threadIdx.x;
  const uint32_t seg = (total + 1023) / 1024;
  const uint64_t lo0 = (uint64_t)t * seg, lo = lo0 < total ? lo0 : total, hi = lo + seg < total ? lo + seg : total;
  uint32_t s = 0;
  for (uint64_t i = lo; i < hi; i++) s += data[i];
  part[t] = s;
  __syncthreads();
  for (uint32_t off = 1; off < 1024; off <<= 1) {
    const uint32_t v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t run = part[t] - s;
  for (uint64_t i = lo; i < hi; i++) {
    const uint32_t v = data[i];
    data[i] = run;
    run += v;
  }
}

__global__ void __launch_bounds__(256) k_ss_scan_tiles(uint32_t* __restrict__ data, uint64_t total, const uint32_t* __restrict__ tile_base) {
  __shared__ uint32_t lds[4];
  const uint64_t base = (uint64_t)blockIdx.x * SS_SCAN_TILE + (uint64_t)threadIdx.x * 16;
  uint32_t v[16], s = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    v[i] = base + i < total ? data[base + i] : 0;
    s += v[i];
  }
  uint32_t run = tile_base[blockIdx.x] + wg_exclusive_scan_256(s, lds, nullptr);
#pragma unroll
  for (int i = 0; i < 16; i++) {
    if (base + i < total) data[base + i] = run;
    run += v[i];
  }
}

// ---- the radix passes; FIRST = the keys are read through raw_key ----
template <bool FIRST>
__global__ void __launch_bounds__(256) k_ss_hist(const SegSortIn in, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ wbase,
                                                 const uint32_t* __restrict__ cbase, int shift, uint32_t* __restrict__ hist) {
  __shared__ uint32_t cnt[4][256];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t w = blockIdx.x * 4 + wv;
  for (int d = lane; d < 256; d += 64) cnt[wv][d] = 0;
  wave_lds_fence();
  WaveJob j;
  if (!wave_job(wbase, cbase, in.n_segs, w, &j)) return;
  const uint32_t i0 = j.wl * SS_KEYS;
  for (int r = 0; r < SS_ROUNDS; r++) {
    const uint32_t i = i0 + (uint32_t)r * 64 + lane;
    if (i < j.n_s) {
      const uint64_t key = FIRST ? raw_key(in, j.seg, i) : keys[(size_t)j.c0 + i];
      atomicAdd(&cnt[wv][(uint32_t)(key >> shift) & 255u], 1u);
    }
  }
  wave_lds_fence();
  uint32_t* __restrict__ out = hist + (size_t)256 * j.wb + j.wl;
  for (int d = lane; d < 256; d += 64) out[(size_t)d * j.nw_s] = cnt[wv][d];
}

template <bool FIRST>
__global__ void __launch_bounds__(256) k_ss_scatter(const SegSortIn in, const uint64_t* __restrict__ keys, uint64_t* __restrict__ out,
                                                    const uint32_t* __restrict__ wbase, const uint32_t* __restrict__ cbase, int shift,
                                                    const uint32_t* __restrict__ hist) {
  __shared__ uint32_t run[4][256];  // next free destination of every digit for this wave
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t w = blockIdx.x * 4 + wv;
  WaveJob j;
  if (!wave_job(wbase, cbase, in.n_segs, w, &j)) return;
  const uint32_t* __restrict__ h = hist + (size_t)256 * j.wb + j.wl;
  for (int d = lane; d < 256; d += 64) run[wv][d] = h[(size_t)d * j.nw_s];
  wave_lds_fence();
  const uint32_t i0 = j.wl * SS_KEYS;
  const uint64_t below = (1ULL << lane) - 1ULL;
  for (int r = 0; r < SS_ROUNDS; r++) {
    const uint32_t i = i0 + (uint32_t)r * 64 + lane;
    const bool valid = i < j.n_s;
    const uint64_t key = valid ? (FIRST ? raw_key(in, j.seg, i) : keys[(size_t)j.c0 + i]) : 0;
    const uint32_t d = (uint32_t)(key >> shift) & 255u;
    uint64_t same = __ballot(valid);  // lanes holding a key with my digit
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const uint64_t bal = __ballot(valid && ((d >> b) & 1u));
      same &= ((d >> b) & 1u) ? bal : ~bal;
    }
    uint32_t dst = 0;
    if (valid) dst = run[wv][d] + (uint32_t)__popcll(same & below);
    wave_lds_fence();  // every lane has read its digit's counter before the group leaders move it on
    if (valid) {
      out[dst] = key;  // dst < cbase[n_segs]: the scanned table places every key inside its own segment
      if ((same & below) == 0) run[wv][d] += (uint32_t)__popcll(same);
    }
    wave_lds_fence();
  }
}

// ---- unique ----
__global__ void __launch_bounds__(256) k_ss_uq_count(uint32_t n_segs, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ wbase,
                                                     const uint32_t* __restrict__ cbase, uint32_t* __restrict__ wave_cnt, uint32_t max_waves) {
  const int lane = threadIdx.x & 63;
  const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w > max_waves) return;
  WaveJob j;
  uint32_t c = 0;
  if (wave_job(wbase, cbase, n_segs, w, &j)) {
    const uint64_t* __restrict__ k = keys + j.c0;
    const uint32_t i0 = j.wl * SS_KEYS;
    for (int r = 0; r < SS_ROUNDS; r++) {
      const uint32_t i = i0 + (uint32_t)r * 64 + lane;
      const bool head = i < j.n_s && (i == 0 || k[i] != k[i - 1]);
      c += (uint32_t)__popcll(__ballot(head));
    }
  }
  if (lane == 0) wave_cnt[w] = c;  // zero past the last wave: the scan runs over max_waves + 1 entries
}

__global__ void __launch_bounds__(256) k_ss_uq_scatter(uint32_t n_segs, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ wbase,
                                                       const uint32_t* __restrict__ cbase, const uint32_t* __restrict__ wave_off,
                                                       uint64_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
  WaveJob j;
  if (!wave_job(wbase, cbase, n_segs, w, &j)) return;
  const uint64_t* __restrict__ k = keys + j.c0;
  const uint32_t i0 = j.wl * SS_KEYS;
  const uint64_t below = (1ULL << lane) - 1ULL;
  uint32_t run = wave_off[w];
  for (int r = 0; r < SS_ROUNDS; r++) {
    const uint32_t i = i0 + (uint32_t)r * 64 + lane;
    const uint64_t key = i < j.n_s ? k[i] : 0;
    const bool head = i < j.n_s && (i == 0 || key != k[i - 1]);
    const uint64_t heads = __ballot(head);
    if (head) out[run + (uint32_t)__popcll(heads & below)] = key;  // at most as many heads as keys: inside the compact buffer
    run += (uint32_t)__popcll(heads);
  }
}

// koff[s] = unique keys of the segments before s; koff[n_segs + 1] = the raw keys of the batch (for the launch record)
__global__ void __launch_bounds__(256) k_ss_koff(uint32_t n_segs, const uint32_t* __restrict__ wbase, const uint32_t* __restrict__ cbase,
                                                 const uint32_t* __restrict__ wave_off, uint64_t* __restrict__ koff) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s <= n_segs) koff[s] = wave_off[wbase[s]];
  if (s == n_segs) koff[n_segs + 1] = cbase[n_segs];
}

}  // namespace

size_t seg_sort_temp_words(uint32_t n_segs, uint32_t max_waves) {
  const size_t table = (size_t)256 * max_waves;
  // cbase, wbase | histogram table | per-wave head counts | tile sums of the largest scan
  return 2 * ((size_t)n_segs + 2) + table + ((size_t)max_waves + 2) + (table / SS_SCAN_TILE + 2) + 64;
}

int seg_sort_passes(int key_bits) { return key_bits <= 0 ? 0 : (key_bits + 7) / 8; }

int seg_sort_unique(const SegSortIn& in, uint64_t* a, uint64_t* b, uint32_t max_waves, int key_bits, uint32_t* temp, size_t temp_words, uint64_t* koff,
                    uint64_t** out, kmcpg_sketch_launch* rec, hipStream_t st) {
  if (in.parts < 1 || in.parts > 8 || key_bits < 0 || key_bits > 64) return -1;
  if (temp_words < seg_sort_temp_words(in.n_segs, max_waves)) return -1;
  const int passes = seg_sort_passes(key_bits);
  if (max_waves && !passes) return -1;  // key_bits == 0 with room for keys: every kept hash is > 0.  Refused before anything is enqueued
  uint32_t launches = 0;
#define SS_LAUNCH(kern, grid, block, ...)                          \
  do {                                                              \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, st, __VA_ARGS__); \
    launches++;                                                     \
  } while (0)
  const uint32_t ns1 = in.n_segs + 1;
  uint32_t* cbase = temp;
  uint32_t* wbase = cbase + ns1 + 1;
  uint32_t* hist = wbase + ns1 + 1;
  const size_t table = (size_t)256 * max_waves;
  uint32_t* wave_cnt = hist + table;      // max_waves + 1
  uint32_t* tile_sum = wave_cnt + max_waves + 2;
  const unsigned wgrid = (max_waves + 3) / 4;
  auto scan = [&](uint32_t* data, uint64_t total) {  // three launches whatever the size
    const unsigned tiles = (unsigned)((total + SS_SCAN_TILE - 1) / SS_SCAN_TILE);
    SS_LAUNCH(k_ss_tile_sums, tiles, 256, data, total, tile_sum);
    ScanOne one{{tile_sum, nullptr}, {tiles, 0}};
    SS_LAUNCH(k_ss_scan_one, 1, 1024, one);
    SS_LAUNCH(k_ss_scan_tiles, tiles, 256, data, total, tile_sum);
  };
  SS_LAUNCH(k_ss_sizes, (ns1 + 255) / 256, 256, in, cbase, wbase);
  {
    ScanOne two{{cbase, wbase}, {ns1, ns1}};
    SS_LAUNCH(k_ss_scan_one, 2, 1024, two);
  }
  const uint64_t* src = nullptr;  // pass 0 reads the raw lists
  uint64_t* dst = b;
  if (max_waves) {
    // max_waves is an upper bound: no wave writes the entries past 256 * wbase[n_segs].  They are zero for the scan of pass 0, which
    // leaves the number of raw keys in each of them; later passes scan those stale totals again (sums that may wrap).  Harmless: the
    // scan is exclusive and every real entry precedes them, so no real entry's offset depends on them, and the histogram and scatter
    // kernels read real entries only.
    if (hipMemsetAsync(hist, 0, table * sizeof(uint32_t), st) != hipSuccess) return -1;
    for (int p = 0; p < passes; p++) {
      if (p == 0) SS_LAUNCH((k_ss_hist<true>), wgrid, 256, in, src, wbase, cbase, 0, hist);
      else SS_LAUNCH((k_ss_hist<false>), wgrid, 256, in, src, wbase, cbase, p * 8, hist);
      scan(hist, table);
      if (p == 0) SS_LAUNCH((k_ss_scatter<true>), wgrid, 256, in, src, dst, wbase, cbase, 0, hist);
      else SS_LAUNCH((k_ss_scatter<false>), wgrid, 256, in, src, dst, wbase, cbase, p * 8, hist);
      src = dst;
      dst = dst == b ? a : b;
    }
    SS_LAUNCH(k_ss_uq_count, (max_waves + 1 + 3) / 4, 256, in.n_segs, src, wbase, cbase, wave_cnt, max_waves);
    scan(wave_cnt, (uint64_t)max_waves + 1);
    SS_LAUNCH(k_ss_uq_scatter, wgrid, 256, in.n_segs, src, wbase, cbase, wave_cnt, dst);
  } else {
    if (hipMemsetAsync(wave_cnt, 0, 2 * sizeof(uint32_t), st) != hipSuccess) return -1;
  }
  SS_LAUNCH(k_ss_koff, (ns1 + 255) / 256, 256, in.n_segs, wbase, cbase, wave_cnt, koff);
#undef SS_LAUNCH
  *out = dst;
  if (rec) {
    rec->kind = 0;
    rec->passes = passes;
    rec->segments = in.n_segs;
    rec->workgroups = wgrid;
    rec->launches = launches;
    rec->key_bits = key_bits;
    rec->keys = 0;  // known once koff is on the host (sketch.cpp)
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace kmcpg
