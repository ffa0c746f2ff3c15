// k1_reads.hip — K1, k-mers and sketches of reads: one wave per short read (k1_kmers<MODE>), one 1024-thread workgroup per long read with
// the prefix XORs of a tile in LDS (k1_kmers_wg<MODE>) or, when the halo does not fit, window scans over scratch arrays in global memory
// (k1_kmers_wg_global); and k1_seg_hash, the same LDS tiles over a segment of a genome.  Forms Short / Wg / WgGlobal of launch_k1
// (k1_kmers.hip) and the first kernel of SegHash.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "device_utils.hpp"
#include "k1_device.hpp"
#include "k1_launch.hpp"
#include "k1_plan.hpp"
#include "kernels.hpp"
#include "nthash.hpp"

namespace kmcpg {

__device__ __forceinline__ int hash_mate_scan(const uint8_t* __restrict__ s, int len, int k, const uint64_t* tab, bool scaled, uint64_t max_hash,
                                              uint64_t* __restrict__ out, int cnt, int lane) {
  const int npos = len - k + 1;
  if (npos <= 0) return cnt;  // ErrShortSeq => no k-mers (util-db-search.go:1060-1062)
  uint64_t cp = 0, cq = 0;
  WTile cur = wave_tile(s, len, 0, tab, cp, cq, lane);
  for (int base = 0; base < npos; base += 64) {
    const WTile nxt = wave_tile(s, len, base + 64, tab, cp, cq, lane);
    const uint64_t h = wave_hash(cur, nxt, k, lane);
    const bool keep = base + lane < npos && h != 0 && (!scaled || h <= max_hash);  // :1097-1103
    const uint64_t m = __ballot(keep);
    if (keep) out[cnt + __popcll(m & ((1ULL << lane) - 1ULL))] = h;
    cnt += __popcll(m);
    cur = nxt;
  }
  return cnt;
}

// all canonical k1-mer (and, if out2, k2-mer) hashes of s, uncompacted (input of the window sketches)
__device__ __forceinline__ void hash_positions_scan(const uint8_t* __restrict__ s, int len, int k1, uint64_t* __restrict__ out1, int k2,
                                                    uint64_t* __restrict__ out2, const uint64_t* tab, int lane) {
  const int n1 = len - k1 + 1, n2 = out2 ? len - k2 + 1 : 0;
  const int nmax = n1 > n2 ? n1 : n2;
  uint64_t cp = 0, cq = 0;
  WTile cur = wave_tile(s, len, 0, tab, cp, cq, lane);
  for (int base = 0; base < nmax; base += 64) {
    const WTile nxt = wave_tile(s, len, base + 64, tab, cp, cq, lane);
    const uint64_t h1 = wave_hash(cur, nxt, k1, lane);
    if (base + lane < n1) out1[base + lane] = h1;
    if (out2) {
      const uint64_t h2 = wave_hash(cur, nxt, k2, lane);
      if (base + lane < n2) out2[base + lane] = h2;
    }
    cur = nxt;
  }
}

// Fallback for k > 65 (the closed form evaluated per k-mer); kept hashes are compacted in order with a wave ballot.
__device__ __forceinline__ int hash_mate(const uint8_t* __restrict__ s, int len, int k, const uint64_t* tab, bool scaled,
                                         uint64_t max_hash, uint64_t* __restrict__ out, int cnt, int lane) {
  if (k <= K1_SCAN_MAX_K) return hash_mate_scan(s, len, k, tab, scaled, max_hash, out, cnt, lane);
  const int npos = len - k + 1;
  if (npos <= 0) return cnt;  // ErrShortSeq => no k-mers (util-db-search.go:1060-1062)
  for (int base = 0; base < npos; base += 64) {
    const int i = base + lane;
    const bool v = i < npos;
    uint64_t h = 0;
    if (v) {
      uint64_t f = 0, r = 0;
      for (int j = 0; j < k; j++) {
        f = rol1(f) ^ tab[s[i + j]];
        r = rol1(r) ^ tab[s[i + k - 1 - j] & 7];
      }
      h = f < r ? f : r;
    }
    const bool keep = v && h != 0 && (!scaled || h <= max_hash);  // :1097-1103
    const uint64_t m = __ballot(keep);
    if (keep) out[cnt + __popcll(m & ((1ULL << lane) - 1ULL))] = h;
    cnt += __popcll(m);
  }
  return cnt;
}

// all canonical kk-mer hashes of s, uncompacted (input of the window sketches)
__device__ __forceinline__ void hash_positions(const uint8_t* __restrict__ s, int len, int kk, const uint64_t* tab, uint64_t* __restrict__ out,
                                               int lane) {
  const int npos = len - kk + 1;
  for (int i = lane; i < npos; i += 64) {
    uint64_t f = 0, r = 0;
    for (int j = 0; j < kk; j++) {
      f = rol1(f) ^ tab[s[i + j]];
      r = rol1(r) ^ tab[s[i + kk - 1 - j] & 7];
    }
    out[i] = f < r ? f : r;
  }
}

__device__ __forceinline__ int argmin_left(const uint64_t* __restrict__ h, int b, int n) {
  int m = b;
  uint64_t mv = h[b];
#pragma unroll 4
  for (int i = b + 1; i < b + n; i++) {
    const uint64_t v = h[i];
    if (v < mv) {  // strict: the leftmost of equal values wins
      mv = v;
      m = i;
    }
  }
  return m;
}

// Closed Syncmer as bio/sketches emits it (NextSyncmer, call site util-db-search.go:1053,1068; semantics pinned by
// demo-searching/README.md:61-68): window of 2k-s-1 bases = 2(k-s) s-mers, m = leftmost minimal canonical s-mer;
// emit the k-mer starting at m if m-w0 < k-s, else the k-mer ending at m+s.  One emission per window.
__device__ __forceinline__ int syncmer_mate(const uint8_t* __restrict__ s, int len, int k, int sm, const uint64_t* tab, bool scaled,
                                            uint64_t max_hash, uint64_t* hk, uint64_t* hs, uint64_t* __restrict__ out, int cnt, int lane) {
  const int L = 2 * k - sm - 1;
  if (sm < 1 || sm > k || len < L || len < k) return cnt;  // ErrShortSeq
  if (k <= K1_SCAN_MAX_K) {
    hash_positions_scan(s, len, k, hk, sm, hs, tab, lane);
  } else {
    hash_positions(s, len, k, tab, hk, lane);
    hash_positions(s, len, sm, tab, hs, lane);
  }
  __threadfence_block();
  const int wsz = 2 * (k - sm);
  const int nw = wsz > 0 ? len - L + 1 : len - k + 1;  // s == k: every k-mer is its own window
  for (int base = 0; base < nw; base += 64) {
    const int w0 = base + lane;
    const bool v = w0 < nw;
    uint64_t h = 0;
    if (v) {
      int pos = w0;
      if (wsz > 0) {
        const int m = argmin_left(hs, w0, wsz);
        pos = (m - w0 < k - sm) ? m : m + sm - k;
      }
      h = hk[pos];
    }
    const bool keep = v && h != 0 && (!scaled || h <= max_hash);
    const uint64_t mk = __ballot(keep);
    if (keep) out[cnt + __popcll(mk & ((1ULL << lane) - 1ULL))] = h;
    cnt += __popcll(mk);
  }
  return cnt;
}

// Minimizer sketch (NextMinimizer, call site util-db-search.go:1055,1081): leftmost minimum of every window of w
// k-mers, emitted when its position changes.  (Parity unpinned: the reference holds no golden for this mode.)
__device__ __forceinline__ int minimizer_mate(const uint8_t* __restrict__ s, int len, int k, int w, const uint64_t* tab, bool scaled,
                                              uint64_t max_hash, uint64_t* hk, uint64_t* __restrict__ out, int cnt, int lane) {
  if (w < 1 || len < k + w - 1) return cnt;  // ErrShortSeq
  if (k <= K1_SCAN_MAX_K) hash_positions_scan(s, len, k, hk, 0, nullptr, tab, lane);
  else hash_positions(s, len, k, tab, hk, lane);
  __threadfence_block();
  const int nw = len - k + 1 - w + 1;
  for (int base = 0; base < nw; base += 64) {
    const int w0 = base + lane;
    const bool v = w0 < nw;
    int m = -1, pm = -2;
    if (v) {
      m = argmin_left(hk, w0, w);
      pm = w0 > 0 ? argmin_left(hk, w0 - 1, w) : -2;
    }
    const uint64_t h = (v && m != pm) ? hk[m] : 0;
    const bool keep = v && m != pm && h != 0 && (!scaled || h <= max_hash);
    const uint64_t mk = __ballot(keep);
    if (keep) out[cnt + __popcll(mk & ((1ULL << lane) - 1ULL))] = h;
    cnt += __popcll(mk);
  }
  return cnt;
}

__device__ __forceinline__ int sketch_mate(const K1Args& a, int mode, const uint8_t* s, int len, const uint64_t* tab, uint64_t* tmp_k, uint64_t* tmp_s,
                                           uint64_t* out, int cnt, int lane) {
  if (mode == 2) return syncmer_mate(s, len, a.k, (int)a.w_or_s, tab, a.scaled != 0, a.max_hash, tmp_k, tmp_s, out, cnt, lane);
  if (mode == 1) return minimizer_mate(s, len, a.k, (int)a.w_or_s, tab, a.scaled != 0, a.max_hash, tmp_k, out, cnt, lane);
  return hash_mate(s, len, a.k, tab, a.scaled != 0, a.max_hash, out, cnt, lane);
}


// one kernel per sketch mode: the plain/FracMinHash form (every short-read search) does not carry the window sketches' registers
template <int MODE>
__global__ void __launch_bounds__(256) k1_kmers(const K1Args a) {
  __shared__ uint64_t tab[256];
  tab[threadIdx.x] = seed_of(threadIdx.x);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * 4;
  for (uint32_t r = wave; r < a.n_reads; r += nwaves) {
    const uint64_t o1 = a.offs[r];
    const int len1 = (int)(a.offs[r + 1] - o1);
    uint64_t o2 = 0;
    int len2 = 0;
    const bool pe = a.offs2 != nullptr;
    if (pe) {
      o2 = a.offs2[r];
      len2 = (int)(a.offs2[r + 1] - o2);
    }
    uint64_t* out = a.hashes + o1 + o2;
    // skip short query: handleQuery :778-786
    const bool skip = len1 < a.min_qlen && !(pe && len2 >= a.min_qlen);
    int cnt = 0, cnt1 = 0;
    if (!skip) {
      uint64_t* tk = a.scratch ? a.scratch + o1 + o2 : nullptr;   // k-mer hashes of the mate being sketched
      uint64_t* ts = a.scratch2 ? a.scratch2 + o1 + o2 : nullptr;  // its s-mer hashes (syncmer mode)
      cnt = sketch_mate(a, MODE, k1_bases(a, r, o1), len1, tab, tk, ts, out, 0, lane);
      cnt1 = cnt;
      if (pe) {
        __threadfence_block();
        cnt = sketch_mate(a, MODE, a.seqs2 + o2, len2, tab, tk, ts, out, cnt, lane);
      }
    }
    if (lane == 0) {
      a.nk_raw[r] = cnt;
      a.nk1[r] = cnt1;
      a.qlen[r] = len1 + len2;
    }
  }
}

// ---- long queries (HiFi reads, -g whole genomes): one 1024-thread workgroup per read -------------------------
constexpr int K1WG = 1024;

// ordered compaction of one tile of K1WG candidates into out[cnt...]; returns the new (uniform) count
__device__ __forceinline__ int wg_compact(bool keep, uint64_t h, uint64_t* __restrict__ out, int cnt, int* s_wave, int tid) {
  const int lane = tid & 63, w = tid >> 6;
  const uint64_t m = __ballot(keep);
  if (lane == 0) s_wave[w] = __popcll(m);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int i = 0; i < K1WG / 64; i++) {
    const int c = s_wave[i];
    if (i < w) before += c;
    total += c;
  }
  if (keep) out[cnt + before + __popcll(m & ((1ULL << lane) - 1ULL))] = h;
  __syncthreads();
  return cnt + __builtin_amdgcn_readfirstlane(total);
}

__device__ __forceinline__ int wg_sketch_mate(const K1Args& a, int mode, const uint8_t* __restrict__ s, int len, const uint64_t* tab, uint64_t* hk,
                                              uint64_t* hs, uint64_t* __restrict__ out, int cnt, int* s_wave, int tid) {
  const int k = a.k;
  const bool scaled = a.scaled != 0;
  if (mode == 0) {
    const int npos = len - k + 1;
    if (npos <= 0) return cnt;
    for (int base = 0; base < npos; base += K1WG) {
      const int i = base + tid;
      const bool v = i < npos;
      const uint64_t h = v ? hash_at(s, i, k, tab) : 0;
      cnt = wg_compact(v && h != 0 && (!scaled || h <= a.max_hash), h, out, cnt, s_wave, tid);
    }
    return cnt;
  }
  if (mode == 2) {  // closed syncmer, see syncmer_mate
    const int sm = (int)a.w_or_s, L = 2 * k - sm - 1;
    if (sm < 1 || sm > k || len < L || len < k) return cnt;
    for (int i = tid; i < len - k + 1; i += K1WG) hk[i] = hash_at(s, i, k, tab);
    for (int i = tid; i < len - sm + 1; i += K1WG) hs[i] = hash_at(s, i, sm, tab);
    __threadfence_block();
    __syncthreads();
    const int wsz = 2 * (k - sm);
    const int nw = wsz > 0 ? len - L + 1 : len - k + 1;
    for (int base = 0; base < nw; base += K1WG) {
      const int w0 = base + tid;
      const bool v = w0 < nw;
      uint64_t h = 0;
      if (v) {
        int pos = w0;
        if (wsz > 0) {
          const int m = argmin_left(hs, w0, wsz);
          pos = (m - w0 < k - sm) ? m : m + sm - k;
        }
        h = hk[pos];
      }
      cnt = wg_compact(v && h != 0 && (!scaled || h <= a.max_hash), h, out, cnt, s_wave, tid);
    }
    __syncthreads();
    return cnt;
  }
  // minimizer, see minimizer_mate
  const int w = (int)a.w_or_s;
  if (w < 1 || len < k + w - 1) return cnt;
  for (int i = tid; i < len - k + 1; i += K1WG) hk[i] = hash_at(s, i, k, tab);
  __threadfence_block();
  __syncthreads();
  const int nw = len - k + 1 - w + 1;
  for (int base = 0; base < nw; base += K1WG) {
    const int w0 = base + tid;
    const bool v = w0 < nw;
    int m = -1, pm = -2;
    if (v) {
      m = argmin_left(hk, w0, w);
      pm = w0 > 0 ? argmin_left(hk, w0 - 1, w) : -2;
    }
    const uint64_t h = (v && m != pm) ? hk[m] : 0;
    cnt = wg_compact(v && m != pm && h != 0 && (!scaled || h <= a.max_hash), h, out, cnt, s_wave, tid);
  }
  __syncthreads();
  return cnt;
}

// LDS-tiled form of wg_sketch_mate: the prefix XORs P, Q (see the K1 header) of one tile — 1024 positions + halo — are
// built in LDS by wave scans + a scan of the 64-base group totals, after which any k-mer or s-mer hash of the tile costs
// four LDS reads; the window scans never go to global memory.  Usable while the halo fits (L = 2k-s-1 <= 512 for syncmers,
// w < 512 for minimizers); otherwise the scratch-buffer version above is used.
constexpr int K1CAP = 2 * K1WG;  // bases per tile: 1024 positions + a halo of at most 1024
struct K1Lds {
  uint64_t ip[K1CAP + 1];                   // ip[n] = P(n) = XOR_{m<n} ror(F[m], m) over the tile's bases, ip[0] = 0
  uint64_t iq[K1CAP + 1];                   // iq[n] = Q(n)
  uint64_t tp[K1CAP / 64], tq[K1CAP / 64];  // totals of the 64-base groups, then their exclusive prefixes
  uint64_t hw[K1WG + K1H];                  // the hashes the windows scan: s-mers (syncmer) or k-mers (minimizer)
  uint64_t m4v[K1WG + K1H];                 // m4v[i] = min(hw[i..i+3]), m4i[i] = its leftmost position: the windows' arg-min reads
  uint16_t m4i[K1WG + K1H];                 // a quarter of the values (two-level scan)
};

// builds L.ip / L.iq over the nb (<= K1CAP) bases at s; all K1WG threads call it; ends with a barrier
__device__ __forceinline__ void wg_prefix(const uint8_t* __restrict__ s, int nb, const uint64_t* tab, K1Lds& L, int tid) {
  const int lane = tid & 63;
  const int rounds = nb > K1WG ? 2 : 1;
  uint64_t ip[2] = {0, 0}, iq[2] = {0, 0};
#pragma unroll
  for (int r = 0; r < 2; r++) {
    if (r < rounds) {
      const int e = r * K1WG + tid;
      uint64_t F = 0, R = 0;
      if (e < nb) {
        const uint8_t b = s[e];
        F = tab[b];
        R = tab[b & 7];
      }
      ip[r] = wave_xor_scan(rorv(F, lane));  // K1WG % 64 == 0: e & 63 == lane
      iq[r] = wave_xor_scan(rolv(R, lane));
      if (lane == 63) {
        L.tp[e >> 6] = ip[r];
        L.tq[e >> 6] = iq[r];
      }
    }
  }
  __syncthreads();
  if (tid < 64) {  // one wave scans the group totals
    const int ng = rounds * (K1WG / 64);
    const uint64_t a = tid < ng ? L.tp[tid] : 0, b = tid < ng ? L.tq[tid] : 0;
    const uint64_t sa = wave_xor_scan(a), sb = wave_xor_scan(b);
    if (tid < ng) {
      L.tp[tid] = sa ^ a;
      L.tq[tid] = sb ^ b;
    }
    if (tid == 0) L.ip[0] = L.iq[0] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 2; r++) {
    if (r < rounds) {
      const int e = r * K1WG + tid;
      L.ip[e + 1] = ip[r] ^ L.tp[e >> 6];
      L.iq[e + 1] = iq[r] ^ L.tq[e >> 6];
    }
  }
  __syncthreads();
}

// canonical hash of the kk-mer at tile position i (i + kk <= nb of the last wg_prefix)
__device__ __forceinline__ uint64_t lds_hash(const K1Lds& L, int i, int kk) {
  const uint64_t f = rolv(L.ip[i + kk] ^ L.ip[i], kk - 1 + i), r = rorv(L.iq[i + kk] ^ L.iq[i], i);
  return f < r ? f : r;
}

// second level of the window arg-min: leftmost minima of every 4 consecutive entries of hw[0..n); ends with a barrier
__device__ __forceinline__ void wg_min4(K1Lds& L, int n, int tid) {
  for (int i = tid; i + 3 < n; i += K1WG) {
    uint64_t mv = L.hw[i];
    int m = i;
#pragma unroll
    for (int j = 1; j < 4; j++) {
      const uint64_t v = L.hw[i + j];
      if (v < mv) {  // strict: the leftmost of equal values wins
        mv = v;
        m = i + j;
      }
    }
    L.m4v[i] = mv;
    L.m4i[i] = (uint16_t)m;
  }
  __syncthreads();
}

// leftmost minimum of hw[b .. b+n): whole groups of 4 through m4v/m4i, the rest one by one (same result as argmin_left)
__device__ __forceinline__ int argmin_left4(const K1Lds& L, int b, int n) {
  if (n < 4) return argmin_left(L.hw, b, n);
  uint64_t mv = L.m4v[b];
  int m = b;       // group whose minimum is the best so far (its position is looked up once, at the end)
  bool grp = true;  // m names a group of 4 (true) or a single position (false)
  int i = b + 4;
  for (; i + 4 <= b + n; i += 4) {
    const uint64_t v = L.m4v[i];
    if (v < mv) {
      mv = v;
      m = i;
    }
  }
  for (; i < b + n; i++) {
    const uint64_t v = L.hw[i];
    if (v < mv) {
      mv = v;
      m = i;
      grp = false;
    }
  }
  return grp ? (int)L.m4i[m] : m;
}

// Ordered compaction of one tile of K1WG candidates with the adjacent repeats dropped on the way (window sketches emit the same
// k-mer for runs of consecutive windows: ~10 k emissions of a HiFi read hold ~1.4 k distinct adjacent values): a candidate is
// written to out[cnt ...] unless it equals the candidate before it in sequence order (the previous kept lane of its wave, else
// the last candidate of an earlier wave of the tile, else `last` = the last candidate of the tiles — and the mate — before).
// raw counts every candidate.  Returns the new (uniform) count.
struct AdjCarry {
  uint64_t last = 0;
  int have = 0;
  int raw = 0;
};
__device__ __forceinline__ int wg_compact_adj(bool keep, uint64_t h, uint64_t* __restrict__ out, int cnt, AdjCarry& c, int* s_wave, int* s_wave2, uint64_t* s_last,
                                              int tid) {
  const int lane = tid & 63, w = tid >> 6;
  const uint64_t m = __ballot(keep);
  const uint64_t lower = m & ((1ULL << lane) - 1ULL);
  if (lane == 0) s_wave[w] = __popcll(m);
  if (m && lane == 63 - __clzll((unsigned long long)m)) s_last[w] = h;  // the wave's last candidate
  __syncthreads();
  // the candidate before this one
  const int src = lower ? 63 - __clzll((unsigned long long)lower) : lane;
  uint64_t prev = __shfl(h, src);
  bool has_prev = lower != 0;
  int raw_total = 0, last_w = -1;
#pragma unroll
  for (int i = 0; i < K1WG / 64; i++) {
    const int cw = s_wave[i];
    raw_total += cw;
    if (cw > 0) last_w = i;
  }
  if (!has_prev) {
    int pw = -1;
    for (int i = w - 1; i >= 0; i--)
      if (s_wave[i] > 0) {
        pw = i;
        break;
      }
    if (pw >= 0) {
      prev = s_last[pw];
      has_prev = true;
    } else if (c.have) {
      prev = c.last;
      has_prev = true;
    }
  }
  const bool keep2 = keep && !(has_prev && h == prev);
  const uint64_t m2 = __ballot(keep2);
  if (lane == 0) s_wave2[w] = __popcll(m2);
  const uint64_t tile_last = last_w >= 0 ? s_last[last_w] : 0;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int i = 0; i < K1WG / 64; i++) {
    const int cw = s_wave2[i];
    if (i < w) before += cw;
    total += cw;
  }
  if (keep2) out[cnt + before + __popcll(m2 & ((1ULL << lane) - 1ULL))] = h;
  // uniform values: kept in scalar registers (the compiler cannot see that every thread computed the same)
  c.raw += __builtin_amdgcn_readfirstlane(raw_total);
  if (__builtin_amdgcn_readfirstlane(last_w) >= 0) {
    c.last = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(tile_last >> 32)) << 32) |
             (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)tile_last);
    c.have = 1;
  }
  __syncthreads();
  return cnt + __builtin_amdgcn_readfirstlane(total);
}

// positions per tile: with a small halo the tile shrinks so that positions + halo fit one scan round of K1WG bases
__device__ __forceinline__ int wg_tile_step(int halo) { return halo <= K1WG / 2 ? K1WG - halo : K1WG; }

__device__ __forceinline__ int wg_sketch_mate_lds(const K1Args& a, int mode, const uint8_t* __restrict__ s, int len, const uint64_t* tab, K1Lds& L,
                                                  uint64_t* __restrict__ out, int cnt, int* s_wave, int tid) {
  const int k = a.k;
  const bool scaled = a.scaled != 0;
  const int nk = len - k + 1;  // k-mer positions
  if (nk <= 0) return cnt;
  if (mode == 0) {
    const int T = wg_tile_step(k - 1);
    for (int p0 = 0; p0 < nk; p0 += T) {
      wg_prefix(s + p0, min(len - p0, T + k - 1), tab, L, tid);
      const bool v = tid < T && p0 + tid < nk;
      const uint64_t h = v ? lds_hash(L, tid, k) : 0;
      cnt = wg_compact(v && h != 0 && (!scaled || h <= a.max_hash), h, out, cnt, s_wave, tid);
    }
    return cnt;
  }
  return cnt;
}

// The window sketches (Closed Syncmer, Minimizer) of one mate in the LDS tile form.  ADJ = false: every emission is written to
// out[cnt...] (what the reference's generateKmers returns); ADJ = true: adjacent repeats are dropped on the way and c.raw counts
// the emissions (input of the sort + unique that queries above -u get anyway).  The arg-min of a window reads the 4-wide minima
// of wg_min4 (two-level scan): 5 + 0 look-ups instead of 20 for the 20-s-mer windows of k = 21, s = 11.
template <bool ADJ>
__device__ __forceinline__ int wg_window_mate_lds(const K1Args& a, int mode, const uint8_t* __restrict__ s, int len, const uint64_t* tab, K1Lds& L,
                                                  uint64_t* __restrict__ out, int cnt, AdjCarry& c, int* s_wave, int* s_wave2, uint64_t* s_last, int tid) {
  const int k = a.k;
  const bool scaled = a.scaled != 0;
  const int nk = len - k + 1;  // k-mer positions
  if (nk <= 0) return cnt;
  auto emit = [&](bool keep, uint64_t h) {
    if (ADJ) cnt = wg_compact_adj(keep, h, out, cnt, c, s_wave, s_wave2, s_last, tid);
    else cnt = wg_compact(keep, h, out, cnt, s_wave, tid);
  };
  if (mode == 2) {  // closed syncmer (see syncmer_mate)
    const int sm = (int)a.w_or_s, Lw = 2 * k - sm - 1;
    if (len < Lw) return cnt;
    const int wsz = 2 * (k - sm);
    const int nw = wsz > 0 ? len - Lw + 1 : nk;
    const int ns = len - sm + 1;
    const int T = wg_tile_step(Lw);
    for (int p0 = 0; p0 < nw; p0 += T) {
      wg_prefix(s + p0, min(len - p0, T + Lw), tab, L, tid);
      const int nst = min(ns - p0, T + max(wsz - 1, 0));
      for (int i = tid; i < nst; i += K1WG) L.hw[i] = lds_hash(L, i, sm);
      __syncthreads();
      const bool two = wsz >= 4 && (a.flags & K1F_TWO_LEVEL);
      if (two) wg_min4(L, nst, tid);
      const bool v = tid < T && p0 + tid < nw;
      uint64_t h = 0;
      if (v) {
        int pos = tid;
        if (wsz > 0) {
          const int m = two ? argmin_left4(L, tid, wsz) : argmin_left(L.hw, tid, wsz);
          pos = (m - tid < k - sm) ? m : m + sm - k;
        }
        h = lds_hash(L, pos, k);
      }
      emit(v && h != 0 && (!scaled || h <= a.max_hash), h);
    }
    return cnt;
  }
  // minimizer (see minimizer_mate)
  const int w = (int)a.w_or_s;
  if (len < k + w - 1) return cnt;
  const int nw = nk - w + 1;
  const int T = wg_tile_step(w + k);
  for (int p0 = 0; p0 < nw; p0 += T) {
    const int b0 = p0 > 0 ? p0 - 1 : 0, off = p0 - b0;  // the window before the tile's first one is needed too
    wg_prefix(s + b0, min(len - b0, T + w + k), tab, L, tid);
    const int nkt = min(nk - b0, T + w);
    for (int i = tid; i < nkt; i += K1WG) L.hw[i] = lds_hash(L, i, k);
    __syncthreads();
    const bool two = w >= 4 && (a.flags & K1F_TWO_LEVEL);
    if (two) wg_min4(L, nkt, tid);
    const int w0 = p0 + tid;
    const bool v = tid < T && w0 < nw;
    int m = -1, pm = -2;
    if (v) {
      m = two ? argmin_left4(L, off + tid, w) : argmin_left(L.hw, off + tid, w);
      pm = w0 <= 0 ? -2 : (two ? argmin_left4(L, off + tid - 1, w) : argmin_left(L.hw, off + tid - 1, w));
    }
    const uint64_t h = (v && m != pm) ? L.hw[m] : 0;
    emit(v && m != pm && h != 0 && (!scaled || h <= a.max_hash), h);
  }
  return cnt;
}

// the per-read loop of the workgroup kernels; LDS = the tile form with prefix arrays in LDS, else the scratch-buffer form
template <bool LDS>
__device__ __forceinline__ void wg_reads(const K1Args& a, int mode, const uint64_t* tab, int* s_wave, K1Lds* lds, int tid) {
  for (uint32_t r = blockIdx.x; r < a.n_reads; r += gridDim.x) {
    const uint64_t o1 = a.offs[r];
    const int len1 = (int)(a.offs[r + 1] - o1);
    uint64_t o2 = 0;
    int len2 = 0;
    const bool pe = a.offs2 != nullptr;
    if (pe) {
      o2 = a.offs2[r];
      len2 = (int)(a.offs2[r + 1] - o2);
    }
    uint64_t* out = a.hashes + o1 + o2;
    const bool skip = len1 < a.min_qlen && !(pe && len2 >= a.min_qlen);
    int cnt = 0, cnt1 = 0;
    if (!skip) {
      if (LDS) {
        cnt = wg_sketch_mate_lds(a, mode, k1_bases(a, r, o1), len1, tab, *lds, out, 0, s_wave, tid);
        cnt1 = cnt;
        if (pe) cnt = wg_sketch_mate_lds(a, mode, a.seqs2 + o2, len2, tab, *lds, out, cnt, s_wave, tid);
      } else {
        uint64_t* tk = a.scratch ? a.scratch + o1 + o2 : nullptr;
        uint64_t* ts = a.scratch2 ? a.scratch2 + o1 + o2 : nullptr;
        cnt = wg_sketch_mate(a, mode, k1_bases(a, r, o1), len1, tab, tk, ts, out, 0, s_wave, tid);
        cnt1 = cnt;
        if (pe) cnt = wg_sketch_mate(a, mode, a.seqs2 + o2, len2, tab, tk, ts, out, cnt, s_wave, tid);
      }
    }
    if (tid == 0) {
      a.nk_raw[r] = cnt;
      a.nk1[r] = cnt1;
      a.qlen[r] = len1 + len2;
    }
  }
}

// The same for the window sketches in the LDS form, with the adjacent-repeat filter of the dedup path fused in.  A query whose
// emissions exceed -u is sorted and uniqued afterwards (:874-908), and window sketches emit runs of equal values, so what the sort
// needs is the sequence without adjacent repeats: it is written to scratch[...] (its length to nk_adj[r]) while the emissions are
// only counted — 1.4 k values instead of 10 k per HiFi read, and no separate k_adj_unique pass.  The emissions themselves are only
// needed as they are for queries that are not deduplicated (<= -u), for those the wave sort takes (<= K1_WAVE_SORT_CAP) and for
// whole-genome queries (device-wide sort): those — short reads in a long-read batch, rare — are sketched a second time into
// hashes[...].  A query that cannot exceed the bound by its length skips the first pass.
template <int MODE>
__device__ __forceinline__ void wg_reads_windows(const K1Args& a, const uint64_t* tab, int* s_wave, int* s_wave2, uint64_t* s_last, K1Lds& L, int tid) {
  const int raw_bound = a.dedup_threshold > K1_WAVE_SORT_CAP ? a.dedup_threshold : K1_WAVE_SORT_CAP;
  for (uint32_t r = blockIdx.x; r < a.n_reads; r += gridDim.x) {
    const uint64_t o1 = a.offs[r];
    const int len1 = (int)(a.offs[r + 1] - o1);
    uint64_t o2 = 0;
    int len2 = 0;
    const bool pe = a.offs2 != nullptr;
    if (pe) {
      o2 = a.offs2[r];
      len2 = (int)(a.offs2[r + 1] - o2);
    }
    const bool skip = len1 < a.min_qlen && !(pe && len2 >= a.min_qlen);
    int raw = 0, raw1 = 0;
    if (!skip) {
      bool need_raw = true;
      if ((a.flags & K1F_FUSED_ADJ) && a.nk_adj && a.scratch && len1 + len2 > raw_bound) {  // (a mate emits at most one value per base)
        AdjCarry c;
        uint64_t* adj = a.scratch + o1 + o2;
        int m = wg_window_mate_lds<true>(a, MODE, k1_bases(a, r, o1), len1, tab, L, adj, 0, c, s_wave, s_wave2, s_last, tid);
        raw1 = c.raw;
        if (pe) m = wg_window_mate_lds<true>(a, MODE, a.seqs2 + o2, len2, tab, L, adj, m, c, s_wave, s_wave2, s_last, tid);
        raw = c.raw;
        need_raw = raw <= raw_bound || raw > (int)HUGE_MIN;
        if (!need_raw && tid == 0) a.nk_adj[r] = m;
      }
      if (need_raw) {
        AdjCarry c;
        uint64_t* out = a.hashes + o1 + o2;
        raw = wg_window_mate_lds<false>(a, MODE, k1_bases(a, r, o1), len1, tab, L, out, 0, c, s_wave, s_wave2, s_last, tid);
        raw1 = raw;
        if (pe) raw = wg_window_mate_lds<false>(a, MODE, a.seqs2 + o2, len2, tab, L, out, raw, c, s_wave, s_wave2, s_last, tid);
      }
    }
    if (tid == 0) {
      a.nk_raw[r] = raw;
      a.nk1[r] = raw1;
      a.qlen[r] = len1 + len2;
    }
  }
}

// One kernel per sketch mode (the other modes' code and registers stay out of it); 64 VGPRs => two workgroups per CU.
template <int MODE>
__global__ void __launch_bounds__(K1WG, 8) k1_kmers_wg(const K1Args a) {
  __shared__ uint64_t tab[256];
  __shared__ int s_wave[K1WG / 64];
  __shared__ K1Lds lds;
  const int tid = threadIdx.x;
  if (tid < 256) tab[tid] = seed_of(tid);
  __syncthreads();
  if constexpr (MODE == 0) {
    wg_reads<true>(a, MODE, tab, s_wave, &lds, tid);
  } else {
    __shared__ int s_wave2[K1WG / 64];
    __shared__ uint64_t s_last[K1WG / 64];
    wg_reads_windows<MODE>(a, tab, s_wave, s_wave2, s_last, lds, tid);
  }
}

// halo too large for the LDS tiles (2k-s-1 > 512, w >= 511, k > 255): window scans over scratch arrays in global memory
__global__ void __launch_bounds__(K1WG) k1_kmers_wg_global(const K1Args a) {
  __shared__ uint64_t tab[256];
  __shared__ int s_wave[K1WG / 64];
  const int tid = threadIdx.x;
  if (tid < 256) tab[tid] = seed_of(tid);
  __syncthreads();
  wg_reads<false>(a, a.mode, tab, s_wave, nullptr, tid);
}

// A whole genome's segment (plain / FracMinHash k-mers; k1_seg.hip has the passes) on the LDS tile form above: the first generation of the
// segment kernels, here with the tile machinery it is made of.
__global__ void __launch_bounds__(K1WG) k1_seg_hash(const K1Args a) {
  __shared__ uint64_t tab[256];
  __shared__ int s_wave[K1WG / 64];
  __shared__ K1Lds lds;
  const int tid = threadIdx.x;
  if (tid < 256) tab[tid] = seed_of(tid);
  __syncthreads();
  const uint32_t r = blockIdx.x / a.segs_max, seg = blockIdx.x % a.segs_max;
  const uint64_t o1 = a.offs[r];
  const int len = (int)(a.offs[r + 1] - o1);
  const int npos = len - a.k + 1;
  const int p_lo = (int)seg * K1SEG;
  int cnt = 0;
  if (len >= a.min_qlen && p_lo < npos) {  // (:778-786 gate; ErrShortSeq => no k-mers)
    const uint8_t* __restrict__ s = k1_bases(a, r, o1);
    uint64_t* __restrict__ out = a.scratch + o1 + p_lo;
    const int p_hi = min(npos, p_lo + K1SEG);
    const bool scaled = a.scaled != 0;
    const int T = wg_tile_step(a.k - 1);
    for (int p0 = p_lo; p0 < p_hi; p0 += T) {
      wg_prefix(s + p0, min(len - p0, T + a.k - 1), tab, lds, tid);
      const bool v = tid < T && p0 + tid < p_hi;
      const uint64_t h = v ? lds_hash(lds, tid, a.k) : 0;
      cnt = wg_compact(v && h != 0 && (!scaled || h <= a.max_hash), h, out, cnt, s_wave, tid);
    }
  }
  if (tid == 0) a.seg_cnt[blockIdx.x] = cnt;
}

template <int MODE>
static void kmers_launch(const K1Args& a, unsigned grid, hipStream_t st, K1Log* log) {
  hipLaunchKernelGGL(k1_kmers<MODE>, dim3(grid), dim3(256), 0, st, a);
  k1_note(log, KMCPG_K1_KMERS, MODE, 0, grid, 256, 0);
}
template <int MODE>
static void kmers_wg_launch(const K1Args& a, unsigned grid, hipStream_t st, K1Log* log) {
  hipLaunchKernelGGL(k1_kmers_wg<MODE>, dim3(grid), dim3(K1WG), 0, st, a);
  k1_note(log, KMCPG_K1_KMERS_WG, MODE, 0, grid, K1WG, 0);
}

void launch_k1_short(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log) {
  if (a.mode == 2) kmers_launch<2>(a, p.grid, st, log);
  else if (a.mode == 1) kmers_launch<1>(a, p.grid, st, log);
  else kmers_launch<0>(a, p.grid, st, log);
}

void launch_k1_wg(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log) {
  if (a.mode == 2) kmers_wg_launch<2>(a, p.grid, st, log);
  else if (a.mode == 1) kmers_wg_launch<1>(a, p.grid, st, log);
  else kmers_wg_launch<0>(a, p.grid, st, log);
}

void launch_k1_wg_global(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log) {
  hipLaunchKernelGGL(k1_kmers_wg_global, dim3(p.grid), dim3(K1WG), 0, st, a);
  k1_note(log, KMCPG_K1_KMERS_WG_GLOBAL, 0, 0, p.grid, K1WG, 0);
}

void launch_k1_seg_hash(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log) {
  hipLaunchKernelGGL(k1_seg_hash, dim3(p.grid), dim3(K1WG), 0, st, a);
  k1_note(log, KMCPG_K1_SEG_HASH, 0, 0, p.grid, K1WG, 0);
}

}  // namespace kmcpg
