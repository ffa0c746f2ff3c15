// k1_windows.hip — K1, window sketches (Closed Syncmer, Minimizer) of long reads: the barrier-free wave form (k1_windows_wave) and the
// rolling form for closed syncmers (k1_windows_roll), which leaves the reads it cannot take on a list for the former.  Forms WindowsWave /
// WindowsRoll of launch_k1 (k1_kmers.hip).
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

// ---- window sketches of long reads, barrier-free form (k <= 65, windows of at most 64 hashes: every practical setting) ---------
// The 1024-thread tile form (k1_kmers_wg, k1_reads.hip) spends its time in workgroup barriers (eight per tile of ~1000 windows: prefix arrays,
// hashes, minima, ordered compaction).  Here the 16 waves of the workgroup never wait for each other while they sketch: the
// windows of a mate are cut into 16 contiguous segments, one per wave; a wave walks its segment in tiles of 64 windows with the
// wave-level machinery of the short-read kernel (prefix XOR scans on DPP, wave_hash), keeps the s-mer / k-mer hashes of the current
// and the next tile in a 2-slot ring in LDS that only it touches (wave-level fences), finds the windows' leftmost minima there,
// filters adjacent repeats with ballot + shuffle and appends to a private piece of a temporary array.  Two workgroup barriers per
// mate remain: one before and one after the pieces are moved together in order (dropping an element that repeats across a segment
// boundary).  Semantics are those of syncmer_mate / minimizer_mate.
constexpr int K1W_THREADS = 512;
constexpr int K1W_WAVES = K1W_THREADS / 64;
// Per wave: a ring over two tiles (position p relative to the segment start lives at p & 127) of the inclusive prefix XORs, the
// hashes the windows scan (s-mers for syncmers, k-mers for minimizers), the k-mer hashes, and the second level of the window
// arg-min: m4v[p] = min(hw[p..p+3]), m4i[p] = offset of its leftmost position.  The kernel is bound by VALU issue (a wave64
// instruction takes four cycles on a 16-lane SIMD), so what counts is instructions per window: hashes come from two LDS look-ups
// of the prefix ring instead of eight cross-lane permutes, and a 20-wide window costs 5 + 8 look-ups instead of 20.
struct K1WRing {
  uint64_t ip[128], iq[128];
  uint64_t hw[128];
  uint64_t hk[128];
  uint64_t m4v[128];
  uint8_t m4i[128];
};
struct K1WShared {
  int cnt[K1W_WAVES], raw[K1W_WAVES];
  uint64_t first[K1W_WAVES], last[K1W_WAVES];
};
struct SeqCarry {  // uniform over the workgroup
  uint64_t last = 0;
  int have = 0, raw = 0, cnt = 0;
};

__device__ __forceinline__ uint64_t readfirst64(uint64_t v) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// canonical hash of the kk-mer at ring position p = 64 T + lane of the tile whose scan is `t` (its exclusive prefixes are in
// registers, the inclusive prefix at the kk-mer's last base comes from the ring)
__device__ __forceinline__ uint64_t ring_hash(const K1WRing& ring, const WTile& t, int p, int kk, int lane) {
  const int e = (p + kk - 1) & 127;
  const uint64_t f = rolv(ring.ip[e] ^ t.ip ^ t.xp, kk - 1 + lane), r = rorv(ring.iq[e] ^ t.iq ^ t.xq, lane);
  return f < r ? f : r;
}

// m4v / m4i of ring position p (needs hw[p .. p+3])
__device__ __forceinline__ void ring_min4(K1WRing& ring, int p) {
  uint64_t mv = ring.hw[p & 127];
  int m = 0;
#pragma unroll
  for (int j = 1; j < 4; j++) {
    const uint64_t x = ring.hw[(p + j) & 127];
    if (x < mv) {  // strict: the leftmost of equal values wins
      mv = x;
      m = j;
    }
  }
  ring.m4v[p & 127] = mv;
  ring.m4i[p & 127] = (uint8_t)m;
}

// leftmost minimum of hw[p0 .. p0+n) through the 4-wide minima (n >= 1); returns the position, *val = the value
__device__ __forceinline__ int ring_argmin(const K1WRing& ring, int p0, int n, uint64_t* val) {
  int i = 0;
  uint64_t mv;
  int m;       // start of the best group (grp) or the best single position
  bool grp;
  if (n >= 4) {
    mv = ring.m4v[p0 & 127];
    m = p0;
    grp = true;
    for (i = 4; i + 4 <= n; i += 4) {
      const uint64_t x = ring.m4v[(p0 + i) & 127];
      if (x < mv) {
        mv = x;
        m = p0 + i;
      }
    }
  } else {
    mv = ring.hw[p0 & 127];
    m = p0;
    grp = false;
    i = 1;
  }
  for (; i < n; i++) {
    const uint64_t x = ring.hw[(p0 + i) & 127];
    if (x < mv) {
      mv = x;
      m = p0 + i;
      grp = false;
    }
  }
  *val = mv;
  return grp ? m + (int)ring.m4i[m & 127] : m;
}

template <int MODE, bool ADJ>
__device__ __forceinline__ void wgw_mate(const K1Args& a, const uint8_t* __restrict__ s, int len, const uint64_t* tab, K1WRing& ring, K1WShared& sh,
                                         uint64_t* __restrict__ temp, uint64_t* __restrict__ fin, SeqCarry& c, int tid) {
  const int lane = tid & 63, w = tid >> 6;
  const int k = a.k;
  const bool scaled = a.scaled != 0;
  const int nk = len - k + 1;
  int wsz = 0, nw = 0, sm = 0;
  if (MODE == 2) {
    sm = (int)a.w_or_s;
    const int Lw = 2 * k - sm - 1;
    wsz = 2 * (k - sm);
    nw = (nk <= 0 || len < Lw) ? 0 : (wsz > 0 ? len - Lw + 1 : nk);
  } else {
    wsz = (int)a.w_or_s;
    nw = (nk <= 0 || len < k + wsz - 1) ? 0 : nk - wsz + 1;
  }
  if (nw <= 0) return;  // ErrShortSeq (uniform)
  const int segw = ((nw + K1W_WAVES * 64 - 1) / (K1W_WAVES * 64)) * 64;  // windows per wave, a multiple of 64
  const int w0s = w * segw, w0e = min(nw, w0s + segw);
  int cnt = 0, raw = 0;
  uint64_t first = 0, last = 0;
  bool any = false;
  if (w0s < w0e) {
    const int ntiles = (w0e - w0s + 63) / 64;
    uint64_t cp = 0, cq = 0;
    WTile B = wave_tile(s, len, w0s, tab, cp, cq, lane);
    ring.ip[lane] = B.ip;
    ring.iq[lane] = B.iq;
    int pm_carry = -2;  // minimizer: arg-min of the window before the tile's first one
    // iteration t: scan tile t+1, hash tile t, windows of tile t-1 (their hashes reach into tile t)
    for (int t = 0; t <= ntiles; t++) {
      const WTile C = wave_tile(s, len, w0s + 64 * (t + 1), tab, cp, cq, lane);
      const int nslot = ((t + 1) & 1) * 64;
      ring.ip[nslot + lane] = C.ip;
      ring.iq[nslot + lane] = C.iq;
      wave_lds_fence();
      const int pt = 64 * t + lane;
      const uint64_t hkv = ring_hash(ring, B, pt, k, lane);
      ring.hk[pt & 127] = hkv;
      ring.hw[pt & 127] = MODE == 2 ? ring_hash(ring, B, pt, sm, lane) : hkv;
      B = C;
      wave_lds_fence();
      if (wsz >= 4) {
        // one pass: the 4-wide minima of this tile's positions 0..60 and of the previous tile's 61..63 (whose last elements
        // have just arrived); the windows below read the previous tile's and this tile's first 57 (wsz <= 60)
        const int pm4 = lane <= 60 ? pt : pt - 64;
        if (pm4 >= 0) ring_min4(ring, pm4);
        wave_lds_fence();
      }
      if (t == 0) continue;
      const int p0 = 64 * (t - 1) + lane;  // this lane's window, relative to w0s
      const bool v = w0s + p0 < w0e;
      uint64_t h = 0;
      bool keep = false;
      if (MODE == 2) {
        int pos = p0;
        if (wsz > 0) {
          uint64_t mv;
          const int m = ring_argmin(ring, p0, wsz, &mv);
          pos = (m - p0 < k - sm) ? m : m + sm - k;
        }
        h = ring.hk[pos & 127];
        keep = v && h != 0 && (!scaled || h <= a.max_hash);
      } else {
        uint64_t mv;
        const int m = ring_argmin(ring, p0, wsz, &mv);
        if (t == 1 && w0s > 0) {  // (uniform branch) window w0s-1 = {k-mer w0s-1} + the first wsz-1 of window w0s
          int pm0 = -1;
          if (lane == 0) {
            const uint64_t x = hash_at(s, w0s - 1, k, tab);
            int m2 = -1;
            uint64_t mv2 = ~0ULL;
            for (int j = 0; j < wsz - 1; j++) {
              const uint64_t y = ring.hk[j & 127];
              if (m2 < 0 || y < mv2) {
                mv2 = y;
                m2 = j;
              }
            }
            pm0 = (m2 < 0 || x <= mv2) ? -1 : m2;  // relative position; -1 = k-mer w0s-1 itself
          }
          pm_carry = __builtin_amdgcn_readfirstlane(pm0);
        }
        int pm = __shfl_up(m, 1);
        if (lane == 0) pm = pm_carry;  // -2 at the very first window of the mate: always emitted
        pm_carry = __builtin_amdgcn_readlane(m, 63);
        h = mv;
        keep = v && m != pm && h != 0 && (!scaled || h <= a.max_hash);
      }
      const uint64_t mk = __ballot(keep);
      const uint64_t lower = mk & ((1ULL << lane) - 1ULL);
      bool keep2 = keep;
      if (ADJ) {
        const int src = lower ? 63 - __clzll((unsigned long long)lower) : lane;
        const uint64_t prev = __shfl(h, src);
        const bool has_prev = lower != 0 || any;
        keep2 = keep && !(has_prev && h == (lower ? prev : last));
      }
      if (mk) {
        const int hi = 63 - __clzll((unsigned long long)mk), lo = __ffsll((unsigned long long)mk) - 1;
        const uint64_t lastv = readfirst64(__shfl(h, hi));
        if (!any) first = readfirst64(__shfl(h, lo));
        last = lastv;
        any = true;
      }
      const uint64_t mk2 = ADJ ? __ballot(keep2) : mk;
      if (keep2) temp[w0s + cnt + __popcll(mk2 & ((1ULL << lane) - 1ULL))] = h;
      cnt += __popcll(mk2);
      raw += __popcll(mk);
      wave_lds_fence();  // the next iteration's hashes and minima overwrite what these windows read
    }
  }
  if (lane == 0) {
    sh.cnt[w] = cnt;
    sh.raw[w] = raw;
    sh.first[w] = first;
    sh.last[w] = last;
  }
  __threadfence_block();
  __syncthreads();
  // the segments' pieces move together, in order
  int off = c.cnt, have = c.have, my_off = 0, my_drop = 0, rawsum = 0;
  uint64_t plast = c.last;
#pragma unroll
  for (int j = 0; j < K1W_WAVES; j++) {
    const int cj = sh.cnt[j];
    rawsum += sh.raw[j];
    const int drop = (ADJ && cj > 0 && have && sh.first[j] == plast) ? 1 : 0;
    if (j == w) {
      my_off = off;
      my_drop = drop;
    }
    off += cj - drop;
    if (sh.raw[j] > 0) {
      plast = sh.last[j];
      have = 1;
    }
  }
  for (int i = lane + my_drop; i < cnt; i += 64) fin[my_off + i - my_drop] = temp[w0s + i];
  c.cnt = __builtin_amdgcn_readfirstlane(off);
  c.have = __builtin_amdgcn_readfirstlane(have);
  c.last = readfirst64(plast);
  c.raw += __builtin_amdgcn_readfirstlane(rawsum);
  __syncthreads();
}

// the per-read loop of the barrier-free window kernel: same contract as wg_reads_windows (scratch[] + nk_adj[] for queries that
// will be sorted, hashes[] for the others)
template <int MODE>
__global__ void __launch_bounds__(K1W_THREADS) k1_windows_wave(const K1Args a) {
  __shared__ uint64_t tab[256];
  __shared__ K1WRing rings[K1W_WAVES];
  __shared__ K1WShared sh;
  const int tid = threadIdx.x;
  if (tid < 256) tab[tid] = seed_of(tid);
  __syncthreads();
  K1WRing& ring = rings[tid >> 6];
  const int raw_bound = a.dedup_threshold > K1_WAVE_SORT_CAP ? a.dedup_threshold : K1_WAVE_SORT_CAP;
  // (behind k1_windows_roll: only the reads that kernel put on its list)
  const uint32_t n_todo = a.seg_only_flagged ? *a.seg_nflag : a.n_reads;
  for (uint32_t it = blockIdx.x; it < n_todo; it += gridDim.x) {
    const uint32_t r = a.seg_only_flagged ? a.seg_list[it] : it;
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
      uint64_t* hs_out = a.hashes + o1 + o2;
      uint64_t* sc_out = a.scratch + o1 + o2;
      bool need_raw = true;
      if (a.nk_adj && len1 + len2 > raw_bound) {  // (a mate emits at most one value per base)
        SeqCarry c;
        wgw_mate<MODE, true>(a, k1_bases(a, r, o1), len1, tab, ring, sh, hs_out, sc_out, c, tid);
        raw1 = c.raw;
        if (pe) wgw_mate<MODE, true>(a, a.seqs2 + o2, len2, tab, ring, sh, hs_out + len1, sc_out, c, tid);
        raw = c.raw;
        need_raw = raw <= raw_bound || raw > (int)HUGE_MIN;
        if (!need_raw && tid == 0) a.nk_adj[r] = c.cnt;
      }
      if (need_raw) {
        SeqCarry c;
        wgw_mate<MODE, false>(a, k1_bases(a, r, o1), len1, tab, ring, sh, sc_out, hs_out, c, tid);
        raw1 = c.raw;
        if (pe) wgw_mate<MODE, false>(a, a.seqs2 + o2, len2, tab, ring, sh, sc_out + len1, hs_out, c, tid);
        raw = c.raw;
      }
    }
    if (tid == 0) {
      a.nk_raw[r] = raw;
      a.nk1[r] = raw1;
      a.qlen[r] = len1 + len2;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Closed-syncmer sketches of long reads by ROLLING (round 6; docs/ROUND_NOTES.md has the costing).  k1_windows_wave gives a lane one
// position and pays ~4.2 wave instructions per window (two 64-bit XOR scans, two closed-form hashes, a two-level arg-min); here a lane
// owns a RUN of consecutive windows of one read (one wave per read, run = windows / 64 rounded up to 16) and walks it on 2-bit codes:
//   * two rolling ntHash states (s-mers and k-mers; nthash.hpp: fh' = rol1(fh) ^ F2[out][in], rh' = ror1(rh ^ R2[out][in]), the pair
//     tables as ONE 16-byte LDS look-up per roll); the codes of the four bases a step needs come from four 16-code shift registers that
//     are refilled every 16 steps (runs start at multiples of 16, so the refill is uniform over the wave);
//   * the leftmost minimum of the window's WSZ = 2 (k - s) s-mer hashes without a data-dependent branch: the s-mer hashes are cut into
//     blocks of WSZ; a block's suffix minima (ties to the left) are scanned in place, in registers, once the block is complete, its
//     prefix minima grow as the next block's hashes arrive, and window i = min(suffix[i], prefix[i + WSZ - 1]) with ties to the suffix
//     (a per-lane monotonic queue would make SOME lane rescan at almost every step);
//   * the k-mer hash of the emission position (within k - s of the window start) from a per-lane ring in LDS ([slot][lane]: every lane
//     keeps to its own two banks whatever slot it reads);
//   * emissions without adjacent repeats go to the lane's own stretch of hashes[] and are moved together in order afterwards, the runs
//     stitched on their first / last values (what k1_windows_wave does across waves).
// Same outputs as k1_windows_wave's fused path: scratch[offs[r] ...] + nk_adj[r], nk_raw / nk1 / qlen.  A read this kernel cannot take
// — any byte other than A/C/G/T in either case, fewer windows than WR_MIN_WINDOWS, longer than the LDS holds, or an emission count
// outside (raw_bound, HUGE_MIN] (the fused path does not apply) — is put on a list for k1_windows_wave, launched right behind.
// Reference: sketches.NewSyncmerSketch / NextSyncmer behind generateKmers (util-db-search.go:1053,1068).
// ------------------------------------------------------------------------------------------------
constexpr int WR_MIN_WINDOWS = 1024;
// (WR_PAD_BASES, wr_words_for, wr_ring, wr_lds_bytes: k1_plan.hpp)

template <int WSZ, int WR_WAVES>
__global__ void __launch_bounds__(64 * WR_WAVES) k1_windows_roll(const K1Args a, int words) {
  extern __shared__ __attribute__((aligned(16))) uint8_t wr_lds[];
  constexpr int KR = WSZ <= 30 ? 16 : 32;
  constexpr int D = WSZ / 2;  // k - s
  uint4* const TK = reinterpret_cast<uint4*>(wr_lds);         // [16] {F2, R2} of the k-mer roll
  uint4* const TS = TK + 16;                                   // [16] ... of the s-mer roll
  uint64_t* const SD = reinterpret_cast<uint64_t*>(TS + 16);   // [4] seeds by code, [4] seeds of the complements
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  uint8_t* const mine_lds = wr_lds + 1024 + (size_t)w * ((size_t)KR * 64 * 8 + (size_t)words * 4);
  uint64_t* const ring = reinterpret_cast<uint64_t*>(mine_lds);                    // [KR][64]
  uint32_t* const Wd = reinterpret_cast<uint32_t*>(mine_lds + (size_t)KR * 64 * 8);  // [words]: 16 codes each
  const int k = a.k, sm = (int)a.w_or_s;
  if (tid < 16) {
    const uint64_t fk = nt2_f2(tid >> 2, tid & 3, k), rk = nt2_r2(tid >> 2, tid & 3, k);
    const uint64_t fs = nt2_f2(tid >> 2, tid & 3, sm), rs = nt2_r2(tid >> 2, tid & 3, sm);
    TK[tid] = make_uint4((uint32_t)fk, (uint32_t)(fk >> 32), (uint32_t)rk, (uint32_t)(rk >> 32));
    TS[tid] = make_uint4((uint32_t)fs, (uint32_t)(fs >> 32), (uint32_t)rs, (uint32_t)(rs >> 32));
    if (tid < 4) {
      nt2_fill_seeds(SD, SD + 4, tid);
    }
  }
  __syncthreads();
  const uint32_t r = blockIdx.x * WR_WAVES + (uint32_t)w;
  if (r >= a.n_reads) return;  // (no barrier below: the waves of a workgroup are independent from here on)
  const uint64_t o1 = a.offs[r];
  const int len = (int)(a.offs[r + 1] - o1);
  const int Lw = 2 * k - sm - 1;
  const int nw = len - Lw + 1;  // windows (WSZ > 0)
  const int raw_bound = a.dedup_threshold > K1_WAVE_SORT_CAP ? a.dedup_threshold : K1_WAVE_SORT_CAP;
  auto leave_to_wave_kernel = [&]() {
    if (lane == 0) a.seg_list[atomicAdd(a.seg_nflag, 1u)] = r;
  };
  if (len < a.min_qlen || len <= raw_bound || nw < WR_MIN_WINDOWS || len + WR_PAD_BASES > (words - 4) * 16) {
    leave_to_wave_kernel();
    return;
  }
  // ---- the read as 2-bit codes (zeros behind its end)
  {
    const uint8_t* __restrict__ s = k1_bases(a, r, o1);
    typedef uint32_t u32x4_any __attribute__((ext_vector_type(4), aligned(1)));
    bool bad = false;
    for (int gi = lane; gi < words; gi += 64) {
      const int b0 = gi * 16;
      uint32_t word = 0;
      if (b0 + 16 <= len) {
        const u32x4_any v = *reinterpret_cast<const u32x4_any*>(s + b0);
        const uint32_t in[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int d = 0; d < 4; d++) {
          const uint32_t c = nt2_codes4(in[d]);
          bad |= !nt2_valid4(in[d], c);
          word |= nt2_fold4(c) << (8 * d);
        }
      } else if (b0 < len) {
        for (int j = 0; b0 + j < len; j++) {
          const uint32_t ch = s[b0 + j], c = (ch >> 1) & 3u;
          bad |= (ch & 0xDFu) != (uint32_t)nt2_letter((int)c);
          word |= c << (2 * j);
        }
      }
      Wd[gi] = word;
    }
    if (__ballot(bad) != 0) {
      leave_to_wave_kernel();
      return;
    }
  }
  wave_lds_fence();
  const int L = (((nw + 63) / 64) + 15) & ~15;  // windows per lane, a multiple of 16
  const int q0 = lane * L, q1 = min(nw, q0 + L);
  const bool scaled = a.scaled != 0;
  const uint64_t max_hash = a.max_hash;
  auto code_at = [&](int q) -> uint32_t { return (Wd[q >> 4] >> (2 * (q & 15))) & 3u; };
  auto start_up = [&](int q, int kk, uint64_t& fh, uint64_t& rh) {  // fh = XOR_j rol(F[j], kk-1-j), rh = XOR_j rol(R[j], j) of the kk-mer at q
    fh = 0;
    rh = 0;
    for (int j = 0; j < kk; j++) {
      const uint32_t c = code_at(q + j);
      fh = nt2_rol1(fh) ^ SD[c];
      rh ^= rolv(SD[4 + c], j);
    }
  };
  auto roll = [&](uint64_t& fh, uint64_t& rh, uint32_t oc, uint32_t ic, const uint4* T) __attribute__((always_inline)) {
    const uint4 t = T[(oc << 2) | ic];
    fh = nt2_rol1(fh) ^ (((uint64_t)t.y << 32) | t.x);
    rh = nt2_ror1(rh ^ (((uint64_t)t.w << 32) | t.z));
  };
  // ---- warm-up: the first block of s-mer hashes, the first D k-mer hashes
  uint64_t x[WSZ];
  int pidx[WSZ];
  uint64_t sfh, srh, kfh, krh;
  start_up(q0, sm, sfh, srh);
  x[0] = sfh < srh ? sfh : srh;
#pragma unroll
  for (int j = 1; j < WSZ; j++) {
    roll(sfh, srh, code_at(q0 + j - 1), code_at(q0 + j - 1 + sm), TS);
    x[j] = sfh < srh ? sfh : srh;
  }
  start_up(q0, k, kfh, krh);
  ring[(q0 & (KR - 1)) * 64 + lane] = kfh < krh ? kfh : krh;
  for (int t = 1; t <= D; t++) {  // k-mer hashes of q0 .. q0 + D: the roll stays ONE position ahead of what the next window may ask for
    roll(kfh, krh, code_at(q0 + t - 1), code_at(q0 + t - 1 + k), TK);
    ring[((q0 + t) & (KR - 1)) * 64 + lane] = kfh < krh ? kfh : krh;
  }
  auto suffix_scan = [&]() __attribute__((always_inline)) {  // x[j] <- min(x[j .. WSZ-1]), pidx[j] <- its leftmost position in the block
    pidx[WSZ - 1] = WSZ - 1;
#pragma unroll
    for (int j = WSZ - 2; j >= 0; j--) {
      const bool left = x[j] <= x[j + 1];
      pidx[j] = left ? j : pidx[j + 1];
      x[j] = left ? x[j] : x[j + 1];
    }
  };
  suffix_scan();
  // the codes a step needs, relative to its window i: s-mer roll out / in (to position i + WSZ), k-mer roll out / in (to i + D + 1)
  const int d_so = WSZ - 1, d_si = WSZ - 1 + sm, d_ko = D, d_ki = D + k;
  uint32_t c_so = 0, c_si = 0, c_ko = 0, c_ki = 0;
  auto refill = [&](int i, int d) -> uint32_t {  // 16 codes from base i + d on (i is a multiple of 16)
    const int b = i + d;
    return nt2_funnel(Wd[(b >> 4) + 1], Wd[b >> 4], (uint32_t)(2 * (b & 15)));
  };
  uint64_t* __restrict__ temp = a.hashes + o1 + q0;
  int cnt = 0, raw = 0;
  uint64_t first = 0, last = 0, pv = ~0ULL;
  int pp = 0;
  auto emit = [&](uint64_t h, bool on) __attribute__((always_inline)) {
    // (almost every window keeps its value — a hash is 0 or above maxHash rarely — so what is kept is tracked with selects; the one
    // branch is the store of a value that differs from the lane's previous one, a fifth of the steps per lane)
    const bool keep = on && h != 0 && (!scaled || h <= max_hash);
    if (keep && (raw == 0 || h != last)) {
      if (cnt == 0) first = h;  // (the first kept value is always stored)
      temp[cnt++] = h;
    }
    last = keep ? h : last;
    raw += keep ? 1 : 0;
  };
  // The step is software-pipelined by hand: the k-mer hash of window i is ASKED for at the top of step i and USED at the top of step
  // i + 1, and the pair-table entries of step i + 1's rolls are asked for at the end of step i — an LDS round trip is ~100 cycles and
  // the first version (three of them waited for in every step, two waves per SIMD) ran at a fifth of the issue rate.
  c_so = refill(q0, d_so);
  c_si = refill(q0, d_si);
  c_ko = refill(q0, d_ko);
  c_ki = refill(q0, d_ki);
  uint4 ts = TS[((c_so & 3u) << 2) | (c_si & 3u)], tk = TK[((c_ko & 3u) << 2) | (c_ki & 3u)];
  uint64_t hq = 0;   // the k-mer hash window i - 1 emits (arriving)
  bool on_q = false;  // ... and whether that window exists
  const int nblk = (L + WSZ - 1) / WSZ;
  int n = 0;  // windows done by every lane (uniform)
  for (int b = 0; b < nblk; b++) {
    const int base = q0 + b * WSZ;
#pragma unroll
    for (int j = 0; j < WSZ; j++, n++) {
      const int i = base + j;
      // window i: the suffix of this block from j on, the first j hashes of the next block
      const bool right = pv < x[j];
      const int m = right ? pp : base + pidx[j];
      const int pos = (m - i < D) ? m : m + sm - k;
      const uint64_t hcur = ring[(pos & (KR - 1)) * 64 + lane];
      emit(hq, on_q);
      // the s-mer hash at i + WSZ joins the next block's prefix; the k-mer hash at i + D + 1 enters the ring
      sfh = nt2_rol1(sfh) ^ (((uint64_t)ts.y << 32) | ts.x);
      srh = nt2_ror1(srh ^ (((uint64_t)ts.w << 32) | ts.z));
      kfh = nt2_rol1(kfh) ^ (((uint64_t)tk.y << 32) | tk.x);
      krh = nt2_ror1(krh ^ (((uint64_t)tk.w << 32) | tk.z));
      const uint64_t hs = sfh < srh ? sfh : srh;
      if (hs < pv) {
        pv = hs;
        pp = i + WSZ;
      }
      x[j] = hs;
      ring[((i + D + 1) & (KR - 1)) * 64 + lane] = kfh < krh ? kfh : krh;
      c_so >>= 2;
      c_si >>= 2;
      c_ko >>= 2;
      c_ki >>= 2;
      if (((n + 1) & 15) == 0) {  // uniform: the next 16 steps' codes
        c_so = refill(q0 + n + 1, d_so);
        c_si = refill(q0 + n + 1, d_si);
        c_ko = refill(q0 + n + 1, d_ko);
        c_ki = refill(q0 + n + 1, d_ki);
      }
      ts = TS[((c_so & 3u) << 2) | (c_si & 3u)];
      tk = TK[((c_ko & 3u) << 2) | (c_ki & 3u)];
      hq = hcur;
      on_q = i < q1;
    }
    suffix_scan();
    pv = ~0ULL;
  }
  emit(hq, on_q);
  // ---- the runs' pieces move together, in order; a run whose first kept value repeats the previous run's last one drops it
  const uint64_t has = __ballot(raw > 0);
  const uint64_t lower = has & ((1ULL << lane) - 1ULL);
  const int src = lower ? 63 - __clzll((unsigned long long)lower) : lane;
  const uint64_t prev_last = __shfl(last, src);
  const int drop = (raw > 0 && lower != 0 && first == prev_last) ? 1 : 0;
  const int mine = cnt - drop;
  int incl = mine, raw_all = raw;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t1 = __shfl_up(incl, off), t2 = __shfl_up(raw_all, off);
    if (lane >= off) {
      incl += t1;
      raw_all += t2;
    }
  }
  const int total = __builtin_amdgcn_readlane(incl, 63), raw_total = __builtin_amdgcn_readlane(raw_all, 63);
  if (raw_total <= raw_bound || raw_total > (int)HUGE_MIN) {  // the fused path does not apply (k1_windows_wave decides the same way)
    leave_to_wave_kernel();
    return;
  }
  // every lane moves its own piece (its stretch of hashes[] -> its place in scratch[]), eight values in flight: a loop over the 64
  // pieces with the whole wave copying one piece at a time was 64 dependent global round trips, ~100 us per read
  {
    uint64_t* __restrict__ fin = a.scratch + o1 + (incl - mine);
    const uint64_t* __restrict__ src = temp + drop;
    int most = mine;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) most = max(most, __shfl_xor(most, off));
    for (int t = 0; t < most; t += 8) {
      uint64_t v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) v[u] = t + u < mine ? src[t + u] : 0;
#pragma unroll
      for (int u = 0; u < 8; u++)
        if (t + u < mine) fin[t + u] = v[u];
    }
  }
  if (lane == 0) {
    a.nk_adj[r] = total;
    a.nk_raw[r] = raw_total;
    a.nk1[r] = raw_total;
    a.qlen[r] = len;
  }
}

template <int MODE>
static void windows_wave_launch(const K1Args& a, unsigned grid, hipStream_t st, K1Log* log) {
  hipLaunchKernelGGL(k1_windows_wave<MODE>, dim3(grid), dim3(K1W_THREADS), 0, st, a);
  k1_note(log, KMCPG_K1_WINDOWS_WAVE, MODE, 0, grid, K1W_THREADS, 0);
}
// k1_windows_roll<WSZ, WAVES>: the 15 forms the plan can name (WSZ 12 / 16 / 20 / 24 / 32 s-mers, 4 / 2 / 1 reads per workgroup)
template <int WSZ, int WAVES>
static void windows_roll_launch(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log) {
  hipLaunchKernelGGL((k1_windows_roll<WSZ, WAVES>), dim3(p.grid), dim3(64 * WAVES), p.lds_bytes, st, a, p.words);
  k1_note(log, KMCPG_K1_WINDOWS_ROLL, WSZ, WAVES, p.grid, 64 * WAVES, p.lds_bytes);
}
template <int WSZ>
static void windows_roll_waves(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log) {
  if (p.waves == 4) windows_roll_launch<WSZ, 4>(a, p, st, log);
  else if (p.waves == 2) windows_roll_launch<WSZ, 2>(a, p, st, log);
  else windows_roll_launch<WSZ, 1>(a, p, st, log);
}

void launch_k1_windows_wave(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log) {
  if (a.mode == 2) windows_wave_launch<2>(a, p.grid, st, log);
  else windows_wave_launch<1>(a, p.grid, st, log);
}

void launch_k1_windows_roll(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log) {
  (void)hipMemsetAsync(a.seg_nflag, 0, sizeof(uint32_t), st);
  switch (p.wsz) {
    case 12: windows_roll_waves<12>(a, p, st, log); break;
    case 16: windows_roll_waves<16>(a, p, st, log); break;
    case 20: windows_roll_waves<20>(a, p, st, log); break;
    case 24: windows_roll_waves<24>(a, p, st, log); break;
    default: windows_roll_waves<32>(a, p, st, log); break;
  }
  windows_wave_launch<2>(a, p.grid2, st, log);
  if (p.debug) {  // how many reads the rolling kernel left to k1_windows_wave
    uint32_t nf = 0;
    (void)hipStreamSynchronize(st);
    (void)hipMemcpy(&nf, a.seg_nflag, sizeof nf, hipMemcpyDeviceToHost);
    fprintf(stderr, "k1_windows_roll<%d>: %u of %u reads left to k1_windows_wave (max_read_len %u, %d words)\n", p.wsz, nf, a.n_reads, p.max_read_len, p.words);
  }
}


}  // namespace kmcpg
