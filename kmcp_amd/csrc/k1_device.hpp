// k1_device.hpp — the wave-level machinery more than one K1 kernel family uses (k1_reads.hip, k1_windows.hip, k1_win_once.hip): the prefix-XOR
// scan on DPP, the 64-base tile and its hashes, the closed-form hash of one position, and the view of a query's bases (k1_seg.hip: k1_bases).
// Everything here is __device__ __forceinline__; a kernel lives in the family file that launches it.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "device_utils.hpp"
#include "k1_plan.hpp"
#include "kernels.hpp"
#include "nthash.hpp"

namespace kmcpg {

// ------------------------------------------------------------------------------------------------
// K1: k-mer generation.  ntHash of the k-mer at position i in closed form:
//     fh(i) = XOR_j rol(F[i+j], k-1-j),   rh(i) = XOR_j rol(R[i+j], j)      (F = seed of the base, R = of its complement)
// Every term is a rotation of a per-position value by an amount that depends on i+j only up to a common rotation, so with
// the prefix XORs  P(n) = XOR_{m<n} ror(F[m], m)  and  Q(n) = XOR_{m<n} rol(R[m], m)
//     fh(i) = rol(P(i+k) ^ P(i), k-1+i),   rh(i) = ror(Q(i+k) ^ Q(i), i)
// i.e. one XOR scan over the bases gives the hashes of every k (and of the s-mers of a syncmer) for two look-ups each,
// instead of k table look-ups per k-mer.  The scans run on DPP within a wave (row_shr 1/2/4/8, row_bcast 15/31).
// ------------------------------------------------------------------------------------------------

// inclusive XOR scan over the 64 lanes of a wave (all lanes must be active)
__device__ __forceinline__ uint32_t wave_xor_scan32(uint32_t v) {
  v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
  v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8: scan within rows of 16
  v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
  v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
  return v;
}
__device__ __forceinline__ uint64_t wave_xor_scan(uint64_t v) {
  const uint32_t lo = wave_xor_scan32((uint32_t)v), hi = wave_xor_scan32((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_last(uint64_t v) {  // lane 63's value, uniform
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
  return ((uint64_t)hi << 32) | lo;
}

// One wave per read: a tile is 64 consecutive bases, lane = base index & 63 (also its rotation amount).
struct WTile {
  uint64_t ip, iq;  // inclusive prefixes P(e+1), Q(e+1) at this lane's base e
  uint64_t xp, xq;  // this base's own terms
};

__device__ __forceinline__ WTile wave_tile(const uint8_t* __restrict__ s, int len, int e0, const uint64_t* tab, uint64_t& cp, uint64_t& cq, int lane) {
  const int e = e0 + lane;
  uint64_t F = 0, R = 0;
  if (e < len) {
    const uint8_t b = s[e];
    F = tab[b];
    R = tab[b & 7];
  }
  WTile t;
  t.xp = rorv(F, lane);
  t.xq = rolv(R, lane);
  t.ip = wave_xor_scan(t.xp) ^ cp;
  t.iq = wave_xor_scan(t.xq) ^ cq;
  cp = wave_last(t.ip);
  cq = wave_last(t.iq);
  return t;
}

// canonical hash of the kk-mer starting at this lane's base of tile c (n = the following tile); every lane must call it
__device__ __forceinline__ uint64_t wave_hash(const WTile& c, const WTile& n, int kk, int lane) {
  const int src = lane + kk - 1;  // the k-mer's last base
  const uint64_t ec = __shfl(c.ip, src & 63), en = __shfl(n.ip, src & 63);
  const uint64_t qc = __shfl(c.iq, src & 63), qn = __shfl(n.iq, src & 63);
  const uint64_t dp = (src >= 64 ? en : ec) ^ c.ip ^ c.xp;
  const uint64_t dq = (src >= 64 ? qn : qc) ^ c.iq ^ c.xq;
  const uint64_t f = rolv(dp, kk - 1 + lane), r = rorv(dq, lane);
  return f < r ? f : r;
}

__device__ __forceinline__ uint64_t hash_at(const uint8_t* __restrict__ s, int i, int kk, const uint64_t* tab) {
  uint64_t f = 0, r = 0;
  for (int j = 0; j < kk; j++) {
    f = rol1(f) ^ tab[s[i + j]];
    r = rol1(r) ^ tab[s[i + kk - 1 - j] & 7];
  }
  return f < r ? f : r;
}

// the first base of query r as the k-mer kernels read it (o1 = offs[r]): in place, or a window's view into its read (K1Args::src)
__device__ __forceinline__ const uint8_t* k1_bases(const K1Args& a, uint32_t r, uint64_t o1) { return a.seqs + (a.src ? a.src[r] : o1); }

}  // namespace kmcpg
