// k1_seg.hip — K1, whole genomes (plain / FracMinHash k-mers): one workgroup per 65536-position segment of a genome, with rolling hashes on
// bytes (k1_seg_roll) or on 2-bit codes (k1_seg_roll2), the helpers of packed batches (k_mark_exc, k_unpack2_list) and the ordered pack
// (k1_seg_pack).  Forms SegRoll / SegRoll2 of launch_k1 (k1_kmers.hip) and the pack of SegHash; the first generation, k1_seg_hash, is made
// of the LDS tile machinery of the long-read kernels and lives with it in k1_reads.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "common.hpp"
#include "device_utils.hpp"
#include "k1_device.hpp"
#include "k1_launch.hpp"
#include "k1_plan.hpp"
#include "kernels.hpp"
#include "nthash.hpp"

namespace kmcpg {

// ---- whole genomes (plain / FracMinHash k-mers): segments of K1SEG positions on their own workgroups ----------------
// Pass 1 hashes a segment and compacts its kept hashes at scratch[offs[r] + seg*K1SEG ...]; pass 2 moves the segments of a
// read together in order (destination = sum of the counts of the earlier segments).
// (K1SEG: k1_plan.hpp; pass 1 in its first form, k1_seg_hash: k1_reads.hip)

// The same segments with ROLLING hashes (round 4).  The prefix-XOR form (k1_seg_hash) prices every k-mer at two 64-bit scans, four variable
// rotates and eight workgroup barriers per 1024 positions — ~150 lane-operations per base, 250 Gbase/s, which had become 42 % of a
// genome-search step.  A genome has what a read lacks: long runs.  Here every lane owns ROLL_L = 128 consecutive k-mer positions and
// rolls ntHash along them as the recurrence is meant to be used,
//     fh(i+1) = rol1(fh(i) ^ rol(F[i], k-1)) ^ F[i+k]        rh(i+1) = ror1(rh(i) ^ R[i] ^ rol(R[i+k], k)),
// after k steps of start-up: two byte look-ups and four seed look-ups (LDS) per k-mer and no cross-lane traffic at all.  A wave takes
// 64 x 128 = 8192 positions, a workgroup of 8 waves one K1SEG segment.  The bases of a wave's stretch are staged in LDS with the
// lanes' runs 132 bytes apart (the lanes walk their runs in step: a 128-byte pitch would put all of them on one bank).  Kept hashes
// must come out in position order, i.e. lane after lane: a first walk counts what each lane keeps (wave prefix sum, then the
// workgroup's over its 8 waves) and holds on to the first two hashes; a lane that kept more walks its run again to write them.  Same outputs as k1_seg_hash (out[], seg_cnt).
constexpr int ROLL_L = 128, ROLL_WAVES = 8, ROLL_PITCH = ROLL_L + 4, ROLL_HALO = 256;
static_assert(64 * ROLL_L * ROLL_WAVES == K1SEG, "a workgroup covers one segment");

__global__ void __launch_bounds__(64 * ROLL_WAVES) k1_seg_roll(const K1Args a) {
  // seeds, and the two rotated copies the recurrence asks for (a look-up instead of two variable 64-bit rotates per k-mer):
  // tab_out[b] = rol(F[b], k-1) leaves fh with the base that drops out, tab_in[b] = rol(R[b], k) enters rh with the new one
  __shared__ uint64_t tab[256], tab_out[256], tab_in[8];
  __shared__ __attribute__((aligned(16))) uint8_t bases[ROLL_WAVES][64 * ROLL_PITCH + ROLL_HALO];
  __shared__ int s_cnt[ROLL_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid < 256) {
    const uint64_t sd = seed_of(tid);
    tab[tid] = sd;
    tab_out[tid] = nt_tab_out(sd, a.k);
    if (tid < 8) tab_in[tid] = nt_tab_in(sd, a.k);
  }
  // As the fallback pass behind k1_seg_roll2 (seg_only_flagged) the launch is a small fixed grid that walks the LIST of segments that
  // kernel marked (a.seg_nflag entries of a.seg_list; none at all for a clean batch); alone, workgroup b takes segment b, once.
  const uint32_t n_todo = a.seg_only_flagged ? *a.seg_nflag : gridDim.x;
  for (uint32_t it = blockIdx.x; it < n_todo; it += gridDim.x) {
  const uint32_t bid = a.seg_only_flagged ? a.seg_list[it] : it;
  const uint32_t r = bid / a.segs_max, seg = bid % a.segs_max;
  const uint64_t o1 = a.offs[r];
  const int len = (int)(a.offs[r + 1] - o1);
  const int k = a.k;
  const int npos = len - k + 1;
  const int p_lo = (int)seg * K1SEG;
  const bool on = len >= a.min_qlen && p_lo < npos;  // (:778-786 gate; ErrShortSeq => no k-mers) — uniform over the workgroup
  const int P0 = p_lo + w * 64 * ROLL_L;             // first position of this wave
  const int wpos = on ? max(0, min(npos - P0, 64 * ROLL_L)) : 0;  // positions of this wave
  uint8_t* __restrict__ B = bases[w];
  auto at = [&](int q) -> int { return (q / ROLL_L) * ROLL_PITCH + (q % ROLL_L); };
  if (wpos > 0) {
    const uint8_t* __restrict__ s = k1_bases(a, r, o1) + P0;
    const int nb = wpos + k - 1;  // bases this wave needs (k <= 128, the launcher checks: they end inside the 65th run slot)
    // 16 bases per lane and turn (a 16-byte piece at a multiple of 16 never crosses the end of a 128-byte run, so it stays in one
    // piece in LDS too; the source is wherever the read starts: unaligned loads), then what is left byte by byte
    typedef uint32_t u32x4_any __attribute__((ext_vector_type(4), aligned(1)));
    const int nb16 = nb & ~15;
    for (int g = lane * 16; g < nb16; g += 64 * 16) {
      const u32x4_any v = *reinterpret_cast<const u32x4_any*>(s + g);
      uint32_t* d = reinterpret_cast<uint32_t*>(B + at(g));
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    for (int g = nb16 + lane; g < nb; g += 64) B[at(g)] = s[g];
  }
  __syncthreads();  // tab[] and the staged bases
  const bool scaled = a.scaled != 0;
  const uint64_t max_hash = a.max_hash;
  const int q0 = lane * ROLL_L;
  const int mine = max(0, min(wpos - q0, ROLL_L));  // k-mer positions of this lane
  // one walk over the lane's run; `emit(h)` sees the kept hashes in position order
  auto walk = [&](auto&& emit) {
    if (mine <= 0) return;
    uint64_t fh = 0, rh = 0;
    for (int j = 0; j < k; j++) {  // start-up (hash_at): fh = XOR_j rol(F[j], k-1-j), rh = XOR_j rol(R[j], j)
      nt_start_step(fh, rh, B[at(q0 + j)], j, tab);
    }
    const uint8_t* __restrict__ run = B + lane * ROLL_PITCH;  // the lane's own 128 bases; what follows them starts 4 bytes later
    for (int t = 0;; t++) {
      const uint64_t h = fh < rh ? fh : rh;
      if (h != 0 && (!scaled || h <= max_hash)) emit(h);
      if (t + 1 >= mine) break;
      const int ti = t + k;  // < 256: k <= 128
      const uint8_t bo = run[t], bi = run[ti + ((ti >> 7) << 2)];
      nt_roll_step(fh, rh, bo, bi, tab, tab_out, tab_in);
    }
  };
  // (a FracMinHash database keeps one hash in hundreds: the first two a lane keeps stay in registers, and the second walk is only
  // taken by a lane that kept more — every lane of an unscaled query, hardly any of a scaled one)
  int c = 0;
  uint64_t h0 = 0, h1 = 0;
  walk([&](uint64_t h) {
    if (c == 0) h0 = h;
    else if (c == 1) h1 = h;
    c++;
  });
  // where this lane's hashes go: behind those of the lower lanes of its wave and of the lower waves of the workgroup
  int incl = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off);
    if (lane >= off) incl += t;
  }
  if (lane == 63) s_cnt[w] = incl;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int i = 0; i < ROLL_WAVES; i++) {
    const int ci = s_cnt[i];
    if (i < w) before += ci;
    total += ci;
  }
  if (c > 0) {
    uint64_t* __restrict__ out = a.scratch + o1 + p_lo + before + (incl - c);
    if (c <= 2) {
      out[0] = h0;
      if (c == 2) out[1] = h1;
    } else {
      int i = 0;
      walk([&](uint64_t h) { out[i++] = h; });
    }
  }
  if (tid == 0) a.seg_cnt[bid] = total;
  __syncthreads();  // bases[] and s_cnt[] are free for the next segment of the list
  }
}

// The same segments once more (round 5), on 2-BIT CODES.  k1_seg_roll above spends ~60 lane-operations per base, most of them on getting
// at its operands: two byte look-ups in LDS with their address arithmetic, four 64-bit table look-ups with theirs.  A genome is A, C, G, T
// almost everywhere, and for those four letters (either case) everything the recurrence needs is a function of two 2-bit codes:
//     fh' = rol1(fh) ^ F2[out][in],   F2[o][i] = rol1(rol(F[o], k-1)) ^ F[i]          rh' = ror1(rh ^ R2[out][in]),   R2[o][i] = R[o] ^ rol(R[i], k)
// Here a wave converts its stretch of bases to codes while it stages them (16 bases per lane and step: (w >> 1) & 3 per byte, one multiply
// folds four codes into a byte, one v_perm rebuilds the canonical letters to check that nothing else was there) into 2 KB of LDS instead
// of 8.4 KB of bytes; a lane then takes its codes 16 at a time from one dword, the incoming ones from a funnel shift of two (the
// offset k is the same for every group), and a roll costs two bit-field extracts, one table address, two look-ups and the 64-bit
// arithmetic: ~22 operations per base.  A segment that holds ANY other byte (N, IUPAC codes, U: their hashes depend on the exact byte)
// is left to k1_seg_roll: this kernel marks it (seg_cnt = -1) and the launcher runs the byte kernel behind it for the marked segments only.
// Same outputs as k1_seg_roll / k1_seg_hash (out[], seg_cnt): tests/test_gpu_parity.py::test_k1_all_forms_across_k and the fuzz sweeps.
// A lane walks R2_L = 256 consecutive positions (round 6; 128 before): what a lane pays once per run — the k start-up steps, its share of
// the scans and of the copy-out — is paid half as often, and a workgroup is 4 waves for the same segment and the same LDS.  512 (2 waves
// per workgroup: half the waves per SIMD) executes the same number of instructions 15 % slower; table indices from two bit-field shifts
// per roll instead of the nibble words: +5 % instructions (profiles/r06_roll2_min.txt).
#ifndef KMCPG_R2_L
#define KMCPG_R2_L 256
#endif
constexpr int R2_L = KMCPG_R2_L, R2_WAVES = K1SEG / (64 * R2_L), R2_G = R2_L / 16;  // positions per lane, waves per workgroup, code words per lane run
constexpr int R2_KEEP = R2_L > 256 ? 6 : R2_L > 128 ? 4 : 2;  // kept hashes a lane holds in registers (a FracMinHash lane keeps R2_L / scale of them: more is a second walk)
static_assert(64 * R2_L * R2_WAVES == K1SEG, "a workgroup covers one segment");
constexpr int R2_PITCH = R2_G + 1;             // dwords per lane run (+ 1: an odd pitch puts the lanes' j-th words on different banks)
constexpr int R2_RUNS = 64 + (9 + R2_G - 1) / R2_G;  // 64 runs + the 9 words that k - 1 <= 127 further bases and the funnel's upper word reach into
constexpr int R2_WORDS = R2_RUNS * R2_PITCH;

__global__ void __launch_bounds__(64 * R2_WAVES) k1_seg_roll2(const K1Args a) {
  // one block of LDS with the pair tables in front: their addresses — table index x 8 — then fit the offset fields of one ds_read2_b64
  // and the walk's inner loop needs no base address (an add per roll)
  struct Sh {
    uint64_t F2[16], R2[16];  // the two pair tables
    uint64_t S[4], RC[4];     // seeds by code (A 0, C 1, T 2, G 3 = (ascii >> 1) & 3), complements
    uint32_t codes[R2_WAVES][R2_WORDS];
    int s_cnt[R2_WAVES];
    int s_bad;
  };
  __shared__ __attribute__((aligned(16))) Sh sh;
  uint64_t* const F2 = sh.F2;
  uint64_t* const R2 = sh.R2;
  uint64_t* const S = sh.S;
  uint64_t* const RC = sh.RC;
  int* const s_cnt = sh.s_cnt;
  int& s_bad = sh.s_bad;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int k = a.k;
  if (tid < 16) {
    F2[tid] = nt2_f2(tid >> 2, tid & 3, k);
    R2[tid] = nt2_r2(tid >> 2, tid & 3, k);
    if (tid < 4) {
      nt2_fill_seeds(S, RC, tid);
    }
  }
  if (tid == 0) s_bad = 0;
  const uint32_t r = blockIdx.x / a.segs_max, seg = blockIdx.x % a.segs_max;
  const uint64_t o1 = a.offs[r];
  const int len = (int)(a.offs[r + 1] - o1);
  const int npos = len - k + 1;
  const int p_lo = (int)seg * K1SEG;
  const bool on = len >= a.min_qlen && p_lo < npos;  // (:778-786 gate; ErrShortSeq => no k-mers) — uniform over the workgroup
  const int P0 = p_lo + w * 64 * R2_L;               // first position of this wave
  const int wpos = on ? max(0, min(npos - P0, 64 * R2_L)) : 0;  // positions of this wave
  uint32_t* __restrict__ Wd = sh.codes[w];
  auto slot = [&](int word) -> int { return (word / R2_G) * R2_PITCH + (word % R2_G); };  // word = base / 16 within the wave's stretch
  __syncthreads();  // s_bad = 0 before anybody raises it
  if (a.codes) {
    // the batch came as 2-bit codes: 16 of them are the 32 bits at bit 2 G of the packed stream (G = the word's first base in the batch) —
    // two dwords and a funnel shift; a foreign byte among the segment's bases has been noted per segment by k_mark_exc
    const uint32_t* __restrict__ C32 = reinterpret_cast<const uint32_t*>(a.codes);
    const uint64_t G0 = o1 + (uint64_t)P0;
    const int nb = wpos > 0 ? wpos + k - 1 : 0;  // bases this wave needs
    for (int gi = lane; gi < R2_G * R2_RUNS; gi += 64) {
      const int b0 = gi * 16;
      uint32_t word = 0;
      if (b0 < nb) {
        const uint64_t G = G0 + (uint64_t)b0;
        const uint64_t d = G >> 4;
        const uint32_t sh = 2u * (uint32_t)(G & 15u);
        const uint32_t lo = C32[d], hi = C32[d + 1];  // (the device copy of the codes ends 16 bytes behind the last base)
        word = nt2_funnel(hi, lo, sh);
        if (b0 + 16 > nb) word &= (1u << (2 * (nb - b0))) - 1u;  // what follows belongs to the next query
      }
      Wd[slot(gi)] = word;
    }
    if (tid == 0 && a.seg_exc && a.seg_exc[blockIdx.x]) s_bad = 1;
  } else {
    const uint8_t* __restrict__ s = k1_bases(a, r, o1) + P0;
    const int nb = wpos > 0 ? wpos + k - 1 : 0;  // bases this wave needs
    typedef uint32_t u32x4_any __attribute__((ext_vector_type(4), aligned(1)));
    bool bad = false;
    for (int gi = lane; gi < R2_G * R2_RUNS; gi += 64) {  // every word the walks may touch gets a value (zero past the stretch)
      const int b0 = gi * 16;
      uint32_t word = 0;
      if (b0 + 16 <= nb) {
        const u32x4_any v = *reinterpret_cast<const u32x4_any*>(s + b0);
        const uint32_t in[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int d = 0; d < 4; d++) {
          const uint32_t c = nt2_codes4(in[d]);   // the code of each byte, in its byte
          bad |= !nt2_valid4(in[d], c);            // ... and back: anything but A/C/G/T in either case differs
          word |= nt2_fold4(c) << (8 * d);         // four codes into one byte
        }
      } else if (b0 < nb) {
        for (int j = 0; b0 + j < nb; j++) {
          const uint32_t ch = s[b0 + j], c = (ch >> 1) & 3u;
          bad |= (ch & 0xDFu) != (uint32_t)nt2_letter((int)c);
          word |= c << (2 * j);
        }
      }
      Wd[slot(gi)] = word;
    }
    if (__ballot(bad) != 0 && lane == 0) s_bad = 1;
  }
  __syncthreads();  // tables, codes, s_bad
  if (s_bad) {  // a byte that is not A/C/G/T: the byte kernel takes this segment
    if (tid == 0) {  // (-1 never reaches k1_seg_pack: the byte kernel, launched right behind over this list, overwrites it)
      a.seg_cnt[blockIdx.x] = -1;
      a.seg_list[atomicAdd(a.seg_nflag, 1u)] = blockIdx.x;
    }
    return;
  }
  const bool scaled = a.scaled != 0;
  const uint64_t max_hash = a.max_hash;
  const int q0 = lane * R2_L;
  const int mine = max(0, min(wpos - q0, R2_L));  // k-mer positions of this lane
  const int kw = k >> 4, ksh = 2 * (k & 15);
  const uint32_t mh_hi = (uint32_t)(max_hash >> 32);
  // SC = FracMinHash database (a constant inside the loops).  The filter `0 < h <= maxHash` (util-db-search.go:1072-1077) keeps one k-mer in
  // ~500 at scale 1000, so the 64-bit minimum and the two 64-bit compares of every step are replaced by a 32-bit test that a kept hash
  // must pass — the upper word of min(fh, rh) is min of the upper words — and only a step where some lane passes it computes h exactly.
  auto walk = [&](auto sc_tag, auto&& emit) __attribute__((always_inline)) {
    constexpr bool SC = decltype(sc_tag)::value;
    if (mine <= 0) return;
    // start-up: fh = XOR_j rol(F[j], k-1-j), rh = XOR_j rol(R[j], j) over the run's first k bases, a code word at a time; the reverse strand
    // is gathered as XOR_j ror(R[j], k-1-j) — one fixed rotate per base like the forward strand — and turned by k - 1 at the end
    uint64_t fh = 0, rh = 0;
    const int w_out = R2_G * lane;
    for (int j0 = 0; j0 < k; j0 += 16) {
      const uint32_t wd = Wd[slot(w_out + (j0 >> 4))];
      const int jn = min(16, k - j0);
      for (int j = 0; j < jn; j++) {
        const uint32_t c = (wd >> (2 * j)) & 3u;
        fh = nt2_rol1(fh) ^ S[c];
        rh = nt2_ror1(rh) ^ RC[c];
      }
    }
    rh = rolv(rh, k - 1);
    auto test = [&](uint64_t f, uint64_t r_) __attribute__((always_inline)) {
      if constexpr (SC) {
        const uint32_t fhi = (uint32_t)(f >> 32), rhi = (uint32_t)(r_ >> 32);
        uint32_t mn;  // (written out: the compiler folds the plain expression into the 64-bit compares below — six instructions for these two)
        asm("v_min_u32 %0, %1, %2" : "=v"(mn) : "v"(fhi), "v"(rhi));
        if (mn <= mh_hi) {
          const uint64_t h = f < r_ ? f : r_;
          if (h != 0 && h <= max_hash) emit(h);
        }
      } else {
        const uint64_t h = f < r_ ? f : r_;
        if (h != 0) emit(h);
      }
    };
    int t = 0;
    for (int g = 0; g < R2_G; g++) {
      const uint32_t outw = Wd[slot(w_out + g)];
      const uint32_t inw = nt2_funnel(Wd[slot(w_out + g + kw + 1)], Wd[slot(w_out + g + kw)], (uint32_t)ksh);
      // the table index of every roll of the group, a nibble each: (code going out << 2) | code coming in
      const uint32_t m[2] = {(nt2_spread(outw & 0xFFFFu) << 2) | nt2_spread(inw & 0xFFFFu), (nt2_spread(outw >> 16) << 2) | nt2_spread(inw >> 16)};
      if (mine - t >= 16) {
#pragma unroll
        for (int j = 0; j < 16; j++) {
          test(fh, rh);
          const uint32_t idx = (m[j >> 3] >> (4 * (j & 7))) & 15u;
          fh = nt2_rol1(fh) ^ F2[idx];
          rh = nt2_ror1(rh ^ R2[idx]);
        }
        t += 16;
        if (t >= mine) return;
      } else {
        for (int j = 0; t < mine; j++, t++) {
          test(fh, rh);
          const uint32_t idx = (m[j >> 3] >> (4 * (j & 7))) & 15u;
          fh = nt2_rol1(fh) ^ F2[idx];
          rh = nt2_ror1(rh ^ R2[idx]);
        }
        return;
      }
    }
  };
  int c = 0;
  uint64_t hk[R2_KEEP] = {};
  auto count2 = [&](uint64_t h) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < R2_KEEP; i++) hk[i] = c == i ? h : hk[i];  // (selects, not branches into an array on the stack)
    c++;
  };
  if (scaled) walk(std::true_type{}, count2);
  else walk(std::false_type{}, count2);
  int incl = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t_ = __shfl_up(incl, off);
    if (lane >= off) incl += t_;
  }
  if (lane == 63) s_cnt[w] = incl;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int i = 0; i < R2_WAVES; i++) {
    const int ci = s_cnt[i];
    if (i < w) before += ci;
    total += ci;
  }
  if (c > 0) {
    uint64_t* __restrict__ out = a.scratch + o1 + p_lo + before + (incl - c);
    if (c <= R2_KEEP) {
#pragma unroll
      for (int i = 0; i < R2_KEEP; i++)
        if (i < c) out[i] = hk[i];
    } else {
      int i = 0;
      auto store = [&](uint64_t h) __attribute__((always_inline)) { out[i++] = h; };
      if (scaled) walk(std::true_type{}, store);
      else walk(std::false_type{}, store);
    }
  }
  if (tid == 0) a.seg_cnt[blockIdx.x] = total;
}

// Packed whole-genome batches (a.codes): which segments hold a foreign byte, and the text of exactly those for the byte kernel.
// k_mark_exc: one thread per run of foreign bytes (positions count from the start of the batch; a run of equal bytes may continue from the
// end of one query into the next) -> seg_exc[(read, segment)] = 1 for every segment whose k-mers cover one of its bytes: segment g of a
// read owns the k-mer positions [g K1SEG, (g + 1) K1SEG), i.e. the bases [g K1SEG, (g + 1) K1SEG + k - 1).
__global__ void __launch_bounds__(256) k_mark_exc(const K1Args a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_exc) return;
  uint64_t pos = a.exc[i].pos;
  const uint64_t end = pos + a.exc[i].len;
  uint32_t lo = 0, hi = a.n_reads;  // the read r with offs[r] <= pos < offs[r + 1]: the last r with offs[r] <= pos
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.offs[mid] <= pos) lo = mid;
    else hi = mid;
  }
  uint32_t r = lo;
  while (pos < end && r < a.n_reads) {
    const uint64_t o1 = a.offs[r], o2 = a.offs[r + 1];
    if (pos >= o2) {  // (empty queries in between)
      r++;
      continue;
    }
    const uint64_t s = pos - o1, e = (end < o2 ? end : o2) - o1;  // the run's bases [s, e) of read r
    const uint64_t g_lo = s >= (uint64_t)(a.k - 1) ? (s - (uint64_t)(a.k - 1)) / K1SEG : 0, g_hi = (e - 1) / K1SEG;
    for (uint64_t g = g_lo; g <= g_hi && g < a.segs_max; g++) a.seg_exc[(uint64_t)r * a.segs_max + g] = 1u;
    pos = o2;
    r++;
  }
}

// the bases of the listed segments (k1_seg_roll2's list: the segments k_mark_exc marked) as text, four per packed byte and thread; a byte
// that straddles the segment's ends is expanded whole (its neighbours' bases get the value they have anyway); k_apply_exc behind this
// launch restores the foreign bytes, the byte kernel behind that reads the text
__global__ void __launch_bounds__(256) k_unpack2_list(const K1Args a) {
  constexpr uint32_t LUT = NT2_LETTERS;
  const uint32_t n_todo = *a.seg_nflag;
  for (uint32_t it = blockIdx.x; it < n_todo; it += gridDim.x) {
    const uint32_t bid = a.seg_list[it];
    const uint32_t r = bid / a.segs_max, seg = bid % a.segs_max;
    const uint64_t o1 = a.offs[r], o2 = a.offs[r + 1];
    const uint64_t g0 = o1 + (uint64_t)seg * K1SEG;
    uint64_t g1 = g0 + K1SEG + (uint64_t)(a.k - 1);
    if (g1 > o2) g1 = o2;
    if (g0 >= g1) continue;
    const uint64_t b0 = g0 >> 2, b1 = (g1 + 3) >> 2;  // packed bytes [b0, b1)
    for (uint64_t b = b0 + threadIdx.x; b < b1; b += blockDim.x) {
      const uint32_t byte = a.codes[b];
      uint32_t v = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) v |= ((LUT >> (8 * ((byte >> (2 * j)) & 3u))) & 0xffu) << (8 * j);
      reinterpret_cast<uint32_t*>(a.seqs_w)[b] = v;
    }
  }
}

__global__ void __launch_bounds__(256) k1_seg_pack(const K1Args a) {
  const uint32_t r = blockIdx.x / a.segs_max, seg = blockIdx.x % a.segs_max;
  const uint64_t o1 = a.offs[r];
  const int len = (int)(a.offs[r + 1] - o1);
  const int npos = len - a.k + 1;
  const int nsegs = npos > 0 ? (npos + K1SEG - 1) / K1SEG : 1;
  if ((int)seg >= nsegs) return;
  const int* __restrict__ sc = a.seg_cnt + (size_t)r * a.segs_max;
  int dest = 0;
  for (uint32_t t = 0; t < seg; t++) dest += sc[t];
  const int cnt = sc[seg];  // >= 0: a segment k1_seg_roll2 marked -1 has been redone by the byte kernel before this launch
  const uint64_t* __restrict__ src = a.scratch + o1 + (uint64_t)seg * K1SEG;
  uint64_t* __restrict__ dst = a.hashes + o1 + dest;
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) dst[i] = src[i];
  if ((int)seg == nsegs - 1 && threadIdx.x == 0) {
    a.nk_raw[r] = dest + cnt;
    a.nk1[r] = dest + cnt;
    a.qlen[r] = len;
  }
}

static void seg_roll_launch(const K1Args& a, unsigned grid, hipStream_t st, K1Log* log) {
  hipLaunchKernelGGL(k1_seg_roll, dim3(grid), dim3(64 * ROLL_WAVES), 0, st, a);
  k1_note(log, KMCPG_K1_SEG_ROLL, 0, 0, grid, 64 * ROLL_WAVES, 0);
}
static void seg_pack_launch(const K1Args& a, unsigned grid, hipStream_t st, K1Log* log) {
  hipLaunchKernelGGL(k1_seg_pack, dim3(grid), dim3(256), 0, st, a);
  k1_note(log, KMCPG_K1_SEG_PACK, 0, 0, grid, 256, 0);
}

void launch_k1_seg_pack(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log) { seg_pack_launch(a, p.grid, st, log); }

void launch_k1_seg_roll(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log) {
  seg_roll_launch(a, p.grid, st, log);
  seg_pack_launch(a, p.grid, st, log);
}

void launch_k1_seg_roll2(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log) {
  (void)hipMemsetAsync(a.seg_nflag, 0, sizeof(uint32_t), st);
  if (p.marks.len) {  // codes with runs of foreign bytes: the segments they reach are marked for the list ...
    (void)hipMemsetAsync(a.seg_exc, 0, p.marks.len * sizeof(uint32_t), st);
    hipLaunchKernelGGL(k_mark_exc, dim3((a.n_exc + 255) / 256), dim3(256), 0, st, a);
    k1_note(log, KMCPG_K1_MARK_EXC, 0, 0, (a.n_exc + 255) / 256, 256, 0);
  }
  hipLaunchKernelGGL(k1_seg_roll2, dim3(p.grid), dim3(64 * R2_WAVES), 0, st, a);  // 2-bit codes; lists the segments it cannot take
  k1_note(log, KMCPG_K1_SEG_ROLL2, 0, 0, p.grid, 64 * R2_WAVES, 0);
  if (p.marks.len) {  // ... and only those become text
    hipLaunchKernelGGL(k_unpack2_list, dim3(p.grid2), dim3(256), 0, st, a);
    k1_note(log, KMCPG_K1_UNPACK2_LIST, 0, 0, p.grid2, 256, 0);
    launch_apply_exc(a.exc, a.n_exc, a.seqs_w, st);
  }
  // the byte kernel does the listed segments: nothing but the read of one counter for a clean batch, where a launch over all segments
  // was up to 2^21 workgroups exiting at once
  if (p.list_fallback) seg_roll_launch(a, p.grid2, st, log);
  seg_pack_launch(a, p.grid, st, log);
}


}  // namespace kmcpg
