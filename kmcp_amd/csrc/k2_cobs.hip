// k2_cobs.hip — K2: the COBS query: row = hash % NumSigs, gather rows, AND the h rows, per-column match counts in bit-sliced
// counters, integer threshold, hit emission (kmcp/cmd/util-db-search.go:6611-7742); SPLIT form + k_threshold_long for long
// queries.  The path is bitwise/integer and HBM-bound; there is no MFMA here by design.  wave = 64 lanes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "common.hpp"
#include "csa.hpp"
#include "device_utils.hpp"
#include "k2_claim.hpp"
#include "k2_short.hpp"
#include "kernels.hpp"

namespace kmcpg {

// ------------------------------------------------------------------------------------------------
// K2: the COBS query.
//
// Work unit = (read, slot) with slot = (group of resident blocks that share NumSigs, tile of LPR*16 bytes of its rows).  LPR
// lanes serve one unit, so a wave carries G = 64/LPR units: LPR = 64 for every whole KiB of a row (GTDB-scale: 1872 B), 32, 16, 8 or 4
// for what is left of it or for narrow rows (a lone 312-column block has 39-byte rows, `kmcp index -b 1024` gives 128-byte ones).  Units are numbered slot-major: all
// waves in flight gather from one (group, tile) slice of the index.  Each lane owns 16 bytes = 128 columns of its unit's rows
// and keeps their match counts as NPL bit-sliced planes (vertical counters): the rows of a group of GR = 8 (or 4) are reduced
// with a carry-save adder tree and the carry word rippled into the upper planes, ~4 VALU ops per loaded dword, which keeps the
// kernel memory-bound; after every group the sectors whose columns cannot reach the threshold any more stop
// loading (exact branch and bound).
// Row indices of a chunk of CH k-mers are computed cooperatively (one exact fastmod per (k-mer, block), fastmod.hpp) into a
// per-wave LDS table — hash loads of the whole chunk first, block constants from LDS: no dependent global loads in that loop;
// k-mers past the end of a read map to the all-zero row appended to each block, so the inner loop has no tail code.
// ------------------------------------------------------------------------------------------------
// 16 bytes of a row.  Index rows are read once per launch and L2 cannot hold a slice (cache note): non-temporal
// loads keep them from displacing the hash/offset lines in L2 (no measurable difference either way in the kernel).
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 load_row16(const uint8_t* p, int nt) {
  const u32x4* q = reinterpret_cast<const u32x4*>(p);
  const u32x4 v = nt ? __builtin_nontemporal_load(q) : *q;
  return make_uint4(v.x, v.y, v.z, v.w);
}

// the same through a pointer the compiler knows to be global memory (a row pointer read from a BlockDev record is a generic one to
// it: flat_load, whose completions cannot be counted in order — every wait becomes "all loads").  With global_load the adders of
// one row group wait for that group's loads only while the next group's are in flight.
typedef const u32x4 __attribute__((address_space(1))) * global_row_ptr;
__device__ __forceinline__ uint4 load_row16_global(const uint8_t* p, int nt) {
  global_row_ptr q = (global_row_ptr)(uintptr_t)p;
  const u32x4 v = nt ? __builtin_nontemporal_load(q) : *q;
  return make_uint4(v.x, v.y, v.z, v.w);
}

// byte `byte` of a group's row, bit `bit` (7 = first column of the byte, index.go:1157) -> global column; false for padding
__device__ __forceinline__ bool group_col(const Seg* __restrict__ segs, const BlockDev* __restrict__ bd, uint32_t byte, uint32_t bit, uint32_t* col) {
  const Seg* s = segs + bd->seg0;
  for (uint32_t i = 0; i < bd->nsegs; i++, s++) {
    if (byte < s->byte_end) {
      const uint32_t c = (byte - s->byte_start) * 8u + (7u - bit);
      *col = s->col_base + c;
      return byte >= s->byte_start && c < s->ncols;
    }
  }
  return false;
}

// SPLIT = true is the long-query form: a unit is (long query, slot, chunk of a.split_chk <= 8192 k-mers); its counts are added to a
// per-query u32 array with atomics and thresholded by k_threshold_long, so a whole genome spreads over the chip instead
// of one wave per (query, slot).

// GR = rows gathered between two pruning tests: 8, or 4 where the launch waits for HBM (the host decides, k2_plan.hpp).  The
// short form is its own instantiation (4 rows in flight; 97 VGPRs, the 8-row form 91) built for at most 4 waves per SIMD: the kernel
// is bound by the L2->fabric path, not by latency (the 8-row form runs as fast at 2 waves per SIMD as at 5), and of the
// occupancy targets tried for the 4-row form this one is the fastest (GTDB scale: 488 ms; 506-510 ms at 5-6 waves, 510 ms at 3,
// starved at 2: profiles/r02_group_rows.txt).  That cap is for the 1-KB tiles only: with several units per wave (narrow rows, where
// a unit's lanes idle once its sector is dead) a fifth wave is worth 1-2 % (128-byte rows at 55 GB: 63.2 -> 62.3 ms).
struct alignas(16) UnitConst {  // one (read, slot) unit as the index phase sees it
  uint64_t ns, mh;  // NumSigs of the slot's block and its fastmod constant
  uint64_t koff;    // first hash of the read (of this chunk of it: SPLIT)
  uint32_t s16;     // row pitch in 16-byte units
  int32_t n;        // k-mers of the read handled by this unit
};

// The body lives in k2_cobs_body.inc and is included twice: as the kernel k2_cobs (one launch = one lane form; the token stream the kernel
// has always had, so the tuned instantiations compile to the ISA they had) and as the device function k2_body, which k2_cobs_pair calls
// for each of its two lane forms.
template <int LPR, int NPL, bool MULTI, bool SPLIT, int GR = 8>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((NPL == 16 && !SPLIT && !MULTI && LPR >= 16) ? 3 : 1, (GR == 4 && LPR == 64) ? 4 : 10))) k2_cobs(const K2Args a) {
#define K2_BID blockIdx.x
#include "k2_cobs_body.inc"
#undef K2_BID
}

template <int LPR, int NPL, bool MULTI, bool SPLIT, int GR>
__device__ __forceinline__ void k2_body(const K2Args& a, const unsigned bid) {
#define K2_BID bid
#include "k2_cobs_body.inc"
#undef K2_BID
}

// A wave's end of the unit queue of a launch piece (k2_claim.hpp): the run in hand.  The same in every lane.
struct K2UnitQueue {
  static constexpr uint64_t NONE = ~0ull;  // no unit: the queue is dry
  unsigned long long* counter;
  uint64_t unit_base, units;
  int lane;
  uint64_t cur = 0, end = 0;
  __device__ __forceinline__ uint64_t take() {
    if (cur == end) {
      unsigned long long tk = 0;
      if (lane == 0) tk = atomicAdd(counter, (unsigned long long)K2_CLAIM_RUN);
      const uint64_t t = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)tk) |
                         ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(tk >> 32)) << 32);
      const K2Run r = k2_claim_run(t, unit_base, units, K2_CLAIM_RUN);
      cur = r.first;
      end = r.last;
      if (cur == end) return NONE;  // tickets ascend: every later run is empty too
    }
    return cur++;
  }
};

// The short-read unit (k2_short.hpp) as a persistent kernel: as many workgroups as the chip holds at once, and every WAVE takes its
// (read, slot) units from the piece's queue (k2_claim.hpp) in runs of K2_CLAIM_RUN until a run comes out empty — no wave waits for the
// other three of its workgroup before it gets new work (under the hardware dispatcher a workgroup's wave slots come back when its slowest
// wave is done, and units differ in length by what their sectors prove), and the kernel is correct on any grid.  A unit is what it is in
// k2_cobs<64, 8|10, false, false, 4>, one tile; the block's constants are loaded again only when the slot changes.
template <int NPL>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 4))) k2_cobs_persist(const K2Args a, const unsigned piece_workgroups, unsigned long long* __restrict__ queue) {
  constexpr int NMAX = K2_SHORT_NMAX<NPL>;  // every read of the launch fits
  __shared__ uint32_t s_all[4][K2_SHORT_ROW<NPL>];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool exact = (a.k2_flags & K2F_EXACT_STOP) != 0;

  K2UnitQueue q{queue, a.unit_base, k2_piece_units((uint64_t)a.n_reads * a.nslots, a.unit_base, piece_workgroups), lane};
  // the slot the wave works on
  uint32_t cur_sidx = 0xffffffffu, tb = 0, s16 = 0;
  const BlockDev* __restrict__ bd = nullptr;
  const uint8_t* __restrict__ tbase = nullptr;
  uint64_t ns = 0, mh = 0;
  bool lv0 = false;
  uint32_t g_rows = 0;    // 16-byte row loads this lane issued (profiling level 2)
  uint64_t g_hashes = 0;  // ... and the hashes of the wave's units
  for (;;) {
    const uint64_t u = q.take();
    if (u == K2UnitQueue::NONE) break;
    // the body's numbering (k2_cobs_body.inc), one unit per wave
    const uint32_t sidx = (uint32_t)(a.slot_major ? u / a.n_reads : u % a.nslots);
    const uint32_t r = (uint32_t)(a.slot_major ? u % a.n_reads : u / a.nslots);
    if (sidx != cur_sidx) {  // wave-uniform
      cur_sidx = sidx;
      const Slot slot = a.slots[sidx];
      bd = a.blocks + k2_uni(slot.block);
      const uint32_t stride = k2_uni(bd->stride);
      ns = k2_uni64(bd->num_sigs);
      mh = k2_uni64(bd->magic_hi);
      s16 = stride >> 4;  // rows are addressed in 16-byte units
      tb = (k2_uni(slot.tile) * 64u + (uint32_t)lane) * 16u;
      tbase = (const uint8_t*)k2_uni64((uint64_t)(uintptr_t)bd->rows) + tb;
      lv0 = tb < stride;
    }
    int n = (int)k2_uni((uint32_t)a.nk[r]);
    if ((a.split_min > 0 && n > a.split_min) || n > NMAX) n = 0;  // long queries are left to the SPLIT launch
    if (n == 0) continue;
    k2_short_index(a, r, ns, mh, s16, n, s_all[wave], lane);
    const uint32_t cmin = k2_uni(k2_short_cmin(a, n));
    const int cm = k2_short_clamp<NPL>(cmin);
    bool lv = lv0;
#define K2T_ROW s_all[wave]
#define K2T_BASE tbase
#define K2T_N n
#define K2T_CM cm
#include "k2_short_tile.inc"
#undef K2T_ROW
#undef K2T_BASE
#undef K2T_N
#undef K2T_CM
    g_hashes += (uint64_t)n;
    k2_emit_tile<NPL>(a, bd, r, tb, cmin, lv, cp, lane);
  }
  k2_short_account(a, blockIdx.x, g_rows, g_hashes, lane);
}

// Two lane forms of one database in ONE launch (long queries, round 6): the first `nba` workgroups are form A's (the 1-KiB tiles), the rest
// form B's (the remainder of the same rows).  A batch of 16 384 HiFi reads is five rounds of the chip on the 64-lane form and a round and a
// third on the 16-lane one: as two launches, the second waits for the last wave of the first and both end on a part-filled round; in one
// grid B's workgroups take the slots A's last waves free (same-box: K2 3.17 -> 3.04 ms).  The same on two streams worked in a fresh process
// and LOST 0.6 ms per batch in one that had created a dozen streams before (streams share hardware queues): profiles/r06_tail_mode.txt.
template <int LPRA, int LPRB, int NPL, bool MULTI>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((NPL == 16 && !MULTI) ? 3 : 1, 10))) k2_cobs_pair(const K2Args a, const K2Args b, const unsigned nba) {
  if (blockIdx.x < nba) k2_body<LPRA, NPL, MULTI, false, 8>(a, blockIdx.x);
  else k2_body<LPRB, NPL, MULTI, false, 8>(b, blockIdx.x - nba);
}

// Every K2 kernel is launched by launch_k2_form, launch_k2_pair_form or launch_k2_persist_form and nowhere else: the kernel's template
// arguments are the function's own, so the record a launch leaves in the log (kmcpg_last_k2_launches) cannot name another form than the
// one that ran.  nb: the workgroups of the piece; grid: those the kernel was launched on where they are not the same (the persistent kernel).
static void note_k2(K2Log* log, int kind, int lpr, int lprb, int npl, bool multi, int gr, unsigned nb, unsigned grid = 0) {
  if (!log) return;
  kmcpg_k2_launch r{};
  r.kind = kind;
  r.lpr = lpr;
  r.lprb = lprb;
  r.npl = npl;
  r.multi = multi ? 1 : 0;
  r.group_rows = gr;
  r.workgroups = nb;
  r.grid = grid ? grid : nb;
  log->push_back(r);
}

template <int LPR, int NPL, bool MULTI, bool SPLIT, int GR>
static void launch_k2_form(const K2Args& b, unsigned nb, hipStream_t st, K2Log* log) {
  hipLaunchKernelGGL((k2_cobs<LPR, NPL, MULTI, SPLIT, GR>), dim3(nb), dim3(256), 0, st, b);
  note_k2(log, SPLIT ? 1 : 0, LPR, 0, NPL, MULTI, GR, nb);
}

template <int LPRA, int LPRB, int NPL, bool MULTI>
static void launch_k2_pair_form(const K2Args& a, const K2Args& b, unsigned nba, unsigned nbb, hipStream_t st, K2Log* log) {
  hipLaunchKernelGGL((k2_cobs_pair<LPRA, LPRB, NPL, MULTI>), dim3(nba + nbb), dim3(256), 0, st, a, b, nba);
  note_k2(log, 2, LPRA, LPRB, NPL, MULTI, 8, nba + nbb);  // both halves are k2_body<..., 8>
}

// The persistent form of a piece of k2_cobs<64, NPL, false, false, 4>: the piece's units and its own counter on the grid k2_persist_grid
// names (k2_claim.hpp).  The record is the launched form's but for `grid`, the witness that this kernel ran: what the piece is, and how many
// workgroups share it.
template <int NPL>
static int launch_k2_persist_form(const K2Args& b, const K2Piece& pc, uint64_t piece, hipStream_t st, K2Log* log) {
  int dev = 0, cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k2_cobs_persist<NPL>, 256, 0) != hipSuccess || cus <= 0 || per_cu <= 0)
    return -1;
  const unsigned nb = k2_persist_grid(pc.workgroups, (unsigned)cus * (unsigned)per_cu, b.persist_wgs);
  hipLaunchKernelGGL((k2_cobs_persist<NPL>), dim3(nb), dim3(256), 0, st, b, pc.workgroups, b.unit_queue + piece * K2_QUEUE_PITCH);
  note_k2(log, 0, 64, 0, NPL, false, 4, pc.workgroups, nb);
  return 0;
}

// The launchers only launch: which kernel, on which grid, is the record's (k2_plan.hpp); they switch over it and visit its grid pieces.
template <int LPR, int NPL, bool SPLIT, int GR>
static int launch_k2_pieces(const K2Launch& l, const K2Args& a, hipStream_t st, K2Log* log) {
  K2Args b = a;
  for (uint64_t i = 0, n = k2_n_pieces(l); i < n; i++) {
    const K2Piece pc = k2_piece(l, i);
    b.unit_base = pc.unit_base;
    if (l.persist) {  // the plan's decision (k2_plan.hpp); the kernel exists for the two forms the plan names, and needs its queue
      if constexpr (LPR == 64 && NPL <= 10 && !SPLIT && GR == 4) {
        if (!b.unit_queue || launch_k2_persist_form<NPL>(b, pc, i, st, log) != 0) return -1;
        continue;
      }
      return -1;
    }
    if (l.multi)
      launch_k2_form<LPR, NPL, true, SPLIT, GR>(b, pc.workgroups, st, log);
    else
      launch_k2_form<LPR, NPL, false, SPLIT, GR>(b, pc.workgroups, st, log);
  }
  return 0;
}

// (The kernels stand in the code object in the order the functions below name them: the plain forms, the pairs, the chunked forms.)
template <int LPR>
static int launch_k2_plain_l(const K2Launch& l, const K2Args& a, hipStream_t st, K2Log* log) {
  const bool four = l.gr == 4;  // the 4-row kernels exist at 8 and 10 planes
  if (!four && l.gr != 8) return -1;
  switch (l.npl) {
    case 8: return four ? launch_k2_pieces<LPR, 8, false, 4>(l, a, st, log) : launch_k2_pieces<LPR, 8, false, 8>(l, a, st, log);
    case 10: return four ? launch_k2_pieces<LPR, 10, false, 4>(l, a, st, log) : launch_k2_pieces<LPR, 10, false, 8>(l, a, st, log);
    case 16: return four ? -1 : launch_k2_pieces<LPR, 16, false, 8>(l, a, st, log);
    case 24: return four ? -1 : launch_k2_pieces<LPR, 24, false, 8>(l, a, st, log);
    default: return -1;
  }
}

static int launch_k2_plain(const K2Launch& l, const K2Args& a, hipStream_t st, K2Log* log) {
  switch (l.lpr) {
    case 4: return launch_k2_plain_l<4>(l, a, st, log);
    case 8: return launch_k2_plain_l<8>(l, a, st, log);
    case 16: return launch_k2_plain_l<16>(l, a, st, log);
    case 32: return launch_k2_plain_l<32>(l, a, st, log);
    case 64: return launch_k2_plain_l<64>(l, a, st, log);
    default: return -1;
  }
}

template <int LPRB>
static int launch_k2_pair_l(const K2Launch& l, const K2Args& a, const K2Args& b, hipStream_t st, K2Log* log) {
  if (l.multi)
    launch_k2_pair_form<64, LPRB, 16, true>(a, b, l.nba, l.nbb, st, log);
  else
    launch_k2_pair_form<64, LPRB, 16, false>(a, b, l.nba, l.nbb, st, log);
  return 0;
}

// a pair record: the 64-lane form (args a) and a narrower one (args b) of the same batch in one grid, both from unit 0.  -1: a record
// this file has no kernel for
int launch_k2_pair(const K2Launch& l, const K2Args& a, const K2Args& b, hipStream_t st, K2Log* log) {
  if (l.kind != K2Kind::Pair || l.lpr != 64 || l.npl != 16 || l.gr != 8) return -1;
  switch (l.lprb) {
    case 32: return launch_k2_pair_l<32>(l, a, b, st, log);
    case 16: return launch_k2_pair_l<16>(l, a, b, st, log);
    case 8: return launch_k2_pair_l<8>(l, a, b, st, log);
    case 4: return launch_k2_pair_l<4>(l, a, b, st, log);
    default: return -1;
  }
}

// a plain or a chunked record, every piece of its grid; `a` complete but for unit_base.  -1: no kernel for the record
int launch_k2(const K2Launch& l, const K2Args& a, hipStream_t st, K2Log* log) {
  if (l.kind == K2Kind::Plain) return launch_k2_plain(l, a, st, log);
  if (l.kind != K2Kind::Split || l.npl != 16 || l.gr != 8) return -1;
  switch (l.lpr) {
    case 4: return launch_k2_pieces<4, 16, true, 8>(l, a, st, log);
    case 8: return launch_k2_pieces<8, 16, true, 8>(l, a, st, log);
    case 16: return launch_k2_pieces<16, 16, true, 8>(l, a, st, log);
    case 32: return launch_k2_pieces<32, 16, true, 8>(l, a, st, log);
    case 64: return launch_k2_pieces<64, 16, true, 8>(l, a, st, log);
    default: return -1;
  }
}

// queries with more than split_min k-mers: meta[0] = how many, meta[1] = their largest NumKmers
__global__ void k_list_long(const int32_t* __restrict__ nk, uint32_t n_reads, int32_t split_min, uint32_t* __restrict__ list, uint32_t* __restrict__ meta) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n_reads && nk[r] > split_min) {
    list[atomicAdd(&meta[0], 1u)] = r;
    atomicMax(&meta[1], (uint32_t)nk[r]);
  }
}

void launch_list_long(const int32_t* nk, uint32_t n_reads, int32_t split_min, uint32_t* list, uint32_t* meta, hipStream_t st) {
  if (n_reads == 0) return;
  hipLaunchKernelGGL(k_list_long, dim3((n_reads + 255) / 256), dim3(256), 0, st, nk, n_reads, split_min, list, meta);
}

// largest NumKmers of the batch (callers compare it with what the stated read length allows)
__global__ void k_max_nk(const int32_t* __restrict__ nk, uint32_t n_reads, unsigned long long* __restrict__ out) {
  int m = 0;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += gridDim.x * blockDim.x) m = max(m, nk[r]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = max(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(out, (unsigned long long)m);
}

void launch_max_nk(const int32_t* nk, uint32_t n_reads, unsigned long long* out, hipStream_t st) {
  if (n_reads == 0) return;
  const unsigned blocks = std::min<unsigned>(1024, (n_reads + 255) / 256);
  hipLaunchKernelGGL(k_max_nk, dim3(blocks), dim3(256), 0, st, nk, n_reads, out);
}

// threshold over the accumulated counts of the long queries (same integer rule as the k2_cobs epilogue); one atomic per wave
// and pass: the lanes that hold a hit get consecutive places (ballot + popcount of the lower lanes)
__global__ void k_threshold_long(const K2Args a) {
  const uint64_t total = (uint64_t)a.n_long * a.ncols_total;
  const int lane = threadIdx.x & 63;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < total; i0 += step) {  // wave-uniform trip count
    const uint64_t i = i0 + (uint64_t)lane;
    uint32_t c = 0, r = 0, col = 0;
    bool pass = false;
    if (i < total && (c = a.long_counts[i]) != 0) {
      const uint32_t li = (uint32_t)(i / a.ncols_total);
      col = (uint32_t)(i % a.ncols_total);
      r = a.long_list[li];
      const int n = a.nk[r];
      uint32_t cmin = count_threshold(n, a.min_qcov, a.min_matched);
      // the -f bound as in the plain kernel's epilogue: a query that took the chunked form because KMCPG_SPLIT_MIN is small is still
      // covered by the table (the host's trusted path for compact results relies on "n <= cmin_fpr_n => bound applied", whichever form ran)
      if (a.cmin_fpr && n <= a.cmin_fpr_n) cmin = max(cmin, (uint32_t)a.cmin_fpr[n]);
      pass = c >= cmin;
    }
    const uint64_t m = __ballot(pass);
    if (m == 0) continue;
    const int leader = __ffsll((unsigned long long)m) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(a.counter, (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    if (pass) {
      const unsigned long long idx = base + (unsigned long long)__popcll(m & ((1ULL << lane) - 1ULL));
      if (idx < a.hit_cap) {
        kmcpg_hit hit;
        hit.read = r;
        hit.col = col;
        hit.count = c;
        a.hits[idx] = hit;
      }
    }
  }
}

void launch_threshold_long(const K2Args& a, hipStream_t st) {
  const uint64_t total = (uint64_t)a.n_long * a.ncols_total;
  if (total == 0) return;
  unsigned blocks = (unsigned)((total + 255) / 256 > 65536 ? 65536 : (total + 255) / 256);
  hipLaunchKernelGGL(k_threshold_long, dim3(blocks), dim3(256), 0, st, a);
}

}  // namespace kmcpg
