// density_core.hpp — the per-lane pieces of k_density (density.hip): ones per (column, row bin) of resident rows, what
// `kmcp utils index-density` counts one byte at a time (kmcp/cmd/index-density.go:171-213).
//
// A wave covers 64 / LPR consecutive rows of one tile of LPR 16-byte lanes per load; lane (s, l) = (lane / LPR, lane % LPR) owns
// bytes 16 l .. 16 l + 15 of the tile in rows R + s, R + s + 64 / LPR, ... and adds them to DENS_NPL bit planes per dword with the
// carry-save adders of csa.hpp.  Rows are walked in SEGMENTS: a segment ends where its bin ends, where the wave's chunk of rows
// ends, or after DENS_SEG_ROWS rows (the planes hold counts below 2^DENS_NPL).  At the end of a segment the lanes that hold
// the same 16 bytes of different rows add their planes (bit-sliced ripple-carry add, one cross-lane move per plane), each of
// them expands its share of the 128 columns to uint32 counts, and the counts go to out[bin][column] in column order.
// Host-compilable: tests/density_check.cpp walks simulated waves through the same functions (tests/test_density_cpu.py).
#pragma once
#include <stdint.h>
#include <string.h>

#include "csa.hpp"

namespace kmcpg {

constexpr int DENS_NPL = 12;                 // planes: a column's count within one segment stays below 4096
constexpr uint64_t DENS_SEG_ROWS = 3968;     // 31 * 128 rows: a multiple of every form's step of 8 * 64 / LPR rows
constexpr uint64_t DENS_SMALL_BIN = 256;     // bins of fewer rows take the bit-extract form (k_density_small)
static_assert(DENS_SEG_ROWS < (1ull << DENS_NPL), "a segment's count must fit the planes");

KMCPG_CSA_HD constexpr uint64_t dens_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
KMCPG_CSA_HD constexpr uint64_t dens_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

// ---- the launch plan (host) and the rows of a wave's chunk (device): one wave per (tile of LPR lanes, chunk of rows) ----------------------
constexpr uint64_t kDensityUnits = 4096;  // waves a launch of the carry-save form aims for
struct DensityPlan {
  int form;            // 0 carry-save planes, 1 bit extracts (bins below DENS_SMALL_BIN rows)
  int lpr, npl;        // form 0: lanes per row tile, planes
  uint32_t ntiles;     // form 0: tiles of lpr lanes
  uint64_t width;      // columns of one bin in `out`
  uint64_t n_bins;
  uint64_t chunk_rows, pieces, n_chunks;  // form 0: rows per wave; pieces a bin is cut into (1: whole bins per chunk)
  uint64_t workgroups;
};
struct DensityArgs {
  const uint8_t* rows;
  uint64_t stride;
  uint32_t lane0, nlanes;
  uint64_t first_row, last_row, bin_rows;
  uint32_t* out;
  uint64_t width;
  uint32_t ntiles;
  uint64_t chunk_rows, pieces, n_chunks;
};
// rows [c0, c1) of chunk c: whole bins per chunk (pieces == 1) or a bin cut into `pieces` chunks of chunk_rows rows; never past last_row,
// whatever the grid
KMCPG_CSA_HD void density_chunk_rows(const DensityArgs& a, uint64_t c, uint64_t& c0, uint64_t& c1) {
  if (a.pieces <= 1) {
    c0 = dens_min(a.last_row, a.first_row + c * a.chunk_rows);
    c1 = a.chunk_rows > a.last_row - c0 ? a.last_row : c0 + a.chunk_rows;
  } else {
    const uint64_t bin = c / a.pieces, piece = c % a.pieces;
    const uint64_t lo = dens_min(a.last_row, a.first_row + bin * a.bin_rows);
    const uint64_t bin_hi = a.bin_rows > a.last_row - lo ? a.last_row : lo + a.bin_rows;
    c0 = dens_min(bin_hi, lo + piece * a.chunk_rows);
    c1 = dens_min(bin_hi, c0 + a.chunk_rows);
  }
}

inline DensityPlan plan_density(uint32_t nlanes, uint64_t rows, uint64_t bin_rows) {
  DensityPlan p{};
  if (bin_rows > rows) bin_rows = rows + 1;  // one short bin: keeps the arithmetic below far from 2^64 (the kernel takes the caller's bin_rows)
  p.n_bins = rows / bin_rows + (rows % bin_rows ? 1 : 0);
  if (bin_rows < DENS_SMALL_BIN) {
    p.form = 1;
    p.width = (uint64_t)nlanes * 128u;
    return p;
  }
  p.form = 0;
  p.npl = DENS_NPL;
  p.lpr = nlanes <= 4 ? 4 : (nlanes <= 8 ? 8 : (nlanes <= 16 ? 16 : (nlanes <= 32 ? 32 : 64)));
  p.ntiles = (nlanes + (uint32_t)p.lpr - 1) / (uint32_t)p.lpr;
  p.width = (uint64_t)p.ntiles * (uint32_t)p.lpr * 128u;
  // One wave per (tile, chunk of rows), 8 loads of 16 B per lane in flight: a CU streams from HBM with about 32 KiB of loads in flight,
  // i.e. four such waves.  At most kDensityUnits waves per launch: 16 per CU, all resident at once — a few workgroups more would run as a
  // second round behind them (measured: 1 026 workgroups took 0.447 ms for what 1 010 did in 0.379 ms).  A chunk is a whole number of
  // bins where there are that many bins (every count is then a plain store); fewer, longer bins are cut into equal pieces.
  const uint64_t step = 8u * (64u / (uint32_t)p.lpr);
  const uint64_t units1 = p.n_bins * p.ntiles;  // waves with one bin per chunk
  if (units1 >= kDensityUnits) {
    const uint64_t m = (units1 + kDensityUnits - 1) / kDensityUnits;
    p.pieces = 1;
    p.chunk_rows = bin_rows * m;
    p.n_chunks = (p.n_bins + m - 1) / m;
  } else {
    uint64_t pieces = dens_min(kDensityUnits / units1, dens_max(1, dens_min(bin_rows, rows) / (8 * step)));
    uint64_t cr = bin_rows;
    if (pieces > 1) {
      cr = (bin_rows + pieces - 1) / pieces;
      cr = dens_min(bin_rows, (cr + step - 1) / step * step);  // whole steps per piece; never longer than the bin
    }
    p.chunk_rows = cr;
    p.pieces = (bin_rows + cr - 1) / cr;
    p.n_chunks = p.n_bins * p.pieces;
  }
  p.workgroups = (p.n_chunks * p.ntiles + 3) / 4;
  return p;
}


struct DensSeg {
  uint64_t bin;  // bin the segment's rows belong to (relative to first_row)
  uint64_t hi;   // one past its last row
  bool whole;    // the segment is the whole bin: its counts may be stored, not added
};
// the segment that starts at row R of a chunk ending at c1; bins of bin_rows rows from first_row, the last one cut at last_row
KMCPG_CSA_HD DensSeg density_next_segment(uint64_t R, uint64_t c1, uint64_t first_row, uint64_t last_row, uint64_t bin_rows) {
  DensSeg g;
  g.bin = (R - first_row) / bin_rows;
  const uint64_t lo = first_row + g.bin * bin_rows;
  const uint64_t bin_hi = bin_rows > last_row - lo ? last_row : lo + bin_rows;
  uint64_t hi = bin_hi < c1 ? bin_hi : c1;
  if (hi - R > DENS_SEG_ROWS) hi = R + DENS_SEG_ROWS;
  g.hi = hi;
  g.whole = R == lo && hi == bin_hi;
  return g;
}

struct DensU4 {
  uint32_t v[4];
};
struct DensPlanes {
  uint32_t p[4][DENS_NPL];  // [dword of the lane's 16 bytes][plane]
};

KMCPG_CSA_HD DensU4 dens_load16(const uint8_t* q) {
  DensU4 r;
#if defined(__HIP_DEVICE_COMPILE__)
  typedef uint32_t v4u __attribute__((ext_vector_type(4)));
  const v4u x = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(q));  // every row is read once
  r.v[0] = x.x;
  r.v[1] = x.y;
  r.v[2] = x.z;
  r.v[3] = x.w;
#else
  memcpy(r.v, q, 16);
#endif
  return r;
}

KMCPG_CSA_HD void dens_zero(DensPlanes& P) {
#pragma unroll
  for (int d = 0; d < 4; d++)
#pragma unroll
    for (int p = 0; p < DENS_NPL; p++) P.p[d][p] = 0;
}

// 8 rows: 7 adders per dword, then one carry of weight 8 ripples
KMCPG_CSA_HD void dens_add8(DensPlanes& P, const DensU4 (&x)[8]) {
#pragma unroll
  for (int d = 0; d < 4; d++) {
    const uint32_t e = csa8_low<DENS_NPL>(P.p[d], x[0].v[d], x[1].v[d], x[2].v[d], x[3].v[d], x[4].v[d], x[5].v[d], x[6].v[d], x[7].v[d]);
    ripple<DENS_NPL, 3>(P.p[d], e);
  }
}
// one row (the short end of a segment)
KMCPG_CSA_HD void dens_add1(DensPlanes& P, const DensU4& x) {
#pragma unroll
  for (int d = 0; d < 4; d++) ripple<DENS_NPL, 0>(P.p[d], x.v[d]);
}

// The rows R + s, R + s + RPW, ... below hi of one lane into its planes; lane_ptr = row 0 of the lane's 16 bytes.
template <int LPR>
KMCPG_CSA_HD void dens_walk(DensPlanes& P, const uint8_t* lane_ptr, uint64_t stride, int s, uint64_t R, uint64_t hi) {
  constexpr uint64_t RPW = 64 / LPR, STEP = 8 * RPW;
  for (; R + STEP <= hi; R += STEP) {
    const uint8_t* q = lane_ptr + (R + (uint64_t)s) * stride;
    DensU4 x[8];
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = dens_load16(q + (uint64_t)j * RPW * stride);
    dens_add8(P, x);
  }
  for (uint64_t r = R + (uint64_t)s; r < hi; r += RPW) dens_add1(P, dens_load16(lane_ptr + r * stride));
}

// A += B, plane by plane (two lanes' counts of the same columns; the sum stays below 2^DENS_NPL by the segment's length)
KMCPG_CSA_HD void dens_plane_add(DensPlanes& A, const DensPlanes& B) {
#pragma unroll
  for (int d = 0; d < 4; d++) {
    uint32_t carry = 0;
#pragma unroll
    for (int p = 0; p < DENS_NPL; p++) {
      uint32_t c2, sum;
      CSA3(c2, sum, A.p[d][p], B.p[d][p], carry);
      A.p[d][p] = sum;
      carry = c2;
    }
  }
}

// bit position of a dword (little endian: byte t in bits 8 t .. 8 t + 7) that holds column c of the dword's 32 columns, MSB of a byte first (index.go:1157)
KMCPG_CSA_HD constexpr int dens_bit_of_col(int c) { return 8 * (c / 8) + 7 - (c % 8); }

// Lane (s, l) expands its share of the lane's 128 columns — columns s * CPL .. s * CPL + CPL - 1, CPL = 128 / (64 / LPR) = 2 LPR — in
// PASSES passes of PC <= 32 columns (one dword's planes, or a byte-aligned part of one): pass q yields the counts of columns
// s * CPL + q * PC + j, j < PC.  The counts of a pass leave through a staging buffer of the wave (LDS on the device) so that
// consecutive lanes write consecutive columns: lane L puts count j at dens_stage_slot(L, j) (odd pitch: no bank conflicts), and
// element i = 0 .. 64 PC - 1 of the pass is read back from there in the order of the tile's columns (dens_stage_read).
template <int LPR>
struct DensForm {
  static constexpr int RPW = 64 / LPR, CPL = 2 * LPR, PC = CPL < 32 ? CPL : 32, PASSES = CPL / PC;
  static constexpr int STAGE_WORDS = 64 * (PC + 1);
};
template <int LPR>
KMCPG_CSA_HD void dens_expand_pass(const DensPlanes& P, int s, int q, uint32_t (&cnt)[DensForm<LPR>::PC]) {
  constexpr int CPL = DensForm<LPR>::CPL, PC = DensForm<LPR>::PC;
  const int d = (s * CPL + q * PC) / 32, sh = (s * CPL + q * PC) % 32;  // PC < 32: a byte-aligned part of one dword
  uint32_t pl[DENS_NPL];
#pragma unroll
  for (int p = 0; p < DENS_NPL; p++) {
    const uint32_t lo = (d & 1) ? P.p[1][p] : P.p[0][p], hi = (d & 1) ? P.p[3][p] : P.p[2][p];
    pl[p] = ((d & 2) ? hi : lo) >> sh;
  }
#pragma unroll
  for (int j = 0; j < PC; j++) {
    const int bit = dens_bit_of_col(j);
    uint32_t v = 0;
#pragma unroll
    for (int p = 0; p < DENS_NPL; p++) v |= ((pl[p] >> bit) & 1u) << p;
    cnt[j] = v;
  }
}
template <int LPR>
KMCPG_CSA_HD int dens_stage_slot(int L, int j) {
  return L * (DensForm<LPR>::PC + 1) + j;
}
// element i of pass q: the lane that counted it, its index there, and its column within the tile's LPR * 128 columns
template <int LPR>
KMCPG_CSA_HD void dens_stage_read(int i, int q, int& L, int& j, uint32_t& tile_col) {
  constexpr int RPW = DensForm<LPR>::RPW, CPL = DensForm<LPR>::CPL, PC = DensForm<LPR>::PC;
  j = i % PC;
  const int rest = i / PC, s = rest % RPW, l = rest / RPW;
  L = s * LPR + l;
  tile_col = (uint32_t)(l * 128 + s * CPL + q * PC + j);
}

}  // namespace kmcpg
