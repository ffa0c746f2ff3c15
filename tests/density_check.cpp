// density_check.cpp — the per-lane pieces of k_density (kmcp_amd/csrc/density_core.hpp) compiled for the host: simulated waves of 64 lanes
// walk a random bit matrix segment by segment exactly as the kernel does (density_next_segment, dens_walk, the butterfly of
// dens_plane_add over the lanes that share 16 bytes, dens_expand_pass through the staging buffer), over the chunks of the kernel's own
// launch plan (plan_density, density_chunk_rows) or chunks given by the case, and the counts are compared with scalar counts of the same
// bits, MSB of a byte first (kmcp/cmd/index-density.go:177-185).  Cases: bins that end inside a group of 8 rows, segments cut at
// the planes' capacity, a short last bin, a sub-range that starts past row 0, chunks that cut bins into pieces.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../kmcp_amd/csrc/density_core.hpp"

using namespace kmcpg;

static uint64_t rng_state = 0x243f6a8885a308d3ULL;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static long wrong = 0, checked = 0, stores_over_nonzero = 0;

template <int LPR>
static void run_case(uint64_t n_rows, uint32_t nlanes, uint64_t first_row, uint64_t last_row, uint64_t bin_rows, uint64_t chunk_rows, int density_pct) {
  const uint64_t stride = (uint64_t)nlanes * 16;
  std::vector<uint8_t> rows(n_rows * stride);
  for (auto& b : rows) {
    uint8_t v = 0;
    for (int t = 0; t < 8; t++) v |= (uint8_t)(((int)(rnd() % 100) < density_pct) << t);
    b = v;
  }
  const uint64_t n = last_row - first_row, n_bins = n / bin_rows + (n % bin_rows ? 1 : 0);
  const uint32_t ntiles = (nlanes + LPR - 1) / LPR;
  const uint64_t width = (uint64_t)ntiles * LPR * 128;
  std::vector<uint32_t> out(n_bins * width, 0);
  constexpr int RPW = 64 / LPR;
  // chunk_rows == 0: the chunks of the kernel's own launch plan (plan_density + density_chunk_rows), else chunks of that many rows
  DensityArgs da{};
  da.first_row = first_row;
  da.last_row = last_row;
  da.bin_rows = bin_rows;
  uint64_t n_chunks = (n + std::max<uint64_t>(1, chunk_rows) - 1) / std::max<uint64_t>(1, chunk_rows);
  if (chunk_rows == 0) {
    const DensityPlan pl = plan_density(nlanes, n, bin_rows);
    if (pl.form != 0 || pl.lpr != LPR || pl.ntiles != ntiles || pl.width != width || pl.n_bins != n_bins || pl.n_chunks * pl.ntiles > kDensityUnits ||
        pl.workgroups != (pl.n_chunks * pl.ntiles + 3) / 4) {
      fprintf(stderr, "plan_density(%u, %llu, %llu): unexpected plan\n", nlanes, (unsigned long long)n, (unsigned long long)bin_rows);
      wrong++;
      return;
    }
    da.chunk_rows = pl.chunk_rows;
    da.pieces = pl.pieces;
    n_chunks = pl.n_chunks;
    // one chunk index past the grid: must be empty, not rows past the request
    uint64_t x0, x1;
    density_chunk_rows(da, n_chunks, x0, x1);
    if (x0 > last_row || x1 > last_row || (pl.pieces <= 1 && x0 != x1)) wrong++;
  }
  for (uint32_t tile = 0; tile < ntiles; tile++)
    for (uint64_t c = 0; c < n_chunks; c++) {
      uint64_t c0, c1;
      if (chunk_rows == 0) {
        density_chunk_rows(da, c, c0, c1);
      } else {
        c0 = first_row + c * chunk_rows;
        c1 = std::min(last_row, c0 + chunk_rows);
      }
      if (c0 < first_row || c1 > last_row || c0 > c1) {
        fprintf(stderr, "chunk %llu = rows %llu..%llu outside the request %llu..%llu\n", (unsigned long long)c, (unsigned long long)c0, (unsigned long long)c1,
                (unsigned long long)first_row, (unsigned long long)last_row);
        wrong++;
        continue;
      }
      uint64_t R = c0;
      while (R < c1) {
        const DensSeg g = density_next_segment(R, c1, first_row, last_row, bin_rows);
        std::vector<DensPlanes> P(64);
        for (int lane = 0; lane < 64; lane++) {
          dens_zero(P[lane]);
          const int l = lane % LPR, s = lane / LPR;
          const uint32_t gl = tile * LPR + l;
          if (gl < nlanes) dens_walk<LPR>(P[lane], rows.data() + (uint64_t)gl * 16, stride, s, R, g.hi);
        }
        for (int m = LPR; m < 64; m <<= 1) {
          std::vector<DensPlanes> Q(64);
          for (int lane = 0; lane < 64; lane++) Q[lane] = P[lane ^ m];
          for (int lane = 0; lane < 64; lane++) dens_plane_add(P[lane], Q[lane]);
        }
        typedef DensForm<LPR> F;
        uint32_t* o = out.data() + g.bin * width + (uint64_t)tile * LPR * 128;
        for (int q = 0; q < F::PASSES; q++) {
          std::vector<uint32_t> stage(F::STAGE_WORDS, 0xdeadbeefu);
          for (int lane = 0; lane < 64; lane++) {
            uint32_t cnt[F::PC];
            dens_expand_pass<LPR>(P[lane], lane / LPR, q, cnt);
            for (int j = 0; j < F::PC; j++) stage[dens_stage_slot<LPR>(lane, j)] = cnt[j];
          }
          for (int k = 0; k < F::PC; k++)
            for (int lane = 0; lane < 64; lane++) {
              int L, j;
              uint32_t tc;
              dens_stage_read<LPR>(k * 64 + lane, q, L, j, tc);
              const uint32_t v = stage[dens_stage_slot<LPR>(L, j)];
              if (tile * (uint32_t)LPR + tc / 128u >= nlanes) continue;
              if (g.whole) {
                if (o[tc]) stores_over_nonzero++;
                o[tc] = v;
              } else {
                o[tc] += v;
              }
            }
        }
        (void)RPW;
        R = g.hi;
      }
    }
  // scalar recount
  for (uint64_t b = 0; b < n_bins; b++) {
    const uint64_t r0 = first_row + b * bin_rows, r1 = bin_rows > last_row - r0 ? last_row : r0 + bin_rows;
    for (uint32_t col = 0; col < nlanes * 128; col++) {
      uint32_t want = 0;
      for (uint64_t r = r0; r < r1; r++) want += (rows[r * stride + col / 8] >> (7 - col % 8)) & 1u;
      checked++;
      if (out[b * width + col] != want) {
        if (wrong < 10)
          fprintf(stderr, "LPR %d rows %llu..%llu bin_rows %llu chunk %llu: bin %llu col %u: %u != %u\n", LPR, (unsigned long long)first_row,
                  (unsigned long long)last_row, (unsigned long long)bin_rows, (unsigned long long)chunk_rows, (unsigned long long)b, col, out[b * width + col], want);
        wrong++;
      }
    }
  }
}

template <int LPR>
static void run_form() {
  constexpr uint64_t STEP = 8 * (64 / LPR);
  const uint32_t full = LPR, part = LPR == 4 ? 1 : LPR / 2 + 1, two = LPR <= 16 ? 2 * LPR + 3 : LPR;
  // bins that end inside a group of 8 rows of a lane, and a short last bin
  run_case<LPR>(3 * STEP + 5, full, 0, 3 * STEP + 5, STEP + 3, 1 << 20, 50);
  run_case<LPR>(1000, part, 0, 1000, 257, 1 << 20, 30);
  // several tiles, the last one narrower than LPR lanes
  run_case<LPR>(700, two, 0, 700, 300, 1 << 20, 10);
  // a sub-range with first_row > 0 that ends in the middle of a bin
  run_case<LPR>(900, full, 37, 37 + 2 * 256 + 100, 256, 1 << 20, 50);
  // one bin over all rows, longer than the planes' capacity: segments of DENS_SEG_ROWS rows are added up (all ones: the largest counts)
  run_case<LPR>(2 * DENS_SEG_ROWS + 77, LPR == 64 ? 3 : 1, 0, 2 * DENS_SEG_ROWS + 77, 2 * DENS_SEG_ROWS + 77, 1ull << 40, 100);
  run_case<LPR>(DENS_SEG_ROWS + 9, 1, 0, DENS_SEG_ROWS + 9, DENS_SEG_ROWS + 10, 1ull << 40, 97);
  // chunks that are whole bins, and chunks that cut bins into pieces
  run_case<LPR>(2048, full, 0, 2048, 256, 512, 50);
  run_case<LPR>(2100, part, 0, 2100, 1000, 8 * STEP, 50);
  // the kernel's own launch plan: bins shorter than a step of the form, bins cut into pieces, many bins per chunk, a bin larger than the range
  for (uint64_t br : {(uint64_t)256, (uint64_t)300, (uint64_t)1000, (uint64_t)2999, (uint64_t)3000, (uint64_t)3001, ~(uint64_t)0}) {
    run_case<LPR>(3010, part, 3, 3003, br, 0, 50);
    run_case<LPR>(3000, LPR == 64 ? 130 : full, 0, 3000, br, 0, 20);  // (the plan takes the narrowest form that covers the lanes: several tiles only at 64)
  }
  run_case<LPR>(4 * DENS_SEG_ROWS, LPR == 64 ? 65 : full, 0, 4 * DENS_SEG_ROWS, 4 * DENS_SEG_ROWS, 0, 100);
  // short bins go through the same code when asked to (the kernel takes the other form below DENS_SMALL_BIN)
  run_case<LPR>(300, part, 3, 290, 7, 70, 50);
  run_case<LPR>(130, 1, 0, 130, 1, 1 << 20, 50);
}

int main() {
  static_assert(dens_bit_of_col(0) == 7 && dens_bit_of_col(7) == 0 && dens_bit_of_col(8) == 15 && dens_bit_of_col(31) == 24, "MSB of a byte is its first column");
  run_form<4>();
  run_form<8>();
  run_form<16>();
  run_form<32>();
  run_form<64>();
  // the segment rule by itself
  {
    DensSeg g = density_next_segment(10, 1000, 10, 600, 256);
    if (!(g.bin == 0 && g.hi == 266 && g.whole)) wrong++;
    g = density_next_segment(522, 1000, 10, 600, 256);
    if (!(g.bin == 2 && g.hi == 600 && g.whole)) wrong++;  // the short last bin
    g = density_next_segment(300, 400, 10, 600, 256);
    if (!(g.bin == 1 && g.hi == 400 && !g.whole)) wrong++;
    g = density_next_segment(0, 1ull << 40, 0, 10000, 10001);
    if (!(g.bin == 0 && g.hi == DENS_SEG_ROWS && !g.whole)) wrong++;
    checked += 4;
  }
  printf("density_check: %ld counts checked, %ld wrong, %ld stores over a non-zero count\n", checked, wrong, stores_over_nonzero);
  return wrong || stores_over_nonzero ? 1 : 0;
}
