// density.hip — index inspection: set bits per (column, row bin) of resident rows, at streaming rate.  The reference counts them
// in one thread, one byte per step down the mapped file (kmcp/cmd/index-density.go:171-213).
//
//   k_density<LPR>      bins of >= DENS_SMALL_BIN rows: carry-save bit planes per lane (density_core.hpp), one wave per (tile of LPR
//                       16-byte lanes, chunk of rows); counts land bin-major, out[bin][column of the lane range]
//   k_density_small     shorter bins (down to one row): one thread per (bin, dword), 32 counters, bit extracts
//   k_density_transpose out[bin][col] -> the ABI's counts[col][bin] for the columns of one block (its byte offset in a group's row applied)
//   k_density_cols      one bin over all rows of a group -> ones[global column] through the group's Seg table
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "density_core.hpp"
#include "kernels.hpp"

namespace kmcpg {

namespace {

// 128 VGPRs at most: 16 waves per CU, each with 8 KiB of loads in flight
template <int LPR>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_density(DensityArgs a) {
  typedef DensForm<LPR> F;
  __shared__ uint32_t stage[4][F::STAGE_WORDS];  // one staging buffer per wave: waves never wait for each other
  const int lane = (int)(threadIdx.x & 63u);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  volatile uint32_t* st = stage[wave];
  const uint64_t unit = (uint64_t)blockIdx.x * 4u + (uint64_t)wave;
  const uint32_t tile = (uint32_t)(unit % a.ntiles);  // neighbouring waves read neighbouring tiles of the same rows
  const uint64_t chunk = unit / a.ntiles;
  if (chunk >= a.n_chunks) return;
  uint64_t R, c1;
  density_chunk_rows(a, chunk, R, c1);
  const int l = lane % LPR, s = lane / LPR;
  const uint32_t gl = tile * (uint32_t)LPR + (uint32_t)l;  // 16-byte lane of the requested range
  const bool active = gl < a.nlanes;                       // the last tile may be narrower than LPR lanes
  const uint8_t* lane_ptr = a.rows + ((uint64_t)a.lane0 + gl) * 16u;
  while (R < c1) {
    const DensSeg g = density_next_segment(R, c1, a.first_row, a.last_row, a.bin_rows);
    DensPlanes P;
    dens_zero(P);
    if (active) dens_walk<LPR>(P, lane_ptr, a.stride, s, R, g.hi);
    // lanes with the same l hold the same 16 bytes of different rows: butterfly over s, every lane ends with the total
#pragma unroll
    for (int m = LPR; m < 64; m <<= 1) {
      DensPlanes Q;
#pragma unroll
      for (int d = 0; d < 4; d++)
#pragma unroll
        for (int p = 0; p < DENS_NPL; p++) Q.p[d][p] = (uint32_t)__shfl_xor((int)P.p[d][p], m, 64);
      dens_plane_add(P, Q);
    }
    // counts out, 32 columns per lane and pass, through the wave's staging buffer: consecutive lanes write consecutive columns
    uint32_t* o = a.out + g.bin * a.width + (uint64_t)tile * (LPR * 128u);
#pragma unroll
    for (int q = 0; q < F::PASSES; q++) {
      uint32_t cnt[F::PC];
      dens_expand_pass<LPR>(P, s, q, cnt);
#pragma unroll
      for (int j = 0; j < F::PC; j++) st[dens_stage_slot<LPR>(lane, j)] = cnt[j];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll 4
      for (int k = 0; k < F::PC; k++) {
        int L, j;
        uint32_t tc;
        dens_stage_read<LPR>(k * 64 + lane, q, L, j, tc);
        const uint32_t v = st[dens_stage_slot<LPR>(L, j)];
        if (tile * (uint32_t)LPR + tc / 128u < a.nlanes) {
          if (g.whole) o[tc] = v;              // this wave alone counts the bin: plain stores
          else if (v) atomicAdd(o + tc, v);     // the bin is shared with other segments: integer adds, any order gives the same result
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    R = g.hi;
  }
}

__global__ __launch_bounds__(256) void k_density_small(DensityArgs a) {
  const uint64_t ndw = (uint64_t)a.nlanes * 4u;
  const uint64_t rows = a.last_row - a.first_row;
  const uint64_t nbins = (rows + a.bin_rows - 1) / a.bin_rows;
  const uint64_t total = nbins * ndw;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t b = i / ndw;
    const uint32_t w = (uint32_t)(i % ndw);
    const uint64_t r0 = a.first_row + b * a.bin_rows;
    const uint64_t r1 = a.bin_rows > a.last_row - r0 ? a.last_row : r0 + a.bin_rows;
    uint32_t cnt[32];
#pragma unroll
    for (int t = 0; t < 32; t++) cnt[t] = 0;
    const uint8_t* q = a.rows + (uint64_t)a.lane0 * 16u + (uint64_t)w * 4u;
    for (uint64_t r = r0; r < r1; r++) {
      const uint32_t x = *reinterpret_cast<const uint32_t*>(q + r * a.stride);
#pragma unroll
      for (int t = 0; t < 32; t++) cnt[t] += (x >> dens_bit_of_col(t)) & 1u;
    }
    uint4* o = reinterpret_cast<uint4*>(a.out + b * a.width + (uint64_t)w * 32u);
#pragma unroll
    for (int t = 0; t < 8; t++) o[t] = make_uint4(cnt[4 * t], cnt[4 * t + 1], cnt[4 * t + 2], cnt[4 * t + 3]);
  }
}

// in[b * width + col0 + c] -> out[c * nb + b], 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void k_density_transpose(const uint32_t* __restrict__ in, uint64_t width, uint32_t col0, uint32_t ncols, uint64_t nb,
                                                           uint32_t* __restrict__ out) {
  __shared__ uint32_t t[32][33];
  const uint64_t b0 = (uint64_t)blockIdx.x * 32u;
  const uint32_t c0 = blockIdx.y * 32u;
  const uint32_t tx = threadIdx.x & 31u, ty = threadIdx.x >> 5;
  for (uint32_t j = ty; j < 32; j += 8) {
    const uint64_t b = b0 + j;
    const uint32_t c = c0 + tx;
    t[j][tx] = (b < nb && c < ncols) ? in[b * width + col0 + c] : 0u;
  }
  __syncthreads();
  for (uint32_t j = ty; j < 32; j += 8) {
    const uint32_t c = c0 + j;
    const uint64_t b = b0 + tx;
    if (c < ncols && b < nb) out[(uint64_t)c * nb + b] = t[tx][j];
  }
}

// in = one bin over a whole group's row (lane 0 on): column c of member seg -> ones[seg.col_base + c]
__global__ void k_density_cols(const uint32_t* __restrict__ in, const Seg* __restrict__ segs, unsigned long long* __restrict__ ones) {
  const Seg sg = segs[blockIdx.y];
  for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < sg.ncols; c += gridDim.x * blockDim.x)
    ones[(uint64_t)sg.col_base + c] = in[(uint64_t)sg.byte_start * 8u + c];
}

// the yardstick of tools/bench_density.py: the same bytes read once with 16 B per lane and one XOR per load, nothing else
__global__ __launch_bounds__(256) void k_stream_probe(const uint8_t* __restrict__ buf, uint64_t n16, uint32_t* __restrict__ out) {
  DensU4 acc{{0, 0, 0, 0}};
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 7 * stride < n16; i += 8 * stride) {
    DensU4 v[8];
#pragma unroll
    for (int r = 0; r < 8; r++) v[r] = dens_load16(buf + (i + r * stride) * 16u);
#pragma unroll
    for (int r = 0; r < 8; r++)
#pragma unroll
      for (int d = 0; d < 4; d++) acc.v[d] ^= v[r].v[d];
  }
  for (; i < n16; i += stride) {
    const DensU4 v = dens_load16(buf + i * 16u);
#pragma unroll
    for (int d = 0; d < 4; d++) acc.v[d] ^= v.v[d];
  }
  if ((acc.v[0] ^ acc.v[1] ^ acc.v[2] ^ acc.v[3]) == 0x12345678u) out[0] = 1;  // keeps the loads alive
}

}  // namespace

void launch_stream_probe(const uint8_t* buf, uint64_t bytes, uint32_t* out, hipStream_t st) {
  if (bytes < 16) return;
  hipLaunchKernelGGL(k_stream_probe, dim3(8192), dim3(256), 0, st, buf, bytes / 16u, out);
}

int launch_density(const DensityPlan& p, DensityArgs a, hipStream_t st) {
  if (a.last_row <= a.first_row || a.bin_rows == 0 || a.nlanes == 0) return -1;
  a.width = p.width;
  if (p.form == 1) {
    const uint64_t total = p.n_bins * (uint64_t)a.nlanes * 4u;
    const unsigned blocks = (unsigned)std::min<uint64_t>((total + 255) / 256, 1u << 20);
    hipLaunchKernelGGL(k_density_small, dim3(blocks), dim3(256), 0, st, a);
    return 0;
  }
  a.ntiles = p.ntiles;
  a.chunk_rows = p.chunk_rows;
  a.pieces = p.pieces;
  a.n_chunks = p.n_chunks;
  if (p.workgroups == 0 || p.workgroups > 0x7fffffffULL) return -1;
  const dim3 grid((unsigned)p.workgroups), block(256);
  switch (p.lpr) {
    case 4: hipLaunchKernelGGL(k_density<4>, grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL(k_density<8>, grid, block, 0, st, a); break;
    case 16: hipLaunchKernelGGL(k_density<16>, grid, block, 0, st, a); break;
    case 32: hipLaunchKernelGGL(k_density<32>, grid, block, 0, st, a); break;
    case 64: hipLaunchKernelGGL(k_density<64>, grid, block, 0, st, a); break;
    default: return -1;
  }
  return 0;
}

void launch_density_transpose(const uint32_t* in, uint64_t width, uint32_t col0, uint32_t ncols, uint64_t nb, uint32_t* out, hipStream_t st) {
  if (ncols == 0 || nb == 0) return;
  hipLaunchKernelGGL(k_density_transpose, dim3((unsigned)((nb + 31) / 32), (ncols + 31) / 32), dim3(256), 0, st, in, width, col0, ncols, nb, out);
}

void launch_density_cols(const uint32_t* in, const Seg* segs, uint32_t nsegs, uint32_t max_ncols, uint64_t* ones, hipStream_t st) {
  if (nsegs == 0 || max_ncols == 0) return;
  hipLaunchKernelGGL(k_density_cols, dim3(std::min<uint32_t>((max_ncols + 255) / 256, 1024u), nsegs), dim3(256), 0, st, in, segs,
                     reinterpret_cast<unsigned long long*>(ones));
}

}  // namespace kmcpg
