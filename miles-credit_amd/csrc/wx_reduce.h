// The one fixed-order fp64 reduction of the verification metrics (wx_metrics.h), the ensemble verification (wx_ensemble.h), the wind
// filter's amplitude sums (wx_wind.h) and the conservation fixers (wx_post.h), and the row tiling of a plane that the first two share.
//
// Why no atomics.  Floating-point addition is not associative and the order in which atomics land differs from run to run, so a sum
// made with them changes its last bits between two calls on the same input.  Every sum here is instead made in an order that the
// shapes alone decide:
//   in a thread    whatever the caller's loop does (thread-strided over the tile, or over the slots of an earlier launch: sum_slots)
//   in a wave      wave_sum: a shuffle-down tree 32, 16, .. 1 -- lane i adds lane i + off -- the result in lane 0
//                  (wave_sum_groups: its steps 32 and 16 alone, one result per lane position 0 .. 15)
//   in a workgroup either block_sum_waves: wave_sum, then the waves added 0, 1, 2, .. by one thread per sum
//                  or     block_sum_tree:  a halving tree 128, 64, .. 1 over 256 threads in LDS -- thread i adds thread i + half
//   across workgroups  each writes its sums to a slot of its own; a LATER launch adds the slots with the pieces above.  No hand-off
//                  inside a launch, and nothing to clear: every slot read was written by the launch before.
// An edit to any of these orders changes the last bits of every operator at once, never of one alone.
//
// Row tiling.  A plane [H][W] is cut into blocks of `rows` whole rows: at most kTileRows rows and kTileElems elements (always at least
// one row); the last block is short where rows does not divide H.  One workgroup of kTileThreads owns one tile = (plane, row block),
// row block fastest.  A tile's rows are contiguous, and the row weight w[h] (1 without weights) is staged into LDS once per tile.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>

namespace wx {

constexpr int kTileRows = 8;
constexpr int kTileElems = 8192;
constexpr int kTileThreads = 256;

struct RowTiles {
  int H, W, rows, row_blocks;
};

// ---- host-only helpers (no HIP call) ---------------------------------------------------------------------------------------------
inline RowTiles row_tiles(int H, int W) {
  const int rows = std::max(1, std::min(std::min(kTileRows, H), kTileElems / W));
  return {H, W, rows, (H + rows - 1) / rows};
}

// "" or the reason a handle on an H x W grid with latitude weights lat_w ([H] on the host, or null) is refused
inline std::string grid_check(int H, int W, const float* lat_w) {
  if (H < 1 || W < 1 || (int64_t)H * W > 2147483647LL) return "bad geometry";
  if (lat_w)
    for (int h = 0; h < H; ++h)
      if (!std::isfinite(lat_w[h])) return "non-finite latitude weight at row " + std::to_string(h);
  return "";
}

// ---- device side -------------------------------------------------------------------------------------------------------------------
struct RowTile {
  int plane, h0, rows, n;   // plane within the variable; first row, rows and elements of this block
  int64_t offset;           // of the block's first element in its plane
};

// tile `local` of a variable (its tiles counted from 0)
__device__ __forceinline__ RowTile row_tile(int local, const RowTiles& g) {
  RowTile t;
  t.plane = local / g.row_blocks;
  t.h0 = (local - t.plane * g.row_blocks) * g.rows;
  t.rows = min(g.rows, g.H - t.h0);
  t.n = t.rows * g.W;
  t.offset = (int64_t)t.h0 * g.W;
  return t;
}

// s_w[kTileRows] = the weights of rows h0 .. h0 + rows - 1 (1 without weights and past the block); ends in the barrier
__device__ __forceinline__ void stage_row_weights(float* s_w, const float* __restrict__ w, int h0, int rows) {
  if (threadIdx.x < kTileRows) s_w[threadIdx.x] = (w && (int)threadIdx.x < rows) ? w[h0 + threadIdx.x] : 1.f;
  __syncthreads();
}

// acc[k] += slot i's k-th sum for i = thread, thread + THREADS, ..: the slots [n][K] that an earlier launch wrote
template <int K, int THREADS>
__device__ __forceinline__ void sum_slots(const double* __restrict__ slots, int n, double (&acc)[K]) {
  for (int i = threadIdx.x; i < n; i += THREADS) {
    const double* s = slots + (size_t)i * K;
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] += s[k];
  }
}

// the K sums of the wave in lane 0
template <int K>
__device__ __forceinline__ void wave_sum(double (&acc)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc[k] += __shfl_down(acc[k], off, 64);
  }
}

// the K sums over the four 16-lane groups of the wave, per lane position: lane c < 16 ends with lanes c, c + 16, c + 32, c + 48 --
// the first two steps of wave_sum's tree (the rows of an MFMA accumulator column; wx_spectrum.h)
template <int K>
__device__ __forceinline__ void wave_sum_groups(double (&acc)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int off = 32; off >= 16; off >>= 1) acc[k] += __shfl_down(acc[k], off, 64);
  }
}

// returns sum k of the workgroup in thread k < K (0 in the others); s_red: [THREADS / 64][K]
template <int K, int THREADS>
__device__ __forceinline__ double block_sum_waves(double (&acc)[K], double (*s_red)[K]) {
  wave_sum<K>(acc);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) s_red[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x < K) {
    s = s_red[0][threadIdx.x];
    for (int wv = 1; wv < THREADS / 64; ++wv) s += s_red[wv][threadIdx.x];
  }
  return s;
}

// a workgroup of 256: sum k in sh[k][0], visible to every thread
template <int K>
__device__ __forceinline__ void block_sum_tree(const double (&s)[K], double (*sh)[256]) {
#pragma unroll
  for (int k = 0; k < K; ++k) sh[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int half = 128; half >= 1; half >>= 1) {
    if ((int)threadIdx.x < half) {
#pragma unroll
      for (int k = 0; k < K; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + half];
    }
    __syncthreads();
  }
}

}  // namespace wx
