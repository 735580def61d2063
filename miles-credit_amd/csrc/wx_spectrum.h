// Zonal power spectra on the device: the per-latitude DFT along longitude of
//   credit/losses/gen_1/power.py::PSDLoss            get_psd (the zonal power spectral density) and forward (a latitude-weighted
//                                                    distance between log-PSDs beyond a wavenumber)
//   credit/losses/gen_1/spectral.py::SpectralLoss2D  the distance between latitude-mean amplitude spectra beyond a wavenumber
// One handle per grid (H, W) with an optional float32 latitude weight table w[H]; a call acts on P planes of a field a (plane p at
// p * stride, float32 [H][W]) and optionally of a second field b of the same shape.  Wh = W / 2 + 1, X_k = sum_x r[x] e^{-2 pi i k x / W},
// mult_k = 1 for k = 0 and 2 for every other bin -- the Nyquist bin of an even W included, the reference's convention:
//   psd[p][h][k]      = mult_k |X_k|^2 / W^2                                    float32 [P][H][Wh], rounded once from fp64
//   mean_psd[p][k]    = sum_h what_h psd[p][h][k],  what = w / sum(w), 1 / H without weights          fp64 [P][Wh]
//   mean_amp[p][k]    = (sum_h w_h |X_k|) / H      (SpectralLoss2D divides by H, not by sum(w))        fp64 [P][Wh]
//   scores[p][0]      = mean_{k >= k_init} sum_h what_h (log(psd_a + 1e-8) - log(psd_b + 1e-8))^2      PSDLoss per plane
//   scores[p][1]      = mean_{k >= k_init} (mean_amp_a[k] - mean_amp_b[k])^2                           SpectralLoss2D per plane
// The reference's scalar losses are the means of the scores over the planes (every plane has the same element count).
//
// Launch 1, spectrum_rows_kernel: the transform, the squares and the row sums; no complex intermediate touches memory.
//   dft     the folded forward transform of wx_dft.h (dft_rows_folded: tile, fold, LDS twiddle table and sum order are stated there).
//           The lane that holds re of (row, k) holds im as well, so |X|^2 needs no exchange.  With b, four more accumulators transform
//           the matching rows of b with the same twiddles and the log difference is formed in registers; the prefetch of the next K
//           chunk is what hides the loads at two waves per SIMD.  A workgroup is four waves on 64 consecutive rows of ONE plane.
//   sums    per (plane, k) five sums over the workgroup's rows, fp64: w psd_a, w psd_b, w |X_a|, w |X_b|, w (log difference)^2 -- in a
//           thread over its four rows ascending, in a wave over the four lane groups (wave_sum_groups of wx_reduce.h), in the workgroup
//           over the waves 0, 1, 2, 3 -- written to the workgroup's own slot.  No atomics.
// Launch 2, spectrum_finish_kernel: one workgroup per plane adds the row-tile slots in ascending order, divides, and sums the two
// scores over k (thread-strided ascending, then block_sum_waves).
// An output depends on its own plane only and every sum has one fixed order: a plane's result is bit-identical whatever P, the split
// of the planes into calls or the plane's position; psd_a is the same with and without b.  The slots are the handle's scratch, grown
// only by a call with more tiles than any before; calls on one handle must be ordered by one stream.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "wx_common.h"
#include "wx_dft.h"
#include "wx_reduce.h"

namespace wx {

constexpr int kSpecSums = 5;          // w psd_a, w psd_b, w |X_a|, w |X_b|, w (log psd_a - log psd_b)^2
constexpr double kSpecLogEps = 1e-8;  // PSDLoss.forward
constexpr size_t kSpecReduceBytes = (size_t)(kDftTileRows / kDftWaveRows) * 2 * kSpecSums * 16 * sizeof(double);

struct SpecTiles {
  int Wh, row_tiles, col_blocks;
};

// ---- host-only helpers (no HIP call) ---------------------------------------------------------------------------------------------
inline SpecTiles spectrum_tiles(int H, int W) {
  const int Wh = W / 2 + 1;
  return {Wh, (H + kDftTileRows - 1) / kDftTileRows, (Wh + kDftTileCols - 1) / kDftTileCols};
}
inline int64_t spectrum_slot_doubles(int H, int W, int64_t n_planes) {
  const SpecTiles t = spectrum_tiles(H, W);
  return n_planes * t.row_tiles * kSpecSums * t.Wh;
}
inline size_t spectrum_lds_bytes(int W) { return std::max(dft_lds_bytes(W), kSpecReduceBytes); }

// "" or the reason wx_spectrum_create refuses.
inline std::string spectrum_check_create(int H, int W, const float* lat_w) {
  if (H < 2 || W < 2) return "H and W must be >= 2, got " + std::to_string(H) + " x " + std::to_string(W);
  if (W > kDftMaxN) return "W must be <= " + std::to_string(kDftMaxN) + " (the twiddle table lies in LDS), got " + std::to_string(W);
  if ((int64_t)H * W > 2147483647LL) return "H * W is beyond 2^31 - 1";
  if (lat_w) {
    double sum = 0.0;
    for (int h = 0; h < H; ++h) {
      if (!std::isfinite(lat_w[h]) || lat_w[h] < 0.f) return "a latitude weight must be finite and >= 0, row " + std::to_string(h) + " is not";
      sum += (double)lat_w[h];
    }
    if (!(sum > 0.0)) return "the latitude weights sum to zero";
  }
  return "";
}

// "" or the reason wx_spectrum_apply refuses, decided on the host before anything is launched.
inline std::string spectrum_check_apply(int H, int W, int n_planes, const float* a, int64_t a_stride, const float* b, int64_t b_stride, int k_init,
                                        const float* psd_a, const float* psd_b, const double* mean_psd_a, const double* mean_psd_b,
                                        const double* mean_amp_a, const double* mean_amp_b, const double* scores) {
  const int64_t hw = (int64_t)H * W;
  const SpecTiles t = spectrum_tiles(H, W);
  if (n_planes < 1) return "n_planes must be >= 1, got " + std::to_string(n_planes);
  if (!a) return "the field a is a null pointer";
  if (scores && !b) return "the scores compare two fields: a scores pointer needs b";
  if (!b && (psd_b || mean_psd_b || mean_amp_b)) return "an output of b needs b";
  if (!psd_a && !psd_b && !mean_psd_a && !mean_psd_b && !mean_amp_a && !mean_amp_b && !scores) return "no output requested: every output pointer is null";
  if (k_init < 0 || k_init >= t.Wh) return "k_init must be in 0 .. W / 2 = " + std::to_string(t.Wh - 1) + ", got " + std::to_string(k_init);
  if ((int64_t)n_planes * t.row_tiles * t.col_blocks > 2147483647LL) return "n_planes takes the call beyond 2^31 - 1 tiles";
  if (a_stride < hw || (b && b_stride < hw)) return "a plane stride is smaller than H * W = " + std::to_string(hw);
  const auto far = [&](const float* p, int64_t s) {      // the planes' extent must be a number the overlap tests can work with
    int64_t v = 0;
    return p && (__builtin_mul_overflow((int64_t)(n_planes - 1), s, &v) || __builtin_add_overflow(v, hw, &v) || v > (1LL << 44));
  };
  if (far(a, a_stride) || far(b, b_stride)) return "a plane stride takes the planes beyond 2^44 floats";
  struct Range { const void* p; int64_t bytes; };
  const Range in[2] = {{a, ((int64_t)(n_planes - 1) * a_stride + hw) * 4}, {b, b ? ((int64_t)(n_planes - 1) * b_stride + hw) * 4 : 0}};
  const int64_t psd_bytes = (int64_t)n_planes * H * t.Wh * 4, mean_bytes = (int64_t)n_planes * t.Wh * 8;
  const Range out[7] = {{psd_a, psd_bytes},      {psd_b, psd_bytes},      {mean_psd_a, mean_bytes},          {mean_psd_b, mean_bytes},
                        {mean_amp_a, mean_bytes}, {mean_amp_b, mean_bytes}, {scores, (int64_t)n_planes * 2 * 8}};
  for (int i = 0; i < 7; ++i) {
    if (!out[i].p) continue;
    for (int j = 0; j < 2; ++j)
      if (in[j].p && bytes_overlap(out[i].p, out[i].bytes, in[j].p, in[j].bytes)) return "an output overlaps an input field";
    for (int j = 0; j < i; ++j)
      if (out[j].p && bytes_overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes)) return "two outputs overlap";
  }
  return "";
}

// ---- device side -------------------------------------------------------------------------------------------------------------------
struct SpecRowsArgs {
  const float* a;
  const float* b;
  int64_t a_stride, b_stride;
  const float* w;      // device [H] or nullptr
  float* psd_a;
  float* psd_b;
  double* slots;       // [P][row_tiles][kSpecSums][Wh]
  int H, W, row_tiles, col_blocks;
};

// Launch 1.  grid = P * row_tiles * col_blocks (column block fastest), LDS spectrum_lds_bytes(W): the table, then the waves' sums.
template <bool HAS_B>
__global__ __launch_bounds__(256) void spectrum_rows_kernel(SpecRowsArgs s, const double2* __restrict__ tab_g) {
  extern __shared__ double2 spectrum_lds[];
  const int H = s.H, W = s.W, Wh = W / 2 + 1;
  dft_stage_table(spectrum_lds, tab_g, W);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int cb = (int)(blockIdx.x % (unsigned)s.col_blocks);
  const int tile = (int)(blockIdx.x / (unsigned)s.col_blocks);
  const int rt = tile % s.row_tiles;
  const int64_t p = tile / s.row_tiles;
  const int h0 = rt * kDftTileRows + wave * kDftWaveRows, k0 = cb * kDftTileCols;
  const bool live = h0 < H;                              // wave-uniform; a wave past the plane keeps zeros and meets the barriers
  constexpr int NF = HAS_B ? 2 : 1;                      // the fields: a, then b
  f64x4_t re[NF][2] = {}, im[NF][2] = {};
  const auto &re_a = re[0], &im_a = im[0], &re_b = re[NF - 1], &im_b = im[NF - 1];
  if (live) {
    const int row = h0 + c;
    const bool row_ok = row < H;
    const float* rows[NF];
    rows[0] = s.a + p * s.a_stride + (int64_t)(row_ok ? row : 0) * W;
    if (HAS_B) rows[NF - 1] = s.b + p * s.b_stride + (int64_t)(row_ok ? row : 0) * W;
    dft_rows_folded<NF, float>(rows, row_ok, W, k0, spectrum_lds, re, im);
  }
  // the lane's elements: rows h0 + g + 4 r, wavenumbers k0 + 16 t + c
  double sums[2][kSpecSums] = {};
  if (live) {
    const double w2 = (double)W * (double)W;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int k = k0 + 16 * t + c;
      const double mult = k == 0 ? 1.0 : 2.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int h = h0 + g + 4 * r;
        if (h < H && k < Wh) {
          const double wv = s.w ? (double)s.w[h] : 1.0;
          const int64_t o = (p * H + h) * Wh + k;
          const double pa = dft_power(re_a[t][r], im_a[t][r]);
          const double psda = mult * pa / w2;
          if (s.psd_a) s.psd_a[o] = (float)psda;
          sums[t][0] += wv * psda;
          sums[t][2] += wv * sqrt(pa);
          if (HAS_B) {
            const double pb = dft_power(re_b[t][r], im_b[t][r]);
            const double psdb = mult * pb / w2;
            if (s.psd_b) s.psd_b[o] = (float)psdb;
            const double d = log(psda + kSpecLogEps) - log(psdb + kSpecLogEps);
            sums[t][1] += wv * psdb;
            sums[t][3] += wv * sqrt(pb);
            sums[t][4] += wv * (d * d);
          }
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) wave_sum_groups<kSpecSums>(sums[t]);   // lanes 0 .. 15: the wave's sums of column c
  __syncthreads();                                       // every wave is through with the table: its memory takes the sums
  double* red = (double*)spectrum_lds;                   // [wave][t][sum][c]
  if (lane < 16) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int i = 0; i < kSpecSums; ++i) red[((wave * 2 + t) * kSpecSums + i) * 16 + c] = sums[t][i];
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * kSpecSums * 16) {
    const int t = threadIdx.x / (kSpecSums * 16), i = (threadIdx.x / 16) % kSpecSums, cc = threadIdx.x & 15;
    const int k = k0 + 16 * t + cc;
    if (k < Wh && (HAS_B || i == 0 || i == 2)) {
      double v = red[((0 * 2 + t) * kSpecSums + i) * 16 + cc];
      for (int wv = 1; wv < kDftTileRows / kDftWaveRows; ++wv) v += red[((wv * 2 + t) * kSpecSums + i) * 16 + cc];
      s.slots[(((p * s.row_tiles + rt) * kSpecSums) + i) * Wh + k] = v;
    }
  }
}

struct SpecFinishArgs {
  const double* slots;
  int Wh, row_tiles, k_init, has_b;
  double wsum, rows;   // sum(w) (H without weights) and H
  double* mean_psd_a;
  double* mean_psd_b;
  double* mean_amp_a;
  double* mean_amp_b;
  double* scores;
};

// Launch 2.  grid = P, one workgroup of 256 per plane.
__global__ __launch_bounds__(256) void spectrum_finish_kernel(SpecFinishArgs f) {
  __shared__ double s_red[4][2];
  const int64_t p = blockIdx.x;
  const int Wh = f.Wh;
  double acc[2] = {0.0, 0.0};
  for (int k = threadIdx.x; k < Wh; k += 256) {
    double s[kSpecSums] = {};
    for (int rt = 0; rt < f.row_tiles; ++rt) {           // the row tiles in ascending order
      const double* slot = f.slots + ((p * f.row_tiles + rt) * kSpecSums) * Wh + k;
      s[0] += slot[0];
      s[2] += slot[2 * (int64_t)Wh];
      if (f.has_b) {
        s[1] += slot[Wh];
        s[3] += slot[3 * (int64_t)Wh];
        s[4] += slot[4 * (int64_t)Wh];
      }
    }
    const double amp_a = s[2] / f.rows;
    if (f.mean_psd_a) f.mean_psd_a[p * Wh + k] = s[0] / f.wsum;
    if (f.mean_amp_a) f.mean_amp_a[p * Wh + k] = amp_a;
    if (f.has_b) {
      const double amp_b = s[3] / f.rows;
      if (f.mean_psd_b) f.mean_psd_b[p * Wh + k] = s[1] / f.wsum;
      if (f.mean_amp_b) f.mean_amp_b[p * Wh + k] = amp_b;
      if (k >= f.k_init) {
        const double d = amp_a - amp_b;
        acc[0] += s[4] / f.wsum;
        acc[1] += d * d;
      }
    }
  }
  if (f.scores) {
    const double v = block_sum_waves<2, 256>(acc, s_red);
    if (threadIdx.x < 2) f.scores[p * 2 + threadIdx.x] = v / (double)(Wh - f.k_init);
  }
}

class Spectrum {
 public:
  Spectrum(int H_, int W_, const float* lat_w_host, int dev) : H(H_), W(W_), device(dev), mem(dev) {
    WX_HIP(hipSetDevice(device));
    std::vector<double2> t;
    dft_table(W, t);
    tab = mem.upload(t.data(), t.size());
    wsum = (double)H;
    if (lat_w_host) {
      w = mem.upload(lat_w_host, (size_t)H);
      wsum = 0.0;
      for (int h = 0; h < H; ++h) wsum += (double)lat_w_host[h];
    }
  }

  void apply(int n_planes, const float* a, int64_t a_stride, const float* b, int64_t b_stride, int k_init, float* psd_a, float* psd_b,
             double* mean_psd_a, double* mean_psd_b, double* mean_amp_a, double* mean_amp_b, double* scores, hipStream_t stream) {
    const std::string why =
        spectrum_check_apply(H, W, n_planes, a, a_stride, b, b_stride, k_init, psd_a, psd_b, mean_psd_a, mean_psd_b, mean_amp_a, mean_amp_b, scores);
    if (!why.empty()) throw std::runtime_error("wx_spectrum_apply: " + why);
    WX_HIP(hipSetDevice(device));
    const SpecTiles t = spectrum_tiles(H, W);
    mem.grow(slots, slots_have, (size_t)spectrum_slot_doubles(H, W, n_planes));
    SpecRowsArgs r;
    r.a = a; r.b = b; r.a_stride = a_stride; r.b_stride = b_stride; r.w = w; r.psd_a = psd_a; r.psd_b = psd_b; r.slots = slots;
    r.H = H; r.W = W; r.row_tiles = t.row_tiles; r.col_blocks = t.col_blocks;
    const dim3 grid((unsigned)((int64_t)n_planes * t.row_tiles * t.col_blocks));
    if (b) hipLaunchKernelGGL(spectrum_rows_kernel<true>, grid, dim3(256), spectrum_lds_bytes(W), stream, r, tab);
    else hipLaunchKernelGGL(spectrum_rows_kernel<false>, grid, dim3(256), spectrum_lds_bytes(W), stream, r, tab);
    WX_HIP(hipGetLastError());
    if (mean_psd_a || mean_psd_b || mean_amp_a || mean_amp_b || scores) {
      SpecFinishArgs f;
      f.slots = slots; f.Wh = t.Wh; f.row_tiles = t.row_tiles; f.k_init = k_init; f.has_b = b ? 1 : 0; f.wsum = wsum; f.rows = (double)H;
      f.mean_psd_a = mean_psd_a; f.mean_psd_b = mean_psd_b; f.mean_amp_a = mean_amp_a; f.mean_amp_b = mean_amp_b; f.scores = scores;
      hipLaunchKernelGGL(spectrum_finish_kernel, dim3((unsigned)n_planes), dim3(256), 0, stream, f);
      WX_HIP(hipGetLastError());
    }
  }

 private:
  int H, W, device;
  DeviceArena mem;
  double2* tab = nullptr;
  float* w = nullptr;
  double* slots = nullptr;
  size_t slots_have = 0;
  double wsum = 0.0;
};

}  // namespace wx
