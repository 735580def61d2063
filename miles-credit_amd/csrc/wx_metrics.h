// Gen-2 verification metrics on the device: the eight per-variable scores of credit/metrics (common.py, anomaly.py) from one
// two-pass reduction over prediction, target and climatology:
//   credit/metrics/common.py:45-87     mse, mae, bias, rmse: mean(w d^2), mean(w |d|), mean(w d), sqrt(mse), d = p - t
//   credit/metrics/common.py:113-119   r2score = 1 - mean(w d^2) / (mean(w (t - tbar)^2) + 1e-12), tbar = mean(w t)
//   credit/metrics/common.py:184-191   log_variance_ratio = log10(mean(w (p - pbar)^2) + eps) - log10(mean(w (t - tbar)^2) + eps)
//   credit/metrics/anomaly.py:288-289  d_f = (p - c) - mean(w (p - c)), d_t = (t - c) - mean(w (t - c))
//   credit/metrics/anomaly.py:336-361  activity = sqrt(mean(w d_f^2) + 1e-12), acc = mean(w d_f d_t) / (activity sqrt(mean(w d_t^2) + 1e-12))
// Every mean is over ALL B L T H W elements of the variable and is NOT divided by the sum of the weights (the reference relies on w
// having mean 1 over latitude); w is w[h], or 1 without latitude weights.
//
// Numerics.  The centred second moments are never formed from raw moments: a surface pressure of 1e5 +- 800 Pa loses R2 at the 1e-5
// to 1e-3 level that way in float32.  Two reading passes instead: pass 1 sums w p, w t, w c (and the d sums, which need no centre),
// a finish launch adds each variable's tiles, pass 2 sums the squares and the product of the CENTRED values, a second finish launch
// adds them and forms the scores.  Every value is widened to fp64 when it is loaded and every sum and every score is fp64; float32
// appears at the eight outputs only.  About 10 fp64 FMAs per 12 loaded bytes is far below the vector fp64 rate of the chip, so
// both passes stay HBM-bound.
//
// Reproducibility.  Every sum is made in the fixed order of wx_reduce.h.  A workgroup owns one tile (variable, plane (b, l, t), block
// of `rows` rows) and writes its sums to its own slot of a scratch slab; the finish launch -- one workgroup per variable -- adds the
// slots of that variable.  A variable's tiles and their order depend on its own shape alone, so any grouping of variables into calls
// gives the same bits.  Four launches per call whatever n_vars is: partials 1, finish 1, partials 2, finish 2.
//
// Layout.  Variable v is [B][L_v][T_v][H][W] fp32 with contiguous batch items, read in place through (pointer, batch stride), channel
// slices included; the climatology is [L_v or 1][T_v or 1][H][W] through (pointer, level stride, time stride), shared by the batch.
// A tile's rows are contiguous, w[h] is one value per row (held in LDS), loads run along W: 16-byte loads when W % 4 == 0 and every
// plane base of the variable sits on 16 bytes (decided per variable on the host), scalar loads otherwise (odd W, a view that starts
// one float into its buffer).  A call without any climatology never touches that stream.
// One handle serves one stream at a time: the scratch slab is the handle's.  It grows (never shrinks) when a call has more tiles than
// any before; every other call allocates nothing.
#pragma once
#include <cmath>
#include <cstring>
#include <string>

#include "wx_common.h"
#include "wx_reduce.h"

namespace wx {

constexpr int kMetricsMaxVars = 32;
constexpr int kMetricsScores = 8;         // rmse, mse, mae, bias, r2score, log_variance_ratio, acc, activity
constexpr int kMetricsSums = 6;           // slots per tile (pass 1 uses 6, pass 2 uses 5) and per variable and pass in `sums`

struct MetricsVar {
  const float* pred;       // batch item b at pred + b * pred_bs: [L][T][H][W]
  const float* target;
  const float* clim;       // level l, time t at clim + l * clim_ls + t * clim_ts: [H][W]; null: no climatology
  int64_t pred_bs, target_bs, clim_ls, clim_ts;   // in floats
  int L, T;
  int tile0, ntiles;       // this variable's tiles: tile0 .. tile0 + ntiles - 1 = (plane, row block), row block fastest
  int vec, pad;            // vec: 16-byte loads
};

struct MetricsArgs {
  MetricsVar v[kMetricsMaxVars];
  const float* w;          // device [H], or null
  int n_vars, B;
  RowTiles g;
  double eps;
};

// ---- device side -------------------------------------------------------------------------------------------------------------------
// pass 1: acc = sum w p, sum w t, sum w c, sum w d, sum w |d|, sum w d^2
// pass 2: acc = sum w (p - pbar)^2, sum w (t - tbar)^2, sum w d_f^2, sum w d_t^2, sum w d_f d_t;  mu = pbar, tbar, mean(w (p - c)), mean(w (t - c))
template <int PASS, bool CLIM>
__device__ __forceinline__ void metrics_accumulate(double w, float pf, float tf, float cf, const double* mu, double* acc) {
  const double p = (double)pf, t = (double)tf;
  if (PASS == 1) {
    const double d = p - t;
    acc[0] = fma(w, p, acc[0]);
    acc[1] = fma(w, t, acc[1]);
    if (CLIM) acc[2] = fma(w, (double)cf, acc[2]);
    acc[3] = fma(w, d, acc[3]);
    acc[4] = fma(w, fabs(d), acc[4]);
    acc[5] = fma(w * d, d, acc[5]);
  } else {
    const double xp = p - mu[0], xt = t - mu[1];
    acc[0] = fma(w * xp, xp, acc[0]);
    acc[1] = fma(w * xt, xt, acc[1]);
    if (CLIM) {
      const double c = (double)cf;
      const double df = (p - c) - mu[2], dt = (t - c) - mu[3];
      acc[2] = fma(w * df, df, acc[2]);
      acc[3] = fma(w * dt, dt, acc[3]);
      acc[4] = fma(w * df, dt, acc[4]);
    }
  }
}

// one tile: n = rows * W contiguous floats at p / t / c; s_w[row] the row's weight
template <int PASS, bool VEC, bool CLIM>
__device__ __forceinline__ void metrics_tile(const float* __restrict__ p, const float* __restrict__ t, const float* __restrict__ c, int n,
                                             int W, const float* s_w, const double* mu, double* acc) {
  if (VEC) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
    const float4* t4 = reinterpret_cast<const float4*>(t);
    const float4* c4 = reinterpret_cast<const float4*>(c);
    const int n4 = n >> 2;
    for (int i = threadIdx.x; i < n4; i += kTileThreads) {
      const float4 a = p4[i], b = t4[i];
      float4 k = make_float4(0.f, 0.f, 0.f, 0.f);
      if (CLIM) k = c4[i];
      const double w = (double)s_w[(unsigned)(i << 2) / (unsigned)W];      // W % 4 == 0: the four values lie in one row
      metrics_accumulate<PASS, CLIM>(w, a.x, b.x, k.x, mu, acc);
      metrics_accumulate<PASS, CLIM>(w, a.y, b.y, k.y, mu, acc);
      metrics_accumulate<PASS, CLIM>(w, a.z, b.z, k.z, mu, acc);
      metrics_accumulate<PASS, CLIM>(w, a.w, b.w, k.w, mu, acc);
    }
  } else {
    for (int i = threadIdx.x; i < n; i += kTileThreads) {
      const float a = p[i], b = t[i];
      float k = 0.f;
      if (CLIM) k = c[i];
      metrics_accumulate<PASS, CLIM>((double)s_w[(unsigned)i / (unsigned)W], a, b, k, mu, acc);
    }
  }
}

// grid = total tiles.  PASS 2 reads the variable's pass-1 sums from `sums`.
template <int PASS>
__global__ __launch_bounds__(kTileThreads) void metrics_partial_kernel(const MetricsArgs a, const double* __restrict__ sums,
                                                                       double* __restrict__ slab) {
  __shared__ float s_w[kTileRows];
  __shared__ double s_red[kTileThreads / 64][kMetricsSums];
  const int tile = blockIdx.x;
  int vi = 0;
  while (vi + 1 < a.n_vars && tile >= a.v[vi + 1].tile0) ++vi;
  const MetricsVar& v = a.v[vi];
  const RowTile rt = row_tile(tile - v.tile0, a.g);
  stage_row_weights(s_w, a.w, rt.h0, rt.rows);
  const int lt = v.L * v.T;
  const int b = rt.plane / lt, r = rt.plane - b * lt;  // r = l * T + t
  const int l = r / v.T, tt = r - l * v.T;
  const int64_t hw = (int64_t)a.g.H * a.g.W;
  const float* p = v.pred + b * v.pred_bs + r * hw + rt.offset;
  const float* t = v.target + b * v.target_bs + r * hw + rt.offset;
  const float* c = v.clim ? v.clim + l * v.clim_ls + tt * v.clim_ts + rt.offset : nullptr;

  double mu[4] = {0.0, 0.0, 0.0, 0.0};
  if (PASS == 2) {
    const double* s = sums + (size_t)vi * kMetricsSums;
    const double inv_n = 1.0 / ((double)a.B * (double)lt * (double)hw);
    mu[0] = s[0] * inv_n;
    mu[1] = s[1] * inv_n;
    mu[2] = (s[0] - s[2]) * inv_n;
    mu[3] = (s[1] - s[2]) * inv_n;
  }
  double acc[kMetricsSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (v.vec) {
    if (c) metrics_tile<PASS, true, true>(p, t, c, rt.n, a.g.W, s_w, mu, acc);
    else metrics_tile<PASS, true, false>(p, t, c, rt.n, a.g.W, s_w, mu, acc);
  } else {
    if (c) metrics_tile<PASS, false, true>(p, t, c, rt.n, a.g.W, s_w, mu, acc);
    else metrics_tile<PASS, false, false>(p, t, c, rt.n, a.g.W, s_w, mu, acc);
  }
  const double s = block_sum_waves<kMetricsSums, kTileThreads>(acc, s_red);
  if (threadIdx.x < kMetricsSums) slab[(size_t)tile * kMetricsSums + threadIdx.x] = s;
}

// grid = n_vars.  PASS 1: sums[v][0..5] = the pass-1 sums.  PASS 2: the eight scores of variable v.
template <int PASS>
__global__ __launch_bounds__(kTileThreads) void metrics_finish_kernel(const MetricsArgs a, const double* __restrict__ slab,
                                                                      double* __restrict__ sums, float* __restrict__ scores) {
  __shared__ double s_red[kMetricsSums][kTileThreads];
  const int vi = blockIdx.x;
  const MetricsVar& v = a.v[vi];
  double acc[kMetricsSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  sum_slots<kMetricsSums, kTileThreads>(slab + (size_t)v.tile0 * kMetricsSums, v.ntiles, acc);
  block_sum_tree<kMetricsSums>(acc, s_red);
  if (PASS == 1) {
    if (threadIdx.x < kMetricsSums) sums[(size_t)vi * kMetricsSums + threadIdx.x] = s_red[threadIdx.x][0];
    return;
  }
  if (threadIdx.x != 0) return;
  const double* s1 = sums + (size_t)vi * kMetricsSums;
  const double inv_n = 1.0 / ((double)a.B * (double)v.L * (double)v.T * (double)a.g.H * (double)a.g.W);
  const double mse = s1[5] * inv_n, mae = s1[4] * inv_n, bias = s1[3] * inv_n;
  const double var_p = s_red[0][0] * inv_n, var_t = s_red[1][0] * inv_n;
  float* out = scores + (size_t)vi * kMetricsScores;
  out[0] = (float)sqrt(mse);
  out[1] = (float)mse;
  out[2] = (float)mae;
  out[3] = (float)bias;
  out[4] = (float)(1.0 - mse / (var_t + 1e-12));
  out[5] = (float)(log10(var_p + a.eps) - log10(var_t + a.eps));
  if (v.clim) {
    const double activity = sqrt(s_red[2][0] * inv_n + 1e-12);
    const double truth = sqrt(s_red[3][0] * inv_n + 1e-12);
    out[6] = (float)((s_red[4][0] * inv_n) / (activity * truth));
    out[7] = (float)activity;
  } else {
    out[6] = __builtin_nanf("");
    out[7] = __builtin_nanf("");
  }
}

class Metrics {
 public:
  Metrics(int H, int W, const float* lat_w, int dev) : g(row_tiles(H, W)), device(dev), mem(dev) {
    WX_HIP(hipSetDevice(device));
    if (lat_w) w = mem.upload(lat_w, (size_t)H);
    sums = (double*)mem.alloc(sizeof(double) * kMetricsMaxVars * kMetricsSums);
  }
  void apply(int n_vars, const float* const* pred, const int64_t* pred_bs, const float* const* target, const int64_t* target_bs,
             const float* const* clim, const int64_t* clim_ls, const int64_t* clim_ts, const int32_t* n_levels, const int32_t* n_time,
             int batch, double eps, float* scores, hipStream_t stream) {
    if (n_vars < 1 || n_vars > kMetricsMaxVars) throw std::runtime_error("wx_metrics_apply: 1.." + std::to_string(kMetricsMaxVars) + " variables");
    if (batch < 1) throw std::runtime_error("wx_metrics_apply: B >= 1");
    MetricsArgs a;
    std::memset(&a, 0, sizeof(a));
    int64_t tiles = 0;
    const bool row_vec = g.W % 4 == 0;
    auto aligned = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    for (int i = 0; i < n_vars; ++i) {
      if (!pred[i] || !target[i]) throw std::runtime_error("wx_metrics_apply: null tensor pointer");
      if (n_levels[i] < 1 || n_time[i] < 1) throw std::runtime_error("wx_metrics_apply: n_levels and n_time must be >= 1");
      if (batch > 1 && (pred_bs[i] < 0 || target_bs[i] < 0)) throw std::runtime_error("wx_metrics_apply: negative batch stride");
      MetricsVar& v = a.v[i];
      v.pred = pred[i];
      v.target = target[i];
      v.pred_bs = batch > 1 ? pred_bs[i] : 0;
      v.target_bs = batch > 1 ? target_bs[i] : 0;
      v.L = n_levels[i];
      v.T = n_time[i];
      v.clim = clim ? clim[i] : nullptr;
      if (v.clim) {
        if (!clim_ls || !clim_ts) throw std::runtime_error("wx_metrics_apply: null argument");
        if (clim_ls[i] < 0 || clim_ts[i] < 0) throw std::runtime_error("wx_metrics_apply: negative climatology stride");
        v.clim_ls = v.L > 1 ? clim_ls[i] : 0;
        v.clim_ts = v.T > 1 ? clim_ts[i] : 0;
      }
      v.vec = row_vec && aligned(v.pred) && aligned(v.target) && v.pred_bs % 4 == 0 && v.target_bs % 4 == 0 &&
              (!v.clim || (aligned(v.clim) && v.clim_ls % 4 == 0 && v.clim_ts % 4 == 0));
      const int64_t nt = (int64_t)batch * v.L * v.T * g.row_blocks;
      if (tiles + nt > 2147483647LL) throw std::runtime_error("wx_metrics_apply: B * n_levels * n_time * row blocks exceeds 2^31 - 1 tiles");
      v.tile0 = (int)tiles;
      v.ntiles = (int)nt;
      tiles += nt;
    }
    a.w = w;
    a.n_vars = n_vars; a.B = batch; a.g = g;
    a.eps = eps;
    WX_HIP(hipSetDevice(device));
    mem.grow(slab, slab_doubles, (size_t)tiles * kMetricsSums);
    const dim3 grid((unsigned)tiles), fin((unsigned)n_vars), block(kTileThreads);
    hipLaunchKernelGGL(metrics_partial_kernel<1>, grid, block, 0, stream, a, sums, slab);
    hipLaunchKernelGGL(metrics_finish_kernel<1>, fin, block, 0, stream, a, slab, sums, scores);
    hipLaunchKernelGGL(metrics_partial_kernel<2>, grid, block, 0, stream, a, sums, slab);
    hipLaunchKernelGGL(metrics_finish_kernel<2>, fin, block, 0, stream, a, slab, sums, scores);
    WX_HIP(hipGetLastError());
  }

 private:
  RowTiles g;
  int device;
  DeviceArena mem;
  float* w = nullptr;
  double* sums = nullptr;
  double* slab = nullptr;
  size_t slab_doubles = 0;
};

}  // namespace wx
