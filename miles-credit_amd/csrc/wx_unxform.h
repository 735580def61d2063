// Output side of the gen-2 variable transforms on the device: the inverse scale and the inverse transform of a list of named tensors
// of y_processed in ONE launch.
//   bridgescaler_transform(inverse_transform)  p = y * std + mean per variable and level (the expression wxengine/forecast.py::InverseScale
//                                              pins: a rounded product, then a rounded sum -- no FMA); a variable without statistics
//                                              skips it altogether
//   credit/postblock/exp.py:73-88     ExpTransform     base^(p + log_base(eps)) - eps, base e / 2 / 10 (expf / exp2f / powf(10, .))
//   credit/postblock/square.py:42-57  SquareTransform  p * p
// Every variable is READ through a (pointer, batch stride) pair: Reconstruct hands out channel slices of y_pred [B][C][T][H][W], whose
// batch items are [n_levels][T][H][W] contiguous but C*T*H*W apart, and they are consumed where they lie.  Every variable is WRITTEN to
// a fresh contiguous [B][n_levels][T][H][W] tensor; the sources are never modified (the reference rebinds the dict entry too).
// HBM-bound: one float4 per thread along longitude where hw % 4 == 0 AND both plane pointers sit on 16 bytes -- a channel slice on a
// grid with odd H*W starts on a 4-byte boundary only -- else the scalar path.
#pragma once
#include <vector>

#include "wx_common.h"
#include "wx_pre.h"

namespace wx {

// enum wx_xform of include/wxengine.h, inverse direction
enum { kUnxNone = 0, kUnxExpE = 1, kUnxExp2 = 2, kUnxExp10 = 3, kUnxSquare = 4 };

struct UnxParams {
  const float* src[kMaxFields];   // variable v, batch item b at src[v] + b * bstride[v]: [n_levels][T][hw]
  float* dst[kMaxFields];         // [B][n_levels][T][hw]
  int64_t bstride[kMaxFields];    // in floats
  const int *ch_var, *ch_level;   // [C] variable / level of each (variable, level) channel
  const int *v_levels, *v_kind, *v_stats;   // [n_vars]
  const float *v_eps, *v_log_eps;           // [n_vars]
  const float *mean, *stdv;                 // [C] (read only where v_stats is set)
  int C, T, hw;
};

__device__ __forceinline__ float xform_inverse(float p, int kind, float eps, float log_eps) {
  switch (kind) {
    case kUnxExpE: return expf(p + log_eps) - eps;
    case kUnxExp2: return exp2f(p + log_eps) - eps;
    case kUnxExp10: return powf(10.0f, p + log_eps) - eps;   // torch.pow(10.0, .), exp.py:71
    case kUnxSquare: return p * p;
    default: return p;
  }
}

// t * s + m as a rounded product and a rounded sum, like the torch expression: hipcc contracts a * b + c into an FMA by default (and
// __fmul_rn / __fadd_rn are plain operators in the HIP headers), so contraction is switched off for exactly these two operations
__device__ __forceinline__ float scale_unfused(float y, float s, float m) {
#pragma clang fp contract(off)
  const float t = y * s;
  return t + m;
}

__global__ __launch_bounds__(256) void unxform_kernel(const UnxParams p) {
  int b, c, t;
  plane_decode(p.C, p.T, b, c, t);
  const int f = p.ch_var[c], l = p.ch_level[c];
  const float* __restrict__ src = p.src[f] + (int64_t)b * p.bstride[f] + ((int64_t)l * p.T + t) * p.hw;
  float* __restrict__ dst = p.dst[f] + (((int64_t)b * p.v_levels[f] + l) * p.T + t) * p.hw;
  const bool scale = p.v_stats[f] != 0;
  const float m = scale ? p.mean[c] : 0.f, s = scale ? p.stdv[c] : 1.f;
  const int kind = p.v_kind[f];
  const float eps = p.v_eps[f], log_eps = p.v_log_eps[f];
  plane_pass4(src, dst, p.hw, [=](float (&v)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (scale) v[j] = scale_unfused(v[j], s, m);
      v[j] = xform_inverse(v[j], kind, eps, log_eps);
    }
  });
}

class Unxform {
 public:
  // kind / eps / log_eps / has_stats: [n_vars]; mean / stdv: one entry per (variable, level) in variable order, or nullptr when no
  // variable has statistics
  Unxform(int n_vars, const int32_t* n_levels, int H, int W, const int32_t* kind, const float* eps, const float* log_eps,
          const int32_t* has_stats, const float* mean, const float* stdv, int dev)
      : nv(n_vars), hw(H * W), device(dev), mem(dev) {
    WX_HIP(hipSetDevice(device));
    std::vector<int> cv, cl, vl(n_levels, n_levels + n_vars), vk(kind, kind + n_vars), vs(has_stats, has_stats + n_vars);
    for (int v = 0; v < n_vars; ++v)
      for (int l = 0; l < n_levels[v]; ++l) { cv.push_back(v); cl.push_back(l); }
    C = (int)cv.size();
    ch_var = mem.upload(cv.data(), C);
    ch_level = mem.upload(cl.data(), C);
    v_levels = mem.upload(vl.data(), nv);
    v_kind = mem.upload(vk.data(), nv);
    v_stats = mem.upload(vs.data(), nv);
    v_eps = mem.upload(eps, nv);
    v_log_eps = mem.upload(log_eps, nv);
    if (mean) { d_mean = mem.upload(mean, C); d_std = mem.upload(stdv, C); }
  }
  int variables() const { return nv; }
  void apply(const float* const* src, const int64_t* batch_stride, float* const* dst, int batch, int n_time, hipStream_t stream) {
    if (batch < 1 || n_time < 1) throw std::runtime_error("wx_unxform_apply: batch and n_time must be >= 1");
    WX_HIP(hipSetDevice(device));
    UnxParams p;
    std::memset(&p, 0, sizeof(p));
    for (int v = 0; v < nv; ++v) {
      if (!src[v] || !dst[v]) throw std::runtime_error("wx_unxform_apply: null tensor pointer");
      if (batch > 1 && batch_stride[v] < 0) throw std::runtime_error("wx_unxform_apply: negative batch stride");
      p.src[v] = src[v]; p.dst[v] = dst[v]; p.bstride[v] = batch_stride[v];
    }
    p.ch_var = ch_var; p.ch_level = ch_level; p.v_levels = v_levels; p.v_kind = v_kind; p.v_stats = v_stats;
    p.v_eps = v_eps; p.v_log_eps = v_log_eps; p.mean = d_mean; p.stdv = d_std;
    p.C = C; p.T = n_time; p.hw = hw;
    launch_plane_pass<unxform_kernel>((int64_t)batch * C * n_time, hw, stream, "wx_unxform_apply: batch * levels * n_time exceeds 65535 planes", p);
  }

 private:
  int nv, hw, device, C = 0;
  DeviceArena mem;
  int *ch_var = nullptr, *ch_level = nullptr, *v_levels = nullptr, *v_kind = nullptr, *v_stats = nullptr;
  float *v_eps = nullptr, *v_log_eps = nullptr, *d_mean = nullptr, *d_std = nullptr;
};

}  // namespace wx
