// Input side of the step on the device:
//   credit/preblock/norm.py:78-98   ERA5Normalizer._normalize_tensor   (t - mean) / clamp(std, min=1e-12), per variable / level
//   credit/preblock/concat.py:96-207 ConcatToTensor                    torch.cat of the named fields along the channel dim
// fused into one pass: every named field [B, n_levels, T, H, W] (fp32, device) is written normalised into its channel
// slot of x [B, C, T, H, W].  HBM-bound copy: one float4 per thread, coalesced along longitude on both sides.
// The channel ORDER (field-type rank, 3d before 2d, stable) is host logic: wxengine/preblock.py.
//
// With a transform table set (wx_pre_set_transforms) a second kernel, pre_xform_kernel, serves the gen-2 chain
//   fill_values* -> (log_transform | sqrt_transform)? -> scaler -> concat
// in the same single pass; per output channel, in this order:
//   credit/preblock/fill_values.py:120-171  FillValues   up to 8 rules; every mask on the ORIGINAL value, numeric rules never match
//                                                         NaN, replacements in rule order (the last matching rule wins)
//   credit/preblock/log.py:84-105           LogTransform log_base(x + eps) - log_base(eps), base e / 2 / 10 (correctly rounded: see xform_forward)
//   credit/preblock/sqrt.py:52-71           SqrtTransform sqrtf(x)
// x < -eps and sqrt of a negative give NaN as in the reference (no fast-math).  The plain kernel shares only the load / store body
// (plane_pass4) with it and is the one that runs when no table is set, so that path keeps its bits.
#pragma once
#include <vector>

#include "wx_common.h"

namespace wx {

constexpr int kMaxFields = 64;

struct PreParams {
  const float* field[kMaxFields];  // [B][n_levels_f][T][HW]
  const int* ch_field;             // [C] field of each output channel
  const int* ch_level;             // [C] level inside that field
  const int* f_levels;             // [n_fields]
  const float *mean, *stdv;        // [C] or nullptr (no normalisation)
  float* x;                        // [B][C][T][HW]
  int C, T, hw, batch;
};

constexpr int kMaxFillRules = 8;
// enum wx_xform / wx_fill_op of include/wxengine.h
enum { kXfNone = 0, kXfLogE = 1, kXfLog2 = 2, kXfLog10 = 3, kXfSqrt = 4 };
enum { kFillNan = 0, kFillEq = 1, kFillNe = 2, kFillLt = 3, kFillLe = 4, kFillGt = 5, kFillGe = 6 };

struct PreXform {
  const int* kind;            // [C]
  const float *eps, *log_eps; // [C] rounded to fp32 on the host (the reference adds Python floats to fp32 tensors)
  const int* n_rules;         // [C] 0 .. kMaxFillRules
  const int* rule_op;         // [C][kMaxFillRules]
  const float *rule_search, *rule_fill;
};

__device__ __forceinline__ bool fill_match(int op, float x, float s) {
  switch (op) {   // comparisons with a NaN x are false, != excepted: fill_values.py:155 ANDs every numeric mask with ~isnan
    case kFillNan: return x != x;
    case kFillEq: return x == s;
    case kFillNe: return x != s && x == x;
    case kFillLt: return x < s;
    case kFillLe: return x <= s;
    case kFillGt: return x > s;
    default: return x >= s;
  }
}

__device__ __forceinline__ float xform_forward(float v, int kind, float eps, float log_eps) {
  switch (kind) {
    // The sum v + eps is the reference's float32 sum; its logarithm is evaluated in double and rounded once, i.e. correctly rounded.
    // The device logf / log2f / log10f are good to 1 ulp, and inside a forecast that is not enough: a variable that went out through
    // e^(p + log_eps) - eps comes back within a few hundredths of an ulp of the float32 value it started from, the host's logarithm
    // returns that value, and a 1-ulp miss here becomes a whole ulp of p (measured: 5.4e-4 of the normalised surface pressure at
    // std 0.003, against 8.7e-5 between the reference's own fp32 and fp64).  The pass stays HBM-bound.
    case kXfLogE: return (float)log((double)(v + eps)) - log_eps;
    case kXfLog2: return (float)log2((double)(v + eps)) - log_eps;
    case kXfLog10: return (float)log10((double)(v + eps)) - log_eps;
    case kXfSqrt: return sqrtf(v);
    default: return v;
  }
}

// The body of a named-tensor pass (pre_assemble_kernel, pre_xform_kernel, unxform_kernel of wx_unxform.h): one plane (b, c, t) per
// blockIdx.y, four longitudes per thread.  Loads 4 floats of the source plane, hands them to op(float (&v)[4]) to transform in place and
// stores 4.  The 16-byte path needs hw % 4 == 0 AND both plane pointers on 16 bytes (a field may be a view that starts on a 4-byte
// boundary); otherwise the scalar path, which pads v with zeros past the end of the plane and stores only what lies inside.
template <typename Op>
__device__ __forceinline__ void plane_pass4(const float* __restrict__ src, float* __restrict__ dst, int hw, Op op) {
  const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
  // No early return for a thread past the plane's end (n <= 0: it loads and stores nothing): behind one, the compiler sinks the
  // kernel's scalar loads of the plane pointers below the branch, onto every workgroup's critical path (measured: 2.5 % of the plain pass).
  const int n = min(4, hw - i);
  const bool vec = n == 4 && (hw & 3) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(src + i);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    for (int k = 0; k < n; ++k) v[k] = src[i + k];
  }
  op(v);
  if (vec) {
    *reinterpret_cast<float4*>(dst + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < n; ++k) dst[i + k] = v[k];
  }
}
// (b, c, t) of this workgroup's plane, for planes laid out [B][C][T]
__device__ __forceinline__ void plane_decode(int C, int T, int& b, int& c, int& t) {
  const int64_t plane = (int64_t)blockIdx.y;
  t = (int)(plane % T);
  c = (int)((plane / T) % C);
  b = (int)(plane / ((int64_t)T * C));
}
// Launches such a kernel over `planes` planes of hw floats.  The plane index is the grid's y dimension, which ends at 65535: more is
// refused with `too_many` here instead of being left to a failing launch.
template <auto Kernel, typename... Args>
inline void launch_plane_pass(int64_t planes, int hw, hipStream_t stream, const char* too_many, const Args&... args) {
  if (planes > 65535) throw std::runtime_error(too_many);
  hipLaunchKernelGGL(Kernel, dim3(cdiv(hw, 1024), (unsigned)planes), dim3(256), 0, stream, args...);
  WX_HIP(hipGetLastError());
}

// Every per-channel quantity is uniform in the workgroup (scalar loads).
__global__ __launch_bounds__(256) void pre_xform_kernel(const PreParams p, const PreXform t) {
  int b, c, tt;
  plane_decode(p.C, p.T, b, c, tt);
  const int f = p.ch_field[c], l = p.ch_level[c];
  const float* __restrict__ src = p.field[f] + (((int64_t)b * p.f_levels[f] + l) * p.T + tt) * p.hw;
  float* __restrict__ dst = p.x + (int64_t)blockIdx.y * p.hw;
  const bool norm = p.mean != nullptr;
  const float m = norm ? p.mean[c] : 0.f;
  const float s = norm ? fmaxf(p.stdv[c], 1e-12f) : 1.f;
  const int kind = t.kind[c], nr = t.n_rules[c];
  const float eps = t.eps[c], log_eps = t.log_eps[c];
  const int* __restrict__ rop = t.rule_op + (int64_t)c * kMaxFillRules;
  const float* __restrict__ rs = t.rule_search + (int64_t)c * kMaxFillRules;
  const float* __restrict__ rf = t.rule_fill + (int64_t)c * kMaxFillRules;
  plane_pass4(src, dst, p.hw, [=](float (&v)[4]) {
    float r[4] = {v[0], v[1], v[2], v[3]};
    for (int k = 0; k < nr; ++k) {
      const int op = rop[k];
      const float sv = rs[k], fv = rf[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = fill_match(op, v[j], sv) ? fv : r[j];   // mask on the original value v, not on r
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      r[j] = xform_forward(r[j], kind, eps, log_eps);
      v[j] = norm ? (r[j] - m) / s : r[j];
    }
  });
}

__global__ __launch_bounds__(256) void pre_assemble_kernel(const PreParams p) {
  int b, c, t;
  plane_decode(p.C, p.T, b, c, t);
  const int f = p.ch_field[c], l = p.ch_level[c];
  const float* __restrict__ src = p.field[f] + (((int64_t)b * p.f_levels[f] + l) * p.T + t) * p.hw;
  float* __restrict__ dst = p.x + (int64_t)blockIdx.y * p.hw;
  const bool norm = p.mean != nullptr;   // without statistics: a plain copy
  const float m = norm ? p.mean[c] : 0.f;
  const float s = norm ? fmaxf(p.stdv[c], 1e-12f) : 1.f;   // std.clamp(min=1e-12), norm.py:98
  plane_pass4(src, dst, p.hw, [=](float (&v)[4]) {
    if (!norm) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (v[j] - m) / s;
  });
}

class PreBlock {
 public:
  PreBlock(int n_fields, const int32_t* n_levels, int T_, int H, int W, const float* mean, const float* stdv, int dev)
      : nf(n_fields), T(T_), hw(H * W), device(dev), mem(dev) {
    if (n_fields < 1 || n_fields > kMaxFields) throw std::runtime_error("wx_pre_create: 1..64 fields");
    if (T_ < 1 || H < 1 || W < 1) throw std::runtime_error("wx_pre_create: bad geometry");
    WX_HIP(hipSetDevice(device));
    std::vector<int> cf, cl, fl(n_levels, n_levels + n_fields);
    for (int f = 0; f < n_fields; ++f) {
      if (n_levels[f] < 1) throw std::runtime_error("wx_pre_create: a field needs at least one level");
      for (int l = 0; l < n_levels[f]; ++l) { cf.push_back(f); cl.push_back(l); }
    }
    C = (int)cf.size();
    levels = fl;
    ch_field = mem.upload(cf.data(), C);
    ch_level = mem.upload(cl.data(), C);
    f_levels = mem.upload(fl.data(), n_fields);
    if ((mean == nullptr) != (stdv == nullptr)) throw std::runtime_error("wx_pre_create: mean and std come together");
    if (mean) { d_mean = mem.upload(mean, C); d_std = mem.upload(stdv, C); }
  }
  int channels() const { return C; }
  // per-output-channel arrays ([C], rules [C][kMaxFillRules]); from now on apply() launches pre_xform_kernel
  void set_transforms(const int32_t* kind, const float* eps, const float* log_eps, const int32_t* n_rules, const int32_t* rule_op,
                      const float* rule_search, const float* rule_fill) {
    for (int c = 0; c < C; ++c) {
      if (kind[c] < kXfNone || kind[c] > kXfSqrt) throw std::runtime_error("wx_pre_set_transforms: unknown transform kind " + std::to_string(kind[c]));
      if (kind[c] >= kXfLogE && kind[c] <= kXfLog10 && !(eps[c] > 0.f && std::isfinite(eps[c]) && std::isfinite(log_eps[c])))
        throw std::runtime_error("wx_pre_set_transforms: a log transform needs a finite eps > 0 and its finite log");
      if (n_rules[c] < 0 || n_rules[c] > kMaxFillRules) throw std::runtime_error("wx_pre_set_transforms: 0 .. 8 fill rules per channel");
      for (int k = 0; k < n_rules[c]; ++k)
        if (rule_op[c * kMaxFillRules + k] < kFillNan || rule_op[c * kMaxFillRules + k] > kFillGe)
          throw std::runtime_error("wx_pre_set_transforms: unknown fill rule op " + std::to_string(rule_op[c * kMaxFillRules + k]));
    }
    WX_HIP(hipSetDevice(device));
    // a second call replaces the table: the buffers it replaces are released first (a synchronous free: launches in flight finish)
    has_xf = false;
    mem.release(xf.kind); mem.release(xf.n_rules); mem.release(xf.eps); mem.release(xf.log_eps);
    mem.release(xf.rule_op); mem.release(xf.rule_search); mem.release(xf.rule_fill);
    const size_t nr = (size_t)C * kMaxFillRules;
    xf.kind = mem.upload(kind, C); xf.n_rules = mem.upload(n_rules, C);
    xf.eps = mem.upload(eps, C); xf.log_eps = mem.upload(log_eps, C);
    xf.rule_op = mem.upload(rule_op, nr); xf.rule_search = mem.upload(rule_search, nr); xf.rule_fill = mem.upload(rule_fill, nr);
    has_xf = true;
  }
  void apply(const float* const* fields, float* x, int batch, hipStream_t stream) {
    if (batch < 1) throw std::runtime_error("wx_pre_apply: batch < 1");
    WX_HIP(hipSetDevice(device));
    PreParams p;
    std::memset(&p, 0, sizeof(p));
    for (int f = 0; f < nf; ++f) {
      if (!fields[f]) throw std::runtime_error("wx_pre_apply: null field pointer");
      p.field[f] = fields[f];
    }
    p.ch_field = ch_field; p.ch_level = ch_level; p.f_levels = f_levels; p.mean = d_mean; p.stdv = d_std;
    p.x = x; p.C = C; p.T = T; p.hw = hw; p.batch = batch;
    const int64_t planes = (int64_t)batch * C * T;
    const char* too_many = "wx_pre_apply: batch * channels * frames exceeds 65535 planes";
    if (has_xf) launch_plane_pass<pre_xform_kernel>(planes, hw, stream, too_many, p, xf);
    else launch_plane_pass<pre_assemble_kernel>(planes, hw, stream, too_many, p);
  }

 private:
  int nf, T, hw, device, C = 0;
  DeviceArena mem;
  std::vector<int> levels;
  int *ch_field = nullptr, *ch_level = nullptr, *f_levels = nullptr;
  float *d_mean = nullptr, *d_std = nullptr;
  PreXform xf = {};
  bool has_xf = false;
};

}  // namespace wx
