// Pressure-level products of the gen-2 post-block chain in ONE pass over a column:
//   credit/postblock/geopotential.py:9-83      pressure_on_interfaces + geopotential (hydrostatic integral on model levels)
//   credit/postblock/pressure_interp.py:44-130 interp_column_to_pressure_levels (linear in log p, Trenberth below ground)
//   credit/postblock/_interp_utils.py:14-40    loglinear_interp_columns (bracket rule, weight clamp)
//   credit/postblock/mslp.py:33-80             mslp_from_surface_pressure
// The reference runs each as torch.vmap over columns in chunks of 1000 behind a permute of the whole state, and the geopotential
// travels through memory between the first two.  Here one thread owns one column of the named tensors as they lie in memory,
// [B][L][T][H][W] fp32: the level stride is T*H*W and adjacent threads read adjacent cells, so every load is coalesced and nothing
// is permuted or staged.  All three products are optional and any combination is one launch.
//
// Where the column lives.  Nothing of the column is held in registers across stages, so there is NO register-resident bound on L
// and no second strategy: the upward integral streams T and q once (that is the HBM pass) and leaves the column's geopotential in
// LDS; the interpolation adds the mid-level pressures to LDS, counts the bracket there, and gathers the two bracketing levels of
// T and of every field from global memory again (lines the first pass or a neighbouring thread has just pulled through L2).  LDS
// holds 2 * L floats per thread as [level][thread] (conflict-free), at most 64 KB per workgroup, which fixes the workgroup size:
//   L <= 32: 256 threads    L <= 64: 128    L <= 128: 64    L <= 137: 32
// (kDiagMaxLevels = 137, the full ERA5 level set).  At L = 16 that is 32 KB per workgroup: five workgroups (20 waves) per CU of
// 160 KB, enough loads in flight for a kernel that is bound by HBM.  The geometry is the only thing that changes with L.
//
// Arithmetic is fp32 in the reference's own order (a cumulative sum from the surface upward, `phis + cumsum`, left-to-right
// products); the compiler may contract a*b+c into one FMA.  One expression is evaluated differently: the interpolation weight
// (log pq - log p_lo) / (log p_hi - log p_lo) is formed as log(pq / p_lo) / log(p_hi / p_lo).  Subtracting two rounded logarithms
// of ~11 that lie 0.03 apart (40 levels and more) costs three digits of the weight; the ratio form keeps them, so the device lands
// nearer the fp64 result than the fp32 reference does.  The bracket is counted on the pressures themselves (log is monotonic).  The model-level geopotential never leaves the chip between the
// integral and the interpolation.  Chain mode (the reference's separate blocks): with q == nullptr the interpolation reads the
// geopotential an earlier launch wrote; the code behind that point is the same, so chain and fused launch agree bit for bit.
#pragma once
#include <vector>

#include "wx_common.h"

namespace wx {

constexpr int kDiagMaxLevels = 137;
constexpr int kDiagMaxPlev = 64;
constexpr int kDiagMaxFields = 8;

struct DiagParams {
  const float *T, *q, *sp, *phis, *t_ns;      // [B][L][T][HW] x 2, [B][1][T][HW], [B][1][phis_T][HW], [B][1][T][HW]
  const float* field[kDiagMaxFields];         // [B][L][T][HW] each
  const float* z_in;                          // chain mode: model-level geopotential written by an earlier launch
  float* z_out;                               // [B][L][T][HW] or nullptr
  float* plev_out[kDiagMaxFields + 2];        // [B][n_plev][T][HW]: fields, then T, then Z; all nullptr = product off
  float* mslp_out;                            // [B][1][T][HW] or nullptr
  const float *a_half, *b_half;               // [L + 1] device
  const float *a_mid, *b_mid;                 // [L] device
  const float* plev;                          // [n_plev] device, Pa
  int L, n_plev, n_fields;
  int flip_vertical;                          // geopotential.py:70-82
  int flip_mid;                               // levels are stored surface -> top (pressure_interp.py:237-241)
  int want_interp;
  int64_t hw, thw, phis_thw, ncol;            // H*W, T*H*W, phis_T*H*W, B*T*H*W
  float temp_height;
};

// geopotential.py:64-65 (its own gas constants) and credit/physics_constants.py (GRAVITY, RDGAS) as pressure_interp.py / mslp.py use them
constexpr float kDiagGeoRd = 287.06f;
constexpr float kDiagGeoGamma = (float)(461.51 / 287.06 - 1.0);
constexpr float kDiagGravity = 9.80665f;
constexpr float kDiagRd = 287.05f;
constexpr float kDiagLapse = 0.0065f;
constexpr float kDiagAlphaStd = (float)(0.0065 * 287.05 / 9.80665);
constexpr float kDiagTopPressure = 0.57f;   // geopotential.py:13, :33

__device__ __forceinline__ float diag_half_pressure(const DiagParams& p, int i, float sp) {
  const float v = p.a_half[i] + p.b_half[i] * sp;
  return v > 0.f ? v : kDiagTopPressure;
}

// mslp.py:51-80
__device__ __forceinline__ float diag_mslp(float sp, float t, float sgp) {
  const float height = sgp / kDiagGravity;
  const float tto = t + kDiagLapse * height;
  const bool m1 = (t <= 290.5f) && (tto > 290.5f);
  const bool m2 = t > 290.5f;
  const bool m3 = (t < 255.0f) && !m1 && !m2;
  float alpha = kDiagAlphaStd;
  if (m1) alpha = kDiagRd * (290.5f - t) / fmaxf(sgp, 1e-6f);
  if (m2) alpha = 0.f;
  float te = m2 ? 0.5f * (290.5f + t) : t;
  if (m3) te = 0.5f * (255.0f + t);
  const float x = sgp / (kDiagRd * fmaxf(te, 1.0f));
  const float ax = alpha * x;
  const float v = sp * expf(x * (1.0f - 0.5f * alpha * x + (ax * ax) / 3.0f));
  return fabsf(height) < 1e-4f ? sp : v;
}

__global__ void diag_column_kernel(const DiagParams p) {
  extern __shared__ float diag_lds[];
  const int tb = blockDim.x, tid = threadIdx.x;
  const int64_t n = (int64_t)blockIdx.x * tb + tid;
  if (n >= p.ncol) return;                       // no barrier below: a thread only touches its own LDS slots
  const int L = p.L;
  float* __restrict__ zs = diag_lds + tid;                    // zs[m * tb]: geopotential, m counts top -> surface
  float* __restrict__ lp = diag_lds + (int64_t)L * tb + tid;  // lp[m * tb]: mid-level pressure
  const int64_t b = n / p.thw, rem = n - b * p.thw;           // rem = t * HW + cell
  const int64_t col3 = b * L * p.thw + rem;                   // + level * thw
  const float sp = p.sp[n];
  const float phis = p.phis ? p.phis[b * p.phis_thw + (p.phis_thw == p.thw ? rem : rem % p.hw)] : 0.f;

  // ---- geopotential on model levels (geopotential.py:64-83): running sum from the first integrated layer
  if (p.q) {
    float acc = 0.f;
    for (int s = 0; s < L; ++s) {
      const int k = p.flip_vertical ? L - 1 - s : s;
      const float up = diag_half_pressure(p, k, sp), lo = diag_half_pressure(p, k + 1, sp);
      const float dlogp = logf(lo / up);
      const float alpha = 1.0f - (up / (lo - up)) * dlogp;
      const float tv = p.T[col3 + k * p.thw] * (1.0f + kDiagGeoGamma * p.q[col3 + k * p.thw]);
      const float rtv = kDiagGeoRd * tv;
      acc += rtv * dlogp;
      const float z = (phis + acc) - rtv * alpha;
      if (p.z_out) p.z_out[col3 + k * p.thw] = z;
      if (p.want_interp) zs[(int64_t)(p.flip_mid ? L - 1 - k : k) * tb] = z;
    }
  } else if (p.want_interp) {
    for (int k = 0; k < L; ++k) zs[(int64_t)(p.flip_mid ? L - 1 - k : k) * tb] = p.z_in[col3 + k * p.thw];
  }

  // ---- model levels -> pressure levels (pressure_interp.py:83-130)
  if (p.want_interp) {
    // level nearest temp_height above ground: first minimum in top -> surface order, as torch.argmin
    int mh = 0;
    float best = 0.f, pres_h = 0.f;
    for (int m = 0; m < L; ++m) {
      const int lev = p.flip_mid ? L - 1 - m : m;
      const float pm = p.a_mid[lev] + p.b_mid[lev] * sp;
      lp[(int64_t)m * tb] = pm;
      const float d = fabsf((zs[(int64_t)m * tb] - phis) / kDiagGravity - p.temp_height);
      if (m == 0 || d < best) { best = d; mh = m; pres_h = pm; }
    }
    const float temp_h = p.T[col3 + (p.flip_mid ? L - 1 - mh : mh) * p.thw];
    const float ts = temp_h + kDiagAlphaStd * temp_h * (sp / pres_h - 1.0f);
    const float sh = phis / kDiagGravity;
    const float tsl = ts + kDiagLapse * sh;
    const float tpl = fminf(tsl, 298.0f);
    const float g_sgp = kDiagGravity / fmaxf(phis, 1.0f);
    const float t_adj = 0.002f * ((2500.0f - sh) * tsl + (sh - 2000.0f) * tpl);
    const float gamma = sh > 2500.0f ? g_sgp * fmaxf(tpl - ts, 0.f) : (sh >= 2000.0f ? g_sgp * (t_adj - ts) : kDiagLapse);
    const float g_rd_g = gamma * kDiagRd / kDiagGravity;
    const int64_t colp = b * p.n_plev * p.thw + rem;          // + j * thw
    for (int j = 0; j < p.n_plev; ++j) {
      const float pj = p.plev[j];
      int cnt = 0;
      for (int m = 0; m < L; ++m) cnt += pj >= lp[(int64_t)m * tb] ? 1 : 0;     // _interp_utils.py:33 (log is monotonic)
      const int hi = min(max(cnt, 1), L - 1), lo = hi - 1;
      const float p_lo = lp[(int64_t)lo * tb], p_hi = lp[(int64_t)hi * tb];
      // (log pj - log p_lo) / (log p_hi - log p_lo) as a quotient of logs of RATIOS: same weight, none of the cancellation
      const float w = fminf(fmaxf(logf(pj / p_lo) / logf(p_hi / p_lo), 0.f), 1.f);
      const int64_t o_lo = col3 + (p.flip_mid ? L - 1 - lo : lo) * p.thw, o_hi = col3 + (p.flip_mid ? L - 1 - hi : hi) * p.thw;
      for (int f = 0; f < p.n_fields; ++f) {
        const float y_lo = p.field[f][o_lo], y_hi = p.field[f][o_hi];
        p.plev_out[f][colp + j * p.thw] = y_lo + w * (y_hi - y_lo);
      }
      const float t_lo = p.T[o_lo], t_hi = p.T[o_hi];
      const float z_lo = zs[(int64_t)lo * tb], z_hi = zs[(int64_t)hi * tb];
      float t_out = t_lo + w * (t_hi - t_lo), z_out = z_lo + w * (z_hi - z_lo);
      if (pj > sp) {   // below ground: Trenberth et al. 1993 Eq. 16 / 15 (pressure_interp.py:121-126)
        const float ln_p = logf(pj / sp);
        const float a = g_rd_g * ln_p;
        t_out = ts * (1.0f + a + 0.5f * (a * a) + (a * a * a) / 6.0f);
        z_out = phis - kDiagRd * ts * ln_p * (1.0f + 0.5f * a + (a * a) / 6.0f);
      }
      p.plev_out[p.n_fields][colp + j * p.thw] = t_out;
      p.plev_out[p.n_fields + 1][colp + j * p.thw] = z_out;
    }
  }

  if (p.mslp_out) p.mslp_out[n] = diag_mslp(sp, p.t_ns[n], phis);
}

// workgroup size for L levels: the largest of 256 / 128 / 64 / 32 threads whose 2 * L floats per thread fit 64 KB of LDS
inline int diag_threads(int L) { return L <= 32 ? 256 : L <= 64 ? 128 : L <= 128 ? 64 : 32; }

class Diag {
 public:
  Diag(int H, int W, int n_levels, int dev) : hw((int64_t)H * W), L(n_levels), device(dev), mem(dev) {
    if (H < 1 || W < 1) throw std::runtime_error("wx_diag_create: bad geometry");
    if (n_levels < 2 || n_levels > kDiagMaxLevels) throw std::runtime_error("wx_diag_create: n_levels must be 2 .. 137");
    WX_HIP(hipSetDevice(device));
    // a_half | b_half | a_mid | b_mid | plev
    coef = (float*)mem.alloc(sizeof(float) * (2 * (L + 1) + 2 * L + kDiagMaxPlev));
  }
  void set_levels(const float* a_half, const float* b_half, const float* a_mid, const float* b_mid, int flip_vertical_) {
    if ((a_half == nullptr) != (b_half == nullptr)) throw std::runtime_error("wx_diag_set_levels: a_half and b_half come together");
    if ((a_mid == nullptr) != (b_mid == nullptr)) throw std::runtime_error("wx_diag_set_levels: a_mid and b_mid come together");
    WX_HIP(hipSetDevice(device));
    if (a_half) {
      WX_HIP(hipMemcpy(coef, a_half, sizeof(float) * (L + 1), hipMemcpyHostToDevice));
      WX_HIP(hipMemcpy(coef + (L + 1), b_half, sizeof(float) * (L + 1), hipMemcpyHostToDevice));
    }
    if (a_mid) {
      WX_HIP(hipMemcpy(coef + 2 * (L + 1), a_mid, sizeof(float) * L, hipMemcpyHostToDevice));
      WX_HIP(hipMemcpy(coef + 2 * (L + 1) + L, b_mid, sizeof(float) * L, hipMemcpyHostToDevice));
      // pressure_interp.py:237-241: orientation from the coefficients at a reference surface pressure
      flip_mid = (a_mid[0] + b_mid[0] * 101325.0f) > (a_mid[L - 1] + b_mid[L - 1] * 101325.0f);
    }
    have_half = a_half != nullptr;
    have_mid = a_mid != nullptr;
    flip_vertical = flip_vertical_ != 0;
  }
  void set_pressure_levels(const float* p_pa, int n, float temp_height_) {
    if (n < 1 || n > kDiagMaxPlev) throw std::runtime_error("wx_diag_set_pressure_levels: n_plev must be 1 .. 64");
    if (!p_pa) throw std::runtime_error("wx_diag_set_pressure_levels: null argument");
    for (int j = 0; j < n; ++j)
      if (!(p_pa[j] > 0.f)) throw std::runtime_error("wx_diag_set_pressure_levels: pressures must be positive (Pa)");
    WX_HIP(hipSetDevice(device));
    WX_HIP(hipMemcpy(coef + 2 * (L + 1) + 2 * L, p_pa, sizeof(float) * n, hipMemcpyHostToDevice));
    n_plev = n;
    temp_height = temp_height_;
  }
  void apply(int batch, int n_time, const float* T, const float* q, const float* sp, const float* phis, int phis_n_time,
             const float* t_ns, const float* const* fields, int n_fields, float* z_model, float* const* plev_out, float* mslp_out,
             hipStream_t stream) {
    if (batch < 1 || n_time < 1) throw std::runtime_error("wx_diag_apply: batch and n_time must be >= 1");
    if (phis_n_time != 1 && phis_n_time != n_time) throw std::runtime_error("wx_diag_apply: phis_n_time must be 1 or n_time");
    if (n_fields < 0 || n_fields > kDiagMaxFields) throw std::runtime_error("wx_diag_apply: n_fields must be 0 .. 8");
    const bool want_plev = plev_out != nullptr, want_mslp = mslp_out != nullptr;
    const bool chain_z = want_plev && !q;                 // the interpolation reads z_model instead of integrating
    const bool want_z = z_model != nullptr && !chain_z;
    if (!want_plev && !want_mslp && !want_z) throw std::runtime_error("wx_diag_apply: no product requested (every output is null)");
    if (!sp || !phis) throw std::runtime_error("wx_diag_apply: every product needs sp and phis");
    const bool integrate = want_z || (want_plev && !chain_z);
    if (integrate) {
      if (!T || !q) throw std::runtime_error("wx_diag_apply: the geopotential needs T and q");
      if (!have_half) throw std::runtime_error("wx_diag_apply: the geopotential needs the half-level coefficients (wx_diag_set_levels a_half / b_half)");
    }
    if (want_plev) {
      if (!T) throw std::runtime_error("wx_diag_apply: the pressure-level set needs T");
      if (chain_z && !z_model) throw std::runtime_error("wx_diag_apply: the pressure-level set needs q (to integrate the geopotential) or z_model (to read it)");
      if (!have_mid) throw std::runtime_error("wx_diag_apply: the pressure-level set needs the mid-level coefficients (wx_diag_set_levels a_mid / b_mid)");
      if (n_plev < 1) throw std::runtime_error("wx_diag_apply: the pressure-level set needs wx_diag_set_pressure_levels");
      if (n_fields > 0 && !fields) throw std::runtime_error("wx_diag_apply: null fields array");
      for (int f = 0; f < n_fields; ++f)
        if (!fields[f]) throw std::runtime_error("wx_diag_apply: null field pointer");
      for (int f = 0; f < n_fields + 2; ++f)
        if (!plev_out[f]) throw std::runtime_error("wx_diag_apply: null pressure-level output pointer");
    }
    if (want_mslp && !t_ns) throw std::runtime_error("wx_diag_apply: MSLP needs the near-surface temperature");
    WX_HIP(hipSetDevice(device));
    DiagParams p;
    std::memset(&p, 0, sizeof(p));
    p.T = T; p.q = integrate ? q : nullptr; p.sp = sp; p.phis = phis; p.t_ns = t_ns;
    p.z_in = chain_z ? z_model : nullptr;
    p.z_out = want_z ? z_model : nullptr;
    p.mslp_out = mslp_out;
    if (want_plev) {
      for (int f = 0; f < n_fields; ++f) p.field[f] = fields[f];
      for (int f = 0; f < n_fields + 2; ++f) p.plev_out[f] = plev_out[f];
    }
    p.a_half = coef; p.b_half = coef + (L + 1); p.a_mid = coef + 2 * (L + 1); p.b_mid = p.a_mid + L; p.plev = p.b_mid + L;
    p.L = L; p.n_plev = n_plev; p.n_fields = want_plev ? n_fields : 0;
    p.flip_vertical = flip_vertical; p.flip_mid = flip_mid; p.want_interp = want_plev;
    p.hw = hw; p.thw = hw * n_time; p.phis_thw = hw * phis_n_time; p.ncol = p.thw * batch;
    p.temp_height = temp_height;
    const int tb = diag_threads(L);
    const int64_t blocks = (p.ncol + tb - 1) / tb;
    if (blocks > INT_MAX) throw std::runtime_error("wx_diag_apply: too many columns for one launch");
    const size_t lds = want_plev ? sizeof(float) * 2 * (size_t)L * tb : 0;   // <= 64 KB by diag_threads
    hipLaunchKernelGGL(diag_column_kernel, dim3((unsigned)blocks), dim3(tb), lds, stream, p);
    WX_HIP(hipGetLastError());
  }
  int levels() const { return L; }

 private:
  int64_t hw;
  int L, device, n_plev = 0;
  DeviceArena mem;
  float* coef = nullptr;
  bool have_half = false, have_mid = false, flip_vertical = true, flip_mid = false;
  float temp_height = 150.0f;
};

}  // namespace wx
