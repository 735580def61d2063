// The wind artifact filter of the gen-2 post-block chain on the device (credit/postblock/wind_filter.py): a jet mask from one level
// of U and V, and a masked Gaussian blend of every target plane, in at most FOUR launches whatever the number of variables and levels:
//   1 wind_dilate_kernel   flag = sqrt(u^2 + v^2) > threshold at the mask level, then the rectangular dilation
//                          clamp(conv2d(flag, ones[dil_lat, dil_lon], zero pad), 0, 1) (wind_filter.py:40-47) -- an OR, exact in any order
//   2 wind_falloff_kernel  the zero-padded Gaussian falloff of the dilated mask (:51-67) -> m [B][H][W] in [0, 1]
//   3 wind_sums_kernel     only with preserve_amplitude (:115-121): per (batch item, target plane) the sums  m f^2  and  m fs^2  in
//                          double, one partial per strip of tile rows in the fixed order of wx_reduce.h; the blend launch adds the
//                          partials in strip order, so two calls on the same input give the same bits
//   4 wind_blend_kernel    every plane (variable, level, batch item) in one grid: target planes  fs = conv2d(f, G, zero pad),
//                          fs *= alpha = min(sqrt(sum m f^2 / (sum m fs^2 + 1e-12)), 4),  out = m fs + (1 - m) f  (:113-123, rounded
//                          products and a rounded sum: a point with m == 0 keeps its bits); every other plane is copied
// All three stencils are SEPARABLE and run on one LDS tile: the 16 x 64 output tile plus its halo is staged in LDS (zero outside the
// grid, exactly conv2d's zero padding -- no wrap in longitude, the reference has none), a row pass along longitude writes a second
// LDS array, a column pass along latitude reads it with 16-byte LDS reads.  The 2-D outer product of the reference is never formed:
// the separable sum differs from its 2-D sum by rounding only.  The blend launch recomputes fs instead of storing it: a target plane
// is read twice and written once.
// Every variable is READ through a (pointer, batch stride) pair where it lies (Reconstruct hands out channel slices of y_pred) and
// WRITTEN to a fresh contiguous [B][n_levels][1][H][W] tensor.  U and V are mask sources and targets: the mask is complete before the
// blend launch writes anything, and outputs never alias inputs.  16-byte global accesses along longitude where W % 4 == 0 and the
// plane pointer sits on 16 bytes, 4-byte accesses otherwise; both fill the same LDS tile, so the results are the same bits.
// Supported range, fixed at construction: every kernel (dilation, falloff, smoothing) odd and at most 33 (latitude) x 65 (longitude)
// -- falloff_sigma <= 8, smoothing sigmas <= 5.33 (latitude) / 10.66 (longitude); any H, W >= 1 (a grid smaller than the kernels is
// all halo); at most 32 variables of at most 256 levels; batch * levels * tiles < 2^31.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "wx_common.h"
#include "wx_reduce.h"

namespace wx {

constexpr int kWindTH = 16, kWindTW = 64;              // output tile: 256 threads x 4 consecutive longitudes
constexpr int kWindMaxKLat = 33, kWindMaxKLon = 65;    // largest kernel along latitude / longitude
constexpr int kWindMaxVars = 32, kWindMaxLevels = 256;

struct WindVars {
  const float* src[kWindMaxVars];     // variable v, batch item b at src[v] + b * bstride[v]: [n_levels][hw]
  float* dst[kWindMaxVars];           // [B][n_levels][hw]
  int64_t bstride[kWindMaxVars];      // in floats
  uint64_t target[kWindMaxVars][kWindMaxLevels / 64];   // bit l: level l of the variable is filtered
  int lvl0[kWindMaxVars + 1];         // prefix sums of the level counts
  int n_vars;
};

// ---- host-only helpers (no HIP call: checked by a stand-alone sanitizer program) -------------------------------------------------
// "" or the reason wx_wind_create refuses; w / n: smoothing latitude, smoothing longitude, falloff latitude, falloff longitude
inline std::string wind_check_create(int H, int W, const float* const w[4], const int n[4], int dil_lat, int dil_lon, float threshold) {
  static const char* const what[4] = {"smoothing latitude", "smoothing longitude", "falloff latitude", "falloff longitude"};
  if (H < 1 || W < 1) return "bad geometry";
  for (int i = 0; i < 4; ++i) {
    const int cap = (i & 1) ? kWindMaxKLon : kWindMaxKLat;
    if (!w[i]) return std::string("null ") + what[i] + " weights";
    if (n[i] < 1 || !(n[i] & 1)) return std::string(what[i]) + " kernel size " + std::to_string(n[i]) + " must be odd and >= 1";
    if (n[i] > cap) return std::string(what[i]) + " kernel size " + std::to_string(n[i]) + " exceeds the supported " + std::to_string(cap);
    for (int k = 0; k < n[i]; ++k)
      if (!std::isfinite(w[i][k])) return std::string(what[i]) + " weights must be finite";
  }
  if (dil_lat < 1 || dil_lon < 1 || !(dil_lat & 1) || !(dil_lon & 1))
    return "dilation sizes must be odd and >= 1 (an even size makes the reference's dilated mask one row or column larger than the field)";
  if (dil_lat > kWindMaxKLat || dil_lon > kWindMaxKLon)
    return "dilation " + std::to_string(dil_lat) + " x " + std::to_string(dil_lon) + " exceeds the supported " +
           std::to_string(kWindMaxKLat) + " x " + std::to_string(kWindMaxKLon);
  if (!std::isfinite(threshold)) return "the speed threshold must be finite";
  return "";
}

// fills `t` from the arguments of wx_wind_apply; "" or the reason.  Target levels beyond a variable's level count are skipped.
inline std::string wind_build_vars(WindVars& t, int n_vars, const float* const* src, const int64_t* bstride, const int32_t* n_levels,
                                   float* const* dst, const int32_t* target_levels, int n_targets, int batch, int64_t tiles) {
  std::memset(&t, 0, sizeof(t));
  if (n_vars < 1 || n_vars > kWindMaxVars) return "1.." + std::to_string(kWindMaxVars) + " variables";
  if (batch < 1) return "batch must be >= 1";
  if (n_targets < 0 || (n_targets > 0 && !target_levels)) return "null target-level list";
  t.n_vars = n_vars;
  for (int v = 0; v < n_vars; ++v) {
    if (!src[v] || !dst[v]) return "null tensor pointer";
    if (n_levels[v] < 1 || n_levels[v] > kWindMaxLevels) return "a variable has 1.." + std::to_string(kWindMaxLevels) + " levels";
    if (batch > 1 && bstride[v] < 0) return "negative batch stride";
    t.src[v] = src[v]; t.dst[v] = dst[v]; t.bstride[v] = bstride[v];
    t.lvl0[v + 1] = t.lvl0[v] + n_levels[v];
    for (int k = 0; k < n_targets; ++k) {
      const int l = target_levels[k];
      if (l < 0) return "negative target level";
      if (l < n_levels[v]) t.target[v][l >> 6] |= uint64_t(1) << (l & 63);
    }
  }
  if ((int64_t)batch * t.lvl0[n_vars] * tiles > 2147483647LL) return "batch * levels * tiles exceeds the grid limit 2^31 - 1";
  return "";
}

// ---- device side -------------------------------------------------------------------------------------------------------------------
struct WindFieldSrc {
  const float* p;
  __device__ bool aligned16() const { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
  __device__ float at(int64_t i) const { return p[i]; }
  __device__ float4 at4(int64_t i) const { return *reinterpret_cast<const float4*>(p + i); }
};

// sqrt(u^2 + v^2) > threshold as torch evaluates it: two rounded squares, a rounded sum (no FMA), a correctly rounded root
__device__ __forceinline__ float wind_flag(float u, float v, float thr) {
#pragma clang fp contract(off)
  const float uu = u * u, vv = v * v;
  return sqrtf(uu + vv) > thr ? 1.f : 0.f;
}

struct WindFlagSrc {
  const float *u, *v;
  float thr;
  __device__ bool aligned16() const { return ((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(v)) & 15) == 0; }
  __device__ float at(int64_t i) const { return wind_flag(u[i], v[i], thr); }
  __device__ float4 at4(int64_t i) const {
    const float4 a = *reinterpret_cast<const float4*>(u + i), b = *reinterpret_cast<const float4*>(v + i);
    return make_float4(wind_flag(a.x, b.x, thr), wind_flag(a.y, b.y, thr), wind_flag(a.z, b.z, thr), wind_flag(a.w, b.w, thr));
  }
};

__host__ __device__ inline int wind_halo4(int k_lon) { return ((k_lon / 2) + 3) & ~3; }   // longitude halo rounded up to 4 columns
// floats of LDS one tile needs: the staged tile with its halo, and the row-pass result
inline size_t wind_lds_floats(int k_lat, int k_lon) {
  const int R = kWindTH + 2 * (k_lat / 2);
  return (size_t)R * (kWindTW + 2 * wind_halo4(k_lon)) + (size_t)R * kWindTW;
}

// The separable stencil at the thread's four outputs: row y0 + tid / 16, columns x0 + (tid % 16) * 4 .. + 3.
//   out[i]    = sum_k w_lat[k] * (sum_j w_lon[j] * src(y - k_lat / 2 + k, x - k_lon / 2 + j)), the source being 0 outside the grid
//               (kOnes: both weight vectors are ones and are not read)
//   centre[i] = the source at the output point itself (0 outside the grid)
// lds: wind_lds_floats(k_lat, k_lon) floats on 16 bytes; `vec`: W % 4 == 0 and the source plane sits on 16 bytes.
template <bool kOnes, typename Src>
__device__ __forceinline__ void wind_conv_tile(const Src& src, bool vec, int H, int W, int y0, int x0, const float* __restrict__ w_lat,
                                               const float* __restrict__ w_lon, int k_lat, int k_lon, float* lds, float out[4],
                                               float centre[4]) {
  const int tid = threadIdx.x;
  const int rh = k_lat / 2, rw = k_lon / 2, rw4 = wind_halo4(k_lon);
  const int R = kWindTH + 2 * rh, RW = kWindTW + 2 * rw4, ng = RW / 4;
  float* raw = lds;
  float* tmp = lds + R * RW;
  __syncthreads();   // a previous tile of this workgroup is done with the LDS
  for (int idx = tid; idx < R * ng; idx += 256) {
    const int r = idx / ng, g = idx - r * ng;
    const int y = y0 - rh + r, x = x0 - rw4 + 4 * g;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (y >= 0 && y < H) {
      const int64_t row = (int64_t)y * W;
      if (vec) {   // x % 4 == 0 and W % 4 == 0: a group lies inside the grid or outside it as a whole
        if (x >= 0 && x < W) q = src.at4(row + x);
      } else {
        if (x >= 0 && x < W) q.x = src.at(row + x);
        if (x + 1 >= 0 && x + 1 < W) q.y = src.at(row + x + 1);
        if (x + 2 >= 0 && x + 2 < W) q.z = src.at(row + x + 2);
        if (x + 3 >= 0 && x + 3 < W) q.w = src.at(row + x + 3);
      }
    }
    *reinterpret_cast<float4*>(raw + r * RW + 4 * g) = q;
  }
  __syncthreads();
  // row pass: one wave per staged row, one lane per output column (consecutive LDS words: no bank conflict)
  for (int idx = tid; idx < R * kWindTW; idx += 256) {
    const int r = idx / kWindTW, c = idx - r * kWindTW;
    const int y = y0 - rh + r;
    float acc = 0.f;
    if (y >= 0 && y < H) {   // a row outside the grid is all zero
      const float* base = raw + r * RW + (rw4 - rw) + c;
      for (int j = 0; j < k_lon; ++j) acc = kOnes ? acc + base[j] : fmaf(w_lon[j], base[j], acc);
    }
    tmp[idx] = acc;
  }
  __syncthreads();
  // column pass: 16 bytes per lane, a wave reads four whole rows of the row-pass array
  const int ty = tid / 16, tx4 = (tid % 16) * 4;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int k = 0; k < k_lat; ++k) {
    const float4 t = *reinterpret_cast<const float4*>(tmp + (ty + k) * kWindTW + tx4);
    if (kOnes) {
      a0 += t.x; a1 += t.y; a2 += t.z; a3 += t.w;
    } else {
      const float w = w_lat[k];
      a0 = fmaf(w, t.x, a0); a1 = fmaf(w, t.y, a1); a2 = fmaf(w, t.z, a2); a3 = fmaf(w, t.w, a3);
    }
  }
  out[0] = a0; out[1] = a1; out[2] = a2; out[3] = a3;
  const float4 c4 = *reinterpret_cast<const float4*>(raw + (ty + rh) * RW + rw4 + tx4);
  centre[0] = c4.x; centre[1] = c4.y; centre[2] = c4.z; centre[3] = c4.w;
}

// the thread's four values of a plane at row y, columns x .. x + 3 (0 outside the grid) / their store
__device__ __forceinline__ void wind_load4(const float* __restrict__ plane, bool vec, int H, int W, int y, int x, float v[4]) {
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if (y >= H || x >= W) return;
  const float* p = plane + (int64_t)y * W + x;
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    for (int i = 0; i < 4 && x + i < W; ++i) v[i] = p[i];
  }
}
__device__ __forceinline__ void wind_store4(float* __restrict__ plane, bool vec, int H, int W, int y, int x, const float v[4]) {
  if (y >= H || x >= W) return;
  float* p = plane + (int64_t)y * W + x;
  if (vec) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int i = 0; i < 4 && x + i < W; ++i) p[i] = v[i];
  }
}
__device__ __forceinline__ bool wind_vec(const void* p, int W) { return (W & 3) == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct WindGrid {
  int H, W, tiles_x, tiles_y;
};

// launch 1: grid = batch * tiles
__global__ __launch_bounds__(256) void wind_dilate_kernel(const float* __restrict__ u, int64_t u_bstride, const float* __restrict__ v,
                                                          int64_t v_bstride, float thr, float* __restrict__ dil, WindGrid g, int k_lat, int k_lon) {
  extern __shared__ __attribute__((aligned(16))) float wind_lds[];
  const int tiles = g.tiles_x * g.tiles_y;
  const int b = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int y0 = (tile / g.tiles_x) * kWindTH, x0 = (tile % g.tiles_x) * kWindTW;
  const WindFlagSrc src{u + (int64_t)b * u_bstride, v + (int64_t)b * v_bstride, thr};
  float out[4], centre[4];
  wind_conv_tile<true>(src, (g.W & 3) == 0 && src.aligned16(), g.H, g.W, y0, x0, nullptr, nullptr, k_lat, k_lon, wind_lds, out, centre);
  for (int i = 0; i < 4; ++i) out[i] = fminf(out[i], 1.f);   // counts of 0 / 1 flags are exact: clamp(., 0, 1)
  float* dst = dil + (int64_t)b * g.H * g.W;
  wind_store4(dst, wind_vec(dst, g.W), g.H, g.W, y0 + threadIdx.x / 16, x0 + (threadIdx.x % 16) * 4, out);
}

// launch 2: grid = batch * tiles
__global__ __launch_bounds__(256) void wind_falloff_kernel(const float* __restrict__ dil, float* __restrict__ mask, WindGrid g,
                                                           const float* __restrict__ w_lat, const float* __restrict__ w_lon, int k_lat, int k_lon) {
  extern __shared__ __attribute__((aligned(16))) float wind_lds[];
  const int tiles = g.tiles_x * g.tiles_y;
  const int b = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int y0 = (tile / g.tiles_x) * kWindTH, x0 = (tile % g.tiles_x) * kWindTW;
  const WindFieldSrc src{dil + (int64_t)b * g.H * g.W};
  float out[4], centre[4];
  wind_conv_tile<false>(src, (g.W & 3) == 0 && src.aligned16(), g.H, g.W, y0, x0, w_lat, w_lon, k_lat, k_lon, wind_lds, out, centre);
  float* dst = mask + (int64_t)b * g.H * g.W;
  wind_store4(dst, wind_vec(dst, g.W), g.H, g.W, y0 + threadIdx.x / 16, x0 + (threadIdx.x % 16) * 4, out);
}

// plane index (batch item, variable, level) -> its pointers; true when the level is filtered
__device__ __forceinline__ bool wind_plane(const WindVars& t, int plane, int hw, int& b, const float*& src, float*& dst) {
  const int total = t.lvl0[t.n_vars];
  b = plane / total;
  const int c = plane - b * total;
  int v = 0;
  while (c >= t.lvl0[v + 1]) ++v;
  const int l = c - t.lvl0[v], nl = t.lvl0[v + 1] - t.lvl0[v];
  src = t.src[v] + (int64_t)b * t.bstride[v] + (int64_t)l * hw;
  dst = t.dst[v] + ((int64_t)b * nl + l) * hw;
  return (t.target[v][l >> 6] >> (l & 63)) & 1;
}

// launch 3 (preserve_amplitude only): grid = batch * levels * tiles_y; partial[(plane * tiles_y + strip) * 2 + {0, 1}] = the sums of
// m f^2 and m fs^2 over one strip of tile rows, in double, tiles in order, then the workgroup (wx_reduce.h)
__global__ __launch_bounds__(256) void wind_sums_kernel(const WindVars t, const float* __restrict__ mask, double* __restrict__ partial,
                                                        WindGrid g, const float* __restrict__ w_lat, const float* __restrict__ w_lon, int k_lat,
                                                        int k_lon) {
  extern __shared__ __attribute__((aligned(16))) float wind_lds[];
  __shared__ double red[4][2];
  const int plane = blockIdx.x / g.tiles_y, strip = blockIdx.x % g.tiles_y;
  const int hw = g.H * g.W;
  int b;
  const float* srcp;
  float* dstp;
  if (!wind_plane(t, plane, hw, b, srcp, dstp)) return;   // the whole workgroup: a pass-through plane has no sums
  const WindFieldSrc src{srcp};
  const bool vec = (g.W & 3) == 0 && src.aligned16();
  const float* m_plane = mask + (int64_t)b * hw;
  const bool vec_m = wind_vec(m_plane, g.W);
  const int y = strip * kWindTH + threadIdx.x / 16;
  double acc[2] = {0.0, 0.0};   // num, den
  for (int tx = 0; tx < g.tiles_x; ++tx) {
    float fs[4], f[4], m[4];
    wind_conv_tile<false>(src, vec, g.H, g.W, strip * kWindTH, tx * kWindTW, w_lat, w_lon, k_lat, k_lon, wind_lds, fs, f);
    wind_load4(m_plane, vec_m, g.H, g.W, y, tx * kWindTW + (threadIdx.x % 16) * 4, m);   // 0 outside the grid: no contribution
    for (int i = 0; i < 4; ++i) {
      acc[0] += (double)m[i] * ((double)f[i] * (double)f[i]);
      acc[1] += (double)m[i] * ((double)fs[i] * (double)fs[i]);
    }
  }
  const double s = block_sum_waves<2, 256>(acc, red);
  if (threadIdx.x < 2) partial[((int64_t)plane * g.tiles_y + strip) * 2 + threadIdx.x] = s;
}

// m fs + (1 - m) f as torch evaluates it: three rounded products / differences and a rounded sum; m == 0 returns f's bits
__device__ __forceinline__ float wind_blend(float m, float fs, float f) {
#pragma clang fp contract(off)
  const float a = m * fs;
  const float w = 1.f - m;
  const float c = w * f;
  return a + c;
}

// launch 4: grid = batch * levels * tiles; partial == nullptr: no amplitude rescaling
__global__ __launch_bounds__(256) void wind_blend_kernel(const WindVars t, const float* __restrict__ mask, const double* __restrict__ partial,
                                                         WindGrid g, const float* __restrict__ w_lat, const float* __restrict__ w_lon, int k_lat,
                                                         int k_lon) {
  extern __shared__ __attribute__((aligned(16))) float wind_lds[];
  const int tiles = g.tiles_x * g.tiles_y;
  const int plane = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int y0 = (tile / g.tiles_x) * kWindTH, x0 = (tile % g.tiles_x) * kWindTW;
  const int y = y0 + threadIdx.x / 16, x = x0 + (threadIdx.x % 16) * 4;
  const int hw = g.H * g.W;
  int b;
  const float* srcp;
  float* dstp;
  const bool filtered = wind_plane(t, plane, hw, b, srcp, dstp);
  const bool vec_o = wind_vec(dstp, g.W);
  if (!filtered) {   // pass-through level: copied, so the output tensor is complete after this launch
    float v[4];
    wind_load4(srcp, wind_vec(srcp, g.W), g.H, g.W, y, x, v);
    wind_store4(dstp, vec_o, g.H, g.W, y, x, v);
    return;
  }
  const WindFieldSrc src{srcp};
  float fs[4], f[4], m[4];
  wind_conv_tile<false>(src, (g.W & 3) == 0 && src.aligned16(), g.H, g.W, y0, x0, w_lat, w_lon, k_lat, k_lon, wind_lds, fs, f);
  const float* m_plane = mask + (int64_t)b * hw;
  wind_load4(m_plane, wind_vec(m_plane, g.W), g.H, g.W, y, x, m);
  if (partial) {
    const double* p = partial + (int64_t)plane * g.tiles_y * 2;
    double num = 0.0, den = 0.0;
    for (int s = 0; s < g.tiles_y; ++s) { num += p[2 * s]; den += p[2 * s + 1]; }   // strip order: the same bits in every workgroup and call
    const float alpha = (float)fmin(sqrt(num / (den + 1e-12)), 4.0);
    for (int i = 0; i < 4; ++i) fs[i] *= alpha;
  }
  float o[4];
  for (int i = 0; i < 4; ++i) o[i] = wind_blend(m[i], fs[i], f[i]);
  wind_store4(dstp, vec_o, g.H, g.W, y, x, o);
}

class Wind {
 public:
  // w / n: smoothing latitude, smoothing longitude, falloff latitude, falloff longitude (host arrays, checked by wind_check_create)
  Wind(int H_, int W_, const float* const w[4], const int n[4], int dil_lat_, int dil_lon_, float threshold, bool preserve_, int dev)
      : H(H_), W(W_), dil_lat(dil_lat_), dil_lon(dil_lon_), thr(threshold), preserve(preserve_), device(dev), mem(dev) {
    WX_HIP(hipSetDevice(device));
    for (int i = 0; i < 4; ++i) {
      k[i] = n[i];
      wdev[i] = mem.upload(w[i], n[i]);
    }
    grid.H = H; grid.W = W;
    grid.tiles_x = (W + kWindTW - 1) / kWindTW;
    grid.tiles_y = (H + kWindTH - 1) / kWindTH;
  }
  int launches() const { return preserve ? 4 : 3; }
  // mask_out: [batch][H][W] on the device, or nullptr (the mask then lives in the object's own buffer)
  void apply(const float* u, int64_t u_bstride, const float* v, int64_t v_bstride, int n_vars, const float* const* src,
             const int64_t* bstride, const int32_t* n_levels, float* const* dst, const int32_t* target_levels, int n_targets, int batch,
             float* mask_out, hipStream_t stream) {
    if (!u || !v) throw std::runtime_error("wx_wind_apply: null u / v pointer");
    if (batch > 1 && (u_bstride < 0 || v_bstride < 0)) throw std::runtime_error("wx_wind_apply: negative batch stride");
    const int64_t tiles = (int64_t)grid.tiles_x * grid.tiles_y;
    WindVars t;
    const std::string why = wind_build_vars(t, n_vars, src, bstride, n_levels, dst, target_levels, n_targets, batch, tiles);
    if (!why.empty()) throw std::runtime_error("wx_wind_apply: " + why);
    WX_HIP(hipSetDevice(device));
    const int64_t planes = (int64_t)batch * t.lvl0[n_vars];
    const size_t hw = (size_t)H * W;
    mem.grow(dil, dil_floats, (size_t)batch * hw);
    if (!mask_out) mem.grow(mask, mask_floats, (size_t)batch * hw);
    float* m = mask_out ? mask_out : mask;
    const size_t lds_d = wind_lds_floats(dil_lat, dil_lon) * sizeof(float), lds_f = wind_lds_floats(k[2], k[3]) * sizeof(float),
                 lds_s = wind_lds_floats(k[0], k[1]) * sizeof(float);
    hipLaunchKernelGGL(wind_dilate_kernel, dim3((unsigned)(batch * tiles)), dim3(256), lds_d, stream, u, u_bstride, v, v_bstride, thr, dil,
                       grid, dil_lat, dil_lon);
    hipLaunchKernelGGL(wind_falloff_kernel, dim3((unsigned)(batch * tiles)), dim3(256), lds_f, stream, dil, m, grid, wdev[2], wdev[3], k[2], k[3]);
    if (preserve) {
      mem.grow(partial, partial_doubles, (size_t)planes * grid.tiles_y * 2);
      hipLaunchKernelGGL(wind_sums_kernel, dim3((unsigned)(planes * grid.tiles_y)), dim3(256), lds_s, stream, t, m, partial, grid, wdev[0],
                         wdev[1], k[0], k[1]);
    }
    hipLaunchKernelGGL(wind_blend_kernel, dim3((unsigned)(planes * tiles)), dim3(256), lds_s, stream, t, m,
                       preserve ? (const double*)partial : (const double*)nullptr, grid, wdev[0], wdev[1], k[0], k[1]);
    WX_HIP(hipGetLastError());
  }

 private:
  int H, W, dil_lat, dil_lon;
  float thr;
  bool preserve;
  int device;
  DeviceArena mem;
  int k[4] = {0, 0, 0, 0};
  float* wdev[4] = {nullptr, nullptr, nullptr, nullptr};
  WindGrid grid;
  float *dil = nullptr, *mask = nullptr;
  double* partial = nullptr;
  size_t dil_floats = 0, mask_floats = 0, partial_doubles = 0;   // scratch sized by the batch seen so far
};

}  // namespace wx
