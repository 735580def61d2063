// Semi-Lagrangian tracer advection of the gen-2 post-block chain on the device (credit/postblock/advect.py): omega from mass
// continuity, an iterative-midpoint back-trajectory from every grid point of every level, and every tracer read trilinearly at its
// departure point, in TWO launches whatever the number of tracers, with one scratch volume:
//   1 advect_velocity_kernel  one thread per column (b, h, w), consecutive threads along w.  The thread walks the levels top ->
//                             surface: p_half = a_half + b_half sp (advect.py:355-363), the spherical divergence (:107-118: periodic
//                             centred dU/dlon, torch.gradient's coordinate-aware d(V cos)/dlat with one-sided first and last row),
//                             omega at the level centre as the mean of the negated running sum of div dp at its two interfaces,
//                             0 at the top (:150-156) -- or omega read from a tensor (:368-369) --, dp/dlevel (:378-379), and the
//                             index-space velocity (columns, rows, levels per second, :374-380) written as ONE 16-byte record per
//                             grid point into the scratch volume [B][L][H][W], top -> surface
//   2 advect_gather_kernel    one thread per (b, level, h, w): n_iterations fixed-point steps  disp = dt V(x0 - disp / 2)  from
//                             disp = 0 (:392-408), V the trilinear interpolant of the records (eight 16-byte loads per step), then
//                             every tracer read trilinearly at x0 - disp (:410-423).  The departure point never leaves registers.
// Sampling in INDEX space: the column is a floating remainder modulo W (torch.remainder: near the poles a displacement is thousands
// of columns) with neighbours i and (i + 1) mod W; row and level are clamped to [0, n - 1] with upper neighbour min(i + 1, n - 1).
// That is what grid_sample(bilinear, border, align_corners=True) over the reference's one-column circular halo computes (:162-203),
// without the halo copy and without the round trip through normalised coordinates.  Interpolation is three nested lerps,
// a + f (b - a), column first: equal neighbours return their own bits, so a zero displacement returns the input bit for bit and a
// zonally uniform state stays zonally uniform.
// Arithmetic follows the reference's float32 order: rounded products and sums (no contraction) and true divisions in the velocity
// kernel; the running sum of div dp is kept in double and rounded per level, as torch.cumsum does on the host.
// level_order "surface_to_top" is an index flip of the DATA's level axis (winds, omega, tracers in, tracers out); the coefficients
// and the scratch volume stay top -> surface.  Every variable is READ through a (pointer, batch stride) pair where it lies and
// WRITTEN to a fresh contiguous [B][L][H][W] tensor; outputs never alias inputs, so a tracer may be U or V itself.
// Supported range: L >= 2 (the reference's torch.gradient raises on one level), W >= 2, H >= 2, at most 32 tracers, B L H W < 2^31
// grid points (offsets into the volumes are 64-bit: B L H W x 16 bytes passes 2^31 at the 0.25-degree grid).
#pragma once
#include <cmath>
#include <cstring>
#include <string>

#include "wx_common.h"

namespace wx {

constexpr int kAdvectMaxTracers = 32;

struct AdvectTracers {
  const float* src[kAdvectMaxTracers];   // tracer t, batch item b at src[t] + b * bstride[t]: [L][hw]
  float* dst[kAdvectMaxTracers];         // [B][L][hw]
  int64_t bstride[kAdvectMaxTracers];    // in floats
  int n;
};

struct AdvectGeom {
  int H, W, L, flip;        // flip: the data's level axis runs surface -> top
  int n_iter;
  float dlon, two_dlon;     // longitude spacing in radians, and twice it (exact)
  float radius, dt, dp_floor;
};

// per-row tables (device): [H] each, and the half-level coefficients [L + 1], top -> surface
struct AdvectTables {
  const float* coslat;     // cos(lat)
  const float* r_coslat;   // R * max(cos(lat), coslat_floor)
  const float* dlat_row;   // torch.gradient(lat_rad): signed radians per row
  const float* ga;         // d/dlat coefficients of rows h - 1, h, h + 1 in the interior; on the first / last row gb is the
  const float* gb;         //   one-sided spacing lat[1] - lat[0] / lat[H - 1] - lat[H - 2], ga and gc are unused
  const float* gc;
  const float* a_half;
  const float* b_half;
};

// ---- host-only helpers (no HIP call) ---------------------------------------------------------------------------------------------
// "" or the reason wx_advect_create refuses; rows: the six per-row tables in the order of AdvectTables
inline std::string advect_check_create(int H, int W, int L, const float* a_half, const float* b_half, const float* const rows[6],
                                       float dlon, float dt, int n_iter, float dp_floor) {
  static const char* const what[6] = {"cos(lat)", "R cos(lat)", "latitude spacing", "gradient coefficient a", "gradient coefficient b",
                                      "gradient coefficient c"};
  if (H < 2 || W < 2) return "bad geometry: at least two latitudes and two longitudes";
  if (L < 2) return "a single level: the reference's torch.gradient over the level axis needs two";
  if (!a_half || !b_half || !rows) return "null coefficient array";
  if (n_iter < 1) return "n_iterations must be >= 1, got " + std::to_string(n_iter);
  if (!std::isfinite(dt) || !std::isfinite(dp_floor)) return "timestep and floors must be finite";
  if (!std::isfinite(dlon) || dlon == 0.f) return "the longitude spacing must be finite and not zero";
  if ((int64_t)L * H * W > 2147483647LL) return "L * H * W exceeds 2^31 - 1 grid points";
  for (int k = 0; k <= L; ++k)
    if (!std::isfinite(a_half[k]) || !std::isfinite(b_half[k])) return "a_half / b_half must be finite";
  for (int i = 0; i < 6; ++i) {
    if (!rows[i]) return std::string("null ") + what[i] + " table";
    for (int h = 0; h < H; ++h)
      if (!std::isfinite(rows[i][h])) return std::string(what[i]) + " must be finite (two equal latitudes?)";
  }
  for (int h = 0; h < H; ++h)
    if (!(rows[1][h] > 0.f) || rows[2][h] == 0.f) return "R cos(lat) must be positive and the latitude spacing not zero";
  if (rows[4][0] == 0.f || rows[4][H - 1] == 0.f) return "the first and last latitude spacing must not be zero";
  return "";
}

inline std::string advect_build_tracers(AdvectTracers& t, int n, const float* const* src, const int64_t* bstride, float* const* dst,
                                        int batch, int64_t points_per_item) {
  std::memset(&t, 0, sizeof(t));
  if (n < 1 || n > kAdvectMaxTracers) return "1.." + std::to_string(kAdvectMaxTracers) + " tracers";
  if (batch < 1) return "batch must be >= 1";
  if ((int64_t)batch * points_per_item > 2147483647LL) return "batch * L * H * W exceeds 2^31 - 1 grid points";
  t.n = n;
  for (int i = 0; i < n; ++i) {
    if (!src[i] || !dst[i]) return "null tensor pointer";
    if (batch > 1 && bstride[i] < 0) return "negative batch stride";
    t.src[i] = src[i]; t.dst[i] = dst[i]; t.bstride[i] = bstride[i];
  }
  return "";
}

// ---- device side -------------------------------------------------------------------------------------------------------------------
// launch 1: grid = ceil(batch * H * W / 256)
__global__ __launch_bounds__(256) void advect_velocity_kernel(const float* __restrict__ u, int64_t u_bs, const float* __restrict__ v,
                                                              int64_t v_bs, const float* __restrict__ sp, int64_t sp_bs,
                                                              const float* __restrict__ omega, int64_t om_bs, float4* __restrict__ vel,
                                                              AdvectGeom g, AdvectTables t, int batch) {
#pragma clang fp contract(off)
  const int64_t hw = (int64_t)g.H * g.W;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= batch * hw) return;
  const int b = (int)(id / hw);
  const int r = (int)(id - b * hw);
  const int h = r / g.W, w = r - h * g.W;
  const int we = w + 1 == g.W ? 0 : w + 1, ww = w == 0 ? g.W - 1 : w - 1;
  const int hn = h == 0 ? 0 : h - 1, hs = h == g.H - 1 ? g.H - 1 : h + 1;   // the rows of the latitude difference
  const float* ub = u + b * u_bs;
  const float* vb = v + b * v_bs;
  const float* ob = omega ? omega + b * om_bs : nullptr;
  const float ps = sp[b * sp_bs + r];
  const float cos_h = t.coslat[h], cos_n = t.coslat[hn], cos_s = t.coslat[hs];
  const float rc = t.r_coslat[h], dlat = t.dlat_row[h], ga = t.ga[h], gb = t.gb[h], gc = t.gc[h];
  const bool edge = h == 0 || h == g.H - 1;
  float4* out = vel + (int64_t)b * g.L * hw + r;
  // p_center of the levels k - 1, k, k + 1, carried along the walk
  float ph_lo = t.a_half[0] + t.b_half[0] * ps;                // p_half[k]
  float ph_hi = t.a_half[1] + t.b_half[1] * ps;                // p_half[k + 1]
  float pc_prev = 0.f, pc = 0.5f * (ph_lo + ph_hi);
  double flux = 0.0;      // running sum of div * dp down to the lower interface of the level
  float om_upper = 0.f;   // omega at the upper interface: 0 at the model top
  for (int k = 0; k < g.L; ++k) {
    const int kd = g.flip ? g.L - 1 - k : k;
    const int64_t lvl = (int64_t)kd * hw;
    const float uc = ub[lvl + r], vc = vb[lvl + r];
    float pc_next = pc, ph_next = ph_hi;
    if (k + 1 < g.L) {
      ph_next = t.a_half[k + 2] + t.b_half[k + 2] * ps;
      pc_next = 0.5f * (ph_hi + ph_next);
    }
    float om;
    if (ob) {
      om = ob[lvl + r];
    } else {
      const float dudlon = (ub[lvl + (int64_t)h * g.W + we] - ub[lvl + (int64_t)h * g.W + ww]) / g.two_dlon;
      const float fn = vb[lvl + (int64_t)hn * g.W + w] * cos_n, fs = vb[lvl + (int64_t)hs * g.W + w] * cos_s;
      float dvcos;
      if (edge) {
        dvcos = (fs - fn) / gb;
      } else {
        const float fc = vc * cos_h;
        dvcos = (ga * fn + gb * fc) + gc * fs;
      }
      const float div = (dudlon + dvcos) / rc;
      const float dp = ph_hi - ph_lo;
      flux += (double)(div * dp);
      const float om_lower = -(float)flux;
      om = 0.5f * (om_upper + om_lower);
      om_upper = om_lower;
    }
    float dpdl;   // torch.gradient(p_center, dim = level), unit spacing
    if (k == 0) dpdl = pc_next - pc;
    else if (k == g.L - 1) dpdl = pc - pc_prev;
    else dpdl = (pc_next - pc_prev) / 2.f;
    dpdl = fmaxf(dpdl, g.dp_floor);
    const float vcol = uc / rc / g.dlon;
    const float vrow = vc / g.radius / dlat;
    const float vlev = om / dpdl;
    out[(int64_t)k * hw] = make_float4(vcol, vrow, vlev, 0.f);
    pc_prev = pc; pc = pc_next; ph_lo = ph_hi; ph_hi = ph_next;
  }
}

// the eight corners and three weights of a sampling point in index space
struct AdvectCorner {
  int i0, i1, j0, j1, k0, k1;
  float fx, fy, fz;
};
__device__ __forceinline__ AdvectCorner advect_corner(float col, float row, float lev, int W, int H, int L) {
  AdvectCorner c;
  const float Wf = (float)W;
  float x = fmodf(col, Wf);        // torch.remainder: the result takes the divisor's sign
  if (x < 0.f) x += Wf;            // a tiny negative remainder rounds to W itself: column 0, weight 0, below
  int i0 = (int)x;
  c.fx = x - (float)i0;
  if (i0 >= W) i0 -= W;
  i0 = min(max(i0, 0), W - 1);     // a non-finite coordinate must not leave the volume
  c.i0 = i0;
  c.i1 = i0 + 1 == W ? 0 : i0 + 1;
  const float y = fminf(fmaxf(row, 0.f), (float)(H - 1));
  const int j0 = min((int)y, H - 1);
  c.fy = y - (float)j0;
  c.j0 = j0;
  c.j1 = min(j0 + 1, H - 1);
  const float z = fminf(fmaxf(lev, 0.f), (float)(L - 1));
  const int k0 = min((int)z, L - 1);
  c.fz = z - (float)k0;
  c.k0 = k0;
  c.k1 = min(k0 + 1, L - 1);
  return c;
}
__device__ __forceinline__ float advect_lerp(float a, float b, float f) { return fmaf(f, b - a, a); }

// launch 2: grid = ceil(batch * L * H * W / 256)
__global__ __launch_bounds__(256) void advect_gather_kernel(const float4* __restrict__ vel, const AdvectTracers t, AdvectGeom g, int batch) {
  const int64_t hw = (int64_t)g.H * g.W, lhw = hw * g.L;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= batch * lhw) return;
  const int b = (int)(id / lhw);
  const int64_t rem = id - b * lhw;
  const int k = (int)(rem / hw);
  const int r = (int)(rem - k * hw);
  const int h = r / g.W, w = r - h * g.W;
  const float col0 = (float)w, row0 = (float)h, lev0 = (float)k;
  const float4* vb = vel + b * lhw;
  float dc = 0.f, dr = 0.f, dl = 0.f;
  for (int it = 0; it < g.n_iter; ++it) {
    const AdvectCorner c = advect_corner(col0 - 0.5f * dc, row0 - 0.5f * dr, lev0 - 0.5f * dl, g.W, g.H, g.L);
    float m[2][3];
    for (int z = 0; z < 2; ++z) {
      const int64_t lv = (int64_t)(z ? c.k1 : c.k0) * hw;
      const int64_t r0 = lv + (int64_t)c.j0 * g.W, r1 = lv + (int64_t)c.j1 * g.W;
      const float4 q00 = vb[r0 + c.i0], q01 = vb[r0 + c.i1], q10 = vb[r1 + c.i0], q11 = vb[r1 + c.i1];
      m[z][0] = advect_lerp(advect_lerp(q00.x, q01.x, c.fx), advect_lerp(q10.x, q11.x, c.fx), c.fy);
      m[z][1] = advect_lerp(advect_lerp(q00.y, q01.y, c.fx), advect_lerp(q10.y, q11.y, c.fx), c.fy);
      m[z][2] = advect_lerp(advect_lerp(q00.z, q01.z, c.fx), advect_lerp(q10.z, q11.z, c.fx), c.fy);
    }
    dc = g.dt * advect_lerp(m[0][0], m[1][0], c.fz);
    dr = g.dt * advect_lerp(m[0][1], m[1][1], c.fz);
    dl = g.dt * advect_lerp(m[0][2], m[1][2], c.fz);
  }
  const AdvectCorner c = advect_corner(col0 - dc, row0 - dr, lev0 - dl, g.W, g.H, g.L);
  const int kd0 = g.flip ? g.L - 1 - c.k0 : c.k0, kd1 = g.flip ? g.L - 1 - c.k1 : c.k1, kdo = g.flip ? g.L - 1 - k : k;
  const int64_t a00 = kd0 * hw + (int64_t)c.j0 * g.W, a01 = kd0 * hw + (int64_t)c.j1 * g.W;
  const int64_t a10 = kd1 * hw + (int64_t)c.j0 * g.W, a11 = kd1 * hw + (int64_t)c.j1 * g.W;
  const int64_t o = b * lhw + kdo * hw + r;
  for (int i = 0; i < t.n; ++i) {
    const float* s = t.src[i] + b * t.bstride[i];
    const float top = advect_lerp(advect_lerp(s[a00 + c.i0], s[a00 + c.i1], c.fx), advect_lerp(s[a01 + c.i0], s[a01 + c.i1], c.fx), c.fy);
    const float bot = advect_lerp(advect_lerp(s[a10 + c.i0], s[a10 + c.i1], c.fx), advect_lerp(s[a11 + c.i0], s[a11 + c.i1], c.fx), c.fy);
    t.dst[i][o] = advect_lerp(top, bot, c.fz);
  }
}

class Advect {
 public:
  // rows: the six per-row tables [H] in the order of AdvectTables (host arrays, built by the caller with the reference's float32
  // expressions); a_half / b_half [L + 1] top -> surface
  Advect(int H, int W, int L, const float* a_half, const float* b_half, const float* const rows[6], float dlon, float dt, int n_iter,
         float dp_floor, bool surface_to_top, int dev)
      : device(dev), mem(dev) {
    WX_HIP(hipSetDevice(device));
    geom.H = H; geom.W = W; geom.L = L; geom.flip = surface_to_top ? 1 : 0;
    geom.n_iter = n_iter;
    geom.dlon = dlon; geom.two_dlon = 2.0f * dlon;
    geom.radius = 6371000.f;
    geom.dt = dt; geom.dp_floor = dp_floor;
    tab.coslat = mem.upload(rows[0], H);
    tab.r_coslat = mem.upload(rows[1], H);
    tab.dlat_row = mem.upload(rows[2], H);
    tab.ga = mem.upload(rows[3], H);
    tab.gb = mem.upload(rows[4], H);
    tab.gc = mem.upload(rows[5], H);
    tab.a_half = mem.upload(a_half, L + 1);
    tab.b_half = mem.upload(b_half, L + 1);
  }
  void apply(const float* u, int64_t u_bs, const float* v, int64_t v_bs, const float* sp, int64_t sp_bs, const float* omega,
             int64_t om_bs, int n_tracers, const float* const* src, const int64_t* bstride, float* const* dst, int batch,
             hipStream_t stream) {
    if (!u || !v || !sp) throw std::runtime_error("wx_advect_apply: null u / v / surface-pressure pointer");
    if (batch > 1 && (u_bs < 0 || v_bs < 0 || sp_bs < 0 || (omega && om_bs < 0))) throw std::runtime_error("wx_advect_apply: negative batch stride");
    const int64_t lhw = (int64_t)geom.L * geom.H * geom.W;
    AdvectTracers t;
    const std::string why = advect_build_tracers(t, n_tracers, src, bstride, dst, batch, lhw);
    if (!why.empty()) throw std::runtime_error("wx_advect_apply: " + why);
    WX_HIP(hipSetDevice(device));
    mem.grow(vel, vel_records, (size_t)batch * lhw);   // scratch sized by the batch seen so far
    const int64_t cols = (int64_t)batch * geom.H * geom.W;
    hipLaunchKernelGGL(advect_velocity_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, stream, u, u_bs, v, v_bs, sp, sp_bs,
                       omega, om_bs, vel, geom, tab, batch);
    hipLaunchKernelGGL(advect_gather_kernel, dim3((unsigned)((batch * lhw + 255) / 256)), dim3(256), 0, stream, (const float4*)vel, t, geom,
                       batch);
    WX_HIP(hipGetLastError());
  }

 private:
  int device;
  DeviceArena mem;
  AdvectGeom geom;
  AdvectTables tab;
  float4* vel = nullptr;
  size_t vel_records = 0;
};

}  // namespace wx
