// The diffusion and pole filter of credit/pol_lapdiff_filt.py (Diffusion_and_Pole_Filter) on the device: the polar zonal low-pass
// polfiltT and the three explicit diffusion schemes polefilt_lap2d_V1 / QV1 / V2, composed from the transforms of wx_sht.h.
//
// With A = scalar analysis, grad(c) = vector_synthesis(sqrt(l (l + 1)) c / a, no toroidal part) = (g_x east, g_y north) and
// div(U, V) = -sqrt(l (l + 1)) s_lm / a, s the spheroidal coefficients of vector_analysis(U, V):
//   L(x)    = grad(A(g_x))_x + grad(A(g_y))_y with (g_x, g_y) = grad(A(x)).  NOT the spectral Laplacian: the components of a gradient
//             are not smooth at the poles and their analysis is a quadrature.
//   scalar  x = lowpass(x); substeps times: x += coef sig[k] L(x)                        (V1: coef 1e8, QV1: 0.5e8)
//   vector  U, V = lowpass(U), lowpass(V); substeps times: (l_x, l_y) = grad(A(L(d))), d = div(U, V) read as coefficients;
//             U -= coef sig[k] l_x, V -= coef sig[k] l_y                                   (V2: coef 2e16)
//   lowpass rows 1 .. indpol and nlat - indpol .. nlat - 1 (row 0 stays, the last row is filtered: the reference's index list), each
//             y_j = A_0 / N + (2 / N) sum_{k=1}^{i-1} (A_k cos + B_k sin) + (1 / N) (A_i cos + B_i sin),  A_k = sum_j x_j cos(2 pi k j / N),
//             B_k likewise with sin, angle 2 pi k j / N: what zeroing Z[i : N - i] of the full FFT and taking the real part of the
//             inverse leaves -- the modes below the cutoff index i whole, mode i at half weight.  i = 0: the rows stay as they are.
// Everything between the load of the input and the single rounding of the output is fp64.
//
// A call runs on one stream without a host sync, in chunks of kPoleChunk planes, so that the two inner analyses of a sub-step are
// ONE call of 2 kPoleChunk = kShtMaxPlanes planes.  Work fields of a chunk of P planes: X [2P] (the field, or U then V), G [2P] and
// A [2P] fp64 planes and C [2P] coefficient planes; a sub-step is
//   scalar  C = A(X);  G = grad(C);  C = A(G) (2P planes);  A[:P] = east of grad(C[:P]), A[P:] = north of grad(C[P:]);  X += coef sig (A[:P] + A[P:])
//   vector  C = vector_analysis(X);  G = grad(div) (one per-degree scale -l (l + 1) / a^2 on the spheroidal part);  C = A(G);  A as above;
//           G[:P] = A[:P] + A[P:];  C[:P] = A(G[:P]);  A = grad(C[:P]);  X -= coef sig A (2P planes)
// Every sum has one fixed order: the transforms' own, the workgroup reduction of wx_reduce.h in the low-pass.  A plane's result is
// bit-identical whatever n_planes and its position.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "wx_common.h"
#include "wx_reduce.h"
#include "wx_sht.h"

namespace wx {

constexpr int kPoleChunk = kShtMaxPlanes / 2;

// ---- host-only helpers (no HIP call) ---------------------------------------------------------------------------------------------
// "" or the reason wx_polefilter_create refuses (after sht_check_create's)
inline std::string polefilter_check_create(int nlat, int nlon, double radius, int indpol, int cutoff, const float* sig) {
  if (indpol < 0) return "indpol must be >= 0, got " + std::to_string(indpol);
  if (nlat < 2 * indpol + 1)
    return "nlat must be >= 2 indpol + 1 = " + std::to_string(2 * indpol + 1) + ", got " + std::to_string(nlat) +
           ": the polar bands (rows 1 .. indpol and nlat - indpol .. nlat - 1) would overlap, and the low-pass with its half-weight mode "
           "is not idempotent";
  if (cutoff < 0 || cutoff > nlon / 2) return "cutoff_index must be in 0 .. nlon / 2 = " + std::to_string(nlon / 2) + ", got " + std::to_string(cutoff);
  if (!std::isfinite(radius) || !(radius > 0.0)) return "radius must be finite and > 0";
  for (int k = 0; k < nlat; ++k)
    if (!std::isfinite(sig[k])) return "a ramp weight must be finite, row " + std::to_string(k) + " is not";
  return "";
}

struct PoleField {
  const void* p;
  int64_t stride;
};
// Do any two planes of n planes of hw elements at a (stride sa) and at b (stride sb) share memory?  Exact for equal strides -- the
// planes of two fields may interleave, as the channels of one tensor do --, the test of the whole ranges otherwise.
inline bool polefilter_planes_overlap(const PoleField& a, const PoleField& b, int n, int64_t hw, int elem) {
  const int64_t ab = ((int64_t)(n - 1) * a.stride + hw) * elem, bb = ((int64_t)(n - 1) * b.stride + hw) * elem;
  if (!bytes_overlap(a.p, ab, b.p, bb)) return false;
  if (a.stride != b.stride || n == 1) return true;
  const int64_t S = a.stride * elem, H = hw * elem;
  const int64_t d = (int64_t)((intptr_t)b.p - (intptr_t)a.p);      // plane j of b against plane i of a: d + (j - i) S, |j - i| <= n - 1
  for (int64_t k = -d / S - 1; k <= -d / S + 1; ++k) {
    const int64_t off = d + k * S;
    if (k > -(int64_t)n && k < (int64_t)n && off < H && -off < H) return true;
  }
  return false;
}
// "" or the reason a call on n inputs and their n outputs is refused.  An output may be its own input (same address, same stride);
// any other overlap of an output with an input or another output is refused.
inline std::string polefilter_check_call(int nlat, int nlon, int n_planes, int dtype, int substeps, double coef, const PoleField* in,
                                         const PoleField* out, int n) {
  for (int i = 0; i < n; ++i)
    if (!in[i].p || !out[i].p) return "a null pointer: every input and output field is needed";
  int64_t strides[4];
  for (int i = 0; i < n; ++i) { strides[i] = in[i].stride; strides[n + i] = out[i].stride; }
  const std::string why = sht_check_planes(nlat, nlon, n_planes, dtype, 2 * n, strides);
  if (!why.empty()) return why;
  if (substeps < 0) return "substeps must be >= 0, got " + std::to_string(substeps);
  if (!std::isfinite(coef)) return "coef must be finite";
  const int64_t hw = (int64_t)nlat * nlon;
  const int elem = dtype == kShtF64 ? 8 : 4;
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) {
      if (i == j && out[i].p == in[j].p && out[i].stride == in[j].stride) continue;      // in place
      if (polefilter_planes_overlap(out[i], in[j], n_planes, hw, elem))
        return "an output overlaps an input that is not its own (in place means the same address and stride)";
    }
    for (int j = 0; j < i; ++j)
      if (polefilter_planes_overlap(out[i], out[j], n_planes, hw, elem)) return "two outputs overlap";
  }
  return "";
}

// The work memory of a call on n_planes planes, in bytes: the fields and coefficients of a chunk and the transform's scratch.
inline int64_t polefilter_workspace(int nlat, int nlon, int lmax, int mmax, int n_planes) {
  const int64_t P = std::min(std::max(n_planes, 1), kPoleChunk);
  return 6 * P * (int64_t)nlat * nlon * 8 + sht_coeff_bytes(lmax, mmax, (int)(2 * P)) + Sht::scratch_bytes(nlat, mmax, (int)(2 * P));
}

// The per-degree scales of grad and of grad(div(.)) on a sphere of radius a.
inline void polefilter_scales(int lmax, double radius, std::vector<double>& grad, std::vector<double>& divgrad) {
  grad.resize(lmax);
  divgrad.resize(lmax);
  for (int l = 0; l < lmax; ++l) {
    const double r = std::sqrt((double)l * (l + 1)) / radius;
    grad[l] = r;
    divgrad[l] = -r * r;
  }
}

// ---- device side -------------------------------------------------------------------------------------------------------------------
// grid (ceil(hw / 256), planes)
template <typename T>
__global__ __launch_bounds__(256) void polefilter_load_kernel(const T* __restrict__ src, int64_t stride, int hw, double* __restrict__ dst) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e < hw) dst[(int64_t)blockIdx.y * hw + e] = (double)src[(int64_t)blockIdx.y * stride + e];
}
template <typename T>
__global__ __launch_bounds__(256) void polefilter_store_kernel(const double* __restrict__ src, int hw, T* __restrict__ dst, int64_t stride) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e < hw) dst[(int64_t)blockIdx.y * stride + e] = (T)src[(int64_t)blockIdx.y * hw + e];
}

// The low-pass in place on X[planes][nlat][nlon]: grid (2 indpol, planes), a workgroup per filtered row; LDS 16 (cut + 1) bytes.
__global__ __launch_bounds__(256) void polefilter_lowpass_kernel(double* __restrict__ X, int nlat, int nlon, int indpol, int cut) {
  extern __shared__ double pole_ab[];                     // (A_k, B_k), k = 0 .. cut
  __shared__ double s_red[4][2];
  const int r = (int)blockIdx.x;
  const int k = r < indpol ? 1 + r : nlat - 2 * indpol + r;
  double* row = X + ((int64_t)blockIdx.y * nlat + k) * nlon;
  const double w0 = 2.0 * kShtPi / (double)nlon;
  for (int q = 0; q <= cut; ++q) {
    double acc[2] = {0.0, 0.0};
    for (int j = threadIdx.x; j < nlon; j += 256) {
      double sn, cs;
      sincos(w0 * (double)(((int64_t)q * j) % nlon), &sn, &cs);
      const double x = row[j];
      acc[0] += x * cs;
      acc[1] += x * sn;
    }
    const double sum = block_sum_waves<2, 256>(acc, s_red);
    if (threadIdx.x < 2) pole_ab[2 * q + threadIdx.x] = sum;
    __syncthreads();
  }
  const double inv = 1.0 / (double)nlon;
  for (int j = threadIdx.x; j < nlon; j += 256) {
    double y = pole_ab[0] * inv;
    for (int q = 1; q <= cut; ++q) {
      double sn, cs;
      sincos(w0 * (double)(((int64_t)q * j) % nlon), &sn, &cs);
      y += (q < cut ? 2.0 * inv : inv) * (pole_ab[2 * q] * cs + pole_ab[2 * q + 1] * sn);
    }
    row[j] = y;
  }
}

// out = a + b over n elements
__global__ __launch_bounds__(256) void polefilter_sum_kernel(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) out[e] = a[e] + b[e];
}

// X[p][k][j] += ((a (+ b)) sig[k]) coef over n = planes * nlat * nlon elements; b may be null
__global__ __launch_bounds__(256) void polefilter_update_kernel(double* __restrict__ X, const double* __restrict__ a, const double* __restrict__ b,
                                                                const float* __restrict__ sig, double coef, int nlat, int nlon, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int k = (int)((e / nlon) % nlat);
  const double l = b ? a[e] + b[e] : a[e];
  X[e] += (l * (double)sig[k]) * coef;
}

class PoleFilter {
 public:
  PoleFilter(Sht& sht_, double radius, int indpol_, int cutoff, const float* sig_host, int dev)
      : sht(sht_), nlat(sht_.n_lat()), nlon(sht_.n_lon()), lmax(sht_.l_max()), mmax(sht_.m_max()), indpol(indpol_), cut(cutoff), device(dev), mem(dev) {
    WX_HIP(hipSetDevice(device));
    std::vector<double> g, dg;
    polefilter_scales(lmax, radius, g, dg);
    s_grad = mem.upload(g.data(), g.size());
    s_divgrad = mem.upload(dg.data(), dg.size());
    sig = mem.upload(sig_host, (size_t)nlat);
  }

  void lowpass(int n_planes, const void* x, int64_t x_stride, int dtype, void* out, int64_t out_stride, hipStream_t stream) {
    run("wx_polefilter_lowpass", n_planes, dtype, 0, 0.0, x, x_stride, nullptr, 0, out, out_stride, nullptr, 0, stream);
  }
  void scalar(int n_planes, const void* x, int64_t x_stride, int dtype, int substeps, double coef, void* out, int64_t out_stride, hipStream_t stream) {
    run("wx_polefilter_scalar", n_planes, dtype, substeps, coef, x, x_stride, nullptr, 0, out, out_stride, nullptr, 0, stream);
  }
  void vector(int n_planes, const void* u, int64_t u_stride, const void* v, int64_t v_stride, int dtype, int substeps, double coef, void* u_out,
              int64_t u_out_stride, void* v_out, int64_t v_out_stride, hipStream_t stream) {
    if (!v || !v_out) throw std::runtime_error("wx_polefilter_vector: a null pointer: every input and output field is needed");
    run("wx_polefilter_vector", n_planes, dtype, substeps, coef, u, u_stride, v, v_stride, u_out, u_out_stride, v_out, v_out_stride, stream);
  }
  // grad(c) on the sphere of the handle's radius: (g_x, g_y) [n_planes][nlat][nlon]
  void gradient(int n_planes, const double* c, void* gx, void* gy, int dtype, hipStream_t stream) {
    if (!gx || !gy) throw std::runtime_error("wx_polefilter_gradient: a null pointer: both components are needed");
    sht.vector_synthesis(n_planes, c, nullptr, s_grad, gx, gy, dtype, stream);
  }

 private:
  // v == nullptr: the scalar form
  void run(const char* fn, int n_planes, int dtype, int substeps, double coef, const void* x, int64_t x_stride, const void* v, int64_t v_stride,
           void* x_out, int64_t x_out_stride, void* v_out, int64_t v_out_stride, hipStream_t stream) {
    const bool vec = v != nullptr;
    const PoleField in[2] = {{x, x_stride}, {v, v_stride}}, out[2] = {{x_out, x_out_stride}, {v_out, v_out_stride}};
    const std::string why = polefilter_check_call(nlat, nlon, n_planes, dtype, substeps, coef, in, out, vec ? 2 : 1);
    if (!why.empty()) throw std::runtime_error(std::string(fn) + ": " + why);
    WX_HIP(hipSetDevice(device));
    const int hw = nlat * nlon;
    const int P0 = std::min(n_planes, kPoleChunk);
    grow(fX, fX_have, (size_t)2 * P0 * hw);
    if (substeps > 0) {
      grow(fG, fG_have, (size_t)2 * P0 * hw);
      grow(fA, fA_have, (size_t)2 * P0 * hw);
      grow(cC, cC_have, (size_t)2 * P0 * lmax * mmax * 2);
    }
    for (int p0 = 0; p0 < n_planes; p0 += kPoleChunk) {
      const int P = std::min(kPoleChunk, n_planes - p0);
      const int64_t ph = (int64_t)P * hw;
      load(x, x_stride, dtype, p0, P, fX, stream);
      if (vec) load(v, v_stride, dtype, p0, P, fX + ph, stream);
      const int NP = vec ? 2 * P : P;                      // the planes of X
      if (cut > 0 && indpol > 0) {
        hipLaunchKernelGGL(polefilter_lowpass_kernel, dim3((unsigned)(2 * indpol), (unsigned)NP), dim3(256), (size_t)(cut + 1) * 16, stream, fX, nlat,
                           nlon, indpol, cut);
        WX_HIP(hipGetLastError());
      }
      double* cHi = cC + (int64_t)P * lmax * mmax * 2;
      for (int it = 0; it < substeps; ++it) {
        if (!vec) {
          sht.analysis(P, fX, hw, kShtF64, cC, stream);
          sht.vector_synthesis(P, cC, nullptr, s_grad, fG, fG + ph, kShtF64, stream);
        } else {
          sht.vector_analysis(P, fX, hw, fX + ph, hw, kShtF64, cC, cHi, stream);
          sht.vector_synthesis(P, cC, nullptr, s_divgrad, fG, fG + ph, kShtF64, stream);
        }
        sht.analysis(2 * P, fG, hw, kShtF64, cC, stream);
        sht.vector_synthesis(P, cC, nullptr, s_grad, fA, nullptr, kShtF64, stream);
        sht.vector_synthesis(P, cHi, nullptr, s_grad, nullptr, fA + ph, kShtF64, stream);
        if (!vec) {
          update(fX, fA, fA + ph, coef, ph, stream);
        } else {
          hipLaunchKernelGGL(polefilter_sum_kernel, dim3((unsigned)cdiv(ph, (int64_t)256)), dim3(256), 0, stream, fA, fA + ph, fG, ph);
          WX_HIP(hipGetLastError());
          sht.analysis(P, fG, hw, kShtF64, cC, stream);
          sht.vector_synthesis(P, cC, nullptr, s_grad, fA, fA + ph, kShtF64, stream);
          update(fX, fA, nullptr, -coef, 2 * ph, stream);
        }
      }
      store(fX, dtype, p0, P, x_out, x_out_stride, stream);
      if (vec) store(fX + ph, dtype, p0, P, v_out, v_out_stride, stream);
    }
  }
  void load(const void* src, int64_t stride, int dtype, int p0, int P, double* dst, hipStream_t stream) {
    const int hw = nlat * nlon;
    const dim3 grid((unsigned)cdiv(hw, 256), (unsigned)P);
    if (dtype == kShtF64) hipLaunchKernelGGL(polefilter_load_kernel<double>, grid, dim3(256), 0, stream, (const double*)src + (int64_t)p0 * stride, stride, hw, dst);
    else hipLaunchKernelGGL(polefilter_load_kernel<float>, grid, dim3(256), 0, stream, (const float*)src + (int64_t)p0 * stride, stride, hw, dst);
    WX_HIP(hipGetLastError());
  }
  void store(const double* src, int dtype, int p0, int P, void* dst, int64_t stride, hipStream_t stream) {
    const int hw = nlat * nlon;
    const dim3 grid((unsigned)cdiv(hw, 256), (unsigned)P);
    if (dtype == kShtF64) hipLaunchKernelGGL(polefilter_store_kernel<double>, grid, dim3(256), 0, stream, src, hw, (double*)dst + (int64_t)p0 * stride, stride);
    else hipLaunchKernelGGL(polefilter_store_kernel<float>, grid, dim3(256), 0, stream, src, hw, (float*)dst + (int64_t)p0 * stride, stride);
    WX_HIP(hipGetLastError());
  }
  void update(double* X, const double* a, const double* b, double coef, int64_t n, hipStream_t stream) {
    hipLaunchKernelGGL(polefilter_update_kernel, dim3((unsigned)cdiv(n, (int64_t)256)), dim3(256), 0, stream, X, a, b, sig, coef, nlat, nlon, n);
    WX_HIP(hipGetLastError());
  }
  void grow(double*& p, size_t& have, size_t want) {
    try {
      mem.grow(p, have, want);
    } catch (const HipError& e) {
      throw HipError("wx_polefilter: a work field of " + std::to_string(want * 8) + " bytes could not be allocated: " + e.what());
    }
  }

  Sht& sht;
  int nlat, nlon, lmax, mmax, indpol, cut, device;
  DeviceArena mem;
  double* s_grad = nullptr;
  double* s_divgrad = nullptr;
  float* sig = nullptr;
  double *fX = nullptr, *fG = nullptr, *fA = nullptr, *cC = nullptr;
  size_t fX_have = 0, fG_have = 0, fA_have = 0, cC_have = 0;
};

}  // namespace wx
