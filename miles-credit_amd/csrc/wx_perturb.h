// Perturbed-initial-condition ensembles on the device: the reference's noise generators for deterministic checkpoints,
//   credit/ensemble/gaussian.py::GaussianNoise      delta = amplitude * r,                        r ~ N(0, 1) per element
//   credit/ensemble/color.py::ColorNoise            delta = amplitude * irfft2(rfft2(r) * S, s = (H, W)),   S [H][W/2 + 1] float32
//   credit/ensemble/temporal.py::TemporalNoise      delta_t = rho * delta_{t-1} + eps_t, per-channel std, hemispheric rescale
// One handle per grid (H, W); a call acts on the P = C * T planes of one member's [1, C, T, H, W] tensor (plane p at p * stride).
//
// White source r: a tape (float32, logical [P][H][W], the reference's torch.randn draws replayed) or the generator of wx_noise.h
// (noise_quad / noise_run4, nothing restated): counter (q, slot, member, step) with q = e >> 2, e = (p * H + h) * W + x the element's
// logical index in the member's tensor, slot SLOT_PERTURB = 16 (slots 0 - 11 are the noise-injection model's).  A row start is in
// general not quad-aligned: noise_run4.  A draw depends on (seed, member, step, e) alone: not on the launch geometry, the plane
// batching, the plane count or on which other members or steps were drawn.
//
// Kind colour: the dense fp64 DFTs of wx_dft.h (MFMA lane layout, LDS twiddle table, DftPhase and the fixed sum order are stated
// there); Wh = W / 2 + 1, a complex number is (re, im) interleaved, so a half-complex row is 2 Wh doubles:
//   pass A  perturb_rows_fwd_kernel   lon, real -> half-complex    X1[(p, h)][n] = sum_x r[(p, h)][x] T_W[x][n]          M = Pb H, N = 2 Wh, K = W
//                                     T_W[x][2k] = cos(2 pi k x / W), T_W[x][2k + 1] = -sin(2 pi k x / W); unfolded
//   pass B  perturb_cols_kernel       lat, complex, two launches: forward with the product by S in the store, then inverse (+i, unscaled)
//                                     per plane  D[l][n] = sum_h cos(.) X[h][n] + (-+sin(.)) Xs[h][n],  (.) = 2 pi l h / H,
//                                     Xs[h][2k] = -X[h][2k + 1], Xs[h][2k + 1] = X[h][2k]                               M = H, N = 2 Wh, K = H
//   pass C  perturb_rows_inv_kernel   lon, half-complex -> real: dft_rows_inverse, scale 1 / (H W), then the epilogue   M = Pb H, N = W, K = 2 Wh
// A wave owns a 16 x 64 tile of D (four accumulators; the A operand is shared by the four), a workgroup of four waves 64 x 64.
// A plane's result is bit-identical whatever P, the batch split or its position in the batch.
// Intermediates are complex fp64 in two scratch buffers of the handle, processed in plane batches: a plane takes 2 * 16 H Wh bytes
// (16.6 MB at 721 x 1440), a batch is min(kPerturbMaxBatch = 64, kPerturbScratchBytes = 256 MiB / that) planes -- 16 planes, 266 MB, at
// 721 x 1440 -- plus 4 H W bytes per plane for the generator's draws (the generator fills a tape of its own for a batch, so that no
// column block of pass A repeats the Philox rounds).  Calls on one handle must be ordered by one stream.
//
// Epilogue (perturb_emit), fused into pass C (white: the only kernel), per element, every operation rounded once (no contraction), the
// reference's order:
//   n   = (float) y                       the reference's float32 `correlated_noise` (white: r)
//   eps = amplitude * n                   ColorNoise / GaussianNoise
//   eps = eps * chan_scale[p]             optional; TemporalNoise: perturbation_std[c] / amplitude
//   d   = prev ? rho * prev + eps : eps   optional AR(1)
//   d   = d * lat_weight[h]               optional hemispheric rescale
//   delta_out = d;  x_out = x + d         either optional; x_out may be x, delta_out may be prev (same pointer and stride)
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "wx_common.h"
#include "wx_dft.h"
#include "wx_noise.h"

namespace wx {

constexpr uint32_t SLOT_PERTURB = 16;
constexpr int kPerturbWhite = 0;
constexpr int kPerturbColour = 1;
constexpr int kPerturbMaxBatch = 64;
constexpr int64_t kPerturbScratchBytes = 256LL << 20;    // both complex buffers of a batch
constexpr int64_t kPerturbMaxElems = 1LL << 34;          // q = e >> 2 is a 32-bit counter word

struct PerturbEpi {
  float amplitude, rho;
  const float* chan_scale;   // device [P] or nullptr
  const float* lat_w;        // device [H] or nullptr
  const float* prev;
  const float* x;
  float* delta_out;
  float* x_out;
  int64_t prev_stride, x_stride, delta_stride, xout_stride;
};

// ---- host-only helpers (no HIP call) ---------------------------------------------------------------------------------------------
inline int64_t perturb_plane_bytes(int H, int W) { return 2LL * 16 * H * (W / 2 + 1); }
inline int perturb_batch_planes(int H, int W) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(kPerturbMaxBatch, kPerturbScratchBytes / perturb_plane_bytes(H, W)));
}

// "" or the reason wx_perturb_create refuses.
inline std::string perturb_check_create(int H, int W, int kind, const float* S) {
  if (kind != kPerturbWhite && kind != kPerturbColour) return "kind must be 0 (white) or 1 (colour), got " + std::to_string(kind);
  if (H < 1 || W < 2) return "H must be >= 1 and W >= 2, got " + std::to_string(H) + " x " + std::to_string(W);
  if ((int64_t)H * W > kPerturbMaxElems) return "H * W is beyond the generator's counter (2^34 elements)";
  if (kind == kPerturbColour) {
    if (H > kDftMaxN || W > kDftMaxN)
      return "the colour filter takes grids up to " + std::to_string(kDftMaxN) + " points a side, got " + std::to_string(H) + " x " + std::to_string(W);
    if (!S) return "the colour filter needs the spectral weights S [H][W / 2 + 1], got a null pointer";
    const int64_t n = (int64_t)H * (W / 2 + 1);
    for (int64_t i = 0; i < n; ++i)
      if (!std::isfinite(S[i])) return "the spectral weights S must be finite, entry " + std::to_string(i) + " is not";
  }
  return "";
}

// "" or the reason wx_perturb_apply refuses, decided on the host before anything is launched or copied.
inline std::string perturb_check_apply(int H, int W, int n_planes, const float* tape, const float* prev, int64_t prev_stride, const float* x,
                                       int64_t x_stride, const float* delta_out, int64_t delta_stride, const float* x_out, int64_t xout_stride) {
  const int64_t hw = (int64_t)H * W;
  if (n_planes < 1) return "n_planes must be >= 1, got " + std::to_string(n_planes);
  if (n_planes > kPerturbMaxElems / hw) return "H * W * n_planes = " + std::to_string(hw) + " * " + std::to_string(n_planes) + " is beyond the generator's counter (2^34 elements)";
  if (!delta_out && !x_out) return "no output requested: delta_out and x_out are both null";
  if (x_out && !x) return "x_out needs x";
  const auto small = [&](const float* p, int64_t s) { return p && s < hw; };
  if (small(prev, prev_stride) || small(x_out ? x : nullptr, x_stride) || small(delta_out, delta_stride) || small(x_out, xout_stride))
    return "a plane stride is smaller than H * W = " + std::to_string(hw);
  const auto far = [&](const float* p, int64_t s) {      // the planes' extent must be a number the overlap tests can work with
    int64_t v = 0;
    return p && (__builtin_mul_overflow((int64_t)(n_planes - 1), s, &v) || __builtin_add_overflow(v, hw, &v) || v > (1LL << 44));
  };
  if (far(prev, prev_stride) || far(x_out ? x : nullptr, x_stride) || far(delta_out, delta_stride) || far(x_out, xout_stride))
    return "a plane stride takes the planes beyond 2^44 floats";
  const auto span = [&](int64_t s) { return ((int64_t)(n_planes - 1) * s + hw) * 4; };   // bytes
  const int64_t tape_bytes = hw * n_planes * 4;
  if (tape && ((delta_out && bytes_overlap(tape, tape_bytes, delta_out, span(delta_stride))) ||
               (x_out && bytes_overlap(tape, tape_bytes, x_out, span(xout_stride)))))
    return "the tape overlaps an output: a later plane batch would read draws that an earlier one has overwritten";
  // an input may be an output's own memory element for element, never a shifted view of it
  const auto shifted = [&](const float* in, int64_t si, const float* out, int64_t so) {
    return in && out && bytes_overlap(in, span(si), out, span(so)) && !(in == out && si == so);
  };
  if (shifted(prev, prev_stride, delta_out, delta_stride) || shifted(prev, prev_stride, x_out, xout_stride) ||
      (x_out && (shifted(x, x_stride, x_out, xout_stride) || shifted(x, x_stride, delta_out, delta_stride))) ||
      shifted(delta_out, delta_stride, x_out, xout_stride) || (delta_out && x_out && delta_out == x_out))
    return "an input overlaps an output without being the same view (same pointer and stride), or the two outputs overlap";
  return "";
}

// ---- device side -------------------------------------------------------------------------------------------------------------------
// One element's epilogue.  Inputs are read before outputs are written: x_out may be x and delta_out may be prev.
__device__ inline void perturb_emit(const PerturbEpi& e, int64_t p, int h, int x, int W, float n) {
  // Plain operators under contract(off): __fmul_rn / __fadd_rn are inline functions of plain operators that carry their own scope's
  // contraction into the caller, where rho * prev + eps then becomes one FMA.
#pragma clang fp contract(off)
  const int64_t o = (int64_t)h * W + x;
  float d = e.amplitude * n;
  if (e.chan_scale) d = d * e.chan_scale[p];
  if (e.prev) {
    const float carried = e.rho * e.prev[p * e.prev_stride + o];
    d = carried + d;
  }
  if (e.lat_w) d = d * e.lat_w[h];
  const float xv = e.x_out ? e.x[p * e.x_stride + o] : 0.f;
  if (e.delta_out) e.delta_out[p * e.delta_stride + o] = d;
  if (e.x_out) e.x_out[p * e.xout_stride + o] = xv + d;
}

// The white kinds and the generator's fill of a batch: one thread per four consecutive x of one row (p, h), planes p0 .. p0 + np - 1.
// RAW: the draws go to raw[(p - p0) H W + h W + x] unscaled (pass A's input); else through the epilogue.  grid = ceil(np H ceil(W / 4) / 256)
template <bool RAW>
__global__ __launch_bounds__(256) void perturb_white_kernel(const float* tape, NoiseState st, int64_t p0, int np, int H, int W, float* raw,
                                                            PerturbEpi epi) {
  const int G = (W + 3) >> 2;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)np * H * G) return;
  const int64_t lrow = idx / G;                       // local row: (p - p0) H + h
  const int x0 = (int)(idx - lrow * G) * 4;
  const int64_t row = p0 * H + lrow;
  const int64_t e0 = row * W + x0;
  const int nx = min(4, W - x0);
  float r[4];
  if (tape) {
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = i < nx ? tape[e0 + i] : 0.f;
  } else {
    noise_run4(st, e0, SLOT_PERTURB, (uint32_t)st.member0, r);
  }
  if (RAW) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nx) raw[lrow * W + x0 + i] = r[i];
  } else {
    const int64_t p = row / H;
    const int h = (int)(row - p * H);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nx) perturb_emit(epi, p, h, x0 + i, W, r[i]);
  }
}

// Pass A.  src [M][W] float32 (M = Pb H rows), out [M][2 Wh] fp64.  grid = (ceil(2 Wh / 64), ceil(M / 64)), LDS 16 W bytes.
__global__ __launch_bounds__(256) void perturb_rows_fwd_kernel(const float* __restrict__ src, int M, int W, const double2* __restrict__ tab_g,
                                                               double* __restrict__ out) {
  extern __shared__ double2 perturb_tab[];
  dft_stage_table(perturb_tab, tab_g, W);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int N = 2 * (W / 2 + 1);
  const int m0 = ((int)blockIdx.y * 4 + wave) * 16, n0 = (int)blockIdx.x * 64;
  if (m0 >= M) return;                                 // wave-uniform, after the only barrier
  const int row = m0 + c;
  const bool row_ok = row < M;
  const float* srow = src + (int64_t)(row_ok ? row : 0) * W;
  DftPhase ph[4];
  bool im[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int n = n0 + 16 * t + c;
    im[t] = n & 1;
    ph[t].init(n >> 1, 4 * g, 12, W);
  }
  f64x4_t acc[4] = {};
  for (int kc = 0; kc < W; kc += 16) {
    const int x0 = kc + 4 * g;
    double a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = (row_ok && x0 + j < W) ? (double)srow[x0 + j] : 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double2 cs = perturb_tab[ph[t].idx];
        acc[t] = mfma_f64_16x16x4(a[j], im[t] ? -cs.y : cs.x, acc[t]);
        ph[t].step(W);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) ph[t].skip(W);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int n = n0 + 16 * t + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + g + 4 * r;
      if (m < M && n < N) out[(int64_t)m * N + n] = acc[t][r];
    }
  }
}

// Pass B.  in, out [Pb][H][N = 2 Wh] fp64 (never the same buffer).  sgn = -1 forward, +1 inverse; S [H][Wh] float32 or nullptr.
// grid = (ceil(N / 64), ceil(H / 64), Pb), LDS 16 H bytes.
__global__ __launch_bounds__(256) void perturb_cols_kernel(const double* __restrict__ in, int H, int N, double sgn, const float* __restrict__ S,
                                                           const double2* __restrict__ tab_g, double* __restrict__ out) {
  extern __shared__ double2 perturb_tab[];
  dft_stage_table(perturb_tab, tab_g, H);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int m0 = ((int)blockIdx.y * 4 + wave) * 16, n0 = (int)blockIdx.x * 64;
  if (m0 >= H) return;
  const int64_t plane = (int64_t)blockIdx.z * H * N;
  const double* X = in + plane;
  DftPhase ph;
  ph.init(m0 + c, 4 * g, 12, H);                       // k = l, the output row
  f64x4_t acc[4] = {};
  for (int kc = 0; kc < H; kc += 16) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int h = kc + 4 * g + j;
      const double2 cs = perturb_tab[ph.idx];
      const double ca = cs.x, sa = sgn * cs.y;
      ph.step(H);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int n = n0 + 16 * t + c;
        const bool ok = h < H && n < N;
        const double v = ok ? X[(int64_t)h * N + n] : 0.0;
        const double w = ok ? X[(int64_t)h * N + (n ^ 1)] : 0.0;   // N is even: n ^ 1 < N
        acc[t] = mfma_f64_16x16x4(ca, v, acc[t]);
        acc[t] = mfma_f64_16x16x4(sa, (n & 1) ? w : -w, acc[t]);
      }
    }
    ph.skip(H);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int n = n0 + 16 * t + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + g + 4 * r;
      if (m < H && n < N) {
        double v = acc[t][r];
        if (S) v *= (double)S[(int64_t)m * (N >> 1) + (n >> 1)];
        out[plane + (int64_t)m * N + n] = v;
      }
    }
  }
}

// Pass C.  in [M][N = 2 Wh] fp64 (M = Pb H rows of planes p0 ..), then the epilogue.  grid = (ceil(W / 64), ceil(M / 64)), LDS 16 W bytes.
__global__ __launch_bounds__(256) void perturb_rows_inv_kernel(const double* __restrict__ in, int M, int H, int W, double scale,
                                                               const double2* __restrict__ tab_g, int64_t p0, PerturbEpi epi) {
  extern __shared__ double2 perturb_tab[];
  dft_stage_table(perturb_tab, tab_g, W);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int Wh = W / 2 + 1, N = 2 * Wh;
  const int m0 = ((int)blockIdx.y * 4 + wave) * 16, n0 = (int)blockIdx.x * 64;
  if (m0 >= M) return;
  const int row = m0 + c;
  const bool row_ok = row < M;
  const double* zrow = in + (int64_t)(row_ok ? row : 0) * N;
  f64x4_t acc[4] = {};
  dft_rows_inverse([&](int k) { return (row_ok && k < Wh) ? make_double2(zrow[2 * k], zrow[2 * k + 1]) : make_double2(0.0, 0.0); }, Wh, W, n0,
                   perturb_tab, acc);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int x = n0 + 16 * t + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + g + 4 * r;
      if (m < M && x < W) {
        const int pl = m / H;
        perturb_emit(epi, p0 + pl, m - pl * H, x, W, (float)(acc[t][r] * scale));
      }
    }
  }
}

class Perturb {
 public:
  Perturb(int H_, int W_, int kind_, const float* S_host, int dev) : H(H_), W(W_), kind(kind_), device(dev), mem(dev) {
    WX_HIP(hipSetDevice(device));
    if (kind == kPerturbColour) {
      std::vector<double2> t;
      dft_table(W, t);
      tab_w = mem.upload(t.data(), t.size());
      dft_table(H, t);
      tab_h = mem.upload(t.data(), t.size());
      S = mem.upload(S_host, (size_t)H * (W / 2 + 1));
    }
  }
  int batch_planes() const { return perturb_batch_planes(H, W); }

  void apply(int n_planes, const float* tape, uint64_t seed, int member, int step, float amplitude, const float* chan_scale_host, float rho,
             const float* prev, int64_t prev_stride, const float* lat_weight_host, const float* x, int64_t x_stride, float* delta_out,
             int64_t delta_stride, float* x_out, int64_t xout_stride, hipStream_t stream) {
    const std::string why = perturb_check_apply(H, W, n_planes, tape, prev, prev_stride, x, x_stride, delta_out, delta_stride, x_out, xout_stride);
    if (!why.empty()) throw std::runtime_error("wx_perturb_apply: " + why);
    WX_HIP(hipSetDevice(device));
    PerturbEpi epi;
    epi.amplitude = amplitude; epi.rho = rho;
    epi.chan_scale = stage(chan_scale_host, (size_t)n_planes, cs_host, cs_dev, cs_have, stream);
    epi.lat_w = stage(lat_weight_host, (size_t)H, lw_host, lw_dev, lw_have, stream);
    epi.prev = prev; epi.x = x_out ? x : nullptr; epi.delta_out = delta_out; epi.x_out = x_out;
    epi.prev_stride = prev_stride; epi.x_stride = x_stride; epi.delta_stride = delta_stride; epi.xout_stride = xout_stride;
    NoiseState st;
    st.seed_lo = (uint32_t)(seed & 0xffffffffu); st.seed_hi = (uint32_t)(seed >> 32); st.member0 = member; st.step = step;
    const int G = (W + 3) >> 2;
    if (kind == kPerturbWhite) {
      const int64_t total = (int64_t)n_planes * H * G;
      hipLaunchKernelGGL(perturb_white_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, tape, st, (int64_t)0, n_planes, H,
                         W, (float*)nullptr, epi);
      WX_HIP(hipGetLastError());
      return;
    }
    const int Wh = W / 2 + 1, N = 2 * Wh;
    const int nb_max = std::min(batch_planes(), n_planes);
    mem.grow(buf_a, a_have, (size_t)nb_max * H * N);
    mem.grow(buf_b, b_have, (size_t)nb_max * H * N);
    if (!tape) mem.grow(raw, raw_have, (size_t)nb_max * H * W);
    const double scale = 1.0 / ((double)H * (double)W);
    for (int p0 = 0; p0 < n_planes; p0 += nb_max) {
      const int nb = std::min(nb_max, n_planes - p0);
      const int M = nb * H;
      const float* src = tape ? tape + (int64_t)p0 * H * W : raw;
      if (!tape) {
        const int64_t total = (int64_t)nb * H * G;
        hipLaunchKernelGGL(perturb_white_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const float*)nullptr, st,
                           (int64_t)p0, nb, H, W, raw, epi);
      }
      const dim3 rows_grid((unsigned)cdiv(N, 64), (unsigned)cdiv(M, 64)), cols_grid((unsigned)cdiv(N, 64), (unsigned)cdiv(H, 64), (unsigned)nb);
      hipLaunchKernelGGL(perturb_rows_fwd_kernel, rows_grid, dim3(256), dft_lds_bytes(W), stream, src, M, W, tab_w, buf_a);
      hipLaunchKernelGGL(perturb_cols_kernel, cols_grid, dim3(256), dft_lds_bytes(H), stream, buf_a, H, N, -1.0, S, tab_h, buf_b);
      hipLaunchKernelGGL(perturb_cols_kernel, cols_grid, dim3(256), dft_lds_bytes(H), stream, buf_b, H, N, 1.0, (const float*)nullptr,
                         tab_h, buf_a);
      hipLaunchKernelGGL(perturb_rows_inv_kernel, dim3((unsigned)cdiv(W, 64), (unsigned)cdiv(M, 64)), dim3(256), dft_lds_bytes(W), stream,
                         buf_a, M, H, W, scale, tab_w, (int64_t)p0, epi);
    }
    WX_HIP(hipGetLastError());
  }

 private:
  // A small host array of a call on the device; uploaded again only when its values change.  The earlier calls on the stream may still
  // read the old values: they are waited for first.
  const float* stage(const float* host, size_t n, std::vector<float>& mirror, float*& dev, size_t& have, hipStream_t stream) {
    if (!host) return nullptr;
    if (dev && mirror.size() == n && std::memcmp(mirror.data(), host, n * sizeof(float)) == 0) return dev;
    WX_HIP(hipStreamSynchronize(stream));
    mirror.clear();
    mem.grow(dev, have, n);
    WX_HIP(hipMemcpy(dev, host, n * sizeof(float), hipMemcpyHostToDevice));
    mirror.assign(host, host + n);
    return dev;
  }

  int H, W, kind, device;
  DeviceArena mem;
  double2* tab_w = nullptr;
  double2* tab_h = nullptr;
  float* S = nullptr;
  double* buf_a = nullptr;
  double* buf_b = nullptr;
  float* raw = nullptr;
  float* cs_dev = nullptr;
  float* lw_dev = nullptr;
  size_t a_have = 0, b_have = 0, raw_have = 0, cs_have = 0, lw_have = 0;
  std::vector<float> cs_host, lw_host;
};

}  // namespace wx
