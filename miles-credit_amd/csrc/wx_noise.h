// Noise injection of the ensemble CrossFormer (credit/models/wxformer/crossformer_ensemble.py CrossFormerWithNoise,
// credit/models/wxformer/stochastic_decomposition_layer.py StochasticDecompositionLayer):
//     y = feature + ((noise_factor * r) * style[c]) * modulation[c],   style = Linear(z) = W z + b,   r ~ N(0, 1) per element
// in the reference's order of operations, fp32, on the engine's token-major maps ([H * W][ld], channels innermost).
//
// The device generator (the reference draws with torch.randn; these draws are a different, documented stream):
//   Philox4x32-10 (Salmon et al., SC'11; the Random123 constants M0 = 0xD2511F53, M1 = 0xCD9E8D57, W0 = 0x9E3779B9,
//   W1 = 0xBB67AE85), key = (seed & 0xffffffff, seed >> 32), counter = (q, slot, member, step):
//     q       quad index = e >> 2, e = the element's LOGICAL index in the reference's tensor of this draw:
//             pixel noise [C][H][W] of one member: e = (c * H + y) * W + x  (independent of the engine's storage layout,
//             launch geometry, precision and kernel variant); latent z [Dn]: e = j
//     slot    0 - 2 the encoder layers encoder_noise_layers.{0,1,2}, 3 - 5 the decoder layers noise_inject{1,2,3} (pixel noise);
//             6 + l the latent of layer slot l; with `correlated` one latent per forward, slot 6
//             16 (SLOT_PERTURB, csrc/wx_perturb.h) the white source of the perturbed-initial-condition noise: e = (p * H + h) * W + x
//             over the P = C * T planes of one member's [1, C, T, H, W] tensor; step = the forecast step
//     member  ensemble member (wx_set_noise member0 + batch row)
//     step    the forward / step coordinate (wx_set_noise step, advanced by one after every forward, wx_step and rollout step)
//   Box-Muller on the four output words (w0, w1, w2, w3) -> normals (n0, n1, n2, n3) of elements 4q .. 4q + 3:
//     u1 = ((w0 >> 8) + 1) * 2^-24  in (0, 1]  (never 0: log(0) = -inf would turn noise_factor = 0 into NaN)
//     u2 = (w1 >> 8) * 2^-24        in [0, 1)
//     rho = sqrt(-2 ln u1);  n0 = rho * cos(2 pi u2);  n1 = rho * sin(2 pi u2)     (sincospi(2 u2): 2 u2 is exact)
//     (n2, n3) the same from (w2, w3).  fp32 libm (logf, sqrtf, sincospif): a float64 restatement of the recipe agrees to a few ulp.
#pragma once
#include "wx_common.h"

namespace wx {

struct NoiseState {        // device-resident: the captured rollout graphs read it, the step is advanced on the device
  uint32_t seed_lo, seed_hi;
  int32_t member0;
  int32_t step;
};

__host__ __device__ inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

__device__ inline void box_muller(uint32_t w0, uint32_t w1, float& n0, float& n1) {
  const float u1 = (float)((w0 >> 8) + 1u) * 5.9604644775390625e-8f;
  const float u2 = (float)(w1 >> 8) * 5.9604644775390625e-8f;
  const float rho = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincospif(2.0f * u2, &s, &c);
  n0 = rho * c;
  n1 = rho * s;
}

// the four normals of quad q
__device__ inline void noise_quad(const NoiseState& st, uint32_t q, uint32_t slot, uint32_t member, float n[4]) {
  uint32_t c[4] = {q, slot, member, (uint32_t)st.step};
  philox4x32_10(c, st.seed_lo, st.seed_hi);
  box_muller(c[0], c[1], n[0], n[1]);
  box_muller(c[2], c[3], n[2], n[3]);
}

// normals of the logical elements e0 .. e0 + 3 (one quad when e0 % 4 == 0, else the two it straddles)
__device__ inline void noise_run4(const NoiseState& st, int64_t e0, uint32_t slot, uint32_t member, float r[4]) {
  float a[4];
  noise_quad(st, (uint32_t)(e0 >> 2), slot, member, a);
  const int off = (int)(e0 & 3);
  if (off == 0) {
    r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = a[3];
    return;
  }
  float b[4];
  noise_quad(st, (uint32_t)(e0 >> 2) + 1u, slot, member, b);
  // k = off + i in 1 .. 6: select without a dynamically indexed register array
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = off + i;
    r[i] = k == 1 ? a[1] : k == 2 ? a[2] : k == 3 ? a[3] : k == 4 ? b[0] : k == 5 ? b[1] : b[2];
  }
}

// style[slot][c] = bias[c] + sum_j W[c][j] z[j] for every active slot of one batch row; z from the generator or a tape
struct NoiseStyleParams {
  const float* w[6];        // [C][Dn] in the float arena, nullptr = slot inactive
  const float* bias[6];     // [C]
  const float* tape_z[6];   // [Dn] of this batch row, or nullptr (generator)
  int C[6];
  float* style;             // [6][cstride]
  int cstride, Dn, correlated, row;
  const NoiseState* st;
};

__global__ __launch_bounds__(256) void noise_style_kernel(NoiseStyleParams p) {
  extern __shared__ float nz_z[];   // [Dn rounded up to 4]
  const int slot = blockIdx.x;
  if (!p.w[slot]) return;
  const NoiseState st = *p.st;
  if (p.tape_z[slot]) {
    for (int j = threadIdx.x; j < p.Dn; j += 256) nz_z[j] = p.tape_z[slot][j];
  } else {
    const uint32_t zslot = p.correlated ? 6u : 6u + (uint32_t)slot;
    for (int q = threadIdx.x; q < (p.Dn + 3) / 4; q += 256) {
      float n[4];
      noise_quad(st, (uint32_t)q, zslot, (uint32_t)(st.member0 + p.row), n);
      *reinterpret_cast<float4*>(nz_z + 4 * q) = make_float4(n[0], n[1], n[2], n[3]);
    }
  }
  __syncthreads();
  const float* w = p.w[slot];
  for (int c = threadIdx.x; c < p.C[slot]; c += 256) {
    float acc = 0.f;
    for (int j = 0; j < p.Dn; ++j) acc = fmaf(w[(int64_t)c * p.Dn + j], nz_z[j], acc);
    p.style[slot * p.cstride + c] = acc + p.bias[slot][c];
  }
}

// In place on a token-major map x[H * W][ld] (C channels): every thread owns four consecutive pixels of one 16-byte channel
// chunk, so the four normals of a Philox call land on four elements of the same channel (consecutive logical indices).
template <typename T>
struct NoiseInjectParams {
  T* x;
  int64_t ld;
  int HW, C;
  const float* style;       // [C] of this slot and row
  const float* nf;          // [1]
  const float* mod;         // [C]
  const float* tape;        // [C][HW] of this row, or nullptr (generator)
  const NoiseState* st;
  int slot, row;
};

template <typename T>
__global__ __launch_bounds__(256) void noise_inject_kernel(NoiseInjectParams<T> p) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const int pieces = p.C / VEC;
  const int64_t groups = ((int64_t)p.HW + 3) / 4;
  const int64_t total = groups * pieces;
  const NoiseState st = *p.st;
  const float nf = *p.nf;
  const uint32_t member = (uint32_t)(st.member0 + p.row);
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t g = idx / pieces;
    const int c0 = (int)(idx - g * pieces) * VEC;
    const int64_t p0 = 4 * g;
    const int np = (int)min((int64_t)4, (int64_t)p.HW - p0);
    float f[4][VEC] = {};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < np) unpack16<T>(*reinterpret_cast<const uint4*>(p.x + (p0 + i) * p.ld + c0), f[i]);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int c = c0 + e;
      const int64_t e0 = (int64_t)c * p.HW + p0;
      float r[4];
      if (p.tape) {
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = i < np ? p.tape[e0 + i] : 0.f;
      } else {
        noise_run4(st, e0, (uint32_t)p.slot, member, r);
      }
      const float sc = p.style[c], md = p.mod[c];
#pragma unroll
      for (int i = 0; i < 4; ++i) f[i][e] = __fadd_rn(f[i][e], __fmul_rn(__fmul_rn(__fmul_rn(nf, r[i]), sc), md));   // no contraction: the reference's rounding
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < np) *reinterpret_cast<uint4*>(p.x + (p0 + i) * p.ld + c0) = pack16<T>(f[i]);
  }
}

__global__ void noise_step_kernel(NoiseState* st) {
  if (threadIdx.x == 0) st->step += 1;
}

}  // namespace wx
