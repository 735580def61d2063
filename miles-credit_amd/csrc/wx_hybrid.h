// Hybrid-level interpolation of the gen-2 block chains on the device: 3-D variables from one set of hybrid sigma-pressure levels onto
// another, linear in log p, column by column:
//   credit/postblock/hybrid_interp.py:29, :61-62   p = max(a + b sp, 0.57 Pa) for source and destination, from the SAME sp
//   credit/postblock/hybrid_interp.py:100-106      source orientation from the coefficients at 101325 Pa; :133-134 the flip
//   credit/postblock/_interp_utils.py:30-40        loglinear_interp_columns: cnt = #{m : p_dst >= p_src[m]}, hi = clamp(cnt, 1, Ls - 1),
//                                                  lo = hi - 1, w = clamp((log p_dst - log p_lo) / (log p_hi - log p_lo), 0, 1),
//                                                  y = y_lo + w (y_hi - y_lo): constant extrapolation outside the source range
// The reference runs this as torch.vmap over columns in chunks of 1000 behind a permute of the whole state.  Here one thread owns one
// column (b, t, cell) of the named tensors as they lie in memory, [B][L][T][H][W] fp32 (the layout of wx_diag.h): the level stride is
// T*H*W, adjacent threads read adjacent cells, every access is coalesced and nothing is permuted or staged.
//
// Brackets cost no traffic.  The bracket of a destination level depends on sp and the coefficients alone.  The host sorts the
// destination levels by their pressure at 101325 Pa once (hybrid_plan) and uploads the coefficients in that order with the permutation;
// a workgroup copies them into LDS (at most 4 x 137 floats + 137 ints, whatever the workgroup size).  A thread visits the destination
// levels in sorted order and finds each bracket by walking a pointer forward over the source pressures, recomputed from the
// coefficients in LDS: no field value is touched.  Where the a / b families cross, a column's own destination order can differ from the
// order at 101325 Pa; the pointer restarts at 0 whenever p_dst decreases, which costs time in those columns only.  With
// non-decreasing source pressures (the reference's precondition) the walk ends at the reference's count; outside that precondition
// every index still lies in [0, Ls - 1].
// Each needed source value is read once: the thread holds the values of its current lo and hi level in registers and loads a
// bracketing level only when it is neither of the two it holds (hi of one destination level is commonly lo of the next, and with
// Ld > Ls the bracket often does not move).  Source levels that bracket nothing are never fetched.  The loop is software-pipelined:
// the bracket of destination level i + 1 is found and its loads are issued BEFORE level i is blended and stored, so the load latency
// hides under the blend, the store and the next walk and does not rest on occupancy alone.
// Arithmetic is fp32.  p_src and p_dst come from ONE function, hybrid_pressure (an explicit fmaf and the floor): equal coefficients
// give equal bits, so with destination == source the weight is exactly 0 (1 at the highest pressure).  The bracket is decided on the
// pressures (log is monotonic) and the weight is log(p_dst / p_lo) / log(p_hi / p_lo), the quotient-of-ratios form of wx_diag.h
// (lines 20-24), which keeps the digits that subtracting two rounded logarithms loses.
// Launch grouping: one call takes up to 32 variables, in launches of at most kHybridGroup = 8 (kernel instances for 1 .. 8): 4 x 8
// value registers per thread.  A variable's result depends on its own values and the column's brackets alone, so every grouping
// gives the same bits per variable.  Inputs are read in place through (pointer, batch stride) pairs and never written.
// Supported range: 2 <= Ls <= 137 (a single source level has no bracket: the reference's gather fails there), 1 <= Ld <= 137,
// B * T * H * W < 2^31 columns; offsets are 64-bit.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "wx_common.h"

namespace wx {

constexpr int kHybridMaxLevels = 137;
constexpr int kHybridMaxVars = 32;
constexpr int kHybridGroup = 8;
constexpr float kHybridMinPressure = 0.57f;   // hybrid_interp.py:29

struct HybridVars {
  const float* src[kHybridGroup];   // variable v, batch item b at src[v] + b * bstride[v]: [Ls][T][hw]
  float* dst[kHybridGroup];         // [B][Ld][T][hw]
  int64_t bstride[kHybridGroup];    // in floats
};

struct HybridGeom {
  int Ls, Ld, flip;            // flip: the data's source level axis runs surface -> top
  int64_t thw, ncol;           // T*H*W, B*T*H*W
  const float* coef;           // device: a_src[Ls] | b_src[Ls] (top -> surface) | a_dst[Ld] | b_dst[Ld] (sorted order)
  const int* perm;             // device: [Ld] stored index of the i-th destination level in sorted order
};

// ---- host-only helpers (no HIP call) ---------------------------------------------------------------------------------------------
// "" or the reason wx_hybrid_create refuses
inline std::string hybrid_check_create(int H, int W, int n_src, const float* a_src, const float* b_src, int n_dst, const float* a_dst,
                                       const float* b_dst) {
  if (H < 1 || W < 1) return "bad geometry";
  if (n_src == 1) return "a single source level has no bracket to interpolate in (the reference's gather fails there); n_src must be 2 .. 137";
  if (n_src < 2 || n_src > kHybridMaxLevels) return "n_src must be 2 .. 137, got " + std::to_string(n_src);
  if (n_dst < 1 || n_dst > kHybridMaxLevels) return "n_dst must be 1 .. 137, got " + std::to_string(n_dst);
  if (!a_src || !b_src || !a_dst || !b_dst) return "null coefficient array";
  for (int m = 0; m < n_src; ++m)
    if (!std::isfinite(a_src[m]) || !std::isfinite(b_src[m])) return "non-finite source coefficient at level " + std::to_string(m);
  for (int j = 0; j < n_dst; ++j)
    if (!std::isfinite(a_dst[j]) || !std::isfinite(b_dst[j])) return "non-finite destination coefficient at level " + std::to_string(j);
  return "";
}

// What the device gets, from midpoint coefficients in stored order: the source flip (hybrid_interp.py:100-106), the source
// coefficients top -> surface, the destination coefficients sorted by their pressure at 101325 Pa (stable) and that permutation.
struct HybridPlan {
  bool flip;
  std::vector<float> coef;   // a_src | b_src | a_dst | b_dst
  std::vector<int> perm;
};
inline HybridPlan hybrid_plan(int Ls, const float* a_src, const float* b_src, int Ld, const float* a_dst, const float* b_dst) {
  HybridPlan p;
  auto ref = [](float a, float b) {      // the reference's float32 a + b * 101325: a rounded product, then a rounded sum
    const float prod = b * 101325.0f;
    return a + prod;
  };
  p.flip = ref(a_src[0], b_src[0]) > ref(a_src[Ls - 1], b_src[Ls - 1]);
  p.coef.resize(2 * (size_t)Ls + 2 * (size_t)Ld);
  for (int m = 0; m < Ls; ++m) {
    const int s = p.flip ? Ls - 1 - m : m;
    p.coef[m] = a_src[s];
    p.coef[Ls + m] = b_src[s];
  }
  p.perm.resize(Ld);
  for (int j = 0; j < Ld; ++j) p.perm[j] = j;
  std::stable_sort(p.perm.begin(), p.perm.end(), [&](int x, int y) { return ref(a_dst[x], b_dst[x]) < ref(a_dst[y], b_dst[y]); });
  for (int i = 0; i < Ld; ++i) {
    p.coef[2 * Ls + i] = a_dst[p.perm[i]];
    p.coef[2 * Ls + Ld + i] = b_dst[p.perm[i]];
  }
  return p;
}

// ---- device side -------------------------------------------------------------------------------------------------------------------
// hybrid_interp.py:61-62 for source and destination alike: one function, one explicit FMA, so equal coefficients give equal bits
__device__ __forceinline__ float hybrid_pressure(float a, float b, float sp) { return fmaxf(fmaf(b, sp, a), kHybridMinPressure); }

struct HybridBracket {
  int lo, hi;
  float w;
};

// grid = ceil(ncol / 256)
template <int NV>
__global__ __launch_bounds__(256) void hybrid_interp_kernel(const HybridVars v, const HybridGeom g, const float* __restrict__ sp,
                                                            int64_t sp_bs) {
  __shared__ float s_coef[4 * kHybridMaxLevels];
  __shared__ int s_perm[kHybridMaxLevels];
  const int Ls = g.Ls, Ld = g.Ld;
  for (int i = threadIdx.x; i < 2 * Ls + 2 * Ld; i += 256) s_coef[i] = g.coef[i];
  for (int i = threadIdx.x; i < Ld; i += 256) s_perm[i] = g.perm[i];
  __syncthreads();
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= g.ncol) return;
  const float* sa = s_coef;
  const float* sb = s_coef + Ls;
  const float* da = s_coef + 2 * Ls;
  const float* db = da + Ld;
  const int64_t thw = g.thw;
  const int64_t b = n / thw, rem = n - b * thw;      // rem = t * HW + cell
  const float ps = sp[b * sp_bs + rem];
  const float* col[NV];
  float* out[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    col[k] = v.src[k] + b * v.bstride[k] + rem;      // + stored level * thw
    out[k] = v.dst[k] + b * Ld * thw + rem;          // + stored level * thw
  }

  int ptr = 0;             // source levels (top -> surface) passed by the walk: the count of _interp_utils.py:33
  float p_prev = 0.f;      // every pressure is >= 0.57
  auto bracket = [&](int i) {
    const float pd = hybrid_pressure(da[i], db[i], ps);
    if (pd < p_prev) ptr = 0;                        // this column's order differs from the order at 101325 Pa: walk again
    p_prev = pd;
    while (ptr < Ls && pd >= hybrid_pressure(sa[ptr], sb[ptr], ps)) ++ptr;
    HybridBracket r;
    r.hi = min(max(ptr, 1), Ls - 1);
    r.lo = r.hi - 1;
    const float p_lo = hybrid_pressure(sa[r.lo], sb[r.lo], ps), p_hi = hybrid_pressure(sa[r.hi], sb[r.hi], ps);
    r.w = fminf(fmaxf(logf(pd / p_lo) / logf(p_hi / p_lo), 0.f), 1.f);
    return r;
  };
  auto level_offset = [&](int m) { return (int64_t)(g.flip ? Ls - 1 - m : m) * thw; };

  HybridBracket cur = bracket(0);
  float y_lo[NV], y_hi[NV];
  {
    const int64_t o_lo = level_offset(cur.lo), o_hi = level_offset(cur.hi);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      y_lo[k] = col[k][o_lo];
      y_hi[k] = col[k][o_hi];
    }
  }
  for (int i = 0; i < Ld; ++i) {
    HybridBracket nxt = cur;
    float n_lo[NV], n_hi[NV];
    if (i + 1 < Ld) {      // the next level's bracket and loads first: they are in flight while this level is blended and stored
      nxt = bracket(i + 1);
      if (nxt.lo == cur.lo) {
#pragma unroll
        for (int k = 0; k < NV; ++k) n_lo[k] = y_lo[k];
      } else if (nxt.lo == cur.hi) {
#pragma unroll
        for (int k = 0; k < NV; ++k) n_lo[k] = y_hi[k];
      } else {
        const int64_t o = level_offset(nxt.lo);
#pragma unroll
        for (int k = 0; k < NV; ++k) n_lo[k] = col[k][o];
      }
      if (nxt.hi == cur.hi) {
#pragma unroll
        for (int k = 0; k < NV; ++k) n_hi[k] = y_hi[k];
      } else if (nxt.hi == cur.lo) {
#pragma unroll
        for (int k = 0; k < NV; ++k) n_hi[k] = y_lo[k];
      } else {
        const int64_t o = level_offset(nxt.hi);
#pragma unroll
        for (int k = 0; k < NV; ++k) n_hi[k] = col[k][o];
      }
    } else {
#pragma unroll
      for (int k = 0; k < NV; ++k) { n_lo[k] = y_lo[k]; n_hi[k] = y_hi[k]; }
    }
    const int64_t o_out = (int64_t)s_perm[i] * thw;
#pragma unroll
    for (int k = 0; k < NV; ++k) out[k][o_out] = y_lo[k] + cur.w * (y_hi[k] - y_lo[k]);
#pragma unroll
    for (int k = 0; k < NV; ++k) { y_lo[k] = n_lo[k]; y_hi[k] = n_hi[k]; }
    cur = nxt;
  }
}

class Hybrid {
 public:
  Hybrid(int H, int W, int n_src, const float* a_src, const float* b_src, int n_dst, const float* a_dst, const float* b_dst, int dev)
      : hw((int64_t)H * W), Ls(n_src), Ld(n_dst), device(dev), mem(dev) {
    const HybridPlan p = hybrid_plan(Ls, a_src, b_src, Ld, a_dst, b_dst);
    flip = p.flip;
    WX_HIP(hipSetDevice(device));
    coef = mem.upload(p.coef.data(), p.coef.size());
    perm = mem.upload(p.perm.data(), p.perm.size());
  }
  void apply(int n_vars, const float* const* src, const int64_t* bstride, float* const* dst, int batch, int n_time, const float* sp,
             int64_t sp_bs, hipStream_t stream) {
    if (n_vars < 1 || n_vars > kHybridMaxVars) throw std::runtime_error("wx_hybrid_apply: 1.." + std::to_string(kHybridMaxVars) + " variables");
    if (batch < 1 || n_time < 1) throw std::runtime_error("wx_hybrid_apply: batch and n_time must be >= 1");
    if ((int64_t)batch * n_time * hw > 2147483647LL) throw std::runtime_error("wx_hybrid_apply: batch * n_time * H * W exceeds 2^31 - 1 columns");
    if (batch > 1 && sp_bs < 0) throw std::runtime_error("wx_hybrid_apply: negative batch stride");
    for (int i = 0; i < n_vars; ++i) {
      if (!src[i] || !dst[i]) throw std::runtime_error("wx_hybrid_apply: null tensor pointer");
      if (batch > 1 && bstride[i] < 0) throw std::runtime_error("wx_hybrid_apply: negative batch stride");
    }
    WX_HIP(hipSetDevice(device));
    HybridGeom g;
    g.Ls = Ls; g.Ld = Ld; g.flip = flip ? 1 : 0;
    g.thw = hw * n_time; g.ncol = g.thw * batch;
    g.coef = coef; g.perm = perm;
    const dim3 grid((unsigned)((g.ncol + 255) / 256)), block(256);
    for (int v0 = 0; v0 < n_vars; v0 += kHybridGroup) {
      const int nv = std::min(kHybridGroup, n_vars - v0);
      HybridVars hv;
      std::memset(&hv, 0, sizeof(hv));
      for (int k = 0; k < nv; ++k) { hv.src[k] = src[v0 + k]; hv.dst[k] = dst[v0 + k]; hv.bstride[k] = batch > 1 ? bstride[v0 + k] : 0; }
      switch (nv) {
        case 1: hipLaunchKernelGGL(hybrid_interp_kernel<1>, grid, block, 0, stream, hv, g, sp, sp_bs); break;
        case 2: hipLaunchKernelGGL(hybrid_interp_kernel<2>, grid, block, 0, stream, hv, g, sp, sp_bs); break;
        case 3: hipLaunchKernelGGL(hybrid_interp_kernel<3>, grid, block, 0, stream, hv, g, sp, sp_bs); break;
        case 4: hipLaunchKernelGGL(hybrid_interp_kernel<4>, grid, block, 0, stream, hv, g, sp, sp_bs); break;
        case 5: hipLaunchKernelGGL(hybrid_interp_kernel<5>, grid, block, 0, stream, hv, g, sp, sp_bs); break;
        case 6: hipLaunchKernelGGL(hybrid_interp_kernel<6>, grid, block, 0, stream, hv, g, sp, sp_bs); break;
        case 7: hipLaunchKernelGGL(hybrid_interp_kernel<7>, grid, block, 0, stream, hv, g, sp, sp_bs); break;
        default: hipLaunchKernelGGL(hybrid_interp_kernel<8>, grid, block, 0, stream, hv, g, sp, sp_bs); break;
      }
    }
    WX_HIP(hipGetLastError());
  }
  int source_levels() const { return Ls; }
  int dest_levels() const { return Ld; }

 private:
  int64_t hw;
  int Ls, Ld, device;
  bool flip = false;
  DeviceArena mem;
  float* coef = nullptr;
  int* perm = nullptr;
};

}  // namespace wx
