// Ensemble verification on the device: CRPS (biased, fair, almost fair), spread and ensemble-mean error of M members against the
// truth from ONE reading pass:
//   credit/losses/gen_1/kcrps.py:64-81            skill - spread, spread = sum_i (2i - M - 1) x_(i) / denom over the sorted members
//   credit/losses/gen_1/almost_fair_crps.py:48-76 skill - (1 - (1 - alpha) / M) sum_{i != j} |x_i - x_j| / (2 M (M - 1))
//   credit/metrics/gen_1/metrics.py:304-313       ens_std (torch.std, ddof 1), ens_mean, ens_rmse = |ens_mean - y| as maps
//   credit/applications/rollout_metrics_noisy_model.py:107-135  sqrt(plane mean of (ens_mean - y)^2), sqrt(plane mean of the members'
//                                                 squared deviations from the ensemble mean)
// All of them are functions of the same per-grid-point quantities, and every member value is needed exactly once, so (M + 1) * 4
// bytes per grid point is all that has to move.
//
// Per grid point.  Work is done on d_i = x_i - y: CRPS, spread and variance are translation invariant and the float32 subtraction
// of nearby values is (nearly) exact, which keeps a 1e5 Pa surface pressure accurate where the reference, which sorts and sums the
// members themselves in float32, loses digits.  With mean_d = sum d_i / M and e_(i) = d_(i) - mean_d over the SORTED d:
//   skill = sum |d_i|     pair = sum_{i<j} |d_i - d_j| = sum_i (2i - M - 1) e_(i)     ss = sum e_i^2     err = mean_d
// (pair is translation invariant too: the centred e keep its terms small when the bias is larger than the spread; ss is centred and
// never formed from raw moments).  The members of a point sit in registers, the kernel is instantiated for the padded member count
// MP = 4, 8, 16, 32, 64, and the sort is a fully unrolled bitonic network: every index is a compile-time constant, so nothing goes
// to scratch.  Ranks M .. MP - 1 hold +INF; they are masked with a select, never with a multiply (INF * 0 is NaN).  The per-point
// sums are float32 for MP <= 16 and float64 for MP = 32 and 64, where a 64-term float32 sum would cost a digit and the sort, not
// HBM, sets the time anyway.  Points per thread and iteration: 4 (16-byte loads) for MP <= 16, 2 (8-byte) for MP = 32, 1 for MP = 64
// and on the scalar path, so that the member registers stay at or below 64 and several waves per SIMD hide the HBM latency.
//
// Per plane (variable, b, level, t) six sums over H x W, weighted by w[h] with latitude weights (not divided by the sum of w, the
// convention of wx_metrics.h):  w skill, w pair, w err^2, w |err|, w ss, w sqrt(ss / (M - 1)), float64, as planes[n_planes][6].
// Optional maps [B][L][T][H][W] float32 from the same pass: ens_mean = y + mean_d, ens_std = sqrt(ss / (M - 1)), ens_abs_err = |err|,
// crps = skill / M - pair / M^2, fair_crps = skill / M - pair / (M (M - 1)), afcrps = skill / M - (1 - (1 - alpha) / M) pair / (M (M - 1)).
//
// Reproducibility.  Every sum is made in the fixed order of wx_reduce.h.  A workgroup owns one tile (variable, plane, block of rows)
// and writes its six sums to its own slot of the handle's slab; the finish launch -- one wave per plane -- adds the plane's slots.
// A plane's tiles depend on the grid alone, so repeated calls and any grouping of variables into calls give identical bits, with
// maps or without -- as long as the variable takes the same load path: the vector path gives a thread 4 (or 2) neighbouring points,
// the scalar path one, so the order of the in-tile sums differs between them, and a layout or slice that changes the 16-byte
// alignment of a variable changes the last bits of its sums (not its maps).  Two launches per call.
//
// Layout.  Variable v, member m, batch item b at member[v * M + m] + b * member_bs[v], [L][T][H][W] contiguous, read in place (the
// per-member buffers of ensemble_rollout, or the reference's [B * M, ...] tensor with pointer x[m] and batch stride M * stride(0)).
// The pointers (M members and six maps per variable) go through a device table owned by the handle: it grows and never shrinks and
// is uploaded on the call's stream from a ring of kEnsRing pinned host slots.  Before a slot is filled again the host waits for
// the upload that last read it, the one enqueued kEnsRing calls earlier: a call does not wait for the kernels before it, but the
// fifth and later of many submits into a deep queue block until that earlier upload has run.  Maps must not overlap an input, the
// plane table or each other: such a call is refused.
// One handle serves one stream at a time.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "wx_common.h"
#include "wx_reduce.h"

namespace wx {

constexpr int kEnsMaxMembers = 64;
constexpr int kEnsMaxVars = 32;
constexpr int kEnsSums = 6;               // w skill, w pair, w err^2, w |err|, w ss, w sqrt(ss / (M - 1))
constexpr int kEnsMaps = 6;               // ens_mean, ens_std, ens_abs_err, crps, fair_crps, afcrps
constexpr int kEnsRing = 4;               // pinned host slots of the pointer table

struct EnsVar {
  const float* target;     // batch item b at target + b * target_bs: [L][T][H][W]
  int64_t target_bs, member_bs;   // in floats
  int L, T;
  int tile0, plane0;       // this variable's tiles start at tile0 ((plane, row block), row block fastest), its planes at plane0
  int nplanes, vec;        // vec: every plane base of members, truth and maps on 16 bytes and W % 4 == 0
};

struct EnsArgs {
  EnsVar v[kEnsMaxVars];
  const float* w;          // device [H], or null
  int n_vars, M;
  RowTiles g;
  float alpha;
};

// ---- host-only helpers (no HIP call) ---------------------------------------------------------------------------------------------
// "" or the reason wx_ensemble_create refuses
inline std::string ensemble_check_create(int H, int W, const float* lat_w, int n_members) {
  if (n_members < 2 || n_members > kEnsMaxMembers) return "2.." + std::to_string(kEnsMaxMembers) + " members";
  return grid_check(H, W, lat_w);
}
inline int ensemble_padded_members(int M) { return M <= 4 ? 4 : M <= 8 ? 8 : M <= 16 ? 16 : M <= 32 ? 32 : 64; }

// ---- device side -------------------------------------------------------------------------------------------------------------------
template <int N>
struct EnsVecT { using type = float; };
template <>
struct EnsVecT<2> { using type = float2; };
template <>
struct EnsVecT<4> { using type = float4; };

template <int N>
__device__ __forceinline__ void ens_load(const float* p, float (&out)[N]) {
  const typename EnsVecT<N>::type v = *reinterpret_cast<const typename EnsVecT<N>::type*>(p);
  if constexpr (N == 1) { out[0] = v; }
  else if constexpr (N == 2) { out[0] = v.x; out[1] = v.y; }
  else { out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w; }
}
template <int N>
__device__ __forceinline__ void ens_store(float* p, const float (&in)[N]) {
  if constexpr (N == 1) { *p = in[0]; }
  else if constexpr (N == 2) { *reinterpret_cast<float2*>(p) = make_float2(in[0], in[1]); }
  else { *reinterpret_cast<float4*>(p) = make_float4(in[0], in[1], in[2], in[3]); }
}

// ascending bitonic network on MP registers: all indices and directions are compile-time constants once the loops are unrolled
template <int MP>
__device__ __forceinline__ void ens_sort(float (&d)[MP]) {
#pragma unroll
  for (int lk = 1; (1 << lk) <= MP; ++lk) {
#pragma unroll
    for (int lj = lk - 1; lj >= 0; --lj) {
#pragma unroll
      for (int i = 0; i < MP; ++i) {
        const int l = i ^ (1 << lj);
        if (l > i) {
          const float lo = fminf(d[i], d[l]), hi = fmaxf(d[i], d[l]);
          const bool up = (i & (1 << lk)) == 0;
          d[i] = up ? lo : hi;
          d[l] = up ? hi : lo;
        }
      }
    }
  }
}

// one tile: n = rows * W contiguous points at `off` floats from every member / truth / map base.  NP points per thread and iteration.
template <int MP, int NP>
__device__ __forceinline__ void ens_tile(const float* const* __restrict__ members, float* const* __restrict__ maps, bool any_map,
                                         const float* __restrict__ truth, int64_t member_off, int64_t map_off, int n, int M, int W,
                                         float alpha, const float* s_w, double* acc) {
  using Acc = typename std::conditional<(MP >= 32), double, float>::type;
  const Acc Mf = (Acc)M;
  const Acc inv_m = (Acc)1 / Mf, inv_m2 = (Acc)1 / (Mf * Mf), inv_mm1 = (Acc)1 / (Mf * (Mf - (Acc)1)), inv_dof = (Acc)1 / (Mf - (Acc)1);
  const Acc af = ((Acc)1 - ((Acc)1 - (Acc)alpha) / Mf) * inv_mm1;
  const float inf = __builtin_inff();
  for (int i = threadIdx.x; i < n / NP; i += kTileThreads) {
    const int p0 = i * NP;
    float y[NP];
    ens_load<NP>(truth + p0, y);
    float d[NP][MP];
    Acc skill[NP], sum[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) skill[q] = sum[q] = (Acc)0;
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      if (m < M) {                                    // uniform
        float x[NP];
        ens_load<NP>(members[m] + member_off + p0, x);
#pragma unroll
        for (int q = 0; q < NP; ++q) {
          const float v = x[q] - y[q];
          d[q][m] = v;
          skill[q] += (Acc)fabsf(v);
          sum[q] += (Acc)v;
        }
      } else {
#pragma unroll
        for (int q = 0; q < NP; ++q) d[q][m] = inf;
      }
    }
    const double w = (double)s_w[(unsigned)p0 / (unsigned)W];          // NP > 1 only with W % 4 == 0: the points lie in one row
    Acc pair[NP], mean[NP], ss[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      ens_sort<MP>(d[q]);
      mean[q] = sum[q] / Mf;
      // sum_r (2 r + 1 - M) e_r = 2 sum_r r e_r + (1 - M) sum_r e_r with r = 0 .. M - 1: the rank is a literal of the unrolled code,
      // not one loop-invariant register per rank
      Acc re = (Acc)0, se = (Acc)0, s2 = (Acc)0;
#pragma unroll
      for (int r = 0; r < MP; ++r) {
        const Acc e = r < M ? (Acc)d[q][r] - mean[q] : (Acc)0;          // a select: the padded ranks hold +INF
        re = fma((Acc)r, e, re);
        se += e;
        s2 = fma(e, e, s2);
      }
      pair[q] = fma((Acc)1 - Mf, se, (Acc)2 * re);
      ss[q] = s2;
      acc[0] = fma(w, (double)skill[q], acc[0]);
      acc[1] = fma(w, (double)pair[q], acc[1]);
      acc[2] = fma(w * (double)mean[q], (double)mean[q], acc[2]);
      acc[3] = fma(w, (double)fabs(mean[q]), acc[3]);
      acc[4] = fma(w, (double)s2, acc[4]);
      acc[5] = fma(w, (double)sqrt(s2 * inv_dof), acc[5]);
    }
    if (any_map) {                                    // uniform
      float o[kEnsMaps][NP];
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        const Acc sk = skill[q] * inv_m;
        o[0][q] = (float)((Acc)y[q] + mean[q]);
        o[1][q] = (float)sqrt(ss[q] * inv_dof);
        o[2][q] = (float)fabs(mean[q]);
        o[3][q] = (float)(sk - pair[q] * inv_m2);
        o[4][q] = (float)(sk - pair[q] * inv_mm1);
        o[5][q] = (float)(sk - pair[q] * af);
      }
#pragma unroll
      for (int k = 0; k < kEnsMaps; ++k)
        if (maps[k]) ens_store<NP>(maps[k] + map_off + p0, o[k]);
    }
  }
}

// grid = total tiles.  table: per variable M member pointers, then kEnsMaps map pointers (null: not wanted).
template <int MP>
__global__ __launch_bounds__(kTileThreads) void ens_tile_kernel(const EnsArgs a, const float* const* __restrict__ table,
                                                                double* __restrict__ slab) {
  __shared__ float s_w[kTileRows];
  __shared__ double s_red[kTileThreads / 64][kEnsSums];
  const int tile = blockIdx.x;
  int vi = 0;
  while (vi + 1 < a.n_vars && tile >= a.v[vi + 1].tile0) ++vi;
  const EnsVar& v = a.v[vi];
  const RowTile rt = row_tile(tile - v.tile0, a.g);
  stage_row_weights(s_w, a.w, rt.h0, rt.rows);
  const int lt = v.L * v.T;
  const int b = rt.plane / lt, r = rt.plane - b * lt;  // r = l * T + t
  const int64_t hw = (int64_t)a.g.H * a.g.W;
  const float* const* members = table + (size_t)vi * (a.M + kEnsMaps);
  float* const* maps = const_cast<float* const*>(reinterpret_cast<const float* const*>(members + a.M));
  bool any_map = false;
#pragma unroll
  for (int k = 0; k < kEnsMaps; ++k) any_map = any_map || maps[k] != nullptr;
  const float* truth = v.target + b * v.target_bs + r * hw + rt.offset;
  const int64_t member_off = b * v.member_bs + r * hw + rt.offset;
  const int64_t map_off = (int64_t)rt.plane * hw + rt.offset;

  double acc[kEnsSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  constexpr int NPV = MP <= 16 ? 4 : MP == 32 ? 2 : 1;
  if (NPV > 1 && v.vec) ens_tile<MP, NPV>(members, maps, any_map, truth, member_off, map_off, rt.n, a.M, a.g.W, a.alpha, s_w, acc);
  else ens_tile<MP, 1>(members, maps, any_map, truth, member_off, map_off, rt.n, a.M, a.g.W, a.alpha, s_w, acc);
  const double s = block_sum_waves<kEnsSums, kTileThreads>(acc, s_red);
  if (threadIdx.x < kEnsSums) slab[(size_t)tile * kEnsSums + threadIdx.x] = s;
}

// grid = total planes, one wave each: the plane's row blocks added lane-strided, then over the wave
__global__ __launch_bounds__(64) void ens_finish_kernel(const EnsArgs a, const double* __restrict__ slab, double* __restrict__ planes) {
  const int plane = blockIdx.x;
  int vi = 0;
  while (vi + 1 < a.n_vars && plane >= a.v[vi + 1].plane0) ++vi;
  const EnsVar& v = a.v[vi];
  const size_t tile0 = (size_t)v.tile0 + (size_t)(plane - v.plane0) * a.g.row_blocks;
  double acc[kEnsSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  sum_slots<kEnsSums, 64>(slab + tile0 * kEnsSums, a.g.row_blocks, acc);
  wave_sum<kEnsSums>(acc);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kEnsSums; ++k) planes[(size_t)plane * kEnsSums + k] = acc[k];
  }
}

class Ensemble {
 public:
  Ensemble(int H, int W, const float* lat_w, int n_members, int dev) : g(row_tiles(H, W)), M(n_members), device(dev), mem(dev) {
    WX_HIP(hipSetDevice(device));
    if (lat_w) w = mem.upload(lat_w, (size_t)H);
    for (int i = 0; i < kEnsRing; ++i) WX_HIP(hipEventCreateWithFlags(&ring_done[i], hipEventDisableTiming));
  }
  Ensemble(const Ensemble&) = delete;
  Ensemble& operator=(const Ensemble&) = delete;
  ~Ensemble() {
    (void)hipSetDevice(device);
    for (int i = 0; i < kEnsRing; ++i) {
      if (ring_done[i]) {
        (void)hipEventSynchronize(ring_done[i]);
        (void)hipEventDestroy(ring_done[i]);
      }
    }
    if (ring) (void)hipHostFree(ring);
  }
  // members: [n_vars * M]; maps: [n_vars * kEnsMaps] (null entries: not wanted) or null; planes: device [sum B L_v T_v][kEnsSums]
  void apply(int n_vars, const float* const* members, const int64_t* member_bs, const float* const* target, const int64_t* target_bs,
             const int32_t* n_levels, const int32_t* n_time, int batch, double alpha, float* const* maps, double* planes,
             hipStream_t stream) {
    if (n_vars < 1 || n_vars > kEnsMaxVars) throw std::runtime_error("wx_ensemble_apply: 1.." + std::to_string(kEnsMaxVars) + " variables");
    if (batch < 1) throw std::runtime_error("wx_ensemble_apply: B >= 1");
    if (!std::isfinite(alpha)) throw std::runtime_error("wx_ensemble_apply: alpha must be finite");
    EnsArgs a;
    std::memset(&a, 0, sizeof(a));
    int64_t tiles = 0, nplanes = 0;
    const bool row_vec = g.W % 4 == 0;
    const int64_t hw = (int64_t)g.H * g.W;
    auto aligned = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    struct Range { uintptr_t lo, hi; };
    std::vector<Range> inputs, outputs;
    const size_t per_var = (size_t)M + kEnsMaps;
    std::vector<const float*> host((size_t)n_vars * per_var, nullptr);
    for (int i = 0; i < n_vars; ++i) {
      if (!target[i]) throw std::runtime_error("wx_ensemble_apply: null tensor pointer");
      if (n_levels[i] < 1 || n_time[i] < 1) throw std::runtime_error("wx_ensemble_apply: n_levels and n_time must be >= 1");
      if (batch > 1 && (member_bs[i] < 0 || target_bs[i] < 0)) throw std::runtime_error("wx_ensemble_apply: negative batch stride");
      EnsVar& v = a.v[i];
      v.target = target[i];
      v.target_bs = batch > 1 ? target_bs[i] : 0;
      v.member_bs = batch > 1 ? member_bs[i] : 0;
      v.L = n_levels[i];
      v.T = n_time[i];
      const int64_t item = (int64_t)v.L * v.T * hw;
      bool vec = row_vec && aligned(v.target) && v.target_bs % 4 == 0 && v.member_bs % 4 == 0;
      inputs.push_back({(uintptr_t)v.target, (uintptr_t)(v.target + (batch - 1) * v.target_bs + item)});
      for (int m = 0; m < M; ++m) {
        const float* p = members[(size_t)i * M + m];
        if (!p) throw std::runtime_error("wx_ensemble_apply: null member pointer (variable " + std::to_string(i) + ", member " + std::to_string(m) + ")");
        host[i * per_var + m] = p;
        vec = vec && aligned(p);
        inputs.push_back({(uintptr_t)p, (uintptr_t)(p + (batch - 1) * v.member_bs + item)});
      }
      for (int k = 0; k < kEnsMaps; ++k) {
        float* p = maps ? maps[(size_t)i * kEnsMaps + k] : nullptr;
        host[i * per_var + M + k] = p;
        if (!p) continue;
        vec = vec && aligned(p);
        outputs.push_back({(uintptr_t)p, (uintptr_t)(p + batch * item)});
      }
      v.vec = vec ? 1 : 0;
      const int64_t np = (int64_t)batch * v.L * v.T;
      if (tiles + np * g.row_blocks > 2147483647LL) throw std::runtime_error("wx_ensemble_apply: B * n_levels * n_time * row blocks exceeds 2^31 - 1 tiles");
      v.tile0 = (int)tiles;
      v.plane0 = (int)nplanes;
      v.nplanes = (int)np;
      tiles += np * g.row_blocks;
      nplanes += np;
    }
    for (size_t i = 0; i < outputs.size(); ++i) {
      const Range& o = outputs[i];
      for (size_t j = i + 1; j < outputs.size(); ++j)
        if (o.lo < outputs[j].hi && outputs[j].lo < o.hi) throw std::runtime_error("wx_ensemble_apply: two maps overlap");
      for (const Range& in : inputs)
        if (o.lo < in.hi && in.lo < o.hi) throw std::runtime_error("wx_ensemble_apply: a map overlaps an input");
      if (o.lo < (uintptr_t)(planes + nplanes * kEnsSums) && (uintptr_t)planes < o.hi)
        throw std::runtime_error("wx_ensemble_apply: a map overlaps the plane table");
    }
    a.w = w;
    a.n_vars = n_vars; a.M = M; a.g = g;
    a.alpha = (float)alpha;
    WX_HIP(hipSetDevice(device));
    mem.grow(slab, slab_doubles, (size_t)tiles * kEnsSums);
    if (host.size() > table_cap) {  // grows only, to the full 32 variables at once: at most one growth per handle
      for (int i = 0; i < kEnsRing; ++i) WX_HIP(hipEventSynchronize(ring_done[i]));
      table_cap = 0;
      mem.release(table);
      if (ring) { WX_HIP(hipHostFree(ring)); ring = nullptr; }
      const size_t cap = (size_t)kEnsMaxVars * per_var;
      table = (const float**)mem.alloc(sizeof(float*) * cap);
      WX_HIP(hipHostMalloc((void**)&ring, sizeof(float*) * cap * kEnsRing, hipHostMallocDefault));
      table_cap = cap;
    }
    const int slot = ring_next;
    ring_next = (ring_next + 1) % kEnsRing;
    WX_HIP(hipEventSynchronize(ring_done[slot]));      // the copy that last read this slot: kEnsRing calls ago
    const float** staged = ring + (size_t)slot * table_cap;
    std::memcpy(staged, host.data(), sizeof(float*) * host.size());
    WX_HIP(hipMemcpyAsync(table, staged, sizeof(float*) * host.size(), hipMemcpyHostToDevice, stream));
    WX_HIP(hipEventRecord(ring_done[slot], stream));
    const dim3 grid((unsigned)tiles), fin((unsigned)nplanes), block(kTileThreads);
    switch (ensemble_padded_members(M)) {
      case 4: hipLaunchKernelGGL(ens_tile_kernel<4>, grid, block, 0, stream, a, table, slab); break;
      case 8: hipLaunchKernelGGL(ens_tile_kernel<8>, grid, block, 0, stream, a, table, slab); break;
      case 16: hipLaunchKernelGGL(ens_tile_kernel<16>, grid, block, 0, stream, a, table, slab); break;
      case 32: hipLaunchKernelGGL(ens_tile_kernel<32>, grid, block, 0, stream, a, table, slab); break;
      default: hipLaunchKernelGGL(ens_tile_kernel<64>, grid, block, 0, stream, a, table, slab); break;
    }
    hipLaunchKernelGGL(ens_finish_kernel, fin, dim3(64), 0, stream, a, slab, planes);
    WX_HIP(hipGetLastError());
  }
  int members() const { return M; }

 private:
  RowTiles g;
  int M, device;
  DeviceArena mem;
  float* w = nullptr;
  double* slab = nullptr;
  size_t slab_doubles = 0;
  const float** table = nullptr;     // device
  const float** ring = nullptr;      // pinned host, kEnsRing slots of table_cap pointers
  size_t table_cap = 0;
  hipEvent_t ring_done[kEnsRing] = {};
  int ring_next = 0;
};

}  // namespace wx
