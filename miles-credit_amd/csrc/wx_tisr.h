// Top-of-atmosphere incident solar radiation (TISR) on the device: the one dynamic forcing of the gen-2 models that is pure astronomy,
//   credit/datasets/gen_2/tisr.py::_compute_tisr   a GraphCast / IFS orbital model, the CMIP6 TSI table, cos(zenith) floored at 0 at
//                                                  every grid point and sub-step, a trapezoid over the n_steps + 1 sub-steps of the
//                                                  window (t - period, t]
// The reference materialises [n_steps + 1, ny, nx] float32 tensors per plane.  Here a plane costs ny * nx * (n_steps + 1) terms of two
// multiplies, two FMAs, one max, one conversion and one fp64 add, with no per-term transcendental and next to no memory traffic:
//   cos z = cos(phi) cos(delta) cos(A + lambda) + sin(phi) sin(delta) = P a - Q b + S c
// with per point      a = cos(phi) cos(lambda), b = cos(phi) sin(lambda), c = sin(phi)            (tisr_point_terms, once at creation)
// and per sub-step k  P = cos(delta) cos A, Q = cos(delta) sin A, S = sin(delta), A = deg2rad(360 solar_time),
//                     C = w_k dt tsi / dist^2 (w = 1/2 at both ends, 1 inside; dt the step in seconds)     (tisr_table_kernel)
//   tisr = sum_k C_k max(cos z_k, 0)                                                                       (tisr_integrate_kernel)
// Table kernel: one thread per (target time, sub-step).  The target times arrive by value in the kernel arguments (TisrTimes, up to
// kTisrMaxTimes = 64 per launch): no H2D copy.  The sub-steps are pandas' date_range(end = t, periods = n_steps + 1, freq = period /
// n_steps): the step is the period's nanoseconds divided by n_steps and TRUNCATED, counted back from t; dt is that step.  The
// reference's float32 quantisation of time is reproduced, because it is systematic (an ulp of the days since J2000 is 42 s until June
// 2022 and 84 s after it: 361 sub-steps of one hour fall onto 86 distinct instants):
//   days        fp64 from the integer ns, ns / 86400e9 + 2440587.5 - 2451545.0, rounded to float32   (_get_j2000_days)
//   TSI         year, day of year and leap year by integer arithmetic (tisr_civil); the fractional year in fp64, rounded to float32;
//               searchsorted / clamp(1, n - 1) / linear interpolation with every operation rounded in float32   (_get_tsi)
// Both are widened to fp64 again and the orbital model, the solar time and the hour-angle offset are evaluated in fp64 with the
// reference's constants.  rotational_phase = days % 1.0 is torch's FLOORED modulo (j - floor(j)): before 2000 the days are negative
// and the phase still lies in [0, 1).  The four coefficients are rounded to float32 once.
// Integration kernel: 256 threads, kTisrPoints = 2 points per thread (p and p + 256: coalesced), a, b, c in registers for the up to
// kTisrTimesPerBlock = 4 target times of the workgroup (blockIdx.y).  The table row of a target time is wave-uniform: it goes through
// LDS in chunks of kTisrChunk = 256 entries (4 KB whatever n_steps is), read back as one broadcast 16-byte word per term.  The sum of a
// point is kept in fp64 and rounded to float32 at the store: a sequential float32 sum of 2 161 terms would alone exceed the error of
// the reference.  A (point, time) result does not depend on the times it shares a call or a workgroup with.
// The destination plane of target time i is dst + i * plane_stride: a channel slot of a wider forcing tensor, or a plane of a batch.
// Nothing outside the ny * nx values of a plane is written.
// Ranges: ny * nx <= 2^31 - 1; n_steps <= kTisrTableEntries - 1; offsets are 64-bit.  The table buffer grows with n_steps (never
// above 64 MB: a longer table takes fewer target times per launch pair) and is reused by the launch pairs of a call, which are
// ordered by the stream; calls on one handle must come on one stream at a time.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "wx_common.h"

namespace wx {

constexpr int kTisrChunk = 256;
constexpr int kTisrPoints = 2;
constexpr int kTisrMaxTimes = 64;
constexpr int kTisrTimesPerBlock = 4;
constexpr int64_t kTisrTableEntries = 1LL << 22;        // float4 entries of the table buffer: 64 MB
constexpr int64_t kTisrLimit = 2147483647LL;
constexpr int64_t kTisrNsPerDay = 86400000000000LL;

struct TisrTimes {
  int64_t t_end[kTisrMaxTimes];   // Unix ns of the target times of one launch
};

struct TisrDate {
  int64_t year;
  int doy;              // 1 .. 366
  int leap;
  int64_t ns_of_day;
};

// Proleptic Gregorian calendar of a Unix time in ns, by integer arithmetic (days-to-civil after H. Hinnant).
__host__ __device__ inline TisrDate tisr_civil(int64_t ns) {
  int64_t days = ns / kTisrNsPerDay;
  if (days * kTisrNsPerDay > ns) --days;                 // floor
  const int64_t z = days + 719468;
  const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
  const int64_t doe = z - era * 146097;                                              // [0, 146096]
  const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;        // [0, 399]
  const int64_t doy_mar = doe - (365 * yoe + yoe / 4 - yoe / 100);                   // day of the year that starts on 1 March
  const int64_t mp = (5 * doy_mar + 2) / 153;
  const int64_t month = mp < 10 ? mp + 3 : mp - 9;
  TisrDate d;
  d.year = yoe + era * 400 + (month <= 2 ? 1 : 0);
  d.leap = (d.year % 4 == 0 && (d.year % 100 != 0 || d.year % 400 == 0)) ? 1 : 0;
  d.doy = (int)(month <= 2 ? doy_mar - 306 : doy_mar + 59 + d.leap) + 1;
  d.ns_of_day = ns - days * kTisrNsPerDay;
  return d;
}

// ---- host-only helpers (no HIP call) ---------------------------------------------------------------------------------------------
// "" or the reason wx_tisr_create refuses.  Nothing is read before the test that makes reading it safe.
inline std::string tisr_check_create(int ny, int nx, const float* lat, const float* lon, int n_tsi, const float* tsi_times,
                                     const float* tsi_values) {
  if (!lat || !lon || !tsi_times || !tsi_values) return "null argument";
  if (ny < 1 || nx < 1 || (int64_t)ny * nx > kTisrLimit) return "ny and nx must be >= 1 and ny * nx <= 2^31 - 1, got " + std::to_string(ny) + " x " + std::to_string(nx);
  if (n_tsi < 2) return "the TSI table needs at least two entries, got " + std::to_string(n_tsi);
  for (int i = 0; i < n_tsi; ++i)
    if (!std::isfinite(tsi_times[i]) || !std::isfinite(tsi_values[i]) || std::fabs(tsi_times[i]) > 1.0e6f)
      return "the TSI table must be finite with |time| <= 1e6 years, entry " + std::to_string(i) + " is not";
  for (int i = 1; i < n_tsi; ++i)
    if (!(tsi_times[i] > tsi_times[i - 1])) return "the TSI times must ascend, entry " + std::to_string(i) + " does not";
  for (int64_t p = 0; p < (int64_t)ny * nx; ++p)
    if (!std::isfinite(lat[p]) || !std::isfinite(lon[p])) return "latitude and longitude must be finite, point " + std::to_string(p) + " is not";
  return "";
}

// "" or the reason wx_tisr_compute refuses, decided on the host before any launch.  year_lo .. year_hi: int(tsi_times[0]) ..
// int(tsi_times[-1]), the years _get_tsi accepts.
inline std::string tisr_check_compute(int n_times, const int64_t* t_end_ns, int64_t period_ns, int n_steps, const void* dst,
                                      int64_t plane_stride, int64_t npts, int64_t year_lo, int64_t year_hi) {
  if (!t_end_ns || !dst) return "null argument";
  if (n_times < 1) return "n_times must be >= 1, got " + std::to_string(n_times);
  if (n_steps < 1 || n_steps > kTisrTableEntries - 1) return "n_steps must be 1 .. 2^22 - 1, got " + std::to_string(n_steps);
  if (period_ns < 1) return "period_ns must be >= 1, got " + std::to_string(period_ns);
  if (period_ns < n_steps) return "a period of " + std::to_string(period_ns) + " ns holds no " + std::to_string(n_steps) + " steps of a whole nanosecond";
  if (plane_stride < npts) return "plane_stride must be >= ny * nx = " + std::to_string(npts) + ", got " + std::to_string(plane_stride);
  const int64_t span = (period_ns / n_steps) * n_steps;
  for (int i = 0; i < n_times; ++i) {
    int64_t first = 0;
    if (__builtin_sub_overflow(t_end_ns[i], span, &first)) return "the window of target time " + std::to_string(i) + " leaves the int64 nanosecond range";
    const int64_t y0 = tisr_civil(first).year, y1 = tisr_civil(t_end_ns[i]).year;
    if (y0 < year_lo || y1 > year_hi)
      return "a sub-step of target time " + std::to_string(i) + " lies in the year " + std::to_string(y0 < year_lo ? y0 : y1) +
             ", outside the TSI table's years " + std::to_string(year_lo) + " .. " + std::to_string(year_hi);
  }
  return "";
}

// a, b, c of every point: fp64 from the float32 degrees, stored as float32.
inline void tisr_point_terms(int64_t npts, const float* lat, const float* lon, std::vector<float>& a, std::vector<float>& b,
                             std::vector<float>& c) {
  a.resize(npts); b.resize(npts); c.resize(npts);
  const double rad = 3.14159265358979323846 / 180.0;
  for (int64_t p = 0; p < npts; ++p) {
    const double phi = (double)lat[p] * rad, lam = (double)lon[p] * rad;
    a[p] = (float)(std::cos(phi) * std::cos(lam));
    b[p] = (float)(std::cos(phi) * std::sin(lam));
    c[p] = (float)std::sin(phi);
  }
}

// ---- one sub-step, on the host as on the device ------------------------------------------------------------------------------------
// _get_tsi on the float32 table: every operation rounded in float32, nothing contracted.
__host__ __device__ inline float tisr_tsi(float fy, const float* __restrict__ tt, const float* __restrict__ tv, int n) {
#pragma clang fp contract(off)
  int lo = 0, hi = n;                               // searchsorted, left: the first index whose time is >= fy
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tt[mid] < fy) lo = mid + 1; else hi = mid;
  }
  const int i1 = lo < 1 ? 1 : (lo > n - 1 ? n - 1 : lo), i0 = i1 - 1;
  const float t = (fy - tt[i0]) / (tt[i1] - tt[i0]);
  const float slope = tv[i1] - tv[i0];
  const float rise = t * slope;
  return tv[i0] + rise;
}

// The float32 days since J2000 of a Unix time in ns (_get_j2000_days).
__host__ __device__ inline float tisr_days32(int64_t ns) { return (float)((double)ns / 86400e9 + 2440587.5 - 2451545.0); }

// Entry k of a target time's table: (C, P, Q, S) of the sub-step at `ns`; w: the trapezoid weight, dt: the step in seconds.
__host__ __device__ inline float4 tisr_entry(int64_t ns, double w, double dt, const float* __restrict__ tsi_t,
                                             const float* __restrict__ tsi_v, int n_tsi) {
  const TisrDate d = tisr_civil(ns);
  const double day_frac = (double)d.ns_of_day / (double)kTisrNsPerDay;
  const double year_frac = ((double)(d.doy - 1) + day_frac) / (double)(365 + d.leap);
  const float fy32 = (float)((double)d.year + year_frac);
  const double tsi = (double)tisr_tsi(fy32, tsi_t, tsi_v, n_tsi);

  const double j = (double)tisr_days32(ns);
  const double theta = j / 365.25;
  const double phase = j - floor(j);
  const double rel = 1.7535 + 6.283076 * theta;
  const double rem = 6.240041 + 6.283020 * theta;
  const double rlls = 4.8951 + 6.283076 * theta;
  const double sin_rel = sin(rel), cos_rel = cos(rel), sin_rem = sin(rem);
  const double rllls = 4.8952 + 6.283320 * theta - 0.0075 * sin_rel - 0.0326 * cos_rel - 0.0003 * sin(2.0 * rel) + 0.0002 * cos(2.0 * rel);
  const double sin_dec = sin(0.409093) * sin(rllls);
  const double cos_dec = sqrt(1.0 - sin_dec * sin_dec);
  const double eot = 591.8 * sin(2.0 * rlls) - 459.4 * sin_rem + 39.5 * sin_rem * cos(2.0 * rlls) - 12.7 * sin(4.0 * rlls) - 4.8 * sin(2.0 * rem);
  const double dist = 1.0001 - 0.0163 * sin_rel + 0.0037 * cos_rel;
  const double solar_time = phase + eot / 86400.0;
  const double A = (360.0 * solar_time) * (3.14159265358979323846 / 180.0);
  return make_float4((float)(w * dt * tsi / (dist * dist)), (float)(cos_dec * cos(A)), (float)(cos_dec * sin(A)), (float)sin_dec);
}

// One term of a point's sum: C max(P a - Q b + S c, 0) in float32.
__host__ __device__ inline float tisr_term(const float4 e, float a, float b, float c) {
  const float cz = fmaf(e.y, a, fmaf(-e.z, b, e.w * c));
  return e.x * fmaxf(cz, 0.f);
}

// ---- device side -------------------------------------------------------------------------------------------------------------------
// grid = ceil(nt * (n_steps + 1) / 256): entry k of target time i at table[i * (n_steps + 1) + k] = (C, P, Q, S)
__global__ __launch_bounds__(256) void tisr_table_kernel(const TisrTimes times, int nt, int64_t step_ns, int n_steps,
                                                         const float* __restrict__ tsi_t, const float* __restrict__ tsi_v, int n_tsi,
                                                         float4* __restrict__ table) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n_entries = (int64_t)n_steps + 1;
  if (idx >= (int64_t)nt * n_entries) return;
  const int i = (int)(idx / n_entries);
  const int k = (int)(idx - (int64_t)i * n_entries);
  const int64_t ns = times.t_end[i] - (int64_t)(n_steps - k) * step_ns;
  table[idx] = tisr_entry(ns, (k == 0 || k == n_steps) ? 0.5 : 1.0, (double)step_ns / 1e9, tsi_t, tsi_v, n_tsi);
}

// grid = (ceil(npts / (256 * kTisrPoints)), ceil(nt / kTisrTimesPerBlock)); no thread leaves before the last barrier
__global__ __launch_bounds__(256) void tisr_integrate_kernel(const float* __restrict__ pa, const float* __restrict__ pb,
                                                             const float* __restrict__ pc, int64_t npts,
                                                             const float4* __restrict__ table, int n_entries, int nt,
                                                             float* __restrict__ dst, int64_t plane_stride) {
  __shared__ float4 tab[kTisrChunk];
  const int tid = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * (256 * kTisrPoints) + tid;
  float a[kTisrPoints], b[kTisrPoints], c[kTisrPoints];
#pragma unroll
  for (int q = 0; q < kTisrPoints; ++q) {
    const int64_t p = p0 + (int64_t)q * 256;
    const bool live = p < npts;
    a[q] = live ? pa[p] : 0.f;
    b[q] = live ? pb[p] : 0.f;
    c[q] = live ? pc[p] : 0.f;
  }
  const int t_first = (int)blockIdx.y * kTisrTimesPerBlock;
  const int t_last = min(nt, t_first + kTisrTimesPerBlock);
  for (int t = t_first; t < t_last; ++t) {            // block-uniform bounds
    const float4* __restrict__ row = table + (int64_t)t * n_entries;
    double acc[kTisrPoints];
#pragma unroll
    for (int q = 0; q < kTisrPoints; ++q) acc[q] = 0.0;
    for (int k0 = 0; k0 < n_entries; k0 += kTisrChunk) {
      const int m = min(kTisrChunk, n_entries - k0);
      __syncthreads();                                 // the previous chunk has been read by every wave
      if (tid < m) tab[tid] = row[k0 + tid];
      __syncthreads();
#pragma unroll 4
      for (int k = 0; k < m; ++k) {
        const float4 e = tab[k];                       // (C, P, Q, S): one address per wave, an LDS broadcast
#pragma unroll
        for (int q = 0; q < kTisrPoints; ++q) {
          acc[q] += (double)tisr_term(e, a[q], b[q], c[q]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < kTisrPoints; ++q) {
      const int64_t p = p0 + (int64_t)q * 256;
      if (p < npts) dst[(int64_t)t * plane_stride + p] = (float)acc[q];
    }
  }
}

class Tisr {
 public:
  Tisr(int ny_, int nx_, const float* lat, const float* lon, int n_tsi_, const float* tsi_times, const float* tsi_values, int dev)
      : npts((int64_t)ny_ * nx_), n_tsi(n_tsi_), device(dev), mem(dev) {
    year_lo = (int64_t)tsi_times[0];                  // int(t_min), int(t_max) of _get_tsi: truncated
    year_hi = (int64_t)tsi_times[n_tsi - 1];
    std::vector<float> a, b, c;
    tisr_point_terms(npts, lat, lon, a, b, c);
    WX_HIP(hipSetDevice(device));
    pa = mem.upload(a.data(), a.size()); pb = mem.upload(b.data(), b.size()); pc = mem.upload(c.data(), c.size());
    tsi_t = mem.upload(tsi_times, (size_t)n_tsi); tsi_v = mem.upload(tsi_values, (size_t)n_tsi);
  }
  void compute(int n_times, const int64_t* t_end_ns, int64_t period_ns, int n_steps, float* dst, int64_t plane_stride, hipStream_t stream) {
    const std::string why = tisr_check_compute(n_times, t_end_ns, period_ns, n_steps, dst, plane_stride, npts, year_lo, year_hi);
    if (!why.empty()) throw std::runtime_error("wx_tisr_compute: " + why);
    const int64_t n_entries = (int64_t)n_steps + 1;
    const int per_launch = (int)std::max<int64_t>(1, std::min<int64_t>(kTisrMaxTimes, kTisrTableEntries / n_entries));
    WX_HIP(hipSetDevice(device));
    mem.grow(table, table_have, (size_t)(std::min<int64_t>(per_launch, n_times) * n_entries));
    const int64_t step_ns = period_ns / n_steps;
    for (int t0 = 0; t0 < n_times; t0 += per_launch) {
      const int nt = std::min(per_launch, n_times - t0);
      TisrTimes tt;
      std::memset(&tt, 0, sizeof(tt));
      for (int i = 0; i < nt; ++i) tt.t_end[i] = t_end_ns[t0 + i];
      const int64_t total = (int64_t)nt * n_entries;
      hipLaunchKernelGGL(tisr_table_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, tt, nt, step_ns, n_steps, tsi_t, tsi_v,
                         n_tsi, table);
      hipLaunchKernelGGL(tisr_integrate_kernel,
                         dim3((unsigned)((npts + 256 * kTisrPoints - 1) / (256 * kTisrPoints)), (unsigned)((nt + kTisrTimesPerBlock - 1) / kTisrTimesPerBlock)),
                         dim3(256), 0, stream, pa, pb, pc, npts, table, (int)n_entries, nt, dst + (int64_t)t0 * plane_stride, plane_stride);
    }
    WX_HIP(hipGetLastError());
  }

 private:
  int64_t npts, year_lo = 0, year_hi = 0;
  int n_tsi, device;
  DeviceArena mem;
  float* pa = nullptr;
  float* pb = nullptr;
  float* pc = nullptr;
  float* tsi_t = nullptr;
  float* tsi_v = nullptr;
  float4* table = nullptr;
  size_t table_have = 0;
};

}  // namespace wx
