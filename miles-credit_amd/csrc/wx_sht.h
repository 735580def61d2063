// Spherical harmonic transforms on the device: the scalar pair, the vector analysis and the two verification spectra of
//   credit/verification/standard.py   zonal_spectrum, div_rot_spectrum (and their average_* means over the planes)
// which the reference computes with torch_harmonics (RealSHT / RealVectorSHT).  Pinned to the mathematics, not to that library: only
// norm = "ortho" is taken, and the vector results are named (spheroidal, toroidal), never a slot index.
//
// Unit sphere.  Row k has colatitude theta_k strictly ascending (north first), column j has phi_j = 2 pi j / nlon; w_k are the
// quadrature weights of int dx on [-1, 1] at cos(theta_k) (Gauss, or Clenshaw-Curtis on the equiangular grid: both sum to 2).
//   table      Pbar_l^m(theta), 0 <= m < mmax, m <= l < lmax, 2 pi int Pbar_l^m Pbar_l'^m sin(theta) dtheta = delta_ll' (Pbar_0^0 =
//              1 / sqrt(4 pi)), no Condon-Shortley sign; csphase multiplies odd m by -1.  Host, fp64: the three-term recurrence in l,
//              seeded along the diagonal.  dPt = (dPbar / dtheta) / sqrt(l (l + 1)) and Qt = (m Pbar / sin theta) / sqrt(l (l + 1))
//              come from the ladder identities (no division by sin theta: they hold at the poles), row l = 0 is zero:
//                dPbar_l^m / dtheta     = ( sqrt((l + m)(l - m + 1)) Pbar_l^{m-1} - sqrt((l - m)(l + m + 1)) Pbar_l^{m+1} ) / 2
//                m Pbar_l^m / sin theta = sqrt((2l + 1) / (2l - 1)) ( sqrt((l - m)(l - m - 1)) Pbar_{l-1}^{m+1} + sqrt((l + m)(l + m - 1)) Pbar_{l-1}^{m-1} ) / 2
//   analysis   F_m(k) = (2 pi / nlon) sum_j x[k][j] e^{-2 pi i m j / nlon};   c[l][m] = sum_k w_k Pbar_l^m(theta_k) F_m(k)
//   synthesis  F_m(k) = sum_l Pbar_l^m(theta_k) c[l][m];   x[k][j] = sum_m F_m(k) e^{+2 pi i m j / nlon} with irfft's Hermitian
//              completion: m = 0 and the Nyquist bin of an even nlon count once and their imaginary parts are ignored
//   vector     u east, v north (u_phi = u, u_theta = -v); Psi_lm = grad Y_lm / sqrt(l (l + 1)), Phi_lm = rhat x Psi_lm:
//              spheroidal s_lm = int u . conj(Psi_lm) dOmega = sum_k w_k ( -dPt Fv - i Qt Fu )
//              toroidal   t_lm = int u . conj(Phi_lm) dOmega = sum_k w_k (  dPt Fu - i Qt Fv )
//              for u = grad chi + rhat x grad psi: s_lm = sqrt(l (l + 1)) chi_lm, t_lm = sqrt(l (l + 1)) psi_lm
//   spectra    mult_m = 1 for m = 0 and 2 otherwise (the Nyquist column too: the reference's times_two)
//              zonal[m] = sum_l mult_m |c_lm|^2,   total[l] = sum_m mult_m |c_lm|^2
// Coefficients are complex fp64, (re, im) interleaved, [plane][lmax][mmax]; entries with l < m are written as zero.
//
// Tables live on the device for l >= m only: order m at kk * (m lmax - m (m - 1) / 2) doubles, row l - m, kk columns.  Where
// theta_k + theta_{nlat-1-k} = pi and w_k = w_{nlat-1-k} hold bit for bit, Pbar_l^m(pi - theta) = (-1)^{l+m} Pbar_l^m(theta) folds the
// rows: with S_k = F(k) + F(nlat-1-k), D_k = F(k) - F(nlat-1-k) the contraction of an even l + m runs over S, of an odd one over D,
// kk = ceil(nlat / 2) rows each (dPt has the opposite parity); the equator row of an odd nlat enters unfolded.  Any other theta runs
// unfolded, kk = nlat.  The weight w_k multiplies the field operand, so the one table serves analysis and synthesis.
//
// Launch A, sht_lon_kernel: planes of float32 or float64 -> F[m][k][n] fp64 in the handle's scratch, n = 2 (plane in pass) + (re, im)
//   innermost: the folded forward transform of wx_dft.h (dft_rows_folded).
// Launch B, sht_legendre_kernel: per m, C[l][n] = sum_k T_m[l][k] B[k][n] on v_mfma_f64_16x16x4_f64.  A wave owns one tile: 16 degrees
//   l of one parity of one m times all n of the pass (up to four accumulators); lane (c = lane & 15, g = lane >> 4) holds A[l_c][k_g]
//   and B[k_g][n_c], and D[g + 4 reg][c].  Every tile contracts over the same kk rows, so the flat tile list (built on the host; l < m
//   is never in it) keeps the chip even.  The vector form accumulates its four products into s and t in the same registers.
// Synthesis, sht_legendre_inv_kernel then sht_lon_inv_kernel: the transposed contraction (tiles of 16 rows k of one m, orders
//   ascending: the long contractions first) and the inverse transform of wx_dft.h (dft_rows_inverse).
// A pass takes up to kShtMaxPlanes planes; more planes take more passes.  Every sum has one fixed order and an output depends on its
// own plane only: coefficients, fields and spectra are bit-identical whatever P, the plane's position or the split into calls.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "wx_common.h"
#include "wx_dft.h"
#include "wx_reduce.h"

namespace wx {

constexpr int kShtMaxPlanes = 32;        // planes of one pass: 64 columns n, four MFMA column blocks
constexpr int kShtF32 = 0, kShtF64 = 1;  // the dtype flag of a field
constexpr double kShtPi = 3.14159265358979323846;

// ---- host-only helpers (no HIP call) ---------------------------------------------------------------------------------------------
// Pbar of order m at K colatitudes: out[(l - m) K + k], m <= l < lmax; no sign.
inline void sht_legendre_column(int m, int lmax, const double* theta, int K, std::vector<double>& out) {
  out.assign((size_t)std::max(0, lmax - m) * K, 0.0);
  if (m >= lmax) return;
  for (int k = 0; k < K; ++k) {
    const double x = std::cos(theta[k]), s = std::sin(theta[k]);
    double diag = 1.0 / std::sqrt(4.0 * kShtPi);
    for (int i = 1; i <= m; ++i) diag = std::sqrt((double)(2 * i + 1) / (double)(2 * i)) * s * diag;
    out[k] = diag;
    if (m + 1 < lmax) out[(size_t)K + k] = std::sqrt((double)(2 * m + 3)) * x * diag;
    for (int l = m + 2; l < lmax; ++l) {
      const double a = std::sqrt((double)(4.0 * l * l - 1.0) / (double)((double)l * l - (double)m * m));
      const double b = std::sqrt((double)((double)(l - 1) * (l - 1) - (double)m * m) / (double)(4.0 * (l - 1) * (l - 1) - 1.0));
      out[(size_t)(l - m) * K + k] = a * (x * out[(size_t)(l - 1 - m) * K + k] - b * out[(size_t)(l - 2 - m) * K + k]);
    }
  }
}

// Column m of table 0 (Pbar), 1 (dPt) or 2 (Qt) at K colatitudes, out[(l - m) K + k]; lo and hi are the Pbar columns m - 1 (unused
// for m = 0) and m + 1 over the same lmax, as sht_legendre_column makes them.
inline void sht_ladder_column(int table, int m, int lmax, int K, const std::vector<double>& lo, const std::vector<double>& hi,
                              std::vector<double>& out) {
  out.assign((size_t)std::max(0, lmax - m) * K, 0.0);
  const auto at = [&](const std::vector<double>& col, int mc, int l, int k) { return (l < mc || l >= lmax) ? 0.0 : col[(size_t)(l - mc) * K + k]; };
  for (int l = std::max(m, 1); l < lmax; ++l) {
    const double norm = std::sqrt((double)l * (l + 1));
    for (int k = 0; k < K; ++k) {
      double v = 0.0;
      if (table == 1) {
        if (m == 0) v = -std::sqrt((double)l * (l + 1)) * at(hi, 1, l, k) / norm;
        else v = (std::sqrt((double)(l + m) * (l - m + 1)) * at(lo, m - 1, l, k) - std::sqrt((double)(l - m) * (l + m + 1)) * at(hi, m + 1, l, k)) / 2.0 / norm;
      } else if (m > 0) {
        const double q = std::sqrt((double)(l - m) * (l - m - 1)) * at(hi, m + 1, l - 1, k) + std::sqrt((double)(l + m) * (l + m - 1)) * at(lo, m - 1, l - 1, k);
        v = std::sqrt((double)(2 * l + 1) / (double)(2 * l - 1)) * q / 2.0 / norm;
      }
      out[(size_t)(l - m) * K + k] = v;
    }
  }
}

// Column m of a table with the sign of csphase, out[(l - m) K + k].
inline void sht_table_column(int table, int m, int lmax, const double* theta, int K, int csphase, std::vector<double>& out) {
  if (table == 0) {
    sht_legendre_column(m, lmax, theta, K, out);
  } else {
    std::vector<double> lo, hi;
    if (m > 0) sht_legendre_column(m - 1, lmax, theta, K, lo);
    sht_legendre_column(m + 1, lmax, theta, K, hi);
    sht_ladder_column(table, m, lmax, K, lo, hi, out);
  }
  if (csphase && (m & 1))
    for (double& v : out) v = -v;
}

// Do the rows fold?  theta_k + theta_{nlat-1-k} = pi and w_k = w_{nlat-1-k}, bit for bit.
inline bool sht_folds(int nlat, const double* theta, const double* w) {
  for (int k = 0; k < (nlat + 1) / 2; ++k) {
    const int mir = nlat - 1 - k;
    if (theta[k] + theta[mir] != kShtPi || w[k] != w[mir]) return false;
  }
  return true;
}

__host__ __device__ inline int64_t sht_table_offset(int m, int lmax, int kk) { return (int64_t)kk * ((int64_t)m * lmax - (int64_t)m * (m - 1) / 2); }

// "" or the reason wx_sht_create (and wx_sht_table) refuses.
inline std::string sht_check_create(int nlat, int nlon, int lmax, int mmax, const double* theta, const double* w, const char* norm) {
  if (nlat < 2 || nlon < 2) return "nlat and nlon must be >= 2, got " + std::to_string(nlat) + " x " + std::to_string(nlon);
  if (nlon > kDftMaxN) return "nlon must be <= " + std::to_string(kDftMaxN) + " (the twiddle table lies in LDS), got " + std::to_string(nlon);
  if (nlat > 32768) return "nlat must be <= 32768, got " + std::to_string(nlat);
  if (lmax < 1 || lmax > 32768) return "lmax must be in 1 .. 32768, got " + std::to_string(lmax);
  if (mmax < 1 || mmax > std::min(lmax, nlon / 2 + 1))
    return "mmax must be in 1 .. min(lmax, nlon / 2 + 1) = " + std::to_string(std::min(lmax, nlon / 2 + 1)) + ", got " + std::to_string(mmax);
  if (!norm || std::strcmp(norm, "ortho") != 0)
    return std::string("norm must be \"ortho\" (the meaning of the library's other norms cannot be pinned here), got ") + (norm ? "\"" + std::string(norm) + "\"" : "null");
  for (int k = 0; k < nlat; ++k) {
    if (!(theta[k] >= 0.0 && theta[k] <= kShtPi)) return "a colatitude must lie in [0, pi], row " + std::to_string(k) + " does not";
    if (k > 0 && !(theta[k] > theta[k - 1])) return "the colatitudes must ascend strictly (north first), row " + std::to_string(k) + " does not";
    if (!std::isfinite(w[k])) return "a quadrature weight must be finite, row " + std::to_string(k) + " is not";
  }
  return "";
}

// "" or the reason wx_sht_table refuses.
inline std::string sht_check_table(int nlat, int lmax, int mmax, const double* theta, int table, int m) {
  if (nlat < 1 || nlat > 32768) return "nlat must be in 1 .. 32768, got " + std::to_string(nlat);
  if (lmax < 1 || lmax > 32768) return "lmax must be in 1 .. 32768, got " + std::to_string(lmax);
  if (mmax < 1 || mmax > lmax) return "mmax must be in 1 .. lmax, got " + std::to_string(mmax);
  if (table < 0 || table > 2) return "table must be 0 (Pbar), 1 (dPbar / dtheta) or 2 (m Pbar / sin theta), got " + std::to_string(table);
  if (m < 0 || m >= mmax) return "m must be in 0 .. mmax - 1, got " + std::to_string(m);
  for (int k = 0; k < nlat; ++k)
    if (!(theta[k] >= 0.0 && theta[k] <= kShtPi)) return "a colatitude must lie in [0, pi], row " + std::to_string(k) + " does not";
  return "";
}

struct ShtRange {
  const void* p;
  int64_t bytes;
};
// "" or why the ranges cannot be one call's: an output that overlaps an input or another output
inline std::string sht_check_ranges(const ShtRange* in, int n_in, const ShtRange* out, int n_out) {
  for (int i = 0; i < n_out; ++i) {
    if (!out[i].p) continue;
    for (int j = 0; j < n_in; ++j)
      if (in[j].p && bytes_overlap(out[i].p, out[i].bytes, in[j].p, in[j].bytes)) return "an output overlaps an input";
    for (int j = 0; j < i; ++j)
      if (out[j].p && bytes_overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes)) return "two outputs overlap";
  }
  return "";
}
// "" or the reason a call on n_planes planes of fields at `stride` elements is refused (the part every call shares)
inline std::string sht_check_planes(int nlat, int nlon, int n_planes, int dtype, int n_fields, const int64_t* stride) {
  const int64_t hw = (int64_t)nlat * nlon;
  if (n_planes < 1) return "n_planes must be >= 1, got " + std::to_string(n_planes);
  if (dtype != kShtF32 && dtype != kShtF64) return "dtype must be 0 (float32) or 1 (float64), got " + std::to_string(dtype);
  for (int i = 0; i < n_fields; ++i) {
    if (stride[i] < hw) return "a plane stride is smaller than nlat * nlon = " + std::to_string(hw);
    int64_t v = 0;
    if (__builtin_mul_overflow((int64_t)(n_planes - 1), stride[i], &v) || __builtin_add_overflow(v, hw, &v) || v > (1LL << 44))
      return "a plane stride takes the planes beyond 2^44 elements";
  }
  return "";
}
inline int64_t sht_field_bytes(int nlat, int nlon, int n_planes, int64_t stride, int dtype) {
  return ((int64_t)(n_planes - 1) * stride + (int64_t)nlat * nlon) * (dtype == kShtF64 ? 8 : 4);
}
inline int64_t sht_coeff_bytes(int lmax, int mmax, int n_planes) { return (int64_t)n_planes * lmax * mmax * 16; }

inline std::string sht_check_analysis(int nlat, int nlon, int lmax, int mmax, int n_planes, const void* x, int64_t stride, int dtype, const double* c) {
  if (!x || !c) return "a null pointer: the field and the coefficients are both needed";
  const std::string why = sht_check_planes(nlat, nlon, n_planes, dtype, 1, &stride);
  if (!why.empty()) return why;
  const ShtRange in[1] = {{x, sht_field_bytes(nlat, nlon, n_planes, stride, dtype)}}, out[1] = {{c, sht_coeff_bytes(lmax, mmax, n_planes)}};
  return sht_check_ranges(in, 1, out, 1);
}
inline std::string sht_check_synthesis(int nlat, int nlon, int lmax, int mmax, int n_planes, const double* c, const void* x, int dtype) {
  if (!x || !c) return "a null pointer: the coefficients and the field are both needed";
  const int64_t stride = (int64_t)nlat * nlon;
  const std::string why = sht_check_planes(nlat, nlon, n_planes, dtype, 1, &stride);
  if (!why.empty()) return why;
  const ShtRange in[1] = {{c, sht_coeff_bytes(lmax, mmax, n_planes)}}, out[1] = {{x, sht_field_bytes(nlat, nlon, n_planes, stride, dtype)}};
  return sht_check_ranges(in, 1, out, 1);
}
inline std::string sht_check_vector(int nlat, int nlon, int lmax, int mmax, int n_planes, const void* u, int64_t u_stride, const void* v,
                                    int64_t v_stride, int dtype, const double* s, const double* t) {
  if (!u || !v || !s || !t) return "a null pointer: u, v, spheroidal and toroidal are all needed";
  const int64_t strides[2] = {u_stride, v_stride};
  const std::string why = sht_check_planes(nlat, nlon, n_planes, dtype, 2, strides);
  if (!why.empty()) return why;
  const ShtRange in[2] = {{u, sht_field_bytes(nlat, nlon, n_planes, u_stride, dtype)}, {v, sht_field_bytes(nlat, nlon, n_planes, v_stride, dtype)}};
  const ShtRange out[2] = {{s, sht_coeff_bytes(lmax, mmax, n_planes)}, {t, sht_coeff_bytes(lmax, mmax, n_planes)}};
  return sht_check_ranges(in, 2, out, 2);
}
// t (the gradient form) and one of u, v (a component alone) may be null
inline std::string sht_check_vector_synthesis(int nlat, int nlon, int lmax, int mmax, int n_planes, const double* s, const double* t, const void* u,
                                              const void* v, int dtype) {
  if (!s) return "a null pointer: the spheroidal coefficients are needed (the toroidal ones may be null)";
  if (!u && !v) return "no output requested: u and v are both null";
  const int64_t stride = (int64_t)nlat * nlon;
  const std::string why = sht_check_planes(nlat, nlon, n_planes, dtype, 1, &stride);
  if (!why.empty()) return why;
  const ShtRange in[2] = {{s, sht_coeff_bytes(lmax, mmax, n_planes)}, {t, sht_coeff_bytes(lmax, mmax, n_planes)}};
  const ShtRange out[2] = {{u, sht_field_bytes(nlat, nlon, n_planes, stride, dtype)}, {v, sht_field_bytes(nlat, nlon, n_planes, stride, dtype)}};
  return sht_check_ranges(in, 2, out, 2);
}
inline std::string sht_check_spectra(int lmax, int mmax, int n_planes, const double* c, const double* zonal, const double* total) {
  if (n_planes < 1) return "n_planes must be >= 1, got " + std::to_string(n_planes);
  if (!c) return "the coefficients are a null pointer";
  if (!zonal && !total) return "no output requested: zonal and total are both null";
  const ShtRange in[1] = {{c, sht_coeff_bytes(lmax, mmax, n_planes)}};
  const ShtRange out[2] = {{zonal, (int64_t)n_planes * mmax * 8}, {total, (int64_t)n_planes * lmax * 8}};
  return sht_check_ranges(in, 1, out, 2);
}

// The tiles of launch B: {m, l0}; the tile's degrees are l0 + step c, c = 0 .. 15 (step 2 folded: one parity of l - m; else 1).
inline void sht_tiles(int lmax, int mmax, bool fold, std::vector<int2>& tiles) {
  tiles.clear();
  for (int m = 0; m < mmax; ++m) {
    if (fold) {
      for (int par = 0; par < 2; ++par)
        for (int l0 = m + par; l0 < lmax; l0 += 32) tiles.push_back(make_int2(m, l0));
    } else {
      for (int l0 = m; l0 < lmax; l0 += 16) tiles.push_back(make_int2(m, l0));
    }
  }
}

// ---- device side -------------------------------------------------------------------------------------------------------------------
struct ShtGeom {
  int nlat, nlon, lmax, mmax, kk, fold;   // kk: the rows a contraction runs over
  int np, nb;                             // planes of this pass; columns of a row of F (a multiple of 16, >= 2 np)
};

// Launch A.  src: plane p of the pass at src + p * stride, [nlat][nlon]; F[m][k][nb].  grid = row_tiles * col_blocks (column block
// fastest) over the np * nlat rows and the mmax wavenumbers, LDS 16 nlon bytes.
template <typename T>
__global__ __launch_bounds__(256) void sht_lon_kernel(const T* __restrict__ src, int64_t stride, ShtGeom s, const double2* __restrict__ tab_g,
                                                      double* __restrict__ F, int col_blocks) {
  extern __shared__ double2 sht_lds[];
  const int W = s.nlon, M = s.np * s.nlat;
  dft_stage_table(sht_lds, tab_g, W);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int cb = (int)(blockIdx.x % (unsigned)col_blocks), rt = (int)(blockIdx.x / (unsigned)col_blocks);
  const int r0 = rt * kDftTileRows + wave * kDftWaveRows, k0 = cb * kDftTileCols;
  if (r0 >= M) return;                                   // wave-uniform, after the only barrier
  const int row = r0 + c;
  const bool row_ok = row < M;
  const int rpl = row_ok ? row / s.nlat : 0, rk = row_ok ? row - rpl * s.nlat : 0;
  const T* arow[1] = {src + (int64_t)rpl * stride + (int64_t)rk * W};
  f64x4_t re[1][2] = {}, im[1][2] = {};
  dft_rows_folded<1, T>(arow, row_ok, W, k0, sht_lds, re, im);
  const double scale = 2.0 * kShtPi / (double)W;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int m = k0 + 16 * t + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int R = r0 + g + 4 * r;
      if (R < M && m < s.mmax) {
        const int pl = R / s.nlat, k = R - pl * s.nlat;
        double2* dst = (double2*)(F + ((int64_t)m * s.nlat + k) * s.nb + 2 * pl);
        *dst = make_double2(scale * re[0][t][r], -(scale * im[0][t][r]));
      }
    }
  }
}

// The field operand of row k (< kk), column n (< nb) of order m: F, or its fold with the mirror row.  odd: the table's parity about
// the equator is odd (the difference enters; nothing at the equator row itself).
__device__ inline double sht_operand(const double* __restrict__ F, const ShtGeom& s, int m, int k, int n, bool odd) {
  const double f = F[((int64_t)m * s.nlat + k) * s.nb + n];
  if (!s.fold) return f;
  const int mir = s.nlat - 1 - k;
  if (mir == k) return odd ? 0.0 : f;
  const double f2 = F[((int64_t)m * s.nlat + mir) * s.nb + n];
  return odd ? f - f2 : f + f2;
}

struct ShtOut {
  double* a;   // coefficients of plane 0 of the pass: c, or spheroidal
  double* b;   // toroidal (vector form)
};

// Launch B.  grid = ceil(n_tiles / 4), a wave per tile; NCB = nb / 16 column blocks.  VEC: tab = dPt, tab2 = Qt, F = Fu, F2 = Fv.
template <bool VEC>
__global__ __launch_bounds__(256) void sht_legendre_kernel(const int2* __restrict__ tiles, int n_tiles, const double* __restrict__ tab,
                                                           const double* __restrict__ tab2, const double* __restrict__ F,
                                                           const double* __restrict__ F2, const double* __restrict__ w, ShtGeom s, ShtOut out) {
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int tile = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (tile >= n_tiles) return;
  const int m = tiles[tile].x, l0 = tiles[tile].y, step = s.fold ? 2 : 1;
  const bool par = s.fold && ((l0 - m) & 1);             // the parity of l + m of every degree of the tile
  const int ncb = s.nb >> 4;
  const int l = l0 + step * c;
  const bool l_ok = l < s.lmax;
  const int64_t roff = sht_table_offset(m, s.lmax, s.kk) + (int64_t)((l_ok ? l : l0) - m) * s.kk;
  const double* arow = tab + roff;
  const double* arow2 = VEC ? tab2 + roff : nullptr;
  f64x4_t acc[4] = {}, acc2[4] = {};
  for (int kc = 0; kc < s.kk; kc += 16) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = kc + 4 * g + j;
      const bool k_ok = k < s.kk;
      const double a = (l_ok && k_ok) ? arow[k] : 0.0;
      const double a2 = (VEC && l_ok && k_ok) ? arow2[k] : 0.0;
      const double wk = k_ok ? w[k] : 0.0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t < ncb) {
          const int n = 16 * t + c;
          if (!VEC) {
            const double b = k_ok ? wk * sht_operand(F, s, m, k, n, par) : 0.0;
            acc[t] = mfma_f64_16x16x4(a, b, acc[t]);
          } else {
            // s += -dPt Fv + Qt (-i Fu),  t += dPt Fu + Qt (-i Fv);  (-i z)[re] = z[im], (-i z)[im] = -z[re];  dPt has the parity !par
            const double sg = (n & 1) ? -1.0 : 1.0;
            const double bu = k_ok ? wk * sht_operand(F, s, m, k, n, !par) : 0.0;
            const double bv = k_ok ? wk * sht_operand(F2, s, m, k, n, !par) : 0.0;
            const double bux = k_ok ? sg * (wk * sht_operand(F, s, m, k, n ^ 1, par)) : 0.0;
            const double bvx = k_ok ? sg * (wk * sht_operand(F2, s, m, k, n ^ 1, par)) : 0.0;
            acc[t] = mfma_f64_16x16x4(a, -bv, acc[t]);
            acc[t] = mfma_f64_16x16x4(a2, bux, acc[t]);
            acc2[t] = mfma_f64_16x16x4(a, bu, acc2[t]);
            acc2[t] = mfma_f64_16x16x4(a2, bvx, acc2[t]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t < ncb) {
      const int n = 16 * t + c, pl = n >> 1;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lo = l0 + step * (g + 4 * r);
        if (lo < s.lmax && pl < s.np) {
          const int64_t o = (((int64_t)pl * s.lmax + lo) * s.mmax + m) * 2 + (n & 1);
          out.a[o] = acc[t][r];
          if (VEC) out.b[o] = acc2[t][r];
        }
      }
    }
  }
}

// Synthesis, first launch.  cin: the coefficients of plane 0 of the pass; G[m][k][nb].  grid = ceil(mmax * ktiles / 4), a wave per
// (m, 16 rows k), orders ascending.
__global__ __launch_bounds__(256) void sht_legendre_inv_kernel(const double* __restrict__ tab, const double* __restrict__ cin, ShtGeom s, int ktiles,
                                                               double* __restrict__ G) {
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int tile = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (tile >= s.mmax * ktiles) return;
  const int m = tile / ktiles, kt = tile - m * ktiles;
  const int ncb = s.nb >> 4;
  const int k = kt * 16 + c;
  const bool k_ok = k < s.kk;
  const double* acol = tab + sht_table_offset(m, s.lmax, s.kk) + (k_ok ? k : 0);
  f64x4_t acc[2][4] = {};                                // [parity of l + m]; unfolded: every degree in [0]
  const int step = s.fold ? 2 : 1;
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    if (par == 1 && !s.fold) break;
    for (int ic = 0; m + par + step * ic < s.lmax; ic += 16) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int l = m + par + step * (ic + 4 * g + j);
        const bool l_ok = l < s.lmax;
        const double a = (l_ok && k_ok) ? acol[(int64_t)(l - m) * s.kk] : 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (t < ncb) {
            const int n = 16 * t + c, pl = n >> 1;
            const double b = (l_ok && pl < s.np) ? cin[(((int64_t)pl * s.lmax + l) * s.mmax + m) * 2 + (n & 1)] : 0.0;
            acc[par][t] = mfma_f64_16x16x4(a, b, acc[par][t]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t < ncb) {
      const int n = 16 * t + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ko = kt * 16 + g + 4 * r;
        if (ko < s.kk) {
          const double e = acc[0][t][r], o = acc[1][t][r];
          G[((int64_t)m * s.nlat + ko) * s.nb + n] = e + o;
          const int mir = s.nlat - 1 - ko;
          if (s.fold && mir != ko) G[((int64_t)m * s.nlat + mir) * s.nb + n] = e - o;
        }
      }
    }
  }
}

// Vector synthesis, first launch: sht_legendre_inv_kernel's tiling on the two vector tables.  With (i z)[re] = -z[im], (i z)[im] = z[re]:
//   Gu = F_phi = sum_l Qt (i s) + dPt t,   Gv = -F_theta = sum_l -dPt s + Qt (i t);   u = lon_synth(Gu), v = lon_synth(Gv)
// Qt has Pbar's parity about the equator and dPt the opposite one, so a product lands in the accumulator of its own symmetry: [0]
// symmetric, [1] antisymmetric, row k = [0] + [1], mirror row = [0] - [1].  Unfolded, the two are simply added.  lscale (may be null):
// a factor per degree l, multiplied into the table operand.  HAS_T false: tor is never read (the gradient form).  COMP: 1 = Gu alone,
// 2 = Gv alone, 3 = both.  sph, tor: the coefficients of plane 0 of the pass.
template <bool HAS_T, int COMP>
__global__ __launch_bounds__(256) void sht_legendre_vinv_kernel(const double* __restrict__ tab_d, const double* __restrict__ tab_q,
                                                                const double* __restrict__ lscale, const double* __restrict__ sph,
                                                                const double* __restrict__ tor, ShtGeom s, int ktiles, double* __restrict__ Gu,
                                                                double* __restrict__ Gv) {
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int tile = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (tile >= s.mmax * ktiles) return;
  const int m = tile / ktiles, kt = tile - m * ktiles;
  const int ncb = s.nb >> 4;
  const int k = kt * 16 + c;
  const bool k_ok = k < s.kk;
  const int64_t coff = sht_table_offset(m, s.lmax, s.kk) + (k_ok ? k : 0);
  const double* dcol = tab_d + coff;
  const double* qcol = tab_q + coff;
  f64x4_t au[2][4] = {}, av[2][4] = {};
  const int step = s.fold ? 2 : 1;
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    if (par == 1 && !s.fold) break;
    for (int ic = 0; m + par + step * ic < s.lmax; ic += 16) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int l = m + par + step * (ic + 4 * g + j);
        const bool l_ok = l < s.lmax;
        const bool a_ok = l_ok && k_ok;
        const double ls = (l_ok && lscale) ? lscale[l] : 1.0;
        const double d = a_ok ? ls * dcol[(int64_t)(l - m) * s.kk] : 0.0;
        const double q = a_ok ? ls * qcol[(int64_t)(l - m) * s.kk] : 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (t < ncb) {
            const int n = 16 * t + c, pl = n >> 1, im = n & 1;
            const bool ok = l_ok && pl < s.np;
            const int64_t base = (((int64_t)pl * s.lmax + l) * s.mmax + m) * 2;
            const double sg = im ? 1.0 : -1.0;
            const double sn = ok ? sph[base + im] : 0.0;
            const double sx = ok ? sg * sph[base + (im ^ 1)] : 0.0;
            const double tn = (HAS_T && ok) ? tor[base + im] : 0.0;
            const double tx = (HAS_T && ok) ? sg * tor[base + (im ^ 1)] : 0.0;
            if (COMP & 1) {
              au[par][t] = mfma_f64_16x16x4(q, sx, au[par][t]);
              if (HAS_T) au[par ^ 1][t] = mfma_f64_16x16x4(d, tn, au[par ^ 1][t]);
            }
            if (COMP & 2) {
              av[par ^ 1][t] = mfma_f64_16x16x4(d, -sn, av[par ^ 1][t]);
              if (HAS_T) av[par][t] = mfma_f64_16x16x4(q, tx, av[par][t]);
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t < ncb) {
      const int n = 16 * t + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ko = kt * 16 + g + 4 * r;
        if (ko < s.kk) {
          const int mir = s.nlat - 1 - ko;
          const bool both = s.fold && mir != ko;
          const int64_t o = ((int64_t)m * s.nlat + ko) * s.nb + n, om = ((int64_t)m * s.nlat + mir) * s.nb + n;
          if (COMP & 1) {
            Gu[o] = au[0][t][r] + au[1][t][r];
            if (both) Gu[om] = au[0][t][r] - au[1][t][r];
          }
          if (COMP & 2) {
            Gv[o] = av[0][t][r] + av[1][t][r];
            if (both) Gv[om] = av[0][t][r] - av[1][t][r];
          }
        }
      }
    }
  }
}

// Synthesis, second launch: dft_rows_inverse on G[m][k][nb].  dst: plane p of the pass at dst + p * nlat * nlon.
// grid = (ceil(nlon / 64), ceil(np * nlat / 64)), LDS 16 nlon bytes.
template <typename T>
__global__ __launch_bounds__(256) void sht_lon_inv_kernel(const double* __restrict__ G, ShtGeom s, const double2* __restrict__ tab_g, T* __restrict__ dst) {
  extern __shared__ double2 sht_lds[];
  const int W = s.nlon, M = s.np * s.nlat;
  dft_stage_table(sht_lds, tab_g, W);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int m0 = ((int)blockIdx.y * 4 + wave) * 16, n0 = (int)blockIdx.x * 64;
  if (m0 >= M) return;
  const int row = m0 + c;
  const bool row_ok = row < M;
  const int rpl = row_ok ? row / s.nlat : 0, rk = row_ok ? row - rpl * s.nlat : 0;
  const double* zrow = G + (int64_t)rk * s.nb + 2 * rpl;  // bin m of the row at zrow + m * nlat * nb: (re, im)
  const int64_t bin = (int64_t)s.nlat * s.nb;
  f64x4_t acc[4] = {};
  dft_rows_inverse([&](int m) { return (row_ok && m < s.mmax) ? *(const double2*)(zrow + (int64_t)m * bin) : make_double2(0.0, 0.0); }, s.mmax, W,
                   n0, sht_lds, acc);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int x = n0 + 16 * t + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int R = m0 + g + 4 * r;
      if (R < M && x < W) dst[(int64_t)R * W + x] = (T)acc[t][r];
    }
  }
}

// Spectra of c[P][lmax][mmax]: grid = P, a workgroup of 256 per plane.  total[l]: a wave per degree, lanes strided over m ascending,
// then wave_sum; zonal[m]: a thread per order, l ascending.
__global__ __launch_bounds__(256) void sht_spectra_kernel(const double* __restrict__ c, int lmax, int mmax, double* __restrict__ zonal,
                                                          double* __restrict__ total) {
  const int64_t p = blockIdx.x;
  const double2* cp = (const double2*)c + p * lmax * mmax;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (total) {
    for (int l = wave; l < lmax; l += 4) {
      double acc[1] = {0.0};
      for (int m = lane; m < mmax && m <= l; m += 64) {
        const double2 z = cp[(int64_t)l * mmax + m];
        acc[0] += (m == 0 ? 1.0 : 2.0) * dft_power(z.x, z.y);
      }
      wave_sum<1>(acc);
      if (lane == 0) total[p * lmax + l] = acc[0];
    }
  }
  if (zonal) {
    for (int m = threadIdx.x; m < mmax; m += 256) {
      double acc = 0.0;
      for (int l = m; l < lmax; ++l) {
        const double2 z = cp[(int64_t)l * mmax + m];
        acc += (m == 0 ? 1.0 : 2.0) * dft_power(z.x, z.y);
      }
      zonal[p * mmax + m] = acc;
    }
  }
}

class Sht {
 public:
  Sht(int nlat_, int nlon_, int lmax_, int mmax_, const double* theta_host, const double* w_host, int csphase_, int dev)
      : nlat(nlat_), nlon(nlon_), lmax(lmax_), mmax(mmax_), csphase(csphase_), device(dev), mem(dev), theta(theta_host, theta_host + nlat_) {
    WX_HIP(hipSetDevice(device));
    fold = sht_folds(nlat, theta_host, w_host);
    kk = fold ? (nlat + 1) / 2 : nlat;
    std::vector<double2> t;
    dft_table(nlon, t);
    twiddle = mem.upload(t.data(), t.size());
    w = mem.upload(w_host, (size_t)nlat);
    std::vector<int2> tl;
    sht_tiles(lmax, mmax, fold, tl);
    n_tiles = (int)tl.size();
    tiles = mem.upload(tl.data(), tl.size());
  }

  int64_t table_bytes() const { return sht_table_offset(mmax, lmax, kk) * 8; }

  void analysis(int n_planes, const void* x, int64_t stride, int dtype, double* c, hipStream_t stream) {
    const std::string why = sht_check_analysis(nlat, nlon, lmax, mmax, n_planes, x, stride, dtype, c);
    if (!why.empty()) throw std::runtime_error("wx_sht_analysis: " + why);
    WX_HIP(hipSetDevice(device));
    if (!tab[0]) build_tables(false);                    // the scalar table: built by the first call that needs it
    WX_HIP(hipMemsetAsync(c, 0, (size_t)sht_coeff_bytes(lmax, mmax, n_planes), stream));   // the entries with l < m
    for (int p0 = 0; p0 < n_planes; p0 += kShtMaxPlanes) {
      const ShtGeom s = pass(std::min(kShtMaxPlanes, n_planes - p0), 1);
      forward_lon(x, stride, dtype, p0, s, buf[0], stream);
      ShtOut o = {c + (int64_t)p0 * lmax * mmax * 2, nullptr};
      hipLaunchKernelGGL(sht_legendre_kernel<false>, dim3((unsigned)cdiv(n_tiles, 4)), dim3(256), 0, stream, tiles, n_tiles, tab[0],
                         (const double*)nullptr, buf[0], (const double*)nullptr, w, s, o);
      WX_HIP(hipGetLastError());
    }
  }

  void vector_analysis(int n_planes, const void* u, int64_t u_stride, const void* v, int64_t v_stride, int dtype, double* sph, double* tor,
                       hipStream_t stream) {
    const std::string why = sht_check_vector(nlat, nlon, lmax, mmax, n_planes, u, u_stride, v, v_stride, dtype, sph, tor);
    if (!why.empty()) throw std::runtime_error("wx_sht_vector_analysis: " + why);
    WX_HIP(hipSetDevice(device));
    if (!tab[1]) build_tables(true);                     // the vector tables: built by the first call that needs them
    WX_HIP(hipMemsetAsync(sph, 0, (size_t)sht_coeff_bytes(lmax, mmax, n_planes), stream));
    WX_HIP(hipMemsetAsync(tor, 0, (size_t)sht_coeff_bytes(lmax, mmax, n_planes), stream));
    for (int p0 = 0; p0 < n_planes; p0 += kShtMaxPlanes) {
      const ShtGeom s = pass(std::min(kShtMaxPlanes, n_planes - p0), 2);
      forward_lon(u, u_stride, dtype, p0, s, buf[0], stream);
      forward_lon(v, v_stride, dtype, p0, s, buf[1], stream);
      ShtOut o = {sph + (int64_t)p0 * lmax * mmax * 2, tor + (int64_t)p0 * lmax * mmax * 2};
      hipLaunchKernelGGL(sht_legendre_kernel<true>, dim3((unsigned)cdiv(n_tiles, 4)), dim3(256), 0, stream, tiles, n_tiles, tab[1], tab[2], buf[0],
                         buf[1], w, s, o);
      WX_HIP(hipGetLastError());
    }
  }

  void synthesis(int n_planes, const double* c, void* x, int dtype, hipStream_t stream) {
    const std::string why = sht_check_synthesis(nlat, nlon, lmax, mmax, n_planes, c, x, dtype);
    if (!why.empty()) throw std::runtime_error("wx_sht_synthesis: " + why);
    WX_HIP(hipSetDevice(device));
    if (!tab[0]) build_tables(false);
    const int ktiles = cdiv(kk, 16);
    for (int p0 = 0; p0 < n_planes; p0 += kShtMaxPlanes) {
      const ShtGeom s = pass(std::min(kShtMaxPlanes, n_planes - p0), 1);
      hipLaunchKernelGGL(sht_legendre_inv_kernel, dim3((unsigned)cdiv((int64_t)mmax * ktiles, 4)), dim3(256), 0, stream, tab[0],
                         c + (int64_t)p0 * lmax * mmax * 2, s, ktiles, buf[0]);
      WX_HIP(hipGetLastError());
      const dim3 grid((unsigned)cdiv(nlon, 64), (unsigned)cdiv((int64_t)s.np * nlat, 64));
      const size_t lds = dft_lds_bytes(nlon);
      const int64_t off = (int64_t)p0 * nlat * nlon;
      if (dtype == kShtF64) hipLaunchKernelGGL(sht_lon_inv_kernel<double>, grid, dim3(256), lds, stream, buf[0], s, twiddle, (double*)x + off);
      else hipLaunchKernelGGL(sht_lon_inv_kernel<float>, grid, dim3(256), lds, stream, buf[0], s, twiddle, (float*)x + off);
      WX_HIP(hipGetLastError());
    }
  }

  // (u, v) [n_planes][nlat][nlon] from spheroidal sph and toroidal tor (null: the gradient form); u or v null: the other component
  // alone.  lscale: [lmax] on the device or null, a factor per degree.
  void vector_synthesis(int n_planes, const double* sph, const double* tor, const double* lscale, void* u, void* v, int dtype, hipStream_t stream) {
    const std::string why = sht_check_vector_synthesis(nlat, nlon, lmax, mmax, n_planes, sph, tor, u, v, dtype);
    if (!why.empty()) throw std::runtime_error("wx_sht_vector_synthesis: " + why);
    WX_HIP(hipSetDevice(device));
    if (!tab[1]) build_tables(true);
    const int ktiles = cdiv(kk, 16);
    const int comp = (u ? 1 : 0) | (v ? 2 : 0);
    for (int p0 = 0; p0 < n_planes; p0 += kShtMaxPlanes) {
      const ShtGeom s = pass(std::min(kShtMaxPlanes, n_planes - p0), 2);
      const dim3 lgrid((unsigned)cdiv((int64_t)mmax * ktiles, 4));
      const int64_t coff = (int64_t)p0 * lmax * mmax * 2;
      const double* sp = sph + coff;
      const double* tp = tor ? tor + coff : nullptr;
#define WX_SHT_VINV(HAS_T, COMP)                                                                                                        \
  hipLaunchKernelGGL((sht_legendre_vinv_kernel<HAS_T, COMP>), lgrid, dim3(256), 0, stream, tab[1], tab[2], lscale, sp, tp, s, ktiles, buf[0], buf[1])
      if (tor) {
        if (comp == 1) WX_SHT_VINV(true, 1); else if (comp == 2) WX_SHT_VINV(true, 2); else WX_SHT_VINV(true, 3);
      } else {
        if (comp == 1) WX_SHT_VINV(false, 1); else if (comp == 2) WX_SHT_VINV(false, 2); else WX_SHT_VINV(false, 3);
      }
#undef WX_SHT_VINV
      WX_HIP(hipGetLastError());
      const dim3 grid((unsigned)cdiv(nlon, 64), (unsigned)cdiv((int64_t)s.np * nlat, 64));
      const size_t lds = dft_lds_bytes(nlon);
      const int64_t off = (int64_t)p0 * nlat * nlon;
      void* dst[2] = {u, v};
      for (int i = 0; i < 2; ++i) {
        if (!dst[i]) continue;
        if (dtype == kShtF64) hipLaunchKernelGGL(sht_lon_inv_kernel<double>, grid, dim3(256), lds, stream, buf[i], s, twiddle, (double*)dst[i] + off);
        else hipLaunchKernelGGL(sht_lon_inv_kernel<float>, grid, dim3(256), lds, stream, buf[i], s, twiddle, (float*)dst[i] + off);
        WX_HIP(hipGetLastError());
      }
    }
  }

  // the scratch of a pass of np planes, in bytes: both buffers
  static int64_t scratch_bytes(int nlat, int mmax, int np) { return 2 * (int64_t)mmax * nlat * ((2 * np + 15) / 16 * 16) * 8; }
  int n_lat() const { return nlat; }
  int n_lon() const { return nlon; }
  int l_max() const { return lmax; }
  int m_max() const { return mmax; }

  void spectra(int n_planes, const double* c, double* zonal, double* total, hipStream_t stream) {
    const std::string why = sht_check_spectra(lmax, mmax, n_planes, c, zonal, total);
    if (!why.empty()) throw std::runtime_error("wx_sht_spectra: " + why);
    WX_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(sht_spectra_kernel, dim3((unsigned)n_planes), dim3(256), 0, stream, c, lmax, mmax, zonal, total);
    WX_HIP(hipGetLastError());
  }

 private:
  // the geometry of a pass of np planes; the scratch of its n_buf fields grows to hold it
  ShtGeom pass(int np, int n_buf) {
    ShtGeom s;
    s.nlat = nlat; s.nlon = nlon; s.lmax = lmax; s.mmax = mmax; s.kk = kk; s.fold = fold ? 1 : 0;
    s.np = np;
    s.nb = (2 * np + 15) / 16 * 16;
    for (int i = 0; i < n_buf; ++i) grow(buf[i], buf_have[i], (size_t)mmax * nlat * s.nb);
    return s;
  }
  void forward_lon(const void* x, int64_t stride, int dtype, int p0, const ShtGeom& s, double* F, hipStream_t stream) {
    const int col_blocks = cdiv(mmax, kDftTileCols);
    const dim3 grid((unsigned)((int64_t)cdiv((int64_t)s.np * nlat, kDftTileRows) * col_blocks));
    const size_t lds = dft_lds_bytes(nlon);
    if (dtype == kShtF64)
      hipLaunchKernelGGL(sht_lon_kernel<double>, grid, dim3(256), lds, stream, (const double*)x + (int64_t)p0 * stride, stride, s, twiddle, F, col_blocks);
    else
      hipLaunchKernelGGL(sht_lon_kernel<float>, grid, dim3(256), lds, stream, (const float*)x + (int64_t)p0 * stride, stride, s, twiddle, F, col_blocks);
    WX_HIP(hipGetLastError());
  }
  // an allocation that fails is an error with the byte count
  void grow(double*& p, size_t& have, size_t want) {
    try {
      mem.grow(p, have, want);
    } catch (const HipError& e) {
      throw HipError("wx_sht: the scratch of " + std::to_string(want * 8) + " bytes could not be allocated: " + e.what());
    }
  }
  // Pinned host memory of one table build, freed whatever happens.
  struct Pinned {
    double* p = nullptr;
    explicit Pinned(size_t n) { WX_HIP(hipHostMalloc((void**)&p, n * sizeof(double), hipHostMallocDefault)); }
    ~Pinned() { (void)hipHostFree(p); }
    Pinned(const Pinned&) = delete;
    Pinned& operator=(const Pinned&) = delete;
  };
  // Builds the scalar table (tab[0]) or the two vector tables (tab[1], tab[2]) on the host and uploads them.  Every Pbar column is
  // made once: the ladders of order m take the columns m - 1 and m + 1 from a window of three that moves with m.  The columns of
  // a table are contiguous on the device, so they gather in a pinned stage and leave in one copy per kStageDoubles.
  void build_tables(bool vector) {
    constexpr size_t kStageDoubles = (size_t)4 << 20;     // 32 MB per table
    const size_t n = (size_t)sht_table_offset(mmax, lmax, kk);
    const int first = vector ? 1 : 0, count = vector ? 2 : 1;
    double* d[2] = {nullptr, nullptr};
    try {
      for (int t = 0; t < count; ++t) d[t] = (double*)mem.alloc(n * sizeof(double));
      const size_t cap = std::max((size_t)lmax * kk, std::min(n, kStageDoubles));
      Pinned stage0(cap), stage1(vector ? cap : 1);
      double* stage[2] = {stage0.p, stage1.p};
      size_t base = 0, fill = 0;
      const auto flush = [&] {
        for (int t = 0; t < count && fill; ++t) WX_HIP(hipMemcpy(d[t] + base, stage[t], fill * sizeof(double), hipMemcpyHostToDevice));
        base += fill;
        fill = 0;
      };
      std::vector<double> lo, mid, hi, col[2];
      if (vector) {
        sht_legendre_column(0, lmax, theta.data(), kk, mid);
        sht_legendre_column(1, lmax, theta.data(), kk, hi);
      }
      for (int m = 0; m < mmax; ++m) {
        if (!vector) {
          sht_legendre_column(m, lmax, theta.data(), kk, col[0]);
        } else {
          sht_ladder_column(1, m, lmax, kk, lo, hi, col[0]);
          sht_ladder_column(2, m, lmax, kk, lo, hi, col[1]);
          lo.swap(mid);                                    // the window moves: (m - 1, m, m + 1) -> (m, m + 1, m + 2)
          mid.swap(hi);
          sht_legendre_column(m + 2, lmax, theta.data(), kk, hi);
        }
        const size_t len = col[0].size();
        if (fill + len > cap) flush();
        const double sign = (csphase && (m & 1)) ? -1.0 : 1.0;
        for (int t = 0; t < count; ++t)
          for (size_t i = 0; i < len; ++i) stage[t][fill + i] = sign * col[t][i];
        fill += len;
      }
      flush();
    } catch (const HipError& e) {
      for (int t = 0; t < count; ++t) mem.release(d[t]);
      throw HipError("wx_sht: " + std::string(vector ? "the two vector tables" : "the scalar table") + " of " + std::to_string(n * 8) +
                     " bytes each could not be built on the device: " + e.what());
    }
    for (int t = 0; t < count; ++t) tab[first + t] = d[t];
  }

  int nlat, nlon, lmax, mmax, csphase, device;
  DeviceArena mem;
  std::vector<double> theta;
  bool fold = false;
  int kk = 0, n_tiles = 0;
  double2* twiddle = nullptr;
  double* w = nullptr;
  int2* tiles = nullptr;
  double* tab[3] = {nullptr, nullptr, nullptr};
  double* buf[2] = {nullptr, nullptr};
  size_t buf_have[2] = {0, 0};
};

}  // namespace wx
