// The dense fp64 DFT along a row of N points that the perturbed-IC noise (wx_perturb.h), the zonal spectra (wx_spectrum.h) and the
// spherical harmonic transforms (wx_sht.h, and wx_polefilter.h on top of them) share: no FFT library and no factorisation, a matrix
// product on v_mfma_f64_16x16x4_f64 whose twiddle matrix never lies in memory.
//   MFMA     D = A B + C (mfma_f64_16x16x4 of wx_common.h): lane l, c = l & 15, g = l >> 4, holds A[c][g], B[g][c] and D[g + 4 reg][c],
//            reg 0 .. 3.  K runs in chunks of 16: lane group g takes k = chunk + 4 g + j in MFMA j = 0 .. 3, so a lane reads four
//            consecutive elements of its row.
//   table    each pass stages (cos, sin)(2 pi j / N), j < N, built on the host in fp64 (dft_table), in LDS: 16 N bytes, hence
//            N <= kDftMaxN.  It is indexed by (k x) mod N kept in INTEGER arithmetic -- DftPhase: one 64-bit modulo at the start, then
//            additions with a conditional subtraction -- which is what keeps the phase exact at N = 1440.
//   fold     forward transform of a real row r[W] onto Wh = W / 2 + 1 bins (dft_rows_folded): with e[x] = r[x] + r[W - x] and
//            o[x] = r[x] - r[W - x] for x = 1 .. ceil(W / 2) - 1 (exact in fp64 for float32 input),  re X_k = sum e[x] cos,
//            -im X_k = sum o[x] sin;  x = 0 and, for even W, x = W / 2 enter unfolded with zero in the sin sum.  K runs over Wh values
//            of x instead of W.  A wave owns 16 rows x 32 wavenumbers: two accumulators hold the cos sums and two the sin sums of the
//            SAME 32 k, so the lane that holds re of (row, k) holds im as well, and one twiddle read feeds both and every field.  A
//            workgroup is four waves on 64 consecutive rows.  A lane's elements and mirrors of the next chunk are fetched before the
//            MFMAs of the current one.
//   inverse  half-complex row -> real row by irfft's conventions (dft_rows_inverse): bin 0 and, for even W, the Nyquist bin count once
//            and their imaginary parts are ignored; every other bin counts twice; unscaled.  A wave owns 16 rows x 64 columns (four
//            accumulators share the A operand), a workgroup of four waves 64 x 64; a lane takes the two bins chunk / 2 + 2 g + b.
//   order    every sum has one fixed order: k ascending by chunk and j (inverse: bin, then re, im); inside an MFMA the hardware's.
//            An output element depends on its own row and column only.
#pragma once
#include <cmath>
#include <vector>

#include "wx_common.h"

namespace wx {

constexpr int kDftMaxN = 4096;        // the LDS table of one pass: 16 bytes per entry, 64 KB
constexpr int kDftWaveRows = 16;      // the folded transform's tile
constexpr int kDftTileRows = 64;      // a workgroup: four waves
constexpr int kDftTileCols = 32;      // wavenumbers of a workgroup: two MFMA column blocks

// (cos, sin)(2 pi j / N), j = 0 .. N - 1, in fp64
inline void dft_table(int N, std::vector<double2>& t) {
  t.resize(N);
  for (int j = 0; j < N; ++j) {
    const double a = 2.0 * 3.14159265358979323846 * (double)j / (double)N;
    t[j] = make_double2(std::cos(a), std::sin(a));
  }
}
inline size_t dft_lds_bytes(int N) { return (size_t)N * sizeof(double2); }

__host__ __device__ inline int dft_wrap(int i, int N) { return i >= N ? i - N : i; }   // i < 2 N
__device__ inline void dft_stage_table(double2* tab, const double2* tab_g, int N) {
  for (int i = threadIdx.x; i < N; i += 256) tab[i] = tab_g[i];
  __syncthreads();
}

// The running table index (k x) mod N of one output column k (any k >= 0: it is reduced here; columns past the last are computed and
// never stored).  x starts at `first` and moves by 1 (step) or on to the lane's place in the next chunk (skip).  The forward passes
// walk (4 g, 12): four steps and a skip are a chunk of 16; the inverse passes (2 g, 8) with ahead() for the lane's second bin.
struct DftPhase {
  int idx, k, chunk;
  __host__ __device__ void init(int k_, int first, int chunk_skip, int N) {
    k = k_ % N;
    idx = (int)(((int64_t)k * first) % N);
    chunk = (int)(((int64_t)k * chunk_skip) % N);
  }
  __host__ __device__ int ahead(int N) const { return dft_wrap(idx + k, N); }
  __host__ __device__ void step(int N) { idx = ahead(N); }
  __host__ __device__ void skip(int N) { idx = dft_wrap(idx + chunk, N); }
};

// The fold of column x: v = r[x], m = its mirror r[W - x] (0 where x has none); e enters the cos sum, o the sin sum.
__host__ __device__ inline bool dft_has_mirror(int W, int x) { return x != 0 && 2 * x != W; }
template <typename T>
__host__ __device__ inline void dft_fold_pair(T v, T m, bool pair, double& e, double& o) {
  e = (double)v + (double)m;
  o = pair ? (double)v - (double)m : 0.0;
}
// The folded operand of column x (0 <= x < Wh) of a row r[W].
template <typename T>
inline void dft_fold(const T* r, int W, int x, double& e, double& o) {
  const bool pair = dft_has_mirror(W, x);
  dft_fold_pair(r[x], pair ? r[W - x] : (T)0, pair, e, o);
}

__device__ inline double dft_power(double re, double im) { return fma(re, re, im * im); }

// The folded forward transform of the lane's row c of NF fields (row[f]: its W elements; row_ok false: zeros, nothing is read) onto
// the wavenumbers k0 + 16 t + c, t = 0, 1: re[f][t] += sum e cos, im[f][t] += sum o sin (-im X).  tab: the staged table of W entries.
template <int NF, typename T>
__device__ __forceinline__ void dft_rows_folded(const T* const (&row)[NF], bool row_ok, int W, int k0, const double2* tab, f64x4_t (&re)[NF][2],
                                                f64x4_t (&im)[NF][2]) {
  const int c = threadIdx.x & 15, g = (threadIdx.x & 63) >> 4, Wh = W / 2 + 1;
  DftPhase ph[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) ph[t].init(k0 + 16 * t + c, 4 * g, 12, W);
  T v[NF][4], m[NF][4];                                  // kept in T: widened at the fold
  const auto fetch = [&](int kc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = kc + 4 * g + j;
      const bool ok = row_ok && x < Wh;
      const bool pair = ok && dft_has_mirror(W, x);      // W - x > x: every element of the row enters once
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        v[f][j] = ok ? row[f][x] : (T)0;
        m[f][j] = pair ? row[f][W - x] : (T)0;
      }
    }
  };
  fetch(0);
  for (int kc = 0; kc < Wh; kc += 16) {
    double e[NF][4], o[NF][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {                        // past the row v = m = 0: both sums get 0
      const bool pair = dft_has_mirror(W, kc + 4 * g + j);
#pragma unroll
      for (int f = 0; f < NF; ++f) dft_fold_pair(v[f][j], m[f][j], pair, e[f][j], o[f][j]);
    }
    fetch(kc + 16);                                      // past the row: every guard is false, nothing is read
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const double2 cs = tab[ph[t].idx];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          re[f][t] = mfma_f64_16x16x4(e[f][j], cs.x, re[f][t]);
          im[f][t] = mfma_f64_16x16x4(o[f][j], cs.y, im[f][t]);
        }
        ph[t].step(W);
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) ph[t].skip(W);
  }
}

// The inverse transform of the lane's row c onto the columns n0 + 16 t + c, t = 0 .. 3, of a row of W: acc[t] += the irfft sum over
// the bins 0 .. n_bins - 1.  bin(m) -> double2: bin m of the lane's row, zero beyond the row's bins.
template <typename Bin>
__device__ __forceinline__ void dft_rows_inverse(Bin bin, int n_bins, int W, int n0, const double2* tab, f64x4_t (&acc)[4]) {
  const int c = threadIdx.x & 15, g = (threadIdx.x & 63) >> 4;
  DftPhase ph[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) ph[t].init(n0 + 16 * t + c, 2 * g, 8, W);
  for (int m0 = 0; m0 < n_bins; m0 += 8) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {                        // the lane's two bins
      const int m = m0 + 2 * g + b;
      const double2 z = bin(m);
      const bool once = m == 0 || 2 * m == W;            // bin 0 and the Nyquist bin: weight 1, imaginary part ignored
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double2 cs = tab[b ? ph[t].ahead(W) : ph[t].idx];
        acc[t] = mfma_f64_16x16x4(z.x, once ? cs.x : 2.0 * cs.x, acc[t]);
        acc[t] = mfma_f64_16x16x4(z.y, once ? 0.0 : -2.0 * cs.y, acc[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) ph[t].skip(W);
  }
}

}  // namespace wx
