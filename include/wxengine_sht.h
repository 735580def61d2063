/*
 * wxengine -- C ABI of the spherical harmonic transforms (csrc/wx_sht.h), an extension of include/wxengine.h: the same library, the
 * same statuses and wx_last_error(), declared in a header of its own (INTEGRATION.md says why).
 *
 * credit/verification/standard.py::zonal_spectrum and div_rot_spectrum compute their spectra with torch_harmonics' RealSHT and
 * RealVectorSHT; here the transforms run on the device in fp64, a longitude DFT and a Legendre contraction on the matrix cores.
 * Pinned to the mathematics: only norm = "ortho" is taken, and the vector results are named spheroidal and toroidal.
 *
 * Unit sphere; row k at colatitude theta[k] strictly ascending in [0, pi] (north first), column j at 2 pi j / nlon; w[k] the
 * quadrature weights of int dx on [-1, 1].  Pbar_l^m: 2 pi int Pbar_l^m Pbar_l'^m sin(theta) dtheta = delta_ll', no
 * Condon-Shortley sign; csphase != 0 multiplies odd m by -1.
 *     analysis   F_m(k) = (2 pi / nlon) sum_j x[k][j] e^{-2 pi i m j / nlon},  c[l][m] = sum_k w[k] Pbar_l^m(theta[k]) F_m(k)
 *     synthesis  F_m(k) = sum_l Pbar_l^m(theta[k]) c[l][m],  x[k][j] = sum_m F_m(k) e^{+2 pi i m j / nlon} with irfft's Hermitian
 *                completion (the imaginary parts of m = 0 and of the Nyquist bin of an even nlon are ignored)
 *     vector     u east, v north; spheroidal s_lm = int u . conj(grad Y_lm) dOmega / sqrt(l (l + 1)),
 *                toroidal t_lm = int u . conj(rhat x grad Y_lm) dOmega / sqrt(l (l + 1)); row l = 0 is zero
 *     spectra    zonal[m] = sum_l mult_m |c_lm|^2, total[l] = sum_m mult_m |c_lm|^2, mult_0 = 1, else 2 (the Nyquist column too)
 * Coefficients: complex float64, (re, im) interleaved, [n_planes][lmax][mmax], contiguous; entries with l < m are written as zero.
 * dtype: 0 = float32, 1 = float64, of a field's planes.
 *
 *   wx_sht_create     theta_host, w_host: HOST arrays [nlat].  WX_ERR_INVALID with the reason: nlat or nlon < 2; nlon > 4096 (the
 *                     twiddle table lies in LDS); lmax < 1; mmax outside 1 .. min(lmax, nlon / 2 + 1); theta outside [0, pi] or not
 *                     strictly ascending; a weight that is not finite; norm other than "ortho".  Where theta[k] + theta[nlat-1-k] =
 *                     pi and w[k] = w[nlat-1-k] hold bit for bit, north and south rows are folded and the table is half the size.
 *                     No table is built here: the scalar table by the first wx_sht_analysis or wx_sht_synthesis, the two vector
 *                     tables by the first wx_sht_vector_analysis (on the host, then uploaded: that call waits for it); an
 *                     allocation that fails is WX_ERR_HIP with the byte count.
 *   wx_sht_analysis   plane p of x at x_dev + p * x_stride elements (stride >= nlat * nlon), [nlat][nlon] contiguous, read where it
 *                     lies; c_dev [n_planes][lmax][mmax][2] float64.
 *   wx_sht_synthesis  c_dev as above -> x_dev [n_planes][nlat][nlon] contiguous, float64 or float32 rounded once.
 *   wx_sht_vector_analysis   u and v as x above -> s_dev (spheroidal) and t_dev (toroidal), each as c_dev.
 *   wx_sht_spectra    c_dev -> zonal_dev [n_planes][mmax] and total_dev [n_planes][lmax] float64; either may be NULL, not both.
 *     Every call: WX_ERR_INVALID with the reason, nothing launched or written, for a null handle or pointer, n_planes < 1, an unknown
 *     dtype, a stride below nlat * nlon or one that takes the planes beyond 2^44 elements, an output that overlaps an input or another
 *     output.  Every sum has one fixed order and no atomics: a plane's results are bit-identical whatever n_planes, the split of the
 *     planes into calls and the plane's position.  The scratch is the handle's own: calls on one handle must be ordered by one stream.
 *   wx_sht_table      host only, needs no GPU: column m of table 0 (Pbar), 1 ((dPbar / dtheta) / sqrt(l (l + 1))) or 2
 *                     ((m Pbar / sin theta) / sqrt(l (l + 1))) as the handle builds it, out_host [lmax - m][nlat] float64 (row l - m);
 *                     folds_out (may be NULL; needs w_host) = 1 where a handle on this grid folds its rows, else 0.  w_host may be
 *                     NULL when folds_out is.
 */
#ifndef WXENGINE_SHT_H
#define WXENGINE_SHT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wx_sht* wx_sht_handle;
int wx_sht_create(int nlat, int nlon, int lmax, int mmax, const double* theta_host, const double* w_host, int csphase, const char* norm,
                  int device, wx_sht_handle* out);
int wx_sht_destroy(wx_sht_handle h);
int wx_sht_analysis(wx_sht_handle h, int n_planes, const void* x_dev, int64_t x_stride, int dtype, double* c_dev, void* stream);
int wx_sht_synthesis(wx_sht_handle h, int n_planes, const double* c_dev, void* x_dev, int dtype, void* stream);
int wx_sht_vector_analysis(wx_sht_handle h, int n_planes, const void* u_dev, int64_t u_stride, const void* v_dev, int64_t v_stride, int dtype,
                           double* s_dev, double* t_dev, void* stream);
int wx_sht_spectra(wx_sht_handle h, int n_planes, const double* c_dev, double* zonal_dev, double* total_dev, void* stream);
int wx_sht_table(int nlat, int lmax, int mmax, const double* theta_host, const double* w_host, int csphase, int table, int m,
                 double* out_host, int* folds_out);

#ifdef __cplusplus
}
#endif
#endif
