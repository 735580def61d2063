/*
 * wxengine -- C ABI of the inverse vector spherical harmonic transform and of the diffusion and pole filter
 * (csrc/wx_sht.h, csrc/wx_polefilter.h), a second extension of include/wxengine.h: the same library, the same statuses and
 * wx_last_error().  It builds on include/wxengine_sht.h, whose definitions and layouts it shares.
 *
 * credit/pol_lapdiff_filt.py::Diffusion_and_Pole_Filter, which conf["predict"]["use_laplace_filter"] applies to every step's
 * prediction, runs on torch_harmonics; here the whole filter runs on the device in fp64.  Pinned to the mathematics: norm "ortho",
 * csphase off, u east and v north, the vector coefficients named spheroidal and toroidal.
 *
 *     vector synthesis   F_theta,m(k) = sum_l dPt s_lm - i Qt t_lm,  F_phi,m(k) = sum_l i Qt s_lm + dPt t_lm,
 *                        u = lon_synth(F_phi), v = -lon_synth(F_theta), the longitude synthesis of wx_sht_synthesis; row l = 0
 *                        contributes nothing.  dPt = (dPbar / dtheta) / sqrt(l (l + 1)), Qt = (m Pbar / sin theta) / sqrt(l (l + 1)).
 *     A(x)               wx_sht_analysis;  grad(c) = vector synthesis of s = sqrt(l (l + 1)) c / radius, t = 0: (g_x east, g_y north)
 *     div(U, V)          -sqrt(l (l + 1)) s_lm / radius, s the spheroidal coefficients of wx_sht_vector_analysis(U, V)
 *     L(x)               grad(A(g_x))_x + grad(A(g_y))_y with (g_x, g_y) = grad(A(x)) -- not the spectral Laplacian
 *     low-pass           rows 1 .. indpol and nlat - indpol .. nlat - 1 (row 0 stays, the last row is filtered); with N = nlon and
 *                        i = cutoff_index: y_j = A_0 / N + (2 / N) sum_{k=1}^{i-1} (A_k cos + B_k sin) + (1 / N) (A_i cos + B_i sin),
 *                        A_k = sum_j x_j cos(2 pi k j / N), B_k likewise with sin: mode i passes at half weight.  i = 0: no row changes.
 *     scalar filter      x = low-pass(x); substeps times x += coef sig[k] L(x)
 *     vector filter      U, V = low-pass(U), low-pass(V); substeps times (l_x, l_y) = grad(A(L(d))), d = div(U, V) read as
 *                        coefficients; U -= coef sig[k] l_x, V -= coef sig[k] l_y
 * polefilt_lap2d_V1 is the scalar filter with coef 1e8, polefilt_lap2d_QV1 with 0.5e8, polefilt_lap2d_V2 the vector filter with 2e16.
 *
 *   wx_sht_vector_synthesis  s_dev (spheroidal), t_dev (toroidal; NULL: the gradient form, half the work), each [n_planes][lmax][mmax][2]
 *                     float64 -> u_dev, v_dev [n_planes][nlat][nlon] contiguous, float64 or float32 rounded once; one of u_dev, v_dev
 *                     may be NULL (that component is not computed).  The two vector tables are built by the first call that needs them.
 *   wx_polefilter_create   theta_host, w_host [nlat] as wx_sht_create (csphase 0, norm "ortho"); sig_host [nlat] float32: the ramp
 *                     sig[k].  WX_ERR_INVALID with the reason for what wx_sht_create refuses and for nlat < 2 indpol + 1 (the polar bands
 *                     would overlap), indpol < 0, cutoff_index outside 0 .. nlon / 2, a radius that is not finite and > 0, a ramp
 *                     weight that is not finite.  The handle owns one wx_sht handle and its work fields.
 *   wx_polefilter_sht      the handle's own transform, for wx_sht_analysis and the other calls of include/wxengine_sht.h; it lives as
 *                     long as the filter and must not be destroyed.
 *   wx_polefilter_lowpass, wx_polefilter_scalar, wx_polefilter_vector   plane p of a field at ptr + p * stride elements (stride >=
 *                     nlat * nlon), read and written where it lies.  substeps = 0 is the low-pass alone.  An output may be its own
 *                     input (the same address and stride).
 *   wx_polefilter_gradient  grad(c_dev) -> gx_dev, gy_dev [n_planes][nlat][nlon] contiguous.
 *   wx_polefilter_workspace  host only: the bytes of work memory (fields, coefficients, the transform's scratch; not its tables) of a
 *                     call on n_planes planes.  A call processes its planes in chunks of 16, so the figure does not grow beyond 16.
 *     Every call: WX_ERR_INVALID with the reason, nothing launched or written, for a null handle or pointer, n_planes < 1, an unknown
 *     dtype, a stride below nlat * nlon or one that takes the planes beyond 2^44 elements, substeps < 0, a coef that is not finite, an
 *     output that overlaps another output or an input that is not its own.  A call runs on `stream` without a host sync; every sum has
 *     one fixed order and no atomics, and a plane's result is bit-identical whatever n_planes and the plane's position.  The work
 *     fields are the handle's own: calls on one handle must be ordered by one stream.
 */
#ifndef WXENGINE_POLEFILTER_H
#define WXENGINE_POLEFILTER_H

#include <stdint.h>

#include "wxengine_sht.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wx_polefilter* wx_polefilter_handle;
int wx_sht_vector_synthesis(wx_sht_handle h, int n_planes, const double* s_dev, const double* t_dev, void* u_dev, void* v_dev, int dtype,
                            void* stream);
int wx_polefilter_create(int nlat, int nlon, int lmax, int mmax, const double* theta_host, const double* w_host, double radius, int indpol,
                         int cutoff_index, const float* sig_host, int device, wx_polefilter_handle* out);
int wx_polefilter_destroy(wx_polefilter_handle h);
int wx_polefilter_sht(wx_polefilter_handle h, wx_sht_handle* out);
int wx_polefilter_lowpass(wx_polefilter_handle h, int n_planes, const void* x_dev, int64_t x_stride, int dtype, void* out_dev, int64_t out_stride,
                          void* stream);
int wx_polefilter_scalar(wx_polefilter_handle h, int n_planes, const void* x_dev, int64_t x_stride, int dtype, int substeps, double coef,
                         void* out_dev, int64_t out_stride, void* stream);
int wx_polefilter_vector(wx_polefilter_handle h, int n_planes, const void* u_dev, int64_t u_stride, const void* v_dev, int64_t v_stride, int dtype,
                         int substeps, double coef, void* u_out_dev, int64_t u_out_stride, void* v_out_dev, int64_t v_out_stride, void* stream);
int wx_polefilter_gradient(wx_polefilter_handle h, int n_planes, const double* c_dev, void* gx_dev, void* gy_dev, int dtype, void* stream);
int wx_polefilter_workspace(int nlat, int nlon, int lmax, int mmax, int n_planes, int64_t* bytes_out);

#ifdef __cplusplus
}
#endif
#endif
