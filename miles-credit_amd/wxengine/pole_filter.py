"""The diffusion and pole filter of credit/pol_lapdiff_filt.py on the device (csrc/wx_polefilter.h, C ABI in
include/wxengine_polefilter.h): conf["predict"]["use_laplace_filter"]'s post-processing of a forecast step, without a copy to the
host and without torch_harmonics.

    dpf = Diffusion_and_Pole_Filter(nlat, nlon, device="cuda")       # the reference's name, argument order and defaults
    y = dpf.diff_lap2d_filt(x)                                       # x [C >= 70, nlat, nlon] in the reference's channel layout
    T = dpf.polefilt_lap2d_V1(T, substeps=5);  Q = dpf.polefilt_lap2d_QV1(Q, 8);  U, V = dpf.polefilt_lap2d_V2(U, V, 6)
    D = dpf.polfiltT(D)                                              # the polar zonal low-pass alone (NOT in place: a new tensor)

Pinned to the mathematics, as the transforms are: norm "ortho", csphase off, lmax = nlat and mmax = min(lmax, nlon // 2
+ 1) where not given, u east and v north.  With A the scalar analysis and grad(c) the vector synthesis of sqrt(l (l + 1)) c / radius
with no toroidal part, L(x) = grad(A(g_x))_x + grad(A(g_y))_y, (g_x, g_y) = grad(A(x)) -- not the spectral Laplacian --
    V1 / QV1   x = polfiltT(x); substeps times x += 1e8 (0.5e8) sig[k] L(x)
    V2         U, V = polfiltT(U), polfiltT(V); substeps times (l_x, l_y) = grad(A(L(d))), d = div(U, V) read as coefficients;
               U -= 2e16 sig[k] l_x, V -= 2e16 sig[k] l_y
sig is the reference's create_sigmoid_ramp_function(nlat, 10), the low-pass filters rows 1 .. 10 and nlat - 10 .. nlat - 1 (row 0
stays, the last row is filtered: the reference's index list) and keeps the zonal modes below the cutoff index whole and the mode
at it at half weight.  Everything between input and output is fp64 (the reference's 3-D getgrad casts to complex64).

Fields are float32 or float64 CUDA tensors [nlat, nlon] or [P, nlat, nlon]; a strided view is read where it lies.  The results are
new tensors of the input's dtype, as in the reference (it clones).  No CPU fallback: construction raises without a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .native import NativeHandle, WXEngineError, _check, _f32, _f64, _stream_ptr, require_gpu
from .sht import SphericalHarmonics, check_transform, grid_nodes

INDPOL = 10                      # the reference's self.indpol: the rows of a polar band and the length of the ramp
MIN_NLAT = 2 * INDPOL + 1
PERIOD = 100                     # the reference's find_nearest(perd, value=100)
COEF_V1, COEF_QV1, COEF_V2 = 1e8, 0.5e8, 2e16
LAYOUT_CHANNELS = 70


def create_sigmoid_ramp_function(array_length: int, ramp_length: int) -> np.ndarray:
    """credit/pol_lapdiff_filt.py::create_sigmoid_ramp_function, float32 [array_length], by the reference's own float32 torch CPU
    operations (bit-identical)."""
    import torch
    array = torch.ones(array_length)
    sigmoid = 1 / (1 + torch.exp(-torch.linspace(-6, 6, ramp_length)))
    array[:ramp_length] = sigmoid
    array[array_length - ramp_length:] = torch.flip(sigmoid, dims=(0,))
    return array.numpy()


def cutoff_index(nlon: int) -> int:
    """The index i of polfiltT at nlon columns: argmin |1 / rfftfreq(nlon)[1:] - 100| in float32, the first minimum, by the
    reference's own torch operations.  The low-pass zeroes Z[i : nlon - i] of the full FFT."""
    import torch
    perd = 1 / torch.fft.rfftfreq(int(nlon))[1:]
    return int(torch.abs(perd - PERIOD).argmin())


def check_filter(nlat, nlon, lmax, mmax, grid, radius):
    """The constructor's checks, without a device.  -> (nlat, nlon, lmax, mmax, radius)"""
    nlat, nlon, lmax, mmax = check_transform(nlat, nlon, lmax, mmax, grid, "ortho")
    if nlat < MIN_NLAT:
        raise ValueError(f"Diffusion_and_Pole_Filter: nlat must be >= {MIN_NLAT}, got {nlat}: the polar bands of the low-pass (rows 1 .. {INDPOL} "
                         f"and nlat - {INDPOL} .. nlat - 1) would overlap, and the low-pass with its half-weight mode is not idempotent")
    radius = float(radius)
    if not (np.isfinite(radius) and radius > 0):
        raise ValueError(f"Diffusion_and_Pole_Filter: radius must be finite and > 0, got {radius!r}")
    return nlat, nlon, lmax, mmax, radius


class Diffusion_and_Pole_Filter:
    def __init__(self, nlat, nlon, device="cuda", lmax=None, mmax=None, grid="legendre-gauss", radius=6.37122e6, omega=7.292e-5,
                 gravity=9.80616, havg=10.0e3, hamp=120.0):
        self.nlat, self.nlon, self.lmax, self.mmax, self.radius = check_filter(nlat, nlon, lmax, mmax, grid, radius)
        self.grid, self.omega, self.gravity, self.havg, self.hamp = grid, omega, gravity, havg, hamp
        self.indpol = INDPOL
        self.sigmoid = create_sigmoid_ramp_function(self.nlat, self.indpol)
        self.cutoff = cutoff_index(self.nlon)
        self.theta, self.w = grid_nodes(self.nlat, grid)
        self._open(device)

    def _open(self, device) -> None:
        import torch
        self.lib = require_gpu("the diffusion and pole filter has no CPU fallback", device)
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self._h = NativeHandle(self.lib.wx_polefilter_destroy)
        _check(self.lib.wx_polefilter_create(self.nlat, self.nlon, self.lmax, self.mmax, _f64(self.theta), _f64(self.w), self.radius, self.indpol,
                                             self.cutoff, _f32(self.sigmoid), self.device.index, self._h.out))
        # the handle's own transform, borrowed: it lives as long as self._h and is never destroyed from here
        h = C.c_void_p()
        _check(self.lib.wx_polefilter_sht(self._h, C.byref(h)))
        self.sht = SphericalHarmonics.borrowed(h, self._h, self.lib, self.device, self.nlat, self.nlon, self.lmax, self.mmax, self.grid)

    def workspace_bytes(self, n_planes: int) -> int:
        """The work memory of a call on n_planes planes (fields, coefficients, the transform's scratch; not its tables)."""
        out = C.c_int64()
        _check(self.lib.wx_polefilter_workspace(self.nlat, self.nlon, self.lmax, self.mmax, int(n_planes), C.byref(out)))
        return out.value

    # ---- the reference's methods -----------------------------------------------------------------------------------------------
    def grid2spec(self, ugrid):
        return self.sht.analysis(ugrid)

    def spec2grid(self, uspec):
        return self.sht.synthesis(uspec)

    def getgrad(self, chispec):
        """(g_x east, g_y north) float64 [..., nlat, nlon]: the gradient on the sphere of `radius` of the coefficients chispec."""
        import torch
        v, P, lead = self.sht._coeffs(chispec, "chispec")
        gx = torch.empty(lead + (self.nlat, self.nlon), dtype=torch.float64, device=self.device)
        gy = torch.empty_like(gx)
        with torch.cuda.device(self.device.index):
            _check(self.lib.wx_polefilter_gradient(self._h, P, C.c_void_p(v.data_ptr()), C.c_void_p(gx.data_ptr()), C.c_void_p(gy.data_ptr()), 1,
                                                   _stream_ptr(self.device.index)))
        return gx, gy

    def _field(self, x, name):
        if getattr(x, "dim", lambda: 0)() not in (2, 3):
            raise WXEngineError(f"{name} must be a CUDA tensor [nlat, nlon] or [P, nlat, nlon] of dtype torch.float32 or torch.float64")
        return self.sht._field(x, name)

    def _scalar(self, T, substeps, coef, name="T", inplace=False):
        """substeps None: the low-pass alone, through its own entry point."""
        import torch
        v, P, stride, lead, dtype = self._field(T, name)
        substeps = None if substeps is None else int(substeps)
        if substeps is not None and substeps < 0:
            raise ValueError(f"Diffusion_and_Pole_Filter: substeps must be >= 0, got {substeps}")
        if inplace:                                           # where the planes lie
            out, o, o_stride = T, v, stride
        else:
            out = o = torch.empty(lead + (self.nlat, self.nlon), dtype=v.dtype, device=self.device)
            o_stride = self.nlat * self.nlon
        with torch.cuda.device(self.device.index):
            if substeps is None:
                _check(self.lib.wx_polefilter_lowpass(self._h, P, C.c_void_p(v.data_ptr()), stride, dtype, C.c_void_p(o.data_ptr()), o_stride,
                                                      _stream_ptr(self.device.index)))
            else:
                _check(self.lib.wx_polefilter_scalar(self._h, P, C.c_void_p(v.data_ptr()), stride, dtype, substeps, coef, C.c_void_p(o.data_ptr()),
                                                     o_stride, _stream_ptr(self.device.index)))
        if o is v and v.data_ptr() != T.data_ptr():
            T.copy_(v.view(T.shape))                          # _field made a contiguous copy: bring the result home
        return out

    def _vector(self, U, V, substeps, coef, inplace=False):
        import torch
        a, P, a_stride, lead, dtype = self._field(U, "U")
        b, Pb, b_stride, lead_b, dtype_b = self._field(V, "V")
        if lead != lead_b or dtype != dtype_b:
            raise WXEngineError(f"U {tuple(U.shape)} {U.dtype} and V {tuple(V.shape)} {V.dtype} must be one shape and dtype")
        substeps = int(substeps)
        if substeps < 0:
            raise ValueError(f"Diffusion_and_Pole_Filter: substeps must be >= 0, got {substeps}")
        hw = self.nlat * self.nlon
        if inplace:
            uo, vo, uo_stride, vo_stride = a, b, a_stride, b_stride
        else:
            uo = torch.empty(lead + (self.nlat, self.nlon), dtype=a.dtype, device=self.device)
            vo = torch.empty_like(uo)
            uo_stride = vo_stride = hw
        with torch.cuda.device(self.device.index):
            _check(self.lib.wx_polefilter_vector(self._h, P, C.c_void_p(a.data_ptr()), a_stride, C.c_void_p(b.data_ptr()), b_stride, dtype, substeps,
                                                 coef, C.c_void_p(uo.data_ptr()), uo_stride, C.c_void_p(vo.data_ptr()), vo_stride,
                                                 _stream_ptr(self.device.index)))
        if inplace:
            for src, dst in ((a, U), (b, V)):
                if src.data_ptr() != dst.data_ptr():
                    dst.copy_(src.view(dst.shape))
        return uo, vo

    def polfiltT(self, D, inddo=None):
        """The polar zonal low-pass of D, a new tensor (the reference's function filters its argument in place and returns it)."""
        if inddo is not None and int(inddo) != self.indpol:
            raise ValueError(f"Diffusion_and_Pole_Filter.polfiltT: the handle filters {self.indpol} rows per band, got inddo={inddo}")
        return self._scalar(D, None, 0.0, "D")

    def polefilt_lap2d_V1(self, T, substeps):
        return self._scalar(T, substeps, COEF_V1)

    def polefilt_lap2d_QV1(self, T, substeps):
        return self._scalar(T, substeps, COEF_QV1)

    def polefilt_lap2d_V2(self, U, V, substeps):
        return self._vector(U, V, substeps, COEF_V2)

    def diff_lap2d_filt(self, BB2_tensor, out=None):
        """The reference's hard-coded layout on [C >= 70, nlat, nlon]: channels 0:16 (U) with 16:32 (V) V2 x 6, 32:48 V1 x 5, 48:64 QV1 x 8,
        64, 65 and 68 V1 x 5, 67 (U) with 66 (V) V2 x 6, 69 QV1 x 4; the rest is copied.  A new tensor, or `out` (which may be the input:
        every filter then runs in place)."""
        import torch
        x = BB2_tensor
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype in (torch.float32, torch.float64) and x.dim() == 3):
            raise WXEngineError("diff_lap2d_filt: the input must be a CUDA tensor [C, nlat, nlon] of dtype torch.float32 or torch.float64")
        if x.shape[0] < LAYOUT_CHANNELS:
            raise WXEngineError(f"diff_lap2d_filt: the reference's channel layout needs at least {LAYOUT_CHANNELS} channels, got {x.shape[0]}")
        if tuple(x.shape[1:]) != (self.nlat, self.nlon) or x.device != self.device:
            raise WXEngineError(f"diff_lap2d_filt: expected [C, {self.nlat}, {self.nlon}] on {self.device}, got {tuple(x.shape)} on {x.device}")
        if out is None:
            out = x.clone()
        else:
            if not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != x.dtype or out.device != x.device:
                raise WXEngineError("diff_lap2d_filt: out must have the input's shape, dtype and device")
            if out.data_ptr() != x.data_ptr() or out.stride() != x.stride():
                out.copy_(x)
        self._vector(out[0:16], out[16:32], 6, COEF_V2, inplace=True)
        self._scalar(out[32:48], 5, COEF_V1, inplace=True)
        self._scalar(out[48:64], 8, COEF_QV1, inplace=True)
        self._scalar(out[64:66], 5, COEF_V1, inplace=True)
        self._vector(out[67:68], out[66:67], 6, COEF_V2, inplace=True)
        self._scalar(out[68:69], 5, COEF_V1, inplace=True)
        self._scalar(out[69:70], 4, COEF_QV1, inplace=True)
        return out
