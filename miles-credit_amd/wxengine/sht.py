"""Spherical harmonic transforms on the device (csrc/wx_sht.h, C ABI in include/wxengine_sht.h): the spectrum of a field by total
wavenumber, and the rotational / divergent kinetic-energy spectra of a wind, without a copy to the host and without torch_harmonics.

The transforms of credit/verification/standard.py (zonal_spectrum, div_rot_spectrum and their averages): a longitude DFT and a
Legendre contraction, both fp64 on the matrix cores.  Pinned to the mathematics, not to torch_harmonics, which cannot be run next to
this code: only norm="ortho" is taken (the meaning of "backward" and "schmidt" cannot be checked here), and the two results of the
vector transform carry names, spheroidal and toroidal, not a slot index (which slot of RealVectorSHT is which cannot be checked either).

Unit sphere.  Row k has colatitude theta_k ascending (north first), column j has phi_j = 2 pi j / nlon.  Pbar_l^m is normalised so
that 2 pi int Pbar_l^m Pbar_l'^m sin(theta) dtheta = delta_ll'; csphase=True multiplies odd m by -1 (the Condon-Shortley sign).

    sht = SphericalHarmonics(nlat, nlon, grid="legendre-gauss")       # lmax = nlat, mmax = min(lmax, nlon // 2 + 1)
    c = sht.analysis(x)                    # complex128 [..., lmax, mmax]: c[l][m] = sum_k w_k Pbar_l^m(theta_k) F_m(k),
                                           #   F_m(k) = (2 pi / nlon) sum_j x[k][j] e^{-2 pi i m j / nlon}; zero where l < m
    x = sht.synthesis(c)                   # float64 [..., nlat, nlon] (dtype=torch.float32: the same, rounded once); Hermitian
                                           #   completion of irfft: imaginary parts of m = 0 and of the Nyquist bin are ignored
    s, t = sht.vector_analysis(u, v)       # u east, v north -> spheroidal s_lm = int u . conj(grad Y_lm) dOmega / sqrt(l (l + 1)),
                                           #   toroidal t_lm = int u . conj(rhat x grad Y_lm) dOmega / sqrt(l (l + 1)); row l = 0 is zero
    zonal, total = sht.spectra(c)          # float64 [..., mmax], [..., lmax]: sum_l mult_m |c_lm|^2, sum_m mult_m |c_lm|^2,
                                           #   mult_0 = 1 and 2 otherwise, the Nyquist column too (the reference's times_two)
    vort, div = sht.vorticity_divergence(s, t, radius)                # coefficients of the vorticity and the divergence

Fields are float32 or float64 device tensors [..., nlat, nlon]; the leading dimensions are planes, and a strided view is read where
it lies when its planes lie at one stride.  Everything stays on the device.  A plane's results are bit-identical whatever the number
of planes, the plane's position or the split into calls.

zonal_spectrum / div_rot_spectrum / average_zonal_spectrum / average_div_rot_spectrum mirror credit/verification/standard.py on device
tensors instead of xarray objects, with lmax = nlat + 1 as there; they share one cached transform per grid and device
(cached_transform, clear_cache).  On a Gauss grid the row l = nlat of m = 0 is then identically zero up to rounding: the nodes are
the roots of P_nlat.  That is the reference's own choice of lmax and is left as it is.

RealSHT and InverseRealSHT are thin callables with torch_harmonics' constructor signature, so reference-style code runs unchanged.
No CPU fallback: a transform raises without a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .native import HandleCache, WXEngineError, _check, _f64, _stream_ptr, require_gpu

MAX_NLON = 4096                 # kDftMaxN (csrc/wx_dft.h): the twiddle table lies in LDS
MAX_DEGREE = 32768
GRIDS = ("equiangular", "legendre-gauss")
NORM_REASON = ('only norm="ortho" is supported: the meaning of torch_harmonics\' "backward" and "schmidt" cannot be pinned without the '
               "library, and an unchecked normalisation would be a silent factor in every spectrum")


def grid_nodes(nlat: int, grid: str):
    """(theta [nlat], w [nlat]) float64: the colatitudes ascending (north first) and the quadrature weights of int dx on [-1, 1]
    -- the Gauss nodes and weights ("legendre-gauss"), or theta_k = pi k / (nlat - 1), poles included, with the Clenshaw-Curtis
    weights ("equiangular").  Both sets sum to 2.  The southern half is computed and the northern mirrored from it, theta_k = pi -
    theta_{nlat-1-k} (exact: pi / 2 <= theta <= pi) and w_k = w_{nlat-1-k}, so the symmetry the device fold tests holds bit for bit."""
    if isinstance(nlat, bool) or int(nlat) != nlat or nlat < 2:
        raise ValueError(f"grid_nodes: nlat must be an integer >= 2, got {nlat!r}")
    nlat = int(nlat)
    if grid == "legendre-gauss":
        x, w = np.polynomial.legendre.leggauss(nlat)
        theta = np.arccos(x[::-1])
        w = w[::-1].copy()
    elif grid == "equiangular":
        n = nlat - 1
        theta = np.pi * np.arange(nlat) / n
        j = np.arange(1, n // 2 + 1)
        b = np.where(2 * j == n, 1.0, 2.0)
        s = (b / (4.0 * j * j - 1.0) * np.cos(2.0 * np.outer(theta, j))).sum(axis=1)
        w = np.where((np.arange(nlat) == 0) | (np.arange(nlat) == n), 1.0, 2.0) / n * (1.0 - s)
    else:
        raise ValueError(f"grid_nodes: grid must be one of {GRIDS}, got {grid!r}")
    half = nlat // 2
    if nlat % 2:
        theta[half] = np.pi / 2
    for k in range(half):
        theta[k] = np.pi - theta[nlat - 1 - k]
        w[k] = w[nlat - 1 - k]
    return theta, w


def check_transform(nlat, nlon, lmax, mmax, grid, norm):
    """The constructor's checks, without a device: those of sht_check_create.  -> (nlat, nlon, lmax, mmax) as ints, defaults filled."""
    for name, v in (("nlat", nlat), ("nlon", nlon)):
        if isinstance(v, bool) or int(v) != v or v < 2:
            raise ValueError(f"SphericalHarmonics: {name} must be an integer >= 2, got {v!r}")
    nlat, nlon = int(nlat), int(nlon)
    if nlon > MAX_NLON:
        raise ValueError(f"SphericalHarmonics: nlon must be <= {MAX_NLON} (the twiddle table lies in LDS), got {nlon}")
    if norm != "ortho":
        raise ValueError(f"SphericalHarmonics: norm={norm!r}: {NORM_REASON}")
    if grid not in GRIDS:
        raise ValueError(f"SphericalHarmonics: grid must be one of {GRIDS}, got {grid!r}")
    lmax = nlat if lmax is None else lmax
    if isinstance(lmax, bool) or int(lmax) != lmax or not 1 <= lmax <= MAX_DEGREE:
        raise ValueError(f"SphericalHarmonics: lmax must be an integer in 1 .. {MAX_DEGREE}, got {lmax!r}")
    lmax = int(lmax)
    top = min(lmax, nlon // 2 + 1)
    mmax = top if mmax is None else mmax
    if isinstance(mmax, bool) or int(mmax) != mmax or not 1 <= mmax <= top:
        raise ValueError(f"SphericalHarmonics: mmax must be an integer in 1 .. min(lmax, nlon // 2 + 1) = {top}, got {mmax!r}")
    return nlat, nlon, lmax, int(mmax)


class SphericalHarmonics:
    def __init__(self, nlat, nlon, lmax=None, mmax=None, grid="equiangular", norm="ortho", csphase=True, device=None):
        self.nlat, self.nlon, self.lmax, self.mmax = check_transform(nlat, nlon, lmax, mmax, grid, norm)
        self.grid, self.norm, self.csphase = grid, norm, bool(csphase)
        self.theta, self.w = grid_nodes(self.nlat, grid)
        self._open(0 if device is None else device)

    @classmethod
    def borrowed(cls, handle, owner, lib, device, nlat, nlon, lmax, mmax, grid, csphase=False):
        """A transform over a native wx_sht handle that another object owns (`owner`, kept alive here; `handle` is never destroyed
        from this side): the pole filter's own transform.  `device` is a torch.device with an index."""
        self = cls.__new__(cls)
        self.nlat, self.nlon, self.lmax, self.mmax = check_transform(nlat, nlon, lmax, mmax, grid, "ortho")
        self.grid, self.norm, self.csphase = grid, "ortho", bool(csphase)
        self.theta, self.w = grid_nodes(self.nlat, grid)
        self.lib, self.device, self._handles, self._owner, self._h = lib, device, None, owner, handle
        return self

    def _open(self, device) -> None:
        import torch
        self.lib = require_gpu("the spherical harmonic transform has no CPU fallback", device)
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self._handles = HandleCache(self.lib, "wx_sht")
        self._h = self._handles.get(self.device.index, lambda: (self.nlat, self.nlon, self.lmax, self.mmax, _f64(self.theta), _f64(self.w),
                                                                int(self.csphase), self.norm.encode(), self.device.index))

    # ---- the planes of a tensor ----------------------------------------------------------------------------------------------------
    def _planes(self, x, name, shape, dtypes):
        """-> (tensor that keeps the memory alive, planes, plane stride in elements, leading shape) of x [..., *shape]."""
        import torch
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype in dtypes and x.dim() >= 2):
            raise WXEngineError(f"{name} must be a CUDA tensor [..., {shape[0]}, {shape[1]}] of dtype {' or '.join(str(d) for d in dtypes)}")
        if tuple(x.shape[-2:]) != shape or x.device != self.device:
            raise WXEngineError(f"{name}: expected [..., {shape[0]}, {shape[1]}] on {self.device}, got {tuple(x.shape)} on {x.device}")
        lead = tuple(x.shape[:-2])
        v = None
        if x.stride(-1) == 1 and x.stride(-2) == shape[1]:
            try:
                v = x.view(-1, *shape)                          # the planes of a view lie at one stride, or this raises
            except RuntimeError:
                v = None
        if v is None or (v.shape[0] > 1 and v.stride(0) < shape[0] * shape[1]):     # an expanded view: planes that share memory
            v = x.contiguous().view(-1, *shape)
        if v.shape[0] < 1:
            raise WXEngineError(f"{name} has no planes: shape {tuple(x.shape)}")
        return v, v.shape[0], (v.stride(0) if v.shape[0] > 1 else shape[0] * shape[1]), lead

    def _field(self, x, name):
        import torch
        v, P, stride, lead = self._planes(x, name, (self.nlat, self.nlon), (torch.float32, torch.float64))
        return v, P, stride, lead, (1 if v.dtype == torch.float64 else 0)

    def _coeffs(self, c, name):
        import torch
        v, P, _, lead = self._planes(c, name, (self.lmax, self.mmax), (torch.complex128,))
        return v.contiguous(), P, lead

    # ---- the transforms ------------------------------------------------------------------------------------------------------------
    def analysis(self, x):
        import torch
        v, P, stride, lead, dtype = self._field(x, "x")
        out = torch.empty(lead + (self.lmax, self.mmax), dtype=torch.complex128, device=self.device)
        with torch.cuda.device(self.device.index):
            _check(self.lib.wx_sht_analysis(self._h, P, C.c_void_p(v.data_ptr()), stride, dtype, C.c_void_p(out.data_ptr()),
                                            _stream_ptr(self.device.index)))
        return out

    def synthesis(self, c, dtype=None):
        import torch
        dtype = torch.float64 if dtype is None else dtype
        if dtype not in (torch.float32, torch.float64):
            raise ValueError(f"SphericalHarmonics.synthesis: dtype must be torch.float32 or torch.float64, got {dtype}")
        v, P, lead = self._coeffs(c, "c")
        out = torch.empty(lead + (self.nlat, self.nlon), dtype=dtype, device=self.device)
        with torch.cuda.device(self.device.index):
            _check(self.lib.wx_sht_synthesis(self._h, P, C.c_void_p(v.data_ptr()), C.c_void_p(out.data_ptr()), 1 if dtype == torch.float64 else 0,
                                             _stream_ptr(self.device.index)))
        return out

    def vector_analysis(self, u, v):
        """(spheroidal, toroidal) of the wind u (east), v (north): complex128 [..., lmax, mmax] each."""
        import torch
        a, P, a_stride, lead, dtype = self._field(u, "u")
        b, Pb, b_stride, lead_b, dtype_b = self._field(v, "v")
        if lead != lead_b or dtype != dtype_b:
            raise WXEngineError(f"u {tuple(u.shape)} {u.dtype} and v {tuple(v.shape)} {v.dtype} must be one shape and dtype")
        s = torch.empty(lead + (self.lmax, self.mmax), dtype=torch.complex128, device=self.device)
        t = torch.empty_like(s)
        with torch.cuda.device(self.device.index):
            _check(self.lib.wx_sht_vector_analysis(self._h, P, C.c_void_p(a.data_ptr()), a_stride, C.c_void_p(b.data_ptr()), b_stride, dtype,
                                                   C.c_void_p(s.data_ptr()), C.c_void_p(t.data_ptr()), _stream_ptr(self.device.index)))
        return s, t

    def vector_synthesis(self, s, t=None, dtype=None, components="uv"):
        """(u east, v north) [..., nlat, nlon] from the spheroidal s and toroidal t coefficients: F_theta = sum_l dPt s - i Qt t,
        F_phi = sum_l i Qt s + dPt t, u = lon_synth(F_phi), v = -lon_synth(F_theta), the longitude synthesis of `synthesis`.
        t=None: no toroidal part (the gradient form, half the work).  components "u" or "v": that component alone (the other is None)."""
        import torch
        dtype = torch.float64 if dtype is None else dtype
        if dtype not in (torch.float32, torch.float64):
            raise ValueError(f"SphericalHarmonics.vector_synthesis: dtype must be torch.float32 or torch.float64, got {dtype}")
        if components not in ("uv", "u", "v"):
            raise ValueError(f"SphericalHarmonics.vector_synthesis: components must be 'uv', 'u' or 'v', got {components!r}")
        a, P, lead = self._coeffs(s, "s")
        b = None
        if t is not None:
            b, Pb, lead_b = self._coeffs(t, "t")
            if lead != lead_b:
                raise WXEngineError(f"s {tuple(s.shape)} and t {tuple(t.shape)} must be one shape")
        u = torch.empty(lead + (self.nlat, self.nlon), dtype=dtype, device=self.device) if "u" in components else None
        v = torch.empty(lead + (self.nlat, self.nlon), dtype=dtype, device=self.device) if "v" in components else None
        ptr = lambda x: C.c_void_p(None if x is None else x.data_ptr())      # noqa: E731
        with torch.cuda.device(self.device.index):
            _check(self.lib.wx_sht_vector_synthesis(self._h, P, ptr(a), ptr(b), ptr(u), ptr(v), 1 if dtype == torch.float64 else 0,
                                                    _stream_ptr(self.device.index)))
        return u, v

    def spectra(self, c):
        """(zonal [..., mmax], total [..., lmax]) float64 of the coefficients c."""
        import torch
        v, P, lead = self._coeffs(c, "c")
        zonal = torch.empty(lead + (self.mmax,), dtype=torch.float64, device=self.device)
        total = torch.empty(lead + (self.lmax,), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device.index):
            _check(self.lib.wx_sht_spectra(self._h, P, C.c_void_p(v.data_ptr()), C.c_void_p(zonal.data_ptr()), C.c_void_p(total.data_ptr()),
                                           _stream_ptr(self.device.index)))
        return zonal, total

    def vorticity_divergence(self, s, t, radius: float = 1.0):
        """(vorticity, divergence) coefficients of a wind on a sphere of `radius` from its (spheroidal, toroidal) coefficients:
        with u = grad chi + rhat x grad psi, s_lm = sqrt(l (l + 1)) chi_lm and the divergence is lap chi = -l (l + 1) chi / a^2 per
        mode, so div_lm = -sqrt(l (l + 1)) s_lm / a for a wind given on the sphere of radius a; the vorticity likewise from t."""
        import torch
        l = torch.arange(self.lmax, dtype=torch.float64, device=s.device)
        f = (-torch.sqrt(l * (l + 1.0)) / float(radius)).reshape(-1, 1)
        return f * t, f * s


_transforms = {}


def cached_transform(nlat, nlon, grid, norm="ortho", device=None) -> SphericalHarmonics:
    """The one SphericalHarmonics behind zonal_spectrum, div_rot_spectrum and their averages on a grid and a device: lmax = nlat + 1
    and csphase off as in credit/verification/standard.py's vector transform (the sign cancels in every spectrum, so the scalar
    spectra share the handle).  It is kept until clear_cache(): its tables are built by the first call that needs them and stay on
    the device -- at 721 x 1440 0.75 GB for the scalar table and 1.5 GB for the two vector tables."""
    key = (int(nlat), int(nlon), grid, norm, str(device))
    if key not in _transforms:
        _transforms[key] = SphericalHarmonics(nlat, nlon, lmax=int(nlat) + 1, grid=grid, norm=norm, csphase=False, device=device)
    return _transforms[key]


def clear_cache() -> None:
    """Drops the transforms that the module's functions keep; their device memory goes with the last reference."""
    _transforms.clear()


class _Callable:
    """torch_harmonics' constructor signature over one SphericalHarmonics, opened by the first call on the tensor's device."""

    def __init__(self, nlat, nlon, lmax=None, mmax=None, grid="equiangular", norm="ortho", csphase=True):
        self.nlat, self.nlon, self.lmax, self.mmax = check_transform(nlat, nlon, lmax, mmax, grid, norm)
        self.grid, self.norm, self.csphase = grid, norm, csphase
        self._sht = None

    def _on(self, x) -> SphericalHarmonics:
        if self._sht is None or self._sht.device != getattr(x, "device", None):
            device = x.device if getattr(x, "is_cuda", False) else None
            self._sht = SphericalHarmonics(self.nlat, self.nlon, self.lmax, self.mmax, self.grid, self.norm, self.csphase, device=device)
        return self._sht


class RealSHT(_Callable):
    def __call__(self, x):
        return self._on(x).analysis(x)

    forward = __call__


class InverseRealSHT(_Callable):
    def __call__(self, c):
        return self._on(c).synthesis(c)

    forward = __call__


def _grid_of(x, name):
    import torch
    if not (isinstance(x, torch.Tensor) and x.dim() >= 2):
        raise WXEngineError(f"{name} must be a tensor [..., nlat, nlon]")
    if not x.is_cuda:
        require_gpu("the spherical harmonic transform has no CPU fallback", x.device)
    return int(x.shape[-2]), int(x.shape[-1])


def zonal_spectrum(field, grid, norm="ortho"):
    """credit/verification/standard.py::zonal_spectrum of a device tensor [..., nlat, nlon]: float64 [..., mmax] on the device,
    sum_l mult_m |c_lm|^2 with lmax = nlat + 1."""
    nlat, nlon = _grid_of(field, "field")
    sht = cached_transform(nlat, nlon, grid, norm, field.device)
    return sht.spectra(sht.analysis(field))[0]


def average_zonal_spectrum(field, grid, norm="ortho"):
    """The mean of zonal_spectrum over the planes: numpy [mmax]."""
    z = zonal_spectrum(field, grid, norm)
    return z.reshape(-1, z.shape[-1]).mean(dim=0).cpu().numpy()


def div_rot_spectrum(u, v, grid, norm="ortho"):
    """credit/verification/standard.py::div_rot_spectrum of a wind (u east, v north): (rotational, divergent) = the (toroidal,
    spheroidal) coefficients, complex128 [..., lmax, mmax] with lmax = nlat + 1, csphase off as there."""
    nlat, nlon = _grid_of(u, "u")
    sht = cached_transform(nlat, nlon, grid, norm, u.device)
    s, t = sht.vector_analysis(u, v)
    return t, s


def average_div_rot_spectrum(u, v, grid, wave_spec="n", norm="ortho"):
    """(rotational, divergent) kinetic-energy spectra averaged over the planes, numpy: by total wavenumber (wave_spec="n": the sum
    over m) or, for anything else, by zonal wavenumber (the sum over l)."""
    nlat, nlon = _grid_of(u, "u")
    sht = cached_transform(nlat, nlon, grid, norm, u.device)
    s, t = sht.vector_analysis(u, v)
    i = 1 if wave_spec == "n" else 0
    out = []
    for c in (t, s):
        spec = sht.spectra(c)[i]
        out.append(spec.reshape(-1, spec.shape[-1]).mean(dim=0).cpu().numpy())
    return out[0], out[1]
