"""The wind artifact filter of the gen-2 post-block chain on the device (credit/postblock/wind_filter.py, csrc/wx_wind.h).

`WindArtifactFilter` takes the reference's argument names and defaults and is a callable on the batch dict like the other post blocks:
    run_forecast(..., step_postblocks=[WindArtifactFilter(u, v, [u, v, T, q], ...), InverseScale(mean, std), ...])
Per call: a blend mask m in [0, 1] from the wind speed at `mask_level` (flag > speed_threshold, rectangular dilation, Gaussian
falloff), then every level of `target_levels` of every variable of `target_vars` becomes m * smooth(f) + (1 - m) * f, the smoothed
field rescaled to the mask-weighted RMS of the original when `preserve_amplitude`.  At most four launches, whatever the number of
variables and levels.  The variables are read where they lie (the channel slices `Reconstruct` hands out) and the dict entries are
rebound to fresh [B, L, 1, H, W] tensors: the inputs are never modified.

UNIT-SENSITIVE, as the reference's docstring warns: the block does no scaling, `speed_threshold` is compared with whatever units U and V
have at the block's position in the chain.  The default is tuned for NORMALISED output: put the block before the inverse scale.

The 1-D Gaussian weights are computed here with the reference's float32 torch expressions (`filter_kernels`) and uploaded once per
(H, W, device).  Supported range, checked at construction: odd dilation sizes, every kernel at most 33 along latitude and 65 along
longitude (falloff_sigma <= 8; smoothing sigma <= 5.33 meridional, <= 10.66 zonal).  No CPU fallback: construction raises without a GPU.
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import Dict, Optional, Sequence

import numpy as np

from .conservation import _pred, _set_pred
from .native import (HandleCache, WXEngineError, _check, _f32, _i32, _named_tensor_args, _stream_ptr, batch_stride, check_named_tensor,
                     require_gpu)

logger = logging.getLogger(__name__)

MAX_KERNEL_LAT, MAX_KERNEL_LON = 33, 65      # kWindMaxKLat, kWindMaxKLon
MAX_VARIABLES, MAX_LEVELS = 32, 256          # kWindMaxVars, kWindMaxLevels


def _gauss1d(sigma: float, size: int):
    """wind_filter.py:54-56 / :74-78: exp(-0.5 (x / sigma)^2) / sum, float32, torch on the CPU."""
    import torch
    x = torch.arange(size, dtype=torch.float32) - size // 2
    g = torch.exp(-0.5 * (x / sigma) ** 2)
    return (g / g.sum()).numpy()


def kernel_sizes(smooth_sigma: float = 1.0, smooth_sigma_zonal: Optional[float] = None, smooth_sigma_meridional: Optional[float] = None,
                 falloff_sigma: float = 4.0) -> Dict[str, int]:
    """Sizes of the four 1-D kernels (wind_filter.py:51-52, :75)."""
    sig_lat = smooth_sigma if smooth_sigma_meridional is None else smooth_sigma_meridional
    sig_lon = smooth_sigma if smooth_sigma_zonal is None else smooth_sigma_zonal
    return {"smooth_lat": int(2 * sig_lat * 3 + 1) | 1, "smooth_lon": int(2 * sig_lon * 3 + 1) | 1,
            "falloff_lat": int(2 * falloff_sigma * 2 + 1) | 1, "falloff_lon": int(2 * falloff_sigma * 4 + 1) | 1}


def filter_kernels(smooth_sigma: float = 1.0, smooth_sigma_zonal: Optional[float] = None, smooth_sigma_meridional: Optional[float] = None,
                   falloff_sigma: float = 4.0) -> Dict[str, np.ndarray]:
    """The four normalised 1-D Gaussians the device convolves with; the longitude falloff has sigma 2 * falloff_sigma (:59)."""
    n = kernel_sizes(smooth_sigma, smooth_sigma_zonal, smooth_sigma_meridional, falloff_sigma)
    sig_lat = smooth_sigma if smooth_sigma_meridional is None else smooth_sigma_meridional
    sig_lon = smooth_sigma if smooth_sigma_zonal is None else smooth_sigma_zonal
    return {"smooth_lat": _gauss1d(sig_lat, n["smooth_lat"]), "smooth_lon": _gauss1d(sig_lon, n["smooth_lon"]),
            "falloff_lat": _gauss1d(falloff_sigma, n["falloff_lat"]), "falloff_lon": _gauss1d(falloff_sigma * 2, n["falloff_lon"])}


class WindArtifactFilter:
    """credit/postblock/wind_filter.py::WindArtifactFilter on the device.  `return_mask=True` also leaves the blend mask
    [B, 1, H, W] of the last call in `self.last_mask`."""

    def __init__(self, u_var: str, v_var: str, target_vars: Sequence[str], mask_level: int = 14,
                 target_levels: Sequence[int] = tuple(range(9, 21)), speed_threshold: float = 3.0193274566643846,
                 smooth_sigma: float = 1.0, smooth_sigma_zonal: Optional[float] = None, smooth_sigma_meridional: Optional[float] = None,
                 dilation_zonal: int = 13, dilation_meridional: int = 5, falloff_sigma: float = 4.0, preserve_amplitude: bool = False,
                 return_mask: bool = False):
        self.u_var, self.v_var = u_var, v_var
        self.target_vars = list(target_vars)
        self.mask_level = int(mask_level)
        self.target_levels = set(int(l) for l in target_levels)
        self.speed_threshold = float(speed_threshold)
        self.smooth_sigma, self.smooth_sigma_zonal, self.smooth_sigma_meridional = smooth_sigma, smooth_sigma_zonal, smooth_sigma_meridional
        self.dilation_zonal, self.dilation_meridional = int(dilation_zonal), int(dilation_meridional)
        self.falloff_sigma = falloff_sigma
        self.preserve_amplitude = bool(preserve_amplitude)
        self.return_mask = bool(return_mask)
        self.last_mask = None
        if not self.target_vars:
            raise ValueError("WindArtifactFilter: target_vars is empty")
        if len(self.target_vars) > MAX_VARIABLES:
            raise ValueError(f"WindArtifactFilter: {len(self.target_vars)} target variables, one call takes at most {MAX_VARIABLES}")
        if len(set(self.target_vars)) != len(self.target_vars):
            raise ValueError("WindArtifactFilter: a variable is listed twice in target_vars")
        if self.mask_level < 0:
            raise ValueError(f"WindArtifactFilter: mask_level {mask_level} is negative")
        if any(l < 0 for l in self.target_levels):
            raise ValueError("WindArtifactFilter: a target level is negative")
        for name, sig in (("smooth_sigma", smooth_sigma), ("smooth_sigma_zonal", smooth_sigma_zonal),
                          ("smooth_sigma_meridional", smooth_sigma_meridional), ("falloff_sigma", falloff_sigma)):
            if sig is not None and not (float(sig) > 0.0 and np.isfinite(float(sig))):
                raise ValueError(f"WindArtifactFilter: {name} = {sig} must be a positive number")
        if not np.isfinite(self.speed_threshold):
            raise ValueError("WindArtifactFilter: speed_threshold must be finite")
        for name, d, cap in (("dilation_zonal", self.dilation_zonal, MAX_KERNEL_LON), ("dilation_meridional", self.dilation_meridional, MAX_KERNEL_LAT)):
            if d < 1:
                raise ValueError(f"WindArtifactFilter: {name} = {d} must be >= 1")
            if d % 2 == 0:
                raise ValueError(f"WindArtifactFilter: {name} = {d} is even; the reference's dilated mask then comes out one "
                                 f"{'column' if 'zonal' in name else 'row'} larger than the field and its forward raises -- use an odd size")
            if d > cap:
                raise ValueError(f"WindArtifactFilter: {name} = {d} exceeds the supported {cap}")
        sizes = kernel_sizes(smooth_sigma, smooth_sigma_zonal, smooth_sigma_meridional, falloff_sigma)
        for name, n in sizes.items():
            cap = MAX_KERNEL_LON if name.endswith("lon") else MAX_KERNEL_LAT
            if n > cap:
                raise ValueError(f"WindArtifactFilter: the {name.replace('_', ' ')} kernel has {n} points, the device kernels take at most "
                                 f"{cap} (falloff_sigma <= 8, smoothing sigma <= 5.33 meridional / 10.66 zonal)")
        self.kernels = filter_kernels(smooth_sigma, smooth_sigma_zonal, smooth_sigma_meridional, falloff_sigma)
        self._levels = np.array(sorted(self.target_levels), np.int32)
        self._warned = set()
        self.lib = require_gpu("the wind artifact filter has no CPU fallback")
        self._handles = HandleCache(self.lib, "wx_wind")   # by (H, W, device)

    def _handle(self, H, W, dev):
        def args():
            weights = [x for n in ("smooth_lat", "smooth_lon", "falloff_lat", "falloff_lon") for x in (_f32(self.kernels[n]), self.kernels[n].size)]
            return (H, W, *weights, self.dilation_meridional, self.dilation_zonal, self.speed_threshold, int(self.preserve_amplitude), dev)
        return self._handles.get((H, W, dev), args)

    def __call__(self, batch_dict: dict) -> dict:
        import torch
        u, v = _pred(batch_dict, self.u_var), _pred(batch_dict, self.v_var)
        check_named_tensor(self.u_var, u, one_time=True)
        check_named_tensor(self.v_var, v, like=(self.u_var, u), one_time=True)
        B, Lu, _, H, W = u.shape
        if self.mask_level >= Lu or self.mask_level >= v.shape[1]:
            raise WXEngineError(f"mask_level {self.mask_level} is beyond the {min(Lu, v.shape[1])} levels of {self.u_var} / {self.v_var}")
        ts = [_pred(batch_dict, k) for k in self.target_vars]
        for key, t in zip(self.target_vars, ts):
            check_named_tensor(key, t, like=(self.u_var, u), one_time=True)
            if t.shape[1] > MAX_LEVELS:
                raise WXEngineError(f"{key}: {t.shape[1]} levels, the kernel takes at most {MAX_LEVELS}")
            out_of_range = [lev for lev in sorted(self.target_levels) if lev >= t.shape[1]]
            if out_of_range and key not in self._warned:   # once per variable, not once per step
                self._warned.add(key)
                logger.warning("WindArtifactFilter: target level(s) %s exceed available levels (%d) for '%s'; skipping them.",
                               out_of_range, t.shape[1], key)
        dev = u.device.index
        h = self._handle(H, W, dev)
        src, bs, nl, outs, dst = _named_tensor_args(ts)
        mask = torch.empty((B, 1, H, W), dtype=torch.float32, device=u.device) if self.return_mask else None
        um, vm = u[:, self.mask_level], v[:, self.mask_level]
        with torch.cuda.device(dev):
            _check(self.lib.wx_wind_apply(h, C.c_void_p(um.data_ptr()), batch_stride(u, B), C.c_void_p(vm.data_ptr()),
                                          batch_stride(v, B), len(ts), src, bs, nl, dst, _i32(self._levels), int(self._levels.size), B,
                                          C.c_void_p(mask.data_ptr()) if mask is not None else None, _stream_ptr(dev)))
        for key, o in zip(self.target_vars, outs):
            _set_pred(batch_dict, key, o)
        if self.return_mask:
            self.last_mask = mask
        return batch_dict

    forward = __call__
