"""Hybrid-level interpolation of the gen-2 block chains on the device (credit/postblock/hybrid_interp.py,
credit/preblock/hybrid_interp.py, credit/postblock/_interp_utils.py; csrc/wx_hybrid.h).

`HybridLevelInterp` takes the reference's argument names and is a callable on the batch dict like the other post blocks; it needs
physical units (pressures in Pa), so in a forecast it goes BEHIND the inverse scale:
    run_forecast(..., step_postblocks=[InverseScale(mean, std), HybridLevelInterp(variables=[...], ...)])
`HybridLevelInterpPre` is the thin pre block over the same engine (`batch[data_type][source][var_key]`): the block that puts a
GFS-level analysis onto the model's levels.
Per call: every configured variable that is present, [B, n_source_levels, n_time, H, W], is interpolated linearly in log p onto the
destination levels, with p = max(a + b sp, 0.57 Pa) for both level sets from the same surface pressure and constant extrapolation
outside the source range.  The variables are read where they lie (channel slices included) and their dict entries are rebound to
fresh contiguous [B, n_dest_levels, n_time, H, W] tensors: the inputs are never modified.

The coefficients come as arrays (`source_a`, `source_b`, `dest_a`, `dest_b`) where the reference names a NetCDF file and two of its
variables, as `GeopotentialDiagnostic` and `SemiLagrangianAdvection` here do; `midpoint_coefficients` does to them what
`load_hybrid_level_coefficients` does to the file's.  No CPU fallback: construction raises without a GPU."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from .native import (HandleCache, WXEngineError, _check, _f32, _named_tensor_args, _stream_ptr, batch_stride, check_named_tensor,
                     copy_batch, load_library, require_gpu)
from .transforms import _check_data_types

MAX_VARIABLES = 32     # kHybridMaxVars
MAX_LEVELS = 137       # kHybridMaxLevels


def midpoint_coefficients(a, b=None, on_interfaces: bool = True, levels: Optional[Sequence[int]] = None):
    """_interp_utils.py:69-80 on arrays, in its order: float64; with `b is None` and a 2-D `a` (the GFS `vcoord` convention, where
    the reference is given one variable name twice) row 0 is a and row 1 is b; interface values averaged to midpoints in float64;
    then the 1-based `levels` subset; then the cast to float32.  -> (a, b) float32 at level midpoints, in stored order."""
    a = np.asarray(a, dtype=np.float64)
    if b is None:
        if a.ndim != 2 or a.shape[0] < 2:
            raise ValueError(f"midpoint_coefficients: without b, a must be the 2-D vcoord array (row 0 = a, row 1 = b), got shape {a.shape}")
        a, b = a[0], a[1]
    else:
        b = np.asarray(b, dtype=np.float64)
    if a.ndim != 1 or b.ndim != 1 or a.shape != b.shape:
        raise ValueError(f"midpoint_coefficients: a and b must be 1-D arrays of one length, got shapes {a.shape} and {b.shape}")
    if on_interfaces:
        a = 0.5 * (a[:-1] + a[1:])
        b = 0.5 * (b[:-1] + b[1:])
    if levels is not None:
        idx = [int(lv) - 1 for lv in levels]
        if any(i < 0 or i >= a.size for i in idx):
            raise ValueError(f"midpoint_coefficients: levels are 1-based midpoint level numbers in 1 .. {a.size}, got {list(levels)}")
        a, b = a[idx], b[idx]
    return a.astype(np.float32), b.astype(np.float32)


class _HybridInterpEngine:
    """credit/postblock/hybrid_interp.py::_HybridLevelInterpEngine on the device: the arguments, the coefficients and `interp_nested`."""

    def __init__(self, variables: List[str] = None, surface_pressure_var: str = None, source_a=None, source_b=None,
                 source_on_interfaces: bool = True, source_levels: Optional[List[int]] = None, dest_a=None, dest_b=None,
                 dest_on_interfaces: bool = True, dest_levels: Optional[List[int]] = None, chunk_size: int = 1000):
        name = "HybridLevelInterp"
        if variables is None or isinstance(variables, str):
            raise ValueError(f"{name}: variables is required (a list of 3-D var_keys)")
        if not isinstance(surface_pressure_var, str):
            raise ValueError(f"{name}: surface_pressure_var is required (the var_key of the surface pressure in Pa)")
        self.variables = list(variables)
        if len(set(self.variables)) != len(self.variables):
            raise ValueError(f"{name}: a variable is listed twice in variables")
        if len(self.variables) > MAX_VARIABLES:
            raise ValueError(f"{name}: {len(self.variables)} variables, one call takes at most {MAX_VARIABLES}")
        self.surface_pressure_var = surface_pressure_var
        self.chunk_size = chunk_size      # accepted for the reference's configs; the device block has no chunks
        if source_a is None:
            raise ValueError(f"{name}: source_a is required (an array; the reference reads it from source_level_info_file)")
        if dest_a is None:
            raise ValueError(f"{name}: dest_a is required (an array; the reference reads it from dest_level_info_file)")
        self.source_a, self.source_b = midpoint_coefficients(source_a, source_b, source_on_interfaces, source_levels)
        self.dest_a, self.dest_b = midpoint_coefficients(dest_a, dest_b, dest_on_interfaces, dest_levels)
        if self.source_a.size == 1:
            raise ValueError(f"{name}: a single source midpoint level has no bracket to interpolate in (the reference's gather fails there)")
        for what, x, least in (("source", self.source_a, 2), ("destination", self.dest_a, 1)):
            if not least <= x.size <= MAX_LEVELS:
                raise ValueError(f"{name}: {x.size} {what} midpoint levels; the device block takes {least} .. {MAX_LEVELS}")
        for what, x in (("source_a", self.source_a), ("source_b", self.source_b), ("dest_a", self.dest_a), ("dest_b", self.dest_b)):
            if not np.isfinite(x).all():
                raise ValueError(f"{name}: {what} has a non-finite midpoint coefficient")
        self.lib = require_gpu("the hybrid-level interpolation has no CPU fallback", load=load_library)
        self._handles = HandleCache(self.lib, "wx_hybrid")   # by (H, W, device)

    def _handle(self, H, W, dev):
        return self._handles.get((H, W, dev), lambda: (H, W, self.source_a.size, _f32(self.source_a), _f32(self.source_b), self.dest_a.size,
                                                       _f32(self.dest_a), _f32(self.dest_b), dev))

    def interp_nested(self, nested: dict) -> None:
        """hybrid_interp.py:108-161: every configured variable present in `nested` ({source: {var_key: tensor}}) onto the destination
        levels; its entry is rebound."""
        import torch
        present = [v for v in self.variables if v in nested.get(v.split("/")[0], {})]
        if not present:
            return
        sp = nested[self.surface_pressure_var.split("/")[0]][self.surface_pressure_var]
        check_named_tensor(self.surface_pressure_var, sp)
        B, _, T, H, W = sp.shape
        if sp.shape[1] != 1:
            raise WXEngineError(f"{self.surface_pressure_var}: shape {tuple(sp.shape)}; the surface pressure is [B, 1, n_time, H, W]")
        ts = [nested[v.split("/")[0]][v] for v in present]
        for key, t in zip(present, ts):
            if hasattr(t, "shape") and len(t.shape) > 1 and t.shape[1] != self.source_a.size:
                raise ValueError(f"HybridLevelInterp: {key!r} has {t.shape[1]} levels but the source "
                                 f"coefficients define {self.source_a.size} midpoint levels.")
            check_named_tensor(key, t, like=(self.surface_pressure_var, sp))
        dev = sp.device.index
        h = self._handle(H, W, dev)
        src, bs, _, outs, dst = _named_tensor_args(ts, out_levels=self.dest_a.size)
        with torch.cuda.device(dev):
            _check(self.lib.wx_hybrid_apply(h, len(ts), src, bs, dst, B, T, C.c_void_p(sp.data_ptr()), batch_stride(sp, B), _stream_ptr(dev)))
        for key, o in zip(present, outs):
            nested[key.split("/")[0]][key] = o


class HybridLevelInterp:
    """credit/postblock/hybrid_interp.py::HybridLevelInterpPost on the device: interpolates the variables of `batch_dict[key]`."""

    def __init__(self, key: str = "y_processed", **engine_kwargs):
        self.key = key
        self.engine = _HybridInterpEngine(**engine_kwargs)

    def __call__(self, batch_dict: dict) -> dict:
        if self.key not in batch_dict:
            raise ValueError(f"Key {self.key!r} not found in batch_dict.")
        self.engine.interp_nested(batch_dict[self.key])
        return batch_dict

    forward = __call__


class HybridLevelInterpPre:
    """credit/preblock/hybrid_interp.py::HybridLevelInterpPre on the device: the interpolation on `batch[data_type]` for every
    requested data type that is present; the caller's dict is not mutated."""

    def __init__(self, data_types: Optional[List[str]] = None, **engine_kwargs):
        self.data_types = _check_data_types(data_types, " Preblocks never operate on 'metadata'.")
        self.engine = _HybridInterpEngine(**engine_kwargs)

    def __call__(self, batch: dict) -> dict:
        batch = copy_batch(batch, self.data_types)
        for data_type in self.data_types:
            if data_type in batch:       # absent (no "target" at inference): skipped
                self.engine.interp_nested(batch[data_type])
        return batch

    forward = __call__
