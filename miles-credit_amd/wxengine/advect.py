"""Semi-Lagrangian tracer advection of the gen-2 block chains on the device (credit/postblock/advect.py, credit/preblock/advect.py,
csrc/wx_advect.h).

`SemiLagrangianAdvection` takes the reference's argument names and defaults and is a callable on the batch dict like the other post
blocks; it needs physical units, so it goes BEHIND the inverse scale:
    run_forecast(..., step_postblocks=[InverseScale(mean, std), SemiLagrangianAdvection(tracer_vars=[q], ...)])
`SemiLagrangianAdvectionPre` is the thin pre block over the same engine (`batch[data_type][source][var_key]`).
Per call, in two launches whatever the number of tracers: omega from mass continuity (or read from `omega_var`), the index-space
velocity of every grid point, an iterative-midpoint back-trajectory, and every tracer read trilinearly at its departure point.  The
variables are read where they lie (the channel slices `Reconstruct` hands out) and the dict entries of the tracers are rebound to fresh
contiguous [B, L, 1, H, W] tensors: the inputs are never modified.

The hybrid coefficients and the coordinates come as arrays (`model_a_half`, `model_b_half`, `latitude`, `longitude`) where the
reference opens NetCDF files, as `GeopotentialDiagnostic` here does.  The metric tables are computed here with the reference's float32
torch expressions on the CPU (`metric_tables`) and uploaded once per (H, W, L, device).  No CPU fallback: construction raises without
a GPU."""
from __future__ import annotations

import ctypes as C
import logging
from typing import Dict, List, Optional, Sequence

import numpy as np

from .diagnostics import _lookup
from .native import (HandleCache, WXEngineError, _check, _f32, _named_tensor_args, _stream_ptr, batch_stride, check_named_tensor, copy_batch,
                     load_library, require_gpu)
from .transforms import _check_data_types

logger = logging.getLogger(__name__)

MAX_TRACERS = 32            # kAdvectMaxTracers
RAD_EARTH = 6371000.0       # credit/physics_constants.py
LEVEL_ORDERS = ("top_to_surface", "surface_to_top")


def slice_half_levels(a_all, b_all, levels: Optional[Sequence[int]]):
    """advect.py:260-266: the half levels around the 1-based model `levels` (None: every half level), float32."""
    a_all, b_all = np.asarray(a_all, np.float32), np.asarray(b_all, np.float32)
    if levels is None:
        return a_all, b_all
    half_idx = [lv - 1 for lv in levels] + [levels[-1]]
    return a_all[half_idx], b_all[half_idx]


def uniform_grid(n_lat: int, n_lon: int):
    """advect.py:313-314: the uniform global grid the reference falls back to, float32 degrees."""
    import torch
    return (torch.linspace(90.0, -90.0, n_lat, dtype=torch.float32).numpy(),
            (torch.arange(n_lon, dtype=torch.float32) * (360.0 / n_lon)).numpy())


def metric_tables(lat_deg, lon_deg, coslat_floor: float = 1e-4) -> Dict[str, np.ndarray]:
    """What the kernels need of the grid, with the reference's float32 torch expressions on the CPU (advect.py:107-118, :316-320,
    :374-376): `rows` [6, H] = cos(lat), R * max(cos(lat), floor), torch.gradient(lat_rad), and the coefficients a, b, c of
    torch.gradient's coordinate-aware difference a f[h - 1] + b f[h] + c f[h + 1] (on the first / last row b holds the one-sided
    spacing); `dlon` = deg2rad(lon[1] - lon[0])."""
    import torch
    lat_deg = torch.as_tensor(np.asarray(lat_deg), dtype=torch.float32)
    lon_deg = torch.as_tensor(np.asarray(lon_deg), dtype=torch.float32)
    lat_rad = torch.deg2rad(lat_deg)
    dlat_row = torch.gradient(lat_rad, edge_order=1)[0]
    dlon = torch.deg2rad(lon_deg[1] - lon_deg[0])
    coslat = torch.cos(lat_rad)
    r_coslat = RAD_EARTH * coslat.clamp(min=float(coslat_floor))
    dx = lat_rad.diff()
    dx1, dx2 = dx[:-1], dx[1:]
    zero = torch.zeros(1)
    ga = torch.cat([zero, -dx2 / (dx1 * (dx1 + dx2)), zero])
    gb = torch.cat([dx[:1], (dx2 - dx1) / (dx1 * dx2), dx[-1:]])
    gc = torch.cat([zero, dx1 / (dx2 * (dx1 + dx2)), zero])
    return {"rows": torch.stack([coslat, r_coslat, dlat_row, ga, gb, gc]).numpy(), "dlon": np.float32(dlon.item())}


class _AdvectionEngine:
    """credit/postblock/advect.py::_SemiLagrangianAdvectionEngine on the device: the arguments, the tables and `advect_nested`."""

    def __init__(self, tracer_vars: Optional[List[str]] = None, u_var: str = "ERA5/prognostic/3d/u_component_of_wind",
                 v_var: str = "ERA5/prognostic/3d/v_component_of_wind", surface_pressure_var: str = "ERA5/prognostic/2d/surface_pressure",
                 timestep_seconds: float = 21600.0, n_iterations: int = 2, omega_var: Optional[str] = None, model_a_half=None,
                 model_b_half=None, levels: Optional[List[int]] = None, level_order: str = "top_to_surface", latitude=None,
                 longitude=None, coslat_floor: float = 1e-4, dp_dlevel_floor: float = 1.0, lon_halo: int = 1):
        name = "SemiLagrangianAdvection"
        if level_order not in LEVEL_ORDERS:
            raise ValueError(f"{name}: level_order {level_order!r} is neither of {LEVEL_ORDERS}")
        if n_iterations < 1:
            raise ValueError(f"{name}: n_iterations = {n_iterations}, the back-trajectory takes at least one")
        if int(lon_halo) < 1:
            raise ValueError(f"{name}: lon_halo = {lon_halo} must be >= 1 (the reference's one-column halo; any width gives the same result)")
        self.tracer_vars = list(tracer_vars) if tracer_vars else ["ERA5/prognostic/3d/specific_humidity"]
        if len(set(self.tracer_vars)) != len(self.tracer_vars):
            raise ValueError(f"{name}: a tracer is listed twice in tracer_vars (the reference would advect it twice)")
        if len(self.tracer_vars) > MAX_TRACERS:
            raise ValueError(f"{name}: {len(self.tracer_vars)} tracers, one call takes at most {MAX_TRACERS}")
        self.u_var, self.v_var, self.surface_pressure_var, self.omega_var = u_var, v_var, surface_pressure_var, omega_var
        self.timestep_seconds, self.n_iterations = float(timestep_seconds), int(n_iterations)
        self.levels, self.level_order = levels, level_order
        self.coslat_floor, self.dp_dlevel_floor, self.lon_halo = float(coslat_floor), float(dp_dlevel_floor), int(lon_halo)
        for what, x in (("timestep_seconds", self.timestep_seconds), ("coslat_floor", self.coslat_floor), ("dp_dlevel_floor", self.dp_dlevel_floor)):
            if not np.isfinite(x):
                raise ValueError(f"{name}: {what} = {x} must be finite")
        for what, x in (("model_a_half", model_a_half), ("model_b_half", model_b_half), ("latitude", latitude), ("longitude", longitude)):
            if x is None:
                raise ValueError(f"{name}: {what} is required (an array; the reference reads it from its level / grid info file)")
        self.a_half, self.b_half = slice_half_levels(model_a_half, model_b_half, levels)
        self.lat_deg = np.asarray(latitude, np.float32).reshape(-1)
        self.lon_deg = np.asarray(longitude, np.float32).reshape(-1)
        if self.lon_deg.size < 2:
            raise ValueError(f"{name}: {self.lon_deg.size} longitude(s); the longitude spacing needs at least two")
        if self.lat_deg.size < 2:
            raise ValueError(f"{name}: {self.lat_deg.size} latitude(s); the latitude spacing needs at least two")
        self._warned = False
        self._tables = {}    # (H, W) -> metric_tables
        self.lib = require_gpu("the semi-Lagrangian advection has no CPU fallback", load=load_library)
        self._handles = HandleCache(self.lib, "wx_advect")   # by (H, W, L, device)

    def grid_for(self, H: int, W: int):
        """advect.py:301-314: the given coordinates where their lengths match the data grid, else the uniform global grid, with one
        warning per object."""
        if self.lat_deg.size == H and self.lon_deg.size == W:
            return self.lat_deg, self.lon_deg
        if not self._warned:
            self._warned = True
            logger.warning("SemiLagrangianAdvection: %d latitudes x %d longitudes were given, the data grid is %d x %d; using the uniform "
                           "global grid linspace(90, -90) x arange * 360 / W instead.", self.lat_deg.size, self.lon_deg.size, H, W)
        return uniform_grid(H, W)

    def _handle(self, H, W, L, dev):
        def args():
            if (H, W) not in self._tables:
                self._tables[(H, W)] = metric_tables(*self.grid_for(H, W), self.coslat_floor)
            t = self._tables[(H, W)]
            return (H, W, L, _f32(self.a_half), _f32(self.b_half), _f32(t["rows"]), float(t["dlon"]), self.timestep_seconds,
                    self.n_iterations, self.dp_dlevel_floor, int(self.level_order == "surface_to_top"), dev)
        return self._handles.get((H, W, L, dev), args)

    def advect_nested(self, nested: dict) -> None:
        """advect.py:325-423: every tracer of `nested` ({source: {var_key: tensor}}) advected one step; the tracers' entries are rebound."""
        import torch
        u = _lookup(nested, self.u_var)
        check_named_tensor(self.u_var, u, one_time=True)
        B, L, _, H, W = u.shape
        named = [(self.v_var, _lookup(nested, self.v_var), L), (self.surface_pressure_var, _lookup(nested, self.surface_pressure_var), 1)]
        if self.omega_var is not None:
            named.append((self.omega_var, _lookup(nested, self.omega_var), L))
        ts = [_lookup(nested, k) for k in self.tracer_vars]
        named += [(k, t, L) for k, t in zip(self.tracer_vars, ts)]
        for key, t, levels in named:
            check_named_tensor(key, t, like=(self.u_var, u), one_time=True)
            if t.shape[1] != levels:
                raise WXEngineError(f"{key}: shape {tuple(t.shape)} does not match {self.u_var}: {tuple(u.shape)} "
                                    f"(the block needs {levels} level(s) here)")
        if self.a_half.size != L + 1:
            raise ValueError(f"SemiLagrangianAdvection: built {self.a_half.size} interface pressures for {L} levels; expected {L + 1}. "
                             "Set `levels` to the model levels present in the data.")
        if L == 1:
            raise WXEngineError("SemiLagrangianAdvection: a single level; the reference's torch.gradient over the level axis raises there too")
        if W < 2 or H < 2:
            raise WXEngineError(f"SemiLagrangianAdvection: a {H} x {W} grid; at least two latitudes and two longitudes")
        dev = u.device.index
        h = self._handle(H, W, L, dev)
        src, bs, _, outs, dst = _named_tensor_args(ts)
        v, sp = named[0][1], named[1][1]
        om = named[2][1] if self.omega_var is not None else None
        with torch.cuda.device(dev):
            _check(self.lib.wx_advect_apply(h, C.c_void_p(u.data_ptr()), batch_stride(u, B), C.c_void_p(v.data_ptr()), batch_stride(v, B),
                                            C.c_void_p(sp.data_ptr()), batch_stride(sp, B), C.c_void_p(om.data_ptr()) if om is not None else None,
                                            batch_stride(om, B) if om is not None else 0, len(ts), src, bs, dst, B, _stream_ptr(dev)))
        for key, o in zip(self.tracer_vars, outs):
            nested[key.split("/")[0]][key] = o


class SemiLagrangianAdvection:
    """credit/postblock/advect.py::SemiLagrangianAdvectionPost on the device: advects the tracers of `batch_dict[key]`."""

    def __init__(self, key: str = "y_processed", **engine_kwargs):
        self.key = key
        self.engine = _AdvectionEngine(**engine_kwargs)

    def __call__(self, batch_dict: dict) -> dict:
        self.engine.advect_nested(batch_dict[self.key])
        return batch_dict

    forward = __call__


class SemiLagrangianAdvectionPre:
    """credit/preblock/advect.py::SemiLagrangianAdvectionPre on the device: one advection step on `batch[data_type]` for every
    requested data type that is present; the caller's dict is not mutated."""

    def __init__(self, data_types: Optional[List[str]] = None, **engine_kwargs):
        self.data_types = _check_data_types(data_types, " Preblocks never operate on 'metadata'.")
        self.engine = _AdvectionEngine(**engine_kwargs)

    def __call__(self, batch: dict) -> dict:
        batch = copy_batch(batch, self.data_types)
        for data_type in self.data_types:
            if data_type in batch:       # absent (no "target" at inference): skipped
                self.engine.advect_nested(batch[data_type])
        return batch

    forward = __call__
