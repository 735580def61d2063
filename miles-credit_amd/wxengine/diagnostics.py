"""Pressure-level products of the gen-2 post-block chain on the device: drop-ins for the reference's

* `GeopotentialDiagnostic`   credit/postblock/geopotential.py:86-228   (geopotential on model levels)
* `PressureInterpDiagnostic` credit/postblock/pressure_interp.py:133-332 (model levels -> pressure levels, Trenberth below ground)
* `MSLPDiagnostic`           credit/postblock/mslp.py:83-159           (mean sea level pressure)

with the reference's constructor argument names and defaults, callables on the batch dict that write the same keys with the same
shapes -- and `PressureLevelProducts`, the fused form: one object, ONE launch for everything requested, the geopotential never
leaving the chip between the integral and the interpolation.  The chain of the three blocks and the fused object give the same bits.

The one difference from the reference: the hybrid coefficients arrive as arrays (`model_a_half`, `model_b_half` on the level
interfaces, `model_a`, `model_b` on the mid levels; the full set `levels` indexes into) instead of a netCDF file name -- xarray is
not on the product path.  `levels` subsets them like the reference (geopotential.py:165-168: half_idx = [lv - 1 ...] + [levels[-1]];
pressure_interp.py:228-231).  `chunk_size` is accepted and ignored: a launch covers every column.

All of it runs in csrc/wx_diag.h through `wx_diag_*`; there is no CPU fallback: without the library or a GPU, construction raises
WXEngineError.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from .engine import WXDiag
from .native import require_gpu

_T = "ARCO_ERA5/prognostic/3d/temperature"
_Q = "ARCO_ERA5/prognostic/3d/specific_humidity"
_SP = "ARCO_ERA5/prognostic/2d/surface_pressure"
_PHIS = "ARCO_ERA5/static/2d/geopotential_at_surface"
_Z = "ARCO_ERA5/derived_diagnostic/3d/geopotential"
_T2M = "ARCO_ERA5/prognostic/2d/2m_temperature"
_MSLP = "ARCO_ERA5/derived_diagnostic/2d/mean_sea_level_pressure"
_UVQ = ("ARCO_ERA5/prognostic/3d/u_component_of_wind", "ARCO_ERA5/prognostic/3d/v_component_of_wind", _Q)


def half_level_subset(a_all, b_all, levels: Optional[Sequence[int]]):
    """Interface coefficients of a subset of 1-based model levels (geopotential.py:165-171)."""
    a, b = np.asarray(a_all, np.float32).ravel(), np.asarray(b_all, np.float32).ravel()
    if levels is None:
        return a, b
    idx = [lv - 1 for lv in levels] + [levels[-1]]
    return a[idx], b[idx]


def mid_level_subset(a_all, b_all, levels: Optional[Sequence[int]]):
    """Mid-level coefficients of a subset of 1-based model levels (pressure_interp.py:228-234)."""
    a, b = np.asarray(a_all, np.float32).ravel(), np.asarray(b_all, np.float32).ravel()
    if levels is None:
        return a, b
    idx = [lv - 1 for lv in levels]
    return a[idx], b[idx]


def pressure_output_key(var_key: str, output_suffix: str = "_PRES") -> str:
    """pressure_interp.py:243-245: "source/field_type/dim/varname" -> "source/derived_diagnostic/dim/varname<suffix>"."""
    parts = var_key.split("/")
    return f"{parts[0]}/derived_diagnostic/{parts[2]}/{parts[3]}{output_suffix}"


def _require_device():
    require_gpu("the pressure-level products have no CPU fallback")


def _lookup(nested: dict, var_key: str):
    return nested[var_key.split("/")[0]][var_key]


class PressureLevelProducts:
    """Everything requested in one launch.  A product is requested by naming its output: `geopotential_output_name` (model-level
    Z; `write_geopotential=False` keeps the name for the pressure-level key but leaves the model-level field unwritten),
    `pressure_levels` (hPa; the `interp_variables`, then T and Z, to "<...>{output_suffix}" keys) and `mslp_output_name` (needs
    `near_surface_temperature_var`); None switches it off."""

    def __init__(self, pressure_levels: Optional[Sequence[float]] = (500.0, 850.0), interp_variables: Sequence[str] = _UVQ,
                 temperature_var: str = _T, specific_humidity_var: str = _Q, surface_pressure_var: str = _SP,
                 surface_geopotential_var: str = _PHIS, near_surface_temperature_var: Optional[str] = _T2M,
                 geopotential_output_name: Optional[str] = _Z, mslp_output_name: Optional[str] = _MSLP,
                 geopotential_var: Optional[str] = None, output_suffix: str = "_PRES", temp_height: float = 150.0,
                 flip_vertical: bool = True, model_a_half=None, model_b_half=None, model_a=None, model_b=None,
                 key: str = "y_processed", static_source_key: str = "ic_raw", levels: Optional[List[int]] = None,
                 write_geopotential: bool = True):
        _require_device()
        self.write_geopotential = bool(write_geopotential) and geopotential_output_name is not None
        self.pressure_levels = None if pressure_levels is None else [float(p) for p in pressure_levels]
        self.interp_variables = list(interp_variables) if self.pressure_levels is not None else []
        self.temperature_var, self.specific_humidity_var = temperature_var, specific_humidity_var
        self.surface_pressure_var, self.surface_geopotential_var = surface_pressure_var, surface_geopotential_var
        self.near_surface_temperature_var = near_surface_temperature_var
        self.geopotential_output_name, self.mslp_output_name = geopotential_output_name, mslp_output_name
        # chain form: the interpolation takes this model-level geopotential from the batch instead of integrating T and q
        self.geopotential_var = geopotential_var
        self.output_suffix, self.temp_height, self.flip_vertical = output_suffix, float(temp_height), bool(flip_vertical)
        self.key, self.static_source_key, self.levels = key, static_source_key, levels
        self.integrates = self.write_geopotential or (self.pressure_levels is not None and geopotential_var is None)
        if self.integrates and (model_a_half is None or model_b_half is None):
            raise ValueError("the geopotential needs model_a_half and model_b_half")
        if self.pressure_levels is not None and (model_a is None or model_b is None):
            raise ValueError("the pressure-level set needs model_a and model_b")
        if mslp_output_name is not None and near_surface_temperature_var is None:
            raise ValueError("MSLP needs near_surface_temperature_var")
        self.model_a_half, self.model_b_half = (None, None) if model_a_half is None else half_level_subset(model_a_half, model_b_half, levels)
        self.model_a, self.model_b = (None, None) if model_a is None else mid_level_subset(model_a, model_b, levels)
        self._dev: Dict[tuple, WXDiag] = {}

    def output_keys(self) -> List[str]:
        keys = [self.geopotential_output_name] if self.write_geopotential else []
        if self.pressure_levels is not None:
            zkey = self.geopotential_var or self.geopotential_output_name or _Z
            keys += [pressure_output_key(v, self.output_suffix) for v in self.interp_variables + [self.temperature_var, zkey]]
        return keys + ([] if self.mslp_output_name is None else [self.mslp_output_name])

    def _device_block(self, H, W, L, device) -> WXDiag:
        k = (H, W, L, device)
        if k not in self._dev:
            d = WXDiag(H, W, L, device)
            d.set_levels(self.model_a_half, self.model_b_half, self.model_a, self.model_b, self.flip_vertical)
            if self.pressure_levels is not None:
                d.set_pressure_levels([p * 100.0 for p in self.pressure_levels], self.temp_height)   # hPa -> Pa
            self._dev[k] = d
        return self._dev[k]

    def __call__(self, batch_dict: dict) -> dict:
        for required_key in (self.key, self.static_source_key):
            if required_key not in batch_dict:
                raise ValueError(f"Key {required_key!r} not found in batch_dict.")
        nested, static_nested = batch_dict[self.key], batch_dict[self.static_source_key]
        sp = _lookup(nested, self.surface_pressure_var)
        phis = _lookup(static_nested, self.surface_geopotential_var)
        if phis.device != sp.device:
            phis = phis.to(sp.device)
        want_plev, want_z, want_mslp = self.pressure_levels is not None, self.write_geopotential, self.mslp_output_name is not None
        need_column = want_plev or want_z
        T = _lookup(nested, self.temperature_var) if need_column else None
        q = _lookup(nested, self.specific_humidity_var) if self.integrates else None
        z_in = _lookup(nested, self.geopotential_var) if (want_plev and self.geopotential_var is not None) else None
        L = T.shape[1] if need_column else max(len(self.model_a) if self.model_a is not None else 2, 2)
        dev = self._device_block(sp.shape[3], sp.shape[4], L, sp.device.index)
        out = dev.apply(sp, phis, T=T, q=q, t_ns=_lookup(nested, self.near_surface_temperature_var) if want_mslp else None,
                        fields=[_lookup(nested, v) for v in self.interp_variables], z_in=z_in, want_z=want_z, want_plev=want_plev,
                        want_mslp=want_mslp)
        keys = self.output_keys()
        values = ([out["z"]] if want_z else []) + (out["plev"] if want_plev else []) + ([out["mslp"]] if want_mslp else [])
        for k, v in zip(keys, values):
            nested.setdefault(k.split("/")[0], {})[k] = v
        return batch_dict

    forward = __call__


class GeopotentialDiagnostic(PressureLevelProducts):
    """credit/postblock/geopotential.py:86-228 on the device; argument names and defaults are the reference's."""

    def __init__(self, output_name: str = _Z, chunk_size: int = 1000, surface_geopotential_var: str = _PHIS,
                 surface_pressure_var: str = _SP, temperature_var: str = _T, specific_humidity_var: str = _Q,
                 flip_vertical: bool = True, model_a_half=None, model_b_half=None, key: str = "y_processed",
                 static_source_key: str = "ic_raw", levels: Optional[List[int]] = None):
        super().__init__(pressure_levels=None, temperature_var=temperature_var, specific_humidity_var=specific_humidity_var,
                         surface_pressure_var=surface_pressure_var, surface_geopotential_var=surface_geopotential_var,
                         near_surface_temperature_var=None, geopotential_output_name=output_name, mslp_output_name=None,
                         flip_vertical=flip_vertical, model_a_half=model_a_half, model_b_half=model_b_half, key=key,
                         static_source_key=static_source_key, levels=levels)
        self.output_name, self.chunk_size = output_name, chunk_size


class PressureInterpDiagnostic(PressureLevelProducts):
    """credit/postblock/pressure_interp.py:133-332 on the device; `geopotential_var` must already be in the batch (chain a
    GeopotentialDiagnostic in front), exactly as in the reference."""

    def __init__(self, pressure_levels: Sequence[float] = (500.0, 850.0), interp_variables: Sequence[str] = _UVQ,
                 temperature_var: str = _T, geopotential_var: str = _Z, surface_pressure_var: str = _SP,
                 surface_geopotential_var: str = _PHIS, output_suffix: str = "_PRES", temp_height: float = 150.0,
                 chunk_size: int = 1000, model_a=None, model_b=None, key: str = "y_processed", static_source_key: str = "ic_raw",
                 levels: Optional[List[int]] = None):
        super().__init__(pressure_levels=pressure_levels, interp_variables=interp_variables, temperature_var=temperature_var,
                         surface_pressure_var=surface_pressure_var, surface_geopotential_var=surface_geopotential_var,
                         near_surface_temperature_var=None, geopotential_output_name=None, mslp_output_name=None,
                         geopotential_var=geopotential_var, output_suffix=output_suffix, temp_height=temp_height, model_a=model_a,
                         model_b=model_b, key=key, static_source_key=static_source_key, levels=levels)
        self.chunk_size = chunk_size


class MSLPDiagnostic(PressureLevelProducts):
    """credit/postblock/mslp.py:83-159 on the device."""

    def __init__(self, output_name: str = _MSLP, surface_pressure_var: str = _SP, temperature_var: str = _T2M,
                 surface_geopotential_var: str = _PHIS, key: str = "y_processed", static_source_key: str = "ic_raw"):
        super().__init__(pressure_levels=None, surface_pressure_var=surface_pressure_var, surface_geopotential_var=surface_geopotential_var,
                         near_surface_temperature_var=temperature_var, geopotential_output_name=None, mslp_output_name=output_name,
                         key=key, static_source_key=static_source_key)
        self.output_name = output_name
