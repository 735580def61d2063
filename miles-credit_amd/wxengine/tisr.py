"""The TISR forcing on the device (credit/datasets/gen_2/tisr.py::TISRDataset, dataset_type "tisr"; csrc/wx_tisr.h): the top-of-
atmosphere incident solar radiation accumulated over the model time step, the one per-step input of the gen-2 models that is pure
astronomy.  With it a rollout needs the initial condition and a clock: `forcing_batches(times)` is what `forecast.run_forecast` takes
as `forcing_batches`, and `compute_into` writes a plane where a forcing pointer of `wx_rollout` already points.

`TISRForcing` takes the reference's configuration under its names (`num_integration_steps`, `lat_spec`, `lon_spec`; the model time step
as `integration_period`) and makes the reference's checks with its messages.  Reading NetCDF stays with the caller: the grid comes as
arrays (`lat`, `lon`, 1-D for a rectangular grid or 2-D for a curvilinear one) where the reference names `latlon_grid_path`, and the
TSI table as two arrays, `ds["time"]` and `ds["tsi"]` of total_solar_irradiance_CMIP6_49r1.nc (credit/metadata).
No CPU fallback: construction raises without the library or a GPU."""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Iterator, Optional, Sequence

import numpy as np

from .native import NativeHandle, WXEngineError, _check, _f32, _stream_ptr, require_gpu

MAX_STEPS = 2 ** 22 - 1      # kTisrTableEntries - 1


def _axis(name: str, spec: Sequence[float]):
    """tisr.py:356-370: one axis of a rectangular grid from [start, end, num_points]."""
    import torch
    if len(spec) != 3:
        raise ValueError(f"{name} spec must be [start, end, num_points], got {list(spec)!r} ({len(spec)} element(s) instead of 3)")
    start, end = float(spec[0]), float(spec[1])
    n = spec[2]
    if not isinstance(n, int) or isinstance(n, bool):
        raise ValueError(f"{name} spec {list(spec)!r}: num_points must be an int, got {type(n).__name__}")
    if n < 1:
        raise ValueError(f"{name} spec {list(spec)!r}: num_points must be >= 1, got {n}")
    return torch.linspace(start, end, n, dtype=torch.float32)


def latlon_grid(lat=None, lon=None, lat_spec=None, lon_spec=None):
    """tisr.py:284-431 without the file: -> (lat, lon) float32 numpy planes [ny, nx] from exactly one source."""
    import torch
    if (lat_spec is None) != (lon_spec is None):
        raise ValueError("TISR config: 'lat_spec' and 'lon_spec' must be supplied together. "
                         f"Got lat_spec={lat_spec!r}, lon_spec={lon_spec!r}.")
    if (lat is None) != (lon is None):
        raise ValueError("TISR config: 'lat' and 'lon' must be supplied together.")
    if (lat is not None) == (lat_spec is not None):
        raise ValueError("Provide exactly one grid source: either ('lat' and 'lon') or ('lat_spec' and 'lon_spec'), not both or neither.")
    if lat_spec is not None:
        lat_t, lon_t = torch.meshgrid(_axis("lat", lat_spec), _axis("lon", lon_spec), indexing="ij")
        return lat_t.contiguous().numpy(), lon_t.contiguous().numpy()
    lat, lon = np.asarray(lat, dtype=np.float32), np.asarray(lon, dtype=np.float32)
    if lat.ndim > 2 or lon.ndim > 2:
        lat, lon = np.squeeze(lat), np.squeeze(lon)
    if lat.ndim == 2 and lon.ndim == 2:
        if lat.shape != lon.shape:
            raise ValueError(f"2-D lat and lon must have one shape, got {lat.shape} and {lon.shape}")
    elif lat.ndim == 1 and lon.ndim == 1:
        lat, lon = np.meshgrid(lat, lon, indexing="ij")
    else:
        raise ValueError(f"Expected lat/lon to be 1-D or 2-D after squeezing, got lat.ndim={lat.ndim}, lon.ndim={lon.ndim}")
    if lat.size < 1:
        raise ValueError("the lat/lon grid is empty")
    return np.ascontiguousarray(lat), np.ascontiguousarray(lon)


def _period_ns(period) -> int:
    if isinstance(period, (int, np.integer)) and not isinstance(period, bool):
        return int(period)
    import pandas as pd
    return int(pd.Timedelta(period).value)


def times_ns(times) -> list:
    """Target times -> Unix nanoseconds: an int is taken as ns, everything else goes through pd.Timestamp; one time or a sequence."""
    if isinstance(times, (str, bytes)) or not isinstance(times, Iterable):
        times = [times]
    out = []
    for t in times:
        if isinstance(t, (int, np.integer)) and not isinstance(t, bool):
            out.append(int(t))
        else:
            import pandas as pd
            out.append(int(pd.Timestamp(t).value))
    return out


class TISRForcing:
    """credit/datasets/gen_2/tisr.py::TISRDataset on the device, driven by a clock instead of an index."""

    def __init__(self, tsi_times, tsi_values, integration_period, num_integration_steps: int = 360, *, lat=None, lon=None,
                 lat_spec=None, lon_spec=None, source_name: str, device=0):
        if not isinstance(source_name, str) or not source_name:
            raise ValueError("TISRForcing: source_name is required (the data source's name in the config)")
        n = num_integration_steps
        if not isinstance(n, int) or isinstance(n, bool) or n <= 0:
            raise ValueError(f"num_integration_steps must be a positive integer, but got {n}")
        if n > MAX_STEPS:
            raise ValueError(f"num_integration_steps must be at most 2^22 - 1, but got {n}")
        self.num_integration_steps = n
        self.period_ns = _period_ns(integration_period)
        if self.period_ns < n:
            raise ValueError(f"integration_period must hold num_integration_steps = {n} steps of a whole nanosecond, got {self.period_ns} ns")
        self.latitude, self.longitude = latlon_grid(lat, lon, lat_spec, lon_spec)
        self.ny, self.nx = self.latitude.shape
        self.tsi_times = np.ascontiguousarray(np.asarray(tsi_times).reshape(-1), dtype=np.float32)
        self.tsi_values = np.ascontiguousarray(np.asarray(tsi_values).reshape(-1), dtype=np.float32)
        if self.tsi_times.size != self.tsi_values.size:
            raise ValueError(f"tsi_times and tsi_values must have one length, got {self.tsi_times.size} and {self.tsi_values.size}")
        if self.tsi_times.size < 2 or not (np.diff(self.tsi_times) > 0).all():
            raise ValueError("the TSI table needs at least two entries with ascending times")
        self.source_name = source_name
        self.key = f"{source_name}/dynamic_forcing/2d/tisr"
        import torch
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.device = torch.device("cuda", dev.index or 0) if dev.type == "cuda" else dev
        self._handle = self._create_handle()

    def _create_handle(self):
        self.lib = require_gpu("the TISR forcing has no CPU fallback", self.device)
        h = NativeHandle(self.lib.wx_tisr_destroy)
        _check(self.lib.wx_tisr_create(self.ny, self.nx, _f32(self.latitude), _f32(self.longitude), self.tsi_times.size,
                                       _f32(self.tsi_times), _f32(self.tsi_values), self.device.index, h.out))
        return h

    def check_years(self, ns: Sequence[int]) -> None:
        """_get_tsi's guard (tisr.py:245-253) on the first and the last sub-step of every window."""
        y_lo, y_hi = int(self.tsi_times[0]), int(self.tsi_times[-1])
        span = (self.period_ns // self.num_integration_steps) * self.num_integration_steps
        ends = np.asarray(ns, dtype=np.int64)
        years = lambda a: a.astype("datetime64[ns]").astype("datetime64[Y]").astype(np.int64) + 1970   # noqa: E731
        bad = (years(ends - span) < y_lo) | (years(ends) > y_hi)
        if bad.any():
            which = ends[bad].astype("datetime64[ns]")
            raise ValueError(f"{int(bad.sum())} target time(s) have sub-steps outside the TSI data range "
                             f"[{float(self.tsi_times[0]):.4f}, {float(self.tsi_times[-1]):.4f}]: {[str(w) for w in which[:5]]}"
                             + (" ..." if bad.sum() > 5 else ""))

    def _launch(self, ns, base_ptr: int, plane_stride: int) -> None:
        import torch
        arr = (C.c_int64 * len(ns))(*ns)
        with torch.cuda.device(self.device.index):
            _check(self.lib.wx_tisr_compute(self._handle, len(ns), arr, self.period_ns, self.num_integration_steps, C.c_void_p(base_ptr),
                                            plane_stride, _stream_ptr(self.device.index)))

    def compute_into(self, times, dst, channel: Optional[int] = None):
        """Writes the plane of time i into `dst[i]` (dst [n, 1.., ny, nx]) or, with `channel`, into `dst[i, channel]` (dst [n, C, 1..,
        ny, nx], e.g. the slot of a [1, n_dyn, 1, H, W] forcing tensor).  Nothing outside those planes is written.  -> dst"""
        import torch
        ns = times_ns(times)
        self.check_years(ns)
        n = len(ns)
        lead = 1 if channel is None else 2
        if not (isinstance(dst, torch.Tensor) and dst.dtype == torch.float32 and dst.device == self.device and dst.dim() >= lead + 2):
            raise WXEngineError(f"compute_into: dst must be a float32 tensor on {self.device} of at least {lead + 2} dims")
        if tuple(dst.shape[-2:]) != (self.ny, self.nx) or dst.shape[0] != n or any(s != 1 for s in dst.shape[lead:-2]):
            raise WXEngineError(f"compute_into: dst of shape {tuple(dst.shape)} does not hold {n} plane(s) of {self.ny} x {self.nx} "
                                f"as [{n}, {'C, ' if lead == 2 else ''}1.., {self.ny}, {self.nx}]")
        if channel is not None and not 0 <= channel < dst.shape[1]:
            raise WXEngineError(f"compute_into: channel {channel} lies outside dst's {dst.shape[1]} channels")
        first = dst[(0,) * (dst.dim() - 2)] if channel is None else dst[(0, channel) + (0,) * (dst.dim() - 4)]
        if not first.is_contiguous():
            raise WXEngineError("compute_into: a plane of dst must be contiguous memory")
        stride = dst.stride(0) if n > 1 else self.ny * self.nx
        if stride < self.ny * self.nx:
            raise WXEngineError(f"compute_into: dst's planes overlap (stride {stride} < {self.ny * self.nx})")
        self._launch(ns, first.data_ptr(), stride)
        return dst

    def compute(self, times):
        """-> [n, ny, nx] float32 on the device, one plane per target time (the window ends at the time)."""
        import torch
        n = len(times_ns(times))
        return self.compute_into(times, torch.empty((n, self.ny, self.nx), dtype=torch.float32, device=self.device))

    def sample(self, t) -> dict:
        """TISRDataset.__getitem__'s input: the plane as [1, 1, ny, nx] under the reference's key, and the time as Unix ns."""
        (ns,) = times_ns(t)
        return {"input": {self.source_name: {self.key: self.compute([ns]).unsqueeze(0)}}, "metadata": {"input_datetime": ns}}

    def forcing_batches(self, times) -> Iterator[dict]:
        """One collated batch per target time, {"input": {source: {key: [1, 1, 1, ny, nx]}}}, computed when it is asked for."""
        for ns in times_ns(times):
            yield {"input": {self.source_name: {self.key: self.compute([ns]).reshape(1, 1, 1, self.ny, self.nx)}}}
