"""Horizontal regridding of the gen-2 pre-block chain on the device (credit/preblock/regrid.py::Regridder, registry names `regrid`
and `Regridder`; csrc/wx_regrid.h).

`Regridder` takes the reference's argument names and is a callable on the batch dict like the other pre blocks: every listed variable
that is present in `batch[data_type][source]` is multiplied, plane by plane, with the sparse weight matrix of an ESMF weights file.
It is the horizontal half of "put an analysis onto the model's grid" and goes in front of `HybridLevelInterpPre`, the vertical half.
The variables are read where they lie (channel slices of a batch included) and their dict entries are rebound to fresh contiguous
[..., ny, nx] or [..., n_b] tensors: the inputs are never modified.

The weights come as arrays where the reference names a NetCDF file: `row`, `col`, `S` (1-based indices, as ESMF writes them), `n_a`,
`n_b` and optionally `dst_grid_dims`, `xc_b`, `yc_b` are the file's variables under their own names, as `HybridLevelInterp` here takes
its coefficients.  `coalesce_weights` does to them what `sparse_coo_tensor(...).coalesce()` does; `fold_flips` turns the reference's
`torch.flip` of the input into a renumbering of the columns, so nothing is flipped or copied at run time.
No CPU fallback: construction raises without a GPU."""
from __future__ import annotations

import ctypes as C
import logging
from typing import List, Optional, Sequence

import numpy as np

from .native import (HandleCache, WXEngineError, _check, _f32, _i32, _stream_ptr, copy_batch, i32_array, i64_array, load_library,
                     ptr_array, require_gpu)
from .transforms import _check_data_types

logger = logging.getLogger(__name__)

MAX_VARIABLES = 32       # kRegridMaxVars
LIMIT = 2 ** 31 - 1      # n_a, n_b, entries, planes of a variable


def coalesce_weights(row, col, S, n_a: int, n_b: int):
    """regrid.py:55-57 and :123-128 on arrays: the 1-based ESMF triplets -> the coalesced matrix as zero-based CSR
    (row_ptr int64 [n_b + 1], col int32 [nnz], val float32 [nnz]).  The weights are cast to float32 first; the entries are sorted by
    (row, col), stably, and the weights of a repeated (row, col) pair are added in float32 in that order."""
    row = np.asarray(row).reshape(-1).astype(np.int64) - 1
    col = np.asarray(col).reshape(-1).astype(np.int64) - 1
    val = np.asarray(S).reshape(-1).astype(np.float32)
    n_a, n_b = int(n_a), int(n_b)
    if not (1 <= n_a <= LIMIT and 1 <= n_b <= LIMIT):
        raise ValueError(f"coalesce_weights: n_a and n_b must be 1 .. 2^31 - 1, got n_a = {n_a}, n_b = {n_b}")
    if not (row.size == col.size == val.size):
        raise ValueError(f"coalesce_weights: row, col and S must have one length, got {row.size}, {col.size} and {val.size}")
    if row.size > LIMIT:
        raise ValueError(f"coalesce_weights: {row.size} entries; the entry count must stay below 2^31")
    if row.size and (row.min() < 0 or row.max() >= n_b):
        bad = row[(row < 0) | (row >= n_b)][0] + 1
        raise ValueError(f"coalesce_weights: row index {bad} lies outside the destination grid 1 .. n_b = {n_b}")
    if col.size and (col.min() < 0 or col.max() >= n_a):
        bad = col[(col < 0) | (col >= n_a)][0] + 1
        raise ValueError(f"coalesce_weights: col index {bad} lies outside the source grid 1 .. n_a = {n_a}")
    key = row * n_a + col
    order = np.argsort(key, kind="stable")
    key = key[order]
    first = np.ones(key.size, dtype=bool)
    first[1:] = key[1:] != key[:-1]
    slot = np.cumsum(first) - 1                       # the coalesced entry each stored entry goes to
    out = np.zeros(int(first.sum()), dtype=np.float32)
    np.add.at(out, slot, val[order])                  # unbuffered: one float32 addition per entry, in order
    ukey = key[first]
    urow = ukey // n_a
    row_ptr = np.zeros(n_b + 1, dtype=np.int64)
    np.cumsum(np.bincount(urow, minlength=n_b), out=row_ptr[1:])
    return row_ptr, (ukey - urow * n_a).astype(np.int32), out


def fold_flips(col, source_shape: Sequence[int], flips: Sequence[int]):
    """y = W flip(x, flips) is W' x with the flip folded into the column indices: -> the zero-based columns of W'.  `source_shape`
    is the spatial shape of x, (n_a,) or (H, W); `flips` are negative axis numbers inside it.  The entries keep their order."""
    shape = tuple(int(s) for s in source_shape)
    col = np.asarray(col)
    if any(not -len(shape) <= d < 0 for d in flips):
        raise ValueError(f"fold_flips: flips {list(flips)} must be negative axis numbers in [{-len(shape)}, -1]")
    idx = list(np.unravel_index(col.astype(np.int64), shape))
    for d in set(flips):
        idx[d] = shape[d] - 1 - idx[d]
    return np.ravel_multi_index(tuple(idx), shape).astype(col.dtype)


class Regridder:
    """credit/preblock/regrid.py::Regridder on the device."""

    def __init__(self, variables: List[str], row=None, col=None, S=None, n_a: int = None, n_b: int = None, dst_grid_dims=None,
                 xc_b=None, yc_b=None, data_types: Optional[List[str]] = None, reshape_to_xy: bool = True,
                 flip_axis: Optional[List[int]] = None):
        name = "Regridder"
        if variables is None or isinstance(variables, str):
            raise ValueError(f"{name}: variables is required (a list of var_keys)")
        if row is None or col is None or S is None or n_a is None or n_b is None:
            raise ValueError(f"{name}: row, col, S, n_a and n_b are required (arrays and sizes; the reference reads them from weight_file)")
        self.n_a, self.n_b = int(n_a), int(n_b)
        raw_dst = np.zeros(0, dtype=np.int64) if dst_grid_dims is None else np.asarray(dst_grid_dims).reshape(-1)
        if len(raw_dst) == 2:
            dst_shape = raw_dst[::-1]            # [nlon, nlat] -> [nlat, nlon]  (regrid.py:61-63)
        elif reshape_to_xy:
            if xc_b is None or yc_b is None:
                raise ValueError(f"{name}: reshape_to_xy without a length-2 dst_grid_dims needs xc_b and yc_b (the shape comes from "
                                 f"their unique values)")
            dst_shape = np.array([np.unique(np.asarray(yc_b)).size, np.unique(np.asarray(xc_b)).size])     # :64-68
        else:
            dst_shape = None
        grid_type = dst_lat = dst_lon = None
        if dst_shape is not None and int(dst_shape[0]) * int(dst_shape[1]) != self.n_b:
            raise ValueError(f"{name}: the destination shape {tuple(int(s) for s in dst_shape)} does not hold n_b = {self.n_b} points")
        if dst_shape is not None and xc_b is not None and yc_b is not None:        # :79-89
            lat2d = np.asarray(yc_b).reshape(dst_shape)
            lon2d = np.asarray(xc_b).reshape(dst_shape)
            if np.allclose(lat2d, lat2d[:, :1]) and np.allclose(lon2d, lon2d[:1, :]):
                grid_type, dst_lat, dst_lon = "rectilinear", lat2d[:, 0], lon2d[0, :]
            else:
                grid_type, dst_lat, dst_lon = "curvilinear", lat2d, lon2d
        self.variables = list(variables)
        self.data_types = _check_data_types(data_types)
        self.reshape_to_xy = reshape_to_xy
        self.flip_axis = flip_axis
        self.dst_grid_type, self.dst_lat, self.dst_lon = grid_type, dst_lat, dst_lon
        self.dst_shape = dst_shape
        self.row_ptr, self.col, self.val = coalesce_weights(row, col, S, self.n_a, self.n_b)
        self.lib = require_gpu("the regridding block has no CPU fallback", load=load_library)
        self._handles = HandleCache(self.lib, "wx_regrid")   # by (device, spatial shape, kept flips)

    def _handle(self, dev, spatial, flips):
        return self._handles.get((dev, spatial, flips), lambda: (
            self.n_a, self.n_b, self.row_ptr.ctypes.data_as(C.POINTER(C.c_int64)),
            _i32(fold_flips(self.col, spatial, flips) if flips else self.col), _f32(self.val), dev))

    def _plan(self, key, x):
        """regrid.py:139-163 without the arithmetic: -> (handle key, batch, batch stride, planes per item, output shape)."""
        import torch
        if not (isinstance(x, torch.Tensor) and x.dim() >= 1):
            raise WXEngineError(f"{key} must be a float32 tensor on the GPU")
        if x.shape[-1] == self.n_a:
            spatial_dims = 1
        elif len(x.shape) >= 2 and (x.shape[-2] * x.shape[-1]) == self.n_a:
            spatial_dims = 2
        else:
            raise ValueError(f"Cannot map input shape {x.shape} to expected source grid size {self.n_a}.")
        lead_shape = tuple(x.shape[:-spatial_dims])
        flips = ()
        if self.flip_axis is not None:
            requested_flips = list(self.flip_axis)
            valid_flips = [d for d in requested_flips if -spatial_dims <= d < 0]
            if valid_flips != requested_flips:
                logger.warning(
                    "Regridder: ignoring invalid flip_axis values %s; spatial axes must be negative "
                    "indices in [%d, -1].",
                    [d for d in requested_flips if d not in valid_flips],
                    -spatial_dims,
                )
            flips = tuple(sorted(set(valid_flips)))
        planes = int(np.prod(lead_shape, dtype=np.int64)) if lead_shape else 1
        if not 1 <= planes <= LIMIT:
            raise WXEngineError(f"{key}: shape {tuple(x.shape)} holds {planes} planes; one variable takes 1 .. 2^31 - 1")
        if not (x.is_cuda and x.dtype == torch.float32):
            raise WXEngineError(f"{key} must be a float32 tensor on the GPU")
        if x.is_contiguous():
            batch, bstride, ppi = 1, 0, planes
        elif lead_shape and x[0].is_contiguous():
            batch, bstride, ppi = lead_shape[0], x.stride(0), planes // lead_shape[0]
        else:
            raise WXEngineError(f"{key}: a batch item must be contiguous memory (the tensor, or each x[b], contiguous)")
        if self.reshape_to_xy and self.dst_shape is not None:
            out_shape = lead_shape + (int(self.dst_shape[0]), int(self.dst_shape[1]))
        else:
            out_shape = lead_shape + (self.n_b,)
        return (x.device.index, tuple(x.shape[-spatial_dims:]), flips), batch, bstride, ppi, out_shape

    def _regrid_many(self, named):
        """[(var_key, tensor)] -> [regridded tensor]: the variables that share a handle and a batch count go to one wx_regrid_apply,
        in chunks of MAX_VARIABLES."""
        import torch
        plans = [self._plan(k, x) for k, x in named]
        outs = [None] * len(named)
        calls = {}
        for i, (hkey, batch, _, _, _) in enumerate(plans):
            calls.setdefault((hkey, batch), []).append(i)
        for (hkey, batch), members in calls.items():
            h = self._handle(*hkey)
            for c0 in range(0, len(members), MAX_VARIABLES):
                chunk = members[c0:c0 + MAX_VARIABLES]
                for i in chunk:
                    outs[i] = torch.empty(plans[i][4], dtype=torch.float32, device=named[i][1].device)
                with torch.cuda.device(hkey[0]):
                    _check(self.lib.wx_regrid_apply(h, len(chunk), ptr_array([named[i][1] for i in chunk]), i64_array([plans[i][2] for i in chunk]),
                                                    i32_array([plans[i][3] for i in chunk]), batch, ptr_array([outs[i] for i in chunk]),
                                                    _stream_ptr(hkey[0])))
        return outs

    def _regrid(self, x):
        """regrid.py:134-175 for one tensor."""
        return self._regrid_many([("the input", x)])[0]

    def __call__(self, batch: dict) -> dict:
        batch = copy_batch(batch, self.data_types)
        for data_type in self.data_types:
            if data_type not in batch:
                continue            # absent (no "target" at inference)
            present = []
            for var_key in self.variables:
                source = var_key.split("/")[0]
                if source not in batch[data_type]:
                    raise KeyError(f"Regridder: source '{source}' not found in batch['{data_type}'].")
                if var_key in batch[data_type][source]:     # absent in this data type (statics exist in "input" only): skipped
                    present.append((var_key, batch[data_type][source][var_key]))
            if present:
                for (var_key, _), y in zip(present, self._regrid_many(present)):
                    batch[data_type][var_key.split("/")[0]][var_key] = y
        return batch

    forward = __call__
