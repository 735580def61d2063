"""Input side of the step on the device: host mirror of the reference's preblocks.

`DevicePreblock` takes the nested batch dict the reference's dataloader produces
(`batch["input"][source][var_key] -> tensor [B, n_levels, T, H, W]`, var_key = "source/field_type/dim/varname"),
orders the variables exactly like `credit/preblock/concat.py::_channel_sort_key` (:22-31: field-type rank
prognostic < static < dynamic_forcing < diagnostic from `credit/datasets/gen_2/channel_utils.py:88-93`, 3d before 2d,
otherwise insertion order -- Python's sort is stable), normalises them like
`credit/preblock/norm.py::ERA5Normalizer._normalize_tensor` (:78-98) and concatenates along the channel dim like
`ConcatToTensor.forward` (:96-207) -- the last two in ONE kernel pass through the C ABI (`wx_pre_*`).  It also returns the
reference's `_channel_map` (var_key -> {"slice", "orig_shape"}).  With `transforms=[...]` (the FillValues / LogTransform /
SqrtTransform descriptors of wxengine/transforms.py) the same single pass also fills and log- / sqrt-transforms the selected
variables in front of the normalisation: the gen-2 chain fill_values -> log_transform | sqrt_transform -> scaler -> concat.
No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict, Optional

import numpy as np

from .native import NativeHandle, WXEngineError, _check, _f32, _i32, _stream_ptr, require_gpu

FIELD_TYPE_RANK = {"prognostic": 0, "static": 1, "dynamic_forcing": 2, "diagnostic": 3}


def channel_sort_key(var_key: str):
    parts = var_key.split("/")
    ft = parts[1] if len(parts) > 1 else ""
    dim = parts[2] if len(parts) > 2 else ""
    return (FIELD_TYPE_RANK.get(ft, len(FIELD_TYPE_RANK)), 0 if dim == "3d" else 1)


def ordered_keys(sources: Dict[str, Dict]) -> list:
    """Concatenation order of `batch["input"]`: sources in insertion order, variables sorted (stably) inside each."""
    out = []
    for _source, variables in sources.items():
        out += sorted(variables.keys(), key=channel_sort_key)
    return out


def _level_stats(key, nl, value, neutral):
    """One statistic of one variable as an [nl] float32 vector: a scalar serves every level, None is `neutral`."""
    if value is None:
        return np.full(nl, neutral, np.float32)
    a = np.asarray(value, np.float32).ravel()
    if a.size == 1:
        a = np.repeat(a, nl)
    if a.size != nl:
        raise ValueError(f"{key}: {a.size} statistics for {nl} levels")
    return a


def channel_stats(keys, levels, mean: Optional[Dict], std: Optional[Dict]):
    """Per-output-channel (mean, std) from per-variable stats (scalar or per-level vectors); variables without stats
    pass through unchanged (norm.py:84-85) = mean 0, std 1."""
    if mean is None:
        return None, None
    names = [k.split("/")[-1] for k in keys]
    m = [_level_stats(k, nl, mean.get(n), 0.0) for k, n, nl in zip(keys, names, levels)]
    s = [_level_stats(k, nl, std[n] if n in mean else None, 1.0) for k, n, nl in zip(keys, names, levels)]
    return np.concatenate(m).astype(np.float32), np.concatenate(s).astype(np.float32)


class DevicePreblock:
    def __init__(self, example_input: Dict[str, Dict], mean: Optional[Dict] = None, std: Optional[Dict] = None,
                 device: Optional[int] = None, transforms=None):
        """`transforms`: descriptors in chain order, compiled against `example_input` (wxengine/transforms.py::compile_channel_table;
        orders the fused kernel does not serve are a ValueError here).  None or [] = the plain normalise + concatenate kernel.
        `device`: GPU index the block lives on; default = the device of the example tensors when they are on a GPU, else the
        current device (rank r of a replicas run works on cuda:r -- a block pinned to GPU 0 would launch on another device's
        stream there)."""
        import torch
        self.lib = require_gpu("the device preblock has no CPU fallback")
        self.keys = ordered_keys(example_input)
        flat = {k: v for src in example_input.values() for k, v in src.items()}
        if device is None:
            on_gpu = [v.device.index for v in flat.values() if getattr(v, "is_cuda", False)]
            device = on_gpu[0] if on_gpu else torch.cuda.current_device()
        self.device = int(device)
        shp = [tuple(flat[k].shape) for k in self.keys]
        if any(len(s) != 5 for s in shp) or len({(s[2], s[3], s[4]) for s in shp}) != 1:
            raise ValueError("fields must be [B, n_levels, T, H, W] on one grid")
        self.levels = [s[1] for s in shp]
        self.T, self.H, self.W = shp[0][2:]
        self.mean, self.std = channel_stats(self.keys, self.levels, mean, std)
        self.channel_map = OrderedDict()
        cur = 0
        for k, nl in zip(self.keys, self.levels):
            # ConcatToTensor flattens (levels x T) per variable in its map; the tensor itself stays [B, C, T, H, W]
            self.channel_map[k] = {"slice": slice(cur, cur + nl * self.T), "orig_shape": (nl, self.T)}
            cur += nl * self.T
        self.channels = sum(self.levels)
        from .transforms import compile_channel_table
        self.transform_table = compile_channel_table(transforms, example_input, self.keys, self.levels) if transforms else None
        self._p = NativeHandle(self.lib.wx_pre_destroy)
        _check(self.lib.wx_pre_create(len(self.levels), _i32(self.levels), self.T, self.H, self.W, _f32(self.mean), _f32(self.std),
                                      self.device, self._p.out))
        if self.transform_table is not None:
            t = self.transform_table
            _check(self.lib.wx_pre_set_transforms(self._p, _i32(t["kind"]), _f32(t["eps"]), _f32(t["log_eps"]), _i32(t["n_rules"]),
                                                  _i32(t["rule_op"]), _f32(t["rule_search"]), _f32(t["rule_fill"])))

    def __call__(self, batch_input: Dict[str, Dict]):
        """-> x [B, C, T, H, W] float32 on the GPU (normalised + concatenated)."""
        import torch
        flat = {k: v for src in batch_input.values() for k, v in src.items()}
        ts = []
        for k, nl in zip(self.keys, self.levels):
            t = flat[k]
            if not t.is_cuda:
                t = t.cuda(self.device, non_blocking=True)
            elif t.device.index != self.device:
                raise WXEngineError(f"{k} is on cuda:{t.device.index} but this preblock was created for cuda:{self.device}")
            t = t.contiguous().float()
            if tuple(t.shape[1:]) != (nl, self.T, self.H, self.W):
                raise ValueError(f"{k}: shape {tuple(t.shape)} does not match the schema")
            ts.append(t)
        B = ts[0].shape[0]
        x = torch.empty((B, self.channels, self.T, self.H, self.W), dtype=torch.float32, device=ts[0].device)
        ptrs = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        with torch.cuda.device(self.device):   # the entry point selects its own device; keep torch's notion of "current" intact
            _check(self.lib.wx_pre_apply(self._p, ptrs, C.c_void_p(x.data_ptr()), B, _stream_ptr(self.device)))
        return x
