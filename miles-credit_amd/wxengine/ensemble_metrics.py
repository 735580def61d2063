"""Ensemble verification on the device (csrc/wx_ensemble.h): CRPS, spread and ensemble-mean error of M members against the truth.

One reading pass over the members and the truth where they lie in HBM gives, per plane (variable, b, level, t), six float64 sums;
everything the reference reports is arithmetic on that plane table, done here on the host:

    credit/losses/gen_1/kcrps.py                  KCRPSLoss(biased=True / False)(y, x).mean()       -> "crps/{var}", "fair_crps/{var}"
    credit/losses/gen_1/almost_fair_crps.py       AlmostFairKCRPSLoss(alpha)(y, x)                  -> "afcrps/{var}"
    credit/ensemble/crps.py                       calculate_crps_per_channel                        -> "crps_per_channel/{var}" (array over levels)
    credit/applications/rollout_metrics_noisy_model.py:107  calculate_ensemble_metrics              -> "ens_rmse/{var}", "ens_spread/{var}", each also
                                                                                                       ".../{var}/{level}"
    credit/applications/rollout_metrics_noisy_model.py:53   compute_spread_skill_metric             -> "spread_skill/{var}"
    credit/metrics/gen_1/metrics.py:247           LatWeightedMetricsEnsemble                        -> result.maps["ens_mean" | "ens_std" | "ens_abs_err"],
                                                                                                       their means "ens_abs_err/{var}", "ens_std/{var}"

    verifier = EnsembleVerification(n_members=16, alpha=0.95, maps=("crps", "ens_std"))
    scores = verifier(members, target)                   # the drop-in
    pending = verifier.submit(members, target)           # in a rollout: kernels and an async copy on the current stream, no sync
    ...
    scores = pending.result()                            # waits on its event; scores.planes[var], scores.maps[name][var]

`members` is a list of M dicts {var_key: [B, L, T, H, W]} (or nested {source: {var: ...}} like y_processed) -- the separate buffers
of `ensemble_rollout` -- or ONE dict of [B * M, L, T, H, W] tensors in the reference's layout (member m of item b is row b * M + m).
Both are read in place and give the same bits.  With latitude weights every sum carries w[h] (not divided by the sum of w, the
convention of wxengine.metrics); the maps are per grid point and carry none.  No CPU fallback: construction raises without a GPU."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from .native import (HandleCache, PendingResult, WXEngineError, _check, _f32, _stream_ptr, batch_stride, copy_out, flatten_named,
                     i32_array, i64_array, ptr_array, require_gpu)

MAX_VARIABLES = 32      # kEnsMaxVars
MAX_MEMBERS = 64        # kEnsMaxMembers
SUM_ORDER = ("skill", "pair", "err2", "abs_err", "ss", "std")                          # a row of the plane table
MAP_ORDER = ("ens_mean", "ens_std", "ens_abs_err", "crps", "fair_crps", "afcrps")      # the map slots of wx_ensemble_apply
SCALAR_ORDER = ("crps", "fair_crps", "afcrps", "ens_rmse", "ens_spread", "spread_skill", "ens_abs_err", "ens_std")
PER_LEVEL = ("ens_rmse", "ens_spread")


def check_arguments(n_members, alpha=1.0, maps=()):
    """The constructor's checks, without a device.  -> (n_members, alpha, maps as a tuple in MAP_ORDER)."""
    if int(n_members) != n_members or not 2 <= int(n_members) <= MAX_MEMBERS:
        raise ValueError(f"EnsembleVerification: n_members must be an integer in 2..{MAX_MEMBERS}; got {n_members!r}")
    alpha = float(alpha)
    if not np.isfinite(alpha):
        raise ValueError(f"EnsembleVerification: alpha must be finite; got {alpha!r}")
    maps = (maps,) if isinstance(maps, str) else tuple(maps)
    for name in maps:
        if name not in MAP_ORDER:
            raise ValueError(f"EnsembleVerification: unknown map {name!r}; the device block writes {list(MAP_ORDER)}")
    return int(n_members), alpha, tuple(name for name in MAP_ORDER if name in maps)


def flatten_state(state: dict, name: str) -> dict:
    """{var: tensor} of a flat or a nested {source: {var: tensor}} dict."""
    return flatten_named(state, name, "EnsembleVerification")


def member_table(members, n_members: int, var_keys: Sequence[str]):
    """The pointer and stride table of wx_ensemble_apply for both member layouts, from anything with data_ptr / stride / shape /
    element_size (no device needed).  -> per variable dict(ptrs=[M addresses], batch_stride=floats between batch items of ONE member,
    shape=(B, L, T, H, W)).  A list of M dicts: member m's tensor is its own buffer.  One dict: [B * M, L, T, H, W], member m of item b
    in row b * M + m, so the pointer is row m and the batch stride M rows."""
    M = n_members
    table = []
    if isinstance(members, dict):
        flat = flatten_state(members, "members")
        for k in var_keys:
            if k not in flat:
                raise KeyError(f"EnsembleVerification: variable '{k}' missing from the members")
            x = flat[k]
            if len(x.shape) != 5 or x.shape[0] % M:
                raise ValueError(f"{k}: the stacked layout is [B * n_members, L, T, H, W] with n_members = {M}; got {tuple(x.shape)}")
            row = x.stride(0)
            table.append(dict(ptrs=[x.data_ptr() + m * row * x.element_size() for m in range(M)], batch_stride=M * row,
                              shape=(x.shape[0] // M,) + tuple(x.shape[1:])))
        return table
    if len(members) != M:
        raise ValueError(f"EnsembleVerification: {len(members)} member dicts for n_members = {M}")
    flats = [flatten_state(m, "members") for m in members]
    for k in var_keys:
        xs = []
        for m, flat in enumerate(flats):
            if k not in flat:
                raise KeyError(f"EnsembleVerification: variable '{k}' missing from member {m}")
            xs.append(flat[k])
        if any(len(x.shape) != 5 or tuple(x.shape) != tuple(xs[0].shape) for x in xs):
            raise ValueError(f"{k}: every member must be one [B, L, T, H, W] shape; got {[tuple(x.shape) for x in xs]}")
        if xs[0].shape[0] > 1 and any(x.stride(0) != xs[0].stride(0) for x in xs):
            raise ValueError(f"{k}: the members' batch strides differ: {[x.stride(0) for x in xs]}")
        table.append(dict(ptrs=[x.data_ptr() for x in xs], batch_stride=xs[0].stride(0), shape=tuple(xs[0].shape)))
    return table


def result_keys(levels: Dict[str, int]) -> List[str]:
    """The keys of a result in order: per score every variable (ens_rmse and ens_spread followed by their levels), then the
    per-channel CRPS arrays.  levels: {var_key: n_levels} in variable order."""
    keys = []
    for name in SCALAR_ORDER:
        for k, L in levels.items():
            keys.append(f"{name}/{k}")
            if name in PER_LEVEL:
                keys += [f"{name}/{k}/{lev}" for lev in range(L)]
    return keys + [f"crps_per_channel/{k}" for k in levels]


def scores_from_planes(planes: Dict[str, np.ndarray], n_members: int, alpha: float, n_points: int) -> dict:
    """The host formulas.  planes: {var_key: float64 [B, L, T, 6]} in SUM_ORDER, n_points = H * W.  Every mean divides by the number
    of elements (never by the sum of the weights)."""
    M = float(n_members)
    per_var = {}
    for k, tab in planes.items():
        tab = np.asarray(tab, dtype=np.float64)
        if tab.ndim != 4 or tab.shape[-1] != len(SUM_ORDER):
            raise ValueError(f"{k}: a plane table is [B, L, T, {len(SUM_ORDER)}]; got {tab.shape}")
        s = {name: tab[..., i] / n_points for i, name in enumerate(SUM_ORDER)}         # plane means
        skill = s["skill"] / M
        fair_spread = s["pair"] / (M * (M - 1.0))
        crps_plane = skill - s["pair"] / (M * M)
        rmse_plane, spread_plane = np.sqrt(s["err2"]), np.sqrt(s["ss"] / M)
        v = {"crps": crps_plane.mean(), "fair_crps": (skill - fair_spread).mean(),
             "afcrps": (skill - (1.0 - (1.0 - alpha) / M) * fair_spread).mean(),
             "ens_rmse": rmse_plane.mean(), "ens_spread": spread_plane.mean(),
             "ens_abs_err": s["abs_err"].mean(), "ens_std": s["std"].mean(),
             "ens_rmse_levels": rmse_plane.mean(axis=(0, 2)), "ens_spread_levels": spread_plane.mean(axis=(0, 2)),
             "crps_per_channel": crps_plane.mean(axis=(0, 2))}
        v["spread_skill"] = (M + 1.0) / (M - 1.0) * v["ens_spread"] / v["ens_rmse"] if v["ens_rmse"] > 0 else float("nan")
        per_var[k] = v
    out = {}
    for name in SCALAR_ORDER:
        for k, v in per_var.items():
            out[f"{name}/{k}"] = float(v[name])
            if name in PER_LEVEL:
                for lev, x in enumerate(v[name + "_levels"]):
                    out[f"{name}/{k}/{lev}"] = float(x)
    for k, v in per_var.items():
        out[f"crps_per_channel/{k}"] = np.array(v["crps_per_channel"], dtype=np.float64)
    return out


class EnsembleScores(dict):
    """The result of one call: the scores by key; `planes[var]` the raw float64 plane table [B, L, T, 6] (SUM_ORDER); `maps[name][var]`
    the requested maps, float32 [B, L, T, H, W] tensors on the device."""

    def __init__(self, scores, planes, maps, n_members):
        super().__init__(scores)
        self.planes, self.maps, self.n_members = planes, maps, n_members

    def reference_ens_std(self, var_key):
        """LatWeightedMetricsEnsemble's "ens_std" (metrics.py:306): torch.std times (M + 1) / (M - 1)."""
        if "ens_std" not in self.maps:
            raise KeyError("reference_ens_std needs the 'ens_std' map: EnsembleVerification(..., maps=('ens_std',))")
        return self.maps["ens_std"][var_key] * (self.n_members + 1) / (self.n_members - 1)


class PendingEnsembleScores(PendingResult):
    """The scores of one `submit`: kernels and the copy of the plane table into a pinned buffer are enqueued, `result()` waits and is
    the EnsembleScores."""

    def __init__(self, owner, pinned, event, shapes, maps, keep):
        def finish(table):
            planes, row = {}, 0
            for k, (B, L, T, H, W) in shapes.items():
                planes[k] = table[row:row + B * L * T].reshape(B, L, T, len(SUM_ORDER)).copy()
                row += B * L * T
            H, W = next(iter(shapes.values()))[3:]
            return EnsembleScores(scores_from_planes(planes, owner.n_members, owner.alpha, H * W), planes, maps, owner.n_members)
        super().__init__(pinned, event, finish, keep)


class EnsembleVerification:
    def __init__(self, n_members: int, alpha: float = 1.0, use_latitude_weights: bool = False, latitude=None, maps=()):
        self.n_members, self.alpha, self.maps = check_arguments(n_members, alpha, maps)
        self.lat_weights = None
        if use_latitude_weights:
            if latitude is None:
                raise ValueError("latitude (degrees) is required when use_latitude_weights=True.")
            from .metrics import cos_lat_weights
            self.lat_weights = cos_lat_weights(latitude)
        self.lib = require_gpu("the ensemble verification has no CPU fallback")
        self._handles = HandleCache(self.lib, "wx_ensemble")   # by (H, W, device)

    def _handle(self, H, W, dev):
        def args():
            if self.lat_weights is not None and self.lat_weights.numel() != H:
                raise ValueError(f"EnsembleVerification: {self.lat_weights.numel()} latitudes but the fields have {H} rows")
            return H, W, _f32(None if self.lat_weights is None else self.lat_weights.numpy()), self.n_members, dev
        return self._handles.get((H, W, dev), args)

    def _on_device(self, x, what, device=None):
        import torch
        if not isinstance(x, torch.Tensor) or (device is None and not x.is_cuda):
            raise WXEngineError(f"{what} must be a 5-D tensor on the GPU")
        x = x.float() if device is None else x.float().to(device)
        if x.dim() != 5:
            raise WXEngineError(f"{what}: expected 5 dimensions, got {tuple(x.shape)}")
        return x if x[0].is_contiguous() else x.contiguous()

    def submit(self, members, target: dict) -> PendingEnsembleScores:
        import torch
        M = self.n_members
        tgt = flatten_state(target, "target")
        var_keys = sorted(tgt)
        with torch.no_grad():
            if isinstance(members, dict):
                flat = flatten_state(members, "members")
                for k in var_keys:
                    if k not in flat:
                        raise KeyError(f"EnsembleVerification: variable '{k}' missing from the members")
                members = {k: self._on_device(flat[k], k) for k in var_keys}
                first = members[var_keys[0]]
            else:
                if len(members) != M:
                    raise ValueError(f"EnsembleVerification: {len(members)} member dicts for n_members = {M}")
                flats = [flatten_state(m, "members") for m in members]
                for m, flat in enumerate(flats):
                    for k in var_keys:
                        if k not in flat:
                            raise KeyError(f"EnsembleVerification: variable '{k}' missing from member {m}")
                members = [{k: self._on_device(flat[k], k) for k in var_keys} for flat in flats]
                for k in var_keys:          # one batch stride per variable: members that disagree are made contiguous
                    if members[0][k].shape[0] > 1 and len({m[k].stride(0) for m in members}) > 1:
                        for m in members:
                            m[k] = m[k].contiguous()
                first = members[0][var_keys[0]]
            device = first.device
            table = member_table(members, M, var_keys)
            truth = [self._on_device(tgt[k], f"target {k}", device) for k in var_keys]
            B, _, _, H, W = table[0]["shape"]
            for k, row, t in zip(var_keys, table, truth):
                if tuple(t.shape) != row["shape"]:
                    raise WXEngineError(f"{k}: members {row['shape']} and target {tuple(t.shape)} must be one [B, n_levels, n_time, H, W] shape")
                if (row["shape"][0], row["shape"][3], row["shape"][4]) != (B, H, W):
                    raise WXEngineError(f"{k}: {row['shape']}; all variables of one call share the batch size and H x W of "
                                        f"{var_keys[0]}: {table[0]['shape']}")
            every = members.values() if isinstance(members, dict) else [x for m in members for x in m.values()]
            if any(x.device != device for x in every):
                raise WXEngineError("EnsembleVerification: all members must be on one device")
            dev = device.index
            h = self._handle(H, W, dev)
            n = len(var_keys)
            shapes = {k: row["shape"] for k, row in zip(var_keys, table)}
            n_planes = [s[0] * s[1] * s[2] for s in shapes.values()]
            planes = torch.empty((sum(n_planes), len(SUM_ORDER)), dtype=torch.float64, device=device)
            maps = {name: {k: torch.empty(shapes[k], dtype=torch.float32, device=device) for k in var_keys} for name in self.maps}
            with torch.cuda.device(dev):
                row0 = 0
                for v0 in range(0, n, MAX_VARIABLES):
                    sl = slice(v0, min(n, v0 + MAX_VARIABLES))
                    k = sl.stop - sl.start
                    ptrs = (C.c_void_p * (k * M))(*[p for row in table[sl] for p in row["ptrs"]])
                    map_ptrs = None
                    if self.maps:
                        map_ptrs = ptr_array([maps[name][key] if name in maps else None for key in var_keys[sl] for name in MAP_ORDER])
                    _check(self.lib.wx_ensemble_apply(
                        h, k, ptrs, i64_array([row["batch_stride"] if B > 1 else 0 for row in table[sl]]),
                        ptr_array(truth[sl]), i64_array([batch_stride(t, B) for t in truth[sl]]),
                        i32_array([row["shape"][1] for row in table[sl]]), i32_array([row["shape"][2] for row in table[sl]]),
                        B, self.alpha, map_ptrs, C.c_void_p(planes[row0].data_ptr()), _stream_ptr(dev)))
                    row0 += sum(n_planes[sl])
                pinned, event = copy_out(planes, dev)
        return PendingEnsembleScores(self, pinned, event, shapes, maps, (members, truth, planes))

    def __call__(self, members, target: dict) -> EnsembleScores:
        return self.submit(members, target).result()

    forward = __call__
