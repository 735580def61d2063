"""Gen-2 verification metrics on the device (credit/metrics/base.py, common.py, anomaly.py; csrc/wx_metrics.h).

`CombinedMetric` takes the arguments of the reference's `BaseCombinedMetric` and is called on the trainer's `full_data_dict` like it:
every variable of `y_processed` is scored against `y_target_processed`, the per-variable scores are combined with the static
weights of `_build_static_weights`, and the returned dict has the reference's keys in the reference's order -- per metric
`"{metric}/{var_key}"` for every variable, then `"{metric}"`.  Where the reference runs three to eight elementwise torch passes and
one `.item()` per metric and variable, all eight scores of up to 32 variables come from ONE device call (two reading passes, fp64
sums), and a call of this class makes one device-to-host copy of [n_vars, 8] floats and one sync:

    metric = CombinedMetric({"rmse": {}, "acc": {"climatology": clim}}, var_weighting="none", use_latitude_weights=True, latitude=lat)
    scores = metric(full_data_dict)                      # the drop-in
    pending = metric.submit(full_data_dict)              # in a rollout: kernels and an async copy on the current stream, no sync
    ...
    scores = pending.result()                            # waits on its event, builds the same dict

Arrays stand where the reference names files: `variances` ({var_key: float}) for `scaler_path`, `latitude` (degrees) for the
`latitude_weights` path, `data_var_keys` (a list) for `channel_schema`, and per metric `climatology` ({var_key or short name: array
or tensor, (lat, lon) or (level, lat, lon)}) for `climatology_path`.  The online climatology (the running sum of the targets over
calls, or the per-call target mean with `accumulate_climatology=False`) is bookkeeping in torch on the device; the kernel sees a
pointer with strides.  Latitude-sharded scoring (lat-band mode) is out of scope.  No CPU fallback: construction raises without a GPU."""
from __future__ import annotations

import ctypes as C
import logging
from typing import Dict, List, Optional

import numpy as np

from .native import (HandleCache, PendingResult, WXEngineError, _check, _f32, _stream_ptr, batch_stride, copy_out, flatten_named,
                     i32_array, i64_array, load_library, ptr_array, require_gpu)

logger = logging.getLogger(__name__)

MAX_VARIABLES = 32     # kMetricsMaxVars
# the order of a scores row (csrc/wx_metrics.h) and the power of sigma each score carries (BaseVariableMetric.scale_power)
METRIC_ORDER = ("rmse", "mse", "mae", "bias", "r2score", "log_variance_ratio", "acc", "activity")
SCALE_POWER = {"rmse": 1, "mse": 2, "mae": 1, "bias": 1, "r2score": 0, "log_variance_ratio": 0, "acc": 0, "activity": 1}
VAR_WEIGHTING_MODES = ("inverse_variance", "manual", "none")
ANOMALY_METRICS = ("acc", "activity")
_SHARED = ("include_computed_diagnostics", "use_latitude_weights", "latitude", "data_var_keys")
_PER_METRIC = {"eps": ("log_variance_ratio",), "climatology": ANOMALY_METRICS, "accumulate_climatology": ANOMALY_METRICS,
               "climatology_path": ANOMALY_METRICS}
_WEIGHTING = ("var_weighting", "variances", "variable_weights", "normalize_weights")


def cos_lat_weights(latitude):
    """credit/losses/base.py::_cos_lat_weights on an array of degrees: cos(deg2rad(lat)) / mean, float32, by the same torch calls."""
    import torch
    lat = torch.tensor(np.asarray(latitude, dtype=np.float64).reshape(-1), dtype=torch.float32)
    weights = torch.cos(torch.deg2rad(lat))
    return weights / weights.mean()


def _same_climatology(a, b) -> bool:
    if a is b:
        return True
    if a is None or b is None or set(a) != set(b):
        return False
    return all(a[k] is b[k] or (tuple(a[k].shape) == tuple(b[k].shape) and np.array_equal(np.asarray(a[k]), np.asarray(b[k]))) for k in a)


class _Weighting:
    """The combination weighting of ONE metric: BaseVariableMetric.__init__ and _build_static_weights (base.py:194-231, :277-310)."""

    def __init__(self, metric_name, var_weighting, variances, variable_weights, normalize_weights):
        self.metric_name = metric_name
        self.scale_power = SCALE_POWER[metric_name]
        if var_weighting == "learnable":
            raise ValueError("CombinedMetric: var_weighting='learnable' is not supported for metrics "
                             "(metrics are not optimized). Use 'inverse_variance', 'manual', or 'none'.")
        if var_weighting not in VAR_WEIGHTING_MODES:
            raise ValueError(f"var_weighting must be one of {VAR_WEIGHTING_MODES}; got {var_weighting!r}")
        self.var_weighting = var_weighting
        self.manual_weights = {k: float(v) for k, v in (variable_weights or {}).items()}
        self.normalize_weights = bool(normalize_weights)
        self._variances = None
        if var_weighting == "inverse_variance" and self.scale_power != 0:      # a dimensionless metric never consults the variances
            if not variances:
                raise ValueError(f"variances is required for var_weighting='{var_weighting}' with metric '{metric_name}' "
                                 f"(scale_power={self.scale_power}).")
            self._variances = {k: float(v) for k, v in variances.items()}

    def build(self, var_keys) -> Dict[str, float]:
        weights = {}
        for var_key in var_keys:
            manual = self.manual_weights.get(var_key, 1.0)
            if self.var_weighting == "inverse_variance":
                if self.scale_power == 0:
                    weights[var_key] = manual
                    continue
                variance = self._variances.get(var_key)
                if variance is None:
                    logger.warning("CombinedMetric: no variance found for '%s'; falling back to weight 1.0. "
                                   "Add it to variances or set a manual entry in variable_weights.", var_key)
                    weights[var_key] = manual
                else:
                    weights[var_key] = manual / max(variance, 1e-12) ** (self.scale_power / 2)
            elif self.var_weighting == "manual":
                if var_key not in self.manual_weights:
                    logger.warning("CombinedMetric: no variable_weights entry for '%s'; using 1.0.", var_key)
                weights[var_key] = manual
            else:
                weights[var_key] = manual
        if self.normalize_weights:
            mean_w = sum(weights.values()) / len(weights)
            if mean_w > 0:
                weights = {k: v / mean_w for k, v in weights.items()}
        return weights


class PendingScores(PendingResult):
    """The scores of one `submit`: kernels and the copy into a pinned buffer are enqueued, `result()` waits for them and is the dict."""

    def __init__(self, owner: "CombinedMetric", pinned, event, var_keys):
        super().__init__(pinned, event, lambda scores: owner._combine(scores, var_keys))


class CombinedMetric:
    """credit/metrics/base.py::BaseCombinedMetric over the registry's rmse, mse, mae, bias, r2score, log_variance_ratio, acc and
    activity, on the device."""

    def __init__(self, metrics: dict, var_weighting: str = "inverse_variance", variances: Optional[dict] = None,
                 variable_weights: Optional[dict] = None, normalize_weights: bool = True, include_computed_diagnostics: bool = True,
                 use_latitude_weights: bool = False, latitude=None, data_var_keys: Optional[List[str]] = None):
        if not metrics:
            raise ValueError("CombinedMetric: 'metrics' must list at least one metric.")
        shared = dict(var_weighting=var_weighting, variances=variances, variable_weights=variable_weights,
                      normalize_weights=normalize_weights)
        self.metric_names = list(metrics)
        self.weightings: Dict[str, _Weighting] = {}
        self.eps = 1e-12
        anomaly_args = {}
        for name, per_metric in metrics.items():
            if name not in METRIC_ORDER:
                raise ValueError(f"CombinedMetric: unknown metric {name!r}; the device block scores {list(METRIC_ORDER)}")
            args = dict(per_metric or {})
            for key in args:
                if key in _SHARED:
                    raise ValueError(f"CombinedMetric: {key!r} is shared by every metric (one pass scores them all); "
                                     f"give it to CombinedMetric, not to {name!r}")
                if key in _PER_METRIC and name not in _PER_METRIC[key]:
                    raise ValueError(f"CombinedMetric: {key!r} is not an argument of {name!r}")
                if key not in _PER_METRIC and key not in _WEIGHTING:
                    raise ValueError(f"CombinedMetric: unknown argument {key!r} of {name!r}")
            if args.get("climatology_path"):
                raise ValueError(f"CombinedMetric: {name!r}: climatology_path is not read here; pass the fields as arrays in "
                                 "climatology={var_key or short name: array (lat, lon) or (level, lat, lon)}")
            w = dict(shared)
            w.update({k: args[k] for k in _WEIGHTING if k in args})
            self.weightings[name] = _Weighting(name, **w)
            if name == "log_variance_ratio":
                self.eps = float(args.get("eps", 1e-12))
            if name in ANOMALY_METRICS:
                anomaly_args[name] = (args.get("climatology"), bool(args.get("accumulate_climatology", True)))
        self.need_climatology = bool(anomaly_args)
        if len(anomaly_args) == 2:
            (ca, aa), (cb, ab) = anomaly_args["acc"], anomaly_args["activity"]
            if not _same_climatology(ca, cb) or aa != ab:
                raise ValueError("CombinedMetric: 'acc' and 'activity' must be given the same climatology (and the same "
                                 "accumulate_climatology): one pass over one climatology serves both")
        clim, self.accumulate_climatology = next(iter(anomaly_args.values())) if anomaly_args else (None, True)
        import torch
        self._climatology = {}
        if clim is not None:
            self._climatology = {k: torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).float() for k, v in clim.items()}
        self._clim_sum: Dict[str, "torch.Tensor"] = {}
        self._clim_count = 0
        self.include_computed_diagnostics = bool(include_computed_diagnostics)
        self.lat_weights = None
        if use_latitude_weights:
            if latitude is None:
                raise ValueError("latitude (degrees) is required when use_latitude_weights=True.")
            self.lat_weights = cos_lat_weights(latitude)
        self.data_var_keys = list(data_var_keys) if data_var_keys is not None else None
        self.var_keys = None
        self._combination_weights = None
        self.last_var_scores = {name: {} for name in self.metric_names}
        self._clim_on = {}
        self.lib = require_gpu("the verification metrics have no CPU fallback", load=load_library)
        self._handles = HandleCache(self.lib, "wx_metrics")   # by (H, W, device)

    # ---- setup (base.py:263-310) ----------------------------------------------------------------------------------------------------
    def _resolve_var_keys(self, pred: dict, target: dict) -> list:
        var_keys = list(self.data_var_keys) if self.data_var_keys is not None else sorted(target.keys())
        have = set(var_keys)
        extras = sorted(k for k in pred if k not in have)
        if extras and self.include_computed_diagnostics:
            var_keys += extras
        elif extras:
            logger.info("CombinedMetric: skipping computed diagnostics %s (include_computed_diagnostics=False).", extras)
        return var_keys

    def _build_static_weights(self, var_keys) -> Dict[str, Dict[str, float]]:
        return {name: self.weightings[name].build(var_keys) for name in self.metric_names}

    # ---- climatology (anomaly.py:162-228) ---------------------------------------------------------------------------------------------
    def _fixed_clim(self, var_key: str, shape, device):
        """-> (tensor [n_levels, H, W] on `device`, level stride) of the fixed climatology, or None."""
        name = var_key if var_key in self._climatology else var_key.rsplit("/", 1)[-1]
        if name not in self._climatology:
            return None
        if (name, device) not in self._clim_on:
            self._clim_on[(name, device)] = self._climatology[name].to(device).contiguous()
        clim = self._clim_on[(name, device)]
        leading = clim.shape[:-2]
        if clim.ndim < 2 or len(leading) > 1:
            raise ValueError(f"CombinedMetric: climatology for '{var_key}' has shape {tuple(clim.shape)}; expected (lat, lon) "
                             "for a 2-D variable or (level, lat, lon) for a 3-D variable.")
        n_levels = leading[0] if leading else 1
        if n_levels not in (1, shape[1]):
            raise ValueError(f"CombinedMetric: climatology for '{var_key}' has {n_levels} levels but the field has {shape[1]}. "
                             "Check that the climatology's level axis matches the data config.")
        if tuple(clim.shape[-2:]) != tuple(shape[-2:]):
            raise ValueError(f"CombinedMetric: climatology for '{var_key}' is on a {tuple(clim.shape[-2:])} grid, the field on "
                             f"{tuple(shape[-2:])}")
        return clim, (shape[-2] * shape[-1] if n_levels > 1 else 0), 0

    def _update_climatology(self, target: dict) -> None:
        if not self.accumulate_climatology or self._climatology:
            return
        batch_size = 0
        for var_key, t in target.items():
            batch_size = t.shape[0]
            s = t.detach().float().sum(dim=0)
            if var_key in self._clim_sum:
                self._clim_sum[var_key] += s
            else:
                self._clim_sum[var_key] = s
        self._clim_count += batch_size

    def _clim_of(self, var_key, p, t):
        """-> (tensor that is kept alive, level stride, time stride): fixed, else the running mean, else this call's target mean."""
        fixed = self._fixed_clim(var_key, p.shape, p.device)
        if fixed is not None:
            return fixed
        thw, hw = p.shape[2] * p.shape[3] * p.shape[4], p.shape[3] * p.shape[4]
        if var_key in self._clim_sum and self._clim_count > 0:
            clim = (self._clim_sum[var_key] / self._clim_count).to(p.device)
            if tuple(clim.shape) != tuple(p.shape[1:]):
                raise ValueError(f"CombinedMetric: the accumulated climatology of '{var_key}' has shape {tuple(clim.shape)}, "
                                 f"the field {tuple(p.shape[1:])}")
            return clim.contiguous(), thw, hw
        logger.debug("CombinedMetric: no climatology for '%s'; using batch target mean.", var_key)
        return t.mean(dim=0).contiguous(), thw, hw

    # ---- the device call ------------------------------------------------------------------------------------------------------------
    def _handle(self, H, W, dev):
        def args():
            if self.lat_weights is not None and self.lat_weights.numel() != H:
                raise ValueError(f"CombinedMetric: {self.lat_weights.numel()} latitudes but the fields have {H} rows; "
                                 "latitude-sharded scoring (lat-band mode) is out of scope")
            return H, W, _f32(None if self.lat_weights is None else self.lat_weights.numpy()), dev
        return self._handles.get((H, W, dev), args)

    def submit(self, full_data_dict: dict) -> PendingScores:
        import torch
        if "y_processed" not in full_data_dict:
            raise KeyError("CombinedMetric requires full_data_dict['y_processed'] — add a 'reconstruct' postblock to postblocks.per_step.")
        if "y_target_processed" not in full_data_dict:
            raise KeyError("CombinedMetric requires full_data_dict['y_target_processed'] — add to postblocks.per_step: "
                           "reconstruct_target: {type: reconstruct, args: {in_key: 'y', out_key: 'y_target_processed'}} "
                           "followed by a bridgescaler_transformer postblock with key: 'y_target_processed'.")
        pred = flatten_named(full_data_dict["y_processed"], "y_processed", "CombinedMetric")
        target = flatten_named(full_data_dict["y_target_processed"], "y_target_processed", "CombinedMetric")
        if self.need_climatology:
            self._update_climatology(target)
        if self.var_keys is None:
            self.var_keys = self._resolve_var_keys(pred, target)
            self._combination_weights = self._build_static_weights(self.var_keys)
        var_keys = self.var_keys
        for var_key in var_keys:          # before anything is enqueued
            if var_key not in pred:
                raise KeyError(f"CombinedMetric: variable '{var_key}' missing from y_processed — "
                               "channel schema and postblocks output disagree.")
            if var_key not in target:
                raise KeyError(f"CombinedMetric: variable '{var_key}' missing from y_target_processed. If this is a "
                               "postblock-computed diagnostic, apply the same compute postblock to the target twin "
                               "(key: 'y_target_processed') or set include_computed_diagnostics: false.")
        ps, ts, cs = [], [], []
        with torch.no_grad():
            for var_key in var_keys:
                p, t = pred[var_key], target[var_key]
                if not isinstance(p, torch.Tensor) or not isinstance(t, torch.Tensor) or not p.is_cuda:
                    raise WXEngineError(f"{var_key} must be a [B, n_levels, n_time, H, W] tensor on the GPU")
                p = p.float()
                t = t.float().to(p.device)
                if p.dim() != 5 or tuple(p.shape) != tuple(t.shape):
                    raise WXEngineError(f"{var_key}: prediction {tuple(p.shape)} and target {tuple(t.shape)} must be one "
                                        "[B, n_levels, n_time, H, W] shape")
                if ps and (p.device != ps[0].device or p.shape[0] != ps[0].shape[0] or p.shape[3:] != ps[0].shape[3:]):
                    raise WXEngineError(f"{var_key}: {tuple(p.shape)} on {p.device}; all variables of one call share the device, the "
                                        f"batch size and H x W of {var_keys[0]}: {tuple(ps[0].shape)} on {ps[0].device}")
                p = p if p[0].is_contiguous() else p.contiguous()
                t = t if t[0].is_contiguous() else t.contiguous()
                ps.append(p)
                ts.append(t)
                if self.need_climatology:
                    cs.append(self._clim_of(var_key, p, t))
            B, _, _, H, W = ps[0].shape
            dev = ps[0].device.index
            h = self._handle(H, W, dev)
            n = len(var_keys)
            scores = torch.empty((n, len(METRIC_ORDER)), dtype=torch.float32, device=ps[0].device)
            with torch.cuda.device(dev):
                for v0 in range(0, n, MAX_VARIABLES):
                    sl = slice(v0, min(n, v0 + MAX_VARIABLES))
                    clim = ((ptr_array([c[0] for c in cs[sl]]), i64_array([c[1] for c in cs[sl]]), i64_array([c[2] for c in cs[sl]]))
                            if cs else (None, None, None))
                    _check(self.lib.wx_metrics_apply(h, sl.stop - sl.start, ptr_array(ps[sl]), i64_array([batch_stride(x, B) for x in ps[sl]]),
                                                     ptr_array(ts[sl]), i64_array([batch_stride(x, B) for x in ts[sl]]), *clim,
                                                     i32_array([x.shape[1] for x in ps[sl]]), i32_array([x.shape[2] for x in ps[sl]]),
                                                     B, self.eps, C.c_void_p(scores[v0].data_ptr()), _stream_ptr(dev)))
                pinned, event = copy_out(scores, dev)
        return PendingScores(self, pinned, event, list(var_keys))

    def _combine(self, scores: np.ndarray, var_keys) -> dict:
        """base.py:402-405 per metric: the per-variable floats, then the float32 mean of weight x score."""
        import torch
        out = {}
        table = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32))
        for name in self.metric_names:
            col = table[:, METRIC_ORDER.index(name)]
            weights = self._combination_weights[name]
            per_var = {k: col[i].item() for i, k in enumerate(var_keys)}
            aggregate = (col * torch.tensor([weights[k] for k in var_keys], dtype=torch.float64).to(torch.float32)).mean().item()
            self.last_var_scores[name] = per_var
            for k in var_keys:
                out[f"{name}/{k}"] = per_var[k]
            out[name] = aggregate
        return out

    def __call__(self, full_data_dict: dict) -> dict:
        return self.submit(full_data_dict).result()

    forward = __call__
