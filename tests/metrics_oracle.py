"""Plain-torch restatement of the gen-2 verification metrics (credit/metrics/base.py, common.py, anomaly.py): the eight per-variable
scores in the reference's operation order, the static combination weights, the online climatology and the returned dict.  Dtype-
parametric: float32 restates the reference's forward (which casts to float32), float64 is the yardstick the device result is held
to.  Runs on whatever device the tensors are on (tools/metrics_time.py times it on the GPU beside the device call)."""
import numpy as np
import torch

ORDER = ("rmse", "mse", "mae", "bias", "r2score", "log_variance_ratio", "acc", "activity")
SCALE_POWER = {"rmse": 1, "mse": 2, "mae": 1, "bias": 1, "r2score": 0, "log_variance_ratio": 0, "acc": 0, "activity": 1}
_EPS = 1e-12


def lat_weights(latitude):
    """_cos_lat_weights: float32 cos(deg2rad(lat)) / mean."""
    lat = torch.tensor(np.asarray(latitude, dtype=np.float64), dtype=torch.float32)
    w = torch.cos(torch.deg2rad(lat))
    return w / w.mean()


def scores(p, t, c, w, eps=1e-12, which=ORDER):
    """The scores `which` of one variable [B, L, T, H, W]; c: the climatology expanded to p's shape, or None (acc and activity are
    then absent); w: (1, 1, 1, H, 1) tensor or 1.0.  Every line is the reference's expression."""
    out = {}
    d = p - t
    if "mse" in which or "rmse" in which:
        mse = (d ** 2 * w).mean() if torch.is_tensor(w) else (d ** 2).mean()
        out["mse"] = mse
        out["rmse"] = torch.sqrt(mse)
    if "mae" in which:
        out["mae"] = (torch.abs(d) * w).mean() if torch.is_tensor(w) else torch.abs(d).mean()
    if "bias" in which:
        out["bias"] = (d * w).mean() if torch.is_tensor(w) else d.mean()
    if "r2score" in which or "log_variance_ratio" in which:
        target_mean = (w * t).mean()
        var_target = (w * (t - target_mean) ** 2).mean()
        if "r2score" in which:
            out["r2score"] = 1.0 - (w * d ** 2).mean() / (var_target + 1e-12)
        if "log_variance_ratio" in which:
            pred_mean = (w * p).mean()
            var_pred = (w * (p - pred_mean) ** 2).mean()
            out["log_variance_ratio"] = torch.log10(var_pred + eps) - torch.log10(var_target + eps)
    if c is not None and ("acc" in which or "activity" in which):
        d_f = (p - c) - (w * (p - c)).mean()
        d_t = (t - c) - (w * (t - c)).mean()
        sdaf = torch.sqrt((w * d_f ** 2).mean() + _EPS)
        out["activity"] = sdaf
        if "acc" in which:
            sdav = torch.sqrt((w * d_t ** 2).mean() + _EPS)
            out["acc"] = (w * d_f * d_t).mean() / (sdaf * sdav)
    return {k: out[k] for k in ORDER if k in out and k in which}


def static_weights(metric, var_keys, var_weighting, variances, variable_weights, normalize_weights):
    """_build_static_weights for one metric (warnings left out)."""
    manual_weights = {k: float(v) for k, v in (variable_weights or {}).items()}
    power = SCALE_POWER[metric]
    weights = {}
    for k in var_keys:
        manual = manual_weights.get(k, 1.0)
        variance = (variances or {}).get(k) if var_weighting == "inverse_variance" and power != 0 else None
        weights[k] = manual if variance is None else manual / max(variance, 1e-12) ** (power / 2)
    if normalize_weights:
        mean_w = sum(weights.values()) / len(weights)
        if mean_w > 0:
            weights = {k: v / mean_w for k, v in weights.items()}
    return weights


class Restatement:
    """BaseCombinedMetric restated, with the arrays of wxengine.metrics.CombinedMetric in the place of the reference's files."""

    def __init__(self, metrics, var_weighting="inverse_variance", variances=None, variable_weights=None, normalize_weights=True,
                 include_computed_diagnostics=True, use_latitude_weights=False, latitude=None, data_var_keys=None, dtype=torch.float32):
        self.metrics = {m: dict(a or {}) for m, a in metrics.items()}
        self.shared = dict(var_weighting=var_weighting, variances=variances, variable_weights=variable_weights,
                           normalize_weights=normalize_weights)
        self.include_computed_diagnostics = include_computed_diagnostics
        self.w = lat_weights(latitude).view(1, 1, 1, -1, 1) if use_latitude_weights else None
        self.data_var_keys = data_var_keys
        self.dtype = dtype
        self.var_keys = None
        self.weights = None
        anomaly = [m for m in self.metrics if m in ("acc", "activity")]
        clim = self.metrics[anomaly[0]].get("climatology") if anomaly else None
        self.accumulate = bool(self.metrics[anomaly[0]].get("accumulate_climatology", True)) if anomaly else True
        self.anomaly = bool(anomaly)
        self.climatology = {k: torch.as_tensor(v).float() for k, v in (clim or {}).items()}
        self.clim_sum, self.clim_count = {}, 0
        self.eps = float(self.metrics.get("log_variance_ratio", {}).get("eps", 1e-12))
        self.last_all_scores = {}

    def _clim(self, key, p, t):
        name = key if key in self.climatology else key.rsplit("/", 1)[-1]
        if name in self.climatology:
            clim = self.climatology[name].to(device=p.device, dtype=p.dtype)
            n_levels = clim.shape[0] if clim.ndim == 3 else 1
            clim = clim.reshape(1, n_levels, 1, *clim.shape[-2:])
        elif key in self.clim_sum and self.clim_count > 0:
            clim = (self.clim_sum[key] / self.clim_count).to(device=p.device, dtype=p.dtype)
        else:
            clim = t.mean(dim=0, keepdim=True)
        return clim.expand_as(p)

    def __call__(self, full, all_scores=False):
        """-> the reference's dict.  all_scores: every one of the eight scores is also kept in `last_all_scores` {var_key: {metric:
        float}} (acc and activity only with an anomaly metric configured), for the scales of the distance."""
        pred = {k: v for s in full["y_processed"].values() for k, v in s.items()}
        target = {k: v for s in full["y_target_processed"].values() for k, v in s.items()}
        if self.anomaly and self.accumulate and not self.climatology:
            for k, t in target.items():      # the running sum stays float32, as the reference's `.float()` makes it
                s = t.detach().float().sum(dim=0)
                self.clim_sum[k] = self.clim_sum[k] + s if k in self.clim_sum else s
                n = t.shape[0]
            self.clim_count += n
        if self.var_keys is None:
            keys = list(self.data_var_keys) if self.data_var_keys is not None else sorted(target)
            extras = sorted(k for k in pred if k not in set(keys))
            self.var_keys = keys + (extras if self.include_computed_diagnostics else [])
            self.weights = {}
            for m, a in self.metrics.items():
                kw = dict(self.shared)
                kw.update({k: a[k] for k in kw if k in a})
                self.weights[m] = static_weights(m, self.var_keys, **kw)
        which = ORDER if all_scores else tuple(self.metrics)
        per_var = {}
        for k in self.var_keys:
            p = pred[k].to(self.dtype)
            t = target[k].to(self.dtype).to(p.device)
            w = self.w.to(device=p.device) if self.w is not None else 1.0
            per_var[k] = scores(p, t, self._clim(k, p, t) if self.anomaly else None, w, self.eps, which)
        self.last_all_scores = {k: {m: v.item() for m, v in s.items()} for k, s in per_var.items()}
        out = {}
        for m in self.metrics:
            for k in self.var_keys:
                out[f"{m}/{k}"] = per_var[k][m].item()
            out[m] = torch.stack([self.weights[m][k] * per_var[k][m] for k in self.var_keys]).mean().item()
        return out
