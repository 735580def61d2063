"""Plain-torch restatement of the reference's ensemble verification, written from the formulas; only what the float32 result
depends on (which values are sorted, weighted and summed, and along which axis) follows the reference:
  credit/losses/gen_1/kcrps.py:64-81              KCRPSLoss (biased and fair): crps_by_sort, written from the formula
  credit/losses/gen_1/almost_fair_crps.py:48-76   AlmostFairKCRPSLoss: crps_by_pairs, written from the formula
  credit/metrics/gen_1/metrics.py:304-313         LatWeightedMetricsEnsemble: ens_std (with its (M + 1) / (M - 1) factor), ens_mean, ens_rmse
  credit/applications/rollout_metrics_noisy_model.py:107-135  calculate_ensemble_metrics;  :56, :69-71  compute_spread_skill_metric
  credit/ensemble/crps.py                         calculate_crps_per_channel = the plane mean of the biased CRPS (properscoring's
                                                  crps_ensemble is the same estimator, skill / M - pair / M^2)
Dtype-parametric: float32 restates the reference's forward, float64 is the yardstick the device result is held to.  With latitude
weights w (H values) every mean over the grid carries w[h] and is not divided by the sum of w; the reference applies none, so that
part is this project's definition.  Runs on whatever device the tensors are on (tools/ens_time.py times it on the GPU)."""
import numpy as np
import torch

MAPS = ("ens_mean", "ens_std", "ens_abs_err", "crps", "fair_crps", "afcrps")
SCALARS = ("crps", "fair_crps", "afcrps", "ens_rmse", "ens_spread", "spread_skill", "ens_abs_err", "ens_std")
PER_LEVEL = ("ens_rmse", "ens_spread")


def lat_weights(latitude):
    """credit/losses/base.py::_cos_lat_weights: float32 cos(deg2rad(lat)) / mean."""
    lat = torch.tensor(np.asarray(latitude, dtype=np.float64), dtype=torch.float32)
    w = torch.cos(torch.deg2rad(lat))
    return w / w.mean()


def crps_by_sort(values, truth, fair):
    """The kernel CRPS of kcrps.py:64-81 from its formula: mean |x_i - y| minus sum_i (2 i - M - 1) x_(i) over the ascending members,
    the sum divided by M (M - 1) when `fair` and by M^2 otherwise.  values [..., M] (members last), truth [...].  The members themselves
    are sorted and weighted, not their differences from the truth: that is the float32 order of the reference."""
    n = values.shape[-1]
    mean_abs_error = (values - truth.unsqueeze(-1)).abs().mean(dim=-1)
    ascending = values.sort(dim=-1).values
    rank = torch.arange(1, n + 1, dtype=values.dtype, device=values.device)
    weight = (2 * rank - n - 1) / (n * (n - 1) if fair else n * n)
    return mean_abs_error - (weight * ascending).sum(dim=-1)


def crps_by_pairs(values, truth, alpha):
    """The almost fair CRPS of almost_fair_crps.py:48-76 from its formula: mean |x_i - y| - (1 - (1 - alpha) / M) sum_{i != j} |x_i - x_j|
    / (2 M (M - 1)), the double sum taken over the full [.., M, M] table of gaps (its diagonal is zero as it stands)."""
    n = values.shape[-1]
    mean_abs_error = (values - truth.unsqueeze(-1)).abs().mean(dim=-1)
    gaps = (values.unsqueeze(-1) - values.unsqueeze(-2)).abs()
    half_mean_gap = gaps.sum(dim=(-1, -2)) * (1.0 / (2 * n * (n - 1)))
    return mean_abs_error - (1.0 - (1.0 - alpha) / n) * half_mean_gap


def ensemble_maps(x, y):
    """metrics.py:304-313 on x [M, B, L, T, H, W], y [B, L, T, H, W]: ens_std WITH the (M + 1) / (M - 1) factor, ens_mean, ens_rmse."""
    m = x.shape[0]
    ens_std = torch.std(x, dim=0) * (m + 1) / (m - 1)
    ens_mean = x.mean(dim=0)
    return ens_std, ens_mean, torch.sqrt((ens_mean - y) ** 2)


def plane_rmse_and_spread(x, y, w=1.0):
    """rollout_metrics_noisy_model.py:107-135 from its equations C3 and C4, per plane [B, L, T]: the root of the grid mean of the squared
    error of the ensemble mean, and the root of the mean over members and grid of the squared departures from the ensemble mean.  The
    caller averages over batch and time.  x [M, B, L, T, H, W], y [B, L, T, H, W]; w: a tensor broadcastable over [.., H, W], or 1.0."""
    centre = x.mean(dim=0)
    rmse = ((centre - y).square() * w).mean(dim=(-2, -1)).sqrt()
    spread = ((x - centre).square() * w).mean(dim=(0, -2, -1)).sqrt()
    return rmse, spread


def variable(x, y, alpha, w=None, dtype=torch.float64, want_maps=True):
    """One variable: x [M, B, L, T, H, W] members, y [B, L, T, H, W] truth, w: None or [H] weights.
    -> (scalars {name: float or array over levels}, maps {name: tensor [B, L, T, H, W]}); maps["ens_std"] carries the reference's
    (M + 1) / (M - 1) factor, the scalar "ens_std" is the mean of the plain sample standard deviation."""
    x, y = x.to(dtype), y.to(dtype)
    M = x.shape[0]
    wt = 1.0 if w is None else w.to(dtype).to(x.device).reshape(1, 1, 1, -1, 1)
    last = torch.movedim(x, 0, -1)          # [B, L, T, H, W, M]
    maps = {"crps": crps_by_sort(last, y, False), "fair_crps": crps_by_sort(last, y, True), "afcrps": crps_by_pairs(last, y, alpha)}
    maps["ens_std"], maps["ens_mean"], maps["ens_abs_err"] = ensemble_maps(x, y)
    rmse, spread = plane_rmse_and_spread(x, y, wt)
    s = {name: (maps[name] * wt).mean().item() for name in ("crps", "fair_crps", "afcrps", "ens_abs_err")}
    s["ens_std"] = (torch.std(x, dim=0) * wt).mean().item()
    s["ens_rmse"], s["ens_spread"] = rmse.mean().item(), spread.mean().item()
    s["ens_rmse_levels"] = rmse.mean(dim=[0, 2]).cpu().numpy().astype(np.float64)
    s["ens_spread_levels"] = spread.mean(dim=[0, 2]).cpu().numpy().astype(np.float64)
    s["spread_skill"] = (M + 1) / (M - 1) * s["ens_spread"] / s["ens_rmse"] if s["ens_rmse"] > 0 else float("nan")
    s["crps_per_channel"] = (maps["crps"] * wt).mean(dim=[0, 2, 3, 4]).cpu().numpy().astype(np.float64)
    return s, (maps if want_maps else {})


def result_dict(per_var):
    """{var_key: scalars of `variable`} in variable order -> the result dict in the order of EnsembleVerification."""
    out = {}
    for name in SCALARS:
        for k, s in per_var.items():
            out[f"{name}/{k}"] = float(s[name])
            if name in PER_LEVEL:
                for lev, v in enumerate(s[name + "_levels"]):
                    out[f"{name}/{k}/{lev}"] = float(v)
    for k, s in per_var.items():
        out[f"crps_per_channel/{k}"] = np.asarray(s["crps_per_channel"], dtype=np.float64)
    return out


def restate(members, truth, alpha, w=None, dtype=torch.float64, want_maps=True):
    """members {var_key: [M, B, L, T, H, W]}, truth {var_key: [B, L, T, H, W]} (tensors) -> (result dict, {map: {var_key: tensor}})."""
    per_var, maps = {}, {m: {} for m in MAPS}
    for k in sorted(truth):
        s, mp = variable(members[k], truth[k], alpha, w, dtype, want_maps)
        per_var[k] = s
        for m, v in mp.items():
            maps[m][k] = v
    return result_dict(per_var), maps


def pair_sums(x):
    """x [..., M] -> (sum_{i<j} |x_i - x_j| by the pairwise tensor, the same by the sorted sum): the identity the kernel rests on."""
    m = x.shape[-1]
    direct = 0.5 * torch.abs(x.unsqueeze(-2) - x.unsqueeze(-1)).sum(dim=(-1, -2))
    s, _ = torch.sort(x)
    i = torch.arange(1, m + 1, dtype=x.dtype)
    return direct, ((2 * i - m - 1) * s).sum(-1)
