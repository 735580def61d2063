"""Cases and inputs of the verification-metrics fixtures (tests/golden/metrics_<case>.npz, tools/make_goldens.py --only metrics),
shared by the generator, the CPU oracle tests, the reference tests and the GPU tests.

The fields are not stored: they are rebuilt here from the keyed Philox stream with +, -, * and casts only (IEEE-exact, so every
machine gets the same bits); the fixture stores their SHA-256 and `case_inputs(..., check=fixture)` compares.  INPUTS describes the
tensors of a case, METRICS_CASES the configurations scored on them (several may share one set of inputs).

Grids: 33 x 67 (odd W: scalar loads; 8-row tiles, five row blocks per plane with a one-row last one), 7 x 19 (one partial tile per
plane), 3 x 1445 (a row longer than any workgroup's stride, W no multiple of 4).  Every field is climatology + anomaly + error:
  sp    1e5 +- 800 Pa, the prediction 60 Pa off: the field on which float32 raw moments lose R2, the log variance ratio and the ACC
  t2m   280 +- 15 K;  q: positive, 1e-3 scale, multiplicative anomalies;  T, U: level-dependent;  unit: +-1 noise
Distance per score: |a - b| / scale with scale = the fp64 rmse of the variable for rmse, mae and bias, the fp64 mse for mse, the
fp64 activity for activity and 1 for r2score, log_variance_ratio and acc.  An aggregate is the mean of weight x score, so its scale
is the same mean of |weight| x scale.  Two equal values are at distance 0 whatever the scale (prediction == target has rmse 0)."""
import hashlib
import os

import numpy as np

from hybrid_cases import gate  # noqa: F401  (the project's gate, re-exported for the tests)

SRC = "ERA5"
ALL8 = ("rmse", "mse", "mae", "bias", "r2score", "log_variance_ratio", "acc", "activity")
DIMENSIONLESS = ("r2score", "log_variance_ratio", "acc")
NAMES = {"sp": "prognostic/2d/surface_pressure", "t2m": "prognostic/2d/t2m", "q2": "prognostic/2d/q2", "T": "prognostic/3d/temperature",
         "U": "prognostic/3d/u_wind", "deep": "prognostic/3d/deep", "same": "diagnostic/2d/same", "const": "diagnostic/2d/const"}
NAMES.update({f"v{i:02d}": f"prognostic/2d/v{i:02d}" for i in range(33)})
KEYS = {k: f"{SRC}/{v}" for k, v in NAMES.items()}

# vars: {name: (kind, levels)}; clim: {name: "2d" | "3d"} -- the fixed climatology fields a configuration may hand over
INPUTS = {
    "sp2d": dict(grid=(33, 67), B=1, T=1, calls=1, vars={"sp": ("sp", 1), "t2m": ("t2m", 1), "q2": ("q", 1)},
                 clim={"sp": "2d", "t2m": "2d", "q2": "2d"}),
    "lev16": dict(grid=(33, 67), B=1, T=1, calls=1, vars={"T": ("T", 16), "U": ("U", 16), "sp": ("sp", 1)}, clim={"T": "3d", "U": "2d"}),
    "b2t2": dict(grid=(33, 67), B=2, T=2, calls=1, vars={"T": ("T", 5), "t2m": ("t2m", 1)}, clim={"T": "3d", "t2m": "2d"}),
    "many": dict(grid=(7, 19), B=1, T=1, calls=1, vars=dict({f"v{i:02d}": ("unit", 1) for i in range(33)}, deep=("T", 137)), clim={}),
    "wide": dict(grid=(3, 1445), B=1, T=1, calls=1, vars={"sp": ("sp", 1), "U": ("U", 2)}, clim={"sp": "2d", "U": "3d"}),
    "online": dict(grid=(33, 67), B=2, T=1, calls=3, vars={"T": ("T", 3), "sp": ("sp", 1)}, clim={}),
    "degenerate": dict(grid=(7, 19), B=1, T=1, calls=1, vars={"same": ("t2m", 1), "const": ("t2m", 1)}, clim={"same": "2d", "const": "2d"}),
}
_MANY_VARIANCES = {KEYS[f"v{i:02d}"]: 0.25 + 0.125 * i for i in range(33) if i != 7}      # v07 has none: the warning and weight 1
_MANY_VARIANCES[KEYS["deep"]] = 400.0
_MANY_WEIGHTS = {KEYS["v03"]: 2.0, KEYS["deep"]: 0.5}
_NO_CLIM6 = {m: {} for m in ALL8[:5]}
_NO_CLIM6["log_variance_ratio"] = {"eps": 1e-6}

# metrics: {metric: per-metric args}; the string "CLIM" stands for the case's climatology dict; lat: latitude weights on
METRICS_CASES = {
    "sp2d": dict(inputs="sp2d", lat=True, metrics={m: ({"climatology": "CLIM"} if m in ("acc", "activity") else {}) for m in ALL8},
                 kwargs=dict(var_weighting="none")),
    "lev16": dict(inputs="lev16", lat=True, metrics={m: ({"climatology": "CLIM"} if m in ("acc", "activity") else {}) for m in ALL8},
                  kwargs=dict(var_weighting="none")),
    "lev16_basic": dict(inputs="lev16", lat=True, metrics={"rmse": {}, "mae": {}, "bias": {}},
                        kwargs=dict(var_weighting="inverse_variance", variances={KEYS["T"]: 225.0, KEYS["U"]: 100.0, KEYS["sp"]: 640000.0})),
    "b2t2": dict(inputs="b2t2", lat=False, metrics={m: ({"climatology": "CLIM"} if m in ("acc", "activity") else {}) for m in ALL8},
                 kwargs=dict(var_weighting="manual", variable_weights={KEYS["T"]: 3.0})),
    "many": dict(inputs="many", lat=False, metrics=_NO_CLIM6,
                 kwargs=dict(var_weighting="inverse_variance", variances=_MANY_VARIANCES, variable_weights=_MANY_WEIGHTS)),
    "many_raw": dict(inputs="many", lat=False, metrics=_NO_CLIM6,
                     kwargs=dict(var_weighting="inverse_variance", variances=_MANY_VARIANCES, variable_weights=_MANY_WEIGHTS,
                                 normalize_weights=False)),
    "wide": dict(inputs="wide", lat=True, metrics={m: ({"climatology": "CLIM"} if m in ("acc", "activity") else {}) for m in ALL8},
                 kwargs=dict(var_weighting="none")),
    "online": dict(inputs="online", lat=True, metrics={"rmse": {}, "acc": {}, "activity": {}}, kwargs=dict(var_weighting="none")),
    "online_noacc": dict(inputs="online", lat=True, kwargs=dict(var_weighting="none"),
                         metrics={"acc": {"accumulate_climatology": False}, "activity": {"accumulate_climatology": False}}),
    "degenerate": dict(inputs="degenerate", lat=True, kwargs=dict(var_weighting="none"),
                       metrics={m: ({"climatology": "CLIM"} if m in ("acc", "activity") else {}) for m in ALL8}),
}


def latitude(H):
    """Degrees, -80 .. 80: cos > 0 everywhere."""
    return -80.0 + 160.0 * np.arange(H, dtype=np.float64) / (H - 1)


def _field(kind, g, shape_c, shape):
    """-> (climatology, target, prediction) float64; the climatology has the shape (L, 1, H, W) and broadcasts over batch and time."""
    u = lambda s: 2.0 * g.random(s) - 1.0      # noqa: E731
    L = shape_c[0]
    lev = np.arange(L, dtype=np.float64).reshape(L, 1, 1, 1)
    if kind == "sp":
        c = 100000.0 + 500.0 * u(shape_c)
        t = c + 300.0 * u(shape)
        p = t + 60.0 + 100.0 * u(shape)
    elif kind == "t2m":
        c = 280.0 + 10.0 * u(shape_c)
        t = c + 5.0 * u(shape)
        p = t + 0.3 + 1.5 * u(shape)
    elif kind == "q":
        c = 0.001 * (0.5 + g.random(shape_c))
        t = c * (0.8 + 0.4 * g.random(shape))
        p = t * (0.9 + 0.2 * g.random(shape))
    elif kind == "T":
        c = 215.0 + 0.5 * lev + 8.0 * u(shape_c)
        t = c + 4.0 * u(shape)
        p = t - 0.4 + 1.2 * u(shape)
    elif kind == "U":
        c = 3.0 * lev - 20.0 + 6.0 * u(shape_c)
        t = c + 9.0 * u(shape)
        p = 0.8 * t + 0.2 * c + 2.5 * u(shape)
    else:
        c = 0.25 * u(shape_c)
        t = c + u(shape)
        p = t + 0.05 + 0.3 * u(shape)
    return c, t, p


def case_inputs(inputs_name, check=None):
    """-> dict(pred=[per call {name: float32 [B, L, T, H, W]}], target=[...], clim={name: float32 (H, W) or (L, H, W)},
    lat=float64 [H]).  `check`: an opened fixture whose sha256 entries must match."""
    spec = INPUTS[inputs_name]
    H, W = spec["grid"]
    B, T = spec["B"], spec["T"]
    g = np.random.Generator(np.random.Philox(key=[2029, sorted(INPUTS).index(inputs_name)]))
    out = dict(pred=[{} for _ in range(spec["calls"])], target=[{} for _ in range(spec["calls"])], clim={}, lat=latitude(H))
    for name, (kind, L) in spec["vars"].items():
        for call in range(spec["calls"]):
            c, t, p = _field(kind, g, (L, 1, H, W), (B, L, T, H, W))
            if inputs_name == "degenerate":
                if name == "same":
                    p = t
                else:                       # a constant target, the prediction's error kept
                    p = 7.5 + (p - t)
                    t = np.full_like(t, 7.5)
            out["pred"][call][name] = p.astype(np.float32)
            out["target"][call][name] = t.astype(np.float32)
            if call == 0 and name in spec["clim"]:
                c = c.astype(np.float32).reshape(L, H, W)
                out["clim"][name] = np.ascontiguousarray(c[0] if spec["clim"][name] == "2d" else c)
    if check is not None:
        for what, arr in flat_inputs(out).items():
            assert input_digest(arr) == str(check[f"sha256:{what}"]), f"{inputs_name}: regenerated input {what} differs from the fixture's"
    return out


def flat_inputs(inp):
    flat = {f"clim:{k}": v for k, v in inp["clim"].items()}
    for call, (p, t) in enumerate(zip(inp["pred"], inp["target"])):
        flat.update({f"pred:{call}:{k}": v for k, v in p.items()})
        flat.update({f"target:{call}:{k}": v for k, v in t.items()})
    return flat


def input_digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def climatology_dict(inputs_name, inp):
    """The case's climatology as a configuration hands it over: the first field under its full var_key, the others under their short
    names (both look-ups of _get_clim)."""
    out = {}
    for i, (name, arr) in enumerate(inp["clim"].items()):
        out[KEYS[name] if i == 0 else KEYS[name].rsplit("/", 1)[-1]] = arr
    return out


def metric_args(case, inp, convert=lambda a: a):
    """{metric: per-metric args} of a case with its climatology put in (`convert` makes of an array what the receiver wants)."""
    c = METRICS_CASES[case]
    clim = {k: convert(v) for k, v in climatology_dict(c["inputs"], inp).items()}
    return {m: {k: (clim if isinstance(v, str) and v == "CLIM" else v) for k, v in args.items()} for m, args in c["metrics"].items()}


def block_args(case, inp, convert=lambda a: a):
    """The keyword arguments of wxengine.metrics.CombinedMetric (and of the restatement) for a case."""
    c = METRICS_CASES[case]
    kw = dict(metrics=metric_args(case, inp, convert), **c["kwargs"])
    if c["lat"]:
        kw.update(use_latitude_weights=True, latitude=inp["lat"])
    return kw


def reference_args(case, inp):
    """-> (keyword arguments of the reference's BaseCombinedMetric, the variances its scaler file would hold or None).  The caller
    serves the variances through `_load_target_variances` and the latitude weights through `_cos_lat_weights`."""
    import torch
    c = METRICS_CASES[case]
    kw = dict(c["kwargs"])
    variances = kw.pop("variances", None)
    kw["metrics"] = metric_args(case, inp, torch.from_numpy)
    if variances is not None:
        kw["scaler_path"] = "scaler.json"
    if c["lat"]:
        kw.update(use_latitude_weights=True, latitude_weights="grid.nc")
    return kw, variances


def state_dicts(inp, call, convert):
    """-> full_data_dict of one call; `convert` makes of a float32 array the tensor the receiver wants."""
    return {"y_processed": {SRC: {KEYS[k]: convert(v) for k, v in inp["pred"][call].items()}},
            "y_target_processed": {SRC: {KEYS[k]: convert(v) for k, v in inp["target"][call].items()}}}


def distance(a, b, scale):
    a, b = float(a), float(b)
    if a == b:
        return 0.0
    return abs(a - b) / scale if scale > 0 else float("inf")


def scales(all64, weights, var_keys):
    """{key of the output dict: scale} from the fp64 scores of one call, {var_key: {metric: score}} with rmse and mse always present,
    and the combination weights {metric: {var_key: weight}}."""
    res = {}
    for metric, w in weights.items():
        per_var = {}
        for k in var_keys:
            if metric in DIMENSIONLESS:
                per_var[k] = 1.0
            elif metric == "mse":
                per_var[k] = all64[k]["mse"]
            elif metric == "activity":
                per_var[k] = all64[k]["activity"]
            else:
                per_var[k] = all64[k]["rmse"]
            res[f"{metric}/{k}"] = per_var[k]
        res[metric] = 1.0 if metric in DIMENSIONLESS else float(np.mean([abs(w[k]) * per_var[k] for k in var_keys]))
    return res


def raw_moments(p, t, c, w_full, pairwise):
    """r2score, log_variance_ratio and acc of ONE variable the careless way: one pass of float32 raw moments (sum w, w p, w t, w c,
    w p p, w t t, w c c, w p t, w p c, w t c), the centred moments formed from them afterwards in float32.  p, t, c, w_full: float32
    arrays of one shape.  Summation is sequential (a running float32 sum) or pairwise (numpy's float32 sum).  What the sp2d case must
    tell from a correct kernel."""
    f = np.float32
    n = f(p.size)

    def total(x):
        x = np.ascontiguousarray(x, dtype=f).reshape(-1)
        return f(np.sum(x, dtype=f)) if pairwise else f(np.cumsum(x, dtype=f)[-1])
    m = {k: total(v) / n for k, v in dict(w=w_full, p=w_full * p, t=w_full * t, c=w_full * c, pp=w_full * p * p, tt=w_full * t * t,
                                          cc=w_full * c * c, pt=w_full * p * t, pc=w_full * p * c, tc=w_full * t * c).items()}
    d = p - t
    mse = total(w_full * d * d) / n
    var_p = m["pp"] - f(2) * m["p"] * m["p"] + m["p"] * m["p"] * m["w"]
    var_t = m["tt"] - f(2) * m["t"] * m["t"] + m["t"] * m["t"] * m["w"]
    r2 = f(1) - mse / (var_t + f(1e-12))
    lvr = np.log10(var_p + f(1e-12)) - np.log10(var_t + f(1e-12))
    mf, mt = m["p"] - m["c"], m["t"] - m["c"]
    # mean(w (p - c - mf)(t - c - mt)) expanded in raw moments
    ff = m["pp"] - f(2) * m["pc"] + m["cc"] - f(2) * mf * mf + mf * mf * m["w"]
    tt = m["tt"] - f(2) * m["tc"] + m["cc"] - f(2) * mt * mt + mt * mt * m["w"]
    ft = m["pt"] - m["pc"] - m["tc"] + m["cc"] - f(2) * mf * mt + mf * mt * m["w"]
    acc = ft / (np.sqrt(np.maximum(ff, f(0)) + f(1e-12)) * np.sqrt(np.maximum(tt, f(0)) + f(1e-12)))
    return {"r2score": float(r2), "log_variance_ratio": float(lvr), "acc": float(acc)}


def load_golden(case, gold_dir):
    """-> (fixture, keys, f32 [calls, n], f64 [calls, n], d_ref [calls, n], scale [calls, n])."""
    g = np.load(os.path.join(gold_dir, f"metrics_{case}.npz"))
    return g, [str(k) for k in g["keys"]], g["f32"], g["f64"], g["d_ref"], g["scale"]
