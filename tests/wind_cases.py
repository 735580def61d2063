"""Inputs of the wind-artifact-filter fixtures (tests/golden/wind_<case>.npz, tools/make_goldens.py --only wind), shared by the
generator, the CPU oracle tests and the GPU tests.

The fields are not stored: they are rebuilt here from the keyed Philox stream with +, -, *, / , sqrt and comparisons only (IEEE-exact,
so every machine gets the same bits); the fixture stores their SHA-256 and `case_inputs(..., check=fixture)` compares.

Every variable is unit-variance noise * 0.8 (four uniforms summed) plus a Gaussian jet in latitude around 0.35 of the latitude range
with a 2-dx zonal ripple on it: amplitude 3.2 in U (the only one that reaches the speed threshold), 1.0 in V, 2.0 in T -- a smooth
part next to the noise keeps the amplitude factor alpha of `preserve_amplitude` between 1 and 2, away from its clamp at 4, except on
the plane `stripe` names: a pure zonal 2-dx stripe 2.5 (-1)^j plus 1 % noise, whose unclamped alpha is ~57.  With B = 2 the second
batch item carries a weaker jet, so the two items have different masks and different alphas.  Points whose mask-level speed lies
within 1e-3 of the threshold are moved away from it (U and V times 1.002): fp32, fp64 and the device take the same decisions."""
import hashlib
import os

import numpy as np

SRC = "CESM"
KEYS = {v: f"{SRC}/prognostic/3d/{v}" for v in ("U", "V", "T")}
JET = {"U": 3.2, "V": 1.0, "T": 2.0}
CAM = dict(speed_threshold=2.8, smooth_sigma=1.2, smooth_sigma_zonal=2.0, smooth_sigma_meridional=0.5, dilation_zonal=15,
           dilation_meridional=5, falloff_sigma=4.0, preserve_amplitude=True)      # config/gen_2/camulator/camulator_gen2_casper.yml:237-259
DEFAULTS = dict(speed_threshold=3.0193274566643846, smooth_sigma=1.0, smooth_sigma_zonal=None, smooth_sigma_meridional=None,
                dilation_zonal=13, dilation_meridional=5, falloff_sigma=4.0, preserve_amplitude=False)     # wind_filter.py:175-190

# args: the constructor arguments; targets: target_vars in order; stripe: (variable, level) of the 2-dx stripe plane
WIND_CASES = {
    "cam48": dict(B=1, L=5, H=48, W=72, args=dict(CAM, mask_level=2, target_levels=[1, 2, 3, 7]), targets=("U", "V", "T"), stripe=("T", 3)),
    "dflt48": dict(B=1, L=5, H=48, W=72, args=dict(DEFAULTS, mask_level=1, target_levels=[0, 1, 3]), targets=("U", "V", "T")),
    "tiny": dict(B=1, L=4, H=7, W=19, args=dict(CAM, mask_level=2, target_levels=[0, 2, 3]), targets=("U", "V", "T")),
    "b2odd": dict(B=2, L=4, H=33, W=50, args=dict(DEFAULTS, preserve_amplitude=True, mask_level=1, target_levels=[0, 1, 3]), targets=("U", "V", "T")),
    "multi": dict(B=1, L=3, H=72, W=200, args=dict(CAM, mask_level=1, target_levels=[0, 2]), targets=("U", "V")),
    "small_k": dict(B=1, L=3, H=72, W=200, args=dict(DEFAULTS, dilation_zonal=1, dilation_meridional=1, falloff_sigma=0.5, smooth_sigma=0.4,
                                                    mask_level=1, target_levels=[0, 2]), targets=("U", "V")),
    "calm": dict(B=1, L=4, H=16, W=24, args=dict(DEFAULTS, speed_threshold=50.0, mask_level=1, target_levels=[0, 1, 3]), targets=("U", "V", "T")),
}
MARGIN = 1e-3


def _exp_neg(t):
    """exp(-t) for t >= 0 from +, * alone (a 14-term series of exp(-t / 256), squared eight times): the same bits everywhere."""
    x = -np.asarray(t, np.float64) / 256.0
    s = np.ones_like(x)
    for k in range(14, 0, -1):
        s = 1.0 + x * s / k
    for _ in range(8):
        s = s * s
    return s


def _noise(g, shape):
    """Unit variance from four uniforms: (sum - 2) * sqrt(3)."""
    return (g.random(shape) + g.random(shape) + g.random(shape) + g.random(shape) - 2.0) * 1.7320508075688772


def filtered_levels(name):
    """The levels of a case that are filtered (those of target_levels that exist), ascending."""
    c = WIND_CASES[name]
    return [l for l in sorted(c["args"]["target_levels"]) if l < c["L"]]


def case_inputs(name, check=None):
    """-> {"U" | "V" | "T": float32 [B, L, 1, H, W]}.  `check`: an opened fixture whose sha256 entries must match."""
    c = WIND_CASES[name]
    B, L, H, W = c["B"], c["L"], c["H"], c["W"]
    g = np.random.Generator(np.random.Philox(key=[2025, sorted(WIND_CASES).index(name)]))
    y = np.arange(H, dtype=np.float64)
    width = max(0.07 * H, 1.5)
    d = (y - 0.35 * (H - 1)) / width
    jet = _exp_neg(0.5 * d * d).reshape(1, 1, 1, H, 1)
    ripple = (1.0 + 0.15 * (1.0 - 2.0 * (np.arange(W) % 2))).reshape(1, 1, 1, 1, W)
    item = (1.0 - 0.2 * np.arange(B, dtype=np.float64)).reshape(B, 1, 1, 1, 1)      # a weaker jet in the second batch item
    out = {}
    for v in ("U", "V", "T"):
        out[v] = (0.8 * _noise(g, (B, L, 1, H, W)) + JET[v] * item * jet * ripple).astype(np.float32)
    if "stripe" in c:
        v, l = c["stripe"]
        stripe = 2.5 * (1.0 - 2.0 * (np.arange(W) % 2)).reshape(1, 1, 1, W)
        out[v][:, l] = (stripe + 0.025 * _noise(g, (B, 1, H, W))).astype(np.float32)
    ml, thr = c["args"]["mask_level"], c["args"]["speed_threshold"]
    u, w = out["U"][:, ml], out["V"][:, ml]
    near = np.abs(np.sqrt(u * u + w * w) - np.float32(thr)) < 2 * MARGIN
    out["U"][:, ml] = np.where(near, u * np.float32(1.002), u)
    out["V"][:, ml] = np.where(near, w * np.float32(1.002), w)
    for dt in (np.float32, np.float64):
        u, w = out["U"][:, ml].astype(dt), out["V"][:, ml].astype(dt)
        speed = np.sqrt(u * u + w * w)
        assert np.abs(speed - dt(thr)).min() >= MARGIN, f"{name}: a mask-level speed sits within {MARGIN} of the threshold"
    share = float((speed > thr).mean())
    if name == "calm":
        assert share == 0.0, name
    else:
        assert 0.02 <= share <= 0.30, f"{name}: {100 * share:.1f} % of the mask level is flagged, outside 2 .. 30 %"
    if check is not None:
        for k in ("U", "V", "T"):
            assert input_digest(out[k]) == str(check[f"sha256:{k}"]), f"{name}: regenerated input {k} differs from the fixture's"
    return out


def input_digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def output_names(name):
    """The compared outputs of a case, in fixture order: the blend mask [B, 1, H, W], then per target variable its filtered planes
    [B, n_filtered, H, W]."""
    return ["mask"] + list(WIND_CASES[name]["targets"])


def load_golden(name, gold_dir):
    """-> (fixture, {out: fp32 golden}, {out: fp64 golden}, {out: d_ref}); the fp64 golden is stored as its float32 difference from the
    fp32 golden (wind_<case>_f64.npz), the layout of the diag fixtures."""
    g = np.load(os.path.join(gold_dir, f"wind_{name}.npz"))
    g64 = np.load(os.path.join(gold_dir, f"wind_{name}_f64.npz"))
    f32 = {v: g[f"f32:{v}"] for v in output_names(name)}
    f64 = {v: f32[v].astype(np.float64) + g64[f"d64:{v}"].astype(np.float64) for v in output_names(name)}
    d_ref = {v: float(g[f"d_ref:{v}"]) for v in output_names(name)}
    return g, f32, f64, d_ref


def filtered_planes(name, var, t):
    """[B, L, 1, H, W] (numpy or torch) -> the filtered planes [B, n_filtered, H, W] in fixture order."""
    return t[:, filtered_levels(name), 0]
