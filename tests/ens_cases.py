"""Cases and inputs of the ensemble-verification fixtures (tests/golden/ens_<case>.npz, tools/make_goldens.py --only ensemble), shared
by the generator, the CPU oracle tests, the reference tests and the GPU tests.

The fields are not stored: they are rebuilt here from the keyed Philox stream with +, -, * and casts only (IEEE-exact, so every
machine gets the same bits); the fixture stores their SHA-256 and `case_inputs(..., check=fixture)` compares.  A variable is a truth
[B, L, T, H, W] and M members [M, B, L, T, H, W]: member = truth + bias + spread x noise, float32.
  sp    1e5 +- 800 Pa, the members 60 Pa off and 150 Pa apart: the field on which sorting and summing the members themselves in
        float32 loses digits
  t2m   280 +- 15 K;  q: positive, 1e-3 scale, multiplicative;  T, U: level-dependent;  unit: +-1 noise
Outside `ties` no member equals another member or the truth at any point (asserted on the float32 values; the rare coincidences
of the draw are moved apart by a fixed rule first), so a sort that mishandles ties cannot hide behind the other cases.  `ties` has
three variables: every member equal (pair = 0, ens_std = 0, crps = |x - y|), two members equal, a member equal to the truth.

Distance: |a - b| / scale; for a map the maximum over the map.  scale is the fp64 mean of the quantity over the variable (for a
scalar score its own fp64 magnitude), except for the ens_mean map, where it is the fp64 mean |ensemble mean - truth|.  Two equal
values are at distance 0 whatever the scale (ens_std of equal members is 0)."""
import hashlib
import os

import numpy as np

from hybrid_cases import gate  # noqa: F401  (the project's gate, re-exported for the tests)

SRC = "ERA5"
NAMES = {"sp": "prognostic/2d/surface_pressure", "t2m": "prognostic/2d/t2m", "q2": "prognostic/2d/q2", "T": "prognostic/3d/temperature",
         "U": "prognostic/3d/u_wind", "unit": "diagnostic/2d/unit", "equal": "diagnostic/2d/equal", "two": "diagnostic/2d/two",
         "hit": "diagnostic/2d/hit"}
NAMES.update({f"v{i:02d}": f"prognostic/2d/v{i:02d}" for i in range(34)})
KEYS = {k: f"{SRC}/{v}" for k, v in NAMES.items()}
MAPS = ("ens_mean", "ens_std", "ens_abs_err", "crps", "fair_crps", "afcrps")
SCALARS = ("crps", "fair_crps", "afcrps", "ens_rmse", "ens_spread", "spread_skill", "ens_abs_err", "ens_std")
PER_LEVEL = ("ens_rmse", "ens_spread")

# vars: {name: (kind, levels)}; map_vars: the variables whose six maps the fixture stores (the others are held by their scalars)
ENS_CASES = {
    "m2": dict(M=2, grid=(7, 19), B=1, T=1, alpha=1.0, lat=False, vars={"t2m": ("t2m", 1), "unit": ("unit", 1)}, map_vars=("t2m", "unit")),
    "m3": dict(M=3, grid=(33, 67), B=2, T=2, alpha=1.0, lat=False, vars={"T": ("T", 5), "sp": ("sp", 1)}, map_vars=("sp",)),
    "m5lat": dict(M=5, grid=(33, 67), B=1, T=1, alpha=1.0, lat=True, vars={"t2m": ("t2m", 1), "q2": ("q", 1)}, map_vars=("t2m", "q2")),
    "m16": dict(M=16, grid=(32, 64), B=1, T=1, alpha=1.0, lat=False, vars={"t2m": ("t2m", 1), "U": ("U", 2)}, map_vars=("t2m", "U")),
    "m17": dict(M=17, grid=(7, 19), B=1, T=1, alpha=1.0, lat=False, vars={"unit": ("unit", 1), "q2": ("q", 1)}, map_vars=("unit", "q2")),
    "m50": dict(M=50, grid=(7, 19), B=1, T=1, alpha=0.95, lat=False, vars={"unit": ("unit", 1), "t2m": ("t2m", 1)}, map_vars=("unit", "t2m")),
    "m64": dict(M=64, grid=(8, 64), B=1, T=1, alpha=1.0, lat=False, vars={"unit": ("unit", 1), "U": ("U", 2)}, map_vars=("unit", "U")),
    "wide": dict(M=4, grid=(3, 1445), B=1, T=1, alpha=1.0, lat=False, vars={"sp": ("sp", 1), "unit": ("unit", 1)}, map_vars=("sp", "unit")),
    "ties": dict(M=4, grid=(7, 19), B=1, T=1, alpha=1.0, lat=False, vars={"equal": ("t2m", 1), "two": ("t2m", 1), "hit": ("t2m", 1)},
                 map_vars=("equal", "two", "hit")),
}


def latitude(H):
    """Degrees, -80 .. 80: cos > 0 everywhere."""
    return -80.0 + 160.0 * np.arange(H, dtype=np.float64) / (H - 1)


def _field(kind, g, M, shape):
    """-> (truth [B, L, T, H, W], members [M, B, L, T, H, W]) float64."""
    u = lambda s: 2.0 * g.random(s) - 1.0      # noqa: E731
    L = shape[1]
    lev = np.arange(L, dtype=np.float64).reshape(1, L, 1, 1, 1)
    ms = (M,) + shape
    if kind == "sp":
        t = 100000.0 + 800.0 * u(shape)
        x = t + 60.0 + 100.0 * u(shape) + 150.0 * u(ms)
    elif kind == "t2m":
        t = 280.0 + 15.0 * u(shape)
        x = t + 0.3 + 1.0 * u(shape) + 1.5 * u(ms)
    elif kind == "q":
        t = 0.001 * (0.5 + g.random(shape))
        x = t * (0.9 + 0.2 * g.random(shape)) * (0.8 + 0.4 * g.random(ms))
    elif kind == "T":
        t = 215.0 + 0.5 * lev + 8.0 * u(shape)
        x = t - 0.4 + 0.8 * u(shape) + 1.2 * u(ms)
    elif kind == "U":
        t = 3.0 * lev - 20.0 + 9.0 * u(shape)
        x = t + 0.5 + 2.0 * u(shape) + 2.5 * u(ms)
    else:
        t = u(shape)
        x = t + 0.05 + 0.2 * u(shape) + 0.3 * u(ms)
    return t, x


def _coincidences(t, x):
    """bool [B, L, T, H, W]: some member equals another member or the truth there (float32 arrays)."""
    allv = np.sort(np.concatenate([t[None], x], axis=0), axis=0)
    return (np.diff(allv, axis=0) == 0).any(axis=0)


_STEP = {"sp": 8.0, "t2m": 0.125, "q": 2.0 ** -16, "T": 0.125, "U": 0.25, "unit": 2.0 ** -6}


def _move_apart(kind, t, x):
    """Where float32 values coincide, member m is moved by (m + 1) steps of a power of two well inside the variable's spread: a fixed
    rule, applied once; the caller asserts that nothing coincides afterwards."""
    hit = _coincidences(t, x)
    if hit.any():
        step = np.float32(_STEP[kind])
        for m in range(x.shape[0]):
            x[m] = np.where(hit, x[m] + step * np.float32(m + 1), x[m]).astype(np.float32)
    return int(hit.sum())


def case_inputs(case, check=None):
    """-> dict(truth={name: float32 [B, L, T, H, W]}, members={name: float32 [M, B, L, T, H, W]}, lat=float64 [H], moved={name: count}).
    `check`: an opened fixture whose sha256 entries must match."""
    c = ENS_CASES[case]
    H, W = c["grid"]
    M, B, T = c["M"], c["B"], c["T"]
    g = np.random.Generator(np.random.Philox(key=[2031, sorted(ENS_CASES).index(case)]))
    out = dict(truth={}, members={}, lat=latitude(H), moved={})
    for name, (kind, L) in c["vars"].items():
        t, x = _field(kind, g, M, (B, L, T, H, W))
        t, x = t.astype(np.float32), x.astype(np.float32)
        if case == "ties":
            if name == "equal":
                x = np.broadcast_to(x[:1], x.shape).copy()
            elif name == "two":
                x[1] = x[0]
            else:
                x[2] = t
            out["moved"][name] = 0
        else:
            out["moved"][name] = _move_apart(kind, t, x)
            assert not _coincidences(t, x).any(), f"{case}/{name}: a member equals another member or the truth"
        out["truth"][name], out["members"][name] = t, x
    if check is not None:
        for what, arr in flat_inputs(out).items():
            assert input_digest(arr) == str(check[f"sha256:{what}"]), f"{case}: regenerated input {what} differs from the fixture's"
    return out


def flat_inputs(inp):
    flat = {f"truth:{k}": v for k, v in inp["truth"].items()}
    flat.update({f"members:{k}": v for k, v in inp["members"].items()})
    return flat


def input_digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def stacked(x):
    """[M, B, ...] -> the reference's [B * M, ...]: member m of item b in row b * M + m."""
    M, B = x.shape[:2]
    return np.ascontiguousarray(np.moveaxis(x, 0, 1)).reshape((B * M,) + x.shape[2:])


def block_args(case, inp):
    """The keyword arguments of wxengine.ensemble_metrics.EnsembleVerification (maps aside) for a case."""
    c = ENS_CASES[case]
    kw = dict(n_members=c["M"], alpha=c["alpha"])
    if c["lat"]:
        kw.update(use_latitude_weights=True, latitude=inp["lat"])
    return kw


def scalar_keys(case):
    """The flat scalar keys of a case in the order of a result (arrays expanded per level)."""
    c = ENS_CASES[case]
    names = sorted(c["vars"], key=lambda n: KEYS[n])
    keys = []
    for s in SCALARS:
        for n in names:
            keys.append(f"{s}/{KEYS[n]}")
            if s in PER_LEVEL:
                keys += [f"{s}/{KEYS[n]}/{lev}" for lev in range(c["vars"][n][1])]
    for n in names:
        keys += [f"crps_per_channel/{KEYS[n]}/{lev}" for lev in range(c["vars"][n][1])]
    return keys


def flat_scalars(result):
    """A result dict (device or restatement) -> {flat key: float} with the per-channel arrays expanded per level."""
    out = {}
    for k, v in result.items():
        if k.startswith("crps_per_channel/"):
            out.update({f"{k}/{lev}": float(x) for lev, x in enumerate(np.asarray(v).reshape(-1))})
        else:
            out[k] = float(v)
    return out


def distance(a, b, scale):
    a, b = float(a), float(b)
    if a == b:
        return 0.0
    return abs(a - b) / scale if scale > 0 else float("inf")


def map_distance(a, b, scale):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = float(np.abs(a - b).max())
    if d == 0.0:
        return 0.0
    return d / scale if scale > 0 else float("inf")


def load_golden(case, gold_dir):
    """-> dict(fix=fixture, keys=[flat scalar keys], f32, f64, d_ref, scale: float64 [n]; maps={(map, name): dict(f32, f64, d_ref,
    scale)}); a map's fp64 golden is stored as its float32 difference from the fp32 golden (ens_<case>_f64.npz), the layout of the
    hybrid fixtures."""
    g = np.load(os.path.join(gold_dir, f"ens_{case}.npz"))
    g64 = np.load(os.path.join(gold_dir, f"ens_{case}_f64.npz"))
    out = dict(fix=g, keys=[str(k) for k in g["keys"]], f32=g["f32"], f64=g64["f64"], d_ref=g["d_ref"], scale=g["scale"], maps={})
    for name in ENS_CASES[case]["map_vars"]:
        for m in MAPS:
            f32 = g[f"map32:{m}:{name}"]
            out["maps"][(m, name)] = dict(f32=f32, f64=f32.astype(np.float64) + g64[f"d64:{m}:{name}"].astype(np.float64),
                                          d_ref=float(g[f"map_d_ref:{m}:{name}"]), scale=float(g[f"map_scale:{m}:{name}"]))
    return out
