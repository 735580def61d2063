"""Inputs of the pressure-level-product fixtures (tests/golden/diag_<case>.npz, tools/make_goldens.py --only diag), shared by
the generator, the CPU oracle tests and the GPU tests.

The 3-D inputs are not stored: they are rebuilt here from the keyed Philox stream with +, -, *, / and comparisons only (IEEE-exact,
so every machine gets the same bits); the fixture stores their SHA-256 and `case_inputs(..., check=fixture)` compares.  Grids:
G9 = 33 x 67 (2 211 columns: nine workgroups of 256, a partial last one; at 128 / 64 / 32 threads a partial last one too) and, for
the two level counts whose G9 fixture would pass 1 MB, G1 = 7 x 19 (133 columns: partial workgroups at 64 and at 32 threads).

What the columns cover: surface pressure 520 - 1040 hPa tied to the surface height through a standard-atmosphere power law; heights in
all three Trenberth regimes (< 2000 m, 2000 - 2500 m, > 2500 m) and a fifth of the columns with PHIS exactly 0; near-surface
temperatures on both sides of 255 K and 290.5 K, and sea-level temperatures above 290.5 K under colder surfaces (every MSLP case);
a_half[0] = b_half[0] = 0 (the 0.57 Pa replacement); target levels out of order, one above the model top, 1000 and 1050 hPa below
much of the ground.  Temperatures fall linearly in p / sp towards 215 K, so the extrapolated values stay physical."""
import hashlib

import numpy as np

GRIDS = {"G9": (33, 67), "G1": (7, 19)}
P0 = 101325.0

# levels: number of model levels; s2t: stored surface -> top (then flip_vertical is False: the reference integrates in stored order);
# plev in hPa
DIAG_CASES = {
    "L16": dict(grid="G9", B=1, T=1, phis_T=1, levels=16, s2t=False, flip_vertical=True, n_fields=3,
                plev=[500.0, 1050.0, 5.0, 850.0, 1000.0, 250.0, 700.0]),
    "L13s2t": dict(grid="G9", B=1, T=1, phis_T=1, levels=13, s2t=True, flip_vertical=False, n_fields=3,
                   plev=[850.0, 1050.0, 5.0, 300.0, 1000.0, 600.0]),
    "L2bt": dict(grid="G9", B=2, T=2, phis_T=1, levels=2, s2t=False, flip_vertical=True, n_fields=0,
                 plev=[500.0, 1050.0, 100.0, 1000.0, 300.0, 700.0]),
    "L40": dict(grid="G9", B=1, T=1, phis_T=1, levels=40, s2t=False, flip_vertical=True, n_fields=3,      # 128-thread workgroups
                plev=[1000.0, 2.0, 500.0, 1050.0, 850.0, 200.0]),
    "L70": dict(grid="G1", B=1, T=2, phis_T=2, levels=70, s2t=False, flip_vertical=True, n_fields=3,      # 64-thread workgroups
                plev=[925.0, 2.0, 1050.0, 500.0, 1000.0, 100.0]),
    "L137": dict(grid="G1", B=1, T=1, phis_T=1, levels=137, s2t=False, flip_vertical=True, n_fields=3,    # 32-thread workgroups
                 plev=[1000.0, 1.0, 850.0, 1050.0, 10.0, 500.0]),
}

SRC = "era5"
KEYS = dict(T=f"{SRC}/prognostic/3d/temperature", q=f"{SRC}/prognostic/3d/specific_humidity",
            u=f"{SRC}/prognostic/3d/u_component_of_wind", v=f"{SRC}/prognostic/3d/v_component_of_wind",
            sp=f"{SRC}/prognostic/2d/surface_pressure", t2m=f"{SRC}/prognostic/2d/2m_temperature",
            phis=f"{SRC}/static/2d/geopotential_at_surface", z=f"{SRC}/derived_diagnostic/3d/geopotential",
            mslp=f"{SRC}/derived_diagnostic/2d/mean_sea_level_pressure")
FIELD_ORDER = ("u", "v", "q")     # interp_variables of the cases with n_fields = 3


def hybrid_coefficients(L):
    """Half- and mid-level (a [Pa], b) of a smooth L-level hybrid coordinate, top -> surface, float32.  eta = 0.3 x + 0.7 x^2,
    b = eta^2, a = (eta - b) p0: a_half[0] = b_half[0] = 0, b_half[L] = 1, and a + b sp rises with the index for every sp used."""
    x = np.arange(L + 1, dtype=np.float64) / L
    eta = 0.3 * x + 0.7 * x * x
    b = eta * eta
    a = (eta - b) * P0
    a_half, b_half = a.astype(np.float32), b.astype(np.float32)
    a_mid = (0.5 * (a[:-1] + a[1:])).astype(np.float32)
    b_mid = (0.5 * (b[:-1] + b[1:])).astype(np.float32)
    return a_half, b_half, a_mid, b_mid


def _away(t, ref, thresholds, margin, step):
    """Move entries of `t` whose companion `ref` lies within `margin` of a threshold by `step` (decision margins of the fixture)."""
    for thr in thresholds:
        t = np.where(np.abs(ref(t) - thr) < margin, t + step, t)
    return t


def case_inputs(name, check=None):
    """-> dict of float32 arrays: T, q, u, v [B, L, T, H, W]; sp, t2m [B, 1, T, H, W]; phis [B, 1, phis_T, H, W]; a_half, b_half,
    a_mid, b_mid (in STORED level order), plev_pa.  `check`: an opened fixture whose sha256 entries must match."""
    c = DIAG_CASES[name]
    H, W = GRIDS[c["grid"]]
    B, T, L = c["B"], c["T"], c["levels"]
    g = np.random.Generator(np.random.Philox(key=[2024, sorted(DIAG_CASES).index(name)]))
    a_half, b_half, a_mid, b_mid = hybrid_coefficients(L)
    # surface height: a fifth exactly 0, the rest spread over the three regimes with 5 m of margin around 2000 m and 2500 m
    r, r2 = g.random((B, 1, c["phis_T"], H, W)), g.random((B, 1, c["phis_T"], H, W))
    height = np.where(r < 0.2, 0.0, np.where(r < 0.55, 5.0 + 1990.0 * r2, np.where(r < 0.75, 2005.0 + 490.0 * r2, 2505.0 + 2695.0 * r2)))
    phis = (height * 9.80665).astype(np.float32)
    h_t = np.broadcast_to(height, (B, 1, T, H, W))
    y = 1.0 - h_t / 44330.0
    sp = (P0 * (y * y * y * y * y) * (0.97 + 0.056 * g.random((B, 1, T, H, W)))).astype(np.float32)
    t_surf = np.maximum(288.0 - 0.0065 * h_t + (60.0 * g.random((B, 1, T, H, W)) - 40.0), 225.0)
    t2m = (t_surf + 2.0 * (2.0 * g.random((B, 1, T, H, W)) - 1.0)).astype(np.float32)
    # keep every MSLP decision 0.01 K away from its threshold, for t2m itself and for the sea-level temperature
    t2m = _away(t2m, lambda t: t.astype(np.float64), (255.0, 290.5), 0.01, np.float32(0.03))
    t2m = _away(t2m, lambda t: t.astype(np.float64) + 0.0065 * h_t, (255.0, 290.5), 0.01, np.float32(0.05)).astype(np.float32)
    s = (a_mid.astype(np.float64).reshape(1, L, 1, 1, 1) + b_mid.astype(np.float64).reshape(1, L, 1, 1, 1) * sp.astype(np.float64)) / sp.astype(np.float64)
    shape3 = (B, L, T, H, W)
    temp = (215.0 + (t_surf - 215.0) * s + (2.0 * g.random(shape3) - 1.0)).astype(np.float32)
    q = (0.012 * s * s * s * (0.2 + 0.8 * g.random(shape3))).astype(np.float32)
    u = (30.0 * (1.0 - s) * (2.0 * g.random((B, 1, T, H, W)) - 1.0) + 5.0 * (2.0 * g.random(shape3) - 1.0)).astype(np.float32)
    v = (15.0 * (1.0 - s) * (2.0 * g.random((B, 1, T, H, W)) - 1.0) + 5.0 * (2.0 * g.random(shape3) - 1.0)).astype(np.float32)
    out = dict(T=temp, q=q, u=u, v=v, sp=sp, t2m=t2m, phis=phis, a_half=a_half, b_half=b_half, a_mid=a_mid, b_mid=b_mid,
               plev_pa=(np.asarray(c["plev"], np.float64) * 100.0).astype(np.float32))
    if c["s2t"]:   # the same atmosphere stored surface -> top, coefficients with it
        for k in ("T", "q", "u", "v"):
            out[k] = np.ascontiguousarray(out[k][:, ::-1])
        for k in ("a_half", "b_half", "a_mid", "b_mid"):
            out[k] = np.ascontiguousarray(out[k][::-1])
    if check is not None:
        for k in ("T", "q", "u", "v", "sp", "t2m", "phis"):
            assert input_digest(out[k]) == str(check[f"sha256:{k}"]), f"{name}: regenerated input {k} differs from the fixture's"
    return out


def input_digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def output_names(name):
    """The output variables of a case, in fixture order: model-level Z, the pressure-level set (fields, T, Z), MSLP."""
    n = DIAG_CASES[name]["n_fields"]
    return ["z_model"] + [f"plev_{f}" for f in FIELD_ORDER[:n]] + ["plev_T", "plev_Z", "mslp"]


def distance(a, b):
    """The fixtures' and the gate's distance: max |a - b| / max |b|."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def gate(d_ref):
    """(bound against the fp32 golden, bound against the fp64 golden) from the reference's own fp32-against-fp64 distance: 4 d_ref
    (FMA contraction, the device logf / expf against the host's, another summation order over at most 137 terms) with the 2e-6 floor
    the engine's exact-fp32 path meets, and 5 d_ref."""
    return max(4.0 * d_ref, 2e-6), 5.0 * d_ref


def load_golden(name, gold_dir):
    """-> (fixture, {var: fp32 golden}, {var: fp64 golden}, {var: d_ref}).  The fp64 golden is stored as its float32 difference from
    the fp32 golden (diag_<case>_f64.npz): exact to ~1e-7 of that difference, half the bytes."""
    import os
    g = np.load(os.path.join(gold_dir, f"diag_{name}.npz"))
    g64 = np.load(os.path.join(gold_dir, f"diag_{name}_f64.npz"))
    f32 = {v: g[f"f32:{v}"] for v in output_names(name)}
    f64 = {v: f32[v].astype(np.float64) + g64[f"d64:{v}"].astype(np.float64) for v in output_names(name)}
    d_ref = {v: float(g[f"d_ref:{v}"]) for v in output_names(name)}
    return g, f32, f64, d_ref
