"""Inputs of the semi-Lagrangian-advection fixtures (tests/golden/advect_<case>.npz, tools/make_goldens.py --only advect), shared by
the generator, the CPU oracle tests and the GPU tests.

The fields are not stored: they are rebuilt here from the keyed Philox stream with +, -, *, / and comparisons only (IEEE-exact, so
every machine gets the same bits); the fixture stores their SHA-256 and `case_inputs(..., check=fixture)` compares.

Winds are given in GRID UNITS and converted to m/s with the grid's own spacing, so that every case moves its tracers by a few cells
whatever its resolution: U = cos(lat) (a zonal jet that varies with longitude and level + noise), V = cos(lat) (a meridional wave that
grows towards the poles + noise); the noise is what gives the flow its divergence, hence omega.  `cos` is a 14-term series (exact arithmetic).  Scaling by
cos(lat) keeps the winds at the poles at zero, where the reference divides by its floor of 1e-4; `polewind` adds 12 m/s (1 - cos lat)
to U to put a real wind there.  Tracers are unit-variance noise (q: plus a vertical gradient), constant in longitude on rows that are
exact poles.  Surface pressure is 950 - 1030 hPa noise.  With B = 2 the second batch item has its own draws.  `surface_to_top` cases
store U, V, omega and the tracers with the level axis flipped; the coefficients stay top -> surface.

Rows within two of either edge (h < 2 or h >= H - 2) are the "edge" region, the rest the "interior": the reference's own
fp32-against-fp64 distance near the poles is one to four orders above the interior's, so every fixture stores d_ref per output AND
region, and every comparison is made per region."""
import hashlib
import os

import numpy as np

from diag_cases import hybrid_coefficients

SRC = "ERA5"
KEYS = {"U": f"{SRC}/prognostic/3d/u_component_of_wind", "V": f"{SRC}/prognostic/3d/v_component_of_wind",
        "sp": f"{SRC}/prognostic/2d/surface_pressure", "q": f"{SRC}/prognostic/3d/specific_humidity",
        "T": f"{SRC}/prognostic/3d/temperature", "omega": f"{SRC}/diagnostic/3d/vertical_velocity"}
R_EARTH, DT = 6371000.0, 21600.0
REGIONS = ("interior", "edge")

# args: constructor arguments that differ from the defaults; tracers: tracer_vars in order; cols / rows: wind amplitudes in grid cells
# per time step at the equator (jet, noise); coef: levels of the hybrid coefficient set the case slices with `levels`
ADVECT_CASES = {
    "tiny": dict(B=1, L=2, H=7, W=19, tracers=("q",), args={}),
    "base36": dict(B=1, L=5, H=24, W=36, tracers=("q", "T"), args={}),
    "b2s2t": dict(B=2, L=4, H=33, W=50, tracers=("q", "T"), args=dict(level_order="surface_to_top")),
    "iter3": dict(B=1, L=8, H=48, W=72, tracers=("q",), args=dict(n_iterations=3, levels=list(range(3, 11))), coef=12),
    "gauss": dict(B=1, L=6, H=25, W=40, tracers=("q", "T"), args=dict(n_iterations=1), lat="gauss"),
    "omega": dict(B=1, L=5, H=24, W=36, tracers=("q",), args=dict(omega_var=KEYS["omega"])),
    "polewind": dict(B=1, L=5, H=24, W=36, tracers=("q", "T"), args={}, polewind=12.0),
}
WIND = dict(jet_cols=4.5, noise_cols=0.6, wave_rows=1.6, noise_rows=0.35, polar=0.0, polar_squarings=2)     # grid cells per time step at the equator
# V = cos(lat) * (wave * (1 + polar * sin(lat)^(2^(k+1))) + noise): on a grid with both pole rows a back-trajectory that starts one row
# from a pole samples its velocity between that row and the pole, where cos(lat) ends V, so a wave of the same amplitude at every
# latitude cannot carry it past the pole row.  The wave therefore grows towards the poles (k = polar_squarings keeps the growth to the
# last rows, so that interior points stay clear of the pole rows' own conditioning), enough for departure ROWS to leave [0, H - 1] in
# every case; the generator asserts it.
# (amplitudes found by scanning against the generator's conditions; the rows next to a pole are where the reference is worst conditioned)
_POLAR = dict(polar=18.0, polar_squarings=5)
WIND_OF_CASE = {"tiny": dict(wave_rows=3.2), "base36": dict(polar=32.0, polar_squarings=3), "omega": _POLAR, "polewind": _POLAR,
                "b2s2t": dict(_POLAR, polar=22.0), "iter3": dict(_POLAR, polar=12.0)}


def _cos(x):
    """cos(x) for |x| <= pi / 2 from +, * alone (14 terms): the same bits everywhere."""
    x2 = np.asarray(x, np.float64) ** 2
    s = np.ones_like(x2)
    for k in range(14, 0, -1):
        s = 1.0 - x2 * s / ((2 * k - 1) * (2 * k))
    return s


def _noise(g, shape):
    """Unit variance from four uniforms: (sum - 2) * sqrt(3)."""
    return (g.random(shape) + g.random(shape) + g.random(shape) + g.random(shape) - 2.0) * 1.7320508075688772


def grid_of(name):
    """-> (latitude [H], longitude [W]) in float32 degrees.  Uniform 90 -> -90 with both poles, or ("gauss") non-uniform latitudes
    stored south -> north between -87 and 87, denser towards the equator."""
    c = ADVECT_CASES[name]
    H, W = c["H"], c["W"]
    t = 2.0 * np.arange(H, dtype=np.float64) / (H - 1) - 1.0
    lat = 87.0 * (1.2 * t - 0.2 * t * t * t) if c.get("lat") == "gauss" else -90.0 * t
    return lat.astype(np.float32), (np.arange(W, dtype=np.float64) * (360.0 / W)).astype(np.float32)


def coefficients(name):
    """-> (model_a_half, model_b_half) as the block's constructor takes them (before `levels` slices them), float32, top -> surface."""
    c = ADVECT_CASES[name]
    a_half, b_half, _, _ = hybrid_coefficients(c.get("coef", c["L"]))
    return a_half, b_half


def block_args(name):
    """The keyword arguments of SemiLagrangianAdvection (device) for a case."""
    c = ADVECT_CASES[name]
    a_half, b_half = coefficients(name)
    lat, lon = grid_of(name)
    return dict(tracer_vars=[KEYS[t] for t in c["tracers"]], u_var=KEYS["U"], v_var=KEYS["V"], surface_pressure_var=KEYS["sp"],
                model_a_half=a_half, model_b_half=b_half, latitude=lat, longitude=lon, **c["args"])


def oracle_args(name):
    """The keyword arguments of advect_oracle.advect for a case (coefficients already sliced)."""
    c = ADVECT_CASES[name]
    a_half, b_half = coefficients(name)
    lv = c["args"].get("levels")
    if lv is not None:
        idx = [i - 1 for i in lv] + [lv[-1]]
        a_half, b_half = a_half[idx], b_half[idx]
    lat, lon = grid_of(name)
    return dict(u_key=KEYS["U"], v_key=KEYS["V"], sp_key=KEYS["sp"], tracers=[KEYS[t] for t in c["tracers"]], a_half=a_half, b_half=b_half,
                lat_deg=lat, lon_deg=lon, dt=DT, n_iterations=c["args"].get("n_iterations", 2), omega_key=c["args"].get("omega_var"),
                level_order=c["args"].get("level_order", "top_to_surface"))


def input_names(name):
    c = ADVECT_CASES[name]
    return ["U", "V", "sp"] + (["omega"] if "omega_var" in c["args"] else []) + [t for t in ("q", "T") if t in c["tracers"]]


def case_inputs(name, check=None):
    """-> {"U" | "V" | tracer | "omega": float32 [B, L, 1, H, W], "sp": float32 [B, 1, 1, H, W]} in the data's level order.
    `check`: an opened fixture whose sha256 entries must match."""
    c = ADVECT_CASES[name]
    B, L, H, W = c["B"], c["L"], c["H"], c["W"]
    amp = dict(WIND, **WIND_OF_CASE.get(name, {}))
    g = np.random.Generator(np.random.Philox(key=[2026, sorted(ADVECT_CASES).index(name)]))
    lat, _ = grid_of(name)
    lat64 = lat.astype(np.float64)
    coslat = _cos(lat64 * (np.pi / 180.0)).reshape(1, 1, 1, H, 1)
    pole = np.abs(lat64) == 90.0
    col_ms = R_EARTH * (2.0 * np.pi / W) / DT                       # m/s that move one column per step at the equator
    row_ms = R_EARTH * (np.abs(lat64[-1] - lat64[0]) * (np.pi / 180.0) / (H - 1)) / DT     # ... one (mean) row per step
    f = (np.arange(W, dtype=np.float64) / W).reshape(1, 1, 1, 1, W)
    lon_wave = 4.0 * f * (1.0 - f)                                   # 0 .. 1 .. 0 around the circle, continuous
    f2 = np.where(f < 0.5, 2.0 * f, 2.0 * f - 1.0)
    lon_wave2 = 8.0 * f2 * (1.0 - f2) - 1.0                          # two waves around the circle, -1 .. 1
    lev = (np.arange(L, dtype=np.float64) / L).reshape(1, L, 1, 1, 1)
    item = (1.0 - 0.3 * np.arange(B, dtype=np.float64)).reshape(B, 1, 1, 1, 1)
    shape = (B, L, 1, H, W)
    u = coslat * col_ms * (amp["jet_cols"] * item * (0.6 + 0.4 * lon_wave) * (1.0 - 0.4 * lev) + amp["noise_cols"] * _noise(g, shape))
    sin2 = 1.0 - coslat * coslat
    sharp = sin2
    for _ in range(amp["polar_squarings"]):
        sharp = sharp * sharp
    polar = 1.0 + amp["polar"] * sharp      # the meridional wave grows towards the poles; cos(lat) still ends it there
    v = coslat * row_ms * (amp["wave_rows"] * polar * item * lon_wave2 * (0.7 + 0.6 * lev) + amp["noise_rows"] * _noise(g, shape))
    if "polewind" in c:
        u = u + c["polewind"] * (1.0 - coslat)
    out = {"U": u.astype(np.float32), "V": v.astype(np.float32),
           "sp": (95000.0 + 8000.0 * g.random((B, 1, 1, H, W))).astype(np.float32)}
    if "omega_var" in c["args"]:
        out["omega"] = (g.random(shape) - 0.5).astype(np.float32)
    for t in ("q", "T"):
        if t in c["tracers"]:
            x = _noise(g, shape) + (2.0 * lev if t == "q" else 0.0)
            x[:, :, :, pole, :] = x[:, :, :, pole, :1]                # one value around an exact pole
            out[t] = x.astype(np.float32)
    if c["args"].get("level_order") == "surface_to_top":
        for k in out:
            if k != "sp":
                out[k] = np.ascontiguousarray(out[k][:, ::-1])
    if check is not None:
        for k in input_names(name):
            assert input_digest(out[k]) == str(check[f"sha256:{k}"]), f"{name}: regenerated input {k} differs from the fixture's"
    return out


def input_digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def region_rows(H):
    """{"interior": row indices, "edge": row indices}: rows within two of either edge are the edge region."""
    h = np.arange(H)
    edge = (h < 2) | (h >= H - 2)
    return {"interior": h[~edge], "edge": h[edge]}


def region_distance(a, b, rows):
    """diag_cases.distance over the rows of one region: max |a - b| / max |b|, arrays [B, L, 1, H, W]."""
    from diag_cases import distance
    return distance(np.asarray(a)[..., rows, :], np.asarray(b)[..., rows, :])


def gate(d_ref):
    """(bound against the fp32 golden, bound against the fp64 golden) from the reference's own fp32-against-fp64 distance of the same
    output and region: max(4 d_ref, 2e-6) and max(5 d_ref, 2e-6) -- diag_cases.gate with its floor on both sides: the fp32 index
    arithmetic (a column coordinate up to W, rounded to 2^-24 relative) has an absolute error of about W 2^-24 whatever d_ref is."""
    return max(4.0 * d_ref, 2e-6), max(5.0 * d_ref, 2e-6)


def load_golden(name, gold_dir):
    """-> (fixture, {tracer: fp32 golden}, {tracer: fp64 golden}, {(tracer, region): d_ref}); the fp64 golden is stored as its
    float32 difference from the fp32 golden (advect_<case>_f64.npz), the layout of the diag fixtures."""
    g = np.load(os.path.join(gold_dir, f"advect_{name}.npz"))
    g64 = np.load(os.path.join(gold_dir, f"advect_{name}_f64.npz"))
    tr = ADVECT_CASES[name]["tracers"]
    f32 = {t: g[f"f32:{t}"] for t in tr}
    f64 = {t: f32[t].astype(np.float64) + g64[f"d64:{t}"].astype(np.float64) for t in tr}
    d_ref = {(t, r): float(g[f"d_ref:{t}:{r}"]) for t in tr for r in REGIONS}
    return g, f32, f64, d_ref
