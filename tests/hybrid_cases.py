"""Inputs of the hybrid-level-interpolation fixtures (tests/golden/hybrid_<case>.npz, tools/make_goldens.py --only hybrid), shared by
the generator, the CPU oracle tests and the GPU tests.

The 3-D inputs are not stored: they are rebuilt here from the keyed Philox stream with +, -, *, / and comparisons only (IEEE-exact, so
every machine gets the same bits); the fixture stores their SHA-256 and `case_inputs(..., check=fixture)` compares.  Grids: G9 =
33 x 67 (2 211 columns: nine workgroups of 256, a partial last one) and G1 = 7 x 19 (133 columns: one partial workgroup) where the
G9 fixture would pass 1 MB (the 127- and 137-level cases, and `shuf` with its ten variables).

Three coefficient families, all  a = (eta - b) p0,  half levels x = k / L:
  F1  diag_cases.hybrid_coefficients: eta = 0.3 x + 0.7 x^2, b = eta^2
  F2  eta = 0.6 x + 0.4 x^3, b = eta^2          (another spacing: its levels interleave with F1's)
  F3  eta = 0.5 x + 0.5 x^2, b = eta^3          (DESTINATION only: below sp = 2/3 p0 its pressures are not monotone in the level
                                                 index, so a column's own order differs from the order at 101325 Pa)
With b = eta^2, a + b sp rises strictly with the level index for every sp > p0 / 2; the surface pressure spans 520 - 1040 hPa.
Every case carries the variable `idx` whose value is the source level index m counted top -> surface: its output is lo + w, the
bracket and the weight themselves, undiluted by a field."""
import hashlib
import os

import numpy as np

from diag_cases import distance, hybrid_coefficients  # noqa: F401  (distance: re-exported for the tests)

GRIDS = {"G9": (33, 67), "G1": (7, 19)}
P0 = 101325.0
MIN_P = 0.57
SRC = "GFS"
SP_SRC = "GFS"
KEYS = {"T": f"{SRC}/prognostic/3d/temperature", "q": f"{SRC}/prognostic/3d/specific_humidity", "idx": f"{SRC}/prognostic/3d/level_index",
        "sp": f"{SP_SRC}/prognostic/2d/surface_pressure"}
KEYS.update({f"f{i}": f"{SRC}/prognostic/3d/field_{i}" for i in range(7)})
HITS = ("above top", "interior", "below bottom")

# src / dst: (family, number of levels); s2t: the source is stored surface -> top; fields: besides `idx`; hits: which of HITS the
# destination levels reach in some column (the generator asserts exactly these)
HYBRID_CASES = {
    "L16to13": dict(grid="G9", B=1, T=1, src=("F1", 16), dst=("F2", 13), fields=("T", "q"), hits=("interior",)),
    "L13s2t": dict(grid="G9", B=1, T=1, src=("F2", 13), dst=("F1", 16), s2t=True, fields=("T", "q"), hits=HITS),
    "L2b2t2": dict(grid="G9", B=2, T=2, src=("F1", 2), dst=("F2", 5), fields=("T", "q"), hits=HITS),
    "shuf": dict(grid="G1", B=1, T=1, src=("F1", 40), dst=("F3", 32), shuffle=True, fields=("T", "q") + tuple(f"f{i}" for i in range(7)),
                 hits=("interior", "below bottom")),
    "L137": dict(grid="G1", B=1, T=1, src=("F1", 137), dst=("F2", 127), fields=("T", "q"), hits=("interior",)),
    "L127": dict(grid="G1", B=1, T=2, src=("F2", 127), dst=("F1", 137), vcoord=True, fields=("T", "q"), hits=HITS),
    "L127sub": dict(grid="G1", B=1, T=2, src=("F2", 127), dst=("F1", 137), vcoord=True, source_levels=list(range(2, 128, 2)),
                    fields=("T", "q"), hits=HITS),
    "one": dict(grid="G1", B=1, T=1, src=("F1", 16), dst=("F2", 5), dest_levels=[3], fields=("T", "q"), hits=("interior",)),
    "floor": dict(grid="G1", B=1, T=1, src=("F1", 8), dst=("F2", 8), src_midpoints=True, fields=("T", "q"), hits=("interior", "below bottom")),
}


def family(which, L):
    """-> (a, b) float64 on the L + 1 interfaces, top -> surface."""
    if which == "F1":
        a_half, b_half, _, _ = hybrid_coefficients(L)
        return a_half.astype(np.float64), b_half.astype(np.float64)
    x = np.arange(L + 1, dtype=np.float64) / L
    if which == "F2":
        eta = 0.6 * x + 0.4 * x * x * x
        b = eta * eta
    else:
        eta = 0.5 * x + 0.5 * x * x
        b = eta * eta * eta
    return ((eta - b) * P0).astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)


def raw_coefficients(name):
    """The coefficient arguments of a case as the block's constructor takes them (arrays in the place of the reference's files):
    source_a, source_b (None with the 2-D vcoord array), source_on_interfaces, source_levels, dest_a, dest_b, dest_on_interfaces,
    dest_levels."""
    c = HYBRID_CASES[name]
    g = np.random.Generator(np.random.Philox(key=[2027, 1000 + sorted(HYBRID_CASES).index(name)]))
    sa, sb = family(*c["src"])
    da, db = family(*c["dst"])
    out = dict(source_on_interfaces=True, source_levels=c.get("source_levels"), dest_on_interfaces=True, dest_levels=c.get("dest_levels"))
    if c.get("src_midpoints"):       # the interfaces 0 .. L - 1 taken AS midpoints: a[0] = b[0] = 0, the one level at the 0.57 Pa floor
        sa, sb = sa[:-1], sb[:-1]
        out["source_on_interfaces"] = False
    if c.get("s2t"):
        sa, sb = sa[::-1], sb[::-1]
    if c.get("shuffle"):             # the destination given on midpoints, in shuffled order
        order = g.permutation(c["dst"][1])
        da, db = (0.5 * (da[:-1] + da[1:]))[order], (0.5 * (db[:-1] + db[1:]))[order]
        out["dest_on_interfaces"] = False
    if c.get("vcoord"):
        out.update(source_a=np.ascontiguousarray(np.stack([sa, sb])), source_b=None)
    else:
        out.update(source_a=np.ascontiguousarray(sa), source_b=np.ascontiguousarray(sb))
    out.update(dest_a=np.ascontiguousarray(da), dest_b=np.ascontiguousarray(db))
    return out


def midpoints(name):
    """-> (source_a, source_b, dest_a, dest_b) float32 at level midpoints in stored order: what _interp_utils.py:69-80 makes of
    raw_coefficients(name), written out here independently of wxengine.hybrid_interp.midpoint_coefficients."""
    r = raw_coefficients(name)

    def mid(a, b, on_interfaces, levels):
        a = np.asarray(a, np.float64)
        if b is None:
            a, b = a[0], a[1]
        b = np.asarray(b, np.float64)
        if on_interfaces:
            a, b = 0.5 * (a[:-1] + a[1:]), 0.5 * (b[:-1] + b[1:])
        if levels is not None:
            a, b = a[[lv - 1 for lv in levels]], b[[lv - 1 for lv in levels]]
        return a.astype(np.float32), b.astype(np.float32)
    return (mid(r["source_a"], r["source_b"], r["source_on_interfaces"], r["source_levels"])
            + mid(r["dest_a"], r["dest_b"], r["dest_on_interfaces"], r["dest_levels"]))


def variables(name):
    """The interpolated variables of a case in order: the fields, then `idx`."""
    return tuple(HYBRID_CASES[name]["fields"]) + ("idx",)


def block_args(name):
    """The keyword arguments of wxengine.hybrid_interp.HybridLevelInterp for a case."""
    return dict(variables=[KEYS[v] for v in variables(name)], surface_pressure_var=KEYS["sp"], **raw_coefficients(name))


def reference_args(name):
    """-> (keyword arguments of the reference's HybridLevelInterpPost, arrays its level-info files hold)."""
    r = raw_coefficients(name)
    vc = r["source_b"] is None
    arrays = {"dst_a": r["dest_a"], "dst_b": r["dest_b"]}
    arrays.update({"vcoord": r["source_a"]} if vc else {"src_a": r["source_a"], "src_b": r["source_b"]})
    kw = dict(variables=[KEYS[v] for v in variables(name)], surface_pressure_var=KEYS["sp"], source_level_info_file="source_levels.nc",
              dest_level_info_file="dest_levels.nc", source_a_var="vcoord" if vc else "src_a", source_b_var="vcoord" if vc else "src_b",
              source_on_interfaces=r["source_on_interfaces"], source_levels=r["source_levels"], dest_a_var="dst_a", dest_b_var="dst_b",
              dest_on_interfaces=r["dest_on_interfaces"], dest_levels=r["dest_levels"])
    return kw, arrays


def case_inputs(name, check=None):
    """-> {field | "idx": float32 [B, Ls, T, H, W] in STORED level order, "sp": float32 [B, 1, T, H, W]}.  `check`: an opened fixture
    whose sha256 entries must match."""
    c = HYBRID_CASES[name]
    H, W = GRIDS[c["grid"]]
    B, T = c["B"], c["T"]
    g = np.random.Generator(np.random.Philox(key=[2027, sorted(HYBRID_CASES).index(name)]))
    sa, sb, _, _ = midpoints(name)
    if c.get("s2t"):
        sa, sb = sa[::-1], sb[::-1]          # top -> surface for building the atmosphere
    Ls = sa.size
    sp = (52000.0 + 52000.0 * g.random((B, 1, T, H, W))).astype(np.float32)
    sp64 = sp.astype(np.float64)
    s = np.maximum(sa.astype(np.float64).reshape(1, Ls, 1, 1, 1) + sb.astype(np.float64).reshape(1, Ls, 1, 1, 1) * sp64, MIN_P) / sp64
    shape3 = (B, Ls, T, H, W)
    t_surf = 288.0 + (60.0 * g.random((B, 1, T, H, W)) - 40.0)
    out = {"sp": sp}
    for f in c["fields"]:
        if f == "T":         # smooth in p / sp, falling towards 215 K, plus 1 K of noise
            x = 215.0 + (t_surf - 215.0) * s + (2.0 * g.random(shape3) - 1.0)
        elif f == "q":       # five decades between the surface and the top
            x = 0.012 * s * s * s * (0.2 + 0.8 * g.random(shape3))
        else:                # unit noise around a level-dependent mean, both signs
            x = 2.0 * g.random(shape3) - 1.0 + 3.0 * (s - 0.5)
        out[f] = x.astype(np.float32)
    out["idx"] = np.broadcast_to(np.arange(Ls, dtype=np.float32).reshape(1, Ls, 1, 1, 1), shape3).copy()
    if c.get("s2t"):
        for k in out:
            if k != "sp":
                out[k] = np.ascontiguousarray(out[k][:, ::-1])
    if check is not None:
        for k in out:
            assert input_digest(out[k]) == str(check[f"sha256:{k}"]), f"{name}: regenerated input {k} differs from the fixture's"
    return out


def input_digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def check_conditions(name, inp):
    """What a case is there for, asserted on its regenerated inputs (float32 pressures, as every implementation forms them): source
    pressures strictly increasing top -> surface in every column (a tie makes the reference divide 0 by 0), the destination levels hit
    exactly the stated ones of HITS, `floor` has exactly one level at the 0.57 Pa floor, `shuf`'s destination order differs from its
    order at 101325 Pa in some columns (and not in all).  -> a one-line summary."""
    c = HYBRID_CASES[name]
    sa, sb, da, db = midpoints(name)
    if (sa[0] + sb[0] * np.float32(P0)) > (sa[-1] + sb[-1] * np.float32(P0)):
        assert c.get("s2t"), name
        sa, sb = sa[::-1], sb[::-1]
    else:
        assert not c.get("s2t"), name
    sp = inp["sp"].reshape(-1, 1)
    ps = np.maximum(sa.reshape(1, -1) + sb.reshape(1, -1) * sp, np.float32(MIN_P))
    pd = np.maximum(da.reshape(1, -1) + db.reshape(1, -1) * sp, np.float32(MIN_P))
    assert ps.dtype == np.float32 and (np.diff(ps, axis=1) > 0).all(), f"{name}: source pressures not strictly increasing in every column"
    assert sp.min() < 56000 and sp.max() > 100000, name
    hit = {"above top": bool((pd < ps[:, :1]).any()), "below bottom": bool((pd > ps[:, -1:]).any()),
           "interior": bool(((pd >= ps[:, :1]) & (pd <= ps[:, -1:])).any())}
    assert {k for k, v in hit.items() if v} == set(c["hits"]), (name, hit, c["hits"])
    at_floor = int((ps[0] == np.float32(MIN_P)).sum())
    assert at_floor == (1 if name == "floor" else 0) and (ps == np.float32(MIN_P)).sum() == at_floor * ps.shape[0], name
    note = ""
    if c.get("shuffle"):
        ref_order = np.argsort(da + db * np.float32(P0), kind="stable")
        assert not np.array_equal(ref_order, np.arange(da.size)), name
        crossed = (np.diff(pd[:, ref_order], axis=1) < 0).any(axis=1)
        assert crossed.any() and not crossed.all(), (name, crossed.mean())
        note = f", destination order differs from the order at 101325 Pa in {int(crossed.sum())} of {crossed.size} columns"
    return f"{ps.shape[0]} columns, {sa.size} -> {da.size} levels, hits {sorted(c['hits'])}{note}"


def gate(d_ref):
    """(bound against the fp32 golden, bound against the fp64 golden) from the reference's own fp32-against-fp64 distance of the same
    variable: max(4 d_ref, 2e-6) and max(5 d_ref, 2e-6) -- diag_cases.gate with its floor on both sides, as for the advection."""
    return max(4.0 * d_ref, 2e-6), max(5.0 * d_ref, 2e-6)


def load_golden(name, gold_dir):
    """-> (fixture, {var: fp32 golden}, {var: fp64 golden}, {var: d_ref}); the fp64 golden is stored as its float32 difference from
    the fp32 golden (hybrid_<case>_f64.npz), the layout of the diag fixtures."""
    g = np.load(os.path.join(gold_dir, f"hybrid_{name}.npz"))
    g64 = np.load(os.path.join(gold_dir, f"hybrid_{name}_f64.npz"))
    vs = variables(name)
    f32 = {v: g[f"f32:{v}"] for v in vs}
    f64 = {v: f32[v].astype(np.float64) + g64[f"d64:{v}"].astype(np.float64) for v in vs}
    d_ref = {v: float(g[f"d_ref:{v}"]) for v in vs}
    return g, f32, f64, d_ref
