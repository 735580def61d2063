"""Cases and inputs of the variable-transform fixtures (tests/golden/xform_<case>.npz, tools/make_goldens.py --only xform), shared by
the generator, the CPU oracle tests and the GPU tests.

A case is a grid, a batch / time size and a list of variables; each variable names its data recipe, its statistics (per level,
scalar or none), its stacked FillValues blocks, its log / sqrt transform and whether the model predicts it (then it is part of y_pred
and of the output side).  The pre chain of a case is  fill* -> (log | sqrt)? -> normalise -> concat,  the post chain  reconstruct ->
inverse scale -> (exp | square)?.

The inputs are not stored: they are rebuilt here from the keyed Philox stream with +, -, *, / and comparisons only (IEEE-exact, so
every machine gets the same bits); the fixture stores their SHA-256 and `case_inputs(..., check=fixture)` compares.

Grids (the smallest at which the two kernels can still go wrong; 1024 cells per workgroup):
    7 x 19  =  133   one partly filled workgroup, odd H*W: scalar path
    33 x 67 = 2211   three workgroups, the last partial; odd H*W, so the channel-slice views of y_pred start on 4-byte boundaries only
    8 x 64  =  512   the all-aligned 16-byte path
    32 x 36 = 1152   one full workgroup and a partial one on the 16-byte path
Data: q-like products of six uniforms (log-normal-like, 1e-9 .. 2e-2) with exact zeros, -0.0, a few values in [-eps, 0) and -- in
the designated NaN cases -- a few below -eps; precipitation with 60 % zeros, a few negatives and NaNs; sea ice with NaNs."""
import hashlib

import numpy as np

SRC = "era5"
GRIDS = {"G1": (7, 19), "G9": (33, 67), "GA": (8, 64), "GB": (32, 36)}

NAN0 = [{"search": "nan", "fill": 0.0}]
# the docstring example of credit/preblock/fill_values.py:43-55, rule for rule
DOC3 = [{"search": "nan", "fill": -1.0}, {"search": 0.0, "op": "==", "fill": 1.0e-4}, {"search": 0.0, "op": "<", "fill": 0.0}]
# the same three with `<=` in the middle: rules 2 and 3 overlap on the negatives, where the LAST one must win (-> 0.0), and the fills stay
# inside the domain of a log with eps 1e-4
OVERLAP3 = [{"search": "nan", "fill": 1.0e-3}, {"search": 0.0, "op": "<=", "fill": 1.0e-4}, {"search": 0.0, "op": "<", "fill": 0.0}]


def V(name, ft, levels, gen, stats=None, fills=(), xf=None, out=True, **kw):
    three_d = kw.pop("three_d", False)
    dim = "3d" if levels > 1 or three_d else "2d"
    return dict(name=name, key=f"{SRC}/{ft}/{dim}/{name}", levels=levels, gen=gen, stats=stats, fills=list(fills), xf=xf,
                out=out and ft in ("prognostic", "diagnostic"), **kw)


def _f64_fields():
    """64 single-level fields, the kMaxFields limit: every transform kind x (scalar statistics | none), and one fill rule set each."""
    xfs = [("log", "e", 1e-8), ("log", "2", 1e-8), ("log", "10", 1e-4), ("sqrt",), None]
    out = []
    for i in range(64):
        xf = xfs[i % 5]
        gen = "q" if xf is not None else "tp"
        fills = [NAN0] if i % 7 == 3 else ([[{"search": 0.0, "op": "<", "fill": 0.0}]] if i % 7 == 5 else [])
        out.append(V(f"f{i:02d}", "prognostic", 1, gen, stats=("scalar" if i % 3 else None), fills=fills, xf=xf,
                     eps=(xf[2] if xf and xf[0] == "log" else 1e-8), nan_in=(i % 7 == 3), neg_in=(i % 7 == 5)))
    return out


# stats: "level" = per-level vectors, "scalar", None.  xf: ("log", base, eps) | ("sqrt",) | None.  below: values under -eps (log) or
# under 0 (sqrt) that the reference turns into NaN.  nan_y: NaNs in this variable's slice of y_pred (they must propagate).
XFORM_CASES = {
    # the arco_era5_wxformer.yml chain: nan -> 0 on sea ice, natural log of q and surface pressure, exp on the way out
    "arco": dict(grid="G9", B=2, T=1, nan_case=True, variables=[
        V("Q", "prognostic", 13, "q", "level", xf=("log", "e", 1e-8), eps=1e-8, below=True),
        V("T", "prognostic", 3, "t", "level"),
        V("SP", "prognostic", 1, "sp", "scalar", xf=("log", "e", 1e-8)),
        V("TP", "diagnostic", 1, "tp", "scalar", fills=[DOC3], nan_in=True, neg_in=True, nan_y=True),
        V("SIC", "static", 1, "sic", None, fills=[NAN0], nan_in=True)]),
    # B = 2 and T = 2 on the scalar path; base 2 and base 10 with eps 1e-4; the overlapping rule set; two stacked FillValues blocks
    # (the second sees the first one's output: NaN -> 0 -> 0.5); a 13-level variable nobody touches
    "b2t2": dict(grid="G1", B=2, T=2, nan_case=False, variables=[
        V("Q", "prognostic", 1, "q", "scalar", fills=[OVERLAP3], xf=("log", "2", 1e-4), eps=1e-4, nan_in=True, neg_in=True, three_d=True),
        V("U", "prognostic", 13, "u", None),
        V("TP", "diagnostic", 1, "tp", "scalar", fills=[[{"search": 0.0, "op": "<", "fill": 0.0}], NAN0], xf=("log", "10", 1e-4),
          nan_in=True, neg_in=True),
        V("SIC", "static", 1, "sic", None, fills=[NAN0, [{"search": 0.0, "op": "==", "fill": 0.5}, {"search": 0.9, "op": ">=", "fill": 1.0}]],
          nan_in=True)]),
    # sqrt / square on the all-aligned 16-byte path, T = 2
    "sqrt": dict(grid="GA", B=1, T=2, nan_case=True, variables=[
        V("Q", "prognostic", 13, "q", "level", xf=("sqrt",), eps=1e-8, below=True),
        V("T", "prognostic", 13, "t", "level"),
        V("TP", "diagnostic", 1, "tp", None, fills=[[{"search": 0.0, "op": "<", "fill": 0.0}], NAN0], xf=("sqrt",), nan_in=True, neg_in=True)]),
    # 16-byte path with a partial second workgroup, B = 2: base 10 / base 2 with eps 1e-8, natural log with eps 1e-4 and no statistics
    "al16": dict(grid="GB", B=2, T=1, nan_case=False, variables=[
        V("Q", "prognostic", 13, "q", "level", xf=("log", "10", 1e-8), eps=1e-8),
        V("SP", "prognostic", 1, "sp", "scalar", xf=("log", "2", 1e-8)),
        V("TP", "diagnostic", 1, "tp", None, xf=("log", "e", 1e-4))]),
    "f64": dict(grid="G1", B=1, T=1, nan_case=False, variables=_f64_fields()),
}

# (mean, std) of the NORMALISED quantity (after the log / sqrt) at level 0; level l scales them by (1 + 0.05 l) and (1 + 0.03 l)
_STATS = {("q", "log", "e", 1e-8): (9.0, 3.0), ("q", "log", "2", 1e-8): (13.0, 4.0), ("q", "log", "10", 1e-8): (4.0, 1.25),
          ("q", "log", "2", 1e-4): (2.5, 2.0), ("q", "log", "10", 1e-4): (0.8, 0.6), ("q", "log", "e", 1e-4): (1.8, 1.4), ("q", "sqrt"): (0.04, 0.03),
          ("sp", "log", "e", 1e-8): (29.5, 0.2), ("sp", "log", "2", 1e-8): (42.6, 0.3), ("tp", "log", "10", 1e-4): (0.6, 0.8),
          ("tp", "log", "e", 1e-4): (1.4, 1.8), ("tp", "sqrt"): (0.06, 0.07), ("q",): (2e-3, 3e-3), ("t",): (255.0, 30.0), ("sp",): (8e4, 1.5e4),
          ("tp",): (4e-3, 9e-3), ("u",): (0.0, 20.0), ("sic",): (0.3, 0.4)}
# the range of the DE-NORMALISED model output p (log / sqrt space) the y_pred recipe aims at
_P_HI = {("q", "log", "e", 1e-8): 14.5, ("q", "log", "2", 1e-8): 20.9, ("q", "log", "10", 1e-8): 6.3, ("q", "log", "2", 1e-4): 7.6,
         ("q", "log", "10", 1e-4): 2.3, ("q", "log", "e", 1e-4): 5.3, ("q", "sqrt"): 0.14, ("sp", "log", "e", 1e-8): 30.0, ("sp", "log", "2", 1e-8): 43.3,
         ("tp", "log", "10", 1e-4): 2.7, ("tp", "log", "e", 1e-4): 6.2, ("tp", "sqrt"): 0.22}
_P_RANGE = {"q": (-1e-4, 2e-2), "t": (200.0, 310.0), "sp": (5e4, 1.05e5), "tp": (-1e-3, 5e-2), "u": (-40.0, 40.0)}


def _tag(v):
    return (v["gen"],) + tuple(v["xf"] or ())


def variable_stats(v):
    """-> (mean, std) float32 arrays of n_levels (per-level) or 1 (scalar) entries, or (None, None)."""
    if v["stats"] is None:
        return None, None
    m0, s0 = _STATS[_tag(v)]
    lv = np.arange(v["levels"] if v["stats"] == "level" else 1, dtype=np.float64)
    return (m0 * (1.0 + 0.05 * lv)).astype(np.float32), (s0 * (1.0 + 0.03 * lv)).astype(np.float32)


def case_stats(name):
    """-> (mean, std) dicts keyed by variable NAME, as DevicePreblock / InverseScale / InverseTransforms take them."""
    mean, std = {}, {}
    for v in XFORM_CASES[name]["variables"]:
        m, s = variable_stats(v)
        if m is not None:
            mean[v["name"]], std[v["name"]] = (m, s) if v["stats"] == "level" else (np.float32(m[0]), np.float32(s[0]))
    return mean, std


def _field(g, v, shape):
    u = g.random
    eps = v.get("eps", 1e-8)
    r = u(shape)                          # the selector of the special values
    if v["gen"] == "q":
        x = 2e-2 * (0.04 + 0.96 * u(shape)) * (0.04 + 0.96 * u(shape)) * (0.04 + 0.96 * u(shape)) * (0.04 + 0.96 * u(shape)) \
            * (0.04 + 0.96 * u(shape)) * (0.04 + 0.96 * u(shape))
        x = np.maximum(x, 1e-9)
        w = u(shape)
        x = np.where(r < 0.01, 0.0, x)
        x = np.where((r >= 0.01) & (r < 0.02), -0.0, x)
        if not (v["xf"] and v["xf"][0] == "sqrt"):
            x = np.where((r >= 0.02) & (r < 0.03), -0.9 * eps * w, x)                  # in [-eps, 0): still inside the log's domain
        if v.get("below"):
            x = np.where((r >= 0.03) & (r < 0.034), -eps * (1.5 + w), x)               # below -eps: NaN expected (log and sqrt)
        if v.get("neg_in"):
            x = np.where((r >= 0.04) & (r < 0.06), -1e-3 * w, x)                        # negatives a fill rule removes
    elif v["gen"] == "tp":
        w = u(shape)
        x = np.where(r < 0.6, 0.0, 0.05 * w * w * w)
        if v.get("neg_in"):
            x = np.where((r >= 0.6) & (r < 0.63), -1e-3 * w, x)
    elif v["gen"] == "sic":
        x = np.where(r < 0.4, 0.0, np.where(r < 0.5, 1.0, u(shape)))
    elif v["gen"] == "sp":
        x = 5e4 + 5.5e4 * u(shape)
    elif v["gen"] == "t":
        x = 200.0 + 110.0 * u(shape)
    else:
        x = -40.0 + 80.0 * u(shape)
    if v.get("nan_in"):
        x = np.where(u(shape) < 0.03, np.nan, x)
    return x.astype(np.float32)


def _prediction(g, v, shape):
    """The model's normalised output for one variable: p = lo + (hi - lo) u in the transformed space, y = (p - mean) / std."""
    tag = _tag(v)
    lo, hi = (-0.02 * _P_HI[tag], _P_HI[tag]) if v["xf"] else _P_RANGE[v["gen"]]
    p = lo + (hi - lo) * g.random(shape)
    m, s = variable_stats(v)
    if m is not None:
        p = (p - m.astype(np.float64).reshape(1, -1, 1, 1, 1)) / s.astype(np.float64).reshape(1, -1, 1, 1, 1)
    if v.get("nan_y"):
        p = np.where(g.random(shape) < 0.004, np.nan, p)
    return p.astype(np.float32)


def out_variables(name):
    """The predicted variables in y_pred channel order (prognostic 3d, prognostic 2d, diagnostic: the target channel map)."""
    vs = [v for v in XFORM_CASES[name]["variables"] if v["out"]]
    rank = lambda v: (0 if "/prognostic/" in v["key"] else 1, 0 if "/3d/" in v["key"] else 1)   # noqa: E731
    return sorted(vs, key=rank)


def target_channel_map(name):
    T, cmap, cur = XFORM_CASES[name]["T"], {}, 0
    for v in out_variables(name):
        cmap[v["key"]] = {"slice": slice(cur, cur + v["levels"] * T), "orig_shape": (v["levels"], T)}
        cur += v["levels"] * T
    return cmap


def case_inputs(name, check=None):
    """-> (fields {key: float32 [B, n_levels, T, H, W]} physical inputs, y_pred float32 [B, C_out, T, H, W] normalised model output)."""
    c = XFORM_CASES[name]
    H, W = GRIDS[c["grid"]]
    g = np.random.Generator(np.random.Philox(key=[2025, sorted(XFORM_CASES).index(name)]))
    fields = {v["key"]: _field(g, v, (c["B"], v["levels"], c["T"], H, W)) for v in c["variables"]}
    y_pred = np.concatenate([_prediction(g, v, (c["B"], v["levels"], c["T"], H, W)) for v in out_variables(name)], axis=1)
    if check is not None:
        for v in c["variables"]:
            assert input_digest(fields[v["key"]]) == str(check[f"sha256:in:{v['name']}"]), f"{name}: regenerated input {v['name']} differs from the fixture's"
        assert input_digest(y_pred) == str(check["sha256:y_pred"]), f"{name}: regenerated y_pred differs from the fixture's"
    return fields, y_pred


def batch_input(name, fields, wrap=lambda a: a):
    """{source: {key: tensor}} in the case's variable order."""
    return {SRC: {v["key"]: wrap(fields[v["key"]]) for v in XFORM_CASES[name]["variables"]}}


def input_digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def pre_blocks(name, mod):
    """The case's pre chain as blocks of `mod` (wxengine.transforms, or a namespace of the reference's classes): every variable's
    FillValues blocks in stacking order, then its log / sqrt."""
    blocks = []
    for v in XFORM_CASES[name]["variables"]:
        for rules in v["fills"]:
            blocks.append(mod.FillValues(rules=rules, variables=[v["key"]], data_types=["input"]))
    for v in XFORM_CASES[name]["variables"]:
        if v["xf"] and v["xf"][0] == "log":
            blocks.append(mod.LogTransform(variables=[v["key"]], data_types=["input"], base=v["xf"][1], eps=v["xf"][2]))
        elif v["xf"]:
            blocks.append(mod.SqrtTransform(variables=[v["key"]], data_types=["input"]))
    return blocks


def post_blocks(name, mod):
    blocks = []
    for v in out_variables(name):
        if v["xf"] and v["xf"][0] == "log":
            blocks.append(mod.ExpTransform(variables=[v["key"]], base=v["xf"][1], eps=v["xf"][2]))
        elif v["xf"]:
            blocks.append(mod.SquareTransform(variables=[v["key"]]))
    return blocks


def level_distance(a, b):
    """The fixtures' and the gate's distance per level: max |a - b| / max |b| over the positions where neither is NaN -> [n_levels].
    Where the two disagree on a NaN position the distance is inf."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.zeros(a.shape[1])
    for l in range(a.shape[1]):
        al, bl = a[:, l], b[:, l]
        if not np.array_equal(np.isnan(al), np.isnan(bl)):
            out[l] = np.inf
            continue
        ok = ~np.isnan(bl)
        out[l] = np.abs(al[ok] - bl[ok]).max() / np.abs(bl[ok]).max()
    return out


def load_golden(name, gold_dir):
    """-> (fixture, f32, f64, d_ref): dicts keyed "pre:<var>" / "post:<var>"; d_ref[...] is a [n_levels] array.  The fp64 golden is
    stored as its float32 difference from the fp32 golden (xform_<case>_f64.npz)."""
    import os
    g = np.load(os.path.join(gold_dir, f"xform_{name}.npz"))
    g64 = np.load(os.path.join(gold_dir, f"xform_{name}_f64.npz"))
    names = [f"pre:{v['name']}" for v in XFORM_CASES[name]["variables"]] + [f"post:{v['name']}" for v in out_variables(name)]
    f32 = {n: g[f"f32:{n}"] for n in names}
    f64 = {n: f32[n].astype(np.float64) + g64[f"d64:{n}"].astype(np.float64) for n in names}
    d_ref = {n: np.atleast_1d(g[f"d_ref:{n}"]).astype(np.float64) for n in names}
    return g, f32, f64, d_ref
