"""Weights and inputs of the regridding fixtures (tests/golden/regrid_<case>.npz, tools/make_goldens.py --only regrid), shared by the
generator, the CPU tests and the GPU tests.

The weights are built here with numpy in the form an ESMF weights file holds them: `row` / `col` 1-based int32, `S` float64, `n_a`,
`n_b`, `dst_grid_dims` and the destination centres `xc_b` / `yc_b`.  The inputs are not stored: they are rebuilt from the keyed Philox
stream with +, -, * and comparisons only (IEEE-exact, so every machine gets the same bits); the fixture stores their SHA-256 and
`case_inputs(..., check=fixture)` compares.

A case = one weight set, its variables (leading shapes in front of the source grid) and its runs (flip_axis, flat or 2-D input):
  block   12 x 20 -> 6 x 10, 2 x 2 average, entries stored in shuffled order, dst_grid_dims = [10, 6]; every leading shape
  bilin   9 x 16 -> 13 x 23 bilinear, periodic in longitude, pole rows; zero weights dropped (1 .. 4 entries per row, the columns of
          one row far apart: i and i + 1, and 15 and 0 across the date line); the flips and the flat input
  cons    33 x 67 -> 7 x 11 conservative: the outer product of 1-D overlap fractions of non-aligned cells, 20 .. 60 entries per row,
          varying inside a slice of 64 rows
  ragged  2 211 flat source points -> 301 flat destination points (four full slices and a partial one, two workgroups of 256),
          reshape_to_xy = False: rows of 0, 1, 63, 64, 65, 200 and 700 entries and random lengths 1 .. 40, repeated (row, col) pairs,
          weights of mixed sign in a third of the rows
  uniq    6 x 10 -> 4 x 5 with a length-1 dst_grid_dims: the shape comes from the unique xc_b / yc_b; a rectilinear and a curvilinear
          coordinate set
  nan     `block` with NaNs at scattered source points (SST over land)"""
import hashlib
import os

import numpy as np

SRC = "GFS"
LONG_ROW = 64            # kRegridLongRow
SLICE = 64


def key_of(v):
    return f"{SRC}/prognostic/2d/{v}"


PLAIN = {"plain": dict(flip_axis=None, flat=False)}
REGRID_CASES = {
    "block": dict(src=(12, 20), dst=(6, 10), vars={"hw": (), "l111": (1, 1, 1), "l232": (2, 3, 2), "l7": (7,), "b2": (2, 3)}, runs=PLAIN),
    "bilin": dict(src=(9, 16), dst=(13, 23), vars={"a": (3,)},
                  runs={"plain": dict(flip_axis=None, flat=False), "flip-1": dict(flip_axis=[-1], flat=False),
                        "flip-2": dict(flip_axis=[-2], flat=False), "flip-1-2": dict(flip_axis=[-1, -2], flat=False),
                        "flip2": dict(flip_axis=[2], flat=False), "flat": dict(flip_axis=None, flat=True),
                        "flatflip-2": dict(flip_axis=[-2], flat=True)}),
    "cons": dict(src=(33, 67), dst=(7, 11), vars={"a": (2,)}, runs=PLAIN),
    "ragged": dict(src=(2211,), dst=(301,), vars={"a": (5,)}, runs={"plain": dict(flip_axis=None, flat=True)}, reshape_to_xy=False),
    "uniq": dict(src=(6, 10), dst=(4, 5), vars={"a": (2,)}, runs=PLAIN),
    "nan": dict(src=(12, 20), dst=(6, 10), vars={"sst": (3,)}, runs=PLAIN, nan=True),
}
RAGGED_ROWS = {3: 0, 5: 1, 64: 63, 70: 64, 71: 65, 130: 200, 200: 700, 299: 0, 300: 65}     # destination row -> coalesced entries


def _stream(name, what):
    return np.random.Generator(np.random.Philox(key=[2028, 100 * sorted(REGRID_CASES).index(name) + what]))


def _centres(n, lo, hi):
    e = np.linspace(lo, hi, n + 1)
    return 0.5 * (e[:-1] + e[1:])


def _overlap(n_src, n_dst):
    """[n_dst, n_src] fraction of destination cell d that source cell s covers, both sets of cells uniform on [0, 1]."""
    es, ed = np.arange(n_src + 1) / n_src, np.arange(n_dst + 1) / n_dst
    lo = np.maximum(es[None, :-1], ed[:-1, None])
    hi = np.minimum(es[None, 1:], ed[1:, None])
    return np.clip(hi - lo, 0.0, None) * n_dst


def weights(name):
    """-> dict(row, col, S, n_a, n_b, dst_grid_dims, xc_b, yc_b[, xc_b_curv, yc_b_curv]): the arrays of the case's weights file."""
    c = REGRID_CASES[name]
    g = _stream(name, 1)
    n_a, n_b = int(np.prod(c["src"])), int(np.prod(c["dst"]))
    if name in ("block", "nan"):
        (H, W), (h, w) = c["src"], c["dst"]
        i, j, di, dj = np.meshgrid(np.arange(h), np.arange(w), np.arange(2), np.arange(2), indexing="ij")
        row = (i * w + j).ravel()
        col = ((2 * i + di) * W + 2 * j + dj).ravel()
        S = np.full(row.size, 0.25)
        lat, lon = _centres(h, -90.0, 90.0), _centres(w, 0.0, 360.0)
    elif name == "bilin":
        (H, W), (h, w) = c["src"], c["dst"]
        lat, lon = np.linspace(-90.0, 90.0, h), np.arange(w) * (360.0 / w)
        dlat, dlon = 180.0 / (H - 1), 360.0 / W
        row, col, S = [], [], []
        for i in range(h):
            i0 = min(int((lat[i] + 90.0) // dlat), H - 2)
            t = (lat[i] + 90.0 - i0 * dlat) / dlat
            for j in range(w):
                j0 = int(lon[j] // dlon)
                s = (lon[j] - j0 * dlon) / dlon
                for ii, jj, wt in ((i0, j0, (1 - t) * (1 - s)), (i0, (j0 + 1) % W, (1 - t) * s), (i0 + 1, j0, t * (1 - s)),
                                   (i0 + 1, (j0 + 1) % W, t * s)):
                    if wt != 0.0:
                        row.append(i * w + j)
                        col.append(ii * W + jj)
                        S.append(wt)
        row, col, S = np.array(row), np.array(col), np.array(S)
    elif name == "cons":
        (H, W), (h, w) = c["src"], c["dst"]
        fy, fx = _overlap(H, h), _overlap(W, w)                      # [h, H], [w, W]
        full = (fy[:, None, :, None] * fx[None, :, None, :]).reshape(h * w, H * W)
        row, col = np.nonzero(full)
        S = full[row, col]
        lat, lon = _centres(h, -90.0, 90.0), _centres(w, 0.0, 360.0)
    elif name == "ragged":
        row, col, S = [], [], []
        for r in range(n_b):
            n = RAGGED_ROWS.get(r, int(g.integers(1, 41)))
            cols = g.choice(n_a, size=n, replace=False)
            wt = 0.1 + g.random(n)
            if r % 3 == 0:
                wt = wt * np.where(g.random(n) < 0.5, -1.0, 1.0)
            n_dup = min(n, 1 + n // 8) if r % 2 == 0 else 0           # repeated (row, col) pairs with weights of their own
            cols = np.concatenate([cols, cols[:n_dup]])
            wt = np.concatenate([wt, 0.05 * g.random(n_dup)])
            row.append(np.full(cols.size, r))
            col.append(cols)
            S.append(wt)
        row, col, S = np.concatenate(row), np.concatenate(col), np.concatenate(S)
        lat, lon = None, None
    elif name == "uniq":
        (H, W), (h, w) = c["src"], c["dst"]
        i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        row = np.concatenate([(i * w + j).ravel()] * 2)
        col = np.concatenate([(i * W + 2 * j).ravel(), ((i + 2) * W + 2 * j + 1).ravel()])
        S = np.concatenate([np.full(h * w, 0.75), np.full(h * w, 0.25)])
        lat, lon = _centres(h, -60.0, 60.0), _centres(w, 0.0, 360.0)
    else:
        raise KeyError(name)
    order = g.permutation(row.size)                                   # a weights file promises no order
    out = dict(row=(row[order] + 1).astype(np.int32), col=(col[order] + 1).astype(np.int32), S=S[order].astype(np.float64), n_a=n_a, n_b=n_b)
    if name == "ragged":
        out.update(dst_grid_dims=np.array([n_b], dtype=np.int32), xc_b=360.0 * g.random(n_b), yc_b=180.0 * g.random(n_b) - 90.0)
    else:
        h, w = c["dst"]
        out.update(dst_grid_dims=np.array([h * w] if name == "uniq" else [w, h], dtype=np.int32),
                   xc_b=np.tile(lon, h).astype(np.float64), yc_b=np.repeat(lat, w).astype(np.float64))
        if name == "uniq":      # the same values, shifted by one column per row: still w unique longitudes, no longer separable
            out.update(xc_b_curv=np.stack([np.roll(lon, -i) for i in range(h)]).ravel(), yc_b_curv=out["yc_b"].copy())
    return out


def variables(name):
    return tuple(REGRID_CASES[name]["vars"])


def block_args(name, run="plain", curvilinear=False):
    """The keyword arguments of wxengine.regrid.Regridder for a run of a case."""
    c, w = REGRID_CASES[name], weights(name)
    xc, yc = (w["xc_b_curv"], w["yc_b_curv"]) if curvilinear else (w["xc_b"], w["yc_b"])
    return dict(variables=[key_of(v) for v in variables(name)], row=w["row"], col=w["col"], S=w["S"], n_a=w["n_a"], n_b=w["n_b"],
                dst_grid_dims=w["dst_grid_dims"], xc_b=xc, yc_b=yc, reshape_to_xy=c.get("reshape_to_xy", True),
                flip_axis=c["runs"][run]["flip_axis"])


def reference_args(name, run="plain", curvilinear=False):
    """-> (keyword arguments of the reference's Regridder, arrays its weights file holds, the file's dimension sizes)."""
    c, w = REGRID_CASES[name], weights(name)
    xc, yc = (w["xc_b_curv"], w["yc_b_curv"]) if curvilinear else (w["xc_b"], w["yc_b"])
    arrays = dict(row=w["row"], col=w["col"], S=w["S"], dst_grid_dims=w["dst_grid_dims"], xc_b=xc, yc_b=yc)
    kw = dict(weight_file="weights.nc", variables=[key_of(v) for v in variables(name)], reshape_to_xy=c.get("reshape_to_xy", True),
              flip_axis=c["runs"][run]["flip_axis"])
    return kw, arrays, dict(n_a=w["n_a"], n_b=w["n_b"], n_s=w["row"].size)


def case_inputs(name, check=None):
    """-> {variable: float32 [*lead, *source shape]}.  `check`: an opened fixture whose sha256 entries must match."""
    c = REGRID_CASES[name]
    g = _stream(name, 2)
    out = {}
    for v, lead in c["vars"].items():
        shape = tuple(lead) + tuple(c["src"])
        x = 250.0 + 80.0 * g.random(shape) - 40.0 * (g.random(shape) < 0.25)      # 210 .. 330, a quarter of the points 40 lower
        if name == "ragged":
            x = x - 270.0                                                          # both signs
        x = x.astype(np.float32)
        if c.get("nan"):
            x[g.random(shape) < 0.08] = np.nan
        out[v] = x
    if check is not None:
        for v in out:
            assert input_digest(out[v]) == str(check[f"sha256:{v}"]), f"{name}: regenerated input {v} differs from the fixture's"
    return out


def run_input(name, run, x):
    """The tensor a run feeds: the 2-D source flattened for a flat run."""
    c = REGRID_CASES[name]
    if c["runs"][run]["flat"] and len(c["src"]) == 2:
        return x.reshape(x.shape[:-2] + (-1,))
    return x


def out_shape(name, lead):
    c = REGRID_CASES[name]
    return tuple(lead) + (tuple(c["dst"]) if c.get("reshape_to_xy", True) else (int(np.prod(c["dst"])),))


def input_digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def row_lengths(name):
    """-> (stored entries per destination row, coalesced entries per destination row)."""
    w = weights(name)
    r, cidx = w["row"].astype(np.int64) - 1, w["col"].astype(np.int64) - 1
    stored = np.bincount(r, minlength=w["n_b"])
    uniq = np.unique(r * w["n_a"] + cidx)
    return stored, np.bincount(uniq // w["n_a"], minlength=w["n_b"])


def check_conditions(name, inp):
    """What a case is there for, asserted on its weights and regenerated inputs.  -> a one-line summary."""
    c, w = REGRID_CASES[name], weights(name)
    stored, coal = row_lengths(name)
    r = w["row"].astype(np.int64)
    assert (np.diff(r) < 0).any(), f"{name}: the entries are stored in sorted order"
    note = ""
    if name in ("block", "nan"):
        assert (coal == 4).all() and list(w["dst_grid_dims"]) == [10, 6]
    if name == "bilin":
        assert coal.min() == 1 and coal.max() == 4, (coal.min(), coal.max())
        cz = w["col"].astype(np.int64) - 1
        spread = np.array([np.ptp(cz[r - 1 == k]) for k in range(w["n_b"])])
        assert spread.max() >= c["src"][1] and (spread[coal == 4] >= c["src"][1]).all(), "the columns of one row do not lie far apart"
        assert np.abs(np.bincount(r - 1, weights=w["S"]) - 1.0).max() < 1e-12
    if name == "cons":
        assert coal.min() >= 20 and coal.max() <= 60 and coal.max() <= LONG_ROW, (coal.min(), coal.max())
        assert all(np.unique(coal[s:s + SLICE]).size > 1 for s in range(0, coal.size, SLICE)), "row lengths do not vary inside a slice"
        assert np.abs(np.bincount(r - 1, weights=w["S"]) - 1.0).max() < 1e-12
    if name == "ragged":
        assert all(coal[k] == n for k, n in RAGGED_ROWS.items()), [(k, coal[k]) for k in RAGGED_ROWS]
        others = np.delete(coal, list(RAGGED_ROWS))
        assert others.min() >= 1 and others.max() <= 40
        assert (stored > coal).sum() > 100 and stored.max() > coal.max(), "no repeated (row, col) pairs"
        signs = np.array([(w["S"][r - 1 == k] < 0).any() and (w["S"][r - 1 == k] > 0).any() for k in range(w["n_b"])])
        assert 0.25 < signs.mean() < 0.4, signs.mean()
        assert w["n_b"] == 301 and w["n_b"] > 4 * SLICE and w["n_b"] > 256 and w["n_b"] % SLICE
        assert (inp["a"] > 0).any() and (inp["a"] < 0).any()
        note = f", {int((coal > LONG_ROW).sum())} long rows, {int((coal == 0).sum())} empty rows, {int((stored - coal).sum())} repeated pairs"
    if name == "uniq":
        assert len(w["dst_grid_dims"]) == 1
        assert (np.unique(w["yc_b"]).size, np.unique(w["xc_b"]).size) == c["dst"]
        assert (np.unique(w["yc_b_curv"]).size, np.unique(w["xc_b_curv"]).size) == c["dst"]
    if c.get("nan"):
        for v, x in inp.items():
            bad = np.isnan(x)
            assert bad.reshape(-1, w["n_a"]).any(axis=1).all() and 0.02 < bad.mean() < 0.2, (name, v)
    else:
        assert all(np.isfinite(x).all() for x in inp.values())
    return f"{w['n_a']} -> {w['n_b']} points, {w['row'].size} stored entries, {coal.min()} .. {coal.max()} per row{note}"


def bound(k, mag):
    """The per-element gate of a float32 result against the float64 one: (k[r] + 2) 2^-24 mag[p, r], the running-error bound of a
    length-k float32 sum in any order, the roundings of the products and of the merged repeated pairs included (each term is rounded
    at most once as a product or a merged weight, once more as a product of the merged weight, and takes part in at most k - 1
    additions of partial sums none of which exceeds mag (1 + k 2^-24))."""
    return (k.astype(np.float64) + 2.0) * 2.0 ** -24 * mag


def load_golden(name, gold_dir):
    """-> (fixture, {(run, var): fp32 golden}, {(run, var): fp64 golden})."""
    g = np.load(os.path.join(gold_dir, f"regrid_{name}.npz"))
    g64 = np.load(os.path.join(gold_dir, f"regrid_{name}_f64.npz"))
    keys = [(run, v) for run in REGRID_CASES[name]["runs"] for v in variables(name)]
    return g, {k: g[f"f32:{k[0]}:{k[1]}"] for k in keys}, {k: g64[f"f64:{k[0]}:{k[1]}"] for k in keys}
