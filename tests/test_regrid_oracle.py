"""The float64 restatement of the regridding block (tests/regrid_oracle.py) against the fixtures the reference's own class wrote
(tools/make_goldens.py --only regrid), and the fixtures against the conditions their cases are there for.  No GPU, no reference tree."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import regrid_oracle as RO  # noqa: E402
from regrid_cases import (REGRID_CASES, bound, case_inputs, check_conditions, load_golden, out_shape, run_input, variables,  # noqa: E402
                          weights)

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", list(REGRID_CASES))
def test_restatement_reproduces_the_goldens(name):
    c, w = REGRID_CASES[name], weights(name)
    g, f32, f64 = load_golden(name, GOLD)
    inp = case_inputs(name, check=g)
    check_conditions(name, inp)
    shape = RO.dst_shape(w["dst_grid_dims"], w["xc_b"], w["yc_b"], c.get("reshape_to_xy", True))
    assert shape == (tuple(c["dst"]) if len(c["dst"]) == 2 else None)
    n_checked = 0
    for run, r in c["runs"].items():
        for v in variables(name):
            y, mag, k = RO.regrid(run_input(name, run, inp[v]), w["row"], w["col"], w["S"], w["n_a"], w["n_b"], shape, r["flip_axis"])
            a32, a64 = f32[(run, v)], f64[(run, v)]
            assert a32.dtype == np.float32 and a64.dtype == np.float64
            assert y.shape == a32.shape == a64.shape == out_shape(name, c["vars"][v])
            bad = np.isnan(y)
            assert np.array_equal(bad, np.isnan(a64)) and np.array_equal(bad, np.isnan(a32)) and bad.any() == bool(c.get("nan"))
            assert not bad.all()
            ok = ~bad.reshape(-1, w["n_b"])
            y2, a64_2, a32_2 = (a.reshape(-1, w["n_b"]) for a in (y, a64, a32.astype(np.float64)))
            assert (np.abs(y2 - a64_2)[ok] <= 1e-14 * mag[ok]).all(), (name, run, v)
            assert (np.abs(a32_2 - a64_2)[ok] <= bound(k, mag)[ok]).all(), (name, run, v)       # the reference's own fp32 output
            assert (a32_2[:, k == 0] == 0).all() and (a64_2[:, k == 0] == 0).all()
            n_checked += int(ok.sum()) + int(bad.sum())
            assert int(ok.sum()) + int(bad.sum()) == y.size
    assert n_checked == sum(int(np.prod(out_shape(name, lead))) for lead in c["vars"].values()) * len(c["runs"])


def test_runs_that_must_agree_agree_in_the_goldens():
    """Flat input equals 2-D input, an ignored flip changes nothing, a kept flip does; `nan` without its NaNs is `block`."""
    _, f32, _ = load_golden("bilin", GOLD)
    plain = f32[("plain", "a")]
    for same in ("flip2", "flat", "flatflip-2"):
        assert np.array_equal(f32[(same, "a")], plain), same
    for other in ("flip-1", "flip-2", "flip-1-2"):
        assert not np.array_equal(f32[(other, "a")], plain), other
    inp = case_inputs("bilin")["a"]
    w = weights("bilin")
    for run, axes in (("flip-1", (-1,)), ("flip-2", (-2,)), ("flip-1-2", (-1, -2))):
        y, _, _ = RO.regrid(np.flip(inp, axis=axes), w["row"], w["col"], w["S"], w["n_a"], w["n_b"], (13, 23))
        y2, _, _ = RO.regrid(inp, w["row"], w["col"], w["S"], w["n_a"], w["n_b"], (13, 23), list(axes))
        assert np.array_equal(y, y2)


def test_destination_attributes_in_the_goldens():
    for name in REGRID_CASES:
        c, w = REGRID_CASES[name], weights(name)
        g, _, _ = load_golden(name, GOLD)
        shape = RO.dst_shape(w["dst_grid_dims"], w["xc_b"], w["yc_b"], c.get("reshape_to_xy", True))
        for tag in ("rect", "curv") if name == "uniq" else ("rect",):
            xc, yc = (w["xc_b_curv"], w["yc_b_curv"]) if tag == "curv" else (w["xc_b"], w["yc_b"])
            kind, lat, lon = RO.dst_grid(shape, xc, yc)
            assert str(g[f"grid_type:{tag}"]) == str(kind), (name, tag)
            if kind is not None:
                assert np.array_equal(g[f"dst_lat:{tag}"], lat) and np.array_equal(g[f"dst_lon:{tag}"], lon)
                assert lat.ndim == (1 if kind == "rectilinear" else 2)
        assert (str(g["grid_type:rect"]) == "None") == (name == "ragged")
    g, _, _ = load_golden("uniq", GOLD)
    assert str(g["grid_type:rect"]) == "rectilinear" and str(g["grid_type:curv"]) == "curvilinear"
