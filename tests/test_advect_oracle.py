"""tests/advect_oracle.py (the torch restatement of csrc/wx_advect.h) against the reference's goldens (tests/golden/advect_*.npz,
written by tools/make_goldens.py --only advect): in fp32 within the gate of the fp32 golden, in fp64 within it of the fp64 golden, for
every case, every tracer and both row regions (tests/advect_cases.py: gate = max(4 d_ref, 2e-6) / max(5 d_ref, 2e-6), d_ref per
tracer AND region), and the properties the index-space sampling is built for.  Needs neither a GPU nor the reference."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import advect_oracle as AO  # noqa: E402
from advect_cases import (ADVECT_CASES, KEYS, REGIONS, case_inputs, gate, load_golden, oracle_args, region_distance,  # noqa: E402
                          region_rows)

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def fields_of(inp):
    return {KEYS[k]: torch.from_numpy(v) for k, v in inp.items()}


@pytest.mark.parametrize("name", list(ADVECT_CASES))
def test_oracle_vs_reference_goldens(name):
    g, f32, f64, d_ref = load_golden(name, GOLD)
    inp = case_inputs(name, check=g)
    rows = region_rows(ADVECT_CASES[name]["H"])
    o32 = AO.advect(fields_of(inp), dtype=torch.float32, **oracle_args(name))
    o64 = AO.advect(fields_of(inp), dtype=torch.float64, **oracle_args(name))
    bad = []
    for t in ADVECT_CASES[name]["tracers"]:
        r32, r64 = o32[KEYS[t]].numpy(), o64[KEYS[t]].numpy()
        assert r32.shape == f32[t].shape == inp[t].shape and r32.dtype == np.float32 and r64.dtype == np.float64, (name, t)
        for r in REGIONS:
            b32, b64 = gate(d_ref[(t, r)])
            d32, d64 = region_distance(r32, f32[t], rows[r]), region_distance(r64, f64[t], rows[r])
            print(f"[advect oracle] {name} {t} {r}: d_ref {d_ref[(t, r)]:.2e}; fp32 vs fp32 golden {d32:.2e} (<= {b32:.2e}), "
                  f"fp64 vs fp64 golden {d64:.2e} (<= {b64:.2e})")
            if not (d32 <= b32 and d64 <= b64):
                bad.append((t, r, d32, b32, d64, b64))
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", ["base36", "b2s2t", "gauss"])
def test_zero_winds_return_the_input_bit_for_bit(name):
    inp = case_inputs(name)
    inp["U"], inp["V"] = np.zeros_like(inp["U"]), np.zeros_like(inp["V"])
    out = AO.advect(fields_of(inp), dtype=torch.float32, **oracle_args(name))
    for t in ADVECT_CASES[name]["tracers"]:
        assert np.array_equal(out[KEYS[t]].numpy(), inp[t]), (name, t)


@pytest.mark.parametrize("name", ["base36", "gauss"])
def test_a_zonally_uniform_state_stays_zonally_uniform(name):
    """Every column the same: the divergence has no zonal part, every column of a row departs from the same row and level, and the
    column lerp of two equal neighbours returns their bits -- whatever the column displacement."""
    inp = {k: np.ascontiguousarray(np.broadcast_to(v[..., 3:4], v.shape)) for k, v in case_inputs(name).items()}
    out = AO.advect(fields_of(inp), dtype=torch.float32, **oracle_args(name))
    for t in ADVECT_CASES[name]["tracers"]:
        o = out[KEYS[t]].numpy()
        assert np.array_equal(o, np.broadcast_to(o[..., :1], o.shape)), (name, t)
        assert not np.array_equal(o, inp[t]), (name, t)        # the meridional and vertical motion are still there


def test_surface_to_top_equals_the_flipped_top_to_surface_run():
    inp = case_inputs("b2s2t")
    args = oracle_args("b2s2t")
    assert args["level_order"] == "surface_to_top"
    s2t = AO.advect(fields_of(inp), dtype=torch.float32, **args)
    flipped = {k: (v if k == "sp" else np.ascontiguousarray(v[:, ::-1])) for k, v in inp.items()}
    t2s = AO.advect(fields_of(flipped), dtype=torch.float32, **dict(args, level_order="top_to_surface"))
    for t in ADVECT_CASES["b2s2t"]["tracers"]:
        assert torch.equal(s2t[KEYS[t]], t2s[KEYS[t]].flip(1)), t
        assert not torch.equal(s2t[KEYS[t]], t2s[KEYS[t]]), t


def test_the_cases_take_the_wrap_the_clamps_and_many_revolutions():
    """What the mutations of the sampling rule need: interior departure columns outside [0, W), departure rows outside [0, H - 1] and
    departure levels outside [0, L - 1] in every case, and in `polewind` displacements of more than one revolution (a single add of W
    does not bring them back)."""
    for name, c in ADVECT_CASES.items():
        _, (col, row, lev) = AO.advect(fields_of(case_inputs(name)), dtype=torch.float64, want_departure=True, **oracle_args(name))
        ri = region_rows(c["H"])["interior"]
        assert bool(((col[:, :, ri] < 0) | (col[:, :, ri] >= c["W"])).any()), name
        assert bool(((row < 0) | (row > c["H"] - 1)).any()), name
        assert bool(((lev < 0) | (lev > c["L"] - 1)).any()), name
        if name == "polewind":
            assert float(col.abs().max()) > 3 * c["W"], float(col.abs().max())
