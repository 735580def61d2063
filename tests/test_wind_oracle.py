"""tests/wind_oracle.py (the torch restatement of csrc/wx_wind.h) against the reference's goldens (tests/golden/wind_*.npz, written by
tools/make_goldens.py --only wind): in fp32 within the gate of the fp32 golden, in fp64 within it of the fp64 golden, for every case,
the blend mask and every filtered plane.  Needs neither a GPU nor the reference."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import wind_oracle as O  # noqa: E402
from diag_cases import distance, gate  # noqa: E402
from wind_cases import KEYS, WIND_CASES, case_inputs, filtered_planes, load_golden, output_names  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def run_oracle(name, inp, dtype):
    c = WIND_CASES[name]
    out, m = O.wind_filter({KEYS[v]: torch.from_numpy(inp[v]) for v in inp}, KEYS["U"], KEYS["V"], [KEYS[v] for v in c["targets"]], c["args"], dtype)
    res = {v: filtered_planes(name, v, out[KEYS[v]]).numpy() for v in c["targets"]}
    res["mask"] = m.numpy()
    return out, res


@pytest.mark.parametrize("name", list(WIND_CASES))
def test_oracle_vs_reference_goldens(name):
    g, f32, f64, d_ref = load_golden(name, GOLD)
    inp = case_inputs(name, check=g)
    _, r32 = run_oracle(name, inp, torch.float32)
    _, r64 = run_oracle(name, inp, torch.float64)
    for v in output_names(name):
        assert r32[v].shape == f32[v].shape and r32[v].dtype == np.float32 and r64[v].dtype == np.float64, (name, v)
        if name == "calm":     # nothing flagged: the mask is exactly 0 and the planes are the inputs
            assert np.array_equal(r32[v], f32[v]) and np.array_equal(r64[v], f64[v]), (name, v)
            continue
        b32, b64 = gate(d_ref[v])
        d32, d64 = distance(r32[v], f32[v]), distance(r64[v], f64[v])
        print(f"[wind oracle] {name} {v}: d_ref {d_ref[v]:.2e}; fp32 vs fp32 golden {d32:.2e} (<= {b32:.2e}), fp64 vs fp64 golden {d64:.2e} (<= {b64:.2e})")
        assert d32 <= b32 and d64 <= b64, (name, v, d32, b32, d64, b64)


def test_oracle_leaves_the_other_levels_alone_and_skips_missing_ones():
    inp = case_inputs("cam48")
    out, _ = run_oracle("cam48", inp, torch.float32)
    for v in WIND_CASES["cam48"]["targets"]:
        assert out[KEYS[v]].shape == inp[v].shape            # level 7 of target_levels does not exist: skipped
        for l in (0, 4):
            assert np.array_equal(out[KEYS[v]][:, l].numpy(), inp[v][:, l])
        assert not np.array_equal(out[KEYS[v]][:, 2].numpy(), inp[v][:, 2])


def test_the_stripe_plane_engages_the_alpha_clamp():
    """cam48, level 3 of T: a 2-dx stripe the smoothing all but removes, so the unclamped amplitude factor is far above 4."""
    inp = case_inputs("cam48")
    c = WIND_CASES["cam48"]
    t = {k: torch.from_numpy(v).double() for k, v in inp.items()}
    m = O.blend_mask(t["U"][:, 2, 0], t["V"][:, 2, 0], c["args"])
    g2d = O.smoothing_kernel(c["args"], torch.float64)
    for l, lo, hi in ((3, 20.0, 200.0), (1, 1.0, 2.0)):
        f = t["T"][:, l]
        fs = O.conv_zero_pad(f, g2d)
        alpha = float(torch.sqrt((m * f * f).sum() / ((m * fs * fs).sum() + 1e-12)))
        assert lo < alpha < hi, (l, alpha)
