"""The wind-filter fixtures against the LIVE reference (credit/postblock/wind_filter.py); skipped where the reference tree is absent.
The regenerated inputs hash to the fixture's, the reference's class reproduces the stored fp32 goldens bit for bit and its two helpers
on double tensors the stored fp64 goldens (kept as float32 differences: to the rounding of that difference)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from wind_cases import KEYS, SRC, WIND_CASES, case_inputs, filtered_levels, load_golden  # noqa: E402

pytestmark = pytest.mark.reference
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", list(WIND_CASES))
def test_reference_reproduces_the_stored_goldens(name):
    import oracle_stub
    oracle_stub.install()
    import credit.postblock.wind_filter as RW
    c = WIND_CASES[name]
    a = c["args"]
    g, f32, f64, _ = load_golden(name, GOLD)
    inp = case_inputs(name, check=g)             # the hashes
    lv = filtered_levels(name)
    assert list(g["levels"]) == lv
    blk = RW.WindArtifactFilter(u_var=KEYS["U"], v_var=KEYS["V"], target_vars=[KEYS[v] for v in c["targets"]], **a)
    with torch.no_grad():
        y = blk({"y_processed": {SRC: {KEYS[v]: torch.from_numpy(inp[v]) for v in inp}}})["y_processed"][SRC]
        u, v = torch.from_numpy(inp["U"])[:, a["mask_level"], 0], torch.from_numpy(inp["V"])[:, a["mask_level"], 0]
        common = (a["speed_threshold"], a["dilation_zonal"], a["dilation_meridional"], a["falloff_sigma"], a["smooth_sigma"],
                  a["smooth_sigma_zonal"], a["smooth_sigma_meridional"])
        m32, _ = RW._compute_blend_mask(u, v, *common)
        m64, g64 = RW._compute_blend_mask(u.double(), v.double(), *common)
        assert np.array_equal(m32.numpy(), f32["mask"])
        assert np.abs(m64.numpy() - f64["mask"]).max() <= 1e-12
        for var in c["targets"]:
            assert np.array_equal(y[KEYS[var]][:, lv, 0].numpy(), f32[var]), (name, var)
            t = torch.from_numpy(inp[var]).double()
            r64 = torch.stack([RW._blend_smoothed(t[:, l], g64, m64, a["preserve_amplitude"])[:, 0] for l in lv], dim=1).numpy()
            assert np.abs(r64 - f64[var]).max() <= 1e-12 * max(1.0, np.abs(r64).max()), (name, var)
