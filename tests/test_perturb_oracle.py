"""The dense-DFT restatement (tests/perturb_oracle.py) against the fixtures of the colour filter: it reproduces the reference's own
float64 evaluation to 1e-12 of its largest value on every case, with no fft call -- so the conventions the device follows (half-complex
bins counted once or twice, the ignored imaginary parts, the 1 / (H W) scale) are pinned on the CPU.  The fixtures are consistent."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import perturb_cases as PC  # noqa: E402
import perturb_oracle as PO  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name,red", PC.FILTER_RUNS)
def test_restatement_reproduces_ref64(name, red):
    g = PC.load_golden(name, GOLD)
    ref64 = g[f"ref64_r{red}"]
    got = PO.colour_filter(PC.tape(name), g[f"S_r{red}"])
    assert got.shape == ref64.shape and ref64.dtype == np.float64
    assert float(np.abs(got - ref64).max()) <= 1e-12 * float(np.abs(ref64).max())


@pytest.mark.parametrize("name,red", PC.FILTER_RUNS)
def test_fixture_is_consistent_and_leaves_the_device_room(name, red):
    g = PC.load_golden(name, GOLD)
    C, T, H, W = PC.PERTURB_CASES[name]["shape"]
    S, r32, r64 = g[f"S_r{red}"], g[f"ref32_r{red}"], g[f"ref64_r{red}"]
    assert S.dtype == np.float32 and S.shape == (H, W // 2 + 1) and S[0, 0] == 0 and np.isfinite(S).all()
    assert abs(float(np.sqrt(np.mean(S.astype(np.float64) ** 2))) - 1.0) < 1e-6          # unit RMS
    assert r32.dtype == np.float32 and r32.shape == r64.shape == (1, C, T, H, W)
    e_ref = float(np.abs(r32.astype(np.float64) - r64).max())
    assert e_ref == float(g[f"E_ref_r{red}"]) and "tape" not in g and "white" not in g     # the key, never the draws
    assert e_ref >= 2 * float(np.spacing(np.float32(np.abs(r64).max()))) / 2                # at least 2x room over half an ulp
    assert float(np.abs(r64.sum(axis=(-2, -1))).max()) <= 1e-10                             # DC removed


def test_reddening_0_is_the_closed_form():
    g = PC.load_golden("g37x72", GOLD)
    S = g["S_r0"]
    assert len(np.unique(S.reshape(-1)[1:])) == 1
    want = PO.white_closed_form(PC.tape("g37x72"))
    assert float(np.abs(want - g["ref64_r0"]).max()) <= 1e-6 * 1.0     # S is the float32 rounding of the constant
    assert float(np.abs(PO.colour_filter(PC.tape("g37x72"), np.full_like(S, 1.0).astype(np.float64) * (S.astype(np.float64) > 0) /
                                          np.sqrt(1.0 - 1.0 / S.size)) - want).max()) <= 1e-12 * float(np.abs(want).max())


def test_batch_formula_and_case_table():
    assert PC.batch_planes(721, 1440) == 16 and PC.batch_planes(19, 37) == 64 and PC.batch_planes(4096, 4096) == 1
    assert PC.PERTURB_CASES["many19x37"]["shape"][0] == 65
    assert PC.TEMPORAL["case"] in PC.PERTURB_CASES
