"""The restatement of the verification metrics (tests/metrics_oracle.py) against the reference's goldens (tests/golden/metrics_*.npz,
tools/make_goldens.py --only metrics), no GPU and no reference tree needed: the regenerated inputs carry the fixture's hashes, the
float32 restatement reproduces the reference's forward to float32 rounding of each score (it restates its operations), the float64
restatement reproduces the stored yardstick, the keys come in the reference's order, and on the pressure field of sp2d a careless
float32 raw-moment evaluation misses the gate, with sequential and with pairwise summation."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import metrics_cases as MC  # noqa: E402
import metrics_oracle as MO  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("case", list(MC.METRICS_CASES))
def test_restatement_reproduces_the_goldens(case):
    c = MC.METRICS_CASES[case]
    g, keys, f32, f64, d_ref, scale = MC.load_golden(case, GOLD)
    inp = MC.case_inputs(c["inputs"], check=g)
    m32 = MO.Restatement(dtype=torch.float32, **MC.block_args(case, inp))
    m64 = MO.Restatement(dtype=torch.float64, **MC.block_args(case, inp))
    assert f32.shape == (MC.INPUTS[c["inputs"]]["calls"], len(keys))
    for call in range(f32.shape[0]):
        o32 = m32(MC.state_dicts(inp, call, torch.from_numpy))
        o64 = m64(MC.state_dicts(inp, call, lambda a: torch.from_numpy(a).double()), all_scores=True)
        assert list(o32) == keys and list(o64) == keys, case
        sc = MC.scales(m64.last_all_scores, m64.weights, m64.var_keys)
        for i, k in enumerate(keys):
            assert all(isinstance(o[k], float) for o in (o32, o64))
            # the same operations as the reference's: float32 rounding of the score itself, no more (1e-6 of its magnitude)
            assert abs(o32[k] - f32[call, i]) <= 1e-6 * max(abs(f32[call, i]), scale[call, i] if np.isfinite(scale[call, i]) else 0.0), (case, call, k)
            assert abs(o64[k] - f64[call, i]) <= 1e-12 * max(1.0, abs(f64[call, i])), (case, call, k)
            assert sc[k] == pytest.approx(scale[call, i], rel=1e-12), (case, call, k)
            assert MC.distance(f32[call, i], f64[call, i], scale[call, i]) == d_ref[call, i]


def test_key_order_is_per_metric_every_variable_then_the_aggregate():
    g, keys, *_ = MC.load_golden("lev16_basic", GOLD)
    vs = sorted(MC.KEYS[v] for v in ("T", "U", "sp"))
    assert keys == [k for m in ("rmse", "mae", "bias") for k in [f"{m}/{v}" for v in vs] + [m]]


def test_float32_raw_moments_miss_the_gate_on_the_pressure_field():
    g, keys, f32, f64, d_ref, scale = MC.load_golden("sp2d", GOLD)
    inp = MC.case_inputs("sp2d", check=g)
    p, t = inp["pred"][0]["sp"], inp["target"][0]["sp"]
    cl = np.broadcast_to(inp["clim"]["sp"], p.shape)
    w = np.broadcast_to(MO.lat_weights(inp["lat"]).numpy().reshape(1, 1, 1, -1, 1), p.shape)
    for pairwise in (False, True):
        raw = MC.raw_moments(p, t, cl, w, pairwise)
        for m in ("r2score", "log_variance_ratio", "acc"):
            i = keys.index(f"{m}/{MC.KEYS['sp']}")
            assert MC.distance(raw[m], f64[0, i], 1.0) > MC.gate(d_ref[0, i])[1], (m, pairwise)


def test_degenerate_inputs_use_every_epsilon():
    """prediction == target: r2score 1, log variance ratio 0, errors 0; a constant target: the +1e-12 is most of the denominator of
    r2score, eps most of the argument of the target's log, and all scores are finite."""
    g, keys, f32, f64, *_ = MC.load_golden("degenerate", GOLD)
    val = dict(zip(keys, f64[0]))
    same, const = MC.KEYS["same"], MC.KEYS["const"]
    assert val[f"rmse/{same}"] == 0.0 and val[f"mae/{same}"] == 0.0 and val[f"r2score/{same}"] == 1.0 and val[f"log_variance_ratio/{same}"] == 0.0
    assert abs(val[f"acc/{same}"] - 1.0) < 1e-9
    # the float32 weights have mean 1 only to float32 rounding, so w t keeps a variance of some 1e-13: the 1e-12 is most of the denominator
    assert 1.0 - val[f"mse/{const}"] / 1e-12 < val[f"r2score/{const}"] < 1.0 - val[f"mse/{const}"] / 2e-12
    assert np.isfinite(f32).all() and np.isfinite(f64).all()
