"""tests/xform_oracle.py (the torch restatement of the two transform kernels) against the goldens of tests/golden/xform_*.npz, which
tools/make_goldens.py --only xform wrote from the reference's own FillValues / LogTransform / SqrtTransform / ExpTransform /
SquareTransform in fp32 and fp64 (the scaler legs between them are the expressions pinned for DevicePreblock / InverseScale:
bridgescaler is not installed where the fixtures are made, so the reference's bridgescaler_transform itself could not be run).
Every value of every fixture is compared; the distance is max |a - b| / max |b| per variable AND level, NaN positions excluded and
required to coincide; the gate is the project's diag_cases.gate(d_ref)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import xform_oracle as O  # noqa: E402
from diag_cases import gate  # noqa: E402
from xform_cases import GRIDS, XFORM_CASES, case_inputs, level_distance, load_golden, out_variables  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in XFORM_CASES:
        g, f32, f64, d_ref = load_golden(name, GOLD)
        fields, y_pred = case_inputs(name, check=g)        # regenerated inputs match the fixtures' SHA-256
        out[name] = (fields, y_pred, f32, f64, d_ref)
    return out


def test_fixtures_hold_what_they_claim(cases):
    for name, (fields, y_pred, f32, f64, d_ref) in cases.items():
        c = XFORM_CASES[name]
        H, W = GRIDS[c["grid"]]
        n_nan = 0
        for k, a in f32.items():
            v = next(v for v in c["variables"] if v["name"] == k.split(":")[1])
            assert a.shape == (c["B"], v["levels"], c["T"], H, W) and d_ref[k].shape == (v["levels"],), (name, k)
            assert np.isnan(a).mean(axis=(0, 2, 3, 4)).max() < 0.01, (name, k)          # fewer than 1 % NaN in every tested level
            assert np.array_equal(np.isnan(a), np.isnan(f64[k])), (name, k)
            n_nan += int(np.isnan(a).sum())
            # d_ref is the reference's own fp32-against-fp64 distance (the fp64 golden is stored as a float32 difference)
            assert d_ref[k] == pytest.approx(level_distance(a, f64[k]), rel=1e-4, abs=1e-12), (name, k)
        assert (n_nan > 0) == c["nan_case"], (name, n_nan)                               # the designated NaN cases have some
        assert y_pred.shape[1] == sum(v["levels"] for v in out_variables(name))
    cs = XFORM_CASES.values()
    assert {c["grid"] for c in cs} == set(GRIDS) and {c["B"] for c in cs} == {1, 2} and {c["T"] for c in cs} == {1, 2}
    assert {v["levels"] for c in cs for v in c["variables"]} >= {1, 13} and max(len(c["variables"]) for c in cs) == 64
    xfs = {v["xf"] for c in cs for v in c["variables"] if v["xf"]}
    assert xfs >= {("log", b, e) for b in ("e", "2", "10") for e in (1e-8, 1e-4)} | {("sqrt",)}
    assert {v["stats"] for c in cs for v in c["variables"]} == {"level", "scalar", None}
    assert any(len(v["fills"]) == 2 for c in cs for v in c["variables"])                 # two stacked FillValues blocks


@pytest.mark.parametrize("name", list(XFORM_CASES))
def test_oracle_fp64_matches_reference_fp64(cases, name):
    fields, y_pred, _, f64, _ = cases[name]
    got = O.case_outputs(name, fields, y_pred, torch.float64)
    for k in f64:
        # the fp64 golden is stored to ~6e-8 of its distance from the fp32 one (<= 6e-6 of the largest value): 1e-12 is far above that
        d = level_distance(got[k], f64[k])
        assert d.max() <= 1e-12, (name, k, d)


@pytest.mark.parametrize("name", list(XFORM_CASES))
def test_oracle_fp32_within_a_quarter_of_the_gate(cases, name):
    fields, y_pred, f32, f64, d_ref = cases[name]
    got = O.case_outputs(name, fields, y_pred, torch.float32)
    for k in f32:
        d32, d64 = level_distance(got[k], f32[k]), level_distance(got[k], f64[k])
        for l in range(len(d32)):
            b32, b64 = gate(d_ref[k][l])
            assert d32[l] <= b32 / 4 and d64[l] <= b64, (name, k, l, d32[l], b32, d64[l], b64)


@pytest.mark.parametrize("name", list(XFORM_CASES))
def test_power_every_transform_and_fill_rule_moves_its_data_by_20_gates(cases, name):
    """A no-op kernel, a skipped rule, a dropped transform or a missing scale cannot pass: leaving any ONE of them out of the oracle
    moves every level of every variable that has it by more than 20 gates (a changed NaN position counts as infinitely far)."""
    import wxengine.transforms as X
    from xform_cases import batch_input, pre_blocks
    fields, y_pred, f32, _, d_ref = cases[name]
    c = XFORM_CASES[name]
    keys = [v["key"] for v in c["variables"]]
    tab = X.compile_channel_table(pre_blocks(name, X), batch_input(name, fields), keys, [v["levels"] for v in c["variables"]])
    first = np.cumsum([0] + [v["levels"] for v in c["variables"]])[:-1]
    n_rules = {v["name"]: int(tab["n_rules"][f]) for v, f in zip(c["variables"], first)}
    assert sum(n_rules.values()) == sum(len(r) for v in c["variables"] for r in v["fills"])      # composing keeps every rule
    skips = ["xf", "scale"] + [f"rule{j}" for j in range(max(n_rules.values()))]
    for skip in skips:
        got = O.case_outputs(name, fields, y_pred, torch.float32, skip=(skip,))
        for k in f32:
            side, var = k.split(":")
            v = next(v for v in c["variables"] if v["name"] == var)
            has = {"xf": v["xf"] is not None, "scale": side == "post" and v["stats"] is not None}.get(skip)
            if has is None:
                has = side == "pre" and int(skip[4:]) < n_rules[var]
            d = level_distance(got[k], f32[k])
            if not has:
                assert d.max() == 0, (name, k, skip)
                continue
            for l in range(len(d)):
                assert d[l] > 20 * gate(d_ref[k][l])[0], (name, k, l, skip, d[l], gate(d_ref[k][l])[0])
