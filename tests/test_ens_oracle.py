"""The restatement of the ensemble verification (tests/ens_oracle.py) against the goldens (tests/golden/ens_*.npz, tools/make_goldens.py
--only ensemble), no GPU and no reference tree needed: the regenerated inputs carry the fixture's hashes, the float32 restatement
reproduces the stored float32 forward (the reference's own classes for the three CRPS flavours) to float32 rounding, the float64
restatement reproduces the stored yardstick, the keys come in the documented order, and the algebraic identities the kernel rests on
hold in float64."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import ens_cases as EC  # noqa: E402
import ens_oracle as EO  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def restated(case, inp, dtype):
    c = EC.ENS_CASES[case]
    w = EO.lat_weights(inp["lat"]) if c["lat"] else None
    members = {EC.KEYS[n]: torch.from_numpy(v) for n, v in inp["members"].items()}
    truth = {EC.KEYS[n]: torch.from_numpy(v) for n, v in inp["truth"].items()}
    return EO.restate(members, truth, c["alpha"], w, dtype)


@pytest.mark.parametrize("case", list(EC.ENS_CASES))
def test_restatement_reproduces_the_goldens(case):
    g = EC.load_golden(case, GOLD)
    inp = EC.case_inputs(case, check=g["fix"])
    r32, m32 = restated(case, inp, torch.float32)
    r64, m64 = restated(case, inp, torch.float64)
    f32, f64 = EC.flat_scalars(r32), EC.flat_scalars(r64)
    assert list(f32) == g["keys"] == list(f64) == EC.scalar_keys(case)
    for i, k in enumerate(g["keys"]):
        # the same operations as the reference's: float32 rounding of the score itself, no more (1e-6 of its magnitude)
        assert abs(f32[k] - g["f32"][i]) <= 1e-6 * max(abs(g["f32"][i]), g["scale"][i]), (case, k)
        assert abs(f64[k] - g["f64"][i]) <= 1e-12 * max(1.0, abs(g["f64"][i])), (case, k)
        assert abs(g["f64"][i]) == g["scale"][i]
        assert EC.distance(g["f32"][i], g["f64"][i], g["scale"][i]) == g["d_ref"][i]
    assert sorted({n for _, n in g["maps"]}) == sorted(EC.ENS_CASES[case]["map_vars"])
    for (m, n), gm in g["maps"].items():
        k = EC.KEYS[n]
        assert gm["f32"].shape == inp["truth"][n].shape and gm["f32"].dtype == np.float32
        assert EC.map_distance(m32[m][k].numpy(), gm["f32"], gm["scale"]) <= 1e-6, (case, m, n)
        # the fp64 golden is stored as a float32 difference from the fp32 one: exact to 2^-24 of that difference
        assert EC.map_distance(m64[m][k].numpy(), gm["f64"], gm["scale"]) <= 1e-6 * max(gm["d_ref"], 1e-6), (case, m, n)
        assert EC.map_distance(gm["f32"], gm["f64"], gm["scale"]) == pytest.approx(gm["d_ref"], rel=1e-5, abs=1e-12)


def test_key_order_is_per_score_every_variable_with_levels_then_the_per_channel_arrays():
    g = EC.load_golden("m3", GOLD)
    T, sp = EC.KEYS["T"], EC.KEYS["sp"]
    want = []                       # variables in sorted key order: .../2d/surface_pressure before .../3d/temperature
    for s in ("crps", "fair_crps", "afcrps"):
        want += [f"{s}/{sp}", f"{s}/{T}"]
    for s in ("ens_rmse", "ens_spread"):
        want += [f"{s}/{sp}", f"{s}/{sp}/0", f"{s}/{T}"] + [f"{s}/{T}/{lev}" for lev in range(5)]
    for s in ("spread_skill", "ens_abs_err", "ens_std"):
        want += [f"{s}/{sp}", f"{s}/{T}"]
    want += [f"crps_per_channel/{sp}/0"] + [f"crps_per_channel/{T}/{lev}" for lev in range(5)]
    assert g["keys"] == want


@pytest.mark.parametrize("case", list(EC.ENS_CASES))
def test_algebraic_identities_in_float64(case):
    c = EC.ENS_CASES[case]
    inp = EC.case_inputs(case)
    M = c["M"]
    for n in c["vars"]:
        x, y = torch.from_numpy(inp["members"][n]).double(), torch.from_numpy(inp["truth"][n]).double()
        pred = torch.movedim(x, 0, -1)
        scale = max(1e-300, float(torch.abs(pred - y[..., None]).mean()))
        close = lambda a, b: float((a - b).abs().max()) <= 1e-11 * scale      # noqa: E731
        fair, biased = EO.crps_by_sort(pred, y, True), EO.crps_by_sort(pred, y, False)
        assert close(fair, EO.crps_by_pairs(pred, y, 1.0)), (case, n)                        # fair CRPS == almost-fair CRPS at alpha = 1
        d = pred - y[..., None]
        skill = d.abs().sum(-1)
        direct, by_sort = EO.pair_sums(d)
        assert close(direct, by_sort), (case, n)                                         # the sorted sum == the pairwise sum
        assert close(biased, skill / M - direct / M ** 2), (case, n)                     # biased CRPS == skill / M - pair / M^2
        assert close(fair, skill / M - direct / (M * (M - 1))), (case, n)
        assert close(EO.crps_by_pairs(pred, y, c["alpha"]), skill / M - (1 - (1 - c["alpha"]) / M) * direct / (M * (M - 1))), (case, n)
        # the kernel's form of the sorted sum: ranks r = 0 .. M - 1 on the centred, sorted d
        e, _ = torch.sort(d - d.mean(-1, keepdim=True))
        r = torch.arange(M, dtype=torch.float64)
        assert close(direct, 2 * (r * e).sum(-1) + (1 - M) * e.sum(-1)), (case, n)
        assert close(torch.std(x, dim=0), torch.sqrt((e ** 2).sum(-1) / (M - 1))), (case, n)


def test_the_cases_are_what_they_are_there_for():
    for case, c in EC.ENS_CASES.items():
        inp = EC.case_inputs(case)
        for n in c["vars"]:
            t, x = inp["truth"][n], inp["members"][n]
            assert x.shape == (c["M"],) + t.shape and t.dtype == x.dtype == np.float32
            assert EC._coincidences(t, x).any() == (case == "ties"), (case, n)
    t = EC.case_inputs("ties")
    eq, two, hit = (t["members"][n] for n in ("equal", "two", "hit"))
    assert (eq == eq[:1]).all() and (two[0] == two[1]).all() and (two[0] != two[2]).all() and (hit[2] == t["truth"]["hit"]).all()
    g = EC.load_golden("ties", GOLD)
    val = dict(zip(g["keys"], g["f64"]))
    k = EC.KEYS["equal"]
    assert val[f"ens_spread/{k}"] == 0.0 and val[f"ens_std/{k}"] == 0.0 and val[f"spread_skill/{k}"] == 0.0
    assert val[f"crps/{k}"] == pytest.approx(float(np.abs(eq[0].astype(np.float64) - t["truth"]["equal"]).mean()), rel=1e-12)
    sp = EC.case_inputs("m3")["truth"]["sp"]
    assert 99000 < sp.min() < 99300 and 100700 < sp.max() < 101000
    # the [B * M] layout: member m of item b in row b * M + m (only B = 2 tells it from the swapped order)
    x = EC.case_inputs("m3")["members"]["sp"]
    s = EC.stacked(x)
    assert np.array_equal(s[1 * 3 + 1], x[1, 1]) and not np.array_equal(s[1 * 2 + 1], x[1, 1])      # row b * M + m, not m * B + b
