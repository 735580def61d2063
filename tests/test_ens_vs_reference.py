"""The ensemble-verification fixtures and the restatement (tests/ens_oracle.py) against the LIVE reference classes
(credit/losses/gen_1/kcrps.py KCRPSLoss, almost_fair_crps.py AlmostFairKCRPSLoss); skipped where the reference tree is absent.  The
classes run unmodified on the reference's [B * M, ...] layout.  LatWeightedMetricsEnsemble, calculate_ensemble_metrics and
calculate_crps_per_channel cannot be imported beside this project's interpreter and packages (tools/make_goldens.py
ensemble_reference says why); they are held by the restatement, which cites their lines."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import ens_cases as EC  # noqa: E402
import ens_oracle as EO  # noqa: E402

pytestmark = pytest.mark.reference
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def classes():
    import oracle_stub
    oracle_stub.install()
    from credit.losses.gen_1.almost_fair_crps import AlmostFairKCRPSLoss
    from credit.losses.gen_1.kcrps import KCRPSLoss
    return KCRPSLoss, AlmostFairKCRPSLoss


@pytest.mark.parametrize("case", list(EC.ENS_CASES))
def test_reference_reproduces_the_goldens_and_the_restatement(classes, case):
    KCRPSLoss, AlmostFairKCRPSLoss = classes
    c = EC.ENS_CASES[case]
    g = EC.load_golden(case, GOLD)
    inp = EC.case_inputs(case, check=g["fix"])
    w = EO.lat_weights(inp["lat"]) if c["lat"] else None
    wt = 1.0 if w is None else w.reshape(1, 1, 1, -1, 1)
    val32 = dict(zip(g["keys"], g["f32"]))
    scale = dict(zip(g["keys"], g["scale"]))
    for n in c["vars"]:
        k = EC.KEYS[n]
        y, x = torch.from_numpy(inp["truth"][n]), torch.from_numpy(EC.stacked(inp["members"][n]))
        with torch.no_grad():
            live = {"crps": KCRPSLoss("none", biased=True)(y, x), "fair_crps": KCRPSLoss("none", biased=False)(y, x),
                    "afcrps": AlmostFairKCRPSLoss(alpha=c["alpha"], reduction="none")(y, x).reshape(y.shape)}
        mine, maps = EO.variable(torch.from_numpy(inp["members"][n]), y, c["alpha"], w, torch.float32)
        for m, ref_map in live.items():
            got = (ref_map * wt).mean().item()
            assert got == val32[f"{m}/{k}"], (case, n, m)                              # the fixture IS the reference's forward
            assert abs(mine[m] - got) <= 1e-6 * max(abs(got), scale[f"{m}/{k}"]), (case, n, m)
            if (m, n) in g["maps"]:
                assert np.array_equal(ref_map.numpy(), g["maps"][(m, n)]["f32"]), (case, n, m)
                assert EC.map_distance(maps[m].numpy(), ref_map.numpy(), g["maps"][(m, n)]["scale"]) <= 1e-6, (case, n, m)
        if not c["lat"]:      # the reduced forms: KCRPSLoss(...)(y, x).mean() and AlmostFairKCRPSLoss(alpha)(y, x)
            assert AlmostFairKCRPSLoss(alpha=c["alpha"])(y, x).item() == val32[f"afcrps/{k}"]
        per_channel = (live["crps"] * wt).mean(dim=[0, 2, 3, 4]).numpy()
        for lev, v in enumerate(per_channel):
            assert float(v) == val32[f"crps_per_channel/{k}/{lev}"], (case, n, lev)
