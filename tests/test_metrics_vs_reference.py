"""The verification-metrics fixtures and the restatement (tests/metrics_oracle.py) against the LIVE reference
(credit/metrics/base.py, common.py, anomaly.py); skipped where the reference tree is absent.  The class runs unmodified; the two
loaders that read files (`_load_target_variances`, `_cos_lat_weights`) serve the case's arrays (monkeypatch).  The online cases make
their three successive calls on ONE object, as a validation loop does."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import metrics_cases as MC  # noqa: E402
import metrics_oracle as MO  # noqa: E402

pytestmark = pytest.mark.reference
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture
def reference(monkeypatch):
    import oracle_stub
    oracle_stub.install()
    import credit.metrics.base as RB
    served = {}
    monkeypatch.setattr(RB, "_load_target_variances", lambda path: dict(served["variances"]))
    monkeypatch.setattr(RB, "_cos_lat_weights", lambda path: MO.lat_weights(served["lat"]))
    return RB, served


@pytest.mark.parametrize("case", list(MC.METRICS_CASES))
def test_reference_reproduces_the_goldens_and_the_restatement(reference, case):
    RB, served = reference
    c = MC.METRICS_CASES[case]
    g, keys, f32, f64, d_ref, scale = MC.load_golden(case, GOLD)
    inp = MC.case_inputs(c["inputs"], check=g)
    kw, served["variances"] = MC.reference_args(case, inp)
    served["lat"] = inp["lat"]
    ref = RB.BaseCombinedMetric(**kw)
    mine = MO.Restatement(dtype=torch.float32, **MC.block_args(case, inp))
    for call in range(f32.shape[0]):
        full = MC.state_dicts(inp, call, torch.from_numpy)
        with torch.no_grad():
            got = ref(full)
        restated = mine(full)
        assert list(got) == keys == list(restated), case
        for i, k in enumerate(keys):
            assert got[k] == f32[call, i], (case, call, k)                       # the fixture IS the reference's forward
            assert abs(restated[k] - got[k]) <= 1e-6 * max(abs(got[k]), scale[call, i] if np.isfinite(scale[call, i]) else 0.0), (case, call, k)
    for name, mod in ref.metric_modules.items():                                  # the static weights, every mode the cases use
        for k, w in mod._combination_weights.items():
            assert mine.weights[name][k] == w, (case, name, k)
        assert list(mod.var_keys) == mine.var_keys


def test_latitude_weights_equal_the_reference_loader(monkeypatch):
    import oracle_stub
    oracle_stub.install()
    import credit.losses.base as RL
    lat = MC.latitude(33)
    before = sys.modules.get("xarray")
    sys.modules["xarray"] = oracle_stub.serve_xarray({"latitude": lat})
    try:
        want = RL._cos_lat_weights("grid.nc")
    finally:
        if before is None:
            sys.modules.pop("xarray", None)
        else:
            sys.modules["xarray"] = before
    assert torch.equal(want, MO.lat_weights(lat))
    from wxengine.metrics import cos_lat_weights
    assert torch.equal(want, cos_lat_weights(lat))
