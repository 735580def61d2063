"""Host side of the verification metrics (wxengine/metrics.py), no GPU needed: how the scored variables are resolved and ordered, the
static combination weights in every mode against hand-computed values and against the restatement, the latitude weights, every
rejection with its reason, the climatology shape errors, and without a GPU the class raises -- after the argument checks --
instead of falling back."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import metrics_cases as MC  # noqa: E402
import metrics_oracle as MO  # noqa: E402

from wxengine import metrics as M  # noqa: E402
from wxengine.engine import WXEngineError  # noqa: E402

A, B_, D = "ERA5/prognostic/3d/a", "ERA5/prognostic/2d/b", "ERA5/diagnostic/2d/d"


@pytest.fixture
def pretend_gpu(monkeypatch):
    """Lets the constructor pass its no-GPU check and spares it the library, for what the host side does before it touches the device."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(M, "load_library", lambda: None)


def test_variables_are_resolved_like_the_reference(pretend_gpu):
    pred, target = {D: 0, B_: 0, A: 0}, {B_: 0, A: 0}
    m = M.CombinedMetric({"rmse": {}}, var_weighting="none")
    assert m._resolve_var_keys(pred, target) == [B_, A, D]                      # sorted target keys, then the sorted extras
    m = M.CombinedMetric({"rmse": {}}, var_weighting="none", include_computed_diagnostics=False)
    assert m._resolve_var_keys(pred, target) == [B_, A]
    m = M.CombinedMetric({"rmse": {}}, var_weighting="none", data_var_keys=[A, B_])
    assert m._resolve_var_keys(pred, target) == [A, B_, D]                      # the schema's order is kept


def test_static_weights_in_every_mode(pretend_gpu, caplog):
    keys = [A, B_, D]
    variances = {A: 4.0, B_: 0.0}                                               # D has none; 0 is floored at 1e-12
    m = M.CombinedMetric({"mse": {}, "rmse": {}, "acc": {}, "activity": {}}, variances=variances, variable_weights={A: 2.0},
                         normalize_weights=False)
    with caplog.at_level(logging.WARNING):
        w = m._build_static_weights(keys)
    assert sum("no variance found for 'ERA5/diagnostic/2d/d'" in r.getMessage() for r in caplog.records) == 3   # not for acc
    assert w["mse"] == {A: 2.0 / 4.0, B_: 1.0 / 1e-12, D: 1.0}
    assert w["rmse"] == {A: 2.0 / 2.0, B_: 1.0 / 1e-12 ** 0.5, D: 1.0} and w["activity"] == w["rmse"]
    assert w["acc"] == {A: 2.0, B_: 1.0, D: 1.0}                                # dimensionless: the variances are not consulted
    n = M.CombinedMetric({"mae": {}}, variances={A: 4.0, B_: 16.0, D: 64.0})._build_static_weights(keys)["mae"]
    raw = np.array([1 / 2.0, 1 / 4.0, 1 / 8.0])
    assert list(n.values()) == pytest.approx(list(raw / raw.mean()), rel=1e-15) and sum(n.values()) == pytest.approx(3.0)
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        w = M.CombinedMetric({"bias": {}}, var_weighting="manual", variable_weights={A: 3.0})._build_static_weights(keys)["bias"]
    assert w == {A: 3.0 / (5.0 / 3.0), B_: 1.0 / (5.0 / 3.0), D: 1.0 / (5.0 / 3.0)}
    assert sum("no variable_weights entry" in r.getMessage() for r in caplog.records) == 2
    assert M.CombinedMetric({"bias": {}}, var_weighting="none", variable_weights={A: 0.0, B_: 0.0, D: 0.0})._build_static_weights(keys)["bias"] \
        == {A: 0.0, B_: 0.0, D: 0.0}                                            # mean weight 0: left alone
    # a metric may override the shared weighting, as the reference's args.update(per_metric_args) allows
    w = M.CombinedMetric({"mse": {"var_weighting": "none"}, "mae": {}}, variances={A: 4.0, B_: 4.0, D: 4.0})._build_static_weights(keys)
    assert w["mse"] == {A: 1.0, B_: 1.0, D: 1.0}
    # dimensionless metrics alone need no variances
    M.CombinedMetric({"r2score": {}, "log_variance_ratio": {}, "acc": {}})


@pytest.mark.parametrize("case", ["many", "many_raw", "b2t2", "lev16_basic"])
def test_static_weights_equal_the_restatement(pretend_gpu, case):
    inp = MC.case_inputs(MC.METRICS_CASES[case]["inputs"])
    kw = MC.block_args(case, inp)
    keys = sorted(MC.KEYS[v] for v in MC.INPUTS[MC.METRICS_CASES[case]["inputs"]]["vars"])
    got = M.CombinedMetric(**kw)._build_static_weights(keys)
    c = MC.METRICS_CASES[case]["kwargs"]
    for m in kw["metrics"]:
        want = MO.static_weights(m, keys, c["var_weighting"], c.get("variances"), c.get("variable_weights"), c.get("normalize_weights", True))
        assert got[m] == want, (case, m)


def test_latitude_weights_are_cosines_over_their_mean_in_float32():
    w = M.cos_lat_weights([-60.0, 0.0, 60.0])
    assert w.dtype == torch.float32 and w.shape == (3,)
    c = torch.cos(torch.deg2rad(torch.tensor([-60.0, 0.0, 60.0])))
    assert torch.equal(w, c / c.mean()) and abs(float(w.mean()) - 1.0) < 1e-6 and torch.equal(w, MO.lat_weights([-60.0, 0.0, 60.0]))


CLIM = {"a": np.zeros((2, 3, 4), np.float32)}


@pytest.mark.parametrize("kw,why", [
    (dict(metrics={}), "must list at least one metric"),
    (dict(metrics=None), "must list at least one metric"),
    (dict(metrics={"crps": {}}), "unknown metric 'crps'"),
    (dict(metrics={"combined": {}}), "unknown metric 'combined'"),
    (dict(var_weighting="learnable"), "var_weighting='learnable' is not supported for metrics"),
    (dict(var_weighting="uniform"), "var_weighting must be one of"),
    (dict(metrics={"rmse": {"var_weighting": "learnable"}}), "not supported for metrics"),
    (dict(var_weighting="inverse_variance", variances=None), "variances is required for var_weighting='inverse_variance' with metric 'rmse' \\(scale_power=1\\)"),
    (dict(metrics={"r2score": {}, "mse": {}}, var_weighting="inverse_variance", variances=None), "with metric 'mse' \\(scale_power=2\\)"),
    (dict(use_latitude_weights=True), "latitude \\(degrees\\) is required when use_latitude_weights=True"),
    (dict(metrics={"acc": {"climatology_path": "clim.nc"}}), "climatology_path is not read here; pass the fields as arrays"),
    (dict(metrics={"acc": {"climatology": CLIM}, "activity": {}}), "'acc' and 'activity' must be given the same climatology"),
    (dict(metrics={"acc": {"climatology": CLIM}, "activity": {"climatology": {"a": np.ones((2, 3, 4), np.float32)}}}), "the same climatology"),
    (dict(metrics={"acc": {"accumulate_climatology": False}, "activity": {}}), "the same climatology"),
    (dict(metrics={"rmse": {"eps": 1e-6}}), "'eps' is not an argument of 'rmse'"),
    (dict(metrics={"mae": {"climatology": CLIM}}), "'climatology' is not an argument of 'mae'"),
    (dict(metrics={"rmse": {"use_latitude_weights": True}}), "'use_latitude_weights' is shared by every metric"),
    (dict(metrics={"rmse": {"delta": 1.0}}), "unknown argument 'delta' of 'rmse'"),
])
def test_constructor_rejections_carry_their_reason(kw, why):
    args = dict(metrics={"rmse": {}}, var_weighting="none")
    args.update(kw)
    with pytest.raises(ValueError, match=why):
        M.CombinedMetric(**args)


def test_equal_climatologies_in_two_dicts_are_accepted(pretend_gpu):
    m = M.CombinedMetric({"acc": {"climatology": CLIM}, "activity": {"climatology": {"a": CLIM["a"].copy()}}}, var_weighting="none")
    assert m.need_climatology and not M.CombinedMetric({"rmse": {}}, var_weighting="none").need_climatology
    assert m._climatology["a"].dtype == torch.float32 and m.last_var_scores == {"acc": {}, "activity": {}}


def test_climatology_shape_errors_are_those_of_get_clim(pretend_gpu):
    clim = {A: np.zeros((2, 3, 4), np.float32), "b": np.zeros((3, 4), np.float32), "c": np.zeros((1, 2, 3, 4), np.float32),
            "e": np.zeros((5, 4), np.float32)}
    m = M.CombinedMetric({"acc": {"climatology": clim}}, var_weighting="none")
    dev = torch.device("cpu")
    t, ls, ts = m._fixed_clim(A, (1, 2, 1, 3, 4), dev)                           # the full key; (level, lat, lon)
    assert tuple(t.shape) == (2, 3, 4) and (ls, ts) == (12, 0)
    t, ls, ts = m._fixed_clim(B_, (1, 7, 1, 3, 4), dev)                          # the short name; one level broadcast over seven
    assert tuple(t.shape) == (3, 4) and (ls, ts) == (0, 0)
    assert m._fixed_clim(D, (1, 1, 1, 3, 4), dev) is None
    with pytest.raises(ValueError, match="has 2 levels but the field has 5"):
        m._fixed_clim(A, (1, 5, 1, 3, 4), dev)
    with pytest.raises(ValueError, match="has shape \\(1, 2, 3, 4\\); expected \\(lat, lon\\) for a 2-D variable or \\(level, lat, lon\\)"):
        m._fixed_clim("ERA5/prognostic/3d/c", (1, 2, 1, 3, 4), dev)
    with pytest.raises(ValueError, match="is on a \\(5, 4\\) grid, the field on \\(3, 4\\)"):
        m._fixed_clim("ERA5/prognostic/2d/e", (1, 1, 1, 3, 4), dev)


def test_state_dict_errors_are_the_reference_key_errors(pretend_gpu):
    m = M.CombinedMetric({"rmse": {}}, var_weighting="none")
    with pytest.raises(KeyError, match="requires full_data_dict\\['y_processed'\\]"):
        m({"y_target_processed": {}})
    with pytest.raises(KeyError, match="requires full_data_dict\\['y_target_processed'\\]"):
        m({"y_processed": {}})
    with pytest.raises(ValueError, match="'y_processed' is empty"):
        m({"y_processed": {"ERA5": {}}, "y_target_processed": {"ERA5": {}}})
    x = torch.zeros(1, 1, 1, 3, 4)
    with pytest.raises(KeyError, match="variable 'ERA5/prognostic/2d/b' missing from y_processed"):
        M.CombinedMetric({"rmse": {}}, var_weighting="none")({"y_processed": {"ERA5": {A: x}}, "y_target_processed": {"ERA5": {A: x, B_: x}}})
    with pytest.raises(KeyError, match="variable 'ERA5/diagnostic/2d/d' missing from y_target_processed"):
        M.CombinedMetric({"rmse": {}}, var_weighting="none")({"y_processed": {"ERA5": {A: x, D: x}}, "y_target_processed": {"ERA5": {A: x}}})
    with pytest.raises(WXEngineError, match="on the GPU"):
        M.CombinedMetric({"rmse": {}}, var_weighting="none")({"y_processed": {"ERA5": {A: x}}, "y_target_processed": {"ERA5": {A: x}}})


def test_every_case_passes_the_argument_checks():
    """Past every ValueError -- to the device error where there is no GPU."""
    for case, c in MC.METRICS_CASES.items():
        kw = MC.block_args(case, MC.case_inputs(c["inputs"]))
        if torch.cuda.is_available():
            M.CombinedMetric(**kw)
        else:
            with pytest.raises(WXEngineError, match="no GPU visible"):
                M.CombinedMetric(**kw)


def test_no_gpu_raises_after_validation_instead_of_falling_back():
    import wxengine
    assert wxengine.CombinedMetric is M.CombinedMetric and wxengine.PendingScores is M.PendingScores
    if torch.cuda.is_available():
        return
    with pytest.raises(WXEngineError, match="no CPU fallback"):
        M.CombinedMetric({"rmse": {}}, var_weighting="none")
    with pytest.raises(ValueError, match="unknown metric"):       # the argument checks come first
        M.CombinedMetric({"spectrum": {}}, var_weighting="none")
