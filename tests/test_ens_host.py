"""Host side of the ensemble verification (wxengine/ensemble_metrics.py), no GPU needed: argument validation, the key order, the host
formulas from a plane table against the float64 restatement, the pointer and stride table for both member layouts, and without a
GPU the class raises -- after the argument checks -- instead of falling back."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import ens_cases as EC  # noqa: E402
import ens_oracle as EO  # noqa: E402

from wxengine import ensemble_metrics as EM  # noqa: E402
from wxengine.engine import WXEngineError  # noqa: E402

A, B_ = "ERA5/prognostic/3d/a", "ERA5/prognostic/2d/b"


def test_argument_validation():
    assert EM.check_arguments(2) == (2, 1.0, ())
    assert EM.check_arguments(64, 0.95, ("crps", "ens_mean")) == (64, 0.95, ("ens_mean", "crps"))      # MAP_ORDER
    assert EM.check_arguments(3, maps="afcrps") == (3, 1.0, ("afcrps",))
    for bad in (1, 65, 0, -3, 2.5):
        with pytest.raises(ValueError, match="n_members must be an integer in 2..64"):
            EM.check_arguments(bad)
    with pytest.raises(ValueError, match="alpha must be finite"):
        EM.check_arguments(4, float("nan"))
    with pytest.raises(ValueError, match="unknown map 'ens_rmse'"):
        EM.check_arguments(4, maps=("ens_rmse",))
    with pytest.raises(ValueError, match="latitude \\(degrees\\) is required"):
        EM.EnsembleVerification(4, use_latitude_weights=True)


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_no_gpu_raises_after_the_argument_checks():
    with pytest.raises(ValueError):
        EM.EnsembleVerification(1)
    with pytest.raises(WXEngineError, match="no CPU fallback"):
        EM.EnsembleVerification(4)


def test_exported_from_the_package():
    import wxengine
    assert wxengine.EnsembleVerification is EM.EnsembleVerification and wxengine.PendingEnsembleScores is EM.PendingEnsembleScores
    from wxengine.rollout import score_ensemble_rollout  # noqa: F401
    assert EM.MAP_ORDER == EC.MAPS and EM.SCALAR_ORDER == EC.SCALARS == EO.SCALARS and EM.MAX_MEMBERS == 64 and EM.MAX_VARIABLES == 32


def test_key_order():
    keys = EM.result_keys({A: 2, B_: 1})
    want = [f"{s}/{v}" for s in ("crps", "fair_crps", "afcrps") for v in (A, B_)]
    for s in ("ens_rmse", "ens_spread"):
        want += [f"{s}/{A}", f"{s}/{A}/0", f"{s}/{A}/1", f"{s}/{B_}", f"{s}/{B_}/0"]
    want += [f"{s}/{v}" for s in ("spread_skill", "ens_abs_err", "ens_std") for v in (A, B_)]
    want += [f"crps_per_channel/{A}", f"crps_per_channel/{B_}"]
    assert keys == want
    tab = {A: np.ones((1, 2, 1, 6)), B_: np.ones((1, 1, 1, 6))}
    assert list(EM.scores_from_planes(tab, 4, 1.0, 10)) == want


def plane_table(x, y, w):
    """The six plane sums [B, L, T, 6] of one variable in float64, written from their definitions."""
    x, y = x.double(), y.double()
    M = x.shape[0]
    d = x - y
    err = d.mean(0)
    e = d - err
    pair = 0.5 * (d.unsqueeze(0) - d.unsqueeze(1)).abs().sum(dim=(0, 1))
    ss = (e ** 2).sum(0)
    q = [d.abs().sum(0), pair, err ** 2, err.abs(), ss, torch.sqrt(ss / (M - 1))]
    wt = 1.0 if w is None else w.double().reshape(1, 1, 1, -1, 1)
    return torch.stack([(v * wt).sum(dim=(-2, -1)) for v in q], dim=-1).numpy()


@pytest.mark.parametrize("case", ["m2", "m3", "m5lat", "m50", "ties"])
def test_host_formulas_from_a_plane_table_equal_the_restatement(case):
    c = EC.ENS_CASES[case]
    inp = EC.case_inputs(case)
    w = EO.lat_weights(inp["lat"]) if c["lat"] else None
    members = {EC.KEYS[n]: torch.from_numpy(v) for n, v in inp["members"].items()}
    truth = {EC.KEYS[n]: torch.from_numpy(v) for n, v in inp["truth"].items()}
    want, _ = EO.restate(members, truth, c["alpha"], w, torch.float64, want_maps=False)
    planes = {k: plane_table(members[k], truth[k], w) for k in sorted(truth)}
    H, W = c["grid"]
    got = EM.scores_from_planes(planes, c["M"], c["alpha"], H * W)
    assert list(got) == list(want) == EM.result_keys({k: truth[k].shape[1] for k in sorted(truth)})
    fg, fw = EC.flat_scalars(got), EC.flat_scalars(want)
    for k in fw:
        assert fg[k] == pytest.approx(fw[k], rel=1e-11, abs=1e-300), (case, k)
    assert got[f"crps_per_channel/{EC.KEYS[next(iter(c['vars']))]}"].shape == (next(iter(c["vars"].values()))[1],)


def test_plane_table_shape_is_checked():
    with pytest.raises(ValueError, match="a plane table is \\[B, L, T, 6\\]"):
        EM.scores_from_planes({A: np.ones((2, 6))}, 4, 1.0, 10)


def test_pointer_and_stride_table_for_both_member_layouts():
    M, B, L, T, H, W = 3, 2, 5, 2, 4, 6
    x = torch.arange(M * B * L * T * H * W, dtype=torch.float32).reshape(M, B, L, T, H, W)
    separate = [{A: x[m].clone()} for m in range(M)]
    tab = EM.member_table(separate, M, [A])
    assert tab[0]["ptrs"] == [separate[m][A].data_ptr() for m in range(M)]
    assert tab[0]["batch_stride"] == L * T * H * W and tab[0]["shape"] == (B, L, T, H, W)
    stacked = torch.from_numpy(EC.stacked(x.numpy()))            # [B * M, L, T, H, W], member m of item b in row b * M + m
    tab = EM.member_table({A: stacked}, M, [A])
    item = L * T * H * W
    assert tab[0]["ptrs"] == [stacked.data_ptr() + 4 * m * item for m in range(M)]
    assert tab[0]["batch_stride"] == M * item and tab[0]["shape"] == (B, L, T, H, W)
    for m in range(M):          # what the kernel reads at (member m, item b) is x[m, b] in both layouts
        for b in range(B):
            off = (tab[0]["ptrs"][m] - stacked.data_ptr()) // 4 + b * tab[0]["batch_stride"]
            assert stacked.reshape(-1)[off] == x[m, b].reshape(-1)[0]
    # channel slices of a wider tensor: read in place through the row stride; nested {source: {var: ...}} dicts are flattened
    wide = torch.zeros(B * M, L + 3, T, H, W)
    view = wide[:, 2:2 + L]
    tab = EM.member_table({"ERA5": {A: view}}, M, [A])
    assert tab[0]["ptrs"][1] == view.data_ptr() + 4 * wide.stride(0) and tab[0]["batch_stride"] == M * wide.stride(0)
    views = [{"ERA5": {A: torch.zeros(B, L + 3, T, H, W)[:, 1:1 + L]}} for _ in range(M)]
    assert EM.member_table(views, M, [A])[0]["batch_stride"] == (L + 3) * T * H * W
    with pytest.raises(ValueError, match="the stacked layout is \\[B \\* n_members, L, T, H, W\\]"):
        EM.member_table({A: stacked[:5]}, M, [A])
    with pytest.raises(ValueError, match="2 member dicts for n_members = 3"):
        EM.member_table(separate[:2], M, [A])
    with pytest.raises(KeyError, match="missing from member 1"):
        EM.member_table([separate[0], {B_: x[1]}, separate[2]], M, [A])
    with pytest.raises(ValueError, match="batch strides differ"):
        EM.member_table([separate[0], separate[1], {A: torch.zeros(B, L + 1, T, H, W)[:, :L]}], M, [A])
    with pytest.raises(ValueError, match="must be one \\[B, L, T, H, W\\] shape"):
        EM.member_table([separate[0], separate[1], {A: x[2][:, :4]}], M, [A])
