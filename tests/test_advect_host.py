"""Host side of the semi-Lagrangian advection (wxengine/advect.py), no GPU needed: the constructor refuses what the block cannot run
with the reason, `levels` slices the half levels as the reference does, the metric tables the device gets equal the reference's float32
torch expressions (torch.gradient itself for the latitude difference), the grid-mismatch fallback and its single warning, the pre
block's `data_types`, and without a GPU the block raises instead of falling back."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from advect_cases import ADVECT_CASES, KEYS, block_args, grid_of  # noqa: E402

from wxengine import advect as A  # noqa: E402
from wxengine.engine import WXEngineError  # noqa: E402


@pytest.mark.parametrize("kw,why", [
    (dict(n_iterations=0), "n_iterations = 0, the back-trajectory takes at least one"),
    (dict(level_order="bottom_up"), "level_order 'bottom_up' is neither of"),
    (dict(lon_halo=0), "lon_halo = 0 must be >= 1"),
    (dict(tracer_vars=[KEYS["q"], KEYS["T"], KEYS["q"]]), "a tracer is listed twice"),
    (dict(tracer_vars=[f"ERA5/prognostic/3d/t{i}" for i in range(33)]), "33 tracers, one call takes at most 32"),
    (dict(coslat_floor=float("nan")), "coslat_floor = nan must be finite"),
    (dict(dp_dlevel_floor=float("inf")), "dp_dlevel_floor = inf must be finite"),
    (dict(timestep_seconds=float("inf")), "timestep_seconds = inf must be finite"),
    (dict(longitude=[0.0]), "1 longitude\\(s\\)"),
    (dict(latitude=[0.0]), "1 latitude\\(s\\)"),
    (dict(model_a_half=None), "model_a_half is required"),
    (dict(latitude=None), "latitude is required"),
])
def test_constructor_rejections_carry_their_reason(kw, why):
    args = block_args("base36")
    args.update(kw)
    for cls in (A.SemiLagrangianAdvection, A.SemiLagrangianAdvectionPre):
        with pytest.raises(ValueError, match=why):
            cls(**args)


def test_levels_slice_the_half_levels_as_the_reference_does():
    a_all, b_all = np.arange(13, dtype=np.float64) * 1.5, np.arange(13, dtype=np.float64) / 12
    levels = list(range(3, 11))
    a, b = A.slice_half_levels(a_all, b_all, levels)
    half_idx = [lv - 1 for lv in levels] + [levels[-1]]          # advect.py:263
    assert a.dtype == b.dtype == np.float32 and a.shape == (9,)
    assert np.array_equal(a, a_all.astype(np.float32)[half_idx]) and np.array_equal(b, b_all.astype(np.float32)[half_idx])
    assert list(half_idx) == list(range(2, 11))
    a, b = A.slice_half_levels(a_all, b_all, None)
    assert a.shape == (13,) and np.array_equal(b, b_all.astype(np.float32))
    a, _ = A.slice_half_levels(a_all, b_all, [2, 5, 9])          # levels that are not adjacent: lower interfaces, then the last upper one
    assert list(a) == [1.5, 6.0, 12.0, 13.5]


@pytest.mark.parametrize("name", ["base36", "gauss", "tiny"])
def test_metric_tables_equal_the_reference_float32_expressions(name):
    lat, lon = grid_of(name)
    H = lat.size
    t = A.metric_tables(lat, lon, 1e-4)
    rows = torch.from_numpy(t["rows"])
    assert rows.dtype == torch.float32 and rows.shape == (6, H)
    lat_rad = torch.deg2rad(torch.from_numpy(lat))                                       # advect.py:316
    assert torch.equal(rows[0], torch.cos(lat_rad))                                      # :107
    assert torch.equal(rows[1], 6371000.0 * torch.cos(lat_rad).clamp(min=1e-4))          # :108 / :374, radius * coslat_safe
    assert torch.equal(rows[2], torch.gradient(lat_rad, edge_order=1)[0])                # :318
    assert t["dlon"] == torch.deg2rad(torch.from_numpy(lon)[1] - torch.from_numpy(lon)[0]).item()      # :319
    if name != "gauss":      # exact poles: cos is below the floor there, and only there
        assert rows[1][0] == rows[1][-1] == np.float32(637.1) and (rows[1][1:-1] > 637.1).all()
    # the three coefficients against torch.gradient itself (:116) on random fields, bit for bit
    g = torch.Generator().manual_seed(0)
    f = torch.randn(2, 3, H, 5, generator=g)
    want = torch.gradient(f, spacing=(lat_rad,), dim=(-2,), edge_order=1)[0]
    a, b, c = (rows[i].view(H, 1) for i in (3, 4, 5))
    mid = a[1:-1] * f[..., :-2, :] + b[1:-1] * f[..., 1:-1, :] + c[1:-1] * f[..., 2:, :]
    assert torch.equal(mid, want[..., 1:-1, :])
    assert torch.equal((f[..., 1, :] - f[..., 0, :]) / b[0], want[..., 0, :])
    assert torch.equal((f[..., -1, :] - f[..., -2, :]) / b[-1], want[..., -1, :])
    if name == "gauss":
        assert float((rows[2].max() - rows[2].min()) / rows[2].abs().max()) > 0.3        # the spacing really varies


@pytest.fixture
def pretend_gpu(monkeypatch):
    """Lets the constructor pass its no-GPU check and spares it the library, for what the host side does before it touches the device."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(A, "load_library", lambda: None)


def test_grid_mismatch_falls_back_to_the_uniform_grid_with_one_warning(pretend_gpu, caplog):
    blk = A.SemiLagrangianAdvection(**block_args("gauss"))           # 25 x 40 coordinates
    lat, lon = grid_of("gauss")
    with caplog.at_level(logging.WARNING, logger="wxengine.advect"):
        same = blk.engine.grid_for(25, 40)
        assert same[0] is blk.engine.lat_deg and np.array_equal(same[0], lat) and np.array_equal(same[1], lon)
        assert not caplog.records
        for _ in range(3):
            la, lo = blk.engine.grid_for(24, 36)
    assert np.array_equal(la, torch.linspace(90.0, -90.0, 24).numpy())                    # advect.py:313
    assert np.array_equal(lo, (torch.arange(36, dtype=torch.float32) * (360.0 / 36)).numpy())
    warned = [r.getMessage() for r in caplog.records]
    assert len(warned) == 1 and "25 latitudes x 40 longitudes were given, the data grid is 24 x 36" in warned[0]


def test_preblock_data_types(pretend_gpu):
    args = block_args("base36")
    with pytest.raises(ValueError, match="Invalid data_types {'metadata'}"):
        A.SemiLagrangianAdvectionPre(data_types=["input", "metadata"], **args)
    pre = A.SemiLagrangianAdvectionPre(**args)
    assert pre.data_types == ["input", "target"]
    seen = []

    def fake(nested):
        seen.append(nested)
        nested["ERA5"][KEYS["q"]] = "advected"
    pre.engine.advect_nested = fake
    batch = {"input": {"ERA5": {KEYS["q"]: "q0"}}, "metadata": {"anything": 1}}        # no "target": skipped silently
    out = pre(batch)
    assert len(seen) == 1 and out["input"]["ERA5"][KEYS["q"]] == "advected" and out["metadata"] is batch["metadata"]
    assert batch["input"]["ERA5"][KEYS["q"]] == "q0" and set(batch) == {"input", "metadata"}      # the caller's dict is not mutated
    only_target = A.SemiLagrangianAdvectionPre(data_types=["target"], **args)
    only_target.engine.advect_nested = fake
    only_target(batch)
    assert len(seen) == 1


def test_every_case_passes_the_argument_checks():
    """Past every ValueError -- to the device error where there is no GPU."""
    for name in ADVECT_CASES:
        if torch.cuda.is_available():
            A.SemiLagrangianAdvection(**block_args(name))
        else:
            with pytest.raises(WXEngineError, match="no GPU visible"):
                A.SemiLagrangianAdvection(**block_args(name))


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_no_gpu_raises_instead_of_falling_back():
    for cls in (A.SemiLagrangianAdvection, A.SemiLagrangianAdvectionPre):
        with pytest.raises(WXEngineError, match="no CPU fallback"):
            cls(**block_args("base36"))
    import wxengine
    assert wxengine.SemiLagrangianAdvection is A.SemiLagrangianAdvection
    assert wxengine.SemiLagrangianAdvectionPre is A.SemiLagrangianAdvectionPre
