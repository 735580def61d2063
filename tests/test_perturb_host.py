"""The host side of the perturbation noise without a GPU: argument checking, `__repr__`, the amplitude rules, the validation of
`perturbed_ensemble_rollout`, the generator's slot, and the new symbols of the C ABI."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import perturb_cases as PC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def WP(monkeypatch):
    import wxengine.perturb as WP
    monkeypatch.setattr(WP._Noise, "_open", lambda self, device: None)
    return WP


def test_exported_lazily_and_raises_without_a_gpu():
    import torch
    import wxengine
    from wxengine.engine import WXEngineError
    assert wxengine.GaussianNoise is wxengine.perturb.GaussianNoise and wxengine.ColorNoise is wxengine.perturb.ColorNoise
    assert wxengine.TemporalNoise is wxengine.perturb.TemporalNoise and wxengine.hemispheric_weights is wxengine.perturb.hemispheric_weights
    if not torch.cuda.is_available():
        for make in (wxengine.GaussianNoise, wxengine.ColorNoise):
            with pytest.raises(WXEngineError, match="no CPU fallback"):
                make()
    with pytest.raises(ValueError, match="TemporalNoise.perturbation_std"):      # the argument's own faults come first
        wxengine.GaussianNoise([0.1, 0.2])


def test_repr_defaults_and_amplitude_rules(WP):
    assert repr(WP.GaussianNoise()) == "GaussianNoise(amplitude=0.05)" and repr(WP.ColorNoise()) == "ColorNoise(amplitude=0.05,reddening=2)"
    assert repr(WP.ColorNoise(0.2, 3)) == "ColorNoise(amplitude=0.2,reddening=3)"
    assert WP.GaussianNoise(0.3)._amp == 0.3 and WP.GaussianNoise(2)._amp == 2.0
    for one in ([0.05], (0.05,), np.array([0.05]), np.float32(0.25) * np.ones(1)):      # rollout_metrics_noisy_ic.py: amplitude * weights
        assert WP.ColorNoise(one)._amp == float(np.asarray(one)[0])
    for many in ([0.1, 0.2], np.ones(3), []):
        with pytest.raises(ValueError, match="TemporalNoise.perturbation_std"):
            WP.ColorNoise(many)
    for bad in (True, "a", None):
        with pytest.raises(TypeError):
            WP.GaussianNoise(bad)
    for bad in (-1, "2", None, float("nan"), True):
        with pytest.raises(ValueError, match="reddening"):
            WP.ColorNoise(0.05, bad)


def test_weights_table(WP):
    for name, red in PC.FILTER_RUNS:
        H, W = PC.PERTURB_CASES[name]["shape"][-2:]
        g = PC.load_golden(name, os.path.join(ROOT, "tests", "golden"))
        S = WP.ColorNoise(1.0, red).weights(H, W)
        # bit for bit beside the live reference on one host (tests/test_perturb_vs_reference.py); across hosts the float32 mean's order differs
        want = g[f"S_r{red}"]
        assert S.dtype == np.float32 and S.shape == want.shape and S[0, 0] == 0, (name, red)
        assert np.abs(S.astype(np.float64) - want).max() <= PC.table_rtol(H, W) * np.abs(want).max(), (name, red)
    with pytest.raises(ValueError, match="W >= 2"):
        WP.ColorNoise().weights(4, 1)
    from wxengine.engine import WXEngineError
    with pytest.raises(WXEngineError, match="up to 4096 points a side"):
        WP.ColorNoise()._weights(5000, 8)


def test_hemispheric_weights(WP):
    g = PC.load_golden("p19x37", os.path.join(ROOT, "tests", "golden"))
    w = WP.hemispheric_weights(g["hemi_lat"], PC.HEMI["north"], PC.HEMI["south"])
    assert w.dtype == np.float32 and np.array_equal(w.view(np.int32), g["hemi_w"].view(np.int32))
    assert np.array_equal(WP.hemispheric_weights([90, 20, 0, -20, -90], 2.0, 4.0), np.array([2, 2, 3, 4, 4], dtype=np.float32))
    assert np.array_equal(WP.hemispheric_weights(g["hemi_lat"]), np.ones(19, dtype=np.float32))


def test_temporal_noise_arguments(WP):
    import torch
    gen = WP.ColorNoise(0.05, 2)
    tn = WP.TemporalNoise(gen)
    assert tn.temporal_correlation == 0.9 and tn.perturbation_std is None and tn._scale is None and tn.lat_weight is None
    assert np.array_equal(WP.TemporalNoise(gen, 0.5, 0.1)._scale, (torch.tensor([0.1]) / torch.tensor([0.05])).numpy())
    per = WP.TemporalNoise(gen, 0.5, torch.tensor([0.1, 0.02, 0.3]))
    x = types.SimpleNamespace(shape=(1, 3, 2, 5, 8), dim=lambda: 5)
    assert np.array_equal(per._chan_scale(x), np.repeat(per._scale, 2)) and per._chan_scale(x).dtype == np.float32
    assert np.array_equal(WP.TemporalNoise(gen, 0.5, 0.1)._chan_scale(x), np.full(6, np.float32(0.1) / np.float32(0.05), dtype=np.float32))
    from wxengine.engine import WXEngineError
    with pytest.raises(WXEngineError, match="perturbation_std has 3 channels"):
        per._chan_scale(types.SimpleNamespace(shape=(1, 4, 2, 5, 8), dim=lambda: 5))
    with pytest.raises(TypeError, match="noise_generator"):
        WP.TemporalNoise(object())
    with pytest.raises(ValueError, match="temporal_correlation"):
        WP.TemporalNoise(gen, float("inf"))
    with pytest.raises(ValueError, match="perturbation_std must be finite"):
        WP.TemporalNoise(gen, 0.9, torch.tensor([0.1, float("nan")]))
    with pytest.raises(ValueError, match="latitudes"):
        WP.TemporalNoise(gen, latitudes=np.zeros((2, 2)))
    with pytest.raises(TypeError):                       # seed and member are required keywords
        tn(None)
    assert "simply optional" in WP.TemporalNoise.__doc__


def test_calls_refuse_what_is_not_a_device_tensor(WP):
    import torch
    from wxengine.engine import WXEngineError
    for noise in (WP.GaussianNoise(), WP.ColorNoise()):
        for bad in (np.zeros((1, 2, 1, 5, 8), dtype=np.float32), torch.zeros((1, 2, 1, 5, 8)), torch.zeros(8)):
            with pytest.raises(WXEngineError, match="float32 CUDA tensor"):
                noise(bad)
    with pytest.raises(WXEngineError, match="float32 CUDA tensor"):
        WP.TemporalNoise(WP.GaussianNoise())(torch.zeros((1, 2, 1, 5, 8)), seed=0, member=0)


def test_perturbed_ensemble_rollout_validates_before_it_touches_the_engine(WP):
    import torch
    from wxengine.config import named_config
    from wxengine.rollout import perturbed_ensemble_rollout
    cfg = named_config("T0")
    engine = types.SimpleNamespace(cfg=cfg)               # any use of the engine itself would raise AttributeError
    x0 = torch.zeros((1, cfg.base_input_channels, cfg.frames, cfg.image_height, cfg.image_width))
    noise = WP.ColorNoise()
    for n in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="n_members"):
            perturbed_ensemble_rollout(engine, x0, [None], n, noise)
    with pytest.raises(ValueError, match="one entry per step"):
        perturbed_ensemble_rollout(engine, x0, [], 2, noise)
    with pytest.raises(TypeError, match="GaussianNoise or ColorNoise"):
        perturbed_ensemble_rollout(engine, x0, [None], 2, lambda x: x)
    with pytest.raises(TypeError, match="TemporalNoise"):
        perturbed_ensemble_rollout(engine, x0, [None], 2, noise, temporal=noise)
    with pytest.raises(ValueError, match="x0 must be a tensor of shape"):
        perturbed_ensemble_rollout(engine, x0[:, :-1], [None], 2, noise)
    for n in (0, cfg.base_input_channels + 1, 2.0):
        with pytest.raises(ValueError, match="n_perturbed"):
            perturbed_ensemble_rollout(engine, x0, [None], 2, noise, n_perturbed=n)


def test_slot_is_documented_where_the_generator_is():
    from wxengine.noise import SLOT_PERTURB
    assert SLOT_PERTURB == PC.SLOT == 16
    csrc = os.path.join(ROOT, "miles-credit_amd", "csrc")
    assert "SLOT_PERTURB = 16" in open(os.path.join(csrc, "wx_perturb.h")).read()
    assert "16 (SLOT_PERTURB" in open(os.path.join(csrc, "wx_noise.h")).read()
    assert "philox" not in open(os.path.join(csrc, "wx_perturb.h")).read().lower().replace("philox4x32-10", "").replace("the philox rounds", "")


def test_abi_symbols_are_exported():
    from wxengine import engine as E
    names = {"wx_perturb_create", "wx_perturb_destroy", "wx_perturb_batch", "wx_perturb_apply"}
    assert names <= set(E.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "wxengine.h")).read()
    assert all(f"int {n}(" in hdr for n in names)
    if os.path.exists(E.LIB_PATH):
        lib = E.load_library()
        assert all(hasattr(lib, n) for n in names)
        assert lib.wx_perturb_apply(None, 1, None, 0, 0, 0, 1.0, None, 0.0, None, 0, None, None, 0, None, 0, None, 0, None) == -1
        assert b"null perturbation handle" in lib.wx_last_error()
        assert lib.wx_perturb_create(5, 1, 1, None, 0, None) == -1 and b"null argument" in lib.wx_last_error()
