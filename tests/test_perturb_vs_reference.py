"""The fixtures of the perturbation noise against the live reference (credit/ensemble): ColorNoise, GaussianNoise and TemporalNoise on
the keyed tapes reproduce tests/golden/perturb_*.npz bit for bit, and the host mirror's tables (ColorNoise.weights,
hemispheric_weights) equal the reference's.  The reference's TemporalNoise reads its latitudes through xarray: a stand-in serves them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import perturb_cases as PC  # noqa: E402

pytestmark = pytest.mark.reference
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


@pytest.fixture(scope="module")
def ref():
    import make_perturb_goldens as MG
    return MG, MG.reference_modules()


@pytest.fixture()
def mirror(monkeypatch):
    """The host mirror's classes without a device: only the tables are asked for."""
    import wxengine.perturb as WP
    monkeypatch.setattr(WP._Noise, "_open", lambda self, device: None)
    return WP


@pytest.mark.parametrize("name,red", PC.FILTER_RUNS)
def test_live_colour_noise_reproduces_the_fixture_and_the_mirror_its_table(ref, mirror, name, red):
    MG, (RC, _, _, _) = ref
    g = PC.load_golden(name, GOLD)
    S, r32, r64 = MG.reference_filter(RC, red, PC.tape(name))
    assert np.array_equal(bits(S), bits(g[f"S_r{red}"]))
    assert np.array_equal(bits(r32), bits(g[f"ref32_r{red}"])) and np.array_equal(bits(r64), bits(g[f"ref64_r{red}"]))
    H, W = PC.PERTURB_CASES[name]["shape"][-2:]
    mine = mirror.ColorNoise(1.0, red).weights(H, W)
    assert mine.dtype == np.float32 and np.array_equal(bits(mine), bits(S))


def test_live_gaussian_temporal_and_rescale_reproduce_the_fixtures(ref, mirror):
    import torch
    MG, (RC, RG, RT, RU) = ref
    t = PC.TEMPORAL
    g = PC.load_golden(t["case"], GOLD)
    tape = PC.tape(t["case"])
    with MG.replay(torch.from_numpy(tape)):
        gauss = RG.GaussianNoise(amplitude=t["amplitude"])(torch.from_numpy(tape)).numpy()
    assert np.array_equal(bits(gauss), bits(g["gauss32"]))
    lat, w = MG.reference_hemi(RU, PC.HEMI)
    assert np.array_equal(bits(w), bits(g["hemi_w"])) and np.array_equal(bits(lat), bits(g["hemi_lat"]))
    mine = mirror.hemispheric_weights(lat, PC.HEMI["north"], PC.HEMI["south"])
    assert mine.dtype == np.float32 and np.array_equal(bits(mine), bits(w))
    assert set(np.unique(w)) >= {np.float32(1.0), np.float32(0.5), np.float32(0.75)}       # 20N, 20S and the equator are rows of the table
    state, delta = MG.reference_temporal(RC, RT, tape, PC.tape(t["case"], ".x"), PC.tape(t["case"], ".prev"), t, lat)
    assert np.array_equal(bits(state), bits(g["temporal_state"])) and np.array_equal(bits(delta), bits(g["temporal_delta"]))
    # the mirror's per-channel scale is the reference's perturbation_std / amplitude in float32
    tn = mirror.TemporalNoise(mirror.ColorNoise(t["amplitude"], t["reddening"]), t["rho"], torch.tensor(t["std"]), latitudes=lat)
    want = (torch.tensor(t["std"]) / torch.tensor([t["amplitude"]])).numpy()
    assert np.array_equal(bits(tn._scale), bits(want)) and np.array_equal(bits(tn.lat_weight), bits(np.ones(lat.size, dtype=np.float32)))
    # ... which, with the fixture's correlated noise, rebuilds the reference's delta in the epilogue's order of operations
    n = torch.from_numpy(g["ref32_r2"])
    sc = torch.from_numpy(tn._scale).view(1, -1, 1, 1, 1)
    rebuilt = (t["rho"] * torch.from_numpy(PC.tape(t["case"], ".prev")) + (t["amplitude"] * n) * sc) * torch.from_numpy(tn.lat_weight).view(1, 1, 1, -1, 1)
    assert np.array_equal(bits(rebuilt.numpy()), bits(g["temporal_delta"]))


def test_names_defaults_and_repr_are_the_references(ref, mirror):
    import inspect
    _, (RC, RG, RT, _) = ref
    for theirs, mine in ((RG.GaussianNoise, mirror.GaussianNoise), (RC.ColorNoise, mirror.ColorNoise)):
        a, b = inspect.signature(theirs.__init__).parameters, inspect.signature(mine.__init__).parameters
        for k, p in a.items():
            assert k in b and b[k].default == p.default, (theirs.__name__, k)
        assert repr(theirs()) == repr(mine()) and repr(theirs(amplitude=0.25)) == repr(mine(amplitude=0.25))
    assert repr(RC.ColorNoise(0.1, 3)) == repr(mirror.ColorNoise(0.1, 3))
    a, b = inspect.signature(RT.TemporalNoise.__init__).parameters, inspect.signature(mirror.TemporalNoise.__init__).parameters
    for k in ("noise_generator", "temporal_correlation", "perturbation_std"):
        assert list(a).index(k) == list(b).index(k) and a[k].default == b[k].default
    a, b = inspect.signature(RT.TemporalNoise.__call__).parameters, inspect.signature(mirror.TemporalNoise.__call__).parameters
    for k in ("x", "previous_perturbation", "forecast_step"):
        assert list(a).index(k) == list(b).index(k) and a[k].default == b[k].default
