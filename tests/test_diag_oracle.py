"""tests/diag_oracle.py (the torch restatement of csrc/wx_diag.h) against the reference's goldens (tests/golden/diag_*.npz, written by
tools/make_goldens.py --only diag from the reference's three post blocks in fp32 and fp64), and the host-side bookkeeping of
wxengine/diagnostics.py.  Every column of every fixture is compared; the distance is max |a - b| / max |b| per output variable."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import diag_oracle as O  # noqa: E402
from diag_cases import DIAG_CASES, GRIDS, case_inputs, distance, gate, load_golden, output_names  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in DIAG_CASES:
        g, f32, f64, d_ref = load_golden(name, GOLD)
        out[name] = (case_inputs(name, check=g), f32, f64, d_ref)
    return out


def test_fixtures_hold_what_they_claim(cases):
    for name, (inp, f32, f64, d_ref) in cases.items():
        c = DIAG_CASES[name]
        H, W = GRIDS[c["grid"]]
        assert inp["a_half"][-1 if c["s2t"] else 0] == 0 and inp["b_half"][-1 if c["s2t"] else 0] == 0    # the 0.57 Pa replacement runs
        assert f32["z_model"].shape == (c["B"], c["levels"], c["T"], H, W) and f32["mslp"].shape == (c["B"], 1, c["T"], H, W)
        assert inp["phis"].shape[2] == c["phis_T"]
        for v in output_names(name):
            if v.startswith("plev_"):
                assert f32[v].shape == (c["B"], len(c["plev"]), c["T"], H, W)
            # d_ref is the reference's own fp32-against-fp64 distance (the fp64 golden is stored as a float32 difference)
            assert d_ref[v] == pytest.approx(distance(f32[v], f64[v]), rel=1e-5)
    assert {c["levels"] for c in DIAG_CASES.values()} >= {2, 13, 16, 40} and any(c["s2t"] for c in DIAG_CASES.values())
    assert any(c["n_fields"] == 0 for c in DIAG_CASES.values()) and any(c["phis_T"] == 1 and c["T"] == 2 and c["B"] == 2 for c in DIAG_CASES.values())


@pytest.mark.parametrize("name", list(DIAG_CASES))
def test_oracle_fp64_matches_reference_fp64(cases, name):
    inp, _, f64, _ = cases[name]
    got = O.all_products(inp, DIAG_CASES[name], torch.float64)
    for v in output_names(name):
        assert got[v].shape == f64[v].shape
        # the fp64 golden is stored to ~1e-7 of its distance from the fp32 one (<= 2.3e-5): 1e-11 is summation-order room on top
        assert distance(got[v], f64[v]) <= 1e-11, (name, v, distance(got[v], f64[v]))


@pytest.mark.parametrize("name", list(DIAG_CASES))
def test_oracle_fp32_within_the_gate(cases, name):
    inp, f32, f64, d_ref = cases[name]
    got = O.all_products(inp, DIAG_CASES[name], torch.float32)
    for v in output_names(name):
        b32, b64 = gate(d_ref[v])
        d32, d64 = distance(got[v], f32[v]), distance(got[v], f64[v])
        print(f"[diag oracle fp32] {name} {v}: vs fp32 golden {d32:.2e} (<= {b32:.2e}), vs fp64 golden {d64:.2e} (<= {b64:.2e})")
        assert d32 <= b32 and d64 <= b64, (name, v, d32, d64)


def test_levels_subsetting_and_key_names():
    from wxengine.diagnostics import half_level_subset, mid_level_subset, pressure_output_key
    a, b = np.arange(10, dtype=np.float32) * 100, np.arange(10, dtype=np.float32) / 10
    ah, bh = half_level_subset(a, b, [3, 5, 6])
    assert list(ah) == [200.0, 400.0, 500.0, 600.0] and np.allclose(bh, [0.2, 0.4, 0.5, 0.6])   # [lv - 1 ...] + [levels[-1]]
    am, bm = mid_level_subset(a[:9], b[:9], [3, 5, 6])
    assert list(am) == [200.0, 400.0, 500.0] and np.allclose(bm, [0.2, 0.4, 0.5])
    assert half_level_subset(a, b, None)[0].shape == (10,) and mid_level_subset(a, b, None)[1].shape == (10,)
    assert pressure_output_key("ARCO_ERA5/prognostic/3d/temperature") == "ARCO_ERA5/derived_diagnostic/3d/temperature_PRES"
    assert pressure_output_key("era5/derived_diagnostic/3d/geopotential", "_P") == "era5/derived_diagnostic/3d/geopotential_P"


def test_constructor_signatures_follow_the_reference():
    import inspect
    from wxengine import diagnostics as D
    want = {
        D.GeopotentialDiagnostic: dict(output_name="ARCO_ERA5/derived_diagnostic/3d/geopotential", chunk_size=1000, flip_vertical=True,
                                       surface_geopotential_var="ARCO_ERA5/static/2d/geopotential_at_surface", key="y_processed",
                                       static_source_key="ic_raw", levels=None, model_a_half=None, model_b_half=None),
        D.PressureInterpDiagnostic: dict(pressure_levels=(500.0, 850.0), output_suffix="_PRES", temp_height=150.0, chunk_size=1000,
                                         geopotential_var="ARCO_ERA5/derived_diagnostic/3d/geopotential", key="y_processed",
                                         static_source_key="ic_raw", levels=None, model_a=None, model_b=None),
        D.MSLPDiagnostic: dict(output_name="ARCO_ERA5/derived_diagnostic/2d/mean_sea_level_pressure",
                               temperature_var="ARCO_ERA5/prognostic/2d/2m_temperature", key="y_processed", static_source_key="ic_raw"),
    }
    for cls, args in want.items():
        params = inspect.signature(cls.__init__).parameters
        for k, v in args.items():
            assert k in params and params[k].default == v, (cls.__name__, k)


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_no_gpu_fails_loudly_at_construction():
    from wxengine import diagnostics as D
    from wxengine.engine import WXDiag, WXEngineError
    a = np.zeros(4, np.float32)
    for make in (lambda: D.GeopotentialDiagnostic(model_a_half=a, model_b_half=a), lambda: D.MSLPDiagnostic(),
                 lambda: D.PressureInterpDiagnostic(model_a=a[:3], model_b=a[:3]),
                 lambda: D.PressureLevelProducts(model_a_half=a, model_b_half=a, model_a=a[:3], model_b=a[:3]), lambda: WXDiag(4, 4, 3)):
        with pytest.raises(WXEngineError):
            make()
