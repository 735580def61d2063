"""tests/diag_oracle.py against the LIVE reference classes (credit/postblock/{geopotential,pressure_interp,mslp}.py) at the fixture
shapes; skipped where the reference tree is absent.  The classes read their coefficients through xarray, which is not installed: a
stand-in module serves the case's arrays, put in place with monkeypatch so it is undone."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import diag_oracle as O  # noqa: E402
from diag_cases import DIAG_CASES, FIELD_ORDER, KEYS, SRC, case_inputs, distance  # noqa: E402

pytestmark = pytest.mark.reference


@pytest.mark.parametrize("name", ["L16", "L13s2t", "L2bt", "L137"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_oracle_matches_live_reference_chain(monkeypatch, name, dtype):
    import oracle_stub
    oracle_stub.install()
    c, inp = DIAG_CASES[name], case_inputs(name)
    coef = dict(a_half=inp["a_half"], b_half=inp["b_half"], a_model=inp["a_mid"], b_model=inp["b_mid"])

    class _DS:
        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def __getitem__(self, key):
            return types.SimpleNamespace(values=coef[key])
    standin = types.ModuleType("xarray")
    standin.open_dataset = lambda _path, **_kw: _DS()
    import credit.postblock.geopotential as RG
    import credit.postblock.mslp as RM
    import credit.postblock.pressure_interp as RP
    monkeypatch.setitem(sys.modules, "xarray", standin)
    monkeypatch.setattr(RG, "xr", standin)
    monkeypatch.setattr(RP, "xr", standin)
    fields = [KEYS[f] for f in FIELD_ORDER[:c["n_fields"]]]
    t = {k: torch.from_numpy(inp[k]).to(dtype) for k in ("T", "q", "u", "v", "sp", "t2m", "phis")}
    batch = {"y_processed": {SRC: {KEYS[k]: t[k] for k in ("T", "q", "u", "v", "sp", "t2m")}},
             "ic_raw": {SRC: {KEYS["phis"]: t["phis"].expand(-1, -1, c["T"], -1, -1)}}}   # geopotential.py:205-209 does not expand PHIS
    with torch.no_grad():
        batch = RG.GeopotentialDiagnostic(output_name=KEYS["z"], surface_geopotential_var=KEYS["phis"], surface_pressure_var=KEYS["sp"],
                                          temperature_var=KEYS["T"], specific_humidity_var=KEYS["q"], flip_vertical=c["flip_vertical"])(batch)
        batch = RP.PressureInterpDiagnostic(pressure_levels=c["plev"], interp_variables=fields, temperature_var=KEYS["T"],
                                            geopotential_var=KEYS["z"], surface_pressure_var=KEYS["sp"],
                                            surface_geopotential_var=KEYS["phis"])(batch)
        batch = RM.MSLPDiagnostic(output_name=KEYS["mslp"], surface_pressure_var=KEYS["sp"], temperature_var=KEYS["t2m"],
                                  surface_geopotential_var=KEYS["phis"])(batch)
    y = batch["y_processed"][SRC]
    want = {"z_model": y[KEYS["z"]], "mslp": y[KEYS["mslp"]]}
    for f, k in [(f, KEYS[f]) for f in FIELD_ORDER[:c["n_fields"]]] + [("T", KEYS["T"]), ("Z", KEYS["z"])]:
        want[f"plev_{f}"] = y[f"{SRC}/derived_diagnostic/3d/{k.split('/')[-1]}_PRES"]
    got = O.all_products(inp, c, dtype)
    assert set(got) == set(want)
    for v, w in want.items():
        assert w.dtype == dtype and got[v].shape == tuple(w.shape)
        # same arithmetic in the same precision: summation-order room only
        assert distance(got[v], w.numpy()) <= (1e-12 if dtype == torch.float64 else 1e-6), (name, v)
