"""The advection fixtures against the LIVE reference (credit/postblock/advect.py); skipped where the reference tree is absent.  The
regenerated inputs hash to the fixture's, the reference's class reproduces the stored fp32 goldens bit for bit and, on double tensors,
the stored fp64 goldens (kept as float32 differences from the fp32 ones: to the rounding of that difference).  The class reads its
coefficients and coordinates through xarray: a stand-in module serves the case's arrays, `get_meta_file_path` is the identity."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from advect_cases import ADVECT_CASES, KEYS, SRC, block_args, case_inputs, load_golden  # noqa: E402

pytestmark = pytest.mark.reference
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def reference():
    import oracle_stub
    oracle_stub.install()
    coef = {}
    before = sys.modules.get("xarray")
    standin = oracle_stub.serve_xarray(coef)
    import credit.postblock.advect as RA
    keep = RA.xr, RA.get_meta_file_path
    RA.xr, RA.get_meta_file_path = standin, (lambda path: path)
    yield RA, coef
    RA.xr, RA.get_meta_file_path = keep
    if before is None:
        del sys.modules["xarray"]
    else:
        sys.modules["xarray"] = before


@pytest.mark.parametrize("name", list(ADVECT_CASES))
def test_reference_reproduces_the_stored_goldens(reference, name):
    RA, coef = reference
    g, f32, f64, _ = load_golden(name, GOLD)
    inp = case_inputs(name, check=g)             # the hashes
    a = block_args(name)
    coef.update(a_half=a.pop("model_a_half"), b_half=a.pop("model_b_half"), latitude=a.pop("latitude"), longitude=a.pop("longitude"))
    blk = RA.SemiLagrangianAdvectionPost(**a)
    for dtype in (torch.float32, torch.float64):
        with torch.no_grad():
            y = blk({"y_processed": {SRC: {KEYS[k]: torch.from_numpy(inp[k]).to(dtype) for k in inp}}})["y_processed"][SRC]
        for t in ADVECT_CASES[name]["tracers"]:
            got = y[KEYS[t]].numpy()
            if dtype == torch.float32:
                assert np.array_equal(got, f32[t]), (name, t)
            else:
                stored = np.abs(f64[t] - f32[t].astype(np.float64)) * 2.0 ** -24       # the rounding of the stored float32 difference
                assert (np.abs(got - f64[t]) <= 1e-12 * max(1.0, np.abs(got).max()) + stored).all(), (name, t)
