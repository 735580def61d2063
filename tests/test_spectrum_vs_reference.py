"""The fixtures of the zonal spectra against the live reference classes (credit/losses/gen_1/power.py::PSDLoss, spectral.py::
SpectralLoss2D): what tools/make_spectrum_goldens.py stored is what the classes give here, bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import spectrum_cases as SC  # noqa: E402

pytestmark = pytest.mark.reference
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def tool():
    import make_spectrum_goldens as tool
    return tool, tool.reference_modules()


@pytest.mark.parametrize("name", list(SC.SPECTRUM_CASES))
def test_live_reference_reproduces_the_fixture(tool, name):
    tool, (RP, RS) = tool
    g = SC.load_golden(name, GOLD)
    pred, target = SC.fields(name)
    psd32, psd64, loss32 = tool.reference_case(RP, RS, pred, target, SC.weights(name), SC.SPECTRUM_CASES[name]["k_init"])
    assert np.array_equal(psd32.view(np.int32), g["psd32"].view(np.int32))
    assert np.array_equal(psd64.view(np.int64), g["psd64"].view(np.int64))
    assert np.array_equal(loss32.view(np.int32), g["loss32"].view(np.int32))
