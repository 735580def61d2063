"""The reference's own spectra code, credit/verification/standard.py, run live with a stand-in torch_harmonics whose RealSHT and
RealVectorSHT are the numpy oracle (tests/sht_oracle.py): what it returns for a tiny xarray-like object must be the fixtures of
tools/make_sht_goldens.py, which the oracle's zonal_spectrum / div_rot_spectrum made.  This pins lmax = nlat + 1, times_two and the
summed axis to the reference's code -- the only thing about the reference's spherical harmonics that can be run without the library.
The stand-in puts the toroidal coefficients in slot 0 and the spheroidal in slot 1, the reference's own naming (vrt, div); which slot
the live library fills with which cannot be checked here and is why wxengine.sht names its results."""
import importlib
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import sht_cases as SC  # noqa: E402
import sht_oracle as O  # noqa: E402

pytestmark = pytest.mark.reference


@pytest.fixture()
def standard(monkeypatch):
    import torch

    class RealSHT:
        def __init__(self, nlat, nlon, lmax=None, mmax=None, grid="equiangular", norm="ortho", csphase=True):
            assert norm == "ortho"
            self.nlat, self.nlon, self.grid, self.csphase = nlat, nlon, grid, csphase
            self.lmax = lmax or nlat
            self.mmax = mmax or O.default_mmax(self.lmax, nlon)

        def __call__(self, x):
            theta, w = O.nodes(self.nlat, self.grid)
            return torch.from_numpy(O.analysis(x.numpy(), theta, w, self.lmax, self.mmax, self.csphase))

    class RealVectorSHT(RealSHT):
        def __call__(self, uv):
            theta, w = O.nodes(self.nlat, self.grid)
            s, t = O.vector_analysis(uv[..., 0, :, :].numpy(), uv[..., 1, :, :].numpy(), theta, w, self.lmax, self.mmax, self.csphase)
            return torch.from_numpy(np.stack((t, s), axis=-3))

    fake = types.ModuleType("torch_harmonics")
    fake.RealSHT, fake.RealVectorSHT = RealSHT, RealVectorSHT
    monkeypatch.setitem(sys.modules, "torch_harmonics", fake)
    monkeypatch.syspath_prepend("/root/reference")
    sys.modules.pop("credit.verification.standard", None)
    mod = importlib.import_module("credit.verification.standard")
    yield mod
    sys.modules.pop("credit.verification.standard", None)


class Values:
    def __init__(self, values):
        self.values = values


class Data:
    def __init__(self, nlat, nlon, values=None, U=None, V=None):
        self.latitude, self.longitude, self.values = np.zeros(nlat), np.zeros(nlon), values
        self.U, self.V = Values(U), Values(V)


@pytest.mark.parametrize("key", ["e", "g"])
def test_the_reference_functions_give_the_fixtures(standard, key):
    g = np.load(os.path.join(SC.GOLD, "sht_small.npz"))
    grid = {"e": "equiangular", "g": "legendre-gauss"}[key]
    x, u, v = g[f"{key}_x"], g[f"{key}_u"], g[f"{key}_v"]
    nlat, nlon = x.shape[-2:]
    zonal = standard.zonal_spectrum(Data(nlat, nlon, values=x), grid).numpy()
    assert zonal.shape == g[f"{key}_zonal"].shape == (2, O.default_mmax(nlat + 1, nlon))
    tol = 64 * (nlat + nlon) * 2.0 ** -53                       # two fp64 evaluations of one sum in different orders
    assert np.abs(zonal - g[f"{key}_zonal"]).max() <= tol * g[f"{key}_zonal"].max()
    assert np.abs(standard.average_zonal_spectrum(Data(nlat, nlon, values=x), grid) - g[f"{key}_zonal"].mean(axis=0)).max() <= tol * g[f"{key}_zonal"].max()
    for ws in ("n", "m"):
        rot, div = standard.average_div_rot_spectrum(Data(nlat, nlon, U=u, V=v), grid, wave_spec=ws)
        assert rot.shape == g[f"{key}_rot_{ws}"].shape and np.abs(rot - g[f"{key}_rot_{ws}"]).max() <= tol * g[f"{key}_rot_{ws}"].max()
        assert np.abs(div - g[f"{key}_div_{ws}"]).max() <= tol * g[f"{key}_div_{ws}"].max()
    if key == "g":                                             # the row l = nlat of m = 0 on a Gauss grid: zero up to rounding
        c = g["g_c"]
        assert np.abs(c[:, nlat, 0]).max() <= 1e-13 * np.abs(c).max() and np.abs(c[:, nlat - 1, 0]).max() > 1e-3 * np.abs(c).max()
