"""The reference's own filter, credit/pol_lapdiff_filt.py, run live over a stand-in torch_harmonics made of the numpy oracle
(tests/polefilter_oracle.py): diff_lap2d_filt on the 70-channel g24x144 tensor must reproduce the oracle's fixture.  This pins the
filtered rows, the cutoff index, the half-weight mode, the constants, the sub-step counts, the order (low-pass first, then the
sub-steps) and the channel map to the reference's code -- the only things about it that can be run without the library.

The stand-in follows the reference's evident meaning: slot 0 is toroidal (vrt), slot 1 spheroidal (div); the forward vector transform
divides by the extra sqrt(l (l + 1)) and the inverse multiplies by it, so that lap * radius * vsht is the divergence and getgrad the
gradient on the sphere of radius a.  Which convention the live library has cannot be checked here.

The reference's 3-D getgrad casts its coefficients to complex64, the oracle does not: the distance is measured, not fixed --
polefilter_cases.REFERENCE_DISTANCE records it (4.62e-08 on fields of 250 and increments of 7.6; 1.4e-13 on the channels of the fp64 2-D path), the test allows 8 times that and
requires the allowance to stay below 1e-3 of the largest increment.  Were it larger, the glue would be wrong, not the precision."""
import importlib
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import polefilter_cases as PC  # noqa: E402
import polefilter_oracle as PO  # noqa: E402
import sht_oracle as O  # noqa: E402

pytestmark = pytest.mark.reference


@pytest.fixture()
def reference(monkeypatch):
    import torch
    made = {}

    def geometry(nlat, nlon, lmax, mmax, grid):
        key = (nlat, nlon, lmax, mmax, grid)
        if key not in made:
            made[key] = PO.Geometry(nlat, nlon, grid, lmax, mmax)
        return made[key]

    class Base:
        def __init__(self, nlat, nlon, lmax=None, mmax=None, grid="equiangular", norm="ortho", csphase=True):
            assert norm == "ortho" and csphase is False
            self.G = geometry(nlat, nlon, lmax, mmax, grid)
            self.lmax, self.mmax = self.G.lmax, self.G.mmax

        def to(self, device):
            return self

    class RealSHT(Base):
        def __call__(self, x):
            return torch.from_numpy(self.G.analysis(x.numpy()))

    class InverseRealSHT(Base):
        def __call__(self, c):
            return torch.from_numpy(self.G.synthesis(c.numpy()))

    class RealVectorSHT(Base):
        def __call__(self, uv):
            s, t = self.G.vector_analysis(uv[..., 0, :, :].numpy(), uv[..., 1, :, :].numpy())
            inv = np.zeros_like(self.G.sq)
            inv[1:] = 1.0 / self.G.sq[1:]
            return torch.from_numpy(np.stack((t * inv, s * inv), axis=-3))

    class InverseRealVectorSHT(Base):
        def __call__(self, c):
            c = c.numpy().astype(np.complex128)
            u, v = self.G.vector_synthesis(self.G.sq * c[..., 1, :, :], self.G.sq * c[..., 0, :, :])
            return torch.from_numpy(np.stack((u, v), axis=-3))

    def legendre_gauss_weights(n, a=-1.0, b=1.0):
        theta, w = O.gauss_nodes(n)
        return np.cos(theta)[::-1].copy(), w[::-1].copy()

    fake = types.ModuleType("torch_harmonics")
    fake.RealSHT, fake.InverseRealSHT, fake.RealVectorSHT, fake.InverseRealVectorSHT = RealSHT, InverseRealSHT, RealVectorSHT, InverseRealVectorSHT
    fake.quadrature = types.SimpleNamespace(legendre_gauss_weights=legendre_gauss_weights)
    monkeypatch.setitem(sys.modules, "torch_harmonics", fake)
    monkeypatch.syspath_prepend("/root/reference")
    sys.modules.pop("credit.pol_lapdiff_filt", None)
    mod = importlib.import_module("credit.pol_lapdiff_filt")
    yield mod
    sys.modules.pop("credit.pol_lapdiff_filt", None)


def test_sig_and_cutoff_index_are_the_live_functions(reference):
    import torch
    from wxengine import pole_filter as PF
    for nlat in (21, 24, 33, 181, 640, 721):
        live = reference.create_sigmoid_ramp_function(nlat, 10).numpy()
        assert live.dtype == np.float32
        assert np.array_equal(PF.create_sigmoid_ramp_function(nlat, 10), live) and np.array_equal(PO.sigmoid_ramp(nlat), live)
    for nlon, want in ((128, 0), (136, 1), (144, 1), (160, 1), (256, 2), (360, 3), (1280, 12), (1440, 13)):
        perd = 1 / torch.fft.rfftfreq(nlon)[1:]
        live = int(reference.find_nearest(perd, value=100)[1])
        assert live == want == PF.cutoff_index(nlon) == PO.cutoff_index(nlon), nlon


def test_the_live_low_pass_is_the_oracle_s(reference):
    import torch
    x = PC.temperature("g32x256", 2)
    for a in (x, x[0]):
        live = reference.polfiltT(torch.from_numpy(a.copy()), 10).numpy()
        want = PO.polfilt_fft(a, 2)
        assert np.abs(live - want).max() <= 64 * 2.0 ** -53 * np.abs(a).max()
        rows = PC.filtered_rows(32)
        assert rows == list(range(1, 11)) + list(range(22, 32))
        keep = [k for k in range(32) if k not in rows]
        assert np.array_equal(live[..., keep, :], a[..., keep, :]) and not np.array_equal(live[..., 31, :], a[..., 31, :])


def test_the_live_diff_lap2d_filt_gives_the_fixture(reference):
    import torch
    nlat, nlon, grid = PC.FILTER_CASES[PC.DIFF_CASE][:3]
    dpf = reference.Diffusion_and_Pole_Filter(nlat=nlat, nlon=nlon, device="cpu", grid=grid, radius=PC.radius(nlat))
    assert (dpf.lmax, dpf.mmax, dpf.indpol) == (nlat, O.default_mmax(nlat, nlon), 10)
    B = PC.diff_tensor()
    live = dpf.diff_lap2d_filt(torch.from_numpy(B.copy())).numpy()
    want = np.concatenate([np.load(os.path.join(PC.GOLD, f))["expected"] for f in PC.DIFF_FILES])
    assert live.shape == want.shape == (70, nlat, nlon)
    d = np.abs(live - want).max(axis=(1, 2))
    print("distance of the live reference from the fixture per channel group:", d[:32].max(), d[32:64].max(), d[64:].max())
    bar = 8 * PC.REFERENCE_DISTANCE
    assert bar <= 1e-3 * PC.INCREMENT_DIFF
    assert d.max() <= bar, (d.max(), bar)
    # the channels of the 2-D path (64 .. 69) are never cast to complex64: fp64 against fp64
    assert d[64:].max() <= 64 * PC.E_REF_DIFF
