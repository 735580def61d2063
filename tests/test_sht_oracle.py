"""The numpy oracle of the spherical harmonic transforms (tests/sht_oracle.py) against scipy and against the mathematics: its three
tables against scipy.special.sph_harm_y and its diff_n=1 gradients on both grids, the Clenshaw-Curtis weights against exact monomial
integrals, round trip and Parseval on Gauss grids, the band-limited comparison on equiangular grids, the potentials of a scipy-built
wind, and the fixtures of tools/make_sht_goldens.py bit for bit.

scipy's gradient is (dY / dtheta, dY / dphi = i m Y): the table Qt = (m Pbar / sin theta) / sqrt(l (l + 1)) is compared after a
product with sin theta, which is also what makes the pole rows of the equiangular grid comparable.  There Qt itself is checked against
its limit: for m = 1 it equals +-dPt, for every other m it is zero.

On an equiangular grid the Clenshaw-Curtis quadrature is exact only for l + l' <= nlat - 1: a field band-limited to l < nlat // 2 is
recovered in those rows, while the rows beyond alias (comparing every row of a full-band field gives errors of 1e-2; that is the
mathematics, not a bug)."""
import os
import sys

import numpy as np
import pytest

scipy_special = pytest.importorskip("scipy.special")

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import sht_cases as SC  # noqa: E402
import sht_oracle as O  # noqa: E402

GRIDS = ("equiangular", "legendre-gauss")


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nlat", [8, 9, 33, 64])
def test_tables_against_scipy(grid, nlat):
    """Both recurrences in fp64: the bar is the size the longdouble yardstick gives the fp64 table's own error at these sizes
    (sht_cases.E_TAB, up to 6.2e-14 at nlat = 64), doubled for scipy's."""
    theta, _ = O.nodes(nlat, grid)
    lmax = nlat + 1
    t = O.tables(lmax, lmax, theta, csphase=True)
    bar = 4 * max(SC.E_TAB[(grid, nlat)], 2e-15)
    sin = np.sin(theta)
    for m in range(lmax):
        for l in range(m, lmax):
            y, g = scipy_special.sph_harm_y(l, m, theta, 0.0, diff_n=1)
            assert np.abs(t["P"][m, l] - y.real).max() <= bar
            if l > 0:
                norm = np.sqrt(l * (l + 1.0))
                assert np.abs(t["dP"][m, l] - g[:, 0].real / norm).max() <= bar and np.abs(t["Q"][m, l] * sin - g[:, 1].imag / norm).max() <= bar
    assert (t["P"][:, 0, :][1:] == 0).all() and (t["dP"][:, 0] == 0).all() and (t["Q"][:, 0] == 0).all() and (t["Q"][0] == 0).all()
    if grid == "equiangular":                                  # the poles: Qt -> dPt for m = 1 (north; its mirror sign south), 0 otherwise
        assert np.abs(t["Q"][1, :, 0] - t["dP"][1, :, 0]).max() <= bar and np.abs(np.abs(t["Q"][1, :, -1]) - np.abs(t["dP"][1, :, -1])).max() <= bar
        assert (np.abs(t["Q"][2:, :, 0]) <= bar).all() and (np.abs(t["Q"][2:, :, -1]) <= 64 * bar).all()
    off = O.tables(lmax, lmax, theta, csphase=False)
    sign = np.where(np.arange(lmax) % 2, -1.0, 1.0)[:, None, None]
    assert all(np.array_equal(off[n] * sign, t[n]) for n in O.TABLES)


@pytest.mark.parametrize("nlat", [2, 3, 8, 9, 33, 64])
def test_clenshaw_curtis_weights_integrate_monomials(nlat):
    theta, w = O.nodes(nlat, "equiangular")
    x = np.cos(theta)
    assert abs(w.sum() - 2.0) <= 8 * nlat * 2.0 ** -53 and (w > 0).all()
    for p in range(nlat):                                      # exact for degree <= nlat - 1
        exact = 0.0 if p % 2 else 2.0 / (p + 1)
        assert abs((w * x ** p).sum() - exact) <= 8 * nlat * 2.0 ** -53


@pytest.mark.parametrize("nlat,nlon", [(8, 16), (9, 16), (33, 64)])
def test_round_trip_and_parseval_on_gauss_grids(nlat, nlon):
    theta, w = O.nodes(nlat, "legendre-gauss")
    lmax, mmax = nlat, O.default_mmax(nlat, nlon)
    c = SC.coefficients(lmax, mmax, 2, 5)
    if 2 * (mmax - 1) == nlon:
        c[..., mmax - 1] = c[..., mmax - 1].real              # the Nyquist column of a real field
    x = O.synthesis(c, theta, nlon)
    back = O.analysis(x, theta, w, lmax, mmax)
    scale = np.abs(c).max()
    assert np.abs(back - c).max() <= 64 * (nlat + nlon) * 2.0 ** -53 * scale * np.sqrt(lmax)
    zonal, total = O.spectra(c)
    energy = 2 * np.pi / nlon * (x * x * w[:, None]).sum(axis=(-2, -1))
    keep = np.ones(mmax, dtype=bool)
    if 2 * (mmax - 1) == nlon:                                 # times_two counts the Nyquist column twice, the integral once
        keep[-1] = False
        energy = energy - (np.abs(c[..., -1]) ** 2).sum(axis=-1)
    assert np.abs(zonal[..., keep].sum(axis=-1) - energy).max() <= 1e-12 * energy.max()
    assert np.abs(zonal.sum(axis=-1) - total.sum(axis=-1)).max() <= 1e-13 * energy.max()


@pytest.mark.parametrize("nlat,nlon", [(9, 16), (33, 64), (37, 72)])
def test_equiangular_grids_recover_a_band_limited_field(nlat, nlon):
    theta, w = O.nodes(nlat, "equiangular")
    lmax, mmax = nlat, O.default_mmax(nlat, nlon)
    cut = nlat // 2
    c = SC.coefficients(lmax, mmax, 2, 6, lcut=cut)
    back = O.analysis(O.synthesis(c, theta, nlon), theta, w, lmax, mmax)
    assert np.abs(back[:, :cut] - c[:, :cut]).max() <= 64 * (nlat + nlon) * 2.0 ** -53 * np.abs(c).max() * np.sqrt(lmax)
    full = SC.coefficients(lmax, mmax, 2, 6)
    aliased = O.analysis(O.synthesis(full, theta, nlon), theta, w, lmax, mmax)
    assert np.abs(aliased - full).max() > 1e-4                 # beyond the band the analysis aliases


def test_scipy_built_wind_gives_its_potentials():
    import make_sht_goldens as G
    f = G.wind()
    assert f["err"] <= 64 * (16 + 32) * 2.0 ** -53 * max(np.abs(f["chi"]).max(), np.abs(f["psi"]).max()) * np.sqrt(12 * 13)
    nlat, nlon, grid, lmax, mmax = SC.geometry(SC.WIND_CASE)
    theta, w = O.nodes(nlat, grid)
    s, t = O.vector_analysis(f["u"], f["v"], theta, w, lmax, mmax)
    zs, zt = O.spectra(s)[0], O.spectra(t)[0]
    energy = 2 * np.pi / nlon * ((f["u"] ** 2 + f["v"] ** 2) * w[:, None]).sum(axis=(-2, -1))
    assert np.abs(zs.sum(axis=-1) + zt.sum(axis=-1) - energy).max() <= 1e-12 * energy.max()      # Parseval of the vector transform


def test_fixtures_reproduce_bit_for_bit():
    import make_sht_goldens as G
    built = G.build()
    for name, arrays in built.items():
        stored = np.load(os.path.join(SC.GOLD, name + ".npz"))
        assert set(stored.files) == set(arrays)
        for key, a in arrays.items():
            assert np.array_equal(stored[key], a), (name, key)
