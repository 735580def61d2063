"""The grids, fields and error bars shared by the spherical harmonic transform tests (tests/test_sht_*.py) and by
tools/make_sht_goldens.py.  numpy only: nothing here imports scipy or the code under test."""
import os

import numpy as np

import sht_oracle as O

U = 2.0 ** -53
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# E_tab: the largest absolute difference between the fp64 tables (Pbar, dPt, Qt; lmax = nlat + 1, every order) and the same recurrence
# in np.longdouble, per grid and nlat -- measured by tests/test_sht_host.py, which asserts that the library's tables stay below these
# figures (they are the measurements, rounded up in the third digit).  nlat = 721: the orders 0, 1, 2, 359, 360, 720, 721.
E_TAB = {
    ("equiangular", 8): 6.92e-16, ("equiangular", 9): 5.15e-16, ("equiangular", 33): 2.25e-14, ("equiangular", 37): 1.76e-14,
    ("equiangular", 64): 4.66e-14, ("equiangular", 181): 7.29e-13, ("equiangular", 721): 8.07e-12,
    ("legendre-gauss", 8): 1.12e-15, ("legendre-gauss", 9): 1.66e-15, ("legendre-gauss", 16): 5.11e-15, ("legendre-gauss", 33): 1.32e-14, ("legendre-gauss", 64): 6.17e-14,
    ("legendre-gauss", 181): 3.34e-13, ("legendre-gauss", 721): 6.54e-12,
}

# name: (nlat, nlon, grid, lmax, mmax or None for min(lmax, nlon // 2 + 1))
GRID_CASES = {
    "e9x16": (9, 16, "equiangular", 9, None), "e9x16p": (9, 16, "equiangular", 10, None),              # below one MFMA tile, odd nlat
    "g8x16": (8, 16, "legendre-gauss", 8, None), "g8x16p": (8, 16, "legendre-gauss", 9, None),          # even nlat
    "e33x64": (33, 64, "equiangular", 33, None), "e33x64p": (33, 64, "equiangular", 34, None),          # equator row, ragged tiles
    "e37x72": (37, 72, "equiangular", 37, None), "e37x72p": (37, 72, "equiangular", 38, None),          # nlon no power of two
    "g64x128": (64, 128, "legendre-gauss", 64, None), "g64x128p": (64, 128, "legendre-gauss", 65, None),
    "e181x360": (181, 360, "equiangular", 181, None), "e181x360p": (181, 360, "equiangular", 182, None),   # indexing beyond small tiles
    "e33x64r": (33, 64, "equiangular", 20, 7),                                                         # a rectangular truncation
    # odd nlon: no Nyquist bin and no fold midpoint.  9 x 15: below one MFMA tile, mmax = 8; 37 x 75: Wh = 38 leaves the K loop a tail,
    # mmax = 37 two column blocks with the second partial
    "e9x15": (9, 15, "equiangular", 9, None), "e37x75": (37, 75, "equiangular", 37, None),
}
WIND_CASE = "g16x32w"                                       # the scipy-built wind of tests/golden/sht_wind.npz: not among the swept grids
ALL_CASES = dict(GRID_CASES, **{WIND_CASE: (16, 32, "legendre-gauss", 12, None)})


def geometry(name):
    nlat, nlon, grid, lmax, mmax = ALL_CASES[name]
    return nlat, nlon, grid, lmax, (O.default_mmax(lmax, nlon) if mmax is None else mmax)


def field(name, planes, seed=0, scale=250.0):
    """[planes, nlat, nlon] float64: a smooth part and noise, of the size of a temperature field."""
    nlat, nlon = ALL_CASES[name][:2]
    rng = np.random.default_rng([seed, nlat, nlon, planes])
    lat = np.linspace(-1.0, 1.0, nlat)[:, None]
    lon = 2 * np.pi * np.arange(nlon)[None, :] / nlon
    x = scale * (1.0 + 0.1 * lat * np.cos(2 * lon) + 0.02 * np.sin(5 * lon + 3 * lat))
    return x[None] + 0.05 * scale * rng.standard_normal((planes, nlat, nlon))


def coefficients(lmax, mmax, planes, seed=0, lcut=None):
    """[planes, lmax, mmax] complex128, zero where l < m (and where l >= lcut), real in column 0."""
    rng = np.random.default_rng([seed, lmax, mmax, planes])
    c = rng.standard_normal((planes, lmax, mmax)) + 1j * rng.standard_normal((planes, lmax, mmax))
    l, m = np.arange(lmax)[:, None], np.arange(mmax)[None, :]
    c = c * (l >= m) / (1.0 + l)
    c[..., 0] = c[..., 0].real
    if lcut is not None:
        c[:, lcut:] = 0
    return c


def row_mass(x):
    """A_k = (2 pi / nlon) sum_j |x[k][j]|: [..., nlat]."""
    return 2 * np.pi / x.shape[-1] * np.abs(np.asarray(x, dtype=np.float64)).sum(axis=-1)


def gamma(name, terms):
    """The relative size of the error of an fp64 sum of `terms` products in any order, doubled (the device and the oracle each make
    one), plus the table term 2 E_tab."""
    nlat, _, grid = ALL_CASES[name][:3]
    return (terms + 16) * U * 2 + 2 * E_TAB[(grid, nlat)]


NOISE_ROW = 4.0        # a table row whose every entry is within this many E_tab of zero holds rounding noise, not values


def analysis_bound(name, x, theta, w, csphase=True):
    """[..., lmax, mmax]: ((nlon + nlat + 16) 2^-53 2 + 2 E_tab) sum_k |w_k Pbar_lm(theta_k)| A_k with A_k = (2 pi / nlon) sum_j |x_kj|.
    One kind of row cannot be held to that: a row (l, m) of the table with max_k |Pbar_lm(theta_k)| <= NOISE_ROW E_tab is rounding
    noise throughout -- in these cases only l = nlat, m = 0 on a Gauss grid with lmax = nlat + 1, whose nodes are the roots of
    P_nlat (max |Pbar| = 0.8 to 1.2 E_tab there; the next smallest row of any table has 0.28).  The folded device table and the
    oracle's unfolded one carry different noise, so sum_k |w_k Pbar| A_k is 1e-26 against a difference of 2.4e-13 (8 x 16, lmax =
    9).  For such a row alone the table term is taken as what E_tab is, an absolute error of an entry: 2 E_tab sum_k |w_k| A_k."""
    nlat, nlon, grid, lmax, mmax = geometry(name)
    P = np.abs(O.tables(lmax, mmax, theta, csphase)["P"])
    e_tab = E_TAB[(grid, nlat)]
    bound = gamma(name, nlon + nlat) * np.einsum("mlk,...k->...lm", P * np.abs(w), row_mass(x))
    noise = (P.max(axis=-1) <= NOISE_ROW * e_tab).T & (np.arange(lmax)[:, None] >= np.arange(mmax)[None, :])      # [lmax][mmax]
    floor = 2 * e_tab * (np.abs(w) * row_mass(x)).sum(axis=-1)
    return np.where(noise, np.maximum(bound, floor[..., None, None]), bound)


def vector_bound(name, u, v, theta, w, csphase=True):
    """(spheroidal, toroidal) bounds: the analogue with |dPt| on one component and |Qt| on the other."""
    nlat, nlon, _, lmax, mmax = geometry(name)
    t = O.tables(lmax, mmax, theta, csphase)
    D, Q = np.abs(t["dP"]) * np.abs(w), np.abs(t["Q"]) * np.abs(w)
    au, av = row_mass(u), row_mass(v)
    g = gamma(name, 2 * (nlon + nlat))
    return (g * (np.einsum("mlk,...k->...lm", D, av) + np.einsum("mlk,...k->...lm", Q, au)),
            g * (np.einsum("mlk,...k->...lm", D, au) + np.einsum("mlk,...k->...lm", Q, av)))


def synthesis_bound(name, c, theta, csphase=True):
    """[..., nlat] (the same for every column): gamma(lmax + 2 mmax) sum_m mult_m sum_l |Pbar_lm(theta_k)| (|re c| + |im c|)."""
    nlat, nlon, _, lmax, mmax = geometry(name)
    T = np.abs(O.tables(lmax, mmax, theta, csphase)["P"])
    mult = np.full(mmax, 2.0)
    mult[0] = 1.0
    mag = (np.abs(c.real) + np.abs(c.imag)) * mult
    return gamma(name, lmax + 2 * mmax) * np.einsum("mlk,...lm->...k", T, mag)


def spectra_bound(c, dc):
    """(zonal, total) bounds of the spectra of coefficients c known to dc: the propagation 2 |c| dc + dc^2, plus the rounding of a sum
    of lmax (mmax) terms in an order of its own."""
    mult = np.full(c.shape[-1], 2.0)
    mult[0] = 1.0
    p = (2 * np.abs(c) * dc + dc * dc) * mult
    z, t = O.spectra(c)
    return p.sum(axis=-2) + (c.shape[-2] + 4) * 2 * U * z, p.sum(axis=-1) + (c.shape[-1] + 4) * 2 * U * t
