"""The grids, fields and error bars shared by the diffusion and pole filter tests (tests/test_polefilter_*.py) and by
tools/make_polefilter_goldens.py.  numpy only: nothing here imports the code under test.

The grids are the smallest at which each code path can still go wrong:
    g24x144   Gauss, cutoff 1: even nlat, folded; only the mean and the half-weight mode survive the low-pass
    e33x160   equiangular, cutoff 1: odd nlat, the equator row unfolded; the parity of dPt
    g32x256   Gauss, cutoff 2: one full mode plus the half mode
    e21x136   equiangular, cutoff 1: the minimum nlat, the two polar bands touch
    g24x144r  Gauss, cutoff 1, lmax 16, mmax 9: a rectangular truncation
    g24x128   Gauss, cutoff 0: the low-pass is the identity
    g8x16, e9x16   below one MFMA tile: the vector synthesis alone (the filter refuses nlat < 21)
The radius is a = 14142 nlat, so that 1e8 lmax^2 / a^2 = 2e16 lmax^4 / a^4 = 0.5: half the explicit schemes' stability limit (the real
640-row grid sits at 1.0 and 2.0).  At the Earth's radius the increments of a small grid vanish below rounding."""
import os

import numpy as np

import polefilter_oracle as PO
import sht_oracle as O

U = 2.0 ** -53
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLD_PLANES = 2
SUBSTEPS = {"V1": 5, "QV1": 8, "V2": 6}

# name: (nlat, nlon, grid, lmax or None for nlat, mmax or None for min(lmax, nlon // 2 + 1), the cutoff index of the low-pass)
FILTER_CASES = {
    "g24x144": (24, 144, "legendre-gauss", None, None, 1),
    "e33x160": (33, 160, "equiangular", None, None, 1),
    "g32x256": (32, 256, "legendre-gauss", None, None, 2),
    "e21x136": (21, 136, "equiangular", None, None, 1),
    "g24x144r": (24, 144, "legendre-gauss", 16, 9, 1),
    "g24x128": (24, 128, "legendre-gauss", None, None, 0),
}
SYNTHESIS_CASES = dict(FILTER_CASES, g8x16=(8, 16, "legendre-gauss", None, None, 0), e9x16=(9, 16, "equiangular", None, None, 0))
DIFF_CASE = "g24x144"
DIFF_FILES = ("polefilter_diff_a.npz", "polefilter_diff_b.npz")      # the expected channels 0:35 and 35:70 (the size limit of a file)

# E_tab: the largest absolute difference between the fp64 tables (Pbar, dPt, Qt; csphase off, the case's lmax and mmax) and the same
# recurrence in np.longdouble -- measured by tools/make_polefilter_goldens.py, rounded up in the third digit.
E_TAB = {
    "g24x144": 1.05e-14, "e33x160": 2.25e-14, "g32x256": 1.32e-14, "e21x136": 1.13e-14, "g24x144r": 4.07e-15, "g24x128": 1.05e-14,
    "g8x16": 1.09e-15, "e9x16": 5.15e-16,
}

# E_ref: the largest absolute difference between the fp64 oracle's result and the same chain in np.longdouble, per case and variant,
# on the fixture's inputs -- measured by tools/make_polefilter_goldens.py, rounded up in the third digit.  The device may differ
# from the fp64 oracle by 16 E_ref: both sum 17 to 25 chained transforms in an order of their own, and each can sit as far from
# exact as the other.  INCREMENT: the largest |output - low-pass(input)| of the same runs, what the sub-steps alone add; the bar must
# stay below 1e-6 of it, so that a wrong term, sign or row cannot hide.
E_REF = {
    ("g24x144", "V1"): 5.20e-13, ("g24x144", "QV1"): 3.99e-13, ("g24x144", "V2"): 1.75e-14,
    ("e33x160", "V1"): 1.03e-12, ("e33x160", "QV1"): 8.73e-13, ("e33x160", "V2"): 2.18e-14,
    ("g32x256", "V1"): 5.87e-13, ("g32x256", "QV1"): 5.42e-13, ("g32x256", "V2"): 2.15e-14,
    ("e21x136", "V1"): 4.57e-13, ("e21x136", "QV1"): 3.87e-13, ("e21x136", "V2"): 2.51e-14,
    ("g24x144r", "V1"): 1.82e-13, ("g24x144r", "QV1"): 1.75e-13, ("g24x144r", "V2"): 1.27e-14,
    ("g24x128", "V1"): 6.04e-13, ("g24x128", "QV1"): 4.81e-13, ("g24x128", "V2"): 2.02e-14,
}
INCREMENT = {                                               # of the sub-steps alone: |output - low-pass(input)|
    ("g24x144", "V1"): 6.762, ("g24x144", "QV1"): 5.841, ("g24x144", "V2"): 1.682,
    ("e33x160", "V1"): 7.201, ("e33x160", "QV1"): 6.286, ("e33x160", "V2"): 1.824,
    ("g32x256", "V1"): 6.366, ("g32x256", "QV1"): 5.477, ("g32x256", "V2"): 1.660,
    ("e21x136", "V1"): 0.712, ("e21x136", "QV1"): 0.612, ("e21x136", "V2"): 0.242,
    ("g24x144r", "V1"): 2.291, ("g24x144r", "QV1"): 1.878, ("g24x144r", "V2"): 0.363,
    ("g24x128", "V1"): 6.518, ("g24x128", "QV1"): 5.641, ("g24x128", "V2"): 1.932,
}
E_REF_DIFF, INCREMENT_DIFF = 5.21e-13, 7.642

# The live reference (credit/pol_lapdiff_filt.py over the oracle as a stand-in torch_harmonics) casts the coefficients of its 3-D
# getgrad to complex64: its distance from the fp64 oracle on the 70-channel g24x144 tensor, as measured by
# tests/test_polefilter_reference.py.  That test allows 8 times this and requires it to stay below 1e-3 of the largest increment.
REFERENCE_DISTANCE = 4.62e-08


def radius(nlat):
    return 14142.0 * nlat


def geometry(name, dtype=np.float64):
    nlat, nlon, grid, lmax, mmax, _ = SYNTHESIS_CASES[name]
    return PO.Geometry(nlat, nlon, grid, lmax, mmax, radius(nlat), dtype)


def _smooth(nlat, nlon, a, b):
    lat = np.linspace(-1.0, 1.0, nlat)[:, None]
    lon = 2 * np.pi * np.arange(nlon)[None, :] / nlon
    return a * lat * np.cos(2 * lon) + b * np.sin(5 * lon + 3 * lat)


def temperature(name, planes, seed=0):
    """[planes, nlat, nlon] float64: 250 +- 25 plus noise of 5."""
    nlat, nlon = SYNTHESIS_CASES[name][:2]
    rng = np.random.default_rng([seed, nlat, nlon, planes, 1])
    return 250.0 + _smooth(nlat, nlon, 20.0, 5.0)[None] + 5.0 * rng.standard_normal((planes, nlat, nlon))


def wind(name, planes, seed=0):
    """(u, v), each [planes, nlat, nlon] float64: a jet of 20, a wave of 5 and noise of 2."""
    nlat, nlon = SYNTHESIS_CASES[name][:2]
    rng = np.random.default_rng([seed, nlat, nlon, planes, 2])
    lat = np.linspace(-1.0, 1.0, nlat)[:, None]
    u = 20.0 * (1 - lat * lat) + _smooth(nlat, nlon, 5.0, 2.0)
    v = _smooth(nlat, nlon, -3.0, 5.0)
    return u[None] + 2.0 * rng.standard_normal((planes, nlat, nlon)), v[None] + 2.0 * rng.standard_normal((planes, nlat, nlon))


def diff_tensor(seed=7):
    """The 70-channel tensor of diff_lap2d_filt on DIFF_CASE in the reference's layout: winds in 0:32 and 66:68, temperature-like else."""
    u, v = wind(DIFF_CASE, 17, seed)
    t = temperature(DIFF_CASE, 36, seed)
    B = np.empty((70,) + t.shape[1:])
    B[0:16], B[16:32], B[67], B[66] = u[:16], v[:16], u[16], v[16]
    B[32:66], B[68:70] = t[:34], t[34:]
    return B


def coefficients(name, planes, seed=0, lcut=None):
    """[planes, lmax, mmax] complex128, zero where l < m (and where l >= lcut), real in column 0."""
    G = SYNTHESIS_CASES[name]
    lmax = G[0] if G[3] is None else G[3]
    mmax = O.default_mmax(lmax, G[1]) if G[4] is None else G[4]
    rng = np.random.default_rng([seed, lmax, mmax, planes, 3])
    c = rng.standard_normal((planes, lmax, mmax)) + 1j * rng.standard_normal((planes, lmax, mmax))
    l, m = np.arange(lmax)[:, None], np.arange(mmax)[None, :]
    c = c * (l >= m) / (1.0 + l)
    c[..., 0] = c[..., 0].real
    if lcut is not None:
        c[:, lcut:] = 0
    return c


def vector_synthesis_bound(name, G, s, t=None, lscale=None):
    """[..., nlat] (the same for every column and for both components): the analogue of sht_cases.synthesis_bound with |dPt| + |Qt| in
    place of |Pbar| -- ((2 lmax + 2 mmax + 16) 2^-53 2 + 2 E_tab) sum_m mult_m sum_l (|dPt| + |Qt|) |lscale_l| (|re s| + |im s| + |re t| + |im t|):
    a sum of 2 lmax products per bin and 2 mmax per column, in any order, the device and the oracle each making one; the table term."""
    T = np.abs(G.tab["dP"]) + np.abs(G.tab["Q"])
    mult = np.full(G.mmax, 2.0)
    mult[0] = 1.0
    mag = np.abs(s.real) + np.abs(s.imag)
    if t is not None:
        mag = mag + np.abs(t.real) + np.abs(t.imag)
    if lscale is not None:
        mag = mag * np.abs(lscale)[:, None]
    gamma = (2 * G.lmax + 2 * G.mmax + 16) * U * 2 + 2 * E_TAB[name]
    return gamma * np.einsum("mlk,...lm->...k", T, mag * mult)


def lowpass_bound(x, i):
    """[..., nlat]: 2 (i + 1) (nlon + 16) 2^-53 sum_j |x_kj| / nlon for a filtered row.  With S = sum_j |x_j|, a cosine or sine sum of
    nlon products, each twiddle good to a few ulp, is off by at most (nlon + 16) 2^-53 S in any order; the rebuilt row adds i + 1
    modes, each with weight at most 2 / nlon -- the constant is 2 (i + 1) (nlon + 16) 2^-53 / nlon times S.  The oracle's own FFT
    error, O(log nlon) 2^-53 S / nlon per mode, is within the 16."""
    nlon = x.shape[-1]
    return 2.0 * (i + 1) * (nlon + 16) * U * np.abs(x).sum(axis=-1) / nlon


def filtered_rows(nlat, inddo=PO.INDPOL):
    return sorted(set(int(r) % nlat for r in np.concatenate([np.arange(-inddo, 0), np.arange(1, inddo + 1)])))
