"""Writes tests/golden/sht_*.npz: what scipy contributes to the spherical harmonic transform tests, so that nothing marked gpu needs it.

    python tools/make_sht_goldens.py            # rewrites the fixtures; tests/test_sht_oracle.py checks that they reproduce bit for bit

  sht_tables.npz   Y_lm(theta, 0) and its gradient from scipy.special.sph_harm_y(diff_n=1) on both grids at nlat 8 and 9, lmax = nlat + 1:
                   P = Y, dP = (dY / dtheta) / sqrt(l (l + 1)), Qs = m Y / sqrt(l (l + 1)) (scipy's second component is dY / dphi = i m Y:
                   the table Qt times sin theta), [m][l][k], at the oracle's nodes
  sht_wind.npz     a wind u = grad chi + rhat x grad psi on the 16 x 32 Gauss grid from random potentials with l < 12, summed from scipy's
                   harmonics and gradients; err = the distance of the fp64 oracle's (s, t) from sqrt(l (l + 1)) (chi, psi)
  sht_small.npz    the oracle's own results on 9 x 16 (equiangular) and 8 x 16 (Gauss), lmax = nlat + 1: coefficients, synthesis, vector
                   parts and spectra -- what the reference-glue test compares the live credit/verification/standard.py with
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sht_cases as SC  # noqa: E402
import sht_oracle as O  # noqa: E402

TABLE_GRIDS = [(grid, nlat) for grid in ("equiangular", "legendre-gauss") for nlat in (8, 9)]
SMALL = {"e": ("equiangular", 9, 16), "g": ("legendre-gauss", 8, 16)}


def scipy_tables(grid, nlat):
    from scipy.special import sph_harm_y
    theta, _ = O.nodes(nlat, grid)
    lmax = nlat + 1
    out = {n: np.zeros((lmax, lmax, nlat)) for n in ("P", "dP", "Qs")}
    for m in range(lmax):
        for l in range(m, lmax):
            y, g = sph_harm_y(l, m, theta, 0.0, diff_n=1)
            out["P"][m, l] = y.real
            if l > 0:
                out["dP"][m, l] = g[:, 0].real / np.sqrt(l * (l + 1.0))
                out["Qs"][m, l] = g[:, 1].imag / np.sqrt(l * (l + 1.0))
    return out


def wind():
    from scipy.special import sph_harm_y
    nlat, nlon, grid, lmax, mmax = SC.geometry(SC.WIND_CASE)
    theta, w = O.nodes(nlat, grid)
    chi, psi = SC.coefficients(lmax, mmax, 2, 21), SC.coefficients(lmax, mmax, 2, 22)
    chi[:, 0] = 0
    psi[:, 0] = 0
    TH, PH = np.meshgrid(theta, 2 * np.pi * np.arange(nlon) / nlon, indexing="ij")
    uth, uph = np.zeros((2, nlat, nlon)), np.zeros((2, nlat, nlon))
    for l in range(1, lmax):
        for m in range(0, min(l, mmax - 1) + 1):
            _, g = sph_harm_y(l, m, TH, PH, diff_n=1)
            gt, gp = g[..., 0], g[..., 1] / np.sin(TH)
            f = 1.0 if m == 0 else 2.0
            for p in range(2):          # grad chi = (gt, gp);  rhat x grad psi = (-gp, gt)
                uth[p] += f * (chi[p, l, m] * gt - psi[p, l, m] * gp).real
                uph[p] += f * (chi[p, l, m] * gp + psi[p, l, m] * gt).real
    u, v = uph, -uth
    s, t = O.vector_analysis(u, v, theta, w, lmax, mmax)
    L = np.sqrt(np.arange(lmax) * (np.arange(lmax) + 1.0))[:, None]
    err = max(np.abs(s - L * chi).max(), np.abs(t - L * psi).max())
    return dict(u=u, v=v, chi=chi, psi=psi, err=np.float64(err))


def small():
    out = {}
    for key, (grid, nlat, nlon) in SMALL.items():
        theta, w = O.nodes(nlat, grid)
        lmax = nlat + 1
        mmax = O.default_mmax(lmax, nlon)
        rng = np.random.default_rng([31, nlat, nlon])
        x, u, v = rng.standard_normal((3, 2, nlat, nlon))
        c = O.analysis(x, theta, w, lmax, mmax)
        s, t = O.vector_analysis(u, v, theta, w, lmax, mmax, csphase=False)
        out.update({f"{key}_x": x, f"{key}_u": u, f"{key}_v": v, f"{key}_c": c, f"{key}_back": O.synthesis(c, theta, nlon), f"{key}_s": s,
                    f"{key}_t": t, f"{key}_zonal": O.zonal_spectrum(x, grid)})
        for ws in ("n", "m"):
            rot, div = O.div_rot_spectrum(u, v, grid, ws)
            out[f"{key}_rot_{ws}"], out[f"{key}_div_{ws}"] = rot.mean(axis=0), div.mean(axis=0)
    return out


def build():
    tables = {}
    for grid, nlat in TABLE_GRIDS:
        for n, a in scipy_tables(grid, nlat).items():
            tables[f"{grid}_{nlat}_{n}"] = a
    return {"sht_tables": tables, "sht_wind": wind(), "sht_small": small()}


if __name__ == "__main__":
    for name, arrays in build().items():
        path = os.path.join(SC.GOLD, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), "bytes")
