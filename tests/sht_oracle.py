"""numpy fp64 oracle of the spherical harmonic transforms of csrc/wx_sht.h: the mathematics restated, nothing shared with the code
under test (not its nodes, not its tables, no fold).

Unit sphere.  Row k has colatitude theta_k ascending (north first), column j has phi_j = 2 pi j / nlon.  Pbar_l^m(theta), 0 <= m <
mmax, m <= l < lmax, is normalised so that 2 pi int Pbar_l^m Pbar_l'^m sin(theta) dtheta = delta_ll' (Pbar_0^0 = 1 / sqrt(4 pi)) and
carries no Condon-Shortley sign; csphase=True multiplies odd m by -1.  Tables come from the three-term recurrence in l seeded along
the diagonal, in the dtype asked for (np.float64, or np.longdouble as the yardstick of the fp64 tables).

    analysis    F_m(k) = (2 pi / nlon) sum_j x[k][j] e^{-2 pi i m j / nlon};  c[l][m] = sum_k w_k Pbar_l^m(theta_k) F_m(k)
    synthesis   F_m(k) = sum_l Pbar_l^m(theta_k) c[l][m];  x[k][j] = sum_m F_m(k) e^{+2 pi i m j / nlon} with irfft's Hermitian
                completion (the imaginary parts of m = 0 and of the Nyquist bin of an even nlon are ignored)
    vector      u east, v north: u_phi = u, u_theta = -v;  Psi_lm = grad Y_lm / sqrt(l (l + 1)), Phi_lm = rhat x Psi_lm
                spheroidal s_lm = int u . conj(Psi_lm) dOmega = sum_k w_k (dPt F^theta - i Qt F^phi)
                toroidal   t_lm = int u . conj(Phi_lm) dOmega = sum_k w_k (dPt F^phi + i Qt F^theta)
                dPt = (dPbar / dtheta) / sqrt(l (l + 1)),  Qt = (m Pbar / sin theta) / sqrt(l (l + 1)),  row l = 0 is zero
    spectra     mult_m = 1 for m = 0 and 2 otherwise (the Nyquist column too: the reference's times_two)
                zonal[m] = sum_l mult_m |c_lm|^2,  total[l] = sum_m mult_m |c_lm|^2
The two derivative tables use the ladder identities, which hold at the poles as well (no division by sin theta):
    dPbar_l^m / dtheta    = ( sqrt((l + m)(l - m + 1)) Pbar_l^{m-1} - sqrt((l - m)(l + m + 1)) Pbar_l^{m+1} ) / 2,  m = 0: -sqrt(l (l + 1)) Pbar_l^1
    m Pbar_l^m / sin theta = sqrt((2l + 1) / (2l - 1)) ( sqrt((l - m)(l - m - 1)) Pbar_{l-1}^{m+1} + sqrt((l + m)(l + m - 1)) Pbar_{l-1}^{m-1} ) / 2
"""
import numpy as np

TABLES = ("P", "dP", "Q")


def gauss_nodes(nlat):
    x, w = np.polynomial.legendre.leggauss(nlat)
    return np.arccos(x[::-1]), w[::-1].copy()


def clenshaw_curtis_nodes(nlat):
    """theta_k = pi k / (nlat - 1) and the Clenshaw-Curtis weights of int dx on [-1, 1], by the cosine-sum formula."""
    n = nlat - 1
    theta = np.pi * np.arange(nlat) / n
    w = np.zeros(nlat)
    for k in range(nlat):
        s = 0.0
        for j in range(1, n // 2 + 1):
            b = 1.0 if 2 * j == n else 2.0
            s += b / (4.0 * j * j - 1.0) * np.cos(2.0 * j * theta[k])
        w[k] = (1.0 if k in (0, n) else 2.0) / n * (1.0 - s)
    return theta, w


def nodes(nlat, grid):
    if grid == "legendre-gauss":
        return gauss_nodes(nlat)
    if grid == "equiangular":
        return clenshaw_curtis_nodes(nlat)
    raise ValueError(grid)


def legendre_order(m, lmax, theta, dtype=np.float64):
    """Pbar_l^m[l][k] of one order m for 0 <= l < lmax (zero where l < m), no Condon-Shortley sign."""
    T = dtype
    theta = np.asarray(theta, dtype=T)
    x, s = np.cos(theta), np.sin(theta)
    P = np.zeros((lmax, theta.size), dtype=T)
    pi = T(np.pi) if T is np.float64 else T(4) * np.arctan(T(1))
    diag = np.full(theta.size, T(1) / np.sqrt(T(4) * pi), dtype=T)
    for i in range(1, m + 1):
        diag = np.sqrt(T(2 * i + 1) / T(2 * i)) * s * diag
    if m < lmax:
        P[m] = diag
    if m + 1 < lmax:
        P[m + 1] = np.sqrt(T(2 * m + 3)) * x * diag
    for l in range(m + 2, lmax):
        a = np.sqrt(T(4 * l * l - 1) / T(l * l - m * m))
        b = np.sqrt(T((l - 1) * (l - 1) - m * m) / T(4 * (l - 1) * (l - 1) - 1))
        P[l] = a * (x * P[l - 1] - b * P[l - 2])
    return P


def legendre(lmax, mmax, theta, dtype=np.float64):
    """Pbar[m][l][k] for 0 <= m < mmax, 0 <= l < lmax."""
    return np.stack([legendre_order(m, lmax, theta, dtype) for m in range(mmax)])


def table_order(name, m, lmax, theta, csphase=True, dtype=np.float64):
    """[lmax][nlat]: order m of table "P", "dP" or "Q"."""
    T = dtype
    mid = legendre_order(m, lmax, theta, dtype)
    if name == "P":
        out = mid
    else:
        hi = legendre_order(m + 1, lmax, theta, dtype)
        lo = legendre_order(m - 1, lmax, theta, dtype) if m > 0 else None
        out = np.zeros_like(mid)
        for l in range(max(m, 1), lmax):
            norm = np.sqrt(T(l * (l + 1)))
            if name == "dP":
                if m == 0:
                    out[l] = -np.sqrt(T(l * (l + 1))) * hi[l] / norm
                else:
                    d = np.sqrt(T((l + m) * (l - m + 1))) * lo[l] - np.sqrt(T((l - m) * (l + m + 1))) * hi[l]
                    out[l] = d / T(2) / norm
            elif m > 0:
                q = np.sqrt(T((l - m) * (l - m - 1))) * hi[l - 1] + np.sqrt(T((l + m) * (l + m - 1))) * lo[l - 1]
                out[l] = np.sqrt(T(2 * l + 1) / T(2 * l - 1)) * q / T(2) / norm
    return -out if (csphase and m % 2) else out


def tables(lmax, mmax, theta, csphase=True, dtype=np.float64):
    """{"P": Pbar, "dP": dPt, "Q": Qt}, each [mmax][lmax][nlat]."""
    return {name: np.stack([table_order(name, m, lmax, theta, csphase, dtype) for m in range(mmax)]) for name in TABLES}


def longitude_dft(x, mmax):
    """F[..., k, m] = (2 pi / nlon) sum_j x[..., k, j] e^{-2 pi i m j / nlon}, by the plain sum."""
    nlon = x.shape[-1]
    j = np.arange(nlon)
    E = np.exp(-2j * np.pi * np.outer(j, np.arange(mmax)) / nlon)
    return (2 * np.pi / nlon) * (np.asarray(x, dtype=np.float64) @ E)


def analysis(x, theta, w, lmax, mmax, csphase=True):
    """c[..., l, m] complex128."""
    P = tables(lmax, mmax, theta, csphase)["P"]
    return np.einsum("mlk,k,...km->...lm", P, w, longitude_dft(x, mmax))


def synthesis(c, theta, nlon, csphase=True):
    """x[..., k, j] float64 from c[..., l, m]."""
    lmax, mmax = c.shape[-2:]
    P = tables(lmax, mmax, theta, csphase)["P"]
    F = np.einsum("mlk,...lm->...km", P, c)
    j = np.arange(nlon)
    x = np.zeros(F.shape[:-1] + (nlon,))
    for m in range(mmax):
        ang = 2 * np.pi * m * j / nlon
        if m == 0 or 2 * m == nlon:
            x += F[..., m, None].real * np.cos(ang)
        else:
            x += 2 * (F[..., m, None].real * np.cos(ang) - F[..., m, None].imag * np.sin(ang))
    return x


def vector_analysis(u, v, theta, w, lmax, mmax, csphase=True):
    """(spheroidal, toroidal), each complex128 [..., l, m]."""
    t = tables(lmax, mmax, theta, csphase)
    Fth, Fph = -longitude_dft(v, mmax), longitude_dft(u, mmax)
    s = np.einsum("mlk,k,...km->...lm", t["dP"], w, Fth) - 1j * np.einsum("mlk,k,...km->...lm", t["Q"], w, Fph)
    tt = np.einsum("mlk,k,...km->...lm", t["dP"], w, Fph) + 1j * np.einsum("mlk,k,...km->...lm", t["Q"], w, Fth)
    return s, tt


def spectra(c):
    """(zonal[..., m], total[..., l]) of c[..., l, m]."""
    p = np.abs(c) ** 2
    mult = np.full(c.shape[-1], 2.0)
    mult[0] = 1.0
    p = p * mult
    return p.sum(axis=-2), p.sum(axis=-1)


def default_mmax(lmax, nlon):
    return min(lmax, nlon // 2 + 1)


def zonal_spectrum(field, grid):
    """credit/verification/standard.py::zonal_spectrum on [..., nlat, nlon]: lmax = nlat + 1, the sum over l."""
    nlat, nlon = field.shape[-2:]
    theta, w = nodes(nlat, grid)
    lmax = nlat + 1
    return spectra(analysis(field, theta, w, lmax, default_mmax(lmax, nlon)))[0]


def div_rot_spectrum(u, v, grid, wave_spec="n"):
    """(rotational, divergent) of credit/verification/standard.py::div_rot_spectrum: wave_spec "n" sums over m, anything else over l."""
    nlat, nlon = u.shape[-2:]
    theta, w = nodes(nlat, grid)
    lmax = nlat + 1
    s, t = vector_analysis(u, v, theta, w, lmax, default_mmax(lmax, nlon))
    i = 1 if wave_spec == "n" else 0
    return spectra(t)[i], spectra(s)[i]
