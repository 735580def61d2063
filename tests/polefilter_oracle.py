"""numpy oracle of the diffusion and pole filter (csrc/wx_polefilter.h), on top of tests/sht_oracle.py: the mathematics of
credit/pol_lapdiff_filt.py restated, nothing shared with the code under test.

Conventions of sht_oracle (unit-sphere tables, u east, v north, csphase off as the filter asks for it), radius a:
    vector synthesis   F_theta = sum_l dPt s - i Qt t,  F_phi = sum_l i Qt s + dPt t,  u = lon_synth(F_phi), v = -lon_synth(F_theta)
    grad(c)            vector_synthesis(sqrt(l (l + 1)) c / a, 0) = (g_x, g_y);   div(U, V) = -sqrt(l (l + 1)) s / a
    L(x)               grad(A(g_x))_x + grad(A(g_y))_y, (g_x, g_y) = grad(A(x))
    polfilt            numpy.fft on rows [-inddo .. -1, 1 .. inddo], Z[i : -i] = 0, the real part of the inverse: the reference's slicing
    V1 / QV1           x = polfilt(x); substeps times x += (L(x) sig[:, None]) coef
    V2                 U, V = polfilt(U), polfilt(V); substeps times (l_x, l_y) = grad(A(L(div(U, V)))); U -= (l_x sig) coef, V likewise
A Geometry built with dtype=np.longdouble evaluates the same chain in extended precision (tables by O.tables(dtype=np.longdouble), the
DFTs as plain sums, the low-pass by its closed form): the yardstick E_ref of the fp64 chain."""
import numpy as np

import sht_oracle as O

INDPOL = 10
COEF = {"V1": 1e8, "QV1": 0.5e8, "V2": 2e16}


# 1 / (1 + exp(-linspace(-6, 6, 10))) as float32 torch computes it (numpy's float32 exp differs in the last bit): recorded values;
# tests/test_polefilter_reference.py holds them against the live create_sigmoid_ramp_function
RAMP = np.array([float.fromhex(h) for h in (
    "0x1.441776p-9", "0x1.3143f2p-7", "0x1.1a2cd2p-5", "0x1.e84156p-4", "0x1.5b62b0p-2", "0x1.524ea6p-1", "0x1.c2f7d4p-1", "0x1.ee5d34p-1",
    "0x1.fb3af0p-1", "0x1.febbeap-1")], dtype=np.float32)


def sigmoid_ramp(nlat):
    """create_sigmoid_ramp_function(nlat, 10): float32 [nlat], the ramp up over the first ten rows and down over the last ten."""
    a = np.ones(nlat, dtype=np.float32)
    a[:INDPOL] = RAMP
    a[nlat - INDPOL:] = RAMP[::-1]
    return a


def cutoff_index(nlon):
    """argmin |1 / rfftfreq(nlon)[1:] - 100| in float32, the first minimum."""
    freq = (np.arange(1, nlon // 2 + 1, dtype=np.float32) * np.float32(1.0 / nlon)).astype(np.float32)
    return int(np.abs(np.float32(1) / freq - np.float32(100)).argmin())


def symmetric_nodes(nlat, grid):
    """sht_oracle's nodes with the northern half mirrored from the southern: theta_k + theta_{nlat-1-k} = pi and w_k = w_{nlat-1-k} bit for
    bit, the grid a transform that folds north onto south is given.  A chain of 20 transforms carries a last-bit difference of the
    nodes to the size of its own rounding, so the fixtures are made on these nodes."""
    theta, w = O.nodes(nlat, grid)
    theta, w = theta.copy(), w.copy()
    if nlat % 2:
        theta[nlat // 2] = np.pi / 2
    for k in range(nlat // 2):
        theta[k] = np.pi - theta[nlat - 1 - k]
        w[k] = w[nlat - 1 - k]
    return theta, w


class Geometry:
    def __init__(self, nlat, nlon, grid, lmax=None, mmax=None, radius=1.0, dtype=np.float64):
        self.nlat, self.nlon, self.grid, self.T = nlat, nlon, grid, dtype
        self.lmax = nlat if lmax is None else lmax
        self.mmax = O.default_mmax(self.lmax, nlon) if mmax is None else mmax
        theta, w = symmetric_nodes(nlat, grid)
        self.theta, self.w = theta.astype(dtype), w.astype(dtype)
        self.radius = dtype(radius)
        self.tab = O.tables(self.lmax, self.mmax, self.theta, csphase=False, dtype=dtype)
        l = np.arange(self.lmax).astype(dtype)
        self.sq = np.sqrt(l * (l + 1))[:, None]
        pi = dtype(np.pi) if dtype is np.float64 else dtype(4) * np.arctan(dtype(1))
        self.pi = pi
        jm = (np.outer(np.arange(nlon), np.arange(self.mmax)) % nlon).astype(dtype)
        ang = 2 * pi * jm / dtype(nlon)
        self.cos, self.sin = np.cos(ang), np.sin(ang)          # [nlon][mmax]

    # ---- transforms -------------------------------------------------------------------------------------------------------------
    def dft(self, x):
        x = np.asarray(x, dtype=self.T)
        f = 2 * self.pi / self.T(self.nlon)
        return f * (x @ self.cos) - 1j * (f * (x @ self.sin))

    def lon_synth(self, F):
        mult = np.full(self.mmax, 2, dtype=self.T)
        mult[0] = 1
        im = mult.copy()
        im[0] = 0
        if self.nlon % 2 == 0 and self.mmax > self.nlon // 2:
            mult[self.nlon // 2], im[self.nlon // 2] = 1, 0
        return (F.real * mult) @ self.cos.T - (F.imag * im) @ self.sin.T

    def analysis(self, x):
        return np.einsum("mlk,k,...km->...lm", self.tab["P"], self.w, self.dft(x))

    def synthesis(self, c):
        return self.lon_synth(np.einsum("mlk,...lm->...km", self.tab["P"], c))

    def vector_analysis(self, u, v):
        Fth, Fph = -self.dft(v), self.dft(u)
        D, Q, w = self.tab["dP"], self.tab["Q"], self.w
        s = np.einsum("mlk,k,...km->...lm", D, w, Fth) - 1j * np.einsum("mlk,k,...km->...lm", Q, w, Fph)
        t = np.einsum("mlk,k,...km->...lm", D, w, Fph) + 1j * np.einsum("mlk,k,...km->...lm", Q, w, Fth)
        return s, t

    def vector_synthesis(self, s, t=None):
        D, Q = self.tab["dP"], self.tab["Q"]
        Fth = np.einsum("mlk,...lm->...km", D, s)
        Fph = 1j * np.einsum("mlk,...lm->...km", Q, s)
        if t is not None:
            Fth = Fth - 1j * np.einsum("mlk,...lm->...km", Q, t)
            Fph = Fph + np.einsum("mlk,...lm->...km", D, t)
        return self.lon_synth(Fph), -self.lon_synth(Fth)

    # ---- the filter's operators -------------------------------------------------------------------------------------------------
    def grad(self, c):
        return self.vector_synthesis(self.sq * c / self.radius)

    def div(self, U, V):
        return -self.sq * self.vector_analysis(U, V)[0] / self.radius

    def L(self, x):
        return self.L_of_coefficients(self.analysis(x))

    def L_of_coefficients(self, c):
        gx, gy = self.grad(c)
        return self.grad(self.analysis(gx))[0] + self.grad(self.analysis(gy))[1]

    def spectral_laplacian(self, x):
        return self.synthesis(-self.sq * self.sq * self.analysis(x) / self.radius ** 2)


def polfilt_fft(D, i, inddo=INDPOL):
    """polfiltT on [..., nlat, nlon] float64, by numpy.fft exactly as the reference slices it; a new array."""
    D = np.array(D, dtype=np.float64)
    for ii in np.concatenate([np.arange(-inddo, 0), np.arange(1, inddo + 1)]):
        Z = np.fft.fft(D[..., ii, :], axis=-1)
        Z[..., i:Z.shape[-1] - i if i else 0] = 0.0            # the reference's Zlow[i:-i]: empty for i = 0
        D[..., ii, :] = np.real(np.fft.ifft(Z, axis=-1))
    return D


def polfilt_closed(D, i, inddo=INDPOL, dtype=np.float64):
    """The same by the closed form: y_j = A_0 / N + (2 / N) sum_{k=1}^{i-1} (A_k cos + B_k sin) + (1 / N) (A_i cos + B_i sin)."""
    T = dtype
    D = np.array(D, dtype=T)
    if i == 0:
        return D
    N = D.shape[-1]
    pi = T(np.pi) if T is np.float64 else T(4) * np.arctan(T(1))
    ang = 2 * pi * (np.outer(np.arange(i + 1), np.arange(N)) % N).astype(T) / T(N)
    cs, sn = np.cos(ang), np.sin(ang)                          # [i + 1][N]
    wgt = np.full(i + 1, T(2) / T(N), dtype=T)
    wgt[0] = wgt[i] = T(1) / T(N)
    for ii in np.concatenate([np.arange(-inddo, 0), np.arange(1, inddo + 1)]):
        x = D[..., ii, :]
        A, B = x @ cs.T, x @ sn.T
        D[..., ii, :] = (A * wgt) @ cs + (B * wgt) @ sn
    return D


def polfilt(G, D, i):
    return polfilt_fft(D, i) if G.T is np.float64 else polfilt_closed(D, i, dtype=G.T)


def scalar_filter(G, x, substeps, coef, sig, i):
    x = polfilt(G, x, i)
    s = np.asarray(sig).astype(G.T)[:, None]
    for _ in range(substeps):
        x = x + (G.L(x) * s) * G.T(coef)
    return x


def vector_filter(G, U, V, substeps, coef, sig, i):
    U, V = polfilt(G, U, i), polfilt(G, V, i)
    s = np.asarray(sig).astype(G.T)[:, None]
    for _ in range(substeps):
        lx, ly = G.grad(G.analysis(G.L_of_coefficients(G.div(U, V))))
        U = U - (lx * s) * G.T(coef)
        V = V - (ly * s) * G.T(coef)
    return U, V


def polefilt_lap2d_V1(G, T, substeps, sig, i):
    return scalar_filter(G, T, substeps, COEF["V1"], sig, i)


def polefilt_lap2d_QV1(G, T, substeps, sig, i):
    return scalar_filter(G, T, substeps, COEF["QV1"], sig, i)


def polefilt_lap2d_V2(G, U, V, substeps, sig, i):
    return vector_filter(G, U, V, substeps, COEF["V2"], sig, i)


def diff_lap2d_filt(G, B, sig, i):
    """The reference's channel map on [C >= 70, nlat, nlon]; a new array."""
    B = np.asarray(B, dtype=G.T)
    out = B.copy()
    out[0:16], out[16:32] = polefilt_lap2d_V2(G, B[0:16], B[16:32], 6, sig, i)
    out[32:48] = polefilt_lap2d_V1(G, B[32:48], 5, sig, i)
    out[48:64] = polefilt_lap2d_QV1(G, B[48:64], 8, sig, i)
    for ch in (64, 65, 68):
        out[ch] = polefilt_lap2d_V1(G, B[ch], 5, sig, i)
    out[67], out[66] = polefilt_lap2d_V2(G, B[67], B[66], 6, sig, i)
    out[69] = polefilt_lap2d_QV1(G, B[69], 4, sig, i)
    return out
