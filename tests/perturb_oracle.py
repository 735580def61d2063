"""A float64 numpy restatement of the colour filter of credit/ensemble/color.py::_create_correlated_noise,
    y = irfft2(rfft2(r) * S, s = (H, W)),
with explicit dense DFT matrices and no fft call: independent of both FFT libraries (torch's on the host, none on the device) and the
statement of what csrc/wx_perturb.h computes, pass by pass.  The phase index (k x) mod N is taken in integers, as on the device."""
import numpy as np


def _phase(n_rows, n_cols, N):
    return 2.0 * np.pi * ((np.outer(np.arange(n_rows), np.arange(n_cols)) % N).astype(np.float64) / N)


def colour_filter(r, S):
    """r [..., H, W] (any float dtype, widened to float64), S [H][W // 2 + 1] float32 -> y [..., H, W] float64."""
    r = np.asarray(r, dtype=np.float64)
    H, W = r.shape[-2:]
    Wh = W // 2 + 1
    S = np.asarray(S, dtype=np.float64)
    assert S.shape == (H, Wh)
    a = _phase(W, Wh, W)                                    # pass A: [x][k], e^{-i a}
    X = r @ (np.cos(a) - 1j * np.sin(a))                    # [..., H, Wh]
    b = _phase(H, H, H)                                     # pass B: [l][h]
    X = np.einsum("lh,...hk->...lk", np.cos(b) - 1j * np.sin(b), X) * S
    Z = np.einsum("hl,...lk->...hk", np.cos(b) + 1j * np.sin(b), X)
    c = _phase(Wh, W, W)                                    # pass C: [k][x]
    w = np.full((Wh, 1), 2.0)
    once = np.zeros((Wh, 1), dtype=bool)
    once[0] = True
    if W % 2 == 0:
        once[-1] = True
    w[once] = 1.0
    Cm = w * np.cos(c)
    Sm = np.where(once, 0.0, -w * np.sin(c))                # irfft ignores the imaginary parts of bin 0 and of the Nyquist bin
    return (Z.real @ Cm + Z.imag @ Sm) / (H * W)


def white_closed_form(r):
    """Reddening 0: S is one constant off DC, (1 - 1 / (H (W // 2 + 1)))^-1/2, so y = (r - mean(r)) / sqrt(1 - 1 / (H (W // 2 + 1)))."""
    r = np.asarray(r, dtype=np.float64)
    H, W = r.shape[-2:]
    return (r - r.mean(axis=(-2, -1), keepdims=True)) / np.sqrt(1.0 - 1.0 / (H * (W // 2 + 1)))
