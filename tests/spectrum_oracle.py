"""fp64 restatement of the zonal spectra (csrc/wx_spectrum.h) with torch.fft in float64: every quantity of wx_spectrum_apply.

X_k = sum_x r[x] e^{-2 pi i k x / W} (torch.fft.rfft), Wh = W // 2 + 1, mult_k = 1 for k = 0 and 2 for every other bin -- the Nyquist
bin of an even W included (PSDLoss.get_psd's convention).  Parseval, which pins the convention: with mean_x r^2 the row's mean square,
    odd W    sum_k psd[k]                        = mean_x r[x]^2
    even W   sum_k psd[k] - psd[W / 2] / 2       = mean_x r[x]^2     (the Nyquist bin is counted twice but occurs once)"""
import numpy as np
import torch

LOG_EPS = 1e-8


def _f64(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64))


def psd(x):
    """PSDLoss.get_psd in float64: [..., H, W] -> [..., H, Wh]."""
    f = torch.fft.rfft(_f64(x), dim=-1)
    W = np.asarray(x).shape[-1]
    mult = torch.full((f.shape[-1],), 2.0, dtype=torch.float64)
    mult[0] = 1.0
    return ((f.real ** 2 + f.imag ** 2) * mult / float(W) ** 2).numpy()


def amplitude(x):
    """|rfft(x)|, unnormalised: [..., H, W] -> [..., H, Wh]."""
    return torch.abs(torch.fft.rfft(_f64(x), dim=-1)).numpy()


def _w(H, weights):
    return np.ones(H, dtype=np.float64) if weights is None else np.asarray(weights, dtype=np.float64).reshape(H)


def mean_psd(x, weights=None):
    """sum_h what_h psd, what = w / sum(w) (1 / H without weights): [..., Wh]."""
    w = _w(np.asarray(x).shape[-2], weights)
    return np.einsum("h,...hk->...k", w / w.sum(), psd(x))


def mean_amp(x, weights=None):
    """(sum_h w_h |X|) / H -- SpectralLoss2D divides by H, not by sum(w): [..., Wh]."""
    H = np.asarray(x).shape[-2]
    return np.einsum("h,...hk->...k", _w(H, weights), amplitude(x)) / H


def scores(pred, target, k_init, weights=None):
    """-> float64 [..., 2]: per plane the PSDLoss term and the SpectralLoss2D term."""
    w = _w(np.asarray(pred).shape[-2], weights)
    d = (np.log(psd(pred) + LOG_EPS) - np.log(psd(target) + LOG_EPS))[..., k_init:] ** 2
    s0 = np.einsum("h,...hk->...k", w / w.sum(), d).mean(axis=-1)
    s1 = ((mean_amp(pred, weights) - mean_amp(target, weights))[..., k_init:] ** 2).mean(axis=-1)
    return np.stack([s0, s1], axis=-1)


def losses(pred, target, k_init, weights=None):
    """-> float64 [2]: PSDLoss(wavenum_init)(target, pred, w) and SpectralLoss2D(wavenum_init)(pred, target, w)."""
    s = scores(pred, target, k_init, weights)
    return s.reshape(-1, 2).mean(axis=0)
