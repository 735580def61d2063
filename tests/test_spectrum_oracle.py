"""The fp64 oracle of the zonal spectra (tests/spectrum_oracle.py) against the fixtures' float64 columns and against what pins its
conventions without any fixture: Parseval for both parities of W, and a single cosine that lands in its own bin alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import spectrum_cases as SC  # noqa: E402
import spectrum_oracle as SO  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", list(SC.SPECTRUM_CASES))
def test_oracle_matches_the_fixtures_fp64_columns(name):
    g = SC.load_golden(name, GOLD)
    pred, target = SC.fields(name)
    w, k_init = SC.weights(name), SC.SPECTRUM_CASES[name]["k_init"]
    assert pred.dtype == np.float32 and target.dtype == np.float32 and w.dtype == np.float32 and (w > 0).all()
    # torch.fft in float64 is good to a few ulps of the largest bin; the scores are sums of well-conditioned terms
    assert np.abs(SO.psd(pred) - g["psd64"]).max() <= 1e-12 * np.abs(g["psd64"]).max()
    assert np.abs(SO.scores(pred, target, k_init, w) - g["scores64"]).max() <= 1e-12 * np.abs(g["scores64"]).max()
    assert np.abs(SO.losses(pred, target, k_init, w) - g["loss64"]).max() <= 1e-12 * np.abs(g["loss64"]).max()
    assert float(g["E_ref"]) == float(np.abs(g["psd32"].astype(np.float64) - g["psd64"]).max()) > 0
    # the reference's float32 losses are the fp64 ones to float32 accuracy
    assert (np.abs(g["loss32"].astype(np.float64) - g["loss64"]) / np.abs(g["loss64"])).max() < 1e-3


@pytest.mark.parametrize("name", list(SC.SPECTRUM_CASES))
def test_parseval(name):
    pred, _ = SC.fields(name)
    W = pred.shape[-1]
    p = SO.psd(pred)
    mean_sq = (pred.astype(np.float64) ** 2).mean(axis=-1)
    total = p.sum(axis=-1) - (p[..., W // 2] / 2 if W % 2 == 0 else 0.0)
    assert np.abs(total - mean_sq).max() <= 1e-12 * mean_sq.max()


@pytest.mark.parametrize("W,m", [(12, 0), (12, 3), (12, 6), (45, 1), (45, 22), (90, 44)])
def test_a_single_cosine_lands_in_its_own_bin(W, m):
    x = np.arange(W)
    r = 2.0 * np.cos(2.0 * np.pi * m * x / W)[None, :].repeat(3, axis=0)
    p = SO.psd(r)
    # amplitude 2: |X_m| = W (2 W at m = 0 and at the Nyquist bin, where the cosine is its own mirror)
    own = 4.0 if m == 0 else (8.0 if 2 * m == W else 2.0)
    assert np.abs(p[:, m] - own).max() <= 1e-12
    rest = np.delete(p, m, axis=-1)
    assert np.abs(rest).max() <= 1e-24
    a = SO.mean_amp(r)
    assert np.abs(a[m] - (2 * W if m == 0 or 2 * m == W else W)).max() <= 1e-10


def test_weight_conventions():
    pred, target = SC.fields("s1")
    H = pred.shape[-2]
    ones = np.ones(H, dtype=np.float32)
    assert np.array_equal(SO.mean_amp(pred), SO.mean_amp(pred, ones)) and np.allclose(SO.mean_psd(pred), SO.mean_psd(pred, ones), rtol=1e-15)
    w = SC.weights("s1")
    # doubling the weights doubles the amplitude spectrum (divided by H) and leaves the PSD mean (divided by sum(w)) alone
    assert np.allclose(SO.mean_amp(pred, 2 * w), 2 * SO.mean_amp(pred, w), rtol=1e-15)
    assert np.allclose(SO.mean_psd(pred, 2 * w), SO.mean_psd(pred, w), rtol=1e-15)
    assert np.array_equal(SO.scores(pred, pred, 2, w), np.zeros((pred.shape[0], 2)))
