"""The cases of the zonal spectra (csrc/wx_spectrum.h, wxengine/spectrum.py), shared by tools/make_spectrum_goldens.py and the tests.
Every grid is the smallest at which a path of the kernel can still go wrong (planes x H x W, k_init):
  s0   3 x  5 x   12   0   one partial tile, Wh = 7 < 32, even W with a Nyquist bin
  s1   2 x 19 x   45   2   odd W: no Nyquist bin, no fold midpoint
  s2   5 x 37 x   90   3   K tail (Wh = 46 is no multiple of 16), two column blocks with the second partial, rows spanning three waves
  s3   2 x 70 x  144  20   two row tiles per plane (the slot reduction), three column blocks (Wh = 73)
  s4   1 x 33 x 1440  20   phase exactness at the production W, the full LDS table
Inputs are generated, never stored.  A case is a red field -- the cumulative sum along longitude of keyed normals, times 3, plus 250:
temperature-like, a large mean and a small amplitude at high wavenumbers -- as `pred`, and `target = pred + 0.5 noise`; the weights
are cos_lat_weights of latitudes at the cell centres (no row at a pole, where float32 cos(90 deg) is negative)."""
import os

import numpy as np

SPECTRUM_CASES = {
    "s0": dict(shape=(3, 5, 12), k_init=0),
    "s1": dict(shape=(2, 19, 45), k_init=2),
    "s2": dict(shape=(5, 37, 90), k_init=3),
    "s3": dict(shape=(2, 70, 144), k_init=20),
    "s4": dict(shape=(1, 33, 1440), k_init=20),
}


def key(name):
    return f"spectrum.{name}"


def fields(name):
    """-> (pred, target) float32 [P, H, W]."""
    from wxengine.synth import keyed_normal
    shape = SPECTRUM_CASES[name]["shape"]
    walk = np.cumsum(keyed_normal(key(name) + ".pred", shape).astype(np.float64), axis=-1)
    pred = (3.0 * walk + 250.0).astype(np.float32)
    target = (pred.astype(np.float64) + 0.5 * keyed_normal(key(name) + ".noise", shape).astype(np.float64)).astype(np.float32)
    return pred, target


def latitudes(H):
    return 90.0 - (np.arange(H, dtype=np.float64) + 0.5) * (180.0 / H)


def weights(name):
    """float32 [H]: cos_lat_weights of the case's latitudes."""
    from wxengine.metrics import cos_lat_weights
    return cos_lat_weights(latitudes(SPECTRUM_CASES[name]["shape"][1])).numpy()


def load_golden(name, gold):
    """-> dict: key, shape, k_init; psd32 float32 and psd64 float64 [P, H, Wh] of `pred` (PSDLoss.get_psd on the float32 field and on
    the same field cast to float64), E_ref = max|psd32 - psd64|; loss32 float32 [2] (PSDLoss, SpectralLoss2D: the live classes in
    float32, with the weights) and loss64 float64 [2] (the same formulas in float64); scores64 float64 [P, 2], the per-plane scores."""
    z = np.load(os.path.join(gold, f"spectrum_{name}.npz"))
    g = {k: z[k] for k in z.files}
    c = SPECTRUM_CASES[name]
    assert str(g["key"]) == key(name) and tuple(g["shape"]) == tuple(c["shape"]) and int(g["k_init"]) == c["k_init"], name
    return g


def r_ref(goldens):
    """The largest relative float32 error of the reference's two losses over the cases."""
    return max(float((np.abs(g["loss32"].astype(np.float64) - g["loss64"]) / np.abs(g["loss64"])).max()) for g in goldens.values())
