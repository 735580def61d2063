"""The cases of the perturbation noise (csrc/wx_perturb.h, wxengine/perturb.py), shared by tools/make_perturb_goldens.py and the tests.
Every grid is the smallest at which a path of the colour filter can still go wrong ([C, T, H, W] of a [1, C, T, H, W] tensor):
  e5x8       3, 1, 5, 8      below one MFMA tile in every pass; even W: the Nyquist bin counts once and its imaginary part is ignored
  o7x9       2, 1, 7, 9      odd W: no Nyquist bin, the last bin counts twice; odd H; reddening 1
  p19x37     2, 2, 19, 37    prime sizes, T = 2, rows that do not start on a quad of the generator; the white and AR(1) fixtures
  t33x64     1, 1, 33, 64    one past the 16 / 32 tile edges in M, N and K (2 Wh = 66: a second column block of one live tile column)
  g37x72     4, 1, 37, 72    the T0 model grid; reddening 0 (a constant table with DC removed: a closed form without a transform) and 2
  d181x360   1, 1, 181, 360  the 1 degree grid: prime H, three row blocks and six column blocks per plane, 23 K chunks
  many19x37  65, 1, 19, 37   one plane more than a plane batch (MAX_BATCH = 64 on this grid): the batch boundary
A fixture stores the key of its tape, never the draws: tape(name) = keyed_normal(key, [1, C, T, H, W])."""
import os

import numpy as np

MAX_BATCH = 64                    # kPerturbMaxBatch
SCRATCH_BYTES = 256 << 20         # kPerturbScratchBytes
SLOT = 16                         # SLOT_PERTURB


def batch_planes(H, W):
    """perturb_batch_planes of csrc/wx_perturb.h."""
    return max(1, min(MAX_BATCH, SCRATCH_BYTES // (2 * 16 * H * (W // 2 + 1))))


def table_rtol(H, W):
    """How far two hosts' float32 `scaling_weights` may lie apart, relative to an entry: the table is elementwise float32 operations
    (exact or correctly rounded alike on every host, bar the vectorised power: one ulp) divided by sqrt(mean(w^2)), a float32 sum of
    n = H (W // 2 + 1) positive terms whose order depends on the host's vector width and thread count.  A blocked or pairwise sum is within
    (log2 n + 1) 2^-24 of the exact one; the square root halves that, the power, the root and the division add an ulp each; two hosts
    differ by at most twice the total."""
    n = H * (W // 2 + 1)
    return 2 * ((np.log2(n) + 1) / 2 + 3) * 2.0 ** -24


PERTURB_CASES = {
    "e5x8": dict(shape=(3, 1, 5, 8), reddening=(2,)),
    "o7x9": dict(shape=(2, 1, 7, 9), reddening=(1,)),
    "p19x37": dict(shape=(2, 2, 19, 37), reddening=(2,)),
    "t33x64": dict(shape=(1, 1, 33, 64), reddening=(3,)),
    "g37x72": dict(shape=(4, 1, 37, 72), reddening=(0, 2)),
    "d181x360": dict(shape=(1, 1, 181, 360), reddening=(2,)),
    "many19x37": dict(shape=(batch_planes(19, 37) + 1, 1, 19, 37), reddening=(2,)),
}
FILTER_RUNS = [(name, r) for name, c in PERTURB_CASES.items() for r in c["reddening"]]

# the white and AR(1) fixtures, on p19x37
TEMPORAL = dict(case="p19x37", amplitude=0.05, reddening=2, rho=0.9, std=(0.1, 0.02), forecast_step=2)
HEMI = dict(lat=(90.0, -90.0, 19), north=1.0, south=0.5)


def key(name):
    return f"perturb.{name}"


def tape(name, suffix=""):
    """float32 [1, C, T, H, W] from the case's key (suffix: the further keyed tensors of the AR(1) fixture)."""
    from wxengine.synth import keyed_normal
    return keyed_normal(key(name) + suffix, (1,) + tuple(PERTURB_CASES[name]["shape"]))


def load_golden(name, gold):
    """-> dict: key; shape; per reddening r: S_r{r} [H][Wh] float32, ref32_r{r} float32 and ref64_r{r} float64 [1, C, T, H, W] at
    amplitude 1, E_ref_r{r} = max|ref32 - ref64|; p19x37 also gauss32, temporal_state, temporal_delta, hemi_w."""
    z = np.load(os.path.join(gold, f"perturb_{name}.npz"))
    g = {k: z[k] for k in z.files}
    assert str(g["key"]) == key(name) and tuple(g["shape"]) == tuple(PERTURB_CASES[name]["shape"]), name
    return g
