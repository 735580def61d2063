"""The oracle against the reference's own forward, module by module.  Fixtures written by tools/make_goldens.py from the reference
CrossFormer: the whole output (model_<name>.npz), T0's sub-module outputs in full (model_T0.npz), T1's as stride-4 samples with
full-map per-channel sums and max|.| plus its dynamic position bias (reference_blocks_T1.npz, --only blocks)."""
import os

import numpy as np
import pytest
import torch

from oracle import wxformer_oracle as O
from wxengine.config import named_config
from wxengine.synth import synth_input, synth_state_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(fname):
    return np.load(os.path.join(GOLD, fname))


@pytest.mark.parametrize("name", ["T0", "T1"])
def test_forward_and_every_block(name):
    cfg = named_config(name)
    sd = synth_state_dict(cfg)
    x = torch.from_numpy(synth_input(cfg))
    mine = {}
    yo = O.forward(cfg, sd, x, capture=mine)
    gy = _load(f"model_{name}.npz")
    assert int(gy["stride"]) == 1
    yr = torch.from_numpy(gy["y"])
    assert float((yr - yo[0, :, 0]).abs().max()) <= 2e-5 * float(yr.abs().max())
    g = gy if name == "T0" else _load(f"reference_blocks_{name}.npz")
    s = 1 if name == "T0" else int(g["stride"])
    checked = 0
    for k in g.files:
        if k.startswith("cap/"):
            n = k[4:]
            v = mine[n][0]
            tol = 2e-5 * max(1.0, float(v.abs().max()))
            ref = torch.from_numpy(g[k])
            got = v[:, ::s, ::s]
            assert ref.shape == got.shape, k
            assert float((ref - got).abs().max()) <= tol, k
            if s > 1:   # the whole map through its per-channel statistics (bounds implied by the element-wise one)
                vd = v.double()
                assert float((torch.from_numpy(g["ch_maxabs/" + n]) - vd.abs().amax(dim=(1, 2))).abs().max()) <= tol, n
                assert float((torch.from_numpy(g["ch_sum/" + n]) - vd.sum(dim=(1, 2))).abs().max()) <= tol * v[0].numel(), n
            checked += 1
    assert checked >= 8


def test_dpb_bias_matches_reference_attention():
    g = _load("reference_blocks_T1.npz")
    cfg = named_config("T1")
    sd = synth_state_dict(cfg)
    want = torch.from_numpy(g["dpb/layers.0.1.layers.0.0.dpb"])
    got = O.dpb_bias(sd, "layers.0.1.layers.0.0.dpb", int(g["dpb_window"]))
    assert float((want - got).abs().max()) < 1e-5


def test_fp64_oracle_bounds_fp32_noise():
    cfg = named_config("T0")
    sd = synth_state_dict(cfg)
    x = synth_input(cfg)
    y32 = O.forward(cfg, sd, x)
    y64 = O.forward(cfg, sd, x, dtype=torch.float64)
    assert float((y32 - y64).abs().max()) < 1e-5
