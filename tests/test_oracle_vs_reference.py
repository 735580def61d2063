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


# ---- the acceptance classes (synth_batches.ACCEPTED_CONFIGS): the fp64 oracle the GPU tests of tests/test_accepted_configs_gpu.py lean
# on, pinned to the live reference classes at the same shapes (dev container only: nothing of the reference is stored)
from synth_batches import ACCEPTED_CONFIGS, accepted_config  # noqa: E402


def _live_reference(cfg, sd):
    import oracle_stub
    oracle_stub.install()
    if cfg.arch == "wxformer":
        from credit.models.wxformer.crossformer import CrossFormer
    else:
        from credit.models.crossformer import CrossFormer
    m = CrossFormer(
        image_height=cfg.image_height, image_width=cfg.image_width, frames=cfg.frames, channels=cfg.channels,
        surface_channels=cfg.surface_channels, input_only_channels=cfg.input_only_channels,
        output_only_channels=cfg.output_only_channels, levels=cfg.levels, dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head,
        global_window_size=cfg.global_window_size, local_window_size=cfg.local_window_size,
        cross_embed_kernel_sizes=cfg.cross_embed_kernel_sizes, cross_embed_strides=cfg.cross_embed_strides,
        use_spectral_norm=cfg.use_spectral_norm, interp=cfg.interp, **({"upsample_v_conv": True} if cfg.upsample_v_conv else {}),
        padding_conf={"activate": cfg.pad_activate, "mode": cfg.pad_mode, "pad_lat": list(cfg.pad_lat), "pad_lon": list(cfg.pad_lon)},
        post_conf={"activate": False})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.eval()


@pytest.mark.reference
@pytest.mark.parametrize("name", list(ACCEPTED_CONFIGS))
def test_accepted_classes_forward_and_blocks_vs_live_reference(name):
    """Same gate as test_forward_and_every_block: the output within 2e-5 * max|y|, every hooked sub-module output (CrossEmbed and
    Transformer of each stage, the four up blocks) within 2e-5 * max(1, max|.|); the fp64 oracle within the fp32 noise of that."""
    cfg = accepted_config(name)
    sd = synth_state_dict(cfg)
    x = torch.from_numpy(synth_input(cfg))
    m = _live_reference(cfg, sd)
    assert list(m.state_dict().keys()) == list(cfg.state_spec().keys())
    want = {f"layers.{s}.{j}" for s in range(4) for j in (0, 1)} | {f"up_block{i}" for i in (1, 2, 3, 4)}
    caps = {}
    hooks = [mod.register_forward_hook(lambda _m, _i, o, n=n: caps.__setitem__(n, o.detach().clone()))
             for n, mod in m.named_modules() if n in want]
    with torch.no_grad():
        yr = m(x)
    for h in hooks:
        h.remove()
    mine = {}
    yo = O.forward(cfg, sd, x, capture=mine)
    assert yo.shape == yr.shape
    assert float((yr - yo).abs().max()) <= 2e-5 * float(yr.abs().max())
    assert set(caps) == want
    for n, ref in caps.items():
        got = mine[n]
        assert ref.shape == got.shape, n
        assert float((ref - got).abs().max()) <= 2e-5 * max(1.0, float(got.abs().max())), n
    y64 = O.forward(cfg, sd, x, dtype=torch.float64)
    assert float((yr - y64).abs().max()) <= 2e-5 * float(yr.abs().max())


@pytest.mark.parametrize("name", [n for n, e in ACCEPTED_CONFIGS.items() if e["cls"] == "W"])
def test_window_class_configs_tell_short_from_long(name, monkeypatch):
    """The power of the class W tests: with the window KIND of the swept side swapped (contiguous <-> dilated) the oracle's output must
    move by at least 10 x the fp32 gate (1e-3 * max|y|) -- on a map of one window the two kinds are the same operation, and a config
    that cannot tell them apart would let a window-index bug through."""
    cfg = accepted_config(name)
    sd = synth_state_dict(cfg)
    x = synth_input(cfg)
    y = O.forward(cfg, sd, x)
    true_attention = O.attention
    for w in ACCEPTED_CONFIGS[name]["swept"]:
        assert any(cfg.local_window_size[s] == w and cfg.stage_hw[s][0] >= 2 * w and cfg.stage_hw[s][1] >= 2 * w for s in range(4)), "local"
        assert any(cfg.global_window_size[s] == w and cfg.stage_hw[s][0] >= 2 * w and cfg.stage_hw[s][1] >= 2 * w for s in range(4)), "global"
        assert all(min(cfg.stage_hw[s]) >= 2 * w for s in range(4) if w in (cfg.local_window_size[s], cfg.global_window_size[s]))

        def swapped(t, sd_, prefix, kind, wsz, dim_head=32, w=w):
            if wsz == w:
                kind = "long" if kind == "short" else "short"
            return true_attention(t, sd_, prefix, kind, wsz, dim_head)
        monkeypatch.setattr(O, "attention", swapped)
        ys = O.forward(cfg, sd, x)
        monkeypatch.setattr(O, "attention", true_attention)
        moved = float((ys - y).abs().max()) / float(y.abs().max())
        assert moved >= 1e-3, f"{name}: swapping the kind of the {w} x {w} windows moves y by {moved:.2e} of max|y| only"
