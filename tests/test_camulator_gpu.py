"""model.type camulator (credit/models/camulator.py) on the GPU: the HIP engine with the legacy CrossEmbed in front of the PixelShuffle
decoder and the frame-averaging entry of the pack kernel, against tests/camulator_oracle.py (fp64) and the reference's own forward
(tests/golden/model_K*.npz).  Gates: the suite's own (test_engine_gpu.check)
    fp32 / fp32s: max|y - ref| <= 1e-4 * max|ref|;   bf16: rel-L2 <= 2e-2 and max err <= 5e-2 * max|ref|;   `pad` bit exact in fp32.
K0 = T0's geometry, K0F = two frames, K0X = K0F with a 236-channel input (two channel groups of the pack kernel) and longitude pads
[13, 11] (its scalar-load path), K2048 = CAMulator's own widths 256 .. 2048 on a 64 x 64 map (bf16 only)."""
import functools

import numpy as np
import pytest
import torch

import camulator_oracle as KO
from camulator_cases import DEMO_LEVELS, GOLD, SMALL, demo_physics, golden, post_model_conf
from synth_batches import FIXER_GATES, fixer_block_error
from test_engine_gpu import check
from wxengine.config import WXConfig, named_config
from wxengine.engine import WXEngine
from wxengine.synth import synth_denorm, synth_forcing, synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
PRECS = ["fp32", "fp32s", "bf16"]
_engines = {}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 oracle of a config, computed once and shared (read only)."""
    cfg = named_config(name)
    sd = synth_state_dict(cfg)
    x = synth_input(cfg)
    cap = {}
    y = KO.forward(cfg, sd, x, dtype=torch.float64, capture=cap)
    return cfg, sd, x, y.numpy(), {k: v[0].numpy() for k, v in cap.items()}


def engine(name, prec):
    if (name, prec) not in _engines:
        cfg, sd = reference(name)[:2]
        eng = WXEngine(cfg, prec, 0)
        eng.load_state_dict(sd)
        eng.finalize()
        _engines[(name, prec)] = eng
    return _engines[(name, prec)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", SMALL)
def test_forward_and_every_block_vs_oracle_and_golden(name, prec):
    cfg, _, x, y_ref, cap = reference(name)
    eng = engine(name, prec)
    xd = torch.from_numpy(x).cuda()
    eng.set_debug(True)
    y = eng.forward(xd).cpu().numpy()
    assert y.shape == y_ref.shape == (1, cfg.base_output_channels, 1) + tuple(cfg.out_hw)
    check(y, y_ref, prec)
    assert len(cap) >= 20
    for k, v in cap.items():
        got = eng.debug_read(k)
        assert got.shape == v.shape, k
        if k == "pad" and prec in ("fp32", "fp32s"):
            # a gather and, at two frames, (a + b) * 0.5: the fp64 mean of two fp32 values rounds to the fp32 one
            assert got.shape[0] == cfg.model_input_channels
            np.testing.assert_array_equal(got, v.astype(np.float32))
        else:
            try:
                check(got, v, prec)
            except AssertionError as e:
                raise AssertionError(f"capture {k}: {e}") from None
    eng.set_debug(False)
    y1 = eng.forward(xd).clone()
    assert torch.equal(y1, eng.forward(xd)), "two runs on the same input must be bit-identical"
    check(y1.cpu().numpy(), y_ref, prec)     # the schedule without the captures
    g = golden(name)
    s = int(g["stride"])
    check(y1[0, :, 0, ::s, ::s].cpu().numpy(), g["y"], prec)
    if prec in ("fp32", "fp32s") and "cap/pad" in g.files:     # pad(avg_pool3d(x)) of the reference itself
        cs = int(g["cap_stride"])
        eng.set_debug(True)
        eng.forward(xd)
        np.testing.assert_array_equal(eng.debug_read("pad")[:, ::cs, ::cs], g["cap/pad"])
        eng.set_debug(False)


@pytest.mark.parametrize("prec", PRECS)
def test_two_frames_enter_as_their_mean(prec):
    """The average is symmetric: swapping the frames changes no bit.  Two equal frames are one frame ((a + a) * 0.5 == a): K0F then
    reproduces K0 -- the same weights, generated per key -- bit for bit.  And the second frame is read: changing it alone moves y."""
    cfg, _, x, _, _ = reference("K0F")
    eng = engine("K0F", prec)
    xd = torch.from_numpy(x).cuda()
    y = eng.forward(xd).clone()
    assert torch.equal(eng.forward(xd.flip(2).contiguous()), y)
    one = xd[:, :, 1:2].contiguous()
    both = torch.cat([one, one], dim=2).contiguous()
    y_one = engine("K0", prec).forward(one)
    assert torch.equal(eng.forward(both), y_one)
    assert not torch.equal(y, y_one)


def test_model_class_forward_and_state_dict():
    from wxengine.model import CamulatorHIP
    cfg, sd, x, y_ref, _ = reference("K0F")
    mc = dict(image_height=37, image_width=72, frames=2, channels=4, surface_channels=4, input_only_channels=4,
              output_only_channels=3, levels=3, dim=[32, 64, 128, 256], depth=[1, 1, 2, 1], global_window_size=[4, 2, 2, 1],
              local_window_size=3, cross_embed_kernel_sizes=[[4, 8, 16, 32], [2, 4], [2, 4], [2, 4]], cross_embed_strides=[2, 2, 2, 2],
              frame_patch_size=1, attn_dropout=0.0, ff_dropout=0.0,
              padding_conf=dict(activate=True, mode="earth", pad_lat=[6, 6], pad_lon=[12, 12]), post_conf=dict(activate=False))
    m = CamulatorHIP(precision="fp32", **mc).to("cuda").eval()
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    xd = torch.from_numpy(x).cuda()
    with torch.no_grad():
        y = m(torch.cat([xd, xd.flip(2)], dim=0))
    assert y.shape == (2, 19, 1, 37, 72) and y.device == xd.device
    check(y[:1].cpu().numpy(), y_ref, "fp32")
    assert torch.equal(y[0], y[1])
    # the engine asks for every reference key it uses; the patch-1 cube embedding is never on the path
    assert set(m.engine.expected_tensors()) == {k for k in cfg.state_spec() if not k.startswith("cube_embedding.")}


@pytest.mark.parametrize("prec", ["fp32", "fp32s"])
def test_in_model_postblock_vs_reference_golden(prec):
    """model_K0F_post.npz: the reference class with its in-model TracerFixer + GlobalMassFixer on the fixers' own demo grid.  x
    carries two frames; the model consumed their mean, the mass fixer reads the last one.  The humidity block -- clamped, then
    rescaled -- within the suite's chain gate; every other channel is the plain forward's, inside the model's own gate."""
    from wxengine.model import CamulatorHIP
    g = np.load(f"{GOLD}/model_K0F_post.npz")
    mc = post_model_conf()
    cfg = WXConfig.from_model_conf(mc, arch="camulator")
    assert cfg.frames == 2 and cfg.base_input_channels == 36 and cfg.base_output_channels == 35
    x = torch.from_numpy(synth_input(cfg)).cuda()
    assert not torch.equal(x[0, :, 0], x[0, :, 1])
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg).items()}
    outs = {}
    for tag, conf in (("y_plain", post_model_conf(post=False)), ("y", mc)):
        m = CamulatorHIP(precision=prec, **conf).to("cuda").eval()
        m.load_state_dict(sd, strict=True)
        assert m.use_post_block == (tag == "y")
        if tag == "y":
            m.set_physics(**demo_physics())
        with torch.no_grad():
            y = m(x)
        assert y.shape == (1, 35, 1, 10, 18)
        outs[tag] = y[0, :, 0].cpu().numpy()
    L = DEMO_LEVELS
    q, rest = slice(L, 2 * L), np.r_[0:L, 2 * L:35]
    check(outs["y_plain"], g["y_plain"], prec)
    moved = fixer_block_error(outs["y_plain"], g["y"], q)
    err = fixer_block_error(outs["y"], g["y"], q)
    print(f"\n[camulator post] {prec}: q block vs the reference {err:.3e} (gate {FIXER_GATES['chain']:g}); the fixers move it by {moved:.3e}")
    assert moved > 20 * FIXER_GATES["chain"]
    assert err <= FIXER_GATES["chain"]
    # the tracer clamp ran: the four upper levels, which the mass fixer (fix_level_num 3 of 7, trapz) leaves alone, end at >= 0
    held = slice(L, L + 4)
    assert float(outs["y_plain"][held].min()) < 0.0 and float(outs["y"][held].min()) == 0.0
    np.testing.assert_array_equal(outs["y"][rest], outs["y_plain"][rest])     # no fixer owns them
    check(outs["y"][rest], g["y"][rest], prec)


@pytest.mark.parametrize("prec", PRECS)
def test_rollout_equals_chained_forwards(prec):
    """wx_rollout at frames == 1 (CAMulator's own configuration), three steps: every step's output and the final state equal three
    chained forward calls with the next input assembled by hand, bit for bit (mean 0 / std 1: y * 1 + 0 is y)."""
    cfg = named_config("K0")
    eng = engine("K0", prec)
    n_prog, n_static, n_dyn = cfg.channels * cfg.levels + cfg.surface_channels, 2, 2
    eng.set_denorm(np.zeros(cfg.base_output_channels, np.float32), np.ones(cfg.base_output_channels, np.float32))
    eng.set_layout(n_prog, n_static, n_dyn)
    x0 = torch.from_numpy(synth_input(cfg)).cuda()
    frcs = [torch.from_numpy(synth_forcing(cfg, n_dyn, t)).cuda() for t in (1, 2, 3)]
    oh, ow = cfg.out_hw
    phys = [torch.empty((1, cfg.base_output_channels, oh, ow), dtype=torch.float32, device="cuda") for _ in range(3)]
    x_final = torch.empty_like(x0)
    eng.rollout(x0, frcs, phys, x_final)
    x = x0
    for t in range(3):
        y = eng.forward(x)
        assert y.shape == (1, cfg.base_output_channels, 1, oh, ow)
        assert torch.equal(phys[t], y[:, :, 0]), f"step {t + 1}"
        nxt = x.clone()
        nxt[:, :n_prog] = y[:, :n_prog]
        nxt[:, n_prog + n_static:] = frcs[t]
        x = nxt
    assert torch.equal(x_final, x)
    assert not torch.equal(phys[0], phys[2])
    mean, std = synth_denorm(cfg.base_output_channels)     # leave the shared engine as the other tests expect it
    eng.set_denorm(mean, std)


def test_camulator_widths_bf16_vs_reference_golden():
    """The first forward at C = 2048: dim [256, 512, 1024, 2048], one block per stage, 64 x 64 (stage maps 32 .. 4), bf16 -- the only
    storage type the engine takes at this width -- against the reference's fp32 forward, the suite's bf16 gate.  Most of the time goes
    into generating and packing 0.2 G synthetic weights."""
    cfg = named_config("K2048")
    g = golden("K2048")
    eng = WXEngine(cfg, "bf16", 0)
    eng.load_state_dict(synth_state_dict(cfg))
    eng.finalize()
    xd = torch.from_numpy(synth_input(cfg)).cuda()
    y = eng.forward(xd).clone()
    assert y.shape == (1, 19, 1, 64, 64)
    assert torch.equal(eng.forward(xd), y)
    s = int(g["stride"])
    ys = y[0, :, 0, ::s, ::s].cpu().numpy().astype(np.float64)
    l2 = np.linalg.norm(ys - g["y"]) / np.linalg.norm(g["y"])
    print(f"\n[camulator] K2048 bf16 rel-L2 {l2:.3e}, max err / max|ref| {np.abs(ys - g['y']).max() / np.abs(g['y']).max():.3e} "
          f"(reference under bf16 autocast: {float(g['bf16_autocast_l2']):.3e})")
    check(ys, g["y"], "bf16")
