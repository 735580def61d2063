"""The noise-injection ensemble (CrossFormerWithNoise) on the MI355X: tape parity against the reference goldens, the device generator
against its numpy restatement, reproducibility across batch splits / steps / graph replay, ensemble spread, and the model class in
the call shape of applications/rollout_metrics_noisy_model.py.  Everything comes from tests/golden/ and wxengine.synth."""
import glob
import os

import numpy as np
import pytest
import torch

from wxengine.config import named_config
from wxengine.engine import WXEngine
from wxengine.noise import layer_shapes, normals, tape_from_key
from wxengine.synth import synth_denorm, synth_forcing, synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PRECS = ("fp32", "fp32s", "bf16")
TAPES = sorted(p for p in glob.glob(os.path.join(GOLD, "ensemble_*.npz")) if "spread" not in p)


def ens_cfg(base="T0", dn=32, **kw):
    cfg = named_config(base)
    cfg.noise_latent_dim = dn
    for k, v in kw.items():
        setattr(cfg, k, v)
    cfg.validate()
    return cfg


def engine(cfg, prec, sd):
    e = WXEngine(cfg, prec, 0)
    e.load_state_dict(sd)
    e.finalize()
    return e


def pre_name(p):
    return f"layers.{p[-1]}.1" if p.startswith("encoder") else f"up_block{p[-1]}"


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("path", TAPES, ids=[os.path.basename(p)[9:-4] for p in TAPES])
def test_tape_parity_with_reference(path, prec):
    z = np.load(path)
    dn, enc, cor = (int(v) for v in z["noise"])
    cfg = ens_cfg(str(z["base"]), dn, encoder_noise=bool(enc), correlated=bool(cor))
    B, st = int(z["batch"]), int(z["stride"])
    e = engine(cfg, prec, synth_state_dict(cfg))
    tape = [torch.from_numpy(d).cuda() for d in tape_from_key(cfg, B, str(z["tape_key"]))]
    e.set_noise_tape(tape)
    caps = [k[4:] for k in z.files if k.startswith("cap/")]
    e.set_debug(bool(caps))
    x = torch.from_numpy(np.repeat(synth_input(cfg), B, axis=0)).cuda()
    y = e.forward(x)
    torch.cuda.synchronize()
    got = y[:, :, 0, ::st, ::st].cpu().numpy()
    ref = z["y"]
    assert np.isfinite(got).all()
    if prec == "bf16":
        err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        assert err <= 2e-2, f"bf16 rel-L2 {err:.3e}"
    else:
        err = float(np.abs(got - ref).max())
        assert err <= 1e-4 * float(z["maxabs"]), f"{prec} max err {err:.3e}"
    for p in caps:   # the engine's captures hold the last batch row, as the goldens do
        g = e.debug_read(p)[:, ::2, ::2]
        r = z["cap/" + p]
        if prec == "bf16":
            assert np.linalg.norm(g - r) / np.linalg.norm(r) <= 2e-2, p
        else:
            assert np.abs(g - r).max() <= 1e-4 * np.abs(r).max(), p
    e.set_noise_tape(None)


@pytest.mark.parametrize("prec", PRECS)
def test_noise_factor_zero_is_bitwise_the_deterministic_engine(prec):
    cfg = ens_cfg("T0", 32)
    sd = synth_state_dict(cfg)
    for p, _ in cfg.noise_layers():
        sd[p + ".noise_factor"] = np.zeros(1, np.float32)
    det_cfg = named_config("T0")
    det = engine(det_cfg, prec, {k: v for k, v in sd.items() if "noise" not in k})
    ens = engine(cfg, prec, sd)
    ens.set_noise(123, 0, 0)
    x = torch.from_numpy(np.repeat(synth_input(cfg), 2, axis=0)).cuda()
    a, b = det.forward(x), ens.forward(x)
    torch.cuda.synchronize()
    assert torch.isfinite(b).all()
    assert torch.equal(a, b)
    assert ens.query("launches") > det.query("launches")   # the noise kernels did run


def raw_draw_model(cfg, latent_probe=False):
    """Weights that expose the draws: style = 1 (W = 0, b = 1), modulation = 1, noise_factor = 1 -> capture - pre = r.  With
    latent_probe: W[c][j] = (j == c % Dn), b = 0 -> style[c] = z[c % Dn], capture - pre = r * z[c % Dn]."""
    sd = synth_state_dict(cfg)
    dn = cfg.noise_latent_dim
    for p, c in cfg.noise_layers():
        w = np.zeros((c, dn), np.float32)
        if latent_probe:
            w[np.arange(c), np.arange(c) % dn] = 1.0
        sd[p + ".noise_transform.weight"] = w
        sd[p + ".noise_transform.bias"] = np.full(c, 0.0 if latent_probe else 1.0, np.float32)
        sd[p + ".modulation"] = np.ones((1, c, 1, 1), np.float32)
        sd[p + ".noise_factor"] = np.ones(1, np.float32)
    return sd


def device_draws(e, cfg):
    out = {}
    for p, c, h, w in layer_shapes(cfg):
        pre, post = e.debug_read(pre_name(p)), e.debug_read(p)
        out[p] = (post.astype(np.float64) - pre, pre)
    return out


def test_device_generator_matches_the_numpy_restatement():
    cfg = ens_cfg("T0", 32)
    e = engine(cfg, "fp32", raw_draw_model(cfg))
    e.set_debug(True)
    x = torch.from_numpy(synth_input(cfg)).cuda()
    seed = 0x1234_5678_9ABC
    pool, per = [], {}
    for member, step in ((0, 0), (1, 0), (0, 1), (3, 7)):
        e.set_noise(seed, member, step)
        e.forward(x)
        torch.cuda.synchronize()
        for slot, (p, c, h, w) in enumerate(layer_shapes(cfg)):
            d, pre = device_draws(e, cfg)[p]
            want = normals(seed, slot, member, step, c * h * w).reshape(c, h, w).astype(np.float64)
            # the add rounds to one ulp of the result; the fp32 transcendentals differ from float64 by a few ulp of the draw
            tol = np.spacing(np.abs(pre + want).astype(np.float32)).astype(np.float64) + 4e-6 * np.abs(want) + 1e-6
            bad = np.abs(d - want) > tol
            assert not bad.any(), f"{p} member {member} step {step}: {bad.sum()} elements off, max {np.abs(d - want).max():.3e}"
            pool.append(d.ravel())
            per[(p, member, step)] = d.ravel()
    a = np.concatenate(pool)
    while a.size < 1_000_000:   # more steps of the same member until >= 1e6 draws
        e.forward(x)
        torch.cuda.synchronize()
        a = np.concatenate([a] + [v[0].ravel() for v in device_draws(e, cfg).values()])
    n = a.size
    assert abs(a.mean()) < 5 / np.sqrt(n) and abs(a.var() - 1) < 5 * np.sqrt(2 / n)
    assert abs((a ** 3).mean()) < 5 * np.sqrt(15 / n) and abs((a ** 4).mean() - 3) < 5 * np.sqrt(96 / n)
    from math import erf, sqrt
    s = np.sort(a)
    cdf = 0.5 * (1 + np.vectorize(erf)(s[:: max(1, n // 200_000)] / sqrt(2)))
    emp = (np.arange(n)[:: max(1, n // 200_000)] + 0.5) / n
    ks = float(np.abs(cdf - emp).max())
    assert ks < 1.63 / np.sqrt(n) + 1e-4, f"KS {ks:.2e}"
    # independence across layers, members and steps
    def corr(u, v):
        m = min(u.size, v.size)
        return abs(np.corrcoef(u[:m], v[:m])[0, 1]), 5 / np.sqrt(m)
    p0, p5 = "encoder_noise_layers.0", "noise_inject3"
    for u, v in ((per[(p0, 0, 0)], per[(p0, 1, 0)]), (per[(p0, 0, 0)], per[(p0, 0, 1)]), (per[(p0, 0, 0)], per[(p5, 0, 0)])):
        r, lim = corr(u, v)
        assert r < lim


@pytest.mark.parametrize("correlated", [False, True])
def test_device_latents_match_the_numpy_restatement(correlated):
    cfg = ens_cfg("T0", 32, correlated=correlated)
    e = engine(cfg, "fp32", raw_draw_model(cfg, latent_probe=True))
    e.set_debug(True)
    seed, member, step = 99, 2, 5
    e.set_noise(seed, member, step)
    e.forward(torch.from_numpy(synth_input(cfg)).cuda())
    torch.cuda.synchronize()
    for slot, (p, c, h, w) in enumerate(layer_shapes(cfg)):
        d, pre = device_draws(e, cfg)[p]
        r = normals(seed, slot, member, step, c * h * w).reshape(c, h, w).astype(np.float64)
        zs = normals(seed, 6 if correlated else 6 + slot, member, step, cfg.noise_latent_dim).astype(np.float64)
        want = r * zs[np.arange(c) % cfg.noise_latent_dim][:, None, None]
        tol = np.spacing(np.abs(pre + want).astype(np.float32)).astype(np.float64) + 1e-5 * np.abs(want) + 1e-6
        assert (np.abs(d - want) <= tol).all(), f"{p}: max {np.abs(d - want).max():.3e}"


@pytest.mark.parametrize("prec", ("fp32", "bf16"))
def test_reproducible_and_batch_split_invariant(prec):
    cfg = ens_cfg("T0", 32)
    sd = synth_state_dict(cfg)
    e = engine(cfg, prec, sd)
    x1 = torch.from_numpy(synth_input(cfg)).cuda()
    x4 = x1.repeat(4, 1, 1, 1, 1).contiguous()
    e.set_noise(5, 0, 3)
    y4 = e.forward(x4).clone()
    e.set_noise(5, 0, 3)
    assert torch.equal(e.forward(x4), y4)                       # same seed: bitwise
    for b in range(4):
        e.set_noise(5, b, 3)
        assert torch.equal(e.forward(x1)[0], y4[b]), b          # row b of B = 4 == member b alone
    assert not torch.equal(y4[0], y4[1])
    e.set_noise(6, 0, 3)
    assert not torch.equal(e.forward(x1)[0], y4[0])              # another seed: other noise
    e.set_noise(5, 0, 4)
    assert not torch.equal(e.forward(x1)[0], y4[0])              # another step: other noise


def _glue(cfg, e, n_static=2, n_dyn=2):
    n_prog = cfg.channels * cfg.levels + cfg.surface_channels
    e.set_layout(n_prog, n_static, n_dyn)
    mean, std = synth_denorm(cfg.base_output_channels)
    e.set_denorm(mean, std)
    return n_dyn


@pytest.mark.parametrize("graph", ["0", "1"])
def test_rollout_equals_steps_with_fresh_noise_per_step(graph, monkeypatch):
    monkeypatch.setenv("WX_GRAPH", graph)
    cfg = ens_cfg("T0", 32)
    sd = synth_state_dict(cfg)
    e = engine(cfg, "bf16", sd)
    n_dyn = _glue(cfg, e)
    n = 4
    x0 = torch.from_numpy(synth_input(cfg)).cuda()
    frc = [torch.from_numpy(synth_forcing(cfg, n_dyn, t + 1)).cuda() for t in range(n)]
    H, W = cfg.out_hw
    # reference: n wx_step calls from step 2 of member 1
    e.set_noise(11, 1, 2)
    ref, x = [], x0
    for t in range(n):
        _, yp, xn = e.step(x, frc[t], want_y=False)
        ref.append(yp.clone())
        x = xn
    outs = []
    for _ in range(3):   # the first call warms up (eager); with WX_GRAPH=1 the later ones replay captured graphs
        e.set_noise(11, 1, 2)
        phys = [torch.empty((1, cfg.base_output_channels, H, W), device="cuda") for _ in range(n)]
        e.rollout(x0, frc, phys_out=phys)
        torch.cuda.synchronize()
        outs.append(phys)
    for phys in outs:
        for t in range(n):
            assert torch.equal(phys[t], ref[t]), t
    # the steps drew distinct noise: replaying step 2's noise at every step gives another trajectory
    e.set_noise(11, 1, 2)
    _, yp_a, _ = e.step(x0, frc[0], want_y=False)
    e.set_noise(11, 1, 3)
    _, yp_b, _ = e.step(x0, frc[0], want_y=False)
    assert not torch.equal(yp_a, yp_b)


def test_ensemble_spread_matches_the_reference():
    z = np.load(os.path.join(GOLD, "ensemble_spread_T0.npz"))
    n = int(z["n_members"])
    cfg = ens_cfg("T0", 32)
    e = engine(cfg, "fp32", synth_state_dict(cfg))
    x = torch.from_numpy(synth_input(cfg)).cuda()
    e.set_noise(2024, 0, 0)
    ys = []
    for m0 in range(0, n, 32):
        e.set_noise(2024, m0, 0)
        ys.append(e.forward(x.repeat(32, 1, 1, 1, 1).contiguous())[:, :, 0].double().cpu())
    y = torch.cat(ys)
    sd = y.std(dim=0)
    dev = sd.mean(dim=(1, 2)).numpy()
    s0, s1 = z["ch_std/0"], z["ch_std/1"]
    ref = 0.5 * (s0 + s1)
    seed_var = float(np.mean(np.abs(s0 - s1) / ref))          # what two reference seeds disagree by
    err = float(np.mean(np.abs(dev - ref) / ref))
    assert err <= 3.0 * seed_var + 0.01, f"per-channel std off by {err:.4f} (reference seed-to-seed {seed_var:.4f})"
    px = sd.mean(dim=0).numpy()
    pref = 0.5 * (z["px_std/0"] + z["px_std/1"])
    assert np.corrcoef(px.ravel(), pref.ravel())[0, 1] > 0.9


def test_model_class_in_the_noisy_rollout_call_shape():
    from wxengine.model import WXFormerEnsembleHIP
    kw = dict(frames=1, channels=4, surface_channels=4, input_only_channels=4, output_only_channels=3, levels=3,
              image_height=37, image_width=72, patch_width=1, patch_height=1, dim=[32, 64, 128, 256], depth=[1, 1, 2, 1],
              global_window_size=[4, 2, 2, 1], local_window_size=3, cross_embed_kernel_sizes=[[4, 8, 16, 32], [2, 4], [2, 4], [2, 4]],
              cross_embed_strides=[2, 2, 2, 2], use_spectral_norm=True, interp=True, noise_latent_dim=32, encoder_noise=True,
              correlated=False, freeze=True, padding_conf=dict(activate=True, mode="earth", pad_lat=[6, 6], pad_lon=[12, 12]))
    model = WXFormerEnsembleHIP(precision="bf16", seed=3, **kw)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(model.cfg).items()})
    ensemble_size = 2
    x = torch.from_numpy(synth_input(model.cfg)).cuda().repeat_interleave(ensemble_size, dim=0)
    outs = []
    with torch.no_grad():
        for k in range(1, 4):   # rollout_metrics_noisy_model: y_pred = model(x, forecast_step=k)
            y = model(x, forecast_step=k)
            assert y.shape == (ensemble_size, model.cfg.base_output_channels, 1, 37, 72)
            outs.append(y.clone())
        assert not torch.equal(outs[0][0], outs[0][1])                  # members differ
        assert not torch.equal(outs[0], outs[1])                        # steps differ
        assert torch.equal(model(x, forecast_step=2), outs[1])          # and reproduce
        model(x)                                                        # no forecast_step: the internal counter goes on
        assert model._step == 4


def test_ensemble_rollout_helper_gives_distinct_reproducible_members():
    from wxengine.rollout import ensemble_rollout
    cfg = ens_cfg("T0", 32)
    e = engine(cfg, "bf16", synth_state_dict(cfg))
    n_dyn = _glue(cfg, e)
    x0 = torch.from_numpy(synth_input(cfg)).cuda()
    frc = [torch.from_numpy(synth_forcing(cfg, n_dyn, t + 1)).cuda() for t in range(3)]
    a = ensemble_rollout(e, x0, frc, 3, seed=1)
    b = ensemble_rollout(e, x0, frc, 3, seed=1)
    torch.cuda.synchronize()
    for m in range(3):
        for t in range(3):
            assert torch.equal(a[m][t], b[m][t])
    assert not torch.equal(a[0][-1], a[1][-1]) and not torch.equal(a[1][-1], a[2][-1])
