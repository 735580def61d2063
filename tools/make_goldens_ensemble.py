#!/usr/bin/env python
"""Golden fixtures of the noise-injection ensemble (dev container only: needs the reference tree).

Loads the build's synthetic name-keyed weights (wxengine.synth, noise keys included) with strict=True into the reference's
`credit.models.wxformer.crossformer_ensemble.CrossFormerWithNoise` (imported through tools/oracle_stub.py like
tools/make_goldens.py) and runs it on CPU fp32.

Tape goldens (ensemble_<name>.npz): torch.randn inside the forward is replaced by a TAPE -- the draws of
wxengine.noise.tape_from_key(cfg, B, key), shape-checked call by call -- so the engine can replay the same draws
(wx_set_noise_tape).  Only the key is stored; the test regenerates the tape.  Stored: y of every member (spatially
strided, CASES), per-member channel sums, max|y|, and (T0 geometries) forward-hook captures of the six noise layers of the
LAST member (what the engine's debug captures hold after a batched forward), spatial stride 2.

Spread golden (ensemble_spread_T0.npz): the reference's own torch.randn, 256 members, two seeds: per-channel ensemble std
(mean over pixels of the std over members) and the per-pixel std map (mean over channels).

    python tools/make_goldens_ensemble.py [--only T0,T0c,T0e,T0U,C1,C3S,spread]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tools"), os.path.join(ROOT, "miles-credit_amd"), ROOT]

import oracle_stub  # noqa: E402

oracle_stub.install()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from wxengine.config import WXConfig, named_config  # noqa: E402
from wxengine.noise import tape_from_key  # noqa: E402
from wxengine.synth import synth_input, synth_state_dict  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
B = 2
# name -> (base config, noise kwargs, y stride)
# (the strides keep every fixture near 0.25 MB: noisy outputs do not compress)
CASES = {
    "T0": ("T0", dict(noise_latent_dim=32), 2),
    "T0c": ("T0", dict(noise_latent_dim=32, correlated=True), 2),
    "T0e": ("T0", dict(noise_latent_dim=32, encoder_noise=False), 2),
    "T0U": ("T0U", dict(noise_latent_dim=32), 2),
    "C1": ("C1", dict(noise_latent_dim=64), 16),
    "C3S": ("C3S", dict(noise_latent_dim=64), 48),
}


def ensemble_config(base: str, noise: dict) -> WXConfig:
    """named_config(base) with the noise kwargs of CrossFormerWithNoise."""
    cfg = named_config(base)
    for k, v in noise.items():
        setattr(cfg, k, v)
    cfg.validate()
    return cfg


def reference_ensemble(cfg):
    from credit.models.wxformer.crossformer_ensemble import CrossFormerWithNoise
    m = CrossFormerWithNoise(
        noise_latent_dim=cfg.noise_latent_dim, encoder_noise=cfg.encoder_noise, correlated=cfg.correlated,
        image_height=cfg.image_height, image_width=cfg.image_width, frames=cfg.frames, channels=cfg.channels,
        surface_channels=cfg.surface_channels, input_only_channels=cfg.input_only_channels,
        output_only_channels=cfg.output_only_channels, levels=cfg.levels, dim=cfg.dim, depth=cfg.depth,
        dim_head=cfg.dim_head, global_window_size=cfg.global_window_size,
        local_window_size=cfg.local_window_size[0], cross_embed_kernel_sizes=cfg.cross_embed_kernel_sizes,
        cross_embed_strides=cfg.cross_embed_strides, use_spectral_norm=cfg.use_spectral_norm, interp=cfg.interp,
        **({"upsample_v_conv": True} if getattr(cfg, "upsample_v_conv", False) else {}),
        padding_conf={"activate": cfg.pad_activate, "mode": getattr(cfg, "pad_mode", "earth"), "pad_lat": list(cfg.pad_lat),
                      "pad_lon": list(cfg.pad_lon)},
        post_conf={"activate": False})
    sd = synth_state_dict(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m.eval()
    return m


class Tape:
    """torch.randn replacement that hands out the tape's tensors in order, checking every requested shape."""

    def __init__(self, draws):
        self.draws = [torch.from_numpy(d) for d in draws]
        self.i = 0

    def __call__(self, *size, **kw):
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        if self.i >= len(self.draws):
            raise AssertionError(f"the forward draws more than the tape's {len(self.draws)} tensors")
        d = self.draws[self.i]
        if tuple(d.shape) != shape:
            raise AssertionError(f"draw {self.i}: the forward asks for {shape}, the tape holds {tuple(d.shape)}")
        self.i += 1
        return d.clone()


def tape_golden(name):
    base, noise, stride = CASES[name]
    cfg = ensemble_config(base, noise)
    m = reference_ensemble(cfg)
    x = torch.from_numpy(synth_input(cfg)).repeat_interleave(B, dim=0)
    key = f"ensemble_tape_{name}"
    tape = Tape(tape_from_key(cfg, B, key))
    caps = {}
    hooks = []
    want = [p for p, _ in cfg.noise_layers()] if base.startswith("T0") else []   # the big maps: y samples only (fixture size)
    for n, mod in m.named_modules():
        if n in want:
            hooks.append(mod.register_forward_hook(lambda _m, _i, o, n=n: caps.__setitem__(n, o[-1].detach().clone())))
    real = torch.randn
    t = time.time()
    try:
        torch.randn = tape
        with torch.no_grad():
            y = m(x)
    finally:
        torch.randn = real
    dt = time.time() - t
    for h in hooks:
        h.remove()
    assert tape.i == len(tape.draws), f"the forward used {tape.i} of {len(tape.draws)} draws"
    out = {"tape_key": np.array(key), "batch": np.int64(B), "stride": np.int64(stride),
           "noise": np.array([cfg.noise_latent_dim, int(cfg.encoder_noise), int(cfg.correlated)], dtype=np.int64),
           "base": np.array(base)}
    a = y[:, :, 0].double()
    out["ch_sum"] = a.sum(dim=(2, 3)).numpy()
    out["maxabs"] = np.float64(a.abs().max())
    out["y"] = y[:, :, 0, ::stride, ::stride].numpy().astype(np.float32)
    for n, v in caps.items():
        out["cap/" + n] = v[:, ::2, ::2].numpy().astype(np.float32)
    np.savez_compressed(os.path.join(GOLD, f"ensemble_{name}.npz"), **out)
    print(f"[golden] ensemble {name}: forward {dt:.2f}s, {len(tape.draws)} draws, max|y| {float(out['maxabs']):.4f}, "
          f"member spread |y0 - y1| max {float((y[0] - y[1]).abs().max()):.4f}")


def spread_golden(n_members=256, seeds=(0, 1), chunk=32):
    cfg = ensemble_config("T0", dict(noise_latent_dim=32))
    m = reference_ensemble(cfg)
    x = torch.from_numpy(synth_input(cfg))
    out = {"n_members": np.int64(n_members)}
    for s in seeds:
        torch.manual_seed(s)
        ys = []
        with torch.no_grad():
            for _ in range(n_members // chunk):
                ys.append(m(x.repeat_interleave(chunk, dim=0))[:, :, 0].double())
        y = torch.cat(ys)
        sd = y.std(dim=0)          # [C, H, W] over members
        out[f"ch_std/{s}"] = sd.mean(dim=(1, 2)).numpy()
        out[f"px_std/{s}"] = sd.mean(dim=0).numpy().astype(np.float32)
        out[f"ch_mean/{s}"] = y.mean(dim=0).mean(dim=(1, 2)).numpy()
        print(f"[golden] spread seed {s}: mean channel std {sd.mean():.4f}")
    np.savez_compressed(os.path.join(GOLD, "ensemble_spread_T0.npz"), **out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(list(CASES) + ["spread"]))
    args = ap.parse_args()
    for n in args.only.split(","):
        if n == "spread":
            spread_golden()
        else:
            tape_golden(n)
