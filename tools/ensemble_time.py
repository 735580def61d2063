#!/usr/bin/env python
"""Cost of the noise-injection ensemble (CrossFormerWithNoise) over the deterministic engine on the same backbone (GPU box).

Both engines live in one process with the same synthetic backbone weights; 40-step wx_rollouts (the benchmark's loop: forward +
tracer fixer + de-normalise + next-input assembly) alternate between them for several rounds, so box-to-box spread cancels.
Prints ms/step of each arm and the overhead, one JSON line per configuration.

    python tools/ensemble_time.py [--configs C3:bf16,C1:bf16] [--steps 40] [--rounds 5] [--noise-dim 128]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "miles-credit_amd"), ROOT]

import torch  # noqa: E402

from wxengine.config import named_config  # noqa: E402
from wxengine.engine import WXEngine  # noqa: E402
from wxengine.rollout import channel_layout  # noqa: E402
from wxengine.synth import synth_denorm, synth_forcing, synth_input, synth_state_dict  # noqa: E402


def make(cfg, sd, prec):
    eng = WXEngine(cfg, prec, 0)
    eng.load_state_dict(sd)
    eng.finalize()
    n_prog, n_static, n_dyn = channel_layout(cfg, n_static=2, n_dyn=2)
    mean, std = synth_denorm(cfg.base_output_channels)
    eng.set_denorm(mean, std)
    eng.set_layout(n_prog, n_static, n_dyn)
    return eng, n_dyn


def run(name, prec, steps, rounds, dn):
    det_cfg = named_config(name)
    ens_cfg = named_config(name)
    ens_cfg.noise_latent_dim = dn
    ens_cfg.validate()
    sd = synth_state_dict(ens_cfg)
    det, n_dyn = make(det_cfg, {k: v for k, v in sd.items() if "noise" not in k}, prec)
    ens, _ = make(ens_cfg, sd, prec)
    x0 = torch.from_numpy(synth_input(det_cfg)).cuda()
    frc = [torch.from_numpy(synth_forcing(det_cfg, n_dyn, t + 1)).cuda() for t in range(steps)]
    H, W = det_cfg.out_hw
    ring = [torch.empty((1, det_cfg.base_output_channels, H, W), device="cuda") for _ in range(2)]
    phys = [ring[t % 2] for t in range(steps)]
    arms = {"deterministic": det, "ensemble": ens}
    times = {k: [] for k in arms}
    for r in range(rounds + 1):   # round 0 warms up (first launches, weight caches)
        for k, e in arms.items():
            if k == "ensemble":
                e.set_noise(0, 0, 0)
            torch.cuda.synchronize()
            t = time.perf_counter()
            e.rollout(x0, frc, phys_out=phys)
            torch.cuda.synchronize()
            if r:
                times[k].append((time.perf_counter() - t) * 1e3 / steps)
    best = {k: min(v) for k, v in times.items()}
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    out = dict(config=name, precision=prec, noise_latent_dim=dn, steps=steps, rounds=rounds,
               ms_per_step_median=med, ms_per_step_best=best,
               overhead_median=med["ensemble"] / med["deterministic"] - 1.0,
               overhead_best=best["ensemble"] / best["deterministic"] - 1.0,
               launches=dict(deterministic=det.query("launches"), ensemble=ens.query("launches")))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3:bf16,C1:bf16")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--noise-dim", type=int, default=128)
    args = ap.parse_args()
    for item in args.configs.split(","):
        name, _, prec = item.partition(":")
        run(name, prec or "bf16", args.steps, args.rounds, args.noise_dim)


if __name__ == "__main__":
    main()
