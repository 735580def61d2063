#!/usr/bin/env python
"""Time the colour filter of the perturbation noise (csrc/wx_perturb.h) with HIP events: 71 planes (one member's prognostic state) of
721 x 1440 and of 181 x 360 through `ColorNoise.__call__` on the generator (fill, four DFT passes per plane batch, epilogue; the ctypes
call included), the same filter through torch.fft.rfft2 / irfft2 in float32 on the same GPU (torch.randn, the table product, the amplitude:
what the reference runs when its tensors are on the device), and one `engine.step` of config C3 in the benchmark's set-up, which is what
the per-step cost of TemporalNoise is to be held against.  Warm-up, repeats, median / min / max.  FLOP are counted from the shapes: the
dense DFTs take 2 M N K per real product, pass B two products per complex step.

    python tools/perturb_time.py [--reps 5] [--warmup 2] [--no-step] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "miles-credit_amd"), ROOT]

import torch  # noqa: E402

from diag_time import timed  # noqa: E402

PLANES = 71


def dense_flop(H, W):
    """FLOP of one plane through the four dense passes."""
    n = 2 * (W // 2 + 1)
    return 2 * H * n * W + 2 * (2 * 2 * H * n * H) + 2 * H * W * n


def emit(res, out):
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-step", action="store_true", help="skip the C3 engine step")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perturb_time: no GPU visible; a time is measured on the GPU or not at all")
    from wxengine.perturb import ColorNoise
    noise = ColorNoise(0.05, 2)
    member_ms = {}
    for H, W in ((181, 360), (721, 1440)):
        x = torch.zeros((1, PLANES, 1, H, W), device="cuda")
        delta = torch.empty_like(x)
        step = [0]

        def device():
            step[0] += 1
            noise.apply(x, seed=1, member=0, step=step[0], delta_out=delta)
        med, lo, hi = timed(device, args.warmup, args.reps)
        assert torch.isfinite(delta).all() and 0.03 < float(delta.std()) < 0.07
        S = torch.from_numpy(noise.weights(H, W)).cuda()

        def vendor():
            return 0.05 * torch.fft.irfft2(torch.fft.rfft2(torch.randn(x.shape, device="cuda"), dim=(-2, -1)) * S, s=(H, W), dim=(-2, -1))
        vmed, vlo, vhi = timed(vendor, args.warmup, args.reps)
        flop = PLANES * dense_flop(H, W)
        member_ms[(H, W)] = med
        emit({"what": "colour filter, one member", "grid": [H, W], "planes": PLANES, "batch_planes": noise.batch_planes(H, W), "call_ms": round(med, 3),
              "call_ms_min": round(lo, 3), "call_ms_max": round(hi, 3), "plane_ms": round(med / PLANES, 4), "dense_GFLOP": round(flop / 1e9, 1),
              "dense_TFLOP_per_s": round(flop / (med * 1e-3) / 1e12, 2), "torch_fft_f32_ms": round(vmed, 3), "torch_fft_f32_ms_min": round(vlo, 3),
              "torch_fft_f32_ms_max": round(vhi, 3), "reps": args.reps}, args.out)
        del x, delta
    if args.no_step:
        return
    from wxengine.config import named_config
    from wxengine.engine import WXEngine
    from wxengine.rollout import channel_layout
    from wxengine.synth import synth_denorm, synth_forcing, synth_input, synth_state_dict
    cfg = named_config("C3")
    eng = WXEngine(cfg, "bf16", 0)
    eng.load_state_dict(synth_state_dict(cfg))
    eng.finalize()
    n_prog, n_static, n_dyn = channel_layout(cfg, n_static=2, n_dyn=2)
    eng.set_denorm(*synth_denorm(cfg.base_output_channels))
    eng.set_layout(n_prog, n_static, n_dyn)
    q = list(range(3 * cfg.levels, 4 * cfg.levels))
    eng.set_tracer_fixer(q, [1e-8] * len(q), None, denorm=True)
    x = torch.from_numpy(synth_input(cfg)).cuda()
    frc = torch.from_numpy(synth_forcing(cfg, n_dyn, 1)).cuda()
    oh, ow = cfg.out_hw
    yp = torch.empty((1, cfg.base_output_channels, oh, ow), device="cuda")
    xn = torch.empty_like(x)
    med, lo, hi = timed(lambda: eng.step(x, frc, want_y=False, phys_out=yp, next_out=xn), max(args.warmup, 3), max(args.reps, 10))
    grid = (cfg.image_height, cfg.image_width)
    emit({"what": "engine.step, C3 bf16", "grid": list(grid), "step_ms": round(med, 3), "step_ms_min": round(lo, 3), "step_ms_max": round(hi, 3),
          "n_prog": n_prog, "colour_member_over_step": round(member_ms.get(grid, float("nan")) / med, 2)}, args.out)


if __name__ == "__main__":
    main()
