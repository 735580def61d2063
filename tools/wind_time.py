#!/usr/bin/env python
"""Time the wind artifact filter (csrc/wx_wind.h through wxengine/wind_filter.py) with HIP events against the torch chain of
tests/wind_oracle.py on the same GPU -- our restatement of the reference's module (one conv2d per filtered plane, the elementwise
tail, two reductions, a stack per variable); the reference itself does not run here.  Two shapes, the CAMulator settings on both:
    cam   192 x 288, 4 variables x 32 levels, 12 filtered (config/gen_2/camulator/camulator_gen2_casper.yml)
    era5  721 x 1440, 4 variables x 13 levels, all filtered
Warm-up, many repeats, median.  Reported per shape: the device block's time and launch count, the achieved GB/s over the algorithmic
bytes (every filtered plane read twice, every plane written once, pass-through planes read once), the torch chain's time and its
launch count (kernels seen by torch.profiler).

    python tools/wind_time.py [--reps 100] [--warmup 10] [--oracle-reps 5]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "miles-credit_amd"), ROOT]

import torch  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def kernel_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--oracle-reps", type=int, default=5)
    args = ap.parse_args()
    import wind_oracle as O
    from wind_cases import CAM
    from wxengine.wind_filter import WindArtifactFilter
    names = ["U", "V", "T", "Qtot"]
    keys = [f"CESM/prognostic/3d/{n}" for n in names]
    for tag, H, W, L, mask_level, levels in (("cam", 192, 288, 32, 14, list(range(9, 21))), ("era5", 721, 1440, 13, 6, list(range(13)))):
        g = torch.Generator(device="cuda").manual_seed(1)
        jet = 3.2 * torch.exp(-0.5 * ((torch.arange(H, device="cuda") - 0.35 * H) / (0.07 * H)) ** 2).reshape(1, 1, 1, H, 1)
        y_pred = 0.8 * torch.randn(1, 4 * L, 1, H, W, device="cuda", generator=g)
        y_pred[:, :L] += jet
        fields = {k: y_pred[:, i * L:(i + 1) * L] for i, k in enumerate(keys)}      # channel slices, as Reconstruct hands them out
        a = dict(CAM, mask_level=mask_level, target_levels=levels)
        blk = WindArtifactFilter(u_var=keys[0], v_var=keys[1], target_vars=keys, **a)
        run = lambda: blk({"y_processed": {"CESM": dict(fields)}})  # noqa: E731
        oracle = lambda: O.wind_filter(fields, keys[0], keys[1], keys, a)  # noqa: E731
        med, lo, hi = timed(run, args.warmup, args.reps)
        omed, _, _ = timed(oracle, 1, args.oracle_reps)
        n_f, n_all = 4 * len(levels), 4 * L
        nbytes = 4 * H * W * (2 * n_f + (n_all - n_f) + n_all)
        res = {"shape": tag, "grid": [H, W], "variables": 4, "levels": L, "filtered_levels": len(levels), "device_us": round(med * 1e3, 1),
               "device_us_min": round(lo * 1e3, 1), "device_us_max": round(hi * 1e3, 1), "device_launches": kernel_launches(run),
               "bytes": nbytes, "GBps": round(nbytes / (med * 1e-3) / 1e9, 1), "torch_chain_us": round(omed * 1e3, 1),
               "torch_chain_launches": kernel_launches(oracle), "speedup_vs_torch_chain": round(omed / med, 1), "reps": args.reps}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
