#!/usr/bin/env python
"""Time the TISR forcing (csrc/wx_tisr.h) with HIP events on the 721 x 1440 grid: num_integration_steps 360 and 2160 (the reference's
default and its own suggestion for a 6 h step), one target time and 40 target times in one call, into a preallocated destination
through `TISRForcing.compute_into` (time conversion, year check and the ctypes call included: what a rollout pays per step).
Warm-up, repeats, median / min / max of HIP-event times; per case the terms per second (points x sub-steps x times / time).  The
kernels move next to no memory: the rate to hold them to is the VALU's, not HBM's.

    python tools/tisr_time.py [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "miles-credit_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from diag_time import timed  # noqa: E402

GRID = (721, 1440)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tisr_time: no GPU visible; a time is measured on the GPU or not at all")
    from tisr_cases import NS_PER_HOUR, load_tsi
    from wxengine.tisr import TISRForcing
    tt, tv = load_tsi(os.path.join(ROOT, "tests", "golden"))
    H, W = GRID
    t0 = int(np.datetime64("2021-06-01T06:00", "ns").astype(np.int64))
    for n_steps in (360, 2160):
        blk = TISRForcing(tt, tv, 6 * NS_PER_HOUR, n_steps, lat_spec=[90, -90, H], lon_spec=[0, 359.75, W], source_name="ERA5")
        for n_times in (1, 40):
            times = [t0 + i * 6 * NS_PER_HOUR for i in range(n_times)]
            dst = torch.empty(n_times, 1, 1, H, W, device="cuda")
            med, lo, hi = timed(lambda: blk.compute_into(times, dst), args.warmup, args.reps)
            assert torch.isfinite(dst).all() and float(dst.max()) > 1.0e7
            terms = H * W * (n_steps + 1) * n_times
            res = {"grid": [H, W], "n_steps": n_steps, "times_per_call": n_times, "call_us": round(med * 1e3, 1),
                   "call_us_min": round(lo * 1e3, 1), "call_us_max": round(hi * 1e3, 1), "plane_us": round(med * 1e3 / n_times, 1),
                   "terms": terms, "Gterms_per_s": round(terms / (med * 1e-3) / 1e9, 1), "reps": args.reps}
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
