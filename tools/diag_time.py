#!/usr/bin/env python
"""Time the fused pressure-level-product launch (csrc/wx_diag.h) with HIP events at the headline grid: 721 x 1440, 16 model
levels, u / v / q + T + Z to 13 pressure levels + MSLP + model-level Z.  Warm-up, many repeats, median; achieved GB/s against the
bytes the products must move (every input read once, every output written once).  Beside it: tests/diag_oracle.py on the same GPU
through torch -- our restatement of the reference's vmap form (the reference itself does not run here).

    python tools/diag_time.py [--reps 200] [--warmup 20] [--oracle-reps 5]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "miles-credit_amd"), ROOT]

import numpy as np  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--oracle-reps", type=int, default=5)
    args = ap.parse_args()
    import diag_oracle as O
    from diag_cases import hybrid_coefficients
    from wxengine.engine import WXDiag
    H, W, L = 721, 1440, 16
    plev = [50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000]
    a_half, b_half, a_mid, b_mid = hybrid_coefficients(L)
    g = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s: torch.rand(*s, device="cuda", generator=g)  # noqa: E731
    height = 3000.0 * r(1, 1, 1, H, W) ** 2
    phis = height * 9.80665
    sp = 101325.0 * (1.0 - height / 44330.0) ** 5.255
    s = (torch.from_numpy(a_mid).cuda().reshape(1, L, 1, 1, 1) + torch.from_numpy(b_mid).cuda().reshape(1, L, 1, 1, 1) * sp) / sp
    T = (215.0 + (288.0 - 0.0065 * height - 215.0) * s + r(1, L, 1, H, W)).contiguous()
    q = (0.012 * s ** 3 * r(1, L, 1, H, W)).contiguous()
    u, v = (20.0 * r(1, L, 1, H, W) - 10.0), (20.0 * r(1, L, 1, H, W) - 10.0)
    t2m = 288.0 - 0.0065 * height + 4.0 * r(1, 1, 1, H, W)
    d = WXDiag(H, W, L)
    d.set_levels(a_half, b_half, a_mid, b_mid, True)
    d.set_pressure_levels([p * 100.0 for p in plev])
    run = lambda: d.apply(sp, phis, T=T, q=q, t_ns=t2m, fields=[u, v, q], want_z=True, want_plev=True, want_mslp=True)  # noqa: E731
    med, lo, hi = timed(run, args.warmup, args.reps)
    n = H * W
    nbytes = 4 * n * (4 * L + 3 + L + 5 * len(plev) + 1)     # T, q, u, v; sp, phis, t2m | Z on model levels, 5 variables x 13 levels, MSLP
    res = {"grid": [H, W], "levels": L, "n_plev": len(plev), "fused_us": round(med * 1e3, 1), "fused_us_min": round(lo * 1e3, 1),
           "fused_us_max": round(hi * 1e3, 1), "bytes": nbytes, "GBps": round(nbytes / (med * 1e-3) / 1e9, 1), "reps": args.reps}

    def oracle():
        z = O.geopotential(T, q, sp, phis, a_half, b_half, True)
        O.to_pressure_levels([u, v, q], T, z, sp, phis, a_mid, b_mid, np.asarray(plev, np.float32) * 100.0)
        O.mslp(sp, t2m, phis)
    omed, _, _ = timed(oracle, 1, args.oracle_reps)
    res["torch_oracle_us"] = round(omed * 1e3, 1)
    res["speedup_vs_torch_oracle"] = round(omed / med, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
