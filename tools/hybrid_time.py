#!/usr/bin/env python
"""Time the hybrid-level interpolation (csrc/wx_hybrid.h) with HIP events at the headline grid, 721 x 1440, on T, q, u, v:
  gfs_ic   127 -> 16 levels (a GFS analysis onto a 16-level model grid: most source levels bracket nothing and are never fetched)
  up       16 -> 32 levels
Warm-up, many repeats, median; the bytes the call must move (every source value that brackets a destination level once + every
output + sp), counted from the brackets themselves, and the rate against them.  Beside it: tests/hybrid_oracle.py on the same GPU
through torch -- our restatement of the reference's form (the reference itself does not run here).

    python tools/hybrid_time.py [--reps 200] [--warmup 20] [--oracle-reps 3]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "miles-credit_amd"), ROOT]

import torch  # noqa: E402

from diag_time import timed  # noqa: E402


def touched_levels(sp, sa, sb, da, db):
    """Mean number of distinct source levels per column that are lo or hi of some destination level (the count rule, fp32)."""
    Ls = sa.numel()
    ps = (sa.view(1, -1, 1, 1, 1) + sb.view(1, -1, 1, 1, 1) * sp).clamp(min=0.57)
    touched = torch.zeros_like(ps, dtype=torch.bool)
    for j in range(da.numel()):       # one destination level at a time: the [Ld, Ls] comparison at this grid would not fit
        pd = (da[j] + db[j] * sp).clamp(min=0.57)
        hi = (pd >= ps).sum(dim=1, keepdim=True).clamp(min=1, max=Ls - 1)
        touched.scatter_(1, hi, True)
        touched.scatter_(1, hi - 1, True)
    return float(touched.sum()) / sp.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--oracle-reps", type=int, default=3)
    args = ap.parse_args()
    import hybrid_oracle as HO
    from hybrid_cases import family
    from wxengine.engine import _stream_ptr
    from wxengine.hybrid_interp import HybridLevelInterp
    H, W = 721, 1440
    src = "GFS"
    keys = [f"{src}/prognostic/3d/{n}" for n in ("temperature", "specific_humidity", "u_component_of_wind", "v_component_of_wind")]
    sp_key = f"{src}/prognostic/2d/surface_pressure"
    g = torch.Generator(device="cuda").manual_seed(1)
    sp = 52000.0 + 52000.0 * torch.rand(1, 1, 1, H, W, device="cuda", generator=g)
    for name, (fs, Ls), (fd, Ld) in (("gfs_ic", ("F2", 127), ("F1", 16)), ("up", ("F1", 16), ("F2", 32))):
        (a_s, b_s), (a_d, b_d) = family(fs, Ls), family(fd, Ld)
        blk = HybridLevelInterp(variables=keys, surface_pressure_var=sp_key, source_a=a_s, source_b=b_s, dest_a=a_d, dest_b=b_d)
        e = blk.engine
        fields = [torch.rand(1, Ls, 1, H, W, device="cuda", generator=g) for _ in keys]

        def run():
            nested = {src: dict(zip(keys, fields))}
            nested[src][sp_key] = sp
            blk({"y_processed": nested})
        med, lo, hi = timed(run, args.warmup, args.reps)
        # the launches alone: ten raw ABI calls back to back into preallocated outputs, per call (no dict, no allocation, no idle gap)
        outs = [torch.empty(1, Ld, 1, H, W, device="cuda") for _ in keys]
        c_src, c_bs = (C.c_void_p * 4)(*[f.data_ptr() for f in fields]), (C.c_int64 * 4)(0, 0, 0, 0)
        c_dst, handle = (C.c_void_p * 4)(*[o.data_ptr() for o in outs]), e._handle(H, W, 0)

        def raw10():
            for _ in range(10):
                e.lib.wx_hybrid_apply(handle, 4, c_src, c_bs, c_dst, 1, 1, C.c_void_p(sp.data_ptr()), 0, _stream_ptr(0))
        rmed, _, _ = timed(raw10, 2, max(args.reps // 10, 5))
        coef = [torch.from_numpy(x).cuda() for x in (e.source_a, e.source_b, e.dest_a, e.dest_b)]
        n_touched = touched_levels(sp, *coef)
        n = H * W
        nbytes = int(4 * n * (len(keys) * (n_touched + Ld) + 1))
        res = {"case": name, "grid": [H, W], "levels": [Ls, Ld], "variables": len(keys), "us": round(med * 1e3, 1), "us_min": round(lo * 1e3, 1),
               "us_max": round(hi * 1e3, 1), "touched_source_levels_per_column": round(n_touched, 2), "bytes": nbytes,
               "GBps": round(nbytes / (med * 1e-3) / 1e9, 1), "launch_us": round(rmed * 1e2, 1),
               "launch_GBps": round(nbytes / (rmed * 1e-4) / 1e9, 1), "us_at_6TBps": round(nbytes / 6e12 * 1e6, 1), "reps": args.reps}
        named = dict(zip(keys, fields))
        omed, _, _ = timed(lambda: HO.interp(named, sp, e.source_a, e.source_b, e.dest_a, e.dest_b), 1, args.oracle_reps)
        res["torch_oracle_us"] = round(omed * 1e3, 1)
        res["speedup_vs_torch_oracle"] = round(omed / med, 1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
