#!/usr/bin/env python
"""Time the ensemble verification (csrc/wx_ensemble.h) with HIP events at the headline grid, 721 x 1440, 64 planes (16 variables of
4 levels), B = 1, for M = 16 and M = 50 members held in separate buffers, as ensemble_rollout leaves them.
Warm-up, many repeats, median; the bytes the call must move, (M + 1) x planes x H x W x 4 (plus 4 bytes per point and requested map),
and the rate against them.  "call" is EnsembleVerification.submit(...).result(), "launch" ten raw wx_ensemble_apply calls back to
back, per call, without maps and with all six.  Beside it: tests/ens_oracle.py on the same GPU through torch in float32 -- our
restatement of the reference's sort, [.., M, M] pairwise tensor, std and mean passes (the reference itself does not run here) -- on
ONE plane, because its pairwise tensor for all 64 planes (M^2 x 265 MB) does not fit beside the ensemble; the figure for 64 planes is
that time x 64 and is marked as extrapolated.

    python tools/ens_time.py [--members 16,50] [--reps 100] [--warmup 10] [--oracle-reps 3]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "miles-credit_amd"), ROOT]

import torch  # noqa: E402

from diag_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="16,50")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--oracle-reps", type=int, default=3)
    ap.add_argument("--grid", default="721,1440")
    args = ap.parse_args()
    import ens_oracle as EO
    from wxengine.engine import _stream_ptr
    from wxengine.ensemble_metrics import MAP_ORDER, EnsembleVerification
    H, W = (int(v) for v in args.grid.split(","))
    n_vars, L = 16, 4
    planes = n_vars * L
    keys = [f"ERA5/prognostic/3d/v{i:02d}" for i in range(n_vars)]
    g = torch.Generator(device="cuda").manual_seed(1)
    truth = {k: 280.0 + 15.0 * torch.randn(1, L, 1, H, W, device="cuda", generator=g) for k in keys}
    for M in (int(v) for v in args.members.split(",")):
        members = [{k: t + 0.3 + 1.5 * torch.randn(t.shape, device="cuda", generator=g) for k, t in truth.items()} for _ in range(M)]
        verifier = EnsembleVerification(M, alpha=0.95)
        med, lo, hi = timed(lambda: verifier.submit(members, truth).result(), args.warmup, args.reps)
        h = verifier._handle(H, W, 0)
        ptrs = (C.c_void_p * (n_vars * M))(*[members[m][k].data_ptr() for k in keys for m in range(M)])
        zeros = (C.c_int64 * n_vars)(*([0] * n_vars))
        levels, ones = (C.c_int32 * n_vars)(*([L] * n_vars)), (C.c_int32 * n_vars)(*([1] * n_vars))
        t_ptrs = (C.c_void_p * n_vars)(*[truth[k].data_ptr() for k in keys])
        table = torch.empty(planes, 6, dtype=torch.float64, device="cuda")
        maps = [torch.empty(1, L, 1, H, W, device="cuda") for _ in range(n_vars * len(MAP_ORDER))]
        map_ptrs = (C.c_void_p * len(maps))(*[x.data_ptr() for x in maps])

        def raw10(mp):
            for _ in range(10):
                st = verifier.lib.wx_ensemble_apply(h, n_vars, ptrs, zeros, t_ptrs, zeros, levels, ones, 1, 0.95, mp, C.c_void_p(table.data_ptr()),
                                                    _stream_ptr(0))
                assert st == 0, verifier.lib.wx_last_error()
        rmed, _, _ = timed(lambda: raw10(None), 2, max(args.reps // 10, 5))
        mmed, _, _ = timed(lambda: raw10(map_ptrs), 2, max(args.reps // 10, 5))
        nbytes = (M + 1) * planes * H * W * 4
        map_bytes = nbytes + len(MAP_ORDER) * planes * H * W * 4
        res = {"members": M, "grid": [H, W], "variables": n_vars, "planes": planes, "ensemble_GB": round(M * planes * H * W * 4 / 1e9, 2),
               "call_us": round(med * 1e3, 1), "call_us_min": round(lo * 1e3, 1), "call_us_max": round(hi * 1e3, 1), "bytes": nbytes,
               "launch_us": round(rmed * 1e2, 1), "launch_GBps": round(nbytes / (rmed * 1e-4) / 1e9, 1),
               "launch_all_maps_us": round(mmed * 1e2, 1), "launch_all_maps_GBps": round(map_bytes / (mmed * 1e-4) / 1e9, 1),
               "us_at_6TBps": round(nbytes / 6e12 * 1e6, 1), "points_per_us": round(planes * H * W / (rmed * 1e2), 1), "reps": args.reps}
        del maps
        k0 = keys[0]
        x1 = torch.stack([members[m][k0][:, :1] for m in range(M)])          # [M, 1, 1, 1, H, W]: one plane
        y1 = truth[k0][:, :1]
        omed, _, _ = timed(lambda: EO.variable(x1, y1, 0.95, None, torch.float32, want_maps=False), 1, args.oracle_reps)
        res["torch_oracle_one_plane_us"] = round(omed * 1e3, 1)
        res["torch_oracle_64_planes_us_extrapolated"] = round(omed * 1e3 * planes, 1)
        res["speedup_vs_torch_oracle_extrapolated"] = round(omed * planes / (rmed / 10), 1)
        print(json.dumps(res), flush=True)
        del members, x1, verifier
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
