#!/usr/bin/env python
"""Time the verification metrics (csrc/wx_metrics.h) with HIP events at the headline grid, 721 x 1440, on the C3 variable set (the
3-D variables at the model's levels, the surface variables, the diagnostics), B = 1:
  clim     all eight scores, every variable with a (level, lat, lon) climatology: three streams, read twice
  noclim   the six scores that need none: two streams, read twice
Warm-up, many repeats, median; the bytes the call must move, 2 x (pred + target [+ climatology]), and the rate against them.  "call"
is CombinedMetric.submit(...).result(), "launch" ten raw wx_metrics_apply calls back to back, per call.  Beside it:
tests/metrics_oracle.py on the same GPU through torch in float32 -- our restatement of the reference's per-metric, per-variable
passes and .item() syncs (the reference itself does not run here).

    python tools/metrics_time.py [--reps 200] [--warmup 20] [--oracle-reps 3] [--step-ms MS]"""
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
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--oracle-reps", type=int, default=3)
    ap.add_argument("--step-ms", type=float, default=None, help="the forecast step time to give the call's share of")
    args = ap.parse_args()
    import metrics_oracle as MO
    from metrics_cases import ALL8, latitude
    from wxengine.config import named_config
    from wxengine.engine import _stream_ptr
    from wxengine.metrics import CombinedMetric
    cfg = named_config("C3")
    H, W = 721, 1440
    src = "ERA5"
    shapes = {f"{src}/prognostic/3d/v{i}": cfg.levels for i in range(cfg.channels)}
    shapes.update({f"{src}/prognostic/2d/s{i}": 1 for i in range(cfg.surface_channels)})
    shapes.update({f"{src}/diagnostic/2d/d{i}": 1 for i in range(cfg.output_only_channels)})
    g = torch.Generator(device="cuda").manual_seed(1)
    target = {k: 280.0 + 15.0 * torch.randn(1, L, 1, H, W, device="cuda", generator=g) for k, L in shapes.items()}
    pred = {k: t + 0.3 + 1.5 * torch.randn(t.shape, device="cuda", generator=g) for k, t in target.items()}
    clim = {k: t[0, :, 0] - 5.0 * torch.rand(t.shape[1], H, W, device="cuda", generator=g) for k, t in target.items()}
    full = {"y_processed": {src: pred}, "y_target_processed": {src: target}}
    planes = sum(shapes.values())
    n = len(shapes)
    for name, metrics in (("clim", {m: ({"climatology": clim} if m in ("acc", "activity") else {}) for m in ALL8}),
                          ("noclim", {m: {} for m in ALL8[:6]})):
        kw = dict(metrics=metrics, var_weighting="none", use_latitude_weights=True, latitude=latitude(H))
        metric = CombinedMetric(**kw)
        med, lo, hi = timed(lambda: metric.submit(full).result(), args.warmup, args.reps)
        h = metric._handle(H, W, 0)
        keys = metric.var_keys
        ptr = lambda xs: (C.c_void_p * n)(*[x.data_ptr() for x in xs])      # noqa: E731
        zeros = (C.c_int64 * n)(*([0] * n))
        cl = (ptr([clim[k] for k in keys]), (C.c_int64 * n)(*([H * W] * n)), zeros) if name == "clim" else (None, None, None)
        levels, ones = (C.c_int32 * n)(*[shapes[k] for k in keys]), (C.c_int32 * n)(*([1] * n))
        scores = torch.empty(n, 8, device="cuda")
        c_p, c_t = ptr([pred[k] for k in keys]), ptr([target[k] for k in keys])

        def raw10():
            for _ in range(10):
                metric.lib.wx_metrics_apply(h, n, c_p, zeros, c_t, zeros, *cl, levels, ones, 1, 1e-12, C.c_void_p(scores.data_ptr()), _stream_ptr(0))
        rmed, _, _ = timed(raw10, 2, max(args.reps // 10, 5))
        streams = 3 if name == "clim" else 2
        nbytes = 2 * streams * planes * H * W * 4
        res = {"case": name, "grid": [H, W], "variables": n, "planes": planes, "state_MB": round(planes * H * W * 4 / 1e6, 1),
               "us": round(med * 1e3, 1), "us_min": round(lo * 1e3, 1), "us_max": round(hi * 1e3, 1), "bytes": nbytes,
               "GBps": round(nbytes / (med * 1e-3) / 1e9, 1), "launch_us": round(rmed * 1e2, 1),
               "launch_GBps": round(nbytes / (rmed * 1e-4) / 1e9, 1), "us_at_6TBps": round(nbytes / 6e12 * 1e6, 1), "reps": args.reps}
        oracle = MO.Restatement(dtype=torch.float32, **kw)
        omed, _, _ = timed(lambda: oracle(full), 1, args.oracle_reps)
        res["torch_oracle_us"] = round(omed * 1e3, 1)
        res["speedup_vs_torch_oracle"] = round(omed / med, 1)
        if args.step_ms:
            res["share_of_step"] = round(med / args.step_ms, 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
