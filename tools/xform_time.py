#!/usr/bin/env python
"""Time the two variable-transform kernels (csrc/wx_pre.h pre_xform_kernel, csrc/wx_unxform.h) with HIP events at the headline grid:
721 x 1440, 13 levels, the arco_era5_wxformer.yml chain -- natural log of specific humidity and surface pressure, one NaN rule on sea
ice.  Two comparisons, each alternated call by call on the same GPU in the same process, medians over many repeats:
    input side   the fused fill -> log -> normalise -> concat pass  against the plain normalise -> concat pass (pre_assemble_kernel)
    output side  the fused inverse scale + exp launch (InverseTransforms) against the torch-op chain it replaces (InverseScale, then
                 torch.exp(y + log_eps) - eps per logged variable) on the same Reconstruct views
Achieved TB/s is against the bytes each pass must move (every value read once and written once).

    python tools/xform_time.py [--reps 200] [--warmup 20]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "miles-credit_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def alternate(fns, warmup, reps):
    """Median / min / max ms of every callable, timed in turns (a, b, a, b, ...) so that both see the same machine state."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import wxengine.transforms as X
    from wxengine.forecast import InverseScale
    from wxengine.preblock import DevicePreblock
    from wxengine.reconstruct import Reconstruct
    H, W, L, P = 721, 1440, 13, "era5/prognostic/"
    g = torch.Generator(device="cuda").manual_seed(1)
    r = lambda nl: torch.rand(1, nl, 1, H, W, device="cuda", generator=g)  # noqa: E731
    QK, SK, ICE = P + "3d/Q", P + "2d/SP", "era5/static/2d/SIC"
    ice = r(1)
    ice[ice < 0.3] = float("nan")
    inp = {"era5": {P + "3d/U": 40 * r(L) - 20, P + "3d/V": 40 * r(L) - 20, P + "3d/T": 200 + 100 * r(L), QK: 2e-2 * r(L) ** 4,
                    SK: 5e4 + 5.5e4 * r(1), P + "2d/t2m": 220 + 90 * r(1), ICE: ice, "era5/static/2d/Z": 5e4 * r(1)}}
    lv = np.arange(L, dtype=np.float32)
    mean = {"U": 0 * lv, "V": 0 * lv, "T": 250 + lv, "Q": 9 + 0.3 * lv, "SP": np.float32(29.8), "t2m": np.float32(280.0)}
    std = {"U": 8 + lv, "V": 8 + lv, "T": 10 + lv, "Q": 3 + 0.1 * lv, "SP": np.float32(0.2), "t2m": np.float32(15.0)}
    chain = [X.FillValues([{"search": "nan", "fill": 0.0}], [ICE]), X.LogTransform([QK, SK])]
    fused_pre, plain_pre = DevicePreblock(inp, mean, std, transforms=chain), DevicePreblock(inp, mean, std)
    (fmed, flo, fhi), (pmed, plo, phi) = alternate([lambda: fused_pre(inp), lambda: plain_pre(inp)], args.warmup, args.reps)
    C_in = fused_pre.channels
    pre_bytes = 2 * 4 * C_in * H * W
    res = {"grid": [H, W], "levels": L, "reps": args.reps,
           "pre": {"channels": C_in, "bytes": pre_bytes, "fused_us": round(fmed * 1e3, 1), "fused_us_min_max": [round(flo * 1e3, 1), round(fhi * 1e3, 1)],
                   "fused_TBps": round(pre_bytes / (fmed * 1e-3) / 1e12, 2), "plain_us": round(pmed * 1e3, 1),
                   "plain_us_min_max": [round(plo * 1e3, 1), round(phi * 1e3, 1)], "plain_TBps": round(pre_bytes / (pmed * 1e-3) / 1e12, 2),
                   "fused_over_plain": round(fmed / pmed, 3)}}

    out_keys = [(P + "3d/U", L), (P + "3d/V", L), (P + "3d/T", L), (QK, L), (SK, 1), (P + "2d/t2m", 1)]
    cmap, cur = {}, 0
    for k, nl in out_keys:
        cmap[k] = {"slice": slice(cur, cur + nl), "orig_shape": (nl, 1)}
        cur += nl
    y_pred = 2 * torch.rand(1, cur, 1, H, W, device="cuda", generator=g) - 1
    rec = Reconstruct()
    views = lambda: rec({"y_pred": y_pred, "metadata": {"target": {"_channel_map": cmap}}})  # noqa: E731
    fused_post, inv = X.InverseTransforms(mean, std, [X.ExpTransform([QK, SK])]), InverseScale(mean, std)
    eps, log_eps = 1e-8, math.log(1e-8)

    def torch_chain():
        full = inv(views())
        y = full["y_processed"]["era5"]
        for k in (QK, SK):
            y[k] = torch.exp(y[k] + log_eps) - eps
        return full
    a, b = fused_post(views())["y_processed"]["era5"], torch_chain()["y_processed"]["era5"]
    same = all(torch.equal(a[k], b[k]) for k, _ in out_keys if k not in (QK, SK))
    rel = max(float(((a[k] - b[k]).abs().max() / b[k].abs().max())) for k in (QK, SK))
    (umed, ulo, uhi), (tmed, tlo, thi) = alternate([lambda: fused_post(views()), torch_chain], args.warmup, args.reps)
    post_bytes = 2 * 4 * cur * H * W
    res["post"] = {"channels": cur, "bytes": post_bytes, "fused_us": round(umed * 1e3, 1), "fused_us_min_max": [round(ulo * 1e3, 1), round(uhi * 1e3, 1)],
                   "fused_TBps": round(post_bytes / (umed * 1e-3) / 1e12, 2), "torch_chain_us": round(tmed * 1e3, 1),
                   "torch_chain_us_min_max": [round(tlo * 1e3, 1), round(thi * 1e3, 1)], "torch_chain_over_fused": round(tmed / umed, 2),
                   "plain_variables_bit_identical": same, "exp_variables_max_rel_diff": rel}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
