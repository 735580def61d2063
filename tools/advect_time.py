#!/usr/bin/env python
"""Time the semi-Lagrangian advection (csrc/wx_advect.h through wxengine/advect.py) with HIP events against the torch chain of
tests/advect_oracle.py on the same GPU -- our restatement of the algorithm in index space (it already spares the reference's halo
copies and grid_sample's normalised coordinates); the reference itself does not run here.  Two grids, one and four tracers each:
    cam   192 x 288, 32 levels
    era5  721 x 1440, 16 levels
Winds 25 m/s cos(lat) (a jet with a zonal wave) + 4 m/s cos(lat) of noise smoothed over 15 x 15 points, so that neighbouring
trajectories end near each other as in a forecast (`--white-noise`: unsmoothed noise, every trajectory on a cache line of its own --
the worst case for the gather); defaults otherwise (two iterations, omega from continuity).
Warm-up, many repeats, median.  Reported per shape: the device block's time and launch count, per kernel its time (torch.profiler) and
the achieved GB/s over the bytes it MUST move -- velocity: U, V and the surface pressure read once, one 16-byte record written per grid
point; gather: every record and every tracer read once, every tracer written once (what the eight-corner reads of two iterations add
comes from the caches) --, the scratch volume's size, and the torch chain's time and launch count.

    python tools/advect_time.py [--reps 50] [--warmup 5] [--oracle-reps 3] [--white-noise]"""
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


def kernels(fn, reps=5):
    """-> (launches per call, {kernel name: mean device time in us}) seen by torch.profiler."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA]
    total = lambda e: getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)  # noqa: E731
    return sum(e.count for e in ev) // reps, {e.key: total(e) / e.count for e in ev}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--oracle-reps", type=int, default=3)
    ap.add_argument("--white-noise", action="store_true")
    args = ap.parse_args()
    import advect_oracle as AO
    from diag_cases import hybrid_coefficients
    from wxengine.advect import SemiLagrangianAdvection, uniform_grid
    src = "ERA5"
    ku, kv, ksp = (f"{src}/prognostic/3d/u_component_of_wind", f"{src}/prognostic/3d/v_component_of_wind",
                   f"{src}/prognostic/2d/surface_pressure")
    for tag, H, W, L in (("cam", 192, 288, 32), ("era5", 721, 1440, 16)):
        g = torch.Generator(device="cuda").manual_seed(1)
        lat, lon = uniform_grid(H, W)
        a_half, b_half, _, _ = hybrid_coefficients(L)
        coslat = torch.cos(torch.deg2rad(torch.from_numpy(lat))).clamp(min=0).cuda().reshape(1, 1, 1, H, 1)
        wave = torch.sin(torch.deg2rad(torch.from_numpy(lon)) * 3).cuda().reshape(1, 1, 1, 1, W)
        # one [1, C, 1, H, W] tensor and channel slices of it, as Reconstruct hands them out
        y = torch.randn(1, 6 * L + 1, 1, H, W, device="cuda", generator=g)
        noise = y[0, :2 * L, 0]
        if not args.white_noise:
            noise = torch.nn.functional.avg_pool2d(noise[None], 15, stride=1, padding=7)[0]
            noise = noise / noise.std()
        y[:, :L] = coslat * (25.0 * (0.7 + 0.3 * wave) + 4.0 * noise[:L].reshape(1, L, 1, H, W))
        y[:, L:2 * L] = coslat * (8.0 * wave + 4.0 * noise[L:].reshape(1, L, 1, H, W))
        y[:, 6 * L:] = 98000.0 + 2000.0 * y[:, 6 * L:]
        names = [f"{src}/prognostic/3d/tracer{i}" for i in range(4)]
        fields = {ku: y[:, :L], kv: y[:, L:2 * L], ksp: y[:, 6 * L:]}
        fields.update({k: y[:, (2 + i) * L:(3 + i) * L] for i, k in enumerate(names)})
        for n_tr in (1, 4):
            blk = SemiLagrangianAdvection(tracer_vars=names[:n_tr], u_var=ku, v_var=kv, surface_pressure_var=ksp, model_a_half=a_half,
                                          model_b_half=b_half, latitude=lat, longitude=lon)
            run = lambda: blk({"y_processed": {src: dict(fields)}})  # noqa: E731
            oracle = lambda: AO.advect(fields, ku, kv, ksp, names[:n_tr], a_half, b_half, lat, lon)  # noqa: E731
            med, lo, hi = timed(run, args.warmup, args.reps)
            omed, _, _ = timed(oracle, 1, args.oracle_reps)
            launches, per_kernel = kernels(run)
            o_launches, _ = kernels(oracle, reps=1)
            pts = L * H * W
            need = {"advect_velocity_kernel": pts * (4 + 4 + 16) + 4 * H * W, "advect_gather_kernel": pts * (16 + 8 * n_tr)}
            res = {"shape": tag, "winds": "white noise" if args.white_noise else "smooth", "grid": [H, W], "levels": L, "tracers": n_tr, "device_us": round(med * 1e3, 1),
                   "device_us_min": round(lo * 1e3, 1), "device_us_max": round(hi * 1e3, 1), "device_launches": launches,
                   "scratch_MB": round(pts * 16 / 1e6, 1), "torch_chain_us": round(omed * 1e3, 1), "torch_chain_launches": o_launches,
                   "speedup_vs_torch_chain": round(omed / med, 1), "reps": args.reps}
            for kname, nbytes in need.items():
                us = next((t for k, t in per_kernel.items() if kname in k), None)
                short = kname.split("_")[1]
                res[f"{short}_bytes"] = nbytes
                if us:
                    res[f"{short}_us"] = round(us, 1)
                    res[f"{short}_GBps"] = round(nbytes / (us * 1e-6) / 1e9, 1)
            print(json.dumps(res), flush=True)
            del blk


if __name__ == "__main__":
    main()
