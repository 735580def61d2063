#!/usr/bin/env python
"""Headline benchmark: forecast-steps/sec of the WXFormer-6h 0.25deg (721x1440) rollout on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...

One "step" = one pass of the hot path: model forward (+ in-model tracer fixer) + de-normalise +
next-input assembly (credit/applications/rollout_to_netcdf.py:274-310), inputs resident in HBM,
synthetic N(0,1) ERA5-shaped tensors and synthetic name-keyed weights of the
`config/gen_2/examples/wxformer_era5_025deg_6hr.yml` architecture (124.0 M parameters).

N > 1: the path shards over independent init times exactly as the reference's rollout does
(rollout_to_netcdf.py:259 `i % world_size == rank`): every rank advances its own forecast, no
data-path collective, weak scaling; value = N*K steps / max-over-ranks time.

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K steps and prints it; the secondary measurements
run only with --full, each as its own object of the line (null otherwise), e.g.
  roofline     - the dominant kernel (the implicit-GEMM MFMA conv kernel), algorithmic FLOPs / HIP-event time
  cpu_baseline - the CPU oracle (oracle/wxformer_oracle.py, torch CPU fp32) timed on this box's host cores
and fp32 / fp32_split / host_delivery / concurrent_forecasts / config2 / config5 (the --no-* options still drop single legs).

--dump-outputs DIR writes what the timed path handed back after its last step (rank 0: the de-normalised output y_phys and
the next model input; the normalised output too with --latband) as DIR/<name>.npy, float32.  An array above DUMP_MAX_ELEMS
elements is written as a fixed sample (DUMP_SEED): sorted flat indices drawn without replacement, the same for every run and
build with the same arguments, whose inputs are seeded too -- so two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(ROOT, "miles-credit_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

WORKLOADS = {
    "C3": "WXFormer-6h 0.25deg 721x1440 (wxformer_era5_025deg_6hr.yml model, type crossformer), B=1 rollout",
    "C1": "WXFormer 1.0deg 181x360 (credit_smoke_test_v2.yml model), B=1 rollout",
    "T1": "tiny 61x120 test model",
}
# the metric names the grid it was measured on: BASELINE.json's headline is the C3 line, the others are labelled as what they are
METRICS = {
    "C3": "forecast-steps/sec (rollout) WXFormer-6h 0.25deg 721x1440",
    "C1": "forecast-steps/sec (rollout) WXFormer-6h 1.0deg 181x360 (BASELINE config 2; NOT the headline grid)",
    "T1": "forecast-steps/sec (rollout) tiny 61x120 test model (NOT the headline grid)",
}
PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3, "fp32s": 2500.0 / 3.0}   # fp32s: three bf16 MFMAs per product  # dense MFMA peaks, /opt/skills/guides/MI355X_MICROARCH.md
DUMP_MAX_ELEMS = 1 << 22   # per array: 16 MB of float32, at most three arrays -> well under 64 MB per dump
DUMP_SEED = 0


def dump_outputs(out_dir, arrays):
    """arrays: name -> device tensor.  Writes out_dir/<name>.npy (float32): the whole array, or its fixed seeded sample."""
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        t = t.detach()
        if t.numel() > DUMP_MAX_ELEMS:
            idx = np.sort(np.random.default_rng(DUMP_SEED).choice(t.numel(), DUMP_MAX_ELEMS, replace=False))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(out_dir, name + ".npy"), t.float().cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="C3", choices=sorted(WORKLOADS))
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32", "fp32s"])
    ap.add_argument("--full", action="store_true", help="also run the secondary measurements after the timed steps (roofline, cpu_baseline, "
                                                        "fp32, fp32_split, host_delivery, concurrent_forecasts, config2, config5)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the timed path computed in its last step to DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--cpu-steps", type=int, default=3, help="timed CPU-oracle forwards of the cpu_baseline leg (after one warm-up)")
    ap.add_argument("--no-config2", action="store_true", help="skip the secondary BASELINE-config-2 (1-degree, 24-step rollout) measurement")
    ap.add_argument("--no-fp32", action="store_true", help="skip the secondary exact-f32 measurement (the mode whose outputs meet "
                                                            "the stated fp32 tolerance against the reference)")
    ap.add_argument("--no-concurrent", action="store_true", help="skip the secondary measurement of two forecasts in flight on the one GPU")
    ap.add_argument("--no-host-delivery", action="store_true", help="skip the PCIe-inclusive measurement (every step's output delivered to pinned host memory)")
    ap.add_argument("--per-step-calls", action="store_true", help="drive the loop with one wx_step call per step from Python "
                                                                  "instead of one wx_rollout call for the K steps")
    ap.add_argument("--latband", action="store_true",
                    help="opt-in: ONE forecast sharded over the N ranks by latitude (SURVEY 8(e) mode 2, strong scaling) instead "
                         "of N independent forecasts; exchanges go through torch.distributed P2P (RCCL)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP engine has no CPU fallback")
    # WX_BENCH_BACKEND=gloo: functional check of the multi-process paths on a box with fewer GPUs than ranks (ranks then
    # share devices and timings mean nothing); the real runs use RCCL ("nccl"), one rank per GPU
    backend = os.environ.get("WX_BENCH_BACKEND", "nccl")
    # started without torchrun: this process becomes the launcher of the N ranks (and exits with their code); `--gpus N` on a node
    # with fewer GPUs fails loudly instead of running one rank (reference: rank discovery credit/distributed.py:193-292)
    from wxengine.replicas import ensure_ranks
    ensure_ranks(args.gpus, backend, [os.path.abspath(__file__), *sys.argv[1:]])
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if backend != "nccl":
        local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    from wxengine.replicas import ReplicaGroup
    grp = ReplicaGroup(backend=backend, n_expected=args.gpus, device_index=local_rank)
    rank, world, dist = grp.rank, grp.world, grp.dist

    from wxengine.config import named_config
    from wxengine.engine import WXEngine
    from wxengine.rollout import channel_layout
    from wxengine.synth import synth_denorm, synth_forcing, synth_input, synth_state_dict

    cfg = named_config(args.config)
    sd = synth_state_dict(cfg)
    eng = WXEngine(cfg, args.precision, local_rank)
    eng.load_state_dict(sd)
    eng.finalize()
    n_prog, n_static, n_dyn = channel_layout(cfg, n_static=2, n_dyn=2)
    mean, std = synth_denorm(cfg.base_output_channels)
    eng.set_denorm(mean, std)
    eng.set_layout(n_prog, n_static, n_dyn)
    # the benchmark config's in-model post block: tracer fixer on the 13 q levels, physical units
    # (wxformer_era5_025deg_6hr.yml:210-216)
    q_inds = list(range(3 * cfg.levels, 4 * cfg.levels))
    eng.set_tracer_fixer(q_inds, [1e-8] * len(q_inds), None, denorm=True)

    dev = torch.device("cuda", local_rank)
    if args.latband:
        return bench_latband(args, cfg, eng, grp, dev, n_dyn)
    # each rank = its own init time (seed) -> independent forecasts, as rollout_to_netcdf.py:259
    x_a = torch.from_numpy(synth_input(cfg, seed=1000 + rank)).to(dev)
    x_b = torch.empty_like(x_a)
    n_frc = 8  # forcing ring pre-staged in HBM (synthetic; the reference reads it from the dataset)
    frcs = [torch.from_numpy(synth_forcing(cfg, n_dyn, t, seed=1000 + rank)).to(dev) for t in range(n_frc)]
    oh, ow = cfg.out_hw
    y_phys = torch.empty((1, cfg.base_output_channels, oh, ow), dtype=torch.float32, device=dev)

    def run(nsteps, x_cur, x_nxt, t0):
        """nsteps forecast steps from x_cur; returns (state after the last step, spare buffer)."""
        if args.per_step_calls:
            for t in range(nsteps):
                eng.step(x_cur, frcs[(t0 + t) % n_frc], want_y=False, phys_out=y_phys, next_out=x_nxt)
                x_cur, x_nxt = x_nxt, x_cur
            return x_cur, x_nxt
        # the predict() loop inside the library: one C-ABI call for the nsteps steps (wx_rollout), same launches per step
        eng.rollout(x_cur, [frcs[(t0 + t) % n_frc] for t in range(nsteps)], [y_phys] * nsteps, x_final=x_nxt)
        return x_nxt, x_cur

    x_cur, x_nxt = run(args.warmup, x_a, x_b, 0) if args.warmup > 0 else (x_a, x_b)
    state = {}

    def timed_work():
        state["x"] = run(args.steps, x_cur, x_nxt, args.warmup)
    elapsed = grp.timed(timed_work, torch.cuda.synchronize)
    x_cur, x_nxt = state["x"]
    finite = bool(torch.isfinite(y_phys).all().item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"y_phys": y_phys, "x_next": x_cur})

    host_delivery = None
    if args.full and rank == 0 and world == 1 and not args.no_host_delivery:
        # What the reference's loop does with every step's output (rollout_to_netcdf.py:289-301: y_pred_phys.cpu().numpy() handed to the
        # writer pool): the PCIe-INCLUSIVE rate, never `value`.  Pinned ring + copy stream (wxengine.output.HostDelivery: step t computes
        # while step t-1 crosses PCIe), and beside it the reference's own form -- a blocking pageable copy per step on the same engine.
        from wxengine.output import HostDelivery
        hd = HostDelivery(eng, x_cur, slots=2)
        nh = max(2, min(args.steps, 20))
        seen = []
        hd.run(x_cur, [frcs[t % n_frc] for t in range(3)], lambda i, a: seen.append(float(a[0, 0, 0, 0])))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        hd.run(x_cur, [frcs[t % n_frc] for t in range(nh)], lambda i, a: seen.append(float(a[0, 0, 0, 0])))
        torch.cuda.synchronize()
        eh = time.perf_counter() - t1
        nb = max(2, min(args.steps, 5))
        xs_, xn_ = x_cur, x_nxt
        eng.step(xs_, frcs[0], want_y=False, phys_out=y_phys, next_out=xn_)
        y_phys.cpu().numpy()
        t1 = time.perf_counter()
        for t in range(nb):
            eng.step(xs_, frcs[t % n_frc], want_y=False, phys_out=y_phys, next_out=xn_)
            y_phys.cpu().numpy()
            xs_, xn_ = xn_, xs_
        eb = (time.perf_counter() - t1) / nb
        # what the D2H link itself gives on THIS box: the same 266 MB from device to pinned host memory, nothing else running,
        # on one copy stream and as two halves on two streams (is 31.8 GB/s the engine's limit or the link's?)
        link = {}
        try:
            pin = torch.empty(y_phys.shape, dtype=torch.float32, pin_memory=True)
            flat_d, flat_h = y_phys.view(-1), pin.view(-1)
            half = flat_d.numel() // 2
            s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
            for name, parts in (("one_stream", [(s1, 0, flat_d.numel())]), ("two_streams", [(s1, 0, half), (s2, half, flat_d.numel())])):
                best_l = None
                for _ in range(4):
                    torch.cuda.synchronize()
                    tl = time.perf_counter()
                    for st, a, b in parts:
                        with torch.cuda.stream(st):
                            flat_h[a:b].copy_(flat_d[a:b], non_blocking=True)
                    torch.cuda.synchronize()
                    el_ = time.perf_counter() - tl
                    best_l = el_ if best_l is None else min(best_l, el_)
                link[name] = round(flat_d.numel() * 4 / best_l / 1e9, 2)
            del pin
        except Exception as exc:   # pinned allocation refused: report it, do not fail the bench
            link = {"error": str(exc)[:120]}
        host_delivery = {"value": round(nh / eh, 3), "d2h_link_GBps": link, "unit": "forecast-steps/sec", "steps": nh, "ms_per_step": round(1e3 * eh / nh, 3),
                         "output_MB_per_step": round(hd.bytes_per_step / 1e6, 1), "d2h_GBps": round(nh * hd.bytes_per_step / eh / 1e9, 2),
                         "blocking_copy_per_step": {"value": round(1.0 / eb, 3), "ms_per_step": round(1e3 * eb, 3), "steps": nb,
                                                    "what": "y_phys.cpu().numpy() after every step (rollout_to_netcdf.py:292), same engine"},
                         "finite_outputs": bool(np.isfinite(seen).all()),
                         "note": "PCIe-inclusive: every step's de-normalised output lands in pinned host memory (2-slot ring, copy stream "
                                 "overlapped with the next step's compute; one wx_step call per step); PCIe Gen5 x16 = 63 GB/s spec"}
        del hd

    concurrent = None
    if args.full and rank == 0 and world == 1 and args.config == "C3" and not args.no_concurrent:
        # Serving option, never `value`: TWO forecasts (init times) in flight on the one GPU, each on its own engine + stream
        # (wxengine.replicas.ForecastPool) -- the reference walks a rank's init times one at a time (rollout_to_netcdf.py:259-262).
        from wxengine.replicas import ForecastPool

        def make():
            e = WXEngine(cfg, args.precision, local_rank)
            e.load_state_dict(sd)
            e.finalize()
            e.set_denorm(mean, std)
            e.set_layout(n_prog, n_static, n_dyn)
            e.set_tracer_fixer(q_inds, [1e-8] * len(q_inds), None, denorm=True)
            return e
        pool = ForecastPool(make, 2, local_rank)
        nc = max(2, min(args.steps, 20))
        jobs = []
        for i in range(2):
            xi = torch.from_numpy(synth_input(cfg, seed=2000 + i)).to(dev)
            jobs.append(dict(x0=xi, forcings=[frcs[t % n_frc] for t in range(nc)], phys_out=[torch.empty_like(y_phys)] * nc, x_final=torch.empty_like(xi)))
        pool.rollout_all([dict(j, forcings=j["forcings"][:3], phys_out=j["phys_out"][:3]) for j in jobs])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        pool.rollout_all(jobs)
        torch.cuda.synchronize()
        ec = time.perf_counter() - t1
        concurrent = {"forecasts_in_flight": 2, "value": round(2 * nc / ec, 3), "unit": "forecast-steps/sec (aggregate of the two forecasts)",
                      "steps_per_forecast": nc, "ms_per_step_per_forecast": round(1e3 * ec / nc, 3),
                      "finite_outputs": bool(all(torch.isfinite(j["phys_out"][0]).all().item() for j in jobs)),
                      "note": "two engines + two HIP streams on one GPU (wxengine.replicas.ForecastPool); each forecast is B = 1 and bit-identical "
                              "to running it alone; the headline `value` above is ONE forecast in flight"}
        del pool, jobs

    roofline = None
    if args.full and rank == 0 and not args.no_roofline:
        eng.profile(True)
        eng.profile_reset()
        nprof = 3
        x_cur, x_nxt = run(nprof, x_cur, x_nxt, 0)
        rows = eng.profile_read()
        eng.profile(False)
        gemm = [r for r in rows if r["name"].startswith("gemm_")]
        g_ms = sum(r["ms"] for r in gemm)
        g_fl = sum(r["flops"] for r in gemm)
        g_n = sum(r["launches"] for r in gemm)
        tot_ms = sum(r["ms"] for r in rows)
        achieved = g_fl / (g_ms * 1e-3) / 1e12
        peak = PEAK_TFLOPS[args.precision]
        # HBM traffic of the same kernel from the PMC passes of tools/collect_profiles.sh (rocprofv3 cannot run inside
        # this process; the summary is committed next to the kernel-stats it was collected with)
        traffic, traffic_note, traffic_step = None, None, None
        tname = next((n for n in ("pmc_traffic_r06.json", "pmc_traffic_r05.json", "pmc_traffic_r04.json", "pmc_traffic_r03.json", "pmc_traffic_r01.json") if os.path.isfile(os.path.join(ROOT, "profiles", n))), None)
        if args.config == "C3" and args.precision == "bf16" and tname:
            pj = json.load(open(os.path.join(ROOT, "profiles", tname)))
            kern = pj["kernels"]
            lib_hash = eng.lib.wx_version().decode().rsplit("wxsrc:", 1)[-1]
            fam = [kern[k] for k in ("wx::conv_gemm_dma_kernel", "wx::gemm_stream_kernel", "wx::gemm8p_kernel") if k in kern]
            if pj.get("wxsrc") != lib_hash:
                # the counters were collected on ANOTHER build of the library (or before round 5 stamped them): not this run's traffic
                traffic_note = (f"stale: profiles/{tname} was collected on library wxsrc:{pj.get('wxsrc')}, this run loaded wxsrc:{lib_hash} "
                                "(re-collect with tools/collect_profiles.sh)")
            elif fam:   # launch-weighted mean over the GEMM kernel families
                nl = sum(k.get("launches", 1) for k in fam)
                traffic = round(sum((k["fetch_bytes_per_launch"] + k["write_bytes_per_launch"]) * k.get("launches", 1) for k in fam) / nl)
                traffic_step = pj.get("engine_bytes_per_step")
        # the same family's kernel time by rocprofv3 (tools/collect_profiles.sh -> profiles/kernel_time_<tag>.json, hash-stamped like the
        # traffic): HIP events around every launch inflate the in-process sum by 5-8 %, so `frac` (events) UNDER-states the kernel
        frac_rocprof, rocprof_note, rocprof_us = None, None, None
        kname = next((n for n in ("kernel_time_r06.json",) if os.path.isfile(os.path.join(ROOT, "profiles", n))), None)
        if args.config == "C3" and args.precision == "bf16" and kname:
            kj = json.load(open(os.path.join(ROOT, "profiles", kname)))
            lib_hash = eng.lib.wx_version().decode().rsplit("wxsrc:", 1)[-1]
            if kj.get("wxsrc") != lib_hash:
                rocprof_note = f"stale: profiles/{kname} is of library wxsrc:{kj.get('wxsrc')}, this run loaded wxsrc:{lib_hash}"
            elif kj.get("gemm_family_us_per_step"):
                rocprof_us = kj["gemm_family_us_per_step"]
                frac_rocprof = round((g_fl / nprof) / (rocprof_us * 1e-6) / 1e12 / peak, 4)
        roofline = {
            "bound": "mfma", "kernel": "wx::conv_gemm_dma_kernel + wx::gemm_stream_kernel (implicit-GEMM MFMA convs; all gemm_* launches)",
            "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4),
            "frac_events": round(achieved / peak, 4), "frac_rocprof": frac_rocprof, "rocprof_kernel_us_per_step": rocprof_us, "rocprof_note": rocprof_note,
            "traffic_per_step": traffic_step, "algorithmic_bytes_per_step": 5.9e9 if args.config == "C3" and args.precision == "bf16" else None,
            "traffic": traffic, "traffic_unit": f"HBM bytes per launch (FETCH_SIZE x2 + WRITE_SIZE; profiles/{tname})", "traffic_note": traffic_note,
            "algorithmic_bytes_per_launch": round(sum(r["bytes"] for r in gemm) / max(g_n, 1)),
            "launches_per_step": g_n // nprof, "avg_launch_us": round(1e3 * g_ms / max(g_n, 1), 2),
            "flops_per_step": g_fl / nprof, "kernel_ms_per_step": round(g_ms / nprof, 3),
            "all_kernels_ms_per_step": round(tot_ms / nprof, 3),
            "by_class_ms_per_step": {r["name"]: round(r["ms"] / nprof, 3) for r in sorted(rows, key=lambda r: -r["ms"])},
        }
        # second bound the north star names: window attention against HBM (algorithmic q|k|v + out bytes over the class's
        # event time -- an event pair adds ~3 us to each ~45 us launch, so this UNDER-states the kernel: profiles/ has rocprofv3's)
        att = [r for r in rows if r["name"] == "window_attn"]
        if att and att[0]["ms"] > 0:
            a_gbs = att[0]["bytes"] / (att[0]["ms"] * 1e-3) / 1e9
            roofline["attention"] = {"bound": "hbm", "kernel": "wx::window_attn_kernel (all launches)", "achieved": round(a_gbs, 1),
                                     "peak": 8000.0, "unit": "GB/s", "frac": round(a_gbs / 8000.0, 4),
                                     "launches_per_step": att[0]["launches"] // nprof,
                                     "avg_launch_us": round(1e3 * att[0]["ms"] / max(att[0]["launches"], 1), 2)}
        # stage 0 runs the one-launch attention sub-block (LN + to_qkv + attention + to_out + residual; q|k|v never reach HBM): its
        # only HBM traffic is the stream in and out, so its GB/s says how little it moves, not how well -- it is issue-bound
        blk = [r for r in rows if r["name"] == "attn_block"]
        if blk and blk[0]["ms"] > 0:
            roofline["attention_block"] = {"kernel": "wx::attn_block_kernel", "launches_per_step": blk[0]["launches"] // nprof,
                                           "avg_launch_us": round(1e3 * blk[0]["ms"] / max(blk[0]["launches"], 1), 2),
                                           "hbm_bytes_per_launch": round(blk[0]["bytes"] / max(blk[0]["launches"], 1)),
                                           "tflops": round(blk[0]["flops"] / (blk[0]["ms"] * 1e-3) / 1e12, 1)}

    cpu_baseline = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import wxformer_oracle as O  # checker/baseline only; never on the product path
        # torch's CPU conv path degrades badly when oversubscribed (256 threads: 281 s/step on the GPU box vs
        # 62 s with 8 threads in the dev container), so the baseline uses the PHYSICAL cores, at most 32, and says so.
        logical = os.cpu_count() or 1
        try:
            import psutil
            physical = psutil.cpu_count(logical=False) or logical
        except Exception:
            physical = logical
        xs = synth_input(cfg, seed=1000)
        n_cpu = max(1, args.cpu_steps)
        # round 6: one timed step at 32 / 64 / 128 threads (capped at the physical cores), the best count then runs the remaining timed steps;
        # every count's time is reported (256 threads = every logical CPU: 281 s/step, not repeated)
        sweep_counts = sorted({min(c, physical) for c in (32, 64, 128)})
        sweep = {}
        with torch.no_grad():
            torch.set_num_threads(sweep_counts[0])
            O.forward(cfg, sd, xs)   # warm-up (thread pool, allocator, first-touch of the activation buffers): not timed
            for c in sweep_counts:
                torch.set_num_threads(c)
                t1 = time.perf_counter()
                O.forward(cfg, sd, xs)
                sweep[c] = time.perf_counter() - t1
            cores = min(sweep, key=sweep.get)
            torch.set_num_threads(cores)
            times = [sweep[cores]]
            for _ in range(n_cpu - 1):
                t1 = time.perf_counter()
                O.forward(cfg, sd, xs)
                times.append(time.perf_counter() - t1)
        cpu_s = float(np.median(times))
        cpu_baseline = {"value": round(1.0 / cpu_s, 5), "unit": "forecast-steps/sec", "cores": cores, "kind": "port",
                        "physical_cores": physical, "logical_cpus": logical,
                        "seconds_per_step": [round(t, 2) for t in times],
                        "seconds_per_step_by_threads": {str(c): round(t, 2) for c, t in sweep.items()},
                        "sample": f"1 warm-up + one timed forecast step at each of {sweep_counts} threads + {n_cpu - 1} more at the best count "
                                  f"({cores}; median of its {len(times)} steps reported) of the same {args.config} workload (forward only), torch CPU "
                                  f"fp32 oracle on {physical} physical cores ({logical} logical CPUs), {cpu_s:.1f} s per step"}

    fp32 = fp32_split = None
    if args.full and rank == 0 and world == 1 and args.precision == "bf16" and not args.no_fp32:
        # the mode whose outputs meet the stated fp32 tolerance against the reference (exact-f32 MFMA, tests/test_engine_gpu.py):
        # same workload, same loop, fewer steps (it is ~8x slower); reported beside the headline, never as `value`
        del eng
        torch.cuda.empty_cache()
        eng32 = WXEngine(cfg, "fp32", local_rank)
        eng32.load_state_dict(sd)
        eng32.finalize()
        eng32.set_denorm(mean, std)
        eng32.set_layout(n_prog, n_static, n_dyn)
        eng32.set_tracer_fixer(q_inds, [1e-8] * len(q_inds), None, denorm=True)
        n32 = max(2, min(args.steps, 5))
        f32 = [frcs[t % n_frc] for t in range(n32)]
        eng32.rollout(x_a, f32[:1], [y_phys], x_final=x_b)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        eng32.rollout(x_a, f32, [y_phys] * n32, x_final=x_b)
        torch.cuda.synchronize()
        e32 = time.perf_counter() - t1
        fp32 = {"value": round(n32 / e32, 4), "unit": "forecast-steps/sec", "steps": n32, "ms_per_step": round(1e3 * e32 / n32, 3),
                "dtype": "fp32 (exact-f32 MFMA v_mfma_f32_16x16x4_f32)", "finite_outputs": bool(torch.isfinite(y_phys).all().item()),
                "note": "parity mode: max|y - reference| <= 1e-4 max|reference| (measured 2.7e-6 on this workload)"}
        y32 = y_phys.clone()
        del eng32
        torch.cuda.empty_cache()
        # round 5: the FAST mode that still meets that tolerance -- fp32 storage, LayerNorm / GroupNorm / softmax statistics in fp32, every
        # implicit GEMM AND the window attention's Q.K^T / P.V as split-bf16 arithmetic (x_hi.W_hi + x_hi.W_lo + x_lo.W_hi on the bf16
        # MFMA pipe, fp32 accumulate; include/wxengine.h lists the window sizes that take it): what a
        # maintainer who needs the reference's fp32 numerics (credit/seed.py:24-25: TF32 off) would run.  Same loop, same workload.
        engs = WXEngine(cfg, "fp32s", local_rank)
        engs.load_state_dict(sd)
        engs.finalize()
        engs.set_denorm(mean, std)
        engs.set_layout(n_prog, n_static, n_dyn)
        engs.set_tracer_fixer(q_inds, [1e-8] * len(q_inds), None, denorm=True)
        ns = max(2, min(args.steps, 10))
        fs = [frcs[t % n_frc] for t in range(ns)]
        engs.rollout(x_a, fs[:n32], [y_phys] * n32, x_final=x_b)       # warm-up = the exact-f32 leg's trajectory: compare its last output
        torch.cuda.synchronize()
        dev_rel = float((y_phys - y32).abs().max() / y32.abs().max())
        t1 = time.perf_counter()
        engs.rollout(x_a, fs, [y_phys] * ns, x_final=x_b)
        torch.cuda.synchronize()
        es = time.perf_counter() - t1
        fp32_split = {"value": round(ns / es, 4), "unit": "forecast-steps/sec", "steps": ns, "ms_per_step": round(1e3 * es / ns, 3),
                      "dtype": "fp32 storage, split-bf16 GEMM arithmetic (3 x v_mfma_f32_16x16x32_bf16 per product, fp32 accumulate)",
                      "split_gemm_launches_per_step": engs.query("split_gemms"),
                      "max_dev_from_exact_f32_engine": round(dev_rel, 9),
                      "finite_outputs": bool(torch.isfinite(y_phys).all().item()),
                      "note": f"tolerance mode: max|y - reference| <= 1e-4 max|reference| (measured 1.04e-5 on this workload's golden; "
                              f"tests/test_engine_gpu.py, both stress families <= 6.5e-5); max|y_phys - exact-f32 engine| after {n32} steps "
                              f"of this run = {dev_rel:.2e} of max|y_phys|"}
        del engs

    config2 = None
    if args.full and rank == 0 and world == 1 and args.config == "C3" and args.precision == "bf16" and not args.no_config2:
        # BASELINE config 2 beside the headline: the 1-degree model, 24-step rollout (the launch-latency regime); never `value`
        cfg1 = named_config("C1")
        e1 = WXEngine(cfg1, "bf16", local_rank)
        e1.load_state_dict(synth_state_dict(cfg1))
        e1.finalize()
        p1, s1, d1 = channel_layout(cfg1, n_static=2, n_dyn=2)
        m1, sd1 = synth_denorm(cfg1.base_output_channels)
        e1.set_denorm(m1, sd1)
        e1.set_layout(p1, s1, d1)
        q1 = list(range(3 * cfg1.levels, 4 * cfg1.levels))
        e1.set_tracer_fixer(q1, [1e-8] * len(q1), None, denorm=True)
        xa1 = torch.from_numpy(synth_input(cfg1, seed=1000)).to(dev)
        xb1 = torch.empty_like(xa1)
        f1 = [torch.from_numpy(synth_forcing(cfg1, d1, t, seed=1000)).to(dev) for t in range(8)]
        oh1, ow1 = cfg1.out_hw
        yp1 = torch.empty((1, cfg1.base_output_channels, oh1, ow1), dtype=torch.float32, device=dev)
        n1 = 24
        e1.rollout(xa1, [f1[t % 8] for t in range(5)], [yp1] * 5, x_final=xb1)
        torch.cuda.synchronize()
        best = None
        for _ in range(3):
            t1 = time.perf_counter()
            e1.rollout(xa1, [f1[t % 8] for t in range(n1)], [yp1] * n1, x_final=xb1)
            torch.cuda.synchronize()
            el = time.perf_counter() - t1
            best = el if best is None else min(best, el)
        config2 = {"metric": METRICS["C1"], "value": round(n1 / best, 2), "unit": "forecast-steps/sec", "steps": n1,
                   "ms_per_step": round(1e3 * best / n1, 4), "dtype": "bf16", "workload": WORKLOADS["C1"],
                   "finite_outputs": bool(torch.isfinite(yp1).all().item()), "note": "best of 3 x 24-step wx_rollout calls after 5 warm-up steps"}
        del e1

    config5 = None
    if args.full and rank == 0 and world == 1 and args.config == "C3" and args.precision == "bf16" and not args.no_config2:
        # BASELINE config 5 (second architecture): the FuXi-6h 0.25-degree forward (the model section of the reference's fuxi_6h_single_step.yml:
        # 640 x 1280, patch 4, 2 frames, 74 channels in / 71 out, dim 1024, 8 heads, 7 x 7 windows, depth 16; 266 M parameters) through wx_fuxi_*: CubeEmbedding, DownBlock, the Swin
        # stage on 84 x 161 padded tokens, UpBlock, fc, patch -> pixel.  Keyed synthetic weights.  The stage is made of timm's Swin V2 block
        # (timm.models.swin_transformer_v2, what fuxi.py:250-260 instantiates: q / v bias, 16 sigmoid(cpb_mlp) bias table, mask over both
        # axes, timm's state-dict keys); timm is not vendored, so that block follows timm's published code (parity unpinned).
        from wxengine.fuxi import FuxiHIP, named_fuxi_config, synth_fuxi_state_dict
        cfg5 = named_fuxi_config("F6H")
        m5 = FuxiHIP(precision="bf16", device=local_rank, cfg=cfg5)
        m5.load_state_dict(synth_fuxi_state_dict(cfg5))
        x5 = torch.randn(1, cfg5.in_chans, cfg5.frames, cfg5.image_height, cfg5.image_width, generator=torch.Generator().manual_seed(5)).to(dev)
        y5 = torch.empty((1, cfg5.out_chans, 1, cfg5.image_height, cfg5.image_width), dtype=torch.float32, device=dev)
        for _ in range(3):
            m5(x5, y5)
        torch.cuda.synchronize()
        best5, n5 = None, 10
        for _ in range(3):
            t1 = time.perf_counter()
            for _ in range(n5):
                m5(x5, y5)
            torch.cuda.synchronize()
            e5 = (time.perf_counter() - t1) / n5
            best5 = e5 if best5 is None else min(best5, e5)
        config5 = {"metric": "FuXi-6h 0.25deg (640x1280, patch 4, dim 1024, depth 16) forwards/sec on 1 MI355X",
                   "value": round(1.0 / best5, 2), "unit": "forwards/sec", "ms_per_forward": round(1e3 * best5, 3), "dtype": "bf16",
                   "params": int(sum(int(np.prod(v)) for v in cfg5.state_spec().values())),
                   "tflops": round(m5.flops / best5 / 1e12, 1), "finite_outputs": bool(torch.isfinite(y5).all().item()),
                   "stage_variant": cfg5.stage,
                   "note": "best of 3 x 10 forwards after 3 warm-ups; whole forward (embedding, down / up blocks, 16-block Swin stage, fc); stage_variant "
                           "'timm' = timm's SwinTransformerV2Block as the reference builds it (state-dict keys of a reference checkpoint; parity "
                           "of the block itself unpinned: timm absent, SURVEY 8(c)); 'cr' = credit/models/swin.py's block (pinned)"}
        del m5
        if not args.no_fp32:   # the same forward in the fast mode that meets the fp32 tolerance (round 5: wx_fuxi_create takes WX_PREC_FP32_SPLIT)
            torch.cuda.empty_cache()
            ms5 = FuxiHIP(precision="fp32s", device=local_rank, cfg=cfg5)
            ms5.load_state_dict(synth_fuxi_state_dict(cfg5))
            ms5(x5, y5)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(3):
                ms5(x5, y5)
            torch.cuda.synchronize()
            e5s = (time.perf_counter() - t1) / 3
            config5["fp32_split"] = {"value": round(1.0 / e5s, 2), "unit": "forwards/sec", "ms_per_forward": round(1e3 * e5s, 3),
                                     "dtype": "fp32 storage, split-bf16 GEMM arithmetic", "finite_outputs": bool(torch.isfinite(y5).all().item()),
                                     "note": "exact-f32 engine: 77 ms per forward (tools/fuxi_time.py fp32 3); measured 1.6e-5 of max|y| from it"}
            del ms5

    if rank == 0:
        total_steps = args.steps * world
        out = {
            "metric": METRICS[args.config],
            "value": round(grp.throughput(args.steps, elapsed), 4), "unit": "forecast-steps/sec", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.precision,
            "data": "synthetic (N(0,1) ERA5-shaped inputs/forcing, name-keyed synthetic weights; no dataset/checkpoint)",
            "config": {"workload": WORKLOADS[args.config], "batch": 1, "init_times_per_gpu": 1,
                       "parallelism": f"replicas over init times x{world} (no data-path collective)",
                       "loop": "one wx_step call per step" if args.per_step_calls else "wx_rollout (the K steps in one C-ABI call)",
                       "total_steps": total_steps, "params": cfg.num_params(), "finite_outputs": finite},
            "roofline": roofline, "cpu_baseline": cpu_baseline, "fp32": fp32, "fp32_split": fp32_split, "host_delivery": host_delivery, "concurrent_forecasts": concurrent, "config2": config2, "config5": config5,
        }
        print(json.dumps(out), flush=True)
    grp.close()


def bench_latband(args, cfg, eng, grp, dev, n_dyn):
    """One forecast over `world` ranks: every rank keeps its latitude band of x / forcing / y resident; no gather in the loop."""
    from wxengine.latband import DistBand
    from wxengine.synth import synth_forcing, synth_input
    dist, rank, world = grp.dist, grp.rank, grp.world
    db = DistBand(eng)
    r0, rows = db.rows
    band = lambda t: t[0, :, 0, r0:r0 + rows].contiguous().to(dev)  # noqa: E731
    x_a = band(torch.from_numpy(synth_input(cfg, seed=1000)))
    x_b = torch.empty_like(x_a)
    n_frc = 8
    frcs = [band(torch.from_numpy(synth_forcing(cfg, n_dyn, t, seed=1000))) for t in range(n_frc)]
    y = torch.empty((cfg.base_output_channels, rows, cfg.image_width), dtype=torch.float32, device=dev)
    y_phys = torch.empty_like(y)

    def run(nsteps, x_cur, x_nxt, t0):
        for t in range(nsteps):
            db.step(x_cur, frcs[(t0 + t) % n_frc], y=y, y_phys=y_phys, x_next=x_nxt)
            x_cur, x_nxt = x_nxt, x_cur
        return x_cur, x_nxt

    x_cur, x_nxt = run(args.warmup, x_a, x_b, 0)
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    db.exchanged_bytes = 0
    t0 = time.perf_counter()
    x_cur, x_nxt = run(args.steps, x_cur, x_nxt, args.warmup)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:   # rank 0's latitude band
        dump_outputs(args.dump_outputs, {"y": y, "y_phys": y_phys, "x_next": x_cur})
    sent_per_step = float(db.sent_bytes_per_step) if db.transport == "rccl" else float(db.exchanged_bytes) / args.steps
    stats = torch.tensor([elapsed, sent_per_step, float(torch.isfinite(y_phys).all().item())],
                         dtype=torch.float64, device=dev if (not dist or dist.get_backend() == "nccl") else "cpu")
    if dist:
        mx = stats.clone()
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        mn = stats.clone()
        dist.all_reduce(mn, op=dist.ReduceOp.MIN)
        elapsed, sent, finite = float(mx[0]), float(mx[1]), bool(mn[2] > 0)
    else:
        elapsed, sent, finite = float(stats[0]), float(stats[1]), bool(stats[2] > 0)
    if rank == 0:
        out = {
            "metric": METRICS[args.config],
            "value": round(args.steps / elapsed, 4), "unit": "forecast-steps/sec", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": args.precision,
            "data": "synthetic (N(0,1) ERA5-shaped inputs/forcing, name-keyed synthetic weights; no dataset/checkpoint)",
            "config": {"workload": WORKLOADS[args.config], "batch": 1,
                       "parallelism": f"lat-band sharding of ONE forecast x{world} (halo / long-attention / GroupNorm exchanges: "
                                      + ("grouped ncclSend/ncclRecv issued by the engine (RCCL)" if db.transport == "rccl" else
                                         f"torch.distributed P2P, backend {dist.get_backend() if dist else 'none'}") + ")",
                       "exchanges_per_step": db.band.num_exchanges, "max_sent_MB_per_rank_per_step": round(sent / 1e6, 2),
                       "params": cfg.num_params(), "finite_outputs": finite},
            "roofline": None, "cpu_baseline": None,
        }
        print(json.dumps(out), flush=True)
    grp.close()


if __name__ == "__main__":
    main()
