#!/usr/bin/env python
"""Time the zonal spectra (csrc/wx_spectrum.h) with HIP events: `ZonalSpectrum.submit` on 64 planes of 721 x 1440 and of 181 x 360
(prediction and target: two launches, the async copy of the table and the ctypes call included), `psd` of one field, the same
quantities through torch.fft.rfft in float32 on the same GPU (what the reference runs when its tensors are on the device), and the
copy of one field to the host that a host-side spectrum would start with.  Warm-up, repeats, median / min / max.  FLOP are counted
from the shapes: after the fold a row takes Wh values of x into Wh cos and Wh sin sums, 2 * 2 * Wh * Wh per row and field; the
fraction is of the MI355X's 78.6 TFLOP/s of fp64 matrix peak.

    python tools/spectrum_time.py [--reps 5] [--warmup 2] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "miles-credit_amd"), ROOT]

import torch  # noqa: E402

from diag_time import timed  # noqa: E402

PLANES = 64
FP64_MATRIX_PEAK = 78.6e12


def folded_flop(H, W, fields):
    """FLOP of one plane of `fields` fields."""
    Wh = W // 2 + 1
    return fields * H * 2 * 2 * Wh * Wh


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
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spectrum_time: no GPU visible; a time is measured on the GPU or not at all")
    from spectrum_cases import latitudes
    from wxengine.spectrum import ZonalSpectrum
    for H, W in ((181, 360), (721, 1440)):
        gen = torch.Generator(device="cuda").manual_seed(1)
        pred = 250.0 + 3.0 * torch.cumsum(torch.randn((PLANES, H, W), device="cuda", generator=gen), dim=-1)
        target = pred + 0.5 * torch.randn((PLANES, H, W), device="cuda", generator=gen)
        spec = ZonalSpectrum(H, W, latitude=latitudes(H))
        k_init = 20
        last = []

        def device():
            last[:] = [spec.submit(pred, target, k_init)]
        med, lo, hi = timed(device, args.warmup, args.reps)
        res = last[0].result()
        assert res.psd_score.shape == (PLANES,) and (res.psd_score > 0).all() and (res.ratio > 0).all()
        pmed, plo, phi = timed(lambda: spec.psd(pred), args.warmup, args.reps)
        w = torch.from_numpy(spec.lat_weights).cuda()

        def vendor():
            fp, ft = torch.fft.rfft(pred, dim=-1), torch.fft.rfft(target, dim=-1)
            mult = torch.full((W // 2 + 1,), 2.0, device="cuda")
            mult[0] = 1.0
            pp, pt = (fp.real ** 2 + fp.imag ** 2) * mult / W ** 2, (ft.real ** 2 + ft.imag ** 2) * mult / W ** 2
            d = (torch.log(pp + 1e-8) - torch.log(pt + 1e-8))[..., k_init:] ** 2
            s0 = torch.matmul(w / w.sum(), d).mean(dim=-1)
            ma, mb = torch.matmul(w, torch.abs(fp)) / H, torch.matmul(w, torch.abs(ft)) / H
            return s0, ((ma - mb)[..., k_init:] ** 2).mean(dim=-1), torch.matmul(w / w.sum(), pp), torch.matmul(w / w.sum(), pt)
        vmed, vlo, vhi = timed(vendor, args.warmup, args.reps)
        s0 = vendor()[0].double().cpu().numpy()
        host = torch.empty(pred.shape, dtype=torch.float32, pin_memory=True)
        cmed, clo, chi = timed(lambda: host.copy_(pred, non_blocking=True), args.warmup, args.reps)
        flop = PLANES * folded_flop(H, W, 2)
        emit({"what": "zonal spectra, compare", "grid": [H, W], "planes": PLANES, "compare_ms": round(med, 3), "compare_ms_min": round(lo, 3),
              "compare_ms_max": round(hi, 3), "folded_GFLOP": round(flop / 1e9, 1), "TFLOP_per_s": round(flop / (med * 1e-3) / 1e12, 2),
              "fraction_of_fp64_matrix_peak": round(flop / (med * 1e-3) / FP64_MATRIX_PEAK, 3), "psd_one_field_ms": round(pmed, 3),
              "psd_one_field_ms_min": round(plo, 3), "psd_one_field_ms_max": round(phi, 3), "torch_fft_f32_ms": round(vmed, 3),
              "torch_fft_f32_ms_min": round(vlo, 3), "torch_fft_f32_ms_max": round(vhi, 3),
              "torch_fft_f32_psd_score_rel_diff": float(abs(s0 - res.psd_score).max() / res.psd_score.max()),
              "copy_one_field_to_host_ms": round(cmed, 3), "copy_one_field_to_host_ms_min": round(clo, 3),
              "copy_one_field_to_host_ms_max": round(chi, 3), "reps": args.reps}, args.out)
        del pred, target, host


if __name__ == "__main__":
    main()
