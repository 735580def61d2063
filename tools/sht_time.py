#!/usr/bin/env python
"""Time the spherical harmonic transforms (csrc/wx_sht.h) with HIP events: analysis, synthesis, vector analysis and
average_div_rot_spectrum of 64 float32 planes at 181 x 360 and 721 x 1440 (equiangular, lmax = nlat + 1 as in
credit/verification/standard.py), and the same quantities through torch.fft.rfft / irfft plus an fp64 torch.einsum against the same
tables, unfolded, on the same GPU -- what torch_harmonics does when its tensors are on the device.  Warm-up, repeats, median / min /
max, one JSON line per grid.  FLOP of the Legendre stage are counted from the shapes (folded rows, l >= m only); the fraction is of
the MI355X's 78.6 TFLOP/s of fp64 matrix peak.  The torch tables are built on the GPU by the same recurrence (a check of the two paths
against each other is part of the line); their bytes are reported next to the handle's.

    python tools/sht_time.py [--reps 5] [--warmup 2] [--grids 181x360,721x1440] [--out FILE]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "miles-credit_amd"), ROOT]

import torch  # noqa: E402

from diag_time import timed  # noqa: E402

PLANES = 64
FP64_MATRIX_PEAK = 78.6e12


def torch_tables(lmax, mmax, theta, vector, device="cuda"):
    """(P, dPt, Qt) float64 [mmax][lmax][nlat] on the GPU, no Condon-Shortley sign: the recurrence in l for every order at once."""
    M = mmax + 1
    th = torch.as_tensor(theta, dtype=torch.float64, device=device)
    x, s = torch.cos(th)[None, :], torch.sin(th)[None, :]
    m = torch.arange(M, dtype=torch.float64, device=device)[:, None]
    step = torch.sqrt((2 * m + 1) / (2 * m).clamp_min(1.0)) * s
    step[0] = 1.0 / math.sqrt(4 * math.pi)
    diag = torch.cumprod(step, dim=0)
    P = torch.zeros((M, lmax, th.numel()), dtype=torch.float64, device=device)
    mi = torch.arange(M, device=device)
    for l in range(lmax):
        a = torch.sqrt((4.0 * l * l - 1.0) / (l * l - m * m).clamp_min(1.0))
        b = torch.sqrt((((l - 1.0) ** 2 - m * m) / max(4.0 * (l - 1.0) ** 2 - 1.0, 1.0)).clamp_min(0.0))
        rec = a * (x * P[:, l - 1] - b * P[:, l - 2]) if l >= 2 else torch.zeros_like(diag)
        first = math.sqrt(2 * l + 1.0) * x * diag                    # taken for the order m = l - 1
        P[:, l] = torch.where((mi == l)[:, None], diag, torch.where((mi == l - 1)[:, None], first, torch.where((mi < l - 1)[:, None], rec, 0.0)))
    if not vector:
        return P[:mmax], None, None
    l = torch.arange(lmax, dtype=torch.float64, device=device)[None, :, None]
    mm = m[:mmax, :, None]
    lo = torch.cat([P[1:2], P[:mmax - 1]], dim=0)             # order m - 1 (m = 0: the slot is multiplied out below)
    hi = P[1:mmax + 1]
    norm = torch.sqrt(l * (l + 1)).clamp_min(1.0)
    d = (torch.sqrt(((l + mm) * (l - mm + 1)).clamp_min(0.0)) * lo - torch.sqrt(((l - mm) * (l + mm + 1)).clamp_min(0.0)) * hi) / 2
    d[0] = -torch.sqrt(l[0] * (l[0] + 1)) * hi[0]
    lo1, hi1 = torch.roll(lo, 1, 1), torch.roll(hi, 1, 1)    # degree l - 1
    lo1[:, 0], hi1[:, 0] = 0, 0
    q = torch.sqrt(((l - mm) * (l - mm - 1)).clamp_min(0.0)) * hi1 + torch.sqrt((l + mm) * (l + mm - 1).clamp_min(0.0)) * lo1
    q = torch.sqrt((2 * l + 1) / (2 * l - 1).clamp_min(1.0)) * q / 2
    q[0] = 0
    keep = (l >= mm) & (l >= 1)
    return P[:mmax], torch.where(keep, d / norm, 0.0), torch.where(keep, q / norm, 0.0)


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
    ap.add_argument("--grids", default="181x360,721x1440")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sht_time: no GPU visible; a time is measured on the GPU or not at all")
    from wxengine import sht as S
    for H, W in [tuple(int(v) for v in g.split("x")) for g in args.grids.split(",")]:
        lmax = H + 1
        gen = torch.Generator(device="cuda").manual_seed(1)
        x = 250.0 + 3.0 * torch.cumsum(torch.randn((PLANES, H, W), device="cuda", generator=gen), dim=-1)
        u, v = 10.0 * torch.randn((2, PLANES, H, W), device="cuda", generator=gen)
        sh = S.cached_transform(H, W, "equiangular", device=x.device)       # lmax = nlat + 1, csphase off: the module functions' own
        mmax, kk = sh.mmax, (H + 1) // 2
        c = sh.analysis(x)
        a_ms = timed(lambda: sh.analysis(x), args.warmup, args.reps)
        s_ms = timed(lambda: sh.synthesis(c), args.warmup, args.reps)
        st = sh.vector_analysis(u, v)                          # builds the vector tables
        v_ms = timed(lambda: sh.vector_analysis(u, v), args.warmup, args.reps)
        d_ms = timed(lambda: S.average_div_rot_spectrum(u, v, "equiangular"), args.warmup, args.reps)

        P, dP, Q = torch_tables(lmax, mmax, sh.theta, True)
        wq = torch.as_tensor(sh.w, device="cuda")
        scale = 2 * math.pi / W

        def t_analysis(f, table):
            F = torch.view_as_real(torch.fft.rfft(f.double(), dim=-1)[..., :mmax]) * scale
            return torch.einsum("mlk,k,pkmr->plmr", table, wq, F)

        def t_synthesis():
            F = torch.einsum("mlk,plmr->pkmr", P, torch.view_as_real(c))
            return torch.fft.irfft(torch.view_as_complex(F.contiguous()), n=W, dim=-1, norm="forward")

        def t_vector():
            Fu = torch.view_as_real(torch.fft.rfft(u.double(), dim=-1)[..., :mmax]) * scale
            Fv = torch.view_as_real(torch.fft.rfft(v.double(), dim=-1)[..., :mmax]) * scale
            du, dv = torch.einsum("mlk,k,pkmr->plmr", dP, wq, Fu), torch.einsum("mlk,k,pkmr->plmr", dP, wq, Fv)
            qu, qv = torch.einsum("mlk,k,pkmr->plmr", Q, wq, Fu), torch.einsum("mlk,k,pkmr->plmr", Q, wq, Fv)
            s = torch.stack((-dv[..., 0] + qu[..., 1], -dv[..., 1] - qu[..., 0]), dim=-1)
            t = torch.stack((du[..., 0] + qv[..., 1], du[..., 1] - qv[..., 0]), dim=-1)
            return s, t

        def t_div_rot():
            s, t = t_vector()
            mult = torch.full((mmax,), 2.0, device="cuda", dtype=torch.float64)
            mult[0] = 1.0
            return [((z ** 2).sum(dim=-1) * mult).sum(dim=-1).mean(dim=0).cpu() for z in (t, s)]

        ta_ms = timed(lambda: t_analysis(x, P), args.warmup, args.reps)
        ts_ms = timed(t_synthesis, args.warmup, args.reps)
        tv_ms = timed(t_vector, args.warmup, args.reps)
        td_ms = timed(t_div_rot, args.warmup, args.reps)
        ca = torch.view_as_complex(t_analysis(x, P).contiguous())
        ts, tt = t_vector()
        diff = lambda a, b: float((a - b).abs().max() / b.abs().max())   # noqa: E731
        flop = PLANES * 4.0 * kk * sum(lmax - m for m in range(mmax))
        table_bytes = 8 * kk * sum(lmax - m for m in range(mmax))
        r3 = lambda t: [round(v, 3) for v in t]   # noqa: E731
        emit({"what": "spherical harmonic transforms", "grid": [H, W], "lmax": lmax, "mmax": mmax, "planes": PLANES, "input": "float32",
              "analysis_ms_med_min_max": r3(a_ms), "synthesis_ms_med_min_max": r3(s_ms), "vector_analysis_ms_med_min_max": r3(v_ms),
              "average_div_rot_spectrum_ms_med_min_max": r3(d_ms),
              "torch_analysis_ms_med_min_max": r3(ta_ms), "torch_synthesis_ms_med_min_max": r3(ts_ms), "torch_vector_ms_med_min_max": r3(tv_ms),
              "torch_div_rot_spectrum_ms_med_min_max": r3(td_ms),
              "legendre_GFLOP_scalar": round(flop / 1e9, 2), "analysis_TFLOP_per_s_of_legendre_flop": round(flop / (a_ms[0] * 1e-3) / 1e12, 2),
              "analysis_fraction_of_fp64_matrix_peak": round(flop / (a_ms[0] * 1e-3) / FP64_MATRIX_PEAK, 4),
              "table_bytes_folded_scalar": table_bytes, "table_bytes_with_vector": 3 * table_bytes, "torch_table_bytes_each": P.numel() * 8,
              "rel_diff_analysis_vs_torch": diff(c, ca), "rel_diff_spheroidal_vs_torch": diff(st[0], torch.view_as_complex(ts.contiguous())),
              "rel_diff_toroidal_vs_torch": diff(st[1], torch.view_as_complex(tt.contiguous())),
              "rel_diff_synthesis_vs_torch": diff(sh.synthesis(c), t_synthesis()), "reps": args.reps}, args.out)
        del x, u, v, c, P, dP, Q, sh, st
        S.clear_cache()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
