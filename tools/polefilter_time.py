#!/usr/bin/env python
"""Time the diffusion and pole filter (csrc/wx_polefilter.h) with HIP events: diff_lap2d_filt on a 70-channel float32 tensor at
181 x 360 (equiangular), 640 x 1280 (legendre-gauss) and 721 x 1440 (equiangular), the inverse vector transform of 64 planes, and the
same composition through torch.fft plus fp64 torch.einsum against the same tables, unfolded, on the same GPU (the restatement of
tools/sht_time.py).  Warm-up, repeats, median / min / max, one JSON line per grid.  The fields are smooth (a forecast, not noise) and
the radius is the Earth's, as in the reference's use.

    python tools/polefilter_time.py [--reps 3] [--warmup 1] [--grids 181x360:equiangular,640x1280:legendre-gauss,721x1440:equiangular] [--out FILE]"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "miles-credit_amd"), ROOT]

import torch  # noqa: E402

from diag_time import timed  # noqa: E402
from sht_time import emit, torch_tables  # noqa: E402

PLANES = 64


class TorchFilter:
    """The filter restated with torch.fft and fp64 einsum against unfolded tables: what the reference does with device tensors."""

    def __init__(self, dpf):
        self.d, self.W = dpf, dpf.nlon
        self.P, self.dP, self.Q = torch_tables(dpf.lmax, dpf.mmax, dpf.theta, True)
        self.w = torch.as_tensor(dpf.w, device="cuda")
        l = torch.arange(dpf.lmax, dtype=torch.float64, device="cuda")[:, None]
        self.sq = torch.sqrt(l * (l + 1))
        self.sig = torch.as_tensor(dpf.sigmoid, device="cuda").double()[:, None]

    def dft(self, x):
        return torch.fft.rfft(x, dim=-1)[..., :self.d.mmax] * (2 * math.pi / self.W)

    def lon(self, F):
        return torch.fft.irfft(F, n=self.W, dim=-1, norm="forward")

    def analysis(self, x):
        return torch.view_as_complex(torch.einsum("mlk,k,pkmr->plmr", self.P, self.w, torch.view_as_real(self.dft(x))).contiguous())

    def inv(self, table, c):
        return torch.view_as_complex(torch.einsum("mlk,plmr->pkmr", table, torch.view_as_real(c)).contiguous())

    def grad(self, c):
        s = self.sq * c / self.d.radius
        return self.lon(1j * self.inv(self.Q, s)), -self.lon(self.inv(self.dP, s))

    def div(self, u, v):
        Fu, Fv = torch.view_as_real(self.dft(u)), torch.view_as_real(self.dft(v))
        dv = torch.view_as_complex(torch.einsum("mlk,k,pkmr->plmr", self.dP, self.w, Fv).contiguous())
        qu = torch.view_as_complex(torch.einsum("mlk,k,pkmr->plmr", self.Q, self.w, Fu).contiguous())
        return -self.sq * (-dv - 1j * qu) / self.d.radius

    def L(self, c):
        gx, gy = self.grad(c)
        return self.grad(self.analysis(gx))[0] + self.grad(self.analysis(gy))[1]

    def lowpass(self, x):
        i = self.d.cutoff
        if i == 0:
            return x
        rows = list(range(1, 11)) + list(range(self.d.nlat - 10, self.d.nlat))
        Z = torch.fft.fft(x[:, rows], dim=-1)
        Z[..., i:self.W - i] = 0
        x = x.clone()
        x[:, rows] = torch.fft.ifft(Z, dim=-1).real
        return x

    def scalar(self, x, n, coef):
        x = self.lowpass(x.double())
        for _ in range(n):
            x = x + self.L(self.analysis(x)) * self.sig * coef
        return x

    def vector(self, u, v, n, coef):
        u, v = self.lowpass(u.double()), self.lowpass(v.double())
        for _ in range(n):
            lx, ly = self.grad(self.analysis(self.L(self.div(u, v))))
            u, v = u - lx * self.sig * coef, v - ly * self.sig * coef
        return u, v

    def diff(self, B):
        out = B.clone()
        u, v = self.vector(B[0:16], B[16:32], 6, 2e16)
        out[0:16], out[16:32] = u, v
        out[32:48] = self.scalar(B[32:48], 5, 1e8)
        out[48:64] = self.scalar(B[48:64], 8, 0.5e8)
        out[64:66] = self.scalar(B[64:66], 5, 1e8)
        u, v = self.vector(B[67:68], B[66:67], 6, 2e16)
        out[67:68], out[66:67] = u, v
        out[68:69] = self.scalar(B[68:69], 5, 1e8)
        out[69:70] = self.scalar(B[69:70], 4, 0.5e8)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--grids", default="181x360:equiangular,640x1280:legendre-gauss,721x1440:equiangular")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch restatement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("polefilter_time: no GPU visible; a time is measured on the GPU or not at all")
    from wxengine.pole_filter import Diffusion_and_Pole_Filter
    for spec in args.grids.split(","):
        size, grid = spec.split(":")
        H, W = (int(v) for v in size.split("x"))
        dpf = Diffusion_and_Pole_Filter(H, W, "cuda", grid=grid)
        lat = torch.linspace(-1, 1, H, device="cuda")[:, None]
        lon = 2 * math.pi * torch.arange(W, device="cuda")[None, :] / W
        ch = torch.arange(70, device="cuda", dtype=torch.float32)[:, None, None]
        B = (250.0 + 20.0 * lat * torch.cos(2 * lon + 0.1 * ch) + 5.0 * torch.sin(5 * lon + 3 * lat + 0.2 * ch)).float().contiguous()
        out = dpf.diff_lap2d_filt(B)                               # builds the tables
        f_ms = timed(lambda: dpf.diff_lap2d_filt(B), args.warmup, args.reps)
        c = dpf.sht.analysis(B[:PLANES])
        vs_ms = timed(lambda: dpf.sht.vector_synthesis(c, c), args.warmup, args.reps)
        g_ms = timed(lambda: dpf.getgrad(c), args.warmup, args.reps)
        r3 = lambda t: [round(v, 3) for v in t]   # noqa: E731
        res = {"what": "diffusion and pole filter", "grid": [H, W], "nodes": grid, "lmax": dpf.lmax, "mmax": dpf.mmax, "cutoff_index": dpf.cutoff,
               "input": "float32", "diff_lap2d_filt_70ch_ms_med_min_max": r3(f_ms), "vector_synthesis_64_planes_ms_med_min_max": r3(vs_ms),
               "getgrad_64_planes_ms_med_min_max": r3(g_ms), "workspace_bytes_16_planes": dpf.workspace_bytes(16),
               "finite": bool(torch.isfinite(out).all()), "largest_change": float((out - B).abs().max()), "reps": args.reps}
        if not args.no_torch:
            tf = TorchFilter(dpf)
            ref = tf.diff(B)
            res["torch_diff_lap2d_filt_70ch_ms_med_min_max"] = r3(timed(lambda: tf.diff(B), args.warmup, args.reps))
            res["torch_getgrad_64_planes_ms_med_min_max"] = r3(timed(lambda: tf.grad(c), args.warmup, args.reps))
            res["max_abs_diff_vs_torch"] = float((out.double() - ref.double()).abs().max())
            del tf, ref
        emit(res, args.out)
        del dpf, B, out, c
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
