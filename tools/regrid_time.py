#!/usr/bin/env python
"""Time the regridding block (csrc/wx_regrid.h) with HIP events on 4 x 127 + 8 planes (four 3-D variables of 127 levels and eight
2-D variables) of the 721 x 1440 grid:
  cons    721 x 1440 -> 181 x 360 conservative (the outer product of 1-D overlap fractions: about 25 entries per row)
  bilin   721 x 1440 -> 640 x 1280 bilinear, periodic in longitude (up to 4 entries per row)
  long    `cons` with every 64th destination row replaced by a 1 000-entry row: the long-row launch's share, as the difference to
          the same matrix with those rows emptied
Warm-up, repeats, median of HIP-event times.  Per case: one wx_regrid_apply for all twelve variables into preallocated outputs, the
same through the host block (dict handling and output allocation included), the bytes the call must move (every source plane read
once + every output plane; the matrix itself is not counted) and the rate against them.  Beside it, on the same GPU and with the same
coalesced matrix: what the reference does when its batch lives on the device, torch.sparse.mm with the two transposes of `_regrid`
(regrid.py:166-172), variable by variable.

    python tools/regrid_time.py [--reps 50] [--warmup 5] [--torch-reps 5] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "miles-credit_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from diag_time import timed  # noqa: E402

SRC_HW = (721, 1440)


def overlap_triplets(n_src, n_dst):
    """-> (dst index, src index, fraction of the destination cell) of the overlapping cell pairs of two uniform 1-D grids."""
    es, ed = np.arange(n_src + 1) / n_src, np.arange(n_dst + 1) / n_dst
    f = np.clip(np.minimum(es[None, 1:], ed[1:, None]) - np.maximum(es[None, :-1], ed[:-1, None]), 0.0, None) * n_dst
    d, s = np.nonzero(f)
    return d, s, f[d, s]


def conservative(dst_hw):
    (H, W), (h, w) = SRC_HW, dst_hw
    dy, sy, fy = overlap_triplets(H, h)
    dx, sx, fx = overlap_triplets(W, w)
    row = (dy[:, None] * w + dx[None, :]).ravel()
    col = (sy[:, None] * W + sx[None, :]).ravel()
    return row + 1, col + 1, (fy[:, None] * fx[None, :]).ravel(), H * W, h * w


def bilinear(dst_hw):
    (H, W), (h, w) = SRC_HW, dst_hw
    lat, lon = np.linspace(-90.0, 90.0, h), np.arange(w) * (360.0 / w)
    dlat, dlon = 180.0 / (H - 1), 360.0 / W
    i0 = np.minimum(((lat + 90.0) // dlat).astype(np.int64), H - 2)
    t = (lat + 90.0 - i0 * dlat) / dlat
    j0 = (lon // dlon).astype(np.int64)
    s = (lon - j0 * dlon) / dlon
    j1 = (j0 + 1) % W
    r = (np.arange(h)[:, None] * w + np.arange(w)[None, :]).ravel()
    rows, cols, S = [], [], []
    for ii, wi in ((i0, 1 - t), (i0 + 1, t)):
        for jj, wj in ((j0, 1 - s), (j1, s)):
            rows.append(r)
            cols.append((ii[:, None] * W + jj[None, :]).ravel())
            S.append((wi[:, None] * wj[None, :]).ravel())
    rows, cols, S = np.concatenate(rows), np.concatenate(cols), np.concatenate(S)
    keep = S != 0.0
    return rows[keep] + 1, cols[keep] + 1, S[keep], H * W, h * w


def with_long_rows(row, col, S, n_a, n_b, entries=1000, empty=False):
    """Every 64th destination row replaced by a row of `entries` entries at random source points (or by an empty row)."""
    g = np.random.Generator(np.random.Philox(key=[2028, 7]))
    long_rows = np.arange(0, n_b, 64)
    keep = ((row - 1) % 64) != 0
    row, col, S = row[keep], col[keep], S[keep]
    if empty:
        return row, col, S, n_a, n_b
    lr = np.repeat(long_rows, entries)
    lc = np.concatenate([g.choice(n_a, size=entries, replace=False) for _ in long_rows])
    return (np.concatenate([row, lr + 1]), np.concatenate([col, lc + 1]), np.concatenate([S, np.full(lr.size, 1.0 / entries)]), n_a, n_b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("regrid_time: no GPU visible; a time is measured on the GPU or not at all")
    from wxengine.engine import _stream_ptr
    from wxengine.regrid import Regridder
    H, W = SRC_HW
    src = "GFS"
    keys = [f"{src}/prognostic/3d/v{i}" for i in range(4)] + [f"{src}/prognostic/2d/s{i}" for i in range(8)]
    g = torch.Generator(device="cuda").manual_seed(1)
    fields = [torch.rand(1, 127, H, W, device="cuda", generator=g) for _ in range(4)] + \
             [torch.rand(1, 1, H, W, device="cuda", generator=g) for _ in range(8)]
    planes = sum(f.shape[1] for f in fields)
    cons = conservative((181, 360))
    cases = (("cons", (181, 360), cons), ("bilin", (640, 1280), bilinear((640, 1280))),
             ("long", (181, 360), with_long_rows(*cons)), ("long_emptied", (181, 360), with_long_rows(*cons, empty=True)))
    results = {}
    for name, (h, w), (row, col, S, n_a, n_b) in cases:
        blk = Regridder(variables=keys, row=row, col=col, S=S, n_a=n_a, n_b=n_b, dst_grid_dims=[w, h])
        lens = np.diff(blk.row_ptr)

        def run():
            return blk({"input": {src: dict(zip(keys, fields))}})
        y_blk = run()["input"][src]
        med, lo, hi = timed(run, args.warmup, args.reps)
        outs = [torch.empty(1, f.shape[1], h, w, device="cuda") for f in fields]
        n = len(fields)
        c_src, c_bs = (C.c_void_p * n)(*[f.data_ptr() for f in fields]), (C.c_int64 * n)()
        c_ppi, c_dst = (C.c_int32 * n)(*[f.shape[1] for f in fields]), (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        handle = blk._handle(0, (H, W), ())

        def raw():
            st = blk.lib.wx_regrid_apply(handle, n, c_src, c_bs, c_ppi, 1, c_dst, _stream_ptr(0))
            assert st == 0, blk.lib.wx_last_error()
        rmed, rlo, rhi = timed(raw, args.warmup, args.reps)
        assert all(torch.equal(o, y_blk[k]) for o, k in zip(outs, keys))
        nbytes = 4 * planes * (n_a + n_b)
        res = {"case": name, "grid": [H, W], "dst": [h, w], "planes": planes, "variables": n, "entries": int(lens.sum()),
               "row_entries_min_mean_max": [int(lens.min()), round(float(lens.mean()), 1), int(lens.max())],
               "long_rows": int((lens > 64).sum()), "apply_us": round(rmed * 1e3, 1), "apply_us_min": round(rlo * 1e3, 1),
               "apply_us_max": round(rhi * 1e3, 1), "block_us": round(med * 1e3, 1), "block_us_min": round(lo * 1e3, 1),
               "block_us_max": round(hi * 1e3, 1), "bytes": nbytes, "apply_GBps": round(nbytes / (rmed * 1e-3) / 1e9, 1),
               "reps": args.reps}
        if not name.startswith("long"):
            try:
                idx = torch.from_numpy(np.stack([np.repeat(np.arange(n_b), lens), blk.col.astype(np.int64)])).cuda()
                Wm = torch.sparse_coo_tensor(idx, torch.from_numpy(blk.val).cuda(), size=(n_b, n_a)).coalesce()

                def ref():
                    out = []
                    for f in fields:                       # regrid.py:166-172, variable by variable as forward() does
                        y_flat = torch.sparse.mm(Wm, f.reshape(-1, n_a).T).T
                        out.append(y_flat.reshape(*f.shape[:-2], h, w))
                    return out
                y_ref = ref()
                tmed, tlo, thi = timed(ref, 1, args.torch_reps)
                err = max(float((a - b).abs().max()) for a, b in zip(y_ref, outs))
                res.update(torch_sparse_mm_us=round(tmed * 1e3, 1), torch_sparse_mm_us_min=round(tlo * 1e3, 1),
                           torch_sparse_mm_us_max=round(thi * 1e3, 1), speedup_vs_torch_sparse_mm=round(tmed / rmed, 2),
                           max_abs_difference_to_torch=err)
            except Exception as e:     # reported, not hidden: the comparison is part of the result
                res["torch_sparse_mm_error"] = f"{type(e).__name__}: {e}"[:300]
        results[name] = res
        if name == "long_emptied":
            share = (results["long"]["apply_us"] - res["apply_us"]) / results["long"]["apply_us"]
            res["long_row_launch_share_of_long_case"] = round(share, 3)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del blk, outs, y_blk


if __name__ == "__main__":
    main()
