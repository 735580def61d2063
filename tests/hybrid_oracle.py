"""Plain-torch restatement of the hybrid-level interpolation (credit/postblock/hybrid_interp.py over
credit/postblock/_interp_utils.py), in fp32 or fp64, on the tensors as they lie ([B, L, n_time, H, W]): no vmap, no permute, no chunks.
Pinned to the reference's own classes by tests/test_hybrid_vs_reference.py and to its goldens by tests/test_hybrid_oracle.py.

`mutation` breaks one rule at a time, for the test that shows the goldens catch it."""
import numpy as np
import torch

MIN_PRESSURE_PA = 0.57      # hybrid_interp.py:29
MUTATIONS = ("flip forgotten", "weight not clamped", "hi not clamped", "linear in p", "floor missing", "sorted output order")
COEFFICIENT_MUTATIONS = ("interfaces not averaged", "levels before averaging")


def midpoint_coefficients(a, b=None, on_interfaces=True, levels=None, mutation=None):
    """_interp_utils.py:69-80 on arrays: float64, the vcoord rows, interface averaging, the 1-based subset, the float32 cast."""
    a = np.asarray(a, np.float64)
    if b is None:
        a, b = a[0], a[1]
    b = np.asarray(b, np.float64)
    idx = None if levels is None else [lv - 1 for lv in levels]
    if mutation == "levels before averaging" and idx is not None and on_interfaces:
        a, b = a[idx + [idx[-1] + 1]], b[idx + [idx[-1] + 1]]
        idx = None
    if on_interfaces:
        if mutation == "interfaces not averaged":
            a, b = a[1:], b[1:]
        else:
            a, b = 0.5 * (a[:-1] + a[1:]), 0.5 * (b[:-1] + b[1:])
    if idx is not None:
        a, b = a[idx], b[idx]
    return torch.from_numpy(a.astype(np.float32)), torch.from_numpy(b.astype(np.float32))


def interp(fields, sp, source_a, source_b, dest_a, dest_b, dtype=torch.float32, mutation=None):
    """fields: {name: [B, Ls, T, H, W]} in stored level order, sp [B, 1, T, H, W], coefficients: float32 midpoint values in stored
    order (midpoint_coefficients) -> {name: [B, Ld, T, H, W]} of `dtype`, in the destination's stored order."""
    sa, sb, da, db = (torch.as_tensor(x, dtype=torch.float32) for x in (source_a, source_b, dest_a, dest_b))
    ref = sa + sb * 101325.0                                   # :102, float32
    flip = bool(ref[0] > ref[-1]) and mutation != "flip forgotten"
    coef_flip = bool(ref[0] > ref[-1])
    if coef_flip:
        sa, sb = torch.flip(sa, (0,)), torch.flip(sb, (0,))    # :105-106
    Ls = sa.shape[0]
    sp = sp.to(dtype)
    lvl = lambda x: x.to(device=sp.device, dtype=dtype).view(1, -1, 1, 1, 1)  # noqa: E731
    floor = (lambda p: p) if mutation == "floor missing" else (lambda p: p.clamp(min=MIN_PRESSURE_PA))
    coord = (lambda p: p) if mutation == "linear in p" else torch.log
    x = coord(floor(lvl(sa) + lvl(sb) * sp))                   # :61   [B, Ls, T, H, W]
    xq = coord(floor(lvl(da) + lvl(db) * sp))                  # :62   [B, Ld, T, H, W]
    cnt = (xq.unsqueeze(2) >= x.unsqueeze(1)).sum(dim=2)       # _interp_utils.py:33
    hi = cnt if mutation == "hi not clamped" else cnt.clamp(min=1, max=Ls - 1)     # unclamped: torch.gather raises out of range
    lo = hi - 1
    x_lo, x_hi = torch.gather(x, 1, lo), torch.gather(x, 1, hi)
    w = (xq - x_lo) / (x_hi - x_lo)
    if mutation != "weight not clamped":
        w = w.clamp(0.0, 1.0)                                  # :37
    out = {}
    for name, t in fields.items():
        t = t.to(dtype)
        if flip:
            t = torch.flip(t, (1,))                            # hybrid_interp.py:134
        y_lo, y_hi = torch.gather(t, 1, lo), torch.gather(t, 1, hi)
        y = y_lo + w * (y_hi - y_lo)                           # :40
        if mutation == "sorted output order":
            y = y[:, torch.argsort(da + db * 101325.0, stable=True)]
        out[name] = y
    return out
