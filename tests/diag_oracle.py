"""Torch restatement of the pressure-level products (csrc/wx_diag.h) in a chosen dtype: the oracle of tests/test_diag_*.py.

Whole tensors at once, levels on dim 1 of [B, L, T, H, W]; no vmap, no permute.  It states what the reference's three column
functions compute (credit/postblock/geopotential.py:37-83, pressure_interp.py:44-130 over _interp_utils.py:14-40, mslp.py:33-80) and is
pinned to them by tests/test_diag_vs_reference.py and, through the fixtures, by tests/test_diag_oracle.py."""
import torch

GRAVITY, RDGAS, LAPSE = 9.80665, 287.05, 0.0065
ALPHA_STD = LAPSE * RDGAS / GRAVITY
GEO_RD, GEO_RV = 287.06, 461.51          # the hydrostatic integral's own gas constants
P_TOP = 0.57


def _col(v, like):
    return torch.as_tensor(v).to(dtype=like.dtype, device=like.device).reshape(1, -1, 1, 1, 1)


def geopotential(T, q, sp, phis, a_half, b_half, flip_vertical=True):
    """Geopotential on model levels [B, L, T, H, W].  Layer k lies between interfaces k and k + 1; the sum starts at stored layer
    L - 1 (flip_vertical) or 0 and runs through the stored order."""
    ph = _col(a_half, T) + _col(b_half, T) * sp
    ph = torch.where(ph > 0, ph, torch.full_like(ph, P_TOP))
    up, lo = ph[:, :-1], ph[:, 1:]
    dlogp = torch.log(lo / up)
    alpha = 1.0 - up / (lo - up) * dlogp
    rtv = GEO_RD * (T * (1.0 + (GEO_RV / GEO_RD - 1.0) * q))
    term = rtv * dlogp
    if flip_vertical:
        run = torch.cumsum(term.flip(1), dim=1).flip(1)
    else:
        run = torch.cumsum(term, dim=1)
    return phis + run - rtv * alpha


def to_pressure_levels(fields, T, Z, sp, phis, a_mid, b_mid, plev_pa, temp_height=150.0):
    """-> list of [B, n_plev, T, H, W]: every field (constant extrapolation), then T and Z (Trenberth below ground).  Levels may be
    stored either way round; the orientation is read off the coefficients at 101 325 Pa."""
    a, b = _col(a_mid, T).flatten(), _col(b_mid, T).flatten()
    if bool(a[0] + b[0] * 101325.0 > a[-1] + b[-1] * 101325.0):
        a, b = a.flip(0), b.flip(0)
        fields, T, Z = [f.flip(1) for f in fields], T.flip(1), Z.flip(1)
    L = T.shape[1]
    pres = _col(a, T) + _col(b, T) * sp                      # [B, L, T, H, W], rising with the index
    logp = torch.log(pres)
    pq = _col(plev_pa, T)                                     # [1, P, 1, 1, 1]
    logq = torch.log(pq)
    # bracket: hi = number of levels at or below the target in log p, kept inside [1, L - 1]
    hi = (logq.unsqueeze(2) >= logp.unsqueeze(1)).sum(dim=2).clamp(1, L - 1)      # [B, P, T, H, W]
    lo = hi - 1
    x_lo, x_hi = torch.gather(logp, 1, lo), torch.gather(logp, 1, hi)
    w = ((logq - x_lo) / (x_hi - x_lo)).clamp(0.0, 1.0)

    def lerp(y):
        y_lo, y_hi = torch.gather(y, 1, lo), torch.gather(y, 1, hi)
        return y_lo + w * (y_hi - y_lo)
    out = [lerp(f) for f in fields]
    # surface temperature from the level nearest temp_height above ground (first minimum)
    h = torch.argmin(torch.abs((Z - phis) / GRAVITY - temp_height), dim=1, keepdim=True)
    t_h, p_h = torch.gather(T, 1, h), torch.gather(pres, 1, h)
    ts = t_h + ALPHA_STD * t_h * (sp / p_h - 1.0)
    sh = phis / GRAVITY
    tsl = ts + LAPSE * sh
    tpl = tsl.clamp(max=298.0)
    g_sgp = GRAVITY / phis.clamp(min=1.0)
    t_adj = 0.002 * ((2500.0 - sh) * tsl + (sh - 2000.0) * tpl)
    gamma = torch.where(sh > 2500.0, g_sgp * (tpl - ts).clamp(min=0.0),
                        torch.where(sh >= 2000.0, g_sgp * (t_adj - ts), torch.full_like(ts, LAPSE)))
    ln = torch.log(pq / sp)
    x = gamma * RDGAS / GRAVITY * ln
    t_below = ts * (1.0 + x + 0.5 * x ** 2 + x ** 3 / 6.0)
    z_below = phis - RDGAS * ts * ln * (1.0 + 0.5 * x + x ** 2 / 6.0)
    below = pq > sp
    out.append(torch.where(below, t_below, lerp(T)))
    out.append(torch.where(below, z_below, lerp(Z)))
    return out


def mslp(sp, t, phis):
    height = phis / GRAVITY
    tto = t + LAPSE * height
    case1 = (t <= 290.5) & (tto > 290.5)
    warm = t > 290.5
    cold = (t < 255.0) & ~case1 & ~warm
    alpha = torch.full_like(t + phis, ALPHA_STD)
    alpha = torch.where(case1, RDGAS * (290.5 - t) / phis.clamp(min=1e-6), alpha)
    alpha = torch.where(warm, torch.zeros_like(alpha), alpha)
    te = torch.where(warm, 0.5 * (290.5 + t), t)
    te = torch.where(cold, 0.5 * (255.0 + t), te)
    x = phis / (RDGAS * te.clamp(min=1.0))
    value = sp * torch.exp(x * (1.0 - 0.5 * alpha * x + (alpha * x) ** 2 / 3.0))
    return torch.where(height.abs() < 1e-4, sp + torch.zeros_like(value), value)


def all_products(inp, case, dtype):
    """Every output variable of a fixture case (tests/diag_cases.py) -> {name: numpy array}."""
    from diag_cases import FIELD_ORDER
    t = {k: torch.from_numpy(v).to(dtype) for k, v in inp.items() if k in ("T", "q", "u", "v", "sp", "t2m", "phis")}
    z = geopotential(t["T"], t["q"], t["sp"], t["phis"], inp["a_half"], inp["b_half"], case["flip_vertical"])
    names = FIELD_ORDER[:case["n_fields"]]
    pl = to_pressure_levels([t[f] for f in names], t["T"], z, t["sp"], t["phis"], inp["a_mid"], inp["b_mid"], inp["plev_pa"])
    out = {"z_model": z, "mslp": mslp(t["sp"], t["t2m"], t["phis"])}
    for f, v in zip(list(names) + ["T", "Z"], pl):
        out[f"plev_{f}"] = v
    return {k: v.numpy() for k, v in out.items()}
