"""Torch restatement of the semi-Lagrangian advection as the device runs it (csrc/wx_advect.h) in a chosen dtype and on a chosen
device: the oracle of tests/test_advect_*.py in fp32 and fp64 on the CPU, and on the GPU the torch chain tools/advect_time.py times the
device block against.

Written from the formulas, not from the reference's code; all fields [B, L, H, W], levels top -> surface:
    p_half = a_half + b_half sp,  dp = p_half[k + 1] - p_half[k],  p_c = (p_half[k] + p_half[k + 1]) / 2
    div    = (dU/dlon + d(V cos lat)/dlat) / (R max(cos lat, floor)): dU/dlon periodic and centred over 2 dlon, d/dlat the
             second-order difference for non-uniform latitudes, one-sided on the first and the last row
    omega  = -(S[k - 1] + S[k]) / 2 with S the running sum of div dp over the levels, S[-1] = 0     (or given)
    V      = (U / (R cos) / dlon,  V / R / dlat_row,  omega / max(dp_c/dlevel, floor))     in columns, rows, levels per second
    disp   = 0;  n_iterations times: disp = dt V(x0 - disp / 2);  out = tracer(x0 - disp)
V(x) and tracer(x) are trilinear in INDEX space: the column a floating remainder modulo W with neighbours i, (i + 1) mod W; row and
level clamped to [0, n - 1] with upper neighbour min(i + 1, n - 1) -- no halo, no normalised coordinates; three nested lerps
a + f (b - a), column first, so equal neighbours give their own bits."""
import math

import torch

RAD_EARTH = 6371000.0


def lat_gradient(f, lat_rad):
    """d f / d lat along dim -2 on the (possibly non-uniform) coordinates lat_rad [H]."""
    dx = lat_rad[1:] - lat_rad[:-1]
    hl, hr = dx[:-1].view(-1, 1), dx[1:].view(-1, 1)
    a, b, c = -hr / (hl * (hl + hr)), (hr - hl) / (hl * hr), hl / (hr * (hl + hr))
    mid = a * f[..., :-2, :] + b * f[..., 1:-1, :] + c * f[..., 2:, :]
    first = (f[..., 1:2, :] - f[..., 0:1, :]) / dx[0]
    last = (f[..., -1:, :] - f[..., -2:-1, :]) / dx[-1]
    return torch.cat([first, mid, last], dim=-2)


def unit_gradient(f, dim):
    """Centred over two points in the interior, one-sided at both ends, unit spacing."""
    n = f.shape[dim]
    lo, hi = f.narrow(dim, 0, 1), f.narrow(dim, n - 1, 1)
    first, last = f.narrow(dim, 1, 1) - lo, hi - f.narrow(dim, n - 2, 1)
    if n == 2:
        return torch.cat([first, last], dim=dim)
    mid = (f.narrow(dim, 2, n - 2) - f.narrow(dim, 0, n - 2)) / 2
    return torch.cat([first, mid, last], dim=dim)


def velocities(u, v, sp, omega, a_half, b_half, lat_deg, lon_deg, coslat_floor=1e-4, dp_dlevel_floor=1.0):
    """u, v [B, L, H, W], sp [B, H, W], omega [B, L, H, W] or None -> index-space velocity [B, L, H, W, 3] (column, row, level)."""
    dtype, dev = u.dtype, u.device
    lat_rad = torch.as_tensor(lat_deg, dtype=dtype, device=dev) * (math.pi / 180.0)
    lon = torch.as_tensor(lon_deg, dtype=dtype, device=dev)
    dlon = (lon[1] - lon[0]) * (math.pi / 180.0)
    dlat_row = unit_gradient(lat_rad, 0).view(-1, 1)
    coslat = torch.cos(lat_rad).view(-1, 1)
    r_cos = RAD_EARTH * coslat.clamp(min=coslat_floor)
    a = torch.as_tensor(a_half, dtype=dtype, device=dev).view(1, -1, 1, 1)
    b = torch.as_tensor(b_half, dtype=dtype, device=dev).view(1, -1, 1, 1)
    p_half = a + b * sp.unsqueeze(1)
    p_c = 0.5 * (p_half[:, :-1] + p_half[:, 1:])
    if omega is None:
        dudlon = (torch.roll(u, -1, dims=-1) - torch.roll(u, 1, dims=-1)) / (2.0 * dlon)
        div = (dudlon + lat_gradient(v * coslat, lat_rad)) / r_cos
        s = torch.cumsum(div * (p_half[:, 1:] - p_half[:, :-1]), dim=1)
        upper = torch.cat([torch.zeros_like(s[:, :1]), -s[:, :-1]], dim=1)
        omega = 0.5 * (upper + -s)
    dpdl = unit_gradient(p_c, 1).clamp(min=dp_dlevel_floor)
    return torch.stack([u / r_cos / dlon, v / RAD_EARTH / dlat_row, omega / dpdl], dim=-1)


def sample(vol, col, row, lev):
    """vol [B, L, H, W, C] at the index-space points col, row, lev [B, L, H, W] -> [B, L, H, W, C]."""
    B, L, H, W, C = vol.shape
    x = torch.remainder(col, W)
    i0 = torch.floor(x)
    fx = (x - i0).unsqueeze(-1)
    i0 = i0.long() % W               # a tiny negative remainder rounds to W itself: column 0, weight 0
    i1 = (i0 + 1) % W
    y = row.clamp(0.0, H - 1)
    j0 = torch.floor(y)
    fy = (y - j0).unsqueeze(-1)
    j0 = j0.long()
    j1 = (j0 + 1).clamp(max=H - 1)
    z = lev.clamp(0.0, L - 1)
    k0 = torch.floor(z)
    fz = (z - k0).unsqueeze(-1)
    k0 = k0.long()
    k1 = (k0 + 1).clamp(max=L - 1)
    flat = vol.reshape(B * L * H * W, C)
    base = torch.arange(B, device=vol.device).view(B, 1, 1, 1) * L

    def at(k, j, i):
        return flat[((base + k) * H + j) * W + i]

    def lerp(p, q, f):
        return p + f * (q - p)
    planes = [lerp(lerp(at(k, j0, i0), at(k, j0, i1), fx), lerp(at(k, j1, i0), at(k, j1, i1), fx), fy) for k in (k0, k1)]
    return lerp(planes[0], planes[1], fz)


def departure(vel, dt, n_iterations):
    """vel [B, L, H, W, 3] -> (column, row, level) of the departure point of every grid point, each [B, L, H, W]."""
    B, L, H, W, _ = vel.shape
    kw = dict(dtype=vel.dtype, device=vel.device)
    col0 = torch.arange(W, **kw).view(1, 1, 1, W).expand(B, L, H, W)
    row0 = torch.arange(H, **kw).view(1, 1, H, 1).expand(B, L, H, W)
    lev0 = torch.arange(L, **kw).view(1, L, 1, 1).expand(B, L, H, W)
    disp = torch.zeros_like(vel)
    for _ in range(n_iterations):
        disp = dt * sample(vel, col0 - 0.5 * disp[..., 0], row0 - 0.5 * disp[..., 1], lev0 - 0.5 * disp[..., 2])
    return col0 - disp[..., 0], row0 - disp[..., 1], lev0 - disp[..., 2]


def advect(fields, u_key, v_key, sp_key, tracers, a_half, b_half, lat_deg, lon_deg, dt=21600.0, n_iterations=2, omega_key=None,
           level_order="top_to_surface", coslat_floor=1e-4, dp_dlevel_floor=1.0, dtype=None, want_departure=False):
    """fields {key: [B, L, 1, H, W]} (sp: [B, 1, 1, H, W]) -> {tracer key: advected [B, L, 1, H, W]}; the inputs are not modified.
    a_half / b_half are the L + 1 half-level coefficients top -> surface whatever `level_order`."""
    flip = level_order == "surface_to_top"

    def prep(key):
        t = fields[key] if dtype is None else fields[key].to(dtype)
        t = t[:, :, 0]
        return t.flip(1) if flip else t
    u, v = prep(u_key), prep(v_key)
    sp = (fields[sp_key] if dtype is None else fields[sp_key].to(dtype))[:, 0, 0]
    vel = velocities(u, v, sp, prep(omega_key) if omega_key is not None else None, a_half, b_half, lat_deg, lon_deg, coslat_floor,
                     dp_dlevel_floor)
    dep = departure(vel, dt, n_iterations)
    vol = torch.stack([prep(k) for k in tracers], dim=-1)
    got = sample(vol, *dep)
    out = {}
    for i, k in enumerate(tracers):
        o = got[..., i]
        out[k] = (o.flip(1) if flip else o).unsqueeze(2).contiguous()
    return (out, dep) if want_departure else out
