"""Torch restatement of the wind artifact filter (csrc/wx_wind.h) in a chosen dtype and on a chosen device: the oracle of
tests/test_wind_*.py in fp32 and fp64 on the CPU, and on the GPU the torch chain tools/wind_time.py times the device block against.

Written from the formulas, not from the reference's code:
    flag = sqrt(u^2 + v^2) > threshold at the mask level            dilated = OR of flag over a dil_lat x dil_lon rectangle
    m    = dilated (*) N(falloff_sigma) x N(2 falloff_sigma), sizes int(4 s + 1) | 1 and int(8 s + 1) | 1, zero padded
    fs   = f (*) N(sig_lat) x N(sig_lon), sizes int(6 s + 1) | 1, zero padded
    alpha = min(sqrt(sum m f^2 / (sum m fs^2 + 1e-12)), 4) per batch item and plane (preserve_amplitude)
    out  = m (alpha fs) + (1 - m) f on the target levels that exist, the other levels unchanged
The dilation is a max-pool (an OR needs no sum), the Gaussians full 2-D zero-padded convolutions with the outer-product kernel."""
import torch
import torch.nn.functional as F


def gauss1d(sigma, size, dtype, device="cpu"):
    x = torch.arange(size, dtype=dtype, device=device) - size // 2
    g = torch.exp(-0.5 * (x / sigma) ** 2)
    return g / g.sum()


def gauss2d(sig_lat, n_lat, sig_lon, n_lon, dtype, device="cpu"):
    return (gauss1d(sig_lat, n_lat, dtype, device)[:, None] * gauss1d(sig_lon, n_lon, dtype, device)[None, :])[None, None]


def conv_zero_pad(x, k):
    return F.conv2d(x, k, padding=(k.shape[-2] // 2, k.shape[-1] // 2))


def blend_mask(u, v, args):
    """u, v [B, H, W] at the mask level -> m [B, 1, H, W]."""
    dtype = u.dtype
    flag = (torch.sqrt(u * u + v * v) > args["speed_threshold"]).to(dtype)[:, None]
    kh, kw = args["dilation_meridional"], args["dilation_zonal"]
    dilated = F.max_pool2d(flag, kernel_size=(kh, kw), stride=1, padding=(kh // 2, kw // 2))     # pads with -inf: never the maximum
    s = args["falloff_sigma"]
    return conv_zero_pad(dilated, gauss2d(s, int(4 * s + 1) | 1, 2 * s, int(8 * s + 1) | 1, dtype, u.device))


def smoothing_kernel(args, dtype, device="cpu"):
    sig_lat = args["smooth_sigma"] if args.get("smooth_sigma_meridional") is None else args["smooth_sigma_meridional"]
    sig_lon = args["smooth_sigma"] if args.get("smooth_sigma_zonal") is None else args["smooth_sigma_zonal"]
    return gauss2d(sig_lat, int(6 * sig_lat + 1) | 1, sig_lon, int(6 * sig_lon + 1) | 1, dtype, device)


def blend(f, g2d, m, preserve_amplitude):
    """f [B, 1, H, W] -> the blended plane."""
    fs = conv_zero_pad(f, g2d)
    if preserve_amplitude:
        num = (m * f * f).sum(dim=(1, 2, 3), keepdim=True)
        den = (m * fs * fs).sum(dim=(1, 2, 3), keepdim=True)
        fs = fs * torch.clamp(torch.sqrt(num / (den + 1e-12)), max=4.0)
    return m * fs + (1 - m) * f


def wind_filter(fields, u_key, v_key, targets, args, dtype=None):
    """fields {key: [B, L, 1, H, W]} -> ({target key: filtered [B, L, 1, H, W]}, m [B, 1, H, W]).  The mask comes from the INPUT U, V."""
    cast = (lambda t: t) if dtype is None else (lambda t: t.to(dtype))
    u, v = cast(fields[u_key]), cast(fields[v_key])
    m = blend_mask(u[:, args["mask_level"], 0], v[:, args["mask_level"], 0], args)
    g2d = smoothing_kernel(args, u.dtype, u.device)
    out = {}
    for key in targets:
        t = cast(fields[key])
        planes = [blend(t[:, l], g2d, m, args["preserve_amplitude"]) if l in set(args["target_levels"]) else t[:, l] for l in range(t.shape[1])]
        out[key] = torch.stack(planes, dim=1)
    return out, m
