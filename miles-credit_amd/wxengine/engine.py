"""ctypes binding of libwxengine.so (C ABI in include/wxengine.h).

PyTorch is used only as the owner of device memory and streams: tensors are handed to
the engine as raw device pointers.  There is NO CPU fallback: if the HIP library is
missing or no GPU is visible, construction raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np

from .config import WXConfig
from .native import (LIB_PATH, NativeHandle, WXEngineError, _check, _check_not_stale, _f32, _gpu_tensor, _i32,  # noqa: F401
                     _named_tensor_args, _stream_ptr, exported_symbols, load_library, require_gpu, wx_band_msg, wx_config,
                     wx_kernel_stat)

WX_ABI_VERSION = 3
ARCH = {"crossformer": 0, "wxformer": 1, "crossformer_upconv": 2, "camulator": 3}
PREC = {"fp32": 0, "bf16": 1, "fp32s": 2}   # fp32s: fp32 storage, split-bf16 GEMM arithmetic (WX_PREC_FP32_SPLIT)


def make_c_config(cfg: WXConfig, precision: str = "bf16", max_batch: int = 1) -> wx_config:
    c = wx_config()
    c.abi_version = WX_ABI_VERSION
    for f in ("image_height", "image_width", "frames", "output_frames", "channels", "surface_channels",
              "input_only_channels", "output_only_channels", "levels", "dim_head"):
        setattr(c, f, int(getattr(cfg, f)))
    for i in range(4):
        c.dim[i] = cfg.dim[i]
        c.depth[i] = cfg.depth[i]
        c.global_window_size[i] = cfg.global_window_size[i]
        c.local_window_size[i] = cfg.local_window_size[i]
        ks = cfg.cross_embed_kernel_sizes[i]
        c.n_embed_kernels[i] = len(ks)
        for j, k in enumerate(ks):
            c.embed_kernels[i][j] = k
        c.embed_strides[i] = cfg.cross_embed_strides[i]
    c.pad_activate = (2 if getattr(cfg, "pad_mode", "earth") == "mirror" else 1) if cfg.pad_activate else 0
    c.pad_lat[0], c.pad_lat[1] = cfg.pad_lat
    c.pad_lon[0], c.pad_lon[1] = cfg.pad_lon
    c.interp = int(cfg.interp)
    c.use_spectral_norm = int(cfg.use_spectral_norm)
    c.precision = PREC[precision]
    c.max_batch = max_batch
    arch = getattr(cfg, "arch", "crossformer")
    if arch == "crossformer" and getattr(cfg, "upsample_v_conv", False):
        arch = "crossformer_upconv"
    c.arch = ARCH[arch]
    c.noise_latent_dim = int(getattr(cfg, "noise_latent_dim", 0))
    c.encoder_noise = int(bool(getattr(cfg, "encoder_noise", True)))
    c.noise_correlated = int(bool(getattr(cfg, "correlated", False)))
    return c


class WXEngine:
    """Owns one wx_handle.  Inputs/outputs are torch CUDA (HIP) tensors, float32, contiguous."""

    def __init__(self, cfg: WXConfig, precision: str = "bf16", device: int = 0):
        self.lib = require_gpu("the wxengine HIP path cannot run and there is no CPU fallback")
        self.cfg = cfg
        self.precision = precision
        self.device = device
        self._h = NativeHandle(self.lib.wx_destroy)
        cc = make_c_config(cfg, precision)
        _check(self.lib.wx_create(C.byref(cc), device, self._h.out))
        self._finalized = False

    # ---- weights -----------------------------------------------------------------
    def expected_tensors(self) -> Dict[str, Tuple[int, ...]]:
        out = {}
        key = C.c_char_p()
        nd = C.c_int()
        shape = (C.c_int64 * 8)()
        for i in range(self.lib.wx_num_tensors(self._h)):
            _check(self.lib.wx_tensor_info(self._h, i, C.byref(key), C.byref(nd), shape))
            out[key.value.decode()] = tuple(shape[d] for d in range(nd.value))
        return out

    def load_state_dict(self, sd) -> None:
        """sd: mapping key -> numpy array / torch tensor (reference state-dict layout)."""
        for k, v in sd.items():
            if hasattr(v, "detach"):
                v = v.detach().to("cpu").float().numpy()
            a = np.ascontiguousarray(v, dtype=np.float32)
            shp = (C.c_int64 * max(a.ndim, 1))(*a.shape) if a.ndim else (C.c_int64 * 1)(1)
            _check(self.lib.wx_load_tensor(self._h, k.encode(), _f32(a), max(a.ndim, 1), shp))
        self._finalized = False

    def finalize(self) -> None:
        _check(self.lib.wx_finalize_weights(self._h))
        self._finalized = True

    # ---- glue configuration --------------------------------------------------------
    def set_denorm(self, mean, std) -> None:
        m, s = _fp(mean).ravel(), _fp(std).ravel()
        _check(self.lib.wx_set_denorm(self._h, _f32(m), _f32(s), m.size))

    def set_tracer_fixer(self, inds, thres, thres_max=None, denorm: bool = False) -> None:
        _check(self.lib.wx_set_tracer_fixer(self._h, _i32(inds), _f32(thres), _f32(thres_max), np.size(inds), int(denorm)))

    def set_layout(self, n_prog: int, n_static: int, n_dyn: int) -> None:
        _check(self.lib.wx_set_layout(self._h, n_prog, n_static, n_dyn))
        self._n_dyn = int(n_dyn)

    def set_layout_groups(self, groups) -> None:
        """groups: iterable of (kind, x_start, src_start, count) with kind in {"prognostic", "dynamic_forcing", "static"} (or
        0 / 1 / 2), i.e. the ChannelGroup list of credit/datasets/gen_2/channel_utils.py:140-250 for any number of sources
        (wxengine.rollout.build_channel_layout produces it from a CREDIT config)."""
        code = {"prognostic": 0, "dynamic_forcing": 1, "static": 2}
        rows = [(code.get(k, k), int(x0), int(0 if s0 is None else s0), int(n)) for k, x0, s0, n in groups]
        _check(self.lib.wx_set_layout_groups(self._h, len(rows), *[_i32([r[i] for r in rows]) for i in range(4)]))
        # the C side sizes the forcing tensor as max(src_start + count) over the forcing groups (wx_engine.hip, set_layout_groups)
        self._n_dyn = max([r[2] + r[3] for r in rows if r[0] == 1], default=0)

    # ---- hot path -------------------------------------------------------------------
    @staticmethod
    def _stream():
        return _stream_ptr()

    @staticmethod
    def _chk_in(t, name):
        if not _gpu_tensor(t, contiguous=True):
            raise WXEngineError(f"{name} must be a contiguous float32 tensor on the GPU")

    def forward(self, x, out=None):
        import torch
        self._chk_in(x, "x")
        cfg = self.cfg
        if x.dim() == 4:
            x = x.unsqueeze(2)
        b = x.shape[0]
        if tuple(x.shape[1:]) != (cfg.base_input_channels, cfg.frames, cfg.image_height, cfg.image_width):
            raise WXEngineError(f"x has shape {tuple(x.shape)}, expected [B, {cfg.base_input_channels}, {cfg.frames}, "
                                f"{cfg.image_height}, {cfg.image_width}]")
        oh, ow = cfg.out_hw
        if out is None:
            out = torch.empty((b, cfg.base_output_channels, cfg.output_frames, oh, ow), dtype=torch.float32, device=x.device)
        _check(self.lib.wx_forward(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), b, self._stream()))
        return out

    def _chk_shape(self, t, name, tail):
        """`t` must hold exactly the trailing dims `tail` after dropping singleton dims (B = 1, T = 1): raw pointers go to the
        library next, so a short forcing tensor or a wrong grid would read / write out of bounds there."""
        if t is None:
            return
        self._chk_in(t, name)
        got = [d for d in t.shape if d != 1]
        want = [d for d in tail if d != 1]
        if got != want:
            raise WXEngineError(f"{name} has shape {tuple(t.shape)}, expected [1, {', '.join(str(d) for d in tail)}] (singleton dims optional)")

    def _chk_step_io(self, x, frc, y, yp, xn):
        cfg = self.cfg
        oh, ow = cfg.out_hw
        self._chk_shape(x, "x", (cfg.base_input_channels, cfg.image_height, cfg.image_width))
        self._chk_shape(y, "y_out", (cfg.base_output_channels, oh, ow))
        self._chk_shape(yp, "phys_out", (cfg.base_output_channels, oh, ow))
        self._chk_shape(xn, "next_out", (cfg.base_input_channels, cfg.image_height, cfg.image_width))
        if frc is not None:
            n_dyn = getattr(self, "_n_dyn", None)
            if n_dyn is None:
                raise WXEngineError("frc given but no channel layout is set (set_layout / set_layout_groups)")
            self._chk_shape(frc, "frc", (n_dyn, cfg.image_height, cfg.image_width))

    def step(self, x, frc=None, want_y=True, want_phys=True, want_next=True, y_out=None, phys_out=None, next_out=None):
        """One rollout iteration. Returns (y, y_phys, x_next); entries are None when not requested.
        Pre-allocated outputs may be passed (y_out / phys_out / next_out) to keep the loop allocation-free."""
        import torch
        self._chk_in(x, "x")
        cfg = self.cfg
        oh, ow = cfg.out_hw
        y = y_out if y_out is not None else (
            torch.empty((1, cfg.base_output_channels, 1, oh, ow), dtype=torch.float32, device=x.device) if want_y else None)
        yp = phys_out if phys_out is not None else (
            torch.empty((1, cfg.base_output_channels, oh, ow), dtype=torch.float32, device=x.device) if want_phys else None)
        xn = next_out if next_out is not None else (torch.empty_like(x) if want_next else None)
        self._chk_step_io(x, frc, y, yp, xn)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        _check(self.lib.wx_step(self._h, p(x), p(frc), p(y), p(yp), p(xn), self._stream()))
        return y, yp, xn

    def rollout(self, x0, forcings, phys_out=None, x_final=None):
        """wx_rollout: len(forcings) forecast steps inside the library (the predict() loop of rollout_to_netcdf.py:262-316).
        forcings[t] enters the input of step t+1 (None entries allowed where no next input is built); phys_out: list of
        len(forcings) tensors / Nones receiving each step's de-normalised output (entries may repeat: a ring); x_final: optional
        tensor receiving the input of the step after the last one.  Bit-identical to calling `step` in a loop."""
        n = len(forcings)
        if n < 1:
            raise WXEngineError("rollout needs at least one step")
        if phys_out is None:
            phys_out = [None] * n
        if len(phys_out) != n:
            raise WXEngineError("phys_out must have one entry per step")
        for t in range(n):
            self._chk_step_io(x0, forcings[t], None, phys_out[t], x_final if t == n - 1 else None)
        vp = C.c_void_p * n
        fa = vp(*[None if f is None else f.data_ptr() for f in forcings])
        ya = vp(*[None if y is None else y.data_ptr() for y in phys_out])
        _check(self.lib.wx_rollout(self._h, C.c_void_p(x0.data_ptr()), fa, n, ya,
                                   None if x_final is None else C.c_void_p(x_final.data_ptr()), self._stream()))
        return phys_out, x_final

    # ---- ensemble noise (CrossFormerWithNoise) ----------------------------------------------
    def set_noise(self, seed: int = 0, member0: int = 0, step: int = 0) -> None:
        """Generator coordinates: batch row b of the next forward is member member0 + b; `step` is the step coordinate of the
        next forward / step, advanced by one on the device after each (include/wxengine.h wx_set_noise)."""
        _check(self.lib.wx_set_noise(self._h, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(member0), int(step)))

    def set_noise_tape(self, draws=None) -> None:
        """Replay `draws` (float32 CUDA tensors in the reference's torch.randn order, each covering the whole batch) instead of
        the generator; None returns to the generator."""
        if draws is None:
            _check(self.lib.wx_set_noise_tape(self._h, None, 0))
            self._tape = None
            return
        draws = list(draws)
        for i, t in enumerate(draws):
            self._chk_in(t, f"draws[{i}]")
        arr = (C.c_void_p * len(draws))(*[t.data_ptr() for t in draws])
        _check(self.lib.wx_set_noise_tape(self._h, arr, len(draws)))
        self._tape = draws   # the engine keeps the raw pointers: keep the tensors alive

    # ---- introspection -----------------------------------------------------------------
    def set_debug(self, level) -> None:
        """Capture level of wx_set_debug: 0 / False off, 1 / True every named activation (fused routes step aside), 2 what the
        default routes leave in memory, with no change to which kernels run."""
        _check(self.lib.wx_set_debug(self._h, int(level)))

    def debug_read(self, name: str) -> np.ndarray:
        shape = (C.c_int64 * 3)()
        _check(self.lib.wx_debug_read(self._h, name.encode(), None, 0, shape))
        out = np.empty((shape[0], shape[1], shape[2]), dtype=np.float32)
        _check(self.lib.wx_debug_read(self._h, name.encode(), _f32(out), out.size, shape))
        return out

    def query(self, key: str) -> int:
        """One integer fact about the engine / its last forward (include/wxengine.h wx_query)."""
        v = C.c_int64(0)
        _check(self.lib.wx_query(self._h, key.encode(), C.byref(v)))
        return int(v.value)

    def info(self) -> dict:
        return {k: self.query(k) for k in ("launches", "precision", "split_gemms")}

    def profile(self, on) -> None:
        """0 off, 1 per kernel class, 2 per kernel class and stage ("gemm_ff1.s2")."""
        _check(self.lib.wx_profile(self._h, int(on)))

    def attach_postblock(self, post) -> None:
        """Run `post` (a WXPostBlock, or None to detach) after every forward, before y_phys / x_next are formed."""
        self._post = post  # keep it alive
        _check(self.lib.wx_attach_postblock(self._h, post._p if post is not None else None))

    def profile_reset(self) -> None:
        _check(self.lib.wx_profile_reset(self._h))

    def profile_read(self):
        arr = (wx_kernel_stat * 256)()
        n = C.c_int()
        _check(self.lib.wx_profile_read(self._h, arr, 256, C.byref(n)))
        return [dict(name=arr[i].name.decode(), launches=arr[i].launches, ms=arr[i].ms, flops=arr[i].flops,
                     bytes=arr[i].bytes) for i in range(n.value)]


def _fp(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class WXPostBlock:
    """Device-side PostBlock (credit/postblock/gen1.py) for pressure-level grids: ordered fixers applied in place."""

    def __init__(self, H: int, W: int, c_in: int, frames: int, c_out: int, device: int = 0):
        self.lib = require_gpu("the post block has no CPU fallback")
        self.shape = (H, W, c_in, frames, c_out)
        self._p = NativeHandle(self.lib.wx_post_destroy)
        _check(self.lib.wx_post_create(H, W, c_in, frames, c_out, device, self._p.out))

    def set_band(self, row0: int, rows: int):
        """Lat-band mode: this block sees rows [row0, row0+rows) only (call before set_grid*; the grid arrays stay whole-grid)."""
        _check(self.lib.wx_post_set_band(self._p, int(row0), int(rows)))

    def set_grid(self, lat2d, lon2d, p_levels, midpoint: bool = False):
        pl = _fp(p_levels)
        _check(self.lib.wx_post_set_grid(self._p, _f32(lat2d), _f32(lon2d), _f32(pl), pl.size, int(midpoint)))

    def set_grid_sigma(self, lat2d, lon2d, coef_a, coef_b, sp_ind: int, midpoint: bool = False):
        """Hybrid sigma-pressure levels p = a + b * surface pressure (credit/physics_core.py:300-368); `sp_ind` is the
        surface-pressure channel (same index in x and y, credit/postblock/gen1.py:306-308)."""
        ca, cb = _fp(coef_a), _fp(coef_b)
        if ca.size != cb.size:
            raise ValueError("coef_a and coef_b must have the same length")
        _check(self.lib.wx_post_set_grid_sigma(self._p, _f32(lat2d), _f32(lon2d), _f32(ca), _f32(cb), ca.size, int(midpoint), int(sp_ind)))

    def set_stats(self, mean_in, std_in, mean_out, std_out):
        _check(self.lib.wx_post_set_stats(self._p, *[_f32(_fp(v).ravel()) for v in (mean_in, std_in, mean_out, std_out)]))

    def add_tracer_fixer(self, inds, thres, thres_max=None, denorm=False):
        _check(self.lib.wx_post_add_tracer_fixer(self._p, _i32(inds), _f32(thres), _f32(thres_max), np.size(inds), int(denorm)))

    def add_mass_fixer(self, q_start, fix_level_num, denorm=False):
        _check(self.lib.wx_post_add_mass_fixer(self._p, q_start, fix_level_num, int(denorm)))

    def add_water_fixer(self, q_start, precip_ind, evapor_ind, n_seconds, denorm=False):
        _check(self.lib.wx_post_add_water_fixer(self._p, q_start, precip_ind, evapor_ind, float(n_seconds), int(denorm)))

    def add_energy_fixer(self, T_start, q_start, U_start, V_start, rad_inds, gph_surf, n_seconds, denorm=False):
        assert np.size(rad_inds) == 6
        _check(self.lib.wx_post_add_energy_fixer(self._p, T_start, q_start, U_start, V_start, _i32(rad_inds), _f32(gph_surf),
                                                 float(n_seconds), int(denorm)))

    def add_energy_fixer_signed(self, T_start, q_start, U_start, V_start, toa, surf, gph_surf, n_seconds, denorm=False):
        """toa / surf: lists of (channel, sign): R_T = sum sign * y[channel] (<= 4 terms), F_S likewise (<= 8)."""
        _check(self.lib.wx_post_add_energy_fixer_signed(self._p, T_start, q_start, U_start, V_start, len(toa), _i32([c for c, _ in toa]),
                                                        _f32([s for _, s in toa]), len(surf), _i32([c for c, _ in surf]),
                                                        _f32([s for _, s in surf]), _f32(gph_surf), float(n_seconds), int(denorm)))

    def add_energy_fixer_updown(self, T_start, q_start, U_start, V_start, flux_inds, gph_surf, n_seconds, denorm=False):
        """GlobalEnergyFixerUpDown (credit/postblock/gen1.py:825-1030); flux_inds = [TOA down solar, TOA up solar, TOA up OLR,
        surf down solar, surf up solar, surf down LW, surf up LW, SH, LH]."""
        assert np.size(flux_inds) == 9
        _check(self.lib.wx_post_add_energy_fixer_updown(self._p, T_start, q_start, U_start, V_start, _i32(flux_inds), _f32(gph_surf),
                                                        float(n_seconds), int(denorm)))

    def apply(self, x, y):
        """x [C_in, frames, H, W], y [C_out, H, W] float32 CUDA tensors (leading batch dim of 1 allowed); y is fixed in place."""
        WXEngine._chk_in(x, "x")
        WXEngine._chk_in(y, "y")
        H, W, c_in, fr, c_out = self.shape
        if x.numel() != c_in * fr * H * W or y.numel() != c_out * H * W:
            raise WXEngineError("post block: tensor sizes do not match the geometry")
        _check(self.lib.wx_post_apply(self._p, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), _stream_ptr()))
        return y


class WXDiag:
    """Device-side pressure-level products (include/wxengine.h wx_diag_*, csrc/wx_diag.h): model-level geopotential, model ->
    pressure levels and MSLP of one set of named tensors in one launch.  The blocks of wxengine/diagnostics.py sit on top."""

    def __init__(self, H: int, W: int, n_levels: int, device: int = 0):
        self.lib = require_gpu("the pressure-level products have no CPU fallback")
        self.H, self.W, self.L, self.device = int(H), int(W), int(n_levels), int(device)
        self._d = NativeHandle(self.lib.wx_diag_destroy)
        _check(self.lib.wx_diag_create(self.H, self.W, self.L, self.device, self._d.out))

    def set_levels(self, a_half=None, b_half=None, a_mid=None, b_mid=None, flip_vertical: bool = True):
        """Hybrid coefficients in the stored level order: a_half / b_half [n_levels + 1] for the geopotential, a_mid / b_mid
        [n_levels] for the interpolation; either pair may be None."""
        arrs = []
        for name, a, n in (("a_half", a_half, self.L + 1), ("b_half", b_half, self.L + 1), ("a_mid", a_mid, self.L), ("b_mid", b_mid, self.L)):
            if a is None:
                arrs.append(None)
                continue
            a = _fp(a).ravel()
            if a.size != n:
                raise WXEngineError(f"n_levels mismatch: {name} has {a.size} entries, the block was created for {self.L} levels ({n} expected)")
            arrs.append(a)
        _check(self.lib.wx_diag_set_levels(self._d, *[_f32(a) for a in arrs], int(bool(flip_vertical))))

    def set_pressure_levels(self, p_pa, temp_height: float = 150.0):
        p = _fp(p_pa).ravel()
        _check(self.lib.wx_diag_set_pressure_levels(self._d, _f32(p), p.size, float(temp_height)))
        self.n_plev = p.size

    def apply(self, sp, phis, T=None, q=None, t_ns=None, fields=(), z_in=None, want_z=False, want_plev=False, want_mslp=False):
        """Named tensors [B, n_levels, n_time, H, W] (sp / t_ns: one level; phis: one level, n_time 1 or that of sp) -> dict with
        "z" [B, n_levels, n_time, H, W], "plev" (list: every field, then T, then Z, each [B, n_plev, n_time, H, W]) and "mslp"
        [B, 1, n_time, H, W] for the products asked for.  `z_in`: chain form, the interpolation reads this geopotential instead of
        integrating T and q.  The tensors are read where they lie: views into a larger tensor are taken as they are, and when the
        batch items of such a view are not adjacent in memory every item is one launch.  Nothing is copied."""
        import torch
        fields = list(fields)
        named = [("sp", sp, 1), ("phis", phis, 1), ("T", T, self.L), ("q", q, self.L), ("t_ns", t_ns, 1), ("z_in", z_in, self.L)]
        named += [(f"fields[{i}]", f, self.L) for i, f in enumerate(fields)]
        if sp is None or sp.dim() != 5:
            raise WXEngineError("sp must be a [B, 1, n_time, H, W] tensor")
        B, _, nT = sp.shape[:3]
        for name, t, nl in named:
            if t is None:
                continue
            if not _gpu_tensor(t, ndim=5):
                raise WXEngineError(f"{name} must be a float32 [B, n_levels, n_time, H, W] tensor on the GPU")
            if not _gpu_tensor(t, device=self.device):
                raise WXEngineError(f"{name} is on cuda:{t.device.index} but this block was created for cuda:{self.device}")
            if nl == self.L and t.shape[1] != self.L:
                raise WXEngineError(f"n_levels mismatch: {name} has {t.shape[1]} levels, the block was created for {self.L}")
            want = (B, nl, nT, self.H, self.W)
            if name == "phis":
                if t.shape[0] not in (1, B) or t.shape[2] not in (1, nT) or (t.shape[1], t.shape[3], t.shape[4]) != (1, self.H, self.W):
                    raise WXEngineError(f"phis has shape {tuple(t.shape)}, expected [{B} or 1, 1, {nT} or 1, {self.H}, {self.W}]")
            elif tuple(t.shape) != want:
                raise WXEngineError(f"{name} has shape {tuple(t.shape)}, expected {list(want)}")
        kw = dict(dtype=torch.float32, device=sp.device)
        out = {}
        if want_z:
            out["z"] = torch.empty((B, self.L, nT, self.H, self.W), **kw)
        if want_plev:
            out["plev"] = [torch.empty((B, getattr(self, "n_plev", 0) or 1, nT, self.H, self.W), **kw) for _ in range(len(fields) + 2)]
        if want_mslp:
            out["mslp"] = torch.empty((B, 1, nT, self.H, self.W), **kw)
        ins = [t for _, t, _ in named if t is not None]
        whole = all(t.is_contiguous() for t in ins) and phis.shape[0] == B
        stream = _stream_ptr(self.device)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
        for b in ([None] if whole else range(B)):
            def item(t, shared=False):
                if t is None or b is None:
                    return t
                t = t[0:1] if (shared and t.shape[0] == 1) else t[b:b + 1]
                if not t.is_contiguous():
                    raise WXEngineError("a batch item of every input must be contiguous [n_levels, n_time, H, W] memory")
                return t
            z_arg = item(out["z"]) if want_z else (item(z_in) if want_plev else None)
            f_arr = (C.c_void_p * max(len(fields), 1))(*[item(f).data_ptr() for f in fields])
            p_arr = (C.c_void_p * (len(fields) + 2))(*[item(t).data_ptr() for t in out["plev"]]) if want_plev else None
            q_arg = None if (z_in is not None and not want_z) else q
            with torch.cuda.device(self.device):
                _check(self.lib.wx_diag_apply(self._d, B if b is None else 1, nT, ptr(item(T)), ptr(item(q_arg)), ptr(item(sp)),
                                              ptr(item(phis, shared=True)), int(phis.shape[2]), ptr(item(t_ns)), f_arr, len(fields),
                                              ptr(z_arg), p_arr, ptr(item(out["mslp"])) if want_mslp else None, stream))
        return out
