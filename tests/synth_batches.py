"""Synthetic named-tensor batches shared by tools/make_goldens.py (golden generation) and the tests (pure numpy / torch:
importable on the GPU box, where the reference is absent)."""
import numpy as np
import torch


def preblock_batch(seed=21):
    """A synthetic gen-2 style batch: deliberately NOT in canonical order, with per-level, scalar and missing statistics."""
    g = np.random.Generator(np.random.Philox(key=[seed, 1]))
    B, T, H, W = 2, 1, 9, 14
    def f(nl):
        return torch.from_numpy(g.standard_normal((B, nl, T, H, W)).astype(np.float32) * 7.0 + 3.0)
    variables = {"era5/dynamic_forcing/2d/tsi": f(1), "era5/prognostic/2d/SP": f(1), "era5/static/2d/LSM": f(1),
                 "era5/prognostic/3d/T": f(4), "era5/prognostic/3d/Q": f(4), "era5/prognostic/2d/t2m": f(1),
                 "era5/static/2d/Z_GDS4_SFC": f(1), "era5/prognostic/3d/U": f(4)}
    mean = {"T": np.array([210., 230., 260., 280.], np.float32), "Q": np.array([1e-6, 1e-4, 2e-3, 8e-3], np.float32),
            "U": np.array([5., 3., 1., 0.], np.float32), "SP": np.float32(9.8e4), "t2m": np.float32(285.), "tsi": np.float32(1.2e6)}
    std = {"T": np.array([8., 9., 12., 15.], np.float32), "Q": np.array([1e-6, 2e-4, 0.0, 5e-3], np.float32),   # a zero std: clamp path
           "U": np.array([20., 15., 10., 6.], np.float32), "SP": np.float32(9.0e3), "t2m": np.float32(15.), "tsi": np.float32(9.0e5)}
    return {"input": {"era5": variables}}, mean, std


def conservation_batch(seed=31, midpoint=True):
    """A gen-2 style `batch_dict` on the reference's 10 x 18 demo grid with 7 hybrid levels (6 mid-level values when
    `midpoint`): y_processed (t1) and x_physical (t0, two frames), physical units, B = 2."""
    g = np.random.Generator(np.random.Philox(key=[seed, 2]))
    B, H, W, L = 2, 10, 18, 6 if midpoint else 7

    def t(a):
        return torch.from_numpy(np.asarray(a, np.float32))

    def state(T):
        return {"cam/prognostic/3d/T": t(250.0 + 30.0 * g.standard_normal((B, L, T, H, W))),
                "cam/prognostic/3d/Qtot": t(np.abs(0.004 + 0.004 * g.standard_normal((B, L, T, H, W)))),
                "cam/prognostic/3d/U": t(12.0 * g.standard_normal((B, L, T, H, W))),
                "cam/prognostic/3d/V": t(8.0 * g.standard_normal((B, L, T, H, W))),
                "cam/prognostic/2d/PS": t(1.0e5 + 2.0e3 * g.standard_normal((B, 1, T, H, W)))}
    y = state(1)
    for k in ("FSUTOA", "FLUT", "FSDS", "FSUS", "FLDS", "FLUS", "SHFLX", "LHFLX"):
        scale = 200.0 if k in ("FSUTOA", "FLUT") else 3.0e6        # TOA terms in W/m2, surface terms in J/m2 (conservation.py)
        y[f"cam/diagnostic/2d/{k}"] = t(np.abs(scale * g.standard_normal((B, 1, 1, H, W))))
    y["cam/diagnostic/2d/PRECT"] = t(np.abs(2e-3 * g.standard_normal((B, 1, 1, H, W))))
    y["cam/diagnostic/2d/QFLX"] = t(-np.abs(1e-3 * g.standard_normal((B, 1, 1, H, W))))
    x = state(2)
    x["cam/dynamic_forcing/2d/SOLIN"] = t(np.abs(300.0 * g.standard_normal((B, 1, 2, H, W))))
    gph = (50.0 + 20.0 * g.standard_normal((H, W))).astype(np.float32)
    return {"y_processed": {"cam": y}, "x_physical": {"cam": x}}, gph


def odd_config(h3, w3, lw, gw, pad=None, depth=(1, 1, 1, 1), arch="crossformer"):
    """Small CrossFormer geometries outside the BASELINE family (stage-3 map h3 x w3, local window lw, long windows gw, optional
    asymmetric earth padding ((top, bottom), (left, right))): used to sweep the lat-band plan and the engine over window / rank
    combinations the named configs do not hit."""
    from wxengine.config import WXConfig
    mc = dict(frames=1, channels=2, surface_channels=2, input_only_channels=2, output_only_channels=1, levels=2,
              image_height=16 * h3 - (sum(pad[0]) if pad else 0), image_width=16 * w3 - (sum(pad[1]) if pad else 0),
              patch_width=1, patch_height=1, cross_embed_kernel_sizes=[[4, 8, 16, 32], [2, 4], [2, 4], [2, 4]],
              cross_embed_strides=[2, 2, 2, 2], dim=[32, 64, 128, 256], depth=list(depth), global_window_size=list(gw),
              local_window_size=lw, interp=True, use_spectral_norm=True,
              padding_conf=dict(activate=bool(pad), mode="earth", pad_lat=list(pad[0]) if pad else [0, 0],
                                pad_lon=list(pad[1]) if pad else [0, 0]))
    return WXConfig.from_model_conf(mc, arch=arch)


ODD_CONFIGS = {
    "w2": dict(h3=2, w3=4, lw=2, gw=(4, 4, 2, 2)),                         # a long window at the deepest stage too
    "w3": dict(h3=3, w3=3, lw=3, gw=(8, 4, 2, 1)),
    "w1": dict(h3=4, w3=4, lw=1, gw=(2, 2, 2, 2)),                         # 1-token local windows
    "w16": dict(h3=6, w3=6, lw=2, gw=(16, 8, 4, 2), depth=(1, 1, 2, 1)),   # 256-token long windows
    "w5p": dict(h3=5, w3=5, lw=5, gw=(8, 4, 2, 1), pad=((13, 11), (9, 7))),  # asymmetric pads, odd image
}


def two_source_conf():
    """A CREDIT config whose model input interleaves two data sources (channel_utils.py:161-250: a field type's channels are
    contiguous only within a source).  x: 14 channels, y: 11, forcing tensor: 3."""
    def grp(v3=(), v2=()):
        return {"vars_3D": list(v3), "vars_2D": list(v2)}
    return {"model": {"levels": 3},
            "data": {"history_len": 1, "source": {
                "era5": {"levels": [500, 700, 850], "variables": {
                    "prognostic": grp(("U", "T"), ("SP",)), "static": grp(v2=("LSM",)),
                    "dynamic_forcing": grp(v2=("tsi",)), "diagnostic": grp(v2=("precip",))}},
                "aux": {"levels": None, "variables": {
                    "prognostic": grp(v2=("sst", "ice")), "static": grp(v2=("depth",)),
                    "dynamic_forcing": grp(v2=("tide", "wind")), "diagnostic": grp(v2=("flux",))}}}}}


def gen2loop_schema(cfg):
    """Variable keys of a gen-2 forecast on a CrossFormer config: (input keys with level counts, output keys with level counts)."""
    L = cfg.levels
    inp = [(f"era5/prognostic/3d/{v}", L) for v in "UVTQ"[:cfg.channels]] + [(f"era5/prognostic/2d/s{i}", 1) for i in range(cfg.surface_channels)]
    inp += [("era5/static/2d/LSM", 1), ("era5/static/2d/Z", 1), ("era5/dynamic_forcing/2d/tsi", 1), ("era5/dynamic_forcing/2d/sza", 1)]
    out = inp[:cfg.channels + cfg.surface_channels] + [(f"era5/diagnostic/2d/d{i}", 1) for i in range(cfg.output_only_channels)]
    return inp, out


def gen2loop_batches(cfg, n_steps=3, seed=77):
    """Initial condition, n_steps - 1 forcing batches (physical units, [1, n_levels, 1, H, W]) and per-variable statistics for the
    composed gen-2 loop (tools/make_goldens.py --only gen2loop drives the reference's run_forecast with exactly these)."""
    inp, out = gen2loop_schema(cfg)
    gen = np.random.Generator(np.random.Philox(key=[seed, 1]))
    H, W = cfg.image_height, cfg.image_width

    def field(nl, scale=1.0, shift=0.0):
        return torch.from_numpy((gen.standard_normal((1, nl, 1, H, W)) * scale + shift).astype(np.float32))
    mean = {k.split("/")[-1]: (np.arange(nl, dtype=np.float32) * 0.1 + 0.3) for k, nl in inp[:-2]}
    std = {k.split("/")[-1]: (np.arange(nl, dtype=np.float32) * 0.2 + 1.5) for k, nl in inp[:-2]}
    mean.update({f"d{i}": np.float32(0.1 * i) for i in range(cfg.output_only_channels)})
    std.update({f"d{i}": np.float32(2.0 + i) for i in range(cfg.output_only_channels)})
    ic = {"input": {"era5": {k: field(nl, 1.5, 0.3) for k, nl in inp}}}
    frcs = [{"input": {"era5": {k: field(1) for k, _ in inp[-2:]}}} for _ in range(n_steps - 1)]
    return ic, frcs, mean, std


# ------------------------------------------------------------------ acceptance classes of wx_create
# One tiny config per class of model that ModelSpec::derive() (csrc/wx_spec.h) / WXConfig.validate() accept and that the named configs
# do not span (tests/test_accepted_configs_gpu.py runs each against the fp64 oracle; tests/test_oracle_vs_reference.py pins the oracle
# itself to the reference at the same shapes).  Strides [2, 2, 2, 2]: the stage maps are (8, 4, 2, 1) x (h3, w3).
#   W  window sides 6, 7, 9, 11 - 15 at dim_head 32: a swept side w sits on maps of >= 2 windows per axis, as the local AND the global
#      window of stages 0 - 2 (widths 32 / 64 / 128); the 256-wide stage 3 takes w again where the map allows (6, 7), else a small one
#   H  dim_head 64 / 128 (the general-head-width kernel) at 36 / 49, 81 and 121 tokens
#   E  CrossEmbed kernel sets    F  interp / use_spectral_norm off, also with the PixelShuffle and upsample_v_conv decoders
# `nkf`: the key-fragment counts (16 tokens each, attn_nkf_tokens in csrc/wx_attn.h) the class claims to run; `embed`: the launches per
# forward that csrc/wx_weights.h:run() / Engine::cross_embed must choose, as {profile(2) kernel class: launches}.
_SMALL = dict(frames=1, channels=2, surface_channels=2, input_only_channels=2, output_only_channels=1, levels=2, patch_width=1,
              patch_height=1, cross_embed_kernel_sizes=[[4, 8, 16, 32], [2, 4], [2, 4], [2, 4]], cross_embed_strides=[2, 2, 2, 2],
              dim=[32, 64, 128, 256], depth=[1, 1, 1, 1], interp=True, use_spectral_norm=True)
_T0_PAD = dict(image_height=37, image_width=72, padding_conf=dict(activate=True, mode="earth", pad_lat=[6, 6], pad_lon=[12, 12]),
               global_window_size=[4, 2, 2, 1], local_window_size=3)     # padded 49 x 96 -> 24 x 48 ... 3 x 6; decoder output 36 x 72


def _sq(h3, lw, gw, **kw):
    return dict(_SMALL, image_height=16 * h3, image_width=16 * h3, local_window_size=list(lw), global_window_size=list(gw), **kw)


ACCEPTED_CONFIGS = {
    # ---- W (stage maps 8 h3, 4 h3, 2 h3, h3)
    "W6_12": dict(cls="W", swept=(6, 12), nkf={4, 10}, mc=_sq(12, (12, 6, 12, 6), (6, 12, 6, 6))),     # 36 of 64 tokens; 144 of 160
    "W7_14": dict(cls="W", swept=(7, 14), nkf={4, 14}, mc=_sq(14, (14, 7, 14, 7), (7, 14, 7, 7))),     # 49 of 64; 196 of 224
    "W9": dict(cls="W", swept=(9,), nkf={1, 7}, mc=_sq(9, (9, 9, 9, 3), (9, 9, 9, 3))),                # 81 of 112 (and 9 of 16 at stage 3)
    "W11": dict(cls="W", swept=(11,), nkf={8}, mc=_sq(11, (11, 11, 11, 1), (11, 11, 11, 1))),          # 121 of 128
    "W13": dict(cls="W", swept=(13,), nkf={12}, mc=_sq(13, (13, 13, 13, 1), (13, 13, 13, 1))),         # 169 of 192
    "W15": dict(cls="W", swept=(15,), nkf={2, 16}, mc=_sq(15, (15, 15, 15, 5), (15, 15, 15, 5))),      # 225 of 256 (and 25 of 32 at stage 3)
    # ---- H
    "H64w6": dict(cls="H", swept=(6,), nkf={4}, mc=_sq(6, (6, 6, 6, 3), (6, 6, 6, 3), dim=[64, 128, 256, 512], dim_head=64)),
    "H64w9": dict(cls="H", swept=(9,), nkf={7}, mc=_sq(9, (9, 9, 9, 3), (9, 9, 9, 3), dim=[64, 128, 256, 512], dim_head=64)),
    "H64w11": dict(cls="H", swept=(11,), nkf={8}, mc=_sq(11, (11, 11, 11, 1), (11, 11, 11, 1), dim=[64, 128, 256, 512], dim_head=64)),
    "H128w7": dict(cls="H", swept=(7,), nkf={4}, mc=_sq(7, (7, 7, 7, 1), (7, 7, 7, 1), dim=[128, 256, 512, 1024], dim_head=128)),
    # 128-wide heads in fp32 storage stop at 64 tokens (four 128 x (16 NKF + 4) fp32 V images pass 160 KB of LDS): bf16 only, and
    # REJECTED_CONFIGS holds the fp32 side
    "H128w9": dict(cls="H", precs=("bf16",), swept=(9,), nkf={7}, mc=_sq(9, (9, 9, 9, 3), (9, 9, 9, 3), dim=[128, 256, 512, 1024], dim_head=128)),
    "H128w11": dict(cls="H", precs=("bf16",), swept=(11,), nkf={8}, mc=_sq(11, (11, 11, 11, 1), (11, 11, 11, 1), dim=[128, 256, 512, 1024], dim_head=128)),
    # ---- E (4 x 4 stage-3 map; windows as ODD_CONFIGS["w2"])
    "E1": dict(cls="E", mc=_sq(4, (2, 2, 2, 2), (4, 4, 2, 2), cross_embed_kernel_sizes=[[4], [2], [2], [2]]),
               embed={"embed_patch": 0, "gemm_embed.s0": 1, "gemm_embed.s1": 1, "gemm_embed.s2": 1, "gemm_embed.s3": 1}),
    "E3": dict(cls="E", mc=_sq(4, (2, 2, 2, 2), (4, 4, 2, 2), cross_embed_kernel_sizes=[[4, 8, 16, 32], [2, 4, 8], [2, 4, 8], [2, 4, 8]]),
               embed={"embed_patch": 1, "gemm_embed.s0": 0, "gemm_embed.s1": 1, "gemm_embed.s2": 1, "gemm_embed.s3": 1}),   # merged as three
    "Eno4": dict(cls="E", mc=_sq(4, (2, 2, 2, 2), (4, 4, 2, 2), cross_embed_kernel_sizes=[[8, 16, 32], [2, 4], [2, 4], [2, 4]]),
                 embed={"embed_patch": 1, "gemm_embed.s0": 0, "gemm_embed.s1": 1}),
    "Eno32": dict(cls="E", mc=_sq(4, (2, 2, 2, 2), (4, 4, 2, 2), cross_embed_kernel_sizes=[[4, 16], [2, 4], [2, 4], [2, 4]]),
                  embed={"embed_patch": 0, "gemm_embed.s0": 2, "gemm_embed.s1": 1}),
    # stage-0 stride 4: 128 x 128 image -> 32 / 16 / 8 / 4 maps, decoder output 64 x 64, resized to the image by interp
    "Es4": dict(cls="E", mc=dict(_sq(8, (2, 2, 2, 2), (4, 4, 2, 2)), cross_embed_strides=[4, 2, 2, 2]),
                embed={"embed_patch": 0, "gemm_embed.s0": 4, "gemm_embed.s1": 1}),
    # ---- F
    "Fi_eq": dict(cls="F", mc=_sq(4, (2, 2, 2, 2), (4, 4, 2, 2), interp=False)),                       # decoder output == image
    "Fi_ne": dict(cls="F", mc=dict(_SMALL, **_T0_PAD, interp=False)),                                 # 36 x 72 out of a 37 x 72 image
    "Fsn": dict(cls="F", mc=dict(_SMALL, **_T0_PAD, use_spectral_norm=False)),
    "Fw": dict(cls="F", arch="wxformer", mc=dict(_SMALL, **_T0_PAD, interp=False, use_spectral_norm=False)),
    "Fu": dict(cls="F", mc=dict(_SMALL, **_T0_PAD, interp=False, use_spectral_norm=False, upsample_v_conv=True)),
}


def accepted_precisions(name):
    return ACCEPTED_CONFIGS[name].get("precs", ("fp32", "fp32s", "bf16"))


def accepted_config(name, precision=None):
    from wxengine.config import WXConfig
    e = ACCEPTED_CONFIGS[name]
    return WXConfig.from_model_conf(e["mc"], arch=e.get("arch", "crossformer"), precision=precision)


# what wx_create must refuse when the engine is created (tests/test_abi_cpu.py): (model conf, precision, words of the reason)
REJECTED_CONFIGS = {
    "dim96": (dict(_sq(4, (2, 2, 2, 2), (4, 4, 2, 2)), dim=[96, 192, 384, 768]), "bf16", "LayerNorm width unsupported"),
    "dim2048_fp32": (dict(_sq(4, (2, 2, 2, 2), (4, 4, 2, 2)), dim=[256, 512, 1024, 2048]), "fp32", "LayerNorm width unsupported"),
    "dim2048_fp32s": (dict(_sq(4, (2, 2, 2, 2), (4, 4, 2, 2)), dim=[256, 512, 1024, 2048]), "fp32s", "LayerNorm width unsupported"),
    # 72 of 288 / 4 fp32 pieces: one per lane would leave eight unread (the statistics were silently wrong before the check)
    "dim288_fp32": (dict(_sq(4, (2, 2, 2, 2), (4, 4, 2, 2)), dim=[288, 576, 1152, 2304]), "fp32", "LayerNorm width unsupported"),
    "dim_head96": (dict(_sq(4, (2, 2, 2, 2), (4, 4, 2, 2)), dim=[96, 192, 384, 768], dim_head=96), "bf16", "dim_head 96"),
    "dh128_w9_fp32": (ACCEPTED_CONFIGS["H128w9"]["mc"], "fp32", "exceeds the kernel's 160 KB of LDS"),
    "dh128_w11_fp32s": (ACCEPTED_CONFIGS["H128w11"]["mc"], "fp32s", "exceeds the kernel's 160 KB of LDS"),
    "c_out631": (dict(_sq(4, (2, 2, 2, 2), (4, 4, 2, 2)), levels=314), "bf16", "too many output channels for the tail kernel"),
}


# ------------------------------------------------------------------ the device PostBlock against the fp64 oracle
# tests/test_fixers_sweep_gpu.py runs every case on the GPU; tests/test_fixers_oracle.py runs the same table through the oracle in
# fp32 and fp64 (the conditioning test).  Grids: G9 = 33 x 67 (2 211 cells: 9 workgroups, 163 live lanes in the last), G257 =
# 181 x 363 (65 703 cells: 257 workgroups, so thread 0 of fix_sum_kernel takes a second trip; 167 live lanes in the last).
# Channel layout of a case with nl carried levels (levels - 1 when midpoint):
#   x [4 nl + 3]:  T | q | U | V | SP | 2 input-only          y [4 nl + 15]:  T | q | U | V | SP | 4 TOA | 8 surface | precip | evapor
FIXER_GRIDS = {"G9": (33, 67, 5.25), "G257": (181, 363, 0.75)}     # rows, columns, longitude step (degrees, exact in fp32)
FIXER_GATES = {"single": 5e-5, "chain": 1e-4, "chain_precip": 2e-3}  # max|got - ref| / max|ref| over the owned block (tests/test_fixers_gpu.py)
SIGNED_48 = dict(toa=(1.0, -1.0, 0.5, -1.0), surf=(1.0, -1.0, 1.0, -1.0, -1.0, -1.0, 2.5, -0.25))   # mixed signs, non-unit magnitudes
SIGNED_11 = dict(toa=(-0.75,), surf=(1.0,))
_FIX_BASE = dict(grid="G9", orient="ns", sigma=False, midpoint=False, denorm=False, frames=1, levels=13, fix=3)


def _fixer_cases():
    """name -> case.  Base: G9, north-to-south, pressure, trapz, denorm off, 1 frame, 13 levels, fix_level_num 3; one or two axes
    move per row.  fix_level_num = 1 stays out: the reference's own denominator is then an empty integral (gen1.py:264-270)."""
    rows = []

    def add(fixer, **kw):
        c = dict(_FIX_BASE, fixer=fixer, **kw)
        name = "-".join([c["grid"], "sig" if c["sigma"] else "prs", fixer] + [f"{k}{int(v) if not isinstance(v, str) else v}" for k, v in kw.items()
                                                                              if k not in ("grid", "sigma")])
        rows.append((name, c))

    for grid in ("G9", "G257"):
        big = grid == "G257"
        for sigma in (False, True):
            g = dict(grid=grid, sigma=sigma)
            for fixer in ("mass", "water", "energy", "signed48", "chain"):     # the fixers and the chain at the base case
                add(fixer, **g)
            add("mass", midpoint=True, **g)
            add("chain", midpoint=True, denorm=True, frames=2, **g)
            add("water", denorm=True, frames=3, **g)
            add("energy", denorm=True, midpoint=True, **g)
            add("signed48", denorm=True, frames=2, levels=2, **g)
            if not sigma:                                       # fix_level_num: the sigma mass fixer rescales SP and has none
                add("mass", fix=2, frames=2, **g)
                add("mass", fix=13, **g)
            if not big:                                         # 64 levels: G9 only
                add("mass", levels=64, fix=64, midpoint=True, **g)
                add("energy", levels=64, denorm=True, **g)
    add("updown")
    add("signed11")
    add("updown", denorm=True, midpoint=True)
    add("mass", levels=2, fix=2, denorm=True)
    add("mass", levels=64, fix=2)
    add("chain", orient="sn")                                   # south-to-north rows
    add("chain", orient="wrap", sigma=True, denorm=True)        # longitudes from 200 degrees through 360
    return dict(rows)


FIXER_CASES = _fixer_cases()


def fixer_case_inputs(name):
    """Everything a case needs, as fp32 numpy arrays (what the engine is handed; the fp64 oracle promotes the same numbers)."""
    c = FIXER_CASES[name]
    H, W, dlon = FIXER_GRIDS[c["grid"]]
    L = c["levels"]
    nl = L - 1 if c["midpoint"] else L
    g = np.random.Generator(np.random.Philox(key=[sorted(FIXER_CASES).index(name), 41]))
    # G9 runs pole to pole (cells of next to no area at both ends); G257 from the pole to the equator, so that its LAST workgroup
    # -- the 257th partial, which only the second trip of fix_sum_kernel's stride loop adds -- holds cells of the largest area
    lat = np.linspace(90.0, -90.0 if c["grid"] == "G9" else 0.0, H)
    if c["orient"] == "sn":
        lat = lat[::-1]
    lon = np.arange(W) * dlon
    if c["orient"] == "wrap":
        lon = (200.0 + lon) % 360.0           # the (-pi, pi] wrap of d_lambda sits inside every row
    lon2d, lat2d = np.meshgrid(lon.astype(np.float32), lat.astype(np.float32))
    eta = np.linspace(0.0, 1.0, L)
    p = np.round(2000.0 + 99000.0 * eta)                                 # Pa, integers: exact in fp32
    coef_a = np.round(2000.0 * (1.0 - eta) + 40000.0 * eta * (1.0 - eta))
    coef_b = (eta ** 2).astype(np.float32)

    def state(dT, fq, dsp):
        return [250.0 + dT + 30.0 * g.standard_normal((nl, H, W)), fq * np.abs(0.004 + 0.004 * g.standard_normal((nl, H, W))),
                12.0 * g.standard_normal((nl, H, W)), 8.0 * g.standard_normal((nl, H, W)), 1.0e5 + dsp + 2.0e3 * g.standard_normal((1, H, W))]
    x = np.concatenate(state(0.0, 1.0, 0.0) + [g.standard_normal((2, H, W))], 0)
    y_state = state(2.0, 1.3, -500.0)   # a warmer, moister, lighter prediction: every fixer has a correction far above its gate to make
    # flux channels of distinct, non-zero global means (J/m2): dropping or mis-signing any one term moves the energy ratio visibly
    flux = (1.0 + 0.3 * np.arange(12))[:, None, None] * 1.0e6 + 5.0e5 * g.standard_normal((12, H, W))
    # precipitation / evaporation of one sign and large against the change of column water: the water ratio
    # (-d(TWC) - E) / P is then a quotient of sums that do not cancel
    # (and it rains four times as much at the equator as at the poles: a sum that loses some rows gives another ratio)
    precip = (np.abs(1.0e-2 * g.standard_normal((1, H, W))) + 1.0e-3) * (1.0 + 3.0 * np.cos(np.deg2rad(lat))[None, :, None] ** 2)
    evapor = -np.abs(5.0e-3 * g.standard_normal((1, H, W)))
    y = np.concatenate(y_state + [flux, precip, evapor], 0)
    lay = dict(nl=nl, T=0, q=nl, U=2 * nl, V=3 * nl, sp=4 * nl, toa=[4 * nl + 1 + k for k in range(4)],
               surf=[4 * nl + 5 + k for k in range(8)], precip=4 * nl + 13, evapor=4 * nl + 14, c_in=4 * nl + 3, c_out=4 * nl + 15)
    stats = None
    if c["denorm"]:   # four distinct vectors, distinct per channel: mean_in != mean_out and std_in != std_out everywhere
        def vec(n):
            blk = [(250.0, 30.0)] * nl + [(4e-3, 4e-3)] * nl + [(1.0, 12.0)] * nl + [(-1.0, 8.0)] * nl + [(1.0e5, 2.0e3)]
            blk += [(0.1, 1.0)] * 2 if n == lay["c_in"] else [(1.0e5, 2.0e6)] * 12 + [(8e-3, 6e-3), (-4e-3, 3e-3)]
            k = np.arange(n)
            return np.array([b[0] for b in blk]) + 0.01 * k * np.array([b[1] for b in blk]), np.array([b[1] for b in blk]) * (1.0 + 0.01 * k)
        mo, so = vec(lay["c_out"])
        mi, si = vec(lay["c_in"])
        mi, si = mi + 0.3 * si, 1.25 * si
        stats = tuple(v.astype(np.float32) for v in (mi, si, mo, so))
        x = (x - stats[0][:, None, None].astype(np.float64)) / stats[1][:, None, None]
        y = (y - stats[2][:, None, None].astype(np.float64)) / stats[3][:, None, None]
    xf = np.full((lay["c_in"], c["frames"], H, W), np.nan, np.float32)   # earlier frames NaN: a read of the wrong frame shows
    xf[:, -1] = x
    return dict(case=c, lay=lay, lat2d=lat2d, lon2d=lon2d, p=p.astype(np.float32), coef_a=coef_a.astype(np.float32), coef_b=coef_b,
                gph=(500.0 + 200.0 * g.standard_normal((H, W))).astype(np.float32), x=xf, y=y.astype(np.float32), stats=stats,
                n_seconds=6 * 3600.0, tracer=dict(inds=list(range(nl, 2 * nl)) + [lay["precip"]], thres=[5e-4] * nl + [2e-3],
                                                  thres_max=[1.2e-2] * nl + [6.0e-2]))


def fixer_case_terms(inp):
    """[(toa terms), (surface terms)] as (channel, sign) lists of the case's energy fixer, or None."""
    lay, fixer = inp["lay"], inp["case"]["fixer"]
    t, s = lay["toa"], lay["surf"]
    if fixer in ("energy", "chain"):
        return [(t[0], 1.0), (t[1], 1.0)], [(s[k], 1.0) for k in range(4)]
    if fixer == "updown":
        return [(t[0], 1.0), (t[1], -1.0), (t[2], -1.0)], list(zip(s[:6], (1.0, -1.0, 1.0, -1.0, -1.0, -1.0)))
    if fixer == "signed48":
        return list(zip(t, SIGNED_48["toa"])), list(zip(s, SIGNED_48["surf"]))
    if fixer == "signed11":
        return [(t[3], SIGNED_11["toa"][0])], [(s[7], SIGNED_11["surf"][0])]
    return None


def fixer_case_oracle(inp, dtype, terms=None):
    """The case through oracle/fixers_oracle.py in `dtype` (fp32: the fp32 grid, as the reference computes); `terms` replaces the
    case's own flux terms."""
    from oracle import fixers_oracle as F
    c, lay = inp["case"], inp["lay"]
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)   # noqa: E731
    x, y, gph = t(inp["x"][:, -1]), t(inp["y"]), t(inp["gph"])
    st = inp["stats"]
    stats = None if st is None else {"in": (t(st[0]), t(st[1])), "out": (t(st[2]), t(st[3]))}
    nl, ns, q, sp = lay["nl"], inp["n_seconds"], lay["q"], lay["sp"]
    if c["sigma"]:
        grid = F.SigmaGrid(inp["lat2d"], inp["lon2d"], inp["coef_a"], inp["coef_b"], midpoint=c["midpoint"], dtype=dtype)
        mass = lambda v: F.mass_fixer_sigma(v, x, grid, q, nl, sp, stats)   # noqa: E731
        water = lambda v: F.water_fixer_sigma(v, x, grid, q, nl, lay["precip"], lay["evapor"], sp, ns, stats)   # noqa: E731
    else:
        grid = F.Grid(inp["lat2d"], inp["lon2d"], inp["p"], midpoint=c["midpoint"], dtype=dtype)
        mass = lambda v: F.mass_fixer(v, x, grid, q, nl, c["fix"], stats)   # noqa: E731
        water = lambda v: F.water_fixer(v, x, grid, q, nl, lay["precip"], lay["evapor"], ns, stats)   # noqa: E731
    terms = terms or fixer_case_terms(inp)
    energy = lambda v: F.energy_fixer_signed(v, x, grid, lay["T"], q, lay["U"], lay["V"], nl, terms[0], terms[1], gph, ns, stats,   # noqa: E731
                                             sp if c["sigma"] else None)
    if c["fixer"] == "mass":
        return mass(y)
    if c["fixer"] == "water":
        return water(y)
    if c["fixer"] == "chain":
        tr = inp["tracer"]
        return energy(water(mass(F.tracer_fixer(y, tr["inds"], tr["thres"], tr["thres_max"], stats))))
    return energy(y)


def fixer_case_owned(inp):
    """[(channel slice, gate)] of the blocks the case's fixers own; every other channel must come back bit-identical."""
    c, lay = inp["case"], inp["lay"]
    nl = lay["nl"]
    T, q, sp, pr = slice(0, nl), slice(nl, 2 * nl), slice(lay["sp"], lay["sp"] + 1), slice(lay["precip"], lay["precip"] + 1)
    one = FIXER_GATES["single"]
    if c["fixer"] == "mass":
        return [(sp if c["sigma"] else q, one)]
    if c["fixer"] == "water":
        return [(pr, one)]
    if c["fixer"] == "chain":   # the tracer clamps q and precipitation; the mass fixer then owns q (pressure) or SP (sigma)
        return [(T, FIXER_GATES["chain"]), (q, FIXER_GATES["chain"]), (pr, FIXER_GATES["chain_precip"])] + (
            [(sp, FIXER_GATES["chain"])] if c["sigma"] else [])
    return [(T, one)]


def fixer_block_error(got, ref, blk):
    """max|got - ref| / max|ref| over a channel block, in the units the tensor is stored in."""
    got, ref = np.asarray(got, np.float64)[blk], np.asarray(ref, np.float64)[blk]
    return float(np.abs(got - ref).max() / np.abs(ref).max())
