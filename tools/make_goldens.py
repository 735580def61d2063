#!/usr/bin/env python
"""Generate golden fixtures from the REAL reference (dev container only).

Imports NCAR/miles-credit from /root/reference (read-only, via tools/oracle_stub.py),
loads the build's synthetic name-keyed weights (wxengine.synth) with strict=True into
`credit.models.crossformer.CrossFormer`, runs it on CPU fp32 and stores outputs as
small .npz files under tests/golden/.  Only data (inputs are regenerated from the
keyed RNG; outputs / strided samples / per-channel statistics) is written — no
reference source.

    python tools/make_goldens.py [--only T0,T1,C1,C3S,C3,pad,glue,diag,xform,wind,advect,hybrid,regrid,metrics,ensemble,camulator]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tools"), os.path.join(ROOT, "miles-credit_amd"), ROOT]

import oracle_stub  # noqa: E402

oracle_stub.install()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from wxengine.config import named_config  # noqa: E402
from wxengine.synth import synth_denorm, synth_forcing, synth_input, synth_state_dict  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def reference_model(cfg, post_conf=None, family="base"):
    if getattr(cfg, "arch", "crossformer") == "camulator":
        return camulator_reference(cfg, post_conf)
    if getattr(cfg, "arch", "crossformer") == "wxformer":
        from credit.models.wxformer.crossformer import CrossFormer
    else:
        from credit.models.crossformer import CrossFormer
    m = CrossFormer(
        image_height=cfg.image_height, image_width=cfg.image_width, frames=cfg.frames, channels=cfg.channels,
        surface_channels=cfg.surface_channels, input_only_channels=cfg.input_only_channels,
        output_only_channels=cfg.output_only_channels, levels=cfg.levels, dim=cfg.dim, depth=cfg.depth,
        dim_head=cfg.dim_head, global_window_size=cfg.global_window_size,
        local_window_size=cfg.local_window_size[0], cross_embed_kernel_sizes=cfg.cross_embed_kernel_sizes,
        cross_embed_strides=cfg.cross_embed_strides, use_spectral_norm=cfg.use_spectral_norm, interp=cfg.interp,
        **({"upsample_v_conv": True} if getattr(cfg, "upsample_v_conv", False) else {}),
        padding_conf={"activate": cfg.pad_activate, "mode": getattr(cfg, "pad_mode", "earth"), "pad_lat": list(cfg.pad_lat),
                      "pad_lon": list(cfg.pad_lon)},
        post_conf=post_conf or {"activate": False})
    sd = synth_state_dict(cfg, family=family)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m.eval()
    return m


def camulator_reference(cfg, post_conf=None):
    """credit.models.camulator.Camulator on CPU with the synthetic weights, strict load (the class takes no output_frames)."""
    from credit.models.camulator import Camulator
    m = Camulator(
        image_height=cfg.image_height, image_width=cfg.image_width, frames=cfg.frames, channels=cfg.channels,
        surface_channels=cfg.surface_channels, input_only_channels=cfg.input_only_channels,
        output_only_channels=cfg.output_only_channels, levels=cfg.levels, dim=cfg.dim, depth=cfg.depth,
        dim_head=cfg.dim_head, global_window_size=cfg.global_window_size,
        local_window_size=tuple(cfg.local_window_size), cross_embed_kernel_sizes=cfg.cross_embed_kernel_sizes,
        cross_embed_strides=cfg.cross_embed_strides, use_spectral_norm=cfg.use_spectral_norm, interp=cfg.interp,
        padding_conf={"activate": cfg.pad_activate, "mode": getattr(cfg, "pad_mode", "earth"), "pad_lat": list(cfg.pad_lat),
                      "pad_lon": list(cfg.pad_lon)},
        post_conf=post_conf or {"activate": False})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg).items()}, strict=True)
    return m.eval()


def camulator_golden(name, stride, cap_stride=0, autocast=False):
    """model_<name>.npz of a camulator config in the layout of model_golden().  The hooked sub-module outputs are stored as
    stride-`cap_stride` samples with their full-map per-channel sums (the layout of reference_blocks_T1.npz), which keeps the file
    under the size limit of a committed file; the input of the first CrossEmbed -- pad(avg_pool3d(x)) -- goes in as `cap/pad`."""
    cfg = named_config(name)
    torch.manual_seed(0)
    m = camulator_reference(cfg)
    x = torch.from_numpy(synth_input(cfg))
    caps = {}
    hooks = []
    if cap_stride:
        want = {f"layers.{s}.{j}" for s in range(4) for j in (0, 1)} | {f"up_block{i}" for i in (1, 2, 3, 4)}
        for n, mod in m.named_modules():
            if n in want:
                hooks.append(mod.register_forward_hook(lambda _m, _i, o, n=n: caps.__setitem__(n, o.detach().clone())))
        hooks.append(m.layers[0][0].register_forward_pre_hook(lambda _m, i: caps.__setitem__("pad", i[0].detach().clone())))
    t = time.time()
    with torch.no_grad():
        y = m(x)
    dt = time.time() - t
    for h in hooks:
        h.remove()
    assert y.shape == (1, cfg.base_output_channels, 1) + tuple(cfg.out_hw), y.shape
    out = {}
    out["ch_sum"], out["ch_sumsq"], out["ch_maxabs"] = channel_stats(y)
    out["stride"] = np.int64(stride)
    out["y"] = y[0, :, 0, ::stride, ::stride].numpy().astype(np.float32)
    if cap_stride:
        out["cap_stride"] = np.int64(cap_stride)
        for n, v in caps.items():
            out["cap/" + n] = v[0, :, ::cap_stride, ::cap_stride].numpy().astype(np.float32)
            out["cap_sum/" + n] = v[0].double().sum(dim=(1, 2)).numpy()
    if autocast:   # what bf16 arithmetic costs at these widths, measured on the reference itself (as for the stress families)
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
            y16 = m(x).float()
        out["bf16_autocast_l2"] = np.float64((y16 - y).norm() / y.norm())
        print(f"[golden] {name}: reference under torch.autocast(bf16) vs its own fp32: rel-L2 {out['bf16_autocast_l2']:.3e}")
    np.savez_compressed(os.path.join(GOLD, f"model_{name}.npz"), **out)
    print(f"[golden] {name}: {len(m.state_dict())} keys, forward {dt:.2f}s  mean|y|={y.abs().mean():.4f} max|y|={y.abs().max():.4f}  "
          f"y sample {out['y'].shape}")


def camulator_post_golden():
    """model_K0F_post.npz: the reference Camulator with its in-model PostBlock (TracerFixer + GlobalMassFixer, simple_demo grid) on
    the case of tests/camulator_cases.py.  y of the same weights with the PostBlock off goes in too: the channels no fixer owns must
    equal it."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from camulator_cases import post_model_conf
    from wxengine.config import WXConfig
    out = {}
    for tag, post in (("y_plain", False), ("y", True)):
        mc = post_model_conf(post)
        cfg = WXConfig.from_model_conf(mc, arch="camulator")
        m = camulator_reference(cfg, mc["post_conf"])
        x = torch.from_numpy(synth_input(cfg))
        with torch.no_grad():
            y = m(x)
        assert y.shape == (1, cfg.base_output_channels, 1, 10, 18), y.shape
        out[tag] = y[0, :, 0].numpy().astype(np.float32)
    L = 7
    moved = np.abs(out["y"] - out["y_plain"]).reshape(out["y"].shape[0], -1).max(axis=1)
    assert (moved[L:2 * L] > 0).all() and (np.delete(moved, np.arange(L, 2 * L)) == 0).all(), moved
    np.savez_compressed(os.path.join(GOLD, "model_K0F_post.npz"), **out)
    print(f"[golden] K0F_post: the fixers move q by up to {moved.max():.3e} (max|q| {np.abs(out['y'][L:2 * L]).max():.3f}); "
          f"{int((out['y_plain'][L:2 * L] < 0).sum())} values below the tracer threshold")


def channel_stats(y):
    """per-channel sum, sum of squares, max-abs of [1,C,1,H,W]."""
    a = y[0, :, 0].double()
    return (a.sum(dim=(1, 2)).numpy(), (a * a).sum(dim=(1, 2)).numpy(), a.abs().amax(dim=(1, 2)).numpy())


def model_golden(name, stride, capture_layers, family="base"):
    """family != base: the stress weight families of wxengine.synth -> model_<name>_<family>.npz"""
    cfg = named_config(name)
    torch.manual_seed(0)
    m = reference_model(cfg, family=family)
    x = torch.from_numpy(synth_input(cfg))
    caps = {}
    hooks = []
    if capture_layers:
        want = {f"layers.{s}.0" for s in range(4)} | {f"layers.{s}.1" for s in range(4)}
        want |= {"up_block1", "up_block2", "up_block3", "up_block4"}
        for n, mod in m.named_modules():
            if n in want:
                hooks.append(mod.register_forward_hook(
                    lambda _m, _i, o, n=n: caps.__setitem__(n, o.detach().clone())))
    t = time.time()
    with torch.no_grad():
        y = m(x)
    dt = time.time() - t
    for h in hooks:
        h.remove()
    out = {}
    s1, s2, mx = channel_stats(y)
    out["ch_sum"], out["ch_sumsq"], out["ch_maxabs"] = s1, s2, mx
    out["stride"] = np.int64(stride)
    out["y"] = y[0, :, 0, ::stride, ::stride].numpy().astype(np.float32)
    for n, v in caps.items():
        out["cap/" + n] = v[0].numpy().astype(np.float32)
    if family != "base":
        # what bf16 ARITHMETIC costs on this family, measured on the reference itself: the same module under torch.autocast(bfloat16)
        # against its own fp32 output.  The bf16 engine is gated against this number (it must not be worse than the framework's own bf16).
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
            y16 = m(x).float()
        out["bf16_autocast_l2"] = np.float64((y16 - y).norm() / y.norm())
        print(f"[golden] {name} ({family}): reference under torch.autocast(bf16) vs its own fp32: rel-L2 {out['bf16_autocast_l2']:.3e}")
    np.savez_compressed(os.path.join(GOLD, f"model_{name}.npz" if family == "base" else f"model_{name}_{family}.npz"), **out)
    print(f"[golden] {name} ({family}): forward {dt:.2f}s  mean|y|={y.abs().mean():.4f} max|y|={y.abs().max():.4f}  "
          f"y sample {out['y'].shape}")


def layout_golden():
    """build_channel_layout + update_x (credit/datasets/gen_2/channel_utils.py:161-291) on a TWO-source config: the prognostic /
    static / forcing channels of the sources interleave in x, and y carries each source's diagnostics after its prognostics."""
    from credit.datasets.gen_2.channel_utils import build_channel_layout, update_x
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from synth_batches import two_source_conf
    conf = two_source_conf()
    groups, n_pred = build_channel_layout(conf)
    code = {"prognostic": 0, "dynamic_forcing": 1, "static": 2}
    rows = [(code[g.field_type], g.x_slice.start, -1 if g.src_slice is None else g.src_slice.start, g.x_slice.stop - g.x_slice.start)
            for g in groups.values()]
    c_in = max(g.x_slice.stop for g in groups.values())
    g = np.random.Generator(np.random.Philox(key=[11, 3]))
    x = torch.from_numpy(g.standard_normal((1, c_in, 1, 5, 6), dtype=np.float32))
    frc = torch.from_numpy(g.standard_normal((1, 3, 1, 5, 6), dtype=np.float32))
    y = torch.from_numpy(g.standard_normal((1, 11, 1, 5, 6), dtype=np.float32))
    xn = update_x(x, frc, y, groups)
    np.savez_compressed(os.path.join(GOLD, "channel_layout_two_sources.npz"), groups=np.array(rows, dtype=np.int64), n_pred=np.int64(n_pred),
                        keys=np.array(list(groups.keys())), x=x.numpy(), frc=frc.numpy(), y=y.numpy(), x_new=xn.numpy())
    print(f"[golden] layout: {len(rows)} groups, n_pred {n_pred}, c_in {c_in}: {rows}")


def pad_golden():
    """credit/boundary_padding.py earth mode, incl. asymmetric pads (tests/test_bondary_padding.py:37-44 shapes)."""
    from credit.boundary_padding import TensorPadding
    out = {}
    g = np.random.Generator(np.random.Philox(key=[7, 7]))
    small = torch.from_numpy(g.standard_normal((1, 2, 1, 7, 10), dtype=np.float32))
    tp = TensorPadding(mode="earth", pad_lat=[3, 2], pad_lon=[4, 3])
    out["small_x"] = small.numpy()
    out["small_pad"] = tp.pad(small).numpy()
    big = torch.from_numpy(g.standard_normal((1, 3, 1, 181, 360), dtype=np.float32))
    tp2 = TensorPadding(mode="earth", pad_lat=[12, 34], pad_lon=[56, 78])
    pb = tp2.pad(big)
    assert torch.equal(tp2.unpad(pb), big)
    out["big_seed"] = np.array([7, 7])
    out["big_pad_strided"] = pb[0, :, 0, ::7, ::11].numpy()
    out["big_pad_sum"] = pb.double().sum(dim=(0, 2, 3, 4)).numpy()
    out["big_pad_shape"] = np.array(pb.shape)
    # mode "mirror" (boundary_padding.py:98-134) on the same shapes
    tm = TensorPadding(mode="mirror", pad_lat=[3, 2], pad_lon=[4, 3])
    out["small_mirror"] = tm.pad(small).numpy()
    tm2 = TensorPadding(mode="mirror", pad_lat=[12, 34], pad_lon=[56, 78])
    pm = tm2.pad(big)
    assert torch.equal(tm2.unpad(pm), big)
    out["big_mirror_strided"] = pm[0, :, 0, ::7, ::11].numpy()
    out["big_mirror_sum"] = pm.double().sum(dim=(0, 2, 3, 4)).numpy()
    np.savez_compressed(os.path.join(GOLD, "earth_pad.npz"), **out)
    print("[golden] earth_pad + mirror:", tuple(pb.shape), tuple(pm.shape))


def glue_conf(cfg, n_static=2, n_dyn=2):
    """Minimal data config understood by build_channel_layout (single source)."""
    n_diag = cfg.output_only_channels
    return {
        "data": {"source": {"ERA5": {
            "levels": list(range(cfg.levels)),
            "variables": {
                "prognostic": {"vars_3D": [f"p3_{i}" for i in range(cfg.channels)],
                               "vars_2D": [f"p2_{i}" for i in range(cfg.surface_channels)]},
                "static": {"vars_2D": [f"s_{i}" for i in range(n_static)]},
                "dynamic_forcing": {"vars_2D": [f"f_{i}" for i in range(n_dyn)]},
                "diagnostic": {"vars_2D": [f"d_{i}" for i in range(n_diag)]},
            }}}},
        "model": {"levels": cfg.levels},
    }


def glue_golden():
    """3-step rollout on T0 through the reference's own pieces: model forward, TracerFixer
    (credit/postblock/gen1.py:111, denorm False so no scaler files are needed), y*std+mean
    (rollout_to_netcdf.py:287) and update_x (channel_utils.py:253)."""
    from credit.datasets.gen_2.channel_utils import build_channel_layout, update_x
    from credit.postblock.gen1 import TracerFixer
    cfg = named_config("T0")
    m = reference_model(cfg)
    conf = glue_conf(cfg)
    groups, n_pred = build_channel_layout(conf)
    assert n_pred == cfg.channels * cfg.levels + cfg.surface_channels
    q_inds = list(range(3 * cfg.levels, 4 * cfg.levels))  # 4th 3-D variable = the tracer
    thres = [-0.05] * len(q_inds)  # normalised-space threshold that actually clamps
    fixer = TracerFixer({"tracer_fixer": {"tracer_inds": q_inds, "tracer_thres": thres, "denorm": False}})
    mean, std = synth_denorm(cfg.base_output_channels)
    mean_t = torch.from_numpy(mean).view(1, -1, 1, 1, 1)
    std_t = torch.from_numpy(std).view(1, -1, 1, 1, 1)
    x = torch.from_numpy(synth_input(cfg))
    out = {"tracer_inds": np.array(q_inds), "tracer_thres": np.array(thres, dtype=np.float32),
           "n_static": np.int64(2), "n_dyn": np.int64(2)}
    with torch.no_grad():
        for step in range(1, 4):
            y = m(x)
            n_clamped = int((y[:, q_inds] < thres[0]).sum())
            y = fixer({"y_pred": y, "x": x})["y_pred"]
            y_phys = (y * std_t + mean_t).squeeze(2)
            out[f"y{step}"] = y[0, :, 0].numpy().astype(np.float32)
            out[f"yphys{step}"] = y_phys[0].numpy().astype(np.float32)
            frc = torch.from_numpy(synth_forcing(cfg, 2, step))
            x = update_x(x, frc, y.detach(), groups)
            out[f"x{step}"] = x[0, :, 0].numpy().astype(np.float32)
            print(f"[golden] glue step {step}: clamped {n_clamped} tracer cells, mean|y|={y.abs().mean():.4f}")
    np.savez_compressed(os.path.join(GOLD, "rollout_T0.npz"), **out)


def long_rollout_golden(name, n_steps, stride, with_fp64=True, family="base", dense_steps=(), dense_stride=16):
    """Row R of SURVEY.md 8(a): the predict() loop (rollout_to_netcdf.py:262-316) for n_steps steps on a full-size grid, through the
    reference's own pieces -- CrossFormer forward (fp32, CPU), TracerFixer, y*std+mean, update_x -- and, beside it, the same
    trajectory from the fp64 oracle (oracle/wxformer_oracle.py::rollout).  Stored per step: strided samples of the
    normalised output of both, and per-channel (sum, sum of squares) of the reference output.  The distance between the two
    trajectories is the noise floor of the reference's OWN arithmetic: what an engine can be asked to match at step t."""
    from credit.datasets.gen_2.channel_utils import build_channel_layout, update_x
    from credit.postblock.gen1 import TracerFixer
    from oracle import wxformer_oracle as O
    cfg = named_config(name)
    m = reference_model(cfg, family=family)
    sd = synth_state_dict(cfg, family=family)
    groups, n_pred = build_channel_layout(glue_conf(cfg))
    q_inds = list(range(3 * cfg.levels, 4 * cfg.levels))
    thres = [-0.05] * len(q_inds)
    fixer = TracerFixer({"tracer_fixer": {"tracer_inds": q_inds, "tracer_thres": thres, "denorm": False}})
    x = torch.from_numpy(synth_input(cfg))
    x64 = x.double()
    x16 = x.clone()   # stress families: the reference's own loop under torch.autocast(bfloat16) -- what bf16 arithmetic costs per step
    ac = []
    out = {"tracer_inds": np.array(q_inds), "tracer_thres": np.array(thres, dtype=np.float32), "n_static": np.int64(2),
           "n_dyn": np.int64(2), "stride": np.int64(stride), "n_steps": np.int64(n_steps)}
    ys, y64s, sums, rel, dense = [], [], [], [], []
    t0 = time.time()
    # a 40-step 0.25-degree trajectory is ~35 min of CPU: checkpointed after every step, so an interrupted run resumes where it stopped
    ckpt = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"wx_rollout_golden_{name}_{family}_{n_steps}_{stride}.pt")
    first = 1
    if os.path.isfile(ckpt):
        st = torch.load(ckpt, weights_only=False)
        first, x, x64, x16, ys, y64s, sums, rel, dense, ac = st["step"] + 1, st["x"], st["x64"], st["x16"], st["ys"], st["y64s"], st["sums"], st["rel"], st["dense"], st["ac"]
        print(f"[golden] {name} ({family}) rollout: resuming at step {first} from {ckpt}", flush=True)
    with torch.no_grad():
        for step in range(first, n_steps + 1):
            frc = torch.from_numpy(synth_forcing(cfg, 2, step))
            y = fixer({"y_pred": m(x), "x": x})["y_pred"]
            x = update_x(x, frc, y.detach(), groups)
            if with_fp64:
                y64 = O.tracer_fix(O.forward(cfg, sd, x64, dtype=torch.float64), q_inds, thres)
                x64 = O.update_x(x64, frc.double(), y64, n_pred, 2)
            else:   # 0.25-degree grid: torch's fp64 CPU convolution of the k = 32 CrossEmbed branch wants 157 GB of scratch
                y64 = y.double()
            if family != "base":
                with torch.autocast("cpu", dtype=torch.bfloat16):
                    y16 = m(x16).float()
                y16 = fixer({"y_pred": y16, "x": x16})["y_pred"]
                x16 = update_x(x16, frc, y16.detach(), groups)
                ac.append(float((y16 - y).norm() / y.norm()))
            ys.append(y[0, :, 0, ::stride, ::stride].numpy().astype(np.float32))
            y64s.append(y64[0, :, 0, ::stride, ::stride].numpy().astype(np.float32))
            if step in dense_steps:   # a denser sample of a few steps (the strided one is one pixel in 1 600)
                dense.append(y[0, :, 0, ::dense_stride, ::dense_stride].numpy().astype(np.float32))
            s1, s2, _ = channel_stats(y)
            sums.append(np.stack([s1, s2]))
            d = (y.double() - y64)[0, :, 0]
            rel.append(float(d.norm() / y64[0, :, 0].norm()))
            torch.save({"step": step, "x": x, "x64": x64, "x16": x16, "ys": ys, "y64s": y64s, "sums": sums, "rel": rel, "dense": dense, "ac": ac}, ckpt + ".tmp")
            os.replace(ckpt + ".tmp", ckpt)
            print(f"[golden] {name} ({family}) rollout step {step}/{n_steps}: mean|y|={y.abs().mean():.4f}  reference-fp32 vs fp64 oracle "
                  f"rel-L2 {rel[-1]:.3e}" + (f"  reference under bf16 autocast {ac[-1]:.3e}" if ac else "") + f"  ({time.time() - t0:.0f}s)", flush=True)
    out["y"] = np.stack(ys)            # [n_steps, C_out, H/stride, W/stride]  reference, fp32
    # the fp64 oracle's trajectory at the same points (without it: an empty array -- tests then gate against the reference alone)
    out["y64"] = np.stack(y64s) if with_fp64 else np.zeros((0,), np.float32)
    out["ch_sums"] = np.stack(sums)    # [n_steps, 2, C_out] float64
    if dense:
        out["y_dense"], out["dense_steps"], out["dense_stride"] = np.stack(dense), np.array(list(dense_steps)), np.int64(dense_stride)
    out["ref_vs_fp64_rel_l2"] = np.array(rel) if with_fp64 else np.full(n_steps, np.nan)
    if ac:
        out["bf16_autocast_l2"] = np.array(ac)
    np.savez_compressed(os.path.join(GOLD, f"rollout_{name}.npz" if family == "base" else f"rollout_{name}_{family}.npz"), **out)
    if os.path.isfile(ckpt):
        os.remove(ckpt)


def swin_golden():
    """the shifted-window attention of credit/models/swin.py, run through the reference's OWN code where it is
    importable here: `SwinTransformerV2CrBlock._make_attention_mask` (:411-427) and `._shifted_window_attn` (:451-486) called on a
    duck-typed `self`, `window_partition / window_reverse` (:88-118) and `WindowMultiHeadAttention.forward` (:299-330: qkv Linear,
    scaled cosine attention, logit-scale clamp, mask, softmax, P V).  What is NOT reference code: the position-bias table fed into
    that forward -- the class computes it with `timm.layers.Mlp`, and timm is neither vendored nor pinned by the reference
    (SURVEY.md 8(c)), so the table is an input of the fixture (seeded) and the meta-MLP restatement in oracle/swin_oracle.py
    stays unpinned.  Stored: inputs, the seam mask, and the attention core's output (the tensor entering `proj`), image layout."""
    import types
    from credit.models import swin as R
    out = {}
    cases = {"rect_shift": ((12, 16), (4, 8), (2, 4), 2, 32), "fuxi_like": ((14, 21), (7, 7), (3, 3), 1, 128),
             "rect_noshift": ((12, 16), (4, 8), (0, 0), 2, 32), "lat_only_shift": ((16, 12), (8, 4), (5, 0), 3, 32)}
    for name, (feat, ws, shift, heads, hd) in cases.items():
        C = heads * hd
        g = torch.Generator().manual_seed(abs(hash(name)) % 2 ** 31 if False else sum(map(ord, name)))
        attn = R.WindowMultiHeadAttention.__new__(R.WindowMultiHeadAttention)
        torch.nn.Module.__init__(attn)
        attn.in_features, attn.window_size, attn.num_heads, attn.sequential_attn = C, ws, heads, False
        attn.qkv = torch.nn.Linear(C, 3 * C)
        attn.proj = torch.nn.Linear(C, C)
        attn.attn_drop = torch.nn.Identity()
        attn.proj_drop = torch.nn.Identity()
        with torch.no_grad():
            attn.qkv.weight.copy_(torch.randn(3 * C, C, generator=g) / C ** 0.5)
            attn.qkv.bias.copy_(torch.randn(3 * C, generator=g) * 0.1)
        attn.logit_scale = torch.nn.Parameter(torch.log(10 * torch.ones(heads)) + torch.randn(heads, generator=g) * 0.3)
        n = ws[0] * ws[1]
        bias = torch.randn(heads, n, n, generator=g) * 0.5
        attn._relative_positional_encodings = lambda b=bias: b.unsqueeze(0)     # the timm-Mlp part: supplied, see the docstring
        blk = types.SimpleNamespace(feat_size=feat, window_size=ws, shift_size=shift, window_area=n, attn=attn)
        blk.register_buffer = lambda k, v, persistent=False, b=blk: setattr(b, k, v)
        R.SwinTransformerV2CrBlock._make_attention_mask(blk)
        captured = {}
        h = attn.proj.register_forward_pre_hook(lambda _m, inp: captured.__setitem__("core", inp[0].detach().clone()))
        x = torch.randn(1, feat[0], feat[1], C, generator=g)
        with torch.no_grad():
            R.SwinTransformerV2CrBlock._shifted_window_attn(blk, x)
        h.remove()
        core = captured["core"].view(-1, ws[0], ws[1], C)                           # windows of the ROLLED map
        core = R.window_reverse(core, ws, feat)
        if any(shift):
            core = torch.roll(core, shifts=shift, dims=(1, 2))
        out[f"{name}/x"] = x[0].numpy().astype(np.float32)
        out[f"{name}/qkv_w"] = attn.qkv.weight.detach().numpy().astype(np.float32)
        out[f"{name}/qkv_b"] = attn.qkv.bias.detach().numpy().astype(np.float32)
        out[f"{name}/bias"] = bias.numpy().astype(np.float32)
        out[f"{name}/logit_scale_raw"] = attn.logit_scale.detach().numpy().astype(np.float32)
        out[f"{name}/core"] = core[0].numpy().astype(np.float32)
        out[f"{name}/mask"] = (blk.attn_mask.numpy().astype(np.float32) if blk.attn_mask is not None else np.zeros((0,), np.float32))
        out[f"{name}/geom"] = np.array([feat[0], feat[1], ws[0], ws[1], shift[0], shift[1], heads, hd], dtype=np.int64)
        print(f"[golden] swin {name}: feat {feat} ws {ws} shift {shift} heads {heads} hd {hd}  mean|core|={core.abs().mean():.4f}")
    np.savez_compressed(os.path.join(GOLD, "swin_attention.npz"), **out)


def swin_block_golden():
    """SURVEY.md 8(f) row 4, part 2: the whole Swin V2 (Cr) BLOCK and a two-block stage, through the reference's own code:
    `SwinTransformerV2CrBlock.forward` (:484-502), `._shifted_window_attn` (:451-486), `._make_attention_mask` (:411-427) and
    `._calc_window_shift` (:405-409) called on a duck-typed `self` that carries real `nn.Linear` / `nn.LayerNorm` modules, and
    `WindowMultiHeadAttention.forward`, `._relative_positional_encodings`, `._make_pair_wise_relative_positions` (:254-330) on a
    `WindowMultiHeadAttention` built without its constructor.  NOT reference code: `timm.layers.Mlp` (the block's `mlp` and the
    attention's `meta_mlp`) -- timm is neither vendored nor pinned; `_Mlp` below restates it as fc1 -> act -> fc2
    (eval mode: its dropouts are identities), which is the part of this fixture that stays unpinned.
    Blocks alternate shift 0 / window // 2 exactly as SwinTransformerV2CrStage (:616-640) builds them."""
    import types
    from credit.models import swin as R

    class _Mlp(torch.nn.Module):
        def __init__(self, i, h, o, act):
            super().__init__()
            self.fc1, self.act, self.fc2 = torch.nn.Linear(i, h), act(), torch.nn.Linear(h, o)

        def forward(self, x):
            return self.fc2(self.act(self.fc1(x)))

    out = {}
    cases = {"rect": ((12, 16), (4, 8), 2, 32, 2), "fuxi_like": ((14, 21), (7, 7), 1, 128, 2), "clipped": ((4, 16), (8, 8), 2, 32, 2)}
    for name, (feat, ws_t, heads, hd, depth) in cases.items():
        C = heads * hd
        g = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
        rnd = lambda *shape, s=1.0: torch.randn(*shape, generator=g) * s  # noqa: E731
        x = rnd(1, feat[0], feat[1], C)
        sd = {}
        ys = []
        cur = x
        for i in range(depth):
            blk = types.SimpleNamespace(dim=C, feat_size=feat, target_shift_size=tuple(0 if i % 2 == 0 else w // 2 for w in ws_t))
            blk.window_size, blk.shift_size = R.SwinTransformerV2CrBlock._calc_window_shift(blk, ws_t)
            ws = blk.window_size
            blk.window_area = ws[0] * ws[1]
            attn = R.WindowMultiHeadAttention.__new__(R.WindowMultiHeadAttention)
            torch.nn.Module.__init__(attn)
            attn.in_features, attn.window_size, attn.num_heads, attn.sequential_attn = C, ws, heads, False
            attn.qkv, attn.proj = torch.nn.Linear(C, 3 * C), torch.nn.Linear(C, C)
            attn.attn_drop, attn.proj_drop = torch.nn.Identity(), torch.nn.Identity()
            attn.meta_mlp = _Mlp(2, 48, heads, torch.nn.ReLU)
            attn.logit_scale = torch.nn.Parameter(torch.log(10 * torch.ones(heads)) + rnd(heads, s=0.3))
            R.WindowMultiHeadAttention._make_pair_wise_relative_positions(attn)
            blk.attn = attn
            blk.norm1, blk.norm2, blk.norm3 = torch.nn.LayerNorm(C), torch.nn.LayerNorm(C), torch.nn.Identity()
            blk.drop_path1, blk.drop_path2 = torch.nn.Identity(), torch.nn.Identity()
            blk.mlp = _Mlp(C, 4 * C, C, torch.nn.GELU)
            with torch.no_grad():
                for lin, sc in ((attn.qkv, C ** -0.5), (attn.proj, C ** -0.5), (blk.mlp.fc1, C ** -0.5), (blk.mlp.fc2, (4 * C) ** -0.5),
                                (attn.meta_mlp.fc1, 0.7), (attn.meta_mlp.fc2, 0.15)):
                    lin.weight.copy_(rnd(*lin.weight.shape, s=sc))
                    lin.bias.copy_(rnd(*lin.bias.shape, s=0.1))
                for nm in (blk.norm1, blk.norm2):
                    nm.weight.copy_(1.0 + rnd(C, s=0.2))
                    nm.bias.copy_(rnd(C, s=0.1))
            blk.register_buffer = lambda k, v, persistent=False, b=blk: setattr(b, k, v)
            R.SwinTransformerV2CrBlock._make_attention_mask(blk)
            blk._shifted_window_attn = types.MethodType(R.SwinTransformerV2CrBlock._shifted_window_attn, blk)
            with torch.no_grad():
                cur = R.SwinTransformerV2CrBlock.forward(blk, cur)
            ys.append(cur[0].numpy().astype(np.float32))
            for mod, pre in ((attn.qkv, "attn.qkv."), (attn.proj, "attn.proj."), (attn.meta_mlp.fc1, "attn.meta_mlp.fc1."),
                             (attn.meta_mlp.fc2, "attn.meta_mlp.fc2."), (blk.norm1, "norm1."), (blk.norm2, "norm2."),
                             (blk.mlp.fc1, "mlp.fc1."), (blk.mlp.fc2, "mlp.fc2.")):
                sd[f"blocks.{i}.{pre}weight"] = mod.weight.detach().numpy().astype(np.float32)
                sd[f"blocks.{i}.{pre}bias"] = mod.bias.detach().numpy().astype(np.float32)
            sd[f"blocks.{i}.attn.logit_scale"] = attn.logit_scale.detach().numpy().astype(np.float32)
        out[f"{name}/x"] = x[0].numpy().astype(np.float32)
        out[f"{name}/geom"] = np.array([feat[0], feat[1], ws_t[0], ws_t[1], heads, hd, depth], dtype=np.int64)
        for k, v in sd.items():
            out[f"{name}/sd/{k}"] = v
        for i, y in enumerate(ys):
            out[f"{name}/y{i}"] = y
        print(f"[golden] swin block {name}: feat {feat} window {ws_t} heads {heads} hd {hd} depth {depth}  mean|y|={np.abs(ys[-1]).mean():.4f}")
    np.savez_compressed(os.path.join(GOLD, "swin_block.npz"), **out)


def attend_golden():
    """SURVEY.md 8(f) row 4, `Attend` (credit/attend.py:94-120, the non-flash branch: softmax(q k^T * scale) v per batch item and
    head) run through the reference class itself.  Stored: q, k, v [b, h, n, d] and the output, two shapes / both scale conventions."""
    from credit.attend import Attend
    out = {}
    for name, (b, h, n, d, scale) in {"n64_d32": (3, 4, 64, 32, None), "n128_d64_scaled": (2, 2, 128, 64, 0.2), "n100_d32": (2, 4, 100, 32, None)}.items():
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        q, k, v = (torch.randn(b, h, n, d, generator=g) for _ in range(3))
        att = Attend(dropout=0.0, flash=False, scale=scale).eval()
        with torch.no_grad():
            o = att(q, k, v)
        for nm, t in (("q", q), ("k", k), ("v", v), ("out", o)):
            out[f"{name}/{nm}"] = t.numpy().astype(np.float32)
        out[f"{name}/scale"] = np.array([np.nan if scale is None else scale], dtype=np.float32)
        print(f"[golden] attend {name}: {tuple(q.shape)} scale {scale} mean|out|={o.abs().mean():.4f}")
    np.savez_compressed(os.path.join(GOLD, "attend.npz"), **out)


FUXI_CASES = ("FT0", "FT1", "FT2", "FT3", "FT4", "FT5", "FT6", "FT7")


def fuxi_golden(names=FUXI_CASES):
    """`--only fuxi` writes every case, `--only fuxi:FT3+FT4` only the named ones (the other golden files stay as they are).
    BASELINE config 5: the FuXi forward through the reference's own modules (credit/models/fuxi.py): `CubeEmbedding`, `DownBlock`,
    `UpBlock`, `get_pad2d`, `UTransformer.forward`, `Fuxi.forward`, `apply_spectral_norm`, the two classes built without their
    constructors (which need timm) and populated with exactly the attributes those constructors set.  In the place of timm's
    `SwinTransformerV2Stage` (not vendored, not pinned: SURVEY.md 8(c)) sits a stage of the reference's OWN V2-Cr blocks
    (credit/models/swin.py: `SwinTransformerV2CrBlock.forward / _shifted_window_attn / _make_attention_mask / _calc_window_shift`,
    `WindowMultiHeadAttention.forward`), shift alternating 0 / window // 2 as SwinTransformerV2CrStage (:616-640) builds them; `_Mlp`
    restates timm.layers.Mlp (fc1 -> act -> fc2).  Weights: wxengine.fuxi.synth_fuxi_state_dict, loaded strict=True -- which also
    pins the key names and shapes of FuxiConfig.state_spec() outside the stage.  Stored: y and four intermediate maps."""
    from credit.models import fuxi as RF
    from credit.models import swin as RS
    from wxengine.fuxi import named_fuxi_config, synth_fuxi_state_dict
    from wxengine.synth import keyed_normal
    nn = torch.nn

    class _Mlp(nn.Module):
        def __init__(self, i, h, o, act):
            super().__init__()
            self.fc1, self.act, self.fc2 = nn.Linear(i, h), act(), nn.Linear(h, o)

        def forward(self, x):
            return self.fc2(self.act(self.fc1(x)))

    class _CrBlock(nn.Module):
        forward = RS.SwinTransformerV2CrBlock.forward
        _shifted_window_attn = RS.SwinTransformerV2CrBlock._shifted_window_attn
        _make_attention_mask = RS.SwinTransformerV2CrBlock._make_attention_mask
        _calc_window_shift = RS.SwinTransformerV2CrBlock._calc_window_shift

        def __init__(self, C, feat, ws_t, heads, shifted, meta_hidden):
            super().__init__()
            self.dim, self.feat_size = C, feat
            self.target_shift_size = tuple(w // 2 if shifted else 0 for w in ws_t)
            self.window_size, self.shift_size = self._calc_window_shift(ws_t)
            self.window_area = self.window_size[0] * self.window_size[1]
            attn = RS.WindowMultiHeadAttention.__new__(RS.WindowMultiHeadAttention)
            nn.Module.__init__(attn)
            attn.in_features, attn.window_size, attn.num_heads, attn.sequential_attn = C, self.window_size, heads, False
            attn.qkv, attn.proj = nn.Linear(C, 3 * C), nn.Linear(C, C)
            attn.attn_drop, attn.proj_drop = nn.Identity(), nn.Identity()
            attn.meta_mlp = _Mlp(2, meta_hidden, heads, nn.ReLU)
            attn.logit_scale = nn.Parameter(torch.zeros(heads))
            attn._make_pair_wise_relative_positions()
            self.attn = attn
            self.norm1, self.norm2, self.norm3 = nn.LayerNorm(C), nn.LayerNorm(C), nn.Identity()
            self.drop_path1, self.drop_path2 = nn.Identity(), nn.Identity()
            self.mlp = _Mlp(C, 4 * C, C, nn.GELU)
            self._make_attention_mask()

    class _CrStage(nn.Module):
        def __init__(self, C, feat, window, heads, depth, meta_hidden):
            super().__init__()
            self.blocks = nn.ModuleList([_CrBlock(C, feat, (window, window), heads, i % 2 == 1, meta_hidden) for i in range(depth)])

        def forward(self, x):
            for b in self.blocks:
                x = b(x)
            return x

    for name in names:
        if name not in FUXI_CASES:
            raise KeyError(f"fuxi golden: no case named {name}")
        cfg = named_fuxi_config(name)
        img = (cfg.frames, cfg.image_height, cfg.image_width)
        patch = (cfg.frame_patch_size, cfg.patch_height, cfg.patch_width)
        m = RF.Fuxi.__new__(RF.Fuxi)
        nn.Module.__init__(m)
        # the attributes Fuxi.__init__ (:358-452) sets, padding_conf / post_conf / noise off
        m.use_interp, m.use_spectral_norm, m.use_padding, m.use_post_block = cfg.interp, cfg.use_spectral_norm, False, False
        m.img_size_original = m.img_size = img
        m.patch_size = patch
        m.input_resolution = (round(img[1] / patch[1] / 2), round(img[2] / patch[2] / 2))
        m.out_chans = cfg.out_chans
        m.cube_embedding = RF.CubeEmbedding(img, patch, cfg.in_chans, cfg.dim)
        ut = RF.UTransformer.__new__(RF.UTransformer)
        nn.Module.__init__(ut)
        # UTransformer.__init__ (:216-276)
        ut.padding = RF.get_pad2d(m.input_resolution, (cfg.window_size, cfg.window_size))
        ut.pad = nn.ZeroPad2d(ut.padding)
        res = (m.input_resolution[0] + ut.padding[2] + ut.padding[3], m.input_resolution[1] + ut.padding[0] + ut.padding[1])
        assert res == cfg.stage_feat, (res, cfg.stage_feat)
        ut.down = RF.DownBlock(cfg.dim, cfg.dim, cfg.groups[0])
        ut.layer = _CrStage(cfg.dim, res, cfg.window_size, cfg.num_heads, cfg.depth, cfg.meta_hidden)
        ut.up = RF.UpBlock(cfg.dim * 2, cfg.dim, cfg.groups[1])
        ut.use_noise = False
        m.u_transformer = ut
        m.fc = nn.Linear(cfg.dim, cfg.out_chans * patch[1] * patch[2])
        if cfg.use_spectral_norm:
            RF.apply_spectral_norm(m)
        sd = synth_fuxi_state_dict(cfg)
        res_ld = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        assert not res_ld.missing_keys and not res_ld.unexpected_keys
        m.eval()
        taps = {}
        hooks = [m.cube_embedding.register_forward_hook(lambda _m, _i, o: taps.__setitem__("embed", o[0, :, 0].permute(1, 2, 0))),
                 ut.down.register_forward_hook(lambda _m, _i, o: taps.__setitem__("down", o[0].permute(1, 2, 0))),
                 ut.layer.register_forward_hook(lambda _m, _i, o: taps.__setitem__("stage_padded", o[0])),
                 ut.register_forward_hook(lambda _m, _i, o: taps.__setitem__("up", o[0].permute(1, 2, 0)))]
        x = torch.from_numpy(keyed_normal("fuxi/x0", (1, cfg.in_chans, cfg.frames, cfg.image_height, cfg.image_width), 1000))
        with torch.no_grad():
            y = RF.Fuxi.forward(m, x)
        for h in hooks:
            h.remove()
        pl, _, pt, _ = ut.padding
        hd, wd = m.input_resolution
        taps["stage"] = taps.pop("stage_padded")[pt: pt + hd, pl: pl + wd]
        assert y.shape == (1, cfg.out_chans, 1, cfg.image_height, cfg.image_width)
        out = {"y": y[0, :, 0].numpy().astype(np.float32), "padding": np.array(ut.padding, dtype=np.int64)}
        for k, v in taps.items():
            out[k] = v.contiguous().numpy().astype(np.float32)
        np.savez_compressed(os.path.join(GOLD, f"fuxi_{name}.npz"), **out)
        print(f"[golden] fuxi {name}: in {tuple(x.shape)} stage map {res} padding {ut.padding}  mean|y|={y.abs().mean():.4f} "
              + " ".join(f"{k}:{tuple(v.shape)}" for k, v in taps.items()))


def fixer_inputs(seed=11):
    """Physically plausible random fields on the reference's 10x18 / 7-level demo grid.
    x: [T(7) | q(7) | U(7) | V(7)] x 2 frames; y: the same 28 + [TOA solar, TOA OLR, surf solar, surf LR, SH, LH, precip, evapor]."""
    g = np.random.Generator(np.random.Philox(key=[seed, 3]))
    H, W, L = 10, 18, 7

    def state():
        T = 250.0 + 30.0 * g.standard_normal((L, H, W))
        q = np.abs(0.004 + 0.004 * g.standard_normal((L, H, W)))
        U = 12.0 * g.standard_normal((L, H, W))
        V = 8.0 * g.standard_normal((L, H, W))
        return np.concatenate([T, q, U, V], 0)
    x = np.stack([state(), state()], 1).astype(np.float32)            # [28, 2, H, W]
    flux = 2.0e6 * g.standard_normal((6, H, W))
    precip = np.abs(2e-3 * g.standard_normal((1, H, W)))
    evapor = -np.abs(1e-3 * g.standard_normal((1, H, W)))
    y = np.concatenate([state() * 1.0, flux, precip, evapor], 0).astype(np.float32)  # [36, H, W]
    return x, y


def fixers_golden():
    """GlobalMassFixer / GlobalWaterFixer / GlobalEnergyFixer of the reference on its own simple_demo grid
    (credit/postblock/gen1.py:188-223), trapz and midpoint, denorm False."""
    from credit.postblock.gen1 import GlobalEnergyFixer, GlobalMassFixer, GlobalWaterFixer
    x_np, y_np = fixer_inputs()
    out = {"x": x_np, "y": y_np}
    L = 7
    for midpoint in (False, True):
        nl = L - 1 if midpoint else L      # midpoint variants take one level fewer (mid-level values)
        tag = "mid" if midpoint else "trapz"
        # channel layout for this variant: first nl levels of each 7-level block
        xs = np.concatenate([x_np[b * L:b * L + nl] for b in range(4)], 0)
        ys = np.concatenate([y_np[b * L:b * L + nl] for b in range(4)] + [y_np[28:]], 0)
        x = torch.from_numpy(xs)[None]
        y = torch.from_numpy(ys)[None, :, None]
        q0 = nl
        base = {"simple_demo": True, "denorm": False, "grid_type": "pressure", "midpoint": midpoint,
                "activate": True, "activate_outside_model": False}
        conf_m = {"global_mass_fixer": dict(base, fix_level_num=3, q_inds=list(range(q0, q0 + nl))),
                  "data": {"lead_time_periods": 6}}
        conf_w = {"global_water_fixer": dict(base, q_inds=list(range(q0, q0 + nl)), precip_ind=4 * nl + 6,
                                             evapor_ind=4 * nl + 7), "data": {"lead_time_periods": 6}}
        conf_e = {"global_energy_fixer": dict(base, T_inds=list(range(0, nl)), q_inds=list(range(q0, q0 + nl)),
                                              U_inds=list(range(2 * nl, 3 * nl)), V_inds=list(range(3 * nl, 4 * nl)),
                                              TOA_rad_inds=[4 * nl, 4 * nl + 1], surf_rad_inds=[4 * nl + 2, 4 * nl + 3],
                                              surf_flux_inds=[4 * nl + 4, 4 * nl + 5]), "data": {"lead_time_periods": 6}}
        with torch.no_grad():
            ym = GlobalMassFixer(conf_m)({"y_pred": y.clone(), "x": x.clone()})["y_pred"]
            yw = GlobalWaterFixer(conf_w)({"y_pred": y.clone(), "x": x.clone()})["y_pred"]
            ye = GlobalEnergyFixer(conf_e)({"y_pred": y.clone(), "x": x.clone()})["y_pred"]
            # chained, in PostBlock order (mass -> water -> energy)
            yc = GlobalEnergyFixer(conf_e)(GlobalWaterFixer(conf_w)(GlobalMassFixer(conf_m)(
                {"y_pred": y.clone(), "x": x.clone()})))["y_pred"]
        for name, t in (("mass", ym), ("water", yw), ("energy", ye), ("chain", yc)):
            assert t.shape == y.shape, (name, t.shape)
            out[f"{tag}_{name}"] = t[0, :, 0].double().numpy()
        print(f"[golden] fixers {tag}: mass dq max {float((ym - y).abs().max()):.3e}  water dP max "
              f"{float((yw - y).abs().max()):.3e}  energy dT max {float((ye - y).abs().max()):.3e}")
    np.savez_compressed(os.path.join(GOLD, "fixers_demo.npz"), **out)


def fixers_frames2_golden():
    """The three fixers handed an `x` of two DIFFERENT frames (they read x_input[:, ..., -1, ...], gen1.py:303, :515, :744):
    inputs [C, 2, H, W] and outputs only.  Frame 0 is a different state altogether, so reading it cannot pass."""
    from credit.postblock.gen1 import GlobalEnergyFixer, GlobalMassFixer, GlobalWaterFixer
    x_np, y_np = fixer_inputs(seed=17)
    x_np[:, 0] = x_np[:, 0] * 1.5 + 1.0     # frame 0: another magnitude as well as other noise
    out = {"x": x_np, "y": y_np}
    L = 7
    for midpoint in (False, True):
        nl = L - 1 if midpoint else L
        tag = "mid" if midpoint else "trapz"
        xs = np.concatenate([x_np[b * L:b * L + nl] for b in range(4)], 0)
        ys = np.concatenate([y_np[b * L:b * L + nl] for b in range(4)] + [y_np[28:]], 0)
        x = torch.from_numpy(xs)[None]             # [1, 4 nl, 2, H, W]
        y = torch.from_numpy(ys)[None, :, None]
        base = {"simple_demo": True, "denorm": False, "grid_type": "pressure", "midpoint": midpoint,
                "activate": True, "activate_outside_model": False}
        q_inds = list(range(nl, 2 * nl))
        conf_m = {"global_mass_fixer": dict(base, fix_level_num=3, q_inds=q_inds), "data": {"lead_time_periods": 6}}
        conf_w = {"global_water_fixer": dict(base, q_inds=q_inds, precip_ind=4 * nl + 6, evapor_ind=4 * nl + 7),
                  "data": {"lead_time_periods": 6}}
        conf_e = {"global_energy_fixer": dict(base, T_inds=list(range(0, nl)), q_inds=q_inds,
                                              U_inds=list(range(2 * nl, 3 * nl)), V_inds=list(range(3 * nl, 4 * nl)),
                                              TOA_rad_inds=[4 * nl, 4 * nl + 1], surf_rad_inds=[4 * nl + 2, 4 * nl + 3],
                                              surf_flux_inds=[4 * nl + 4, 4 * nl + 5]), "data": {"lead_time_periods": 6}}
        with torch.no_grad():
            ym = GlobalMassFixer(conf_m)({"y_pred": y.clone(), "x": x.clone()})["y_pred"]
            yw = GlobalWaterFixer(conf_w)({"y_pred": y.clone(), "x": x.clone()})["y_pred"]
            ye = GlobalEnergyFixer(conf_e)({"y_pred": y.clone(), "x": x.clone()})["y_pred"]
            yc = GlobalEnergyFixer(conf_e)(GlobalWaterFixer(conf_w)(GlobalMassFixer(conf_m)(
                {"y_pred": y.clone(), "x": x.clone()})))["y_pred"]
        # only the channels a fixer (or the chain) may change are stored: the rest equal y
        out[f"{tag}_mass"] = ym[0, nl:2 * nl, 0].numpy()
        out[f"{tag}_water"] = yw[0, 4 * nl + 6, 0].numpy()
        out[f"{tag}_energy"] = ye[0, :nl, 0].numpy()
        out[f"{tag}_chain"] = np.concatenate([yc[0, :2 * nl, 0].numpy(), yc[0, 4 * nl + 6:4 * nl + 7, 0].numpy()], 0)
        for name, t in (("mass", ym), ("water", yw), ("energy", ye), ("chain", yc)):
            assert t.shape == y.shape, (name, t.shape)
        print(f"[golden] two-frame fixers {tag}: mass dq max {float((ym - y).abs().max()):.3e}  water dP max "
              f"{float((yw - y).abs().max()):.3e}  energy dT max {float((ye - y).abs().max()):.3e}")
    # TracerFixer (gen1.py:136-167) on the q block and the precipitation of the same y; each threshold IS a value of its channel,
    # so `<` against `<=` and `>=` against `>` are both exercised at equality
    from credit.postblock.gen1 import TracerFixer
    inds = list(range(L, 2 * L)) + [4 * L + 6]
    pairs = [sorted((float(y_np[c, 2, 3]), float(y_np[c, 5, 7]))) for c in inds]
    conf_t = {"tracer_fixer": {"tracer_inds": inds, "tracer_thres": [p[0] for p in pairs], "tracer_thres_max": [p[1] for p in pairs],
                               "denorm": False}}
    with torch.no_grad():
        yt = TracerFixer(conf_t)({"y_pred": torch.from_numpy(y_np.copy())[None, :, None]})["y_pred"]
    out["tracer_inds"] = np.array(inds, np.int32)
    out["tracer_thres"] = np.array([p[0] for p in pairs], np.float64)
    out["tracer_thres_max"] = np.array([p[1] for p in pairs], np.float64)
    out["tracer"] = yt[0, inds, 0].numpy()
    print(f"[golden] tracer fixer: {int((yt[0, :, 0] != torch.from_numpy(y_np)).sum())} values clamped")
    np.savez_compressed(os.path.join(GOLD, "fixers_frames2.npz"), **out)


def fixers_updown_golden():
    """GlobalEnergyFixerUpDown of the reference on its simple_demo grid (gen1.py:866-879), trapz and midpoint.
    Channel layout of y: [T|q|U|V] + 9 flux channels [TOA dn solar, TOA up solar, OLR, surf dn solar, surf up solar, surf dn LW,
    surf up LW, SH, LH]."""
    from credit.postblock.gen1 import GlobalEnergyFixerUpDown
    x_np, y_np = fixer_inputs(seed=13)
    g = np.random.Generator(np.random.Philox(key=[13, 9]))
    L, H, W = 7, 10, 18
    flux = np.abs(3.0e6 * g.standard_normal((9, H, W))).astype(np.float32)
    out = {"x": x_np, "y": y_np[:28], "flux": flux}
    for midpoint in (False, True):
        nl = L - 1 if midpoint else L
        tag = "mid" if midpoint else "trapz"
        xs = np.concatenate([x_np[b * L:b * L + nl] for b in range(4)], 0)
        ys = np.concatenate([y_np[b * L:b * L + nl] for b in range(4)] + [flux], 0)
        x = torch.from_numpy(xs)[None]
        y = torch.from_numpy(ys)[None, :, None]
        f0 = 4 * nl
        cfg = {"simple_demo": True, "denorm": False, "grid_type": "pressure", "midpoint": midpoint, "activate": True,
               "activate_outside_model": False, "T_inds": list(range(0, nl)), "q_inds": list(range(nl, 2 * nl)),
               "U_inds": list(range(2 * nl, 3 * nl)), "V_inds": list(range(3 * nl, 4 * nl)),
               "TOA_down_solar_ind": f0, "TOA_up_solar_ind": f0 + 1, "TOA_up_OLR_ind": f0 + 2, "surf_down_solar_ind": f0 + 3,
               "surf_up_solar_ind": f0 + 4, "surf_down_LW_ind": f0 + 5, "surf_up_LW_ind": f0 + 6, "surf_SH_ind": f0 + 7,
               "surf_LH_ind": f0 + 8}
        with torch.no_grad():
            ye = GlobalEnergyFixerUpDown({"global_energy_fixer_updown": cfg, "data": {"lead_time_periods": 6}})(
                {"y_pred": y.clone(), "x": x.clone()})["y_pred"]
        out[f"{tag}_updown"] = ye[0, :, 0].double().numpy()
        print(f"[golden] updown energy fixer {tag}: dT max {float((ye - y).abs().max()):.3e}")
    np.savez_compressed(os.path.join(GOLD, "fixers_updown.npz"), **out)


def preblock_golden():
    """ERA5Normalizer (stats injected, the NetCDF reading bypassed: xarray is absent) -> ConcatToTensor of the reference."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from synth_batches import preblock_batch
    from credit.preblock.concat import ConcatToTensor
    from credit.preblock.norm import ERA5Normalizer
    batch, mean, std = preblock_batch()
    n = ERA5Normalizer.__new__(ERA5Normalizer)
    torch.nn.Module.__init__(n)
    n._mean = {k: torch.tensor(np.array(v), dtype=torch.float32) for k, v in mean.items()}
    n._std = {k: torch.tensor(np.array(v), dtype=torch.float32) for k, v in std.items()}
    x, meta = ConcatToTensor()(n(batch))
    cmap = meta["input"]["_channel_map"]
    out = {"x": x.numpy(), "keys": np.array(list(cmap.keys())), "starts": np.array([v["slice"].start for v in cmap.values()]),
           "stops": np.array([v["slice"].stop for v in cmap.values()])}
    x2, _ = ConcatToTensor()(batch)   # concatenation only
    out["x_raw"] = x2.numpy()
    np.savez_compressed(os.path.join(GOLD, "preblock.npz"), **out)
    print(f"[golden] preblock: x {tuple(x.shape)} order {list(cmap.keys())}")


def conservation_golden():
    """Gen-2 name-keyed fixers (credit/postblock/conservation.py) on a hybrid sigma grid; `get_forward_data` (xarray) is
    replaced by an in-memory provider of the arrays defined here, the classes and physics core run unmodified."""
    import credit.postblock.conservation as G2
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from synth_batches import conservation_batch
    lat = np.array([90, 70, 50, 30, 10, -10, -30, -50, -70, -90], dtype=np.float64)
    lon2d, lat2d = np.meshgrid(np.arange(0, 360, 20, dtype=np.float64), lat)

    class _V:
        def __init__(self, a):
            self.values = a
    out = {}
    for midpoint in (True, False):
        tag = "mid" if midpoint else "trapz"
        batch, gph = conservation_batch(midpoint=midpoint)
        fake = {"lon2d": _V(lon2d), "lat2d": _V(lat2d), "coef_a": _V(SIGMA_A), "coef_b": _V(SIGMA_B), "PHIS": _V(gph)}
        G2.get_forward_data = lambda _f: fake
        phys = dict(save_loc_physics="in-memory.nc", lon_lat_level_name=["lon2d", "lat2d", "coef_a", "coef_b"], grid_type="sigma",
                    midpoint=midpoint)
        P = "cam/prognostic/"
        D = "cam/diagnostic/2d/"
        fixers = [
            G2.TracerFixer([P + "3d/Qtot", D + "PRECT"], [1e-9, 0.0], [None, 1.0]),
            G2.GlobalMassFixer(P + "3d/Qtot", P + "2d/PS", **phys),
            G2.GlobalWaterFixer(P + "3d/Qtot", P + "2d/PS", D + "PRECT", D + "QFLX", 6, **phys),
            G2.GlobalEnergyFixerUpDown(P + "3d/T", P + "3d/Qtot", P + "3d/U", P + "3d/V", P + "2d/PS", ["PHIS"],
                                       "cam/dynamic_forcing/2d/SOLIN", D + "FSUTOA", D + "FLUT", D + "FSDS", D + "FSUS", D + "FLDS",
                                       D + "FLUS", D + "SHFLX", D + "LHFLX", 6, **phys)]
        with torch.no_grad():
            for f in fixers:
                batch = f(batch)
        for k in (P + "2d/PS", D + "PRECT", P + "3d/T", P + "3d/Qtot"):
            out[f"{tag}:{k}"] = batch["y_processed"]["cam"][k].numpy()
        print(f"[golden] gen-2 conservation chain {tag}: done")
    np.savez_compressed(os.path.join(GOLD, "conservation_gen2.npz"), **out)


def diag_golden():
    """Pressure-level products: the reference's GeopotentialDiagnostic -> PressureInterpDiagnostic -> MSLPDiagnostic chain (and with
    them its three column functions, credit/postblock/{geopotential,pressure_interp,mslp}.py) run unmodified in fp32 and in fp64 on
    every case of tests/diag_cases.py.  The classes read their coefficients through xarray, which is absent: a stand-in `xarray`
    module in sys.modules whose open_dataset serves the case's arrays takes its place.  Written per case: diag_<case>.npz (the 2-D
    inputs, coefficients, SHA-256 of every regenerated input, the fp32 outputs and d_ref = the reference's own fp32-against-fp64
    distance per output variable) and diag_<case>_f64.npz (the fp64 outputs as float32 differences from the fp32 ones).
    The generator refuses to write a fixture in which a discrete choice could flip between fp32 and fp64."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from diag_cases import DIAG_CASES, FIELD_ORDER, KEYS, SRC, case_inputs, distance, input_digest, output_names
    coef = {}
    standin = oracle_stub.serve_xarray(coef)
    import credit.postblock.geopotential as RG
    import credit.postblock.mslp as RM
    import credit.postblock.pressure_interp as RP
    RG.xr = RP.xr = standin   # in case an earlier item of this run imported them over the hollow stand-in

    for name, c in DIAG_CASES.items():
        inp = case_inputs(name)
        coef.update(a_half=inp["a_half"], b_half=inp["b_half"], a_model=inp["a_mid"], b_model=inp["b_mid"])
        fields = [KEYS[f] for f in FIELD_ORDER[:c["n_fields"]]]
        blocks = [RG.GeopotentialDiagnostic(output_name=KEYS["z"], surface_geopotential_var=KEYS["phis"], surface_pressure_var=KEYS["sp"],
                                            temperature_var=KEYS["T"], specific_humidity_var=KEYS["q"], flip_vertical=c["flip_vertical"]),
                  RP.PressureInterpDiagnostic(pressure_levels=c["plev"], interp_variables=fields, temperature_var=KEYS["T"],
                                              geopotential_var=KEYS["z"], surface_pressure_var=KEYS["sp"],
                                              surface_geopotential_var=KEYS["phis"]),
                  RM.MSLPDiagnostic(output_name=KEYS["mslp"], surface_pressure_var=KEYS["sp"], temperature_var=KEYS["t2m"],
                                    surface_geopotential_var=KEYS["phis"])]
        res = {}
        for dtype in (torch.float32, torch.float64):
            t = {k: torch.from_numpy(inp[k]).to(dtype) for k in ("T", "q", "u", "v", "sp", "t2m", "phis")}
            batch = {"y_processed": {SRC: {KEYS[k]: t[k] for k in ("T", "q", "u", "v", "sp", "t2m")}},
                     # GeopotentialDiagnostic.forward flattens PHIS without expanding it (geopotential.py:205-209), so the reference
                     # gets the static plane repeated over n_time; the device blocks take it with n_time == 1
                     "ic_raw": {SRC: {KEYS["phis"]: t["phis"].expand(-1, -1, c["T"], -1, -1)}}}
            with torch.no_grad():
                for blk in blocks:
                    batch = blk(batch)
            y = batch["y_processed"][SRC]
            pres = lambda k: y[f"{SRC}/derived_diagnostic/3d/{KEYS[k].split('/')[-1]}_PRES"]   # noqa: E731
            out = {"z_model": y[KEYS["z"]], "mslp": y[KEYS["mslp"]], "plev_T": pres("T"), "plev_Z": pres("z")}
            for f in FIELD_ORDER[:c["n_fields"]]:
                out[f"plev_{f}"] = pres(f)
            assert all(v.dtype == dtype for v in out.values()), name
            res[dtype] = {k: v.contiguous().numpy() for k, v in out.items()}
        # ---- no discrete choice may flip between the two precisions
        th = 150.0
        picks = []
        for dtype in (torch.float32, torch.float64):
            z = torch.from_numpy(res[dtype]["z_model"])
            d = torch.abs((z - torch.from_numpy(inp["phis"]).to(dtype)) / 9.80665 - th)
            if c["s2t"]:
                d = d.flip(1)
            picks.append(torch.argmin(d, dim=1))
            two = torch.sort(d, dim=1).values[:, :2]
            assert float((two[:, 1] - two[:, 0]).min()) >= 0.5, f"{name}: two levels within 0.5 m of being nearest to {th} m"
        assert torch.equal(picks[0], picks[1]), f"{name}: fp32 and fp64 choose different temp_height levels"
        for dt in (np.float32, np.float64):
            sh = inp["phis"].astype(dt) / dt(9.80665)
            assert min(np.abs(sh - 2000.0).min(), np.abs(sh - 2500.0).min()) >= 0.01, f"{name}: a surface height sits on a regime boundary"
            t2 = inp["t2m"].astype(dt)
            tto = t2 + dt(0.0065) * sh
            for thr in (290.5, 255.0):
                assert min(np.abs(t2 - thr).min(), np.abs(tto - thr).min()) >= 1e-3, f"{name}: a temperature sits on {thr} K"
        sh = inp["phis"] / np.float32(9.80665)
        t2, hb = inp["t2m"], np.broadcast_to(sh, inp["t2m"].shape)
        cover = {"phis == 0": (inp["phis"] == 0).any(), "< 2000 m": ((sh > 0) & (sh < 2000)).any(), "2000 - 2500 m": ((sh >= 2000) & (sh <= 2500)).any(),
                 "> 2500 m": (sh > 2500).any(), "mslp case 1": ((t2 <= 290.5) & (t2 + 0.0065 * hb > 290.5)).any(), "mslp warm": (t2 > 290.5).any(),
                 "mslp cold": (t2 < 255.0).any(), "below ground": (inp["plev_pa"].max() > inp["sp"]).any(), "sp range": inp["sp"].min() < 56000 and inp["sp"].max() > 100000}
        assert all(cover.values()), (name, cover)
        fix = {k: inp[k] for k in ("sp", "t2m", "phis", "a_half", "b_half", "a_mid", "b_mid", "plev_pa")}
        f64 = {}
        for k in ("T", "q", "u", "v", "sp", "t2m", "phis"):
            fix[f"sha256:{k}"] = np.array(input_digest(inp[k]))
        d_ref = {}
        for v in output_names(name):
            a32, a64 = res[torch.float32][v], res[torch.float64][v]
            assert np.isfinite(a32).all() and np.isfinite(a64).all(), (name, v)
            fix[f"f32:{v}"] = a32
            f64[f"d64:{v}"] = (a64 - a32.astype(np.float64)).astype(np.float32)
            d_ref[v] = distance(a32, a64)
            fix[f"d_ref:{v}"] = np.float64(d_ref[v])
        np.savez_compressed(os.path.join(GOLD, f"diag_{name}.npz"), **fix)
        np.savez_compressed(os.path.join(GOLD, f"diag_{name}_f64.npz"), **f64)
        sizes = [os.path.getsize(os.path.join(GOLD, f"diag_{name}{s}.npz")) for s in ("", "_f64")]
        assert max(sizes) < 1000000, (name, sizes)
        print(f"[golden] diag {name}: {inp['sp'].size} columns, files {sizes[0] // 1024} + {sizes[1] // 1024} KB, T range "
              f"{res[torch.float32]['plev_T'].min():.1f} .. {res[torch.float32]['plev_T'].max():.1f} K, d_ref "
              + ", ".join(f"{k} {v:.2e}" for k, v in d_ref.items()))


def wind_golden():
    """Wind artifact filter: the reference's WindArtifactFilter (credit/postblock/wind_filter.py) run unmodified in fp32, and its two
    helpers `_compute_blend_mask` / `_blend_smoothed` on double tensors (the class itself casts to float) as the fp64 side, on every
    case of tests/wind_cases.py.  Written per case: wind_<case>.npz (SHA-256 of every regenerated input, the fp32 blend mask and the
    fp32 FILTERED planes per target variable, d_ref = the reference's own fp32-against-fp64 distance per output) and
    wind_<case>_f64.npz (the fp64 outputs as float32 differences from the fp32 ones)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import credit.postblock.wind_filter as RW
    from diag_cases import distance
    from wind_cases import KEYS, SRC, WIND_CASES, case_inputs, filtered_levels, input_digest, output_names

    for name, c in WIND_CASES.items():
        inp = case_inputs(name)
        a = c["args"]
        targets = [KEYS[v] for v in c["targets"]]
        lv = filtered_levels(name)
        blk = RW.WindArtifactFilter(u_var=KEYS["U"], v_var=KEYS["V"], target_vars=targets, **a)
        batch = {"y_processed": {SRC: {KEYS[v]: torch.from_numpy(inp[v]) for v in ("U", "V", "T")}}}
        with torch.no_grad():
            y = blk(batch)["y_processed"][SRC]
            u, v = torch.from_numpy(inp["U"]), torch.from_numpy(inp["V"])
            common = (a["speed_threshold"], a["dilation_zonal"], a["dilation_meridional"], a["falloff_sigma"], a["smooth_sigma"],
                      a["smooth_sigma_zonal"], a["smooth_sigma_meridional"])
            m32, _ = RW._compute_blend_mask(u[:, a["mask_level"], 0], v[:, a["mask_level"], 0], *common)
            m64, g64 = RW._compute_blend_mask(u[:, a["mask_level"], 0].double(), v[:, a["mask_level"], 0].double(), *common)
            res32, res64 = {"mask": m32.numpy()}, {"mask": m64.numpy()}
            for var in c["targets"]:
                t = torch.from_numpy(inp[var])
                assert y[KEYS[var]].shape == t.shape and y[KEYS[var]].dtype == torch.float32
                for l in range(c["L"]):      # the levels that are not filtered come back untouched
                    assert l in lv or torch.equal(y[KEYS[var]][:, l], t[:, l]), (name, var, l)
                res32[var] = y[KEYS[var]][:, lv, 0].contiguous().numpy()
                res64[var] = torch.stack([RW._blend_smoothed(t[:, l].double(), g64, m64, a["preserve_amplitude"])[:, 0] for l in lv], dim=1).numpy()
        fix, f64, d_ref = {}, {}, {}
        for k in ("U", "V", "T"):
            fix[f"sha256:{k}"] = np.array(input_digest(inp[k]))
        fix["levels"] = np.array(lv, np.int32)
        for o in output_names(name):
            a32, a64 = res32[o], res64[o]
            assert a32.dtype == np.float32 and a64.dtype == np.float64 and np.isfinite(a32).all() and np.isfinite(a64).all(), (name, o)
            fix[f"f32:{o}"] = a32
            f64[f"d64:{o}"] = (a64 - a32.astype(np.float64)).astype(np.float32)
            d_ref[o] = distance(a32, a64) if np.abs(a64).max() > 0 else 0.0
            fix[f"d_ref:{o}"] = np.float64(d_ref[o])
        if name == "calm":
            assert not res32["mask"].any() and all(np.array_equal(res32[v], inp[v][:, lv, 0]) for v in c["targets"])
        else:       # the fp32 and the fp64 side flag the same points
            assert np.array_equal(res32["mask"] > 0, res64["mask"] > 0), name
        np.savez_compressed(os.path.join(GOLD, f"wind_{name}.npz"), **fix)
        np.savez_compressed(os.path.join(GOLD, f"wind_{name}_f64.npz"), **f64)
        sizes = [os.path.getsize(os.path.join(GOLD, f"wind_{name}{s}.npz")) for s in ("", "_f64")]
        assert max(sizes) < 1000000, (name, sizes)
        print(f"[golden] wind {name}: {c['B']} x {c['L']} x {c['H']} x {c['W']}, mask > 0.5 on {100 * float((res32['mask'] > 0.5).mean()):.1f} %, "
              f"files {sizes[0] // 1024} + {sizes[1] // 1024} KB, d_ref " + ", ".join(f"{k} {v:.2e}" for k, v in d_ref.items()))


def advect_golden():
    """Semi-Lagrangian advection: the reference's SemiLagrangianAdvectionPost (credit/postblock/advect.py) run unmodified on float32
    and on double tensors, on every case of tests/advect_cases.py.  The class reads its coefficients and coordinates through xarray,
    which is absent: the stand-in `xarray` module of diag_golden serves the case's arrays, and `get_meta_file_path` is the identity.
    Written per case: advect_<case>.npz (SHA-256 of every regenerated input, the fp32 tracers, d_ref = the reference's own
    fp32-against-fp64 distance per tracer AND row region) and advect_<case>_f64.npz (the fp64 tracers as float32 differences from the
    fp32 ones).  The generator refuses to write a fixture that misses one of the conditions the cases are there for; the departure
    points it looks at are those of tests/advect_oracle.py in fp64, whose tracers it first checks against the reference's."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import advect_oracle as AO
    from advect_cases import (ADVECT_CASES, KEYS, REGIONS, SRC, block_args, case_inputs, input_digest, input_names, oracle_args,
                              region_distance, region_rows)
    coef = {}
    standin = oracle_stub.serve_xarray(coef)
    import credit.postblock.advect as RA
    RA.xr = standin
    RA.get_meta_file_path = lambda path: path

    for name, c in ADVECT_CASES.items():
        inp = case_inputs(name)
        a = block_args(name)
        coef.update(a_half=a.pop("model_a_half"), b_half=a.pop("model_b_half"), latitude=a.pop("latitude"), longitude=a.pop("longitude"))
        blk = RA.SemiLagrangianAdvectionPost(**a)
        res = {}
        for dtype in (torch.float32, torch.float64):
            batch = {"y_processed": {SRC: {KEYS[k]: torch.from_numpy(inp[k]).to(dtype) for k in inp}}}
            with torch.no_grad():
                y = blk(batch)["y_processed"][SRC]
            res[dtype] = {t: y[KEYS[t]].contiguous().numpy() for t in c["tracers"]}
            assert all(v.dtype == (np.float32 if dtype == torch.float32 else np.float64) and v.shape == inp[t].shape
                       for t, v in res[dtype].items()), name
        rows = region_rows(c["H"])
        fix, f64, d_ref = {}, {}, {}
        for k in input_names(name):
            fix[f"sha256:{k}"] = np.array(input_digest(inp[k]))
        for t in c["tracers"]:
            a32, a64 = res[torch.float32][t], res[torch.float64][t]
            assert np.isfinite(a32).all() and np.isfinite(a64).all(), (name, t)
            fix[f"f32:{t}"] = a32
            f64[f"d64:{t}"] = (a64 - a32.astype(np.float64)).astype(np.float32)
            for r in REGIONS:
                d_ref[(t, r)] = region_distance(a32, a64, rows[r])
                fix[f"d_ref:{t}:{r}"] = np.float64(d_ref[(t, r)])
        # ---- what the cases are there for (fp64)
        oa = oracle_args(name)
        o64, dep = AO.advect({KEYS[k]: torch.from_numpy(inp[k]) for k in inp}, dtype=torch.float64, want_departure=True, **oa)
        for t in c["tracers"]:
            assert np.abs(o64[KEYS[t]].numpy() - res[torch.float64][t]).max() <= 1e-9 * np.abs(res[torch.float64][t]).max(), (name, t)
        col, row, lev = (x.numpy() for x in dep)       # [B, L, H, W], levels top -> surface
        L, H, W = c["L"], c["H"], c["W"]
        ri = rows["interior"]
        disp = (np.abs(col - np.arange(W).reshape(1, 1, 1, W))[:, :, ri].max(), np.abs(row - np.arange(H).reshape(1, 1, H, 1))[:, :, ri].max(),
                np.abs(lev - np.arange(L).reshape(1, L, 1, 1))[:, :, ri].max())
        wraps = bool(((col[:, :, ri] < 0) | (col[:, :, ri] >= W)).any())
        clamped = (bool(((row < 0) | (row > H - 1)).any()), bool(((lev < 0) | (lev > L - 1)).any()))
        moved = {t: float(np.abs(res[torch.float64][t] - inp[t]).max() / np.abs(inp[t]).max()) for t in c["tracers"]}
        np.savez_compressed(os.path.join(GOLD, f"advect_{name}.npz"), **fix)
        np.savez_compressed(os.path.join(GOLD, f"advect_{name}_f64.npz"), **f64)
        sizes = [os.path.getsize(os.path.join(GOLD, f"advect_{name}{s}.npz")) for s in ("", "_f64")]
        print(f"[golden] advect {name}: {c['B']} x {L} x {H} x {W}, files {sizes[0] // 1024} + {sizes[1] // 1024} KB; interior displacement "
              f"{disp[0]:.2f} columns, {disp[1]:.2f} rows, {disp[2]:.2f} levels; wrap {wraps}; clamped rows {clamped[0]}, levels {clamped[1]}; moved "
              + ", ".join(f"{t} {m:.2f}" for t, m in moved.items()) + "; d_ref "
              + ", ".join(f"{t} {r} {d:.2e}" for (t, r), d in d_ref.items()), flush=True)
        assert all(d_ref[(t, "interior")] <= 1e-5 for t in c["tracers"]), name
        assert name == "polewind" or all(d_ref[(t, "edge")] <= 2e-4 for t in c["tracers"]), name
        assert wraps or name == "omega", name
        assert disp[0] >= 3.0 and disp[1] >= 0.5 and disp[2] >= 0.3, (name, disp)
        assert all(clamped), (name, clamped)
        assert all(m >= 0.1 for m in moved.values()), (name, moved)
        assert max(sizes) < 133000, (name, sizes)


def hybrid_golden():
    """Hybrid-level interpolation: the reference's HybridLevelInterpPost (credit/postblock/hybrid_interp.py) run unmodified on float32
    and on double tensors, on every case of tests/hybrid_cases.py.  The class reads its coefficients through xarray, which is absent:
    the stand-in `xarray` module serves the case's arrays to credit.postblock._interp_utils, and `get_meta_file_path` is the identity.
    Written per case: hybrid_<case>.npz (SHA-256 of every regenerated input, the fp32 outputs, d_ref = the reference's own
    fp32-against-fp64 distance per variable) and hybrid_<case>_f64.npz (the fp64 outputs as float32 differences from the fp32 ones).
    The generator refuses to write a fixture that misses one of the conditions its case is there for (hybrid_cases.check_conditions)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from hybrid_cases import HYBRID_CASES, KEYS, SRC, case_inputs, check_conditions, distance, input_digest, reference_args, variables
    coef = {}
    standin = oracle_stub.serve_xarray(coef)
    import credit.postblock._interp_utils as RU
    import credit.postblock.hybrid_interp as RH
    RU.xr = standin
    RU.get_meta_file_path = lambda path: path

    for name, c in HYBRID_CASES.items():
        inp = case_inputs(name)
        summary = check_conditions(name, inp)
        kw, arrays = reference_args(name)
        coef.clear()
        coef.update(arrays)
        blk = RH.HybridLevelInterpPost(**kw)
        res = {}
        for dtype in (torch.float32, torch.float64):
            batch = {"y_processed": {SRC: {KEYS[k]: torch.from_numpy(inp[k]).to(dtype) for k in inp}}}
            with torch.no_grad():
                y = blk(batch)["y_processed"][SRC]
            res[dtype] = {v: y[KEYS[v]].contiguous().numpy() for v in variables(name)}
            n_dst = blk.engine.dest_a.shape[0]
            assert all(o.dtype == (np.float32 if dtype == torch.float32 else np.float64)
                       and o.shape == (c["B"], n_dst, c["T"]) + inp["sp"].shape[3:] for o in res[dtype].values()), name
        fix, f64, d_ref = {}, {}, {}
        for k in inp:
            fix[f"sha256:{k}"] = np.array(input_digest(inp[k]))
        for v in variables(name):
            a32, a64 = res[torch.float32][v], res[torch.float64][v]
            assert np.isfinite(a32).all() and np.isfinite(a64).all(), (name, v)
            fix[f"f32:{v}"] = a32
            f64[f"d64:{v}"] = (a64 - a32.astype(np.float64)).astype(np.float32)
            d_ref[v] = distance(a32, a64)
            fix[f"d_ref:{v}"] = np.float64(d_ref[v])
        np.savez_compressed(os.path.join(GOLD, f"hybrid_{name}.npz"), **fix)
        np.savez_compressed(os.path.join(GOLD, f"hybrid_{name}_f64.npz"), **f64)
        sizes = [os.path.getsize(os.path.join(GOLD, f"hybrid_{name}{s}.npz")) for s in ("", "_f64")]
        assert max(sizes) < 1000000, (name, sizes)
        print(f"[golden] hybrid {name}: {summary}; files {sizes[0] // 1024} + {sizes[1] // 1024} KB; d_ref "
              + ", ".join(f"{k} {v:.2e}" for k, v in d_ref.items()), flush=True)


def regrid_reference(standin_args, name, run, curvilinear=False):
    """The reference's Regridder (credit/preblock/regrid.py) for a run of a case of tests/regrid_cases.py, reading the case's arrays
    through the stand-in dataset."""
    from regrid_cases import reference_args
    import credit.preblock.regrid as RR
    arrays, sizes = standin_args
    kw, arr, sz = reference_args(name, run, curvilinear)
    arrays.clear(), arrays.update(arr), sizes.clear(), sizes.update(sz)
    return RR.Regridder(**kw)


def regrid_golden():
    """Horizontal regridding: the reference's Regridder run unmodified on every case, variable and run of tests/regrid_cases.py.  The
    class reads its weights through xarray, which is absent: a stand-in module serves the case's arrays, sizes and `name in ds`.  The
    float64 truth is the SAME instance with its `weights` buffer converted to double and its cached matrix cleared, on double inputs.
    Written per case: regrid_<case>.npz (SHA-256 of every regenerated input, the fp32 outputs per run and variable, the destination
    attributes) and regrid_<case>_f64.npz (the fp64 outputs).  The generator refuses to write a fixture that misses the condition its
    case is there for (regrid_cases.check_conditions), whose fp32 output misses the gate of the device tests (regrid_cases.bound), or
    whose fp64 output the restatement (tests/regrid_oracle.py) does not reproduce."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import regrid_oracle as RO
    from regrid_cases import REGRID_CASES, SRC, bound, case_inputs, check_conditions, input_digest, key_of, out_shape, run_input, variables, weights
    arrays, sizes = {}, {}
    standin = oracle_stub.serve_xarray_dataset(arrays, sizes)
    import credit.preblock.regrid as RR
    RR.xr = standin

    for name, c in REGRID_CASES.items():
        inp = case_inputs(name)
        summary = check_conditions(name, inp)
        w = weights(name)
        fix, f64 = {f"sha256:{v}": np.array(input_digest(inp[v])) for v in inp}, {}
        worst = 0.0
        for run in c["runs"]:
            blk = regrid_reference((arrays, sizes), name, run)
            res = {}
            for dtype in (torch.float32, torch.float64):
                if dtype == torch.float64:
                    blk.weights = blk.weights.double()
                    blk._W = None
                batch = {"input": {SRC: {key_of(v): torch.from_numpy(run_input(name, run, inp[v])).to(dtype) for v in inp}}}
                with torch.no_grad():
                    y = blk(batch)["input"][SRC]
                res[dtype] = {v: y[key_of(v)].contiguous().numpy() for v in inp}
            shape = RO.dst_shape(w["dst_grid_dims"], w["xc_b"], w["yc_b"], c.get("reshape_to_xy", True))
            assert (None if blk.dst_shape is None else tuple(int(s) for s in blk.dst_shape)) == shape, name
            for v in variables(name):
                a32, a64 = res[torch.float32][v], res[torch.float64][v]
                assert a32.dtype == np.float32 and a64.dtype == np.float64 and a32.shape == a64.shape == out_shape(name, c["vars"][v]), (name, v)
                mine, mag, k = RO.regrid(run_input(name, run, inp[v]), w["row"], w["col"], w["S"], w["n_a"], w["n_b"],
                                         shape if c.get("reshape_to_xy", True) else None, c["runs"][run]["flip_axis"])
                bad = np.isnan(a64)
                assert np.array_equal(bad, np.isnan(mine)) and np.array_equal(bad, np.isnan(a32)) and bad.any() == bool(c.get("nan")), (name, v)
                mag2 = mag.reshape(-1, w["n_b"])
                scale = np.where(np.isnan(mag2), 0.0, mag2)
                assert (np.abs(np.where(bad, 0.0, mine - a64)).reshape(-1, w["n_b"]) <= 1e-14 * scale).all(), (name, run, v)
                err = np.abs(np.where(bad, 0.0, a32.astype(np.float64) - a64)).reshape(-1, w["n_b"])
                gate = np.where(np.isnan(mag2), 0.0, bound(k, mag2))
                assert (err <= gate).all(), (name, run, v, "the reference's own float32 output misses the gate")
                worst = max(worst, float((err[gate > 0] / gate[gate > 0]).max()))
                if name == "ragged":
                    assert (a32.reshape(-1, w["n_b"])[:, k == 0] == 0).all() and (k == 0).sum() == 2
                fix[f"f32:{run}:{v}"] = a32
                f64[f"f64:{run}:{v}"] = a64
        for tag, curv in (("rect", False), ("curv", True)) if name == "uniq" else (("rect", False),):
            blk = regrid_reference((arrays, sizes), name, "plain", curv)
            if curv:
                batch = {"input": {SRC: {key_of(v): torch.from_numpy(inp[v]) for v in inp}}}
                assert all(np.array_equal(blk(batch)["input"][SRC][key_of(v)].numpy(), fix[f"f32:plain:{v}"]) for v in inp)
            fix[f"grid_type:{tag}"] = np.array(str(blk.dst_grid_type))
            if blk.dst_grid_type is not None:
                fix[f"dst_lat:{tag}"], fix[f"dst_lon:{tag}"] = np.asarray(blk.dst_lat), np.asarray(blk.dst_lon)
        if name == "uniq":
            assert str(fix["grid_type:rect"]) == "rectilinear" and str(fix["grid_type:curv"]) == "curvilinear"
        np.savez_compressed(os.path.join(GOLD, f"regrid_{name}.npz"), **fix)
        np.savez_compressed(os.path.join(GOLD, f"regrid_{name}_f64.npz"), **f64)
        sizes_kb = [os.path.getsize(os.path.join(GOLD, f"regrid_{name}{s}.npz")) for s in ("", "_f64")]
        assert max(sizes_kb) < 1000000, (name, sizes_kb)
        print(f"[golden] regrid {name}: {summary}; files {sizes_kb[0] // 1024} + {sizes_kb[1] // 1024} KB; the reference's fp32 output "
              f"at {worst:.2f} of the gate", flush=True)


def metrics_reference(case, inp):
    """The reference's BaseCombinedMetric for a case of tests/metrics_cases.py: the class runs unmodified; the two loaders that read
    files (the scaler's variances, the grid's latitude) serve the case's arrays."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import metrics_cases as MC
    import metrics_oracle as MO
    import credit.metrics.base as RB
    kw, variances = MC.reference_args(case, inp)
    RB._load_target_variances = lambda path: dict(variances)
    RB._cos_lat_weights = lambda path: MO.lat_weights(inp["lat"])
    return RB.BaseCombinedMetric(**kw)


def metrics_hooks_f64(ref, full64):
    """The reference's own per-variable hooks called on DOUBLE tensors (its forward casts to float32): _score_variable for the
    plain metrics, the anomaly lines of _AnomalyMetricBase.forward (anomaly.py:269-291) and _score_anomaly for acc and activity.
    To be called right after ref(full) of the same call, so that the online climatology is the one of that call."""
    pred = {k: v for s in full64["y_processed"].values() for k, v in s.items()}
    target = {k: v for s in full64["y_target_processed"].values() for k, v in s.items()}
    out = {}
    with torch.no_grad():
        for name, mod in ref.metric_modules.items():
            for k in mod.var_keys:
                p, t = pred[k], target[k]
                if hasattr(mod, "_score_anomaly"):
                    clim = mod._get_clim(k, p)
                    if clim is None:
                        clim = t.mean(dim=0, keepdim=True)
                    clim = clim.to(p.device, p.dtype).expand_as(p)
                    lat_w = mod._lat_w(p)
                    w = lat_w if lat_w is not None else 1.0
                    d_f = (p - clim) - (w * (p - clim)).mean()
                    d_t = (t - clim) - (w * (t - clim)).mean()
                    out[f"{name}/{k}"] = mod._score_anomaly(d_f, d_t, w).item()
                else:
                    out[f"{name}/{k}"] = mod._score_variable(p, t, var_key=k).item()
    return out


def metrics_golden():
    """Verification metrics: the reference's BaseCombinedMetric forward (float32) on every case of tests/metrics_cases.py, and the
    float64 restatement of tests/metrics_oracle.py cross-checked against the reference's _score_variable / _score_anomaly hooks on
    double tensors.  Written per case: metrics_<case>.npz with the SHA-256 of every regenerated input, the keys of the returned dict
    and per call the fp32 values, the fp64 values, d_ref (the reference's fp32-against-fp64 distance) and the scale of the distance.
    The sp2d fixture is refused unless a float32 raw-moment evaluation of r2score, log_variance_ratio and acc misses the gate on the
    pressure variable with sequential and with pairwise summation."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import metrics_cases as MC
    import metrics_oracle as MO
    for case, c in MC.METRICS_CASES.items():
        inp = MC.case_inputs(c["inputs"])
        ref = metrics_reference(case, inp)
        mine = MO.Restatement(dtype=torch.float64, **MC.block_args(case, inp))
        rows = {"f32": [], "f64": [], "d_ref": [], "scale": []}
        keys = None
        for call in range(MC.INPUTS[c["inputs"]]["calls"]):
            full = MC.state_dicts(inp, call, torch.from_numpy)
            full64 = MC.state_dicts(inp, call, lambda a: torch.from_numpy(a).double())
            with torch.no_grad():
                o32 = ref(full)
            hooks = metrics_hooks_f64(ref, full64)
            o64 = mine(full64, all_scores=True)
            assert list(o32) == list(o64), case
            keys = list(o32)
            for k, v in hooks.items():
                assert abs(v - o64[k]) <= 1e-10 * max(1.0, abs(v)), (case, call, k, v, o64[k])
            sc = MC.scales(mine.last_all_scores, mine.weights, mine.var_keys)
            assert all(np.isfinite(o32[k]) and np.isfinite(o64[k]) for k in keys), case
            rows["f32"].append([o32[k] for k in keys])
            rows["f64"].append([o64[k] for k in keys])
            rows["scale"].append([sc[k] for k in keys])
            rows["d_ref"].append([MC.distance(o32[k], o64[k], sc[k]) for k in keys])
            if case == "sp2d":
                key = MC.KEYS["sp"]
                p, t = inp["pred"][0]["sp"], inp["target"][0]["sp"]
                cl = np.broadcast_to(inp["clim"]["sp"], p.shape)
                w = np.broadcast_to(MO.lat_weights(inp["lat"]).numpy().reshape(1, 1, 1, -1, 1), p.shape)
                for pairwise in (False, True):
                    raw = MC.raw_moments(p, t, cl, w, pairwise)
                    for m, v in raw.items():
                        k = f"{m}/{key}"
                        bound = MC.gate(MC.distance(o32[k], o64[k], sc[k]))[1]
                        miss = MC.distance(v, o64[k], sc[k])
                        print(f"[golden] metrics sp2d raw moments ({'pairwise' if pairwise else 'sequential'}) {m}: {v!r} against "
                              f"{o64[k]!r}: distance {miss:.2e}, gate {bound:.2e}")
                        assert miss > bound, (m, pairwise, miss, bound)
        fix = {f"sha256:{k}": np.array(MC.input_digest(v)) for k, v in MC.flat_inputs(inp).items()}
        fix["keys"] = np.array(keys)
        fix.update({k: np.array(v, dtype=np.float64) for k, v in rows.items()})
        path = os.path.join(GOLD, f"metrics_{case}.npz")
        np.savez_compressed(path, **fix)
        d = fix["d_ref"]
        print(f"[golden] metrics {case}: {len(keys)} keys x {d.shape[0]} calls, {os.path.getsize(path) // 1024} KB; max d_ref {d.max():.2e}, "
              f"median {np.median(d):.2e}", flush=True)


def ensemble_reference(case, inp):
    """The reference's own classes on a case of tests/ens_cases.py, float32 forward: KCRPSLoss(biased=True / False) and
    AlmostFairKCRPSLoss(alpha) run unmodified on the [B * M, ...] layout.  -> {var name: {"crps" | "fair_crps" | "afcrps": map}}.
    credit/metrics/gen_1/metrics.py (LatWeightedMetricsEnsemble) and credit/applications/rollout_metrics_noisy_model.py
    (calculate_ensemble_metrics) do not import here (datetime.UTC; names credit.metrics no longer exports), and credit/ensemble/crps.py
    needs properscoring: those three are pinned through tests/ens_oracle.py, which restates metrics.py:304-313,
    rollout_metrics_noisy_model.py:107-135 and the identity of calculate_crps_per_channel with the plane mean of the biased CRPS."""
    import ens_cases as EC
    from credit.losses.gen_1.almost_fair_crps import AlmostFairKCRPSLoss
    from credit.losses.gen_1.kcrps import KCRPSLoss
    alpha = EC.ENS_CASES[case]["alpha"]
    out = {}
    with torch.no_grad():
        for name in inp["truth"]:
            y, x = torch.from_numpy(inp["truth"][name]), torch.from_numpy(EC.stacked(inp["members"][name]))
            out[name] = {"crps": KCRPSLoss("none", biased=True)(y, x), "fair_crps": KCRPSLoss("none", biased=False)(y, x),
                         # (its forward squeezes a single-level variable's level axis away: almost_fair_crps.py:23)
                         "afcrps": AlmostFairKCRPSLoss(alpha=alpha, reduction="none")(y, x).reshape(y.shape)}
            assert abs(AlmostFairKCRPSLoss(alpha=alpha, reduction="mean")(y, x).item() - out[name]["afcrps"].mean().item()) == 0.0
    return out


def ensemble_golden():
    """Ensemble verification: per case of tests/ens_cases.py the float32 forward (the reference's KCRPSLoss and AlmostFairKCRPSLoss
    live for the three CRPS maps and their means, the restatement of tests/ens_oracle.py in float32 for the rest) and the float64
    restatement.  Written per case: ens_<case>.npz with the SHA-256 of every regenerated input, the flat scalar keys, their fp32
    values, d_ref (the fp32-against-fp64 distance) and scale, and for the case's map variables the six fp32 maps with d_ref and
    scale; ens_<case>_f64.npz with the fp64 scalars and each map's fp64 golden as its float32 difference from the fp32 one."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ens_cases as EC
    import ens_oracle as EO
    for case, c in EC.ENS_CASES.items():
        inp = EC.case_inputs(case)
        live = ensemble_reference(case, inp)
        w = EO.lat_weights(inp["lat"]) if c["lat"] else None
        members = {EC.KEYS[n]: torch.from_numpy(v) for n, v in inp["members"].items()}
        truth = {EC.KEYS[n]: torch.from_numpy(v) for n, v in inp["truth"].items()}
        r32, m32 = EO.restate(members, truth, c["alpha"], w, torch.float32)
        r64, m64 = EO.restate(members, truth, c["alpha"], w, torch.float64)
        wt32 = 1.0 if w is None else w.reshape(1, 1, 1, -1, 1)
        for n, lv in live.items():          # the live classes replace the restatement wherever they speak
            k = EC.KEYS[n]
            for m, ref_map in lv.items():
                scale = m64[m][k].abs().mean().item()
                assert EC.map_distance(m32[m][k], ref_map, scale) <= 1e-6, (case, n, m)
                m32[m][k] = ref_map
                r32[f"{m}/{k}"] = (ref_map * wt32).mean().item()
            r32[f"crps_per_channel/{k}"] = (lv["crps"] * wt32).mean(dim=[0, 2, 3, 4]).numpy().astype(np.float64)
            y64, x64 = torch.from_numpy(inp["truth"][n]).double(), torch.from_numpy(EC.stacked(inp["members"][n])).double()
            from credit.losses.gen_1.kcrps import KCRPSLoss
            for m, biased in (("crps", True), ("fair_crps", False)):      # the reference's class on double tensors against the fp64 restatement
                d = (KCRPSLoss("none", biased=biased)(y64, x64) - m64[m][k]).abs().max().item()
                assert d <= 1e-11 * max(1.0, m64[m][k].abs().max().item()), (case, n, m, d)
        f32, f64 = EC.flat_scalars(r32), EC.flat_scalars(r64)
        keys = EC.scalar_keys(case)
        assert list(f32) == keys == list(f64), case
        scale = [abs(f64[k]) for k in keys]
        fix = {f"sha256:{k}": np.array(EC.input_digest(v)) for k, v in EC.flat_inputs(inp).items()}
        fix.update(keys=np.array(keys), f32=np.array([f32[k] for k in keys], dtype=np.float64), scale=np.array(scale, dtype=np.float64),
                   d_ref=np.array([EC.distance(f32[k], f64[k], sc) for k, sc in zip(keys, scale)], dtype=np.float64),
                   moved=np.array([inp["moved"][n] for n in c["vars"]]))
        fix64 = {"f64": np.array([f64[k] for k in keys], dtype=np.float64)}
        worst_map = 0.0
        for n in c["map_vars"]:
            k = EC.KEYS[n]
            for m in EC.MAPS:
                a32, a64 = m32[m][k].numpy().astype(np.float32), m64[m][k].numpy()
                sc = float(np.abs(m64["ens_abs_err"][k].numpy()).mean()) if m == "ens_mean" else float(np.abs(a64).mean())
                fix[f"map32:{m}:{n}"] = a32
                fix[f"map_scale:{m}:{n}"] = np.array(sc)
                fix[f"map_d_ref:{m}:{n}"] = np.array(EC.map_distance(a32, a64, sc))
                fix64[f"d64:{m}:{n}"] = (a64 - a32.astype(np.float64)).astype(np.float32)
                worst_map = max(worst_map, float(fix[f"map_d_ref:{m}:{n}"]))
        paths = [os.path.join(GOLD, f"ens_{case}.npz"), os.path.join(GOLD, f"ens_{case}_f64.npz")]
        np.savez_compressed(paths[0], **fix)
        np.savez_compressed(paths[1], **fix64)
        sizes = [os.path.getsize(p) for p in paths]
        assert max(sizes) < 1_000_000, (case, sizes)
        print(f"[golden] ensemble {case}: {len(keys)} scalars, {len(c['map_vars']) * len(EC.MAPS)} maps, files {sizes[0] // 1024} + "
              f"{sizes[1] // 1024} KB; moved apart {dict(inp['moved'])}; max scalar d_ref {fix['d_ref'].max():.2e}, max map d_ref "
              f"{worst_map:.2e}", flush=True)
        if case == "m3":
            k = EC.KEYS["sp"]
            print("[golden] ensemble m3 surface pressure d_ref: " + ", ".join(
                f"{m} {float(fix[f'map_d_ref:{m}:sp']):.2e}" for m in EC.MAPS), flush=True)


def xform_golden():
    """Variable transforms: the reference's own FillValues / LogTransform / SqrtTransform (credit/preblock/{fill_values,log,sqrt}.py)
    and ExpTransform / SquareTransform (credit/postblock/{exp,square}.py) run unmodified, stacked as the cases of tests/xform_cases.py
    say, in fp32 and in fp64.  The scaler legs between them are NOT the reference's class: bridgescaler is not installed, so
    bridgescaler_transform cannot be run; they are the expressions already pinned for DevicePreblock and InverseScale,
    (t - mean) / std.clamp(min=1e-12) (credit/preblock/norm.py:98) and t * std + mean, with float32 statistics.  Written per case:
    xform_<case>.npz (SHA-256 of every regenerated input, the fp32 outputs "f32:pre:<var>" / "f32:post:<var>" and d_ref = the
    reference's own fp32-against-fp64 distance per variable AND level, NaN positions excluded) and xform_<case>_f64.npz (the fp64
    outputs as float32 differences from the fp32 ones).  Refused: a level with 1 % NaN or more, a designated NaN case without one,
    NaN positions that differ between the two precisions."""
    import types
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from credit.postblock.exp import ExpTransform
    from credit.postblock.square import SquareTransform
    from credit.preblock.fill_values import FillValues
    from credit.preblock.log import LogTransform
    from credit.preblock.sqrt import SqrtTransform
    from xform_cases import (SRC, XFORM_CASES, batch_input, case_inputs, case_stats, input_digest, level_distance, out_variables, post_blocks,
                             pre_blocks, target_channel_map)
    ref = types.SimpleNamespace(FillValues=FillValues, LogTransform=LogTransform, SqrtTransform=SqrtTransform, ExpTransform=ExpTransform,
                                SquareTransform=SquareTransform)
    for name, c in XFORM_CASES.items():
        fields, y_pred = case_inputs(name)
        mean, std = case_stats(name)
        res = {}
        for dtype in (torch.float32, torch.float64):
            st = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dtype).reshape(1, -1, 1, 1, 1)   # noqa: E731
            batch = {"input": batch_input(name, fields, lambda a: torch.from_numpy(a).to(dtype))}
            with torch.no_grad():
                for blk in pre_blocks(name, ref):
                    batch = blk(batch)
                out = {}
                for v in c["variables"]:
                    t = batch["input"][SRC][v["key"]]
                    if v["name"] in mean:
                        t = (t - st(mean[v["name"]])) / st(std[v["name"]]).clamp(min=1e-12)
                    out[f"pre:{v['name']}"] = t
                y = torch.from_numpy(y_pred).to(dtype).flatten(1, 2)
                nested = {SRC: {}}
                for key, info in target_channel_map(name).items():
                    t = y[:, info["slice"]].unflatten(1, info["orig_shape"])
                    n = key.split("/")[-1]
                    nested[SRC][key] = t * st(std[n]) + st(mean[n]) if n in mean else t
                full = {"y_processed": nested}
                for blk in post_blocks(name, ref):
                    full = blk(full)
                for v in out_variables(name):
                    out[f"post:{v['name']}"] = full["y_processed"][SRC][v["key"]]
            assert all(t.dtype == dtype for t in out.values()), name
            res[dtype] = {k: t.contiguous().numpy() for k, t in out.items()}
        fix, f64, n_nan, worst = {}, {}, 0, 0.0
        for v in c["variables"]:
            fix[f"sha256:in:{v['name']}"] = np.array(input_digest(fields[v["key"]]))
        fix["sha256:y_pred"] = np.array(input_digest(y_pred))
        for k in res[torch.float32]:
            a32, a64 = res[torch.float32][k], res[torch.float64][k]
            share = np.isnan(a32).mean(axis=(0, 2, 3, 4))
            assert share.max() < 0.01, (name, k, share)
            n_nan += int(np.isnan(a32).sum())
            d = level_distance(a32, a64)
            assert np.isfinite(d).all(), f"{name} {k}: NaN positions differ between fp32 and fp64"
            fix[f"f32:{k}"] = a32
            f64[f"d64:{k}"] = np.nan_to_num(a64 - a32.astype(np.float64), nan=0.0).astype(np.float32)
            fix[f"d_ref:{k}"] = d
            worst = max(worst, d.max())
        assert (n_nan > 0) == c["nan_case"], (name, n_nan)
        np.savez_compressed(os.path.join(GOLD, f"xform_{name}.npz"), **fix)
        np.savez_compressed(os.path.join(GOLD, f"xform_{name}_f64.npz"), **f64)
        sizes = [os.path.getsize(os.path.join(GOLD, f"xform_{name}{s}.npz")) for s in ("", "_f64")]
        assert max(sizes) < 1000000, (name, sizes)
        print(f"[golden] xform {name}: {len(res[torch.float32])} outputs, {n_nan} NaN, files {sizes[0] // 1024} + {sizes[1] // 1024} KB, worst d_ref {worst:.2e}")


def reconstruct_golden():
    """Reconstruct -> FlattenToTensor of the reference (no scaler) on a synthetic y_pred + channel map."""
    from credit.postblock.reconstruct import FlattenToTensor, Reconstruct
    g = np.random.Generator(np.random.Philox(key=[41, 1]))
    B, H, W = 2, 9, 14
    y = torch.from_numpy(g.standard_normal((B, 11, 1, H, W)).astype(np.float32))
    cmap = {"era5/prognostic/3d/T": {"slice": slice(0, 4), "orig_shape": (4, 1)},
            "era5/prognostic/3d/Q": {"slice": slice(4, 8), "orig_shape": (4, 1)},
            "era5/prognostic/2d/SP": {"slice": slice(8, 9), "orig_shape": (1, 1)},
            "era5/diagnostic/2d/tp": {"slice": slice(9, 10), "orig_shape": (1, 1)},
            "era5/diagnostic/2d/evap": {"slice": slice(10, 11), "orig_shape": (1, 1)}}
    bd = {"y_pred": y.clone(), "metadata": {"target": {"_channel_map": cmap}}}
    bd = Reconstruct()(bd)
    out = {"y": y.numpy()}
    for k, v in bd["y_processed"]["era5"].items():
        out["rec:" + k] = v.numpy()
    bd["y_processed"]["era5"]["era5/prognostic/2d/SP"] = bd["y_processed"]["era5"]["era5/prognostic/2d/SP"] * 2.0
    bd = FlattenToTensor()(bd)
    out["flat"] = bd["y_pred"].numpy()
    np.savez_compressed(os.path.join(GOLD, "reconstruct.npz"), **out)
    print("[golden] reconstruct / flatten:", tuple(bd["y_pred"].shape))


def assemble_golden():
    """assemble_rollout_batch of the reference (rollout_utils.py:322-430): which tensor object each key is routed to."""
    from credit.trainers.rollout_utils import assemble_rollout_batch
    def t(v):
        return torch.full((1, 1, 1, 2, 2), float(v))
    keys_ic = ["era5/prognostic/3d/T", "era5/prognostic/2d/SP", "era5/static/2d/LSM", "era5/dynamic_forcing/2d/tsi",
               "era5/dynamic_forcing/2d/sza", "era5/diagnostic/2d/tp"]
    ic = {"input": {"era5": {k: t(100 + i) for i, k in enumerate(keys_ic)}, "empty": {}}}
    pred = {"era5": {"era5/prognostic/3d/T": t(200), "era5/prognostic/2d/SP": t(201), "era5/diagnostic/2d/tp": t(202)}}
    cur = {"input": {"era5": {"era5/dynamic_forcing/2d/tsi": t(300)}}, "target": None}   # sza missing -> carried forward
    out = assemble_rollout_batch({"y_processed": pred, "ic_preprocessed": ic}, cur, 1)
    res = {"keys": np.array(list(out["input"]["era5"].keys())), "vals": np.array([float(v.flatten()[0]) for v in out["input"]["era5"].values()]),
           "sources": np.array(list(out["input"].keys()))}
    np.savez_compressed(os.path.join(GOLD, "assemble_rollout.npz"), **res)
    print("[golden] assemble_rollout_batch:", dict(zip(res["keys"], res["vals"])))



def gen2loop_golden():
    """The COMPOSED gen-2 loop: the reference's own `run_forecast` (credit/trainers/rollout_utils.py:204-319) driven for three steps on T0
    -- its `apply_preblocks` over the reference's ERA5Normalizer (statistics injected: xarray is absent) + ConcatToTensor (with a
    ChannelSchema, so the diagnostics reach the target channel map as at inference), the reference CrossFormer, its `apply_postblocks`
    over the reference's Reconstruct and an inverse scaler, its `assemble_rollout_batch` between steps.  The inverse scaler is the one
    block that is not reference code (the reference's is a bridgescaler wrapper; bridgescaler is not installable here): y * std + mean
    per variable, written here as a BasePostblock.  Stored: every y_processed variable of every step (stride 2 in both map axes)."""
    import credit.trainers.rollout_utils as RU
    from credit.datasets.gen_2.channel_utils import ChannelSchema
    from credit.postblock.base import BasePostblock
    from credit.postblock.reconstruct import Reconstruct
    from credit.preblock.concat import ConcatToTensor
    from credit.preblock.norm import ERA5Normalizer
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from synth_batches import gen2loop_batches, gen2loop_schema
    cfg = named_config("T0")
    n_steps = 3
    ic, frcs, mean, std = gen2loop_batches(cfg, n_steps)
    inp, out = gen2loop_schema(cfg)

    norm = ERA5Normalizer.__new__(ERA5Normalizer)
    torch.nn.Module.__init__(norm)
    norm._mean = {k: torch.tensor(np.array(v), dtype=torch.float32) for k, v in mean.items()}
    norm._std = {k: torch.tensor(np.array(v), dtype=torch.float32) for k, v in std.items()}
    concat = ConcatToTensor()
    concat.set_schema(ChannelSchema([{"var_key": k, "n_levels": nl, "n_time": 1} for k, nl in inp],
                                    [{"var_key": k, "n_levels": nl, "n_time": 1} for k, nl in out]))

    class InverseScale(BasePostblock):
        def forward(self, batch_dict):
            for src, variables in batch_dict["y_processed"].items():
                for key in list(variables):
                    name = key.split("/")[-1]
                    if name in mean:
                        variables[key] = variables[key] * torch.as_tensor(std[name]).reshape(1, -1, 1, 1, 1) + torch.as_tensor(mean[name]).reshape(1, -1, 1, 1, 1)
            return batch_dict
    step_pre = torch.nn.ModuleDict({"norm": norm, "concat": concat})
    step_post = torch.nn.ModuleDict({"reconstruct": Reconstruct(), "inverse_scaler": InverseScale()})
    model = reference_model(cfg)
    t0 = np.datetime64("2020-01-01T00").astype("datetime64[ns]").astype(np.int64)
    ic_batch = {"input": ic["input"], "metadata": {"era5": {"input_datetime": torch.tensor([int(t0)])}}}
    RU.decode_time = lambda ns, calendar="standard": __import__("pandas").Timestamp(int(ns))   # cftime is absent; the standard calendar is plain pandas
    got = []

    def save(y_processed, init_time, step, fhr_per_step, save_dir, pool):
        got.append({k: v.clone() for k, v in y_processed["era5"].items()})
    conf = {"data": {"timestep": "6h", "history_len": 1}}
    RU.run_forecast(conf, n_steps, "unused", torch.nn.ModuleDict(), step_pre, step_post, torch.nn.ModuleDict(), model,
                    iter([ic_batch] + frcs), torch.device("cpu"), None, save, verbose=False)
    assert len(got) == n_steps
    res = {"keys": np.array(list(got[0].keys()))}
    for s, d in enumerate(got):
        for k, v in d.items():
            res[f"step{s}:{k}"] = v.numpy()[..., ::2, ::2]
    np.savez_compressed(os.path.join(GOLD, "gen2_loop_T0.npz"), **res)
    print(f"[golden] gen-2 composed loop (reference run_forecast, T0, {n_steps} steps): {len(got[0])} variables per step, "
          f"max |y| {max(float(v.abs().max()) for v in got[-1].values()):.3f}")


def fuxi_timm_golden():
    """BASELINE config 5's default stage variant is timm's SwinTransformerV2Stage, and timm is not installable in the build container:
    the engine's timm block follows timm's published source and is unpinned.  This entry pins it wherever `import timm` works: it builds
    the reference Fuxi (credit/models/fuxi.py) at the FT0 geometry with the real timm stage, loads the build's synthetic weights and
    writes tests/golden/fuxi_timm_FT{0,1,2}T.npz, which tests/test_fuxi.py picks up (and skips, loudly, while the files are absent)."""
    try:
        import timm  # noqa: F401
        if "MagicMock" in type(timm).__name__ or not hasattr(timm, "__version__") or not isinstance(timm.__version__, str):
            raise ImportError("timm is the oracle stub")
    except Exception as e:   # noqa: BLE001
        print(f"[golden] fuxi_timm: SKIPPED -- `import timm` does not give the real package here ({e}); run "
              "`python tools/make_goldens.py --only fuxi_timm` in an environment that has timm to pin BASELINE config 5's default stage")
        return
    from credit.models.fuxi import Fuxi
    from wxengine.fuxi import named_fuxi_config, synth_fuxi_state_dict
    from wxengine.synth import keyed_normal
    for name in ("FT0T", "FT1T", "FT2T"):   # tests/test_fuxi.py's three geometries with the reference's own stage
        cfg = named_fuxi_config(name)
        m = Fuxi(image_height=cfg.image_height, patch_height=cfg.patch_height, image_width=cfg.image_width, patch_width=cfg.patch_width,
                 levels=cfg.levels, frames=cfg.frames, frame_patch_size=cfg.frame_patch_size, dim=cfg.dim, num_groups=cfg.num_groups,
                 channels=cfg.channels, surface_channels=cfg.surface_channels, input_only_channels=cfg.input_only_channels,
                 output_only_channels=cfg.output_only_channels, num_heads=cfg.num_heads, depth=cfg.depth, window_size=cfg.window_size,
                 use_spectral_norm=cfg.use_spectral_norm, interp=cfg.interp)
        sd = synth_fuxi_state_dict(cfg)
        res = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        bad = [k for k in list(res.missing_keys) + list(res.unexpected_keys) if not k.endswith(("relative_position_index", "relative_coords_table", "attn_mask"))]
        assert not bad, f"{name}: the synthetic state dict and the reference module disagree on keys: {bad[:6]}"
        m.eval()   # built and loaded on the CPU, never moved or cast: the case FuxiConfig.timm_qkv_unnormalised = True describes
        x = torch.from_numpy(keyed_normal("fuxi/x0", (1, cfg.in_chans, cfg.frames, cfg.image_height, cfg.image_width), 1000))
        with torch.no_grad():
            y = m(x)
        np.savez_compressed(os.path.join(GOLD, f"fuxi_timm_{name}.npz"), y=y[0, :, 0].numpy().astype(np.float32), timm_version=np.array(timm.__version__))
        print(f"[golden] fuxi_timm {name}: y {tuple(y.shape)} mean|y| {float(y.abs().mean()):.4f} (timm {timm.__version__})")


SIGMA_A = np.array([200.0, 5000.0, 12000.0, 14000.0, 9000.0, 3000.0, 0.0], dtype=np.float32)       # Pa
SIGMA_B = np.array([0.0, 0.0, 0.08, 0.3, 0.6, 0.88, 1.0], dtype=np.float32)


def fixers_sigma_golden():
    """The same three fixers on a hybrid sigma-pressure grid (gen1.py sigma branches).  The reference reads its grid
    from `save_loc_physics` through xarray (absent here): `get_forward_data` is replaced by an in-memory stand-in that
    serves the arrays this script defines -- the fixer classes and physics_hybrid_sigma_level run unmodified."""
    import credit.postblock.gen1 as G
    x_np, y_np = fixer_inputs(seed=12)
    g = np.random.Generator(np.random.Philox(key=[12, 5]))
    H, W, L = 10, 18, 7
    sp_x = (1.0e5 + 2.0e3 * g.standard_normal((1, 2, H, W))).astype(np.float32)
    sp_y = (1.0e5 + 2.0e3 * g.standard_normal((1, H, W))).astype(np.float32)
    gph = (50.0 + 20.0 * g.standard_normal((H, W))).astype(np.float32)
    lat = np.array([90, 70, 50, 30, 10, -10, -30, -50, -70, -90], dtype=np.float64)
    lon = np.arange(0, 360, 20, dtype=np.float64)
    lon2d, lat2d = np.meshgrid(lon, lat)

    class _V:
        def __init__(self, a):
            self.values = a
    fake = {"lon2d": _V(lon2d), "lat2d": _V(lat2d), "coef_a": _V(SIGMA_A), "coef_b": _V(SIGMA_B), "gph": _V(gph)}
    G.get_forward_data = lambda _f: fake
    out = {"x": x_np, "y": y_np, "sp_x": sp_x, "sp_y": sp_y, "gph": gph, "coef_a": SIGMA_A, "coef_b": SIGMA_B}
    for midpoint in (False, True):
        nl = L - 1 if midpoint else L
        tag = "mid" if midpoint else "trapz"
        xs = np.concatenate([x_np[b * L:b * L + nl] for b in range(4)] + [sp_x], 0)            # [4 nl + 1, 2, H, W]
        ys = np.concatenate([y_np[b * L:b * L + nl] for b in range(4)] + [y_np[28:], sp_y], 0)  # [4 nl + 8 + 1, H, W]
        # SP sits at the same index in x and y (gen1.py:306-308): pad x with zero channels up to y's SP index
        sp_ind = 4 * nl + 8
        xs = np.concatenate([xs[:4 * nl], np.zeros((8, 2, H, W), np.float32), xs[4 * nl:]], 0)
        x = torch.from_numpy(xs)[None]
        y = torch.from_numpy(ys)[None, :, None]
        base = {"simple_demo": False, "denorm": False, "grid_type": "sigma", "midpoint": midpoint, "activate": True,
                "activate_outside_model": False, "lon_lat_level_name": ["lon2d", "lat2d", "coef_a", "coef_b"],
                "sp_inds": sp_ind}
        q0 = nl
        mass = dict(base, fix_level_num=3, q_inds=list(range(q0, q0 + nl)))
        data = {"lead_time_periods": 6, "save_loc_physics": "in-memory.nc"}
        conf_m = {"global_mass_fixer": mass, "data": data}
        conf_w = {"global_mass_fixer": mass, "data": data,
                  "global_water_fixer": dict(base, q_inds=list(range(q0, q0 + nl)), precip_ind=4 * nl + 6, evapor_ind=4 * nl + 7)}
        conf_e = {"global_mass_fixer": mass, "data": data,
                  "global_energy_fixer": dict(base, T_inds=list(range(0, nl)), q_inds=list(range(q0, q0 + nl)),
                                              U_inds=list(range(2 * nl, 3 * nl)), V_inds=list(range(3 * nl, 4 * nl)),
                                              TOA_rad_inds=[4 * nl, 4 * nl + 1], surf_rad_inds=[4 * nl + 2, 4 * nl + 3],
                                              surf_flux_inds=[4 * nl + 4, 4 * nl + 5], surface_geopotential_name=["gph"])}
        with torch.no_grad():
            ym = G.GlobalMassFixer(conf_m)({"y_pred": y.clone(), "x": x.clone()})["y_pred"]
            yw = G.GlobalWaterFixer(conf_w)({"y_pred": y.clone(), "x": x.clone()})["y_pred"]
            ye = G.GlobalEnergyFixer(conf_e)({"y_pred": y.clone(), "x": x.clone()})["y_pred"]
            yc = G.GlobalEnergyFixer(conf_e)(G.GlobalWaterFixer(conf_w)(G.GlobalMassFixer(conf_m)(
                {"y_pred": y.clone(), "x": x.clone()})))["y_pred"]
        for name, t in (("mass", ym), ("water", yw), ("energy", ye), ("chain", yc)):
            assert t.shape == y.shape, (name, t.shape)
            out[f"{tag}_{name}"] = t[0, :, 0].double().numpy()
        print(f"[golden] sigma fixers {tag}: mass dSP max {float((ym - y).abs().max()):.3e}  water dP max "
              f"{float((yw - y).abs().max()):.3e}  energy dT max {float((ye - y).abs().max()):.3e}")
    np.savez_compressed(os.path.join(GOLD, "fixers_sigma.npz"), **out)


def blocks_golden(stride=4):
    """T1 (T0's full maps are in model_T0.npz): every sub-module output (module-name depth <= 4, cube embedding aside) that
    oracle/wxformer_oracle.py also captures, as a stride-`stride` sample of each map plus full-map per-channel sums and max|.|, and
    the dynamic position bias of the first attention -> reference_blocks_T1.npz (tests/test_oracle_vs_reference.py)."""
    from oracle import wxformer_oracle as O
    cfg = named_config("T1")
    m = reference_model(cfg)
    x = torch.from_numpy(synth_input(cfg))
    caps = {}
    hooks = [mod.register_forward_hook(lambda _m, _i, o, n=n: caps.__setitem__(n, o.detach().clone()))
             for n, mod in m.named_modules() if n.count(".") <= 4 and n and not n.startswith("cube")]
    with torch.no_grad():
        m(x)
    for h in hooks:
        h.remove()
    mine = {}
    O.forward(cfg, synth_state_dict(cfg), x, capture=mine)
    out = {"stride": np.int64(stride)}
    for n, v in caps.items():
        if n in mine and tuple(mine[n].shape) == tuple(v.shape):
            v = v[0].double()
            out["cap/" + n] = v[:, ::stride, ::stride].numpy().astype(np.float32)
            out["ch_sum/" + n] = v.sum(dim=(1, 2)).numpy()
            out["ch_maxabs/" + n] = v.abs().amax(dim=(1, 2)).numpy()
    att = m.layers[0][1].layers[0][0]
    wsz = att.window_size
    pos = torch.arange(-wsz, wsz + 1)
    rel = torch.stack(torch.meshgrid(pos, pos, indexing="ij")).reshape(2, -1).t().float()
    with torch.no_grad():
        out["dpb/layers.0.1.layers.0.0.dpb"] = att.dpb(rel)[att.rel_pos_indices].numpy().astype(np.float32)
    out["dpb_window"] = np.int64(wsz)
    np.savez_compressed(os.path.join(GOLD, "reference_blocks_T1.npz"), **out)
    print(f"[golden] blocks T1: {len([k for k in out if k.startswith('cap/')])} module outputs, stride {stride}")


def state_specs_golden():
    """Parameter / buffer names and shapes of the reference class per config -> reference_state_specs.json (tests/test_abi_cpu.py)."""
    import json
    specs = {}
    for name in ("T0", "T1", "T0W", "T0U", "T0M", "T0F"):
        specs[name] = {k: list(v.shape) for k, v in reference_model(named_config(name)).state_dict().items()}
    with open(os.path.join(GOLD, "reference_state_specs.json"), "w") as f:   # one line per config
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(specs[n], sort_keys=True)}" for n in sorted(specs)) + "\n}\n")
    print(f"[golden] state specs of {sorted(specs)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="pad,T0,T1,blocks,specs,glue,swin,swinblock,fuxi,attend,rollC1,rollC3S,rollC3,T0M,layout,fixers,frames2,sigma,updown,pre,gen2,rec,asm,gen2loop,fuxi_timm,C1,C3S,C3,T0W,C1W,T0U,T0F,RT,stress")
    args = ap.parse_args()
    os.makedirs(GOLD, exist_ok=True)
    torch.set_num_threads(os.cpu_count() or 1)
    for item in args.only.split(","):
        if item == "pad":
            pad_golden()
        elif item == "glue":
            glue_golden()
        elif item == "swin":
            swin_golden()
        elif item == "swinblock":
            swin_block_golden()
        elif item == "fuxi":
            fuxi_golden()
        elif item.startswith("fuxi:"):   # named cases only, joined with "+"
            fuxi_golden(tuple(item[len("fuxi:"):].split("+")))
        elif item == "attend":
            attend_golden()
        elif item == "rollC1":      # BASELINE config 2: 24-step rollout on the 1-degree grid
            long_rollout_golden("C1", 24, 20)
        elif item == "rollC3S":     # 8 steps on the 0.25-degree grid (small-width model)
            long_rollout_golden("C3S", 8, 40, with_fp64=False)
        elif item == "rollC1stress":   # 8 steps of the 1-degree model on the "stress" weight family (logits +-40, pre-GELU 1e2)
            long_rollout_golden("C1", 8, 20, family="stress")
        elif item == "rollC3":      # BASELINE config 3 itself: its 40 steps of the FULL-width 124 M-parameter model on the 0.25-degree grid
            long_rollout_golden("C3", 40, 40, with_fp64=False, dense_steps=(1, 10, 20, 40), dense_stride=16)   # (rounds 2-4 stored 6 steps; ~30 min of CPU for 40; round 6: + stride-16 samples of four steps)
        elif item == "layout":
            layout_golden()
        elif item == "fixers":
            fixers_golden()
        elif item == "frames2":
            fixers_frames2_golden()
        elif item == "sigma":
            fixers_sigma_golden()
        elif item == "updown":
            fixers_updown_golden()
        elif item == "pre":
            preblock_golden()
        elif item == "gen2":
            conservation_golden()
        elif item == "diag":        # pressure-level products: geopotential, p-level interpolation, MSLP
            diag_golden()
        elif item == "wind":        # wind artifact filter: jet mask, masked Gaussian blend
            wind_golden()
        elif item == "advect":      # semi-Lagrangian tracer advection: omega, back-trajectory, trilinear gather
            advect_golden()
        elif item == "regrid":      # horizontal regridding: an ESMF sparse weight matrix on every plane
            regrid_golden()
        elif item == "hybrid":      # hybrid-level interpolation: one set of hybrid levels onto another, linear in log p
            hybrid_golden()
        elif item == "metrics":     # gen-2 verification metrics: rmse, mse, mae, bias, r2score, log_variance_ratio, acc, activity
            metrics_golden()
        elif item == "ensemble":    # ensemble verification: CRPS (biased, fair, almost fair), spread, ensemble-mean error
            ensemble_golden()
        elif item == "xform":       # gen-2 variable transforms: fill_values, log / sqrt in, exp / square out
            xform_golden()
        elif item == "rec":
            reconstruct_golden()
        elif item == "asm":
            assemble_golden()
        elif item == "gen2loop":    # the composed gen-2 loop through the reference's own run_forecast
            gen2loop_golden()
        elif item == "fuxi_timm":   # BASELINE config 5's default stage: only where `import timm` works (skips loudly otherwise)
            fuxi_timm_golden()
        elif item in ("T0", "T1", "T0W", "T0U", "T0M", "T0F", "T0H", "T1H", "T0X"):
            model_golden(item, 1, capture_layers=(item in ("T0", "T0W", "T0U")))
        elif item == "camulator":   # credit/models/camulator.py: K0 / K0F with sampled sub-module outputs, K0X, K2048 (bf16 autocast figure)
            camulator_golden("K0", 1, cap_stride=2)
            camulator_golden("K0F", 1, cap_stride=2)
            camulator_golden("K0X", 2)
            camulator_golden("K2048", 1, autocast=True)
            camulator_post_golden()
        elif item == "blocks":
            blocks_golden()
        elif item == "specs":
            state_specs_golden()
        elif item == "RT":   # the model of the reference's own tests/test_crossformer.py
            model_golden(item, 2, False)
        elif item == "C1W":
            model_golden(item, 8, False)
        elif item == "C1":
            model_golden(item, 8, False)
        elif item in ("C3S", "C3"):
            model_golden(item, 16, False)
        elif item == "stressC3S":   # the stress families at HEADLINE map size (721 x 1440): the kernel instantiations only that size selects
            for fam in ("stress", "stress_hi"):
                model_golden("C3S", 16, False, family=fam)
        elif item == "stressC3":    # ... and through the full-width 124 M-parameter model
            for fam in ("stress", "stress_hi"):
                model_golden("C3", 16, False, family=fam)
        elif item == "stress":   # the stress weight families (wxengine.synth.FAMILIES) through the reference: T0 / T1 full maps, C1 strided
            for fam in ("stress", "stress_hi"):
                model_golden("T0", 1, False, family=fam)
                model_golden("T1", 1, False, family=fam)
                model_golden("C1", 8, False, family=fam)
        else:
            raise SystemExit(f"unknown item {item}")


if __name__ == "__main__":
    main()
