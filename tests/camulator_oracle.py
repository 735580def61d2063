"""CPU oracle of credit/models/camulator.py::Camulator.forward (torch CPU, fp32 or fp64) -- test infrastructure, built from the
pieces of oracle/wxformer_oracle.py:

    pad -> mean of the two frames (frames == 2) -> 4 x (legacy-padded CrossEmbed -> Transformer) -> UpBlockPS x 3 (+ skip concat)
    -> conv3x3 / PixelShuffle / conv3x3 head -> unpad -> bilinear

Capture names are those of wxformer_oracle.forward; "pad" is what the first CrossEmbed reads, i.e. the padded AVERAGE.
tools/make_goldens.py --only camulator pins it to the reference class (tests/golden/model_K*.npz)."""
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle import wxformer_oracle as O


def average_frames(x: torch.Tensor) -> torch.Tensor:
    """camulator.py:587-590.  x [B, C, T, H, W] -> [B, C, H, W]: F.avg_pool3d(x, (2, 1, 1)).squeeze(2) at T == 2 -- a two-element
    average pool computes (a + b) / 2, and a division by two is the multiplication by 0.5 bit for bit -- or squeeze(2) at T == 1."""
    if x.shape[2] == 1:
        return x[:, :, 0]
    if x.shape[2] != 2:
        raise ValueError("camulator: frames must be 1 or 2")
    return (x[:, :, 0] + x[:, :, 1]) * 0.5


def forward(cfg, sd: Dict, x, dtype=torch.float32, capture: Optional[Dict] = None) -> torch.Tensor:
    """Camulator.forward (camulator.py:577-613) without the in-model PostBlock.
    x [B, C_in, frames, H, W] (or [B, C, H, W] when frames == 1) -> [B, C_out, 1, H, W]."""
    x = O._as_t(x, dtype)
    if x.dim() == 4:
        x = x.unsqueeze(2)
    if cfg.pad_activate:   # :582-583, on the five-dimensional tensor: every frame is padded alike
        x = (O.mirror_pad if getattr(cfg, "pad_mode", "earth") == "mirror" else O.earth_pad)(x, cfg.pad_lat, cfg.pad_lon)
    x = average_frames(x)
    if capture is not None:
        capture["pad"] = x
    g = cfg.dim[0]   # GroupNorm groups of every UpBlockPS (:537-539)
    outs = []
    for bi in range(x.shape[0]):
        cap = capture if bi == 0 else None
        z = x[bi:bi + 1]
        enc = []
        for s in range(4):
            z = O.cross_embed(z, sd, f"layers.{s}.0", list(cfg.cross_embed_kernel_sizes[s]), cfg.cross_embed_strides[s], "crossformer")
            if cap is not None:
                cap[f"layers.{s}.0"] = z
            z = O.transformer(z, sd, f"layers.{s}.1", cfg.depth[s], cfg.local_window_size[s], cfg.global_window_size[s],
                              cfg.dim_head, cap)
            if cap is not None:
                cap[f"layers.{s}.1"] = z
            enc.append(z)
        for i in (1, 2, 3):
            if i > 1:
                z = torch.cat([z, enc[4 - i]], dim=1)   # :599-603: up_block2 takes stage 2's stream, up_block3 stage 1's
            z = O.up_block_ps(z, sd, f"up_block{i}", g)
            if cap is not None:
                cap[f"up_block{i}"] = z
        z = torch.cat([z, enc[0]], dim=1)
        z = O.pixel_shuffle2(F.conv2d(z, O.folded_weight(sd, "up_block4.0", dtype), O._bias(sd, "up_block4.0", dtype), padding=1))
        z = F.conv2d(z, O.folded_weight(sd, "up_block4.2", dtype), O._bias(sd, "up_block4.2", dtype), padding=1)
        if cap is not None:
            cap["up_block4"] = z
        if cfg.pad_activate:
            z = O.earth_unpad(z, cfg.pad_lat, cfg.pad_lon)
        if cfg.interp:
            z = O.bilinear_resize(z, cfg.image_height, cfg.image_width)
        outs.append(z)
    return torch.cat(outs, dim=0).unsqueeze(2)
