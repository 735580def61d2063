"""Synthetic, name-keyed weights and inputs (SURVEY.md §8(c) "Fixture plan").

Real checkpoints cannot be shipped (25-124 M parameters) and torch's init order
is not reproducible without the reference code, so every tensor is generated
from a counter-based RNG (numpy Philox) keyed by the FNV-1a hash of its
state-dict key.  The same generator feeds the reference (when building golden
fixtures), the oracle and the engine, so all three see bit-identical weights.

Spectral-norm caveat (SURVEY.md header): `eval()` uses the stored `weight_u`,
`weight_v` without power iteration, so random u/v make activations explode.  We
store u/v after `POWER_ITERS` power iterations on `weight_orig`, which is what a
trained checkpoint holds.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

POWER_ITERS = 6
_FNV_OFFSET = 0xCBF29CE484222325
_FNV_PRIME = 0x100000001B3


def fnv1a64(text: str) -> int:
    h = _FNV_OFFSET
    for b in text.encode("utf-8"):
        h ^= b
        h = (h * _FNV_PRIME) & 0xFFFFFFFFFFFFFFFF
    return h


def keyed_normal(key: str, shape, seed: int = 0) -> np.ndarray:
    """float32 N(0,1) tensor that depends only on (key, seed, shape)."""
    g = np.random.Generator(np.random.Philox(key=[fnv1a64(key), seed & 0xFFFFFFFFFFFFFFFF]))
    return g.standard_normal(size=shape, dtype=np.float32)


def is_transposed_conv(prefix: str, arch: str = "crossformer", upconv: bool = False) -> bool:
    """ConvTranspose2d modules of the legacy decoder (reference crossformer.py:92,572):
    their spectral norm is taken over weight dim 1.  The wxformer decoder and the upsample_v_conv variant have none."""
    if arch in ("wxformer", "camulator") or upconv:
        return False
    return prefix == "up_block4" or (prefix.startswith("up_block") and prefix.endswith(".conv"))


def _l2n(v, eps=1e-12):
    return v / max(float(np.linalg.norm(v)), eps)


def power_iterate(w_mat: np.ndarray, u0: np.ndarray, iters: int = POWER_ITERS):
    """torch.nn.utils.spectral_norm's power iteration (fp32), returns (u, v)."""
    u = _l2n(u0.astype(np.float32))
    v = None
    for _ in range(iters):
        v = _l2n(w_mat.T @ u)
        u = _l2n(w_mat @ v)
    return u.astype(np.float32), v.astype(np.float32)


# Weight FAMILIES.  "base" (every fixture of rounds 1-3): kaiming-like weights, gains 1 + 0.1 z, shifts 0.1 z -- activations O(1), LayerNorm
# inputs with means near 0, attention logits of a few units.  Trained checkpoints are not like that, so two stress families push the
# places a well-conditioned family cannot reach:
#   "stress"    -- the bf16 engine's gates still apply: CrossEmbed biases of one sign (residual-stream rows with |mean| / sigma of ~5: at
#                  |mean| / sigma = r a bf16 STREAM carries r * 2^-8 / sqrt(12) of rounding noise per normalised element, so r ~ 8 is where
#                  bf16 storage itself reaches the 2e-2 gate), attention LayerNorm gains x ATTN_GAIN (softmax logits of +-40 and more),
#                  FeedForward LayerNorm gains x FF_GAIN (pre-GELU |x| ~ 1e2), decoder conv biases of one sign (GroupNorm groups with
#                  |mean| / sigma ~ 10).
#   "stress_hi" -- fp32 engine (the parity mode): |mean| / sigma of 30-300 in the LayerNorm and GroupNorm inputs (one-pass variance
#                  cancellation), the same gains, and ONE hidden unit per FeedForward whose pre-activation exceeds the f16 range
#                  (b1 = 7e4; its W2 column is scaled by 1e-4 so that the unit does not drown the rest of the signal).  The bf16
#                  engine must stay finite on it and is reported, not gated at 2e-2.
FAMILIES = {
    "base": None,
    "stress": dict(embed_bias=3.0, embed_spread=0.05, attn_gain=8.0, ff_gain=60.0, res_bias=0.0, dec_bias=4.0, dec_spread=0.02, overflow=False),
    "stress_hi": dict(embed_bias=100.0, embed_spread=0.002, attn_gain=1.0, ff_gain=1.0, res_bias=1.0, dec_bias=60.0, dec_spread=0.001, overflow=True),
}
OVERFLOW_B1 = 7.0e4      # > 65504 = the largest finite f16
OVERFLOW_W2_SCALE = 1.0e-4


def _family_adjust(key: str, shape, val: np.ndarray, z: np.ndarray, fam) -> np.ndarray:
    """One tensor of a stress family from its base value `val` and its N(0,1) draw `z` (same draw as the base family)."""
    parts = key.split(".")
    if key.startswith("layers.") and parts[2] == "0" and key.endswith(".bias"):          # CrossEmbed conv biases
        return (fam["embed_bias"] * (1.0 + fam["embed_spread"] * z)).astype(np.float32)
    if key.startswith("layers.") and len(parts) >= 6 and parts[2] == "1" and ".dpb." not in key:
        if key.endswith(".norm.g"):                                                          # attention LayerNorm gain
            return (val * fam["attn_gain"]).astype(np.float32)
        if key.endswith(".layers.0.g"):                                                      # FeedForward LayerNorm gain
            return (val * fam["ff_gain"]).astype(np.float32)
        if fam["res_bias"] and key.endswith((".to_out.bias", ".layers.4.bias")):               # residual-branch biases of one sign: the row mean keeps growing
            return (fam["res_bias"] * (1.0 + 0.02 * z)).astype(np.float32)
        if fam["overflow"] and key.endswith(".layers.1.bias"):                               # hidden unit 3: beyond the f16 range
            out = val.copy()
            out[3] = OVERFLOW_B1
            return out
        if fam["overflow"] and key.endswith((".layers.4.weight_orig", ".layers.4.weight")):  # ... and its W2 column, damped
            out = val.copy()
            out[:, 3] *= OVERFLOW_W2_SCALE
            return out
    if key.startswith("up_block") and ".b." in key and key.endswith(".bias") and len(shape) == 1 and parts[2] in ("0", "3"):
        return (fam["dec_bias"] * (1.0 + fam["dec_spread"] * z)).astype(np.float32)        # 3x3 conv biases in front of a GroupNorm
    return val


def synth_state_dict(cfg, seed: int = 0, family: str = "base") -> "OrderedDict[str, np.ndarray]":
    """Full reference-layout state dict (numpy float32) for `cfg.state_spec()`; `family` picks the weight family above."""
    fam = FAMILIES[family]
    spec = cfg.state_spec()
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for key, shape in spec.items():
        if key.endswith((".weight_u", ".weight_v")):
            continue  # filled below with their weight_orig
        z = keyed_normal(key, shape, seed)
        if key.endswith(".noise_factor"):   # noise layers: magnitudes that matter against the activations
            sd[key] = (0.3 * (1.0 + 0.1 * z)).astype(np.float32)
            continue
        if key.endswith(".modulation"):
            sd[key] = (1.0 + 0.5 * np.tanh(z)).astype(np.float32)
            continue
        if key.endswith(".weight_orig") or (key.endswith(".weight") and len(shape) >= 2):
            fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else shape[0]
            sd[key] = (z / np.sqrt(max(fan_in, 1))).astype(np.float32)
        elif key.endswith((".g", ".weight")) and (len(shape) == 1 or key.endswith(".g")):
            sd[key] = (1.0 + 0.1 * z).astype(np.float32)  # LN/GN gains
        else:
            sd[key] = (0.1 * z).astype(np.float32)  # biases, LN/GN shifts
        if fam is not None:
            sd[key] = _family_adjust(key, shape, sd[key], z, fam)
    for key, shape in spec.items():
        if not key.endswith(".weight_u"):
            continue
        base = key[: -len(".weight_u")]
        w = sd[base + ".weight_orig"]
        transposed = is_transposed_conv(base, getattr(cfg, "arch", "crossformer"), bool(getattr(cfg, "upsample_v_conv", False)))
        if transposed:  # ConvTranspose2d: spectral_norm(dim=1)
            w_mat = np.moveaxis(w, 1, 0).reshape(w.shape[1], -1)
        else:
            w_mat = w.reshape(w.shape[0], -1)
        u, v = power_iterate(w_mat, keyed_normal(key, (w_mat.shape[0],), seed))
        sd[base + ".weight_u"] = u
        sd[base + ".weight_v"] = v
    return OrderedDict((k, sd[k]) for k in spec)


def synth_input(cfg, seed: int = 1000) -> np.ndarray:
    """x0 ~ N(0,1), float32 [1, C_in, frames, H, W] (SURVEY.md §8(d) 'Synthetic inputs')."""
    return keyed_normal("x0", (1, cfg.base_input_channels, cfg.frames, cfg.image_height, cfg.image_width), seed)


def synth_forcing(cfg, n_dyn: int, step: int, seed: int = 1000) -> np.ndarray:
    """Per-step dynamic forcing, float32 [1, n_dyn, 1, H, W]."""
    return keyed_normal(f"frc{step}", (1, n_dyn, 1, cfg.image_height, cfg.image_width), seed)


def synth_denorm(n_out: int, seed: int = 0):
    """Per-output-channel (mean, std) with std in [0.5, 2], mean in [-1, 1]."""
    z = keyed_normal("denorm", (2, n_out), seed)
    mean = np.tanh(z[0]).astype(np.float32)
    std = (0.5 + 1.5 / (1.0 + np.exp(-z[1]))).astype(np.float32)
    return mean, std
