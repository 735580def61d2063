"""Host side of the ensemble noise (CrossFormerWithNoise): a numpy restatement of the engine's generator and the draw tapes.

The engine's generator (csrc/wx_noise.h) is Philox4x32-10 keyed by the 64-bit seed, counter (quad, slot, member, step), with
Box-Muller on each pair of output words.  `normals` restates it in numpy (float64 transcendentals, rounded to float32: the device's
fp32 libm agrees to a few ulp), so tests can check the device draws element by element without a GPU-side reference.

A *tape* is the list of tensors the reference's forward draws with torch.randn, in its order: per noise layer (encoder 0..2, then
decoder 1..3) the latent z [B, Dn] then the pixel noise [B, C, H, W]; with `correlated` one latent first, then the pixel draws.
Tapes used by the goldens are generated from named keys (`tape_from_key`), so a fixture stores the key, never the draws.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from .synth import keyed_normal

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
SLOT_LATENT = 6   # latent of layer slot l: slot 6 + l (6 alone when correlated)
SLOT_PERTURB = 16  # the white source of the perturbed-initial-condition noise (csrc/wx_perturb.h, wxengine.perturb): element index
#                    e = (p * H + h) * W + x over the P = C * T planes of one member's [1, C, T, H, W] tensor, step = the forecast step;
#                    normals(seed, SLOT_PERTURB, member, step, n) are the first n draws of a call.  Slots 0 - 11 are the noise layers'.


def philox4x32_10(ctr, key) -> np.ndarray:
    """Philox4x32-10 (Random123).  ctr: uint32 array [..., 4]; key: (k0, k1).  Returns uint32 [..., 4]."""
    c = [np.asarray(ctr, dtype=np.uint64)[..., i].copy() for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def _box_muller(w0, w1):
    u1 = ((w0 >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w1 >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    rho = np.sqrt(-2.0 * np.log(u1))
    return rho * np.cos(2.0 * np.pi * u2), rho * np.sin(2.0 * np.pi * u2)


def normals(seed: int, slot: int, member: int, step: int, n: int) -> np.ndarray:
    """The first n normals (logical element index 0 .. n-1) the engine draws for (slot, member, step), float32."""
    nq = (n + 3) // 4
    ctr = np.zeros((nq, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(nq, dtype=np.uint32)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = slot, member, step
    w = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    n0, n1 = _box_muller(w[:, 0], w[:, 1])
    n2, n3 = _box_muller(w[:, 2], w[:, 3])
    return np.stack([n0, n1, n2, n3], axis=-1).reshape(-1)[:n].astype(np.float32)


def layer_shapes(cfg) -> List[Tuple[str, int, int, int]]:
    """[(prefix, C, H, W)] of the noise layers in draw order (the stage map each one acts on)."""
    hw = cfg.stage_hw
    out = []
    for p, c in cfg.noise_layers():
        s = int(p.rsplit(".", 1)[-1]) if p.startswith("encoder") else 3 - int(p[-1])
        out.append((p, c, hw[s][0], hw[s][1]))
    return out


def tape_shapes(cfg, batch: int) -> List[Tuple[int, ...]]:
    """Shapes of the reference forward's torch.randn calls, in order."""
    dn = cfg.noise_latent_dim
    shapes: List[Tuple[int, ...]] = [(batch, dn)] if cfg.correlated else []
    for _, c, h, w in layer_shapes(cfg):
        if not cfg.correlated:
            shapes.append((batch, dn))
        shapes.append((batch, c, h, w))
    return shapes


def tape_from_key(cfg, batch: int, key: str) -> List[np.ndarray]:
    """A draw tape from named keyed-normal streams: entry i = keyed_normal(f"{key}.{i}", shape_i)."""
    return [keyed_normal(f"{key}.{i}", shp) for i, shp in enumerate(tape_shapes(cfg, batch))]
