"""Every class of model wx_create accepts, not only the named configs: the HIP engine against the fp64 oracle at the tiny configs of
synth_batches.ACCEPTED_CONFIGS (W: window sides 6 - 15, H: wide heads at 36 - 121 tokens, E: CrossEmbed kernel sets, F: interp /
use_spectral_norm off), output and every per-block capture, with the suite's stated gates (test_engine_gpu.check):
    fp32 / fp32s: max|y - ref| <= 1e-4 * max|ref|;   bf16: rel-L2 <= 2e-2 and max err <= 5e-2 * max|ref|;   `pad` bit exact in fp32.
Proof of path: wx_query "attn_nkf_mask" / "attn_block_nkf_mask" (which key-fragment counts the two attention kernels ran with) and the
profile's launch counts (which CrossEmbed route ran)."""
import functools

import numpy as np
import pytest
import torch

from oracle import wxformer_oracle as O
from synth_batches import ACCEPTED_CONFIGS, accepted_config, accepted_precisions
from test_engine_gpu import check
from wxengine.engine import WXEngine
from wxengine.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
PRECS = ["fp32", "fp32s", "bf16"]
NKF_ALL = {1, 2, 4, 7, 8, 10, 12, 14, 16}     # window_attn_kernel's instantiations (attn_nkf_tokens)
NKF_BLOCK = {1, 2, 4, 7, 8}                   # attn_block_kernel's
_masks = {}                                   # (name, mode) -> (window kernel mask, block kernel mask) of one forward


def names(cls):
    return [n for n, e in ACCEPTED_CONFIGS.items() if e["cls"] == cls]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 oracle of a config, computed once and shared (read only)."""
    cfg = accepted_config(name)
    sd = synth_state_dict(cfg)
    x = synth_input(cfg)
    cap = {}
    y = O.forward(cfg, sd, x, dtype=torch.float64, capture=cap)
    return cfg, sd, x, y.numpy(), {k: v[0].numpy() for k, v in cap.items()}


def make_engine(name, prec):
    cfg, sd, _, _, _ = reference(name)
    eng = WXEngine(cfg, prec, 0)     # reads the WX_* switches here
    eng.load_state_dict(sd)
    eng.finalize()
    return eng


def bits(mask):
    return {n for n in range(64) if mask >> n & 1}


def worst(got, ref):
    d = np.asarray(got, np.float64) - ref
    return np.abs(d).max() / np.abs(ref).max(), np.linalg.norm(d) / np.linalg.norm(ref)


def run_against_oracle(name, prec, mode=""):
    """Forward + every debug capture against the fp64 oracle, then two plain forwards bit-identical.  Returns the engine."""
    cfg, _, x, y_ref, cap = reference(name)
    eng = make_engine(name, prec)
    xd = torch.from_numpy(x).cuda()
    eng.set_debug(True)
    y = eng.forward(xd).cpu().numpy()
    assert y.shape == y_ref.shape == (1, cfg.output_channels, 1) + tuple(cfg.out_hw)
    w_max, w_l2, w_key = (*worst(y, y_ref), "y")
    first = None       # the first capture outside the gate names the kernel
    for k, v in cap.items():
        got = eng.debug_read(k)
        assert got.shape == v.shape, k
        m, l2 = worst(got, v)
        if first is None and k != "pad" and (m > 1e-4 if prec != "bf16" else (m > 5e-2 or l2 > 2e-2)):
            first = f"{k} ({m:.3e}, rel-L2 {l2:.3e})"
        if m > w_max:
            w_max, w_l2, w_key = m, l2, k
    print(f"\n[accepted] {name} {prec}{mode}: worst max err / max|ref| {w_max:.3e} (rel-L2 {w_l2:.3e}) at {w_key}; y: {worst(y, y_ref)[0]:.3e}"
          + (f"; FIRST capture outside the gate: {first}" if first else ""))
    check(y, y_ref, prec)
    for k, v in cap.items():
        got = eng.debug_read(k)
        if k == "pad" and prec in ("fp32", "fp32s"):
            np.testing.assert_array_equal(got, v.astype(np.float32))   # pure data movement: bit exact
        else:
            try:
                check(got, v, prec)
            except AssertionError as e:
                raise AssertionError(f"capture {k}: {e}") from None
    assert len(cap) >= 20
    eng.set_debug(False)
    y1 = eng.forward(xd).clone()
    _masks[(name, prec + mode)] = (eng.query("attn_nkf_mask"), eng.query("attn_block_nkf_mask"))
    assert torch.equal(y1, eng.forward(xd)), "two runs on the same input must be bit-identical"
    check(y1.cpu().numpy(), y_ref, prec)    # the schedule without the captures (the fused FeedForward forms are off under debug)
    return eng


def assert_window_kernel_took(name, key, claimed):
    win, blk = _masks[(name, key)]
    assert claimed <= bits(win), f"{name} {key}: window_attn_kernel ran NKF {sorted(bits(win))}, the class claims {sorted(claimed)}"
    return blk


@pytest.mark.parametrize("prec", ["fp32", "fp32s"])
@pytest.mark.parametrize("name", names("W"))
def test_window_sides_fp32(name, prec):
    """Class W on the fp32 storage modes: window_attn_kernel at every swept side (fp32s: its three-MFMA form at 2 / 4 / 7 / 8 key
    fragments, the exact-f32 products at the others)."""
    run_against_oracle(name, prec)
    assert assert_window_kernel_took(name, prec, ACCEPTED_CONFIGS[name]["nkf"]) == 0    # the block kernel is bf16 only


@pytest.mark.parametrize("block", ["1", "0"])
@pytest.mark.parametrize("name", names("W"))
def test_window_sides_bf16(name, block, monkeypatch):
    """Class W in bf16, twice: WX_ATTN_BLOCK=1 (the one-launch attention sub-block wherever attn_block_kernel<C, NKF> exists: widths
    32 - 256 at <= 8 key fragments) and WX_ATTN_BLOCK=0 (the to_qkv | window_attn_kernel | to_out chain everywhere), each against the
    oracle."""
    monkeypatch.setenv("WX_ATTN_BLOCK", block)
    run_against_oracle(name, "bf16", f"/block{block}")
    win, blk = _masks[(name, f"bf16/block{block}")]
    claimed = ACCEPTED_CONFIGS[name]["nkf"]
    if block == "0":
        assert claimed <= bits(win) and blk == 0
    else:   # every width here is 32 - 256: the block kernel takes what it has an instantiation for, the chain the larger windows
        assert claimed & NKF_BLOCK <= bits(blk) and claimed - NKF_BLOCK <= bits(win), (sorted(bits(win)), sorted(bits(blk)))


@pytest.mark.parametrize("name,prec", [(n, p) for n in names("H") for p in accepted_precisions(n)])
def test_wide_heads(name, prec):
    """Class H: dim_head 64 / 128 on the general-head-width kernel at 4 (partly filled), 7 (partly filled) and 8 key fragments.
    (dim_head 128 at 81 / 121 tokens is a bf16 model: in fp32 storage the kernel's four V images pass 160 KB of LDS and wx_create
    refuses the config -- tests/test_abi_cpu.py::test_create_time_rejections_c_abi.)"""
    run_against_oracle(name, prec)
    assert assert_window_kernel_took(name, prec, ACCEPTED_CONFIGS[name]["nkf"]) == 0    # the block kernel is built around 32-wide heads


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", names("E"))
def test_cross_embed_kernel_sets(name, prec):
    """Class E, and which route the packer chose: the LDS-patch kernel (stride 2 with k = 32; k = 4 rides along), one GEMM per branch
    (stage 0 otherwise; single branches), one merged GEMM per stage (same-parity kernels of stages 1 - 3, three of them included)."""
    eng = run_against_oracle(name, prec)
    eng.profile(2)
    eng.forward(torch.from_numpy(reference(name)[2]).cuda())
    got = {r["name"]: r["launches"] for r in eng.profile_read()}
    eng.profile(0)
    for k, n in ACCEPTED_CONFIGS[name]["embed"].items():
        assert sum(v for kk, v in got.items() if kk == k or kk.startswith(k + ".")) == n, (k, {kk: v for kk, v in got.items() if "embed" in kk})


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", names("F"))
def test_flags(name, prec):
    """Class F: interp = False (the tail crops, never resizes: output size = decoder size minus the pads, equal to the image or not),
    use_spectral_norm = False (plain `weight` keys, no fold), and both with the PixelShuffle and the upsample_v_conv decoder."""
    run_against_oracle(name, prec)


def test_every_key_fragment_count_ran():
    """The union over this file: window_attn_kernel at every NKF it is built for, attn_block_kernel at every NKF it is built for.  (A
    class not run before this test in the same session -- a -k selection -- is run here, forward only.)"""
    for name in names("W") + names("H"):
        for prec, env in (("fp32", None), ("bf16/block1", "1")):
            if (name, prec) in _masks or (env and ACCEPTED_CONFIGS[name]["cls"] == "H") or prec.split("/")[0] not in accepted_precisions(name):
                continue
            with pytest.MonkeyPatch.context() as mp:
                if env:
                    mp.setenv("WX_ATTN_BLOCK", env)
                eng = make_engine(name, prec.split("/")[0])
            eng.forward(torch.from_numpy(reference(name)[2]).cuda())
            _masks[(name, prec)] = (eng.query("attn_nkf_mask"), eng.query("attn_block_nkf_mask"))
    win = functools.reduce(lambda a, b: a | b, (m[0] for m in _masks.values()))
    blk = functools.reduce(lambda a, b: a | b, (m[1] for m in _masks.values()))
    assert bits(win) == NKF_ALL and bits(blk) == NKF_BLOCK, (sorted(bits(win)), sorted(bits(blk)))
