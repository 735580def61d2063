"""Teacher-forced per-sub-block parity of the bf16 routes the engine takes BY DEFAULT (tests/teacher_forced.py explains the distance d).

The per-block tests of test_engine_gpu / test_variants_gpu switch captures on at level 1, and at level 1 the engine leaves the PRE /
POST forms of the fused FeedForward (wx_ff.h, wx_ff_split.h) and the k-blocked attention chain for their unfused forms.  Here every
engine runs at capture level 2 -- the kernels of a capture-free forward, captured where their results are row-major in memory --
and every link between two captures is compared element by element with the oracle's fp64 function of the engine's own input.

Routes (one bf16 engine per case; the profile of the CAPTURED forward proves which kernels ran):

  plain      WX_ATTN_BLOCK=0 WX_NO_FFFUSE=1 WX_NO_STREAM=1 WX_NO_WREG=1    T1, C1, T5     the reference measurement: b_plain
  ff_fused   WX_FF_MIN_WGS=0 WX_ATTN_BLOCK=0                               T1, C1         out_ff_fused (PRE), out_ff_qkv_fused (POST); T1:
                                                                                          200 tokens at C = 128 = 2 tiles, the last of
                                                                                          72; 50 at C = 256 = one ragged 64-tile
  default    --                                                            C1, T1         attn_block, ff_fused / ff_fused_split
  attn_block WX_ATTN_BLOCK=1                                               T1, T5, RT     the one-launch attention block everywhere
  stream     WX_STREAM_MIN_ROWS=0                                          T5, C1         persistent GEMMs + k-blocked attention chain
  wreg       WX_WREG_MIN_ROWS=0 WX_SKINNY_MAX=0                            T5, C1         weight-stationary GEMMs
  plain / ff_fused on the "stress" weight family                           T1

The bf16 gate is measured, then held: b_plain = the worst d over all links of the plain-chain engines, per weight family.  The plain
chain is held to 1.25 x b_plain, every other route to 2 x b_plain (the fused forms round the hidden tensor to f16 and never round x1,
so they should be no worse than the chain; the factor 2 is for a different order of the LayerNorm partial sums and of the K walk).
2 x b_plain <= 0.1 is a CONDITION: the CPU stand-in of test_teacher_forced_cpu needs 0.015 and its weakest mutant 0.30 -- a route that
needs more is a kernel to look into, not a figure to record.

Measured on MI355X (worst d over the links of each engine; teacher_forced.B_PLAIN records b_plain):
  plain      T1 0.0126   C1 0.0121   T5 0.0105                 -> b_plain(base) = 0.0126 (a FeedForward link at C = 32); gates 0.0158 / 0.0252
  ff_fused   T1 0.0126   C1 0.0118   (their out+ff links: 0.0075 / 0.0101)
  default    C1 0.0147   T1 0.0126   (C1: the attention block of stage 2, 2 x 2 long windows)
  attn_block T1 0.0126   T5 0.0098   RT 0.0125
  stream     T5 0.0131   C1 0.0147   (T5: a k-blocked attention sub-block of stage 2)
  wreg       T5 0.0093   C1 0.0147
  stress     plain T1 0.0135 -> b_plain(stress) = 0.0135; gates 0.0169 / 0.0270;   ff_fused T1 0.0135 (out+ff 0.0129)
  fp32s C1   worst row error 1.4e-5 of max_row|ref| (tolerance 1e-4)
What the gate found when it was first run: the PRE form of ff_fused_kernel (wx_ff.h) rounded x1 = x + W_out . o + b_o to bf16 and
used the rounded value as the residual too, although x1 is never stored on that path -- out+ff links at d = 0.0324 (T1, stage 2, token
163 of 200) and 0.0432 (C1, stage 1), over 2 x b_plain = 0.0252, every row alike (not a tile edge).  A CPU model of the launch gives
0.028 - 0.044 with the rounded residual and 0.006 - 0.010 without.  The kernel now keeps what the rounding took off in the
accumulators of the second GEMM, so the residual is x1 in fp32; the figures above are from after that change.

Every case also asserts that the level-2 forward is bit-identical to the same engine's forward with captures off, and that a level-1
forward still produces every capture the reference names.

One fp32s engine (C1, default switches) at level 2 must report the PRE / POST counts of the one-launch split-bf16 FeedForward that
test_variants_gpu computes without captures; its links are held per token row to the suite's stated fp32 tolerance,
|got - ref| <= 1e-4 * max_row|ref|.

The convolutional rest of the forward -- CrossEmbeds, UpBlocks, the up_block4 head, the tail -- is judged the same way from the
captures of the decoder's stored intermediates: test_bf16_conv_links_teacher_forced and test_fp32_conv_links_teacher_forced below
(their routes, gates and measurements are in the former's docstring)."""
import os

import pytest
import torch

import teacher_forced as TF
from wxengine.config import named_config
from wxengine.engine import WXEngine
from wxengine.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu

PLAIN = {"WX_ATTN_BLOCK": "0", "WX_NO_FFFUSE": "1", "WX_NO_STREAM": "1", "WX_NO_WREG": "1"}
FF_FUSED = {"WX_FF_MIN_WGS": "0", "WX_ATTN_BLOCK": "0"}
ROUTES = {
    "plain": PLAIN,
    "ff_fused": FF_FUSED,
    "default": {},
    "attn_block": {"WX_ATTN_BLOCK": "1"},
    "stream": {"WX_STREAM_MIN_ROWS": "0"},
    "wreg": {"WX_WREG_MIN_ROWS": "0", "WX_SKINNY_MAX": "0"},
}
CASES = [("plain", n, "base") for n in ("T1", "C1", "T5")] + [("ff_fused", n, "base") for n in ("T1", "C1")] + \
        [("default", n, "base") for n in ("C1", "T1")] + [("attn_block", n, "base") for n in ("T1", "T5", "RT")] + \
        [("stream", n, "base") for n in ("T5", "C1")] + [("wreg", n, "base") for n in ("T5", "C1")] + \
        [("plain", "T1", "stress"), ("ff_fused", "T1", "stress")]


def _engine(name, prec, env, family="base"):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        cfg = named_config(name)
        sd = synth_state_dict(cfg, family=family)
        eng = WXEngine(cfg, prec, 0)   # the switches are read when the engine is created
        eng.load_state_dict(sd)
        eng.finalize()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return cfg, sd, eng


def _level1_names(cfg):
    """Every capture a level-1 forward has always produced: the names of the oracle's own capture dict."""
    names = ["pad"] + [f"layers.{s}.{j}" for s in range(4) for j in (0, 1)] + [f"up_block{i}" for i in (1, 2, 3, 4)]
    for p in TF.pairs(cfg):
        names += [p.attn, p.ff]
    return names


def _captured_forward(eng, cfg, x):
    """(y at level 0, y at level 2, the level-2 captures, the profile rows and the k-blocked count of the CAPTURED forward)."""
    y0 = eng.forward(x).clone()
    eng.set_debug(2)
    eng.profile(3)
    eng.profile_reset()
    y2 = eng.forward(x).clone()
    torch.cuda.synchronize()
    rows = [r["name"] for r in eng.profile_read()]
    eng.profile(0)
    caps = TF.read_captures(eng, cfg)
    queries = {k: eng.query(k) for k in ("attn_blk", "ff_split_pre", "ff_split_post")}
    eng.set_debug(1)
    eng.forward(x)
    for k in _level1_names(cfg):
        assert eng.debug_read(k).ndim == 3, k
    eng.set_debug(0)
    return y0, y2, caps, rows, queries


def _prove_route(route, name, rows, queries, kinds, attn_outs):
    """The kernels the route is about ran in the captured forward, and the links that only exist on that route were built."""
    base = {r.split("@")[0].split(".")[0] for r in rows}
    tags = {r.split("@")[1] for r in rows if "@" in r}
    if route == "plain":
        assert not any("fused" in b or b.startswith("attn_block") for b in base), rows
        assert not tags & {"stream", "stream_lc", "wreg"}, rows
        assert {"qkv", "core", "out", "ff"} <= kinds and not kinds & {"attn", "out+ff"}, kinds
    elif route == "ff_fused":
        assert {"out_ff_fused", "out_ff_qkv_fused"} <= base, rows
        assert {"out+ff", "qkv", "core"} <= kinds, kinds    # (qkv: also the POST form's q|k|v, read behind the next attention)
    elif route == "default":
        assert any(b.startswith("attn_block") for b in base) and base & {"ff_fused", "ff_fused_split"}, rows
        assert {"attn", "ff"} <= kinds, kinds
    elif route == "attn_block":
        assert any(b.startswith("attn_block") for b in base), rows
        assert "attn" in kinds, kinds
    elif route == "stream":
        assert tags & {"stream", "stream_lc"} and queries["attn_blk"] >= 2, (rows, queries)
        assert {"attn", "ff"} <= kinds, kinds    # the k-blocked chain leaves the sub-block's output only
        assert sum(o.startswith(("layers.2.", "layers.3.")) for o in attn_outs) >= 2, attn_outs
    elif route == "wreg":
        assert "wreg" in tags, rows


@pytest.mark.parametrize("route,name,family", CASES, ids=["-".join(c) for c in CASES])
def test_bf16_route_links_teacher_forced(route, name, family):
    cfg, sd, eng = _engine(name, "bf16", ROUTES[route], family)
    x = torch.from_numpy(synth_input(cfg)).cuda()
    y0, y2, caps, rows, queries = _captured_forward(eng, cfg, x)
    assert torch.equal(y0, y2), f"{route} {name}: capture level 2 changed the forward (max {float((y0 - y2).abs().max()):.3e})"
    links = TF.build_links(cfg, sd, caps, "bf16")
    _prove_route(route, name, rows, queries, {k.kind for k in links}, [k.out for k in links if k.kind == "attn"])
    assert len(links) >= 2 * 2 * sum(cfg.depth), len(links)    # at least the attention and the FeedForward of every sub-block pair
    res = [TF.link_distance(k, TF.A_BF16) for k in links]
    by_kind = {}
    for r in res:
        if r.d >= by_kind.get(r.kind, r).d:
            by_kind[r.kind] = r
    w = max(res, key=lambda r: r.d)
    b_plain = TF.B_PLAIN[family]
    gate = (TF.PLAIN_FACTOR if route == "plain" else TF.ROUTE_FACTOR) * b_plain
    print(f"[teacher-forced] {route} {name} {family}: {len(links)} links, worst d {w.d:.4f} ({w.kind} -> {w.out}, channel {w.channel}, token {w.token}); "
          f"gate {gate:.4f}; per kind " + ", ".join(f"{k} {r.d:.4f}" for k, r in sorted(by_kind.items())))
    assert TF.ROUTE_FACTOR * b_plain <= TF.B_CEIL
    bad = [r for r in res if not r.d <= gate]
    assert not bad, f"{route} {name} {family}: {len(bad)} link(s) over d = {gate:.4f}: " + "; ".join(
        f"{r.kind} -> {r.out} d {r.d:.4f} at channel {r.channel}, token {r.token}" for r in bad[:8])


def test_fp32s_default_route_links_teacher_forced():
    cfg, sd, eng = _engine("C1", "fp32s", {})
    x = torch.from_numpy(synth_input(cfg)).cuda()
    y0, y2, caps, rows, queries = _captured_forward(eng, cfg, x)
    assert torch.equal(y0, y2), "fp32s C1: capture level 2 changed the forward"
    # the counts of test_split_feedforward_takes_out_projection / _makes_next_qkv, now under captures
    n_sub = sum(2 * d for d, c in zip(cfg.depth, cfg.dim) if c in (128, 256))
    n_post = sum((d if gw > 1 else 0) + (d - 1) for d, c, gw in zip(cfg.depth, cfg.dim, cfg.global_window_size) if c in (128, 256))
    assert n_sub > 0 and queries["ff_split_pre"] == n_sub and queries["ff_split_post"] == n_post, queries
    links = TF.build_links(cfg, sd, caps, "fp32s")
    kinds = {k.kind for k in links}
    assert {"qkv", "core", "out", "ff", "out+ff"} <= kinds, kinds
    assert sum(k.kind == "out+ff" for k in links) == n_sub
    worst = 0.0
    for k in links:
        e, tok = TF.fp32_row_excess(k)
        worst = max(worst, e)
        assert e <= TF.FP32_TOL, f"fp32s C1 {k.kind} -> {k.out}: |got - ref| = {e:.3e} of the row's max|ref| at token {tok}"
    print(f"[teacher-forced] fp32s C1 default: {len(links)} links, worst row error {worst:.3e} of max_row|ref| (tolerance {TF.FP32_TOL:.0e})")


# --------------------------------------------------------------------------- #
# CrossEmbed, decoder, tail (teacher_forced.build_conv_links)
# --------------------------------------------------------------------------- #
CONV_PLAIN = {"WX_NO_GEMM8P": "1", "WX_NO_EMBED_MERGE": "1", "WX_NO_EMBED_RIDE4": "1", "WX_NO_EMBED_SPLIT": "1", "WX_NO_SPLIT_K": "1",
              "WX_GN_FOLD_TILES": "0"}
CONV_ROUTES = {
    "conv_plain": CONV_PLAIN,
    "default": {},
    "gemm8p": {"WX_GEMM8P_MIN_ROWS": "1"},
    "kb128": {"WX_GEMM_CFG": "1"},
    "kb64": {"WX_GEMM_CFG": "2"},
    "no_patch": {"WX_NO_PATCH": "1"},
    "no_planar": {"WX_NO_PLANAR": "1"},
}
CONV_CASES = [("conv_plain", n) for n in ("T0", "T1", "T0W", "T0U", "T5")] + \
             [("default", n) for n in ("T0", "T1", "T0X", "T0F", "T0M", "T0W", "T0U", "RT", "T5", "C1", "C1W")] + \
             [("gemm8p", n) for n in ("T5", "C1")] + [("kb128", "T5"), ("kb64", "T5"), ("no_patch", "T1"), ("no_planar", "T1")]
FP32_CONV_CASES = [("fp32", n) for n in ("T1", "T0W", "T0U")] + [("fp32s", n) for n in ("T1", "T0W", "T0U", "C1")]
SKIP_EMBED0 = ("C1", "C1W")     # the one link left out (teacher_forced.build_conv_links says why)


def _captured_conv_forward(eng, cfg, x):
    """(y at level 0, y at level 2, the level-2 captures with "y", profile row -> launches and the split-K count of the CAPTURED forward)."""
    y0 = eng.forward(x).clone()
    eng.set_debug(2)
    eng.profile(3)
    eng.profile_reset()
    y2 = eng.forward(x).clone()
    torch.cuda.synchronize()
    rows = {r["name"]: r["launches"] for r in eng.profile_read()}
    eng.profile(0)
    caps = TF.read_captures(eng, cfg, TF.conv_capture_names(cfg))
    caps["y"] = y2[0].reshape(-1, y2.shape[-2], y2.shape[-1]).cpu().numpy()
    splitk = eng.query("splitk_gemms")
    eng.set_debug(1)
    eng.forward(x)
    for k in _level1_names(cfg):
        assert eng.debug_read(k).ndim == 3, k
    eng.set_debug(0)
    return y0, y2, caps, rows, splitk


def _prove_conv_route(route, name, cfg, rows, splitk):
    """The kernels the route is about ran in the captured forward (profile rows "class.sSTAGE@family" -> launches)."""
    cls = lambda c: sum(n for r, n in rows.items() if r.split("@")[0].split(".")[0] == c)
    fam = lambda c, f: sum(n for r, n in rows.items() if r.split(".")[0] == c and r.endswith("@" + f))
    any8p = sum(n for r, n in rows.items() if r.endswith("@gemm8p"))
    k32 = max(cfg.cross_embed_kernel_sizes[0]) == 32
    if route == "conv_plain":
        assert all(rows.get(f"gemm_embed.s{s}") == 2 for s in (1, 2, 3)) and any8p == 0 and splitk == 0, (rows, splitk)
        assert cls("embed_patch") == 1 and cls("gn_stats") == 6, rows     # the partials folded by their own launch, twice per UpBlock
    elif route == "default":
        if name in SKIP_EMBED0:     # the 1-degree grid: merged CrossEmbed, split-K with its finish kernel, merged parities
            assert all(rows.get(f"gemm_embed.s{s}") == 1 for s in (1, 2, 3)) and splitk >= 1, (rows, splitk)
            assert TF.decoder_form(cfg) != "convt" or cls("gemm_convT4") == 1, rows
        assert (cls("embed_patch") == 1) if k32 else (rows.get("gemm_embed.s0", 0) >= 3 and cls("embed_patch") == 0), rows
    elif route == "gemm8p":
        assert fam("gemm_conv3", "gemm8p") >= 2 and fam("gemm_convT2", "gemm8p") >= 1, rows
    elif route in ("kb128", "kb64"):
        assert cls("gemm_conv3") == 6 and any8p == 0, rows    # (the K step is a launch parameter of conv_gemm_dma: no row of its own)
    elif route == "no_patch":
        assert rows.get("gemm_embed.s0", 0) >= 4 and cls("embed_patch") == 0, rows
    elif route == "no_planar":
        assert cls("embed_patch") == 1, rows


def _conv_case(route, name, prec):
    cfg, sd, eng = _engine(name, prec, CONV_ROUTES[route])
    x = torch.from_numpy(synth_input(cfg)).cuda()
    y0, y2, caps, rows, splitk = _captured_conv_forward(eng, cfg, x)
    del eng     # the engine's device memory goes with it: the references below run on the CPU
    assert torch.equal(y0, y2), f"{route} {name} {prec}: capture level 2 changed the forward (max {float((y0 - y2).abs().max()):.3e})"
    _prove_conv_route(route, name, cfg, rows, splitk)
    links = TF.build_conv_links(cfg, sd, caps, prec, skip_embed0=name in SKIP_EMBED0)
    assert len(links) == len(TF.conv_link_specs(cfg, name in SKIP_EMBED0)) >= 4 + 3 * 5 + 2 - (name in SKIP_EMBED0), [k.kind for k in links]
    return cfg, links, splitk


@pytest.mark.parametrize("route,name", CONV_CASES, ids=["-".join(c) for c in CONV_CASES])
def test_bf16_conv_links_teacher_forced(route, name):
    """CrossEmbed, UpBlock, head and tail links of the bf16 engine (teacher_forced.build_conv_links), one engine per case.

    Routes: conv_plain (the 128 x 128 implicit GEMM only; the reference measurement b_conv), default, gemm8p (the eight-phase kernel's
    conv and ConvTranspose-k2 forms from one row), kb128 / kb64 (128- / 64-byte K steps of conv_gemm_dma), no_patch (stage-0 CrossEmbed on
    the implicit GEMM), no_planar (the patch kernel on the pixel-major input).  conv_plain is held to 1.25 x b_conv, every other route to
    2 x b_conv; the tail, fp32 out of a stored map on every engine, to 1e-4 of max_row|ref| per pixel.

    Measured on MI355X (worst d over the links of each engine: kind -> capture, channel, pixel; teacher_forced.B_PLAIN_CONV records b_conv):
      conv_plain  T0  0.0085  head -> up_block4, 1, 1854          T1  0.0088  c2 -> up_block3.c2, 23, 1349
                  T0W 0.0141  head -> up_block4, 14, 785          T0U 0.0119  head -> up_block4, 14, 392
                  T5  0.0090  embed -> layers.0.0, 92, 2355       -> b_conv(base) = 0.0141; gates 0.0176 / 0.0282
      default     T0 0.0087  T1 0.0088  T0X 0.0096  T0F 0.0105  T0M 0.0085  T0W 0.0141  T0U 0.0117  RT 0.0206 (head, 7, 58603)  T5 0.0090
                  C1 0.0090  C1W 0.0156 (head, 7, 852)
      gemm8p      T5 0.0090  C1 0.0088        kb128 T5 0.0090     kb64 T5 0.0090     no_patch T1 0.0088     no_planar T1 0.0088
      tail        1.0e-7 - 1.4e-7 of max_row|ref| on every engine (RT: 0, its resize is the identity)
      fp32        T1 5.2e-6  T0W 5.1e-6  T0U 4.0e-6;   fp32s  T1 1.2e-5  T0W 1.4e-5  T0U 1.1e-5  C1 1.2e-5   (tolerance 1e-4)
    b_conv is set by the `head` link of the PixelShuffle / upsample decoders, which the table of links defines from the concatenated map
    to up_block4 -- two launches with a stored, rounded map between them (head_ps / head_us and head_fin judge the two on their own:
    0.0089 / 0.0000 and 0.0130 at most).  The worst link of ONE launch is 0.0097 (sharp, C1W), 0.0090 on the conv_plain engines; both
    GroupNorm links stay within one ulp of the stored output everywhere (d = 0).  The gate found no kernel at fault: the CPU stand-in of
    test_teacher_forced_cpu needs 0.0144 (the same two-launch head), its weakest mutant reaches 0.079.  The engine refused no
    environment of the table."""
    cfg, links, splitk = _conv_case(route, name, "bf16")
    b_conv = TF.B_PLAIN_CONV["base"]
    gate = (TF.PLAIN_FACTOR if route == "conv_plain" else TF.ROUTE_FACTOR) * b_conv
    tail = [k for k in links if k.kind == "tail"]
    assert len(tail) == 1
    e_tail, tok = TF.fp32_row_excess(tail[0])
    res = [TF.link_distance(k, TF.A_BF16) for k in links if k.kind != "tail"]
    by_kind = {}
    for r in res:
        if r.d >= by_kind.get(r.kind, r).d:
            by_kind[r.kind] = r
    w = max(res, key=lambda r: r.d)
    print(f"[teacher-forced conv] {route} {name}: {len(links)} links, split-K launches {splitk}, worst d {w.d:.4f} ({w.kind} -> {w.out}, channel {w.channel}, "
          f"pixel {w.token}); gate {gate:.4f}; tail {e_tail:.2e}; per kind " + ", ".join(f"{k} {r.d:.4f}" for k, r in sorted(by_kind.items())))
    assert TF.ROUTE_FACTOR * b_conv <= TF.B_CEIL
    assert e_tail <= TF.FP32_TOL, f"{route} {name} tail: |got - ref| = {e_tail:.3e} of the row's max|ref| at pixel {tok}"
    bad = [r for r in res if not r.d <= gate]
    assert not bad, f"{route} {name}: {len(bad)} link(s) over d = {gate:.4f}: " + "; ".join(
        f"{r.kind} -> {r.out} d {r.d:.4f} at channel {r.channel}, pixel {r.token}" for r in bad[:8])


@pytest.mark.parametrize("prec,name", FP32_CONV_CASES, ids=["-".join(c) for c in FP32_CONV_CASES])
def test_fp32_conv_links_teacher_forced(prec, name):
    """The same links of the fp32 and split-bf16 engines on their default routes, held per pixel row to |got - ref| <= 1e-4 max_row|ref|."""
    cfg, links, _ = _conv_case("default", name, prec)
    worst = (0.0, None, 0)
    for k in links:
        e, tok = TF.fp32_row_excess(k)
        worst = max(worst, (e, k.kind + " -> " + k.out, tok))
        assert e <= TF.FP32_TOL, f"{prec} {name} {k.kind} -> {k.out}: |got - ref| = {e:.3e} of the row's max|ref| at pixel {tok}"
    print(f"[teacher-forced conv] {prec} {name} default: {len(links)} links, worst row error {worst[0]:.3e} of max_row|ref| ({worst[1]}, pixel {worst[2]}; "
          f"tolerance {TF.FP32_TOL:.0e})")
