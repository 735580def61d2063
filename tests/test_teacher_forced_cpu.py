"""The teacher-forced per-element gate (tests/teacher_forced.py) sees what the suite's norm gates miss -- shown without a GPU.

"Engine" here is a stand-in: the oracle's FeedForward with bf16-rounded operand, weights, hidden tensor and output, in fp32
arithmetic (what a bf16 kernel with fp32 accumulation computes, up to summation order).  On the FeedForward links of stages 1 - 3 of
T1 (800 / 200 / 50 tokens) and C1 (5760 / 1440 / 360 tokens) -- inputs = the oracle's own stream, rounded to bf16 -- it must pass the
bf16 gate the GPU test holds the fused routes to, and three faults of the kind a tile kernel produces must not:

  chunk   the last 8 tokens of the map lose one 32-wide chunk of the hidden dimension (a ragged last tile that skips a K step)
  b2      the last token loses b2 on the channel with the largest |b2| (an epilogue that drops the bias on its last row)
  stats   the last 16 tokens are normalised with the LayerNorm statistics of the token 16 before them (partials of the wrong row)

Each mutant's rel-L2 over the sub-block's output is printed next to its d: with base weights most of them sit under the 2e-2 the
per-block norm gates allow for the sub-block's own output (that is the record of why this gate exists, not an assertion about the
older tests).

The convolutional links (CrossEmbed, UpBlocks, head, tail: teacher_forced.build_conv_links) get the same treatment on T0, T1 and
the two other decoder forms of T0's geometry (T0W PixelShuffle, T0U upsample + conv).  Stand-in: the oracle's function of the link
with bf16-rounded operand, weights and output in fp32 arithmetic, GroupNorm statistics in fp64; the tail in fp32 from the bf16 map,
not rounded.  Every link is judged on its own: inputs = the oracle's own stream rounded to bf16.  Faults:

  border   3x3 conv (c1, c2): the bottom tap row of the LAST output row reads the map's last row where it should read the zero
           padding below the edge (a halo origin off by one row at the map border)
  chunk    3x3 conv: the last 8 pixels lose 32 input channels of the centre tap (a ragged tile that skips a K step)
  gn_tail  GroupNorm (n1, n2): the statistics leave out the pixels beyond the last full 128-row tile (partials of a ragged tile
           dropped); applied where the map is no multiple of 128 pixels and has at least one full tile.  It moves every pixel, so
           there are no faulty pixels to name
  scatter  ConvTranspose-k2 / PixelShuffle `up` link: dy and dx swapped in the 2 x 2 scatter of the last input column
  lerp     tail: i1 = i0 on the last output row THAT INTERPOLATES.  (On the very last output row the index rule already clamps i1 to
           i0 whenever the map is enlarged -- every configuration here -- so there the fault named in the first place changes nothing.)

The tail is held to FP32_TOL per pixel row (fp32_row_excess), everything else to ROUTE_FACTOR x B_PLAIN_CONV = 0.0282.  Figures: the
stand-in needs d = 0.0089 on T0 and T1, 0.0144 / 0.0117 on T0W / T0U (their `head` link: two launches with a stored map between them),
1.2e-7 on the tail; the weakest mutants reach scatter 3.7, border 1.55, chunk 0.52, gn_tail 0.079 (T1, up_block2: 32 of 800 pixels left
out), lerp 3.8e-2 of max_row|ref| -- at a rel-L2 of the link's output of 1e-2 - 4e-2 for chunk, gn_tail and lerp."""
import math

import pytest
import torch
import torch.nn.functional as F

import teacher_forced as TF
from oracle import wxformer_oracle as O
from wxengine.config import named_config
from wxengine.synth import synth_input, synth_state_dict


def _bf(t):
    return t.float().to(torch.bfloat16).float()


def _standin(x1, sd, p, mutant=None):
    """x1 [1, C, H, W] fp32 holding bf16 values -> bf16-rounded x1 + FF(x1) as fp64, with one of the faults above."""
    f32 = torch.float32
    g, b = O._as_t(sd[p + ".layers.0.g"], f32), O._as_t(sd[p + ".layers.0.b"], f32)
    _, c, h, w = x1.shape
    mean = x1.mean(dim=1, keepdim=True)
    var = ((x1 - mean) ** 2).mean(dim=1, keepdim=True)
    if mutant == "stats":
        m, v = mean.reshape(-1).clone(), var.reshape(-1).clone()
        m[-16:], v[-16:] = mean.reshape(-1)[-32:-16], var.reshape(-1)[-32:-16]
        mean, var = m.reshape(1, 1, h, w), v.reshape(1, 1, h, w)
    xn = _bf((x1 - mean) / torch.sqrt(var + 1e-5) * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1))
    w1, w2 = _bf(O.folded_weight(sd, p + ".layers.1")), _bf(O.folded_weight(sd, p + ".layers.4"))
    b2 = O._bias(sd, p + ".layers.4", f32)
    hid = F.conv2d(xn, w1, O._bias(sd, p + ".layers.1", f32))
    hid = _bf(0.5 * hid * (1 + torch.erf(hid / math.sqrt(2))))
    if mutant == "chunk":
        hid = hid.reshape(1, 4 * c, h * w).clone()
        hid[:, :32, -8:] = 0
        hid = hid.reshape(1, 4 * c, h, w)
    upd = F.conv2d(hid, w2, b2)
    if mutant == "b2":
        ch = int(b2.abs().argmax())
        upd = upd.clone()
        upd[0, ch, -1, -1] -= b2[ch]
    return _bf(x1 + upd).double()


@pytest.fixture(scope="module", params=[("T1", "base"), ("C1", "base"), ("T1", "stress")], ids=lambda p: "-".join(p))
def ff_links(request):
    """(config, family, [(name, x1 fp32 [bf16 values], fp64 reference)]) of the FeedForward sub-blocks of stages 1 - 3."""
    name, fam = request.param
    cfg = named_config(name)
    sd = synth_state_dict(cfg, family=fam)
    cap = TF.encoder_captures(cfg, sd, synth_input(cfg))
    out = []
    for p in TF.pairs(cfg):
        if p.stage == 0:
            continue
        x1 = _bf(cap[p.attn])
        out.append((p.ff, x1, TF.ref_ff(x1.double(), sd, p.ff)))
    assert len(out) == 2 * sum(cfg.depth[1:])
    return name, fam, sd, out


def test_gate_is_recorded_and_under_its_ceiling():
    for fam, b in TF.B_PLAIN.items():
        assert b is not None and 0 < TF.ROUTE_FACTOR * b <= TF.B_CEIL, (fam, b)


def test_standin_passes_and_every_mutant_fails(ff_links):
    name, fam, sd, links = ff_links
    gate = TF.ROUTE_FACTOR * TF.B_PLAIN[fam]
    worst_ok, weakest = 0.0, {}
    for key, x1, ref in links:
        d_ok = TF.link_distance(TF.Link("ff", key, _standin(x1, sd, key), ref, x1.double()), TF.A_BF16)
        worst_ok = max(worst_ok, d_ok.d)
        assert d_ok.d <= gate, f"{name} {fam} {key}: the unmutated stand-in needs d = {d_ok.d:.4f} > {gate:.4f} (channel {d_ok.channel}, token {d_ok.token})"
        # (stress family: LayerNorm gains of 60 make the update ~100 x b2 -- the dropped bias is inside one ulp of the stored output)
        for mut in ("chunk", "b2", "stats") if fam == "base" else ("chunk", "stats"):
            got = _standin(x1, sd, key, mut)
            r = TF.link_distance(TF.Link("ff", key, got, ref, x1.double()), TF.A_BF16)
            l2 = TF.rel_l2(got, ref)
            print(f"[teacher-forced cpu] {name} {fam} {key} C={x1.shape[1]} tokens={x1.shape[2] * x1.shape[3]}: stand-in d {d_ok.d:.4f} | "
                  f"mutant {mut}: d {r.d:.3f} at token {r.token}, rel-L2 of the sub-block output {l2:.2e}")
            assert r.d > gate, f"{name} {fam} {key}: mutant '{mut}' passes the gate (d = {r.d:.4f} <= {gate:.4f})"
            n_tok = x1.shape[2] * x1.shape[3]
            assert r.token >= n_tok - {"chunk": 8, "b2": 1, "stats": 16}[mut], (mut, r.token)   # the gate names the faulty rows
            weakest[mut] = min(weakest.get(mut, math.inf), r.d)
    print(f"[teacher-forced cpu] {name} {fam}: stand-in worst d {worst_ok:.4f} (gate {gate:.4f}); weakest mutants " +
          ", ".join(f"{m} {v:.3f}" for m, v in weakest.items()))


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_links_of_the_oracles_own_stream_are_exact(prec):
    """The references themselves: captures made of the oracle's fp64 functions -- q|k|v with the engine's q scaling of `prec`, the
    attention core on them, to_out, the FeedForward -- must (a) compose to the oracle's own attention() / feedforward() sub-blocks and
    (b) come back from build_links with d = 0 on every kind of link, x_in chained from sub-block to sub-block as the engine chains it."""
    cfg = named_config("T1")
    sd = synth_state_dict(cfg)
    f64 = torch.float64
    q_scale = cfg.dim_head ** -0.5 * math.log2(math.e) if prec == "bf16" else 1.0
    score_scale = math.log(2.0) if prec == "bf16" else cfg.dim_head ** -0.5
    cap = TF.encoder_captures(cfg, sd, synth_input(cfg), f64)
    full, pre = {}, {}
    for p in TF.pairs(cfg):
        x_in = cap[p.x_in]
        c = x_in.shape[1]
        if p.wsz == 1:
            o = TF.ref_qkv(x_in, sd, p.attn, 1.0)[:, 2 * c:]
        else:
            full[p.attn + ".qkv"] = TF.ref_qkv(x_in, sd, p.attn, q_scale)
            o = TF.ref_core(full[p.attn + ".qkv"], sd, p.attn, p.kind, p.wsz, cfg.dim_head, score_scale)
        full[p.attn + ".attn"] = o
        x1 = TF.ref_out(x_in, o, sd, p.attn)
        scale = float(cap[p.attn].abs().max())
        assert float((x1 - cap[p.attn]).abs().max()) <= 1e-12 * scale, p.attn      # qkv -> core -> out == oracle.attention + x
        assert float((TF.ref_ff(x1, sd, p.ff) - cap[p.ff]).abs().max()) <= 1e-12 * scale, p.ff
    for k in list(cap) + list(full):
        full[k] = cap[k] if k in cap else full[k]
    as_np = lambda d: {k: v[0].numpy() for k, v in d.items()}
    n_pairs = 2 * sum(cfg.depth)
    # every capture there: the unfused chain's links
    links = TF.build_links(cfg, sd, as_np(full), prec)
    kinds = [k.kind for k in links]
    assert kinds.count("out") == n_pairs and kinds.count("ff") == n_pairs and kinds.count("core") == kinds.count("qkv") - cfg.depth[3]
    # the sub-block outputs only (attention block kernel, k-blocked chain) / no attention outputs (out-projection deferred)
    links += TF.build_links(cfg, sd, as_np(cap), prec)
    attn_outs = {p.attn for p in TF.pairs(cfg)}
    links += TF.build_links(cfg, sd, as_np({k: v for k, v in full.items() if k not in attn_outs}), prec)
    kinds = [k.kind for k in links]
    assert kinds.count("attn") == n_pairs and kinds.count("out+ff") == n_pairs, kinds
    for k in links:
        assert TF.link_distance(k, 0.0).d <= 1e-10, (k.kind, k.out)
        assert TF.fp32_row_excess(k)[0] <= 1e-12, (k.kind, k.out)


# --------------------------------------------------------------------------- #
# CrossEmbed, decoder, tail
# --------------------------------------------------------------------------- #
F32 = torch.float32
CONV_MUTANTS = {"border": ("c1", "c2"), "chunk": ("c1", "c2"), "gn_tail": ("n1", "n2"), "scatter": ("up",), "lerp": ("tail",)}


def _sd_bf16(sd):
    """The state dict a bf16 engine computes with: every convolution's folded weight rounded to bf16 (biases, GroupNorm affines fp32)."""
    out = {}
    for k, v in sd.items():
        if k.endswith(".weight_orig"):
            out[k[:-5]] = _bf(O.folded_weight(sd, k[:-12])).numpy()
        elif not k.endswith((".weight_u", ".weight_v")):
            t = O._as_t(v, F32)
            out[k] = (_bf(t) if t.dim() == 4 else t).numpy()
    return out


def _axis32(n_in, n_out):
    d = torch.arange(n_out, dtype=F32)
    scale = torch.tensor(n_in, dtype=F32) / torch.tensor(n_out, dtype=F32)
    src = (scale.double() * (d + 0.5).double() - 0.5).float().clamp(min=0.0)     # the oracle's index rule (bilinear_resize)
    i0 = torch.floor(src).long().clamp(max=n_in - 1)
    return i0, (i0 + 1).clamp(max=n_in - 1), src - i0.float()


def _lerp_row(cfg, z):
    """The last output row whose i1 differs from i0 under the correct rule."""
    i0, i1, _ = _axis32(z.shape[-2] - sum(cfg.pad_lat), cfg.image_height)
    return int((i1 != i0).nonzero().max())


def _tail32(cfg, z, mutant=None):
    z = O.earth_unpad(z, cfg.pad_lat, cfg.pad_lon)
    r0, r1, lr = _axis32(z.shape[-2], cfg.image_height)
    c0, c1, lc = _axis32(z.shape[-1], cfg.image_width)
    if mutant == "lerp":
        r1 = r1.clone()
        row = int((r1 != r0).nonzero().max())
        r1[row] = r0[row]
    rows = z[..., r0, :] * (1 - lr).view(-1, 1) + z[..., r1, :] * lr.view(-1, 1)
    return rows[..., c0] * (1 - lc) + rows[..., c1] * lc


def _gn32(x, g, b, groups, res, mutant=None):
    """GroupNorm + SiLU (+ shortcut) on the fp32 map x: statistics in fp64, the rest in fp32."""
    _, c, h, w = x.shape
    m = h * w
    xs = x.double().reshape(1, groups, c // groups, m)
    if mutant == "gn_tail":
        xs = xs[..., : m // 128 * 128]
    mean = xs.mean(dim=(2, 3))
    var = (xs ** 2).mean(dim=(2, 3)) - mean ** 2
    a = (1.0 / torch.sqrt(var + 1e-5)).repeat_interleave(c // groups, dim=1).view(1, c, 1, 1)
    mu = mean.repeat_interleave(c // groups, dim=1).view(1, c, 1, 1)
    y = (x - mu.float()) * a.float() * g.view(1, c, 1, 1) + b.view(1, c, 1, 1)
    y = y * torch.sigmoid(y)
    return y if res is None else y + res


def _conv_standin(cfg, sdb, sp, ins, mutant=None):
    """One link in a bf16 kernel's arithmetic: ins = fp32 tensors holding bf16 values -> the stored output as fp64."""
    form = TF.decoder_form(cfg)
    ub = sp.out.split(".")[0]
    if sp.kind == "tail":
        return _tail32(cfg, ins[0], mutant).double()       # fp32 out of a stored map: not rounded
    if sp.kind in ("n1", "n2"):
        q = ub + (".b.1" if sp.kind == "n1" else ".b.4")
        return _bf(_gn32(ins[0], O._as_t(sdb[q + ".weight"], F32), O._as_t(sdb[q + ".bias"], F32), cfg.dim[0],
                         ins[1] if sp.kind == "n2" else None, mutant)).double()
    if sp.kind == "head" and form != "convt":              # two launches: the shuffled / upsampled map is stored in between
        specs = {k.kind: k for k in TF.conv_link_specs(cfg)}
        mid = _bf(TF.conv_link_fn(cfg, sdb, specs["head_ps" if form == "ps" else "head_us"], ins))
        return _bf(TF.conv_link_fn(cfg, sdb, specs["head_fin"], [mid])).double()
    y = TF.conv_link_fn(cfg, sdb, sp, ins).clone()
    if mutant in ("border", "chunk"):
        x = ins[0]
        wgt = O.folded_weight(sdb, ub + (".b.0" if sp.kind == "c1" else ".b.3"), F32)
        if mutant == "border":
            y[:, :, -1:, :] += F.conv2d(x[:, :, -1:, :], wgt[:, :, 2:3, :], padding=(0, 1))
        else:
            y[0, :, -1, -8:] -= wgt[:, :32, 1, 1] @ x[0, :32, -1, -8:]
    if mutant == "scatter":
        _, c, h2, _ = y.shape
        y[..., -2:] = y[..., -2:].reshape(1, c, h2 // 2, 2, 2).transpose(-1, -2).reshape(1, c, h2, 2)
    return _bf(y).double()


@pytest.fixture(scope="module", params=["T0", "T1", "T0W", "T0U"])
def conv_stream(request):
    """(config, weights, bf16 weights, the oracle's fp32 captures of the whole forward rounded to bf16 -- "y" fp32)."""
    cfg = named_config(request.param)
    sd = synth_state_dict(cfg)
    cap = {}
    O.forward(cfg, sd, synth_input(cfg), capture=cap)
    cap = TF.decoder_captures(cfg, sd, {k: v[:1] for k, v in cap.items()})
    return request.param, cfg, sd, _sd_bf16(sd), {k: _bf(v) for k, v in cap.items()}


def _conv_gate():
    b = TF.B_PLAIN_CONV["base"]
    assert b is not None and 0 < TF.ROUTE_FACTOR * b <= TF.B_CEIL, b
    return TF.ROUTE_FACTOR * b


def _one_link(cfg, sd, sp, ins, got):
    """The link `sp` through build_conv_links, from captures that hold nothing but its inputs and its output."""
    caps = {k: v[0].numpy() for k, v in zip(sp.ins, ins)}
    caps[sp.out] = got[0].numpy()
    links = [k for k in TF.build_conv_links(cfg, sd, caps, "bf16") if k.kind == sp.kind]
    assert len(links) == 1 and links[0].out == sp.out, (sp, [k.kind for k in links])
    return links[0]


def test_conv_gate_is_recorded_and_under_its_ceiling():
    _conv_gate()


def test_conv_standin_passes_and_every_mutant_fails(conv_stream):
    name, cfg, sd, sdb, cap = conv_stream
    gate = _conv_gate()
    worst_ok, worst_tail, weakest, applied = 0.0, 0.0, {}, set()
    for sp in TF.conv_link_specs(cfg):
        ins = [cap[k] for k in sp.ins]
        link = _one_link(cfg, sd, sp, ins, _conv_standin(cfg, sdb, sp, ins))
        _, _, h, w = link.ref.shape
        if sp.kind == "tail":
            e, tok = TF.fp32_row_excess(link)
            worst_tail = max(worst_tail, e)
            assert e <= TF.FP32_TOL, f"{name} tail: the stand-in needs {e:.3e} at pixel {tok}"
        else:
            d_ok = TF.link_distance(link, TF.A_BF16)
            worst_ok = max(worst_ok, d_ok.d)
            assert d_ok.d <= gate, f"{name} {sp.kind} -> {sp.out}: the unmutated stand-in needs d = {d_ok.d:.4f} > {gate:.4f} (channel {d_ok.channel}, pixel {d_ok.token})"
        for mut, kinds in CONV_MUTANTS.items():
            if sp.kind not in kinds:
                continue
            if mut == "gn_tail" and (h * w < 128 or h * w % 128 == 0):
                continue    # no full tile / no ragged one: the fault does not exist on this map
            if mut == "scatter" and TF.decoder_form(cfg) == "upconv":
                continue    # no scatter: its `up` is a 3x3 conv
            bad = _one_link(cfg, sd, sp, ins, _conv_standin(cfg, sdb, sp, ins, mut))
            l2 = TF.rel_l2(bad.got, bad.ref)
            applied.add(mut)
            if mut == "lerp":
                e, tok = TF.fp32_row_excess(bad)
                print(f"[teacher-forced cpu] {name} tail {h}x{w}: stand-in {worst_tail:.2e} | mutant lerp: row error {e:.3e} at pixel {tok} (row {tok // w}), rel-L2 {l2:.2e}")
                assert e > TF.FP32_TOL, f"{name}: mutant 'lerp' passes the tail's tolerance ({e:.3e})"
                assert tok // w == _lerp_row(cfg, ins[0]), (tok, w)
                weakest[mut] = min(weakest.get(mut, math.inf), e)
                continue
            r = TF.link_distance(bad, TF.A_BF16)
            print(f"[teacher-forced cpu] {name} {sp.kind} -> {sp.out} C={bad.ref.shape[1]} {h}x{w}: stand-in d {d_ok.d:.4f} | "
                  f"mutant {mut}: d {r.d:.3f} at pixel {r.token}, rel-L2 of the link's output {l2:.2e}")
            assert r.d > gate, f"{name} {sp.kind} -> {sp.out}: mutant '{mut}' passes the gate (d = {r.d:.4f} <= {gate:.4f})"
            if mut == "border":
                assert r.token >= (h - 1) * w, (mut, r.token)
            elif mut == "chunk":
                assert r.token >= h * w - 8, (mut, r.token)
            elif mut == "scatter":
                assert r.token % w >= w - 2, (mut, r.token)
            weakest[mut] = min(weakest.get(mut, math.inf), r.d)
    want = set(CONV_MUTANTS) - ({"scatter"} if TF.decoder_form(cfg) == "upconv" else set())
    assert applied == want, (applied, want)
    print(f"[teacher-forced cpu] {name} conv links: stand-in worst d {worst_ok:.4f} (gate {gate:.4f}), tail {worst_tail:.2e}; weakest mutants " +
          ", ".join(f"{m} {v:.3g}" for m, v in weakest.items()))


@pytest.mark.parametrize("name", ["T0", "T1", "T0W", "T0U"])
def test_conv_links_of_the_oracles_own_stream_are_exact(name):
    """The references themselves: the decoder rebuilt link by link from the oracle's fp64 functions must (a) compose to the oracle's
    own up_block / up_block_ps, head and forward, and (b) come back from build_conv_links with d = 0 on every link."""
    cfg = named_config(name)
    sd = synth_state_dict(cfg)
    cap = {}
    y = O.forward(cfg, sd, synth_input(cfg), torch.float64, capture=cap)
    cap = {k: v[:1] for k, v in cap.items()}
    dec = TF.decoder_captures(cfg, sd, cap, torch.float64)
    for k in ("up_block1", "up_block2", "up_block3", "up_block4"):
        assert float((dec[k] - cap[k]).abs().max()) <= 1e-12 * float(cap[k].abs().max()), k
    y0 = y[0].reshape(1, -1, y.shape[-2], y.shape[-1])
    assert dec["y"].shape == y0.shape and float((dec["y"] - y0).abs().max()) <= 1e-12 * float(y0.abs().max())
    specs = TF.conv_link_specs(cfg)
    assert set(TF.conv_capture_names(cfg)) >= {k for sp in specs for k in sp.ins + (sp.out,)} - {"y"}
    links = TF.build_conv_links(cfg, sd, {k: v[0].numpy() for k, v in dec.items()}, "bf16")
    assert [k.kind for k in links] == [sp.kind for sp in specs] and len(links) >= 4 + 3 * 5 + 2
    assert len(TF.build_conv_links(cfg, sd, {k: v[0].numpy() for k, v in dec.items()}, "bf16", skip_embed0=True)) == len(links) - 1
    for k in links:
        assert TF.link_distance(k, 0.0).d <= 1e-10, (k.kind, k.out)
        assert TF.fp32_row_excess(k)[0] <= 1e-12, (k.kind, k.out)
