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
older tests)."""
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
