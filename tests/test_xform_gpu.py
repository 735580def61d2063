"""The gen-2 variable transforms on the device (csrc/wx_pre.h pre_xform_kernel and csrc/wx_unxform.h through wxengine/transforms.py)
against the reference's goldens (tests/golden/xform_*.npz): the fused input pass and the fused output launch per variable and level
under the gate of tests/diag_cases.gate -- max(4 d_ref, 2e-6) against the fp32 golden, 5 d_ref against the fp64 golden, NaN positions
coinciding exactly --, the chain of single post blocks and repeated applies bit-identical to them, y_pred untouched, untouched
variables and `transforms=[]` bit-identical to the plain kernel, tensors that start on 4-byte boundaries, the ABI refusals, and one
3-step run_forecast with a log on a 3-D and a 2-D variable whose every step is gated against tests/xform_oracle.py.
Every value of every fixture is compared.

Measured on MI355X, worst variable per case, d_ref -> device against the fp32 golden / against the fp64 golden.  Input side: arco ln SP
3.5e-6 -> 0 / 3.5e-6 (every logged or filled variable equals the fp32 golden bit for bit); b2t2 2.4e-7 -> 0 / 2.4e-7; sqrt 8.8e-8 -> 8.6e-8 /
8.8e-8; al16 8.5e-8 -> 0 / 8.5e-8; f64 5.1e-8 -> 5.7e-8 / 1.1e-7.  Output side: arco q 9.0e-7 -> 9.4e-8 / 9.0e-7; b2t2 q 2.2e-7 -> 9.7e-8 /
2.4e-7; sqrt 1.8e-7 -> 0 / 2.0e-7; al16 q 6.0e-7 -> 9.6e-8 / 7.3e-7; f64 1.5e-7 -> 1.0e-7 / 2.3e-7.  Forecast, steps 1 - 3: ln sp input 1.4e-4 ->
1.6e-4 / 1.4e-4, then 8.7e-5 -> 0 / 8.7e-5 and 8.9e-5 -> 0 / 8.9e-5; q output 6.5e-7 .. 6.9e-7 -> 9.0e-8 .. 9.5e-8 / <= 6.9e-7.  Every variable and level
is inside the gate.  With the device logf instead of the double-precision logarithm the fixtures passed as well, but the forecast's ln sp
input of steps 2 - 3 came to 5.4e-4 against its gate of 3.5e-4 (a 1-ulp miss of logf where the true value lies on a float32): see
csrc/wx_pre.h xform_forward."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import xform_oracle as O  # noqa: E402
from diag_cases import gate  # noqa: E402
from xform_cases import (SRC, XFORM_CASES, batch_input, case_inputs, case_stats, level_distance, load_golden, out_variables, post_blocks,  # noqa: E402
                         pre_blocks, target_channel_map)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))   # NaN == NaN here


def variable_slices(pre):
    out, cur = {}, 0
    for k, nl in zip(pre.keys, pre.levels):
        out[k] = slice(cur, cur + nl)
        cur += nl
    return out


def reconstructed(name, y_pred):
    from wxengine.reconstruct import Reconstruct
    return Reconstruct()({"y_pred": y_pred, "metadata": {"target": {"_channel_map": target_channel_map(name)}}})


def check_gates(tag, got, f32, f64, d_ref):
    """-> list of (tag, level, d32, b32, d64, b64) outside the gate; prints every figure."""
    d32, d64, bad = level_distance(got, f32), level_distance(got, f64), []
    for l in range(len(d32)):
        b32, b64 = gate(d_ref[l])
        if not (d32[l] <= b32 and d64[l] <= b64):
            bad.append((tag, l, d32[l], b32, d64[l], b64))
    w = int(np.argmax(d32))
    print(f"[xform gpu] {tag}: worst level {w}: d_ref {d_ref[w]:.2e}; vs fp32 golden {d32[w]:.2e} (<= {gate(d_ref[w])[0]:.2e}), "
          f"vs fp64 golden {d64[w]:.2e} (<= {gate(d_ref[w])[1]:.2e}); max over levels vs fp64 {d64.max():.2e}")
    return bad


@pytest.fixture(scope="module")
def runs():
    """Per case: inputs on the GPU, goldens, the fused input pass and the fused output launch (computed once, shared, never modified)."""
    import wxengine.transforms as X
    from wxengine.preblock import DevicePreblock
    out = {}
    for name in XFORM_CASES:
        g, f32, f64, d_ref = load_golden(name, GOLD)
        fields, y_pred = case_inputs(name, check=g)
        mean, std = case_stats(name)
        inp = batch_input(name, fields, lambda a: torch.from_numpy(a).cuda())
        pre = DevicePreblock(inp, mean, std, transforms=pre_blocks(name, X))
        x = pre(inp)
        y = torch.from_numpy(y_pred).cuda()
        keep = y.clone()
        fused = X.InverseTransforms(mean, std, post_blocks(name, X))
        yp = fused(reconstructed(name, y))["y_processed"][SRC]
        torch.cuda.synchronize()
        out[name] = dict(f32=f32, f64=f64, d_ref=d_ref, inp=inp, pre=pre, x=x, y=y, keep=keep, fused=fused, yp=yp, mean=mean, std=std)
    return out


@pytest.mark.parametrize("name", list(XFORM_CASES))
def test_input_side_vs_reference_goldens(runs, name):
    r = runs[name]
    c = XFORM_CASES[name]
    assert tuple(r["x"].shape[:3]) == (c["B"], sum(v["levels"] for v in c["variables"]), c["T"])
    sl, bad = variable_slices(r["pre"]), []
    for v in c["variables"]:
        k = f"pre:{v['name']}"
        bad += check_gates(f"{name} {k}", r["x"][:, sl[v["key"]]].cpu().numpy(), r["f32"][k], r["f64"][k], r["d_ref"][k])
    assert not bad, bad


@pytest.mark.parametrize("name", list(XFORM_CASES))
def test_output_side_vs_reference_goldens(runs, name):
    r, bad = runs[name], []
    for v in out_variables(name):
        k = f"post:{v['name']}"
        got = r["yp"][v["key"]]
        assert got.is_contiguous() or (v["stats"] is None and v["xf"] is None)          # a fresh tensor, unless passed through
        bad += check_gates(f"{name} {k}", got.cpu().numpy(), r["f32"][k], r["f64"][k], r["d_ref"][k])
    assert not bad, bad
    assert same_bits(r["y"], r["keep"])                                                 # y_pred is never modified


@pytest.mark.parametrize("name", list(XFORM_CASES))
def test_chain_of_single_post_blocks_is_bit_identical_to_the_fused_launch(runs, name):
    import wxengine.transforms as X
    from wxengine.forecast import InverseScale
    r = runs[name]
    full = reconstructed(name, r["y"])
    views = dict(full["y_processed"][SRC])
    for blk in [InverseScale(r["mean"], r["std"])] + post_blocks(name, X):
        full = blk(full)
    for v in out_variables(name):
        assert same_bits(full["y_processed"][SRC][v["key"]], r["yp"][v["key"]]), (name, v["name"])
    assert same_bits(r["y"], r["keep"])
    again = r["fused"](reconstructed(name, r["y"]))["y_processed"][SRC]                 # a repeated apply
    for v in out_variables(name):
        assert same_bits(again[v["key"]], r["yp"][v["key"]]), (name, v["name"])
        if v["stats"] is None and v["xf"] is None:                                      # pass-through: the view itself, untouched
            assert again[v["key"]].data_ptr() == views[v["key"]].data_ptr() and same_bits(again[v["key"]], views[v["key"]])
        else:
            assert again[v["key"]].data_ptr() != views[v["key"]].data_ptr()


@pytest.mark.parametrize("name", list(XFORM_CASES))
def test_untouched_variables_and_repeats_are_bit_identical_to_the_plain_kernel(runs, name):
    from wxengine.preblock import DevicePreblock
    r = runs[name]
    plain = DevicePreblock(r["inp"], r["mean"], r["std"])
    assert plain.transform_table is None and r["pre"].transform_table is not None
    xp = plain(r["inp"])
    sl = variable_slices(plain)
    assert plain.keys == r["pre"].keys and plain.channel_map == r["pre"].channel_map
    n_untouched = 0
    for v in XFORM_CASES[name]["variables"]:
        if not v["fills"] and v["xf"] is None:
            n_untouched += 1
            assert same_bits(xp[:, sl[v["key"]]], r["x"][:, sl[v["key"]]]), (name, v["name"])
        else:
            assert not same_bits(xp[:, sl[v["key"]]], r["x"][:, sl[v["key"]]]), (name, v["name"])
    assert n_untouched or name in ("al16",)
    assert same_bits(r["pre"](r["inp"]), r["x"])                                         # a repeated apply
    empty = DevicePreblock(r["inp"], r["mean"], r["std"], transforms=[])
    assert empty.transform_table is None and same_bits(empty(r["inp"]), xp)             # transforms=[] is the plain block


@pytest.mark.parametrize("name", ["al16", "sqrt", "arco"])
def test_tensors_that_start_on_4_byte_boundaries(runs, name):
    """hw % 4 == 0 does not make a plane 16-byte aligned: fields and y_pred that begin one float into their storage (and, at B = 2, the
    channel-slice views of such a y_pred) must give the same bits as the aligned ones -- on the fused input pass, the plain input
    pass and the output launch."""
    from wxengine.preblock import DevicePreblock
    r = runs[name]

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        s = buf[1:].view(t.shape)
        s.copy_(t)
        assert s.data_ptr() % 16 == 4 and s.is_contiguous()
        return s
    inp = {SRC: {k: shifted(t) for k, t in r["inp"][SRC].items()}}
    assert same_bits(r["pre"](inp), r["x"])
    plain = DevicePreblock(r["inp"], r["mean"], r["std"])
    assert plain.transform_table is None and same_bits(plain(inp), plain(r["inp"]))
    y = shifted(r["y"])
    yp = r["fused"](reconstructed(name, y))["y_processed"][SRC]
    for v in out_variables(name):
        assert same_bits(yp[v["key"]], r["yp"][v["key"]]), (name, v["name"])
    assert same_bits(y, r["keep"])


def test_abi_refusals_return_a_status_and_a_reason(runs):
    from wxengine.engine import load_library
    lib = load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    F = lambda *a: (C.c_float * len(a))(*a)        # noqa: E731
    I = lambda *a: (C.c_int32 * len(a))(*a)        # noqa: E731
    pre = C.c_void_p()
    assert lib.wx_pre_create(2, I(1, 1), 1, 4, 4, None, None, 0, C.byref(pre)) == 0
    ok = dict(kind=I(1, 0), eps=F(1e-8, 1.0), log_eps=F(-18.4, 0.0), n_rules=I(1, 0), rule_op=I(*([0] * 16)), rule_search=F(*([0.0] * 16)),
              rule_fill=F(*([0.0] * 16)))
    order = ("kind", "eps", "log_eps", "n_rules", "rule_op", "rule_search", "rule_fill")

    def set_tf(handle=pre, **kw):
        a = dict(ok, **kw)
        return lib.wx_pre_set_transforms(handle, *[a[k] for k in order]), lib.wx_last_error().decode()
    assert set_tf()[0] == 0
    for kw, reason in ((dict(kind=I(5, 0)), "unknown transform kind"), (dict(kind=I(0, -1)), "unknown transform kind"),
                       (dict(n_rules=I(9, 0)), "0 .. 8 fill rules"), (dict(n_rules=I(0, -1)), "0 .. 8 fill rules"),
                       (dict(eps=F(0.0, 1.0)), "eps > 0"), (dict(eps=F(-1e-8, 1.0)), "eps > 0"), (dict(eps=F(float("nan"), 1.0)), "eps > 0"),
                       (dict(rule_op=I(7, *([0] * 15))), "unknown fill rule op")):
        status, msg = set_tf(**kw)
        assert status == -1 and reason in msg, (kw, status, msg)
    for k in order:
        status, msg = set_tf(**{k: None})
        assert status == -1 and "null argument" in msg, (k, status, msg)
    status, msg = set_tf(handle=None)
    assert status == -1 and "null pre-block handle" in msg
    assert lib.wx_pre_destroy(pre) == 0

    u = C.c_void_p()
    okc = dict(n_vars=2, n_levels=I(1, 2), H=4, W=4, kind=I(1, 4), eps=F(1e-8, 1.0), log_eps=F(-18.4, 0.0), has_stats=I(1, 0), mean=F(0.0, 0.0, 0.0),
               std=F(1.0, 1.0, 1.0))
    corder = ("n_vars", "n_levels", "H", "W", "kind", "eps", "log_eps", "has_stats", "mean", "std")

    def create(**kw):
        a = dict(okc, **kw)
        return lib.wx_unxform_create(*[a[k] for k in corder], 0, C.byref(u)), lib.wx_last_error().decode()
    for kw, reason in ((dict(kind=I(5, 0)), "unknown transform kind"), (dict(eps=F(0.0, 1.0)), "eps > 0"), (dict(n_vars=65), "1..64 variables"),
                       (dict(n_vars=0), "1..64 variables"), (dict(n_levels=I(1, 0)), "at least one level"), (dict(H=0), "bad geometry"),
                       (dict(mean=None), "mean / std are null"), (dict(kind=None), "null argument"), (dict(n_levels=None), "null argument"),
                       (dict(has_stats=None), "null argument")):
        status, msg = create(**kw)
        assert status == -1 and reason in msg and not u.value, (kw, status, msg)
    assert lib.wx_unxform_create(*[okc[k] for k in corder], 0, None) == -1
    assert create()[0] == 0 and u.value
    t = torch.zeros(1, 3, 1, 4, 4, device="cuda")
    src, dst, bs = (C.c_void_p * 2)(t.data_ptr(), t.data_ptr()), (C.c_void_p * 2)(t.data_ptr(), t.data_ptr()), (C.c_int64 * 2)(0, 0)
    for args, reason in (((None, bs, dst, 1, 1), "null argument"), ((src, None, dst, 1, 1), "null argument"), ((src, bs, None, 1, 1), "null argument"),
                         ((src, bs, dst, 0, 1), "must be >= 1"), ((src, bs, dst, 1, 0), "must be >= 1"),
                         (((C.c_void_p * 2)(t.data_ptr(), None), bs, dst, 1, 1), "null tensor pointer")):
        status = lib.wx_unxform_apply(u, *args, None)
        assert status == -1 and reason in lib.wx_last_error().decode(), (reason, status, lib.wx_last_error().decode())
    assert lib.wx_unxform_apply(None, src, bs, dst, 1, 1, None) == -1
    assert lib.wx_unxform_destroy(u) == 0


def test_plane_limit_on_the_plain_pass():
    """One plane per (batch, channel, frame) in the launch's y dimension: 65535 planes run (one field of 65535 levels on a 1 x 1 grid,
    no statistics: a copy, bit for bit), 65536 are refused with a reason before anything is launched -- as on the fused pass."""
    from wxengine.engine import load_library
    lib = load_library()
    src = torch.randn(65536, generator=torch.Generator().manual_seed(7)).cuda()
    for n in (65535, 65536):
        pre = C.c_void_p()
        assert lib.wx_pre_create(1, (C.c_int32 * 1)(n), 1, 1, 1, None, None, 0, C.byref(pre)) == 0
        x = torch.full((n,), float("nan"), device="cuda")
        status = lib.wx_pre_apply(pre, (C.c_void_p * 1)(src.data_ptr()), C.c_void_p(x.data_ptr()), 1, None)
        torch.cuda.synchronize()
        if n == 65535:
            assert status == 0, lib.wx_last_error().decode()
            assert same_bits(x, src[:n])
        else:
            assert status == -1 and "exceeds 65535 planes" in lib.wx_last_error().decode(), (status, lib.wx_last_error().decode())
            assert bool(torch.isnan(x).all())                                           # nothing was launched
        assert lib.wx_pre_destroy(pre) == 0


def test_host_refusals_on_the_device_objects(runs):
    import wxengine.transforms as X
    from wxengine.engine import WXEngineError
    r = runs["b2t2"]
    Q = "era5/prognostic/3d/Q"
    with pytest.raises(ValueError, match="second exp / square"):
        X.InverseTransforms(r["mean"], r["std"], [X.ExpTransform([Q]), X.SquareTransform([])])(reconstructed("b2t2", r["y"]))
    with pytest.raises(ValueError, match="works on"):
        X.InverseTransforms(r["mean"], r["std"], [X.ExpTransform([Q], key="y_target_processed")])
    full = reconstructed("b2t2", r["y"])
    full["y_processed"][SRC][Q] = full["y_processed"][SRC][Q].transpose(3, 4).contiguous().transpose(3, 4)
    with pytest.raises(WXEngineError, match="contiguous"):
        X.SquareTransform([Q])(full)


def test_three_step_forecast_with_a_log_on_a_3d_and_a_2d_variable():
    """run_forecast on T0 (fp32): natural log of Q (3-D) and s0 (2-D, surface pressure) on the way in, exp on the way out, then the
    geopotential diagnostic on the physical q and surface pressure.  At EVERY step the pairs y_pred -> y_processed and x_physical -> x are
    gated against tests/xform_oracle.py run on the captured tensors: d_ref is the oracle's own fp32-against-fp64 distance per variable
    and level, the gate diag_cases.gate(d_ref).  No gate on the accumulated trajectory."""
    import wxengine.transforms as X
    from diag_cases import hybrid_coefficients
    from synth_batches import gen2loop_batches, gen2loop_schema
    from wxengine.config import named_config
    from wxengine.diagnostics import GeopotentialDiagnostic
    from wxengine.forecast import run_forecast
    from wxengine.model import WXFormerHIP
    from wxengine.synth import synth_state_dict
    cfg = named_config("T0")
    sd = synth_state_dict(cfg)
    ic, frcs, _, _ = gen2loop_batches(cfg, 3)
    inp, out = gen2loop_schema(cfg)
    L, P = cfg.levels, "era5/prognostic/"
    QK, SK = P + "3d/Q", P + "2d/s0"
    # statistics of the quantities the model sees: Q and s0 in log space (ln(q / 1e-8 + 1) ~ 13, ln(sp / 1e-8 + 1) ~ 29.8), T in kelvin
    stats = {"T": (250.0, 4.0), "Q": (13.0, 0.15), "U": (0.0, 8.0), "V": (0.0, 8.0), "s0": (29.83, 0.003), "s1": (280.0, 4.0), "Z": (6000.0, 800.0)}
    mean = {k.split("/")[-1]: np.full(nl, stats.get(k.split("/")[-1], (0.3, 1.5))[0], np.float32) for k, nl in inp[:-2]}
    std = {k.split("/")[-1]: np.full(nl, stats.get(k.split("/")[-1], (0.3, 1.5))[1], np.float32) for k, nl in inp[:-2]}
    mean.update({f"d{i}": np.float32(0.1 * i) for i in range(cfg.output_only_channels)})
    std.update({f"d{i}": np.float32(2.0 + i) for i in range(cfg.output_only_channels)})
    for k, v in ic["input"]["era5"].items():       # the IC in physical units; q and the surface pressure positive
        n = k.split("/")[-1]
        z = (v - 0.3) / 1.5
        if n == "Q":
            ic["input"]["era5"][k] = 4.5e-3 * (1.0 + 0.12 * z).clamp(min=0.2)
        elif n == "s0":
            ic["input"]["era5"][k] = 9.0e4 * (1.0 + 0.003 * z)
        elif n in stats:
            ic["input"]["era5"][k] = z * stats[n][1] + stats[n][0]
    cmap, cur = {}, 0
    for k, nl in out:
        cmap[k] = {"slice": slice(cur, cur + nl), "orig_shape": (nl, 1)}
        cur += nl
    mc = dict(image_height=37, image_width=72, frames=1, channels=4, surface_channels=4, input_only_channels=4,
              output_only_channels=3, levels=3, dim=[32, 64, 128, 256], depth=[1, 1, 2, 1],
              global_window_size=[4, 2, 2, 1], local_window_size=3,
              cross_embed_kernel_sizes=[[4, 8, 16, 32], [2, 4], [2, 4], [2, 4]], cross_embed_strides=[2, 2, 2, 2],
              padding_conf=dict(activate=True, mode="earth", pad_lat=[6, 6], pad_lon=[12, 12]), post_conf=dict(activate=False))
    model = WXFormerHIP(precision="fp32", **mc).to("cuda").eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    a_half, b_half, _, _ = hybrid_coefficients(L)
    zkey = "era5/derived_diagnostic/3d/geopotential"
    captured = []

    def capture(full):      # a post block: sees this step's input pair and output pair
        captured.append(dict(x_physical={k: v.clone() for k, v in full["x_physical"]["era5"].items()}, x=full["x"].clone(),
                             y_pred=full["y_pred"].clone(), y_processed={k: v.clone() for k, v in full["y_processed"]["era5"].items()}))
        return full
    pre_tf = [X.LogTransform([QK, SK], data_types=["input"])]
    chain = [X.InverseTransforms(mean, std, [X.ExpTransform([QK, SK])]), capture,
             GeopotentialDiagnostic(output_name=zkey, specific_humidity_var=QK, temperature_var=P + "3d/T", surface_pressure_var=SK,
                                    surface_geopotential_var="era5/static/2d/Z", model_a_half=a_half, model_b_half=b_half)]
    cu = lambda b: {"input": {s: {k: v.cuda() for k, v in d.items()} for s, d in b["input"].items()}}  # noqa: E731
    seen = []

    def consume(yp, step):
        assert tuple(yp["era5"][zkey].shape) == (1, L, 1, cfg.image_height, cfg.image_width)
        assert bool(torch.isfinite(yp["era5"][zkey]).all()), step                        # physical q and sp reached the diagnostic
        seen.append(step)
    run_forecast(model, cu(ic), [cu(f) for f in frcs], 3, cmap, mean, std, chain, consume, pre_transforms=pre_tf)
    assert seen == [1, 2, 3] and len(captured) == 3
    xf = {QK: ("log", "e", 1e-8), SK: ("log", "e", 1e-8)}
    bad = []
    for step, cap in enumerate(captured, 1):
        fields = {"era5": {k: v.cpu().numpy() for k, v in cap["x_physical"].items()}}
        o32, o64 = (O.pre_variables(pre_tf, fields, mean, std, dt) for dt in (torch.float32, torch.float64))
        c0 = 0
        from wxengine.preblock import ordered_keys
        for k in ordered_keys(fields):
            nl = fields["era5"][k].shape[1]
            a32, a64 = o32[k].numpy(), o64[k].numpy()
            bad += check_gates(f"step {step} x {k}", cap["x"][:, c0:c0 + nl].cpu().numpy(), a32, a64, level_distance(a32, a64))
            c0 += nl
        y = cap["y_pred"].cpu().numpy()
        p32, p64 = (O.post_named(y, cmap, mean, std, xf, dt) for dt in (torch.float32, torch.float64))
        for k in cmap:
            a32, a64 = p32[k].numpy(), p64[k].numpy()
            bad += check_gates(f"step {step} y {k}", cap["y_processed"][k].cpu().numpy(), a32, a64, level_distance(a32, a64))
        assert float(cap["y_processed"][QK].min()) > 0 and 5e4 < float(cap["y_processed"][SK].mean()) < 2e5, step   # physical units
    assert not bad, bad
