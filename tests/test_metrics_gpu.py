"""The verification metrics on the device (csrc/wx_metrics.h through wxengine/metrics.py) against the reference's goldens
(tests/golden/metrics_*.npz): every score of every variable and every aggregate, at every call, under the project's gate
(hybrid_cases.gate): against the fp32 golden max(4 d_ref, 2e-6), against the fp64 golden max(5 d_ref, 2e-6), d_ref being the
reference's own fp32-against-fp64 distance of the same score, stored in the fixture; the distance and its scales are those of
tests/metrics_cases.py.  On the pressure field of sp2d a float32 raw-moment kernel misses that gate by a factor of ten to 1e5
(tests/test_metrics_oracle.py).

Then the bit-exact properties (a second object and a second call, untouched inputs, submit(...).result() against __call__, 34
variables in two calls against 34 calls of one), inputs read in place from channel-slice views on a side stream -- at the cases' odd
widths bit for bit, and on a 32 x 64 crop at an aligned and a one-float-shifted offset, where the 16-byte and the scalar loads are
both held to the restatement --, the rejections at call, the statuses and messages of the C ABI, and one composed three-step
run_forecast on the T0 model whose `consume` scores every step with `submit`."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import metrics_cases as MC  # noqa: E402
import metrics_oracle as MO  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
cuda = lambda a: torch.from_numpy(a).cuda()      # noqa: E731


def make_metric(case, inp, **kw):
    from wxengine.metrics import CombinedMetric
    args = MC.block_args(case, inp)
    args.update(kw)
    return CombinedMetric(**args)


@pytest.fixture(scope="module")
def runs():
    """Per case: inputs, their state dicts on the GPU, goldens, the metric object and its outputs per call (computed once, shared)."""
    out, shared = {}, {}
    for case, c in MC.METRICS_CASES.items():
        g, keys, f32, f64, d_ref, scale = MC.load_golden(case, GOLD)
        if c["inputs"] not in shared:
            inp = MC.case_inputs(c["inputs"], check=g)
            shared[c["inputs"]] = (inp, [MC.state_dicts(inp, call, cuda) for call in range(len(inp["pred"]))])
        inp, fulls = shared[c["inputs"]]
        m = make_metric(case, inp)
        got = [m(full) for full in fulls]
        out[case] = dict(inp=inp, fulls=fulls, keys=keys, f32=f32, f64=f64, d_ref=d_ref, scale=scale, metric=m, got=got)
    return out


@pytest.mark.parametrize("case", list(MC.METRICS_CASES))
def test_every_score_and_aggregate_vs_reference_goldens(runs, case):
    r = runs[case]
    bad, worst = [], (0.0, 0.0)
    for call, got in enumerate(r["got"]):
        assert list(got) == r["keys"], case
        for i, k in enumerate(r["keys"]):
            assert isinstance(got[k], float) and np.isfinite(got[k]), (case, call, k)
            b32, b64 = MC.gate(r["d_ref"][call, i])
            d32 = MC.distance(got[k], r["f32"][call, i], r["scale"][call, i])
            d64 = MC.distance(got[k], r["f64"][call, i], r["scale"][call, i])
            worst = (max(worst[0], d32 / b32), max(worst[1], d64 / b64))
            if not (d32 <= b32 and d64 <= b64):
                bad.append((call, k, got[k], d32, b32, d64, b64))
    print(f"[metrics gpu] {case}: {len(r['keys'])} keys x {len(r['got'])} calls; worst distance / bound: vs fp32 golden {worst[0]:.3f}, "
          f"vs fp64 golden {worst[1]:.3f}")
    assert not bad, (case, bad[:8])
    for name in r["metric"].metric_names:            # last_var_scores per metric: the last call's per-variable floats
        assert r["metric"].last_var_scores[name] == {k.split("/", 1)[1]: v for k, v in r["got"][-1].items() if k.startswith(name + "/")}


@pytest.mark.parametrize("case", list(MC.METRICS_CASES))
def test_bit_exact_properties(runs, case):
    r = runs[case]
    keep = [{s: {k: v.clone() for k, v in full[s][MC.SRC].items()} for s in full} for full in r["fulls"]]
    again, pending = make_metric(case, r["inp"]), make_metric(case, r["inp"])
    for call, full in enumerate(r["fulls"]):
        assert again(full) == r["got"][call], (case, call)                      # a second object: the same bits
        p = pending.submit(full)
        assert p.result() == r["got"][call] and p.result() is p.result() and p.done(), (case, call)
    if len(r["fulls"]) == 1 or not r["metric"].accumulate_climatology:
        assert r["metric"](r["fulls"][-1]) == r["got"][-1], case                # a second call of the first object
    for full, kept in zip(r["fulls"], keep):
        for s in full:
            for k, v in full[s][MC.SRC].items():
                assert torch.equal(v, kept[s][k]), (case, s, k)                 # the inputs are never modified


def test_34_variables_in_two_calls_equal_34_calls_of_one(runs):
    r = runs["many"]
    full = r["fulls"][0]
    assert len(full["y_processed"][MC.SRC]) == 34
    for name in MC.INPUTS["many"]["vars"]:
        k = MC.KEYS[name]
        one = make_metric("many", r["inp"], data_var_keys=[k], include_computed_diagnostics=False, var_weighting="none")(full)
        for m in MC.METRICS_CASES["many"]["metrics"]:
            assert one[f"{m}/{k}"] == r["got"][0][f"{m}/{k}"], (m, k)


def _as_views(full, shift, crop=None):
    """The variables of both state dicts as channel slices of ONE [B, C, T, H, W] tensor each (with B = 2 the batch items of a view
    are not adjacent) that starts 4 + shift floats into its buffer.  Variables with another n_time get a tensor of their own."""
    out, flats = {}, []
    for s in full:
        groups = {}
        for k, v in full[s][MC.SRC].items():
            v = v if crop is None else v[..., :crop[0], :crop[1]]
            groups.setdefault(v.shape[2], []).append((k, v))
        out[s] = {MC.SRC: {}}
        for items in groups.values():
            B, _, T, H, W = items[0][1].shape
            C_all = 1 + sum(v.shape[1] for _, v in items)
            n = B * C_all * T * H * W
            flat = torch.full((n + 8,), 7.0, device="cuda")
            big = flat[4 + shift:4 + shift + n].view(B, C_all, T, H, W)
            assert (big.data_ptr() % 16 == 0) == (shift == 0)
            c0 = 1
            for k, v in items:
                big[:, c0:c0 + v.shape[1]] = v
                out[s][MC.SRC][k] = big[:, c0:c0 + v.shape[1]]
                c0 += v.shape[1]
            flats.append(flat)
    return out, flats


@pytest.mark.parametrize("case", ["sp2d", "b2t2", "wide"])
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "unaligned"])
def test_channel_slice_views_on_a_side_stream_give_the_same_bits(runs, case, shift):
    """W is odd (or no multiple of 4) in these cases: scalar loads either way, so the result is the contiguous tensors' bit for bit."""
    r = runs[case]
    views, flats = _as_views(r["fulls"][0], shift)
    keep = [f.clone() for f in flats]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = make_metric(case, r["inp"])(views)
    side.synchronize()
    assert got == r["got"][0], case
    assert all(torch.equal(f, k) for f, k in zip(flats, keep))        # the inputs and the guard values around them are untouched


@pytest.mark.parametrize("case", ["lev16", "b2t2"])
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "unaligned"])
def test_16_byte_and_scalar_loads_on_a_32_x_64_crop(runs, case, shift):
    """W = 64: aligned views take the 16-byte loads, the one-float-shifted ones the scalar loads.  Both are held to the restatement on
    the same tensors under the gate, d_ref being the restatement's own fp32-against-fp64 distance."""
    r = runs[case]
    H, W = 32, 64
    inp = dict(r["inp"], lat=MC.latitude(H), clim={k: np.ascontiguousarray(v[..., :H, :W]) for k, v in r["inp"]["clim"].items()})
    views, flats = _as_views(r["fulls"][0], shift, crop=(H, W))
    keep = [f.clone() for f in flats]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = make_metric(case, inp)(views)
    side.synchronize()
    assert all(torch.equal(f, k) for f, k in zip(flats, keep))
    cpu = {s: {MC.SRC: {k: v.cpu().contiguous() for k, v in views[s][MC.SRC].items()}} for s in views}
    m32 = MO.Restatement(dtype=torch.float32, **MC.block_args(case, inp))
    m64 = MO.Restatement(dtype=torch.float64, **MC.block_args(case, inp))
    w32 = m32(cpu)
    w64 = m64({s: {MC.SRC: {k: v.double() for k, v in cpu[s][MC.SRC].items()}} for s in cpu}, all_scores=True)
    sc = MC.scales(m64.last_all_scores, m64.weights, m64.var_keys)
    assert list(got) == list(w64)
    worst = 0.0
    for k in got:
        b32, b64 = MC.gate(MC.distance(w32[k], w64[k], sc[k]))
        d32, d64 = MC.distance(got[k], w32[k], sc[k]), MC.distance(got[k], w64[k], sc[k])
        worst = max(worst, d32 / b32, d64 / b64)
        assert d32 <= b32 and d64 <= b64, (case, shift, k, got[k], w32[k], w64[k], d32, b32, d64, b64)
    print(f"[metrics gpu] {case} 32 x 64 crop, shift {shift}: worst distance / bound {worst:.3f}")


def test_274_tiles_of_one_variable_take_the_finish_kernel_round_its_loop_twice():
    """The finish launch adds a variable's tiles 256 at a time; the fixtures stop at 137 (`deep` in `many`).  137 levels x B = 2 on
    7 x 19 is 274 tiles, one row block per plane.  All eight scores, with a per-level climatology and latitude weights, are held to
    the restatement on the same tensors under the gate, d_ref being the restatement's own fp32-against-fp64 distance."""
    from wxengine.metrics import CombinedMetric
    H, W, L, B = 7, 19, 137, 2
    g = np.random.Generator(np.random.Philox(key=[2029, 274]))
    c, t, p = MC._field("T", g, (L, 1, H, W), (B, L, 1, H, W))
    key = MC.KEYS["deep"]
    clim = {key: np.ascontiguousarray(c.astype(np.float32).reshape(L, H, W))}
    kw = dict(metrics={m: ({"climatology": clim} if m in ("acc", "activity") else {}) for m in MC.ALL8}, var_weighting="none",
              use_latitude_weights=True, latitude=MC.latitude(H))
    cpu = {"y_processed": {MC.SRC: {key: torch.from_numpy(p.astype(np.float32))}},
           "y_target_processed": {MC.SRC: {key: torch.from_numpy(t.astype(np.float32))}}}
    got = CombinedMetric(**kw)({s: {MC.SRC: {k: v.cuda() for k, v in cpu[s][MC.SRC].items()}} for s in cpu})
    m32, m64 = MO.Restatement(dtype=torch.float32, **kw), MO.Restatement(dtype=torch.float64, **kw)
    w32 = m32(cpu)
    w64 = m64({s: {MC.SRC: {k: v.double() for k, v in cpu[s][MC.SRC].items()}} for s in cpu}, all_scores=True)
    sc = MC.scales(m64.last_all_scores, m64.weights, m64.var_keys)
    assert list(got) == list(w64) and {f"{m}/{key}" for m in MC.ALL8} <= set(got)
    worst = 0.0
    for k in got:
        b32, b64 = MC.gate(MC.distance(w32[k], w64[k], sc[k]))
        d32, d64 = MC.distance(got[k], w32[k], sc[k]), MC.distance(got[k], w64[k], sc[k])
        worst = max(worst, d32 / b32, d64 / b64)
        assert d32 <= b32 and d64 <= b64, (k, got[k], w32[k], w64[k], d32, b32, d64, b64)
    print(f"[metrics gpu] 274 tiles of one variable: worst distance / bound {worst:.3f}")


def test_rejections_at_call_carry_their_reason(runs):
    from wxengine.engine import WXEngineError
    r = runs["sp2d"]
    full = r["fulls"][0]
    key = MC.KEYS["sp"]

    def swapped(side, t):
        return dict(full, **{side: {MC.SRC: dict(full[side][MC.SRC], **{key: t})}})
    sp = full["y_processed"][MC.SRC][key]
    with pytest.raises(WXEngineError, match="on the GPU"):
        make_metric("sp2d", r["inp"])(swapped("y_processed", sp.cpu()))
    with pytest.raises(WXEngineError, match="must be one \\[B, n_levels, n_time, H, W\\] shape"):
        make_metric("sp2d", r["inp"])(swapped("y_processed", sp[:, :, 0]))
    with pytest.raises(WXEngineError, match="must be one \\[B, n_levels, n_time, H, W\\] shape"):
        make_metric("sp2d", r["inp"])(swapped("y_target_processed", sp[..., :30].contiguous()))
    with pytest.raises(ValueError, match="33 latitudes but the fields have 7 rows; latitude-sharded scoring \\(lat-band mode\\) is out of scope"):
        make_metric("sp2d", r["inp"])(runs["many"]["fulls"][0])
    # float64 and float16 inputs and a target on the host are converted and moved, as the reference's .float() / .to() do
    got = make_metric("sp2d", r["inp"])({"y_processed": {MC.SRC: {k: v.double() for k, v in full["y_processed"][MC.SRC].items()}},
                                         "y_target_processed": {MC.SRC: {k: v.cpu() for k, v in full["y_target_processed"][MC.SRC].items()}}})
    assert got == r["got"][0]


def test_c_abi_statuses_and_messages(runs):
    from wxengine.engine import _f32, load_library
    r = runs["sp2d"]
    lib = load_library()
    full = r["fulls"][0]
    p, t = full["y_processed"][MC.SRC][MC.KEYS["sp"]], full["y_target_processed"][MC.SRC][MC.KEYS["sp"]]
    H, W = p.shape[3:]
    w = MO.lat_weights(r["inp"]["lat"]).numpy()
    scores = torch.zeros(1, 8, device="cuda")
    one = lambda x: (C.c_void_p * 1)(x.data_ptr())      # noqa: E731
    z64, l1 = (C.c_int64 * 1)(0), (C.c_int32 * 1)(1)
    sc = C.c_void_p(scores.data_ptr())
    ok = lambda h: (h, 1, one(p), z64, one(t), z64, None, None, None, l1, l1, 1, 1e-12, sc, None)      # noqa: E731
    assert lib.wx_metrics_apply(*ok(None)) == -1 and b"null metrics handle" in lib.wx_last_error()
    assert lib.wx_metrics_destroy(None) == 0
    h = C.c_void_p()
    assert lib.wx_metrics_create(H, W, _f32(w), 0, None) == -1 and b"null argument" in lib.wx_last_error()
    assert lib.wx_metrics_create(0, W, _f32(w), 0, C.byref(h)) == -1 and b"bad geometry" in lib.wx_last_error()
    assert lib.wx_metrics_create(H, 0, None, 0, C.byref(h)) == -1 and b"bad geometry" in lib.wx_last_error()
    bad = w.copy()
    bad[5] = np.nan
    assert lib.wx_metrics_create(H, W, _f32(bad), 0, C.byref(h)) == -1 and b"non-finite latitude weight at row 5" in lib.wx_last_error()
    assert lib.wx_metrics_create(H, W, _f32(w), 99, C.byref(h)) == -1 and b"no such GPU device" in lib.wx_last_error()
    assert not h.value
    assert lib.wx_metrics_create(H, W, _f32(w), 0, C.byref(h)) == 0, lib.wx_last_error()
    for i in (2, 3, 4, 5, 9, 10, 13):          # pred, its strides, target, its strides, n_levels, n_time, scores
        a = list(ok(h))
        a[i] = None
        assert lib.wx_metrics_apply(*a) == -1 and b"null argument" in lib.wx_last_error(), i
    null1 = (C.c_void_p * 1)(None)
    a = list(ok(h)); a[2] = null1      # noqa: E702
    assert lib.wx_metrics_apply(*a) == -1 and b"null tensor pointer" in lib.wx_last_error()
    a = list(ok(h)); a[4] = null1      # noqa: E702
    assert lib.wx_metrics_apply(*a) == -1 and b"null tensor pointer" in lib.wx_last_error()
    a = list(ok(h)); a[6] = one(t)      # noqa: E702  a climatology without its stride arrays
    assert lib.wx_metrics_apply(*a) == -1 and b"null argument" in lib.wx_last_error()
    for n in (0, 33):
        a = list(ok(h)); a[1] = n      # noqa: E702
        assert lib.wx_metrics_apply(*a) == -1 and b"1..32 variables" in lib.wx_last_error()
    a = list(ok(h)); a[11] = 0      # noqa: E702
    assert lib.wx_metrics_apply(*a) == -1 and b"B >= 1" in lib.wx_last_error()
    a = list(ok(h)); a[9] = (C.c_int32 * 1)(0)      # noqa: E702
    assert lib.wx_metrics_apply(*a) == -1 and b"n_levels and n_time must be >= 1" in lib.wx_last_error()
    assert lib.wx_metrics_apply(*ok(h)) == 0, lib.wx_last_error()
    torch.cuda.synchronize()
    row = scores[0].cpu().numpy()
    key = MC.KEYS["sp"]
    for j, m in enumerate(MC.ALL8[:6]):
        assert float(row[j]) == r["got"][0][f"{m}/{key}"], m
    assert np.isnan(row[6]) and np.isnan(row[7])          # no climatology: NaN in the last two slots
    # a null entry among climatology pointers: that variable alone goes without
    c = cuda(r["inp"]["clim"]["sp"])
    two = lambda x, y: (C.c_void_p * 2)(x.data_ptr(), y.data_ptr())      # noqa: E731
    s2 = torch.zeros(2, 8, device="cuda")
    clim2 = (C.c_void_p * 2)(c.data_ptr(), None)
    z2, l2 = (C.c_int64 * 2)(0, 0), (C.c_int32 * 2)(1, 1)
    assert lib.wx_metrics_apply(h, 2, two(p, p), z2, two(t, t), z2, clim2, z2, z2, l2, l2, 1, 1e-12, C.c_void_p(s2.data_ptr()), None) == 0
    torch.cuda.synchronize()
    s2 = s2.cpu().numpy()
    assert float(s2[0, 6]) == r["got"][0][f"acc/{key}"] and float(s2[0, 7]) == r["got"][0][f"activity/{key}"]
    assert np.isnan(s2[1, 6:]).all() and np.array_equal(s2[1, :6], s2[0, :6]) and np.array_equal(s2[0, :6], row[:6])
    assert lib.wx_metrics_destroy(h) == 0


def test_composed_three_step_forecast_scores_every_step_with_submit():
    """run_forecast on the T0 synthetic model with [InverseScale]; `consume` builds y_target_processed from synthetic targets and calls
    submit -- no host sync inside the loop.  After the loop the three results are held to the restatement on the same tensors under
    the gate, d_ref being the restatement's own fp32-against-fp64 distance."""
    from synth_batches import gen2loop_batches, gen2loop_schema
    from wxengine.config import named_config
    from wxengine.forecast import InverseScale, run_forecast
    from wxengine.metrics import CombinedMetric, PendingScores
    from wxengine.model import WXFormerHIP
    from wxengine.synth import synth_state_dict
    cfg = named_config("T0")
    sd = synth_state_dict(cfg)
    ic, frcs, mean, std = gen2loop_batches(cfg, 3)
    _, out = gen2loop_schema(cfg)
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
    cu = lambda b: {"input": {s: {k: v.cuda() for k, v in d.items()} for s, d in b["input"].items()}}  # noqa: E731
    H = cfg.image_height
    kw = dict(metrics={m: {} for m in MC.ALL8}, var_weighting="none", use_latitude_weights=True, latitude=MC.latitude(H))
    metric = CombinedMetric(**kw)
    gen = torch.Generator(device="cuda").manual_seed(11)
    pendings, kept = [], []

    def consume(yp, step):
        target = {src: {k: v + 0.25 * v.abs().mean() * torch.randn(v.shape, device="cuda", generator=gen) for k, v in d.items()}
                  for src, d in yp.items()}
        p = metric.submit({"y_processed": yp, "y_target_processed": target})
        assert isinstance(p, PendingScores)
        pendings.append(p)
        kept.append(({s: dict(d) for s, d in yp.items()}, target))
    run_forecast(model, cu(ic), [cu(f) for f in frcs], 3, cmap, mean, std, [InverseScale(mean, std)], consume)
    assert len(pendings) == 3
    m32, m64 = MO.Restatement(dtype=torch.float32, **kw), MO.Restatement(dtype=torch.float64, **kw)
    for step, (p, (yp, target)) in enumerate(zip(pendings, kept)):
        got = p.result()
        cpu = lambda d, dt: {s: {k: v.cpu().to(dt) for k, v in x.items()} for s, x in d.items()}      # noqa: E731
        w32 = m32({"y_processed": cpu(yp, torch.float32), "y_target_processed": cpu(target, torch.float32)})
        w64 = m64({"y_processed": cpu(yp, torch.float64), "y_target_processed": cpu(target, torch.float64)}, all_scores=True)
        sc = MC.scales(m64.last_all_scores, m64.weights, m64.var_keys)
        assert list(got) == list(w64)
        worst = 0.0
        for k in got:
            b32, b64 = MC.gate(MC.distance(w32[k], w64[k], sc[k]))
            d32, d64 = MC.distance(got[k], w32[k], sc[k]), MC.distance(got[k], w64[k], sc[k])
            worst = max(worst, d32 / b32, d64 / b64)
            assert d32 <= b32 and d64 <= b64, (step, k, got[k], w32[k], w64[k])
        print(f"[metrics gpu] forecast step {step + 1}: {len(got)} keys, worst distance / bound {worst:.3f}")
