"""The wind artifact filter on the device (csrc/wx_wind.h through wxengine/wind_filter.py) against the reference's goldens
(tests/golden/wind_*.npz): the blend mask and EVERY filtered plane of every case under the gate of tests/diag_cases.gate (against the
fp32 golden max(4 d_ref, 2e-6), against the fp64 golden 5 d_ref, d_ref being the reference's own fp32-against-fp64 distance stored in
the fixture), the bit-exact properties (pass-through levels, a calm field, points with m == 0, repeated calls, untouched inputs), inputs
read in place from channel-slice views at aligned and unaligned offsets and on a side stream, the skipped level with its single
warning, the rejections with their reasons, and one composed three-step run_forecast against the tests/wind_oracle.py chain.

Measured on MI355X, worst of the six non-trivial cases, d_ref -> device against the fp32 golden / against the fp64 golden: mask 5.9e-7 ->
6.6e-7 / 1.8e-7; U 3.9e-7 -> 4.4e-7 / 2.4e-7; V 5.6e-7 -> 6.7e-7 / 2.4e-7; T 4.2e-7 -> 5.1e-7 / 2.1e-7.  The tightest fp64 bound is tiny's T
(6.2e-7; the device is at 8.9e-8).  In calm every output equals its input bit for bit.  Every output is inside the gate; the file runs in
under 3 s."""
import ctypes as C
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import wind_oracle as O  # noqa: E402
from diag_cases import distance, gate  # noqa: E402
from wind_cases import KEYS, SRC, WIND_CASES, case_inputs, filtered_levels, filtered_planes, load_golden, output_names  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def make_block(name, **kw):
    from wxengine.wind_filter import WindArtifactFilter
    c = WIND_CASES[name]
    args = dict(c["args"], return_mask=True)
    args.update(kw)
    return WindArtifactFilter(u_var=KEYS["U"], v_var=KEYS["V"], target_vars=[KEYS[v] for v in c["targets"]], **args)


def batch_of(t):
    return {"y_processed": {SRC: {KEYS[v]: t[v] for v in t}}}


@pytest.fixture(scope="module")
def runs():
    """Per case: inputs on the GPU, goldens, and the block's outputs and mask (computed once, shared, never modified)."""
    out = {}
    for name in WIND_CASES:
        g, f32, f64, d_ref = load_golden(name, GOLD)
        inp = case_inputs(name, check=g)
        t = {v: torch.from_numpy(inp[v]).cuda() for v in inp}
        blk = make_block(name)
        y = blk(batch_of(t))["y_processed"][SRC]
        torch.cuda.synchronize()
        out[name] = dict(inp=inp, t=t, f32=f32, f64=f64, d_ref=d_ref, blk=blk, mask=blk.last_mask,
                         y={v: y[KEYS[v]] for v in WIND_CASES[name]["targets"]})
    return out


@pytest.mark.parametrize("name", list(WIND_CASES))
def test_mask_and_every_filtered_plane_vs_reference_goldens(runs, name):
    r = runs[name]
    got = {v: filtered_planes(name, v, r["y"][v]).cpu().numpy() for v in WIND_CASES[name]["targets"]}
    got["mask"] = r["mask"].cpu().numpy()
    bad = []
    for v in output_names(name):
        assert got[v].shape == r["f32"][v].shape, (name, v, got[v].shape)
        if name == "calm":      # nothing flagged: m is exactly 0 and every plane keeps its bits
            assert np.array_equal(got[v], r["f32"][v]), (name, v)
            continue
        b32, b64 = gate(r["d_ref"][v])
        d32, d64 = distance(got[v], r["f32"][v]), distance(got[v], r["f64"][v])
        print(f"[wind gpu] {name} {v}: d_ref {r['d_ref'][v]:.2e}; vs fp32 golden {d32:.2e} (<= {b32:.2e}), vs fp64 golden {d64:.2e} (<= {b64:.2e})")
        if not (np.isfinite(got[v]).all() and d32 <= b32 and d64 <= b64):
            bad.append((v, d32, b32, d64, b64))
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", list(WIND_CASES))
def test_bit_exact_properties(runs, name):
    r = runs[name]
    c = WIND_CASES[name]
    lv = filtered_levels(name)
    keep = {v: r["t"][v].clone() for v in r["t"]}
    again = make_block(name)(batch_of(r["t"]))["y_processed"][SRC]       # a second object, a second call: the same bits
    twice = r["blk"](batch_of(r["t"]))["y_processed"][SRC]
    untouched = (r["mask"] == 0).expand(c["B"], len(lv), c["H"], c["W"])
    n_zero = int((r["mask"] == 0).sum())
    if name == "calm":
        assert n_zero == r["mask"].numel()
    elif name != "tiny":      # (7 x 19 lies inside the falloff of its jet everywhere)
        assert 0 < n_zero < r["mask"].numel()
    for v in c["targets"]:
        y, t = r["y"][v], r["t"][v]
        assert y.shape == t.shape and y.is_contiguous() and y.data_ptr() != t.data_ptr()
        assert torch.equal(again[KEYS[v]], y) and torch.equal(twice[KEYS[v]], y), (name, v)
        for l in range(c["L"]):
            if l not in lv:
                assert torch.equal(y[:, l], t[:, l]), (name, v, l)           # pass-through levels
        yf, tf = filtered_planes(name, v, y), filtered_planes(name, v, t)
        assert torch.equal(yf[untouched], tf[untouched]), (name, v)          # m == 0: the input's bits
        if name == "calm":
            assert torch.equal(y, t)
        else:
            assert not torch.equal(yf, tf)
    assert torch.equal(r["blk"].last_mask, r["mask"])
    for v in r["t"]:
        assert torch.equal(r["t"][v], keep[v]), (name, v)                    # the inputs are never modified


@pytest.mark.parametrize("name", ["cam48", "b2odd", "tiny", "multi"])
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "unaligned"])
def test_channel_slice_views_and_a_side_stream(runs, name, shift):
    """The variables as Reconstruct hands them out: channel slices of one [B, C, 1, H, W] tensor (with B = 2 the batch items of a view
    are not adjacent).  shift 1 starts that tensor one float into its buffer, so no plane sits on 16 bytes even where H * W % 4 == 0."""
    r = runs[name]
    c, t = WIND_CASES[name], runs[name]["t"]
    order = ("T", "U", "V")
    C_all = 1 + 3 * c["L"]
    n = c["B"] * C_all * c["H"] * c["W"]
    flat = torch.full((n + 4,), 7.0, device="cuda")
    big = flat[shift:shift + n].view(c["B"], C_all, 1, c["H"], c["W"])
    views, c0 = {}, 1
    for v in order:
        big[:, c0:c0 + c["L"]] = t[v]
        views[v] = big[:, c0:c0 + c["L"]]
        c0 += c["L"]
    if c["H"] * c["W"] % 4 == 0:
        assert all((views[v].data_ptr() % 16 == 0) == (shift == 0) for v in order)
    keep = flat.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        blk = make_block(name)
        y = blk(batch_of(views))["y_processed"][SRC]
    side.synchronize()
    assert torch.equal(blk.last_mask, r["mask"])
    for v in c["targets"]:
        assert torch.equal(y[KEYS[v]], r["y"][v]), (name, v)
    assert torch.equal(flat, keep)


def test_skipped_level_keeps_the_shape_and_warns_once_per_variable(runs, caplog):
    r = runs["cam48"]
    blk = make_block("cam48")
    with caplog.at_level(logging.WARNING, logger="wxengine.wind_filter"):
        for _ in range(2):
            y = blk(batch_of(r["t"]))["y_processed"][SRC]
    warned = [rec.getMessage() for rec in caplog.records if "exceed available levels" in rec.getMessage()]
    assert len(warned) == 3 and all("[7]" in w and "(5)" in w for w in warned)
    assert sorted(w.split("'")[1] for w in warned) == sorted(KEYS[v] for v in ("U", "V", "T"))
    for v in ("U", "V", "T"):
        assert y[KEYS[v]].shape == r["t"][v].shape and torch.equal(y[KEYS[v]], r["y"][v])


def test_without_the_mask_option_the_results_are_the_same_bits(runs):
    r = runs["b2odd"]
    blk = make_block("b2odd", return_mask=False)
    y = blk(batch_of(r["t"]))["y_processed"][SRC]
    assert blk.last_mask is None
    for v in WIND_CASES["b2odd"]["targets"]:
        assert torch.equal(y[KEYS[v]], r["y"][v])


def test_rejections_at_call_carry_their_reason(runs):
    from wxengine.engine import WXEngineError, load_library
    r = runs["cam48"]
    t = r["t"]
    with pytest.raises(WXEngineError, match="mask_level 5 is beyond the 5 levels"):
        make_block("cam48", mask_level=5)(batch_of(t))
    with pytest.raises(WXEngineError, match="must be a float32"):
        make_block("cam48")(batch_of(dict(t, T=t["T"].double())))
    with pytest.raises(WXEngineError, match="on the GPU"):
        make_block("cam48")(batch_of(dict(t, V=t["V"].cpu())))
    with pytest.raises(WXEngineError, match="H x W must agree"):
        make_block("cam48")(batch_of(dict(t, T=t["T"][..., :40].contiguous())))
    with pytest.raises(WXEngineError, match="does not match"):
        make_block("cam48")(batch_of(dict(t, V=t["V"][..., :24, :].contiguous())))
    # the C ABI: a null handle or pointer is an error status with its reason, not a crash
    lib = load_library()
    one, one64, lv = (C.c_void_p * 1)(t["U"].data_ptr()), (C.c_int64 * 1)(0), (C.c_int32 * 1)(5)
    out = torch.empty_like(t["U"])
    dst = (C.c_void_p * 1)(out.data_ptr())
    assert lib.wx_wind_apply(None, t["U"].data_ptr(), 0, t["V"].data_ptr(), 0, 1, one, one64, lv, dst, None, 0, 1, None, None) == -1
    assert b"null wind-filter handle" in lib.wx_last_error()
    assert lib.wx_wind_destroy(None) == 0
    k = np.array([0.25, 0.5, 0.25], np.float32)
    kp = k.ctypes.data_as(C.POINTER(C.c_float))
    h = C.c_void_p()
    assert lib.wx_wind_create(48, 72, kp, 3, kp, 3, kp, 3, kp, 3, 5, 12, 2.8, 0, 0, C.byref(h)) == -1 and b"must be odd" in lib.wx_last_error()
    assert lib.wx_wind_create(48, 72, kp, 3, kp, 3, kp, 3, None, 3, 5, 13, 2.8, 0, 0, C.byref(h)) == -1 and b"null falloff longitude" in lib.wx_last_error()
    assert lib.wx_wind_create(48, 72, kp, 3, kp, 2, kp, 3, kp, 3, 5, 13, 2.8, 0, 0, C.byref(h)) == -1 and b"smoothing longitude kernel size 2" in lib.wx_last_error()
    assert lib.wx_wind_create(48, 72, kp, 3, kp, 3, kp, 3, kp, 3, 5, 13, 2.8, 0, 0, None) == -1
    assert not h.value
    assert lib.wx_wind_create(48, 72, kp, 3, kp, 3, kp, 3, kp, 3, 5, 13, 2.8, 0, 0, C.byref(h)) == 0, lib.wx_last_error()
    assert lib.wx_wind_apply(h, None, 0, t["V"].data_ptr(), 0, 1, one, one64, lv, dst, None, 0, 1, None, None) == -1 and b"null" in lib.wx_last_error()
    null1 = (C.c_void_p * 1)(None)
    assert lib.wx_wind_apply(h, t["U"].data_ptr(), 0, t["V"].data_ptr(), 0, 1, null1, one64, lv, dst, None, 0, 1, None, None) == -1
    assert b"null tensor pointer" in lib.wx_last_error()
    assert lib.wx_wind_apply(h, t["U"].data_ptr(), 0, t["V"].data_ptr(), 0, 33, one, one64, lv, dst, None, 0, 1, None, None) == -1
    assert b"1..32 variables" in lib.wx_last_error()
    assert lib.wx_wind_destroy(h) == 0


def test_composed_three_step_forecast_equals_the_oracle_chain():
    """run_forecast with a stand-in model that returns fixed tensors and the chain [WindArtifactFilter, InverseScale] -- the filter in
    front of the inverse scale, on normalised values, as the shipped config runs it.  Against the tests/wind_oracle.py chain followed by
    t * std + mean on the CPU; the gate is the project's, with d_ref = the oracle's own fp32-against-fp64 distance per variable."""
    from wxengine.forecast import InverseScale, run_forecast
    from wxengine.wind_filter import WindArtifactFilter
    c = WIND_CASES["cam48"]
    L, H, W = c["L"], c["H"], c["W"]
    order = ("U", "V", "T")
    a, b = case_inputs("cam48"), case_inputs("dflt48")
    steps = [a, b, {v: np.ascontiguousarray(a[v][:, ::-1]) for v in a}]     # level 2, the mask level, stays where it is
    y_preds = [torch.from_numpy(np.concatenate([s[v] for v in order], axis=1)).cuda() for s in steps]    # [1, 3 L, 1, H, W]
    calls = []

    def model(x):
        calls.append(tuple(x.shape))
        return y_preds[len(calls) - 1]
    cmap = {KEYS[v]: {"slice": slice(i * L, (i + 1) * L), "orig_shape": (L, 1)} for i, v in enumerate(order)}
    mean = {v: (np.arange(L, dtype=np.float32) * 0.7 + 1.0 + i) for i, v in enumerate(order)}
    std = {v: (np.arange(L, dtype=np.float32) * 0.3 + 2.0 + i) for i, v in enumerate(order)}
    ic = {"input": {SRC: {KEYS[v]: torch.from_numpy(a[v]).cuda() for v in order}}}
    args = dict(c["args"])
    blk = WindArtifactFilter(u_var=KEYS["U"], v_var=KEYS["V"], target_vars=[KEYS[v] for v in order], **args)
    seen = []

    def consume(yp, step):
        fields = {KEYS[v]: torch.from_numpy(steps[step - 1][v]) for v in order}
        want = {}
        for dtype in (torch.float32, torch.float64):
            o, _ = O.wind_filter(fields, KEYS["U"], KEYS["V"], [KEYS[v] for v in order], args, dtype)
            want[dtype] = {v: (o[KEYS[v]] * torch.from_numpy(std[v]).to(dtype).reshape(1, -1, 1, 1, 1)
                               + torch.from_numpy(mean[v]).to(dtype).reshape(1, -1, 1, 1, 1)).numpy() for v in order}
        for v in order:
            got = yp[SRC][KEYS[v]].cpu().numpy()
            assert got.shape == (1, L, 1, H, W)
            d_ref = distance(want[torch.float32][v], want[torch.float64][v])
            b32, b64 = gate(d_ref)
            d32, d64 = distance(got, want[torch.float32][v]), distance(got, want[torch.float64][v])
            print(f"[wind gpu] forecast step {step} {v}: d_ref {d_ref:.2e}; vs fp32 oracle {d32:.2e} (<= {b32:.2e}), vs fp64 oracle {d64:.2e} (<= {b64:.2e})")
            assert d32 <= b32 and d64 <= b64, (step, v, d32, b32, d64, b64)
        seen.append(step)
    run_forecast(model, ic, [{"input": {}}, {"input": {}}], 3, cmap, mean, std, [blk, InverseScale(mean, std)], consume)
    assert seen == [1, 2, 3] and len(calls) == 3
    for yp, s in zip(y_preds, steps):      # y_pred itself was read in place and never written
        assert torch.equal(yp.cpu(), torch.from_numpy(np.concatenate([s[v] for v in order], axis=1)))
