"""The hybrid-level interpolation on the device (csrc/wx_hybrid.h through wxengine/hybrid_interp.py) against the reference's goldens
(tests/golden/hybrid_*.npz): every variable of every case under the gate of tests/hybrid_cases.gate -- against the fp32 golden
max(4 d_ref, 2e-6), against the fp64 golden max(5 d_ref, 2e-6), d_ref being the reference's own fp32-against-fp64 distance of the same
variable, stored in the fixture.  At 127 and 137 levels d_ref of the q-like field is 2e-4 (the reference's fp32 log cancellation, not
slack chosen here), which is why the 16-level cases and the level-index variable `idx` (output = lo + w) are in every run: there the
bound is at or near the 2e-6 floor.

Then the bit-exact properties (a second object and a second call, untouched inputs, fresh contiguous outputs, a constant column, a
level set interpolated onto itself, nine variables in one call against nine calls of one), inputs read in place from channel-slice
views at an aligned and a one-float-shifted offset on a side stream, the surface pressure under another source, absent variables, the
pre block, the rejections with their reasons and the statuses of the C ABI, and one composed three-step run_forecast with
[InverseScale, HybridLevelInterp] against tests/hybrid_oracle.py.  The figures measured on MI355X are in DESIGN.md."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import hybrid_oracle as HO  # noqa: E402
from hybrid_cases import (HYBRID_CASES, KEYS, SRC, block_args, case_inputs, distance, gate, load_golden, midpoints, variables)  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def make_block(name, **kw):
    from wxengine.hybrid_interp import HybridLevelInterp
    args = block_args(name)
    args.update(kw)
    return HybridLevelInterp(**args)


def batch_of(t):
    return {"y_processed": {SRC: {KEYS[v]: t[v] for v in t}}}


def run(blk, t, names):
    y = blk(batch_of(t))["y_processed"][SRC]
    return {v: y[KEYS[v]] for v in names}


@pytest.fixture(scope="module")
def runs():
    """Per case: inputs on the GPU, goldens, and the block's outputs (computed once, shared, never modified)."""
    out = {}
    for name in HYBRID_CASES:
        g, f32, f64, d_ref = load_golden(name, GOLD)
        inp = case_inputs(name, check=g)
        t = {v: torch.from_numpy(inp[v]).cuda() for v in inp}
        blk = make_block(name)
        y = run(blk, t, variables(name))
        torch.cuda.synchronize()
        out[name] = dict(inp=inp, t=t, f32=f32, f64=f64, d_ref=d_ref, blk=blk, y=y)
    return out


@pytest.mark.parametrize("name", list(HYBRID_CASES))
def test_every_variable_vs_reference_goldens(runs, name):
    r = runs[name]
    bad = []
    for v in variables(name):
        got = r["y"][v].cpu().numpy()
        assert got.shape == r["f32"][v].shape and np.isfinite(got).all(), (name, v)
        b32, b64 = gate(r["d_ref"][v])
        d32, d64 = distance(got, r["f32"][v]), distance(got, r["f64"][v])
        print(f"[hybrid gpu] {name} {v}: d_ref {r['d_ref'][v]:.2e}; vs fp32 golden {d32:.2e} (<= {b32:.2e}), "
              f"vs fp64 golden {d64:.2e} (<= {b64:.2e})")
        if not (d32 <= b32 and d64 <= b64):
            bad.append((v, d32, b32, d64, b64))
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", list(HYBRID_CASES))
def test_bit_exact_properties(runs, name):
    r = runs[name]
    vs = variables(name)
    n_dst = midpoints(name)[2].size
    keep = {v: r["t"][v].clone() for v in r["t"]}
    again = run(make_block(name), r["t"], vs)        # a second object, a second call: the same bits
    twice = run(r["blk"], r["t"], vs)
    const = np.float32(0.0031415927)
    flat = dict(r["t"], T=torch.full_like(r["t"]["T"], float(const)))
    level = run(r["blk"], flat, ("T",))["T"]
    for v in vs:
        y, t = r["y"][v], r["t"][v]
        assert y.shape == (t.shape[0], n_dst) + t.shape[2:] and y.dtype == torch.float32 and y.is_contiguous(), (name, v)
        assert torch.equal(again[v], y) and torch.equal(twice[v], y), (name, v)
        assert again[v].data_ptr() != y.data_ptr() and twice[v].data_ptr() != y.data_ptr() and y.data_ptr() != t.data_ptr()
    assert torch.equal(level, torch.full_like(level, float(const))), name      # a constant column: that constant's bits at every level
    for v in r["t"]:
        assert torch.equal(r["t"][v], keep[v]), (name, v)         # the inputs are never modified


@pytest.mark.parametrize("name", ["L16to13", "L13s2t"])
def test_a_level_set_onto_itself_returns_the_input_bits(runs, name):
    """destination == source (the same arrays): w is exactly 0 at every level but the one of highest pressure, where it is exactly 1 and
    y_lo + (y_hi - y_lo) may round: that level is held to the gate, with d_ref from the restatement's own fp32-against-fp64 distance."""
    r = runs[name]
    sa, sb, _, _ = midpoints(name)
    blk = make_block(name, source_a=sa, source_b=sb, source_on_interfaces=False, source_levels=None, dest_a=sa, dest_b=sb,
                     dest_on_interfaces=False, dest_levels=None)
    y = run(blk, r["t"], variables(name))
    last = 0 if HYBRID_CASES[name].get("s2t") else sa.size - 1          # the stored index of the highest pressure
    rest = [k for k in range(sa.size) if k != last]
    want = {}
    for dtype in (torch.float32, torch.float64):
        want[dtype] = HO.interp({v: torch.from_numpy(r["inp"][v]) for v in variables(name)}, torch.from_numpy(r["inp"]["sp"]), sa, sb, sa, sb,
                                dtype=dtype)
    for v in variables(name):
        assert torch.equal(y[v][:, rest], r["t"][v][:, rest]), (name, v)
        w32, w64 = want[torch.float32][v][:, last].numpy(), want[torch.float64][v][:, last].numpy()
        b32, b64 = gate(distance(w32, w64))
        d32, d64 = distance(y[v][:, last].cpu().numpy(), w32), distance(y[v][:, last].cpu().numpy(), w64)
        print(f"[hybrid gpu] {name} onto itself, {v}, highest-pressure level: vs fp32 {d32:.2e} (<= {b32:.2e}), vs fp64 {d64:.2e} (<= {b64:.2e})")
        assert d32 <= b32 and d64 <= b64, (name, v)


def test_nine_variables_in_one_call_equal_nine_calls_of_one(runs):
    r = runs["shuf"]
    fields = HYBRID_CASES["shuf"]["fields"]
    assert len(fields) == 9
    for v in fields:
        one = run(make_block("shuf", variables=[KEYS[v]]), r["t"], (v,))
        assert torch.equal(one[v], r["y"][v]), v


@pytest.mark.parametrize("name", ["L16to13", "L2b2t2", "L13s2t"])
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "unaligned"])
def test_channel_slice_views_and_a_side_stream(runs, name, shift):
    """The variables as Reconstruct hands them out: channel slices of one [B, C, T, H, W] tensor (with B = 2 the batch items of a view
    are not adjacent).  shift 1 starts that tensor one float into its buffer, so no plane sits on 16 bytes."""
    r = runs[name]
    c, t = HYBRID_CASES[name], runs[name]["t"]
    B, T = c["B"], c["T"]
    H, W = t["sp"].shape[3:]
    order = sorted(t)
    C_all = 1 + sum(t[v].shape[1] for v in order)
    n = B * C_all * T * H * W
    flat = torch.full((n + 8,), 7.0, device="cuda")
    big = flat[4 + shift:4 + shift + n].view(B, C_all, T, H, W)
    assert (big.data_ptr() % 16 == 0) == (shift == 0)
    views, c0 = {}, 1
    for v in order:
        nl = t[v].shape[1]
        big[:, c0:c0 + nl] = t[v]
        views[v] = big[:, c0:c0 + nl]
        c0 += nl
    keep = flat.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y = run(make_block(name), views, variables(name))
    side.synchronize()
    for v in variables(name):
        assert torch.equal(y[v], r["y"][v]), (name, v)
    assert torch.equal(flat, keep)            # the inputs and the guard values around them are untouched


def test_surface_pressure_under_another_source_and_absent_variables(runs):
    r = runs["L16to13"]
    t = r["t"]
    sp_key = "ERA5/prognostic/2d/surface_pressure"
    blk = make_block("L16to13", surface_pressure_var=sp_key, variables=[KEYS["T"], f"{SRC}/prognostic/3d/absent", KEYS["idx"]])
    nested = {SRC: {KEYS["T"]: t["T"], KEYS["q"]: t["q"], KEYS["idx"]: t["idx"]}, "ERA5": {sp_key: t["sp"]}}
    blk({"y_processed": nested})
    assert torch.equal(nested[SRC][KEYS["T"]], r["y"]["T"]) and torch.equal(nested[SRC][KEYS["idx"]], r["y"]["idx"])
    assert nested[SRC][KEYS["q"]] is t["q"] and nested["ERA5"][sp_key] is t["sp"] and len(nested[SRC]) == 3
    # none of the variables present: a batch without any surface pressure passes through
    other = {SRC: {KEYS["q"]: t["q"]}}
    make_block("L16to13", variables=[KEYS["T"]])({"y_processed": other})
    assert list(other) == [SRC] and list(other[SRC]) == [KEYS["q"]] and other[SRC][KEYS["q"]] is t["q"]
    make_block("L16to13", variables=[KEYS["T"]])({"y_processed": {}})
    with pytest.raises(KeyError):
        make_block("L16to13")({"y_processed": {SRC: {KEYS["T"]: t["T"]}}})       # a variable present, the surface pressure not


def test_pre_block_interpolates_the_present_data_types_and_leaves_the_callers_dict(runs):
    from wxengine.hybrid_interp import HybridLevelInterpPre
    r = runs["L16to13"]
    nested = {SRC: {KEYS[v]: r["t"][v] for v in r["t"]}}
    batch = {"input": nested, "metadata": {"note": 1}}
    out = HybridLevelInterpPre(**block_args("L16to13"))(batch)
    assert batch["input"] is nested and nested[SRC][KEYS["q"]] is r["t"]["q"] and "target" not in out
    for v in variables("L16to13"):
        assert torch.equal(out["input"][SRC][KEYS[v]], r["y"][v])
    assert out["input"][SRC][KEYS["sp"]] is r["t"]["sp"] and out["metadata"] is batch["metadata"]
    both = HybridLevelInterpPre(data_types=["target"], **block_args("L16to13"))({"input": nested, "target": nested})
    assert both["input"] is nested and torch.equal(both["target"][SRC][KEYS["T"]], r["y"]["T"]) and nested[SRC][KEYS["T"]] is r["t"]["T"]


def test_rejections_at_call_carry_their_reason(runs):
    from wxengine.engine import WXEngineError, _f32, load_library
    r = runs["L16to13"]
    t = r["t"]
    with pytest.raises(WXEngineError, match="must be a float32"):
        make_block("L16to13")(batch_of(dict(t, T=t["T"].double())))
    with pytest.raises(WXEngineError, match="on the GPU"):
        make_block("L16to13")(batch_of(dict(t, q=t["q"].cpu())))
    with pytest.raises(WXEngineError, match="must be a float32 \\[B, n_levels, n_time, H, W\\]"):
        make_block("L16to13")(batch_of(dict(t, q=t["q"][:, :, 0])))
    with pytest.raises(WXEngineError, match="H x W must agree"):
        make_block("L16to13")(batch_of(dict(t, T=t["T"][..., :30].contiguous())))
    with pytest.raises(WXEngineError, match="does not match"):
        make_block("L16to13")(batch_of(dict(t, sp=t["sp"].expand(2, -1, -1, -1, -1).contiguous())))
    with pytest.raises(WXEngineError, match="n_time"):
        make_block("L16to13")(batch_of(dict(t, q=t["q"].expand(-1, -1, 2, -1, -1).contiguous())))
    with pytest.raises(WXEngineError, match="a batch item must be contiguous"):
        make_block("L16to13")(batch_of(dict(t, q=t["q"].transpose(3, 4).contiguous().transpose(3, 4))))
    with pytest.raises(WXEngineError, match="the surface pressure is \\[B, 1, n_time, H, W\\]"):
        make_block("L16to13")(batch_of(dict(t, sp=t["T"])))
    with pytest.raises(ValueError, match="has 15 levels but the source coefficients define 16 midpoint levels"):
        make_block("L16to13")(batch_of(dict(t, T=t["T"][:, :15].contiguous())))
    if torch.cuda.device_count() > 1:
        with pytest.raises(WXEngineError, match="one device"):
            make_block("L16to13")(batch_of(dict(t, q=t["q"].to("cuda:1"))))
    # the C ABI: a null handle or pointer, a count out of range or a non-finite coefficient is an error status with its reason
    lib = load_library()
    sa, sb, da, db = midpoints("L16to13")
    H, W = t["sp"].shape[3:]
    one, one64 = (C.c_void_p * 1)(t["q"].data_ptr()), (C.c_int64 * 1)(0)
    out = torch.empty_like(r["y"]["q"])
    dst = (C.c_void_p * 1)(out.data_ptr())
    sp = C.c_void_p(t["sp"].data_ptr())
    assert lib.wx_hybrid_apply(None, 1, one, one64, dst, 1, 1, sp, 0, None) == -1 and b"null hybrid-interpolation handle" in lib.wx_last_error()
    assert lib.wx_hybrid_destroy(None) == 0
    h = C.c_void_p()
    create = lambda *a: lib.wx_hybrid_create(*a)  # noqa: E731
    ok = (H, W, 16, _f32(sa), _f32(sb), 13, _f32(da), _f32(db), 0)
    assert create(*ok, None) == -1 and b"null argument" in lib.wx_last_error()
    assert create(H, W, 16, None, _f32(sb), 13, _f32(da), _f32(db), 0, C.byref(h)) == -1 and b"null coefficient" in lib.wx_last_error()
    assert create(H, W, 16, _f32(sa), _f32(sb), 13, _f32(da), None, 0, C.byref(h)) == -1 and b"null coefficient" in lib.wx_last_error()
    assert create(H, W, 1, _f32(sa), _f32(sb), 13, _f32(da), _f32(db), 0, C.byref(h)) == -1 and b"a single source level" in lib.wx_last_error()
    assert create(H, W, 138, _f32(sa), _f32(sb), 13, _f32(da), _f32(db), 0, C.byref(h)) == -1 and b"n_src must be 2 .. 137" in lib.wx_last_error()
    assert create(H, W, 16, _f32(sa), _f32(sb), 0, _f32(da), _f32(db), 0, C.byref(h)) == -1 and b"n_dst must be 1 .. 137" in lib.wx_last_error()
    assert create(H, W, 16, _f32(sa), _f32(sb), 138, _f32(da), _f32(db), 0, C.byref(h)) == -1 and b"n_dst must be 1 .. 137" in lib.wx_last_error()
    assert create(0, W, 16, _f32(sa), _f32(sb), 13, _f32(da), _f32(db), 0, C.byref(h)) == -1 and b"bad geometry" in lib.wx_last_error()
    bad = sa.copy()
    bad[5] = np.inf
    assert create(H, W, 16, _f32(bad), _f32(sb), 13, _f32(da), _f32(db), 0, C.byref(h)) == -1 and b"non-finite source coefficient at level 5" in lib.wx_last_error()
    bad = db.copy()
    bad[12] = np.nan
    assert create(H, W, 16, _f32(sa), _f32(sb), 13, _f32(da), _f32(bad), 0, C.byref(h)) == -1 and b"non-finite destination coefficient at level 12" in lib.wx_last_error()
    assert create(H, W, 16, _f32(sa), _f32(sb), 13, _f32(da), _f32(db), 99, C.byref(h)) == -1 and b"no such GPU device" in lib.wx_last_error()
    assert not h.value
    assert create(*ok, C.byref(h)) == 0, lib.wx_last_error()
    assert lib.wx_hybrid_apply(h, 1, None, one64, dst, 1, 1, sp, 0, None) == -1 and b"null argument" in lib.wx_last_error()
    assert lib.wx_hybrid_apply(h, 1, one, None, dst, 1, 1, sp, 0, None) == -1 and b"null argument" in lib.wx_last_error()
    assert lib.wx_hybrid_apply(h, 1, one, one64, None, 1, 1, sp, 0, None) == -1 and b"null argument" in lib.wx_last_error()
    assert lib.wx_hybrid_apply(h, 1, one, one64, dst, 1, 1, None, 0, None) == -1 and b"null argument" in lib.wx_last_error()
    null1 = (C.c_void_p * 1)(None)
    assert lib.wx_hybrid_apply(h, 1, null1, one64, dst, 1, 1, sp, 0, None) == -1 and b"null tensor pointer" in lib.wx_last_error()
    assert lib.wx_hybrid_apply(h, 1, one, one64, null1, 1, 1, sp, 0, None) == -1 and b"null tensor pointer" in lib.wx_last_error()
    assert lib.wx_hybrid_apply(h, 0, one, one64, dst, 1, 1, sp, 0, None) == -1 and b"1..32 variables" in lib.wx_last_error()
    assert lib.wx_hybrid_apply(h, 33, one, one64, dst, 1, 1, sp, 0, None) == -1 and b"1..32 variables" in lib.wx_last_error()
    assert lib.wx_hybrid_apply(h, 1, one, one64, dst, 0, 1, sp, 0, None) == -1 and b"batch and n_time must be >= 1" in lib.wx_last_error()
    assert lib.wx_hybrid_apply(h, 1, one, one64, dst, 1, 0, sp, 0, None) == -1 and b"batch and n_time must be >= 1" in lib.wx_last_error()
    assert lib.wx_hybrid_apply(h, 1, one, one64, dst, 1, 1, sp, 0, None) == 0, lib.wx_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, r["y"]["q"])
    assert lib.wx_hybrid_destroy(h) == 0


def test_composed_three_step_forecast_equals_the_restatement():
    """run_forecast with a stand-in model that returns fixed NORMALISED tensors and the chain [InverseScale, HybridLevelInterp] -- the
    block behind the inverse scale, because it needs pressures in Pa -- putting 16-level output onto 13 levels.  The initial condition
    holds a static field only, so nothing of the 13-level output is routed back into the 16-level input.  Against normalised * std +
    mean followed by tests/hybrid_oracle.py on the CPU; the gate is hybrid_cases.gate per variable, with d_ref = the restatement's own
    fp32-against-fp64 distance."""
    from wxengine.forecast import InverseScale, run_forecast
    H, W = 7, 19
    a = {k: np.ascontiguousarray(v[..., :H, :W]) for k, v in case_inputs("L16to13").items()}
    order = ("T", "q", "idx", "sp")
    nl = {v: a[v].shape[1] for v in order}
    steps = [a, dict(a, T=a["T"] + np.float32(1.5)), dict(a, sp=a["sp"] + np.float32(700.0))]
    short = {v: KEYS[v].split("/")[-1] for v in order}
    oro = f"{SRC}/static/2d/orography"
    mean = {short[v]: (np.arange(nl[v], dtype=np.float32) * 0.5 + (78000.0 if v == "sp" else 1.0 + i)) for i, v in enumerate(order)}
    std = {short[v]: (np.arange(nl[v], dtype=np.float32) * 0.25 + (15000.0 if v == "sp" else 2.0 + i)) for i, v in enumerate(order)}
    mean["orography"], std["orography"] = np.zeros(1, np.float32), np.ones(1, np.float32)

    def normalised(s):
        return {v: ((s[v].astype(np.float64) - mean[short[v]].reshape(1, -1, 1, 1, 1)) / std[short[v]].reshape(1, -1, 1, 1, 1)).astype(np.float32)
                for v in order}
    norm = [normalised(s) for s in steps]
    y_preds = [torch.from_numpy(np.concatenate([n[v] for v in order], axis=1)).cuda() for n in norm]     # [1, 3 * 16 + 1, 1, H, W]
    calls = []

    def model(x):
        calls.append(tuple(x.shape))
        return y_preds[len(calls) - 1]
    cmap, c0 = {}, 0
    for v in order:
        cmap[KEYS[v]] = {"slice": slice(c0, c0 + nl[v]), "orig_shape": (nl[v], 1)}
        c0 += nl[v]
    ic = {"input": {SRC: {oro: torch.zeros(1, 1, 1, H, W, device="cuda")}}}
    blk = make_block("L16to13")
    sa, sb, da, db = midpoints("L16to13")
    seen = []

    def consume(yp, step):
        want = {}
        for dtype in (torch.float32, torch.float64):
            phys = {v: torch.from_numpy(norm[step - 1][v]).to(dtype) * torch.from_numpy(std[short[v]]).to(dtype).reshape(1, -1, 1, 1, 1)
                    + torch.from_numpy(mean[short[v]]).to(dtype).reshape(1, -1, 1, 1, 1) for v in order}
            want[dtype] = HO.interp({v: phys[v] for v in ("T", "q", "idx")}, phys["sp"], sa, sb, da, db, dtype=dtype)
        for v in ("T", "q", "idx"):
            got = yp[SRC][KEYS[v]].cpu().numpy()
            assert got.shape == (1, 13, 1, H, W)
            w32, w64 = want[torch.float32][v].numpy(), want[torch.float64][v].numpy()
            d_ref = distance(w32, w64)
            b32, b64 = gate(d_ref)
            d32, d64 = distance(got, w32), distance(got, w64)
            print(f"[hybrid gpu] forecast step {step} {v}: d_ref {d_ref:.2e}; vs fp32 restatement {d32:.2e} (<= {b32:.2e}), "
                  f"vs fp64 restatement {d64:.2e} (<= {b64:.2e})")
            assert d32 <= b32 and d64 <= b64, (step, v, d32, b32, d64, b64)
        assert yp[SRC][KEYS["sp"]].shape == (1, 1, 1, H, W)
        seen.append(step)
    run_forecast(model, ic, [{"input": {}}, {"input": {}}], 3, cmap, mean, std, [InverseScale(mean, std), blk], consume)
    assert seen == [1, 2, 3] and len(calls) == 3
    for yp, n in zip(y_preds, norm):      # y_pred itself was read in place and never written
        assert torch.equal(yp.cpu(), torch.from_numpy(np.concatenate([n[v] for v in order], axis=1)))
