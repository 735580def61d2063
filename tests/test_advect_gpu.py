"""The semi-Lagrangian advection on the device (csrc/wx_advect.h through wxengine/advect.py) against the reference's goldens
(tests/golden/advect_*.npz): every tracer of every case in both row regions under the gate of tests/advect_cases.gate -- against the
fp32 golden max(4 d_ref, 2e-6), against the fp64 golden max(5 d_ref, 2e-6), d_ref being the reference's own fp32-against-fp64 distance
of the same tracer and region, stored in the fixture.  The 2e-6 floor stands on both sides because the fp32 index arithmetic has an
absolute error of about W 2^-24 whatever d_ref is.  The edge rows of `polewind` get a loose bound this way (d_ref ~ 3e-3): that is the
reference's own conditioning there -- it divides a 12 m/s wind by its cos(lat) floor of 1e-4 and wraps the result around the globe
hundreds of times -- not slack chosen here.

Then the bit-exact properties (zero winds, a second object and a second call, untouched inputs, fresh contiguous outputs), inputs read
in place from channel-slice views at an aligned and a one-float-shifted offset on a side stream, the omega input bypassing continuity,
a wind as its own tracer, the grid-mismatch fallback, the pre block, the rejections with their reasons and the null-argument statuses
of the C ABI, and one composed three-step run_forecast with [InverseScale, SemiLagrangianAdvection] against the
tests/advect_oracle.py chain.  The figures measured on MI355X are in DESIGN.md (semi-Lagrangian advection)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import advect_oracle as AO  # noqa: E402
from advect_cases import (ADVECT_CASES, KEYS, REGIONS, SRC, block_args, case_inputs, gate, grid_of, load_golden, oracle_args,  # noqa: E402
                          region_distance, region_rows)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def make_block(name, **kw):
    from wxengine.advect import SemiLagrangianAdvection
    args = block_args(name)
    args.update(kw)
    return SemiLagrangianAdvection(**args)


def batch_of(t):
    return {"y_processed": {SRC: {KEYS[v]: t[v] for v in t}}}


def run(blk, t, tracers):
    y = blk(batch_of(t))["y_processed"][SRC]
    return {v: y[KEYS[v]] for v in tracers}


@pytest.fixture(scope="module")
def runs():
    """Per case: inputs on the GPU, goldens, and the block's outputs (computed once, shared, never modified)."""
    out = {}
    for name, c in ADVECT_CASES.items():
        g, f32, f64, d_ref = load_golden(name, GOLD)
        inp = case_inputs(name, check=g)
        t = {v: torch.from_numpy(inp[v]).cuda() for v in inp}
        blk = make_block(name)
        y = run(blk, t, c["tracers"])
        torch.cuda.synchronize()
        out[name] = dict(inp=inp, t=t, f32=f32, f64=f64, d_ref=d_ref, blk=blk, y=y)
    return out


@pytest.mark.parametrize("name", list(ADVECT_CASES))
def test_every_tracer_and_region_vs_reference_goldens(runs, name):
    r = runs[name]
    rows = region_rows(ADVECT_CASES[name]["H"])
    bad = []
    for v in ADVECT_CASES[name]["tracers"]:
        got = r["y"][v].cpu().numpy()
        assert got.shape == r["f32"][v].shape and np.isfinite(got).all(), (name, v)
        for reg in REGIONS:
            b32, b64 = gate(r["d_ref"][(v, reg)])
            d32, d64 = region_distance(got, r["f32"][v], rows[reg]), region_distance(got, r["f64"][v], rows[reg])
            print(f"[advect gpu] {name} {v} {reg}: d_ref {r['d_ref'][(v, reg)]:.2e}; vs fp32 golden {d32:.2e} (<= {b32:.2e}), "
                  f"vs fp64 golden {d64:.2e} (<= {b64:.2e})")
            if not (d32 <= b32 and d64 <= b64):
                bad.append((v, reg, d32, b32, d64, b64))
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", list(ADVECT_CASES))
def test_bit_exact_properties(runs, name):
    r = runs[name]
    c = ADVECT_CASES[name]
    keep = {v: r["t"][v].clone() for v in r["t"]}
    again = run(make_block(name), r["t"], c["tracers"])        # a second object, a second call: the same bits
    twice = run(r["blk"], r["t"], c["tracers"])
    calm = dict(r["t"], U=torch.zeros_like(r["t"]["U"]), V=torch.zeros_like(r["t"]["V"]))
    if "omega" in calm:
        calm["omega"] = torch.zeros_like(calm["omega"])
    still = run(r["blk"], calm, c["tracers"])
    for v in c["tracers"]:
        y, t = r["y"][v], r["t"][v]
        assert y.shape == t.shape and y.dtype == torch.float32 and y.is_contiguous() and y.data_ptr() != t.data_ptr()
        assert torch.equal(again[v], y) and torch.equal(twice[v], y), (name, v)
        assert again[v].data_ptr() != y.data_ptr() and twice[v].data_ptr() != y.data_ptr()
        assert torch.equal(still[v], t), (name, v)            # zero winds: the input's bits
        assert not torch.equal(y, t)
    for v in r["t"]:
        assert torch.equal(r["t"][v], keep[v]), (name, v)         # the inputs are never modified


@pytest.mark.parametrize("name", ["base36", "b2s2t", "tiny", "omega"])
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "unaligned"])
def test_channel_slice_views_and_a_side_stream(runs, name, shift):
    """The variables as Reconstruct hands them out: channel slices of one [B, C, 1, H, W] tensor (with B = 2 the batch items of a view
    are not adjacent).  shift 1 starts that tensor one float into its buffer, so no plane sits on 16 bytes."""
    r = runs[name]
    c, t = ADVECT_CASES[name], runs[name]["t"]
    order = sorted(t)
    C_all = 1 + sum(t[v].shape[1] for v in order)
    n = c["B"] * C_all * c["H"] * c["W"]
    flat = torch.full((n + 4,), 7.0, device="cuda")
    big = flat[shift:shift + n].view(c["B"], C_all, 1, c["H"], c["W"])
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
        y = run(make_block(name), views, c["tracers"])
    side.synchronize()
    for v in c["tracers"]:
        assert torch.equal(y[v], r["y"][v]), (name, v)
    assert torch.equal(flat, keep)


def test_omega_input_bypasses_continuity(runs):
    """`omega` case.  With omega given, U and V enter a grid point's velocity record pointwise only; through continuity the top level's
    divergence would enter omega at every level below it.  The given omega moves no point by a whole level, so a trajectory that starts
    at level >= 2 never reads a level-0 record: with the level-0 winds replaced by zeros (no divergence there), levels >= 2 keep their
    bits.  The same replacement with continuity on changes them."""
    r = runs["omega"]
    oa = oracle_args("omega")
    _, (_, _, lev) = AO.advect({KEYS[k]: torch.from_numpy(v) for k, v in r["inp"].items()}, dtype=torch.float64, want_departure=True, **oa)
    L = ADVECT_CASES["omega"]["L"]
    assert float((lev - torch.arange(L).view(1, L, 1, 1)).abs().max()) < 1.0
    t2 = dict(r["t"], U=r["t"]["U"].clone(), V=r["t"]["V"].clone())
    t2["U"][:, 0] = 0
    t2["V"][:, 0] = 0
    y2 = run(r["blk"], t2, ("q",))["q"]
    assert torch.equal(y2[:, 2:], r["y"]["q"][:, 2:])
    assert not torch.equal(y2[:, 0], r["y"]["q"][:, 0])
    cont = make_block("omega", omega_var=None)
    a, b = run(cont, r["t"], ("q",))["q"], run(cont, t2, ("q",))["q"]
    assert not torch.equal(a[:, 2:], b[:, 2:])
    assert not torch.equal(a, r["y"]["q"])


def test_a_wind_may_be_its_own_tracer(runs):
    r = runs["b2s2t"]
    t = dict(r["t"], U2=r["t"]["U"].clone())
    keys = dict(KEYS, U2=f"{SRC}/prognostic/3d/u_copy")
    nested = {SRC: {keys[v]: t[v] for v in t}}
    make_block("b2s2t", tracer_vars=[KEYS["U"], KEYS["V"], keys["U2"], KEYS["q"]])({"y_processed": nested})
    assert torch.equal(nested[SRC][KEYS["U"]], nested[SRC][keys["U2"]])       # the winds are read from the inputs
    assert torch.equal(nested[SRC][KEYS["q"]], r["y"]["q"])
    assert not torch.equal(nested[SRC][KEYS["U"]], r["t"]["U"]) and not torch.equal(nested[SRC][KEYS["V"]], r["t"]["V"])


def test_grid_mismatch_fallback_equals_the_explicit_uniform_grid(runs, caplog):
    import logging
    from wxengine.advect import uniform_grid
    r = runs["base36"]
    lat_g, lon_g = grid_of("gauss")            # 25 x 40: does not match the 24 x 36 data
    lat_u, lon_u = uniform_grid(24, 36)
    fallback = make_block("base36", latitude=lat_g, longitude=lon_g)
    with caplog.at_level(logging.WARNING, logger="wxengine.advect"):
        a = run(fallback, r["t"], ("q", "T"))
        a2 = run(fallback, r["t"], ("q", "T"))
    assert len([rec for rec in caplog.records if "using the uniform global grid" in rec.getMessage()]) == 1
    b = run(make_block("base36", latitude=lat_u, longitude=lon_u), r["t"], ("q", "T"))
    for v in ("q", "T"):
        assert torch.equal(a[v], b[v]) and torch.equal(a2[v], b[v])
    wrong = run(make_block("base36", latitude=lat_g[:24], longitude=lon_u), r["t"], ("q", "T"))     # matching lengths are used as given
    assert not torch.equal(wrong["q"], b["q"])


def test_pre_block_advects_the_present_data_types_and_leaves_the_callers_dict(runs):
    from wxengine.advect import SemiLagrangianAdvectionPre
    r = runs["base36"]
    nested = {SRC: {KEYS[v]: r["t"][v] for v in r["t"]}}
    batch = {"input": nested, "metadata": {"note": 1}}
    out = SemiLagrangianAdvectionPre(**block_args("base36"))(batch)
    assert batch["input"] is nested and nested[SRC][KEYS["q"]] is r["t"]["q"] and "target" not in out
    for v in ("q", "T"):
        assert torch.equal(out["input"][SRC][KEYS[v]], r["y"][v])
    assert out["input"][SRC][KEYS["U"]] is r["t"]["U"] and out["metadata"] is batch["metadata"]
    both = SemiLagrangianAdvectionPre(data_types=["target"], **block_args("base36"))({"input": nested, "target": nested})
    assert both["input"] is nested and torch.equal(both["target"][SRC][KEYS["T"]], r["y"]["T"])


def test_rejections_at_call_carry_their_reason(runs):
    from wxengine.engine import WXEngineError, load_library
    r = runs["base36"]
    t = r["t"]
    with pytest.raises(WXEngineError, match="must be a float32"):
        make_block("base36")(batch_of(dict(t, T=t["T"].double())))
    with pytest.raises(WXEngineError, match="on the GPU"):
        make_block("base36")(batch_of(dict(t, V=t["V"].cpu())))
    with pytest.raises(WXEngineError, match="H x W must agree"):
        make_block("base36")(batch_of(dict(t, T=t["T"][..., :30].contiguous())))
    with pytest.raises(WXEngineError, match="does not match"):
        make_block("base36")(batch_of(dict(t, sp=t["sp"].expand(2, -1, -1, -1, -1).contiguous())))
    with pytest.raises(WXEngineError, match="n_time = 2"):
        make_block("base36")(batch_of(dict(t, q=t["q"].expand(-1, -1, 2, -1, -1).contiguous())))
    with pytest.raises(ValueError, match="built 6 interface pressures for 4 levels; expected 5. Set `levels`"):
        make_block("base36")(batch_of({k: (v if k == "sp" else v[:, :4].contiguous()) for k, v in t.items()}))
    a2 = np.array([0.0, 2000.0], np.float32), np.array([0.0, 1.0], np.float32)
    with pytest.raises(WXEngineError, match="a single level"):
        make_block("base36", model_a_half=a2[0], model_b_half=a2[1])(batch_of({k: (v if k == "sp" else v[:, :1].contiguous()) for k, v in t.items()}))
    with pytest.raises(KeyError, match="absent"):
        make_block("base36", tracer_vars=[f"{SRC}/prognostic/3d/absent"])(batch_of(t))
    if torch.cuda.device_count() > 1:
        with pytest.raises(WXEngineError, match="one device"):
            make_block("base36")(batch_of(dict(t, q=t["q"].to("cuda:1"))))
    # the C ABI: a null handle or pointer is an error status with its reason, not a crash
    lib = load_library()
    one, one64 = (C.c_void_p * 1)(t["q"].data_ptr()), (C.c_int64 * 1)(0)
    out = torch.empty_like(t["q"])
    dst = (C.c_void_p * 1)(out.data_ptr())
    u, v, sp = t["U"].data_ptr(), t["V"].data_ptr(), t["sp"].data_ptr()
    assert lib.wx_advect_apply(None, u, 0, v, 0, sp, 0, None, 0, 1, one, one64, dst, 1, None) == -1
    assert b"null advection handle" in lib.wx_last_error()
    assert lib.wx_advect_destroy(None) == 0
    from wxengine.advect import metric_tables
    from wxengine.engine import _f32
    a_half, b_half = block_args("base36")["model_a_half"], block_args("base36")["model_b_half"]
    tab = metric_tables(*grid_of("base36"))
    rows, dlon = _f32(tab["rows"]), float(tab["dlon"])
    h = C.c_void_p()
    create = lambda *a: lib.wx_advect_create(*a)  # noqa: E731
    assert create(24, 36, 5, _f32(a_half), _f32(b_half), None, dlon, 21600.0, 2, 1.0, 0, 0, C.byref(h)) == -1 and b"null argument" in lib.wx_last_error()
    assert create(24, 36, 5, None, _f32(b_half), rows, dlon, 21600.0, 2, 1.0, 0, 0, C.byref(h)) == -1 and b"null coefficient" in lib.wx_last_error()
    assert create(24, 36, 5, _f32(a_half), _f32(b_half), rows, dlon, 21600.0, 0, 1.0, 0, 0, C.byref(h)) == -1 and b"n_iterations must be >= 1" in lib.wx_last_error()
    assert create(24, 36, 1, _f32(a_half), _f32(b_half), rows, dlon, 21600.0, 2, 1.0, 0, 0, C.byref(h)) == -1 and b"a single level" in lib.wx_last_error()
    assert create(24, 1, 5, _f32(a_half), _f32(b_half), rows, dlon, 21600.0, 2, 1.0, 0, 0, C.byref(h)) == -1 and b"bad geometry" in lib.wx_last_error()
    assert create(24, 36, 5, _f32(a_half), _f32(b_half), rows, 0.0, 21600.0, 2, 1.0, 0, 0, C.byref(h)) == -1 and b"longitude spacing" in lib.wx_last_error()
    assert create(24, 36, 5, _f32(a_half), _f32(b_half), rows, dlon, float("inf"), 2, 1.0, 0, 0, C.byref(h)) == -1 and b"must be finite" in lib.wx_last_error()
    bad_rows = tab["rows"].copy()
    bad_rows[2, 7] = 0.0
    assert create(24, 36, 5, _f32(a_half), _f32(b_half), _f32(bad_rows), dlon, 21600.0, 2, 1.0, 0, 0, C.byref(h)) == -1 and b"spacing not zero" in lib.wx_last_error()
    assert create(24, 36, 5, _f32(a_half), _f32(b_half), rows, dlon, 21600.0, 2, 1.0, 0, 0, None) == -1
    assert not h.value
    assert create(24, 36, 5, _f32(a_half), _f32(b_half), rows, dlon, 21600.0, 2, 1.0, 0, 0, C.byref(h)) == 0, lib.wx_last_error()
    assert lib.wx_advect_apply(h, None, 0, v, 0, sp, 0, None, 0, 1, one, one64, dst, 1, None) == -1 and b"null" in lib.wx_last_error()
    assert lib.wx_advect_apply(h, u, 0, v, 0, None, 0, None, 0, 1, one, one64, dst, 1, None) == -1 and b"null" in lib.wx_last_error()
    assert lib.wx_advect_apply(h, u, 0, v, 0, sp, 0, None, 0, 1, None, one64, dst, 1, None) == -1 and b"null" in lib.wx_last_error()
    null1 = (C.c_void_p * 1)(None)
    assert lib.wx_advect_apply(h, u, 0, v, 0, sp, 0, None, 0, 1, null1, one64, dst, 1, None) == -1 and b"null tensor pointer" in lib.wx_last_error()
    assert lib.wx_advect_apply(h, u, 0, v, 0, sp, 0, None, 0, 33, one, one64, dst, 1, None) == -1 and b"1..32 tracers" in lib.wx_last_error()
    assert lib.wx_advect_apply(h, u, 0, v, 0, sp, 0, None, 0, 1, one, one64, dst, 0, None) == -1 and b"batch must be >= 1" in lib.wx_last_error()
    assert lib.wx_advect_apply(h, u, 0, v, 0, sp, 0, None, 0, 1, one, one64, dst, 1, None) == 0, lib.wx_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, r["y"]["q"])
    assert lib.wx_advect_destroy(h) == 0


def test_composed_three_step_forecast_equals_the_oracle_chain():
    """run_forecast with a stand-in model that returns fixed NORMALISED tensors and the chain [InverseScale, SemiLagrangianAdvection] --
    the block behind the inverse scale, because it needs physical units.  Against normalised * std + mean followed by the
    tests/advect_oracle.py chain on the CPU; the gate is advect_cases.gate per tracer and row region, with d_ref = the oracle's own
    fp32-against-fp64 distance there."""
    from wxengine.forecast import InverseScale, run_forecast
    c = ADVECT_CASES["base36"]
    L, H, W = c["L"], c["H"], c["W"]
    order = ("U", "V", "q", "T", "sp")
    nl = {v: (1 if v == "sp" else L) for v in order}
    a, b = case_inputs("base36"), case_inputs("polewind")
    steps = [a, b, dict(a, V=-a["V"])]
    short = {v: KEYS[v].split("/")[-1] for v in order}
    mean = {short[v]: (np.arange(nl[v], dtype=np.float32) * 0.5 + (96000.0 if v == "sp" else 1.0 + i)) for i, v in enumerate(order)}
    std = {short[v]: (np.arange(nl[v], dtype=np.float32) * 0.25 + (4000.0 if v == "sp" else 2.0 + i)) for i, v in enumerate(order)}

    def normalised(s):
        return {v: ((s[v].astype(np.float64) - mean[short[v]].reshape(1, -1, 1, 1, 1)) / std[short[v]].reshape(1, -1, 1, 1, 1)).astype(np.float32)
                for v in order}
    norm = [normalised(s) for s in steps]
    y_preds = [torch.from_numpy(np.concatenate([n[v] for v in order], axis=1)).cuda() for n in norm]     # [1, 4 L + 1, 1, H, W]
    calls = []

    def model(x):
        calls.append(tuple(x.shape))
        return y_preds[len(calls) - 1]
    cmap, c0 = {}, 0
    for v in order:
        cmap[KEYS[v]] = {"slice": slice(c0, c0 + nl[v]), "orig_shape": (nl[v], 1)}
        c0 += nl[v]
    ic = {"input": {SRC: {KEYS[v]: torch.from_numpy(a[v]).cuda() for v in order}}}
    blk = make_block("base36")
    oa = oracle_args("base36")
    rows = region_rows(H)
    seen = []

    def consume(yp, step):
        want = {}
        for dtype in (torch.float32, torch.float64):
            fields = {KEYS[v]: torch.from_numpy(norm[step - 1][v]).to(dtype) * torch.from_numpy(std[short[v]]).to(dtype).reshape(1, -1, 1, 1, 1)
                      + torch.from_numpy(mean[short[v]]).to(dtype).reshape(1, -1, 1, 1, 1) for v in order}
            want[dtype] = {v: o.numpy() for v, o in zip(("q", "T"), AO.advect(fields, dtype=dtype, **oa).values())}
        for v in ("q", "T"):
            got = yp[SRC][KEYS[v]].cpu().numpy()
            assert got.shape == (1, L, 1, H, W)
            for reg in REGIONS:
                d_ref = region_distance(want[torch.float32][v], want[torch.float64][v], rows[reg])
                b32, b64 = gate(d_ref)
                d32, d64 = region_distance(got, want[torch.float32][v], rows[reg]), region_distance(got, want[torch.float64][v], rows[reg])
                print(f"[advect gpu] forecast step {step} {v} {reg}: d_ref {d_ref:.2e}; vs fp32 oracle {d32:.2e} (<= {b32:.2e}), "
                      f"vs fp64 oracle {d64:.2e} (<= {b64:.2e})")
                assert d32 <= b32 and d64 <= b64, (step, v, reg, d32, b32, d64, b64)
        seen.append(step)
    run_forecast(model, ic, [{"input": {}}, {"input": {}}], 3, cmap, mean, std, [InverseScale(mean, std), blk], consume)
    assert seen == [1, 2, 3] and len(calls) == 3
    for yp, n in zip(y_preds, norm):      # y_pred itself was read in place and never written
        assert torch.equal(yp.cpu(), torch.from_numpy(np.concatenate([n[v] for v in order], axis=1)))
