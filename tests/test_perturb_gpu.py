"""The perturbation noise on the device (csrc/wx_perturb.h through the raw C ABI and through wxengine/perturb.py) against the fixtures
(tests/golden/perturb_*.npz, the reference's own classes on keyed tapes).

The bar of the colour filter is derived, not tuned: the device accumulates in fp64 and rounds once to float32, so it may be no further
from the reference's fp64 evaluation than the reference's own float32 run is,
    max|device - ref64| <= E_ref = max|ref32 - ref64|   (absolute, over all planes of the case; hence max|device - ref32| <= 2 E_ref),
and every plane sums to zero within H W E_ref (the DC bin is removed).  Everything else is bit for bit: the epilogue against the same
float32 torch operations on the device's own amplitude-1 output, batching, in-place, strided destinations, and the generator's
independence of members, steps, plane counts and batching around a draw.  Every output lies between guard bands."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import perturb_cases as PC  # noqa: E402
import perturb_oracle as PO  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
GUARD, FILL = 96, -7777.25


@pytest.fixture(scope="module")
def lib():
    from wxengine.engine import load_library
    return load_library()


@pytest.fixture(scope="module")
def goldens():
    return {name: PC.load_golden(name, GOLD) for name in PC.PERTURB_CASES}


def guarded(shape):
    """-> (buffer, view of `shape` between two guard bands of FILL)."""
    n = int(np.prod(shape))
    buf = torch.full((2 * GUARD + n,), FILL, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_ok(buf):
    return bool((buf[:GUARD] == FILL).all() and (buf[-GUARD:] == FILL).all())


class Raw:
    """One handle of the raw C ABI."""

    def __init__(self, lib, H, W, kind, S=None):
        self.lib, self.H, self.W = lib, H, W
        self.h = C.c_void_p()
        s = None if S is None else np.ascontiguousarray(S, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))
        assert lib.wx_perturb_create(H, W, kind, s, 0, C.byref(self.h)) == 0, lib.wx_last_error()

    def close(self):
        assert self.lib.wx_perturb_destroy(self.h) == 0

    def apply(self, n_planes, tape=None, seed=0, member=0, step=0, amplitude=1.0, chan_scale=None, rho=0.0, prev=None, lat_weight=None, x=None,
              delta_out=None, x_out=None, strides=None, handle="own"):
        hw = self.H * self.W
        st = dict(prev=hw, x=hw, delta=hw, x_out=hw)
        st.update(strides or {})
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
        return self.lib.wx_perturb_apply(self.h if handle == "own" else handle, n_planes, p(tape), C.c_uint64(seed), member, step, amplitude,
                                         f(chan_scale), rho, p(prev), st["prev"], f(lat_weight), p(x), st["x"], p(delta_out), st["delta"],
                                         p(x_out), st["x_out"], C.c_void_p(torch.cuda.current_stream().cuda_stream))


def device_filter(lib, g, name, red, S=None):
    """The device's amplitude-1 output of a filter run on the case's tape (S: another table than the fixture's), between guard bands
    -> float32 [1, C, T, H, W] on the device."""
    shape = (1,) + tuple(PC.PERTURB_CASES[name]["shape"])
    H, W = shape[-2:]
    r = Raw(lib, H, W, 1, g[f"S_r{red}"] if S is None else S)
    tape = torch.from_numpy(PC.tape(name)).cuda()
    buf, out = guarded(shape)
    assert r.apply(int(np.prod(shape[:-2])), tape=tape, delta_out=out) == 0, lib.wx_last_error()
    torch.cuda.synchronize()
    r.close()
    assert guards_ok(buf) and torch.equal(tape.cpu(), torch.from_numpy(PC.tape(name)))
    return out


@pytest.mark.parametrize("name,red", PC.FILTER_RUNS)
def test_filter_is_no_further_from_fp64_than_the_reference(lib, goldens, name, red):
    g = goldens[name]
    H, W = PC.PERTURB_CASES[name]["shape"][-2:]
    got = device_filter(lib, g, name, red).cpu().numpy().astype(np.float64)
    e_ref = float(g[f"E_ref_r{red}"])
    d64 = float(np.abs(got - g[f"ref64_r{red}"]).max())
    d32 = float(np.abs(got - g[f"ref32_r{red}"].astype(np.float64)).max())
    sums = float(np.abs(got.sum(axis=(-2, -1))).max())
    print(f"perturb {name} r{red}: |dev - ref64| {d64:.3e} = {d64 / e_ref:.3f} E_ref, |dev - ref32| {d32:.3e} = {d32 / e_ref:.3f} E_ref, "
          f"max |plane sum| {sums:.3e} of {H * W * e_ref:.3e}")
    assert np.isfinite(got).all()
    assert d64 <= e_ref, f"{name} r{red}: {d64:.3e} from ref64, the reference's own float32 run {e_ref:.3e}"
    assert d32 <= 2 * e_ref
    assert sums <= H * W * e_ref


def test_reddening_0_is_a_closed_form_without_a_transform(lib, goldens):
    g = goldens["g37x72"]
    got = device_filter(lib, g, "g37x72", 0).cpu().numpy().astype(np.float64)
    want = PO.white_closed_form(PC.tape("g37x72"))
    d = float(np.abs(got - want).max())
    print(f"perturb g37x72 r0 closed form: {d:.3e} = {d / float(g['E_ref_r0']):.3f} E_ref")
    assert d <= float(g["E_ref_r0"])


def test_classes_give_the_raw_results(lib, goldens):
    from wxengine.perturb import ColorNoise, GaussianNoise
    g = goldens["p19x37"]
    tape = torch.from_numpy(PC.tape("p19x37")).cuda()
    cn = ColorNoise(1.0, 2)
    # the table is built by float32 torch operations on this host: the fixture's to PC.table_rtol (bit for bit beside the live reference,
    # tests/test_perturb_vs_reference.py); the class is the raw call on the table it built
    S = cn.weights(19, 37)
    assert np.abs(S.astype(np.float64) - g["S_r2"]).max() <= PC.table_rtol(19, 37) * np.abs(g["S_r2"]).max()
    assert torch.equal(cn(tape, white=tape), device_filter(lib, g, "p19x37", 2, S=S))
    assert cn.batch_planes(19, 37) == PC.batch_planes(19, 37)
    # GaussianNoise on a tape is amplitude * tape, bit for bit -- the reference's own result
    got = GaussianNoise(0.05)(tape, white=tape)
    assert torch.equal(got, 0.05 * tape) and np.array_equal(got.cpu().numpy().view(np.int32), g["gauss32"].view(np.int32))
    assert torch.equal(GaussianNoise([0.05])(tape, white=tape), got)


def test_generator_draws_are_the_documented_stream_and_depend_on_nothing_else(lib):
    from wxengine.noise import SLOT_PERTURB, normals
    assert SLOT_PERTURB == PC.SLOT == 16
    Cc, T, H, W = PC.PERTURB_CASES["p19x37"]["shape"]
    P, n = Cc * T, Cc * T * H * W
    r = Raw(lib, H, W, 0)
    draws = {}

    def draw(seed, member, step, planes=P):
        buf, out = guarded((planes, H, W))
        assert r.apply(planes, seed=seed, member=member, step=step, delta_out=out) == 0, lib.wx_last_error()
        torch.cuda.synchronize()
        assert guards_ok(buf)
        return out.cpu().numpy()
    for seed, member, step in ((7, 0, 0), (7, 1, 0), (7, 0, 1), ((1 << 40) + 5, 3, 9)):
        got = draws[(seed, member, step)] = draw(seed, member, step)
        want = normals(seed, 16, member, step, n).reshape(P, H, W).astype(np.float64)
        tol = 4e-6 * np.abs(want) + 1e-6       # the fp32 transcendentals against float64: tests/test_ensemble_gpu.py's tolerance of a draw
        assert (np.abs(got - want) <= tol).all(), f"seed {seed} member {member} step {step}: max {np.abs(got - want).max():.3e}"
    # other members and steps were drawn in between; a longer and a shorter call hold the same draws
    assert np.array_equal(draw(7, 0, 0), draws[(7, 0, 0)])
    assert np.array_equal(draw(7, 0, 0, planes=P + 3)[:P], draws[(7, 0, 0)]) and np.array_equal(draw(7, 0, 0, planes=1)[0], draws[(7, 0, 0)][0])
    for a, b in itertools.combinations(draws, 2):
        assert not np.array_equal(draws[a], draws[b]), (a, b)
    r.close()
    # the colour filter on the generator: 65 planes go in two batches, 3 planes in one; the shared planes have the same bits
    g = PC.load_golden("many19x37", GOLD)
    rc = Raw(lib, H, W, 1, g["S_r2"])
    outs = []
    for planes in (PC.batch_planes(H, W) + 1, 3):
        buf, out = guarded((planes, H, W))
        assert rc.apply(planes, seed=7, member=2, step=1, delta_out=out) == 0, lib.wx_last_error()
        torch.cuda.synchronize()
        assert guards_ok(buf)
        outs.append(out)
    assert torch.equal(outs[0][:3], outs[1]) and torch.isfinite(outs[0]).all() and float(outs[0].std()) > 0.5
    # ... and are the filter of the white kind's draws: fp64 accumulation and one rounding, half an ulp of the largest float32 output
    rw = Raw(lib, H, W, 0)
    draws3 = torch.empty((3, H, W), device="cuda")
    assert rw.apply(3, seed=7, member=2, step=1, delta_out=draws3) == 0, lib.wx_last_error()
    rw.close()
    want = PO.colour_filter(draws3.cpu().numpy(), g["S_r2"])
    half_ulp = float(np.spacing(np.float32(np.abs(want).max()))) / 2
    assert float(np.abs(outs[1].cpu().numpy() - want).max()) <= half_ulp + 1e-12 * float(np.abs(want).max())
    rc.close()


def test_epilogue_is_the_references_float32_operations_bit_for_bit(lib, goldens):
    g = goldens["p19x37"]
    Cc, T, H, W = PC.PERTURB_CASES["p19x37"]["shape"]
    P, shape = Cc * T, (1, Cc, T, H, W)
    n = device_filter(lib, g, "p19x37", 2)
    tape = torch.from_numpy(PC.tape("p19x37")).cuda()
    x = torch.from_numpy(PC.tape("p19x37", ".x")).cuda()
    prev = torch.from_numpy(PC.tape("p19x37", ".prev")).cuda()
    scale_c = np.array([2.0, 0.4], dtype=np.float32) / np.float32(0.05)
    scale_p = np.repeat(scale_c, T)
    lw = g["hemi_w"]
    r = Raw(lib, H, W, 1, g["S_r2"])
    amp, rho = 0.05, 0.9
    for use_cs, use_prev, use_lw, use_x in itertools.product((False, True), repeat=4):
        bd, d = guarded(shape)
        bx, xo = guarded(shape)
        assert r.apply(P, tape=tape, amplitude=amp, chan_scale=scale_p if use_cs else None, rho=rho, prev=prev if use_prev else None,
                       lat_weight=lw if use_lw else None, x=x if use_x else None, delta_out=d, x_out=xo if use_x else None) == 0, lib.wx_last_error()
        torch.cuda.synchronize()
        want = amp * n
        if use_cs:
            want = want * torch.from_numpy(scale_c).cuda().view(1, -1, 1, 1, 1)
        if use_prev:
            want = rho * prev + want
        if use_lw:
            want = want * torch.from_numpy(lw).cuda().view(1, 1, 1, -1, 1)
        what = f"chan_scale {use_cs}, prev {use_prev}, lat_weight {use_lw}, x {use_x}"
        assert torch.equal(d, want), what
        assert guards_ok(bd) and guards_ok(bx), what
        if use_x:
            assert torch.equal(xo, x + want), what
            xi = x.clone()                      # in place: x_out = x
            assert r.apply(P, tape=tape, amplitude=amp, chan_scale=scale_p if use_cs else None, rho=rho, prev=prev if use_prev else None,
                           lat_weight=lw if use_lw else None, x=xi, x_out=xi) == 0, lib.wx_last_error()
            assert torch.equal(xi, xo), what
        else:
            assert (xo == FILL).all()
    r.close()
    # the white kind goes through the same epilogue
    rw = Raw(lib, H, W, 0)
    bd, d = guarded(shape)
    assert rw.apply(P, tape=tape, amplitude=amp, chan_scale=scale_p, rho=rho, prev=prev, lat_weight=lw, x=x, delta_out=d, x_out=x) == 0
    assert torch.equal(d, (rho * prev + (amp * tape) * torch.from_numpy(scale_c).cuda().view(1, -1, 1, 1, 1)) * torch.from_numpy(lw).cuda().view(1, 1, 1, -1, 1))
    assert torch.equal(x, torch.from_numpy(PC.tape("p19x37", ".x")).cuda() + d) and guards_ok(bd)
    rw.close()


def test_temporal_noise_is_one_call_of_the_same_epilogue(lib, goldens):
    from wxengine.perturb import ColorNoise, TemporalNoise
    g = goldens["p19x37"]
    t = PC.TEMPORAL
    tape = torch.from_numpy(PC.tape("p19x37")).cuda()
    x = torch.from_numpy(PC.tape("p19x37", ".x")).cuda()
    prev = torch.from_numpy(PC.tape("p19x37", ".prev")).cuda()
    cn = ColorNoise(t["amplitude"], t["reddening"])
    n = device_filter(lib, g, "p19x37", 2, S=cn.weights(19, 37))
    tn = TemporalNoise(cn, t["rho"], torch.tensor(t["std"]), latitudes=g["hemi_lat"], north_scale=1.0, south_scale=0.5)
    state, delta = tn(x, prev, 2, seed=0, member=0, white=tape)
    sc = (torch.tensor(t["std"]) / torch.tensor([t["amplitude"]])).cuda().view(1, -1, 1, 1, 1)
    want = (t["rho"] * prev + (t["amplitude"] * n) * sc) * torch.from_numpy(g["hemi_w"]).cuda().view(1, 1, 1, -1, 1)
    assert torch.equal(delta, want) and torch.equal(state, x + want)
    state1, delta1 = tn(x, prev, 1, seed=0, member=0, white=tape)      # forecast_step 1 ignores the previous perturbation
    assert torch.equal(delta1, ((t["amplitude"] * n) * sc) * torch.from_numpy(g["hemi_w"]).cuda().view(1, 1, 1, -1, 1))
    # against the reference's own run (its rescale weights are all 1): the device's n is within 2 E_ref of the reference's
    tn1 = TemporalNoise(cn, t["rho"], torch.tensor(t["std"]), latitudes=g["hemi_lat"])
    _, d = tn1(x, prev, 2, seed=0, member=0, white=tape)
    bound = t["amplitude"] * max(t["std"]) / t["amplitude"] * 2 * float(g["E_ref_r2"]) + 4 * float(np.spacing(np.float32(np.abs(g["temporal_delta"]).max())))
    assert float(np.abs(d.cpu().numpy().astype(np.float64) - g["temporal_delta"]).max()) <= bound


def test_batching_and_strided_destinations(lib, goldens):
    g = goldens["many19x37"]
    P, _, H, W = PC.PERTURB_CASES["many19x37"]["shape"]
    assert P == PC.batch_planes(H, W) + 1
    r = Raw(lib, H, W, 1, g["S_r2"])
    n = C.c_int(0)
    assert lib.wx_perturb_batch(r.h, C.byref(n)) == 0 and n.value == P - 1
    tape = torch.from_numpy(PC.tape("many19x37")).cuda().view(P, H, W)
    bo, one = guarded((P, H, W))
    assert r.apply(P, tape=tape, delta_out=one) == 0, lib.wx_last_error()
    bp, per = guarded((P, H, W))
    for p in range(P):
        assert r.apply(1, tape=tape[p], delta_out=per[p]) == 0, lib.wx_last_error()
    torch.cuda.synchronize()
    assert torch.equal(one, per) and guards_ok(bo) and guards_ok(bp)
    # a channel range of a wider tensor, and planes at twice the plane stride: the neighbours keep their bits
    bw, wide = guarded((1, 6, 2, H, W))
    assert r.apply(4, tape=tape[:4], delta_out=wide[:, 2:4]) == 0, lib.wx_last_error()
    assert torch.equal(wide[0, 2:4].reshape(4, H, W), one[:4]) and (wide[:, :2] == FILL).all() and (wide[:, 4:] == FILL).all() and guards_ok(bw)
    bw, wide = guarded((1, 6, 2, H, W))
    x = torch.full((1, 6, 2, H, W), 1.5, device="cuda")
    assert r.apply(6, tape=tape[:6], x=x[:, :, 1], x_out=wide[:, :, 0], strides=dict(x=2 * H * W, x_out=2 * H * W)) == 0, lib.wx_last_error()
    assert torch.equal(wide[0, :, 0], 1.5 + one[:6]) and (wide[:, :, 1] == FILL).all() and guards_ok(bw)
    r.close()


def test_refusals_leave_the_outputs_untouched(lib, goldens):
    S = goldens["e5x8"]["S_r2"]
    h = C.c_void_p()
    sp = S.ctypes.data_as(C.POINTER(C.c_float))
    for args, msg in (((0, 8, 1, sp), b"H must be >= 1 and W >= 2"), ((5, 1, 1, sp), b"H must be >= 1 and W >= 2"), ((5, 8, 1, None), b"got a null pointer"),
                      ((5, 8, 2, sp), b"kind must be 0 (white) or 1 (colour)"), ((1 << 18, 1 << 17, 0, None), b"beyond the generator's counter"),
                      ((5, 5000, 1, sp), b"up to 4096 points a side")):
        assert lib.wx_perturb_create(*args, 0, C.byref(h)) == -1 and msg in lib.wx_last_error(), (args, lib.wx_last_error())
    bad = S.copy()
    bad[3, 2] = np.inf
    assert lib.wx_perturb_create(5, 8, 1, bad.ctypes.data_as(C.POINTER(C.c_float)), 0, C.byref(h)) == -1 and b"must be finite, entry 17" in lib.wx_last_error()
    assert lib.wx_perturb_create(5, 8, 1, sp, 0, None) == -1 and b"null argument" in lib.wx_last_error()
    r = Raw(lib, 5, 8, 1, S)
    P = 3
    tape = torch.from_numpy(PC.tape("e5x8")).cuda().view(P, 5, 8)
    bd, d = guarded((P, 5, 8))
    bx, xo = guarded((P, 5, 8))
    x = torch.ones((P, 5, 8), device="cuda")
    ok = dict(tape=tape, x=x, delta_out=d, x_out=xo)
    for change, msg in ((dict(handle=None), b"null perturbation handle"), (dict(n_planes=0), b"n_planes must be >= 1"),
                        (dict(n_planes=1 << 30), b"beyond the generator's counter"), (dict(delta_out=None, x_out=None), b"no output requested"),
                        (dict(x=None), b"x_out needs x"), (dict(strides=dict(delta=39)), b"a plane stride is smaller than H * W = 40"),
                        (dict(strides=dict(x=39)), b"a plane stride is smaller than H * W = 40"),
                        (dict(prev=x, strides=dict(prev=8)), b"a plane stride is smaller than H * W = 40"),
                        (dict(delta_out=tape), b"the tape overlaps an output"), (dict(x_out=tape[1:]), b"the tape overlaps an output"),
                        (dict(x_out=d[1:], n_planes=2), b"the two outputs overlap"), (dict(x=xo.view(-1)[8:], n_planes=2), b"without being the same view")):
        kw = dict(ok, n_planes=P)
        kw.update(change)
        n_planes = kw.pop("n_planes")
        assert r.apply(n_planes, **kw) == -1 and msg in lib.wx_last_error(), (change, lib.wx_last_error())
    torch.cuda.synchronize()
    assert (d == FILL).all() and (xo == FILL).all() and guards_ok(bd) and guards_ok(bx) and (x == 1).all()
    assert torch.equal(tape.cpu().view(-1), torch.from_numpy(PC.tape("e5x8")).view(-1))
    assert r.apply(P, **ok) == 0, lib.wx_last_error()
    assert lib.wx_perturb_batch(None, None) == -1 and b"null perturbation handle" in lib.wx_last_error()
    r.close()
    assert lib.wx_perturb_destroy(None) == 0


@pytest.fixture(scope="module")
def t0_engine():
    from wxengine.config import named_config
    from wxengine.engine import WXEngine
    from wxengine.synth import synth_denorm, synth_forcing, synth_input, synth_state_dict
    cfg = named_config("T0")
    e = WXEngine(cfg, "fp32", 0)
    e.load_state_dict(synth_state_dict(cfg))
    e.finalize()
    e.set_layout(cfg.channels * cfg.levels + cfg.surface_channels, 2, 2)
    e.set_denorm(*synth_denorm(cfg.base_output_channels))
    x0 = torch.from_numpy(synth_input(cfg)).cuda()
    frc = [torch.from_numpy(synth_forcing(cfg, 2, t + 1)).cuda() for t in range(3)]
    return cfg, e, x0, frc


def test_end_to_end_perturbed_ensemble_on_t0(t0_engine):
    import ens_cases as EC
    from wxengine.ensemble_metrics import EnsembleVerification
    from wxengine.perturb import ColorNoise
    from wxengine.rollout import perturbed_ensemble_rollout, score_ensemble_rollout
    cfg, e, x0, frc = t0_engine
    keep = x0.clone()
    plain, _ = e.rollout(x0, frc, phys_out=[torch.empty((1, cfg.base_output_channels) + tuple(cfg.out_hw), device="cuda") for _ in frc])
    noise = ColorNoise(0.05, 2)
    out = perturbed_ensemble_rollout(e, x0, frc, 3, noise, seed=5)
    assert torch.equal(x0, keep) and len(out) == 3 and all(len(m) == 3 for m in out)
    assert all(torch.isfinite(y).all() and y.shape == plain[0].shape for m in out for y in m)
    for m in range(3):
        single = perturbed_ensemble_rollout(e, x0, frc, 1, noise, seed=5, member0=m)
        assert all(torch.equal(a, b) for a, b in zip(single[0], out[m])), m
        assert not any(torch.equal(a, b) for a, b in zip(out[m], plain))
    assert not torch.equal(out[0][0], out[1][0]) and not torch.equal(out[1][2], out[2][2])
    for member in perturbed_ensemble_rollout(e, x0, frc, 2, ColorNoise(0.0, 2), seed=5):
        assert all(torch.equal(a, b) for a, b in zip(member, plain))
    n_ch = cfg.base_output_channels
    cmap = {"ERA5/prognostic/3d/first": slice(0, cfg.levels), "ERA5/diagnostic/2d/last": slice(n_ch - 1, n_ch)}
    verifier = EnsembleVerification(3, alpha=0.95, use_latitude_weights=True, latitude=EC.latitude(plain[0].shape[2]))
    pend = score_ensemble_rollout(out, plain, verifier, cmap)
    for p in pend:
        flat = EC.flat_scalars(p.result())
        spreads = [v for k, v in flat.items() if k.startswith("ens_spread/")]
        assert spreads and all(np.isfinite(v) and v > 0 for v in spreads), flat


def test_end_to_end_temporal_noise_carries_the_members_delta(t0_engine):
    from wxengine.perturb import ColorNoise, TemporalNoise
    from wxengine.rollout import perturbed_ensemble_rollout
    cfg, e, x0, frc = t0_engine
    noise = ColorNoise(0.05, 2)
    deltas = []
    out = perturbed_ensemble_rollout(e, x0, frc, 2, None, seed=5, member0=4, temporal=TemporalNoise(noise, temporal_correlation=0.9), deltas=deltas)
    assert len(out) == 2 and all(torch.isfinite(y).all() for m in out for y in m) and not torch.equal(out[0][2], out[1][2])
    n_prog = cfg.channels * cfg.levels + cfg.surface_channels
    for m, carried in enumerate(deltas):
        assert len(carried) == 3
        d1 = noise(x0, seed=5, member=4 + m, step=1)
        assert torch.equal(carried[0], d1[:, :n_prog])
        eps2 = noise(x0[:, :n_prog], seed=5, member=4 + m, step=2)
        assert torch.equal(carried[1], 0.9 * d1[:, :n_prog] + eps2)
