"""The ensemble verification on the device (csrc/wx_ensemble.h through wxengine/ensemble_metrics.py) against the goldens
(tests/golden/ens_*.npz): every scalar and every stored map of every case under the project's gate (hybrid_cases.gate): against the
fp32 golden max(4 d_ref, 2e-6), against the fp64 golden max(5 d_ref, 2e-6), d_ref being the reference's own fp32-against-fp64
distance of the same quantity, stored in the fixture; the distance and its scales are those of tests/ens_cases.py.

Then the bit-exact properties (a second call and a second object, both member layouts, maps requested or not, 34 variables in two
calls against 34 calls of one, a side stream, untouched inputs), m16 read through views at an aligned and a one-float-shifted
offset (the 16-byte and the scalar loads, both held to the goldens), the statuses and messages of the C ABI, and one composed run:
ensemble_rollout of three members over two steps scored by score_ensemble_rollout without a sync inside the loop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import ens_cases as EC  # noqa: E402
import ens_oracle as EO  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731


def make_verifier(case, inp, **kw):
    from wxengine.ensemble_metrics import EnsembleVerification
    args = EC.block_args(case, inp)
    args.update(kw)
    return EnsembleVerification(**args)


def separate(inp):
    """The members as M dicts of their own [B, L, T, H, W] buffers, nested under the source like y_processed."""
    M = next(iter(inp["members"].values())).shape[0]
    return [{EC.SRC: {EC.KEYS[n]: cuda(x[m]) for n, x in inp["members"].items()}} for m in range(M)]


def same_bits(a, b):
    fa, fb = EC.flat_scalars(a), EC.flat_scalars(b)
    return (list(fa) == list(fb) and all(fa[k] == fb[k] or (np.isnan(fa[k]) and np.isnan(fb[k])) for k in fa)
            and list(a.planes) == list(b.planes) and all(np.array_equal(a.planes[k], b.planes[k]) for k in a.planes))


def same_maps(a, b):
    return list(a.maps) == list(b.maps) and all(torch.equal(a.maps[m][k], b.maps[m][k]) for m in a.maps for k in a.maps[m])


@pytest.fixture(scope="module")
def runs():
    """Per case: inputs, members and truth on the GPU, goldens, the verifier and its result with all six maps (computed once, shared)."""
    out = {}
    for case in EC.ENS_CASES:
        g = EC.load_golden(case, GOLD)
        inp = EC.case_inputs(case, check=g["fix"])
        members = separate(inp)
        truth = {EC.SRC: {EC.KEYS[n]: cuda(t) for n, t in inp["truth"].items()}}
        v = make_verifier(case, inp, maps=EC.MAPS)
        out[case] = dict(inp=inp, g=g, members=members, truth=truth, verifier=v, got=v(members, truth))
    return out


def check_against_goldens(case, g, got, what):
    """Every scalar and every stored map against both goldens under the gate.  -> (worst distance / bound vs fp32, vs fp64)."""
    flat = EC.flat_scalars(got)
    assert list(flat) == g["keys"], (case, what)
    bad, worst = [], [0.0, 0.0]
    for i, k in enumerate(g["keys"]):
        assert np.isfinite(flat[k]), (case, what, k)
        b32, b64 = EC.gate(g["d_ref"][i])
        d32, d64 = EC.distance(flat[k], g["f32"][i], g["scale"][i]), EC.distance(flat[k], g["f64"][i], g["scale"][i])
        worst = [max(worst[0], d32 / b32), max(worst[1], d64 / b64)]
        if not (d32 <= b32 and d64 <= b64):
            bad.append((k, flat[k], g["f32"][i], g["f64"][i], d32, b32, d64, b64))
    assert sorted({n for _, n in g["maps"]}) == sorted(EC.ENS_CASES[case]["map_vars"])
    for (m, n), gm in g["maps"].items():
        k = EC.KEYS[n]
        # the fixture's ens_std is LatWeightedMetricsEnsemble's, with its (M + 1) / (M - 1) factor
        dev = (got.reference_ens_std(k) if m == "ens_std" else got.maps[m][k]).cpu().numpy()
        assert dev.shape == gm["f32"].shape and np.isfinite(dev).all(), (case, what, m, n)
        b32, b64 = EC.gate(gm["d_ref"])
        d32, d64 = EC.map_distance(dev, gm["f32"], gm["scale"]), EC.map_distance(dev, gm["f64"], gm["scale"])
        worst = [max(worst[0], d32 / b32), max(worst[1], d64 / b64)]
        if not (d32 <= b32 and d64 <= b64):
            bad.append((f"map {m}:{n}", d32, b32, d64, b64))
    assert not bad, (case, what, bad[:8])
    return worst


@pytest.mark.parametrize("case", list(EC.ENS_CASES))
def test_every_scalar_and_map_vs_goldens(runs, case):
    r = runs[case]
    worst = check_against_goldens(case, r["g"], r["got"], "separate members")
    print(f"[ens gpu] {case}: {len(r['g']['keys'])} scalars, {len(r['g']['maps'])} maps; worst distance / bound: vs fp32 golden {worst[0]:.3f}, "
          f"vs fp64 golden {worst[1]:.3f}")
    if case == "m3":      # is the device nearer the fp64 result than the fp32 reference, on the surface pressure?
        for m in ("crps", "fair_crps", "ens_mean"):
            gm = r["g"]["maps"][(m, "sp")]
            dev = r["got"].maps[m][EC.KEYS["sp"]].cpu().numpy()
            print(f"[ens gpu] m3 surface pressure {m}: device to fp64 {EC.map_distance(dev, gm['f64'], gm['scale']):.2e}, "
                  f"fp32 reference to fp64 {gm['d_ref']:.2e}")
    for k, tab in r["got"].planes.items():
        n = [n for n in r["inp"]["truth"] if EC.KEYS[n] == k][0]
        assert tab.shape == r["inp"]["truth"][n].shape[:3] + (6,) and tab.dtype == np.float64


@pytest.mark.parametrize("case", list(EC.ENS_CASES))
def test_bit_exact_properties(runs, case):
    from wxengine.ensemble_metrics import PendingEnsembleScores
    r = runs[case]
    keep_m = [{k: v.clone() for k, v in m[EC.SRC].items()} for m in r["members"]]
    keep_t = {k: v.clone() for k, v in r["truth"][EC.SRC].items()}
    again = r["verifier"](r["members"], r["truth"])                                   # a second call of the first object
    assert same_bits(again, r["got"]) and same_maps(again, r["got"]), case
    other = make_verifier(case, r["inp"], maps=EC.MAPS)                               # a second object, through submit
    p = other.submit(r["members"], r["truth"])
    assert isinstance(p, PendingEnsembleScores)
    res = p.result()
    assert same_bits(res, r["got"]) and same_maps(res, r["got"]) and p.result() is res and p.done(), case
    # the reference's [B * M, ...] layout, one tensor per variable: the same bits
    stacked = {EC.KEYS[n]: cuda(EC.stacked(x)) for n, x in r["inp"]["members"].items()}
    keep_s = {k: v.clone() for k, v in stacked.items()}
    res = other(stacked, r["truth"])
    assert same_bits(res, r["got"]) and same_maps(res, r["got"]), case
    # maps requested or not (and only some of them): the plane table keeps its bits
    for maps in ((), ("fair_crps",)):
        res = make_verifier(case, r["inp"], maps=maps)(r["members"], r["truth"])
        assert same_bits(res, r["got"]) and list(res.maps) == list(maps), (case, maps)
        for m in maps:
            assert all(torch.equal(res.maps[m][k], r["got"].maps[m][k]) for k in res.maps[m]), (case, m)
    for m, kept in zip(r["members"], keep_m):                                         # the inputs are never modified
        assert all(torch.equal(m[EC.SRC][k], kept[k]) for k in kept), case
    assert all(torch.equal(r["truth"][EC.SRC][k], keep_t[k]) for k in keep_t) and all(torch.equal(stacked[k], keep_s[k]) for k in keep_s)


def test_34_variables_in_two_calls_equal_34_calls_of_one():
    from wxengine.ensemble_metrics import EnsembleVerification
    M, shape = 4, (1, 1, 1, 7, 19)
    g = np.random.Generator(np.random.Philox(key=[2031, 99]))
    keys = [EC.KEYS[f"v{i:02d}"] for i in range(34)]
    truth = {k: cuda((2.0 * g.random(shape) - 1.0).astype(np.float32)) for k in keys}
    members = [{k: truth[k] + cuda((0.1 + 0.5 * (2.0 * g.random(shape) - 1.0)).astype(np.float32)) for k in keys} for _ in range(M)]
    v = EnsembleVerification(M, maps=("crps",))
    all34 = v(members, truth)
    assert list(all34.planes) == sorted(keys) and len(all34.planes) == 34
    for k in keys:
        one = v([{k: m[k]} for m in members], {k: truth[k]})
        assert np.array_equal(one.planes[k], all34.planes[k]) and torch.equal(one.maps["crps"][k], all34.maps["crps"][k]), k
        for s in EC.SCALARS:
            assert one[f"{s}/{k}"] == all34[f"{s}/{k}"], (s, k)


@pytest.mark.parametrize("case", ["m3", "m16", "m64"])
def test_a_side_stream_gives_the_same_bits(runs, case):
    r = runs[case]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = make_verifier(case, r["inp"], maps=EC.MAPS)(r["members"], r["truth"])
    side.synchronize()
    assert same_bits(got, r["got"]) and same_maps(got, r["got"]), case


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "unaligned"])
def test_m16_through_views_takes_16_byte_and_scalar_loads(runs, shift):
    """W = 64: views that start on 16 bytes take the 16-byte loads, the one-float-shifted ones the scalar loads.  Both are held to
    the goldens under the gate; the guard values around the views are untouched."""
    r = runs["m16"]
    flats = []

    def view(t):
        flat = torch.full((t.numel() + 8,), 7.0, device="cuda")
        v = flat[4 + shift:4 + shift + t.numel()].view(t.shape)
        assert (v.data_ptr() % 16 == 0) == (shift == 0)
        v.copy_(t)
        flats.append(flat)
        return v
    members = [{k: view(t) for k, t in m[EC.SRC].items()} for m in r["members"]]
    truth = {k: view(t) for k, t in r["truth"][EC.SRC].items()}
    keep = [f.clone() for f in flats]
    got = make_verifier("m16", r["inp"], maps=EC.MAPS)(members, truth)
    worst = check_against_goldens("m16", r["g"], got, f"views shifted by {shift}")
    print(f"[ens gpu] m16 through views, shift {shift}: worst distance / bound: vs fp32 golden {worst[0]:.3f}, vs fp64 golden {worst[1]:.3f}")
    assert all(torch.equal(f, k) for f, k in zip(flats, keep))
    if shift == 0:
        assert same_bits(got, r["got"]) and same_maps(got, r["got"])


@pytest.mark.parametrize("M", [3, 7, 20])
def test_vector_loads_of_the_4_8_and_32_member_instantiations(M):
    """The fixtures reach the 4-, 8- and 32-member instantiations at odd widths only.  On 8 x 64 they take their vector loads (16 bytes
    for 4 and 8, 8 bytes for 32); scalars and maps are held to the restatement on the same tensors under the gate, d_ref being the
    restatement's own fp32-against-fp64 distance, and a one-float-shifted view (scalar loads) to the same."""
    from wxengine.ensemble_metrics import EnsembleVerification
    g = np.random.Generator(np.random.Philox(key=[2031, 100 + M]))
    key, shape = EC.KEYS["unit"], (1, 2, 1, 8, 64)
    t, x = EC._field("unit", g, M, shape)
    t, x = t.astype(np.float32), x.astype(np.float32)
    r32, m32 = EO.restate({key: torch.from_numpy(x)}, {key: torch.from_numpy(t)}, 0.9, None, torch.float32)
    r64, m64 = EO.restate({key: torch.from_numpy(x)}, {key: torch.from_numpy(t)}, 0.9, None, torch.float64)
    w32, w64 = EC.flat_scalars(r32), EC.flat_scalars(r64)
    v = EnsembleVerification(M, alpha=0.9, maps=EC.MAPS)
    for shift in (0, 1):
        flat = torch.zeros((M + 1) * t.size + 8, device="cuda")
        views = [flat[4 + shift + i * t.size:4 + shift + (i + 1) * t.size].view(shape) for i in range(M + 1)]
        for dst, src in zip(views, [t] + list(x)):
            dst.copy_(torch.from_numpy(src))
        got = v([{key: m} for m in views[1:]], {key: views[0]})
        flat_got = EC.flat_scalars(got)
        assert list(flat_got) == list(w64)
        worst = 0.0
        for k in flat_got:
            scale = abs(w64[k])
            b32, b64 = EC.gate(EC.distance(w32[k], w64[k], scale))
            d32, d64 = EC.distance(flat_got[k], w32[k], scale), EC.distance(flat_got[k], w64[k], scale)
            worst = max(worst, d32 / b32, d64 / b64)
            assert d32 <= b32 and d64 <= b64, (M, shift, k, flat_got[k], w32[k], w64[k])
        for m in EC.MAPS:
            dev = (got.reference_ens_std(key) if m == "ens_std" else got.maps[m][key]).cpu().numpy()
            a32, a64 = m32[m][key].numpy(), m64[m][key].numpy()
            scale = float(np.abs(m64["ens_abs_err"][key].numpy()).mean()) if m == "ens_mean" else float(np.abs(a64).mean())
            b32, b64 = EC.gate(EC.map_distance(a32, a64, scale))
            d32, d64 = EC.map_distance(dev, a32, scale), EC.map_distance(dev, a64, scale)
            worst = max(worst, d32 / b32, d64 / b64)
            assert d32 <= b32 and d64 <= b64, (M, shift, m, d32, b32, d64, b64)
        print(f"[ens gpu] {M} members on 8 x 64, shift {shift}: worst distance / bound {worst:.3f}")


def test_66_row_blocks_take_the_finish_kernel_round_its_loop_twice():
    """The finish launch adds a plane's row blocks 64 at a time; no fixture has more than five.  521 x 4 with 3 members is 66 blocks
    of 8 rows, the last of one row, and W % 4 == 0: an aligned view takes the 16-byte loads, a one-float-shifted one the scalar
    loads.  Scalars and maps, with latitude weights, are held to the restatement on the same tensors under the gate, d_ref being the
    restatement's own fp32-against-fp64 distance."""
    from wxengine.ensemble_metrics import EnsembleVerification
    M, H, W = 3, 521, 4
    g = np.random.Generator(np.random.Philox(key=[2031, 66]))
    key, shape = EC.KEYS["unit"], (1, 1, 1, H, W)
    t, x = EC._field("unit", g, M, shape)
    t, x = t.astype(np.float32), x.astype(np.float32)
    w = EO.lat_weights(EC.latitude(H))
    r32, m32 = EO.restate({key: torch.from_numpy(x)}, {key: torch.from_numpy(t)}, 0.9, w, torch.float32)
    r64, m64 = EO.restate({key: torch.from_numpy(x)}, {key: torch.from_numpy(t)}, 0.9, w, torch.float64)
    w32, w64 = EC.flat_scalars(r32), EC.flat_scalars(r64)
    v = EnsembleVerification(M, alpha=0.9, maps=EC.MAPS, use_latitude_weights=True, latitude=EC.latitude(H))
    for shift in (0, 1):
        flat = torch.zeros((M + 1) * t.size + 8, device="cuda")
        views = [flat[4 + shift + i * t.size:4 + shift + (i + 1) * t.size].view(shape) for i in range(M + 1)]
        assert (views[0].data_ptr() % 16 == 0) == (shift == 0)
        for dst, src in zip(views, [t] + list(x)):
            dst.copy_(torch.from_numpy(src))
        got = v([{key: m} for m in views[1:]], {key: views[0]})
        flat_got = EC.flat_scalars(got)
        assert list(flat_got) == list(w64)
        worst = 0.0
        for k in flat_got:
            scale = abs(w64[k])
            b32, b64 = EC.gate(EC.distance(w32[k], w64[k], scale))
            d32, d64 = EC.distance(flat_got[k], w32[k], scale), EC.distance(flat_got[k], w64[k], scale)
            worst = max(worst, d32 / b32, d64 / b64)
            assert d32 <= b32 and d64 <= b64, (shift, k, flat_got[k], w32[k], w64[k])
        for m in EC.MAPS:
            dev = (got.reference_ens_std(key) if m == "ens_std" else got.maps[m][key]).cpu().numpy()
            a32, a64 = m32[m][key].numpy(), m64[m][key].numpy()
            scale = float(np.abs(m64["ens_abs_err"][key].numpy()).mean()) if m == "ens_mean" else float(np.abs(a64).mean())
            b32, b64 = EC.gate(EC.map_distance(a32, a64, scale))
            d32, d64 = EC.map_distance(dev, a32, scale), EC.map_distance(dev, a64, scale)
            worst = max(worst, d32 / b32, d64 / b64)
            assert d32 <= b32 and d64 <= b64, (shift, m, d32, b32, d64, b64)
        print(f"[ens gpu] 66 row blocks on 521 x 4, shift {shift}: worst distance / bound {worst:.3f}")


def test_rejections_at_call_carry_their_reason(runs):
    from wxengine.engine import WXEngineError
    r = runs["m2"]
    v = make_verifier("m2", r["inp"])
    k = EC.KEYS["t2m"]
    one = lambda m: {k: m[EC.SRC][k]}      # noqa: E731
    truth = {k: r["truth"][EC.SRC][k]}
    with pytest.raises(ValueError, match="1 member dicts for n_members = 2"):
        v([one(r["members"][0])], truth)
    with pytest.raises(WXEngineError, match="on the GPU"):
        v([one(r["members"][0]), {k: r["members"][1][EC.SRC][k].cpu()}], truth)
    with pytest.raises(WXEngineError, match="must be one \\[B, n_levels, n_time, H, W\\] shape"):
        v([one(m) for m in r["members"]], {k: truth[k][..., :5].contiguous()})
    with pytest.raises(KeyError, match="missing from member 1"):
        v([one(r["members"][0]), {"other": truth[k]}], truth)
    # float64 members and a truth on the host are converted and moved, as the reference's .float() / .to() do
    got = v([{k: m[EC.SRC][k].double()} for m in r["members"]], {k: truth[k].cpu()})
    assert np.array_equal(got.planes[k], r["got"].planes[k])


def test_c_abi_statuses_and_messages(runs):
    from wxengine.engine import _f32, load_library
    r = runs["m5lat"]
    lib = load_library()
    k = EC.KEYS["t2m"]
    xs = [m[EC.SRC][k] for m in r["members"]]
    t = r["truth"][EC.SRC][k]
    M = len(xs)
    H, W = t.shape[3:]
    w = EO.lat_weights(r["inp"]["lat"]).numpy()
    planes = torch.zeros(1, 6, dtype=torch.float64, device="cuda")
    ptrs = lambda ts: (C.c_void_p * len(ts))(*[x.data_ptr() if x is not None else None for x in ts])      # noqa: E731
    z64, l1 = (C.c_int64 * 1)(0), (C.c_int32 * 1)(1)
    pl = C.c_void_p(planes.data_ptr())
    ok = lambda h: (h, 1, ptrs(xs), z64, ptrs([t]), z64, l1, l1, 1, 1.0, None, pl, None)      # noqa: E731
    assert lib.wx_ensemble_apply(*ok(None)) == -1 and b"null ensemble handle" in lib.wx_last_error()
    assert lib.wx_ensemble_destroy(None) == 0
    h = C.c_void_p()
    assert lib.wx_ensemble_create(H, W, _f32(w), M, 0, None) == -1 and b"null argument" in lib.wx_last_error()
    for bad in (1, 65, 0, -2):
        assert lib.wx_ensemble_create(H, W, _f32(w), bad, 0, C.byref(h)) == -1 and b"2..64 members" in lib.wx_last_error(), bad
    assert lib.wx_ensemble_create(0, W, _f32(w), M, 0, C.byref(h)) == -1 and b"bad geometry" in lib.wx_last_error()
    assert lib.wx_ensemble_create(H, 0, None, M, 0, C.byref(h)) == -1 and b"bad geometry" in lib.wx_last_error()
    nan_w = w.copy()
    nan_w[5] = np.inf
    assert lib.wx_ensemble_create(H, W, _f32(nan_w), M, 0, C.byref(h)) == -1 and b"non-finite latitude weight at row 5" in lib.wx_last_error()
    assert lib.wx_ensemble_create(H, W, _f32(w), M, 99, C.byref(h)) == -1 and b"no such GPU device" in lib.wx_last_error()
    assert not h.value
    assert lib.wx_ensemble_create(H, W, _f32(w), M, 0, C.byref(h)) == 0, lib.wx_last_error()
    for i in (2, 3, 4, 5, 6, 7, 11):          # members, their strides, target, its strides, n_levels, n_time, planes
        a = list(ok(h))
        a[i] = None
        assert lib.wx_ensemble_apply(*a) == -1 and b"null argument" in lib.wx_last_error(), i
    for n in (0, 33):
        a = list(ok(h)); a[1] = n      # noqa: E702
        assert lib.wx_ensemble_apply(*a) == -1 and b"1..32 variables" in lib.wx_last_error()
    a = list(ok(h)); a[2] = ptrs(xs[:2] + [None] + xs[3:])      # noqa: E702
    assert lib.wx_ensemble_apply(*a) == -1 and b"null member pointer (variable 0, member 2)" in lib.wx_last_error()
    a = list(ok(h)); a[4] = (C.c_void_p * 1)(None)      # noqa: E702
    assert lib.wx_ensemble_apply(*a) == -1 and b"null tensor pointer" in lib.wx_last_error()
    a = list(ok(h)); a[8] = 0      # noqa: E702
    assert lib.wx_ensemble_apply(*a) == -1 and b"B >= 1" in lib.wx_last_error()
    a = list(ok(h)); a[6] = (C.c_int32 * 1)(0)      # noqa: E702
    assert lib.wx_ensemble_apply(*a) == -1 and b"n_levels and n_time must be >= 1" in lib.wx_last_error()
    fresh = torch.empty_like(t)
    for overlapped in (xs[1], t):             # a map that is a member, a map that is the truth
        a = list(ok(h)); a[10] = ptrs([None, None, None, fresh, overlapped, None])      # noqa: E702
        assert lib.wx_ensemble_apply(*a) == -1 and b"a map overlaps an input" in lib.wx_last_error()
    a = list(ok(h)); a[10] = ptrs([None, fresh, None, fresh, None, None])      # noqa: E702  two map slots on one buffer
    assert lib.wx_ensemble_apply(*a) == -1 and b"two maps overlap" in lib.wx_last_error()
    keep = [x.clone() for x in xs]
    a = list(ok(h)); a[10] = ptrs([None, None, None, fresh, None, None])      # noqa: E702
    assert lib.wx_ensemble_apply(*a) == 0, lib.wx_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(planes.cpu().numpy().reshape(1, 1, 1, 6), r["got"].planes[k])
    assert torch.equal(fresh, r["got"].maps["crps"][k]) and all(torch.equal(x, kx) for x, kx in zip(xs, keep))
    assert lib.wx_ensemble_destroy(h) == 0


def test_composed_ensemble_rollout_scored_every_step_without_a_sync():
    """The smallest ensemble configuration of tests/test_ensemble_gpu.py (T0, 32 latent dimensions), 3 members, 2 steps:
    ensemble_rollout, then score_ensemble_rollout against synthetic targets, then result() after the loop.  The scores are held to the
    restatement on CPU copies of the same device outputs under the gate, d_ref being the restatement's own fp32-against-fp64 distance."""
    from wxengine.config import named_config
    from wxengine.engine import WXEngine
    from wxengine.ensemble_metrics import EnsembleVerification, PendingEnsembleScores
    from wxengine.rollout import ensemble_rollout, score_ensemble_rollout
    from wxengine.synth import synth_denorm, synth_forcing, synth_input, synth_state_dict
    cfg = named_config("T0")
    cfg.noise_latent_dim = 32
    cfg.validate()
    e = WXEngine(cfg, "bf16", 0)
    e.load_state_dict(synth_state_dict(cfg))
    e.finalize()
    n_static, n_dyn, M, n_steps = 2, 2, 3, 2
    e.set_layout(cfg.channels * cfg.levels + cfg.surface_channels, n_static, n_dyn)
    e.set_denorm(*synth_denorm(cfg.base_output_channels))
    x0 = torch.from_numpy(synth_input(cfg)).cuda()
    frc = [torch.from_numpy(synth_forcing(cfg, n_dyn, t + 1)).cuda() for t in range(n_steps)]
    out = ensemble_rollout(e, x0, frc, M, seed=1)
    n_ch = cfg.base_output_channels
    cmap = {"ERA5/prognostic/3d/first": {"slice": slice(0, cfg.levels)}, "ERA5/prognostic/3d/second": slice(cfg.levels, 2 * cfg.levels),
            "ERA5/diagnostic/2d/last": slice(n_ch - 1, n_ch)}
    gen = torch.Generator(device="cuda").manual_seed(11)
    targets = [out[0][t] + 0.25 * out[0][t].abs().mean() * torch.randn(out[0][t].shape, device="cuda", generator=gen) for t in range(n_steps)]
    verifier = EnsembleVerification(M, alpha=0.95, use_latitude_weights=True, latitude=EC.latitude(out[0][0].shape[2]))
    pendings = score_ensemble_rollout(out, targets, verifier, cmap)
    assert len(pendings) == n_steps and all(isinstance(p, PendingEnsembleScores) for p in pendings)
    w = EO.lat_weights(EC.latitude(out[0][0].shape[2]))
    sl = {k: (v["slice"] if isinstance(v, dict) else v) for k, v in cmap.items()}
    for step, p in enumerate(pendings):
        got = EC.flat_scalars(p.result())
        members = {k: torch.stack([out[m][step][:, s].unsqueeze(2).cpu() for m in range(M)]) for k, s in sl.items()}
        truth = {k: targets[step][:, s].unsqueeze(2).cpu() for k, s in sl.items()}
        w32 = EC.flat_scalars(EO.restate(members, truth, 0.95, w, torch.float32, want_maps=False)[0])
        w64 = EC.flat_scalars(EO.restate(members, truth, 0.95, w, torch.float64, want_maps=False)[0])
        assert list(got) == list(w64)
        worst = 0.0
        for k in got:
            scale = abs(w64[k])
            b32, b64 = EC.gate(EC.distance(w32[k], w64[k], scale))
            d32, d64 = EC.distance(got[k], w32[k], scale), EC.distance(got[k], w64[k], scale)
            worst = max(worst, d32 / b32, d64 / b64)
            assert d32 <= b32 and d64 <= b64, (step, k, got[k], w32[k], w64[k])
        print(f"[ens gpu] ensemble rollout step {step + 1}: {len(got)} keys, worst distance / bound {worst:.3f}")
