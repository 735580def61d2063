"""The device PostBlock (csrc/wx_post.h through wx_post_* / wx_attach_postblock) against the fp64 oracle (oracle/fixers_oracle.py at
dtype=torch.float64) beyond the reference's 10 x 18 demo grid: tests/synth_batches.py::FIXER_CASES on G9 = 33 x 67 (9 workgroups,
a partial last one) and G257 = 181 x 363 (257 workgroups: a second trip of fix_sum_kernel's stride loop), pressure and hybrid sigma
grids, trapz / midpoint, denorm with four distinct statistics vectors, 1 - 3 input frames (all but the last NaN), 2 / 13 / 64 levels,
fix_level_num 2 / 3 / n_levels, 1 - 4 TOA and 1 - 8 surface flux terms; the tracer fixer; the two-frame golden of the reference's
own classes; and the registry class with post_conf.activate = True.

Gates are the project's (tests/test_fixers_gpu.py against the reference goldens): 5e-5 of the owned block's maximum for one fixer,
1e-4 for T / q / SP of a chain, 2e-3 for a chain's precipitation.  tests/test_fixers_oracle.py::test_sweep_case_is_well_conditioned
holds the fp32 oracle to a quarter of each gate on the same inputs.  Cases whose engine error lies between a quarter of the gate and
the gate: none.
fix_level_num = 1 stays accepted by wx_post_add_mass_fixer but is not swept: the reference's own denominator is then an empty integral
(gen1.py:264-270)."""
import numpy as np
import pytest
import torch

from oracle import fixers_oracle as F
from synth_batches import (FIXER_CASES, FIXER_GATES, fixer_block_error, fixer_case_inputs, fixer_case_oracle, fixer_case_owned,
                           fixer_case_terms)
from wxengine.engine import WXEngineError, WXPostBlock

from test_fixers_oracle import FRAMES2_GOLD, frames2_variant, rel

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def build_block(inp):
    c, lay = inp["case"], inp["lay"]
    H, W = inp["lat2d"].shape
    pb = WXPostBlock(H, W, lay["c_in"], c["frames"], lay["c_out"])
    if c["sigma"]:
        pb.set_grid_sigma(inp["lat2d"], inp["lon2d"], inp["coef_a"], inp["coef_b"], lay["sp"], c["midpoint"])
    else:
        pb.set_grid(inp["lat2d"], inp["lon2d"], inp["p"], c["midpoint"])
    dn = c["denorm"]
    if dn:
        pb.set_stats(*inp["stats"])
    ns, blocks = inp["n_seconds"], (lay["T"], lay["q"], lay["U"], lay["V"])
    terms = fixer_case_terms(inp)
    if c["fixer"] == "chain":
        tr = inp["tracer"]
        pb.add_tracer_fixer(tr["inds"], tr["thres"], tr["thres_max"], denorm=dn)
    if c["fixer"] in ("mass", "chain"):
        pb.add_mass_fixer(lay["q"], c["fix"], denorm=dn)
    if c["fixer"] in ("water", "chain"):
        pb.add_water_fixer(lay["q"], lay["precip"], lay["evapor"], ns, denorm=dn)
    if c["fixer"] in ("energy", "chain"):
        pb.add_energy_fixer(*blocks, [t[0] for t in terms[0] + terms[1]], inp["gph"], ns, denorm=dn)
    elif c["fixer"] == "updown":
        pb.add_energy_fixer_updown(*blocks, [t[0] for t in terms[0] + terms[1]], inp["gph"], ns, denorm=dn)
    elif c["fixer"].startswith("signed"):
        pb.add_energy_fixer_signed(*blocks, terms[0], terms[1], inp["gph"], ns, denorm=dn)
    return pb


@pytest.mark.parametrize("name", list(FIXER_CASES))
def test_sweep_case_matches_fp64_oracle(name):
    inp = fixer_case_inputs(name)
    ref = fixer_case_oracle(inp, torch.float64).numpy()
    pb = build_block(inp)
    xd = torch.from_numpy(inp["x"]).cuda()
    got = pb.apply(xd, torch.from_numpy(inp["y"]).cuda()).cpu().numpy()
    again = pb.apply(xd, torch.from_numpy(inp["y"]).cuda()).cpu().numpy()   # the same block object on a fresh copy of y
    assert np.isfinite(got).all()
    owned = np.zeros(got.shape[0], bool)
    errs = []
    for blk, gate in fixer_case_owned(inp):
        err = fixer_block_error(got, ref, blk)
        note = "   <-- between a quarter of the gate and the gate" if gate / 4 < err < gate else ""
        print(f"{name} channels {blk.start}:{blk.stop} engine vs fp64 oracle {err:.3e} (gate {gate:g}){note}")
        errs.append((err, gate))
        owned[blk] = True
    assert all(err < gate for err, gate in errs), errs
    np.testing.assert_array_equal(bits(got[~owned]), bits(inp["y"][~owned]))     # channels no fixer owns: bit-identical to the input
    np.testing.assert_array_equal(bits(again), bits(got))                        # fixed-order fp64 sums: reproducible to the bit


def test_level_limits():
    inp = fixer_case_inputs("G9-prs-mass")
    H, W = inp["lat2d"].shape
    for n in (1, 65):
        lv = np.linspace(1000.0, 100000.0, n).astype(np.float32)
        with pytest.raises(WXEngineError, match="levels"):
            WXPostBlock(H, W, 8, 1, 8).set_grid(inp["lat2d"], inp["lon2d"], lv, False)
        with pytest.raises(WXEngineError, match="levels"):
            WXPostBlock(H, W, 8, 1, 8).set_grid_sigma(inp["lat2d"], inp["lon2d"], lv, np.linspace(0, 1, n), 0, False)
    pb = WXPostBlock(H, W, 70, 1, 70)
    pb.set_grid(inp["lat2d"], inp["lon2d"], np.linspace(1000.0, 100000.0, 64).astype(np.float32), False)   # 64: the last accepted count
    for bad in (0, 65):
        with pytest.raises(WXEngineError, match="fix_level_num"):
            pb.add_mass_fixer(0, bad)
    for n_toa, n_srf in ((0, 1), (5, 1), (1, 0), (1, 9)):
        with pytest.raises(WXEngineError, match="flux terms|null argument"):
            pb.add_energy_fixer_signed(0, 0, 0, 0, [(0, 1.0)] * n_toa, [(1, 1.0)] * n_srf, inp["gph"], 21600.0)


# ------------------------------------------------------------------------------------------------------------------ tracer
def tracer_inputs():
    """y [7, 33, 67]: channels 0 / 2 clamped from below only (block A); 1 / 3 / 4 from both sides (block B); 5 / 6 unlisted.  Every
    listed channel holds values exactly AT each threshold and one ulp on either side; channel 3 has an upper threshold of 0 and
    holds -0.0 (which `>=` replaces by +0.0, as the reference's masked assignment does, and `>` would leave)."""
    g = np.random.Generator(np.random.Philox(key=[3, 43]))
    H, W = 33, 67
    y = g.standard_normal((7, H, W)).astype(np.float32)
    a = dict(inds=[0, 2], thres=[-0.5, 0.25], thres_max=None)
    b = dict(inds=[1, 3, 4], thres=[-1.0, -5.0, 0.0], thres_max=[0.75, 0.0, 1.0])
    return y, a, b


def plant(y, ch, k, values):
    f = np.float32
    edge = [v for t in values for v in (f(t), np.nextafter(f(t), f(np.inf)), np.nextafter(f(t), f(-np.inf)))]
    y[ch, k, :len(edge)] = edge


def test_tracer_fixer_clamps_bit_equal_without_denorm():
    y, a, b = tracer_inputs()
    for blk in (a, b):
        for k, ch in enumerate(blk["inds"]):
            plant(y, ch, 0, [blk["thres"][k]] + ([blk["thres_max"][k]] if blk["thres_max"] else []))
    y[3, 1, :8] = -0.0
    for blk in (a, b):
        pb = WXPostBlock(33, 67, 1, 1, 7)
        pb.add_tracer_fixer(blk["inds"], blk["thres"], blk["thres_max"])
        got = pb.apply(torch.zeros(1, 1, 33, 67).cuda(), torch.from_numpy(y).cuda()).cpu().numpy()
        ref = F.tracer_fixer(torch.from_numpy(y), blk["inds"], blk["thres"], blk["thres_max"]).numpy()
        assert int((ref != y).sum()) > 500
        np.testing.assert_array_equal(bits(got), bits(ref))           # clamped and unlisted channels alike, signed zeros included
    assert bits(ref[3, 1, :8]).tolist() == [0] * 8


def test_tracer_fixer_with_denorm():
    y, a, b = tracer_inputs()
    # channels 0 - 2: generic statistics (the round trip (v * std + mean - mean) / std may move untouched values: gate against the
    # fp64 oracle); channels 3 / 4: std 2, mean 1, where v * 2 + 1 rounds once with or without a fused multiply-add and the engine
    # must equal the fp32 oracle to the bit
    mean = np.array([0.3, -0.7, 1.9, 1.0, 1.0, 5.0, -3.0], np.float32)
    std = np.array([1.7, 0.6, 2.3, 2.0, 2.0, 0.1, 9.0], np.float32)
    a = dict(a, thres=[0.0, 1.5])                                            # physical units now
    b = dict(b, thres=[-1.0, -5.0, 0.0], thres_max=[-0.25, 0.0, 2.5])
    for k, ch in enumerate(b["inds"][1:], 1):                               # normalised values whose physical value IS the threshold
        plant(y, ch, 0, [(b["thres"][k] - 1.0) / 2.0, (b["thres_max"][k] - 1.0) / 2.0])
    t = lambda v, dt: torch.from_numpy(v).to(dt)   # noqa: E731
    for blk in (a, b):
        pb = WXPostBlock(33, 67, 1, 1, 7)
        pb.set_stats(np.zeros(1, np.float32), np.ones(1, np.float32), mean, std)
        pb.add_tracer_fixer(blk["inds"], blk["thres"], blk["thres_max"], denorm=True)
        got = pb.apply(torch.zeros(1, 1, 33, 67).cuda(), torch.from_numpy(y).cuda()).cpu().numpy()
        r32, r64 = (F.tracer_fixer(t(y, dt), blk["inds"], blk["thres"], blk["thres_max"], {"out": (t(mean, dt), t(std, dt))}).numpy()
                    for dt in (torch.float32, torch.float64))
        other = [c for c in range(7) if c not in blk["inds"]]
        np.testing.assert_array_equal(bits(got[other]), bits(y[other]))
        for ch in blk["inds"]:
            assert fixer_block_error(r32, r64, slice(ch, ch + 1)) <= FIXER_GATES["single"] / 4
            err = fixer_block_error(got, r64, slice(ch, ch + 1))
            print(f"tracer denorm channel {ch}: engine vs fp64 oracle {err:.3e}")
            assert err < FIXER_GATES["single"]
            assert float(np.abs(r64[ch] - y[ch]).max()) > 0.1                # it clamps
            if ch in (3, 4):
                np.testing.assert_array_equal(bits(got[ch]), bits(r32[ch]))


# ------------------------------------------------------------------------------------------- the reference's two-frame golden
@pytest.mark.parametrize("midpoint", [False, True])
def test_fixers_read_the_last_of_two_frames_golden(midpoint):
    from test_fixers_gpu import demo_latlon
    g = np.load(FRAMES2_GOLD)
    tag = "mid" if midpoint else "trapz"
    x2, y, nl = frames2_variant(g, midpoint)
    lat2d, lon2d, p = demo_latlon()
    ns = 6 * 3600.0
    rad = [4 * nl + k for k in range(6)]
    xd = x2.contiguous().cuda()            # [C_in, frames = 2, H, W]: two different frames

    def run(build):
        pb = WXPostBlock(10, 18, 4 * nl, 2, 4 * nl + 8)
        pb.set_grid(lat2d, lon2d, p, midpoint)
        build(pb)
        return pb.apply(xd, y.clone().cuda()).cpu().numpy()

    ym = run(lambda pb: pb.add_mass_fixer(nl, 3))
    yw = run(lambda pb: pb.add_water_fixer(nl, 4 * nl + 6, 4 * nl + 7, ns))
    ye = run(lambda pb: pb.add_energy_fixer(0, nl, 2 * nl, 3 * nl, rad, np.ones((10, 18), np.float32), ns))

    def chain(pb):
        pb.add_mass_fixer(nl, 3)
        pb.add_water_fixer(nl, 4 * nl + 6, 4 * nl + 7, ns)
        pb.add_energy_fixer(0, nl, 2 * nl, 3 * nl, rad, np.ones((10, 18), np.float32), ns)
    yc = run(chain)
    qs, pr = slice(nl, 2 * nl), 4 * nl + 6
    assert rel(ym[qs], g[f"{tag}_mass"]) < 5e-5
    assert rel(yw[pr], g[f"{tag}_water"]) < 5e-5
    assert rel(ye[:nl], g[f"{tag}_energy"]) < 5e-5
    gc = g[f"{tag}_chain"]
    for got, want, tol in ((yc[:nl], gc[:nl], 1e-4), (yc[qs], gc[nl:2 * nl], 1e-4), (yc[pr], gc[2 * nl], 2e-3)):
        assert rel(got, want) < tol
    np.testing.assert_array_equal(ym[:nl], y[:nl].numpy())
    np.testing.assert_array_equal(yw[:pr], y[:pr].numpy())
    np.testing.assert_array_equal(ye[nl:], y[nl:].numpy())


# ------------------------------------------------------------------------------------------------------- the registry path
# T0F (two input frames) with 8 output-only channels; the 3-D variables deliberately not in the sweep's order
REG = dict(U=0, V=3, T=6, q=9, sp=12, toa=[13, 14], surf_rad=[15, 16], surf_flux=[17, 18], precip=19, evapor=20)


def registry_model_conf(post_conf):
    return dict(image_height=37, image_width=72, frames=2, output_frames=1, channels=4, surface_channels=4, input_only_channels=4,
                output_only_channels=8, levels=3, dim=[32, 64, 128, 256], depth=[1, 1, 2, 1], global_window_size=[4, 2, 2, 1],
                local_window_size=3, patch_width=1, patch_height=1, cross_embed_kernel_sizes=[[4, 8, 16, 32], [2, 4], [2, 4], [2, 4]],
                cross_embed_strides=[2, 2, 2, 2], interp=True, use_spectral_norm=True,
                padding_conf=dict(activate=True, mode="earth", pad_lat=[6, 6], pad_lon=[12, 12]), post_conf=post_conf)


def registry_post_conf(grid_type="pressure", midpoint=False, denorm=True):
    base = dict(activate=True, activate_outside_model=False, denorm=denorm, grid_type=grid_type, midpoint=midpoint, sp_inds=REG["sp"],
                q_inds=[REG["q"] + k for k in range(3)])
    blocks = {f"{v}_inds": [REG[v] + k for k in range(3)] for v in "TUV"}
    return dict(activate=True, data=dict(lead_time_periods=3),
                global_mass_fixer=dict(base, fix_level_num=2),
                global_water_fixer=dict(base, precip_ind=REG["precip"], evapor_ind=REG["evapor"]),
                global_energy_fixer=dict(base, **blocks, TOA_rad_inds=REG["toa"], surf_rad_inds=REG["surf_rad"],
                                         surf_flux_inds=REG["surf_flux"]))


def registry_physics(sigma, midpoint):
    H, W = 37, 72
    lon2d, lat2d = np.meshgrid(np.arange(W, dtype=np.float32) * 5.0, np.linspace(88, -88, H, dtype=np.float32))
    n_p = 4 if midpoint else 3                    # the model carries 3 levels per variable: mid-level values of 4 interfaces
    eta = np.linspace(0.0, 1.0, n_p)
    g = np.random.Generator(np.random.Philox(key=[9, 47]))
    ph = dict(lat2d=lat2d, lon2d=lon2d, gph_surf=(500.0 + 200.0 * g.standard_normal((H, W))).astype(np.float32))
    if sigma:
        ph.update(coef_a=np.round(2000.0 * (1 - eta) + 40000.0 * eta * (1 - eta)).astype(np.float32), coef_b=(eta ** 2).astype(np.float32))
    else:
        ph.update(p_levels=np.round(20000.0 + 80000.0 * eta).astype(np.float32))
    return ph


def registry_stats():
    """Output statistics (set_denorm, 24 channels) and input statistics (set_physics, 20 channels): physical magnitudes per block,
    distinct per channel, and the input ones differ from the output ones on every channel."""
    blk = {REG["T"]: (250.0, 10.0), REG["q"]: (8e-3, 3e-3), REG["U"]: (1.0, 8.0), REG["V"]: (-1.0, 6.0)}
    mo, so = np.zeros(24), np.ones(24)
    for s, (m, d) in blk.items():
        mo[s:s + 3], so[s:s + 3] = m, d
    mo[12], so[12] = 1.0e5, 1.0e3
    mo[13:19], so[13:19] = (1.0 + 0.3 * np.arange(6)) * 1.0e6, 2.0e5
    mo[19], so[19], mo[20], so[20] = 8e-3, 1e-3, -4e-3, 5e-4
    k = np.arange(24)
    mo, so = mo + 0.01 * k * so, so * (1.0 + 0.01 * k)
    mi, si = (mo - 0.4 * so)[:20].copy(), (1.2 * so)[:20].copy()
    mi[13:], si[13:] = 0.2, 1.3
    return tuple(v.astype(np.float32) for v in (mi, si, mo, so))


def registry_model(post_conf):
    from wxengine.config import WXConfig
    from wxengine.model import WXFormerHIP
    from wxengine.synth import synth_state_dict
    mc = registry_model_conf(post_conf)
    cfg = WXConfig.from_model_conf(dict(registry_model_conf(dict(activate=False))))
    m = WXFormerHIP(precision="fp32", **mc).to("cuda").eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg).items()})
    return m, cfg


@pytest.mark.parametrize("grid_type,midpoint", [("pressure", False), ("sigma", True)])
def test_registry_class_runs_the_in_model_fixers(grid_type, midpoint):
    """post_conf.activate = True through WXFormerHIP._build_post: the output is the same model's forward with the post block off,
    followed by the fp64 oracle chain mass -> water -> energy on that y and the LAST frame of x."""
    from wxengine.synth import synth_input
    sigma = grid_type == "sigma"
    mi, si, mo, so = registry_stats()
    ph = registry_physics(sigma, midpoint)
    plain, cfg = registry_model(dict(activate=False))
    assert cfg.frames == 2 and cfg.base_input_channels == 20 and cfg.base_output_channels == 24
    x = torch.from_numpy(synth_input(cfg)).cuda()
    assert not torch.equal(x[0, :, 0], x[0, :, 1])
    with torch.no_grad():
        y_plain = plain(x).clone()
    m, _ = registry_model(registry_post_conf(grid_type, midpoint))
    assert m.use_post_block
    m.set_denorm(mo, so)
    m.set_physics(mean_in=mi, std_in=si, **ph)
    with torch.no_grad():
        y = m(x)
    assert y.shape == y_plain.shape == (1, 24, 1, 37, 72)
    got, y0 = y[0, :, 0].cpu().numpy(), y_plain[0, :, 0].cpu().numpy()

    def chain(dt):
        t = lambda a: torch.from_numpy(np.asarray(a)).to(dt)   # noqa: E731
        stats = {"in": (t(mi), t(si)), "out": (t(mo), t(so))}
        xl, gph, ns = t(x[0, :, -1].cpu().numpy()), t(ph["gph_surf"]), 3 * 3600.0
        toa, surf = [(c, 1.0) for c in REG["toa"]], [(c, 1.0) for c in REG["surf_rad"] + REG["surf_flux"]]
        if sigma:
            grid = F.SigmaGrid(ph["lat2d"], ph["lon2d"], ph["coef_a"], ph["coef_b"], midpoint=midpoint, dtype=dt)
            v = F.mass_fixer_sigma(t(y0), xl, grid, REG["q"], 3, REG["sp"], stats)
            v = F.water_fixer_sigma(v, xl, grid, REG["q"], 3, REG["precip"], REG["evapor"], REG["sp"], ns, stats)
        else:
            grid = F.Grid(ph["lat2d"], ph["lon2d"], ph["p_levels"], midpoint=midpoint, dtype=dt)
            v = F.mass_fixer(t(y0), xl, grid, REG["q"], 3, 2, stats)
            v = F.water_fixer(v, xl, grid, REG["q"], 3, REG["precip"], REG["evapor"], ns, stats)
        return F.energy_fixer_signed(v, xl, grid, REG["T"], REG["q"], REG["U"], REG["V"], 3, toa, surf, gph, ns, stats,
                                     REG["sp"] if sigma else None).numpy()
    r32, r64 = chain(torch.float32), chain(torch.float64)
    own = [(slice(REG["T"], REG["T"] + 3), 1e-4), (slice(REG["precip"], REG["precip"] + 1), 2e-3),
           (slice(REG["sp"], REG["sp"] + 1), 1e-4) if sigma else (slice(REG["q"], REG["q"] + 3), 1e-4)]
    owned = np.zeros(24, bool)
    for blk, gate in own:
        assert fixer_block_error(r32, r64, blk) <= gate / 4                      # the inputs are well conditioned
        assert fixer_block_error(y0, r64, blk) > 20 * gate                       # and the chain has work to do
        err = fixer_block_error(got, r64, blk)
        print(f"registry {grid_type} channels {blk.start}:{blk.stop} engine vs fp64 oracle {err:.3e} (gate {gate:g})")
        assert err < gate
        owned[blk] = True
    np.testing.assert_array_equal(bits(got[~owned]), bits(y0[~owned]))


def test_registry_class_refuses_incomplete_physics():
    from wxengine.synth import synth_input
    mi, si, mo, so = registry_stats()
    ph = registry_physics(False, False)
    m, cfg = registry_model(registry_post_conf())
    x = torch.from_numpy(synth_input(cfg)).cuda()
    with pytest.raises(WXEngineError, match="set_physics"):                      # fixers active, no grid
        m(x)
    m.set_physics(**ph)
    with pytest.raises(WXEngineError, match="denorm fixers need"):               # denorm, neither set_denorm nor input statistics
        m(x)
    m.set_denorm(mo, so)
    with pytest.raises(WXEngineError, match="denorm fixers need"):               # ... output statistics alone are not enough
        m(x)
    m.set_physics(**dict(ph, p_levels=None), mean_in=mi, std_in=si)
    with pytest.raises(WXEngineError, match="p_levels"):
        m(x)
    for key, other, word in (("midpoint", True, "midpoint"), ("grid_type", "sigma", "grid_type")):
        pc = registry_post_conf()
        pc["global_water_fixer"][key] = other
        bad, _ = registry_model(pc)
        bad.set_denorm(mo, so)
        bad.set_physics(mean_in=mi, std_in=si, **ph)
        with pytest.raises(ValueError, match=word):
            bad(x)
    with pytest.raises(ValueError, match="grid_type"):
        pc = registry_post_conf()
        pc["global_mass_fixer"]["grid_type"] = "height"
        registry_model(pc)[0](x)
