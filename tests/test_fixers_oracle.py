"""The fixer oracle (oracle/fixers_oracle.py) against the reference's GlobalMass/Water/EnergyFixer on its own
simple_demo grid (tests/golden/fixers_demo.npz, produced by tools/make_goldens.py --only fixers)."""
import os

import numpy as np
import pytest
import torch

from oracle import fixers_oracle as F

GOLD = os.path.join(os.path.dirname(__file__), "golden", "fixers_demo.npz")


def demo_grid(midpoint, dtype=torch.float32):
    lat = np.array([90, 70, 50, 30, 10, -10, -30, -50, -70, -90], dtype=np.float64)
    lon = np.arange(0, 360, 20, dtype=np.float64)
    lon2d, lat2d = np.meshgrid(lon, lat)
    p = np.array([100, 30000, 50000, 70000, 80000, 90000, 100000], dtype=np.float64)
    return F.Grid(lat2d, lon2d, p, midpoint=midpoint, dtype=dtype)


def variant(g, midpoint):
    L = 7
    nl = L - 1 if midpoint else L
    x = np.concatenate([g["x"][b * L:b * L + nl] for b in range(4)], 0)[:, -1]
    y = np.concatenate([g["y"][b * L:b * L + nl] for b in range(4)] + [g["y"][28:]], 0)
    return torch.from_numpy(x), torch.from_numpy(y), nl


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("midpoint", [False, True])
def test_fixers_match_reference(midpoint):
    g = np.load(GOLD)
    tag = "mid" if midpoint else "trapz"
    x, y, nl = variant(g, midpoint)
    grid = demo_grid(midpoint)
    gph = torch.ones(10, 18)
    ns = 6 * 3600.0
    ym = F.mass_fixer(y, x, grid, nl, nl, 3)
    yw = F.water_fixer(y, x, grid, nl, nl, 4 * nl + 6, 4 * nl + 7, ns)
    ye = F.energy_fixer(y, x, grid, 0, nl, 2 * nl, 3 * nl, nl, (4 * nl, 4 * nl + 1), (4 * nl + 2, 4 * nl + 3),
                        (4 * nl + 4, 4 * nl + 5), gph, ns)
    yc = F.energy_fixer(F.water_fixer(F.mass_fixer(y, x, grid, nl, nl, 3), x, grid, nl, nl, 4 * nl + 6, 4 * nl + 7, ns),
                        x, grid, 0, nl, 2 * nl, 3 * nl, nl, (4 * nl, 4 * nl + 1), (4 * nl + 2, 4 * nl + 3),
                        (4 * nl + 4, 4 * nl + 5), gph, ns)
    # per-channel-block relative tolerance: the reference sums ~1e18-magnitude global integrals in fp32
    # (order-dependent at ~1e-6); we sum in fp64
    qs = slice(nl, 2 * nl)
    assert rel(ym[qs].numpy(), g[f"{tag}_mass"][qs]) < 5e-5
    assert rel(yw[4 * nl + 6].numpy(), g[f"{tag}_water"][4 * nl + 6]) < 5e-5
    assert rel(ye[:nl].numpy(), g[f"{tag}_energy"][:nl]) < 5e-5
    for blk, tol in ((slice(0, nl), 1e-4), (qs, 1e-4), (slice(4 * nl + 6, 4 * nl + 7), 2e-3)):
        # chained: the water ratio is a small difference of large global integrals of the (mass-fixed) q, so the
        # 1e-7 fp32 noise of that q shows up at ~2e-4 in the precipitation ratio -- in the reference as well
        assert rel(yc[blk].numpy(), g[f"{tag}_chain"][blk]) < tol
    # untouched channels are bit-identical
    np.testing.assert_array_equal(ym[:nl].numpy(), y[:nl].numpy())
    np.testing.assert_array_equal(yw[:4 * nl + 6].numpy(), y[:4 * nl + 6].numpy())


def test_mass_fixer_conserves_dry_air_mass():
    """The property the reference's gen2 test asserts (tests/test_conservation_gen2.py:241-274): after the fix the
    global dry-air mass of the prediction equals that of the input.  Exact for the midpoint rule; with the
    trapezoidal rule the fixed level ind_fix-1 is also the end point of the last 'held' interval, so the reference
    algorithm itself only conserves to ~1e-4 there."""
    g = np.load(GOLD)
    x, y, nl = variant(g, True)
    grid = demo_grid(True, torch.float64)
    x, y = x.double(), y.double()
    yf = F.mass_fixer(y, x, grid, nl, nl, 3)
    m_in = grid.wsum(F.column_integral(1 - x[nl:2 * nl], grid.p, True) / F.GRAVITY)
    m_out = grid.wsum(F.column_integral(1 - yf[nl:2 * nl], grid.p, True) / F.GRAVITY)
    assert abs(float(m_out - m_in)) <= 1e-9 * abs(float(m_in))
    xt, yt, nt = variant(g, False)
    gt = demo_grid(False, torch.float64)
    yft = F.mass_fixer(yt.double(), xt.double(), gt, nt, nt, 3)
    mi = gt.wsum(F.column_integral(1 - xt[nt:2 * nt].double(), gt.p, False) / F.GRAVITY)
    mo = gt.wsum(F.column_integral(1 - yft[nt:2 * nt], gt.p, False) / F.GRAVITY)
    assert abs(float(mo - mi)) <= 1e-3 * abs(float(mi))


def test_cell_area_matches_torch_gradient():
    lat = torch.tensor([90., 70, 50, 30, 10, -10, -30, -50, -70, -90]).view(-1, 1).expand(10, 18)
    lon = torch.arange(0, 360, 20.).view(1, -1).expand(10, 18)
    d_phi = torch.gradient(torch.sin(torch.deg2rad(lat)), dim=0, edge_order=2)[0]
    d_lam = torch.gradient(torch.deg2rad(lon), dim=1, edge_order=2)[0]
    d_lam = (d_lam + torch.pi) % (2 * torch.pi) - torch.pi
    want = torch.abs(F.RAD_EARTH ** 2 * d_phi * d_lam)
    np.testing.assert_allclose(F.cell_area(lat, lon).numpy(), want.numpy(), rtol=2e-5)  # fp32 edge stencils


# ---- hybrid sigma-pressure grid (tests/golden/fixers_sigma.npz, tools/make_goldens.py --only sigma) -----------------
SIGMA_GOLD = os.path.join(os.path.dirname(__file__), "golden", "fixers_sigma.npz")


def sigma_variant(g, midpoint):
    L = 7
    nl = L - 1 if midpoint else L
    H, W = g["gph"].shape
    x = np.concatenate([g["x"][b * L:b * L + nl] for b in range(4)] + [np.zeros((8, 2, H, W), np.float32), g["sp_x"]], 0)[:, -1]
    y = np.concatenate([g["y"][b * L:b * L + nl] for b in range(4)] + [g["y"][28:], g["sp_y"]], 0)
    return torch.from_numpy(x), torch.from_numpy(y), nl


@pytest.mark.parametrize("midpoint", [False, True])
def test_sigma_fixers_match_reference(midpoint):
    g = np.load(SIGMA_GOLD)
    tag = "mid" if midpoint else "trapz"
    x, y, nl = sigma_variant(g, midpoint)
    lat = np.array([90, 70, 50, 30, 10, -10, -30, -50, -70, -90], dtype=np.float64)
    lon2d, lat2d = np.meshgrid(np.arange(0, 360, 20, dtype=np.float64), lat)
    grid = F.SigmaGrid(lat2d, lon2d, g["coef_a"], g["coef_b"], midpoint=midpoint)
    gph = torch.from_numpy(g["gph"])
    ns, sp = 6 * 3600.0, 4 * nl + 8
    rad = ((4 * nl, 4 * nl + 1), (4 * nl + 2, 4 * nl + 3), (4 * nl + 4, 4 * nl + 5))
    ym = F.mass_fixer_sigma(y, x, grid, nl, nl, sp)
    yw = F.water_fixer_sigma(y, x, grid, nl, nl, 4 * nl + 6, 4 * nl + 7, sp, ns)
    ye = F.energy_fixer_sigma(y, x, grid, 0, nl, 2 * nl, 3 * nl, nl, *rad, sp, gph, ns)
    yc = F.energy_fixer_sigma(F.water_fixer_sigma(F.mass_fixer_sigma(y, x, grid, nl, nl, sp), x, grid, nl, nl, 4 * nl + 6,
                                                  4 * nl + 7, sp, ns), x, grid, 0, nl, 2 * nl, 3 * nl, nl, *rad, sp, gph, ns)
    assert rel(ym[sp].numpy(), g[f"{tag}_mass"][sp]) < 5e-6          # surface pressure rescaled
    np.testing.assert_array_equal(ym[:sp].numpy(), y[:sp].numpy())  # q untouched on sigma grids
    assert rel(yw[4 * nl + 6].numpy(), g[f"{tag}_water"][4 * nl + 6]) < 5e-5
    assert rel(ye[:nl].numpy(), g[f"{tag}_energy"][:nl]) < 5e-5
    for blk, tol in ((slice(0, nl), 1e-4), (slice(sp, sp + 1), 1e-5), (slice(4 * nl + 6, 4 * nl + 7), 2e-3)):
        assert rel(yc[blk].numpy(), g[f"{tag}_chain"][blk]) < tol


UPDOWN_GOLD = os.path.join(os.path.dirname(__file__), "golden", "fixers_updown.npz")


def updown_variant(g, midpoint):
    L = 7
    nl = L - 1 if midpoint else L
    x = np.concatenate([g["x"][b * L:b * L + nl] for b in range(4)], 0)[:, -1]
    y = np.concatenate([g["y"][b * L:b * L + nl] for b in range(4)] + [g["flux"]], 0)
    return torch.from_numpy(x), torch.from_numpy(y), nl


@pytest.mark.parametrize("midpoint", [False, True])
def test_energy_updown_matches_reference(midpoint):
    g = np.load(UPDOWN_GOLD)
    tag = "mid" if midpoint else "trapz"
    x, y, nl = updown_variant(g, midpoint)
    ye = F.energy_fixer_updown(y, x, demo_grid(midpoint), 0, nl, 2 * nl, 3 * nl, nl, [4 * nl + k for k in range(9)],
                               torch.ones(10, 18), 6 * 3600.0)
    assert rel(ye[:nl].numpy(), g[f"{tag}_updown"][:nl]) < 5e-5
    np.testing.assert_array_equal(ye[nl:].numpy(), y[nl:].numpy())


# ---- the signed-term energy fixer: pinned to the functions the goldens above pin, bit for bit ---------------------------------
@pytest.mark.parametrize("midpoint", [False, True])
def test_energy_fixer_signed_reproduces_the_pinned_energy_fixers(midpoint):
    g = np.load(GOLD)
    x, y, nl = variant(g, midpoint)
    grid, gph, ns = demo_grid(midpoint), torch.ones(10, 18), 6 * 3600.0
    f0 = 4 * nl
    want = F.energy_fixer(y, x, grid, 0, nl, 2 * nl, 3 * nl, nl, (f0, f0 + 1), (f0 + 2, f0 + 3), (f0 + 4, f0 + 5), gph, ns)
    got = F.energy_fixer_signed(y, x, grid, 0, nl, 2 * nl, 3 * nl, nl, [(f0, 1.0), (f0 + 1, 1.0)], [(f0 + k, 1.0) for k in range(2, 6)], gph, ns)
    assert torch.equal(got, want) and not torch.equal(got, y)
    gu = np.load(UPDOWN_GOLD)
    xu, yu, nl = updown_variant(gu, midpoint)
    flux = [4 * nl + k for k in range(9)]
    want = F.energy_fixer_updown(yu, xu, grid, 0, nl, 2 * nl, 3 * nl, nl, flux, gph, ns)
    got = F.energy_fixer_signed(yu, xu, grid, 0, nl, 2 * nl, 3 * nl, nl, list(zip(flux[:3], (1.0, -1.0, -1.0))),
                                list(zip(flux[3:], (1.0, -1.0, 1.0, -1.0, -1.0, -1.0))), gph, ns)
    assert torch.equal(got, want)
    gs = np.load(SIGMA_GOLD)
    xs, ys, nl = sigma_variant(gs, midpoint)
    lon2d, lat2d = np.meshgrid(np.arange(0, 360, 20, dtype=np.float64), np.array([90, 70, 50, 30, 10, -10, -30, -50, -70, -90.0]))
    sg = F.SigmaGrid(lat2d, lon2d, gs["coef_a"], gs["coef_b"], midpoint=midpoint)
    f0, sp, gph = 4 * nl, 4 * nl + 8, torch.from_numpy(gs["gph"])
    want = F.energy_fixer_sigma(ys, xs, sg, 0, nl, 2 * nl, 3 * nl, nl, (f0, f0 + 1), (f0 + 2, f0 + 3), (f0 + 4, f0 + 5), sp, gph, ns)
    got = F.energy_fixer_signed(ys, xs, sg, 0, nl, 2 * nl, 3 * nl, nl, [(f0, 1.0), (f0 + 1, 1.0)], [(f0 + k, 1.0) for k in range(2, 6)],
                                gph, ns, sp_ind=sp)
    assert torch.equal(got, want)


# ---- two different input frames, and the tracer fixer (tests/golden/fixers_frames2.npz, tools/make_goldens.py --only frames2) ----
FRAMES2_GOLD = os.path.join(os.path.dirname(__file__), "golden", "fixers_frames2.npz")


def frames2_variant(g, midpoint):
    """x [4 nl, 2, H, W] (BOTH frames), y [4 nl + 8, H, W]."""
    L = 7
    nl = L - 1 if midpoint else L
    x = np.concatenate([g["x"][b * L:b * L + nl] for b in range(4)], 0)
    y = np.concatenate([g["y"][b * L:b * L + nl] for b in range(4)] + [g["y"][28:]], 0)
    return torch.from_numpy(x), torch.from_numpy(y), nl


@pytest.mark.parametrize("midpoint", [False, True])
def test_fixers_read_the_last_of_two_frames(midpoint):
    g = np.load(FRAMES2_GOLD)
    tag = "mid" if midpoint else "trapz"
    x2, y, nl = frames2_variant(g, midpoint)
    assert not np.allclose(x2[:, 0].numpy(), x2[:, 1].numpy(), rtol=0.1)
    grid, gph, ns = demo_grid(midpoint), torch.ones(10, 18), 6 * 3600.0
    rad = ((4 * nl, 4 * nl + 1), (4 * nl + 2, 4 * nl + 3), (4 * nl + 4, 4 * nl + 5))

    def run(x):
        ym = F.mass_fixer(y, x, grid, nl, nl, 3)
        yw = F.water_fixer(y, x, grid, nl, nl, 4 * nl + 6, 4 * nl + 7, ns)
        ye = F.energy_fixer(y, x, grid, 0, nl, 2 * nl, 3 * nl, nl, *rad, gph, ns)
        yc = F.energy_fixer(F.water_fixer(ym, x, grid, nl, nl, 4 * nl + 6, 4 * nl + 7, ns), x, grid, 0, nl, 2 * nl, 3 * nl, nl, *rad, gph, ns)
        return ym, yw, ye, yc
    ym, yw, ye, yc = (t.numpy() for t in run(x2[:, -1]))
    qs, pr = slice(nl, 2 * nl), 4 * nl + 6
    assert rel(ym[qs], g[f"{tag}_mass"]) < 5e-5
    assert rel(yw[pr], g[f"{tag}_water"]) < 5e-5
    assert rel(ye[:nl], g[f"{tag}_energy"]) < 5e-5
    gc = g[f"{tag}_chain"]
    for got, want, tol in ((yc[:nl], gc[:nl], 1e-4), (yc[qs], gc[nl:2 * nl], 1e-4), (yc[pr], gc[2 * nl], 2e-3)):
        assert rel(got, want) < tol
    # the golden tells the frames apart: frame 0 misses every gate by orders of magnitude
    zm, zw, ze, _ = (t.numpy() for t in run(x2[:, 0]))
    assert min(rel(zm[qs], g[f"{tag}_mass"]), rel(zw[pr], g[f"{tag}_water"]), rel(ze[:nl], g[f"{tag}_energy"])) > 1e-2


def test_tracer_fixer_matches_reference():
    g = np.load(FRAMES2_GOLD)
    y = torch.from_numpy(g["y"])
    inds = [int(i) for i in g["tracer_inds"]]
    got = F.tracer_fixer(y, inds, g["tracer_thres"], g["tracer_thres_max"])
    assert np.array_equal(got[inds].numpy().view(np.int32), g["tracer"].view(np.int32))
    assert int((got != y).sum()) > 100                                        # it clamps on both sides ...
    other = [c for c in range(y.shape[0]) if c not in inds]
    assert torch.equal(got[other], y[other])                                  # ... only the listed channels
    lo_only = F.tracer_fixer(y, inds, g["tracer_thres"])
    assert torch.equal(torch.minimum(lo_only[inds], torch.from_numpy(g["tracer_thres_max"]).float().view(-1, 1, 1)), got[inds])
    # signed zero at an upper threshold of 0: `>=` replaces -0.0 by the threshold, as the reference's masked assignment does
    z = F.tracer_fixer(torch.tensor([[[-0.0, 0.0, -1.0, 1.0]]]), [0], [-5.0], [0.0])
    assert z.numpy().view(np.int32).ravel().tolist() == [0, 0, np.float32(-1.0).view(np.int32), 0]
    # de-normalised clamp: thresholds are physical values
    st = {"out": (torch.tensor([2.0]), torch.tensor([4.0]))}
    d = F.tracer_fixer(torch.tensor([[[-1.0, 0.0, 1.0]]]), [0], [0.0], [4.0], st)     # physical -2, 2, 6 -> 0, 2, 4
    assert d.ravel().tolist() == [-0.5, 0.0, 0.5]


# ---- conditioning of the device sweep's cases (tests/synth_batches.py::FIXER_CASES, run on the GPU by test_fixers_sweep_gpu.py) ----
from synth_batches import FIXER_CASES, fixer_block_error, fixer_case_inputs, fixer_case_oracle, fixer_case_owned, fixer_case_terms  # noqa: E402


@pytest.mark.parametrize("name", list(FIXER_CASES))
def test_sweep_case_is_well_conditioned(name):
    """The oracle in fp32 (fp32 grid, as the reference computes) and in fp64 agree to a QUARTER of the case's gate on every block a
    fixer owns: what the GPU test then measures against the fp64 oracle is the engine, not the inputs."""
    inp = fixer_case_inputs(name)
    y32 = fixer_case_oracle(inp, torch.float32)
    y64 = fixer_case_oracle(inp, torch.float64)
    assert y32.dtype == torch.float32 and y64.dtype == torch.float64 and bool(torch.isfinite(y64).all())
    owned = np.zeros(y64.shape[0], bool)
    for blk, gate in fixer_case_owned(inp):
        err = fixer_block_error(y32.numpy(), y64.numpy(), blk)
        print(f"{name} channels {blk.start}:{blk.stop} fp32 vs fp64 oracle {err:.3e} (gate {gate:g})")
        assert err <= gate / 4
        assert fixer_block_error(inp["y"], y64.numpy(), blk) > 20 * gate          # the fixer moves its block far beyond the gate
        owned[blk] = True
    assert np.array_equal(y64.numpy()[~owned], inp["y"][~owned].astype(np.float64))
    terms = fixer_case_terms(inp)
    if terms and len(terms[1]) > 1:     # every flux term counts: without the last surface term T moves by several gates
        short = fixer_case_oracle(inp, torch.float64, terms=(terms[0], terms[1][:-1]))
        blk, gate = next(b for b in fixer_case_owned(inp) if b[0].start == 0)
        assert fixer_block_error(short.numpy(), y64.numpy(), blk) > 4 * gate


def test_sweep_table_moves_every_axis_on_every_grid():
    for grid in ("G9", "G257"):
        for sigma in (False, True):
            cs = [c for c in FIXER_CASES.values() if c["grid"] == grid and c["sigma"] == sigma]
            assert {c["fixer"] for c in cs} >= {"mass", "water", "energy", "signed48", "chain"}
            assert {c["midpoint"] for c in cs} == {False, True} and {c["denorm"] for c in cs} == {False, True}
            assert {c["frames"] for c in cs} == {1, 2, 3} and {c["levels"] for c in cs} >= {2, 13}
            if not sigma:
                assert {c["fix"] for c in cs if c["fixer"] == "mass"} >= {2, 3, 13}
    g9 = [c for c in FIXER_CASES.values() if c["grid"] == "G9"]
    assert {c["fixer"] for c in g9} >= {"updown", "signed11"} and {c["orient"] for c in g9} == {"ns", "sn", "wrap"}
    assert any(c["levels"] == 64 and c["fix"] == 64 for c in g9) and any(c["levels"] == 64 and c["fix"] == 2 for c in g9)
    assert all(c["fix"] >= 2 for c in FIXER_CASES.values())
