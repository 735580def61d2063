"""Lat-band sharding on the GPU: one forecast split over n ranks must reproduce the unsharded engine.

The oracle here is the UNSHARDED engine (itself pinned to the reference's goldens in test_engine_gpu.py): sharding may only
change the fp32 summation order of the GroupNorm statistics (summed per rank, then in rank order) and, in bf16, which
LayerNorm statistics path feeds a GEMM -- so
  fp32 engine:  max|y_sharded - y| <= 1e-5 * max|y|   (observed <= 1e-6; the reference's own sharded-vs-unsharded gate is
                atol 1e-5 per layer, tests/test_domain_parallel_multigpu.py:115,160,246)
  bf16 engine:  rel-L2 <= 1e-2 and max err <= 5e-2 * max|y| (observed 4e-3 .. 6e-3 / 7e-3).  In bf16 an fp32-ulp difference
                in one GroupNorm scale flips a few bf16 roundings, and those flips compound through the remaining layers, so
                two bf16 runs that differ anywhere agree only to the bf16 noise level; the fp32 rows prove the algorithm.
Ranks are VIRTUAL (n engines in this process on the one GPU, exchanges = device copies of the staging slices) except in the
last test, which runs two real processes over torch.distributed (gloo, host-staged) on the same GPU."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from wxengine.config import named_config
from wxengine.engine import WXEngine, WXEngineError
from wxengine.latband import BandRank, DistBand, VirtualBands, split_rows
from wxengine.synth import synth_denorm, synth_forcing, synth_input, synth_state_dict

pytestmark = pytest.mark.gpu


def _layout(cfg):
    n_prog = cfg.channels * cfg.levels + cfg.surface_channels
    n_dyn = min(2, cfg.base_input_channels - n_prog)
    return n_prog, cfg.base_input_channels - n_prog - n_dyn, n_dyn


def _setup(cfg):
    mean, std = synth_denorm(cfg.base_output_channels)
    n_prog, n_static, n_dyn = _layout(cfg)

    def f(e):
        e.set_denorm(mean, std)
        e.set_layout(n_prog, n_static, n_dyn)
    return f


def _reference(cfg, sd, prec):
    eng = WXEngine(cfg, prec, 0)
    eng.load_state_dict(sd)
    eng.finalize()
    _setup(cfg)(eng)
    return eng


def _close(a, b, prec, l2_tol=1e-2, max_tol=5e-2, fp32_tol=1e-5):
    a, b = a.double(), b.double()
    scale = b.abs().max().item()
    err = (a - b).abs().max().item()
    assert torch.isfinite(a).all()
    if prec == "fp32":
        assert err <= fp32_tol * scale, f"fp32 sharded vs unsharded: {err:.3e} (scale {scale:.3e})"
    elif prec == "fp32s":
        # split-bf16 arithmetic: a band rank's stage-0 CrossEmbed runs the exact-f32 patch kernel (its input planes are not split) and
        # its GEMM tiles group rows differently, so the two runs differ by the mode's own product error (~1e-5), not by summation order
        assert err <= 5e-5 * scale, f"fp32s sharded vs unsharded: {err:.3e} (scale {scale:.3e})"
    else:
        l2 = ((a - b).norm() / b.norm()).item()
        assert l2 <= l2_tol and err <= max_tol * scale, f"bf16 sharded vs reference: rel-L2 {l2:.3e} max {err:.3e} (scale {scale:.3e})"


@pytest.mark.parametrize("name,prec,n", [("T0", "fp32", 2), ("T0", "fp32", 3), ("T1", "fp32", 3), ("T1", "fp32", 8), ("T1", "bf16", 2), ("T1", "fp32s", 3), ("C1", "fp32s", 5),
                                         ("C1", "fp32", 5), ("C1", "bf16", 4), ("T0W", "fp32", 2), ("T0W", "fp32", 3), ("C1W", "fp32", 4),
                                         ("C1W", "bf16", 5)])
def test_sharded_step_equals_unsharded(name, prec, n):
    """Ragged bands (T1/3, C1/5), ranks that own no rows at the deepest stages (T0, T1/8) or no grid rows at all because their
    band is pole padding (T1/8), y / y_phys / x_next of wx_step."""
    cfg = named_config(name)
    sd = synth_state_dict(cfg)
    x = torch.from_numpy(synth_input(cfg)).cuda()
    n_dyn = _layout(cfg)[2]
    frc = torch.from_numpy(synth_forcing(cfg, n_dyn, 1)).cuda() if n_dyn else None
    y0, p0, x0 = _reference(cfg, sd, prec).step(x, frc)
    vb = VirtualBands(cfg, sd, n, prec, setup=_setup(cfg))
    assert vb.starts[0] == 0 and vb.starts[-1] == cfg.image_height
    y, p, xn = vb.step(x, frc, want_phys=True, want_next=True)
    _close(y, y0, prec)
    _close(p, p0, prec)
    _close(xn, x0, prec)
    n_prog, n_static, _ = _layout(cfg)
    # static and forcing channels of x_next are copies: exact
    assert torch.equal(xn[:, n_prog:n_prog + n_static], x[:, n_prog:n_prog + n_static])
    if n_dyn:
        assert torch.equal(xn[:, n_prog + n_static:], frc)
    if n > 1:
        assert vb.exchanged_bytes > 0


@pytest.mark.parametrize("name,prec,n", [("T1", "fp32", 3), ("C1", "bf16", 4), ("C1W", "fp32", 4)])
def test_overlapped_exchanges_are_bit_identical(name, prec, n, monkeypatch):
    """Comm / compute overlap (wx_band_comm_stream): exchanges on a second stream between two events while the interior rows of the
    3x3 convolution behind a halo exchange are computed.  (a) asynchronous device copies on a side stream give the SAME bits as
    copies on the compute stream -- a missing event edge shows up here as a stale halo row; repeated to give a race a chance;
    (b) the interior / boundary split changes only the partition of the GroupNorm tile partials: against the default (unsplit)
    program the difference stays at summation noise."""
    cfg = named_config(name)
    sd = synth_state_dict(cfg)
    x = torch.from_numpy(synth_input(cfg)).cuda()
    monkeypatch.setenv("WX_BAND_SPLIT", "1")     # the split program, exchanges on the compute stream
    sync = VirtualBands(cfg, sd, n, prec, setup=_setup(cfg))
    monkeypatch.delenv("WX_BAND_SPLIT")
    y_sync = sync.step(x)[0].clone()
    asy = VirtualBands(cfg, sd, n, prec, setup=_setup(cfg), async_copies=True)   # wx_band_comm_stream switches the split on
    for _ in range(4):
        y_async = asy.step(x)[0]
        torch.cuda.synchronize()
        assert torch.equal(y_async, y_sync)
    whole = VirtualBands(cfg, sd, n, prec, setup=_setup(cfg))     # default: unsplit program
    y_whole = whole.step(x)[0]
    _close(y_sync, y_whole, prec, l2_tol=8e-3)

    def conv3_launches(vb):   # is the split taken?  it launches the 3x3 convolutions as interior + two boundary rows
        for b in vb.ranks:
            b.eng.profile(1)
        vb.step(x)
        torch.cuda.synchronize()
        return sum(r["launches"] for b in vb.ranks for r in b.eng.profile_read() if r["name"] == "gemm_conv3")
    assert conv3_launches(sync) > conv3_launches(whole)


@pytest.mark.parametrize("key", ["w2", "w3", "w1", "w16", "w5p"])
def test_odd_geometries_engine_vs_oracle_and_sharded(key):
    """Window / pad combinations outside the BASELINE family: the unsharded fp32 engine against the CPU oracle (1e-4 * max|y|),
    then 2 and 3 lat-band ranks against the unsharded engine (1e-5 * max|y|)."""
    from oracle import wxformer_oracle as O
    from synth_batches import ODD_CONFIGS, odd_config
    cfg = odd_config(**ODD_CONFIGS[key])
    sd = synth_state_dict(cfg)
    x = synth_input(cfg)
    y_ref = O.forward(cfg, sd, x)
    eng = WXEngine(cfg, "fp32", 0)
    eng.load_state_dict(sd)
    eng.finalize()
    xg = torch.from_numpy(x).cuda()
    y0 = eng.forward(xg)
    err = (y0.cpu() - y_ref).abs().max().item()
    assert err <= 1e-4 * y_ref.abs().max().item(), f"{key}: engine vs oracle {err:.3e}"
    for n in (2, 3):
        if n > cfg.stage_hw[0][0] // cfg.local_window_size[0]:
            continue
        y, _, _ = VirtualBands(cfg, sd, n, "fp32").step(xg)
        _close(y, y0, "fp32")


def test_baseline_config4_geometry_eight_ranks_fp32():
    """BASELINE config 4: the 0.25-degree model over 8 ranks (ragged stage-1/2 bands, three ranks without stage-3 rows),
    fp32 engine so that the comparison is not blurred by bf16: sharded == unsharded to 1e-5 * max|y| (observed 1.5e-6)."""
    cfg = named_config("C3")
    sd = synth_state_dict(cfg)
    x = torch.from_numpy(synth_input(cfg)).cuda()
    ref = WXEngine(cfg, "fp32", 0)
    ref.load_state_dict(sd)
    ref.finalize()
    y0 = ref.forward(x).clone()
    del ref
    vb = VirtualBands(cfg, sd, 8, "fp32")
    assert vb.starts == [0, 61, 161, 261, 361, 461, 561, 661, 721]
    y, _, _ = vb.step(x)
    _close(y, y0, "fp32")
    assert 1.5e9 < vb.exchanged_bytes < 3.5e9          # ~3.2 GB in fp32 (1.6 GB in bf16) cross the ranks per step
    del vb
    torch.cuda.empty_cache()


def test_baseline_config4_geometry_eight_ranks_bf16_vs_unsharded_and_reference_golden():
    """The same 8-rank split at the BENCHMARK dtype: the sharded bf16 forecast agrees with the unsharded bf16 engine to bf16
    noise (two bf16 runs that differ in one GroupNorm ulp decorrelate at that level) AND -- in the same test -- with the
    reference's own fp32 CPU output (tests/golden/model_C3.npz, strided samples + per-channel sums) inside the single-step
    bf16 bar of tests/test_engine_gpu.py.  Observed: 6.7e-3 vs the unsharded engine, 8.6e-3 vs the reference."""
    import os
    cfg = named_config("C3")
    sd = synth_state_dict(cfg)
    x = torch.from_numpy(synth_input(cfg)).cuda()
    ref = WXEngine(cfg, "bf16", 0)
    ref.load_state_dict(sd)
    ref.finalize()
    y0 = ref.forward(x).clone()
    del ref
    vb = VirtualBands(cfg, sd, 8, "bf16")
    y, _, _ = vb.step(x)
    _close(y, y0, "bf16")
    assert 0.7e9 < vb.exchanged_bytes < 1.8e9
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "model_C3.npz"))
    st = int(g["stride"])
    got = y[0, :, 0, ::st, ::st].double().cpu().numpy()
    want = g["y"].astype(np.float64)
    l2 = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert l2 <= 2e-2 and np.abs(got - want).max() <= 5e-2 * np.abs(want).max(), f"sharded bf16 vs reference golden: rel-L2 {l2:.3e}"
    del vb
    torch.cuda.empty_cache()


def test_sharded_rollout_feeds_bands_back():
    """3 steps: every rank keeps only its own band of x between steps (no gather in the loop)."""
    cfg = named_config("T1")
    sd = synth_state_dict(cfg)
    ref = _reference(cfg, sd, "fp32")
    vb = VirtualBands(cfg, sd, 3, "fp32", setup=_setup(cfg))
    x = torch.from_numpy(synth_input(cfg)).cuda()
    xs = x.clone()
    n_dyn = _layout(cfg)[2]
    for t in range(1, 4):
        frc = torch.from_numpy(synth_forcing(cfg, n_dyn, t)).cuda()
        y0, _, x = ref.step(x, frc, want_phys=False)
        y, _, xs = vb.step(xs, frc, want_next=True)
        _close(y, y0, "fp32")
    _close(xs, x, "fp32")


def _physics(cfg, row0=None, rows=None, denorm=False):
    """mass + water + energy fixers on a pressure-level grid (gen1.py:280-1030), optionally restricted to a band"""
    from wxengine.engine import WXPostBlock
    H, W, L = cfg.image_height, cfg.image_width, cfg.levels
    n_up = cfg.channels * L
    pb = WXPostBlock(H, W, cfg.base_input_channels, 1, cfg.base_output_channels)
    if row0 is not None:
        pb.set_band(row0, rows)
    lat = np.linspace(89.0, -89.0, H, dtype=np.float32)
    lon = np.arange(W, dtype=np.float32) * (360.0 / W)
    lon2d, lat2d = np.meshgrid(lon, lat)
    pb.set_grid(lat2d, lon2d, np.linspace(5000.0, 100000.0, L).astype(np.float32), False)
    if denorm:   # physical magnitudes: U, V ~ 5 m/s, T ~ 250 K, q ~ 4 g/kg, fluxes small against the column energy
        def stats(nch):
            m, sd = np.zeros(nch, np.float32), np.full(nch, 1e-2, np.float32)
            m[:2 * L], sd[:2 * L] = 0.0, 5.0
            m[2 * L:3 * L], sd[2 * L:3 * L] = 250.0, 10.0
            m[3 * L:4 * L], sd[3 * L:4 * L] = 4e-3, 5e-4
            return m, sd
        (mi, si), (mo, so) = stats(cfg.base_input_channels), stats(cfg.base_output_channels)
        pb.set_stats(mi, si, mo, so)
    gph = (np.random.default_rng(7).uniform(0.0, 3.0e4, (H, W))).astype(np.float32)
    extra = cfg.base_output_channels - n_up - cfg.surface_channels       # diagnostic channels after the surface block
    assert extra >= 2
    d0 = n_up + cfg.surface_channels
    pb.add_mass_fixer(3 * L, 2, denorm)
    pb.add_water_fixer(3 * L, d0, d0 + 1, 21600.0, denorm)
    rad = [n_up, n_up + 1, n_up + 2, n_up + 3, d0, d0 + 1]
    pb.add_energy_fixer(2 * L, 3 * L, 0, L, rad, gph, 21600.0, denorm)
    return pb


@pytest.mark.parametrize("name,n,denorm", [("T1", 3, True), ("C1", 4, True)])
def test_sharded_conservation_fixers(name, n, denorm):
    """The post block's global integrals under sharding: local sums, every rank's sums to everyone, added in rank order.
    fp32 engine.  The correction ratios are fp64 sums rounded to fp32, so a different summation order moves a ratio by one
    fp32 ulp; the mass fixer then rewrites q as 1 - (1 - q) * ratio, where one ulp of a number near 1 (6e-8) is 1.2e-4 in units
    of std(q) = 5e-4 -- that conditioning is the reference's own (gen1.py:372-391).  Observed: 1.2e-4 on the two fixed q levels,
    <= 6e-6 elsewhere; tolerance 5e-4 * max|y|."""
    cfg = named_config(name)
    sd = synth_state_dict(cfg)
    x = torch.from_numpy(synth_input(cfg)).cuda()
    n_dyn = _layout(cfg)[2]
    frc = torch.from_numpy(synth_forcing(cfg, n_dyn, 1)).cuda()
    ref = _reference(cfg, sd, "fp32")
    y_plain, _, _ = ref.step(x, frc)
    pb0 = _physics(cfg, denorm=denorm)
    ref.attach_postblock(pb0)
    y0, p0, x0 = ref.step(x, frc)
    assert not torch.equal(y0, y_plain)
    keep = []

    def factory(r, row0, rows):
        keep.append(_physics(cfg, row0, rows, denorm))
        return keep[-1]
    vb = VirtualBands(cfg, sd, n, "fp32", setup=_setup(cfg), post_factory=factory)
    assert vb.ranks[0].num_exchanges == VirtualBands(cfg, sd, n, "fp32", setup=_setup(cfg)).ranks[0].num_exchanges + 3
    y, p, xn = vb.step(x, frc, want_phys=True, want_next=True)
    _close(y, y0, "fp32", fp32_tol=5e-4)
    _close(p, p0, "fp32", fp32_tol=5e-4)
    _close(xn, x0, "fp32", fp32_tol=5e-4)
    other = [c for c in range(cfg.base_output_channels) if not 3 * cfg.levels <= c < 4 * cfg.levels]
    _close(y[:, other], y0[:, other], "fp32", fp32_tol=2e-5)
    with pytest.raises(WXEngineError, match="latitude band"):
        keep[0].apply(x[0], y[0, :, 0].clone())      # a band block cannot run on its own


def test_band_mode_guards():
    cfg = named_config("T0")
    sd = synth_state_dict(cfg)
    eng = WXEngine(cfg, "fp32", 0)
    eng.load_state_dict(sd)
    with pytest.raises(WXEngineError, match="finalize"):
        BandRank(eng, 0, 2)
    eng.finalize()
    with pytest.raises(WXEngineError, match="bad rank"):
        BandRank(eng, 2, 2)
    band = BandRank(eng, 0, 2)
    x = torch.from_numpy(synth_input(cfg)).cuda()
    with pytest.raises(WXEngineError, match="lat-band mode"):
        eng.forward(x)                      # the whole-grid entry points are closed on a band engine
    with pytest.raises(WXEngineError, match="no exchange is pending"):
        band.resume()
    with pytest.raises(WXEngineError, match="already enabled"):
        BandRank(eng, 0, 2)
    xb = split_rows(x, [band.row0, band.row0 + band.rows])[0]
    xid = band.begin(xb, None, torch.empty(band.band_shape(cfg.base_output_channels), device="cuda"))
    assert xid == 0 and band.messages(0)[0]  # rank 0 of 2 owes rank 1 the rows under its halo
    with pytest.raises(WXEngineError, match="still waiting"):
        band.begin(xb)
    w = WXEngine(named_config("T0U"), "fp32", 0)
    w.load_state_dict(synth_state_dict(named_config("T0U")))
    w.finalize()
    with pytest.raises(WXEngineError, match="upsample_v_conv"):
        BandRank(w, 0, 2)


def test_rccl_transport_world_of_one():
    """The in-engine RCCL driver (dlopen'd librccl, ncclCommInitRank, whole step in one C call) on the one GPU we have: a
    communicator of one rank, so the grouped send/recv lists are empty -- what this pins is the binding, the communicator
    life cycle and the segment loop; the message lists themselves are the ones the gloo tests move."""
    cfg = named_config("T1")
    sd = synth_state_dict(cfg)
    x = torch.from_numpy(synth_input(cfg)).cuda()
    frc = torch.from_numpy(synth_forcing(cfg, _layout(cfg)[2], 1)).cuda()
    y0, p0, x0 = _reference(cfg, sd, "fp32").step(x, frc)
    eng = _reference(cfg, sd, "fp32")
    db = DistBand(eng, transport="rccl")
    assert db.transport == "rccl" and db.rows == (0, cfg.image_height)
    xb, fb = x[0, :, 0].contiguous(), frc[0, :, 0].contiguous()
    yp, xn = torch.empty_like(y0[0, :, 0]), torch.empty_like(xb)
    for _ in range(2):
        y, yp, xn = db.step(xb, fb, y_phys=yp, x_next=xn)
    _close(y, y0[0, :, 0], "fp32")
    _close(yp, p0[0], "fp32")
    _close(xn, x0[0, :, 0], "fp32")


# ---- two real processes over torch.distributed on the one GPU ---------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    cfg = named_config("T1")
    sd = synth_state_dict(cfg)
    eng = WXEngine(cfg, "fp32", 0)
    eng.load_state_dict(sd)
    eng.finalize()
    _setup(cfg)(eng)
    db = DistBand(eng)
    r0, rows = db.rows
    x = torch.from_numpy(synth_input(cfg)).cuda()
    n_dyn = _layout(cfg)[2]
    frc = torch.from_numpy(synth_forcing(cfg, n_dyn, 1)).cuda()
    xb = x[0, :, 0, r0:r0 + rows].contiguous()
    fb = frc[0, :, 0, r0:r0 + rows].contiguous()
    xn = torch.empty_like(xb)
    y, _, xn = db.step(xb, fb, x_next=xn)
    torch.cuda.synchronize()
    q.put((rank, r0, rows, y.cpu().numpy(), xn.cpu().numpy(), db.exchanged_bytes))
    dist.barrier()
    dist.destroy_process_group()


def test_two_processes_gloo_on_one_gpu():
    world = 2
    cfg = named_config("T1")
    sd = synth_state_dict(cfg)
    x = torch.from_numpy(synth_input(cfg)).cuda()
    frc = torch.from_numpy(synth_forcing(cfg, _layout(cfg)[2], 1)).cuda()
    y0, _, x0 = _reference(cfg, sd, "fp32").step(x, frc, want_phys=False)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert res[0][1] == 0 and res[0][1] + res[0][2] == res[1][1] and res[1][1] + res[1][2] == cfg.image_height
    y = torch.from_numpy(np.concatenate([r[3] for r in res], axis=1))
    xn = torch.from_numpy(np.concatenate([r[4] for r in res], axis=1))
    _close(y, y0[0, :, 0].cpu(), "fp32")
    _close(xn, x0[0, :, 0].cpu(), "fp32")
    assert all(r[5] > 0 for r in res)


# ---- two real processes, one GPU each, RCCL inside the engine -----------------------------------------------------------
def _worker_rccl(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    cfg = named_config("T1")
    sd = synth_state_dict(cfg)
    eng = WXEngine(cfg, "fp32", rank)
    eng.load_state_dict(sd)
    eng.finalize()
    _setup(cfg)(eng)
    db = DistBand(eng)                       # nccl backend -> transport "rccl": grouped ncclSend / ncclRecv issued by the engine
    assert db.transport == "rccl"
    r0, rows = db.rows
    x = torch.from_numpy(synth_input(cfg)).cuda()
    n_dyn = _layout(cfg)[2]
    frc = torch.from_numpy(synth_forcing(cfg, n_dyn, 1)).cuda()
    xb = x[0, :, 0, r0:r0 + rows].contiguous()
    fb = frc[0, :, 0, r0:r0 + rows].contiguous()
    xn = torch.empty_like(xb)
    for _ in range(2):                        # twice: the second step reuses the communicator and the staging buffers
        y, _, xn = db.step(xb, fb, x_next=xn)
    torch.cuda.synchronize()
    q.put((rank, r0, rows, y.cpu().numpy(), xn.cpu().numpy(), db.sent_bytes_per_step))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: RCCL refuses two ranks on one device")
def test_two_processes_rccl_two_gpus():
    """The multi-rank branch of wx_band_step_rccl (grouped ncclSend / ncclRecv per exchange, csrc/wx_engine.hip) with a REAL peer
    over xGMI: every earlier test of that driver ran a communicator of one.  Skipped on the single-GPU boxes of this round."""
    world = 2
    cfg = named_config("T1")
    sd = synth_state_dict(cfg)
    x = torch.from_numpy(synth_input(cfg)).cuda()
    frc = torch.from_numpy(synth_forcing(cfg, _layout(cfg)[2], 1)).cuda()
    y0, _, x0 = _reference(cfg, sd, "fp32").step(x, frc, want_phys=False)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_rccl, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=900) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert res[0][1] == 0 and res[0][1] + res[0][2] == res[1][1] and res[1][1] + res[1][2] == cfg.image_height
    y = torch.from_numpy(np.concatenate([r[3] for r in res], axis=1))
    xn = torch.from_numpy(np.concatenate([r[4] for r in res], axis=1))
    _close(y, y0[0, :, 0].cpu(), "fp32")
    _close(xn, x0[0, :, 0].cpu(), "fp32")
    assert all(r[5] > 0 for r in res)
