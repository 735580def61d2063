"""The TISR forcing on the device (csrc/wx_tisr.h, wxengine/tisr.py) against the fixtures of the reference's own functions.

The bar is derived, not chosen: per case, max|device - ref64| <= E_ref = max|ref32 - ref64| of that case -- the device result may be no
further from the reference's fp64 evaluation (on the same float32 days and float32 TSI) than the reference's own float32 result is --
and hence max|device - ref32| <= 2 E_ref.  Errors are absolute and over every plane of the case: a relative error means nothing at the
terminator.  Every case goes through the raw C ABI and through TISRForcing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from tisr_cases import NS_PER_HOUR, TISR_CASES, load_golden, load_tsi, period_ns, times_ns  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SRC = "ERA5"
_cache = {}


def golden(name):
    if name not in _cache:
        _cache[name] = load_golden(name, GOLD)
    return _cache[name]


@pytest.fixture(scope="module")
def lib():
    from wxengine.engine import load_library
    return load_library()


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def create(lib, lat, lon, tt, tv, ny=None, nx=None, n_tsi=None, device=0):
    keep = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (lat, lon, tt, tv)]
    h = C.c_void_p()
    st = lib.wx_tisr_create(lat.shape[0] if ny is None else ny, lat.shape[1] if nx is None else nx, *[None if a is None else fptr(a) for a in keep[:2]],
                            len(tt) if n_tsi is None else n_tsi, *[None if a is None else fptr(a) for a in keep[2:]], device, C.byref(h))
    return st, h, lib.wx_last_error().decode() if st else ""


def compute(lib, h, ns, period, n_steps, dst, stride):
    arr = (C.c_int64 * max(len(ns), 1))(*ns)
    st = lib.wx_tisr_compute(h, len(ns), arr, period, n_steps, C.c_void_p(dst.data_ptr()), stride,
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return st, lib.wx_last_error().decode() if st else ""


def forcing_of(name, **over):
    from wxengine.tisr import TISRForcing
    c, f = TISR_CASES[name], golden(name)
    tt, tv = load_tsi(GOLD)
    grid = dict(lat=f["lat"], lon=f["lon"]) if c.get("curvilinear") else dict(lat_spec=c["lat_spec"], lon_spec=c["lon_spec"])
    return TISRForcing(tt, tv, **dict(dict(integration_period=period_ns(name), num_integration_steps=c["n_steps"], source_name=SRC, **grid), **over))


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_bar(name, got, how):
    f = golden(name)
    assert got.dtype == np.float32 and got.shape == f["ref64"].shape, (name, how, got.shape)
    e_ref = float(f["E_ref"])
    d64 = float(np.abs(got.astype(np.float64) - f["ref64"]).max())
    d32 = float(np.abs(got.astype(np.float64) - f["ref32"].astype(np.float64)).max())
    print(f"[tisr gpu] {name} ({how}): {got.shape[0]} plane(s), to ref64 {d64 / e_ref:.3f} E_ref, to ref32 {d32 / e_ref:.3f} E_ref "
          f"(E_ref {e_ref:.3e} J/m2, {e_ref / f['ref64'].max():.2e} of the maximum)")
    assert d64 <= e_ref, (name, how, d64, e_ref)
    assert d32 <= 2.0 * e_ref, (name, how, d32, e_ref)


@pytest.mark.parametrize("name", list(TISR_CASES))
def test_every_case_meets_the_bar_through_the_abi_and_the_class(lib, name):
    f = golden(name)
    tt, tv = load_tsi(GOLD)
    ny, nx = f["lat"].shape
    n, npts = len(f["times_ns"]), ny * nx
    st, h, msg = create(lib, f["lat"], f["lon"], tt, tv)
    assert st == 0, msg
    guard, fill = 64, -7777.25
    buf = torch.full((2 * guard + n * npts,), fill, device="cuda")
    dst = buf[guard:guard + n * npts]
    dst.fill_(float("nan"))
    st, msg = compute(lib, h, [int(t) for t in f["times_ns"]], period_ns(name), int(f["n_steps"]), dst, npts)
    assert st == 0, msg
    torch.cuda.synchronize()
    assert (buf[:guard] == fill).all() and (buf[-guard:] == fill).all() and not torch.isnan(dst).any()
    raw = dst.reshape(n, ny, nx).clone()
    check_bar(name, raw.cpu().numpy(), "C ABI")
    assert lib.wx_tisr_destroy(h) == 0

    blk = forcing_of(name)
    assert np.array_equal(blk.latitude.view(np.int32), f["lat"].view(np.int32)) and np.array_equal(blk.longitude.view(np.int32), f["lon"].view(np.int32))
    times = TISR_CASES[name]["times"]
    times = list(times_ns(name)) if isinstance(times, tuple) else times           # strings for the listed times, int ns for the range
    y = blk.compute(times)
    torch.cuda.synchronize()
    assert y.shape == (n, ny, nx) and y.dtype == torch.float32 and y.is_cuda and y.is_contiguous()
    check_bar(name, y.cpu().numpy(), "TISRForcing")
    assert same_bits(y, raw)


@pytest.mark.parametrize("name", ["rect1h", "curv"])
def test_many_times_in_one_call_equal_one_call_per_time(name):
    """3 times (one workgroup row of target times) and 65 (two launch pairs, the second with one time): bit for bit."""
    blk = forcing_of(name)
    ns = [int(t) for t in times_ns(name)]
    together = blk.compute(ns)
    for i, t in enumerate(ns):
        assert same_bits(blk.compute([t])[0], together[i]), (name, i)
    assert same_bits(blk.compute(ns[1:]), together[1:])                            # another grouping of the same times
    torch.cuda.synchronize()


def test_strided_destinations_and_untouched_neighbours():
    name = "rect1h"
    blk = forcing_of(name)
    ns = [int(t) for t in times_ns(name)]
    want = blk.compute(ns)
    H, W = blk.ny, blk.nx
    fill = -7777.25
    frc = torch.full((1, 4, 1, H, W), fill, device="cuda")                          # the slot of a [1, n_dyn, 1, H, W] forcing tensor
    assert blk.compute_into(ns[0], frc, channel=2) is frc
    torch.cuda.synchronize()
    assert same_bits(frc[0, 2, 0], want[0]) and (frc[0, :2] == fill).all() and (frc[0, 3] == fill).all()
    wide = torch.full((3, 5, 1, H, W), fill, device="cuda")                         # three times into channel 4 of a batch of three
    blk.compute_into(ns, wide, channel=4)
    named = torch.full((3, 1, 1, H, W), fill, device="cuda")                        # a [B, 1, 1, H, W] named tensor
    blk.compute_into(ns, named)
    padded = torch.full((3, 2, H, W), fill, device="cuda")[:, :1]                   # [3, 1, H, W] with a plane stride of 2 H W
    blk.compute_into(ns, padded)
    torch.cuda.synchronize()
    assert same_bits(wide[:, 4, 0], want) and (wide[:, :4] == fill).all()
    assert same_bits(named[:, 0, 0], want) and same_bits(padded[:, 0], want) and (padded._base[:, 1] == fill).all()
    from wxengine.engine import WXEngineError
    for bad, kw in ((torch.zeros(3, H, W + 1, device="cuda"), {}), (torch.zeros(2, H, W, device="cuda"), {}),
                    (torch.zeros(3, 2, H, W, device="cuda"), {}), (torch.zeros(3, 2, H, W, device="cuda"), dict(channel=2)),
                    (torch.zeros(3, H, W, device="cuda", dtype=torch.float64), {}), (torch.zeros(3, H, W), {}),
                    (torch.zeros(3, H, 2 * W, device="cuda")[:, :, ::2], {})):
        with pytest.raises(WXEngineError, match="compute_into"):
            blk.compute_into(ns, bad, **kw)


def test_sample_and_forcing_batches():
    blk = forcing_of("rect1h")
    ns = [int(t) for t in times_ns("rect1h")]
    want = blk.compute(ns)
    key = f"{SRC}/dynamic_forcing/2d/tisr"
    s = blk.sample("2021-06-01 06:00")
    assert list(s) == ["input", "metadata"] and s["metadata"] == {"input_datetime": ns[0]} and list(s["input"]) == [SRC]
    assert list(s["input"][SRC]) == [key] and s["input"][SRC][key].shape == (1, 1, 19, 37) and same_bits(s["input"][SRC][key][0, 0], want[0])
    batches = list(blk.forcing_batches(TISR_CASES["rect1h"]["times"]))
    assert len(batches) == 3
    for i, b in enumerate(batches):
        assert list(b) == ["input"] and list(b["input"][SRC]) == [key]
        assert b["input"][SRC][key].shape == (1, 1, 1, 19, 37) and same_bits(b["input"][SRC][key][0, 0, 0], want[i])
    with pytest.raises(ValueError, match=r"1 target time\(s\) have sub-steps outside the TSI data range \[1850\.5000, 2299\.5000\]"):
        blk.compute(["2021-06-01", "1849-12-31 12:00"])


def test_abi_refusals(lib):
    tt, tv = load_tsi(GOLD)
    f = golden("curv")
    lat, lon = f["lat"], f["lon"]
    npts = lat.size
    for kw, why in ((dict(ny=0), "ny and nx must be >= 1 and ny * nx <= 2^31 - 1, got 0 x 3"),
                    (dict(nx=-1), "ny and nx must be >= 1 and ny * nx <= 2^31 - 1, got 5 x -1"),
                    (dict(ny=65536, nx=65536), "ny and nx must be >= 1 and ny * nx <= 2^31 - 1, got 65536 x 65536"),
                    (dict(n_tsi=1), "the TSI table needs at least two entries, got 1"),
                    (dict(n_tsi=0), "the TSI table needs at least two entries, got 0")):
        st, bad, msg = create(lib, lat, lon, tt, tv, **kw)
        assert st == -1 and not bad.value and msg == "wx_tisr_create: " + why, msg
    down = tt.copy()
    down[7] = down[6]
    st, bad, msg = create(lib, lat, lon, down, tv)
    assert st == -1 and msg == "wx_tisr_create: the TSI times must ascend, entry 7 does not"
    nan = tv.copy()
    nan[3] = np.nan
    st, bad, msg = create(lib, lat, lon, tt, nan)
    assert st == -1 and msg == "wx_tisr_create: the TSI table must be finite with |time| <= 1e6 years, entry 3 is not"
    inf = lon.copy()
    inf[1, 2] = np.inf
    st, bad, msg = create(lib, lat, inf, tt, tv)
    assert st == -1 and msg == "wx_tisr_create: latitude and longitude must be finite, point 5 is not"
    for a in ((None, lon, tt, tv), (lat, None, tt, tv), (lat, lon, None, tv), (lat, lon, tt, None)):
        st, bad, msg = create(lib, *a, ny=5, nx=3, n_tsi=450)
        assert st == -1 and msg == "wx_tisr_create: null argument"
    assert lib.wx_tisr_create(5, 3, fptr(lat), fptr(lon), 450, fptr(tt), fptr(tv), 0, None) == -1
    assert lib.wx_last_error() == b"wx_tisr_create: null argument"
    st, bad, msg = create(lib, lat, lon, tt, tv, device=99)
    assert st == -1 and "no such GPU device" in msg

    st, h, msg = create(lib, lat, lon, tt[:171], tv[:171])                          # the table ends at 2020.5
    assert st == 0 and h.value, msg
    fill = -7777.25
    dst = torch.full((2, npts), fill, device="cuda")
    t0, hour = int(np.datetime64("2019-06-01T06:00", "ns").astype(np.int64)), NS_PER_HOUR
    assert compute(lib, None, [t0], hour, 7, dst, npts) == (-1, "wx_tisr_compute: null TISR handle")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    one = (C.c_int64 * 1)(t0)
    assert lib.wx_tisr_compute(h, 1, None, hour, 7, C.c_void_p(dst.data_ptr()), npts, stream) == -1
    assert lib.wx_last_error() == b"wx_tisr_compute: null argument"
    assert lib.wx_tisr_compute(h, 1, one, hour, 7, None, npts, stream) == -1 and lib.wx_last_error() == b"wx_tisr_compute: null argument"
    y1849 = int(np.datetime64("1850-01-01T00:30", "ns").astype(np.int64))          # the window starts in 1849
    y2021 = int(np.datetime64("2021-01-01T00:00", "ns").astype(np.int64))          # the last sub-step is the year 2021
    for args, why in ((([], hour, 7, npts), "n_times must be >= 1, got 0"),
                      (([t0], hour, 0, npts), "n_steps must be 1 .. 2^22 - 1, got 0"),
                      (([t0], hour, -3, npts), "n_steps must be 1 .. 2^22 - 1, got -3"),
                      (([t0], hour, 2 ** 22, npts), "n_steps must be 1 .. 2^22 - 1, got 4194304"),
                      (([t0], 0, 7, npts), "period_ns must be >= 1, got 0"),
                      (([t0], -hour, 7, npts), f"period_ns must be >= 1, got {-hour}"),
                      (([t0], 6, 7, npts), "a period of 6 ns holds no 7 steps of a whole nanosecond"),
                      (([t0, t0], hour, 7, npts - 1), f"plane_stride must be >= ny * nx = {npts}, got {npts - 1}"),
                      (([t0, y1849], hour, 7, npts), "a sub-step of target time 1 lies in the year 1849, outside the TSI table's years 1850 .. 2020"),
                      (([y2021, t0], hour, 7, npts), "a sub-step of target time 0 lies in the year 2021, outside the TSI table's years 1850 .. 2020"),
                      (([-2 ** 63 + 5], hour, 7, npts), "the window of target time 0 leaves the int64 nanosecond range")):
        st, msg = compute(lib, h, args[0], args[1], args[2], dst, args[3])
        assert st == -1 and msg == "wx_tisr_compute: " + why, msg
    torch.cuda.synchronize()
    assert (dst == fill).all()                                                      # a refused call touches nothing
    ok = int(np.datetime64("2020-12-31T23:00", "ns").astype(np.int64))             # the last half year: extrapolated, not refused
    assert compute(lib, h, [ok, int(np.datetime64("1850-01-01T01:00", "ns").astype(np.int64))], hour, 7, dst, npts) == (0, "")
    torch.cuda.synchronize()
    assert torch.isfinite(dst).all() and (dst >= 0).all() and dst.max() > 1.0e6
    assert lib.wx_tisr_destroy(h) == 0 and lib.wx_tisr_destroy(None) == 0


def test_short_forecast_with_the_forcing_from_a_clock():
    """run_forecast on the T0 synthetic model (fp32) with `forcing_batches` from TISRForcing equals, bit for bit, the same run fed the
    planes computed ahead of time; the forcing reaches the model (another clock gives another forecast)."""
    from synth_batches import gen2loop_batches, gen2loop_schema
    from wxengine.config import named_config
    from wxengine.forecast import InverseScale, run_forecast
    from wxengine.model import WXFormerHIP
    from wxengine.synth import synth_state_dict
    from wxengine.tisr import TISRForcing
    cfg = named_config("T0")
    sd = synth_state_dict(cfg)
    ic, _, mean, std = gen2loop_batches(cfg, 3)
    _, out = gen2loop_schema(cfg)
    H, W = cfg.image_height, cfg.image_width
    tt, tv = load_tsi(GOLD)
    blk = TISRForcing(tt, tv, "6h", 90, lat_spec=[90, -90, H], lon_spec=[0, 355, W], source_name="era5")
    clock = ["2021-06-01 06:00", "2021-06-01 12:00", "2021-06-01 18:00"]
    key, sza = "era5/dynamic_forcing/2d/tisr", "era5/dynamic_forcing/2d/sza"
    inner = {("era5/dynamic_forcing/2d/tisr" if k.endswith("/tsi") else k): v.cuda() for k, v in ic["input"]["era5"].items()}
    inner[key] = blk.compute(clock[:1]).reshape(1, 1, 1, H, W)
    ic = {"input": {"era5": inner}}
    mean, std = dict(mean, tisr=np.float32(5.0e6)), dict(std, tisr=np.float32(6.0e6))
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

    def with_sza(batches):           # the other forcing of the T0 schema stays what the initial condition holds
        for b in batches:
            yield {"input": {"era5": dict(b["input"]["era5"], **{sza: inner[sza]})}}

    def run(batches):
        kept = []
        run_forecast(model, ic, with_sza(batches), 3, cmap, mean, std, [InverseScale(mean, std)],
                     lambda yp, step: kept.append({k: v.clone() for k, v in yp["era5"].items()}))
        torch.cuda.synchronize()
        return kept
    live = run(blk.forcing_batches(clock[1:]))
    planes = blk.compute(clock[1:])
    ahead = run([{"input": {"era5": {key: planes[i].reshape(1, 1, 1, H, W)}}} for i in range(2)])
    other = run(blk.forcing_batches(["2021-06-01 00:00", "2021-06-02 00:00"]))
    assert len(live) == len(ahead) == 3
    for step in range(3):
        for k in live[step]:
            assert torch.isfinite(live[step][k]).all() and same_bits(live[step][k], ahead[step][k]), (step, k)
    assert all(same_bits(other[0][k], live[0][k]) for k in live[0])                # step 1 sees the initial condition alone
    assert any(not same_bits(other[2][k], live[2][k]) for k in live[2])
