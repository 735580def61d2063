"""Host side of the TISR forcing (wxengine/tisr.py) without a GPU: the argument checks with the reference's messages, the grid sources, the
time conversions, the dict shapes and keys of `sample` and `forcing_batches` -- with the device call replaced by a stand-in that fills
the planes on the CPU -- and that the batches route through `RolloutRouter` as a dynamic forcing."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from tisr_cases import TISR_CASES, curvilinear_grid, load_tsi, times_ns  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
KW = dict(integration_period="1h", lat_spec=[90, -90, 5], lon_spec=[0, 270, 4], source_name="ERA5")


@pytest.fixture
def host_only(monkeypatch):
    """TISRForcing whose handle is not created and whose launch writes i + 1 into plane i, on the CPU."""
    import wxengine.tisr as WT
    launched = []

    def launch(self, ns, base_ptr, plane_stride):
        launched.append((list(ns), plane_stride))
        for i in range(len(ns)):
            self._dst_planes[i].fill_(float(i + 1))
    real_into = WT.TISRForcing.compute_into

    def compute_into(self, times, dst, channel=None):
        self._dst_planes = [dst[i] if channel is None else dst[i, channel] for i in range(dst.shape[0])]
        return real_into(self, times, dst, channel)
    monkeypatch.setattr(WT.TISRForcing, "_create_handle", lambda self: None)
    monkeypatch.setattr(WT.TISRForcing, "_launch", launch)
    monkeypatch.setattr(WT.TISRForcing, "compute_into", compute_into)
    tt, tv = load_tsi(GOLD)
    return (lambda **kw: WT.TISRForcing(tt, tv, **dict(dict(KW, device="cpu"), **kw))), launched


def test_exported_lazily_and_raises_without_a_gpu():
    import wxengine
    from wxengine.engine import WXEngineError
    from wxengine.tisr import TISRForcing
    assert wxengine.TISRForcing is TISRForcing
    if not torch.cuda.is_available():
        tt, tv = load_tsi(GOLD)
        with pytest.raises(WXEngineError, match="no GPU visible: the TISR forcing has no CPU fallback"):
            TISRForcing(tt, tv, **KW)


def test_argument_checks_come_first_with_the_references_words():
    from wxengine.tisr import TISRForcing
    tt, tv = load_tsi(GOLD)
    lat1, lon1 = np.linspace(90, -90, 5), np.linspace(0, 270, 4)
    for kw, why in (
            (dict(lon_spec=None), r"TISR config: 'lat_spec' and 'lon_spec' must be supplied together\. Got lat_spec=\[90, -90, 5\], lon_spec=None\."),
            (dict(lat_spec=None, lon_spec=None), "Provide exactly one grid source: .* not both or neither"),
            (dict(lat=lat1, lon=lon1), "Provide exactly one grid source: .* not both or neither"),
            (dict(lat_spec=None, lon_spec=None, lat=lat1), "'lat' and 'lon' must be supplied together"),
            (dict(lat_spec=[90, -90]), r"lat spec must be \[start, end, num_points\], got \[90, -90\] \(2 element\(s\) instead of 3\)"),
            (dict(lon_spec=[0, 270, 4.0]), r"lon spec \[0, 270, 4\.0\]: num_points must be an int, got float"),
            (dict(lon_spec=[0, 270, True]), r"lon spec \[0, 270, True\]: num_points must be an int, got bool"),
            (dict(lat_spec=[90, -90, 0]), r"lat spec \[90, -90, 0\]: num_points must be >= 1, got 0"),
            (dict(lat_spec=None, lon_spec=None, lat=np.zeros((2, 3)), lon=np.zeros(3)), r"Expected lat/lon to be 1-D or 2-D after squeezing, got lat\.ndim=2, lon\.ndim=1"),
            (dict(lat_spec=None, lon_spec=None, lat=np.zeros((2, 3)), lon=np.zeros((3, 2))), r"2-D lat and lon must have one shape"),
            (dict(num_integration_steps=0), "num_integration_steps must be a positive integer, but got 0"),
            (dict(num_integration_steps=2.0), r"num_integration_steps must be a positive integer, but got 2\.0"),
            (dict(num_integration_steps=2 ** 22), r"num_integration_steps must be at most 2\^22 - 1"),
            (dict(integration_period=5, num_integration_steps=6), "integration_period must hold num_integration_steps = 6 steps"),
            (dict(integration_period="-1h"), "integration_period must hold"),
            (dict(source_name=""), "source_name is required")):
        with pytest.raises(ValueError, match=why):
            TISRForcing(tt, tv, **dict(KW, **kw))
    with pytest.raises(TypeError):
        TISRForcing(tt, tv, "1h", 360, lat_spec=[90, -90, 5], lon_spec=[0, 270, 4])            # source_name is required
    for a, b, why in ((tt[:1], tv[:1], "at least two entries"), (tt[::-1], tv, "ascending times"), (tt, tv[:-1], "one length")):
        with pytest.raises(ValueError, match=why):
            TISRForcing(a, b, **KW)


def test_grid_sources():
    from wxengine.tisr import latlon_grid
    lat, lon = latlon_grid(lat_spec=[90, -90, 5], lon_spec=[0, 270, 4])
    assert lat.shape == lon.shape == (5, 4) and lat.dtype == lon.dtype == np.float32
    assert lat[:, 0].tolist() == [90.0, 45.0, 0.0, -45.0, -90.0] and lon[0].tolist() == [0.0, 90.0, 180.0, 270.0]
    one = latlon_grid(lat_spec=[-33.25, 0, 1], lon_spec=[151.0, 0, 1])
    assert one[0].tolist() == [[-33.25]] and one[1].tolist() == [[151.0]]              # num_points = 1: the start
    l2, o2 = latlon_grid(lat=lat[:, 0].astype(np.float64), lon=lon[0])                  # 1-D arrays: the meshgrid, cast to float32
    assert np.array_equal(l2, lat) and np.array_equal(o2, lon) and l2.dtype == np.float32 and l2.flags.c_contiguous
    cl, co = curvilinear_grid()
    l3, o3 = latlon_grid(lat=cl[None], lon=co[None])                                    # [1, ny, nx] as a file stores it
    assert np.array_equal(l3, cl) and np.array_equal(o3, co)


def test_times_are_unix_nanoseconds():
    import pandas as pd
    from wxengine.tisr import times_ns as to_ns
    want = int(times_ns("rect1h")[0])
    for t in ("2021-06-01 06:00", pd.Timestamp("2021-06-01 06:00"), np.datetime64("2021-06-01T06:00"), want, np.int64(want),
              pd.Timestamp("2021-06-01 08:00", tz="Europe/Berlin")):
        assert to_ns(t) == [want] and to_ns([t, t]) == [want, want]
    assert to_ns(pd.date_range("2021-06-01 06:00", periods=3, freq="6h")) == [want + i * 6 * 3600 * 10 ** 9 for i in range(3)]
    assert to_ns(TISR_CASES["rect1h"]["times"]) == [int(t) for t in times_ns("rect1h")]


def test_dict_shapes_keys_and_calls(host_only):
    make, launched = host_only
    blk = make()
    assert (blk.ny, blk.nx, blk.period_ns, blk.num_integration_steps, blk.key) == (5, 4, 3600 * 10 ** 9, 360, "ERA5/dynamic_forcing/2d/tisr")
    y = blk.compute(["2021-06-01 06:00", "2021-06-01 12:00", "2021-06-01 18:00"])
    assert y.shape == (3, 5, 4) and y[:, 0, 0].tolist() == [1.0, 2.0, 3.0] and launched[-1][1] == 20 and len(launched[-1][0]) == 3
    s = blk.sample("2021-06-01 06:00")
    ns = int(times_ns("rect1h")[0])
    assert list(s) == ["input", "metadata"] and s["metadata"] == {"input_datetime": ns} and launched[-1] == ([ns], 20)
    assert list(s["input"]) == ["ERA5"] and list(s["input"]["ERA5"]) == [blk.key] and s["input"]["ERA5"][blk.key].shape == (1, 1, 5, 4)
    gen = blk.forcing_batches(["2021-06-01 06:00", "2021-06-01 12:00"])
    before = len(launched)
    first = next(gen)
    assert len(launched) == before + 1                                                  # computed when asked for, one time per batch
    assert list(first) == ["input"] and first["input"]["ERA5"][blk.key].shape == (1, 1, 1, 5, 4) and len(list(gen)) == 1
    frc = torch.full((1, 3, 1, 5, 4), -1.0)
    blk.compute_into(ns, frc, channel=1)
    assert (frc[0, 1] == 1.0).all() and (frc[0, 0] == -1.0).all() and (frc[0, 2] == -1.0).all()
    with pytest.raises(ValueError, match=r"2 target time\(s\) have sub-steps outside the TSI data range \[1850\.5000, 2299\.5000\]: \['1849"):
        blk.compute(["1849-06-01", "2021-06-01", "1850-01-01 00:30"])
    assert make(num_integration_steps=7, integration_period=pd_hours(3)).period_ns == 3 * 3600 * 10 ** 9


def pd_hours(h):
    import pandas as pd
    return pd.Timedelta(hours=h)


def test_forcing_batches_feed_the_rollout_router(host_only):
    from wxengine.forecast import FROM_FORCING, RolloutRouter
    make, _ = host_only
    blk = make(source_name="era5")
    ic = {"era5": {"era5/prognostic/3d/T": torch.zeros(1, 2, 1, 5, 4), "era5/static/2d/LSM": torch.zeros(1, 1, 1, 5, 4),
                   blk.key: torch.zeros(1, 1, 1, 5, 4)}}
    router = RolloutRouter(ic)
    assert ("era5", blk.key, FROM_FORCING) in router.rows
    pred = {"era5": {"era5/prognostic/3d/T": torch.ones(1, 2, 1, 5, 4)}}
    for b in blk.forcing_batches(["2021-06-01 06:00", "2021-06-01 12:00"]):
        nxt = router(pred, b["input"], ic)
        assert list(nxt["era5"]) == list(ic["era5"]) and nxt["era5"][blk.key] is b["input"]["era5"][blk.key]
        assert nxt["era5"][blk.key].shape == ic["era5"][blk.key].shape and (nxt["era5"][blk.key] == 1.0).all()
    assert not router._warned
