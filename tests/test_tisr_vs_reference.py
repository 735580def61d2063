"""The TISR fixtures against the LIVE reference (credit/datasets/gen_2/tisr.py), to the bit; skipped where the reference tree is absent.
The module reads its TSI table through xarray: a stand-in serves the arrays that scipy reads from the reference's NetCDF-3 file."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from tisr_cases import TISR_CASES, load_golden, load_tsi, period_ns, times_ns  # noqa: E402

pytestmark = pytest.mark.reference
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def reference():
    import make_tisr_goldens as MG
    before = sys.modules.get("xarray")
    T = MG.reference_module()
    yield T, MG
    if before is None:
        sys.modules.pop("xarray", None)
    else:
        sys.modules["xarray"] = before


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int64 if a.dtype == np.float64 else np.int32),
                                                                        b.view(np.int64 if b.dtype == np.float64 else np.int32))


def test_the_tsi_table_is_the_one_the_reference_reads(reference):
    T, _ = reference
    tt, tv = T._cmip6_tsi_data()
    gt, gv = load_tsi(GOLD)
    assert same_bits(tt.numpy(), gt) and same_bits(tv.numpy(), gv)


@pytest.mark.parametrize("name", list(TISR_CASES))
def test_reference_reproduces_the_goldens_bit_for_bit(reference, name):
    import pandas as pd
    T, MG = reference
    f = load_golden(name, GOLD)
    tt, tv = (torch.from_numpy(a) for a in load_tsi(GOLD))
    lat, lon = MG.reference_grid(T, name)
    assert same_bits(lat[0].numpy(), f["lat"]) and same_bits(lon[0].numpy(), f["lon"])
    period = pd.Timedelta(period_ns(name), unit="ns")
    for i, t in enumerate(times_ns(name)[:8]):                     # `curv`: eight of the 65 planes
        r32, r64, days = MG.reference_planes(T, pd.Timestamp(int(t)), period, TISR_CASES[name]["n_steps"], lat, lon, tt, tv)
        assert same_bits(days, f["days32"][i]) and same_bits(r32, f["ref32"][i]) and same_bits(r64, f["ref64"][i]), (name, i)


def test_grid_spec_errors_are_the_references(reference):
    """wxengine.tisr.latlon_grid raises the reference's ValueErrors with its words (the path becomes the lat / lon arrays)."""
    from wxengine.tisr import latlon_grid
    T, _ = reference
    for lat_spec, lon_spec in (([90, -90], [0, 359, 4]), ([90, -90, 3], [0, 359, 4, 1]), ([90, -90, 2.5], [0, 359, 4]),
                               ([90, -90, True], [0, 359, 4]), ([90, -90, 3], [0, 359, 0]), ([90, -90, 3], [0, 359, -2])):
        with pytest.raises(ValueError) as theirs:
            T._get_latlon_grid(lat_spec=lat_spec, lon_spec=lon_spec)
        with pytest.raises(ValueError) as ours:
            latlon_grid(lat_spec=lat_spec, lon_spec=lon_spec)
        assert str(ours.value) == str(theirs.value)
    lat, lon = latlon_grid(lat_spec=[90, -90, 19], lon_spec=[0, 360, 37])
    rl, ro = T._get_latlon_grid(lat_spec=[90, -90, 19], lon_spec=[0, 360, 37])
    assert same_bits(lat, rl[0].numpy()) and same_bits(lon, ro[0].numpy())
    with pytest.raises(ValueError, match="Provide exactly one grid source"):
        T._get_latlon_grid()
    with pytest.raises(ValueError, match="Provide exactly one grid source"):
        latlon_grid()


def test_years_outside_the_table_raise(reference):
    import pandas as pd
    T, _ = reference
    tt, tv = (torch.from_numpy(a[:171]) for a in load_tsi(GOLD))                # 1850.5 .. 2020.5: int64 ns end in 2262, before the table
    assert tt[-1] == 2020.5
    for t in ("1849-12-31 23:00", "2021-01-01 00:30", "1850-01-01 00:30", "2021-01-01 00:00"):
        # the third: the window starts in 1849; the fourth: the last sub-step IS the year 2021
        ts = pd.date_range(end=pd.Timestamp(t), periods=4, freq=pd.Timedelta(hours=1) / 3)
        with pytest.raises(ValueError, match=r"timestamp\(s\) fall outside the TSI data range \[1850\.5000, 2020\.5000\]"):
            T._get_tsi(ts, tt, tv)
    for t in ("1850-01-01 01:00", "2020-12-31 23:00"):                          # the first and the last half year: extrapolated
        ts = pd.date_range(end=pd.Timestamp(t), periods=4, freq=pd.Timedelta(hours=1) / 3)
        assert torch.isfinite(T._get_tsi(ts, tt, tv)).all()
