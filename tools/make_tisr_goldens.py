"""Fixtures of the TISR forcing from the reference's own functions (credit/datasets/gen_2/tisr.py); needs the reference tree.

    python tools/make_tisr_goldens.py

tests/golden/tisr_tsi_cmip6.npz   the CMIP6 TSI table the reference reads (`time`, `tsi` of total_solar_irradiance_CMIP6_49r1.nc;
                                  NetCDF-3, read with scipy), as `_cmip6_tsi_data` returns it through an xarray stand-in
tests/golden/tisr_<case>.npz      per case of tests/tisr_cases.py: the grid as `_get_latlon_grid` builds it (or the curvilinear planes),
                                  the target times, `days32` (`_get_j2000_days` of every sub-step), `ref32` (`_compute_tisr` as it is),
                                  `ref64` (the reference's functions on double tensors from the SAME float32 days and float32 TSI) and
                                  E_ref = max|ref32 - ref64| over the case
The generator refuses a case in which the restatement (tests/tisr_oracle.py) is further from ref64 than ref32 is, or whose float32
days the restatement does not reproduce to the bit."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden")
for p in (HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

TSI_FILE = "total_solar_irradiance_CMIP6_49r1.nc"


def read_tsi_file(path):
    """-> {"time", "tsi"} as native float32 arrays (the file stores big-endian floats)."""
    from scipy.io import netcdf_file
    with netcdf_file(path, "r", mmap=False) as f:
        return {k: f.variables[k].data.astype(np.float32) for k in ("time", "tsi")}


def reference_module(arrays=None):
    """credit.datasets.gen_2.tisr with an `xr` whose open_dataset serves `arrays` (default: the TSI file's own)."""
    import oracle_stub
    oracle_stub.install()
    import credit.datasets.gen_2.tisr as T
    from credit.metadata import get_meta_file_path
    served = arrays if arrays is not None else read_tsi_file(get_meta_file_path(TSI_FILE))

    class _Dataset:
        def __getitem__(self, name):
            return types.SimpleNamespace(values=served[name])

        def close(self):
            pass
    T.xr = types.SimpleNamespace(open_dataset=lambda _path, **_kw: _Dataset())
    return T


def reference_grid(T, name):
    import torch
    from tisr_cases import TISR_CASES, curvilinear_grid
    c = TISR_CASES[name]
    if c.get("curvilinear"):
        lat, lon = curvilinear_grid()
        return torch.from_numpy(lat).unsqueeze(0), torch.from_numpy(lon).unsqueeze(0)
    return T._get_latlon_grid(lat_spec=c["lat_spec"], lon_spec=c["lon_spec"])


def reference_planes(T, t, period, n_steps, lat, lon, tsi_t, tsi_v):
    """-> (ref32, ref64, days32) of one target time."""
    import pandas as pd
    ref32 = T._compute_tisr(t, period, n_steps, lat, lon, tsi_t, tsi_v)
    ts = pd.date_range(end=t, periods=n_steps + 1, freq=period / n_steps)
    tsi = T._get_tsi(ts, tsi_t, tsi_v)
    j32 = T._get_j2000_days(ts)
    orb = T._get_orbital_parameters(j32.double().unsqueeze(-1).unsqueeze(-1))
    cz = T._get_cosine_zenith_angle(orb["cos_declination"], orb["sin_declination"], lat.double(),
                                    T._get_hour_angle(T._get_solar_time(orb["rotational_phase"], orb["eq_of_time_seconds"]), lon.double()))
    inst = T._get_instantaneous_toa_tisr(tsi.double().unsqueeze(-1).unsqueeze(-1), 1.0 / orb["solar_distance_au"] ** 2, cz)
    ref64 = T._get_integrated_toa_tisr(inst, period, n_steps)
    return ref32.numpy(), ref64.numpy(), j32.numpy()


def main():
    import pandas as pd
    import torch
    import tisr_oracle as TO
    from tisr_cases import TISR_CASES, period_ns, times_ns
    T = reference_module()
    tsi_t, tsi_v = T._cmip6_tsi_data()
    assert tsi_t.dtype == torch.float32 and tsi_t.shape == (450,)
    np.savez_compressed(os.path.join(GOLD, "tisr_tsi_cmip6.npz"), time=tsi_t.numpy(), tsi=tsi_v.numpy())
    for name, c in TISR_CASES.items():
        lat, lon = reference_grid(T, name)
        period, n = pd.Timedelta(period_ns(name), unit="ns"), c["n_steps"]
        r32, r64, days = [], [], []
        for t_ns in times_ns(name):
            a, b, j = reference_planes(T, pd.Timestamp(int(t_ns)), period, n, lat, lon, tsi_t, tsi_v)
            r32.append(a), r64.append(b), days.append(j)
        r32, r64, days = np.stack(r32), np.stack(r64), np.stack(days)
        assert r32.dtype == np.float32 and r64.dtype == np.float64 and days.dtype == np.float32
        e_ref = float(np.abs(r32.astype(np.float64) - r64).max())
        mine = [TO.tisr(int(t), period_ns(name), n, lat[0].numpy(), lon[0].numpy(), tsi_t.numpy(), tsi_v.numpy()) for t in times_ns(name)]
        assert np.array_equal(np.stack([m[1] for m in mine]).view(np.int32), days.view(np.int32)), f"{name}: the float32 days differ"
        e_mine = float(np.abs(np.stack([m[0] for m in mine]).astype(np.float64) - r64).max())
        assert e_ref > 0.0 and e_mine <= e_ref, f"{name}: the restatement is {e_mine:.3e} from ref64, the reference {e_ref:.3e}: replace the case"
        path = os.path.join(GOLD, f"tisr_{name}.npz")
        np.savez_compressed(path, lat=lat[0].numpy(), lon=lon[0].numpy(), times_ns=times_ns(name), period_ns=np.int64(period_ns(name)),
                            n_steps=np.int64(n), days32=days, ref32=r32, ref64=r64, E_ref=np.float64(e_ref))
        print(f"[golden] tisr {name}: {len(r32)} planes of {r32.shape[1]} x {r32.shape[2]}, max {r64.max():.4e} J/m2, E_ref {e_ref:.3e} "
              f"({e_ref / r64.max():.2e} of it), restatement / E_ref {e_mine / e_ref:.3f}, distinct days {len(np.unique(days[0]))} of "
              f"{n + 1}, file {os.path.getsize(path) // 1024} KB")


if __name__ == "__main__":
    main()
