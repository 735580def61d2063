"""The cases of the TISR forcing (csrc/wx_tisr.h, wxengine/tisr.py), shared by tools/make_tisr_goldens.py and the tests.  Every grid is
tiny; a case is there for a place where the kernels can go wrong:
  rect1h    19 x 37 with both poles, 703 points (no multiple of 64, more than one workgroup), the default 1 h / 360 steps, three
            target times in one call: boreal summer, the December solstice (polar night and day), 1995 (negative days since J2000)
  rect6h    6 h / 2160 steps, the reference's own suggestion: nine table chunks, the longest sum
  rect3h    3 h / 90 steps: a window that ends before 2000 begins while the days cross -1 .. 0, the leap day of 2024 (the coarser
            ulp of the float32 days) and a window that crosses the turn of the year 2031
  chunk     n_steps = the table chunk size, so the last chunk holds one entry
  ends      n_steps = 1: both trapezoid ends and nothing between them
  one       a 1 x 1 grid: one thread of one workgroup has work
  curv      a 5 x 3 curvilinear grid (2-D latitude and longitude), n_steps = 7 -- 3 h is no multiple of 7 ns, the step is truncated as
            pandas truncates it --, 65 hourly target times across the turn of the year 2000: more than one launch pair per call"""
import os

import numpy as np

SRC = "ERA5"
CHUNK = 256          # kTisrChunk of csrc/wx_tisr.h
MAX_TIMES = 64       # kTisrMaxTimes
NS_PER_HOUR = 3_600_000_000_000

RECT = dict(lat_spec=[90, -90, 19], lon_spec=[0, 360, 37])
TISR_CASES = {
    "rect1h": dict(RECT, period_h=1, n_steps=360, times=["2021-06-01 06:00", "2021-12-21 12:00", "1995-03-01 00:00"]),
    "rect6h": dict(RECT, period_h=6, n_steps=2160, times=["2021-12-21 12:00"]),
    "rect3h": dict(RECT, period_h=3, n_steps=90, times=["1999-12-31 21:00", "2024-02-29 18:00", "2031-01-01 00:00"]),
    "chunk": dict(RECT, period_h=6, n_steps=CHUNK, times=["2024-02-29 18:00", "2021-06-01 06:00"]),
    "ends": dict(RECT, period_h=1, n_steps=1, times=["2021-06-01 06:00"]),
    "one": dict(lat_spec=[-33.25, 0, 1], lon_spec=[151.0, 0, 1], period_h=6, n_steps=360,
                times=["2021-06-01 06:00", "2021-12-21 12:00", "2024-02-29 18:00", "2031-01-01 00:00"]),
    "curv": dict(curvilinear=True, period_h=3, n_steps=7, times=("1999-12-30 18:00", 65)),
}


def times_ns(name):
    """The target times of a case as int64 Unix nanoseconds (numpy's datetime64 arithmetic: no pandas needed)."""
    t = TISR_CASES[name]["times"]
    if isinstance(t, tuple):
        t0 = np.datetime64(t[0].replace(" ", "T"), "ns").astype(np.int64)
        return t0 + np.arange(t[1], dtype=np.int64) * NS_PER_HOUR
    return np.array([np.datetime64(s.replace(" ", "T"), "ns").astype(np.int64) for s in t], dtype=np.int64)


def period_ns(name):
    return TISR_CASES[name]["period_h"] * NS_PER_HOUR


def curvilinear_grid():
    """5 x 3, rotated against the parallels, across the date line and up to 88.5 degrees north."""
    i, j = np.meshgrid(np.arange(5.0), np.arange(3.0), indexing="ij")
    return (28.5 + 15.0 * i - 2.25 * j).astype(np.float32), (171.0 + 1.5 * i + 6.5 * j).astype(np.float32)


def load_tsi(gold):
    """The CMIP6 annual-mean TSI table of IFS cycle 49r1, 1850.5 .. 2299.5: (times, values), float32 [450]."""
    z = np.load(os.path.join(gold, "tisr_tsi_cmip6.npz"))
    return z["time"], z["tsi"]


def load_golden(name, gold):
    """-> dict: lat, lon [ny, nx] float32; times_ns [n]; period_ns, n_steps; days32 [n, n_steps + 1]; ref32 [n, ny, nx] float32;
    ref64 [n, ny, nx] float64; E_ref."""
    z = np.load(os.path.join(gold, f"tisr_{name}.npz"))
    g = {k: z[k] for k in z.files}
    assert np.array_equal(g["times_ns"], times_ns(name)) and int(g["period_ns"]) == period_ns(name), name
    assert int(g["n_steps"]) == TISR_CASES[name]["n_steps"], name
    return g
