"""A numpy restatement of the device algorithm of csrc/wx_tisr.h (not of the reference's tensor program): the coefficient table in
float64 from integer nanoseconds, with the reference's float32 quantisation of the days since J2000 and of the fractional year; the
per-point terms in float32; the sum in float64, rounded to float32 once.  tests/test_tisr_oracle.py holds it to the fixtures of the
reference's own functions (tools/make_tisr_goldens.py) under the bar the device tests use."""
import numpy as np

NS_PER_DAY = 86_400_000_000_000


def substeps_ns(t_end_ns, period_ns, n_steps):
    """pd.date_range(end=t, periods=n_steps + 1, freq=period / n_steps) as int64 ns: the step is the period's ns divided by n_steps and
    truncated, and the instants count back from t."""
    step = int(period_ns) // int(n_steps)
    return int(t_end_ns) - (int(n_steps) - np.arange(int(n_steps) + 1, dtype=np.int64)) * step, step


def j2000_days32(ns):
    """_get_j2000_days: float64 days since J2000.0 rounded to float32."""
    return (ns.astype(np.float64) / 86400e9 + 2440587.5 - 2451545.0).astype(np.float32)


def civil(ns):
    """-> (year, day of year from 1, leap year, ns since midnight) by integer arithmetic (proleptic Gregorian)."""
    ns = np.asarray(ns, dtype=np.int64)
    days = np.floor_divide(ns, NS_PER_DAY)
    z = days + 719468
    era = np.floor_divide(z, 146097)
    doe = z - era * 146097
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy_mar = doe - (365 * yoe + yoe // 4 - yoe // 100)           # day of the year that starts on 1 March
    mp = (5 * doy_mar + 2) // 153
    month = np.where(mp < 10, mp + 3, mp - 9)
    year = yoe + era * 400 + (month <= 2)
    leap = (year % 4 == 0) & ((year % 100 != 0) | (year % 400 == 0))
    doy = np.where(month <= 2, doy_mar - 306, doy_mar + 59 + leap) + 1
    return year, doy, leap, ns - days * NS_PER_DAY


def frac_year32(ns):
    """_get_tsi's fractional year: float64, then float32."""
    year, doy, leap, ns_of_day = civil(ns)
    day_frac = ns_of_day.astype(np.float64) / np.float64(NS_PER_DAY)
    year_frac = (doy - 1 + day_frac) / (365 + leap)
    return (year + year_frac).astype(np.float32)


def tsi32(fy32, tsi_times, tsi_values):
    """_get_tsi's searchsorted / clamp(1, n - 1) / linear interpolation, every operation in float32."""
    tt, tv = np.asarray(tsi_times, np.float32), np.asarray(tsi_values, np.float32)
    idx = np.clip(np.searchsorted(tt, fy32, side="left"), 1, len(tt) - 1)
    lo, hi = idx - 1, idx
    t = (fy32 - tt[lo]) / (tt[hi] - tt[lo])
    return tv[lo] + t * (tv[hi] - tv[lo])


def table(t_end_ns, period_ns, n_steps, tsi_times, tsi_values):
    """-> (C, P, Q, S) float32 [n_steps + 1] and the float32 days."""
    ns, step = substeps_ns(t_end_ns, period_ns, n_steps)
    j32 = j2000_days32(ns)
    tsi = tsi32(frac_year32(ns), tsi_times, tsi_values).astype(np.float64)
    j = j32.astype(np.float64)
    theta = j / 365.25
    phase = j - np.floor(j)                                        # torch's floored j % 1.0
    rel = 1.7535 + 6.283076 * theta
    rem = 6.240041 + 6.283020 * theta
    rlls = 4.8951 + 6.283076 * theta
    rllls = (4.8952 + 6.283320 * theta - 0.0075 * np.sin(rel) - 0.0326 * np.cos(rel) - 0.0003 * np.sin(2.0 * rel)
             + 0.0002 * np.cos(2.0 * rel))
    sin_dec = np.sin(np.float64(0.409093)) * np.sin(rllls)
    cos_dec = np.sqrt(1.0 - sin_dec ** 2)
    sin_rem = np.sin(rem)
    eot = (591.8 * np.sin(2.0 * rlls) - 459.4 * sin_rem + 39.5 * sin_rem * np.cos(2.0 * rlls) - 12.7 * np.sin(4.0 * rlls)
           - 4.8 * np.sin(2.0 * rem))
    dist = 1.0001 - 0.0163 * np.sin(rel) + 0.0037 * np.cos(rel)
    solar_time = phase + eot / 86400.0
    A = np.deg2rad(360.0 * solar_time)
    w = np.ones(n_steps + 1)
    w[0] = w[-1] = 0.5
    C = w * (step / 1e9) * tsi / dist ** 2
    f32 = lambda v: v.astype(np.float32)   # noqa: E731
    return (f32(C), f32(cos_dec * np.cos(A)), f32(cos_dec * np.sin(A)), f32(sin_dec)), j32


def point_terms(lat, lon):
    """-> (a, b, c) float32 planes, computed in float64 from the float32 degrees."""
    phi, lam = np.deg2rad(np.asarray(lat, np.float32).astype(np.float64)), np.deg2rad(np.asarray(lon, np.float32).astype(np.float64))
    return ((np.cos(phi) * np.cos(lam)).astype(np.float32), (np.cos(phi) * np.sin(lam)).astype(np.float32),
            np.sin(phi).astype(np.float32))


def tisr(t_end_ns, period_ns, n_steps, lat, lon, tsi_times, tsi_values):
    """-> (plane float32 [ny, nx], float32 days [n_steps + 1])."""
    (C, P, Q, S), j32 = table(t_end_ns, period_ns, n_steps, tsi_times, tsi_values)
    a, b, c = point_terms(lat, lon)
    k = (slice(None),) + (None,) * a.ndim
    cz = P[k] * a - Q[k] * b + S[k] * c                            # float32
    term = C[k] * np.maximum(cz, np.float32(0.0))                  # float32
    return term.astype(np.float64).sum(axis=0).astype(np.float32), j32
