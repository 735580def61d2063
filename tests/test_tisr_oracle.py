"""The numpy restatement of the device algorithm (tests/tisr_oracle.py) against the fixtures of the reference's own functions
(tools/make_tisr_goldens.py), on the CPU, under the bar of the device tests:
    max|x - ref64| <= E_ref = max|ref32 - ref64|  per case, absolute, over every plane of the case
(no further from the reference's fp64 evaluation than the reference's own float32 result is), hence max|x - ref32| <= 2 E_ref.  The
float32 days since J2000 of every sub-step equal the reference's to the bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import tisr_oracle as TO  # noqa: E402
from tisr_cases import CHUNK, MAX_TIMES, TISR_CASES, load_golden, load_tsi, period_ns, times_ns  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_the_fixtures_hold_what_the_cases_are_there_for():
    tt, tv = load_tsi(GOLD)
    assert tt.dtype == tv.dtype == np.float32 and tt.shape == tv.shape == (450,) and tt[0] == 1850.5 and tt[-1] == 2299.5
    assert (np.diff(tt) > 0).all() and 1350.0 < tv.min() and tv.max() < 1370.0
    g = {name: load_golden(name, GOLD) for name in TISR_CASES}
    for name, f in g.items():
        n, T = len(f["times_ns"]), int(f["n_steps"]) + 1
        assert f["lat"].dtype == f["lon"].dtype == f["ref32"].dtype == f["days32"].dtype == np.float32 and f["ref64"].dtype == np.float64
        assert f["days32"].shape == (n, T) and f["ref32"].shape == f["ref64"].shape == (n,) + f["lat"].shape == (n,) + f["lon"].shape
        assert float(f["E_ref"]) == np.abs(f["ref32"].astype(np.float64) - f["ref64"]).max() > 0.0
        assert (f["ref64"] >= 0.0).all() and f["ref64"].max() > 1.0e6
    rect = g["rect1h"]
    assert rect["lat"].shape == (19, 37) and rect["lat"].size % 64 != 0 and rect["lat"].size > 512 and abs(rect["lat"][0, 0]) == 90.0
    assert len(np.unique(rect["days32"][0])) < 100                        # 361 sub-steps of an hour collapse onto 86 instants
    dec = rect["ref64"][1]
    assert (dec[0] == 0.0).all() and (dec[-1] > 0.0).all()                # 21 December: polar night in the north, polar day in the south
    assert (rect["days32"][2] < 0).all()                                  # 1995
    d99 = g["rect3h"]["days32"][0]
    assert d99.min() < -0.7 and d99.max() < -0.6 and (g["curv"]["days32"] < 0).any() and (g["curv"]["days32"] > 0).any()
    assert np.diff(g["rect3h"]["days32"][1]).min() >= 0 and g["rect3h"]["days32"][1, 0] > 8766.0      # 2024: an ulp of 2^-10 days
    assert int(g["chunk"]["n_steps"]) + 1 == CHUNK + 1 and int(g["rect6h"]["n_steps"]) == 2160 and int(g["ends"]["n_steps"]) == 1
    assert g["one"]["lat"].shape == (1, 1) and g["curv"]["lat"].shape == (5, 3) and len(g["curv"]["times_ns"]) == MAX_TIMES + 1
    assert period_ns("curv") % 7 != 0 and not np.allclose(g["curv"]["lat"], g["curv"]["lat"][:, :1])


def test_the_integer_calendar_is_numpys():
    g = np.random.Generator(np.random.Philox(key=[5, 5]))
    ns = np.concatenate([g.integers(-3_000_000_000 * 10 ** 9, 9_000_000_000 * 10 ** 9, 4000),
                         (np.array(["1999-12-31T23:59:59.999999999", "2000-01-01", "2000-02-29", "2000-12-31", "1900-03-01", "2100-02-28T12",
                                    "2024-02-29T18", "2024-12-31T23", "1969-12-31T23:59:59", "1970-01-01"], dtype="datetime64[ns]")).astype(np.int64)])
    year, doy, leap, ns_of_day = TO.civil(ns)
    d = ns.astype("datetime64[ns]")
    y = d.astype("datetime64[Y]")
    assert np.array_equal(year, y.astype(np.int64) + 1970)
    assert np.array_equal(doy, (d.astype("datetime64[D]") - y.astype("datetime64[D]")).astype(np.int64) + 1)
    assert np.array_equal(leap, ((y + 1).astype("datetime64[D]") - y.astype("datetime64[D]")).astype(np.int64) == 366)
    assert np.array_equal(ns_of_day, (d - d.astype("datetime64[D]")).astype(np.int64)) and ns_of_day.min() >= 0


@pytest.mark.parametrize("name", list(TISR_CASES))
def test_restatement_meets_the_bar(name):
    f = load_golden(name, GOLD)
    tt, tv = load_tsi(GOLD)
    got = [TO.tisr(int(t), period_ns(name), TISR_CASES[name]["n_steps"], f["lat"], f["lon"], tt, tv) for t in times_ns(name)]
    planes, days = np.stack([p for p, _ in got]), np.stack([j for _, j in got])
    assert planes.dtype == np.float32 and days.dtype == np.float32
    assert np.array_equal(days.view(np.int32), f["days32"].view(np.int32)), "the float32 days differ from the reference's"
    e_ref = float(f["E_ref"])
    d64 = float(np.abs(planes.astype(np.float64) - f["ref64"]).max())
    d32 = float(np.abs(planes.astype(np.float64) - f["ref32"].astype(np.float64)).max())
    print(f"[tisr oracle] {name}: E_ref {e_ref:.3e} ({e_ref / f['ref64'].max():.2e} of the maximum), restatement to ref64 {d64 / e_ref:.3f} E_ref, "
          f"to ref32 {d32 / e_ref:.3f} E_ref")
    assert d64 <= e_ref and d32 <= 2.0 * e_ref
