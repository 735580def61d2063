"""The spherical harmonic transforms on the device (csrc/wx_sht.h through the raw C ABI of include/wxengine_sht.h and through
wxengine/sht.py) against the fp64 oracle (tests/sht_oracle.py, given the device's own nodes) and a scipy-built wind fixture.

The bars are derived, not tuned (tests/sht_cases.py).  The device and the oracle both sum in fp64, in different orders, over the same
tables up to E_tab (the tables' distance from the np.longdouble recurrence, measured in tests/test_sht_host.py), so with u = 2^-53:
  coefficient    |dev - oracle| <= ((nlon + nlat + 16) u 2 + 2 E_tab) sum_k |w_k Pbar_lm(theta_k)| (2 pi / nlon) sum_j |x_kj|
                 the forward error of an fp64 sum of nlon + nlat products in any order, for both sides, plus the table term
                 (a table row that is rounding noise throughout -- l = nlat, m = 0 on a Gauss grid -- takes the table term as the
                 absolute error E_tab is: sht_cases.analysis_bound says why and how such a row is told)
  vector         the same with |dPt| on one component's row masses and |Qt| on the other's, 2 (nlon + nlat) terms
  synthesis      |dev - oracle| <= ((lmax + 2 mmax + 16) u 2 + 2 E_tab) sum_m mult_m sum_l |Pbar_lm(theta_k)| (|re c_lm| + |im c_lm|)
  spectra        the coefficient bound dc propagated, sum mult (2 |c| dc + dc^2), plus (terms + 4) 2 u of the value for the sum itself
  round trip     on a Gauss grid, of a field band-limited to l < lmax: the analysis bound carried through the synthesis
                 (sum_m mult_m sum_l |Pbar| dc) plus the synthesis bound
Everything else is bit for bit: independence of the plane count, the position and the split of a call, strided views, float32 input
against the same values in float64, csphase, the module's zonal_spectrum against spectra(analysis(x)), and synthesis to float32 against
the float64 result rounded once.  Every output lies between guard bands and no input is modified."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import sht_cases as SC  # noqa: E402
import sht_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, FILL = 96, -7777.25
P_ACC = 3


@pytest.fixture(scope="module")
def lib():
    from wxengine.native import load_library
    return load_library()


def nodes(name):
    from wxengine.sht import grid_nodes
    nlat, _, grid = SC.ALL_CASES[name][:3]
    return grid_nodes(nlat, grid)


def guarded(shape, dtype=torch.float64):
    """-> (buffer, view of `shape` between two guard bands of FILL)."""
    n = int(np.prod(shape))
    buf = torch.full((2 * GUARD + n,), FILL, device="cuda", dtype=dtype)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_ok(buf):
    return bool((buf[:GUARD] == FILL).all() and (buf[-GUARD:] == FILL).all())


def vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def as_complex(t):
    return t.cpu().numpy().view(np.complex128)[..., 0]


class Raw:
    """One handle of the raw C ABI."""

    def __init__(self, lib, name, theta=None, w=None, csphase=1):
        self.lib = lib
        self.nlat, self.nlon, _, self.lmax, self.mmax = SC.geometry(name)
        t0, w0 = nodes(name)
        self.theta, self.w = (t0 if theta is None else theta), (w0 if w is None else w)
        self.h = C.c_void_p()
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
        st = lib.wx_sht_create(self.nlat, self.nlon, self.lmax, self.mmax, f64(self.theta), f64(self.w), csphase, b"ortho", 0, C.byref(self.h))
        assert st == 0, lib.wx_last_error()

    def close(self):
        assert self.lib.wx_sht_destroy(self.h) == 0

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def analysis(self, x, stride=None, P=None):
        """x: device [P, nlat, nlon] float32 / float64 -> complex128 [P, lmax, mmax] on the host; guards and input checked."""
        P = x.shape[0] if P is None else P
        buf, c = guarded((P, self.lmax, self.mmax, 2))
        keep = x.clone()
        st = self.lib.wx_sht_analysis(self.h, P, vp(x), self.nlat * self.nlon if stride is None else stride, 1 if x.dtype == torch.float64 else 0,
                                      vp(c), self.stream())
        assert st == 0, self.lib.wx_last_error()
        torch.cuda.synchronize()
        assert guards_ok(buf) and torch.equal(x, keep)
        return as_complex(c)

    def synthesis(self, c, dtype=torch.float64):
        P = c.shape[0]
        cd = torch.from_numpy(np.ascontiguousarray(c).view(np.float64).reshape(P, self.lmax, self.mmax, 2)).cuda()
        keep = cd.clone()
        buf, x = guarded((P, self.nlat, self.nlon), dtype)
        assert self.lib.wx_sht_synthesis(self.h, P, vp(cd), vp(x), 1 if dtype == torch.float64 else 0, self.stream()) == 0, self.lib.wx_last_error()
        torch.cuda.synchronize()
        assert guards_ok(buf) and torch.equal(cd, keep)
        return x.cpu().numpy()

    def vector(self, u, v):
        P, hw = u.shape[0], self.nlat * self.nlon
        bs, s = guarded((P, self.lmax, self.mmax, 2))
        bt, t = guarded((P, self.lmax, self.mmax, 2))
        ku, kv = u.clone(), v.clone()
        st = self.lib.wx_sht_vector_analysis(self.h, P, vp(u), hw, vp(v), hw, 1 if u.dtype == torch.float64 else 0, vp(s), vp(t), self.stream())
        assert st == 0, self.lib.wx_last_error()
        torch.cuda.synchronize()
        assert guards_ok(bs) and guards_ok(bt) and torch.equal(u, ku) and torch.equal(v, kv)
        return as_complex(s), as_complex(t)

    def spectra(self, c):
        P = c.shape[0]
        cd = torch.from_numpy(np.ascontiguousarray(c).view(np.float64).reshape(P, self.lmax, self.mmax, 2)).cuda()
        bz, z = guarded((P, self.mmax))
        bt, t = guarded((P, self.lmax))
        assert self.lib.wx_sht_spectra(self.h, P, vp(cd), vp(z), vp(t), self.stream()) == 0, self.lib.wx_last_error()
        torch.cuda.synchronize()
        assert guards_ok(bz) and guards_ok(bt)
        return z.cpu().numpy(), t.cpu().numpy()


_case_cache = {}


def case(lib, name):
    """Per grid case the inputs, the device results of one call each and the oracle's, computed once and never changed."""
    if name in _case_cache:
        return _case_cache[name]
    nlat, nlon, grid, lmax, mmax = SC.geometry(name)
    theta, w = nodes(name)
    x, u, v = SC.field(name, P_ACC, 0), SC.field(name, P_ACC, 1, 30.0), SC.field(name, P_ACC, 2, 20.0)
    coef = SC.coefficients(lmax, mmax, P_ACC, 3)
    r = Raw(lib, name)
    d = dict(theta=theta, w=w, x=x, u=u, v=v, coef=coef)
    d["c_dev"] = r.analysis(torch.from_numpy(x).cuda())
    d["x_dev"] = r.synthesis(coef)
    d["s_dev"], d["t_dev"] = r.vector(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda())
    d["c"] = O.analysis(x, theta, w, lmax, mmax)
    d["zt_dev"] = r.spectra(d["c"])
    r.close()
    _case_cache[name] = d
    return d


@pytest.mark.parametrize("name", list(SC.GRID_CASES))
def test_analysis_meets_the_derived_bound(lib, name):
    d = case(lib, name)
    bound = SC.analysis_bound(name, d["x"], d["theta"], d["w"])
    err = np.abs(d["c_dev"] - d["c"])
    l, m = np.arange(d["c"].shape[-2])[:, None], np.arange(d["c"].shape[-1])[None, :]
    print(name, "analysis: max err", err.max(), "max err / bound", (err / np.maximum(bound, 1e-300)).max())
    assert (d["c_dev"][..., l < m] == 0).all()
    assert (err <= bound).all()


@pytest.mark.parametrize("name", list(SC.GRID_CASES))
def test_synthesis_meets_the_derived_bound(lib, name):
    d = case(lib, name)
    nlon = SC.geometry(name)[1]
    want = O.synthesis(d["coef"], d["theta"], nlon)
    bound = SC.synthesis_bound(name, d["coef"], d["theta"])[..., None]
    err = np.abs(d["x_dev"] - want)
    print(name, "synthesis: max err", err.max(), "max err / bound", (err / bound).max())
    assert (err <= bound).all()


@pytest.mark.parametrize("name", list(SC.GRID_CASES))
def test_vector_analysis_meets_the_derived_bound(lib, name):
    d = case(lib, name)
    _, _, _, lmax, mmax = SC.geometry(name)
    s, t = O.vector_analysis(d["u"], d["v"], d["theta"], d["w"], lmax, mmax)
    bs, bt = SC.vector_bound(name, d["u"], d["v"], d["theta"], d["w"])
    es, et = np.abs(d["s_dev"] - s), np.abs(d["t_dev"] - t)
    print(name, "vector: max err", es.max(), et.max(), "max err / bound", (es / np.maximum(bs, 1e-300)).max(), (et / np.maximum(bt, 1e-300)).max())
    assert (d["s_dev"][..., 0, :] == 0).all() and (d["t_dev"][..., 0, :] == 0).all()
    assert (es <= bs).all() and (et <= bt).all()
    assert np.abs(s).max() > 1.0 and np.abs(t).max() > 1.0


@pytest.mark.parametrize("name", list(SC.GRID_CASES))
def test_spectra_meet_the_propagated_bound(lib, name):
    d = case(lib, name)
    z, t = O.spectra(d["c"])
    bz, bt = SC.spectra_bound(d["c"], np.zeros(d["c"].shape))        # the device sums the oracle's own coefficients: only the sum's rounding
    zd, td = d["zt_dev"]
    print(name, "spectra: max rel err", (np.abs(zd - z) / z.max()).max(), (np.abs(td - t) / t.max()).max())
    assert (np.abs(zd - z) <= bz).all() and (np.abs(td - t) <= bt).all()
    # and of the device's own coefficients: the coefficient bound propagated
    dc = SC.analysis_bound(name, d["x"], d["theta"], d["w"])
    r = Raw(lib, name)
    zd2, td2 = r.spectra(d["c_dev"])
    r.close()
    bz2, bt2 = SC.spectra_bound(d["c"], dc)
    assert (np.abs(zd2 - z) <= bz2).all() and (np.abs(td2 - t) <= bt2).all()


@pytest.mark.parametrize("name", ["g8x16", "g64x128"])
def test_round_trip_on_gauss_grids(lib, name):
    nlat, nlon, grid, lmax, mmax = SC.geometry(name)
    theta, w = nodes(name)
    coef = SC.coefficients(lmax, mmax, 2, 7)
    x = O.synthesis(coef, theta, nlon)                         # band-limited to l < lmax = nlat: the Gauss quadrature is exact
    r = Raw(lib, name)
    c_dev = r.analysis(torch.from_numpy(x).cuda())
    back = r.synthesis(c_dev)
    r.close()
    dc = SC.analysis_bound(name, x, theta, w)
    T = np.abs(O.tables(lmax, mmax, theta)["P"])
    mult = np.full(mmax, 2.0)
    mult[0] = 1.0
    carried = np.einsum("mlk,...lm->...k", T, dc * mult * 2)   # re and im each within dc
    bound = (carried + SC.synthesis_bound(name, coef, theta))[..., None]
    err = np.abs(back - x)
    print(name, "round trip: max err", err.max(), "max err / bound", (err / bound).max())
    assert (err <= bound).all()


def test_scipy_built_wind_gives_its_potentials(lib):
    """u = grad chi + rhat x grad psi built from scipy's harmonics and gradients (tests/golden/sht_wind.npz): s = sqrt(l (l + 1)) chi and
    t = sqrt(l (l + 1)) psi to the derived vector bound plus the fixture's own distance from its potentials (`err`: that of the fp64
    oracle's transform of the fixture, stored when it was made); vorticity_divergence scales them by -sqrt(l (l + 1)) / a."""
    from wxengine.sht import SphericalHarmonics
    name = "g16x32w"
    g = np.load(os.path.join(SC.GOLD, "sht_wind.npz"))
    nlat, nlon, grid, lmax, mmax = SC.geometry(name)
    theta, w = nodes(name)
    sht = SphericalHarmonics(nlat, nlon, lmax=lmax, grid=grid, csphase=True)
    s, t = sht.vector_analysis(torch.from_numpy(g["u"]).cuda(), torch.from_numpy(g["v"]).cuda())
    L = np.sqrt(np.arange(lmax) * (np.arange(lmax) + 1.0))[:, None]
    bs, bt = SC.vector_bound(name, g["u"], g["v"], theta, w)
    es, et = np.abs(s.cpu().numpy() - L * g["chi"]), np.abs(t.cpu().numpy() - L * g["psi"])
    print("wind: max err", es.max(), et.max(), "fixture err", float(g["err"]))
    assert (es <= bs + float(g["err"])).all() and (et <= bt + float(g["err"])).all()
    vort, div = sht.vorticity_divergence(s, t, radius=2.0)
    f = torch.from_numpy(-L / 2.0).cuda()
    assert torch.equal(vort, f * t) and torch.equal(div, f * s)


def test_unfolded_rows_give_the_same_coefficients(lib):
    """A southern theta moved by two ulp of pi no longer sums to pi with its mirror: the handle runs unfolded (tests/test_sht_host.py
    checks the detection itself) and the unfolded contraction meets the same bars."""
    name = "e33x64p"
    d = case(lib, name)
    theta = d["theta"].copy()
    theta[-6] -= 2.0 ** -50
    nlat, nlon, _, lmax, mmax = SC.geometry(name)
    r = Raw(lib, name, theta=theta)
    c_dev = r.analysis(torch.from_numpy(d["x"]).cuda())
    x_dev = r.synthesis(d["coef"])
    s_dev, t_dev = r.vector(torch.from_numpy(d["u"]).cuda(), torch.from_numpy(d["v"]).cuda())
    r.close()
    assert not np.array_equal(c_dev, d["c_dev"])               # another order of summation: the fold is really off
    assert (np.abs(c_dev - O.analysis(d["x"], theta, d["w"], lmax, mmax)) <= SC.analysis_bound(name, d["x"], theta, d["w"])).all()
    assert (np.abs(x_dev - O.synthesis(d["coef"], theta, nlon)) <= SC.synthesis_bound(name, d["coef"], theta)[..., None]).all()
    s, t = O.vector_analysis(d["u"], d["v"], theta, d["w"], lmax, mmax)
    bs, bt = SC.vector_bound(name, d["u"], d["v"], theta, d["w"])
    assert (np.abs(s_dev - s) <= bs).all() and (np.abs(t_dev - t) <= bt).all()


# ---- bit for bit ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(lib):
    """33 planes (more than one pass) on 33 x 64, lmax = 34: everything of one call each."""
    name = "e33x64p"
    x, u, v = SC.field(name, 33, 11), SC.field(name, 33, 12, 30.0), SC.field(name, 33, 13, 20.0)
    nlat, nlon, _, lmax, mmax = SC.geometry(name)
    coef = SC.coefficients(lmax, mmax, 33, 14)
    r = Raw(lib, name)
    out = dict(name=name, x=x, u=u, v=v, coef=coef, c=r.analysis(torch.from_numpy(x).cuda()), xs=r.synthesis(coef))
    out["s"], out["t"] = r.vector(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda())
    out["z"], out["tot"] = r.spectra(out["c"])
    r.close()
    return out


@pytest.mark.parametrize("planes", [[0], [32], [1, 2, 3], list(range(5, 33))])
def test_a_plane_does_not_depend_on_the_call_it_is_in(lib, many, planes):
    """1, 3 and 28 planes, at other positions and in other passes than in the call on all 33."""
    r = Raw(lib, many["name"])
    sel = lambda a: torch.from_numpy(np.ascontiguousarray(a[planes])).cuda()   # noqa: E731
    assert np.array_equal(r.analysis(sel(many["x"])), many["c"][planes])
    assert np.array_equal(r.synthesis(many["coef"][planes]), many["xs"][planes])
    s, t = r.vector(sel(many["u"]), sel(many["v"]))
    assert np.array_equal(s, many["s"][planes]) and np.array_equal(t, many["t"][planes])
    z, tot = r.spectra(many["c"][planes])
    assert np.array_equal(z, many["z"][planes]) and np.array_equal(tot, many["tot"][planes])
    r.close()


def test_strided_planes_and_float32_input(lib, many):
    r = Raw(lib, many["name"])
    nlat, nlon = r.nlat, r.nlon
    x32 = torch.from_numpy(many["x"][:4].astype(np.float32)).cuda()
    wide = torch.full((4, nlat * nlon + 37), 3.5, device="cuda", dtype=torch.float32)
    wide[:, :nlat * nlon] = x32.reshape(4, -1)
    c32 = r.analysis(x32)
    assert np.array_equal(r.analysis(wide, stride=nlat * nlon + 37, P=4), c32)                     # a strided view, read where it lies
    assert np.array_equal(r.analysis(x32.double()), c32)                                          # float32 enters fp64 exactly
    u32, v32 = torch.from_numpy(many["u"][:2].astype(np.float32)).cuda(), torch.from_numpy(many["v"][:2].astype(np.float32)).cuda()
    s32, t32 = r.vector(u32, v32)
    s64, t64 = r.vector(u32.double(), v32.double())
    assert np.array_equal(s32, s64) and np.array_equal(t32, t64)
    r.close()


def test_csphase_is_the_sign_of_odd_orders(lib, many):
    r = Raw(lib, many["name"], csphase=0)
    c = r.analysis(torch.from_numpy(many["x"][:3]).cuda())
    s, t = r.vector(torch.from_numpy(many["u"][:3]).cuda(), torch.from_numpy(many["v"][:3]).cuda())
    xs = r.synthesis(many["coef"][:3] * np.where(np.arange(r.mmax) % 2, -1.0, 1.0))
    r.close()
    sign = np.where(np.arange(r.mmax) % 2, -1.0, 1.0)
    assert np.array_equal(c * sign, many["c"][:3]) and np.array_equal(s * sign, many["s"][:3]) and np.array_equal(t * sign, many["t"][:3])
    assert np.array_equal(xs, many["xs"][:3])


def test_synthesis_to_float32_is_the_float64_result_rounded_once(lib, many):
    r = Raw(lib, many["name"])
    x32 = r.synthesis(many["coef"][:3], torch.float32)
    r.close()
    assert x32.dtype == np.float32 and np.array_equal(x32, many["xs"][:3].astype(np.float32))


def test_the_python_layer_is_the_raw_abi(lib, many):
    """SphericalHarmonics, RealSHT / InverseRealSHT and the module's spectra against the raw calls, bit for bit; leading dimensions
    are planes and a strided view is accepted."""
    from wxengine import sht as S
    name = many["name"]
    nlat, nlon, grid, lmax, mmax = SC.geometry(name)
    sh = S.SphericalHarmonics(nlat, nlon, lmax=lmax, grid=grid)
    x = torch.from_numpy(many["x"][:6]).cuda()
    c = sh.analysis(x.view(2, 3, nlat, nlon))
    assert c.shape == (2, 3, lmax, mmax) and c.dtype == torch.complex128 and np.array_equal(c.cpu().numpy().reshape(6, lmax, mmax), many["c"][:6])
    both = torch.from_numpy(many["x"][:6]).cuda().view(3, 2, nlat, nlon)
    assert np.array_equal(sh.analysis(both[:, 1]).cpu().numpy(), many["c"][1:6:2])                  # a strided view
    back = sh.synthesis(torch.from_numpy(many["coef"][:3]).cuda())
    assert np.array_equal(back.cpu().numpy(), many["xs"][:3])
    assert np.array_equal(sh.synthesis(torch.from_numpy(many["coef"][:3]).cuda(), dtype=torch.float32).cpu().numpy(), many["xs"][:3].astype(np.float32))
    s, t = sh.vector_analysis(torch.from_numpy(many["u"][:3]).cuda(), torch.from_numpy(many["v"][:3]).cuda())
    assert np.array_equal(s.cpu().numpy(), many["s"][:3]) and np.array_equal(t.cpu().numpy(), many["t"][:3])
    z, tot = sh.spectra(c)
    assert np.array_equal(z.cpu().numpy().reshape(6, mmax), many["z"][:6]) and np.array_equal(tot.cpu().numpy().reshape(6, lmax), many["tot"][:6])
    assert np.array_equal(S.RealSHT(nlat, nlon, lmax=lmax, grid=grid)(x).cpu().numpy(), many["c"][:6])
    assert np.array_equal(S.InverseRealSHT(nlat, nlon, lmax=lmax, grid=grid)(torch.from_numpy(many["coef"][:3]).cuda()).cpu().numpy(), many["xs"][:3])
    # the module's functions use lmax = nlat + 1 = 34, this case's
    assert torch.equal(S.zonal_spectrum(x, grid), sh.spectra(sh.analysis(x))[0])
    assert np.array_equal(S.average_zonal_spectrum(x, grid), z.reshape(6, mmax).mean(dim=0).cpu().numpy())
    u, v = torch.from_numpy(many["u"][:3]).cuda(), torch.from_numpy(many["v"][:3]).cuda()
    off = S.SphericalHarmonics(nlat, nlon, lmax=lmax, grid=grid, csphase=False)
    s0, t0 = off.vector_analysis(u, v)
    rot, div = S.div_rot_spectrum(u, v, grid)
    assert torch.equal(rot, t0) and torch.equal(div, s0)
    for wave_spec, i in (("n", 1), ("m", 0)):
        a_rot, a_div = S.average_div_rot_spectrum(u, v, grid, wave_spec=wave_spec)
        assert np.array_equal(a_rot, off.spectra(t0)[i].mean(dim=0).cpu().numpy()) and np.array_equal(a_div, off.spectra(s0)[i].mean(dim=0).cpu().numpy())
    # and the oracle's restatement of the reference's functions (its own nodes: theta differs in the last bit)
    zo = O.zonal_spectrum(many["x"][:6], grid)
    assert np.allclose(S.zonal_spectrum(x, grid).cpu().numpy(), zo, rtol=1e-10, atol=1e-10 * zo.max())


def test_refusals_with_a_live_handle(lib):
    """Decided on the host before a launch: nothing is written."""
    r = Raw(lib, "g8x16")
    hw, st = r.nlat * r.nlon, r.stream()
    x = torch.zeros((2, r.nlat, r.nlon), device="cuda", dtype=torch.float64)
    buf, c = guarded((2, r.lmax, r.mmax, 2))
    calls = [
        (lambda: lib.wx_sht_analysis(r.h, 0, vp(x), hw, 1, vp(c), st), b"n_planes must be >= 1"),
        (lambda: lib.wx_sht_analysis(r.h, 2, vp(x), hw - 1, 1, vp(c), st), b"a plane stride is smaller than nlat * nlon"),
        (lambda: lib.wx_sht_analysis(r.h, 2, vp(x), 1 << 50, 1, vp(c), st), b"beyond 2^44"),
        (lambda: lib.wx_sht_analysis(r.h, 2, vp(x), hw, 2, vp(c), st), b"dtype must be 0 (float32) or 1 (float64)"),
        (lambda: lib.wx_sht_analysis(r.h, 2, None, hw, 1, vp(c), st), b"null pointer"),
        (lambda: lib.wx_sht_analysis(r.h, 1, vp(x), hw, 1, vp(x), st), b"an output overlaps an input"),
        (lambda: lib.wx_sht_synthesis(r.h, 1, vp(c), vp(c), 1, st), b"an output overlaps an input"),
        (lambda: lib.wx_sht_vector_analysis(r.h, 1, vp(x), hw, vp(x[1]), hw, 1, vp(c), vp(c), st), b"two outputs overlap"),
        (lambda: lib.wx_sht_spectra(r.h, 1, vp(c), None, None, st), b"no output requested"),
        (lambda: lib.wx_sht_spectra(r.h, 1, vp(c), vp(c), None, st), b"an output overlaps an input"),
    ]
    for call, why in calls:
        assert call() == -1 and why in lib.wx_last_error(), (why, lib.wx_last_error())
    torch.cuda.synchronize()
    assert guards_ok(buf) and bool((c == FILL).all())
    r.close()
