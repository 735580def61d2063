"""The inverse vector transform and the diffusion and pole filter on the device (csrc/wx_sht.h, csrc/wx_polefilter.h, through
wxengine/sht.py, wxengine/pole_filter.py and the raw C ABI of include/wxengine_polefilter.h) against the numpy oracle
(tests/polefilter_oracle.py) and its fixtures (tools/make_polefilter_goldens.py).

The bars are derived or measured on the CPU, never taken from the device (tests/polefilter_cases.py):
  vector synthesis  ((2 lmax + 2 mmax + 16) u 2 + 2 E_tab) sum_m mult_m sum_l (|dPt| + |Qt|) |lscale_l| (|re s| + |im s| + |re t| + |im t|)
  low-pass          2 (i + 1) (nlon + 16) u sum_j |x_kj| / nlon on a filtered row; every other row, row 0 included, bit for bit
  V1, QV1, V2, diff_lap2d_filt   16 E_ref, E_ref the distance of the fp64 oracle from the same chain in np.longdouble, plus 2^-24 max |x|
                    for a float32 output; the bar is asserted to lie below 1e-6 of the largest increment of the sub-steps
Everything else is bit for bit: a plane whatever the batch and its position, in place against out of place, strided against contiguous,
null t against a zero t, one component against both, filter_rollout against direct calls."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import polefilter_cases as PC  # noqa: E402
import polefilter_oracle as PO  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
WX_ERR_INVALID = -1
_made = {}


def transform(name):
    from wxengine.sht import SphericalHarmonics
    if ("sht", name) not in _made:
        nlat, nlon, grid, lmax, mmax, _ = PC.SYNTHESIS_CASES[name]
        _made[("sht", name)] = SphericalHarmonics(nlat, nlon, lmax, mmax, grid, csphase=False)
    return _made[("sht", name)]


def pole_filter(name):
    from wxengine.pole_filter import Diffusion_and_Pole_Filter
    if ("dpf", name) not in _made:
        nlat, nlon, grid, lmax, mmax, i = PC.FILTER_CASES[name]
        d = Diffusion_and_Pole_Filter(nlat, nlon, "cuda", lmax, mmax, grid, radius=PC.radius(nlat))
        assert d.cutoff == i and np.array_equal(d.sigmoid, PO.sigmoid_ramp(nlat))
        _made[("dpf", name)] = d
    return _made[("dpf", name)]


def geometry(name):
    if ("geo", name) not in _made:
        _made[("geo", name)] = PC.geometry(name)
    return _made[("geo", name)]


def golden(name):
    if ("gold", name) not in _made:
        _made[("gold", name)] = dict(np.load(os.path.join(PC.GOLD, f"polefilter_{name}.npz")))
    return _made[("gold", name)]


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def host(t):
    return t.cpu().numpy()


def vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- 1. the inverse vector transform -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PC.SYNTHESIS_CASES))
def test_vector_synthesis_against_the_oracle(name):
    sht, G = transform(name), geometry(name)
    assert np.array_equal(sht.theta, G.theta)                  # the oracle's mirrored nodes are the device's
    s, t = PC.coefficients(name, 3, 1), PC.coefficients(name, 3, 2)
    u, v = sht.vector_synthesis(dev(s, torch.complex128), dev(t, torch.complex128))
    uo, vo = G.vector_synthesis(s, t)
    bound = PC.vector_synthesis_bound(name, G, s, t)[..., None]
    assert u.dtype == torch.float64 and u.shape == (3, G.nlat, G.nlon)
    eu, ev = np.abs(host(u) - uo), np.abs(host(v) - vo)
    print(name, "worst ratio to the bound", float((eu / bound).max()), float((ev / bound).max()))
    assert (eu <= bound).all() and (ev <= bound).all()
    assert np.abs(uo).max() > 0.1 and np.abs(vo).max() > 0.1
    # null t: the gradient form, against the oracle and bit for bit a zero t
    g_u, g_v = sht.vector_synthesis(dev(s, torch.complex128))
    z_u, z_v = sht.vector_synthesis(dev(s, torch.complex128), dev(np.zeros_like(t), torch.complex128))
    uo, vo = G.vector_synthesis(s)
    bound = PC.vector_synthesis_bound(name, G, s)[..., None]
    assert (np.abs(host(g_u) - uo) <= bound).all() and (np.abs(host(g_v) - vo) <= bound).all()
    assert torch.equal(g_u, z_u) and torch.equal(g_v, z_v)
    # one component alone is that component of both, with and without t; float32 is the float64 result rounded once
    for tt, (bu, bv) in ((t, (u, v)), (None, (g_u, g_v))):
        td = None if tt is None else dev(tt, torch.complex128)
        only_u, none_v = sht.vector_synthesis(dev(s, torch.complex128), td, components="u")
        none_u, only_v = sht.vector_synthesis(dev(s, torch.complex128), td, components="v")
        assert none_u is None and none_v is None and torch.equal(only_u, bu) and torch.equal(only_v, bv)
    u32, v32 = sht.vector_synthesis(dev(s, torch.complex128), dev(t, torch.complex128), dtype=torch.float32)
    assert u32.dtype == torch.float32 and torch.equal(u32, u.float()) and torch.equal(v32, v.float())


@pytest.mark.parametrize("name", ["g24x144", "e33x160", "g24x144r", "g8x16"])
def test_vector_synthesis_is_bit_identical_whatever_the_batch(name):
    sht = transform(name)
    s, t = PC.coefficients(name, 3, 1), PC.coefficients(name, 3, 2)
    u3, v3 = sht.vector_synthesis(dev(s, torch.complex128), dev(t, torch.complex128))
    order = [(5 * p + 2) % 3 for p in range(33)]               # more than one 32-plane pass, every plane at many positions
    u33, v33 = sht.vector_synthesis(dev(s[order], torch.complex128), dev(t[order], torch.complex128))
    for p, src in enumerate(order):
        assert torch.equal(u33[p], u3[src]) and torch.equal(v33[p], v3[src]), p
    for src in range(3):
        u1, v1 = sht.vector_synthesis(dev(s[src], torch.complex128), dev(t[src], torch.complex128))
        assert u1.shape == u3.shape[1:] and torch.equal(u1, u3[src]) and torch.equal(v1, v3[src])
    g3 = sht.vector_synthesis(dev(s, torch.complex128), components="u")[0]
    g33 = sht.vector_synthesis(dev(s[order], torch.complex128), components="u")[0]
    assert all(torch.equal(g33[p], g3[src]) for p, src in enumerate(order))


@pytest.mark.parametrize("name", ["g24x144", "g32x256", "g24x144r", "g8x16"])
def test_gauss_round_trip_with_the_vector_analysis(name):
    """Coefficients cut at lcut = nlat // 2: the Gauss quadrature of the analysis is exact for them, so analysis(synthesis(s, t)) = (s, t)
    up to the synthesis bound carried through the analysis, sum_k |w_k| (|dPt| + |Qt|) 2 pi (du_k + dv_k), plus the analysis' own error
    (sht_cases.vector_bound's form with this file's E_tab)."""
    sht, G = transform(name), geometry(name)
    lcut = min(G.nlat // 2, G.lmax)
    s, t = PC.coefficients(name, 3, 3, lcut), PC.coefficients(name, 3, 4, lcut)
    s[:, 0], t[:, 0] = 0, 0
    u, v = sht.vector_synthesis(dev(s, torch.complex128), dev(t, torch.complex128))
    s2, t2 = sht.vector_analysis(u, v)
    T = (np.abs(G.tab["dP"]) + np.abs(G.tab["Q"])) * np.abs(G.w)
    d_field = PC.vector_synthesis_bound(name, G, s, t)                                    # [3, nlat], per component
    mass = 2 * np.pi / G.nlon * (np.abs(host(u)).sum(axis=-1) + np.abs(host(v)).sum(axis=-1))
    gamma = (2 * (G.nlon + G.nlat) + 16) * U * 2 + 2 * PC.E_TAB[name]
    bound = np.einsum("mlk,...k->...lm", T, 2 * np.pi * 2 * d_field + gamma * mass)
    # the oracle's own round trip closes to 1e-14 (tests/test_polefilter_cpu.py); the device's to its bound
    es, et = np.abs(host(s2) - s), np.abs(host(t2) - t)
    print(name, "round trip", es.max(), et.max(), "bound at the worst entry", float(bound.flat[np.argmax(es)]))
    assert (es <= bound + 1e-14).all() and (et <= bound + 1e-14).all()


@pytest.mark.parametrize("name", ["g24x144", "e33x160", "g24x144r"])
def test_getgrad_carries_the_per_degree_scale(name):
    d, G = pole_filter(name), geometry(name)
    c = PC.coefficients(name, 3, 5)
    gx, gy = d.getgrad(dev(c, torch.complex128))
    ox, oy = G.grad(c)
    lscale = (G.sq / G.radius)[:, 0]
    bound = PC.vector_synthesis_bound(name, G, c, lscale=lscale)[..., None]
    assert (np.abs(host(gx) - ox) <= bound).all() and (np.abs(host(gy) - oy) <= bound).all() and np.abs(ox).max() > 0
    # grid2spec and spec2grid are the handle's own transform
    x = PC.temperature(name, 2)
    cs = d.grid2spec(dev(x))
    assert np.abs(host(cs) - G.analysis(x)).max() <= 1e-11 * np.abs(G.analysis(x)).max()
    assert np.abs(host(d.spec2grid(cs)) - G.synthesis(G.analysis(x))).max() <= 1e-11 * 300


# ---- 2. the low-pass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PC.FILTER_CASES))
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_low_pass(name, dtype):
    d, g = pole_filter(name), golden(name)
    i, nlat = PC.FILTER_CASES[name][5], PC.FILTER_CASES[name][0]
    x = np.concatenate([g["T"], g["U"][:1]])                   # 3 planes
    xd = dev(x, dtype)
    xin = host(xd).astype(np.float64)                          # what the device reads
    keep = xd.clone()
    y = d.polfiltT(xd)
    assert y.dtype == dtype and y.shape == xd.shape and torch.equal(xd, keep) and y.data_ptr() != xd.data_ptr()
    want = PO.polfilt_fft(xin, i)
    rows = PC.filtered_rows(nlat)
    other = [k for k in range(nlat) if k not in rows]
    assert 0 in other and nlat - 1 in rows
    assert torch.equal(y[:, other], xd[:, other])              # row 0 included: bit for bit
    bound = PC.lowpass_bound(xin, i)[..., None] + (2.0 ** -24 * np.abs(want) if dtype == torch.float32 else 0.0)
    err = np.abs(host(y).astype(np.float64) - want)
    print(name, dtype, "worst ratio to the bound", float((err / bound)[:, rows].max()))
    assert (err[:, rows] <= bound[:, rows]).all()
    if i == 0:
        assert torch.equal(y, xd)                              # nothing is launched on the rows: the identity
        for fn in (d.polefilt_lap2d_V1, d.polefilt_lap2d_QV1):
            assert torch.equal(fn(xd, 0), xd)
        u0, v0 = d.polefilt_lap2d_V2(xd, xd.flip(0), 0)
        assert torch.equal(u0, xd) and torch.equal(v0, xd.flip(0))
    else:
        assert np.abs(want - xin)[:, rows].max() > 1.0         # the test sees the filter
        assert torch.equal(d.polefilt_lap2d_V1(xd, 0), y)      # substeps = 0 is the low-pass alone
        assert torch.equal(d.polefilt_lap2d_V2(xd, xd, 0)[1], y)
    assert torch.equal(d.polfiltT(xd[1]), y[1])                # a 2-D field


# ---- 3. the filters against the oracle's fp64 result -------------------------------------------------------------------------------
def run_variant(d, var, T, Uw, Vw):
    if var == "V1":
        return (d.polefilt_lap2d_V1(T, PC.SUBSTEPS[var]),)
    if var == "QV1":
        return (d.polefilt_lap2d_QV1(T, PC.SUBSTEPS[var]),)
    return d.polefilt_lap2d_V2(Uw, Vw, PC.SUBSTEPS[var])


@pytest.mark.parametrize("name", sorted(PC.FILTER_CASES))
@pytest.mark.parametrize("var", ["V1", "QV1", "V2"])
def test_filters_against_the_fixture(name, var):
    d, g = pole_filter(name), golden(name)
    bar = 16 * PC.E_REF[(name, var)]
    assert bar < 1e-6 * PC.INCREMENT[(name, var)]
    want = (g[var],) if var != "V2" else (g["V2u"], g["V2v"])
    got = run_variant(d, var, dev(g["T"]), dev(g["U"]), dev(g["V"]))
    for a, b in zip(got, want):
        err = np.abs(host(a) - b).max()
        print(name, var, "distance from the oracle", err, "bar", bar)
        assert a.dtype == torch.float64 and np.isfinite(host(a)).all() and err <= bar
    # strided views are read where they lie; in place is out of place, bit for bit
    big = torch.full((PC.GOLD_PLANES, 3, *g["T"].shape[1:]), -7777.25, device="cuda", dtype=torch.float64)
    big[:, 0], big[:, 1], big[:, 2] = dev(g["T"]), dev(g["U"]), dev(g["V"])
    strided = run_variant(d, var, big[:, 0], big[:, 1], big[:, 2])
    assert all(torch.equal(a, b) for a, b in zip(strided, got))
    if var == "V2":
        d._vector(big[:, 1], big[:, 2], PC.SUBSTEPS[var], 2e16, inplace=True)
        assert torch.equal(big[:, 1], got[0]) and torch.equal(big[:, 2], got[1]) and torch.equal(big[:, 0], dev(g["T"]))
    else:
        d._scalar(big[:, 0], PC.SUBSTEPS[var], 1e8 if var == "V1" else 0.5e8, inplace=True)
        assert torch.equal(big[:, 0], got[0]) and torch.equal(big[:, 1], dev(g["U"]))


@pytest.mark.parametrize("var", ["V1", "V2"])
def test_filters_float32(var):
    """float32 fields: the oracle on the float32 values, the bar 16 E_ref plus one rounding of the output, 2^-24 max |x|."""
    name = "g24x144"
    d, g, G = pole_filter(name), golden(name), geometry(name)
    i, sig = PC.FILTER_CASES[name][5], PO.sigmoid_ramp(G.nlat)
    T, Uw, Vw = (dev(g[k][:1], torch.float32) for k in ("T", "U", "V"))
    Th, Uh, Vh = (host(a).astype(np.float64) for a in (T, Uw, Vw))
    if var == "V1":
        want = (PO.polefilt_lap2d_V1(G, Th, PC.SUBSTEPS[var], sig, i),)
    else:
        want = PO.polefilt_lap2d_V2(G, Uh, Vh, PC.SUBSTEPS[var], sig, i)
    got = run_variant(d, var, T, Uw, Vw)
    for a, b in zip(got, want):
        bar = 16 * PC.E_REF[(name, var)] + 2.0 ** -24 * np.abs(b).max()
        assert a.dtype == torch.float32 and np.abs(host(a).astype(np.float64) - b).max() <= bar
    # the same values as float64 give the same fp64 chain: the float32 result is its one rounding
    got64 = run_variant(d, var, T.double(), Uw.double(), Vw.double())
    assert all(torch.equal(a, b.float()) for a, b in zip(got, got64))


def test_a_plane_is_bit_identical_whatever_the_batch():
    name = "e33x160"
    d, g = pole_filter(name), golden(name)
    T, Uw, Vw = dev(g["T"]), dev(g["U"]), dev(g["V"])
    v1 = d.polefilt_lap2d_V1(T, 2)
    u2, v2 = d.polefilt_lap2d_V2(Uw, Vw, 2)
    order = [(3 * p + 1) % 2 for p in range(33)]               # three chunks of 16, 16 and 1 planes
    b1 = d.polefilt_lap2d_V1(T[order], 2)
    bu, bv = d.polefilt_lap2d_V2(Uw[order], Vw[order], 2)
    for p, src in enumerate(order):
        assert torch.equal(b1[p], v1[src]) and torch.equal(bu[p], u2[src]) and torch.equal(bv[p], v2[src]), p
    one = d.polefilt_lap2d_V1(T[1], 2)
    assert one.shape == T.shape[1:] and torch.equal(one, v1[1])
    ou, ov = d.polefilt_lap2d_V2(Uw[0], Vw[0], 2)
    assert torch.equal(ou, u2[0]) and torch.equal(ov, v2[0])


# ---- 4. diff_lap2d_filt and the rollout ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def diff():
    d = pole_filter(PC.DIFF_CASE)
    B = PC.diff_tensor()
    want = np.concatenate([np.load(os.path.join(PC.GOLD, f))["expected"] for f in PC.DIFF_FILES])
    return d, B, want, d.diff_lap2d_filt(dev(B))


def test_diff_lap2d_filt_against_the_fixture(diff):
    d, B, want, got = diff
    bar = 16 * PC.E_REF_DIFF
    assert bar < 1e-6 * PC.INCREMENT_DIFF
    err = np.abs(host(got) - want).max(axis=(1, 2))
    print("diff_lap2d_filt: distance from the oracle per channel group", err[:32].max(), err[32:64].max(), err[64:].max(), "bar", bar)
    assert got.shape == (70, 24, 144) and err.max() <= bar
    # channels beyond 70 are copied; a float32 tensor is the fp64 chain of its values rounded once
    more = torch.cat([dev(B), dev(B[:2]) + 1.0])
    out = d.diff_lap2d_filt(more)
    assert torch.equal(out[:70], got) and torch.equal(out[70:], more[70:])
    b32 = dev(B, torch.float32)
    keep = b32.clone()
    o32 = d.diff_lap2d_filt(b32)
    assert o32.dtype == torch.float32 and torch.equal(b32, keep) and torch.equal(o32, d.diff_lap2d_filt(b32.double()).float())


def test_filter_rollout_is_two_direct_calls(diff):
    from wxengine.rollout import filter_rollout
    d, B, want, got = diff
    steps = [dev(B, torch.float32)[None].clone(), (dev(B, torch.float32) * 1.01)[None].clone()]
    direct = [d.diff_lap2d_filt(y[0]) for y in steps]
    out = filter_rollout(steps, d)
    assert out is steps and all(y.shape == (1, 70, 24, 144) for y in out)
    assert torch.equal(out[0][0], direct[0]) and torch.equal(out[1][0], direct[1])
    with pytest.raises(ValueError, match=r"must be \[1, C, H, W\]"):
        filter_rollout([steps[0][0]], d)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_the_class_refuses():
    from wxengine.native import WXEngineError
    from wxengine.pole_filter import Diffusion_and_Pole_Filter
    d = pole_filter("g24x144")
    good = torch.zeros((2, 24, 144), device="cuda")
    for bad in (torch.zeros((2, 24, 144)), torch.zeros((2, 24, 143), device="cuda"), torch.zeros((2, 25, 144), device="cuda"),
                torch.zeros((2, 24, 144), device="cuda", dtype=torch.float16), torch.zeros((1, 2, 24, 144), device="cuda"), torch.zeros(144, device="cuda")):
        for call in (lambda: d.polefilt_lap2d_V1(bad, 5), lambda: d.polefilt_lap2d_QV1(bad, 8), lambda: d.polefilt_lap2d_V2(bad, bad, 6),
                     lambda: d.polefilt_lap2d_V2(good, bad, 6), lambda: d.polfiltT(bad), lambda: d.diff_lap2d_filt(bad)):
            with pytest.raises(WXEngineError):
                call()
    with pytest.raises(WXEngineError, match="must be one shape and dtype"):
        d.polefilt_lap2d_V2(good, good[:1], 6)
    with pytest.raises(WXEngineError, match="at least 70 channels, got 69"):
        d.diff_lap2d_filt(torch.zeros((69, 24, 144), device="cuda"))
    with pytest.raises(ValueError, match="substeps must be >= 0"):
        d.polefilt_lap2d_V1(good, -1)
    with pytest.raises(ValueError, match="nlat must be >= 21, got 20"):
        Diffusion_and_Pole_Filter(20, 144, "cuda")


def test_the_abi_refuses_and_launches_nothing():
    from wxengine.native import load_library
    lib = load_library()
    d = pole_filter("g24x144")
    h, hw = d._h, 24 * 144
    x = torch.arange(3 * hw, device="cuda", dtype=torch.float64)
    y = torch.full((4 * hw,), -7777.25, device="cuda", dtype=torch.float64)
    keep_x, keep_y = x.clone(), y.clone()
    nan, inf = float("nan"), float("inf")

    def scalar(n=3, xp=x, xs=hw, dtype=1, sub=2, coef=1e8, op=y, os_=hw):
        return lib.wx_polefilter_scalar(h, n, vp(xp), xs, dtype, sub, coef, vp(op), os_, stream())

    def vector(n=1, up=x, us=hw, vp_=x[hw:], vs=hw, dtype=1, sub=2, coef=2e16, uo=y, uos=hw, vo=y[hw:], vos=hw):
        return lib.wx_polefilter_vector(h, n, vp(up), us, vp(vp_), vs, dtype, sub, coef, vp(uo), uos, vp(vo), vos, stream())
    for call, why in ((lambda: scalar(xp=None), b"a null pointer"), (lambda: scalar(op=None), b"a null pointer"), (lambda: scalar(n=0), b"n_planes must be >= 1, got 0"),
                    (lambda: scalar(dtype=2), b"dtype must be 0 (float32) or 1 (float64)"), (lambda: scalar(xs=hw - 1), b"a plane stride is smaller than nlat * nlon"),
                    (lambda: scalar(os_=hw - 1), b"a plane stride is smaller"), (lambda: scalar(sub=-1), b"substeps must be >= 0, got -1"),
                    (lambda: scalar(coef=nan), b"coef must be finite"), (lambda: scalar(coef=inf), b"coef must be finite"),
                    (lambda: scalar(op=x[8:]), b"an output overlaps an input that is not its own"), (lambda: scalar(op=x, os_=hw + 8, n=2), b"an output overlaps an input that is not its own"),
                    (lambda: vector(vp_=None), b"a null pointer"), (lambda: vector(vo=None), b"a null pointer"), (lambda: vector(uo=None), b"a null pointer"),
                    (lambda: vector(vo=y[8:]), b"two outputs overlap"), (lambda: vector(uo=x[hw:]), b"an output overlaps an input that is not its own"),
                    (lambda: vector(n=0), b"n_planes must be >= 1"), (lambda: vector(sub=-2), b"substeps must be >= 0"), (lambda: vector(coef=nan), b"coef must be finite"),
                    (lambda: vector(vs=3), b"a plane stride is smaller")):
        assert call() == WX_ERR_INVALID and why in lib.wx_last_error(), lib.wx_last_error()
    st = lib.wx_polefilter_lowpass(h, 1, vp(x), hw, 1, vp(x[4:]), hw, stream())
    assert st == WX_ERR_INVALID and b"wx_polefilter_lowpass: an output overlaps" in lib.wx_last_error()
    c = torch.zeros((24, 24, 2), device="cuda", dtype=torch.float64)
    sh = d.sht._h
    for call, why in ((lambda: lib.wx_sht_vector_synthesis(sh, 1, None, None, vp(y), vp(y[hw:]), 1, stream()), b"the spheroidal coefficients are needed"),
                    (lambda: lib.wx_sht_vector_synthesis(sh, 1, vp(c), None, None, None, 1, stream()), b"no output requested: u and v are both null"),
                    (lambda: lib.wx_sht_vector_synthesis(sh, 0, vp(c), None, vp(y), None, 1, stream()), b"n_planes must be >= 1"),
                    (lambda: lib.wx_sht_vector_synthesis(sh, 1, vp(c), None, vp(y), None, 5, stream()), b"dtype must be 0"),
                    (lambda: lib.wx_sht_vector_synthesis(sh, 1, vp(c), None, vp(y), vp(y[8:]), 1, stream()), b"two outputs overlap"),
                    (lambda: lib.wx_sht_vector_synthesis(sh, 1, vp(c), vp(c), vp(c), None, 1, stream()), b"an output overlaps an input"),
                    (lambda: lib.wx_polefilter_gradient(h, 1, vp(c), vp(y), None, 1, stream()), b"both components are needed")):
        assert call() == WX_ERR_INVALID and why in lib.wx_last_error(), lib.wx_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, keep_x) and torch.equal(y, keep_y)
    # in place (the same address and stride) is accepted
    assert scalar(op=x, sub=0) == 0, lib.wx_last_error()
    torch.cuda.synchronize()
    assert torch.equal(y, keep_y) and torch.equal(x.view(3, 24, 144)[:, 0], keep_x.view(3, 24, 144)[:, 0]) and not torch.equal(x, keep_x)
