"""The host side of the spherical harmonic transforms without a GPU: the lazy exports and the refusal to run on the CPU, every refusal
of the Python mirror and of the C ABI with its message (the library's come before any device is asked for), the extension header
against native._EXTENSION_PROTOTYPES argument by argument, null handles, the nodes of grid_nodes, and the library's host-built tables
(wx_sht_table) against the oracle and against scipy's values in tests/golden/sht_tables.npz.

E_tab, the largest absolute difference of a table (Pbar, dPt, Qt; lmax = nlat + 1) from the same recurrence in np.longdouble, must be at
most twice the same figure of the oracle's own fp64 table.  Measured (the library's tables are bit for bit the oracle's, so the two
figures agree), the largest of the three tables:
    equiangular      nlat 8: 6.92e-16   9: 5.15e-16   33: 2.25e-14   37: 1.76e-14   64: 4.66e-14   181: 7.29e-13   721: 8.07e-12
    legendre-gauss   nlat 8: 1.12e-15   9: 1.66e-15   16: 5.11e-15   33: 1.32e-14   64: 6.17e-14   181: 3.34e-13   721: 6.54e-12
(nlat = 181 and 721 over the orders 0, 1, 2, nlat // 2 - 1, nlat // 2, nlat - 1, nlat; the smaller ones over every order).  These are the
figures of sht_cases.E_TAB, which the device tests' bars use.  They come from one libm's cos, sin and sqrt; this file asserts that the
library stays below E_TAB_MARGIN = 1.5 times them, the room given to another libm's last bits (the issue's own requirement is the
comparison with the oracle's table, asserted without a margin)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import sht_cases as SC  # noqa: E402
import sht_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"wx_sht_create", "wx_sht_destroy", "wx_sht_analysis", "wx_sht_synthesis", "wx_sht_vector_analysis", "wx_sht_spectra", "wx_sht_table"}
WX_ERR_INVALID = -1
E_TAB_MARGIN = 1.5


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("wx_build", os.path.join(ROOT, "miles-credit_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(force=False, verbose=False)
    from wxengine.native import load_library
    return load_library()


@pytest.fixture()
def S(monkeypatch):
    import wxengine.sht as S
    monkeypatch.setattr(S.SphericalHarmonics, "_open", lambda self, device: None)
    return S


def f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))


def test_exported_lazily_and_raises_without_a_gpu():
    import torch
    import wxengine
    from wxengine.native import WXEngineError
    for name in ("SphericalHarmonics", "RealSHT", "InverseRealSHT", "grid_nodes", "zonal_spectrum", "average_zonal_spectrum", "div_rot_spectrum",
                 "average_div_rot_spectrum"):
        assert getattr(wxengine, name) is getattr(wxengine.sht, name)
    if not torch.cuda.is_available():
        with pytest.raises(WXEngineError, match="no CPU fallback"):
            wxengine.SphericalHarmonics(9, 16)
        with pytest.raises(WXEngineError, match="no CPU fallback"):
            wxengine.zonal_spectrum(torch.zeros((9, 16)), "equiangular")
        with pytest.raises(WXEngineError, match="no CPU fallback"):
            wxengine.RealSHT(9, 16)(torch.zeros((9, 16)))
    with pytest.raises(ValueError, match="nlat must be an integer >= 2"):        # the argument's own faults come first
        wxengine.SphericalHarmonics(1, 16)


def test_constructor_refusals_and_defaults(S):
    for nlat, nlon in ((1, 16), (9, 1), (9.5, 16), (True, 16)):
        with pytest.raises(ValueError, match="must be an integer >= 2"):
            S.SphericalHarmonics(nlat, nlon)
    with pytest.raises(ValueError, match="nlon must be <= 4096"):
        S.SphericalHarmonics(9, 4097)
    for norm in ("backward", "schmidt", None):
        for make in (S.SphericalHarmonics, S.RealSHT, S.InverseRealSHT):
            with pytest.raises(ValueError, match='only norm="ortho" is supported: the meaning of'):
                make(9, 16, norm=norm)
    with pytest.raises(ValueError, match="grid must be one of"):
        S.SphericalHarmonics(9, 16, grid="lobatto")
    for lmax in (0, -1, 2.5, 40000):
        with pytest.raises(ValueError, match="lmax must be an integer in 1"):
            S.SphericalHarmonics(9, 16, lmax=lmax)
    for lmax, mmax in ((9, 0), (9, 10), (20, 10), (4, 5), (9, 2.5)):
        with pytest.raises(ValueError, match=r"mmax must be an integer in 1 \.\. min\(lmax, nlon // 2 \+ 1\)"):
            S.SphericalHarmonics(9, 16, lmax=lmax, mmax=mmax)
    s = S.SphericalHarmonics(9, 16)
    assert (s.lmax, s.mmax, s.grid, s.norm, s.csphase) == (9, 9, "equiangular", "ortho", True)
    assert S.SphericalHarmonics(33, 64, lmax=34).mmax == 33 and S.SphericalHarmonics(721, 1440, lmax=722).mmax == 721
    assert S.SphericalHarmonics(33, 64, lmax=20, mmax=7, grid="legendre-gauss").mmax == 7
    r = S.RealSHT(9, 16, lmax=10, grid="legendre-gauss", norm="ortho", csphase=False)      # torch_harmonics' signature
    assert (r.nlat, r.nlon, r.lmax, r.mmax, r.csphase) == (9, 16, 10, 9, False)


def test_calls_refuse_what_is_not_a_device_tensor(S):
    import torch
    from wxengine.native import WXEngineError
    s = S.SphericalHarmonics(9, 16)
    s.device = torch.device("cuda", 0)
    for bad in (np.zeros((2, 9, 16)), torch.zeros((2, 9, 16)), torch.zeros(16)):
        with pytest.raises(WXEngineError, match=r"x must be a CUDA tensor \[\.\.\., 9, 16\] of dtype torch.float32 or torch.float64"):
            s.analysis(bad)
        with pytest.raises(WXEngineError, match="u must be a CUDA tensor"):
            s.vector_analysis(bad, bad)
        with pytest.raises(WXEngineError, match=r"c must be a CUDA tensor \[\.\.\., 9, 9\] of dtype torch.complex128"):
            s.synthesis(bad)
        with pytest.raises(WXEngineError, match="c must be a CUDA tensor"):
            s.spectra(bad)
    with pytest.raises(ValueError, match="dtype must be torch.float32 or torch.float64"):
        s.synthesis(None, dtype=torch.float16)


def test_vorticity_divergence_is_the_documented_scaling(S):
    import torch
    s = S.SphericalHarmonics(9, 16)
    a = torch.arange(81, dtype=torch.float64).reshape(9, 9).to(torch.complex128) + 1j
    b = a * (0.5 - 2j)
    vort, div = s.vorticity_divergence(a, b, radius=6.371e6)
    f = -np.sqrt(np.arange(9.0) * (np.arange(9.0) + 1))[:, None] / 6.371e6
    for got, want in ((vort.numpy(), f * b.numpy()), (div.numpy(), f * a.numpy())):      # one rounding per product and per division
        assert np.abs(got - want).max() <= 2.0 ** -51 * np.abs(want).max() and (got[0] == 0).all()


@pytest.mark.parametrize("grid", ["equiangular", "legendre-gauss"])
@pytest.mark.parametrize("nlat", [2, 3, 8, 9, 33, 64, 181, 721])
def test_grid_nodes(grid, nlat):
    """numpy only; ascending, the oracle's to rounding, summing to 2, and symmetric bit for bit as the device fold tests it."""
    from wxengine.sht import grid_nodes
    theta, w = grid_nodes(nlat, grid)
    to, wo = O.nodes(nlat, grid) if nlat <= 181 else (theta, w)
    assert theta.dtype == np.float64 and w.dtype == np.float64 and theta.shape == w.shape == (nlat,)
    assert (np.diff(theta) > 0).all() and theta[0] >= 0 and theta[-1] <= np.pi
    assert np.abs(theta - to).max() <= 4 * np.pi * 2.0 ** -53 and np.abs(w - wo).max() <= 64 * 2.0 ** -53
    assert abs(w.sum() - 2.0) <= nlat * 2.0 ** -52
    assert np.array_equal(theta + theta[::-1], np.full(nlat, np.pi)) and np.array_equal(w, w[::-1])
    if grid == "equiangular":
        assert theta[0] == 0.0 and theta[-1] == np.pi
    # exactness: a Gauss rule integrates x^p for p <= 2 nlat - 1, Clenshaw-Curtis for p <= nlat - 1
    x = np.cos(theta)
    for p in range(0, (2 * nlat if grid == "legendre-gauss" else nlat) if nlat <= 64 else 8):
        exact = 0.0 if p % 2 else 2.0 / (p + 1)
        assert abs((w * x ** p).sum() - exact) <= 8 * nlat * 2.0 ** -53, (p, (w * x ** p).sum())


def _header_declarations():
    """{name: [argument text]} of every `int wx_name(args);` of include/wxengine_sht.h, comments stripped."""
    hdr = open(os.path.join(ROOT, "include", "wxengine_sht.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    decls = {}
    for name, args in re.findall(r"\b(?:int|const\s+char\s*\*)\s*(wx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr):
        args = " ".join(args.split())
        decls[name] = [] if args in ("", "void") else [a.strip() for a in args.split(",")]
    return decls


_SCALARS = {"int": (C.c_int, C.c_int32), "int32_t": (C.c_int, C.c_int32), "int64_t": (C.c_int64,), "uint64_t": (C.c_uint64,),
            "float": (C.c_float,), "double": (C.c_double,)}


def test_extension_prototypes_match_the_header_argument_by_argument(lib):
    from wxengine.native import _EXTENSION_PROTOTYPES, _PROTOTYPES, exported_symbols
    decls = _header_declarations()
    assert set(decls) == NAMES == set(_EXTENSION_PROTOTYPES)
    assert len(_PROTOTYPES) == 111 and not NAMES & set(_PROTOTYPES) and not NAMES & set(exported_symbols())
    main = open(os.path.join(ROOT, "include", "wxengine.h")).read()
    assert "wx_sht" not in main and "wxengine_sht.h" not in main
    for name, args in sorted(decls.items()):
        assert hasattr(lib, name), f"{name} declared in include/wxengine_sht.h but not exported"
        ctypes_args = _EXTENSION_PROTOTYPES[name][0]
        assert getattr(lib, name).argtypes == ctypes_args and _EXTENSION_PROTOTYPES[name][1] is C.c_int
        assert len(args) == len(ctypes_args), f"{name}: {len(args)} arguments in the header, {len(ctypes_args)} in _EXTENSION_PROTOTYPES"
        for i, (arg, ct) in enumerate(zip(args, ctypes_args)):
            words = re.sub(r"\bconst\b", " ", arg).split()
            if "*" in arg or "[" in arg or re.fullmatch(r"wx_\w*handle", words[0]):
                assert ct in (C.c_void_p, C.c_char_p) or issubclass(ct, C._Pointer), f"{name} argument {i} `{arg}` is a pointer"
            else:
                assert words[0] in _SCALARS and ct in _SCALARS[words[0]], f"{name} argument {i} `{arg}`: _EXTENSION_PROTOTYPES has {ct.__name__}"


def test_null_handles(lib):
    """Every function but the create with None for every pointer and 0 for every scalar: destroying nothing is WX_OK, the rest
    WX_ERR_INVALID with a reason, never a crash."""
    from wxengine.native import _EXTENSION_PROTOTYPES
    assert lib.wx_sht_destroy(None) == 0
    for name in sorted(NAMES - {"wx_sht_create", "wx_sht_destroy"}):
        args = [None if (ct in (C.c_void_p, C.c_char_p) or issubclass(ct, C._Pointer)) else 0 for ct in _EXTENSION_PROTOTYPES[name][0]]
        assert getattr(lib, name)(*args) == WX_ERR_INVALID, name
        why = lib.wx_last_error()
        assert (b"null sht handle" in why and name.encode() in why) if name != "wx_sht_table" else b"wx_sht_table: null argument" in why


def test_create_refusals_come_before_the_device(lib):
    from wxengine.sht import grid_nodes
    theta, w = grid_nodes(9, "equiangular")
    h = C.c_void_p()

    def create(nlat=9, nlon=16, lmax=9, mmax=9, theta=theta, w=w, norm=b"ortho", out=C.byref(h)):
        return lib.wx_sht_create(nlat, nlon, lmax, mmax, f64(theta), f64(w), 1, norm, 0, out)
    bad_theta, desc, nan_w, beyond = theta.copy(), theta.copy(), w.copy(), theta.copy()
    bad_theta[4] = bad_theta[3]
    desc[:] = theta[::-1]
    nan_w[2] = np.nan
    beyond[-1] = 3.2
    for kw, why in ((dict(nlat=1), b"nlat and nlon must be >= 2"), (dict(nlon=1), b"nlat and nlon must be >= 2"),
                    (dict(nlon=4098), b"nlon must be <= 4096 (the twiddle table lies in LDS)"), (dict(lmax=0, mmax=1), b"lmax must be in 1 .. 32768"),
                    (dict(mmax=0), b"mmax must be in 1 .. min(lmax, nlon / 2 + 1) = 9, got 0"), (dict(mmax=10, lmax=12), b"mmax must be in 1 .. min(lmax, nlon / 2 + 1) = 9, got 10"),
                    (dict(lmax=4, mmax=5), b"mmax must be in 1 .. min(lmax, nlon / 2 + 1) = 4, got 5"),
                    (dict(norm=b"backward"), b'norm must be "ortho" (the meaning of the library\'s other norms cannot be pinned here), got "backward"'),
                    (dict(norm=b"schmidt"), b'norm must be "ortho"'), (dict(norm=None), b'norm must be "ortho"'),
                    (dict(theta=bad_theta), b"the colatitudes must ascend strictly (north first), row 4 does not"),
                    (dict(theta=desc), b"the colatitudes must ascend strictly"), (dict(theta=beyond), b"a colatitude must lie in [0, pi], row 8 does not"),
                    (dict(w=nan_w), b"a quadrature weight must be finite, row 2 is not"),
                    (dict(theta=None), b"wx_sht_create: null argument"), (dict(w=None), b"wx_sht_create: null argument"), (dict(out=None), b"wx_sht_create: null argument")):
        assert create(**kw) == WX_ERR_INVALID and why in lib.wx_last_error(), (kw, lib.wx_last_error())
    import torch
    if not torch.cuda.is_available():                      # an accepted grid gets as far as the device
        assert create() != 0 and b"ortho" not in lib.wx_last_error()


def table(lib, nlat, lmax, mmax, theta, w, csphase, t, m, folds=False):
    out = np.full((lmax - m, nlat), np.nan)
    f = C.c_int(-1)
    st = lib.wx_sht_table(nlat, lmax, mmax, f64(theta), f64(w), csphase, t, m, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(f) if folds else None)
    assert st == 0, lib.wx_last_error()
    return (out, f.value) if folds else out


def test_table_refusals(lib):
    theta = np.linspace(0.1, 3.0, 8)
    out = np.zeros((9, 8))
    po = out.ctypes.data_as(C.POINTER(C.c_double))
    for args, why in (((0, 9, 9, f64(theta), None, 1, 0, 0, po, None), b"nlat must be in 1 .. 32768"), ((8, 0, 1, f64(theta), None, 1, 0, 0, po, None), b"lmax must be in"),
                      ((8, 9, 10, f64(theta), None, 1, 0, 0, po, None), b"mmax must be in 1 .. lmax"), ((8, 9, 9, f64(theta), None, 1, 3, 0, po, None), b"table must be 0 (Pbar)"),
                      ((8, 9, 9, f64(theta), None, 1, 0, 9, po, None), b"m must be in 0 .. mmax - 1"), ((8, 9, 9, f64(theta), None, 1, 0, -1, po, None), b"m must be in"),
                      ((8, 9, 9, f64(theta * 2), None, 1, 0, 0, po, None), b"a colatitude must lie in [0, pi]"),
                      ((8, 9, 9, f64(theta), None, 1, 0, 0, po, C.byref(C.c_int())), b"null argument"), ((8, 9, 9, f64(theta), None, 1, 0, 0, None, None), b"null argument")):
        assert lib.wx_sht_table(*args) == WX_ERR_INVALID and why in lib.wx_last_error(), lib.wx_last_error()


@pytest.mark.parametrize("grid", ["equiangular", "legendre-gauss"])
@pytest.mark.parametrize("nlat", [8, 9, 16, 33, 37, 64, 181, 721])
def test_tables_against_the_oracle(lib, grid, nlat):
    from wxengine.sht import grid_nodes
    theta, w = grid_nodes(nlat, grid)
    lmax = nlat + 1
    orders = range(lmax) if nlat <= 64 else (0, 1, 2, nlat // 2 - 1, nlat // 2, nlat - 1, nlat)
    worst = {}
    for ti, name in enumerate(O.TABLES):
        e_lib = e_orc = 0.0
        for m in orders:
            got = table(lib, nlat, lmax, lmax, theta, w, 1, ti, m)
            ref = O.table_order(name, m, lmax, theta, True, np.longdouble)[m:]
            orc = O.table_order(name, m, lmax, theta, True)[m:]
            assert np.isfinite(got).all() and got.shape == ref.shape
            e_lib, e_orc = max(e_lib, float(np.abs(got - ref).max())), max(e_orc, float(np.abs(orc - ref).max()))
            if name != "P":
                assert m > 0 or lmax < 2 or (got[0] == 0).all()                      # row l = 0 is zero
        print(grid, nlat, name, "E_tab", e_lib, "oracle", e_orc)
        assert e_lib <= 2 * e_orc
        worst[name] = e_lib
    if (grid, nlat) in SC.E_TAB:
        assert max(worst.values()) <= E_TAB_MARGIN * SC.E_TAB[(grid, nlat)]
    top = table(lib, nlat, lmax, lmax, theta, w, 1, 0, 0)          # |Pbar_l^m| <= sqrt((2l + 1) / (4 pi)), met at the poles by m = 0
    assert np.abs(top).max() <= np.sqrt((2 * lmax + 1) / (4 * np.pi))
    # csphase off: the sign of the odd orders, exactly
    for m in (0, 1, 2, 3):
        for ti in range(3):
            on, off = table(lib, nlat, lmax, lmax, theta, w, 1, ti, m), table(lib, nlat, lmax, lmax, theta, w, 0, ti, m)
            assert np.array_equal(on, -off if m % 2 else off)


def test_tables_against_scipy_fixture(lib):
    """tests/golden/sht_tables.npz holds scipy.special.sph_harm_y and its gradients at the oracle's nodes (nlat 8 and 9, both grids)."""
    g = np.load(os.path.join(SC.GOLD, "sht_tables.npz"))
    for grid in ("equiangular", "legendre-gauss"):
        for nlat in (8, 9):
            theta, _ = O.nodes(nlat, grid)
            lmax = nlat + 1
            for m in range(lmax):
                P, dP, Q = (table(lib, nlat, lmax, lmax, theta, None, 1, ti, m) for ti in range(3))
                key = f"{grid}_{nlat}_"
                # scipy's own distance from the fp64 oracle is 2e-15 at these sizes (tests/test_sht_oracle.py): four times that
                assert np.abs(P - g[key + "P"][m, m:]).max() <= 8e-15 and np.abs(dP - g[key + "dP"][m, m:]).max() <= 8e-15
                assert np.abs(Q * np.sin(theta) - g[key + "Qs"][m, m:]).max() <= 8e-15


def test_fold_detection(lib):
    from wxengine.sht import grid_nodes
    for grid in ("equiangular", "legendre-gauss"):
        for nlat in (2, 8, 9, 33, 64, 181, 721):
            theta, w = grid_nodes(nlat, grid)
            assert table(lib, nlat, 3, 3, theta, w, 1, 0, 0, folds=True)[1] == 1
            moved, heavier = theta.copy(), w.copy()
            moved[nlat - 1 - nlat // 3] -= 2.0 ** -50         # a southern row by two ulp of pi: the sum with its mirror is no longer pi
            heavier[-1] = np.nextafter(heavier[-1], 9.0)
            assert table(lib, nlat, 3, 3, moved, w, 1, 0, 0, folds=True)[1] == 0 and table(lib, nlat, 3, 3, theta, heavier, 1, 0, 0, folds=True)[1] == 0
    theta, w = O.nodes(33, "legendre-gauss")                  # nodes that are symmetric only to rounding do not fold
    assert not np.array_equal(theta + theta[::-1], np.full(33, np.pi)) and table(lib, 33, 3, 3, theta, w, 1, 0, 0, folds=True)[1] == 0
