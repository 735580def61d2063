"""The host side of the zonal spectra without a GPU: every refusal with its message (the Python mirror's and, where the library is
built, the C ABI's own, which come before any device is asked for), key order and flattening of the named-tensor form, the
bookkeeping of PendingSpectra with the device call replaced, and construction without a GPU."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import spectrum_cases as SC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"wx_spectrum_create", "wx_spectrum_destroy", "wx_spectrum_apply"}


@pytest.fixture()
def WS(monkeypatch):
    import wxengine.spectrum as WS
    monkeypatch.setattr(WS.ZonalSpectrum, "_open", lambda self, device: None)
    return WS


def test_exported_lazily_and_raises_without_a_gpu():
    import torch
    import wxengine
    from wxengine.engine import WXEngineError
    assert wxengine.ZonalSpectrum is wxengine.spectrum.ZonalSpectrum and wxengine.PendingSpectra is wxengine.spectrum.PendingSpectra
    assert wxengine.SpectrumResult is wxengine.spectrum.SpectrumResult
    if not torch.cuda.is_available():
        with pytest.raises(WXEngineError, match="no CPU fallback"):
            wxengine.ZonalSpectrum(5, 12)
    with pytest.raises(ValueError, match="must be integers >= 2"):      # the argument's own faults come first
        wxengine.ZonalSpectrum(1, 12)


def test_constructor_refusals(WS):
    for H, W in ((1, 12), (5, 1), (0, 0), (5.5, 12)):
        with pytest.raises(ValueError, match="H and W must be integers >= 2"):
            WS.ZonalSpectrum(H, W)
    with pytest.raises(ValueError, match="W must be <= 4096"):
        WS.ZonalSpectrum(5, 4097)
    assert WS.ZonalSpectrum(2, 4096).Wh == 2049 and WS.ZonalSpectrum(5, 45).Wh == 23
    for bad in (np.inf, np.nan, -0.5):
        w = np.ones(5, dtype=np.float32)
        w[3] = bad
        with pytest.raises(ValueError, match="finite and >= 0"):
            WS.ZonalSpectrum(5, 12, lat_weights=w)
    with pytest.raises(ValueError, match="sum to zero"):
        WS.ZonalSpectrum(5, 12, lat_weights=np.zeros(5))
    with pytest.raises(ValueError, match="4 latitude weights but the grid has 5 rows"):
        WS.ZonalSpectrum(5, 12, lat_weights=np.ones(4))
    with pytest.raises(ValueError, match="not both"):
        WS.ZonalSpectrum(5, 12, latitude=np.zeros(5), lat_weights=np.ones(5))
    s = WS.ZonalSpectrum(5, 12, latitude=SC.latitudes(5))
    assert s.lat_weights.dtype == np.float32 and np.array_equal(s.lat_weights, SC.weights("s0"))
    assert WS.ZonalSpectrum(5, 12).lat_weights is None


def test_wavenum_refusals(WS):
    assert WS.check_wavenum(0, 12) == 0 and WS.check_wavenum(6, 12) == 6 and WS.check_wavenum(22, 45) == 22
    for bad, W in ((-1, 12), (7, 12), (23, 45), (2.5, 12), (True, 12)):
        with pytest.raises(ValueError, match=r"wavenum_init must be an integer in 0 \.\. W // 2"):
            WS.check_wavenum(bad, W)
    s = WS.ZonalSpectrum(5, 12)
    with pytest.raises(ValueError, match="wavenum_init"):      # the default of 20 is beyond a 12-point row: told before any tensor is looked at
        s.submit(None, None)


def test_calls_refuse_what_is_not_a_device_tensor(WS):
    import torch
    from wxengine.engine import WXEngineError
    s = WS.ZonalSpectrum(5, 12)
    s.device = torch.device("cuda", 0)
    for bad in (np.zeros((2, 5, 12), dtype=np.float32), torch.zeros((2, 5, 12)), torch.zeros(12)):
        with pytest.raises(WXEngineError, match="float32 CUDA tensor"):
            s.psd(bad)
        with pytest.raises(WXEngineError, match="float32 CUDA tensor"):
            s.compare(bad, bad, 2)
    with pytest.raises(TypeError, match="both be tensors or both be named"):
        s.submit({"t": torch.zeros((1, 1, 1, 5, 12))}, torch.zeros((1, 1, 1, 5, 12)), 2)


def test_named_tensor_keys_and_flattening(WS):
    a, b, c = object(), object(), object()
    flat = WS.flatten_named({"era5": {"v": a, "t": b}, "sst": c}, "pred")
    assert list(flat) == ["sst", "t", "v"] and flat["v"] is a and flat["sst"] is c
    pairs = WS.pair_named({"era5": {"v": a, "t": b, "extra": c}}, {"t": c, "v": b})
    assert list(pairs) == ["t", "v"] and pairs["t"] == (b, c) and pairs["v"] == (a, b)      # the target's variables, sorted
    with pytest.raises(KeyError, match="variable 'q' missing from the prediction"):
        WS.pair_named({"t": a}, {"q": b})
    with pytest.raises(ValueError, match="'target' is empty"):
        WS.pair_named({"t": a}, {"era5": {}})
    offsets, total = WS.table_layout({"t": 3, "v": 2}, 7)
    assert offsets == {"t": 0, "v": 3 * 30} and total == 5 * 30


class FakeEvent:
    def __init__(self):
        self.waits, self.ready = 0, False

    def query(self):
        return self.ready

    def synchronize(self):
        self.waits += 1


def test_pending_spectra_bookkeeping(WS):
    Wh, leads = 7, {"t": (1, 3, 1), "v": (1, 2, 1)}
    offsets, total = WS.table_layout({"t": 3, "v": 2}, Wh)
    table = np.arange(total, dtype=np.float64) + 1.0
    ev = FakeEvent()
    pend = WS.PendingSpectra(types.SimpleNamespace(numpy=lambda: table), ev, leads, Wh, 2, True, ("inputs",))
    assert not pend.done() and ev.waits == 0 and pend._keep is not None
    res = pend.result()
    assert ev.waits == 1 and pend.done() and pend._keep is None and pend.result() is res and ev.waits == 1
    assert list(res) == ["t", "v"]
    t, v = res["t"], res["v"]
    assert t.mean_psd_pred.shape == (1, 3, 1, Wh) and t.psd_score.shape == (1, 3, 1) and v.mean_amp_target.shape == (1, 2, 1, Wh)
    assert np.array_equal(t.mean_psd_pred.reshape(-1), table[:21]) and np.array_equal(t.mean_psd_target.reshape(-1), table[21:42])
    assert np.array_equal(t.mean_amp_pred.reshape(-1), table[42:63]) and np.array_equal(t.mean_amp_target.reshape(-1), table[63:84])
    assert np.array_equal(t.psd_score.reshape(-1), table[84:90:2]) and np.array_equal(t.amp_score.reshape(-1), table[85:90:2])
    o = offsets["v"]
    assert np.array_equal(v.mean_psd_pred.reshape(-1), table[o:o + 14]) and np.array_equal(v.amp_score.reshape(-1), table[o + 57:o + 60:2])
    assert t.psd_loss == table[84:90:2].mean() and t.spectral_loss == table[85:90:2].mean() and t.wavenum_init == 2
    assert np.array_equal(t.ratio, t.mean_psd_pred / t.mean_psd_target)
    table[:] = 0                                            # the result owns its numbers: the pinned buffer may be reused
    assert t.mean_psd_pred[0, 0, 0, 0] == 1.0
    # a tensor pair: one unnamed field, the result is the SpectrumResult itself
    one = WS.PendingSpectra(types.SimpleNamespace(numpy=lambda: np.ones(2 * 30)), FakeEvent(), {None: (2,)}, Wh, 0, False, None)
    assert isinstance(one.result(), WS.SpectrumResult) and one.result().ratio.shape == (2, Wh) and (one.result().ratio == 1).all()


def test_abi_symbols_and_the_refusals_that_need_no_device():
    from wxengine import engine as E
    assert NAMES <= set(E.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "wxengine.h")).read()
    assert all(f"int {n}(" in hdr for n in NAMES)
    if not os.path.exists(E.LIB_PATH):
        return
    lib = E.load_library()
    assert all(hasattr(lib, n) for n in NAMES)
    h = C.c_void_p()
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    w = np.ones(5, dtype=np.float32)
    cases = [((1, 12, None), b"H and W must be >= 2"), ((5, 1, None), b"H and W must be >= 2"), ((5, 4097, None), b"W must be <= 4096"),
             ((5, 12, f(np.where(np.arange(5) == 3, np.inf, w))), b"finite and >= 0, row 3"),
             ((5, 12, f(np.where(np.arange(5) == 2, np.nan, w))), b"finite and >= 0, row 2"),
             ((5, 12, f(np.where(np.arange(5) == 1, -1.0, w))), b"finite and >= 0, row 1"), ((5, 12, f(0 * w)), b"sum to zero")]
    for (H, W, lw), why in cases:
        assert lib.wx_spectrum_create(H, W, lw, 0, C.byref(h)) == -1 and why in lib.wx_last_error() and not h.value, why
    assert lib.wx_spectrum_create(5, 12, None, 0, None) == -1 and b"null argument" in lib.wx_last_error()
    assert lib.wx_spectrum_apply(None, 1, None, 60, None, 60, 0, None, None, None, None, None, None, None, None) == -1
    assert b"null spectrum handle" in lib.wx_last_error()
    assert lib.wx_spectrum_destroy(None) == 0
