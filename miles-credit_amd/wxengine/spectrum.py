"""Zonal power spectra on the device (csrc/wx_spectrum.h): how blurred is a forecast, and from which wavenumber on does it lose energy?

The per-latitude DFT along longitude of credit/losses/gen_1/power.py::PSDLoss and spectral.py::SpectralLoss2D, as a dense fp64 DFT on
the matrix cores with the real input folded; nothing of a field crosses to the host but the latitude-mean spectra and two scores per
plane.  Wh = W // 2 + 1 wavenumbers; bin 0 counts once and every other bin twice (the Nyquist bin of an even W too: the reference's).

    spectrum = ZonalSpectrum(H, W, latitude=lat_degrees)           # or lat_weights=[H], or neither (w = 1)
    psd = spectrum.psd(x)                                          # float32 [..., H, Wh]  = PSDLoss.get_psd(x)
    mean = spectrum.mean_spectrum(x)                               # float64 [..., Wh]     = sum_h w_h psd / sum(w)
    r = spectrum.compare(pred, target, wavenum_init=20)            # SpectrumResult
    r.psd_loss, r.spectral_loss                                    # PSDLoss()(target, pred, w), SpectralLoss2D()(pred, target, w)
    r.ratio                                                        # mean_psd_pred / mean_psd_target per k: the blurring curve
    pending = spectrum.submit(pred, target)                        # in a rollout: kernels and an async copy, no sync
    ...
    r = pending.result()                                           # waits on its event

`pred` and `target` are float32 device tensors [..., H, W] (strided views are read where they lie when their planes lie at one stride)
or named tensors, {var: [B, L, T, H, W]} or {source: {var: ...}} as in CombinedMetric: the result is then {var: SpectrumResult} in
sorted key order, a variable of L levels being L planes.  With latitude weights w (the [H] of `lat_weights`, or cos_lat_weights of
`latitude`) the PSD quantities use w / sum(w) and the amplitude spectrum (sum_h w_h |X|) / H, each its reference's convention.
No CPU fallback: construction raises without a GPU."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np

from .native import NativeHandle, PendingResult, WXEngineError, _check, _f32, _stream_ptr, copy_out, require_gpu
from .native import flatten_named as _flatten_named

MAX_W = 4096            # kDftMaxN (csrc/wx_dft.h): the twiddle table lies in LDS
PARTS = ("mean_psd_pred", "mean_psd_target", "mean_amp_pred", "mean_amp_target")     # the [P][Wh] blocks of a variable's table, then [P][2]


def check_grid(H, W, lat_weights=None) -> Optional[np.ndarray]:
    """The constructor's checks, without a device: those of spectrum_check_create.  -> the weights as float32 [H], or None."""
    if int(H) != H or int(W) != W or H < 2 or W < 2:
        raise ValueError(f"ZonalSpectrum: H and W must be integers >= 2, got {H!r} x {W!r}")
    if W > MAX_W:
        raise ValueError(f"ZonalSpectrum: W must be <= {MAX_W} (the twiddle table lies in LDS), got {W}")
    if lat_weights is None:
        return None
    w = np.ascontiguousarray(np.asarray(lat_weights, dtype=np.float32).reshape(-1))
    if w.size != H:
        raise ValueError(f"ZonalSpectrum: {w.size} latitude weights but the grid has {H} rows")
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("ZonalSpectrum: a latitude weight must be finite and >= 0")
    if not float(w.astype(np.float64).sum()) > 0:
        raise ValueError("ZonalSpectrum: the latitude weights sum to zero")
    return w


def check_wavenum(wavenum_init, W) -> int:
    Wh = W // 2 + 1
    if isinstance(wavenum_init, bool) or int(wavenum_init) != wavenum_init or not 0 <= int(wavenum_init) < Wh:
        raise ValueError(f"ZonalSpectrum: wavenum_init must be an integer in 0 .. W // 2 = {Wh - 1}, got {wavenum_init!r}")
    return int(wavenum_init)


def flatten_named(state: dict, name: str) -> dict:
    """{var: tensor} of a flat or a nested {source: {var: tensor}} dict, in sorted key order."""
    flat = _flatten_named(state, name, "ZonalSpectrum")
    return {k: flat[k] for k in sorted(flat)}


def pair_named(pred: dict, target: dict) -> dict:
    """{var: (pred tensor, target tensor)} over the target's variables in sorted order; a variable missing from pred is a KeyError."""
    p, t = flatten_named(pred, "pred"), flatten_named(target, "target")
    for k in t:
        if k not in p:
            raise KeyError(f"ZonalSpectrum: variable '{k}' missing from the prediction")
    return {k: (p[k], t[k]) for k in t}


class SpectrumResult:
    """One field's comparison.  With `lead` the field's leading shape ([B, L, T] of a named tensor): psd_score and amp_score float64
    [*lead]; psd_loss and spectral_loss their means, the reference's two scalars; mean_psd_pred / mean_psd_target / mean_amp_pred /
    mean_amp_target float64 [*lead, Wh]; ratio = mean_psd_pred / mean_psd_target."""

    def __init__(self, table: np.ndarray, scores: np.ndarray, lead, wavenum_init: int):
        Wh = table.shape[-1]
        for i, name in enumerate(PARTS):
            setattr(self, name, table[i].reshape(tuple(lead) + (Wh,)))
        self.psd_score = scores[:, 0].reshape(tuple(lead))
        self.amp_score = scores[:, 1].reshape(tuple(lead))
        self.psd_loss = float(scores[:, 0].mean())
        self.spectral_loss = float(scores[:, 1].mean())
        self.wavenum_init = wavenum_init
        with np.errstate(divide="ignore", invalid="ignore"):
            self.ratio = self.mean_psd_pred / self.mean_psd_target


def table_layout(planes: Dict[str, int], Wh: int):
    """Where each variable's results lie in the float64 table of one submit: per variable four [P][Wh] blocks (PARTS) and [P][2] scores.
    -> ({var: offset in doubles}, total doubles)"""
    offsets, at = {}, 0
    for k, P in planes.items():
        offsets[k] = at
        at += P * (4 * Wh + 2)
    return offsets, at


class PendingSpectra(PendingResult):
    """The spectra of one `submit`: the kernels and the copy of the table into a pinned buffer are enqueued, `result()` waits and is
    {var: SpectrumResult} of named tensors, the SpectrumResult of a tensor pair."""

    def __init__(self, pinned, event, leads, Wh, wavenum_init, named, keep):
        def finish(host):
            table = np.array(host, dtype=np.float64)
            planes = {k: int(np.prod(lead, dtype=np.int64)) for k, lead in leads.items()}
            offsets, _ = table_layout(planes, Wh)
            out = {}
            for k, lead in leads.items():
                P, o = planes[k], offsets[k]
                out[k] = SpectrumResult(table[o:o + 4 * P * Wh].reshape(4, P, Wh), table[o + 4 * P * Wh:o + 4 * P * Wh + 2 * P].reshape(P, 2),
                                        lead, wavenum_init)
            return out if named else out[None]
        super().__init__(pinned, event, finish, keep)


class ZonalSpectrum:
    def __init__(self, H: int, W: int, latitude=None, lat_weights=None, device=0):
        if latitude is not None and lat_weights is not None:
            raise ValueError("ZonalSpectrum: give latitude (degrees) or lat_weights, not both")
        if latitude is not None:
            from .metrics import cos_lat_weights
            lat_weights = cos_lat_weights(latitude).clamp_min(0.0).numpy()      # float32 cos(90 deg) is -4.4e-8: a pole row weighs nothing
        self.lat_weights = check_grid(H, W, lat_weights)
        self.H, self.W, self.Wh = int(H), int(W), int(W) // 2 + 1
        self._open(device)

    def _open(self, device) -> None:
        import torch
        self.lib = require_gpu("the zonal spectrum has no CPU fallback", device)
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self._h = NativeHandle(self.lib.wx_spectrum_destroy)
        _check(self.lib.wx_spectrum_create(self.H, self.W, _f32(self.lat_weights), self.device.index, self._h.out))

    # ---- the planes of a tensor ----------------------------------------------------------------------------------------------------
    def _planes(self, x, name):
        """-> (tensor that keeps the memory alive, pointer, planes, plane stride in floats, leading shape)."""
        import torch
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2):
            raise WXEngineError(f"{name} must be a float32 CUDA tensor [..., H, W]")
        if tuple(x.shape[-2:]) != (self.H, self.W) or x.device != self.device:
            raise WXEngineError(f"{name}: expected [..., {self.H}, {self.W}] on {self.device}, got {tuple(x.shape)} on {x.device}")
        lead = tuple(x.shape[:-2])
        v = None
        if x.stride(-1) == 1 and x.stride(-2) == self.W:
            try:
                v = x.view(-1, self.H, self.W)                  # the planes of a view lie at one stride, or this raises
            except RuntimeError:
                v = None
        if v is None or (v.shape[0] > 1 and v.stride(0) < self.H * self.W):      # an expanded view: planes that share memory
            v = x.contiguous().view(-1, self.H, self.W)
        if v.shape[0] < 1:
            raise WXEngineError(f"{name} has no planes: shape {tuple(x.shape)}")
        return v, v.data_ptr(), v.shape[0], (v.stride(0) if v.shape[0] > 1 else self.H * self.W), lead

    def _apply(self, P, a, a_stride, b=None, b_stride=0, k_init=0, psd_a=None, psd_b=None, mean_psd_a=None, mean_psd_b=None, mean_amp_a=None,
               mean_amp_b=None, scores=None):
        vp = lambda p: None if p is None else C.c_void_p(p)   # noqa: E731
        _check(self.lib.wx_spectrum_apply(self._h, P, vp(a), a_stride, vp(b), b_stride, k_init, vp(psd_a), vp(psd_b), vp(mean_psd_a),
                                          vp(mean_psd_b), vp(mean_amp_a), vp(mean_amp_b), vp(scores), _stream_ptr(self.device.index)))

    # ---- one field -----------------------------------------------------------------------------------------------------------------
    def psd(self, x):
        """PSDLoss.get_psd(x): float32 [..., H, Wh] on the device."""
        import torch
        keep, ptr, P, stride, lead = self._planes(x, "x")
        out = torch.empty(lead + (self.H, self.Wh), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device.index):
            self._apply(P, ptr, stride, psd_a=out.data_ptr())
        return out

    def mean_spectrum(self, x):
        """The latitude-mean PSD of x: float64 [..., Wh] on the device."""
        import torch
        keep, ptr, P, stride, lead = self._planes(x, "x")
        out = torch.empty(lead + (self.Wh,), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device.index):
            self._apply(P, ptr, stride, mean_psd_a=out.data_ptr())
        return out

    # ---- two fields ----------------------------------------------------------------------------------------------------------------
    def submit(self, pred, target, wavenum_init: int = 20) -> PendingSpectra:
        import torch
        k_init = check_wavenum(wavenum_init, self.W)
        named = isinstance(pred, dict) or isinstance(target, dict)
        if named and not (isinstance(pred, dict) and isinstance(target, dict)):
            raise TypeError("ZonalSpectrum: pred and target must both be tensors or both be named tensors")
        pairs = pair_named(pred, target) if named else {None: (pred, target)}
        Wh = self.Wh
        with torch.no_grad():
            fields = {}
            for k, (p, t) in pairs.items():
                label = "" if k is None else f"{k}: "
                a, b = self._planes(p, f"{label}pred"), self._planes(t, f"{label}target")
                if a[4] != b[4]:
                    raise WXEngineError(f"{label}pred {tuple(p.shape)} and target {tuple(t.shape)} must be one shape")
                fields[k] = (a, b)
            leads = {k: a[4] for k, (a, _) in fields.items()}
            offsets, total = table_layout({k: a[2] for k, (a, _) in fields.items()}, Wh)
            table = torch.empty((total,), dtype=torch.float64, device=self.device)
            base = table.data_ptr()
            with torch.cuda.device(self.device.index):
                for k, (a, b) in fields.items():
                    P, o = a[2], base + 8 * offsets[k]
                    block = 8 * P * Wh
                    self._apply(P, a[1], a[3], b[1], b[3], k_init, mean_psd_a=o, mean_psd_b=o + block, mean_amp_a=o + 2 * block,
                                mean_amp_b=o + 3 * block, scores=o + 4 * block)
                pinned, event = copy_out(table, self.device.index)
        return PendingSpectra(pinned, event, leads, Wh, k_init, named, (fields, table))

    def compare(self, pred, target, wavenum_init: int = 20):
        return self.submit(pred, target, wavenum_init).result()

    __call__ = compare
