"""Perturbed-initial-condition ensembles on the device (credit/ensemble/gaussian.py, color.py, temporal.py, utils.hemispheric_rescale;
csrc/wx_perturb.h): the ensemble route of applications/rollout_metrics_noisy_ic.py, which works with every deterministic checkpoint.

`GaussianNoise`, `ColorNoise` and `TemporalNoise` take the reference's names, defaults and `__repr__`.  A call is one
`wx_perturb_apply` on the planes of one member's tensor: the white source is the engine's generator (Philox4x32-10 / Box-Muller,
`wxengine.noise.normals(seed, SLOT_PERTURB, member, step, n)` element for element) or, with `white=`, a tape that replays the
reference's `torch.randn` draws; the colour filter is `irfft2(rfft2(r) * S)` by dense fp64 DFTs on the matrix cores; amplitude,
per-channel scale, AR(1) term, hemispheric rescale and `x + delta` follow in the reference's float32 order of operations.  Nothing of
a member's state crosses to the host.  No CPU fallback: construction raises without the library or a GPU."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .native import HandleCache, WXEngineError, _check, _f32, _stream_ptr, require_gpu
from .noise import SLOT_PERTURB  # noqa: F401  (the generator's slot of these draws)

KIND_WHITE, KIND_COLOUR = 0, 1
MAX_SIDE = 4096              # kDftMaxN (csrc/wx_dft.h): the colour filter keeps a pass's twiddle table in LDS
MAX_ELEMENTS = 1 << 34       # kPerturbMaxElems: the generator's counter


def _scalar_amplitude(amplitude) -> float:
    """A scalar, or the length-1 sequence rollout_metrics_noisy_ic.py makes with its default `weights`."""
    if amplitude is None or isinstance(amplitude, (bool, str, bytes)):
        raise TypeError(f"amplitude must be a number or a length-1 sequence, got {type(amplitude).__name__}")
    if isinstance(amplitude, (int, float, np.integer, np.floating)):
        return float(amplitude)
    try:
        arr = np.asarray(amplitude, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise TypeError(f"amplitude must be a number or a length-1 sequence, got {type(amplitude).__name__}") from None
    if arr.size != 1:
        raise ValueError(f"amplitude must be a scalar or a length-1 sequence, got {arr.size} values: in the reference a longer array "
                         "multiplied into a 5-D tensor does not broadcast over channels; per-channel amplitudes are "
                         "TemporalNoise.perturbation_std")
    return float(arr[0])


def hemispheric_weights(latitudes, north_scale: float = 1.0, south_scale: float = 1.0) -> np.ndarray:
    """The weights of credit/ensemble/utils.py::hemispheric_rescale for float32 latitudes [H] (from +90 to -90), float32: north_scale at
    and above 20N, south_scale at and below 20S, linear in between -- by the reference's own float32 torch operations."""
    import torch
    lat = torch.from_numpy(np.ascontiguousarray(np.asarray(latitudes, dtype=np.float32).reshape(-1)))
    weights = torch.ones_like(lat)
    for i, la in enumerate(lat):
        if la >= 20:
            weights[i] = north_scale
        elif la <= -20:
            weights[i] = south_scale
        else:
            frac = (la + 20) / 40
            weights[i] = (1 - frac) * south_scale + frac * north_scale
    return weights.numpy()


def _planes(t, H: int, W: int, name: str):
    """-> (pointer, planes, plane stride in floats) of a float32 CUDA tensor [..., H, W] whose planes lie at one stride."""
    try:
        v = t.view(-1, H, W)
    except RuntimeError:
        raise WXEngineError(f"{name}: the planes of a tensor of shape {tuple(t.shape)} and strides {tuple(t.stride())} do not lie at one stride") from None
    if v.stride(2) != 1 or v.stride(1) != W:
        raise WXEngineError(f"{name}: a plane must be contiguous memory")
    return v.data_ptr(), v.shape[0], (v.stride(0) if v.shape[0] > 1 else H * W)


class _Noise:
    kind = KIND_WHITE

    def __init__(self, amplitude, device=0):
        self._amp = _scalar_amplitude(amplitude)
        self.amplitude = amplitude
        self._open(device)

    def _open(self, device) -> None:
        self.lib = require_gpu("the perturbation noise has no CPU fallback", device)
        self._handles = HandleCache(self.lib, "wx_perturb")   # by (H, W, device)

    def _weights(self, H: int, W: int):
        return None

    def _handle(self, H: int, W: int, index: int):
        return self._handles.get((H, W, index), lambda: (H, W, self.kind, _f32(self._weights(H, W)), index))

    def batch_planes(self, H: int, W: int, device: int = 0) -> int:
        """The number of planes the colour filter takes through its scratch at a time on this grid."""
        n = C.c_int(0)
        _check(self.lib.wx_perturb_batch(self._handle(H, W, device), C.byref(n)))
        return n.value

    def _check_x(self, x, name="x"):
        import torch
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2):
            raise WXEngineError(f"{name} must be a float32 CUDA tensor [..., H, W]")
        return int(x.shape[-2]), int(x.shape[-1])

    def apply(self, x, *, seed: int = 0, member: int = 0, step: int = 0, white=None, chan_scale=None, rho: float = 0.0, prev=None,
              lat_weight=None, delta_out=None, x_out=None, amplitude: Optional[float] = None):
        """One wx_perturb_apply on the planes of `x` ([..., H, W]; the generator counts elements over the flattened leading dims).
        delta_out / x_out: tensors of x's shape (planes at one stride), or None; x_out may be x.  -> (delta_out, x_out)"""
        import torch
        H, W = self._check_x(x)
        xp, P, xs = _planes(x, H, W, "x")
        ptr = [None, None, None, None]         # white, prev, delta_out, x_out
        stride = [H * W] * 4
        for i, (t, name) in enumerate(((white, "white"), (prev, "previous_perturbation"), (delta_out, "delta_out"), (x_out, "x_out"))):
            if t is None:
                continue
            self._check_x(t, name)
            if tuple(t.shape) != tuple(x.shape) or t.device != x.device:
                raise WXEngineError(f"{name} must have x's shape {tuple(x.shape)} and device, got {tuple(t.shape)} on {t.device}")
            if i == 0 and not t.is_contiguous():
                raise WXEngineError("white: the tape must be contiguous")
            ptr[i], _, stride[i] = _planes(t, H, W, name)
        for arr, n, name in ((chan_scale, P, "chan_scale"), (lat_weight, H, "lat_weight")):
            if arr is not None and np.asarray(arr).shape != (n,):
                raise WXEngineError(f"{name} must have {n} entries, got shape {np.asarray(arr).shape}")
        vp = lambda p: None if p is None else C.c_void_p(p)   # noqa: E731
        with torch.cuda.device(x.device.index):
            _check(self.lib.wx_perturb_apply(self._handle(H, W, x.device.index), P, vp(ptr[0]), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                             int(member), int(step), self._amp if amplitude is None else amplitude, _f32(chan_scale), rho,
                                             vp(ptr[1]), stride[1], _f32(lat_weight), C.c_void_p(xp), xs, vp(ptr[2]), stride[2], vp(ptr[3]),
                                             stride[3], _stream_ptr(x.device.index)))
        return delta_out, x_out

    def __call__(self, x, *, seed: int = 0, member: int = 0, step: int = 0, white=None):
        """-> the perturbation of `x`: a float32 CUDA tensor of x's shape.  white: the tape, a float32 CUDA tensor of x's shape that
        replaces the generator's draws (the reference's torch.randn)."""
        import torch
        self._check_x(x)
        delta = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        self.apply(x, seed=seed, member=member, step=step, white=white, delta_out=delta)
        return delta


class GaussianNoise(_Noise):
    """credit/ensemble/gaussian.py::GaussianNoise on the device: amplitude * r, r ~ N(0, 1) per element."""
    kind = KIND_WHITE

    def __init__(self, amplitude: float = 0.05, *, device=0):
        super().__init__(amplitude, device)

    def __repr__(self) -> str:
        return f"GaussianNoise(amplitude={self.amplitude})"


class ColorNoise(_Noise):
    """credit/ensemble/color.py::ColorNoise on the device: white noise filtered by 1 / (|f_y|^reddening + f_x^reddening) in the
    frequency domain, DC removed, the table normalised to unit RMS; times amplitude."""
    kind = KIND_COLOUR

    def __init__(self, amplitude: float = 0.05, reddening: int = 2, *, device=0):
        if isinstance(reddening, bool) or not isinstance(reddening, (int, float, np.integer, np.floating)) or not np.isfinite(reddening) or reddening < 0:
            raise ValueError(f"reddening must be a number >= 0, got {reddening!r}")
        self.reddening = reddening
        super().__init__(amplitude, device)

    def weights(self, H: int, W: int) -> np.ndarray:
        """`scaling_weights` of _create_correlated_noise, [H][W // 2 + 1] float32, by the reference's own float32 torch CPU operations
        (the reference builds the table in float32 whatever the input's dtype): bit-identical to it."""
        import torch
        if H < 1 or W < 2:
            raise ValueError(f"ColorNoise.weights: H must be >= 1 and W >= 2, got {H} x {W}")
        freq_y = torch.abs(torch.fft.fftfreq(H)).reshape(-1, 1)
        freq_x = torch.fft.rfftfreq(W)
        power_spectrum = freq_y ** self.reddening + freq_x ** self.reddening
        scaling_weights = 1.0 / torch.where(power_spectrum > 0, power_spectrum, 1.0)
        scaling_weights[..., 0, 0] = 0
        scaling_weights = scaling_weights / torch.sqrt(torch.mean(scaling_weights ** 2))
        return scaling_weights.numpy()

    def _weights(self, H: int, W: int):
        if max(H, W) > MAX_SIDE:
            raise WXEngineError(f"ColorNoise: the filter takes grids up to {MAX_SIDE} points a side, got {H} x {W}")
        return self.weights(H, W)

    def __repr__(self) -> str:
        return f"ColorNoise(amplitude={self.amplitude},reddening={self.reddening})"


class TemporalNoise:
    """credit/ensemble/temporal.py::TemporalNoise on the device: delta_t = rho * delta_{t-1} + eps_t with eps_t from `noise_generator`,
    scaled per channel by perturbation_std / amplitude, optionally rescaled by hemisphere; one wx_perturb_apply per call.

    The reference reads the latitudes from a `terrain_file` and cannot run without the rescale (its `hemispheric_rescale=False`
    path calls `False(...)`).  Here the latitude array itself is the argument and the rescale is simply optional: `latitudes=None`
    applies none."""

    def __init__(self, noise_generator, temporal_correlation: float = 0.9, perturbation_std=None, latitudes=None,
                 north_scale: float = 1.0, south_scale: float = 1.0):
        if not isinstance(noise_generator, _Noise):
            raise TypeError("noise_generator must be a wxengine.perturb GaussianNoise or ColorNoise")
        if isinstance(temporal_correlation, bool) or not isinstance(temporal_correlation, (int, float)) or not np.isfinite(temporal_correlation):
            raise ValueError(f"temporal_correlation must be a finite number, got {temporal_correlation!r}")
        self.noise_generator = noise_generator
        self.temporal_correlation = temporal_correlation
        self.perturbation_std = perturbation_std
        self._scale = None
        if perturbation_std is not None:
            import torch
            if isinstance(perturbation_std, (int, float)) and not isinstance(perturbation_std, bool):
                perturb_tensor = torch.tensor([perturbation_std], dtype=torch.float32)
            else:
                perturb_tensor = torch.as_tensor(perturbation_std).detach().cpu().to(torch.float32).reshape(-1)
                if perturb_tensor.numel() < 1:
                    raise ValueError("perturbation_std must be a number or a per-channel tensor, got an empty one")
            if not bool(torch.isfinite(perturb_tensor).all()):
                raise ValueError("perturbation_std must be finite")
            self._scale = (perturb_tensor / torch.tensor([noise_generator._amp], dtype=torch.float32)).numpy()   # temporal.py:97
        self.lat_weight = None
        if latitudes is not None:
            lat = np.asarray(latitudes, dtype=np.float32)
            if lat.ndim != 1 or lat.size < 1 or not np.isfinite(lat).all():
                raise ValueError("latitudes must be a finite 1-D array [H]")
            self.lat_weight = hemispheric_weights(lat, north_scale, south_scale)

    def _chan_scale(self, x):
        if self._scale is None:
            return None
        planes = int(np.prod(x.shape[:-2]))
        if self._scale.size == 1:
            return np.full((planes,), self._scale[0], dtype=np.float32)
        if x.dim() != 5 or x.shape[1] != self._scale.size:
            raise WXEngineError(f"perturbation_std has {self._scale.size} channels, x of shape {tuple(x.shape)} is not [B, {self._scale.size}, T, H, W]")
        return np.tile(np.repeat(self._scale, x.shape[2]), x.shape[0]).astype(np.float32)

    def __call__(self, x, previous_perturbation=None, forecast_step: int = 1, *, seed: int, member: int, white=None, out=None):
        """-> (perturbed_state, current_perturbation).  The generator's step coordinate is `forecast_step`; `out` receives the perturbed
        state (x itself: in place)."""
        import torch
        gen = self.noise_generator
        H, _ = gen._check_x(x)
        if self.lat_weight is not None and self.lat_weight.size != H:
            raise WXEngineError(f"latitudes has {self.lat_weight.size} entries, x has {H} rows")
        prev = None if forecast_step == 1 else previous_perturbation
        delta = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        state = out if out is not None else torch.empty(x.shape, dtype=torch.float32, device=x.device)
        gen.apply(x, seed=seed, member=member, step=forecast_step, white=white, chan_scale=self._chan_scale(x),
                  rho=float(self.temporal_correlation), prev=prev, lat_weight=self.lat_weight, delta_out=delta, x_out=state)
        return state, delta
