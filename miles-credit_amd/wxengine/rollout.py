"""The autoregressive hot loop of credit/applications/rollout_to_netcdf.py:274-310 on the engine.

    for step in 1..n: y = model(x) [+tracer fixer]; y_phys = y*std+mean; x = update_x(x, frc_t, y)

All tensors stay in HBM: forcing for every step is pre-staged on the device (the `tisr` plane of a step is made there from the
step's valid time alone: `wxengine.tisr.TISRForcing.compute_into(t, frc, channel=k)`), y_phys is written into a
caller-provided ring so the host can drain it asynchronously (the reference does `.cpu().numpy()` every
step, rollout_to_netcdf.py:292), and the next input is assembled by the engine's tail kernel.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from .engine import WXEngine


def channel_layout(cfg, n_static: int, n_dyn: int):
    """Single-source layout (credit/datasets/gen_2/channel_utils.py:161-250): x = [prog | static | dyn]."""
    n_prog = cfg.channels * cfg.levels + cfg.surface_channels
    if n_prog + n_static + n_dyn != cfg.base_input_channels:
        raise ValueError("n_prog + n_static + n_dyn must equal the model's input channels")
    return n_prog, n_static, n_dyn


_INPUT_ORDER = ("prognostic", "static", "dynamic_forcing")   # concat rank of the input tensor (channel_utils.py:88-93)
_OUTPUT_ORDER = ("prognostic", "diagnostic")                  # one source's block of the prediction tensor


def _source_widths(conf):
    """[(source name, {field type: channel count})] from `conf["data"]["source"]`: 3-D variables count once per level (the
    source's own level list, else `model.levels`), 2-D variables once."""
    data = conf["data"]
    default_levels = int((conf.get("model") or {}).get("levels") or 0)
    table = []
    for name, src in data["source"].items():
        src = src or {}
        if src.get("history_len", data.get("history_len", 1)) != 1:
            raise ValueError(f"build_channel_layout: source '{name}' has history_len != 1; the flat rollout cannot shift a history window")
        n_levels = len(src["levels"]) if src.get("levels") else default_levels
        widths = {}
        for field_type, grp in (src.get("variables") or {}).items():
            grp = grp or {}
            n3, n2 = len(grp.get("vars_3D") or []), len(grp.get("vars_2D") or [])
            if n3 and not n_levels:
                raise ValueError(f"build_channel_layout: source '{name}' defines 3D variables but no level count is set")
            widths[field_type] = n3 * n_levels + n2
        table.append((name, widths))
    return table


def build_channel_layout(conf):
    """The channel bookkeeping of credit/datasets/gen_2/channel_utils.py:161-250 for any number of data sources.

    Returns (groups, n_pred): groups = [(field_type, x_start, src_start or None, count), ...] in input-channel order, one per
    (source, field_type) run -- with several sources a field type's channels are contiguous only within a source -- ready for
    WXEngine.set_layout_groups; n_pred = number of prognostic channels.  Three tensors are described at once: the input x
    (per source: prognostic | static | dynamic_forcing), the prediction y (per source: prognostic | diagnostic) and the forcing
    tensor (every source's dynamic-forcing channels, source-major); a group's src_start is its offset in y (prognostic) or in
    the forcing tensor (dynamic_forcing).  Raises ValueError like the reference (history_len != 1, 3-D variables without a
    level count)."""
    table = _source_widths(conf)
    # exclusive prefix sums over the sources: where each source's block starts in y and in the forcing tensor
    y_start, frc_start, y_cur, frc_cur = {}, {}, 0, 0
    for name, w in table:
        y_start[name], frc_start[name] = y_cur, frc_cur
        y_cur += sum(w.get(ft, 0) for ft in _OUTPUT_ORDER)
        frc_cur += w.get("dynamic_forcing", 0)
    source_offset = {"prognostic": y_start, "dynamic_forcing": frc_start}
    groups, x_cur = [], 0
    for name, w in table:
        for ft in _INPUT_ORDER:
            n = w.get(ft, 0)
            if n:
                groups.append((ft, x_cur, source_offset[ft][name] if ft in source_offset else None, n))
                x_cur += n
    return groups, sum(n for ft, _, _, n in groups if ft == "prognostic")


def rollout(engine: WXEngine, x0: torch.Tensor, forcings: Sequence[Optional[torch.Tensor]],
            keep_phys: bool = True, keep_y: bool = False):
    """Run len(forcings) forecast steps. forcings[t] feeds the input of step t+2 (None on the last step).

    Returns (y_list, y_phys_list); lists are empty when not kept (bench mode keeps only the last)."""
    x = x0
    ys: List[torch.Tensor] = []
    phys: List[torch.Tensor] = []
    n = len(forcings)
    for t in range(n):
        frc = forcings[t]
        last = t == n - 1
        y, yp, xn = engine.step(x, frc, want_y=keep_y, want_phys=True, want_next=not last or frc is not None)
        if keep_y:
            ys.append(y)
        if keep_phys:
            phys.append(yp)
        elif last:
            phys.append(yp)
        if xn is not None:
            x = xn
    return ys, phys


def ensemble_rollout(engine: WXEngine, x0: torch.Tensor, forcings: Sequence[Optional[torch.Tensor]], n_members: int,
                     seed: int = 0, step0: int = 0, member0: int = 0):
    """A noise-injection ensemble (CrossFormerWithNoise engine) as one wx_rollout per member: member m runs the generator's
    member coordinate member0 + m from step step0, so every member is its own reproducible trajectory.

    Returns [member][step] de-normalised outputs (engine.set_denorm must have been called)."""
    cfg = engine.cfg
    oh, ow = cfg.out_hw
    out = []
    for m in range(n_members):
        engine.set_noise(seed, member0 + m, step0)
        phys = [torch.empty((1, cfg.base_output_channels, oh, ow), dtype=torch.float32, device=x0.device) for _ in forcings]
        engine.rollout(x0, forcings, phys_out=phys)
        out.append(phys)
    return out


def perturbed_ensemble_rollout(engine: WXEngine, x0: torch.Tensor, forcings: Sequence[Optional[torch.Tensor]], n_members: int, noise, *,
                               seed: int = 0, member0: int = 0, n_perturbed: Optional[int] = None, temporal=None, deltas=None):
    """A perturbed-initial-condition ensemble of a deterministic engine (applications/rollout_metrics_noisy_ic.py:384-415): member m
    starts from x0 + noise(x0) on the first `n_perturbed` input channels (default: all of them, as the reference perturbs the whole
    assembled input) with the generator's coordinates (seed, member0 + m, step 1), and runs one wx_rollout.

    noise: a wxengine.perturb GaussianNoise or ColorNoise.  temporal: a wxengine.perturb.TemporalNoise (its own generator is used and
    `noise` is ignored): the member is run step by step, and before every later step t = 2, 3, ... the prognostic channels of the next
    input are perturbed in place with delta_t = rho * delta_{t-1} + eps_t (generator step t), the member's delta being carried on the
    device.  The prognostic channels are the first channels * levels + surface_channels of the input (the single-source layout).
    deltas: an optional list that receives, per member, the list of its carried perturbations [delta_1, delta_2, ...].

    Returns [member][step] de-normalised outputs in the shape `ensemble_rollout` returns (engine.set_denorm must have been called):
    `score_ensemble_rollout` takes them unchanged."""
    from .perturb import TemporalNoise, _Noise
    cfg = engine.cfg
    if isinstance(n_members, bool) or not isinstance(n_members, int) or n_members < 1:
        raise ValueError(f"perturbed_ensemble_rollout: n_members must be a positive integer, got {n_members!r}")
    if len(forcings) < 1:
        raise ValueError("perturbed_ensemble_rollout: forcings must have one entry per step, got none")
    if temporal is not None and not isinstance(temporal, TemporalNoise):
        raise TypeError("perturbed_ensemble_rollout: temporal must be a wxengine.perturb.TemporalNoise or None")
    if temporal is None and not isinstance(noise, _Noise):
        raise TypeError("perturbed_ensemble_rollout: noise must be a wxengine.perturb GaussianNoise or ColorNoise")
    want = (1, cfg.base_input_channels, cfg.frames, cfg.image_height, cfg.image_width)
    if not isinstance(x0, torch.Tensor) or tuple(x0.shape) != want:
        raise ValueError(f"perturbed_ensemble_rollout: x0 must be a tensor of shape {want}, got "
                         f"{tuple(x0.shape) if isinstance(x0, torch.Tensor) else type(x0).__name__}")
    n_in = cfg.base_input_channels
    n_pert = n_in if n_perturbed is None else n_perturbed
    if isinstance(n_pert, bool) or not isinstance(n_pert, int) or not 1 <= n_pert <= n_in:
        raise ValueError(f"perturbed_ensemble_rollout: n_perturbed must be 1 .. {n_in}, got {n_perturbed!r}")
    n_carry = min(n_pert, cfg.channels * cfg.levels + cfg.surface_channels)
    oh, ow = cfg.out_hw
    n = len(forcings)
    out = []
    for m in range(n_members):
        member = member0 + m
        x = x0.clone()
        head = x[:, :n_pert]
        phys = [torch.empty((1, cfg.base_output_channels, oh, ow), dtype=torch.float32, device=x0.device) for _ in forcings]
        if temporal is None:
            noise.apply(head, seed=seed, member=member, step=1, x_out=head)
            engine.rollout(x, forcings, phys_out=phys)
        else:
            _, delta = temporal(head, None, 1, seed=seed, member=member, out=head)
            delta = delta[:, :n_carry]
            carried = [delta]
            for t in range(n):
                last = t == n - 1
                _, _, xn = engine.step(x, forcings[t], want_y=False, phys_out=phys[t], want_next=not last)
                if not last:
                    prog = xn[:, :n_carry]
                    _, delta = temporal(prog, delta, t + 2, seed=seed, member=member, out=prog)
                    carried.append(delta)
                    x = xn
            if deltas is not None:
                deltas.append(carried)
        out.append(phys)
    return out


def score_ensemble_rollout(out, targets, verifier, channel_map):
    """Score the [member][step] output of `ensemble_rollout` where it lies: every step is submitted to `verifier` (an
    ensemble_metrics.EnsembleVerification) without a host sync, the members read as channel slices of their own buffers.

    channel_map: {var_key: slice, or {"slice": slice, ...} as in run_forecast's channel map} over the output channels; a variable of
    n channels is scored as n levels.  targets[step]: a [1, C, H, W] tensor in the output's channel layout, or {var_key: [1, L, 1, H, W]}.
    Returns the list of PendingEnsembleScores, one per step; call result() on them after the loop."""
    if len(out) != verifier.n_members:
        raise ValueError(f"score_ensemble_rollout: {len(out)} members for a verifier of {verifier.n_members}")
    n_steps = len(out[0])
    if any(len(m) != n_steps for m in out) or len(targets) != n_steps:
        raise ValueError("score_ensemble_rollout: every member and the targets must have one entry per step")
    slices = {k: (v["slice"] if isinstance(v, dict) else v) for k, v in channel_map.items()}
    split = lambda y: {k: y[:, sl].unsqueeze(2) for k, sl in slices.items()}      # noqa: E731  [1, L, H, W] -> [1, L, 1, H, W] views
    pending = []
    for step in range(n_steps):
        target = targets[step]
        pending.append(verifier.submit([split(member[step]) for member in out], target if isinstance(target, dict) else split(target)))
    return pending


def spectra_of_rollout(out, targets, spectrum, channel_map, wavenum_init=20):
    """The zonal spectra of the per-step output of a rollout against the truth, where the output lies: every step is submitted to
    `spectrum` (a spectrum.ZonalSpectrum) without a host sync, the variables read as channel slices of the step's buffer.

    out[step]: a [1, C, H, W] tensor; channel_map as for score_ensemble_rollout (a variable of n channels is n planes);
    targets[step]: a [1, C, H, W] tensor in the output's channel layout, or {var_key: [1, L, 1, H, W]}.
    Returns the list of PendingSpectra, one per step; call result() on them after the loop: {var_key: SpectrumResult}."""
    if len(targets) != len(out):
        raise ValueError("spectra_of_rollout: the output and the targets must have one entry per step")
    slices = {k: (v["slice"] if isinstance(v, dict) else v) for k, v in channel_map.items()}
    split = lambda y: {k: y[:, sl].unsqueeze(2) for k, sl in slices.items()}      # noqa: E731  [1, L, H, W] -> [1, L, 1, H, W] views
    pending = []
    for y, target in zip(out, targets):
        pending.append(spectrum.submit(split(y), target if isinstance(target, dict) else split(target), wavenum_init))
    return pending


def filter_rollout(out, dpf):
    """The diffusion and pole filter on the per-step physical output of a rollout, where it lies: the device counterpart of
    rollout_metrics.py's `if use_laplace_filter: y_pred = dpf.diff_lap2d_filt(y_pred.to(device).squeeze())` before scoring and saving.

    out[step]: a [1, C, H, W] tensor (C >= 70, the reference's channel layout); dpf: a pole_filter.Diffusion_and_Pole_Filter on H x W.
    Every step is filtered in place without a host sync.  Returns `out`."""
    for y in out:
        if y.dim() != 4 or y.shape[0] != 1:
            raise ValueError(f"filter_rollout: a step's output must be [1, C, H, W], got {tuple(y.shape)}")
        dpf.diff_lap2d_filt(y[0], out=y[0])
    return out
