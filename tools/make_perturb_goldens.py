"""Fixtures of the perturbation noise from the reference's own classes (credit/ensemble/color.py, gaussian.py, temporal.py, utils.py);
needs the reference tree.

    python tools/make_perturb_goldens.py

tests/golden/perturb_<case>.npz   per case of tests/perturb_cases.py: `key` (the tape is keyed_normal(key, shape): the draws are never
                                  stored), `shape`, and per reddening r of the case, at amplitude 1: `S_r<r>` (the reference's
                                  float32 `scaling_weights`), `ref32_r<r>` (ColorNoise on the float32 tape), `ref64_r<r>` (the
                                  reference's own code on the same tape cast to float64) and `E_ref_r<r>` = max|ref32 - ref64|.
                                  p19x37 also holds `gauss32` (GaussianNoise), `temporal_state` / `temporal_delta` (TemporalNoise on the
                                  tapes `.x`, `.prev` and the case's own) and `hemi_w` (hemispheric_rescale's weights).
The reference draws with torch.randn / torch.randn_like: both are replaced by the tape while a reference call runs.  The generator
refuses a case that leaves the device less than 2x room: E_ref must be at least twice half an ulp of the largest float32 output."""
import contextlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden")
for p in (HERE, os.path.join(ROOT, "tests"), os.path.join(ROOT, "miles-credit_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def reference_modules():
    import oracle_stub
    oracle_stub.install()
    import credit.ensemble.color as RC
    import credit.ensemble.gaussian as RG
    import credit.ensemble.temporal as RT
    import credit.ensemble.utils as RU
    return RC, RG, RT, RU


@contextlib.contextmanager
def replay(tape):
    """torch.randn(*shape) and torch.randn_like(x) return `tape` (a torch tensor) inside the block."""
    import torch
    real, real_like = torch.randn, torch.randn_like

    def randn(*shape, **_kw):
        assert tuple(shape) == tuple(tape.shape), (shape, tape.shape)
        return tape

    def randn_like(x, **_kw):
        assert x.shape == tape.shape
        return tape
    torch.randn, torch.randn_like = randn, randn_like
    try:
        yield
    finally:
        torch.randn, torch.randn_like = real, real_like


def capture_weights(RC, noise, shape):
    """The reference's `scaling_weights`: the table it multiplies into the spectrum, read from a run on a unit spectrum."""
    import torch
    H, W = shape[-2:]
    seen = {}
    real_irfft2 = torch.fft.irfft2

    def spy(filtered, **kw):
        seen["filtered"] = filtered
        return real_irfft2(filtered, **kw)
    real_rfft2 = torch.fft.rfft2
    torch.fft.irfft2, torch.fft.rfft2 = spy, lambda x, **kw: torch.ones((H, W // 2 + 1), dtype=torch.complex64)
    try:
        with replay(torch.zeros((H, W))):
            noise._create_correlated_noise((H, W), torch.device("cpu"))
    finally:
        torch.fft.irfft2, torch.fft.rfft2 = real_irfft2, real_rfft2
    return seen["filtered"].real.contiguous().numpy()


def reference_filter(RC, reddening, tape):
    """-> (S, ref32, ref64) at amplitude 1."""
    import torch
    noise = RC.ColorNoise(amplitude=1.0, reddening=reddening)
    t32 = torch.from_numpy(tape)
    with replay(t32):
        ref32 = noise(t32)
    t64 = t32.double()
    with replay(t64):
        ref64 = noise(t64)
    assert ref32.dtype == torch.float32 and ref64.dtype == torch.float64
    return capture_weights(RC, noise, tape.shape), ref32.numpy(), ref64.numpy()


def reference_temporal(RC, RT, tape, x, prev, cfg, latitudes):
    import torch
    RT.xr = types.SimpleNamespace(open_dataset=lambda _p: types.SimpleNamespace(
        load=lambda: types.SimpleNamespace(latitude=types.SimpleNamespace(values=latitudes))))
    tn = RT.TemporalNoise(RC.ColorNoise(amplitude=cfg["amplitude"], reddening=cfg["reddening"]), temporal_correlation=cfg["rho"],
                          perturbation_std=torch.tensor(cfg["std"], dtype=torch.float32), hemispheric_rescale=True, terrain_file=RT.__file__)
    t = torch.from_numpy(tape)
    with replay(t):
        state, delta = tn(torch.from_numpy(x), torch.from_numpy(prev), cfg["forecast_step"])
    assert state.dtype == torch.float32 and delta.dtype == torch.float32
    return state.numpy(), delta.numpy()


def reference_hemi(RU, cfg):
    import torch
    lat = torch.linspace(*cfg["lat"], dtype=torch.float32)
    return lat.numpy(), RU.hemispheric_rescale(torch.ones((1, 1, 1, lat.numel(), 1)), lat, cfg["north"], cfg["south"]).reshape(-1).numpy()


def main():
    import torch
    import perturb_oracle as PO
    from perturb_cases import HEMI, PERTURB_CASES, TEMPORAL, key, tape
    RC, RG, RT, RU = reference_modules()
    for name, c in PERTURB_CASES.items():
        r = tape(name)
        out = dict(key=np.str_(key(name)), shape=np.array(c["shape"], dtype=np.int64))
        for red in c["reddening"]:
            S, r32, r64 = reference_filter(RC, red, r)
            e_ref = float(np.abs(r32.astype(np.float64) - r64).max())
            half_ulp = float(np.spacing(np.float32(np.abs(r64).max()))) / 2
            e_mine = float(np.abs(PO.colour_filter(r, S) - r64).max())
            assert S.dtype == np.float32 and e_ref >= 2 * half_ulp, f"{name} r{red}: E_ref {e_ref:.3e} leaves less than 2x room over {half_ulp:.3e}: change the key"
            assert e_mine <= 1e-12 * np.abs(r64).max(), f"{name} r{red}: the restatement is {e_mine:.3e} from ref64"
            out.update({f"S_r{red}": S, f"ref32_r{red}": r32, f"ref64_r{red}": r64, f"E_ref_r{red}": np.float64(e_ref)})
            print(f"[golden] perturb {name} r{red}: shape {c['shape']}, max|y| {np.abs(r64).max():.3f}, E_ref {e_ref:.3e} "
                  f"({e_ref / half_ulp:.1f} half ulps), restatement {e_mine:.2e}")
        if name == TEMPORAL["case"]:
            t = torch.from_numpy(r)
            with replay(t):
                out["gauss32"] = RG.GaussianNoise(amplitude=TEMPORAL["amplitude"])(t).numpy()
            out["hemi_lat"], out["hemi_w"] = reference_hemi(RU, HEMI)
            out["temporal_state"], out["temporal_delta"] = reference_temporal(RC, RT, r, tape(name, ".x"), tape(name, ".prev"), TEMPORAL, out["hemi_lat"])
        path = os.path.join(GOLD, f"perturb_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"[golden] perturb {name}: file {os.path.getsize(path) // 1024} KB")


if __name__ == "__main__":
    main()
