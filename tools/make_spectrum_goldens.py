"""Fixtures of the zonal spectra from the reference's own classes (credit/losses/gen_1/power.py::PSDLoss, spectral.py::SpectralLoss2D);
needs the reference tree.

    python tools/make_spectrum_goldens.py

tests/golden/spectrum_<case>.npz   per case of tests/spectrum_cases.py: `key`, `shape`, `k_init` (the fields are generated from the key,
                                   never stored); `psd32`, PSDLoss.get_psd of the float32 `pred`; `psd64`, the same method on the field
                                   cast to float64; `E_ref` = max|psd32 - psd64|; `loss32` [2], PSDLoss(k_init)(target, pred, w) and
                                   SpectralLoss2D(k_init)(pred, target, w) as the classes run (float32); `loss64` [2] and `scores64`
                                   [P, 2], the same formulas in float64 (tests/spectrum_oracle.py: the classes cast their input to
                                   float32 themselves, so their forward cannot be run in float64).
The generator refuses a case whose smallest PSD bin is within ten times the 1e-8 inside the logarithm (the scores would then measure
that constant, not the spectra), and one whose restatement does not reproduce get_psd in float64."""
import os
import sys

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
    import credit.losses.gen_1.power as RP
    import credit.losses.gen_1.spectral as RS
    return RP, RS


def reference_case(RP, RS, pred, target, w, k_init):
    """-> (psd32, psd64, loss32): the live classes on float32 [P, H, W] fields, weights [H]."""
    import torch
    cpu = torch.device("cpu")
    p32, t32 = torch.from_numpy(pred), torch.from_numpy(target)
    wt = torch.from_numpy(w).reshape(1, -1, 1)
    psd_loss = RP.PSDLoss(wavenum_init=k_init)
    psd32 = psd_loss.get_psd(p32, cpu, torch.float32)
    psd64 = psd_loss.get_psd(p32.double(), cpu, torch.float64)
    loss32 = torch.stack([psd_loss(t32, p32, wt), RS.SpectralLoss2D(wavenum_init=k_init)(p32, t32, wt)])
    assert psd32.dtype == torch.float32 and psd64.dtype == torch.float64 and loss32.dtype == torch.float32
    return psd32.numpy(), psd64.numpy(), loss32.numpy()


def main():
    import spectrum_oracle as SO
    from spectrum_cases import SPECTRUM_CASES, fields, key, weights
    RP, RS = reference_modules()
    for name, c in SPECTRUM_CASES.items():
        pred, target = fields(name)
        w = weights(name)
        psd32, psd64, loss32 = reference_case(RP, RS, pred, target, w, c["k_init"])
        e_ref = float(np.abs(psd32.astype(np.float64) - psd64).max())
        mine = SO.psd(pred)
        assert np.abs(mine - psd64).max() <= 1e-12 * np.abs(psd64).max(), f"{name}: the restatement is not get_psd in float64"
        smallest = min(float(psd64.min()), float(SO.psd(target).min()))
        assert smallest > 10 * SO.LOG_EPS, f"{name}: the smallest PSD bin {smallest:.3e} is near the 1e-8 inside the logarithm: change the key"
        scores64 = SO.scores(pred, target, c["k_init"], w)
        loss64 = SO.losses(pred, target, c["k_init"], w)
        rel = np.abs(loss32.astype(np.float64) - loss64) / np.abs(loss64)
        out = dict(key=np.str_(key(name)), shape=np.array(c["shape"], dtype=np.int64), k_init=np.int64(c["k_init"]), psd32=psd32, psd64=psd64,
                   E_ref=np.float64(e_ref), loss32=loss32, loss64=loss64, scores64=scores64)
        path = os.path.join(GOLD, f"spectrum_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"[golden] spectrum {name}: shape {c['shape']}, PSD {psd64.min():.3e} .. {psd64.max():.3e}, E_ref {e_ref:.3e}, "
              f"losses {loss64[0]:.6e} {loss64[1]:.6e}, float32 relative errors {rel[0]:.2e} {rel[1]:.2e}, file {os.path.getsize(path) // 1024} KB")


if __name__ == "__main__":
    main()
