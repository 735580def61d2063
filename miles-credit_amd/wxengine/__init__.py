"""wxengine: host side of the MI355X-native CrossFormer / WXFormer forecast-step engine.

Everything here sits above the C ABI of include/wxengine.h (libwxengine.so, built by __graft_entry__.build()):
  engine    ctypes binding: WXEngine, WXPostBlock, DevicePreblock handles
  model     the registry-facing nn.Module (reference constructor kwargs and state-dict key names)
  rollout   the autoregressive step loop;  latband: one forecast sharded over ranks by latitude
  wind_filter       the wind artifact filter post block (WindArtifactFilter, exported here)
  advect            semi-Lagrangian tracer advection, post and pre block (SemiLagrangianAdvection, SemiLagrangianAdvectionPre, exported here)
  hybrid_interp     hybrid-level interpolation, post and pre block (HybridLevelInterp, HybridLevelInterpPre, midpoint_coefficients, exported here)
  regrid            horizontal regridding pre block, an ESMF sparse weight matrix on every plane (Regridder, coalesce_weights, fold_flips, exported here)
  tisr              the TISR dynamic forcing per step from a clock, top-of-atmosphere incident solar radiation (TISRForcing, exported here)
  perturb           perturbed-initial-condition ensembles: white, colour-filtered and AR(1) noise on a member's planes (GaussianNoise, ColorNoise, TemporalNoise, hemispheric_weights, exported here)
  metrics           the gen-2 verification metrics, eight scores per variable from one reduction (CombinedMetric, PendingScores, exported here)
  ensemble_metrics  ensemble verification, CRPS / spread / ensemble-mean error from one reading pass (EnsembleVerification, PendingEnsembleScores, exported here)
  spectrum          zonal power spectra, PSD / latitude-mean spectra / spectral scores from a folded fp64 DFT (ZonalSpectrum, PendingSpectra, SpectrumResult, exported here)
  sht               spherical harmonic transforms, scalar pair / vector analysis / spectra by zonal and total wavenumber (SphericalHarmonics, RealSHT, InverseRealSHT, grid_nodes, zonal_spectrum, average_zonal_spectrum, div_rot_spectrum, average_div_rot_spectrum, exported here)
  pole_filter       the diffusion and pole filter of a forecast step, polar zonal low-pass and three explicit diffusion schemes on the transforms (Diffusion_and_Pole_Filter, exported here)
  config / synth    model geometry, name-keyed synthetic weights and inputs for tests and the benchmark
There is no CPU fallback: without the HIP library or a GPU, construction raises.
"""


def __getattr__(name):   # lazily: importing the package stays free of torch
    if name == "WindArtifactFilter":
        from .wind_filter import WindArtifactFilter
        return WindArtifactFilter
    if name in ("SemiLagrangianAdvection", "SemiLagrangianAdvectionPre"):
        from . import advect
        return getattr(advect, name)
    if name in ("HybridLevelInterp", "HybridLevelInterpPre", "midpoint_coefficients"):
        from . import hybrid_interp
        return getattr(hybrid_interp, name)
    if name in ("Regridder", "coalesce_weights", "fold_flips"):
        from . import regrid
        return getattr(regrid, name)
    if name == "TISRForcing":
        from .tisr import TISRForcing
        return TISRForcing
    if name in ("GaussianNoise", "ColorNoise", "TemporalNoise", "hemispheric_weights"):
        from . import perturb
        return getattr(perturb, name)
    if name in ("CombinedMetric", "PendingScores"):
        from . import metrics
        return getattr(metrics, name)
    if name in ("EnsembleVerification", "PendingEnsembleScores", "EnsembleScores"):
        from . import ensemble_metrics
        return getattr(ensemble_metrics, name)
    if name in ("ZonalSpectrum", "PendingSpectra", "SpectrumResult"):
        from . import spectrum
        return getattr(spectrum, name)
    if name in ("SphericalHarmonics", "RealSHT", "InverseRealSHT", "grid_nodes", "zonal_spectrum", "average_zonal_spectrum", "div_rot_spectrum",
                "average_div_rot_spectrum", "cached_transform", "clear_cache"):
        from . import sht
        return getattr(sht, name)
    if name == "Diffusion_and_Pole_Filter":
        from .pole_filter import Diffusion_and_Pole_Filter
        return Diffusion_and_Pole_Filter
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
