"""Host side of the wind artifact filter (wxengine/wind_filter.py), no GPU needed: the kernel sizes and 1-D weights the device gets
equal the reference's expressions, the constructor refuses what the kernels cannot run with the reason, and without a GPU the block
raises instead of falling back."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from wind_cases import CAM, DEFAULTS, KEYS  # noqa: E402

from wxengine.engine import WXEngineError  # noqa: E402
from wxengine.wind_filter import WindArtifactFilter, filter_kernels, kernel_sizes  # noqa: E402

SIG = ("smooth_sigma", "smooth_sigma_zonal", "smooth_sigma_meridional", "falloff_sigma")


def reference_expression(sigma, size):
    """wind_filter.py:54-56 / :74-78 as stated in the issue: arange - size // 2, exp(-0.5 (x / sigma)^2), divided by its sum, float32."""
    x = torch.arange(size, dtype=torch.float32) - size // 2
    g = torch.exp(-0.5 * (x / sigma) ** 2)
    return (g / g.sum()).numpy()


@pytest.mark.parametrize("args,sizes,sigmas", [
    (DEFAULTS, dict(smooth_lat=7, smooth_lon=7, falloff_lat=17, falloff_lon=33), (1.0, 1.0, 4.0, 8.0)),
    (CAM, dict(smooth_lat=5, smooth_lon=13, falloff_lat=17, falloff_lon=33), (0.5, 2.0, 4.0, 8.0)),
    (dict(DEFAULTS, falloff_sigma=8.0), dict(smooth_lat=7, smooth_lon=7, falloff_lat=33, falloff_lon=65), (1.0, 1.0, 8.0, 16.0)),
    (dict(DEFAULTS, falloff_sigma=0.5, smooth_sigma=0.4), dict(smooth_lat=3, smooth_lon=3, falloff_lat=3, falloff_lon=5), (0.4, 0.4, 0.5, 1.0)),
], ids=["defaults", "camulator", "falloff8", "small"])
def test_kernel_sizes_and_weights_equal_the_reference_expressions(args, sizes, sigmas):
    kw = {k: args[k] for k in SIG}
    assert kernel_sizes(**kw) == sizes
    k = filter_kernels(**kw)
    for name, sigma in zip(("smooth_lat", "smooth_lon", "falloff_lat", "falloff_lon"), sigmas):
        assert k[name].dtype == np.float32 and k[name].shape == (sizes[name],)
        assert np.array_equal(k[name], reference_expression(sigma, sizes[name])), name     # the longitude falloff has sigma DOUBLED
        assert abs(float(k[name].sum()) - 1.0) < 1e-6 and np.array_equal(k[name], k[name][::-1])


@pytest.mark.reference
@pytest.mark.parametrize("args", [DEFAULTS, CAM], ids=["defaults", "camulator"])
def test_weights_multiply_out_to_the_live_reference_kernels(args):
    import oracle_stub
    oracle_stub.install()
    import credit.postblock.wind_filter as RW
    z = torch.zeros(1, 4, 4)
    _, g2d = RW._compute_blend_mask(z, z, args["speed_threshold"], args["dilation_zonal"], args["dilation_meridional"], args["falloff_sigma"],
                                    args["smooth_sigma"], args["smooth_sigma_zonal"], args["smooth_sigma_meridional"])
    k = filter_kernels(**{s: args[s] for s in SIG})
    assert np.array_equal(np.outer(k["smooth_lat"], k["smooth_lon"]), g2d[0, 0].numpy())


U, V = KEYS["U"], KEYS["V"]


@pytest.mark.parametrize("kw,why", [
    (dict(dilation_zonal=12), "dilation_zonal = 12 is even"),
    (dict(dilation_meridional=4), "dilation_meridional = 4 is even"),
    (dict(dilation_zonal=0), "dilation_zonal = 0 must be >= 1"),
    (dict(dilation_zonal=67), "dilation_zonal = 67 exceeds the supported 65"),
    (dict(dilation_meridional=35), "dilation_meridional = 35 exceeds the supported 33"),
    (dict(smooth_sigma=0.0), "smooth_sigma = 0.0 must be a positive number"),
    (dict(smooth_sigma_zonal=-1.0), "smooth_sigma_zonal = -1.0 must be a positive number"),
    (dict(smooth_sigma_meridional=float("nan")), "smooth_sigma_meridional = nan must be a positive number"),
    (dict(falloff_sigma=0), "falloff_sigma = 0 must be a positive number"),
    (dict(falloff_sigma=8.5), "falloff lat kernel has 35 points, the device kernels take at most 33"),
    (dict(smooth_sigma=6.0), "smooth lat kernel has 37 points, the device kernels take at most 33"),
    (dict(smooth_sigma_zonal=11.0), "smooth lon kernel has 67 points, the device kernels take at most 65"),
    (dict(target_vars=[]), "target_vars is empty"),
    (dict(mask_level=-1), "mask_level -1 is negative"),
    (dict(target_levels=[3, -2]), "a target level is negative"),
    (dict(speed_threshold=float("inf")), "speed_threshold must be finite"),
])
def test_constructor_rejections_carry_their_reason(kw, why):
    args = dict(u_var=U, v_var=V, target_vars=[U, V])
    args.update(kw)
    with pytest.raises(ValueError, match=why):
        WindArtifactFilter(**args)


def test_the_largest_supported_kernels_pass_the_argument_checks():
    """falloff_sigma 8 (33 x 65), dilation 33 x 65, smoothing 33 x 65: past every ValueError -- to the device error where there is no GPU."""
    args = dict(u_var=U, v_var=V, target_vars=[U, V], falloff_sigma=8.0, dilation_zonal=65, dilation_meridional=33,
                smooth_sigma_meridional=5.3, smooth_sigma_zonal=10.6)
    if torch.cuda.is_available():
        WindArtifactFilter(**args)
    else:
        with pytest.raises(WXEngineError, match="no GPU visible"):
            WindArtifactFilter(**args)


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_no_gpu_raises_instead_of_falling_back():
    with pytest.raises(WXEngineError, match="no CPU fallback"):
        WindArtifactFilter(U, V, [U, V])
    import wxengine
    assert wxengine.WindArtifactFilter is WindArtifactFilter
