"""The binding layer of libwxengine.so (C ABI in include/wxengine.h and its extension include/wxengine_sht.h): the ctypes prototypes
and the loader, the owner of a native handle, and what every device product needs to hand torch tensors to the library -- the GPU guard, the per-geometry handle cache, the
named-tensor test and pointer tables, and the pending result of an asynchronous call.

PyTorch is used only as the owner of device memory and streams: tensors are handed to the library as raw device pointers.  There is
NO CPU fallback: if the HIP library is missing or no GPU is visible, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# WX_LIBRARY: an alternate build of the SAME sources (A/B timing of compile-time switches); the source-hash check still applies
LIB_PATH = os.environ.get("WX_LIBRARY") or os.path.join(_HERE, "libwxengine.so")


class wx_config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("image_height", C.c_int32), ("image_width", C.c_int32),
        ("frames", C.c_int32), ("output_frames", C.c_int32),
        ("channels", C.c_int32), ("surface_channels", C.c_int32), ("input_only_channels", C.c_int32),
        ("output_only_channels", C.c_int32), ("levels", C.c_int32),
        ("dim", C.c_int32 * 4), ("depth", C.c_int32 * 4), ("dim_head", C.c_int32),
        ("global_window_size", C.c_int32 * 4), ("local_window_size", C.c_int32 * 4),
        ("n_embed_kernels", C.c_int32 * 4), ("embed_kernels", (C.c_int32 * 4) * 4), ("embed_strides", C.c_int32 * 4),
        ("pad_activate", C.c_int32), ("pad_lat", C.c_int32 * 2), ("pad_lon", C.c_int32 * 2),
        ("interp", C.c_int32), ("use_spectral_norm", C.c_int32), ("precision", C.c_int32), ("max_batch", C.c_int32),
        ("arch", C.c_int32),
        ("noise_latent_dim", C.c_int32), ("encoder_noise", C.c_int32), ("noise_correlated", C.c_int32),
    ]


class wx_band_msg(C.Structure):
    _fields_ = [("peer", C.c_int32), ("offset", C.c_int64), ("bytes", C.c_int64)]


class wx_kernel_stat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double)]


class WXEngineError(RuntimeError):
    pass


_lib = None

_PROTOTYPES = {
    "wx_create": ([C.POINTER(wx_config), C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "wx_load_tensor": ([C.c_void_p, C.c_char_p, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int64)], C.c_int),
    "wx_finalize_weights": ([C.c_void_p], C.c_int),
    "wx_destroy": ([C.c_void_p], C.c_int),
    "wx_num_tensors": ([C.c_void_p], C.c_int),
    "wx_tensor_info": ([C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int64)], C.c_int),
    "wx_set_denorm": ([C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int], C.c_int),
    "wx_set_tracer_fixer": ([C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int], C.c_int),
    "wx_set_layout": ([C.c_void_p, C.c_int, C.c_int, C.c_int], C.c_int),
    "wx_set_layout_groups": ([C.c_void_p, C.c_int] + [C.POINTER(C.c_int32)] * 4, C.c_int),
    "wx_forward": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p], C.c_int),
    "wx_step": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "wx_rollout": ([C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p], C.c_int),
    "wx_band_enable": ([C.c_void_p, C.c_int, C.c_int], C.c_int),
    "wx_band_info": ([C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int)], C.c_int),
    "wx_band_set_staging": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64], C.c_int),
    "wx_band_exchange": ([C.c_void_p, C.c_int, C.POINTER(wx_band_msg), C.c_int, C.POINTER(C.c_int), C.POINTER(wx_band_msg), C.c_int,
                          C.POINTER(C.c_int)], C.c_int),
    "wx_band_begin": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)], C.c_int),
    "wx_band_resume": ([C.c_void_p, C.POINTER(C.c_int)], C.c_int),
    "wx_band_rccl_unique_id": ([C.POINTER(C.c_uint8)], C.c_int),
    "wx_band_rccl_init": ([C.c_void_p, C.POINTER(C.c_uint8)], C.c_int),
    "wx_band_step_rccl": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "wx_band_plan_create": ([C.POINTER(wx_config), C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "wx_band_plan_destroy": ([C.c_void_p], C.c_int),
    "wx_band_plan_num_exchanges": ([C.c_void_p, C.POINTER(C.c_int)], C.c_int),
    "wx_band_plan_exchange_name": ([C.c_void_p, C.c_int, C.POINTER(C.c_char_p)], C.c_int),
    "wx_band_plan_messages": ([C.c_void_p, C.c_int, C.c_int, C.POINTER(wx_band_msg), C.c_int, C.POINTER(C.c_int), C.POINTER(wx_band_msg),
                               C.c_int, C.POINTER(C.c_int)], C.c_int),
    "wx_band_plan_partition": ([C.c_void_p, C.c_int, C.POINTER(C.c_int32)], C.c_int),
    "wx_set_noise": ([C.c_void_p, C.c_uint64, C.c_int, C.c_int], C.c_int),
    "wx_set_noise_tape": ([C.c_void_p, C.POINTER(C.c_void_p), C.c_int], C.c_int),
    "wx_set_debug": ([C.c_void_p, C.c_int], C.c_int),
    "wx_debug_read": ([C.c_void_p, C.c_char_p, C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_int64)], C.c_int),
    "wx_query": ([C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)], C.c_int),
    "wx_profile": ([C.c_void_p, C.c_int], C.c_int),
    "wx_profile_reset": ([C.c_void_p], C.c_int),
    "wx_profile_read": ([C.c_void_p, C.POINTER(wx_kernel_stat), C.c_int, C.POINTER(C.c_int)], C.c_int),
    "wx_post_create": ([C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "wx_post_destroy": ([C.c_void_p], C.c_int),
    "wx_post_set_band": ([C.c_void_p, C.c_int, C.c_int], C.c_int),
    "wx_pre_create": ([C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int,
                       C.POINTER(C.c_void_p)], C.c_int),
    "wx_pre_destroy": ([C.c_void_p], C.c_int),
    "wx_pre_channels": ([C.c_void_p, C.POINTER(C.c_int)], C.c_int),
    "wx_pre_apply": ([C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_void_p], C.c_int),
    "wx_pre_set_transforms": ([C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                               C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float)], C.c_int),
    "wx_unxform_create": ([C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float),
                           C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "wx_unxform_destroy": ([C.c_void_p], C.c_int),
    "wx_unxform_apply": ([C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p], C.c_int),
    "wx_post_set_grid": ([C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int], C.c_int),
    "wx_post_set_grid_sigma": ([C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                C.c_int, C.c_int, C.c_int], C.c_int),
    "wx_post_set_stats": ([C.c_void_p] + [C.POINTER(C.c_float)] * 4, C.c_int),
    "wx_post_add_tracer_fixer": ([C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int], C.c_int),
    "wx_post_add_mass_fixer": ([C.c_void_p, C.c_int, C.c_int, C.c_int], C.c_int),
    "wx_post_add_water_fixer": ([C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int], C.c_int),
    "wx_post_add_energy_fixer_signed": ([C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                         C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_int], C.c_int),
    "wx_post_add_energy_fixer_updown": ([C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                         C.c_float, C.c_int], C.c_int),
    "wx_post_add_energy_fixer": ([C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_float, C.c_int], C.c_int),
    "wx_post_apply": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "wx_attach_postblock": ([C.c_void_p, C.c_void_p], C.c_int),
    "wx_diag_create": ([C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "wx_diag_destroy": ([C.c_void_p], C.c_int),
    "wx_diag_set_levels": ([C.c_void_p] + [C.POINTER(C.c_float)] * 4 + [C.c_int], C.c_int),
    "wx_diag_set_pressure_levels": ([C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_float], C.c_int),
    "wx_diag_apply": ([C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                       C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p], C.c_int),
    "wx_wind_create": ([C.c_int, C.c_int] + [C.POINTER(C.c_float), C.c_int] * 4 + [C.c_int, C.c_int, C.c_float, C.c_int, C.c_int,
                        C.POINTER(C.c_void_p)], C.c_int),
    "wx_wind_destroy": ([C.c_void_p], C.c_int),
    "wx_wind_apply": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                       C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_void_p, C.c_void_p], C.c_int),
    "wx_advect_create": ([C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_float,
                          C.c_int, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "wx_advect_destroy": ([C.c_void_p], C.c_int),
    "wx_advect_apply": ([C.c_void_p] + [C.c_void_p, C.c_int64] * 4 + [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                         C.POINTER(C.c_void_p), C.c_int, C.c_void_p], C.c_int),
    "wx_hybrid_create": ([C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float),
                          C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "wx_hybrid_destroy": ([C.c_void_p], C.c_int),
    "wx_hybrid_apply": ([C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.c_int, C.c_int,
                         C.c_void_p, C.c_int64, C.c_void_p], C.c_int),
    "wx_regrid_create": ([C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int,
                          C.POINTER(C.c_void_p)], C.c_int),
    "wx_regrid_destroy": ([C.c_void_p], C.c_int),
    "wx_regrid_apply": ([C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int,
                         C.POINTER(C.c_void_p), C.c_void_p], C.c_int),
    "wx_tisr_create": ([C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                        C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "wx_tisr_destroy": ([C.c_void_p], C.c_int),
    "wx_tisr_compute": ([C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p], C.c_int),
    "wx_perturb_create": ([C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "wx_perturb_destroy": ([C.c_void_p], C.c_int),
    "wx_perturb_batch": ([C.c_void_p, C.POINTER(C.c_int)], C.c_int),
    "wx_perturb_apply": ([C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_float), C.c_float, C.c_void_p,
                          C.c_int64, C.POINTER(C.c_float), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p], C.c_int),
    "wx_spectrum_create": ([C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "wx_spectrum_destroy": ([C.c_void_p], C.c_int),
    "wx_spectrum_apply": ([C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int] + [C.c_void_p] * 7 + [C.c_void_p],
                          C.c_int),
    "wx_metrics_create": ([C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "wx_metrics_destroy": ([C.c_void_p], C.c_int),
    "wx_metrics_apply": ([C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                          C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                          C.c_int, C.c_double, C.c_void_p, C.c_void_p], C.c_int),
    "wx_ensemble_create": ([C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "wx_ensemble_destroy": ([C.c_void_p], C.c_int),
    "wx_ensemble_apply": ([C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                           C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_double, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p],
                          C.c_int),
    "wx_winattn_create": ([C.c_void_p, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "wx_winattn_apply": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "wx_winattn_destroy": ([C.c_void_p], C.c_int),
    "wx_band_comm_stream": ([C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)], C.c_int),
    "wx_swin_create": ([C.c_void_p, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "wx_swin_load": ([C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_float), C.c_int64], C.c_int),
    "wx_swin_finalize": ([C.c_void_p], C.c_int),
    "wx_swin_apply": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "wx_swin_flops": ([C.c_void_p, C.POINTER(C.c_double)], C.c_int),
    "wx_swin_destroy": ([C.c_void_p], C.c_int),
    "wx_fuxi_create": ([C.c_void_p, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "wx_fuxi_load": ([C.c_void_p, C.c_char_p, C.POINTER(C.c_float), C.c_int64], C.c_int),
    "wx_fuxi_finalize": ([C.c_void_p], C.c_int),
    "wx_fuxi_forward": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "wx_fuxi_debug_map": ([C.c_void_p, C.c_char_p, C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_int64)], C.c_int),
    "wx_fuxi_query": ([C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)], C.c_int),
    "wx_fuxi_flops": ([C.c_void_p, C.POINTER(C.c_double)], C.c_int),
    "wx_fuxi_destroy": ([C.c_void_p], C.c_int),
    "wx_last_error": ([], C.c_char_p),
    "wx_version": ([], C.c_char_p),
}

# include/wxengine_sht.h: the extension header of the same library, bound by load_library() as well
_EXTENSION_PROTOTYPES = {
    "wx_sht_create": ([C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_char_p, C.c_int,
                       C.POINTER(C.c_void_p)], C.c_int),
    "wx_sht_destroy": ([C.c_void_p], C.c_int),
    "wx_sht_analysis": ([C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p], C.c_int),
    "wx_sht_synthesis": ([C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p], C.c_int),
    "wx_sht_vector_analysis": ([C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_void_p], C.c_int),
    "wx_sht_spectra": ([C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "wx_sht_table": ([C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int,
                      C.POINTER(C.c_double), C.POINTER(C.c_int)], C.c_int),
}

# include/wxengine_polefilter.h: the inverse vector transform and the diffusion and pole filter, bound by load_library() as well
_POLEFILTER_PROTOTYPES = {
    "wx_sht_vector_synthesis": ([C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p], C.c_int),
    "wx_polefilter_create": ([C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_int, C.c_int,
                              C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "wx_polefilter_destroy": ([C.c_void_p], C.c_int),
    "wx_polefilter_sht": ([C.c_void_p, C.POINTER(C.c_void_p)], C.c_int),
    "wx_polefilter_lowpass": ([C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p], C.c_int),
    "wx_polefilter_scalar": ([C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int64, C.c_void_p],
                             C.c_int),
    "wx_polefilter_vector": ([C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_void_p,
                              C.c_int64, C.c_void_p, C.c_int64, C.c_void_p], C.c_int),
    "wx_polefilter_gradient": ([C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p], C.c_int),
    "wx_polefilter_workspace": ([C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)], C.c_int),
}


def exported_symbols():
    """The functions of include/wxengine.h (the extension header's are _EXTENSION_PROTOTYPES)."""
    return sorted(_PROTOTYPES)


def load_library():
    """dlopen libwxengine.so (torch must be imported first so its bundled HIP runtime is the one bound)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise WXEngineError(f"{LIB_PATH} not found: build it with `python miles-credit_amd/build.py` "
                            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    import torch  # noqa: F401  (loads libamdhip64 with the SONAME our library needs)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (args, res) in list(_PROTOTYPES.items()) + list(_EXTENSION_PROTOTYPES.items()) + list(_POLEFILTER_PROTOTYPES.items()):
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    _check_not_stale(lib)
    _lib = lib
    return lib


def _check_not_stale(lib):
    """The .so is git-ignored and ships prebuilt: make sure it was built from the sources lying next to it (build.py embeds
    their hash in wx_version()).  WX_ALLOW_STALE=1 downgrades the error for bisecting with an old library."""
    build_py = os.path.join(os.path.dirname(_HERE), "build.py")
    if not os.path.isfile(build_py) or not os.path.isdir(os.path.join(os.path.dirname(_HERE), "csrc")):
        return   # installed without sources: nothing to compare with
    import importlib.util
    spec = importlib.util.spec_from_file_location("_wx_build", build_py)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = mod.source_hash()
    have = lib.wx_version().decode().rsplit("wxsrc:", 1)[-1]
    if have != want and os.environ.get("WX_ALLOW_STALE") != "1":
        raise WXEngineError(f"{LIB_PATH} was built from other sources (library wxsrc:{have}, sources wxsrc:{want}): "
                            "rebuild with `python miles-credit_amd/build.py`")


def _check(status: int):
    if status != 0:
        msg = load_library().wx_last_error().decode()
        raise WXEngineError(f"wxengine error {status}: {msg}")


class NativeHandle:
    """One handle of the C ABI and the wx_*_destroy that frees it.  ctypes takes the object itself wherever a handle is an argument
    (`_as_parameter_`); `out` is the out argument of the wx_*_create call that fills it."""

    def __init__(self, destroy):
        self._as_parameter_ = C.c_void_p()
        self._destroy = destroy

    @property
    def out(self):
        return C.byref(self._as_parameter_)

    def close(self) -> None:
        h, self._as_parameter_ = self._as_parameter_, C.c_void_p()
        if h.value:
            self._destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _gpu_tensor(t, ndim=None, contiguous=False, item_contiguous=False, device=None, dtype=None) -> bool:
    """The test of a tensor that goes to the library as a raw pointer: a torch tensor on the GPU, float32 (or `dtype`) and, where
    asked, of `ndim` dims, contiguous as a whole or per batch item, on GPU `device`.  The caller words the error."""
    import torch
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == (dtype or torch.float32)
            and (ndim is None or t.dim() == ndim) and (not contiguous or t.is_contiguous())
            and (not item_contiguous or t[0].is_contiguous()) and (device is None or t.device.index == device))


def _f32(a):
    """float* to a numpy argument (made contiguous float32 if it is not; the pointer keeps the array alive); None stays None."""
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))


def _stream_ptr(device=None):
    """torch's current stream on `device` (None: the current device) as the ABI's stream argument."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_gpu(phrase: str, device=None, load=None):
    """The library, for a constructor: WXEngineError "no GPU visible: `phrase`" where torch sees no GPU (or `device`, anything
    torch.device takes, is not one).  `load`: the caller's own name for load_library, where its host tests stub that name."""
    import torch
    if not torch.cuda.is_available() or (device is not None and not isinstance(device, int) and torch.device(device).type != "cuda"):
        raise WXEngineError(f"no GPU visible: {phrase}")
    return (load or load_library)()


class HandleCache(dict):
    """{key: NativeHandle}: one native handle per key (a geometry and a device), made on first use by `lib`'s `<family>_create` and
    freed by its `<family>_destroy`.  The library is first touched on a miss, so an object can be constructed without one."""

    def __init__(self, lib, family: str):
        super().__init__()
        self._lib, self._family = lib, family

    def get(self, key, make_args):
        """The handle of `key`; only on a miss `make_args()` is called, for wx_*_create's arguments in front of the out argument."""
        try:
            return self[key]
        except KeyError:
            h = NativeHandle(getattr(self._lib, self._family + "_destroy"))
            _check(getattr(self._lib, self._family + "_create")(*make_args(), h.out))
            self[key] = h
            return h


def ptr_array(ts):
    """void*[n] of the tensors' addresses; a None entry stays a null pointer."""
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def i64_array(xs):
    return (C.c_int64 * len(xs))(*xs)


def i32_array(xs):
    """int32_t[n] of a short list, without _i32's detour through numpy: these are built on every call of a product."""
    return (C.c_int32 * len(xs))(*xs)


def batch_stride(t, B: int) -> int:
    """Floats between two batch items of `t`, as the library takes it: 0 when B = 1 (the stride of a size-1 dim means nothing)."""
    return t.stride(0) if B > 1 else 0


def check_named_tensor(key, t, like=None, one_time=False) -> None:
    """The test of a named tensor [B, n_levels, n_time, H, W] that goes to the library as (pointer, batch stride): float32 on the
    GPU, 5-D, n_time 1 where the block takes `one_time` level only, every batch item contiguous, and -- with `like`, the
    (key, tensor) every tensor of the call is compared with -- on its device with its batch, n_time, H and W."""
    if not _gpu_tensor(t, ndim=5):
        raise WXEngineError(f"{key} must be a float32 [B, n_levels, {1 if one_time else 'n_time'}, H, W] tensor on the GPU")
    shape = t.shape
    if one_time and shape[2] != 1:
        raise WXEngineError(f"{key}: n_time = {shape[2]}; the device block takes one time level (n_time must be 1)")
    if not t[0].is_contiguous():
        raise WXEngineError(f"{key}: a batch item must be contiguous [n_levels, {1 if one_time else 'n_time'}, H, W] memory")
    if like is not None:
        like_key, ref = like
        if t.device != ref.device:
            raise WXEngineError(f"{key} is on {t.device}, {like_key} on {ref.device}: all tensors of one call live on one device")
        ref_shape = ref.shape
        if shape[0] != ref_shape[0] or shape[2:] != ref_shape[2:]:
            raise WXEngineError(f"{key}: shape {tuple(shape)} does not match {like_key}: {tuple(ref_shape)} "
                                f"(batch, n_time and H x W must agree)")


def _named_tensor_args(ts, out_levels=None):
    """A list of named tensors [B, n_levels, T, H, W] (checked by the caller: check_named_tensor), read where they lie -> (source
    pointer array, batch strides in floats, levels, fresh contiguous outputs -- of `out_levels` levels where given, else of their
    input's --, their pointer array)."""
    import torch
    B = ts[0].shape[0]
    outs = [torch.empty(t.shape if out_levels is None else (B, out_levels, *t.shape[2:]), dtype=torch.float32, device=t.device) for t in ts]
    return ptr_array(ts), i64_array([batch_stride(t, B) for t in ts]), i32_array([t.shape[1] for t in ts]), outs, ptr_array(outs)


def flatten_named(state: dict, name: str, owner: str) -> dict:
    """{var: tensor} of a flat or a nested {source: {var: tensor}} dict `name` of the block `owner`, in the dict's order."""
    flat = {}
    for key, value in state.items():
        if isinstance(value, dict):
            flat.update(value)
        else:
            flat[key] = value
    if not flat:
        raise ValueError(f"{owner}: '{name}' is empty")
    return flat


def copy_batch(batch: dict, data_types) -> dict:
    """A pre block's copy of the batch (credit/preblock/base.py:12-22): new dicts down to the variable level of every data type of
    `data_types` that is present, so the caller's dicts are never mutated; the tensors are shared."""
    batch = dict(batch)
    for data_type in data_types:
        if isinstance(batch.get(data_type), dict):
            batch[data_type] = {src: dict(v) if isinstance(v, dict) else v for src, v in batch[data_type].items()}
    return batch


def copy_out(table, device):
    """Behind the kernels on the current stream of GPU `device`: the copy of `table` into a fresh pinned buffer and an event.
    -> (pinned, event)"""
    import torch
    pinned = torch.empty(table.shape, dtype=table.dtype, pin_memory=True)
    pinned.copy_(table, non_blocking=True)
    event = torch.cuda.Event()
    event.record(torch.cuda.current_stream(device))
    return pinned, event


class PendingResult:
    """The result of one `submit`: the kernels and the copy into `pinned` are enqueued (copy_out), `result()` waits on `event` once
    and is `finish(host array)`; `keep` holds what the kernels read and write until then."""

    def __init__(self, pinned, event, finish, keep=None):
        self._pinned, self._event, self._finish, self._keep = pinned, event, finish, keep
        self._result = None

    def done(self) -> bool:
        return self._result is not None or self._event.query()

    def result(self):
        if self._result is None:
            self._event.synchronize()
            self._result = self._finish(self._pinned.numpy())
            self._keep = None
        return self._result
