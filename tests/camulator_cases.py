"""Shared pieces of the CAMulator tests (model.type camulator, credit/models/camulator.py): the named configs, the model section of
the in-model PostBlock case, and the helpers that load a golden written by tools/make_goldens.py --only camulator."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL = ("K0", "K0F", "K0X")      # every precision; K2048 (CAMulator's own widths) is a bf16 model
DEMO_LEVELS = 7


def post_model_conf(post=True):
    """K0F's widths and two frames on the grid the reference's fixers carry for their own demo (`simple_demo`: 10 x 18, seven
    pressure levels, credit/postblock/gen1.py:188-223), padded to 16 x 32, with an in-model PostBlock: a TracerFixer on the humidity
    block and a GlobalMassFixer.  The input tensor carries two frames; the model consumes their mean and the fixer reads the last
    frame, as in fixers_frames2.npz.  Channels: x = [T | q | U | V] x 7 levels + 4 surface + 4 input-only, y = the 28 + 4 + 3."""
    L = DEMO_LEVELS
    q_inds = list(range(L, 2 * L))
    conf = dict(frames=2, channels=4, surface_channels=4, input_only_channels=4, output_only_channels=3, levels=L,
                image_height=10, image_width=18, patch_width=1, patch_height=1,
                cross_embed_kernel_sizes=[[4, 8, 16, 32], [2, 4], [2, 4], [2, 4]], cross_embed_strides=[2, 2, 2, 2],
                dim=[32, 64, 128, 256], depth=[1, 1, 1, 1], global_window_size=[2, 2, 2, 1], local_window_size=[2, 2, 2, 1],
                interp=True, use_spectral_norm=True,
                padding_conf=dict(activate=True, mode="earth", pad_lat=[3, 3], pad_lon=[7, 7]))
    if not post:
        return dict(conf, post_conf=dict(activate=False))
    off = dict(activate=False, activate_outside_model=False)
    conf["post_conf"] = dict(
        activate=True, skebs=dict(activate=False), data=dict(lead_time_periods=6),
        tracer_fixer=dict(activate=True, denorm=False, tracer_inds=q_inds, tracer_thres=[0.0] * L),
        global_mass_fixer=dict(activate=True, activate_outside_model=False, simple_demo=True, denorm=False, grid_type="pressure",
                               midpoint=False, fix_level_num=3, q_inds=q_inds),
        global_water_fixer=dict(off), global_energy_fixer=dict(off))
    return conf


def demo_physics():
    """The grid and levels `simple_demo` builds inside the reference's fixers (gen1.py:190-218), for set_physics."""
    lon2d, lat2d = np.meshgrid(np.arange(18, dtype=np.float32) * 20.0, np.arange(90, -91, -20).astype(np.float32))
    return dict(lat2d=lat2d, lon2d=lon2d, p_levels=np.array([100, 30000, 50000, 70000, 80000, 90000, 100000], np.float32))


def golden(name):
    return np.load(os.path.join(GOLD, f"model_{name}.npz"))
