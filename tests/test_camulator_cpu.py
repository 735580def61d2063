"""model.type camulator (credit/models/camulator.py) without a GPU: the config and its refusals in Python and through the C ABI,
the reference-layout state dict, the host model class, and tests/camulator_oracle.py against the reference's own forward
(tests/golden/model_K*.npz, tools/make_goldens.py --only camulator)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import camulator_oracle as KO
from camulator_cases import DEMO_LEVELS, GOLD, demo_physics, golden, post_model_conf
from oracle import wxformer_oracle as O
from wxengine import engine as E
from wxengine.config import WXConfig, named_config
from wxengine.synth import synth_input, synth_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_GATE = 2e-5    # tests/test_oracle_vs_reference.py: max|ref - oracle| <= 2e-5 * max|ref| (sub-module outputs: * max(1, max|.|))


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("wx_build", os.path.join(ROOT, "miles-credit_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(force=False, verbose=False)
    return E.load_library()


@functools.lru_cache(maxsize=None)
def _weights(name):
    return synth_state_dict(named_config(name))


def _k0_conf(**over):
    mc = dict(image_height=37, image_width=72, frames=1, channels=4, surface_channels=4, input_only_channels=4,
              output_only_channels=3, levels=3, dim=[32, 64, 128, 256], depth=[1, 1, 2, 1], global_window_size=[4, 2, 2, 1],
              local_window_size=3, cross_embed_kernel_sizes=[[4, 8, 16, 32], [2, 4], [2, 4], [2, 4]], cross_embed_strides=[2, 2, 2, 2],
              padding_conf=dict(activate=True, mode="earth", pad_lat=[6, 6], pad_lon=[12, 12]))
    mc.update(over)
    return mc


# ------------------------------------------------------------------ config and state dict
def test_named_configs_and_the_two_input_widths():
    k0, k0f, k0x, wide = (named_config(n) for n in ("K0", "K0F", "K0X", "K2048"))
    assert all(c.arch == "camulator" and c.output_frames == 1 for c in (k0, k0f, k0x, wide))
    assert WXConfig.from_model_conf(_k0_conf(), arch="camulator") == k0
    assert WXConfig.from_model_conf(_k0_conf(frames=2), arch="camulator") == k0f
    assert (k0.frames, k0f.frames, k0x.frames) == (1, 2, 2) and k0x.pad_lon == (13, 11)
    # the tensor carries `frames` times the channels; the first conv takes one frame's worth (camulator.py:462, :485, :587-588)
    assert (k0.input_channels, k0.model_input_channels) == (20, 20)
    assert (k0f.input_channels, k0f.model_input_channels) == (40, 20)
    assert (k0x.input_channels, k0x.model_input_channels) == (472, 236)     # 236 -> 256 padded: two channel groups of the pack kernel
    t0f = named_config("T0F")                                               # every other class: frames fold into channels
    assert t0f.input_channels == t0f.model_input_channels == 40
    assert k0.stage_hw == named_config("T0").stage_hw == k0f.stage_hw
    assert wide.dim == (256, 512, 1024, 2048) and wide.stage_hw == [(32, 32), (16, 16), (8, 8), (4, 4)] and not wide.pad_activate
    for c in (k0, k0f, k0x):
        for prec in ("fp32", "fp32s", "bf16"):
            c.check_precision(prec)
        spec = c.state_spec()
        assert spec["layers.0.0.convs.0.weight_orig"][1] == c.model_input_channels and "layers.0.0.convs.0.1.weight_orig" not in spec
        assert spec["cube_embedding.proj.weight"] == (32, c.model_input_channels, c.frames, 1, 1)
        assert "up_block1.sharp.weight" in spec and "up_block1.sharp.weight_orig" not in spec     # camulator.py:22-28 skips "sharp"
        assert spec["up_block4.0.weight_orig"] == (4 * c.output_channels, 64, 3, 3) and "up_block4.2.weight_orig" in spec
    assert len(k0f.state_spec()) == 516 and k0f.state_spec()["cube_embedding.proj.weight"] == (32, 20, 2, 1, 1)
    assert synth_input(k0f).shape == (1, 20, 2, 37, 72)


@pytest.mark.reference
@pytest.mark.parametrize("sn", [True, False])
@pytest.mark.parametrize("name", ["K0", "K0F", "K0X"])
def test_state_spec_equals_the_reference_class(name, sn):
    import oracle_stub
    oracle_stub.install()
    from credit.models.camulator import Camulator
    base = named_config(name)
    mc = _k0_conf(frames=base.frames, levels=base.levels, use_spectral_norm=sn,
                  padding_conf=dict(activate=True, mode="earth", pad_lat=list(base.pad_lat), pad_lon=list(base.pad_lon)))
    cfg = WXConfig.from_model_conf(mc, arch="camulator")
    with torch.device("meta"):
        ref = Camulator(**mc, post_conf=dict(activate=False))
    assert [(k, tuple(v.shape)) for k, v in ref.state_dict().items()] == list(cfg.state_spec().items())


def test_synthetic_weights_in_every_family():
    """Every weight family fills exactly the spec; the decoder's `sharp` convs stay plain (no u / v to iterate), every other conv
    carries iterated u / v whose sigma is near the true spectral norm."""
    from wxengine.synth import FAMILIES
    cfg = named_config("K0F")
    spec = cfg.state_spec()
    base = _weights("K0F")
    for fam in FAMILIES:
        sd = synth_state_dict(cfg, family=fam)
        assert [(k, v.shape) for k, v in sd.items()] == list(spec.items())
        assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in sd.values())
        assert not [k for k in sd if k.startswith("up_block1.sharp.weight_")]
        np.testing.assert_array_equal(sd["up_block1.sharp.weight"], base["up_block1.sharp.weight"])
    assert float(synth_state_dict(cfg, family="stress")["layers.0.0.convs.0.bias"].min()) > 2.0     # the one-sign CrossEmbed biases reach this arch's keys
    w = base["up_block1.conv.weight_orig"].reshape(512, -1)      # Conv2d: spectral norm over dim 0, as for wxformer
    sigma = base["up_block1.conv.weight_u"] @ (w @ base["up_block1.conv.weight_v"])
    assert 0.9 * np.linalg.svd(w, compute_uv=False)[0] < sigma


def test_refusals_python():
    with pytest.raises(ValueError, match="frames must be 1 or 2"):
        WXConfig.from_model_conf(_k0_conf(frames=3), arch="camulator")
    with pytest.raises(ValueError, match="noise layers"):
        WXConfig.from_model_conf(_k0_conf(noise_latent_dim=16), arch="camulator")
    with pytest.raises(ValueError, match="upsample_v_conv"):
        WXConfig.from_model_conf(_k0_conf(upsample_v_conv=True), arch="camulator")
    with pytest.raises(ValueError, match="output_frames"):
        WXConfig.from_model_conf(_k0_conf(output_frames=2), arch="camulator")


def test_2048_wide_model_is_a_bf16_model():
    """CAMulator's own widths: accepted in bf16, refused with fp32 storage in the words tests/synth_batches.py dim2048_fp32* pins."""
    wide = named_config("K2048")
    wide.check_precision("bf16")
    for prec in ("fp32", "fp32s"):
        with pytest.raises(ValueError, match="LayerNorm width unsupported"):
            wide.check_precision(prec)


def _create(lib, cc):
    h = ctypes.c_void_p()
    st = lib.wx_create(ctypes.byref(cc), 0, ctypes.byref(h))
    if st == 0:
        lib.wx_destroy(h)
    return st, lib.wx_last_error()


def test_refusals_and_acceptance_c_abi(lib):
    """wx_create checks the config before it looks for a device (tests/test_abi_cpu.py): -1 = WX_ERR_INVALID with the reason; an
    accepted config gets to an engine, or without a GPU to the device error."""
    hdr = open(os.path.join(ROOT, "include", "wxengine.h")).read()
    assert int(re.search(r"WX_ARCH_CAMULATOR\s*=\s*(\d+)", hdr).group(1)) == E.ARCH["camulator"] == 3
    assert int(re.search(r"#define\s+WX_ABI_VERSION\s+(\d+)", hdr).group(1)) == E.WX_ABI_VERSION == 3   # the struct did not change
    have_gpu = torch.cuda.is_available()
    for name in ("K0", "K0F", "K0X"):
        for prec in ("fp32", "fp32s", "bf16"):
            cc = E.make_c_config(named_config(name), prec)
            assert cc.arch == 3
            st, err = _create(lib, cc)
            assert (st == 0) if have_gpu else (st not in (0, -1)), (name, prec, err)
    wide = E.make_c_config(named_config("K2048"), "bf16")
    st, err = _create(lib, wide)
    assert (st == 0) if have_gpu else (st not in (0, -1)), err
    for prec in ("fp32", "fp32s"):
        st, err = _create(lib, E.make_c_config(named_config("K2048"), prec))
        assert st == -1 and b"LayerNorm width unsupported" in err
    cc = E.make_c_config(named_config("K0F"), "bf16")
    cc.frames = 3
    st, err = _create(lib, cc)
    assert st == -1 and b"frames must be 1 or 2" in err
    cc = E.make_c_config(named_config("K0"), "bf16")
    cc.noise_latent_dim = 16
    st, err = _create(lib, cc)
    assert st == -1 and b"noise layers" in err
    cc = E.make_c_config(named_config("K0"), "bf16")
    cc.output_frames = 2
    st, err = _create(lib, cc)
    assert st == -1 and b"output_frames" in err
    cc = E.make_c_config(named_config("K0"), "bf16")     # a wrong abi_version fails as before, whatever the arch
    cc.abi_version = E.WX_ABI_VERSION + 1
    st, err = _create(lib, cc)
    assert st == -1 and b"abi_version mismatch" in err
    cc = E.make_c_config(named_config("K0"), "bf16")     # one past the last arch is still unknown
    cc.arch = 4
    st, err = _create(lib, cc)
    assert st == -1 and b"unknown wx_config.arch" in err
    # lat-band mode: the plan builder shares the check (host only)
    plan = ctypes.c_void_p()
    cc = E.make_c_config(named_config("K0"), "bf16")
    assert lib.wx_band_plan_create(ctypes.byref(cc), 2, ctypes.byref(plan)) == -1
    assert b"camulator arch is not wired" in lib.wx_last_error()
    cc.arch = E.ARCH["wxformer"]                         # the same geometry as a wxformer is planned as before
    assert lib.wx_band_plan_create(ctypes.byref(cc), 2, ctypes.byref(plan)) == 0
    lib.wx_band_plan_destroy(plan)


def test_library_exports_nothing_new(lib):
    hdr = open(os.path.join(ROOT, "include", "wxengine.h")).read()
    declared = set(re.findall(r"\b(wx_[a-z_]+)\s*\(", hdr)) - {"wx_engine"}
    assert declared == set(E.exported_symbols()) and not [n for n in declared if "camulator" in n]


# ------------------------------------------------------------------ the host model class
def test_model_class_mirrors_the_reference_interface():
    from wxengine.model import CamulatorHIP, WXFormerHIP
    cfg = named_config("K0F")
    m = CamulatorHIP(precision="fp32", **_k0_conf(frames=2), post_conf=dict(activate=False), frame_patch_size=1, attn_dropout=0.0,
                     ff_dropout=0.0, some_future_kwarg=1)
    assert isinstance(m, WXFormerHIP) and m.cfg == cfg and m.frames == 2 and m.output_frames == 1
    assert list(m.state_dict().keys()) == list(cfg.state_spec().keys())
    synth = {k: torch.from_numpy(v) for k, v in _weights("K0F").items()}
    res = m.load_state_dict(synth, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.state_dict()["up_block2.sharp.weight"], synth["up_block2.sharp.weight"])
    # no legacy key migration for this arch: a ZeroPad2d-style key is simply not one of the model's
    moved = {(k.replace(".convs.0.", ".convs.0.1.") if k.startswith("layers.0.0.convs.0.") else k): v for k, v in synth.items()}
    res = m.load_state_dict(moved, strict=False)
    assert "layers.0.0.convs.0.bias" in res.missing_keys and "layers.0.0.convs.0.1.bias" in res.unexpected_keys
    with pytest.raises(TypeError, match="output_frames"):
        CamulatorHIP(**_k0_conf(), output_frames=1)
    with pytest.raises(ValueError, match="frames must be 1 or 2"):
        CamulatorHIP(**_k0_conf(frames=4))
    with pytest.raises(E.WXEngineError):      # no CPU fallback
        m(torch.from_numpy(synth_input(cfg)))


@pytest.mark.reference
def test_the_reference_yaml_model_section_constructs():
    """config/gen_2/camulator/camulator_gen2_casper.yml with `type: "camulator_hip"` and precision bf16: same state-dict keys and
    shapes as the reference class built from the same section (both on the meta device: 0.7 G parameters)."""
    import oracle_stub
    oracle_stub.install()
    import yaml
    from credit.models.camulator import Camulator
    from wxengine.model import CamulatorHIP
    with open(os.path.join(oracle_stub.REFERENCE_ROOT, "config", "gen_2", "camulator", "camulator_gen2_casper.yml")) as f:
        mc = yaml.safe_load(f)["model"]
    assert mc.pop("type") == "camulator"
    with torch.device("meta"):
        m = CamulatorHIP(precision="bf16", **mc)
        ref = Camulator(**mc)
    assert m.cfg.dim == (256, 512, 1024, 2048) and m.cfg.stage_hw == [(144, 192), (72, 96), (36, 48), (18, 24)]
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    for prec in ("fp32", "fp32s"):
        with pytest.raises(ValueError, match="LayerNorm width unsupported"):
            m.cfg.check_precision(prec)


# ------------------------------------------------------------------ the oracle against the reference's forward
def test_average_is_what_avg_pool3d_computes():
    x = torch.from_numpy(synth_input(named_config("K0X")))
    want = torch.nn.functional.avg_pool3d(x, kernel_size=(2, 1, 1)).squeeze(2)
    assert torch.equal(KO.average_frames(x), want)
    assert torch.equal(KO.average_frames(x[:, :, :1]), x[:, :, 0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", ["K0", "K0F", "K0X", "K2048"])
def test_oracle_vs_reference_golden(name, dtype):
    cfg = named_config(name)
    g = golden(name)
    cap = {}
    y = KO.forward(cfg, _weights(name), synth_input(cfg), dtype=dtype, capture=cap)
    assert y.shape == (1, cfg.base_output_channels, 1) + tuple(cfg.out_hw)
    s = int(g["stride"])
    yr = torch.from_numpy(g["y"]).double()
    assert float((yr - y[0, :, 0, ::s, ::s].double()).abs().max()) <= REF_GATE * float(yr.abs().max())
    a = y[0, :, 0].double()
    tol = REF_GATE * float(yr.abs().max())
    assert float((torch.from_numpy(g["ch_sum"]) - a.sum(dim=(1, 2))).abs().max()) <= tol * a[0].numel()
    assert float((torch.from_numpy(g["ch_maxabs"]) - a.abs().amax(dim=(1, 2))).abs().max()) <= tol
    caps = [k[4:] for k in g.files if k.startswith("cap/")]
    assert (len(caps) == 13) if name in ("K0", "K0F") else not caps
    for n in caps:
        cs = int(g["cap_stride"])
        v = cap[n][0].double()
        ref = torch.from_numpy(g["cap/" + n]).double()
        if n == "pad" and dtype == torch.float32:      # a gather and one exact average: bit for bit
            assert torch.equal(ref, v[:, ::cs, ::cs])
        tol = REF_GATE * max(1.0, float(v.abs().max()))
        assert ref.shape == v[:, ::cs, ::cs].shape, n
        assert float((ref - v[:, ::cs, ::cs]).abs().max()) <= tol, n
        assert float((torch.from_numpy(g["cap_sum/" + n]) - v.sum(dim=(1, 2))).abs().max()) <= tol * v[0].numel(), n


def test_one_frame_equals_the_wxformer_oracle_on_renamed_keys():
    """k - s is even for every kernel of every YAML: padding (k - s) // 2 on both sides IS the ZeroPad2d split, so at frames == 1 the
    model is the wxformer class on the same weights with the CrossEmbed keys moved to convs.<b>.1.  fp64: the two conv calls (implicit
    against explicit zero padding) may sum in another order, which costs at most K * 2^-53 per dot product of K <= 20 480 terms
    (2.3e-12) and far less on average; 1e-10 of the maximum is three orders below one fp32 ulp, so a padding that differed by a
    single row or column could not pass."""
    cfg, w = named_config("K0"), named_config("T0W")
    sd = _weights("K0")
    renamed = {re.sub(r"^(layers\.\d\.0\.convs\.\d)\.", r"\1.1.", k): v for k, v in sd.items()}
    assert sum(k not in sd for k in renamed) == 40 and len(renamed) == len(sd)     # 10 branches x (bias, weight_orig, u, v)
    x = synth_input(cfg)
    ck, cw = {}, {}
    yk = KO.forward(cfg, sd, x, dtype=torch.float64, capture=ck)
    yw = O.forward(w, renamed, x, dtype=torch.float64, capture=cw)
    assert set(ck) == set(cw)
    assert torch.equal(ck["pad"], cw["pad"])
    for n in ck:
        assert float((ck[n] - cw[n]).abs().max()) <= 1e-10 * float(cw[n].abs().max()), n
    assert float((yk - yw).abs().max()) <= 1e-10 * float(yw.abs().max())


def test_post_case_is_well_conditioned():
    """model_K0F_post.npz (the reference class with its in-model TracerFixer + GlobalMassFixer): the oracle forward followed by the
    fixers' oracle reproduces it inside the suite's fixer gate, in fp32 and in fp64; the fixers have work far above that gate; no
    other channel moves."""
    from oracle import fixers_oracle as F
    from synth_batches import FIXER_GATES, fixer_block_error
    g = np.load(os.path.join(GOLD, "model_K0F_post.npz"))
    mc = post_model_conf()
    cfg = WXConfig.from_model_conf(mc, arch="camulator")
    x = synth_input(cfg)
    L, q = DEMO_LEVELS, slice(DEMO_LEVELS, 2 * DEMO_LEVELS)
    ph = demo_physics()
    sd = synth_state_dict(cfg)
    for dt in (torch.float32, torch.float64):
        y0 = KO.forward(cfg, sd, x, dtype=dt)[0, :, 0]
        assert float((torch.from_numpy(g["y_plain"]).double() - y0.double()).abs().max()) <= REF_GATE * float(np.abs(g["y_plain"]).max())
        grid = F.Grid(ph["lat2d"], ph["lon2d"], ph["p_levels"], midpoint=False, dtype=dt)
        v = F.tracer_fixer(y0, list(range(L, 2 * L)), [0.0] * L)
        v = F.mass_fixer(v, torch.from_numpy(x[0, :, -1]).to(dt), grid, L, L, 3).numpy()
        assert fixer_block_error(v, g["y"], q) <= FIXER_GATES["chain"]
    assert fixer_block_error(g["y_plain"], g["y"], q) > 20 * FIXER_GATES["chain"]
    rest = np.r_[0:L, 2 * L:g["y"].shape[0]]
    np.testing.assert_array_equal(g["y"][rest], g["y_plain"][rest])
