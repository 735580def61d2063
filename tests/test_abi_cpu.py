"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every declared symbol,
the host mirror behaves like the reference's interface, and nothing silently falls back to the CPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from wxengine import engine as E
from wxengine.config import WXConfig, named_config
from wxengine.synth import synth_input, synth_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("wx_build", os.path.join(ROOT, "miles-credit_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(force=False, verbose=False)
    return E.load_library()


def test_library_exports_every_symbol_in_header(lib):
    hdr = open(os.path.join(ROOT, "include", "wxengine.h")).read()
    declared = set(re.findall(r"\b(wx_[a-z_]+)\s*\(", hdr))
    declared -= {"wx_engine"}
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/wxengine.h but not exported"
    assert declared == set(E.exported_symbols())
    assert b"gfx950" in lib.wx_version()


def _header_declarations():
    """{name: [argument text]} of every `int | const char* wx_name(args);` of include/wxengine.h, comments stripped."""
    hdr = open(os.path.join(ROOT, "include", "wxengine.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    decls = {}
    for name, args in re.findall(r"\b(?:int|const\s+char\s*\*)\s*(wx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr):
        args = " ".join(args.split())
        decls[name] = [] if args in ("", "void") else [a.strip() for a in args.split(",")]
    return decls


_SCALARS = {"int": (ctypes.c_int, ctypes.c_int32), "int32_t": (ctypes.c_int, ctypes.c_int32), "int64_t": (ctypes.c_int64,),
            "uint64_t": (ctypes.c_uint64,), "float": (ctypes.c_float,), "double": (ctypes.c_double,)}


def test_prototypes_match_the_header_argument_by_argument(lib):
    """engine._PROTOTYPES against include/wxengine.h by position: a pointer (anything with * or [, or a handle typedef) must be a
    ctypes pointer class, a scalar must be the ctypes type of exactly its C type -- a c_int where the header says int64_t would
    corrupt the argument silently."""
    from wxengine.native import _PROTOTYPES
    decls = _header_declarations()
    assert len(decls) == 111 and set(decls) == set(_PROTOTYPES)
    for name, args in sorted(decls.items()):
        ctypes_args = _PROTOTYPES[name][0]
        assert len(args) == len(ctypes_args), f"{name}: {len(args)} arguments in the header, {len(ctypes_args)} in _PROTOTYPES"
        for i, (arg, ct) in enumerate(zip(args, ctypes_args)):
            words = re.sub(r"\bconst\b", " ", arg).split()
            if "*" in arg or "[" in arg or re.fullmatch(r"wx_\w*handle|wx_band_plan", words[0]):
                is_pointer = ct in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ct, ctypes._Pointer)
                assert is_pointer, f"{name} argument {i} `{arg}` is a pointer, _PROTOTYPES has {ct.__name__}"
            else:
                assert words[0] in _SCALARS, f"{name} argument {i} `{arg}`: unknown scalar type"
                assert ct in _SCALARS[words[0]], f"{name} argument {i} `{arg}`: _PROTOTYPES has {ct.__name__}"


WX_ERR_INVALID, WX_ERR_STATE = -1, -2
NULL_HANDLE_IS_STATE = {"wx_fuxi_finalize", "wx_fuxi_forward", "wx_fuxi_query", "wx_swin_apply", "wx_swin_finalize", "wx_winattn_apply"}


def test_every_function_takes_a_null_handle_as_an_error(lib):
    """Every exported function but the creates, wx_last_error, wx_version and wx_band_rccl_unique_id, called with None for every
    pointer and 0 for every scalar: a destroy of nothing is WX_OK, everything else an error status with its reason -- WX_ERR_STATE
    for the six Swin / FuXi / window-attention calls that say so, WX_ERR_INVALID for the rest -- and never a crash."""
    from wxengine.native import _PROTOTYPES
    skipped = {"wx_last_error", "wx_version", "wx_band_rccl_unique_id"}
    names = [n for n in E.exported_symbols() if not n.endswith("_create") and n not in skipped]
    destroys = [n for n in names if n.endswith("_destroy")]
    assert len(destroys) == 18
    got = {}
    for name in names:
        args = [None if (ct in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ct, ctypes._Pointer)) else 0 for ct in _PROTOTYPES[name][0]]
        got[name] = getattr(lib, name)(*args)
        if name not in destroys:
            assert got[name] < 0 and lib.wx_last_error(), name
    want = {n: 0 if n in destroys else WX_ERR_STATE if n in NULL_HANDLE_IS_STATE else WX_ERR_INVALID for n in names}
    assert NULL_HANDLE_IS_STATE <= set(names) and got == want, {n: (got[n], want[n]) for n in names if got[n] != want[n]}


def test_config_struct_matches_header_layout():
    # 4-byte ints only, so the ctypes mirror and the C struct agree when the field count does
    hdr = open(os.path.join(ROOT, "include", "wxengine.h")).read()
    body = hdr[hdr.index("typedef struct wx_config {"):hdr.index("} wx_config;")]
    n_ints = 0
    for decl in re.findall(r"int32_t\s+([^;]+);", body):
        for var in decl.split(","):
            dims = [int(d) for d in re.findall(r"\[(\d+)\]", var)]
            n_ints += int(np.prod(dims)) if dims else 1
    assert ctypes.sizeof(E.wx_config) == 4 * n_ints


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_no_gpu_fails_loudly(lib):
    with pytest.raises(E.WXEngineError):
        E.WXEngine(named_config("T0"), "fp32")
    h = ctypes.c_void_p()
    cc = E.make_c_config(named_config("T0"), "fp32")
    assert lib.wx_create(ctypes.byref(cc), 0, ctypes.byref(h)) != 0
    assert lib.wx_last_error()


def test_null_handle_is_an_error_not_a_crash(lib):
    assert lib.wx_finalize_weights(None) != 0
    assert b"null" in lib.wx_last_error()
    assert lib.wx_forward(None, None, None, 1, None) != 0


def test_model_shim_mirrors_reference_interface():
    from wxengine.model import WXFormerHIP
    cfg = named_config("T0")
    mc = dict(image_height=37, image_width=72, frames=1, channels=4, surface_channels=4, input_only_channels=4,
              output_only_channels=3, levels=3, dim=[32, 64, 128, 256], depth=[1, 1, 2, 1],
              global_window_size=[4, 2, 2, 1], local_window_size=3,
              cross_embed_kernel_sizes=[[4, 8, 16, 32], [2, 4], [2, 4], [2, 4]], cross_embed_strides=[2, 2, 2, 2],
              padding_conf=dict(activate=True, mode="earth", pad_lat=[6, 6], pad_lon=[12, 12]),
              post_conf=dict(activate=False), some_future_kwarg=1)
    m = WXFormerHIP(precision="fp32", **mc)
    sd = m.state_dict()
    assert list(sd.keys()) == list(cfg.state_spec().keys())
    assert m.image_height == 37 and m.use_padding and m.use_interp
    synth = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg).items()}
    res = m.load_state_dict(synth, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    np.testing.assert_array_equal(m.state_dict()["up_block4.bias"].numpy(), synth["up_block4.bias"].numpy())
    # strict=False tolerates extra / missing keys like the reference's loader (base_model.py:77-80)
    extra = dict(synth)
    extra["not_a_key"] = torch.zeros(1)
    del extra["up_block4.bias"]
    res = m.load_state_dict(extra, strict=False)
    assert res.missing_keys == ["up_block4.bias"] and res.unexpected_keys == ["not_a_key"]
    with pytest.raises(RuntimeError):
        m.load_state_dict(extra, strict=True)
    # no CPU fallback
    with pytest.raises(E.WXEngineError):
        m(torch.from_numpy(synth_input(cfg)))
    assert isinstance(m, torch.nn.Module) and sum(p.numel() for p in m.parameters()) > 0


def test_config_validation_errors():
    base = dict(image_height=37, image_width=72, frames=1, channels=4, surface_channels=4, input_only_channels=4,
                output_only_channels=3, levels=3, dim=[32, 64, 128, 256], depth=[1, 1, 2, 1],
                global_window_size=[4, 2, 2, 1], local_window_size=3, cross_embed_strides=[2, 2, 2, 2],
                padding_conf=dict(activate=True, mode="earth", pad_lat=[6, 6], pad_lon=[12, 12]))
    WXConfig.from_model_conf(base)
    with pytest.raises(ValueError):  # window does not divide the stage map
        WXConfig.from_model_conf(dict(base, local_window_size=5))
    up = WXConfig.from_model_conf(dict(base, upsample_v_conv=True))  # Upsample + Conv3x3 decoder (crossformer.py:87-92)
    assert up.state_spec()["up_block1.conv.weight_orig"] == (128, 256, 3, 3) and "up_block4.1.weight_orig" in up.state_spec()
    with pytest.raises(ValueError):  # the flag belongs to the legacy class only
        WXConfig.from_model_conf(dict(base, upsample_v_conv=True), arch="wxformer")
    mir = WXConfig.from_model_conf(dict(base, padding_conf=dict(activate=True, mode="mirror", pad_lat=[6, 6], pad_lon=[12, 12])))
    assert mir.pad_mode == "mirror" and E.make_c_config(mir, "bf16").pad_activate == 2 and E.make_c_config(WXConfig.from_model_conf(base)).pad_activate == 1
    with pytest.raises(ValueError):
        WXConfig.from_model_conf(dict(base, padding_conf=dict(activate=True, mode="zeros", pad_lat=[6, 6], pad_lon=[12, 12])))
    with pytest.raises(ValueError):   # reflect padding needs pad < height
        WXConfig.from_model_conf(dict(base, padding_conf=dict(activate=True, mode="mirror", pad_lat=[37, 6], pad_lon=[12, 12])))
    with pytest.raises(ValueError):
        WXConfig.from_model_conf(dict(base, patch_height=2, patch_width=2))
    # dim_head (crossformer.py:372-401): 32 / 64 / 128, dividing every stage width (96: the standalone attention operators only --
    # no width the LayerNorm kernels take is a multiple of it; test_create_time_rejections_python)
    wide = WXConfig.from_model_conf(dict(base, dim=[64, 128, 256, 512], dim_head=64))
    assert wide.heads == (1, 2, 4, 8) and E.make_c_config(wide, "bf16").dim_head == 64
    with pytest.raises(ValueError):
        WXConfig.from_model_conf(dict(base, dim_head=64))               # 32 is not a multiple of 64
    with pytest.raises(ValueError):
        WXConfig.from_model_conf(dict(base, dim=[48, 96, 192, 384], dim_head=48))


def test_create_time_rejections_python():
    """WXConfig mirrors ModelSpec::derive(): what no kernel can run is refused when the config is built, with wx_create's words."""
    from synth_batches import ACCEPTED_CONFIGS, REJECTED_CONFIGS, accepted_config, accepted_precisions
    for name, (mc, prec, why) in REJECTED_CONFIGS.items():
        with pytest.raises(ValueError, match=why):
            WXConfig.from_model_conf(mc, precision=prec)
    # the 2048-wide model is a bf16 model: accepted there, and by from_model_conf without a precision
    wide = WXConfig.from_model_conf(REJECTED_CONFIGS["dim2048_fp32"][0])
    wide.check_precision("bf16")
    with pytest.raises(ValueError, match="LayerNorm width"):
        wide.check_precision("fp32")
    for name in ACCEPTED_CONFIGS:
        for prec in accepted_precisions(name):
            accepted_config(name, prec)


def test_create_time_rejections_c_abi(lib):
    """wx_create checks the config before it looks for a device: a shape no kernel runs is WX_ERR_INVALID with the reason at create
    time (it used to pass wx_create, load and finalize, and throw inside the first wx_forward); every acceptance class gets past the
    config check -- to an engine where a GPU is present, to the device error where none is."""
    from synth_batches import ACCEPTED_CONFIGS, REJECTED_CONFIGS, accepted_config, accepted_precisions
    have_gpu = torch.cuda.is_available()
    for name, (mc, prec, why) in REJECTED_CONFIGS.items():
        # the ABI's own check: the struct is built from an unvalidated WXConfig (the Python mirror would refuse first)
        cfg = WXConfig(**{k: tuple(tuple(x) if isinstance(x, list) else x for x in v) if isinstance(v, list) else v for k, v in mc.items()})
        h = ctypes.c_void_p()
        cc = E.make_c_config(cfg, prec)
        assert lib.wx_create(ctypes.byref(cc), 0, ctypes.byref(h)) == -1, name      # WX_ERR_INVALID
        assert why.encode() in lib.wx_last_error(), (name, lib.wx_last_error())
        assert not h.value
    for name in ACCEPTED_CONFIGS:
        for prec in accepted_precisions(name):
            h = ctypes.c_void_p()
            cc = E.make_c_config(accepted_config(name), prec)
            st = lib.wx_create(ctypes.byref(cc), 0, ctypes.byref(h))
            if have_gpu:
                assert st == 0, (name, prec, lib.wx_last_error())
                lib.wx_destroy(h)
            else:
                assert st != 0 and st != -1, (name, prec, lib.wx_last_error())       # not a config error: the missing device
    # the plan builder shares the check (host only)
    plan = ctypes.c_void_p()
    cc = E.make_c_config(accepted_config("W9"), "bf16")
    cc.dim[0], cc.dim[1], cc.dim[2], cc.dim[3] = 96, 192, 384, 768
    assert lib.wx_band_plan_create(ctypes.byref(cc), 2, ctypes.byref(plan)) == -1 and b"LayerNorm width" in lib.wx_last_error()


def test_named_configs_match_survey_parameter_counts():
    assert named_config("C1").num_params() == 25_371_688
    assert named_config("C3").num_params() == 124_038_620
    assert named_config("C3").stage_hw == [(400, 800), (200, 400), (100, 200), (50, 100)]
    assert named_config("C1").padded_hw == (241, 384)


def test_synthetic_weights_are_deterministic_and_warm():
    cfg = named_config("T0")
    a, b = synth_state_dict(cfg), synth_state_dict(cfg)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    # u, v are iterated: sigma ~ the true spectral norm (so eval() does not explode, SURVEY.md header)
    w = a["layers.1.1.layers.0.1.layers.1.weight_orig"].reshape(256, 64)
    sigma = a["layers.1.1.layers.0.1.layers.1.weight_u"] @ (w @ a["layers.1.1.layers.0.1.layers.1.weight_v"])
    true = np.linalg.svd(w, compute_uv=False)[0]
    assert 0.9 * true < sigma <= true * 1.001


def test_state_spec_equals_reference_state_dict():
    """The reference class's state-dict names and shapes per config (tools/make_goldens.py --only specs)."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "reference_state_specs.json")) as f:
        specs = json.load(f)
    assert sorted(specs) == sorted(("T0", "T1", "T0W", "T0U", "T0M", "T0F"))
    for name, spec in specs.items():
        ref = {k: tuple(v) for k, v in spec.items()}
        assert ref == dict(named_config(name).state_spec())


def _t0w_model():
    from wxengine.model import WXFormerPSHIP
    cfg = named_config("T0W")
    mc = dict(image_height=37, image_width=72, frames=1, channels=4, surface_channels=4, input_only_channels=4,
              output_only_channels=3, levels=3, dim=[32, 64, 128, 256], depth=[1, 1, 2, 1],
              global_window_size=[4, 2, 2, 1], local_window_size=3,
              cross_embed_kernel_sizes=[[4, 8, 16, 32], [2, 4], [2, 4], [2, 4]], cross_embed_strides=[2, 2, 2, 2],
              padding_conf=dict(activate=True, mode="earth", pad_lat=[6, 6], pad_lon=[12, 12]), post_conf=dict(activate=False))
    return cfg, WXFormerPSHIP(precision="fp32", **mc)


def test_load_state_dict_migrates_legacy_crossembed_keys_and_ddp_prefix():
    """Reference behaviour: wxformer/crossformer.py:247-283 (convs.<i>.X -> convs.<i>.1.X) and DDP's `module.` prefix.
    Before the fix a legacy checkpoint left 40 CrossEmbed tensors at zero without a word."""
    cfg, m = _t0w_model()
    synth = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg).items()}
    assert list(m.state_dict().keys()) == list(synth.keys())
    legacy = {}
    for k, v in synth.items():
        parts = k.split(".")
        if len(parts) > 5 and parts[2] == "0" and parts[3] == "convs" and parts[5] == "1":
            k = ".".join(parts[:5] + parts[6:])
        legacy[k] = v
    n_legacy = sum(1 for k in legacy if k not in synth)
    assert n_legacy > 0
    res = m.load_state_dict(legacy, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in synth.items():
        assert torch.equal(m.state_dict()[k], v), k
    # DDP checkpoint of the legacy layout
    _, m2 = _t0w_model()
    res = m2.load_state_dict({"module." + k: v for k, v in legacy.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m2.state_dict()["layers.0.0.convs.0.1.weight_orig"], synth["layers.0.0.convs.0.1.weight_orig"])
    # a key the checkpoint already carries in the new layout is never clobbered by its legacy alias
    both = dict(synth)
    both["layers.0.0.convs.0.bias"] = torch.full_like(synth["layers.0.0.convs.0.1.bias"], 7.0)
    res = m2.load_state_dict(both, strict=False)
    assert res.unexpected_keys == ["layers.0.0.convs.0.bias"]
    assert torch.equal(m2.state_dict()["layers.0.0.convs.0.1.bias"], synth["layers.0.0.convs.0.1.bias"])


def test_load_state_dict_rejects_same_numel_other_layout():
    """torch raises "size mismatch"; the engine used to compare numel() only and scrambled a transposed ConvTranspose weight."""
    from wxengine.model import WXFormerHIP
    cfg = named_config("T0")
    mc = dict(image_height=37, image_width=72, frames=1, channels=4, surface_channels=4, input_only_channels=4,
              output_only_channels=3, levels=3, dim=[32, 64, 128, 256], depth=[1, 1, 2, 1],
              global_window_size=[4, 2, 2, 1], local_window_size=3,
              cross_embed_kernel_sizes=[[4, 8, 16, 32], [2, 4], [2, 4], [2, 4]], cross_embed_strides=[2, 2, 2, 2],
              padding_conf=dict(activate=True, mode="earth", pad_lat=[6, 6], pad_lon=[12, 12]), post_conf=dict(activate=False))
    m = WXFormerHIP(precision="fp32", **mc)
    synth = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg).items()}
    key = "up_block1.conv.weight_orig"
    assert tuple(synth[key].shape) == (256, 128, 2, 2)
    bad = dict(synth)
    bad[key] = synth[key].reshape(128, 256, 2, 2)
    with pytest.raises(RuntimeError, match="size mismatch for up_block1.conv.weight_orig"):
        m.load_state_dict(bad, strict=False)
    ok = dict(synth)
    g = "layers.0.1.layers.0.0.norm.g"
    ok[g] = synth[g].reshape(-1)       # (1, C, 1, 1) vs (C,): singleton dims only
    m.load_state_dict(ok, strict=True)
    assert torch.equal(m.state_dict()[g].reshape(-1), synth[g].reshape(-1))


def test_c_abi_load_tensor_checks_the_shape(lib):
    # needs no GPU: wx_create refuses without one, so drive the check through a band plan-free path when a device exists
    if not torch.cuda.is_available():
        pytest.skip("wx_create needs a device; the Python-side check is covered above")
    eng = E.WXEngine(named_config("T0"), "fp32")
    w = np.zeros((128, 256, 2, 2), np.float32)
    with pytest.raises(E.WXEngineError, match="size mismatch"):
        eng.load_state_dict({"up_block1.conv.weight_orig": w})


def test_load_model_mirrors_the_reference_error_handler(tmp_path, caplog):
    """credit/models/base_model.py:57-87 + checkpoint.py:25-31: unexpected keys raise, missing keys warn.  With the reference importable
    the class INHERITS `BaseModel.load_model`; without it `wxengine.model._standalone_load_model` is attached -- same contract either way."""
    import logging
    from wxengine.model import WXFormerHIP
    cfg = named_config("T0")
    mc = dict(type="crossformer_hip", image_height=37, image_width=72, frames=1, channels=4, surface_channels=4, input_only_channels=4,
              output_only_channels=3, levels=3, dim=[32, 64, 128, 256], depth=[1, 1, 2, 1],
              global_window_size=[4, 2, 2, 1], local_window_size=3,
              cross_embed_kernel_sizes=[[4, 8, 16, 32], [2, 4], [2, 4], [2, 4]], cross_embed_strides=[2, 2, 2, 2],
              padding_conf=dict(activate=True, mode="earth", pad_lat=[6, 6], pad_lon=[12, 12]), post_conf=dict(activate=False),
              precision="fp32")
    synth = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg).items()}
    conf = {"save_loc": str(tmp_path), "model": mc}
    with pytest.raises(ValueError):
        WXFormerHIP.load_model(conf)
    torch.save({"model_state_dict": synth}, tmp_path / "checkpoint.pt")
    m = WXFormerHIP.load_model(conf)
    assert torch.equal(m.state_dict()["up_block4.bias"], synth["up_block4.bias"])
    part = dict(synth)
    del part["up_block4.bias"]
    torch.save(part, tmp_path / "model_checkpoint.pt")      # bare state dict, and this file name wins
    with caplog.at_level(logging.WARNING):
        WXFormerHIP.load_model(conf)
    assert any(r.levelno >= logging.WARNING and ("partial" in r.getMessage() or "absent from the checkpoint" in r.getMessage())
               for r in caplog.records)
    torch.save(dict(synth, stray=torch.zeros(1)), tmp_path / "model_checkpoint.pt")
    with pytest.raises(RuntimeError, match="stray"):
        WXFormerHIP.load_model(conf)


def test_library_version_carries_the_source_hash(lib):
    import importlib.util
    spec = importlib.util.spec_from_file_location("wx_build2", os.path.join(ROOT, "miles-credit_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert lib.wx_version().decode().endswith("wxsrc:" + mod.source_hash())
    assert mod.built_hash() == mod.source_hash() and not mod.needs_build()
    # a library built from other sources is refused by the loader
    class Fake:
        @staticmethod
        def wx_version():
            return b"wxengine 0.2 (gfx950) wxsrc:0123456789abcdef"
    with pytest.raises(E.WXEngineError, match="built from other sources"):
        E._check_not_stale(Fake())


def test_run_time_switches_are_read_in_one_place_and_documented():
    """Every WX_* switch of the native code is read by Options::from_env() (csrc/wx_options.h) and nowhere else, and the
    INTEGRATION.md table lists exactly those switches."""
    csrc = os.path.join(ROOT, "miles-credit_amd", "csrc")
    readers = sorted(f for f in os.listdir(csrc) if "getenv" in open(os.path.join(csrc, f)).read())
    assert readers == ["wx_options.h"]
    read = set(re.findall(r'"(WX_[A-Z0-9_]+)"', open(os.path.join(csrc, "wx_options.h")).read()))
    doc = set(re.findall(r"^\| `(WX_[A-Z0-9_]+)` \|", open(os.path.join(ROOT, "INTEGRATION.md")).read(), re.M))
    assert read and read == doc, f"read but not documented: {sorted(read - doc)}; documented but not read: {sorted(doc - read)}"
