"""The noise-injection ensemble (CrossFormerWithNoise, model.type crossformer-ensemble) on the host side: the generator's numpy
restatement, configuration and state-dict layout, the registry path, and an oracle composition that pins the reference's draw order
against the tape goldens (tests/golden/ensemble_*.npz, tools/make_goldens_ensemble.py)."""
import copy
import glob
import os
import sys
import textwrap

import numpy as np
import pytest
import torch

from oracle import wxformer_oracle as O
from wxengine.config import named_config
from wxengine.noise import normals, philox4x32_10, tape_from_key, tape_shapes
from wxengine.synth import synth_input, synth_state_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF = "/root/reference"


def ensemble_config(base, noise_latent_dim=32, **kw):
    cfg = named_config(base)
    cfg.noise_latent_dim = noise_latent_dim
    for k, v in kw.items():
        setattr(cfg, k, v)
    cfg.validate()
    return cfg


def golden_config(z):
    dn, enc, cor = (int(v) for v in z["noise"])
    return ensemble_config(str(z["base"]), dn, encoder_noise=bool(enc), correlated=bool(cor))


# --------------------------------------------------------------------------- generator
def test_philox_known_answer_vectors():
    """Random123's known-answer vectors of Philox4x32-10 (kat_vectors: counter 0 / key 0 and all-ones)."""
    got = philox4x32_10(np.zeros((1, 4), np.uint32), (0, 0))[0]
    assert [f"{v:08x}" for v in got] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    got = philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), (0xFFFFFFFF, 0xFFFFFFFF))[0]
    assert [f"{v:08x}" for v in got] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]


def test_normals_are_standard_and_keyed():
    a = normals(7, 0, 0, 0, 1 << 20).astype(np.float64)
    assert np.isfinite(a).all()
    assert abs(a.mean()) < 5e-3 and abs(a.std() - 1.0) < 5e-3
    # every coordinate of the counter and the key changes the stream
    for other in (normals(8, 0, 0, 0, 4096), normals(7, 1, 0, 0, 4096), normals(7, 0, 1, 0, 4096), normals(7, 0, 0, 1, 4096)):
        assert abs(np.corrcoef(a[:4096], other)[0, 1]) < 0.08
    # the prefix property: element e does not depend on how many are drawn
    np.testing.assert_array_equal(normals(7, 0, 0, 0, 10), a[:10].astype(np.float32))


def test_box_muller_never_takes_log_of_zero():
    """u1 = ((w0 >> 8) + 1) 2^-24 lies in (0, 1]: the all-zero word gives the smallest u1, not 0."""
    from wxengine.noise import _box_muller
    n0, n1 = _box_muller(np.array([0, 0xFFFFFFFF], np.uint32), np.array([0, 0], np.uint32))
    assert np.isfinite(n0).all() and np.isfinite(n1).all()
    assert n0[1] == 0.0   # u1 = 1 -> rho = 0


# --------------------------------------------------------------------------- configuration
def test_noise_config_parsing_and_spec():
    cfg = ensemble_config("T0", 32)
    spec = cfg.state_spec()
    noise = {k: v for k, v in spec.items() if "noise" in k}
    assert len(noise) == 24
    assert noise["encoder_noise_layers.0.noise_transform.weight"] == (32, 32)
    assert noise["encoder_noise_layers.2.modulation"] == (1, 128, 1, 1)
    assert noise["noise_inject1.noise_transform.bias"] == (128,)
    assert noise["noise_inject3.noise_factor"] == (1,)
    assert not any(k.startswith("encoder_noise_layers") and k.endswith(("weight_orig", "weight_u", "weight_v")) for k in spec)
    assert len([k for k in ensemble_config("T0", 32, encoder_noise=False).state_spec() if "noise" in k]) == 12
    # the deterministic configurations are unchanged
    assert not any("noise" in k for k in named_config("T0").state_spec())
    from wxengine.config import WXConfig
    mc = dict(image_height=37, image_width=72, levels=3, noise_latent_dim=16, encoder_noise=False, correlated=True,
              encoder_noise_factor=0.1, decoder_noise_factor=0.2, freeze=True)
    c = WXConfig.from_model_conf(dict(mc, dim=[32, 64, 128, 256], frames=1, cross_embed_strides=[2, 2, 2, 2],
                                      global_window_size=[4, 2, 2, 1], local_window_size=3,
                                      padding_conf=dict(activate=True, mode="earth", pad_lat=[6, 6], pad_lon=[12, 12])))
    assert (c.noise_latent_dim, c.encoder_noise, c.correlated, c.encoder_noise_factor, c.decoder_noise_factor) == (16, False, True, 0.1, 0.2)
    assert [s for s in tape_shapes(c, 2)][:2] == [(2, 16), (2, 128, 6, 12)]


def test_noise_config_rejections():
    cfg = named_config("T0W")
    cfg.noise_latent_dim = 8
    with pytest.raises(ValueError, match="wxformer"):
        cfg.validate()
    cfg = named_config("T0")
    cfg.noise_latent_dim = -1
    with pytest.raises(ValueError):
        cfg.validate()


def test_c_abi_rejects_noise_with_wxformer_and_lat_band():
    """Host-only entry point (wx_band_plan_create builds the configuration without a GPU)."""
    import ctypes as C
    from wxengine import engine as E
    try:
        lib = E.load_library()
    except E.WXEngineError as e:
        pytest.skip(str(e))
    plan = C.c_void_p()
    cfg = ensemble_config("T0", 16)
    cc = E.make_c_config(cfg, "bf16")
    assert cc.noise_latent_dim == 16 and cc.encoder_noise == 1 and cc.noise_correlated == 0
    assert lib.wx_band_plan_create(C.byref(cc), 2, C.byref(plan)) == -1
    assert b"noise" in lib.wx_last_error()
    cc0 = E.make_c_config(named_config("T0"), "bf16")   # deterministic: the plan builds as before
    assert lib.wx_band_plan_create(C.byref(cc0), 2, C.byref(plan)) == 0
    lib.wx_band_plan_destroy(plan)
    w = E.make_c_config(named_config("T0W"), "bf16")
    w.noise_latent_dim = 16
    assert lib.wx_band_plan_create(C.byref(w), 2, C.byref(plan)) == -1
    assert b"wxformer" in lib.wx_last_error()
    assert lib.wx_set_noise(None, 0, 0, 0) == -1 and lib.wx_set_noise_tape(None, None, 0) == -1


def test_synth_noise_weights_and_unchanged_backbone():
    cfg = ensemble_config("T0", 32)
    sd = synth_state_dict(cfg)
    base = synth_state_dict(named_config("T0"))
    for k, v in base.items():
        np.testing.assert_array_equal(sd[k], v)
    nf = sd["noise_inject1.noise_factor"][0]
    assert 0.2 < nf < 0.4
    m = sd["encoder_noise_layers.1.modulation"]
    assert m.min() > 0.5 and m.max() < 1.5
    w = sd["noise_inject2.noise_transform.weight"]
    assert abs(float(w.std()) - 1 / np.sqrt(32)) < 0.05


# --------------------------------------------------------------------------- against the live reference
def _ref_models():
    import oracle_stub
    oracle_stub.install()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from credit.models.wxformer.crossformer_ensemble import CrossFormerWithNoise
    return CrossFormerWithNoise


@pytest.mark.reference
@pytest.mark.parametrize("encoder_noise", [True, False])
def test_state_spec_equals_reference_state_dict(encoder_noise):
    CrossFormerWithNoise = _ref_models()
    sys.path.insert(0, os.path.join(os.path.dirname(GOLD), "..", "tools"))
    from make_goldens_ensemble import reference_ensemble
    cfg = ensemble_config("T0", 32, encoder_noise=encoder_noise)
    ref = reference_ensemble(cfg)
    assert isinstance(ref, CrossFormerWithNoise)
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert want == {k: tuple(v) for k, v in cfg.state_spec().items()}
    assert len([k for k in want if "noise" in k]) == (24 if encoder_noise else 12)


@pytest.mark.reference
def test_registry_builds_the_ensemble_class_and_loads_reference_checkpoints(tmp_path):
    CrossFormerWithNoise = _ref_models()
    import importlib
    import credit.models as cm
    import wxengine.model as wm
    from credit.models.base_model import BaseModel
    if not issubclass(wm.WXFormerHIP, BaseModel):
        importlib.reload(wm)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    custom = tmp_path / "my_models.py"
    custom.write_text(textwrap.dedent(f"""
        import sys
        sys.path[:0] = [{os.path.join(root, 'miles-credit_amd')!r}]
        from wxengine.model import register_ensemble
        register_ensemble("crossformer-ensemble_hip")
    """))
    model = dict(type="crossformer-ensemble_hip", frames=1, channels=4, surface_channels=4, input_only_channels=4,
                 output_only_channels=3, levels=3, image_height=37, image_width=72, patch_width=1, patch_height=1,
                 dim=[32, 64, 128, 256], depth=[1, 1, 2, 1], global_window_size=[4, 2, 2, 1], local_window_size=3,
                 cross_embed_kernel_sizes=[[4, 8, 16, 32], [2, 4], [2, 4], [2, 4]], cross_embed_strides=[2, 2, 2, 2],
                 use_spectral_norm=True, interp=True, noise_latent_dim=16, encoder_noise=True, correlated=False, freeze=True,
                 padding_conf=dict(activate=True, mode="earth", pad_lat=[6, 6], pad_lon=[12, 12]))
    conf = {"model": copy.deepcopy(model), "custom_models": [str(custom)]}
    m = cm.load_model(conf)
    assert isinstance(m, wm.WXFormerEnsembleHIP) and isinstance(m, BaseModel)
    ref_kwargs = {k: v for k, v in model.items() if k != "type"}
    ref_kwargs["post_conf"] = {"activate": False}
    ref = CrossFormerWithNoise(**ref_kwargs)
    res = m.load_state_dict(ref.state_dict(), strict=False)
    assert not res.missing_keys and not res.unexpected_keys
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    # the reference's own initial values of the noise scalars ride along
    np.testing.assert_allclose(m.state_dict()["noise_inject1.noise_factor"].numpy(), [0.275])
    assert m.noise_latent_dim == 16 and m.encoder_noise and not m.correlated


# --------------------------------------------------------------------------- oracle composition (draw order)
def noisy_forward(cfg, sd, x, tape):
    """CrossFormerWithNoise.forward from oracle/wxformer_oracle.py pieces plus the injection, replaying `tape` in the reference's
    draw order: per layer (latent, pixel) -- or one latent first when correlated -- encoder 0..2 then decoder 1..3."""
    t = dict((k, torch.from_numpy(np.asarray(v))) for k, v in sd.items())
    draws = iter(torch.from_numpy(d) for d in tape)
    z_shared = next(draws) if cfg.correlated else None
    caps = {}

    def inject(p, feat):
        z = z_shared if cfg.correlated else next(draws)
        r = next(draws)
        pixel = t[p + ".noise_factor"] * r
        style = torch.nn.functional.linear(z, t[p + ".noise_transform.weight"], t[p + ".noise_transform.bias"])
        out = feat + pixel * style.view(*style.shape, 1, 1) * t[p + ".modulation"]
        caps[p] = out[-1]
        return out

    x = torch.from_numpy(x)
    x = O.earth_pad(x, cfg.pad_lat, cfg.pad_lon)
    b, c, tt, h, w = x.shape
    z = x.reshape(b, c * tt, h, w)
    enc = []
    for s in range(4):
        z = torch.cat([O.cross_embed(z[i:i + 1], t, f"layers.{s}.0", list(cfg.cross_embed_kernel_sizes[s]), cfg.cross_embed_strides[s])
                       for i in range(b)])
        z = torch.cat([O.transformer(z[i:i + 1], t, f"layers.{s}.1", cfg.depth[s], cfg.local_window_size[s], cfg.global_window_size[s],
                                     cfg.dim_head, None) for i in range(b)])
        if cfg.encoder_noise and s < 3:
            z = inject(f"encoder_noise_layers.{s}", z)
        enc.append(z)
    upconv = bool(getattr(cfg, "upsample_v_conv", False))

    def ub(v, prefix):
        return torch.cat([O.up_block(v[i:i + 1], t, prefix, cfg.dim[0], upconv) for i in range(b)])
    z = inject("noise_inject1", ub(z, "up_block1"))
    z = inject("noise_inject2", ub(torch.cat([z, enc[2]], dim=1), "up_block2"))
    z = inject("noise_inject3", ub(torch.cat([z, enc[1]], dim=1), "up_block3"))
    z = torch.cat([z, enc[0]], dim=1)
    if upconv:
        z = torch.nn.functional.conv2d(O.upsample2x(z), O.folded_weight(t, "up_block4.1"), O._bias(t, "up_block4.1", torch.float32), padding=1)
    else:
        z = torch.nn.functional.conv_transpose2d(z, O.folded_weight(t, "up_block4"), O._bias(t, "up_block4", torch.float32), stride=2, padding=1)
    z = O.earth_unpad(z, cfg.pad_lat, cfg.pad_lon)
    if cfg.interp:
        z = O.bilinear_resize(z, cfg.image_height, cfg.image_width)
    assert next(draws, None) is None, "tape not fully consumed"
    return z, caps


TAPE_GOLDENS = sorted(glob.glob(os.path.join(GOLD, "ensemble_T*.npz")))


@pytest.mark.parametrize("path", TAPE_GOLDENS, ids=[os.path.basename(p) for p in TAPE_GOLDENS])
def test_oracle_composition_reproduces_the_tape_goldens(path):
    z = np.load(path)
    cfg = golden_config(z)
    B, st = int(z["batch"]), int(z["stride"])
    sd = synth_state_dict(cfg)
    tape = tape_from_key(cfg, B, str(z["tape_key"]))
    x = np.repeat(synth_input(cfg), B, axis=0)
    with torch.no_grad():
        y, caps = noisy_forward(cfg, sd, x, tape)
    scale = float(z["maxabs"])
    err = float(np.abs(y[:, :, ::st, ::st].numpy() - z["y"]).max())
    assert err <= 1e-5 * scale, f"{os.path.basename(path)}: y max err {err:.3e} (max|y| {scale:.3f})"
    for p, _ in cfg.noise_layers():
        ref = z["cap/" + p]
        got = caps[p][:, ::2, ::2].numpy()
        e = float(np.abs(got - ref).max())
        assert e <= 1e-5 * float(np.abs(ref).max()), f"{p}: {e:.3e}"
    # the noise matters: member 0 and member 1 differ by far more than the tolerance
    assert float(np.abs(z["y"][0] - z["y"][1]).max()) > 0.05 * scale
