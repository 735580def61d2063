"""The pressure-level products on the device (csrc/wx_diag.h through wxengine/diagnostics.py) against the reference's goldens
(tests/golden/diag_*.npz): the fused launch per output variable under the gate of tests/diag_cases.gate, the chain of the three
blocks and every product subset bit-identical to it, inputs read in place from views on a side stream, the rejections with their
reasons, and one composed run_forecast.  Every column of every fixture is compared.

Measured on MI355X, worst of the six cases, d_ref -> device against the fp32 golden / against the fp64 golden: model-level Z 2.1e-6 ->
2.2e-6 / 2.1e-6; u 1.0e-5 -> 1.1e-5 / 1.4e-6; v 2.1e-5 -> 2.3e-5 / 2.8e-6; q 2.3e-5 -> 2.4e-5 / 3.8e-6; T 3.3e-7 -> 3.9e-7 / 3.3e-7; Z on
pressure levels 6.4e-7 -> 7.7e-7 / 5.5e-7; MSLP 1.5e-7 -> 1.4e-7 / 1.5e-7.  Every variable is inside the gate."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from diag_cases import DIAG_CASES, FIELD_ORDER, KEYS, SRC, case_inputs, distance, gate, hybrid_coefficients, load_golden, output_names  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
PROG = ("T", "q", "u", "v", "sp", "t2m")


def pres_key(k):
    return f"{SRC}/derived_diagnostic/3d/{KEYS[k].split('/')[-1]}_PRES"


def out_key(v):
    return {"z_model": KEYS["z"], "mslp": KEYS["mslp"], "plev_T": pres_key("T"), "plev_Z": pres_key("z")}.get(v) or pres_key(v[5:])


def common(name, inp):
    c = DIAG_CASES[name]
    return dict(pressure_levels=c["plev"], interp_variables=[KEYS[f] for f in FIELD_ORDER[:c["n_fields"]]], temperature_var=KEYS["T"],
                surface_pressure_var=KEYS["sp"], surface_geopotential_var=KEYS["phis"], model_a=inp["a_mid"], model_b=inp["b_mid"])


def fused_block(name, inp, **kw):
    from wxengine.diagnostics import PressureLevelProducts
    args = dict(common(name, inp), specific_humidity_var=KEYS["q"], near_surface_temperature_var=KEYS["t2m"],
                geopotential_output_name=KEYS["z"], mslp_output_name=KEYS["mslp"], flip_vertical=DIAG_CASES[name]["flip_vertical"],
                model_a_half=inp["a_half"], model_b_half=inp["b_half"])
    args.update(kw)
    return PressureLevelProducts(**args)


def chain_blocks(name, inp):
    from wxengine.diagnostics import GeopotentialDiagnostic, MSLPDiagnostic, PressureInterpDiagnostic
    geo = GeopotentialDiagnostic(output_name=KEYS["z"], surface_geopotential_var=KEYS["phis"], surface_pressure_var=KEYS["sp"],
                                 temperature_var=KEYS["T"], specific_humidity_var=KEYS["q"], flip_vertical=DIAG_CASES[name]["flip_vertical"],
                                 model_a_half=inp["a_half"], model_b_half=inp["b_half"])
    interp = PressureInterpDiagnostic(geopotential_var=KEYS["z"], **common(name, inp))
    msl = MSLPDiagnostic(output_name=KEYS["mslp"], surface_pressure_var=KEYS["sp"], temperature_var=KEYS["t2m"],
                         surface_geopotential_var=KEYS["phis"])
    return geo, interp, msl


def batch_of(t):
    return {"y_processed": {SRC: {KEYS[k]: t[k] for k in PROG}}, "ic_raw": {SRC: {KEYS["phis"]: t["phis"]}}}


@pytest.fixture(scope="module")
def runs():
    """Per case: inputs on the GPU, goldens, and the fused launch's outputs (computed once, shared, never modified)."""
    out = {}
    for name in DIAG_CASES:
        g, f32, f64, d_ref = load_golden(name, GOLD)
        inp = case_inputs(name, check=g)
        t = {k: torch.from_numpy(inp[k]).cuda() for k in PROG + ("phis",)}
        y = fused_block(name, inp)(batch_of(t))["y_processed"][SRC]
        torch.cuda.synchronize()
        out[name] = dict(inp=inp, t=t, f32=f32, f64=f64, d_ref=d_ref, fused={v: y[out_key(v)] for v in output_names(name)})
    return out


@pytest.mark.parametrize("name", list(DIAG_CASES))
def test_fused_launch_vs_reference_goldens(runs, name):
    r = runs[name]
    bad = []
    for v in output_names(name):
        got = r["fused"][v].cpu().numpy()
        assert got.shape == r["f32"][v].shape, (name, v, got.shape)
        b32, b64 = gate(r["d_ref"][v])
        d32, d64 = distance(got, r["f32"][v]), distance(got, r["f64"][v])
        print(f"[diag gpu] {name} {v}: d_ref {r['d_ref'][v]:.2e}; vs fp32 golden {d32:.2e} (<= {b32:.2e}), vs fp64 golden {d64:.2e} (<= {b64:.2e})")
        if not (np.isfinite(got).all() and d32 <= b32 and d64 <= b64):
            bad.append((v, d32, b32, d64, b64))
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", list(DIAG_CASES))
def test_chain_of_three_blocks_is_bit_identical_to_the_fused_launch(runs, name):
    r = runs[name]
    batch = batch_of(r["t"])
    for blk in chain_blocks(name, r["inp"]):
        batch = blk(batch)
    y = batch["y_processed"][SRC]
    for v in output_names(name):
        assert torch.equal(y[out_key(v)], r["fused"][v]), (name, v)


@pytest.mark.parametrize("name", ["L16", "L13s2t", "L2bt", "L40"])
def test_every_product_subset_alone(runs, name):
    r = runs[name]
    geo, _, msl = chain_blocks(name, r["inp"])
    y = geo(batch_of(r["t"]))["y_processed"][SRC]                                   # Z only
    assert torch.equal(y[KEYS["z"]], r["fused"]["z_model"]) and KEYS["mslp"] not in y and pres_key("T") not in y
    y = msl(batch_of(r["t"]))["y_processed"][SRC]                                   # MSLP only
    assert torch.equal(y[KEYS["mslp"]], r["fused"]["mslp"]) and KEYS["z"] not in y
    y = fused_block(name, r["inp"], write_geopotential=False, mslp_output_name=None,
                    near_surface_temperature_var=None)(batch_of(r["t"]))["y_processed"][SRC]    # pressure levels without model-level Z or MSLP
    assert KEYS["z"] not in y and KEYS["mslp"] not in y
    for v in output_names(name):
        if v.startswith("plev_"):
            assert torch.equal(y[out_key(v)], r["fused"][v]), (name, v)


@pytest.mark.parametrize("name", ["L16", "L2bt"])
def test_inputs_are_read_in_place_from_views_on_a_side_stream(runs, name):
    """The named tensors as Reconstruct hands them out: slices of one [B, C, T, H, W] tensor (with B = 2 the batch items of a
    view are not adjacent in memory).  No contiguous copy may be assumed, and the launch follows the current stream."""
    r = runs[name]
    t = r["t"]
    big = torch.cat([torch.full_like(t["sp"], 7.0)] + [t[k] for k in PROG] + [torch.full_like(t["sp"], -3.0)], dim=1)
    views, c0 = {}, 1
    for k in PROG:
        views[k] = big[:, c0:c0 + t[k].shape[1]]
        c0 += t[k].shape[1]
        assert views[k].data_ptr() != t[k].data_ptr() and views[k].untyped_storage().data_ptr() == big.untyped_storage().data_ptr()
    views["phis"] = t["phis"]
    keep = big.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y = fused_block(name, r["inp"])(batch_of(views))["y_processed"][SRC]
    side.synchronize()
    for v in output_names(name):
        assert torch.equal(y[out_key(v)], r["fused"][v]), (name, v)
    assert torch.equal(big, keep)


def test_rejections_carry_their_reason(runs):
    from wxengine.engine import WXDiag, WXEngineError
    r = runs["L16"]
    inp, t = r["inp"], r["t"]
    H, W = t["sp"].shape[3:]
    with pytest.raises(WXEngineError, match="n_levels must be 2"):
        WXDiag(H, W, 1)                                                              # L = 1
    d = WXDiag(H, W, 16)
    with pytest.raises(WXEngineError, match="n_plev must be 1"):
        d.set_pressure_levels([])                                                    # n_plev = 0
    d.set_levels(None, None, inp["a_mid"], inp["b_mid"])
    d.set_pressure_levels(inp["plev_pa"])
    with pytest.raises(WXEngineError, match="half-level coefficients"):               # coefficients of a requested product missing
        d.apply(t["sp"], t["phis"], T=t["T"], q=t["q"], want_z=True)
    d.set_levels(inp["a_half"], inp["b_half"], None, None)
    with pytest.raises(WXEngineError, match="mid-level coefficients"):
        d.apply(t["sp"], t["phis"], T=t["T"], q=t["q"], want_plev=True)
    with pytest.raises(WXEngineError, match="near-surface temperature"):              # an input of a requested product missing
        d.apply(t["sp"], t["phis"], want_mslp=True)
    with pytest.raises(WXEngineError, match="n_levels mismatch"):
        d.apply(t["sp"], t["phis"], T=t["T"][:, :13].contiguous(), q=t["q"][:, :13].contiguous(), want_z=True)
    with pytest.raises(WXEngineError, match="n_levels mismatch"):
        d.set_levels(inp["a_half"][:-1], inp["b_half"][:-1])
    with pytest.raises(WXEngineError, match="no product requested"):
        d.apply(t["sp"], t["phis"], T=t["T"], q=t["q"])
    geo, _, _ = chain_blocks("L16", inp)
    with pytest.raises(ValueError, match="ic_raw"):
        geo({"y_processed": batch_of(t)["y_processed"]})
    with pytest.raises(ValueError, match="y_processed"):
        geo({"ic_raw": batch_of(t)["ic_raw"]})


def test_composed_two_step_forecast_delivers_the_products():
    """run_forecast on T0 with [InverseScale, GeopotentialDiagnostic, PressureInterpDiagnostic, MSLPDiagnostic]: the new keys reach
    `consume` with the right shapes and finite values, and equal the fused object applied to the same y_processed."""
    from synth_batches import gen2loop_batches, gen2loop_schema
    from wxengine.config import named_config
    from wxengine.diagnostics import GeopotentialDiagnostic, MSLPDiagnostic, PressureInterpDiagnostic, PressureLevelProducts
    from wxengine.forecast import InverseScale, run_forecast
    from wxengine.model import WXFormerHIP
    from wxengine.synth import synth_state_dict
    cfg = named_config("T0")
    sd = synth_state_dict(cfg)
    ic, frcs, _, _ = gen2loop_batches(cfg, 2)
    inp, out = gen2loop_schema(cfg)
    L, P = cfg.levels, "era5/prognostic/"
    # physical statistics: T, Q, surface pressure (s0) and 2 m temperature (s1) land in plausible ranges after InverseScale
    phys = {"T": (250.0, 4.0), "Q": (5e-3, 2e-4), "U": (0.0, 8.0), "V": (0.0, 8.0), "s0": (9.0e4, 800.0), "s1": (280.0, 4.0),
            "Z": (6000.0, 800.0)}
    mean = {k.split("/")[-1]: np.full(nl, phys.get(k.split("/")[-1], (0.3, 1.5))[0], np.float32) for k, nl in inp[:-2]}
    std = {k.split("/")[-1]: np.full(nl, phys.get(k.split("/")[-1], (0.3, 1.5))[1], np.float32) for k, nl in inp[:-2]}
    mean.update({f"d{i}": np.float32(0.1 * i) for i in range(cfg.output_only_channels)})
    std.update({f"d{i}": np.float32(2.0 + i) for i in range(cfg.output_only_channels)})
    for k, v in ic["input"]["era5"].items():     # the IC in the same physical units (normalised values unchanged)
        n = k.split("/")[-1]
        if n in phys:
            ic["input"]["era5"][k] = ((v - 0.3) / 1.5) * phys[n][1] + phys[n][0]
    cmap, cur = {}, 0
    for k, nl in out:
        cmap[k] = {"slice": slice(cur, cur + nl), "orig_shape": (nl, 1)}
        cur += nl
    mc = dict(image_height=37, image_width=72, frames=1, channels=4, surface_channels=4, input_only_channels=4,
              output_only_channels=3, levels=3, dim=[32, 64, 128, 256], depth=[1, 1, 2, 1],
              global_window_size=[4, 2, 2, 1], local_window_size=3,
              cross_embed_kernel_sizes=[[4, 8, 16, 32], [2, 4], [2, 4], [2, 4]], cross_embed_strides=[2, 2, 2, 2],
              padding_conf=dict(activate=True, mode="earth", pad_lat=[6, 6], pad_lon=[12, 12]), post_conf=dict(activate=False))
    model = WXFormerHIP(precision="fp32", **mc).to("cuda").eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    a_half, b_half, a_mid, b_mid = hybrid_coefficients(L)
    names = dict(temperature_var=P + "3d/T", surface_pressure_var=P + "2d/s0", surface_geopotential_var="era5/static/2d/Z")
    zkey, mkey = "era5/derived_diagnostic/3d/geopotential", "era5/derived_diagnostic/2d/mean_sea_level_pressure"
    plev = dict(pressure_levels=[500.0, 850.0, 1000.0], interp_variables=[P + "3d/U", P + "3d/V", P + "3d/Q"], model_a=a_mid, model_b=b_mid)
    chain = [InverseScale(mean, std),
             GeopotentialDiagnostic(output_name=zkey, specific_humidity_var=P + "3d/Q", model_a_half=a_half, model_b_half=b_half, **names),
             PressureInterpDiagnostic(geopotential_var=zkey, **plev, **names),
             MSLPDiagnostic(output_name=mkey, temperature_var=P + "2d/s1", surface_pressure_var=P + "2d/s0",
                            surface_geopotential_var="era5/static/2d/Z")]
    fused = PressureLevelProducts(specific_humidity_var=P + "3d/Q", near_surface_temperature_var=P + "2d/s1", geopotential_output_name=zkey,
                                  mslp_output_name=mkey, model_a_half=a_half, model_b_half=b_half, **plev, **names)
    cu = lambda b: {"input": {s: {k: v.cuda() for k, v in d.items()} for s, d in b["input"].items()}}  # noqa: E731
    ic_cu = cu(ic)
    H, W = cfg.image_height, cfg.image_width
    new = {zkey: (1, L, 1, H, W), mkey: (1, 1, 1, H, W)}
    new.update({f"era5/derived_diagnostic/3d/{n}_PRES": (1, 3, 1, H, W) for n in ("U", "V", "Q", "T", "geopotential")})
    seen = []

    def consume(yp, step):
        y = yp["era5"]
        again = fused({"y_processed": {"era5": {k: v for k, v in y.items() if k not in new}}, "ic_raw": ic_cu["input"]})["y_processed"]["era5"]
        for k, shape in new.items():
            assert tuple(y[k].shape) == shape, (step, k, tuple(y[k].shape))
            assert bool(torch.isfinite(y[k]).all()), (step, k)
            assert torch.equal(y[k], again[k]), (step, k)
        seen.append(step)
    run_forecast(model, ic_cu, [cu(f) for f in frcs], 2, cmap, mean, std, chain, consume)
    assert seen == [1, 2]
