"""tests/xform_oracle.py and the variable selection of wxengine/transforms.py against the LIVE reference classes
(credit/preblock/{fill_values,log,sqrt,_utils}.py, credit/postblock/{exp,square}.py) at the fixture shapes; skipped where the
reference tree is absent.  The scaler legs are the expressions pinned for DevicePreblock / InverseScale (bridgescaler is absent)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import xform_oracle as O  # noqa: E402
from xform_cases import (SRC, XFORM_CASES, batch_input, case_inputs, case_stats, level_distance, out_variables, post_blocks, pre_blocks,  # noqa: E402
                         target_channel_map)

pytestmark = pytest.mark.reference


def _reference():
    import oracle_stub
    oracle_stub.install()
    from credit.postblock.exp import ExpTransform
    from credit.postblock.square import SquareTransform
    from credit.preblock.fill_values import FillValues
    from credit.preblock.log import LogTransform
    from credit.preblock.sqrt import SqrtTransform
    return types.SimpleNamespace(FillValues=FillValues, LogTransform=LogTransform, SqrtTransform=SqrtTransform, ExpTransform=ExpTransform,
                                 SquareTransform=SquareTransform)


@pytest.mark.parametrize("name", list(XFORM_CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_oracle_matches_live_reference_chain(name, dtype):
    ref = _reference()
    fields, y_pred = case_inputs(name)
    mean, std = case_stats(name)
    st = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dtype).reshape(1, -1, 1, 1, 1)   # noqa: E731
    got = O.case_outputs(name, fields, y_pred, dtype)
    batch = {"input": batch_input(name, fields, lambda a: torch.from_numpy(a).to(dtype))}
    with torch.no_grad():
        for blk in pre_blocks(name, ref):
            batch = blk(batch)
        for v in XFORM_CASES[name]["variables"]:
            t = batch["input"][SRC][v["key"]]
            if v["name"] in mean:
                t = (t - st(mean[v["name"]])) / st(std[v["name"]]).clamp(min=1e-12)
            d = level_distance(got[f"pre:{v['name']}"], t.numpy())
            assert d.max() <= (0 if dtype == torch.float32 else 1e-14), (name, v["name"], d)
        y = torch.from_numpy(y_pred).to(dtype).flatten(1, 2)
        nested = {SRC: {}}
        for key, info in target_channel_map(name).items():
            t, n = y[:, info["slice"]].unflatten(1, info["orig_shape"]), key.split("/")[-1]
            nested[SRC][key] = t * st(std[n]) + st(mean[n]) if n in mean else t
        full = {"y_processed": nested}
        for blk in post_blocks(name, ref):
            full = blk(full)
        for v in out_variables(name):
            d = level_distance(got[f"post:{v['name']}"], full["y_processed"][SRC][v["key"]].numpy())
            assert d.max() <= (0 if dtype == torch.float32 else 1e-14), (name, v["name"], d)


def test_variable_selection_expands_like_the_reference():
    _reference()
    from credit.preblock._utils import _parse_variable_selection
    from wxengine.transforms import parse_variable_selection
    t = torch.zeros(1)
    state = {"input": {"era5": {"era5/prognostic/3d/Q": t, "era5/prognostic/3d/T": t, "era5/prognostic/2d/SP": t, "era5/static/2d/Z": t},
                       "goes": {"goes/prognostic/2d/C07": t, "goes/prognostic/2d/C13": t}},
             "target": {"era5": {"era5/prognostic/3d/Q": t, "era5/diagnostic/2d/TP": t}, "goes": {"goes/prognostic/2d/C07": t}}}
    selections = [[], ["era5"], ["era5/prognostic"], ["era5/prognostic/3d"], ["goes/prognostic/2d/C13", "era5/prognostic/3d/Q"],
                  ["era5/prognostic/3d/Q", "era5/prognostic", "era5/prognostic/3d/Q"], ["era5/static/2d/Z"], ["era5/prog"], ["nothing/here"],
                  ["era5/diagnostic"], ["goes", "era5/static"]]
    for sel in selections:
        for dts in (None, ["input"], ["target"], ["input", "target"], ["target", "input"]):
            assert parse_variable_selection(sel, state, dts) == _parse_variable_selection(sel, state, dts), (sel, dts)
    # a variable present only under "input" (a static field) is selected through ["input", "target"] and absent from ["target"]
    assert "era5/static/2d/Z" in parse_variable_selection([], state, ["input", "target"])
    assert "era5/static/2d/Z" not in parse_variable_selection([], state, ["target"])
    assert parse_variable_selection(["era5/prog"], state, ["input"]) == []              # a partial path ends at a "/"
