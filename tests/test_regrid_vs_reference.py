"""The regridding fixtures, the restatement (tests/regrid_oracle.py) and wxengine.regrid.coalesce_weights against the LIVE reference
(credit/preblock/regrid.py); skipped where the reference tree is absent.  The class reads its weights through xarray: a stand-in
module serves the case's arrays, its dimension sizes and `name in ds`."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import regrid_oracle as RO  # noqa: E402
from regrid_cases import (REGRID_CASES, SRC, case_inputs, key_of, load_golden, reference_args, run_input, variables, weights)  # noqa: E402

pytestmark = pytest.mark.reference
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture
def reference(monkeypatch):
    import oracle_stub
    oracle_stub.install()
    arrays, sizes = {}, {}
    before = sys.modules.get("xarray")
    standin = oracle_stub.serve_xarray_dataset(arrays, sizes)
    import credit.preblock.regrid as RR
    monkeypatch.setattr(RR, "xr", standin)

    def make(name, run="plain", curvilinear=False, **over):
        kw, arr, sz = reference_args(name, run, curvilinear)
        arrays.clear(), arrays.update(arr), sizes.clear(), sizes.update(sz)
        return RR.Regridder(**dict(kw, **over))
    yield RR, make
    if before is None:
        sys.modules.pop("xarray", None)
    else:
        sys.modules["xarray"] = before


def batch_of(name, run, inp, dtype=torch.float32):
    return {SRC: {key_of(v): torch.from_numpy(run_input(name, run, inp[v])).to(dtype) for v in inp}}


@pytest.mark.parametrize("name", list(REGRID_CASES))
def test_reference_reproduces_the_goldens_bit_for_bit(reference, name):
    _, make = reference
    g, f32, f64 = load_golden(name, GOLD)
    inp = case_inputs(name, check=g)
    w = weights(name)
    for run in REGRID_CASES[name]["runs"]:
        blk = make(name, run)
        with torch.no_grad():
            y = blk({"input": batch_of(name, run, inp)})["input"][SRC]
        for v in variables(name):
            got = y[key_of(v)].numpy()
            assert got.dtype == np.float32 and np.array_equal(got, f32[(run, v)], equal_nan=True), (name, run, v)
        blk.weights = blk.weights.double()          # the float64 truth: the same instance, its weights in double, its matrix rebuilt
        blk._W = None
        with torch.no_grad():
            y = blk({"input": batch_of(name, run, inp, torch.float64)})["input"][SRC]
        for v in variables(name):
            got = y[key_of(v)].numpy()
            _, mag, _ = RO.regrid(run_input(name, run, inp[v]), w["row"], w["col"], w["S"], w["n_a"], w["n_b"], None,
                                  REGRID_CASES[name]["runs"][run]["flip_axis"])
            bad = np.isnan(got)
            assert np.array_equal(bad, np.isnan(f64[(run, v)]))
            err = np.abs(np.where(bad, 0.0, got - f64[(run, v)])).reshape(-1, w["n_b"])
            assert (err <= 1e-14 * np.where(np.isnan(mag), 0.0, mag)).all(), (name, run, v)
    for tag in ("rect", "curv") if name == "uniq" else ("rect",):
        blk = make(name, "plain", tag == "curv")
        assert str(blk.dst_grid_type) == str(g[f"grid_type:{tag}"])
        if blk.dst_grid_type is not None:
            assert np.array_equal(blk.dst_lat, g[f"dst_lat:{tag}"]) and np.array_equal(blk.dst_lon, g[f"dst_lon:{tag}"])


@pytest.mark.parametrize("name", list(REGRID_CASES))
def test_coalesce_weights_equals_the_reference_matrix(reference, name):
    """Indices and float32 values of `_get_W`'s coalesced matrix, bit for bit: the same order of the repeated pairs' additions."""
    from wxengine.regrid import coalesce_weights
    _, make = reference
    w = weights(name)
    W = make(name)._get_W(torch.device("cpu"))
    row_ptr, col, val = coalesce_weights(w["row"], w["col"], w["S"], w["n_a"], w["n_b"])
    idx = W.indices().numpy()
    assert np.array_equal(idx[1], col) and np.array_equal(np.bincount(idx[0], minlength=w["n_b"]), np.diff(row_ptr))
    assert (np.diff(idx[0]) >= 0).all() and np.array_equal(W.values().numpy(), val)
    dense = RO.dense_matrix(w["row"], w["col"], w["S"], w["n_a"], w["n_b"])
    assert np.abs(W.to_dense().numpy().astype(np.float64) - dense).max() <= 2.0 ** -23 * np.abs(dense).max()


def test_pre_block_behaviours(reference, caplog):
    RR, make = reference
    name = "bilin"
    inp = case_inputs(name)
    _, f32, _ = load_golden(name, GOLD)
    blk = make(name)
    assert blk.data_types == ["input", "target"] and tuple(blk.dst_shape) == (13, 23)
    with pytest.raises(ValueError, match="Invalid data_types"):
        make(name, data_types=["input", "metadata"])
    # absent "target": skipped; the caller's dict is not mutated
    nested = batch_of(name, "plain", inp)
    batch = {"input": nested}
    out = blk(batch)
    assert batch["input"] is nested and nested[SRC][key_of("a")].shape == (3, 9, 16) and list(out) == ["input"]
    assert np.array_equal(out["input"][SRC][key_of("a")].numpy(), f32[("plain", "a")])
    # a variable absent in one data type: skipped there
    both = {"input": batch_of(name, "plain", inp), "target": {SRC: {"GFS/prognostic/2d/other": torch.zeros(2)}}}
    out = blk(both)
    assert list(out["target"][SRC]) == ["GFS/prognostic/2d/other"] and out["input"][SRC][key_of("a")].shape == (3, 13, 23)
    # an absent source
    with pytest.raises(KeyError, match=r"Regridder: source 'GFS' not found in batch\['input'\]\."):
        blk({"input": {"ERA5": {}}})
    # a shape that is neither reading of the source grid
    with pytest.raises(ValueError, match=r"Cannot map input shape torch\.Size\(\[3, 9, 17\]\) to expected source grid size 144\."):
        blk({"input": {SRC: {key_of("a"): torch.zeros(3, 9, 17)}}})
    # the flip warning; flat input equal to 2-D input
    with caplog.at_level(logging.WARNING, logger="credit.preblock.regrid"):
        y = make(name, "flip2")({"input": batch_of(name, "flip2", inp)})["input"][SRC][key_of("a")]
    assert "Regridder: ignoring invalid flip_axis values [2]; spatial axes must be negative indices in [-2, -1]." in caplog.text
    assert np.array_equal(y.numpy(), f32[("plain", "a")])
    flat = make(name, "flat")({"input": batch_of(name, "flat", inp)})["input"][SRC][key_of("a")]
    assert flat.shape == (3, 13, 23) and np.array_equal(flat.numpy(), f32[("plain", "a")])
    # a kept flip is torch.flip in front of the unflipped block
    x = torch.from_numpy(inp["a"])
    y = make(name, "flip-1-2")({"input": {SRC: {key_of("a"): x}}})["input"][SRC][key_of("a")]
    y2 = make(name)({"input": {SRC: {key_of("a"): torch.flip(x, dims=[-1, -2])}}})["input"][SRC][key_of("a")]
    assert torch.equal(y, y2)
    # reshape_to_xy = False keeps the output flat
    rg = make("ragged")
    assert rg.dst_shape is None and rg.dst_grid_type is None
