"""The hybrid-interpolation fixtures, the restatement (tests/hybrid_oracle.py) and wxengine.hybrid_interp.midpoint_coefficients against
the LIVE reference (credit/postblock/hybrid_interp.py, credit/preblock/hybrid_interp.py, credit/postblock/_interp_utils.py); skipped
where the reference tree is absent.  The classes read their coefficients through xarray: a stand-in module serves the case's arrays
to credit.postblock._interp_utils, and `get_meta_file_path` is the identity (both put in place with monkeypatch)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import hybrid_oracle as HO  # noqa: E402
from hybrid_cases import (HYBRID_CASES, KEYS, SRC, case_inputs, load_golden, midpoints, raw_coefficients, reference_args,  # noqa: E402
                          variables)

pytestmark = pytest.mark.reference
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture
def reference(monkeypatch):
    import oracle_stub
    oracle_stub.install()
    coef = {}
    before = sys.modules.get("xarray")
    standin = oracle_stub.serve_xarray(coef)
    import credit.postblock._interp_utils as RU
    import credit.postblock.hybrid_interp as RH
    import credit.preblock.hybrid_interp as RP
    monkeypatch.setattr(RU, "xr", standin)
    monkeypatch.setattr(RU, "get_meta_file_path", lambda path: path)
    yield RU, RH, RP, coef
    if before is None:
        sys.modules.pop("xarray", None)
    else:
        sys.modules["xarray"] = before


def batch_of(inp, dtype=torch.float32):
    return {SRC: {KEYS[k]: torch.from_numpy(inp[k]).to(dtype) for k in inp}}


@pytest.mark.parametrize("name", list(HYBRID_CASES))
def test_reference_reproduces_the_goldens_and_the_restatement(reference, name):
    _, RH, _, coef = reference
    g, f32, f64, _ = load_golden(name, GOLD)
    inp = case_inputs(name, check=g)             # the hashes
    kw, arrays = reference_args(name)
    coef.update(arrays)
    blk = RH.HybridLevelInterpPost(**kw)
    sa, sb, da, db = midpoints(name)
    for dtype in (torch.float32, torch.float64):
        with torch.no_grad():
            y = blk({"y_processed": batch_of(inp, dtype)})["y_processed"][SRC]
        fields = {v: torch.from_numpy(inp[v]) for v in variables(name)}
        mine = HO.interp(fields, torch.from_numpy(inp["sp"]), sa, sb, da, db, dtype=dtype)
        for v in variables(name):
            got = y[KEYS[v]].numpy()
            if dtype == torch.float32:
                assert np.array_equal(got, f32[v]), (name, v)
                assert np.abs(mine[v].numpy() - got).max() <= 1e-6 * np.abs(got).max(), (name, v)
            else:
                stored = np.abs(f64[v] - f32[v].astype(np.float64)) * 2.0 ** -24       # the rounding of the stored float32 difference
                assert (np.abs(got - f64[v]) <= 1e-12 * max(1.0, np.abs(got).max()) + stored).all(), (name, v)
                assert np.abs(mine[v].numpy() - got).max() <= 1e-12 * np.abs(got).max(), (name, v)


@pytest.mark.parametrize("name", list(HYBRID_CASES))
def test_midpoint_coefficients_equal_the_reference_loader(reference, name):
    """Every case's coefficient arguments: interfaces -> midpoints, a `levels` subset (L127sub, one), the 2-D vcoord convention
    (L127, L127sub), midpoints given directly (floor, shuf)."""
    from wxengine.hybrid_interp import midpoint_coefficients
    RU, _, _, coef = reference
    r = raw_coefficients(name)
    kw, arrays = reference_args(name)
    coef.update(arrays)
    for side in ("source", "dest"):
        want = RU.load_hybrid_level_coefficients(kw[f"{side}_level_info_file"], kw[f"{side}_a_var"], kw[f"{side}_b_var"],
                                                 kw[f"{side}_on_interfaces"], kw[f"{side}_levels"])
        got = midpoint_coefficients(r[f"{side}_a"], r[f"{side}_b"], r[f"{side}_on_interfaces"], r[f"{side}_levels"])
        mine = HO.midpoint_coefficients(r[f"{side}_a"], r[f"{side}_b"], r[f"{side}_on_interfaces"], r[f"{side}_levels"])
        for w, g, m in zip(want, got, mine):
            assert w.dtype == torch.float32 and g.dtype == np.float32
            assert np.array_equal(w.numpy(), g) and torch.equal(w, m), (name, side)
    assert all(np.array_equal(a, b) for a, b in zip(midpoints(name), midpoint_coefficients(
        r["source_a"], r["source_b"], r["source_on_interfaces"], r["source_levels"]) + midpoint_coefficients(
        r["dest_a"], r["dest_b"], r["dest_on_interfaces"], r["dest_levels"])))


def test_levels_subset_is_applied_after_the_averaging(reference):
    from wxengine.hybrid_interp import midpoint_coefficients
    RU, _, _, coef = reference
    a = np.array([0.0, 10.0, 40.0, 90.0, 160.0, 250.0])
    b = np.array([0.0, 0.1, 0.3, 0.6, 0.8, 1.0])
    coef.update(a=a, b=b, vc=np.stack([a, b]))
    for on_if, levels in ((True, [2, 5]), (True, [4, 1, 3]), (False, [6, 2]), (True, None)):
        want = RU.load_hybrid_level_coefficients("f.nc", "a", "b", on_if, levels)
        got = midpoint_coefficients(a, b, on_if, levels)
        got_vc = midpoint_coefficients(np.stack([a, b]), None, on_if, levels)
        want_vc = RU.load_hybrid_level_coefficients("f.nc", "vc", "vc", on_if, levels)
        for w, g, wv, gv in zip(want, got, want_vc, got_vc):
            assert np.array_equal(w.numpy(), g) and np.array_equal(wv.numpy(), gv) and np.array_equal(g, gv)


def test_pre_block_data_types_early_return_and_level_count_error(reference):
    _, RH, RP, coef = reference
    name = "L16to13"
    inp = case_inputs(name)
    kw, arrays = reference_args(name)
    coef.update(arrays)
    sa, sb, da, db = midpoints(name)
    with pytest.raises(ValueError, match="Invalid data_types"):
        RP.HybridLevelInterpPre(data_types=["input", "metadata"], **kw)
    pre = RP.HybridLevelInterpPre(data_types=["input"], **kw)
    nested = batch_of(inp)
    batch = {"input": nested, "target": batch_of(inp)}
    with torch.no_grad():
        out = pre(batch)
    assert batch["input"] is nested and nested[SRC][KEYS["T"]].shape[1] == 16          # the caller's dict is not mutated
    assert out["target"][SRC][KEYS["T"]].shape[1] == 16                                # "target" was not requested
    mine = HO.interp({v: torch.from_numpy(inp[v]) for v in variables(name)}, torch.from_numpy(inp["sp"]), sa, sb, da, db)
    for v in variables(name):
        assert torch.equal(out["input"][SRC][KEYS[v]], mine[v]), v
    # none of the variables present: the call returns before it looks up the surface pressure
    post = RH.HybridLevelInterpPost(**kw)
    empty = {"y_processed": {SRC: {"GFS/prognostic/3d/other": torch.zeros(1)}}}
    assert post(empty) is empty and list(empty["y_processed"][SRC]) == ["GFS/prognostic/3d/other"]
    # one present, one absent: the absent one is skipped silently
    some = {"y_processed": {SRC: {KEYS["T"]: torch.from_numpy(inp["T"]), KEYS["sp"]: torch.from_numpy(inp["sp"])}}}
    with torch.no_grad():
        y = post(some)["y_processed"][SRC]
    assert torch.equal(y[KEYS["T"]], mine["T"]) and KEYS["q"] not in y
    # a level count that is not the source's
    short = {"y_processed": {SRC: {KEYS["T"]: torch.from_numpy(inp["T"][:, :15]), KEYS["sp"]: torch.from_numpy(inp["sp"])}}}
    with pytest.raises(ValueError, match=r"HybridLevelInterp: 'GFS/prognostic/3d/temperature' has 15 levels but the source "
                                         r"coefficients define 16 midpoint levels\."):
        post(short)
