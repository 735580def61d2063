"""Host side of the hybrid-level interpolation (wxengine/hybrid_interp.py), no GPU needed: `midpoint_coefficients` against
hand-computed values (the vcoord rows, float64 averaging, the subset AFTER the averaging, the float32 cast), the constructor's
rejections with their reasons, the pre block's `data_types` and its copy of the caller's dicts, and without a GPU the block raises
-- after the argument checks -- instead of falling back."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from hybrid_cases import HYBRID_CASES, KEYS, block_args, midpoints  # noqa: E402

from wxengine import hybrid_interp as HI  # noqa: E402
from wxengine.engine import WXEngineError  # noqa: E402

A_IF = np.array([0.0, 10.0, 40.0, 90.0, 160.0])
B_IF = np.array([0.0, 0.1, 0.3, 0.6, 1.0])


def test_midpoint_coefficients_hand_computed():
    a, b = HI.midpoint_coefficients(A_IF, B_IF)
    assert a.dtype == b.dtype == np.float32
    assert list(a) == [5.0, 25.0, 65.0, 125.0] and np.array_equal(b, np.array([0.05, 0.2, 0.45, 0.8], np.float32))
    a, b = HI.midpoint_coefficients(A_IF, B_IF, on_interfaces=False)
    assert list(a) == list(A_IF) and np.array_equal(b, B_IF.astype(np.float32))
    a, b = HI.midpoint_coefficients(A_IF, B_IF, levels=[4, 2])                   # 1-based, in the order given, AFTER the averaging
    assert list(a) == [125.0, 25.0] and np.array_equal(b, np.array([0.8, 0.2], np.float32))
    a, b = HI.midpoint_coefficients(A_IF, B_IF, on_interfaces=False, levels=[5, 1])
    assert list(a) == [160.0, 0.0] and list(b) == [1.0, 0.0]
    a, b = HI.midpoint_coefficients(np.stack([A_IF, B_IF]))                      # the GFS vcoord convention: row 0 = a, row 1 = b
    assert list(a) == [5.0, 25.0, 65.0, 125.0] and np.array_equal(b, np.array([0.05, 0.2, 0.45, 0.8], np.float32))
    a, _ = HI.midpoint_coefficients(np.stack([A_IF, B_IF, B_IF]), levels=[3])    # further rows of vcoord are ignored
    assert list(a) == [65.0]


def test_midpoint_averaging_is_done_in_float64_before_the_cast():
    lo, hi = 1.0, 1.0 + 2.0 ** -23          # neighbours in float32: their float64 mean rounds to even, a float32 mean of casts too --
    x = np.array([lo, hi + 2.0 ** -40])     # but hi + 2^-40 casts DOWN to hi first; in float64 the mean lies above the tie and rounds UP
    a, _ = HI.midpoint_coefficients(x, x)
    assert a[0] == np.float32(hi) and np.float32(0.5) * (np.float32(x[0]) + np.float32(x[1])) == np.float32(lo)


@pytest.mark.parametrize("name", list(HYBRID_CASES))
def test_midpoint_coefficients_of_every_case(name):
    args = block_args(name)
    got = (HI.midpoint_coefficients(args["source_a"], args["source_b"], args["source_on_interfaces"], args["source_levels"])
           + HI.midpoint_coefficients(args["dest_a"], args["dest_b"], args["dest_on_interfaces"], args["dest_levels"]))
    for g, w in zip(got, midpoints(name)):
        assert g.dtype == np.float32 and np.array_equal(g, w), name


@pytest.mark.parametrize("kw,why", [
    (dict(variables=None), "variables is required"),
    (dict(variables="GFS/prognostic/3d/temperature"), "variables is required"),
    (dict(surface_pressure_var=None), "surface_pressure_var is required"),
    (dict(variables=[KEYS["T"], KEYS["q"], KEYS["T"]]), "a variable is listed twice"),
    (dict(variables=[f"GFS/prognostic/3d/v{i}" for i in range(33)]), "33 variables, one call takes at most 32"),
    (dict(source_a=None), "source_a is required"),
    (dict(dest_a=None, dest_b=None), "dest_a is required"),
    (dict(source_b=None), "without b, a must be the 2-D vcoord array"),
    (dict(source_b=B_IF), "a and b must be 1-D arrays of one length"),
    (dict(source_levels=[0, 1]), "levels are 1-based midpoint level numbers in 1 .. 16"),
    (dict(dest_levels=[14]), "levels are 1-based midpoint level numbers in 1 .. 13"),
    (dict(source_levels=[3]), "a single source midpoint level has no bracket"),
    (dict(source_a=np.arange(140.0), source_b=np.arange(140.0)), "139 source midpoint levels; the device block takes 2 .. 137"),
    (dict(dest_a=np.arange(139.0), dest_b=np.arange(139.0)), "138 destination midpoint levels; the device block takes 1 .. 137"),
    (dict(dest_levels=[]), "0 destination midpoint levels"),
    (dict(dest_a=np.array([0.0, np.nan, 3.0]), dest_b=np.zeros(3)), "dest_a has a non-finite midpoint coefficient"),
    (dict(source_a=np.arange(17.0), source_b=np.full(17, np.inf)), "source_b has a non-finite midpoint coefficient"),
])
def test_constructor_rejections_carry_their_reason(kw, why):
    args = block_args("L16to13")
    args.update(kw)
    for cls in (HI.HybridLevelInterp, HI.HybridLevelInterpPre):
        with pytest.raises(ValueError, match=why):
            cls(**args)


@pytest.fixture
def pretend_gpu(monkeypatch):
    """Lets the constructor pass its no-GPU check and spares it the library, for what the host side does before it touches the device."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(HI, "load_library", lambda: None)


def test_engine_arguments_keep_the_reference_names(pretend_gpu):
    blk = HI.HybridLevelInterp(key="y", chunk_size=7, **block_args("L127sub"))
    e = blk.engine
    assert blk.key == "y" and e.chunk_size == 7 and e.surface_pressure_var == KEYS["sp"] and e.variables[-1] == KEYS["idx"]
    assert e.source_a.shape == (63,) and e.dest_a.shape == (137,) and e.source_a.dtype == np.float32
    with pytest.raises(ValueError, match="Key 'y' not found"):
        blk({"y_processed": {}})
    # none of the variables present: returns before it looks up the surface pressure (hybrid_interp.py:117-120)
    batch = {"y": {"GFS": {"GFS/prognostic/3d/other": 1}}}
    assert blk(batch) is batch
    with pytest.raises(KeyError):
        blk({"y": {"GFS": {KEYS["T"]: 1}}})          # present, but no surface pressure


def test_preblock_data_types_and_copy(pretend_gpu):
    args = block_args("L16to13")
    with pytest.raises(ValueError, match="Invalid data_types {'metadata'}"):
        HI.HybridLevelInterpPre(data_types=["input", "metadata"], **args)
    pre = HI.HybridLevelInterpPre(**args)
    assert pre.data_types == ["input", "target"]
    seen = []

    def fake(nested):
        seen.append(nested)
        nested["GFS"][KEYS["q"]] = "interpolated"
    pre.engine.interp_nested = fake
    batch = {"input": {"GFS": {KEYS["q"]: "q0", KEYS["T"]: "t0"}}, "metadata": {"anything": 1}}        # no "target": skipped silently
    out = pre(batch)
    assert len(seen) == 1 and out["input"]["GFS"][KEYS["q"]] == "interpolated" and out["metadata"] is batch["metadata"]
    assert batch["input"]["GFS"][KEYS["q"]] == "q0" and set(batch) == {"input", "metadata"}      # the caller's dict is not mutated
    assert out["input"]["GFS"][KEYS["T"]] is batch["input"]["GFS"][KEYS["T"]]
    only_target = HI.HybridLevelInterpPre(data_types=["target"], **args)
    only_target.engine.interp_nested = fake
    only_target(batch)
    assert len(seen) == 1


def test_every_case_passes_the_argument_checks():
    """Past every ValueError -- to the device error where there is no GPU."""
    for name in HYBRID_CASES:
        if torch.cuda.is_available():
            HI.HybridLevelInterp(**block_args(name))
        else:
            with pytest.raises(WXEngineError, match="no GPU visible"):
                HI.HybridLevelInterp(**block_args(name))


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_no_gpu_raises_after_validation_instead_of_falling_back():
    for cls in (HI.HybridLevelInterp, HI.HybridLevelInterpPre):
        with pytest.raises(WXEngineError, match="no CPU fallback"):
            cls(**block_args("L16to13"))
        with pytest.raises(ValueError, match="a variable is listed twice"):       # the argument checks come first
            cls(**dict(block_args("L16to13"), variables=[KEYS["T"], KEYS["T"]]))
    import wxengine
    assert wxengine.HybridLevelInterp is HI.HybridLevelInterp and wxengine.HybridLevelInterpPre is HI.HybridLevelInterpPre
    assert wxengine.midpoint_coefficients is HI.midpoint_coefficients
