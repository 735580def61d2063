"""Host side of wxengine/transforms.py without a GPU: argument validation (the reference's errors: credit/preblock/fill_values.py:78-96,
log.py:56-73, sqrt.py:44-50, postblock/exp.py:53-60), the orders and rule counts the fused kernel refuses, the composition of stacked
FillValues blocks, and the compiled channel table of a known batch."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from wxengine import transforms as X  # noqa: E402

Q, T, SP, SIC = "era5/prognostic/3d/Q", "era5/prognostic/3d/T", "era5/prognostic/2d/SP", "era5/static/2d/SIC"


def example():
    z = lambda n: torch.zeros(1, n, 1, 2, 3)   # noqa: E731
    return {"era5": {Q: z(3), T: z(2), SP: z(1), SIC: z(1)}}


KEYS, LEVELS = [Q, T, SP, SIC], [3, 2, 1, 1]


def table(transforms):
    return X.compile_channel_table(transforms, example(), KEYS, LEVELS)


def test_argument_validation_mirrors_the_reference():
    with pytest.raises(ValueError, match="Invalid data_types"):
        X.FillValues([], data_types=["metadata"])
    with pytest.raises(ValueError, match="Invalid data_types"):
        X.LogTransform([Q], data_types=["input", "prediction"])
    with pytest.raises(ValueError, match="Invalid data_types"):
        X.SqrtTransform([Q], data_types=["y"])
    with pytest.raises(ValueError, match="must have 'search' and 'fill'"):
        X.FillValues([{"search": "nan"}])
    with pytest.raises(ValueError, match="must have 'search' and 'fill'"):
        X.FillValues([{"fill": 0.0}])
    with pytest.raises(ValueError, match="'search' must be 'nan' or a number"):
        X.FillValues([{"search": "inf", "fill": 0.0}])
    with pytest.raises(ValueError, match="'op' must be one of"):
        X.FillValues([{"search": 0.0, "op": "eq", "fill": 0.0}])
    X.FillValues([{"search": "nan", "op": "whatever", "fill": 0.0}])          # op is not looked at for "nan" (fill_values.py:94)
    with pytest.raises(ValueError, match="Unsupported log base '3'"):
        X.LogTransform([Q], base="3")
    with pytest.raises(ValueError, match="Unsupported base 'E'"):
        X.ExpTransform([Q], base="E")                                        # before any GPU is asked for
    with pytest.raises(ValueError):
        X.LogTransform([Q], eps=0.0)                                         # math.log(0.0), as in the reference
    with pytest.raises(ValueError):
        X.ExpTransform([Q], eps=-1e-8)
    lt = X.LogTransform([Q], base="10", eps=1e-4)
    assert lt.data_types == ["input", "target"] and lt._log_eps == math.log10(1e-4) and lt._eps == 1e-4
    assert X.LogTransform([Q], base="2")._log_eps == math.log2(1e-8) and X.LogTransform([Q])._log_eps == math.log(1e-8)
    assert X.FillValues([]).variables == [] and X.FillValues([], variables=None).data_types == ["input", "target"]


def test_constructor_signatures_follow_the_reference():
    import inspect
    want = {X.FillValues: dict(variables=None, data_types=None), X.LogTransform: dict(data_types=None, base="e", eps=1e-8),
            X.SqrtTransform: dict(data_types=None), X.ExpTransform: dict(eps=1e-8, base="e", key="y_processed"),
            X.SquareTransform: dict(key="y_processed")}
    for cls, args in want.items():
        params = inspect.signature(cls.__init__).parameters
        assert list(params)[1] == ("rules" if cls is X.FillValues else "variables")
        for k, v in args.items():
            assert k in params and params[k].default == v, (cls.__name__, k)


def test_orders_and_rule_counts_the_kernel_does_not_serve_are_refused():
    nan0 = [{"search": "nan", "fill": 0.0}]
    with pytest.raises(ValueError, match="behind a log / sqrt"):
        table([X.LogTransform([Q]), X.FillValues(nan0, [Q])])
    with pytest.raises(ValueError, match="behind a log / sqrt"):
        table([X.SqrtTransform(["era5/prognostic"]), X.FillValues(nan0)])     # the empty list reaches Q too
    with pytest.raises(ValueError, match="second log / sqrt"):
        table([X.LogTransform([Q]), X.SqrtTransform([Q])])
    with pytest.raises(ValueError, match="second log / sqrt"):
        table([X.LogTransform([Q]), X.LogTransform(["era5/prognostic/3d"], base="2")])
    with pytest.raises(ValueError, match="9 fill rules"):
        table([X.FillValues([{"search": float(i), "fill": 0.0} for i in range(9)], [Q])])
    with pytest.raises(ValueError, match="9 fill rules"):
        table([X.FillValues([{"search": float(i), "fill": 0.0} for i in range(5)], [Q]), X.FillValues([{"search": float(i), "fill": 1.0} for i in range(4)])])
    with pytest.raises(ValueError, match="without 'input'"):
        table([X.LogTransform([Q], data_types=["target"])])
    with pytest.raises(ValueError, match="descriptors"):
        table([object()])
    # what IS served: fills on one variable, a log on another, in any interleaving; eight rules
    assert table([X.LogTransform([Q]), X.FillValues(nan0, [SIC]), X.SqrtTransform([SP])]) is not None
    assert table([X.FillValues([{"search": float(i), "fill": 0.0} for i in range(8)], [Q])])["n_rules"][0] == 8
    assert table([]) is None and table(None) is None and table([X.LogTransform(["goes"])]) is None


def test_compiled_channel_table_of_a_known_batch():
    tab = table([X.FillValues([{"search": "nan", "fill": -1.0}, {"search": 0.0, "fill": 1e-4}, {"search": 0.0, "op": "<", "fill": 0.0}], [Q]),
                 X.FillValues([{"search": "nan", "fill": 0.0}], ["era5/static"]),
                 X.LogTransform([Q, SP], base="10", eps=1e-4), X.SqrtTransform([T])])
    assert list(tab["kind"]) == [3, 3, 3, 4, 4, 3, 0] and list(tab["n_rules"]) == [3, 3, 3, 0, 0, 0, 1]
    assert tab["kind"].dtype == np.int32 and tab["eps"].dtype == np.float32 and tab["rule_op"].shape == (7, 8)
    assert list(tab["eps"][[0, 5]]) == [np.float32(1e-4)] * 2 and list(tab["log_eps"][[0, 5]]) == [np.float32(-4.0)] * 2
    assert list(tab["rule_op"][0, :3]) == [0, 1, 3] and list(tab["rule_fill"][1, :3]) == [np.float32(-1.0), np.float32(1e-4), np.float32(0.0)]
    assert list(tab["rule_op"][6, :1]) == [0] and tab["rule_fill"][6, 0] == 0.0
    t64 = X.compile_channel_table([X.LogTransform([Q], eps=1e-8)], example(), KEYS, LEVELS, dtype=np.float64)
    assert t64["eps"][0] == 1e-8 and t64["log_eps"][0] == math.log(1e-8) and float(tab["eps"][0]) != 1e-4   # float32 rounds, float64 does not


def test_stacked_fill_blocks_compose_exactly():
    """Block 2 sees block 1's OUTPUT; the kernel looks at the original value only.  The composed list must give block2(block1(x)) for
    every class of value -- checked by brute force against the two blocks applied one after the other."""
    f = np.float32
    b1 = X.FillValues([{"search": "nan", "fill": 0.0}, {"search": 5.0, "op": ">", "fill": 7.0}, {"search": -1.0, "op": "<=", "fill": float("nan")}]).compiled_rules()
    b2 = X.FillValues([{"search": 0.0, "op": "==", "fill": 0.5}, {"search": "nan", "fill": -3.0}, {"search": 6.0, "op": ">=", "fill": 1.0},
                       {"search": 2.0, "op": "!=", "fill": 9.0}]).compiled_rules()
    both = X.compose_fill_rules(b1, b2)
    assert len(both) == 7
    for x in (f("nan"), f(0.0), f(-0.0), f(-1.0), f(-2.0), f(2.0), f(3.0), f(5.0), f(5.5), f(6.0), f(100.0), f(-0.5)):
        want, got = X.apply_fill_rules(b2, X.apply_fill_rules(b1, x)), X.apply_fill_rules(both, x)
        assert (np.isnan(want) and np.isnan(got)) or want == got, (x, want, got)
    b3 = X.FillValues([{"search": 9.0, "fill": -9.0}, {"search": 0.5, "op": "<", "fill": 0.25}]).compiled_rules()
    three = X.compose_fill_rules(both, b3)
    for x in (f("nan"), f(0.0), f(-1.0), f(2.0), f(3.0), f(5.5), f(6.0), f(0.3)):
        want = X.apply_fill_rules(b3, X.apply_fill_rules(b2, X.apply_fill_rules(b1, x)))
        got = X.apply_fill_rules(three, x)
        assert (np.isnan(want) and np.isnan(got)) or want == got, (x, want, got)


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_no_gpu_fails_loudly_at_construction():
    from wxengine.engine import WXEngineError
    from wxengine.preblock import DevicePreblock
    for make in (lambda: X.ExpTransform([Q]), lambda: X.SquareTransform([Q]), lambda: X.InverseTransforms({}, {}),
                 lambda: DevicePreblock(example(), transforms=[X.LogTransform([Q])])):
        with pytest.raises(WXEngineError):
            make()
