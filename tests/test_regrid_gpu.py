"""The regridding block on the device (csrc/wx_regrid.h, wxengine/regrid.py) against the fixtures of the reference's own class.

Gate, per element and derived, not measured: |y_dev - y64| <= (k[r] + 2) 2^-24 mag[p, r] with mag = sum |float32(S) x| over the stored
entries of row r and k[r] their number (regrid_cases.bound): the running-error bound of a length-k float32 sum in any order, product
roundings and merged repeated pairs included.  The reference's own float32 output meets it (asserted by the generator; worst 0.42).
Every element is compared; rows without entries are exactly 0.0; for `nan` the NaN mask equals the golden's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import regrid_oracle as RO  # noqa: E402
from regrid_cases import (REGRID_CASES, SRC, block_args, bound, case_inputs, key_of, load_golden, out_shape, run_input, variables,  # noqa: E402
                          weights)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
_cache = {}


def fixture_of(name):
    """-> (inputs, fp32 goldens, fp64 goldens), loaded and hash-checked once."""
    if name not in _cache:
        g, f32, f64 = load_golden(name, GOLD)
        _cache[name] = (case_inputs(name, check=g), f32, f64)
    return _cache[name]


def gate_of(name, run, v):
    """-> (mag [planes, n_b], k [n_b]) of a run's variable, computed once."""
    if (name, run, v) not in _cache:
        w = weights(name)
        _, mag, k = RO.regrid(run_input(name, run, fixture_of(name)[0][v]), w["row"], w["col"], w["S"], w["n_a"], w["n_b"], None,
                              REGRID_CASES[name]["runs"][run]["flip_axis"])
        _cache[(name, run, v)] = (mag, k)
    return _cache[(name, run, v)]


def check_against_golden(name, run, v, got, report):
    """Every element of `got` (numpy float32) against the fp64 golden under the gate.  -> the worst error / gate ratio."""
    w = weights(name)
    _, _, f64 = fixture_of(name)
    want = f64[(run, v)]
    mag, k = gate_of(name, run, v)
    assert got.dtype == np.float32 and got.shape == want.shape == out_shape(name, REGRID_CASES[name]["vars"][v]), (name, run, v, got.shape)
    g2, w2 = got.reshape(-1, w["n_b"]).astype(np.float64), want.reshape(-1, w["n_b"])
    bad = np.isnan(w2)
    assert np.array_equal(np.isnan(g2), bad), (name, run, v, "NaN mask differs from the golden's")
    assert bad.any() == bool(REGRID_CASES[name].get("nan"))
    err = np.where(bad, 0.0, np.abs(g2 - w2))
    gate = np.where(bad, 0.0, bound(k, np.where(bad, 0.0, mag)))
    ratio = float((err[gate > 0] / gate[gate > 0]).max())
    report.append(f"{name}/{run}/{v}: worst error / gate {ratio:.3f}")
    print(report[-1])
    assert (err <= gate).all(), (name, run, v, ratio)
    assert err.size == got.size and (g2[:, k == 0] == 0.0).all() and not np.signbit(g2[:, k == 0]).any()
    return ratio


def device_inputs(name, run):
    """-> ({var_key: GPU tensor}, {var_key: bit copy for the unchanged check}); `b2` is a channel slice of a wider tensor."""
    inp, _, _ = fixture_of(name)
    xs = {}
    for v in inp:
        x = torch.from_numpy(run_input(name, run, inp[v])).cuda()
        if v == "b2":
            wide = torch.full((2, 5) + tuple(x.shape[2:]), float("nan"), device="cuda")
            wide[:, 1:4] = x
            x = wide[:, 1:4]
            assert not x.is_contiguous() and x[0].is_contiguous()
        xs[key_of(v)] = x
    return xs, {k: x.clone() for k, x in xs.items()}


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", list(REGRID_CASES))
def test_every_case_and_shape_through_the_block(name):
    from wxengine.regrid import Regridder
    report = []
    for run in REGRID_CASES[name]["runs"]:
        blk = Regridder(**block_args(name, run))
        xs, keep = device_inputs(name, run)
        first = next(iter(xs))
        inner = dict(xs)
        batch = {"input": {SRC: inner}, "target": {SRC: {first: xs[first]}}}
        out = blk(batch)
        torch.cuda.synchronize()
        assert batch["input"][SRC] is inner and all(inner[k] is xs[k] for k in xs) and list(batch["target"][SRC]) == [first]
        for k in xs:
            assert same_bits(xs[k], keep[k]), f"{k}: the source was written"
        for v in variables(name):
            y = out["input"][SRC][key_of(v)]
            assert y.is_contiguous() and y.dtype == torch.float32 and y.is_cuda
            check_against_golden(name, run, v, y.cpu().numpy(), report)
        assert same_bits(out["target"][SRC][first], out["input"][SRC][first])
        assert len(blk._handles) == 1


def test_groupings_give_the_same_bits():
    """A plane alone equals the same plane inside a group of 7 or 12, on short rows (block) and on long and empty rows (ragged); a
    variable alone equals the same variable among three."""
    from wxengine.regrid import Regridder
    blk = Regridder(**block_args("block"))
    xs, _ = device_inputs("block", "plain")
    three = {key_of(v): xs[key_of(v)] for v in ("l111", "l7", "l232")}          # 1, 7 and 12 planes in one call
    together = blk({"input": {SRC: dict(three)}})["input"][SRC]
    for k, x in three.items():
        alone = blk({"input": {SRC: {k: x}}})["input"][SRC][k]
        assert same_bits(alone, together[k]), k
        planes_in, planes_out = x.reshape(-1, 12, 20), together[k].reshape(-1, 6, 10)
        assert planes_in.shape[0] in (1, 7, 12)
        for p in range(planes_in.shape[0]):
            one = blk._regrid(planes_in[p].contiguous())
            assert one.shape == (6, 10) and same_bits(one, planes_out[p]), (k, p)
    rg = Regridder(**block_args("ragged"))
    x = device_inputs("ragged", "plain")[0][key_of("a")]
    y = rg._regrid(x)
    for p in range(5):
        assert same_bits(rg._regrid(x[p].contiguous()), y[p]), p
    y12 = rg._regrid(torch.cat([x, x, x[:2]]))                                    # 12 planes: a full group and a tail of 4
    assert same_bits(y12[:5], y) and same_bits(y12[5:10], y) and same_bits(y12[10:], y[:2])
    torch.cuda.synchronize()


def test_flips_flat_input_and_the_cached_handle():
    from wxengine.regrid import Regridder
    x = device_inputs("bilin", "plain")[0][key_of("a")]
    plain = Regridder(**block_args("bilin"))
    y = plain._regrid(x)
    again = plain._regrid(x)                                                       # the cached handle
    assert same_bits(y, again) and len(plain._handles) == 1
    flat = plain._regrid(x.reshape(3, -1))
    assert flat.shape == (3, 13, 23) and same_bits(flat, y) and len(plain._handles) == 2      # another spatial shape: another handle
    for run, dims in (("flip-1", [-1]), ("flip-2", [-2]), ("flip-1-2", [-1, -2])):
        folded = Regridder(**block_args("bilin", run))._regrid(x)
        assert same_bits(folded, plain._regrid(torch.flip(x, dims=dims))), run
        assert not same_bits(folded, y)
    for run in ("flip2", "flatflip-2"):                                            # ignored flips: the unflipped handle
        blk = Regridder(**block_args("bilin", run))
        assert same_bits(blk._regrid(run_input_t("bilin", run, x)), y), run
        assert list(blk._handles)[0][2] == ()
    torch.cuda.synchronize()


def run_input_t(name, run, x):
    return x.reshape(x.shape[:-2] + (-1,)) if REGRID_CASES[name]["runs"][run]["flat"] else x


def test_more_than_32_variables_go_in_chunks():
    from wxengine.regrid import Regridder
    inp, _, _ = fixture_of("block")
    base = torch.from_numpy(inp["l7"]).cuda()
    names = [f"{SRC}/prognostic/2d/v{i}" for i in range(35)]
    xs = {n: (base[i % 7] + float(i)).contiguous() for i, n in enumerate(names)}
    blk = Regridder(**dict(block_args("block"), variables=names))
    out = blk({"input": {SRC: dict(xs)}})["input"][SRC]
    for n in names:
        assert out[n].shape == (6, 10) and same_bits(out[n], blk._regrid(xs[n])), n
    torch.cuda.synchronize()


# ---- the raw ABI ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from wxengine.engine import load_library
    return load_library()


def csr_args(row_ptr, col, val):
    row_ptr, col, val = np.ascontiguousarray(row_ptr, np.int64), np.ascontiguousarray(col, np.int32), np.ascontiguousarray(val, np.float32)
    return (row_ptr.ctypes.data_as(C.POINTER(C.c_int64)), col.ctypes.data_as(C.POINTER(C.c_int32)), val.ctypes.data_as(C.POINTER(C.c_float)),
            (row_ptr, col, val))


def create(lib, n_a, n_b, row_ptr, col, val):
    rp, c, v, keep = csr_args(row_ptr, col, val)
    h = C.c_void_p()
    st = lib.wx_regrid_create(n_a, n_b, rp, c, v, 0, C.byref(h))
    return st, h, lib.wx_last_error().decode() if st else ""


def apply(lib, h, srcs, strides, ppis, batch, dsts):
    n = len(srcs)
    return lib.wx_regrid_apply(h, n, (C.c_void_p * n)(*[s.data_ptr() for s in srcs]), (C.c_int64 * n)(*strides), (C.c_int32 * n)(*ppis),
                               batch, (C.c_void_p * n)(*[d.data_ptr() for d in dsts]), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_abi_refusals(lib):
    rp, col, val = [0, 1, 3], [0, 1, 2], [1.0, 0.5, 0.5]
    st, h, _ = create(lib, 3, 2, rp, col, val)
    assert st == 0 and h.value
    for args, why in (((0, 2, rp, col, val), "n_a must be 1 .. 2^31 - 1, got 0"),
                      ((2 ** 31, 2, rp, col, val), "n_a must be 1 .. 2^31 - 1, got 2147483648"),
                      ((3, 0, rp, col, val), "n_b must be 1 .. 2^31 - 1, got 0"),
                      ((3, 2 ** 31, rp, col, val), "n_b must be 1 .. 2^31 - 1, got 2147483648"),
                      ((3, 2, [1, 1, 3], col, val), "row_ptr must start at 0, got 1"),
                      ((3, 2, [0, 2, 1], col, val), "row_ptr decreases at row 1"),
                      ((3, 1, [0, 2 ** 31], col, val), "the entry count must stay below 2^31, got 2147483648"),
                      ((3, 2, rp, [0, 1, 3], val), "column index 3 at entry 2 lies outside [0, n_a = 3)"),
                      ((3, 2, rp, [0, -1, 2], val), "column index -1 at entry 1 lies outside [0, n_a = 3)")):
        st, bad, msg = create(lib, *args)
        assert st == -1 and not bad.value and msg == "wx_regrid_create: " + why, (args[:2], msg)
    p_rp, p_col, p_val, keep = csr_args(rp, col, val)
    out = C.c_void_p()
    for a in ((None, p_col, p_val), (p_rp, None, p_val), (p_rp, p_col, None)):
        assert lib.wx_regrid_create(3, 2, *a, 0, C.byref(out)) == -1 and lib.wx_last_error() == b"wx_regrid_create: null weight array"
    assert lib.wx_regrid_create(3, 2, p_rp, p_col, p_val, 0, None) == -1 and lib.wx_last_error() == b"wx_regrid_create: null argument"
    assert lib.wx_regrid_create(3, 2, p_rp, p_col, p_val, 99, C.byref(out)) == -1 and b"no such GPU device" in lib.wx_last_error()

    x, y = torch.ones(2, 3, device="cuda"), torch.zeros(2, 2, device="cuda")
    assert apply(lib, None, [x], [0], [2], 1, [y]) == -1 and lib.wx_last_error() == b"wx_regrid_apply: null regridding handle"
    one = (C.c_void_p * 1)(x.data_ptr())
    i64, i32, dst = (C.c_int64 * 1)(0), (C.c_int32 * 1)(2), (C.c_void_p * 1)(y.data_ptr())
    for a in ((None, i64, i32, 1, dst), (one, None, i32, 1, dst), (one, i64, None, 1, dst), (one, i64, i32, 1, None)):
        assert lib.wx_regrid_apply(h, 1, *a, None) == -1 and lib.wx_last_error() == b"wx_regrid_apply: null argument"
    null = (C.c_void_p * 1)(None)
    assert lib.wx_regrid_apply(h, 1, null, i64, i32, 1, dst, None) == -1 and lib.wx_last_error() == b"wx_regrid_apply: null tensor pointer"
    assert lib.wx_regrid_apply(h, 1, one, i64, i32, 1, null, None) == -1 and lib.wx_last_error() == b"wx_regrid_apply: null tensor pointer"
    for n in (0, 33, -1):
        many = (C.c_void_p * 33)(*[x.data_ptr()] * 33)
        assert lib.wx_regrid_apply(h, n, many, (C.c_int64 * 33)(), (C.c_int32 * 33)(*[1] * 33), 1, many, None) == -1
        assert lib.wx_last_error() == b"wx_regrid_apply: 1..32 variables"
    assert apply(lib, h, [x], [0], [2], 0, [y]) == -1 and lib.wx_last_error() == b"wx_regrid_apply: batch must be >= 1"
    assert apply(lib, h, [x], [0], [0], 1, [y]) == -1 and lib.wx_last_error() == b"wx_regrid_apply: planes_per_item must be >= 1"
    assert apply(lib, h, [x], [-3], [1], 2, [y]) == -1 and lib.wx_last_error() == b"wx_regrid_apply: negative batch stride"
    assert apply(lib, h, [x], [0], [2 ** 30], 2, [y]) == -1 and b"exceeds 2^31 - 1 planes" in lib.wx_last_error()
    assert torch.equal(y, torch.zeros_like(y)) and torch.equal(x, torch.ones_like(x))           # a refused call touches nothing
    assert apply(lib, h, [x], [0], [2], 1, [y]) == 0
    torch.cuda.synchronize()
    assert y.tolist() == [[1.0, 1.0], [1.0, 1.0]]
    assert lib.wx_regrid_destroy(h) == 0 and lib.wx_regrid_destroy(None) == 0


def test_abi_writes_every_destination_element_and_nothing_else(lib):
    """`ragged` (empty rows, long rows, a partial last slice) through the raw ABI: two variables, one of them B = 2 as a channel slice;
    the destination buffers are pre-filled with NaN and lie between sentinels."""
    from wxengine.regrid import coalesce_weights
    w = weights("ragged")
    n_a, n_b = w["n_a"], w["n_b"]
    st, h, msg = create(lib, n_a, n_b, *coalesce_weights(w["row"], w["col"], w["S"], n_a, n_b))
    assert st == 0, msg
    inp = fixture_of("ragged")[0]["a"]                                             # [5, n_a]
    x0 = torch.from_numpy(inp).cuda()                                              # 5 planes, contiguous
    wide = torch.full((2, 4, n_a), float("nan"), device="cuda")
    wide[:, 1:3] = torch.from_numpy(inp[:4].reshape(2, 2, n_a)).cuda()
    x1 = wide[:, 1:3]                                                              # B = 2, 2 planes per item, batch stride 4 n_a
    keep0, keep_wide = x0.clone(), wide.clone()
    guard, fill = 64, -7777.25
    buf = torch.full((2 * guard + (5 + 4) * n_b,), fill, device="cuda")
    y0, y1 = buf[guard:guard + 5 * n_b], buf[guard + 5 * n_b:guard + 9 * n_b]
    y0.fill_(float("nan")), y1.fill_(float("nan"))
    # one call per batch count, as the host block makes them
    assert apply(lib, h, [x0], [0], [5], 1, [y0]) == 0, lib.wx_last_error()
    assert apply(lib, h, [x1], [x1.stride(0)], [2], 2, [y1]) == 0, lib.wx_last_error()
    torch.cuda.synchronize()
    assert (buf[:guard] == fill).all() and (buf[-guard:] == fill).all()
    assert same_bits(x0, keep0) and same_bits(wide, keep_wide)
    assert not torch.isnan(buf).any(), "a destination element was not written"
    report = []
    got = y0.reshape(5, n_b).cpu().numpy()
    check_against_golden("ragged", "plain", "a", got, report)
    assert np.array_equal(y1.reshape(4, n_b).cpu().numpy(), got[:4])              # the slice's planes: the same bits
    _, k = gate_of("ragged", "plain", "a")
    assert (k == 0).sum() == 2 and (got[:, k == 0] == 0.0).all()
    assert lib.wx_regrid_destroy(h) == 0


def test_more_plane_groups_than_one_grid_holds(lib):
    """65 537 plane groups: gridDim.y holds 65 535, so the call takes a second pair of launches.  A 2 x 2 matrix keeps it at 4 MB; its
    sums are exact in float32 up to one rounding, which torch makes in the same place."""
    st, h, msg = create(lib, 2, 2, [0, 2, 3], [0, 1, 1], [0.5, 0.5, 1.0])
    assert st == 0, msg
    planes = 65536 * 8 + 3
    x = torch.rand(planes, 2, device="cuda") * 100.0 - 50.0
    y = torch.full((planes, 2), float("nan"), device="cuda")
    assert apply(lib, h, [x], [0], [planes], 1, [y]) == 0, lib.wx_last_error()
    torch.cuda.synchronize()
    want = torch.stack([0.5 * x[:, 0] + 0.5 * x[:, 1], x[:, 1]], dim=1)
    assert same_bits(y, want)
    assert lib.wx_regrid_destroy(h) == 0
