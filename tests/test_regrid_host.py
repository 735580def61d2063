"""Host side of the regridding block (wxengine/regrid.py) without a GPU: coalesce_weights and fold_flips against the oracle's dense
matrix, the shape and attribute rules, every error text, the untouched caller's dict, and the refusal to construct without a GPU."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import regrid_oracle as RO  # noqa: E402
from regrid_cases import REGRID_CASES, block_args, case_inputs, key_of, row_lengths, weights  # noqa: E402

from wxengine import regrid as R  # noqa: E402
from wxengine.engine import WXEngineError  # noqa: E402


def dense_of(row_ptr, col, val, n_a):
    W = np.zeros((row_ptr.size - 1, n_a))
    for r in range(row_ptr.size - 1):
        W[r, col[row_ptr[r]:row_ptr[r + 1]]] = val[row_ptr[r]:row_ptr[r + 1]]
    return W


@pytest.mark.parametrize("name", list(REGRID_CASES))
def test_coalesce_weights_against_the_dense_matrix(name):
    w = weights(name)
    row_ptr, col, val = R.coalesce_weights(w["row"], w["col"], w["S"], w["n_a"], w["n_b"])
    assert row_ptr.dtype == np.int64 and col.dtype == np.int32 and val.dtype == np.float32
    stored, coal = row_lengths(name)
    assert row_ptr[0] == 0 and np.array_equal(np.diff(row_ptr), coal) and col.size == val.size == row_ptr[-1]
    for r in range(w["n_b"]):
        assert (np.diff(col[row_ptr[r]:row_ptr[r + 1]]) > 0).all(), f"row {r}: columns not strictly increasing"
    want = RO.dense_matrix(w["row"], w["col"], w["S"], w["n_a"], w["n_b"])
    got = dense_of(row_ptr, col, val, w["n_a"])
    assert np.array_equal(got != 0, want != 0)
    absw = np.zeros_like(want)
    np.add.at(absw, (w["row"].astype(np.int64) - 1, w["col"].astype(np.int64) - 1), np.abs(w["S"].astype(np.float32)).astype(np.float64))
    merged = (stored > coal)
    assert np.array_equal(got[~merged], want[~merged])                       # nothing merged: the float32 weights themselves
    assert (np.abs(got - want) <= 2.0 * 2.0 ** -24 * absw).all()            # a merged pair or triple: at most two float32 additions
    assert merged.any() == (name == "ragged")


def test_coalesce_weights_sums_repeated_pairs_in_float32_in_stored_order():
    row = np.array([2, 1, 2, 2, 1, 2])
    col = np.array([3, 1, 3, 1, 1, 3])
    S = np.array([1.0, 0.1, 2.0 ** -24, 5.0, 0.2, 2.0 ** -24])
    row_ptr, c, v = R.coalesce_weights(row, col, S, 4, 3)
    assert row_ptr.tolist() == [0, 1, 3, 3] and c.tolist() == [0, 0, 2]
    f = np.float32
    assert v[0] == f(0.1) + f(0.2) and v[1] == f(5.0)
    assert v[2] == f(1.0)                     # (1 + 2^-24) + 2^-24 in float32, in stored order: both halves of an ulp are lost
    _, _, v2 = R.coalesce_weights(row[::-1], col[::-1], S[::-1], 4, 3)
    assert v2[2] == f(1.0) + f(2.0 ** -23)    # the other order keeps them
    # the cast to float32 comes first
    _, _, v3 = R.coalesce_weights([1, 1], [1, 1], [1.0 + 2.0 ** -30, -1.0], 1, 1)
    assert v3[0] == 0.0


def test_coalesce_weights_refuses_indices_outside_their_grids():
    ok = dict(row=[1, 2], col=[1, 3], S=[1.0, 1.0], n_a=3, n_b=2)
    R.coalesce_weights(**ok)
    with pytest.raises(ValueError, match=r"row index 3 lies outside the destination grid 1 \.\. n_b = 2"):
        R.coalesce_weights(**dict(ok, row=[1, 3]))
    with pytest.raises(ValueError, match=r"row index 0 lies outside the destination grid"):
        R.coalesce_weights(**dict(ok, row=[0, 1]))
    with pytest.raises(ValueError, match=r"col index 4 lies outside the source grid 1 \.\. n_a = 3"):
        R.coalesce_weights(**dict(ok, col=[1, 4]))
    with pytest.raises(ValueError, match=r"col index 0 lies outside the source grid"):
        R.coalesce_weights(**dict(ok, col=[0, 1]))
    with pytest.raises(ValueError, match="must have one length"):
        R.coalesce_weights(**dict(ok, S=[1.0]))
    with pytest.raises(ValueError, match=r"n_a and n_b must be 1 \.\. 2\^31 - 1"):
        R.coalesce_weights(**dict(ok, n_a=2 ** 31))
    rp, c, v = R.coalesce_weights([], [], [], 3, 2)
    assert rp.tolist() == [0, 0, 0] and c.size == 0 and v.size == 0


@pytest.mark.parametrize("flips", [(-1,), (-2,), (-1, -2), (-2, -1)])
def test_fold_flips_equals_an_explicit_flip(flips):
    w = weights("bilin")
    shape = REGRID_CASES["bilin"]["src"]
    row_ptr, col, val = R.coalesce_weights(w["row"], w["col"], w["S"], w["n_a"], w["n_b"])
    folded = R.fold_flips(col, shape, flips)
    assert folded.dtype == col.dtype and folded.shape == col.shape and not np.array_equal(folded, col)
    W, Wf = dense_of(row_ptr, col, val, w["n_a"]), dense_of(row_ptr, folded, val, w["n_a"])
    perm = np.flip(np.arange(w["n_a"]).reshape(shape), axis=flips).ravel()      # flip(x).ravel() = x.ravel()[perm]
    assert np.array_equal(Wf[:, perm], W)
    x = case_inputs("bilin")["a"].astype(np.float64)
    ya, yb = np.flip(x, axis=flips).reshape(3, -1) @ W.T, x.reshape(3, -1) @ Wf.T
    assert np.abs(ya - yb).max() <= 1e-12 * np.abs(ya).max()
    assert np.array_equal(R.fold_flips(folded, shape, flips), col)               # an involution
    y, _, _ = RO.regrid(x, w["row"], w["col"], w["S"], w["n_a"], w["n_b"], None, list(flips))
    assert np.abs(y - x.reshape(3, -1) @ Wf.T).max() <= 1e-12 * np.abs(y).max()


def test_fold_flips_flat_and_refusals():
    col = np.array([0, 3, 5], dtype=np.int32)
    assert R.fold_flips(col, (6,), [-1]).tolist() == [5, 2, 0]
    assert R.fold_flips(col, (2, 3), []).tolist() == [0, 3, 5]
    assert R.fold_flips(col, (2, 3), [-1, -1]).tolist() == [2, 5, 3]
    for bad in ([0], [1], [-3], [-2, 2]):
        with pytest.raises(ValueError, match="negative axis numbers"):
            R.fold_flips(col, (2, 3), bad)


@pytest.fixture
def host(monkeypatch):
    """Lets the constructor pass on a machine without a GPU; no device call is ever reached in these tests."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(R, "load_library", lambda: None)


def test_shape_and_attribute_rules(host):
    blk = R.Regridder(**block_args("block"))
    assert tuple(blk.dst_shape) == (6, 10) and blk.n_a == 240 and blk.n_b == 60 and blk.data_types == ["input", "target"]
    assert blk.dst_grid_type == "rectilinear" and blk.dst_lat.shape == (6,) and blk.dst_lon.shape == (10,)
    assert isinstance(blk.dst_lat, np.ndarray) and blk.reshape_to_xy is True and blk.flip_axis is None
    u = R.Regridder(**block_args("uniq"))
    w = weights("uniq")
    assert tuple(u.dst_shape) == (4, 5) and u.dst_grid_type == "rectilinear"
    assert np.array_equal(u.dst_lat, w["yc_b"].reshape(4, 5)[:, 0]) and np.array_equal(u.dst_lon, w["xc_b"][:5])
    uc = R.Regridder(**block_args("uniq", curvilinear=True))
    assert tuple(uc.dst_shape) == (4, 5) and uc.dst_grid_type == "curvilinear" and uc.dst_lat.shape == uc.dst_lon.shape == (4, 5)
    assert np.array_equal(uc.dst_lon, w["xc_b_curv"].reshape(4, 5))
    rg = R.Regridder(**block_args("ragged"))
    assert rg.dst_shape is None and rg.dst_grid_type is None and rg.dst_lat is None and rg.dst_lon is None
    # a length-2 dst_grid_dims is reversed whatever reshape_to_xy says, and the attributes follow
    nb = R.Regridder(**dict(block_args("block"), reshape_to_xy=False))
    assert tuple(nb.dst_shape) == (6, 10) and nb.dst_grid_type == "rectilinear"
    # no coordinates: no attributes
    nc = R.Regridder(**dict(block_args("block"), xc_b=None, yc_b=None))
    assert tuple(nc.dst_shape) == (6, 10) and nc.dst_grid_type is None and nc.dst_lat is None
    for name in REGRID_CASES:
        for tag in ("rect", "curv") if name == "uniq" else ("rect",):
            b = R.Regridder(**block_args(name, curvilinear=tag == "curv"))
            g = np.load(os.path.join(os.path.dirname(__file__), "golden", f"regrid_{name}.npz"))
            assert str(b.dst_grid_type) == str(g[f"grid_type:{tag}"])
            if b.dst_grid_type is not None:
                assert np.array_equal(b.dst_lat, g[f"dst_lat:{tag}"]) and np.array_equal(b.dst_lon, g[f"dst_lon:{tag}"])


def test_constructor_error_texts(host):
    a = block_args("block")
    with pytest.raises(ValueError, match=r"Invalid data_types \{'metadata'\}\. Valid options are \('input', 'target'\)\."):
        R.Regridder(**dict(a, data_types=["input", "metadata"]))
    with pytest.raises(ValueError, match="variables is required"):
        R.Regridder(**dict(a, variables="GFS/prognostic/2d/hw"))
    with pytest.raises(ValueError, match="row, col, S, n_a and n_b are required"):
        R.Regridder(**dict(a, S=None))
    with pytest.raises(ValueError, match="needs xc_b and yc_b"):
        R.Regridder(**dict(block_args("uniq"), xc_b=None))
    with pytest.raises(ValueError, match=r"destination shape \(6, 10\) does not hold n_b = 61 points"):
        R.Regridder(**dict(a, n_b=61))
    with pytest.raises(ValueError, match="col index 241 lies outside the source grid"):
        R.Regridder(**dict(a, col=np.where(a["col"] == 1, 241, a["col"])))


def test_call_error_texts_warning_and_untouched_dict(host, caplog):
    a = block_args("block")
    blk = R.Regridder(**a)
    k_hw, k_7 = key_of("hw"), key_of("l7")
    other = torch.zeros(3)
    inner = {"GFS/prognostic/2d/other": other}
    batch = {"input": {"GFS": inner}, "metadata": {"datetime": [1, 2]}}
    out = blk(batch)                     # no listed variable present, no "target": nothing to do, and nothing shared but the tensors
    assert out is not batch and out["input"] is not batch["input"] and out["input"]["GFS"] is not inner
    assert out["input"]["GFS"]["GFS/prognostic/2d/other"] is other and out["metadata"] == batch["metadata"]
    assert list(batch) == ["input", "metadata"] and list(inner) == ["GFS/prognostic/2d/other"]
    with pytest.raises(KeyError, match=r"Regridder: source 'GFS' not found in batch\['input'\]\."):
        blk({"input": {"ERA5": {}}})
    with pytest.raises(KeyError, match=r"not found in batch\['target'\]"):
        blk({"input": {"GFS": {}}, "target": {"ERA5": {}}})
    bad = {"input": {"GFS": {k_hw: torch.zeros(12, 21)}}}
    with pytest.raises(ValueError, match=r"Cannot map input shape torch\.Size\(\[12, 21\]\) to expected source grid size 240\."):
        blk(bad)
    assert list(bad["input"]["GFS"]) == [k_hw] and bad["input"]["GFS"][k_hw].shape == (12, 21)
    # a CPU tensor is refused (no fallback), after the layout is known
    with pytest.raises(WXEngineError, match="must be a float32 tensor on the GPU"):
        blk({"input": {"GFS": {k_7: torch.zeros(7, 12, 20)}}})
    # the flip warning, in the reference's words, for the flips outside the spatial dimensions
    fl = R.Regridder(**dict(a, flip_axis=[2, -1]))
    with caplog.at_level(logging.WARNING, logger="wxengine.regrid"):
        with pytest.raises(WXEngineError):
            fl({"input": {"GFS": {k_7: torch.zeros(7, 12, 20)}}})
    assert "Regridder: ignoring invalid flip_axis values [2]; spatial axes must be negative indices in [-2, -1]." in caplog.text
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="wxengine.regrid"):
        with pytest.raises(WXEngineError):
            R.Regridder(**dict(a, flip_axis=[-2]))({"input": {"GFS": {k_7: torch.zeros(7, 240)}}})
    assert "ignoring invalid flip_axis values [-2]; spatial axes must be negative indices in [-1, -1]." in caplog.text
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="wxengine.regrid"):
        with pytest.raises(WXEngineError):
            R.Regridder(**dict(a, flip_axis=[-1, -2]))({"input": {"GFS": {k_7: torch.zeros(7, 12, 20)}}})
    assert "ignoring" not in caplog.text


def test_layout_detection_prefers_the_flat_reading(host):
    """regrid.py:140-145: a last dimension equal to n_a wins over a product of the last two."""
    w = weights("uniq")
    blk = R.Regridder(**block_args("uniq"))
    x = torch.zeros(1, 60)        # also 1 * 60 = n_a
    with pytest.raises(WXEngineError, match="on the GPU"):
        blk._plan("x", x)
    assert RO.spatial_dims((1, 60), w["n_a"]) == 1 and RO.spatial_dims((6, 10), w["n_a"]) == 2


def test_plane_count_of_a_variable_is_bounded(host):
    """The ABI takes the plane count as a 32-bit int: 2^31 planes are refused on the host (an expanded tensor: no memory behind it)."""
    blk = R.Regridder(variables=["GFS/prognostic/2d/x"], row=[1], col=[1], S=[1.0], n_a=1, n_b=1, dst_grid_dims=[1, 1])
    with pytest.raises(WXEngineError, match=r"holds 2147483648 planes; one variable takes 1 \.\. 2\^31 - 1"):
        blk._plan("x", torch.zeros(1, 1).expand(2 ** 31, 1))
    with pytest.raises(WXEngineError, match="holds 0 planes"):
        blk._plan("x", torch.zeros(0, 1))
    with pytest.raises(WXEngineError, match="on the GPU"):
        blk._plan("x", torch.zeros(1, 1).expand(2 ** 31 - 1, 1))


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_construction_raises_without_a_gpu():
    with pytest.raises(WXEngineError, match="no GPU visible: the regridding block has no CPU fallback"):
        R.Regridder(**block_args("block"))


def test_lazy_export():
    import wxengine
    assert wxengine.Regridder is R.Regridder and wxengine.coalesce_weights is R.coalesce_weights and wxengine.fold_flips is R.fold_flips
    assert R.MAX_VARIABLES == 32
