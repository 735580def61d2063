"""credit/preblock/regrid.py::Regridder restated in float64 numpy, from its formulas: the test-side truth of the regridding block.

    W = coalesce(sparse(row - 1, col - 1, float32(S)))        regrid.py:55-57, :107-109, :123-128
    x -> flip(x, the flips inside the spatial dimensions)     :139-163
    y[p, r] = sum_j W[r, j] x[p, j]                           :166-167
    y -> [..., ny, nx] or [..., n_b]                          :170-175

`regrid` also returns what the gate of the device result is made of: mag[p, r] = sum over the STORED entries of |float32(S) x| and
k[r], the number of stored entries of row r (before repeated pairs are merged).  Nothing is multiplied that the row does not
reference: a NaN source point reaches exactly the rows that name it."""
import numpy as np


def dst_shape(dst_grid_dims, xc_b, yc_b, reshape_to_xy):
    """regrid.py:60-71."""
    raw = np.asarray(dst_grid_dims).reshape(-1)
    if len(raw) == 2:
        return tuple(int(s) for s in raw[::-1])
    if reshape_to_xy:
        return (np.unique(yc_b).size, np.unique(xc_b).size)
    return None


def dst_grid(shape, xc_b, yc_b):
    """regrid.py:79-89 -> (grid type, dst_lat, dst_lon)."""
    if shape is None or xc_b is None or yc_b is None:
        return None, None, None
    lat2d, lon2d = np.asarray(yc_b).reshape(shape), np.asarray(xc_b).reshape(shape)
    if np.allclose(lat2d, lat2d[:, :1]) and np.allclose(lon2d, lon2d[:1, :]):
        return "rectilinear", lat2d[:, 0], lon2d[0, :]
    return "curvilinear", lat2d, lon2d


def dense_matrix(row, col, S, n_a, n_b):
    """The coalesced matrix, dense float64 [n_b, n_a], from float32 weights."""
    W = np.zeros((n_b, n_a), dtype=np.float64)
    np.add.at(W, (np.asarray(row, np.int64) - 1, np.asarray(col, np.int64) - 1), np.asarray(S).astype(np.float32).astype(np.float64))
    return W


def spatial_dims(shape, n_a):
    if shape[-1] == n_a:
        return 1
    if len(shape) >= 2 and shape[-2] * shape[-1] == n_a:
        return 2
    raise ValueError(f"Cannot map input shape {tuple(shape)} to expected source grid size {n_a}.")


def regrid(x, row, col, S, n_a, n_b, shape=None, flip_axis=None):
    """x [..., n_a] or [..., H, W] -> (y float64 [..., *shape] or [..., n_b], mag [planes, n_b], k [n_b])."""
    x = np.asarray(x, dtype=np.float64)
    sd = spatial_dims(x.shape, n_a)
    lead = x.shape[:-sd]
    flips = [d for d in (flip_axis or []) if -sd <= d < 0]
    if flips:
        x = np.flip(x, axis=tuple(flips))
    xf = x.reshape(-1, n_a)
    r, c = np.asarray(row, np.int64) - 1, np.asarray(col, np.int64) - 1
    w = np.asarray(S).astype(np.float32).astype(np.float64)
    terms = w[:, None] * xf.T[c]                      # [entries, planes]
    y = np.zeros((n_b, xf.shape[0]))
    mag = np.zeros((n_b, xf.shape[0]))
    np.add.at(y, r, terms)
    np.add.at(mag, r, np.abs(terms))
    k = np.bincount(r, minlength=n_b)
    return y.T.reshape(lead + (tuple(shape) if shape is not None else (n_b,))), mag.T, k
