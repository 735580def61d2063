"""bench.py --dump-outputs without a GPU: what lands in DIR/<name>.npy for small and for large arrays."""
import numpy as np
import torch


def test_dump_outputs_writes_small_arrays_whole_and_a_fixed_sample_of_large_ones(tmp_path):
    import bench
    n = 3 * bench.DUMP_MAX_ELEMS + 5
    big = torch.arange(n, dtype=torch.float32)          # value = flat index (exact in float32 below 2**24)
    small = torch.randn(2, 3, 4, dtype=torch.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_MAX_ELEMS,)
    np.testing.assert_array_equal(a, b)                  # the same sample every time
    assert (np.diff(a) > 0).all() and a[0] >= 0 and a[-1] < n   # sorted, distinct, in range
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (2, 3, 4)
    np.testing.assert_array_equal(s, small.float().numpy())
    assert 3 * a.nbytes <= 64 << 20                      # the most arrays one dump writes (--latband: y, y_phys, x_next)
