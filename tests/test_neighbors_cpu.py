"""Neighbour-list entry points (rsasa_precompute_neighbors*, reference src/lib.rs:69-84) as seen without a GPU: exported,
bound, their record layout, the new status and the loud failure on a GPU-less host."""
import ctypes as C

import numpy as np
import pytest


def test_neighbor_symbols_exported_and_bound():
    from rustsasa_amd import _capi
    lib = _capi.load()
    for name in ("rsasa_precompute_neighbors", "rsasa_precompute_neighbors_batch"):
        assert hasattr(lib, name)
        assert name in _capi.SYMBOLS


def test_neighbor_dtype_is_neighbordata():
    from rustsasa_amd import NEIGHBOR_DTYPE
    assert NEIGHBOR_DTYPE.itemsize == 8
    assert NEIGHBOR_DTYPE.fields["threshold_squared"][1] == 0
    assert NEIGHBOR_DTYPE.fields["idx"][1] == 4
    assert NEIGHBOR_DTYPE["idx"] == np.dtype("<u4")


def test_buffer_too_small_has_a_status_string():
    from rustsasa_amd import _capi
    assert _capi.RSASA_ERR_BUFFER_TOO_SMALL == -8
    s = _capi.status_string(_capi.RSASA_ERR_BUFFER_TOO_SMALL)
    assert s != "unknown status" and "small" in s


def test_no_gpu_neighbors_fail_loudly():
    import rustsasa_amd
    from rustsasa_amd import _capi
    if rustsasa_amd.device_count() > 0:
        pytest.skip("a GPU is visible; the loud-failure path is for GPU-less hosts")
    x = np.zeros(3, np.float32)
    offsets = np.zeros(4, np.uint64)
    entries = np.zeros(16, _capi.NEIGHBOR_DTYPE)
    rc = _capi.load().rsasa_precompute_neighbors(None, x.ctypes.data, x.ctypes.data, x.ctypes.data, x.ctypes.data,
                                                 None, 3, None, 0, 1.4, float("nan"), offsets.ctypes.data,
                                                 entries.ctypes.data, 16)
    assert rc == _capi.RSASA_ERR_NO_DEVICE
    so = np.array([0, 3], np.uint32)
    rc = _capi.load().rsasa_precompute_neighbors_batch(None, x.ctypes.data, x.ctypes.data, x.ctypes.data, x.ctypes.data,
                                                       None, so.ctypes.data, 1, 1.4, float("nan"), offsets.ctypes.data,
                                                       entries.ctypes.data, 16)
    assert rc == _capi.RSASA_ERR_NO_DEVICE
