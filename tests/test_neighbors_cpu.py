"""Neighbour-list entry points (rsasa_precompute_neighbors*, reference src/lib.rs:69-84) as seen without a GPU: exported,
bound, their record layout, the new status and the loud failure on a GPU-less host; and the plain model of the lists
(neighbor_model.py) pinned to the oracle, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import nb_helpers as nh
import neighbor_model as nm
import tie_cases as tc


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


# ---- the plain model (tests/neighbor_model.py) pinned to the oracle, byte for byte -------------------------------

def _pin(x, y, z, r, ids, probe, max_radius=None):
    """The model's lists equal the oracle's (re-sorted by (d^2, idx)); returns them."""
    want = nh.oracle_csr(x, y, z, r, ids, probe, max_radius)
    got = nm.neighbor_csr(x, y, z, r, ids, probe, max_radius)
    nh.assert_same(got, want)
    return got


@pytest.mark.parametrize("name", ["1jcd.pdb", "151L_H3.pdb", "bad_seqadv_1A06.pdb", "example.cif"])
@pytest.mark.parametrize("probe", [1.4, 0.0, 3.0])
def test_model_matches_oracle_on_fixtures(name, probe):
    _pin(*nh.protor(name), probe)


def test_model_matches_oracle_on_tie_case_cutoffs_and_folds():
    fam = tc.generate()
    n = 0
    for case in fam["cutoff"] + fam["fold"]:
        for st in case.structures:
            _pin(*st.soa(), case.probe)
            n += 1
    assert n > 300


def test_model_matches_oracle_at_exact_max_search_cutoffs():
    """tie_cases.ms_cutoffs: d^2 == max_search^2 exactly with max_radius below r_0; the model lists atom 1 for atom 0
    at the flip and one f32 step above it, not below."""
    cases = tc.ms_cutoffs()
    assert len(cases) >= 20
    for c in cases:
        for mr, listed in [(v, True) for v in c.inside] + [(v, False) for v in c.outside]:
            offs, ent = _pin(*c.st.soa(), c.probe, mr)
            assert (1 in ent["idx"][int(offs[0]):int(offs[1])].tolist()) == listed
        x, y, z = c.st.x, c.st.y, c.st.z
        d = [np.float32(x[0] - x[1]), np.float32(y[0] - y[1]), np.float32(z[0] - z[1])]
        ms = np.float32(c.m_in) + np.float32(c.m_in) + np.float32(2.0) * np.float32(c.probe)
        assert d[0] * d[0] + d[1] * d[1] + d[2] * d[2] == ms * ms


@pytest.mark.parametrize("n, shared", [(513, False), (770, False), (1100, True)])
def test_model_matches_oracle_on_tight_clusters(n, shared):
    cols, c0 = nh.tight_cluster(n, seed=n, shared_ids=shared)
    offs, _ = _pin(*cols, 1.4)
    k = np.diff(offs.astype(np.int64))[c0:]
    if shared:
        assert k.min() == n - n // 3 and k.max() == n - 1
    else:
        assert np.all(k == n - 1)


@pytest.mark.parametrize("max_radius", [1.2, -0.5, 10.0, 1e30])
def test_model_matches_oracle_for_max_radius_overrides(max_radius):
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    _pin(x, y, z, r, ids, 1.4, max_radius)


def test_model_fold_max_skips_nan_and_nan_means_none():
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    r = r.copy()
    r[17] = np.nan
    want = _pin(x, y, z, r, ids, 1.4)
    nh.assert_same(nm.neighbor_csr(x, y, z, r, ids, 1.4, float("nan")), want)
    nh.assert_same(nm.neighbor_csr(x, y, z, r, ids, 1.4, float(nm.fold_max(r))), want)


@pytest.mark.parametrize("max_radius", [-1.4, -2.0, float("inf"), float("-inf")])
def test_model_rejects_invalid_max_radius(max_radius):
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    with pytest.raises(ValueError):
        nm.neighbor_csr(x, y, z, r, ids, 1.4, max_radius)
