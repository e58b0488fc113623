"""Contact-count entry points (rsasa_contact_points*) as seen without a GPU: exported and bound, the Python side's
argument checks (they raise before any C call), contact_areas on hand-made counts, and the exact CPU model of the
counts (contacts_model.py) pinned to the oracle - the yardstick the GPU tests compare with."""
import numpy as np
import pytest

import contacts_model as cm
import nb_helpers as nh
from oracle import pyoracle as po

# (fixture, probe, n_points) at W = 8: a point count with remainder points (97 = 12 * 8 + 1) and a second protein
CONFIGS = [("1jcd.pdb", 1.4, 100), ("1jcd.pdb", 1.4, 97), ("2drt.pdb", 1.2, 100)]
W = 8


def test_contact_symbols_exported_and_bound():
    from rustsasa_amd import _capi
    lib = _capi.load()
    for name in ("rsasa_contact_points", "rsasa_contact_points_batch"):
        assert hasattr(lib, name)
        assert name in _capi.SYMBOLS
        assert getattr(lib, name).argtypes == _capi.SYMBOLS[name][1]


class _NoCall:
    """Stands in for the library: any C call fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def _ctx():
    from rustsasa_amd import Context
    c = object.__new__(Context)
    c._lib = _NoCall()
    c._h = None
    return c


def test_argument_errors_raise_before_the_c_call():
    c = _ctx()
    x = np.zeros(5, np.float32)
    with pytest.raises(ValueError):
        c.contact_points(x, x, x[:4], x)                             # a short column
    with pytest.raises(ValueError):
        c.contact_points(x, x, x, x, ids=np.zeros(4, np.uint64))
    with pytest.raises(ValueError):
        c.contact_points(x.reshape(5, 1), x, x, x)                    # not 1-D
    for n in (0, -3, 2.5):
        with pytest.raises(ValueError):
            c.contact_points(x, x, x, x, n_points=n)
        with pytest.raises(ValueError):
            c.contact_points_batch(x, x, x, x, None, [0, 5], n_points=n)
    with pytest.raises(ValueError):
        c.contact_points_batch(x, x, x, x, None, [0, 2, 4])            # offsets cover 4 of 5 atoms
    with pytest.raises(ValueError):
        c.contact_points_batch(x, x, x, x, None, np.zeros((2, 2), np.uint32))


def test_contact_areas_expression_and_rows():
    from rustsasa_amd import contact_areas
    r = np.array([1.7, 1.52, 1.88], np.float32)
    offs = np.array([0, 2, 2, 5], np.uint64)                          # atom 1 has an empty list
    counts = np.array([0, 37, 100, 1, 99], np.uint32)
    for probe, n in ((1.4, 100), (1.2, 97), (3.0, 70000)):
        got = contact_areas(counts, offs, r, probe, n)
        assert got.dtype == np.float32 and got.shape == (5,)
        for e, i in enumerate([0, 0, 2, 2, 2]):
            R = np.float32(r[i]) + np.float32(probe)
            want = np.float32(np.float32(np.float32(np.float32(12.566371) * np.float32(R * R)) * np.float32(counts[e]))
                              * np.float32(np.float32(1.0) / np.float32(n)))
            assert got[e] == want
    # an area of every point of the lattice is the reference's value of an atom without neighbours
    x = np.array([0.0, 50.0], np.float32)
    z0 = np.zeros(2, np.float32)
    rr = np.array([1.5, 1.9], np.float32)
    full = contact_areas(np.array([100, 100], np.uint32), np.array([0, 1, 2], np.uint64), rr, 1.4, 100)
    assert full.tobytes() == po.calculate_sasa_internal(x, z0, z0, rr, None, 1.4, 100, 8).tobytes()
    with pytest.raises(ValueError):
        contact_areas(counts[:4], offs, r)                           # offsets[-1] = 5 counts
    with pytest.raises(ValueError):
        contact_areas(counts, offs[:3], r)                           # one offset per atom and the end
    with pytest.raises(ValueError):
        contact_areas(counts, np.array([0, 3, 2, 5], np.uint64), r)  # decreasing
    with pytest.raises(ValueError):
        contact_areas(counts, offs, r, n_points=0)


# ---- the model pinned to the oracle ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def models():
    out = {}
    for name, probe, n in CONFIGS:
        cols = nh.protor(name)
        out[(name, probe, n)] = (cols,) + cm.contact_counts(*cols, probe, n, W)
    return out


@pytest.mark.parametrize("name, probe, n_points", CONFIGS)
def test_model_exposed_counts_equal_oracle(models, name, probe, n_points):
    cols, offs, ent, cov, exc = models[(name, probe, n_points)]
    _, _, by_w = cm.contact_counts_ws(*cols, probe, n_points, (W,), lists=(offs, ent))
    buried = by_w[W][2]
    _, pts, _ = po.calculate_sasa_internal(*cols, probe, n_points, W, return_details=True)
    assert np.array_equal(n_points - buried, pts.astype(np.int64))
    # per atom: sum(exclusive) <= buried <= sum(covered), and no entry hides more than is buried
    n = len(cols[0])
    rows = np.repeat(np.arange(n), np.diff(offs.astype(np.int64)))
    s_cov, s_exc, m_cov = (np.zeros(n, np.int64) for _ in range(3))
    np.add.at(s_cov, rows, cov.astype(np.int64))
    np.add.at(s_exc, rows, exc.astype(np.int64))
    np.maximum.at(m_cov, rows, cov.astype(np.int64))
    assert np.all(s_exc <= buried) and np.all(buried <= s_cov) and np.all(m_cov <= buried)
    assert (cov > 0).any() and (exc > 0).any() and (cov == 0).any()


@pytest.mark.parametrize("name, probe, n_points", CONFIGS)
def test_model_pair_oracle(models, name, probe, n_points):
    cols, offs, ent, cov, exc = models[(name, probe, n_points)]
    n_in, n_out = cm.pair_check(*cols, probe, n_points, W, offs, ent, cov, n_pairs=400, seed=11)
    assert n_in + n_out == 400 and n_in > 300


@pytest.mark.parametrize("name, probe, n_points", CONFIGS)
def test_model_deletion_oracle(models, name, probe, n_points):
    cols, offs, ent, cov, exc = models[(name, probe, n_points)]
    n_cmp = cm.deletion_check(*cols, probe, n_points, W, offs, ent, exc, n_del=12, seed=12)
    assert n_cmp >= 11 * (len(cols[0]) - 1)


def test_model_batch_is_per_structure():
    a, b = nh.protor("2drt.pdb"), nh.protor("1jcd.pdb")
    cat = [np.concatenate([a[k], b[k]]) for k in range(5)]
    so = np.array([0, len(a[0]), len(a[0]) + len(b[0])], np.uint32)
    cov, exc = cm.contact_counts_batch(*cat, so, 1.4, 101, W)
    _, _, c1, x1 = cm.contact_counts(*a, 1.4, 101, W)
    _, _, c2, x2 = cm.contact_counts(*b, 1.4, 101, W)
    assert np.array_equal(cov, np.concatenate([c1, c2])) and np.array_equal(exc, np.concatenate([x1, x2]))
