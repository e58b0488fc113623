"""Exposure vectors and the volume made from them (rsasa_exposure_vectors*, rsasa_sas_volume) as seen without a GPU:
the symbols are exported and bound, the Python side's argument checks raise before any C call, the CPU model of the
vectors (exposure_model.py) follows the interface's summation tree literally - and that tree is not numpy's own order -
and the host utility rsasa_sas_volume equals the model's double formula, gives a lone sphere's volume, approaches the
analytic union of two spheres, and skips non-finite atoms."""
import numpy as np
import pytest

import exposure_model as em
import nb_helpers as nh
import points_model as pm
from oracle import pyoracle as po

F = np.float32
TREE_POINTS = (1, 63, 64, 65, 100, 129, 257)


def test_exposure_symbols_exported_and_bound():
    from rustsasa_amd import _capi
    lib = _capi.load()
    for name in ("rsasa_exposure_vectors", "rsasa_exposure_vectors_batch", "rsasa_sas_volume"):
        assert hasattr(lib, name)
        assert name in _capi.SYMBOLS
        assert getattr(lib, name).argtypes == _capi.SYMBOLS[name][1]
    assert lib.rsasa_abi_version() == 4


class _NoCall:
    """Stands in for the library: any C call fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_argument_errors_raise_before_the_c_call():
    import rustsasa_amd
    c = object.__new__(rustsasa_amd.Context)
    c._lib = _NoCall()
    c._h = None
    x = np.zeros(5, np.float32)
    with pytest.raises(ValueError):
        c.exposure_vectors(x, x, x[:4], x)                         # a short column
    with pytest.raises(ValueError):
        c.exposure_vectors(x, x, x, x, ids=np.zeros(4, np.uint64))
    for n in (0, -3, 2.5):
        with pytest.raises(ValueError):
            c.exposure_vectors(x, x, x, x, n_points=n)
        with pytest.raises(ValueError):
            c.exposure_vectors_batch(x, x, x, x, None, [0, 5], n_points=n)
    with pytest.raises(ValueError):
        c.exposure_vectors_batch(x, x, x, x, None, [0, 2, 4])       # offsets cover 4 of 5 atoms
    v, k = np.zeros((5, 3), np.float32), np.zeros(5, np.uint32)
    with pytest.raises(ValueError):
        rustsasa_amd.sas_volume(v[:4], k, x, x, x, x)
    with pytest.raises(ValueError):
        rustsasa_amd.sas_volume(v, k[:4], x, x, x, x)
    with pytest.raises(ValueError):
        rustsasa_amd.sas_volume(v, k, x, x, x, x, n_points=0)
    with pytest.raises(ValueError):
        rustsasa_amd.sas_volume(v, k, x, x, x, x, structure_offsets=[0, 2, 4])
    with pytest.raises(ValueError):
        rustsasa_amd.sas_volume(v, k, x, x, x, x, origins=np.zeros((2, 3)))


def test_sas_volume_argument_errors_from_the_library():
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    lib = _capi.load()
    x = np.ones(3, np.float32)
    v, k = np.zeros((3, 3), np.float32), np.zeros(3, np.uint32)
    so = np.array([0, 3], np.uint32)
    vol = np.zeros(1)

    def call(x_=x, v_=v, k_=k, so_=so, n_points=100, vol_=vol):
        return lib.rsasa_sas_volume(ptr(x_), ptr(x), ptr(x), ptr(x), ptr(v_), ptr(k_), ptr(so_), len(so) - 1, 1.4,
                                    n_points, None, ptr(vol_), None)
    assert call() == _capi.RSASA_OK
    assert call(n_points=0) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert call(x_=None) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert call(v_=None) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert call(k_=None) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert call(so_=None) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert call(vol_=None) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert call(so_=np.array([1, 3], np.uint32)) == _capi.RSASA_ERR_INVALID_ARGUMENT
    bad = np.array([0, 3, 2], np.uint32)
    assert lib.rsasa_sas_volume(ptr(x), ptr(x), ptr(x), ptr(x), ptr(v), ptr(k), ptr(bad), 2, 1.4, 100, None,
                                ptr(np.zeros(2)), None) == _capi.RSASA_ERR_INVALID_ARGUMENT


# ---- the model follows the tree -----------------------------------------------------------------------------------

def _tree_by_hand(mask_row, n_points):
    """One atom's vector by a scalar loop that follows the interface's words: terms, six halvings per chunk, chunks
    ascending."""
    out = []
    n_chunks = -(-n_points // 64)
    for s in po.sphere_points(n_points):
        E = None
        for c in range(n_chunks):
            t = []
            for lane in range(64):
                p = c * 64 + lane
                t.append(F(s[p]) if p < n_points and mask_row[p] else F(0.0))
            for h in (32, 16, 8, 4, 2, 1):
                for lane in range(h):
                    t[lane] = F(t[lane] + t[lane + h])
            E = t[0] if c == 0 else F(E + t[0])
        out.append(E)
    return np.array(out, F)


@pytest.mark.parametrize("n_points", TREE_POINTS)
def test_model_equals_the_tree_followed_literally(n_points):
    rng = np.random.default_rng(n_points)
    mask = np.concatenate([rng.random((3, n_points)) < 0.5, rng.random((1, n_points)) < 0.05,
                           np.ones((1, n_points), bool), np.zeros((1, n_points), bool)])
    got = em.vectors_of(mask, n_points)
    assert got.dtype == F and got.shape == (len(mask), 3)
    for i, row in enumerate(mask):
        assert np.array_equal(em.bits(got[i]), em.bits(_tree_by_hand(row, n_points))), (n_points, i)
    assert not em.bits(got[-1]).any()                      # no exposed point: +0.0 in every component
    # the all-true row is the tree over the whole lattice, whatever the mask's padding
    assert np.array_equal(em.bits(got[-2]), em.bits(em.vectors_of(np.ones((1, n_points), bool), n_points)[0]))


def test_the_tree_is_not_numpys_order():
    """The whole lattice of 100 points: the tree's float32 sums differ from np.sum(dtype=float32) - numpy's pairwise
    order - in every component, so a summation in another order does not pass for the interface's."""
    n = 100
    tree = em.vectors_of(np.ones((1, n), bool), n)[0]
    flat = np.array([np.sum(s, dtype=F) for s in po.sphere_points(n)], F)
    assert flat.dtype == F
    assert (em.bits(tree) != em.bits(flat)).any()
    assert np.allclose(tree, flat, rtol=0, atol=1e-5)      # ... by rounding only


# ---- rsasa_sas_volume ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def jcd():
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    mask = pm.exposed_masks(x, y, z, r, ids, 1.4, 100, 8)
    return (x, y, z, r), em.vectors_of(mask, 100), mask.sum(axis=1).astype(np.uint32)


def test_sas_volume_equals_the_model_on_1jcd(jcd):
    """Both are double sums of the same terms in the same order: equal, not close."""
    import rustsasa_amd
    cols, v, k = jcd
    vol, area = rustsasa_amd.sas_volume(v, k, *cols, 1.4, 100)
    want_vol, want_area = em.volume_of(*cols, v, k, 1.4, 100)
    assert vol.dtype == np.float64 and vol.shape == (1,) and area.shape == (1,)
    assert vol[0] == want_vol[0] and area[0] == want_area[0]
    assert 2.0e4 < vol[0] < 3.5e4                          # 1jcd: 1 052 atoms, about 26 000 A^3 inside the SAS
    # the area is the sum of the atoms' values, up to their float32 rounding
    assert area[0] == pytest.approx(float(pm.sasa_of(cols[3], 1.4, k, 100).astype(np.float64).sum()), rel=1e-6)
    # another origin: the model's again, and the same volume up to the dots' discretisation
    o = np.array([[1.0, -2.0, 3.0]])
    vol_o, _ = rustsasa_amd.sas_volume(v, k, *cols, 1.4, 100, origins=o)
    assert vol_o[0] == em.volume_of(*cols, v, k, 1.4, 100, origins=o)[0][0]
    assert vol_o[0] == pytest.approx(vol[0], rel=0.05)


@pytest.mark.parametrize("so", [(0, 0, 1052), (0, 1052, 1052), (0, 400, 1052)])
def test_sas_volume_equals_the_model_on_a_batch_with_an_empty_structure(jcd, so):
    import rustsasa_amd
    cols, v, k = jcd
    so = np.array(so, np.uint32)
    assert int(so[-1]) == len(k)
    vol, area = rustsasa_amd.sas_volume(v, k, *cols, 1.4, 100, structure_offsets=so)
    want_vol, want_area = em.volume_of(*cols, v, k, 1.4, 100, so)
    assert np.array_equal(vol, want_vol) and np.array_equal(area, want_area)
    for s in range(2):
        if so[s] == so[s + 1]:
            assert vol[s] == 0.0 and area[s] == 0.0        # an empty structure
        else:
            assert vol[s] > 0.0


@pytest.mark.parametrize("n_points", [100, 960])
def test_lone_sphere_has_its_volume(n_points):
    """The origin at the centre: (c - o) . E vanishes and V = (a / 3) R n = 4/3 pi R^3."""
    import rustsasa_amd
    x, y, z, r = (np.array([v], F) for v in (3.0, -7.5, 11.25, 1.8))
    v = em.vectors_of(np.ones((1, n_points), bool), n_points)
    k = np.array([n_points], np.uint32)
    vol, area = rustsasa_amd.sas_volume(v, k, x, y, z, r, 1.4, n_points, origins=[[3.0, -7.5, 11.25]])
    R = float(F(1.8) + F(1.4))
    assert vol[0] == pytest.approx(4.0 / 3.0 * np.pi * R ** 3, rel=1e-12)
    assert area[0] == pytest.approx(4.0 * np.pi * R ** 2, rel=1e-12)
    # origins None: the mean centre is the centre
    assert rustsasa_amd.sas_volume(v, k, x, y, z, r, 1.4, n_points)[0][0] == vol[0]


# |V - V_union| / V_union of the model on the six cases, measured (radii 1.8 and 1.5, probe 1.4, origin = mean centre):
#   n_points   d = 1.0    d = 2.5    d = 4.0
#   100        0.875 %    0.227 %    0.569 %
#   960        0.292 %    0.210 %    0.038 %
# The bound at each point count is twice the largest of its three errors.
UNION_BOUND = {100: 2 * 0.00876, 960: 2 * 0.00293}


@pytest.mark.parametrize("d", [1.0, 2.5, 4.0])
@pytest.mark.parametrize("n_points", [100, 960])
def test_two_overlapping_spheres_approach_the_analytic_union(n_points, d):
    """Radii 1.8 and 1.5 at probe 1.4 (R = 3.2 and 2.9), centres d apart: the volume from the model's vectors against
    4/3 pi (R1^3 + R2^3) minus the lens.  The dots' relative errors, measured: 0.875 %, 0.227 %, 0.569 % at 100
    points and 0.292 %, 0.210 %, 0.038 % at 960 (d = 1.0, 2.5, 4.0); the bound is twice the largest at each point
    count: 1.752 % and 0.586 %."""
    import rustsasa_amd
    x, y, z = np.array([0.0, d], F), np.zeros(2, F), np.zeros(2, F)
    r = np.array([1.8, 1.5], F)
    mask = pm.exposed_masks(x, y, z, r, None, 1.4, n_points, 8)
    k = mask.sum(axis=1).astype(np.uint32)
    assert 0 < k[0] < n_points and 0 < k[1] < n_points     # each sphere partly inside the other
    vol, _ = rustsasa_amd.sas_volume(em.vectors_of(mask, n_points), k, x, y, z, r, 1.4, n_points)
    R = (r + F(1.4)).astype(np.float64)
    want = em.union_volume(R[0], R[1], d)
    err = abs(vol[0] - want) / want
    print(f"n_points {n_points} d {d}: V {vol[0]:.6f} union {want:.6f} relative error {err:.5%}")
    assert err <= UNION_BOUND[n_points]


def test_non_finite_atoms_are_skipped(jcd):
    import rustsasa_amd
    cols, v, k = jcd
    x, y, z, r = (a.copy() for a in cols)
    x[5], y[40], z[77], r[17], x[900] = np.nan, np.nan, np.inf, np.nan, -np.inf
    bad = [5, 17, 40, 77, 900]
    keep = np.setdiff1d(np.arange(len(x)), bad)
    vol, area = rustsasa_amd.sas_volume(v, k, x, y, z, r, 1.4, 100)
    assert np.isfinite(vol[0]) and np.isfinite(area[0])
    # ... the structure without those atoms, mean centre included
    sub, _ = rustsasa_amd.sas_volume(v[keep], k[keep], x[keep], y[keep], z[keep], r[keep], 1.4, 100)
    assert vol[0] == sub[0]
    want_vol, want_area = em.volume_of(x, y, z, r, v, k, 1.4, 100)
    assert vol[0] == want_vol[0] and area[0] == want_area[0]
    # every atom non-finite: nothing is summed
    nan = np.full(3, np.nan, F)
    one = np.ones(3, F)
    vol, area = rustsasa_amd.sas_volume(v[:3], k[:3], nan, one, one, one, 1.4, 100)
    assert vol[0] == 0.0 and area[0] == 0.0
