"""Accessible-point entry points (rsasa_accessible_points*) as seen without a GPU: exported and bound, the Python
side's argument checks (they raise before any C call), unpack_points / surface_points on hand-made words, and the
exact CPU model of the masks (points_model.py) pinned to the oracle's accessible-point counts - the yardstick the GPU
tests compare with."""
import numpy as np
import pytest

import nb_helpers as nh
import points_model as pm
import tie_cases as tc
from oracle import pyoracle as po


def test_points_symbols_exported_and_bound():
    from rustsasa_amd import _capi
    lib = _capi.load()
    for name in ("rsasa_accessible_points", "rsasa_accessible_points_batch"):
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
        c.accessible_points(x, x, x[:4], x)                       # a short column
    with pytest.raises(ValueError):
        c.accessible_points(x, x, x, x, ids=np.zeros(4, np.uint64))
    with pytest.raises(ValueError):
        c.accessible_points(x.reshape(5, 1), x, x, x)              # not 1-D
    for n in (0, -3, 2.5):
        with pytest.raises(ValueError):
            c.accessible_points(x, x, x, x, n_points=n)
        with pytest.raises(ValueError):
            c.accessible_points_batch(x, x, x, x, None, [0, 5], n_points=n)
    with pytest.raises(ValueError):
        c.accessible_points_batch(x, x, x, x, None, [0, 2, 4])      # offsets cover 4 of 5 atoms
    with pytest.raises(ValueError):
        c.accessible_points_batch(x, x, x, x, None, [0, 3, 6])      # ... 6 of 5
    with pytest.raises(ValueError):
        c.accessible_points_batch(x, x, x, x, None, np.zeros((2, 2), np.uint32))
    with pytest.raises(ValueError):
        c.surface_points(x, x, x, x, n_points=0)


# ---- the model pinned to the oracle ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["1jcd.pdb", "151L_H3.pdb", "example.cif"])
@pytest.mark.parametrize("n_points, Ws", [(100, (8, 1)), (101, (16,)), (960, (8,))])
def test_model_counts_equal_oracle_on_fixtures(name, n_points, Ws):
    x, y, z, r, ids = nh.protor(name)
    masks = pm.exposed_masks_ws(x, y, z, r, ids, 1.4, n_points, Ws)
    for W in Ws:
        out, pts, _ = po.calculate_sasa_internal(x, y, z, r, ids, 1.4, n_points, W, return_details=True)
        assert np.array_equal(masks[W].sum(axis=1), pts)
        assert pm.sasa_of(r, 1.4, masks[W].sum(axis=1), n_points).tobytes() == out.tobytes()
    # the single-W form is the same model
    assert np.array_equal(pm.exposed_masks(x, y, z, r, ids, 1.4, n_points, Ws[0]), masks[Ws[0]])


def test_model_counts_equal_oracle_on_every_tie_case():
    n = 0
    for case in tc.all_cases():
        for st in case.structures:
            m = pm.exposed_masks(*st.soa(), case.probe, case.n_points, case.W)
            _, pts, _ = tc.oracle_counts(st, case.probe, case.n_points, case.W)
            assert np.array_equal(m.sum(axis=1), pts), (case.family, case.label)
            n += 1
    assert n > 10000


def test_model_sees_the_rule_at_exact_ties():
    """The fused `<` and the remainder `<=` differ exactly at dot == limit: a model that used one rule for every
    point would fail one of the two families."""
    fam = tc.generate()
    ties = [c for c in fam["fused"] + fam["remainder"] if c.tie]
    assert len(ties) >= 300
    for case in ties[:40]:
        for st in case.structures:
            for W in (case.W, 1):
                m = pm.exposed_masks(*st.soa(), case.probe, case.n_points, W)
                _, pts, _ = tc.oracle_counts(st, case.probe, case.n_points, W)
                assert np.array_equal(m.sum(axis=1), pts)


# ---- unpack_points / surface_points on hand-made words ---------------------------------------------------------

def test_unpack_points_bit_order_and_padding():
    from rustsasa_amd import unpack_points
    n = 40  # two words, 24 padding bits
    w = np.array([[0x00000001, 0x00000080],          # points 0 and 39
                  [0x80000000, 0x00000001],          # points 31 and 32
                  [0x00000000, 0xFFFFFF00]],         # only padding bits: no point
                 np.uint32)
    m = unpack_points(w, n)
    assert m.shape == (3, n) and m.dtype == bool
    assert np.nonzero(m[0])[0].tolist() == [0, 39]
    assert np.nonzero(m[1])[0].tolist() == [31, 32]
    assert not m[2].any()
    # the model's packing writes no padding bits and inverts unpack_points
    packed = pm.pack(m)
    assert packed.dtype == np.uint32 and packed.shape == (3, 2)
    assert packed.tolist() == [[1, 0x80], [0x80000000, 1], [0, 0]]
    rng = np.random.default_rng(1)
    for n in (1, 31, 32, 33, 100, 127, 960):
        mm = rng.random((7, n)) < 0.5
        pk = pm.pack(mm)
        assert pk.shape == (7, (n + 31) // 32)
        assert np.array_equal(unpack_points(pk, n), mm)
        if n % 32:
            assert not (pk[:, -1] >> np.uint32(n % 32)).any()
    with pytest.raises(ValueError):
        unpack_points(w, 65)  # three words expected
    with pytest.raises(ValueError):
        unpack_points(w, 0)


def test_surface_points_are_centre_plus_R_s():
    from rustsasa_amd import sphere_points, surface_points
    n = 100
    x = np.array([1.5, -2.25, 10.0], np.float32)
    y = np.array([0.1, 3.3, -7.7], np.float32)
    z = np.array([-4.0, 0.5, 2.2], np.float32)
    r = np.array([1.7, 1.52, 1.88], np.float32)
    probe = 1.4
    m = np.zeros((3, n), bool)
    m[0, [0, 5, 99]] = True
    m[2, :] = True
    atom, xyz = surface_points(pm.pack(m), x, y, z, r, probe, n)
    assert atom.dtype == np.uint32 and xyz.dtype == np.float32
    assert atom.tolist() == [0, 0, 0] + [2] * n
    sx, sy, sz = sphere_points(n)
    assert np.array_equal(sx, po.sphere_points(n)[0])
    pts = [(0, 0), (0, 5), (0, 99)] + [(2, p) for p in range(n)]
    for k, (i, p) in enumerate(pts):
        R = np.float32(r[i]) + np.float32(probe)
        for c, s, col in ((x, sx, 0), (y, sy, 1), (z, sz, 2)):
            assert xyz[k, col] == np.float32(np.float32(c[i]) + np.float32(R * np.float32(s[p])))
    atom0, xyz0 = surface_points(np.zeros((3, 4), np.uint32), x, y, z, r, probe, n)
    assert atom0.shape == (0,) and xyz0.shape == (0, 3)
    with pytest.raises(ValueError):
        surface_points(pm.pack(m), x[:2], y[:2], z[:2], r[:2], probe, n)
