"""Group-contact entry points (rsasa_group_contacts*) as seen without a GPU: exported and bound, the Python side's
argument checks (they raise before any C call), group_areas on a hand-made case, and the exact CPU model of the counts
(groups_model.py) pinned to the oracle on the multi-chain fixtures - the yardstick the GPU tests compare with."""
import os

import numpy as np
import pytest

import groups_model as gm
import nb_helpers as nh

FIXTURES = ("1jcd.pdb", "2drt.pdb", "freesasa/3w7y.pdb", "freesasa/4c1a.pdb")
WS = (1, 8)
N_POINTS = (100, 960)
PROBE = 1.4
# With vdW radii every protein chain holds the structure's largest radius (a sulphur where there is one, a carbon
# otherwise), so no sub-structure changes the candidate rule: the share of oracle comparisons skipped for it must be 0
# on these fixtures (test_fixtures_have_several_chains_with_the_largest_radius checks the premise).
MAX_SKIPPED_SHARE = 0.0


def test_group_symbols_exported_and_bound():
    from rustsasa_amd import _capi
    lib = _capi.load()
    assert lib.rsasa_abi_version() == 4
    for name in ("rsasa_group_contacts", "rsasa_group_contacts_batch"):
        assert hasattr(lib, name)
        assert name in _capi.SYMBOLS
        assert getattr(lib, name).argtypes == _capi.SYMBOLS[name][1]
    header = open(os.path.join(os.path.dirname(_capi.__file__), "..", "include", "rustsasa_amd.h")).read()
    assert "int rsasa_group_contacts(" in header and "int rsasa_group_contacts_batch(" in header
    assert "#define RSASA_ABI_VERSION 4" in header


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
    g = np.zeros(5, np.uint32)
    with pytest.raises(ValueError):
        c.group_contacts(x, x, x, x, None, g[:4])                       # a label short
    with pytest.raises(ValueError):
        c.group_contacts(x, x, x, x, None, np.zeros(5, np.float32))     # labels are integers
    with pytest.raises(ValueError):
        c.group_contacts(x, x, x, x, None, np.array([0, 1, 2, 3, -1]))  # ... in [0, 2^32)
    with pytest.raises(ValueError):
        c.group_contacts(x, x, x, x, None, np.array([0, 1, 2, 3, 1 << 32], np.int64))
    with pytest.raises(ValueError):
        c.group_contacts(x, x, x, x, None, g.reshape(5, 1))             # not 1-D
    with pytest.raises(ValueError):
        c.group_contacts(x, x, x[:4], x, None, g)                       # a short column
    with pytest.raises(ValueError):
        c.group_contacts(x.reshape(5, 1), x, x, x, None, g)
    with pytest.raises(ValueError):
        c.group_contacts(x, x, x, x, np.zeros(4, np.uint64), g)
    for n in (0, -3, 2.5):
        with pytest.raises(ValueError):
            c.group_contacts(x, x, x, x, None, g, n_points=n)
        with pytest.raises(ValueError):
            c.group_contacts_batch(x, x, x, x, None, g, [0, 5], n_points=n)
    with pytest.raises(ValueError):
        c.group_contacts_batch(x, x, x, x, None, g, [0, 2, 4])          # offsets cover 4 of 5 atoms
    with pytest.raises(ValueError):
        c.group_contacts_batch(x, x, x, x, None, g[:4], [0, 5])
    with pytest.raises(ValueError):
        c.group_contacts_batch(x, x, x, x, None, g, np.zeros((2, 2), np.uint32))


def test_group_areas_on_a_hand_made_case():
    from rustsasa_amd import contact_areas, group_areas
    r = np.array([1.7, 1.52, 1.88, 1.7], np.float32)
    groups = np.array([7, 7, 2, 0xFFFFFFFF], np.uint32)
    offs = np.array([0, 2, 3, 3, 5], np.uint64)                        # atom 2 has no row
    partner = np.array([2, 0xFFFFFFFF, 2, 2, 7], np.uint32)
    counts = np.array([10, 0, 37, 100, 1], np.uint32)
    for probe, n in ((1.4, 100), (1.2, 97)):
        frm, to, area = group_areas(offs, partner, counts, groups, r, probe, n)
        assert frm.dtype == np.uint32 and to.dtype == np.uint32 and area.dtype == np.float64
        # sorted by (from, to); (7, 2) sums the rows of atoms 0 and 1; the row of 0 points stays
        assert frm.tolist() == [7, 7, 0xFFFFFFFF, 0xFFFFFFFF] and to.tolist() == [2, 0xFFFFFFFF, 2, 7]
        per_row = contact_areas(counts, offs, r, probe, n)
        R0 = np.float32(r[0]) + np.float32(probe)
        assert per_row[0] == np.float32(np.float32(np.float32(np.float32(12.566371) * np.float32(R0 * R0)) * np.float32(10.0))
                                        * np.float32(np.float32(1.0) / np.float32(n)))
        want = [float(per_row[0]) + float(per_row[2]), 0.0, float(per_row[3]), float(per_row[4])]
        assert area.tolist() == want
    # (A, B) and (B, A) are separate entries
    frm, to, area = group_areas(np.array([0, 1, 2], np.uint64), np.array([1, 0], np.uint32), np.array([5, 9], np.uint32),
                                np.array([0, 1], np.uint32), r[:2], 1.4, 100)
    assert list(zip(frm.tolist(), to.tolist())) == [(0, 1), (1, 0)] and area[0] != area[1]
    # no rows
    frm, to, area = group_areas(np.zeros(3, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32), groups[:2], r[:2])
    assert len(frm) == len(to) == len(area) == 0
    with pytest.raises(ValueError):
        group_areas(offs, partner[:4], counts, groups, r)               # a partner label per row
    with pytest.raises(ValueError):
        group_areas(offs, partner, counts, groups[:3], r)               # a label per atom
    with pytest.raises(ValueError):
        group_areas(offs, partner, counts[:4], groups, r)
    with pytest.raises(ValueError):
        group_areas(offs, partner, counts, groups, r, n_points=0)


# ---- the model ---------------------------------------------------------------------------------------------------

def test_model_on_a_hand_made_list():
    """Atom 0 among one atom of its own label, one of label 3 and two of label 9 whose caps overlap: the unions by
    their definitions, from per-entry hit sets computed point by point here."""
    x = np.array([0.0, 2.0, -2.0, 0.0, 1.5], np.float32)
    y = np.array([0.0, 0.0, 0.0, 2.0, 1.5], np.float32)
    z = np.zeros(5, np.float32)
    r = np.full(5, 1.5, np.float32)
    g = np.array([5, 9, 3, 5, 9], np.uint32)
    n_points, W = 64, 8
    offs, partner, buried, only, self_free, free = gm.group_counts(x, y, z, r, None, g, 1.4, n_points, W)
    # the same from contacts_model's per-entry pieces: the per-entry hit sets of atom 0, by label
    import contacts_model as cm
    import tie_cases as tc
    from oracle import pyoracle as po
    lo, le = nh.oracle_csr(x, y, z, r, None, 1.4)
    assert np.diff(lo.astype(np.int64)).tolist() == [4, 4, 4, 4, 4]
    sx, sy, sz = po.sphere_points(n_points)
    hits = {}
    for e in range(int(lo[0]), int(lo[1])):
        j = int(le["idx"][e])
        hits[j] = np.array([tc.point_occluded((x[0], y[0], z[0]), r[0], (x[j], y[j], z[j]), r[j], 1.4,
                                              (sx[p], sy[p], sz[p]), fused=True) for p in range(n_points)])
    self_ = hits[3]
    c9, c3 = (hits[1] | hits[4]) & ~self_, hits[2] & ~self_
    assert partner[:2].tolist() == [3, 9] and offs[:2].tolist() == [0, 2]       # ascending label, own label no row
    assert buried[:2].tolist() == [int(c3.sum()), int(c9.sum())]
    assert only[:2].tolist() == [int((c3 & ~c9).sum()), int((c9 & ~c3).sum())]
    assert self_free[0] == n_points - self_.sum() and free[0] == n_points - (self_ | c3 | c9).sum()
    both = hits[1] & hits[4] & ~self_                                         # a real union: a sum counts these twice
    assert both.any() and c9.sum() == (hits[1] & ~self_).sum() + (hits[4] & ~self_).sum() - both.sum()
    # free is what contacts_model buries
    _, _, by_w = cm.contact_counts_ws(x, y, z, r, None, 1.4, n_points, (W,))
    assert np.array_equal(n_points - free.astype(np.int64), by_w[W][2])


@pytest.fixture(scope="module")
def fixtures():
    return {name: gm.labelled_fixture(name) for name in FIXTURES}


def test_fixtures_have_several_chains_with_the_largest_radius(fixtures):
    for name, (cols, chain, residue, names) in fixtures.items():
        assert len(names) >= 2, name
        rmax = nh.fold_max(cols[3])
        for h in range(len(names)):
            assert nh.fold_max(cols[3][chain == h]) == rmax, (name, names[h])
        assert len(np.unique(residue)) > 10 * len(names)


@pytest.mark.parametrize("n_points", N_POINTS)
@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("name", FIXTURES)
def test_model_against_the_oracle_by_chain(fixtures, name, W, n_points):
    cols, chain, _, names = fixtures[name]
    model = gm.group_counts(*cols, chain, PROBE, n_points, W)
    offs, partner, buried, only, self_free, free = model
    # shape and order of the rows; the identities
    atom = gm.rows_of(offs)
    assert len(partner) == len(buried) == len(only) == int(offs[-1]) > 0
    assert not (partner == chain[atom]).any()
    same = atom[1:] == atom[:-1]
    assert np.all(partner[1:][same] > partner[:-1][same])
    n = len(cols[0])
    s_bur, m_bur, s_only = (np.zeros(n, np.int64) for _ in range(3))
    np.add.at(s_bur, atom, buried.astype(np.int64))
    np.maximum.at(m_bur, atom, buried.astype(np.int64))
    np.add.at(s_only, atom, only.astype(np.int64))
    lost = self_free.astype(np.int64) - free.astype(np.int64)
    assert np.all(m_bur <= lost) and np.all(lost <= s_bur) and np.all(s_only <= lost)
    one = np.diff(offs.astype(np.int64)) == 1
    assert one.any() and np.array_equal(lost[one], s_bur[one]) and np.array_equal(lost[one], s_only[one])
    assert (buried > 0).any() and (only > 0).any()
    # the three oracles
    total = skipped = 0
    for check in (gm.alone_check, gm.pair_check, gm.deletion_check):
        done, skip = check(*cols, chain, PROBE, n_points, W, model)
        assert done > 0
        total += done + skip
        skipped += skip
    assert skipped <= MAX_SKIPPED_SHARE * total, (skipped, total)


def test_model_by_residue_and_degenerate_labellings(fixtures):
    cols, chain, residue, _ = fixtures["1jcd.pdb"]
    n = len(cols[0])
    import contacts_model as cm
    offs_c, ent_c, cov, exc = cm.contact_counts(*cols, PROBE, 100, 8)
    buried_c = cm.contact_counts_ws(*cols, PROBE, 100, (8,), lists=(offs_c, ent_c))[2][8][2]
    # all labels equal: no rows, self_free == free == the exposed points
    m = gm.group_counts(*cols, np.full(n, 3, np.uint32), PROBE, 100, 8, lists=(offs_c, ent_c))
    assert int(m[0][-1]) == 0 and np.array_equal(m[4], m[5]) and np.array_equal(100 - m[5].astype(np.int64), buried_c)
    # label = index: self_free == n_points, one row per entry, buried == covered and only == exclusive
    m = gm.group_counts(*cols, np.arange(n, dtype=np.uint32), PROBE, 100, 8, lists=(offs_c, ent_c))
    assert np.all(m[4] == 100) and np.array_equal(m[0], offs_c)
    by_idx = np.lexsort((ent_c["idx"], gm.rows_of(offs_c)))
    assert np.array_equal(m[1], ent_c["idx"][by_idx])
    assert np.array_equal(m[2], cov[by_idx]) and np.array_equal(m[3], exc[by_idx])
    # by residue: the alone oracle on the residues that hold the largest radius, and nothing depends on list order
    m = gm.group_counts(*cols, residue, PROBE, 100, 8, lists=(offs_c, ent_c))
    done, skipped = gm.alone_check(*cols, residue, PROBE, 100, 8, m)
    assert done + skipped == len(np.unique(residue)) and done >= 100 and skipped <= done // 10
    rng = np.random.default_rng(5)
    shuffled = ent_c.copy()
    o = offs_c.astype(np.int64)
    for i in range(n):
        shuffled[o[i]:o[i + 1]] = ent_c[o[i]:o[i + 1]][rng.permutation(o[i + 1] - o[i])]
    m2 = gm.group_counts(*cols, residue, PROBE, 100, 8, lists=(offs_c, shuffled))
    for a, b in zip(m, m2):
        assert np.array_equal(a, b)


def test_model_batch_is_per_structure(fixtures):
    a, ga = fixtures["2drt.pdb"][:2]
    b, gb = fixtures["1jcd.pdb"][:2]
    cat = [np.concatenate([a[k], b[k]]) for k in range(5)]
    so = np.array([0, len(a[0]), len(a[0]), len(a[0]) + len(b[0])], np.uint32)   # (an empty structure between them)
    got = gm.group_counts_batch(*cat, np.concatenate([ga, gb]), so, PROBE, 101, 8)
    m1, m2 = gm.group_counts(*a, ga, PROBE, 101, 8), gm.group_counts(*b, gb, PROBE, 101, 8)
    assert np.array_equal(got[0], np.concatenate([m1[0], m2[0][1:] + m1[0][-1]]))
    for k in range(1, 6):
        assert np.array_equal(got[k], np.concatenate([m1[k], m2[k]]))
