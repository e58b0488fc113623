"""The twelve families that share one host prologue and one set of scratch buffers (neighbors.cpp: neighbour lists,
accessible points, exposure vectors, atom depth, surface components, contact counts, contact owners, group contacts,
radial counts, half-sphere exposure, atoms within a cutoff, nearest atoms - the last three add the flags, directions,
counts and rows to the scratch and keep the centres' ranks in the neighbour runs' map; the radial counts write
(class << 2) | flags into the sorted-flags buffer those three read as plain flags, and stand before them in the walk, so
the forward walk runs radial -> hse / within / nearest with flags NULL over class bits and the reverse walk the other
way), walked in an order that makes every shared buffer grow, be reused while oversized, and serve another family than
the one that sized it.
What the per-family suites cannot see: a first call on a fresh context whose every list is empty (no fill has ever run,
the entries' buffer does not exist yet), and a result that depends on which family ran before.

Inputs: A one atom (its list is empty), B the 1jcd fixture, C a batch of A, an empty structure and B.  Every result of
the walk is compared byte for byte with the same call on a context that made no other call; B is also compared with the
Python models (points, depth, components, half-sphere counts, within-lists, nearest lists), so the comparison is not only
the library against itself."""
import functools

import numpy as np
import pytest

import components_model as cm
import depth_model as dm
import exposure_model as em
import hse_cases as hc
import hse_model as hm
import nb_helpers as nh
import nearest_model as nm
import owners_model as om
import points_model as pm
import radial_cases as rc
import radial_model as rm
import within_model as wm

pytestmark = pytest.mark.gpu

PROBE = 1.4
N_POINTS = (100, 129)  # 4 mask words, 4 points past the fused 96; 5 words, the last holding the one point past the fused 128
ORDER = ("points", "groups", "depth", "contacts", "owners", "components", "exposure", "neighbours", "radial", "hse", "within",
         "nearest")
CUTOFF_TRIO = ("hse", "within", "nearest")   # n_points is ignored (by "radial" too)
RADIAL_CLASSES = 16
HSE_CUTOFF, WITHIN_CUTOFF, NEAREST_K = 13.0, 8.0, 16


@functools.lru_cache(maxsize=None)
def _inputs():
    """{name: (x, y, z, r, ids, groups, structure_offsets or None)}."""
    bx, by, bz, br, bids = nh.protor("1jcd.pdb")
    n = len(bx)
    bgroups = (np.arange(n, dtype=np.int64) * 3 // n).astype(np.uint32)
    f = lambda *v: np.array(v, np.float32)  # noqa: E731
    a = (f(1.0), f(-2.0), f(3.0), f(1.7), np.array([7], np.uint64), np.array([0], np.uint32), None)
    b = (bx, by, bz, br, bids, bgroups, None)
    c = tuple(np.concatenate([p, q]) for p, q in zip(a[:6], b[:6])) + (np.array([0, 1, 1, 1 + n], np.uint32),)
    return {"A": a, "B": b, "C": c}


def _link(r, n_points):
    import rustsasa_amd
    return rustsasa_amd.default_link(r, PROBE, n_points)


@functools.lru_cache(maxsize=None)
def _dirs(n):
    return hc.random_dirs(n, 83)


@functools.lru_cache(maxsize=None)
def _classes(n):
    return rc.classes_of(n, RADIAL_CLASSES, 84)


def _call(ctx, family, inp, n_points):
    """The family's call on `inp` (the single-structure method, or the batch method when the input has offsets) as a
    tuple of arrays."""
    x, y, z, r, ids, groups, so = inp
    batch = so is not None
    cols = (x, y, z, r, ids)
    if family == "neighbours":
        return ctx.precompute_neighbors_batch(*cols, so, PROBE) if batch else ctx.precompute_neighbors(*cols, PROBE)
    if family == "hse":
        tail = (PROBE, _dirs(len(x)), None, HSE_CUTOFF)
        return ctx.half_sphere_exposure_batch(*cols, so, *tail) if batch else ctx.half_sphere_exposure(*cols, *tail)
    if family == "within":
        tail = (PROBE, None, WITHIN_CUTOFF)
        return ctx.atoms_within_batch(*cols, so, *tail) if batch else ctx.atoms_within(*cols, *tail)
    if family == "nearest":
        tail = (PROBE, NEAREST_K)
        return ctx.nearest_atoms_batch(*cols, so, *tail) if batch else ctx.nearest_atoms(*cols, *tail)
    if family == "radial":
        tail = (PROBE, rc.EDGES, _classes(len(x)), RADIAL_CLASSES, None, True)
        return ctx.radial_counts_batch(*cols, so, *tail) if batch else ctx.radial_counts(*cols, *tail)
    if family == "owners":
        tail = (PROBE, n_points, True)
        return ctx.contact_owners_batch(*cols, so, *tail) if batch else ctx.contact_owners(*cols, *tail)
    if family == "groups":
        tail = (PROBE, n_points)
        return ctx.group_contacts_batch(*cols, groups, so, *tail) if batch else ctx.group_contacts(*cols, groups, *tail)
    if family == "components":
        tail = (PROBE, n_points, _link(r, n_points))
        return ctx.surface_components_batch(*cols, so, *tail) if batch else ctx.surface_components(*cols, *tail)
    single, many = {"points": (ctx.accessible_points, ctx.accessible_points_batch),
                    "depth": (ctx.atom_depth, ctx.atom_depth_batch),
                    "contacts": (ctx.contact_points, ctx.contact_points_batch),
                    "exposure": (ctx.exposure_vectors, ctx.exposure_vectors_batch)}[family]
    return many(*cols, so, PROBE, n_points) if batch else single(*cols, PROBE, n_points)


def _alone(family, name, n_points):
    """The call on a context that makes no other call."""
    import rustsasa_amd
    with rustsasa_amd.Context(0) as ctx:
        return _call(ctx, family, _inputs()[name], n_points)


def _same(got, want):
    return len(got) == len(want) and all(
        g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


@pytest.fixture(scope="module")
def alone():
    """{(family, input, n_points): the result on a fresh context}, computed once and left unchanged."""
    return {(f, i, n): _alone(f, i, n) for n in N_POINTS for f in ORDER for i in _inputs()}


# ---- fresh contexts: the first call has nothing but empty lists ---------------------------------------------------

@pytest.mark.parametrize("family", ORDER)
def test_first_call_on_a_fresh_context_has_only_empty_lists(alone, family):
    n_points = 100
    x, y, z, r, ids, groups, _ = _inputs()["A"]
    got = alone[(family, "A", n_points)]  # (raises unless the call returned RSASA_OK)
    full = pm.pack(np.ones((1, n_points), bool))
    sasa = pm.sasa_of(r, PROBE, np.array([n_points]), n_points)
    none = np.zeros(2, np.uint64)
    if family == "neighbours":
        offsets, entries = got
        assert np.array_equal(offsets, none) and entries.shape == (0,)
        return
    if family == "hse":
        up, down = got
        assert up.dtype == down.dtype == np.uint32 and up.tolist() == [0] and down.tolist() == [0]
        return
    if family in ("within", "nearest"):
        offsets, entries = got
        assert np.array_equal(offsets, none) and entries.shape == (0,) and entries.dtype == wm.WITHIN_DTYPE
        return
    if family == "radial":
        table, pairs = got
        assert table.dtype == np.uint32 and table.shape == (1, RADIAL_CLASSES, len(rc.EDGES)) and not table.any()
        assert pairs.dtype == np.uint64 and pairs.shape == (1, RADIAL_CLASSES, RADIAL_CLASSES, len(rc.EDGES)) and not pairs.any()
        return
    if family == "owners":
        offsets, entries, owned, value, owner = got
        assert np.array_equal(offsets, none) and entries.shape == owned.shape == (0,) and owned.dtype == np.uint32
        assert owner.dtype == np.uint32 and owner.shape == (1, n_points) and np.all(owner == om.FREE)     # 0xFFFFFFFF
        assert value.tobytes() == sasa.tobytes()                        # every point free: the full sphere
        return
    assert got[-1].tobytes() == sasa.tobytes()
    if family == "points":
        assert np.array_equal(got[0], full)  # every point accessible
    elif family == "exposure":
        vectors, free, _ = got
        want = em.vectors_of(np.ones((1, n_points), bool), n_points)  # every lattice point, in the kernel's fixed order
        assert free.tolist() == [n_points] and vectors.dtype == want.dtype and vectors.tobytes() == want.tobytes()
    elif family == "contacts":
        offsets, entries, covered, exclusive, _ = got
        assert np.array_equal(offsets, none) and entries.shape == covered.shape == exclusive.shape == (0,)
    elif family == "groups":
        offsets, partner, buried, only, self_free, free, _ = got
        assert np.array_equal(offsets, none) and partner.shape == buried.shape == only.shape == (0,)
        assert self_free.tolist() == [n_points] and free.tolist() == [n_points]
    elif family == "depth":
        depth, nearest, free, _ = got
        want_depth, want_nearest, _ = dm.atom_depth(x, y, z, r, ids, PROBE, n_points, mask=np.ones((1, n_points), bool))
        assert free.tolist() == [n_points] and nearest.tolist() == [0] and want_nearest.tolist() == [0]
        assert depth.tobytes() == want_depth.tobytes()  # the atom's own nearest dot
    else:
        offsets, labels, free, _ = got
        want_off, want_labels, _ = cm.components(x, y, z, r, ids, PROBE, n_points, _link(r, n_points),
                                                 mask=np.ones((1, n_points), bool))
        assert free.tolist() == [n_points] and np.array_equal(offsets, want_off) and np.array_equal(labels, want_labels)


# ---- the walk: one context through every family and back -----------------------------------------------------------

@pytest.mark.parametrize("n_points", N_POINTS)
def test_walk_through_the_families_and_back(alone, n_points):
    import rustsasa_amd
    with rustsasa_amd.Context(0) as ctx:
        for step, family in enumerate(ORDER + ORDER[::-1]):
            for name in ("B", "A", "C"):  # grows the buffers, reuses them oversized, then a batch
                got = _call(ctx, family, _inputs()[name], n_points)
                assert _same(got, alone[(family, name, n_points)]), (step, family, name)


# ---- input B against the models ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_points", N_POINTS)
def test_fixture_equals_the_models(alone, n_points):
    x, y, z, r, ids, _, _ = _inputs()["B"]
    mask = pm.exposed_masks(x, y, z, r, ids, PROBE, n_points, 8)
    free_want = mask.sum(axis=1).astype(np.uint32)
    words, sasa = alone[("points", "B", n_points)]
    assert np.array_equal(words, pm.pack(mask))
    assert sasa.tobytes() == pm.sasa_of(r, PROBE, free_want, n_points).tobytes()
    depth, nearest, free, _ = alone[("depth", "B", n_points)]
    want_depth, want_nearest, _ = dm.atom_depth(x, y, z, r, ids, PROBE, n_points, mask=mask)
    assert np.array_equal(free, free_want) and np.array_equal(nearest, want_nearest)
    assert depth.tobytes() == want_depth.tobytes()
    offsets, labels, free, _ = alone[("components", "B", n_points)]
    want_off, want_labels, _ = cm.components(x, y, z, r, ids, PROBE, n_points, _link(r, n_points), mask=mask)
    assert np.array_equal(free, free_want) and np.array_equal(offsets, want_off) and np.array_equal(labels, want_labels)
    up, down = alone[("hse", "B", n_points)]
    want_up, want_down = hm.counts(x, y, z, _dirs(len(x)), None, HSE_CUTOFF)
    assert up.tobytes() == want_up.tobytes() and down.tobytes() == want_down.tobytes() and up.any() and down.any()
    within = wm.lists(x, y, z, None, WITHIN_CUTOFF)
    assert _same(alone[("within", "B", n_points)], within)
    assert _same(alone[("nearest", "B", n_points)], nm.truncate(*wm.lists(x, y, z, None, float("inf")), NEAREST_K))
    assert wm.lengths(within[0]).max() > NEAREST_K
    offsets, entries, owned, value, owner = alone[("owners", "B", n_points)]
    want = om.owners(x, y, z, r, ids, PROBE, n_points, 8)
    nh.assert_same((offsets, entries), want[:2])
    assert np.array_equal(owned, want[2]) and np.array_equal(owner, want[3]) and owned.any()
    assert np.array_equal((owner == om.FREE).sum(axis=1).astype(np.uint32), free_want)
    assert value.tobytes() == pm.sasa_of(r, PROBE, free_want, n_points).tobytes()
    table, pairs = alone[("radial", "B", n_points)]
    want = rm.counts(x, y, z, rc.EDGES, _classes(len(x)), RADIAL_CLASSES, None)
    assert table.dtype == want.dtype and np.array_equal(table, want) and table.any(axis=(0, 2)).all()
    assert np.array_equal(pairs, rm.pairs_from_counts(want, [0, len(x)], _classes(len(x))))
