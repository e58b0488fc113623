"""Exposure vectors on the GPU (rsasa_exposure_vectors*, k_exposure_vectors of points.hip) against the exact CPU model
(exposure_model.vectors_of on the masks of points_model.py).  The float32 summation order is part of the interface, so
every comparison of vectors and values is one of bit patterns (np.array_equal on view(uint32), tobytes): no tolerance.
The cases sit on the kernel's own edges:

  - 64 points per chunk, NCH chunks per pass, NCH = 2 up to 128 points and 4 above: 1, 63 / 64 / 65, 128 / 129,
    256 / 257 (the second pass of NCH = 4), 960; 100 points with a remainder of 4 (W = 8), none (W = 1) and 4 of 16
  - the list staged in LDS 256 entries at a time: lists of 5, 256 and 512 entries, five stages on 1jcd at probe 33, and an
    empty list
  - the early exit of a pass: atoms with no exposed point, whose three sums are exactly +0.0
  - batches, shared ids, non-finite input, argument errors, and a device batch in flight across a call."""
import numpy as np
import pytest

import bench_workloads as bw
import exposure_model as em
import nb_helpers as nh
import point_edge_cases as pe
import points_model as pm

pytestmark = pytest.mark.gpu

F = np.float32
# (n_points, W): chunk edges, the remainder rule at 100 points, both sides of the launcher's split, the second pass, 960
EDGE_CASES = ((1, 8), (63, 8), (64, 8), (65, 8), (100, 8), (100, 1), (100, 16), (128, 8), (129, 8), (256, 8), (257, 8),
              (960, 8))
CLUSTERS = (6, 257, 513)           # K = 5, 256, 512 (point_edge_cases.CLUSTER_SIZES)
LIST_POINTS = (100, 129)
FULL_LIST_SETTING = "probe_33"


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def jcd():
    return pe.fixture("1jcd.pdb")


@pytest.fixture(scope="module")
def jcd_masks(jcd):
    """{(n_points, W): model mask} of 1jcd at probe 1.4 for every edge case, computed once."""
    by_n = {}
    for n, W in EDGE_CASES:
        by_n.setdefault(n, []).append(W)
    got = pe.pmap(lambda n: pm.exposed_masks_ws(*jcd, 1.4, n, tuple(by_n[n])), by_n)
    return {(n, W): got[n][W] for n, W in EDGE_CASES}


def _check_shapes(got, n_atoms):
    vectors, free, sasa = got
    assert vectors.dtype == F and vectors.shape == (n_atoms, 3)
    assert free.dtype == np.uint32 and free.shape == (n_atoms,)
    assert sasa.dtype == F and sasa.shape == (n_atoms,)


def _check_against_mask(got, mask, r, probe, n_points):
    """vectors, free and sasa of a call against the model on `mask`."""
    _check_shapes(got, len(mask))
    vectors, free, sasa = got
    assert np.array_equal(free, mask.sum(axis=1).astype(np.uint32))
    want = em.vectors_of(mask, n_points)
    assert np.array_equal(em.bits(vectors), em.bits(want)), n_points
    assert sasa.tobytes() == pm.sasa_of(r, probe, free, n_points).tobytes()


def _far_atom(cols, dy=500.0):
    """`cols` and one atom 500 A off in y: its list is empty."""
    x, y, z, r, ids = cols
    cat = lambda a, v, t: np.ascontiguousarray(np.append(a, v).astype(t))  # noqa: E731
    return (cat(x, x[0], F), cat(y, y.max() + dy, F), cat(z, z[0], F), cat(r, 1.7, F),
            cat(ids, 7 * 10 ** 6, np.uint64))


def _full_sum(n_points):
    return em.vectors_of(np.ones((1, n_points), bool), n_points)[0]


# ---- 1: point counts around chunks, passes and the two instantiations ----------------------------------------------

@pytest.mark.parametrize("n_points,W", EDGE_CASES)
def test_point_count_edges(ctx, jcd, jcd_masks, n_points, W):
    mask = jcd_masks[(n_points, W)]
    try:
        ctx.set_simd_width(W)
        got = ctx.exposure_vectors(*jcd, 1.4, n_points)
        words, _ = ctx.accessible_points(*jcd, 1.4, n_points)
        soa = ctx.calculate_sasa_soa(*jcd, 1.4, n_points)
    finally:
        ctx.set_simd_width(8)
    _check_against_mask(got, mask, jcd[3], 1.4, n_points)
    assert np.array_equal(got[1].astype(np.int64), pe.popcount(words))
    assert got[2].tobytes() == soa.tobytes()
    assert 0 < int(got[1].sum()) < mask.size and (got[1] == 0).any()   # exposed and buried atoms both


def test_edge_case_classes():
    ns = {n for n, _ in EDGE_CASES}
    assert {1, 63, 64, 65, 128, 129, 256, 257, 960} <= ns
    assert pe.nch(128) == 2 and pe.nch(129) == 4 and -(-257 // 64) == 5 > 4       # 257: a second pass of one chunk
    assert {W for n, W in EDGE_CASES if n == 100} == {1, 8, 16}


# ---- 2: list lengths around the LDS stage, and an empty list -------------------------------------------------------

@pytest.mark.parametrize("n_points", LIST_POINTS)
@pytest.mark.parametrize("n", CLUSTERS)
def test_cluster_list_lengths_and_an_empty_list(ctx, n, n_points):
    assert n in pe.CLUSTER_SIZES
    base, c0 = nh.tight_cluster(n, seed=n)
    cols = _far_atom(base)
    lists = nh.oracle_csr(*cols, 1.4)
    k = np.diff(lists[0].astype(np.int64))
    assert k[c0:-1].min() == k[c0:-1].max() == n - 1 and k[-1] == 0 and k[:c0].max() < pe.PT_STAGE
    mask = pm.exposed_masks(*cols, 1.4, n_points, 8, lists)
    got = ctx.exposure_vectors(*cols, 1.4, n_points)
    _check_against_mask(got, mask, cols[3], 1.4, n_points)
    # the far atom: every point a term
    assert got[1][-1] == n_points and np.array_equal(em.bits(got[0][-1]), em.bits(_full_sum(n_points)))


@pytest.fixture(scope="module")
def full_list_masks():
    """(list lengths, {n_points: model mask}) of the full-list input, the lists built once and the masks side by side."""
    cols, probe = pe.full_list_cols(FULL_LIST_SETTING)
    lists = nh.oracle_csr(*cols, probe)
    return np.diff(lists[0].astype(np.int64)), pe.pmap(lambda n: pm.exposed_masks(*cols, probe, n, 8, lists), LIST_POINTS)


@pytest.mark.parametrize("n_points", LIST_POINTS)
def test_lists_of_every_atom(ctx, full_list_masks, n_points):
    """1jcd at probe 33: lists of 866 .. 1 051 entries, four and five stages; most atoms are buried completely (the early
    exit fires, and the next pass stages again from entry 0), some sweep every stage."""
    cols, probe = pe.full_list_cols(FULL_LIST_SETTING)
    pe.assert_full_lists(FULL_LIST_SETTING, full_list_masks[0])
    mask = full_list_masks[1][n_points]
    assert 0 < mask.sum() < 0.5 * mask.size and int((~mask.any(axis=1)).sum()) > len(mask) // 2
    got = ctx.exposure_vectors(*cols, probe, n_points)
    _check_against_mask(got, mask, cols[3], probe, n_points)
    assert not em.bits(got[0][got[1] == 0]).any()


# ---- 3: the early exit: no exposed point, three sums of exactly +0.0 -----------------------------------------------

@pytest.mark.parametrize("n_points", [100, 257])
def test_buried_atoms_have_exactly_positive_zero(ctx, n_points):
    f = lambda *a: np.array(a, F)  # noqa: E731
    # atom 0 inside atom 1: one entry buries every point of every pass
    pair = (f(0, 0.1), f(0, 0), f(0, 0), f(1.0, 3.0), None)
    vectors, free, sasa = ctx.exposure_vectors(*pair, 1.4, n_points)
    assert free.tolist() == [0, n_points] and sasa[0] == 0.0
    assert em.bits(vectors[0]).tolist() == [0, 0, 0]       # +0.0: bits 0x00000000, not -0.0
    assert np.array_equal(em.bits(vectors[1]), em.bits(_full_sum(n_points)))
    # the coincident atoms of a cluster (lists of 299 entries, two stages): the smaller ones lie inside the largest
    cols, c0 = nh.tight_cluster(300, seed=300)
    mask = pm.exposed_masks(*cols, 1.4, n_points, 8)
    buried = ~mask.any(axis=1)
    assert buried[c0:].sum() >= 7 and mask[c0:].any()
    got = ctx.exposure_vectors(*cols, 1.4, n_points)
    _check_against_mask(got, mask, cols[3], 1.4, n_points)
    assert np.array_equal(got[1] == 0, buried)
    assert not em.bits(got[0][buried]).any()
    assert em.bits(got[0][~buried]).any(axis=1).all()       # ... and an exposed atom is no zero vector here


# ---- 4: batches ----------------------------------------------------------------------------------------------------

def _batch(parts):
    so = np.zeros(len(parts) + 1, np.uint32)
    so[1:] = np.cumsum([len(p[0]) for p in parts])
    return [np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in range(5)], so


def test_mixed_batch_equals_per_structure(ctx, jcd):
    empty = (np.zeros(0, F),) * 4 + (np.zeros(0, np.uint64),)
    one = (np.array([1.0], F), np.array([2.0], F), np.array([3.0], F), np.array([1.5], F), np.array([1], np.uint64))
    parts = [empty, one, jcd, nh.tight_cluster(6, seed=6)[0], nh.tight_cluster(257, seed=257)[0]]
    cat, so = _batch(parts)
    for n_points in (100, 129):
        got = ctx.exposure_vectors_batch(*cat, so, 1.4, n_points)
        _check_shapes(got, int(so[-1]))
        for s, p in enumerate(parts):
            b, e = int(so[s]), int(so[s + 1])
            if e == b:
                continue
            single = ctx.exposure_vectors(*p, 1.4, n_points)
            for k in range(3):
                assert got[k][b:e].tobytes() == single[k].tobytes(), (n_points, s, k)
        # the lone atom
        assert got[1][so[1]] == n_points and np.array_equal(em.bits(got[0][so[1]]), em.bits(_full_sum(n_points)))
    # an empty batch and a batch of empty structures
    for so0 in ([0], [0, 0, 0]):
        got = ctx.exposure_vectors_batch(*empty, np.array(so0, np.uint32), 1.4, 100)
        _check_shapes(got, 0)


def test_batch_with_shared_ids_equals_the_model(ctx, jcd):
    """Atoms that share an id never occlude each other: the first third of each cluster shares one."""
    parts = [nh.tight_cluster(20, seed=20, shared_ids=True)[0], jcd, nh.tight_cluster(300, seed=300, shared_ids=True)[0]]
    cat, so = _batch(parts)
    n_points = 100
    mask = pm.exposed_masks_batch(*cat, so, 1.4, n_points, 8)
    got = ctx.exposure_vectors_batch(*cat, so, 1.4, n_points)
    _check_against_mask(got, mask, cat[3], 1.4, n_points)
    without = pm.exposed_masks_batch(*cat[:4], None, so, 1.4, n_points, 8)
    assert not np.array_equal(mask, without)               # (the ids do change the result)


# ---- 5: non-finite input and argument errors -----------------------------------------------------------------------

def test_nan_coordinate_and_radius(ctx, jcd):
    x, y, z, r, ids = jcd
    x, r = x.copy(), r.copy()
    x[5] = np.nan
    r[17] = np.nan
    for n_points in (100, 129):
        mask = pm.exposed_masks(x, y, z, r, ids, 1.4, n_points, 8)
        assert mask[5].all() and mask[17].all()
        vectors, free, sasa = ctx.exposure_vectors(x, y, z, r, ids, 1.4, n_points)
        full = em.bits(_full_sum(n_points))
        assert free[5] == n_points and free[17] == n_points
        assert np.array_equal(em.bits(vectors[5]), full) and np.array_equal(em.bits(vectors[17]), full)
        assert np.isnan(sasa[17]) and not np.isnan(sasa[5])
        assert np.array_equal(free, mask.sum(axis=1).astype(np.uint32))
        assert np.array_equal(em.bits(vectors), em.bits(em.vectors_of(mask, n_points)))
        want, _ = ctx.calculate_sasa_batch(x, y, z, r, ids, np.array([0, len(x)], np.uint32), 1.4, n_points)
        assert sasa.tobytes() == want.tobytes()


def test_infinite_coordinate_then_usable(ctx, jcd, jcd_masks):
    import rustsasa_amd
    x, y, z, r, ids = jcd
    bad = x.copy()
    bad[3] = np.inf
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.exposure_vectors(bad, y, z, r, ids, 1.4, 100)
    assert e.value.status == -5
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.exposure_vectors_batch(bad, y, z, r, ids, np.array([0, len(x)], np.uint32), 1.4, 100)
    assert e.value.status == -5
    _check_against_mask(ctx.exposure_vectors(x, y, z, r, ids, 1.4, 100), jcd_masks[(100, 8)], r, 1.4, 100)


def test_argument_errors_from_the_library(ctx, jcd, jcd_masks):
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    lib = _capi.load()
    x, y, z, r, ids = jcd
    n = len(x)
    v, k = np.zeros((n, 3), F), np.zeros(n, np.uint32)
    cols = (ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids))
    bad = _capi.RSASA_ERR_INVALID_ARGUMENT
    assert lib.rsasa_exposure_vectors(ctx._h, *cols, n, 1.4, 0, ptr(v), ptr(k), None) == bad
    assert lib.rsasa_exposure_vectors(ctx._h, *cols, n, 1.4, 100, None, ptr(k), None) == bad
    assert lib.rsasa_exposure_vectors(ctx._h, *cols, n, 1.4, 100, ptr(v), None, None) == bad
    assert lib.rsasa_exposure_vectors(ctx._h, *cols, n, -5.0, 100, ptr(v), ptr(k), None) == bad   # probe + max_r <= 0
    so = np.array([0, n], np.uint32)
    assert lib.rsasa_exposure_vectors_batch(ctx._h, *cols, ptr(so), 1, 1.4, 0, ptr(v), ptr(k), None) == bad
    assert lib.rsasa_exposure_vectors_batch(ctx._h, *cols, ptr(so), 1, 1.4, 100, None, ptr(k), None) == bad
    assert lib.rsasa_exposure_vectors_batch(ctx._h, *cols, ptr(so), 1, 1.4, 100, ptr(v), None, None) == bad
    assert lib.rsasa_exposure_vectors_batch(ctx._h, *cols, None, 1, 1.4, 100, ptr(v), ptr(k), None) == bad
    down = np.array([0, 600, 500, n], np.uint32)
    assert lib.rsasa_exposure_vectors_batch(ctx._h, *cols, ptr(down), 3, 1.4, 100, ptr(v), ptr(k), None) == bad
    assert not v.any() and not k.any()                     # nothing was written
    # out_sasa is optional; the context is still usable
    assert lib.rsasa_exposure_vectors(ctx._h, *cols, n, 1.4, 100, ptr(v), ptr(k), None) == _capi.RSASA_OK
    mask = jcd_masks[(100, 8)]
    assert np.array_equal(k, mask.sum(axis=1).astype(np.uint32))
    assert np.array_equal(em.bits(v), em.bits(em.vectors_of(mask, 100)))


# ---- 6: next to a device batch in flight ---------------------------------------------------------------------------

def test_device_batch_in_flight_undisturbed(ctx, jcd, jcd_masks):
    torch = pytest.importorskip("torch")
    b = bw.synthetic_proteome(12, seed=4)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cols = (t(b.x), t(b.y), t(b.z), t(b.radius), t(b.ids.view(np.int64)))
    alone = torch.zeros(b.n_atoms, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.enqueue_device(*cols, b.structure_offsets, out_atom_sasa=alone, probe_radius=1.4, n_points=100)
    ctx.wait()
    out = torch.zeros(b.n_atoms, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.enqueue_device(*cols, b.structure_offsets, out_atom_sasa=out, probe_radius=1.4, n_points=100)
    got = ctx.exposure_vectors(*jcd, 1.4, 100)
    ctx.wait()
    assert out.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    _check_against_mask(got, jcd_masks[(100, 8)], jcd[3], 1.4, 100)


# ---- 7: the volume from the GPU's vectors --------------------------------------------------------------------------

def test_volume_from_gpu_vectors_equals_volume_from_model_vectors(ctx, jcd, jcd_masks):
    import rustsasa_amd
    x, y, z, r, ids = jcd
    vectors, free, _ = ctx.exposure_vectors(x, y, z, r, ids, 1.4, 100)
    mask = jcd_masks[(100, 8)]
    got = rustsasa_amd.sas_volume(vectors, free, x, y, z, r, 1.4, 100)
    want = rustsasa_amd.sas_volume(em.vectors_of(mask, 100), mask.sum(axis=1).astype(np.uint32), x, y, z, r, 1.4, 100)
    assert got[0][0] == want[0][0] and got[1][0] == want[1][0] and got[0][0] > 0.0
