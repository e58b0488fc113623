"""Neighbour lists (rsasa_precompute_neighbors*, neighbors.hip) at the edges of their own kernels and host code, byte
for byte against the oracle (and the plain model, tests/neighbor_model.py, where a case is small):

  - the fill kernel's LDS staging of 512 keys (kNbStage) and the spill ranking's 256-key tiles and grid stride
  - the count scan's chunks (256 counts per block up to 262 144 atoms, more beyond: the carry across tiles)
  - exact cutoffs of the membership rule (nb_accept: d^2 == max_search^2, d^2 == sr^2) and cell faces
  - max_radius overrides: equal to the fold maximum, negative, huge (ms^2 = +inf), invalid; an explicit NaN is "no
    override" (the fold maximum), as documented in include/rustsasa_amd.h
  - grid edges: 16-bit and 32-bit cell starts, whole windows, grids over 1 024 cells long, flat grids, corner cells
  - one context through calls of different sizes and kinds (the nb_* workspace), degenerate inputs.

Every result is also checked for its invariants: offsets[0] == 0, non-decreasing, offsets[-1] == len(entries), and
every idx below its structure's size."""
import numpy as np
import pytest

import bench_workloads as bw
import neighbor_model as nm
import tie_cases as tc
from nb_helpers import (PROBE, assert_same, check_invariants, fold_max, oracle_active_csr, oracle_batch_csr,
                        oracle_csr, protor, scan_chunk, scan_input, tight_cluster)

pytestmark = pytest.mark.gpu

NB_STAGE = 512  # keys one wave stages in LDS in k_neighbor_fill (kNbStage, neighbors.hip); longer lists spill
SPILL_GRID = 4096  # k_neighbor_rank_spill's grid is capped at 4 096 workgroups, one list each per round


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


def _lens(offs):
    return np.diff(offs.astype(np.int64))


def list_sizes(so):
    """The size of each list's structure (check_invariants' bound on idx)."""
    k = np.diff(np.asarray(so, np.int64))
    return np.repeat(k, k)


def single(ctx, x, y, z, r, ids, probe=PROBE, max_radius=None, model=False, **kw):
    """One precompute_neighbors call checked against the oracle (and the model); returns the result."""
    got = ctx.precompute_neighbors(x, y, z, r, ids, probe, max_radius=max_radius, **kw)
    check_invariants(got, len(x))
    assert_same(got, oracle_csr(x, y, z, r, ids, probe, max_radius))
    if model:
        assert_same(got, nm.neighbor_csr(x, y, z, r, ids, probe, max_radius))
    return got


def batch(ctx, x, y, z, r, ids, so, probe=PROBE, max_radius=None, model=False):
    """One precompute_neighbors_batch call checked against the oracle structure by structure."""
    got = ctx.precompute_neighbors_batch(x, y, z, r, ids, so, probe, max_radius=max_radius)
    check_invariants(got, list_sizes(so))
    assert_same(got, oracle_batch_csr(x, y, z, r, ids, so, probe, max_radius))
    if model:
        offs, ent = got
        for s in range(len(so) - 1):
            b, e = int(so[s]), int(so[s + 1])
            lo, hi = int(offs[b]), int(offs[e])
            assert_same((offs[b:e + 1] - offs[b], ent[lo:hi]),
                        nm.neighbor_csr(x[b:e], y[b:e], z[b:e], r[b:e], None if ids is None else ids[b:e], probe,
                                        max_radius))
    return got


def pack_columns(parts):
    so = np.zeros(len(parts) + 1, np.uint32)
    so[1:] = np.cumsum([len(p[0]) for p in parts])
    cat = [np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in range(5)]
    return cat, so


# ---- 1. the LDS staging, the spill ranking's tiles and grid stride ----------------------------------------------

@pytest.mark.parametrize("n", [2, 64, 65, 66, 512, 513, 514, 768, 769, 770])
def test_cluster_list_lengths_around_staging_and_tiles(ctx, n):
    """K = n - 1: 511 / 512 / 513 around the staging, 767 / 768 / 769 around the spill ranking's 256-key tiles."""
    cols, c0 = tight_cluster(n, seed=n)
    offs, _ = single(ctx, *cols, model=n >= 512)
    assert np.all(_lens(offs)[c0:] == n - 1)
    assert (n - 1 > NB_STAGE) == (int(_lens(offs).max()) > NB_STAGE)


def test_cluster_with_more_spilled_lists_than_the_spill_grid(ctx):
    """About 4 200 lists of 4 199 entries: more spilled lists than workgroups, so the grid-stride loop runs twice."""
    n = 4200
    cols, c0 = tight_cluster(n, seed=7, protein="example.cif")
    offs, _ = single(ctx, *cols)
    k = _lens(offs)
    assert np.all(k[c0:] == n - 1)
    assert int(np.sum(k > NB_STAGE)) > SPILL_GRID


def test_cluster_with_shared_ids_in_spilled_lists(ctx):
    n = 1100
    cols, c0 = tight_cluster(n, seed=11, shared_ids=True)
    offs, _ = single(ctx, *cols, model=True)
    k = _lens(offs)[c0:]
    assert k.min() == n - n // 3 and k.max() == n - 1 and k.min() > NB_STAGE


def test_real_structure_with_lists_on_both_sides_of_the_staging(ctx):
    """151L_H3 at max_radius 10: lists of 118 to 617 entries, some above the staging (both routes in one structure);
    1jcd at the same value stays below it."""
    x, y, z, r, ids = protor("151L_H3.pdb")
    k = _lens(single(ctx, x, y, z, r, ids, max_radius=10.0, model=True)[0])
    assert k.min() < NB_STAGE < k.max() and int(np.sum(k > NB_STAGE)) >= 10
    x, y, z, r, ids = protor("1jcd.pdb")
    k = _lens(single(ctx, x, y, z, r, ids, max_radius=10.0)[0])
    assert k.max() <= NB_STAGE


# ---- 2. the count scan's chunks ---------------------------------------------------------------------------------

_scan_input = scan_input


SCAN_SIZES = [262144, 262145, 524289]
SCAN_PROBE = 0.0  # (short lists: the scan, not the lists, is under test here)


_chunk = scan_chunk


@pytest.mark.parametrize("kind", ["single", "batch"])
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_sizing_call_offsets(ctx, n, kind):
    """Chunks of 256, 512 and 768 counts per scan block: several tiles per block (the running carry), a partial last
    tile and empty trailing blocks.  The sizing call (out_entries NULL: count and scan, no fill) returns the offsets
    and RSASA_ERR_BUFFER_TOO_SMALL."""
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    assert _chunk(n) == {262144: 256, 262145: 512, 524289: 768}[n]
    x, y, z, r, ids, so = _scan_input(n, kind)
    want = oracle_batch_csr(x, y, z, r, ids, so, SCAN_PROBE)[0]
    offs = np.zeros(n + 1, np.uint64)
    rc = _capi.load().rsasa_precompute_neighbors_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so),
                                                       len(so) - 1, SCAN_PROBE, float("nan"), ptr(offs), None, 0)
    assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL
    assert np.array_equal(offs, want)


@pytest.mark.parametrize("kind", ["single", "batch"])
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_chunks_full_lists(ctx, n, kind):
    x, y, z, r, ids, so = _scan_input(n, kind)
    if kind == "single":
        single(ctx, x, y, z, r, ids, SCAN_PROBE)
    else:
        batch(ctx, x, y, z, r, ids, so, SCAN_PROBE)


# ---- 3. exact cutoffs -------------------------------------------------------------------------------------------

def _cutoff_structures():
    """The tie cases' candidate cutoffs (d^2 == sr^2 exactly among them) and cell-face layouts, grouped by probe."""
    by_probe = {}
    for case in tc.generate()["cutoff"]:
        by_probe.setdefault(case.probe, []).extend(case.structures)
    return by_probe


def test_exact_sr_cutoffs_and_cell_faces_in_packed_batches(ctx):
    cases = tc.generate()["cutoff"]
    assert sum(c.family == "cutoff" and c.tie for c in cases) >= 20  # d^2 == sr^2 exactly
    assert sum(c.family == "cellface" for c in cases) >= 40
    n = 0
    for probe, sts in _cutoff_structures().items():
        batch(ctx, *tc.pack(sts), probe, model=True)
        n += len(sts)
    assert n >= 200


def test_exact_sr_cutoffs_singly(ctx):
    cases = [c for c in tc.generate()["cutoff"] if c.tie][:10]
    for c in cases:
        for st in c.structures:
            single(ctx, *st.soa(), c.probe, model=True)


def test_exact_max_search_cutoffs(ctx):
    """d^2 == max_search^2 exactly, max_radius below r_0: atom 1 listed for atom 0 at the flip and one f32 step above,
    not one or two steps below (tie_cases.ms_cutoffs, each side confirmed by the oracle)."""
    cases = tc.ms_cutoffs()
    assert len(cases) >= 20
    for c in cases:
        d = [c.st.x[0] - c.st.x[1], c.st.y[0] - c.st.y[1], c.st.z[0] - c.st.z[1]]
        ms = np.float32(c.m_in) + np.float32(c.m_in) + np.float32(2.0) * np.float32(c.probe)
        assert d[0] * d[0] + d[1] * d[1] + d[2] * d[2] == ms * ms
        for mr, listed in [(v, True) for v in c.inside] + [(v, False) for v in c.outside]:
            offs, ent = single(ctx, *c.st.soa(), c.probe, max_radius=mr, model=True)
            assert (1 in ent["idx"][int(offs[0]):int(offs[1])].tolist()) == listed


# ---- 4. max_radius ----------------------------------------------------------------------------------------------

def test_max_radius_equal_to_fold_max_and_nan_are_none(ctx):
    x, y, z, r, ids = protor("1jcd.pdb")
    r = r.copy()
    r[17] = np.nan  # (skipped by the fold)
    want = single(ctx, x, y, z, r, ids)
    assert_same(ctx.precompute_neighbors(x, y, z, r, ids, PROBE, max_radius=fold_max(r)), want)
    assert_same(ctx.precompute_neighbors(x, y, z, r, ids, PROBE, max_radius=float("nan")), want)
    so = np.array([0, len(x)], np.uint32)
    assert_same(ctx.precompute_neighbors_batch(x, y, z, r, ids, so, PROBE, max_radius=float("nan")), want)


def test_negative_max_radius(ctx):
    x, y, z, r, ids = protor("1jcd.pdb")
    offs, _ = single(ctx, x, y, z, r, ids, max_radius=-0.5, model=True)
    assert 0 < int(offs[-1])


def test_huge_max_radius_lists_every_pair(ctx):
    """max_radius 1e30: ms^2 and sr^2 overflow to +inf and the grid is 3 cells wide, so every atom lists every other
    atom; two atoms 4e19 A apart have d^2 = +inf and still pass."""
    x, y, z, r, ids = protor("1jcd.pdb")
    x, y, z = (np.ascontiguousarray(a[:300]) for a in (x, y, z))
    x = np.append(x, np.float32([2e19, -2e19]))
    y, z = np.append(y, np.float32([0, 0])), np.append(z, np.float32([0, 0]))
    r = np.append(r[:300], np.float32([1.5, 1.5]))
    ids = np.arange(1, 303, dtype=np.uint64)
    offs, ent = single(ctx, x, y, z, r, ids, max_radius=1e30, model=True)
    n = len(x)
    assert np.all(_lens(offs) == n - 1)
    far = ent[int(offs[n - 1]):]  # every key of the far atom's list is d^2 = +inf: ordered by idx alone
    assert np.array_equal(far["idx"], np.arange(n - 1))


@pytest.mark.parametrize("max_radius", [-1.4, -2.0, float("inf"), float("-inf")])
def test_invalid_max_radius_then_usable(ctx, max_radius):
    import rustsasa_amd
    x, y, z, r, ids = protor("1jcd.pdb")
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.precompute_neighbors(x, y, z, r, ids, PROBE, max_radius=max_radius)
    assert e.value.status == -1
    so = np.array([0, len(x)], np.uint32)
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.precompute_neighbors_batch(x, y, z, r, ids, so, PROBE, max_radius=max_radius)
    assert e.value.status == -1
    single(ctx, x, y, z, r, ids)


# ---- 5. grid edges ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_atoms", [65535, 65536])
def test_largest_structure_binned_in_lds_and_smallest_that_is_not(ctx, n_atoms):
    """65 535 atoms: 16-bit relative cell starts; 65 536: absolute 32-bit ones (nb_runs' two loads)."""
    rng = np.random.default_rng(n_atoms)
    xyz = rng.uniform(0, 110, size=(n_atoms, 3)).astype(np.float32)
    r = rng.uniform(1.2, 2.0, n_atoms).astype(np.float32)
    single(ctx, *(np.ascontiguousarray(xyz[:, k]) for k in range(3)), r, np.arange(n_atoms, dtype=np.uint64))


@pytest.mark.parametrize("dims_z", [16, 32])
def test_grid_of_exactly_whole_windows(ctx, dims_z):
    """cell 3.0; dims 48 x 48 x dims_z = one / two windows of 36 864 cells exactly."""
    rng = np.random.default_rng(dims_z)
    box = np.array([134.0, 134.0, 38.0 if dims_z == 16 else 86.0])
    xyz = rng.uniform(0, 1, size=(6000, 3)) * box
    xyz[0] = 0.0
    xyz[1] = box
    xyz = xyz.astype(np.float32)
    r = np.full(len(xyz), 1.6, np.float32)
    ids = np.arange(len(xyz), dtype=np.uint64)
    cell, inv, _ = nm.grid_params(PROBE, 1.6)
    dims = [int(np.ceil(float((xyz[:, k].max() + cell - (xyz[:, k].min() - cell)) * inv))) + 1 for k in range(3)]
    assert dims == [48, 48, dims_z]
    single(ctx, *(np.ascontiguousarray(xyz[:, k]) for k in range(3)), r, ids)


def test_grids_longer_than_1024_cells_along_each_axis(ctx):
    b = bw.synthetic_proteome(6, seed=9)
    so = b.structure_offsets
    x, y, z = b.x.copy(), b.y.copy(), b.z.copy()
    for s, axis in ((1, x), (3, y), (4, z)):
        half = (so[s] + so[s + 1]) // 2
        axis[half:so[s + 1]] += np.float32(4000.0)  # > 1024 cells of probe + max_r between the halves
    batch(ctx, x, y, z, b.radius, b.ids, so)


def _flat_and_corner_structures(rng):
    """Structures one cell layer thick along z, along y and z (a line), atoms in the corner cells of a box, a lone
    atom and a pair."""
    out = []
    xy = rng.uniform(0, 40, (400, 2))
    out.append(np.column_stack([xy, np.full(400, 5.0)]))                         # a plane
    out.append(np.column_stack([rng.uniform(0, 60, 120), np.full(120, -3.0), np.full(120, 7.0)]))  # a line
    box = np.array([30.0, 22.0, 17.0])
    corners = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], float) * box
    near = corners[:, None, :] + rng.uniform(-1.0, 1.0, (8, 6, 3))               # neighbours of every corner
    inner = rng.uniform(0, 1, (300, 3)) * box
    out.append(np.concatenate([corners, np.clip(near.reshape(-1, 3), 0, box), inner]))
    out.append(np.array([[1.0, 2.0, 3.0]]))
    out.append(np.array([[1.0, 2.0, 3.0], [3.5, 2.0, 3.0]]))
    parts = []
    for xyz in out:
        xyz = xyz.astype(np.float32)
        n = len(xyz)
        parts.append((xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy(), rng.uniform(1.2, 2.0, n).astype(np.float32),
                      np.arange(1, n + 1, dtype=np.uint64)))
    return parts


@pytest.mark.parametrize("probe", [PROBE, 0.0])
def test_flat_grids_and_corner_cells(ctx, probe):
    parts = _flat_and_corner_structures(np.random.default_rng(23))
    for p in parts:
        single(ctx, *p, probe, model=True)
    cat, so = pack_columns(parts)
    batch(ctx, *cat, so, probe, model=True)


# ---- 6. one context, many calls ---------------------------------------------------------------------------------

def test_one_context_through_calls_of_every_kind():
    """A fresh context (its remembered cell capacity starts from its first call): big, small, big; with and without
    ids; with and without active_indices; a sparse structure that overflows the remembered cells (regrow and run
    again); a call that fails on an infinite coordinate; then the first calls again."""
    import rustsasa_amd
    big = bw.synthetic_proteome(30, seed=8)
    bigc = (big.x, big.y, big.z, big.radius, big.ids, big.structure_offsets)
    small = protor("1jcd.pdb")
    mid = protor("151L_H3.pdb")
    rng = np.random.default_rng(31)
    sp = (rng.uniform(0, 1, (300, 3)) * np.array([30000.0, 100.0, 100.0])).astype(np.float32)  # ~9 M cells
    sparse = (sp[:, 0].copy(), sp[:, 1].copy(), sp[:, 2].copy(), rng.uniform(1.2, 2.0, 300).astype(np.float32),
              np.arange(300, dtype=np.uint64))
    act = rng.permutation(len(mid[0]))[:700].astype(np.uint32)
    want = {"big": oracle_batch_csr(*bigc), "small": oracle_csr(*small), "mid": oracle_csr(*mid),
            "mid_noid": oracle_csr(*mid[:4], None), "mid_act": oracle_active_csr(*mid, act),
            "sparse": oracle_csr(*sparse)}
    assert big.n_atoms * 20 < 9_000_000  # (the capacity a first call of `big` remembers is below the sparse grid's)
    with rustsasa_amd.Context(0) as c:
        run = {"big": lambda: c.precompute_neighbors_batch(*bigc, PROBE),
               "small": lambda: c.precompute_neighbors(*small, PROBE),
               "mid": lambda: c.precompute_neighbors(*mid, PROBE),
               "mid_noid": lambda: c.precompute_neighbors(*mid[:4], None, PROBE),
               "mid_act": lambda: c.precompute_neighbors(*mid, PROBE, active_indices=act),
               "sparse": lambda: c.precompute_neighbors(*sparse, PROBE)}
        seq = ["big", "small", "big", "mid", "mid_noid", "mid", "mid_act", "mid", "sparse", "inf", "small", "big",
               "mid_act", "sparse"]
        for step in seq:
            if step == "inf":
                bad = small[0].copy()
                bad[3] = np.inf
                with pytest.raises(rustsasa_amd.RsasaError) as e:
                    c.precompute_neighbors(bad, *small[1:], PROBE)
                assert e.value.status == -5
                continue
            got = run[step]()
            size = {"big": list_sizes(big.structure_offsets), "mid_act": len(mid[0])}.get(step, len(got[0]) - 1)
            check_invariants(got, size)
            assert_same(got, want[step])


# ---- 7. degenerate inputs ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["empty", "reversed", "single", "permutation"])
def test_active_indices_shapes(ctx, kind):
    x, y, z, r, ids = protor("1jcd.pdb")
    n = len(x)
    act = {"empty": np.zeros(0, np.uint32), "reversed": np.arange(n - 1, -1, -1, dtype=np.uint32),
           "single": np.array([n // 2], np.uint32),
           "permutation": np.random.default_rng(3).permutation(n).astype(np.uint32)}[kind]
    got = ctx.precompute_neighbors(x, y, z, r, ids, PROBE, active_indices=act)
    check_invariants(got, n)
    assert len(got[0]) == len(act) + 1
    assert_same(got, oracle_active_csr(x, y, z, r, ids, act))
    assert_same(got, nm.neighbor_csr(x, y, z, r, ids, PROBE, active_indices=act))
    if kind in ("empty", "single"):
        assert int(got[0][-1]) == 0


def test_no_structures_and_only_empty_structures(ctx):
    e = np.zeros(0, np.float32)
    offs, ent = ctx.precompute_neighbors_batch(e, e, e, e, np.zeros(0, np.uint64), np.zeros(1, np.uint32), PROBE)
    assert offs.tolist() == [0] and len(ent) == 0
    offs, ent = ctx.precompute_neighbors_batch(e, e, e, e, None, np.zeros(5, np.uint32), PROBE)
    assert offs.tolist() == [0] and len(ent) == 0
    offs, ent = ctx.precompute_neighbors_batch(e, e, e, e, None, np.zeros(5, np.uint32), 0.0)
    assert offs.tolist() == [0] and len(ent) == 0
    single(ctx, *protor("1jcd.pdb"))  # (and the context is still usable)


def test_thousands_of_tiny_structures(ctx):
    """Every structure of the tie cases (two to five atoms each) in one batch: structure-relative idx
    (orig - atom_begin) across thousands of grids."""
    sts = [st for case in tc.all_cases() for st in case.structures]
    assert len(sts) >= 3000
    x, y, z, r, ids, so = tc.pack(sts)
    got = batch(ctx, x, y, z, r, ids, so)
    assert int(got[0][-1]) > len(sts)
