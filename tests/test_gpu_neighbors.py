"""Neighbour lists on the GPU (rsasa_precompute_neighbors*, reference src/lib.rs:69-84, spatial_grid.rs:195-465)
against the oracle's lists, byte for byte.  The oracle keeps push order on distance ties (its insertion sort); the
engine's documented order is (d^2, idx), one of the orders the reference's sort_unstable_by may give, so the oracle's
lists are re-sorted by (d^2, idx) with a stable sort before the comparison."""
import numpy as np
import pytest

import bench_workloads as bw
import structio as sio
import tie_cases as tc
from nb_helpers import PROBE, assert_same, csr, fold_max, oracle_csr, protor, sorted_lists
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


# ---- the reference's unit case (tests/units.rs:132-209) ------------------------------------------------------------

def test_reference_unit_case(ctx):
    c = np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0], [20, 20, 20]], np.float32)
    x, y, z = (np.ascontiguousarray(c[:, k]) for k in range(3))
    r = np.full(4, 1.5, np.float32)
    ids = np.arange(1, 5, dtype=np.uint64)
    got = ctx.precompute_neighbors(x, y, z, r, ids, PROBE)
    lists = ctx.neighbor_lists(x, y, z, r, ids, PROBE)
    assert set(lists[0]["idx"].tolist()) == {1, 2}
    assert 0 in lists[1]["idx"] and 0 in lists[2]["idx"]
    assert len(lists[3]) == 0
    assert lists[0]["threshold_squared"][0] == np.float32(np.float32(1.5) + np.float32(1.4)) ** 2
    # the lists do not depend on the grid: the test's own grid and precompute_neighbors' agree
    assert_same(got, oracle_csr(x, y, z, r, ids, max_radius=1.5, cell_size=5.0, max_search_radius=1.5 + 1.5 + 2.8))
    assert_same(got, oracle_csr(x, y, z, r, ids))


# ---- fixtures ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("probe", [PROBE, 0.5])
def test_example_cif_vdw(ctx, probe):
    x, y, z, r, ids = sio.soa_vdw(sio.read_structure(sio.data_path("example.cif")))
    assert_same(ctx.precompute_neighbors(x, y, z, r, ids, probe), oracle_csr(x, y, z, r, ids, probe))


@pytest.mark.parametrize("name", ["1jcd.pdb", "151L_H3.pdb", "bad_seqadv_1A06.pdb", "example.cif"])
@pytest.mark.parametrize("probe", [PROBE, 3.0])
def test_fixtures_protor(ctx, name, probe):
    x, y, z, r, ids = protor(name)
    assert_same(ctx.precompute_neighbors(x, y, z, r, ids, probe), oracle_csr(x, y, z, r, ids, probe))


# ---- ids -----------------------------------------------------------------------------------------------------------

def test_duplicate_ids(ctx):
    x, y, z, r, ids = protor("1jcd.pdb")
    dup = (ids // np.uint64(3)).astype(np.uint64)  # every id shared by up to three neighbouring atoms
    want = oracle_csr(x, y, z, r, dup)
    assert_same(ctx.precompute_neighbors(x, y, z, r, dup, PROBE), want)
    assert want[0][-1] < oracle_csr(x, y, z, r, ids)[0][-1]


def test_colliding_id_folds(ctx):
    x, y, z, r, ids = protor("1jcd.pdb")
    ids = ids.astype(np.uint64).copy()
    # every second atom gets an id whose 32-bit fold equals its predecessor's: equal folds, different ids ...
    col = ids.copy()
    for i in range(1, len(col), 2):
        col[i] = tc.colliding_id(int(col[i - 1]), 0x1234 + i)
    assert_same(ctx.precompute_neighbors(x, y, z, r, col, PROBE), oracle_csr(x, y, z, r, col))
    # ... and some pairs with really equal ids among them
    col[1::6] = col[0::6][:len(col[1::6])]
    assert_same(ctx.precompute_neighbors(x, y, z, r, col, PROBE), oracle_csr(x, y, z, r, col))


def test_no_ids(ctx):
    x, y, z, r, _ = protor("151L_H3.pdb")
    assert_same(ctx.precompute_neighbors(x, y, z, r, None, PROBE), oracle_csr(x, y, z, r, None))


# ---- max_radius as given -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_radius", [2.5, 1.2])
def test_max_radius_given(ctx, max_radius):
    """Above the true maximum (1.88 for ProtOr carbons), and below it: there the max_search test binds."""
    x, y, z, r, ids = protor("1jcd.pdb")
    got = ctx.precompute_neighbors(x, y, z, r, ids, PROBE, max_radius=max_radius)
    assert_same(got, oracle_csr(x, y, z, r, ids, max_radius=max_radius))
    assert not np.array_equal(got[0], ctx.precompute_neighbors(x, y, z, r, ids, PROBE)[0])


# ---- active_indices ------------------------------------------------------------------------------------------------

def test_active_indices_subset(ctx):
    x, y, z, r, ids = protor("1jcd.pdb")
    rng = np.random.default_rng(11)
    act = rng.permutation(len(x))[: len(x) * 2 // 3].astype(np.uint32)
    got = ctx.precompute_neighbors(x, y, z, r, ids, PROBE, active_indices=act)
    # the reference bins only the active atoms: the oracle on the gathered subset, idx mapped back
    gx, gy, gz, gr, gi = x[act], y[act], z[act], r[act], ids[act]
    lists = po.neighbor_lists(gx, gy, gz, gr, gi, probe_radius=PROBE, max_radius=fold_max(gr))
    mapped = []
    for lst in lists:
        m = lst.copy()
        m["idx"] = act[lst["idx"]]
        mapped.append(m)
    want = csr(sorted_lists(mapped, x, y, z, centre_of=act))
    assert_same(got, want)
    assert len(got[0]) == len(act) + 1


def test_active_indices_invalid(ctx):
    import rustsasa_amd
    x, y, z, r, ids = protor("1jcd.pdb")
    for act in ([0, 1, 1], [0, len(x)]):
        with pytest.raises(rustsasa_amd.RsasaError) as e:
            ctx.precompute_neighbors(x, y, z, r, ids, PROBE, active_indices=np.array(act, np.uint32))
        assert e.value.status == -1
    assert_same(ctx.precompute_neighbors(x, y, z, r, ids, PROBE), oracle_csr(x, y, z, r, ids))


# ---- non-finite input and tiny inputs ------------------------------------------------------------------------------

def test_nan_coordinate_and_radius(ctx):
    x, y, z, r, ids = protor("1jcd.pdb")
    x, r = x.copy(), r.copy()
    x[5] = np.nan
    r[17] = np.nan
    got = ctx.precompute_neighbors(x, y, z, r, ids, PROBE)
    assert_same(got, oracle_csr(x, y, z, r, ids))
    offs, ent = got
    assert offs[6] == offs[5] and offs[18] == offs[17]  # both have empty lists
    assert 5 not in ent["idx"]                            # the NaN coordinate is nobody's neighbour
    assert np.isnan(ent["threshold_squared"][ent["idx"] == 17]).all() and (ent["idx"] == 17).any()


def test_zero_and_one_atom(ctx):
    e = np.zeros(0, np.float32)
    offs, ent = ctx.precompute_neighbors(e, e, e, e, None, PROBE)
    assert offs.tolist() == [0] and len(ent) == 0
    one = np.ones(1, np.float32)
    offs, ent = ctx.precompute_neighbors(one, one, one, one, np.ones(1, np.uint64), PROBE)
    assert offs.tolist() == [0, 0] and len(ent) == 0


def test_infinite_coordinate_then_usable(ctx):
    import rustsasa_amd
    x, y, z, r, ids = protor("1jcd.pdb")
    bad = x.copy()
    bad[3] = np.inf
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.precompute_neighbors(bad, y, z, r, ids, PROBE)
    assert e.value.status == -5
    assert_same(ctx.precompute_neighbors(x, y, z, r, ids, PROBE), oracle_csr(x, y, z, r, ids))


# ---- long lists: the global-memory staging -------------------------------------------------------------------------

def test_spill_path_cluster(ctx):
    """2 500 atoms inside one probe sphere plus a protein: K > 2 000, far above the fill kernel's LDS staging of 512
    keys (kNbStage, neighbors.hip): the cluster's lists are ranked in global scratch (k_neighbor_rank_spill)."""
    x, y, z, r, ids = protor("1jcd.pdb")
    rng = np.random.default_rng(5)
    n = 2500
    c = rng.uniform(-0.6, 0.6, size=(n, 3)).astype(np.float32) + np.array([x[0], y[0], z[0]], np.float32)
    c[:40] = c[0]  # a few coincident atoms: equal d^2, order by idx
    X = np.concatenate([x, c[:, 0]])
    Y = np.concatenate([y, c[:, 1]])
    Z = np.concatenate([z, c[:, 2]])
    R = np.concatenate([r, np.full(n, 1.6, np.float32)])
    I = np.concatenate([ids, np.arange(10 ** 6, 10 ** 6 + n, dtype=np.uint64)])
    got = ctx.precompute_neighbors(X, Y, Z, R, I, PROBE)
    assert int(np.max(np.diff(got[0].astype(np.int64)))) > 2000
    assert_same(got, oracle_csr(X, Y, Z, R, I))


# ---- batches -------------------------------------------------------------------------------------------------------

def test_batch_mixed_sizes(ctx):
    """Empty and one-atom structures, fixtures, and one structure of >= 65 536 atoms (the batch-wide binning)."""
    parts = [(np.zeros(0, np.float32),) * 4 + (np.zeros(0, np.uint64),)]
    parts.append((np.array([1.0], np.float32), np.array([2.0], np.float32), np.array([3.0], np.float32),
                  np.array([1.5], np.float32), np.array([1], np.uint64)))
    parts.append(protor("1jcd.pdb"))
    parts.append(parts[0])
    big = bw.synthetic_uniform(70000, seed=9)
    parts.append(big.structure(0))
    parts.append(protor("151L_H3.pdb"))
    so = np.zeros(len(parts) + 1, np.uint32)
    so[1:] = np.cumsum([len(p[0]) for p in parts])
    cat = [np.concatenate([p[k] for p in parts]) for k in range(5)]
    assert max(np.diff(so)) >= 65536
    got_o, got_e = ctx.precompute_neighbors_batch(*cat, so, PROBE)
    assert len(got_o) == so[-1] + 1
    for s, p in enumerate(parts):
        b, e = int(so[s]), int(so[s + 1])
        wo, we = oracle_csr(*p)
        assert np.array_equal(got_o[b:e + 1] - got_o[b], wo)
        assert got_e[int(got_o[b]):int(got_o[e])].tobytes() == we.tobytes()


def test_proteome_counts_match_sasa_path(ctx):
    """synthetic_proteome(40, seed=3): list lengths equal the SASA path's out_neighbor_counts of the same batch."""
    torch = pytest.importorskip("torch")
    b = bw.synthetic_proteome(40, seed=3)
    offs, ent = ctx.precompute_neighbors_batch(b.x, b.y, b.z, b.radius, b.ids, b.structure_offsets, PROBE)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    x, y, z, r, ids = t(b.x), t(b.y), t(b.z), t(b.radius), t(b.ids.view(np.int64))
    out = torch.zeros(b.n_atoms, dtype=torch.float32, device=dev)
    k = torch.zeros(b.n_atoms, dtype=torch.int32, device=dev)
    ctx.enqueue_device(x, y, z, r, ids, b.structure_offsets, out_atom_sasa=out, out_neighbor_counts=k,
                       probe_radius=PROBE, n_points=100)
    ctx.wait()
    counts = k.cpu().numpy().view(np.uint32).astype(np.uint64)
    assert np.array_equal(np.diff(offs), counts)
    assert int(offs[-1]) == len(ent)
    # and the lists of a few structures byte for byte
    for s in (0, 17, 39):
        lo, hi = int(b.structure_offsets[s]), int(b.structure_offsets[s + 1])
        wo, we = oracle_csr(*b.structure(s))
        assert np.array_equal(offs[lo:hi + 1] - offs[lo], wo)
        assert ent[int(offs[lo]):int(offs[hi])].tobytes() == we.tobytes()


# ---- sizing --------------------------------------------------------------------------------------------------------

def test_buffer_too_small_leaves_entries(ctx):
    from rustsasa_amd import NEIGHBOR_DTYPE, _capi
    from rustsasa_amd._capi import ptr
    x, y, z, r, ids = protor("1jcd.pdb")
    want_o, want_e = oracle_csr(x, y, z, r, ids)
    total = int(want_o[-1])
    offs = np.zeros(len(x) + 1, np.uint64)
    ent = np.zeros(total - 1, NEIGHBOR_DTYPE)
    ent["idx"] = 0xDEADBEEF
    before = ent.tobytes()
    lib = _capi.load()
    rc = lib.rsasa_precompute_neighbors(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), len(x), None, 0, PROBE,
                                        float("nan"), ptr(offs), ptr(ent), total - 1)
    assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL
    assert ent.tobytes() == before
    assert np.array_equal(offs, want_o)
    offs2 = np.zeros(len(x) + 1, np.uint64)
    rc = lib.rsasa_precompute_neighbors(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), len(x), None, 0, PROBE,
                                        float("nan"), ptr(offs2), None, 0)
    assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL and np.array_equal(offs2, want_o)


# ---- next to a device batch in flight ------------------------------------------------------------------------------

def test_concurrent_with_device_batch(ctx):
    torch = pytest.importorskip("torch")
    b = bw.synthetic_proteome(12, seed=4)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out = torch.zeros(b.n_atoms, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.enqueue_device(t(b.x), t(b.y), t(b.z), t(b.radius), t(b.ids.view(np.int64)), b.structure_offsets,
                       out_atom_sasa=out, probe_radius=PROBE, n_points=100)
    x, y, z, r, ids = protor("1jcd.pdb")
    got = ctx.precompute_neighbors(x, y, z, r, ids, PROBE)
    ctx.wait()
    assert_same(got, oracle_csr(x, y, z, r, ids))
    want = po.calculate_sasa_batch(b.x, b.y, b.z, b.radius, b.ids, b.structure_offsets, PROBE, 100, 8, threads=0)
    assert np.array_equal(out.cpu().numpy(), want)
