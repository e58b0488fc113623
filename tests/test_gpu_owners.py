"""Contact owners on the GPU (rsasa_contact_owners*: every buried sphere point of an atom given to the entry of its
neighbour list with the smallest float32 margin dot - limit) against the exact CPU model of owners_model.py and the
neighbour, point, contact and SASA calls of the same build.  Every comparison is exact: np.array_equal or a byte
comparison."""
import numpy as np
import pytest

import bench_workloads as bw
import nb_helpers as nh
import owner_cases as oc
import owners_model as om
import point_edge_cases as pe
import tie_cases as tc

pytestmark = pytest.mark.gpu

WS = (1, 4, 8, 16)
N_POINTS = (100, 101, 127, 960)
PROBES = (1.4, 3.0)
FIXTURES = ["example.cif:vdw", "1jcd.pdb", "151L_H3.pdb"]
EDGE_POINTS = (1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256, 257, 513)   # chunks of 64; passes of 2 and 4 chunks
CLUSTER_POINTS = (100, 300)
CLUSTER_WS = (8, 16)
FULL_LIST = ("probe_42", 100, 8)   # (setting of point_edge_cases, n_points, W): every atom in every list, five stages


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fixture_models():
    """{(fixture, probe, n_points): (offsets, entries, {W: (owned, owner)})}, computed once on a few threads."""
    def one(key):
        f, p, n = key
        return om.owners_ws(*pe.fixture(f), p, n, WS)
    return pe.pmap(one, [(f, p, n) for f in FIXTURES for p in PROBES for n in N_POINTS])


@pytest.fixture(scope="module")
def edge_models():
    cols, _ = nh.tight_cluster(6, seed=6)
    lists = nh.oracle_csr(*cols, 1.4)
    return pe.pmap(lambda n: om.owners_ws(*cols, 1.4, n, WS, lists), EDGE_POINTS)


def _named_case(name):
    if name == "late_owner":
        return oc.late_owner()[0]
    if name == "dup_stage":
        return oc.dup_stage()[0]
    if name == "dups":
        return oc.dups()[0]
    return nh.tight_cluster(name, seed=name)[0]


CLUSTER_CASES = list(pe.CLUSTER_SIZES) + ["late_owner", "dup_stage", "dups"]


@pytest.fixture(scope="module")
def cluster_models():
    def one(key):
        name, n = key
        return om.owners_ws(*_named_case(name), 1.4, n, CLUSTER_WS)
    return pe.pmap(one, [(c, n) for c in CLUSTER_CASES for n in CLUSTER_POINTS])


def _check_shapes(got, n_atoms, n_points):
    offs, ent, owned, sasa, owner = got
    assert offs.dtype == np.uint64 and offs.shape == (n_atoms + 1,)
    assert owned.dtype == np.uint32 and owner.dtype == np.uint32 and sasa.dtype == np.float32
    assert owned.shape == ent.shape == (int(offs[-1]),) and sasa.shape == (n_atoms,) and owner.shape == (n_atoms, n_points)


def _assert_owners(got, model):
    """got = contact_owners(..., points=True), model = (offsets, entries, owned, owner)"""
    nh.assert_same(got[:2], model[:2])
    assert np.array_equal(got[2], model[2])
    assert np.array_equal(got[4], model[3])


def _check_against_model(ctx, cols, probe, n_points, model, Ws, batch=False):
    offs_m, ent_m, by_w = model
    n = len(cols[0])
    so = np.array([0, n], np.uint32)
    try:
        for W in Ws:
            ctx.set_simd_width(W)
            got = ctx.contact_owners(*cols, probe, n_points, points=True)
            _check_shapes(got, n, n_points)
            _assert_owners(got, (offs_m, ent_m) + by_w[W])
            if batch:
                bgot = ctx.contact_owners_batch(*cols, so, probe, n_points, points=True)
                for k in range(5):
                    assert got[k].tobytes() == bgot[k].tobytes(), k
    finally:
        ctx.set_simd_width(8)


# ---- 1: fixtures, every point count and lane count --------------------------------------------------------------

@pytest.mark.parametrize("n_points", N_POINTS)
@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_owners(ctx, fixture_models, name, probe, n_points):
    cols = pe.fixture(name)
    n = len(cols[0])
    so = np.array([0, n], np.uint32)
    offs_m, ent_m, by_w = fixture_models[(name, probe, n_points)]
    rows = np.repeat(np.arange(n), np.diff(offs_m.astype(np.int64)))
    try:
        for W in WS:
            ctx.set_simd_width(W)
            got = ctx.contact_owners(*cols, probe, n_points, points=True)
            bgot = ctx.contact_owners_batch(*cols, so, probe, n_points, points=True)
            _check_shapes(got, n, n_points)
            _assert_owners(got, (offs_m, ent_m) + by_w[W])
            for k in range(5):
                assert got[k].tobytes() == bgot[k].tobytes(), k
            # without the owner rows: the same counts
            plain = ctx.contact_owners(*cols, probe, n_points)
            assert len(plain) == 4 and all(plain[k].tobytes() == got[k].tobytes() for k in range(4))
            # the lists: contact_points' of the same build, byte for byte; the values: the SASA path's
            cp = ctx.contact_points(*cols, probe, n_points)
            assert got[0].tobytes() == cp[0].tobytes() and got[1].tobytes() == cp[1].tobytes()
            want, _ = ctx.calculate_sasa_batch(*cols, so, probe, n_points)
            assert got[3].tobytes() == want.tobytes() and bgot[3].tobytes() == want.tobytes()
            # a partition of the buried points, between exclusive and covered entry by entry
            words, _ = ctx.accessible_points(*cols, probe, n_points)
            buried = n_points - pe.popcount(words)
            s = np.zeros(n, np.int64)
            np.add.at(s, rows, got[2].astype(np.int64))
            assert np.array_equal(s, buried)
            assert np.array_equal((got[4] != om.FREE).sum(axis=1), buried)
            assert np.all(cp[3] <= got[2]) and np.all(got[2] <= cp[2])
    finally:
        ctx.set_simd_width(8)


# ---- 2: point counts at the chunk and pass edges ----------------------------------------------------------------

@pytest.mark.parametrize("n_points", EDGE_POINTS)
def test_point_counts_at_chunk_and_pass_edges(ctx, edge_models, n_points):
    """1jcd.pdb and a 6-atom cluster beside it (lists of 5), at every lane count."""
    cols, c0 = nh.tight_cluster(6, seed=6)
    model = edge_models[n_points]
    assert np.diff(model[0].astype(np.int64))[c0:].tolist() == [5] * 6
    _check_against_model(ctx, cols, 1.4, n_points, model, WS, batch=True)


# ---- 3: list lengths at the pad and stage edges, late owners, twins ---------------------------------------------

@pytest.mark.parametrize("n_points", CLUSTER_POINTS)
@pytest.mark.parametrize("case", CLUSTER_CASES)
def test_list_lengths_at_pad_and_stage_edges(ctx, cluster_models, case, n_points):
    cols = _named_case(case)
    model = cluster_models[(case, n_points)]
    k = np.diff(model[0].astype(np.int64))
    if isinstance(case, int):
        c0 = len(cols[0]) - case
        assert k[c0:].min() == k[c0:].max() == case - 1 and k[:c0].max() < pe.PT_STAGE
    elif case == "late_owner":
        oc.assert_late_owner(model[2][8][1], oc.late_owner()[1])
    elif case == "dup_stage":
        _, centre, twin = oc.dup_stage()
        oc.assert_dup_stage(cols, centre, twin, model[0], model[1])
        for W in CLUSTER_WS:
            assert model[2][W][0][int(model[0][centre]) + oc.PT_STAGE] == 0
    else:
        _, original, twins = oc.dups()
        _, e_twin = oc.twin_entries(model[0], model[1], original, twins)
        for W in CLUSTER_WS:
            assert not model[2][W][0][e_twin].any()
    _check_against_model(ctx, cols, 1.4, n_points, model, CLUSTER_WS)
    if case in ("dup_stage", "dups"):
        # the later twin owns nothing although it covers points
        cp = ctx.contact_points(*cols, 1.4, n_points)
        got = ctx.contact_owners(*cols, 1.4, n_points)
        if case == "dups":
            sel = e_twin
        else:
            sel = np.array([int(model[0][centre]) + oc.PT_STAGE])
        assert not got[2][sel].any() and cp[2][sel].any()


def test_cluster_classes():
    ks = [n - 1 for n in pe.CLUSTER_SIZES]
    assert {1, 2, 3, 4, 5, 255, 256, 257, 258, 511, 512, 513, 768} <= set(ks)
    assert tc.n_fused(300, 16) == 288 > 256 and tc.n_fused(100, 8) == 96 and pe.nch(100) == 2 and pe.nch(300) == 4


# ---- 4: every atom in every list --------------------------------------------------------------------------------

def test_lists_of_every_atom(ctx):
    setting, n_points, W = FULL_LIST
    cols, probe = pe.full_list_cols(setting)
    model = om.owners_ws(*cols, probe, n_points, (W,))
    pe.assert_full_lists(setting, np.diff(model[0].astype(np.int64)))
    owner = model[2][W][1]
    assert (owner[owner != om.FREE] >= 4 * pe.PT_STAGE).any()          # owners in the fifth stage
    _check_against_model(ctx, cols, probe, n_points, model, (W,), batch=True)


# ---- 5: counts wider than 16 bits -------------------------------------------------------------------------------

def test_count_width(ctx):
    f = lambda *a: np.array(a, np.float32)  # noqa: E731
    n_points = 70_000
    one = (f(0, 0.1), f(0, 0), f(0, 0), f(1.0, 3.0), None)               # atom 0 inside atom 1
    # ... and inside a smaller atom 2 further off, which wins a cap of about 4 % of atom 0's sphere
    two = (f(0, 0.1, -0.6), f(0, 0, 0), f(0, 0, 0), f(1.0, 3.3, 3.0), None)
    for cols, k0 in ((one, 1), (two, 2)):
        got = ctx.contact_owners(*cols, 1.4, n_points, points=True)
        model = om.owners(*cols, 1.4, n_points, 8)
        _assert_owners(got, model)
        assert int(got[0][1]) == k0
        assert int(got[2][:k0].sum()) == n_points and int(got[2][0]) > 65535
    assert 0 < int(got[2][1]) < n_points - 65535                          # both neighbours own a part of atom 0


# ---- 6: ids -----------------------------------------------------------------------------------------------------

def test_ids(ctx):
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    col = ids.astype(np.uint64).copy()
    for i in range(1, len(col), 2):
        col[i] = tc.colliding_id(int(col[i - 1]), 0x1234 + i)   # equal 32-bit folds, different ids
    col2 = col.copy()
    col2[1::6] = col2[0::6][:len(col2[1::6])]                   # ... and some really equal ids among them
    shared = (ids // np.uint64(3)).astype(np.uint64)
    for variant in (shared, col, col2, None):
        got = ctx.contact_owners(x, y, z, r, variant, 1.4, 100, points=True)
        _assert_owners(got, om.owners(x, y, z, r, variant, 1.4, 100, 8))
        if variant is not None:
            rows = np.repeat(np.arange(len(x)), np.diff(got[0].astype(np.int64)))
            assert not (variant[got[1]["idx"].astype(np.int64)] == variant[rows]).any()
    cols, c0 = nh.tight_cluster(400, seed=5, shared_ids=True)
    got = ctx.contact_owners(*cols, 1.4, 100, points=True)
    _assert_owners(got, om.owners(*cols, 1.4, 100, 8))
    rows = np.repeat(np.arange(len(cols[0])), np.diff(got[0].astype(np.int64)))
    assert not (cols[4][got[1]["idx"].astype(np.int64)] == cols[4][rows]).any()


# ---- 7: batches -------------------------------------------------------------------------------------------------

def test_mixed_batch_equals_per_structure(ctx):
    parts = [(np.zeros(0, np.float32),) * 4 + (np.zeros(0, np.uint64),)]
    parts.append((np.array([1.0], np.float32), np.array([2.0], np.float32), np.array([3.0], np.float32),
                  np.array([1.5], np.float32), np.array([1], np.uint64)))
    parts.append(nh.protor("1jcd.pdb"))
    parts.append(parts[0])
    parts.append(bw.synthetic_uniform(n_atoms=70_000, seed=9).structure(0))
    parts.append(nh.protor("151L_H3.pdb"))
    so = np.zeros(len(parts) + 1, np.uint32)
    so[1:] = np.cumsum([len(p[0]) for p in parts])
    cat = [np.concatenate([p[k] for p in parts]) for k in range(5)]
    assert max(np.diff(so)) >= 65536
    for n_points in (100, 960):
        got = ctx.contact_owners_batch(*cat, so, 1.4, n_points, points=True)
        offs, ent, owned, sasa, owner = got
        _check_shapes(got, int(so[-1]), n_points)
        for s, p in enumerate(parts):
            b, e = int(so[s]), int(so[s + 1])
            if e == b:
                continue
            o1, e1, c1, s1, w1 = ctx.contact_owners(*p, 1.4, n_points, points=True)
            lo, hi = int(offs[b]), int(offs[e])
            assert np.array_equal(offs[b:e + 1] - offs[b], o1)
            assert ent[lo:hi].tobytes() == e1.tobytes()
            assert np.array_equal(owned[lo:hi], c1) and np.array_equal(owner[b:e], w1)
            assert sasa[b:e].tobytes() == s1.tobytes()
        lo, hi = int(offs[so[2]]), int(offs[so[3]])
        _, _, m_owned, m_owner = om.owners(*parts[2], 1.4, n_points, 8)
        assert np.array_equal(owned[lo:hi], m_owned) and np.array_equal(owner[so[2]:so[3]], m_owner)
        assert offs[so[1]] == offs[so[1] + 1] and (owner[so[1]] == om.FREE).all()   # the lone atom: every point free
        want, _ = ctx.calculate_sasa_batch(*cat, so, 1.4, n_points)
        assert sasa.tobytes() == want.tobytes()


# ---- 8: non-finite input ----------------------------------------------------------------------------------------

def test_nan_coordinate_and_radius(ctx):
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    x, r = x.copy(), r.copy()
    x[5] = np.nan
    r[17] = np.nan
    for n_points in (100, 101):
        got = ctx.contact_owners(x, y, z, r, ids, 1.4, n_points, points=True)
        offs, ent, owned, sasa, owner = got
        assert offs[5] == offs[6] and offs[17] == offs[18]          # empty lists
        assert (owner[5] == om.FREE).all() and (owner[17] == om.FREE).all()
        idx = ent["idx"].astype(np.int64)
        assert not (idx == 5).any()                                  # nobody's neighbour
        assert (idx == 17).any() and not owned[idx == 17].any()      # a NaN limit never hits and so never owns
        _assert_owners(got, om.owners(x, y, z, r, ids, 1.4, n_points, 8))
        want, _ = ctx.calculate_sasa_batch(x, y, z, r, ids, np.array([0, len(x)], np.uint32), 1.4, n_points)
        assert sasa.tobytes() == want.tobytes()


def test_infinite_coordinate_then_usable(ctx):
    import rustsasa_amd
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    bad = x.copy()
    bad[3] = np.inf
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.contact_owners(bad, y, z, r, ids, 1.4, 100, points=True)
    assert e.value.status == -5
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.contact_owners_batch(bad, y, z, r, ids, np.array([0, len(x)], np.uint32), 1.4, 100)
    assert e.value.status == -5
    _assert_owners(ctx.contact_owners(x, y, z, r, ids, 1.4, 100, points=True), om.owners(x, y, z, r, ids, 1.4, 100, 8))


# ---- 9: sizing and argument errors from the library -------------------------------------------------------------

def test_sizing_and_argument_errors_from_the_library(ctx):
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    lib = _capi.load()
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    n, n_points = len(x), 100
    want = om.owners(x, y, z, r, ids, 1.4, n_points, 8)
    total = int(want[0][-1])
    so = np.array([0, n], np.uint32)

    def call(offs, ent, owned, cap, owner=None, sasa=None, n_points=n_points, probe=1.4):
        return lib.rsasa_contact_owners(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), n, probe, n_points,
                                        ptr(offs), ptr(ent), ptr(owned), cap, ptr(owner), ptr(sasa))

    def bcall(offs, ent, owned, cap, owner=None, so=so):
        return lib.rsasa_contact_owners_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), len(so) - 1,
                                              1.4, n_points, ptr(offs), ptr(ent), ptr(owned), cap, ptr(owner), None)
    ent = np.zeros(total, _capi.NEIGHBOR_DTYPE)
    owned = np.full(total, 7, np.uint32)
    owner = np.full((n, n_points), 7, np.uint32)
    for f in (call, bcall):
        # an entry buffer NULL, or one entry short: the offsets, and nothing else
        for args in ((None, owned, total), (ent, None, total), (ent, owned, total - 1)):
            offs = np.zeros(n + 1, np.uint64)
            assert f(offs, *args, owner=owner) == _capi.RSASA_ERR_BUFFER_TOO_SMALL
            assert np.array_equal(offs, want[0])
            assert ent.tobytes() == bytes(ent.nbytes) and (owned == 7).all() and (owner == 7).all()
    # argument errors
    offs = np.zeros(n + 1, np.uint64)
    assert call(offs, ent, owned, total, n_points=0) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert call(offs, ent, owned, total, probe=-5.0) == _capi.RSASA_ERR_INVALID_ARGUMENT   # probe + max_r <= 0
    assert call(None, ent, owned, total) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert bcall(offs, ent, owned, total, so=np.array([0, 600, 500, n], np.uint32)) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert bcall(offs, ent, owned, total, so=np.array([1, n], np.uint32)) == _capi.RSASA_ERR_INVALID_ARGUMENT
    # out_owner NULL and given: the same owned; out_sasa is optional; a larger capacity is fine
    big = [np.zeros(total + 5, _capi.NEIGHBOR_DTYPE), np.zeros(total + 5, np.uint32)]
    assert call(offs, *big, total + 5) == _capi.RSASA_OK
    assert np.array_equal(offs, want[0]) and big[0][:total].tobytes() == want[1].tobytes()
    assert np.array_equal(big[1][:total], want[2]) and not big[1][total:].any()
    for f in (call, bcall):
        ent2, owned2 = np.zeros(total, _capi.NEIGHBOR_DTYPE), np.zeros(total, np.uint32)
        assert f(offs, ent2, owned2, total, owner=owner) == _capi.RSASA_OK
        assert np.array_equal(owned2, want[2]) and np.array_equal(owner, want[3]) and ent2.tobytes() == want[1].tobytes()
        owner[:] = 7
    # no atoms: offsets [0], whatever the buffers
    o0 = np.ones(1, np.uint64)
    assert lib.rsasa_contact_owners(ctx._h, None, None, None, None, None, 0, 1.4, 100, ptr(o0), None, None, 0, None,
                                    None) == _capi.RSASA_OK and o0[0] == 0
    o0[0] = 1
    assert lib.rsasa_contact_owners_batch(ctx._h, None, None, None, None, None, ptr(np.zeros(1, np.uint32)), 0, 1.4, 100,
                                          ptr(o0), None, None, 0, None, None) == _capi.RSASA_OK and o0[0] == 0


# ---- 10: one context, other families in between, a device batch in flight ---------------------------------------

def test_interleaved_with_the_other_families(ctx):
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    small = nh.protor("151L_H3.pdb")
    want = om.owners(x, y, z, r, ids, 1.4, 100, 8)
    want_small = om.owners(*small, 1.4, 127, 8)
    groups = (np.arange(len(x)) // 9).astype(np.uint32)
    first = ctx.contact_owners(x, y, z, r, ids, 1.4, 100, points=True)
    _assert_owners(first, want)
    others = [lambda: ctx.contact_points(x, y, z, r, ids, 1.4, 960),
              lambda: ctx.group_contacts(x, y, z, r, ids, groups, 1.4, 100),
              lambda: ctx.accessible_points(*small, 1.4, 50),
              lambda: ctx.atoms_within(x, y, z, r, ids, 1.4, cutoff=8.0)]
    before = [f() for f in others]
    for f, ref in zip(others, before):
        _assert_owners(ctx.contact_owners(*small, 1.4, 127, points=True), want_small)
        again = f()
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(again, ref))
        got = ctx.contact_owners(x, y, z, r, ids, 1.4, 100, points=True)
        assert all(got[k].tobytes() == first[k].tobytes() for k in range(5))


def test_device_batch_in_flight_undisturbed(ctx):
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
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    got = ctx.contact_owners(x, y, z, r, ids, 1.4, 100, points=True)
    ctx.wait()
    assert out.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    _assert_owners(got, om.owners(x, y, z, r, ids, 1.4, 100, 8))
