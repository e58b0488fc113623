"""Contact counts on the GPU (rsasa_contact_points*: per entry of each atom's neighbour list, the sphere points of the
atom it occludes and those only it occludes - the reference's own per-point tests, src/lib.rs:129-146,183-207) against
the exact CPU model of contacts_model.py, the neighbour, point and SASA calls of the same build, and the oracle.  Every
comparison is exact: np.array_equal or a byte comparison."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bench_workloads as bw
import contacts_model as cm
import nb_helpers as nh
import structio as sio
import tie_cases as tc

pytestmark = pytest.mark.gpu

WS = (1, 4, 8, 16)
N_POINTS = (100, 101, 127, 960)
PROBES = (1.4, 3.0)
FIXTURES = ["example.cif:vdw", "1jcd.pdb", "151L_H3.pdb", "bad_seqadv_1A06.pdb", "example.cif"]


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


def _fixture(name):
    if name.endswith(":vdw"):
        return sio.soa_vdw(sio.read_structure(sio.data_path(name.split(":")[0])))
    return nh.protor(name)


def _threads():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(16, n))


@pytest.fixture(scope="module")
def fixture_models():
    """{(fixture, probe, n_points): (offsets, entries, {W: (covered, exclusive, buried)})} for every combination of
    test 1, computed once on a few threads."""
    keys = [(f, p, n) for f in FIXTURES for p in PROBES for n in N_POINTS]

    def one(key):
        f, p, n = key
        return cm.contact_counts_ws(*_fixture(f), p, n, WS)
    with ThreadPoolExecutor(_threads()) as ex:
        return dict(zip(keys, ex.map(one, keys)))


def _popcount(words):
    return np.unpackbits(words.view(np.uint8), axis=1).sum(axis=1).astype(np.int64)


def _check_shapes(got, n_atoms):
    offs, ent, cov, exc, sasa = got
    assert offs.dtype == np.uint64 and offs.shape == (n_atoms + 1,)
    assert cov.dtype == np.uint32 and exc.dtype == np.uint32 and sasa.dtype == np.float32
    assert cov.shape == exc.shape == ent.shape == (int(offs[-1]),) and sasa.shape == (n_atoms,)


def _assert_counts(got, model):
    """got = contact_points(...), model = (offsets, entries, covered, exclusive)"""
    nh.assert_same(got[:2], model[:2])
    assert np.array_equal(got[2], model[2]) and np.array_equal(got[3], model[3])


# ---- 1: fixtures, every point count and lane count --------------------------------------------------------------

@pytest.mark.parametrize("n_points", N_POINTS)
@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_counts(ctx, fixture_models, name, probe, n_points):
    x, y, z, r, ids = _fixture(name)
    n = len(x)
    so = np.array([0, n], np.uint32)
    offs_m, ent_m, by_w = fixture_models[(name, probe, n_points)]
    rows = np.repeat(np.arange(n), np.diff(offs_m.astype(np.int64)))
    try:
        for W in WS:
            ctx.set_simd_width(W)
            got = ctx.contact_points(x, y, z, r, ids, probe, n_points)
            bgot = ctx.contact_points_batch(x, y, z, r, ids, so, probe, n_points)
            _check_shapes(got, n)
            # the lists: those of precompute_neighbors of the same build, and the oracle's
            nb = ctx.precompute_neighbors_batch(x, y, z, r, ids, so, probe)
            nh.assert_same(got[:2], nb)
            cov_m, exc_m, buried_m = by_w[W]
            _assert_counts(got, (offs_m, ent_m, cov_m, exc_m))
            for k in range(4):
                assert got[k].tobytes() == bgot[k].tobytes(), k
            # the values: the SASA path's
            want, _ = ctx.calculate_sasa_batch(x, y, z, r, ids, so, probe, n_points)
            assert got[4].tobytes() == want.tobytes() and bgot[4].tobytes() == want.tobytes()
            # against the point masks: sum(exclusive) <= buried <= sum(covered), max(covered) <= buried
            words, _ = ctx.accessible_points(x, y, z, r, ids, probe, n_points)
            buried = n_points - _popcount(words)
            assert np.array_equal(buried, buried_m)
            s_cov, s_exc, m_cov = (np.zeros(n, np.int64) for _ in range(3))
            np.add.at(s_cov, rows, got[2].astype(np.int64))
            np.add.at(s_exc, rows, got[3].astype(np.int64))
            np.maximum.at(m_cov, rows, got[2].astype(np.int64))
            assert np.all(s_exc <= buried) and np.all(buried <= s_cov) and np.all(m_cov <= buried)
    finally:
        ctx.set_simd_width(8)


# ---- 2: the pair and deletion oracles through the GPU ----------------------------------------------------------

@pytest.mark.parametrize("n_points", [100, 97])
def test_pair_and_deletion_oracles(ctx, n_points):
    cols = nh.protor("1jcd.pdb")
    offs, ent, cov, exc, _ = ctx.contact_points(*cols, 1.4, n_points)
    nh.assert_same((offs, ent), nh.oracle_csr(*cols, 1.4))
    n_in, n_out = cm.pair_check(*cols, 1.4, n_points, 8, offs, ent, cov, n_pairs=400, seed=21)
    assert n_in + n_out == 400 and n_in > 300
    n_cmp = cm.deletion_check(*cols, 1.4, n_points, 8, offs, ent, exc, n_del=12, seed=22)
    assert n_cmp >= 11 * (len(cols[0]) - 1)


# ---- 3: lists longer than one LDS stage ------------------------------------------------------------------------

@pytest.mark.parametrize("n", [300, 1000])
def test_long_lists(ctx, n):
    cols, c0 = nh.tight_cluster(n, seed=n)
    for n_points in (100, 127):
        model = cm.contact_counts(*cols, 1.4, n_points, 8)
        assert int(np.diff(model[0].astype(np.int64))[c0:].min()) == n - 1 > 256
        got = ctx.contact_points(*cols, 1.4, n_points)
        _assert_counts(got, model)


# ---- 4: counts wider than 16 bits ------------------------------------------------------------------------------

def test_count_width(ctx):
    f = lambda *a: np.array(a, np.float32)  # noqa: E731
    cols = (f(0, 0.1), f(0, 0), f(0, 0), f(1.0, 3.0), None)   # atom 0 inside atom 1
    n_points = 70_000
    got = ctx.contact_points(*cols, 1.4, n_points)
    model = cm.contact_counts(*cols, 1.4, n_points, 8)
    _assert_counts(got, model)
    assert got[0].tolist() == [0, 1, 2]
    assert int(got[2][0]) > 65535 and int(got[2][0]) == n_points and int(got[3][0]) == n_points


# ---- 5: ids ------------------------------------------------------------------------------------------------------

def test_ids(ctx):
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    col = ids.astype(np.uint64).copy()
    for i in range(1, len(col), 2):
        col[i] = tc.colliding_id(int(col[i - 1]), 0x1234 + i)   # equal 32-bit folds, different ids
    col2 = col.copy()
    col2[1::6] = col2[0::6][:len(col2[1::6])]                   # ... and some really equal ids among them
    shared = (ids // np.uint64(3)).astype(np.uint64)
    for variant in (shared, col, col2, None):
        got = ctx.contact_points(x, y, z, r, variant, 1.4, 100)
        _assert_counts(got, cm.contact_counts(x, y, z, r, variant, 1.4, 100, 8))
        if variant is not None:
            rows = np.repeat(np.arange(len(x)), np.diff(got[0].astype(np.int64)))
            assert not (variant[got[1]["idx"].astype(np.int64)] == variant[rows]).any()
    cols, c0 = nh.tight_cluster(400, seed=5, shared_ids=True)
    got = ctx.contact_points(*cols, 1.4, 100)
    _assert_counts(got, cm.contact_counts(*cols, 1.4, 100, 8))
    rows = np.repeat(np.arange(len(cols[0])), np.diff(got[0].astype(np.int64)))
    assert not (cols[4][got[1]["idx"].astype(np.int64)] == cols[4][rows]).any()


# ---- 6: batches --------------------------------------------------------------------------------------------------

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
        offs, ent, cov, exc, sasa = ctx.contact_points_batch(*cat, so, 1.4, n_points)
        _check_shapes((offs, ent, cov, exc, sasa), int(so[-1]))
        for s, p in enumerate(parts):
            b, e = int(so[s]), int(so[s + 1])
            if e == b:
                continue
            o1, e1, c1, x1, s1 = ctx.contact_points(*p, 1.4, n_points)
            lo, hi = int(offs[b]), int(offs[e])
            assert np.array_equal(offs[b:e + 1] - offs[b], o1)
            assert ent[lo:hi].tobytes() == e1.tobytes()
            assert np.array_equal(cov[lo:hi], c1) and np.array_equal(exc[lo:hi], x1)
            assert sasa[b:e].tobytes() == s1.tobytes()
        lo, hi = int(offs[so[2]]), int(offs[so[3]])
        _, _, mc, mx = cm.contact_counts(*parts[2], 1.4, n_points, 8)
        assert np.array_equal(cov[lo:hi], mc) and np.array_equal(exc[lo:hi], mx)
        assert offs[so[1]] == offs[so[1] + 1]          # the lone atom: no list, every point exposed
        want, _ = ctx.calculate_sasa_batch(*cat, so, 1.4, n_points)
        assert sasa.tobytes() == want.tobytes()


# ---- 7: non-finite input -----------------------------------------------------------------------------------------

def test_nan_coordinate_and_radius(ctx):
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    x, r = x.copy(), r.copy()
    x[5] = np.nan
    r[17] = np.nan
    for n_points in (100, 101):
        got = ctx.contact_points(x, y, z, r, ids, 1.4, n_points)
        offs, ent, cov, exc, sasa = got
        assert offs[5] == offs[6] and offs[17] == offs[18]          # empty lists
        idx = ent["idx"].astype(np.int64)
        assert not (idx == 5).any()                                  # nobody's neighbour
        assert (idx == 17).any() and not cov[idx == 17].any() and not exc[idx == 17].any()
        _assert_counts(got, cm.contact_counts(x, y, z, r, ids, 1.4, n_points, 8))
        want, _ = ctx.calculate_sasa_batch(x, y, z, r, ids, np.array([0, len(x)], np.uint32), 1.4, n_points)
        assert sasa.tobytes() == want.tobytes()


def test_infinite_coordinate_then_usable(ctx):
    import rustsasa_amd
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    bad = x.copy()
    bad[3] = np.inf
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.contact_points(bad, y, z, r, ids, 1.4, 100)
    assert e.value.status == -5
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.contact_points_batch(bad, y, z, r, ids, np.array([0, len(x)], np.uint32), 1.4, 100)
    assert e.value.status == -5
    _assert_counts(ctx.contact_points(x, y, z, r, ids, 1.4, 100), cm.contact_counts(x, y, z, r, ids, 1.4, 100, 8))


# ---- 8: sizing and argument errors from the library --------------------------------------------------------------

def test_sizing_and_argument_errors_from_the_library(ctx):
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    lib = _capi.load()
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    n = len(x)
    want = cm.contact_counts(x, y, z, r, ids, 1.4, 100, 8)
    total = int(want[0][-1])
    so = np.array([0, n], np.uint32)

    def call(offs, ent, cov, exc, cap, sasa=None, n_points=100, probe=1.4):
        return lib.rsasa_contact_points(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), n, probe, n_points,
                                        ptr(offs), ptr(ent), ptr(cov), ptr(exc), cap, ptr(sasa))

    def bcall(offs, ent, cov, exc, cap, so=so):
        return lib.rsasa_contact_points_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), len(so) - 1,
                                              1.4, 100, ptr(offs), ptr(ent), ptr(cov), ptr(exc), cap, None)
    ent = np.zeros(total, _capi.NEIGHBOR_DTYPE)
    cov = np.full(total, 7, np.uint32)
    exc = np.full(total, 7, np.uint32)
    for f in (call, bcall):
        # any of the three entry buffers NULL, or one entry short: the offsets, and nothing else
        for args in ((None, cov, exc, total), (ent, None, exc, total), (ent, cov, None, total),
                     (ent, cov, exc, total - 1)):
            offs = np.zeros(n + 1, np.uint64)
            assert f(offs, *args) == _capi.RSASA_ERR_BUFFER_TOO_SMALL
            assert np.array_equal(offs, want[0])
            assert ent.tobytes() == bytes(ent.nbytes) and (cov == 7).all() and (exc == 7).all()
    # argument errors
    offs = np.zeros(n + 1, np.uint64)
    assert call(offs, ent, cov, exc, total, n_points=0) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert call(offs, ent, cov, exc, total, probe=-5.0) == _capi.RSASA_ERR_INVALID_ARGUMENT   # probe + max_r <= 0
    assert call(None, ent, cov, exc, total) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert bcall(offs, ent, cov, exc, total, so=np.array([0, 600, 500, n], np.uint32)) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert bcall(offs, ent, cov, exc, total, so=np.array([1, n], np.uint32)) == _capi.RSASA_ERR_INVALID_ARGUMENT
    # out_sasa is optional; the context is still usable; a larger capacity is fine
    big = [np.zeros(total + 5, _capi.NEIGHBOR_DTYPE), np.zeros(total + 5, np.uint32), np.zeros(total + 5, np.uint32)]
    assert call(offs, *big, total + 5) == _capi.RSASA_OK
    _assert_counts((offs, big[0][:total], big[1][:total], big[2][:total]), want)
    # no atoms: offsets [0], whatever the buffers
    o0 = np.ones(1, np.uint64)
    assert lib.rsasa_contact_points(ctx._h, None, None, None, None, None, 0, 1.4, 100, ptr(o0), None, None, None, 0,
                                    None) == _capi.RSASA_OK and o0[0] == 0


# ---- 9: next to a device batch in flight ------------------------------------------------------------------------

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
    got = ctx.contact_points(x, y, z, r, ids, 1.4, 100)
    ctx.wait()
    assert out.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    _assert_counts(got, cm.contact_counts(x, y, z, r, ids, 1.4, 100, 8))
