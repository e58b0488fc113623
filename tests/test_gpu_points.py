"""Accessible-point masks on the GPU (rsasa_accessible_points*, the decisions behind reference src/lib.rs:96-223)
against the exact CPU model of points_model.py, and their values against the SASA path and the oracle.  Every
comparison is exact: np.array_equal or a byte comparison."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bench_workloads as bw
import nb_helpers as nh
import points_model as pm
import structio as sio
import tie_cases as tc
from oracle import pyoracle as po

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
    return max(1, min(8, n))


@pytest.fixture(scope="module")
def fixture_models():
    """{(fixture, probe, n_points): {W: model mask}} for every combination of test 1, computed once (numpy releases
    the interpreter lock in the large array operations, so a few threads share the work)."""
    keys = [(f, p, n) for f in FIXTURES for p in PROBES for n in N_POINTS]

    def one(key):
        f, p, n = key
        x, y, z, r, ids = _fixture(f)
        return pm.exposed_masks_ws(x, y, z, r, ids, p, n, WS)
    with ThreadPoolExecutor(_threads()) as ex:
        return dict(zip(keys, ex.map(one, keys)))


def _check_masks(words, n_points):
    assert words.dtype == np.uint32 and words.shape[1] == pm.words_of(n_points)
    if n_points % 32:
        assert not (words[:, -1] >> np.uint32(n_points % 32)).any()  # the padding bits are 0


def _popcount(words):
    return np.unpackbits(words.view(np.uint8), axis=1).sum(axis=1)


# ---- 1 / 2: fixtures, every point count and lane count ----------------------------------------------------------

@pytest.mark.parametrize("n_points", N_POINTS)
@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_masks_and_values(ctx, fixture_models, name, probe, n_points):
    x, y, z, r, ids = _fixture(name)
    so = np.array([0, len(x)], np.uint32)
    try:
        for W in WS:
            ctx.set_simd_width(W)
            words, sasa = ctx.accessible_points(x, y, z, r, ids, probe, n_points)
            _check_masks(words, n_points)
            assert np.array_equal(words, pm.pack(fixture_models[(name, probe, n_points)][W])), W
            bwords, bsasa = ctx.accessible_points_batch(x, y, z, r, ids, so, probe, n_points)
            assert np.array_equal(bwords, words)
            # the values: the SASA path's, the oracle's, and the reference's expression of the popcount
            want, _ = ctx.calculate_sasa_batch(x, y, z, r, ids, so, probe, n_points)
            assert sasa.tobytes() == want.tobytes() and bsasa.tobytes() == want.tobytes()
            oracle = po.calculate_sasa_batch(x, y, z, r, ids, so, probe, n_points, W, threads=0)
            assert sasa.tobytes() == oracle.tobytes()
            assert pm.sasa_of(r, probe, _popcount(words), n_points).tobytes() == want.tobytes()
    finally:
        ctx.set_simd_width(8)


# ---- 3: every tie case, one batch per (probe, n_points, W) --------------------------------------------------------

def test_tie_cases(ctx):
    groups = {}
    for case in tc.all_cases():
        groups.setdefault((case.probe, case.n_points, case.W), []).extend(case.structures)
    n = 0
    try:
        for (probe, n_points, W), sts in sorted(groups.items()):
            x, y, z, r, ids, so = tc.pack(sts)
            ctx.set_simd_width(W)
            words, sasa = ctx.accessible_points_batch(x, y, z, r, ids, so, probe, n_points)
            _check_masks(words, n_points)
            want = pm.exposed_masks_batch(x, y, z, r, ids, so, probe, n_points, W)
            assert np.array_equal(words, pm.pack(want)), (probe, n_points, W)
            n += len(sts)
    finally:
        ctx.set_simd_width(8)
    assert n > 10000


# ---- 4: ids ------------------------------------------------------------------------------------------------------

def test_ids(ctx):
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    col = ids.astype(np.uint64).copy()
    for i in range(1, len(col), 2):
        col[i] = tc.colliding_id(int(col[i - 1]), 0x1234 + i)   # equal 32-bit folds, different ids
    col2 = col.copy()
    col2[1::6] = col2[0::6][:len(col2[1::6])]                   # ... and some really equal ids among them
    for variant in ((ids // np.uint64(3)).astype(np.uint64), col, col2, None):
        words, _ = ctx.accessible_points(x, y, z, r, variant, 1.4, 100)
        assert np.array_equal(words, pm.pack(pm.exposed_masks(x, y, z, r, variant, 1.4, 100, 8)))
    dup, _ = ctx.accessible_points(x, y, z, r, (ids // np.uint64(3)).astype(np.uint64), 1.4, 100)
    assert not np.array_equal(dup, ctx.accessible_points(x, y, z, r, ids, 1.4, 100)[0])


def test_own_id_never_buries(ctx):
    """A larger copy of atom 0 at its own centre (the structure's largest radius unchanged): with atom 0's id it is
    skipped and atom 0 keeps exactly its mask; with another id it buries atom 0 completely."""
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    alone, _ = ctx.accessible_points(x, y, z, r, ids, 1.4, 100)
    assert alone[0].any()
    big = np.float32(r[0] + np.float32(0.2))
    assert big <= r.max()
    X, Y, Z = (np.append(a, a[0]).astype(np.float32) for a in (x, y, z))
    R = np.append(r, big).astype(np.float32)
    for copy_id, buried in ((ids[0], False), (np.uint64(10 ** 9), True)):
        I = np.append(ids, copy_id).astype(np.uint64)
        words, _ = ctx.accessible_points(X, Y, Z, R, I, 1.4, 100)
        assert np.array_equal(words, pm.pack(pm.exposed_masks(X, Y, Z, R, I, 1.4, 100, 8)))
        if buried:
            assert not words[0].any()
        else:
            assert np.array_equal(words[0], alone[0])


# ---- 5: lists longer than one LDS stage ------------------------------------------------------------------------

@pytest.mark.parametrize("n", [300, 1000])
def test_long_lists(ctx, n):
    cols, c0 = nh.tight_cluster(n, seed=n)
    offs, _ = nh.oracle_csr(*cols)
    assert int(np.diff(offs.astype(np.int64))[c0:].min()) == n - 1 > 256
    for n_points in (100, 127):
        words, _ = ctx.accessible_points(*cols, 1.4, n_points)
        assert np.array_equal(words, pm.pack(pm.exposed_masks(*cols, 1.4, n_points, 8)))


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
        words, sasa = ctx.accessible_points_batch(*cat, so, 1.4, n_points)
        assert words.shape == (int(so[-1]), pm.words_of(n_points))
        for s, p in enumerate(parts):
            b, e = int(so[s]), int(so[s + 1])
            if e == b:
                continue
            w1, s1 = ctx.accessible_points(*p, 1.4, n_points)
            assert np.array_equal(words[b:e], w1) and sasa[b:e].tobytes() == s1.tobytes()
        assert np.array_equal(words[so[2]:so[3]],
                              pm.pack(pm.exposed_masks(*parts[2], 1.4, n_points, 8)))
        assert words[so[1]].tolist() == [0xFFFFFFFF] * (n_points // 32) + ([(1 << (n_points % 32)) - 1]
                                                                         if n_points % 32 else [])


def test_proteome_popcounts_equal_sasa_path(ctx):
    b = bw.synthetic_proteome(n_structures=500)
    words, sasa = ctx.accessible_points_batch(b.x, b.y, b.z, b.radius, b.ids, b.structure_offsets, 1.4, 100)
    want, _ = ctx.calculate_sasa_batch(b.x, b.y, b.z, b.radius, b.ids, b.structure_offsets, 1.4, 100)
    _check_masks(words, 100)
    assert pm.sasa_of(b.radius, 1.4, _popcount(words), 100).tobytes() == want.tobytes()
    assert sasa.tobytes() == want.tobytes()


# ---- 7: the reference's sanity cases at 50 000 points -----------------------------------------------------------

def test_sanity_cases_50000_points(ctx):
    n = 50_000
    full = np.full(pm.words_of(n), 0xFFFFFFFF, np.uint32)
    full[-1] = (1 << (n % 32)) - 1
    f = lambda *a: np.array(a, np.float32)  # noqa: E731
    words, sasa = ctx.accessible_points(f(0), f(0), f(0), f(1.5), None, 1.4, n)      # a lone sphere
    assert np.array_equal(words[0], full)
    words, _ = ctx.accessible_points(f(0, 0.1), f(0, 0), f(0, 0), f(1.0, 3.0), None, 1.4, n)  # one inside the other
    assert not words[0].any() and np.array_equal(words[1], full)
    words, _ = ctx.accessible_points(f(0, 50), f(0, 0), f(0, 0), f(1.5, 1.5), None, 1.4, n)  # two far spheres
    assert np.array_equal(words, np.stack([full, full]))


# ---- 8: non-finite input -----------------------------------------------------------------------------------------

def test_nan_coordinate_and_radius(ctx):
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    x, r = x.copy(), r.copy()
    x[5] = np.nan
    r[17] = np.nan
    for n_points in (100, 101):
        words, sasa = ctx.accessible_points(x, y, z, r, ids, 1.4, n_points)
        full = pm.pack(np.ones((1, n_points), bool))[0]
        assert np.array_equal(words[5], full) and np.array_equal(words[17], full)
        assert np.isnan(sasa[17]) and not np.isnan(sasa[5])
        assert np.array_equal(words, pm.pack(pm.exposed_masks(x, y, z, r, ids, 1.4, n_points, 8)))
        want, _ = ctx.calculate_sasa_batch(x, y, z, r, ids, np.array([0, len(x)], np.uint32), 1.4, n_points)
        assert sasa.tobytes() == want.tobytes()


def test_infinite_coordinate_then_usable(ctx):
    import rustsasa_amd
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    bad = x.copy()
    bad[3] = np.inf
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.accessible_points(bad, y, z, r, ids, 1.4, 100)
    assert e.value.status == -5
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.accessible_points_batch(bad, y, z, r, ids, np.array([0, len(x)], np.uint32), 1.4, 100)
    assert e.value.status == -5
    words, _ = ctx.accessible_points(x, y, z, r, ids, 1.4, 100)
    assert np.array_equal(words, pm.pack(pm.exposed_masks(x, y, z, r, ids, 1.4, 100, 8)))


def test_argument_errors_from_the_library(ctx):
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    lib = _capi.load()
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    n = len(x)
    words = np.zeros((n, 4), np.uint32)
    assert lib.rsasa_accessible_points(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), n, 1.4, 0, ptr(words),
                                       None) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert lib.rsasa_accessible_points(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), n, -5.0, 100, ptr(words),
                                       None) == _capi.RSASA_ERR_INVALID_ARGUMENT      # probe + max_r <= 0
    so = np.array([0, 600, 500, n], np.uint32)
    assert lib.rsasa_accessible_points_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), 3, 1.4, 100,
                                             ptr(words), None) == _capi.RSASA_ERR_INVALID_ARGUMENT
    # out_sasa is optional; the context is still usable
    assert lib.rsasa_accessible_points(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), n, 1.4, 100, ptr(words),
                                       None) == _capi.RSASA_OK
    assert np.array_equal(words, pm.pack(pm.exposed_masks(x, y, z, r, ids, 1.4, 100, 8)))


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
    words, _ = ctx.accessible_points(x, y, z, r, ids, 1.4, 100)
    ctx.wait()
    assert out.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    assert np.array_equal(words, pm.pack(pm.exposed_masks(x, y, z, r, ids, 1.4, 100, 8)))


# ---- 10: surface_points ------------------------------------------------------------------------------------------

def test_surface_points_1jcd(ctx):
    from rustsasa_amd import sphere_points
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    probe, n = 1.4, 100
    words, _ = ctx.accessible_points(x, y, z, r, ids, probe, n)
    atom, xyz = ctx.surface_points(x, y, z, r, ids, probe, n)
    assert len(atom) == int(_popcount(words).sum()) > 0
    mask = pm.exposed_masks(x, y, z, r, ids, probe, n, 8)
    ai, pi = np.nonzero(mask)
    assert np.array_equal(atom, ai.astype(np.uint32))
    sx, sy, sz = sphere_points(n)
    R = r[ai] + np.float32(probe)
    want = np.stack([x[ai] + R * sx[pi], y[ai] + R * sy[pi], z[ai] + R * sz[pi]], axis=1)
    assert want.dtype == np.float32 and xyz.tobytes() == want.tobytes()
