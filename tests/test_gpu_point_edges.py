"""Point masks and contact counts (rsasa_accessible_points*, rsasa_contact_points*, points.hip) at the edges of their
own kernels, against the exact models (points_model.py, contacts_model.py) and the oracle.  The cases are built around
the kernels' constants:

  - a wave takes 64 points per chunk (kWave) and NCH chunks per pass; the launcher takes NCH = 2 up to 128 points and
    NCH = 4 above: dead chunks (n <= 64; 129 .. 192), both sides of 128 / 129, exactly one pass (256), the smallest
    second pass (257: one live chunk of four), two passes and one point more (512 / 513)
  - each chunk's ballot is two 32-bit mask words, written under `wi < words`: one word (n < 32), odd word counts, the
    padding bits of the last word
  - n_fused = n - n % W splits the fused rule from the remainder rule, and the REM instantiation is chosen per pass:
    every point a remainder point, the remainder alone in a later chunk, the remainder alone in the second pass
  - the list is staged in LDS kPtStage = 256 entries at a time, in groups of four padded with (0, 0, 0, -inf): lists of
    1 .. 5, 255 .. 260, 511 .. 513 and 768 entries, one pass and several, and 866 .. 1 051 entries (four and five
    stages) on a real structure where the early exit of k_accessible_points fires and the next pass stages again from
    entry 0
  - limit = (t - d^2 - R^2) / 2R with R = r + probe zero, negative, tiny and huge
  - the contact tests (ct_test) at every exact tie of tie_cases.py
  - the lattice cached by n_points and the nb_* / pt_* / ct_* buffers through one context's calls of every kind
  - the order of the atoms: a permutation of the input permutes the result.

The cluster cross product of test 2 is thinned at 960 points (the models' expensive part): all fifteen cluster sizes
run at 100 points (one pass of two chunks), 130 (one pass of four chunks, one dead, the remainder alone in its third)
and 300 (two passes; W = 16 with a remainder in the second, W = 1 without); at 960 points (four passes, no remainder)
one size per stage class runs: K = 4 (one short stage), 256 (one full stage, the last list staged once), 257 (two
stages, three padding entries), 259 (K % 4 = 3), 513 (three stages) and 768 (three full stages).

Every comparison is exact: np.array_equal or a byte comparison."""
import functools

import numpy as np
import pytest

import bench_workloads as bw
import nb_helpers as nh
import point_edge_cases as pe
import points_model as pm
import tie_cases as tc
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

WS = pe.WS
EDGE_POINTS = pe.EDGE_POINTS
EDGE_FIXTURES = ("1jcd.pdb", "example.cif:vdw")
CLUSTER_POINTS = (100, 130, 300, 960)
CLUSTER_WS = (1, 16)
CLUSTERS_AT_960 = (5, 257, 258, 260, 514, 769)
FULL_LIST_SETTINGS = pe.FULL_LIST_SETTINGS
FULL_LIST_POINTS = (100, 300)
FULL_LIST_WS = (8, 16)
DEGENERATE_POINTS = (100, 271)


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


def _cluster_keys():
    return [(n, p) for p in CLUSTER_POINTS for n in pe.CLUSTER_SIZES if p != 960 or n in CLUSTERS_AT_960]


_full_list_cols = pe.full_list_cols


def _degenerate(k):
    cols = nh.protor("1jcd.pdb")
    label, probe, r = pe.degenerate_settings(cols[3])[k]
    return label, pe.with_radii(cols, r), probe


@pytest.fixture(scope="module")
def edge_models():
    """{(fixture, n_points): models} of test 1, computed once on at most 16 threads."""
    return pe.pmap(lambda k: pe.models(pe.fixture(k[0]), 1.4, k[1]), [(f, n) for f in EDGE_FIXTURES for n in EDGE_POINTS])


@pytest.fixture(scope="module")
def cluster_models():
    return pe.pmap(lambda k: pe.models(nh.tight_cluster(k[0], seed=k[0])[0], 1.4, k[1], CLUSTER_WS), _cluster_keys())


@pytest.fixture(scope="module")
def full_list_models():
    def one(k):
        cols, probe = _full_list_cols(k[0])
        return pe.models(cols, probe, k[1], FULL_LIST_WS)
    return pe.pmap(one, [(s, n) for s in FULL_LIST_SETTINGS for n in FULL_LIST_POINTS])


@pytest.fixture(scope="module")
def degenerate_models():
    def one(k):
        _, cols, probe = _degenerate(k[0])
        return pe.models(cols, probe, k[1])
    return pe.pmap(one, [(s, n) for s in range(10) for n in DEGENERATE_POINTS])


def _check_masks(words, n_atoms, n_points):
    assert words.dtype == np.uint32 and words.shape == (n_atoms, (n_points + 31) // 32)
    if n_points % 32:
        assert not (words[:, -1] >> np.uint32(n_points % 32)).any()  # the padding bits are 0


def _check_shapes(got, n_atoms):
    offs, ent, cov, exc, sasa = got
    assert offs.dtype == np.uint64 and offs.shape == (n_atoms + 1,)
    assert cov.dtype == np.uint32 and exc.dtype == np.uint32 and sasa.dtype == np.float32
    assert cov.shape == exc.shape == ent.shape == (int(offs[-1]),) and sasa.shape == (n_atoms,)


def _check_against_models(ctx, cols, probe, n_points, W, model, batch=False):
    """accessible_points and contact_points at the context's lane count W: masks, lists and counts equal the models,
    every sasa output equals the oracle at W byte for byte; batch: the _batch forms equal the single forms."""
    offs_m, ent_m, by_w = model
    mask_m, cov_m, exc_m, _ = by_w[W]
    n = len(cols[0])
    words, sasa = ctx.accessible_points(*cols, probe, n_points)
    _check_masks(words, n, n_points)
    assert np.array_equal(words, pm.pack(mask_m)), (n_points, W)
    got = ctx.contact_points(*cols, probe, n_points)
    _check_shapes(got, n)
    nh.assert_same(got[:2], (offs_m, ent_m))
    assert np.array_equal(got[2], cov_m), (n_points, W)
    assert np.array_equal(got[3], exc_m), (n_points, W)
    oracle = po.calculate_sasa_internal(*cols, probe, n_points, W, threads=0)
    assert sasa.tobytes() == oracle.tobytes() and got[4].tobytes() == oracle.tobytes(), (n_points, W)
    if batch:
        so = np.array([0, n], np.uint32)
        bwords, bsasa = ctx.accessible_points_batch(*cols, so, probe, n_points)
        assert bwords.tobytes() == words.tobytes() and bwords.shape == words.shape
        assert bsasa.tobytes() == oracle.tobytes()
        bgot = ctx.contact_points_batch(*cols, so, probe, n_points)
        for k in range(5):
            assert bgot[k].tobytes() == got[k].tobytes(), k
        want, _ = ctx.calculate_sasa_batch(*cols, so, probe, n_points)   # (a cross-check: the SASA path of this build)
        assert want.tobytes() == oracle.tobytes()
    return words, got


# ---- 1: point counts around chunks, words, passes and the two kernel instantiations -----------------------------

def test_edge_point_classes():
    pe.assert_edge_point_classes()
    nf = {(n, W): tc.n_fused(n, W) for n in EDGE_POINTS for W in WS}
    assert nf[(15, 16)] == 0 and nf[(3, 4)] == 0                    # every point a remainder point
    assert nf[(130, 16)] == 128 and nf[(67, 4)] == 64               # the remainder alone in a later chunk
    assert nf[(259, 16)] == 256 and nf[(271, 16)] == 256 and nf[(257, 8)] == 256   # ... alone in the second pass


@pytest.mark.parametrize("n_points", EDGE_POINTS)
@pytest.mark.parametrize("name", EDGE_FIXTURES)
def test_edge_point_counts(ctx, edge_models, name, n_points):
    cols = pe.fixture(name)
    try:
        for W in WS:
            ctx.set_simd_width(W)
            _check_against_models(ctx, cols, 1.4, n_points, W, edge_models[(name, n_points)], batch=True)
    finally:
        ctx.set_simd_width(8)


# ---- 2: list lengths around the staging, one pass and several ---------------------------------------------------

@pytest.mark.parametrize("n,n_points", _cluster_keys())
def test_cluster_list_lengths_around_the_staging(ctx, cluster_models, n, n_points):
    cols, c0 = nh.tight_cluster(n, seed=n)
    model = cluster_models[(n, n_points)]
    k = np.diff(model[0].astype(np.int64))
    assert k[c0:].min() == k[c0:].max() == n - 1 and k[:c0].max() < pe.PT_STAGE   # K = n - 1 in the whole cluster
    try:
        for W in CLUSTER_WS:
            ctx.set_simd_width(W)
            _check_against_models(ctx, cols, 1.4, n_points, W, model)
    finally:
        ctx.set_simd_width(8)


def test_cluster_classes():
    ks = [n - 1 for n in pe.CLUSTER_SIZES]
    assert {1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 768} <= set(ks)
    near = [k for k in ks if 256 < k < 262]
    assert {k % 4 for k in near} == {0, 1, 2, 3}                    # every padding count next to a stage boundary
    stages = lambda k: -(-k // pe.PT_STAGE)  # noqa: E731
    assert {stages(n - 1) for n in CLUSTERS_AT_960} == {stages(k) for k in ks} == {1, 2, 3}
    assert tc.n_fused(300, 16) == 288 > 256 and tc.n_fused(300, 1) == 300 and tc.n_fused(960, 16) == 960
    assert tc.n_fused(130, 16) == 128 and pe.nch(100) == 2 and pe.nch(130) == 4


# ---- 3: five stages on a real structure, nearly everything buried -----------------------------------------------

@pytest.mark.parametrize("n_points", FULL_LIST_POINTS)
@pytest.mark.parametrize("setting", sorted(FULL_LIST_SETTINGS))
def test_lists_of_every_atom(ctx, full_list_models, setting, n_points):
    cols, probe = _full_list_cols(setting)
    n = len(cols[0])
    model = full_list_models[(setting, n_points)]
    k = np.diff(model[0].astype(np.int64))
    pe.assert_full_lists(setting, k)
    for W in FULL_LIST_WS:
        mask = model[2][W][0]
        assert 0 < mask.sum() < 0.5 * mask.size             # the early exit fires; some atom sweeps every stage
        assert int((~mask.any(axis=1)).sum()) > n // 2      # most atoms are buried completely
    try:
        for W in FULL_LIST_WS:
            ctx.set_simd_width(W)
            _check_against_models(ctx, cols, probe, n_points, W, model, batch=True)
    finally:
        ctx.set_simd_width(8)


# ---- 4: radii and probes off the protein range ------------------------------------------------------------------

@pytest.mark.parametrize("n_points", DEGENERATE_POINTS)
@pytest.mark.parametrize("k", range(10))
def test_degenerate_radii_and_probes(ctx, degenerate_models, k, n_points):
    label, cols, probe = _degenerate(k)
    try:
        for W in WS:
            ctx.set_simd_width(W)
            _check_against_models(ctx, cols, probe, n_points, W, degenerate_models[(k, n_points)], batch=True)
    finally:
        ctx.set_simd_width(8)


@functools.lru_cache(maxsize=None)
def _ordinary():
    b = bw.synthetic_proteome(30, seed=8)
    return tuple(b.structure(0)), tuple(b.structure(4))


def _degenerate_batch(k):
    """The degenerate copy of 1jcd between two ordinary structures: (columns, structure offsets, probe)."""
    label, cols, probe = _degenerate(k)
    first, last = _ordinary()
    parts = [first, cols, last]
    so = np.zeros(len(parts) + 1, np.uint32)
    so[1:] = np.cumsum([len(p[0]) for p in parts])
    return [np.ascontiguousarray(np.concatenate([p[j] for p in parts])) for j in range(5)], so, probe


DEGENERATE_BATCH = (100, 16)   # n_points, W: n_fused = 96, both rules


@pytest.fixture(scope="module")
def degenerate_batch_models():
    def one(k):
        cat, so, probe = _degenerate_batch(k)
        return pe.batch_models(*cat, so, probe, *DEGENERATE_BATCH)
    _ordinary()   # (built once, before the threads start)
    return pe.pmap(one, range(10))


@pytest.mark.parametrize("k", range(10))
def test_degenerate_radii_and_probes_in_a_batch(ctx, degenerate_batch_models, k):
    """One grid and one largest radius per structure: the ordinary neighbours keep their own lists."""
    cat, so, probe = _degenerate_batch(k)
    n_points, W = DEGENERATE_BATCH
    mask_m, cov_m, exc_m = degenerate_batch_models[k]
    oracle = po.calculate_sasa_batch(*cat, so, probe, n_points, W, threads=0)
    try:
        ctx.set_simd_width(W)
        words, sasa = ctx.accessible_points_batch(*cat, so, probe, n_points)
        got = ctx.contact_points_batch(*cat, so, probe, n_points)
    finally:
        ctx.set_simd_width(8)
    _check_masks(words, int(so[-1]), n_points)
    assert np.array_equal(words, pm.pack(mask_m))
    _check_shapes(got, int(so[-1]))
    nh.assert_same(got[:2], nh.oracle_batch_csr(*cat, so, probe))
    assert np.array_equal(got[2], cov_m) and np.array_equal(got[3], exc_m)
    assert sasa.tobytes() == oracle.tobytes() and got[4].tobytes() == oracle.tobytes()


# ---- 5: every tie case through the contact kernel ---------------------------------------------------------------

def test_tie_cases_contacts(ctx):
    groups = {}
    for case in tc.all_cases():
        groups.setdefault((case.probe, case.n_points, case.W), []).extend(case.structures)
    n = 0
    try:
        for (probe, n_points, W), sts in sorted(groups.items()):
            x, y, z, r, ids, so = tc.pack(sts)
            ctx.set_simd_width(W)
            got = ctx.contact_points_batch(x, y, z, r, ids, so, probe, n_points)
            _check_shapes(got, int(so[-1]))
            nh.assert_same(got[:2], nh.oracle_batch_csr(x, y, z, r, ids, so, probe))
            _, cov_m, exc_m = pe.batch_models(x, y, z, r, ids, so, probe, n_points, W)
            assert np.array_equal(got[2], cov_m), (probe, n_points, W)
            assert np.array_equal(got[3], exc_m), (probe, n_points, W)
            oracle = po.calculate_sasa_batch(x, y, z, r, ids, so, probe, n_points, W, threads=0)
            assert got[4].tobytes() == oracle.tobytes(), (probe, n_points, W)
            n += len(sts)
    finally:
        ctx.set_simd_width(8)
    assert n > 10000


# ---- 6: a permutation of the atoms permutes the result ----------------------------------------------------------

def _entry_table(cols, offs, ent, cov, exc, to_old=None):
    """Every entry as (atom, d^2 bits, idx, threshold bits, covered, exclusive), atoms and idx in the numbering
    `to_old` maps to, each atom's entries sorted by (d^2, idx)."""
    x, y, z = cols[:3]
    rows = np.repeat(np.arange(len(x), dtype=np.int64), np.diff(offs.astype(np.int64)))
    j = ent["idx"].astype(np.int64)
    dx, dy, dz = x[rows] - x[j], y[rows] - y[j], z[rows] - z[j]
    d2 = dx * dx + dy * dy + dz * dz
    assert d2.dtype == np.float32
    if to_old is not None:
        rows, j = to_old[rows], to_old[j]
    t = np.stack([rows, d2.view(np.uint32).astype(np.int64), j,
                  np.ascontiguousarray(ent["threshold_squared"]).view(np.uint32).astype(np.int64),
                  cov.astype(np.int64), exc.astype(np.int64)], axis=1)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


@pytest.mark.parametrize("which", ["151L_H3", "cluster_300"])
def test_permuting_the_atoms_permutes_the_result(ctx, which):
    cols = nh.protor("151L_H3.pdb") if which == "151L_H3" else nh.tight_cluster(300, seed=300)[0]
    n, n_points, W = len(cols[0]), 130, 16
    model = pe.models(cols, 1.4, n_points, (W,))
    mask_m, cov_m, exc_m, _ = model[2][W]
    lens_m = np.diff(model[0].astype(np.int64))
    want_table = _entry_table(cols, model[0], model[1], cov_m, exc_m)
    want_sasa = po.calculate_sasa_internal(*cols, 1.4, n_points, W, threads=0)
    try:
        ctx.set_simd_width(W)
        _check_against_models(ctx, cols, 1.4, n_points, W, model)
        for seed in (1, 2, 3):
            perm = np.random.default_rng(seed).permutation(n)        # new atom i is old atom perm[i]
            pc = tuple(np.ascontiguousarray(a[perm]) for a in cols)
            words, sasa = ctx.accessible_points(*pc, 1.4, n_points)
            assert np.array_equal(words, pm.pack(mask_m)[perm])
            assert sasa.tobytes() == want_sasa[perm].tobytes()
            got = ctx.contact_points(*pc, 1.4, n_points)
            _check_shapes(got, n)
            assert np.array_equal(np.diff(got[0].astype(np.int64)), lens_m[perm])
            assert got[4].tobytes() == want_sasa[perm].tobytes()
            assert np.array_equal(_entry_table(pc, *got[:4], to_old=perm), want_table)
    finally:
        ctx.set_simd_width(8)


# ---- 7: one context, many calls ---------------------------------------------------------------------------------

def test_one_context_through_point_and_contact_calls():
    """A fresh context through accessible_points, contact_points, their _batch forms, precompute_neighbors,
    calculate_sasa_batch and surface_points: n_points 960, 100, 960, 64, 50 000, 1, 129, 100 (the cached lattice
    shrinks, grows and is hit again from both families), sizes big, small, big, lane counts changed in between, a
    sparse structure whose grid overflows the remembered cells, a call that fails on an infinite coordinate, then the
    first calls again.  The big batch is checked against the oracle's values and lists and the sum rules."""
    import rustsasa_amd
    big = bw.synthetic_proteome(30, seed=8)
    bigc = (big.x, big.y, big.z, big.radius, big.ids)
    bso = big.structure_offsets
    small = nh.protor("1jcd.pdb")
    rng = np.random.default_rng(31)
    sp = (rng.uniform(0, 1, (300, 3)) * np.array([30000.0, 100.0, 100.0])).astype(np.float32)  # ~9 M cells
    sparse = (sp[:, 0].copy(), sp[:, 1].copy(), sp[:, 2].copy(), rng.uniform(1.2, 2.0, 300).astype(np.float32),
              np.arange(300, dtype=np.uint64))
    f = lambda *a: np.array(a, np.float32)  # noqa: E731
    two = (f(0, 0.1), f(0, 0), f(0, 0), f(1.0, 3.0), None)          # atom 0 inside atom 1
    assert big.n_atoms * 20 < 9_000_000 and big.n_structures == 30
    mkeys = {"small100": (small, 100, 16), "small64": (small, 64, 4), "small1": (small, 1, 8),
             "sparse129": (sparse, 129, 4), "two50000": (two, 50_000, 8)}
    M = pe.pmap(lambda k: pe.models(mkeys[k][0], 1.4, mkeys[k][1], (mkeys[k][2],)), mkeys)
    big_lists = nh.oracle_batch_csr(*bigc, bso)
    big_sasa = {n: po.calculate_sasa_batch(*bigc, bso, 1.4, n, 8, threads=0) for n in (960, 100)}
    big_rows = np.repeat(np.arange(big.n_atoms), np.diff(big_lists[0].astype(np.int64)))
    seen = {}

    def big_points(c, n_points):
        words, sasa = c.accessible_points_batch(*bigc, bso, 1.4, n_points)
        _check_masks(words, big.n_atoms, n_points)
        assert sasa.tobytes() == big_sasa[n_points].tobytes()
        assert pm.sasa_of(big.radius, 1.4, pe.popcount(words), n_points).tobytes() == big_sasa[n_points].tobytes()
        seen[n_points] = n_points - pe.popcount(words)

    def big_contacts(c, n_points):
        got = c.contact_points_batch(*bigc, bso, 1.4, n_points)
        _check_shapes(got, big.n_atoms)
        nh.assert_same(got[:2], big_lists)
        assert got[4].tobytes() == big_sasa[n_points].tobytes()
        buried = seen[n_points]
        s_cov, s_exc, m_cov = (np.zeros(big.n_atoms, np.int64) for _ in range(3))
        np.add.at(s_cov, big_rows, got[2].astype(np.int64))
        np.add.at(s_exc, big_rows, got[3].astype(np.int64))
        np.maximum.at(m_cov, big_rows, got[2].astype(np.int64))
        assert np.all(s_exc <= buried) and np.all(buried <= s_cov) and np.all(m_cov <= buried)
        assert np.all(got[3] <= got[2]) and int(got[2].max()) <= n_points

    def modelled(c, key, batch=False):
        cols, n_points, W = mkeys[key]
        c.set_simd_width(W)
        return _check_against_models(c, cols, 1.4, n_points, W, M[key], batch=batch)

    def surface(c):
        from rustsasa_amd import sphere_points
        x, y, z, r, ids = small
        c.set_simd_width(16)
        atom, xyz = c.surface_points(x, y, z, r, ids, 1.4, 100)
        ai, pi = np.nonzero(M["small100"][2][16][0])
        sx, sy, sz = sphere_points(100)
        R = r[ai] + np.float32(1.4)
        want = np.stack([x[ai] + R * sx[pi], y[ai] + R * sy[pi], z[ai] + R * sz[pi]], axis=1)
        assert np.array_equal(atom, ai.astype(np.uint32)) and xyz.tobytes() == want.tobytes()

    def infinite(c):
        bad = small[0].copy()
        bad[3] = np.inf
        for call in (c.accessible_points, c.contact_points):
            with pytest.raises(rustsasa_amd.RsasaError) as e:
                call(bad, *small[1:], 1.4, 100)
            assert e.value.status == -5

    def neighbours(c, cols, want):
        nh.assert_same(c.precompute_neighbors(*cols, 1.4), want)

    def sasa_big(c, n_points):
        got, _ = c.calculate_sasa_batch(*bigc, bso, 1.4, n_points)
        assert got.tobytes() == big_sasa[n_points].tobytes()

    def w8(c):
        c.set_simd_width(8)

    first = [lambda c: big_points(c, 960),                          # 960, big, W = 8
             lambda c: modelled(c, "small100", batch=True),         # 100, small, W = 16
             w8,
             lambda c: big_contacts(c, 960)]                        # 960 again, from the contact side, big
    seq = first + [
        lambda c: modelled(c, "small64", batch=True),               # 64: one chunk of the NCH = 2 kernel, W = 4
        lambda c: modelled(c, "two50000"),                          # 50 000 points, two atoms
        lambda c: modelled(c, "small1", batch=True),                # 1 point
        lambda c: neighbours(c, sparse, M["sparse129"][:2]),        # the cell array regrows
        lambda c: modelled(c, "sparse129", batch=True),             # 129: the NCH = 4 kernel, W = 4
        infinite,
        w8,
        lambda c: sasa_big(c, 100),
        surface,                                                    # 100 again (W = 16)
        lambda c: neighbours(c, small, M["small100"][:2]),
        w8,
        lambda c: big_points(c, 100),
        lambda c: big_contacts(c, 100),
    ] + first
    with rustsasa_amd.Context(0) as c:
        for step in seq:
            step(c)


# ---- 8: surface_points off the one tested shape -----------------------------------------------------------------

@pytest.mark.parametrize("n_points", [33, 257])
def test_surface_points(ctx, edge_models, n_points):
    from rustsasa_amd import sphere_points
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    probe = 1.4
    atom, xyz = ctx.surface_points(x, y, z, r, ids, probe, n_points)
    mask = edge_models[("1jcd.pdb", n_points)][2][8][0]
    ai, pi = np.nonzero(mask)
    assert len(atom) == len(ai) > 0
    assert np.array_equal(atom, ai.astype(np.uint32))
    sx, sy, sz = sphere_points(n_points)
    R = r[ai] + np.float32(probe)
    want = np.stack([x[ai] + R * sx[pi], y[ai] + R * sy[pi], z[ai] + R * sz[pi]], axis=1)
    assert want.dtype == np.float32 and xyz.tobytes() == want.tobytes()
