"""Group contacts on the GPU (rsasa_group_contacts*: per atom and partner group, the sphere points the group's atoms
occlude among those the atom's own group leaves free, and those no other foreign group occludes; k_group_order and
k_group_points of points.hip) against the exact CPU model of groups_model.py, and against the point, contact and SASA
calls of the same build.  The edge inputs are those of point_edge_cases.py, with labels alternating (index mod 3) and
blocked (runs of 40 atoms).  Every comparison is exact: np.array_equal or a byte comparison."""
import numpy as np
import pytest

import bench_workloads as bw
import groups_model as gm
import nb_helpers as nh
import point_edge_cases as pe
import tail_cases as tl
import tie_cases as tc

pytestmark = pytest.mark.gpu

WS = pe.WS
FIXTURES = ("1jcd.pdb", "2drt.pdb", "freesasa/3w7y.pdb", "freesasa/4c1a.pdb")
FIXTURE_SETTINGS = ((100, 8), (960, 8), (101, 16), (127, 4), (100, 1))   # (n_points, W)
LABELLINGS = ("alternating", "blocked")
CLUSTER_SIZES = (2, 5, 256, 257, 258, 260, 514, 769)
CLUSTER_POINTS = (100, 300)
FULL_LIST_POINTS = (100, 300)
DEGENERATE_POINTS = (100, 271)


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


def labels(kind, n):
    i = np.arange(n, dtype=np.uint32)
    return {"alternating": i % np.uint32(3), "blocked": i // np.uint32(40)}[kind]


def _check_shapes(got, n_atoms):
    offs, partner, buried, only, self_free, free, sasa = got
    assert offs.dtype == np.uint64 and offs.shape == (n_atoms + 1,) and offs[0] == 0
    for a in (partner, buried, only):
        assert a.dtype == np.uint32 and a.shape == (int(offs[-1]),)
    for a in (self_free, free):
        assert a.dtype == np.uint32 and a.shape == (n_atoms,)
    assert sasa.dtype == np.float32 and sasa.shape == (n_atoms,)


def _assert_model(got, model, what=None):
    """got = group_contacts(...), model = groups_model.group_counts(...): element for element."""
    _check_shapes(got, len(model[4]))
    for k, name in enumerate(("offsets", "partner", "buried", "only", "self_free", "free")):
        assert np.array_equal(got[k], model[k]), (name, what)


def _assert_identities(got, groups):
    """Row order and the sum rules on every atom."""
    offs, partner, buried, only, self_free, free, _ = got
    n = len(self_free)
    atom = gm.rows_of(offs)
    assert not (partner == groups[atom]).any()
    same = atom[1:] == atom[:-1]
    assert np.all(partner[1:][same] > partner[:-1][same])          # ascending unsigned, no label twice
    s_bur, m_bur, s_only = (np.zeros(n, np.int64) for _ in range(3))
    np.add.at(s_bur, atom, buried.astype(np.int64))
    np.maximum.at(m_bur, atom, buried.astype(np.int64))
    np.add.at(s_only, atom, only.astype(np.int64))
    lost = self_free.astype(np.int64) - free.astype(np.int64)
    assert np.all(m_bur <= lost) and np.all(lost <= s_bur) and np.all(s_only <= lost)
    one = np.diff(offs.astype(np.int64)) == 1
    assert np.array_equal(lost[one], s_bur[one]) and np.array_equal(lost[one], s_only[one])
    assert np.all(only <= buried)


def _run_both(ctx, cols, groups, probe, n_points):
    """The single and the batch form of one structure: equal byte for byte, sasa that of calculate_sasa_batch."""
    n = len(cols[0])
    so = np.array([0, n], np.uint32)
    got = ctx.group_contacts(*cols, groups, probe, n_points)
    bgot = ctx.group_contacts_batch(*cols, groups, so, probe, n_points)
    for k in range(7):
        assert got[k].tobytes() == bgot[k].tobytes(), k
    want, _ = ctx.calculate_sasa_batch(*cols, so, probe, n_points)
    assert got[6].tobytes() == want.tobytes()
    return got


# ---- 1: fixtures by chain and by residue, single and batch -------------------------------------------------------

@pytest.fixture(scope="module")
def fixture_models():
    fx = {name: gm.labelled_fixture(name) for name in FIXTURES}
    keys = [(name, by, n, W) for name in FIXTURES for by in (1, 2) for n, W in FIXTURE_SETTINGS]
    return fx, pe.pmap(lambda k: gm.group_counts(*fx[k[0]][0], fx[k[0]][k[1]], 1.4, k[2], k[3]), keys)


@pytest.mark.parametrize("by", [1, 2], ids=["chain", "residue"])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_by_chain_and_residue(ctx, fixture_models, name, by):
    fx, models = fixture_models
    cols, groups = fx[name][0], fx[name][by]
    try:
        for n_points, W in FIXTURE_SETTINGS:
            ctx.set_simd_width(W)
            got = _run_both(ctx, cols, groups, 1.4, n_points)
            _assert_model(got, models[(name, by, n_points, W)], (n_points, W))
            _assert_identities(got, groups)
            words, _ = ctx.accessible_points(*cols, 1.4, n_points)
            assert np.array_equal(got[5].astype(np.int64), pe.popcount(words))
    finally:
        ctx.set_simd_width(8)


def test_batch_of_fixtures_with_labels_reused(ctx, fixture_models):
    """Chain numbers start at 0 in every structure: equal values in two structures never meet."""
    fx, models = fixture_models
    parts = [fx[name] for name in FIXTURES]
    empty = tuple(np.zeros(0, np.float32) for _ in range(4)) + (np.zeros(0, np.uint64),)
    cols = [parts[0][0], empty, parts[1][0], parts[2][0], parts[3][0]]
    groups = [parts[0][1], np.zeros(0, np.uint32), parts[1][1], parts[2][1], parts[3][1]]
    so = np.zeros(len(cols) + 1, np.uint32)
    so[1:] = np.cumsum([len(c[0]) for c in cols])
    cat = [np.ascontiguousarray(np.concatenate([c[k] for c in cols])) for k in range(5)]
    g = np.concatenate(groups)
    assert len(set(g.tolist())) < sum(len(p[3]) for p in parts)      # values are reused
    for n_points, W in ((100, 8), (960, 8)):
        got = ctx.group_contacts_batch(*cat, g, so, 1.4, n_points)
        _check_shapes(got, int(so[-1]))
        want = [models[(name, 1, n_points, W)] for name in FIXTURES]
        base = 0
        offs = [np.zeros(1, np.uint64)]
        for m in want:
            offs.append(m[0][1:] + np.uint64(base))
            base += int(m[0][-1])
        assert np.array_equal(got[0], np.concatenate(offs))
        for k in range(1, 6):
            assert np.array_equal(got[k], np.concatenate([m[k] for m in want])), k
        sasa, _ = ctx.calculate_sasa_batch(*cat, so, 1.4, n_points)
        assert got[6].tobytes() == sasa.tobytes()


# ---- 2: the two degenerate labellings against the point and contact calls ----------------------------------------

@pytest.mark.parametrize("n_points,W", [(100, 8), (130, 16), (960, 8)])
@pytest.mark.parametrize("name", ["1jcd.pdb", "151L_H3.pdb"])
def test_all_labels_equal_and_label_is_index(ctx, name, n_points, W):
    cols = nh.protor(name)
    n = len(cols[0])
    try:
        ctx.set_simd_width(W)
        words, sasa = ctx.accessible_points(*cols, 1.4, n_points)
        for value in (0, 7, 0xFFFFFFFF):
            got = _run_both(ctx, cols, np.full(n, value, np.uint32), 1.4, n_points)
            assert int(got[0][-1]) == 0 and not got[0].any() and len(got[1]) == 0
            assert np.array_equal(got[4], got[5]) and np.array_equal(got[5].astype(np.int64), pe.popcount(words))
            assert got[6].tobytes() == sasa.tobytes()
        idx = np.arange(n, dtype=np.uint32)
        got = _run_both(ctx, cols, idx, 1.4, n_points)
        offs, ent, cov, exc, _ = ctx.contact_points(*cols, 1.4, n_points)
        assert np.all(got[4] == n_points) and np.array_equal(got[0], offs)
        by_idx = np.lexsort((ent["idx"], gm.rows_of(offs)))          # the rows are in ascending label = idx order
        assert np.array_equal(got[1], ent["idx"][by_idx])
        assert np.array_equal(got[2], cov[by_idx]) and np.array_equal(got[3], exc[by_idx])
        assert np.array_equal(got[5].astype(np.int64), pe.popcount(words))
        _assert_identities(got, idx)
    finally:
        ctx.set_simd_width(8)


# ---- 3: point counts at the chunk, word and pass edges; n_points % W != 0 ----------------------------------------

@pytest.fixture(scope="module")
def edge_models():
    cols = nh.protor("1jcd.pdb")
    n = len(cols[0])
    keys = [(kind, p, W) for kind in LABELLINGS for p in pe.EDGE_POINTS for W in WS]
    return pe.pmap(lambda k: gm.group_counts(*cols, labels(k[0], n), 1.4, k[1], k[2]), keys)


def test_edge_point_classes():
    pe.assert_edge_point_classes()
    for W in (4, 8, 16):
        assert any(n % W for n in pe.EDGE_POINTS)
    assert all(n % 1 == 0 for n in pe.EDGE_POINTS)                  # W = 1: never a remainder


@pytest.mark.parametrize("n_points", pe.EDGE_POINTS)
@pytest.mark.parametrize("kind", LABELLINGS)
def test_edge_point_counts(ctx, edge_models, kind, n_points):
    cols = nh.protor("1jcd.pdb")
    g = labels(kind, len(cols[0]))
    try:
        for W in WS:
            ctx.set_simd_width(W)
            got = _run_both(ctx, cols, g, 1.4, n_points)
            _assert_model(got, edge_models[(kind, n_points, W)], (n_points, W))
            _assert_identities(got, g)
    finally:
        ctx.set_simd_width(8)


# ---- 4: lists longer than the LDS stage --------------------------------------------------------------------------

def cluster_labels(kind, n_total, c0):
    """The protein by `kind`; the cluster likewise, or (kind "many") every cluster atom a label of its own, descending:
    more rows than the registers of k_group_points hold, and labels in no order."""
    g = labels("blocked" if kind == "many" else kind, n_total)
    if kind == "many":
        g[c0:] = np.uint32(0xFFFFFFFF) - np.arange(n_total - c0, dtype=np.uint32)
    return g


@pytest.fixture(scope="module")
def cluster_models():
    def one(k):
        n, p, kind = k
        cols, c0 = nh.tight_cluster(n, seed=n)
        return gm.group_counts(*cols, cluster_labels(kind, len(cols[0]), c0), 1.4, p, 16)
    return pe.pmap(one, [(n, p, kind) for n in CLUSTER_SIZES for p in CLUSTER_POINTS for kind in LABELLINGS + ("many",)])


@pytest.mark.parametrize("kind", LABELLINGS + ("many",))
@pytest.mark.parametrize("n_points", CLUSTER_POINTS)
@pytest.mark.parametrize("n", CLUSTER_SIZES)
def test_cluster_list_lengths_around_the_staging(ctx, cluster_models, n, n_points, kind):
    cols, c0 = nh.tight_cluster(n, seed=n)
    g = cluster_labels(kind, len(cols[0]), c0)
    model = cluster_models[(n, n_points, kind)]
    if kind == "many":
        assert int(np.diff(model[0].astype(np.int64))[c0:].min()) == n - 1    # a row per entry
    try:
        ctx.set_simd_width(16)
        got = _run_both(ctx, cols, g, 1.4, n_points)
        _assert_model(got, model, (n, n_points, kind))
        _assert_identities(got, g)
    finally:
        ctx.set_simd_width(8)


def test_cluster_classes():
    ks = [n - 1 for n in CLUSTER_SIZES]
    stages = lambda k: -(-k // pe.PT_STAGE)  # noqa: E731
    assert {stages(k) for k in ks} == {1, 2, 3} and {255, 256, 257} <= set(ks)
    assert any(k > 4 * pe.WAVE for k in ks)                          # rows behind the 256 counted in registers
    assert tc.n_fused(300, 16) == 288 > 256 and tc.n_fused(100, 16) == 96


@pytest.fixture(scope="module")
def full_list_models():
    def one(k):
        cols, probe = pe.full_list_cols(k[0])
        return gm.group_counts(*cols, labels(k[2], len(cols[0])), probe, k[1], 8)
    return pe.pmap(one, [(s, p, kind) for s in pe.FULL_LIST_SETTINGS for p in FULL_LIST_POINTS for kind in LABELLINGS])


@pytest.mark.parametrize("kind", LABELLINGS)
@pytest.mark.parametrize("n_points", FULL_LIST_POINTS)
@pytest.mark.parametrize("setting", sorted(pe.FULL_LIST_SETTINGS))
def test_lists_of_every_atom(ctx, full_list_models, setting, n_points, kind):
    cols, probe = pe.full_list_cols(setting)
    g = labels(kind, len(cols[0]))
    model = full_list_models[(setting, n_points, kind)]
    got = _run_both(ctx, cols, g, probe, n_points)
    _assert_model(got, model, (setting, n_points, kind))
    k = np.diff(ctx.precompute_neighbors(*cols, probe)[0].astype(np.int64))
    pe.assert_full_lists(setting, k)
    if kind == "blocked":
        assert int(np.diff(got[0].astype(np.int64)).max()) == 26    # 27 blocks of 40 atoms, one of them the atom's own


# ---- 5: radii and probes off the protein range -------------------------------------------------------------------

def _degenerate(k):
    cols = nh.protor("1jcd.pdb")
    label, probe, r = pe.degenerate_settings(cols[3])[k]
    return pe.with_radii(cols, r), probe


@pytest.fixture(scope="module")
def degenerate_models():
    def one(key):
        k, p, kind, W = key
        cols, probe = _degenerate(k)
        return gm.group_counts(*cols, labels(kind, len(cols[0])), probe, p, W)
    return pe.pmap(one, [(k, p, kind, W) for k in range(10) for p in DEGENERATE_POINTS for kind in LABELLINGS
                         for W in (8, 16)])


@pytest.mark.parametrize("kind", LABELLINGS)
@pytest.mark.parametrize("n_points", DEGENERATE_POINTS)
@pytest.mark.parametrize("k", range(10))
def test_degenerate_radii_and_probes(ctx, degenerate_models, k, n_points, kind):
    cols, probe = _degenerate(k)
    g = labels(kind, len(cols[0]))
    try:
        for W in (8, 16):
            ctx.set_simd_width(W)
            got = _run_both(ctx, cols, g, probe, n_points)
            _assert_model(got, degenerate_models[(k, n_points, kind, W)], (k, n_points, kind, W))
    finally:
        ctx.set_simd_width(8)


# ---- 6: every exact tie ------------------------------------------------------------------------------------------

def test_tie_cases(ctx):
    by_setting = {}
    for case in tc.all_cases():
        by_setting.setdefault((case.probe, case.n_points, case.W), []).extend(case.structures)
    packed = {key: tc.pack(sts) for key, sts in by_setting.items()}

    def tie_labels(kind, so):
        # within each structure: alternating = index mod 2; blocked = the first atom against the rest
        first = np.repeat(so[:-1].astype(np.int64), np.diff(so.astype(np.int64)))
        local = np.arange(int(so[-1]), dtype=np.int64) - first
        return (local % 2 if kind == "alternating" else np.minimum(local, 1)).astype(np.uint32)

    keys = [(key, kind) for key in sorted(packed) for kind in LABELLINGS]
    models = pe.pmap(lambda k: gm.group_counts_batch(*packed[k[0]][:5], tie_labels(k[1], packed[k[0]][5]), packed[k[0]][5],
                                                     k[0][0], k[0][1], k[0][2]), keys)
    n = 0
    try:
        for (probe, n_points, W), kind in keys:
            x, y, z, r, ids, so = packed[(probe, n_points, W)]
            g = tie_labels(kind, so)
            ctx.set_simd_width(W)
            got = ctx.group_contacts_batch(x, y, z, r, ids, g, so, probe, n_points)
            _assert_model(got, models[((probe, n_points, W), kind)], (probe, n_points, W, kind))
            want, _ = ctx.calculate_sasa_batch(x, y, z, r, ids, so, probe, n_points)
            assert got[6].tobytes() == want.tobytes()
            n += len(so) - 1
    finally:
        ctx.set_simd_width(8)
    assert n > 20000


# ---- 7: non-finite input -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", LABELLINGS)
def test_nan_coordinate_and_radius(ctx, kind):
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    x, r = x.copy(), r.copy()
    x[5] = np.nan
    r[17] = np.nan
    g = labels(kind, len(x))
    g[17] = 999                                                        # a label of its own: its rows hold only itself
    for n_points in (100, 101):
        got = _run_both(ctx, (x, y, z, r, ids), g, 1.4, n_points)
        offs, partner, buried, only, self_free, free, sasa = got
        assert offs[5] == offs[6] and offs[17] == offs[18]            # empty lists: no rows, every point free
        assert self_free[5] == free[5] == self_free[17] == free[17] == n_points
        rows17 = partner == 999
        assert rows17.any() and not buried[rows17].any() and not only[rows17].any()   # kept, with zero counts
        _assert_model(got, gm.group_counts(x, y, z, r, ids, g, 1.4, n_points, 8), (kind, n_points))


def test_infinite_coordinate_then_usable(ctx):
    import rustsasa_amd
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    g = labels("blocked", len(x))
    bad = x.copy()
    bad[3] = np.inf
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.group_contacts(bad, y, z, r, ids, g, 1.4, 100)
    assert e.value.status == -5
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.group_contacts_batch(bad, y, z, r, ids, g, np.array([0, len(x)], np.uint32), 1.4, 100)
    assert e.value.status == -5
    _assert_model(ctx.group_contacts(x, y, z, r, ids, g, 1.4, 100), gm.group_counts(x, y, z, r, ids, g, 1.4, 100, 8))


# ---- 8: label values ---------------------------------------------------------------------------------------------

def test_extreme_and_unsorted_labels(ctx):
    cols = nh.protor("1jcd.pdb")
    n = len(cols[0])
    rng = np.random.default_rng(77)
    pool = np.array([0, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 1, 0xFFFFFFFE, 12345], np.uint32)
    g = pool[rng.integers(0, len(pool), n)]                             # in no order along the atoms
    assert (g == 0).any() and (g == 0xFFFFFFFF).any() and np.any(np.diff(g.astype(np.int64)) < 0)
    for n_points in (100, 300):
        got = _run_both(ctx, cols, g, 1.4, n_points)
        _assert_model(got, gm.group_counts(*cols, g, 1.4, n_points, 8), n_points)
        _assert_identities(got, g)
        assert (got[1] == 0).any() and (got[1] == 0xFFFFFFFF).any() and (got[1] >= 0x80000000).any()
        atom = gm.rows_of(got[0])
        k = np.diff(got[0].astype(np.int64))
        i = int(np.argmax(k))
        assert k[i] >= 4 and np.all(np.diff(got[1][atom == i].astype(np.int64)) > 0)


# ---- 9: sizing and argument errors from the library --------------------------------------------------------------

def test_sizing_and_argument_errors_from_the_library(ctx):
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    lib = _capi.load()
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    n = len(x)
    g = labels("blocked", n)
    want = gm.group_counts(x, y, z, r, ids, g, 1.4, 100, 8)
    total = int(want[0][-1])
    so = np.array([0, n], np.uint32)
    sf, fr = np.zeros(n, np.uint32), np.zeros(n, np.uint32)

    def call(offs, grp, bur, onl, cap, sasa=None, n_points=100, probe=1.4, group=g, self_free=sf, free=fr):
        return lib.rsasa_group_contacts(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(group), n, probe, n_points,
                                        ptr(offs), ptr(grp), ptr(bur), ptr(onl), cap, ptr(self_free), ptr(free), ptr(sasa))

    def bcall(offs, grp, bur, onl, cap, so=so, group=g):
        return lib.rsasa_group_contacts_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(group), ptr(so),
                                              len(so) - 1, 1.4, 100, ptr(offs), ptr(grp), ptr(bur), ptr(onl), cap, ptr(sf),
                                              ptr(fr), None)
    cols = [np.full(total, 7, np.uint32) for _ in range(3)]
    for f in (call, bcall):
        # any of the three row buffers NULL, or one row short: the offsets, and nothing else
        for args in ((None, cols[1], cols[2], total), (cols[0], None, cols[2], total), (cols[0], cols[1], None, total),
                     (cols[0], cols[1], cols[2], total - 1), (None, None, None, 0)):
            offs = np.zeros(n + 1, np.uint64)
            sf[:] = 9
            fr[:] = 9
            assert f(offs, *args) == _capi.RSASA_ERR_BUFFER_TOO_SMALL
            assert np.array_equal(offs, want[0])
            assert all((c == 7).all() for c in cols) and (sf == 9).all() and (fr == 9).all()
    # argument errors
    offs = np.zeros(n + 1, np.uint64)
    assert call(offs, *cols, total, group=None) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert bcall(offs, *cols, total, group=None) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert call(offs, *cols, total, self_free=None) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert call(offs, *cols, total, free=None) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert call(offs, *cols, total, n_points=0) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert call(offs, *cols, total, probe=-5.0) == _capi.RSASA_ERR_INVALID_ARGUMENT            # probe + max_r <= 0
    assert call(None, *cols, total) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert bcall(offs, *cols, total, so=np.array([0, 600, 500, n], np.uint32)) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert bcall(offs, *cols, total, so=np.array([1, n], np.uint32)) == _capi.RSASA_ERR_INVALID_ARGUMENT
    assert not offs.any() and all((c == 7).all() for c in cols)
    # out_sasa is optional; the context is still usable; a larger capacity is fine
    big = [np.zeros(total + 5, np.uint32) for _ in range(3)]
    assert call(offs, *big, total + 5) == _capi.RSASA_OK
    _assert_model((offs, big[0][:total], big[1][:total], big[2][:total], sf, fr, np.zeros(n, np.float32)), want)
    sasa = np.zeros(n, np.float32)
    assert call(offs, *big, total + 5, sasa=sasa) == _capi.RSASA_OK
    assert sasa.tobytes() == ctx.calculate_sasa_batch(x, y, z, r, ids, so, 1.4, 100)[0].tobytes()
    # no atoms: offsets [0], whatever the buffers
    o0 = np.ones(1, np.uint64)
    assert lib.rsasa_group_contacts(ctx._h, None, None, None, None, None, None, 0, 1.4, 100, ptr(o0), None, None, None,
                                    0, None, None, None) == _capi.RSASA_OK and o0[0] == 0
    o0 = np.ones(1, np.uint64)
    s0 = np.zeros(1, np.uint32)
    assert lib.rsasa_group_contacts_batch(ctx._h, None, None, None, None, None, None, ptr(s0), 0, 1.4, 100, ptr(o0), None,
                                          None, None, 0, None, None, None) == _capi.RSASA_OK and o0[0] == 0
    got = ctx.group_contacts(*(np.zeros(0, np.float32),) * 4, None, np.zeros(0, np.uint32), 1.4, 100)
    _check_shapes(got, 0)


# ---- 10: a structure that takes the batch-wide binning route ------------------------------------------------------

def test_structure_of_65536_atoms(ctx):
    case = tl.get("2^20+1")
    x, y, z, r, ids, so = case.cols
    n = case.n_atoms
    assert n >= tl.LDS_MAX_ATOMS and len(so) == 2
    g = labels("blocked", n)
    for n_points in (100, 130):
        got = ctx.group_contacts_batch(x, y, z, r, ids, g, so, tl.PROBE, n_points)
        _assert_model(got, gm.group_counts(x, y, z, r, ids, g, tl.PROBE, n_points, 8), n_points)
        _assert_identities(got, g)
        want, _ = ctx.calculate_sasa_batch(x, y, z, r, ids, so, tl.PROBE, n_points)
        assert got[6].tobytes() == want.tobytes()
        assert int(got[0][-1]) > 0 and (got[2] > 0).any()


# ---- 11: next to a device batch in flight -------------------------------------------------------------------------

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
    g = labels("blocked", len(x))
    got = ctx.group_contacts(x, y, z, r, ids, g, 1.4, 100)
    ctx.wait()
    assert out.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    _assert_model(got, gm.group_counts(x, y, z, r, ids, g, 1.4, 100, 8))
