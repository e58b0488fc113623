"""Dot links and dot geodesics on the GPU (rsasa_dot_links*, rsasa_dot_geodesics*, geodesics.hip) against the exact CPU
model (geodesics_model.py: the header's definitions in numpy float32 - lists from components_model.edges_of, distances
by a heap Dijkstra in float32, sources by the tight-edge fixed point).  Lists are sorted by a total key and the distances
are the least solution of a monotone equation, so every comparison is for equality, byte for byte.  The cases
(geodesics_cases.py, component_cases.py, depth_cases.py, sweep_cases.py; pinned by test_geodesics_cpu.py) sit on the
kernels' own edges."""
import functools
import threading

import numpy as np
import pytest

import bench_workloads as bw
import component_cases as cc
import geodesics_cases as gc
import geodesics_model as gm
import points_model as pm
import sweep_cases as sc
import test_gpu_family_walk as fw

pytestmark = pytest.mark.gpu

F = np.float32
INF = F(np.inf)
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


def _case(name):
    if name.startswith("margin_pair"):
        return sc.margin_pair(int(name[len("margin_pair"):]))
    return gc.get(name)


def _link(c, n_points, link=None):
    return cc.default_link(c.r, c.probe, n_points) if link is None else F(link)


@functools.lru_cache(maxsize=None)
def _lists(name, n_points=100, link=None, W=8):
    c = _case(name)
    return gm.links_batch(*c.cols, c.so, c.probe, n_points, _link(c, n_points, link), W)


def _links(ctx, c, n_points=100, link=None):
    return ctx.dot_links_batch(*c.cols, c.so, c.probe, n_points, link)


def _check_links(got, want, c, n_points):
    off, loff, ent, free, sasa = got
    w_off, w_loff, w_ent, mask = want
    assert off.dtype == loff.dtype == np.uint64 and ent.dtype == gm.WITHIN and free.dtype == np.uint32 and sasa.dtype == F
    assert np.array_equal(off, w_off) and np.array_equal(free, mask.sum(axis=1))
    assert np.array_equal(loff, w_loff), np.flatnonzero(loff != w_loff)[:8]
    assert ent.tobytes() == w_ent.tobytes()
    assert sasa.tobytes() == pm.sasa_of(c.r, c.probe, free, n_points).tobytes()


def _symmetric(off, loff, ent, so):
    """Every entry (a -> b, d2) has its twin (b -> a, d2)."""
    import rustsasa_amd
    e = rustsasa_amd.edge_index(loff, ent, rustsasa_amd.dot_structure_offsets(off, so))
    fwd = np.stack([e[0], e[1], ent["d2"].view(np.uint32).astype(np.int64)], -1)
    bwd = fwd[:, [1, 0, 2]]
    key = lambda t: t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]  # noqa: E731
    return np.array_equal(key(fwd), key(bwd)) and not (e[0] == e[1]).any()


def _geo(ctx, c, seeds, n_points=100, limit=None, link=None):
    return ctx.dot_geodesics_batch(*c.cols, c.so, c.probe, n_points, seeds, limit, link, True)


def _want_geo(name, seeds, n_points=100, limit=np.inf, link=None, W=8):
    c = _case(name)
    return gm.geodesics_batch(*c.cols, c.so, c.probe, n_points, _link(c, n_points, link), seeds, limit,
                              lists=_lists(name, n_points, link, W))


def _check_geo(got, want):
    off, dist, free, sasa, source = got
    w_off, w_dist, w_src, mask = want
    assert dist.dtype == F and source.dtype == np.uint32
    assert np.array_equal(off, w_off) and np.array_equal(free, mask.sum(axis=1))
    assert dist.tobytes() == w_dist.tobytes(), np.flatnonzero(dist.view(np.uint32) != w_dist.view(np.uint32))[:8]
    assert np.array_equal(source, w_src), np.flatnonzero(source != w_src)[:8]


# ---- 1: the lists ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["example_vdw", "jcd", "cavity", "corner", "tiny", "overlap_batch"])
def test_lists_equal_the_model(ctx, name):
    c = _case(name)
    got = _links(ctx, c)
    _check_links(got, _lists(name), c, 100)
    assert _symmetric(got[0], got[1], got[2], c.so)
    again = _links(ctx, c)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


@pytest.mark.parametrize("n_points", cc.CHUNK_POINTS)
def test_own_dots_in_several_chunks(ctx, n_points):
    c = _case("multi_chunk")
    _check_links(_links(ctx, c, n_points), _lists("multi_chunk", n_points), c, n_points)


@pytest.mark.parametrize("n_points", [100, cc.CHUNK_POINTS[0]])
@pytest.mark.parametrize("name", ["tiny", "overlap_batch"])
def test_the_lists_span_the_components_of_the_same_sweep(ctx, name, n_points):
    """k_dot_link and k_component_link hold the same sweep twice (reach, staging, chunk loops, edge test), and a change
    made in one of them only shows here: a union-find on the host over the lists, the smallest dot of a tree its root,
    gives the labels of surface_components_batch at the same link, element for element.  65 points: an atom's own dots
    take two chunks of 64 lanes, the second a single point."""
    import rustsasa_amd
    c = _case(name)
    link = _link(c, n_points)
    off, loff, ent, _, _ = _links(ctx, c, n_points, link)
    c_off, labels, _, _ = ctx.surface_components_batch(*c.cols, c.so, c.probe, n_points, link)
    assert np.array_equal(off, c_off) and len(labels) == int(off[-1]) > 0
    first = rustsasa_amd.dot_structure_offsets(off, c.so)
    a, b = rustsasa_amd.edge_index(loff, ent, first)
    parent = list(range(len(labels)))

    def find(d):
        while parent[d] != d:
            parent[d] = d = parent[parent[d]]
        return d

    for u, v in zip(a.tolist(), b.tolist()):
        u, v = find(u), find(v)
        parent[max(u, v)] = min(u, v)
    roots = np.array([find(d) for d in range(len(labels))], np.int64)
    base = np.repeat(first[:-1], np.diff(first))
    assert len(a) > 0 and np.array_equal(roots - base, labels.astype(np.int64))


def test_zero_weight_edges_at_link_zero(ctx):
    c = _case("twins")
    got = _links(ctx, c, 100, 0.0)
    _check_links(got, _lists("twins", 100, 0.0), c, 100)
    assert len(got[2]) == 180 and not got[2]["d2"].any()     # the 90 dots of atom 1 and their twins of atom 2


def test_pole_tie_on_both_sides_of_the_tie(ctx):
    c = _case("pole_tie")
    below = np.nextafter(F(3.0), F(0.0))
    got = _links(ctx, c, 1, F(3.0))
    assert got[1].tolist() == [0, 1, 2] and got[2].tolist() == [(9.0, 1), (9.0, 0)]
    assert _links(ctx, c, 1, below)[1].tolist() == [0, 0, 0]
    _check_links(got, _lists("pole_tie", 1, F(3.0)), c, 1)


def test_far_link_in_six_directions_and_both_orders(ctx):
    c = _case("far_link")
    got = _links(ctx, c, cc.FAR_POINTS, cc.H)
    _check_links(got, _lists("far_link", cc.FAR_POINTS, cc.H), c, cc.FAR_POINTS)
    assert _symmetric(got[0], got[1], got[2], c.so)


@pytest.mark.parametrize("link", [3.0, 5.0, 6.33, 1e4, 1e6])
def test_long_lists_on_a_lone_atom(ctx, link):
    """The sort has no staging, so no length is special; the lists of a lone atom at 960 points pass 64, 256 and 512
    entries on the way to all 959 (R = 3.16: the diameter is 6.32); at 1e4 the reach is the whole grid, and 1e6 is more
    than 65536 h, where k_dot_link stages without its cut."""
    c = _case("lone")
    got = _links(ctx, c, 960, link)
    _check_links(got, _lists("lone", 960, link), c, 960)
    longest = int(np.diff(got[1].astype(np.int64)).max())
    assert longest == 959 if link > 6.32 else 64 < longest < 959


def test_atoms_of_0_1_63_64_and_65_dots(ctx):
    c = _case("dot_counts")
    got = _links(ctx, c, gc.COUNT_POINTS)
    assert got[3][c.info["first"]].tolist() == list(gc.COUNTS)
    _check_links(got, _lists("dot_counts", gc.COUNT_POINTS), c, gc.COUNT_POINTS)


def test_nan_atoms_have_empty_lists(ctx):
    c = _case("corner")
    x, y, z, r, ids = c.cols
    xn, rn = x.copy(), r.copy()
    xn[5] = np.nan
    rn[17] = np.nan
    link = _link(c, 100)
    want = gm.links(xn, y, z, rn, ids, 1.4, 100, link)
    got = ctx.dot_links(xn, y, z, rn, ids, 1.4, 100, link)
    off, loff = got[0].astype(np.int64), got[1].astype(np.int64)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2].tobytes() == want[2].tobytes()
    for i in (5, 17):
        assert off[i + 1] - off[i] == 100 and loff[off[i + 1]] == loff[off[i]]
    # as seeds they are 0, otherwise unreachable
    seeds = np.zeros(int(off[-1]), np.uint8)
    seeds[off[5]] = 1
    _, dist, _, _, src = ctx.dot_geodesics(xn, y, z, rn, ids, 1.4, 100, seeds, None, link, True)
    assert dist[off[5]] == 0 and src[off[5]] == off[5] and np.isinf(np.delete(dist, off[5])).all()


def test_whole_grid_reach_and_structures_that_fail_the_margins(ctx):
    c = _case("corner")
    wide = F(3.0) * cc.H
    _check_links(_links(ctx, c, 100, wide), _lists("corner", 100, float(wide)), c, 100)
    m = _case("margin_pair0")
    _check_links(_links(ctx, m), _lists("margin_pair0"), m, 100)


def test_one_structure_of_65536_atoms(ctx):
    """32-bit cell starts behind three small structures; the masks are the engine's own, as in test_gpu_components.py."""
    import rustsasa_amd
    c = _case("tail")
    words, _ = ctx.accessible_points_batch(*c.cols, c.so, c.probe, 100)
    mask = rustsasa_amd.unpack_points(words, 100).astype(bool)
    want = gm.links_batch(*c.cols, c.so, c.probe, 100, _link(c, 100), mask=mask)
    _check_links(_links(ctx, c), want, c, 100)
    # a patch of 6 A around one dot of the big structure
    D = int(want[0][-1])
    seeds = gc.one_seed(D, D - 1000)
    w = gm.geodesics_batch(*c.cols, c.so, c.probe, 100, _link(c, 100), seeds, 6.0, lists=want)
    _check_geo(_geo(ctx, c, seeds, 100, 6.0), w)
    assert 10 < np.isfinite(w[1]).sum() < 2000


def test_sizing_in_two_calls_and_argument_rules(ctx):
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    lib = _capi.load()
    c = _case("corner")
    x, y, z, r, ids = c.cols
    n = c.n_atoms
    w_off, w_loff, w_ent, _ = _lists("corner")
    D, E = int(w_off[-1]), len(w_ent)
    link = float(_link(c, 100))
    cols = (ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids))
    so = np.array([0, n], np.uint32)
    bad, small, ok = _capi.RSASA_ERR_INVALID_ARGUMENT, _capi.RSASA_ERR_BUFFER_TOO_SMALL, _capi.RSASA_OK
    off, nl = np.zeros(n + 1, np.uint64), np.full(1, 77, np.uint64)
    loff, ent = np.full(D + 1, 0xAB, np.uint64), np.zeros(E, gm.WITHIN)
    ent["idx"] = 0xABCDEF01
    one = lambda *a: lib.rsasa_dot_links(ctx._h, *a)            # noqa: E731
    many = lambda *a: lib.rsasa_dot_links_batch(ctx._h, *a)     # noqa: E731
    tail = (ptr(off), ptr(nl), ptr(loff), D, ptr(ent), E, None, None)
    for v in (float("nan"), -1.0, float("inf")):
        assert one(*cols, n, 1.4, 100, v, *tail) == bad and many(*cols, ptr(so), 1, 1.4, 100, v, *tail) == bad
    assert one(ptr(x), None, ptr(z), ptr(r), ptr(ids), n, 1.4, 100, link, *tail) == bad
    assert one(*cols, n, 1.4, 100, link, None, *tail[1:]) == bad
    assert one(*cols, n, 1.4, 100, link, ptr(off), None, *tail[2:]) == bad
    assert one(*cols, n, 1.4, 0, link, *tail) == bad
    assert many(*cols, None, 1, 1.4, 100, link, *tail) == bad
    assert not off.any() and nl[0] == 77 and (loff == 0xAB).all() and (ent["idx"] == 0xABCDEF01).all()
    # the first call: nothing but the two totals
    assert one(*cols, n, 1.4, 100, link, ptr(off), ptr(nl), None, 0, None, 0, None, None) == small
    assert np.array_equal(off, w_off) and nl[0] == E
    for dots_cap, cap in ((D - 1, E), (D, E - 1)):
        off[:], nl[0] = 0, 77
        assert many(*cols, ptr(so), 1, 1.4, 100, link, ptr(off), ptr(nl), ptr(loff), dots_cap, ptr(ent), cap, None, None) == small
        assert np.array_equal(off, w_off) and nl[0] == E and (loff == 0xAB).all() and (ent["idx"] == 0xABCDEF01).all()
    # the second call
    assert one(*cols, n, 1.4, 100, link, *tail) == ok
    assert np.array_equal(loff, w_loff) and ent.tobytes() == w_ent.tobytes()
    # no atoms
    off[:], nl[0], loff[0] = 7, 77, 7
    assert one(*cols, 0, 1.4, 100, link, *tail) == ok and off[0] == 0 and nl[0] == 0 and loff[0] == 0
    # the geodesics' own rules
    dist, src, seeds = np.full(D, 5, F), np.zeros(D, np.uint32), gc.one_seed(D)
    geo = lambda *a: lib.rsasa_dot_geodesics(ctx._h, *cols, n, 1.4, 100, *a)     # noqa: E731
    for v in (float("nan"), -1.0, -float("inf")):
        assert geo(link, ptr(seeds), D, v, ptr(off), ptr(dist), ptr(src), None, None) == bad
    assert geo(float("inf"), ptr(seeds), D, 3.0, ptr(off), ptr(dist), ptr(src), None, None) == bad
    assert geo(link, ptr(seeds), D, 3.0, None, ptr(dist), ptr(src), None, None) == bad
    assert (dist == 5).all()
    off[:] = 0
    for wrong in (D - 1, D + 1, 0):
        assert geo(link, ptr(seeds), wrong, 3.0, ptr(off), ptr(dist), ptr(src), None, None) == bad
        msg = lib.rsasa_context_last_error(ctx._h).decode()
        assert str(wrong) in msg and str(D) in msg and np.array_equal(off, w_off) and (dist == 5).all()
    assert geo(link, None, D, 3.0, ptr(off), ptr(dist), ptr(src), None, None) == bad
    assert geo(link, ptr(seeds), D, 3.0, ptr(off), None, ptr(src), None, None) == bad
    assert geo(link, ptr(seeds), D, float("inf"), ptr(off), ptr(dist), None, None, None) == ok
    assert dist[0] == 0 and ctx.geodesic_rounds()[0] >= 2 and ctx.geodesic_rounds()[1] == 0
    assert geo(link, ptr(seeds), D, 3.0, ptr(off), ptr(dist), ptr(src), None, None) == ok and min(ctx.geodesic_rounds()) >= 2
    assert lib.rsasa_context_geodesic_rounds(ctx._h, None) == bad and lib.rsasa_context_geodesic_rounds(None, None) == bad
    assert lib.rsasa_dot_geodesics(ctx._h, *cols, 0, 1.4, 100, link, None, 0, 3.0, ptr(off), None, None, None, None) == ok
    assert ctx.geodesic_rounds() == (0, 0)
    assert lib.rsasa_dot_geodesics(ctx._h, *cols, 0, 1.4, 100, link, None, 1, 3.0, ptr(off), None, None, None, None) == bad


# ---- 2: distances and sources ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["example_vdw", "jcd"])
def test_one_seed_with_and_without_a_limit(ctx, name):
    c = _case(name)
    D = int(_lists(name)[0][-1])
    seeds = gc.one_seed(D, D // 3)
    for limit in (np.inf, 12.0):
        want = _want_geo(name, seeds, 100, limit)
        _check_geo(_geo(ctx, c, seeds, 100, None if np.isinf(limit) else limit), want)
    assert 50 < np.isfinite(want[1]).sum() < D // 2                      # a patch


def test_limit_zero_and_the_limit_at_a_tie(ctx):
    c = _case("corner")
    D = int(_lists("corner")[0][-1])
    seeds = gc.one_seed(D, 7)
    full = _want_geo("corner", seeds)[1]
    got = _geo(ctx, c, seeds, 100, 0.0)
    assert got[1][7] == 0 and np.isinf(np.delete(got[1], 7)).all() and got[4][7] == 7
    _check_geo(got, _want_geo("corner", seeds, 100, 0.0))
    # a limit equal to a model distance keeps that dot; one ulp below loses it and what is only reachable through it
    order = np.argsort(full, kind="stable")
    v = int(order[np.isfinite(full).sum() // 2])
    at, below = full[v], np.nextafter(full[v], F(0.0))
    g_at, g_below = _geo(ctx, c, seeds, 100, at), _geo(ctx, c, seeds, 100, below)
    _check_geo(g_at, _want_geo("corner", seeds, 100, at))
    _check_geo(g_below, _want_geo("corner", seeds, 100, below))
    assert g_at[1][v] == at and np.isinf(g_below[1][v]) and g_below[4][v] == NONE
    assert np.isfinite(g_below[1]).sum() < np.isfinite(g_at[1]).sum() <= np.isfinite(full).sum()


def test_no_seeds_all_seeds_and_seeds_in_one_structure_only(ctx):
    c = _case("tiny")
    off = _lists("tiny")[0].astype(np.int64)
    D = int(off[-1])
    got = _geo(ctx, c, np.zeros(D, np.uint8))
    assert np.isinf(got[1]).all() and (got[4] == NONE).all()
    got = _geo(ctx, c, np.full(D, 255, np.uint8))
    _check_geo(got, _want_geo("tiny", np.ones(D, np.uint8)))
    assert not got[1].any()
    seeds = np.zeros(D, np.uint8)
    b, e = int(off[c.so[2]]), int(off[c.so[3]])                      # the two-atom structure
    seeds[b + 3] = 1
    got = _geo(ctx, c, seeds)
    _check_geo(got, _want_geo("tiny", seeds))
    assert np.isfinite(got[1][b:e]).all() and np.isinf(got[1][:b]).all() and np.isinf(got[1][e:]).all()
    assert (got[4][b:e] == 3).all()


def test_a_void_is_unreachable_from_outer_seeds(ctx):
    import rustsasa_amd
    c = _case("cavity")
    off, labels, _, _ = ctx.surface_components_batch(*c.cols, c.so, c.probe, 100)
    outer = np.bincount(labels).argmax()
    seeds = gc.one_seed(len(labels), int(outer))
    got = _geo(ctx, c, seeds)
    _check_geo(got, _want_geo("cavity", seeds))
    assert np.array_equal(np.isfinite(got[1]), labels == outer) and (labels != outer).any()
    sasa, _ = ctx.calculate_sasa_batch(*c.cols, c.so, c.probe, 100)
    assert np.array_equal(got[0], off) and got[3].tobytes() == sasa.tobytes()
    assert np.array_equal(rustsasa_amd.dot_seeds(off, [0]).nonzero()[0], np.arange(int(off[0]), int(off[1])))


def test_of_two_coincident_seeds_the_smaller_wins_everywhere(ctx):
    c = _case("twins")
    off = _lists("twins")[0].astype(np.int64)
    a, b = int(off[1]) + 4, int(off[2]) + 4                          # a dot of atom 1 and its twin of atom 2
    seeds = np.zeros(int(off[-1]), np.uint8)
    seeds[[a, b]] = 1
    got = _geo(ctx, c, seeds)
    _check_geo(got, _want_geo("twins", seeds))
    assert got[1][a] == got[1][b] == 0 and (got[4][np.isfinite(got[1])] == a).all() and np.isfinite(got[1]).sum() > 100


def test_equal_sums_do_not_move_a_source(ctx):
    c = _case("equal_sum")
    got = _geo(ctx, c, c.info["seeds"], 1, None, c.info["link"])
    assert got[1].tolist() == [0.0, 0.0, 1.0, 4.0] and got[4].tolist() == [0, 1, 1, 1]
    _check_geo(got, _want_geo("equal_sum", c.info["seeds"], 1, np.inf, float(c.info["link"])))


def test_a_chain_of_more_hops_than_rounds_between_two_looks(ctx):
    c = _case("chain")
    off, loff, ent, _ = _lists("chain")
    D = int(off[-1])
    seeds = gc.one_seed(D, 0)
    want = _want_geo("chain", seeds)
    _check_geo(_geo(ctx, c, seeds), want)
    assert gm.hops(loff.astype(np.int64), ent["idx"], seeds).max() >= 200
    dist = ctx.dot_geodesics(*c.cols, c.probe, 100, seeds)[1]
    assert dist.tobytes() == want[1].tobytes() and 200 <= ctx.geodesic_rounds()[0] <= D + 1 and ctx.geodesic_rounds()[1] == 0


@pytest.mark.parametrize("W", [1, 16])
def test_lane_counts(W):
    import rustsasa_amd
    c = _case("corner")
    with rustsasa_amd.Context(0, W) as ctx:
        _check_links(_links(ctx, c, 129), _lists("corner", 129, None, W), c, 129)
        seeds = gc.one_seed(int(_lists("corner", 129, None, W)[0][-1]), 11)
        _check_geo(_geo(ctx, c, seeds, 129, 9.0), _want_geo("corner", seeds, 129, 9.0, None, W))


# ---- 3: one context, other families, a batch in flight, threads ----------------------------------------------------------

def test_single_call_equals_batch_call_and_empty_batches(ctx):
    for name in ("cavity", "twins"):
        c = _case(name)
        one = ctx.dot_links(*c.cols, c.probe, 100)
        many = _links(ctx, c)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(one, many))
        seeds = gc.one_seed(int(one[0][-1]), 5)
        g1 = ctx.dot_geodesics(*c.cols, c.probe, 100, seeds, 8.0, None, True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g1, _geo(ctx, c, seeds, 100, 8.0)))
    e = np.zeros(0, F)
    for so in ([0], [0, 0, 0]):
        got = ctx.dot_links_batch(e, e, e, e, np.zeros(0, np.uint64), np.array(so, np.uint32), 1.4, 100)
        assert got[0].tolist() == [0] and got[1].tolist() == [0] and len(got[2]) == 0
        got = ctx.dot_geodesics_batch(e, e, e, e, np.zeros(0, np.uint64), np.array(so, np.uint32), 1.4, 100, np.zeros(0, np.uint8))
        assert got[0].tolist() == [0] and len(got[1]) == 0


def test_walk_through_the_other_families(ctx):
    import rustsasa_amd
    inputs = fw._inputs()

    def both(cx, inp):
        x, y, z, r, ids, _, so = inp
        if so is None:
            lk = cx.dot_links(x, y, z, r, ids, fw.PROBE, 100)
            seeds = gc.one_seed(int(lk[0][-1]), int(lk[0][-1]) // 2)
            return lk + cx.dot_geodesics(x, y, z, r, ids, fw.PROBE, 100, seeds, 15.0, None, True)
        lk = cx.dot_links_batch(x, y, z, r, ids, so, fw.PROBE, 100)
        seeds = gc.one_seed(int(lk[0][-1]), int(lk[0][-1]) // 2)
        return lk + cx.dot_geodesics_batch(x, y, z, r, ids, so, fw.PROBE, 100, seeds, 15.0, None, True)

    alone = {}
    for name, inp in inputs.items():
        with rustsasa_amd.Context(0) as fresh:
            alone[name] = both(fresh, inp)
    for family in fw.ORDER:
        for name in ("B", "A", "C"):
            fw._call(ctx, family, inputs[name], 100)
            assert fw._same(both(ctx, inputs[name]), alone[name]), (family, name)


def test_beside_a_device_batch_in_flight(ctx):
    torch = pytest.importorskip("torch")
    c = _case("cavity")
    b = bw.synthetic_proteome(12, seed=4)
    dev = torch.device("cuda", 0)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cols = (tt(b.x), tt(b.y), tt(b.z), tt(b.radius), tt(b.ids.view(np.int64)))
    alone = torch.zeros(b.n_atoms, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.enqueue_device(*cols, b.structure_offsets, out_atom_sasa=alone, probe_radius=1.4, n_points=100)
    ctx.wait()
    out = torch.zeros(b.n_atoms, dtype=torch.float32, device=dev)
    seeds = gc.one_seed(int(_lists("cavity")[0][-1]), 9)
    torch.cuda.synchronize()
    ctx.enqueue_device(*cols, b.structure_offsets, out_atom_sasa=out, probe_radius=1.4, n_points=100)
    lk = _links(ctx, c)
    g = _geo(ctx, c, seeds, 100, 10.0)
    ctx.wait()
    assert out.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    _check_links(lk, _lists("cavity"), c, 100)
    _check_geo(g, _want_geo("cavity", seeds, 100, 10.0))


def test_eight_threads_on_one_context(ctx):
    names = ["corner", "tiny", "twins", "cavity"]
    seeds = [gc.one_seed(int(_lists(n)[0][-1]), 2) for n in names]
    want = [(_lists(n), _want_geo(n, s, 100, 7.0)) for n, s in zip(names, seeds)]
    errors = []

    def work(t):
        try:
            for k in range(4):
                n = (t + k) % len(names)
                c = _case(names[n])
                _check_links(_links(ctx, c), want[n][0], c, 100)
                _check_geo(_geo(ctx, c, seeds[n], 100, 7.0), want[n][1])
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)[:300]))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:4]
