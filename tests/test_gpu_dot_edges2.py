"""The dot families on the GPU past their first suites (geodesics.hip, patches.hip, gd_phase and ps_run of neighbors.cpp)
against the exact CPU models (geodesics_model.py, patches_model.py), byte for byte, on the cases of dot_edge2_cases.py
(pinned by test_dot_edges2_cpu.py):

  A  every case of the shared sweep's edges (sweep_cases.py) through the three instantiations of k_dot_link - count and
     fill through the lists, the weights through geodesics seeded in the middle of every structure and through patches -
     and the lists against the components of k_component_link, which holds the same sweep a second time;
  B  a path of N dots for N = 1 .. 18, so that the relaxation and the source phase end on every position of a group of
     rounds between two looks of the host, and a dot of 1 201 entries;
  C  the sampler's queue outgrown in the second step of a pick and twice in one structure, and 600 workgroups."""
import functools

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import component_cases as cc
import dot_edge2_cases as d2
import geodesics_cases as gc
import geodesics_model as gm
import patches_model as pmod
import point_edge_cases as pe
import sweep_cases as sc
import test_gpu_geodesics as tgg
import test_gpu_patches as tgp
import test_gpu_sweep_edges as tse

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


@pytest.fixture(scope="module", autouse=True)
def _all_masks():
    pe.pmap(lambda run: tse._masks(*run), tse.RUNS)      # side by side, once; test_gpu_sweep_edges.py finds them there


def _masks(name, n_points):
    """The model's masks of a sweep case: those test_gpu_sweep_edges.py keeps; margin_twelve is the structures of
    margin_under and margin_over in turn, and a structure's masks do not depend on the rest of its batch."""
    if name == "margin_twelve":
        u, o = sc.get("margin_under"), sc.get("margin_over")
        mu, mo = tse._masks("margin_under", n_points), tse._masks("margin_over", n_points)
        rows = lambda c, m, s: m[int(c.so[s]):int(c.so[s + 1])]     # noqa: E731
        return np.concatenate([rows(c, m, s) for s in range(6) for c, m in ((u, mu), (o, mo))])
    return tse._masks(name, n_points)


@functools.lru_cache(maxsize=None)
def _lists(name, n_points, link):
    c = d2.case(name)
    return gm.links_batch(*c.cols, c.so, c.probe, n_points, F(link), mask=_masks(name, n_points))


@functools.lru_cache(maxsize=None)
def _own_lists(name, n_points, link):
    """The lists of a case of dot_edge2_cases.py itself."""
    c = d2.get(name)
    return gm.links_batch(*c.cols, c.so, c.probe, n_points, F(link))


def _check_lists(ctx, c, n_points, link, want):
    got = ctx.dot_links_batch(*c.cols, c.so, c.probe, n_points, link)
    tgg._check_links(got, want, c, n_points)
    assert len(want[2]) == 0 or tgg._symmetric(got[0], got[1], got[2], c.so)
    return got


# ---- A1, A2: count and fill -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n_points", d2.LIST_RUNS)
def test_lists_of_the_sweep_s_edge_cases_equal_the_model(ctx, name, n_points):
    c = d2.case(name)
    link = d2.link_of(name, n_points)
    want = _lists(name, n_points, float(link))
    assert c.n_atoms == len(want[3])
    _check_lists(ctx, c, n_points, link, want)


@pytest.mark.parametrize("n_points,k", [(n, k) for n in sc.CROWDED_POINTS for k in range(len(d2.crowded_links(n)))])
def test_crowded_cells_at_four_links(ctx, n_points, k):
    """Link 0, ball's link, the case's own (waves of 64 staged atoms over many steps, lists over 400) and, at 65 points, a
    link whose reach is the whole grid (every dot linked to every other: 1 625 * 1 624 entries)."""
    c = sc.get("crowded_cells")
    link = d2.crowded_links(n_points)[k]
    want = _lists("crowded_cells", n_points, float(link))
    _check_lists(ctx, c, n_points, link, want)
    longest = int(np.diff(want[1].astype(np.int64)).max())
    assert (longest == 0, 0 < longest < 64, longest > 400, longest == int(want[0][-1]) - 1)[k]


# ---- A3: the weights -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n_points", d2.WEIGHT_RUNS)
def test_geodesics_from_the_middle_of_every_structure(ctx, name, n_points):
    """k_dot_link<kWeights> stores the batch-wide dot number: a seed in the middle of every structure's dots, so that its
    number within the structure, its number in the batch and 0 all differ behind the first structure."""
    c = d2.case(name)
    link = d2.link_of(name, n_points)
    lists = _lists(name, n_points, float(link))
    seeds = d2.middle_seeds(lists[0], c.so)
    n_seeds = int(seeds.sum())
    assert n_seeds == int((np.diff(lists[0].astype(np.int64)[c.so.astype(np.int64)]) > 0).sum()) >= 1
    for limit in (np.inf, d2.finite_limit(name)):
        want = gm.geodesics_batch(*c.cols, c.so, c.probe, n_points, link, seeds, limit, lists=lists)
        got = ctx.dot_geodesics_batch(*c.cols, c.so, c.probe, n_points, seeds, None if np.isinf(limit) else limit, link, True)
        tgg._check_geo(got, want)
        assert np.isfinite(want[1]).sum() >= n_seeds


@pytest.mark.parametrize("name,n_points", [("margin_twelve", 100), ("half_link", cc.FAR_POINTS)])
def test_patches_of_twelve_structures_at_the_sweep_s_edges(ctx, name, n_points):
    c = d2.case(name)
    link = d2.link_of(name, n_points)
    lists = _lists(name, n_points, float(link))
    want = pmod.patches_batch(*c.cols, c.so, c.probe, n_points, link, 6.0, 5, lists=lists)
    got = ctx.dot_patches_batch(*c.cols, c.so, c.probe, n_points, 6.0, 5, link, True)
    tgp._check(got, want, c, n_points)
    assert len(c.so) - 1 == 12 and ctx.patch_stats()[0] == len(want[2]) >= 12


# ---- A4: the lists against the components of the other copy of the sweep ---------------------------------------------------

@pytest.mark.parametrize("name,n_points", d2.CROSS_RUNS)
def test_the_lists_span_the_components_at_the_sweep_s_edges(ctx, name, n_points):
    """test_gpu_geodesics.py's cross test on more of the sweep's edges: the connected components of the lists, the smallest
    dot of each its label, are the labels of surface_components_batch at the same link, element for element."""
    import rustsasa_amd
    c = d2.case(name)
    link = d2.cross_link(name, n_points)
    off, loff, ent, _, _ = ctx.dot_links_batch(*c.cols, c.so, c.probe, n_points, link)
    c_off, labels, _, _ = ctx.surface_components_batch(*c.cols, c.so, c.probe, n_points, link)
    D = int(off[-1])
    assert np.array_equal(off, c_off) and len(labels) == D > 0
    first = rustsasa_amd.dot_structure_offsets(off, c.so)
    a, b = rustsasa_amd.edge_index(loff, ent, first)
    _, comp = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(D, D)), directed=False)
    smallest = np.full(comp.max() + 1, D, np.int64)
    np.minimum.at(smallest, comp, np.arange(D))
    base = np.repeat(first[:-1], np.diff(first))
    assert len(a) > 0 and np.array_equal(smallest[comp] - base, labels.astype(np.int64))
    assert len(np.unique(labels.astype(np.int64) + base)) >= len(c.so) - 1


# ---- B: gd_phase at every position of a group of rounds ---------------------------------------------------------------------

@pytest.mark.parametrize("n", range(1, d2.ROW_MAX + 1))
def test_a_path_of_n_dots_from_either_end_from_both_and_with_a_limit(ctx, n):
    """The relaxation settles at least one hop a round, so it and the source phase take between 1 and n rounds, the empty
    one included: whichever position of a group of kGdRounds rounds the empty round takes, the host must find it there
    and must not give up before (n = 8: the last of the first group at the latest, n = 9: the first of the second)."""
    c = d2.row(n)
    lists = _own_lists("row%d" % n, 1, 1.0)
    line = np.arange(n, dtype=F)
    first, last = gc.one_seed(n, 0), gc.one_seed(n, n - 1)
    limit = (n - 1) / 2
    runs = [(first, None, line, np.zeros(n, np.uint32)),
            (last, None, line[::-1], np.full(n, n - 1, np.uint32)),
            (first | last, None, np.minimum(line, line[::-1]), np.where(line <= line[::-1], 0, n - 1).astype(np.uint32)),
            (first, limit, np.where(line <= F(limit), line, INF), np.where(line <= F(limit), 0, NONE).astype(np.uint32))]
    for seeds, lim, dist, source in runs:
        got = ctx.dot_geodesics(*c.cols, c.probe, 1, seeds, lim, d2.ROW_LINK, True)
        rounds = ctx.geodesic_rounds()
        assert got[1].dtype == F and got[1].tobytes() == dist.astype(F).tobytes(), (lim, got[1])
        assert np.array_equal(got[4], source), (lim, got[4])
        assert 1 <= rounds[0] <= n and 1 <= rounds[1] <= n, rounds
        want = gm.geodesics_batch(*c.cols, c.so, c.probe, 1, d2.ROW_LINK, seeds, np.inf if lim is None else lim, lists=lists)
        tgg._check_geo(got, want)


def test_a_dot_of_1201_entries_through_the_relaxation_and_the_sources(ctx):
    c = d2.hub(1200)
    lists = _own_lists("hub1200", 1, float(d2.HUB_LINK))
    seeds = gc.one_seed(1202, 0)
    want = gm.geodesics_batch(*c.cols, c.so, c.probe, 1, d2.HUB_LINK, seeds, lists=lists)
    got = ctx.dot_geodesics_batch(*c.cols, c.so, c.probe, 1, seeds, None, d2.HUB_LINK, True)
    tgg._check_geo(got, want)
    assert got[1][1] == 9.0 and np.isfinite(got[1]).all() and not got[4].any()
    assert len(np.unique(got[1])) < 1202 - 200                    # hundreds of tied distances


# ---- C1: an overflow in the second step of a pick ------------------------------------------------------------------------------

def _patches(ctx, name, n_points, link, spacing, max_centres=None):
    c = d2.get(name)
    want = pmod.patches_batch(*c.cols, c.so, c.probe, n_points, F(link), spacing, max_centres,
                              lists=_own_lists(name, n_points, float(link)))
    got = ctx.dot_patches_batch(*c.cols, c.so, c.probe, n_points, spacing, max_centres, link, True)
    tgp._check(got, want, c, n_points)
    return got, want


@pytest.mark.parametrize("n_disc", d2.HUB_DISCS)
def test_the_hub_fills_the_queue_in_the_second_step_of_the_first_pick(ctx, n_disc):
    """Step 1 of the only pick lowers the hub, step 2 exactly n_disc dots: PS_QUEUE of them are queued, one more and the
    pick goes on by the stamps - with the dots that the queue did hold among those that must still push."""
    got, _ = _patches(ctx, "hub%d" % n_disc, 1, d2.HUB_LINK, np.inf)
    picks, steps, overflows = ctx.patch_stats()
    assert got[2].tolist() == [0] and picks == 1 and steps >= 3
    assert overflows == (1 if n_disc > d2.PS_QUEUE else 0)


@pytest.mark.parametrize("spacing,max_centres", [(3.0, None), (0.0, 40)])
@pytest.mark.parametrize("n_disc", d2.HUB_DISCS[1:])
def test_the_hub_with_later_picks_that_queue_again(ctx, n_disc, spacing, max_centres):
    got, want = _patches(ctx, "hub%d" % n_disc, 1, d2.HUB_LINK, spacing, max_centres)
    picks, _, overflows = ctx.patch_stats()
    assert picks == len(want[2]) == (5 if max_centres is None else 40) and overflows >= 1


# ---- C2: two overflows in one structure -----------------------------------------------------------------------------------------

def test_two_full_overflows_twice_in_one_structure(ctx):
    P = d2.TWO_FULL_POINTS
    got, _ = _patches(ctx, "two_full", P, d2.TWO_FULL_LINK, np.inf)
    assert got[2].tolist() == [0, P] and np.isinf(got[3]).all() and ctx.patch_stats()[0] == 2 and ctx.patch_stats()[2] == 2
    got, want = _patches(ctx, "two_full", P, d2.TWO_FULL_LINK, 2.0)
    assert ctx.patch_stats()[0] == len(want[2]) > 4 and ctx.patch_stats()[2] >= 2


def test_two_full_as_two_structures_overflows_in_two_workgroups(ctx):
    P = d2.TWO_FULL_POINTS
    c = d2.two_full_batch()
    got, _ = _patches(ctx, "two_full_batch", P, d2.TWO_FULL_LINK, np.inf)
    assert got[1].tolist() == [0, 1, 2] and got[2].tolist() == [0, 0]
    assert ctx.patch_stats()[0] == 2 and ctx.patch_stats()[2] == 2
    for s in range(2):
        one = ctx.dot_patches(*c.part(s), c.probe, P, np.inf, None, d2.TWO_FULL_LINK)
        assert ctx.patch_stats()[0] == 1 and ctx.patch_stats()[2] == 1
        assert np.array_equal(one[2], got[2][s:s + 1]) and one[3].tobytes() == got[3][s:s + 1].tobytes()
        assert one[4].tobytes() == got[4][s * P:(s + 1) * P].tobytes() and np.array_equal(one[5], got[5][s * P:(s + 1) * P])


# ---- C3: more structures than two workgroups a CU ---------------------------------------------------------------------------------

def test_rows_batch_lists_and_geodesics(ctx):
    c = d2.rows_batch()
    lists = _own_lists("rows_batch", 1, 1.0)
    _check_lists(ctx, c, 1, d2.ROW_LINK, lists)
    seeds = d2.last_seeds(lists[0], c.so)
    want = gm.geodesics_batch(*c.cols, c.so, c.probe, 1, d2.ROW_LINK, seeds, lists=lists)
    got = ctx.dot_geodesics_batch(*c.cols, c.so, c.probe, 1, seeds, None, d2.ROW_LINK, True)
    tgg._check_geo(got, want)
    assert 1 <= ctx.geodesic_rounds()[0] <= d2.ROW_MAX and 1 <= ctx.geodesic_rounds()[1] <= d2.ROW_MAX


@pytest.mark.parametrize("run", range(len(d2.ROWS_RUNS)))
def test_rows_batch_patches_of_600_workgroups(ctx, run):
    (spacing, max_centres), K = d2.ROWS_RUNS[run], d2.ROWS_CENTRES[run]
    got, want = _patches(ctx, "rows_batch", 1, d2.ROW_LINK, spacing, max_centres)
    assert len(want[2]) == K and ctx.patch_stats()[0] == K and ctx.patch_stats()[2] == 0
    assert np.array_equal(np.diff(got[1].astype(np.int64)), np.diff(want[1].astype(np.int64))) and int(got[1][-1]) == K


def test_rows_batch_sizing_of_the_bound(ctx):
    """The first of the two calls, as test_gpu_patches.py's sizing test makes it: the bound of max_centres = 2 over 600
    structures, 32 of them empty and 32 of one dot."""
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    lib = _capi.load()
    c = d2.rows_batch()
    x, y, z, r, ids = c.cols
    S = len(c.so) - 1
    per = np.diff(c.so.astype(np.int64))
    cols = (ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(c.so), S, 1.0, 1)
    off, bound = np.zeros(c.n_atoms + 1, np.uint64), np.full(1, 77, np.uint64)
    for max_centres, want in ((2, int(np.minimum(per, 2).sum())), (1, int((per > 0).sum())), (0xFFFFFFFF, c.n_atoms)):
        rc = lib.rsasa_dot_patches_batch(ctx._h, *cols, 1.0, 0.0, max_centres, ptr(off), ptr(bound), None, None, None, 0,
                                         None, None, 0, None, None)
        assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL and bound[0] == want and ctx.patch_stats() == (0, 0, 0)
        assert np.array_equal(off, np.arange(c.n_atoms + 1, dtype=np.uint64))
    assert int(np.minimum(per, 2).sum()) == d2.ROWS_CENTRES[3]
