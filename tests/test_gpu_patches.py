"""Dot patches on the GPU (rsasa_dot_patches*, patches.hip) against the exact CPU model (patches_model.py: the header's
definition on geodesics_model.py - a float32 argmax with ties to the smallest dot, a Dijkstra from scratch from all
centres so far, the sources at the end).  The kernel relaxes incrementally from the previous pick; its fixed point is
the least solution for the larger seed set, so every comparison is for equality, byte for byte.  The cases
(patches_cases.py, geodesics_cases.py; pinned by test_patches_cpu.py) sit on the sampler's own edges: its workgroup
width, its queue's capacity, ties in the argmax, structures that end at different picks."""
import functools
import threading

import numpy as np
import pytest

import bench_workloads as bw
import component_cases as cc
import geodesics_model as gm
import patches_cases as pc
import patches_model as pmod
import points_model as pm

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


def _link(c, n_points, link=None):
    return cc.default_link(c.r, c.probe, n_points) if link is None else F(link)


@functools.lru_cache(maxsize=None)
def _lists(name, n_points=100, link=None, W=8):
    c = pc.get(name)
    return gm.links_batch(*c.cols, c.so, c.probe, n_points, _link(c, n_points, link), W)


@functools.lru_cache(maxsize=None)
def _want(name, n_points=100, spacing=6.0, max_centres=None, link=None, W=8):
    c = pc.get(name)
    return pmod.patches_batch(*c.cols, c.so, c.probe, n_points, _link(c, n_points, link), spacing, max_centres,
                              lists=_lists(name, n_points, link, W))


def _run(ctx, c, n_points=100, spacing=6.0, max_centres=None, link=None):
    return ctx.dot_patches_batch(*c.cols, c.so, c.probe, n_points, spacing, max_centres, link, True)


def _check(got, want, c, n_points):
    off, c_off, centres, cover, dist, source, free, sasa = got
    w_off, w_coff, w_centres, w_cover, w_dist, w_src, mask = want
    assert off.dtype == c_off.dtype == np.uint64 and centres.dtype == source.dtype == free.dtype == np.uint32
    assert cover.dtype == dist.dtype == sasa.dtype == F
    assert np.array_equal(off, w_off) and np.array_equal(free, mask.sum(axis=1))
    assert np.array_equal(c_off, w_coff), (c_off, w_coff)
    assert np.array_equal(centres, w_centres), np.flatnonzero(centres != w_centres)[:8]
    assert cover.tobytes() == w_cover.tobytes()
    assert dist.tobytes() == w_dist.tobytes(), np.flatnonzero(dist.view(np.uint32) != w_dist.view(np.uint32))[:8]
    assert np.array_equal(source, w_src), np.flatnonzero(source != w_src)[:8]
    assert sasa.tobytes() == pm.sasa_of(c.r, c.probe, free, n_points).tobytes()


def _same(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 1: byte for byte against the model -------------------------------------------------------------------------------

def test_the_ladder_by_hand(ctx):
    c = pc.get("ladder")
    got = _run(ctx, c, 1, 0.0, None, 1.0)
    assert got[0].tolist() == [0, 1, 2, 3, 4, 5] and got[1].tolist() == [0, 5]
    assert got[2].tolist() == [0, 4, 2, 1, 3] and got[3].tolist() == [np.inf, 4.0, 2.0, 1.0, 1.0]
    assert not got[4].any() and got[5].tolist() == [0, 1, 2, 3, 4]
    _check(got, _want("ladder", 1, 0.0, None, 1.0), c, 1)
    got = _run(ctx, c, 1, 1.0, None, 1.0)
    assert got[2].tolist() == [0, 4, 2] and got[4].tolist() == [0.0, 1.0, 0.0, 1.0, 0.0] and got[5].tolist() == [0, 0, 2, 2, 4]
    _check(got, _want("ladder", 1, 1.0, None, 1.0), c, 1)
    assert ctx.patch_stats()[0] == 3


@pytest.mark.parametrize("name,n_points,spacing,max_centres", [
    ("cavity", 100, 8.0, None), ("cavity", 100, np.inf, None), ("twins", 100, 0.0, None), ("twins", 960, 3.0, None),
    ("corner", 100, 0.0, 40), ("corner", 100, 3.0, None), ("corner", 100, 6.0, None), ("corner", 100, np.inf, None),
    ("corner", 100, 3.0, 1), ("corner", 100, 3.0, 2), ("corner", 100, 3.0, 7), ("tiny", 100, 1.5, None),
    ("tiny", 100, 0.0, 7), ("dot_counts", pc.gc.COUNT_POINTS, 3.0, None), ("chain", 100, np.inf, None),
    ("chain", 100, 60.0, None), ("jcd", 100, 12.0, None), ("example_vdw", 100, 12.0, 7), ("overlap_batch", 100, 6.0, None)])
def test_patches_equal_the_model(ctx, name, n_points, spacing, max_centres):
    c = pc.get(name)
    got = _run(ctx, c, n_points, spacing, max_centres)
    want = _want(name, n_points, spacing, max_centres)
    _check(got, want, c, n_points)
    picks, steps, _ = ctx.patch_stats()
    assert picks == int(got[1][-1]) == len(got[2]) and steps >= picks
    if name == "cavity" and spacing == 8.0:
        assert len(got[2]) == 32 and np.isinf(got[3][:2]).all() and np.isfinite(got[3][2:]).all()
    if name == "chain" and np.isinf(spacing):
        assert len(got[2]) == 1 and 200 <= steps <= len(got[4]) + 1       # one pick of more than 200 steps


def test_jcd_at_six_angstrom(ctx):
    c = pc.get("jcd")
    got = _run(ctx, c, 100, 6.0)
    _check(got, _want("jcd", 100, 6.0), c, 100)
    assert len(got[2]) == 148 and (got[4] <= F(6.0)).all()


@pytest.mark.parametrize("n_points", pc.LONE_POINTS)
def test_a_lone_atom_of_exactly_n_dots(ctx, n_points):
    """D = n_points: one dot, a wave, a workgroup's stride and the queue's capacity, each less and more."""
    c = pc.get("lone")
    for spacing, max_centres in ((3.0, None), (0.0, 3)):
        got = _run(ctx, c, n_points, spacing, max_centres)
        assert int(got[0][-1]) == n_points
        _check(got, _want("lone", n_points, spacing, max_centres), c, n_points)


@pytest.mark.parametrize("n_points", pc.FULL_POINTS)
def test_a_first_pick_that_lowers_every_other_dot_in_one_step(ctx, n_points):
    """Every dot is linked to every other: the first pick lowers n_points - 1 dots in one step.  Up to the queue's capacity
    they are queued; one more and the pick finishes on the stamp scan, which patch_stats counts."""
    c = pc.get("lone")
    got = _run(ctx, c, n_points, np.inf, None, pc.FULL_LINK)
    _check(got, _want("lone", n_points, np.inf, None, pc.FULL_LINK), c, n_points)
    assert len(got[2]) == 1 and ctx.patch_stats()[0] == 1
    assert ctx.patch_stats()[2] == (1 if n_points - 1 > pc.PS_QUEUE else 0)
    got = _run(ctx, c, n_points, 2.0, None, pc.FULL_LINK)
    _check(got, _want("lone", n_points, 2.0, None, pc.FULL_LINK), c, n_points)
    assert len(got[2]) > 3 and (ctx.patch_stats()[2] > 0) == (n_points - 1 > pc.PS_QUEUE)


@pytest.mark.parametrize("W", [1, 16])
def test_lane_counts(W):
    import rustsasa_amd
    c = pc.get("corner")
    with rustsasa_amd.Context(0, W) as cx:
        _check(_run(cx, c, 129, 4.0), _want("corner", 129, 4.0, None, None, W), c, 129)


def test_single_call_equals_batch_call_and_empty_batches(ctx):
    for name, spacing, max_centres in (("cavity", 8.0, None), ("twins", 2.0, 5), ("ladder", 6.0, None)):
        c = pc.get(name)
        one = ctx.dot_patches(*c.cols, c.probe, 100, spacing, max_centres)
        assert one[1].tolist() == [0, len(one[2])]
        assert _same(one, _run(ctx, c, 100, spacing, max_centres))
        no_src = ctx.dot_patches(*c.cols, c.probe, 100, spacing, max_centres, None, False)
        assert no_src[5] is None and _same(no_src[:5] + no_src[6:], one[:5] + one[6:])
    e = np.zeros(0, F)
    for so in ([0], [0, 0, 0]):
        got = ctx.dot_patches_batch(e, e, e, e, np.zeros(0, np.uint64), np.array(so, np.uint32), 1.4, 100)
        assert got[0].tolist() == [0] and got[1].tolist() == [0] * len(so) and len(got[2]) == len(got[4]) == 0
        assert ctx.patch_stats() == (0, 0, 0)


# ---- 2: a second witness, independence, identities ---------------------------------------------------------------------

@pytest.mark.parametrize("name,spacing,max_centres", [("cavity", 8.0, None), ("mixed", 6.0, 7), ("corner", 3.0, None)])
def test_the_geodesics_from_the_centres_give_the_same_dist_and_source(ctx, name, spacing, max_centres):
    import rustsasa_amd
    c = pc.get(name)
    off, c_off, centres, _, dist, source, _, _ = _run(ctx, c, 100, spacing, max_centres)
    seeds = rustsasa_amd.dot_seeds_from(c_off, centres, off, c.so)
    assert int(seeds.sum()) == len(centres) > 0
    g = ctx.dot_geodesics_batch(*c.cols, c.so, c.probe, 100, seeds, None, None, True)
    assert g[1].tobytes() == dist.tobytes() and np.array_equal(g[4], source)
    which = rustsasa_amd.patch_index(off, source, c_off, centres, c.so)
    assert ((which >= 0) == np.isfinite(dist)).all() and (max_centres is not None or (which >= 0).all())


def test_structures_of_a_batch_are_sampled_independently(ctx):
    """tiny, the ladder's row, cavity and a lone atom in one batch end at different picks; the batch equals the structures
    run one by one, with a bound that cuts some of them short and with one that cuts none."""
    c = pc.get("mixed")
    D = int(_lists("mixed")[0][-1])
    for max_centres in (7, D):
        got = _run(ctx, c, 100, 6.0, max_centres)
        _check(got, _want("mixed", 100, 6.0, max_centres), c, 100)
        per = np.diff(got[1].astype(np.int64))
        assert len(set(per.tolist())) >= 3 and per[1] == per[3] == 0 and (per <= max_centres).all()
        off = got[0].astype(np.int64)
        for s in range(len(c.so) - 1):
            b, e = int(c.so[s]), int(c.so[s + 1])
            if e == b:
                continue
            one = ctx.dot_patches(*c.part(s), c.probe, 100, 6.0, max_centres, _link(c, 100))
            cb, ce = int(got[1][s]), int(got[1][s + 1])
            db, de = int(off[b]), int(off[e])
            assert np.array_equal(one[2], got[2][cb:ce]) and one[3].tobytes() == got[3][cb:ce].tobytes()
            assert one[4].tobytes() == got[4][db:de].tobytes() and np.array_equal(one[5], got[5][db:de])
    assert (np.diff(_run(ctx, c, 100, 6.0, 7)[1].astype(np.int64)) == 7).any()      # the bound did cut


@pytest.mark.parametrize("name,spacing", [("mixed", 6.0), ("cavity", np.inf), ("dot_counts", 3.0)])
def test_the_first_centres_are_the_component_labels(ctx, name, spacing):
    c = pc.get(name)
    n_points = pc.gc.COUNT_POINTS if name == "dot_counts" else 100
    off, c_off, centres, cover, dist, _, _, _ = _run(ctx, c, n_points, spacing)
    _, labels, _, _ = ctx.surface_components_batch(*c.cols, c.so, c.probe, n_points)
    assert ctx.patch_stats()[0] == int(c_off[-1])
    doff = off.astype(np.int64)
    for s in range(len(c.so) - 1):
        cs, cv = centres[int(c_off[s]):int(c_off[s + 1])], cover[int(c_off[s]):int(c_off[s + 1])]
        lab = np.unique(labels[int(doff[c.so[s]]):int(doff[c.so[s + 1]])])
        first = np.isinf(cv)
        assert np.array_equal(cs[first], lab) and first[:len(lab)].all() and not first[len(lab):].any()
        assert (cv[1:] <= cv[:-1]).all()
    assert (dist <= F(spacing)).all()
    if np.isinf(spacing):
        assert np.array_equal(np.sort(centres), np.unique(labels))


def test_the_dots_of_nan_atoms_are_centres_of_their_own(ctx):
    c = pc.get("corner")
    x, y, z, r, ids = c.cols
    xn, rn = x.copy(), r.copy()
    xn[5] = np.nan
    rn[17] = np.nan
    link = _link(c, 100)
    so = np.array([0, c.n_atoms], np.uint32)
    want = pmod.patches_batch(xn, y, z, rn, ids, so, 1.4, 100, link, 4.0)
    got = ctx.dot_patches(xn, y, z, rn, ids, 1.4, 100, 4.0, None, link)
    off = got[0].astype(np.int64)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and got[3].tobytes() == want[3].tobytes()
    assert got[4].tobytes() == want[4].tobytes() and np.array_equal(got[5], want[5])
    for i in (5, 17):
        mine = np.arange(off[i], off[i + 1])
        assert len(mine) == 100 and np.isin(mine, got[2]).all() and not got[4][mine].any() and np.array_equal(got[5][mine], mine)
        assert np.isinf(got[3][np.isin(got[2], mine)]).all()


# ---- 3: sizing and the argument rules -----------------------------------------------------------------------------------

def test_sizing_in_two_calls_and_argument_rules(ctx):
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    lib = _capi.load()
    c = pc.get("mixed")
    x, y, z, r, ids = c.cols
    n, S = c.n_atoms, len(c.so) - 1
    want = _want("mixed", 100, 6.0, 7)
    w_off = want[0]
    D, K = int(w_off[-1]), len(want[2])
    per = np.diff(w_off.astype(np.int64)[c.so.astype(np.int64)])
    B = int(np.minimum(per, 7).sum())
    assert K < B < D
    link = float(_link(c, 100))
    cols = (ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(c.so), S, 1.4, 100)
    bad, small, ok = _capi.RSASA_ERR_INVALID_ARGUMENT, _capi.RSASA_ERR_BUFFER_TOO_SMALL, _capi.RSASA_OK
    off, bound, c_off = np.zeros(n + 1, np.uint64), np.full(1, 77, np.uint64), np.full(S + 1, 0xAB, np.uint64)
    centres, cover = np.full(B, 0xABCDEF01, np.uint32), np.full(B, 5, F)
    dist, src = np.full(D, 5, F), np.full(D, 0xABCDEF01, np.uint32)
    many = lambda *a: lib.rsasa_dot_patches_batch(ctx._h, *a)     # noqa: E731
    outs = (ptr(off), ptr(bound), ptr(c_off), ptr(centres), ptr(cover), B, ptr(dist), ptr(src), D, None, None)

    def untouched():
        return ((c_off == 0xAB).all() and (centres == 0xABCDEF01).all() and (cover == 5).all() and (dist == 5).all()
                and (src == 0xABCDEF01).all())

    # the argument rules: nothing is written
    for spacing in (float("nan"), -1.0, -float("inf"), -1e-30):
        assert many(*cols, link, spacing, 7, *outs) == bad
    assert many(*cols, link, 6.0, 0, *outs) == bad
    for v in (float("nan"), -1.0, float("inf")):
        assert many(*cols, v, 6.0, 7, *outs) == bad
    assert many(*cols, link, 6.0, 7, None, *outs[1:]) == bad and many(*cols, link, 6.0, 7, ptr(off), None, *outs[2:]) == bad
    assert many(*cols[:5], None, S, 1.4, 100, link, 6.0, 7, *outs) == bad
    assert many(*cols[:8], 0, link, 6.0, 7, *outs) == bad
    assert many(ptr(x), None, *cols[2:], link, 6.0, 7, *outs) == bad
    assert not off.any() and bound[0] == 77 and untouched()
    # sizing: the two totals, and nothing else; no sampling runs
    sizing = [(None, ptr(centres), ptr(cover), B, ptr(dist), ptr(src), D), (ptr(c_off), None, ptr(cover), B, ptr(dist), ptr(src), D),
              (ptr(c_off), ptr(centres), None, B, ptr(dist), ptr(src), D), (ptr(c_off), ptr(centres), ptr(cover), B, None, ptr(src), D),
              (ptr(c_off), ptr(centres), ptr(cover), B - 1, ptr(dist), ptr(src), D),
              (ptr(c_off), ptr(centres), ptr(cover), B, ptr(dist), ptr(src), D - 1), (None, None, None, 0, None, None, 0)]
    for a in sizing:
        off[:], bound[0] = 0, 77
        assert many(*cols, link, 6.0, 7, ptr(off), ptr(bound), *a, None, None) == small
        assert np.array_equal(off, w_off) and bound[0] == B and untouched() and ctx.patch_stats() == (0, 0, 0)
    # the bound follows max_centres, and D always suffices
    for mc, b in ((1, int(np.minimum(per, 1).sum())), (0xFFFFFFFF, D)):
        assert many(*cols, link, 6.0, mc, ptr(off), ptr(bound), None, None, None, 0, None, None, 0, None, None) == small
        assert bound[0] == b
    # the second call; -0.0 is 0 and a source may be left out
    assert many(*cols, link, 6.0, 7, *outs) == ok
    assert np.array_equal(c_off, want[1]) and np.array_equal(centres[:K], want[2]) and cover[:K].tobytes() == want[3].tobytes()
    assert dist.tobytes() == want[4].tobytes() and np.array_equal(src, want[5]) and (centres[K:] == 0xABCDEF01).all()
    assert ctx.patch_stats()[0] == K
    src[:] = 0xABCDEF01
    assert many(*cols, link, 6.0, 7, *outs[:7], None, *outs[8:]) == ok and (src == 0xABCDEF01).all()
    assert dist.tobytes() == want[4].tobytes()
    lad = pc.get("ladder")
    a5 = tuple(ptr(a) for a in lad.cols)
    o5, b5, co5, ce5, cv5, d5 = (np.zeros(6, np.uint64), np.zeros(1, np.uint64), np.zeros(2, np.uint64), np.zeros(5, np.uint32),
                                 np.zeros(5, F), np.zeros(5, F))
    assert lib.rsasa_dot_patches(ctx._h, *a5, 5, 1.0, 1, 1.0, -0.0, 0xFFFFFFFF, ptr(o5), ptr(b5), ptr(co5), ptr(ce5), ptr(cv5), 5,
                                 ptr(d5), None, 5, None, None) == ok
    assert b5[0] == 5 and co5.tolist() == [0, 5] and ce5.tolist() == [0, 4, 2, 1, 3] and not d5.any()
    # no atoms
    off[:], bound[0], c_off[:] = 7, 77, 7
    assert lib.rsasa_dot_patches(ctx._h, *cols[:5], 0, 1.4, 100, link, 6.0, 7, *outs) == ok
    assert off[0] == 0 and bound[0] == 0 and c_off[0] == c_off[1] == 0 and ctx.patch_stats() == (0, 0, 0)
    zero = np.zeros(S + 1, np.uint32)
    c_off[:] = 7
    assert many(*cols[:5], ptr(zero), S, 1.4, 100, link, 6.0, 7, *outs) == ok and not c_off.any() and bound[0] == 0
    assert lib.rsasa_context_patch_stats(ctx._h, None) == bad and lib.rsasa_context_patch_stats(None, None) == bad


def test_a_call_without_dots_after_a_dense_one(ctx):
    """What a dense call left in the workspace is not read by the next: a batch of empty structures, a structure whose
    only atom is buried (no dot) and a sparse batch right behind a dense call return their own results."""
    dense = pc.get("cavity")
    _check(_run(ctx, dense, 100, 8.0), _want("cavity", 100, 8.0), dense, 100)
    assert ctx.patch_stats()[0] == 32
    e = np.zeros(0, F)
    got = ctx.dot_patches_batch(e, e, e, e, np.zeros(0, np.uint64), np.array([0, 0], np.uint32), 1.4, 100)
    assert [len(a) for a in got[2:6]] == [0, 0, 0, 0] and got[1].tolist() == [0, 0] and ctx.patch_stats() == (0, 0, 0)
    # a buried atom has no dot: the structure of the second atom alone gets centres
    c = pc.get("twins")
    x, y, z, r, ids = (a[:2].copy() for a in c.cols)              # atom 0 lies inside atom 1
    so = np.array([0, 1, 2], np.uint32)
    one = ctx.dot_patches_batch(x, y, z, r, ids, np.array([0, 2], np.uint32), 1.4, 100, 3.0)
    assert one[7][0] == 0 and one[6][0] == 0 and len(one[2]) > 1
    two = ctx.dot_patches_batch(x, y, z, r, ids, so, 1.4, 100, 3.0)
    assert int(two[0][1]) == 100 and two[1][1] > 1 and two[1][2] > two[1][1]
    tiny = pc.get("tiny")
    _check(_run(ctx, tiny, 100, 1.5), _want("tiny", 100, 1.5), tiny, 100)


# ---- 4: one context, other families, a batch in flight, threads ----------------------------------------------------------

def test_beside_other_families_and_a_device_batch_in_flight(ctx):
    torch = pytest.importorskip("torch")
    c = pc.get("cavity")
    b = bw.synthetic_proteome(12, seed=4)
    dev = torch.device("cuda", 0)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cols = (tt(b.x), tt(b.y), tt(b.z), tt(b.radius), tt(b.ids.view(np.int64)))
    alone = torch.zeros(b.n_atoms, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.enqueue_device(*cols, b.structure_offsets, out_atom_sasa=alone, probe_radius=1.4, n_points=100)
    ctx.wait()
    out = torch.zeros(b.n_atoms, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.enqueue_device(*cols, b.structure_offsets, out_atom_sasa=out, probe_radius=1.4, n_points=100)
    first = _run(ctx, c, 100, 8.0)
    seeds = pc.gc.one_seed(len(first[4]), 9)
    geo = ctx.dot_geodesics_batch(*c.cols, c.so, c.probe, 100, seeds, 10.0, None, True)
    links = ctx.dot_links_batch(*c.cols, c.so, c.probe, 100)
    comps = ctx.surface_components_batch(*c.cols, c.so, c.probe, 100)
    second = _run(ctx, c, 100, 8.0)
    ctx.wait()
    assert out.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    _check(first, _want("cavity", 100, 8.0), c, 100)
    assert _same(first, second)
    w = gm.geodesics_batch(*c.cols, c.so, c.probe, 100, _link(c, 100), seeds, 10.0, lists=_lists("cavity"))
    assert geo[1].tobytes() == w[1].tobytes() and np.array_equal(geo[4], w[2])
    assert links[2].tobytes() == _lists("cavity")[2].tobytes() and np.array_equal(comps[0], first[0])


def test_eight_threads_on_one_context(ctx):
    jobs = [("corner", 3.0, None), ("tiny", 1.5, None), ("twins", 2.0, 5), ("cavity", 8.0, None)]
    want = [_want(n, 100, s, m) for n, s, m in jobs]
    errors = []

    def work(t):
        try:
            for k in range(4):
                j = (t + k) % len(jobs)
                name, spacing, max_centres = jobs[j]
                c = pc.get(name)
                _check(_run(ctx, c, 100, spacing, max_centres), want[j], c, 100)
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)[:300]))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:4]
