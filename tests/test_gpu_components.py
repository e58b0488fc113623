"""Surface components on the GPU (rsasa_surface_components*, components.hip) against the exact CPU model
(components_model.py: the header's definition in numpy float32 on the masks of points_model.py, components by scipy).
A label is a minimum over a set, so every comparison is array_equal: labels, dot offsets and counts.  The cases
(depth_cases.py, component_cases.py, pinned by test_components_cpu.py) sit on the kernels' own edges: a void under the
surface, exact ties at link 0 and at d2 == link * link, edges between atoms three cells apart in every direction, own
dots in 2 to 15 lane chunks, a reach that covers the whole grid, structures of 0, 1 and 2 atoms, dots of another
structure in the middle of a ball, and the 32-bit cell starts of a structure of 65 536 atoms."""
import functools

import numpy as np
import pytest

import bench_workloads as bw
import component_cases as cc
import components_model as cm
import depth_cases as dc
import point_edge_cases as pe
import points_model as pm

pytestmark = pytest.mark.gpu

F = np.float32
CORNER_POINTS = (1, 63, 64, 65, 100, 128, 129)


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


def _link(c, n_points):
    return cc.default_link(c.r, c.probe, n_points)


@functools.lru_cache(maxsize=None)
def _model(name, n_points=100, link=None):
    c = cc.get(name)
    return cm.components_batch(*c.cols, c.so, c.probe, n_points, _link(c, n_points) if link is None else link)


def _check(got, want, r, probe, n_points):
    off, labels, free, sasa = got
    w_off, w_labels, mask = want
    n = len(mask)
    assert off.dtype == np.uint64 and labels.dtype == np.uint32 and free.dtype == np.uint32 and sasa.dtype == F
    assert off.shape == (n + 1,) and free.shape == sasa.shape == (n,)
    assert np.array_equal(off, w_off)
    assert np.array_equal(free, mask.sum(axis=1).astype(np.uint32))
    assert np.array_equal(labels, w_labels), np.flatnonzero(labels != w_labels)[:8]
    assert sasa.tobytes() == pm.sasa_of(r, probe, free, n_points).tobytes()


def _run(ctx, c, n_points=100, link=None):
    return ctx.surface_components_batch(*c.cols, c.so, c.probe, n_points, link)


# ---- 1: every case against the model ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ball", "cavity", "corner", "tiny", "overlap_batch"])
def test_cases_equal_the_model(ctx, name):
    c = cc.get(name)
    got = _run(ctx, c)
    _check(got, _model(name), c.r, c.probe, 100)
    # consistency with the other point calls
    words, sasa = ctx.accessible_points_batch(*c.cols, c.so, c.probe, 100)
    assert np.array_equal(got[2].astype(np.int64), pe.popcount(words)) and got[3].tobytes() == sasa.tobytes()
    assert np.array_equal(got[0], np.concatenate([[0], np.cumsum(got[2].astype(np.uint64))]).astype(np.uint64))
    # the same call twice: the labels do not depend on the schedule
    again = _run(ctx, c)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_overlap_batch_links_nothing_across_structures(ctx):
    o, b = cc.get("overlap_batch"), cc.get("ball")
    off, labels, free, _ = _run(ctx, o)
    alone = ctx.surface_components(*b.cols, b.probe, 100)
    lone = int(off[-2])
    assert free[-1] == 100 and len(labels) == lone + 100
    assert np.array_equal(labels[:lone], alone[1]) and np.array_equal(off[:-1], alone[0])
    assert not labels[lone:].any()                              # the lone atom's dots: one component, number 0 of its own


def test_cavity_at_960_points(ctx):
    c = cc.get("cavity")
    _check(_run(ctx, c, 960), _model("cavity", 960), c.r, c.probe, 960)


@pytest.mark.parametrize("n_points", CORNER_POINTS)
def test_point_counts_on_corner(ctx, n_points):
    c = cc.get("corner")
    _check(_run(ctx, c, n_points), _model("corner", n_points), c.r, c.probe, n_points)


def test_corner_with_a_reach_over_the_whole_grid_and_with_none(ctx):
    c = cc.get("corner")
    wide = F(3.0) * cc.H
    got = _run(ctx, c, 100, wide)
    _check(got, _model("corner", 100, wide), c.r, c.probe, 100)
    assert not got[1].any()                                     # one component
    got = _run(ctx, c, 100, F(1e-3))
    _check(got, _model("corner", 100, F(1e-3)), c.r, c.probe, 100)
    assert np.array_equal(got[1], np.arange(len(got[1])))       # every dot alone


def test_twins_at_link_zero(ctx):
    c = cc.get("twins")
    got = _run(ctx, c, 100, 0.0)
    _check(got, _model("twins", 100, 0.0), c.r, c.probe, 100)
    assert len(got[1]) == 268 and len(np.unique(got[1])) == 178


def test_pole_tie_on_both_sides_of_the_tie(ctx):
    c = cc.get("pole_tie")
    below = np.nextafter(F(3.0), F(0.0))
    assert np.array_equal(_run(ctx, c, 1, F(3.0))[1], [0, 0])
    assert np.array_equal(_run(ctx, c, 1, below)[1], [0, 1])
    _check(_run(ctx, c, 1, F(3.0)), _model("pole_tie", 1, F(3.0)), c.r, c.probe, 1)
    _check(_run(ctx, c, 1, below), _model("pole_tie", 1, below), c.r, c.probe, 1)


def test_far_link_in_six_directions_and_both_orders(ctx):
    c = cc.get("far_link")
    got = _run(ctx, c, cc.FAR_POINTS, cc.H)
    _check(got, _model("far_link", cc.FAR_POINTS, cc.H), c.r, c.probe, cc.FAR_POINTS)
    assert not got[1].any()                                     # every pair is one component


@pytest.mark.parametrize("n_points", cc.CHUNK_POINTS)
def test_multi_chunk(ctx, n_points):
    c = cc.get("multi_chunk")
    _check(_run(ctx, c, n_points), _model("multi_chunk", n_points), c.r, c.probe, n_points)


def test_tail_structure(ctx):
    """32-bit cell starts behind three small structures.  The masks of 65 536 atoms take the point model minutes, so
    they are the engine's own (accessible_points_batch, pinned to the oracle at this size by test_gpu_tail_edges.py)."""
    import rustsasa_amd
    c = cc.get("tail")
    words, _ = ctx.accessible_points_batch(*c.cols, c.so, c.probe, 100)
    mask = rustsasa_amd.unpack_points(words, 100).astype(bool)
    link = _link(c, 100)
    want = cm.components_batch(*c.cols, c.so, c.probe, 100, link, mask=mask)
    _check(_run(ctx, c), want, c.r, c.probe, 100)


# ---- 2: non-finite input, argument errors, sizing ----------------------------------------------------------------------

def test_nan_atoms_are_singletons_and_inf_is_refused(ctx):
    import rustsasa_amd
    c = cc.get("corner")
    x, y, z, r, ids = c.cols
    xn, rn = x.copy(), r.copy()
    xn[5] = np.nan
    rn[17] = np.nan
    link = _link(c, 100)
    mask = pm.exposed_masks(xn, y, z, rn, ids, 1.4, 100, 8)
    assert mask[5].all() and mask[17].all()
    want = cm.components(xn, y, z, rn, ids, 1.4, 100, link, mask=mask)
    got = ctx.surface_components(xn, y, z, rn, ids, 1.4, 100, link)
    _check(got, want, rn, 1.4, 100)
    off, labels = got[:2]
    for i in (5, 17):
        b, e = int(off[i]), int(off[i + 1])
        assert e - b == 100 and np.array_equal(labels[b:e], np.arange(b, e))
    bad = x.copy()
    bad[3] = np.inf
    for call in (lambda: ctx.surface_components(bad, y, z, r, ids, 1.4, 100),
                 lambda: ctx.surface_components_batch(bad, y, z, r, ids, c.so, 1.4, 100)):
        with pytest.raises(rustsasa_amd.RsasaError) as e:
            call()
        assert e.value.status == -5
    _check(_run(ctx, c), _model("corner"), c.r, c.probe, 100)


def test_argument_errors_and_sizing_from_the_library(ctx):
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    lib = _capi.load()
    c = cc.get("corner")
    x, y, z, r, ids = c.cols
    n = c.n_atoms
    w_off, w_labels, _ = _model("corner")
    total = len(w_labels)
    link = float(_link(c, 100))
    off, labels = np.zeros(n + 1, np.uint64), np.full(total, 0xABCDEF01, np.uint32)
    cols = (ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids))
    so = np.array([0, n], np.uint32)
    bad, small = _capi.RSASA_ERR_INVALID_ARGUMENT, _capi.RSASA_ERR_BUFFER_TOO_SMALL
    one = lambda *a: lib.rsasa_surface_components(ctx._h, *a)            # noqa: E731
    many = lambda *a: lib.rsasa_surface_components_batch(ctx._h, *a)     # noqa: E731
    for v in (float("nan"), -1.0, float("inf")):
        assert one(*cols, n, 1.4, 100, v, ptr(off), ptr(labels), total, None, None) == bad
        assert many(*cols, ptr(so), 1, 1.4, 100, v, ptr(off), ptr(labels), total, None, None) == bad
    assert one(ptr(x), None, ptr(z), ptr(r), ptr(ids), n, 1.4, 100, link, ptr(off), ptr(labels), total, None, None) == bad
    assert one(*cols, n, 1.4, 100, link, None, ptr(labels), total, None, None) == bad
    assert one(*cols, n, 1.4, 0, link, ptr(off), ptr(labels), total, None, None) == bad
    assert many(*cols, None, 1, 1.4, 100, link, ptr(off), ptr(labels), total, None, None) == bad
    assert many(ptr(x), ptr(y), ptr(z), None, ptr(ids), ptr(so), 1, 1.4, 100, link, ptr(off), ptr(labels), total, None, None) == bad
    assert not off.any() and (labels == 0xABCDEF01).all()       # nothing was written
    # sizing: the offsets are written, the labels are not
    assert one(*cols, n, 1.4, 100, link, ptr(off), ptr(labels), total - 1, None, None) == small
    assert np.array_equal(off, w_off) and (labels == 0xABCDEF01).all()
    off[:] = 0
    assert many(*cols, ptr(so), 1, 1.4, 100, link, ptr(off), None, total, None, None) == small
    assert np.array_equal(off, w_off)
    # no atoms is OK; out_free and out_sasa are optional; the context is still usable
    off[:] = 7
    assert one(*cols, 0, 1.4, 100, link, ptr(off), None, 0, None, None) == _capi.RSASA_OK and off[0] == 0
    assert one(*cols, n, 1.4, 100, link, ptr(off), ptr(labels), total, None, None) == _capi.RSASA_OK
    assert np.array_equal(off, w_off) and np.array_equal(labels, w_labels)


# ---- 3: single and batch; one context, other families, a batch in flight -----------------------------------------------

def test_single_call_equals_batch_call(ctx):
    for name in ("cavity", "twins", "corner"):
        c = cc.get(name)
        one = ctx.surface_components(*c.cols, c.probe, 100)
        many = ctx.surface_components_batch(*c.cols, c.so, c.probe, 100)
        for k in range(4):
            assert one[k].tobytes() == many[k].tobytes(), (name, k)
    e = np.zeros(0, F)
    for so in ([0], [0, 0, 0]):
        got = ctx.surface_components_batch(e, e, e, e, np.zeros(0, np.uint64), np.array(so, np.uint32), 1.4, 100)
        assert got[0].tolist() == [0] and all(len(a) == 0 for a in got[1:])
    got = ctx.surface_components(e, e, e, e, None, 1.4, 100)
    assert got[0].tolist() == [0] and all(len(a) == 0 for a in got[1:])


def test_between_the_other_families_and_beside_a_batch_in_flight(ctx):
    torch = pytest.importorskip("torch")
    c, t = cc.get("cavity"), cc.get("twins")
    want = _model("cavity")
    b = bw.synthetic_proteome(12, seed=4)
    dev = torch.device("cuda", 0)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cols = (tt(b.x), tt(b.y), tt(b.z), tt(b.radius), tt(b.ids.view(np.int64)))
    alone = torch.zeros(b.n_atoms, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.enqueue_device(*cols, b.structure_offsets, out_atom_sasa=alone, probe_radius=1.4, n_points=100)
    ctx.wait()
    words0, _ = ctx.accessible_points(*c.cols, c.probe, 100)
    dp0 = ctx.atom_depth(*t.cols, t.probe, 129)
    out = torch.zeros(b.n_atoms, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.enqueue_device(*cols, b.structure_offsets, out_atom_sasa=out, probe_radius=1.4, n_points=100)
    got = ctx.surface_components(*c.cols, c.probe, 100)
    ctx.wait()
    assert out.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    _check(got, want, c.r, c.probe, 100)
    # the other families through the same buffers, before and after
    nb = ctx.precompute_neighbors(*c.cols, c.probe)
    dp1 = ctx.atom_depth(*t.cols, t.probe, 129)
    words1, _ = ctx.accessible_points(*c.cols, c.probe, 100)
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(dp0, dp1)) and words0.tobytes() == words1.tobytes()
    assert len(nb[0]) == c.n_atoms + 1
    _check(ctx.surface_components(*c.cols, c.probe, 100), want, c.r, c.probe, 100)
