"""The second pass over the radial counts on the GPU - k_sort_kinds, k_radial_counts, k_radial_pairs (radial.hip) - on the
cases of radial_edge_cases.py, pinned by test_radial_edges_cpu.py: the thin, long, slanted and crowded grids and the
structures one coordinate ulp on either side of the margins' limit (cutoff_edge_cases.py) with each cutoff at which the
stop rule holds with equality as the last edge; an exact tie on every edge at every n_bins from 1 to 32, repeated edges
and squares that overflow into the bin search's padding; structure boundaries and empty structures on the pair kernel's
chunk edges at rows of 1 to 512 cells; and eight threads on one context over radial counts, contact owners, half-sphere
exposure and contact counts.  Tables and pair tables are compared with the exact model (radial_model.py) cell for cell;
the half-sphere exposure of the same context is a second witness that does not share the model.  No tolerances."""
import functools
import threading

import numpy as np
import pytest

import cutoff_edge_cases as ce
import hse_cases as hc
import hse_model as hm
import nb_helpers as nh
import owners_model as om
import point_edge_cases as pe
import radial_cases as rc
import radial_edge_cases as re_
import radial_model as rm
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

F = np.float32
NC = re_.N_CLASSES


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


def _run(ctx, c, edges, classes, n_classes, flags, pairs=True):
    return ctx.radial_counts_batch(c.x, c.y, c.z, c.r, None, c.so, c.probe, edges, classes, n_classes, flags, pairs)


def _equal(got, want, what=None):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), [int(got[tuple(b)]) for b in bad[:5]],
                           [int(want[tuple(b)]) for b in bad[:5]])


def _contact(ctx, c, cutoff, flags):
    up, down = ctx.half_sphere_exposure_batch(c.x, c.y, c.z, c.r, None, c.so, c.probe, None, flags, cutoff)
    assert not down.any()
    return up.astype(np.int64)


def _table_pairs_and_witness(ctx, c, cl, edges, flags, what):
    """Table and pair tables against the model; the cumulative sums over bins and classes against up + down of
    half_sphere_exposure at every edge."""
    want = rm.counts_batch(c.x, c.y, c.z, c.so, edges, cl, NC, flags)
    got, pairs = _run(ctx, c, edges, cl, NC, flags)
    _equal(got, want, what)
    _equal(pairs, rm.pairs_from_counts(want, c.so, cl), what)
    cum = np.cumsum(got.astype(np.int64), axis=2).sum(axis=1)
    for k, cutoff in enumerate(edges):
        assert np.array_equal(cum[:, k], _contact(ctx, c, cutoff, flags)), (what, k, cutoff)
    return got


# ---- A: awkward grids and the margin structures ---------------------------------------------------------------------------------

@pytest.mark.parametrize("fk", [None, "eighth"])
@pytest.mark.parametrize("name", ce.GRID_NAMES + ce.MARGIN_NAMES)
def test_radial_counts_on_the_sweep_cases(ctx, name, fk):
    c = ce.swept(name)
    cl = re_.swept_classes(name)
    flags = re_.flags_of(c, fk)
    lists = re_.swept_edge_lists(name)
    assert len(lists) == 5                                              # every structure is under 1 000 atoms: a covering edge
    for edges in lists:
        got = _table_pairs_and_witness(ctx, c, cl, edges, flags, (name, fk, edges))
    sizes = np.diff(c.so.astype(np.int64))
    centre = np.ones(c.n_atoms, bool) if flags is None else (flags & 2) != 0
    assert np.array_equal(got.sum(axis=(1, 2)), np.where(centre, np.repeat(sizes, sizes) - 1, 0))   # the covering edge


# ---- B: exact ties in the last swept shell, at the margins' edge ---------------------------------------------------------------------

def _edge_case(ctx, c, seed, what):
    cl = re_.grid_classes(c, seed)
    for fk in (None, "eighth"):
        for edges in re_.EDGE_LISTS:
            _table_pairs_and_witness(ctx, c, cl, edges, re_.flags_of(c, fk), (what, fk, edges))
    return cl


@pytest.mark.parametrize("axis,sign", ce.DIRECTIONS)
def test_edge_at_margin(ctx, axis, sign):
    for which in ce.WHICH:
        c = ce.edge_at_margin(axis, sign, which)
        cl = _edge_case(ctx, c, 760, (axis, sign, which))
        got = _run(ctx, c, re_.EDGE_LISTS[0], cl, NC, None, pairs=False)
        for cen in (c.info["hi"], c.info["lo"]):                        # the six ties at d2 == c2, three of them in shell 3
            assert got[cen, :, 1].sum() == 6 and got[cen, :, 0].sum() == 0
            ties = [a for a, _, _ in c.info["tie"][cen]]
            assert np.array_equal(got[cen, :, 1], np.bincount(cl[ties], minlength=NC))


def test_edge_under_and_over_interleaved_in_one_batch(ctx):
    c = ce.edge_twelve()
    cl = _edge_case(ctx, c, 761, "twelve")
    got, pairs = _run(ctx, c, re_.EDGE_LISTS[1], cl, NC, None)
    for s in range(len(c.so) - 1):
        b, e = int(c.so[s]), int(c.so[s + 1])
        one, one_pairs = _run(ctx, hc.part(c, s), re_.EDGE_LISTS[1], cl[b:e], NC, None)
        _equal(one, got[b:e], s)
        _equal(one_pairs, pairs[s:s + 1], s)


# ---- C: the bin search ----------------------------------------------------------------------------------------------------------------

def _ladder(ctx, edges):
    cl = re_.ladder_classes()
    for moved in (False, True):
        c = re_.ladder(moved)
        got = _run(ctx, c, edges, cl, NC, c.flags, pairs=False)
        _equal(got, rm.counts(c.x, c.y, c.z, edges, cl, NC, c.flags), (edges, moved))
        _equal(got[0], re_.ladder_row(edges, moved), (edges, moved, "row"))
        assert not got[1:].any()
        _equal(_run(ctx, c, edges, cl, NC, None, pairs=False), rm.counts(c.x, c.y, c.z, edges, cl, NC, None), (edges, moved, None))


@pytest.mark.parametrize("n_bins", range(1, 33))
def test_an_exact_tie_on_every_edge(ctx, n_bins):
    _ladder(ctx, re_.ladder_edges(n_bins))


@pytest.mark.parametrize("n_bins", re_.REPEAT_BINS)
def test_the_first_of_equal_edges_takes_the_tie(ctx, n_bins):
    _ladder(ctx, re_.ladder_edges(n_bins, repeated=True))


def test_squares_that_overflow_meet_the_padding(ctx):
    c = hc.cluster()
    cl = rc.case_classes("cluster")
    for flags in (None, ce.one_in_eight(c.n_atoms)):
        want = rm.counts(c.x, c.y, c.z, re_.OVERFLOW_EDGES, cl, NC, flags)
        got, pairs = _run(ctx, c, re_.OVERFLOW_EDGES, cl, NC, flags)
        _equal(got, want)
        _equal(pairs, rm.pairs_from_counts(want, c.so, cl))
        assert not got[:, :, 2:].any() and got[:, :, 1].any()
    assert np.all(got.sum(axis=(1, 2)) == np.where((flags & 2) != 0, c.n_atoms - 1, 0))
    for edges in ((1e20,), (1e19, 1e20, 2e20, 3e20, float(np.finfo(F).max))):       # +inf alone; three +inf behind one edge
        _equal(_run(ctx, c, edges, cl, NC, None, pairs=False), rm.counts(c.x, c.y, c.z, edges, cl, NC, None), edges)


# ---- D: the pair kernel ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,extra", [("edges", False), ("edges", True), ("span", False), ("span", True)])
@pytest.mark.parametrize("n_classes,n_bins", re_.PAIR_SHAPES)
def test_structures_on_the_chunk_edges_of_the_pair_kernel(ctx, n_classes, n_bins, layout, extra):
    c = re_.chunk_batch(extra, layout)
    cl = re_.chunk_classes(c.n_atoms, n_classes)
    edges = re_.chunk_edges(n_bins)
    sizes = np.diff(c.so.astype(np.int64))
    want = rm.counts_batch(c.x, c.y, c.z, c.so, edges, cl, n_classes, None)
    want_pairs = rm.pairs_from_counts(want, c.so, cl)
    got, pairs = _run(ctx, c, edges, cl, n_classes, None)
    _equal(got, want)
    _equal(pairs, want_pairs)
    assert pairs.shape == (len(sizes), n_classes, n_classes, n_bins)
    assert not pairs[sizes == 0].any() and pairs[sizes > 1].any(axis=(1, 2, 3)).all() and int((sizes == 0).sum()) == 5
    _equal(_run(ctx, c, edges, cl, n_classes, None, pairs="only"), want_pairs)
    flags = re_.chunk_flags(c.n_atoms)
    want = rm.counts_batch(c.x, c.y, c.z, c.so, edges, cl, n_classes, flags)
    got_f, pairs_f = _run(ctx, c, edges, cl, n_classes, flags)
    _equal(got_f, want)
    _equal(pairs_f, rm.pairs_from_counts(want, c.so, cl))
    _equal(_run(ctx, c, edges, cl, n_classes, flags, pairs="only"), pairs_f)
    for s in np.flatnonzero(sizes):                                     # every non-empty structure alone: the same table
        b, e = int(c.so[s]), int(c.so[s + 1])
        _equal(_run(ctx, hc.part(c, s), edges, cl[b:e], n_classes, None, pairs="only"), pairs[s:s + 1], s)


# ---- E: threads ------------------------------------------------------------------------------------------------------------------------------

JOIN_SECONDS = 120.0


def _single(c):
    return len(c.so) == 2


def _thread_call(ctx, call, name):
    """The call on the input as a tuple of arrays (the batch forms where the input is a batch)."""
    c = re_.thread_case(name)
    if call == "radial":
        return _run(ctx, c, rc.EDGES, rc.case_classes(name) if name != "1jcd" else re_.grid_classes(c, 770), NC, None)
    if call == "hse":
        if _single(c):
            return ctx.half_sphere_exposure(*c.cols, c.probe, c.dirs, None, 13.0)
        return ctx.half_sphere_exposure_batch(*c.cols, c.so, c.probe, c.dirs, None, 13.0)
    if call == "owners":
        if _single(c):
            return ctx.contact_owners(*c.cols, c.probe, re_.THREAD_POINTS, points=True)
        return ctx.contact_owners_batch(*c.cols, c.so, c.probe, re_.THREAD_POINTS, points=True)
    assert call == "contacts"
    if _single(c):
        return ctx.contact_points(*c.cols, c.probe, re_.THREAD_POINTS)
    return ctx.contact_points_batch(*c.cols, c.so, c.probe, re_.THREAD_POINTS)


@functools.lru_cache(maxsize=None)
def _thread_wants():
    """{(call, input): the tuple of arrays from the models and the oracle}, computed once before any thread starts."""
    out = {}
    for name in ce.THREAD_INPUTS:
        c = re_.thread_case(name)
        cl = rc.case_classes(name) if name != "1jcd" else re_.grid_classes(c, 770)
        table = rm.counts_batch(c.x, c.y, c.z, c.so, rc.EDGES, cl, NC, None)
        out[("radial", name)] = (table, rm.pairs_from_counts(table, c.so, cl))
        out[("hse", name)] = hm.counts_batch(c.x, c.y, c.z, c.so, c.dirs, None, 13.0)
        offs, ent = nh.oracle_batch_csr(*c.cols, c.so, c.probe)
        sasa = po.calculate_sasa_batch(*c.cols, c.so, c.probe, re_.THREAD_POINTS, 8, threads=0)
        owned, owner = om.owners_batch(*c.cols, c.so, c.probe, re_.THREAD_POINTS, 8)
        out[("owners", name)] = (offs, ent, owned, sasa, owner)
        _, cov, exc = pe.batch_models(*c.cols, c.so, c.probe, re_.THREAD_POINTS, 8)
        out[("contacts", name)] = (offs, ent, cov, exc, sasa)
    return out


def _same(got, want):
    return len(got) == len(want) and all(np.asarray(g).dtype == np.asarray(w).dtype and g.shape == w.shape
                                         and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def test_threads_on_radial_owners_hse_and_contacts_share_one_context(ctx):
    """Eight threads on one context, ten rounds each, rotating over the four calls and the three inputs; every result
    against its model.  One process, no churn of contexts."""
    wants = _thread_wants()
    for key, want in wants.items():                                     # single-threaded first: the models hold
        assert _same(_thread_call(ctx, *key), want), key
    errors = []

    def work(tid):
        try:
            for it in range(re_.THREAD_ROUNDS):
                name = ce.thread_input(tid, it)
                for call in re_.thread_calls(tid, it):
                    if not _same(_thread_call(ctx, call, name), wants[(call, name)]):
                        errors.append((tid, it, call, name, "differs"))
        except Exception as e:  # noqa: BLE001
            errors.append((tid, repr(e)))

    threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(re_.THREADS)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_SECONDS)
    assert not [n for n, t in enumerate(threads) if t.is_alive()], "threads still running"
    assert errors == []
