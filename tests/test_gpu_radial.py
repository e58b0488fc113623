"""Radial counts on the GPU (rsasa_radial_counts*, k_sort_kinds / k_radial_counts / k_radial_pairs of radial.hip) against
the exact CPU model (radial_model.py: the header's definition in numpy float32).  The tables are integers with no order,
so every comparison is np.array_equal.  The cases are those of the half-sphere exposure (hse_cases.py: exact ties at the
last edge, sweeps the stop rule ends after 1 .. 5 shells or that cover the grid, tie partners in the last swept shell,
runs of more than 64 atoms, structures that fail the margins, batches down to empty structures and up to 32-bit cell
starts) with seeded classes and edge lists, and what the histogram and the pair tables add (radial_cases.py): rows of 1
to 512 cells, 64 lanes adding to one cell, inner, duplicated, zero and underflowing edges, 300 structures in one
workgroup of the pair kernel, a pair cell above 2^32."""
import functools

import numpy as np
import pytest

import hse_cases as hc
import radial_cases as rc
import radial_model as rm

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _model(name, edges, n_classes=rc.N_CLASSES):
    """The model's table of a case of hse_cases.py with its seeded classes and its own flags (computed once, shared,
    never written to)."""
    c = getattr(hc, name)()
    t = rm.counts_batch(c.x, c.y, c.z, c.so, edges, rc.case_classes(name, n_classes), n_classes, c.flags)
    t.setflags(write=False)
    return t


def _run(ctx, c, edges, classes=None, n_classes=None, flags="own", pairs=False, probe=None, r=None):
    flags = c.flags if isinstance(flags, str) else flags
    probe = c.probe if probe is None else probe
    r = c.r if r is None else r
    if len(c.so) == 2:
        return ctx.radial_counts(c.x, c.y, c.z, r, None, probe, edges, classes, n_classes, flags, pairs)
    return ctx.radial_counts_batch(c.x, c.y, c.z, r, None, c.so, probe, edges, classes, n_classes, flags, pairs)


def _equal(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), [int(got[tuple(b)]) for b in bad[:5]], [int(want[tuple(b)]) for b in bad[:5]])


def _contact(ctx, c, cutoff, flags="own"):
    flags = c.flags if isinstance(flags, str) else flags
    if len(c.so) == 2:
        up, down = ctx.half_sphere_exposure(c.x, c.y, c.z, c.r, None, c.probe, None, flags, cutoff)
    else:
        up, down = ctx.half_sphere_exposure_batch(c.x, c.y, c.z, c.r, None, c.so, c.probe, None, flags, cutoff)
    return up.astype(np.int64) + down


# ---- 1: the cluster ----------------------------------------------------------------------------------------------------------

def test_cluster_at_the_contact_radii_with_four_classes(ctx):
    c = hc.cluster()
    got = _run(ctx, c, rc.EDGES, rc.case_classes("cluster"), rc.N_CLASSES)
    _equal(got, _model("cluster", rc.EDGES))
    assert got.shape == (c.n_atoms, 4, 4) and all(got[:, b, k].any() for b in range(4) for k in range(4))


def test_cluster_with_its_cutoffs_as_an_edge_list(ctx):
    c = hc.cluster()
    edges = tuple(hc.cluster_cutoffs())            # 0, half a cell, ..., FLT_MAX: its square overflows, the whole grid is swept
    got = _run(ctx, c, edges, rc.case_classes("cluster"), rc.N_CLASSES)
    _equal(got, _model("cluster", edges))
    assert not got[:, :, 0].any()                                   # no two atoms coincide
    assert np.all(got.sum(axis=(1, 2)) == c.n_atoms - 1)            # everybody else lies in some bin


def test_one_class_and_one_bin_is_the_contact_number(ctx):
    c = hc.cluster()
    for cutoff in (13.0, float(c.h)):
        got = _run(ctx, c, (cutoff,))
        assert got.shape == (c.n_atoms, 1, 1)
        assert np.array_equal(got[:, 0, 0].astype(np.int64), _contact(ctx, c, cutoff))
        _equal(got, _model("cluster", (cutoff,), 1))


def test_cumulative_identity_with_the_half_sphere_exposure(ctx):
    c = hc.cluster()
    cl = rc.case_classes("cluster")
    edges = tuple(hc.cluster_cutoffs())
    flags = np.random.default_rng(31).integers(0, 4, c.n_atoms).astype(np.uint8)
    for fl in (None, flags):
        cum = np.cumsum(_run(ctx, c, edges, cl, rc.N_CLASSES, flags=fl).astype(np.int64), axis=2)
        for k, cutoff in enumerate(edges):
            assert np.array_equal(cum[:, :, k].sum(1), _contact(ctx, c, cutoff, fl)), (k, cutoff)
        base = np.full(c.n_atoms, 3, np.uint8) if fl is None else fl
        for b in range(rc.N_CLASSES):                               # per class: the partner bit cleared on the others
            only = np.where(cl == b, base, base & 2).astype(np.uint8)
            assert np.array_equal(cum[:, b, edges.index(13.0)], _contact(ctx, c, 13.0, only)), b


# ---- 2: histogram sizes --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_classes,n_bins", rc.SHAPES)
def test_rows_of_every_width(ctx, n_classes, n_bins):
    c = hc.cluster()
    cl = rc.case_classes("cluster", n_classes)
    edges = tuple(float(e) for e in rc.edges_of(n_bins))
    got, pairs = _run(ctx, c, edges, cl, n_classes, pairs=True)
    want = _model("cluster", edges, n_classes)
    assert got.shape == (c.n_atoms, n_classes, n_bins)
    _equal(got, want)
    _equal(pairs, rm.pairs_from_counts(want, c.so, cl))


def test_classes_below_n_classes_that_no_atom_has_leave_empty_rows(ctx):
    c = hc.cluster()
    cl = np.where(rc.case_classes("cluster") % 2 == 0, 0, 2).astype(np.uint8)
    got, pairs = _run(ctx, c, rc.EDGES, cl, 5, pairs=True)
    want = rm.counts(c.x, c.y, c.z, rc.EDGES, cl, 5)
    _equal(got, want)
    assert not got[:, [1, 3, 4]].any() and got[:, 0].any() and got[:, 2].any()
    _equal(pairs, rm.pairs_from_counts(want, c.so, cl))
    assert not pairs[0, [1, 3, 4]].any() and not pairs[0, :, [1, 3, 4]].any()
    _equal(_run(ctx, c, rc.EDGES, cl), want[:, :3])                   # n_classes None: max(classes) + 1


# ---- 3: contention and ties ----------------------------------------------------------------------------------------------------

def test_crowded_cell_one_cell_for_all_lanes_then_sixteen_classes(ctx):
    c = hc.crowd()
    _equal(_run(ctx, c, (13.0,)), _model("crowd", (13.0,), 1))       # 64 lanes add to the same LDS cell at once
    _equal(_run(ctx, c, (3.0,)), _model("crowd", (3.0,), 1))
    cl = rc.case_classes("crowd", 16)
    _equal(_run(ctx, c, rc.EDGES, cl, 16), _model("crowd", rc.EDGES, 16))         # ... and scatter


@pytest.mark.parametrize("edges,tie_bin,moved_bin", [((13.0,), 0, None), ((12.0, 13.0, 14.0), 1, 2), ((13.0, 13.0), 0, None),
                                                     ((12.0, 13.0, 13.0, 14.0), 1, 3)])
def test_exact_ties_land_in_the_first_bin_whose_edge_they_meet(ctx, edges, tie_bin, moved_bin):
    t, m = hc.ties(), hc.ties(True)
    cl = np.array([0, 0, 1, 2], np.uint8)
    got = _run(ctx, t, edges, cl, 3)
    want = np.zeros((4, 3, len(edges)), np.uint32)
    want[0, :, tie_bin] = 1                                         # d2 == 169 == e2 exactly: one partner of each class
    _equal(got, want)
    _equal(got, rm.counts(t.x, t.y, t.z, edges, cl, 3, t.flags))
    got = _run(ctx, m, edges, cl, 3)                                # one ulp further out: the next bin, or nowhere
    want = np.zeros((4, 3, len(edges)), np.uint32)
    if moved_bin is not None:
        want[0, :, moved_bin] = 1
    _equal(got, want)
    _equal(got, rm.counts(m.x, m.y, m.z, edges, cl, 3, m.flags))
    for c in (t, m):
        _equal(_run(ctx, c, edges, cl, 3, flags=None), rm.counts(c.x, c.y, c.z, edges, cl, 3, None))


# ---- 4: small edges --------------------------------------------------------------------------------------------------------------

def test_a_zero_edge_holds_the_coincident_atoms_and_an_underflowing_edge_too(ctx):
    c = hc.hand()
    cl = np.array([0, 1, 0, 1, 2, 2], np.uint8)
    got = _run(ctx, c, (0.0, 2.0, 3.0, 5.0), cl, 3)
    assert got[0].tolist() == [[0, 1, 0, 0], [0, 0, 2, 0], [1, 0, 0, 0]]
    assert got[4].tolist() == [[1, 1, 0, 0], [0, 0, 2, 0], [0, 0, 0, 0]] and not got[[1, 2, 3, 5]].any()
    for edges in ((0.0, 2.0, 3.0, 5.0), (1e-30, 5.0), (-0.0,), (0.0, 0.0), (1e-30,), (3.0, 3.0, 5.0)):
        assert edges[0] != 1e-30 or rm.e2_of(edges)[0] == 0.0        # the square underflows to 0
        _equal(_run(ctx, c, edges, cl, 3), rm.counts(c.x, c.y, c.z, edges, cl, 3, c.flags))
        _equal(_run(ctx, c, edges, cl, 3, flags=None), rm.counts(c.x, c.y, c.z, edges, cl, 3, None))
    k = hc.cluster()
    got = _run(ctx, k, (1e-30, float(k.h)))
    assert not got[:, :, 0].any()
    _equal(got, _model("cluster", (1e-30, float(k.h)), 1))


# ---- 5: the stop rule ------------------------------------------------------------------------------------------------------------

def test_tie_partners_in_the_last_swept_shell(ctx):
    c = hc.edge()
    cl = rc.case_classes("edge")
    hi, lo = c.info["hi"], c.info["lo"]
    got = _run(ctx, c, (hc.EDGE_CUTOFF,), cl, rc.N_CLASSES)
    _equal(got, _model("edge", (hc.EDGE_CUTOFF,)))
    assert got[[hi, lo]].sum(axis=(1, 2)).tolist() == [6, 6]        # the six ties, three of them in shell 3; none at 7
    got = _run(ctx, c, (hc.EDGE_CUTOFF, 7.0), cl, rc.N_CLASSES)
    _equal(got, _model("edge", (hc.EDGE_CUTOFF, 7.0)))
    assert got[[hi, lo], :, 0].sum(1).tolist() == [6, 6] and got[[hi, lo], :, 1].sum(1).min() >= 6      # those at 7 count now
    above = float(np.nextafter(F(hc.EDGE_CUTOFF), F(np.inf)))
    for edges in ((2.0, hc.EDGE_CUTOFF), (above,), (4.9,), (hc.EDGE_CUTOFF, hc.EDGE_CUTOFF)):
        _equal(_run(ctx, c, edges, cl, rc.N_CLASSES), _model("edge", edges))


# ---- 6: margins and bad atoms ------------------------------------------------------------------------------------------------------

def test_a_radius_of_70_fails_the_margins(ctx):
    c = hc.odd_radius()
    cl = rc.case_classes("cluster")
    for edges in (rc.EDGES, (3.28,), (0.0, 13.0)):
        got = _run(ctx, c, edges, cl, rc.N_CLASSES)
        _equal(got, _model("cluster", edges))                       # the radius changes the grid, not the table


def test_a_nan_coordinate_fails_the_margins_and_counts_nowhere(ctx):
    c = hc.nan_atom()
    a = c.info["atom"]
    cl = rc.case_classes("nan_atom")
    for edges in (rc.EDGES, (float(c.h), hc.COVER)):
        got, pairs = _run(ctx, c, edges, cl, rc.N_CLASSES, pairs=True)
        want = _model("nan_atom", edges)
        _equal(got, want)
        _equal(pairs, rm.pairs_from_counts(want, c.so, cl))
        assert not got[a].any()
    assert np.all(np.delete(got.sum(axis=(1, 2)), a) == c.n_atoms - 2)   # at COVER: everybody but the NaN atom and oneself


def test_result_does_not_depend_on_probe_or_radii(ctx):
    c = hc.cluster()
    cl = rc.case_classes("cluster")
    for kw in (dict(probe=0.5), dict(probe=3.0), dict(r=c.r * F(2.0))):
        _equal(_run(ctx, c, rc.EDGES, cl, rc.N_CLASSES, **kw), _model("cluster", rc.EDGES))


# ---- 7: flags and classes ----------------------------------------------------------------------------------------------------------

def test_flags(ctx):
    c = hc.cluster()
    n = c.n_atoms
    cl = rc.case_classes("cluster")
    rng = np.random.default_rng(21)
    half = rng.permutation(n) < n // 2
    base = _run(ctx, c, rc.EDGES, cl, rc.N_CLASSES, flags=None)
    _equal(base, _model("cluster", rc.EDGES))
    _equal(_run(ctx, c, rc.EDGES, cl, rc.N_CLASSES, flags=np.full(n, 3, np.uint8)), base)
    _equal(_run(ctx, c, rc.EDGES, cl, rc.N_CLASSES, flags=np.full(n, 0xFB, np.uint8)), base)      # the other bits are ignored
    for name, flags in (("centres only", np.full(n, 2, np.uint8)), ("partners only", np.full(n, 1, np.uint8)),
                        ("none", np.zeros(n, np.uint8)), ("disjoint", np.where(half, 1, 2).astype(np.uint8)),
                        ("mixed", rng.integers(0, 4, n).astype(np.uint8)),
                        ("unused bits", (rng.integers(0, 4, n) | 0xF4).astype(np.uint8)),
                        ("one in eight", np.where(np.arange(n) % 8 == 0, 3, 0).astype(np.uint8))):
        got, pairs = _run(ctx, c, rc.EDGES, cl, rc.N_CLASSES, flags=flags, pairs=True)
        want = rm.counts(c.x, c.y, c.z, rc.EDGES, cl, rc.N_CLASSES, flags)
        _equal(got, want)
        _equal(pairs, rm.pairs_from_counts(want, c.so, cl))
        assert not got[(flags & 2) == 0].any(), name                # rows of non-centres are zero
        if name in ("centres only", "partners only", "none"):
            assert not got.any() and not pairs.any()
    got = _run(ctx, c, rc.EDGES, cl, rc.N_CLASSES, flags=np.where(half, 1, 2).astype(np.uint8))
    assert got[~half].sum(axis=(1, 2)).min() > 0


def test_no_classes_with_three_classes(ctx):
    c = hc.cluster()
    got, pairs = _run(ctx, c, rc.EDGES, None, 3, pairs=True)
    assert got.shape == (c.n_atoms, 3, 4) and pairs.shape == (1, 3, 3, 4)
    _equal(got[:, :1], _model("cluster", rc.EDGES, 1))
    assert not got[:, 1:].any() and not pairs[0, 1:].any() and not pairs[0, :, 1:].any()
    assert np.array_equal(pairs[0, 0, 0], got[:, 0].astype(np.uint64).sum(0))


def test_a_permutation_of_the_atoms_permutes_the_rows(ctx):
    c = hc.crowd()
    cl = rc.case_classes("crowd")
    perm = np.random.default_rng(23).permutation(c.n_atoms)
    flags = np.random.default_rng(24).integers(0, 4, c.n_atoms).astype(np.uint8)
    base, pairs = _run(ctx, c, rc.EDGES, cl, rc.N_CLASSES, flags=flags, pairs=True)
    got, pairs_p = ctx.radial_counts(c.x[perm], c.y[perm], c.z[perm], c.r[perm], None, c.probe, rc.EDGES, cl[perm], rc.N_CLASSES,
                                     flags[perm], True)
    _equal(got, base[perm])
    _equal(pairs_p, pairs)


# ---- 8: batches and pair tables --------------------------------------------------------------------------------------------------

def _parts_equal_the_batch(ctx, c, cl, got, pairs):
    for s in range(len(c.so) - 1):
        p = hc.part(c, s)
        b, e = int(c.so[s]), int(c.so[s + 1])
        one, one_pairs = _run(ctx, p, rc.EDGES, cl[b:e], rc.N_CLASSES, pairs=True)
        _equal(one, got[b:e])
        _equal(one_pairs, pairs[s:s + 1])


def _batch_and_its_tables(ctx, name):
    c = getattr(hc, name)()
    cl = rc.case_classes(name)
    want = _model(name, rc.EDGES)
    want_pairs = rm.pairs_from_counts(want, c.so, cl)
    got, pairs = _run(ctx, c, rc.EDGES, cl, rc.N_CLASSES, pairs=True)
    _equal(got, want)
    _equal(pairs, want_pairs)
    assert pairs.shape == (len(c.so) - 1, rc.N_CLASSES, rc.N_CLASSES, len(rc.EDGES))
    only = _run(ctx, c, rc.EDGES, cl, rc.N_CLASSES, pairs="only")             # out_counts = NULL
    _equal(only, pairs)
    _equal(_run(ctx, c, rc.EDGES, cl, rc.N_CLASSES), want)                      # out_pairs = NULL
    return c, cl, got, pairs


def test_interleaved_structures_never_count_each_other(ctx):
    c, cl, got, pairs = _batch_and_its_tables(ctx, "interleaved")
    _parts_equal_the_batch(ctx, c, cl, got, pairs)
    both = rm.counts(c.x, c.y, c.z, rc.EDGES, cl, rc.N_CLASSES)       # as one structure: everybody has more partners
    assert np.all(got.sum(axis=(1, 2)) < both.sum(axis=(1, 2)))
    sym, sym_pairs = _run(ctx, c, rc.EDGES, cl, rc.N_CLASSES, flags=None, pairs=True)
    assert np.array_equal(sym_pairs, sym_pairs.transpose(0, 2, 1, 3)) and sym_pairs.any()       # flags NULL: symmetric
    flags = np.random.default_rng(25).integers(0, 4, c.n_atoms).astype(np.uint8)
    got, pairs = _run(ctx, c, rc.EDGES, cl, rc.N_CLASSES, flags=flags, pairs=True)
    want = rm.counts_batch(c.x, c.y, c.z, c.so, rc.EDGES, cl, rc.N_CLASSES, flags)
    _equal(got, want)
    _equal(pairs, rm.pairs_from_counts(want, c.so, cl))
    assert not np.array_equal(pairs, pairs.transpose(0, 2, 1, 3))


def test_empty_and_one_atom_structures(ctx):
    c, cl, got, pairs = _batch_and_its_tables(ctx, "tiny_batch")
    _parts_equal_the_batch(ctx, c, cl, got, pairs)
    sizes = np.diff(c.so.astype(np.int64))
    assert not pairs[sizes <= 1].any() and pairs[sizes == 40].all(axis=(2, 3)).any()
    e = np.zeros(0, F)
    for so in ([0], [0, 0, 0]):
        t, p = ctx.radial_counts_batch(e, e, e, e, None, np.array(so, np.uint32), pairs=True)
        assert t.shape == (0, 1, 4) and p.shape == (len(so) - 1, 1, 1, 4) and not p.any()
    t, p = ctx.radial_counts(e, e, e, e, pairs=True)
    assert t.shape == (0, 1, 4) and p.shape == (1, 1, 1, 4) and not p.any()
    one, p = ctx.radial_counts(np.ones(1, F), np.ones(1, F), np.ones(1, F), np.ones(1, F), pairs=True)
    assert one.shape == (1, 1, 4) and not one.any() and not p.any()


def test_batch_with_a_structure_of_65536_atoms(ctx):
    c, cl, got, pairs = _batch_and_its_tables(ctx, "tail_batch")
    b = int(c.so[-2])
    centres = c.info["centres"]
    total = got.sum(axis=(1, 2))
    assert total[b:][centres].min() >= 1 and total[b:].sum() == total[b:][centres].sum()
    big = hc.part(c, len(c.so) - 2)
    alone, alone_pairs = _run(ctx, big, rc.EDGES, cl[b:], rc.N_CLASSES, pairs=True)
    _equal(alone, got[b:])
    _equal(alone_pairs, pairs[-1:])


def test_three_hundred_structures_in_one_workgroup_of_the_pair_kernel(ctx):
    c = rc.many_small()
    cl = rc.classes_of(c.n_atoms, 3, 63)
    edges = (1.5, 3.0, 8.0)
    got, pairs = _run(ctx, c, edges, cl, 3, pairs=True)
    want = rm.counts_batch(c.x, c.y, c.z, c.so, edges, cl, 3)
    _equal(got, want)
    _equal(pairs, rm.pairs_from_counts(want, c.so, cl))
    assert np.all(got.sum(axis=(1, 2)) == 2) and np.all(pairs.sum(axis=(1, 2, 3)) == 6)
    _equal(_run(ctx, c, edges, cl, 3, pairs="only"), pairs)


def test_a_pair_cell_above_2_to_the_32(ctx):
    c = rc.big_box()
    n = c.n_atoms
    assert n * (n - 1) == 4303294400 > 2 ** 32
    got, pairs = _run(ctx, c, (rc.BOX_EDGE,), pairs=True)
    assert got.shape == (n, 1, 1) and got.dtype == np.uint32 and pairs.shape == (1, 1, 1, 1) and pairs.dtype == np.uint64
    assert np.array_equal(got[:, 0, 0], np.full(n, n - 1, np.uint32))           # every row is N - 1 = 65 599
    assert int(pairs[0, 0, 0, 0]) == n * (n - 1)


# ---- 9: errors and reuse -----------------------------------------------------------------------------------------------------------

def test_argument_errors_leave_the_context_usable(ctx):
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    lib = _capi.load()
    c = hc.edge()
    n = c.n_atoms
    cl = rc.case_classes("edge")
    want = _model("edge", (hc.EDGE_CUTOFF, 7.0))
    out = np.zeros((n, 4, 2), np.uint32)
    table = np.zeros((1, 4, 4, 2), np.uint64)
    cols = (ptr(c.x), ptr(c.y), ptr(c.z), ptr(c.r), None)
    so = np.array([0, n], np.uint32)
    falling = np.array([0, 40, 30, n], np.uint32)
    bad, ok = _capi.RSASA_ERR_INVALID_ARGUMENT, _capi.RSASA_OK
    one, many = lib.rsasa_radial_counts, lib.rsasa_radial_counts_batch
    E = lambda *v: np.array(v, F)  # noqa: E731
    good = E(hc.EDGE_CUTOFF, 7.0)
    cl_bad = cl.copy()
    cl_bad[n - 1] = 4                                               # a class byte equal to n_classes, on the last atom

    def call(edges, n_bins=None, n_classes=4, classes=cl, counts=out, pairs=table, batch=False, offsets=so, n_struct=1, x=c.x):
        where = (ptr(offsets), n_struct) if batch else (n,)
        return (many if batch else one)(ctx._h, ptr(x), *cols[1:], *where, c.probe, None, ptr(classes), n_classes, ptr(edges),
                                        len(edges) if n_bins is None else n_bins, ptr(counts), ptr(pairs))

    finite, order = "edges must be finite and not negative", "edges must be non-decreasing"
    errors = [
        (lambda: call(good, n_bins=0), "n_bins must be in [1, 32]"),
        (lambda: call(np.full(33, 5.0, F)), "n_bins must be in [1, 32]"),
        (lambda: call(good, n_classes=0), "n_classes must be in [1, 16]"),
        (lambda: call(good, n_classes=17), "n_classes must be in [1, 16]"),
        (lambda: call(E(5.0, float("nan"))), finite),
        (lambda: call(E(-1.0, 5.0)), finite),
        (lambda: call(E(5.0, float("inf"))), finite),
        (lambda: call(E(-1e-30, 5.0), batch=True), finite),
        (lambda: call(E(7.0, 5.0)), order),
        (lambda: call(E(5.0, 7.0, 6.0), batch=True), order),
        (lambda: call(good, classes=cl_bad), "classes must lie below n_classes"),
        (lambda: call(good, classes=cl, n_classes=3, batch=True), "classes must lie below n_classes"),
        (lambda: call(None, n_bins=2), "NULL argument"),
        (lambda: call(good, counts=None, pairs=None), "NULL argument"),
        (lambda: call(good, counts=None, pairs=None, batch=True), "NULL argument"),
        (lambda: call(good, x=None), "NULL argument"),
        (lambda: call(good, batch=True, offsets=None), "NULL argument"),
        (lambda: call(good, batch=True, offsets=falling, n_struct=3), "structure_offsets must be non-decreasing"),
    ]
    for k, (f, message) in enumerate(errors):
        assert f() == bad, k
        assert message in lib.rsasa_context_last_error(ctx._h).decode(), (k, lib.rsasa_context_last_error(ctx._h))
        assert not out.any() and not table.any(), k                 # nothing was written
        _equal(_run(ctx, c, (hc.EDGE_CUTOFF, 7.0), cl, rc.N_CLASSES), want)      # and the next call is right
    assert one(ctx._h, *cols, n, -5.0, None, ptr(cl), 4, ptr(good), 2, ptr(out), ptr(table)) == bad    # probe + max_r <= 0
    assert not out.any() and not table.any()
    # no structure and no atoms: OK with every pointer NULL, and the tables of empty structures are zeroed
    assert call(good, batch=True, offsets=so[1:], n_struct=0) == ok and not out.any()
    assert one(ctx._h, None, None, None, None, None, 0, 1.4, None, None, 1, ptr(good), 2, None, None) == ok
    stale = np.full((2, 4, 4, 2), 7, np.uint64)
    empty = np.zeros(3, np.uint32)
    assert many(ctx._h, None, None, None, None, None, ptr(empty), 2, 1.4, None, None, 4, ptr(good), 2, None, ptr(stale)) == ok
    assert not stale.any()
    stale[:] = 7
    assert one(ctx._h, None, None, None, None, None, 0, 1.4, None, None, 4, ptr(good), 2, None, ptr(stale)) == ok
    assert not stale[0].any() and np.all(stale[1] == 7)             # the single form has one table
    # -0.0 and equal edges stand; either output alone stands
    assert call(E(-0.0, -0.0)) == ok
    _equal(out, _model("edge", (-0.0, -0.0)))
    assert call(E(7.0, 7.0), pairs=None) == ok
    _equal(out, _model("edge", (7.0, 7.0)))
    assert call(good, counts=None) == ok
    _equal(table, rm.pairs_from_counts(want, c.so, cl))
    assert call(good) == ok
    _equal(out, want)


def test_python_argument_checks(ctx):
    import rustsasa_amd
    c = hc.hand()
    cl = np.array([0, 1, 0, 1, 2, 2])
    for kw in (dict(flags=c.flags[:3]), dict(flags=c.flags.astype(F)), dict(flags=np.full(6, 256)), dict(classes=cl[:3]),
               dict(classes=cl.astype(F)), dict(classes=np.full(6, 256)), dict(classes=np.full(6, -1)), dict(n_classes=0),
               dict(n_classes=17), dict(n_classes=2.5), dict(edges=()), dict(edges=np.ones(33)), dict(edges=np.ones((2, 2))),
               dict(pairs="all")):
        with pytest.raises(ValueError):
            ctx.radial_counts(*c.cols, **kw)
    for kw in (dict(classes=cl, n_classes=2), dict(edges=(2.0, 1.0)), dict(edges=(float("nan"),))):
        with pytest.raises(rustsasa_amd.RsasaError) as e:
            ctx.radial_counts(*c.cols, **kw)
        assert e.value.status == -1
    got = ctx.radial_counts(*c.cols, edges=np.array([0, 2, 3, 5], np.float64), classes=cl.astype(np.int64),
                            flags=c.flags.astype(np.int64))
    assert got.shape == (6, 3, 4) and got[0].tolist() == [[0, 1, 0, 0], [0, 0, 2, 0], [1, 0, 0, 0]]


def test_an_infinite_coordinate_is_refused_and_the_next_call_is_right(ctx):
    import rustsasa_amd
    c = hc.edge()
    cl = rc.case_classes("edge")
    x = c.x.copy()
    x[5] = np.inf
    for call in (lambda: ctx.radial_counts(x, c.y, c.z, c.r, None, c.probe, rc.EDGES, cl, rc.N_CLASSES, None, True),
                 lambda: ctx.radial_counts_batch(x, c.y, c.z, c.r, None, c.so, c.probe, rc.EDGES, cl, rc.N_CLASSES, None, "only")):
        with pytest.raises(rustsasa_amd.RsasaError) as e:
            call()
        assert e.value.status == -5
        _equal(_run(ctx, c, rc.EDGES, cl, rc.N_CLASSES), _model("edge", rc.EDGES))


def _family_calls(ctx, c):
    import rustsasa_amd
    groups = (np.arange(c.n_atoms) % 5).astype(np.uint32)
    link = rustsasa_amd.default_link(c.r, c.probe, 100)
    return [lambda: ctx.precompute_neighbors(*c.cols, c.probe),
            lambda: ctx.accessible_points(*c.cols, c.probe, 100),
            lambda: ctx.exposure_vectors(*c.cols, c.probe, 100),
            lambda: ctx.atom_depth(*c.cols, c.probe, 100),
            lambda: ctx.surface_components(*c.cols, c.probe, 100, link),
            lambda: ctx.contact_points(*c.cols, c.probe, 100),
            lambda: ctx.group_contacts(*c.cols, groups, c.probe, 100),
            lambda: ctx.half_sphere_exposure(*c.cols, c.probe, c.dirs, None, 13.0),
            lambda: ctx.atoms_within(*c.cols, c.probe, None, 8.0),
            lambda: ctx.nearest_atoms(*c.cols, c.probe, 16),
            lambda: ctx.calculate_sasa_soa(*c.cols, c.probe, 100)]


def test_between_calls_of_every_other_family(ctx):
    import rustsasa_amd
    c, t = hc.edge(), hc.tiny_batch()
    cl, cl_t = rc.case_classes("edge"), rc.case_classes("tiny_batch")
    want, want_t = _model("edge", rc.EDGES), _model("tiny_batch", rc.EDGES)
    want_pairs = rm.pairs_from_counts(want_t, t.so, cl_t)
    with rustsasa_amd.Context(0) as fresh:
        alone = [call() for call in _family_calls(fresh, c)]
    tup = lambda v: (v,) if isinstance(v, np.ndarray) else tuple(v)  # noqa: E731
    for call, ref in zip(_family_calls(ctx, c), alone):
        before = call()
        _equal(_run(ctx, c, rc.EDGES, cl, rc.N_CLASSES), want)
        got, pairs = _run(ctx, t, rc.EDGES, cl_t, rc.N_CLASSES, pairs=True)
        _equal(got, want_t)
        _equal(pairs, want_pairs)
        after = call()
        assert len(tup(before)) == len(tup(after)) == len(tup(ref))
        for a, b_, r in zip(tup(before), tup(after), tup(ref)):
            assert a.tobytes() == b_.tobytes() == r.tobytes()


def test_changing_classes_bins_and_flags_between_calls(ctx):
    c = hc.cluster()
    flags = np.random.default_rng(27).integers(0, 4, c.n_atoms).astype(np.uint8)
    # wide, narrow, wide again; flags and classes come and go: the workspace's buffers are found sized by other calls
    for n_classes, n_bins, fl, with_classes in ((16, 32, None, True), (1, 1, flags, False), (5, 13, flags, True), (1, 1, None, False),
                                                (16, 32, flags, True), (3, 7, None, True)):
        cl = rc.case_classes("cluster", n_classes) if with_classes else None
        edges = tuple(float(e) for e in rc.edges_of(n_bins))
        got, pairs = _run(ctx, c, edges, cl, n_classes, flags=fl, pairs=True)
        want = _model("cluster", edges, n_classes) if fl is None and with_classes else rm.counts(c.x, c.y, c.z, edges, cl, n_classes, fl)
        _equal(got, want)
        _equal(pairs, rm.pairs_from_counts(want, c.so, cl))
