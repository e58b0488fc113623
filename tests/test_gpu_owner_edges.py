"""The second pass over the contact owners on the GPU (k_contact_owners and its co_test, points.hip) on the cases of
owner_edge_cases.py, pinned by test_owner_edges_cpu.py: every exact tie of tie_cases.py - co_test writes out the two
dots of pt_hit itself, and only a point at dot == limit tells its `<` and `<=` from the original's -, lists of two and
three windows of 256 entries at three and four passes, where owned[] is added to across passes, and the degenerate
radius / probe batches the contact counts run.  Lists against the oracle, owned and owner against owners_model.py, the
values against the oracle byte for byte.  No tolerances."""
import numpy as np
import pytest

import nb_helpers as nh
import owner_cases as oc
import owner_edge_cases as oe
import owners_model as om
import point_edge_cases as pe
import tie_cases as tc
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


def _check_shapes(got, n_atoms, n_points):
    offs, ent, owned, sasa, owner = got
    assert offs.dtype == np.uint64 and offs.shape == (n_atoms + 1,)
    assert owned.dtype == np.uint32 and owner.dtype == np.uint32 and sasa.dtype == np.float32
    assert owned.shape == ent.shape == (int(offs[-1]),) and sasa.shape == (n_atoms,) and owner.shape == (n_atoms, n_points)


def _batch_against_the_models(ctx, cat, so, probe, n_points, W, model=None):
    """contact_owners_batch(points=True) at the context's lane count W: the lists equal the oracle's, owned and owner the
    model's, the values the oracle's byte for byte; entry by entry exclusive <= owned <= covered of contact_points_batch."""
    got = ctx.contact_owners_batch(*cat, so, probe, n_points, points=True)
    _check_shapes(got, int(so[-1]), n_points)
    nh.assert_same(got[:2], nh.oracle_batch_csr(*cat, so, probe))
    owned_m, owner_m = om.owners_batch(*cat, so, probe, n_points, W) if model is None else model
    bad = np.flatnonzero(got[2] != owned_m)
    assert bad.size == 0, ("owned", probe, n_points, W, bad.size, bad[:5], got[2][bad[:5]], owned_m[bad[:5]])
    bad = np.argwhere(got[4] != owner_m)
    assert len(bad) == 0, ("owner", probe, n_points, W, len(bad), bad[:5].tolist())
    oracle = po.calculate_sasa_batch(*cat, so, probe, n_points, W, threads=0)
    assert got[3].tobytes() == oracle.tobytes(), (probe, n_points, W)
    cp = ctx.contact_points_batch(*cat, so, probe, n_points)
    assert cp[0].tobytes() == got[0].tobytes() and cp[1].tobytes() == got[1].tobytes()
    assert np.all(cp[3] <= got[2]) and np.all(got[2] <= cp[2]), (probe, n_points, W)
    return got


# ---- 1: every tie case through the owner kernel ---------------------------------------------------------------------------

def test_tie_cases_owners(ctx):
    n = 0
    try:
        for (probe, n_points, W), sts in sorted(oe.tie_groups().items()):
            x, y, z, r, ids, so = tc.pack(sts)
            ctx.set_simd_width(W)
            _batch_against_the_models(ctx, (x, y, z, r, ids), so, probe, n_points, W)
            n += len(sts)
    finally:
        ctx.set_simd_width(8)
    assert n > 10000


# ---- 2: three and four passes over two and three windows ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def pass_window_models():
    return pe.pmap(lambda k: oe.pass_window_model(*k), oe.PASS_WINDOW_CASES)


@pytest.mark.parametrize("name,n_points", oe.PASS_WINDOW_CASES)
def test_owned_adds_up_across_passes_window_by_window(ctx, pass_window_models, name, n_points):
    cols, c0 = oe.named_cols(name)
    offs_m, ent_m, by_w = pass_window_models[(name, n_points)]
    n = len(cols[0])
    k = int(np.diff(offs_m.astype(np.int64))[c0])
    assert oe.passes(n_points) >= 3 and oe.windows(k) >= 2 and oe.passes(n_points) + oe.windows(k) >= 6
    so = np.array([0, n], np.uint32)
    try:
        for W in oe.WS:
            owned_m, owner_m = by_w[W]
            # the case bites: in every pass of 256 points, every window of the list owns a point of the cluster's spheres
            o = owner_m[c0:]
            for p0 in range(0, n_points, 4 * pe.WAVE):
                part = o[:, p0:p0 + 4 * pe.WAVE]
                part = part[part != om.FREE]
                assert {int(v) for v in np.unique(part // oc.PT_STAGE)} == set(range(oe.windows(k))), (W, p0)
            ctx.set_simd_width(W)
            got = ctx.contact_owners(*cols, 1.4, n_points, points=True)
            _check_shapes(got, n, n_points)
            nh.assert_same(got[:2], (offs_m, ent_m))
            assert np.array_equal(got[2], owned_m), W
            assert np.array_equal(got[4], owner_m), W
            again = ctx.contact_owners_batch(*cols, so, 1.4, n_points)   # over its own earlier result, without the owner rows
            assert all(again[j].tobytes() == got[j].tobytes() for j in range(4)), W
            oracle = po.calculate_sasa_internal(*cols, 1.4, n_points, W, threads=0)
            assert got[3].tobytes() == oracle.tobytes(), W
    finally:
        ctx.set_simd_width(8)


# ---- 3: radii and probes off the protein range, in a batch ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def degenerate_models():
    return oe.degenerate_models()


@pytest.mark.parametrize("k", range(oe.N_DEGENERATE))
def test_degenerate_radii_and_probes_in_a_batch(ctx, degenerate_models, k):
    cat, so, probe = oe.degenerate_batch(k)
    n_points, W = oe.DEGENERATE_BATCH
    try:
        ctx.set_simd_width(W)
        _batch_against_the_models(ctx, cat, so, probe, n_points, W, degenerate_models[k])
    finally:
        ctx.set_simd_width(8)
