"""The sibling of test_gpu_family_walk_fields.py for the dot curvature: it shares the prologue of the point runs and, in
the scratch, `free` and `row_offsets` with the depth, component, link, crowding, fields and group runs; its pair counts
and moments are buffers of its own that the call zeroes before the kernel adds to them.  One context is walked through
the twelve families and back with a dot-curvature call (and, every other step, a dot-links call at another link before
it) after every step, on the walk's own inputs (A one atom, B the 1jcd fixture, C a batch of A, an empty structure and
B); every dot-curvature result equals, byte for byte, the same call on a context that made no other call, and B equals
the model."""
import numpy as np
import pytest

import curvature_model as cvm
import points_model as pm
import test_gpu_family_walk as fw

pytestmark = pytest.mark.gpu

N_POINTS = 100
REACH = 3.0


def _curvature(ctx, inp):
    x, y, z, r, ids, _, so = inp
    tail = (fw.PROBE, N_POINTS, REACH)
    return ctx.dot_curvature(x, y, z, r, ids, *tail) if so is None else ctx.dot_curvature_batch(x, y, z, r, ids, so, *tail)


@pytest.fixture(scope="module")
def alone():
    import rustsasa_amd
    out = {}
    for name, inp in fw._inputs().items():
        with rustsasa_amd.Context(0) as ctx:
            out[name] = _curvature(ctx, inp)
    return out


def test_first_call_on_a_fresh_context(alone):
    off, pairs, mom, free, sasa = alone["A"]    # one atom: its list is empty, no fill has ever run
    assert off.tolist() == [0, N_POINTS] and free.tolist() == [N_POINTS]
    assert pairs.shape == (N_POINTS,) and pairs.dtype == np.uint32 and mom.shape == (N_POINTS, 8) and mom.dtype == np.int64
    x, y, z, r = fw._inputs()["A"][:4]
    _, w_pairs, w_mom, _ = cvm.rows(x, y, z, r, np.ones((1, N_POINTS), bool), fw.PROBE, N_POINTS, REACH)
    assert np.array_equal(pairs, w_pairs) and np.array_equal(mom, w_mom) and pairs.all()


def test_walk_with_the_dot_curvature_after_every_step(alone):
    import rustsasa_amd
    with rustsasa_amd.Context(0) as ctx:
        for step, family in enumerate(fw.ORDER + fw.ORDER[::-1]):
            for name in ("B", "A", "C"):
                inp = fw._inputs()[name]
                fw._call(ctx, family, inp, N_POINTS)
                if step % 2:
                    x, y, z, r, ids, _, so = inp
                    tail = (fw.PROBE, N_POINTS, 1.25)
                    ctx.dot_links(x, y, z, r, ids, *tail) if so is None else ctx.dot_links_batch(x, y, z, r, ids, so, *tail)
                assert fw._same(_curvature(ctx, inp), alone[name]), (step, family, name)


def test_fixture_equals_the_model(alone):
    x, y, z, r, ids, _, _ = fw._inputs()["B"]
    mask = pm.exposed_masks(x, y, z, r, ids, fw.PROBE, N_POINTS, 8)
    w_off, w_pairs, w_mom, _ = cvm.rows(x, y, z, r, mask, fw.PROBE, N_POINTS, REACH)
    off, pairs, mom, free, sasa = alone["B"]
    assert np.array_equal(off, w_off) and np.array_equal(pairs, w_pairs) and np.array_equal(mom, w_mom)
    assert mom.any(axis=0).all() and np.array_equal(free, mask.sum(axis=1))
    assert sasa.tobytes() == pm.sasa_of(r, fw.PROBE, mask.sum(axis=1), N_POINTS).tobytes()
    c_off, c_pairs = alone["C"][:2]             # the batch: A's dots, then B's, offsets batch-global
    assert np.array_equal(c_off[1:].astype(np.int64) - N_POINTS, off.astype(np.int64)) and len(c_pairs) == N_POINTS + len(pairs)
