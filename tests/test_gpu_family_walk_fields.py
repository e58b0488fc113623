"""The sibling of test_gpu_family_walk_crowding.py for the dot fields: they share the prologue of the point runs and, in
the scratch, `free` and `row_offsets` with the depth, component, crowding and group runs and `flags` / `sorted_flags` with
the four runs on the grid alone - the radial counts leave (class << 2) | flags in the sorted bytes, of which the fields
read bit 0.  One context is walked through the twelve families and back with a dot-fields call (and, every other step, a
dot-crowding call before it) after every step, on the walk's own inputs (A one atom, B the 1jcd fixture, C a batch of A,
an empty structure and B); every dot-fields result equals, byte for byte, the same call on a context that made no other
call, and B equals the model."""
import numpy as np
import pytest

import crowding_cases as cc
import fields_cases as fc
import fields_model as fm
import points_model as pm
import test_gpu_family_walk as fw

pytestmark = pytest.mark.gpu

N_POINTS = 100
KINDS = (fm.INV_D, fm.STEP, fm.INV_1PD, fm.INV_D2)
CUTOFF = 10.0


def _flags(n):
    return cc.random_flags(n, 86)


def _weights(n):
    return fc.weights(n, len(KINDS), 87)


def _fields(ctx, inp):
    x, y, z, r, ids, _, so = inp
    tail = (fw.PROBE, N_POINTS, _weights(len(x)), KINDS, CUTOFF, _flags(len(x)))
    return ctx.dot_fields(x, y, z, r, ids, *tail) if so is None else ctx.dot_fields_batch(x, y, z, r, ids, so, *tail)


@pytest.fixture(scope="module")
def alone():
    import rustsasa_amd
    out = {}
    for name, inp in fw._inputs().items():
        with rustsasa_amd.Context(0) as ctx:
            out[name] = _fields(ctx, inp)
    return out


def test_first_call_on_a_fresh_context(alone):
    off, rows, free, sasa = alone["A"]          # one atom: its list is empty, no fill has ever run
    assert off.tolist() == [0, N_POINTS] and free.tolist() == [N_POINTS]
    assert rows.shape == (N_POINTS, len(KINDS)) and rows.dtype == np.int64
    x, y, z, r = fw._inputs()["A"][:4]
    want = fm.sums(x, y, z, r, np.ones((1, N_POINTS), bool), fw.PROBE, N_POINTS, _weights(1), KINDS, CUTOFF, _flags(1))[1]
    assert np.array_equal(rows, want)


def test_walk_with_the_dot_fields_after_every_step(alone):
    import rustsasa_amd
    with rustsasa_amd.Context(0) as ctx:
        for step, family in enumerate(fw.ORDER + fw.ORDER[::-1]):
            for name in ("B", "A", "C"):
                inp = fw._inputs()[name]
                fw._call(ctx, family, inp, N_POINTS)
                if step % 2:
                    x, y, z, r, ids, _, so = inp
                    tail = (fw.PROBE, N_POINTS, (4.0, 10.0), _flags(len(x))[::-1].copy())
                    ctx.dot_crowding(x, y, z, r, ids, *tail) if so is None else ctx.dot_crowding_batch(x, y, z, r, ids, so, *tail)
                assert fw._same(_fields(ctx, inp), alone[name]), (step, family, name)


def test_fixture_equals_the_model(alone):
    x, y, z, r, ids, _, _ = fw._inputs()["B"]
    mask = pm.exposed_masks(x, y, z, r, ids, fw.PROBE, N_POINTS, 8)
    w_off, w_rows = fm.sums(x, y, z, r, mask, fw.PROBE, N_POINTS, _weights(len(x)), KINDS, CUTOFF, _flags(len(x)))
    off, rows, free, sasa = alone["B"]
    assert np.array_equal(off, w_off) and np.array_equal(rows, w_rows) and rows.any(axis=0).all()
    assert np.array_equal(free, mask.sum(axis=1))
    assert sasa.tobytes() == pm.sasa_of(r, fw.PROBE, mask.sum(axis=1), N_POINTS).tobytes()
    c_off, c_rows = alone["C"][:2]              # the batch: A's dots, then B's, offsets batch-global
    assert np.array_equal(c_off[1:].astype(np.int64) - N_POINTS, off.astype(np.int64)) and len(c_rows) == N_POINTS + len(rows)
