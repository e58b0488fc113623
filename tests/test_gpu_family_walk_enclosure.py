"""The sibling of test_gpu_family_walk.py and test_gpu_family_walk_crowding.py for the fourteenth family: the dot
enclosure shares the prologue of the point runs and, in the scratch, `free` and `row_offsets` with the depth, component,
group and crowding runs and `flags` / `sorted_flags` with the runs on the grid alone and with the crowding - the radial
counts leave (class << 2) | flags in the sorted bytes, of which the enclosure reads bit 0.  One context is walked through
the twelve families and back with a dot-enclosure call after every step, on the walk's own inputs (A one atom, B the 1jcd
fixture, C a batch of A, an empty structure and B); in every other step a dot-crowding call with OTHER flag bytes stands
between the family's call and the enclosure's, so that the two newest families follow one another too.  Every
dot-enclosure result equals, byte for byte, the same call on a context that made no other call, and B equals the model."""
import numpy as np
import pytest

import crowding_cases as cc
import enclosure_model as em
import points_model as pm
import test_gpu_family_walk as fw

pytestmark = pytest.mark.gpu

N_POINTS = 100
N_DIRS = 30
REACH = 8.0
CROWD_EDGES = (5.0, 9.0)


def _flags(n):
    return cc.random_flags(n, 86)


def _crowd_flags(n):
    return cc.random_flags(n, 87)


def _enclose(ctx, inp):
    x, y, z, r, ids, _, so = inp
    tail = (fw.PROBE, N_POINTS, N_DIRS, REACH, _flags(len(x)))
    return ctx.dot_enclosure(x, y, z, r, ids, *tail) if so is None else ctx.dot_enclosure_batch(x, y, z, r, ids, so, *tail)


def _crowd(ctx, inp):
    x, y, z, r, ids, _, so = inp
    tail = (fw.PROBE, N_POINTS, CROWD_EDGES, _crowd_flags(len(x)))
    return ctx.dot_crowding(x, y, z, r, ids, *tail) if so is None else ctx.dot_crowding_batch(x, y, z, r, ids, so, *tail)


@pytest.fixture(scope="module")
def alone():
    import rustsasa_amd
    out = {}
    for name, inp in fw._inputs().items():
        with rustsasa_amd.Context(0) as ctx:
            out[name] = _enclose(ctx, inp)
    return out


def test_first_call_on_a_fresh_context(alone):
    off, words, free, sasa = alone["A"]          # one atom: its list is empty, no fill has ever run
    assert off.tolist() == [0, N_POINTS] and free.tolist() == [N_POINTS] and words.shape == (N_POINTS,)
    x, y, z, r = fw._inputs()["A"][:4]
    want = em.blocked(x, y, z, r, np.ones((1, N_POINTS), bool), fw.PROBE, N_POINTS, N_DIRS, REACH, _flags(1))[1]
    assert np.array_equal(words, want)
    assert np.array_equal(words, em.own_bits(N_POINTS, N_DIRS) if _flags(1)[0] & 1 else np.zeros(N_POINTS, np.uint32))


def test_walk_with_the_dot_enclosure_after_every_step(alone):
    import rustsasa_amd
    assert (_flags(700) & 1 != _crowd_flags(700) & 1).any()              # the crowding leaves other flags behind
    with rustsasa_amd.Context(0) as ctx:
        for step, family in enumerate(fw.ORDER + fw.ORDER[::-1]):
            for name in ("B", "A", "C"):
                fw._call(ctx, family, fw._inputs()[name], N_POINTS)
                if step % 2:
                    _crowd(ctx, fw._inputs()[name])
                assert fw._same(_enclose(ctx, fw._inputs()[name]), alone[name]), (step, family, name)


def test_fixture_equals_the_model(alone):
    x, y, z, r, ids, _, _ = fw._inputs()["B"]
    mask = pm.exposed_masks(x, y, z, r, ids, fw.PROBE, N_POINTS, 8)
    w_off, w_words = em.blocked(x, y, z, r, mask, fw.PROBE, N_POINTS, N_DIRS, REACH, _flags(len(x)))
    off, words, free, sasa = alone["B"]
    assert np.array_equal(off, w_off) and np.array_equal(words, w_words) and words.any() and not (words >> np.uint32(N_DIRS)).any()
    assert np.array_equal(free, mask.sum(axis=1))
    assert sasa.tobytes() == pm.sasa_of(r, fw.PROBE, mask.sum(axis=1), N_POINTS).tobytes()
    c_off, c_words = alone["C"][:2]             # the batch: A's dots, then B's, offsets batch-global
    assert np.array_equal(c_off[1:].astype(np.int64) - N_POINTS, off.astype(np.int64)) and len(c_words) == N_POINTS + len(words)
