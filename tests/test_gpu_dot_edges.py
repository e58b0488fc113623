"""The second suite of the dot crowding and the dot enclosure on the GPU (k_dot_crowding of crowding.hip, k_dot_enclosure
of enclosure.hip): the cases of dot_edge_cases.py - lattices whose masks take a second and a third trip of 64 words, every
class of pass with staging batches that make the lane groups' split matter, the stop rules at their clamps and
boundaries, the cuts and the ties at coordinates of 65536 h - against the exact CPU models (crowding_model.py,
enclosure_model.py) by np.array_equal.  test_dot_edges_cpu.py pins every case to what it is named for."""
import numpy as np
import pytest

import crowding_cases as cc
import crowding_model as cm
import dot_edge_cases as de
import enclosure_cases as ec
import enclosure_model as em
import points_model as pm

pytestmark = pytest.mark.gpu

_MASKS = {}


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


def _masks(c):
    """The masks of a case, computed once and shared by both families (the key is the input itself)."""
    key = (c.x.tobytes(), c.y.tobytes(), c.z.tobytes(), c.r.tobytes(), c.so.tobytes(), float(c.probe), c.n_points)
    if key not in _MASKS:
        _MASKS[key] = cc.masks(c)
    return _MASKS[key]


def _equal(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), [int(got[tuple(b)]) for b in bad[:5]],
                           [int(want[tuple(b)]) for b in bad[:5]])


def _rest(c, mask, off, free, sasa):
    _equal(off, cm.offsets_of(mask))
    want_free = mask.sum(axis=1).astype(np.uint32)
    _equal(free, want_free)
    assert sasa.tobytes() == pm.sasa_of(c.r, c.probe, want_free, c.n_points).tobytes()


def _crowding(ctx, c, edges=None):
    """dot_crowding against the model: offsets, rows, free and the values."""
    edges = c.edges if edges is None else edges
    mask = _masks(c)
    if len(c.so) == 2:
        off, rows, free, sasa = ctx.dot_crowding(*c.cols, c.probe, c.n_points, edges, c.flags)
    else:
        off, rows, free, sasa = ctx.dot_crowding_batch(*c.cols, c.so, c.probe, c.n_points, edges, c.flags)
    _rest(c, mask, off, free, sasa)
    _equal(rows, cm.counts_batch(c.x, c.y, c.z, c.r, c.so, mask, c.probe, c.n_points, edges, c.flags)[1])
    return off, rows, mask


def _enclosure(ctx, c, reach=None):
    """dot_enclosure against the model: offsets, words, free and the values."""
    reach = c.reach if reach is None else reach
    mask = _masks(c)
    if len(c.so) == 2:
        off, words, free, sasa = ctx.dot_enclosure(*c.cols, c.probe, c.n_points, c.n_dirs, reach, c.flags)
    else:
        off, words, free, sasa = ctx.dot_enclosure_batch(*c.cols, c.so, c.probe, c.n_points, c.n_dirs, reach, c.flags)
    _rest(c, mask, off, free, sasa)
    _equal(words, em.blocked_batch(c.x, c.y, c.z, c.r, c.so, mask, c.probe, c.n_points, c.n_dirs, reach, c.flags)[1])
    return off, words, mask


# ---- A: lattices past 2048 points --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n_points", de.BIG)
def test_masks_of_65_and_129_words(ctx, name, n_points):
    """The second and third trip of the mask compaction, the rank carried from one to the next and the early exit in a
    later one, in both kernels; and k_accessible_points and k_mask_free themselves past 2048 points."""
    c = de.big(name, n_points)
    mask = _masks(c)
    packed, sasa = ctx.accessible_points_batch(*c.cols, c.so, c.probe, n_points)
    assert packed.shape == (c.n_atoms, -(-n_points // 32))
    _equal(packed, pm.pack(mask))
    assert sasa.tobytes() == pm.sasa_of(c.r, c.probe, mask.sum(axis=1), n_points).tobytes()
    off, rows, _ = _crowding(ctx, c)
    assert rows.any() and int(off[-1]) == int(mask.sum())
    off, words, _ = _enclosure(ctx, ec.of(c))
    if name == "lone":
        assert off.tolist() == [0, n_points] and np.array_equal(words, em.own_bits(n_points, ec.N_DIRS)) and words.any()
        assert np.array_equal(rows, np.tile(np.array([[0, 1, 0]], np.uint32), (n_points, 1)))
    else:
        assert (words & ~em.own_bits(n_points, ec.N_DIRS)[np.nonzero(mask)[1]]).any()


# ---- B: every class of pass ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_cluster", de.SPLIT_CLUSTERS)
def test_every_class_of_pass_for_the_crowding(ctx, n_cluster):
    """The case's own three edges, and n_bins = 4 and 5: the two sides of the launch split between the kernel with four
    and with eight counters a dot."""
    c = de.split(n_cluster)
    off, rows, mask = _crowding(ctx, c)
    assert de.pass_classes(mask.sum(axis=1)[c.info["owners"]]) == set(de.CLASSES)
    assert all(rows[int(off[o]):int(off[o + 1])].any() for o in c.info["owners"])
    for edges in ((3.5, 4.5, 6.0, 9.0), (3.5, 4.5, 5.0, 6.0, 9.0)):
        _, more, _ = _crowding(ctx, c, edges)
        assert more.shape[1] == len(edges) and np.array_equal(more.sum(axis=1), rows.sum(axis=1))


@pytest.mark.parametrize("n_cluster", de.SPLIT_CLUSTERS)
def test_every_class_of_pass_for_the_enclosure(ctx, n_cluster):
    c = ec.of(de.split(n_cluster), reach=de.SPLIT_REACH)
    off, words, mask = _enclosure(ctx, c)
    own = em.own_bits(c.n_points, c.n_dirs)
    assert all((words[int(off[o]):int(off[o + 1])] & ~own[np.flatnonzero(mask[o])]).any() for o in c.info["owners"])


# ---- C: the stop rules ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shells,on,reach", de.boundary_reaches(),
                         ids=["%d%s" % (s, "" if on else "+") for s, on, _ in de.boundary_reaches()])
def test_enclosure_at_the_stop_rules_boundaries(ctx, shells, on, reach):
    """Reach (s - 2.5) h, which the rule admits after s shells, and the float above it, which needs one shell more."""
    _enclosure(ctx, de.boundary_case(reach))


@pytest.mark.parametrize("shell", [s for s in cc.LAST_SHELLS if s != cc.LAST_SHELL])
def test_crowding_tie_partners_in_the_last_swept_shell_down_to_the_clamp(ctx, shell):
    c = cc.last_shell(shell)
    off, rows, _ = _crowding(ctx, c)
    for owner, k, _ in c.info["ties"]:
        assert rows[int(off[owner]) + k, -1] >= 1


@pytest.mark.parametrize("shell", [s for s in ec.LAST_SHELLS if s != ec.LAST_SHELL])
def test_enclosure_rays_stopped_in_the_last_swept_shell_down_to_the_clamp(ctx, shell):
    c = ec.last_shell(shell)
    off, words, _ = _enclosure(ctx, c)
    for owner, k, m, _ in c.info["rays"]:
        assert (int(words[int(off[owner]) + k]) >> m) & 1


# ---- D: coordinates of 65536 h -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis,sign", de.MARGIN_MOVES)
@pytest.mark.parametrize("name", de.MOVED)
def test_enclosure_cuts_and_last_shells_just_under_the_margins(ctx, name, axis, sign):
    c = de.moved_enclosure(name, axis, sign)
    off, words, mask = _enclosure(ctx, c)
    assert (words & ~em.own_bits(c.n_points, c.n_dirs)[np.nonzero(mask)[1]]).any()


def test_the_obstacle_that_only_the_absolute_term_of_the_staging_cut_keeps(ctx):
    c = de.abs_candidate(de.ABS_SEED)
    off, words, _ = _enclosure(ctx, c)
    assert int(words[int(off[c.info["owner"]])]) & 1


@pytest.mark.parametrize("axis,sign", de.MARGIN_MOVES)
@pytest.mark.parametrize("kind", ["last", "below"])
def test_crowding_ties_just_under_the_margins(ctx, kind, axis, sign):
    c = de.moved_tie(kind, axis, sign)
    off, rows, mask = _crowding(ctx, c)
    assert rows[de.rank_of(mask[0], cc.TIE_DOT)].tolist() == {"last": [1, 1], "below": [1, 0]}[kind]
