"""The inputs of dot_edge_cases.py without a GPU: every case pinned, from the models alone, to what it is named for in the
frame that k_dot_crowding and k_dot_enclosure share - the trips of the mask compaction, the classes of a pass and the
staging batches the lane groups share out, the stop rules at their clamps, the cuts and the ties at coordinates of
65536 h - and the emulated sweeps' switches (`early`, `abs_term`) showing that each case bites."""
import numpy as np
import pytest

import crowding_cases as cc
import crowding_model as cm
import depth_model as dm
import dot_edge_cases as de
import enclosure_cases as ec
import enclosure_model as em
import sweep_cases as sc
import sweep_model as sm

F = np.float32


def _part(c, s=0):
    b, e = int(c.so[s]), int(c.so[s + 1])
    return c.x[b:e], c.y[b:e], c.z[b:e], c.r[b:e]


def _crowding(c):
    mask = cc.masks(c)
    off, rows = cm.counts_batch(c.x, c.y, c.z, c.r, c.so, mask, c.probe, c.n_points, c.edges, c.flags)
    return off, rows, mask


def _enclosure(c, **kw):
    mask = ec.masks(c)
    args = dict(n_dirs=c.n_dirs, reach=c.reach, flags=c.flags)
    args.update(kw)
    off, words = em.blocked_batch(c.x, c.y, c.z, c.r, c.so, mask, c.probe, c.n_points, **args)
    return off, words, mask


# ---- the classes of a pass ---------------------------------------------------------------------------------------------------

def test_pass_classes_mirror_the_kernels_choice_of_lanes():
    assert de.PASS == 128 and de.WAVE == 64 and len(de.CLASSES) == 16
    want = {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 8: 8, 9: 16, 16: 16, 17: 32, 32: 32, 33: 64, 64: 64, 65: de.TWO, 128: de.TWO}
    assert {n: de.lanes_of(n) for n in want} == want
    assert de.passes_of(0) == [] and de.passes_of(128) == [(False, de.TWO)]
    assert de.passes_of(129) == [(False, de.TWO), (True, 1)]
    assert de.passes_of(2049)[-1] == (True, 1) and len(de.passes_of(2049)) == 17
    assert de.pass_classes([3, 0, 300]) == {(False, 4), (False, de.TWO), (True, de.TWO), (True, 64)}
    assert [de.groups_of(P) for P in de.LANES] == [64, 32, 16, 8, 4, 2, 1, 1]


def test_the_first_suites_reach_no_later_pass_of_four_lanes_or_fewer():
    """What the cases of test_gpu_crowding.py / test_gpu_enclosure.py reach, each pinned: a change of a radius that moved a
    case to other classes would show here."""
    got = {c.name + str(c.n_points): de.pass_classes(cc.masks(c).sum(axis=1))
           for c in (cc.caps(), cc.lone(), cc.pair(), cc.of_depth("cavity"))}
    T = de.TWO
    assert got["caps65"] == {(False, T), (False, 1), (False, 64)}
    assert got["lone960"] == {(False, T), (True, T), (True, 64)}
    assert got["pair960"] == {(False, T), (True, T), (True, 8)}
    assert got["cavity100"] == {(False, P) for P in de.LANES if P != T}     # every group size, no later pass
    assert not set().union(*got.values()) & {(True, 1), (True, 2), (True, 4)}


# ---- A: lattices past 2048 points --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n_points", de.BIG)
def test_big_lattices_take_a_second_trip_over_the_masks_words(name, n_points):
    c = de.big(name, n_points)
    mask = cc.masks(c)
    words = -(-n_points // 32)
    assert words == {2049: 65, 4097: 129}[n_points] and -(-words // de.WAVE) == {2049: 2, 4097: 3}[n_points]
    free = mask.sum(axis=1)
    past = mask[:, de.TRIP_POINTS:].sum(axis=1)
    if name == "lone":
        assert free.tolist() == [2049] and past.tolist() == [1] and de.passes_of(2049)[-1] == (True, 1)
    else:
        # buried points on both sides of point 2048: the rank carried into a later trip is not the point number
        assert (past > 0).all() and (free - past > 0).all() and not mask[:, :de.TRIP_POINTS].all(axis=1).any()
        assert (free.tolist(), past.tolist()) == {2049: ([1601, 1661], [1, 1]), 4097: ([3197, 3327], [1454, 1801])}[n_points]
        assert (free > de.PASS).all()
        # a pass that starts in one trip and ends in the next: the early exit and the carry both decide its points
        rank_at_trip = (free - past)
        assert (rank_at_trip % de.PASS != 0).all()
    off, rows, _ = _crowding(c)
    assert len(rows) == int(free.sum()) and rows.any()
    e = ec.of(c)
    _, blocked, _ = _enclosure(e)
    if name == "lone":
        assert np.array_equal(blocked, em.own_bits(n_points, 30))
    else:
        assert (blocked & ~em.own_bits(n_points, 30)[np.nonzero(mask)[1]]).any()


# ---- B: every class of pass ----------------------------------------------------------------------------------------------------

def test_split_owners_reach_all_sixteen_classes():
    counts = de.split_counts()
    assert len(counts) == len(de.SPLIT_FIRST) + len(de.SPLIT_LATER)
    for t, n in zip(de.SPLIT_FIRST + de.SPLIT_LATER, counts):
        assert de.passes_of(n) == de.passes_of(t) and abs(n - t) <= 1, (t, n)
    assert {de.passes_of(n)[-1] for n in counts} == set(de.CLASSES)
    assert all(de.passes_of(n)[:-1] == [(False, de.TWO)] * (n > de.PASS) for n in counts)   # a later pass follows a full one
    # the group counts the cluster sizes are chosen against
    assert [n for n in de.SPLIT_CLUSTERS] == [3, 50, 70]


@pytest.mark.parametrize("n_cluster", de.SPLIT_CLUSTERS)
def test_split_structures_are_what_they_are_named_for(n_cluster):
    c = de.split(n_cluster)
    off, rows, mask = _crowding(c)
    e = ec.of(c, reach=de.SPLIT_REACH)
    _, words, _ = _enclosure(e)
    free = mask.sum(axis=1)
    owners = c.info["owners"]
    assert free[owners].tolist() == c.info["free"] == list(de.split_counts())     # the cluster buries none of their points
    assert (c.flags >> 1).any() and (c.flags[owners] & 1).all()
    own = em.own_bits(c.n_points, e.n_dirs)
    seen = {}
    for s, o in enumerate(owners):
        x, y, z, r = _part(c, s)
        assert len(x) == 2 + n_cluster and sm.margins_hold(x, y, z, r, c.probe)
        R = r + F(c.probe)
        d = np.sqrt(sum((a[2:].astype(np.float64) - float(a[0])) ** 2 for a in (x, y, z)))
        assert (d > (R[0] + R[2:]) + 0.1).all() and (d < 9.0).all()               # off the owner, inside the reach and the edges
        klass = de.passes_of(free[o])[-1]
        G = de.groups_of(klass[1])
        crowd, enclose = de.staged_batches(c, s), de.staged_batches(c, s, drop_owner=True)
        cover = int(c.flags[o + 1] & 1)
        assert cover == (n_cluster != 3) and sum(enclose) == n_cluster + cover and sum(crowd) == sum(enclose) + 1, (s, crowd)
        # the cluster sits in one staging step (the cover beside it or in a step of its own); the owner's cell holds the owner
        assert crowd[0] == 1 and max(enclose) in {3: (3,), 50: (50, 51), 70: (64,)}[n_cluster], (s, crowd, enclose)
        # the staging cut of k_dot_enclosure lets every one of them pass
        far = ((F(e.reach) + R[0]) + R[1:]) * em.SLACK
        dd = np.stack([x[1:] - x[0], y[1:] - y[0], z[1:] - z[0]])
        assert ((dd * dd).sum(axis=0) <= far * far).all()
        dots = slice(int(off[o]), int(off[o + 1]))
        kinds = seen.setdefault(klass, dict(G=G, crowd=[], enclose=[], rows=False, words=False))
        kinds["crowd"] += crowd
        kinds["enclose"] += enclose
        kinds["rows"] |= bool(rows[dots].any())
        kinds["words"] |= bool((words[dots] & ~own[np.flatnonzero(mask[o])]).any())
        # the last pass's dots themselves meet the cluster (the last points of the lattice are the cap's)
        last = slice(int(off[o + 1]) - (int(free[o]) - 1) % de.PASS - 1, int(off[o + 1]))
        assert rows[last].any() and (words[last] & ~own[np.flatnonzero(mask[o])][-(last.stop - last.start):]).any(), s
    assert set(seen) == set(de.CLASSES)
    for klass, k in seen.items():
        G = k["G"]
        assert k["rows"] and k["words"], klass
        if G >= 2:
            assert min(k["crowd"]) < G                                            # group 0 works alone: the other groups add 0
        if n_cluster == 3 and G >= 4:
            assert 3 in k["enclose"]                                              # fewer obstacles than groups
        if n_cluster == 3 and G == 2:
            assert 3 in k["enclose"]                                              # an odd count over two groups
        if (n_cluster == 50 and 2 <= G < 64) or (n_cluster == 70 and G in (2, 4)):
            assert any(n > G and n % G for n in k["enclose"]), (klass, k["enclose"])   # the groups' loops end unevenly
        if n_cluster == 50 and G == 64:
            assert max(k["enclose"]) < G
        if n_cluster == 70:
            assert 64 in k["enclose"] and min(k["enclose"]) < 8                   # a full staging batch and the rest of its step


# ---- C: the stop rules at their clamps --------------------------------------------------------------------------------------

def test_boundary_reaches_stop_where_they_are_named_for():
    assert [s for s, _, _ in de.boundary_reaches()] == [3, 3, 4, 4, 5, 5, 6, 6, 7, 7]
    for s, on, L in de.boundary_reaches():
        assert em.stop_shell(L, sc.H, 40, True) == (s if on else s + 1, True), (s, on)
    assert de.reach_of(sc.H, 3) == float(F(0.5) * sc.H)


@pytest.mark.parametrize("shell", cc.LAST_SHELLS)
def test_crowding_last_shell_at_every_shell(shell):
    c = cc.last_shell(shell)
    off, rows, mask = _crowding(c)
    x, y, z, r = _part(c)
    g = sm.grid(x, y, z, r, c.probe)
    assert sm.margins_hold(x, y, z, r, c.probe) and g.h == F(2.0) and c.edges[-1] == (shell - 1.5) * 2.0
    owners = np.array([c.info["hi"], c.info["lo"]])
    assert mask[owners].all()
    good, stop, by_rule, found = cm.sweep_counts(x, y, z, r, mask, c.probe, c.n_points, c.edges, None, owners)
    assert stop.tolist() == [shell] * 2 and by_rule.all() and all(shell in f for f in found)
    early, e_stop, _, _ = cm.sweep_counts(x, y, z, r, mask, c.probe, c.n_points, c.edges, None, owners, early=True)
    assert e_stop.tolist() == [shell - 1] * 2
    assert cm.stop_shell(c.edges[-1], g.h, 40, True) == (shell, True)
    assert cm.stop_shell(float(np.nextafter(F(c.edges[-1]), F(np.inf))), g.h, 40, True) == (shell + 1, True)
    lost = {int(o): 0 for o in owners}
    for owner, k, partner in c.info["ties"]:
        row = int(off[owner]) + k
        assert rows[row, -1] >= 1                                            # the tie counts in the last bin
        assert np.array_equal(good[owner][k], rows[row])
        gap = int(np.abs(g.cells[partner] - g.cells[owner]).max())
        assert gap in (shell, shell - 1)
        if gap == shell:                                                     # the side the owner leans to: in that shell and
            without = np.ones(c.n_atoms, np.uint8)                           # in no earlier one; it alone sets the count
            without[partner] = 0
            w_rows = cm.counts(x, y, z, r, mask, c.probe, c.n_points, c.edges, without)[1]
            assert rows[row, -1] == w_rows[row, -1] + 1                      # (at shell 3 the owner, 2 away, is in that bin too)
            assert early[owner][k, -1] == w_rows[row, -1]                    # one shell sooner loses it
            lost[owner] += 1
    assert sorted(lost.values()) == [3, 3]
    for o in owners:
        assert (early[int(o)] <= good[int(o)]).all()


@pytest.mark.parametrize("shell", ec.LAST_SHELLS)
def test_enclosure_last_shell_at_every_shell(shell):
    c = ec.last_shell(shell)
    off, words, mask = _enclosure(c)
    x, y, z, r = _part(c)
    g = sm.grid(x, y, z, r, c.probe)
    assert sm.margins_hold(x, y, z, r, c.probe) and g.h == F(2.0) and c.reach == (shell - 2.5) * 2.0
    owners = np.array([c.info["hi"], c.info["lo"]])
    assert mask[owners].all()
    got, stop, by_rule, shells = em.sweep_blocked(x, y, z, r, mask, c.probe, c.n_points, c.n_dirs, c.reach, None, owners)
    assert stop.tolist() == [shell] * 2 and by_rule.all()
    early, e_stop, e_rule, _ = em.sweep_blocked(x, y, z, r, mask, c.probe, c.n_points, c.n_dirs, c.reach, None, owners, early=True)
    assert e_stop.tolist() == [shell - 1] * 2 and e_rule.all()
    lost = {int(o): 0 for o in owners}
    for owner, k, m, obstacle in c.info["rays"]:
        n = owners.tolist().index(owner)
        bit = np.uint32(1) << np.uint32(m)
        assert np.array_equal(got[owner], words[int(off[owner]):int(off[owner + 1])])
        assert int(np.abs(g.cells[obstacle] - g.cells[owner]).max()) == shell      # its cell lies in that shell
        assert words[int(off[owner]) + k] & bit                                    # the ray is stopped,
        assert all((per[k] & bit) == 0 for s, per in shells[n].items() if s != shell)   # by that shell alone
        assert shells[n][shell][k] & bit
        assert em.own_bits(c.n_points, c.n_dirs)[k] & bit == 0
        without = np.ones(c.n_atoms, np.uint8)
        without[obstacle] = 0
        assert _enclosure(c, flags=without)[1][int(off[owner]) + k] & bit == 0     # and by that obstacle alone
        assert early[owner][k] & bit == 0                                          # one shell sooner loses it
        lost[owner] += 1
    assert sorted(lost.values()) == [3, 3]


def test_the_shell_3_clamp_is_the_half_cell_reach():
    """At shell 2 the rule's lim is -h / 2, whose square is a plausible bound: reach h / 2 passes it.  The clamp s >= 3
    keeps the sweep going; a rule clamped one shell low is `early`."""
    c = ec.last_shell(3)
    h = F(2.0)
    lim = (F(2.0) - F(2.5)) * h
    assert lim == -c.reach and F(c.reach) * F(c.reach) <= lim * lim
    assert em.stop_shell(c.reach, h, 40, True) == (3, True) and em.stop_shell(c.reach, h, 40, True, early=True) == (2, True)
    d = cc.last_shell(2)
    lim = (F(1.0) - F(1.5)) * h
    assert lim == -d.edges[-1] and F(d.edges[-1]) ** 2 <= lim * lim
    assert cm.stop_shell(d.edges[-1], h, 40, True) == (2, True) and cm.stop_shell(d.edges[-1], h, 40, True, early=True) == (1, True)


# ---- D: coordinates of 65536 h -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis,sign", de.MARGIN_MOVES)
@pytest.mark.parametrize("name", de.MOVED)
def test_moved_enclosure_cases_hold_the_margins_and_the_sweep_equals_the_model(name, axis, sign):
    c = de.moved_enclosure(name, axis, sign)
    off, words, mask = _enclosure(c)
    col = (c.x, c.y, c.z)[axis]
    for s in range(len(c.so) - 1):
        x, y, z, r = _part(c, s)
        b = int(c.so[s])
        assert sm.margins_hold(x, y, z, r, c.probe)
        two_steps = 2 * float(np.spacing(F(131072.0)))                   # (one step may round back onto the same floats)
        assert not sm.margins_hold(*sc._moved(np.stack([x, y, z], -1), axis, sign, two_steps).T, r, c.probe)
        owners = np.array([2]) if name == "prefilter_edge" else np.array([c.info["hi"], c.info["lo"]])
        got = em.sweep_blocked(x, y, z, r, mask[b:b + len(x)], c.probe, c.n_points, c.n_dirs, c.reach, None, owners)[0]
        for o in owners:
            assert np.array_equal(got[int(o)], words[int(off[b + o]):int(off[b + o + 1])]), (s, int(o))
    assert np.abs(col).max() > 65536.0 * 2.0 - 200.0 and float(np.spacing(F(np.abs(col).max()))) >= 2.0 / 256
    own = em.own_bits(c.n_points, c.n_dirs)[np.nonzero(mask)[1]]
    assert (words & ~own).any()


@pytest.mark.parametrize("axis,sign", de.MARGIN_MOVES)
@pytest.mark.parametrize("kind", ["last", "below"])
def test_moved_ties_are_exact_again(kind, axis, sign):
    c = de.moved_tie(kind, axis, sign)
    x, y, z, r = _part(c)
    assert sm.margins_hold(x, y, z, r, c.probe) and np.abs((x, y, z)[axis]).max() > 65536.0 * 3.1 - 200.0
    off, rows, mask = _crowding(c)
    assert mask[0, cc.TIE_DOT]
    rank = de.rank_of(mask[0], cc.TIE_DOT)
    _, qx, qy, qz = (a[rank] for a in dm.dots_of(x, y, z, r, mask, c.probe, c.n_points))
    dx, dy, dz = x[1] - qx, y[1] - qy, z[1] - qz
    d2 = dx * dx + dy * dy + dz * dz
    e2 = cm.e2_of(c.edges)
    assert d2.dtype == F and dy == 0 and dz == 0
    row = rows[int(off[0]) + rank]
    if kind == "last":
        assert e2[-1] == d2 and row.tolist() == [1, 1]                       # the owner in bin 0, the partner ON the last edge
    else:
        assert e2[-1] < d2 and np.nextafter(F(c.edges[-1]), F(np.inf)) ** 2 == d2 and row.tolist() == [1, 0]


def test_the_staging_cuts_absolute_term_keeps_a_bit_that_the_relative_slack_loses():
    """The search over ABS_SEEDS (dot_edge_cases.abs_search) pinned: seed 514 is the first whose structure, under the
    margins at z of about 65536 h, loses a bit of the model when the staging cut is taken without its h / 64."""
    assert de.ABS_SEEDS == tuple(range(500, 540)) and de.abs_search() == de.ABS_SEED == 514
    c = de.abs_candidate(de.ABS_SEED)
    want, full, bare = de.abs_lost(c)
    assert np.array_equal(want, full)                                        # the cut as built loses nothing
    assert (want & ~bare).any() and (bare & ~want == 0).all() and want[0] & 1 and not bare[0] & 1   # dot 0, ray 0
    x, y, z, r = _part(c)
    h = float(F(c.probe) + r.max())
    assert sm.margins_hold(x, y, z, r, c.probe) and abs(c.reach - 0.5 * h) < 1e-6
    assert float(np.spacing(z[0])) >= h / 256 and z.min() > 131072.0
    R = r.astype(np.float64) + c.probe
    d = float(z[1]) - float(z[0])
    full_reach = c.reach + R[0] + R[1]
    assert full_reach * (1 + 2.0 ** -10) < d <= full_reach * (1 + 2.0 ** -10) + h / 64   # between the two cuts
    without = np.array([1, 0, 1, 1], np.uint8)
    assert _enclosure(c, flags=without)[1][0] & 1 == 0                        # that obstacle alone stops the ray
