"""The two proofs that let k_atom_depth (depth.hip) and k_component_link (components.hip) cut their shell sweep short,
checked without a GPU on real float32 numbers: the emulation of the sweep (sweep_model.py: shells, runs, stop rule,
margins test and reach as the kernels form them) against the brute-force models (depth_model.py, components_model.py),
on the cases of sweep_cases.py, on the small cases of depth_cases.py and component_cases.py (all but `tail` and
`example_vdw`, of 65 536 and 2 622 atoms), and on RANDOM_STRUCTURES = 2500 seeded random structures of 2 to 12 atoms that
sit next to cell borders and next to the 65536 h limit of the margins.  Then every case of sweep_cases.py is pinned to what
it is named for, from the emulation alone, and every switch of the emulation - one way a kernel could be wrong each - is
shown to change a result on a named case: the cases bite."""
import functools

import numpy as np
import pytest

import component_cases as cc
import components_model as cm
import depth_cases as dc
import depth_model as dm
import point_edge_cases as pe
import points_model as pm
import sweep_cases as sc
import sweep_model as sm

F = np.float32
RANDOM_STRUCTURES = 2500
OTHER_RUNS = [(n, 100) for n in dc.SMALL] + [("pole_tie", 1), ("far_link", cc.FAR_POINTS), ("multi_chunk", 129)]
ALL_RUNS = sc.runs() + OTHER_RUNS


def _case(name):
    return sc.get(name) if name in sc.CASES else cc.get(name)


@functools.lru_cache(maxsize=None)
def _masks(name, n_points):
    c = _case(name)
    return pm.exposed_masks_batch(*c.cols, c.so, c.probe, n_points, 8)


@pytest.fixture(scope="module", autouse=True)
def _all_masks():
    pe.pmap(lambda run: _masks(*run), ALL_RUNS)      # side by side, once


def _parts(name, n_points):
    """[(s, x, y, z, r, mask)] of the structures of a case that hold atoms."""
    c, mask = _case(name), _masks(name, n_points)
    return [(s,) + c.part(s)[:4] + (mask[int(c.so[s]):int(c.so[s + 1])],) for s in range(len(c.so) - 1) if c.so[s + 1] > c.so[s]]


@functools.lru_cache(maxsize=None)
def _sweeps(name, n_points):
    """{structure: (Sweep, Grid)} with the kernel's own rule."""
    c = _case(name)
    return {s: sm.sweep_depth(x, y, z, r, m, c.probe, n_points) for s, x, y, z, r, m in _parts(name, n_points)}


def _link(c, s, n_points):
    return cc.default_link(c.part(s)[3], c.probe, n_points)


# ---- agreement with brute force ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n_points", ALL_RUNS)
def test_the_sweep_holds_the_brute_force_key(name, n_points):
    """The stop-rule proof on real numbers: the key the emulated sweep ends with is depth_model.keys_of's, bit for bit,
    for every atom; and the per-owner table the emulation looks its keys up in reduces to the same keys."""
    c = _case(name)
    for s, x, y, z, r, m in _parts(name, n_points):
        want = dm.keys_of(x, y, z, r, m, c.probe, n_points)
        assert np.array_equal(sm.pair_keys(x, y, z, r, m, c.probe, n_points).min(axis=1), want), (name, s)
        sw, g = _sweeps(name, n_points)[s]
        bad = np.flatnonzero(sw.keys != want)
        assert bad.size == 0, (name, s, bad[:5], sw.stop[bad[:5]])
        held = sw.keys != dm.NONE_KEY
        win = (sw.keys[held] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        shell = np.abs(g.cells[win] - g.cells[np.flatnonzero(held)]).max(axis=1)
        assert np.array_equal(sw.found[held], shell)                  # found in the shell its cell lies in


def test_one_spare_shell_is_enough_in_these_cases():
    """stop_shift = 1 is exact in exact arithmetic as well: an unseen atom's nearest dot is at least (s - 1) h away, so
    the rule `best_d2 <= ((s - 2) h)^2` carries a full spare shell, of which the roundings at the margins' limit use a
    quarter.  No counterexample is hunted for; this records that none shows on the cases at the limit, nor (below) in
    the random search."""
    for name in ("margin_under", "margin_small_h", "column_z"):
        c = _case(name)
        n_points = sc.points_of(name)[0]
        for s, x, y, z, r, m in _parts(name, n_points):
            got = sm.sweep_depth(x, y, z, r, m, c.probe, n_points, stop_shift=1)[0]
            assert np.array_equal(got.keys, _sweeps(name, n_points)[s][0].keys), (name, s)


# ---- the reach -------------------------------------------------------------------------------------------------------------------

def _reach_misses(x, y, z, r, mask, probe, n_points, link, **kw):
    """The atom pairs that carry an edge of the model and lie outside the reach; and how many carry one."""
    _, _, _, edges, owner = cm.components(x, y, z, r, None, probe, n_points, link, mask=mask, with_edges=True)
    pairs, ends, g = sm.reach_pairs(x, y, z, r, probe, link, **kw)
    need = sm.edge_atom_pairs(g, edges, owner)
    return need - pairs, len(need), ends


@pytest.mark.parametrize("name,n_points", ALL_RUNS)
def test_every_edge_of_the_model_lies_within_the_reach(name, n_points):
    c = _case(name)
    for s, x, y, z, r, m in _parts(name, n_points):
        links = [_link(c, s, n_points)]
        if name in ("far_link", "half_link"):
            links = [cc.H if name == "far_link" else sc.HALF_LINK]
        if name == "crowded_cells":
            links += [F(0.0), F(4.0) * (F(c.probe) + np.max(r))]
        for link in links:
            missed = _reach_misses(x, y, z, r, m, c.probe, n_points, link)[0]
            assert not missed, (name, s, link, sorted(missed)[:5])


# ---- a seeded random search next to cell borders and next to the limit ----------------------------------------------------------

def _random_structure(rng):
    """2 to 12 atoms on the corners of the cell lattice, each a hair to a twentieth of a cell off its border, the whole
    translated along one axis so that fabsf(min) + dim * h lies within a few cells under 65536 h (or, one time in eight,
    left near the origin); a random mask at 12 points, a random link up to 2 h."""
    n = int(rng.integers(2, 13))
    r = rng.choice(dc.RADII, n).astype(F)
    probe = float(rng.choice([1.4, 0.0, 0.5]))
    h = float(F(probe) + r.max())
    k = rng.integers(0, 7, (n, 3)) * np.array([1, rng.integers(0, 2), rng.integers(0, 2)])   # long on x, flat or not on y, z
    off = rng.choice([-1.0, 1.0], (n, 3)) * h * 10.0 ** rng.uniform(-6.0, -1.3, (n, 3))
    xyz = (k * h + off).astype(F)
    if rng.integers(0, 8):
        axis, sign = int(rng.integers(0, 3)), float(rng.choice([-1.0, 1.0]))
        t = 65536.0 * h - rng.uniform(7.0, 12.0) * h
        xyz[:, axis] = xyz[:, axis] + F(sign * t)
        a, lim = sm.margin_sums(*xyz.T, r, probe)
        gap = max(0.0, float(lim) - float(a.max()) - rng.integers(0, 4) * float(np.spacing(lim)))
        xyz[:, axis] = xyz[:, axis] + F(sign * gap)            # close the rest of the gap, to a few ulps under the limit
    mask = rng.random((n, 12)) < 0.4
    mask[rng.integers(0, n)] = True
    return tuple(np.ascontiguousarray(xyz[:, k]) for k in range(3)) + (r, mask, probe, F(rng.uniform(0.0, 2.0) * h))


def _brute_edges(x, y, z, r, mask, probe, n_points, link):
    owner, qx, qy, qz = dm.dots_of(x, y, z, r, mask, probe, n_points)
    dx, dy, dz = qx[:, None] - qx[None, :], qy[:, None] - qy[None, :], qz[:, None] - qz[None, :]
    d2 = dx * dx + dy * dy + dz * dz
    assert d2.dtype == F
    a, b = np.nonzero(np.triu(d2 <= F(link) * F(link), 1))
    return np.stack([a, b], -1), owner


def test_random_structures_next_to_cell_borders_and_the_limit():
    """RANDOM_STRUCTURES structures (see the head of the file): the sweep's key is the brute-force key with the kernel's
    rule AND with one spare shell less, and every edge (all dot pairs, by the float32 test) lies within the reach."""
    rng = np.random.default_rng(81)
    hold = shift1 = stopped = edges_seen = 0
    for n in range(RANDOM_STRUCTURES):
        x, y, z, r, mask, probe, link = _random_structure(rng)
        want = dm.keys_of(x, y, z, r, mask, probe, 12)
        sw, g = sm.sweep_depth(x, y, z, r, mask, probe, 12)
        assert np.array_equal(sw.keys, want), (n, x, y, z, r)
        hold += sm.margins_hold(x, y, z, r, probe)
        stopped += int(sw.by_rule.sum())
        shift1 += int((sm.sweep_depth(x, y, z, r, mask, probe, 12, stop_shift=1)[0].keys != want).sum())
        edges, owner = _brute_edges(x, y, z, r, mask, probe, 12, link)
        pairs, _, g = sm.reach_pairs(x, y, z, r, probe, link)
        need = sm.edge_atom_pairs(g, edges, owner)
        assert need <= pairs, (n, sorted(need - pairs)[:5], link)
        edges_seen += len(need)
    assert hold >= RANDOM_STRUCTURES // 2 and stopped >= RANDOM_STRUCTURES and edges_seen >= RANDOM_STRUCTURES
    assert shift1 == 0          # (a failure here would be the sharpest input there is: pin it as a case)


# ---- the margins ---------------------------------------------------------------------------------------------------------------

def test_margins_classification():
    under, over = sc.get("margin_under"), sc.get("margin_over")
    for n, (axis, sign) in enumerate(sc.DIRECTIONS):
        u, o = under.part(n)[:4], over.part(n)[:4]
        assert sm.margins_hold(*u, under.probe) and not sm.margins_hold(*o, over.probe), (axis, sign)
        a, lim = sm.margin_sums(*u, under.probe)
        assert int(np.argmax(a)) == axis and float(lim) - float(a[axis]) <= 2.0 * float(np.spacing(lim))    # just under
        a, lim = sm.margin_sums(*o, over.probe)
        assert 0.0 < float(a[axis]) - float(lim) <= 2.0 * float(np.spacing(lim))                              # just over
        assert np.sign(u[axis][0]) == sign and abs(float(u[axis][0])) > 2.1e5 and float(np.spacing(np.abs(u[axis][0]))) == 1.0 / 64.0
        assert not sm.odd_input(*o)                             # it is the coordinates' size that fails, nothing else
    twelve = sc.get("margin_twelve")
    assert [sm.margins_hold(*twelve.part(s)[:4], twelve.probe) for s in range(12)] == [True, False] * 6
    small = sc.get("margin_small_h")
    for s in range(3):
        p = small.part(s)[:4]
        a, lim = sm.margin_sums(*p, small.probe)
        assert sm.margins_hold(*p, small.probe) and float(lim) - float(a.max()) <= 2.0 * float(np.spacing(lim))
        assert 0.09 < float(np.max(p[3])) < 0.1 and 6.0e3 < float(np.abs(np.stack(p[:3])).max()) < 6.6e3
    large = sc.get("margin_large_h")
    assert sm.margins_hold(*large.part(0)[:4], large.probe) and F(large.probe) + large.r.max() == F(40.0)
    odd = sc.get("odd_beside_even")
    assert [sm.margins_hold(*odd.part(s)[:4], odd.probe) for s in range(3)] == [True, False, False]
    assert [sm.odd_input(*odd.part(s)[:4]) for s in range(3)] == [False, True, True]
    assert np.max(odd.part(1)[3]) == np.max(odd.part(0)[3])     # the negative radius leaves max_r alone


def test_the_margin_cases_stop_early_or_sweep_everything():
    for name, early in (("margin_under", True), ("margin_over", False)):
        for s, (sw, g) in _sweeps(name, 100).items():
            last = np.array([g.s_last(i) for i in range(len(sw.keys))])
            assert tuple(g.dims) == (8, 8, 8)
            if early:
                assert sw.by_rule.sum() >= 200 and (sw.stop[sw.by_rule] < last[sw.by_rule]).all() and {3, 4} <= set(sw.stop.tolist())
            else:
                assert not sw.by_rule.any() and np.array_equal(sw.stop, last) and sw.stop.max() >= 6
    sweeps = _sweeps("odd_beside_even", 100)
    assert sweeps[0][0].by_rule.sum() >= 800 and not sweeps[1][0].by_rule.any() and not sweeps[2][0].by_rule.any()
    assert sweeps[1][0].stop.max() >= 9 and _case("odd_beside_even").n_atoms == 3 * 925


# ---- the cases are what they are named for ----------------------------------------------------------------------------------

def test_column_z():
    c = sc.get("column_z")
    mask = _masks("column_z", 1)
    n = sc.COLUMN_ATOMS
    assert mask.shape[1] == 1 and np.flatnonzero(mask[:n, 0]).tolist() == [n - 1]          # one dot, on the top atom
    owner, qx, qy, qz = dm.dots_of(*c.part(0)[:4], mask[:n], c.probe, 1)
    assert qx[0] == 0.0 and qy[0] == 0.0 and qz[0] == c.z[n - 1] + (c.r[n - 1] + F(c.probe))   # the exact +z pole
    sw, g = _sweeps("column_z", 1)[0]
    assert tuple(g.dims) == (3, 3, 25)
    depth = dm.split(sw.keys)[1]
    assert 22.0 < depth[0] / g.h < 23.0
    long_ = np.flatnonzero((sw.stop >= 20) & ~sw.by_rule)
    assert long_.size >= 1 and sw.stop.max() >= 23
    for i in long_:                                                                  # x and y clipped on both sides
        s, kind, faces = sm.position_class(g, i, n - 1)
        assert s >= 15 and kind == "rim" and {"x-", "x+", "y-", "y+"} <= set(faces)
        assert all(len(np.concatenate(sm.shell_steps(g, i, t)[0])) <= 9 * 3 for t in range(2, s + 1))
    # the second column: the grid goes on past the top dot, sweeps end by the rule at a large s
    sw2, g2 = _sweeps("column_z", 1)[1]
    assert np.flatnonzero(mask[n:, 0]).tolist() == [n - 1, n + sc.COLUMN_EXTRAS - 1, n + sc.COLUMN_EXTRAS, n + sc.COLUMN_EXTRAS + 1]
    assert (sw2.by_rule & (sw2.stop >= 8)).sum() >= 10 and g2.dims[2] > 25


@pytest.mark.parametrize("axis,sign", [(0, 1), (0, -1), (1, 1), (1, -1)])
def test_slants(axis, sign):
    """Along x the last atom - the only one with a dot - lies for the low atoms in a row INSIDE the shell's square, in
    its high (+) or low (-) cell, at s >= 5.  The kernel has such cells only along x: along y the same atom lies in a rim
    row at |dy| = s, whose x-run is clipped on both sides (the grid is 3 cells wide there)."""
    name = sc.SLANT_NAMES[(axis, sign)]
    mask = _masks(name, 1)
    last = sc.SLANT_ATOMS - 1
    assert np.flatnonzero(mask[:, 0]).tolist() == [last]
    sw, g = _sweeps(name, 1)[0]
    assert g.dims[1 - axis] == 3 and g.dims[axis] >= 15
    low = np.arange(20)
    assert ((sw.keys[low] & np.uint64(0xFFFFFFFF)) == last).all()
    for i in low:
        s, kind, faces = sm.position_class(g, i, last)
        assert s >= 5 and s == abs(int(g.cells[last, axis] - g.cells[i, axis]))
        if axis == 0:
            assert kind == ("inside-high" if sign > 0 else "inside-low")
        else:
            assert kind == "rim" and {"x-", "x+"} <= set(faces)
    assert sw.stop.max() >= 14 and sw.by_rule.any() and (~sw.by_rule).any()


def test_crowded_cells():
    sw, g = _sweeps("crowded_cells", 100)[0]
    assert g.h == F(21.4) and sw.longest_run > sm.WAVE
    ball = g.cells[:-1]
    cells, count = np.unique(ball, axis=0, return_counts=True)
    assert len(cells) == 8 and count.min() >= 90 and (cells.max(axis=0) - cells.min(axis=0) == 1).all()
    # the cut `q <= p` inside a cell's run and inside a 64-atom staging batch: atoms kept and atoms dropped in one batch
    idx = g.cells[:, 0] + g.cells[:, 1] * g.dims[0] + g.cells[:, 2] * g.dims[0] * g.dims[1]
    f = g.pos - g.starts[idx]                                   # place in the own cell's run (shell 0, one run)
    length = g.starts[idx + 1] - g.starts[idx]
    free = _masks("crowded_cells", 100).any(axis=1)
    inside = free & (f % sm.WAVE != sm.WAVE - 1) & (f + 1 < length) & (f >= sm.WAVE)
    assert inside.sum() >= 50
    # the far atom buries nothing and is buried by nothing
    assert _masks("crowded_cells", 100)[-1].all()
    assert np.array_equal(_masks("crowded_cells", 100)[:-1], _masks("ball", 100))
    assert _masks("crowded_cells", 65)[:-1].any(axis=1).sum() >= 200     # own dots in two chunks at 65 points


def test_chain():
    c = sc.get("chain")
    off, labels, mask = cm.components(*c.cols, c.probe, 100, _link(c, 0, 100), mask=_masks("chain", 100))
    assert not labels.any() and mask.any(axis=1).all() and c.n_atoms == 384          # one component of every atom
    place = c.info["place"]
    assert off[1] > 0 and (place[0] < 38 or place[0] >= 384 - 38)                       # dot 0 is on an atom of the outer tenth
    g = sm.grid(*c.cols[:4], c.probe)
    assert g.dims[0] >= 240 and tuple(g.dims[1:]) == (3, 3)
    assert np.abs(np.diff(g.pos[:64])).mean() > 50.0                                   # input order against cell order


# ---- the cases bite -----------------------------------------------------------------------------------------------------------

def _changed(name, n_points, s, **switches):
    c = _case(name)
    _, x, y, z, r, m = [p for p in _parts(name, n_points) if p[0] == s][0]
    got = sm.sweep_depth(x, y, z, r, m, c.probe, n_points, **switches)[0]
    return int((got.keys != _sweeps(name, n_points)[s][0].keys).sum())


def test_a_stop_rule_without_its_spare_shells_loses_a_key_on_column_z():
    assert _changed("column_z", 1, 1, stop_shift=0) >= 1
    assert _changed("column_z", 1, 1, stop_shift=1) == 0        # (see test_one_spare_shell_is_enough_in_these_cases)


def test_dropping_the_inside_cells_loses_keys_on_the_matching_slant():
    assert _changed("slant_xp", 1, 0, drop_hi=True) >= 20
    assert _changed("slant_xm", 1, 0, drop_lo=True) >= 20


def test_reading_only_a_shell_s_first_64_rows_loses_keys_on_the_turned_ball():
    """Shell 4 has 81 rows in the middle of the grid.  In `ball` itself the few winners of shell 4 lie at dz = 0, among the
    first 64 rows, and the switch changed nothing there when this was written (an accident of its seed, not
    asserted); in the ball turned by a quarter they lie in the last rows."""
    sw, g = _sweeps("ball_turned", 100)[0]
    assert sw.found.max() >= 4 and tuple(g.dims) == (11, 11, 11)
    assert _changed("ball_turned", 100, 0, rows_first_step_only=True) >= 1


def test_reading_only_a_step_s_first_64_atoms_loses_keys_on_crowded_cells():
    assert _changed("crowded_cells", 100, 0, atoms_first_step_only=True) >= 1


def test_a_reach_one_shell_short_loses_edges_on_far_link_and_half_link():
    """far_link: cells 3 apart at link = h; the pair's later atom stands in cell 3 of 6, so its sweep ends with the grid
    at shell 3 (S would be 4).  half_link: cells 3 apart at link = h / 2, where S = 3 is the smallest integer with
    (S - 2.5) h >= link and the grid goes on beyond it: the reach itself is what must not be one shorter."""
    c = sc.get("half_link")
    for s, x, y, z, r, m in _parts("half_link", cc.FAR_POINTS):
        assert m.all()
        pairs, ends, g = sm.reach_pairs(x, y, z, r, c.probe, sc.HALF_LINK)
        later = 0 if g.pos[0] > g.pos[1] else 1
        assert ends[later] == 3 and g.s_last(later) >= 4 and sm.margins_hold(x, y, z, r, c.probe)
        missed, n_need, ends = _reach_misses(x, y, z, r, m, c.probe, cc.FAR_POINTS, sc.HALF_LINK, reach_shift=-1)
        assert missed == {(later, 1 - later)} and n_need == 4 and ends[later] == 2, s
    c = cc.get("far_link")
    for s, x, y, z, r, m in _parts("far_link", cc.FAR_POINTS):
        missed, n_need, ends = _reach_misses(x, y, z, r, m, c.probe, cc.FAR_POINTS, cc.H, reach_shift=-1)
        assert len(missed) == 1 and n_need == 3, s


def test_half_link_pairs():
    pairs = sc.half_link_pairs()
    assert [p[:2] for p in pairs] == sc.DIRECTIONS
    c = sc.get("half_link")
    for n, (axis, sign, base, dist, off) in enumerate(pairs):
        assert 2.5 * float(cc.H) - 0.25 <= dist < 2.5 * float(cc.H)
        for swap in (0, 1):
            part = c.part(2 * n + swap)
            assert cc._cell_gap(part, axis) == 3 and sc.cross_edges(part, sc.HALF_LINK) >= 1
