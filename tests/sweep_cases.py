"""The inputs of the sweep-edge tests (test_sweep_cpu.py, test_gpu_sweep_edges.py), each named for what it reaches in
the Chebyshev shell sweep that k_atom_depth (depth.hip) and k_component_link (components.hip) share: the stop rule, the
reach, and the margins test that decides per structure whether either may cut the sweep short.  Built with
depth_cases._case, so they drop into both families' checks.  Seeded and small (under about 1000 atoms a structure);
test_sweep_cpu.py pins every case to what it is named for from the emulation (sweep_model.py) alone.  Plain helper module
(not a conftest)."""
import functools

import numpy as np

import component_cases as cc
import depth_cases as dc
import sweep_model as sm

F = np.float32
PROBE = dc.PROBE
H = F(PROBE) + dc.RADII.max()          # 3.28: the cell size of every ProtOr case here
COLUMN_ATOMS = 48
COLUMN_SPACING = 1.5                   # A
COLUMN_RADII = np.array([1.76, 1.88], F)
DIRECTIONS = cc.DIRECTIONS             # (axis, sign): +x, -x, +y, -y, +z, -z


def _part(xyz, r):
    return dc._cols(np.ascontiguousarray(xyz, F), np.ascontiguousarray(r, F))


# ---- column_z: 24 shells through a grid 3 cells wide on two axes ----------------------------------------------------------

def _column(n, rng):
    xyz = np.zeros((n, 3))
    xyz[:, 2] = np.arange(n) * COLUMN_SPACING
    r = rng.choice(COLUMN_RADII, n)
    r[:2] = COLUMN_RADII                 # both radii are there: h = 3.28
    return xyz, r


# the second column's extra atoms, relative to its bottom atom: six that carry the column on beyond its top, displaced
# sideways out of cover of the top atom's pole, and three decoys around the bottom atom found by a seeded scan (see
# column_z): A beside it, B below it, C below B.
COLUMN_EXTRA_DX = 4.0
COLUMN_EXTRAS = 6
COLUMN_DECOYS = ((8.15, 0.0, -3.1), (0.0, 0.0, -10.4), (0.0, 0.0, -13.4))


@functools.lru_cache(maxsize=None)
def column_z():
    """Two structures, run at ONE lattice point, which is exactly (0, 0, 1): an atom's only point is its +z pole.
    0: a straight column of 48 atoms along +z, 1.5 A apart.  Every pole but the top atom's lies inside the next atom:
       one accessible dot.  The grid is 3 x 3 x 25; the sweeps of the low atoms run 20 and more shells with x and y
       clipped on both sides from shell 2 on, 9 rows a shell, and end where the shells cover the grid.
    1: the same column, six atoms more beyond its top, displaced sideways out of the top atom's pole, and three decoys at
       its foot: the grid goes on past the top dot, so sweeps end by the stop rule at large s; the decoys put a dot (B's)
       one shell beyond where a stop rule without its two spare shells would end the bottom atom's sweep."""
    rng = np.random.default_rng(31)
    xyz, r = _column(COLUMN_ATOMS, rng)
    top = xyz[-1]
    extra = top + np.stack([np.full(COLUMN_EXTRAS, COLUMN_EXTRA_DX), np.zeros(COLUMN_EXTRAS),
                            (1 + np.arange(COLUMN_EXTRAS)) * COLUMN_SPACING], -1)
    decoys = np.array(COLUMN_DECOYS)
    xyz2 = np.concatenate([xyz, extra, decoys])
    r2 = np.concatenate([r, rng.choice(COLUMN_RADII, COLUMN_EXTRAS), np.full(len(decoys), COLUMN_RADII[1])])
    return dc._case("column_z", [_part(xyz, r), _part(xyz2, r2)])


# ---- slant_*: the winner in an inside row's low / high cell (x) or in a clipped rim run (y), at large s ----------------------
# The kernels' rows are (y, z) and only x has inside cells: slant_xp / slant_xm reach the high / low one; slant_yp / slant_ym
# cannot - their winner lies in a rim row at |dy| = s whose x-run is clipped at both faces - and are named for their axis only.

SLANT_ATOMS = 40
SLANT_A, SLANT_C = 0.8, 0.6            # the direction (a, c): a > c > 0
SLANT_NAMES = {(0, 1): "slant_xp", (0, -1): "slant_xm", (1, 1): "slant_yp", (1, -1): "slant_ym"}


@functools.lru_cache(maxsize=None)
def slant(axis, sign):
    """A column of 40 atoms 1.5 A apart along (+-a, 0, c) (axis 0) or (0, +-a, c) (axis 1), a = 0.8, c = 0.6, run at ONE
    lattice point: the pole of every atom lies inside the next atom up the slant (1.5 < 2 R c), so only the last atom has
    a dot, and for the low atoms it lies many cells away along the axis and fewer along z."""
    rng = np.random.default_rng(41 + 2 * axis + (sign < 0))
    step = np.zeros(3)
    step[axis], step[2] = sign * SLANT_A, SLANT_C
    xyz = np.arange(SLANT_ATOMS)[:, None] * COLUMN_SPACING * step[None, :] + np.array([3.0, -2.0, 1.0])
    r = rng.choice(COLUMN_RADII, SLANT_ATOMS)
    r[:2] = COLUMN_RADII
    return dc._case(SLANT_NAMES[(axis, sign)], [_part(np.round(xyz, 3), r)])


# ---- the margins: just under and just over 65536 h ------------------------------------------------------------------------

MARGIN_BALL_RADIUS = 8.0
MARGIN_VOID_CENTRE = np.array([1.0, 0.0, -1.0])
MARGIN_VOID_RADIUS = 3.0


@functools.lru_cache(maxsize=None)
def small_ball():
    """The `ball` recipe at radius 8 A with a void: (xyz float64 rounded to 1e-3, r)."""
    rng = np.random.default_rng(51)
    n = int(MARGIN_BALL_RADIUS // dc.SPACING)
    g = np.arange(-n, n + 1) * dc.SPACING
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    xyz = xyz[np.linalg.norm(xyz, axis=1) <= MARGIN_BALL_RADIUS]
    xyz = xyz[np.linalg.norm(xyz - MARGIN_VOID_CENTRE, axis=1) > MARGIN_VOID_RADIUS]
    xyz = xyz + rng.uniform(-dc.JITTER, dc.JITTER, xyz.shape)
    xyz = xyz[rng.permutation(len(xyz))]
    r = rng.choice(dc.RADII, len(xyz)).astype(F)
    r[:len(dc.RADII)] = dc.RADII         # the largest radius is there
    return np.round(xyz, 3), r


def _moved(xyz, axis, sign, t):
    """float32 coordinates of xyz translated by sign * t along the axis: the sum is taken in float32."""
    out = np.ascontiguousarray(xyz, F).copy()
    out[:, axis] = out[:, axis] + F(sign * t)
    assert out.dtype == F
    return out


def _edge_shift(xyz, r, probe, axis, sign):
    """(under, over): the largest translation on the grid of `step` (the coordinate ulp at the limit) for which the
    structure passes sm.margins_hold, and that plus one step, for which it fails; found by bisection and checked."""
    h = float(F(probe) + np.max(r))
    step = float(np.spacing(F(65536.0 * h)))
    held = lambda k: sm.margins_hold(*_moved(xyz, axis, sign, k * step).T, r, probe)  # noqa: E731
    lo, hi = int((65536.0 * h - 64.0 * h) / step), int(65536.0 * h / step)
    assert held(lo) and not held(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if held(mid):
            lo = mid
        else:
            hi = mid
    return lo * step, hi * step


@functools.lru_cache(maxsize=None)
def margin_shifts():
    xyz, r = small_ball()
    return {d: _edge_shift(xyz, r, PROBE, *d) for d in DIRECTIONS}


@functools.lru_cache(maxsize=None)
def margin(which):
    """which "under" / "over": the small ball translated in float32 along each axis and sign so that fabsf(min) + dim * h
    lands just under / just over 65536 h (about 2.15e5 A, coordinate ulp 1/64 A): six structures in DIRECTIONS order."""
    xyz, r = small_ball()
    sh = margin_shifts()
    parts = [_part(_moved(xyz, *d, sh[d][which == "over"]), r) for d in DIRECTIONS]
    return dc._case("margin_" + which, parts)


@functools.lru_cache(maxsize=None)
def margin_twelve():
    u, o = margin("under"), margin("over")
    parts = [c.part(s)[:4] + (None,) for s in range(6) for c in (u, o)]     # under, over, under, over, ...
    return dc._case("margin_twelve", parts)


@functools.lru_cache(maxsize=None)
def margin_pair(n):
    u, o = margin("under"), margin("over")
    return dc._case("margin_pair%d" % n, [u.part(n)[:4] + (None,), o.part(n)[:4] + (None,)])


SMALL_H_SCALE = 0.03


@functools.lru_cache(maxsize=None)
def margin_small_h():
    """The small ball scaled by 0.03 at probe 0: radii 0.085 to 0.098, h about 0.098, translated along +x, -y and +z to
    just under 65536 h (about 6.4e3, coordinate ulp 2^-11 = h / 200)."""
    xyz, r = small_ball()
    xyz_s = np.round(xyz * SMALL_H_SCALE, 5)
    r_s = ((r.astype(np.float64) + PROBE) * SMALL_H_SCALE).astype(F)
    parts = [_part(_moved(xyz_s, *d, _edge_shift(xyz_s, r_s, 0.0, *d)[0]), r_s) for d in ((0, 1), (1, -1), (2, 1))]
    return dc._case("margin_small_h", parts, probe=0.0)


LARGE_H_SCALE = 40.0 / float(H)


@functools.lru_cache(maxsize=None)
def margin_large_h():
    """The small ball scaled so that h = 40 at probe 10 (radii 24.4 to 30), at the origin."""
    xyz, r = small_ball()
    r_s = ((r.astype(np.float64) + PROBE) * LARGE_H_SCALE - 10.0).astype(F)
    return dc._case("margin_large_h", [_part(np.round(xyz * LARGE_H_SCALE, 2), r_s)], probe=10.0)


# ---- one structure that stops early beside two that must sweep everything ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def odd_beside_even():
    """`ball` three times in one batch: as it is; with one surface atom's radius at -0.25 (odd_radii bit 0, max_r
    unchanged); with one surface atom's radius at 64.5.  info["odd"]: that atom."""
    b = dc.ball()
    x, y, z, r, _ = b.part(0)
    odd = int(np.argmax(x.astype(np.float64) ** 2 + y.astype(np.float64) ** 2 + z.astype(np.float64) ** 2))
    neg, big = r.copy(), r.copy()
    neg[odd], big[odd] = -0.25, 64.5
    return dc._case("odd_beside_even", [(x, y, z, r, None), (x, y, z, neg, None), (x, y, z, big, None)], odd=odd)


# ---- a hundred atoms a cell ------------------------------------------------------------------------------------------------

CROWDED_POINTS = (100, 65)


@functools.lru_cache(maxsize=None)
def crowded_cells():
    """`ball` plus one atom of radius 20 about 52 A away, which buries nothing: h = 21.4, and the far atom is placed so
    that cell borders run through the ball's centre on every axis - a 2 x 2 x 2 block of cells of about 115 atoms."""
    b = dc.ball()
    x, y, z, r, _ = b.part(0)
    h = float(F(PROBE) + F(20.0))
    far = np.array([-2.0 * h, -h, -h])      # min = far - h: borders at 0 on every axis
    xyz = np.concatenate([np.stack([x, y, z], -1), far[None, :].astype(F)])
    return dc._case("crowded_cells", [_part(xyz, np.append(r, F(20.0)))])


# ---- a long chain against the cell order --------------------------------------------------------------------------------------

CHAIN_ATOMS = 384
CHAIN_SEED = 62


@functools.lru_cache(maxsize=None)
def chain():
    """384 atoms in a line along x, 2.0 A apart, radius 1.76, input order a seeded permutation: one long component whose
    dot numbers are scrambled against the cell order and whose smallest dot sits near one end.  info["place"]: the place
    along the line of every input atom."""
    place = np.random.default_rng(CHAIN_SEED).permutation(CHAIN_ATOMS)
    xyz = np.zeros((CHAIN_ATOMS, 3))
    xyz[:, 0] = place * 2.0
    xyz += np.array([-100.0, 4.5, 7.25])
    return dc._case("chain", [_part(xyz, np.full(CHAIN_ATOMS, 1.76, F))], place=place)


# ---- a winner in a shell's rows past the first 64 ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ball_turned():
    """`ball` turned by a quarter about x, (x, y, z) -> (x, z, -y): in `ball` itself no deep atom's nearest dot lies in
    the rows past the first 64 of shell 4 (81 rows: the rows of the highest z); turned, those that lay at dy = -4 do."""
    x, y, z, r, _ = dc.ball().part(0)
    return dc._case("ball_turned", [(x, z, -y, r, None)])


# ---- pairs three cells apart that link at h / 2 -------------------------------------------------------------------------------

HALF_LINK = cc.H * F(0.5)


def _triple(axis, sign, base, dist, off, swap):
    """component_cases._pair and a third atom `off` cells below the pair along the axis: it links with nobody, places
    the grid, and makes it long enough that the reach S, not the last shell of the grid, ends the sweep of the pair's
    later atom."""
    x, y, z, r, _ = cc._pair(axis, sign, base, dist, swap)
    cols = [x, y, z]
    far = [a[0] for a in cols]
    far[axis] = F(float(cols[axis].min()) - off * float(cc.H))
    return tuple(np.append(a, F(v)) for a, v in zip(cols, far)) + (np.append(r, cc.MAX_R), None)


def cross_edges(part, link, n_points=cc.FAR_POINTS):
    """component_cases.cross_edges at another link and with bystanders: the edges between atoms 0 and 1."""
    import depth_model as dm
    x, y, z, r = part[:4]
    owner, qx, qy, qz = dm.dots_of(x, y, z, r, np.ones((len(x), n_points), bool), PROBE, n_points)
    a, b = np.flatnonzero(owner == 0), np.flatnonzero(owner == 1)
    dx, dy, dz = qx[a, None] - qx[None, b], qy[a, None] - qy[None, b], qz[a, None] - qz[None, b]
    d2 = dx * dx + dy * dy + dz * dz
    assert d2.dtype == F
    return int((d2 <= F(link) * F(link)).sum())


@functools.lru_cache(maxsize=None)
def half_link_pairs():
    """As component_cases.far_link_pairs, for link = h / 2, where the reach is S = 3, the smallest there is: centres just
    under 2 h + link apart, cells that differ by 3, at least one edge - and the third atom of _triple, so that the later
    atom of the pair has a last shell beyond S.  (In far_link that atom's sweep ends with the grid, at shell 3.)"""
    rng = np.random.default_rng(71)
    out = []
    for axis, sign in DIRECTIONS:
        for _ in range(4000):
            base = float(np.round(rng.uniform(-60.0, 60.0), 3))
            dist = float(2.5 * float(cc.H) - rng.uniform(0.02, 0.25))
            off = float(np.round(rng.uniform(4.0, 5.0), 3))
            part = _triple(axis, sign, base, dist, off, False)
            if cc._cell_gap(part, axis) == 3 and cross_edges(part, HALF_LINK) > 0:
                out.append((axis, sign, base, dist, off))
                break
        else:
            raise AssertionError(("no pair found", axis, sign))
    return out


@functools.lru_cache(maxsize=None)
def half_link():
    parts = [_triple(*p, swap) for p in half_link_pairs() for swap in (False, True)]
    return dc._case("half_link", parts)


# ---- the table ---------------------------------------------------------------------------------------------------------------

CASES = {"column_z": column_z, "slant_xp": lambda: slant(0, 1), "slant_xm": lambda: slant(0, -1),
         "slant_yp": lambda: slant(1, 1), "slant_ym": lambda: slant(1, -1),
         "margin_under": lambda: margin("under"), "margin_over": lambda: margin("over"), "margin_twelve": margin_twelve,
         "margin_small_h": margin_small_h, "margin_large_h": margin_large_h, "odd_beside_even": odd_beside_even,
         "crowded_cells": crowded_cells, "chain": chain, "ball_turned": ball_turned, "half_link": half_link}
# the point count(s) each case is run at
POINTS = {"column_z": (1,), "slant_xp": (1,), "slant_xm": (1,), "slant_yp": (1,), "slant_ym": (1,), "crowded_cells": CROWDED_POINTS,
          "half_link": (cc.FAR_POINTS,)}


def points_of(name):
    return POINTS.get(name, (100,))


def get(name):
    return CASES[name]()


def runs():
    """[(case, n_points)] of every run of every case; margin_twelve repeats under and over and is left to the batch tests."""
    return [(name, n) for name in CASES if name != "margin_twelve" for n in points_of(name)]
