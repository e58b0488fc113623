"""The inputs of the second pass over the dot families (test_dot_edges2_cpu.py, test_gpu_dot_edges2.py): the cases of
sweep_cases.py with the links they are run at through k_dot_link (geodesics.hip), and new ones named for what they reach
in the host loop gd_phase (neighbors.cpp) and in k_patch_sample's queue (patches.hip).  Every coordinate of the new cases
is exact in float32 and every atom has ONE lattice point, the exact +z pole (0, 0, 1), at radius 1 and probe 1: the dots
lie at the atoms' (x, y) and z = 2, all accessible.  The CPU file pins every case to what it is named for from the models
alone.  Plain helper module (not a conftest)."""
import functools

import numpy as np

import component_cases as cc
import depth_cases as dc
import geodesics_cases as gc
import patches_cases as pc
import sweep_cases as sc

F = np.float32
PS_QUEUE = pc.PS_QUEUE
GD_ROUNDS = 8                      # kGdRounds of device_types.h: rounds between two looks of the host at the flags

# ---- A: the shared sweep's cases through the dot-link kernels -------------------------------------------------------------

LIST_RUNS = sc.runs() + [("margin_twelve", 100)]
# the cases of several structures, and the two single ones asked for: the weights fill is observed on these
WEIGHT_RUNS = [("column_z", 1), ("margin_under", 100), ("margin_over", 100), ("margin_twelve", 100), ("margin_small_h", 100),
               ("half_link", cc.FAR_POINTS), ("odd_beside_even", 100), ("crowded_cells", 100), ("chain", 100)]
CROSS_RUNS = [("half_link", cc.FAR_POINTS), ("crowded_cells", 65)] + [("margin_pair%d" % n, 100) for n in range(6)]


def case(name):
    if name.startswith("margin_pair"):
        return sc.margin_pair(int(name[len("margin_pair"):]))
    return sc.get(name)


def ball_link(n_points=100):
    """The default link of `ball` (about 1.74 at 100 points)."""
    b = dc.get("ball")
    return cc.default_link(b.r, b.probe, n_points)


def link_of(name, n_points):
    """The link a sweep case is run at: h / 2 for half_link; ball's default for odd_beside_even, whose own default
    follows its radius of 64.5 to 35 A; the default otherwise."""
    c = case(name)
    if name == "half_link":
        return sc.HALF_LINK
    if name == "odd_beside_even":
        return ball_link(100)
    return cc.default_link(c.r, c.probe, n_points)


def cross_link(name, n_points):
    """The link of a run of CROSS_RUNS: link_of, but ball's default for crowded_cells (its own gives one component)."""
    return ball_link(100) if name == "crowded_cells" else link_of(name, n_points)


def crowded_links(n_points):
    """The links of crowded_cells: 0, ball's default at 100 points, its own default (h = 21.4: 11.4 at 100 points, 14.1 at
    65), and - at 65 points only - four cells: the reach is the whole grid and every dot is linked to every other."""
    c = sc.get("crowded_cells")
    links = [F(0.0), ball_link(100), cc.default_link(c.r, c.probe, n_points)]
    if n_points == 65:
        links.append(F(4.0) * (F(c.probe) + c.r.max()))
    return links


def finite_limit(name):
    """The finite limit of a case's geodesics: 6 A, in the units of the case (margin_small_h is the ball scaled by 0.03)."""
    return 6.0 * sc.SMALL_H_SCALE if name == "margin_small_h" else 6.0


def middle_seeds(off, so):
    """uint8[D]: one seed per structure that has a dot, the dot in the middle of its range [b, e): b + (e - b) // 2."""
    off = np.asarray(off).astype(np.int64)
    seeds = np.zeros(int(off[-1]), np.uint8)
    for s in range(len(so) - 1):
        b, e = int(off[int(so[s])]), int(off[int(so[s + 1])])
        if e > b:
            seeds[b + (e - b) // 2] = 1
    return seeds


def last_seeds(off, so):
    """uint8[D]: the last dot of every structure that has one."""
    off = np.asarray(off).astype(np.int64)
    seeds = np.zeros(int(off[-1]), np.uint8)
    for s in range(len(so) - 1):
        b, e = int(off[int(so[s])]), int(off[int(so[s + 1])])
        if e > b:
            seeds[e - 1] = 1
    return seeds


# ---- B: a path of N dots -----------------------------------------------------------------------------------------------------

ROW_MAX = 18
ROW_LINK = F(1.0)


def _row_part(n):
    xyz = np.zeros((n, 3), F)
    xyz[:, 0] = np.arange(n)
    return dc._cols(xyz, np.ones(n, F))


@functools.lru_cache(maxsize=None)
def row(n):
    """patches_cases.ladder with n atoms, centres at x = 0 .. n - 1: link 1 joins neighbours only, a path of n dots with
    every weight exactly 1.  From a seed at one end the relaxation needs at most n rounds, the empty one included: n = 8
    can end on the last round of the first group of GD_ROUNDS, n = 9 on the first of the second."""
    return dc._case("row%d" % n, [_row_part(n)], probe=1.0, link=ROW_LINK)


# ---- C: the queue past the first step, two overflows, many workgroups --------------------------------------------------------

HUB_LINK = F(10.0)
HUB_STEP = 0.125
HUB_RADIUS = 2.5
HUB_LATTICE = 1257                 # the points of the 0.125 lattice within 2.5 of the origin
HUB_DISCS = (PS_QUEUE, PS_QUEUE + 1, 1200)


@functools.lru_cache(maxsize=None)
def disc_points():
    """float64[HUB_LATTICE, 2]: the points of the 0.125 lattice no further than 2.5 from the origin, sorted by (x, y)."""
    n = int(HUB_RADIUS / HUB_STEP)
    g = np.arange(-n, n + 1) * HUB_STEP
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    xy = xy[(xy ** 2).sum(axis=1) <= HUB_RADIUS ** 2]
    return xy[np.lexsort((xy[:, 1], xy[:, 0]))]


@functools.lru_cache(maxsize=None)
def hub(n_disc):
    """Dot 0 at x = 16, dot 1 - the hub - at x = 7, then n_disc dots on the disc around the origin, link 10: dot 0's only
    neighbour is the hub (9 away; the disc is at least 13.5 away), and the hub is linked to dot 0 and to every disc dot
    (at most 9.5 away).  The first pick is dot 0: its first step lowers the hub alone, its second step - the queue holds
    the hub, whose value cannot change then - lowers exactly the n_disc disc dots."""
    xy = disc_points()[:n_disc]
    assert len(xy) == n_disc
    xyz = np.zeros((n_disc + 2, 3), F)
    xyz[0, 0], xyz[1, 0] = 16.0, 7.0
    xyz[2:, :2] = xy
    assert np.array_equal(xyz[2:, :2].astype(np.float64), xy)
    return dc._case("hub%d" % n_disc, [dc._cols(xyz, np.ones(n_disc + 2, F))], probe=1.0, link=HUB_LINK)


TWO_FULL_POINTS = PS_QUEUE + 2
TWO_FULL_LINK = F(8.0)             # more than the lone atom's diameter of 6.32, far less than the 100 A between the two
TWO_FULL_APART = 100.0


def _lone_parts():
    x, y, z, r, _ = gc.get("lone").part(0)
    return (x, y, z, r, None), (x + F(TWO_FULL_APART), y, z, r, None)


@functools.lru_cache(maxsize=None)
def two_full():
    """geodesics_cases.lone and a copy 100 A along x in ONE structure, run at TWO_FULL_POINTS and link 8: within an atom
    every dot is linked to every other, between the atoms nothing is.  The first step of the first pick (dot 0) lowers
    PS_QUEUE + 1 dots, and so does the first step of the second pick (the second atom's first dot): two overflows, the
    queue in use again in between."""
    a, b = _lone_parts()
    return dc._case("two_full", [tuple(np.concatenate([p, q]) for p, q in zip(a[:4], b[:4])) + (None,)], link=TWO_FULL_LINK)


@functools.lru_cache(maxsize=None)
def two_full_batch():
    """The same two atoms as two structures of a batch."""
    return dc._case("two_full_batch", list(_lone_parts()), link=TWO_FULL_LINK)


ROWS_STRUCTURES = 600              # more than two workgroups per CU of a device of 256 CUs
ROWS_PERIOD = ROW_MAX + 1
ROWS_RUNS = ((0.0, None), (1.0, None), (np.inf, None), (0.0, 2))     # (spacing, max_centres)
ROWS_CENTRES = (5356, 2602, 568, 1104)                                 # the centres of each run, from the model


@functools.lru_cache(maxsize=None)
def rows_batch():
    """600 structures, structure s is row(s % 19): every 19th is empty, 5 356 dots in all."""
    return dc._case("rows_batch", [_row_part(s % ROWS_PERIOD) for s in range(ROWS_STRUCTURES)], probe=1.0, link=ROW_LINK)


CASES = {"two_full": two_full, "two_full_batch": two_full_batch, "rows_batch": rows_batch}


def get(name):
    if name.startswith("row") and name[3:].isdigit():
        return row(int(name[3:]))
    if name.startswith("hub"):
        return hub(int(name[3:]))
    return CASES[name]()
