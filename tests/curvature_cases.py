"""The inputs of the dot-curvature tests (test_curvature_cpu.py, test_gpu_curvature.py), each named for what it reaches in
k_dot_curvature (curvature.hip) or in the definition's drop rule.  Seeded or exact; the CPU file pins every case to what
it is named for from the model (curvature_model.py) alone, the GPU file compares the kernel with the model.  Cases of the
other dot families are taken as they are (geodesics_cases, sweep_cases, crowding_cases, depth_cases).  Plain helper module
(not a conftest)."""
import functools
from dataclasses import dataclass, field

import numpy as np

import component_cases as cc
import crowding_cases as crc
import curvature_model as cvm
import depth_cases as dc
import depth_model as dm
import geodesics_cases as gc
import points_model as pm
import sweep_cases as sc
import sweep_model as sm

F = np.float32
WAVE = sm.WAVE


@dataclass
class Case:
    name: str
    x: np.ndarray
    y: np.ndarray
    z: np.ndarray
    r: np.ndarray
    so: np.ndarray
    n_points: int = 100
    reach: float = 3.0
    probe: float = dc.PROBE
    info: dict = field(default_factory=dict)

    @property
    def cols(self):
        return self.x, self.y, self.z, self.r, None

    @property
    def n_atoms(self):
        return len(self.x)

    def part(self, s):
        b, e = int(self.so[s]), int(self.so[s + 1])
        return tuple(a[b:e] for a in (self.x, self.y, self.z, self.r))


def of(c, n_points, reach, name=None, **info):
    """A case of another family (anything with x, y, z, r, so, probe) at a point count and a reach."""
    return Case(name or c.name, c.x, c.y, c.z, c.r, np.asarray(c.so, np.uint32), n_points, float(reach), c.probe,
                dict(getattr(c, "info", {}), **info))


def _build(name, parts, n_points, reach, probe=dc.PROBE, **info):
    """parts: [(xyz [n, 3], r [n])] - one per structure."""
    so = np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])]).astype(np.uint32)
    xyz = np.concatenate([np.asarray(p[0], F).reshape(-1, 3) for p in parts]) if parts else np.zeros((0, 3), F)
    r = np.concatenate([np.asarray(p[1], F) for p in parts]) if parts else np.zeros(0, F)
    return Case(name, *(np.ascontiguousarray(xyz[:, k]) for k in range(3)), np.ascontiguousarray(r), so, n_points, float(reach),
                probe, info)


@functools.lru_cache(maxsize=None)
def masks(c_key, W=8):
    c = _KEYED[c_key]
    if c.n_atoms == 0:
        return np.zeros((0, c.n_points), bool)
    return pm.exposed_masks_batch(c.x, c.y, c.z, c.r, None, c.so, c.probe, c.n_points, W)


_KEYED = {}


def key(c):
    """A hashable handle of a case for the cached model (cases are built once and live as long as the session)."""
    k = (c.name, c.n_points, float(c.reach), id(c.x))
    _KEYED[k] = c
    return k


@functools.lru_cache(maxsize=None)
def _model(c_key, W):
    c = _KEYED[c_key]
    return cvm.rows_batch(c.x, c.y, c.z, c.r, None, c.so, c.probe, c.n_points, c.reach, W, masks(c_key, W))


def model(c, W=8):
    """(dot_offsets, pairs, moments, dropped, mask) of a case: computed once, shared and left unchanged."""
    return _model(key(c), W)


# ---- the lone sphere of the header's figures ------------------------------------------------------------------------------------

SPHERE_RADIUS = 1.8


@functools.lru_cache(maxsize=None)
def sphere(n_points, reach):
    """One atom of radius 1.8 at an inexact place: R = 3.2, every dot accessible."""
    return _build("sphere", [(np.array([[5.5, -2.25, 9.0]]), np.array([SPHERE_RADIUS]))], n_points, reach)


# ---- hand tables: one point is the exact +z pole (0, 0, 1) -------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def two_dots():
    """Two atoms of radius 1 at probe 1 and ONE lattice point: dots at (0, 0, 2) and (3, 0, 6), normals (0, 0, 1).  From
    dot 0: d = (3, 0, 4), d2 = 25, h = 4, t = (3, 0, 0), t2 = 9, g = 4 / 9 (rounded), XX = 9 g, everything else 0; from
    dot 1 the chord is reversed: h = -4, g = -4 / 9."""
    xyz = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 4.0]])
    return _build("two_dots", [(xyz, np.ones(2))], 1, 5.0, probe=1.0)


@functools.lru_cache(maxsize=None)
def axis_pair():
    """Two atoms of radius 1 at probe 1 on the x axis 6 apart, at TWO lattice points: four dots, all accessible (the
    spheres of radius 2 do not meet)."""
    xyz = np.array([[0.0, 0.0, 0.0], [6.0, 0.0, 0.0]])
    return _build("axis_pair", [(xyz, np.ones(2))], 2, 16.0, probe=1.0)


# ---- the drop rule ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def coincident():
    """Probe 0: two atoms of radius 0 at the same place - their dots are their centres, nobody buries anybody - and an
    atom of radius 1 whose dot lies 3 along x from them, ONE point each: dots 0 and 1 coincide (d2 == 0: the pair does
    not count) and both see dot 2 at d2 == 9 with h == 0."""
    xyz = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [4.0, 2.0, 2.0]])
    return _build("coincident", [(xyz, np.array([0.0, 0.0, 1.0]))], 1, 3.0, probe=0.0)


@functools.lru_cache(maxsize=None)
def above():
    """Three atoms of radius 1 at probe 0 and ONE point: dots at (0, 0, 1), (0, 0, 4) - straight above the first, t2 == 0:
    the pair does not count in either direction - and (4, 0, 1), which dot 0 sees at d2 == 16 == reach^2 with h == 0 and
    dot 1 at d2 == 25, beyond the reach."""
    xyz = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 3.0], [4.0, 0.0, 0.0]])
    return _build("above", [(xyz, np.ones(3))], 1, 4.0, probe=0.0)


BOUND_X = 4096.0      # 4096^2 == 2^24


@functools.lru_cache(maxsize=None)
def bound():
    """Three atoms, ONE point each (probe 1, radius 1): dot 1 lies 4096 along x from dot 0 - d2 == 2^24 exactly, a term
    AT the bound: the pair counts - and dot 2 lies at (-4096, 1.25): d2 = fl(2^24 + 1.5625) = 2^24 + 2, the next float
    above the bound, and the pair does not count; dots 1 and 2 are 8192 apart.  The reach covers everything."""
    xyz = np.array([[0.0, 0.0, 0.0], [BOUND_X, 0.0, 0.0], [-BOUND_X, 1.25, 0.0]])
    return _build("bound", [(xyz, np.ones(3))], 1, 16384.0, probe=1.0)


def nan_case(which):
    c = {"coordinate": crc.nan_coordinate, "radius": crc.nan_radius}[which]()
    return of(c, c.n_points, 3.0)


# ---- dots per atom, point counts, chunks -----------------------------------------------------------------------------------------

POINT_COUNTS = (1, 2, 63, 64, 65, 100, 960)


def dot_counts():
    """geodesics_cases.dot_counts: first atoms with 0, 1, 63, 64 and 65 dots of 65."""
    return of(gc.dot_counts(), gc.COUNT_POINTS, 3.0)


def cluster(n_points, reach=3.0):
    """component_cases.multi_chunk: two lone atoms and a cluster of three, as three structures."""
    return of(cc.multi_chunk(), n_points, reach)


def lone960():
    """geodesics_cases.lone at 960 points: 15 chunks of own dots against 15 chunks of staged ones; the reach covers the
    sphere, so every dot pairs with the other 959."""
    return of(gc.lone(), 960, 8.0)


# ---- staging rounds ----------------------------------------------------------------------------------------------------------------

CELL_COUNTS = (63, 64, 65, 200)
CELL_SPACING = 3.5
CELL_FAR_RADIUS = 20.0


@functools.lru_cache(maxsize=None)
def cell_of(k):
    """k atoms of radius 0.3 (R = 1.7) on a cubic lattice of 3.5 A - nobody buries anybody - inside ONE cell of a grid
    whose cell size h = 21.4 a far atom of radius 20 sets (sweep_cases.crowded_cells' placement: cell borders at 0 on
    every axis): the own cell's step of shell 0 stages k atoms, 64 to a round.  8 points."""
    h = float(F(dc.PROBE) + F(CELL_FAR_RADIUS))
    g = 1.0 + CELL_SPACING * np.arange(6)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:k]
    far = np.array([[-2.0 * h, -h, -h]])
    return _build("cell_of_%d" % k, [(np.concatenate([xyz, far]), np.append(np.full(k, 0.3), CELL_FAR_RADIUS))], 8, 3.0)


# ---- reaches -----------------------------------------------------------------------------------------------------------------------

def reaches(h):
    """0, 1e-30 (its square underflows), h / 2, 1.5, 3.0, 6.0."""
    return (0.0, 1e-30, float(F(0.5) * F(h)), 1.5, 3.0, 6.0)


def reach_case(reach):
    return of(dc.get("cavity"), 20, reach)


def whole_grid():
    """depth_cases.corner at a reach of 64: above the structure's diameter, every shell of the grid is swept."""
    return of(dc.get("corner"), 33, 64.0)


# ---- tie partners in the last swept shell, six directions -------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def last_shell_tie(d):
    """Direction d of sweep_cases.half_link (its structures 2 d and 2 d + 1: a pair of atoms whose cells differ by 3 along
    the axis and a bystander, in both index orders) at 960 points, run at the largest reach L <= h / 2 for which some
    dot pair ACROSS the two atoms has d2 == L * L exactly in float32: the reach S is 3, the partner atom lies in the
    last swept shell, and the pair is an exact tie.  info: L, below (the float under L), d2 (= L * L)."""
    hl = sc.half_link()
    parts = [(np.stack(hl.part(s)[:3], -1), hl.part(s)[3]) for s in (2 * d, 2 * d + 1)]
    n_points = cc.FAR_POINTS
    x, y, z, r = hl.part(2 * d)[:4]
    owner, qx, qy, qz = dm.dots_of(x, y, z, r, np.ones((3, n_points), bool), hl.probe, n_points)
    a, b = np.flatnonzero(owner == 0), np.flatnonzero(owner == 1)
    dx, dy, dz = qx[b][None, :] - qx[a][:, None], qy[b][None, :] - qy[a][:, None], qz[b][None, :] - qz[a][:, None]
    d2 = dx * dx + dy * dy + dz * dz
    assert d2.dtype == F
    for v in np.unique(d2[d2 <= sc.HALF_LINK * sc.HALF_LINK])[::-1]:
        L = F(np.sqrt(v))
        if L * L == v and L <= sc.HALF_LINK:
            break
    else:
        raise AssertionError(("no exact tie", d))
    return _build("last_shell_tie_%d" % d, parts, n_points, float(L), L=L, below=np.nextafter(L, F(0.0)), d2=v)


# ---- the staging cut ----------------------------------------------------------------------------------------------------------------

CUT_REACH = 1.25
CUT_RADII = (1.5, 1.25)


@functools.lru_cache(maxsize=None)
def at_the_cut(beyond):
    """Two atoms on the x axis and a bystander that keeps the grid long: the second atom's centre lies EXACTLY at the
    staging cut of the first - x = ((R_0 + reach) + h) + R_1 in float32, every operand exact - or (beyond) one float
    further.  No dot of the two is within the reach of a dot of the other (the cut leaves a whole h): the rows are the
    model's either way."""
    R0, R1 = F(CUT_RADII[0]) + F(dc.PROBE), F(CUT_RADII[1]) + F(dc.PROBE)
    h = F(dc.PROBE) + F(max(CUT_RADII))
    lim = ((R0 + F(CUT_REACH)) + h) + R1
    xj = np.nextafter(lim, F(np.inf)) if beyond else lim
    xyz = np.array([[0.0, 0.0, 0.0], [float(xj), 0.0, 0.0], [-12.0, 0.5, 0.25]])
    return _build("cut_beyond" if beyond else "cut_at", [(xyz, np.array(CUT_RADII + (1.5,)))], 33, CUT_REACH, lim=lim)


BARE_Z = 90000.0            # coordinates whose float32 step is 1 / 128: the dots are rounded by far more than a sum of radii is
BARE_RADIUS = 1.505
BARE_REACH = 0.75
BARE_A = 2.0 ** -13


@functools.lru_cache(maxsize=None)
def bare_cut():
    """The pair that only the + h of the staging cut keeps.  Probe 0, ONE point (the +z pole).  Atom 0 of radius 1.505
    at z = 90000: its dot's z, 90001.505, is rounded UP to 90001.5078125.  Atom 1 of radius 0 - its dot is its centre -
    lies 0.75 above that dot and 2^-13 to the side: d2 = fl(2^-26 + 0.5625) = 0.5625 = reach * reach, a tie, and
    t2 = 2^-26 > 0, so the pair counts (h = 0.75, XX = 0.75).  The centres are 2.2578 apart, more than
    R_0 + R_1 + reach = 2.255: a cut at that sum drops atom 1; the kernel's, a whole h wider, keeps it.  Atom 2 stands
    aside.  The structure passes the margins (|min| + dim * h is under 65536 h = 98 631)."""
    zq = float(F(BARE_Z) + F(BARE_RADIUS))
    xyz = np.array([[0.0, 0.0, BARE_Z], [BARE_A, 0.0, zq + BARE_REACH], [4.0, 0.0, BARE_Z]])
    return _build("bare_cut", [(xyz, np.array([BARE_RADIUS, 0.0, BARE_RADIUS]))], 1, BARE_REACH, probe=0.0)


# ---- the grids of the shared sweep ---------------------------------------------------------------------------------------------------

SWEEP_RUNS = (("column_z", 1), ("slant_xp", 1), ("slant_xm", 1), ("slant_yp", 1), ("slant_ym", 1), ("margin_under", 100),
              ("margin_over", 100), ("margin_small_h", 100))


def sweep_case(name, n_points):
    """A case of sweep_cases.py at the default reach of 3 A, in the units of the case (margin_small_h is scaled by 0.03);
    at ONE point, where a structure has a handful of dots many cells apart, at 16 A: eight shells of its thin grid."""
    reach = 3.0 * sc.SMALL_H_SCALE if name == "margin_small_h" else 16.0 if n_points == 1 else 3.0
    return of(sc.get(name), n_points, reach)


# ---- batches -----------------------------------------------------------------------------------------------------------------------

def small_batch(name):
    """depth_cases.tiny (empty and one-atom structures) or overlap_batch (structures that lie on top of each other)."""
    return of(dc.get(name), 33, 3.0)


BIG_SHAPE = (32, 32, 64)
BIG_SPACING = 6.1
BIG_SAMPLE = 48


@functools.lru_cache(maxsize=None)
def big():
    """Empty structures, two small ones and ONE structure of 65 536 atoms: a 32 x 32 x 64 lattice of 6.1 A, jittered by
    0.4 A, radius 1.6 (R = 3.0: a few neighbours overlap), at 4 points."""
    rng = np.random.default_rng(83)
    g = [np.arange(n) * BIG_SPACING for n in BIG_SHAPE]
    xyz = np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3) + rng.uniform(-0.4, 0.4, (65536, 3))
    xyz = np.round(xyz[rng.permutation(65536)], 3)
    t = dc.get("tiny")
    small = [(np.stack(t.part(s)[:3], -1), t.part(s)[3]) for s in range(len(t.so) - 1)]
    empty = (np.zeros((0, 3)), np.zeros(0))
    return _build("big", [empty] + small + [empty, (xyz, np.full(65536, 1.6)), empty], 4, 3.0, big=len(small) + 2)


def big_sample_rows(c, mask, sample):
    """(pairs, moments) of the dots of the atoms `sample` (indices within the big structure) against the dots of the
    atoms that can hold a partner - centres within R_i + R_j + reach + 1 A, a float64 prefilter a whole A wider than the
    triangle inequality asks - by the model's pair_rows."""
    s = c.info["big"]
    b, e = int(c.so[s]), int(c.so[s + 1])
    x, y, z, r = c.x[b:e], c.y[b:e], c.z[b:e], c.r[b:e]
    xyz = np.stack([x, y, z], -1).astype(np.float64)
    ps, ms = [], []
    for i in sample:
        near = np.flatnonzero(np.linalg.norm(xyz - xyz[i], axis=1) <= 2 * (1.6 + c.probe) + c.reach + 1.0)
        sub = np.zeros_like(mask[b:e])
        sub[near] = mask[b:e][near]
        owner, q, n = cvm.dots(x, y, z, r, sub, c.probe, c.n_points)
        every = np.arange(len(owner))
        p, m, _ = cvm.pair_rows(q, n, every[owner == i], every, c.reach)
        ps.append(p)
        ms.append(m)
    return np.concatenate(ps), np.concatenate(ms)
