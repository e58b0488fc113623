"""The inputs of the dot-enclosure tests (test_enclosure_cpu.py, test_gpu_enclosure.py) beyond those of crowding_cases.py,
each named for what it reaches in k_dot_enclosure (enclosure.hip).  Seeded and small; the CPU file pins every case to
what it is named for from the models alone, the GPU file compares the kernel with the model.  A case is a batch with its
lattice size, its directions, its reach and its flag bytes (None: every atom is an obstacle).  Plain helper module (not a
conftest)."""
import functools
from dataclasses import dataclass, field

import numpy as np

import crowding_cases as cc
import depth_model as dm
import enclosure_model as em
import hse_cases as hc
import points_model as pm

F = np.float32
FLT_MAX = float(np.finfo(F).max)
N_DIRS = 30
REACH = 10.0
DIRS_SWEEP = (1, 2, 31, 32)
COVER = 64.0        # above every small structure's diameter: the whole grid is swept


def reaches(h):
    """0, a reach whose square underflows, half a cell, the usual one, the whole grid, and the largest float."""
    return (0.0, 1e-30, float(F(0.5) * F(h)), REACH, COVER, FLT_MAX)


@dataclass
class Case:
    name: str
    x: np.ndarray
    y: np.ndarray
    z: np.ndarray
    r: np.ndarray
    so: np.ndarray
    n_points: int = 100
    n_dirs: int = N_DIRS
    reach: float = REACH
    flags: np.ndarray = None
    probe: float = cc.PROBE
    info: dict = field(default_factory=dict)

    @property
    def cols(self):
        return self.x, self.y, self.z, self.r, None

    @property
    def n_atoms(self):
        return len(self.x)


def _case(name, parts, **kw):
    """parts: [(xyz [n, 3], r [n])] - one per structure."""
    so = np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])]).astype(np.uint32)
    xyz = np.concatenate([np.asarray(p[0], F).reshape(-1, 3) for p in parts])
    r = np.concatenate([np.asarray(p[1], F) for p in parts])
    return Case(name, *(np.ascontiguousarray(xyz[:, k]) for k in range(3)), np.ascontiguousarray(r), so, **kw)


def of(c, **kw):
    """A case of crowding_cases.py (or anything with its columns) as an enclosure case."""
    kw.setdefault("n_points", getattr(c, "n_points", 100))
    kw.setdefault("flags", getattr(c, "flags", None))
    kw.setdefault("info", getattr(c, "info", {}))
    return Case(c.name, c.x, c.y, c.z, c.r, c.so, probe=c.probe, **kw)


def of_depth(name, **kw):
    return of(cc.of_depth(name), **kw)


def masks(c, W=8):
    return pm.exposed_masks_batch(c.x, c.y, c.z, c.r, None, c.so, c.probe, c.n_points, W)


# ---- exact ties ----------------------------------------------------------------------------------------------------------
# One lattice point and one direction, both exactly (0, 0, 1).  The owner sits at the origin with R_i = 1/8 (radius and
# probe 1/16 each), so its dot is q = (0, 0, 1/8); the obstacle has R_j = 1/8 too, R2 = 2^-6, and L = 512.  Every
# coordinate is dyadic and every sum below is exact in float32 unless said otherwise.  L is 4096 R_j for the sake of
# `past_L`: the far end's offset there is one ulp of L, 2^-14, and its square 2^-28 must not vanish beside R2 = 2^-6
# (whose ulp is 2^-29) - with L of the order of R_j the end-cap's e2 rounds back to R2 and the case would hit.
TIE_R = 0.125
TIE_L = 512.0
TIE_ULP_L = 2.0 ** -14          # the ulp of a float32 in [512, 1024)
TIE_KINDS = {
    # name: ((dx, dz) of the obstacle from the dot, hit)
    "perp_tie": ((TIE_R, TIE_R), True),                          # t = 1/8 <= L; d2 - t*t = 2^-5 - 2^-6 == R2
    "perp_miss": ((float(np.nextafter(F(TIE_R), F(1))), TIE_R), False),     # dx one ulp larger: 2^-6 + 2^-28 > R2
    "at_L": ((TIE_R, TIE_L), True),                              # t == L takes the t <= L arm (d2 rounds to L^2: 0 <= R2)
    "past_L": ((TIE_R, TIE_L + TIE_ULP_L), False),               # t = nextafter(L): the end cap, e2 = 2^-6 + 2^-28 > R2
    "cap_tie": ((0.0, TIE_L + TIE_R), True),                     # the end cap, e2 = (1/8)^2 == R2
    "cap_miss": ((0.0, TIE_L + TIE_R + TIE_ULP_L), False),       # one ulp further
}


@functools.lru_cache(maxsize=None)
def ray_ties():
    """One structure of two atoms per kind of TIE_KINDS, in that order; info: kinds, hit (per structure)."""
    parts = []
    for (dx, dz), _ in TIE_KINDS.values():
        parts.append((np.array([[0.0, 0.0, 0.0], [dx, 0.0, TIE_R + dz]]), [TIE_R / 2, TIE_R / 2]))
    return _case("ray_ties", parts, n_points=1, n_dirs=1, reach=TIE_L, probe=TIE_R / 2,
                 info=dict(kinds=list(TIE_KINDS), hit=[h for _, h in TIE_KINDS.values()]))


# ---- the stop rule -------------------------------------------------------------------------------------------------------

LAST_SHELL = 5
LAST_REACH = 5.0    # = (5 - 2.5) * 2: the rule is met after shell 5 with equality
LAST_POINTS = 100
LAST_INSIDE = 1.6   # how far behind the ray's far end the obstacle's centre lies, along the axis (R_j = 2)


def _owners():
    eps = F(40.0) - np.nextafter(F(40.0), F(0.0))
    return np.full(3, F(40.0) - eps, F), np.full(3, 20.0, F)


def _dots(c):
    full = np.ones((1, LAST_POINTS), bool)
    _, qx, qy, qz = dm.dots_of(c[:1], c[1:2], c[2:], np.array([1.5], F), full, 0.5, LAST_POINTS)
    return np.stack([qx, qy, qz], -1)


LAST_SHELLS = (3, 4, 5)     # 3: the rule's clamp - the first shell after which it may stop a sweep


def last_reach(shell):
    """(shell - 2.5) h with h = 2: the reach that the rule meets, with equality, after `shell` shells."""
    return (shell - 2.5) * 2.0


@functools.lru_cache(maxsize=None)
def last_shell(shell=LAST_SHELL):
    """hse_cases.edge()'s grid (cell size exactly 2: probe 0.5, largest radius 1.5, atoms at 0 and 80 fix it), reach
    5 = (5 - 2.5) h: the stop rule is met, with equality, after shell 5.  Owner `hi` sits one ulp under a cell's upper
    boundary on every axis, owner `lo` exactly on a lower one; both have radius 1.5 (R = h) and every point free.  For
    hi along +x, +y, +z and for lo along -x, -y, -z - the side the owner leans to; on the other side shell 5 is out of
    any ray's reach -: the dot k and the direction m that lean that way most, and an obstacle of radius 1.5 (R_j = h)
    whose centre lies LAST_INSIDE beyond the far end of that ray along the axis, so the end is inside its sphere; its
    cell is five from the owner's.  info: hi, lo, rays = [(owner, dot rank k, direction m, obstacle)].
    shell 4 and 3 (the clamp s >= 3): the same with the reach (shell - 2.5) h = 3 and 1 = h / 2; the obstacle's cell is
    four and three from the owner's."""
    reach = last_reach(shell)
    hi, lo = _owners()
    u = em.directions(N_DIRS).astype(np.float64)
    pts, rays = [np.zeros(3, F), np.full(3, hc.EDGE_BOX, F), hi, lo], []
    for o_idx, c, sign in ((2, hi, 1.0), (3, lo, -1.0)):
        q = _dots(c)
        for axis in range(3):
            k = int(np.argmax(sign * q[:, axis].astype(np.float64)))
            m = int(np.argmax(sign * u[:, axis]))
            p = q[k].astype(np.float64) + reach * u[m]
            p[axis] += sign * LAST_INSIDE
            rays.append((o_idx, k, m, len(pts)))
            pts.append(p.astype(F))
    xyz = np.array(pts, F)
    return _case("last_shell" if shell == LAST_SHELL else "last_shell_%d" % shell, [(xyz, np.full(len(xyz), 1.5, F))],
                 n_points=LAST_POINTS, reach=reach, probe=0.5, info=dict(hi=2, lo=3, rays=rays, shell=shell))


# ---- the prefilter -------------------------------------------------------------------------------------------------------

EDGE_BEHIND = {"tie": 2.0, "inside": 1.95, "outside": 2.5}   # (outside: the tie's position moved up by one ulp of it)


@functools.lru_cache(maxsize=None)
def prefilter_edge():
    """last_shell()'s grid and owners, one structure per (owner, kind): lattice point 0 and direction 0 are both exactly
    (0, 0, 1), so the dot is c_i + (0, 0, 2) and the ray's far end c_i + (0, 0, 7); the obstacle (R_j = 2) lies on that
    line 2 behind the end (the end ON its sphere: an end-cap tie, |c_j - c_i| = L + R_i + R_j exactly), 1.95 behind it
    (99.4 % of that) or one ulp more than 2 (a miss).  info: cases = [(structure, kind)]; in every structure the atoms
    are 0, 1 (the grid's corners), 2 (the owner), 3 (the obstacle)."""
    parts, cases = [], []
    for c in _owners():
        for kind, behind in EDGE_BEHIND.items():
            p = c.copy()
            p[2] = (c[2] + F(2.0)) + F(LAST_REACH) + F(min(behind, 2.0))
            if kind == "outside":
                p[2] = np.nextafter(p[2], F(np.inf))
            parts.append((np.array([np.zeros(3, F), np.full(3, hc.EDGE_BOX, F), c, p], F), np.full(4, 1.5, F)))
            cases.append((len(parts) - 1, kind))
    return _case("prefilter_edge", parts, n_points=LAST_POINTS, reach=LAST_REACH, probe=0.5, info=dict(cases=cases))
