"""The inputs of the dot-crowding tests (test_crowding_cpu.py, test_gpu_crowding.py), each named for what it reaches in
k_dot_crowding (crowding.hip).  Seeded and small; the CPU file pins every case to what it is named for from the models
alone, the GPU file compares the kernel with the model.  A case is a batch with its lattice size, its edges and its flag
bytes (None: every atom is a partner).  Plain helper module (not a conftest)."""
import functools
from dataclasses import dataclass, field

import numpy as np

import depth_cases as dc
import depth_model as dm
import hse_cases as hc
import points_model as pm

F = np.float32
PROBE = dc.PROBE
EDGES = (6.0, 8.0, 10.0)
PASS = 128          # kDcPass: the dots one sweep of k_dot_crowding serves
POINT_COUNTS = (1, 63, 64, 65, 100, 960)


@dataclass
class Case:
    name: str
    x: np.ndarray
    y: np.ndarray
    z: np.ndarray
    r: np.ndarray
    so: np.ndarray
    n_points: int = 100
    edges: tuple = EDGES
    flags: np.ndarray = None
    probe: float = PROBE
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


def of_depth(name, **kw):
    """A case of depth_cases.py as a crowding case."""
    c = dc.get(name)
    return Case(name, c.x, c.y, c.z, c.r, c.so, probe=c.probe, **kw)


def masks(c, W=8):
    return pm.exposed_masks_batch(c.x, c.y, c.z, c.r, None, c.so, c.probe, c.n_points, W)


# ---- dots per atom -----------------------------------------------------------------------------------------------------

CAP_POINTS = 65
CAP_TARGETS = (0, 1, 63, 64, 65)
CAP_OWNER = (np.array([3.25, -1.5, 7.75]), 1.5)     # R = 2.9
CAP_COVER_RADIUS = 3.0                              # R = 4.4


def _cap_pair(d):
    """The owner and a larger atom d away from it, opposite the LAST lattice point: the nearer it comes, the more of the
    owner's points it buries, those furthest from the last point first."""
    from oracle import pyoracle as po
    s = np.stack([np.asarray(a, F) for a in po.sphere_points(CAP_POINTS)], -1).astype(np.float64)
    c, r = CAP_OWNER
    other = np.round(c - s[-1] / np.linalg.norm(s[-1]) * d, 3)
    return np.array([c, other]), np.array([r, CAP_COVER_RADIUS])


@functools.lru_cache(maxsize=None)
def _cap_distances():
    """{free count of the owner: a distance that gives it}, scanned on a grid of 0.02 A with the points model."""
    out = {}
    for d in np.arange(7.4, 1.0, -0.02):
        xyz, r = _cap_pair(float(d))
        m = pm.exposed_masks(*(xyz[:, k].astype(F) for k in range(3)), r.astype(F), None, PROBE, CAP_POINTS, 8)
        out.setdefault(int(m[0].sum()), float(d))
    return out


@functools.lru_cache(maxsize=None)
def caps():
    """Five structures of two atoms at 65 points: the first atom of each has 0, 1, 63, 64 and 65 accessible points - no
    dot, one lane, one lane short of a full wave, a full wave, a second dot in lane 0 -, and the one point of the
    second structure's is the last of the lattice."""
    dist = _cap_distances()
    return _case("caps", [_cap_pair(dist[t]) for t in CAP_TARGETS], n_points=CAP_POINTS,
                 info=dict(owners=[2 * k for k in range(len(CAP_TARGETS))], free=list(CAP_TARGETS)))


@functools.lru_cache(maxsize=None)
def corner(n_points):
    return of_depth("corner", n_points=n_points)


@functools.lru_cache(maxsize=None)
def lone(n_points=960):
    """One atom: every point is free, 960 dots take every pass (eight sweeps); its only partner is itself, at R."""
    return _case("lone", [(np.array([[1.0, -2.0, 3.0]]), [1.7])], n_points=n_points, edges=(3.0, 3.2, 10.0))


@functools.lru_cache(maxsize=None)
def pair(n_points=960):
    return _case("pair", [(np.array([[1.0, -2.0, 3.0], [4.5, -1.0, 2.0]]), [1.7, 1.88])], n_points=n_points,
                 edges=(3.0, 3.2, 5.0, 7.0))


# ---- exact ties --------------------------------------------------------------------------------------------------------

TIE_OWNER = (np.array([12.3, -4.7, 8.1], F), F(1.7))
TIE_POINTS = 65
TIE_DOT = 17
TIE_DX = 7.3
TIE_KINDS = ("last", "inner", "duplicate", "below")


def tie_geometry(probe=PROBE, partner_r=1.5, dx=TIE_DX, centre=None):
    """(xyz [2, 3] float32, r, q, edge): the owner (at `centre`, float32; None: TIE_OWNER's) and a partner moved from
    the owner's dot TIE_DOT along x alone: d2 = fl(ddx * ddx) with ddx = fl(c_j.x - q.x), and edge = |ddx| ties with it
    exactly."""
    c, r = TIE_OWNER
    if centre is not None:
        c = np.asarray(centre, F)
    m = np.zeros((1, TIE_POINTS), bool)
    m[0, TIE_DOT] = True
    _, qx, qy, qz = dm.dots_of(c[:1], c[1:2], c[2:], np.array([r], F), m, probe, TIE_POINTS)
    p = np.array([qx[0] + F(dx), qy[0], qz[0]], F)
    edge = np.abs(p[0] - qx[0])
    assert edge.dtype == F
    return np.stack([c, p]), np.array([r, partner_r], F), (qx[0], qy[0], qz[0]), edge


@functools.lru_cache(maxsize=None)
def tie(kind):
    """last: the tie is at the last edge; inner: at an inner one; duplicate: at an edge given twice (the first takes
    it); below: the last edge is nextafter(|dx|, 0) and the partner is lost."""
    xyz, r, _, e = tie_geometry()
    edges = {"last": (3.2, float(e)), "inner": (3.2, float(e), 9.0), "duplicate": (3.2, float(e), float(e), 9.0),
             "below": (3.2, float(np.nextafter(e, F(0.0))))}[kind]
    return _case("tie_" + kind, [(xyz, r)], n_points=TIE_POINTS, edges=edges, info=dict(owner=0, partner=1, dot=TIE_DOT))


@functools.lru_cache(maxsize=None)
def tie_zero(edge0):
    """Probe 0 and a partner of radius 0 exactly ON the owner's dot TIE_DOT (it buries nothing: R_j = 0): d2 = 0, which
    lies in the bin of an edge 0 and of an edge whose square underflows (edge0 = 0.0 or 1e-30)."""
    xyz, r, q, _ = tie_geometry(probe=0.0, partner_r=0.0, dx=0.0)
    return _case("tie_zero", [(xyz, r)], n_points=TIE_POINTS, edges=(edge0, 1.0, 4.0), probe=0.0,
                 info=dict(owner=0, partner=1, dot=TIE_DOT))


# ---- the stop rule -----------------------------------------------------------------------------------------------------

LAST_SHELL = 4
LAST_EDGE = 5.0     # = (4 - 1.5) * 2: the rule is met after shell 4 with equality
LAST_POINTS = 100


LAST_SHELLS = (2, 3, 4)     # 2: the rule's clamp - the first shell after which it may stop a sweep
LAST_PARTNER_RADIUS = {2: 0.25, 3: 1.25, 4: 1.25}   # (at shell 2 the partner lies 1 from the dot: R_j = 0.75 leaves it free)


def last_edges(shell):
    """The edges of last_shell(shell): the last one (shell - 1.5) h with h = 2, which the rule meets with equality."""
    last = (shell - 1.5) * 2.0
    return (2.0, 4.0, last) if shell == LAST_SHELL else (last / 4, last / 2, last)


@functools.lru_cache(maxsize=None)
def last_shell(shell=LAST_SHELL):
    """hse_cases.edge()'s grid (cell size exactly 2: probe 0.5, largest radius 1.5, atoms at 0 and 80 fix it), last edge
    5 = (4 - 1.5) h: the stop rule is met, with equality, after shell 4.  Owner `hi` sits one ulp under a cell's upper
    boundary on every axis, owner `lo` exactly on a lower one; both have radius 1.5 (R = h) and every point free.  For
    both, along +x, -x, +y, -y, +z, -z: the owner's outermost dot that way, and a partner moved 5 on along that axis
    alone - an exact tie at the last edge, up to 7 from the owner: in shell 4, the last one swept, on the side the owner
    leans to.  info: hi, lo, ties = [(owner, dot rank, partner)].
    shell 3 and 2 (the clamp s >= 2): the same with the last edge (shell - 1.5) h = 3 and 1 and the partners moved that
    far; at shell 2 the partners have radius 0.25, so that the dot 1 away from their centre stays accessible (the owners
    keep every point: `dot rank` is the point's number at every shell)."""
    last = last_edges(shell)[-1]
    eps = F(40.0) - np.nextafter(F(40.0), F(0.0))
    hi, lo = np.full(3, F(40.0) - eps, F), np.full(3, 20.0, F)
    pts, ties = [np.zeros(3, F), np.full(3, hc.EDGE_BOX, F), hi, lo], []
    full = np.ones((1, LAST_POINTS), bool)
    for o_idx, c in ((2, hi), (3, lo)):
        _, qx, qy, qz = dm.dots_of(c[:1], c[1:2], c[2:], np.array([1.5], F), full, 0.5, LAST_POINTS)
        q = np.stack([qx, qy, qz], -1)
        for axis in range(3):
            for sign in (1.0, -1.0):
                k = int(np.argmax(sign * q[:, axis].astype(np.float64)))
                p = q[k].copy()
                p[axis] = q[k, axis] + F(sign * last)
                ties.append((o_idx, k, len(pts)))
                pts.append(p)
    xyz = np.array(pts, F)
    r = np.full(len(xyz), LAST_PARTNER_RADIUS[shell], F)
    r[[0, 1, 2, 3]] = 1.5
    return _case("last_shell" if shell == LAST_SHELL else "last_shell_%d" % shell, [(xyz, r)], n_points=LAST_POINTS,
                 edges=last_edges(shell), probe=0.5, info=dict(hi=2, lo=3, ties=ties, shell=shell))


def reach_edges(h, shells):
    """A last edge that the rule admits after `shells` shells and not sooner: (shells - 1.5) h in float32."""
    return (float(F(0.5) * F(h)), float((F(shells) - F(1.5)) * F(h)))


REACHES = (2, 3, 4, 5, 6)
COVER = 64.0    # above the ball's diameter: every atom counts for every dot, the whole grid is swept


# ---- staging -------------------------------------------------------------------------------------------------------------

PACKED_ATOMS = 70
PACKED_PARTNERS = (63, 64, 65, 70)


@functools.lru_cache(maxsize=None)
def packed():
    """Four structures of 70 atoms in a cube of 1.2 A, which one cell holds (but for the lowest atom of an axis): one
    step of shell 0 with two staging batches, with 63, 64, 65 and all 70 of them flagged as partners (garbage in the
    other bits) - batches in which some, and in which all 64 lanes stage an atom."""
    rng = np.random.default_rng(91)
    parts, flags = [], []
    for k, n_par in enumerate(PACKED_PARTNERS):
        xyz = np.round(rng.uniform(0.0, 1.2, (PACKED_ATOMS, 3)) + np.array([5.0 * k, 2.0, -3.0]), 3)
        parts.append((xyz, rng.choice(dc.RADII, PACKED_ATOMS)))
        f = (rng.integers(0, 128, PACKED_ATOMS) << 1).astype(np.uint8)
        f[rng.permutation(PACKED_ATOMS)[:n_par]] |= 1
        flags.append(f)
    return _case("packed", parts, n_points=33, edges=(2.0, 4.0), flags=np.concatenate(flags))


@functools.lru_cache(maxsize=None)
def crowd():
    """hse_cases.crowd(): a cell of more than 200 atoms - an x-run of several staging batches in one step."""
    c = hc.crowd()
    return Case("crowd", c.x, c.y, c.z, c.r, c.so, n_points=20, edges=(4.0, 8.0))


def random_flags(n, seed):
    """Every pattern of the partner bit, garbage in the other seven."""
    return np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8)


# ---- non-finite input --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def nan_coordinate():
    c = corner(33)
    y = c.y.copy()
    y[7] = np.nan
    return Case("nan_coordinate", c.x, y, c.z, c.r, c.so, n_points=33, edges=(4.0, 9.0), info=dict(atom=7))


@functools.lru_cache(maxsize=None)
def nan_radius():
    c = corner(33)
    r = c.r.copy()
    r[9] = np.nan
    return Case("nan_radius", c.x, c.y, c.z, r, c.so, n_points=33, edges=(4.0, 9.0), info=dict(atom=9))


# ---- the radial witness ------------------------------------------------------------------------------------------------

def with_dots(c, dot_offsets, mask):
    """The batch with every structure's dots appended to it as centre-only atoms of radius 0: (x, y, z, r, so, flags,
    rows) - rows[d] is the batch position of dot d.  flags: bit 0 the case's partner bit on the atoms, bit 1 on the dots."""
    fl = np.ones(c.n_atoms, np.uint8) if c.flags is None else (c.flags & 1).astype(np.uint8)
    cols, so, flags, rows = [[], [], [], []], [0], [], []
    for s in range(len(c.so) - 1):
        b, e = int(c.so[s]), int(c.so[s + 1])
        _, qx, qy, qz = dm.dots_of(c.x[b:e], c.y[b:e], c.z[b:e], c.r[b:e], mask[b:e], c.probe, c.n_points)
        for col, a, q in zip(cols, (c.x[b:e], c.y[b:e], c.z[b:e], c.r[b:e]), (qx, qy, qz, np.zeros(len(qx), F))):
            col.extend([a, q])
        flags.extend([fl[b:e], np.full(len(qx), 2, np.uint8)])
        rows.append(so[-1] + (e - b) + np.arange(len(qx)))
        so.append(so[-1] + (e - b) + len(qx))
    cat = [np.ascontiguousarray(np.concatenate(col), F) for col in cols]
    return (*cat, np.asarray(so, np.uint32), np.concatenate(flags), np.concatenate(rows).astype(np.int64))
