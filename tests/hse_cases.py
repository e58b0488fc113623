"""The inputs of the half-sphere exposure tests (test_hse_cpu.py, test_gpu_hse.py), each named for what it reaches in
k_half_sphere (hse.hip).  Seeded and small; the CPU file pins every case to what it is named for from the models alone,
the GPU file compares the kernel with the model.  Plain helper module (not a conftest)."""
import functools
from dataclasses import dataclass, field

import numpy as np

import depth_cases as dc
import tail_cases as tc

F = np.float32
PROBE = 1.4
RADII = dc.RADII


@dataclass
class Case:
    name: str
    x: np.ndarray
    y: np.ndarray
    z: np.ndarray
    r: np.ndarray
    so: np.ndarray
    dirs: np.ndarray = None
    flags: np.ndarray = None
    probe: float = PROBE
    info: dict = field(default_factory=dict)

    @property
    def cols(self):
        return self.x, self.y, self.z, self.r, None

    @property
    def n_atoms(self):
        return len(self.x)

    @property
    def h(self):
        return F(self.probe) + np.max(self.r)


def _case(name, xyz, r, so=None, **kw):
    xyz = np.asarray(xyz, F)
    so = np.array([0, len(xyz)], np.uint32) if so is None else np.asarray(so, np.uint32)
    return Case(name, *(np.ascontiguousarray(xyz[:, k]) for k in range(3)), np.ascontiguousarray(r, F), so, **kw)


def random_dirs(n, seed):
    """Directions of every length between 1e-3 and 1e3, none of them zero or NaN."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return (d * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(F)


# ---- the protein-like cluster ----------------------------------------------------------------------------------------

N_CLUSTER = 2000
COVER = 64.0   # a cutoff above the cluster's diameter: every atom counts for every other


@functools.lru_cache(maxsize=None)
def cluster():
    """2 000 atoms, a jittered 2 A lattice cut to a ball (the packing of a protein interior), in shuffled order, with
    directions of all lengths.  h = 1.4 + 1.88: about 12 cells per axis, so a cutoff of 13 A is swept over five shells
    by the atoms in the middle and ends at the grid's faces for those outside."""
    rng = np.random.default_rng(41)
    g = np.arange(-8, 9) * 2.0
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    xyz = xyz[np.argsort(np.linalg.norm(xyz, axis=1), kind="stable")[:N_CLUSTER]]
    xyz = xyz + rng.uniform(-0.3, 0.3, xyz.shape) + np.array([12.0, -7.0, 31.0])
    xyz = xyz[rng.permutation(len(xyz))]
    r = rng.choice(RADII, len(xyz)).astype(F)
    r[0] = RADII.max()
    return _case("cluster", np.round(xyz, 3), r, dirs=random_dirs(len(xyz), 42))


def cluster_cutoffs():
    """0, half a cell, one, two and three cells, 13 A, the whole cluster, FLT_MAX (c2 overflows to +inf)."""
    h = cluster().h
    return [0.0, float(F(0.5) * h), float(h), float(F(2.0) * h), float(F(3.0) * h), 13.0, COVER, float(np.finfo(F).max)]


@functools.lru_cache(maxsize=None)
def crowd():
    """The cluster with 200 more atoms inside one cell at its middle: an x-run of more than 64 atoms, so the loop over a
    step's atoms takes several trips; the sweeps of the middle atoms reach shell 5 (121 rows: two steps)."""
    c = cluster()
    rng = np.random.default_rng(43)
    mid = np.array([12.0, -7.0, 31.0]) + np.array([0.4, 0.4, 0.4])
    extra = np.round(mid + rng.uniform(0.0, 1.0, (200, 3)), 3)
    xyz = np.concatenate([np.stack([c.x, c.y, c.z], -1), extra.astype(F)])
    r = np.concatenate([c.r, rng.choice(RADII, 200).astype(F)])
    return _case("crowd", xyz, r, dirs=random_dirs(len(xyz), 44))


@functools.lru_cache(maxsize=None)
def odd_radius():
    """The cluster with one radius of 70: sh_margins_hold fails (a radius above 64) and the cell is 71.4 A."""
    c = cluster()
    r = c.r.copy()
    r[7] = 70.0
    return Case("odd_radius", c.x, c.y, c.z, r, c.so, c.dirs)


@functools.lru_cache(maxsize=None)
def nan_atom():
    """The cluster with one NaN coordinate: sh_margins_hold fails, the atom gets 0 / 0 and counts for nobody."""
    c = cluster()
    y = c.y.copy()
    y[11] = np.nan
    return Case("nan_atom", c.x, y, c.z, c.r, c.so, c.dirs, info=dict(atom=11))


# ---- hand cases --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hand():
    """Cutoff 5.  Centre 0 at (1, 2, 3) with direction (0, 0, 2): atom 1 along +u (up), atom 2 along -u (down), atom 3
    exactly perpendicular (side +0: up), atom 4 coincident with atom 0 (up, while atom 0 itself is not counted), atom 5
    beyond the cutoff: 3 / 1.  Centre 4, the coincident atom, with direction (-1, 0, 0): atom 0 (side -0, and -0 >= 0: up),
    atoms 1 and 2 (side +0: up), atom 3 (side -3: down): 3 / 1.  The others are partners only: 0 / 0."""
    xyz = [[1, 2, 3], [1, 2, 6], [1, 2, 1], [4, 2, 3], [1, 2, 3], [1, 9, 3]]
    dirs = np.array([[0, 0, 2], [1, 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0], [1, 0, 0]], F)
    flags = np.array([3, 1, 1, 1, 3, 1], np.uint8)
    return _case("hand", xyz, np.full(6, 1.5, F), dirs=dirs, flags=flags,
                 info=dict(cutoff=5.0, up=[3, 0, 0, 0, 3, 0], down=[1, 0, 0, 0, 1, 0]))


TIE_ORIGIN = (100.0, 200.0, -300.0)
TIE_OFFSETS = ((5.0, 12.0, 0.0), (3.0, 4.0, 12.0), (0.0, 0.0, 13.0))


def _outward(v, origin):
    return np.nextafter(F(v), F(np.inf) if v >= origin else F(-np.inf))


@functools.lru_cache(maxsize=None)
def ties(moved=False):
    """Integer coordinates, C = 13: partners at offsets (5, 12, 0), (3, 4, 12), (0, 0, 13) from the centre have
    d2 == c2 == 169 exactly and count.  moved: one coordinate of each (x, y and z in turn) lies one ulp further out, its
    d2 is above 169 and it does not count."""
    o = np.array(TIE_ORIGIN)
    pts = [o] + [o + np.array(d) for d in TIE_OFFSETS]
    xyz = np.array(pts, F)
    if moved:
        for k, axis in ((1, 0), (2, 1), (3, 2)):
            xyz[k, axis] = _outward(xyz[k, axis], o[axis])
    flags = np.array([3, 1, 1, 1], np.uint8)
    return _case("ties_moved" if moved else "ties", xyz, np.full(4, 1.5, F), flags=flags,
                 dirs=np.tile(np.array([[1.0, 1.0, 1.0]], F), (4, 1)), info=dict(cutoff=13.0))


# ---- the reach -----------------------------------------------------------------------------------------------------------

EDGE_CUTOFF = 5.0   # = (3 - 1/2) * 2: the stop rule is met after shell 3 with equality
EDGE_BOX = 80.0


@functools.lru_cache(maxsize=None)
def edge():
    """Cell size exactly 2 (probe 0.5, largest radius 1.5; atoms at 0 and 80 fix the grid: cell = floor((v + 2) / 2)),
    integer coordinates, C = 5: the rule c2 <= ((s - 1/2) h)^2 is met, with equality, after shell 3.  Centre `hi` sits one
    ulp under a cell's upper boundary on every axis, centre `lo` exactly on a lower boundary.  For both, along +x, -x,
    +y, -y, +z, -z: a tie partner at distance exactly 5 - in shell 3, the last one swept, on the side the centre leans
    to, in shell 2 on the other - and a partner at distance 7 on that axis, which never counts: on the side the centre
    leans to it lies in shell 4, the first one not swept, on the other in shell 3.  Some 300 more atoms on integer
    positions fill the box.
    info: hi, lo, and per centre the lists tie / far of (atom, axis, sign)."""
    rng = np.random.default_rng(45)
    eps = F(40.0) - np.nextafter(F(40.0), F(0.0))
    hi = np.full(3, F(40.0) - eps, F)          # cell 20 on every axis, at its upper edge
    lo = np.full(3, 20.0, F)                   # cell 11, at its lower edge
    pts, info = [np.zeros(3, F), np.full(3, EDGE_BOX, F), hi, lo], dict(hi=2, lo=3, tie={2: [], 3: []}, far={2: [], 3: []})
    for c_idx, c in ((2, hi), (3, lo)):
        for axis in range(3):
            for sign in (1.0, -1.0):
                for dist, key in ((5.0, "tie"), (7.0, "far")):
                    p = c.copy()
                    p[axis] = c[axis] + F(sign * dist)
                    info[key][c_idx].append((len(pts), axis, int(sign)))
                    pts.append(p)
    fill = rng.integers(2, 79, (300, 3)).astype(F)
    fill = fill[(np.abs(fill - 40.0).max(axis=1) > 8) & (np.abs(fill - 20.0).max(axis=1) > 8)]   # away from both centres
    xyz = np.concatenate([np.array(pts, F), fill])
    r = rng.choice(np.array([1.3, 1.4, 1.5], F), len(xyz)).astype(F)
    r[0] = 1.5
    return _case("edge", xyz, r, probe=0.5, dirs=random_dirs(len(xyz), 46), info=info)


# ---- batches -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def interleaved():
    """The cluster dealt out to two structures atom by atom: each atom's nearest neighbours belong to the other
    structure and must never count."""
    c = cluster()
    a, b = np.arange(0, c.n_atoms, 2), np.arange(1, c.n_atoms, 2)
    o = np.concatenate([a, b])
    return Case("interleaved", c.x[o], c.y[o], c.z[o], c.r[o], np.array([0, len(a), c.n_atoms], np.uint32), c.dirs[o])


@functools.lru_cache(maxsize=None)
def tiny_batch():
    """Empty and one-atom structures in first, middle and last place, between structures of 2, 40 and 3 atoms."""
    rng = np.random.default_rng(47)
    sizes = [0, 1, 2, 0, 1, 40, 3, 1, 0]
    xyz = np.round(rng.uniform(0.0, 9.0, (sum(sizes), 3)), 3)
    so = np.concatenate([[0], np.cumsum(sizes)])
    return _case("tiny_batch", xyz, rng.choice(RADII, len(xyz)), so, dirs=random_dirs(len(xyz), 48))


N_TAIL_CENTRES = 256


@functools.lru_cache(maxsize=None)
def tail_batch():
    """Three small structures and one of 65 536 atoms (32-bit absolute cell starts: tail_cases.case_2_20_1) with 256
    centres flagged in it - the first and last 16 atoms of its cell order among them; every atom is a partner."""
    big = tc.case_2_20_1().structures[0]
    small = [tc.small_structure(n, seed=3000 + n) for n in (5, 400, 3)]
    sts = small + [big]
    so = np.concatenate([[0], np.cumsum([len(s) for s in sts])]).astype(np.uint32)
    cat = [np.ascontiguousarray(np.concatenate([getattr(s, k) for s in sts])) for k in "xyzr"]
    n, b = int(so[-1]), int(so[-2])
    mn, inv, dims = tc.grid_of(big.x, big.y, big.z, big.r, tc.PROBE)
    order = np.argsort(tc.cell_index(big.x, big.y, big.z, mn, inv, dims), kind="stable")
    rng = np.random.default_rng(49)
    ends = np.concatenate([order[:16], order[-16:]])
    rest = np.setdiff1d(np.arange(len(big)), ends)
    centres = np.sort(np.concatenate([ends, rng.permutation(rest)[:N_TAIL_CENTRES - len(ends)]]))
    flags = np.full(n, 3, np.uint8)
    flags[b:] = 1
    flags[b + centres] = 3
    return Case("tail_batch", *cat, so, random_dirs(n, 50), flags, tc.PROBE,
                dict(centres=centres, first=order[:16], last=order[-16:]))


def part(c, s):
    """Structure s of a batch case as a case of its own."""
    b, e = int(c.so[s]), int(c.so[s + 1])
    return Case(f"{c.name}[{s}]", c.x[b:e], c.y[b:e], c.z[b:e], c.r[b:e], np.array([0, e - b], np.uint32),
                None if c.dirs is None else c.dirs[b:e], None if c.flags is None else c.flags[b:e], c.probe)
