"""The inputs of the atom-depth tests (test_depth_cpu.py, test_gpu_depth.py), each named for what it reaches in
k_atom_depth (depth.hip).  Seeded; the CPU file pins every case to its class from the model alone, the GPU file compares
the kernel with the model.  Every case is a batch: (x, y, z, r, ids) and structure offsets.  Plain helper module (not a
conftest)."""
import functools
from dataclasses import dataclass, field

import numpy as np

import tail_cases as tc

F = np.float32
PROBE = 1.4
RADII = np.array([1.42, 1.46, 1.61, 1.64, 1.76, 1.77, 1.88], F)   # ProtOr-like
SPACING = 2.0        # A, the cubic lattice of the ball
BALL_RADIUS = 12.0   # A
JITTER = 0.05        # A
VOID_CENTRE = np.array([3.0, 2.0, -3.0])   # off the ball's centre, 8 A under its surface
VOID_RADIUS = 3.8    # A: atoms nearer to VOID_CENTRE are removed


@dataclass
class Case:
    name: str
    x: np.ndarray
    y: np.ndarray
    z: np.ndarray
    r: np.ndarray
    ids: np.ndarray
    so: np.ndarray
    probe: float = PROBE
    info: dict = field(default_factory=dict)

    @property
    def cols(self):
        return self.x, self.y, self.z, self.r, self.ids

    @property
    def n_atoms(self):
        return len(self.x)

    def part(self, s):
        b, e = int(self.so[s]), int(self.so[s + 1])
        return tuple(a[b:e] for a in self.cols)


def _case(name, parts, probe=PROBE, **info):
    """parts: [(x, y, z, r, ids or None)]; missing ids rise through the batch."""
    so = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.uint32)
    cat = [np.ascontiguousarray(np.concatenate([np.asarray(p[k], F) for p in parts])) for k in range(4)]
    ids = np.arange(1, int(so[-1]) + 1, dtype=np.uint64)
    for s, p in enumerate(parts):
        if p[4] is not None:
            ids[int(so[s]):int(so[s + 1])] = p[4]
    return Case(name, *cat, ids, so, probe, info)


def _ball_atoms(seed=11):
    rng = np.random.default_rng(seed)
    n = int(BALL_RADIUS // SPACING)
    g = np.arange(-n, n + 1) * SPACING
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    xyz = xyz[np.linalg.norm(xyz, axis=1) <= BALL_RADIUS]
    xyz = xyz + rng.uniform(-JITTER, JITTER, xyz.shape)
    xyz = xyz[rng.permutation(len(xyz))]          # input order is not cell order
    r = rng.choice(RADII, len(xyz))
    return np.round(xyz, 3).astype(F), r.astype(F)


def _cols(xyz, r, ids=None):
    return tuple(np.ascontiguousarray(xyz[:, k]) for k in range(3)) + (r, ids)


@functools.lru_cache(maxsize=None)
def ball():
    """A solid ball: its central atoms find their nearest dot far beyond the 5x5x5 block of the neighbour sweep."""
    xyz, r = _ball_atoms()
    return _case("ball", [_cols(xyz, r)])


@functools.lru_cache(maxsize=None)
def cavity():
    """The ball with a void off its centre: the void holds accessible dots, and the atoms around it are nearer to
    those than to the outer surface.  info["rim"]: the atoms within 2 A of the void's wall."""
    xyz, r = _ball_atoms()
    d = np.linalg.norm(xyz.astype(np.float64) - VOID_CENTRE, axis=1)
    keep = d > VOID_RADIUS
    xyz, r, d = xyz[keep], r[keep], d[keep]
    return _case("cavity", [_cols(xyz, r)], rim=np.flatnonzero(d <= VOID_RADIUS + 2.0))


@functools.lru_cache(maxsize=None)
def twins():
    """Atoms 1 and 2 coincide and share an id (they do not occlude each other): identical masks, identical dots, exact
    ties in d2 for every atom.  Atom 0 lies inside them, buried; atom 3 stands beside them."""
    xyz = np.array([[0.3, 0.1, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [5.0, 0.5, 0.25]], F)
    r = np.array([0.5, 2.0, 2.0, 1.7], F)
    ids = np.array([5, 9, 9, 12], np.uint64)
    return _case("twins", [_cols(xyz, r, ids)])


@functools.lru_cache(maxsize=None)
def corner():
    """A small block of 5 x 4 x 3 atoms: a grid of a few cells per axis, every atom in an outermost occupied cell of
    some axis, so every sweep clips at grid faces and ends where the shells cover the grid or one shell before."""
    rng = np.random.default_rng(12)
    g = np.stack(np.meshgrid(np.arange(5), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3) * 2.1
    xyz = np.round(g + rng.uniform(-JITTER, JITTER, g.shape) + np.array([40.0, -17.0, 5.0]), 3).astype(F)
    xyz = xyz[rng.permutation(len(xyz))]
    return _case("corner", [_cols(xyz, rng.choice(RADII, len(xyz)).astype(F))])


@functools.lru_cache(maxsize=None)
def tiny():
    """Structures of 1 and 2 atoms, an empty structure between two others, 3 atoms."""
    e = np.zeros(0, F)
    one = (np.array([1.0], F), np.array([2.0], F), np.array([3.0], F), np.array([1.5], F), None)
    two = (np.array([0.0, 2.5], F), np.array([0.0, 0.5], F), np.array([0.0, -0.5], F), np.array([1.61, 1.88], F), None)
    three = (np.array([9.0, 10.0, 11.5], F), np.array([9.0, 9.5, 9.0], F), np.array([9.0, 9.0, 9.5], F),
             np.array([1.42, 1.76, 1.64], F), None)
    return _case("tiny", [one, (e, e, e, e, None), two, (e, e, e, e, None), three])


@functools.lru_cache(maxsize=None)
def overlap_batch():
    """The ball and a single atom at the ball's centre as two structures of one batch: the atom's dots lie in the
    middle of the ball and must count for nobody there."""
    b = ball()
    lone = (np.array([0.0], F), np.array([0.0], F), np.array([0.0], F), np.array([1.7], F), None)
    return _case("overlap_batch", [b.part(0)[:4] + (None,), lone])


@functools.lru_cache(maxsize=None)
def tail():
    """One structure of 65 536 atoms (32-bit absolute cell starts) behind a few small ones (16-bit relative)."""
    big = tc.case_2_20_1().structures[0]
    small = [tc.small_structure(n, seed=2000 + n) for n in (5, 400, 3)]
    parts = [(s.x, s.y, s.z, s.r, None) for s in small + [big]]
    return _case("tail", parts, probe=tc.PROBE, blob=big.blob)


CASES = {"ball": ball, "cavity": cavity, "twins": twins, "corner": corner, "tiny": tiny, "overlap_batch": overlap_batch,
         "tail": tail}
SMALL = ("ball", "cavity", "twins", "corner", "tiny", "overlap_batch")


def get(name):
    return CASES[name]()


def grid_cells(x, y, z, r, probe):
    """(cell size float32, dims int[3], cell coordinates int[N, 3]) of one structure's grid (tail_cases.grid_of)."""
    mn, inv, dims = tc.grid_of(x, y, z, r, probe)
    c = np.stack([np.minimum(((a - mn[k]) * inv).astype(np.int64), dims[k] - 1) for k, a in enumerate((x, y, z))], -1)
    return F(probe) + np.max(r), dims, c
