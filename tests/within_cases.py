"""The inputs of the atoms-within-a-cutoff tests (test_within_cpu.py, test_gpu_within.py).  The sweep's own edges come
from hse_cases.py (cluster, crowd, ties, edge, odd_radius, nan_atom, hand, interleaved, tiny_batch, tail_batch); the cases
added here sit on what k_within_fill (within.hip) adds to the sweep: the LDS staging of K_WN_STAGE keys, the bitonic
network's padding to a power of two, the 256-key tiles of the long lists' ranking, and keys that tie in d2.  Seeded and
small; the CPU file pins every case to what it is named for from the model alone.  Plain helper module (not a conftest)."""
import functools

import numpy as np

import hse_cases as hc
from hse_cases import Case, _case  # noqa: F401  (Case: the tests build variants)

F = np.float32
K_WN_STAGE = 1024   # kWnStage (within.hip): keys a wave stages and sorts in LDS; a longer list goes through global scratch
SPILL_TILE = 256    # keys k_neighbor_rank_spill (neighbors.hip) compares at a time
BALL_CUTOFF = 8.0   # covers a ball of radius 3.5


def _balls(name, sizes, seed, flags=None):
    """A batch of tight balls (radius 3.5 A, centres 40 A apart) of the given sizes: under BALL_CUTOFF every atom of a
    ball lists all the others, so the lists of ball b are sizes[b] - 1 long."""
    rng = np.random.default_rng(seed)
    parts = []
    for b, n in enumerate(sizes):
        v = rng.normal(size=(n, 3))
        v *= (3.5 * rng.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=1)[:, None]
        parts.append(np.round(v + np.array([40.0 * b, -11.0, 5.0]), 3))
    xyz = np.concatenate(parts)
    so = np.concatenate([[0], np.cumsum(sizes)])
    r = rng.choice(hc.RADII, len(xyz)).astype(F)
    return _case(name, xyz, r, so, flags=flags, info=dict(sizes=list(sizes), cutoff=BALL_CUTOFF))


@functools.lru_cache(maxsize=None)
def stage_edges():
    """Lists of S - 1, S and S + 1 entries, S = K_WN_STAGE: the longest that is sorted in LDS with one key of room, the
    one that fills the staging, and the shortest that goes through global scratch (five tiles, the last of one key)."""
    return _balls("stage_edges", [K_WN_STAGE, K_WN_STAGE + 1, K_WN_STAGE + 2], 61)


@functools.lru_cache(maxsize=None)
def tile_edges():
    """Long lists of 5 * SPILL_TILE - 1, 5 * SPILL_TILE and 5 * SPILL_TILE + 1 entries: a last tile short of one key, whole
    tiles only, and a sixth tile of one key."""
    t = 5 * SPILL_TILE
    return _balls("tile_edges", [t, t + 1, t + 2], 62)


@functools.lru_cache(maxsize=None)
def double_edges():
    """Lists of 2 S - 1, 2 S and 2 S + 1 entries; one atom in eight is a centre (every atom is a partner), which keeps the
    entries at 1.6 million."""
    sizes = [2 * K_WN_STAGE, 2 * K_WN_STAGE + 1, 2 * K_WN_STAGE + 2]
    flags = np.where(np.arange(sum(sizes)) % 8 == 3, 3, 1).astype(np.uint8)
    return _balls("double_edges", sizes, 63, flags)


POW2_LISTS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 511, 512, 513)


@functools.lru_cache(maxsize=None)
def pow2_edges():
    """Lists one short of, at and one above the powers of two the bitonic network pads to."""
    return _balls("pow2_edges", [k + 1 for k in POW2_LISTS], 64)


N_COINCIDENT = (K_WN_STAGE + 76, 300)


@functools.lru_cache(maxsize=None)
def coincident():
    """Two structures: 1 100, and 300, atoms at one point with six more one A around it.  Every d2 among the coincident
    atoms is 0, so their order is by idx alone; the first structure's lists are longer than one stage (ranked in global
    scratch), the second's are sorted in LDS."""
    rng = np.random.default_rng(65)
    around = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], float)
    parts, sizes = [], []
    for s, n in enumerate(N_COINCIDENT):
        at = np.array([3.25 + 30.0 * s, -8.5, 17.75])
        xyz = np.concatenate([np.tile(at, (n, 1)), at + around])
        parts.append(xyz[rng.permutation(len(xyz))])
        sizes.append(len(xyz))
    xyz = np.concatenate(parts)
    return _case("coincident", xyz, np.full(len(xyz), 1.7, F), np.concatenate([[0], np.cumsum(sizes)]),
                 info=dict(cutoff=2.0, n=N_COINCIDENT))


EQUAL_ORIGIN = (1024.0, 2048.0, -3072.0)


@functools.lru_cache(maxsize=None)
def equal_d2():
    """A centre at a large origin and, around it, every signed permutation of the offsets (1.25, 2.5, 3.75), (0.5, 0.5, 4)
    and (2, 2, 2): 48 + 24 + 8 atoms in three classes of one d2 bit pattern each (the offsets and their squares are exact
    at this magnitude), in shuffled order, so that different idx share a d2 in the centre's list - and in each other's."""
    import itertools
    rng = np.random.default_rng(66)
    pts = {(0.0, 0.0, 0.0)}
    for off in ((1.25, 2.5, 3.75), (0.5, 0.5, 4.0), (2.0, 2.0, 2.0)):
        for perm in itertools.permutations(off):
            for sign in itertools.product((1.0, -1.0), repeat=3):
                pts.add(tuple(p * s for p, s in zip(perm, sign)))
    offs = np.array(sorted(pts))
    offs = offs[rng.permutation(len(offs))]
    centre = int(np.flatnonzero((offs == 0.0).all(axis=1))[0])
    xyz = offs + np.array(EQUAL_ORIGIN)
    return _case("equal_d2", xyz, np.full(len(xyz), 1.6, F), info=dict(cutoff=6.0, centre=centre, classes=(48, 24, 8)))


@functools.lru_cache(maxsize=None)
def overlap():
    """Two structures in the same space: the first 700 atoms of the cluster, twice, at the very same coordinates.  A list
    that crossed structures would hold an entry of d2 = 0."""
    c = hc.cluster()
    k = 700
    cat = lambda a: np.concatenate([a[:k], a[:k]])  # noqa: E731
    return Case("overlap", cat(c.x), cat(c.y), cat(c.z), cat(c.r), np.array([0, k, 2 * k], np.uint32))
