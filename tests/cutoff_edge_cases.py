"""The inputs of the second pass over the three cutoff sweeps (test_cutoff_edges_cpu.py, test_gpu_cutoff_edges.py):
k_half_sphere (hse.hip), k_within_* (within.hip) and k_nearest (nearest.hip), which all run one wave per centre over
shell_sweep.h and stop by sh_cutoff_reached (cutoff_sweep.h).  Four groups:

    the awkward grids of sweep_cases.py (thin, long, slanted, crowded, odd beside even), adapted from depth_cases.Case to
    hse_cases.Case - built for the depth and component sweeps, never yet given to the cutoff kernels;
    the margins' edge: sweep_cases' margin structures, and hse_cases.edge() / nearest_cases.knn_edge() translated in
    float32 to one coordinate ulp on either side of the 65536 h limit of sh_margins_hold;
    knn_dense: 3 000 atoms in one cell in descending order of distance, which takes k_nearest's staging through several
    compactions with a bound in force, and 40 nearer partners that arrive from shell 1 afterwards;
    the inputs of the call-order and thread tests.

Seeded and small; the CPU file pins every case to what it is named for from the models and emulations alone.  Plain
helper module (not a conftest)."""
import functools

import numpy as np

import hse_cases as hc
import nearest_cases as nc
import sweep_cases as sc
import sweep_model as sm
from hse_cases import Case

F = np.float32
DIRECTIONS = sc.DIRECTIONS             # (axis, sign): +x, -x, +y, -y, +z, -z
WHICH = ("under", "over")


# ---- depth_cases.Case -> hse_cases.Case ------------------------------------------------------------------------------------

def adapt(c, seed, name=None):
    """A depth_cases.Case (part(s), so, probe) as an hse_cases.Case with random directions of all lengths; ids are dropped
    (the cutoff sweeps take none into account)."""
    return Case(name or c.name, c.x, c.y, c.z, c.r, np.asarray(c.so, np.uint32), hc.random_dirs(c.n_atoms, seed), None,
                c.probe, dict(c.info))


GRID_NAMES = ("column_z", "slant_xp", "slant_xm", "slant_yp", "slant_ym", "chain", "crowded_cells", "odd_beside_even",
              "ball_turned")
MARGIN_NAMES = ("margin_under", "margin_over", "margin_twelve", "margin_small_h", "margin_large_h")


@functools.lru_cache(maxsize=None)
def swept(name):
    """A case of sweep_cases.py by name, adapted."""
    return adapt(sc.get(name), 900 + (GRID_NAMES + MARGIN_NAMES).index(name))


def cell_cutoffs(c):
    """(s - 1/2) h for s = 1, 2, 3 at the case's own h, formed in float32 as hse_cases.cluster_cutoffs forms its own."""
    h = c.h
    return [float((F(s) - F(0.5)) * h) for s in (1, 2, 3)]


def hse_cutoffs(c, name=None):
    """13 A (4 h for margin_small_h, as in within_cutoffs) and the three cutoffs at which the stop rule is met with equality."""
    return [float(F(4.0) * c.h) if name == "margin_small_h" else 13.0] + cell_cutoffs(c)


def within_cutoffs(c, name):
    """8 and 13 A (2.5 h and 4 h for margin_small_h, whose cell is 0.1 A), and a cutoff that covers the largest structure
    where that has under 1 000 atoms."""
    out = [float(F(2.5) * c.h), float(F(4.0) * c.h)] if name == "margin_small_h" else [8.0, 13.0]
    if int(np.diff(c.so.astype(np.int64)).max()) < 1000:
        out.append(covering_cutoff(c))
    return out


def covering_cutoff(c):
    """A cutoff above the diameter of every structure of the case."""
    d = 0.0
    for s in range(len(c.so) - 1):
        b, e = int(c.so[s]), int(c.so[s + 1])
        if e > b:
            ext = [float(a[b:e].astype(np.float64).max() - a[b:e].astype(np.float64).min()) for a in (c.x, c.y, c.z)]
            d = max(d, float(np.sqrt(sum(v * v for v in ext))))
    return float(F(1.05 * d + 1.0))


def nearest_cutoffs(c, name):
    return [None, float(F(4.0) * c.h) if name == "margin_small_h" else 13.0]


NEAREST_KS = (1, 16, 256)


def ends_sample(c, s, n=10, seed=0):
    """About a dozen atoms of structure s (indices within it): the two ends of its longest axis and a seeded choice."""
    p = hc.part(c, s)
    xyz = np.stack([p.x, p.y, p.z], -1).astype(np.float64)
    axis = int(np.argmax(xyz.max(axis=0) - xyz.min(axis=0)))
    ends = [int(np.argmin(xyz[:, axis])), int(np.argmax(xyz[:, axis]))]
    rest = np.random.default_rng(seed).permutation(p.n_atoms)[:n]
    return np.unique(np.concatenate([ends, rest])).astype(np.int64)


# ---- the exact-tie case at the margins' edge ----------------------------------------------------------------------------------

def _xyz(c):
    return np.stack([c.x, c.y, c.z], -1)


@functools.lru_cache(maxsize=None)
def edge_shifts():
    """{(axis, sign): (under, over)} for hse_cases.edge(): sweep_cases._edge_shift's largest translation that passes the
    margins test and the next one, one coordinate ulp further, that fails it."""
    e = hc.edge()
    return {d: sc._edge_shift(_xyz(e), e.r, e.probe, *d) for d in DIRECTIONS}


@functools.lru_cache(maxsize=None)
def edge_at_margin(axis, sign, which):
    """hse_cases.edge() translated in float32 along the axis to just under / just over 65536 h (h = 2: about 1.31e5, a
    coordinate ulp of 1/128).  The coordinates are integers and stay exact; `hi`, one ulp under a cell's upper boundary
    at the origin, rounds onto that boundary along the translated axis.  info as in edge(), and shift."""
    e = hc.edge()
    t = edge_shifts()[(axis, sign)][WHICH.index(which)]
    xyz = sc._moved(_xyz(e), axis, sign, t)
    return Case(f"edge_{which}_{'xyz'[axis]}{'+' if sign > 0 else '-'}", *(np.ascontiguousarray(xyz[:, k]) for k in range(3)),
                e.r, e.so, e.dirs, None, e.probe, dict(e.info, shift=t, axis=axis, sign=sign))


def _batch(name, parts, **info):
    so = np.concatenate([[0], np.cumsum([p.n_atoms for p in parts])]).astype(np.uint32)
    cat = lambda k: np.ascontiguousarray(np.concatenate([getattr(p, k) for p in parts]))  # noqa: E731
    flags = None if parts[0].flags is None else cat("flags")
    dirs = None if parts[0].dirs is None else cat("dirs")
    return Case(name, cat("x"), cat("y"), cat("z"), cat("r"), so, dirs, flags, parts[0].probe, info)


@functools.lru_cache(maxsize=None)
def edge_twelve():
    """The six `under` and the six `over` structures interleaved in one batch: under, over, under, over, ... in
    DIRECTIONS order.  The margins are decided per structure."""
    parts = [edge_at_margin(*d, w) for d in DIRECTIONS for w in WHICH]
    return _batch("edge_twelve", parts, members=parts)


# ---- the k-th neighbour in the last swept shell, at the margins' edge ---------------------------------------------------------

# nearest_cases.knn_edge's fractional offsets on multiples of 1/64, which a coordinate near 1.31e5 (ulp 1/128) holds exactly
KNN_NEAR, KNN_FAR = 1.0 / 64.0, 127.0 / 64.0      # the centre's place in its cell along the axis (0.02, 1.98)
KNN_TRUE = 2.0 + 3.0 / 64.0                       # the true k-th neighbour, ahead along the axis (2.04): 1.023 h
KNN_GRAIN = 64.0


@functools.lru_cache(maxsize=None)
def knn_edge_64(k):
    """nearest_cases.knn_edge(k) with every coordinate on a multiple of 1/64: the same groups, the same roles."""
    rng = np.random.default_rng(81 + k)
    pts, flags, groups = [np.zeros(3), np.full(3, 80.0)], [1, 1], []
    for n, (axis, sign) in enumerate(nc.EDGE_DIRECTIONS):
        across = (axis + 1) % 3
        lower = nc.EDGE_H * (np.array([8.0, 8.0, 8.0]) + 4.0 * n) - 2.0
        c = lower + 1.0
        c[axis] = lower[axis] + (KNN_FAR if sign > 0 else KNN_NEAR)
        centre = len(pts)
        pts.append(c.copy())
        flags.append(3)
        for _ in range(k - 1):                                           # inside the centre's cell, behind it
            p = c + rng.uniform(-0.6, 0.6, 3)
            p[axis] = c[axis] - sign * rng.uniform(0.08, 1.68)
            pts.append(np.round(p * KNN_GRAIN) / KNN_GRAIN)
            flags.append(1)
        d = c.copy()
        d[axis] -= sign * 2.0
        d[across] -= 2.0
        diagonal = len(pts)
        pts.append(d)
        flags.append(1)
        t = c.copy()
        t[axis] += sign * KNN_TRUE
        true_kth = len(pts)
        pts.append(t)
        flags.append(1)
        groups.append(dict(axis=axis, sign=sign, centre=centre, diagonal=diagonal, true_kth=true_kth))
    xyz = np.array(pts, F)
    assert np.array_equal(xyz * F(KNN_GRAIN), np.round(xyz * F(KNN_GRAIN)))
    r = np.full(len(xyz), 1.4, F)
    r[0] = 1.5
    return hc._case(f"knn_edge64_{k}", xyz, r, probe=0.5, flags=np.array(flags, np.uint8), info=dict(k=k, groups=groups))


@functools.lru_cache(maxsize=None)
def knn_edge_at_margin(k, axis, sign, which):
    """knn_edge_64(k) translated like edge_at_margin, by the shifts found for itself."""
    e = knn_edge_64(k)
    t = sc._edge_shift(_xyz(e), e.r, e.probe, axis, sign)[WHICH.index(which)]
    xyz = sc._moved(_xyz(e), axis, sign, t)
    assert np.array_equal(xyz.astype(np.float64), _xyz(e).astype(np.float64) + np.eye(3)[axis] * sign * t)   # exact
    return Case(f"knn_edge{k}_{which}_{'xyz'[axis]}{'+' if sign > 0 else '-'}", *(np.ascontiguousarray(xyz[:, n]) for n in range(3)),
                e.r, e.so, None, e.flags, e.probe, dict(e.info, shift=t))


@functools.lru_cache(maxsize=None)
def knn_edge_twelve(k):
    """All six translations of knn_edge_64(k), under and over interleaved, in one batch."""
    parts = [knn_edge_at_margin(k, *d, w) for d in DIRECTIONS for w in WHICH]
    return _batch(f"knn_edge{k}_twelve", parts, members=parts, k=k)


# ---- k_nearest past its first compaction ------------------------------------------------------------------------------------------

DENSE_H = float(F(1.4) + F(1.88))
DENSE_ATOMS = 3000
DENSE_NEAR = 40
DENSE_SEED = 2    # (of 0 .. 20, one for which every condition pinned in test_cutoff_edges_cpu.py holds)
DENSE_KS = (1, 64, 255, 256)


@functools.lru_cache(maxsize=None)
def knn_dense(odd=False):
    """Anchors at 0 and 8 h fix an 11^3 grid (cell = floor(v / h) + 1).  3 000 atoms uniformly inside the cell of index 4 on
    every axis, 0.05 to 3.2 from its lower corner, in DESCENDING order of distance from the centre `last`, which sits 0.02
    from that corner and comes after them: its wave stages the farthest first, so every compaction keeps keys that the
    next batches undercut - a second and third compaction with a bound in force, and a bound that is replaced.  Forty
    partners in the diagonally adjacent cell (shell 1), 0.05 to 0.5 beyond the corner on every axis, nearer to `last`
    than almost everything in its own cell: keys below the bound that arrive after shell 0 was compacted.
    Centres: `last`, atom 5 and atom 1 500; every atom is a partner.  odd: one anchor's radius is 70 - the margins fail
    and the cell is 71.4 A.
    info: last, near (the forty), centres."""
    rng = np.random.default_rng(DENSE_SEED)
    h = DENSE_H
    corner = np.full(3, 3.0 * h)
    last = corner + 0.02
    inside = corner + rng.uniform(0.05, 3.2, (DENSE_ATOMS, 3))
    inside = inside[np.argsort(-np.linalg.norm(inside - last, axis=1), kind="stable")]
    near = corner - rng.uniform(0.05, 0.5, (DENSE_NEAR, 3))
    xyz = np.round(np.concatenate([np.zeros((1, 3)), np.full((1, 3), 8.0 * h), inside, near, last[None, :]]), 3)
    n = len(xyz)
    r = np.full(n, 1.88, F)
    if odd:
        r[1] = 70.0
    flags = np.ones(n, np.uint8)
    centres = [n - 1, 5, 1500]
    flags[centres] = 3
    return hc._case("knn_dense_odd" if odd else "knn_dense", xyz, r, flags=flags,
                    info=dict(last=n - 1, near=np.arange(2 + DENSE_ATOMS, 2 + DENSE_ATOMS + DENSE_NEAR), centres=centres))


@functools.lru_cache(maxsize=None)
def knn_dense_thrice():
    """knn_dense three times in one batch, every atom of the second a centre: some 3 000 compacting waves in one launch,
    and a rank map that runs on past a structure boundary."""
    a = knn_dense()
    every = Case(a.name, a.x, a.y, a.z, a.r, a.so, None, np.full(a.n_atoms, 3, np.uint8), a.probe)
    return _batch("knn_dense_thrice", [a, every, a])


# ---- call order and threads ---------------------------------------------------------------------------------------------------------

def one_in_eight(n, phase=5):
    """Flags "one centre in eight": every atom a partner."""
    return np.where(np.arange(n) % 8 == phase, 3, 1).astype(np.uint8)


def margins_of(c, s=0):
    p = hc.part(c, s)
    return sm.margins_hold(p.x, p.y, p.z, p.r, p.probe)


THREADS, THREAD_ROUNDS = 8, 6
THREAD_INPUTS = ("1jcd", "edge", "tiny_batch")


def thread_input(tid, it):
    """The input thread tid uses in round it: every thread meets every input, and in every round all three are in use."""
    return THREAD_INPUTS[(tid + it) % len(THREAD_INPUTS)]
