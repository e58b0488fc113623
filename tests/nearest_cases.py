"""The inputs of the k-nearest-atoms tests (test_nearest_cpu.py, test_gpu_nearest.py).  The sweep's own edges come from
hse_cases.py and the sort's from within_cases.py; the cases added here sit on what k_nearest (nearest.hip) adds: a stop
rule fed by what the sweep has found (knn_edge) and a staging that is compacted when the next batch might not fit
(knn_stage).  Seeded and small; the CPU file pins every case to what it is named for from the model and the emulated
sweep alone.  Plain helper module (not a conftest)."""
import functools

import numpy as np

import hse_cases as hc
import nearest_model as nm
import within_cases as wc
from hse_cases import Case, _case  # noqa: F401  (Case: the tests build variants)

F = np.float32

EDGE_DIRECTIONS = ((0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1))   # (axis, sign)
EDGE_H = 2.0          # the cell size: probe 0.5, largest radius 1.5, as hse_cases.edge()
EDGE_KS = (1, 16)
TIE_KS = (1, 47, 48, 49, 72, 73, 80, 81)   # on within_cases.equal_d2(): classes of 48, 24 and 8 equal keys


@functools.lru_cache(maxsize=None)
def knn_edge(k):
    """Cell size exactly 2 (atoms at 0 and 80 fix the grid: cell = floor((v + 2) / 2)).  Six groups four cells apart on every axis, one per
    axis direction (axis, sign).  In each, a centre at fraction 0.99 of its cell along the direction (0.5 across it); k - 1
    partners inside its own cell, all nearer than 0.95 h; a DIAGONAL partner one cell back along the axis and one cell
    down across it, at 1.414 h, in shell 1; and the TRUE k-th neighbour 1.02 h ahead along the axis, which is two cells
    on: shell 2.  After shell 1 the sweep holds k keys whose k-th is the diagonal one (d2 = 2 h^2 > (0.5 h)^2: go on);
    after shell 2 the k-th is the true one (1.04 h^2 <= (1.5 h)^2: stop) - found in the last shell swept.  A rule relaxed
    by one shell stops after shell 1 with the diagonal partner in the list.  Only the six centres are centres.
    info: per direction the centre, the diagonal partner and the true k-th neighbour (atom indices)."""
    rng = np.random.default_rng(81 + k)
    pts = [np.zeros(3), np.full(3, 80.0)]
    flags = [1, 1]
    groups = []
    for n, (axis, sign) in enumerate(EDGE_DIRECTIONS):
        across = (axis + 1) % 3
        cell = np.array([8.0, 8.0, 8.0]) + 4.0 * n                       # the centre's cell, the same on every axis
        lower = EDGE_H * cell - 2.0
        c = lower + 1.0
        c[axis] = lower[axis] + (1.98 if sign > 0 else 0.02)
        centre = len(pts)
        pts.append(c.copy())
        flags.append(3)
        for _ in range(k - 1):                                           # inside the centre's cell, behind it
            p = c + rng.uniform(-0.6, 0.6, 3)
            p[axis] = c[axis] - sign * rng.uniform(0.08, 1.68)
            pts.append(np.round(p, 3))
            flags.append(1)
        d = c.copy()
        d[axis] -= sign * 2.0
        d[across] -= 2.0
        diagonal = len(pts)
        pts.append(d)
        flags.append(1)
        t = c.copy()
        t[axis] += sign * 2.04
        true_kth = len(pts)
        pts.append(t)
        flags.append(1)
        groups.append(dict(axis=axis, sign=sign, centre=centre, diagonal=diagonal, true_kth=true_kth))
    xyz = np.array(pts, F)
    r = np.full(len(xyz), 1.4, F)
    r[0] = 1.5
    return _case(f"knn_edge_{k}", xyz, r, probe=0.5, flags=np.array(flags, np.uint8), info=dict(k=k, groups=groups))


STAGE_SIZES = (nm.TRIGGER, nm.TRIGGER + 1, nm.TRIGGER + 2, nm.K_NN_STAGE + 76)
STAGE_KS = (256, 1)


@functools.lru_cache(maxsize=None)
def knn_stage():
    """Balls like within_cases._balls of T, T + 1, T + 2 and 1 100 atoms, T = 961 = kNnStage - 64 + 1: a centre of the
    first ball stages at most T - 1 keys, one short of the trigger, and is never compacted; in the second a centre that
    meets another batch after its last partner is compacted with exactly T keys staged; in the third with T or T + 1;
    the fourth overfills the staging outright.  One atom in four is a centre, every atom a partner."""
    flags = np.where(np.arange(sum(STAGE_SIZES)) % 4 == 1, 3, 1).astype(np.uint8)
    return wc._balls("knn_stage", list(STAGE_SIZES), 67, flags)


def case(name):
    """A case of this file, of within_cases.py or of hse_cases.py by name."""
    for mod in (wc, hc):
        if hasattr(mod, name) and name not in ("Case", "_case"):
            return getattr(mod, name)()
    return globals()[name]()
