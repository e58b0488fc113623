"""The inputs of the surface-component tests (test_components_cpu.py, test_gpu_components.py) beyond those of
depth_cases.py, each named for what it reaches in k_component_link (components.hip).  Seeded; the CPU file pins every
case to what it is named for from the model alone, the GPU file compares the kernels with the model.  Plain helper module
(not a conftest)."""
import functools

import numpy as np

import depth_cases as dc
import depth_model as dm
import structio as sio
import tail_cases as tc

F = np.float32
MAX_R = dc.RADII.max()
H = F(dc.PROBE) + MAX_R            # the cell size of a structure whose largest radius is MAX_R
CHUNK_POINTS = (65, 128, 129, 960)  # an atom's own dots take 2, 2, 3 and 15 chunks of 64 lanes
FAR_POINTS = 960
DIRECTIONS = [(axis, sign) for axis in range(3) for sign in (1, -1)]


def default_link(r, probe, n_points):
    """rustsasa_amd.default_link, restated: float32(1.5 sqrt(4 pi / n) (max finite radius folded from 0 + probe))."""
    r = np.asarray(r, F).astype(np.float64)
    r = r[np.isfinite(r)]
    return F(1.5 * np.sqrt(4.0 * np.pi / n_points) * (max(0.0, r.max() if r.size else 0.0) + float(probe)))


@functools.lru_cache(maxsize=None)
def pole_tie():
    """Two atoms 3 apart along x with one lattice point each, the exact +z pole: both dots are exact, d2 == 9."""
    xyz = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]], F)
    return dc._case("pole_tie", [dc._cols(xyz, np.array([1.0, 1.0], F))], probe=1.0)


def _pair(axis, sign, base, dist, swap):
    lo = np.array([7.0, -3.0, 11.0], np.float64)
    lo[axis] = base
    hi = lo.copy()
    hi[axis] = base + sign * dist
    xyz = np.stack([hi, lo] if swap else [lo, hi]).astype(F)
    return dc._cols(xyz, np.array([MAX_R, MAX_R], F))


def _cell_gap(part, axis):
    x, y, z, r = part[:4]
    _, _, c = dc.grid_cells(x, y, z, r, dc.PROBE)
    return abs(int(c[0, axis]) - int(c[1, axis]))


def cross_edges(part, link, n_points=FAR_POINTS):
    """How many edges join a dot of the first atom to a dot of the second (both atoms wholly accessible)."""
    x, y, z, r = part[:4]
    owner, qx, qy, qz = dm.dots_of(x, y, z, r, np.ones((2, n_points), bool), dc.PROBE, n_points)
    a, b = np.flatnonzero(owner == 0), np.flatnonzero(owner == 1)
    dx, dy, dz = qx[a, None] - qx[None, b], qy[a, None] - qy[None, b], qz[a, None] - qz[None, b]
    d2 = dx * dx + dy * dy + dz * dz
    assert d2.dtype == F
    return int((d2 <= H * H).sum())


@functools.lru_cache(maxsize=None)
def far_link_pairs():
    """[(axis, sign, base, dist)]: per direction a pair of atoms of the largest radius whose centres lie just under
    2 h + link apart (link = h) with cells that differ by 3 along the axis - the lower atom's cell coordinate rounds
    below 1 - and at least one edge between them.  Found by a seeded scan of the lower atom's place and the distance."""
    rng = np.random.default_rng(21)
    out = []
    for axis, sign in DIRECTIONS:
        for _ in range(4000):
            base = float(np.round(rng.uniform(-60.0, 60.0), 3))
            dist = float(3.0 * float(H) - rng.uniform(0.02, 0.25))
            part = _pair(axis, sign, base, dist, False)
            if _cell_gap(part, axis) == 3 and cross_edges(part, H) > 0:
                out.append((axis, sign, base, dist))
                break
        else:
            raise AssertionError(("no pair found", axis, sign))
    return out


@functools.lru_cache(maxsize=None)
def far_link(extra=0.0):
    """The pairs of far_link_pairs as one batch, each in both index orders (12 structures); `extra` moves the atoms of
    every pair that much further apart."""
    parts = [_pair(axis, sign, base, dist + extra, swap) for axis, sign, base, dist in far_link_pairs() for swap in (False, True)]
    return dc._case("far_link", parts)


@functools.lru_cache(maxsize=None)
def multi_chunk():
    """Two lone atoms and a cluster of 3 as three structures: run at CHUNK_POINTS, an atom's own dots fill several
    chunks of 64 lanes, the last one partly."""
    lone = lambda v, r: (np.array([v[0]], F), np.array([v[1]], F), np.array([v[2]], F), np.array([r], F), None)  # noqa: E731
    xyz = np.array([[0.0, 0.0, 0.0], [2.4, 0.3, -0.2], [1.1, 2.2, 0.4]], F)
    cluster = dc._cols(xyz, np.array([1.88, 1.42, 1.64], F))
    return dc._case("multi_chunk", [lone((5.5, -2.25, 9.0), 1.76), cluster, lone((-30.0, 4.0, 0.125), 1.42)])


@functools.lru_cache(maxsize=None)
def example_vdw():
    """example.cif with van der Waals radii (the reference's unit-test input): pockets of a few dots beside the outer
    surface, and atoms that own dots of two components."""
    x, y, z, r, ids = sio.soa_vdw(sio.read_structure(sio.data_path("example.cif")))
    return dc._case("example_vdw", [(x, y, z, r, ids)])


CASES = dict(dc.CASES, pole_tie=pole_tie, far_link=far_link, multi_chunk=multi_chunk, example_vdw=example_vdw)


def get(name):
    return CASES[name]()


def tail_grid(case):
    """(min, inv, dims) of the last structure of the `tail` case."""
    b, e = int(case.so[-2]), int(case.so[-1])
    return tc.grid_of(case.x[b:e], case.y[b:e], case.z[b:e], case.r[b:e], case.probe)
