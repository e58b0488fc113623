"""The inputs of the dot-link and dot-geodesic tests (test_geodesics_cpu.py, test_gpu_geodesics.py) beyond those of
depth_cases.py and component_cases.py, each named for what it reaches in geodesics.hip.  Seeded; the CPU file pins every
case to what it is named for from the model alone, the GPU file compares the kernels with the model.  Plain helper module
(not a conftest)."""
import functools

import numpy as np

import component_cases as cc
import depth_cases as dc
import points_model as pm
import structio as sio

F = np.float32
COUNT_POINTS = 65                 # the lattice of dot_counts: a lone atom has 65 dots, a chunk of 64 lanes and one more
COUNTS = (0, 1, 63, 64, 65)
CHAIN_ATOMS, CHAIN_STEP = 130, 3.0


@functools.lru_cache(maxsize=None)
def jcd():
    """The 1jcd fixture (three short chains) with van der Waals radii."""
    atoms = [a for a in sio.read_structure(sio.data_path("1jcd.pdb")) if not a.hetero]
    x, y, z, r, ids = sio.soa_vdw(atoms)
    return dc._case("jcd", [(x, y, z, r, ids)])


@functools.lru_cache(maxsize=None)
def lone():
    """One atom: at 960 points and a link of twice its expanded radius and more every dot is linked to every other - 959
    entries per list, 15 chunks of own dots against 15 chunks of staged ones."""
    return dc._case("lone", [(np.array([5.5], F), np.array([-2.25], F), np.array([9.0], F), np.array([1.76], F), None)])


@functools.lru_cache(maxsize=None)
def chain():
    """A straight chain of atoms 3 A apart along x: from a seed at one end the far end is more than 200 edges away at
    100 points and the default link (387 A of chain, edges of at most 1.8 A) - many times the rounds between two looks of
    the host at the relaxation's flags."""
    x = (np.arange(CHAIN_ATOMS) * CHAIN_STEP).astype(F)
    zero = np.zeros(CHAIN_ATOMS, F)
    return dc._case("chain", [(x, zero + F(0.25), zero - F(1.5), zero + F(1.8), None)])


@functools.lru_cache(maxsize=None)
def equal_sum():
    """Four atoms with ONE lattice point each (the exact +z pole), so the dots are exact: dot 0 at (-1, 2^-11), dot 1 at
    (1, 0), dot 2 at (0, 0), dot 3 at (0, 3), all at z = 2.  Seeds 0 and 1, link 3.  w(1, 2) = 1, w(0, 2) = 1 + 2^-23,
    w(2, 3) = 3: dist[2] = 1 comes from seed 1 alone, and fl(1 + 3) == fl((1 + 2^-23) + 3) = 4 - the path from seed 0
    reaches dot 3 at its dist but dot 2 above its dist, so source[3] is 1, and a (dist, source) pair minimised as one
    64-bit number can end on 0."""
    xyz = np.array([[-1.0, 2.0 ** -11, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 3.0, 0.0]], F)
    return dc._case("equal_sum", [dc._cols(xyz, np.ones(4, F))], probe=1.0, link=F(3.0), seeds=np.array([1, 1, 0, 0], np.uint8))


def _free_of_victim(dist):
    x = np.array([0.0, dist], F)
    z = np.zeros(2, F)
    r = np.array([1.2, 1.9], F)
    return int(pm.exposed_masks(x, z, z, r, None, dc.PROBE, COUNT_POINTS, 8)[0].sum())


@functools.lru_cache(maxsize=None)
def dot_counts():
    """Five two-atom structures (the last a lone pair far apart) whose first atoms have 0, 1, 63, 64 and 65 accessible
    points of 65: a small atom beside a larger one at a distance found by a scan.  info["first"]: those atoms."""
    found = {}
    for d in np.round(np.arange(0.0, 7.0, 0.01), 2):
        k = _free_of_victim(float(d))
        if k in COUNTS and k not in found:
            found[k] = float(d)
    assert sorted(found) == list(COUNTS), sorted(found)
    parts, first = [], []
    for n, k in enumerate(COUNTS):
        first.append(2 * n)
        parts.append((np.array([0.0, found[k]], F) + F(20.0 * n), np.zeros(2, F), np.zeros(2, F), np.array([1.2, 1.9], F), None))
    return dc._case("dot_counts", parts, first=np.array(first))


CASES = dict(cc.CASES, jcd=jcd, lone=lone, chain=chain, equal_sum=equal_sum, dot_counts=dot_counts)


def get(name):
    return CASES[name]()


def one_seed(n_dots, which=0):
    s = np.zeros(n_dots, np.uint8)
    if n_dots:
        s[which] = 1
    return s
