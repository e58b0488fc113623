"""The inputs of the radial-count tests (test_radial_cpu.py, test_gpu_radial.py): the cases of hse_cases.py - named for
what they reach in the shell sweep - with seeded class bytes and edge lists, and the few cases only the histogram and the
pair tables need.  Seeded and small; the CPU file pins every new case to what it is named for from the models alone, the
GPU file compares the kernels with the model.  Plain helper module (not a conftest)."""
import functools

import numpy as np

import hse_cases as hc

F = np.float32
EDGES = (6.0, 8.0, 10.0, 12.0)     # the contact-number radii
N_CLASSES = 4

# n_classes x n_bins of the row: one cell; 21 and 63 below a wave's width in the row write, 64 at it, 65 one past it; 512
# the widest row (2 KiB of LDS per wave)
SHAPES = ((1, 1), (3, 7), (7, 9), (2, 32), (5, 13), (16, 32))


def classes_of(n, n_classes, seed):
    """A class byte per atom, every class below n_classes present when n allows."""
    cl = np.random.default_rng(seed).integers(0, n_classes, n).astype(np.uint8)
    cl[:min(n, n_classes)] = np.arange(min(n, n_classes), dtype=np.uint8)
    return cl


def edges_of(n_bins, last=12.0):
    """n_bins increasing radii up to `last`, float32."""
    return (np.arange(1, n_bins + 1, dtype=np.float64) * (last / n_bins)).astype(F)


def case_classes(name, n_classes=N_CLASSES):
    """The seeded class bytes of an hse_cases case (the seed is the name's)."""
    c = getattr(hc, name)()
    return classes_of(c.n_atoms, n_classes, sum(map(ord, name)) + 131 * n_classes)


# ---- many structures in one workgroup of k_radial_pairs ----------------------------------------------------------------------

N_SMALL, SMALL_ATOMS = 300, 3


@functools.lru_cache(maxsize=None)
def many_small():
    """300 structures of three atoms each within 4 A: the 900 atoms fit one workgroup of k_radial_pairs (1 024 atoms), which
    walks 300 structures and adds to 300 tables."""
    rng = np.random.default_rng(61)
    xyz = np.round(rng.uniform(0.0, 4.0, (N_SMALL * SMALL_ATOMS, 3)), 3)
    so = np.arange(0, N_SMALL * SMALL_ATOMS + 1, SMALL_ATOMS)
    return hc._case("many_small", xyz, rng.choice(hc.RADII, len(xyz)), so)


# ---- a pair cell above 2^32 ----------------------------------------------------------------------------------------------------

N_BOX, BOX, BOX_EDGE = 65600, 40.0, 100.0


@functools.lru_cache(maxsize=None)
def big_box():
    """One structure of 65 600 atoms in a 40 A box, to be counted with one class and the one edge 100: the box's diagonal
    is 69.3 A, so every atom counts for every other - every row is N - 1 = 65 599 and the pair cell is
    65 600 * 65 599 = 4 303 294 400, above 2^32.  (32-bit cell starts too: more than 65 535 atoms.)"""
    rng = np.random.default_rng(62)
    xyz = rng.uniform(0.0, BOX, (N_BOX, 3)).astype(F)
    return hc._case("big_box", xyz, np.full(N_BOX, 1.5, F))
