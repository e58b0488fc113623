"""The inputs of the dot-fields tests (test_fields_cpu.py, test_gpu_fields.py): those of crowding_cases.py - each named
for what it reaches in the frame k_dot_fields (fields.hip) takes from k_dot_crowding - with the cutoff at the case's last
edge and seeded weights, and the cases that only the fields have: weights at the bound of a term, NaN and infinite
weights, and a sum that wraps.  A case is a crowding case with its weights [N, C], its kinds and its cutoff.  Plain
helper module (not a conftest)."""
import functools
from dataclasses import dataclass

import numpy as np

import crowding_cases as cc
import depth_cases as dc
import fields_model as fm

F = np.float32
ALL_KINDS = (fm.STEP, fm.INV_D, fm.INV_D2, fm.INV_1PD)
# 1, 2, 3 and 4 channels over every kind: all kinds different, and kinds repeated
CHANNEL_KINDS = ((0,), (1,), (2,), (3,), (0, 1), (2, 3), (1, 1), (3, 3), (0, 1, 2), (1, 2, 3), (2, 2, 0), (3, 0, 3),
                 (0, 1, 2, 3), (3, 2, 1, 0), (1, 1, 1, 1), (2, 3, 2, 3))


@dataclass
class FCase:
    c: cc.Case              # the geometry, lattice size, probe and flag bytes
    weights: np.ndarray     # float32[N, C]
    kinds: tuple
    cutoff: float

    def __getattr__(self, name):    # (x, y, z, r, so, n_points, probe, flags, cols, n_atoms, info, name)
        return getattr(self.c, name)


def weights(n, n_channels, seed):
    """Seeded weights like partial charges and hydropathies: uniform in [-1, 1], one in eight exactly 0."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1.0, 1.0, (n, n_channels))
    w[rng.integers(0, 8, (n, n_channels)) == 0] = 0.0
    return np.ascontiguousarray(w, F)


def of(c, kinds=ALL_KINDS, cutoff=None, seed=31, w=None):
    """A crowding case as a fields case: the cutoff is its last edge unless given."""
    kinds = tuple(kinds)
    return FCase(c, weights(c.n_atoms, len(kinds), seed) if w is None else np.ascontiguousarray(w, F), kinds,
                 float(c.edges[-1]) if cutoff is None else float(cutoff))


def masks(f, W=8):
    return cc.masks(f.c, W)


def model(f, W=8, flags="own"):
    """(dot_offsets, sums, mask) of the case from fields_model."""
    mask = masks(f, W)
    fl = f.flags if isinstance(flags, str) else flags
    off, rows = fm.sums_batch(f.x, f.y, f.z, f.r, f.so, mask, f.probe, f.n_points, f.weights, f.kinds, f.cutoff, fl)
    return off, rows, mask


def crowding_names():
    """The cases of crowding_cases.py, by name: {name: a function that makes the crowding case}."""
    out = {"caps": cc.caps, "lone": cc.lone, "pair": cc.pair, "packed": cc.packed, "crowd": cc.crowd,
           "nan_coordinate": cc.nan_coordinate, "nan_radius": cc.nan_radius}
    for n in cc.POINT_COUNTS:
        out["corner_%d" % n] = functools.partial(cc.corner, n)
    for kind in cc.TIE_KINDS:
        out["tie_" + kind] = functools.partial(cc.tie, kind)
    for e0 in (0.0, 1e-30):
        out["tie_zero_%g" % e0] = functools.partial(cc.tie_zero, e0)
    for s in cc.LAST_SHELLS:
        out["last_shell_%d" % s] = functools.partial(cc.last_shell, s)
    return out


# ---- the bound of a term ---------------------------------------------------------------------------------------------------

BOUND = float(2.0 ** 24)
ABOVE = float(np.nextafter(F(BOUND), F(np.inf)))


@functools.lru_cache(maxsize=None)
def special_weights():
    """corner(33) under STEP in four channels (t = w exactly): the channels are seeded weights with, at seeded atoms,
    0: +2^24 and -2^24 (the largest terms that count);  1: the next float above, both signs (they add nothing);
    2: NaN, +inf and -inf (they add nothing);  3: the smallest subnormal and 2^-25 (which round to 0: ties to even) and
    3 * 2^-25 (which rounds to 2)."""
    c = cc.corner(33)
    w = weights(c.n_atoms, 4, 77)
    pick = np.random.default_rng(78).permutation(c.n_atoms)
    w[pick[0:4], 0] = [BOUND, -BOUND, BOUND, -BOUND]
    w[pick[4:8], 1] = [ABOVE, -ABOVE, ABOVE, -ABOVE]
    w[pick[8:14], 2] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf]
    w[:, 3] = 0.0
    w[pick[14:17], 3] = [float(np.nextafter(F(0), F(1))), 2.0 ** -25, 3 * 2.0 ** -25]
    return FCase(c, w, (fm.STEP,) * 4, 9.0)


# ---- a sum that wraps ------------------------------------------------------------------------------------------------------

WRAP_ATOMS = 33000
WRAP_BALL = 3.0
WRAP_RADIUS, WRAP_PROBE = 0.2, 0.1      # a cell of 0.3: a grid of some twenty cells per axis, lists of a few hundred entries
WRAP_CUTOFF = 8.0                       # above the ball's diameter: every atom is a partner of every dot


@functools.lru_cache(maxsize=None)
def wrap_ball():
    """33 000 atoms in a ball of 3 A at ONE lattice point, every weight 2^24 under STEP, the cutoff covering the ball:
    every dot sums 33 000 terms of 2^48 = 33 000 * 2^48 > 2^63, which wraps."""
    rng = np.random.default_rng(5)
    v = rng.normal(size=(WRAP_ATOMS, 3))
    v *= (WRAP_BALL * rng.uniform(0, 1, WRAP_ATOMS) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    c = cc._case("wrap_ball", [(np.round(v, 4), np.full(WRAP_ATOMS, WRAP_RADIUS))], n_points=1, edges=(WRAP_CUTOFF,),
                 probe=WRAP_PROBE)
    return FCase(c, np.full((WRAP_ATOMS, 1), BOUND, F), (fm.STEP,), WRAP_CUTOFF)


def wrapped(n_terms, term=1 << 48):
    """int64: n_terms * term in two's complement."""
    v = (n_terms * term) % (1 << 64)
    return v - (1 << 64) if v >= 1 << 63 else v


# ---- batches ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def big_batch():
    """depth_cases.tail() - a structure of 65 536 atoms behind three small ones - with an empty structure in front, one
    in the middle and one behind."""
    d = dc.get("tail")
    so = np.concatenate([[0], d.so[:2], d.so[1:], d.so[-1:]]).astype(np.uint32)
    c = cc.Case("big_batch", d.x, d.y, d.z, d.r, so, n_points=12, edges=(9.0,), probe=d.probe)
    return of(c, (fm.INV_D, fm.INV_1PD), seed=41)
