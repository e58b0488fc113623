"""An exact CPU model of the atom depths (rsasa_atom_depth*): the definition of include/rustsasa_amd.h followed literally
in numpy float32, brute force over every (target atom, accessible dot) pair of a structure, in chunks.

    R_j = r_j + p;  q = c_j + R_j * s_k (per component);  d = c_i - q;  d2 = (dx*dx + dy*dy) + dz*dz
    key_i = min over the accessible (j, k) of the structure whose d2 is no NaN of (bits(d2) << 32) | j

numpy's float32 operators round every product and sum on its own (nothing is fused), which is the definition's
arithmetic.  The masks come from points_model.py (pinned to the oracle).  A minimum has no order: no tolerance anywhere.
Plain helper module (not a conftest)."""
import numpy as np

import points_model as pm
from oracle import pyoracle as po

F = np.float32
NONE_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
_PAIRS = 1 << 22   # (target, dot) pairs evaluated at once


def dots_of(x, y, z, r, mask, probe, n_points):
    """(owner int64[D], qx, qy, qz float32[D]): the accessible dots of one structure in float32, as surface_points()
    lists them."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    sx, sy, sz = (np.asarray(a, F) for a in po.sphere_points(n_points))
    j, k = np.nonzero(mask)
    with np.errstate(invalid="ignore", over="ignore"):
        R = r[j] + F(probe)
        q = x[j] + R * sx[k], y[j] + R * sy[k], z[j] + R * sz[k]
    assert all(c.dtype == F for c in q)
    return (j.astype(np.int64),) + q


def keys_of(x, y, z, r, mask, probe, n_points, sample=None):
    """uint64[len(sample)]: key_i of the target atoms `sample` (indices; None: every atom) of ONE structure against all
    its accessible dots; NONE_KEY where no dot has a d2 that is not NaN."""
    x, y, z = (np.ascontiguousarray(a, F) for a in (x, y, z))
    tgt = np.arange(len(x)) if sample is None else np.asarray(sample, np.int64)
    owner, qx, qy, qz = dots_of(x, y, z, r, mask, probe, n_points)
    out = np.full(len(tgt), NONE_KEY, np.uint64)
    if len(owner) == 0 or len(tgt) == 0:
        return out
    low = owner.astype(np.uint64)
    step = max(1, _PAIRS // len(owner))
    for a in range(0, len(tgt), step):
        t = tgt[a:a + step]
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy, dz = x[t, None] - qx[None, :], y[t, None] - qy[None, :], z[t, None] - qz[None, :]
            d2 = dx * dx + dy * dy + dz * dz
        assert d2.dtype == F
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low[None, :]
        key[np.isnan(d2)] = NONE_KEY
        out[a:a + step] = key.min(axis=1)
    return out


def keys_of_sample_near(x, y, z, r, mask, probe, n_points, sample, slack=0.05):
    """keys_of(..., sample=sample) for a large structure, dot for dot the same keys: a target's nearest dot is at most
    U = |c_i - c_j| + |R_j| away, j the nearest atom that has a dot, so a dot of an atom further than U + max |R| from
    the target cannot be the nearest; only the dots of the atoms within U + max |R| + slack are evaluated (float64
    distances; slack covers float32 rounding of coordinates below 10^4 by a wide margin).  Finite input only."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    assert np.isfinite(x).all() and np.isfinite(y).all() and np.isfinite(z).all() and np.isfinite(r).all()
    assert max(np.abs(x).max(), np.abs(y).max(), np.abs(z).max()) < 1e4
    has = mask.any(axis=1)
    out = np.full(len(sample), NONE_KEY, np.uint64)
    if not has.any():
        return out
    xyz = np.stack([x, y, z], -1).astype(np.float64)
    R = np.abs(r.astype(np.float64) + float(probe))
    for n, i in enumerate(np.asarray(sample, np.int64)):
        d = np.sqrt(((xyz - xyz[i]) ** 2).sum(axis=1))
        U = (d + R)[has].min()
        near = np.flatnonzero(has & (d <= U + R.max() + slack))
        sub_mask = mask[near]
        k = keys_of(np.append(x[near], x[i]), np.append(y[near], y[i]), np.append(z[near], z[i]), np.append(r[near], r[i]),
                    np.vstack([sub_mask, np.zeros((1, mask.shape[1]), bool)]), probe, n_points, sample=[len(near)])[0]
        if k != NONE_KEY:
            k = (k & ~np.uint64(0xFFFFFFFF)) | np.uint64(near[int(k & np.uint64(0xFFFFFFFF))])
        out[n] = k
    return out


def split(keys):
    """keys -> (d2 bits uint32, depth float32 = sqrtf(d2) correctly rounded, nearest uint32); +inf and 0xFFFFFFFF where
    there is no dot."""
    keys = np.asarray(keys, np.uint64)
    bits = (keys >> np.uint64(32)).astype(np.uint32)
    with np.errstate(invalid="ignore"):
        depth = np.sqrt(bits.view(F))   # numpy's float32 sqrt is the correctly rounded one
    assert depth.dtype == F
    none = keys == NONE_KEY
    depth[none] = np.inf
    return bits, depth, (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def atom_depth(x, y, z, r, ids, probe, n_points, W=8, mask=None, sample=None):
    """(depth float32, nearest uint32, mask) of one structure; mask bool[N, n_points] defaults to points_model's."""
    if mask is None:
        mask = pm.exposed_masks(x, y, z, r, ids, probe, n_points, W)
    _, depth, nearest = split(keys_of(x, y, z, r, mask, probe, n_points, sample))
    return depth, nearest, mask


def atom_depth_batch(x, y, z, r, ids, so, probe, n_points, W=8, mask=None):
    """(depth, nearest, mask) of every structure of a batch, rows in batch order, nearest within the structure."""
    n = int(so[-1]) if len(so) > 1 else 0
    if mask is None:
        mask = pm.exposed_masks_batch(x, y, z, r, ids, so, probe, n_points, W)
    depth, nearest = np.zeros(n, F), np.zeros(n, np.uint32)
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        if e > b:
            _, depth[b:e], nearest[b:e] = split(keys_of(x[b:e], y[b:e], z[b:e], r[b:e], mask[b:e], probe, n_points))
    return depth, nearest, mask


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)
