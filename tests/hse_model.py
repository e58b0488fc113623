"""The half-sphere exposure of include/rustsasa_amd.h (rsasa_half_sphere_exposure*) in numpy float32, every operation
written out in the header's order and nothing fused: the exact model the GPU counts are compared with for equality.

    counts / counts_batch   the definition.  Structures of up to DENSE atoms are evaluated pair by pair; above that the
                            candidates of a centre come from a scipy cKDTree ball query at 1.01 C + 1e-3 - a superset of
                            the pairs whose float32 d2 can be <= c2 - and the float32 rule decides every one of them, so
                            the tree never decides anything.
    brute64                 the same counts from a float64 brute force, for inputs whose pair distances keep away from C.
    sweep_counts            what k_half_sphere (hse.hip) does for one centre, shell by shell, on the emulated grid of
                            sweep_model.py: the counts it would hold and the shell it stops after.

Plain helper module (not a conftest)."""
import numpy as np

import sweep_model as sm

F = np.float32
PARTNER, CENTRE = 1, 2
DENSE = 6000       # atoms up to which a structure is evaluated pair by pair
_PAIRS = 1 << 22   # pairs evaluated at once


def c2_of(cutoff):
    with np.errstate(over="ignore"):
        return F(cutoff) * F(cutoff)


def rule(cx, cy, cz, ux, uy, uz, px, py, pz, c2):
    """(up, down) bool arrays of the pairs (centre, partner) given by broadcasting: the header's arithmetic.  ux None:
    side is +0 for everybody."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = px - cx, py - cy, pz - cz
        d2 = dx * dx + dy * dy + dz * dz
        assert d2.dtype == F
        hit = d2 <= c2
        if ux is None:
            return hit, np.zeros_like(hit)
        side = dx * ux + dy * uy + dz * uz
        assert side.dtype == F
        above = side >= F(0.0)
    return hit & above, hit & ~above


def _flags(flags, n):
    return np.full(n, PARTNER | CENTRE, np.uint8) if flags is None else np.asarray(flags).astype(np.uint8)


def _dirs(dirs, n):
    if dirs is None:
        return None
    d = np.ascontiguousarray(dirs, F)
    assert d.shape == (n, 3)
    return d


def counts(x, y, z, dirs=None, flags=None, cutoff=13.0):
    """(up uint32[N], down uint32[N]) of ONE structure."""
    x, y, z = (np.ascontiguousarray(a, F) for a in (x, y, z))
    n = len(x)
    fl, d = _flags(flags, n), _dirs(dirs, n)
    c2 = c2_of(cutoff)
    up, down = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    cen = np.flatnonzero(fl & CENTRE)
    par = np.flatnonzero(fl & PARTNER)
    if len(cen) == 0 or len(par) == 0:
        return up, down
    if n <= DENSE or not np.isfinite(c2):
        step = max(1, _PAIRS // len(par))
        for a in range(0, len(cen), step):
            i = cen[a:a + step]
            u = (None,) * 3 if d is None else (d[i, 0, None], d[i, 1, None], d[i, 2, None])
            um, dm_ = rule(x[i, None], y[i, None], z[i, None], *u, x[None, par], y[None, par], z[None, par], c2)
            notself = i[:, None] != par[None, :]
            up[i] = (um & notself).sum(axis=1)
            down[i] = (dm_ & notself).sum(axis=1)
        return up, down
    from scipy.spatial import cKDTree
    xyz = np.stack([x, y, z], -1).astype(np.float64)
    ok = np.isfinite(xyz).all(axis=1)           # (a NaN coordinate counts for nobody and gets 0 / 0)
    par = par[ok[par]]
    tree = cKDTree(xyz[par])
    reach = 1.01 * float(cutoff) + 1e-3
    for i in cen[ok[cen]]:
        j = par[np.asarray(tree.query_ball_point(xyz[i], reach), np.int64)]
        j = j[j != i]
        u = (None,) * 3 if d is None else (d[i, 0], d[i, 1], d[i, 2])
        um, dm_ = rule(x[i], y[i], z[i], *u, x[j], y[j], z[j], c2)
        up[i], down[i] = um.sum(), dm_.sum()
    return up, down


def counts_batch(x, y, z, so, dirs=None, flags=None, cutoff=13.0):
    x, y, z = (np.ascontiguousarray(a, F) for a in (x, y, z))
    n = len(x)
    fl, d = _flags(flags, n), _dirs(dirs, n)
    up, down = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        up[b:e], down[b:e] = counts(x[b:e], y[b:e], z[b:e], None if d is None else d[b:e], fl[b:e], cutoff)
    return up, down


def brute64(x, y, z, dirs, flags, cutoff):
    """(up, down, band, side_band): the counts from float64 arithmetic on the float32 inputs; band is the smallest
    |d / C - 1| over the pairs and side_band the smallest |side| / (d |u|) over the pairs that count - a pair nearer than
    1e-4 to the cutoff, or to the plane, may fall on the other side in float32.  Finite input, no zero direction, no
    coincident atoms, C > 0."""
    xyz = np.stack([x, y, z], -1).astype(np.float64)
    u = np.asarray(dirs, np.float64)
    n = len(x)
    fl = _flags(flags, n)
    d = xyz[None, :, :] - xyz[:, None, :]                      # [i, j] = c_j - c_i
    dist = np.sqrt((d * d).sum(-1))
    side = (d * u[:, None, :]).sum(-1)
    pair = ((fl[:, None] & CENTRE) != 0) & ((fl[None, :] & PARTNER) != 0) & ~np.eye(n, dtype=bool)
    hit = pair & (dist <= float(cutoff))
    band = np.abs(dist[pair] / float(cutoff) - 1.0).min() if pair.any() else np.inf
    rel = np.abs(side) / np.where(hit, dist * np.linalg.norm(u, axis=1)[:, None], 1.0)
    side_band = rel[hit].min() if hit.any() else np.inf
    return (hit & (side >= 0)).sum(1).astype(np.uint32), (hit & ~(side >= 0)).sum(1).astype(np.uint32), band, side_band


# ---- the sweep of k_half_sphere ----------------------------------------------------------------------------------------

def stop_shell(cutoff, h, s_last, margins, half=0.5):
    """The shell k_half_sphere stops after (float32, as written in hse.hip) and whether the rule stopped it."""
    c2 = c2_of(cutoff)
    s = 0
    while True:
        if s >= s_last:
            return s, False
        if margins and s >= 1:
            lim = (F(s) - F(half)) * F(h)
            lim2 = lim * lim
            if c2 <= lim2 and lim2 >= F(1e-30):
                return s, True
        s += 1


def sweep_counts(x, y, z, r, probe, dirs, flags, cutoff, sample, margins=None, half=0.5, **switches):
    """(up, down, stop, by_rule, found) over the atoms `sample` of ONE structure, swept as the kernel sweeps them.
    found[n]: the shells in which a counting partner of sample[n] was met (a sorted list)."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    n = len(x)
    fl, d = _flags(flags, n), _dirs(dirs, n)
    g = sm.grid(x, y, z, r, probe)
    if margins is None:
        margins = sm.margins_hold(x, y, z, r, probe)
    c2 = c2_of(cutoff)
    up, down = np.zeros(len(sample), np.uint32), np.zeros(len(sample), np.uint32)
    stop, by_rule, found = np.zeros(len(sample), np.int64), np.zeros(len(sample), bool), []
    for k, i in enumerate(sample):
        stop[k], by_rule[k] = stop_shell(cutoff, g.h, g.s_last(i), margins, half)
        shells = []
        if fl[i] & CENTRE:
            u = (None,) * 3 if d is None else tuple(d[i])
            for s in range(int(stop[k]) + 1):
                for flat in sm.shell_steps(g, i, s, **switches)[0]:
                    j = g.order[flat]
                    j = j[(j != i) & ((fl[j] & PARTNER) != 0)]
                    um, dm_ = rule(x[i], y[i], z[i], *u, x[j], y[j], z[j], c2)
                    up[k] += um.sum()
                    down[k] += dm_.sum()
                    if um.any() or dm_.any():
                        shells.append(s)
        found.append(sorted(set(shells)))
    return up, down, stop, by_rule, found
