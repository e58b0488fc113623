"""The dot crowding of include/rustsasa_amd.h (rsasa_dot_crowding*) in numpy float32, every operation written out in the
header's order and nothing fused: the exact model the GPU rows are compared with for equality.

    R_i = r_i + p;  q = c_i + R_i * s_k (per component);  dx = c_j.x - q.x;  d2 = (dx*dx + dy*dy) + dz*dz
    j counts for the dot iff (flags[j] & 1) and d2 <= e2[-1];  bin = the smallest b with d2 <= e2[b]

    counts / counts_batch   the definition: depth_model.dots_of for the dots (the order of surface_points and of
                            surface_components), radial_model.bins for the rule, every (dot, partner) pair of a structure.
                            A structure of more than hse_model.DENSE atoms takes a dot's candidates from a cKDTree ball
                            query at 1.01 edges[-1] + 1e-3 - a superset of what float32 can accept - and the float32 rule
                            decides every one of them.
    brute64                 the same table from float64 arithmetic, for inputs whose distances keep away from every edge.
    stop_shell, sweep_counts  what k_dot_crowding (crowding.hip) does for the dots of one atom, shell by shell, on the
                            emulated grid of sweep_model.py, with a switch that stops one shell early.

The masks come from points_model.py (pinned to the oracle).  Plain helper module (not a conftest)."""
import numpy as np

import depth_model as dm
import hse_model as hm
import points_model as pm
import radial_model as rm
import sweep_model as sm

F = np.float32
PARTNER = 1
MAX_BINS = 8       # RSASA_CROWD_MAX_BINS
_PAIRS = 1 << 22   # (dot, partner) pairs evaluated at once


def e2_of(edges):
    e2 = rm.e2_of(edges)
    assert len(e2) <= MAX_BINS
    return e2


def _partners(flags, n):
    return np.arange(n) if flags is None else np.flatnonzero(np.asarray(flags).astype(np.uint8) & PARTNER)


def offsets_of(mask):
    """uint64[N + 1]: the exclusive scan of the masks' popcounts."""
    return np.concatenate([[0], np.cumsum(mask.sum(axis=1, dtype=np.int64))]).astype(np.uint64)


def rows_of(qx, qy, qz, x, y, z, par, e2):
    """uint32[D, B]: the rows of the dots q against the partners `par` (indices into x, y, z)."""
    n_bins = len(e2)
    out = np.zeros((len(qx), n_bins), np.uint32)
    if len(qx) == 0 or len(par) == 0:
        return out
    step = max(1, _PAIRS // len(par))
    for a in range(0, len(qx), step):
        sl = slice(a, a + step)
        hit, k = rm.bins(qx[sl, None], qy[sl, None], qz[sl, None], x[None, par], y[None, par], z[None, par], e2)
        for m in range(hit.shape[0]):
            out[a + m] = np.bincount(k[m][hit[m]], minlength=n_bins).astype(np.uint32)
    return out


def counts(x, y, z, r, mask, probe, n_points, edges, flags=None):
    """(dot_offsets uint64[N + 1], counts uint32[D, B]) of ONE structure with the masks bool[N, n_points]."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    e2 = e2_of(edges)
    par = _partners(flags, len(x))
    owner, qx, qy, qz = dm.dots_of(x, y, z, r, mask, probe, n_points)
    off = offsets_of(mask)
    assert len(owner) == int(off[-1])
    if len(x) <= hm.DENSE or not np.isfinite(e2[-1]):
        return off, rows_of(qx, qy, qz, x, y, z, par, e2)
    from scipy.spatial import cKDTree
    xyz = np.stack([x, y, z], -1).astype(np.float64)
    par = par[np.isfinite(xyz[par]).all(axis=1)]            # (a NaN partner counts for nobody)
    out = np.zeros((len(owner), len(e2)), np.uint32)
    if len(par) == 0:
        return off, out
    tree = cKDTree(xyz[par])
    q = np.stack([qx, qy, qz], -1).astype(np.float64)
    ok = np.flatnonzero(np.isfinite(q).all(axis=1))         # (a NaN dot has a zero row)
    reach = 1.01 * float(np.ascontiguousarray(edges, F)[-1]) + 1e-3
    for d, near in zip(ok, tree.query_ball_point(q[ok], reach)):
        j = par[np.asarray(near, np.int64)]
        hit, k = rm.bins(qx[d], qy[d], qz[d], x[j], y[j], z[j], e2)
        out[d] = np.bincount(k[hit], minlength=len(e2)).astype(np.uint32)
    return off, out


def counts_batch(x, y, z, r, so, mask, probe, n_points, edges, flags=None):
    """(dot_offsets uint64[N + 1] batch-global, counts uint32[D, B]) of every structure of a batch."""
    n = int(so[-1]) if len(so) > 1 else 0
    rows = [np.zeros((0, len(e2_of(edges))), np.uint32)]
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        if e > b:
            rows.append(counts(x[b:e], y[b:e], z[b:e], r[b:e], mask[b:e], probe, n_points, edges,
                               None if flags is None else np.asarray(flags)[b:e])[1])
    return offsets_of(mask[:n]), np.concatenate(rows)


def model_batch(x, y, z, r, ids, so, probe, n_points, edges, flags=None, W=8):
    """counts_batch with points_model's masks: (dot_offsets, counts, mask)."""
    mask = pm.exposed_masks_batch(x, y, z, r, ids, so, probe, n_points, W)
    return counts_batch(x, y, z, r, so, mask, probe, n_points, edges, flags) + (mask,)


def brute64(x, y, z, r, mask, probe, n_points, edges, flags=None):
    """(counts, band float64[D]): the rows from float64 arithmetic on the float32 inputs and lattice; band[d] is the
    smallest |distance - e| over the partners of dot d and the edges e.  Finite input, increasing edges."""
    from oracle import pyoracle as po
    s = np.stack([np.asarray(a, F) for a in po.sphere_points(n_points)], -1).astype(np.float64)
    xyz = np.stack([x, y, z], -1).astype(np.float64)
    R = np.asarray(r, F).astype(np.float64) + float(F(probe))
    i, k = np.nonzero(mask)
    q = xyz[i] + R[i, None] * s[k]
    par = _partners(flags, len(x))
    e = np.asarray(edges, F).astype(np.float64)
    out = np.zeros((len(i), len(e)), np.uint32)
    if len(i) == 0 or len(par) == 0:
        return out, np.full(len(i), np.inf)
    d = np.sqrt(((xyz[par][None, :, :] - q[:, None, :]) ** 2).sum(-1))
    band = np.abs(d[:, :, None] - e[None, None, :]).min(axis=(1, 2))
    b = (e[None, None, :] < d[:, :, None]).sum(-1)
    for m in range(len(i)):
        out[m] = np.bincount(b[m][b[m] < len(e)], minlength=len(e)).astype(np.uint32)
    return out, band


# ---- the sweep of k_dot_crowding ---------------------------------------------------------------------------------------

def stop_shell(last_edge, h, s_last, margins, early=False):
    """(the shell k_dot_crowding stops after, whether the rule stopped it): float32, as written in crowding.hip - after
    shell s >= 2 when e2[-1] <= lim2, lim = (float(s) - 1.5f) * h, lim2 >= 1e-30.  early: the rule with 0.5 in place
    of 1.5 from shell 1 on, which is met one shell sooner - a kernel that forgot the dots' distance from their atom."""
    with np.errstate(over="ignore", under="ignore"):
        c2 = F(last_edge) * F(last_edge)
    s = 0
    while True:
        if s >= s_last:
            return s, False
        if margins and s >= (1 if early else 2):
            lim = (F(s) - F(0.5 if early else 1.5)) * F(h)
            lim2 = lim * lim
            if c2 <= lim2 and lim2 >= F(1e-30):
                return s, True
        s += 1


def sweep_counts(x, y, z, r, mask, probe, n_points, edges, flags, sample, margins=None, early=False, **switches):
    """(rows {atom: uint32[free, B]}, stop int64[len(sample)], by_rule bool[...], found [sorted shells]) for the dots of
    the atoms `sample` of ONE structure, swept as the kernel sweeps them; found[n]: the shells in which some dot of
    sample[n] met a counting partner."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    n = len(x)
    e2 = e2_of(edges)
    fl = np.full(n, PARTNER, np.uint8) if flags is None else np.asarray(flags).astype(np.uint8)
    last = float(np.ascontiguousarray(edges, F)[-1])
    g = sm.grid(x, y, z, r, probe)
    if margins is None:
        margins = sm.margins_hold(x, y, z, r, probe)
    owner, qx, qy, qz = dm.dots_of(x, y, z, r, mask, probe, n_points)
    rows, found = {}, []
    stop, by_rule = np.zeros(len(sample), np.int64), np.zeros(len(sample), bool)
    for m, i in enumerate(sample):
        stop[m], by_rule[m] = stop_shell(last, g.h, g.s_last(i), margins, early)
        mine = np.flatnonzero(owner == i)
        row = np.zeros((len(mine), len(e2)), np.uint32)
        shells = []
        if len(mine):
            for s in range(int(stop[m]) + 1):
                for flat in sm.shell_steps(g, i, s, **switches)[0]:
                    j = g.order[flat]
                    j = j[(fl[j] & PARTNER) != 0]
                    add = rows_of(qx[mine], qy[mine], qz[mine], x, y, z, j, e2)
                    row += add
                    if add.any():
                        shells.append(s)
        rows[int(i)] = row
        found.append(sorted(set(shells)))
    return rows, stop, by_rule, found
