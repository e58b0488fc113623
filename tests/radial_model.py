"""The radial counts of include/rustsasa_amd.h (rsasa_radial_counts*) in numpy float32, every operation written out in
the header's order and nothing fused: the exact model the GPU tables are compared with for equality.

    counts / counts_batch   the definition.  Structures of up to hse_model.DENSE atoms are evaluated pair by pair; above
                            that the candidates of a centre come from a scipy cKDTree ball query at 1.01 edges[-1] + 1e-3
                            - a superset of the pairs whose float32 d2 can be <= e2[-1] - and the float32 rule decides
                            every one of them, so the tree never decides anything.
    pairs_from_counts       the uint64 sums of the rows by (structure, class of the centre).
    brute64                 the same table from a float64 brute force, for inputs whose pair distances keep away from
                            every edge.
    sweep_counts            what k_radial_counts (radial.hip) does for one centre, shell by shell, on the emulated grid of
                            sweep_model.py: the row it would hold and the shell it stops after.

Plain helper module (not a conftest)."""
import numpy as np

import hse_model as hm
import sweep_model as sm

F = np.float32
PARTNER, CENTRE = 1, 2
MAX_CLASSES, MAX_BINS = 16, 32   # RSASA_RADIAL_MAX_CLASSES, RSASA_RADIAL_MAX_BINS
_PAIRS = 1 << 22                 # pairs evaluated at once


def e2_of(edges):
    """The squared edges: one float32 product each (may overflow to +inf, may underflow to 0)."""
    e = np.ascontiguousarray(edges, F)
    assert e.ndim == 1 and 1 <= len(e) <= MAX_BINS
    with np.errstate(over="ignore", under="ignore"):
        e2 = e * e
    assert e2.dtype == F
    return e2


def bins(cx, cy, cz, px, py, pz, e2):
    """(hit bool, bin int64) of the pairs (centre, partner) given by broadcasting: the header's arithmetic.  hit: d2 <=
    e2[-1]; bin: the smallest k with d2 <= e2[k], that is the number of k with e2[k] < d2 (e2 does not decrease)."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = px - cx, py - cy, pz - cz
        d2 = dx * dx + dy * dy + dz * dz
        assert d2.dtype == F
        hit = d2 <= e2[-1]
        k = np.zeros(d2.shape, np.int64)
        for edge in e2[:-1]:
            k += edge < d2
    return hit, k


def _flags(flags, n):
    return np.full(n, PARTNER | CENTRE, np.uint8) if flags is None else np.asarray(flags).astype(np.uint8)


def _classes(classes, n, n_classes):
    cl = np.zeros(n, np.int64) if classes is None else np.asarray(classes).astype(np.int64)
    assert cl.shape == (n,) and 1 <= n_classes <= MAX_CLASSES and (n == 0 or (0 <= cl.min() and cl.max() < n_classes))
    return cl


def _add(row_table, i, cl_j, hit, k, n_bins):
    """Adds the partners (classes cl_j [M], hit / k [R, M]) of the centres i [R] to their rows."""
    n_cells = row_table.shape[1] * n_bins
    cell = cl_j[None, :] * n_bins + k
    for a, row in enumerate(i):
        row_table[row] += np.bincount(cell[a][hit[a]], minlength=n_cells).astype(np.uint32).reshape(-1, n_bins)


def counts(x, y, z, edges, classes=None, n_classes=1, flags=None):
    """uint32[N, n_classes, n_bins] of ONE structure."""
    x, y, z = (np.ascontiguousarray(a, F) for a in (x, y, z))
    n = len(x)
    fl, cl, e2 = _flags(flags, n), _classes(classes, n, n_classes), e2_of(edges)
    n_bins = len(e2)
    out = np.zeros((n, n_classes, n_bins), np.uint32)
    cen = np.flatnonzero(fl & CENTRE)
    par = np.flatnonzero(fl & PARTNER)
    if len(cen) == 0 or len(par) == 0:
        return out
    if n <= hm.DENSE or not np.isfinite(e2[-1]):
        step = max(1, _PAIRS // len(par))
        for a in range(0, len(cen), step):
            i = cen[a:a + step]
            hit, k = bins(x[i, None], y[i, None], z[i, None], x[None, par], y[None, par], z[None, par], e2)
            _add(out, i, cl[par], hit & (i[:, None] != par[None, :]), k, n_bins)
        return out
    from scipy.spatial import cKDTree
    xyz = np.stack([x, y, z], -1).astype(np.float64)
    ok = np.isfinite(xyz).all(axis=1)           # (a NaN coordinate counts for nobody and gets a zero row)
    par = par[ok[par]]
    tree = cKDTree(xyz[par])
    reach = 1.01 * float(np.ascontiguousarray(edges, F)[-1]) + 1e-3
    for i in cen[ok[cen]]:
        j = par[np.asarray(tree.query_ball_point(xyz[i], reach), np.int64)]
        j = j[j != i]
        hit, k = bins(x[i], y[i], z[i], x[j], y[j], z[j], e2)
        _add(out, [i], cl[j], hit[None, :], k[None, :], n_bins)
    return out


def counts_batch(x, y, z, so, edges, classes=None, n_classes=1, flags=None):
    x, y, z = (np.ascontiguousarray(a, F) for a in (x, y, z))
    n = len(x)
    fl, cl = _flags(flags, n), _classes(classes, n, n_classes)
    out = np.zeros((n, n_classes, len(e2_of(edges))), np.uint32)
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        out[b:e] = counts(x[b:e], y[b:e], z[b:e], edges, cl[b:e], n_classes, fl[b:e])
    return out


def pairs_from_counts(table, so, classes=None):
    """uint64[S, C, C, B]: [s, a] is the sum of the rows of the atoms of structure s whose class is a."""
    table = np.asarray(table)
    n, n_classes, n_bins = table.shape
    cl = _classes(classes, n, n_classes)
    out = np.zeros((len(so) - 1, n_classes, n_classes, n_bins), np.uint64)
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        for a in range(n_classes):
            out[s, a] = table[b:e][cl[b:e] == a].astype(np.uint64).sum(axis=0, dtype=np.uint64)
    return out


def brute64(x, y, z, edges, classes, n_classes, flags):
    """(table, band): the table from float64 arithmetic on the float32 inputs; band is the smallest |d / e - 1| over the
    pairs and the edges e > 0 - a pair nearer than 1e-4 to an edge may fall in the other bin in float32.  Finite input,
    no coincident atoms, increasing edges."""
    xyz = np.stack([x, y, z], -1).astype(np.float64)
    n = len(x)
    fl, cl = _flags(flags, n), _classes(classes, n, n_classes)
    e = np.asarray(edges, F).astype(np.float64)
    d = xyz[None, :, :] - xyz[:, None, :]
    dist = np.sqrt((d * d).sum(-1))
    pair = ((fl[:, None] & CENTRE) != 0) & ((fl[None, :] & PARTNER) != 0) & ~np.eye(n, dtype=bool)
    band = min((np.abs(dist[pair] / v - 1.0).min() for v in e if v > 0), default=np.inf) if pair.any() else np.inf
    k = (e[None, None, :] < dist[:, :, None]).sum(-1)          # the edges below the distance: the bin, len(e) = beyond
    out = np.zeros((n, n_classes, len(e)), np.uint32)
    for i, j in zip(*np.nonzero(pair & (k < len(e)))):
        out[i, cl[j], k[i, j]] += 1
    return out, band


# ---- the sweep of k_radial_counts --------------------------------------------------------------------------------------

def sweep_counts(x, y, z, r, probe, edges, classes, n_classes, flags, sample, margins=None, half=0.5, **switches):
    """(rows uint32[len(sample), C, B], stop, by_rule, found) over the atoms `sample` of ONE structure, swept as the kernel
    sweeps them: the stop rule is hse_model.stop_shell at the last edge.  found[n]: the shells in which a counting
    partner of sample[n] was met (a sorted list)."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    n = len(x)
    fl, cl, e2 = _flags(flags, n), _classes(classes, n, n_classes), e2_of(edges)
    n_bins = len(e2)
    last = float(np.ascontiguousarray(edges, F)[-1])
    g = sm.grid(x, y, z, r, probe)
    if margins is None:
        margins = sm.margins_hold(x, y, z, r, probe)
    rows = np.zeros((len(sample), n_classes, n_bins), np.uint32)
    stop, by_rule, found = np.zeros(len(sample), np.int64), np.zeros(len(sample), bool), []
    for m, i in enumerate(sample):
        stop[m], by_rule[m] = hm.stop_shell(last, g.h, g.s_last(i), margins, half)
        shells = []
        if fl[i] & CENTRE:
            for s in range(int(stop[m]) + 1):
                for flat in sm.shell_steps(g, i, s, **switches)[0]:
                    j = g.order[flat]
                    j = j[(j != i) & ((fl[j] & PARTNER) != 0)]
                    hit, k = bins(x[i], y[i], z[i], x[j], y[j], z[j], e2)
                    _add(rows, [m], cl[j], hit[None, :], k[None, :], n_bins)
                    if hit.any():
                        shells.append(s)
        found.append(sorted(set(shells)))
    return rows, stop, by_rule, found
