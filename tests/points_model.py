"""An exact CPU model of the accessible-point masks (rsasa_accessible_points*): the reference's per-point decisions
(AtomSasaKernel, reference src/lib.rs:96-223) restated in numpy float32 on the oracle's neighbour lists and the
oracle's lattice.

Per list entry, in the reference's order (lib.rs:101-136): v = centre - neighbour, d^2 = (vx*vx + vy*vy) + vz*vz,
R = r + probe, limit = (threshold_squared - d^2 - R*R) / (2 R).  A point p < n_points - n_points % W is occluded when
some entry gives fmaf(sx, vx, fmaf(sy, vy, sz*vz)) < limit (tie_cases.fmaf_vec, the exact fmaf), a later point when
some entry gives (sx*vx + sy*vy) + sz*vz <= limit in plain float32.  Exposed = not occluded.  No tolerance anywhere.
Plain helper module (not a conftest)."""
import numpy as np

import nb_helpers as nh
import tie_cases as tc
from oracle import pyoracle as po

F = np.float32
_BLOCK = 1 << 22  # entries x points evaluated at once (float64 temporaries of fmaf_vec: 32 MiB each)


def words_of(n_points: int) -> int:
    return (n_points + 31) // 32


def sasa_of(r, probe, exposed, n_points):
    """((4 pi R^2) k) / n in the reference's float32 expression (lib.rs:220-222), k = exposed-point counts."""
    R = F(r) + F(probe) if np.isscalar(r) else np.asarray(r, F) + F(probe)
    R2 = R * R
    k = np.asarray(exposed).astype(F)
    with np.errstate(invalid="ignore"):
        return ((F(4.0) * F(np.pi)) * R2) * k * (F(1.0) / F(n_points))


def exposed_masks(x, y, z, r, ids, probe, n_points, W, lists=None):
    """bool[N, n_points]: point p of atom i is exposed.  One structure; `lists` (offsets, entries) defaults to the
    oracle's lists of calculate_sasa_internal (max_radius = fold(0, max) of the radii)."""
    return exposed_masks_ws(x, y, z, r, ids, probe, n_points, (W,), lists)[W]


def exposed_masks_ws(x, y, z, r, ids, probe, n_points, Ws, lists=None):
    """{W: exposed_masks(..., W)} for several lane counts at the cost of about one: occluded is an OR over the list
    per point, so the fused rule's OR over points [0, max n_fused) and the remainder rule's over [min n_fused,
    n_points) are taken once and each W takes its columns from them."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    n = len(x)
    offs, ent = nh.oracle_csr(x, y, z, r, ids, probe) if lists is None else lists
    offs = offs.astype(np.int64)
    sx, sy, sz = po.sphere_points(n_points)
    nfs = {W: tc.n_fused(n_points, W) for W in Ws}
    f_hi, u_lo = max(nfs.values()), min(nfs.values())
    occ_f = np.zeros((n, f_hi), bool)            # fused rule, points [0, f_hi)
    occ_u = np.zeros((n, n_points - u_lo), bool)  # remainder rule, points [u_lo, n_points)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(offs))
    j = ent["idx"].astype(np.int64)
    probe = F(probe)
    with np.errstate(invalid="ignore", over="ignore"):
        vx, vy, vz = x[rows] - x[j], y[rows] - y[j], z[rows] - z[j]
        d2 = vx * vx + vy * vy + vz * vz
        R = r[rows] + probe
        R2 = R * R
        limit = (ent["threshold_squared"].astype(F) - d2 - R2) / (F(2.0) * R)
    assert limit.dtype == F
    step = max(1, _BLOCK // max(n_points, 1))
    a = 0
    while a < n:
        # whole rows, about `step` entries
        b = int(np.searchsorted(offs, offs[a] + step, side="right")) - 1
        b = min(max(b, a + 1), n)
        e0, e1 = offs[a], offs[b]
        if e1 > e0:
            cv = [t[e0:e1, None] for t in (vx, vy, vz, limit)]
            nonempty = np.nonzero(np.diff(offs[a:b + 1]) > 0)[0]
            starts = offs[a + nonempty] - e0
            with np.errstate(invalid="ignore", over="ignore"):
                if f_hi:
                    f = slice(0, f_hi)
                    dot = tc.fmaf_vec(sx[None, f], cv[0], tc.fmaf_vec(sy[None, f], cv[1], sz[None, f] * cv[2]))
                    occ_f[a + nonempty] = np.logical_or.reduceat(dot < cv[3], starts, axis=0)
                if u_lo < n_points:
                    u = slice(u_lo, n_points)
                    dot = sx[None, u] * cv[0] + sy[None, u] * cv[1] + sz[None, u] * cv[2]
                    assert dot.dtype == F
                    occ_u[a + nonempty] = np.logical_or.reduceat(dot <= cv[3], starts, axis=0)
        a = b
    return {W: ~np.concatenate([occ_f[:, :nf], occ_u[:, nf - u_lo:]], axis=1) for W, nf in nfs.items()}


def exposed_masks_batch(x, y, z, r, ids, so, probe, n_points, W):
    """exposed_masks of every structure of a batch (one grid and one max radius each), rows in batch order."""
    out = np.zeros((int(so[-1]) if len(so) > 1 else 0, n_points), bool)
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        if e > b:
            out[b:e] = exposed_masks(x[b:e], y[b:e], z[b:e], r[b:e], None if ids is None else ids[b:e], probe,
                                     n_points, W)
    return out


def pack(mask):
    """bool[N, n_points] -> the engine's words uint32[N, (n_points + 31) // 32] (bit p & 31 of word p >> 5)."""
    n, p = mask.shape
    padded = np.zeros((n, words_of(p) * 32), bool)
    padded[:, :p] = mask
    return np.packbits(padded, axis=1, bitorder="little").view("<u4").astype(np.uint32)
