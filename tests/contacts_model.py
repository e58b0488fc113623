"""An exact CPU model of the contact counts (rsasa_contact_points*): for each atom the hit matrix [K, n_points] of its
neighbour list against the lattice, built from the reference's own per-point occlusion tests (AtomSasaKernel,
reference src/lib.rs:129-146,183-207) on the oracle's lists, with the float32 expressions of points_model.py:
v = centre - neighbour, d^2 = (vx*vx + vy*vy) + vz*vz, R = r + probe, limit = (threshold_squared - d^2 - R*R) / (2 R);
a point p < n_points - n_points % W is hit when fmaf(sx, vx, fmaf(sy, vy, sz*vz)) < limit (tie_cases.fmaf_vec), a later
point when (sx*vx + sy*vy) + sz*vz <= limit.  covered = the sum of an entry's row; exclusive = its sum over the columns
that exactly one row of the atom hits.  No tolerance anywhere.

The two oracle checks (pair_check, deletion_check) tie counts to whole runs of the oracle on changed structures.
Plain helper module (not a conftest)."""
import numpy as np

import nb_helpers as nh
import tie_cases as tc
from oracle import pyoracle as po

F = np.float32
_BLOCK = 1 << 22  # entries x points evaluated at once (float64 temporaries of fmaf_vec: 32 MiB each)


def contact_counts_ws(x, y, z, r, ids, probe, n_points, Ws, lists=None):
    """(offsets, entries, {W: (covered uint32[total], exclusive uint32[total], buried int64[N])}) for one structure;
    buried[i] = the points of atom i that some entry hits.  `lists` (offsets, entries) defaults to the oracle's lists
    of calculate_sasa_internal, sorted by (d^2, idx).  The fused and remainder tests are evaluated once for all Ws."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    n = len(x)
    offs, ent = nh.oracle_csr(x, y, z, r, ids, probe) if lists is None else lists
    o = offs.astype(np.int64)
    total = int(o[-1])
    sx, sy, sz = po.sphere_points(n_points)
    nfs = {W: tc.n_fused(n_points, W) for W in Ws}
    f_hi, u_lo = max(nfs.values()), min(nfs.values())
    out = {W: (np.zeros(total, np.uint32), np.zeros(total, np.uint32), np.zeros(n, np.int64)) for W in Ws}
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(o))
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
        b = int(np.searchsorted(o, o[a] + step, side="right")) - 1
        b = min(max(b, a + 1), n)
        e0, e1 = o[a], o[b]
        if e1 > e0:
            cv = [t[e0:e1, None] for t in (vx, vy, vz, limit)]
            hit_f = hit_u = None
            with np.errstate(invalid="ignore", over="ignore"):
                if f_hi:
                    f = slice(0, f_hi)
                    dot = tc.fmaf_vec(sx[None, f], cv[0], tc.fmaf_vec(sy[None, f], cv[1], sz[None, f] * cv[2]))
                    hit_f = dot < cv[3]
                if u_lo < n_points:
                    u = slice(u_lo, n_points)
                    dot = sx[None, u] * cv[0] + sy[None, u] * cv[1] + sz[None, u] * cv[2]
                    assert dot.dtype == F
                    hit_u = dot <= cv[3]
            nonempty = np.nonzero(np.diff(o[a:b + 1]) > 0)[0]
            starts = o[a + nonempty] - e0
            seg = np.repeat(np.arange(len(starts)), np.diff(np.append(starts, e1 - e0)))  # entry -> its atom's row
            for W, nf in nfs.items():
                parts = ([hit_f[:, :nf]] if nf else []) + ([hit_u[:, nf - u_lo:]] if nf < n_points else [])
                hit = np.concatenate(parts, axis=1) if len(parts) > 1 else parts[0]
                per_point = np.add.reduceat(hit.astype(np.int32), starts, axis=0)  # [atoms, n_points]: entries hitting
                cov, exc, buried = out[W]
                cov[e0:e1] = hit.sum(axis=1)
                exc[e0:e1] = (hit & (per_point == 1)[seg]).sum(axis=1)
                buried[a + nonempty] = (per_point > 0).sum(axis=1)
        a = b
    return offs, ent, out


def contact_counts(x, y, z, r, ids, probe, n_points, W, lists=None):
    """(offsets, entries, covered, exclusive) of one structure at lane count W."""
    offs, ent, out = contact_counts_ws(x, y, z, r, ids, probe, n_points, (W,), lists)
    return offs, ent, out[W][0], out[W][1]


def contact_counts_batch(x, y, z, r, ids, so, probe, n_points, W):
    """(covered, exclusive) of every structure of a batch (one grid and one max radius each), in batch order - aligned
    with nb_helpers.oracle_batch_csr."""
    cov, exc = [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)]
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        if e > b:
            _, _, c, x_ = contact_counts(x[b:e], y[b:e], z[b:e], r[b:e], None if ids is None else ids[b:e], probe,
                                         n_points, W)
            cov.append(c)
            exc.append(x_)
    return np.concatenate(cov), np.concatenate(exc)


def _sub(cols, ids, sel):
    return [np.ascontiguousarray(a[sel]) for a in cols], None if ids is None else np.ascontiguousarray(ids[sel])


def pair_check(x, y, z, r, ids, probe, n_points, W, offs, ent, covered, n_pairs=400, seed=0):
    """For n_pairs seeded entries (i, j) of the lists: the oracle on the two-atom structure {i, j}.  When j is in that
    structure's list for i, n_points - (i's accessible points) must equal covered; when it is not, covered must be 0.
    Returns (pairs in the list, pairs not in it)."""
    o = offs.astype(np.int64)
    rng = np.random.default_rng(seed)
    picks = np.sort(rng.choice(int(o[-1]), size=min(n_pairs, int(o[-1])), replace=False))
    rows = np.searchsorted(o, picks, side="right") - 1
    n_in = n_out = 0
    for e, i in zip(picks.tolist(), rows.tolist()):
        j = int(ent["idx"][e])
        (px, py, pz, pr), pid = _sub((x, y, z, r), ids, [i, j])
        lists = po.neighbor_lists(px, py, pz, pr, pid, probe_radius=probe, max_radius=nh.fold_max(pr))
        _, pts, _ = po.calculate_sasa_internal(px, py, pz, pr, pid, probe, n_points, W, return_details=True)
        if len(lists[0]):
            assert int(covered[e]) == n_points - int(pts[0]), (i, j, int(covered[e]), n_points - int(pts[0]))
            n_in += 1
        else:
            assert int(covered[e]) == 0, (i, j, int(covered[e]))
            n_out += 1
    return n_in, n_out


def deletion_check(x, y, z, r, ids, probe, n_points, W, offs, ent, exclusive, n_del=12, seed=0):
    """For n_del seeded atoms j (skipping one that is the structure's only atom with the largest radius): the oracle on
    the structure without j.  Every other atom i must have pts_i + exclusive[(i, j)] accessible points, or pts_i when j
    is not in its list.  Returns the number of atoms compared."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    n = len(x)
    o = offs.astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(o))
    _, pts, _ = po.calculate_sasa_internal(x, y, z, r, ids, probe, n_points, W, return_details=True)
    rmax = F(nh.fold_max(r))
    rng = np.random.default_rng(seed)
    n_cmp = 0
    for j in rng.choice(n, size=min(n_del, n), replace=False).tolist():
        if r[j] == rmax and np.count_nonzero(r == rmax) == 1:
            continue
        keep = np.arange(n) != j
        (kx, ky, kz, kr), kid = _sub((x, y, z, r), ids, keep)
        _, pts_wo, _ = po.calculate_sasa_internal(kx, ky, kz, kr, kid, probe, n_points, W, return_details=True)
        gain = np.zeros(n, np.int64)
        m = ent["idx"].astype(np.int64) == j
        gain[rows[m]] = exclusive[m]
        want = (pts.astype(np.int64) + gain)[keep]
        bad = np.nonzero(pts_wo.astype(np.int64) != want)[0]
        assert len(bad) == 0, (j, bad[:10].tolist())
        n_cmp += n - 1
    return n_cmp
