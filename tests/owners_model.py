"""An exact CPU model of the contact owners (rsasa_contact_owners*): the definition of include/rustsasa_amd.h taken
literally, on the oracle's lists and with the float32 expressions of contacts_model.py
(v = centre - neighbour, d^2 = (vx*vx + vy*vy) + vz*vz, R = r + probe, limit = (threshold_squared - d^2 - R*R) / (2 R)).

For atom i, position e of its list (sorted by (d^2, idx)) and lattice point p, the margin is
    m(e, p) = fmaf(sx, vx, fmaf(sy, vy, sz*vz)) - limit    for p < n_fused,
    m(e, p) = ((sx*vx + sy*vy) + sz*vz) - limit            for later points:
the same dot as the hit rule for that point, followed by one float32 subtraction, unfused (the hit rules: dot < limit
with the fused dot of tie_cases.fmaf_vec, dot <= limit for later points).  owner(p) is found by walking the list in order: entry e takes the point
if hit(e, p) and either nobody owns it yet or m(e, p) < m(owner, p).  Without NaN this is the hitting entry with the
smallest (m, e): the earlier position wins an exact tie, -0 and +0 tie, a NaN limit never hits and so never owns, a
free point has owner 0xFFFFFFFF.  owned[e] = #{p : owner(p) = e}.  No tolerance anywhere.

The walk is a loop over list positions, vectorised over the atoms of a block and the points.  Plain helper module (not
a conftest)."""
import numpy as np

import nb_helpers as nh
import tie_cases as tc
from oracle import pyoracle as po

F = np.float32
FREE = 0xFFFFFFFF
_BLOCK = 1 << 22  # entries x points evaluated at once (float64 temporaries of fmaf_vec: 32 MiB each)


def entry_terms(x, y, z, r, probe, offs, ent):
    """Per entry of the lists, in float32 as the kernels compute them: (rows, j, vx, vy, vz, d2, R, limit); rows / j
    are the atom that owns the list and the neighbour."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    o = offs.astype(np.int64)
    rows = np.repeat(np.arange(len(x), dtype=np.int64), np.diff(o))
    j = ent["idx"].astype(np.int64)
    probe = F(probe)
    with np.errstate(invalid="ignore", over="ignore"):
        vx, vy, vz = x[rows] - x[j], y[rows] - y[j], z[rows] - z[j]
        d2 = vx * vx + vy * vy + vz * vz
        R = r[rows] + probe
        limit = (ent["threshold_squared"].astype(F) - d2 - R * R) / (F(2.0) * R)
    assert limit.dtype == F and d2.dtype == F
    return rows, j, vx, vy, vz, d2, R, limit


def row_blocks(o, n_points):
    """(a, b): runs of whole rows of the CSR offsets o (int64) holding about _BLOCK / n_points entries each."""
    n = len(o) - 1
    step = max(1, _BLOCK // max(n_points, 1))
    a = 0
    while a < n:
        b = int(np.searchsorted(o, o[a] + step, side="right")) - 1
        b = min(max(b, a + 1), n)
        yield a, b
        a = b


def dots(terms, e0, e1, pts, f_hi, u_lo):
    """The two dot products of entries [e0, e1): fused over points [0, f_hi), plain over points [u_lo, n_points);
    None where the range is empty."""
    sx, sy, sz = pts
    vx, vy, vz = (t[e0:e1, None] for t in terms[2:5])
    dot_f = dot_u = None
    with np.errstate(invalid="ignore", over="ignore"):
        if f_hi:
            f = slice(0, f_hi)
            dot_f = tc.fmaf_vec(sx[None, f], vx, tc.fmaf_vec(sy[None, f], vy, sz[None, f] * vz))
        if u_lo < len(sx):
            u = slice(u_lo, len(sx))
            dot_u = sx[None, u] * vx + sy[None, u] * vy + sz[None, u] * vz
            assert dot_u.dtype == F
    return dot_f, dot_u


def hits_and_margins(dot_f, dot_u, limit, nf, u_lo, n_points):
    """(hit bool[E, n_points], m float32[E, n_points]) at n_fused = nf from dots()' products; limit: float32[E]."""
    lim = limit[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        parts_h, parts_m = [], []
        if nf:
            parts_h.append(dot_f[:, :nf] < lim)
            parts_m.append(dot_f[:, :nf] - lim)
        if nf < n_points:
            du = dot_u[:, nf - u_lo:]
            parts_h.append(du <= lim)
            parts_m.append(du - lim)
    hit = np.concatenate(parts_h, axis=1) if len(parts_h) > 1 else parts_h[0]
    m = np.concatenate(parts_m, axis=1) if len(parts_m) > 1 else parts_m[0]
    assert m.dtype == F
    return hit, m


def walk(hit, m, starts, sizes):
    """owner uint32[A, n_points] of A atoms whose lists are rows [starts[k], starts[k] + sizes[k]) of hit / m: the
    definition's walk over list positions."""
    A, n = len(starts), hit.shape[1]
    best_m = np.full((A, n), np.inf, F)
    best_e = np.full((A, n), FREE, np.uint32)
    for k in range(int(sizes.max(initial=0))):
        sel = np.nonzero(sizes > k)[0]
        idx = starts[sel] + k
        cur_m, cur_e = best_m[sel], best_e[sel]
        with np.errstate(invalid="ignore"):
            take = hit[idx] & ((cur_e == FREE) | (m[idx] < cur_m))
        best_m[sel] = np.where(take, m[idx], cur_m)
        best_e[sel] = np.where(take, np.uint32(k), cur_e)
    return best_e


def owners_ws(x, y, z, r, ids, probe, n_points, Ws, lists=None):
    """(offsets, entries, {W: (owned uint32[total], owner uint32[N, n_points])}) for one structure.  `lists`
    (offsets, entries) defaults to the oracle's lists of calculate_sasa_internal, sorted by (d^2, idx).  The dot
    products are evaluated once for all Ws."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    n = len(x)
    offs, ent = nh.oracle_csr(x, y, z, r, ids, probe) if lists is None else lists
    o = offs.astype(np.int64)
    total = int(o[-1])
    pts = po.sphere_points(n_points)
    nfs = {W: tc.n_fused(n_points, W) for W in Ws}
    f_hi, u_lo = max(nfs.values()), min(nfs.values())
    out = {W: (np.zeros(total, np.uint32), np.full((n, n_points), FREE, np.uint32)) for W in Ws}
    terms = entry_terms(x, y, z, r, probe, offs, ent)
    for a, b in row_blocks(o, n_points):
        e0, e1 = int(o[a]), int(o[b])
        if e1 == e0:
            continue
        dot_f, dot_u = dots(terms, e0, e1, pts, f_hi, u_lo)
        starts, sizes = o[a:b] - e0, np.diff(o[a:b + 1])
        # a point's owner depends on its own column alone: one walk per rule, the lane counts choose among the columns
        own_f = own_u = None
        if f_hi:
            own_f = walk(*hits_and_margins(dot_f, None, terms[7][e0:e1], f_hi, f_hi, f_hi), starts, sizes)
        if u_lo < n_points:
            own_u = walk(*hits_and_margins(None, dot_u, terms[7][e0:e1], 0, 0, n_points - u_lo), starts, sizes)
        for W, nf in nfs.items():
            parts = ([own_f[:, :nf]] if nf else []) + ([own_u[:, nf - u_lo:]] if nf < n_points else [])
            own = np.concatenate(parts, axis=1) if len(parts) > 1 else parts[0]
            owned, owner = out[W]
            owner[a:b] = own
            at, _ = np.nonzero(own != FREE)
            np.add.at(owned, e0 + starts[at] + own[own != FREE].astype(np.int64), 1)
    return offs, ent, out


def owners(x, y, z, r, ids, probe, n_points, W, lists=None):
    """(offsets, entries, owned, owner) of one structure at lane count W."""
    offs, ent, out = owners_ws(x, y, z, r, ids, probe, n_points, (W,), lists)
    return offs, ent, out[W][0], out[W][1]


def owners_batch(x, y, z, r, ids, so, probe, n_points, W):
    """(owned, owner) of every structure of a batch (one grid and one max radius each), in batch order - aligned with
    nb_helpers.oracle_batch_csr."""
    owned, owner = [np.zeros(0, np.uint32)], [np.zeros((0, n_points), np.uint32)]
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        if e > b:
            _, _, c, w = owners(x[b:e], y[b:e], z[b:e], r[b:e], None if ids is None else ids[b:e], probe, n_points, W)
            owned.append(c)
            owner.append(w)
    return np.concatenate(owned), np.concatenate(owner)
