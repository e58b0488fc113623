"""The lists of include/rustsasa_amd.h's rsasa_atoms_within* in numpy float32, every operation written out in the header's
order and nothing fused: the exact model the GPU lists are compared with byte for byte.

    lists / lists_batch   the definition, as CSR (offsets uint64[N + 1], entries WITHIN_DTYPE[total]), every list sorted
                          by the 64-bit key (bits(d2) << 32) | idx.  Structures of up to hse_model.DENSE atoms are
                          evaluated pair by pair; above that the candidates of a centre come from a scipy cKDTree ball
                          query at 1.01 C + 1e-3 - a superset of the pairs whose float32 d2 can be <= c2 - and the
                          float32 rule decides every one of them, so the tree never decides anything.
    brute64               the same lists from a float64 brute force (as sets of partners, and the band that says whether
                          float32 may decide a pair differently).

Plain helper module (not a conftest)."""
import numpy as np

import hse_model as hm
from hse_model import CENTRE, PARTNER, F, c2_of

WITHIN_DTYPE = np.dtype([("d2", "<f4"), ("idx", "<u4")])


def d2_of(cx, cy, cz, px, py, pz):
    """The header's d2 of the pairs (centre, partner) given by broadcasting."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = px - cx, py - cy, pz - cz
        d2 = dx * dx + dy * dy + dz * dz
    assert d2.dtype == F
    return d2


def keys(d2, idx):
    return (np.ascontiguousarray(d2, F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(idx).astype(np.uint64)


def _csr(n, rows, d2, idx):
    """Rows of (centre, d2, idx) in any order -> CSR with every list sorted by key."""
    rows = np.asarray(rows, np.int64)
    order = np.lexsort((keys(d2, idx), rows))
    entries = np.empty(len(rows), WITHIN_DTYPE)
    entries["d2"] = np.asarray(d2, F)[order]
    entries["idx"] = np.asarray(idx, np.uint32)[order]
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return offsets, entries


def lists(x, y, z, flags=None, cutoff=8.0, upper_only=False):
    """(offsets, entries) of ONE structure."""
    x, y, z = (np.ascontiguousarray(a, F) for a in (x, y, z))
    n = len(x)
    fl = hm._flags(flags, n)
    c2 = c2_of(cutoff)
    cen = np.flatnonzero(fl & CENTRE)
    par = np.flatnonzero(fl & PARTNER)
    rows, d2s, idxs = [], [], []
    if len(cen) and len(par):
        if n <= hm.DENSE or not np.isfinite(c2):
            step = max(1, hm._PAIRS // len(par))
            for a in range(0, len(cen), step):
                i = cen[a:a + step]
                d2 = d2_of(x[i, None], y[i, None], z[i, None], x[None, par], y[None, par], z[None, par])
                with np.errstate(invalid="ignore"):
                    hit = (d2 <= c2) & (i[:, None] != par[None, :])
                if upper_only:
                    hit &= par[None, :] > i[:, None]
                r, c = np.nonzero(hit)
                rows.append(i[r]); d2s.append(d2[r, c]); idxs.append(par[c])
        else:
            from scipy.spatial import cKDTree
            xyz = np.stack([x, y, z], -1).astype(np.float64)
            ok = np.isfinite(xyz).all(axis=1)           # (a NaN coordinate is in nobody's list and has an empty one)
            par = par[ok[par]]
            tree = cKDTree(xyz[par])
            reach = 1.01 * float(cutoff) + 1e-3
            for i in cen[ok[cen]]:
                j = par[np.asarray(tree.query_ball_point(xyz[i], reach), np.int64)]
                j = j[(j > i) if upper_only else (j != i)]
                d2 = d2_of(x[i], y[i], z[i], x[j], y[j], z[j])
                hit = d2 <= c2
                rows.append(np.full(int(hit.sum()), i)); d2s.append(d2[hit]); idxs.append(j[hit])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)  # noqa: E731
    return _csr(n, cat(rows, np.int64), cat(d2s, F), cat(idxs, np.uint32))


def lists_batch(x, y, z, so, flags=None, cutoff=8.0, upper_only=False):
    x, y, z = (np.ascontiguousarray(a, F) for a in (x, y, z))
    n = len(x)
    fl = hm._flags(flags, n)
    offs, ents, total = [np.zeros(1, np.uint64)], [], np.uint64(0)
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        o, en = lists(x[b:e], y[b:e], z[b:e], fl[b:e], cutoff, upper_only)
        offs.append(o[1:] + total)
        ents.append(en)
        total += o[-1]
    return np.concatenate(offs), (np.concatenate(ents) if ents else np.zeros(0, WITHIN_DTYPE))


def lengths(offsets):
    return np.diff(offsets.astype(np.int64))


def brute64(x, y, z, flags, cutoff, upper_only=False):
    """(partner sets per atom, band): the lists' members from float64 arithmetic on the float32 inputs; band is the
    smallest |d / C - 1| over the pairs - a pair nearer than 1e-4 to the cutoff may fall on the other side in float32.
    Finite input, C > 0."""
    xyz = np.stack([x, y, z], -1).astype(np.float64)
    n = len(x)
    fl = hm._flags(flags, n)
    d = xyz[None, :, :] - xyz[:, None, :]
    dist = np.sqrt((d * d).sum(-1))
    pair = ((fl[:, None] & CENTRE) != 0) & ((fl[None, :] & PARTNER) != 0) & ~np.eye(n, dtype=bool)
    if upper_only:
        pair &= np.arange(n)[None, :] > np.arange(n)[:, None]
    hit = pair & (dist <= float(cutoff))
    band = np.abs(dist[pair] / float(cutoff) - 1.0).min() if pair.any() else np.inf
    return [set(np.flatnonzero(hit[i]).tolist()) for i in range(n)], dist, band
