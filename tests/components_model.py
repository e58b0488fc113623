"""An exact CPU model of the surface components (rsasa_surface_components*): the definition of include/rustsasa_amd.h
followed literally.

    dots    (j, k) with k in A_j, ordered by (j, k), numbered from 0 per structure
    q       = c_j + R_j * s_k per component, R_j = r_j + p                        (depth_model.dots_of)
    edge    dx = q_a.x - q_b.x, ...; d2 = dx*dx + dy*dy + dz*dz; d2 <= link * link (numpy float32: nothing is fused)
    label   the smallest dot number of the dot's connected component

Candidate pairs come from a float64 k-d tree over the float32 dots at link * (1 + 1e-5) + 1e-4, a superset of the real
edges (the float32 d2 of two dots differs from their exact squared distance by a few 2^-24 of itself, whatever the size
of the coordinates; they are kept below 10^6, raised from 10^4 for the cases of sweep_cases.py that sit at the
margins' limit near 2.15e5 A); each candidate is decided by the float32 expression.
Dots with a non-finite position have a NaN d2 against everybody and are left out of the tree.  The masks come from
points_model.py (pinned to the oracle).  A minimum over a set has no order: no tolerance anywhere.  Plain helper module
(not a conftest)."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

import depth_model as dm
import points_model as pm

F = np.float32


def edges_of(qx, qy, qz, link):
    """int64[E, 2]: the linked pairs a < b of the dots (qx, qy, qz), by the header's float32 test."""
    qx, qy, qz = (np.ascontiguousarray(a, F) for a in (qx, qy, qz))
    ok = np.flatnonzero(np.isfinite(qx) & np.isfinite(qy) & np.isfinite(qz))
    if len(ok) < 2:
        return np.zeros((0, 2), np.int64)
    # (the tree sees the float32 dots exactly, and the float32 d2 of two of them is within a few 2^-24 of the exact one
    # relative to itself at any magnitude; the bound only keeps 1e-4 well above a float64 ulp of the coordinates)
    assert max(np.abs(qx[ok]).max(), np.abs(qy[ok]).max(), np.abs(qz[ok]).max()) < 1e6
    pts = np.stack([qx[ok], qy[ok], qz[ok]], -1).astype(np.float64)
    cand = cKDTree(pts).query_pairs(float(link) * (1.0 + 1e-5) + 1e-4, output_type="ndarray")
    a, b = ok[cand[:, 0]], ok[cand[:, 1]]
    dx, dy, dz = qx[a] - qx[b], qy[a] - qy[b], qz[a] - qz[b]
    d2 = dx * dx + dy * dy + dz * dz
    link2 = F(link) * F(link)
    assert d2.dtype == F and link2.dtype == F
    keep = d2 <= link2
    return np.stack([np.minimum(a, b)[keep], np.maximum(a, b)[keep]], -1).astype(np.int64)


def labels_of(n_dots, edges):
    """uint32[n_dots]: per dot the smallest dot of its connected component."""
    if n_dots == 0:
        return np.zeros(0, np.uint32)
    g = coo_matrix((np.ones(len(edges), np.int8), (edges[:, 0], edges[:, 1])), shape=(n_dots, n_dots))
    _, comp = connected_components(g, directed=False)
    first = np.full(comp.max() + 1, n_dots, np.int64)
    np.minimum.at(first, comp, np.arange(n_dots))
    return first[comp].astype(np.uint32)


def components(x, y, z, r, ids, probe, n_points, link, W=8, mask=None, with_edges=False):
    """(dot_offsets uint64[N + 1], labels uint32[D], mask) of one structure; mask bool[N, n_points] defaults to
    points_model's.  with_edges: the edges (dot numbers) and the dots' owners come too."""
    if mask is None:
        mask = pm.exposed_masks(x, y, z, r, ids, probe, n_points, W)
    owner, qx, qy, qz = dm.dots_of(x, y, z, r, mask, probe, n_points)
    edges = edges_of(qx, qy, qz, link)
    off = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.uint64)
    labels = labels_of(len(owner), edges)
    return (off, labels, mask, edges, owner) if with_edges else (off, labels, mask)


def components_batch(x, y, z, r, ids, so, probe, n_points, link, W=8, mask=None):
    """(dot_offsets, labels, mask) of every structure of a batch: offsets batch-global, labels within the structure."""
    n = int(so[-1]) if len(so) > 1 else 0
    if mask is None:
        mask = pm.exposed_masks_batch(x, y, z, r, ids, so, probe, n_points, W)
    off = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.uint64)
    labels = np.zeros(int(off[n]), np.uint32)
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        if e > b:
            labels[int(off[b]):int(off[e])] = components(x[b:e], y[b:e], z[b:e], r[b:e], None, probe, n_points, link,
                                                         mask=mask[b:e])[1]
    return off, labels, mask


def sizes(labels):
    """(representatives, dots) of the components of one structure, largest first, ties to the smaller label."""
    rep, n = np.unique(labels, return_counts=True)
    order = np.lexsort((rep, -n))
    return rep[order], n[order]
