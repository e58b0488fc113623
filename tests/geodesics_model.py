"""An exact CPU model of the dot links and the dot geodesics (rsasa_dot_links*, rsasa_dot_geodesics*): the definitions of
include/rustsasa_amd.h followed literally.

    dots, q, edge   exactly those of the surface components (components_model.edges_of: d2 <= link * link in float32)
    list of dot a   every other dot b of its structure with d2 <= link * link, as (d2, idx = b's dot number within the
                    structure), ascending by the key (bits(d2) << 32) | idx; both directions of every edge
    weight          The edge weight is w(a, b) = sqrtf(d2), correctly rounded (numpy's float32 sqrt).
    path length     The length of a path v0 ... vk is the left-to-right sum ((0 + w1) + w2) + ...
    dist[v]         dist[v] is the minimum over all paths from any seed to v whose length, and hence every prefix, is
                    <= limit; +inf where there is none.  A seed has dist 0.
    source[v]       the smallest seed dot number, within the structure, from which a path to v exists on which every
                    vertex is reached at exactly its dist (the trivial path included); 0xFFFFFFFF where dist is +inf

Float addition of a non-negative number is monotone and never decreases its left operand, so dist is the unique least
solution of dist[v] = min(seed ? 0 : inf, min_u fl(dist[u] + w(u, v))) with values > limit replaced by inf, and a heap
Dijkstra in np.float32 computes it: every comparison below is for equality.  source is the least fixed point of
source[v] = min(seed ? v : none, min over u with fl(dist[u] + w) == dist[v] finite of source[u]), iterated to rest.
The masks come from points_model.py (pinned to the oracle).  Plain helper module (not a conftest)."""
import heapq

import numpy as np

import components_model as cm
import depth_model as dm
import points_model as pm

F = np.float32
WITHIN = np.dtype([("d2", "<f4"), ("idx", "<u4")])
NONE = np.uint32(0xFFFFFFFF)


def lists_of(qx, qy, qz, link):
    """(link_offsets int64[D + 1], entries WITHIN[E]) of the dots (qx, qy, qz) of ONE structure."""
    qx, qy, qz = (np.ascontiguousarray(a, F) for a in (qx, qy, qz))
    n = len(qx)
    e = cm.edges_of(qx, qy, qz, link)
    a, b = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    dx, dy, dz = qx[a] - qx[b], qy[a] - qy[b], qz[a] - qz[b]
    d2 = dx * dx + dy * dy + dz * dz
    assert d2.dtype == F
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64)
    order = np.lexsort((key, a))
    ent = np.zeros(len(a), WITHIN)
    ent["d2"], ent["idx"] = d2[order], b[order]
    off = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=n))]).astype(np.int64)
    return off, ent


def links(x, y, z, r, ids, probe, n_points, link, W=8, mask=None):
    """(dot_offsets uint64[N + 1], link_offsets uint64[D + 1], entries, mask) of one structure."""
    if mask is None:
        mask = pm.exposed_masks(x, y, z, r, ids, probe, n_points, W)
    _, qx, qy, qz = dm.dots_of(x, y, z, r, mask, probe, n_points)
    off = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.uint64)
    loff, ent = lists_of(qx, qy, qz, link)
    return off, loff.astype(np.uint64), ent, mask


def links_batch(x, y, z, r, ids, so, probe, n_points, link, W=8, mask=None):
    """The same of every structure of a batch: both offsets batch-global, idx within the structure."""
    n = int(so[-1]) if len(so) > 1 else 0
    if mask is None:
        mask = pm.exposed_masks_batch(x, y, z, r, ids, so, probe, n_points, W)
    off = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.uint64)
    loffs, ents, base = [np.zeros(1, np.uint64)], [np.zeros(0, WITHIN)], 0
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        if e > b:
            _, lo, en, _ = links(x[b:e], y[b:e], z[b:e], r[b:e], None, probe, n_points, link, mask=mask[b:e])
            loffs.append(lo[1:] + np.uint64(base))
            ents.append(en)
            base += len(en)
    assert len(np.concatenate(loffs)) == int(off[n]) + 1
    return off, np.concatenate(loffs), np.concatenate(ents), mask


def weights(entries):
    w = np.sqrt(np.ascontiguousarray(entries["d2"], F))   # numpy's float32 sqrt is the correctly rounded one
    assert w.dtype == F
    return w


def dijkstra(link_offsets, idx, w, seeds, limit=np.inf, with_hops=False):
    """dist float32[D] of ONE structure (idx: dot numbers within it) by a heap Dijkstra in np.float32.  with_hops: and
    the number of edges of the path that gave each dist (0 where there is none)."""
    off = np.asarray(link_offsets, np.int64)
    n = len(off) - 1
    limit = F(limit)
    dist = np.full(n, np.inf, F)
    n_hops = np.zeros(n, np.int64)
    heap = []
    for s in np.flatnonzero(np.asarray(seeds) != 0):
        dist[s] = F(0.0)
        heap.append((0.0, int(s)))
    heapq.heapify(heap)
    while heap:
        d, u = heapq.heappop(heap)
        if d > dist[u]:
            continue
        v = idx[off[u]:off[u + 1]]
        nd = F(d) + w[off[u]:off[u + 1]]
        assert nd.dtype == F
        for k in np.flatnonzero((nd <= limit) & (nd < dist[v])):
            if nd[k] < dist[v[k]]:
                dist[v[k]] = nd[k]
                n_hops[v[k]] = n_hops[u] + 1
                heapq.heappush(heap, (float(nd[k]), int(v[k])))
    return (dist, n_hops) if with_hops else dist


def sources_of(link_offsets, idx, w, dist, seeds):
    """source uint32[D] of ONE structure: the tight-edge fixed point, iterated until nothing changes."""
    off = np.asarray(link_offsets, np.int64)
    n = len(off) - 1
    u = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    v = idx.astype(np.int64)
    with np.errstate(invalid="ignore"):
        tight = ((dist[u] + w) == dist[v]) & np.isfinite(dist[v])
    u, v = u[tight], v[tight]
    src = np.where(np.asarray(seeds) != 0, np.arange(n), int(NONE)).astype(np.int64)
    while True:
        new = src.copy()
        np.minimum.at(new, v, src[u])
        if np.array_equal(new, src):
            return src.astype(np.uint32)
        src = new


def geodesics_batch(x, y, z, r, ids, so, probe, n_points, link, seeds, limit=np.inf, W=8, mask=None, lists=None):
    """(dot_offsets uint64[N + 1], dist float32[D], source uint32[D], mask) of every structure of a batch; seeds: one byte
    per dot of the batch.  lists: links_batch's result at the same arguments, if the caller has it."""
    off, loff, ent, mask = lists if lists is not None else links_batch(x, y, z, r, ids, so, probe, n_points, link, W, mask)
    D = int(off[-1])
    seeds = np.asarray(seeds)
    assert seeds.shape == (D,)
    w = weights(ent)
    dist, src = np.full(D, np.inf, F), np.full(D, NONE, np.uint32)
    for s in range(len(so) - 1):
        b, e = int(off[int(so[s])]), int(off[int(so[s + 1])])
        if e > b:
            lo = loff[b:e + 1].astype(np.int64)
            sl = slice(int(lo[0]), int(lo[-1]))
            dist[b:e] = dijkstra(lo - lo[0], ent["idx"][sl], w[sl], seeds[b:e], limit)
            src[b:e] = sources_of(lo - lo[0], ent["idx"][sl], w[sl], dist[b:e], seeds[b:e])
    return off, dist, src, mask


def hops(link_offsets, idx, seeds):
    """int64[D]: the fewest edges from a seed to every dot of ONE structure (-1: none), breadth first."""
    off = np.asarray(link_offsets, np.int64)
    n = len(off) - 1
    out = np.full(n, -1, np.int64)
    front = np.flatnonzero(np.asarray(seeds) != 0)
    out[front] = 0
    k = 0
    while len(front):
        k += 1
        nb = np.unique(np.concatenate([idx[off[u]:off[u + 1]] for u in front]).astype(np.int64)) if len(front) else front
        front = nb[out[nb] < 0]
        out[front] = k
    return out
