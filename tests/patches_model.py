"""An exact CPU model of the dot patches (rsasa_dot_patches*): the definition of include/rustsasa_amd.h followed
literally on geodesics_model.py.

    graph, weights, path length   those of the dot geodesics at the same link (gm.links_batch, gm.weights)
    pick k                        m = max dist_k in float32; stop when k == min(max_centres, D_s), or m is finite and
                                  m <= spacing; else c_k = the smallest dot with dist_k == m (numpy's argmax takes the
                                  first of equal values) and cover[k] = m
    dist_{k+1}                    gm.dijkstra from ALL centres so far, from scratch - nothing incremental here: that the
                                  kernel's incremental relaxation reaches these bits is what the tests show
    source                        gm.sources_of for the seed set `centres`, once at the end

Plain helper module (not a conftest)."""
import numpy as np

import geodesics_model as gm

F = np.float32
NONE = gm.NONE


def sample(loff, idx, w, spacing, max_centres=None, on_pick=None):
    """(centres uint32[K], cover float32[K], dist float32[D], source uint32[D]) of ONE structure whose lists are
    (loff int64[D + 1] from 0, idx within the structure, w).  on_pick(k, c, dist_before, dist_after): called per pick."""
    loff = np.asarray(loff, np.int64)
    n = len(loff) - 1
    k_max = n if max_centres is None else min(int(max_centres), n)
    spacing = F(spacing)
    dist = np.full(n, np.inf, F)
    seeds = np.zeros(n, np.uint8)
    centres, cover = [], []
    while len(centres) < k_max:
        m = dist.max()
        assert m.dtype == F
        if np.isfinite(m) and m <= spacing:
            break
        c = int(np.argmax(dist))
        assert dist[c] == m and not (dist[:c] == m).any()
        centres.append(c)
        cover.append(m)
        seeds[c] = 1
        after = gm.dijkstra(loff, idx, w, seeds)
        if on_pick is not None:
            on_pick(len(centres) - 1, c, dist, after)
        dist = after
    source = gm.sources_of(loff, idx, w, dist, seeds) if n else np.zeros(0, np.uint32)
    return np.array(centres, np.uint32), np.array(cover, F), dist, source


def patches_batch(x, y, z, r, ids, so, probe, n_points, link, spacing, max_centres=None, W=8, mask=None, lists=None):
    """(dot_offsets uint64[N + 1], centre_offsets uint64[S + 1], centres uint32[K], cover float32[K], dist float32[D],
    source uint32[D], mask) of every structure of a batch.  lists: gm.links_batch's result at the same arguments."""
    off, loff, ent, mask = lists if lists is not None else gm.links_batch(x, y, z, r, ids, so, probe, n_points, link, W, mask)
    D = int(off[-1])
    w = gm.weights(ent)
    dist, src = np.full(D, np.inf, F), np.full(D, NONE, np.uint32)
    c_off, cs, cv = [0], [np.zeros(0, np.uint32)], [np.zeros(0, F)]
    for s in range(len(so) - 1):
        b, e = int(off[int(so[s])]), int(off[int(so[s + 1])])
        if e > b:
            lo = loff[b:e + 1].astype(np.int64)
            sl = slice(int(lo[0]), int(lo[-1]))
            c, v, dist[b:e], src[b:e] = sample(lo - lo[0], ent["idx"][sl].astype(np.int64), w[sl], spacing, max_centres)
            cs.append(c)
            cv.append(v)
        c_off.append(c_off[-1] + (len(cs[-1]) if e > b else 0))
    return off, np.array(c_off, np.uint64), np.concatenate(cs), np.concatenate(cv), dist, src, mask
