"""The lists of include/rustsasa_amd.h's rsasa_nearest_atoms*: the list rsasa_atoms_within defines (within_model.py, numpy
float32, nothing fused), cut at k - the exact model the GPU lists are compared with byte for byte.

    lists / lists_batch   the definition: within_model.lists at the same flags and cutoff (None: +inf), every list cut to
                          its first k entries.
    lists_by_sort         the same lists by an independent computation: per centre a stable argsort of the keys
                          (bits(d2) << 32) | idx over ALL partners, of which the first k eligible ones are taken.  It
                          never builds the whole within-lists, so it also serves structures too large for them.
    brute64               the k nearest partners from a float64 brute force, and the relative gap between the k-th and the
                          (k + 1)-th distance that says whether float32 may choose differently.
    sweep                 k_nearest (nearest.hip) emulated for single centres over sweep_model's grid and shells - NOT a
                          second brute force: the 64-candidate batches, the staging with its compaction trigger and bound,
                          the stop rule by counting.  Its keyword switches exist only so that the CPU tests can show that
                          a case bites; each is one way a kernel could be wrong.

Plain helper module (not a conftest)."""
from dataclasses import dataclass, field

import numpy as np

import hse_model as hm
import sweep_model as sm
import within_model as wm
from hse_model import CENTRE, PARTNER, F
from within_model import WITHIN_DTYPE

MAX_K = 256         # RSASA_NEAREST_MAX_K
K_NN_STAGE = 1024   # kNnStage (nearest.hip): keys a wave stages in LDS between compactions
WAVE = sm.WAVE
TRIGGER = K_NN_STAGE - WAVE + 1   # the smallest number of staged keys at which the next batch of 64 might not fit
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def _cutoff(cutoff):
    return np.inf if cutoff is None else cutoff


def truncate(offsets, entries, k):
    """Every list of a CSR cut to its first k entries."""
    off = offsets.astype(np.int64)
    n = np.minimum(np.diff(off), k)
    keep = (np.arange(len(entries)) - np.repeat(off[:-1], np.diff(off))) < k
    out = np.zeros(len(off), np.uint64)
    out[1:] = np.cumsum(n)
    return out, np.ascontiguousarray(entries[keep])


def lists(x, y, z, flags=None, k=16, cutoff=None):
    """(offsets, entries) of ONE structure."""
    return truncate(*wm.lists(x, y, z, flags, _cutoff(cutoff)), k)


def lists_by_sort(x, y, z, flags=None, k=16, cutoff=None):
    """lists() of ONE structure without the within-lists: keys over all partners, stable argsort, the first k eligible."""
    x, y, z = (np.ascontiguousarray(a, F) for a in (x, y, z))
    n = len(x)
    fl = hm._flags(flags, n)
    c2 = hm.c2_of(_cutoff(cutoff))
    cen, par = np.flatnonzero(fl & CENTRE), np.flatnonzero(fl & PARTNER)
    counts = np.zeros(n, np.int64)
    parts = []
    step = max(1, (1 << 22) // max(len(par), 1))
    for a in range(0, len(cen), step):
        i = cen[a:a + step]
        d2 = wm.d2_of(x[i, None], y[i, None], z[i, None], x[None, par], y[None, par], z[None, par])
        with np.errstate(invalid="ignore"):
            ok = (d2 <= c2) & (i[:, None] != par[None, :])
        key = wm.keys(d2, np.broadcast_to(par[None, :], d2.shape))
        key[~ok] = NONE                                      # (no entry has this key: idx < 2^31)
        if key.shape[1] > 8192:                              # wide rows: select the k smallest first (the keys are distinct)
            key = np.partition(key, min(k, key.shape[1]) - 1, axis=1)[:, :k]
        order = np.argsort(key, axis=1, kind="stable")[:, :k]
        first = np.take_along_axis(key, order, axis=1)
        for row, ii in zip(first, i):
            row = row[row != NONE]
            counts[ii] = len(row)
            parts.append(row)
    key = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
    entries = np.empty(len(key), WITHIN_DTYPE)
    entries["d2"] = (key >> np.uint64(32)).astype(np.uint32).view(F)
    entries["idx"] = (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum(counts)
    return offsets, entries


def lists_batch(x, y, z, so, flags=None, k=16, cutoff=None, by_sort=False):
    x, y, z = (np.ascontiguousarray(a, F) for a in (x, y, z))
    fl = hm._flags(flags, len(x))
    offs, ents, total = [np.zeros(1, np.uint64)], [], np.uint64(0)
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        o, en = (lists_by_sort if by_sort else lists)(x[b:e], y[b:e], z[b:e], fl[b:e], k, cutoff)
        offs.append(o[1:] + total)
        ents.append(en)
        total += o[-1]
    return np.concatenate(offs), (np.concatenate(ents) if ents else np.zeros(0, WITHIN_DTYPE))


def brute64(x, y, z, flags, k):
    """(partners per atom in order of float64 distance, dist, band): the k nearest partners of every centre from float64
    arithmetic on the float32 inputs (no cutoff); band is the smallest relative gap d_(k+1) / d_k - 1 over the centres
    with more than k partners - below 1e-4 float32 may pick the other one.  Finite input."""
    xyz = np.stack([x, y, z], -1).astype(np.float64)
    n = len(x)
    fl = hm._flags(flags, n)
    d = xyz[None, :, :] - xyz[:, None, :]
    dist = np.sqrt((d * d).sum(-1))
    out, band = [], np.inf
    for i in range(n):
        if not fl[i] & CENTRE:
            out.append([])
            continue
        j = np.flatnonzero(((fl & PARTNER) != 0) & (np.arange(n) != i))
        j = j[np.argsort(dist[i, j], kind="stable")]
        if len(j) > k:
            band = min(band, dist[i, j[k]] / dist[i, j[k - 1]] - 1.0)
        out.append(j[:k].tolist())
    return out, dist, band


# ---- k_nearest, emulated ---------------------------------------------------------------------------------------------------

def cutoff_reached(margins, s, h, c2, lim_shift=-0.5):
    """sh_cutoff_reached (cutoff_sweep.h) in float32, for one c2 or an array of them.  lim_shift -0.5 is the rule;
    +0.5 is the rule relaxed by one shell."""
    if not (margins and s >= 1):
        return np.zeros(np.shape(c2), bool) if np.ndim(c2) else False
    lim = (F(s) + F(lim_shift)) * F(h)
    lim2 = lim * lim
    with np.errstate(invalid="ignore"):
        return (np.asarray(c2, F) <= lim2) & bool(lim2 >= F(1e-30))


def grid(x, y, z, r, probe):
    """sweep_model.grid, and for a structure with NaN coordinates the grid the engine builds for it: fminf / fmaxf pass
    over a NaN, and a NaN coordinate falls into cell 0 of its axis (f2u_sat).  (Such a structure fails the margins, so
    its sweeps cover the whole grid whatever the cells are.)"""
    nan = np.isnan(x) | np.isnan(y) | np.isnan(z)
    if not nan.any():
        return sm.grid(x, y, z, r, probe)
    h = F(probe) + np.max(r)
    inv = F(1.0) / h
    mn = np.array([np.fmin.reduce(a) for a in (x, y, z)], F) - h
    mx = np.array([np.fmax.reduce(a) for a in (x, y, z)], F) + h
    dims = np.ceil((mx - mn) * inv).astype(np.int64) + 1
    with np.errstate(invalid="ignore"):
        cells = np.stack([np.where(np.isnan(a), 0, np.minimum(np.nan_to_num((a - mn[k]) * inv).astype(np.int64), dims[k] - 1))
                          for k, a in enumerate((x, y, z))], -1)
    idx = cells[:, 0] + cells[:, 1] * dims[0] + cells[:, 2] * dims[0] * dims[1]
    order = np.argsort(idx, kind="stable")
    pos = np.empty_like(order)
    pos[order] = np.arange(len(order))
    starts = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=int(dims.prod())))]).astype(np.int64)
    return sm.Grid(h, dims, cells, order, pos, starts)


@dataclass
class Sweep:
    """What sweep() returns: per sampled centre its list, the shell it stopped after and why, the staged keys at each
    compaction, and the most keys the staging ever held."""
    lists: list = field(default_factory=list)          # WITHIN_DTYPE arrays
    stop: list = field(default_factory=list)           # the shell the sweep stopped after
    by_rule: list = field(default_factory=list)        # "cutoff", "kth" or "" (the shells covered the grid)
    compactions: list = field(default_factory=list)    # per centre: the keys held at each compaction
    most_held: list = field(default_factory=list)


def sweep(x, y, z, r, probe, flags=None, k=16, cutoff=None, sample=None, lim_shift=-0.5, keep_unsorted=False,
          stage=K_NN_STAGE, margins=None):
    """The sweeps of the centres `sample` (None: every centre) of ONE structure.
    lim_shift +0.5: the stop rule relaxed by one shell.  keep_unsorted: a compaction keeps the first k staged keys as
    they stand instead of the k smallest."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    n = len(x)
    fl = hm._flags(flags, n)
    c2 = hm.c2_of(_cutoff(cutoff))
    g = grid(x, y, z, r, probe)
    if margins is None:
        margins = sm.margins_hold(x, y, z, r, probe)
    out = Sweep()
    for i in (np.flatnonzero(fl & CENTRE) if sample is None else sample):
        i = int(i)
        assert fl[i] & CENTRE
        s_last = g.s_last(i)
        held = np.zeros(0, np.uint64)
        bound, comp, most, s, why = NONE, [], 0, 0, ""
        while True:
            for flat in sm.shell_steps(g, i, s)[0]:
                for f0 in range(0, len(flat), WAVE):
                    if len(held) + WAVE > stage:                       # the next 64 might not fit
                        comp.append(len(held))
                        held = (held if keep_unsorted else np.sort(held))[:k]
                        bound = held[k - 1]
                    j = g.order[flat[f0:f0 + WAVE]]
                    d2 = wm.d2_of(x[i], y[i], z[i], x[j], y[j], z[j])
                    with np.errstate(invalid="ignore"):
                        acc = (j != i) & ((fl[j] & PARTNER) != 0) & (d2 <= c2)
                    cand = wm.keys(d2, j)
                    acc &= cand <= bound
                    held = np.concatenate([held, cand[acc]])
                    assert len(held) <= stage
                    most = max(most, len(held))
            if s >= s_last:
                break
            if cutoff_reached(margins, s, g.h, c2, lim_shift):
                why = "cutoff"
                break
            if margins and s >= 1 and len(held) >= k:
                d2_held = (held >> np.uint64(32)).astype(np.uint32).view(F)
                if int(cutoff_reached(margins, s, g.h, d2_held, lim_shift).sum()) >= k:
                    why = "kth"
                    break
            s += 1
        key = np.sort(held)[:k]
        li = np.empty(len(key), WITHIN_DTYPE)
        li["d2"] = (key >> np.uint64(32)).astype(np.uint32).view(F)
        li["idx"] = (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        out.lists.append(li)
        out.stop.append(s)
        out.by_rule.append(why)
        out.compactions.append(comp)
        out.most_held.append(most)
    return out
