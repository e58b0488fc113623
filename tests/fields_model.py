"""The dot fields of include/rustsasa_amd.h (rsasa_dot_fields*) in numpy float32, every operation written out in the
header's order and nothing fused: the exact model the GPU rows are compared with for equality.

    R_i = r_i + p;  q = c_i + R_i * s_k (per component);  dx = c_j.x - q.x;  d2 = (dx*dx + dy*dy) + dz*dz;  d = sqrtf(d2)
    j counts for the dot iff (flags[j] & 1) and d2 <= c2 = cutoff * cutoff
    g = 1 | 1 / d | 1 / d2 | 1 / (1 + d);  t = w[j][c] * g[kinds[c]];  |t| <= 2^24:  sums[dot][c] += rint(t * 2^24)  (int64, wraps)

numpy's float32 division and square root are correctly rounded and keep subnormals, as the header asks of the device.

    sums / sums_batch       the definition: depth_model.dots_of for the dots (the order of surface_points and of
                            dot_crowding's rows), every (dot, partner) pair of a structure.  A structure of more than
                            hse_model.DENSE atoms takes a dot's candidates from a cKDTree ball query at 1.01 cutoff + 1e-3
                            - a superset of what float32 can accept - and the float32 rule decides every one of them.
    brute64                 the same sums as float64 numbers from float64 arithmetic, with the sum of the terms' magnitudes,
                            the number of terms and the nearest a partner comes to the cutoff.
    sweep_sums              what k_dot_fields (fields.hip) does for the dots of one atom, shell by shell, on the emulated grid
                            of sweep_model.py under crowding_model.stop_shell, with its switch that stops one shell early.

The masks come from points_model.py (pinned to the oracle).  Plain helper module (not a conftest)."""
import numpy as np

import crowding_model as cm
import depth_model as dm
import hse_model as hm
import points_model as pm
import sweep_model as sm

F = np.float32
PARTNER = 1
STEP, INV_D, INV_D2, INV_1PD = 0, 1, 2, 3
KINDS = (STEP, INV_D, INV_D2, INV_1PD)
MAX_CHANNELS = 4    # RSASA_FIELD_MAX_CHANNELS
FRACTION_BITS = 24
BOUND = F(2.0 ** 24)
_PAIRS = 1 << 21    # (dot, partner) pairs evaluated at once


def c2_of(cutoff):
    """cutoff * cutoff: one float32 product (may overflow to +inf, underflow to 0); -0.0 is 0."""
    with np.errstate(over="ignore", under="ignore"):
        c = F(cutoff) + F(0.0)
        return c * c


def weights_of(weights, n):
    w = np.ascontiguousarray(weights, F)
    if w.ndim == 1:
        w = w[:, None]
    assert w.shape[0] == n and 1 <= w.shape[1] <= MAX_CHANNELS
    return w


def kinds_of(kinds, n_channels):
    k = [INV_D] * n_channels if kinds is None else [int(v) for v in np.atleast_1d(kinds)]
    assert len(k) == n_channels and all(v in KINDS for v in k)
    return k


def _partners(flags, n):
    return np.arange(n) if flags is None else np.flatnonzero(np.asarray(flags).astype(np.uint8) & PARTNER)


def factors(d2):
    """[g of STEP, INV_D, INV_D2, INV_1PD] for float32 d2, each float32, the header's expressions."""
    d2 = np.asarray(d2, F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        d = np.sqrt(d2)
        one = F(1.0)
        g = [np.ones_like(d2), one / d, one / d2, one / (one + d)]
    assert all(a.dtype == F for a in g)
    return g


def fixed(t):
    """int64: rint(t * 2^24) where |t| <= 2^24, else 0 (a NaN fails the comparison).  t float32."""
    t = np.asarray(t)
    assert t.dtype == F
    with np.errstate(invalid="ignore"):
        ok = np.abs(t) <= BOUND
    return np.rint(np.where(ok, t, F(0.0)).astype(np.float64) * 2.0 ** FRACTION_BITS).astype(np.int64)


def wrap_sum(v, axis):
    """The int64 sum along an axis in two's complement, wrapping."""
    return np.ascontiguousarray(v, np.int64).view(np.uint64).sum(axis=axis, dtype=np.uint64).view(np.int64)


def rows_of(qx, qy, qz, x, y, z, par, w, kinds, c2):
    """int64[D, C]: the rows of the dots q against the partners `par` (indices into x, y, z and the rows of w)."""
    n_ch = len(kinds)
    out = np.zeros((len(qx), n_ch), np.int64)
    if len(qx) == 0 or len(par) == 0:
        return out
    px, py, pz, pw = x[par], y[par], z[par], w[par]
    step = max(1, _PAIRS // len(par))
    for a in range(0, len(qx), step):
        sl = slice(a, a + step)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            dx, dy, dz = px[None, :] - qx[sl, None], py[None, :] - qy[sl, None], pz[None, :] - qz[sl, None]
            d2 = dx * dx + dy * dy + dz * dz
            assert d2.dtype == F
            hit = d2 <= c2
            g = factors(d2)
            for c, kind in enumerate(kinds):
                t = pw[None, :, c] * g[kind]
                assert t.dtype == F
                out[sl, c] = wrap_sum(np.where(hit, fixed(t), 0), 1)
    return out


def sums(x, y, z, r, mask, probe, n_points, weights, kinds=None, cutoff=10.0, flags=None):
    """(dot_offsets uint64[N + 1], sums int64[D, C]) of ONE structure with the masks bool[N, n_points]."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    w = weights_of(weights, len(x))
    kinds = kinds_of(kinds, w.shape[1])
    c2 = c2_of(cutoff)
    par = _partners(flags, len(x))
    owner, qx, qy, qz = dm.dots_of(x, y, z, r, mask, probe, n_points)
    off = cm.offsets_of(mask)
    assert len(owner) == int(off[-1])
    if len(x) <= hm.DENSE or not np.isfinite(c2):
        return off, rows_of(qx, qy, qz, x, y, z, par, w, kinds, c2)
    from scipy.spatial import cKDTree
    xyz = np.stack([x, y, z], -1).astype(np.float64)
    par = par[np.isfinite(xyz[par]).all(axis=1)]            # (a NaN partner counts for nobody)
    out = np.zeros((len(owner), len(kinds)), np.int64)
    if len(par) == 0:
        return off, out
    tree = cKDTree(xyz[par])
    q = np.stack([qx, qy, qz], -1).astype(np.float64)
    ok = np.flatnonzero(np.isfinite(q).all(axis=1))         # (a NaN dot has a zero row)
    reach = 1.01 * float(F(cutoff)) + 1e-3
    for d, near in zip(ok, tree.query_ball_point(q[ok], reach)):
        j = par[np.asarray(near, np.int64)]
        out[d] = rows_of(qx[d:d + 1], qy[d:d + 1], qz[d:d + 1], x, y, z, j, w, kinds, c2)[0]
    return off, out


def sums_batch(x, y, z, r, so, mask, probe, n_points, weights, kinds=None, cutoff=10.0, flags=None):
    """(dot_offsets uint64[N + 1] batch-global, sums int64[D, C]) of every structure of a batch."""
    n = int(so[-1]) if len(so) > 1 else 0
    w = weights_of(weights, len(x))
    rows = [np.zeros((0, w.shape[1]), np.int64)]
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        if e > b:
            rows.append(sums(x[b:e], y[b:e], z[b:e], r[b:e], mask[b:e], probe, n_points, w[b:e], kinds, cutoff,
                             None if flags is None else np.asarray(flags)[b:e])[1])
    return cm.offsets_of(mask[:n]), np.concatenate(rows)


def model_batch(x, y, z, r, ids, so, probe, n_points, weights, kinds=None, cutoff=10.0, flags=None, W=8):
    """sums_batch with points_model's masks: (dot_offsets, sums, mask)."""
    mask = pm.exposed_masks_batch(x, y, z, r, ids, so, probe, n_points, W)
    return sums_batch(x, y, z, r, so, mask, probe, n_points, weights, kinds, cutoff, flags) + (mask,)


def values(s):
    """float64: sums * 2^-24 by a direct product."""
    return np.asarray(s, np.int64).astype(np.float64) / float(1 << FRACTION_BITS)


def brute64(qx, qy, qz, x, y, z, par, w, kinds, cutoff):
    """(total float64[D, C], absolute float64[D, C], n int64[D], band float64[D]): from the SAME float32 dots and centres
    in float64 arithmetic, the sum of the terms w * g(d) over the partners with d <= cutoff, the sum of their
    magnitudes, their number, and the smallest |d - cutoff| over all partners.  Finite input, no d of 0."""
    q = np.stack([qx, qy, qz], -1).astype(np.float64)
    p = np.stack([x[par], y[par], z[par]], -1).astype(np.float64)
    d = np.sqrt(((p[None, :, :] - q[:, None, :]) ** 2).sum(-1))
    cut = float(F(cutoff))
    hit = d <= cut
    g = [np.ones_like(d), 1.0 / d, 1.0 / (d * d), 1.0 / (1.0 + d)]
    w64 = np.asarray(w, F)[par].astype(np.float64)
    total = np.zeros((len(q), len(kinds)))
    absolute = np.zeros_like(total)
    for c, kind in enumerate(kinds):
        t = np.where(hit, w64[None, :, c] * g[kind], 0.0)
        total[:, c], absolute[:, c] = t.sum(axis=1), np.abs(t).sum(axis=1)
    return total, absolute, hit.sum(axis=1), np.abs(d - cut).min(axis=1)


# ---- the sweep of k_dot_fields -------------------------------------------------------------------------------------------

def sweep_sums(x, y, z, r, mask, probe, n_points, weights, kinds, cutoff, flags, sample, margins=None, early=False, **switches):
    """(rows {atom: int64[free, C]}, stop int64[len(sample)], by_rule bool[...], found [sorted shells]) for the dots of the
    atoms `sample` of ONE structure, swept as the kernel sweeps them - crowding_model.stop_shell with the cutoff for the
    last edge; found[n]: the shells in which some dot of sample[n] met a partner within the cutoff."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    n = len(x)
    w = weights_of(weights, n)
    kinds = kinds_of(kinds, w.shape[1])
    c2 = c2_of(cutoff)
    fl = np.full(n, PARTNER, np.uint8) if flags is None else np.asarray(flags).astype(np.uint8)
    g = sm.grid(x, y, z, r, probe)
    if margins is None:
        margins = sm.margins_hold(x, y, z, r, probe)
    owner, qx, qy, qz = dm.dots_of(x, y, z, r, mask, probe, n_points)
    ones = np.ones((n, 1), F)
    rows, found = {}, []
    stop, by_rule = np.zeros(len(sample), np.int64), np.zeros(len(sample), bool)
    for m, i in enumerate(sample):
        stop[m], by_rule[m] = cm.stop_shell(float(F(cutoff)), g.h, g.s_last(i), margins, early)
        mine = np.flatnonzero(owner == i)
        row = np.zeros((len(mine), len(kinds)), np.int64)
        shells = []
        if len(mine):
            for s in range(int(stop[m]) + 1):
                for flat in sm.shell_steps(g, i, s, **switches)[0]:
                    j = g.order[flat]
                    j = j[(fl[j] & PARTNER) != 0]
                    add = rows_of(qx[mine], qy[mine], qz[mine], x, y, z, j, w, kinds, c2)
                    row = wrap_sum(np.stack([row, add]), 0)
                    if rows_of(qx[mine], qy[mine], qz[mine], x, y, z, j, ones, [STEP], c2).any():
                        shells.append(s)
        rows[int(i)] = row
        found.append(sorted(set(shells)))
    return rows, stop, by_rule, found
