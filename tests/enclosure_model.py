"""The dot enclosure of include/rustsasa_amd.h (rsasa_dot_enclosure*) in numpy float32, every operation written out in the
header's order and nothing fused: the exact model the GPU words are compared with for equality.

    R_i = r_i + p;  q = c_i + R_i * s_k (per component);  R_j = r_j + p;  R2 = R_j * R_j
    dx = c_j.x - q.x;  d2 = (dx*dx + dy*dy) + dz*dz;  t = (dx*u.x + dy*u.y) + dz*u.z
    j != i stops ray m iff (flags[j] & 1), t > 0 and (t <= L ? d2 - t*t : |d - L u|^2) <= R2
    the own atom stops ray m iff (flags[i] & 1) and (u.x*s.x + u.y*s.y) + u.z*s.z < 0

    blocked / blocked_batch   the definition: depth_model.dots_of for the dots (the order of surface_points, of
                              surface_components and of dot_crowding), every (dot, obstacle, direction) of a structure.
                              A structure of more than hse_model.DENSE atoms takes a dot's candidates from a cKDTree ball
                              query at 1.01 (L + max R) + 1e-3 - a superset of what float32 can accept - and the float32
                              rule decides every one of them.
    brute64                   the same words from float64 arithmetic, with the margins of every decision.
    stop_shell, sweep_blocked what k_dot_enclosure (enclosure.hip) does for the dots of one atom, shell by shell, on the
                              emulated grid of sweep_model.py, with its two cuts, and with a switch for a stop rule that
                              forgets R_j.

The masks come from points_model.py (pinned to the oracle).  Plain helper module (not a conftest)."""
import numpy as np

import depth_model as dm
import hse_model as hm
import points_model as pm
import sweep_model as sm

F = np.float32
PARTNER = 1
MAX_DIRS = 32      # RSASA_ENCLOSE_MAX_DIRS
SLACK = F(1.0009765625)   # 1 + 2^-10: the factor of the kernel's cuts
_TRIPLES = 1 << 22  # (dot, obstacle) pairs evaluated at once, per direction


def directions(n_dirs):
    """float32[n_dirs, 3]: rsasa_sphere_points(n_dirs)."""
    from oracle import pyoracle as po
    assert 1 <= n_dirs <= MAX_DIRS
    return np.stack([np.asarray(a, F) for a in po.sphere_points(n_dirs)], -1)


def _obstacles(flags, n):
    return np.arange(n) if flags is None else np.flatnonzero(np.asarray(flags).astype(np.uint8) & PARTNER)


def offsets_of(mask):
    """uint64[N + 1]: the exclusive scan of the masks' popcounts."""
    return np.concatenate([[0], np.cumsum(mask.sum(axis=1, dtype=np.int64))]).astype(np.uint64)


def own_bits(n_points, n_dirs):
    """uint32[n_points]: the own-atom rule of every lattice point, from u_m and s_k alone."""
    from oracle import pyoracle as po
    s = np.stack([np.asarray(a, F) for a in po.sphere_points(n_points)], -1)
    u = directions(n_dirs)
    out = np.zeros(n_points, np.uint32)
    for m in range(n_dirs):
        dot = u[m, 0] * s[:, 0] + u[m, 1] * s[:, 1] + u[m, 2] * s[:, 2]
        assert dot.dtype == F
        out |= (dot < F(0.0)).astype(np.uint32) << np.uint32(m)
    return out


def pair_bits(qx, qy, qz, cx, cy, cz, R2, L, u, cut2=None):
    """uint32 of the broadcast shape: bit m - the obstacle (c, R2) stops ray m of the dot q.  cut2 (optional): the
    kernel's lane cut, d2 <= cut2 before any direction is tried."""
    L = F(L)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        dx, dy, dz = cx - qx, cy - qy, cz - qz
        d2 = dx * dx + dy * dy + dz * dz
        assert d2.dtype == F
        out = np.zeros(d2.shape, np.uint32)
        for m in range(len(u)):
            ux, uy, uz = u[m]
            t = dx * ux + dy * uy + dz * uz
            perp = d2 - t * t
            ex, ey, ez = dx - L * ux, dy - L * uy, dz - L * uz
            e2 = ex * ex + ey * ey + ez * ez
            v = np.where(t <= L, perp, e2)
            assert v.dtype == F
            hit = (t > F(0.0)) & (v <= R2)
            if cut2 is not None:
                hit &= d2 <= cut2
            out |= hit.astype(np.uint32) << np.uint32(m)
    return out


def words_of(owner, qx, qy, qz, x, y, z, R2, obs, L, u):
    """uint32[D]: the OR over the obstacles `obs` (indices into x, y, z, R2), the dot's owner left out."""
    out = np.zeros(len(qx), np.uint32)
    if len(qx) == 0 or len(obs) == 0:
        return out
    step = max(1, _TRIPLES // len(obs))
    for a in range(0, len(qx), step):
        sl = slice(a, a + step)
        bits = pair_bits(qx[sl, None], qy[sl, None], qz[sl, None], x[None, obs], y[None, obs], z[None, obs], R2[None, obs], L, u)
        bits[obs[None, :] == owner[sl, None]] = 0
        out[sl] = np.bitwise_or.reduce(bits, axis=1)
    return out


def _r2(r, probe):
    with np.errstate(invalid="ignore", over="ignore"):
        R = np.ascontiguousarray(r, F) + F(probe)
        return R, R * R


def blocked(x, y, z, r, mask, probe, n_points, n_dirs, reach, flags=None, atoms=None):
    """(dot_offsets uint64[N + 1], blocked uint32[D]) of ONE structure with the masks bool[N, n_points].  atoms: only
    the dots of these atoms (their words in dot order; the offsets are still the structure's)."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    n = len(x)
    u = directions(n_dirs)
    off = offsets_of(mask)
    fl = np.full(n, PARTNER, np.uint8) if flags is None else np.asarray(flags).astype(np.uint8)
    obs = _obstacles(flags, n)
    sub = mask
    if atoms is not None:
        sub = np.zeros_like(mask)
        sub[atoms] = mask[atoms]
    owner, qx, qy, qz = dm.dots_of(x, y, z, r, sub, probe, n_points)
    k = np.nonzero(sub)[1]
    own = np.where((fl[owner] & PARTNER) != 0, own_bits(n_points, n_dirs)[k], np.uint32(0)).astype(np.uint32)
    R, R2 = _r2(r, probe)
    if n <= hm.DENSE:
        return off, own | words_of(owner, qx, qy, qz, x, y, z, R2, obs, reach, u)
    from scipy.spatial import cKDTree
    xyz = np.stack([x, y, z], -1).astype(np.float64)
    obs = obs[np.isfinite(xyz[obs]).all(axis=1) & np.isfinite(R[obs])]      # (a NaN obstacle stops nothing)
    out = own.copy()
    if len(obs) == 0:
        return off, out
    ball = 1.01 * (float(F(reach)) + float(np.abs(R[obs]).max())) + 1e-3
    assert np.isfinite(ball), "a dense structure needs a finite reach"
    tree = cKDTree(xyz[obs])
    q = np.stack([qx, qy, qz], -1).astype(np.float64)
    ok = np.flatnonzero(np.isfinite(q).all(axis=1))                          # (a NaN dot is stopped by nobody)
    for a in range(0, len(ok), 1024):                                        # (dot, candidate) pairs, flat
        dots = ok[a:a + 1024]
        near = tree.query_ball_point(q[dots], ball)
        lens = np.array([len(v) for v in near], np.int64)
        if lens.sum() == 0:
            continue
        d = np.repeat(dots, lens)
        j = obs[np.concatenate([np.asarray(v, np.int64) for v in near])]
        bits = pair_bits(qx[d], qy[d], qz[d], x[j], y[j], z[j], R2[j], reach, u)
        bits[j == owner[d]] = 0
        np.bitwise_or.at(out, d, bits)
    return off, out


def blocked_batch(x, y, z, r, so, mask, probe, n_points, n_dirs, reach, flags=None):
    """(dot_offsets uint64[N + 1] batch-global, blocked uint32[D]) of every structure of a batch."""
    n = int(so[-1]) if len(so) > 1 else 0
    words = [np.zeros(0, np.uint32)]
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        if e > b:
            words.append(blocked(x[b:e], y[b:e], z[b:e], r[b:e], mask[b:e], probe, n_points, n_dirs, reach,
                                 None if flags is None else np.asarray(flags)[b:e])[1])
    return offsets_of(mask[:n]), np.concatenate(words)


def model_batch(x, y, z, r, ids, so, probe, n_points, n_dirs, reach, flags=None, W=8):
    """blocked_batch with points_model's masks: (dot_offsets, blocked, mask)."""
    mask = pm.exposed_masks_batch(x, y, z, r, ids, so, probe, n_points, W)
    return blocked_batch(x, y, z, r, so, mask, probe, n_points, n_dirs, reach, flags) + (mask,)


def popcount(words):
    w = np.asarray(words, np.uint32)
    return ((w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & np.uint32(1)).sum(axis=1).astype(np.int64)


def brute64(x, y, z, r, mask, probe, n_points, n_dirs, reach, flags=None):
    """(blocked uint32[D], firm bool[D]): the words from float64 arithmetic on the float32 inputs, lattice and directions.
    A decision is hit = (t > 0) and (v <= R2) with v = d2 - t^2 below t = L and |d - L u|^2 above (the two meet at
    t = L, up to L^2 (|u|^2 - 1)); it is firm when v lies more than V_BAND above R2, or t more than T_BAND below 0, or
    both lie that far on the hitting side.  firm[d]: every decision of dot d is.  Finite input."""
    from oracle import pyoracle as po
    s = np.stack([np.asarray(a, F) for a in po.sphere_points(n_points)], -1).astype(np.float64)
    u = directions(n_dirs).astype(np.float64)
    xyz = np.stack([x, y, z], -1).astype(np.float64)
    R = np.asarray(r, F).astype(np.float64) + float(F(probe))
    L = float(F(reach))
    i, k = np.nonzero(mask)
    q = xyz[i] + R[i, None] * s[k]
    obs = _obstacles(flags, len(x))
    fl = np.ones(len(x), bool) if flags is None else (np.asarray(flags).astype(np.uint8) & PARTNER) != 0
    out = np.zeros(len(i), np.uint32)
    firm = np.ones(len(i), bool)
    d = xyz[obs][None, :, :] - q[:, None, :]
    d2 = (d ** 2).sum(-1)
    other = obs[None, :] != i[:, None]
    for m in range(n_dirs):
        t = d @ u[m]
        v = np.where(t <= L, d2 - t * t, ((d - L * u[m]) ** 2).sum(-1))
        gap = v - (R[obs] ** 2)[None, :]
        hit = (t > 0) & (gap <= 0) & other
        sure = (gap > V_BAND) | (t < -T_BAND) | ((gap < -V_BAND) & (t > T_BAND)) | ~other
        firm &= sure.all(axis=1)
        own = fl[i] & (s[k] @ u[m] < 0)
        out |= (hit.any(axis=1) | own).astype(np.uint32) << np.uint32(m)
    return out, firm


V_BAND = 2.0 ** -11   # see test_enclosure_cpu.py for the derivation
T_BAND = 2.0 ** -15


# ---- the sweep of k_dot_enclosure --------------------------------------------------------------------------------------

def stop_shell(L, h, s_last, margins, early=False):
    """(the shell k_dot_enclosure stops after, whether the rule stopped it): float32, as written in enclosure.hip - after
    shell s >= 3 when L * L <= lim2, lim = (float(s) - 2.5f) * h, lim2 >= 1e-30.  early: the rule with 1.5 in place of
    2.5 from shell 2 on, which is met one shell sooner - a kernel that forgot the obstacle's own radius."""
    with np.errstate(over="ignore", under="ignore"):
        ll = F(L) * F(L)
    s = 0
    while True:
        if s >= s_last:
            return s, False
        if margins and s >= (2 if early else 3):
            lim = (F(s) - F(1.5 if early else 2.5)) * F(h)
            lim2 = lim * lim
            if ll <= lim2 and lim2 >= F(1e-30):
                return s, True
        s += 1


def sweep_blocked(x, y, z, r, mask, probe, n_points, n_dirs, reach, flags, sample, margins=None, early=False, cuts=True,
                  abs_term=True, **switches):
    """(words {atom: uint32[free]}, stop int64[len(sample)], by_rule bool[...], shells [{shell: uint32[free]}]) for the
    dots of the atoms `sample` of ONE structure, swept as the kernel sweeps them: the owner dropped by its position,
    the staging cut and the lane cut where the margins hold (cuts=False: neither; abs_term=False: the staging cut
    without its absolute h / 64 - a kernel that trusted the relative slack alone).  shells[n][s]: the bits that the
    obstacles of shell s set on the dots of sample[n] (the own-atom bits are in no shell)."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    n = len(x)
    u = directions(n_dirs)
    L = F(reach)
    fl = np.full(n, PARTNER, np.uint8) if flags is None else np.asarray(flags).astype(np.uint8)
    g = sm.grid(x, y, z, r, probe)
    if margins is None:
        margins = sm.margins_hold(x, y, z, r, probe)
    owner, qx, qy, qz = dm.dots_of(x, y, z, r, mask, probe, n_points)
    k_of = np.nonzero(mask)[1]
    own = own_bits(n_points, n_dirs)
    R, R2 = _r2(r, probe)
    h64 = F(g.h) * F(0.015625)
    words, shells = {}, []
    stop, by_rule = np.zeros(len(sample), np.int64), np.zeros(len(sample), bool)
    for m, i in enumerate(sample):
        stop[m], by_rule[m] = stop_shell(L, g.h, g.s_last(i), margins, early)
        mine = np.flatnonzero(owner == i)
        word = (own[k_of[mine]] if fl[i] & PARTNER else np.zeros(len(mine), np.uint32)).astype(np.uint32)
        per = {}
        if len(mine):
            for s in range(int(stop[m]) + 1):
                add = np.zeros(len(mine), np.uint32)
                for flat in sm.shell_steps(g, i, s, **switches)[0]:
                    j = g.order[flat]
                    j = j[((fl[j] & PARTNER) != 0) & (j != i)]
                    cut2 = None
                    if margins and cuts and len(j):
                        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                            ddx, ddy, ddz = x[j] - x[i], y[j] - y[i], z[j] - z[i]
                            dd2 = ddx * ddx + ddy * ddy + ddz * ddz
                            far = ((L + R[i]) + R[j]) * SLACK + (h64 if abs_term else F(0.0))
                            far2 = far * far
                            j = j[~(far2 >= F(1e-30)) | (dd2 <= far2)]
                            near = (L + R[j]) * SLACK
                            near2 = near * near
                            cut2 = np.where(near2 >= F(1e-30), near2, F(np.inf)).astype(F)[None, :]
                    if len(j):
                        bits = pair_bits(qx[mine, None], qy[mine, None], qz[mine, None], x[None, j], y[None, j], z[None, j],
                                         R2[None, j], L, u, cut2)
                        add |= np.bitwise_or.reduce(bits, axis=1)
                word |= add
                per[s] = add
        words[int(i)] = word
        shells.append(per)
    return words, stop, by_rule, shells
