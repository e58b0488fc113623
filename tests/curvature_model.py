"""An exact CPU model of the dot curvature (rsasa_dot_curvature*): the definition of include/rustsasa_amd.h followed
literally, brute force in numpy float32.

    dots, q         exactly those of the surface components and the dot links (depth_model.dots_of)
    normal          of dot (i, k): the lattice point s_k itself, float32
    per pair        dx = q_b - q_a; d2 = dx*dx + dy*dy + dz*dz; h = (n.x*dx + n.y*dy) + n.z*dz; t = d - h n;
                    t2 = (tx*tx + ty*ty) + tz*tz; g = h / t2; terms = [d2, h, (tx*tx) g, (ty*ty) g, (tz*tz) g, (tx*ty) g,
                    (tx*tz) g, (ty*tz) g] - numpy float32 arithmetic is unfused and its division correctly rounded
    a pair counts   iff b != a, d2 <= reach * reach, d2 > 0, t2 > 0 and every |term| <= 2^24 (a NaN fails everywhere);
                    then 1 to pairs[a] and rint(term * 2^24) to moments[a, :] - wrapping 64-bit sums

rows() also reports, per dot, the pairs that pass b != a, d2 <= reach * reach and d2 > 0 but are dropped by t2 or by a
term's bound: where that is 0, pairs[a] is the length of the dot's list of links at link = reach less its entries with
d2 == 0.  sweep_rows() is NOT a second brute force: it emulates what one wave of k_dot_curvature (curvature.hip) stages
for one atom - the shells of the reach, the 64-atom staging rounds, the staging cut - and sums over the dots of the
staged atoms only; its keyword switches exist so that the CPU tests can show that a case bites.  The masks come from
points_model.py (pinned to the oracle).  Plain helper module (not a conftest)."""
import numpy as np

import depth_model as dm
import points_model as pm
import sweep_model as sm
from oracle import pyoracle as po

F = np.float32
COLUMNS = 8
D2, H, XX, YY, ZZ, XY, XZ, YZ = range(8)
BOUND = F(2.0 ** 24)
ONE = 1 << 24
_PAIRS = 1 << 21   # (a, b) pairs evaluated at once


def reach2_of(reach):
    r = F(reach) + F(0.0)          # (-0.0 is 0)
    with np.errstate(over="ignore", under="ignore"):
        return r * r


def normals_of(mask, n_points):
    """float32[D, 3]: the lattice points of the accessible dots of a mask, in dot order."""
    s = np.stack([np.asarray(a, F) for a in po.sphere_points(n_points)], -1)
    return s[np.nonzero(mask)[1]]


def terms_of(dx, dy, dz, nx, ny, nz):
    """(terms float32[8, ...], t2): the eight terms of pairs with chord (dx, dy, dz) and normal (nx, ny, nz)."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        d2 = dx * dx + dy * dy + dz * dz
        h = (nx * dx + ny * dy) + nz * dz
        tx, ty, tz = dx - h * nx, dy - h * ny, dz - h * nz
        t2 = (tx * tx + ty * ty) + tz * tz
        g = h / t2
        terms = np.stack([d2, h, (tx * tx) * g, (ty * ty) * g, (tz * tz) * g, (tx * ty) * g, (tx * tz) * g, (ty * tz) * g])
    assert terms.dtype == F and t2.dtype == F
    return terms, t2


def _fixed(terms, counts):
    """int64[8, A]: the wrapping sums over the last axis of rint(term * 2^24) of the pairs that count."""
    with np.errstate(invalid="ignore"):
        fx = np.rint(np.where(counts[None], terms, F(0.0)).astype(np.float64) * float(ONE)).astype(np.int64)
    return fx.view(np.uint64).sum(axis=-1, dtype=np.uint64).view(np.int64)


def pair_rows(q, n, a_idx, b_idx, reach):
    """(pairs uint32[A], moments int64[A, 8], dropped int64[A]) of the dots a_idx of ONE structure against the dots
    b_idx of it (q float32[D, 3], n float32[D, 3])."""
    a_idx, b_idx = np.asarray(a_idx, np.int64), np.asarray(b_idx, np.int64)
    A, B = len(a_idx), len(b_idx)
    pairs, mom, dropped = np.zeros(A, np.uint32), np.zeros((A, COLUMNS), np.int64), np.zeros(A, np.int64)
    if A == 0 or B == 0:
        return pairs, mom, dropped
    r2 = reach2_of(reach)
    qb = q[b_idx]
    step = max(1, _PAIRS // B)
    for lo in range(0, A, step):
        ai = a_idx[lo:lo + step]
        qa, na = q[ai], n[ai]
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy, dz = (qb[None, :, k] - qa[:, None, k] for k in range(3))
        terms, t2 = terms_of(dx, dy, dz, na[:, None, 0], na[:, None, 1], na[:, None, 2])
        with np.errstate(invalid="ignore"):
            hit = (b_idx[None, :] != ai[:, None]) & (terms[D2] <= r2) & (terms[D2] > F(0.0))
            counts = hit & (t2 > F(0.0)) & (np.abs(terms) <= BOUND).all(axis=0)
        pairs[lo:lo + step] = counts.sum(axis=1)
        dropped[lo:lo + step] = (hit & ~counts).sum(axis=1)
        mom[lo:lo + step] = _fixed(terms, counts).T
    return pairs, mom, dropped


def dots(x, y, z, r, mask, probe, n_points):
    """(owner int64[D], q float32[D, 3], n float32[D, 3]) of ONE structure."""
    owner, qx, qy, qz = dm.dots_of(x, y, z, r, mask, probe, n_points)
    return owner, np.stack([qx, qy, qz], -1), normals_of(mask, n_points)


def rows(x, y, z, r, mask, probe, n_points, reach, sample=None):
    """(dot_offsets uint64[N + 1], pairs, moments, dropped) of ONE structure; sample: only the dots of these atoms (the
    rows of the others stay zero)."""
    owner, q, n = dots(x, y, z, r, mask, probe, n_points)
    off = np.concatenate([[0], np.cumsum(np.asarray(mask).sum(axis=1))]).astype(np.uint64)
    every = np.arange(len(owner))
    a_idx = every if sample is None else every[np.isin(owner, np.asarray(sample))]
    p, m, d = pair_rows(q, n, a_idx, every, reach)
    pairs, mom, dropped = np.zeros(len(owner), np.uint32), np.zeros((len(owner), COLUMNS), np.int64), np.zeros(len(owner), np.int64)
    pairs[a_idx], mom[a_idx], dropped[a_idx] = p, m, d
    return off, pairs, mom, dropped


def rows_batch(x, y, z, r, ids, so, probe, n_points, reach, W=8, mask=None):
    """(dot_offsets, pairs, moments, dropped, mask) of every structure of a batch: dots of different structures never
    pair; dot_offsets and the rows run over the whole batch."""
    n = int(so[-1]) if len(so) > 1 else 0
    if mask is None:
        mask = pm.exposed_masks_batch(x, y, z, r, ids, so, probe, n_points, W) if n else np.zeros((0, n_points), bool)
    off = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.uint64)
    out = [np.zeros(0, np.uint32)], [np.zeros((0, COLUMNS), np.int64)], [np.zeros(0, np.int64)]
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        if e > b:
            got = rows(x[b:e], y[b:e], z[b:e], r[b:e], mask[b:e], probe, n_points, reach)[1:]
            for acc, v in zip(out, got):
                acc.append(v)
    return (off,) + tuple(np.concatenate(a) for a in out) + (mask,)


U = 2.0 ** -24      # the unit roundoff of float32


def sums64(x, y, z, r, mask, probe, n_points, reach):
    """(sums float64[D, 8], bounds float64[D, 8]): the same eight sums of ONE structure with the terms evaluated in
    float64 from the float32 dots and normals, over the pairs the float32 model counts, and how far the model's
    fixed-point sums may lie from them.  Per pair, with u = 2^-24, d the chord, t its tangential part, |n| <= 1 + 3 u:
        d2      the subtraction rounds each component (u), three squares and two sums of positives (3 u): 6 u d2
        h       the same inputs (u), three products and two sums (3 u): 5 u |d|
        tensor  t_k = d_k - h n_k carries u |d_k| + |dh| |n_k| + u |h n_k| + u |t_k| <= 8 u |d|; a product T_i T_j of
                components of T = t / |t| moves by at most 4 times that over |t|, doubled for the quotient by t2 computed
                from the same t: 64 u |d| / |t|; five more roundings (two squares or a product, the sum's two, the
                division, the last product): 8 u in all - times |h|, plus h's own error
    and half a unit of 2^-24 per term for the conversion.  The bound is evaluated from the float64 chords."""
    owner, q, n = dots(x, y, z, r, mask, probe, n_points)
    D = len(owner)
    out, bounds = np.zeros((D, COLUMNS)), np.zeros((D, COLUMNS))
    r2 = reach2_of(reach)
    for a in range(D):
        d32 = q - q[a]
        t32, t2 = terms_of(d32[:, 0], d32[:, 1], d32[:, 2], n[a, 0], n[a, 1], n[a, 2])
        with np.errstate(invalid="ignore"):
            counts = (np.arange(D) != a) & (t32[D2] <= r2) & (t32[D2] > 0) & (t2 > 0) & (np.abs(t32) <= BOUND).all(axis=0)
        d = (q[counts].astype(np.float64) - q[a].astype(np.float64))
        na = n[a].astype(np.float64)
        h = d @ na
        t = d - h[:, None] * na[None, :]
        g = h / (t * t).sum(axis=1)
        out[a] = [(d * d).sum(), h.sum(), (t[:, 0] ** 2 * g).sum(), (t[:, 1] ** 2 * g).sum(), (t[:, 2] ** 2 * g).sum(),
                  (t[:, 0] * t[:, 1] * g).sum(), (t[:, 0] * t[:, 2] * g).sum(), (t[:, 1] * t[:, 2] * g).sum()]
        dn, tn = np.sqrt((d * d).sum(axis=1)), np.sqrt((t * t).sum(axis=1))
        e_h = 5 * U * dn
        e_t = np.abs(h) * (64 * U * dn / tn + 8 * U) + e_h
        half = 0.5 * U * len(h)
        bounds[a] = [6 * U * (dn * dn).sum() + half, e_h.sum() + half] + [e_t.sum() + half] * 6
    return out, bounds


def values(pairs, moments):
    """rustsasa_amd.curvature_values restated per dot with an eigen-solver: float64 (mean, gaussian, k1, k2,
    shape_index), from the 2 x 2 tensor that M leaves in the plane orthogonal to its eigenvector of least |eigenvalue|."""
    out = np.full((len(pairs), 5), np.nan)
    for d in range(len(pairs)):
        if pairs[d] == 0 or moments[d, D2] == 0:
            continue
        s = [int(v) for v in moments[d]]
        w = -2.0 / s[D2]
        M = w * np.array([[s[XX], s[XY], s[XZ]], [s[XY], s[YY], s[YZ]], [s[XZ], s[YZ], s[ZZ]]], np.float64)
        val, vec = np.linalg.eigh(M)
        keep = np.delete(np.arange(3), np.argmin(np.abs(val)))
        P = vec[:, keep]
        m2, m1 = np.linalg.eigvalsh(P.T @ M @ P)
        k1, k2 = 3 * m1 - m2, 3 * m2 - m1
        out[d] = [w * s[H], k1 * k2, k1, k2, (2 / np.pi) * np.arctan2(k1 + k2, k1 - k2)]
    return out


# ---- the emulated sweep ------------------------------------------------------------------------------------------------------

def staged_rounds(x, y, z, r, mask, probe, reach, i, g=None, margins=None, reach_shift=0, cut_h=True):
    """[input indices of the atoms staged in one round] for the wave of atom i of ONE structure, round by round as
    k_dot_curvature meets them: shells 0 .. s_end, 64-row steps, 64 atoms of a step's runs at a time; an atom is staged
    when it has a dot and, where the cut is on, when float32 |c_j - c_i|^2 <= (((R_i + reach) + h) + R_j)^2.
    reach_shift: the last shell moved; cut_h False: the cut without its + h.  Rounds that stage nobody are left out."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    g = sm.grid(x, y, z, r, probe) if g is None else g
    if margins is None:
        margins = sm.margins_hold(x, y, z, r, probe)
    L = F(reach) + F(0.0)
    free = np.asarray(mask).any(axis=1)
    s_end = sm.s_end_of(L, g.h, g.s_last(i), margins, reach_shift)
    cut = margins and L <= F(65536.0) * g.h
    R = r + F(probe)
    base = (R[i] + L) + g.h if cut_h else R[i] + L
    out = []
    for s in range(min(s_end, g.s_last(i)) + 1):
        for flat in sm.shell_steps(g, i, s)[0]:
            for lo in range(0, len(flat), sm.WAVE):
                j = g.order[flat[lo:lo + sm.WAVE]]
                keep = free[j]
                if cut:
                    with np.errstate(invalid="ignore", over="ignore"):
                        ex, ey, ez = x[j] - x[i], y[j] - y[i], z[j] - z[i]
                        lim = base + R[j]
                        keep = keep & (ex * ex + ey * ey + ez * ez <= lim * lim)
                if keep.any():
                    out.append(j[keep])
    return out


def sweep_rows(x, y, z, r, mask, probe, n_points, reach, sample, **switches):
    """(pairs, moments) of the dots of the atoms `sample` of ONE structure, in dot order, from the emulated sweep."""
    owner, q, n = dots(x, y, z, r, mask, probe, n_points)
    g = sm.grid(x, y, z, r, probe)
    every = np.arange(len(owner))
    ps, ms = [], []
    for i in sample:
        staged = staged_rounds(x, y, z, r, mask, probe, reach, int(i), g, **switches)
        atoms = np.concatenate(staged) if staged else np.zeros(0, np.int64)
        assert len(np.unique(atoms)) == len(atoms)          # an atom is met in one shell, one step, one round
        p, m, _ = pair_rows(q, n, every[owner == i], every[np.isin(owner, atoms)], reach)
        ps.append(p)
        ms.append(m)
    return np.concatenate(ps), np.concatenate(ms)
