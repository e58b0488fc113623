"""Occlusion decisions at their exact edges: an independent model of one decision and a generator of tiny
structures that sit on it.

The kernels are checked for bit-equality with the oracle (oracle/sasa_oracle.c) on typical inputs.  This module
builds the inputs where a kernel's correctness rests on a hand-derived argument instead: a surface point whose
`dot` equals its `limit` exactly (the fused rule's `<` and the remainder rule's `<=` differ only there), points a
few ulps and a few 2^-11 |limit| from it (the f16 filter's margin band of k_occlusion_mx), the rim of a patch of
16 points (its patch test), nearly concentric atoms whose v lies in f16's subnormal range (the filter's constant
margin), the admission range of k_occlusion_mx, the candidate cutoffs of the spatial grid and 64-bit ids whose
32-bit folds collide.

The model restates the reference's decision for one (atom i, neighbour j, point k) in numpy float32 arithmetic, in
the reference's order (lib.rs:101-136), with the fused dot product from the host libm's `fmaf` (correctly
rounded); the candidate rule and the grid's reach (spatial_grid.rs:307-335, lib.rs:76-80) decide whether j is a
neighbour of i at all.  A generated case is kept only if the oracle's exposed-point count of atom i changes across
it, so every case can tell a right kernel from a wrong one.  Plain helper module (not a conftest).
"""
from __future__ import annotations

import ctypes
import ctypes.util
import functools
import math
from dataclasses import dataclass, field

import numpy as np

from oracle import pyoracle as po

F = np.float32
_FOLD_MUL = 0x9E3779B1
_M32 = 0xFFFFFFFF

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]
_libm.fmaf.restype = ctypes.c_float


def fmaf(a, b, c) -> np.float32:
    """The host libm's fmaf (glibc: correctly rounded)."""
    return F(_libm.fmaf(float(a), float(b), float(c)))


def fmaf_vec(a, b, c) -> np.ndarray:
    """fmaf over arrays: a*b is exact in float64, a*b + c is rounded to odd in float64 (two-sum error, then the
    sticky bit), and round-to-odd at 53 bits followed by round-to-nearest at 24 is the correctly rounded result.
    test_oracle_ties.py compares it with the libm function on every operand triple it is used on."""
    a, b, c = (np.asarray(t, np.float32).astype(np.float64) for t in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    away = (e != 0) & ((e < 0) != (s < 0))
    t = np.where(away, np.nextafter(s, 0.0), s)
    bits = t.view(np.int64) | np.where(e != 0, 1, 0).astype(np.int64)
    return bits.view(np.float64).astype(np.float32)


def fold_id(i: int) -> int:
    """device_utils.h fold_id: lo ^ hi * 0x9E3779B1 (mod 2^32)."""
    return ((i & _M32) ^ (((i >> 32) * _FOLD_MUL) & _M32)) & _M32


def colliding_id(a: int, hi_b: int) -> int:
    """A 64-bit id with high word hi_b whose fold equals fold_id(a)."""
    lo_b = fold_id(a) ^ ((hi_b * _FOLD_MUL) & _M32)
    return ((hi_b & _M32) << 32) | lo_b


def quotient_3op(num, d):
    """k_occlusion_mx's limit (occlusion_mx.inc, prep): y = RN(1 / d), q0 = RN(num y), r = fma(-q0, d, num),
    RN(fma(r, y, q0))."""
    num, d = F(num), F(d)
    y = F(1.0) / d
    q0 = num * y
    r = fmaf(-q0, d, num)
    return fmaf(r, y, q0)


def ulps(v, n: int) -> np.float32:
    """v moved by n float32 steps (towards +inf for n > 0)."""
    v = F(v)
    to = F(np.inf) if n > 0 else F(-np.inf)
    for _ in range(abs(n)):
        v = np.nextafter(v, to)
    return v


@functools.lru_cache(maxsize=None)
def sphere(n_points: int):
    x, y, z = po.sphere_points(n_points)
    return x, y, z


# ---- the decision model --------------------------------------------------------------------------------------

def _as_u32(v) -> int:
    """Rust `f32 as u32` (saturating, NaN -> 0)."""
    v = float(v)
    if not v > 0.0:
        return 0
    return min(int(v), _M32)


def pair_terms(ci, ri, cj, rj, probe):
    """(vx, vy, vz, limit) of neighbour j for atom i, lib.rs:101-102,129-136 and spatial_grid.rs:336-339."""
    probe = F(probe)
    R = F(ri) + probe
    R2 = R * R
    vx, vy, vz = F(ci[0]) - F(cj[0]), F(ci[1]) - F(cj[1]), F(ci[2]) - F(cj[2])
    d2 = vx * vx + vy * vy + vz * vz
    tj = F(rj) + probe
    t = tj * tj
    limit = (t - d2 - R2) / (F(2.0) * R)
    return vx, vy, vz, limit


def point_dot(s, v, fused: bool) -> np.float32:
    """The reference's dot product of point s with v: fused chain (lib.rs:143-144) or plain products (lib.rs:185)."""
    if fused:
        return fmaf(s[0], v[0], fmaf(s[1], v[1], F(s[2]) * F(v[2])))
    return F(s[0]) * F(v[0]) + F(s[1]) * F(v[1]) + F(s[2]) * F(v[2])


def point_occluded(ci, ri, cj, rj, probe, s, fused: bool) -> bool:
    """Does neighbour j occlude point s of atom i: `dot < limit` (fused rule) or `dot <= limit` (remainder rule)."""
    vx, vy, vz, limit = pair_terms(ci, ri, cj, rj, probe)
    dot = point_dot(s, (vx, vy, vz), fused)
    return bool(dot < limit) if fused else bool(dot <= limit)


def n_fused(n_points: int, W: int) -> int:
    """Points [0, n_fused) take the fused rule, the last n_points % W the remainder rule (lib.rs:104-106)."""
    return n_points - n_points % W


@dataclass
class Structure:
    x: np.ndarray
    y: np.ndarray
    z: np.ndarray
    r: np.ndarray
    ids: np.ndarray

    @staticmethod
    def of(coords, radii, ids=None):
        c = np.asarray(coords, np.float32).reshape(-1, 3)
        ids = np.arange(1, len(c) + 1, dtype=np.uint64) if ids is None else np.asarray(ids, np.uint64)
        return Structure(c[:, 0].copy(), c[:, 1].copy(), c[:, 2].copy(), np.asarray(radii, np.float32), ids)

    @property
    def n(self) -> int:
        return len(self.x)

    def centre(self, i):
        return (self.x[i], self.y[i], self.z[i])

    def soa(self):
        return self.x, self.y, self.z, self.r, self.ids


def candidates(st: Structure, probe):
    """Per atom, the neighbours the reference lists (spatial_grid.rs:195-335 with lib.rs:69-84): other ids, in a cell
    the half shell reaches, d^2 <= max_search^2 and d^2 <= (r_i + max_r + 2 probe)^2."""
    probe = F(probe)
    max_r = F(0.0)
    for r in st.r:
        max_r = F(max(max_r, r))
    cell = probe + max_r
    max_search = max_r + max_r + F(2.0) * probe
    ms2 = max_search * max_search
    inv = F(1.0) / cell
    extent = int(math.ceil(float(max_search / cell)))
    mins = [F(np.min(a)) - cell for a in (st.x, st.y, st.z)]
    cells = [(_as_u32((st.x[i] - mins[0]) * inv), _as_u32((st.y[i] - mins[1]) * inv),
              _as_u32((st.z[i] - mins[2]) * inv)) for i in range(st.n)]
    out = []
    for i in range(st.n):
        sr = st.r[i] + max_r + F(2.0) * probe
        sr2 = sr * sr
        lst = []
        for j in range(st.n):
            if j == i or st.ids[j] == st.ids[i]:
                continue
            if any(abs(cells[i][a] - cells[j][a]) > extent for a in range(3)):
                continue
            dx, dy, dz = st.x[i] - st.x[j], st.y[i] - st.y[j], st.z[i] - st.z[j]
            d2 = dx * dx + dy * dy + dz * dz
            if d2 <= ms2 and d2 <= sr2:
                lst.append(j)
        out.append(lst)
    return out


def model_counts(st: Structure, probe, n_points: int, W: int):
    """The model's exposed-point count and candidate count K of every atom."""
    sx, sy, sz = sphere(n_points)
    nf = n_fused(n_points, W)
    cands = candidates(st, probe)
    counts = np.zeros(st.n, np.uint32)
    for i in range(st.n):
        occ = np.zeros(n_points, bool)
        for j in cands[i]:
            vx, vy, vz, limit = pair_terms(st.centre(i), st.r[i], st.centre(j), st.r[j], probe)
            if nf:
                dot = fmaf_vec(sx[:nf], vx, fmaf_vec(sy[:nf], vy, sz[:nf] * vz))
                occ[:nf] |= dot < limit
            if nf < n_points:
                dot = sx[nf:] * vx + sy[nf:] * vy + sz[nf:] * vz
                occ[nf:] |= dot <= limit
        counts[i] = n_points - int(occ.sum())
    return counts, np.array([len(c) for c in cands], np.uint32)


def oracle_counts(st: Structure, probe, n_points: int, W: int):
    """The oracle's (values, exposed-point counts, K)."""
    return po.calculate_sasa_internal(*st.soa(), probe, n_points, W, return_details=True)


def mx_admits(st: Structure, probe, i: int) -> bool:
    """k_occlusion_mx's admission of atom i (occlusion_mx.inc ok_atoms, in f32): R = r + probe >= 0.5,
    sr = r + max_r + 2 probe <= 64, probe in [0, 32] and every radius of the structure in [0, 64]."""
    probe = F(probe)
    max_r = F(0.0)
    for r in st.r:
        max_r = F(max(max_r, r))
    R = st.r[i] + probe
    sr = st.r[i] + max_r + F(2.0) * probe
    radii_ok = bool(np.all((st.r >= F(0.0)) & (st.r <= F(64.0))))
    return bool(R >= F(0.5) and sr <= F(64.0) and F(0.0) <= probe <= F(32.0) and radii_ok)


# ---- patches of 16 points (context.cpp) ---------------------------------------------------------------------

def bisect_points(idx, lo, hi, x, y, z):
    """context.cpp bisect_points: split along the widest axis (ties by index) into halves of whole 16s."""
    n = hi - lo
    if n <= 16:
        return
    mn = [F(2.0)] * 3
    mx = [F(-2.0)] * 3
    cs = (x, y, z)
    for i in range(lo, hi):
        for k in range(3):
            c = cs[k][idx[i]]
            mn[k] = min(mn[k], c)
            mx[k] = max(mx[k], c)
    ax = 0
    for k in (1, 2):
        if mx[k] - mn[k] > mx[ax] - mn[ax]:
            ax = k
    c = cs[ax]
    idx[lo:hi] = sorted(idx[lo:hi], key=lambda a: (float(c[a]), a))
    left = ((n + 15) // 16 // 2) * 16
    bisect_points(idx, lo, lo + left, x, y, z)
    bisect_points(idx, lo + left, hi, x, y, z)


@functools.lru_cache(maxsize=None)
def patches(n_points: int, W: int):
    """The lattice's patches (more than 128 points): lists of original point indices, 16 per patch - the fused-rule
    points in bisect_points order, then the remainder points."""
    x, y, z = sphere(n_points)
    nf = n_fused(n_points, W)
    idx = list(range(nf))
    bisect_points(idx, 0, nf, x, y, z)
    idx += list(range(nf, n_points))
    return [idx[b:b + 16] for b in range(0, n_points, 16)]


# ---- cases ----------------------------------------------------------------------------------------------------

@dataclass
class Case:
    family: str
    probe: float
    n_points: int
    W: int
    structures: list            # [Structure]: the variants around the edge (every one a structure of its own)
    atom: int = 0               # the atom whose decision is on the edge
    tie: bool = False           # the exposed / occluded side has dot == limit exactly
    edge: str = ""              # family c: which edge of k_occlusion_mx's admission range
    label: str = ""
    want_k_change: bool = False  # family e: the observable is atom `atom`'s candidate count
    meta: dict = field(default_factory=dict)

    def __post_init__(self):
        self.probe = float(F(self.probe))  # (the f32 value every side computes with)


def _walk_flip(decide, v0, lo_bound=None):
    """The pair (a, nextafter(a, +inf)) around v0 where decide() turns from False to True (decide must be monotone
    near v0: a larger value occludes more).  None if no flip within 4096 steps."""
    v = F(v0)
    d = decide(v)
    for _ in range(4096):
        w = np.nextafter(v, F(-np.inf) if d else F(np.inf))
        if lo_bound is not None and w < lo_bound:
            return None
        dw = decide(w)
        if dw != d:
            return (w, v) if d else (v, w)
        v = w
    return None


def _radius_variants(r_exp, r_occ, limit, R, tj):
    """r_j values around the flip: both sides, +-2 and +-4 ulps from it, and offsets of m 2^-11 |limit| in limit
    (d limit / d r_j = (r_j + probe) / R) for m = 1, 2, 4, 8 on either side."""
    out = [r_exp, r_occ, ulps(r_exp, -1), ulps(r_occ, 1), ulps(r_exp, -3), ulps(r_occ, 3)]
    step = abs(float(limit)) * 2.0 ** -11 * float(R) / max(float(tj), 1e-3)
    for m in (1, 2, 4, 8):
        for sgn in (-1, 1):
            r = F(float(r_exp) + sgn * m * step)
            if r >= 0:
                out.append(r)
    return out


def _confirmed(case: Case, lo: Structure, hi: Structure) -> bool:
    """The oracle's exposed-point count of the watched atom drops across the edge."""
    _, p_lo, k_lo = oracle_counts(lo, case.probe, case.n_points, case.W)
    _, p_hi, k_hi = oracle_counts(hi, case.probe, case.n_points, case.W)
    if case.want_k_change:
        return int(k_lo[case.atom]) != int(k_hi[case.atom])
    return int(p_lo[case.atom]) > int(p_hi[case.atom])


def _radius_case(rng, family, probe, n_points, W, ci, ri, v, k, extra=(), edge="", label="", rj_bounds=(0.0, 63.0)):
    """Neighbour j at ci - v whose radius walks to the flip of point k of atom i (atom 0); `extra` atoms
    (coords, radius) complete the structure."""
    sx, sy, sz = sphere(n_points)
    s = (sx[k], sy[k], sz[k])
    fused = k < n_fused(n_points, W)
    ci = tuple(F(c) for c in ci)
    cj = tuple(F(ci[a] - F(v[a])) for a in range(3))
    R = F(ri) + F(probe)
    P = np.array([float(ci[a]) + float(R) * float(s[a]) for a in range(3)])
    rj0 = float(np.linalg.norm(P - np.array(cj, float))) - float(probe)
    if not (rj_bounds[0] <= rj0 <= rj_bounds[1]):
        return None
    flip = _walk_flip(lambda rj: point_occluded(ci, ri, cj, rj, probe, s, fused), rj0, lo_bound=F(0.0))
    if flip is None:
        return None
    r_exp, r_occ = flip
    vx, vy, vz, lim_e = pair_terms(ci, ri, cj, r_exp, probe)
    dot = point_dot(s, (vx, vy, vz), fused)
    lim_o = pair_terms(ci, ri, cj, r_occ, probe)[3]
    tie = bool(dot == lim_e) if fused else bool(dot == lim_o)
    radii = _radius_variants(r_exp, r_occ, lim_e, R, F(r_exp) + F(probe))
    ec = [c for c, _ in extra]
    er = [r for _, r in extra]
    sts = [Structure.of([ci, cj] + ec, [ri, r] + er) for r in radii]
    case = Case(family, float(probe), n_points, W, sts, 0, tie, edge, label,
                meta={"k": k, "fused": fused, "dot": float(dot), "limit": float(lim_e if fused else lim_o),
                      "rj": float(r_exp)})
    lo = Structure.of([ci, cj] + ec, [ri, ulps(r_exp, -4)] + er)
    hi = Structure.of([ci, cj] + ec, [ri, ulps(r_occ, 4)] + er)
    return case if _confirmed(case, lo, hi) else None


def _coord_case(family, probe, n_points, W, ci, ri, rj, k, w, edge="", label=""):
    """Neighbour j of fixed radius rj placed at distance rj + probe from point k of atom i (atom 0), in direction w;
    its coordinate along w's largest component walks to the flip of point k."""
    sx, sy, sz = sphere(n_points)
    s = (sx[k], sy[k], sz[k])
    fused = k < n_fused(n_points, W)
    ci = np.array(ci, np.float32)
    R = F(ri) + F(probe)
    cj = np.array([float(ci[a]) + float(R) * float(s[a]) + (float(rj) + float(probe)) * float(w[a])
                   for a in range(3)], np.float32)
    a = int(np.argmax(np.abs(w)))

    def at(xa):
        q = cj.copy()
        q[a] = xa
        return q

    def occ(xa):
        return point_occluded(ci, ri, at(xa), rj, probe, s, fused)
    if w[a] > 0:  # a larger coordinate takes j away from the point
        flip = _walk_flip(lambda xa: not occ(xa), cj[a])
        if flip is None:
            return None
        x_occ, x_exp = flip
        out = 1
    else:
        flip = _walk_flip(occ, cj[a])
        if flip is None:
            return None
        x_exp, x_occ = flip
        out = -1
    xs = [x_exp, x_occ, ulps(x_exp, out), ulps(x_occ, -out), ulps(x_exp, 3 * out), ulps(x_occ, -3 * out)]
    vx, vy, vz, lim_e = pair_terms(ci, ri, at(x_exp), rj, probe)
    # offsets of m 2^-11 |limit| in dot - limit: its derivative along the coordinate is -(s_a + v_a / R)
    g = abs(float(s[a]) + float((vx, vy, vz)[a]) / float(R))
    if g > 1e-3:
        step = abs(float(lim_e)) * 2.0 ** -11 / g
        for m in (1, 2, 4, 8):
            for sgn in (-1, 1):
                xs.append(F(float(x_exp) + sgn * m * step))
    dot = point_dot(s, (vx, vy, vz), fused)
    vo = pair_terms(ci, ri, at(x_occ), rj, probe)
    dot_o = point_dot(s, vo[:3], fused)
    tie = bool(dot == lim_e) if fused else bool(dot_o == vo[3])
    sts = [Structure.of([ci, at(x)], [ri, rj]) for x in xs]
    case = Case(family, float(probe), n_points, W, sts, 0, tie, edge, label,
                meta={"k": k, "fused": fused, "dot": float(dot if fused else dot_o),
                      "limit": float(lim_e if fused else vo[3])})
    lo = Structure.of([ci, at(ulps(x_exp, 4 * out))], [ri, rj])
    hi = Structure.of([ci, at(ulps(x_occ, -4 * out))], [ri, rj])
    return case if _confirmed(case, lo, hi) else None


def _unit(rng, mode="random"):
    if mode == "diag":
        u = rng.choice([-1.0, 1.0], 3)
    elif mode == "axis":
        u = np.zeros(3)
        u[rng.integers(3)] = rng.choice([-1.0, 1.0])
    else:
        u = rng.normal(size=3)
    return u / np.linalg.norm(u)


def _pick_point(rng, n_points, W, rem: bool, ks=None):
    nf = n_fused(n_points, W)
    if ks is not None:
        return int(rng.choice(ks))
    if rem:
        return int(rng.integers(nf, n_points))
    return int(rng.integers(0, nf))


def _flip_family(rng, family, want, settings, rem, tries=40, rj_target=None, want_ties=0, max_other=None, **kw):
    """Cases of a family: for each (probe, n_points, W, ri range, |v| range, direction mode) in turn, random
    configurations until `want` confirmed cases (`tries` attempts per case).  With rj_target = (lo, hi) the
    neighbour is placed instead: at distance r_j + probe from point k, in a random direction, r_j drawn from it."""
    out = []
    i = 0
    attempts = 0
    n_ties = 0
    while (len(out) < want or n_ties < want_ties) and attempts < max(want, want_ties) * tries:
        probe, n_points, W, ri_rng, d_rng, mode = settings[i % len(settings)]
        attempts += 1
        ri = F(rng.uniform(*ri_rng)) if isinstance(ri_rng, tuple) else F(ri_rng)
        ci = F(rng.uniform(-40, 40, 3))
        k = _pick_point(rng, n_points, W, rem)
        if rj_target is None:
            v = F(_unit(rng, mode) * rng.uniform(*d_rng))
        else:
            sx, sy, sz = sphere(n_points)
            s = np.array([sx[k], sy[k], sz[k]], float)
            R = float(F(ri) + F(probe))
            v = F(-(R * s + (rng.uniform(*rj_target) + probe) * _unit(rng)))
        c = _radius_case(rng, family, probe, n_points, W, ci, ri, v, k, **kw)
        if c is not None and (c.tie or max_other is None or len(out) - n_ties < max_other):
            out.append(c)
            n_ties += c.tie
            i += 1
    return out


def _fused_ties(rng, want):
    # point counts of 4 to 8 tiles of 16 (k_occlusion_mx's NT), without and with remainder points
    settings = [(1.4, n, W, (1.0, 2.0), (1.5, 5.5), "random") for n in (64, 96, 112, 128) for W in (1, 4, 8, 16)]
    settings += [(1.4, n, W, (1.0, 2.0), (1.5, 5.5), "random") for n, W in ((100, 8), (100, 16), (103, 4))]
    return _flip_family(rng, "fused", 0, settings, rem=False, want_ties=want, max_other=want // 2)


def _remainder_ties(rng, want):
    settings = []
    for n_points, W in ((35, 8), (63, 4), (66, 16), (100, 8), (103, 4), (127, 4), (110, 16)):
        settings.append((1.4, n_points, W, (1.0, 2.0), (1.5, 5.5), "random"))
    return _flip_family(rng, "remainder", 0, settings, rem=True, want_ties=want, max_other=want // 2)


def _range_edges(rng, want):
    """k_occlusion_mx's admission range (occlusion_mx.inc ok_atoms): probe in [0, 32], R = r + probe >= 0.5,
    sr = r + max_r + 2 probe <= 64, every radius in [0, 64]; each edge and one f32 step beyond it."""
    out = {}

    def run(edge, settings, rem=False, **kw):
        out[edge] = _flip_family(rng, "range", want, settings, rem, edge=edge, label=edge, **kw)

    run("probe0", [(0.0, 100, 8, (1.0, 2.5), (1.0, 4.0), "random"), (0.0, 100, 8, (1.0, 2.5), (1.0, 4.0), "diag")])
    # (one step below probe 0 is no input: the API rejects negative probes)
    # probe 32 with every radius 0: R = 32 and sr = 64 exactly; a coordinate of the neighbour walks to the flip
    for edge, probe in (("probe32", F(32.0)), ("probe32_plus", ulps(32.0, 1))):
        lst = []
        for _ in range(want * 40):
            if len(lst) >= want:
                break
            k = int(rng.integers(0, 96))
            sx, sy, sz = sphere(100)
            w = _unit(rng)
            if np.dot(w, [sx[k], sy[k], sz[k]]) > 0.9:
                continue  # (|v| = 32 |s + w| stays below sr = 64)
            c = _coord_case("range", probe, 100, 8, F(rng.uniform(-40, 40, 3)), F(0.0), F(0.0), k, w,
                            edge=edge, label=edge)
            if c is not None:
                lst.append(c)
        out[edge] = lst
    run("R_half", [(0.0, 100, 8, 0.5, (0.8, 3.0), "random"), (0.0, 100, 8, 0.5, (0.8, 3.0), "diag")])
    run("R_half_minus", [(0.0, 100, 8, float(ulps(0.5, -1)), (0.8, 3.0), "random")])
    # sr exactly 64: probe 16, r_i = max_r = 16 (a third atom far away holds max_r), r_j below it
    big = [((F(200.0), F(200.0), F(200.0)), F(16.0))]
    run("sr64", [(16.0, 100, 8, 16.0, None, None)], extra=big, rj_target=(2.0, 15.0), rj_bounds=(0.0, 15.9))
    # (r_i = max_r two steps above 16: r_i + max_r + 32 = 64 + one step; one step above 16 rounds back to 64)
    run("sr64_plus", [(16.0, 100, 8, float(ulps(16.0, 2)), None, None)], extra=big, rj_target=(2.0, 15.0),
        rj_bounds=(0.0, 15.9))
    # a radius of exactly 64 in the structure (and one step above it): no atom of it can be admitted - with max_r = 64,
    # sr <= 64 needs r = probe = 0 and then R < 0.5 - so both hand the whole structure to the general kernel
    r64 = [((F(400.0), F(400.0), F(400.0)), F(64.0))]
    r64p = [((F(400.0), F(400.0), F(400.0)), ulps(64.0, 1))]
    run("radius64", [(1.4, 100, 8, (1.0, 2.0), (1.5, 5.0), "random")], extra=r64)
    run("radius64_plus", [(1.4, 100, 8, (1.0, 2.0), (1.5, 5.0), "random")], extra=r64p)
    # the largest |limit| a flip allows (|limit| <= |v| <= sr <= 64) with R = 0.5 and v along a cube diagonal:
    # a neighbour of radius ~ |v| with atom i on its surface
    run("large_limit_diag", [(0.0, 100, 8, 0.5, (40.0, 62.0), "diag")], rj_bounds=(30.0, 63.4))
    return out


def _f16_subnormal_v(rng, want):
    """Nearly concentric atoms: |v| of a few 1e-6, every component in f16's subnormal range (steps of 2^-24) just
    below a step, so that k_occlusion_mx's f16 filter (prep: v rounded towards zero) loses almost a step per component;
    v along point k, the point covered last, whose flip is walked.  Only the filter's constant 3e-4 covers this loss
    (2^-9 of |v| and of |limit| are far smaller)."""
    out = []
    q = 2.0 ** -24
    settings = [(100, 8), (64, 16), (128, 4), (103, 4), (960, 8), (129, 8)]
    attempts = 0
    while len(out) < want and attempts < 40 * want:
        n_points, W = settings[len(out) % len(settings)]
        attempts += 1
        sx, sy, sz = sphere(n_points)
        k = _pick_point(rng, n_points, W, rem=n_fused(n_points, W) < n_points and rng.random() < 0.3)
        s = np.array([sx[k], sy[k], sz[k]], float)
        mag = rng.uniform(1e-6, 4e-6)
        v = np.array([np.sign(c) * (np.floor(abs(c) * mag / q) + 0.97) * q for c in s], np.float32)
        ri = F(rng.choice([0.5, 0.75, 1.0]))
        case = _radius_case(rng, "f16_subnormal_v", 0.0, n_points, W, (F(0.0), F(0.0), F(0.0)), ri, v, k,
                            label="f16_subnormal_v")
        if case is not None:
            out.append(case)
    return out


def _patch_rims(rng, want):
    """More than 128 points: a neighbour on the line through a patch's centre; the patch's last covered point
    flips."""
    out = []
    settings = [(129, 8), (144, 16), (960, 8), (1100, 8), (1344, 16), (960, 16)]
    attempts = 0
    while len(out) < want and attempts < 40 * want:
        n_points, W = settings[len(out) % len(settings)]
        attempts += 1
        pts = patches(n_points, W)
        sx, sy, sz = sphere(n_points)
        p = pts[int(rng.integers(len(pts) - 1))]  # (a whole patch of fused-rule points)
        c = np.array([sx[p].sum(), sy[p].sum(), sz[p].sum()], float)
        c /= np.linalg.norm(c)
        probe = F(rng.choice([1.4, 0.0, 4.0]))
        ri = F(rng.uniform(1.0, 2.5))
        D = float(rng.uniform(1.5, 6.0))
        ci = F(rng.uniform(-40, 40, 3))
        v = F(-c * D)  # j on the patch's side of atom i
        # the point of the patch covered last: largest s . v
        dots = sx[p] * v[0] + sy[p] * v[1] + sz[p] * v[2]
        k = int(p[int(np.argmax(dots))])
        case = _radius_case(rng, "patch", probe, n_points, W, ci, ri, v, k, label=f"patch{len(pts)}")
        if case is not None:
            out.append(case)
    return out


def _cutoffs(rng, want):
    """A neighbour at exactly the candidate cutoff d^2 = sr^2 (= max_search^2 when r_i = max_r), on an axis and on
    diagonals, one coordinate walked to where the candidate count K changes; and atoms on cell faces with a
    neighbour two cells away."""
    out = []
    attempts = 0
    n_exact = 0
    while (len(out) < want or n_exact < want) and attempts < 40 * want:
        attempts += 1
        probe = F(rng.choice([1.4, 0.0, 0.7]))
        ri = F(rng.uniform(1.0, 2.0))
        rj = F(rng.uniform(1.0, 2.0)) if rng.random() < 0.5 else ri  # (r_i = max_r: the max_search cutoff too)
        max_r = F(max(ri, rj))
        sr = ri + max_r + F(2.0) * probe
        mode = ["axis", "diag", "random"][len(out) % 3]
        u = _unit(rng, mode)
        ci = F(rng.uniform(-20, 20, 3))
        a = int(np.argmax(np.abs(u)))
        cj = F(ci - u * float(sr))
        sgn = -1.0 if u[a] > 0 else 1.0  # moving cj[a] by sgn grows the distance

        def outside(xa, cj=cj, a=a):
            q = cj.copy()
            q[a] = xa
            return len(candidates(Structure.of([ci, q], [ri, rj]), probe)[0]) == 0
        # the pair leaves the list as cj[a] moves by sgn: a walk on the f32 values of that coordinate
        if sgn > 0:
            flip = _walk_flip(outside, cj[a])
            if flip is None:
                continue
            x_in, x_out = flip
        else:
            flip = _walk_flip(lambda xa: not outside(xa), cj[a])
            if flip is None:
                continue
            x_out, x_in = flip
        step = 1 if sgn > 0 else -1
        xs = [x_in, x_out, ulps(x_in, -step), ulps(x_out, step)]
        sts = []
        for xa in xs:
            q = cj.copy()
            q[a] = xa
            sts.append(Structure.of([ci, q], [ri, rj]))
        d = [ci[t] - sts[0].centre(1)[t] for t in range(3)]
        exact = bool(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] == sr * sr)  # (the inside side: d^2 == sr^2 in f32)
        case = Case("cutoff", float(probe), 100, 8, sts, 0, exact, "", f"cutoff_{mode}", want_k_change=True)
        if (exact or len(out) < want) and _confirmed(case, sts[0], sts[1]):
            out.append(case)
            n_exact += exact
    # cell faces: atom coordinates min + m cell_size exactly (min = the smallest coordinate - cell_size), a neighbour
    # two cells away along an axis and along a diagonal
    for probe, r in ((1.4, 1.5), (0.0, 2.0), (1.0, 1.0), (0.5, 1.5)):
        cell = F(probe) + F(r)
        for m in (1, 2, 3):
            for d in ((2, 0, 0), (2, 2, 0), (2, 2, 2), (0, 2, 1)):
                base = np.array([F(3.0), F(-7.0), F(11.0)], np.float32)
                ci = base + F(m) * cell
                cj = np.array([ci[k] + F(d[k]) * cell for k in range(3)], np.float32)
                st = Structure.of([base, ci, cj], [r, r, r])
                out.append(Case("cellface", float(probe), 100, 8, [st], 1, False, "", "cellface"))
    return out


def _fold_collisions(rng, want):
    """Atoms i, j with different 64-bit ids and equal 32-bit folds, j occluding points of i; controls with equal
    ids and with unrelated ids (structures of their own).  The ids fall, so they stay in play."""
    out = []
    while len(out) < want:
        probe = F(1.4)
        ci = F(rng.uniform(-30, 30, 3))
        v = F(_unit(rng) * rng.uniform(2.0, 3.5))
        cj = F(ci - v)
        r = [F(rng.uniform(1.2, 1.9)), F(rng.uniform(1.2, 1.9))]
        a = int(rng.integers(1 << 40, 1 << 63))
        b = colliding_id(a, int(rng.integers(1, 1 << 31)))
        if b == a or fold_id(b) != fold_id(a):
            continue
        hi, lo = max(a, b), min(a, b)
        third = F(ci + F(_unit(rng) * 2.8))
        unrelated = int(rng.integers(1, 1 << 40))
        # (and the colliding pair beside a far pair of equal ids: hash tables over the full ids keep this structure's ids)
        f1, f2 = F(ci + F(40.0)), F(ci + F(np.array([41.5, 40.0, 40.0])))
        sts = [Structure.of([ci, cj, third], r + [F(1.5)], [hi, lo, 7]),            # colliding folds
               Structure.of([ci, cj, third], r + [F(1.5)], [hi, hi, 7]),            # equal ids
               Structure.of([ci, cj, third], r + [F(1.5)], [unrelated + 9, unrelated, 7]),  # unrelated ids
               Structure.of([ci, cj, third, f1, f2], r + [F(1.5)] * 3, [hi, lo, 7, 9, 9])]
        vals = [oracle_counts(s, probe, 100, 8)[1] for s in sts]
        if vals[0][0] == vals[1][0]:
            continue  # j does not reach any point of i
        out.append(Case("fold", float(probe), 100, 8, sts, 0, False, "", "fold",
                        meta={"ids": (hi, lo)}))
    return out


# the minimum numbers of oracle-confirmed cases per family (and per edge of family c)
MINIMUM = {"fused_ties": 200, "remainder_ties": 100, "patch": 50, "range_edge": 20, "cutoff": 20, "cutoff_exact": 20,
           "fold": 10, "f16_subnormal_v": 20}


@functools.lru_cache(maxsize=None)
def generate(seed: int = 20261016):
    """All families, seeded.  {"fused": [...], "remainder": [...], "range": {edge: [...]}, "patch": [...],
    "cutoff": [...], "fold": [...]}."""
    rng = np.random.default_rng(seed)
    fam = {}
    fam["fused"] = _fused_ties(rng, 220)
    fam["remainder"] = _remainder_ties(rng, 110)
    fam["range"] = _range_edges(rng, 24)
    fam["patch"] = _patch_rims(rng, 60)
    fam["cutoff"] = _cutoffs(rng, 30)
    fam["fold"] = _fold_collisions(rng, 16)
    fam["f16_subnormal_v"] = _f16_subnormal_v(rng, 30)
    return fam


def all_cases(seed: int = 20261016):
    fam = generate(seed)
    out = []
    for k, v in fam.items():
        if isinstance(v, dict):
            for lst in v.values():
                out += lst
        else:
            out += v
    return out


def report(seed: int = 20261016) -> dict:
    """Confirmed-case counts (exact ties counted apart)."""
    fam = generate(seed)
    rep = {"fused_ties": sum(c.tie for c in fam["fused"]), "fused": len(fam["fused"]),
           "remainder_ties": sum(c.tie for c in fam["remainder"]), "remainder": len(fam["remainder"]),
           "patch": len(fam["patch"]), "cutoff": sum(c.family == "cutoff" for c in fam["cutoff"]),
           "cutoff_exact": sum(c.family == "cutoff" and c.tie for c in fam["cutoff"]),
           "cellface": sum(c.family == "cellface" for c in fam["cutoff"]), "fold": len(fam["fold"]),
           "f16_subnormal_v": len(fam["f16_subnormal_v"])}
    for edge, lst in fam["range"].items():
        rep["range_" + edge] = len(lst)
    return rep


def pack(structures):
    """Concatenates structures into batch columns (x, y, z, r, ids, structure offsets)."""
    so = np.zeros(len(structures) + 1, np.uint32)
    so[1:] = np.cumsum([s.n for s in structures])
    cat = lambda name: np.concatenate([getattr(s, name) for s in structures])  # noqa: E731
    return cat("x"), cat("y"), cat("z"), cat("r"), cat("ids"), so


# ---- the max_search cutoff of the neighbour lists (not part of generate(): the SASA path always uses max_r) --------

@dataclass
class MsCutoff:
    """Atom 1 at d^2 == max_search^2 from atom 0 exactly (in f32) for max_radius `m_in`, max_radius given below r_0 so
    the max_search test binds.  `inside` / `outside`: max_radius values (the flip and one more f32 step each way) for
    which the oracle does / does not list atom 1 for atom 0."""
    st: Structure
    probe: float
    m_in: float
    inside: tuple
    outside: tuple


def _in_list0(st: Structure, probe, max_radius) -> bool:
    lists = po.neighbor_lists(*st.soa(), probe_radius=probe, max_radius=max_radius)
    return 1 in lists[0]["idx"].tolist()


@functools.lru_cache(maxsize=None)
def ms_cutoffs(seed: int = 20261017, want: int = 24):
    """Pairs at exactly d^2 == max_search^2, max_search = 2 max_radius + 2 probe, with max_radius below r_0 (so
    sr_0 = r_0 + max_radius + 2 probe is larger and only max_search decides): one coordinate of atom 1 is walked in
    f32 steps to where d^2 <= max_search^2 flips and kept if d^2 equals max_search^2 there; then max_radius is walked
    in f32 steps to where the oracle's list of atom 0 changes, which must be at that max_radius.  Kept: the cases the
    oracle confirms on both sides, at the flip and one f32 step beyond it."""
    rng = np.random.default_rng(seed)
    out = []
    attempts = 0
    while len(out) < want and attempts < 400 * want:
        attempts += 1
        probe = F(rng.choice([1.4, 0.7, 0.0]))
        m = F(rng.uniform(0.8, 1.6))
        ri = F(m + F(rng.uniform(0.3, 1.0)))
        rj = F(rng.uniform(0.5, 2.5))
        ms = m + m + F(2.0) * probe
        ms2 = ms * ms
        u = _unit(rng, "diag" if len(out) % 2 else "random")
        ci = F(rng.uniform(-20, 20, 3))
        cj = F(ci - u * float(ms))
        a = int(np.argmax(np.abs(u)))

        def d2_of(xa, cj=cj, a=a):
            q = cj.copy()
            q[a] = xa
            d = ci - q
            return d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        flip = _walk_flip(lambda xa: not d2_of(xa) <= ms2, cj[a]) if u[a] < 0 else \
            _walk_flip(lambda xa: d2_of(xa) <= ms2, cj[a])
        if flip is None:
            continue
        x_in = flip[0] if u[a] < 0 else flip[1]
        if d2_of(x_in) != ms2:
            continue
        q = cj.copy()
        q[a] = x_in
        st = Structure.of([ci, q], [ri, rj])
        mflip = _walk_flip(lambda mr: _in_list0(st, probe, mr), m)
        if mflip is None or mflip[1] != m:
            continue  # (the grid's reach, not max_search, decides this pair)
        inside, outside = (m, ulps(m, 1)), (mflip[0], ulps(mflip[0], -1))
        if all(_in_list0(st, probe, v) for v in inside) and not any(_in_list0(st, probe, v) for v in outside):
            out.append(MsCutoff(st, float(probe), float(m), tuple(float(v) for v in inside),
                                tuple(float(v) for v in outside)))
    return out
