"""The routing of one k_occlusion_mx launch (rustsasa_amd/csrc/occlusion_mx.inc), emulated in numpy: which integers
decide what code an atom runs through - NOT a second SASA oracle (values always come from oracle/pyoracle.py).

For a batch (columns, structure offsets, probe, n_points, lane count W, ids or None, atoms per wave) and an order of
the atoms inside a cell the model follows the launch: the cell-sorted order (cells x fastest, structures in batch
order; the grid is tail_cases.grid_of / cell_index, pinned to the engine), the blocks of atoms_per_wave atoms, each
structure's group shift, the group starts, a group's union size U and its narrowing, chunk count and self0, the three
reasons a whole group is left to the general kernel, and per atom the candidate count K (the reference's rule in
float32 as sweep_chunk writes it), the fold rule, the near count, prep's second pass and - for atoms with K <= 16,
whose candidates all sit in tile 0 - bounds on the number of points the f16 filter leaves to phase B and, above 128
points, on the tiles of 16 points that outlive the patch test (live_tile_bounds).

Which instantiation takes a structure: the one with ids (256 union slots) if two of its ids are equal, the id-less
one (320 slots, the 1.95 bump of the shift) otherwise - what the device's id check decides for ids that rise apart
from the equal ones (mx_cases.py builds no others).

The keyword switches exist only so that the CPU tests can show that a case bites; each is one way the kernel could
be wrong.  Plain helper module (not a conftest)."""
import functools
from dataclasses import dataclass, field

import numpy as np

import tail_cases as tc
import tie_cases as ti

F = np.float32
CAP = 128            # kMxCap
UNION_IDS = 256      # kMxUnion
UNION_NO_IDS = 320   # 64 * NS, NS = 5
MAX_SHIFT = 3        # kMxXShift
APW = 64             # kMxAtoms
APW_MULTI = 16       # kMxAtomsMulti
NEAR_SCALE2 = F(1.8)  # kMxNearScale2


def grid_group_shift(n_atoms, n_cells):
    """device_types.h grid_group_shift, in float32."""
    per_cell = F(n_atoms) / F(n_cells if n_cells else 1)
    return 0 if per_cell >= F(1.0) else 1 if per_cell >= F(0.6) else 2 if per_cell >= F(0.3) else 3


def group_shift(n_atoms, n_cells, has_ids):
    """The shift k_occlusion_mx groups a structure's atoms by: grid_group_shift capped at 3; the id-less instantiation
    takes 1 for 0 when n_atoms < 1.95 n_cells (float32)."""
    s = min(grid_group_shift(n_atoms, n_cells), MAX_SHIFT)
    if not has_ids and s == 0 and F(n_atoms) < F(1.95) * F(n_cells):
        s = 1
    return s


def launch_apw(n_atoms, n_points, forced=None):
    """launch_occlusion's atoms per wave: the forced value within the kernel's limit, or halved from the limit while
    more than 8 and apw x (256 x 4 x 7 x rounds) exceeds the batch."""
    multi = n_points > 128
    apw_max = APW_MULTI if multi else APW
    if forced:
        return min(int(forced), apw_max)
    rounds = 16 if multi else 4
    apw = apw_max
    while apw > 8 and apw * (256 * 4 * 7 * rounds) > n_atoms:
        apw >>= 1
    return apw


def pieces(n_atoms, apw, nw, resident=1 << 30):
    """The persistent launches' (more than 128 points) pieces: (workgroups, blocks of every piece)."""
    n_wg = min(-(-n_atoms // (nw * apw)), resident)
    n_wblocks = -(-n_atoms // apw)
    n_pieces = min(8, n_wg)
    per = -(-n_wblocks // n_pieces)
    out = []
    for p in range(n_pieces):
        first = min(p * per, n_wblocks)
        out.append(min(per, n_wblocks - first))
    return n_wg, out


@dataclass
class Struct:
    base: int                 # first cell-sorted position
    n: int
    dims: np.ndarray
    n_cells: int
    max_r: np.float32
    has_ids: bool             # the instantiation with ids takes it
    shift: int
    admitted: np.ndarray      # bool per atom (input order within the structure): ok_atoms
    starts: np.ndarray        # cell -> first cell-sorted position (absolute), n_cells + 1 entries


@dataclass
class Group:
    g0: int                   # cell-sorted positions [g0, g1)
    g1: int
    sid: int
    block: int
    cx_first: int
    cx_last: int
    U_first: int              # the union before any narrowing
    U: int
    narrowed: int             # times the group was narrowed
    n_chunk: int
    self0: int
    reason: str               # "" (taken), "union", "range", "first_chunk"
    cut_by_block: bool        # it starts on a block's first atom and on nothing else


@dataclass
class Launch:
    apw: int
    order: np.ndarray         # cell-sorted position -> input index
    cell: np.ndarray          # cell-sorted position -> cell index within the structure
    sid: np.ndarray           # cell-sorted position -> structure
    structs: list
    blocks: list              # (first, behind)
    groups: list
    K: np.ndarray             # input order; -1 where the kernel never counts (atoms of deferred groups)
    K_all: np.ndarray         # input order: the candidate rule over the atom's own 5 x 5 x 5 block, every atom
    near: np.ndarray          # input order; -1 as above
    reason: np.ndarray        # input order: "" taken, "union" / "range" / "first_chunk" (group), "cap", "fold"
    lo: np.ndarray            # input order: survivor bounds, -1 where not computed (K > 16, deferred, no bounds asked)
    hi: np.ndarray
    rem_exposed: np.ndarray   # input order: exposed remainder points where lo / hi are computed
    group_of: np.ndarray = field(default=None)  # input order -> index into groups

    @property
    def deferred(self):
        return np.flatnonzero(self.reason != "")

    @property
    def n_deferred(self):
        return int((self.reason != "").sum())

    @property
    def second_pass(self):
        return self.K > 64

    def table(self):
        """The group table as plain tuples (for comparisons between switches and orders)."""
        return [(g.g0, g.g1, g.U, g.narrowed, g.n_chunk, g.self0, g.reason) for g in self.groups]


def keeps_ids(ids):
    """Two equal ids in the structure."""
    return len(np.unique(ids)) < len(ids)


def _cells(x, y, z, r, probe):
    mn, inv, dims = tc.grid_of(x, y, z, r, probe)
    c = [np.minimum(((a - mn[k]) * inv).astype(np.int64), dims[k] - 1) for k, a in enumerate((x, y, z))]
    idx = c[0] + c[1] * dims[0] + c[2] * dims[0] * dims[1]
    if len(x):
        assert np.array_equal(idx, tc.cell_index(x, y, z, mn, inv, dims))
    return np.asarray(dims, np.int64), np.stack(c, -1) if len(x) else np.zeros((0, 3), np.int64), idx


def survivor_bounds(ci, R, cands, probe, n_points, W):
    """(lo, hi, exposed remainder points) for an atom at ci with R = r + probe and candidate records (x, y, z, r), all in
    tile 0.  lo: fused-rule points no candidate occludes.  hi: those whose float32 dot - limit is, for every candidate,
    not below minus twice the margin prep lowers the f16 limit by."""
    sx, sy, sz = ti.sphere(n_points)
    nf = ti.n_fused(n_points, W)
    occluded = np.zeros(nf, bool)
    surely_dead = np.zeros(nf, bool)
    rem_occ = np.zeros(n_points - nf, bool)
    R = F(R)
    R2 = R * R
    twoR = F(2.0) * R
    for o in cands:
        vx, vy, vz = F(ci[0]) - F(o[0]), F(ci[1]) - F(o[1]), F(ci[2]) - F(o[2])
        d2 = vx * vx + vy * vy + vz * vz
        tj = F(o[3]) + F(probe)
        limit = (tj * tj - d2 - R2) / twoR
        dot = ti.fmaf_vec(sx[:nf], vx, ti.fmaf_vec(sy[:nf], vy, sz[:nf] * vz))
        occluded |= dot < limit
        m3 = np.abs(vz) + np.abs(vy) + np.abs(vx)
        a = ti.fmaf(m3, F(1.5 * 2.0 ** -9), F(3e-4))
        lim = limit - a
        margin = float(a) + 2.0 ** -9 * abs(float(lim))
        diff = ti.fmaf_vec(np.full(nf, -1.0, F), np.full(nf, limit, F), dot)   # dot - limit as the matrix pipe rounds it
        surely_dead |= diff.astype(np.float64) < -2.0 * margin
        if nf < n_points:
            rem_occ |= (sx[nf:] * vx + sy[nf:] * vy + sz[nf:] * vz) <= limit
    return int((~occluded).sum()), int((~surely_dead).sum()), int((~rem_occ).sum())


def _f16_rtz(v):
    """float32 -> float16 towards zero (v_cvt_pkrtz_f16_f32), as float64."""
    v = float(F(v))
    h = np.float16(v)
    if abs(float(h)) > abs(v):
        h = np.nextafter(h, np.float16(0.0))
    return float(h)


def _f16_up(v):
    """float32 -> float16 towards +inf (context.cpp f16_round_up), as float64."""
    v = float(F(v))
    h = np.float16(v)
    if float(h) < v:
        h = np.nextafter(h, np.float16(np.inf))
    return float(h)


@functools.lru_cache(maxsize=None)
def _patch_table(n_points, W):
    """(centres as f16 [n_patches, 3], eps as f16 rounded up) of context.cpp's patch table, as float64."""
    sx, sy, sz = ti.sphere(n_points)
    cs, es = [], []
    for p in ti.patches(n_points, W):
        q = np.stack([sx[p], sy[p], sz[p]], -1).astype(np.float64)
        c = q.sum(0)
        c16 = np.array([float(np.float16(F(v))) for v in c / np.sqrt((c * c).sum())])
        eps = float(np.sqrt(((q - c16) ** 2).sum(1)).max())
        cs.append(c16)
        es.append(_f16_up(F(eps * 1.001 + 1e-4)))
    return np.array(cs), np.array(es)


def live_tile_bounds(ci, R, cands, probe, n_points, W):
    """More than 128 points: bounds (lo, hi) on the tiles of 16 points the patch test leaves alive, for an atom whose
    candidates all sit in tile 0, and the tiles that hold a point no candidate occludes.  The table entries are
    context.cpp's (centre: the normalised sum of the patch's points as f16, eps: the largest distance to it, times 1.001
    plus 1e-4, rounded up), the candidate's operands prep's (v and the lowered limit towards zero, 1.002 |v| towards
    zero).  The five products are exact in float64; a tile counts as surely dead / surely alive when the sum is beyond
    2^-18 of the terms' sizes - more than a float32 accumulation in any order can be off by."""
    sx, sy, sz = ti.sphere(n_points)
    nf = ti.n_fused(n_points, W)
    pts = ti.patches(n_points, W)
    R = F(R)
    ops = []
    exposed = np.ones(n_points, bool)
    for o in cands:
        vx, vy, vz = F(ci[0]) - F(o[0]), F(ci[1]) - F(o[1]), F(ci[2]) - F(o[2])
        d2 = vz * vz + vy * vy + vx * vx
        tj = F(o[3]) + F(probe)
        limit = (tj * tj - d2 - R * R) / (F(2.0) * R)
        m3 = np.abs(vz) + np.abs(vy) + np.abs(vx)
        lim = limit - ti.fmaf(m3, F(1.5 * 2.0 ** -9), F(3e-4))
        lim = ti.fmaf(F(-2.0 ** -9), np.abs(lim), lim)
        ops.append((_f16_rtz(vx), _f16_rtz(vy), _f16_rtz(vz), _f16_rtz(lim), _f16_rtz(F(1.002) * np.sqrt(d2))))
        dot = ti.fmaf_vec(sx[:nf], vx, ti.fmaf_vec(sy[:nf], vy, sz[:nf] * vz))
        exposed[:nf] &= ~(dot < limit)
        exposed[nf:] &= ~((sx[nf:] * vx + sy[nf:] * vy + sz[nf:] * vz) <= limit)
    c16, eps16 = _patch_table(n_points, W)
    dead = np.zeros(len(pts), bool)
    alive = np.ones(len(pts), bool)
    for vx, vy, vz, lim, vn in ops:
        terms = np.stack([c16[:, 2] * vz, c16[:, 1] * vy, c16[:, 0] * vx, np.full(len(pts), -lim), eps16 * vn])
        d, slack = terms.sum(0), 2.0 ** -18 * np.abs(terms).sum(0)
        dead |= d < -slack
        alive &= d > slack
    lo, hi = alive.sum(), (~dead).sum()
    with_exposed = [(k, bool(dead[k])) for k, p in enumerate(pts) if exposed[p].any()]
    return int(lo), int(hi), with_exposed


def launch(x, y, z, r, so, probe, n_points, W, ids=None, atoms_per_wave=None, order="asc", bounds=False,
           cap=CAP, union_delta=0, first_chunk_rule=True, midpoint_up=False, block_starts=True, dims_or=False):
    """One launch of k_occlusion_mx over the batch.  order: "asc" / "desc" - the atoms of a cell by rising / falling
    input index.  The last six keywords are the switches (see the module's text); dims_or: the grid's size
    tested on the bitwise OR of the three cell counts, which 1024 cells on one axis and any on another exceed."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    so = np.asarray(so, np.int64)
    N = len(x)
    probe = F(probe)
    apw = launch_apw(N, n_points, atoms_per_wave)
    structs, order_l, cell_l, sid_l, cxyz_l = [], [], [], [], []
    base = 0
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        n = e - b
        dims, c3, idx = _cells(x[b:e], y[b:e], z[b:e], r[b:e], probe)
        n_cells = int(np.prod(dims))
        has_ids = ids is not None and n > 0 and keeps_ids(ids[b:e])
        st = ti.Structure(x[b:e], y[b:e], z[b:e], r[b:e], None)
        max_r = F(np.max(r[b:e], initial=F(0.0)))
        radii_bad = bool(((r[b:e] < 0) | (r[b:e] > F(64.0))).any())
        # (tie_cases.mx_admits, once per distinct radius: the verdict depends on the atom through its radius alone)
        rr = r[b:e]
        verdict = {float(v): ti.mx_admits(st, probe, int(np.flatnonzero(rr == v)[0])) for v in np.unique(rr)}
        adm = np.array([verdict[float(v)] for v in rr], bool) & (not radii_bad) & bool(
            (int(dims[0]) | int(dims[1]) | int(dims[2])) <= 1024 if dims_or else dims.max() <= 1024)
        key = np.arange(n) if order == "asc" else -np.arange(n)
        o = np.lexsort((key, idx))
        starts = base + np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n_cells))]).astype(np.int64)
        structs.append(Struct(base, n, dims, n_cells, max_r, has_ids, group_shift(n, n_cells, has_ids), adm, starts))
        order_l.append(b + o)
        cell_l.append(idx[o])
        sid_l.append(np.full(n, s, np.int64))
        cxyz_l.append(c3[o])
        base += n
    order_a = np.concatenate(order_l) if order_l else np.zeros(0, np.int64)
    cell = np.concatenate(cell_l) if cell_l else np.zeros(0, np.int64)
    sid = np.concatenate(sid_l) if sid_l else np.zeros(0, np.int64)
    cxyz = np.concatenate(cxyz_l) if cxyz_l else np.zeros((0, 3), np.int64)
    blocks = [(b, min(b + apw, N)) for b in range(0, N, apw)]
    sx_, sy_, sz_, sr_ = x[order_a], y[order_a], z[order_a], r[order_a]
    folds = None if ids is None else np.array([ti.fold_id(int(v)) for v in np.asarray(ids, np.uint64)[order_a]], np.uint64)

    # group starts
    shift_of = np.array([st.shift for st in structs], np.int64)[sid] if N else np.zeros(0, np.int64)
    bx = cxyz[:, 0] >> shift_of
    natural = np.ones(N, bool)
    if N > 1:
        natural[1:] = (sid[1:] != sid[:-1]) | (cxyz[1:, 1] != cxyz[:-1, 1]) | (cxyz[1:, 2] != cxyz[:-1, 2]) | (bx[1:] != bx[:-1])
    forced = np.zeros(N, bool)
    if block_starts:
        forced[[b for b, _ in blocks]] = True
    starts = natural | forced

    def union_rows(st, gcy, gcz, x_lo, x_hi):
        """(first, behind) cell-sorted positions of the 25 x-runs, the own row first; rows outside the grid are empty."""
        rows = []
        dx, dy, dz = (int(v) for v in st.dims)
        for ddz, ddy in [(0, 0)] + [(a, b) for a in range(-2, 3) for b in range(-2, 3) if (a, b) != (0, 0)]:
            yy, zz = gcy + ddy, gcz + ddz
            if 0 <= yy < dy and 0 <= zz < dz:
                c0 = (zz * dy + yy) * dx + x_lo
                rows.append((int(st.starts[c0]), int(st.starts[c0 + (x_hi - x_lo) + 1])))
        return rows

    K = np.full(N, -1, np.int64)
    near = np.full(N, -1, np.int64)
    reason = np.full(N, "", dtype=object)
    lo = np.full(N, -1, np.int64)
    hi = np.full(N, -1, np.int64)
    rem = np.full(N, -1, np.int64)
    group_of = np.full(N, -1, np.int64)
    groups = []
    spans = blocks if block_starts else ([(0, N)] if N else [])
    for bi, (b0, b1) in enumerate(spans):
        g0 = b0
        while g0 < b1:
            later = np.flatnonzero(starts[g0 + 1:b1])
            g1 = g0 + 1 + int(later[0]) if len(later) else b1
            st = structs[int(sid[g0])]
            k_union = (UNION_IDS if st.has_ids else UNION_NO_IDS) + union_delta
            cx_first = int(cxyz[g0, 0])
            gcy, gcz = int(cxyz[g0, 1]), int(cxyz[g0, 2])
            U_first, narrowed = None, 0
            while True:
                cx_last = int(cxyz[g1 - 1, 0])
                x_lo, x_hi = max(cx_first - 2, 0), min(cx_last + 2, int(st.dims[0]) - 1)
                rows = union_rows(st, gcy, gcz, x_lo, x_hi)
                U = sum(e - f for f, e in rows)
                if U_first is None:
                    U_first = U
                if U <= k_union or cx_last == cx_first:
                    break
                mid = (cx_first + cx_last + (1 if midpoint_up else 0)) >> 1
                if mid >= cx_last:
                    mid = cx_last - 1
                g1 = g0 + int(np.flatnonzero(cxyz[g0:g1, 0] > mid)[0])
                narrowed += 1
            n_chunk = (min(U, k_union) + 63) >> 6
            self0 = g0 - rows[0][0]
            inp = order_a[g0:g1]
            adm = st.admitted[inp - int(so[int(sid[g0])])]
            why = ""
            if U > k_union:
                why = "union"
            elif not adm.all():
                why = "range"
            elif first_chunk_rule and self0 + (g1 - g0) > 64:
                why = "first_chunk"
            cut = bool(forced[g0] and not natural[g0])
            group_of[g0:g1] = len(groups)
            groups.append(Group(g0, g1, int(sid[g0]), bi if block_starts else g0 // apw, cx_first, cx_last, U_first, U,
                                narrowed, n_chunk, self0, why, cut))
            if why:
                reason[g0:g1] = why
            else:
                members = np.concatenate([np.arange(f, e) for f, e in rows]) if rows else np.zeros(0, np.int64)
                ox, oy, oz, orr = sx_[members], sy_[members], sz_[members], sr_[members]
                for p in range(g0, g1):
                    my_sr = sr_[p] + st.max_r + F(2.0) * probe
                    sr2 = my_sr * my_sr
                    ddx, ddy, ddz = sx_[p] - ox, sy_[p] - oy, sz_[p] - oz
                    d2 = ddx * ddx + ddy * ddy + ddz * ddz
                    other = members != p
                    acc = (d2 <= sr2) & other
                    K[p] = int(acc.sum())
                    Rr = sr_[p] + probe
                    R2 = Rr * Rr
                    near[p] = int((acc & (d2 < NEAR_SCALE2 * R2)).sum())
                    fold_hit = st.has_ids and bool((folds[members][other] == folds[p]).any())
                    if fold_hit:
                        reason[p] = "fold"
                    elif K[p] > cap:
                        reason[p] = "cap"
                    elif bounds and 0 < K[p] <= 16:
                        cands = [(ox[k], oy[k], oz[k], orr[k]) for k in np.flatnonzero(acc)]
                        lo[p], hi[p], rem[p] = survivor_bounds((sx_[p], sy_[p], sz_[p]), Rr, cands, probe, n_points, W)
            g0 = g1

    # the candidate rule over every atom's own 5 x 5 x 5 block (what the oracle counts, equal ids apart)
    K_all = np.zeros(N, np.int64)
    for p in range(N):
        st = structs[int(sid[p])]
        cx, cy, cz = (int(v) for v in cxyz[p])
        rows = union_rows(st, cy, cz, max(cx - 2, 0), min(cx + 2, int(st.dims[0]) - 1))
        members = np.concatenate([np.arange(f, e) for f, e in rows])
        my_sr = sr_[p] + st.max_r + F(2.0) * probe
        ddx, ddy, ddz = sx_[p] - sx_[members], sy_[p] - sy_[members], sz_[p] - sz_[members]
        d2 = ddx * ddx + ddy * ddy + ddz * ddz
        ok = (d2 <= my_sr * my_sr) & (members != p)
        if ids is not None:
            full = np.asarray(ids, np.uint64)[order_a]
            ok &= full[members] != full[p]
        K_all[p] = int(ok.sum())

    def unsort(a):
        out = np.empty_like(a)
        out[order_a] = a
        return out

    return Launch(apw, order_a, cell, sid, structs, blocks, groups, unsort(K), unsort(K_all), unsort(near),
                  unsort(reason), unsort(lo), unsort(hi), unsort(rem), unsort(group_of))
