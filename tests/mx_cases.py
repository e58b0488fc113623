"""Inputs that sit on the integer limits of k_occlusion_mx (occlusion_mx.inc), each named for its edge; the figures come
from mx_model.py (test_mx_cases_cpu.py pins them, test_gpu_mx_edges.py runs them).

Geometry: probe 0.5 and largest radius 1.5 make the cell 2.0 (reciprocal 0.5, exact) and the candidate cutoff of a
1.5 A atom 4.0 A.  A structure is a list of CLUMPS: n atoms of one radius at the corner of a cell plus an offset, 2^-10 A
apart along x - atoms overlap freely, only the arithmetic matters.  A clump at the corner of cell 1 on every axis puts
the grid's minimum there, so the cells are the ones written down (the builder checks it against the model's grid).
Clumps three cells apart in y or z share no union.

Ids: 1, 2, ... in input order (they rise: the device's id check drops them and the id-less instantiation, 320 union
slots, takes the structure).  `dup=(i, j)` gives atom j atom i's id: the structure then keeps its ids (256 slots).
Plain helper module (not a conftest)."""
import functools
from dataclasses import dataclass, field

import numpy as np

import mx_model as mm
import tie_cases as ti

F = np.float32
PROBE = 0.5
R = 1.5
STEP = 2.0 ** -10
KEY = (8, PROBE, 100)   # (W, probe, n_points) of the cases that do not say otherwise


def clump(cell, n, r=R, f=(0.0, 0.0, 0.0)):
    return (tuple(cell), int(n), float(r), tuple(f))


def build(clumps, dup=None, check=True):
    """The structure of the clumps, in the order given; with dup = (i, j) atom j gets atom i's id."""
    xs, ys, zs, rs, want = [], [], [], [], []
    for cell, n, r, f in clumps:
        if n == 0:
            continue
        k = np.arange(n)
        xs.append(2.0 * (cell[0] - 1) + f[0] + k * STEP)
        ys.append(np.full(n, 2.0 * (cell[1] - 1) + f[1]))
        zs.append(np.full(n, 2.0 * (cell[2] - 1) + f[2]))
        rs.append(np.full(n, r))
        want += [cell] * n
    x, y, z, r = (np.concatenate(a).astype(np.float32) for a in (xs, ys, zs, rs))
    ids = np.arange(1, len(x) + 1, dtype=np.uint64)
    if dup is not None:
        i, j = dup
        assert 0 <= i < j
        ids[j] = ids[i]
    st = ti.Structure(x, y, z, r, ids)
    if check:
        _, c3, _ = mm._cells(x, y, z, r, F(PROBE))
        assert np.array_equal(c3, np.array(want)), "a clump is not in the cell it names"
        assert r.max() == F(R)
    return st


def markers(y_cell):
    """Two lone atoms, three cells apart from y_cell - 3 and from each other: with equal ids (build's dup) the structure
    keeps its ids and neither meets the other's fold."""
    return [clump((1, y_cell, 1), 1), clump((1, y_cell + 3, 1), 1)]


@dataclass
class Case:
    name: str
    family: str
    structures: list
    W: int = KEY[0]
    probe: float = PROBE
    n_points: int = KEY[2]
    apw: int = None            # RSASA_ATOMS_PER_WAVE of the pinned run (None: 64, or 16 above 128 points)
    watch: int = 0             # the atom (of structure 0) whose group / figures the case is named for
    expect: dict = field(default_factory=dict)

    def __post_init__(self):
        if self.apw is None:
            self.apw = 16 if self.n_points > 128 else 64
        self.x, self.y, self.z, self.r, self.ids, self.so = ti.pack(self.structures)

    @property
    def key(self):
        return (self.W, float(F(self.probe)), self.n_points)

    @property
    def n(self):
        return len(self.x)

    def model(self, order="asc", apw="case", bounds=False, **switches):
        return mm.launch(self.x, self.y, self.z, self.r, self.so, self.probe, self.n_points, self.W, self.ids,
                         self.apw if apw == "case" else apw, order, bounds, **switches)


# ---- union size ------------------------------------------------------------------------------------------------------

_FY = {-2: 0.0, 0: 1.0, 2: 1.9}   # offsets that keep clumps of neighbouring rows 4.9 A apart or more
_ROWS8 = [(-2, -2), (-2, 0), (-2, 2), (0, -2), (0, 2), (2, -2), (2, 0), (2, 2)]


def _spread(total, k, most=60):
    q, rem = divmod(total, k)
    out = [q + (1 if i < rem else 0) for i in range(k)]
    assert max(out) <= most
    return out


def union_case(U, with_ids, t=4):
    """A single-cell group of t atoms (cell (1, 3, 3)) whose union holds exactly U atoms: eight clumps in the rows two
    cells away, none within reach of another."""
    cl = []
    for (dy, dz), n in zip(_ROWS8, _spread(U - t, 8)):
        cl.append(clump((1, 3 + dy, 3 + dz), n, f=(0.0, _FY[dy], _FY[dz])))
    watch = sum(c[1] for c in cl)
    cl.append(clump((1, 3, 3), t, f=(0.0, 1.0, 1.0)))
    dup = None
    if with_ids:
        cl += markers(8)
        dup = (watch + t, watch + t + 1)
    k = mm.UNION_IDS if with_ids else mm.UNION_NO_IDS
    return Case(f"union_{'ids' if with_ids else 'noids'}_{U}", "union", [build(cl, dup)], watch=watch,
                expect=dict(U=U, n_chunk=(min(U, k) + 63) >> 6, reason="union" if U > k else "", narrowed=0, self0=0))


def narrow_case(cells, with_ids):
    """One atom in each of `cells` (cells 4 .. 7 of one row: one aligned block at shift 2 and 3).  Clumps in the rows around
    cell 4 fill the union of [2, 6]; one at cell 2 and one at cell 7 overfill any wider one.  (4, 5) narrows once,
    (4, 5, 6, 7) twice; a far atom stretches the grid until the shift is 3."""
    k = mm.UNION_IDS if with_ids else mm.UNION_NO_IDS
    per = (k - 46) // 6
    rows6 = [(-2, -2), (-2, 2), (0, -2), (0, 2), (2, -2), (2, 2)]
    cl = [clump((1, 1, 1), 1)]
    for dy, dz in rows6:
        cl.append(clump((4, 3 + dy, 3 + dz), per, f=(0.0, _FY[dy], _FY[dz])))
    cl.append(clump((2, 1, 3), 40, f=(0.0, 0.0, 1.0)))
    cl.append(clump((7, 5, 3), 40, f=(0.0, 1.9, 1.0)))
    watch = sum(c[1] for c in cl)
    for c in cells:
        cl.append(clump((c, 3, 3), 1, f=(0.0, 1.0, 1.0)))
    cl.append(clump((1, 1, 30), 1))
    dup = None
    if with_ids:
        n = sum(c[1] for c in cl)
        cl += markers(9)
        dup = (n, n + 1)
    full = 6 * per + 80 + len(cells)
    # (the narrowed group's union, cells [2, 6]: the clump at cell 7 and the atom there are left out)
    return Case(f"narrow{len(cells) // 2}_{'ids' if with_ids else 'noids'}", "union", [build(cl, dup)], watch=watch,
                expect=dict(U_first=full, U=6 * per + 40 + min(len(cells), 3), narrowed=len(cells) // 2, reason="",
                            shift=3))


def first_chunk_case(glen):
    """Own row: 30 + 29 atoms in the two cells left of a group of glen atoms (self0 = 59); 60 atoms in front put the
    group inside the second block of 64."""
    cl = [clump((1, 1, 1), 60), clump((2, 1, 4), 30), clump((3, 1, 4), 29), clump((4, 1, 4), glen)]
    return Case(f"first_chunk_{59 + glen}", "first_chunk", [build(cl)], watch=119,
                expect=dict(self0=59, glen=glen, reason="first_chunk" if 59 + glen > 64 else ""))


# ---- candidate list --------------------------------------------------------------------------------------------------

_SQUARE = [(1, 1, 1), (1, 2, 1), (1, 1, 2), (1, 2, 2)]


def cluster_case(n):
    """n atoms in four cells around one corner, all within reach of each other: K = n - 1 for every atom."""
    cl = [clump(c, m) for c, m in zip(_SQUARE, _spread(n, 4, most=64))]
    return Case(f"cluster_K{n - 1}", "list", [build(cl)], expect=dict(K=n - 1))


def lone_cap_case():
    """129 atoms of radius 1.0 (cutoff 3.5 A) and one of 1.5 (4.0 A) 3.75 A from all of them: it lists 129, they list 128;
    it shares the group of the first cell (shift 2: a far atom stretches the grid)."""
    cl = [clump(c, m, r=1.0) for c, m in zip(_SQUARE, (33, 32, 32, 32))]
    cl.append(clump((2, 1, 1), 1, f=(1.5, 1.0, 1.0)))
    cl.append(clump((1, 1, 16), 1))
    return Case("lone_K129", "list", [build(cl)], watch=129, expect=dict(K=129, mates=128, shift=2))


def spill_case(with_ids, fifth):
    """Four cells of 64 atoms around one corner (K = 255, four chunks) and, id-less, a fifth clump of 40 two cells on
    (five chunks): the lists run past the buffer and end on the struct's last record."""
    cl = [clump(c, 64) for c in _SQUARE]
    if fifth:
        cl.append(clump((1, 3, 1), 40))
    dup = None
    if with_ids:
        cl += markers(6 if fifth else 5)
        dup = (sum(c[1] for c in cl) - 2, sum(c[1] for c in cl) - 1)
    return Case(f"spill_{'ids' if with_ids else 'noids'}_{5 if fifth else 4}", "list", [build(cl, dup)],
                expect=dict(n_chunk=5 if fifth else 4))


def near_case(nc, nb):
    """Atom 0 alone in its cell, nc atoms 2.0 A away (near: d^2 < 1.8 R^2 = 7.2) and nb atoms 2.83 A away (not near)."""
    cl = [clump((1, 1, 1), 1), clump((1, 2, 1), nc), clump((1, 2, 2), nb)]
    return Case(f"near_{nc}", "list", [build(cl)], expect=dict(K=nc + nb, near=nc))


# ---- group shift -----------------------------------------------------------------------------------------------------

LINE_CELLS = 20


def line(n, dup=False, cells=LINE_CELLS):
    """n atoms spread over `cells` cells of one row; dup: the last atom carries the first one's id (nineteen cells apart)."""
    per = _spread(n, cells, most=64)
    st = build([clump((c + 1, 1, 1), m) for c, m in enumerate(per)], check=n >= cells)
    if dup:
        st.ids[-1] = st.ids[0]
    return st


@functools.lru_cache(maxsize=None)
def line_cells():
    """Cells of line()'s grid (it does not depend on n once every cell is taken)."""
    s = line(LINE_CELLS * 2)
    return int(np.prod(mm._cells(s.x, s.y, s.z, s.r, F(PROBE))[0]))


def shift_thresholds():
    """{name: (n below, n at or above, shift below, shift above, id-less?)} around 0.3, 0.6, 1.0 atoms per cell and the
    id-less 1.95 rule."""
    nc = line_cells()
    out = {}
    for name, thr, lo_s, hi_s in (("0.3", 0.3, 3, 2), ("0.6", 0.6, 2, 1), ("1.0", 1.0, 1, 0)):
        n = int(np.ceil(thr * nc))
        while F(n) / F(nc) < F(thr):
            n += 1
        while F(n - 1) / F(nc) >= F(thr):
            n -= 1
        out[name] = (n - 1, n, lo_s, hi_s)
    n = int(1.95 * nc)
    while F(n) < F(1.95) * F(nc):
        n += 1
    while not F(n - 1) < F(1.95) * F(nc):
        n -= 1
    out["1.95"] = (n - 1, n, 1, 0)
    return out


def shift_cases():
    out = []
    for name, (n_lo, n_hi, s_lo, s_hi) in shift_thresholds().items():
        for n, s in ((n_lo, s_lo), (n_hi, s_hi)):
            if name != "1.95":
                out.append(Case(f"shift_{name}_ids_{n}", "shift", [line(n, dup=True)], expect=dict(shift=s)))
            # (id-less: 0 becomes 1 below 1.95 atoms per cell)
            s_no = s if name == "1.95" else max(s, 1)
            out.append(Case(f"shift_{name}_noids_{n}", "shift", [line(n)], expect=dict(shift=s_no)))
    return out


# ---- blocks ----------------------------------------------------------------------------------------------------------

def block_cases(apw):
    e = ti.Structure.of(np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.uint64))
    sizes = [apw - 3, 7, 0, 2 * apw + 5] + ([apw - 8] if apw > 8 else [])   # 4 apw + 1 atoms; the third one empty
    many = [line(n) if n else e for n in sizes]
    return [Case(f"blocks{apw}_one", "blocks", [line(apw)], apw=apw, expect=dict(n_blocks=1, last=apw)),
            # (six cells for the blocks of 8: five atoms a cell, so that a block's end cuts a cell there as well)
            Case(f"blocks{apw}_four", "blocks", [line(4 * apw, cells=6 if apw == 8 else LINE_CELLS)], apw=apw,
                 expect=dict(n_blocks=4, last=apw)),
            Case(f"blocks{apw}_four_plus_one", "blocks", many, apw=apw, expect=dict(n_blocks=5, last=1))]


# ---- phase B forms and many points -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pair_case(n_points, W, lo_min, hi_max, rem_only=False):
    """Atom 0 (radius 1.0) and one occluder (radius 1.5) at the first distance, in steps of 1 / 64 A, at which the model's
    bounds on atom 0's filter survivors lie inside [lo_min, hi_max].  rem_only: the occluder sits opposite the
    remainder points and leaves only them exposed."""
    sx, sy, sz = ti.sphere(n_points)
    nf = ti.n_fused(n_points, W)
    if rem_only:
        u = -np.array([sx[nf:].sum(), sy[nf:].sum(), sz[nf:].sum()], float)
    else:
        u = np.array([1.0, 1.0, 1.0])
    u /= np.linalg.norm(u)
    for step in range(1, 218):   # (up to 3.4 A: inside atom 0's cutoff of 3.5 A)
        d = step / 64.0
        b = np.round(u * d * 1024.0) / 1024.0
        lo, hi, rem = mm.survivor_bounds((0.0, 0.0, 0.0), 1.5, [(b[0], b[1], b[2], 1.5)], PROBE, n_points, W)
        if lo >= lo_min and hi <= hi_max and (not rem_only or rem >= 1):
            st = ti.Structure.of([(0.0, 0.0, 0.0), tuple(b)], [1.0, 1.5])
            name = f"pair_{n_points}_{W}_{'rem' if rem_only else f'{lo_min}_{hi_max}'}"
            return Case(name, "many" if n_points > 128 else "phase_b", [st], W=W, n_points=n_points,
                        expect=dict(lo=lo, hi=hi, rem=rem))
    raise AssertionError(("no distance gives the survivor count", n_points, W, lo_min, hi_max, rem_only))


@functools.lru_cache(maxsize=None)
def tiles_case(n_points, W, want):
    """As pair_case, at the first distance at which exactly `want` tiles of 16 points outlive the patch test by the
    model's bounds (the filter works through them eight per trip: 8 and 16 fill their trips, 9 and 17 start another)."""
    for step, u in ((s, d) for d in ((1, 1, 1), (1, 0, 0), (0, 0, 1), (1, 2, 3), (0, 1, 0), (3, 1, 2))
                    for s in range(100, 870)):   # (steps of 1 / 256 A along a few directions)
        b = np.round(np.array(u) / np.linalg.norm(u) * (step / 256.0) * 1024.0) / 1024.0
        lo, hi, _ = mm.live_tile_bounds((0.0, 0.0, 0.0), 1.5, [(b[0], b[1], b[2], 1.5)], PROBE, n_points, W)
        if lo == hi == want:
            st = ti.Structure.of([(0.0, 0.0, 0.0), tuple(b)], [1.0, 1.5])
            return Case(f"tiles_{n_points}_{W}_{want}", "many", [st], W=W, n_points=n_points, expect=dict(tiles=want))
    raise AssertionError(("no distance gives the live tiles", n_points, W, want))


PHASE_B_POINTS = ((96, 8), (100, 8), (100, 16), (112, 16), (128, 8))
PHASE_B_RANGES = ((0, 0), (1, 4), (5, 8), (9, 1 << 20))
MANY_POINTS = ((129, 8), (144, 16), (1024, 8), (1025, 16), (1040, 16), (1344, 8))
MANY_RANGES = ((1, 63), (65, 128), (193, 1 << 20))
# atoms of the many-point batches: with 16 atoms per wave and 4 waves per workgroup (129 and 144 points) 200 atoms are 4
# workgroups - a piece each -, 512 exactly eight, 513 nine with 33 wave blocks in pieces of 5 - the seventh has 3, the last
# none; with 12 waves (1024 points and more: launch_occlusion's choice, which depends on the kernel's LDS size and is not
# pinned here) 1536 are eight workgroups and 1552 nine
MANY_SIZES = (200, 512, 513, 1536, 1552)
SEG_OFFSETS = (1984, 2048, 2016)


def phase_b_cases():
    out = [pair_case(n, W, a, b) for n, W in PHASE_B_POINTS for a, b in PHASE_B_RANGES]
    out += [pair_case(100, 8, 0, 0, True), pair_case(100, 16, 0, 0, True)]
    return out


def many_point_cases():
    out = [pair_case(n, W, a, b) for n, W in MANY_POINTS for a, b in MANY_RANGES if a < n]
    return out + [tiles_case(n, W, t) for n, W in ((1024, 8), (1025, 16), (1344, 8)) for t in (8, 9, 16, 17)]


def many_point_batch(n_points, W, n_atoms):
    """The (n_points, W) pairs and lines of 40 atoms, cut to exactly n_atoms atoms: 16 atoms per wave make n_atoms / 16
    wave blocks, 4, 8 or 12 of them a workgroup."""
    sts = [c.structures[0] for c in many_point_cases() if (c.n_points, c.W) == (n_points, W)]
    if n_atoms >= 1536:   # (lists of 127 and 129 candidates and a union of 320 among them)
        sts += [cluster_case(128).structures[0], cluster_case(130).structures[0], union_case(320, False).structures[0]]
    left = n_atoms - sum(s.n for s in sts)
    while left > 0:
        sts.append(line(min(left, 40)))
        left -= sts[-1].n
    return Case(f"many_{n_points}_{W}_{n_atoms}", "many", sts, W=W, n_points=n_points)


# ---- ids -------------------------------------------------------------------------------------------------------------

def fold_case(same_union):
    """Atoms 0 and 2 carry different ids with one 32-bit fold, 4.5 A apart in one union (same_union) or three rows apart;
    atom 1 is atom 0's neighbour; the two markers share an id, so the structure keeps its ids."""
    a = 0x1234_5678_9ABC
    b = ti.colliding_id(a, 5000)
    assert b > a and ti.fold_id(a) == ti.fold_id(b)
    far = clump((3, 1, 1), 1, f=(0.5, 0.0, 0.0)) if same_union else clump((1, 4, 1), 1)
    st = build([clump((1, 1, 1), 2, f=(0.0, 0.0, 0.0)), far] + markers(4 if same_union else 7))
    st.x[1] = F(2.0)   # (the neighbour: 2.0 A from atom 0, in cell 2)
    st.ids[:] = np.array([a, a + 1, b, b + 1, b + 1], np.uint64)
    return Case(f"fold_{'same' if same_union else 'other'}_union", "ids", [st],
                expect=dict(deferred=[0, 2] if same_union else []))


def seg_case(offset):
    """A structure of 64 atoms that keeps its ids at cell-sorted positions [offset, offset + 64): 1984 fills bit 31 of
    the bitmaps' first word, 2048 bit 0 of the second, 2016 straddles the two.  Lines of 200 atoms with rising ids in front
    of it and behind."""
    sts = []
    left = offset
    while left > 0:
        sts.append(line(min(left, 200)))
        left -= sts[-1].n
    keep = build([clump(c, 16) for c in _SQUARE])
    keep.ids[40] = keep.ids[3]   # (cells two apart: one union, so both meet the other's fold)
    sts += [keep, line(200), line(57)]
    return Case(f"ids_seg_{offset}", "ids_seg", sts, apw=0, expect=dict(first=offset))


# ---- admission -------------------------------------------------------------------------------------------------------

def range_cases():
    """What sends every group of a structure to the general kernel whatever its size: a radius above 64 anywhere in it
    (StructGrid::odd_radii), a grid of more than 1024 cells along an axis (1024 is taken)."""
    def ends(x_max):
        return ti.Structure.of([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (x_max - 1.0, 0.0, 0.0), (x_max, 0.0, 0.0)], [R] * 4)
    big = ti.Structure.of([(0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (70.0, 0.0, 0.0)], [R, R, 64.5])
    return [Case("range_radius_64.5", "range", [big], expect=dict(deferred=3)),
            Case("range_dim_1024", "range", [ends(2042.0)], expect=dict(deferred=0, dim_x=1024)),
            Case("range_dim_1025", "range", [ends(2044.0)], expect=dict(deferred=4, dim_x=1025))]


# ---- all of them -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    for U in (40, 100, 150, 230, 300, 320, 321):
        out.append(union_case(U, False))
    for U in (40, 100, 150, 256, 257):
        out.append(union_case(U, True))
    for ids in (False, True):
        out += [narrow_case((4, 5), ids), narrow_case((4, 5, 6, 7), ids)]
    out += [first_chunk_case(5), first_chunk_case(6)]
    out += [cluster_case(n) for n in (17, 18, 65, 66, 113, 114, 128, 129, 130)]
    out += [lone_cap_case(), spill_case(False, False), spill_case(False, True), spill_case(True, False)]
    out += [near_case(nc, nb) for nc, nb in ((0, 20), (15, 10), (16, 10), (17, 10), (64, 10))]
    out += shift_cases()
    for apw in (8, 23, 64):
        out += block_cases(apw)
    out += phase_b_cases()
    out += many_point_cases()
    out += [fold_case(True), fold_case(False)]
    out += range_cases()
    # the list's and the union's limits once more with 6, 7 and 8 tiles of points and 16 lanes
    for W, n_points in ((8, 96), (16, 100), (16, 112), (8, 128)):
        for c in [o for o in out if o.name in OTHER_KEYS]:
            out.append(Case(f"{c.name}_{n_points}_{W}", c.family, c.structures, W=W, n_points=n_points, watch=c.watch,
                            expect=c.expect))
    return out


OTHER_KEYS = ("cluster_K65", "cluster_K127", "cluster_K128", "cluster_K129", "lone_K129", "spill_noids_5", "union_noids_320",
              "union_noids_321", "union_ids_256", "union_ids_257", "first_chunk_64", "first_chunk_65", "near_16")


def by_name(name):
    return next(c for c in all_cases() if c.name == name)


def packed(key, reverse=False, families=None):
    """The structures of every case with this (W, probe, n_points), one batch (reverse: in the opposite order)."""
    sts = [s for c in all_cases() if c.key == key and (families is None or c.family in families) for s in c.structures]
    if reverse:
        sts = sts[::-1]
    return Case(f"packed_{key}{'_rev' if reverse else ''}", "packed", sts, W=key[0], probe=key[1], n_points=key[2])


def keys():
    return sorted({c.key for c in all_cases()})


def report():
    """One line per case: the model's figures for the watched atom and its group (from the repository root: PYTHONPATH=. python tests/mx_cases.py)."""
    lines = []
    for c in all_cases():
        m = c.model(bounds=True)
        g = m.groups[m.group_of[c.watch]]
        w = c.watch
        lines.append(f"{c.name}: atoms {c.n} W {c.W} points {c.n_points} apw {m.apw} blocks {len(m.blocks)} shift "
                     f"{m.structs[0].shift} ids {int(m.structs[0].has_ids)} | group len {g.g1 - g.g0} U {g.U_first}->{g.U} "
                     f"narrowed {g.narrowed} chunks {g.n_chunk} self0 {g.self0} {g.reason or 'taken'} | K {m.K[w]} near "
                     f"{m.near[w]} survivors [{m.lo[w]}, {m.hi[w]}] | deferred {m.n_deferred}")
    return lines


if __name__ == "__main__":
    print("\n".join(report()))
