"""Inputs that sit on the structural limits of k_occlusion_fast and k_occlusion_v3, each named for its edge; the figures
come from pa_model.py (test_pa_cases_cpu.py pins them, test_gpu_pa_edges.py runs them).

Geometry (as mx_cases.py): probe 0.5 and largest radius 1.5 make the cell 2.0 (reciprocal 0.5, exact) and the cutoff of
a 1.5 A atom 4.0 A = two cells.  Atom 0 (the anchor) sits at the origin and puts the grid's minimum at -2; atom 1 (the
TARGET, `watch`) sits at the centre of cell (5, 5, 5), alone in its cell, so that its row culling is far from every
rounding: the rows two cells off diagonally are dropped by 0.5 of thr, the others keep whole cells with 0.17 cells to
spare.  Partners are CLUMPS: n atoms of one kind in one cell, 2^-12 A apart along x - atoms overlap freely, only the
arithmetic matters.  A clump is named by its cell's offset from the target's:

  NEAR   the 6 face neighbours, 2.0 A away: accepted and near (d^2 < 1.5625 R^2 = 6.25)
  FAR    the 12 edge and 8 corner neighbours, 2.83 / 3.46 A away: accepted, not near
  SWEPT  54 cells on the outside of the swept block, the clump 4.9 A away: swept but not accepted, which makes T and K
         independent of each other

Every atom of a clump gives the same answer to the target's tests and the target is alone in its cell, so nothing a
case is named for depends on the order of the atoms inside a cell (the CPU test checks it with three orders).

What cannot be built: 25 non-empty runs.  A row two cells off in y AND z needs gy^2 + gz^2 <= thr = 4.00004 with sr at
its largest (two cells).  For two OPPOSITE corner rows the four squared gaps are (2 - uy)^2 + (1 + uy)^2 and the same in
uz, at least 4.5 each, 9 together - more than 2 thr - so one of each opposite pair is always dropped and 23 rows are the
most: `swept_rows23` has them (the target at u = (0.5, 0.7, 0.5) reaches both rows two cells up in y), `swept_rows21`
every row a centred target reaches.  The anchor has radius 1.0: the atom on the grid's lowest faces has u = 0, and
with the largest radius its reach would end exactly on cell faces.  Both id layouts of k_occlusion_v3 are reachable:
a batch the per-atom kernels take keeps a cell-sorted copy of the 64-bit ids; the list-mode launch behind
k_occlusion_mx (test_packed_key_past_the_matrix_core_threshold) reads the caller's ids through sorted_orig.
Plain helper module (not a conftest)."""
import functools
from dataclasses import dataclass, field

import numpy as np

import pa_model as pm
import tie_cases as ti

F = np.float32
PROBE = 0.5
R = 1.5
STEP = 2.0 ** -12
TC = (5, 5, 5)
KEY = (8, PROBE, 100)

NEAR = [(0, 0, -1), (0, -1, 0), (-1, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)]
FAR = [(a, b, c) for c in (-1, 0, 1) for b in (-1, 0, 1) for a in (-1, 0, 1) if abs(a) + abs(b) + abs(c) >= 2]
MID = (1.0, 1.0, 1.0)


def _edge(d):
    return 1.9 if d > 0 else 0.1


# (cell offset, position inside the cell) of the swept-only slots: the far x cells of the nine inner rows, and the
# three cells of the twelve rows two cells off in y or z
SWEPT = [((sx, b, c), (_edge(sx), 1.0, 1.0)) for sx in (-2, 2) for b in (-1, 0, 1) for c in (-1, 0, 1)]
SWEPT += [((a, sy, c), (1.0, _edge(sy), 1.0)) for sy in (-2, 2) for a in (-1, 0, 1) for c in (-1, 0, 1)]
SWEPT += [((a, b, sz), (1.0, 1.0, _edge(sz))) for sz in (-2, 2) for a in (-1, 0, 1) for b in (-1, 0, 1)]
ROW1 = [((a, -1, -2), (1.0, 1.0, 0.1)) for a in (-1, 0, 1)]       # run 1, the first a centred target sweeps
PRE = [s for s in SWEPT if (s[0][2] + 2) * 5 + s[0][1] + 2 < 12]   # the 26 swept-only slots of the runs before the own row
LAST = [((a, b, 2), (1.0, 1.0, 1.9)) for b in (-1, 0, 1) for a in (-1, 0, 1)]   # runs 21 - 23, the last ones
BEFORE = [o for o in FAR if o[2] == -1] + [(0, 0, -1)] + [(-1, -1, 0), (0, -1, 0), (1, -1, 0)]   # runs 6 - 8 and 11


def row_of(off):
    return (off[2] + 2) * 5 + off[1] + 2


def spread(total, k):
    q, rem = divmod(total, k)
    return [q + (1 if i < rem else 0) for i in range(k)]


def over(slots, total, f=MID, r=R):
    """`total` atoms of radius r spread evenly over the slots (cell offsets, or (offset, position) pairs)."""
    out = []
    for s, n in zip(slots, spread(total, len(slots))):
        off, pos = s if isinstance(s[0], tuple) else (s, f)
        if n:
            out.append((off, n, pos, r))
    return out


def build(clumps, dup=(), target_f=MID):
    """anchor (radius 1.0), target (at target_f inside its cell), then the clumps (offset, n, position, radius) in the
    order given.  dup: indices (counted over the clumps' atoms) that carry the target's id."""
    xs, ys, zs, rs = [0.0, 2.0 * (TC[0] - 1) + target_f[0]], [0.0, 2.0 * (TC[1] - 1) + target_f[1]], \
        [0.0, 2.0 * (TC[2] - 1) + target_f[2]], [1.0, R]
    want = [(1, 1, 1), TC]
    for off, n, f, r in clumps:
        cell = tuple(TC[k] + off[k] for k in range(3))
        for k in range(n):
            xs.append(2.0 * (cell[0] - 1) + f[0] + k * STEP)
            ys.append(2.0 * (cell[1] - 1) + f[1])
            zs.append(2.0 * (cell[2] - 1) + f[2])
            rs.append(r)
        want += [cell] * n
    idv = np.arange(1, len(xs) + 1, dtype=np.uint64)
    for j in dup:
        idv[2 + j] = idv[1]
    st = ti.Structure.of(np.stack([xs, ys, zs], -1), rs, idv)
    m = pm.launch(st.x, st.y, st.z, st.r, [0, st.n], PROBE, 100, 8)
    assert np.array_equal(m.cxyz, np.array(want)), "a clump is not in the cell it names"
    return st


def line(n):
    """n atoms along x, filler whose atoms have a handful of candidates each: a corner atom of radius 1.0 at the origin -
    the atom on the grid's lowest faces must not have the largest radius, or its reach ends exactly on cell faces - and
    the others (radius 1.5) three to a cell, 0.7 A up in y and z, off every cell face."""
    xs = [0.0] + [2.0 * (k // 3) + (0.3, 0.8, 1.3)[k % 3] for k in range(max(n - 1, 0))]
    xs = np.array(xs[:n])
    yz = np.where(np.arange(n) == 0, 0.0, 0.7)
    return ti.Structure.of(np.stack([xs, yz, yz], -1), np.where(np.arange(n) == 0, 1.0, R))


EMPTY = ti.Structure.of(np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.uint64))


@dataclass
class Case:
    name: str
    family: str
    structures: list
    kernel: str = "fast"         # "fast": no kernel forced; "v3": RSASA_OCCLUSION_KERNEL=3 up to 128 points, default above
    W: int = KEY[0]
    probe: float = PROBE
    n_points: int = KEY[2]
    apw: int = None              # RSASA_ATOMS_PER_WAVE of the run (None: the launch's own)
    watch: int = 1
    expect: dict = field(default_factory=dict)

    def __post_init__(self):
        self.x, self.y, self.z, self.r, self.ids, self.so = ti.pack(self.structures)

    @property
    def key(self):
        return (self.W, float(F(self.probe)), self.n_points)

    @property
    def n(self):
        return len(self.x)

    @property
    def forced(self):
        """RSASA_OCCLUSION_KERNEL of the run, or None."""
        if self.kernel == "fast":
            return None
        n_rem = self.n_points - ti.n_fused(self.n_points, self.W)
        return None if self.n_points > 128 or n_rem > pm.FAST_MAX_REM else "3"

    def model(self, order="asc", apw="case", kernel="case", **kw):
        return pm.launch(self.x, self.y, self.z, self.r, self.so, self.probe, self.n_points, self.W, self.ids,
                         self.forced if kernel == "case" else kernel, self.apw if apw == "case" else apw, order, **kw)


def at(c, n_points, W, kernel=None, tag=None):
    """The case at another point count and lane count."""
    return Case(f"{c.name}_{tag or f'{n_points}_{W}'}", c.family, c.structures, kernel or c.kernel, W, c.probe, n_points,
                c.apw, c.watch, c.expect)


# ---- k_occlusion_fast -------------------------------------------------------------------------------------------------

def swept_case(T):
    """T swept atoms, 8 of them accepted (one per corner cell); T = 1: the target alone in its block."""
    if T == 1:
        return Case("swept_T1", "swept", [build([])], expect=dict(T=1, K=0, deferred=False, runs=1))
    cl = over([o for o in FAR if abs(o[0]) + abs(o[1]) + abs(o[2]) == 3], 8) + over(SWEPT, T - 9)
    return Case(f"swept_T{T}", "swept", [build(cl)], expect=dict(T=T, K=8, deferred=T > 256))


def run_at_case(p):
    """p swept-only atoms in the runs before the target's own row, whose run then starts at flat position p (p = 255:
    the target is the 256th swept atom and the last)."""
    cl = over(PRE, p) + ([] if p == 255 else over(NEAR[3:], 3) + over(LAST, 5))
    return Case(f"swept_run_at_{p}", "swept", [build(cl)], expect=dict(run_at=p, deferred=False))


def rows21_case():
    cl = []
    for c in range(-2, 3):
        for b in range(-2, 3):
            if abs(b) == 2 and abs(c) == 2 or (b, c) == (0, 0):
                continue
            f = (1.0, _edge(b) if abs(b) == 2 else 1.0, _edge(c) if abs(c) == 2 else 1.0)
            cl.append(((0, b, c), 1, f, R))
    cl.append(((1, 0, 0), 1, MID, R))
    return Case("swept_rows21", "swept", [build(cl)], expect=dict(runs=21, T=22, deferred=False))


def rows23_case():
    """The most rows a target can reach: at u = (0.5, 0.7, 0.5) both rows two cells up in y and two off in z are swept
    (gaps 1.3 and 1.5: 3.94 <= thr), the two opposite ones are not (1.7 and 1.5).  One atom in the middle cell of each."""
    cl = [((0, b, c), 1, MID, R) for c in range(-2, 3) for b in range(-2, 3)
          if (b, c) != (0, 0) and not (b == -2 and abs(c) == 2)]
    cl.append(((1, 0, 0), 1, MID, R))
    return Case("swept_rows23", "swept", [build(cl, target_f=(1.0, 1.4, 1.0))], expect=dict(runs=23, T=24, deferred=False))


def list_case(K, n_near=6):
    """K accepted atoms (up to six of them near, one per face cell) and 20 swept-only ones."""
    nn = min(K, n_near)
    cl = over(NEAR, nn) + over(FAR, K - nn) + over(SWEPT[:20], 20)
    return Case(f"list_K{K}", "list", [build(cl)], expect=dict(K=K, T=K + 21, deferred=K > 144))


def list_ids_case(with_ids):
    """150 atoms in reach; the six near ones, each alone in its cell, carry the target's id or do not."""
    cl = over(NEAR, 6) + over(FAR, 144)
    c = Case(f"list_150_{'ids' if with_ids else 'noids'}", "list", [build(cl, dup=range(6) if with_ids else ())],
             expect=dict(K=144 if with_ids else 150, A=150, deferred=not with_ids))
    return c


def near_case(nA, n_far, tag=""):
    cl = over(NEAR, nA) + over(FAR, n_far)
    K = nA + n_far
    nA4 = min(K, (nA + 3) & ~3)
    return Case(f"near_nA{nA}_far{n_far}{tag}", "near", [build(cl)], expect=dict(K=K, nA=nA, nA4=nA4, nB=K - nA4))


@functools.lru_cache(maxsize=None)
def near_tile_case(nB, G):
    """nA a multiple of 4 (phase B starts right behind the near candidates), nB far candidates and so many survivors
    that phase B tiles the lanes with G candidate groups: the first of a fixed list of near layouts and radii for which
    the model says so.  Its last trip reads kTileSteps * G records from slot nA + (steps - 1) * G on: into the padding."""
    lo, hi = (1, 8) if G == 8 else (33, 64)
    for nA in (8, 4, 12):
        for k in (6, 2, 3, 4, 5, 1):
            for rn in (1.5, 1.4, 1.3, 1.2, 1.1, 1.0, 0.9, 0.8, 0.7):
                st = build(over(NEAR[:k], nA, r=rn) + over(FAR, nB))
                f = pm.launch(st.x, st.y, st.z, st.r, [0, st.n], PROBE, 100, 8).fast(1)
                if f["nA"] == nA and f["nB"] == nB and lo <= f["S"] <= hi:
                    return Case(f"near_tiles_nB{nB}_G{G}", "near", [st],
                                expect=dict(K=nA + nB, nA=nA, nA4=nA, nB=nB, G=G))
    raise AssertionError(("no layout gives the tiling", nB, G))


def far_only():
    return Case("far_only", "survivors", [build(over(FAR, 20))], expect=dict(K=20, nA=0))


@functools.lru_cache(maxsize=None)
def second_chunk_case(n_points):
    """65 points (HALF1) and 97 (two full halves), W = 1: four near candidates on such sides of the target that points of
    the second chunk outlive phase A and at most 64 points in all - phase B's compact form fetches them by ds_bpermute
    from the second chunk's registers.  The first of the layouts, in a fixed order, for which the model says so."""
    import itertools
    for sub in itertools.combinations(NEAR, 2):
        st = build(over(list(sub), 4) + over(FAR, 12))
        f = pm.launch(st.x, st.y, st.z, st.r, [0, st.n], PROBE, n_points, 1).fast(1)
        if f["form"] == "tiles" and f["S_second"] > 0 and f["nA"] == 4:
            return Case(f"second_chunk_{n_points}", "survivors", [st], W=1, n_points=n_points,
                        expect=dict(K=16, nA=4, nB=12, second=True))
    raise AssertionError(("no layout leaves a survivor in the second chunk", n_points))


def mixed():
    return Case("mixed", "points", [build(over(NEAR[:4], 4) + over(FAR, 20) + over(SWEPT[:10], 10))],
                expect=dict(K=24, nA=4))


def lonely():
    return Case("lonely", "points", [build(over(SWEPT, 20))], expect=dict(K=0, T=21))


def buried():
    return Case("buried", "points", [build(over(NEAR, 60) + over(FAR, 40))], expect=dict(K=100, nA=None, exposed=0))


SURVIVOR_POINTS = (8, 9, 16, 17, 32, 33, 64, 65)
POINTS = ((64, 1), (65, 1), (96, 8), (97, 1), (100, 8), (104, 8), (128, 8), (100, 16), (127, 4), (98, 8), (65, 8))
POINTS_REM = ((100, 8), (100, 16), (127, 4), (98, 8), (65, 8))


def fast_wave_batches():
    """{forced atoms per wave: [cases]}: 4 apw k - 1, 4 apw k and 4 apw k + 1 atoms (apw as the launch caps and rounds
    it) for k = 1, 2, with a structure boundary and an empty structure inside a group of 10, and a target with 145
    candidates (the batch's deferred atom) first, in the middle and last of its group of 10."""
    out = {}
    dense = list_case(145).structures[0]
    p_t = int(pm.launch(dense.x, dense.y, dense.z, dense.r, [0, dense.n], PROBE, 100, 8).pos[1])
    for forced in (1, 3, 10, 11, 25, 40, 64):
        apw = pm.launch_apw(1000, True, forced)
        cases = []
        for k in (1, 2):
            for d in (-1, 0, 1):
                n = 4 * apw * k + d
                # (no structure of one atom: alone it has the largest radius on the lowest faces, its reach ends on cell faces)
                sts = [line(2), EMPTY, line(n - 2)] if n >= 4 else [line(n), EMPTY]
                cases.append(Case(f"waves{forced}_{n}", "waves", sts, apw=forced, watch=0, expect=dict(n=n, apw=apw)))
        for where in (0, 5, 9):
            lead = (where - p_t) % 10 + 10
            sts = [line(lead - 4), EMPTY, line(4), dense, line(13)]
            cases.append(Case(f"waves{forced}_deferred_at_{where}", "waves", sts, apw=forced, watch=lead + 1,
                              expect=dict(where=where, apw=apw)))
        out[forced] = cases
    return out


def block_count_cases():
    """n_blocks = 7, 8, 9, 16 and 17 at the launch's own one atom per wave: the XCD remap's per = 0, 1, 1, 2, 2."""
    return [Case(f"waves_blocks{nb}", "waves", [line(4 * nb - 2 - 1), line(2)], watch=0,
                 expect=dict(n_blocks=nb, per=nb // 8, apw=1)) for nb in (7, 8, 9, 16, 17)]


# ---- k_occlusion_v3 ---------------------------------------------------------------------------------------------------

def v3(name, family, clumps, expect, **kw):
    return Case(name, family, [build(clumps, **kw)], kernel="v3", expect=expect)


def flush_cases():
    out = [v3("flush_A128_one", "flush", over(BEFORE, 128) + over(LAST, 30), dict(flushes=[128])),
           v3("flush_A129_last_step", "flush", over(NEAR + FAR, 129), dict(flushes=[129])),
           v3("flush_A129_then_nothing", "flush", over(BEFORE, 129) + over(LAST, 100), dict(flushes=[129, 0])),
           v3("flush_192_exactly", "flush", over(BEFORE, 192) + over([(1, 0, 0), (0, 1, 0), (0, 0, 1)], 10) + over(LAST, 40),
              dict(flushes=[192, 10], mid_window=True)),
           v3("flush_three", "flush", over(BEFORE, 192) + over([(1, 0, 0), (0, 1, 0)], 192) + over([(0, 0, 1)], 16),
              dict(n_flushes=3))]
    return out


def window_cases():
    out = [v3(f"windows_T{T}", "windows", over(NEAR, 6) + over(SWEPT, T - 7), dict(T=T, windows=-(-T // 256)))
           for T in (256, 257, 512, 513)]
    out += [v3(f"windows_run_at_{p}", "windows", over(PRE, p) + over(NEAR[3:], 3) + over(LAST, 5), dict(run_at=p))
            for p in (255, 256, 257)]
    out.append(v3("windows_run_straddles_256", "windows", over(ROW1, 200) + over(BEFORE[:3], 100) + over(NEAR, 6),
                  dict(straddle=1)))
    out.append(v3("windows_no_run_starts", "windows", over(ROW1, 100) + over(BEFORE[:3], 600) + over(NEAR, 6),
                  dict(empty_window=1)))
    return out


def _one_flush():
    return over(NEAR[:4], 4) + over(FAR, 20) + over(SWEPT[:10], 10)


def _several_open():
    """Two flushes; the first holds only atoms below and beside the target: half the sphere stays open."""
    return over(BEFORE, 192) + over([(1, 0, 0), (0, 1, 0), (0, 0, 1)], 10) + over(LAST, 40)


def _several_buried():
    """Two flushes; the first holds near atoms on all six sides (the list passes 128 only in run 18): buried by it."""
    return over(NEAR, 60) + over(FAR[:12], 24) + over([(0, 1, 1)], 200)


GROUP_POINTS = (129, 256, 257, 960)


def group_cases():
    out = []
    for n in GROUP_POINTS:
        out.append(at(v3("groups_one_flush", "groups", _one_flush(), dict(single=True)), n, 8))
        out.append(at(v3("groups_several_open", "groups", _several_open(), dict(single=False, done=False)), n, 8))
        out.append(at(v3("groups_several_buried", "groups", _several_buried(), dict(single=False, done=True)), n, 8))
    # (the done exit below 128 points as well: one group)
    out.append(v3("groups_several_buried_100", "groups", _several_buried(), dict(single=False, done=True)))
    out.append(v3("groups_several_open_100", "groups", _several_open(), dict(single=False, done=False)))
    return out


REM_POINTS = {1: 97, 4: 100, 5: 101, 8: 104, 9: 105, 15: 111}   # n_rem -> n_points at W = 16


def remainder_cases():
    out = []
    for n_rem, n_points in REM_POINTS.items():
        shift, groups = pm.rem_tiling(n_rem)
        for K, cl in ((1, over(NEAR[:1], 1)), (groups, over(NEAR + FAR, groups)),
                      (192, over(BEFORE, 132) + over([(1, 0, 0), (0, 1, 0), (0, 0, 1)], 60))):
            c = v3(f"rem{n_rem}_K{K}", "remainder", cl + over(SWEPT[:6], 6),
                   dict(K=K, rem_shift=shift, rem_groups=groups, n_flushes=2 if K == 192 else 1))
            out.append(at(c, n_points, 16, tag=f"{n_points}"))
    return out


def id_cases():
    base = over(NEAR[:3], 3) + over(FAR[:6], 6)
    return [v3("ids_dup_near", "ids", base, dict(K=8, A=9, id_hit=True), dup=[0]),
            v3("ids_dup_far", "ids", base, dict(K=8, A=9, id_hit=True), dup=[5]),
            v3("ids_dup_only", "ids", over(NEAR[:1], 1), dict(K=0, A=1, id_hit=True), dup=[0])]


def v3_wave_batches():
    out = {}
    small = v3("x", "x", _one_flush(), {}).structures[0]
    for forced in (1, 7, 8, 9):
        apw = pm.launch_apw(1000, False, forced)
        cases = []
        for d in (-1, 0, 1):
            n = max(4 * apw + d, small.n + 2)
            n = 4 * apw * (-(-n // (4 * apw))) + d
            a = 3 if n - 2 - small.n == 1 else 2   # (no structure of one atom, see fast_wave_batches)
            rest = n - a - small.n
            sts = [line(a), EMPTY, small] + ([line(rest)] if rest else [])
            cases.append(Case(f"v3waves{forced}_{n}", "v3waves", sts, kernel="v3", apw=forced, watch=a + 1,
                              expect=dict(n=n, apw=apw)))
        out[forced] = cases
    return out


# ---- both kernels: reach ----------------------------------------------------------------------------------------------

REACH_CELLS = (256, 1024, 4000)


@functools.lru_cache(maxsize=None)
def reach_cases():
    """tie_cases' cutoff and cellface structures (100 points, 8 lanes), each with one anchor atom that makes the grid
    about 256, 1 024 and 4 000 cells long along one axis, the pair at its low end and at its high end.  The anchor has
    the structure's smallest radius and is far out of reach: the pair's arithmetic does not change, tol grows to 4e-3
    cells and fx carries the rounding of a long grid.  (structures, flips): flips lists the pairs of structure indices
    across which the oracle's K of atom `atom` must still change."""
    fam = ti.generate()["cutoff"]
    cut = [c for c in fam if c.family == "cutoff"][:6]
    face = [c for c in fam if c.family == "cellface"][:6]
    out = []
    for c in cut + face:
        for cells in REACH_CELLS:
            for axis in range(3):
                for end in (1, -1):
                    sts = []
                    for st in c.structures:
                        cell = float(F(c.probe) + st.r.max())
                        a = np.array([st.x[0], st.y[0], st.z[0]], np.float64)
                        a[axis] += end * cells * cell
                        sts.append(ti.Structure.of(
                            np.concatenate([np.stack([st.x, st.y, st.z], -1), a[None, :]]),
                            np.concatenate([st.r, [st.r.min()]]),
                            np.concatenate([st.ids, [st.ids.max() + 1]])))
                    out.append(Case(f"reach_{c.family}{len(out)}_{cells}_{'xyz'[axis]}_{'low' if end > 0 else 'high'}",
                                    "reach", sts, kernel="both", probe=c.probe, watch=c.atom,
                                    expect=dict(cells=cells, axis=axis, flip=c.family == "cutoff")))
    return out


# ---- all of them ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def all_cases():
    """Every case that runs alone (the wave batches and the reach cases have functions of their own)."""
    out = [swept_case(T) for T in (1, 64, 65, 128, 129, 192, 193, 255, 256, 257)]
    out += [run_at_case(p) for p in (31, 32, 33, 63, 64, 65, 255)] + [rows21_case(), rows23_case()]
    out += [list_case(K) for K in (0, 63, 64, 65, 128, 129, 143, 144, 145)]
    out += [list_ids_case(True), list_ids_case(False)]
    out += [near_case(nA, 20) for nA in (0, 1, 3, 4, 5)] + [near_case(64, 0), near_case(5, 0)]
    out += [near_tile_case(nB, G) for nB in (1, 9) for G in (8, 1)]
    out += [at(far_only(), n, 1) for n in SURVIVOR_POINTS] + [second_chunk_case(65), second_chunk_case(97)]
    out += [at(mixed(), n, W) for n, W in POINTS]
    out += [at(c, n, W) for n, W in POINTS_REM for c in (lonely(), buried())]
    # the list's and the sweep's limits once more with remainder points, with HALF1 and with one chunk
    for n, W in ((100, 16), (96, 8), (64, 1), (128, 8)):
        out += [at(c, n, W) for c in (swept_case(256), swept_case(257), list_case(144), list_case(145))]
    out += flush_cases() + window_cases() + group_cases() + remainder_cases() + id_cases()
    return out


MINIMUM = {"swept": 19, "list": 11, "near": 11, "survivors": 10, "points": 21, "flush": 5, "windows": 9, "groups": 14,
           "remainder": 18, "ids": 3}


def by_name(name):
    return next(c for c in all_cases() if c.name == name)


def keys(kernel=None):
    return sorted({c.key for c in all_cases() if kernel is None or c.kernel == kernel})


def packed(key, reverse=False, kernel="fast", families=None, apw=None):
    """The structures of every case of this kernel with this (W, probe, n_points), one batch."""
    sts = [s for c in all_cases() if c.key == key and c.kernel == kernel and (families is None or c.family in families)
           for s in c.structures]
    if reverse:
        sts = sts[::-1]
    return Case(f"packed_{kernel}_{key}{'_rev' if reverse else ''}", "packed", sts, kernel=kernel, W=key[0], probe=key[1],
                n_points=key[2], apw=apw)


def deferring_batch(n_single, n_dense=0):
    """List cases packed together: list_K144 (defers nothing), n_single copies of list_K145 (its target defers, alone)
    and n_dense structures of 146 atoms in the cell beside the target, which all defer with it (147 atoms each)."""
    dense = build(over(NEAR[3:4], 146))
    sts = [list_case(63).structures[0], list_case(144).structures[0]] + [list_case(145).structures[0]] * n_single + \
        [dense] * n_dense
    return Case(f"defers_{n_single}_{n_dense}", "packed", sts)


def report():
    lines = []
    for c in all_cases():
        m = c.model()
        w = c.watch
        extra = f"flushes {m.v3(w)['flushes']}" if c.kernel == "v3" else f"deferred {m.n_deferred}"
        lines.append(f"{c.name}: atoms {c.n} W {c.W} points {c.n_points} T {m.T[w]} K {m.K[w]} {extra}")
    return lines


if __name__ == "__main__":
    print("\n".join(report()))
