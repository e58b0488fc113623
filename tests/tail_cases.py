"""The inputs of the tail-binning edge tests (test_tail_cases_cpu.py, test_gpu_tail_edges.py): structures of 65 536
atoms or more - binned by the batch-wide kernels of kernels.hip (k_zero_cells, k_cell_hist, k_scan_*, k_scatter) - in
grids chosen so that the cell scan runs past one tile per workgroup, and batches with several such structures.

A structure is a set of compact blobs (a jittered lattice, DENSITY atoms / A^3, up to 512 atoms each) spread through a
box whose extent fixes the grid: probe 0.5 and largest radius 1.5 make the cell 2.0 (reciprocal 0.5, exact), and atoms at
0 and at 2 D - 6 on each axis make ceil((L + 4) / 2) + 1 = D cells.  So every atom sits among neighbours - a misplaced
run of a cell's atoms changes lists and values - while the number of cells is an integer chosen in advance.

The module also restates the grid formula (oracle/sasa_oracle.c grid_new), the cell index and the placement arithmetic
of k_grid_scan / k_grid_bases / scan_range in numpy, for the CPU test that pins the cases and for the GPU test's
expected cell counts.  Plain helper module (not a conftest)."""
import functools
from dataclasses import dataclass, field

import numpy as np

PROBE = 0.5
R_MAX = 1.5
CELL = 2.0

SCAN_BLOCKS = 1024     # kScanBlocks: workgroups of the cell scan
TILE = 1024            # entries one workgroup scans per tile (256 threads x uint4)
LDS_MAX_ATOMS = 65536  # kLdsMaxAtoms: structures with fewer atoms are binned in LDS
WINDOW_CELLS = 36864   # kWindowCells
STRUCTS_PER_BLOCK = 256  # structures per workgroup of k_grid_params / k_grid_bases
SEGMENT_ATOMS = 4096   # kSegmentAtoms: atoms per bounds segment

BLOB_SIDE = 8          # lattice sites per axis of a blob: 512 atoms
DENSITY = 0.05         # atoms / A^3, as bench_workloads.synthetic_uniform
JITTER = 0.7           # A, as there (least separation: spacing - 2 * jitter = 1.31 A)
GAP = 4.5              # least distance between two blobs' boxes: above the largest cutoff, 1.5 + 1.5 + 2 * 0.5


def lattice_spacing():
    return (1.0 / DENSITY) ** (1.0 / 3.0)


def blob_extent():
    a = lattice_spacing()
    return (BLOB_SIDE - 1) * a + 2.0 * JITTER


def _blob(n, rng):
    """n <= 512 atoms on distinct sites of the 8^3 lattice, jittered, in [0, blob_extent()]^3; (xyz, site numbers)."""
    a = lattice_spacing()
    site = rng.permutation(BLOB_SIDE ** 3)[:n]
    g = np.stack(np.unravel_index(site, (BLOB_SIDE,) * 3), -1).astype(np.float64)
    xyz = g * a + rng.uniform(0.0, 2.0 * JITTER, size=g.shape)
    return xyz, site


@dataclass
class Structure:
    x: np.ndarray
    y: np.ndarray
    z: np.ndarray
    r: np.ndarray
    dims: tuple            # the intended grid (None: not a boxed structure - its grid is whatever the formula gives)
    blob: np.ndarray       # blob number of every atom (-1: the two atoms that fix the extent)
    site: np.ndarray       # lattice site of every atom within its blob (-1: as above)

    def __len__(self):
        return len(self.x)


def boxed_structure(dims, n_atoms, seed):
    """n_atoms atoms in a grid of exactly dims cells: two atoms (radius 1.5) at 0 and at 2 D - 6, the others in blobs of
    512 (the last one smaller) whose slots are spread evenly over the box from its first corner to its last, in the
    order of the cell index (x fastest, z slowest).  Atom order is shuffled: input order is not cell order."""
    rng = np.random.default_rng(seed)
    ext = np.array([2.0 * d - 6.0 for d in dims])
    size = blob_extent()
    pitch = size + GAP
    n_slots = np.floor((ext - 1.0 - size) / pitch).astype(np.int64) + 1
    assert np.all(n_slots >= 1), (dims, n_slots)
    # stretched: the first slot starts 0.5 A inside the box, the last ends 0.5 A inside its far side
    step = np.where(n_slots > 1, (ext - 1.0 - size) / np.maximum(n_slots - 1, 1), 0.0)
    n_blob_atoms = n_atoms - 2
    n_blobs = -(-n_blob_atoms // BLOB_SIDE ** 3)
    total_slots = int(np.prod(n_slots))
    assert total_slots >= n_blobs, (dims, n_slots, n_blobs)
    chosen = np.unique(np.round(np.linspace(0, total_slots - 1, n_blobs)).astype(np.int64))
    assert len(chosen) == n_blobs
    iz, iy, ix = np.unravel_index(chosen, (n_slots[2], n_slots[1], n_slots[0]))
    origin = 0.5 + np.stack([ix, iy, iz], -1) * step
    parts, blob, site = [np.zeros((1, 3)), ext[None, :]], [np.full(2, -1)], [np.full(2, -1)]
    left = n_blob_atoms
    for k in range(n_blobs):
        n = min(left, BLOB_SIDE ** 3)
        xyz, st = _blob(n, rng)
        parts.append(xyz + origin[k])
        blob.append(np.full(n, k))
        site.append(st)
        left -= n
    xyz = np.round(np.concatenate(parts), 3)
    r = rng.choice(np.array([1.3, 1.4, 1.5], np.float32), size=n_atoms)
    r[:2] = R_MAX
    order = rng.permutation(n_atoms)
    xyz, r = xyz[order].astype(np.float32), r[order].astype(np.float32)
    assert xyz.min() == 0.0 and np.array_equal(xyz.max(0), ext.astype(np.float32)) and r.max() == np.float32(R_MAX)
    return Structure(*(np.ascontiguousarray(xyz[:, k]) for k in range(3)), r, tuple(dims),
                     np.concatenate(blob)[order], np.concatenate(site)[order])


def small_structure(n_atoms, seed, origin=(0.0, 0.0, 0.0)):
    """One blob (or the first n_atoms of one): a structure binned in LDS, its grid not fixed in advance."""
    rng = np.random.default_rng(seed)
    xyz, site = _blob(n_atoms, rng)
    xyz = np.round(xyz + np.asarray(origin), 3).astype(np.float32)
    r = rng.choice(np.array([1.3, 1.4, 1.5], np.float32), size=n_atoms).astype(np.float32)
    return Structure(*(np.ascontiguousarray(xyz[:, k]) for k in range(3)), r, None, np.zeros(n_atoms, np.int64), site)


def empty_structure():
    e = np.zeros(0, np.float32)
    return Structure(e, e, e, e, (1, 1, 1), np.zeros(0, np.int64), np.zeros(0, np.int64))


@dataclass
class Case:
    name: str
    structures: list
    ids: np.ndarray = None
    expect: dict = field(default_factory=dict)   # the scan figures the case is named for (test_tail_cases_cpu.py)

    def __post_init__(self):
        cat = lambda k: np.ascontiguousarray(np.concatenate([getattr(s, k) for s in self.structures]))  # noqa: E731
        self.x, self.y, self.z, self.r = cat("x"), cat("y"), cat("z"), cat("r")
        self.so = np.concatenate([[0], np.cumsum([len(s) for s in self.structures])]).astype(np.uint32)
        if self.ids is None:
            self.ids = np.arange(1, len(self.x) + 1, dtype=np.uint64)   # rising: the id check drops them

    @property
    def cols(self):
        return self.x, self.y, self.z, self.r, self.ids, self.so

    @property
    def n_atoms(self):
        return len(self.x)

    def tails(self):
        return [s for s, st in enumerate(self.structures) if len(st) >= LDS_MAX_ATOMS]


# ---- the arithmetic of the grid and of the tail's placement, restated ------------------------------------------------

F = np.float32


def grid_of(x, y, z, r, probe=PROBE):
    """(min f32[3], inv f32, dims int[3]) as grid_new computes them (f32 throughout); an empty structure has one cell."""
    if len(x) == 0:
        return np.zeros(3, F), F(1.0), np.ones(3, np.int64)
    cell = F(probe) + np.max(r)
    inv = F(1.0) / cell
    mn = np.array([x.min(), y.min(), z.min()], F) - cell
    mx = np.array([x.max(), y.max(), z.max()], F) + cell
    dims = np.ceil((mx - mn) * inv).astype(np.int64) + 1
    assert mn.dtype == F and inv.dtype == F
    return mn, inv, dims


def cell_index(x, y, z, mn, inv, dims):
    c = [np.minimum(((a - mn[k]) * inv).astype(np.int64), dims[k] - 1) for k, a in enumerate((x, y, z))]
    return c[0] + c[1] * dims[0] + c[2] * dims[0] * dims[1]


def lds_cell_slots(n_cells):
    return (n_cells + 1 + 7) & ~7


@dataclass
class Layout:
    dims: list            # per structure
    n_cells: list         # per structure
    n_cells_sum: int      # what the device reports (Timings n_cells): cells of all grids
    cells_s: int          # 16-bit entries of the LDS-binned structures
    tail_cell_begin: int
    tail_atom_base: int
    tail_entries: int     # tail cells + end sentinel
    cell_base: dict       # tail structure -> first entry, relative to tail_cell_begin
    chunk: int
    tiles: int
    active: int           # workgroups whose range is not empty
    mod4: int             # (total_cells + 1) % 4
    occupied: np.ndarray  # sorted entries (relative to tail_cell_begin) of the tail cells that hold atoms


def layout(case):
    dims, n_cells, cells_s, atoms_s, cells_l, base, occ = [], [], 0, 0, 0, {}, []
    for s, st in enumerate(case.structures):
        mn, inv, d = grid_of(st.x, st.y, st.z, st.r)
        nc = int(np.prod(d))
        dims.append(tuple(int(v) for v in d))
        n_cells.append(nc)
        if len(st) < LDS_MAX_ATOMS:
            cells_s += lds_cell_slots(nc)
            atoms_s += len(st)
        else:
            base[s] = cells_l
            occ.append(np.unique(cell_index(st.x, st.y, st.z, mn, inv, d)) + cells_l)
            cells_l += nc
    tail_begin = (cells_s // 2 + 1023) & ~1023
    entries = cells_l + 1
    chunk = -(-entries // SCAN_BLOCKS)
    chunk = (chunk + TILE - 1) & ~(TILE - 1)
    return Layout(dims, n_cells, sum(n_cells), cells_s, tail_begin, atoms_s, entries, base, chunk, chunk // TILE,
                  -(-entries // chunk), (tail_begin + cells_l + 1) % 4,
                  np.concatenate(occ) if occ else np.zeros(0, np.int64))


# ---- the cases -------------------------------------------------------------------------------------------------------

DIMS_2_20 = (41, 75, 341)        # 1 048 575 cells: 2^20 entries with the sentinel
DIMS_2_20_1 = (32, 32, 1024)     # 1 048 576 cells: 2^20 + 1 entries; one z layer is one tile
DIMS_FIVE_TILES = (41, 41, 2977)  # 5 004 337 cells (= 1 mod 4)
# batch (a): cell counts = 1, 1, 0 mod 4, so the second and third cell_base are 1 and 2 mod 4 and the entries 3 mod 4
DIMS_A = ((41, 41, 189), (41, 45, 189), (40, 41, 201))
SIZES_A = (65536, 65537, 70000)


@functools.lru_cache(maxsize=None)
def _tail(k):
    return boxed_structure(DIMS_A[k], SIZES_A[k], seed=100 + k)


@functools.lru_cache(maxsize=None)
def _big():
    return boxed_structure(DIMS_2_20_1, 65536, seed=21)


def case_2_20():
    return Case("2^20", [boxed_structure(DIMS_2_20, 65536, seed=20)],
                expect=dict(entries=1 << 20, chunk=1024, tiles=1, active=1024, mod4=0))


def case_2_20_1():
    return Case("2^20+1", [_big()], expect=dict(entries=(1 << 20) + 1, chunk=2048, tiles=2, active=513, mod4=1))


def case_five_tiles():
    return Case("five_tiles", [boxed_structure(DIMS_FIVE_TILES, 65536, seed=22)],
                expect=dict(entries=5004338, chunk=5120, tiles=5, active=978, mod4=2))


def batch_a():
    n = sum(int(np.prod(d)) for d in DIMS_A)
    return Case("batch_a", [_tail(0), _tail(1), _tail(2)],
                expect=dict(entries=n + 1, chunk=1024, tiles=1, active=-(-(n + 1) // 1024), mod4=3))


N_TINY = 300   # more than the 256 structures of one k_grid_params / k_grid_bases workgroup


def _batch_b_structures():
    tiny = [small_structure(3 + k % 5, seed=1000 + k) for k in range(N_TINY)]
    lds = boxed_structure((40, 40, 72), 20000, seed=30)       # 115 200 cells: four windows
    return [_tail(0)] + tiny[:150] + [lds, empty_structure()] + tiny[150:] + \
        [_tail(1), small_structure(400, seed=31), _tail(2)]


def batch_b(duplicate_ids=False):
    """tail, 150 tiny structures, LDS-binned structure of four windows, empty structure, 150 tiny structures, tail, small
    structure, tail: the second and third tail structures sit in the second workgroup of k_grid_params / k_grid_bases
    (the sums of the first 256 structures reach them through k_grid_scan).  duplicate_ids: in the second tail
    structure the 8 atoms of a lattice column of a blob share an id - lattice neighbours, 2.7 A apart, that then do
    not occlude each other."""
    sts = _batch_b_structures()
    case = Case("batch_b_dup" if duplicate_ids else "batch_b", sts)
    if duplicate_ids:
        s = case.tails()[1]
        b, e = int(case.so[s]), int(case.so[s + 1])
        st = sts[s]
        ids = case.ids.copy()
        dup = st.blob >= 0
        ids[b:e][dup] = (10 ** 9 + st.blob[dup] * (BLOB_SIDE ** 3) + st.site[dup] // BLOB_SIDE).astype(np.uint64)
        case.ids = ids
    n = sum(int(np.prod(d)) for d in DIMS_A)
    case.expect = dict(entries=n + 1, chunk=1024, tiles=1, active=-(-(n + 1) // 1024), mod4=3)
    return case


def batch_c():
    """The 2^20 + 1 structure in front of batch (a): chunks of 2048 entries whose boundaries fall inside every structure,
    and cell bases of 0, 1 and 2 mod 4 behind it."""
    n = sum(int(np.prod(d)) for d in DIMS_A) + int(np.prod(DIMS_2_20_1))
    chunk = ((-(-(n + 1) // 1024)) + 1023) & ~1023
    return Case("batch_c", [_big(), _tail(0), _tail(1), _tail(2)],
                expect=dict(entries=n + 1, chunk=chunk, tiles=chunk // 1024, active=-(-(n + 1) // chunk), mod4=3))


CASES = {"2^20": case_2_20, "2^20+1": case_2_20_1, "five_tiles": case_five_tiles, "batch_a": batch_a,
         "batch_b": batch_b, "batch_b_dup": functools.partial(batch_b, True), "batch_c": batch_c}


@functools.lru_cache(maxsize=None)
def get(name):
    return CASES[name]()


# ---- trajectory ------------------------------------------------------------------------------------------------------

N_FRAMES = 3


def trajectory():
    """(xyz f32[3, N, 3], r, ids, residue offsets, dims of every frame): the 2^20 + 1 structure; in frame f the blobs
    of the last z slot and the atom at the far corner move 20 (f + 1) A outwards along z (the grid gains
    10 (f + 1) layers: past 2^20 cells in every frame) and blob 3 + f moves 1 A along z (half its atoms change cells)."""
    st = _big()
    xyz0 = np.stack([st.x, st.y, st.z], -1).astype(np.float64)
    top = st.z > np.float32(2.0 * DIMS_2_20_1[2] - 6.0 - 1.0 - blob_extent())
    assert (st.blob[top] == -1).sum() == 1 and 500 < top.sum() < 4 * BLOB_SIDE ** 3 + 2
    frames, dims = [], []
    for f in range(N_FRAMES):
        xyz = xyz0.copy()
        xyz[top, 2] += 20.0 * (f + 1)
        xyz[st.blob == 3 + f, 2] += 1.0
        frames.append(np.round(xyz, 3).astype(np.float32))
        dims.append((DIMS_2_20_1[0], DIMS_2_20_1[1], DIMS_2_20_1[2] + 10 * (f + 1)))
    n = len(st)
    res = np.arange(0, n + 1, 8, dtype=np.uint32)
    assert res[-1] == n
    return np.stack(frames), st.r, np.arange(1, n + 1, dtype=np.uint64), res, dims


def trajectory_case():
    """The frames as the batch the engine makes of them (k_expand_frames): one structure per frame."""
    xyz, r, ids, _, dims = trajectory()
    sts = []
    st0 = _big()
    for f in range(N_FRAMES):
        sts.append(Structure(*(np.ascontiguousarray(xyz[f, :, k]) for k in range(3)), r, dims[f], st0.blob, st0.site))
    n = sum(int(np.prod(d)) for d in dims)
    chunk = ((-(-(n + 1) // 1024)) + 1023) & ~1023
    return Case("trajectory", sts, ids=np.tile(ids, N_FRAMES),
                expect=dict(entries=n + 1, chunk=chunk, tiles=chunk // 1024, active=-(-(n + 1) // chunk),
                            mod4=(n + 1) % 4))
