"""The inputs of the LDS-binning edge tests (test_window_cases_cpu.py, test_gpu_window_edges.py): structures of fewer
than 65 536 atoms - binned by k_sort_window (kernels.hip), one workgroup per window of 36 864 cells - chosen so that the
kernel's seams are met by construction and not where a random cloud happens to land on them:

    (a) ladder     structure sizes on both sides of one slot (1 024 atoms), of the record pass's second chunk (4 096), of
                   the registers' share (8 192) and of the rest atoms' trips of 4 096
    (b) windows    grids whose last window has 1, 2, 8, 38 or 36 863 cells, a window without an atom, and a batch in
                   which a grid without padding behind its end marker is followed by other structures
    (c) staging    a second window of 2 303, 2 304 and 2 305 atoms (the LDS stages 2 304 records), and one whose slot atoms
                   and rest atoms both leave through the LDS and by direct stores
    (d) dense      65 535 atoms, more than 40 000 of them in one cell: 16-bit counters, cursors and starts at their top
    (e) single     the sizes and grids of (a) and (b) that one host structure of up to 8 192 atoms can have

Grids are fixed as in tail_cases.py: probe 0.5 and largest radius 1.5 make the cell 2.0, and atoms at 0 and at 2 D - 6 on
an axis make D cells on it; no other atom lies above 2 D - 6.5, so the top layer of every axis is empty in exact
arithmetic and a last window inside the top z layer holds no atom.  Thick grids take the blobs of tail_cases; a grid with
an axis too short for a blob takes a jittered lattice of the same density through the whole box (lattice_structure), and
the ladder's structures are single blocks of a denser lattice (at tail_cases.DENSITY 12 289 atoms fill 30 722 cells
before the grid's margins: no one-window grid holds them).

Every structure carries 64-bit ids in no order, some with pairs of equal ids whose effect on the oracle's values the CPU
test asserts.  The module restates the arithmetic of k_sort_window that the cases are named for (windows, counter words,
the end marker, sorted positions) in numpy.  EXPECT holds what every structure is meant to be - grid and atoms per
window - as numbers; the CPU test compares them with what tc.grid_of / tc.cell_index give.  Plain helper module (not a
conftest)."""
import functools
from dataclasses import dataclass, field

import numpy as np

import tail_cases as tc
from oracle import pyoracle as po

PROBE = tc.PROBE
W = tc.WINDOW_CELLS

THREADS = 1024            # kSortWindowThreads
SLOT_ATOMS = 8 * THREADS  # kSlots * 1024: the atoms whose cell and position stay in registers
CHUNK_ATOMS = 4 * THREADS  # kChunk slots: the record pass skips its second chunk unless a structure has more atoms
TRIP_ATOMS = 4 * THREADS  # rest atoms per trip of the workgroup
STAGE = W * 2 // 32       # kStage: records the counter memory stages
PER = 19                  # kPer: counter words one thread scans
SINGLE_ATOMS = 8192       # host_batch.cpp kSingleAtoms
assert STAGE == 2304 and PER == ((W // 2 + THREADS - 1) // THREADS) | 1

N_POINTS = 100
HASH = np.uint64(0x9E3779B97F4A7C15)   # an odd multiplier: a bijection of the 64-bit ids


@dataclass
class Structure(tc.Structure):
    ids: np.ndarray = None                       # uint64, in no order
    pairs: list = field(default_factory=list)    # (i, j): atoms given one id, chosen so that a value changes


# ---- ids --------------------------------------------------------------------------------------------------------------

def _near(st, i, reach):
    d2 = (st.x.astype(np.float64) - float(st.x[i])) ** 2 + (st.y.astype(np.float64) - float(st.y[i])) ** 2 + \
        (st.z.astype(np.float64) - float(st.z[i])) ** 2
    return d2, np.flatnonzero(d2 <= reach * reach)


def pair_matters(st, i, j):
    """Whether one id for atoms i and j changes the oracle's value of i or of j.  Decided on the atoms within 12 A of i:
    spheres touch within 2 (1.5 + 0.5) = 4 A, j is within 4 A of i, so every atom that decides either value is there."""
    d2, near = _near(st, i, 12.0)
    if d2[j] > 16.0:
        return False
    pi, pj = int(np.searchsorted(near, i)), int(np.searchsorted(near, j))
    sub = [np.ascontiguousarray(a[near]) for a in (st.x, st.y, st.z, st.r)]
    ids = np.arange(len(near), dtype=np.uint64)
    base = po.calculate_sasa_internal(*sub, ids, PROBE, N_POINTS, 8)
    ids[pj] = ids[pi]
    dup = po.calculate_sasa_internal(*sub, ids, PROBE, N_POINTS, 8)
    return bool(base[pi] != dup[pi] or base[pj] != dup[pj])


def find_pair(st, first, second=None):
    """(i, j): i among the atoms `first` (tried in order), j one of its four nearest atoms (among the atoms `second`, a
    mask, if given) such that the pair matters."""
    for i in np.asarray(first, np.int64)[:48]:
        d2, _ = _near(st, int(i), 12.0)
        d2[i] = np.inf
        if second is not None:
            d2[~second] = np.inf
        for j in np.argsort(d2)[:4]:
            if d2[j] <= 16.0 and pair_matters(st, int(i), int(j)):
                return int(i), int(j)
    raise AssertionError("no pair of neighbours whose shared id changes a value")


def _with_ids(st, seed, pairs=()):
    """The structure with hashed ids (all different, in no order); the later atom of every pair takes the earlier
    one's id, as _id_variants.with_pair of test_gpu_parity.py does."""
    n = len(st)
    ids = (np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(10 + 1000003 * seed)) * HASH
    assert len(np.unique(ids)) == n
    pairs = [(min(p), max(p)) for p in pairs]
    for i, j in pairs:
        ids[j] = ids[i]
    return Structure(st.x, st.y, st.z, st.r, st.dims, st.blob, st.site, ids, pairs)


def _subset(st, keep):
    """The atoms `keep` (a mask) of a tail_cases structure, in their input order."""
    return tc.Structure(*(np.ascontiguousarray(a[keep]) for a in (st.x, st.y, st.z, st.r)), st.dims, st.blob[keep],
                        st.site[keep])


# ---- the arithmetic of k_sort_window, restated ------------------------------------------------------------------------

def cells_of(st):
    """(cell index of every atom, dims): tc.cell_index on tc.grid_of."""
    mn, inv, d = tc.grid_of(st.x, st.y, st.z, st.r)
    return tc.cell_index(st.x, st.y, st.z, mn, inv, d), tuple(int(v) for v in d)


def clamp_lowered(st):
    """Atoms whose cell coordinate the clamp to dim - 1 lowered on some axis (cell_coords; none is meant to be)."""
    mn, inv, d = tc.grid_of(st.x, st.y, st.z, st.r)
    n = 0
    for k, a in enumerate((st.x, st.y, st.z)):
        n += int(np.sum(((a - mn[k]) * inv).astype(np.int64) > d[k] - 1))
    return n


def n_windows(n_cells):
    return -(-n_cells // W)


def window_atoms(st):
    cell, d = cells_of(st)
    return np.bincount(cell // W, minlength=n_windows(int(np.prod(d)))).tolist()


def last_window(n_cells):
    """What the last window of a grid of n_cells cells is to k_sort_window and to lds_cell_slots."""
    nc = n_cells - (n_windows(n_cells) - 1) * W
    n_words = (nc + 1) >> 1
    return dict(n_cells=nc, odd=nc & 1, n_words=n_words, words_mod_per=n_words % PER,
                start_stores=(nc + 1 + 7) // 8, padding=tc.lds_cell_slots(n_cells) - n_cells - 1)


def rest_atoms(n):
    """(atoms beyond the registers' share, trips of the workgroup over them, live lanes of the last trip's last slot
    pass - its atoms modulo 4 096, 0: a full trip)."""
    rest = max(0, n - SLOT_ATOMS)
    return rest, -(-rest // TRIP_ATOMS), rest % TRIP_ATOMS


def runs_of(st):
    """(cell of every atom, start, end): the run of sorted positions [start, end) of every atom's cell, counted from
    the first position of the cell's window (`rel` of the kernel is start + the atom's arrival number)."""
    cell, d = cells_of(st)
    count = np.bincount(cell, minlength=int(np.prod(d)))
    start = np.cumsum(count) - count
    placed = start[(cell // W) * W]
    return cell, start[cell] - placed, start[cell] + count[cell] - placed


def staging_populations(st, window):
    """Atoms of `window` by (slot | rest) x (cell's run ends at or below STAGE | starts at or above it): the atoms
    whose way out - LDS or direct store - does not depend on the order of arrival."""
    cell, start, end = runs_of(st)
    mine = cell // W == window
    slot = np.arange(len(st)) < SLOT_ATOMS
    return dict(slot_staged=int(np.sum(mine & slot & (end <= STAGE))), slot_direct=int(np.sum(mine & slot & (start >= STAGE))),
                rest_staged=int(np.sum(mine & ~slot & (end <= STAGE))), rest_direct=int(np.sum(mine & ~slot & (start >= STAGE))))


def census_centres(n):
    """The first input atom, the last, and input atom 8 192 where it exists (the first rest atom), else the middle."""
    return sorted({0, n - 1, SLOT_ATOMS if n > SLOT_ATOMS else n // 2}) if n else []


def extent(st):
    return float(max(np.ptp(st.x), np.ptp(st.y), np.ptp(st.z))) if len(st) else 0.0


# ---- generators -----------------------------------------------------------------------------------------------------

BLOCK_SPACING = 2.4   # A: 0.072 atoms / A^3 (proteins are denser still)
BLOCK_JITTER = 0.5    # A (least separation: spacing - 2 * jitter = 1.4 A)


def block_structure(n, seed, origin):
    """n atoms on distinct sites of the smallest cubic lattice that holds them, jittered, in input order a random walk
    over the sites; the first atom has the largest radius (the cell is 2.0).  The grid is what the formula gives."""
    rng = np.random.default_rng(seed)
    m = 1
    while m ** 3 < n:
        m += 1
    site = rng.permutation(m ** 3)[:n]
    g = np.stack(np.unravel_index(site, (m,) * 3), -1).astype(np.float64)
    xyz = np.round(g * BLOCK_SPACING + rng.uniform(0.0, 2.0 * BLOCK_JITTER, size=g.shape) + np.asarray(origin), 3)
    xyz = xyz.astype(np.float32)
    r = rng.choice(np.array([1.3, 1.4, 1.5], np.float32), size=n).astype(np.float32)
    r[0] = tc.R_MAX
    return tc.Structure(*(np.ascontiguousarray(xyz[:, k]) for k in range(3)), r, None, np.zeros(n, np.int64), site)


Z_GROUP = 4   # lattice layers along z that lattice_structure keeps or leaves out together


def lattice_structure(dims, n_atoms, seed):
    """n_atoms atoms in a grid of exactly dims cells, for boxes with an axis shorter than a blob: two atoms (radius 1.5)
    at 0 and at 2 D - 6, the others on a jittered lattice of tail_cases.DENSITY through the box from 0.5 A inside its
    first corner to 0.5 A inside its last.  An axis holds floor((L - 1) / a) + 1 sites, stretched over it; the jitter is
    2 * JITTER or what the axis leaves.  Fewer atoms than sites: groups of Z_GROUP z layers spread evenly over the box
    are kept whole (every atom keeps its neighbours), and sites are dropped at random from those to reach the count.
    Coordinates are rounded to 3 decimals and the order is shuffled, as tc.boxed_structure does."""
    rng = np.random.default_rng(seed)
    a = tc.lattice_spacing()
    ext = np.array([2.0 * d - 6.0 for d in dims])
    m = np.floor((ext - 1.0) / a).astype(np.int64) + 1
    width = np.minimum(2.0 * tc.JITTER, ext - 1.0 - (m - 1) * a)
    step = np.where(m > 1, (ext - 1.0 - width) / np.maximum(m - 1, 1), 0.0)
    assert np.all(step[m > 1] - width[m > 1] > 1.3)
    n_sites = n_atoms - 2
    per_group = int(m[0] * m[1]) * Z_GROUP
    n_groups = -(-int(m[2]) // Z_GROUP)
    assert 0 < n_sites <= int(np.prod(m)), (dims, n_sites, int(np.prod(m)))
    iz, iy, ix = np.meshgrid(np.arange(m[2]), np.arange(m[1]), np.arange(m[0]), indexing="ij")
    sites = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], -1)
    for want in range(-(-n_sites // per_group), n_groups + 1):   # (one more if the box's last, short group is among them)
        groups = np.unique(np.round(np.linspace(0, n_groups - 1, want)).astype(np.int64))
        idx = sites[np.isin(sites[:, 2] // Z_GROUP, groups)]
        if len(idx) >= n_sites:
            break
    idx = idx[np.sort(rng.permutation(len(idx))[:n_sites])]
    xyz = 0.5 + idx * step + rng.uniform(0.0, 1.0, size=idx.shape) * width
    xyz = np.round(np.concatenate([np.zeros((1, 3)), ext[None, :], xyz]), 3)
    r = rng.choice(np.array([1.3, 1.4, 1.5], np.float32), size=n_atoms)
    r[:2] = tc.R_MAX
    site = np.concatenate([[-1, -1], idx[:, 0] + m[0] * (idx[:, 1] + m[1] * idx[:, 2])])
    blob = np.concatenate([[-1, -1], idx[:, 2] // Z_GROUP])
    order = rng.permutation(n_atoms)
    xyz, r = xyz[order].astype(np.float32), r[order].astype(np.float32)
    assert xyz.min() == 0.0 and np.array_equal(xyz.max(0), ext.astype(np.float32)) and r.max() == np.float32(tc.R_MAX)
    return tc.Structure(*(np.ascontiguousarray(xyz[:, k]) for k in range(3)), r, tuple(dims), blob[order], site[order])


def without_window(st, window):
    """The structure without the atoms of one window (the two atoms that fix the grid are in the first and the last)."""
    cell, _ = cells_of(st)
    assert np.all(cell[st.blob < 0] // W != window)
    return _subset(st, cell // W != window)


def with_window_counts(st, counts):
    """The structure cut down to counts[w] atoms in window w: of every window its blobs in their order and of a blob its
    sites in theirs, as many as the count asks for (whole blobs and a part of one: the atoms keep their neighbours)."""
    cell, _ = cells_of(st)
    win = cell // W
    keep = st.blob < 0
    rank = np.lexsort((st.site, st.blob))
    for w, n in enumerate(counts):
        cand = rank[(win[rank] == w) & (st.blob[rank] >= 0)]
        n -= int(np.sum(keep & (win == w)))
        assert 0 <= n <= len(cand), (w, n, len(cand))
        keep[cand[:n]] = True
    out = _subset(st, keep)
    got = window_atoms(out)
    assert got[:len(counts)] == list(counts) and not any(got[len(counts):])
    return out


FINE_SIDE = 35        # sites per axis of the fine lattice of (d): 42 875 atoms
FINE_STEP = 0.05      # A: the lattice spans 1.7 A, inside one cell of 2.0 A


def dense_structure(dims, corner, seed, n_atoms=65535):
    """n_atoms atoms in a grid of dims cells: FINE_SIDE^3 of them on a lattice of distinct coordinates whose first site
    is `corner` (0.1 A inside a cell), the others in the blobs of tc.boxed_structure."""
    rng = np.random.default_rng(seed)
    n_fine = FINE_SIDE ** 3
    st = tc.boxed_structure(dims, n_atoms - n_fine, seed)
    g = np.stack(np.unravel_index(rng.permutation(n_fine), (FINE_SIDE,) * 3), -1)
    fine = np.round(np.asarray(corner, np.float64) + g * FINE_STEP, 3).astype(np.float32)
    assert len(np.unique(fine, axis=0)) == n_fine
    order = rng.permutation(n_atoms)
    cat = lambda a, b: np.ascontiguousarray(np.concatenate([a, b])[order])  # noqa: E731
    r = rng.choice(np.array([1.3, 1.4, 1.5], np.float32), size=n_fine).astype(np.float32)
    return tc.Structure(cat(st.x, fine[:, 0]), cat(st.y, fine[:, 1]), cat(st.z, fine[:, 2]), cat(st.r, r), tuple(dims),
                        cat(st.blob, np.full(n_fine, -2)), cat(st.site, np.arange(n_fine)))


# ---- the structures ---------------------------------------------------------------------------------------------------

LADDER = (1, 2, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12287, 12288, 12289)
# structures with a pair of equal ids (the sizes of the single-structure cases among them; the ids of the others are all
# different, and the sort drops them); past 8 192 atoms the pair's later atom is a rest atom
LADDER_PAIRS = (1024, 1025, 4096, 4097, 8191, 8192, 8193, 12289)

DIMS = {
    "thin_W+1": (5, 73, 101), "thin_2W+2": (10, 73, 101), "thin_2W+38": (11, 14, 479), "thick_3W+38": (23, 65, 74),
    "thick_3W+1": (37, 49, 61), "lattice_3W-1": (13, 47, 181), "thick_3W+8": (25, 56, 79),
}
DIMS_STAGE = DIMS["thick_3W+1"]
STAGE_COUNTS = {"stage_2303": (1000, 2303, 1000), "stage_2304": (1000, 2304, 1000), "stage_2305": (1000, 2305, 1000),
                "stage_mixed": (3500, 3000, 3500)}
DIMS_DENSE = {"dense_even": (52, 52, 52), "dense_odd": (53, 52, 52)}


def _ladder(n):
    k = LADDER.index(n)
    st = block_structure(n, 200 + k, origin=(37.0 * k - 200.0, -11.5 * k, 3.25 * k - 20.0))
    pairs = []
    if n in LADDER_PAIRS:
        # the later atom of the pair: past the registers' share where the structure has rest atoms
        first = np.arange(SLOT_ATOMS, n) if n > SLOT_ATOMS else np.arange(n // 2, n)
        pairs.append(find_pair(st, first, np.arange(n) < min(n // 2, SLOT_ATOMS)))
    return _with_ids(st, 200 + k, pairs)


def _boxed(name, n_atoms, seed):
    d = DIMS[name]
    blobs = all(2.0 * v - 7.0 >= tc.blob_extent() for v in d)
    st = tc.boxed_structure(d, n_atoms, seed) if blobs else lattice_structure(d, n_atoms, seed)
    return _with_ids(st, seed, [find_pair(st, np.flatnonzero(st.blob >= 0)[seed:])])


def _hole():
    st = without_window(tc.boxed_structure(DIMS_STAGE, 9000, 47), 1)
    return _with_ids(st, 48, [find_pair(st, np.flatnonzero(st.blob >= 0)[100:])])


@functools.lru_cache(maxsize=None)
def _stage_base():
    return tc.boxed_structure(DIMS_STAGE, 24 * tc.BLOB_SIDE ** 3 + 2, 50)


def _stage(name):
    st = with_window_counts(_stage_base(), STAGE_COUNTS[name])
    seed = 51 + sorted(STAGE_COUNTS).index(name)
    cell, start, end = runs_of(st)
    mine = cell // W == 1
    if name == "stage_mixed":
        # both atoms in window 1, in cells on opposite sides of position STAGE: the cells that end nearest below it
        # have their y and z neighbours above it
        below = np.flatnonzero(mine & (end <= STAGE))
        pair = find_pair(st, below[np.argsort(-end[below], kind="stable")], mine & (start >= STAGE))
    else:
        pair = find_pair(st, np.flatnonzero(mine)[10:])
    return _with_ids(st, seed, [pair])


def _dense(name):
    d = DIMS_DENSE[name]
    # the fine lattice in the first window of one structure and in the last window of the other
    corner = (20.1, 20.1, 10.1) if name == "dense_even" else (60.1, 60.1, 90.1)
    return _with_ids(dense_structure(d, corner, 60 + len(name)), 60)


def _single(name):
    st = lattice_structure(DIMS[name[len("single_"):]], 4097, 70 + len(name))
    return _with_ids(st, 70, [find_pair(st, np.flatnonzero(st.blob >= 0)[30:])])


def _empty():
    e = tc.empty_structure()
    return Structure(e.x, e.y, e.z, e.r, e.dims, e.blob, e.site, np.zeros(0, np.uint64), [])


BUILDERS = {f"ladder_{n}": functools.partial(_ladder, n) for n in LADDER}
BUILDERS.update({
    "thin_W+1": functools.partial(_boxed, "thin_W+1", 7490, 41),          # every site of the lattice
    "thin_2W+2": functools.partial(_boxed, "thin_2W+2", 12000, 42),
    "thin_2W+38": functools.partial(_boxed, "thin_2W+38", 12000, 43),
    "thick_3W+38": functools.partial(_boxed, "thick_3W+38", 9000, 44),
    "thick_3W+1": functools.partial(_boxed, "thick_3W+1", 9000, 45),
    "lattice_3W-1": functools.partial(_boxed, "lattice_3W-1", 12000, 46),
    "thick_3W+8": functools.partial(_boxed, "thick_3W+8", 9000, 49),
    "hole": _hole,
    "empty": _empty,
})
BUILDERS.update({n: functools.partial(_stage, n) for n in STAGE_COUNTS})
BUILDERS.update({n: functools.partial(_dense, n) for n in DIMS_DENSE})
BUILDERS.update({"single_" + n: functools.partial(_single, "single_" + n) for n in ("thin_W+1", "thin_2W+2", "thin_2W+38")})


@functools.lru_cache(maxsize=None)
def structure(name):
    return BUILDERS[name]()


# What every structure is meant to be: (dims, atoms of every window).  Counted once with window_atoms (tc.cell_index in
# numpy) and written down; test_window_cases_cpu.py holds the generators to them.
EXPECT = {
    "ladder_1": ((3, 3, 3), [1]),
    "ladder_2": ((4, 4, 4), [2]),
    "ladder_1023": ((16, 16, 16), [1023]),
    "ladder_1024": ((16, 16, 16), [1024]),
    "ladder_1025": ((16, 16, 16), [1025]),
    "ladder_4095": ((22, 22, 22), [4095]),
    "ladder_4096": ((22, 22, 22), [4096]),
    "ladder_4097": ((23, 23, 23), [4097]),
    "ladder_8191": ((28, 28, 28), [8191]),
    "ladder_8192": ((28, 28, 28), [8192]),
    "ladder_8193": ((28, 28, 28), [8193]),
    "ladder_12287": ((32, 32, 32), [12287]),
    "ladder_12288": ((32, 32, 32), [12288]),
    "ladder_12289": ((32, 32, 32), [12289]),
    "thin_W+1": ((5, 73, 101), [7490, 0]),
    "thin_2W+2": ((10, 73, 101), [6120, 5880, 0]),
    "thin_2W+38": ((11, 14, 479), [5924, 6076, 0]),
    "thick_3W+38": ((23, 65, 74), [3317, 2740, 2943, 0]),
    "thick_3W+1": ((37, 49, 61), [3203, 2931, 2866, 0]),
    "lattice_3W-1": ((13, 47, 181), [4290, 3610, 4100]),
    "thick_3W+8": ((25, 56, 79), [3073, 3072, 2855, 0]),
    "hole": ((37, 49, 61), [3223, 0, 2863, 0]),
    "empty": ((1, 1, 1), [0]),
    "stage_2303": ((37, 49, 61), [1000, 2303, 1000, 0]),
    "stage_2304": ((37, 49, 61), [1000, 2304, 1000, 0]),
    "stage_2305": ((37, 49, 61), [1000, 2305, 1000, 0]),
    "stage_mixed": ((37, 49, 61), [3500, 3000, 3500, 0]),
    "dense_even": ((52, 52, 52), [48508, 6007, 6483, 4537]),
    "dense_odd": ((53, 52, 52), [5633, 5794, 6418, 47690]),
    "single_thin_W+1": ((5, 73, 101), [4097, 0]),
    "single_thin_2W+2": ((10, 73, 101), [2047, 2050, 0]),
    "single_thin_2W+38": ((11, 14, 479), [2070, 2027, 0]),
}

# ---- the cases --------------------------------------------------------------------------------------------------------

WINDOW_SHAPES = ("thin_W+1", "thin_2W+2", "thin_2W+38", "thick_3W+38", "thick_3W+1", "lattice_3W-1", "thick_3W+8", "hole")
BATCHES = {
    "ladder": [f"ladder_{n}" for n in LADDER],
    "ladder_reversed": [f"ladder_{n}" for n in LADDER[:6:-1]] + ["empty"] + [f"ladder_{n}" for n in LADDER[6::-1]],
    # (lattice_3W-1 has no padding behind its end marker: the empty structure's cell_base follows it directly)
    "interleaved": ["thick_3W+8", "lattice_3W-1", "empty", "ladder_1025", "thin_W+1", "thin_2W+2"],
    "staging": list(STAGE_COUNTS),
    "dense": list(DIMS_DENSE),
}
BATCHES.update({n: [n] for n in WINDOW_SHAPES})
SORT_CASES = ("ladder", "ladder_reversed") + WINDOW_SHAPES + ("interleaved", "staging")   # (a), (b), (c)

SINGLE_SIZES = (1, 1024, 1025, 4096, 4097, 8191, 8192, 8193)   # (e); 8 193: the other side of kSingleAtoms
SINGLE_CASES = tuple(f"ladder_{n}" for n in SINGLE_SIZES) + ("single_thin_W+1", "single_thin_2W+2", "single_thin_2W+38")


def names_of(case):
    return BATCHES[case]


@functools.lru_cache(maxsize=None)
def get(case):
    sts = [structure(n) for n in BATCHES[case]]
    return tc.Case(case, sts, ids=np.concatenate([s.ids for s in sts]))


def n_cells_sum(case):
    return sum(int(np.prod(EXPECT[n][0])) for n in BATCHES[case])


def census_flags(case):
    """Flag bytes of a batch: every atom a partner (1), census_centres of every structure centres as well (3)."""
    c = get(case)
    fl = np.ones(c.n_atoms, np.uint8)
    for s, st in enumerate(c.structures):
        fl[int(c.so[s]) + np.asarray(census_centres(len(st)), np.int64)] = 3
    return fl


def census_cutoff(case):
    """Four times the largest extent of the batch's structures: beyond every atom of every structure, and the stop rule
    of cutoff_sweep.h - c2 <= ((s - 0.5) h)^2 - cannot fire while a shell of the grid is left (s h stays below
    the extent + 4 h)."""
    return 4.0 * max(extent(st) for st in get(case).structures)


def residue_offsets(n):
    """Offsets that leave out the first three and the last atoms, residues of 7 atoms with an empty one among them."""
    if n < 24:
        return np.array([0, 0] if n < 2 else [1, 1, n - 1], np.uint32)
    ro = np.arange(3, n - 4, 7, dtype=np.uint32)
    return np.insert(ro, 2, ro[2])
