"""The inputs of the second pass over the radial counts (test_radial_edges_cpu.py, test_gpu_radial_edges.py): what the
first suite of k_radial_counts / k_radial_pairs (radial.hip) never gave them.

    ladder          one centre and 32 partners at the integer distances 1 .. 32: with the edges 1 .. n_bins every partner
                    ties with one edge exactly, at every n_bins from 1 to 32 - every padded size P of the bin search and
                    every first step `half` -, and one float32 ulp further out it belongs to the next bin;
    OVERFLOW_EDGES  two edges whose squares overflow to +inf, where they meet the search's padding;
    chunk_batch     structure boundaries and empty structures exactly on the 1 024-atom chunk edges of k_radial_pairs, and
                    a structure across three chunks, with N a multiple of the chunk and one more;
    PAIR_SHAPES     rows of 1, 3, 256, 260 and 512 cells for it.

The awkward grids and the margins' edge come from cutoff_edge_cases.py; this module only adds their classes and edge
lists.  Seeded, cached and small; the CPU file pins every case to what it is named for from radial_model alone.  Plain
helper module (not a conftest)."""
import functools

import numpy as np

import cutoff_edge_cases as ce
import hse_cases as hc
import radial_cases as rc

F = np.float32
FLT_MAX = float(np.finfo(F).max)
N_CLASSES = rc.N_CLASSES

# ---- exact ties on every edge --------------------------------------------------------------------------------------------

LADDER = 32                        # partners, at distances 1 .. 32 (RSASA_RADIAL_MAX_BINS)
REPEAT_BINS = (3, 5, 8, 17, 31, 32)


@functools.lru_cache(maxsize=None)
def ladder(moved=False):
    """Atom 0, the centre (flag 2, class 0), at hse_cases.TIE_ORIGIN; atom k = 1 .. 32 a partner (flag 1, class
    (k - 1) % 4) k further along +x: dx = k exactly, d2 = k * k exactly, and the edge k squares to the same number.
    moved: every partner's x is the next float32 above, so dx = k + an ulp of a coordinate near 100 (exact: k <= 32 has
    bits to spare) and d2 > k * k."""
    o = np.array(hc.TIE_ORIGIN, np.float64)
    xyz = np.tile(o, (LADDER + 1, 1)).astype(F)
    for k in range(1, LADDER + 1):
        v = F(o[0] + k)
        xyz[k, 0] = np.nextafter(v, F(np.inf)) if moved else v
    flags = np.full(LADDER + 1, 1, np.uint8)
    flags[0] = 2
    return hc._case("ladder_moved" if moved else "ladder", xyz, np.full(LADDER + 1, 1.5, F), flags=flags)


def ladder_classes():
    return np.concatenate([[0], np.arange(LADDER) % N_CLASSES]).astype(np.uint8)


def ladder_edges(n_bins, repeated=False):
    """The edges 1 .. n_bins.  repeated: runs of 1, 3 and 2 equal edges in turn, each run holding its first edge -
    (1, 2, 2, 2, 5, 5, 7, 8, 8, 8, 11, 11, 13, ...) - cut to n_bins."""
    e = np.arange(1, n_bins + 1, dtype=np.float64)
    if repeated:
        k, run = 0, 0
        while k < n_bins:
            n = (1, 3, 2)[run % 3]
            e[k:k + n] = e[k]
            k, run = k + n, run + 1
    return tuple(float(v) for v in e)


def ladder_row(edges, moved=False):
    """The centre's row worked out from the construction alone: partner k, at distance k, goes to the first bin whose
    edge is >= k; moved, just beyond k, to the first whose edge is > k; to none if there is no such edge."""
    e = np.asarray(edges, np.float64)
    row = np.zeros((N_CLASSES, len(e)), np.uint32)
    for k in range(1, LADDER + 1):
        ok = np.flatnonzero(e > k if moved else e >= k)
        if len(ok):
            row[(k - 1) % N_CLASSES, ok[0]] += 1
    return row


# ---- squares that overflow -------------------------------------------------------------------------------------------------

def overflow_edges():
    """(h, 1e19, 1e20, FLT_MAX) on hse_cases.cluster(): the squares are finite, finite (1e38), +inf, +inf."""
    return (float(hc.cluster().h), 1e19, 1e20, FLT_MAX)


OVERFLOW_EDGES = overflow_edges()


# ---- awkward grids and the margins' edge: classes and edge lists -----------------------------------------------------------

def grid_classes(c, seed):
    return rc.classes_of(c.n_atoms, N_CLASSES, seed)


def swept_classes(name):
    return grid_classes(ce.swept(name), 700 + (ce.GRID_NAMES + ce.MARGIN_NAMES).index(name))


def swept_edges(name):
    """The three cutoffs at which the stop rule holds with equality and 13 A (4 h for margin_small_h, whose cell is 0.1 A),
    in ascending order (13 A comes first under margin_large_h's cell of 40 A)."""
    c = ce.swept(name)
    return tuple(sorted(ce.cell_cutoffs(c) + [float(F(4.0) * c.h) if name == "margin_small_h" else 13.0]))


def prefixes(edges):
    """Every non-empty prefix (the full list last): each edge is once the last one, the stop rule's."""
    return [tuple(edges[:k]) for k in range(1, len(edges) + 1)]


def swept_edge_lists(name):
    """The prefixes of swept_edges, and a covering cutoff as a single edge where the largest structure is under 1 000 atoms."""
    c = ce.swept(name)
    out = prefixes(swept_edges(name))
    if int(np.diff(c.so.astype(np.int64)).max()) < 1000:
        out.append((ce.covering_cutoff(c),))
    return out


EDGE_LISTS = ((2.0, hc.EDGE_CUTOFF), (hc.EDGE_CUTOFF, 7.0), (float(np.nextafter(F(hc.EDGE_CUTOFF), F(np.inf))),))


def flags_of(c, fk):
    """fk: None, or "eighth" (cutoff_edge_cases.one_in_eight: one centre in eight, every atom a partner)."""
    return None if fk is None else ce.one_in_eight(c.n_atoms)


# ---- k_radial_pairs: structures on the chunk edges ---------------------------------------------------------------------------

CHUNK = 1024                       # kRdChunk
PAIR_THREADS = 256                 # kRdThreads
BOX = 8.0                          # under three cells of 2.9 A

# (n_classes, n_bins): widths 1 and 4, a row of exactly 256 cells, 260 cells (four threads hold a second cell), 512 cells
PAIR_SHAPES = ((1, 1), (3, 1), (16, 16), (10, 26), (16, 32))

# No batch of 4 096 atoms has structure boundaries on 1 024 AND 2 048 and a structure across three chunks (that one
# would have to cross two of the three inner chunk edges): two layouts.
LAYOUTS = {"edges": (0, 1024, 0, 0, 1024, 2048, 0, 0),     # offsets 0 0 1024 1024 1024 2048 4096 4096 4096
           "span": (0, 1024, 0, 0, 2500, 572, 0, 0)}       # offsets 0 0 1024 1024 1024 3524 4096 4096 4096


@functools.lru_cache(maxsize=None)
def chunk_batch(extra=False, layout="edges"):
    """Random points in a box of 8 A (every structure in the same box: they never count each other), radii 1.5.  An empty
    structure in front, two in a row at offset 1 024, two at the end; N = 4 096.  extra: a one-atom structure before the
    trailing empty ones, N = 4 097 - a fifth chunk of one atom."""
    sizes = list(LAYOUTS[layout])
    if extra:
        sizes.insert(len(sizes) - 2, 1)
    rng = np.random.default_rng(71 + len(layout))
    xyz = np.round(rng.uniform(0.0, BOX, (sum(sizes), 3)), 3)
    so = np.concatenate([[0], np.cumsum(sizes)])
    return hc._case(f"chunk_{layout}{'_extra' if extra else ''}", xyz, np.full(len(xyz), 1.5, F), so)


def chunk_classes(n, n_classes, seed=72):
    """Seeded class bytes; from ten classes on, chunk c of 1 024 atoms lacks class (5 c + 3) % n_classes."""
    cl = rc.classes_of(n, n_classes, seed + n_classes)
    if n_classes >= 10:
        for c in range(-(-n // CHUNK)):
            part = cl[c * CHUNK:(c + 1) * CHUNK]
            gone = (5 * c + 3) % n_classes
            part[part == gone] = (gone + 1) % n_classes
    return cl


def chunk_edges(n_bins):
    return tuple(float(e) for e in rc.edges_of(n_bins))


def chunk_flags(n, seed=73):
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)


# ---- threads ---------------------------------------------------------------------------------------------------------------------

THREADS, THREAD_ROUNDS = 8, 10
THREAD_CALLS = ("radial", "owners", "hse", "contacts")


THREAD_POINTS = 100


@functools.lru_cache(maxsize=None)
def thread_case(name):
    """An input of cutoff_edge_cases.THREAD_INPUTS: the 1jcd fixture without hetero atoms, or the case of hse_cases.py."""
    if name != "1jcd":
        return getattr(hc, name)()
    import structio as sio
    atoms = [a for a in sio.read_structure(sio.data_path("1jcd.pdb")) if not a.hetero]
    x, y, z, r, _ = sio.soa_vdw(atoms)
    return hc.Case("1jcd", *(np.ascontiguousarray(a, F) for a in (x, y, z, r)), np.array([0, len(x)], np.uint32),
                   hc.random_dirs(len(x), 950))


def thread_calls(tid, it):
    """The four calls in the order thread tid makes them in round it, on the input cutoff_edge_cases.thread_input(tid, it):
    in every round the threads start at different calls."""
    k = (tid + it) % len(THREAD_CALLS)
    return THREAD_CALLS[k:] + THREAD_CALLS[:k]
