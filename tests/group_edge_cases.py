"""The inputs of the group-contact edge tests (test_group_edges_cpu.py, test_gpu_group_edges.py): labellings of the
tight clusters that give k_group_points long own prefixes, foreign runs of whole LDS stages and a last foreign entry in
a padded and in an unpadded group of four; a batch that mixes both binning routes, spilled neighbour lists, tiny and
empty structures; thousands of tiny structures; and the sizes at which the row-offset scan takes several tiles.  The
CPU file pins every input to the class it is named for, from the oracle's lists and the labels alone; the GPU file
compares k_group_order / k_group_points / gp_run with groups_model.py on them.  Plain helper module (not a conftest)."""
import functools

import numpy as np

import groups_model as gm
import nb_helpers as nh
import point_edge_cases as pe
import tail_cases as tl

PROBE = 1.4
W = 16                           # the lane count of the cluster cases: 100 -> 96 fused, 300 -> 288 fused
CLUSTER_SIZES = (258, 514, 769)  # K = n - 1 = 257, 513, 768 in the whole cluster: two, three and three full stages
CLUSTER_POINTS = (100, 300)      # one pass of NCH = 2; two passes of NCH = 4
CLUSTER_KINDS = ("one_label", "head_against_rest", "own_then_many", "two_long_runs")
OWN_BLOCK = 300                  # own_then_many: the cluster atoms that share one label
ROW_REGS = 4 * pe.WAVE           # rows of an atom that k_group_points counts in registers (kGpRowRegs * kWave)
NB_STAGE = 512                   # keys k_neighbor_fill stages per list (kNbStage); longer lists spill

# cluster labels, all above the protein's "blocked" labels (index // 40 < 27)
LABEL_A, LABEL_B, LABEL_C = 1000, 2000, 3000


def blocked(n):
    return np.arange(n, dtype=np.uint32) // np.uint32(40)


def cluster_keys():
    return [(n, kind) for n in CLUSTER_SIZES for kind in CLUSTER_KINDS if kind != "own_then_many" or n >= 514]


def cluster_labels(kind, n_total, c0, block=OWN_BLOCK):
    """The protein in blocks of 40; the cluster [c0, n_total) by `kind`:
    one_label          every cluster atom B: n_own = n - 1, no rows
    head_against_rest  atom c0 A, the others B: from c0 one foreign run of n - 1 entries; from the others n - 2 own
                       entries, then one foreign entry, the last of the list
    own_then_many      the first `block` (300) atoms A, every other atom a label of its own above 2^31, in no order: an own
                       prefix (or a first foreign run) that ends inside the second stage, then n - 300 runs of one
    two_long_runs      atom c0 A, the halves of the rest B and C: from c0 two runs with their seam inside a stage"""
    g = blocked(n_total)
    n = n_total - c0
    if kind == "one_label":
        g[c0:] = LABEL_B
    elif kind == "head_against_rest":
        g[c0:] = LABEL_B
        g[c0] = LABEL_A
    elif kind == "own_then_many":
        assert n > block
        g[c0:c0 + block] = LABEL_A
        rest = n - block
        scattered = np.random.default_rng(n).permutation(rest).astype(np.uint64) * np.uint64(7919)
        g[c0 + block:] = (np.uint64(0x80000001) + scattered).astype(np.uint32)
    elif kind == "two_long_runs":
        half = (n - 1) // 2
        g[c0] = LABEL_A
        g[c0 + 1:c0 + 1 + half] = LABEL_B
        g[c0 + 1 + half:] = LABEL_C
    else:
        raise KeyError(kind)
    return g


@functools.lru_cache(maxsize=None)
def cluster(n, kind, shared_ids=False):
    """(columns, labels, first cluster index) of tight_cluster(n, seed=n) under `kind`."""
    cols, c0 = nh.tight_cluster(n, seed=n, shared_ids=shared_ids)
    return cols, cluster_labels(kind, len(cols[0]), c0), c0


def list_classes(offs, ent, g, base=None):
    """What k_group_order makes of every list, from the lists and the labels alone: (n_own int64[n], rows int64[n],
    runs) with runs[i] the lengths of atom i's foreign runs in ascending label order.  base: the first atom of every
    atom's structure (idx is relative to it); None: one structure."""
    o = offs.astype(np.int64)
    n = len(o) - 1
    atom = np.repeat(np.arange(n, dtype=np.int64), np.diff(o))
    j = ent["idx"].astype(np.int64) + (0 if base is None else np.asarray(base, np.int64)[atom])
    lab = g[j]
    own = lab == g[atom]
    n_own = np.bincount(atom[own], minlength=n).astype(np.int64)
    fa, fl = atom[~own], lab[~own]
    order = np.lexsort((fl, fa))
    fa, fl = fa[order], fl[order]
    head = np.ones(len(fa), bool)
    head[1:] = (fa[1:] != fa[:-1]) | (fl[1:] != fl[:-1])
    starts = np.nonzero(head)[0]
    lens = np.diff(np.append(starts, len(fa)))
    rows = np.bincount(fa[starts], minlength=n).astype(np.int64)
    cuts = np.cumsum(rows)[:-1]
    return n_own, rows, np.split(lens, cuts)


def row_offsets(offs, ent, g, base=None):
    """out_offsets of a group call: the prefix sum of the distinct foreign labels in every atom's list."""
    _, rows, _ = list_classes(offs, ent, g, base)
    out = np.zeros(len(rows) + 1, np.uint64)
    out[1:] = np.cumsum(rows)
    return out


def structure_base(so):
    so = np.asarray(so, np.int64)
    return np.repeat(so[:-1], np.diff(so))


# ---- the model on many threads ----------------------------------------------------------------------------------

MODEL_CHUNK = 4096   # atoms per task


def batch_model(x, y, z, r, ids, groups, so, probe, n_points, W, chunk=None):
    """groups_model.group_counts_batch, computed in tasks of `chunk` (MODEL_CHUNK) atoms on pe.pmap's threads: every task is
    gm.group_counts on its whole structure with the oracle's lists of the task's atoms and empty lists elsewhere (a
    list's counts depend on nothing outside it), and the tasks' rows are joined in atom order."""
    chunk = chunk or MODEL_CHUNK
    tasks, lists = [], {}
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        if e > b:
            lists[s] = nh.oracle_csr(x[b:e], y[b:e], z[b:e], r[b:e], None if ids is None else ids[b:e], probe)
            tasks += [(s, a, min(a + chunk, e - b)) for a in range(0, e - b, chunk)]

    def one(task):
        s, a, c = task
        b, e = int(so[s]), int(so[s + 1])
        o = lists[s][0].astype(np.int64)
        k = np.zeros(e - b, np.int64)
        k[a:c] = np.diff(o[a:c + 1])
        lo = np.zeros(e - b + 1, np.uint64)
        lo[1:] = np.cumsum(k)
        m = gm.group_counts(x[b:e], y[b:e], z[b:e], r[b:e], None if ids is None else ids[b:e], groups[b:e], probe,
                            n_points, W, lists=(lo, lists[s][1][o[a]:o[c]]))
        return (np.diff(m[0].astype(np.int64))[a:c],) + m[1:4] + (m[4][a:c], m[5][a:c])
    done = pe.pmap(one, tasks)
    cat = lambda k, dt: np.concatenate([done[t][k] for t in tasks]).astype(dt) if tasks else np.zeros(0, dt)  # noqa: E731
    offs = np.zeros(int(so[-1]) + 1, np.uint64)
    offs[1:] = np.cumsum(cat(0, np.int64))
    return (offs,) + tuple(cat(k, np.uint32) for k in range(1, 6))


def slice_model(model, so, s):
    """Structure s of a batch model, its offsets rebased to 0."""
    b, e = int(so[s]), int(so[s + 1])
    lo, hi = int(model[0][b]), int(model[0][e])
    return (model[0][b:e + 1] - model[0][b],) + tuple(m[lo:hi] for m in model[1:4]) + tuple(m[b:e] for m in model[4:6])


def join_models(models):
    """The batch model of structures whose own models are `models`, in that order."""
    offs, base = [np.zeros(1, np.uint64)], 0
    for m in models:
        offs.append(m[0][1:] + np.uint64(base))
        base += int(m[0][-1])
    return (np.concatenate(offs),) + tuple(np.concatenate([m[k] for m in models]) for k in range(1, 6))


# ---- batches ----------------------------------------------------------------------------------------------------

def pack(parts):
    """[(columns, labels)] -> (the five columns concatenated, labels, structure offsets)."""
    so = np.zeros(len(parts) + 1, np.uint32)
    so[1:] = np.cumsum([len(c[0]) for c, _ in parts])
    cat = [np.ascontiguousarray(np.concatenate([c[k] for c, _ in parts])) for k in range(5)]
    return cat, np.ascontiguousarray(np.concatenate([g for _, g in parts]).astype(np.uint32)), so


def _empty():
    e = np.zeros(0, np.float32)
    return (e, e, e, e, np.zeros(0, np.uint64)), np.zeros(0, np.uint32)


MIXED_NAMES = ("empty", "single_atom", "overlapping_pair", "1jcd_by_chain", "cluster_300_shared_ids", "tail", "empty_2",
               "2drt_by_residue", "cluster_600_shared_ids")


@functools.lru_cache(maxsize=None)
def mixed_parts():
    """The structures of the mixed batch, in order, as [(columns, labels)]; labels start at 0 in every structure.  The
    first eight are: empty, one atom, two overlapping atoms with different labels, 1jcd by chain,
    tight_cluster(300, shared_ids=True) as head_against_rest, the smallest structure of tail_cases.py on the
    batch-wide binning route in blocks of 40, empty, 2drt by residue.  A list has to hold more than 512 entries to
    leave the neighbour staging, which the 299 of the 300-cluster do not: a ninth structure,
    tight_cluster(600, shared_ids=True) as head_against_rest, has lists of 400 (the atoms that share an id) and of 599
    entries, so both routes of the fill kernel in one structure."""
    f = lambda *a: np.array(a, np.float32)  # noqa: E731
    one = ((f(1.0), f(2.0), f(3.0), f(1.5), np.array([1], np.uint64)), np.zeros(1, np.uint32))
    two = ((f(0.0, 1.5), f(0.0, 0.5), f(0.0, 0.0), f(1.7, 1.5), np.array([1, 2], np.uint64)), np.array([0, 1], np.uint32))
    jcd = gm.labelled_fixture("1jcd.pdb")
    drt = gm.labelled_fixture("2drt.pdb")

    def shared_cluster(n):
        cols, c0 = nh.tight_cluster(n, seed=n, shared_ids=True)
        return cols, cluster_labels("head_against_rest", len(cols[0]), c0)
    st = tl._tail(0)
    tail = ((st.x, st.y, st.z, st.r, np.arange(1, len(st) + 1, dtype=np.uint64)), blocked(len(st)))
    return [_empty(), one, two, (jcd[0], jcd[1]), shared_cluster(300), tail, _empty(), (drt[0], drt[2]),
            shared_cluster(600)]


def mixed_batch(reverse=False):
    parts = mixed_parts()
    return pack(parts[::-1] if reverse else parts)


N_TINY = 3000


@functools.lru_cache(maxsize=None)
def tiny_batch():
    """3 000 structures of 1 to 4 atoms within 1.5 A of each other, labels index % 2 within the structure."""
    rng = np.random.default_rng(41)
    parts = []
    for s in range(N_TINY):
        n = 1 + s % 4
        xyz = (rng.uniform(-40.0, 40.0, (1, 3)) + rng.uniform(0.0, 1.5, (n, 3))).astype(np.float32)
        cols = (xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy(), rng.uniform(1.2, 1.9, n).astype(np.float32),
                np.arange(1, n + 1, dtype=np.uint64))
        parts.append((cols, np.arange(n, dtype=np.uint32) % np.uint32(2)))
    return pack(parts)


# ---- the row-offset scan ----------------------------------------------------------------------------------------

SCAN_SIZES = (262145, 524289)   # chunks of 512 and 768 counts per scan block: two and three tiles
SCAN_KINDS = ("single", "batch")
SCAN_PROBE = 0.0
SCAN_FULL = (262145, "batch", 64)   # the one full call: n, kind, n_points


@functools.lru_cache(maxsize=4)
def scan_case(n, kind):
    """(x, y, z, r, ids, so, labels) of nb_helpers.scan_input, labels index % 3."""
    cols = nh.scan_input(n, kind)
    return cols + (np.arange(n, dtype=np.uint32) % np.uint32(3),)
