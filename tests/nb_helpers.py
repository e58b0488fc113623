"""Shared helpers of the neighbour-list tests: the oracle's lists in the engine's CSR form and order, comparisons and
the invariants every result must hold.  The oracle keeps push order on distance ties (its insertion sort); the
engine's documented order is (d^2, idx), one of the orders the reference's sort_unstable_by may give, so the oracle's
lists are re-sorted by (d^2, idx) with a stable sort before a comparison.  Plain helper module (not a conftest)."""
import numpy as np

import bench_workloads as bw
from oracle import pyoracle as po

PROBE = 1.4


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def fold_max(r):
    """fold(0.0, f32::max) of the radii (lib.rs:259-262): NaN radii are skipped."""
    r = _f32(r)
    r = r[~np.isnan(r)]
    return float(max(np.float32(0.0), np.max(r, initial=np.float32(0.0))))


def sorted_lists(lists, x, y, z, centre_of=None):
    """Each list re-sorted by (d^2, idx), d^2 the centre-relative key of spatial_grid.rs:452-462 in f32."""
    x, y, z = _f32(x), _f32(y), _f32(z)
    out = []
    for a, lst in enumerate(lists):
        c = a if centre_of is None else centre_of[a]
        j = lst["idx"].astype(np.int64)
        dx, dy, dz = x[c] - x[j], y[c] - y[j], z[c] - z[j]
        d2 = dx * dx + dy * dy + dz * dz
        assert d2.dtype == np.float32
        out.append(lst[np.lexsort((lst["idx"], d2))])
    return out


def csr(lists):
    from neighbor_model import NEIGHBOR_DTYPE
    offs = np.zeros(len(lists) + 1, np.uint64)
    offs[1:] = np.cumsum([len(lst) for lst in lists], dtype=np.uint64)
    ent = np.concatenate([lst.astype(NEIGHBOR_DTYPE) for lst in lists]) if lists else np.zeros(0, NEIGHBOR_DTYPE)
    return offs, ent


def sorted_csr(offs, ent, x, y, z, centre_of=None):
    """sorted_lists on a whole CSR at once (the same order, for lists of many atoms)."""
    x, y, z = _f32(x), _f32(y), _f32(z)
    n = len(offs) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(offs.astype(np.int64)))
    c = rows if centre_of is None else np.asarray(centre_of, np.int64)[rows]
    j = ent["idx"].astype(np.int64)
    dx, dy, dz = x[c] - x[j], y[c] - y[j], z[c] - z[j]
    with np.errstate(over="ignore"):  # (far pairs under a huge max_radius: d^2 = +inf)
        d2 = dx * dx + dy * dy + dz * dz
    assert d2.dtype == np.float32 and not np.isnan(d2).any()
    # d^2 >= 0 and never NaN in a list: its bits order like the numbers, so (d^2, idx) is one 64-bit key
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ent["idx"].astype(np.uint64)
    return offs, ent[np.lexsort((key, rows))]


def oracle_csr(x, y, z, r, ids, probe=PROBE, max_radius=None, **kw):
    if max_radius is None:
        max_radius = fold_max(r)
    lists = po.neighbor_lists(x, y, z, r, ids, probe_radius=probe, max_radius=max_radius, **kw)
    offs, ent = csr(lists)
    return sorted_csr(offs, ent, x, y, z)


def oracle_active_csr(x, y, z, r, ids, act, probe=PROBE, max_radius=None):
    """The reference bins only the active atoms: the oracle on the gathered subset, idx mapped back."""
    act = np.asarray(act, np.uint32)
    gi = None if ids is None else ids[act]
    gx, gy, gz, gr = x[act], y[act], z[act], r[act]
    lists = po.neighbor_lists(gx, gy, gz, gr, gi, probe_radius=probe,
                              max_radius=fold_max(gr) if max_radius is None else max_radius)
    offs, ent = csr(lists)
    ent = ent.copy()
    ent["idx"] = act[ent["idx"]]
    return sorted_csr(offs, ent, x, y, z, centre_of=act)


def oracle_batch_csr(x, y, z, r, ids, so, probe=PROBE, max_radius=None):
    """The batch call's expected result: each structure on its own (max_radius None: its own maximum), idx relative to
    the structure, offsets batch-global."""
    offs, ents, base = [np.zeros(1, np.uint64)], [], 0
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        o, en = oracle_csr(x[b:e], y[b:e], z[b:e], r[b:e], None if ids is None else ids[b:e], probe, max_radius)
        offs.append(o[1:] + np.uint64(base))
        ents.append(en)
        base += len(en)
    from neighbor_model import NEIGHBOR_DTYPE
    return np.concatenate(offs), np.concatenate(ents) if ents else np.zeros(0, NEIGHBOR_DTYPE)


def assert_same(got, want):
    go, ge = got
    wo, we = want
    assert np.array_equal(go, wo)
    assert ge.tobytes() == we.tobytes()


def check_invariants(got, sizes):
    """offsets[0] == 0, non-decreasing, offsets[-1] == len(entries); every idx below its structure's size (`sizes`:
    one size per list, or one int for all)."""
    offs, ent = got
    assert offs.dtype == np.uint64 and offs[0] == 0
    assert np.all(np.diff(offs.astype(np.int64)) >= 0)
    assert int(offs[-1]) == len(ent)
    lim = np.repeat(np.broadcast_to(np.asarray(sizes, np.int64), (len(offs) - 1,)), np.diff(offs.astype(np.int64)))
    assert np.all(ent["idx"].astype(np.int64) < lim)


def protor(name):
    xyz, r, _, ids = bw.fixture_soa(name)
    x, y, z = (np.ascontiguousarray(xyz[:, k]).astype(np.float32) for k in range(3))
    return x, y, z, _f32(r), ids


def tight_cluster(n, seed, protein="1jcd.pdb", shared_ids=False):
    """`protein` plus an isolated cluster of n atoms inside a ball of radius 0.6 A, 200 A beyond the protein, the first
    min(n, 8) coincident.  Every cluster atom's list is the n - 1 others (distinct ids): d <= 1.2 A is inside every
    cutoff and the ball is smaller than a cell.  shared_ids: the first third of the cluster shares one id, so the id
    rule removes entries inside lists that are still long.  Returns the columns and the cluster's first index."""
    x, y, z, r, ids = protor(protein)
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = d * (0.6 * rng.uniform(0, 1, (n, 1)) ** (1 / 3)) + np.array([x.max() + 200.0, y.mean(), z.mean()])
    c = c.astype(np.float32)
    c[:min(n, 8)] = c[0]
    cid = np.arange(10 ** 6, 10 ** 6 + n, dtype=np.uint64)
    if shared_ids:
        cid[:n // 3] = cid[0]
    cr = rng.uniform(1.2, 1.9, n).astype(np.float32)
    cat = lambda a, b: np.ascontiguousarray(np.concatenate([a, b]))  # noqa: E731
    return (cat(x, c[:, 0]), cat(y, c[:, 1]), cat(z, c[:, 2]), cat(r, cr), cat(ids, cid)), len(x)


SCAN_BLOCKS = 1024  # k_nb_scan_*: 1 024 blocks, chunks of a multiple of 256 counts


def scan_chunk(n):
    """Counts per scan block for n atoms (nb_scan_range)."""
    chunk = (n + SCAN_BLOCKS - 1) // SCAN_BLOCKS
    return (chunk + 255) // 256 * 256


def scan_input(n, kind):
    """n atoms: one jittered lattice (single) or a proteome-like batch cut to exactly n atoms."""
    if kind == "single":
        b = bw.synthetic_uniform(n, seed=n % 997)
        return b.x, b.y, b.z, b.radius, b.ids, np.array([0, n], np.uint32)
    b = bw.synthetic_proteome(200, seed=6)
    reps = -(-n // b.n_atoms)
    so = [0]
    for _ in range(reps):
        so += [int(o) + so[-1] for o in b.structure_offsets[1:]]
    so = np.array([o for o in so if o < n] + [n], np.uint32)
    tile = lambda a: np.ascontiguousarray(np.tile(a, reps)[:n])  # noqa: E731
    return tile(b.x), tile(b.y), tile(b.z), tile(b.radius), tile(b.ids), so
