"""Host-memory entry points at their routing limits, against the oracle bit for bit.

Calls that hand over host memory pick a path by size, and every path has host code of its own that decides values
without ever raising an error when it is wrong (rustsasa_amd/csrc/host_batch.cpp, combine.cpp):

  * the small path (run_small_host_batch) takes up to kSmallAtoms = 32 768 atoms in up to kSmallStructures = 256
    structures; the host computes bounds and grids itself (small_structure_grid / small_grid restate k_bounds /
    make_grid).  32 768 is also kMxMinAtoms: exactly 32 768 atoms is the one size at which the small path runs
    k_occlusion_mx - without the device's id check, on folded ids;
  * one structure of up to kSingleAtoms = 8 192 atoms is read from pinned memory with no upload, and a pinned defer
    flag decides whether the general kernel runs;
  * the call combiner merges per-structure calls of up to 32 768 atoms into blocks of up to 196 608 atoms;
  * trajectories are cut into chunks of max(1, 2^25 / n_atoms) frames; residue offsets that do not cover every atom
    get a gap entry per frame that a 2-D copy leaves behind.

Every value is compared with the oracle (oracle/pyoracle.py) at the same lane count, probe and point count.  Where a
route can be observed it is asserted: a context created with RSASA_SMALL_PATH=0 (read under RSASA_TUNING=1) runs the
general path, and with rising ids a batch of 32 768 atoms or more that reaches the general path adds one to
ids_dropped() (its device id check finds the ids rising), while the small path never runs that check.  Below 32 768
atoms the general path keeps 64-bit ids without a check too, so there the two routes look alike and only the values
are compared; the docstrings name the limit that sends each case where it goes.
"""
import os
import threading

import numpy as np
import pytest

import bench_workloads as bw
import tie_cases as tc
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

PROBE = 1.4
SMALL_ATOMS = 32768       # host_batch.cpp kSmallAtoms (= kMxMinAtoms, occlusion.hip)
SMALL_STRUCTURES = 256    # host_batch.cpp kSmallStructures
SINGLE_ATOMS = 8192       # host_batch.cpp kSingleAtoms
WINDOW_CELLS = 36864      # device_types.h kWindowCells: small_grid takes at most 64 windows
CHUNK_ATOMS = 32 << 20    # rsasa_calculate_sasa_trajectory: chunks of max(1, 2^25 / n_atoms) frames


# ---- builders ---------------------------------------------------------------------------------------------------------

def _context(small_path: bool):
    """A fresh context on GPU 0 that runs the small path (the default) or never does (RSASA_SMALL_PATH=0)."""
    import rustsasa_amd
    old = os.environ.get("RSASA_SMALL_PATH")
    os.environ["RSASA_SMALL_PATH"] = "1" if small_path else "0"
    try:
        return rustsasa_amd.Context(0)
    finally:
        if old is None:
            del os.environ["RSASA_SMALL_PATH"]
        else:
            os.environ["RSASA_SMALL_PATH"] = old


@pytest.fixture(scope="module")
def ctxs():
    small, general = _context(True), _context(False)
    yield small, general
    small.close()
    general.close()


@pytest.fixture(scope="module")
def prot():
    return bw.synthetic_proteome(40, seed=19)


def _oracle(x, y, z, r, ids, so, probe=PROBE, n_points=100):
    if len(so) == 2:
        return po.calculate_sasa_internal(x, y, z, r, ids, probe, n_points, 8, threads=0)
    return po.calculate_sasa_batch(x, y, z, r, ids, so, probe, n_points, 8, threads=0)


def _rising(so):
    """1, 2, ... within every structure (what the reader hands over for a PDB file)."""
    so = np.asarray(so, np.int64)
    sizes = np.diff(so)
    return (np.arange(so[-1]) - np.repeat(so[:-1], sizes) + 1).astype(np.uint64)


def _hashed(n, rng):
    """Distinct 64-bit ids in no order (hashes, as SASAOptions::process passes them)."""
    ids = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64, endpoint=False)
    assert len(np.unique(ids)) == n
    return ids


def _pair_that_matters(x, y, z, r, rng, probe=PROBE, n_points=100):
    """Atoms (i, j) of one structure, j the nearest neighbour of i, such that one id for both changes the oracle's value
    of i or j.  Decided on the atoms within 12 A of i: every atom whose sphere can touch i's or j's is among them."""
    xyz = np.stack([x, y, z], 1).astype(np.float64)
    for i in rng.permutation(len(x))[:32]:
        d2 = np.sum((xyz - xyz[i]) ** 2, 1)
        if not np.isfinite(d2[i]):
            continue
        near = np.flatnonzero(d2 <= 144.0)
        d2[i] = np.inf
        j = int(np.argmin(d2))
        if j not in near:
            continue
        pi, pj = int(np.searchsorted(near, i)), int(np.searchsorted(near, j))
        sub = [np.ascontiguousarray(a[near]) for a in (x, y, z, r)]
        ids = np.arange(len(near), dtype=np.uint64)
        base = po.calculate_sasa_internal(*sub, ids, probe, n_points, 8)
        ids[pj] = ids[pi]
        dup = po.calculate_sasa_internal(*sub, ids, probe, n_points, 8)
        if base[pi] != dup[pi] or base[pj] != dup[pj]:
            return int(i), j
    raise AssertionError("no neighbour pair whose shared id changes a value")


def _id_sets(so, pair, rng):
    """rising ids, hashed ids, the hashed ids with atoms i, j of `pair` given one id, the hashed ids with i, j given
    different ids whose 32-bit folds (device_utils.h fold_id) are equal, and no ids."""
    n = int(so[-1])
    i, j = pair
    hashed = _hashed(n, rng)
    dup = hashed.copy()
    dup[j] = dup[i]
    col = hashed.copy()
    col[j] = np.uint64(tc.colliding_id(int(hashed[i]), (int(hashed[i]) >> 32) ^ 0x5BD1E995))
    assert col[j] != col[i] and tc.fold_id(int(col[j])) == tc.fold_id(int(col[i])) and len(np.unique(col)) == n
    return {"rising": _rising(so), "hashed": hashed, "duplicate": dup, "colliding": col, "none": None}


def _check_id_sets(wants):
    """The duplicate pair changes a value; the colliding pair does not (its ids differ): a kernel that took equal folds
    for equal ids would give the duplicate's values."""
    assert not np.array_equal(wants["duplicate"], wants["hashed"])
    assert np.array_equal(wants["colliding"], wants["hashed"])


def _cut(so, n_structures, rng):
    """The structures of offsets `so` cut further at random atoms until there are n_structures of them (a piece of a
    structure is no larger than the structure: its grid stays within the small path's windows)."""
    n = int(so[-1])
    free = np.setdiff1d(np.arange(1, n), so)
    extra = rng.choice(free, n_structures - (len(so) - 1), replace=False)
    return np.union1d(so, extra).astype(np.uint32)


def _ragged_residues(prot, n):
    """The proteome's residue offsets within n atoms, without the first and last few residues, with two empty
    residues (a repeated offset) in between."""
    ro = prot.residue_offsets[prot.residue_offsets <= n][3:-4].astype(np.uint32)
    ro = np.insert(ro, [7, len(ro) // 2], ro[[7, len(ro) // 2]])
    assert ro[0] > 0 and ro[-1] < n and np.any(np.diff(ro.astype(np.int64)) == 0)
    return ro


# ---- 1. small-path limits -------------------------------------------------------------------------------------------

def _limit_batch(prot, n, n_structures, rng):
    """n atoms of the proteome; n_structures None: the proteome's own structures (the last one cut at n)."""
    so = np.append(prot.structure_offsets[prot.structure_offsets < n], np.uint32(n)).astype(np.uint32)
    if n_structures is not None:
        so = _cut(so, n_structures, rng)
    cols = [np.ascontiguousarray(a[:n]) for a in (prot.x, prot.y, prot.z, prot.radius)]
    return cols, so


@pytest.mark.parametrize("n,n_structures,small", [
    (SMALL_ATOMS - 1, None, True),
    (SMALL_ATOMS, None, True),
    (SMALL_ATOMS + 1, None, False),
    (SMALL_ATOMS, SMALL_STRUCTURES, True),
    (SMALL_ATOMS, SMALL_STRUCTURES + 1, False),
])
def test_small_path_atom_and_structure_limits(ctxs, prot, n, n_structures, small):
    """Batches on both sides of kSmallAtoms and kSmallStructures (run_small_host_batch: S > 256 or N > 32 768 is the
    general path's), each with rising ids, hashed ids, a duplicate pair, a colliding-fold pair and no ids, and residue
    offsets that skip the first and last atoms and hold empty residues.  Exactly 32 768 atoms is the one size at which
    the small path runs k_occlusion_mx (kMxMinAtoms), with ids_check = 0 and folded ids only: a collision of folds falls
    back to the full ids.  The route is asserted through ids_dropped() with rising ids: the small path leaves it alone,
    the general path at 32 768 atoms or more adds one; at 32 767 both leave it alone (the per-atom kernels keep their
    ids unchecked)."""
    small_ctx, general_ctx = ctxs
    rng = np.random.default_rng(n + 7 * (n_structures or 0))
    (x, y, z, r), so = _limit_batch(prot, n, n_structures, rng)
    assert len(so) - 1 == (n_structures or len(so) - 1) and so[-1] == n
    s = int(np.argmax(np.diff(so.astype(np.int64))))
    b, e = int(so[s]), int(so[s + 1])
    pair = tuple(b + k for k in _pair_that_matters(x[b:e], y[b:e], z[b:e], r[b:e], rng))
    ro = _ragged_residues(prot, n)
    drops_general = 1 if n >= SMALL_ATOMS else 0
    drops = {id(small_ctx): 0 if small else drops_general, id(general_ctx): drops_general}
    wants = {}
    for name, ids in _id_sets(so, pair, rng).items():
        want = wants[name] = _oracle(x, y, z, r, ids, so)
        for c in (small_ctx, general_ctx):
            d0 = c.ids_dropped()
            atom, res = c.calculate_sasa_batch(x, y, z, r, ids, so, PROBE, 100, residue_offsets=ro)
            assert np.array_equal(atom, want), (name, c is small_ctx, int(np.sum(atom != want)))
            assert np.array_equal(res, po.residue_sums(want, ro)), (name, c is small_ctx)
            if name == "rising":
                assert c.ids_dropped() - d0 == drops[id(c)], ("route", c is small_ctx)
    _check_id_sets(wants)


@pytest.mark.parametrize("n", [SINGLE_ATOMS, SINGLE_ATOMS + 1])
def test_single_structure_limit(ctxs, n):
    """One structure of kSingleAtoms atoms (read from pinned memory, no upload: small_run's `single`) and one of a single
    atom more (the one-upload small path), through the column entry point with every id set and through the AoS entry
    (calculate_sasa_internal), on the small path and on the general path.  Below 32 768 atoms the routes cannot be told
    apart from outside: the values are compared."""
    import rustsasa_amd
    small_ctx, general_ctx = ctxs
    rng = np.random.default_rng(n)
    xyz, r, _ = bw.synthetic_structure(n + 400, rng)
    x, y, z = (np.ascontiguousarray(xyz[:n, k]) for k in range(3))
    r = np.ascontiguousarray(r[:n])
    so = np.array([0, n], np.uint32)
    wants = {}
    for name, ids in _id_sets(so, _pair_that_matters(x, y, z, r, rng), rng).items():
        want = wants[name] = _oracle(x, y, z, r, ids, so)
        for c in (small_ctx, general_ctx):
            got = c.calculate_sasa_soa(x, y, z, r, ids, PROBE, 100)
            assert np.array_equal(got, want), (name, c is small_ctx, int(np.sum(got != want)))
            if ids is not None:
                got = c.calculate_sasa_internal(rustsasa_amd.make_atoms(x, y, z, r, ids), PROBE, 100)
                assert np.array_equal(got, want), ("AoS", name, c is small_ctx)
    _check_id_sets(wants)


# ---- 2. host bounds equal device bounds ---------------------------------------------------------------------------

def _edge_structures():
    """Structures of 400 atoms each at the values where small_structure_grid (fminf / fmaxf on the host) and k_bounds
    (ordered-int atomics) could differ, or where the host's odd_radii bit changes."""
    out = {}
    xyz, radius, _, _ = bw.fixture_soa("1jcd.pdb")

    def piece(k):  # 400 atoms of one compact protein
        sl = slice(100 * k, 100 * k + 400)
        return [np.ascontiguousarray(xyz[sl, c], dtype=np.float32) for c in range(3)] + [radius[sl].copy()]

    for order in ("-0 first", "+0 first"):
        x, y, z, r = piece(1)
        x -= x.min()                            # +0.0 at the minimum of x, the maximum of y, the minimum of z ...
        y -= y.max()
        z -= z.min()
        neg, pos = (3, 5) if order == "-0 first" else (5, 3)
        x[neg], x[pos] = np.float32(-0.0), np.float32(0.0)   # ... and -0.0 beside it, in either order
        y[neg + 10], y[pos + 10] = np.float32(-0.0), np.float32(0.0)
        z[neg + 20] = np.float32(-0.0)
        assert np.signbit(x[neg]) and not np.signbit(x[pos]) and x.min() == 0.0 and y.max() == 0.0 and z.min() == 0.0
        out["signed zeros, " + order] = (x, y, z, r)
    x, y, z, r = piece(2)
    r = -r
    r[57] = -r[57]
    out["all radii negative but one"] = (x, y, z, r)
    for name, v in (("radius 64", np.float32(64.0)), ("radius above 64", np.nextafter(np.float32(64.0), np.float32(np.inf)))):
        x, y, z, r = piece(3)
        r[200] = v
        out[name] = (x, y, z, r)
    for sign in (1.0, -1.0):
        big = np.float32(sign * 1e8)
        x, y, z, r = piece(4)
        x = (x.astype(np.float64) - (x.max() if sign > 0 else x.min()) + float(big)).astype(np.float32)
        assert (np.max(np.abs(x)) == np.float32(1e8)) and np.sum(np.abs(x) == np.float32(1e8)) >= 1
        out[f"coordinate at {sign * 1e8:+.0e}"] = (x, y, z, r)
        x2 = x.copy()
        x2[int(np.argmax(np.abs(x2)))] = np.nextafter(big, np.float32(sign * np.inf))
        out[f"coordinate beyond {sign * 1e8:+.0e}"] = (x2, y, z, r)
    return out


@pytest.mark.parametrize("probe", [PROBE, 0.0])
def test_host_bounds_equal_device_bounds(ctxs, prot, probe):
    """Each edge structure alone (the single-structure path) and all of them in one batch of exactly 32 768 atoms (the
    small path's largest batch, the matrix-core kernel with the host's odd_radii bits: negative radii, radii above 64
    and coordinates beyond 1e8 must reach the general kernel), on the small path and with RSASA_SMALL_PATH=0, at probe
    1.4 and probe 0.  Rising ids: the batch's route shows in ids_dropped()."""
    small_ctx, general_ctx = ctxs
    edges = _edge_structures()
    for name, (x, y, z, r) in edges.items():
        ids = np.arange(1, len(x) + 1, dtype=np.uint64)
        want = _oracle(x, y, z, r, ids, np.array([0, len(x)], np.uint32), probe)
        for c in (small_ctx, general_ctx):
            got = c.calculate_sasa_soa(x, y, z, r, ids, probe, 100)
            assert np.array_equal(got, want, equal_nan=True), (name, probe, c is small_ctx, int(np.sum(got != want)))
    # the edge structures, then the proteome's structures up to 32 768 atoms
    cols = [list(v) for v in zip(*edges.values())]
    n_edge = sum(len(v) for v in cols[0])
    fill = SMALL_ATOMS - n_edge
    cols = [np.concatenate(c + [a[:fill]]) for c, a in zip(cols, (prot.x, prot.y, prot.z, prot.radius))]
    sizes = [len(v[0]) for v in edges.values()]
    so_fill = np.append(prot.structure_offsets[prot.structure_offsets < fill], np.uint32(fill))
    so = np.concatenate([[0], np.cumsum(sizes), n_edge + so_fill[1:]]).astype(np.uint32)
    assert so[-1] == SMALL_ATOMS and len(so) - 1 <= SMALL_STRUCTURES
    x, y, z, r = cols
    ids = _rising(so)
    want = _oracle(x, y, z, r, ids, so, probe)
    for c, drops in ((small_ctx, 0), (general_ctx, 1)):
        d0 = c.ids_dropped()
        atom, _ = c.calculate_sasa_batch(x, y, z, r, ids, so, probe, 100)
        assert np.array_equal(atom, want, equal_nan=True), (probe, c is small_ctx, int(np.sum(atom != want)))
        assert c.ids_dropped() - d0 == drops, ("route", probe, c is small_ctx)


def test_cell_size_zero_or_subnormal_is_handed_over_with_the_device_status(ctxs):
    """probe + largest radius that is zero or subnormal: small_grid refuses a cell size whose reciprocal is not finite and
    hands the structure to the general path, which must report what the device batch path reports for the same atoms.
    A subnormal cell size whose reciprocal is finite (coincident atoms: a grid of a few cells) is the small path's own
    and must still agree with the device path - and with the oracle, where the call succeeds."""
    import torch
    import rustsasa_amd
    small_ctx, general_ctx = ctxs
    dev = torch.device("cuda:0")
    n = 50
    rng = np.random.default_rng(5)
    spread = rng.uniform(0, 10, size=(n, 3)).astype(np.float32)
    cases = {
        "zero": (spread, np.zeros(n, np.float32)),
        "subnormal, infinite reciprocal": (spread, np.where(np.arange(n) == 3, np.float32(1e-40), np.float32(0.0))),
        "subnormal, finite reciprocal, spread atoms": (spread, np.where(np.arange(n) == 3, np.float32(3e-39), np.float32(0.0))),
        "subnormal, finite reciprocal, coincident atoms": (np.zeros((n, 3), np.float32), np.full(n, np.float32(3e-39))),
    }
    ref = bw.synthetic_structure(300, rng)
    rx, ry, rz = (np.ascontiguousarray(ref[0][:, k]) for k in range(3))
    r_ok = np.ascontiguousarray(ref[1])
    want_ok = _oracle(rx, ry, rz, r_ok, None, np.array([0, len(rx)], np.uint32))

    def status(f):
        try:
            return 0, f()
        except rustsasa_amd.RsasaError as e:
            return e.status, None

    for name, (xyz, r) in cases.items():
        x, y, z = (np.ascontiguousarray(xyz[:, k]) for k in range(3))
        so = np.array([0, n], np.uint32)

        def device_run():
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
            out = torch.full((n,), -1.0, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            general_ctx.enqueue_device(t(x), t(y), t(z), t(r), None, so, out, probe_radius=0.0, n_points=100,
                                       stream=torch.cuda.current_stream().cuda_stream)
            general_ctx.wait()
            return out.cpu().numpy()

        s_dev, v_dev = status(device_run)
        for c in (small_ctx, general_ctx):
            s, v = status(lambda: c.calculate_sasa_soa(x, y, z, r, None, 0.0, 100))
            assert s == s_dev, (name, c is small_ctx, s, s_dev)
            if s == 0:
                assert np.array_equal(v, v_dev, equal_nan=True), (name, c is small_ctx)
            assert np.array_equal(c.calculate_sasa_soa(rx, ry, rz, r_ok, None, PROBE, 100), want_ok)
        if s_dev == 0:
            assert np.array_equal(v_dev, _oracle(x, y, z, r, None, so, 0.0), equal_nan=True), name
        elif name.startswith("zero") or "infinite" in name:
            assert s_dev == rustsasa_amd._capi.RSASA_ERR_INVALID_ARGUMENT, (name, s_dev)


def _boxed_structure(dims, rng):
    """One structure whose grid is exactly dims[0] x dims[1] x dims[2] cells: probe 0.5 and largest radius 1.5 make the
    cell 2.0 (reciprocal 0.5, exact), and atoms at 0 and at 2 D - 6 on each axis make ceil((L + 4) / 2) + 1 = D.
    Two protein pieces (one at each end of the box, so that the first and the last windows see neighbours) and
    sparse atoms between them."""
    ext = np.array([2.0 * d - 6.0 for d in dims])
    piece, pr, _, _ = bw.fixture_soa("1jcd.pdb")
    piece = piece - piece.min(0)
    assert np.all(piece.max(0) < ext - 2.0)
    far = ext - 1.0 - piece.max(0) + piece
    sparse = rng.uniform(0, 1, size=(1000, 3)) * ext
    xyz = np.concatenate([[np.zeros(3), ext], piece + 1.0, sparse, far]).astype(np.float32)
    pr = np.minimum(pr, np.float32(1.5))
    r = np.concatenate([[1.5, 1.5], pr, rng.uniform(1.2, 1.5, 1000), pr]).astype(np.float32)
    assert xyz.min() == 0.0 and np.array_equal(xyz.max(0), ext.astype(np.float32))
    return [np.ascontiguousarray(xyz[:, k]) for k in range(3)] + [r]


@pytest.mark.parametrize("dims,windows", [((48, 48, 64), 4), ((48, 48, 65), 5), ((128, 128, 144), 64),
                                          ((128, 128, 145), 65)])
def test_grid_windows_at_the_small_path_limit(ctxs, dims, windows):
    """Grids of exactly 4 windows of 36 864 cells (the single-structure call's work list fits run_small_host_batch's
    win1[4]), 5 windows (it spills into the vector), exactly 64 windows = 64 * kWindowCells cells (the largest grid
    small_grid takes) and one z layer more (nc > 64 * kWindowCells: the general path).  The cell count is confirmed
    through a timed run (timing on: the general path reports n_cells).  The structure alone, and beside a small
    structure in one batch (S > 1: the work list is always the vector)."""
    import rustsasa_amd
    small_ctx, general_ctx = ctxs
    rng = np.random.default_rng(dims[2])
    x, y, z, r = _boxed_structure(dims, rng)
    n = len(x)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    n_cells = dims[0] * dims[1] * dims[2]
    with rustsasa_amd.Context(0) as t:
        t.enable_timing(True)
        timed = t.calculate_sasa_soa(x, y, z, r, ids, 0.5, 100)
        assert t.timings()["n_cells"] == n_cells
    assert -(-n_cells // WINDOW_CELLS) == windows and (n_cells <= 64 * WINDOW_CELLS) == (windows <= 64)
    want = _oracle(x, y, z, r, ids, np.array([0, n], np.uint32), 0.5)
    assert np.array_equal(timed, want)
    for c in (small_ctx, general_ctx):
        got = c.calculate_sasa_soa(x, y, z, r, ids, 0.5, 100)
        assert np.array_equal(got, want), (dims, c is small_ctx, int(np.sum(got != want)))
    sxyz, sr, _, _ = bw.fixture_soa("1jcd.pdb")
    m = len(sr)
    so = np.array([0, m, m + n], np.uint32)
    cols = [np.concatenate([a, b]).astype(np.float32) for a, b in
            zip((sxyz[:, 0], sxyz[:, 1], sxyz[:, 2], np.minimum(sr, np.float32(1.5))), (x, y, z, r))]
    ids2 = _rising(so)
    want2 = _oracle(*cols, ids2, so, 0.5)
    assert np.array_equal(want2[m:], want)
    for c in (small_ctx, general_ctx):
        atom, _ = c.calculate_sasa_batch(*cols, ids2, so, 0.5, 100)
        assert np.array_equal(atom, want2), (dims, "batch", c is small_ctx)


def test_dense_blob_fires_the_pinned_defer_flag(ctxs):
    """A dense blob of 1 500 atoms through the single-structure call: k_occlusion_fast leaves atoms to the general kernel
    and says so through the pinned defer flag (small_run), which the host reads after the stream has drained.  With
    timing on, the same call takes the general path and reports the deferred atoms; the timing-off run must give the
    same values, and both the oracle's."""
    import rustsasa_amd
    small_ctx, _ = ctxs
    rng = np.random.default_rng(99)
    n = 1500
    blob = rng.normal(scale=4.0, size=(n, 3)).astype(np.float32)
    x, y, z = (np.ascontiguousarray(blob[:, k]) for k in range(3))
    r = rng.uniform(1.2, 2.0, n).astype(np.float32)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    want = _oracle(x, y, z, r, ids, np.array([0, n], np.uint32))
    with rustsasa_amd.Context(0) as t:
        t.enable_timing(True)
        timed = t.calculate_sasa_soa(x, y, z, r, ids, PROBE, 100)
        n_deferred = t.timings()["n_deferred"]
    assert 0 < n_deferred < n
    assert np.array_equal(timed, want)
    got = small_ctx.calculate_sasa_soa(x, y, z, r, ids, PROBE, 100)
    assert np.array_equal(got, want)
    got = small_ctx.calculate_sasa_internal(rustsasa_amd.make_atoms(x, y, z, r, ids), PROBE, 100)
    assert np.array_equal(got, want)


# ---- 3. call combiner with ids that matter -------------------------------------------------------------------------

def test_call_combining_with_ids_that_matter():
    """32 host threads on one shared context (set_call_combining(0)) call with structures of 16 500 to 21 000 atoms:
    every merged block of two calls or more holds more than 32 768 atoms, so k_occlusion_mx runs on the unpacked
    records.  Calls with rising ids, with a duplicate pair, with a colliding-fold pair and without ids are mixed, through
    the column and the AoS entries.  Calls with ids and without must never share a block (Request::same_settings): a
    call's records carry id 0 where it has none, and a block without ids drops its members' ids.  Every call must equal
    the oracle for its own ids, and the counters must show that calls were merged."""
    import rustsasa_amd
    rng = np.random.default_rng(23)
    structs = []
    for n_t in (16500, 18000, 19500, 21000):
        xyz, r, _ = bw.synthetic_structure(n_t + 300, rng)
        x, y, z = (np.ascontiguousarray(xyz[:n_t, k]) for k in range(3))
        r = np.ascontiguousarray(r[:n_t])
        sets = _id_sets(np.array([0, n_t], np.uint32), _pair_that_matters(x, y, z, r, rng), rng)
        sets = {k: sets[k] for k in ("rising", "duplicate", "colliding", "none")}
        wants = {k: _oracle(x, y, z, r, v, np.array([0, n_t], np.uint32)) for k, v in sets.items()}
        assert not np.array_equal(wants["duplicate"], wants["rising"])
        assert np.array_equal(wants["colliding"], wants["rising"])
        structs.append(((x, y, z, r), sets, wants))
    variants = ("rising", "duplicate", "colliding", "none")
    n_threads, n_iter = 32, 10
    errors, done = [], []
    shared = rustsasa_amd.Context(0)
    shared.set_call_combining(0)
    b0, c0 = rustsasa_amd.Context.call_combining_stats(0)

    def work(tid):
        try:
            for it in range(n_iter):
                (x, y, z, r), sets, wants = structs[(tid + 3 * it) % len(structs)]
                v = variants[(tid + it) % len(variants)]
                ids = sets[v]
                if ids is not None and (tid + it) % 3 == 0:
                    got = shared.calculate_sasa_internal(rustsasa_amd.make_atoms(x, y, z, r, ids), PROBE, 100)
                else:
                    got = shared.calculate_sasa_soa(x, y, z, r, ids, PROBE, 100)
                if not np.array_equal(got, wants[v]):
                    errors.append((tid, it, v, int(np.sum(got != wants[v]))))
            done.append(tid)
        except Exception as e:  # noqa: BLE001
            errors.append((tid, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(n_threads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in threads), "a combined call hangs"
    b1, c1 = rustsasa_amd.Context.call_combining_stats(0)
    shared.close()
    assert errors == [] and len(done) == n_threads, errors[:8]
    assert c1 - c0 == n_threads * n_iter, "every call is the combiner's (at most 32 768 atoms, finite input)"
    assert b1 - b0 < c1 - c0, f"{c1 - c0} calls in {b1 - b0} batches: nothing was merged"


# ---- 4. trajectories at scale ----------------------------------------------------------------------------------------

def _tiled_residue_sums(atom, ro):
    """Residue sums of every frame of `atom` [F, N] for offsets ro that need not cover the atoms: one residue_sums call
    over all frames with a gap residue between one frame's last offset and the next frame's first."""
    f, n = atom.shape
    offs = (np.arange(f, dtype=np.int64)[:, None] * n + ro.astype(np.int64)[None, :]).ravel()
    sums = po.residue_sums(atom.ravel(), offs.astype(np.uint32))
    return np.append(sums, np.float32(0)).reshape(f, len(ro))[:, :len(ro) - 1]


def test_trajectory_on_the_matrix_core_kernel_with_hashed_ids_and_nan():
    """A topology of about 40 000 atoms in 3 frames (120 000 atoms: k_occlusion_mx), hashed ids, one NaN coordinate in
    frame 1.  Each structure is within the large id table (4 097 .. 55 296 atoms, k_ids_distinct): the distinct hashed
    ids are found distinct there and dropped (a batch that first ran without the tables runs again with them, from
    rsasa_batch_wait), twice; with one duplicate pair every frame keeps its ids.  Every frame against the oracle: the
    NaN frame gets the oracle's values, the other frames are untouched by it."""
    import rustsasa_amd
    rng = np.random.default_rng(41)
    xyz, r, res = bw.synthetic_structure(40000, rng)
    n = len(r)
    assert 40000 <= n <= 55296
    frames = (xyz[None].astype(np.float64) + rng.normal(scale=0.2, size=(3, n, 3))).astype(np.float32)
    frames[1, 1234, 1] = np.nan
    ro = res.astype(np.uint32)
    hashed = _hashed(n, rng)
    i, j = _pair_that_matters(frames[0, :, 0], frames[0, :, 1], frames[0, :, 2], r, rng)
    dup = hashed.copy()
    dup[j] = dup[i]
    wants = {}
    for name, ids in (("hashed", hashed), ("duplicate", dup)):
        wants[name] = np.stack([_oracle(frames[f, :, 0], frames[f, :, 1], frames[f, :, 2], r, ids,
                                        np.array([0, n], np.uint32)) for f in range(3)])
    assert not np.array_equal(wants["duplicate"][0], wants["hashed"][0])
    with rustsasa_amd.Context(0) as c:
        for run, (name, ids, kept, dropped) in enumerate((("hashed", hashed, 0, 1), ("hashed", hashed, 0, 1),
                                                           ("duplicate", dup, 3, 0))):
            d0 = c.ids_dropped()
            atom, rs = c.calculate_sasa_trajectory(frames, r, ids, PROBE, 100, residue_offsets=ro)
            for f in range(3):
                assert np.array_equal(atom[f], wants[name][f], equal_nan=True), (run, name, f)
                assert np.array_equal(rs[f], po.residue_sums(wants[name][f], ro), equal_nan=True), (run, name, f)
            assert (c.ids_kept(), c.ids_dropped() - d0) == (kept, dropped), (run, name)


@pytest.fixture(scope="module")
def seam():
    """A topology of 4 100 atoms in 2^25 // 4 100 + 2 = 8 186 frames (33.6 M atoms, 0.4 GB): the first chunk holds 8 184
    frames, the second two.  Per-frame jitter, so every frame differs."""
    rng = np.random.default_rng(43)
    n = 4100
    xyz, r, res = bw.synthetic_structure(n + 300, rng)
    xyz, r = xyz[:n].astype(np.float32), np.ascontiguousarray(r[:n])
    ro = res[res <= n].astype(np.uint32)
    if ro[-1] != n:
        ro = np.append(ro, np.uint32(n))
    n_frames = CHUNK_ATOMS // n + 2
    frames = np.empty((n_frames, n, 3), np.float32)
    step = 1024
    for f0 in range(0, n_frames, step):
        f1 = min(n_frames, f0 + step)
        frames[f0:f1] = xyz[None] + rng.standard_normal((f1 - f0, n, 3), dtype=np.float32) * np.float32(0.05)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    return frames, r, ids, ro


def test_trajectory_chunk_seam(seam):
    """Frames on both sides of the chunk seam (xyz + f0 * n_atoms * 3, out_atom_sasa + f0 * n_atoms, the residue rows of a
    chunk after the first): all 8 186 frames against calculate_sasa_batch on the same coordinates (structure offsets
    f * n_atoms, a path pinned to the oracle elsewhere), frames 0, 8 183, 8 184 and 8 185 against the oracle itself.  With
    residue offsets that cover the atoms exactly and with offsets that skip atoms at both ends and hold an empty
    residue (a gap entry per frame, removed by the 2-D copy), with and without atom values."""
    import rustsasa_amd
    frames, r, ids, ro_exact = seam
    n_frames, n = frames.shape[:2]
    per_chunk = CHUNK_ATOMS // n
    assert n_frames - per_chunk == 2
    ro_skip = np.insert(ro_exact[2:-3], 6, ro_exact[8]).astype(np.uint32)
    assert ro_skip[0] > 0 and ro_skip[-1] < n and np.any(np.diff(ro_skip.astype(np.int64)) == 0)
    so = (np.arange(n_frames + 1, dtype=np.int64) * n).astype(np.uint32)
    with rustsasa_amd.Context(0) as c:
        ref, _ = c.calculate_sasa_batch(*(frames[:, :, k].ravel() for k in range(3)), np.tile(r, n_frames),
                                        np.tile(ids, n_frames), so, PROBE, 100)
        ref = ref.reshape(n_frames, n)
        picked = (0, per_chunk - 1, per_chunk, per_chunk + 1)
        for f in picked:
            want = _oracle(frames[f, :, 0], frames[f, :, 1], frames[f, :, 2], r, ids, np.array([0, n], np.uint32))
            assert np.array_equal(ref[f], want), f
        assert not np.array_equal(ref[per_chunk], ref[per_chunk + 1])
        for ro_name, ro in (("exact", ro_exact), ("skips both ends", ro_skip)):
            want_res = _tiled_residue_sums(ref, ro)
            for want_atoms in (True, False):
                atom, rs = c.calculate_sasa_trajectory(frames, r, ids, PROBE, 100, residue_offsets=ro,
                                                       want_atoms=want_atoms)
                if want_atoms:
                    bad = np.flatnonzero(np.any(atom != ref, axis=1))
                    assert bad.size == 0, (ro_name, bad[:8])
                else:
                    assert atom is None
                bad = np.flatnonzero(np.any(rs != want_res, axis=1))
                assert bad.size == 0, (ro_name, want_atoms, bad[:8])
                for f in picked:
                    assert np.array_equal(rs[f], po.residue_sums(ref[f], ro)), (ro_name, want_atoms, f)
                del atom, rs


def test_trajectory_input_errors_leave_the_context_working():
    """residue_offsets[-1] > n_atoms and decreasing residue offsets are RSASA_ERR_INVALID_ARGUMENT; an infinite
    coordinate in one frame is the call's error (the grid of that frame overflows: RSASA_ERR_GRID_TOO_LARGE).  After
    each, the same context computes a good trajectory bit for bit."""
    import rustsasa_amd
    from rustsasa_amd import _capi
    xyz, r, res, ids = bw.fixture_soa("1jcd.pdb")
    rng = np.random.default_rng(61)
    n = len(r)
    frames = np.stack([xyz + rng.normal(scale=0.3, size=xyz.shape) for _ in range(3)]).astype(np.float32)
    ro = res.astype(np.uint32)
    wants = [_oracle(frames[f, :, 0], frames[f, :, 1], frames[f, :, 2], r, ids, np.array([0, n], np.uint32))
             for f in range(3)]
    beyond = ro.copy()
    beyond[-1] = n + 1
    falling = ro.copy()
    falling[4], falling[5] = ro[5], ro[4]
    assert falling[4] > falling[5]
    inf_frames = frames.copy()
    inf_frames[1, 17, 2] = np.inf
    bad = ((frames, beyond, _capi.RSASA_ERR_INVALID_ARGUMENT), (frames, falling, _capi.RSASA_ERR_INVALID_ARGUMENT),
           (inf_frames, ro, _capi.RSASA_ERR_GRID_TOO_LARGE))
    with rustsasa_amd.Context(0) as c:
        for k, (fr, offs, status) in enumerate(bad):
            with pytest.raises(rustsasa_amd.RsasaError) as e:
                c.calculate_sasa_trajectory(fr, r, ids, PROBE, 100, residue_offsets=offs)
            assert e.value.status == status, (k, e.value)
            atom, rs = c.calculate_sasa_trajectory(frames, r, ids, PROBE, 100, residue_offsets=ro)
            for f in range(3):
                assert np.array_equal(atom[f], wants[f]), (k, f)
                assert np.array_equal(rs[f], po.residue_sums(wants[f], ro)), (k, f)
