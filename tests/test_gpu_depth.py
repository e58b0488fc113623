"""Atom depth on the GPU (rsasa_atom_depth*, k_atom_depth of depth.hip) against the exact CPU model (depth_model.py: the
header's definition in numpy float32 on the masks of points_model.py).  A minimum has no order, so every comparison is one
of bit patterns: depth as uint32, nearest as it is, free and sasa against the other point calls.  The cases
(depth_cases.py, pinned by test_depth_cpu.py) sit on the kernel's own edges: sweeps of 3, 4, 5 and more shells, a void
under the surface, exact ties, shells clipped at every grid face, structures of 0, 1 and 2 atoms, dots of another
structure in the middle of a ball, and the 32-bit cell starts of a structure of 65 536 atoms."""
import functools

import numpy as np
import pytest

import bench_workloads as bw
import depth_cases as dc
import depth_model as dm
import point_edge_cases as pe
import points_model as pm

pytestmark = pytest.mark.gpu

F = np.float32
POINT_COUNTS = (1, 32, 33, 64, 65, 100, 960)
TAIL_SAMPLE = 512


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _model(name, n_points=100, W=8):
    c = dc.get(name)
    return dm.atom_depth_batch(*c.cols, c.so, c.probe, n_points, W)


def _check(got, want, r, probe, n_points):
    depth, nearest, free, sasa = got
    w_depth, w_nearest, mask = want
    n = len(mask)
    assert depth.dtype == F and nearest.dtype == np.uint32 and free.dtype == np.uint32 and sasa.dtype == F
    assert depth.shape == nearest.shape == free.shape == sasa.shape == (n,)
    bad = np.flatnonzero((dm.bits(depth) != dm.bits(w_depth)) | (nearest != w_nearest))
    assert bad.size == 0, (bad.size, bad[:5], depth[bad[:5]], w_depth[bad[:5]], nearest[bad[:5]], w_nearest[bad[:5]])
    assert np.array_equal(free, mask.sum(axis=1).astype(np.uint32))
    assert sasa.tobytes() == pm.sasa_of(r, probe, free, n_points).tobytes()


# ---- 1: every case against the model ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", dc.SMALL)
def test_cases_equal_the_model(ctx, name):
    c = dc.get(name)
    got = ctx.atom_depth_batch(*c.cols, c.so, c.probe, 100)
    _check(got, _model(name), c.r, c.probe, 100)
    words, sasa = ctx.accessible_points_batch(*c.cols, c.so, c.probe, 100)
    assert np.array_equal(got[2].astype(np.int64), pe.popcount(words)) and got[3].tobytes() == sasa.tobytes()


def test_overlap_batch_equals_the_ball_alone(ctx):
    o, b = dc.get("overlap_batch"), dc.get("ball")
    got = ctx.atom_depth_batch(*o.cols, o.so, o.probe, 100)
    alone = ctx.atom_depth(*b.cols, b.probe, 100)
    for k in range(4):
        assert got[k][:-1].tobytes() == alone[k].tobytes(), k
    assert got[1][-1] == 0 and got[2][-1] == 100                # the lone atom: its own dots, index 0 of its structure


@functools.lru_cache(maxsize=None)
def _tail_reference():
    """(sample, depth, nearest, free) of the tail structure.  The masks of 65 536 atoms take the point model minutes, so
    they are the engine's own (accessible_points_batch, pinned to the oracle at this size by test_gpu_tail_edges.py).
    The sample: atoms with no accessible point (in a structure this sparse the deepest there are), the first and last
    atoms of the cell order and those around eight seams of it, and random ones.  The model evaluates the sample against
    all dots of the structure (depth_model.keys_of_sample_near: the dots that cannot be the nearest are left out by a
    bound, the keys are those of keys_of)."""
    import rustsasa_amd
    import tail_cases as tc
    c = dc.get("tail")
    b, e = int(c.so[-2]), int(c.so[-1])
    with rustsasa_amd.Context(0) as cx:
        words, _ = cx.accessible_points_batch(*c.cols, c.so, c.probe, 100)
    mask = rustsasa_amd.unpack_points(words, 100).astype(bool)[b:e]
    x, y, z, r = (a[b:e] for a in c.cols[:4])
    rng = np.random.default_rng(5)
    buried = np.flatnonzero(~mask.any(axis=1))
    buried = buried[rng.permutation(len(buried))[:192]]
    mn, inv, dims = tc.grid_of(x, y, z, r, c.probe)
    order = np.argsort(tc.cell_index(x, y, z, mn, inv, dims), kind="stable")
    seams = np.concatenate([order[:32], order[-32:],
                            order[np.arange(1, 9)[:, None] * (len(order) // 9) + np.arange(-8, 8)].ravel()])
    fixed = np.unique(np.concatenate([buried, seams]))
    rest = np.setdiff1d(rng.permutation(e - b), fixed, assume_unique=False)
    sample = np.sort(np.concatenate([fixed, rng.permutation(rest)[:TAIL_SAMPLE - len(fixed)]]))
    _, depth, nearest = dm.split(dm.keys_of_sample_near(x, y, z, r, mask, c.probe, 100, sample))
    return sample, depth, nearest, mask.sum(axis=1).astype(np.uint32), len(buried)


def test_tail_structure_on_a_sample(ctx):
    c = dc.get("tail")
    b = int(c.so[-2])
    sample, w_depth, w_nearest, w_free, n_buried = _tail_reference()
    assert len(sample) == TAIL_SAMPLE and len(np.unique(sample)) == TAIL_SAMPLE and np.isfinite(w_depth).all()
    depth, nearest, free, sasa = ctx.atom_depth_batch(*c.cols, c.so, c.probe, 100)
    assert np.array_equal(dm.bits(depth[b:][sample]), dm.bits(w_depth))
    assert np.array_equal(nearest[b:][sample], w_nearest)
    assert np.array_equal(free[b:], w_free) and np.isfinite(depth).all()
    # the small structures in front of it, against the model proper
    for s in range(len(c.so) - 2):
        p = c.part(s)
        w = dm.atom_depth(*p, c.probe, 100)
        lo, hi = int(c.so[s]), int(c.so[s + 1])
        assert np.array_equal(dm.bits(depth[lo:hi]), dm.bits(w[0])) and np.array_equal(nearest[lo:hi], w[1])


# ---- 2: point counts and lane counts -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n_points,W", [(n, 8) for n in POINT_COUNTS] + [(100, 1)])
def test_point_counts_and_widths_on_cavity(ctx, n_points, W):
    c = dc.get("cavity")
    try:
        ctx.set_simd_width(W)
        got = ctx.atom_depth(*c.cols, c.probe, n_points)
        words, sasa = ctx.accessible_points(*c.cols, c.probe, n_points)
    finally:
        ctx.set_simd_width(8)
    _check(got, _model("cavity", n_points, W), c.r, c.probe, n_points)
    assert np.array_equal(got[2].astype(np.int64), pe.popcount(words)) and got[3].tobytes() == sasa.tobytes()


# ---- 3: single and batch, permutation ----------------------------------------------------------------------------------

def test_single_call_equals_batch_call(ctx):
    for name in ("cavity", "twins", "corner"):
        c = dc.get(name)
        one = ctx.atom_depth(*c.cols, c.probe, 100)
        many = ctx.atom_depth_batch(*c.cols, c.so, c.probe, 100)
        for k in range(4):
            assert one[k].tobytes() == many[k].tobytes(), (name, k)
    import rustsasa_amd  # noqa: F401
    e = np.zeros(0, F)
    for so in ([0], [0, 0, 0]):
        got = ctx.atom_depth_batch(e, e, e, e, np.zeros(0, np.uint64), np.array(so, np.uint32), 1.4, 100)
        assert all(len(a) == 0 for a in got)
    assert all(len(a) == 0 for a in ctx.atom_depth(e, e, e, e, None, 1.4, 100))


def test_a_permutation_of_the_atoms_permutes_the_result(ctx):
    c = dc.get("cavity")
    w_depth, w_nearest, mask = _model("cavity")
    # no ties between atoms in this case
    owner, qx, qy, qz = dm.dots_of(*c.cols[:4], mask, c.probe, 100)
    for i in range(c.n_atoms):
        d2 = (c.x[i] - qx) * (c.x[i] - qx) + (c.y[i] - qy) * (c.y[i] - qy) + (c.z[i] - qz) * (c.z[i] - qz)
        first = owner[d2 == d2.min()]
        assert first.min() == first.max(), i                    # the smallest d2 belongs to one atom
    perm = np.random.default_rng(3).permutation(c.n_atoms)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(c.n_atoms)
    base = ctx.atom_depth(*c.cols, c.probe, 100)
    got = ctx.atom_depth(*(a[perm] for a in c.cols), c.probe, 100)
    assert got[0].tobytes() == base[0][perm].tobytes()
    assert np.array_equal(got[1], inv[base[1][perm]].astype(np.uint32))
    assert np.array_equal(got[2], base[2][perm]) and got[3].tobytes() == base[3][perm].tobytes()


# ---- 4: one context, other families, a batch in flight -----------------------------------------------------------------

def test_between_the_other_families_and_beside_a_batch_in_flight(ctx):
    torch = pytest.importorskip("torch")
    c, t = dc.get("cavity"), dc.get("twins")
    want = _model("cavity")
    b = bw.synthetic_proteome(12, seed=4)
    dev = torch.device("cuda", 0)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cols = (tt(b.x), tt(b.y), tt(b.z), tt(b.radius), tt(b.ids.view(np.int64)))
    alone = torch.zeros(b.n_atoms, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.enqueue_device(*cols, b.structure_offsets, out_atom_sasa=alone, probe_radius=1.4, n_points=100)
    ctx.wait()
    words0, _ = ctx.accessible_points(*c.cols, c.probe, 100)
    ex0 = ctx.exposure_vectors(*t.cols, t.probe, 129)
    out = torch.zeros(b.n_atoms, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.enqueue_device(*cols, b.structure_offsets, out_atom_sasa=out, probe_radius=1.4, n_points=100)
    got = ctx.atom_depth(*c.cols, c.probe, 100)
    ctx.wait()
    assert out.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    _check(got, want, c.r, c.probe, 100)
    # the other families through the same buffers, before and after
    nb = ctx.precompute_neighbors(*c.cols, c.probe)
    ex1 = ctx.exposure_vectors(*t.cols, t.probe, 129)
    words1, _ = ctx.accessible_points(*c.cols, c.probe, 100)
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(ex0, ex1)) and words0.tobytes() == words1.tobytes()
    assert len(nb[0]) == c.n_atoms + 1
    _check(ctx.atom_depth(*c.cols, c.probe, 100), want, c.r, c.probe, 100)
    tw = ctx.atom_depth(*t.cols, t.probe, 960)
    _check(tw, _model("twins", 960), t.r, t.probe, 960)


# ---- 5: argument errors and non-finite input ---------------------------------------------------------------------------

def test_argument_errors_from_the_library(ctx):
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    lib = _capi.load()
    c = dc.get("corner")
    x, y, z, r, ids = c.cols
    n = c.n_atoms
    d, k = np.zeros(n, F), np.zeros(n, np.uint32)
    cols = (ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids))
    bad = _capi.RSASA_ERR_INVALID_ARGUMENT
    assert lib.rsasa_atom_depth(ctx._h, *cols, n, 1.4, 0, ptr(d), ptr(k), None, None) == bad
    assert lib.rsasa_atom_depth(ctx._h, *cols, n, 1.4, 100, None, ptr(k), None, None) == bad
    assert lib.rsasa_atom_depth(ctx._h, *cols, n, 1.4, 100, ptr(d), None, None, None) == bad
    assert lib.rsasa_atom_depth(ctx._h, *cols, n, -5.0, 100, ptr(d), ptr(k), None, None) == bad   # probe + max_r <= 0
    so = np.array([0, n], np.uint32)
    assert lib.rsasa_atom_depth_batch(ctx._h, *cols, ptr(so), 1, 1.4, 0, ptr(d), ptr(k), None, None) == bad
    assert lib.rsasa_atom_depth_batch(ctx._h, *cols, ptr(so), 1, 1.4, 100, None, ptr(k), None, None) == bad
    assert lib.rsasa_atom_depth_batch(ctx._h, *cols, ptr(so), 1, 1.4, 100, ptr(d), None, None, None) == bad
    assert lib.rsasa_atom_depth_batch(ctx._h, *cols, None, 1, 1.4, 100, ptr(d), ptr(k), None, None) == bad
    down = np.array([0, 40, 30, n], np.uint32)
    assert lib.rsasa_atom_depth_batch(ctx._h, *cols, ptr(down), 3, 1.4, 100, ptr(d), ptr(k), None, None) == bad
    assert not d.any() and not k.any()                     # nothing was written
    # out_free and out_sasa are optional; no atoms is OK; the context is still usable
    assert lib.rsasa_atom_depth(ctx._h, *cols, 0, 1.4, 100, None, None, None, None) == _capi.RSASA_OK
    assert lib.rsasa_atom_depth(ctx._h, *cols, n, 1.4, 100, ptr(d), ptr(k), None, None) == _capi.RSASA_OK
    w = _model("corner")
    assert np.array_equal(dm.bits(d), dm.bits(w[0])) and np.array_equal(k, w[1])


def test_non_finite_input_as_exposure_vectors(ctx):
    import rustsasa_amd
    c = dc.get("corner")
    x, y, z, r, ids = c.cols
    bad = x.copy()
    bad[3] = np.inf
    for call in (lambda: ctx.atom_depth(bad, y, z, r, ids, 1.4, 100), lambda: ctx.exposure_vectors(bad, y, z, r, ids, 1.4, 100),
                 lambda: ctx.atom_depth_batch(bad, y, z, r, ids, c.so, 1.4, 100)):
        with pytest.raises(rustsasa_amd.RsasaError) as e:
            call()
        assert e.value.status == -5
    # NaN is taken, as there: the atom itself has no depth and its dots count for nobody
    xn, rn = x.copy(), r.copy()
    xn[5] = np.nan
    rn[17] = np.nan
    mask = pm.exposed_masks(xn, y, z, rn, ids, 1.4, 100, 8)
    assert mask[5].all() and mask[17].all()
    want = dm.atom_depth(xn, y, z, rn, ids, 1.4, 100, mask=mask)
    got = ctx.atom_depth(xn, y, z, rn, ids, 1.4, 100)
    assert np.array_equal(dm.bits(got[0]), dm.bits(want[0])) and np.array_equal(got[1], want[1])
    assert np.isinf(got[0][5]) and got[1][5] == 0xFFFFFFFF and np.isfinite(got[0][17]) and not (got[1] == 17).any()
    assert np.array_equal(got[2], mask.sum(axis=1).astype(np.uint32))
    _check(ctx.atom_depth(*c.cols, c.probe, 100), _model("corner"), c.r, c.probe, 100)
