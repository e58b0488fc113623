"""Dot crowding on the GPU (rsasa_dot_crowding*, k_dot_crowding of crowding.hip) against the exact CPU model
(crowding_model.py: the header's definition in numpy float32) cell for cell by np.array_equal, and against a second
witness on the GPU itself: radial_counts_batch with the dots appended to every structure as centre-only atoms - another
kernel on another grid.  The cases are crowding_cases.py's (test_crowding_cpu.py pins each to what it is named for)."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import crowding_cases as cc
import crowding_model as cm
import depth_cases as dc
import points_model as pm
import sweep_cases as sc

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


def _run(ctx, c, edges=None, flags="own", n_points=None):
    flags = c.flags if isinstance(flags, str) else flags
    edges = c.edges if edges is None else edges
    n_points = c.n_points if n_points is None else n_points
    if len(c.so) == 2:
        return ctx.dot_crowding(*c.cols, c.probe, n_points, edges, flags)
    return ctx.dot_crowding_batch(*c.cols, c.so, c.probe, n_points, edges, flags)


def _model(c, edges=None, flags="own", W=8):
    flags = c.flags if isinstance(flags, str) else flags
    mask = cc.masks(c, W)
    off, rows = cm.counts_batch(c.x, c.y, c.z, c.r, c.so, mask, c.probe, c.n_points, c.edges if edges is None else edges, flags)
    return off, rows, mask


def _equal(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), [int(got[tuple(b)]) for b in bad[:5]], [int(want[tuple(b)]) for b in bad[:5]])


def _check(ctx, c, edges=None, flags="own"):
    """The call against the model: offsets, rows, free and the values."""
    off, rows, free, sasa = _run(ctx, c, edges, flags)
    w_off, w_rows, mask = _model(c, edges, flags)
    _equal(off, w_off)
    _equal(rows, w_rows)
    want_free = mask.sum(axis=1).astype(np.uint32)
    _equal(free, want_free)
    assert sasa.tobytes() == pm.sasa_of(c.r, c.probe, want_free, c.n_points).tobytes()
    return off, rows, mask


def _witness(ctx, c, off, rows, mask, edges=None):
    """The same table from k_radial_counts with the dots as centre-only atoms."""
    x, y, z, r, so, flags, where = cc.with_dots(c, off, mask)
    r = r.copy()
    r[0] = max(r[0], F(0.5))                 # (some radius must be positive when the probe is 0)
    table = ctx.radial_counts_batch(x, y, z, r, None, so, c.probe, c.edges if edges is None else edges, None, 1, flags)
    _equal(table[where, 0, :], rows)
    assert not table[np.setdiff1d(np.arange(len(x)), where)].any()


# ---- dots per atom -------------------------------------------------------------------------------------------------------

def test_atoms_with_0_1_63_64_and_65_dots(ctx):
    c = cc.caps()
    off, rows, mask = _check(ctx, c)
    assert np.diff(off.astype(np.int64))[c.info["owners"]].tolist() == [0, 1, 63, 64, 65] and rows.any()
    _witness(ctx, c, off, rows, mask)


@pytest.mark.parametrize("n_points", cc.POINT_COUNTS)
def test_corner_at_every_point_count(ctx, n_points):
    c = cc.corner(n_points)
    off, rows, mask = _check(ctx, c)
    assert rows.any(axis=0).all()
    _witness(ctx, c, off, rows, mask)


def test_lone_atom_at_960_points_takes_every_pass(ctx):
    c = cc.lone()
    off, rows, _ = _check(ctx, c)
    assert off.tolist() == [0, 960] and np.array_equal(rows, np.tile(np.array([[0, 1, 0]], np.uint32), (960, 1)))
    _, none, _, _ = _run(ctx, c, flags=np.array([0xFE], np.uint8))        # the owner without its partner bit
    assert none.shape == (960, 3) and not none.any()


def test_pair_at_960_points(ctx):
    c = cc.pair()
    off, rows, mask = _check(ctx, c)
    assert (np.diff(off.astype(np.int64)) > cc.PASS).all() and rows[:, 1:].any(axis=0).all() and not rows[:, 0].any()
    _witness(ctx, c, off, rows, mask)


# ---- exact ties ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", cc.TIE_KINDS)
def test_exact_ties_at_the_edges(ctx, kind):
    c = cc.tie(kind)
    off, rows, mask = _check(ctx, c)
    row = rows[int(mask[0, :cc.TIE_DOT].sum())]
    assert row.tolist() == {"last": [1, 1], "inner": [1, 1, 0], "duplicate": [1, 1, 0, 0], "below": [1, 0]}[kind]
    _witness(ctx, c, off, rows, mask)


@pytest.mark.parametrize("edge0", [0.0, 1e-30])
def test_edge_zero_and_an_edge_whose_square_underflows(ctx, edge0):
    c = cc.tie_zero(edge0)
    off, rows, mask = _check(ctx, c)
    assert rows[cc.TIE_DOT, 0] == 1 and rows[:65, 0].sum() == 1
    _witness(ctx, c, off, rows, mask)


# ---- the stop rule -----------------------------------------------------------------------------------------------------------

def test_tie_partners_in_the_last_swept_shell(ctx):
    c = cc.last_shell()
    off, rows, mask = _check(ctx, c)
    for owner, k, _ in c.info["ties"]:
        assert rows[int(off[owner]) + k, -1] >= 1
    _witness(ctx, c, off, rows, mask)


@pytest.mark.parametrize("reach", cc.REACHES + ("grid",))
def test_reaches_of_two_to_six_shells_and_the_whole_grid(ctx, reach):
    edges = (4.0, cc.COVER) if reach == "grid" else cc.reach_edges(sc.H, reach)
    c = cc.of_depth("cavity", n_points=20, edges=edges)
    off, rows, mask = _check(ctx, c)
    if reach == "grid":
        assert (rows.sum(axis=1) == c.n_atoms).all()                    # everybody lies in some bin of every dot
    _witness(ctx, c, off, rows, mask)


@pytest.mark.parametrize("name", ["column_z", "slant_xp", "slant_xm", "slant_yp", "slant_ym", "margin_under", "margin_over",
                                  "margin_small_h", "margin_large_h", "odd_beside_even", "crowded_cells"])
def test_thin_long_slanted_margin_and_odd_grids(ctx, name):
    d = sc.get(name)
    h = float(F(d.probe) + np.max(d.r[np.isfinite(d.r)]))
    n_points = sc.points_of(name)[0] if name in sc.POINTS else 20
    c = cc.Case(name, d.x, d.y, d.z, d.r, d.so, n_points=n_points, edges=(1.2 * h, 2.7 * h), probe=d.probe)
    _check(ctx, c)


# ---- staging -----------------------------------------------------------------------------------------------------------------

def test_a_cell_of_200_atoms_and_63_64_65_partners(ctx):
    _check(ctx, cc.crowd())
    c = cc.packed()
    off, rows, mask = _check(ctx, c)
    _witness(ctx, c, off, rows, mask)


# ---- flags and bins ----------------------------------------------------------------------------------------------------------

def test_flag_patterns_and_zero_rows_after_a_dense_call(ctx):
    c = cc.of_depth("ball", n_points=33)
    dense = _check(ctx, c)[1]
    assert dense.all(axis=1).any()
    for seed in (1, 2):
        _check(ctx, c, flags=cc.random_flags(c.n_atoms, seed))
    off, rows, free, _ = _run(ctx, c, flags=np.full(c.n_atoms, 0xFE, np.uint8))   # no partner: every row written, as zeros
    assert rows.shape == dense.shape and not rows.any()
    one = np.zeros(c.n_atoms, np.uint8)
    one[5] = 1
    _check(ctx, c, flags=one)


@pytest.mark.parametrize("edges", [(7.0,), (0.0, 2.0, 3.5, 3.5, 5.0, 6.5, 8.0, 11.0)])
def test_one_bin_and_eight(ctx, edges):
    c = cc.of_depth("cavity", n_points=20, edges=edges)
    off, rows, mask = _check(ctx, c)
    assert rows.shape[1] == len(edges)
    _witness(ctx, c, off, rows, mask)


# ---- non-finite input --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["nan_coordinate", "nan_radius"])
def test_a_nan_atom_has_zero_rows_and_counts_for_nobody(ctx, name):
    c = getattr(cc, name)()
    off, rows, mask = _check(ctx, c)
    a = c.info["atom"]
    assert int(off[a + 1] - off[a]) == c.n_points and not rows[int(off[a]):int(off[a + 1])].any() and rows.any()


def test_an_infinite_coordinate_is_refused_and_the_next_call_is_right(ctx):
    import rustsasa_amd
    c = cc.corner(33)
    x = c.x.copy()
    x[3] = np.inf
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.dot_crowding(x, c.y, c.z, c.r, None, c.probe, 33, c.edges)
    assert e.value.status == -5                                          # RSASA_ERR_GRID_TOO_LARGE
    _check(ctx, c)


# ---- batches -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tiny", "overlap_batch"])
def test_small_batches(ctx, name):
    c = cc.of_depth(name, n_points=33, edges=(2.0, 6.0, 14.0))
    off, rows, mask = _check(ctx, c)
    if name == "overlap_batch":
        assert rows[-33:].sum(axis=1).tolist() == [1] * 33               # the lone atom's dots see the lone atom only
    _witness(ctx, c, off, rows, mask)


N_TAIL_SAMPLE = 48
TAIL_POINTS = 12


def test_a_structure_of_65536_atoms_with_32_bit_cell_starts(ctx):
    """Offsets and free against surface_components on the same input, a seeded sample of the big structure's atoms
    against the model, and every row against the radial witness."""
    d = dc.get("tail")
    c = cc.Case("tail", d.x, d.y, d.z, d.r, d.so, n_points=TAIL_POINTS, edges=(5.0, 9.0), probe=d.probe)
    off, rows, free, sasa = _run(ctx, c)
    c_off, _, c_free, c_sasa = ctx.surface_components_batch(*c.cols, c.so, c.probe, TAIL_POINTS, 0.0)
    assert off.tobytes() == c_off.tobytes() and free.tobytes() == c_free.tobytes() and sasa.tobytes() == c_sasa.tobytes()
    words, _ = ctx.accessible_points_batch(*c.cols, c.so, c.probe, TAIL_POINTS)
    mask = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(len(words), -1)[:, :TAIL_POINTS]
    assert np.array_equal(mask.sum(axis=1), free)
    b, e = int(c.so[-2]), int(c.so[-1])
    assert e - b == 65536
    have = np.flatnonzero(free[b:e])
    sample = np.sort(np.random.default_rng(17).permutation(have)[:N_TAIL_SAMPLE])
    from scipy.spatial import cKDTree
    import depth_model as dm
    sub = np.zeros_like(mask[b:e])
    sub[sample] = mask[b:e][sample]
    _, qx, qy, qz = dm.dots_of(c.x[b:e], c.y[b:e], c.z[b:e], c.r[b:e], sub, c.probe, TAIL_POINTS)
    xyz = np.stack([c.x[b:e], c.y[b:e], c.z[b:e]], -1).astype(np.float64)
    tree = cKDTree(xyz)
    want = np.zeros((len(qx), 2), np.uint32)
    for n, near in enumerate(tree.query_ball_point(np.stack([qx, qy, qz], -1).astype(np.float64), 9.2)):
        want[n] = cm.rows_of(qx[n:n + 1], qy[n:n + 1], qz[n:n + 1], c.x[b:e], c.y[b:e], c.z[b:e], np.asarray(near, np.int64),
                             cm.e2_of(c.edges))[0]
    got = np.concatenate([rows[int(off[b + i]):int(off[b + i + 1])] for i in sample])
    _equal(got, want)
    assert got.any(axis=0).all()
    _witness(ctx, c, off, rows, mask)


# ---- identities ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_points", [100, 129])
def test_offsets_free_and_values_are_those_of_the_other_families(ctx, n_points):
    c = cc.of_depth("cavity", n_points=n_points)
    off, rows, free, sasa = _run(ctx, c)
    c_off, labels, c_free, c_sasa = ctx.surface_components(*c.cols, c.probe, n_points)
    words, p_sasa = ctx.accessible_points(*c.cols, c.probe, n_points)
    assert off.tobytes() == c_off.tobytes() and free.tobytes() == c_free.tobytes()
    assert sasa.tobytes() == c_sasa.tobytes() == p_sasa.tobytes() and len(labels) == len(rows)
    assert np.array_equal(free, cc.masks(c).sum(axis=1))
    assert np.array_equal(words, pm.pack(cc.masks(c)))


# ---- protocol ------------------------------------------------------------------------------------------------------------------

def _raw(ctx, c, edges, counts, cap, offsets, n_points=None, flags=None, batch=False):
    from rustsasa_amd import _capi
    lib = _capi.load()
    p = _capi.ptr
    n_points = c.n_points if n_points is None else n_points
    if isinstance(edges, tuple) and len(edges) and edges[0] == "n_bins":      # ("n_bins", a count, the array handed over)
        n_bins, e = edges[1], np.ascontiguousarray(edges[2], F)
    else:
        e = np.ascontiguousarray(edges, F) if edges is not None else None
        n_bins = len(e) if e is not None else 3
    head = (ctx._h, p(c.x), p(c.y), p(c.z), p(c.r), None)
    tail = (C.c_float(c.probe), n_points, p(flags), p(e), n_bins, p(offsets), p(counts), cap, None, None)
    if batch:
        return lib.rsasa_dot_crowding_batch(*head, p(c.so), len(c.so) - 1, *tail)
    return lib.rsasa_dot_crowding(*head, c.n_atoms, *tail)


def test_sizing_protocol(ctx):
    c = cc.corner(33)
    w_off, w_rows, _ = _model(c)
    n_dots = int(w_off[-1])
    off = np.zeros(c.n_atoms + 1, np.uint64)
    assert _raw(ctx, c, c.edges, None, 0, off) == -8 and np.array_equal(off, w_off)      # RSASA_ERR_BUFFER_TOO_SMALL
    rows = np.full((n_dots, 3), 0xABABABAB, np.uint32)
    off[:] = 0
    assert _raw(ctx, c, c.edges, rows, n_dots - 1, off) == -8 and np.array_equal(off, w_off)
    assert (rows == 0xABABABAB).all()                                                    # nothing else is written
    assert _raw(ctx, c, c.edges, rows, n_dots, off) == 0 and np.array_equal(rows, w_rows)
    big = np.full((n_dots + 7, 3), 0xABABABAB, np.uint32)
    assert _raw(ctx, c, c.edges, big, n_dots + 7, off, batch=True) == 0
    assert np.array_equal(big[:n_dots], w_rows) and (big[n_dots:] == 0xABABABAB).all()
    none = cc.Case("none", *(np.zeros(0, F),) * 4, np.array([0], np.uint32))
    off0 = np.full(1, 9, np.uint64)
    assert _raw(ctx, none, c.edges, None, 0, off0) == 0 and off0[0] == 0                 # no atoms


def test_argument_rules(ctx):
    import rustsasa_amd
    c = cc.corner(33)
    off = np.zeros(c.n_atoms + 1, np.uint64)
    rows = np.zeros((c.n_atoms * 33, 8), np.uint32)
    cap = len(rows)
    bad = [(float("nan"),), (-1.0,), (float("inf"),), (6.0, 5.0), ("n_bins", 0, (6.0,)), ("n_bins", 9, (1.0,) * 9)]
    for edges in bad:
        assert _raw(ctx, c, edges, rows, cap, off) == -1, edges                          # RSASA_ERR_INVALID_ARGUMENT
    assert _raw(ctx, c, None, rows, cap, off) == -1                                      # NULL edges
    assert _raw(ctx, c, c.edges, rows, cap, None) == -1                                  # NULL offsets
    assert _raw(ctx, c, c.edges, rows, cap, off, n_points=0) == -1
    for edges in ((-0.0, 6.0), (6.0, 6.0), (1e-30, 3.4e38)):
        assert _raw(ctx, c, edges, rows, cap, off) == 0, edges
    with pytest.raises(ValueError):
        ctx.dot_crowding(*c.cols, c.probe, 33, edges=(1.0,) * 9)
    with pytest.raises(ValueError):
        ctx.dot_crowding(*c.cols, c.probe, 33, edges=())
    with pytest.raises(ValueError):
        ctx.dot_crowding(*c.cols, c.probe, 33, flags=np.zeros(c.n_atoms - 1, np.uint8))
    with pytest.raises(rustsasa_amd.RsasaError):
        ctx.dot_crowding(*c.cols, c.probe, 33, edges=(3.0, 2.0))
    _check(ctx, c)                                                                       # the context is as usable as before


@pytest.mark.parametrize("W", [1, 16])
def test_lane_counts_change_the_masks_and_the_dots_with_them(W):
    import rustsasa_amd
    c = cc.of_depth("cavity", n_points=100)
    with rustsasa_amd.Context(0, simd_width=W) as ctx:
        off, rows, free, _ = _run(ctx, c)
    w_off, w_rows, mask = _model(c, W=W)
    _equal(off, w_off)
    _equal(rows, w_rows)
    assert np.array_equal(free, mask.sum(axis=1))


# ---- sharing -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _walk_inputs():
    return cc.of_depth("ball", n_points=33), cc.of_depth("tiny", n_points=33), cc.lone(65)


def test_one_context_walked_through_this_family_between_the_others(ctx):
    """dot_crowding between surface_components, radial_counts, half_sphere_exposure, atom_depth and accessible_points on
    one context, forwards and back: it shares free, row_offsets, flags and sorted_flags with them.  Every result equals
    the same call on a fresh context."""
    import rustsasa_amd
    inputs = _walk_inputs()
    fl = cc.random_flags(inputs[0].n_atoms, 9)

    def others(cx, c, k):
        if len(c.so) != 2:
            return cx.surface_components_batch(*c.cols, c.so, c.probe, c.n_points)
        return (cx.surface_components(*c.cols, c.probe, c.n_points),
                (cx.radial_counts(*c.cols, c.probe, (4.0, 8.0), fl[:c.n_atoms] % 4, 4, fl[:c.n_atoms]),),
                cx.half_sphere_exposure(*c.cols, c.probe, None, fl[:c.n_atoms], 9.0),
                cx.atom_depth(*c.cols, c.probe, c.n_points), cx.accessible_points(*c.cols, c.probe, c.n_points))[k % 5]

    def crowd(cx, c):
        return _run(cx, c, flags=fl[:c.n_atoms] if c.n_atoms == len(fl) else None)

    with rustsasa_amd.Context(0) as fresh:
        alone = [crowd(fresh, c) for c in inputs]
    same = lambda a, b: all(g.tobytes() == w.tobytes() and g.shape == w.shape for g, w in zip(a, b))  # noqa: E731
    for k in list(range(5)) + list(range(5))[::-1]:
        for c, want in zip(inputs, alone):
            others(ctx, c, k)
            assert same(crowd(ctx, c), want), (k, c.name)
    w_off, w_rows, _ = _model(inputs[0], flags=fl)
    _equal(alone[0][0], w_off)
    _equal(alone[0][1], w_rows)


def test_a_call_beside_a_device_batch_in_flight(ctx):
    torch = pytest.importorskip("torch")
    import bench_workloads as bw
    c = cc.of_depth("cavity", n_points=33)
    w_off, w_rows, _ = _model(c)
    b = bw.synthetic_proteome(12, seed=4)
    dev = torch.device("cuda", 0)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cols = (tt(b.x), tt(b.y), tt(b.z), tt(b.radius), tt(b.ids.view(np.int64)))
    alone = torch.zeros(b.n_atoms, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.enqueue_device(*cols, b.structure_offsets, out_atom_sasa=alone, probe_radius=1.4, n_points=100)
    ctx.wait()
    out = torch.zeros(b.n_atoms, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.enqueue_device(*cols, b.structure_offsets, out_atom_sasa=out, probe_radius=1.4, n_points=100)
    off, rows, _, _ = _run(ctx, c)
    ctx.wait()
    assert out.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    _equal(off, w_off)
    _equal(rows, w_rows)


def test_eight_threads_on_one_context(ctx):
    cases = [cc.corner(33), cc.of_depth("tiny", n_points=33, edges=(2.0, 6.0, 14.0)), cc.lone(65), cc.packed()]
    want = [_model(c)[:2] for c in cases]
    errors = []

    def work(t):
        try:
            for k in range(6):
                n = (t + k) % len(cases)
                off, rows, _, _ = _run(ctx, cases[n])
                if not (np.array_equal(off, want[n][0]) and np.array_equal(rows, want[n][1])):
                    errors.append((t, k, n))
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:4]
