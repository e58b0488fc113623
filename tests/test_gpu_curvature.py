"""Dot curvature on the GPU (rsasa_dot_curvature*, k_dot_curvature of curvature.hip) against the exact CPU model
(curvature_model.py: the header's definition in numpy float32) row for row by np.array_equal, and against a second witness
from the same build: where the model reports no dropped pair, pairs[d] is the length of dot_links' list at link = reach
less its entries with d2 == 0; dot_offsets, free and sasa are those of dot_crowding_batch and calculate_sasa_batch.  The
cases are curvature_cases.py's (test_curvature_cpu.py pins them)."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import curvature_cases as cvc
import curvature_model as cvm
import depth_cases as dc
import points_model as pm

pytestmark = pytest.mark.gpu

F = np.float32
ONE = 1 << 24


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


def _run(ctx, c, reach=None):
    reach = c.reach if reach is None else reach
    if len(c.so) == 2:
        return ctx.dot_curvature(*c.cols, c.probe, c.n_points, reach)
    return ctx.dot_curvature_batch(*c.cols, c.so, c.probe, c.n_points, reach)


def _equal(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), [int(got[tuple(b)]) for b in bad[:5]], [int(want[tuple(b)]) for b in bad[:5]])


def _check(ctx, c, W=8):
    """The call against the model: offsets, pairs, moments, free and the values."""
    off, pairs, mom, free, sasa = _run(ctx, c)
    w_off, w_pairs, w_mom, dropped, mask = cvc.model(c, W)
    _equal(off, w_off)
    _equal(pairs, w_pairs)
    _equal(mom, w_mom)
    want_free = mask.sum(axis=1).astype(np.uint32)
    _equal(free, want_free)
    assert sasa.tobytes() == pm.sasa_of(c.r, c.probe, want_free, c.n_points).tobytes()
    return off, pairs, mom, dropped


def _witness(ctx, c, pairs=None, dropped=None):
    """pairs against the lists of dot_links_batch of the same build at link = reach; offsets, free and the values
    against dot_links_batch, dot_crowding_batch and calculate_sasa_batch."""
    off, got, _, free, sasa = _run(ctx, c)
    if pairs is not None:
        _equal(got, pairs)
    if dropped is None:
        dropped = cvc.model(c)[3]
    l_off, l_loff, l_ent, l_free, l_sasa = ctx.dot_links_batch(*c.cols, c.so, c.probe, c.n_points, c.reach)
    c_off, _, c_free, c_sasa = ctx.dot_crowding_batch(*c.cols, c.so, c.probe, c.n_points, (4.0,))
    atom, _ = ctx.calculate_sasa_batch(*c.cols, c.so, c.probe, c.n_points)
    assert off.tobytes() == l_off.tobytes() == c_off.tobytes() and free.tobytes() == l_free.tobytes() == c_free.tobytes()
    assert sasa.tobytes() == l_sasa.tobytes() == c_sasa.tobytes() == atom.tobytes()
    lo = l_loff.astype(np.int64)
    zero = np.concatenate([[0], np.cumsum(l_ent["d2"] == 0)])
    length = np.diff(lo) - (zero[lo[1:]] - zero[lo[:-1]])
    clean = dropped == 0
    assert clean.any() or len(got) == 0
    _equal(got[clean].astype(np.int64), length[clean])
    return got


# ---- dots per atom, point counts ---------------------------------------------------------------------------------------------------

def test_atoms_with_0_1_63_64_and_65_dots(ctx):
    c = cvc.dot_counts()
    off, pairs, mom, dropped = _check(ctx, c)
    assert np.diff(off.astype(np.int64))[c.info["first"]].tolist() == [0, 1, 63, 64, 65] and pairs.any() and mom.any(axis=0).all()
    _witness(ctx, c, pairs, dropped)


@pytest.mark.parametrize("n_points", cvc.POINT_COUNTS)
def test_every_point_count(ctx, n_points):
    c = cvc.cluster(n_points)
    off, pairs, mom, dropped = _check(ctx, c)
    assert pairs.any() and int(off[-1]) >= n_points                       # (at ONE point: the cluster's three poles)
    _witness(ctx, c, pairs, dropped)


def test_lone_atom_at_960_points_pairs_every_dot_with_every_other(ctx):
    c = cvc.lone960()
    off, pairs, mom, dropped = _check(ctx, c)
    assert off.tolist() == [0, 960] and (pairs + dropped == 959).all() and pairs.min() > 900
    _witness(ctx, c, pairs, dropped)


# ---- staging -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", cvc.CELL_COUNTS)
def test_63_64_65_staged_atoms_in_one_round_and_a_cell_of_200(ctx, k):
    c = cvc.cell_of(k)
    off, pairs, mom, dropped = _check(ctx, c)
    assert int(off[-1]) == 8 * (k + 1) and pairs[:8 * k].all()
    _witness(ctx, c, pairs, dropped)


# ---- reaches ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", range(6))
def test_reaches_from_zero_to_six(ctx, which):
    h = float(F(dc.PROBE) + dc.RADII.max())
    c = cvc.reach_case(cvc.reaches(h)[which])
    off, pairs, mom, dropped = _check(ctx, c)
    assert pairs.any() == (which >= 2)
    _witness(ctx, c, pairs, dropped)


def test_a_reach_that_covers_the_whole_grid(ctx):
    c = cvc.whole_grid()
    off, pairs, mom, dropped = _check(ctx, c)
    assert (pairs + dropped == int(off[-1]) - 1).all()                   # every dot meets every other
    _witness(ctx, c, pairs, dropped)


@pytest.mark.parametrize("d", range(6))
def test_tie_partners_in_the_last_swept_shell(ctx, d):
    c = cvc.last_shell_tie(d)
    off, pairs, mom, dropped = _check(ctx, c)
    near = _run(ctx, c, reach=float(c.info["below"]))[1]
    lost = np.flatnonzero(pairs > near)
    assert len(lost) >= 4 and set(np.searchsorted(off.astype(np.int64), lost, side="right") - 1) >= {0, 1, 3, 4}
    _witness(ctx, c, pairs, dropped)


@pytest.mark.parametrize("beyond", [False, True])
def test_an_atom_exactly_at_the_staging_cut_and_one_float_beyond(ctx, beyond):
    c = cvc.at_the_cut(beyond)
    off, pairs, mom, dropped = _check(ctx, c)
    assert pairs.any()
    _witness(ctx, c, pairs, dropped)


def test_the_pair_that_only_the_h_of_the_cut_keeps(ctx):
    c = cvc.bare_cut()
    off, pairs, mom, dropped = _check(ctx, c)
    assert pairs.tolist() == [1, 1, 0] and mom[0].tolist() == [9 * ONE // 16, 3 * ONE // 4, 3 * ONE // 4, 0, 0, 0, 0, 0]
    _witness(ctx, c, pairs, dropped)


# ---- the grids of the shared sweep -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n_points", cvc.SWEEP_RUNS)
def test_thin_slanted_and_margin_grids(ctx, name, n_points):
    """margin_over fails the margins: its sweeps cover the grid and its staging cut is off."""
    c = cvc.sweep_case(name, n_points)
    off, pairs, mom, dropped = _check(ctx, c)
    assert pairs.any() or name.startswith("slant")                       # (a slanted column has one dot)
    _witness(ctx, c, pairs, dropped)


# ---- the drop rule ------------------------------------------------------------------------------------------------------------------------

def test_coincident_dots_a_dot_straight_above_and_the_bound_of_2_to_the_24(ctx):
    off, pairs, mom, dropped = _check(ctx, cvc.coincident())
    assert pairs.tolist() == [1, 1, 2]
    _witness(ctx, cvc.coincident(), pairs, dropped)                      # the links list the coincident dot at d2 == 0
    off, pairs, mom, dropped = _check(ctx, cvc.above())
    assert pairs.tolist() == [1, 0, 1] and dropped.tolist() == [1, 1, 0]
    off, pairs, mom, dropped = _check(ctx, cvc.bound())
    assert pairs.tolist() == [1, 1, 0] and mom[0, 0] == ONE * ONE
    off, pairs, mom, dropped = _check(ctx, cvc.two_dots())
    assert mom[:, 1].tolist() == [4 * ONE, -4 * ONE]
    _check(ctx, cvc.axis_pair())


@pytest.mark.parametrize("which", ["coordinate", "radius"])
def test_a_nan_atom_has_zero_rows_and_pairs_with_nobody(ctx, which):
    c = cvc.nan_case(which)
    off, pairs, mom, dropped = _check(ctx, c)
    a = c.info["atom"]
    mine = slice(int(off[a]), int(off[a + 1]))
    assert int(off[a + 1] - off[a]) == c.n_points and not pairs[mine].any() and not mom[mine].any() and pairs.any()


def test_an_infinite_coordinate_is_refused_and_the_next_call_is_right(ctx):
    import rustsasa_amd
    c = cvc.cluster(65)
    x = c.x.copy()
    x[3] = np.inf
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.dot_curvature_batch(x, c.y, c.z, c.r, None, c.so, c.probe, 65, 3.0)
    assert e.value.status == -5                                          # RSASA_ERR_GRID_TOO_LARGE
    _check(ctx, c)


def test_zero_rows_after_a_dense_call_on_the_same_context(ctx):
    c = cvc.reach_case(6.0)
    off, pairs, mom, _ = _check(ctx, c)
    assert pairs.all() and mom[:, 0].all()
    _, z_pairs, z_mom, _, _ = _run(ctx, c, reach=0.0)                     # every row is written, as zeros
    assert z_pairs.shape == pairs.shape and z_mom.shape == mom.shape and not z_pairs.any() and not z_mom.any()
    few = cvc.reach_case(cvc.reaches(float(F(dc.PROBE) + dc.RADII.max()))[2])
    _check(ctx, few)                                                     # and a sparse call after the dense one is the model's
    _check(ctx, c)


# ---- batches ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tiny", "overlap_batch"])
def test_small_batches(ctx, name):
    c = cvc.small_batch(name)
    off, pairs, mom, dropped = _check(ctx, c)
    if name == "overlap_batch":                                          # dots of different structures never pair
        for s in range(len(c.so) - 1):
            b, e = int(c.so[s]), int(c.so[s + 1])
            alone = ctx.dot_curvature(*(a[b:e] for a in c.cols[:4]), None, c.probe, c.n_points, c.reach)
            _equal(alone[1], pairs[int(off[b]):int(off[e])])
            _equal(alone[2], mom[int(off[b]):int(off[e])])
    _witness(ctx, c, pairs, dropped)


def test_empty_structures_and_a_structure_of_65536_atoms(ctx):
    """Offsets, free and the values against dot_crowding_batch on the same input; a seeded sample of the big structure's
    atoms against the model's pair_rows; every row of the small structures against the model; and the link witness on
    every row that the sample shows clean."""
    c = cvc.big()
    off, pairs, mom, free, sasa = _run(ctx, c)
    c_off, _, c_free, c_sasa = ctx.dot_crowding_batch(*c.cols, c.so, c.probe, c.n_points, (4.0,))
    assert off.tobytes() == c_off.tobytes() and free.tobytes() == c_free.tobytes() and sasa.tobytes() == c_sasa.tobytes()
    words, _ = ctx.accessible_points_batch(*c.cols, c.so, c.probe, c.n_points)
    mask = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(len(words), -1)[:, :c.n_points]
    assert np.array_equal(mask.sum(axis=1), free)
    s = c.info["big"]
    b, e = int(c.so[s]), int(c.so[s + 1])
    assert e - b == 65536 and int(off[e] - off[b]) > 65536
    small = cvc.Case("small", c.x[:b], c.y[:b], c.z[:b], c.r[:b], c.so[:s + 1], c.n_points, c.reach, c.probe)
    _, w_pairs, w_mom, _, _ = cvm.rows_batch(*small.cols, small.so, c.probe, c.n_points, c.reach, mask=mask[:b])
    _equal(pairs[:int(off[b])], w_pairs)
    _equal(mom[:int(off[b])], w_mom)
    have = np.flatnonzero(free[b:e])
    sample = np.sort(np.random.default_rng(17).permutation(have)[:cvc.BIG_SAMPLE])
    w_pairs, w_mom = cvc.big_sample_rows(c, mask, sample)
    rows = np.concatenate([np.arange(int(off[b + i]), int(off[b + i + 1])) for i in sample])
    _equal(pairs[rows], w_pairs)
    _equal(mom[rows], w_mom)
    assert w_pairs.any() and w_mom.any(axis=0).all()
    _, l_loff, l_ent, _, _ = ctx.dot_links_batch(*c.cols, c.so, c.probe, c.n_points, c.reach)
    assert not (l_ent["d2"] == 0).any()
    length = np.diff(l_loff.astype(np.int64))
    assert (pairs <= length).all() and (pairs == length).mean() > 0.99   # a dropped pair is rare: a dot straight above another


# ---- protocol ------------------------------------------------------------------------------------------------------------------------------

def _raw(ctx, c, pairs, mom, cap, offsets, reach=None, n_points=None, batch=False, free=None, sasa=None):
    from rustsasa_amd import _capi
    lib = _capi.load()
    p = _capi.ptr
    n_points = c.n_points if n_points is None else n_points
    reach = c.reach if reach is None else reach
    head = (ctx._h, p(c.x), p(c.y), p(c.z), p(c.r), None)
    tail = (C.c_float(c.probe), n_points, C.c_float(reach), p(offsets), p(pairs), p(mom), cap, p(free), p(sasa))
    if batch:
        return lib.rsasa_dot_curvature_batch(*head, p(c.so), len(c.so) - 1, *tail)
    return lib.rsasa_dot_curvature(*head, c.n_atoms, *tail)


def test_sizing_protocol(ctx):
    c = cvc.of(dc.get("corner"), 33, 3.0)
    w_off, w_pairs, w_mom, _, _ = cvc.model(c)
    n_dots = int(w_off[-1])
    fill, pfill = np.int64(-0x5454545454545455), np.uint32(0xABABABAB)
    off = np.zeros(c.n_atoms + 1, np.uint64)
    assert _raw(ctx, c, None, None, 0, off) == -8 and np.array_equal(off, w_off)         # RSASA_ERR_BUFFER_TOO_SMALL
    pairs, mom = np.full(n_dots, pfill, np.uint32), np.full((n_dots, 8), fill, np.int64)
    free = np.full(c.n_atoms, pfill, np.uint32)
    off[:] = 0
    assert _raw(ctx, c, pairs, mom, n_dots - 1, off, free=free) == -8 and np.array_equal(off, w_off)
    assert (pairs == pfill).all() and (mom == fill).all() and (free == pfill).all()      # nothing else is written
    assert _raw(ctx, c, pairs, None, n_dots, off) == -8 and _raw(ctx, c, None, mom, n_dots, off) == -8
    assert (pairs == pfill).all() and (mom == fill).all()
    assert _raw(ctx, c, pairs, mom, n_dots, off, free=free) == 0
    assert np.array_equal(pairs, w_pairs) and np.array_equal(mom, w_mom) and np.array_equal(free, np.diff(w_off.astype(np.int64)))
    big_p, big_m = np.full(n_dots + 7, pfill, np.uint32), np.full((n_dots + 7, 8), fill, np.int64)
    assert _raw(ctx, c, big_p, big_m, n_dots + 7, off, batch=True) == 0
    assert np.array_equal(big_p[:n_dots], w_pairs) and (big_p[n_dots:] == pfill).all()
    assert np.array_equal(big_m[:n_dots], w_mom) and (big_m[n_dots:] == fill).all()
    none = cvc.Case("none", *(np.zeros(0, F),) * 4, np.array([0, 0], np.uint32), 33, 3.0)
    off0 = np.full(1, 9, np.uint64)
    assert _raw(ctx, none, None, None, 0, off0) == 0 and off0[0] == 0                    # no atoms
    got = ctx.dot_curvature_batch(*none.cols, np.array([0, 0, 0], np.uint32), 1.4, 33, 3.0)
    assert got[0].tolist() == [0] and got[1].shape == (0,) and got[2].shape == (0, 8) and got[2].dtype == np.int64


def test_argument_rules(ctx):
    import rustsasa_amd
    c = cvc.of(dc.get("corner"), 33, 3.0)
    off = np.zeros(c.n_atoms + 1, np.uint64)
    pairs, mom = np.zeros(c.n_atoms * 33, np.uint32), np.zeros((c.n_atoms * 33, 8), np.int64)
    cap = len(pairs)
    for reach in (float("nan"), -1.0, float("inf"), -float("inf"), -1e-45):
        assert _raw(ctx, c, pairs, mom, cap, off, reach=reach) == -1, reach              # RSASA_ERR_INVALID_ARGUMENT
        assert _raw(ctx, c, pairs, mom, cap, off, reach=reach, batch=True) == -1, reach
    assert _raw(ctx, c, pairs, mom, cap, None) == -1                                     # NULL offsets
    assert _raw(ctx, c, pairs, mom, cap, off, n_points=0) == -1
    for reach in (-0.0, 0.0, 1e-30, 3.4e38):
        assert _raw(ctx, c, pairs, mom, cap, off, reach=reach) == 0, reach
    n_dots = int(off[-1])
    assert (pairs[:n_dots] + cvc.model(cvc.of(dc.get("corner"), 33, 3.4e38))[3] == n_dots - 1).all()   # reach2 = +inf: everybody
    assert _raw(ctx, c, pairs, mom, cap, off, reach=-0.0) == 0 and not pairs.any() and not mom.any()   # -0.0 is 0
    _check(ctx, cvc.of(dc.get("corner"), 33, 3.4e38))
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.dot_curvature(*c.cols, c.probe, 33, reach=float("nan"))
    assert e.value.status == -1
    with pytest.raises(ValueError):
        ctx.dot_curvature(*c.cols, c.probe, 0)
    with pytest.raises(ValueError):
        ctx.dot_curvature(c.x[:-1], c.y, c.z, c.r, None, c.probe, 33)
    _check(ctx, c)                                                                       # the context is as usable as before


@pytest.mark.parametrize("W", [1, 16])
def test_lane_counts_change_the_masks_and_the_dots_with_them(W):
    import rustsasa_amd
    c = cvc.of(dc.get("cavity"), 100, 3.0)
    with rustsasa_amd.Context(0, simd_width=W) as ctx:
        off, pairs, mom, free, _ = _run(ctx, c)
    w_off, w_pairs, w_mom, _, mask = cvc.model(c, W)
    _equal(off, w_off)
    _equal(pairs, w_pairs)
    _equal(mom, w_mom)
    assert np.array_equal(free, mask.sum(axis=1))


def test_the_values_of_a_protein_like_ball(ctx):
    """curvature_values on the kernel's rows: convex on the outside of the ball, concave in its void."""
    import rustsasa_amd
    c = cvc.of(dc.get("cavity"), 100, 3.0)
    off, pairs, mom, free, _ = _run(ctx, c)
    mean, gauss, k1, k2, si = rustsasa_amd.curvature_values(pairs, mom)
    ok = pairs > 0
    assert ok.mean() > 0.99 and np.isfinite(mean[ok]).all() and (k1[ok] >= k2[ok]).all() and (np.abs(si[ok]) <= 1).all()
    owner = np.repeat(np.arange(c.n_atoms), np.diff(off.astype(np.int64)))
    centre = np.stack([c.x, c.y, c.z], -1).astype(np.float64)
    inner = np.linalg.norm(centre[owner] - dc.VOID_CENTRE, axis=1) < dc.VOID_RADIUS + 2.5
    outer = np.linalg.norm(centre[owner], axis=1) > dc.BALL_RADIUS - 1.0
    assert inner.sum() > 20 and outer.sum() > 200
    assert np.nanmedian(mean[outer]) > 0 > np.nanmedian(mean[inner])
    per_atom = rustsasa_amd.dot_means(off, mean)
    assert per_atom.shape == (c.n_atoms,)


# ---- sharing ---------------------------------------------------------------------------------------------------------------------------------

def test_a_call_beside_a_device_batch_in_flight(ctx):
    torch = pytest.importorskip("torch")
    import bench_workloads as bw
    c = cvc.reach_case(3.0)
    w_off, w_pairs, w_mom, _, _ = cvc.model(c)
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
    off, pairs, mom, _, _ = _run(ctx, c)
    ctx.wait()
    assert out.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    _equal(off, w_off)
    _equal(pairs, w_pairs)
    _equal(mom, w_mom)


@functools.lru_cache(maxsize=None)
def _thread_cases():
    return (cvc.cluster(65), cvc.small_batch("tiny"), cvc.cell_of(65), cvc.of(dc.get("corner"), 33, 3.0))


def test_eight_threads_on_one_context(ctx):
    cases = _thread_cases()
    want = [cvc.model(c)[:3] for c in cases]
    errors = []

    def work(t):
        try:
            for k in range(6):
                n = (t + k) % len(cases)
                got = _run(ctx, cases[n])
                if not all(np.array_equal(g, w) for g, w in zip(got[:3], want[n])):
                    errors.append((t, k, n))
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:4]
