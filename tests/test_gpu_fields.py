"""Dot fields on the GPU (rsasa_dot_fields*, k_dot_fields of fields.hip) against the exact CPU model (fields_model.py: the
header's definition in numpy float32) cell for cell by np.array_equal, and against a second witness on the GPU itself:
all-ones weights under STEP are 2^24 times dot_crowding_batch's cumulative counts of the same build.  The cases are
fields_cases.py's: those of crowding_cases.py with weights, and the fields' own (test_fields_cpu.py pins them)."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import crowding_cases as cc
import fields_cases as fc
import fields_model as fm
import points_model as pm
import sweep_cases as sc

pytestmark = pytest.mark.gpu

F = np.float32
ONE = 1 << 24


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


def _run(ctx, f, flags="own"):
    flags = f.flags if isinstance(flags, str) else flags
    tail = (f.probe, f.n_points, f.weights, f.kinds, f.cutoff, flags)
    if len(f.so) == 2:
        return ctx.dot_fields(*f.cols, *tail)
    return ctx.dot_fields_batch(*f.cols, f.so, *tail)


def _equal(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), [int(got[tuple(b)]) for b in bad[:5]], [int(want[tuple(b)]) for b in bad[:5]])


def _check(ctx, f, flags="own"):
    """The call against the model: offsets, rows, free and the values."""
    off, rows, free, sasa = _run(ctx, f, flags)
    w_off, w_rows, mask = fc.model(f, flags=flags)
    _equal(off, w_off)
    _equal(rows, w_rows)
    want_free = mask.sum(axis=1).astype(np.uint32)
    _equal(free, want_free)
    assert sasa.tobytes() == pm.sasa_of(f.r, f.probe, want_free, f.n_points).tobytes()
    return off, rows, mask


def _witness(ctx, c, cutoff=None):
    """STEP with ones against dot_crowding_batch of the same build at the one edge `cutoff`; offsets, free and the
    values against it."""
    cutoff = float(c.edges[-1]) if cutoff is None else cutoff
    f = fc.of(c, kinds=(fm.STEP,), w=np.ones((c.n_atoms, 1)), cutoff=cutoff)
    off, rows, free, sasa = ctx.dot_fields_batch(*f.cols, f.so, f.probe, f.n_points, f.weights, f.kinds, cutoff, f.flags)
    c_off, c_rows, c_free, c_sasa = ctx.dot_crowding_batch(*c.cols, c.so, c.probe, c.n_points, (cutoff,), c.flags)
    assert off.tobytes() == c_off.tobytes() and free.tobytes() == c_free.tobytes() and sasa.tobytes() == c_sasa.tobytes()
    _equal(rows, c_rows.astype(np.int64) * ONE)
    return rows


# ---- dots per atom -------------------------------------------------------------------------------------------------------

def test_atoms_with_0_1_63_64_and_65_dots(ctx):
    f = fc.of(cc.caps())
    off, rows, _ = _check(ctx, f)
    assert np.diff(off.astype(np.int64))[f.info["owners"]].tolist() == [0, 1, 63, 64, 65] and rows.any(axis=0).all()
    _witness(ctx, f.c)


@pytest.mark.parametrize("n_points", cc.POINT_COUNTS)
def test_corner_at_every_point_count(ctx, n_points):
    f = fc.of(cc.corner(n_points))
    off, rows, _ = _check(ctx, f)
    assert rows.any(axis=0).all()
    _witness(ctx, f.c)


def test_lone_atom_at_960_points_takes_every_pass(ctx):
    c = cc.lone()
    f = fc.of(c, w=np.ones((1, 4)))
    off, rows, _ = _check(ctx, f)
    assert off.tolist() == [0, 960] and (rows[:, 0] == ONE).all() and rows.all()
    _, none, _, _ = _run(ctx, f, flags=np.array([0xFE], np.uint8))        # the owner without its partner bit
    assert none.shape == (960, 4) and not none.any()


def test_pair_at_960_points(ctx):
    f = fc.of(cc.pair())
    off, rows, _ = _check(ctx, f)
    assert (np.diff(off.astype(np.int64)) > cc.PASS).all() and rows.any(axis=0).all()
    _witness(ctx, f.c)


# ---- channels and kinds ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kinds", fc.CHANNEL_KINDS, ids=lambda k: "".join(map(str, k)))
def test_one_to_four_channels_over_every_kind(ctx, kinds):
    f = fc.of(cc.of_depth("cavity", n_points=20, edges=(9.0,)), kinds=kinds, seed=50 + len(kinds))
    off, rows, _ = _check(ctx, f)
    assert rows.shape[1] == len(kinds) and rows.any(axis=0).all()
    last = len(kinds) - 1                                                  # a channel does not depend on its neighbours
    alone = fc.FCase(f.c, f.weights[:, last:].copy(), kinds[last:], f.cutoff)
    _equal(_run(ctx, alone)[1][:, 0], rows[:, last])


def test_a_one_dimensional_weight_array_and_the_default_kind(ctx):
    import rustsasa_amd
    c = cc.corner(33)
    w = fc.weights(c.n_atoms, 1, 9)
    off, rows, _, _ = ctx.dot_fields(*c.cols, c.probe, 33, w[:, 0])
    f = fc.FCase(c, w, (fm.INV_D,), 10.0)
    w_off, w_rows, _ = fc.model(f)
    _equal(off, w_off)
    _equal(rows, w_rows)
    assert np.array_equal(rustsasa_amd.field_values(rows), fm.values(w_rows))
    means = rustsasa_amd.dot_means(off, rustsasa_amd.field_values(rows)[:, 0])
    assert means.shape == (c.n_atoms,) and np.isfinite(means[np.diff(off.astype(np.int64)) > 0]).all()


# ---- exact ties ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", cc.TIE_KINDS)
def test_exact_ties_at_the_cutoff(ctx, kind):
    f = fc.of(cc.tie(kind), seed=3)
    _check(ctx, f)
    _witness(ctx, f.c)


def test_the_tie_partner_is_gained_at_the_cutoff_and_lost_just_below(ctx):
    last, below = fc.of(cc.tie("last"), seed=3), fc.of(cc.tie("below"), seed=3)
    (_, rows, mask), (_, b_rows, _) = _check(ctx, last), _check(ctx, below)
    d = int(mask[0, :cc.TIE_DOT].sum())
    assert (rows[d] != b_rows[d]).all()


@pytest.mark.parametrize("edge0", [0.0, 1e-30])
def test_a_coincident_partner_at_d2_zero(ctx, edge0):
    c = cc.tie_zero(edge0)
    w = np.zeros((2, 4), F)
    w[1] = 3.0
    for cutoff in (edge0, 4.0):
        off, rows, _ = _check(ctx, fc.of(c, w=w, cutoff=cutoff))
        assert rows[cc.TIE_DOT, [0, 3]].tolist() == [3 * ONE, 3 * ONE]      # STEP and 1 / (1 + 0) count the partner
    assert rows[cc.TIE_DOT, 1] == rows[cc.TIE_DOT, 2] == 0                  # 1 / 0 is infinite: nothing (weight 0 elsewhere)
    _witness(ctx, c, edge0)


# ---- the stop rule -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shell", cc.LAST_SHELLS)
def test_tie_partners_in_the_last_swept_shell(ctx, shell):
    c = cc.last_shell(shell)
    f = fc.of(c, kinds=(fm.STEP, fm.INV_D, fm.INV_1PD), w=np.ones((c.n_atoms, 3)))
    off, rows, _ = _check(ctx, f)
    near = fc.model(fc.FCase(c, f.weights, f.kinds, float(np.nextafter(F(c.edges[-1]), F(0)))))[1]
    for owner, k, _ in c.info["ties"]:
        assert rows[int(off[owner]) + k, 0] - near[int(off[owner]) + k, 0] >= ONE      # the tie partner's term is there
    _witness(ctx, c)


@pytest.mark.parametrize("reach", cc.REACHES + ("grid",))
def test_reaches_of_two_to_six_shells_and_the_whole_grid(ctx, reach):
    edges = (4.0, cc.COVER) if reach == "grid" else cc.reach_edges(sc.H, reach)
    c = cc.of_depth("cavity", n_points=20, edges=edges)
    f = fc.of(c, kinds=(fm.STEP, fm.INV_D2), seed=60)
    _check(ctx, f)
    rows = _witness(ctx, c)
    if reach == "grid":
        assert (rows[:, 0] == c.n_atoms * ONE).all()                      # everybody counts for every dot


# ---- staging -----------------------------------------------------------------------------------------------------------------

def test_a_cell_of_200_atoms_and_63_64_65_partners(ctx):
    _check(ctx, fc.of(cc.crowd(), kinds=(fm.INV_D, fm.INV_1PD)))
    _witness(ctx, cc.crowd())
    f = fc.of(cc.packed())
    assert (f.flags >> 1).any()                                           # garbage in the other flag bits
    _check(ctx, f)
    _witness(ctx, f.c)


# ---- flags, weights -------------------------------------------------------------------------------------------------------------

def test_flag_patterns_and_zero_rows_after_a_dense_call(ctx):
    f = fc.of(cc.of_depth("ball", n_points=33))
    dense = _check(ctx, f)[1]
    assert dense.all(axis=1).any()
    for seed in (1, 2):
        _check(ctx, f, flags=cc.random_flags(f.n_atoms, seed))
    off, rows, free, _ = _run(ctx, f, flags=np.full(f.n_atoms, 0xFE, np.uint8))   # no partner: every row written, as zeros
    assert rows.shape == dense.shape and not rows.any()
    _check(ctx, f)
    off, rows, free, _ = _run(ctx, fc.FCase(f.c, np.zeros_like(f.weights), f.kinds, f.cutoff))   # no weight: the same
    assert rows.shape == dense.shape and not rows.any()


def test_nan_infinite_and_bound_weights(ctx):
    f = fc.special_weights()
    off, rows, _ = _check(ctx, f)
    assert rows.any(axis=0).all() and (np.abs(rows[:, 0]) >= 1 << 47).any() and set(np.unique(rows[:, 3]).tolist()) <= {0, 2}
    for kind in (fm.INV_D, fm.INV_D2, fm.INV_1PD):                         # the same weights under the other kinds
        _check(ctx, fc.FCase(f.c, f.weights, (kind,) * 4, f.cutoff))


def test_the_sum_wraps_on_the_gpu_as_in_the_model(ctx):
    f = fc.wrap_ball()
    off, rows, free, _ = _run(ctx, f)
    w_off, w_rows, mask = fc.model(f)
    _equal(off, w_off)
    _equal(rows, w_rows)
    assert len(rows) >= 16 and (rows == fc.wrapped(fc.WRAP_ATOMS)).all() and fc.wrapped(fc.WRAP_ATOMS) < 0


# ---- non-finite input --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["nan_coordinate", "nan_radius"])
def test_a_nan_atom_has_zero_rows_and_counts_for_nobody(ctx, name):
    c = getattr(cc, name)()
    f = fc.of(c, w=np.ones((c.n_atoms, 4)))
    off, rows, _ = _check(ctx, f)
    a = c.info["atom"]
    assert int(off[a + 1] - off[a]) == c.n_points and not rows[int(off[a]):int(off[a + 1])].any() and rows.any()
    _witness(ctx, c)


def test_an_infinite_coordinate_is_refused_and_the_next_call_is_right(ctx):
    import rustsasa_amd
    f = fc.of(cc.corner(33))
    x = f.x.copy()
    x[3] = np.inf
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.dot_fields(x, f.y, f.z, f.r, None, f.probe, 33, f.weights, f.kinds, f.cutoff)
    assert e.value.status == -5                                          # RSASA_ERR_GRID_TOO_LARGE
    _check(ctx, f)


# ---- batches -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tiny", "overlap_batch"])
def test_small_batches(ctx, name):
    c = cc.of_depth(name, n_points=33, edges=(2.0, 6.0, 14.0))
    f = fc.of(c, kinds=(fm.STEP, fm.INV_D), w=np.ones((c.n_atoms, 2)))
    off, rows, _ = _check(ctx, f)
    if name == "overlap_batch":
        assert (rows[-33:, 0] == ONE).all()                              # the lone atom's dots see the lone atom only
    _witness(ctx, c)


N_TAIL_SAMPLE = 48


def test_empty_structures_and_a_structure_of_65536_atoms(ctx):
    """Offsets, free and the values against dot_crowding_batch on the same input, a seeded sample of the big structure's
    atoms against the model, every row of the small structures against it, and the STEP witness on every row."""
    f = fc.big_batch()
    c = f.c
    assert np.diff(c.so.astype(np.int64)).tolist() == [0, 5, 0, 400, 3, 65536, 0]
    off, rows, free, sasa = _run(ctx, f)
    c_off, c_rows, c_free, c_sasa = ctx.dot_crowding_batch(*c.cols, c.so, c.probe, c.n_points, (f.cutoff,))
    assert off.tobytes() == c_off.tobytes() and free.tobytes() == c_free.tobytes() and sasa.tobytes() == c_sasa.tobytes()
    words, _ = ctx.accessible_points_batch(*c.cols, c.so, c.probe, c.n_points)
    mask = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(len(words), -1)[:, :c.n_points]
    assert np.array_equal(mask.sum(axis=1), free)
    b, e = int(c.so[-3]), int(c.so[-2])
    assert e - b == 65536
    small = slice(0, b)
    _, want_small = fm.sums_batch(c.x[small], c.y[small], c.z[small], c.r[small], c.so[:-2], mask[small], c.probe, c.n_points,
                                  f.weights[small], f.kinds, f.cutoff)
    _equal(rows[:int(off[b])], want_small)
    have = np.flatnonzero(free[b:e])
    sample = np.sort(np.random.default_rng(17).permutation(have)[:N_TAIL_SAMPLE])
    sub = np.zeros_like(mask[b:e])
    sub[sample] = mask[b:e][sample]
    _, want = fm.sums(c.x[b:e], c.y[b:e], c.z[b:e], c.r[b:e], sub, c.probe, c.n_points, f.weights[b:e], f.kinds, f.cutoff)
    got = np.concatenate([rows[int(off[b + i]):int(off[b + i + 1])] for i in sample])
    _equal(got, want)
    assert got.any(axis=0).all()
    ones = ctx.dot_fields_batch(*c.cols, c.so, c.probe, c.n_points, np.ones(c.n_atoms, F), (fm.STEP,), f.cutoff)[1]
    _equal(ones, c_rows.astype(np.int64) * ONE)


# ---- identities ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_points", [100, 129])
def test_offsets_free_and_values_are_those_of_the_other_families(ctx, n_points):
    c = cc.of_depth("cavity", n_points=n_points)
    f = fc.of(c, kinds=(fm.INV_D,))
    off, rows, free, sasa = _run(ctx, f)
    c_off, c_rows, c_free, c_sasa = ctx.dot_crowding_batch(*c.cols, c.so, c.probe, n_points, c.edges)
    atom, _ = ctx.calculate_sasa_batch(*c.cols, c.so, c.probe, n_points)
    assert off.tobytes() == c_off.tobytes() and free.tobytes() == c_free.tobytes() and len(rows) == len(c_rows)
    assert sasa.tobytes() == c_sasa.tobytes() == atom.tobytes()
    assert np.array_equal(free, cc.masks(c).sum(axis=1))


# ---- protocol ------------------------------------------------------------------------------------------------------------------

def _raw(ctx, f, sums, cap, offsets, kinds="own", n_channels=None, cutoff=None, weights="own", n_points=None, batch=False):
    from rustsasa_amd import _capi
    lib = _capi.load()
    p = _capi.ptr
    n_points = f.n_points if n_points is None else n_points
    k = np.ascontiguousarray(f.kinds, np.uint8) if isinstance(kinds, str) else kinds
    w = f.weights if isinstance(weights, str) else weights
    n_channels = len(f.kinds) if n_channels is None else n_channels
    cutoff = f.cutoff if cutoff is None else cutoff
    head = (ctx._h, p(f.x), p(f.y), p(f.z), p(f.r), None)
    tail = (C.c_float(f.probe), n_points, None, p(w), p(k), n_channels, C.c_float(cutoff), p(offsets), p(sums), cap, None, None)
    if batch:
        return lib.rsasa_dot_fields_batch(*head, p(f.so), len(f.so) - 1, *tail)
    return lib.rsasa_dot_fields(*head, f.n_atoms, *tail)


def test_sizing_protocol(ctx):
    f = fc.of(cc.corner(33), kinds=(fm.INV_D, fm.STEP, fm.INV_1PD))
    w_off, w_rows, _ = fc.model(f)
    n_dots = int(w_off[-1])
    fill = np.int64(-0x5454545454545455)
    off = np.zeros(f.n_atoms + 1, np.uint64)
    assert _raw(ctx, f, None, 0, off) == -8 and np.array_equal(off, w_off)               # RSASA_ERR_BUFFER_TOO_SMALL
    rows = np.full((n_dots, 3), fill, np.int64)
    off[:] = 0
    assert _raw(ctx, f, rows, n_dots - 1, off) == -8 and np.array_equal(off, w_off)
    assert (rows == fill).all()                                                          # nothing else is written
    assert _raw(ctx, f, rows, n_dots, off) == 0 and np.array_equal(rows, w_rows)
    big = np.full((n_dots + 7, 3), fill, np.int64)
    assert _raw(ctx, f, big, n_dots + 7, off, batch=True) == 0
    assert np.array_equal(big[:n_dots], w_rows) and (big[n_dots:] == fill).all()
    none = fc.FCase(cc.Case("none", *(np.zeros(0, F),) * 4, np.array([0], np.uint32)), np.zeros((0, 3), F), f.kinds, 10.0)
    off0 = np.full(1, 9, np.uint64)
    assert _raw(ctx, none, None, 0, off0) == 0 and off0[0] == 0                          # no atoms
    off0[0] = 9
    assert _raw(ctx, none, None, 0, off0, weights=None) == 0 and off0[0] == 0            # (and no weights with them)


def test_argument_rules(ctx):
    import rustsasa_amd
    f = fc.of(cc.corner(33))
    off = np.zeros(f.n_atoms + 1, np.uint64)
    rows = np.zeros((f.n_atoms * 33, 4), np.int64)
    cap = len(rows)
    u8 = lambda *v: np.array(v, np.uint8)  # noqa: E731
    assert _raw(ctx, f, rows, cap, off, n_channels=0) == -1                              # RSASA_ERR_INVALID_ARGUMENT
    assert _raw(ctx, f, rows, cap, off, kinds=u8(0, 1, 2, 3, 0), n_channels=5) == -1
    assert _raw(ctx, f, rows, cap, off, kinds=u8(0, 1, 2, 4)) == -1
    assert _raw(ctx, f, rows, cap, off, kinds=u8(255), n_channels=1) == -1
    assert _raw(ctx, f, rows, cap, off, kinds=None) == -1                                # NULL kinds
    assert _raw(ctx, f, rows, cap, off, weights=None) == -1                              # NULL weights
    for cutoff in (float("nan"), -1.0, float("inf"), -float("inf")):
        assert _raw(ctx, f, rows, cap, off, cutoff=cutoff) == -1, cutoff
    assert _raw(ctx, f, rows, cap, None) == -1                                           # NULL offsets
    assert _raw(ctx, f, rows, cap, off, n_points=0) == -1
    for cutoff in (-0.0, 0.0, 1e-30, 3.4e38):
        assert _raw(ctx, f, rows, cap, off, cutoff=cutoff) == 0, cutoff
    zero = np.zeros_like(rows[:int(off[-1])])
    assert _raw(ctx, f, zero, len(zero), off, cutoff=-0.0) == 0
    _equal(zero, fc.model(fc.FCase(f.c, f.weights, f.kinds, 0.0))[1])                    # -0.0 is 0
    big = fc.FCase(f.c, f.weights, f.kinds, 3.4e38)                                      # c2 = +inf: the whole grid
    _check(ctx, big)
    with pytest.raises(ValueError):
        ctx.dot_fields(*f.cols, f.probe, 33)                                             # no weights
    with pytest.raises(ValueError):
        ctx.dot_fields(*f.cols, f.probe, 33, np.zeros((f.n_atoms, 5), F))
    with pytest.raises(ValueError):
        ctx.dot_fields(*f.cols, f.probe, 33, np.zeros((f.n_atoms - 1, 2), F))
    with pytest.raises(ValueError):
        ctx.dot_fields(*f.cols, f.probe, 33, f.weights, kinds=(1, 2))                    # four channels, two kinds
    with pytest.raises(ValueError):
        ctx.dot_fields(*f.cols, f.probe, 33, f.weights, flags=np.zeros(f.n_atoms - 1, np.uint8))
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.dot_fields(*f.cols, f.probe, 33, f.weights, kinds=(0, 1, 2, 7))
    assert e.value.status == -1
    with pytest.raises(rustsasa_amd.RsasaError):
        ctx.dot_fields(*f.cols, f.probe, 33, f.weights, cutoff=float("nan"))
    _check(ctx, f)                                                                       # the context is as usable as before


@pytest.mark.parametrize("W", [1, 16])
def test_lane_counts_change_the_masks_and_the_dots_with_them(W):
    import rustsasa_amd
    f = fc.of(cc.of_depth("cavity", n_points=100), kinds=(fm.INV_D, fm.INV_1PD))
    with rustsasa_amd.Context(0, simd_width=W) as ctx:
        off, rows, free, _ = _run(ctx, f)
    w_off, w_rows, mask = fc.model(f, W=W)
    _equal(off, w_off)
    _equal(rows, w_rows)
    assert np.array_equal(free, mask.sum(axis=1))


# ---- sharing -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _walk_inputs():
    return (fc.of(cc.of_depth("ball", n_points=33)), fc.of(cc.of_depth("tiny", n_points=33), kinds=(fm.INV_D2,)),
            fc.of(cc.lone(65), kinds=(fm.STEP, fm.INV_1PD)))


def test_one_context_walked_through_this_family_between_the_others(ctx):
    """dot_fields between dot_crowding, dot_enclosure, surface_components, radial_counts, half_sphere_exposure and
    atom_depth on one context, forwards and back: it shares free, row_offsets, flags and sorted_flags with them.  Every
    result equals the same call on a fresh context."""
    import rustsasa_amd
    inputs = _walk_inputs()
    fl = cc.random_flags(inputs[0].n_atoms, 9)

    def others(cx, c, k):
        if len(c.so) != 2:
            return (cx.surface_components_batch(*c.cols, c.so, c.probe, c.n_points),
                    cx.dot_crowding_batch(*c.cols, c.so, c.probe, c.n_points, (3.0, 7.0)))[k % 2]
        return (lambda: cx.dot_crowding(*c.cols, c.probe, c.n_points, (4.0, 8.0), fl[:c.n_atoms][::-1].copy()),
                lambda: cx.dot_enclosure(*c.cols, c.probe, c.n_points, 30, 8.0, fl[:c.n_atoms]),
                lambda: cx.surface_components(*c.cols, c.probe, c.n_points),
                lambda: cx.radial_counts(*c.cols, c.probe, (4.0, 8.0), fl[:c.n_atoms] % 4, 4, fl[:c.n_atoms]),
                lambda: cx.half_sphere_exposure(*c.cols, c.probe, None, fl[:c.n_atoms], 9.0),
                lambda: cx.atom_depth(*c.cols, c.probe, c.n_points))[k % 6]()

    def fields(cx, f):
        return _run(cx, f, flags=fl[:f.n_atoms] if f.n_atoms == len(fl) else None)

    with rustsasa_amd.Context(0) as fresh:
        alone = [fields(fresh, f) for f in inputs]
    same = lambda a, b: all(g.tobytes() == w.tobytes() and g.shape == w.shape for g, w in zip(a, b))  # noqa: E731
    for k in list(range(6)) + list(range(6))[::-1]:
        for f, want in zip(inputs, alone):
            others(ctx, f.c, k)
            assert same(fields(ctx, f), want), (k, f.name)
    w_off, w_rows, _ = fc.model(inputs[0], flags=fl)
    _equal(alone[0][0], w_off)
    _equal(alone[0][1], w_rows)


def test_a_call_beside_a_device_batch_in_flight(ctx):
    torch = pytest.importorskip("torch")
    import bench_workloads as bw
    f = fc.of(cc.of_depth("cavity", n_points=33))
    w_off, w_rows, _ = fc.model(f)
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
    off, rows, _, _ = _run(ctx, f)
    ctx.wait()
    assert out.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    _equal(off, w_off)
    _equal(rows, w_rows)


def test_eight_threads_on_one_context(ctx):
    cases = [fc.of(cc.corner(33)), fc.of(cc.of_depth("tiny", n_points=33, edges=(2.0, 6.0, 14.0)), kinds=(fm.INV_D,)),
             fc.of(cc.lone(65), kinds=(fm.STEP, fm.INV_D2)), fc.of(cc.packed(), kinds=(fm.INV_1PD, fm.INV_D, fm.STEP))]
    want = [fc.model(f)[:2] for f in cases]
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
