"""Dot enclosure on the GPU (rsasa_dot_enclosure*, k_dot_enclosure of enclosure.hip) against the exact CPU model
(enclosure_model.py: the header's definition in numpy float32) word for word by np.array_equal.  The cases are those of
enclosure_cases.py and crowding_cases.py (test_enclosure_cpu.py and test_crowding_cpu.py pin each to what it is named
for)."""
import ctypes as C
import threading

import numpy as np
import pytest

import crowding_cases as cc
import depth_cases as dc
import enclosure_cases as ec
import enclosure_model as em
import points_model as pm
import sweep_cases as sc

pytestmark = pytest.mark.gpu

F = np.float32
_UNSET = object()
_MASKS = {}


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


def _masks(c, W=8):
    key = (c.name, c.n_atoms, c.n_points, float(c.probe), W)
    if key not in _MASKS:
        _MASKS[key] = ec.masks(c, W)
    return _MASKS[key]


def _args(c, n_dirs, reach, flags):
    return (c.n_dirs if n_dirs is None else n_dirs, c.reach if reach is None else reach, c.flags if flags is _UNSET else flags)


def _run(ctx, c, n_dirs=None, reach=None, flags=_UNSET):
    n_dirs, reach, flags = _args(c, n_dirs, reach, flags)
    if len(c.so) == 2:
        return ctx.dot_enclosure(*c.cols, c.probe, c.n_points, n_dirs, reach, flags)
    return ctx.dot_enclosure_batch(*c.cols, c.so, c.probe, c.n_points, n_dirs, reach, flags)


def _model(c, n_dirs=None, reach=None, flags=_UNSET, W=8):
    n_dirs, reach, flags = _args(c, n_dirs, reach, flags)
    mask = _masks(c, W)
    off, words = em.blocked_batch(c.x, c.y, c.z, c.r, c.so, mask, c.probe, c.n_points, n_dirs, reach, flags)
    return off, words, mask


def _equal(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), [hex(int(got[b])) for b in bad[:5]], [hex(int(want[b])) for b in bad[:5]])


def _check(ctx, c, n_dirs=None, reach=None, flags=_UNSET):
    """The call against the model: offsets, words, free and the values."""
    off, words, free, sasa = _run(ctx, c, n_dirs, reach, flags)
    w_off, w_words, mask = _model(c, n_dirs, reach, flags)
    _equal(off, w_off)
    _equal(words, w_words)
    want_free = mask.sum(axis=1).astype(np.uint32)
    _equal(free, want_free)
    assert sasa.tobytes() == pm.sasa_of(c.r, c.probe, want_free, c.n_points).tobytes()
    return off, words, mask


def _own(c, mask):
    return em.own_bits(c.n_points, c.n_dirs)[np.nonzero(mask)[1]]


# ---- structures ------------------------------------------------------------------------------------------------------------

STRUCTURES = ("cavity", "ball", "corner", "tiny")


@pytest.mark.parametrize("name", STRUCTURES)
def test_structures_at_100_points_30_directions_reach_10(ctx, name):
    c = ec.of_depth(name)
    off, words, mask = _check(ctx, c)
    assert (words & ~_own(c, mask)).any() and not (words >> np.uint32(30)).any()
    if name in ("cavity", "ball"):
        n = em.popcount(words)
        assert (int(n.min()), float(np.median(n)), int(n.max())) == {"cavity": (13, 17.0, 30), "ball": (13, 17.0, 25)}[name]


@pytest.mark.parametrize("n_dirs", ec.DIRS_SWEEP)
@pytest.mark.parametrize("name", STRUCTURES)
def test_structures_at_1_2_31_and_32_directions(ctx, name, n_dirs):
    off, words, _ = _check(ctx, ec.of_depth(name), n_dirs=n_dirs)
    assert words.any() and (n_dirs == 32 or not (words >> np.uint32(n_dirs)).any())


@pytest.mark.parametrize("k", range(6))
@pytest.mark.parametrize("name", STRUCTURES)
def test_structures_at_every_reach(ctx, name, k):
    """Reach 0, 1e-30 (its square underflows), h / 2, 10, 64 (the whole grid) and FLT_MAX (its square overflows)."""
    c = ec.of_depth(name)
    reach = ec.reaches(float(F(c.probe) + np.max(c.r)))[k]
    _check(ctx, c, reach=reach)


# ---- dots per atom ---------------------------------------------------------------------------------------------------------

def test_atoms_with_0_1_63_64_and_65_dots(ctx):
    c = ec.of(cc.caps())
    off, words, mask = _check(ctx, c)
    assert np.diff(off.astype(np.int64))[c.info["owners"]].tolist() == [0, 1, 63, 64, 65] and (words & ~_own(c, mask)).any()


def test_lone_atom_at_960_points_takes_every_pass(ctx):
    c = ec.of(cc.lone())
    off, words, mask = _check(ctx, c)
    assert off.tolist() == [0, 960] and np.array_equal(words, em.own_bits(960, 30)) and words.any()
    _, none, _, _ = _run(ctx, c, flags=np.array([0xFE], np.uint8))        # the owner without its obstacle bit
    assert none.shape == (960,) and not none.any()


def test_pair_at_960_points(ctx):
    c = ec.of(cc.pair())
    off, words, mask = _check(ctx, c)
    assert (np.diff(off.astype(np.int64)) > cc.PASS).all() and (words & ~_own(c, mask)).any()


def test_corner_at_960_points_one_sweep_and_several_side_by_side(ctx):
    c = ec.of(cc.corner(960))
    off, words, mask = _check(ctx, c)
    free = np.diff(off.astype(np.int64))
    assert free.max() > cc.PASS and 0 < free[free > 0].min() < cc.PASS


# ---- constructed cases -----------------------------------------------------------------------------------------------------

def test_every_ray_tie(ctx):
    c = ec.ray_ties()
    off, words, _ = _check(ctx, c)
    assert words[0::2].tolist() == [int(h) for h in c.info["hit"]] == [1, 0, 1, 0, 1, 0] and not words[1::2].any()


def test_rays_stopped_in_the_last_swept_shell(ctx):
    c = ec.last_shell()
    off, words, _ = _check(ctx, c)
    for owner, k, m, _ in c.info["rays"]:
        assert (int(words[int(off[owner]) + k]) >> m) & 1


def test_obstacles_at_the_prefilters_reach(ctx):
    c = ec.prefilter_edge()
    off, words, _ = _check(ctx, c)
    for s, kind in c.info["cases"]:
        assert int(words[int(off[int(c.so[s]) + 2])]) & 1 == (0 if kind == "outside" else 1), (s, kind)


def test_a_cell_of_200_atoms_and_63_64_65_obstacles(ctx):
    _check(ctx, ec.of(cc.crowd()))
    c = ec.of(cc.packed())
    off, words, mask = _check(ctx, c)
    _check(ctx, c, reach=1.0)
    assert (words & ~_own(c, mask)).any()


# ---- grids -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["column_z", "slant_xp", "slant_xm", "slant_yp", "slant_ym", "margin_under", "margin_over",
                                  "margin_small_h", "margin_large_h", "odd_beside_even", "crowded_cells"])
def test_thin_long_slanted_margin_and_odd_grids(ctx, name):
    d = sc.get(name)
    h = float(F(d.probe) + np.max(d.r[np.isfinite(d.r)]))
    n_points = sc.points_of(name)[0] if name in sc.POINTS else 20
    c = ec.Case(name, d.x, d.y, d.z, d.r, d.so, n_points=n_points, reach=2.7 * h, probe=d.probe)
    _check(ctx, c)
    _check(ctx, c, reach=0.4 * h, n_dirs=32)


# ---- flags -----------------------------------------------------------------------------------------------------------------

def test_flag_patterns_the_or_split_and_zero_words_after_a_dense_call(ctx):
    c = ec.of_depth("ball", n_points=33)
    dense = _check(ctx, c)[1]
    assert dense.any()
    for seed in (1, 2):
        _check(ctx, c, flags=cc.random_flags(c.n_atoms, seed))
    part = np.random.default_rng(23).integers(0, 3, c.n_atoms)
    split = [_run(ctx, c, flags=((part == k) | 0xF0).astype(np.uint8))[1] for k in range(3)]    # the GPU alone
    assert np.array_equal(split[0] | split[1] | split[2], dense) and all(s.any() for s in split)
    off, words, free, _ = _run(ctx, c, flags=np.full(c.n_atoms, 0xFE, np.uint8))   # no obstacle: every word written, as zero
    assert words.shape == dense.shape and not words.any()
    one = np.zeros(c.n_atoms, np.uint8)
    one[5] = 1
    _check(ctx, c, flags=one)


# ---- non-finite input --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["nan_coordinate", "nan_radius"])
def test_a_nan_atom_stops_nothing_and_is_stopped_by_nothing(ctx, name):
    c = ec.of(getattr(cc, name)())
    off, words, mask = _check(ctx, c)
    a = c.info["atom"]
    assert int(off[a + 1] - off[a]) == c.n_points
    assert np.array_equal(words[int(off[a]):int(off[a + 1])], em.own_bits(c.n_points, c.n_dirs))
    assert (words & ~_own(c, mask)).any()


def test_an_infinite_coordinate_is_refused_and_the_next_call_is_right(ctx):
    import rustsasa_amd
    c = ec.of(cc.corner(33))
    x = c.x.copy()
    x[3] = np.inf
    with pytest.raises(rustsasa_amd.RsasaError) as e:
        ctx.dot_enclosure(x, c.y, c.z, c.r, None, c.probe, 33)
    assert e.value.status == -5                                          # RSASA_ERR_GRID_TOO_LARGE
    _check(ctx, c)


# ---- batches -----------------------------------------------------------------------------------------------------------------

def test_a_batch_with_empty_structures(ctx):
    a, b = ec.of(cc.corner(33)), ec.of_depth("tiny", n_points=33)
    so = np.concatenate([[0, 0], a.so[1:], [a.so[-1]], a.so[-1] + b.so[1:], [a.so[-1] + b.so[-1]]]).astype(np.uint32)
    c = ec.Case("gaps", *(np.concatenate([p, q]) for p, q in zip(a.cols[:4], b.cols[:4])), so, n_points=33)
    assert (np.diff(so.astype(np.int64)) == 0).sum() >= 3 and so[1] == 0 and so[-1] == so[-2]
    off, words, _ = _check(ctx, c)
    _equal(words[:int(off[a.n_atoms])], _model(a)[1])                    # other structures stop nothing
    _check(ctx, ec.Case("empty", *(np.zeros(0, F),) * 4, np.array([0, 0, 0], np.uint32), n_points=33))


N_TAIL_SAMPLE = 2000
TAIL_POINTS = 12


def test_a_structure_of_65536_atoms_with_32_bit_cell_starts(ctx):
    """Every offset, free and the values against dot_crowding_batch on the same input, and the words of a seeded sample of
    2 000 of the big structure's atoms against the model."""
    d = dc.get("tail")
    c = ec.Case("tail", d.x, d.y, d.z, d.r, d.so, n_points=TAIL_POINTS, n_dirs=30, reach=8.0, probe=d.probe)
    off, words, free, sasa = _run(ctx, c)
    c_off, _, c_free, c_sasa = ctx.dot_crowding_batch(*c.cols, c.so, c.probe, TAIL_POINTS, (8.0,))
    assert off.tobytes() == c_off.tobytes() and free.tobytes() == c_free.tobytes() and sasa.tobytes() == c_sasa.tobytes()
    packed, _ = ctx.accessible_points_batch(*c.cols, c.so, c.probe, TAIL_POINTS)
    mask = ((packed[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(len(packed), -1)[:, :TAIL_POINTS]
    assert np.array_equal(mask.sum(axis=1), free)
    b, e = int(c.so[-2]), int(c.so[-1])
    assert e - b == 65536
    have = np.flatnonzero(free[b:e])
    sample = np.sort(np.random.default_rng(17).permutation(have)[:N_TAIL_SAMPLE])
    assert len(sample) == N_TAIL_SAMPLE
    _, want = em.blocked(c.x[b:e], c.y[b:e], c.z[b:e], c.r[b:e], mask[b:e], c.probe, TAIL_POINTS, c.n_dirs, c.reach, atoms=sample)
    got = np.concatenate([words[int(off[b + i]):int(off[b + i + 1])] for i in sample])
    _equal(got, want)
    assert got.any() and (got != em.own_bits(TAIL_POINTS, 30)[np.nonzero(mask[b:e][sample])[1]]).any()
    small = ec.Case("head", c.x[:b], c.y[:b], c.z[:b], c.r[:b], c.so[:-1], n_points=TAIL_POINTS, reach=8.0, probe=d.probe)
    _equal(words[:int(off[b])], _model(small)[1])                        # the small structures before it


# ---- identities ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_points", [100, 129])
def test_offsets_free_and_values_are_those_of_the_other_families(ctx, n_points):
    c = ec.of_depth("cavity", n_points=n_points)
    off, words, free, sasa = _run(ctx, c)
    c_off, rows, c_free, c_sasa = ctx.dot_crowding_batch(*c.cols, c.so, c.probe, n_points, (10.0,))
    s_off, labels, _, _ = ctx.surface_components(*c.cols, c.probe, n_points)
    total = ctx.calculate_sasa_batch(*c.cols, c.so, c.probe, n_points)
    atom_sasa = total[0] if isinstance(total, tuple) else total
    assert off.tobytes() == c_off.tobytes() == s_off.tobytes() and free.tobytes() == c_free.tobytes()
    assert sasa.tobytes() == c_sasa.tobytes() == np.ascontiguousarray(atom_sasa, F).tobytes()
    assert len(labels) == len(rows) == len(words) and np.array_equal(free, _masks(c).sum(axis=1))


# ---- protocol ------------------------------------------------------------------------------------------------------------------

def _raw(ctx, c, words, cap, offsets, reach=10.0, n_dirs=30, n_points=None, flags=None, batch=False):
    from rustsasa_amd import _capi
    lib = _capi.load()
    p = _capi.ptr
    n_points = c.n_points if n_points is None else n_points
    head = (ctx._h, p(c.x), p(c.y), p(c.z), p(c.r), None)
    tail = (C.c_float(c.probe), n_points, p(flags), C.c_float(reach), n_dirs, p(offsets), p(words), cap, None, None)
    if batch:
        return lib.rsasa_dot_enclosure_batch(*head, p(c.so), len(c.so) - 1, *tail)
    return lib.rsasa_dot_enclosure(*head, c.n_atoms, *tail)


def test_sizing_protocol(ctx):
    c = ec.of(cc.corner(33))
    w_off, w_words, _ = _model(c)
    n_dots = int(w_off[-1])
    off = np.zeros(c.n_atoms + 1, np.uint64)
    assert _raw(ctx, c, None, 0, off) == -8 and np.array_equal(off, w_off)               # RSASA_ERR_BUFFER_TOO_SMALL
    words = np.full(n_dots, 0xABABABAB, np.uint32)
    off[:] = 0
    assert _raw(ctx, c, words, n_dots - 1, off) == -8 and np.array_equal(off, w_off)
    assert (words == 0xABABABAB).all()                                                   # nothing else is written
    assert _raw(ctx, c, words, n_dots, off) == 0 and np.array_equal(words, w_words)
    big = np.full(n_dots + 7, 0xABABABAB, np.uint32)
    assert _raw(ctx, c, big, n_dots + 7, off, batch=True) == 0
    assert np.array_equal(big[:n_dots], w_words) and (big[n_dots:] == 0xABABABAB).all()
    none = ec.Case("none", *(np.zeros(0, F),) * 4, np.array([0], np.uint32))
    off0 = np.full(1, 9, np.uint64)
    assert _raw(ctx, none, None, 0, off0) == 0 and off0[0] == 0                          # no atoms


def test_argument_rules(ctx):
    import rustsasa_amd
    c = ec.of(cc.corner(33))
    off = np.zeros(c.n_atoms + 1, np.uint64)
    words = np.zeros(c.n_atoms * 33, np.uint32)
    cap = len(words)
    for n_dirs in (0, 33, 0xFFFFFFFF):
        assert _raw(ctx, c, words, cap, off, n_dirs=n_dirs) == -1, n_dirs                # RSASA_ERR_INVALID_ARGUMENT
    for reach in (float("nan"), float("inf"), -1.0, -float("inf")):
        assert _raw(ctx, c, words, cap, off, reach=reach) == -1, reach
    assert _raw(ctx, c, words, cap, None) == -1                                          # NULL offsets
    assert _raw(ctx, c, words, cap, off, n_points=0) == -1
    assert _raw(ctx, c, words, cap, off, batch=True) == 0
    from rustsasa_amd import _capi
    assert _capi.load().rsasa_dot_enclosure(ctx._h, None, None, None, None, None, c.n_atoms, C.c_float(1.4), 33, None,
                                            C.c_float(10.0), 30, _capi.ptr(off), _capi.ptr(words), cap, None, None) == -1
    for n_dirs in (1, 32):
        assert _raw(ctx, c, words, cap, off, n_dirs=n_dirs) == 0
    assert _raw(ctx, c, words, cap, off, reach=-0.0) == 0                                # -0.0 is 0
    _equal(words[:int(off[-1])], _model(c, reach=0.0)[1])
    for bad in (dict(n_dirs=0), dict(n_dirs=33), dict(reach=float("nan")), dict(reach=float("inf")), dict(reach=-1.0)):
        with pytest.raises(rustsasa_amd.RsasaError) as e:
            ctx.dot_enclosure(*c.cols, c.probe, 33, **bad)
        assert e.value.status == -1
    with pytest.raises(ValueError):
        ctx.dot_enclosure(*c.cols, c.probe, 33, flags=np.zeros(c.n_atoms - 1, np.uint8))
    _check(ctx, c)                                                                       # the context is as usable as before


@pytest.mark.parametrize("W", [1, 16])
def test_lane_counts_change_the_masks_and_the_dots_with_them(W):
    import rustsasa_amd
    c = ec.of_depth("cavity")
    with rustsasa_amd.Context(0, simd_width=W) as ctx:
        off, words, free, _ = _run(ctx, c)
    w_off, w_words, mask = _model(c, W=W)
    _equal(off, w_off)
    _equal(words, w_words)
    assert np.array_equal(free, mask.sum(axis=1))


# ---- sharing -------------------------------------------------------------------------------------------------------------------

def test_one_context_walked_through_this_family_between_the_others(ctx):
    """dot_enclosure between dot_crowding, surface_components, radial_counts, half_sphere_exposure and atom_depth on one
    context, forwards and back: it shares free, row_offsets, flags and sorted_flags with them.  Every result equals the
    same call on a fresh context."""
    import rustsasa_amd
    inputs = (ec.of_depth("ball", n_points=33), ec.of_depth("tiny", n_points=33), ec.of(cc.lone(65)))
    fl = cc.random_flags(inputs[0].n_atoms, 9)

    def others(cx, c, k):
        if len(c.so) != 2:
            return cx.dot_crowding_batch(*c.cols, c.so, c.probe, c.n_points, (4.0, 9.0))
        return (cx.dot_crowding(*c.cols, c.probe, c.n_points, (6.0, 8.0), fl[:c.n_atoms]),
                cx.surface_components(*c.cols, c.probe, c.n_points),
                (cx.radial_counts(*c.cols, c.probe, (4.0, 8.0), fl[:c.n_atoms] % 4, 4, fl[:c.n_atoms]),),
                cx.half_sphere_exposure(*c.cols, c.probe, None, fl[:c.n_atoms], 9.0),
                cx.atom_depth(*c.cols, c.probe, c.n_points))[k % 5]

    def enclose(cx, c):
        return _run(cx, c, flags=fl[:c.n_atoms] if c.n_atoms == len(fl) else None)

    with rustsasa_amd.Context(0) as fresh:
        alone = [enclose(fresh, c) for c in inputs]
    same = lambda a, b: all(g.tobytes() == w.tobytes() and g.shape == w.shape for g, w in zip(a, b))  # noqa: E731
    for k in list(range(5)) + list(range(5))[::-1]:
        for c, want in zip(inputs, alone):
            others(ctx, c, k)
            assert same(enclose(ctx, c), want), (k, c.name)
    w_off, w_words, _ = _model(inputs[0], flags=fl)
    _equal(alone[0][0], w_off)
    _equal(alone[0][1], w_words)


def test_a_call_beside_a_device_batch_in_flight(ctx):
    torch = pytest.importorskip("torch")
    import bench_workloads as bw
    c = ec.of_depth("cavity", n_points=33)
    w_off, w_words, _ = _model(c)
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
    off, words, _, _ = _run(ctx, c)
    ctx.wait()
    assert out.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    _equal(off, w_off)
    _equal(words, w_words)


def test_eight_threads_on_one_context(ctx):
    cases = [ec.of(cc.corner(33)), ec.of_depth("tiny", n_points=33), ec.of(cc.lone(65)), ec.of(cc.packed())]
    want = [_model(c)[:2] for c in cases]
    errors = []

    def work(t):
        try:
            for k in range(6):
                n = (t + k) % len(cases)
                off, words, _, _ = _run(ctx, cases[n])
                if not (np.array_equal(off, want[n][0]) and np.array_equal(words, want[n][1])):
                    errors.append((t, k, n))
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:4]
