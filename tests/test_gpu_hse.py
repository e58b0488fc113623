"""Half-sphere exposure on the GPU (rsasa_half_sphere_exposure*, k_half_sphere of hse.hip) against the exact CPU model
(hse_model.py: the header's definition in numpy float32).  The counts are integers with no order, so every comparison
is np.array_equal.  The cases (hse_cases.py, pinned by test_hse_cpu.py) sit on the kernel's own edges: exact ties at the
cutoff, sweeps that the stop rule ends after 1 .. 5 shells or that cover the grid, tie partners in the last swept shell,
shells of more than 64 rows and runs of more than 64 atoms, structures that fail the margins, cell sizes that change
under the same coordinates, every flag pattern, batches down to empty structures and up to 32-bit cell starts."""
import functools

import numpy as np
import pytest

import bench_workloads as bw
import hse_cases as hc
import hse_model as hm

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _model(name, cutoff, with_dirs=True):
    c = getattr(hc, name)()
    return hm.counts_batch(c.x, c.y, c.z, c.so, c.dirs if with_dirs else None, c.flags, cutoff)


def _run(ctx, c, cutoff, dirs="own", flags="own", probe=None, r=None):
    dirs = c.dirs if isinstance(dirs, str) else dirs
    flags = c.flags if isinstance(flags, str) else flags
    probe = c.probe if probe is None else probe
    r = c.r if r is None else r
    if len(c.so) == 2:
        return ctx.half_sphere_exposure(c.x, c.y, c.z, r, None, probe, dirs, flags, cutoff)
    return ctx.half_sphere_exposure_batch(c.x, c.y, c.z, r, None, c.so, probe, dirs, flags, cutoff)


def _equal(got, want):
    assert got[0].dtype == got[1].dtype == np.uint32 and got[0].shape == got[1].shape == want[0].shape
    bad = np.flatnonzero((got[0] != want[0]) | (got[1] != want[1]))
    assert bad.size == 0, (bad.size, bad[:5], got[0][bad[:5]], want[0][bad[:5]], got[1][bad[:5]], want[1][bad[:5]])


# ---- 1: hand cases -------------------------------------------------------------------------------------------------------

def test_hand_cases(ctx):
    c = hc.hand()
    up, down = _run(ctx, c, c.info["cutoff"])
    assert up.tolist() == c.info["up"] and down.tolist() == c.info["down"]    # self never counts, its coincident twin does
    _equal((up, down), _model("hand", c.info["cutoff"]))


# ---- 2: exact ties -------------------------------------------------------------------------------------------------------

def test_exact_ties_count_and_one_ulp_further_does_not(ctx):
    t, m = hc.ties(), hc.ties(True)
    up, down = _run(ctx, t, 13.0)
    assert up.tolist() == [3, 0, 0, 0] and not down.any()
    up, down = _run(ctx, m, 13.0)
    assert not up.any() and not down.any()
    _equal(_run(ctx, t, 13.0, flags=None), hm.counts(t.x, t.y, t.z, t.dirs, None, 13.0))
    _equal(_run(ctx, m, 13.0, flags=None), hm.counts(m.x, m.y, m.z, m.dirs, None, 13.0))


# ---- 3: the reach ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(8))
def test_cluster_at_every_reach(ctx, k):
    cutoff = hc.cluster_cutoffs()[k]
    c = hc.cluster()
    got = _run(ctx, c, cutoff)
    _equal(got, _model("cluster", cutoff))
    if k == 0:
        assert not got[0].any() and not got[1].any()                  # no two atoms coincide
    if k >= 6:
        assert np.all(got[0] + got[1] == c.n_atoms - 1)


def test_tie_partners_in_the_last_swept_shell(ctx):
    c = hc.edge()
    up, down = _run(ctx, c, hc.EDGE_CUTOFF)
    _equal((up, down), _model("edge", hc.EDGE_CUTOFF))
    for centre in (c.info["hi"], c.info["lo"]):
        assert up[centre] + down[centre] == 6                         # the six tie partners, three of them in shell 3
    above = float(np.nextafter(F(hc.EDGE_CUTOFF), F(np.inf)))
    for cutoff in (above, 4.9, 7.0):
        _equal(_run(ctx, c, cutoff), _model("edge", cutoff))
    # the partners alone with the two centres: nothing else is there to be counted
    keep = np.array([c.info["hi"], c.info["lo"]] + [a for k in ("tie", "far") for ci in (2, 3) for a, _, _ in c.info[k][ci]] + [0, 1])
    flags = np.zeros(c.n_atoms, np.uint8)
    flags[keep] = 1
    flags[[c.info["hi"], c.info["lo"]]] = 3
    up, down = _run(ctx, c, hc.EDGE_CUTOFF, flags=flags)
    _equal((up, down), hm.counts(c.x, c.y, c.z, c.dirs, flags, hc.EDGE_CUTOFF))
    assert (up + down)[[c.info["hi"], c.info["lo"]]].tolist() == [6, 6] and (up + down).sum() == 12


# ---- 4: a shell of more than 64 rows, a run of more than 64 atoms ------------------------------------------------------------

def test_crowded_cell_and_wide_shells(ctx):
    for cutoff in (13.0, 3.0):
        _equal(_run(ctx, hc.crowd(), cutoff), _model("crowd", cutoff))


# ---- 5: the whole grid -----------------------------------------------------------------------------------------------------

def test_a_radius_of_70_fails_the_margins(ctx):
    c = hc.odd_radius()
    for cutoff in (13.0, 3.28, 0.0):
        got = _run(ctx, c, cutoff)
        _equal(got, _model("odd_radius", cutoff))
        _equal(got, _model("cluster", cutoff))                          # the radius changes the grid, not the counts


def test_a_nan_coordinate_fails_the_margins_and_counts_for_nobody(ctx):
    c = hc.nan_atom()
    a = c.info["atom"]
    for cutoff in (13.0, float(c.h), hc.COVER):
        got = _run(ctx, c, cutoff)
        _equal(got, _model("nan_atom", cutoff))
        assert got[0][a] == 0 and got[1][a] == 0
    total = got[0] + got[1]                                             # at COVER: everybody but the NaN atom and oneself
    assert np.all(np.delete(total, a) == c.n_atoms - 2)


# ---- 6: independence from the cell size --------------------------------------------------------------------------------------

def test_result_does_not_depend_on_probe_or_radii(ctx):
    c = hc.cluster()
    for cutoff in (13.0, 6.56):
        base = _run(ctx, c, cutoff)
        _equal(base, _model("cluster", cutoff))
        for kw in (dict(probe=0.5), dict(probe=3.0), dict(r=c.r * F(2.0))):
            got = _run(ctx, c, cutoff, **kw)
            assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), kw


# ---- 7: flags and dirs -------------------------------------------------------------------------------------------------------

def test_flags(ctx):
    c = hc.cluster()
    n = c.n_atoms
    rng = np.random.default_rng(21)
    half = rng.permutation(n) < n // 2
    base = _run(ctx, c, 13.0, flags=None)
    _equal(base, _model("cluster", 13.0))
    _equal(_run(ctx, c, 13.0, flags=np.full(n, 3, np.uint8)), base)
    _equal(_run(ctx, c, 13.0, flags=np.full(n, 0xFB, np.uint8)), base)            # the other bits are ignored
    for name, flags in (("centres only", np.full(n, 2, np.uint8)), ("partners only", np.full(n, 1, np.uint8)),
                        ("disjoint", np.where(half, 1, 2).astype(np.uint8)),
                        ("mixed", rng.integers(0, 4, n).astype(np.uint8)),
                        ("one in eight", np.where(np.arange(n) % 8 == 0, 3, 0).astype(np.uint8))):
        got = _run(ctx, c, 13.0, flags=flags)
        _equal(got, hm.counts(c.x, c.y, c.z, c.dirs, flags, 13.0))
        assert not (got[0] + got[1])[(flags & 2) == 0].any(), name                 # rows of non-centres are zero
        if name in ("centres only", "partners only"):
            assert not got[0].any() and not got[1].any()
    got = _run(ctx, c, 13.0, flags=np.where(half, 1, 2).astype(np.uint8))
    assert (got[0] + got[1])[~half].min() > 0


def test_dirs(ctx):
    c = hc.cluster()
    n = c.n_atoms
    contact = _model("cluster", 13.0, False)
    got = _run(ctx, c, 13.0, dirs=None)
    _equal(got, contact)
    assert not got[1].any()
    _equal(_run(ctx, c, 13.0, dirs=np.zeros((n, 3), F)), got)                     # zero directions: side +0, all up
    own = _run(ctx, c, 13.0)
    assert np.array_equal(own[0] + own[1], got[0])                                # up + down is the contact number
    d = c.dirs.copy()
    d[::7, 1] = np.nan
    d[3::7] = 0.0
    d[5::7] *= F(1e30)
    nan = _run(ctx, c, 13.0, dirs=d)
    _equal(nan, hm.counts(c.x, c.y, c.z, d, None, 13.0))
    assert not nan[0][::7].any() and np.array_equal(nan[1][::7], got[0][::7])     # a NaN component: everybody down
    assert not nan[1][3::7].any()
    vectors, free, _ = ctx.exposure_vectors(*c.cols, c.probe, 100)
    ev = _run(ctx, c, 13.0, dirs=vectors)
    _equal(ev, hm.counts(c.x, c.y, c.z, vectors, None, 13.0))
    exposed = free > 0
    assert exposed.sum() > 100 and ev[0][exposed].mean() < ev[1][exposed].mean()   # fewer atoms on the exposed side


# ---- 8: batches --------------------------------------------------------------------------------------------------------------

def _parts_equal_the_batch(ctx, c, cutoff, got):
    for s in range(len(c.so) - 1):
        p = hc.part(c, s)
        b, e = int(c.so[s]), int(c.so[s + 1])
        one = _run(ctx, p, cutoff)
        assert np.array_equal(one[0], got[0][b:e]) and np.array_equal(one[1], got[1][b:e]), s


def test_interleaved_structures_never_count_each_other(ctx):
    c = hc.interleaved()
    got = _run(ctx, c, 13.0)
    _equal(got, _model("interleaved", 13.0))
    _parts_equal_the_batch(ctx, c, 13.0, got)
    both = hm.counts(c.x, c.y, c.z, c.dirs, None, 13.0)                   # as one structure: everybody has more partners
    assert np.all(got[0] + got[1] < both[0] + both[1])


def test_empty_and_one_atom_structures(ctx):
    c = hc.tiny_batch()
    got = _run(ctx, c, 13.0)
    _equal(got, _model("tiny_batch", 13.0))
    _parts_equal_the_batch(ctx, c, 13.0, got)
    e = np.zeros(0, F)
    for so in ([0], [0, 0, 0]):
        out = ctx.half_sphere_exposure_batch(e, e, e, e, None, np.array(so, np.uint32), 1.4, None, None, 13.0)
        assert all(len(a) == 0 for a in out)
    assert all(len(a) == 0 for a in ctx.half_sphere_exposure(e, e, e, e))
    one = ctx.half_sphere_exposure(np.ones(1, F), np.ones(1, F), np.ones(1, F), np.ones(1, F))
    assert one[0].tolist() == [0] and one[1].tolist() == [0]


def test_batch_with_a_structure_of_65536_atoms(ctx):
    c = hc.tail_batch()
    got = _run(ctx, c, 13.0)
    want = _model("tail_batch", 13.0)
    _equal(got, want)
    b = int(c.so[-2])
    centres = c.info["centres"]
    assert (got[0] + got[1])[b:][centres].min() >= 1 and (got[0] + got[1])[b:].sum() == (got[0] + got[1])[b:][centres].sum()
    big = hc.part(c, len(c.so) - 2)
    alone = _run(ctx, big, 13.0)
    assert np.array_equal(alone[0], got[0][b:]) and np.array_equal(alone[1], got[1][b:])
    for s in range(len(c.so) - 2):
        p = hc.part(c, s)
        one = _run(ctx, p, 13.0)
        lo, hi = int(c.so[s]), int(c.so[s + 1])
        assert np.array_equal(one[0], got[0][lo:hi]) and np.array_equal(one[1], got[1][lo:hi])


# ---- 9: permutation ------------------------------------------------------------------------------------------------------------

def test_a_permutation_of_the_atoms_permutes_the_rows(ctx):
    c = hc.crowd()
    perm = np.random.default_rng(23).permutation(c.n_atoms)
    flags = np.random.default_rng(24).integers(0, 4, c.n_atoms).astype(np.uint8)
    base = _run(ctx, c, 13.0, flags=flags)
    got = ctx.half_sphere_exposure(c.x[perm], c.y[perm], c.z[perm], c.r[perm], None, c.probe, c.dirs[perm], flags[perm], 13.0)
    assert np.array_equal(got[0], base[0][perm]) and np.array_equal(got[1], base[1][perm])


# ---- 10: one context -------------------------------------------------------------------------------------------------------------

def _family_calls(ctx, c):
    import rustsasa_amd
    groups = (np.arange(c.n_atoms) % 5).astype(np.uint32)
    link = rustsasa_amd.default_link(c.r, c.probe, 100)
    return [lambda: ctx.precompute_neighbors(*c.cols, c.probe),
            lambda: ctx.accessible_points(*c.cols, c.probe, 100),
            lambda: ctx.exposure_vectors(*c.cols, c.probe, 100),
            lambda: ctx.atom_depth(*c.cols, c.probe, 100),
            lambda: ctx.surface_components(*c.cols, c.probe, 100, link),
            lambda: ctx.contact_points(*c.cols, c.probe, 100),
            lambda: ctx.group_contacts(*c.cols, groups, c.probe, 100),
            lambda: ctx.calculate_sasa_soa(*c.cols, c.probe, 100)]


def test_between_calls_of_every_other_family(ctx):
    import rustsasa_amd
    c, t = hc.edge(), hc.tiny_batch()
    want, want_t = _model("edge", hc.EDGE_CUTOFF), _model("tiny_batch", 13.0)
    with rustsasa_amd.Context(0) as fresh:
        alone = [call() for call in _family_calls(fresh, c)]
    tup = lambda v: (v,) if isinstance(v, np.ndarray) else tuple(v)  # noqa: E731
    for call, ref in zip(_family_calls(ctx, c), alone):
        before = call()
        _equal(_run(ctx, c, hc.EDGE_CUTOFF), want)
        _equal(_run(ctx, t, 13.0), want_t)
        after = call()
        assert len(tup(before)) == len(tup(after)) == len(tup(ref))
        for a, b_, r in zip(tup(before), tup(after), tup(ref)):
            assert a.tobytes() == b_.tobytes() == r.tobytes()


def test_argument_errors_leave_the_context_usable(ctx):
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    lib = _capi.load()
    c = hc.edge()
    n = c.n_atoms
    want = _model("edge", hc.EDGE_CUTOFF)
    up, down = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    cols = (ptr(c.x), ptr(c.y), ptr(c.z), ptr(c.r), None)
    so = np.array([0, n], np.uint32)
    falling = np.array([0, 40, 30, n], np.uint32)
    bad, ok = _capi.RSASA_ERR_INVALID_ARGUMENT, _capi.RSASA_OK
    one, many = lib.rsasa_half_sphere_exposure, lib.rsasa_half_sphere_exposure_batch
    tail = (ptr(c.dirs), None, hc.EDGE_CUTOFF, ptr(up), ptr(down))
    cut = "cutoff must be finite and not negative"
    errors = [
        (lambda: one(ctx._h, *cols, n, c.probe, ptr(c.dirs), None, float("nan"), ptr(up), ptr(down)), bad, cut),
        (lambda: one(ctx._h, *cols, n, c.probe, ptr(c.dirs), None, float("inf"), ptr(up), ptr(down)), bad, cut),
        (lambda: one(ctx._h, *cols, n, c.probe, ptr(c.dirs), None, -1.0, ptr(up), ptr(down)), bad, cut),
        (lambda: many(ctx._h, *cols, ptr(so), 1, c.probe, ptr(c.dirs), None, -1e-30, ptr(up), ptr(down)), bad, cut),
        (lambda: one(ctx._h, *cols, n, c.probe, ptr(c.dirs), None, hc.EDGE_CUTOFF, None, ptr(down)), bad, "NULL argument"),
        (lambda: one(ctx._h, *cols, n, c.probe, ptr(c.dirs), None, hc.EDGE_CUTOFF, ptr(up), None), bad, "NULL argument"),
        (lambda: many(ctx._h, *cols, ptr(so), 1, c.probe, ptr(c.dirs), None, hc.EDGE_CUTOFF, None, ptr(down)), bad, "NULL argument"),
        (lambda: one(ctx._h, None, ptr(c.y), ptr(c.z), ptr(c.r), None, n, c.probe, *tail), bad, "NULL argument"),
        (lambda: many(ctx._h, *cols, None, 1, c.probe, *tail), bad, "NULL argument"),
        (lambda: many(ctx._h, *cols, ptr(falling), 3, c.probe, *tail), bad, "structure_offsets must be non-decreasing"),
        (lambda: many(ctx._h, *cols, ptr(so[1:]), 0, c.probe, *tail), ok, ""),                     # no structure: OK
        (lambda: one(ctx._h, *cols, n, -5.0, *tail), bad, None),                                    # probe + max_r <= 0
    ]
    for k, (call, status, message) in enumerate(errors):
        assert call() == status, k
        if message:
            assert message in lib.rsasa_context_last_error(ctx._h).decode(), (k, lib.rsasa_context_last_error(ctx._h))
        assert not up.any() and not down.any(), k                     # nothing was written
        _equal(_run(ctx, c, hc.EDGE_CUTOFF), want)                    # and the next call is right
    # no atoms: OK with every pointer NULL; -0.0 is 0
    assert one(ctx._h, None, None, None, None, None, 0, 1.4, None, None, 13.0, None, None) == ok
    assert one(ctx._h, *cols, n, c.probe, ptr(c.dirs), None, -0.0, ptr(up), ptr(down)) == ok
    assert not up.any() and not down.any()
    assert one(ctx._h, *cols, n, c.probe, *tail) == ok
    _equal((up, down), want)


def test_python_argument_checks(ctx):
    c = hc.hand()
    with pytest.raises(ValueError):
        ctx.half_sphere_exposure(*c.cols, dirs=c.dirs[:, :2])
    with pytest.raises(ValueError):
        ctx.half_sphere_exposure(*c.cols, flags=c.flags[:3])
    with pytest.raises(ValueError):
        ctx.half_sphere_exposure(*c.cols, flags=c.flags.astype(np.float32))
    with pytest.raises(ValueError):
        ctx.half_sphere_exposure(*c.cols, flags=np.full(c.n_atoms, 256))
    got = ctx.half_sphere_exposure(*c.cols, dirs=c.dirs.astype(np.float64), flags=c.flags.astype(np.int64), cutoff=5.0)
    assert got[0].tolist() == c.info["up"] and got[1].tolist() == c.info["down"]


def test_an_infinite_coordinate_is_refused_and_the_next_call_is_right(ctx):
    import rustsasa_amd
    c = hc.edge()
    x = c.x.copy()
    x[5] = np.inf
    for call in (lambda: ctx.half_sphere_exposure(x, c.y, c.z, c.r, None, c.probe, c.dirs, None, hc.EDGE_CUTOFF),
                 lambda: ctx.half_sphere_exposure_batch(x, c.y, c.z, c.r, None, c.so, c.probe, c.dirs, None, hc.EDGE_CUTOFF)):
        with pytest.raises(rustsasa_amd.RsasaError) as e:
            call()
        assert e.value.status == -5
        _equal(_run(ctx, c, hc.EDGE_CUTOFF), _model("edge", hc.EDGE_CUTOFF))


def test_beside_a_device_batch_in_flight(ctx):
    torch = pytest.importorskip("torch")
    c = hc.crowd()
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
    got = _run(ctx, c, 13.0)
    ctx.wait()
    assert out.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    _equal(got, _model("crowd", 13.0))
