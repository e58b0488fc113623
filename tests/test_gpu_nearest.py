"""The k nearest atoms on the GPU (rsasa_nearest_atoms*, k_nearest / k_nearest_gather of nearest.hip) against the exact CPU
model (nearest_model.py: the within-lists of within_model.py, cut at k).  Every list is sorted by a key of distinct values
and cut at a fixed place, so every comparison is exact: the offsets equal, the entries equal as bytes.  The cases sit on
the sweep's edges (hse_cases.py), on the sort's (within_cases.py) and on what k_nearest adds (nearest_cases.py, pinned by
test_nearest_cpu.py): a stop rule fed by what the sweep holds, a staging compacted when the next batch might not fit,
and cuts inside classes of equal d2."""
import functools

import numpy as np
import pytest

import bench_workloads as bw
import hse_cases as hc
import nearest_cases as nc
import nearest_model as nm
import within_cases as wc
import within_model as wm

pytestmark = pytest.mark.gpu

F = np.float32
FLT_MAX = float(np.finfo(F).max)
INF = float("inf")


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _1jcd():
    import structio as sio
    atoms = [a for a in sio.read_structure(sio.data_path("1jcd.pdb")) if not a.hetero]
    x, y, z, r, _ = sio.soa_vdw(atoms)
    return hc.Case("1jcd", *(np.ascontiguousarray(a, F) for a in (x, y, z, r)), np.array([0, len(x)], np.uint32))


def _case(name):
    return _1jcd() if name == "1jcd" else nc.case(name)


@functools.lru_cache(maxsize=None)
def _within(name, cutoff):
    """The within-lists of a named case with its own flags (cutoff None: +inf), computed once and left unchanged."""
    c = _case(name)
    return wm.lists_batch(c.x, c.y, c.z, c.so, c.flags, INF if cutoff is None else cutoff)


def _model(name, k, cutoff=None):
    return nm.truncate(*_within(name, cutoff), k)


def _run(ctx, c, k, cutoff=None, flags="own", probe=None, r=None):
    flags = c.flags if isinstance(flags, str) else flags
    probe = c.probe if probe is None else probe
    r = c.r if r is None else r
    if len(c.so) == 2:
        return ctx.nearest_atoms(c.x, c.y, c.z, r, None, probe, k, flags, cutoff)
    return ctx.nearest_atoms_batch(c.x, c.y, c.z, r, None, c.so, probe, k, flags, cutoff)


def _equal(got, want):
    assert got[0].dtype == np.uint64 and got[1].dtype == wm.WITHIN_DTYPE and got[0].shape == want[0].shape
    bad = np.flatnonzero(got[0] != want[0])
    assert bad.size == 0, ("offsets", bad.size, bad[:5], got[0][bad[:5]], want[0][bad[:5]])
    if got[1].tobytes() != want[1].tobytes():
        k = np.flatnonzero((got[1]["d2"].view(np.uint32) != want[1]["d2"].view(np.uint32)) | (got[1]["idx"] != want[1]["idx"]))
        atom = np.searchsorted(want[0], k[:5], side="right") - 1
        raise AssertionError(("entries", k.size, k[:5], atom, got[1][k[:5]], want[1][k[:5]]))


def _check(ctx, name, k, cutoff=None):
    got = _run(ctx, _case(name), k, cutoff)
    _equal(got, _model(name, k, cutoff))
    return got


def _list(got, i):
    return got[1][int(got[0][i]):int(got[0][i + 1])]


# ---- 1: a protein ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,cutoff", [(1, None), (16, None), (30, None), (64, None), (256, None), (30, 4.5), (30, 8.0), (256, 200.0)])
def test_1jcd(ctx, k, cutoff):
    c = _1jcd()
    got = _check(ctx, "1jcd", k, cutoff)
    n = wm.lengths(got[0])
    if cutoff is None or cutoff == 200.0:
        assert np.all(n == min(k, c.n_atoms - 1))
    else:
        assert n.max() <= k and (n.min() < k or cutoff > 4.5)            # short lists under the cutoff


# ---- 2: hand lists, exact ties -------------------------------------------------------------------------------------------------

def test_hand_lists(ctx):
    c = hc.hand()
    full = [(0.0, 4), (4.0, 2), (9.0, 1), (9.0, 3), (49.0, 5)]
    for k in (1, 2, 3, 4, 5, 6, 256):
        off, ent = _run(ctx, c, k)
        n = min(k, 5)
        assert off.tolist() == [0, n, n, n, n, 2 * n, 2 * n]
        assert ent[:n].tolist() == full[:n] and ent[n:].tolist() == [(0.0, 0)] + full[1:n]
    off, ent = _run(ctx, c, 3, 5.0)
    assert ent[:3].tolist() == [(0.0, 4), (4.0, 2), (9.0, 1)]           # the tie at 9 is cut: the smaller idx stays
    off, ent = _run(ctx, c, 256, 5.0)
    assert off.tolist() == [0, 4, 4, 4, 4, 8, 8] and ent[:4].tolist() == full[:4]


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_exact_ties_at_the_cutoff(ctx, k):
    t, m = hc.ties(), hc.ties(True)
    off, ent = _run(ctx, t, k, 13.0)
    assert off.tolist() == [0] + [min(k, 3)] * 4 and ent.tolist() == [(169.0, 1), (169.0, 2), (169.0, 3)][:k]
    assert _run(ctx, m, k, 13.0)[0][-1] == 0                            # one ulp further out: outside the cutoff
    for c in (t, m):
        _equal(_run(ctx, c, k, 13.0, flags=None), nm.lists(c.x, c.y, c.z, None, k, 13.0))
        _equal(_run(ctx, c, k, None, flags=None), nm.lists(c.x, c.y, c.z, None, k))


# ---- 3: the stop rule ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", nc.EDGE_KS)
def test_the_kth_neighbour_in_the_last_swept_shell(ctx, k):
    c = nc.knn_edge(k)
    got = _run(ctx, c, k)
    _equal(got, nm.lists(c.x, c.y, c.z, c.flags, k))
    for gr in c.info["groups"]:                                         # all six directions
        li = _list(got, gr["centre"])
        assert len(li) == k and li["idx"][-1] == gr["true_kth"] and gr["diagonal"] not in li["idx"]


# ---- 4: cuts inside classes of equal d2 ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", nc.TIE_KS)
def test_equal_d2_is_cut_by_idx(ctx, k):
    c = wc.equal_d2()
    got = _check(ctx, "equal_d2", k)
    full = _list(_within("equal_d2", None), c.info["centre"])
    assert _list(got, c.info["centre"]).tobytes() == full[:k].tobytes() and len(full) == 80


# ---- 5, 6: the staging and its compaction -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [16, 256])
def test_coincident_atoms_keep_the_smallest_idx(ctx, k):
    c = wc.coincident()
    got = _check(ctx, "coincident", k)
    assert np.all(wm.lengths(got[0]) == k)
    for s, n in enumerate(c.info["n"]):
        b, e = int(c.so[s]), int(c.so[s + 1])
        same = np.flatnonzero((c.x[b:e] == np.median(c.x[b:e])) & (c.y[b:e] == np.median(c.y[b:e])) & (c.z[b:e] == np.median(c.z[b:e])))
        for i in (int(same[0]), int(same[-1])):                          # k coincident atoms at d2 0: idx alone decides
            li = _list(got, b + i)
            assert not li["d2"].any() and li["idx"].tolist() == same[same != i][:k].tolist()
    _check(ctx, "coincident", k, 0.0)
    _check(ctx, "coincident", k, 2.0)


@pytest.mark.parametrize("k", nc.STAGE_KS)
def test_staging_at_the_compaction_trigger(ctx, k):
    c = nc.knn_stage()
    got = _check(ctx, "knn_stage", k)
    assert np.array_equal(wm.lengths(got[0]), np.where((c.flags & 2) != 0, k, 0))


# ---- 7, 8, 9: the sweep's edges ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cluster", "crowd"])
@pytest.mark.parametrize("k", [1, 64, 256])
def test_cluster_and_crowd(ctx, name, k):
    got = _check(ctx, name, k)
    assert np.all(wm.lengths(got[0]) == k)
    _check(ctx, name, k, 13.0)


def test_the_whole_grid_when_the_margins_fail(ctx):
    c = hc.cluster()
    for k in (30, 256):
        got = _check(ctx, "odd_radius", k)
        _equal(got, _model("cluster", k))                               # the radius changes the grid, not the lists
        _equal(_run(ctx, c, k, probe=-0.25), got)                       # a negative probe fails the margins too
        _equal(_run(ctx, c, k, probe=3.0), got)
        _equal(_run(ctx, c, k, r=c.r * F(2.0)), got)


def test_a_nan_coordinate_is_in_nobodys_list(ctx):
    c = hc.nan_atom()
    a = c.info["atom"]
    for k, cutoff in ((30, None), (256, None), (30, 13.0)):
        off, ent = _check(ctx, "nan_atom", k, cutoff)
        assert off[a] == off[a + 1] and not (ent["idx"] == a).any() and not np.isnan(ent["d2"]).any()
    assert np.all(np.delete(wm.lengths(_check(ctx, "nan_atom", 64)[0]), a) == 64)


# ---- 10: flags -------------------------------------------------------------------------------------------------------------------------

def test_flags(ctx):
    c = hc.part(hc.interleaved(), 0)                                     # every other atom of the cluster
    n = c.n_atoms
    rng = np.random.default_rng(21)
    half = rng.permutation(n) < n // 2
    k = 30
    base = _run(ctx, c, k, flags=None)
    _equal(base, nm.lists(c.x, c.y, c.z, None, k))
    _equal(_run(ctx, c, k, flags=np.full(n, 3, np.uint8)), base)
    _equal(_run(ctx, c, k, flags=np.full(n, 0xFB, np.uint8)), base)                # the other bits are ignored
    for name, flags in (("centres only", np.full(n, 2, np.uint8)), ("partners only", np.full(n, 1, np.uint8)),
                        ("neither", np.zeros(n, np.uint8)), ("disjoint", np.where(half, 1, 2).astype(np.uint8)),
                        ("mixed", rng.integers(0, 4, n).astype(np.uint8)),
                        ("one in eight", np.where(np.arange(n) % 8 == 0, 3, 0).astype(np.uint8)),
                        ("one centre in eight", np.where(np.arange(n) % 8 == 5, 3, 1).astype(np.uint8))):
        for cutoff in (None, 8.0):
            got = _run(ctx, c, k, cutoff, flags=flags)
            _equal(got, nm.lists(c.x, c.y, c.z, flags, k, cutoff))
            assert not wm.lengths(got[0])[(flags & 2) == 0].any(), name                  # non-centres have empty lists
            assert np.all((flags[got[1]["idx"]] & 1) != 0), name                         # only partners are listed
            if name in ("centres only", "partners only", "neither"):
                assert got[0][-1] == 0
            if name == "disjoint" and cutoff is None:                                    # partner-only and centre-only atoms
                assert np.all(wm.lengths(got[0])[~half] == k)


# ---- 11 - 14: batches ----------------------------------------------------------------------------------------------------------------------

def _parts_equal_the_batch(ctx, c, k, got, cutoff=None):
    for s in range(len(c.so) - 1):
        b, e = int(c.so[s]), int(c.so[s + 1])
        off, ent = _run(ctx, hc.part(c, s), k, cutoff)
        assert np.array_equal(off + got[0][b], got[0][b:e + 1]), s
        assert ent.tobytes() == got[1][int(got[0][b]):int(got[0][e])].tobytes(), s


def test_empty_one_atom_and_short_structures(ctx):
    c = hc.tiny_batch()
    sizes = np.diff(c.so.astype(np.int64))
    for k in (1, 2, 16, 39, 40, 256):
        got = _check(ctx, "tiny_batch", k)
        assert np.array_equal(wm.lengths(got[0]), np.minimum(np.repeat(sizes, sizes) - 1, k))   # lists of n - 1 below k + 1 atoms
    _parts_equal_the_batch(ctx, c, 16, _check(ctx, "tiny_batch", 16))
    e = np.zeros(0, F)
    for so in ([0], [0, 0, 0]):
        off, ent = ctx.nearest_atoms_batch(e, e, e, e, None, np.array(so, np.uint32))
        assert off.tolist() == [0] and len(ent) == 0
    off, ent = ctx.nearest_atoms(e, e, e, e)
    assert off.tolist() == [0] and len(ent) == 0
    off, ent = ctx.nearest_atoms(np.ones(1, F), np.ones(1, F), np.ones(1, F), np.ones(1, F))
    assert off.tolist() == [0, 0] and len(ent) == 0


def test_structures_in_the_same_space_never_list_each_other(ctx):
    for name in ("overlap", "interleaved"):
        for k, cutoff in ((30, None), (64, 8.0)):
            got = _check(ctx, name, k, cutoff)
            assert (got[1]["d2"] > 0).all()                             # overlap: the twin at d2 = 0 is another structure's
        _parts_equal_the_batch(ctx, _case(name), 64, got, 8.0)


def test_batch_with_a_structure_of_65536_atoms(ctx):
    c = hc.tail_batch()
    k = 30
    got = _run(ctx, c, k)
    _equal(got, nm.lists_batch(c.x, c.y, c.z, c.so, c.flags, k, by_sort=True))
    b = int(c.so[-2])
    n = wm.lengths(got[0])[b:]
    assert np.all(n[c.info["centres"]] == k) and n.sum() == k * len(c.info["centres"])
    off, ent = _run(ctx, hc.part(c, len(c.so) - 2), k)
    assert np.array_equal(off + got[0][b], got[0][b:]) and ent.tobytes() == got[1][int(got[0][b]):].tobytes()


# ---- 15: the cutoff's ends -------------------------------------------------------------------------------------------------------------

def test_cutoff_zero_flt_max_and_infinity(ctx):
    for name in ("crowd", "tiny_batch", "equal_d2"):
        c = _case(name)
        assert _check(ctx, name, 16, 0.0)[0][-1] == 0                   # all lists empty
        none = _check(ctx, name, 16)
        for cutoff in (FLT_MAX, INF):                                   # c2 = +inf either way
            _equal(_run(ctx, c, 16, cutoff), none)
    assert _run(ctx, hc.crowd(), 16, -0.0)[0][-1] == 0


# ---- 16 - 18: the C interface ------------------------------------------------------------------------------------------------------------

def _c_calls(ctx, c, so=None):
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    lib = _capi.load()
    cols = (ptr(c.x), ptr(c.y), ptr(c.z), ptr(c.r), None)
    so = np.array([0, c.n_atoms], np.uint32) if so is None else so
    one = lambda fl, k, cut, o, e, cap: lib.rsasa_nearest_atoms(ctx._h, *cols, c.n_atoms, c.probe, fl, k, cut, o, e, cap)  # noqa: E731
    many = lambda fl, k, cut, o, e, cap: lib.rsasa_nearest_atoms_batch(ctx._h, *cols, ptr(so), len(so) - 1, c.probe, fl, k, cut, o, e, cap)  # noqa: E731
    return lib, one, many


def test_sizing_protocol(ctx):
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    c = hc.crowd()
    n = c.n_atoms
    k = 30
    flags = np.where(np.arange(n) % 3 == 0, 3, 1).astype(np.uint8)
    centres = int(((flags & 2) != 0).sum())
    lib, one, many = _c_calls(ctx, c)
    for cutoff in (3.0, INF):
        want = nm.lists(c.x, c.y, c.z, flags, k, cutoff)
        total = int(want[0][-1])
        assert (total < centres * k) == (cutoff == 3.0)                 # short lists under the cutoff
        for call in (one, many):
            for cap, buf in ((0, None), (0, total), (total - 1, total), (total, None)):
                off = np.full(n + 1, 0xAAAAAAAAAAAAAAAA, np.uint64)
                ent = None if buf is None else np.full(buf, 0xAA, np.uint8).repeat(8).view(wm.WITHIN_DTYPE)
                assert call(ptr(flags), k, cutoff, ptr(off), ptr(ent), cap) == _capi.RSASA_ERR_BUFFER_TOO_SMALL, (cap, buf)
                assert "out_entries" in lib.rsasa_context_last_error(ctx._h).decode()
                assert np.array_equal(off, want[0])                        # the offsets are written
                assert ent is None or np.all(ent.view(np.uint8) == 0xAA)   # and nothing else
            for cap in (total, centres * k, centres * k + 7):              # exactly offsets[-1]; centres * k always suffices
                off = np.zeros(n + 1, np.uint64)
                ent = np.full(cap, 0xAA, np.uint8).repeat(8).view(wm.WITHIN_DTYPE)
                assert call(ptr(flags), k, cutoff, ptr(off), ptr(ent), cap) == _capi.RSASA_OK
                _equal((off, ent[:total]), want)
                assert np.all(ent[total:].view(np.uint8) == 0xAA)
    # every list empty: a NULL buffer is still too small (as in rsasa_atoms_within), one of no entries is not
    off = np.ones(n + 1, np.uint64)
    assert one(None, k, 0.0, ptr(off), None, 0) == _capi.RSASA_ERR_BUFFER_TOO_SMALL and not off.any()
    off = np.ones(n + 1, np.uint64)
    ent = np.zeros(1, wm.WITHIN_DTYPE)
    assert one(None, k, 0.0, ptr(off), ptr(ent), 0) == _capi.RSASA_OK and not off.any()
    # no atoms: out_offsets[0] = 0
    off = np.ones(1, np.uint64)
    assert lib.rsasa_nearest_atoms(ctx._h, None, None, None, None, None, 0, 1.4, None, 16, INF, ptr(off), None, 0) == _capi.RSASA_OK
    assert off[0] == 0


def test_argument_errors_leave_the_context_usable(ctx):
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    c = hc.edge()
    n = c.n_atoms
    k = 16
    want = nm.lists(c.x, c.y, c.z, None, k)
    off = np.zeros(n + 1, np.uint64)
    ent = np.zeros(int(want[0][-1]), wm.WITHIN_DTYPE)
    lib, one, many = _c_calls(ctx, c)
    cols = (ptr(c.x), ptr(c.y), ptr(c.z), ptr(c.r), None)
    falling = np.array([0, 40, 30, n], np.uint32)
    out = (ptr(off), ptr(ent), len(ent))
    cut, bad_k = "cutoff must be +inf or finite, and not negative", "k must be in [1, 256]"
    errors = [
        (lambda: one(None, 0, INF, *out), bad_k),
        (lambda: one(None, 257, INF, *out), bad_k),
        (lambda: many(None, 0, 8.0, *out), bad_k),
        (lambda: many(None, 257, 8.0, *out), bad_k),
        (lambda: one(None, k, float("nan"), *out), cut),
        (lambda: one(None, k, -1.0, *out), cut),
        (lambda: many(None, k, float("nan"), *out), cut),
        (lambda: many(None, k, -1e-30, *out), cut),
        (lambda: many(None, k, -INF, *out), cut),
        (lambda: one(None, k, INF, None, ptr(ent), len(ent)), "NULL argument"),
        (lambda: lib.rsasa_nearest_atoms(ctx._h, None, ptr(c.y), ptr(c.z), ptr(c.r), None, n, c.probe, None, k, INF, *out), "NULL argument"),
        (lambda: lib.rsasa_nearest_atoms_batch(ctx._h, *cols, None, 1, c.probe, None, k, INF, *out), "NULL argument"),
        (lambda: lib.rsasa_nearest_atoms_batch(ctx._h, *cols, ptr(falling), 3, c.probe, None, k, INF, *out),
         "structure_offsets must be non-decreasing"),
        (lambda: lib.rsasa_nearest_atoms(ctx._h, *cols, n, -5.0, None, k, INF, *out), None),                # probe + max_r <= 0
    ]
    for e, (call, message) in enumerate(errors):
        assert call() == _capi.RSASA_ERR_INVALID_ARGUMENT, e
        if message:
            assert message in lib.rsasa_context_last_error(ctx._h).decode(), (e, lib.rsasa_context_last_error(ctx._h))
        assert not off.any() and not ent.view(np.uint8).any(), e         # nothing was written
        _equal(_run(ctx, c, k), want)                                    # and the next call is right
    assert one(None, k, INF, *out) == _capi.RSASA_OK
    _equal((off, ent), want)
    assert many(None, k, INF, *out) == _capi.RSASA_OK
    _equal((off, ent), want)


def test_an_infinite_coordinate_is_refused_and_the_next_call_is_right(ctx):
    import rustsasa_amd
    c = hc.edge()
    x = c.x.copy()
    x[5] = np.inf
    want = nm.lists(c.x, c.y, c.z, None, 16)
    for call in (lambda: ctx.nearest_atoms(x, c.y, c.z, c.r, None, c.probe, 16),
                 lambda: ctx.nearest_atoms_batch(x, c.y, c.z, c.r, None, c.so, c.probe, 16)):
        with pytest.raises(rustsasa_amd.RsasaError) as e:
            call()
        assert e.value.status == -5
        _equal(_run(ctx, c, 16, flags=None), want)


# ---- 19: the relation to atoms_within, on the GPU alone ----------------------------------------------------------------------------------

def test_the_lists_are_atoms_within_cut_at_k(ctx):
    j, c = _1jcd(), hc.cluster()
    flags = np.where(np.arange(c.n_atoms) % 4 == 0, 3, 1).astype(np.uint8)
    for case, fl, cutoff, ks in ((j, None, 8.0, (1, 30, 64, 256)), (c, flags, hc.COVER, (1, 64, 256))):
        within = ctx.atoms_within(case.x, case.y, case.z, case.r, None, case.probe, fl, cutoff)
        for k in ks:
            _equal(_run(ctx, case, k, cutoff, flags=fl), nm.truncate(*within, k))
    assert wm.lengths(within[0]).max() == c.n_atoms - 1                 # the covering cutoff: every partner is listed


# ---- 20: one context ------------------------------------------------------------------------------------------------------------------------

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
            lambda: ctx.half_sphere_exposure(*c.cols, c.probe, c.dirs, None, 13.0),
            lambda: ctx.atoms_within(*c.cols, c.probe, None, 8.0),
            lambda: ctx.calculate_sasa_soa(*c.cols, c.probe, 100)]


def test_between_calls_of_every_other_family(ctx):
    """The rows, the ranks (the neighbour runs' idx_map buffer) and the scan are shared scratch: every other family's
    results are the same before and after, and the same as on a context that never ran this call."""
    import rustsasa_amd
    c, t = hc.edge(), hc.tiny_batch()
    flags = np.where(np.arange(c.n_atoms) % 3 == 1, 3, 1).astype(np.uint8)
    want, want_t = nm.lists(c.x, c.y, c.z, flags, 16), _model("tiny_batch", 16)
    tup = lambda v: (v,) if isinstance(v, np.ndarray) else tuple(v)  # noqa: E731
    with rustsasa_amd.Context(0) as fresh:
        alone = [call() for call in _family_calls(fresh, c)]
    for call, ref in zip(_family_calls(ctx, c), alone):
        before = call()
        _equal(_run(ctx, c, 16, flags=flags), want)
        _equal(_run(ctx, t, 16), want_t)
        after = call()
        assert len(tup(before)) == len(tup(after)) == len(tup(ref))
        for a, b_, r in zip(tup(before), tup(after), tup(ref)):
            assert a.tobytes() == b_.tobytes() == r.tobytes()
    act = np.arange(0, c.n_atoms, 3, dtype=np.uint32)                    # idx_map of a neighbour run, then the ranks, then idx_map
    nb = tup(ctx.precompute_neighbors(*c.cols, c.probe, active_indices=act))
    _equal(_run(ctx, c, 16, flags=flags), want)
    for a, b_ in zip(nb, tup(ctx.precompute_neighbors(*c.cols, c.probe, active_indices=act))):
        assert a.tobytes() == b_.tobytes()


def test_beside_a_device_batch_in_flight(ctx):
    torch = pytest.importorskip("torch")
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
    got = _run(ctx, hc.crowd(), 64)
    ctx.wait()
    assert out.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    _equal(got, _model("crowd", 64))
