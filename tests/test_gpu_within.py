"""Atoms within a cutoff on the GPU (rsasa_atoms_within*, k_within_count / k_within_fill of within.hip) against the exact
CPU model (within_model.py: the header's definition in numpy float32).  Every list is sorted by a key of distinct
values, so every comparison is exact: the offsets equal, the entries equal as bytes.  The cases sit on the sweep's edges
(hse_cases.py) and on the fill's (within_cases.py, pinned by test_within_cpu.py): lists one short of, at and above the LDS
staging, the powers of two the sort pads to, the tiles of the long lists' ranking, and keys that tie in d2."""
import functools

import numpy as np
import pytest

import bench_workloads as bw
import hse_cases as hc
import within_cases as wc
import within_model as wm

pytestmark = pytest.mark.gpu

F = np.float32
FLT_MAX = float(np.finfo(F).max)


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


def _case(name):
    return getattr(wc, name)() if hasattr(wc, name) and name not in ("Case", "_case") else getattr(hc, name)()


@functools.lru_cache(maxsize=None)
def _model(name, cutoff, upper=False):
    c = _case(name)
    return wm.lists_batch(c.x, c.y, c.z, c.so, c.flags, cutoff, upper)


def _run(ctx, c, cutoff, upper=False, flags="own", probe=None, r=None):
    flags = c.flags if isinstance(flags, str) else flags
    probe = c.probe if probe is None else probe
    r = c.r if r is None else r
    if len(c.so) == 2:
        return ctx.atoms_within(c.x, c.y, c.z, r, None, probe, flags, cutoff, upper)
    return ctx.atoms_within_batch(c.x, c.y, c.z, r, None, c.so, probe, flags, cutoff, upper)


def _equal(got, want):
    assert got[0].dtype == np.uint64 and got[1].dtype == wm.WITHIN_DTYPE and got[0].shape == want[0].shape
    bad = np.flatnonzero(got[0] != want[0])
    assert bad.size == 0, ("offsets", bad.size, bad[:5], got[0][bad[:5]], want[0][bad[:5]])
    if got[1].tobytes() != want[1].tobytes():
        k = np.flatnonzero((got[1]["d2"].view(np.uint32) != want[1]["d2"].view(np.uint32)) | (got[1]["idx"] != want[1]["idx"]))
        atom = np.searchsorted(want[0], k[:5], side="right") - 1
        raise AssertionError(("entries", k.size, k[:5], atom, got[1][k[:5]], want[1][k[:5]]))


def _both(ctx, name, cutoff):
    """The case against the model with upper_only off and on; returns the full lists."""
    c = _case(name)
    full = _run(ctx, c, cutoff)
    _equal(full, _model(name, cutoff))
    _equal(_run(ctx, c, cutoff, upper=True), _model(name, cutoff, True))
    return full


# ---- 1: a protein ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _1jcd():
    import structio as sio
    atoms = [a for a in sio.read_structure(sio.data_path("1jcd.pdb")) if not a.hetero]
    x, y, z, r, _ = sio.soa_vdw(atoms)
    return hc.Case("1jcd", *(np.ascontiguousarray(a, F) for a in (x, y, z, r)), np.array([0, len(x)], np.uint32))


@pytest.mark.parametrize("cutoff", [4.5, 8.0, 13.0, 15.0, 200.0])
def test_1jcd(ctx, cutoff):
    c = _1jcd()
    want = wm.lists(c.x, c.y, c.z, None, cutoff)
    got = _run(ctx, c, cutoff)
    _equal(got, want)
    _equal(_run(ctx, c, cutoff, upper=True), wm.lists(c.x, c.y, c.z, None, cutoff, True))
    if cutoff == 200.0:
        assert np.all(wm.lengths(got[0]) == c.n_atoms - 1)            # the cutoff covers the structure: long lists


# ---- 2: hand lists, exact ties, the reach ------------------------------------------------------------------------------------

def test_hand_lists(ctx):
    c = hc.hand()
    off, ent = _both(ctx, "hand", c.info["cutoff"])
    assert off.tolist() == [0, 4, 4, 4, 4, 8, 8]
    assert ent[:4].tolist() == [(0.0, 4), (4.0, 2), (9.0, 1), (9.0, 3)] and ent[4:].tolist() == [(0.0, 0), (4.0, 2), (9.0, 1), (9.0, 3)]


def test_exact_ties_are_listed_and_one_ulp_further_is_not(ctx):
    t, m = hc.ties(), hc.ties(True)
    off, ent = _run(ctx, t, 13.0)
    assert off.tolist() == [0, 3, 3, 3, 3] and ent.tolist() == [(169.0, 1), (169.0, 2), (169.0, 3)]
    assert _run(ctx, m, 13.0)[0][-1] == 0
    for c in (t, m):
        for upper in (False, True):
            _equal(_run(ctx, c, 13.0, upper, flags=None), wm.lists(c.x, c.y, c.z, None, 13.0, upper))


def test_tie_partners_in_the_last_swept_shell(ctx):
    c = hc.edge()
    off, ent = _both(ctx, "edge", hc.EDGE_CUTOFF)
    for centre in (c.info["hi"], c.info["lo"]):
        li = ent[int(off[centre]):int(off[centre + 1])]
        assert li["d2"].tolist() == [25.0] * 6 and li["idx"].tolist() == sorted(a for a, _, _ in c.info["tie"][centre])
    above = float(np.nextafter(F(hc.EDGE_CUTOFF), F(np.inf)))
    for cutoff in (above, 4.9, 7.0):
        _both(ctx, "edge", cutoff)


@pytest.mark.parametrize("k", range(8))
def test_cluster_at_every_reach(ctx, k):
    """0, half a cell .. three cells, 13 A, the whole cluster (lists of 1 999: the long lists' route), FLT_MAX (c2 = +inf)."""
    cutoff = hc.cluster_cutoffs()[k]
    got = _both(ctx, "cluster", cutoff)
    if k == 0:
        assert got[0][-1] == 0
    if k >= 6:
        assert np.all(wm.lengths(got[0]) == hc.N_CLUSTER - 1) and hc.N_CLUSTER - 1 > wc.K_WN_STAGE


def test_crowded_cell_and_wide_shells(ctx):
    for cutoff in (13.0, 3.0):
        _both(ctx, "crowd", cutoff)


def test_the_whole_grid_when_the_margins_fail(ctx):
    c = hc.cluster()
    for cutoff in (13.0, 3.28):
        got = _both(ctx, "odd_radius", cutoff)
        _equal(got, _model("cluster", cutoff))                          # the radius changes the grid, not the lists
        _equal(_run(ctx, c, cutoff, probe=-0.25), got)                  # a negative probe fails the margins too
        _equal(_run(ctx, c, cutoff, probe=3.0), got)
        _equal(_run(ctx, c, cutoff, r=c.r * F(2.0)), got)


def test_a_nan_coordinate_is_in_nobodys_list(ctx):
    c = hc.nan_atom()
    a = c.info["atom"]
    for cutoff in (13.0, hc.COVER):
        off, ent = _both(ctx, "nan_atom", cutoff)
        assert off[a] == off[a + 1] and not (ent["idx"] == a).any() and not np.isnan(ent["d2"]).any()
    assert np.all(np.delete(wm.lengths(off), a) == c.n_atoms - 2)


# ---- 3: the staging, the sort and the long lists -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["stage_edges", "tile_edges", "double_edges", "pow2_edges"])
def test_lists_at_the_edges_of_the_fill(ctx, name):
    c = _case(name)
    got = _both(ctx, name, wc.BALL_CUTOFF)
    sizes = np.repeat(np.array(c.info["sizes"]), c.info["sizes"])
    centre = np.ones(c.n_atoms, bool) if c.flags is None else (c.flags & 2) != 0
    assert np.array_equal(wm.lengths(got[0]), np.where(centre, sizes - 1, 0))


def test_coincident_atoms_are_ordered_by_idx(ctx):
    c = wc.coincident()
    off, ent = _both(ctx, "coincident", c.info["cutoff"])
    assert (ent["d2"] == 0.0).sum() == sum(n * (n - 1) for n in c.info["n"])
    _both(ctx, "coincident", 0.0)                                        # cutoff 0 lists exactly the coincident atoms


def test_equal_d2_is_ordered_by_idx(ctx):
    c = wc.equal_d2()
    off, ent = _both(ctx, "equal_d2", c.info["cutoff"])
    li = ent[int(off[c.info["centre"]]):int(off[c.info["centre"] + 1])]
    assert np.unique(li["d2"]).tolist() == [12.0, 16.5, 21.875] and len(li) == 80


# ---- 4: flags ---------------------------------------------------------------------------------------------------------------------

def test_flags(ctx):
    c = hc.cluster()
    n = c.n_atoms
    rng = np.random.default_rng(21)
    half = rng.permutation(n) < n // 2
    base = _run(ctx, c, 8.0, flags=None)
    _equal(base, _model("cluster", 8.0))
    _equal(_run(ctx, c, 8.0, flags=np.full(n, 3, np.uint8)), base)
    _equal(_run(ctx, c, 8.0, flags=np.full(n, 0xFB, np.uint8)), base)               # the other bits are ignored
    for name, flags in (("centres only", np.full(n, 2, np.uint8)), ("partners only", np.full(n, 1, np.uint8)),
                        ("neither", np.zeros(n, np.uint8)), ("disjoint", np.where(half, 1, 2).astype(np.uint8)),
                        ("mixed", rng.integers(0, 4, n).astype(np.uint8)),
                        ("one in eight", np.where(np.arange(n) % 8 == 0, 3, 0).astype(np.uint8))):
        for upper in (False, True):
            got = _run(ctx, c, 8.0, upper, flags=flags)
            _equal(got, wm.lists(c.x, c.y, c.z, flags, 8.0, upper))
            assert not wm.lengths(got[0])[(flags & 2) == 0].any(), name                  # non-centres have empty lists
            assert np.all((flags[got[1]["idx"]] & 1) != 0), name                         # only partners are listed
            if name in ("centres only", "partners only", "neither"):
                assert got[0][-1] == 0


# ---- 5: batches -------------------------------------------------------------------------------------------------------------------

def _parts_equal_the_batch(ctx, c, cutoff, got):
    for s in range(len(c.so) - 1):
        b, e = int(c.so[s]), int(c.so[s + 1])
        off, ent = _run(ctx, hc.part(c, s), cutoff)
        assert np.array_equal(off + got[0][b], got[0][b:e + 1]), s
        assert ent.tobytes() == got[1][int(got[0][b]):int(got[0][e])].tobytes(), s


def test_structures_in_the_same_space_never_list_each_other(ctx):
    for name in ("interleaved", "overlap"):
        got = _both(ctx, name, 8.0)
        _parts_equal_the_batch(ctx, _case(name), 8.0, got)
    assert (got[1]["d2"] > 0).all()                                      # overlap: the twin at d2 = 0 is another structure's


def test_empty_and_one_atom_structures(ctx):
    c = hc.tiny_batch()
    got = _both(ctx, "tiny_batch", 8.0)
    _parts_equal_the_batch(ctx, c, 8.0, got)
    e = np.zeros(0, F)
    for so in ([0], [0, 0, 0]):
        off, ent = ctx.atoms_within_batch(e, e, e, e, None, np.array(so, np.uint32))
        assert off.tolist() == [0] and len(ent) == 0
    off, ent = ctx.atoms_within(e, e, e, e)
    assert off.tolist() == [0] and len(ent) == 0
    off, ent = ctx.atoms_within(np.ones(1, F), np.ones(1, F), np.ones(1, F), np.ones(1, F))
    assert off.tolist() == [0, 0] and len(ent) == 0


def test_batch_with_a_structure_of_65536_atoms(ctx):
    c = hc.tail_batch()
    got = _both(ctx, "tail_batch", 13.0)
    b = int(c.so[-2])
    k = wm.lengths(got[0])[b:]
    assert k[c.info["centres"]].min() >= 1 and k.sum() == k[c.info["centres"]].sum()
    off, ent = _run(ctx, hc.part(c, len(c.so) - 2), 13.0)
    assert np.array_equal(off + got[0][b], got[0][b:]) and ent.tobytes() == got[1][int(got[0][b]):].tobytes()


# ---- 6: the cutoff's ends ---------------------------------------------------------------------------------------------------------

def test_cutoff_zero_and_a_cutoff_whose_square_overflows(ctx):
    for name in ("crowd", "tiny_batch", "equal_d2"):
        assert not _both(ctx, name, 0.0)[1]["d2"].any()                 # only coincident atoms, if there are any
        got = _both(ctx, name, FLT_MAX)
        c = _case(name)
        sizes = np.diff(c.so.astype(np.int64))
        assert np.array_equal(wm.lengths(got[0]), np.repeat(sizes, sizes) - 1)
    _both(ctx, "crowd", -0.0)


# ---- 7: the C interface -------------------------------------------------------------------------------------------------------------

def test_sizing_protocol(ctx):
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    lib = _capi.load()
    c = hc.crowd()
    n = c.n_atoms
    want = _model("crowd", 6.0)
    total = int(want[0][-1])
    cols = (ptr(c.x), ptr(c.y), ptr(c.z), ptr(c.r), None)
    so = np.array([0, n], np.uint32)
    calls = (lambda o, e, cap: lib.rsasa_atoms_within(ctx._h, *cols, n, c.probe, None, 6.0, 0, ptr(o), e, cap),
             lambda o, e, cap: lib.rsasa_atoms_within_batch(ctx._h, *cols, ptr(so), 1, c.probe, None, 6.0, 0, ptr(o), e, cap))
    for call in calls:
        for cap, buf in ((0, None), (0, total), (total - 1, total), (total, None)):
            off = np.full(n + 1, 0xAAAAAAAAAAAAAAAA, np.uint64)
            ent = None if buf is None else np.full(buf, 0xAA, np.uint8).repeat(8).view(wm.WITHIN_DTYPE)
            assert call(off, ptr(ent), cap) == _capi.RSASA_ERR_BUFFER_TOO_SMALL, (cap, buf)
            assert "out_entries" in lib.rsasa_context_last_error(ctx._h).decode()
            assert np.array_equal(off, want[0])                            # the offsets are written
            assert ent is None or np.all(ent.view(np.uint8) == 0xAA)       # and nothing else
        for cap in (total, total + 7):
            off = np.zeros(n + 1, np.uint64)
            ent = np.full(cap, 0xAA, np.uint8).repeat(8).view(wm.WITHIN_DTYPE)
            assert call(off, ptr(ent), cap) == _capi.RSASA_OK
            _equal((off, ent[:total]), want)
            assert np.all(ent[total:].view(np.uint8) == 0xAA)
    # every list empty: a NULL buffer is still too small (as in rsasa_precompute_neighbors), one of no entries is not
    off = np.ones(n + 1, np.uint64)
    assert lib.rsasa_atoms_within(ctx._h, *cols, n, c.probe, None, 0.0, 0, ptr(off), None, 0) == _capi.RSASA_ERR_BUFFER_TOO_SMALL
    assert not off.any()
    off = np.ones(n + 1, np.uint64)
    ent = np.zeros(1, wm.WITHIN_DTYPE)
    assert lib.rsasa_atoms_within(ctx._h, *cols, n, c.probe, None, 0.0, 0, ptr(off), ptr(ent), 0) == _capi.RSASA_OK and not off.any()
    # no atoms: out_offsets[0] = 0
    off = np.ones(1, np.uint64)
    assert lib.rsasa_atoms_within(ctx._h, None, None, None, None, None, 0, 1.4, None, 8.0, 0, ptr(off), None, 0) == _capi.RSASA_OK
    assert off[0] == 0


def test_argument_errors_leave_the_context_usable(ctx):
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    lib = _capi.load()
    c = hc.edge()
    n = c.n_atoms
    want = _model("edge", hc.EDGE_CUTOFF)
    off = np.zeros(n + 1, np.uint64)
    ent = np.zeros(int(want[0][-1]), wm.WITHIN_DTYPE)
    cols = (ptr(c.x), ptr(c.y), ptr(c.z), ptr(c.r), None)
    so = np.array([0, n], np.uint32)
    falling = np.array([0, 40, 30, n], np.uint32)
    bad = _capi.RSASA_ERR_INVALID_ARGUMENT
    one, many = lib.rsasa_atoms_within, lib.rsasa_atoms_within_batch
    out = (ptr(off), ptr(ent), len(ent))
    cut = "cutoff must be finite and not negative"
    errors = [
        (lambda: one(ctx._h, *cols, n, c.probe, None, float("nan"), 0, *out), cut),
        (lambda: one(ctx._h, *cols, n, c.probe, None, float("inf"), 0, *out), cut),
        (lambda: one(ctx._h, *cols, n, c.probe, None, -1.0, 1, *out), cut),
        (lambda: many(ctx._h, *cols, ptr(so), 1, c.probe, None, -1e-30, 0, *out), cut),
        (lambda: many(ctx._h, *cols, ptr(so), 1, c.probe, None, float("nan"), 0, *out), cut),
        (lambda: one(ctx._h, *cols, n, c.probe, None, hc.EDGE_CUTOFF, 0, None, ptr(ent), len(ent)), "NULL argument"),
        (lambda: one(ctx._h, None, ptr(c.y), ptr(c.z), ptr(c.r), None, n, c.probe, None, hc.EDGE_CUTOFF, 0, *out), "NULL argument"),
        (lambda: many(ctx._h, *cols, None, 1, c.probe, None, hc.EDGE_CUTOFF, 0, *out), "NULL argument"),
        (lambda: many(ctx._h, *cols, ptr(falling), 3, c.probe, None, hc.EDGE_CUTOFF, 0, *out), "structure_offsets must be non-decreasing"),
        (lambda: one(ctx._h, *cols, n, -5.0, None, hc.EDGE_CUTOFF, 0, *out), None),                 # probe + max_r <= 0
    ]
    for k, (call, message) in enumerate(errors):
        assert call() == bad, k
        if message:
            assert message in lib.rsasa_context_last_error(ctx._h).decode(), (k, lib.rsasa_context_last_error(ctx._h))
        assert not off.any() and not ent.view(np.uint8).any(), k         # nothing was written
        _equal(_run(ctx, c, hc.EDGE_CUTOFF), want)                       # and the next call is right
    assert one(ctx._h, *cols, n, c.probe, None, hc.EDGE_CUTOFF, 0, *out) == _capi.RSASA_OK
    _equal((off, ent), want)


def test_an_infinite_coordinate_is_refused_and_the_next_call_is_right(ctx):
    import rustsasa_amd
    c = hc.edge()
    x = c.x.copy()
    x[5] = np.inf
    for call in (lambda: ctx.atoms_within(x, c.y, c.z, c.r, None, c.probe, None, hc.EDGE_CUTOFF),
                 lambda: ctx.atoms_within_batch(x, c.y, c.z, c.r, None, c.so, c.probe, None, hc.EDGE_CUTOFF)):
        with pytest.raises(rustsasa_amd.RsasaError) as e:
            call()
        assert e.value.status == -5
        _equal(_run(ctx, c, hc.EDGE_CUTOFF), _model("edge", hc.EDGE_CUTOFF))


def test_a_first_guess_that_is_too_small_is_repeated(ctx):
    """Lists far longer than 0.25 C^3 + 16 (the wrapper's guess): the wrapper's second call at the size the offsets give."""
    c = wc.coincident()
    _equal(_run(ctx, c, 1.0), _model("coincident", 1.0))


# ---- 8: one context -----------------------------------------------------------------------------------------------------------------

def test_list_lengths_are_the_half_sphere_counts(ctx):
    rng = np.random.default_rng(31)
    for c, cutoff in ((hc.crowd(), 13.0), (hc.tiny_batch(), 6.0), (hc.edge(), hc.EDGE_CUTOFF)):
        for flags in (None, rng.integers(0, 4, c.n_atoms).astype(np.uint8)):
            off, _ = _run(ctx, c, cutoff, flags=flags)
            if len(c.so) == 2:
                up, down = ctx.half_sphere_exposure(c.x, c.y, c.z, c.r, None, c.probe, c.dirs, flags, cutoff)
            else:
                up, down = ctx.half_sphere_exposure_batch(c.x, c.y, c.z, c.r, None, c.so, c.probe, c.dirs, flags, cutoff)
            assert np.array_equal(wm.lengths(off), up.astype(np.int64) + down)


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
            lambda: ctx.calculate_sasa_soa(*c.cols, c.probe, 100)]


def test_between_calls_of_every_other_family(ctx):
    """The long lists of the neighbour runs (a staging of 512) and of this run (1 024) share the scan and the scratch: the
    cluster of coincident atoms takes both routes in turn."""
    import rustsasa_amd
    c, t, s = hc.edge(), hc.tiny_batch(), hc.part(wc.coincident(), 0)
    want, want_t, want_s = _model("edge", hc.EDGE_CUTOFF), _model("tiny_batch", 8.0), wm.lists(s.x, s.y, s.z, None, 2.0)
    tup = lambda v: (v,) if isinstance(v, np.ndarray) else tuple(v)  # noqa: E731
    with rustsasa_amd.Context(0) as fresh:
        alone = [call() for call in _family_calls(fresh, c)]
        alone_s = tup(fresh.precompute_neighbors(*s.cols, s.probe))
    for call, ref in zip(_family_calls(ctx, c), alone):
        before = call()
        _equal(_run(ctx, c, hc.EDGE_CUTOFF), want)
        _equal(_run(ctx, t, 8.0), want_t)
        after = call()
        assert len(tup(before)) == len(tup(after)) == len(tup(ref))
        for a, b_, r in zip(tup(before), tup(after), tup(ref)):
            assert a.tobytes() == b_.tobytes() == r.tobytes()
    for _ in range(2):
        _equal(_run(ctx, s, 2.0), want_s)
        for a, r in zip(tup(ctx.precompute_neighbors(*s.cols, s.probe)), alone_s):
            assert a.tobytes() == r.tobytes()


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
    got = _run(ctx, hc.crowd(), 13.0)
    ctx.wait()
    assert out.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    _equal(got, _model("crowd", 13.0))
