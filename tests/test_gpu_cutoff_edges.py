"""The second pass over the three cutoff sweeps on the GPU - k_half_sphere (hse.hip), k_within_* (within.hip), k_nearest
(nearest.hip) - on the cases of cutoff_edge_cases.py, pinned by test_cutoff_edges_cpu.py: thin, long, slanted and
crowded grids; structures one coordinate ulp on either side of the margins' limit, with exact ties in the last swept
shell; a staging compacted three times with a bound in force; the shared scratch reused across k, flags and dirs; eight
threads on one context.  Everything is compared with the exact models (hse_model.py, within_model.py, nearest_model.py)
byte for byte: offsets equal, entries equal as bytes, up / down equal.  No tolerances anywhere."""
import functools
import threading

import numpy as np
import pytest

import cutoff_edge_cases as ce
import hse_cases as hc
import hse_model as hm
import nearest_cases as nc
import nearest_model as nm
import within_model as wm

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


# ---- cases by key, flags by key, models computed once -------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _1jcd():
    import structio as sio
    atoms = [a for a in sio.read_structure(sio.data_path("1jcd.pdb")) if not a.hetero]
    x, y, z, r, _ = sio.soa_vdw(atoms)
    return hc.Case("1jcd", *(np.ascontiguousarray(a, F) for a in (x, y, z, r)), np.array([0, len(x)], np.uint32),
                   hc.random_dirs(len(x), 950))


def _case(key):
    """("swept", name) | ("edge_at", axis, sign, which) | ("edge_twelve",) | ("knn_twelve", k) | ("dense", odd) | ("thrice",) |
    (name,) of hse_cases.py | ("1jcd",)."""
    kind = key[0]
    if kind == "swept":
        return ce.swept(key[1])
    if kind == "edge_at":
        return ce.edge_at_margin(*key[1:])
    if kind == "edge_twelve":
        return ce.edge_twelve()
    if kind == "knn_twelve":
        return ce.knn_edge_twelve(key[1])
    if kind == "dense":
        return ce.knn_dense(key[1])
    if kind == "thrice":
        return ce.knn_dense_thrice()
    return _1jcd() if kind == "1jcd" else getattr(hc, kind)()


def _flags(c, fk):
    """fk: "own", None, "eighth" (one centre in eight, every atom a partner), "zeros", "mixed"."""
    if fk == "own":
        return c.flags
    if fk == "eighth":
        return ce.one_in_eight(c.n_atoms)
    if fk == "zeros":
        return np.zeros(c.n_atoms, np.uint8)
    if fk == "mixed":
        return np.random.default_rng(960).integers(0, 4, c.n_atoms).astype(np.uint8)
    assert fk is None
    return None


@functools.lru_cache(maxsize=None)
def _m_hse(key, cutoff, dirs=True, fk="own"):
    c = _case(key)
    return hm.counts_batch(c.x, c.y, c.z, c.so, c.dirs if dirs else None, _flags(c, fk), cutoff)


@functools.lru_cache(maxsize=None)
def _m_within(key, cutoff, upper=False, fk="own"):
    c = _case(key)
    return wm.lists_batch(c.x, c.y, c.z, c.so, _flags(c, fk), cutoff, upper)


@functools.lru_cache(maxsize=None)
def _m_nearest256(key, cutoff, fk="own"):
    c = _case(key)
    return nm.lists_batch(c.x, c.y, c.z, c.so, _flags(c, fk), nm.MAX_K, cutoff, by_sort=True)


def _m_nearest(key, k, cutoff=None, fk="own"):
    return nm.truncate(*_m_nearest256(key, cutoff, fk), k)


# ---- the calls --------------------------------------------------------------------------------------------------------------------

def _single(c):
    return len(c.so) == 2


def _hse(ctx, c, cutoff, dirs=True, fk="own"):
    d, fl = (c.dirs if dirs else None), _flags(c, fk)
    if _single(c):
        return ctx.half_sphere_exposure(*c.cols, c.probe, d, fl, cutoff)
    return ctx.half_sphere_exposure_batch(*c.cols, c.so, c.probe, d, fl, cutoff)


def _within(ctx, c, cutoff, upper=False, fk="own"):
    if _single(c):
        return ctx.atoms_within(*c.cols, c.probe, _flags(c, fk), cutoff, upper)
    return ctx.atoms_within_batch(*c.cols, c.so, c.probe, _flags(c, fk), cutoff, upper)


def _nearest(ctx, c, k, cutoff=None, fk="own"):
    if _single(c):
        return ctx.nearest_atoms(*c.cols, c.probe, k, _flags(c, fk), cutoff)
    return ctx.nearest_atoms_batch(*c.cols, c.so, c.probe, k, _flags(c, fk), cutoff)


def _counts_equal(got, want, what=None):
    for name, g, w in zip(("up", "down"), got, want):
        assert g.dtype == np.uint32 and g.shape == w.shape, (what, name)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, name, bad.size, bad[:5], g[bad[:5]], w[bad[:5]])


def _lists_equal(got, want, what=None):
    assert got[0].dtype == np.uint64 and got[1].dtype == wm.WITHIN_DTYPE and got[0].shape == want[0].shape, what
    bad = np.flatnonzero(got[0] != want[0])
    assert bad.size == 0, (what, "offsets", bad.size, bad[:5], got[0][bad[:5]], want[0][bad[:5]])
    if got[1].tobytes() != want[1].tobytes():
        k = np.flatnonzero((got[1]["d2"].view(np.uint32) != want[1]["d2"].view(np.uint32)) | (got[1]["idx"] != want[1]["idx"]))
        atom = np.searchsorted(want[0], k[:5], side="right") - 1
        raise AssertionError((what, "entries", k.size, k[:5], atom, got[1][k[:5]], want[1][k[:5]]))


def _list(got, i):
    return got[1][int(got[0][i]):int(got[0][i + 1])]


def _slice_of_lists(got, b, e):
    return got[0][b:e + 1] - got[0][b], got[1][int(got[0][b]):int(got[0][e])]


def _alone(c):
    """(s, the structure, its atom range): the structure in the middle of a batch, run alone."""
    s = (len(c.so) - 1) // 2
    return s, hc.part(c, s), int(c.so[s]), int(c.so[s + 1])


# ---- the three families on a case ----------------------------------------------------------------------------------------------------

def _hse_family(ctx, key, cutoffs):
    c = _case(key)
    s, p, b, e = _alone(c)
    for cutoff in cutoffs:
        got = _hse(ctx, c, cutoff)
        _counts_equal(got, _m_hse(key, cutoff), (key, cutoff))
        if not _single(c):
            _counts_equal(_hse(ctx, p, cutoff), (got[0][b:e], got[1][b:e]), (key, cutoff, "alone", s))
    got = _hse(ctx, c, cutoffs[0], dirs=False)
    _counts_equal(got, _m_hse(key, cutoffs[0], False), (key, "no dirs"))
    assert not got[1].any()


def _within_family(ctx, key, cutoffs):
    c = _case(key)
    s, p, b, e = _alone(c)
    for cutoff in cutoffs:
        for upper in (False, True):
            got = _within(ctx, c, cutoff, upper)
            _lists_equal(got, _m_within(key, cutoff, upper), (key, cutoff, upper))
            if not _single(c):
                _lists_equal(_within(ctx, p, cutoff, upper), _slice_of_lists(got, b, e), (key, cutoff, upper, "alone", s))


def _nearest_family(ctx, key, cutoffs, ks=ce.NEAREST_KS):
    c = _case(key)
    s, p, b, e = _alone(c)
    for cutoff in cutoffs:
        for k in ks:
            got = _nearest(ctx, c, k, cutoff)
            _lists_equal(got, _m_nearest(key, k, cutoff), (key, k, cutoff))
            if not _single(c):
                _lists_equal(_nearest(ctx, p, k, cutoff), _slice_of_lists(got, b, e), (key, k, cutoff, "alone", s))


# ---- A, B: awkward grids and the margin structures ---------------------------------------------------------------------------------------

SWEPT = ce.GRID_NAMES + ce.MARGIN_NAMES


@pytest.mark.parametrize("name", SWEPT)
def test_half_sphere_exposure_on_the_sweep_cases(ctx, name):
    _hse_family(ctx, ("swept", name), ce.hse_cutoffs(ce.swept(name), name))


@pytest.mark.parametrize("name", SWEPT)
def test_atoms_within_on_the_sweep_cases(ctx, name):
    c = ce.swept(name)
    cutoffs = ce.within_cutoffs(c, name)
    assert len(cutoffs) == 3                                            # every structure is under 1 000 atoms: a covering one
    _within_family(ctx, ("swept", name), cutoffs)
    sizes = np.diff(c.so.astype(np.int64))
    got = _within(ctx, c, cutoffs[2])
    assert np.array_equal(wm.lengths(got[0]), np.repeat(sizes, sizes) - 1)


@pytest.mark.parametrize("name", SWEPT)
def test_nearest_atoms_on_the_sweep_cases(ctx, name):
    c = ce.swept(name)
    _nearest_family(ctx, ("swept", name), ce.nearest_cutoffs(c, name))
    sizes = np.diff(c.so.astype(np.int64))
    got = _nearest(ctx, c, 256)
    assert np.array_equal(wm.lengths(got[0]), np.minimum(np.repeat(sizes, sizes) - 1, 256))


def test_the_odd_structures_have_the_lists_of_the_even_one(ctx):
    c = ce.swept("odd_beside_even")
    n = int(c.so[1])
    same = hc.Case(c.name, c.x, c.y, c.z, c.r, c.so, np.tile(c.dirs[:n], (3, 1)), None, c.probe)
    up, down = _hse(ctx, same, 13.0)
    assert up[:n].tobytes() == up[n:2 * n].tobytes() == up[2 * n:].tobytes() and up.any() and down.any()
    assert down[:n].tobytes() == down[n:2 * n].tobytes() == down[2 * n:].tobytes()
    for got in (_within(ctx, c, 8.0), _nearest(ctx, c, 256), _nearest(ctx, c, 16, 13.0)):
        a, b_, d = (_slice_of_lists(got, s * n, (s + 1) * n) for s in range(3))
        assert np.array_equal(a[0], b_[0]) and np.array_equal(a[0], d[0]) and a[1].tobytes() == b_[1].tobytes() == d[1].tobytes()


# ---- B: exact ties in the last swept shell, at the margins' edge ------------------------------------------------------------------------------

def _edge_checks(c, within, hse_none, nearest, base=0):
    """On one translated edge() structure whose atoms start at `base` of the outputs."""
    info = c.info
    for cen in (info["hi"], info["lo"]):
        li = _list(within, base + cen)
        ties = {a for a, _, _ in info["tie"][cen]}
        far = {a for a, _, _ in info["far"][cen]}
        assert ties <= set(li["idx"].tolist()) and not far & set(li["idx"].tolist())
        assert set(li["idx"][li["d2"] == F(25.0)].tolist()) == ties      # all six, at d2 == c2 exactly
        assert hse_none[0][base + cen] == len(li) and hse_none[1][base + cen] == 0
        assert _list(nearest, base + cen).tobytes() == li.tobytes()


@pytest.mark.parametrize("axis,sign", ce.DIRECTIONS)
def test_edge_at_margin(ctx, axis, sign):
    cut = hc.EDGE_CUTOFF
    for which in ce.WHICH:
        key = ("edge_at", axis, sign, which)
        c = _case(key)
        within = _within(ctx, c, cut)
        _lists_equal(within, _m_within(key, cut), key)
        _lists_equal(_within(ctx, c, cut, True), _m_within(key, cut, True), key)
        none = _hse(ctx, c, cut, dirs=False)
        _counts_equal(none, _m_hse(key, cut, False), key)
        _counts_equal(_hse(ctx, c, cut), _m_hse(key, cut), key)
        nearest = _nearest(ctx, c, 256, cut)
        _lists_equal(nearest, within, key)                               # no list reaches 256: the within-list itself
        _edge_checks(c, within, none, nearest)
        for k in (1, 16):
            _lists_equal(_nearest(ctx, c, k), _m_nearest(key, k), (key, k))
            _lists_equal(_nearest(ctx, c, k, cut), _m_nearest(key, k, cut), (key, k, cut))


def test_edge_under_and_over_interleaved_in_one_batch(ctx):
    key, cut = ("edge_twelve",), hc.EDGE_CUTOFF
    c = _case(key)
    within, none, nearest = _within(ctx, c, cut), _hse(ctx, c, cut, dirs=False), _nearest(ctx, c, 256, cut)
    _lists_equal(within, _m_within(key, cut))
    _counts_equal(none, _m_hse(key, cut, False))
    _counts_equal(_hse(ctx, c, cut), _m_hse(key, cut))
    _lists_equal(nearest, within)
    _lists_equal(_nearest(ctx, c, 16), _m_nearest(key, 16))
    for s, p in enumerate(c.info["members"]):                            # under, over, under, over, ...
        b, e = int(c.so[s]), int(c.so[s + 1])
        _edge_checks(p, within, none, nearest, b)
        _lists_equal(_within(ctx, p, cut), _slice_of_lists(within, b, e), s)
        _counts_equal(_hse(ctx, p, cut, dirs=False), (none[0][b:e], none[1][b:e]), s)
        _lists_equal(_nearest(ctx, p, 256, cut), _slice_of_lists(nearest, b, e), s)


@pytest.mark.parametrize("k", nc.EDGE_KS)
def test_knn_edge_at_margin(ctx, k):
    key = ("knn_twelve", k)
    c = _case(key)
    got = _nearest(ctx, c, k)
    _lists_equal(got, _m_nearest(key, k), key)
    for s, p in enumerate(c.info["members"]):
        b, e = int(c.so[s]), int(c.so[s + 1])
        for gr in p.info["groups"]:                                      # all six directions, under and over
            li = _list(got, b + gr["centre"])
            assert len(li) == k and li["idx"][-1] == gr["true_kth"] and gr["diagonal"] not in li["idx"], (s, gr)
        _lists_equal(_nearest(ctx, p, k), _slice_of_lists(got, b, e), s)
    _lists_equal(_nearest(ctx, c, k, 13.0), _m_nearest(key, k, 13.0), key)
    _lists_equal(_within(ctx, c, 8.0), _m_within(key, 8.0), key)
    _counts_equal(_hse(ctx, c, 13.0, dirs=False), _m_hse(key, 13.0, False), key)


# ---- C: k_nearest past its first compaction ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("k", ce.DENSE_KS)
def test_knn_dense(ctx, k, odd):
    key = ("dense", odd)
    c = _case(key)
    got = _nearest(ctx, c, k)
    _lists_equal(got, _m_nearest(key, k), (key, k))
    assert np.array_equal(wm.lengths(got[0]), np.where((c.flags & 2) != 0, k, 0))
    n_near = int(np.isin(_list(got, c.info["last"])["idx"], c.info["near"]).sum())
    assert n_near == (0 if k == 1 else ce.DENSE_NEAR)                    # the keys from shell 1, below the bound


@pytest.mark.parametrize("cutoff", [1.0, 3.0])
def test_knn_dense_under_a_cutoff_below_and_above_the_bound(ctx, cutoff):
    key = ("dense", False)
    c = _case(key)
    within = _within(ctx, c, cutoff)
    _lists_equal(within, _m_within(key, cutoff), (key, cutoff))
    for k in ce.DENSE_KS:
        got = _nearest(ctx, c, k, cutoff)
        _lists_equal(got, _m_nearest(key, k, cutoff), (key, k, cutoff))
        _lists_equal(got, nm.truncate(*within, k), (key, k, cutoff, "within cut at k"))
    short = len(_list(got, c.info["last"])) < 256
    assert short == (cutoff == 1.0)


def test_knn_dense_three_times_in_one_batch(ctx):
    key = ("thrice",)
    c = _case(key)
    k = 16
    got = _nearest(ctx, c, k)
    _lists_equal(got, nm.truncate(*_m_nearest256(key, None), k))
    assert np.array_equal(wm.lengths(got[0]), np.where((c.flags & 2) != 0, k, 0))
    for s in range(3):
        b, e = int(c.so[s]), int(c.so[s + 1])
        _lists_equal(_nearest(ctx, hc.part(c, s), k), _slice_of_lists(got, b, e), s)


# ---- D: call order inside the families -------------------------------------------------------------------------------------------------------

def _sequence(ctx, key):
    """Every call's result against the model; between the calls k, flags and dirs change under the shared scratch."""
    c = _case(key)
    big = hc.cluster()
    act = np.arange(0, big.n_atoms, 3, dtype=np.uint32)
    # nearest_atoms: the rows keep the largest size, the stride changes under them
    for k in (256, 1, 255, 256):
        _lists_equal(_nearest(ctx, c, k, None, None), _m_nearest(key, k, None, None), (key, "k", k))
    # the rank pointer: non-null, null over a stale map, non-null; in between a neighbour run's idx_map in the same buffer
    nb = None
    for step, fk in enumerate(("eighth", None, "eighth")):
        _lists_equal(_nearest(ctx, c, 16, None, fk), _m_nearest(key, 16, None, fk), (key, "flags", step))
        got = ctx.precompute_neighbors(*big.cols, big.probe, active_indices=act)
        assert nb is None or all(a.tobytes() == b_.tobytes() for a, b_ in zip(nb, got))
        nb = got
        _lists_equal(_nearest(ctx, c, 256, 13.0, fk), _m_nearest(key, 256, 13.0, fk), (key, "flags", step, 13.0))
    # atoms_within: flags, none, all zero (every list empty: no fill), flags; upper_only on and off
    for step, (fk, upper) in enumerate((("eighth", False), (None, True), ("zeros", False), ("eighth", True), (None, False),
                                        ("zeros", True), ("eighth", False))):
        got = _within(ctx, c, 8.0, upper, fk)
        _lists_equal(got, _m_within(key, 8.0, upper, fk), (key, "within", step))
        assert fk != "zeros" or got[0][-1] == 0
    # half_sphere_exposure: dirs, none (down all zero), dirs; flags likewise
    for step, (dirs, fk) in enumerate(((True, None), (False, None), (True, None), (True, "eighth"), (False, "eighth"),
                                       (True, None), (True, "mixed"), (True, "eighth"))):
        got = _hse(ctx, c, 13.0, dirs, fk)
        _counts_equal(got, _m_hse(key, 13.0, dirs, fk), (key, "hse", step))
        assert dirs or not got[1].any()


@pytest.mark.parametrize("order", [("cluster", "tiny_batch"), ("tiny_batch", "cluster")])
def test_call_order_inside_the_families(order):
    """One fresh context per order: the large input first (the buffers are sized once and reused oversized), then the
    small one first (they grow)."""
    import rustsasa_amd
    with rustsasa_amd.Context(0) as fresh:
        for name in order + order[:1]:
            _sequence(fresh, (name,))


# ---- E: threads -----------------------------------------------------------------------------------------------------------------------------------

JOIN_SECONDS = 120.0


def _thread_calls(c):
    """[(name, call(ctx) -> tuple of arrays)] of one round on one input."""
    return [("hse", lambda ctx: _hse(ctx, c, 13.0)), ("within", lambda ctx: _within(ctx, c, 8.0)),
            ("nearest", lambda ctx: _nearest(ctx, c, 30)),
            ("sasa", lambda ctx: (ctx.calculate_sasa_soa(*c.cols, c.probe, 100),))]


def _same(got, want):
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
                                         for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def _thread_wants():
    """{input: {call: result}} from the models, computed once before any thread starts; the SASA reference is filled in by
    one single-threaded call."""
    out = {}
    for name in ce.THREAD_INPUTS:
        key = (name,)
        out[name] = dict(hse=_m_hse(key, 13.0), within=_m_within(key, 8.0), nearest=_m_nearest(key, 30))
    return out


def _hammer(contexts, wants):
    errors = []

    def work(tid):
        try:
            ctx = contexts[tid % len(contexts)]
            for it in range(ce.THREAD_ROUNDS):
                name = ce.thread_input(tid, it)
                for call, run in _thread_calls(_case((name,))):
                    if not _same(run(ctx), wants[name][call]):
                        errors.append((tid, it, name, call, "differs"))
        except Exception as e:  # noqa: BLE001
            errors.append((tid, repr(e)))

    threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(ce.THREADS)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_SECONDS)
    hung = [n for n, t in enumerate(threads) if t.is_alive()]
    assert not hung, ("threads still running", hung)
    return errors


@pytest.mark.parametrize("shared", [False, True])
def test_threads_on_the_three_cutoff_families_and_sasa(ctx, shared):
    import rustsasa_amd
    wants = {name: dict(w) for name, w in _thread_wants().items()}
    for name in ce.THREAD_INPUTS:                                        # single-threaded: the SASA reference, and the models hold
        for call, run in _thread_calls(_case((name,))):
            got = run(ctx)
            if call == "sasa":
                wants[name][call] = got
            else:
                assert _same(got, wants[name][call]), (name, call)
    contexts = [rustsasa_amd.Context(0) for _ in range(1 if shared else ce.THREADS)]
    try:
        assert _hammer(contexts, wants) == []
    finally:
        for c in contexts:
            c.close()
