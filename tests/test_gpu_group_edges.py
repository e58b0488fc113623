"""Group contacts (rsasa_group_contacts*: k_group_order and k_group_points of points.hip, gp_run of neighbors.cpp) past
their first suite, on the inputs of group_edge_cases.py - test_group_edges_cpu.py pins each to its class - against the
exact model of groups_model.py:

  - label runs: own prefixes of 257 .. 768 entries (several LDS stages of own entries), one foreign run over whole
    stages, two runs whose seam falls inside a stage, an own prefix that ends inside the second stage in front of 214
    and 469 rows (both sides of the 256 rows counted in registers), and a single foreign entry that is the last of a
    list of several stages, alone in a padded group of four and closing a full one
  - one batch with both binning routes, lists on both sides of the neighbour staging, ids that shorten long lists, one
    and two atoms and empty structures, forwards and backwards; 3 000 structures of one to four atoms
  - the row-offset scan at two and three tiles per block
  - permuted atoms, order-preserving and order-reversing relabellings
  - one context through group calls of every size between the calls of the other families
  - off-range radii and probes, several structures per batch.

Every comparison is exact: np.array_equal or a byte comparison."""
import numpy as np
import pytest

import bench_workloads as bw
import group_edge_cases as ge
import groups_model as gm
import nb_helpers as nh
import point_edge_cases as pe
import points_model as pm
from test_gpu_groups import _assert_identities, _assert_model, _check_shapes, _run_both

pytestmark = pytest.mark.gpu

PERMUTED = (130, 16)          # n_points, W of test 5
DEGENERATE = (271, 16)        # n_points, W of test 8: 256 fused points, the remainder alone in the second pass
WALK_BIG_POINTS = (260, 64)   # the big batch of test 7, first and later: two passes of four chunks (256 fused points and
                              # a remainder alone in the second), and one chunk of the NCH = 2 kernel


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


def _sizing_call(ctx, x, y, z, r, ids, g, so, probe, n_points):
    """rsasa_group_contacts_batch with no row buffers: (return code, out_offsets)."""
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    n = len(x)
    offs = np.full(n + 1, 7, np.uint64)
    sf, fr = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    rc = _capi.load().rsasa_group_contacts_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(g), ptr(so),
                                                 len(so) - 1, probe, n_points, ptr(offs), None, None, None, 0, ptr(sf),
                                                 ptr(fr), None)
    return rc, offs


# ---- 1: cluster labellings ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cluster_models():
    def one(k):
        cols, g, _ = ge.cluster(k[0], k[1])
        return gm.group_counts(*cols, g, ge.PROBE, k[2], ge.W)
    return pe.pmap(one, [(n, kind, p) for n, kind in ge.cluster_keys() for p in ge.CLUSTER_POINTS])


@pytest.mark.parametrize("n_points", ge.CLUSTER_POINTS)
@pytest.mark.parametrize("n,kind", ge.cluster_keys())
def test_cluster_labellings(ctx, cluster_models, n, kind, n_points):
    cols, g, c0 = ge.cluster(n, kind)
    try:
        ctx.set_simd_width(ge.W)
        got = _run_both(ctx, cols, g, ge.PROBE, n_points)
    finally:
        ctx.set_simd_width(8)
    _assert_model(got, cluster_models[(n, kind, n_points)], (n, kind, n_points))
    _assert_identities(got, g)
    if kind == "one_label":
        assert got[0][c0] == got[0][-1] and np.array_equal(got[4][c0:], got[5][c0:])   # no rows, self_free == free


# ---- 2: one batch of everything -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed_models():
    cat, g, so = ge.mixed_batch()
    return {p: ge.batch_model(*cat, g, so, ge.PROBE, p, 8) for p in (100, 300)}


@pytest.mark.parametrize("reverse", [False, True], ids=["forwards", "backwards"])
@pytest.mark.parametrize("n_points", [100, 300])
def test_mixed_batch(ctx, mixed_models, n_points, reverse):
    so_f = ge.mixed_batch()[2]
    S = len(so_f) - 1
    order = list(range(S))[::-1] if reverse else list(range(S))
    want = ge.join_models([ge.slice_model(mixed_models[n_points], so_f, s) for s in order])
    cat, g, so = ge.mixed_batch(reverse)
    got = ctx.group_contacts_batch(*cat, g, so, ge.PROBE, n_points)
    _assert_model(got, want, (n_points, reverse))
    sasa, _ = ctx.calculate_sasa_batch(*cat, so, ge.PROBE, n_points)
    assert got[6].tobytes() == sasa.tobytes()
    # structure by structure through the single call
    singles, sasas = [], []
    for s in range(S):
        b, e = int(so[s]), int(so[s + 1])
        one = ctx.group_contacts(*(c[b:e] for c in cat), g[b:e], ge.PROBE, n_points)
        _check_shapes(one, e - b)
        singles.append(one[:6])
        sasas.append(one[6])
    joined = ge.join_models(singles)
    for k in range(6):
        assert np.array_equal(got[k], joined[k]), k
    assert got[6].tobytes() == np.concatenate(sasas).tobytes()
    # the structures of one and two atoms
    s1, s2 = order.index(1), order.index(2)
    a, b = int(so[s1]), int(so[s2])
    assert got[0][a] == got[0][a + 1] and got[4][a] == got[5][a] == n_points
    assert np.diff(got[0][b:b + 3].astype(np.int64)).tolist() == [1, 1]
    assert got[1][int(got[0][b]):int(got[0][b + 2])].tolist() == [1, 0] and got[4][b] == got[4][b + 1] == n_points


# ---- 3: thousands of tiny structures ------------------------------------------------------------------------------

def test_tiny_structures(ctx):
    cat, g, so = ge.tiny_batch()
    got = ctx.group_contacts_batch(*cat, g, so, ge.PROBE, 100)
    _assert_model(got, ge.batch_model(*cat, g, so, ge.PROBE, 100, 8))
    sasa, _ = ctx.calculate_sasa_batch(*cat, so, ge.PROBE, 100)
    assert got[6].tobytes() == sasa.tobytes()
    sizes = np.diff(so.astype(np.int64))
    assert (got[2] > 0).any() and int(got[0][-1]) == int(sizes[sizes > 1].sum())   # a row per atom that has company


# ---- 4: the row-offset scan -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ge.SCAN_KINDS)
@pytest.mark.parametrize("n", ge.SCAN_SIZES)
def test_scan_sizing_call_row_offsets(ctx, n, kind):
    """Chunks of 512 and 768 row counts per scan block.  The sizing call (no row buffers: order, count and scan, no
    point tests) returns RSASA_ERR_BUFFER_TOO_SMALL and the offsets: the prefix sum of the distinct foreign labels in
    the oracle's list of every atom."""
    from rustsasa_amd import _capi
    x, y, z, r, ids, so, g = ge.scan_case(n, kind)
    offs, ent = nh.oracle_batch_csr(x, y, z, r, ids, so, ge.SCAN_PROBE)
    want = ge.row_offsets(offs, ent, g, ge.structure_base(so))
    rc, got = _sizing_call(ctx, x, y, z, r, ids, g, so, ge.SCAN_PROBE, 64)
    assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL
    assert np.array_equal(got, want)


def test_scan_full_call(ctx):
    """One full call at 262 145 atoms (a batch of 102 structures, 64 points), compared with the model: on the threads of
    group_edge_cases.batch_model it takes less than the model of test_structure_of_65536_atoms, so the weaker
    comparison with accessible_points_batch was not needed.  The offsets are also those of the sizing call."""
    from rustsasa_amd import _capi
    n, kind, n_points = ge.SCAN_FULL
    x, y, z, r, ids, so, g = ge.scan_case(n, kind)
    got = ctx.group_contacts_batch(x, y, z, r, ids, g, so, ge.SCAN_PROBE, n_points)
    _assert_model(got, ge.batch_model(x, y, z, r, ids, g, so, ge.SCAN_PROBE, n_points, 8))
    rc, offs = _sizing_call(ctx, x, y, z, r, ids, g, so, ge.SCAN_PROBE, n_points)
    assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL and np.array_equal(offs, got[0])
    words, sasa = ctx.accessible_points_batch(x, y, z, r, ids, so, ge.SCAN_PROBE, n_points)
    assert np.array_equal(got[5].astype(np.int64), pe.popcount(words)) and got[6].tobytes() == sasa.tobytes()


# ---- 5: permuted atoms, relabelled groups ---------------------------------------------------------------------------

def _take_atoms(got, perm):
    """The result with the atoms in the order perm (new atom i is old atom perm[i]), every atom's rows as they are."""
    o = got[0].astype(np.int64)
    k = np.diff(o)[perm]
    offs = np.zeros(len(perm) + 1, np.uint64)
    offs[1:] = np.cumsum(k)
    first = np.repeat(o[:-1][perm], k)
    rows = first + np.arange(int(k.sum())) - np.repeat(offs[:-1].astype(np.int64), k)
    return (offs,) + tuple(a[rows] for a in got[1:4]) + tuple(a[perm] for a in got[4:7])


def _reverse_rows(got):
    """Every atom's rows in reverse order."""
    o = got[0].astype(np.int64)
    k = np.diff(o)
    rows = np.repeat(o[1:] - 1, k) - (np.arange(int(o[-1])) - np.repeat(o[:-1], k))
    return (got[0],) + tuple(a[rows] for a in got[1:4]) + got[4:7]


def _permuted_input(which):
    if which == "151L_H3":
        cols = nh.protor("151L_H3.pdb")
        return cols, ge.blocked(len(cols[0]))
    # own_then_many on 300 atoms: a block of 100, so an own prefix of 99 entries in front of 200 runs of one
    cols, c0 = nh.tight_cluster(300, seed=300)
    return cols, ge.cluster_labels("own_then_many", len(cols[0]), c0, block=100)


@pytest.fixture(scope="module")
def permuted_models():
    return pe.pmap(lambda w: gm.group_counts(*_permuted_input(w)[0], _permuted_input(w)[1], ge.PROBE, *PERMUTED),
                   ["151L_H3", "cluster_300"])


@pytest.mark.parametrize("which", ["151L_H3", "cluster_300"])
def test_permutation_and_relabelling(ctx, permuted_models, which):
    cols, g = _permuted_input(which)
    n = len(cols[0])
    n_points, W = PERMUTED
    try:
        ctx.set_simd_width(W)
        first = _run_both(ctx, cols, g, ge.PROBE, n_points)
        _assert_model(first, permuted_models[which], which)
        assert int(np.diff(first[0].astype(np.int64)).max()) >= (200 if which == "cluster_300" else 3)
        for seed in (1, 2, 3):
            perm = np.random.default_rng(seed).permutation(n)            # new atom i is old atom perm[i]
            got = ctx.group_contacts(*(np.ascontiguousarray(a[perm]) for a in cols), np.ascontiguousarray(g[perm]),
                                     ge.PROBE, n_points)
            _check_shapes(got, n)
            want = _take_atoms(first, perm)
            for k in range(6):
                assert np.array_equal(got[k], want[k]), (seed, k)
            assert got[6].tobytes() == want[6].tobytes()
        # order-preserving: g -> 2 g + 5 on the labels below 2^30 (the others stay, above all of those)
        low = g < np.uint32(1 << 30)
        f = lambda a: np.where(a < np.uint32(1 << 30), a * np.uint32(2) + np.uint32(5), a).astype(np.uint32)  # noqa: E731
        u = np.unique(g)
        assert low.any() and np.all(np.diff(f(u).astype(np.int64)) > 0) and not np.array_equal(f(g), g)
        got = ctx.group_contacts(*cols, f(g), ge.PROBE, n_points)
        assert np.array_equal(got[1], f(first[1]))
        for k in (0, 2, 3, 4, 5):
            assert np.array_equal(got[k], first[k]), k
        assert got[6].tobytes() == first[6].tobytes()
        # order-reversing: g -> 0xFFFFFFFF - g
        got = ctx.group_contacts(*cols, np.uint32(0xFFFFFFFF) - g, ge.PROBE, n_points)
        want = _reverse_rows(first)
        assert np.array_equal(got[1], np.uint32(0xFFFFFFFF) - want[1])
        for k in (0, 2, 3, 4, 5):
            assert np.array_equal(got[k], want[k]), k
        assert got[6].tobytes() == first[6].tobytes()
    finally:
        ctx.set_simd_width(8)


# ---- 6: ids -----------------------------------------------------------------------------------------------------------

ID_KINDS = ("head_against_rest", "alternating")


def _id_case(kind):
    cols, c0 = nh.tight_cluster(514, seed=514, shared_ids=True)
    n = len(cols[0])
    g = np.arange(n, dtype=np.uint32) % np.uint32(3) if kind == "alternating" else ge.cluster_labels(kind, n, c0)
    return cols, g, c0


@pytest.fixture(scope="module")
def id_models():
    return pe.pmap(lambda k: gm.group_counts(*_id_case(k[0])[0], _id_case(k[0])[1], ge.PROBE, k[1], ge.W),
                   [(kind, p) for kind in ID_KINDS for p in ge.CLUSTER_POINTS])


@pytest.mark.parametrize("n_points", ge.CLUSTER_POINTS)
@pytest.mark.parametrize("kind", ID_KINDS)
def test_ids_shorten_long_lists(ctx, id_models, kind, n_points):
    cols, g, c0 = _id_case(kind)
    k = np.diff(nh.oracle_csr(*cols, ge.PROBE)[0].astype(np.int64))
    plain = np.diff(nh.oracle_csr(*cols[:4], None, ge.PROBE)[0].astype(np.int64))
    short = k < plain
    assert short.sum() == 514 // 3 and k[short].min() > pe.PT_STAGE and plain[short].min() == 513
    try:
        ctx.set_simd_width(ge.W)
        got = _run_both(ctx, cols, g, ge.PROBE, n_points)
    finally:
        ctx.set_simd_width(8)
    _assert_model(got, id_models[(kind, n_points)], (kind, n_points))
    _assert_identities(got, g)
    without = ctx.group_contacts(*cols[:4], None, g, ge.PROBE, n_points)
    assert not np.array_equal(without[0], got[0]) or not np.array_equal(without[2], got[2])   # the ids matter here


def test_own_id_never_buries(ctx):
    """Every atom with one id: no list, so no rows and every point free, whatever the labels.  And the larger copy of
    atom 0 at its own centre (test_gpu_points.py): with atom 0's id it is no entry of atom 0's list."""
    x, y, z, r, ids = nh.protor("1jcd.pdb")
    n = len(x)
    for g in (ge.blocked(n), np.arange(n, dtype=np.uint32)):
        got = _run_both(ctx, (x, y, z, r, np.full(n, 7, np.uint64)), g, ge.PROBE, 100)
        assert int(got[0][-1]) == 0 and len(got[1]) == 0
        assert np.all(got[4] == 100) and np.all(got[5] == 100)
    big = np.float32(r[0] + np.float32(0.2))
    assert big <= r.max()
    X, Y, Z = (np.append(a, a[0]).astype(np.float32) for a in (x, y, z))
    R = np.append(r, big).astype(np.float32)
    g = np.append(ge.blocked(n), np.uint32(999)).astype(np.uint32)
    alone = ctx.group_contacts(x, y, z, r, ids, g[:n], ge.PROBE, 100)
    for copy_id, buried in ((ids[0], False), (np.uint64(10 ** 9), True)):
        I = np.append(ids, copy_id).astype(np.uint64)  # noqa: E741
        got = _run_both(ctx, (X, Y, Z, R, I), g, ge.PROBE, 100)
        _assert_model(got, gm.group_counts(X, Y, Z, R, I, g, ge.PROBE, 100, 8), buried)
        rows0 = slice(int(got[0][0]), int(got[0][1]))
        if buried:
            assert got[5][0] == 0 and 999 in got[1][rows0].tolist()
        else:
            assert 999 not in got[1][rows0].tolist() and got[5][0] == alone[5][0] and got[4][0] == alone[4][0]
            assert np.array_equal(got[2][rows0], alone[2][int(alone[0][0]):int(alone[0][1])])


# ---- 7: one context, many calls -----------------------------------------------------------------------------------

def _walk_big():
    big = bw.synthetic_proteome(30, seed=8)
    bg = ((np.arange(big.n_atoms, dtype=np.int64) - ge.structure_base(big.structure_offsets)) // 40).astype(np.uint32)
    return big, bg


@pytest.fixture(scope="module")
def walk_big_models():
    big, bg = _walk_big()
    return {p: ge.batch_model(big.x, big.y, big.z, big.radius, big.ids, bg, big.structure_offsets, ge.PROBE, p, 8)
            for p in WALK_BIG_POINTS}


def test_one_context_through_group_calls(cluster_models, walk_big_models):
    """A fresh context through group calls between those of the other families: the big batch (30 structures, labels
    index // 40 within each, 260 points: the model's cost is the point count's, and 260 is still two passes of four
    chunks), 1jcd at 100 points and W = 16, own_then_many at 769 atoms and 300 points (469 rows per atom: those past
    the registers are stored into row buffers that earlier calls have filled), the same atoms under one_label (no rows, in
    buffers that still hold rows), a sizing call, a call that fails on an infinite coordinate, precompute_neighbors,
    contact_points and accessible_points on other sizes, lane counts changed in between, the sparse structure whose
    grid overflows the remembered cells, then the first three calls again.  Every group call against its model."""
    import rustsasa_amd
    from rustsasa_amd import _capi
    big, bg = _walk_big()
    bigc = (big.x, big.y, big.z, big.radius, big.ids)
    bso = big.structure_offsets
    small = nh.protor("1jcd.pdb")
    sg = ge.blocked(len(small[0]))
    mid = nh.protor("151L_H3.pdb")
    rng = np.random.default_rng(31)
    sp = (rng.uniform(0, 1, (300, 3)) * np.array([30000.0, 100.0, 100.0])).astype(np.float32)  # ~9 M cells
    sparse = (sp[:, 0].copy(), sp[:, 1].copy(), sp[:, 2].copy(), rng.uniform(1.2, 2.0, 300).astype(np.float32),
              np.arange(300, dtype=np.uint64))
    spg = np.arange(300, dtype=np.uint32) % np.uint32(2)
    assert big.n_atoms * 20 < 9_000_000 and big.n_structures == 30 and bg.max() > 50
    otm, otm_g, c0 = ge.cluster(769, "own_then_many")
    _, one_g, _ = ge.cluster(769, "one_label")
    gkeys = {"small100": (small, sg, 100, 16), "small64": (small, sg, 64, 4), "otm300": (otm, otm_g, 300, ge.W),
             "one300": (otm, one_g, 300, ge.W), "sparse129": (sparse, spg, 129, 4),
             "mid130": (mid, ge.blocked(len(mid[0])), 130, 8)}
    G = {k: ge.batch_model(*cols, g, np.array([0, len(g)], np.uint32), ge.PROBE, p, W, chunk=128)
         for k, (cols, g, p, W) in gkeys.items() if k not in ("otm300", "one300")}
    G["otm300"], G["one300"] = cluster_models[(769, "own_then_many", 300)], cluster_models[(769, "one_label", 300)]
    pkeys = {"small64": (small, 64, 4), "mid130": (mid, 130, 8), "sparse129": (sparse, 129, 4)}
    P = pe.pmap(lambda k: pe.models(pkeys[k][0], ge.PROBE, pkeys[k][1], (pkeys[k][2],)), pkeys)
    big_model = walk_big_models
    assert int(np.diff(G["otm300"][0].astype(np.int64))[c0:].min()) == 469 > ge.ROW_REGS
    assert int(big_model[64][0][-1]) > 200_000 and int(G["one300"][0][-1]) < 30_000   # row buffers shrink and grow

    def big_groups(c, n_points):
        got = c.group_contacts_batch(*bigc, bg, bso, ge.PROBE, n_points)
        _assert_model(got, big_model[n_points], ("big", n_points))
        sasa, _ = c.calculate_sasa_batch(*bigc, bso, ge.PROBE, n_points)
        assert got[6].tobytes() == sasa.tobytes()

    def groups(c, key):
        cols, g, n_points, W = gkeys[key]
        c.set_simd_width(W)
        got = _run_both(c, cols, g, ge.PROBE, n_points)
        _assert_model(got, G[key], key)
        _assert_identities(got, g)
        return got

    def one_label(c):
        got = groups(c, "one300")
        assert got[0][c0] == got[0][-1] and np.array_equal(got[4][c0:], got[5][c0:])

    def sizing(c):
        c.set_simd_width(16)
        rc, offs = _sizing_call(c, *small, sg, np.array([0, len(sg)], np.uint32), ge.PROBE, 100)
        assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL and np.array_equal(offs, G["small100"][0])

    def infinite(c):
        bad = small[0].copy()
        bad[3] = np.inf
        with pytest.raises(rustsasa_amd.RsasaError) as e:
            c.group_contacts(bad, *small[1:], sg, ge.PROBE, 100)
        assert e.value.status == -5

    def neighbours(c, key):
        nh.assert_same(c.precompute_neighbors(*pkeys[key][0], ge.PROBE), P[key][:2])

    def contacts(c, key):
        cols, n_points, W = pkeys[key]
        c.set_simd_width(W)
        got = c.contact_points(*cols, ge.PROBE, n_points)
        nh.assert_same(got[:2], P[key][:2])
        assert np.array_equal(got[2], P[key][2][W][1]) and np.array_equal(got[3], P[key][2][W][2])

    def points(c, key):
        cols, n_points, W = pkeys[key]
        c.set_simd_width(W)
        words, _ = c.accessible_points(*cols, ge.PROBE, n_points)
        assert np.array_equal(words, pm.pack(P[key][2][W][0]))

    def w8(c):
        c.set_simd_width(8)

    first = [w8,
             lambda c: big_groups(c, WALK_BIG_POINTS[0]),     # big, W = 8
             lambda c: groups(c, "small100"),                 # 100 points, small, W = 16
             lambda c: groups(c, "otm300")]                   # rows past the registers, W = 16
    seq = first + [
        one_label,                                            # no rows, in buffers that hold rows
        sizing,
        lambda c: contacts(c, "small64"),                     # the lattice shrinks to 64 points, W = 4
        lambda c: groups(c, "small64"),
        infinite,
        lambda c: neighbours(c, "sparse129"),                 # the cell array regrows
        lambda c: groups(c, "sparse129"),                     # 129 points: the NCH = 4 kernel, W = 4
        lambda c: points(c, "mid130"),
        lambda c: groups(c, "mid130"),
        lambda c: contacts(c, "sparse129"),
        w8,
        lambda c: big_groups(c, WALK_BIG_POINTS[1]),
        lambda c: points(c, "small64"),
    ] + first
    with rustsasa_amd.Context(0) as c:
        for step in seq:
            step(c)


# ---- 8: radii and probes off the protein range, several structures per batch --------------------------------------

def _degenerate_batches():
    """{probe: (columns, labels, structure offsets)}: the degenerate copies of 1jcd that share a probe, in one batch
    between two ordinary structures."""
    cols = nh.protor("1jcd.pdb")
    b = bw.synthetic_proteome(30, seed=8)
    first, last = tuple(b.structure(0)), tuple(b.structure(4))
    by_probe = {}
    for label, probe, r in pe.degenerate_settings(cols[3]):
        by_probe.setdefault(probe, []).append(pe.with_radii(cols, r))
    assert sum(len(v) for v in by_probe.values()) == 10 and len(by_probe[1.4]) == 5 and len(by_probe[0.0]) == 2
    return {probe: ge.pack([(c, ge.blocked(len(c[0]))) for c in [first] + sts + [last]]) for probe, sts in by_probe.items()}


@pytest.fixture(scope="module")
def degenerate_models():
    batches = _degenerate_batches()
    return batches, {probe: ge.batch_model(*cat, g, so, probe, *DEGENERATE, chunk=128) for probe, (cat, g, so) in batches.items()}


@pytest.mark.parametrize("probe", [1.4, 0.0, 0.05, 33.0, 2.0])
def test_degenerate_radii_and_probes_in_a_batch(ctx, degenerate_models, probe):
    batches, models = degenerate_models
    assert sorted(batches) == sorted([1.4, 0.0, 0.05, 33.0, 2.0])
    cat, g, so = batches[probe]
    n_points, W = DEGENERATE
    try:
        ctx.set_simd_width(W)
        got = ctx.group_contacts_batch(*cat, g, so, probe, n_points)
        sasa, _ = ctx.calculate_sasa_batch(*cat, so, probe, n_points)
    finally:
        ctx.set_simd_width(8)
    _assert_model(got, models[probe], probe)
    assert got[6].tobytes() == sasa.tobytes()
