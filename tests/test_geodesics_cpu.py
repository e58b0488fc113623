"""The dot links and dot geodesics without a GPU: the model (geodesics_model.py) against witnesses - a chaotic
Bellman-Ford that must reach the same bits, a float64 Dijkstra and the float64 chord within a derived rounding margin, a
lone atom by hand; exact identities; every input of geodesics_cases.py pinned to what it is named for, each with the
switch that shows it bites; the host helpers against direct loops; the binding table; and the new rules of
entry_checks.h in a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import dijkstra as sp_dijkstra

import component_cases as cc
import components_model as cm
import depth_model as dm
import geodesics_cases as gc
import geodesics_model as gm

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24          # the relative error of one float32 rounding
NONE = 0xFFFFFFFF


def _one(name, n_points=100, link=None):
    """The lists of a one-structure case: (case, link_offsets int64, idx, w float32, d2, dots (qx, qy, qz), mask)."""
    c = gc.get(name)
    link = cc.default_link(c.r, c.probe, n_points) if link is None else F(link)
    off, loff, ent, mask = gm.links(*c.cols[:4], c.ids, c.probe, n_points, link)
    q = dm.dots_of(*c.cols[:4], mask, c.probe, n_points)[1:]
    return c, loff.astype(np.int64), ent["idx"].astype(np.int64), gm.weights(ent), ent["d2"], q, mask


def _chaotic(loff, idx, w, seeds, limit, rng, share=0.7):
    """dist by Bellman-Ford over a random `share` of the edges per round, in place, until a full round changes nothing."""
    n = len(loff) - 1
    u = np.repeat(np.arange(n), np.diff(loff))
    dist = np.where(seeds != 0, F(0.0), F(np.inf)).astype(F)
    rounds = 0
    while True:
        rounds += 1
        full = rounds % 4 == 0
        m = np.ones(len(u), bool) if full else rng.random(len(u)) < share
        nd = dist[u[m]] + w[m]
        assert nd.dtype == F
        nd[~(nd <= F(limit))] = np.inf
        new = dist.copy()
        np.minimum.at(new, idx[m], nd)
        if full and np.array_equal(new, dist):
            return dist, rounds
        dist = new


# ---- 1: the model against witnesses --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n_points,link", [("corner", 100, None), ("cavity", 100, None), ("twins", 100, None),
                                                ("twins", 100, 0.0), ("equal_sum", 1, 3.0), ("example_vdw", 100, None)])
def test_chaotic_relaxation_reaches_the_models_bits(name, n_points, link):
    _, loff, idx, w, _, _, _ = _one(name, n_points, link)
    n = len(loff) - 1
    rng = np.random.default_rng(31)
    runs = 1 if name == "example_vdw" else 3
    for k in range(runs):
        seeds = np.zeros(n, np.uint8)
        seeds[rng.integers(0, n, 1 + 2 * k)] = 1
        for limit in (np.inf, 9.0, 2.5)[:3 if runs > 1 else 1]:
            want = gm.dijkstra(loff, idx, w, seeds, limit)
            got, _ = _chaotic(loff, idx, w, seeds, limit, rng)
            assert got.tobytes() == want.tobytes(), (name, k, limit)


@pytest.mark.parametrize("name", ["corner", "cavity", "jcd"])
def test_float64_dijkstra_and_the_chord_within_the_rounding_margin(name):
    """With e = 2^-24: a path of k edges carries k roundings of sqrt (each at most e of its weight, e L together) and
    k - 1 of a sum (each at most e of a partial sum, which is at most the float32 length), so its float32 length L32 and
    its length L64 with the same d2 satisfy |L32 - L64| <= k e max(L32, L64) (1 + k e), the last factor being the second
    order.  The shorter path of either arithmetic is a path of the other, so the two minima differ by no more, with k
    the larger of the two paths' edge counts: the issue's hops 2^-24 dist.  For the chord the roundings of d2 itself
    count too: dx carries e, dx * dx 3 e, the sum of three squares 5 e, its root 2.5 e and the root's rounding 1 e, the
    running sum 1 e - 4.5 e an edge, taken as 5 k e; a path is no shorter than the chord between its ends."""
    _, loff, idx, w, d2, q, _ = _one(name)
    n = len(loff) - 1
    seeds = np.zeros(n, np.uint8)
    seeds[[n // 5, n // 2]] = 1
    d32, k32 = gm.dijkstra(loff, idx, w, seeds, with_hops=True)
    g = csr_matrix((np.sqrt(d2.astype(np.float64)) + 1e-300, idx, loff), shape=(n, n))
    d64, pred = sp_dijkstra(g, directed=True, indices=np.flatnonzero(seeds), return_predecessors=True, min_only=True)[:2]
    k64 = np.zeros(n, np.int64)
    for v in np.argsort(d64):                       # (a predecessor is settled before its successor)
        if pred[v] >= 0:
            k64[v] = k64[pred[v]] + 1
    assert np.array_equal(np.isfinite(d32), np.isfinite(d64))
    fin = np.isfinite(d32)
    k = np.maximum(k32, k64)[fin]
    margin = k * EPS * np.maximum(d32[fin].astype(np.float64), d64[fin]) * (1.0 + k * EPS)
    assert (np.abs(d32[fin].astype(np.float64) - d64[fin]) <= margin).all()
    assert k32.max() >= 10                          # (paths of ten edges and more are among those compared)
    pts = np.stack(q, -1).astype(np.float64)
    s = np.flatnonzero(seeds)
    chord = np.min(np.linalg.norm(pts[:, None, :] - pts[None, s, :], axis=-1), axis=1)
    assert (d32[fin].astype(np.float64) * (1.0 + 5.0 * k32[fin] * EPS) >= chord[fin]).all()


def test_a_lone_atom_by_hand():
    """One atom, 100 points, R = 3.16: one component; the dot farthest in space from dot 0 is nearly antipodal (chord
    above 1.95 R), its dist is no shorter than that chord and no longer than 1.5 pi R - the great circle is pi R, and a
    path over lattice dots at the default link (1.5 dot spacings) wanders less than half as much again."""
    c, loff, idx, w, _, q, mask = _one("lone")
    assert mask.all() and len(w) > 0
    R = float(F(c.r[0]) + F(c.probe))
    seeds = gc.one_seed(100, 0)
    dist = gm.dijkstra(loff, idx, w, seeds)
    assert np.isfinite(dist).all()
    pts = np.stack(q, -1).astype(np.float64)
    chord = np.linalg.norm(pts - pts[0], axis=1)
    far = int(np.argmax(chord))
    assert chord[far] > 1.95 * R and chord[far] * (1 - 1e-5) <= dist[far] <= 1.5 * np.pi * R
    assert dist[far] > 2.0 * R * 0.975 and (dist <= 1.5 * np.pi * R).all()
    assert (gm.sources_of(loff, idx, w, dist, seeds) == 0).all()


# ---- 2: identities ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cavity", "example_vdw"])
def test_finite_exactly_where_the_component_holds_a_seed(name):
    c, loff, idx, w, _, q, _ = _one(name)
    n = len(loff) - 1
    labels = cm.labels_of(n, cm.edges_of(*q, cc.default_link(c.r, c.probe, 100)))
    assert len(np.unique(labels)) > 1
    rng = np.random.default_rng(8)
    seeds = np.zeros(n, np.uint8)
    seeds[rng.integers(0, n, 2)] = 1
    small = np.flatnonzero(labels != np.bincount(labels).argmax())
    seeds[small[0]] = 1
    dist = gm.dijkstra(loff, idx, w, seeds)
    assert np.array_equal(np.isfinite(dist), np.isin(labels, labels[seeds != 0]))
    src = gm.sources_of(loff, idx, w, dist, seeds)
    assert np.array_equal(src == NONE, np.isinf(dist)) and (seeds[src[src != NONE]] != 0).all()
    assert np.array_equal(labels[src[src != NONE]], labels[src != NONE])           # a source lies in the dot's component
    one = gc.one_seed(n, int(small[0]))
    d1 = gm.dijkstra(loff, idx, w, one)
    assert (gm.sources_of(loff, idx, w, d1, one)[np.isfinite(d1)] == small[0]).all()  # a single seed is everybody's source


def test_a_permutation_of_the_atoms_permutes_the_results():
    c = gc.get("corner")
    link = cc.default_link(c.r, c.probe, 100)
    off, loff, ent, mask = gm.links(*c.cols[:4], c.ids, c.probe, 100, link)
    perm = np.random.default_rng(4).permutation(c.n_atoms)
    cols = [a[perm] for a in c.cols]
    off2, loff2, ent2, mask2 = gm.links(*cols[:4], cols[4], c.probe, 100, link)
    assert np.array_equal(mask2, mask[perm])
    # new dot -> old dot: atom perm[i]'s block of dots, in order
    old = np.concatenate([np.arange(int(off[p]), int(off[p + 1])) for p in perm]).astype(np.int64)
    new_of = np.empty_like(old)
    new_of[old] = np.arange(len(old))
    seeds = gc.one_seed(len(old), 37)
    d = gm.dijkstra(loff.astype(np.int64), ent["idx"], gm.weights(ent), seeds)
    seeds2 = np.zeros_like(seeds)
    seeds2[new_of[37]] = 1
    d2 = gm.dijkstra(loff2.astype(np.int64), ent2["idx"], gm.weights(ent2), seeds2)
    assert d2.tobytes() == d[old].tobytes()
    assert np.array_equal(np.diff(loff2.astype(np.int64)), np.diff(loff.astype(np.int64))[old])
    s2 = gm.sources_of(loff2.astype(np.int64), ent2["idx"], gm.weights(ent2), d2, seeds2)
    assert (s2[np.isfinite(d2)] == new_of[37]).all()


def test_lists_are_sorted_symmetric_and_without_self():
    for name, n_points, link in (("example_vdw", 100, None), ("twins", 100, 0.0), ("pole_tie", 1, 3.0)):
        _, loff, idx, _, d2, _, _ = _one(name, n_points, link)
        n = len(loff) - 1
        u = np.repeat(np.arange(n), np.diff(loff))
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
        same = u[1:] == u[:-1]
        assert (key[1:][same] > key[:-1][same]).all() and (u != idx).all()
        fwd = set(zip(u.tolist(), idx.tolist(), d2.view(np.uint32).tolist()))
        assert fwd == {(b, a, k) for a, b, k in fwd}
    _, loff, idx, _, d2, _, _ = _one("example_vdw")
    assert len(idx) == 140176 and len(loff) - 1 == 16843 and np.diff(loff).max() == 20 and np.diff(loff).min() == 0
    assert abs(float(np.sqrt(d2.min())) - 0.087) < 1e-3


def test_the_figures_of_the_example():
    _, loff, idx, w, _, _, _ = _one("example_vdw")
    n = len(loff) - 1
    labels_size = np.bincount(cm.labels_of(n, np.stack([np.repeat(np.arange(n), np.diff(loff)), idx], -1)))
    outer = int(labels_size.argmax())
    dist = gm.dijkstra(loff, idx, w, gc.one_seed(n, outer))
    assert abs(float(dist[np.isfinite(dist)].max()) - 141.02) < 0.01
    assert np.isfinite(gm.dijkstra(loff, idx, w, gc.one_seed(n, outer), 12.0)).sum() == 421


# ---- 3: every case is what it is named for ---------------------------------------------------------------------------------

def _packed(n, edges, seeds, order):
    """(dist, source) minimised as ONE 64-bit number, edges relaxed in the given order until nothing changes."""
    key = np.full(n, (int(F(np.inf).view(np.uint32)) << 32) | NONE, np.uint64)
    for s in np.flatnonzero(seeds):
        key[s] = s
    changed = True
    while changed:
        changed = False
        for e in order:
            u, v, w = edges[e]
            d = (F(np.uint32(int(key[u]) >> 32).view(F)) + F(w))
            cand = (int(F(d).view(np.uint32)) << 32) | (int(key[u]) & NONE)
            if np.isfinite(d) and cand < int(key[v]):
                key[v] = cand
                changed = True
    return (key >> np.uint64(32)).astype(np.uint32).view(F), (key & np.uint64(NONE)).astype(np.uint32)


def test_equal_sum_moves_a_packed_source_and_not_the_models():
    c, loff, idx, w, _, _, mask = _one("equal_sum", 1, 3.0)
    assert mask.all() and len(loff) - 1 == 4
    seeds = c.info["seeds"]
    dist = gm.dijkstra(loff, idx, w, seeds)
    src = gm.sources_of(loff, idx, w, dist, seeds)
    assert dist.tolist() == [0.0, 0.0, 1.0, 4.0] and src.tolist() == [0, 1, 1, 1]
    u = np.repeat(np.arange(4), np.diff(loff))
    edges = list(zip(u.tolist(), idx.tolist(), w.tolist()))
    w02 = [e for e, (a, b, _) in enumerate(edges) if (a, b) == (0, 2)][0]
    w12 = [e for e, (a, b, _) in enumerate(edges) if (a, b) == (1, 2)][0]
    w23 = [e for e, (a, b, _) in enumerate(edges) if (a, b) == (2, 3)][0]
    assert edges[w02][2] == float(F(1.0) + F(2.0 ** -23)) and edges[w12][2] == 1.0 and edges[w23][2] == 3.0
    assert F(edges[w02][2]) + F(3.0) == F(4.0)                                  # the two sums are equal
    late = _packed(4, edges, seeds, [w02, w23, w12, w23])                      # dot 2 hears of seed 0 first
    early = _packed(4, edges, seeds, [w12, w23, w02, w23])
    assert late[0].tolist() == early[0].tolist() == dist.tolist()               # the distances do not care
    assert late[1][3] == 0 and early[1][3] == 1                                 # the packed source does: schedule dependent
    assert src[3] == 1


def test_chain_is_longer_than_the_rounds_between_two_looks():
    text = open(os.path.join(ROOT, "rustsasa_amd", "csrc", "device_types.h")).read()
    k_rounds = int(re.search(r"constexpr uint32_t kGdRounds = (\d+);", text).group(1))
    _, loff, idx, w, _, _, _ = _one("chain")
    n = len(loff) - 1
    seeds = gc.one_seed(n, 0)
    h = gm.hops(loff, idx, seeds)
    assert (h >= 0).all() and h.max() >= 200 and h.max() > 10 * k_rounds
    dist, k = gm.dijkstra(loff, idx, w, seeds, with_hops=True)
    assert k.max() >= 200 and dist.max() > (gc.CHAIN_ATOMS - 1) * gc.CHAIN_STEP
    # the switch: a relaxation stopped after the first look has not arrived
    u = np.repeat(np.arange(n), np.diff(loff))
    d = np.where(seeds != 0, F(0), F(np.inf)).astype(F)
    for _ in range(k_rounds):
        new = d.copy()
        np.minimum.at(new, idx, d[u] + w)
        d = new
    assert np.isinf(d).sum() > n // 2


def test_lone_twins_counts_and_fixtures_are_what_they_are_named_for():
    _, loff, _, _, _, _, _ = _one("lone", 960, 6.33)
    assert (np.diff(loff) == 959).all()
    _, loff, _, _, _, _, _ = _one("lone", 960, 5.0)
    assert 512 < np.diff(loff).max() < 959
    _, loff, _, _, _, _, _ = _one("lone", 960, 3.0)
    assert 64 < np.diff(loff).max() < 512
    _, loff, idx, w, _, _, _ = _one("twins", 100, 0.0)
    assert len(w) == 180 and not w.any()                                        # zero-weight edges only
    c = gc.get("dot_counts")
    mask = gm.links_batch(*c.cols, c.so, c.probe, gc.COUNT_POINTS, cc.default_link(c.r, c.probe, gc.COUNT_POINTS))[3]
    assert mask.sum(axis=1)[c.info["first"]].tolist() == list(gc.COUNTS)
    assert gc.get("jcd").n_atoms > 500 and len(gc.get("jcd").so) == 2


def test_a_limit_one_ulp_below_a_distance_loses_the_dot_and_what_hangs_on_it():
    _, loff, idx, w, _, _, _ = _one("corner")
    n = len(loff) - 1
    seeds = gc.one_seed(n, 7)
    full = gm.dijkstra(loff, idx, w, seeds)
    v = int(np.argsort(full, kind="stable")[np.isfinite(full).sum() // 2])
    at, below = gm.dijkstra(loff, idx, w, seeds, full[v]), gm.dijkstra(loff, idx, w, seeds, np.nextafter(full[v], F(0)))
    assert at[v] == full[v] and np.isinf(below[v])
    assert np.array_equal(at[np.isfinite(at)], full[np.isfinite(at)]) and (full[np.isinf(at)] > full[v]).all()
    assert np.isfinite(below).sum() < np.isfinite(at).sum()
    zero = gm.dijkstra(loff, idx, w, seeds, 0.0)
    assert np.isfinite(zero).sum() == 1 and zero[7] == 0


# ---- 4: the helpers and the binding table ------------------------------------------------------------------------------------

def test_helpers_against_direct_loops():
    import rustsasa_amd
    c = gc.get("tiny")
    off, loff, ent, _ = gm.links_batch(*c.cols, c.so, c.probe, 100, cc.default_link(c.r, c.probe, 100))
    D = int(off[-1])
    # dot_seeds
    for atoms in ([0], [2, 5], [], np.array([1, 1, 4])):
        want = np.zeros(D, np.uint8)
        for i in atoms:
            want[int(off[i]):int(off[i + 1])] = 1
        got = rustsasa_amd.dot_seeds(off, atoms)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    m = np.zeros(c.n_atoms, bool)
    m[[0, 3]] = True
    assert np.array_equal(rustsasa_amd.dot_seeds(off, m), rustsasa_amd.dot_seeds(off, [0, 3]))
    with pytest.raises(ValueError):
        rustsasa_amd.dot_seeds(off, [c.n_atoms])
    # dot_structure_offsets
    dso = rustsasa_amd.dot_structure_offsets(off, c.so)
    assert dso.dtype == np.int64 and dso.tolist() == [int(off[int(s)]) for s in c.so]
    assert rustsasa_amd.dot_structure_offsets(off).tolist() == [0, D]
    # edge_index gives the dot graph unchanged
    e = rustsasa_amd.edge_index(loff, ent, dso)
    assert e.dtype == np.int64 and e.shape == (2, len(ent))
    k = 0
    for s in range(len(c.so) - 1):
        for d in range(int(dso[s]), int(dso[s + 1])):
            for j in range(int(loff[d]), int(loff[d + 1])):
                assert e[0, k] == d and e[1, k] == int(dso[s]) + int(ent["idx"][j])
                k += 1
    assert k == len(ent) > 0


def test_binding_table_and_the_documents():
    from rustsasa_amd import _capi
    header = open(os.path.join(ROOT, "include", "rustsasa_amd.h")).read()
    assert "#define RSASA_ABI_VERSION 4" in header
    assert "rsasa_dot_links, rsasa_dot_links_batch; rsasa_dot_geodesics, rsasa_dot_geodesics_batch;\n * rsasa_context_geodesic_rounds. */" in header
    assert "rsasa_dot_links*: for out_link_offsets and out_entries" in header
    for name, n_args in (("rsasa_dot_links", 18), ("rsasa_dot_links_batch", 19), ("rsasa_dot_geodesics", 18),
                         ("rsasa_dot_geodesics_batch", 19), ("rsasa_context_geodesic_rounds", 2)):
        assert f"int {name}(" in header
        res, args = _capi.SYMBOLS[name]
        assert res is C.c_int and len(args) == n_args
    extra = 1
    assert _capi.SYMBOLS["rsasa_dot_links_batch"][1][10] is C.c_float                        # link
    assert _capi.SYMBOLS["rsasa_dot_links_batch"][1][14] is C.c_size_t and _capi.SYMBOLS["rsasa_dot_links_batch"][1][16] is C.c_size_t
    g = _capi.SYMBOLS["rsasa_dot_geodesics_batch"][1]
    assert g[9 + extra] is C.c_float and g[11 + extra] is C.c_size_t and g[12 + extra] is C.c_float    # link, n_seed_bytes, limit
    lib = _capi.load()
    assert all(hasattr(lib, n) for n in ("rsasa_dot_links", "rsasa_dot_links_batch", "rsasa_dot_geodesics", "rsasa_dot_geodesics_batch",
                                         "rsasa_context_geodesic_rounds"))
    assert lib.rsasa_abi_version() == 4
    # the definition, in the same words everywhere
    squash = lambda t: re.sub(r"[\s*/#`>]+", " ", t)  # noqa: E731
    docs = {"header": header, "model": gm.__doc__, "README": open(os.path.join(ROOT, "README.md")).read(),
            "DESIGN": open(os.path.join(ROOT, "DESIGN.md")).read()}
    for sentence in ("The edge weight is w(a, b) = sqrtf(d2), correctly rounded",
                     "The length of a path v0 ... vk is the left-to-right sum ((0 + w1) + w2) + ...",
                     "dist[v] is the minimum over all paths from any seed to v whose length, and hence every prefix, is <= limit"):
        for where, text in docs.items():
            assert squash(sentence) in squash(text), (where, sentence)
    for doc in ("README", "DESIGN"):
        assert "dot_links" in docs[doc] and "dot_geodesics" in docs[doc]
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "rsasa_dot_links" in integ and "rsasa_dot_geodesics" in integ
    srcs = open(os.path.join(ROOT, "rustsasa_amd", "csrc", "Makefile")).read()
    assert " geodesics.hip " in srcs and "-ffp-contract=off" in srcs


def test_python_argument_checks_without_a_gpu():
    """The checks Context.dot_geodesics makes before it reaches the library, on a Context that has none (no call below
    gets as far as the C entry point: each must raise first)."""
    import rustsasa_amd
    assert "dot_seeds" in rustsasa_amd.__all__ and "dot_structure_offsets" in rustsasa_amd.__all__
    for name in ("dot_links", "dot_links_batch", "dot_geodesics", "dot_geodesics_batch", "geodesic_rounds"):
        assert callable(getattr(rustsasa_amd.Context, name))
    ctx = object.__new__(rustsasa_amd.Context)              # no device, no handle, no library
    c = gc.get("tiny")
    ok = np.zeros(10, np.uint8)
    one = lambda seeds, **kw: ctx.dot_geodesics(*c.cols, c.probe, 100, seeds, **kw)                      # noqa: E731
    many = lambda seeds, **kw: ctx.dot_geodesics_batch(*c.cols, c.so, c.probe, 100, seeds, **kw)        # noqa: E731
    for call in (one, many):
        for seeds in (None, np.zeros(10, F), np.zeros((5, 2), np.uint8), np.array(["a"]), 3):
            with pytest.raises(ValueError, match="seeds must be a 1-D array"):
                call(seeds)
        for limit in (-1.0, float("nan"), -float("inf"), -1e-30):
            with pytest.raises(ValueError, match="limit must be None"):
                call(ok, limit=limit)
        with pytest.raises(ValueError):
            call(ok, limit="far")
        with pytest.raises(ValueError, match="n_points"):
            ctx.dot_links(*c.cols, c.probe, 0)
    for seeds, limit in ((ok, None), (ok.astype(bool), 0.0), (ok.astype(np.int64), float("inf")), (ok, -0.0)):
        with pytest.raises(AttributeError):                 # the checks pass; the Context has no library to call
            one(seeds, limit=limit)
    with pytest.raises(ValueError, match="the length of x"):
        ctx.dot_links(c.x, c.y[:-1], c.z, c.r, c.ids)


def test_new_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "geodesic_checks_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "rustsasa_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "geodesic_checks_test.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "geodesic checks ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-2000:])


@pytest.mark.parametrize("name,n_points,link", [("example_vdw", 100, None), ("far_link", cc.FAR_POINTS, float(cc.H)),
                                                ("margin_pair0", 100, None), ("twins", 100, None), ("lone", 960, 1e4)])
def test_the_staging_cut_keeps_every_linked_pair(name, n_points, link):
    """k_dot_link stages atom j for atom i only if, in float32, |c_j - c_i|^2 <= (((R_i + link) + h) + R_j)^2.  The same
    expression on the owners of every edge of the model: none is cut, and the exact centre distance stays h / 2 and more
    inside the bound (the proof needs h / 8 of the whole h).  This restates the expression in numpy: it tests the proof,
    not the kernel - a change of the expression in k_dot_link goes unnoticed here.  What catches a cut that is too tight
    in the code are the GPU comparisons with the model on far_link (centres just under R_i + R_j + link apart), on the
    margin pairs and on the 65 536-atom structure (test_gpu_geodesics.py)."""
    import sweep_cases as sc
    c = sc.margin_pair(0) if name == "margin_pair0" else gc.get(name)
    link = F(cc.default_link(c.r, c.probe, n_points) if link is None else link)
    off, loff, ent, mask = gm.links_batch(*c.cols, c.so, c.probe, n_points, link)
    owner = np.repeat(np.arange(c.n_atoms), np.diff(off.astype(np.int64)))
    sid = np.repeat(np.arange(len(c.so) - 1), np.diff(c.so.astype(np.int64)))
    base = off.astype(np.int64)[c.so[:-1].astype(np.int64)][sid]
    a = np.repeat(np.arange(len(loff) - 1), np.diff(loff.astype(np.int64)))
    i, j = owner[a], owner[ent["idx"].astype(np.int64) + base[owner[a]]]
    assert len(i) > 0
    h = np.array([F(c.probe) + c.r[int(c.so[s]):int(c.so[s + 1])].max() if c.so[s + 1] > c.so[s] else F(0) for s in range(len(c.so) - 1)], F)[sid]
    R = c.r + F(c.probe)
    ex, ey, ez = c.x[j] - c.x[i], c.y[j] - c.y[i], c.z[j] - c.z[i]
    lim = ((R[i] + link) + h[i]) + R[j]
    d2 = ex * ex + ey * ey + ez * ez
    assert d2.dtype == F and lim.dtype == F and (d2 <= lim * lim).all()
    exact = np.sqrt((c.x[j].astype(np.float64) - c.x[i]) ** 2 + (c.y[j].astype(np.float64) - c.y[i]) ** 2 + (c.z[j].astype(np.float64) - c.z[i]) ** 2)
    assert (exact <= R[i].astype(np.float64) + R[j] + float(link) + 0.5 * h[i]).all()
    assert (owner[a] != j).any() or name == "lone"                  # edges between different atoms are among them


def test_the_bench_tool_records_the_resources_of_the_file_head():
    """tools/bench_geodesics.py writes its KERNELS table into profiles/geodesics_bench.json beside the times; the table,
    the one in the head of geodesics.hip and the committed record must be the same numbers."""
    import ast
    import json
    head = open(os.path.join(ROOT, "rustsasa_amd", "csrc", "geodesics.hip")).read().split("#include")[0]
    rows = re.findall(r"^//   (k_\w+)(?:<k(\w+)>)?\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", head, re.M)
    want = {(f"{n}<{m.lower()}>" if m else n): {"vgprs": int(v), "sgprs": int(s), "lds_bytes": int(lds), "scratch": int(sc)}
            for n, m, v, s, lds, sc in rows}
    assert len(want) == 8 and all(r["scratch"] == 0 for r in want.values())
    tool = open(os.path.join(ROOT, "tools", "bench_geodesics.py")).read()
    table = ast.literal_eval(re.search(r"^KERNELS = (\{.*?\}\})$", tool, re.M | re.S).group(1))
    assert table == want
    record = json.load(open(os.path.join(ROOT, "profiles", "geodesics_bench.json")))
    assert record["kernels"] == want and [c["workload"] for c in record["cases"]] == ["proteome", "real_coords"]
