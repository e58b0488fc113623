"""The atoms-within-a-cutoff lists without a GPU: the float32 model (within_model.py) against a float64 brute force, hand
lists and its own properties; every case of within_cases.py pinned to what it is named for; the header, the bindings,
the Python argument rules (which raise before any C call) and the numpy helpers edge_index / closest_pairs."""
import os
import subprocess

import numpy as np
import pytest

import hse_cases as hc
import hse_model as hm
import within_cases as wc
import within_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BAND = 1e-4
SEEDS = (100, 102, 103, 104, 107, 108)   # (test_hse_cpu.py's: no pair lies within BAND of a cutoff)
CUTOFFS64 = (3.5, 6.0, 13.0)


def _list(offsets, entries, i):
    return entries[int(offsets[i]):int(offsets[i + 1])]


def _sorted_lists(offsets, entries):
    """Every list ascending by key, keys distinct."""
    k = wm.keys(entries["d2"], entries["idx"])
    inner = np.ones(len(k), bool)
    inner[offsets[:-1][offsets[:-1] < len(k)].astype(np.int64)] = False
    return bool(np.all(k[1:][inner[1:]] > k[:-1][inner[1:]]))


# ---- the model ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_model_equals_a_float64_brute_force(seed):
    xyz = np.random.default_rng(seed).uniform(0.0, 20.0, (60, 3)).astype(F)
    x, y, z = (xyz[:, k].copy() for k in range(3))
    rng = np.random.default_rng(seed + 2)
    for flags in (None, rng.integers(0, 4, len(x)).astype(np.uint8)):
        for cutoff in CUTOFFS64:
            for upper in (False, True):
                want, dist, band = wm.brute64(x, y, z, flags, cutoff, upper)
                assert band > BAND, (cutoff, band)
                off, ent = wm.lists(x, y, z, flags, cutoff, upper)
                assert _sorted_lists(off, ent)
                for i in range(len(x)):
                    li = _list(off, ent, i)
                    assert set(li["idx"].tolist()) == want[i], (cutoff, i)
                    assert np.allclose(np.sqrt(li["d2"].astype(np.float64)), dist[i, li["idx"]], rtol=1e-6)
                assert off[-1] > 0 or flags is not None


def test_hand_lists():
    """hse_cases.hand(): cutoff 5, centres 0 and 4 (coincident), partners everybody.  From (1, 2, 3): atom 4 at d2 0, atom 2
    at 4, atoms 1 and 3 at 9, atom 5 at 49 (out)."""
    c = hc.hand()
    off, ent = wm.lists(c.x, c.y, c.z, c.flags, 5.0)
    assert off.tolist() == [0, 4, 4, 4, 4, 8, 8]
    assert _list(off, ent, 0).tolist() == [(0.0, 4), (4.0, 2), (9.0, 1), (9.0, 3)]
    assert _list(off, ent, 4).tolist() == [(0.0, 0), (4.0, 2), (9.0, 1), (9.0, 3)]
    off, ent = wm.lists(c.x, c.y, c.z, c.flags, 5.0, upper_only=True)
    assert off.tolist() == [0, 4, 4, 4, 4, 4, 4] and _list(off, ent, 0).tolist() == [(0.0, 4), (4.0, 2), (9.0, 1), (9.0, 3)]
    off, ent = wm.lists(c.x, c.y, c.z, None, 5.0, upper_only=True)
    assert [(_list(off, ent, i)["idx"]).tolist() for i in range(6)] == [[4, 2, 1, 3], [4, 3, 2], [4, 3], [4], [], []]
    assert _list(off, ent, 1)["d2"].tolist() == [9.0, 18.0, 25.0]            # from (1, 2, 6): atom 4, atom 3, atom 2


def test_exact_ties_are_listed_and_one_ulp_further_is_not():
    t, m = hc.ties(), hc.ties(True)
    off, ent = wm.lists(t.x, t.y, t.z, t.flags, 13.0)
    assert off.tolist() == [0, 3, 3, 3, 3] and ent.tolist() == [(169.0, 1), (169.0, 2), (169.0, 3)]
    off, ent = wm.lists(m.x, m.y, m.z, m.flags, 13.0)
    assert off[-1] == 0


@pytest.mark.parametrize("name,cutoff", [("cluster", 8.0), ("crowd", 4.5), ("nan_atom", 13.0), ("edge", hc.EDGE_CUTOFF)])
def test_model_properties(name, cutoff):
    c = getattr(hc, name)()
    n = c.n_atoms
    off, ent = wm.lists(c.x, c.y, c.z, None, cutoff)
    assert _sorted_lists(off, ent)
    assert not np.isnan(ent["d2"]).any() and (ent["d2"] >= 0).all()
    # symmetry: (i, j, d2 bits) occurs exactly when (j, i, d2 bits) does
    i = np.repeat(np.arange(n), wm.lengths(off))
    fwd = np.stack([i, ent["idx"].astype(np.int64), ent["d2"].view(np.uint32).astype(np.int64)], -1)
    bwd = fwd[:, [1, 0, 2]]
    assert np.array_equal(fwd[np.lexsort(fwd.T[::-1])], bwd[np.lexsort(bwd.T[::-1])])
    # lengths: up + down of the half-sphere model, with the case's own flags too
    rng = np.random.default_rng(5)
    for flags in (None, rng.integers(0, 4, n).astype(np.uint8)):
        o2, e2 = wm.lists(c.x, c.y, c.z, flags, cutoff)
        up, down = hm.counts(c.x, c.y, c.z, c.dirs, flags, cutoff)
        assert np.array_equal(wm.lengths(o2), (up + down).astype(np.int64))
        # upper_only: the full lists filtered to idx > i
        o3, e3 = wm.lists(c.x, c.y, c.z, flags, cutoff, upper_only=True)
        ii = np.repeat(np.arange(n), wm.lengths(o2))
        keep = e2["idx"] > ii
        assert e3.tobytes() == e2[keep].tobytes()
        assert np.array_equal(wm.lengths(o3), np.bincount(ii[keep], minlength=n))


def test_tree_route_equals_the_pair_route(monkeypatch):
    c = hc.cluster()
    flags = np.where(np.arange(c.n_atoms) % 5 == 0, 3, 1).astype(np.uint8)
    dense = wm.lists(c.x, c.y, c.z, flags, 8.0)
    monkeypatch.setattr(hm, "DENSE", 100)
    tree = wm.lists(c.x, c.y, c.z, flags, 8.0)
    assert np.array_equal(dense[0], tree[0]) and dense[1].tobytes() == tree[1].tobytes()
    n = hc.nan_atom()
    dense_n = wm.lists(n.x, n.y, n.z, None, 6.0, True)
    monkeypatch.setattr(hm, "DENSE", 6000)
    pair_n = wm.lists(n.x, n.y, n.z, None, 6.0, True)
    assert np.array_equal(dense_n[0], pair_n[0]) and dense_n[1].tobytes() == pair_n[1].tobytes()


# ---- the cases -----------------------------------------------------------------------------------------------------------

def _batch(c, cutoff, upper=False):
    return wm.lists_batch(c.x, c.y, c.z, c.so, c.flags, cutoff, upper)


@pytest.mark.parametrize("name,first", [("stage_edges", wc.K_WN_STAGE - 1), ("tile_edges", 5 * wc.SPILL_TILE - 1),
                                        ("double_edges", 2 * wc.K_WN_STAGE - 1)])
def test_edge_batches_have_the_lists_they_are_named_for(name, first):
    c = getattr(wc, name)()
    off, ent = _batch(c, wc.BALL_CUTOFF)
    k = wm.lengths(off)
    centre = np.ones(c.n_atoms, bool) if c.flags is None else (c.flags & 2) != 0
    for s in range(3):
        b, e = int(c.so[s]), int(c.so[s + 1])
        assert e - b == first + 1 + s
        assert np.all(k[b:e][centre[b:e]] == first + s) and not k[b:e][~centre[b:e]].any()
        assert centre[b:e].sum() >= 100
    assert first < wc.K_WN_STAGE or name != "stage_edges"
    assert _sorted_lists(off, ent)


def test_pow2_edges():
    c = wc.pow2_edges()
    k = wm.lengths(_batch(c, wc.BALL_CUTOFF)[0])
    for s, want in enumerate(wc.POW2_LISTS):
        assert np.all(k[int(c.so[s]):int(c.so[s + 1])] == want)
    for p in (2, 4, 64, 128, 512):
        assert {p - 1, p, p + 1} <= set(wc.POW2_LISTS)


def test_coincident():
    c = wc.coincident()
    off, ent = _batch(c, c.info["cutoff"])
    k = wm.lengths(off)
    for s, n in enumerate(c.info["n"]):
        b, e = int(c.so[s]), int(c.so[s + 1])
        same = (c.x[b:e] == np.median(c.x[b:e])) & (c.y[b:e] == np.median(c.y[b:e])) & (c.z[b:e] == np.median(c.z[b:e]))
        assert same.sum() == n
        assert np.all(k[b:e][same] == n - 1 + 6)
        i = b + int(np.flatnonzero(same)[0])
        li = _list(off, ent, i)
        zero = li[li["d2"] == 0.0]
        assert len(zero) == n - 1 and np.all(np.diff(zero["idx"].astype(np.int64)) > 0)     # d2 ties: idx alone orders
        assert np.all(li["d2"][n - 1:] == 1.0)
    assert c.info["n"][0] - 1 >= wc.K_WN_STAGE > c.info["n"][1] + 5


def test_equal_d2():
    c = wc.equal_d2()
    off, ent = _batch(c, c.info["cutoff"])
    li = _list(off, ent, c.info["centre"])
    values, counts = np.unique(li["d2"].view(np.uint32), return_counts=True)
    assert sorted(counts.tolist()) == sorted(c.info["classes"]) and len(li) == sum(c.info["classes"])
    assert values.tolist() == sorted(F(v).view(np.uint32) for v in (12.0, 16.5, 21.875))
    assert _sorted_lists(off, ent)
    all_keys = wm.lengths(off)
    assert all_keys.min() > 0


def test_overlap():
    c = wc.overlap()
    off, ent = _batch(c, 8.0)
    k = wm.lengths(off)
    half = c.n_atoms // 2
    assert np.array_equal(k[:half], k[half:]) and ent[:int(off[half])].tobytes() == ent[int(off[half]):].tobytes()
    assert (ent["d2"] > 0).all() and ent["idx"].max() < half
    o1, e1 = wm.lists(c.x, c.y, c.z, None, 8.0)                      # as one structure every atom meets its twin at d2 = 0
    assert np.all(wm.lengths(o1) == 2 * k + 1)


def test_imported_batches():
    for name in ("interleaved", "tiny_batch"):
        c = getattr(hc, name)()
        off, ent = _batch(c, 8.0)
        up, down = hm.counts_batch(c.x, c.y, c.z, c.so, None, c.flags, 8.0)
        assert np.array_equal(wm.lengths(off), (up + down).astype(np.int64))
        sizes = np.diff(c.so.astype(np.int64))
        owner = np.repeat(np.repeat(np.arange(len(sizes)), sizes), wm.lengths(off))
        assert np.all(ent["idx"] < sizes[owner])


# ---- the header and the bindings -------------------------------------------------------------------------------------------

def test_symbols_are_declared_and_bound():
    import ctypes as C
    from rustsasa_amd import _capi
    header = open(os.path.join(ROOT, "include", "rustsasa_amd.h")).read()
    one, many = _capi.SYMBOLS["rsasa_atoms_within"], _capi.SYMBOLS["rsasa_atoms_within_batch"]
    assert "int rsasa_atoms_within(" in header and "int rsasa_atoms_within_batch(" in header
    assert one[0] is C.c_int and len(one[1]) == 14 and one[1][6] is C.c_size_t and one[1][7] is C.c_float
    assert one[1][9] is C.c_float and one[1][10] is C.c_int and one[1][13] is C.c_size_t
    assert many[0] is C.c_int and len(many[1]) == 15 and many[1][7] is C.c_size_t and many[1][8] is C.c_float
    assert many[1][10] is C.c_float and many[1][11] is C.c_int and many[1][14] is C.c_size_t
    assert "#define RSASA_WITHIN_PARTNER 1" in header and "#define RSASA_WITHIN_CENTRE 2" in header
    assert "#define RSASA_ABI_VERSION 4" in header
    assert _capi.WITHIN_PARTNER == 1 and _capi.WITHIN_CENTRE == 2
    assert _capi.WITHIN_DTYPE == wm.WITHIN_DTYPE and _capi.WITHIN_DTYPE.itemsize == 8
    lib = _capi.load()
    assert lib.rsasa_abi_version() == 4 and hasattr(lib, "rsasa_atoms_within") and hasattr(lib, "rsasa_atoms_within_batch")


def test_rsasa_within_t_is_eight_bytes(tmp_path):
    src = tmp_path / "within_size.c"
    src.write_text('#include <stddef.h>\n#include "rustsasa_amd.h"\n'
                   "_Static_assert(sizeof(rsasa_within_t) == 8, \"size\");\n"
                   "_Static_assert(offsetof(rsasa_within_t, d2) == 0 && offsetof(rsasa_within_t, idx) == 4, \"layout\");\n"
                   "int main(void) { return 0; }\n")
    p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]


class _NoCalls:
    """In place of the loaded library: any C call is a failure."""
    def __getattr__(self, name):
        raise AssertionError(f"C call {name} before the arguments were checked")


def test_python_argument_errors_raise_before_any_c_call():
    import rustsasa_amd
    ctx = rustsasa_amd.Context.__new__(rustsasa_amd.Context)
    ctx._lib, ctx._h = _NoCalls(), None
    c = hc.hand()
    so = np.array([0, 2, 6], np.uint32)
    for call, so_args in ((ctx.atoms_within, ()), (ctx.atoms_within_batch, (so,))):
        args = (c.x, c.y, c.z, c.r, None) + so_args
        for bad in (dict(flags=c.flags[:3]), dict(flags=c.flags.astype(np.float32)), dict(flags=np.full(6, 256)),
                    dict(flags=np.full(6, -1)), dict(flags=c.flags.reshape(2, 3)),
                    dict(cutoff=float("nan")), dict(cutoff=-1.0), dict(cutoff=float("inf")), dict(cutoff=-1e-30)):
            with pytest.raises(ValueError):
                call(*args, **bad)
        with pytest.raises(ValueError):
            call(c.x, c.y[:4], c.z, c.r, None, *so_args)
        with pytest.raises(AssertionError, match="C call rsasa_atoms_within"):      # good arguments do reach the call
            call(*args, flags=c.flags.astype(np.int64), cutoff=5.0)
    with pytest.raises(ValueError):
        ctx.atoms_within_batch(c.x, c.y, c.z, c.r, None, np.array([0, 2, 5], np.uint32))


# ---- the numpy helpers -------------------------------------------------------------------------------------------------------

def _helper_batch():
    """Structures of 40, 0, 25 and 1 atoms (an empty one in the middle) with residue-like labels, disjoint by structure."""
    rng = np.random.default_rng(71)
    sizes = [40, 0, 25, 1]
    so = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    xyz = np.round(rng.uniform(0.0, 12.0, (sum(sizes), 3)), 3).astype(F)
    labels = np.concatenate([np.arange(n) // 4 + 100 * s for s, n in enumerate(sizes)]).astype(np.int32)
    off, ent = wm.lists_batch(xyz[:, 0], xyz[:, 1], xyz[:, 2], so, None, 6.0)
    return so, labels, off, ent


def test_edge_index_against_a_direct_loop():
    import rustsasa_amd
    so, labels, off, ent = _helper_batch()
    want = []
    for s in range(len(so) - 1):
        for i in range(int(so[s]), int(so[s + 1])):
            for e in _list(off, ent, i):
                want.append((i, int(so[s]) + int(e["idx"])))
    got = rustsasa_amd.edge_index(off, ent, so)
    assert got.dtype == np.int64 and got.shape == (2, len(ent)) and got.T.tolist() == [list(w) for w in want]
    single = wm.lists(np.arange(5, dtype=F), np.zeros(5, F), np.zeros(5, F), None, 1.0)
    assert rustsasa_amd.edge_index(*single).T.tolist() == [[0, 1], [1, 0], [1, 2], [2, 1], [2, 3], [3, 2], [3, 4], [4, 3]]
    empty = rustsasa_amd.edge_index(np.zeros(1, np.uint64), np.zeros(0, wm.WITHIN_DTYPE))
    assert empty.shape == (2, 0)
    with pytest.raises(ValueError):
        rustsasa_amd.edge_index(off, ent[:-1], so)
    with pytest.raises(ValueError):
        rustsasa_amd.edge_index(off, ent, so[:-1])


def test_closest_pairs_against_a_direct_loop():
    import rustsasa_amd
    so, labels, off, ent = _helper_batch()
    best = {}
    for s in range(len(so) - 1):
        for i in range(int(so[s]), int(so[s + 1])):
            for e in _list(off, ent, i):
                a, b = int(labels[i]), int(labels[int(so[s]) + int(e["idx"])])
                if a != b:
                    best[(a, b)] = min(best.get((a, b), np.inf), float(e["d2"]))
    la, lb, dist = rustsasa_amd.closest_pairs(off, ent, labels, so)
    assert la.dtype == lb.dtype == np.int64 and dist.dtype == F
    assert list(zip(la.tolist(), lb.tolist())) == sorted(best)
    assert dist.tobytes() == np.sqrt(np.array([best[k] for k in sorted(best)], F)).tobytes()
    assert len(best) > 50 and all((b, a) in best for a, b in best)
    with pytest.raises(ValueError):
        rustsasa_amd.closest_pairs(off, ent, labels[:-1], so)
    with pytest.raises(ValueError):
        rustsasa_amd.closest_pairs(off, ent, labels.astype(F), so)
