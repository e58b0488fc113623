"""The k nearest atoms without a GPU: the model (nearest_model.py: the within-lists cut at k) against an independent
argsort, a float64 brute force and hand lists; k_nearest's sweep emulated (its stop rule by counting, its staging with the
compaction trigger) against the model; every case of nearest_cases.py pinned to what it is named for, with the switch
that shows it bites; the header, the bindings, the argument rules and the numpy helpers."""
import functools
import os
import subprocess

import numpy as np
import pytest

import hse_cases as hc
import nearest_cases as nc
import nearest_model as nm
import sweep_model as sm
import within_cases as wc
import within_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BAND = 1e-4
KS = (1, 16, 30, 64, 256)


def _list(offsets, entries, i):
    return entries[int(offsets[i]):int(offsets[i + 1])]


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


@functools.lru_cache(maxsize=None)
def _1jcd():
    import structio as sio
    atoms = [a for a in sio.read_structure(sio.data_path("1jcd.pdb")) if not a.hetero]
    x, y, z, r, _ = sio.soa_vdw(atoms)
    return hc.Case("1jcd", *(np.ascontiguousarray(a, F) for a in (x, y, z, r)), np.array([0, len(x)], np.uint32))


def _case(name):
    return _1jcd() if name == "1jcd" else nc.case(name)


# ---- the model -------------------------------------------------------------------------------------------------------------

def test_truncate_cuts_every_list():
    off = np.array([0, 3, 3, 4, 9], np.uint64)
    ent = np.zeros(9, wm.WITHIN_DTYPE)
    ent["idx"] = np.arange(9)
    o, e = nm.truncate(off, ent, 2)
    assert o.tolist() == [0, 2, 2, 3, 5] and e["idx"].tolist() == [0, 1, 3, 4, 5]
    o, e = nm.truncate(off, ent, 5)
    assert o.tolist() == off.tolist() and e.tobytes() == ent.tobytes()


@pytest.mark.parametrize("name,k,cutoff", [("cluster", 30, None), ("cluster", 64, 6.0), ("crowd", 256, None), ("crowd", 1, 13.0),
                                           ("nan_atom", 16, None), ("equal_d2", 49, None), ("interleaved", 30, 4.5),
                                           ("tiny_batch", 16, None), ("coincident", 16, None), ("knn_stage", 256, None)])
def test_model_equals_an_independent_argsort(name, k, cutoff):
    c = _case(name)
    rng = np.random.default_rng(7)
    for flags in (c.flags, rng.integers(0, 4, c.n_atoms).astype(np.uint8)):
        a = nm.lists_batch(c.x, c.y, c.z, c.so, flags, k, cutoff)
        b = nm.lists_batch(c.x, c.y, c.z, c.so, flags, k, cutoff, by_sort=True)
        assert _same(a, b)
        assert wm.lengths(a[0]).max() <= k


def test_independent_route_on_a_structure_of_65536_atoms():
    """The route the GPU test of the 65 536-atom structure compares with (rows too wide for a full argsort: the k smallest
    keys are selected first), against the within-lists at a cutoff that leaves every centre k partners or more."""
    c = hc.tail_batch()
    big = hc.part(c, len(c.so) - 2)
    a = nm.lists_by_sort(big.x, big.y, big.z, big.flags, 30)
    b = nm.lists(big.x, big.y, big.z, big.flags, 30, cutoff=13.0)
    assert np.all(wm.lengths(b[0])[c.info["centres"]] == 30) and _same(a, b)


SEEDS64 = (101, 102, 107, 111)   # (of 100 .. 111, those whose float64 gaps stay above BAND)


@pytest.mark.parametrize("seed", SEEDS64)
def test_model_equals_a_float64_brute_force(seed):
    """60 uniform atoms in a 20 A box; k = 1, 5, 16, 59 and 80 (more than there are).  The smallest relative gap between
    the k-th and the (k + 1)-th distance over these seeds and k is 2.37e-4 (seed 101, k = 16), above the band of 1e-4
    inside which float32 could choose the other atom."""
    xyz = np.random.default_rng(seed).uniform(0.0, 20.0, (60, 3)).astype(F)
    x, y, z = (xyz[:, k].copy() for k in range(3))
    rng = np.random.default_rng(seed + 2)
    for flags in (None, rng.integers(0, 4, len(x)).astype(np.uint8)):
        for k in (1, 5, 16, 59, 80):
            want, dist, band = nm.brute64(x, y, z, flags, k)
            assert band > BAND, (k, band)
            off, ent = nm.lists(x, y, z, flags, k)
            for i in range(len(x)):
                li = _list(off, ent, i)
                assert li["idx"].tolist() == want[i], (k, i)
                assert np.allclose(np.sqrt(li["d2"].astype(np.float64)), dist[i, li["idx"]], rtol=1e-6)


def test_hand_lists():
    """hse_cases.hand(): centres 0 and 4 (coincident).  From (1, 2, 3): atom 4 at d2 0, atom 2 at 4, atoms 1 and 3 at 9
    (the smaller idx first), atom 5 at 49."""
    c = hc.hand()
    full = [(0.0, 4), (4.0, 2), (9.0, 1), (9.0, 3), (49.0, 5)]
    for k in (1, 2, 3, 4, 5, 6, 256):
        off, ent = nm.lists(c.x, c.y, c.z, c.flags, k)
        n = min(k, 5)
        assert off.tolist() == [0, n, n, n, n, 2 * n, 2 * n]
        assert _list(off, ent, 0).tolist() == full[:n]
        assert _list(off, ent, 4).tolist() == [(0.0, 0)] + full[1:n]
    off, ent = nm.lists(c.x, c.y, c.z, c.flags, 3, cutoff=5.0)
    assert _list(off, ent, 0).tolist() == full[:3]                     # the tie at 9 is cut: atom 1 stays, atom 3 goes
    off, ent = nm.lists(c.x, c.y, c.z, c.flags, 256, cutoff=5.0)
    assert _list(off, ent, 0).tolist() == full[:4]
    t = hc.ties()
    for k in (1, 2, 3, 4):
        off, ent = nm.lists(t.x, t.y, t.z, t.flags, k, cutoff=13.0)
        assert ent.tolist() == [(169.0, 1), (169.0, 2), (169.0, 3)][:k] and off.tolist() == [0] + [min(k, 3)] * 4


def test_nan_atom_and_short_structures():
    c = hc.nan_atom()
    a = c.info["atom"]
    off, ent = nm.lists(c.x, c.y, c.z, None, 30)
    assert off[a] == off[a + 1] and not (ent["idx"] == a).any() and not np.isnan(ent["d2"]).any()
    assert np.all(np.delete(wm.lengths(off), a) == 30)
    t = hc.tiny_batch()
    off, ent = nm.lists_batch(t.x, t.y, t.z, t.so, None, 16)
    sizes = np.diff(t.so.astype(np.int64))
    assert np.array_equal(wm.lengths(off), np.minimum(np.repeat(sizes, sizes) - 1, 16))   # lists of n - 1 where n - 1 < k


# ---- the emulated sweep ------------------------------------------------------------------------------------------------------

_WITHIN = {}


def _model(c, k, cutoff):
    """nm.lists of a one-structure case; the within-lists behind it are computed once per (case, cutoff)."""
    key = (c.name, cutoff)
    if key not in _WITHIN:
        _WITHIN[key] = wm.lists(c.x, c.y, c.z, c.flags, np.inf if cutoff is None else cutoff)
    return nm.truncate(*_WITHIN[key], k)


def _sweep_equals_model(c, k, cutoff, sample, **kw):
    want = _model(c, k, cutoff)
    sw = nm.sweep(c.x, c.y, c.z, c.r, c.probe, c.flags, k, cutoff, sample=sample, **kw)
    for n, i in enumerate(sample):
        assert sw.lists[n].tobytes() == _list(*want, i).tobytes(), (c.name, k, cutoff, int(i))
    return sw


@pytest.mark.parametrize("name", ["cluster", "crowd", "1jcd", "coincident", "equal_d2", "odd_radius", "nan_atom"])
def test_emulated_sweep_equals_the_model(name):
    c = _case(name)
    if len(c.so) > 2:
        c = hc.part(c, 0)
    rng = np.random.default_rng(11)
    sample = np.sort(rng.permutation(c.n_atoms)[:40])
    if name == "nan_atom":
        sample[0] = c.info["atom"]
    margins = sm.margins_hold(c.x, c.y, c.z, c.r, c.probe)
    assert margins == (name not in ("odd_radius", "nan_atom"))
    most = 0
    for k in KS:
        for cutoff in (None, 8.0):
            sw = _sweep_equals_model(c, k, cutoff, sample)
            most = max(most, max(sw.most_held))
            if not margins:
                assert not any(sw.by_rule)                                   # the whole grid
            elif name in ("cluster", "crowd", "1jcd") and cutoff is None:
                assert all(w == "kth" or s == 0 for w, s in zip(sw.by_rule, sw.stop)) or c.n_atoms <= k
                if k <= 64:
                    assert max(sw.stop) <= 5
            if name == "coincident":
                assert all(comp for comp in sw.compactions)                  # 1 100 atoms in one cell: always compacted
    if name == "odd_radius":
        assert most > nm.TRIGGER                                             # one cell of 2 000 atoms


def test_sweep_stops_by_the_cutoff_or_by_what_it_holds():
    c = hc.cluster()
    mid = int(np.argmin((c.x - 12.0) ** 2 + (c.y + 7.0) ** 2 + (c.z - 31.0) ** 2))
    by_kth = _sweep_equals_model(c, 16, 13.0, [mid])
    by_cut = _sweep_equals_model(c, 256, 4.0, [mid])
    assert by_kth.by_rule == ["kth"] and by_cut.by_rule == ["cutoff"] and by_kth.stop[0] < 5


# ---- the cases -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", nc.EDGE_KS)
def test_knn_edge(k):
    c = nc.knn_edge(k)
    g = sm.grid(c.x, c.y, c.z, c.r, c.probe)
    assert g.h == F(nc.EDGE_H) and sm.margins_hold(c.x, c.y, c.z, c.r, c.probe)
    want = nm.lists(c.x, c.y, c.z, c.flags, k)
    assert np.flatnonzero(wm.lengths(want[0])).tolist() == [gr["centre"] for gr in c.info["groups"]]
    assert [(gr["axis"], gr["sign"]) for gr in c.info["groups"]] == list(nc.EDGE_DIRECTIONS)
    for gr in c.info["groups"]:
        i, axis, sign = gr["centre"], gr["axis"], gr["sign"]
        unit = np.zeros(3, np.int64)
        unit[axis] = sign
        li = _list(*want, i)
        assert len(li) == k and li["idx"][-1] == gr["true_kth"] and gr["diagonal"] not in li["idx"]
        assert np.all(g.cells[li["idx"][:-1]] == g.cells[i])                             # k - 1 partners in its own cell
        assert np.array_equal(g.cells[gr["true_kth"]] - g.cells[i], 2 * unit)             # the k-th in shell 2, on the axis
        d = g.cells[gr["diagonal"]] - g.cells[i]
        assert d[axis] == -sign and np.abs(d).max() == 1 and np.abs(d).sum() == 2         # the diagonal one in shell 1
        h = float(g.h)
        assert abs(np.sqrt(li["d2"][-1]) / h - 1.02) < 1e-3
        assert abs(np.sqrt(wm.d2_of(c.x[i], c.y[i], c.z[i], *(a[gr["diagonal"]] for a in (c.x, c.y, c.z)))) / h - 1.4142) < 1e-3
        if k > 1:
            assert np.sqrt(li["d2"][-2]) / h < 0.95
    centres = [gr["centre"] for gr in c.info["groups"]]
    right = _sweep_equals_model(c, k, None, centres)
    assert right.stop == [2] * 6 and right.by_rule == ["kth"] * 6                         # found in the last shell swept
    relaxed = nm.sweep(c.x, c.y, c.z, c.r, c.probe, c.flags, k, sample=centres, lim_shift=0.5)
    assert relaxed.stop == [1] * 6
    for n, gr in enumerate(c.info["groups"]):                                             # the case bites
        assert relaxed.lists[n].tobytes() != _list(*want, gr["centre"]).tobytes()
        assert relaxed.lists[n]["idx"][-1] == gr["diagonal"]


@pytest.mark.parametrize("k", nc.STAGE_KS)
def test_knn_stage(k):
    c = nc.knn_stage()
    T = nm.TRIGGER
    assert T == 961 and nc.STAGE_SIZES[:3] == (T, T + 1, T + 2) and nc.STAGE_SIZES[3] > nm.K_NN_STAGE + nm.WAVE
    seen = []
    for s in range(4):
        p = hc.part(c, s)
        centres = np.flatnonzero(p.flags & 2)
        assert len(centres) >= 200
        sw = _sweep_equals_model(p, k, None, centres)
        bad = nm.sweep(p.x, p.y, p.z, p.r, p.probe, p.flags, k, sample=centres, keep_unsorted=True)
        want = _model(p, k, None)
        wrong = [bad.lists[n].tobytes() != _list(*want, i).tobytes() for n, i in enumerate(centres)]
        compacted = [bool(comp) for comp in sw.compactions]
        assert [w <= cp for w, cp in zip(wrong, compacted)] == [True] * len(centres)      # only a compaction can go wrong
        seen.append((max(sw.most_held), sorted({comp[0] for comp in sw.compactions if comp}), sum(wrong)))
    if k == 256:                                                                         # the sweep sees the whole ball
        assert seen[0][:2] == (T - 1, [])          # one short of the trigger: never compacted
        assert seen[1][:2] == (T, [])              # at it, with no batch to follow: never compacted
        assert seen[2][:2] == (T + 1, [T])         # one above: compacted with exactly T keys staged
        assert seen[2][2] >= 10 and seen[3][2] >= 200                                    # the case bites
        assert min(seen[3][1]) > T and max(seen[3][1]) <= nm.K_NN_STAGE
    else:                                                                                # k = 1 stops after shell 1
        assert seen[0][1] == [] and seen[3][1] and seen[3][2] >= 100


def test_tie_classes_are_cut_by_idx():
    c = wc.equal_d2()
    i = c.info["centre"]
    full = _list(*wm.lists(c.x, c.y, c.z, None, np.inf), i)
    assert len(full) == 80 and [int((full["d2"] == v).sum()) for v in (12.0, 16.5, 21.875)] == [8, 24, 48]
    assert nc.TIE_KS == (1, 47, 48, 49, 72, 73, 80, 81)
    # the classes in order of d2 hold 8, 24 and 48 keys: the cut falls inside a class, except at 80 and 81 (the list's end)
    for k in nc.TIE_KS:
        li = _list(*nm.lists(c.x, c.y, c.z, None, k), i)
        assert li.tobytes() == full[:k].tobytes() and len(li) == min(k, 80)
        last = li["d2"][-1]
        kept, cls = li["idx"][li["d2"] == last], full["idx"][full["d2"] == last]
        assert kept.tolist() == np.sort(cls)[:len(kept)].tolist()                         # the smaller idx are kept
        if k < 80:
            assert 0 < len(kept) < len(cls) or k in (8, 32)
        _sweep_equals_model(c, k, None, np.arange(c.n_atoms))


# ---- the header and the bindings -----------------------------------------------------------------------------------------------

def test_symbols_are_declared_and_bound():
    import ctypes as C
    import rustsasa_amd
    from rustsasa_amd import _capi
    header = open(os.path.join(ROOT, "include", "rustsasa_amd.h")).read()
    one, many = _capi.SYMBOLS["rsasa_nearest_atoms"], _capi.SYMBOLS["rsasa_nearest_atoms_batch"]
    assert "int rsasa_nearest_atoms(" in header and "int rsasa_nearest_atoms_batch(" in header
    assert one[0] is C.c_int and len(one[1]) == 14 and one[1][6] is C.c_size_t and one[1][7] is C.c_float
    assert one[1][9] is C.c_uint32 and one[1][10] is C.c_float and one[1][13] is C.c_size_t
    assert many[0] is C.c_int and len(many[1]) == 15 and many[1][7] is C.c_size_t and many[1][8] is C.c_float
    assert many[1][10] is C.c_uint32 and many[1][11] is C.c_float and many[1][14] is C.c_size_t
    assert "#define RSASA_NEAREST_MAX_K 256" in header and "#define RSASA_ABI_VERSION 4" in header
    assert _capi.NEAREST_MAX_K == rustsasa_amd.NEAREST_MAX_K == nm.MAX_K == 256
    lib = _capi.load()
    assert lib.rsasa_abi_version() == 4 and hasattr(lib, "rsasa_nearest_atoms") and hasattr(lib, "rsasa_nearest_atoms_batch")


def test_header_declares_the_documented_signatures(tmp_path):
    src = tmp_path / "nearest_decl.c"
    src.write_text('#include "rustsasa_amd.h"\n'
                   "int (*one)(rsasa_context_t *, const float *, const float *, const float *, const float *, const uint64_t *,\n"
                   "           size_t, float, const uint8_t *, uint32_t, float, uint64_t *, rsasa_within_t *, size_t) = rsasa_nearest_atoms;\n"
                   "int (*many)(rsasa_context_t *, const float *, const float *, const float *, const float *, const uint64_t *,\n"
                   "            const uint32_t *, size_t, float, const uint8_t *, uint32_t, float, uint64_t *, rsasa_within_t *,\n"
                   "            size_t) = rsasa_nearest_atoms_batch;\n"
                   "_Static_assert(RSASA_NEAREST_MAX_K == 256, \"max k\");\n"
                   "int main(void) { return 0; }\n")
    p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]


def test_argument_rules_in_c(tmp_path):
    exe = str(tmp_path / "nearest_checks_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "rustsasa_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "nearest_checks_test.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "nearest checks ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-2000:])


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
    for call, so_args in ((ctx.nearest_atoms, ()), (ctx.nearest_atoms_batch, (so,))):
        args = (c.x, c.y, c.z, c.r, None) + so_args
        for bad in (dict(flags=c.flags[:3]), dict(flags=c.flags.astype(np.float32)), dict(flags=np.full(6, 256)),
                    dict(flags=np.full(6, -1)), dict(flags=c.flags.reshape(2, 3)),
                    dict(cutoff=float("nan")), dict(cutoff=-1.0), dict(cutoff=-float("inf")), dict(cutoff=-1e-30),
                    dict(k=0), dict(k=257), dict(k=-1), dict(k=2.5), dict(k=16.0), dict(k=True), dict(k=1 << 32)):
            with pytest.raises(ValueError):
                call(*args, **bad)
        with pytest.raises(ValueError):
            call(c.x, c.y[:4], c.z, c.r, None, *so_args)
        for good in (dict(k=1), dict(k=256, cutoff=None), dict(k=np.int64(30), cutoff=float("inf")), dict(cutoff=0.0),
                     dict(cutoff=-0.0), dict(flags=c.flags.astype(np.int64), cutoff=5.0)):
            with pytest.raises(AssertionError, match="C call rsasa_nearest_atoms"):      # good arguments do reach the call
                call(*args, **good)
    with pytest.raises(ValueError):
        ctx.nearest_atoms_batch(c.x, c.y, c.z, c.r, None, np.array([0, 2, 5], np.uint32))


# ---- the numpy helpers -----------------------------------------------------------------------------------------------------------

def _helper_batch(k):
    """Structures of 40, 0, 25, 1 and 3 atoms (an empty one in the middle, two with fewer than k + 1 atoms)."""
    rng = np.random.default_rng(72)
    sizes = [40, 0, 25, 1, 3]
    so = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    xyz = np.round(rng.uniform(0.0, 12.0, (sum(sizes), 3)), 3).astype(F)
    flags = np.where(np.arange(sum(sizes)) % 5 == 2, 1, 3).astype(np.uint8)
    off, ent = nm.lists_batch(xyz[:, 0], xyz[:, 1], xyz[:, 2], so, flags, k)
    return so, off, ent


def test_nearest_table_and_edge_index_against_direct_loops():
    import rustsasa_amd
    k = 6
    so, off, ent = _helper_batch(k)
    n = len(off) - 1
    idx, d2 = rustsasa_amd.nearest_table(off, ent, k, so)
    assert idx.dtype == np.int64 and d2.dtype == F and idx.shape == d2.shape == (n, k)
    edges = []
    for s in range(len(so) - 1):
        for i in range(int(so[s]), int(so[s + 1])):
            li = _list(off, ent, i)
            for col in range(k):
                if col < len(li):
                    assert idx[i, col] == int(so[s]) + int(li["idx"][col]) and d2[i, col] == li["d2"][col]
                    edges.append([i, int(so[s]) + int(li["idx"][col])])
                else:
                    assert idx[i, col] == -1 and d2[i, col] == np.inf
    assert (idx == -1).sum() > 0 and rustsasa_amd.edge_index(off, ent, so).T.tolist() == edges
    wide_idx, wide_d2 = rustsasa_amd.nearest_table(off, ent, k + 2, so)
    assert np.array_equal(wide_idx[:, :k], idx) and (wide_idx[:, k:] == -1).all() and np.isinf(wide_d2[:, k:]).all()
    single = nm.lists(np.arange(5, dtype=F), np.zeros(5, F), np.zeros(5, F), None, 2)
    assert rustsasa_amd.nearest_table(*single, 2)[0].tolist() == [[1, 2], [0, 2], [1, 3], [2, 4], [3, 2]]
    empty = rustsasa_amd.nearest_table(np.zeros(1, np.uint64), np.zeros(0, wm.WITHIN_DTYPE), 4)
    assert empty[0].shape == empty[1].shape == (0, 4)
    for bad in (lambda: rustsasa_amd.nearest_table(off, ent, k - 1, so), lambda: rustsasa_amd.nearest_table(off, ent, 0, so),
                lambda: rustsasa_amd.nearest_table(off, ent[:-1], k, so), lambda: rustsasa_amd.nearest_table(off, ent, k, so[:-1])):
        with pytest.raises(ValueError):
            bad()
