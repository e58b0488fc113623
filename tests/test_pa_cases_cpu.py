"""The inputs of test_gpu_pa_edges.py (pa_cases.py) pinned, on the CPU, to the limits of k_occlusion_fast and
k_occlusion_v3 they are named for - by the routing model (pa_model.py) - and the model pinned to the oracle and to the
launch's arithmetic.

Two admission conditions hold for every case.  (1) Row culling uses the raw v_sqrt_f32 and heuristic factors that the
model does not imitate to the bit: T and the swept cells of every atom must be the same with every cull width widened
and narrowed by 1e-3 (relative, plus 1e-3 cells).  (2) Order inside a cell is arrival order on the device and not
defined: whatever a GPU run asserts or a case is named for must be the same with the atoms of a cell in rising, in
falling and in a seeded random input order.  A case that fails either is a bug in the generator, never skipped."""
import numpy as np
import pytest

import pa_cases as pc
import pa_model as pm
import tie_cases as ti

F = np.float32
CASES = pc.all_cases()
IDS = [c.name for c in CASES]
FAST_WAVES = [c for v in pc.fast_wave_batches().values() for c in v] + pc.block_count_cases()
V3_WAVES = [c for v in pc.v3_wave_batches().values() for c in v]
BATCHES = FAST_WAVES + V3_WAVES
_ORACLE = {}


def _oracle(st, c):
    key = (id(st), c.key)
    if key not in _ORACLE:
        _ORACLE[key] = (st, ti.oracle_counts(st, c.probe, c.n_points, c.W))
    return _ORACLE[key][1]


def _models(c, _cache={}):
    if c.name not in _cache:
        _cache[c.name] = tuple(c.model(order=o, seed=7) for o in ("asc", "desc", "random"))
    return _cache[c.name]


def _same_sweep(a, b):
    """T and the set of swept cells - the rows kept and [x0, x1] of each, empty cells included - of every atom are the
    same.  (The generator keeps atoms of the largest radius off the grid's lowest faces, where u = 0 would put the row
    two cells up exactly on the margin: build()'s anchor and line()'s corner atom have radius 1.0, and no structure has
    one atom only.)"""
    return np.array_equal(a.T, b.T) and np.array_equal(a.x0, b.x0) and np.array_equal(a.x1, b.x1) and \
        np.array_equal(a.run_len, b.run_len)


def _detail(c, m):
    return m.v3(c.watch) if c.kernel == "v3" else m.fast(c.watch)


def test_every_family_has_its_cases():
    for fam, least in pc.MINIMUM.items():
        n = sum(c.family == fam for c in CASES)
        assert n >= least, (fam, n, least)
    assert len(set(IDS)) == len(IDS)
    assert len(FAST_WAVES) == 7 * 9 + 5 and len(V3_WAVES) == 4 * 3
    assert len(pc.reach_cases()) == 12 * 3 * 3 * 2


def test_print_the_case_table():
    for c in CASES:
        m = _models(c)[0]
        d = _detail(c, m)
        print(f"{c.name}: atoms {c.n} T {d['T']} K {d['K']} flushes {d.get('flushes', '-')} deferred {m.n_deferred}")


@pytest.mark.parametrize("c", CASES + BATCHES, ids=[c.name for c in CASES + BATCHES])
def test_cull_widths_do_not_decide(c):
    m = _models(c)[0] if c in CASES else c.model()
    for widen in (1e-3, -1e-3):
        w = c.model(widen=widen)
        bad = np.flatnonzero((w.x0 != m.x0).any(1) | (w.x1 != m.x1).any(1) | (w.T != m.T))
        assert _same_sweep(w, m), (widen, bad[:5].tolist())


@pytest.mark.parametrize("c", CASES + BATCHES, ids=[c.name for c in CASES + BATCHES])
def test_order_inside_a_cell_does_not_matter(c):
    ms = _models(c) if c in CASES else tuple(c.model(order=o, seed=7) for o in ("asc", "desc", "random"))
    a = ms[0]
    for m in ms[1:]:
        for name in ("T", "A", "K", "deferred"):
            assert np.array_equal(getattr(a, name), getattr(m, name)), name
        assert a.n_deferred == m.n_deferred
        if c.n_points <= 128 or c.kernel == "v3":
            assert _detail(c, a) == _detail(c, m)
        assert a.runs(c.watch) == m.runs(c.watch)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_case_sits_on_its_edge(c):
    m = _models(c)[0]
    w, e = c.watch, c.expect
    d = _detail(c, m)
    for k in ("T", "K", "A", "nA", "nA4", "nB", "G", "deferred", "rem_shift", "rem_groups"):
        if e.get(k) is not None:
            assert d[k] == e[k], (k, d[k], e[k])
    runs = m.runs(w)
    if c.kernel == "fast":
        assert m.fast_kernel and c.forced is None
        assert d["deferred"] == (d["T"] > 256 or d["K"] > 144)
        assert d["HALF1"] == (ti.n_fused(c.n_points, c.W) <= 96) and d["n_rem"] <= 4
        assert d["trips"] == [(s, s + 64 < d["T"]) for s in range(0, d["T"], 128)]
        if "runs" in e:
            assert len(runs) == e["runs"]
        if "run_at" in e:
            own = [f for r, f, n in runs if r == 12]
            assert own == [e["run_at"]] and d["T"] <= 256
        if c.family in ("swept", "list", "near", "points", "survivors") and runs:
            rows = [r for r, _, _ in runs]
            # (empty runs between non-empty ones, except where the case is the count of runs itself)
            assert c.name in ("swept_T1", "swept_rows21", "swept_rows23") or max(rows) - min(rows) + 1 > len(rows)
        if c.name == "swept_rows23":
            # both rows two cells up in y and two off in z, neither of the opposite ones: 23 is the most (pa_cases.py)
            assert {r for r, _, _ in runs} == set(range(25)) - {pc.row_of((0, -2, -2)), pc.row_of((0, -2, 2))}
        if c.family == "list" and not d["deferred"]:
            assert d["pad"] == (d["K"], d["K"] + 16) and d["pad"][1] <= pm.FAST_CAP + pm.CAND_PAD
            assert d["passes"] == -(-d["K"] // 64)
        if c.name.startswith("list_150"):
            assert int(m.A[w]) == 150 and sum(int(c.ids[q] == c.ids[w]) for q in range(c.n)) == (7 if "_ids" in c.name else 1)
        if c.name.startswith("near_nA64"):
            assert d["nA"] == d["K"] == 64 and d["nB"] == 0
        if c.name.startswith("near_tiles"):
            assert d["form"] == "tiles" and d["nA"] % 4 == 0
            # the last trip's two steps read up to slot nA + (steps rounded up to 2) G - 1: behind K, inside the padding
            last = d["nA4"] + (-(-d["steps"] // 2) * 2) * d["G"] - 1
            assert d["K"] <= last < d["pad"][1]
        if c.family == "survivors" and not e.get("second"):
            assert c.W == 1 and d["nA"] == 0 and d["S"] == c.n_points and d["nB"] == 20
            assert d["form"] == ("broadcast" if c.n_points > 64 else "tiles")
            assert d["G"] == {8: 8, 9: 4, 16: 4, 17: 2, 32: 2, 33: 1, 64: 1, 65: None}[c.n_points]
        if e.get("second"):
            # survivors in the second chunk on the compact path, with HALF1 (65 fused points) and without (97)
            assert d["form"] == "tiles" and d["S_second"] > 0 and d["HALF1"] == (c.n_points == 65)
        if c.name.startswith("buried"):
            assert _oracle(c.structures[0], c)[1][w] == 0
        if c.name.startswith("lonely"):
            assert d["K"] == 0 and _oracle(c.structures[0], c)[1][w] == c.n_points
        # (nothing but the target and the atoms the model names defers)
        if c.family in ("swept", "list") and c.name not in ("list_150_noids",):
            assert m.n_deferred == int(d["deferred"]), (m.n_deferred, np.flatnonzero(m.deferred)[:5])
    else:
        assert not m.fast_kernel and m.n_deferred == 0
        assert (c.forced == "3") == (c.n_points <= 128 and d["n_rem"] <= 4)
        fl = d["flushes"]
        assert sum(fl) == d["A"] and all(n <= pm.LIST_CAP for n in fl) and all(n > pm.LIST_FLUSH for n in fl[:-1])
        assert d["single_flush"] == (len(fl) == 1) and d["sweeps"] == (1 if len(fl) == 1 else d["n_groups"])
        assert d["n_groups"] == -(-(-(-c.n_points // 64)) // 2)
        if "flushes" in e:
            assert fl == e["flushes"]
        if "n_flushes" in e:
            assert len(fl) == e["n_flushes"]
        if e.get("mid_window"):
            first = d["flush_at"][0]
            assert first % 256 and any(first <= f < (first // 256 + 1) * 256 for _, f, _ in runs)
        if c.name == "flush_192_exactly":
            # the 192 sit in runs 6 - 11, the target's own run starts at flat position 192: it is in none of the first three steps
            assert [f for r, f, n in runs if r == 12] == [192] and fl[0] == pm.LIST_CAP
        if "windows" in e:
            assert len(d["windows"]) == e["windows"]
        if "run_at" in e:
            assert e["run_at"] in [f for _, f, _ in runs]
        if e.get("straddle"):
            assert d["windows"][1][2] is not None
        if e.get("empty_window"):
            assert any(not starts and strad is not None for _, starts, strad in d["windows"])
        if "single" in e:
            assert d["single_flush"] == e["single"]
        if "done" in e:
            # `done` is decided after the first flush of the first sweep, on the first group's points (the first 128 and the
            # remainder points).  Buried: the atoms of that flush alone leave the oracle no point of the whole sphere.  Open:
            # they leave a fused-rule point among the first 128 alive, so the exit cannot fire whatever the rest does.
            q = m.flat(w)
            acc = m._tests(w, q)[0]
            head = q[np.flatnonzero(acc)][:fl[0]]
            sub = ti.Structure.of(np.stack([c.x, c.y, c.z], -1)[[0, w] + head.tolist()], c.r[[0, w] + head.tolist()])
            left = int(ti.oracle_counts(sub, c.probe, c.n_points, c.W)[1][1])
            first_group = int(m._survivors(w, head)[:128].sum())
            assert (left == 0) == e["done"] and (first_group == 0) == e["done"], (left, first_group)
        if "id_hit" in e:
            assert d["id_hit_first_pass"] == e["id_hit"] and d["A"] == d["K"] + 1


@pytest.mark.parametrize("c", CASES + BATCHES, ids=[c.name for c in CASES + BATCHES])
def test_model_counts_are_the_oracles(c):
    m = _models(c)[0] if c in CASES else c.model()
    for s, st in enumerate(c.structures):
        if st.n:
            b, e = int(c.so[s]), int(c.so[s + 1])
            assert np.array_equal(m.K[b:e], _oracle(st, c)[2].astype(np.int64)), (s, c.name)


SWITCHES = [("swept_limit", 255, ["swept_T256", "swept_run_at_255", "swept_T256_100_16"]),
            ("swept_limit", 257, ["swept_T257", "swept_T257_64_1"]),
            ("cap", 143, ["list_K144", "list_150_ids", "list_K144_128_8"]),
            ("cap", 145, ["list_K145", "list_K145_96_8"]),
            ("flush_at", 127, ["flush_A128_one"]),
            ("flush_at", 129, ["flush_A129_then_nothing"]),
            ("window", 255, ["windows_T256", "windows_T512", "windows_run_at_255"]),
            ("window", 257, ["windows_T257", "windows_T513", "windows_run_at_256"])]


@pytest.mark.parametrize("name,value,cases", SWITCHES, ids=[f"{a}={b}" for a, b, _ in SWITCHES])
def test_each_switch_bites(name, value, cases):
    for cn in cases:
        c = pc.by_name(cn)
        m = _models(c)[0]
        w = c.model(**{name: value})
        if c.kernel == "fast":
            assert w.n_deferred != m.n_deferred, f"{name}={value} leaves n_deferred of {cn} at {m.n_deferred}"
        else:
            a, b = m.v3(c.watch), w.v3(c.watch)
            assert (a["flushes"], a["windows"]) != (b["flushes"], b["windows"]), f"{name}={value} changes nothing in {cn}"


def test_launch_arithmetic_by_hand():
    # atoms per wave: forced, capped at 40 and rounded down to tens (fast), capped at 8 (v3); n / 32 768 by default
    assert [pm.launch_apw(1000, True, f) for f in (1, 3, 10, 11, 25, 40, 64)] == [1, 3, 10, 10, 20, 40, 40]
    assert [pm.launch_apw(1000, False, f) for f in (1, 7, 8, 9)] == [1, 7, 8, 8]
    assert [pm.launch_apw(n, True) for n in (1, 32767, 65535, 65536, 32768 * 11, 32768 * 39)] == [1, 1, 1, 2, 10, 30]
    # which kernel: 128 points and 4 remainder points are the fast kernel's, 129 points or 5 remainder points are not
    assert pm.uses_fast(100, 128, 8) and not pm.uses_fast(100, 129, 8) and pm.uses_fast(100, 100, 8)
    assert not pm.uses_fast(100, 101, 16) and not pm.uses_fast(100, 100, 8, "3") and pm.uses_fast(40000, 100, 8, "4")
    assert not pm.uses_fast(32768, 100, 8) and pm.uses_fast(32767, 100, 8)
    # blocks, the remap's per and the waves' ranges: 27 atoms at 1 per wave are 7 blocks (per 0: no remap), 36 are 9
    # (per 1: block 8 keeps its number), 64 are 16 (per 2: block 1 takes the third quarter... of eight: atoms 8 - 11)
    m = pc.block_count_cases()
    assert [(c.n, c.model().n_blocks, c.model().per) for c in m] == [(27, 7, 0), (31, 8, 1), (35, 9, 1), (63, 16, 2),
                                                                    (67, 17, 2)]
    assert [pm.remap(b, 16) for b in range(16)] == [0, 2, 4, 6, 8, 10, 12, 14, 1, 3, 5, 7, 9, 11, 13, 15]
    assert [pm.remap(b, 17) for b in (0, 1, 8, 15, 16)] == [0, 2, 1, 15, 16]
    assert [pm.remap(b, 7) for b in range(7)] == list(range(7))
    w = pm.waves(85, 20, True)   # 85 atoms, 20 per wave: two blocks (per 0), the fifth wave has 5 atoms
    assert [(b, e) for b, e, _ in w] == [(0, 20), (20, 40), (40, 60), (60, 80), (80, 85)]
    assert w[0][2] == [(0, 10), (10, 20)] and w[4][2] == [(80, 85)]
    assert sorted(a for b, e, _ in pm.waves(67, 1, True) for a in range(b, e)) == list(range(67))
    # the list-mode launch: 1 024 workgroups while nothing is known, 16 at least, half the hint, never more than N / 4
    assert pm.list_trips(20000, 65, None) == (1024, 1) and pm.list_trips(20000, 65, 0) == (16, 2)
    assert pm.list_trips(20000, 200, 65) == (33, 2) and pm.list_trips(20000, 129, 4000) == (1024, 1)
    assert pm.list_trips(40, 3, None) == (10, 1) and pm.list_trips(20000, 0, 200) == (100, 0)
    assert [pm.rem_tiling(n) for n in (1, 4, 5, 8, 9, 15)] == [(2, 16), (2, 16), (3, 8), (3, 8), (4, 4), (4, 4)]


def test_wave_batches_sit_on_their_edges():
    for forced, cases in pc.fast_wave_batches().items():
        apw = pm.launch_apw(1000, True, forced)
        sizes = [c.n for c in cases[:6]]
        assert sizes == [4 * apw * k + d for k in (1, 2) for d in (-1, 0, 1)]
        for c in cases:
            m = c.model()
            assert m.apw == apw and m.fast_kernel and any(s.n == 0 for s in c.structures)
            groups = [g for _, _, gs in pm.waves(c.n, apw, True) for g in gs]
            assert sorted(a for g in groups for a in range(*g)) == list(range(c.n))
            # a structure ends inside a group (the empty one with it)
            assert any(g0 < int(b) < g1 for g0, g1 in groups for b in c.so[1:-1]) or apw == 1
            if "where" in c.expect:
                d = np.flatnonzero(m.deferred)
                assert len(d) == 1 and d[0] == c.watch and m.K[c.watch] == 145
                g = next(g for g in groups if g[0] <= m.pos[c.watch] < g[1])
                if apw >= 10:
                    assert m.pos[c.watch] - g[0] == c.expect["where"] and g[1] - g[0] == 10
    for forced, cases in pc.v3_wave_batches().items():
        apw = pm.launch_apw(1000, False, forced)
        for c in cases:
            m = c.model()
            assert m.apw == apw and not m.fast_kernel and c.n % (4 * apw) in (0, 1, 4 * apw - 1)
            ws = pm.waves(c.n, apw, False)
            assert any(b < int(c.so[1]) < e for b, e, _ in ws) or apw == 1


def test_deferring_batches_count():
    for ns, nd, want in ((0, 0, 0), (65, 0, 65), (53, 1, 200), (129, 0, 129)):
        c = pc.deferring_batch(ns, nd)
        assert c.n < pm.MX_MIN_ATOMS and c.model().n_deferred == want, (ns, nd, c.model().n_deferred)


def test_reach_cases_keep_their_flips():
    """The long grids: the intended cell counts, the model's K equal to the oracle's and the oracle's K still flipping
    across every cutoff pair.  The first admission condition cannot hold here and is not asked for: a pair at the exact
    cutoff along y or z puts its row at b2 = thr - gy^2 with gy one rounding away from sr - these cases exist to stand
    on the culling margins (tol up to 4e-3 cells), and the GPU test asserts nothing of the model for them, only the
    oracle's values and K."""
    seen = set()
    for c in pc.reach_cases():
        m = c.model(kernel="4")
        d = c.model(kernel="4", order="desc")
        assert np.array_equal(d.T, m.T) and np.array_equal(d.K, m.K)
        ks = []
        for s, st in enumerate(c.structures):
            b = int(c.so[s])
            k = _oracle(st, c)[2]
            assert np.array_equal(m.K[b:b + st.n], k.astype(np.int64)), (c.name, s)
            ks.append(int(k[c.watch]))
            dims = pm.tc.grid_of(st.x, st.y, st.z, st.r, F(c.probe))[2]
            assert abs(int(dims[c.expect["axis"]]) - c.expect["cells"]) <= 8, (c.name, dims)
            seen.add((c.expect["cells"], c.expect["axis"]))
        if c.expect["flip"]:
            assert ks[0] != ks[1] and ks[2] != ks[3] and ks[0] == ks[2], (c.name, ks)
    assert len(seen) == 9
