"""The inputs of test_gpu_mx_edges.py (mx_cases.py) pinned, on the CPU, to the limits of k_occlusion_mx they are named
for - by the routing model (mx_model.py) - and the model pinned to the oracle and to the header's arithmetic.

Order inside a cell is arrival order on the device and not defined: every figure a GPU run asserts must be the same
with the atoms of a cell in rising and in falling input order.  Atoms of one cell and radius are one kind (the cases'
clumps); the deferred SET is compared as the kinds it holds - (structure, cell, radius), counted."""
from fractions import Fraction

import numpy as np
import pytest

import mx_cases as mc
import mx_model as mm
import tie_cases as ti

F = np.float32
CASES = mc.all_cases()
IDS = [c.name for c in CASES]


def _models(c, _cache={}):
    if c.name not in _cache:
        _cache[c.name] = (c.model(bounds=True), c.model(order="desc", bounds=True))
    return _cache[c.name]


def _watch_group(c, m):
    return m.groups[m.group_of[c.watch]]


def _deferred_kinds(c, m):
    d = m.deferred
    pos = np.empty(c.n, np.int64)
    pos[m.order] = np.arange(c.n)
    return sorted((int(m.sid[pos[i]]), int(m.cell[pos[i]]), float(c.r[i]), m.reason[i]) for i in d)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_case_sits_on_its_edge(c):
    m, _ = _models(c)
    g = _watch_group(c, m)
    st = m.structs[0]
    e = c.expect
    if c.family == "union":
        assert st.has_ids == ("_ids" in c.name)
        for k in ("U", "U_first", "n_chunk", "reason", "narrowed", "self0"):
            if k in e:
                assert getattr(g, k) == e[k], (k, getattr(g, k), e[k])
        if "shift" in e:
            assert st.shift == e["shift"]
        limit = mm.UNION_IDS if st.has_ids else mm.UNION_NO_IDS
        if c.name.startswith("narrow"):
            assert g.U_first > limit >= g.U and g.cx_first == g.cx_last == 4
        else:
            assert g.g1 - g.g0 == 4 and g.cx_first == g.cx_last
            assert m.n_deferred == (4 if e["U"] > limit else 0)
    elif c.family == "first_chunk":
        assert (g.self0, g.g1 - g.g0, g.reason) == (e["self0"], e["glen"], e["reason"])
        assert g.U <= mm.UNION_IDS and m.n_deferred == (e["glen"] if e["reason"] else 0)
    elif c.name.startswith("cluster"):
        n = c.n
        assert np.all(m.K_all == n - 1) and np.all(m.K == n - 1)
        assert m.n_deferred == (n if n - 1 > mm.CAP else 0)
        assert np.all(m.second_pass == (n - 1 > 64)) and np.all((m.K + 15) // 16 == (n - 1 + 15) // 16)
    elif c.name.startswith("lone_K129"):
        assert st.shift == e["shift"] and m.K[c.watch] == 129 and m.reason[c.watch] == "cap" and m.n_deferred == 1
        mates = np.flatnonzero(m.group_of == m.group_of[c.watch])
        assert len(mates) == 34 and g.reason == "" and np.all(m.K[mates[mates != c.watch]] == e["mates"])
    elif c.name.startswith("spill"):
        big = np.flatnonzero((m.K >= 192) & (m.K <= 320))   # past the last record the sweep may store to
        assert len(big) >= 256 and np.all(m.reason[m.K > mm.CAP] == "cap")
        gs = {m.group_of[i] for i in big}
        assert all(m.groups[k].n_chunk == e["n_chunk"] and m.groups[k].reason == "" for k in gs)
        assert c.n >= 256   # four waves' worth of atoms: one workgroup whose four lists are all in use
    elif c.name.startswith("near"):
        assert (m.K[0], m.near[0]) == (e["K"], e["near"]) and m.reason[0] == ""
    elif c.family == "shift":
        assert st.has_ids == ("_ids_" in c.name) and st.shift == e["shift"]
        assert st.shift == mm.group_shift(c.n, st.n_cells, st.has_ids)
    elif c.family == "blocks":
        assert len(m.blocks) == e["n_blocks"] and m.blocks[-1][1] - m.blocks[-1][0] == e["last"] and m.apw == c.apw
        if c.name.endswith("four_plus_one"):
            assert c.n == 4 * c.apw + 1 and any(s.n == 0 for s in m.structs[1:-1])
            assert any(m.sid[b - 1] != m.sid[b] for b in range(1, c.n) if b % c.apw)   # a structure ends inside a wave
        if c.name.endswith("_four"):
            ends = [b for b, _ in m.blocks[1:]]
            assert any(m.cell[b - 1] == m.cell[b] for b in ends)                            # a cell cut by a block's end
            assert any(gr.cut_by_block for gr in m.groups)                              # a group cut by a block's end
    elif c.name.startswith("tiles"):
        st0 = c.structures[0]
        lo, hi, with_exposed = mm.live_tile_bounds(st0.centre(0), 1.5, [(st0.x[1], st0.y[1], st0.z[1], st0.r[1])], c.probe,
                                                   c.n_points, c.W)
        assert m.K[0] == 1 and lo == hi == e["tiles"]
        # (the patch test may only drop tiles whose points are all occluded: what its margins are for)
        assert not any(dead for _, dead in with_exposed)
    elif c.family in ("phase_b", "many"):
        lo_min, hi_max = (0, 0) if c.name.endswith("rem") else (int(v) for v in c.name.split("_")[3:5])
        assert m.K[0] == 1 and lo_min <= m.lo[0] <= m.hi[0] <= hi_max and (m.lo[0], m.hi[0]) == (e["lo"], e["hi"])
        if c.name.endswith("rem"):
            assert m.rem_exposed[0] >= 1   # only remainder points survive
        if c.n_points > 128:
            st0 = c.structures[0]
            lo, hi, with_exposed = mm.live_tile_bounds(st0.centre(0), 1.5, [(st0.x[1], st0.y[1], st0.z[1], st0.r[1])],
                                                       c.probe, c.n_points, c.W)
            assert len(with_exposed) <= lo <= hi and not any(dead for _, dead in with_exposed)
    elif c.family == "ids":
        assert st.has_ids and sorted(m.deferred.tolist()) == e["deferred"]
        assert all(m.reason[i] == "fold" for i in e["deferred"])
        assert ti.fold_id(int(c.ids[0])) == ti.fold_id(int(c.ids[2])) and c.ids[0] != c.ids[2]
    elif c.family == "range":
        assert m.n_deferred == e["deferred"] and set(m.reason[m.deferred]) <= {"range"}
        assert all(g.U <= 4 for g in m.groups)   # (nothing but the admission rule is in the way)
        if "dim_x" in e:
            assert int(st.dims[0]) == e["dim_x"]
    else:
        raise AssertionError(c.family)


def test_every_chunk_count_and_phase_b_form_is_there():
    chunks = {True: set(), False: set()}
    for c in CASES:
        m, _ = _models(c)
        for g in m.groups:
            if not g.reason:
                chunks[m.structs[g.sid].has_ids].add(g.n_chunk)
    assert chunks[False] >= {1, 2, 3, 4, 5} and chunks[True] >= {1, 2, 3, 4}
    forms = {k: set() for k in mc.PHASE_B_POINTS}
    for c in mc.phase_b_cases():
        m, _ = _models(c)
        lo, hi = int(m.lo[0]), int(m.hi[0])
        forms[(c.n_points, c.W)].add(0 if hi == 0 else 4 if hi <= 4 else 8 if 5 <= lo and hi <= 8 else 9 if lo >= 9 else -1)
    assert all(v == {0, 4, 8, 9} for v in forms.values()), forms
    # many points: the survivors' list is flushed when it passes 64 entries - never, once, several times
    for n_points, W in mc.MANY_POINTS:
        got = set()
        for c in mc.many_point_cases():
            if (c.n_points, c.W) == (n_points, W) and c.name.startswith("pair"):
                m, _ = _models(c)
                lo, hi = int(m.lo[0]), int(m.hi[0])
                got.add(0 if hi < 64 else 1 if 65 <= lo and hi <= 128 else 3 if lo > 192 else -1)
        assert got == ({0, 1, 3} if n_points > 192 else {0, 1}), (n_points, W, got)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_order_inside_a_cell_does_not_matter(c):
    a, d = _models(c)
    assert a.n_deferred == d.n_deferred
    assert _deferred_kinds(c, a) == _deferred_kinds(c, d)
    assert a.table() == d.table()
    for name in ("K_all", "lo", "hi", "rem_exposed"):
        assert np.array_equal(getattr(a, name), getattr(d, name)), name
    # (K and the near count of an atom are its own; -1 marks an atom of a deferred group, which a block's end may cut
    # through a cell: the kinds above cover that)
    both = (a.K >= 0) & (d.K >= 0)
    assert np.array_equal(a.K[both], d.K[both]) and np.array_equal(a.near[both], d.near[both])


SWITCHES = [("cap=127", dict(cap=127), "cluster_K128"), ("cap=129", dict(cap=129), "cluster_K129"),
            ("cap=129", dict(cap=129), "lone_K129"),
            ("union-1", dict(union_delta=-1), "union_noids_320"), ("union-1", dict(union_delta=-1), "union_ids_256"),
            ("union+1", dict(union_delta=1), "union_noids_321"), ("union+1", dict(union_delta=1), "union_ids_257"),
            ("first_chunk", dict(first_chunk_rule=False), "first_chunk_65"),
            ("midpoint", dict(midpoint_up=True), "narrow2_noids"), ("midpoint", dict(midpoint_up=True), "narrow2_ids"),
            ("blocks", dict(block_starts=False), "blocks23_four"), ("blocks", dict(block_starts=False), "blocks64_four"),
            ("blocks", dict(block_starts=False), "first_chunk_64"), ("dims_or", dict(dims_or=True), "range_dim_1024")]


@pytest.mark.parametrize("name,switch,case", SWITCHES, ids=[f"{a}-{c}" for a, _, c in SWITCHES])
def test_each_switch_bites(name, switch, case):
    c = mc.by_name(case)
    m, _ = _models(c)
    w = c.model(**switch)
    assert (w.n_deferred, w.table()) != (m.n_deferred, m.table())
    if name not in ("midpoint", "blocks"):
        assert w.n_deferred != m.n_deferred   # (what the GPU test's count would show)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_model_counts_are_the_oracles(c):
    m, _ = _models(c)
    for s, st in enumerate(c.structures):
        if st.n == 0:
            continue
        b, e = int(c.so[s]), int(c.so[s + 1])
        _, pts, k = ti.oracle_counts(st, c.probe, c.n_points, c.W)
        assert np.array_equal(m.K_all[b:e], k.astype(np.int64))
        swept = m.K[b:e] >= 0
        assert np.array_equal(m.K[b:e][swept], k.astype(np.int64)[swept])   # the union holds every candidate
        have = m.lo[b:e] >= 0
        assert np.array_equal((m.lo[b:e] + m.rem_exposed[b:e])[have], pts.astype(np.int64)[have])


def test_three_step_quotient_is_the_division_on_the_cases_limits():
    n = 0
    for c in mc.phase_b_cases() + mc.many_point_cases():
        st = c.structures[0]
        for i, j in ((0, 1), (1, 0)):
            Rr = st.r[i] + F(c.probe)
            vx, vy, vz, limit = ti.pair_terms(st.centre(i), st.r[i], st.centre(j), st.r[j], c.probe)
            tj = st.r[j] + F(c.probe)
            num = tj * tj - (vx * vx + vy * vy + vz * vz) - Rr * Rr
            assert ti.quotient_3op(num, F(2.0) * Rr) == limit == num / (F(2.0) * Rr)
            n += 1
    assert n > 50


def test_group_shift_thresholds_by_direct_arithmetic():
    nc = mc.line_cells()

    def rn(q):   # a rational rounded to float32
        return F(q.numerator) / F(q.denominator) if q.denominator < 2 ** 24 and q.numerator < 2 ** 24 else F(float(q))

    thr = mc.shift_thresholds()
    for name, t in (("0.3", F(0.3)), ("0.6", F(0.6)), ("1.0", F(1.0))):
        n_lo, n_hi, s_lo, s_hi = thr[name]
        assert n_hi == n_lo + 1
        assert rn(Fraction(n_lo, nc)) < t <= rn(Fraction(n_hi, nc))
        assert (mm.grid_group_shift(n_lo, nc), mm.grid_group_shift(n_hi, nc)) == (s_lo, s_hi)
        for ids in (True, False):
            assert mm.group_shift(n_lo, nc, ids) == (s_lo if ids else max(s_lo, 1))
            assert mm.group_shift(n_hi, nc, ids) == (s_hi if ids else max(s_hi, 1))
    n_lo, n_hi, s_lo, s_hi = thr["1.95"]
    prod = F(float(Fraction(float(F(1.95))) * nc))   # 1.95f x n_cells, rounded once
    assert n_hi == n_lo + 1 and F(n_lo) < prod and not F(n_hi) < prod and n_lo >= nc
    assert (mm.group_shift(n_lo, nc, False), mm.group_shift(n_hi, nc, False)) == (1, 0) == (s_lo, s_hi)
    assert mm.group_shift(n_lo, nc, True) == 0
    # the header's own table
    for n, cells, want in ((3, 10, 2), (29, 100, 3), (30, 100, 2), (59, 100, 2), (60, 100, 1), (99, 100, 1), (100, 100, 0),
                           (5, 0, 0)):
        assert mm.grid_group_shift(n, cells) == want
    # the shift shows in the deferred count around 1.95: pairs of cells overrun the first chunk, single cells do not
    lo, hi = mc.by_name(f"shift_1.95_noids_{n_lo}"), mc.by_name(f"shift_1.95_noids_{n_hi}")
    assert _models(lo)[0].n_deferred > 0 == _models(hi)[0].n_deferred


def test_launch_rule_and_pieces():
    assert [mm.launch_apw(n, 100) for n in (100, 229375, 229376, 458752, 917503, 917504, 1835008)] == [8, 8, 8, 16, 16, 32, 64]
    assert [mm.launch_apw(n, 960) for n in (100, 917504, 1835008)] == [8, 8, 16]
    assert mm.launch_apw(100, 100, 23) == 23 and mm.launch_apw(100, 960, 23) == 16 and mm.launch_apw(100, 100, 99) == 64
    # fewer than eight workgroups (a piece each), exactly eight, nine; blocks that the pieces do not divide; an empty piece
    assert mm.pieces(16 * 4 * 3, 16, 4) == (3, [4, 4, 4])
    assert mm.pieces(16 * 4 * 8, 16, 4) == (8, [4] * 8)
    assert mm.pieces(16 * 4 * 8 + 1, 16, 4) == (9, [5, 5, 5, 5, 5, 5, 3, 0])
    assert mm.pieces(16 * 12 * 8 + 16, 16, 12) == (9, [13] * 7 + [6])
    for n_points, W in mc.MANY_POINTS:
        for n_atoms in mc.MANY_SIZES:
            c = mc.many_point_batch(n_points, W, n_atoms)
            assert c.n == n_atoms and c.model().apw == 16


@pytest.mark.parametrize("key", mc.keys(), ids=str)
def test_packed_batches_are_order_independent(key):
    for rev in (False, True):
        c = mc.packed(key, rev)
        a, d = c.model(), c.model(order="desc")
        assert a.n_deferred == d.n_deferred and _deferred_kinds(c, a) == _deferred_kinds(c, d)
        if c.n_points <= 128:
            a, d = c.model(apw=0), c.model(order="desc", apw=0)   # the launch's own rule: blocks of 8
            assert a.apw == 8 and a.n_deferred == d.n_deferred


@pytest.mark.parametrize("offset", mc.SEG_OFFSETS)
def test_ids_seg_cases_sit_on_their_bits(offset):
    c = mc.seg_case(offset)
    a, d = _models(c)
    keep = [s for s, st in enumerate(a.structs) if st.has_ids]
    assert len(keep) == 1 and a.structs[keep[0]].base == offset and a.structs[keep[0]].n == 64 and a.apw == 8
    first, last = offset >> 6, (offset + 63) >> 6
    assert (first >> 5, first & 31, last >> 5, last & 31) == {1984: (0, 31, 0, 31), 2048: (1, 0, 1, 0),
                                                            2016: (0, 31, 1, 0)}[offset]
    for s, st in enumerate(c.structures):
        rising = bool(np.all(st.ids[1:] > st.ids[:-1]))
        assert rising != (s == keep[0])
    assert a.n_deferred == d.n_deferred == 2 and _deferred_kinds(c, a) == _deferred_kinds(c, d)
    assert set(a.reason[a.deferred]) == {"fold"}
