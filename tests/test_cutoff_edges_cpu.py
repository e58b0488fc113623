"""The cases of cutoff_edge_cases.py without a GPU: each pinned to what it is named for from the models (hse_model.py,
within_model.py, nearest_model.py) and the emulations (sweep_model.grid, nearest_model.sweep, hse_model.sweep_counts)
alone - a stop shell and the rule that stopped it, the compactions of the staging, exact ties in the last swept shell, the
margins holding or failing - with the emulation's mutants (lim_shift=+0.5, keep_unsorted) shown to bite where a case is
built for them.  On every sampled centre of every case the emulated list equals nearest_model.lists."""
import functools

import numpy as np
import pytest

import cutoff_edge_cases as ce
import hse_cases as hc
import hse_model as hm
import nearest_model as nm
import sweep_cases as sc
import sweep_model as sm
import within_model as wm

F = np.float32
INF = float("inf")


def _list(offsets, entries, i):
    return entries[int(offsets[i]):int(offsets[i + 1])]


@functools.lru_cache(maxsize=None)
def _within(name, s, cutoff):
    """The within-lists of structure s of a swept case with every atom centre and partner, computed once."""
    p = hc.part(ce.swept(name), s)
    return wm.lists(p.x, p.y, p.z, None, INF if cutoff is None else cutoff)


def _sweeps(name, s, k, cutoff, sample):
    """nm.sweep on the sampled centres of structure s, every list compared with the model; returns the Sweep."""
    p = hc.part(ce.swept(name), s)
    want = nm.truncate(*_within(name, s, cutoff), k)
    sw = nm.sweep(p.x, p.y, p.z, p.r, p.probe, None, k, cutoff, sample=sample)
    for n, i in enumerate(sample):
        assert sw.lists[n].tobytes() == _list(*want, i).tobytes(), (name, s, k, cutoff, int(i))
    return sw


def _grid(c, s=0):
    p = hc.part(c, s)
    return sm.grid(p.x, p.y, p.z, p.r, p.probe)


# ---- the adapter -------------------------------------------------------------------------------------------------------------

def test_adapter_keeps_the_structures_and_adds_directions():
    for name in ce.GRID_NAMES + ce.MARGIN_NAMES:
        d, c = sc.get(name), ce.swept(name)
        assert c.so.dtype == np.uint32 and np.array_equal(c.so, d.so) and c.probe == d.probe and c.flags is None
        for s in range(len(d.so) - 1):
            p = hc.part(c, s)
            assert all(a.tobytes() == b.tobytes() for a, b in zip((p.x, p.y, p.z, p.r), d.part(s)[:4]))
        assert c.dirs.shape == (c.n_atoms, 3) and c.dirs.dtype == F and np.isfinite(c.dirs).all() and c.dirs.any(axis=1).all()
        assert c.n_atoms < 10000
    assert [len(ce.swept(n).so) - 1 for n in ("column_z", "odd_beside_even", "margin_twelve", "margin_small_h")] == [2, 3, 12, 3]


def test_cutoffs_of_the_three_families():
    c = ce.swept("chain")
    h = float(c.h)
    assert ce.hse_cutoffs(c)[0] == 13.0 and np.allclose(ce.hse_cutoffs(c)[1:], [0.5 * h, 1.5 * h, 2.5 * h], rtol=1e-6)
    assert len(ce.within_cutoffs(c, "chain")) == 3 and ce.within_cutoffs(c, "chain")[2] > 2.0 * 383      # covers the chain
    small = ce.swept("margin_small_h")
    assert np.allclose(ce.within_cutoffs(small, "margin_small_h")[:2], [2.5 * float(small.h), 4.0 * float(small.h)], rtol=1e-6)
    for name in ce.GRID_NAMES + ce.MARGIN_NAMES:                       # every structure here is under 1 000 atoms: a covering cutoff
        c = ce.swept(name)
        cover = ce.within_cutoffs(c, name)[-1]
        for s in range(len(c.so) - 1):
            p = hc.part(c, s)
            assert np.all(wm.lengths(wm.lists(p.x, p.y, p.z, None, cover)[0]) == p.n_atoms - 1), (name, s)


# ---- A: thin, long, slanted and crowded grids ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["column_z", "slant_xp", "slant_xm", "slant_yp", "slant_ym"])
def test_columns_and_slants_sweep_to_the_end_of_a_thin_grid(name):
    c = ce.swept(name)
    for s in range(len(c.so) - 1):
        p, g = hc.part(c, s), _grid(c, s)
        assert ce.margins_of(c, s) and g.h == sc.H and sorted(g.dims)[0] == 3 and p.n_atoms < 256 + 1
        sample = ce.ends_sample(c, s)
        s_last = [g.s_last(i) for i in sample]
        assert max(s_last) >= 14
        sw = _sweeps(name, s, 256, None, sample)                        # fewer than k + 1 atoms: the shells cover the grid
        assert sw.by_rule == [""] * len(sample) and sw.stop == s_last
        assert max(sw.most_held) == p.n_atoms - 1
        for k in (1, 16):
            sw = _sweeps(name, s, k, None, sample)
            assert all(w == "kth" for w in sw.by_rule) and max(sw.stop) < min(s_last)
        for k in ce.NEAREST_KS:                                         # (5 - 1/2) h >= 13 > (4 - 1/2) h
            sw = _sweeps(name, s, k, 13.0, sample)
            assert all((w, st) == ("cutoff", 5) or (w == "kth" and st < 5) for w, st in zip(sw.by_rule, sw.stop))
            assert k == 1 or sw.by_rule == ["cutoff"] * len(sample)


def test_chain_runs_a_hundred_shells_of_nine_rows():
    c = ce.swept("chain")
    g = _grid(c)
    assert g.dims.tolist() == [246, 3, 3] and ce.margins_of(c)
    place = c.info["place"]
    sample = ce.ends_sample(c, 0)
    assert {0, sc.CHAIN_ATOMS - 1} <= set(place[sample].tolist())       # both ends of the line
    sw = _sweeps("chain", 0, 256, None, sample)
    assert sw.by_rule == ["kth"] * len(sample) and max(sw.stop) > 80 and min(sw.stop) > 80
    assert all(st < g.s_last(i) for st, i in zip(sw.stop, sample)) and not any(sw.compactions)
    # 16 atoms 2 A apart: eight on either side, and the rule is met by shell 6, well below 10 - except for the atoms within
    # eight places of an end, whose 16th neighbour is up to 32 A = 10.1 h away: both ends stop after shell 11
    sw = _sweeps("chain", 0, 16, None, sample)
    inner = np.minimum(place[sample], sc.CHAIN_ATOMS - 1 - place[sample]) >= 16
    assert sw.by_rule == ["kth"] * len(sample) and inner.sum() >= 6
    assert all(st < 10 for st, a in zip(sw.stop, inner) if a)
    assert [st for st, pl in zip(sw.stop, place[sample]) if pl in (0, sc.CHAIN_ATOMS - 1)] == [11, 11]
    for k in (16, 256):
        sw = _sweeps("chain", 0, k, 13.0, sample)
        assert sw.by_rule == ["cutoff"] * len(sample) and sw.stop == [5] * len(sample)
    _sweeps("chain", 0, 1, None, sample)
    _sweeps("chain", 0, 1, 13.0, sample)


def test_crowded_cells_fill_the_staging_without_a_compaction():
    c = ce.swept("crowded_cells")
    assert float(c.h) == float(F(21.4)) and ce.margins_of(c)
    sample = ce.ends_sample(c, 0)
    sw = _sweeps("crowded_cells", 0, 256, None, sample)
    assert max(sw.most_held) > 900 and max(sw.most_held) < nm.TRIGGER and not any(sw.compactions)
    assert all(w == "kth" for w in sw.by_rule)
    for k in ce.NEAREST_KS:
        sw = _sweeps("crowded_cells", 0, k, 13.0, sample)
        assert {"cutoff", "kth"} <= set(sw.by_rule) and not any(sw.compactions)
    _sweeps("crowded_cells", 0, 1, None, sample)
    _sweeps("crowded_cells", 0, 16, None, sample)


def test_odd_beside_even_one_structure_stops_by_a_rule_and_two_never_do():
    c = ce.swept("odd_beside_even")
    assert [ce.margins_of(c, s) for s in range(3)] == [True, False, False]
    sample = ce.ends_sample(c, 0, n=6)
    if c.info["odd"] not in sample:
        sample = np.append(sample, c.info["odd"])
    for k, cutoff in ((1, None), (16, 13.0), (256, None), (256, 13.0)):
        stops = []
        for s in range(3):
            sw = _sweeps("odd_beside_even", s, k, cutoff, sample)
            g = _grid(c, s)
            if s == 0:
                assert all(w in ("kth", "cutoff") for w in sw.by_rule) and max(sw.stop) <= 5
            else:
                assert sw.by_rule == [""] * len(sample) and sw.stop == [g.s_last(i) for i in sample]
            stops.append(sw.stop)
        assert min(stops[1]) >= 6 and stops[2] == [2] * len(sample)
    # the odd radius changes the grid, not the lists: any atom's up / down, within-list and nearest list are the same thrice
    n = hc.part(c, 0).n_atoms
    up, down = hm.counts_batch(c.x, c.y, c.z, c.so, np.tile(c.dirs[:n], (3, 1)), None, 13.0)
    assert up[:n].tobytes() == up[n:2 * n].tobytes() == up[2 * n:].tobytes() and up.any()
    assert down[:n].tobytes() == down[n:2 * n].tobytes() == down[2 * n:].tobytes() and down.any()
    for cutoff in (8.0, None):
        a, b_, d = (_within("odd_beside_even", s, cutoff) for s in range(3))
        assert a[1].tobytes() == b_[1].tobytes() == d[1].tobytes() and np.array_equal(a[0], b_[0]) and np.array_equal(a[0], d[0])


def test_ball_turned_equals_the_model_on_its_sample():
    c = ce.swept("ball_turned")
    sample = ce.ends_sample(c, 0)
    for k in ce.NEAREST_KS:
        sw = _sweeps("ball_turned", 0, k, None, sample)
        assert all(w == "kth" for w in sw.by_rule)
    sw = _sweeps("ball_turned", 0, 256, 13.0, sample)
    assert {"cutoff", "kth"} <= set(sw.by_rule) and max(sw.stop) == 5


# ---- B: the margins' edge ----------------------------------------------------------------------------------------------------------

def test_margin_structures_hold_or_fail_and_the_sweeps_follow():
    want = {"margin_under": [True] * 6, "margin_over": [False] * 6, "margin_twelve": [True, False] * 6,
            "margin_small_h": [True] * 3, "margin_large_h": [True]}
    for name, holds in want.items():
        c = ce.swept(name)
        assert [ce.margins_of(c, s) for s in range(len(c.so) - 1)] == holds, name
        cutoff = ce.nearest_cutoffs(c, name)[1]
        for s in ((0, 1, 5, 10, 11) if name == "margin_twelve" else range(len(holds))):
            sample = ce.ends_sample(c, s, n=4)
            g = _grid(c, s)
            for k, cut in ((16, None), (256, cutoff)):
                sw = _sweeps(name, s, k, cut, sample)
                if holds[s]:
                    assert all(w in ("kth", "cutoff") or st == g.s_last(i) for w, st, i in zip(sw.by_rule, sw.stop, sample))
                    assert any(sw.by_rule)
                else:
                    assert sw.by_rule == [""] * len(sample) and sw.stop == [g.s_last(i) for i in sample]
    big = float(np.abs(ce.swept("margin_under").x).max())
    assert big > 2.0e5 and float(np.abs(ce.swept("margin_small_h").x).max()) > 6.0e3


@pytest.mark.parametrize("axis,sign", ce.DIRECTIONS)
def test_edge_at_margin_keeps_its_ties_in_the_last_swept_shell(axis, sign):
    e = hc.edge()
    under_t, over_t = ce.edge_shifts()[(axis, sign)]
    assert over_t - under_t == 0.015625 and under_t == (130988.0 if sign > 0 else 130984.0)
    for which in ce.WHICH:
        c = ce.edge_at_margin(axis, sign, which)
        info = c.info
        xyz = np.stack([c.x, c.y, c.z], -1)
        ref = np.stack([e.x, e.y, e.z], -1)
        hi_like = np.flatnonzero(ref[:, axis] != np.round(ref[:, axis]))     # `hi`, one ulp under 40, and its partners
        assert info["hi"] in hi_like and len(hi_like) == 13
        want = ref[:, axis].astype(np.float64) + sign * info["shift"]
        want[hi_like] = np.round(ref[hi_like, axis]) + sign * info["shift"]  # they round onto the integer: `hi` onto its cell boundary
        assert want[info["hi"]] == 40.0 + sign * info["shift"]
        assert np.array_equal(xyz[:, axis].astype(np.float64), want)         # everything else is moved exactly
        moved = np.abs(xyz[:, axis].astype(np.float64) - np.round(xyz[:, axis]))
        assert np.all(moved == (0.0 if which == "under" else 0.015625))      # integers / one ulp of 65536 h further
        others = [k for k in range(3) if k != axis]
        assert xyz[:, others].tobytes() == ref[:, others].tobytes()
        assert ce.margins_of(c) == (which == "under")
        g = _grid(c)
        assert g.h == F(2.0)
        off, ent = wm.lists(c.x, c.y, c.z, None, hc.EDGE_CUTOFF)
        centres = [info["hi"], info["lo"]]
        for cen in centres:
            ties = [a for a, _, _ in info["tie"][cen]]
            far = [a for a, _, _ in info["far"][cen]]
            d2 = wm.d2_of(c.x[cen], c.y[cen], c.z[cen], c.x[ties], c.y[ties], c.z[ties])
            assert d2.tolist() == [25.0] * 6                            # d2 == c2 exactly, out there too
            shells = np.abs(g.cells[ties] - g.cells[cen]).max(axis=1)
            assert sorted(shells.tolist()) == [2, 2, 2, 3, 3, 3]
            li = _list(off, ent, cen)
            assert set(ties) <= set(li["idx"].tolist()) and not set(far) & set(li["idx"].tolist())
            assert int((li["d2"] == F(25.0)).sum()) == 6
        sw = nm.sweep(c.x, c.y, c.z, c.r, c.probe, None, 256, hc.EDGE_CUTOFF, sample=centres)
        up, down, stop, by_rule, found = hm.sweep_counts(c.x, c.y, c.z, c.r, c.probe, None, None, hc.EDGE_CUTOFF, centres)
        want_up, _ = hm.counts(c.x, c.y, c.z, None, None, hc.EDGE_CUTOFF)
        for n, cen in enumerate(centres):
            assert sw.lists[n].tobytes() == _list(off, ent, cen).tobytes()
            assert up[n] == want_up[cen] == len(_list(off, ent, cen)) and down[n] == 0 and found[n][-1] == 3
        if which == "under":                                           # the rule is met, with equality, after shell 3
            assert sw.by_rule == ["cutoff"] * 2 and sw.stop == [3, 3] and stop.tolist() == [3, 3] and by_rule.all()
            short = hm.sweep_counts(c.x, c.y, c.z, c.r, c.probe, None, None, hc.EDGE_CUTOFF, centres, half=-0.5)
            assert short[2].tolist() == [2, 2] and (short[0] < up).all()               # a rule one shell early loses ties
        else:                                                          # the margins fail: the whole grid
            assert sw.by_rule == ["", ""] and sw.stop == [g.s_last(i) for i in centres] == [22, 31]
            assert stop.tolist() == [22, 31] and not by_rule.any()
    assert e.n_atoms == c.n_atoms


def test_edge_twelve_interleaves_under_and_over():
    c = ce.edge_twelve()
    assert len(c.so) == 13 and [ce.margins_of(c, s) for s in range(12)] == [True, False] * 6
    for s, p in enumerate(c.info["members"]):
        q = hc.part(c, s)
        assert q.x.tobytes() == p.x.tobytes() and q.y.tobytes() == p.y.tobytes() and q.z.tobytes() == p.z.tobytes()


@pytest.mark.parametrize("k", ce.nc.EDGE_KS)
def test_knn_edge_at_margin(k):
    """The pin test_nearest_cpu.py makes for knn_edge, after the construction was moved onto multiples of 1/64 and
    translated to the margins' edge: it holds in all six directions."""
    base = ce.knn_edge_64(k)
    assert sm.grid(base.x, base.y, base.z, base.r, base.probe).h == F(ce.nc.EDGE_H)
    for axis, sign in ce.DIRECTIONS:
        for which in ce.WHICH:
            c = ce.knn_edge_at_margin(k, axis, sign, which)
            g = sm.grid(c.x, c.y, c.z, c.r, c.probe)
            assert ce.margins_of(c) == (which == "under") and float(np.abs([c.x, c.y, c.z][axis]).max()) > 1.3e5
            want = nm.lists(c.x, c.y, c.z, c.flags, k)
            groups = c.info["groups"]
            centres = [gr["centre"] for gr in groups]
            assert np.flatnonzero(wm.lengths(want[0])).tolist() == centres
            for gr in groups:
                i = gr["centre"]
                unit = np.zeros(3, np.int64)
                unit[gr["axis"]] = gr["sign"]
                li = _list(*want, i)
                assert len(li) == k and li["idx"][-1] == gr["true_kth"] and gr["diagonal"] not in li["idx"]
                assert np.all(g.cells[li["idx"][:-1]] == g.cells[i])                       # k - 1 partners in its own cell
                assert np.array_equal(g.cells[gr["true_kth"]] - g.cells[i], 2 * unit)      # the k-th in shell 2, on the axis
                d = g.cells[gr["diagonal"]] - g.cells[i]
                assert d[gr["axis"]] == -gr["sign"] and np.abs(d).max() == 1 and np.abs(d).sum() == 2
                assert li["d2"][-1] == F(ce.KNN_TRUE) ** 2                                 # exact: (2 + 3/64)^2
                assert wm.d2_of(c.x[i], c.y[i], c.z[i], *(a[gr["diagonal"]] for a in (c.x, c.y, c.z))) == F(8.0)
                if k > 1:
                    assert np.sqrt(li["d2"][-2]) / 2.0 < 0.95
            right = nm.sweep(c.x, c.y, c.z, c.r, c.probe, c.flags, k, sample=centres)
            for n, i in enumerate(centres):
                assert right.lists[n].tobytes() == _list(*want, i).tobytes()
            if which == "over":
                assert right.by_rule == [""] * 6 and right.stop == [g.s_last(i) for i in centres]
                continue
            assert right.stop == [2] * 6 and right.by_rule == ["kth"] * 6                   # found in the last shell swept
            relaxed = nm.sweep(c.x, c.y, c.z, c.r, c.probe, c.flags, k, sample=centres, lim_shift=0.5)
            assert relaxed.stop == [1] * 6
            for n, gr in enumerate(groups):                                                 # the case bites
                assert relaxed.lists[n].tobytes() != _list(*want, gr["centre"]).tobytes()
                assert relaxed.lists[n]["idx"][-1] == gr["diagonal"]
    t = ce.knn_edge_twelve(k)
    assert [ce.margins_of(t, s) for s in range(12)] == [True, False] * 6 and np.array_equal(t.flags, np.tile(base.flags, 12))


# ---- C: k_nearest past its first compaction ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _dense_sweep(odd, k, cutoff=None, keep_unsorted=False):
    c = ce.knn_dense(odd)
    return nm.sweep(c.x, c.y, c.z, c.r, c.probe, c.flags, k, cutoff, sample=c.info["centres"], keep_unsorted=keep_unsorted)


def test_knn_dense_is_built_as_described():
    c = ce.knn_dense()
    g = _grid(c)
    last, near = c.info["last"], c.info["near"]
    assert c.n_atoms == 2 + ce.DENSE_ATOMS + ce.DENSE_NEAR + 1 and last == c.n_atoms - 1 and c.info["centres"] == [last, 5, 1500]
    assert g.dims.tolist() == [11, 11, 11] and g.h == F(ce.DENSE_H) and ce.margins_of(c) and np.all(c.r == F(1.88))
    assert np.all(g.cells[2:2 + ce.DENSE_ATOMS] == 4) and np.all(g.cells[last] == 4) and np.all(g.cells[near] == 3)
    d2 = wm.d2_of(c.x[last], c.y[last], c.z[last], c.x[2:2 + ce.DENSE_ATOMS], c.y[2:2 + ce.DENSE_ATOMS], c.z[2:2 + ce.DENSE_ATOMS])
    assert np.all(np.diff(d2.astype(np.float64)) <= 1e-2) and d2[0] > 25.0 and d2[-1] < 0.1   # descending (to the rounding)
    assert np.flatnonzero(c.flags & 2).tolist() == [5, 1500, last] and np.all(c.flags & 1)
    o = ce.knn_dense(True)
    go = _grid(o)
    assert not ce.margins_of(o) and go.h == F(71.4) and go.dims.max() <= 4
    assert len(np.unique(go.cells, axis=0)) == 1                                             # all in one cell: shell 0


def test_knn_dense_compacts_again_with_a_bound_in_force():
    c = ce.knn_dense()
    last, near = c.info["last"], c.info["near"]
    at = {k: _dense_sweep(False, k) for k in ce.DENSE_KS}
    assert len(at[256].compactions[0]) >= 3 and len(at[1].compactions[0]) >= 2            # `last`
    assert len(at[256].compactions[2]) >= 2                                                 # atom 1 500
    assert at[256].most_held[0] == nm.K_NN_STAGE
    # (every compaction after the first happens with the last one's bound in force and replaces it)
    for k in ce.DENSE_KS:
        sw, want = at[k], nm.lists(c.x, c.y, c.z, c.flags, k)
        assert all(w == "kth" and st in (1, 2) for w, st in zip(sw.by_rule, sw.stop)), k
        wrong = 0
        bad = _dense_sweep(False, k, keep_unsorted=True)
        for n, i in enumerate(c.info["centres"]):
            assert sw.lists[n].tobytes() == _list(*want, i).tobytes(), (k, i)
            wrong += bad.lists[n].tobytes() != _list(*want, i).tobytes()
        assert wrong >= 1, k                                                                # the case bites
    # keys below the bound that arrive from shell 1 after shell 0 was compacted
    for k, n_near in ((1, 0), (64, ce.DENSE_NEAR), (256, ce.DENSE_NEAR)):
        assert int(np.isin(at[k].lists[0]["idx"], near).sum()) == n_near, k
    g = _grid(c)
    assert np.all(np.abs(g.cells[near] - g.cells[last]).max(axis=1) == 1)


def test_knn_dense_with_an_odd_radius_stages_everything_in_shell_0():
    """All 3 042 partners lie in the centre's own cell, in input order.  `last` is compacted three times, atom 1 500 twice;
    atom 5, the sixth farthest from `last`, meets its nearest partners first and is compacted once, with a bound that lets
    almost nothing more in."""
    o = ce.knn_dense(True)
    for k in (1, 256):
        sw, want = _dense_sweep(True, k), nm.lists(o.x, o.y, o.z, o.flags, k)
        assert sw.by_rule == ["", "", ""]
        assert len(sw.compactions[0]) >= 3 and all(len(cp) >= 1 for cp in sw.compactions)
        assert k == 1 or len(sw.compactions[2]) >= 2
        for n, i in enumerate(o.info["centres"]):
            assert sw.lists[n].tobytes() == _list(*want, i).tobytes()
    even = nm.lists(*(getattr(ce.knn_dense(), a) for a in "xyz"), o.flags, 256)
    assert even[1].tobytes() == want[1].tobytes()                                            # the radius changes the grid only


def test_knn_dense_cutoffs_below_and_above_the_bound():
    c = ce.knn_dense()
    last = c.info["last"]
    full = _dense_sweep(False, 256).lists[0]
    assert F(1.0) < full["d2"][-1] < F(9.0)                                                  # c2 = 1 is under the k-th d2, c2 = 9 above
    for cutoff, short in ((1.0, True), (3.0, False)):
        for k in ce.DENSE_KS:
            sw, want = _dense_sweep(False, k, cutoff), nm.lists(c.x, c.y, c.z, c.flags, k, cutoff)
            for n, i in enumerate(c.info["centres"]):
                assert sw.lists[n].tobytes() == _list(*want, i).tobytes()
            assert (len(_list(*want, last)) < k) == (short and k >= 255)
    assert not any(_dense_sweep(False, 256, 1.0).compactions) and all(_dense_sweep(False, 256, 3.0).compactions)


def test_knn_dense_thrice():
    t, c = ce.knn_dense_thrice(), ce.knn_dense()
    n = c.n_atoms
    assert t.so.tolist() == [0, n, 2 * n, 3 * n] and int(((t.flags & 2) != 0).sum()) == n + 6
    assert np.all(t.flags[n:2 * n] == 3) and t.flags[:n].tobytes() == t.flags[2 * n:].tobytes() == c.flags.tobytes()


# ---- E: the threads' rotation -------------------------------------------------------------------------------------------------------

def test_thread_rotation_covers_every_input_on_every_thread():
    for tid in range(ce.THREADS):
        assert {ce.thread_input(tid, it) for it in range(ce.THREAD_ROUNDS)} == set(ce.THREAD_INPUTS)
    for it in range(ce.THREAD_ROUNDS):
        assert {ce.thread_input(tid, it) for tid in range(ce.THREADS)} == set(ce.THREAD_INPUTS)
