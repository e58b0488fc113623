"""The dot curvature without a GPU: the model (curvature_model.py: the header's definition in numpy float32) pinned to a
float64 evaluation, to the sphere, to hand tables, to its invariances and to every clause of the drop rule; the cases of
curvature_cases.py pinned to what they are named for; the emulated sweep and staging cut of k_dot_curvature against the
model, with the switches that show a case bites; curvature_values against a per-dot eigen-solver; the bindings, the
Python rules that need no GPU and the stand-alone checks program under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import curvature_cases as cvc
import curvature_model as cvm
import depth_cases as dc
import sweep_cases as sc
import sweep_model as sm
from rustsasa_amd import (CURV_COLUMNS, CURV_D2, CURV_H, CURV_XX, CURV_XY, CURV_XZ, CURV_YY, CURV_YZ, CURV_ZZ,
                          curvature_values)

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 24
U = 2.0 ** -24


def _one(c, s=0):
    """(x, y, z, r, mask) of structure s of a case."""
    b, e = int(c.so[s]), int(c.so[s + 1])
    return c.part(s) + (cvc.masks(cvc.key(c))[b:e],)


def test_constants_are_the_models():
    assert (CURV_D2, CURV_H, CURV_XX, CURV_YY, CURV_ZZ, CURV_XY, CURV_XZ, CURV_YZ) == tuple(range(8)) == \
        (cvm.D2, cvm.H, cvm.XX, cvm.YY, cvm.ZZ, cvm.XY, cvm.XZ, cvm.YZ)
    assert CURV_COLUMNS == cvm.COLUMNS == 8 and cvm.ONE == ONE and cvm.BOUND == 2.0 ** 24
    text = open(os.path.join(ROOT, "rustsasa_amd", "csrc", "device_types.h")).read()
    assert "constexpr uint32_t kCurvColumns = 8;" in text


# ---- the model against float64, the sphere, the trace ----------------------------------------------------------------------------

@pytest.mark.parametrize("name,n_points,reach", [("cluster", 65, 3.0), ("sphere", 100, 3.0), ("corner", 33, 6.0)])
def test_model_stays_within_the_derived_bound_of_a_float64_evaluation(name, n_points, reach):
    """The bound is curvature_model.sums64's, derived there from the roundings of one pair and summed over the pairs of
    the row; it is stated, not tuned."""
    c = {"cluster": lambda: cvc.cluster(n_points, reach), "sphere": lambda: cvc.sphere(n_points, reach),
         "corner": lambda: cvc.of(dc.get("corner"), n_points, reach)}[name]()
    for s in range(len(c.so) - 1):
        x, y, z, r, mask = _one(c, s)
        _, pairs, mom, _ = cvm.rows(x, y, z, r, mask, c.probe, n_points, reach)
        want, bound = cvm.sums64(x, y, z, r, mask, c.probe, n_points, reach)
        got = mom.astype(np.float64) / ONE
        assert pairs.any() or len(pairs) <= n_points
        worst = np.abs(got - want) / np.maximum(bound, 1e-300)
        print(name, s, "largest |model - float64| / bound per column:", worst.max(axis=0) if len(worst) else None)
        assert (np.abs(got - want) <= bound).all()


@pytest.mark.parametrize("n_points,reach", [(100, 1.5), (100, 3.0), (960, 1.5), (960, 3.0)])
def test_lone_sphere_has_mean_curvature_one_over_R(n_points, reach):
    """On a sphere every chord has h = -d2 / (2 R) exactly, so H R - 1 = -(2 R Sum(dh) + Sum(dd2)) / Sum(d2) with dh, dd2
    the errors of the float32 terms against the true sphere.  A dot's coordinate is c + R s rounded twice (the product: u R;
    the sum: u (|c| + R)) and s is a unit vector up to 3 u: e_q = u (|c|_inf + 2 R) + 3 u R per coordinate.  A chord
    component errs by 2 e_q + u |d|; h by sqrt(3) (1 + 3 u) times that plus 3 u |h| for its own arithmetic; d2 by 2 |d|
    sqrt(3) times that plus 3 u d2; |h| <= |d| <= reach (1 + 4 u); half a unit of 2^-24 each for the conversion."""
    c = cvc.sphere(n_points, reach)
    _, pairs, mom, dropped, mask = cvc.model(c)
    R = float(F(cvc.SPHERE_RADIUS) + F(c.probe))
    assert mask.all() and (pairs > 0).all() and not dropped.any()
    mean = curvature_values(pairs, mom)[0]
    L = reach * (1 + 4 * U)
    e_q = U * (max(abs(float(c.x[0])), abs(float(c.y[0])), abs(float(c.z[0]))) + 2 * R) + 3 * U * R
    e_d = 2 * e_q + U * L
    e_h = np.sqrt(3.0) * (1 + 3 * U) * e_d + 3 * U * L + 0.5 * U
    e_d2 = 2 * L * np.sqrt(3.0) * e_d + 3 * U * L * L + 0.5 * U
    bound = pairs * (2 * R * e_h + e_d2) / (mom[:, CURV_D2] / ONE)
    print(n_points, reach, "largest |H R - 1|:", np.abs(mean * R - 1).max(), "smallest bound:", bound.min())
    assert (np.abs(mean * R - 1) <= bound).all() and bound.max() < 2e-4
    k1 = curvature_values(pairs, mom)[2]
    assert (k1 * R > 0.99).all()        # the split is loose by nature (the header says how loose); it never falls below


@pytest.mark.parametrize("name", ["cluster", "sphere", "cavity"])
def test_the_three_diagonal_moments_add_up_to_the_height(name):
    """Per pair e_k = fl(fl(t_k^2) g): their sum is g Sum(s_k) (1 + u), g = h / t2 (1 + u), t2 = Sum(s_k) (1 + 2 u) - the
    squares are shared, so their roundings cancel - : within 5 u |h| of h, |h| <= reach; four conversions of half a unit:
    (5 reach + 3) units of 2^-24 per pair."""
    c = {"cluster": cvc.cluster(100), "sphere": cvc.sphere(960, 3.0), "cavity": cvc.reach_case(6.0)}[name]
    _, pairs, mom, _, _ = cvc.model(c)
    diff = np.abs(mom[:, CURV_XX] + mom[:, CURV_YY] + mom[:, CURV_ZZ] - mom[:, CURV_H])
    bound = pairs.astype(np.float64) * (5 * c.reach + 3)
    print(name, "largest |XX + YY + ZZ - H| over its bound:", (diff / np.maximum(bound, 1)).max())
    assert pairs.any() and (diff <= bound).all()


# ---- hand tables -------------------------------------------------------------------------------------------------------------------

def test_hand_table_of_two_dots():
    c = cvc.two_dots()
    off, pairs, mom, dropped, mask = cvc.model(c)
    assert mask.all() and off.tolist() == [0, 1, 2] and pairs.tolist() == [1, 1] and not dropped.any()
    g = F(4.0) / F(9.0)
    xx = int(np.rint(float(F(9.0) * g) * ONE))
    assert mom[0].tolist() == [25 * ONE, 4 * ONE, xx, 0, 0, 0, 0, 0]
    assert mom[1].tolist() == [25 * ONE, -4 * ONE, -xx, 0, 0, 0, 0, 0]
    assert abs(xx - 4 * ONE) <= 2                                        # 9 * fl(4 / 9) is 4 to a rounding
    mean = curvature_values(pairs, mom)[0]
    assert mean.tolist() == [-8.0 / 25.0, 8.0 / 25.0]                    # dot 1 lies above dot 0's plane: concave from 0
    # beyond the reach nothing counts
    assert not cvm.rows(*_one(c), c.probe, 1, float(np.nextafter(F(5.0), F(0.0))))[1].any()


def test_hand_table_of_two_atoms_on_an_axis_at_two_points():
    """Both atoms have the dots R s_0 = (0, 0, 2) and R s_1 above their centres; each dot sees three others.  The table is
    computed here step by step in scalar float32, not by the model's vector expression."""
    from oracle import pyoracle as po
    c = cvc.axis_pair()
    off, pairs, mom, dropped, mask = cvc.model(c)
    assert mask.all() and off.tolist() == [0, 2, 4] and pairs.tolist() == [3, 3, 3, 3] and not dropped.any()
    s = np.stack([np.asarray(a, F) for a in po.sphere_points(2)], -1)
    assert s[0].tolist() == [0.0, 0.0, 1.0]
    q = [np.array([F(cx) + F(2.0) * s[k][0], F(0.0) + F(2.0) * s[k][1], F(0.0) + F(2.0) * s[k][2]], F) for cx in (0.0, 6.0) for k in (0, 1)]
    for a in range(4):
        n = s[a % 2]
        want = [0] * 8
        for b in range(4):
            if b == a:
                continue
            d = q[b] - q[a]
            d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            h = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]
            t = [d[k] - h * n[k] for k in range(3)]
            t2 = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
            g = h / t2
            terms = [d2, h, (t[0] * t[0]) * g, (t[1] * t[1]) * g, (t[2] * t[2]) * g, (t[0] * t[1]) * g, (t[0] * t[2]) * g,
                     (t[1] * t[2]) * g]
            assert all(type(v) is F for v in terms) and d2 <= F(16.0) * F(16.0) and t2 > 0
            want = [w + int(np.rint(float(v) * ONE)) for w, v in zip(want, terms)]
        assert mom[a].tolist() == want, a
    # the pole dots 0 and 2 see the other pole dot flat (h = 0) and the side dot of their own atom 2 below (h = -2) - as
    # they see the other atom's side dot
    assert mom[0, CURV_D2] == mom[3, CURV_D2] != mom[1, CURV_D2] == mom[2, CURV_D2] and mom[0, CURV_H] == mom[2, CURV_H] == -4 * ONE


# ---- invariances --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def knot():
    """Five atoms with coordinates in [40, 44]: every dot coordinate lies in [36, 48], inside one binade."""
    rng = np.random.default_rng(5)
    xyz = np.round(rng.uniform(40.0, 44.0, (5, 3)), 3)
    return cvc._build("knot", [(xyz, rng.choice(dc.RADII, 5))], 33, 3.0)


def test_a_permutation_of_the_atoms_permutes_the_rows_and_changes_no_bits(knot):
    off, pairs, mom, _, mask = cvc.model(knot)
    perm = np.array([3, 0, 4, 1, 2])
    p = cvc._build("knot_perm", [(np.stack([knot.x, knot.y, knot.z], -1)[perm], knot.r[perm])], 33, 3.0)
    p_off, p_pairs, p_mom, _, p_mask = cvc.model(p)
    assert np.array_equal(p_mask, mask[perm]) and pairs.any()
    for new, old in enumerate(perm):
        a, b = slice(int(p_off[new]), int(p_off[new + 1])), slice(int(off[old]), int(off[old + 1]))
        assert np.array_equal(p_pairs[a], pairs[b]) and np.array_equal(p_mom[a], mom[b])


def test_a_translation_by_a_power_of_two_inside_the_binade_changes_no_bits(knot):
    """+8 keeps every centre and every dot inside [32, 64): c + 8 and fl(c + R s) + 8 are exact, every chord is the same."""
    off, pairs, mom, _, mask = cvc.model(knot)
    xyz = np.stack([knot.x, knot.y, knot.z], -1) + F(8.0)
    assert xyz.dtype == F and np.array_equal(xyz - F(8.0), np.stack([knot.x, knot.y, knot.z], -1))
    t = cvc._build("knot_moved", [(xyz, knot.r)], 33, 3.0)
    t_off, t_pairs, t_mom, _, t_mask = cvc.model(t)
    q = cvm.dots(*_one(t), t.probe, 33)[1]
    assert q.min() >= 32.0 and q.max() < 64.0 and cvm.dots(*_one(knot), knot.probe, 33)[1].min() >= 32.0
    assert np.array_equal(t_mask, mask) and np.array_equal(t_pairs, pairs) and np.array_equal(t_mom, mom)


# ---- the drop rule ------------------------------------------------------------------------------------------------------------------

def test_a_coincident_pair_does_not_count():
    c = cvc.coincident()
    off, pairs, mom, dropped, mask = cvc.model(c)
    q = cvm.dots(*_one(c), c.probe, 1)[1]
    assert mask.all() and np.array_equal(q[0], q[1]) and not np.array_equal(q[0], q[2])
    assert pairs.tolist() == [1, 1, 2] and not dropped.any()              # (d2 == 0 is no `dropped`: links have no such entry either)
    assert mom[0].tolist() == mom[1].tolist() == [9 * ONE, 0, 0, 0, 0, 0, 0, 0] and mom[2, CURV_D2] == 18 * ONE


def test_a_dot_straight_above_does_not_count():
    c = cvc.above()
    off, pairs, mom, dropped, mask = cvc.model(c)
    assert mask.all() and pairs.tolist() == [1, 0, 1] and dropped.tolist() == [1, 1, 0]
    assert mom[0].tolist() == mom[2].tolist() == [16 * ONE, 0, 0, 0, 0, 0, 0, 0] and not mom[1].any()
    assert np.isnan(np.array(curvature_values(pairs, mom))[:, 1]).all()


def test_a_term_of_2_to_the_24_counts_and_the_next_float_does_not():
    c = cvc.bound()
    off, pairs, mom, dropped, mask = cvc.model(c)
    q = cvm.dots(*_one(c), c.probe, 1)[1]
    d2 = lambda d: d[0] * d[0] + d[1] * d[1] + d[2] * d[2]  # noqa: E731
    assert mask.all() and d2(q[1] - q[0]) == F(2.0 ** 24) and d2(q[2] - q[0]) == np.nextafter(F(2.0 ** 24), F(np.inf))
    assert pairs.tolist() == [1, 1, 0] and dropped.tolist() == [1, 1, 2]
    assert mom[0].tolist() == mom[1].tolist() == [ONE * ONE, 0, 0, 0, 0, 0, 0, 0] and not mom[2].any()


@pytest.mark.parametrize("which", ["coordinate", "radius"])
def test_a_nan_atom_has_zero_rows_and_pairs_with_nobody(which):
    c = cvc.nan_case(which)
    a = c.info["atom"]
    off, pairs, mom, dropped, mask = cvc.model(c)
    mine = slice(int(off[a]), int(off[a + 1]))
    assert mask[a].all() and not pairs[mine].any() and not mom[mine].any() and pairs.any()
    keep = np.arange(c.n_atoms) != a
    x, y, z, r, m = _one(c)
    _, w_pairs, w_mom, _ = cvm.rows(x[keep], y[keep], z[keep], r[keep], m[keep], c.probe, c.n_points, c.reach)
    rest = np.ones(len(pairs), bool)
    rest[mine] = False
    assert np.array_equal(pairs[rest], w_pairs) and np.array_equal(mom[rest], w_mom)


def test_ties_at_the_reach_are_in_and_one_float_under_they_are_out():
    c = cvc.above()                                                       # d2 == 16 == 4 * 4 between dots 0 and 2
    assert cvm.rows(*_one(c), c.probe, 1, 4.0)[1].tolist() == [1, 0, 1]
    assert cvm.rows(*_one(c), c.probe, 1, float(np.nextafter(F(4.0), F(0.0))))[1].tolist() == [0, 0, 0]
    assert cvm.rows(*_one(c), c.probe, 1, 5.0)[1].tolist() == [1, 1, 2]   # dots 1 and 2: d2 == 25


@pytest.mark.parametrize("reach", [0.0, -0.0, 1e-30])
def test_reach_zero_and_a_reach_whose_square_underflows_give_zero_rows(reach):
    c = cvc.cluster(65, reach)
    off, pairs, mom, dropped, mask = cvc.model(c)
    assert int(off[-1]) > 100 and not pairs.any() and not mom.any() and not dropped.any()
    z = cvc.coincident()                                                  # d2 == 0 <= 0 passes the reach and fails d2 > 0
    assert not cvm.rows(*_one(z), z.probe, 1, reach)[1].any()


# ---- the emulated sweep ------------------------------------------------------------------------------------------------------------

def _sweep_equals_model(c, per_structure=6, **kw):
    off, pairs, mom, _, mask = cvc.model(c)
    seen = 0
    for s in range(len(c.so) - 1):
        b, e = int(c.so[s]), int(c.so[s + 1])
        have = np.flatnonzero(mask[b:e].any(axis=1))
        sample = have[np.linspace(0, len(have) - 1, min(per_structure, len(have))).astype(int)] if len(have) else have
        if len(sample) == 0:
            continue
        p, m = cvm.sweep_rows(*c.part(s), mask[b:e], c.probe, c.n_points, c.reach, sample, **kw)
        rows = np.concatenate([np.arange(int(off[b + i]), int(off[b + i + 1])) for i in sample])
        assert np.array_equal(p, pairs[rows]) and np.array_equal(m, mom[rows]), (c.name, s)
        seen += int(p.sum())
    return seen


@pytest.mark.parametrize("name", ["cluster65", "dot_counts", "cell65", "cell200", "column_z", "slant_xp", "slant_ym", "margin_over",
                                  "half_h", "six", "coincident", "above", "cut_at", "cut_beyond", "bare_cut"])
def test_sweep_equals_the_model_on_the_cases(name):
    h = float(F(dc.PROBE) + dc.RADII.max())
    c = {"cluster65": lambda: cvc.cluster(65), "dot_counts": cvc.dot_counts, "cell65": lambda: cvc.cell_of(65),
         "cell200": lambda: cvc.cell_of(200), "column_z": lambda: cvc.sweep_case("column_z", 1),
         "slant_xp": lambda: cvc.sweep_case("slant_xp", 1), "slant_ym": lambda: cvc.sweep_case("slant_ym", 1),
         "margin_over": lambda: cvc.sweep_case("margin_over", 100), "half_h": lambda: cvc.reach_case(cvc.reaches(h)[2]),
         "six": lambda: cvc.reach_case(6.0), "coincident": cvc.coincident, "above": cvc.above,
         "cut_at": lambda: cvc.at_the_cut(False), "cut_beyond": lambda: cvc.at_the_cut(True), "bare_cut": cvc.bare_cut}[name]()
    few = 2 if name in ("margin_over", "six", "half_h") else 6
    # (the slanted columns have one dot each, and at the cut nothing is within the reach: equal, and all zero)
    assert _sweep_equals_model(c, few) > 0 or name in ("slant_xp", "slant_ym", "cut_at", "cut_beyond")
    if name == "column_z":
        assert sm.s_end_of(F(c.reach), sm.grid(*c.part(1), c.probe).h, 99, True) == 8


def test_the_cases_are_what_they_are_named_for():
    # dots per atom
    c = cvc.dot_counts()
    assert cvc.masks(cvc.key(c)).sum(axis=1)[c.info["first"]].tolist() == [0, 1, 63, 64, 65]
    # staging rounds of 63, 64 and 64 + 1 atoms; a cell of 200
    for k in cvc.CELL_COUNTS:
        c = cvc.cell_of(k)
        x, y, z, r, mask = _one(c)
        g = sm.grid(x, y, z, r, c.probe)
        assert mask.all() and len(np.unique(g.cells[:k], axis=0)) == 1 and sm.margins_hold(x, y, z, r, c.probe)
        rounds = [len(a) for a in cvm.staged_rounds(x, y, z, r, mask, c.probe, c.reach, 0, g)]
        assert rounds[:2] == {63: [63], 64: [64], 65: [64, 1], 200: [64, 64]}[k][:2]
    # the cut: exactly at it the atom is staged, one float beyond it is not; the margins hold
    for beyond in (False, True):
        c = cvc.at_the_cut(beyond)
        x, y, z, r, mask = _one(c)
        assert sm.margins_hold(x, y, z, r, c.probe) and mask.any(axis=1).all()
        staged = np.concatenate(cvm.staged_rounds(x, y, z, r, mask, c.probe, c.reach, 0))
        assert (1 in staged) == (not beyond) and x[1] == (np.nextafter(c.info["lim"], F(np.inf)) if beyond else c.info["lim"])
        assert 1 in np.concatenate(cvm.staged_rounds(x, y, z, r, mask, c.probe, c.reach, 0, margins=False))   # without the margins: no cut
    # a structure that fails the margins beside one that passes
    u, o = cvc.sweep_case("margin_under", 100), cvc.sweep_case("margin_over", 100)
    assert all(sm.margins_hold(*u.part(s), u.probe) and not sm.margins_hold(*o.part(s), o.probe) for s in range(6))
    # the reaches: h / 2 sweeps three shells, 6 A five, and the whole-grid reach every shell there is
    c = cvc.reach_case(3.0)
    h = sm.grid(*c.part(0), c.probe).h
    assert h == F(dc.PROBE) + dc.RADII.max() and [sm.s_end_of(F(L), h, 99, True) for L in cvc.reaches(h)] == [3, 3, 3, 3, 4, 5]
    w = cvc.whole_grid()
    g = sm.grid(*w.part(0), w.probe)
    assert all(sm.s_end_of(F(w.reach), g.h, g.s_last(i), True) == g.s_last(i) for i in range(w.n_atoms))
    # the big structure
    b = cvc.big()
    assert np.diff(b.so.astype(np.int64)).tolist()[-3:] == [0, 65536, 0] and 0 in np.diff(b.so.astype(np.int64)).tolist()[:1]


@pytest.mark.parametrize("d", range(6))
def test_one_shell_short_loses_the_tie_partner_in_the_last_swept_shell(d):
    c = cvc.last_shell_tie(d)
    L, below = c.info["L"], c.info["below"]
    x, y, z, r = c.part(0)
    mask = np.ones((3, c.n_points), bool)                                 # the three atoms are far apart: every point is free
    assert np.array_equal(cvc.masks(cvc.key(c))[:3], mask) and L * L == c.info["d2"] and L <= sc.HALF_LINK
    g = sm.grid(x, y, z, r, c.probe)
    assert abs(int(g.cells[0, d // 2]) - int(g.cells[1, d // 2])) == 3 == sm.s_end_of(L, g.h, 99, True)
    assert min(g.s_last(0), g.s_last(1)) >= 3 and sm.margins_hold(x, y, z, r, c.probe)
    _, pairs, mom, _ = cvm.rows(x, y, z, r, mask, c.probe, c.n_points, L, sample=[0, 1])
    _, near, _, _ = cvm.rows(x, y, z, r, mask, c.probe, c.n_points, below, sample=[0, 1])
    ties = np.flatnonzero(pairs > near)
    assert len(ties) >= 2 and (ties < c.n_points).any() and (ties >= c.n_points).any()     # both ends of the tie lose it
    for i in (0, 1):
        mine = slice(i * c.n_points, (i + 1) * c.n_points)
        p, m = cvm.sweep_rows(x, y, z, r, mask, c.probe, c.n_points, L, [i])
        assert np.array_equal(p, pairs[mine]) and np.array_equal(m, mom[mine])
        short = cvm.sweep_rows(x, y, z, r, mask, c.probe, c.n_points, L, [i], reach_shift=-1)[0]
        mine_ties = ties[(ties >= mine.start) & (ties < mine.stop)] - mine.start
        assert (short[mine_ties] < p[mine_ties]).all()


def test_a_cut_without_its_h_loses_the_tie_partner():
    c = cvc.bare_cut()
    x, y, z, r, mask = _one(c)
    off, pairs, mom, dropped, _ = cvc.model(c)
    q = cvm.dots(x, y, z, r, mask, c.probe, 1)[1]
    assert sm.margins_hold(x, y, z, r, c.probe) and mask.all() and pairs.tolist() == [1, 1, 0] and not dropped.any()
    assert float(q[0, 2]) > cvc.BARE_Z + float(F(cvc.BARE_RADIUS)) and q[1, 2] - q[0, 2] == F(0.75)      # rounded up; 0.75 above it
    d = q[1] - q[0]
    assert d[0] * d[0] + d[1] * d[1] + d[2] * d[2] == F(0.75) * F(0.75) and d[0] != 0          # a tie, by rounding
    assert mom[0].tolist() == [9 * ONE // 16, 3 * ONE // 4, 3 * ONE // 4, 0, 0, 0, 0, 0]
    centres = float(np.hypot(float(x[1]) - float(x[0]), float(z[1]) - float(z[0])))
    assert centres > cvc.BARE_RADIUS + 0.0 + cvc.BARE_REACH                                     # beyond R_i + R_j + reach
    for i in (0, 1):
        full = cvm.sweep_rows(x, y, z, r, mask, c.probe, 1, c.reach, [i])[0]
        bare = cvm.sweep_rows(x, y, z, r, mask, c.probe, 1, c.reach, [i], cut_h=False)[0]
        assert full.tolist() == [1] and bare.tolist() == [0]


# ---- curvature_values ----------------------------------------------------------------------------------------------------------------

def test_curvature_values_against_a_per_dot_eigen_solver():
    """Both bounds are derived.  M has the eigenvalues (l1, l2, e), e the one of least magnitude (M n ~ 0); the per-dot
    solver (curvature_model.values) projects M onto the other two eigenvectors and returns l1, l2 themselves.  The closed
    form takes tr = l1 + l2 + e and |M|_F^2 = l1^2 + l2^2 + e^2, so its root is sqrt((l1 - l2)^2 + d) with
    d = e^2 - 2 e (l1 + l2), which lies within |d| / (root + l1 - l2) <= sqrt(|d|) of l1 - l2: each of m1, m2 within
    E = (|e| + sqrt(|d|)) / 2 of l1, l2, and k1 = 3 m1 - m2, k2 = 3 m2 - m1 within 4 E; the mean is the same expression in
    both.  For the order: k1 - tr M = 2 (m1 - m2) >= 0 = tr M - k2 exactly, and tr M is H to the trace identity, whose
    bound of (5 reach + 3) units per pair becomes 2 pairs (5 reach + 3) / Sum(d2) on the ratio.  Float64 roundoff of the
    two solvers: 64 machine epsilons of the scale."""
    c = cvc.reach_case(6.0)
    _, pairs, mom, _, _ = cvc.model(c)
    rows = np.flatnonzero(pairs >= 8)[::7]
    got = np.stack(curvature_values(pairs[rows], mom[rows]), -1)
    want = cvm.values(pairs[rows], mom[rows])
    m = mom[rows].astype(np.float64)
    w = -2.0 / m[:, CURV_D2]
    M = np.empty((len(rows), 3, 3))
    for (i, j), col in zip(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)), (CURV_XX, CURV_YY, CURV_ZZ, CURV_XY, CURV_XZ, CURV_YZ)):
        M[:, i, j] = M[:, j, i] = w * m[:, col]
    val = np.linalg.eigvalsh(M)
    e = val[np.arange(len(rows)), np.argmin(np.abs(val), axis=1)]
    tr = val.sum(axis=1)
    scale = np.abs(val).max(axis=1)
    roundoff = 64 * np.finfo(np.float64).eps * scale
    E = (np.abs(e) + np.sqrt(np.abs(e * e - 2 * e * (tr - e)))) / 2
    err = np.abs(got[:, 2:4] - want[:, 2:4]).max(axis=1)
    print("largest |e| / scale:", (np.abs(e) / scale).max(), "largest |closed form - eigh| / bound:", (err / (4 * E + roundoff)).max())
    assert len(rows) > 50 and (err <= 4 * E + roundoff).all() and (np.abs(got[:, 0] - want[:, 0]) <= roundoff).all()
    mean, gauss, k1, k2, si = got.T
    assert (np.abs(k1 + k2 - 2 * tr) <= 4 * roundoff).all() and (k1 >= k2).all()
    slack = 2 * pairs[rows] * (5 * c.reach + 3) / m[:, CURV_D2] + 4 * roundoff
    assert (k1 + slack >= mean).all() and (mean >= k2 - slack).all()
    assert np.array_equal(gauss, k1 * k2) and (np.abs(si) <= 1).all()
    assert np.array_equal(si, (2 / np.pi) * np.arctan2(k1 + k2, k1 - k2))


def test_directions_with_the_normals_are_tangential_whatever_the_curvatures():
    c = cvc.sphere(960, 3.0)
    _, pairs, mom, _, _ = cvc.model(c)
    n = cvm.normals_of(np.ones((1, 960), bool), 960).astype(np.float64)
    free = curvature_values(pairs, mom, directions=True)
    with_n = curvature_values(pairs, mom, directions=True, normals=3.0 * n)            # (any length: they are normalised)
    assert all(np.array_equal(a, b) for a, b in zip(free[:5], with_n[:5]))
    for d in with_n[5:]:
        assert np.allclose(np.linalg.norm(d, axis=1), 1) and (np.abs((d * n).sum(axis=1)) < 1e-12).all()
    # a parabolic dot, M = diag(1 / 4, 0, 0) with normal z: m2 = 0 ties with the normal's eigenvalue.  With the normal the
    # second direction is y; without it the choice between y and z is not determined
    mom = np.zeros((1, 8), np.int64)
    mom[0, CURV_D2], mom[0, CURV_XX] = 8 * ONE, -ONE
    one = np.ones(1, np.uint32)
    v = curvature_values(one, mom, True, np.array([[0.0, 0.0, 1.0]]))
    assert (float(v[2][0]), float(v[3][0])) == (0.75, -0.25)
    assert np.abs(v[5][0]).tolist() == [1.0, 0.0, 0.0] and np.abs(v[6][0]).tolist() == [0.0, 1.0, 0.0]
    assert abs(curvature_values(one, mom, True)[6][0][0]) == 0.0
    with pytest.raises(ValueError):
        curvature_values(one, mom, True, np.zeros((2, 3)))


def test_curvature_values_on_a_sphere_a_saddle_and_empty_rows():
    c = cvc.sphere(960, 3.0)
    _, pairs, mom, _, _ = cvc.model(c)
    mean, gauss, k1, k2, si, d1, d2 = curvature_values(pairs, mom, directions=True)
    R = 3.2
    assert (si > 0.9).all() and (gauss > 0).all() and np.allclose(mean * R, 1, atol=1e-5)
    n = cvm.normals_of(np.ones((1, 960), bool), 960).astype(np.float64)
    assert np.allclose(np.linalg.norm(d1, axis=1), 1) and np.allclose(np.linalg.norm(d2, axis=1), 1)
    assert (np.abs((d1 * n).sum(axis=1)) < 0.05).all() and (np.abs((d2 * n).sum(axis=1)) < 0.05).all()
    assert (np.abs((d1 * d2).sum(axis=1)) < 1e-9).all()
    # a hand-made saddle: k1 = 1 along x, k2 = -1 along y, normal z; Taubin's m1 = (3 k1 + k2) / 8, m2 = (k1 + 3 k2) / 8
    mom = np.zeros((3, 8), np.int64)
    mom[0, CURV_D2], mom[0, CURV_XX], mom[0, CURV_YY] = 8 * ONE, -ONE, ONE      # M = -2 / 8 diag(-1, 1, 0) = diag(1/4, -1/4, 0)
    mom[2, CURV_H] = 5
    v = curvature_values(np.array([4, 0, 3], np.uint32), mom, directions=True)
    assert [float(a[0]) for a in v[:5]] == [0.0, -1.0, 1.0, -1.0, 0.0]
    assert np.abs(v[5][0]).tolist() == [1.0, 0.0, 0.0] and np.abs(v[6][0]).tolist() == [0.0, 1.0, 0.0]
    assert all(np.isnan(a[1:]).all() for a in v)                          # pairs == 0; Sum(d2) == 0
    assert all(a.dtype == np.float64 for a in v) and curvature_values(np.zeros(0, np.uint32), np.zeros((0, 8), np.int64))[0].shape == (0,)
    for bad in ((np.zeros(3, np.uint32), np.zeros((3, 8), np.uint64)), (np.zeros(3, np.uint32), np.zeros((3, 7), np.int64)),
                (np.zeros(2, np.uint32), np.zeros((3, 8), np.int64))):
        with pytest.raises(ValueError):
            curvature_values(*bad)


# ---- the bindings ---------------------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_and_bound():
    import ctypes as C
    from rustsasa_amd import _capi
    header = open(os.path.join(ROOT, "include", "rustsasa_amd.h")).read()
    for k, name in enumerate(("D2", "H", "XX", "YY", "ZZ", "XY", "XZ", "YZ")):
        assert f"#define RSASA_CURV_{name} {k}\n" in header, name
    assert "#define RSASA_CURV_COLUMNS 8" in header and "#define RSASA_ABI_VERSION 4" in header
    additive = header[header.index("Additive under 4"):header.index("#define RSASA_ABI_VERSION")]
    assert "rsasa_dot_curvature, rsasa_dot_curvature_batch" in additive and "RSASA_CURV_COLUMNS" in additive
    for name, extra in (("rsasa_dot_curvature", 0), ("rsasa_dot_curvature_batch", 1)):
        assert f"int {name}(" in header
        res, args = _capi.SYMBOLS[name]
        assert res is C.c_int and len(args) == 16 + extra and args[-3] is C.c_size_t and args[-7] is C.c_float
    assert _capi.CURV_COLUMNS == 8
    lib = _capi.load()
    assert hasattr(lib, "rsasa_dot_curvature") and hasattr(lib, "rsasa_dot_curvature_batch") and lib.rsasa_abi_version() == 4


class _StubLib:
    """The two entry points as recorders: what Python checks, it checks before it gets here."""
    def __init__(self):
        self.calls = []

    def rsasa_dot_curvature(self, *a):
        self.calls.append(("one", a))
        return 0

    def rsasa_dot_curvature_batch(self, *a):
        self.calls.append(("batch", a))
        return 0


def test_python_argument_rules_need_no_gpu():
    import inspect
    import rustsasa_amd
    for name in ("dot_curvature", "dot_curvature_batch"):
        sig = inspect.signature(getattr(rustsasa_amd.Context, name))
        assert sig.parameters["reach"].default == 3.0 and sig.parameters["n_points"].default == 100
        assert sig.parameters["probe_radius"].default == 1.4
    for name in ("CURV_COLUMNS", "CURV_D2", "CURV_H", "CURV_XX", "CURV_YY", "CURV_ZZ", "CURV_XY", "CURV_XZ", "CURV_YZ",
                 "curvature_values"):
        assert name in rustsasa_amd.__all__, name
    # the rules Python enforces before the C call, on a context without a device
    ctx = rustsasa_amd.Context.__new__(rustsasa_amd.Context)
    ctx._lib, ctx._h = _StubLib(), None
    x = np.arange(4, dtype=F)
    for n_points in (0, -3, 2.5):
        with pytest.raises(ValueError):
            ctx.dot_curvature(x, x, x, x, None, 1.4, n_points)
    with pytest.raises(ValueError):
        ctx.dot_curvature(x[:3], x, x, x)                                               # columns of different lengths
    with pytest.raises(ValueError):
        ctx.dot_curvature(x, x, x, x, np.arange(3, dtype=np.uint64))                    # ids too
    with pytest.raises(ValueError):
        ctx.dot_curvature(x.reshape(2, 2), x, x, x)
    with pytest.raises(ValueError):
        ctx.dot_curvature_batch(x, x, x, x, None, np.array([0, 3], np.uint32))          # the offsets cover 3 atoms of 4
    assert ctx._lib.calls == []                                                         # none of them reached the library
    off, pairs, mom, free, sasa = ctx.dot_curvature(x, x, x, x, None, 1.0, 33, reach=2.5)
    kind, a = ctx._lib.calls[0]
    assert kind == "one" and a[6:10] == (4, 1.0, 33, 2.5) and a[13] == 16 * 4           # n, probe, points, reach; the capacity
    assert off.tolist() == [0] * 5 and pairs.shape == (0,) and mom.shape == (0, 8) and mom.dtype == np.int64
    assert free.shape == sasa.shape == (4,)
    ctx.dot_curvature_batch(x, x, x, x, None, np.array([0, 1, 4], np.uint32))
    kind, a = ctx._lib.calls[1]
    assert kind == "batch" and a[7:11] == (2, 1.4, 100, 3.0) and a[14] == 16 * 4


def test_reach_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "curvature_checks_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "rustsasa_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "curvature_checks_test.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "curvature checks ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-2000:])
