"""The dot fields without a GPU: the model (fields_model.py) against a float64 sum under a derived bound, under a
permutation of the atoms, on two hand tables and against the crowding model as a witness (all-ones weights under STEP are
2^24 times the number of partners within the cutoff); the rule that skips a term; exact ties at the cutoff; the emulated
sweep of k_dot_fields with its stop rule against the model, and one shell early on the last-shell cases; a sum that
wraps; the dots per atom that run every lane layout; field_values against a direct loop; the binding table; and
check_fields in a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import crowding_cases as cc
import crowding_model as cm
import depth_model as dm
import fields_cases as fc
import fields_model as fm
import sweep_model as sm
from rustsasa_amd import (FIELD_INV_1PD, FIELD_INV_D, FIELD_INV_D2, FIELD_MAX_CHANNELS, FIELD_PARTNER, FIELD_STEP,
                          field_values)

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 24


def _part(c, s=0):
    b, e = int(c.so[s]), int(c.so[s + 1])
    return c.x[b:e], c.y[b:e], c.z[b:e], c.r[b:e]


def test_constants_are_the_models():
    assert (FIELD_STEP, FIELD_INV_D, FIELD_INV_D2, FIELD_INV_1PD) == fm.KINDS == (0, 1, 2, 3)
    assert FIELD_MAX_CHANNELS == fm.MAX_CHANNELS == 4 and FIELD_PARTNER == fm.PARTNER == 1


# ---- the model -----------------------------------------------------------------------------------------------------------

def test_model_stays_within_the_derived_bound_of_a_float64_sum():
    """300 random dots against 400 random atoms, every kind.  The bound is derived, not measured: a term takes at most
    eight float32 roundings (three differences, the sum of squares counted as three, the root, the quotient or the sum
    under it, the product - each 2^-24 relative at most), and the fixed point adds half a unit, 2^-25, per term:
        |sums * 2^-24 - sum t64| <= 8 * 2^-24 * sum |t64| + n * 2^-25.
    Dots with a partner within 1e-4 A of the cutoff are left out (float32 may decide the hit the other way)."""
    rng = np.random.default_rng(21)
    n_dots, n_atoms, cutoff = 300, 400, 10.0
    q = rng.uniform(-12.0, 12.0, (n_dots, 3)).astype(F)
    x, y, z = (np.ascontiguousarray(a) for a in rng.uniform(-12.0, 12.0, (3, n_atoms)).astype(F))
    w = fc.weights(n_atoms, 4, 22)
    par = np.arange(n_atoms)
    got = fm.values(fm.rows_of(q[:, 0], q[:, 1], q[:, 2], x, y, z, par, w, fc.ALL_KINDS, fm.c2_of(cutoff)))
    total, absolute, n, band = fm.brute64(q[:, 0], q[:, 1], q[:, 2], x, y, z, par, w, fc.ALL_KINDS, cutoff)
    far = band > 1e-4
    assert far.mean() > 0.9 and n[far].min() >= 1
    bound = 8 * 2.0 ** -24 * absolute + n[:, None] * 2.0 ** -25
    share = np.abs(got - total)[far] / bound[far]
    print("largest share of the bound, per kind:", share.max(axis=0))
    assert (share <= 1.0).all()


def test_model_is_unchanged_under_a_permutation_of_the_atoms():
    f = fc.of(cc.of_depth("corner", n_points=33, edges=(3.0, 5.5, 9.0), flags=cc.random_flags(60, 5)))
    off, rows, mask = fc.model(f)
    perm = np.random.default_rng(8).permutation(f.n_atoms)
    x, y, z, r = (a[perm] for a in _part(f))
    p_off, p_rows = fm.sums(x, y, z, r, mask[perm], f.probe, f.n_points, f.weights[perm], f.kinds, f.cutoff, f.flags[perm])
    assert rows.any(axis=0).all()
    for new, old in enumerate(perm):                        # the dots of an atom keep their order; the atoms moved
        assert np.array_equal(p_rows[int(p_off[new]):int(p_off[new + 1])], rows[int(off[old]):int(off[old + 1])])


def test_hand_table_of_a_lone_atom():
    """One atom of radius 1.7 at probe 1.4: R = 3.1, every point free, and the only partner of any dot is the owner at
    d2 = R^2 up to the roundings of q: weight 1 gives 2^24 under STEP, and 1 / 3.1, 1 / 9.61 and 1 / 4.1 within 2e-6
    under the other kinds.  Without its partner bit the rows are zero."""
    c = cc.lone(65)
    f = fc.of(c, w=np.ones((1, 4)))
    off, rows, mask = fc.model(f)
    assert mask.all() and off.tolist() == [0, 65] and rows.shape == (65, 4)
    assert (rows[:, 0] == ONE).all()
    assert np.abs(fm.values(rows[:, 1:]) - np.array([1 / 3.1, 1 / 9.61, 1 / 4.1])).max() < 2e-6
    _, none, _ = fc.model(f, flags=np.array([254], np.uint8))
    assert none.shape == (65, 4) and not none.any()


def test_hand_table_of_two_atoms_on_an_axis():
    """Atoms at z = 0 and z = 10 with R = 2 at ONE lattice point, (0, 0, 1): the dots are (0, 0, 2) and (0, 0, 12), and
    every distance is exact - dot 0 has its owner at 2 and the other atom at 8, dot 1 its owner at 2 and the other at 12,
    beyond the cutoff 10.  Weights 1 and -0.5.  Dot 0: STEP 1 - 0.5; INV_D 1/2 - 0.5/8; INV_D2 1/4 - 0.5/64; INV_1PD
    rint(fl(1/3) 2^24) + rint(-0.5 fl(1/9) 2^24) with fl(1/3) = 11184811 * 2^-25 - a tie, which goes to the even
    5592406 - and fl(1/9) = 14913081 * 2^-27, -932067.5625 -> -932068.  Dot 1: -0.5 times 1, 1/2, 1/4 and fl(1/3)."""
    x, y, z, r = np.zeros(2, F), np.zeros(2, F), np.array([0, 10], F), np.full(2, 0.6, F)
    mask = np.ones((2, 1), bool)
    assert np.array_equal(np.stack(dm.dots_of(x, y, z, r, mask, 1.4, 1)[1:], -1), [[0, 0, 2], [0, 0, 12]])
    w = np.array([[1.0] * 4, [-0.5] * 4], F)
    off, rows = fm.sums(x, y, z, r, mask, 1.4, 1, w, fc.ALL_KINDS, 10.0)
    assert off.tolist() == [0, 1, 2]
    assert rows[0].tolist() == [ONE // 2, 7 * ONE // 16, 31 * ONE // 128, 5592406 - 932068]
    assert rows[1].tolist() == [-ONE // 2, -ONE // 4, -ONE // 8, -2796203]      # -0.5 fl(1/3) 2^24 = -2796202.75
    at_12 = fm.sums(x, y, z, r, mask, 1.4, 1, w, fc.ALL_KINDS, 12.0)[1]          # a tie at the cutoff: the other atom counts
    assert at_12[1, 0] == ONE // 2 and at_12[0].tolist() == rows[0].tolist()
    only = fm.sums(x, y, z, r, mask, 1.4, 1, w, fc.ALL_KINDS, 10.0, flags=[0, 1])[1]
    assert only[0].tolist() == [-ONE // 2, -ONE // 16, -ONE // 128, -932068] and only[1].tolist() == rows[1].tolist()


@pytest.mark.parametrize("name", sorted(fc.crowding_names()))
def test_all_ones_under_step_is_the_crowding_count_at_that_edge(name):
    """The witness: weight 1 and STEP add 2^24 per partner within the cutoff - 2^24 times the cumulative count of the
    crowding model at the last edge, on every case."""
    c = fc.crowding_names()[name]()
    f = fc.of(c, kinds=(fm.STEP,), w=np.ones((c.n_atoms, 1)))
    off, rows, mask = fc.model(f)
    c_off, c_rows = cm.counts_batch(c.x, c.y, c.z, c.r, c.so, mask, c.probe, c.n_points, c.edges, c.flags)
    assert np.array_equal(off, c_off)
    assert np.array_equal(rows[:, 0], c_rows.sum(axis=1).astype(np.int64) * ONE)
    for edge in c.edges[:-1]:                                    # and at the inner edges, as cutoffs of their own
        inner = fc.model(fc.of(c, kinds=(fm.STEP,), w=np.ones((c.n_atoms, 1)), cutoff=edge))[1]
        e2 = cm.e2_of(c.edges)
        k = int(np.searchsorted(e2, cm.e2_of([edge])[0], side="right"))
        assert np.array_equal(inner[:, 0], c_rows[:, :k].sum(axis=1).astype(np.int64) * ONE)


# ---- the rule that skips a term ---------------------------------------------------------------------------------------------

def test_a_term_of_2_to_the_24_counts_and_the_next_float_does_not():
    assert fm.fixed(np.array([fc.BOUND, -fc.BOUND], F)).tolist() == [1 << 48, -(1 << 48)]
    assert fm.fixed(np.array([fc.ABOVE, -fc.ABOVE], F)).tolist() == [0, 0] and fc.ABOVE == 2.0 ** 24 + 2.0
    assert fm.fixed(np.array([np.nan, np.inf, -np.inf], F)).tolist() == [0, 0, 0]
    # ties go to the even: 2^-25 is half a unit -> 0, 3 * 2^-25 -> 2; the smallest subnormal -> 0; t * 2^24 is exact
    assert fm.fixed(np.array([2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -149, 2.0 ** -24, -(2.0 ** -25)], F)).tolist() == [0, 2, 0, 1, 0]


def test_special_weights_add_what_the_rule_says():
    f = fc.special_weights()
    off, rows, mask = fc.model(f)
    clean = f.weights.copy()
    with np.errstate(invalid="ignore"):
        clean[~(np.abs(clean) <= F(fc.BOUND))] = 0.0          # what adds nothing, taken out by hand
    assert (clean[:, 0] == fc.BOUND).sum() == 2 and (clean[:, 0] == -fc.BOUND).sum() == 2
    assert (np.abs(f.weights[:, 1]) > fc.BOUND).sum() == 4 and not np.isfinite(f.weights[:, 2]).all()
    want = fc.model(fc.FCase(f.c, clean, f.kinds, f.cutoff))[1]
    assert np.array_equal(rows, want) and rows.any(axis=0).all()
    dropped = clean.copy()
    dropped[np.abs(dropped[:, 0]) == F(fc.BOUND), 0] = 0.0        # the terms of +-2^24 do count: without them the sums differ
    assert (np.abs(rows[:, 0] - fc.model(fc.FCase(f.c, dropped, f.kinds, f.cutoff))[1][:, 0]) >= 1 << 48).any()
    assert (rows[:, 3] == 2).any() and set(np.unique(rows[:, 3]).tolist()) <= {0, 2}


@pytest.mark.parametrize("edge0", [0.0, 1e-30])
def test_a_coincident_partner_counts_where_its_factor_is_finite(edge0):
    """tie_zero: a partner exactly ON the owner's dot, d2 = 0.  g is 1 under STEP and under INV_1PD (1 / (1 + 0)), and
    the term counts; it is +inf under INV_D and INV_D2, the term is infinite (NaN for a weight of 0) and adds nothing.
    With the cutoff 0 (and one whose square underflows to 0) d2 = 0 is the only hit."""
    c = cc.tie_zero(edge0)
    w = np.zeros((2, 4), F)
    w[1] = 3.0
    f = fc.of(c, w=w, cutoff=edge0)
    assert fm.c2_of(edge0) == 0
    off, rows, mask = fc.model(f)
    assert mask[0].all() and mask[1].all()
    assert rows[cc.TIE_DOT].tolist() == [3 * ONE, 0, 0, 3 * ONE]
    assert not np.delete(rows[:65], cc.TIE_DOT, axis=0).any()          # no other dot of the owner has d2 = 0
    zero = fc.model(fc.of(c, w=np.zeros((2, 4)), cutoff=edge0))[1]      # 0 * inf = NaN: nothing
    assert not zero.any()


def test_ties_at_the_cutoff_gain_or_lose_the_partners_term():
    last, below = fc.of(cc.tie("last"), seed=3), fc.of(cc.tie("below"), seed=3)
    assert np.nextafter(F(last.cutoff), F(0)) == F(below.cutoff)
    (off, rows, mask), (_, b_rows, _) = fc.model(last), fc.model(below)
    d = int(mask[0, :cc.TIE_DOT].sum())
    xyz, r, q, e = cc.tie_geometry()
    g = fm.factors(e * e)
    term = np.array([fm.fixed(last.weights[1, k] * g[kind])[()] for k, kind in enumerate(last.kinds)])
    assert term.all() and np.array_equal(rows[d] - b_rows[d], term)     # the partner's term, and nothing else
    keep = np.arange(len(rows)) != d
    assert np.array_equal(rows[keep][:65 - 1], b_rows[keep][:65 - 1])   # the owner's other dots are further away


# ---- the sweep -----------------------------------------------------------------------------------------------------------

def _sweep_equals_model(f, sample_size=10):
    off, rows, mask = fc.model(f)
    for s in range(len(f.so) - 1):
        b, e = int(f.so[s]), int(f.so[s + 1])
        if e == b:
            continue
        sample = np.sort(np.random.default_rng(7 + s).permutation(e - b)[:sample_size])
        fl = None if f.flags is None else f.flags[b:e]
        got, stop, by_rule, _ = fm.sweep_sums(*_part(f, s), mask[b:e], f.probe, f.n_points, f.weights[b:e], f.kinds, f.cutoff,
                                              fl, sample)
        for i in sample:
            assert np.array_equal(got[int(i)], rows[int(off[b + i]):int(off[b + i + 1])]), (f.name, s, int(i))


@pytest.mark.parametrize("name", ["caps", "packed", "pair", "corner"])
def test_sweep_equals_the_model_on_the_cases(name):
    c = {"caps": cc.caps, "packed": cc.packed, "pair": lambda: cc.pair(65), "corner": lambda: cc.corner(33)}[name]()
    _sweep_equals_model(fc.of(c))


@pytest.mark.parametrize("shell", cc.LAST_SHELLS)
def test_one_shell_early_loses_the_tie_partners_terms(shell):
    c = cc.last_shell(shell)
    f = fc.of(c, kinds=(fm.STEP, fm.INV_D), w=np.ones((c.n_atoms, 2)))
    off, rows, mask = fc.model(f)
    assert sm.margins_hold(*_part(c), c.probe) and sm.grid(*_part(c), c.probe).h == F(2.0)
    owners = np.array([c.info["hi"], c.info["lo"]])
    args = (*_part(c), mask, c.probe, c.n_points, f.weights, f.kinds, f.cutoff, None, owners)
    good, stop, by_rule, found = fm.sweep_sums(*args)
    assert stop.tolist() == [shell] * 2 and by_rule.all() and all(shell in s for s in found)
    early, e_stop, _, _ = fm.sweep_sums(*args, early=True)
    assert e_stop.tolist() == [shell - 1] * 2
    lost = 0
    for o in owners:
        want = rows[int(off[o]):int(off[o + 1])]
        assert np.array_equal(good[int(o)], want)
        assert (early[int(o)] <= want).all()                               # (the weights are positive)
        lost += int((want[:, 0] - early[int(o)][:, 0]).sum()) // ONE
    assert lost >= 6                                                       # three leaning directions of each owner


# ---- a sum that wraps ------------------------------------------------------------------------------------------------------

def test_2_to_the_15_and_one_terms_of_2_to_the_24_wrap():
    n = (1 << 15) + 1
    x = np.linspace(0.0, 1.0, n).astype(F)
    zero = np.zeros(n, F)
    w = np.full((n, 1), fc.BOUND, F)
    q = np.array([0.5], F), np.array([2.0], F), np.array([0.0], F)
    row = fm.rows_of(*q, x, zero, zero, np.arange(n), w, (fm.STEP,), fm.c2_of(5.0))
    assert row.tolist() == [[-(1 << 63) + (1 << 48)]] == [[fc.wrapped(n)]]
    assert fm.rows_of(*q, x, zero, zero, np.arange(n - 1), w, (fm.STEP,), fm.c2_of(5.0)).tolist() == [[-(1 << 63)]]
    assert fm.rows_of(*q, x, zero, zero, np.arange(n - 2), w, (fm.STEP,), fm.c2_of(5.0)).tolist() == [[(1 << 63) - (1 << 48)]]


def test_the_wrap_ball_is_accepted_and_wraps():
    """33 000 atoms in a ball of 3 A: the oracle takes the structure (its grid is some twenty cells per axis), it has
    accessible dots at one lattice point, and every dot's sum is 33 000 * 2^48 wrapped."""
    f = fc.wrap_ball()
    off, rows, mask = fc.model(f)
    assert f.n_atoms == fc.WRAP_ATOMS == 33000 > 1 << 15 and mask.shape == (33000, 1) and 16 <= mask.sum() < 33000
    d = np.sqrt(f.x.astype(np.float64) ** 2 + f.y ** 2 + f.z ** 2)
    assert d.max() <= fc.WRAP_BALL + 1e-3 and 2 * (fc.WRAP_BALL + f.r.max() + f.probe) < fc.WRAP_CUTOFF
    assert fc.wrapped(33000) < 0 and (rows == fc.wrapped(33000)).all() and len(rows) == int(mask.sum())


# ---- the cases run every lane layout -----------------------------------------------------------------------------------------

def test_corner_and_caps_have_atoms_of_every_lane_layout():
    """A pass of n <= 32 dots runs on P = 1, 2, 4, 8, 16 or 32 lanes, one of 33 to 64 on 64, one of 65 or more gives
    lanes a second dot: corner(100) with caps() has atoms of 0, 1, 2, 3-4, 5-8, 9-16, 17-32, 33-64 and 65 dots."""
    free = np.concatenate([cc.masks(cc.corner(100)).sum(axis=1), cc.masks(cc.caps()).sum(axis=1)])
    for lo, hi in ((0, 0), (1, 1), (2, 2), (3, 4), (5, 8), (9, 16), (17, 32), (33, 64), (65, 65)):
        assert ((free >= lo) & (free <= hi)).any(), (lo, hi)


# ---- the host helpers and the bindings ------------------------------------------------------------------------------------

def test_field_values_against_a_direct_loop():
    rng = np.random.default_rng(3)
    s = rng.integers(-(1 << 52), 1 << 52, (37, 3)).astype(np.int64)
    s[0] = [0, 1, -1]
    s[1] = [1 << 24, -(1 << 24), (1 << 24) + 1]
    got = field_values(s)
    assert got.dtype == np.float64 and got.shape == s.shape
    for i in range(s.shape[0]):
        for c in range(s.shape[1]):
            assert got[i, c] == int(s[i, c]) / 16777216.0
    assert got[1].tolist() == [1.0, -1.0, 1.0 + 2.0 ** -24] and np.array_equal(got, fm.values(s))
    assert field_values(np.zeros((0, 2), np.int64)).shape == (0, 2)
    with pytest.raises(ValueError):
        field_values(s.astype(np.uint32))


def test_symbols_are_declared_and_bound():
    import ctypes as C
    from rustsasa_amd import _capi
    header = open(os.path.join(ROOT, "include", "rustsasa_amd.h")).read()
    for line in ("#define RSASA_FIELD_PARTNER 1", "#define RSASA_FIELD_MAX_CHANNELS 4", "#define RSASA_FIELD_STEP 0",
                 "#define RSASA_FIELD_INV_D 1", "#define RSASA_FIELD_INV_D2 2", "#define RSASA_FIELD_INV_1PD 3",
                 "#define RSASA_ABI_VERSION 4"):
        assert line in header, line
    additive = header[header.index("Additive under 4"):header.index("#define RSASA_ABI_VERSION")]
    assert "rsasa_dot_fields, rsasa_dot_fields_batch" in additive and "RSASA_FIELD_MAX_CHANNELS" in additive
    for name, extra in (("rsasa_dot_fields", 0), ("rsasa_dot_fields_batch", 1)):
        assert f"int {name}(" in header
        res, args = _capi.SYMBOLS[name]
        assert res is C.c_int and len(args) == 19 + extra and args[-3] is C.c_size_t and args[-6] is C.c_float
        assert args[-7] is C.c_uint32
    assert _capi.FIELD_MAX_CHANNELS == 4
    lib = _capi.load()
    assert hasattr(lib, "rsasa_dot_fields") and hasattr(lib, "rsasa_dot_fields_batch") and lib.rsasa_abi_version() == 4


def test_python_argument_rules_need_no_gpu():
    import rustsasa_amd
    assert hasattr(rustsasa_amd.Context, "dot_fields") and hasattr(rustsasa_amd.Context, "dot_fields_batch")
    for name in ("FIELD_STEP", "FIELD_INV_D", "FIELD_INV_D2", "FIELD_INV_1PD", "FIELD_PARTNER", "FIELD_MAX_CHANNELS",
                 "field_values"):
        assert name in rustsasa_amd.__all__, name


def test_channel_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "fields_checks_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "rustsasa_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "fields_checks_test.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "fields checks ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-2000:])
