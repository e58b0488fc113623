"""The dot enclosure without a GPU: the model (enclosure_model.py) against a float64 brute force, hand tables, the pinned
distributions of two structures and exact identities; the emulated sweep of k_dot_enclosure with its stop rule and its
two cuts against the model on every case, and a stop rule that forgets R_j on the last-shell case; every input of
enclosure_cases.py pinned to what it is named for; the host helpers against direct loops; the binding table; and
check_enclosure in a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import crowding_cases as cc
import enclosure_cases as ec
import enclosure_model as em
import depth_model as dm
import sweep_cases as sc
import sweep_model as sm

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _part(c, s=0):
    b, e = int(c.so[s]), int(c.so[s + 1])
    return c.x[b:e], c.y[b:e], c.z[b:e], c.r[b:e]


def _model(c, **kw):
    mask = ec.masks(c)
    args = dict(n_dirs=c.n_dirs, reach=c.reach, flags=c.flags)
    args.update(kw)
    off, words = em.blocked_batch(c.x, c.y, c.z, c.r, c.so, mask, c.probe, c.n_points, **args)
    return off, words, mask


# ---- the model -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["corner", "twins"])
def test_model_equals_a_float64_brute_force(name):
    c = ec.of_depth(name, n_points=33, reach=6.0)
    mask = ec.masks(c)
    x, y, z, r = _part(c)
    # The float32 rounding bounds of a decision at reach 6.  Coordinates below 64 carry an ulp of 2^-18 at most: a
    # component of q takes two roundings and dx one more, 1.5 ulp per axis, |delta d| <= sqrt(3) * 1.5 * 2^-18 < 1e-5.
    # t = d . u: |delta t| <= |delta d| |u| + 3 * 2^-24 |d| < 1.3e-5 < T_BAND = 2^-15 for the |d| <= 6 + 3.5 that a hit
    # needs.  v, arm t <= L: d2 carries 2 |d| |delta d| + 3 * 2^-24 d2 < 2.1e-4, t*t carries 2 L |delta t| + 2^-24 L^2
    # < 1.6e-4, the difference 2^-24 of at most 91 more: under 3.8e-4.  Arm t > L: |e| <= 3.5, and e carries delta d and the
    # rounding of L u: under 1e-4.  Where the two models take different arms, |t - L| < 1.3e-5 and the arms differ by
    # (t - L)^2 + L^2 ||u|^2 - 1| < 36 * 2^-21 = 1.8e-5.  In all under 4.1e-4 < V_BAND = 2^-11.  A pair further than
    # L + R_j + 1 from the dot misses by more than 2 (L + R_j) in v, far above any of this.  Dots with a decision inside
    # the bands are left out.
    assert max(np.abs(x).max(), np.abs(y).max(), np.abs(z).max()) < 64 and float(r.max()) + c.probe < 3.5
    assert em.V_BAND == 2.0 ** -11 and em.T_BAND == 2.0 ** -15
    want, firm = em.brute64(x, y, z, r, mask, c.probe, c.n_points, c.n_dirs, c.reach)
    off, got = em.blocked(x, y, z, r, mask, c.probe, c.n_points, c.n_dirs, c.reach)
    assert len(got) == int(off[-1]) == len(firm) and firm.mean() > 0.9
    assert np.array_equal(got[firm], want[firm])
    own = em.own_bits(c.n_points, c.n_dirs)[np.nonzero(mask)[1]]
    assert (got & ~own)[firm].any() and not (got >> np.uint32(c.n_dirs)).any()     # obstacles set bits of their own


def test_hand_table_of_a_lone_atom():
    """One atom, 65 points, 30 directions: every point is free and a word is the own-atom rule, bit m set iff
    u_m . s_k < 0, computed here by a direct loop.  Direction 0 and point 0 are both (0, 0, 1).  Without the obstacle
    bit the words are zero, and the reach plays no part."""
    from oracle import pyoracle as po
    c = ec.of(cc.lone(65))
    off, words, mask = _model(c)
    assert mask.all() and off.tolist() == [0, 65]
    s = np.stack([np.asarray(a, F) for a in po.sphere_points(65)], -1)
    u = np.stack([np.asarray(a, F) for a in po.sphere_points(30)], -1)
    assert s[0].tolist() == [0.0, 0.0, 1.0] and u[0].tolist() == [0.0, 0.0, 1.0]
    want = np.zeros(65, np.uint32)
    for k in range(65):
        for m in range(30):
            if F(F(u[m, 0] * s[k, 0]) + F(u[m, 1] * s[k, 1])) + F(u[m, 2] * s[k, 2]) < 0:
                want[k] |= np.uint32(1) << np.uint32(m)
    assert np.array_equal(words, want) and want.any() and want[0] & 1 == 0
    assert not _model(c, flags=np.array([254], np.uint8))[1].any()
    assert np.array_equal(_model(c, reach=0.0)[1], want)


def test_hand_table_of_two_atoms_on_the_z_axis():
    """Atoms at z = 0 and z = 10 with R = 2 (radius 0.6, probe 1.4) at ONE lattice point and ONE direction, both
    (0, 0, 1): the dots are (0, 0, 2) and (0, 0, 12).  The ray of the first dot meets the second sphere at z = 8, a gap
    of 6: reach 6 stops it (the far end ON the sphere), the float below 6 does not.  The second dot looks away from the
    first atom (t < 0) and is never stopped."""
    x, y, z, r = np.zeros(2, F), np.zeros(2, F), np.array([0, 10], F), np.full(2, 0.6, F)
    mask = np.ones((2, 1), bool)
    assert np.array_equal(np.stack(dm.dots_of(x, y, z, r, mask, 1.4, 1)[1:], -1), [[0, 0, 2], [0, 0, 12]])
    for reach, first in ((6.0, 1), (float(np.nextafter(F(6.0), F(0.0))), 0), (0.0, 0), (7.0, 1), (20.0, 1), (ec.FLT_MAX, 1)):
        off, words = em.blocked(x, y, z, r, mask, 1.4, 1, 1, reach)
        assert off.tolist() == [0, 1, 2] and words.tolist() == [first, 0], reach
    assert em.blocked(x, y, z, r, mask, 1.4, 1, 1, 6.0, flags=[1, 0])[1].tolist() == [0, 0]     # the obstacle bit
    assert em.blocked(x[::-1], y, z[::-1].copy(), r, mask, 1.4, 1, 1, 6.0)[1].tolist() == [0, 1]


def test_cavity_has_sealed_dots_where_the_ball_has_none():
    """Blocked directions of 30 at 100 points and reach 10: min / median / max 13 / 17 / 30 on `cavity` (the dots on the
    internal void are sealed), 13 / 17 / 25 on the solid `ball`."""
    got = {}
    for name in ("cavity", "ball"):
        off, words, _ = _model(ec.of_depth(name))
        n = em.popcount(words)
        got[name] = (len(words), int(n.min()), float(np.median(n)), int(n.max()))
    assert got == {"cavity": (2425, 13, 17.0, 30), "ball": (2391, 13, 17.0, 25)}


def test_or_over_a_split_of_the_obstacles_and_a_permutation():
    c = ec.of_depth("corner", n_points=33)
    off, words, mask = _model(c)
    rng = np.random.default_rng(23)
    part = rng.integers(0, 3, c.n_atoms)
    split = [_model(c, flags=(part == k).astype(np.uint8))[1] for k in range(3)]
    assert np.array_equal(split[0] | split[1] | split[2], words) and all(s.any() for s in split)
    perm = rng.permutation(c.n_atoms)
    p_off, p_words = em.blocked(c.x[perm], c.y[perm], c.z[perm], c.r[perm], mask[perm], c.probe, 33, c.n_dirs, c.reach)
    for new, old in enumerate(perm):
        assert np.array_equal(p_words[int(p_off[new]):int(p_off[new + 1])], words[int(off[old]):int(off[old + 1])])


# ---- the sweep -----------------------------------------------------------------------------------------------------------

def reach_of(h, shells):
    """A reach that the rule admits after `shells` shells and not sooner: (shells - 2.5) h in float32, 0 below that."""
    return float(max(F(shells) - F(2.5), F(0.0)) * F(h))


@pytest.mark.parametrize("shells", cc.REACHES)
def test_stop_shell_at_every_reach(shells):
    h, L = sc.H, reach_of(sc.H, shells)
    met = max(shells, 3)
    assert em.stop_shell(L, h, 40, True) == (met, True)                       # after `met` shells, not sooner
    assert em.stop_shell(float(np.nextafter(F(L), F(np.inf))), h, 40, True) == (met + (shells >= 3), True)
    assert em.stop_shell(L, h, 40, False) == (40, False)                      # no margins: the whole grid
    assert em.stop_shell(L, h, met, True) == (met, False) and em.stop_shell(L, h, 2, True) == (2, False)
    assert em.stop_shell(ec.FLT_MAX, h, 40, True) == (40, False)              # L * L = +inf: never met
    assert em.stop_shell(1e-30, 1e-17, 40, True) == (40, False)               # lim2 below 1e-30: never met
    assert em.stop_shell(L, h, 40, True, early=True)[0] == max(shells - 1, 2)


def _sweep_equals_model(c, sample_size=12, owners=None, **kw):
    off, words, mask = _model(c)
    out = []
    for s in range(len(c.so) - 1):
        b, e = int(c.so[s]), int(c.so[s + 1])
        if e == b:
            continue
        sample = np.sort(np.random.default_rng(7 + s).permutation(e - b)[:sample_size]) if owners is None else owners
        fl = None if c.flags is None else c.flags[b:e]
        got, stop, by_rule, shells = em.sweep_blocked(*_part(c, s), mask[b:e], c.probe, c.n_points, c.n_dirs, c.reach, fl,
                                                      sample, **kw)
        for i in sample:
            assert np.array_equal(got[int(i)], words[int(off[b + i]):int(off[b + i + 1])]), (c.name, s, int(i))
        out.append((stop, by_rule, shells))
    return out


@pytest.mark.parametrize("shells", cc.REACHES)
def test_sweep_with_the_stop_rule_equals_the_model_at_every_reach(shells):
    c = ec.of_depth("cavity", n_points=20, reach=reach_of(sc.H, shells))
    (stop, by_rule, _), = _sweep_equals_model(c)
    assert (stop[by_rule] == max(shells, 3)).all() and by_rule.any()


@pytest.mark.parametrize("name", ["caps", "packed", "last_shell", "prefilter_edge", "cavity"])
def test_sweep_equals_the_model_on_the_cases(name):
    c = {"caps": lambda: ec.of(cc.caps()), "packed": lambda: ec.of(cc.packed(), reach=3.0), "last_shell": ec.last_shell,
         "prefilter_edge": ec.prefilter_edge, "cavity": lambda: ec.of_depth("cavity", n_points=20)}[name]()
    _sweep_equals_model(c)
    _sweep_equals_model(c, sample_size=4, cuts=False)


@pytest.mark.parametrize("name", ["column_z", "slant_xp", "slant_ym", "odd_beside_even"])
def test_sweep_equals_the_model_on_thin_long_and_odd_grids(name):
    d = sc.get(name)
    n_points = sc.points_of(name)[0] if name != "odd_beside_even" else 20
    c = ec.Case(name, d.x, d.y, d.z, d.r, d.so, n_points=n_points, reach=5.0, probe=d.probe)
    out = _sweep_equals_model(c, sample_size=6)
    if name == "odd_beside_even":
        assert out[0][1].any() and not out[1][1].any() and not out[2][1].any()     # odd radii: the whole grid


def test_a_rule_that_forgets_the_obstacles_radius_loses_the_rays_of_the_last_shell():
    c = ec.last_shell()
    off, words, mask = _model(c)
    assert sm.margins_hold(*_part(c), c.probe) and sm.grid(*_part(c), c.probe).h == F(2.0)
    owners = np.array([c.info["hi"], c.info["lo"]])
    assert mask[owners].all()
    (stop, by_rule, shells), = _sweep_equals_model(c, owners=owners)
    assert stop.tolist() == [ec.LAST_SHELL] * 2 and by_rule.all()
    early, e_stop, e_rule, _ = em.sweep_blocked(*_part(c), mask, c.probe, c.n_points, c.n_dirs, c.reach, None, owners,
                                                early=True)
    assert e_stop.tolist() == [ec.LAST_SHELL - 1] * 2 and e_rule.all()
    g = sm.grid(*_part(c), c.probe)
    lost = {int(o): 0 for o in owners}
    for owner, k, m, obstacle in c.info["rays"]:
        n = owners.tolist().index(owner)
        bit = np.uint32(1) << np.uint32(m)
        assert int(np.abs(g.cells[obstacle] - g.cells[owner]).max()) == ec.LAST_SHELL      # its cell lies in shell 5
        assert words[int(off[owner]) + k] & bit                                            # the ray is stopped,
        assert all((per[k] & bit) == 0 for s, per in shells[n].items() if s != ec.LAST_SHELL)   # by shell 5 alone
        assert shells[n][ec.LAST_SHELL][k] & bit
        assert em.own_bits(c.n_points, c.n_dirs)[k] & bit == 0
        without = np.ones(c.n_atoms, np.uint8)
        without[obstacle] = 0
        assert _model(c, flags=without)[1][int(off[owner]) + k] & bit == 0                 # and by that obstacle alone
        assert early[owner][k] & bit == 0
        lost[owner] += 1
    assert sorted(lost.values()) == [3, 3]
    for o in owners:
        want = words[int(off[o]):int(off[o + 1])]
        assert (early[int(o)] & ~want == 0).all() and em.popcount(want).sum() - em.popcount(early[int(o)]).sum() >= 3


# ---- the cases are what they are named for --------------------------------------------------------------------------------

@pytest.mark.parametrize("n", range(len(ec.TIE_KINDS)))
def test_ray_ties_are_exact(n):
    c = ec.ray_ties()
    kind, hit = c.info["kinds"][n], c.info["hit"][n]
    x, y, z, r = _part(c, n)
    s = em.directions(1)[0]
    assert s.tolist() == [0.0, 0.0, 1.0]
    L, p = F(c.reach), F(c.probe)
    R = r + p
    q = x[0] + R[0] * s[0], y[0] + R[0] * s[1], z[0] + R[0] * s[2]
    R2 = R[1] * R[1]
    dx, dy, dz = x[1] - q[0], y[1] - q[1], z[1] - q[2]
    d2 = dx * dx + dy * dy + dz * dz
    t = dx * s[0] + dy * s[1] + dz * s[2]
    perp = d2 - t * t
    ex, ey, ez = dx - L * s[0], dy - L * s[1], dz - L * s[2]
    e2 = ex * ex + ey * ey + ez * ez
    assert all(v.dtype == F for v in (d2, t, perp, e2)) and dy == 0 and R2 == F(2.0 ** -6) and t == dz > 0
    ulp = F(2.0 ** -28)
    if kind == "perp_tie":
        assert dx == R[1] and t < L and perp == R2                       # bit for bit
    elif kind == "perp_miss":
        assert dx == np.nextafter(R[1], F(1)) and t < L and perp == R2 + ulp
    elif kind == "at_L":
        assert dx == R[1] and t == L and perp <= R2 and e2 == R2
    elif kind == "past_L":
        assert dx == R[1] and t == np.nextafter(L, F(np.inf)) and e2 == R2 + ulp and perp <= R2    # only the arm tells
    elif kind == "cap_tie":
        assert dx == 0 and dz == L + R[1] and e2 == R2
    else:
        assert dx == 0 and dz == np.nextafter(L + R[1], F(np.inf)) and e2 > R2
    off, words, mask = _model(c)
    assert mask.all() and off.tolist() == list(range(0, 2 * len(ec.TIE_KINDS) + 1))
    assert words[2 * n] == int(hit) and words[2 * n + 1] == 0            # the obstacle's own dot looks away


def test_prefilter_edge_lies_at_the_cuts_reach():
    c = ec.prefilter_edge()
    off, words, mask = _model(c)
    for s, kind in c.info["cases"]:
        x, y, z, r = _part(c, s)
        b = int(c.so[s])
        assert mask[b + 2].all() and sm.margins_hold(x, y, z, r, c.probe)
        dist = float(np.sqrt((float(x[3]) - float(x[2])) ** 2 + (float(y[3]) - float(y[2])) ** 2 + (float(z[3]) - float(z[2])) ** 2))
        full = c.reach + 2.0 + 2.0                                       # L + R_i + R_j
        assert 0.99 * full <= dist <= full * (1 + 1e-6), (kind, dist)
        assert dist == full if kind == "tie" else (dist < full if kind == "inside" else dist > full)
        word = words[int(off[b + 2])]                                    # dot 0 of the owner, ray 0
        assert word & 1 == (0 if kind == "outside" else 1)
        without = np.ones(c.n_atoms, np.uint8)
        without[b + 3] = 0
        assert _model(c, flags=without)[1][int(off[b + 2])] & 1 == 0     # nothing else stops that ray


def test_non_finite_cases():
    """A NaN obstacle stops no ray: the others' words are those of the structure without it.  Its own dots are stopped
    by no other atom, and their own-atom bits stay as the lattice gives them."""
    for make in (cc.nan_coordinate, cc.nan_radius):
        c = ec.of(make())
        off, words, mask = _model(c)
        a = c.info["atom"]
        assert mask[a].all()
        assert np.array_equal(words[int(off[a]):int(off[a + 1])], em.own_bits(c.n_points, c.n_dirs))
        keep = np.arange(c.n_atoms) != a
        rest = em.blocked(c.x[keep], c.y[keep], c.z[keep], c.r[keep], mask[keep], c.probe, c.n_points, c.n_dirs, c.reach)[1]
        assert np.array_equal(np.delete(words, np.arange(int(off[a]), int(off[a + 1]))), rest) and rest.any()


# ---- the host helpers and the bindings ------------------------------------------------------------------------------------

def test_helpers_against_direct_loops():
    import rustsasa_amd
    from oracle import pyoracle as po
    rng = np.random.default_rng(3)
    for n_dirs in (1, 30, 32):
        top = (1 << n_dirs) - 1
        words = (rng.integers(0, 1 << 32, 40, dtype=np.uint64) & np.uint64(top)).astype(np.uint32)
        words[:2] = (0, top)
        frac = rustsasa_amd.enclosure_fraction(words, n_dirs)
        esc = rustsasa_amd.escape_vectors(words, n_dirs)
        assert frac.dtype == np.float64 and frac.shape == (40,) and esc.dtype == np.float64 and esc.shape == (40, 3)
        u = np.stack([np.asarray(a, np.float32) for a in po.sphere_points(n_dirs)], -1).astype(np.float64)
        for d, w in enumerate(words):
            bits = [(int(w) >> m) & 1 for m in range(n_dirs)]
            assert frac[d] == sum(bits) / n_dirs
            want = np.zeros(3)
            for m in range(n_dirs):
                if not bits[m]:
                    want += u[m]
            assert np.array_equal(esc[d], want)
        assert frac[0] == 0.0 and frac[1] == 1.0 and not esc[1].any()                 # sealed: no way out
    off = np.array([0, 3, 3, 40], np.uint64)
    means = rustsasa_amd.dot_means(off, frac)                                          # dot_means takes a fraction unchanged
    assert means[0] == sum(float(v) for v in frac[:3]) / 3 and np.isnan(means[1])
    for bad in ((words, 0), (words, 33), (words.astype(np.int64), 32), (words.reshape(4, 10), 32), (np.array([2], np.uint32), 1)):
        with pytest.raises(ValueError):
            rustsasa_amd.enclosure_fraction(*bad)
        with pytest.raises(ValueError):
            rustsasa_amd.escape_vectors(*bad)
    assert rustsasa_amd.ENCLOSE_PARTNER == em.PARTNER == 1 and rustsasa_amd.ENCLOSE_MAX_DIRS == em.MAX_DIRS == 32


def test_symbols_are_declared_and_bound():
    import ctypes as C
    from rustsasa_amd import _capi
    header = open(os.path.join(ROOT, "include", "rustsasa_amd.h")).read()
    assert "#define RSASA_ENCLOSE_PARTNER 1" in header and "#define RSASA_ENCLOSE_MAX_DIRS 32" in header
    assert "#define RSASA_ABI_VERSION 4" in header and _capi.ENCLOSE_MAX_DIRS == 32
    assert "RSASA_ENCLOSE_MAX_DIRS, rsasa_dot_enclosure, rsasa_dot_enclosure_batch. */" in header    # additive under 4
    assert "rsasa_dot_enclosure*: for out_blocked" in header
    for name, extra in (("rsasa_dot_enclosure", 0), ("rsasa_dot_enclosure_batch", 1)):
        assert f"int {name}(" in header
        res, args = _capi.SYMBOLS[name]
        assert res is C.c_int and len(args) == 17 + extra and args[-3] is C.c_size_t
        assert args[10 + extra] is C.c_float and args[11 + extra] is C.c_uint32       # reach, n_dirs
    lib = _capi.load()
    assert hasattr(lib, "rsasa_dot_enclosure") and hasattr(lib, "rsasa_dot_enclosure_batch")


def test_reach_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "enclosure_checks_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "rustsasa_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "enclosure_checks_test.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "enclosure checks ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-2000:])
