"""The half-sphere exposure without a GPU: the model (hse_model.py) against a float64 brute force and against counts
worked out by hand, every case of hse_cases.py pinned to what it is named for with the cell arithmetic of
sweep_model.py, the emulated sweep of k_half_sphere (its stop rule included) against the plain model,
pseudo_cb_directions against a direct loop, the binding table, and check_cutoff in a stand-alone program under the
address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import hse_cases as hc
import hse_model as hm
import sweep_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BAND = 1e-4
SEEDS = (100, 102, 103, 104, 107, 108)   # chosen so that no pair lies within BAND of a cutoff or of a centre's plane
CUTOFFS64 = (3.5, 6.0, 13.0)


def _small_cluster(seed, n=60):
    xyz = np.random.default_rng(seed).uniform(0.0, 20.0, (n, 3)).astype(F)
    return xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy(), hc.random_dirs(n, seed + 1)


# ---- the model ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_model_equals_a_float64_brute_force(seed):
    x, y, z, dirs = _small_cluster(seed)
    rng = np.random.default_rng(seed + 2)
    for flags in (None, rng.integers(0, 4, len(x)).astype(np.uint8)):
        for cutoff in CUTOFFS64:
            up, down, band, side_band = hm.brute64(x, y, z, dirs, flags, cutoff)
            assert band > BAND and side_band > BAND, (cutoff, band, side_band)   # zero pairs in the band: none is left out
            got = hm.counts(x, y, z, dirs, flags, cutoff)
            assert np.array_equal(got[0], up) and np.array_equal(got[1], down), cutoff
            assert (up + down).sum() > 0


def test_hand_cases():
    c = hc.hand()
    up, down = hm.counts(c.x, c.y, c.z, c.dirs, c.flags, c.info["cutoff"])
    assert up.tolist() == c.info["up"] and down.tolist() == c.info["down"]
    # two atoms 3 apart on x: at cutoff 3 each counts the other, on the side its direction says; at 2.9 nobody counts
    x, y, z = np.array([0, 3], F), np.array([1, 1], F), np.array([-2, -2], F)
    dirs = np.array([[1, 0, 0], [1, 0, 0]], F)
    assert [a.tolist() for a in hm.counts(x, y, z, dirs, None, 3.0)] == [[1, 0], [0, 1]]
    assert [a.tolist() for a in hm.counts(x, y, z, dirs, None, 2.9)] == [[0, 0], [0, 0]]
    assert [a.tolist() for a in hm.counts(x, y, z, None, None, 3.0)] == [[1, 1], [0, 0]]            # no dirs: all up
    # three atoms on a line at 0, 3, 7: cutoff 4 links the neighbours only, cutoff 7 all; a partner-only atom gets 0 / 0
    x, y, z = np.array([0, 3, 7], F), np.zeros(3, F), np.zeros(3, F)
    dirs = np.array([[-1, 0, 0], [2, 0, 0], [0, 1, 0]], F)
    assert [a.tolist() for a in hm.counts(x, y, z, dirs, None, 4.0)] == [[0, 1, 1], [1, 1, 0]]
    assert [a.tolist() for a in hm.counts(x, y, z, dirs, None, 7.0)] == [[0, 1, 2], [2, 1, 0]]
    assert [a.tolist() for a in hm.counts(x, y, z, dirs, [3, 1, 2], 7.0)] == [[0, 0, 2], [1, 0, 0]]
    # a NaN direction sends everybody down; a NaN coordinate counts for nobody and gets 0 / 0
    dirs[1, 2] = np.nan
    assert [a.tolist() for a in hm.counts(x, y, z, dirs, None, 7.0)] == [[0, 0, 2], [2, 2, 0]]
    x[2] = np.nan
    assert [a.tolist() for a in hm.counts(x, y, z, dirs, None, 7.0)] == [[0, 0, 0], [1, 1, 0]]
    # c2 = +inf: every atom whose d2 is no NaN counts
    assert [a.tolist() for a in hm.counts(x, y, z, None, None, float(np.finfo(F).max))] == [[1, 1, 0], [0, 0, 0]]


def test_exact_ties_count_and_one_ulp_further_does_not():
    t, m = hc.ties(), hc.ties(True)
    assert all(float(v) == int(v) for a in (t.x, t.y, t.z) for v in a) and t.x[0] != 0 and t.y[0] != 0 and t.z[0] != 0
    d = np.stack([t.x - t.x[0], t.y - t.y[0], t.z - t.z[0]], -1)[1:]
    assert np.array_equal(d, np.array(hc.TIE_OFFSETS, F)) and np.all((d.astype(np.float64) ** 2).sum(1) == 169.0)
    assert [a.tolist() for a in hm.counts(t.x, t.y, t.z, t.dirs, t.flags, 13.0)] == [[3, 0, 0, 0], [0, 0, 0, 0]]
    # one coordinate of each partner differs by one ulp, away from the centre
    diff = [(k, a) for k in range(4) for a, (p, q) in enumerate(((t.x, m.x), (t.y, m.y), (t.z, m.z))) if p[k] != q[k]]
    assert diff == [(1, 0), (2, 1), (3, 2)]
    for k, a in diff:
        p, q, o = ((t.x, m.x), (t.y, m.y), (t.z, m.z))[a][0][k], ((t.x, m.x), (t.y, m.y), (t.z, m.z))[a][1][k], hc.TIE_ORIGIN[a]
        assert abs(float(q) - o) > abs(float(p) - o) and q in (np.nextafter(p, F(np.inf)), np.nextafter(p, F(-np.inf)))
    assert [a.tolist() for a in hm.counts(m.x, m.y, m.z, m.dirs, m.flags, 13.0)] == [[0, 0, 0, 0], [0, 0, 0, 0]]


# ---- the cases are what they are named for -------------------------------------------------------------------------------

def test_cluster_and_its_variants():
    c = hc.cluster()
    assert c.n_atoms == hc.N_CLUSTER and sm.margins_hold(c.x, c.y, c.z, c.r, c.probe)
    g = sm.grid(c.x, c.y, c.z, c.r, c.probe)
    assert g.h == F(1.4) + F(1.88) and g.dims.min() >= 11
    xyz = np.stack([c.x, c.y, c.z], -1).astype(np.float64)
    diam = np.linalg.norm(xyz.max(0) - xyz.min(0))
    assert diam < hc.COVER                                          # COVER covers the grid: everybody counts for everybody
    cut = hc.cluster_cutoffs()
    assert cut[0] == 0.0 and cut[-1] == float(np.finfo(F).max) and not np.isfinite(hm.c2_of(cut[-1]))
    mid = int(np.argmin(np.linalg.norm(xyz - xyz.mean(0), axis=1)))
    stops = [hm.stop_shell(C, g.h, g.s_last(mid), True) for C in cut]
    # the middle atom: the rule stops it after shells 1, 1, 2, 3, 4, 5; the last two cutoffs sweep the whole grid
    assert stops[:6] == [(1, True), (1, True), (2, True), (3, True), (4, True), (5, True)], stops
    assert stops[6] == stops[7] == (g.s_last(mid), False)
    assert (2 * 4 + 1) ** 2 > sm.WAVE                               # a shell of more than 64 rows from s = 4 on
    up, down = hm.counts(c.x, c.y, c.z, c.dirs, None, hc.COVER)
    assert np.all(up + down == c.n_atoms - 1)
    # one radius of 70 / one NaN coordinate: the margins fail, the whole grid is swept
    o, n = hc.odd_radius(), hc.nan_atom()
    assert not sm.margins_hold(o.x, o.y, o.z, o.r, o.probe) and sm.odd_input(o.x, o.y, o.z, o.r)
    assert not sm.margins_hold(n.x, n.y, n.z, n.r, n.probe) and np.isnan(n.y[n.info["atom"]])
    up, down = hm.counts(n.x, n.y, n.z, n.dirs, None, hc.COVER)
    a = n.info["atom"]
    assert up[a] == down[a] == 0 and np.all(np.delete(up + down, a) == n.n_atoms - 2)


def test_crowd_has_a_run_of_more_than_64_atoms():
    c = hc.crowd()
    g = sm.grid(c.x, c.y, c.z, c.r, c.probe)
    per_cell = np.diff(g.starts)
    assert per_cell.max() >= 200 and sm.margins_hold(c.x, c.y, c.z, c.r, c.probe)
    i = int(g.order[g.starts[int(np.argmax(per_cell))]])           # an atom of the crowded cell
    steps, longest = sm.shell_steps(g, i, 0)
    assert longest >= 200 and len(steps[0]) > 3 * sm.WAVE            # shell 0: one run, four trips of the atom loop
    s, by_rule = hm.stop_shell(13.0, g.h, g.s_last(i), True)
    assert (s, by_rule) == (5, True) and len(sm.shell_steps(g, i, 5)[0]) == 2    # 121 rows: two steps


def test_edge_partners_lie_in_the_last_swept_and_the_first_unswept_shell():
    c = hc.edge()
    info = c.info
    g = sm.grid(c.x, c.y, c.z, c.r, c.probe)
    assert g.h == F(2.0) and sm.margins_hold(c.x, c.y, c.z, c.r, c.probe)
    hi, lo = info["hi"], info["lo"]
    # hi: one ulp under the upper boundary of its cell on every axis; lo: on the lower boundary of its cell
    for k, a in enumerate((c.x, c.y, c.z)):
        assert g.cells[hi][k] == 20 and int((np.nextafter(a[hi], F(np.inf)) + F(2.0)) * F(0.5)) == 21
        assert g.cells[lo][k] == 11 and int((np.nextafter(a[lo], F(-np.inf)) + F(2.0)) * F(0.5)) == 10
    for centre, lean in ((hi, 1), (lo, -1)):
        assert hm.stop_shell(hc.EDGE_CUTOFF, g.h, g.s_last(centre), True) == (3, True)
        lim = (F(3) - F(0.5)) * g.h
        assert lim * lim == hm.c2_of(hc.EDGE_CUTOFF)                 # the rule is met with equality
        for j, axis, sign in info["tie"][centre]:
            d = [a[j] - a[centre] for a in (c.x, c.y, c.z)]
            assert d[axis] == F(5.0 * sign) and sum(abs(float(v)) for v in d) == 5.0      # d2 == c2 exactly
            assert sm.position_class(g, centre, j)[0] == (3 if sign == lean else 2)      # 3: the last swept shell
        for j, axis, sign in info["far"][centre]:
            assert sm.position_class(g, centre, j)[0] == (4 if sign == lean else 3)      # 4: the first unswept shell
    up, down = hm.counts(c.x, c.y, c.z, c.dirs, None, hc.EDGE_CUTOFF)
    assert up[hi] + down[hi] == 6 and up[lo] + down[lo] == 6
    # the emulated sweep finds all six, three of them in shell 3; a rule that stops a shell earlier loses those three
    su, sd, stop, by_rule, found = hm.sweep_counts(*c.cols[:4], c.probe, c.dirs, None, hc.EDGE_CUTOFF, [hi, lo])
    assert np.array_equal(su + sd, [6, 6]) and found == [[2, 3], [2, 3]] and by_rule.all()
    assert np.array_equal(su, up[[hi, lo]]) and np.array_equal(sd, down[[hi, lo]])
    su, sd, stop, *_ = hm.sweep_counts(*c.cols[:4], c.probe, c.dirs, None, hc.EDGE_CUTOFF, [hi, lo], half=-0.5)
    assert np.array_equal(stop, [2, 2]) and np.array_equal(su + sd, [3, 3])
    # one ulp above the cutoff the rule is met a shell later
    assert hm.stop_shell(float(np.nextafter(F(hc.EDGE_CUTOFF), F(np.inf))), g.h, g.s_last(hi), True) == (4, True)


def test_batches():
    c = hc.interleaved()
    assert c.so.tolist() == [0, 1000, 2000]
    one = hm.counts(c.x, c.y, c.z, c.dirs, None, 13.0)
    two = hm.counts_batch(c.x, c.y, c.z, c.so, c.dirs, None, 13.0)
    assert np.all(two[0] + two[1] < one[0] + one[1])                # every atom loses partners to the other structure
    t = hc.tiny_batch()
    sizes = np.diff(t.so.astype(np.int64)).tolist()
    assert sizes[0] == 0 and sizes[-1] == 0 and 0 in sizes[1:-1] and sizes[1] == 1 and sizes[-2] == 1 and 1 in sizes[2:-2]


def test_tail_batch():
    import tail_cases as tc
    c = hc.tail_batch()
    n_big = int(c.so[-1] - c.so[-2])
    assert n_big >= tc.LDS_MAX_ATOMS and len(c.so) == 5
    b = int(c.so[-2])
    centres = c.info["centres"]
    assert len(centres) == len(np.unique(centres)) == hc.N_TAIL_CENTRES
    assert np.array_equal(np.flatnonzero(c.flags[b:] & 2), centres) and np.all(c.flags & 1) and np.all(c.flags[:b] == 3)
    big = hc.part(c, 3)
    g = sm.grid(big.x, big.y, big.z, big.r, big.probe)
    assert set(g.order[:16]) <= set(centres) and set(g.order[-16:]) <= set(centres)   # the ends of the cell order
    assert sm.margins_hold(big.x, big.y, big.z, big.r, big.probe)
    up, down = hm.counts(big.x, big.y, big.z, big.dirs, big.flags, 13.0)              # the ball-query path of the model
    assert big.n_atoms > hm.DENSE and (up + down)[centres].min() >= 1 and not (up + down)[np.setdiff1d(np.arange(n_big), centres)].any()
    # the candidates decide nothing: a dense evaluation of a few centres gives the same rows
    few = centres[::32]
    sub = np.flatnonzero(np.abs(big.x[:, None] - big.x[None, few]).min(axis=1) <= 14.0)
    for i in few:
        um, dm_ = hm.rule(big.x[i], big.y[i], big.z[i], *big.dirs[i], big.x[sub], big.y[sub], big.z[sub], hm.c2_of(13.0))
        notself = sub != i
        assert (um & notself).sum() == up[i] and (dm_ & notself).sum() == down[i]


# ---- the emulated sweep of k_half_sphere equals the plain model ------------------------------------------------------------

@pytest.mark.parametrize("name", ["cluster", "crowd", "edge", "odd_radius"])   # (the grid emulation takes no NaN)
def test_sweep_with_the_stop_rule_equals_the_model(name):
    c = getattr(hc, name)()
    rng = np.random.default_rng(7)
    sample = np.sort(rng.permutation(c.n_atoms)[:24])
    cutoffs = [hc.EDGE_CUTOFF, 4.9, 7.0] if name == "edge" else [float(c.h), 9.84, 13.0]
    for cutoff in cutoffs:
        want = hm.counts(c.x, c.y, c.z, c.dirs, c.flags, cutoff)
        up, down, stop, by_rule, _ = hm.sweep_counts(*c.cols[:4], c.probe, c.dirs, c.flags, cutoff, sample)
        assert np.array_equal(up, want[0][sample]) and np.array_equal(down, want[1][sample]), cutoff
        if name == "odd_radius":
            assert not by_rule.any()
        elif name != "edge":
            assert by_rule.any()


# ---- pseudo_cb_directions ------------------------------------------------------------------------------------------------

def test_pseudo_cb_directions_against_a_direct_loop():
    import rustsasa_amd
    rng = np.random.default_rng(9)
    sizes = [0, 1, 2, 3, 17, 0, 40, 1]
    off = np.concatenate([[0], np.cumsum(sizes)])
    ca = np.cumsum(rng.normal(size=(off[-1], 3)) * 2.2, axis=0).astype(F)
    ca[30] = ca[29]                                                 # a neighbour that coincides with the atom
    got = rustsasa_amd.pseudo_cb_directions(ca, off)
    assert got.dtype == F and got.shape == (off[-1], 3)
    want = np.zeros((off[-1], 3), np.float64)
    c64 = ca.astype(np.float64)
    for b, e in zip(off[:-1], off[1:]):
        for i in range(b + 1, e - 1):
            for nb in (i - 1, i + 1):
                d = c64[i] - c64[nb]
                length = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
                if length > 0.0:
                    want[i] += d / length
    assert np.array_equal(got, want.astype(F))
    ends = np.unique(np.concatenate([off[:-1][np.diff(off) > 0], off[1:][np.diff(off) > 0] - 1]))
    assert not got[ends].any() and np.isfinite(got).all() and got[30].any() and np.abs(got).max() <= 2.0
    assert rustsasa_amd.HSE_PARTNER == hm.PARTNER == 1 and rustsasa_amd.HSE_CENTRE == hm.CENTRE == 2
    with pytest.raises(ValueError):
        rustsasa_amd.pseudo_cb_directions(ca, [0, 5])
    with pytest.raises(ValueError):
        rustsasa_amd.pseudo_cb_directions(ca[:, :2], off)
    assert rustsasa_amd.pseudo_cb_directions(np.zeros((0, 3)), [0]).shape == (0, 3)


# ---- the bindings and the cutoff rule --------------------------------------------------------------------------------------

def test_symbols_are_declared_and_bound():
    import ctypes as C
    from rustsasa_amd import _capi
    header = open(os.path.join(ROOT, "include", "rustsasa_amd.h")).read()
    one, many = _capi.SYMBOLS["rsasa_half_sphere_exposure"], _capi.SYMBOLS["rsasa_half_sphere_exposure_batch"]
    assert "int rsasa_half_sphere_exposure(" in header and "int rsasa_half_sphere_exposure_batch(" in header
    assert one[0] is C.c_int and len(one[1]) == 13 and one[1][6] is C.c_size_t and one[1][7] is C.c_float and one[1][10] is C.c_float
    assert many[0] is C.c_int and len(many[1]) == 14 and many[1][7] is C.c_size_t and many[1][8] is C.c_float and many[1][11] is C.c_float
    assert "#define RSASA_HSE_PARTNER 1" in header and "#define RSASA_HSE_CENTRE 2" in header


def test_cutoff_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "hse_checks_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "rustsasa_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "hse_checks_test.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "hse checks ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-2000:])
