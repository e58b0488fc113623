"""The dot crowding without a GPU: the model (crowding_model.py) against a float64 brute force, hand tables, the radial
model on the same structure with the dots appended as centre-only atoms, and the scan of the masks' popcounts; the
emulated sweep of k_dot_crowding with its stop rule against the model on every case, and one shell early on the
last-shell case; every input of crowding_cases.py pinned to what it is named for; dot_means against a direct loop; the
binding table; and check_crowding in a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import crowding_cases as cc
import crowding_model as cm
import depth_cases as dc
import depth_model as dm
import points_model as pm
import radial_model as rm
import sweep_cases as sc
import sweep_model as sm

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _part(c, s=0):
    b, e = int(c.so[s]), int(c.so[s + 1])
    return c.x[b:e], c.y[b:e], c.z[b:e], c.r[b:e]


def _model(c):
    mask = cc.masks(c)
    off, rows = cm.counts_batch(c.x, c.y, c.z, c.r, c.so, mask, c.probe, c.n_points, c.edges, c.flags)
    return off, rows, mask


# ---- the model -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["corner", "twins"])
def test_model_equals_a_float64_brute_force(name):
    c = cc.of_depth(name, n_points=33, edges=(3.0, 5.5, 9.0))
    mask = cc.masks(c)
    x, y, z, r = _part(c)
    want, band = cm.brute64(x, y, z, r, mask, c.probe, c.n_points, c.edges)
    # The float32 rounding bound on a distance: coordinates below 64 carry an ulp of 2^-18 at most; a component of q
    # takes two roundings and dx one more (1.5 ulp per axis, three axes), the squares and sums another 2^-22 relative of
    # a d below 10: under 2.5e-5 in all.  Rows with a pair nearer than 16 * 2^-18 = 6.1e-5 to an edge are left out.
    assert max(np.abs(x).max(), np.abs(y).max(), np.abs(z).max()) < 64
    far = band > 16 * 2.0 ** -18
    off, got = cm.counts(x, y, z, r, mask, c.probe, c.n_points, c.edges)
    assert len(got) == int(off[-1]) == len(far) and far.mean() > 0.9
    assert np.array_equal(got[far], want[far]) and got[far].any()


def test_hand_table_of_a_lone_atom():
    """One atom of radius 1.7 at probe 1.4: R = 3.1 (float32 3.1000001), every point free, and the only atom around any
    dot is the owner, R away: with edges (3.0, 3.2, 10.0) it lies in bin 1 of every row.  Without its partner bit the
    rows are zero."""
    c = cc.lone(65)
    off, rows, mask = _model(c)
    assert mask.all() and off.tolist() == [0, 65]
    assert np.array_equal(rows, np.tile(np.array([[0, 1, 0]], np.uint32), (65, 1)))
    _, none = cm.counts(*_part(c), mask, c.probe, c.n_points, c.edges, flags=np.array([254], np.uint8))
    assert none.shape == (65, 3) and not none.any()


def test_hand_table_of_two_atoms_on_an_axis():
    """Atoms at x = 0 and x = 10 with R = 2 (radius 0.6, probe 1.4) at ONE lattice point, which is (0, 0, 1): the dots
    are (0, 0, 2) and (10, 0, 2).  Each dot has its owner at distance 2 and the other atom at sqrt(104) = 10.198: edges
    (2, 10, 10.2) put them in bins 0 and 2; edges (1.9, 1.95) count neither."""
    x, y, z, r = np.array([0, 10], F), np.zeros(2, F), np.zeros(2, F), np.full(2, 0.6, F)
    mask = np.ones((2, 1), bool)
    assert np.array_equal(np.stack(dm.dots_of(x, y, z, r, mask, 1.4, 1)[1:], -1), [[0, 0, 2], [10, 0, 2]])
    off, rows = cm.counts(x, y, z, r, mask, 1.4, 1, (2.0, 10.0, 10.2))
    assert off.tolist() == [0, 1, 2] and rows.tolist() == [[1, 0, 1], [1, 0, 1]]
    assert not cm.counts(x, y, z, r, mask, 1.4, 1, (1.9, 1.95))[1].any()
    assert cm.counts(x, y, z, r, mask, 1.4, 1, (2.0, 10.0, 10.2), flags=[0, 1])[1].tolist() == [[0, 0, 1], [1, 0, 0]]


@pytest.mark.parametrize("name", ["ball", "cavity", "corner"])
def test_model_equals_the_radial_model_with_the_dots_as_centres(name):
    c = cc.of_depth(name, n_points=33, flags=cc.random_flags(dc.get(name).n_atoms, 5))
    off, rows, mask = _model(c)
    x, y, z, r, so, flags, where = cc.with_dots(c, off, mask)
    table = rm.counts_batch(x, y, z, so, c.edges, None, 1, flags)
    assert np.array_equal(table[where, 0, :], rows) and rows.any()
    assert not table[:c.n_atoms].any()                                  # the atoms are no centres


def test_cavity_discriminates_where_the_ball_does_not():
    """The count within 10 A of a dot: 81 to 472 on `cavity`, 88 to 153 on the solid `ball` (100 points)."""
    spans = {}
    for name in ("cavity", "ball"):
        _, rows, _ = _model(cc.of_depth(name))
        within = rows.sum(axis=1)
        spans[name] = (int(within.min()), int(within.max()))
    assert spans == {"cavity": (81, 472), "ball": (88, 153)}


def test_dot_offsets_are_the_scan_of_the_popcounts():
    c = cc.of_depth("tiny", n_points=65)
    off, rows, mask = _model(c)
    free = mask.sum(axis=1)
    assert off.dtype == np.uint64 and off[0] == 0 and np.array_equal(np.diff(off.astype(np.int64)), free)
    assert len(rows) == int(free.sum())


# ---- the sweep -----------------------------------------------------------------------------------------------------------

def _sweep_equals_model(c, sample_size=12, **kw):
    off, rows, mask = _model(c)
    stops = []
    for s in range(len(c.so) - 1):
        b, e = int(c.so[s]), int(c.so[s + 1])
        if e == b:
            continue
        sample = np.sort(np.random.default_rng(7 + s).permutation(e - b)[:sample_size])
        fl = None if c.flags is None else c.flags[b:e]
        got, stop, by_rule, _ = cm.sweep_counts(*_part(c, s), mask[b:e], c.probe, c.n_points, c.edges, fl, sample, **kw)
        for i in sample:
            assert np.array_equal(got[int(i)], rows[int(off[b + i]):int(off[b + i + 1])]), (c.name, s, int(i))
        stops.append((stop, by_rule))
    return stops


@pytest.mark.parametrize("reach", cc.REACHES)
def test_sweep_with_the_stop_rule_equals_the_model_at_every_reach(reach):
    c = cc.of_depth("cavity", n_points=20, edges=cc.reach_edges(sc.H, reach))
    (stop, by_rule), = _sweep_equals_model(c)
    assert (stop[by_rule] == reach).all() and by_rule.any()             # met after `reach` shells, not sooner


@pytest.mark.parametrize("name", ["caps", "packed", "last_shell", "pair"])
def test_sweep_equals_the_model_on_the_cases(name):
    c = getattr(cc, name)()
    if name == "pair":
        c = cc.pair(65)
    _sweep_equals_model(c)


@pytest.mark.parametrize("name", ["column_z", "slant_xp", "slant_ym", "odd_beside_even"])
def test_sweep_equals_the_model_on_thin_long_and_odd_grids(name):
    d = sc.get(name)
    n_points = sc.points_of(name)[0] if name != "odd_beside_even" else 20
    c = cc.Case(name, d.x, d.y, d.z, d.r, d.so, n_points=n_points, edges=(4.0, 9.0), probe=d.probe)
    stops = _sweep_equals_model(c, sample_size=6)
    if name == "odd_beside_even":
        assert stops[0][1].any() and not stops[1][1].any() and not stops[2][1].any()   # odd radii: the whole grid


def test_one_shell_early_loses_the_tie_partners_of_the_last_shell():
    c = cc.last_shell()
    off, rows, mask = _model(c)
    assert sm.margins_hold(*_part(c), c.probe) and sm.grid(*_part(c), c.probe).h == F(2.0)
    owners = np.array([c.info["hi"], c.info["lo"]])
    good, stop, by_rule, found = cm.sweep_counts(*_part(c), mask, c.probe, c.n_points, c.edges, None, owners)
    assert stop.tolist() == [cc.LAST_SHELL] * 2 and by_rule.all() and all(cc.LAST_SHELL in f for f in found)
    early, e_stop, _, _ = cm.sweep_counts(*_part(c), mask, c.probe, c.n_points, c.edges, None, owners, early=True)
    assert e_stop.tolist() == [cc.LAST_SHELL - 1] * 2
    lost = 0
    for o in owners:
        want = rows[int(off[o]):int(off[o + 1])]
        assert np.array_equal(good[int(o)], want)
        lost += int(want.sum()) - int(early[int(o)].sum())
        assert (early[int(o)] <= want).all()
    assert lost >= 6                                                    # three leaning directions of each owner


# ---- the cases are what they are named for --------------------------------------------------------------------------------

def test_caps_free_counts_and_the_last_point():
    c = cc.caps()
    mask = cc.masks(c)
    owners = c.info["owners"]
    assert mask[owners].sum(axis=1).tolist() == [0, 1, 63, 64, 65] == c.info["free"]
    assert np.flatnonzero(mask[owners[1]]).tolist() == [cc.CAP_POINTS - 1]
    _, rows, _ = _model(c)
    assert rows.any()


def test_pass_counts():
    assert cc.PASS == 128 and cc.POINT_COUNTS == (1, 63, 64, 65, 100, 960)
    assert cc.masks(cc.lone()).sum() == 960 and -(-960 // cc.PASS) == 8       # every pass, the last one half full
    m = cc.masks(cc.pair())
    assert (m.sum(axis=1) > cc.PASS).all() and not m.all()
    free = cc.masks(cc.corner(960)).sum(axis=1)
    assert free.max() > cc.PASS and free.min() < cc.PASS                      # one sweep and several, side by side
    c = cc.last_shell()
    assert cc.masks(c)[[c.info["hi"], c.info["lo"]]].sum(axis=1).tolist() == [100, 100]   # a second dot in 36 lanes


@pytest.mark.parametrize("kind", cc.TIE_KINDS)
def test_ties_are_exact(kind):
    c = cc.tie(kind)
    xyz, r, q, e = cc.tie_geometry()
    with np.errstate(over="ignore"):
        dx, dy, dz = xyz[1, 0] - q[0], xyz[1, 1] - q[1], xyz[1, 2] - q[2]
        d2 = dx * dx + dy * dy + dz * dz
    assert d2.dtype == F and dy == 0 and dz == 0 and d2 == e * e            # d2 == e2, bit for bit
    off, rows, mask = _model(c)
    assert mask[0, cc.TIE_DOT]
    row = rows[int(off[0]) + int(mask[0, :cc.TIE_DOT].sum())]
    e2 = cm.e2_of(c.edges)
    if kind == "below":
        assert e2[-1] < d2 and row.tolist() == [1, 0]                       # the owner, 3.1 away, in bin 0; the partner: lost
    else:
        k = 1
        assert e2[k] == d2 and row[0] == 1 and row[k] == 1 and row.sum() == 2   # the owner in bin 0, the partner alone in bin 1
        if kind == "duplicate":
            assert e2[2] == d2 and row[2] == 0                              # the first of equal edges takes it


@pytest.mark.parametrize("edge0", [0.0, 1e-30])
def test_zero_and_underflowing_edges_hold_the_coincident_partner(edge0):
    c = cc.tie_zero(edge0)
    assert cm.e2_of(c.edges)[0] == 0
    off, rows, mask = _model(c)
    assert mask[0].all() and mask[1].all()                                  # R_j = 0 buries nothing
    row = rows[cc.TIE_DOT]
    assert row[0] == 1 and rows[:65, 0].sum() == 1 + 0                      # only that dot has somebody at d2 = 0
    assert rows[65:, 0].all()                                               # the partner's own dots coincide with it


def test_packed_partner_counts_and_steps():
    c = cc.packed()
    for s, n_par in enumerate(cc.PACKED_PARTNERS):
        b, e = int(c.so[s]), int(c.so[s + 1])
        assert int((c.flags[b:e] & 1).sum()) == n_par and e - b == cc.PACKED_ATOMS > sm.WAVE
        g = sm.grid(*_part(c, s), c.probe)
        assert np.diff(g.starts).max() >= cc.PACKED_ATOMS - 3 > sm.WAVE     # (all but the lowest atom of an axis) in one cell:
    assert (c.flags >> 1).any()                                             # two staging batches in its step
    g = sm.grid(*_part(cc.crowd()), cc.crowd().probe)
    assert np.diff(g.starts).max() > 200                                    # a cell of more than 200 atoms


def test_non_finite_cases():
    for c in (cc.nan_coordinate(), cc.nan_radius()):
        off, rows, mask = _model(c)
        a = c.info["atom"]
        assert mask[a].all() and not rows[int(off[a]):int(off[a + 1])].any()    # its own dots: zero rows
        clean = cc.corner(33)
        keep = np.arange(c.n_atoms) != a
        if c.name == "nan_coordinate":                                          # it counts for nobody: the others' rows are
            sub = cc.Case("sub", clean.x[keep], clean.y[keep], clean.z[keep], clean.r[keep],   # those of the structure without it
                          np.array([0, c.n_atoms - 1], np.uint32), n_points=33, edges=c.edges)
            _, sub_rows = cm.counts(*_part(sub), mask[keep], sub.probe, 33, sub.edges)
            assert np.array_equal(np.delete(rows, np.arange(int(off[a]), int(off[a + 1])), axis=0), sub_rows)


# ---- the host helpers and the bindings ------------------------------------------------------------------------------------

def test_dot_means_against_a_direct_loop():
    import rustsasa_amd
    rng = np.random.default_rng(3)
    sizes = np.array([0, 3, 1, 0, 65, 2, 0])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    v = rng.integers(0, 500, int(off[-1])).astype(np.uint32)
    got = rustsasa_amd.dot_means(off, v)
    assert got.dtype == np.float64 and got.shape == (7,)
    for i, n in enumerate(sizes):
        if n == 0:
            assert np.isnan(got[i])
        else:
            assert got[i] == sum(float(t) for t in v[int(off[i]):int(off[i + 1])]) / n
    with pytest.raises(ValueError):
        rustsasa_amd.dot_means(off, v[:-1])
    with pytest.raises(ValueError):
        rustsasa_amd.dot_means(off[::-1], v)
    assert rustsasa_amd.CROWD_PARTNER == cm.PARTNER == 1 and rustsasa_amd.CROWD_MAX_BINS == cm.MAX_BINS == 8


def test_symbols_are_declared_and_bound():
    import ctypes as C
    from rustsasa_amd import _capi
    header = open(os.path.join(ROOT, "include", "rustsasa_amd.h")).read()
    assert "#define RSASA_CROWD_PARTNER 1" in header and "#define RSASA_CROWD_MAX_BINS 8" in header
    assert "#define RSASA_ABI_VERSION 4" in header
    for name, extra in (("rsasa_dot_crowding", 0), ("rsasa_dot_crowding_batch", 1)):
        assert f"int {name}(" in header
        res, args = _capi.SYMBOLS[name]
        assert res is C.c_int and len(args) == 17 + extra and args[-3] is C.c_size_t
    lib = _capi.load()
    assert hasattr(lib, "rsasa_dot_crowding") and hasattr(lib, "rsasa_dot_crowding_batch")


def test_bin_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "crowding_checks_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "rustsasa_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "crowding_checks_test.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "crowding checks ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-2000:])
