"""The radial counts without a GPU: the model (radial_model.py) against a float64 brute force, against a table worked out
by hand and against the half-sphere model through the cumulative and the per-class identity; the emulated sweep of
k_radial_counts (its stop rule included) against the plain model; every new case of radial_cases.py pinned to what it is
named for; pairs_from_counts and radial_density against direct loops; the binding table; and check_radial / check_classes
in a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import hse_cases as hc
import hse_model as hm
import radial_cases as rc
import radial_model as rm
import sweep_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BAND = 1e-4
SEEDS = (100, 102, 103, 104, 107, 108)   # test_hse_cpu.py's: no pair lies within BAND of 3.5, 6 or 13 A
EDGES64 = (3.5, 6.0, 13.0)


def _small_cluster(seed, n=60):
    xyz = np.random.default_rng(seed).uniform(0.0, 20.0, (n, 3)).astype(F)
    return xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy()


# ---- the model ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_model_equals_a_float64_brute_force(seed):
    x, y, z = _small_cluster(seed)
    rng = np.random.default_rng(seed + 2)
    cl = rc.classes_of(len(x), 3, seed + 3)
    for flags in (None, rng.integers(0, 4, len(x)).astype(np.uint8)):
        want, band = rm.brute64(x, y, z, EDGES64, cl, 3, flags)
        assert band > BAND, band                                     # zero pairs in the band: none is left out
        got = rm.counts(x, y, z, EDGES64, cl, 3, flags)
        assert got.dtype == np.uint32 and np.array_equal(got, want)
        assert all(want[:, :, k].sum() > 0 for k in range(3))


def test_hand_case():
    """hse_cases.hand(): atoms 0 and 4 coincide at (1, 2, 3) and are the centres; atom 1 is 3 away (z), atom 2 is 2 away,
    atom 3 is 3 away (x), atom 5 is 7 away.  Classes (0, 1, 0, 1, 2, 2), edges (0, 2, 3, 5), so e2 = (0, 4, 9, 25).
    Centre 0: atom 4 (class 2, d2 0) in bin 0 - the bin of the coincident atoms -, atom 2 (class 0, d2 4) in bin 1, atoms 1
    and 3 (class 1, d2 9) in bin 2 - an exact tie goes to the bin whose edge it meets -, atom 5 nowhere; itself never.
    Centre 4: atom 0 (class 0) in bin 0, atom 2 in bin 1, atoms 1 and 3 in bin 2.  The others are partners only."""
    c = hc.hand()
    cl = np.array([0, 1, 0, 1, 2, 2], np.uint8)
    got = rm.counts(c.x, c.y, c.z, (0.0, 2.0, 3.0, 5.0), cl, 3, c.flags)
    want = np.zeros((6, 3, 4), np.uint32)
    want[0] = [[0, 1, 0, 0], [0, 0, 2, 0], [1, 0, 0, 0]]
    want[4] = [[1, 1, 0, 0], [0, 0, 2, 0], [0, 0, 0, 0]]
    assert np.array_equal(got, want)
    pairs = rm.pairs_from_counts(got, c.so, cl)
    assert pairs.shape == (1, 3, 3, 4) and np.array_equal(pairs[0, 0], want[0]) and np.array_equal(pairs[0, 2], want[4])
    assert not pairs[0, 1].any()
    # of equal edges the first takes the pair; an edge whose square underflows to 0 holds the coincident atoms only
    got = rm.counts(c.x, c.y, c.z, (3.0, 3.0, 5.0), cl, 3, c.flags)
    assert got[0].tolist() == [[1, 0, 0], [2, 0, 0], [1, 0, 0]]
    assert rm.e2_of([1e-30])[0] == 0.0
    got = rm.counts(c.x, c.y, c.z, (1e-30, 5.0), cl, 3, c.flags)
    assert got[0].tolist() == [[0, 1], [0, 2], [1, 0]] and got[4].tolist() == [[1, 1], [0, 2], [0, 0]]
    # a NaN coordinate counts nowhere and gets a zero row; an overflowing last edge counts everybody else
    y = c.y.copy()
    y[2] = np.nan
    got = rm.counts(c.x, y, c.z, (2.0, float(np.finfo(F).max)), None, 1, None)
    assert not got[2].any() and got[:, 0, :].sum(1).tolist() == [4, 4, 0, 4, 4, 4] and got[0, 0].tolist() == [1, 3]


def test_cumulative_and_per_class_identities_with_the_half_sphere_model():
    c = hc.cluster()
    edges = hc.cluster_cutoffs()
    assert np.all(np.diff(np.array(edges, F)) >= 0) and edges[0] == 0.0 and not np.isfinite(rm.e2_of(edges)[-1])
    cl = rc.case_classes("cluster")
    flags = np.random.default_rng(5).integers(0, 4, c.n_atoms).astype(np.uint8)
    for fl in (None, flags):
        table = rm.counts(c.x, c.y, c.z, edges, cl, rc.N_CLASSES, fl)
        cum = np.cumsum(table.astype(np.int64), axis=2)
        for k, cutoff in enumerate(edges):
            up, down = hm.counts(c.x, c.y, c.z, None, fl, cutoff)
            assert np.array_equal(cum[:, :, k].sum(1), up.astype(np.int64) + down), cutoff
        base = np.full(c.n_atoms, 3, np.uint8) if fl is None else fl
        for b in range(rc.N_CLASSES):
            only = np.where(cl == b, base, base & 2).astype(np.uint8)        # the partner bit cleared on the other classes
            up, down = hm.counts(c.x, c.y, c.z, None, only, 13.0)
            assert np.array_equal(cum[:, b, edges.index(13.0)], up.astype(np.int64) + down), b


# ---- the emulated sweep of k_radial_counts equals the plain model ----------------------------------------------------------

@pytest.mark.parametrize("name", ["cluster", "crowd", "edge"])
def test_sweep_with_the_stop_rule_equals_the_model(name):
    c = getattr(hc, name)()
    cl = rc.case_classes(name)
    sample = np.sort(np.random.default_rng(7).permutation(c.n_atoms)[:24])
    lists = [(2.0, hc.EDGE_CUTOFF), (hc.EDGE_CUTOFF, 7.0), (4.9,)] if name == "edge" else [rc.EDGES, (float(c.h), 9.84, 13.0), (3.0,)]
    for edges in lists:
        want = rm.counts(c.x, c.y, c.z, edges, cl, rc.N_CLASSES, c.flags)
        rows, stop, by_rule, _ = rm.sweep_counts(*c.cols[:4], c.probe, edges, cl, rc.N_CLASSES, c.flags, sample)
        assert np.array_equal(rows, want[sample]), edges
        assert by_rule.any() and want[sample].sum() > 0


def test_a_stop_rule_one_shell_off_loses_the_tie_partners_of_edge():
    c = hc.edge()
    hi, lo = c.info["hi"], c.info["lo"]
    cl = rc.case_classes("edge")
    edges = (2.0, hc.EDGE_CUTOFF)
    want = rm.counts(c.x, c.y, c.z, edges, cl, rc.N_CLASSES, None)[[hi, lo]]
    assert want.sum(axis=(1, 2)).tolist() == [6, 6] and want[:, :, 1].sum(1).tolist() == [6, 6]
    rows, stop, by_rule, found = rm.sweep_counts(*c.cols[:4], c.probe, edges, cl, rc.N_CLASSES, None, [hi, lo])
    assert np.array_equal(rows, want) and stop.tolist() == [3, 3] and by_rule.all() and found == [[2, 3], [2, 3]]
    # the switch: a rule that is met one shell earlier leaves shell 3 unswept and loses the three ties that lie there
    rows, stop, *_ = rm.sweep_counts(*c.cols[:4], c.probe, edges, cl, rc.N_CLASSES, None, [hi, lo], half=-0.5)
    assert stop.tolist() == [2, 2] and rows.sum(axis=(1, 2)).tolist() == [3, 3]
    # (one that is met a shell later, half = 1.5, sweeps shell 4 for nothing: the partners at 7 are beyond the edge)
    rows, stop, *_ = rm.sweep_counts(*c.cols[:4], c.probe, edges, cl, rc.N_CLASSES, None, [hi, lo], half=1.5)
    assert stop.tolist() == [4, 4] and np.array_equal(rows, want)
    # with 7 as the last edge the partners at 7 count too, in the bin behind the ties'
    want7 = rm.counts(c.x, c.y, c.z, (hc.EDGE_CUTOFF, 7.0), cl, rc.N_CLASSES, None)[[hi, lo]]
    assert want7[:, :, 0].sum(1).tolist() == [6, 6] and want7[:, :, 1].sum(1).min() >= 6


# ---- the new cases are what they are named for -----------------------------------------------------------------------------

def test_new_cases():
    assert sorted(a * b for a, b in rc.SHAPES) == [1, 21, 63, 64, 65, 512]
    assert all(1 <= a <= rm.MAX_CLASSES and 1 <= b <= rm.MAX_BINS for a, b in rc.SHAPES)
    assert (rm.MAX_CLASSES, rm.MAX_BINS) in rc.SHAPES and sm.WAVE == 64
    for n_classes, n_bins in rc.SHAPES:
        e = rc.edges_of(n_bins)
        assert e.dtype == F and len(e) == n_bins and np.all(np.diff(e) > 0) and e[-1] == F(12.0)
        cl = rc.classes_of(2000, n_classes, 1)
        assert cl.dtype == np.uint8 and set(cl.tolist()) == set(range(n_classes))
    m = rc.many_small()
    assert len(m.so) == rc.N_SMALL + 1 and np.all(np.diff(m.so.astype(np.int64)) == 3) and m.n_atoms == 900 < 1024
    t = rm.counts_batch(m.x, m.y, m.z, m.so, (8.0,), None, 1, None)
    assert np.all(t == 2)                                           # both others, nobody of another structure
    b = rc.big_box()
    xyz = np.stack([b.x, b.y, b.z], -1).astype(np.float64)
    assert b.n_atoms == rc.N_BOX > 65535 and np.linalg.norm(xyz.max(0) - xyz.min(0)) < rc.BOX_EDGE * 0.7
    assert rc.N_BOX * (rc.N_BOX - 1) == 4303294400 > 2 ** 32 == 4294967296 and rc.N_BOX - 1 < 2 ** 31
    assert len(np.unique(xyz, axis=0)) == rc.N_BOX and sm.margins_hold(b.x, b.y, b.z, b.r, b.probe)
    for name in ("cluster", "crowd", "edge", "interleaved", "tiny_batch", "tail_batch"):
        cl = rc.case_classes(name)
        assert len(cl) == getattr(hc, name)().n_atoms and cl.max() == rc.N_CLASSES - 1
        assert np.array_equal(cl, rc.case_classes(name))            # seeded


# ---- helpers ---------------------------------------------------------------------------------------------------------------

def test_pairs_from_counts_against_a_direct_loop_and_its_symmetry():
    c = hc.tiny_batch()
    cl = rc.case_classes("tiny_batch")
    flags = np.random.default_rng(11).integers(0, 4, c.n_atoms).astype(np.uint8)
    for fl in (None, flags):
        table = rm.counts_batch(c.x, c.y, c.z, c.so, rc.EDGES, cl, rc.N_CLASSES, fl)
        got = rm.pairs_from_counts(table, c.so, cl)
        want = np.zeros((len(c.so) - 1, rc.N_CLASSES, rc.N_CLASSES, len(rc.EDGES)), np.uint64)
        for s in range(len(c.so) - 1):
            for i in range(int(c.so[s]), int(c.so[s + 1])):
                for b in range(rc.N_CLASSES):
                    for k in range(len(rc.EDGES)):
                        want[s, cl[i], b, k] += np.uint64(table[i, b, k])
        assert got.dtype == np.uint64 and np.array_equal(got, want) and got.sum() == table.sum() > 0
        if fl is None:
            assert np.array_equal(got, got.transpose(0, 2, 1, 3))   # d2 is symmetric bit for bit
        else:
            assert not np.array_equal(got, got.transpose(0, 2, 1, 3))
    big = np.full((3, 1, 1), 2 ** 31 - 1, np.uint32)                # the sums are 64 bits wide
    assert rm.pairs_from_counts(big, [0, 3]).tolist() == [[[[3 * (2 ** 31 - 1)]]]]


def test_radial_density_against_direct_computation():
    import rustsasa_amd
    assert rustsasa_amd.RADIAL_PARTNER == rm.PARTNER == 1 and rustsasa_amd.RADIAL_CENTRE == rm.CENTRE == 2
    assert rustsasa_amd.RADIAL_MAX_CLASSES == rm.MAX_CLASSES == 16 and rustsasa_amd.RADIAL_MAX_BINS == rm.MAX_BINS == 32
    counts = np.random.default_rng(13).integers(0, 50, (7, 3, 4)).astype(np.uint32)
    edges = (0.0, 6.0, 6.0, 12.0)
    got = rustsasa_amd.radial_density(counts, edges)
    assert got.dtype == np.float64 and got.shape == counts.shape
    prev = 0.0
    for k, e in enumerate(edges):
        vol = 4.0 / 3.0 * np.pi * (e ** 3 - prev ** 3)
        prev = e
        if vol == 0.0:
            assert np.isnan(got[..., k]).all()                      # an empty shell
        else:
            assert np.array_equal(got[..., k], counts[..., k].astype(np.float64) / vol)
    assert np.isnan(got[..., 0]).all() and np.isnan(got[..., 2]).all() and np.isfinite(got[..., 1]).all()
    one = rustsasa_amd.radial_density(np.array([8, 16]), np.array([1.0, 2.0], F))
    assert np.array_equal(one, [8 / (4 / 3 * np.pi), 16 / (4 / 3 * np.pi * 7)])
    for bad in ((1.0, 2.0, 3.0), (2.0, 1.0), (-1.0, 2.0), (1.0, np.inf)):
        with pytest.raises(ValueError):
            rustsasa_amd.radial_density(np.zeros((3, 2)), bad)


# ---- the bindings and the argument rules -------------------------------------------------------------------------------------

def test_symbols_are_declared_and_bound():
    import ctypes as C
    from rustsasa_amd import _capi
    header = open(os.path.join(ROOT, "include", "rustsasa_amd.h")).read()
    one, many = _capi.SYMBOLS["rsasa_radial_counts"], _capi.SYMBOLS["rsasa_radial_counts_batch"]
    assert "int rsasa_radial_counts(" in header and "int rsasa_radial_counts_batch(" in header
    assert one[0] is C.c_int and len(one[1]) == 15 and one[1][6] is C.c_size_t and one[1][7] is C.c_float
    assert one[1][10] is C.c_uint32 and one[1][12] is C.c_uint32 and one[1][11] is C.c_void_p and one[1][14] is C.c_void_p
    assert many[0] is C.c_int and len(many[1]) == 16 and many[1][7] is C.c_size_t and many[1][8] is C.c_float
    assert many[1][11] is C.c_uint32 and many[1][13] is C.c_uint32 and many[1][12] is C.c_void_p and many[1][15] is C.c_void_p
    for macro in ("RSASA_RADIAL_PARTNER 1", "RSASA_RADIAL_CENTRE 2", "RSASA_RADIAL_MAX_CLASSES 16", "RSASA_RADIAL_MAX_BINS 32",
                  "RSASA_ABI_VERSION 4"):
        assert "#define " + macro + "\n" in header, macro
    assert _capi.RADIAL_MAX_CLASSES == 16 and _capi.RADIAL_MAX_BINS == 32
    lib = _capi.load()
    assert lib.rsasa_abi_version() == 4 and hasattr(lib, "rsasa_radial_counts") and hasattr(lib, "rsasa_radial_counts_batch")


def test_bin_and_class_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "radial_checks_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "rustsasa_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "radial_checks_test.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "radial checks ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-2000:])
