"""k_sort_window (kernels.hip) - the LDS binning of every structure of fewer than 65 536 atoms - at its seams: the
registers' share of 8 192 atoms and its slots of 1 024, the rest atoms' trips of 4 096, the 2 304 records the LDS stages,
last windows of 1, 2, 8, 38 and 36 863 cells with the end marker in either half of a word, a word of its own or a
thread's run of its own, windows without atoms, grids without padding behind the marker, 16-bit cursors at 65 535, and
the instantiation that bins one host structure of up to 8 192 atoms.  The inputs (window_cases.py, pinned by
test_window_cases_cpu.py) meet every one of them by construction.

SASA alone is a forgiving witness of a sort (an atom one cell off its cell is still inside the 5 x 5 x 5 block), so next
to values, neighbour counts and neighbour lists the tests take a census: atoms_within_batch with a cutoff larger than
the structure from a few centres.  Its stop rule never fires, so the wave sweeps every shell of the grid - it reads the
start of every row's run, of the cells beside it and the end marker - and every sorted record, and returns all other
atoms of the structure as (d2, idx) sorted by key: every atom placed exactly once, its coordinates intact (the bits of
d2), its sorted_orig right (idx), every run length right.  The lists of every atom at cutoff 3.0 (the sweep stops after
shell 2) lose a record that sits one cell off its cell on the rim.  Every comparison is with the CPU models and exact.
Run on a MI355X with `pytest -m gpu`."""
import functools
import os

import numpy as np
import pytest

import hse_model as hm
import nb_helpers as nh
import within_model as wm
import window_cases as wc
from neighbor_model import NEIGHBOR_DTYPE
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

PROBE = wc.PROBE
N_POINTS = wc.N_POINTS
NEAR = 3.0   # the cutoff of the all-centre lists


# ---- expected results, per structure (the batches share structures) --------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sasa_of(name):
    st = wc.structure(name)
    if not len(st):
        return np.zeros(0, np.float32)
    return po.calculate_sasa_batch(st.x, st.y, st.z, st.r, st.ids, np.array([0, len(st)], np.uint32), PROBE, N_POINTS, 8,
                                   threads=0)


@functools.lru_cache(maxsize=None)
def _neighbours_of(name):
    st = wc.structure(name)
    if not len(st):
        return np.zeros(1, np.uint64), np.zeros(0, NEIGHBOR_DTYPE)
    return nh.oracle_csr(st.x, st.y, st.z, st.r, st.ids, PROBE)


@functools.lru_cache(maxsize=None)
def _census_of(name, centres, cutoff):
    st = wc.structure(name)
    fl = np.ones(len(st), np.uint8)
    fl[np.asarray(centres, np.int64)] = 3
    return wm.lists(st.x, st.y, st.z, fl, cutoff)


@functools.lru_cache(maxsize=None)
def _near_of(name):
    st = wc.structure(name)
    return wm.lists(st.x, st.y, st.z, None, NEAR)


def _join(parts):
    """CSR results of the structures of a batch -> the batch's (offsets over all atoms, idx within the structure)."""
    offs, total = [np.zeros(1, np.uint64)], np.uint64(0)
    for o, _ in parts:
        offs.append(o[1:] + total)
        total += o[-1]
    return np.concatenate(offs), np.concatenate([e for _, e in parts])


def _want_sasa(case):
    return np.concatenate([_sasa_of(n) for n in wc.names_of(case)])


def _want_neighbours(case):
    return _join([_neighbours_of(n) for n in wc.names_of(case)])


def _want_census(case):
    cutoff = wc.census_cutoff(case)
    return _join([_census_of(n, tuple(wc.census_centres(len(wc.structure(n)))), cutoff) for n in wc.names_of(case)])


def _want_near(case):
    return _join([_near_of(n) for n in wc.names_of(case)])


# ---- runs -------------------------------------------------------------------------------------------------------------

def _device_run(ctx, case):
    """calculate_sasa_batch on device-resident columns (as _device_run of test_gpu_tail_edges.py)."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    x, y, z, r, ids = t(case.x), t(case.y), t(case.z), t(case.r), t(case.ids.view(np.int64))
    out = torch.full((case.n_atoms,), -1.0, dtype=torch.float32, device=dev)
    k = torch.full((case.n_atoms,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.enqueue_device(x, y, z, r, ids, case.so, out, None, None, k, PROBE, N_POINTS,
                       stream=torch.cuda.current_stream().cuda_stream)
    ctx.wait()
    return out.cpu().numpy(), k.cpu().numpy().view(np.uint32)


def _assert_values(what, got, want):
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


def _assert_lists(what, got, want):
    go, ge = got
    wo, we = want
    assert go.dtype == np.uint64 and ge.dtype == wm.WITHIN_DTYPE
    bad = np.flatnonzero(np.diff(go.astype(np.int64)) != np.diff(wo.astype(np.int64))) if len(go) == len(wo) else None
    assert np.array_equal(go, wo), (what, None if bad is None else (bad.size, bad[:5]))
    assert ge.tobytes() == we.tobytes(), (what, int(np.sum(ge != we)), np.flatnonzero(ge != we)[:5])


# (a) the atom-count ladder and its reverse, (b) the window shapes and the interleaved batch, (c) the staging structures.
# Each of the three tests below runs every batch twice through a fresh context of its own (the first call of a context
# finds the cell array too small and runs again; every call bins the batch anew with k_sort_window<false>).  They are
# three because the CPU models of the ladder's 76 803 atoms, whose sizes are given, take a second and a half together.

@pytest.mark.parametrize("case", wc.SORT_CASES)
def test_values_counts_neighbour_lists_and_cells(case):
    """Values and neighbour counts of the device entry, the number of cells the device reports (the case is the case
    there too), and the neighbour lists."""
    import rustsasa_amd
    cs = wc.get(case)
    sizes = np.diff(cs.so.astype(np.int64))
    want, lists = _want_sasa(case), _want_neighbours(case)
    want_k = np.diff(lists[0].astype(np.int64)).astype(np.uint32)
    with rustsasa_amd.Context(0) as c:
        c.enable_timing(True)
        for rep in range(2):
            atom, k = _device_run(c, cs)
            assert c.timings()["n_cells"] == wc.n_cells_sum(case), (case, rep)
            _assert_values((case, rep), atom, want)
            assert np.array_equal(k, want_k), (case, rep, int(np.sum(k != want_k)), np.flatnonzero(k != want_k)[:5])
            got = c.precompute_neighbors_batch(*cs.cols, PROBE)
            nh.check_invariants(got, np.repeat(sizes, sizes))
            nh.assert_same(got, lists)


@pytest.mark.parametrize("case", wc.SORT_CASES)
def test_census_of_every_structure(case):
    """The census from the first, the last and the 8 193rd (else the middle) input atom of every structure: each list
    is every other atom of the structure, byte for byte."""
    import rustsasa_amd
    cs = wc.get(case)
    sizes = np.diff(cs.so.astype(np.int64))
    flags, cutoff = wc.census_flags(case), wc.census_cutoff(case)
    census = _want_census(case)
    centre = np.flatnonzero(flags == 3)
    assert np.array_equal(np.diff(census[0].astype(np.int64))[centre], np.repeat(sizes, sizes)[centre] - 1)
    assert len(census[1]) == int(np.sum(np.repeat(sizes, sizes)[centre] - 1))
    with rustsasa_amd.Context(0) as c:
        for rep in range(2):
            _assert_lists((case, rep), c.atoms_within_batch(*cs.cols, PROBE, flags=flags, cutoff=cutoff), census)


@pytest.mark.parametrize("case", wc.SORT_CASES)
def test_lists_of_every_atom_at_3A(case):
    """atoms_within_batch with every atom a centre at 3.0 A: the sweep stops after shell 2, so a record that sits a
    cell off its cell drops out of the lists of the atoms on the other rim."""
    import rustsasa_amd
    cs = wc.get(case)
    near = _want_near(case)
    with rustsasa_amd.Context(0) as c:
        for rep in range(2):
            _assert_lists((case, rep), c.atoms_within_batch(*cs.cols, PROBE, cutoff=NEAR), near)


def test_dense_cells_census_and_half_sphere_counts():
    """(d) two structures of 65 535 atoms with 42 875 atoms in one cell, in the first window of one and in the last of
    the other: cursors and cell starts up to 65 535 in either half of a counter word.  The census (lists of 65 534
    entries) and half_sphere_exposure counts - over the whole structure from the census centres, and at 13 A from 64
    centres of each structure, half of them inside the dense cell; the models are quadratic, so no SASA and no lists
    of every atom.  The counts run twice through the context, the census once."""
    import rustsasa_amd
    cs = wc.get("dense")
    sizes = np.diff(cs.so.astype(np.int64))
    flags, cutoff = wc.census_flags("dense"), wc.census_cutoff("dense")
    census = wm.lists_batch(cs.x, cs.y, cs.z, cs.so, flags, cutoff)
    assert np.diff(census[0].astype(np.int64))[flags == 3].tolist() == [65534] * 6
    rng = np.random.default_rng(5)
    dirs = rng.normal(size=(cs.n_atoms, 3)).astype(np.float32)
    some = np.ones(cs.n_atoms, np.uint8)
    for s, st in enumerate(cs.structures):
        fine = np.flatnonzero(st.blob == -2)
        rest = np.flatnonzero(st.blob >= 0)
        some[int(cs.so[s]) + np.concatenate([rng.choice(fine, 32, replace=False), rng.choice(rest, 32, replace=False)])] = 3
    all_up, all_down = hm.counts_batch(cs.x, cs.y, cs.z, cs.so, dirs, flags, cutoff)
    assert np.array_equal((all_up + all_down)[flags == 3], np.full(6, 65534, np.uint32))
    up13, down13 = hm.counts_batch(cs.x, cs.y, cs.z, cs.so, dirs, some, 13.0)
    assert int((up13 + down13).max()) > 40000
    with rustsasa_amd.Context(0) as c:
        # (once: a list of 65 534 entries is ranked by k_neighbor_rank_spill, quadratic in its length - 0.9 s a call)
        _assert_lists("dense", c.atoms_within_batch(*cs.cols, PROBE, flags=flags, cutoff=cutoff), census)
        for rep in range(2):
            up, down = c.half_sphere_exposure_batch(*cs.cols, PROBE, dirs=dirs, flags=flags, cutoff=cutoff)
            assert np.array_equal(up, all_up) and np.array_equal(down, all_down), ("dense", rep)
            up, down = c.half_sphere_exposure_batch(*cs.cols, PROBE, dirs=dirs, flags=some, cutoff=13.0)
            assert np.array_equal(up, up13) and np.array_equal(down, down13), ("dense", rep)
    assert sizes.tolist() == [65535, 65535]


# ---- (e) one host structure -----------------------------------------------------------------------------------------

def _context(small_path):
    """A fresh context that runs the small path (the default) or never does (as _context of test_gpu_host_paths.py)."""
    import rustsasa_amd
    old = os.environ.get("RSASA_SMALL_PATH")
    os.environ["RSASA_SMALL_PATH"] = "1" if small_path else "0"
    try:
        return rustsasa_amd.Context(0)
    finally:
        if old is None:
            del os.environ["RSASA_SMALL_PATH"]
        else:
            os.environ["RSASA_SMALL_PATH"] = old


@pytest.fixture(scope="module")
def ctxs():
    small, general = _context(True), _context(False)
    yield small, general
    small.close()
    general.close()


def _sequential_sums(values, ro):
    out = np.zeros(len(ro) - 1, np.float32)
    for k in range(len(ro) - 1):
        acc = np.float32(0.0)
        for v in values[int(ro[k]):int(ro[k + 1])]:
            acc = np.float32(acc + v)
        out[k] = acc
    return out


@pytest.mark.parametrize("name", wc.SINGLE_CASES)
def test_one_host_structure_per_call(ctxs, name):
    """(e) one structure from pageable numpy through calculate_sasa_batch (with residue offsets that do not cover all
    atoms) and through calculate_sasa_soa.  Up to kSingleAtoms = 8 192 atoms the default context bins it with
    k_sort_window<true> (run_small_host_batch: S == 1, N <= 8 192, no timing; small_grid takes these grids, of at most 64
    windows), 8 193 atoms take the one-upload small path and k_sort_window<false>; the context created with
    RSASA_SMALL_PATH=0 and the timed one run the general path.  Below 32 768 atoms the routes cannot be told apart
    from outside (test_gpu_host_paths.py): the limits above send each call where it goes, and all three must give the
    oracle's values; the timed run also reports the grid's cells."""
    import rustsasa_amd
    st = wc.structure(name)
    n = len(st)
    so = np.array([0, n], np.uint32)
    ro = wc.residue_offsets(n)
    want = po.calculate_sasa_internal(st.x, st.y, st.z, st.r, st.ids, PROBE, N_POINTS, 8, threads=0)
    assert want.tobytes() == _sasa_of(name).tobytes()
    want_res = _sequential_sums(want, ro)
    assert want_res.tobytes() == po.residue_sums(want, ro).tobytes()
    if st.pairs:   # a record that lost its id shows in the values
        i, j = st.pairs[0]
        without = po.calculate_sasa_internal(st.x, st.y, st.z, st.r, None, PROBE, N_POINTS, 8, threads=0)
        assert want[i] != without[i] or want[j] != without[j]
    with rustsasa_amd.Context(0) as timed:
        timed.enable_timing(True)
        _assert_values((name, "timed"), timed.calculate_sasa_soa(st.x, st.y, st.z, st.r, st.ids, PROBE, N_POINTS), want)
        assert timed.timings()["n_cells"] == int(np.prod(wc.EXPECT[name][0]))
    for c in ctxs:
        for rep in range(2):
            what = (name, c is ctxs[0], rep)
            atom, res = c.calculate_sasa_batch(st.x, st.y, st.z, st.r, st.ids, so, PROBE, N_POINTS, residue_offsets=ro)
            _assert_values(what, atom, want)
            assert res.tobytes() == want_res.tobytes(), what
            _assert_values(what, c.calculate_sasa_soa(st.x, st.y, st.z, st.r, st.ids, PROBE, N_POINTS), want)
