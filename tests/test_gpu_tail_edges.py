"""The batch-wide ("tail") binning route - k_zero_cells, k_cell_hist, k_scan_reduce / block_sums / apply, k_scatter,
placed by k_grid_params / scan / bases - where the rest of the suite never takes it: cell scans of two, four and five
tiles per workgroup, all 1024 scan workgroups active, batches of several structures of 65 536 atoms or more with
cell bases off the 16-byte vectors the scan kernels work on, such structures behind more than 256 others and behind
LDS-binned ones, and trajectory frames of such a system.  The inputs (tail_cases.py, pinned by test_tail_cases_cpu.py)
keep every atom among neighbours, so a run of sorted atoms that a wrong prefix misplaces changes lists and values.
Every comparison is with the CPU oracle and exact.  Run on a MI355X with `pytest -m gpu`."""
import functools

import numpy as np
import pytest

import nb_helpers as nh
import point_edge_cases as pe
import points_model as pm
import tail_cases as tc
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

PROBE = tc.PROBE


def _case(name):
    return tc.trajectory_case() if name == "trajectory" else tc.get(name)


@functools.lru_cache(maxsize=None)
def _want_sasa(name, n_points=100):
    return po.calculate_sasa_batch(*_case(name).cols, PROBE, n_points, 8, threads=0)


@functools.lru_cache(maxsize=None)
def _want_lists(name):
    return nh.oracle_batch_csr(*_case(name).cols, PROBE)


def _want_counts(name):
    return np.diff(_want_lists(name)[0].astype(np.int64)).astype(np.uint32)


def _device_run(ctx, case, n_points=100, want_k=True):
    """calculate_sasa_batch on device-resident columns (as _device_run of test_gpu_parity.py, at this file's probe)."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    x, y, z, r, ids = t(case.x), t(case.y), t(case.z), t(case.r), t(case.ids.view(np.int64))
    out = torch.full((case.n_atoms,), -1.0, dtype=torch.float32, device=dev)
    k = torch.full((case.n_atoms,), -1, dtype=torch.int32, device=dev) if want_k else None
    torch.cuda.synchronize()
    ctx.enqueue_device(x, y, z, r, ids, case.so, out, None, None, k, PROBE, n_points,
                       stream=torch.cuda.current_stream().cuda_stream)
    ctx.wait()
    return out.cpu().numpy(), None if k is None else k.cpu().numpy().view(np.uint32)


def _assert_values(name, atom, want):
    bad = np.flatnonzero(atom != want)
    assert bad.size == 0, (name, bad.size, bad[:5], atom[bad[:5]], want[bad[:5]])


RUNS = [(n, None) for n in ("2^20", "2^20+1", "five_tiles", "batch_a", "batch_b_dup")] + \
       [(n, o) for n in ("batch_b", "batch_c") for o in ("0", "1")]


@pytest.mark.parametrize("name,overlap", RUNS)
def test_values_counts_cells_and_lists(name, overlap, monkeypatch):
    """Per-atom values, neighbour counts and the neighbour lists of every case, twice through one fresh context (the
    first call of the five-tile case finds the cell array too small and runs again, the second does not), and the
    number of cells the device reports: the case is the case there too.  overlap: RSASA_OVERLAP_TAIL, the tail's binning
    on the side stream beside the occlusion launch over the LDS-binned structures."""
    import rustsasa_amd
    case = tc.get(name)
    L = tc.layout(case)
    want, want_k, lists = _want_sasa(name), _want_counts(name), _want_lists(name)
    if overlap is not None:
        monkeypatch.setenv("RSASA_OVERLAP_TAIL", overlap)
    with rustsasa_amd.Context(0) as c:
        c.enable_timing(True)
        for rep in range(2):
            atom, k = _device_run(c, case)
            assert c.timings()["n_cells"] == L.n_cells_sum, (name, rep)
            _assert_values(name, atom, want)
            assert np.array_equal(k, want_k), (name, rep, int(np.sum(k != want_k)))
            got = c.precompute_neighbors_batch(*case.cols, PROBE)
            nh.check_invariants(got, np.repeat(np.diff(case.so.astype(np.int64)), np.diff(case.so.astype(np.int64))))
            nh.assert_same(got, lists)


@pytest.mark.parametrize("name", ["batch_a", "2^20+1"])
def test_point_masks_and_contact_counts(name):
    """accessible_points_batch and contact_points_batch read the tail's 32-bit cell starts as well.  The models of
    the point tests take minutes at this size: the masks are checked through their popcounts (sasa_of gives the
    oracle's values byte for byte), the contact lists against the oracle's, the counts by the sum rules of
    test_one_context_through_point_and_contact_calls."""
    import rustsasa_amd
    case = tc.get(name)
    n, n_points = case.n_atoms, 100
    want, lists = _want_sasa(name), _want_lists(name)
    rows = np.repeat(np.arange(n), np.diff(lists[0].astype(np.int64)))
    with rustsasa_amd.Context(0) as c:
        for rep in range(2):
            words, sasa = c.accessible_points_batch(*case.cols, PROBE, n_points)
            assert words.shape == (n, pm.words_of(n_points)) and words.dtype == np.uint32
            assert not np.any(words[:, -1] >> np.uint32(n_points % 32))      # no bit past the last point
            assert sasa.tobytes() == want.tobytes()
            exposed = pe.popcount(words)
            assert pm.sasa_of(case.r, PROBE, exposed, n_points).tobytes() == want.tobytes()
            buried = n_points - exposed
            got = c.contact_points_batch(*case.cols, PROBE, n_points)
            nh.assert_same(got[:2], lists)
            assert got[4].tobytes() == want.tobytes()
            assert got[2].shape == got[3].shape == (len(lists[1]),)
            s_cov, s_exc, m_cov = (np.zeros(n, np.int64) for _ in range(3))
            np.add.at(s_cov, rows, got[2].astype(np.int64))
            np.add.at(s_exc, rows, got[3].astype(np.int64))
            np.maximum.at(m_cov, rows, got[2].astype(np.int64))
            assert np.all(s_exc <= buried) and np.all(buried <= s_cov) and np.all(m_cov <= buried)
            assert np.all(got[3] <= got[2]) and int(got[2].max()) <= n_points


def test_960_points_over_three_tail_structures():
    """The many-point kernel over batch (a)."""
    import rustsasa_amd
    case = tc.get("batch_a")
    want = _want_sasa("batch_a", 960)
    with rustsasa_amd.Context(0) as c:
        for rep in range(2):
            atom, _ = _device_run(c, case, n_points=960, want_k=False)
            _assert_values("batch_a@960", atom, want)


def test_trajectory_of_a_system_past_the_lds_limit():
    """Trajectory mode on 65 536 atoms: every frame is a tail structure (k_expand_frames tiles the system), the grids
    differ per frame (all past 2^20 cells: the scan runs four tiles per workgroup).  Residue sums as well."""
    import rustsasa_amd
    xyz, r, ids, ro, dims = tc.trajectory()
    assert xyz.shape == (tc.N_FRAMES, 65536, 3) and len(set(dims)) == tc.N_FRAMES
    assert tc.layout(tc.trajectory_case()).tiles == 4
    want = [po.calculate_sasa_internal(xyz[f, :, 0], xyz[f, :, 1], xyz[f, :, 2], r, ids, PROBE, 100, 8, threads=0)
            for f in range(tc.N_FRAMES)]
    assert _want_sasa("trajectory").tobytes() == np.concatenate(want).tobytes()
    with rustsasa_amd.Context(0) as c:
        for rep in range(2):
            atom, rsum = c.calculate_sasa_trajectory(xyz, r, ids, PROBE, 100, residue_offsets=ro)
            assert atom.shape == (tc.N_FRAMES, len(r)) and rsum.shape == (tc.N_FRAMES, len(ro) - 1)
            for f in range(tc.N_FRAMES):
                _assert_values(f"frame {f}", atom[f], want[f])
                assert np.array_equal(rsum[f], po.residue_sums(want[f], ro))
        # the same frames as a batch: lists and counts frame by frame
        case = tc.trajectory_case()
        nh.assert_same(c.precompute_neighbors_batch(*case.cols, PROBE), _want_lists("trajectory"))


def test_host_entries_equal_the_device_path():
    """Batch (b) from host memory - calculate_sasa_batch and one host_batch_enqueue / host_batch_wait pair - against
    the device-resident call and the oracle."""
    import rustsasa_amd
    case = tc.get("batch_b")
    want = _want_sasa("batch_b")
    with rustsasa_amd.Context(0) as c:
        dev, _ = _device_run(c, case, want_k=False)
        _assert_values("device", dev, want)
        for rep in range(2):
            atom, _ = c.calculate_sasa_batch(*case.cols, PROBE, 100)
            assert atom.tobytes() == dev.tobytes()
            queued, _ = c.host_batch_enqueue(*case.cols, PROBE, 100)
            c.host_batch_wait()
            assert queued.tobytes() == dev.tobytes()
