"""The inputs of test_gpu_tail_edges.py (tail_cases.py) are what that file relies on: every structure's grid has the
intended dimensions, the cell scan's chunk, tiles per workgroup, active workgroups and uint4 remainder are the ones each
case is named for, the structures are placed where the batches mean them to be, and every atom sits among neighbours
where the scan's seams are - from the grid formula and the placement arithmetic restated in numpy (tail_cases.layout)
and the oracle's neighbour lists.  No GPU, nothing of the engine."""
import numpy as np
import pytest

import nb_helpers as nh
import tail_cases as tc

ALL = sorted(tc.CASES) + ["trajectory"]


def _case(name):
    return tc.trajectory_case() if name == "trajectory" else tc.get(name)


@pytest.mark.parametrize("name", ALL)
def test_grids_and_scan_figures_are_the_intended_ones(name):
    case = _case(name)
    L = tc.layout(case)
    for s, st in enumerate(case.structures):
        if st.dims is not None:
            assert L.dims[s] == tuple(st.dims), (name, s)
            assert L.n_cells[s] == int(np.prod(st.dims))
        if s in L.cell_base:
            assert st.dims is not None and len(st) >= tc.LDS_MAX_ATOMS
    got = dict(entries=L.tail_entries, chunk=L.chunk, tiles=L.tiles, active=L.active, mod4=L.mod4)
    assert got == case.expect, name
    assert L.tail_entries == sum(L.n_cells[s] for s in L.cell_base) + 1
    assert L.chunk * tc.SCAN_BLOCKS >= L.tail_entries > (L.chunk - tc.TILE) * tc.SCAN_BLOCKS
    assert L.n_cells_sum < 2 ** 31


def test_what_each_case_is_named_for():
    L = {n: tc.layout(_case(n)) for n in ALL}
    a = L["2^20"]
    # 2^20 entries: one tile each, every workgroup active and full, nothing clamped; alone, so the tail begins at 0
    assert a.tail_entries == tc.SCAN_BLOCKS * tc.TILE and a.tiles == 1 and a.active == tc.SCAN_BLOCKS
    assert a.tail_cell_begin == 0 and a.tail_atom_base == 0
    b = L["2^20+1"]
    # one entry more: two tiles each, the last active workgroup holds the end sentinel alone, 511 are clamped
    assert b.tiles == 2 and b.active == 513 and (b.tail_entries - 1) == (b.active - 1) * b.chunk
    assert tc.SCAN_BLOCKS - b.active == 511
    assert L["five_tiles"].tiles >= 5
    assert {1, 2, 3} <= {v.mod4 for v in L.values()}
    # small x * y layers: the empty last z layer is a short end of the range
    for n in ("2^20+1", "five_tiles"):
        d = L[n].dims[0]
        assert d[0] * d[1] <= 2 * tc.TILE and d[2] > 1000

    ca, la = tc.get("batch_a"), L["batch_a"]
    assert [len(s) for s in ca.structures] == [65536, 65537, 70000] and ca.tails() == [0, 1, 2]
    assert 65537 % tc.SEGMENT_ATOMS == 1                                   # a last bounds segment of one atom
    assert len(set(la.dims)) == 3
    assert [la.cell_base[s] % 4 for s in (1, 2)] == [1, 2]

    for n in ("batch_b", "batch_b_dup"):
        cb, lb = tc.get(n), L[n]
        t = cb.tails()
        sizes = [len(s) for s in cb.structures]
        assert len(t) == 3 and t[0] == 0 and t[-1] == len(sizes) - 1
        # the later tail structures are placed by the second workgroup of k_grid_params / k_grid_bases
        assert t[1] >= tc.STRUCTS_PER_BLOCK and t[2] >= tc.STRUCTS_PER_BLOCK
        between = sizes[t[0] + 1:t[1]]
        assert 0 in between and sizes[t[1] + 1:t[2]] == [400]
        assert any(0 < m < tc.LDS_MAX_ATOMS and lb.n_cells[t[0] + 1 + k] > 3 * tc.WINDOW_CELLS
                   for k, m in enumerate(between))
        assert lb.tail_cell_begin > 0 and lb.tail_cell_begin % 1024 == 0 and lb.tail_atom_base > 0
        # (lds_cell_slots is a multiple of 8: cells_s is never odd; an odd number of eights is what can be had)
        assert lb.cells_s % 8 == 0 and (lb.cells_s // 8) % 2 == 1
        assert [lb.cell_base[s] % 4 for s in t[1:]] == [1, 2]

    lc = L["batch_c"]
    assert tc.get("batch_c").tails() == [0, 1, 2, 3] and lc.tiles >= 2
    assert [lc.cell_base[s] % 4 for s in (1, 2, 3)] == [0, 1, 2]

    lt = L["trajectory"]
    assert len(set(lt.dims)) == tc.N_FRAMES and min(lt.n_cells) > 1 << 20 and lt.tiles >= 3


def _tail_structures():
    """Every distinct tail structure of the cases, by name."""
    out = {}
    for n in ALL:
        case = _case(n)
        for s in case.tails():
            st = case.structures[s]
            if not any(st is o for o in out.values()):
                out[f"{n}[{s}]"] = st
    return out


def test_every_tail_atom_sits_among_neighbours():
    """At least 99 % of a tail structure's atoms have two neighbours or more in the oracle's lists, and the mean list
    holds 8 or more: a sparse input - where most atoms have no neighbour and SASA is the full sphere wherever the atom
    was binned - cannot pass as a test of binning."""
    sts = _tail_structures()
    assert len(sts) == 9   # 2^20, 2^20 + 1, five tiles, the three of batch (a), the three frames

    def one(key):
        st = sts[key]
        offs, _ = nh.oracle_csr(st.x, st.y, st.z, st.r, None, tc.PROBE)
        k = np.diff(offs.astype(np.int64))
        return float(np.mean(k >= 2)), float(k.mean())
    import point_edge_cases as pe
    for key, (frac, mean) in pe.pmap(one, sts).items():
        assert frac >= 0.99 and mean >= 8.0, (key, frac, mean)


def _occupied_in(L, lo, hi):
    a, b = np.searchsorted(L.occupied, [lo, hi])
    return b > a


@pytest.mark.parametrize("name", ALL)
def test_atoms_sit_at_the_seams_of_the_scan(name):
    case = _case(name)
    L = tc.layout(case)
    assert len(L.occupied) and L.occupied[-1] < L.tail_entries - 1
    # the last workgroup whose range holds a cell that can hold an atom (the last structure's cell of the atom at its
    # far corner: every later cell is in the padding) has occupied cells - by that atom at the least
    s = case.tails()[-1]
    d = L.dims[s]
    last_cell = L.cell_base[s] + (d[0] - 2) + (d[1] - 2) * d[0] + (d[2] - 2) * d[0] * d[1]
    assert L.occupied[-1] == last_cell
    w = last_cell // L.chunk
    assert _occupied_in(L, w * L.chunk, min((w + 1) * L.chunk, L.tail_entries))
    if L.tiles > 1:
        # occupied cells in the first and in the last tile of one workgroup (the carry between tiles is observed)
        both = [w for w in range(L.active) if _occupied_in(L, w * L.chunk, w * L.chunk + tc.TILE) and
                _occupied_in(L, (w + 1) * L.chunk - tc.TILE, (w + 1) * L.chunk)]
        assert len(both) >= 10, (name, len(both))
    if len(case.tails()) > 1:
        # every structure has a chunk boundary inside its cells with occupied cells on both sides
        for s in case.tails():
            lo, hi = L.cell_base[s], L.cell_base[s] + L.n_cells[s]
            edges = [e for e in range(-(-lo // L.chunk) * L.chunk, hi, L.chunk) if lo < e < hi and
                     _occupied_in(L, lo, e) and _occupied_in(L, e, hi)]
            assert edges, (name, s)


def test_duplicate_ids_matter():
    """batch_b_dup: the second tail structure's shared ids remove entries from the oracle's lists."""
    plain, dup = tc.get("batch_b"), tc.get("batch_b_dup")
    s = dup.tails()[1]
    b, e = int(dup.so[s]), int(dup.so[s + 1])
    assert np.array_equal(plain.ids[:b], dup.ids[:b]) and np.array_equal(plain.ids[e:], dup.ids[e:])
    assert len(np.unique(dup.ids[b:e])) < (e - b) // 4
    assert not np.all(np.diff(dup.ids[b:e].astype(np.int64)) > 0)
    st = dup.structures[s]
    k0 = np.diff(nh.oracle_csr(st.x, st.y, st.z, st.r, plain.ids[b:e], tc.PROBE)[0].astype(np.int64))
    k1 = np.diff(nh.oracle_csr(st.x, st.y, st.z, st.r, dup.ids[b:e], tc.PROBE)[0].astype(np.int64))
    assert np.all(k1 <= k0) and int(np.sum(k1 < k0)) > (e - b) // 2
