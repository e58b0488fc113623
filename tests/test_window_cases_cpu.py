"""The inputs of test_gpu_window_edges.py (window_cases.py) reach the limits of k_sort_window they are named for: every
structure's grid has the intended dimensions and the intended atoms in every window, the last windows have the cell
counts, parities, counter words and paddings of the issue's table, the ladder's sizes give the slot, chunk and trip
counts on both sides of every threshold, the staging structures put whole cells of slot atoms and of rest atoms on both
sides of position 2 304, the dense structures end a 16-bit cursor at 65 535 in either half of a word, and the pairs of
equal ids change values - from the grid formula and the kernel's arithmetic restated in numpy (tail_cases.py,
window_cases.py) and the oracle.  No GPU, nothing of the engine."""
import numpy as np
import pytest

import nb_helpers as nh
import tail_cases as tc
import window_cases as wc
from oracle import pyoracle as po

W = wc.W
ALL = sorted(wc.BUILDERS)


def test_every_structure_is_listed():
    assert set(wc.EXPECT) == set(wc.BUILDERS)
    used = {n for names in wc.BATCHES.values() for n in names} | set(wc.SINGLE_CASES)
    assert used == set(wc.BUILDERS)


@pytest.mark.parametrize("name", ALL)
def test_grid_windows_and_atoms_per_window(name):
    st = wc.structure(name)
    dims, atoms = wc.EXPECT[name]
    cell, d = wc.cells_of(st)
    assert d == dims, name
    if st.dims is not None:
        assert tuple(st.dims) == dims
    n_cells = int(np.prod(dims))
    assert len(atoms) == wc.n_windows(n_cells) and sum(atoms) == len(st) < tc.LDS_MAX_ATOMS
    assert wc.window_atoms(st) == atoms, name
    # no cell coordinate was lowered by the clamp: "the top layer is empty" holds, and a cell is floor((x - min) / 2)
    assert wc.clamp_lowered(st) == 0
    if len(st):
        assert int(cell.min()) >= 0 and int(cell.max()) < n_cells
        assert st.r.max() == np.float32(tc.R_MAX) and tc.grid_of(st.x, st.y, st.z, st.r)[1] == np.float32(0.5)
    # ids: all different but for the pairs, in no order
    assert st.ids.dtype == np.uint64 and len(np.unique(st.ids)) == len(st) - len(st.pairs)
    if len(st) > 2:
        steps = np.diff(st.ids.astype(np.float64))
        assert np.any(steps > 0) and np.any(steps < 0)


# name -> (cells, cells of the last window, odd, counter words, words % 19, 16-byte stores of cell starts,
#          16-bit entries of padding behind the end marker, the last window holds atoms)
TABLE = {
    "thin_W+1": (W + 1, 1, 1, 1, 1, 1, 6, False),
    "thin_2W+2": (2 * W + 2, 2, 0, 1, 1, 1, 5, False),
    "thin_2W+38": (2 * W + 38, 38, 0, 19, 0, 5, 1, False),
    "thick_3W+38": (3 * W + 38, 38, 0, 19, 0, 5, 1, False),
    "thick_3W+1": (3 * W + 1, 1, 1, 1, 1, 1, 6, False),
    "lattice_3W-1": (3 * W - 1, W - 1, 1, W // 2, 2, W // 8, 0, True),
    "thick_3W+8": (3 * W + 8, 8, 0, 4, 4, 2, 7, False),
}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_last_window_is_the_one_of_the_table(name):
    n_cells, last, odd, n_words, mod_per, stores, padding, populated = TABLE[name]
    dims, atoms = wc.EXPECT[name]
    assert int(np.prod(dims)) == n_cells and min(dims) >= 4
    lw = wc.last_window(n_cells)
    assert lw == dict(n_cells=last, odd=odd, n_words=n_words, words_mod_per=mod_per, start_stores=stores, padding=padding)
    # the end marker: with an odd number of cells the upper half of the last counter word, else the word after - the
    # first word of the next thread's run of kPer when the words are a multiple of kPer
    assert (2 * n_words == last + 1) == bool(odd)
    assert stores == -(-(last + 1) // 8)
    assert (atoms[-1] > 0) == populated
    if not populated:   # the whole last window lies in the top z layer, which holds no atom
        assert (len(atoms) - 1) * W >= (dims[2] - 1) * dims[0] * dims[1]
    assert all(a > 0 for a in atoms[:-1])   # every other window holds atoms
    for single in ("single_" + name,):
        if single in wc.EXPECT:
            assert wc.EXPECT[single][0] == dims and all(a > 0 for a in wc.EXPECT[single][1][:-1])
            assert len(wc.structure(single)) == 4097


def test_window_without_an_atom_between_two_that_have_some():
    dims, atoms = wc.EXPECT["hole"]
    assert dims == wc.DIMS["thick_3W+1"] and atoms[1] == 0 and atoms[0] > 0 and atoms[2] > 0   # total = 0, placed > 0


def test_ladder_sizes_slots_chunks_and_trips():
    assert wc.LADDER == (1, 2, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12287, 12288, 12289)
    slots = {n: min(8, -(-n // wc.THREADS)) for n in wc.LADDER}             # slot k is loaded iff 1024 k < n
    assert [slots[n] for n in wc.LADDER] == [1, 1, 1, 1, 2, 4, 4, 5, 8, 8, 8, 8, 8, 8]
    assert [n > wc.CHUNK_ATOMS for n in wc.LADDER] == [False] * 7 + [True] * 7   # the record pass's second chunk
    assert {n: wc.rest_atoms(n) for n in wc.LADDER[8:]} == {
        8191: (0, 0, 0), 8192: (0, 0, 0), 8193: (1, 1, 1), 12287: (4095, 1, 4095), 12288: (4096, 1, 0), 12289: (4097, 2, 1)}
    assert 4096 % tc.SEGMENT_ATOMS == 0 and 4097 % tc.SEGMENT_ATOMS == 1     # the seam of k_bounds
    for n in wc.LADDER:
        st = wc.structure(f"ladder_{n}")
        dims, atoms = wc.EXPECT[f"ladder_{n}"]
        assert len(st) == n and atoms == [n] and int(np.prod(dims)) <= W      # a one-window grid of its own
    grids = [tc.grid_of(*(getattr(wc.structure(f"ladder_{n}"), k) for k in "xyzr"))[0] for n in wc.LADDER]
    assert len({tuple(g.tolist()) for g in grids}) == len(wc.LADDER)           # every grid has its own origin
    case = wc.get("ladder")
    assert case.n_atoms == 76803 and np.diff(case.so.astype(np.int64)).tolist() == list(wc.LADDER)
    assert not np.any(case.so[1:-1] % 4 == 0)                                 # no structure starts at an aligned atom
    rev = wc.get("ladder_reversed")
    sizes = np.diff(rev.so.astype(np.int64)).tolist()
    assert sizes == list(wc.LADDER[:6:-1]) + [0] + list(wc.LADDER[6::-1]) and len(sizes) == 15 and sizes[7] == 0
    # (the reversed order has the aligned starts the first batch has none of: the structure of 8 193 atoms starts at
    # 36 864 and three more at multiples of 4 096, k_bounds' segment)
    assert [int(o) for o in rev.so[1:-1] if o % 4 == 0] == [36864, 61440, 73728, 76800]
    assert all(o % tc.SEGMENT_ATOMS == 0 for o in (36864, 61440, 73728))


def test_interleaved_batch_puts_structures_behind_an_unpadded_marker():
    names = wc.names_of("interleaved")
    k = names.index("lattice_3W-1")
    assert names[k + 1:k + 4] == ["empty", "ladder_1025", "thin_W+1"] and k > 0 and len(names) > k + 4
    n_cells = [int(np.prod(wc.EXPECT[n][0])) for n in names]
    base = np.concatenate([[0], np.cumsum([tc.lds_cell_slots(c) for c in n_cells])])   # cell_base (k_grid_bases)
    assert base[k + 1] - base[k] == n_cells[k] + 1          # the empty structure's cell_base follows the marker directly
    assert base[k + 2] - base[k + 1] == 8 and len(wc.EXPECT["ladder_1025"][1]) == 1
    assert wc.n_cells_sum("interleaved") == sum(n_cells)
    L = tc.layout(wc.get("interleaved"))
    assert L.n_cells == n_cells and L.cells_s == base[-1] and not L.cell_base


@pytest.mark.parametrize("name,want", [
    ("stage_2303", dict(slot_staged=2303, slot_direct=0, rest_staged=0, rest_direct=0)),
    ("stage_2304", dict(slot_staged=2304, slot_direct=0, rest_staged=0, rest_direct=0)),
    # (one atom past the staging area, and it is alone in its cell: its way out is known)
    ("stage_2305", dict(slot_staged=2304, slot_direct=1, rest_staged=0, rest_direct=0)),
    ("stage_mixed", dict(slot_staged=1873, slot_direct=578, rest_staged=431, rest_direct=118)),
])
def test_staging_populations(name, want):
    st = wc.structure(name)
    dims, atoms = wc.EXPECT[name]
    assert dims == wc.DIMS_STAGE and atoms[:3] == list(wc.STAGE_COUNTS[name]) and atoms[3] == 0
    assert wc.STAGE == 2304 and [wc.STAGE_COUNTS[n][1] for n in ("stage_2303", "stage_2304", "stage_2305")] == [2303, 2304, 2305]
    assert atoms[0] > 0                                      # placed > 0 in window 1
    got = wc.staging_populations(st, 1)
    assert got == want
    if name == "stage_mixed":
        assert len(st) > wc.SLOT_ATOMS and min(got.values()) >= 50
        # the id pair: both atoms in window 1, in cells on opposite sides of position 2 304
        cell, start, end = wc.runs_of(st)
        (i, j), = st.pairs
        assert cell[i] // W == 1 and cell[j] // W == 1
        assert sorted([(int(end[i]) <= wc.STAGE) - (int(start[i]) >= wc.STAGE),
                       (int(end[j]) <= wc.STAGE) - (int(start[j]) >= wc.STAGE)]) == [-1, 1]
    else:
        assert len(st) <= wc.SLOT_ATOMS


@pytest.mark.parametrize("name,odd,window", [("dense_even", 0, 0), ("dense_odd", 1, 3)])
def test_dense_structures_end_a_cursor_at_65535(name, odd, window):
    st = wc.structure(name)
    assert len(st) == 65535 == tc.LDS_MAX_ATOMS - 1
    cell, start, end = wc.runs_of(st)
    count = np.bincount(cell)
    assert count.max() > 40000 and int(count.argmax()) // W == window
    dense = cell == count.argmax()
    xyz = np.stack([st.x, st.y, st.z], -1)[dense]
    assert len(np.unique(xyz, axis=0)) == len(xyz) and np.all(np.ptp(xyz, axis=0) < 2.0)
    # the last occupied cell's cursor ends at 65 535 = 0xFFFF, in the low half of its word (even cell) or the upper one
    last = int(cell.max())
    placed = int(np.sum(cell < (last // W) * W))
    assert int(end[cell == last][0]) + placed == 65535
    assert ((last - (last // W) * W) & 1) == odd
    assert wc.EXPECT[name][0] == wc.DIMS_DENSE[name]


def _cases_with_ids():
    return list(wc.SORT_CASES) + list(wc.SINGLE_CASES)


@pytest.mark.parametrize("case", _cases_with_ids())
def test_id_pairs_change_values(case):
    """Every case of (a), (b), (c), (e) holds a pair of equal ids inside a structure that changes the oracle's values
    (one atom cannot: ladder_1).  pair_matters decides on the atoms within 12 A; for the smaller structures the whole
    structure's values are compared as well."""
    sts = [wc.structure(n) for n in (wc.names_of(case) if case in wc.BATCHES else [case])]
    n_pairs = 0
    for st in sts:
        for i, j in st.pairs:
            assert i < j and st.ids[i] == st.ids[j]
            assert wc.pair_matters(st, i, j)
            n_pairs += 1
            if len(st) <= 4400:
                with_ids = po.calculate_sasa_internal(st.x, st.y, st.z, st.r, st.ids, wc.PROBE, wc.N_POINTS, 8)
                without = po.calculate_sasa_internal(st.x, st.y, st.z, st.r, None, wc.PROBE, wc.N_POINTS, 8)
                assert with_ids[i] != without[i] or with_ids[j] != without[j]
    assert n_pairs >= 1 or case == "ladder_1"
    if case in ("ladder", "ladder_reversed"):
        # structures whose ids are all different (the sort drops them) beside ones that keep them; past 8 192 atoms
        # the pair's later atom is a rest atom
        assert 0 < sum(1 for st in sts if st.pairs) < len(sts)
        for st in sts:
            if len(st) > wc.SLOT_ATOMS and st.pairs:
                assert st.pairs[0][1] >= wc.SLOT_ATOMS > st.pairs[0][0]


@pytest.mark.parametrize("case", list(wc.SORT_CASES) + ["dense"])
def test_census_reaches_every_cell_and_every_atom(case):
    """The census cutoff lies beyond every pair of the structure, and the stop rule of cutoff_sweep.h
    (c2 <= ((s - 0.5) h)^2, h = 2) cannot be met before the shells cover the grid (s_last <= the largest dimension - 1)."""
    c = wc.get(case)
    cutoff = wc.census_cutoff(case)
    fl = wc.census_flags(case)
    assert np.all((fl == 1) | (fl == 3))
    for s, st in enumerate(c.structures):
        if not len(st):
            continue
        dims = wc.EXPECT[wc.names_of(case)[s]][0]
        assert cutoff >= 4.0 * wc.extent(st) and np.float32(cutoff) ** 2 > ((max(dims) - 1 - 0.5) * 2.0) ** 2
        xyz = np.stack([st.x, st.y, st.z], -1).astype(np.float64)
        centres = wc.census_centres(len(st))
        assert np.flatnonzero(fl[int(c.so[s]):int(c.so[s + 1])] == 3).tolist() == centres
        assert {0, len(st) - 1} <= set(centres) and (len(st) <= wc.SLOT_ATOMS or wc.SLOT_ATOMS in centres)
        for i in centres:
            assert np.sqrt(((xyz - xyz[i]) ** 2).sum(-1)).max() < 0.5 * cutoff


def test_single_cases_are_on_both_sides_of_the_limit():
    sizes = [len(wc.structure(n)) for n in wc.SINGLE_CASES]
    assert sizes == [1, 1024, 1025, 4096, 4097, 8191, 8192, 8193, 4097, 4097, 4097]
    assert sum(n <= wc.SINGLE_ATOMS for n in sizes) == 10
    for n in wc.SINGLE_CASES:   # (small_grid takes up to 64 windows)
        assert len(wc.EXPECT[n][1]) <= 64
    for n in sizes:
        ro = wc.residue_offsets(n)
        assert np.all(np.diff(ro.astype(np.int64)) >= 0) and int(ro[-1]) <= n
        assert int(ro[-1]) - int(ro[0]) < n                  # the offsets do not cover all atoms
        if n > 24:
            assert ro[0] > 0 and ro[-1] < n and np.any(np.diff(ro.astype(np.int64)) == 0)


def test_atoms_sit_among_neighbours():
    """SASA and the neighbour lists are witnesses only where atoms have neighbours: in every structure of 1 000 atoms or
    more, at least 95 % of the atoms have two neighbours or more in the oracle's lists."""
    import point_edge_cases as pe
    names = [n for n in ALL if len(wc.structure(n)) >= 1000 and not n.startswith("dense")]

    def one(name):
        st = wc.structure(name)
        k = np.diff(nh.oracle_csr(st.x, st.y, st.z, st.r, None, wc.PROBE)[0].astype(np.int64))
        return float(np.mean(k >= 2))
    for name, frac in pe.pmap(one, names).items():
        assert frac >= 0.95, (name, frac)
