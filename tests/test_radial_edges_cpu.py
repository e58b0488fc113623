"""The cases of radial_edge_cases.py without a GPU: each pinned to what it is named for from radial_model.py alone - the
ladder's partner k in bin k - 1 at every n_bins (one ulp further out in bin k, or nowhere), the first of several equal
edges taking the pair, the overflowing edges' empty bins, the offsets of chunk_batch on the chunk edges of k_radial_pairs,
a chunk without a class - and the emulated sweep of k_radial_counts (radial_model.sweep_counts: its stop rule at the last
edge) against the plain model on the awkward grids, the margin structures and the exact ties at the margins' edge."""
import numpy as np
import pytest

import cutoff_edge_cases as ce
import hse_cases as hc
import radial_cases as rc
import radial_edge_cases as re_
import radial_model as rm

F = np.float32


def _ladder_counts(c, edges, flags="own"):
    return rm.counts(c.x, c.y, c.z, edges, re_.ladder_classes(), re_.N_CLASSES, c.flags if flags == "own" else flags)


# ---- the ladder ----------------------------------------------------------------------------------------------------------

def test_ladder_is_built_as_described():
    for moved in (False, True):
        c = re_.ladder(moved)
        assert c.n_atoms == 33 and c.flags.tolist() == [2] + [1] * 32 and re_.ladder_classes().tolist() == [0] + [0, 1, 2, 3] * 8
        assert (c.x[0], c.y[0], c.z[0]) == tuple(F(v) for v in hc.TIE_ORIGIN)
        assert np.all(c.y == c.y[0]) and np.all(c.z == c.z[0])
        dx = c.x[1:] - c.x[0]
        k = np.arange(1, 33, dtype=F)
        e2 = rm.e2_of(re_.ladder_edges(32))
        assert np.array_equal(e2, k * k)
        if moved:
            assert np.all(dx > k) and np.all(dx * dx > e2) and np.all(dx * dx < rm.e2_of(np.arange(2, 34))), "one ulp, not a bin"
            assert np.array_equal(c.x[1:], np.nextafter(re_.ladder().x[1:], F(np.inf)))
        else:
            assert np.array_equal(dx, k) and np.array_equal(dx * dx, e2)           # d2 == e2 exactly


@pytest.mark.parametrize("n_bins", range(1, 33))
def test_ladder_partner_k_lands_in_bin_k_minus_1(n_bins):
    edges = re_.ladder_edges(n_bins)
    assert edges == tuple(float(k) for k in range(1, n_bins + 1))
    got = _ladder_counts(re_.ladder(), edges)
    want = np.zeros((re_.N_CLASSES, n_bins), np.uint32)
    for k in range(1, n_bins + 1):
        want[(k - 1) % 4, k - 1] = 1                                    # ... and nowhere else; partners beyond n_bins nowhere
    assert np.array_equal(got[0], want) and not got[1:].any() and got[0].sum() == n_bins
    assert np.array_equal(re_.ladder_row(edges), want)
    got = _ladder_counts(re_.ladder(True), edges)
    want = np.zeros((re_.N_CLASSES, n_bins), np.uint32)
    for k in range(1, n_bins):
        want[(k - 1) % 4, k] = 1                                        # the next bin; partner n_bins is beyond the last edge
    assert np.array_equal(got[0], want) and not got[1:].any() and got[0].sum() == n_bins - 1
    assert np.array_equal(re_.ladder_row(edges, True), want)
    # every atom a centre and a partner: the model's rows are what the GPU test compares with
    both = _ladder_counts(re_.ladder(), edges, None)
    assert both[0].sum() == n_bins and both[16].sum() == 2 * min(n_bins, 16)      # sixteen atoms on either side of atom 16


def test_bin_counts_take_every_padded_size_and_first_step():
    def half_of(n_bins):                                                # k_radial_counts' first step
        half = 1
        while 2 * half < n_bins:
            half <<= 1
        return 0 if n_bins == 1 else half
    assert {half_of(n) for n in range(1, 33)} == {0, 1, 2, 4, 8, 16}
    assert [half_of(n) for n in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)] == [0, 1, 2, 2, 4, 4, 8, 8, 16, 16]


@pytest.mark.parametrize("n_bins", re_.REPEAT_BINS)
def test_the_first_of_equal_edges_takes_the_pair(n_bins):
    edges = re_.ladder_edges(n_bins, repeated=True)
    assert edges[:7] == (1.0, 2.0, 2.0, 2.0, 5.0, 5.0, 7.0)[:n_bins] and len(edges) == n_bins
    assert all(a <= b for a, b in zip(edges, edges[1:])) and (n_bins < 4 or len(set(edges)) < n_bins)
    e = np.array(edges)
    later = np.flatnonzero(np.concatenate([[False], e[1:] == e[:-1]]))  # the second, third edge of a run
    for moved in (False, True):
        got = _ladder_counts(re_.ladder(moved), edges)
        assert not got[0][:, later].any() and not got[1:].any()
        assert np.array_equal(got[0], re_.ladder_row(edges, moved))
    got = _ladder_counts(re_.ladder(), edges)
    assert got[0].sum() == int(e[-1])                                   # everybody up to the last edge counts once
    if n_bins >= 5:
        assert got[0][:, 4].sum() == 3 and got[0][:, 1].sum() == 1      # 3, 4 and 5 meet the first 5; 2 the first 2


# ---- overflowing squares -----------------------------------------------------------------------------------------------------

def test_overflowing_edges_leave_their_bins_empty():
    c = hc.cluster()
    e2 = rm.e2_of(re_.OVERFLOW_EDGES)
    assert np.isfinite(e2[:2]).all() and np.isinf(e2[2:]).all() and e2[1] > 1e37 and re_.OVERFLOW_EDGES[3] == float(np.finfo(F).max)
    cl = rc.case_classes("cluster")
    got = rm.counts(c.x, c.y, c.z, re_.OVERFLOW_EDGES, cl, rc.N_CLASSES, None)
    assert not got[:, :, 2:].any() and got[:, :, 1].any() and got[:, :, 0].any()
    assert np.all(got.sum(axis=(1, 2)) == c.n_atoms - 1)


# ---- the pair kernel's batches ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", sorted(re_.LAYOUTS))
def test_chunk_batch_has_its_structures_on_the_chunk_edges(layout):
    c, x = re_.chunk_batch(False, layout), re_.chunk_batch(True, layout)
    assert c.n_atoms == 4096 == 4 * re_.CHUNK and x.n_atoms == 4097
    so = c.so.astype(np.int64).tolist()
    assert so[:5] == [0, 0, 1024, 1024, 1024] and so[-3:] == [4096] * 3 and len(so) == 9
    assert x.so.astype(np.int64).tolist() == so[:-2] + [4097] * 3      # one atom, then the two empty structures
    assert x.x[:4096].tobytes() == c.x.tobytes()
    sizes = np.diff(c.so.astype(np.int64))
    if layout == "edges":
        assert 2048 in so and sizes.max() == 2048
    else:
        big = int(np.argmax(sizes))
        assert sizes[big] == 2500 and so[big] // 1024 == 1 and (so[big + 1] - 1) // 1024 == 3      # chunks 1, 2 and 3
    xyz = np.stack([c.x, c.y, c.z], -1)
    assert xyz.min() >= 0.0 and xyz.max() <= re_.BOX < 3 * float(c.h) and float(c.h) == float(F(1.4) + F(1.5))


def test_pair_shapes_and_the_chunk_without_a_class():
    cells = [a * b for a, b in re_.PAIR_SHAPES]
    assert cells == [1, 3, 256, 260, 512]

    def width(n):                                                       # k_radial_pairs' sub-group width
        w = 1
        while w < n and w < re_.PAIR_THREADS:
            w <<= 1
        return w
    assert [width(n) for n in cells] == [1, 4, 256, 256, 256]
    assert [max(0, n - re_.PAIR_THREADS) for n in cells] == [0, 0, 0, 4, 256]     # threads that hold a second cell
    for n in (4096, 4097):
        cl = re_.chunk_classes(n, 16)
        missing = [(c, k) for c in range(-(-n // 1024)) for k in range(16) if not (cl[c * 1024:(c + 1) * 1024] == k).any()]
        assert (1, 8) in missing and len(missing) >= 4
        assert set(cl.tolist()) == set(range(16))                        # every class somewhere
        for n_classes, _ in re_.PAIR_SHAPES:
            cl = re_.chunk_classes(n, n_classes)
            assert cl.dtype == np.uint8 and cl.max() == n_classes - 1 and len(cl) == n


def test_most_cells_of_the_chunk_tables_are_non_zero():
    c = re_.chunk_batch(False, "span")
    b, e = int(c.so[4]), int(c.so[5])
    cl = re_.chunk_classes(c.n_atoms, 16)
    t = rm.counts(c.x[b:e], c.y[b:e], c.z[b:e], re_.chunk_edges(32), cl[b:e], 16, None)
    assert (t != 0).mean() > 0.5
    pairs = rm.pairs_from_counts(t, [0, e - b], cl[b:e])
    assert (pairs != 0).mean() > 0.9


# ---- the emulated sweep on the awkward grids and at the margins' edge ---------------------------------------------------------------

@pytest.mark.parametrize("name", ce.GRID_NAMES + ce.MARGIN_NAMES)
def test_sweep_equals_the_model_on_the_adapted_grid_cases(name):
    c = ce.swept(name)
    cl = re_.swept_classes(name)
    n_struct = len(c.so) - 1
    lists = re_.swept_edge_lists(name)
    full = re_.swept_edges(name)
    assert len(lists) == 5 and lists[3] == full and len(lists[4]) == 1  # four prefixes and the covering edge
    assert [len(e) for e in lists[:4]] == [1, 2, 3, 4] and all(a <= b for a, b in zip(full, full[1:]))
    assert set(ce.cell_cutoffs(c)) < set(full) == {e[-1] for e in lists[:4]}      # every equality cutoff is once the last edge
    mid = lists[full.index(ce.cell_cutoffs(c)[1])]
    ruled = 0
    for s in (range(n_struct) if n_struct <= 6 else (0, 1, 5, 10, 11)):
        p = hc.part(c, s)
        b, e = int(c.so[s]), int(c.so[s + 1])
        sample = ce.ends_sample(c, s, n=4)
        for edges in (mid, full):                                       # (3/2) h as the last edge: equality; the full list
            want = rm.counts(p.x, p.y, p.z, edges, cl[b:e], re_.N_CLASSES, None)
            rows, stop, by_rule, _ = rm.sweep_counts(p.x, p.y, p.z, p.r, p.probe, edges, cl[b:e], re_.N_CLASSES, None, sample)
            assert np.array_equal(rows, want[sample]), (name, s, edges)
            ruled += int(by_rule.sum())
            if edges == mid and ce.margins_of(c, s):
                assert np.all(stop[by_rule] == 2)                       # c2 <= ((2 - 1/2) h)^2 with equality: after shell 2
    # (margin_over fails the margins; odd_beside_even's cutoffs follow its radius of 70 and cover the even structure's grid)
    assert ruled > 0 or name in ("margin_over", "odd_beside_even")


@pytest.mark.parametrize("axis,sign", ce.DIRECTIONS)
def test_sweep_keeps_the_ties_of_edge_at_the_margins_edge(axis, sign):
    for which in ce.WHICH:
        c = ce.edge_at_margin(axis, sign, which)
        cl = re_.grid_classes(c, 760)
        centres = [c.info["hi"], c.info["lo"]]
        for edges in re_.EDGE_LISTS:
            want = rm.counts(c.x, c.y, c.z, edges, cl, re_.N_CLASSES, None)
            rows, stop, by_rule, _ = rm.sweep_counts(c.x, c.y, c.z, c.r, c.probe, edges, cl, re_.N_CLASSES, None, centres)
            assert np.array_equal(rows, want[centres]), (which, edges)
            assert by_rule.all() == (which == "under") and by_rule.any() == (which == "under")
        want = rm.counts(c.x, c.y, c.z, re_.EDGE_LISTS[0], cl, re_.N_CLASSES, None)[centres]
        assert want[:, :, 1].sum(1).tolist() == [6, 6]                  # the six ties, in the last bin
        if which == "under":
            short = rm.sweep_counts(c.x, c.y, c.z, c.r, c.probe, re_.EDGE_LISTS[0], cl, re_.N_CLASSES, None, centres, half=-0.5)
            assert short[1].tolist() == [2, 2] and short[0].sum(axis=(1, 2)).tolist() == [3, 3]    # a rule one shell early bites


def test_thread_rotation_covers_every_call_on_every_input():
    seen = {(call, ce.thread_input(t, it)) for t in range(re_.THREADS) for it in range(re_.THREAD_ROUNDS)
            for call in re_.thread_calls(t, it)[:1]}
    assert seen == {(c, i) for c in re_.THREAD_CALLS for i in ce.THREAD_INPUTS}          # as the first call of a round
    assert all(sorted(re_.thread_calls(t, it)) == sorted(re_.THREAD_CALLS) for t in range(8) for it in range(10))
