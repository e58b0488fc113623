"""The cases of dot_edge2_cases.py without a GPU: each pinned, from the models alone (geodesics_model.py,
patches_model.py, sweep_model.py), to what it is named for - the path of row(N) and the rounds it can take, the hub whose
second step lowers exactly n_disc dots, the two first steps of two_full that outgrow the queue, the four centre counts of
rows_batch, the run step of crowded_cells that stages more than a wave of atoms - and the table of runs that puts the
shared sweep's cases through the dot-link kernels."""
import functools
import os
import re

import numpy as np
import pytest

import component_cases as cc
import depth_cases as dc
import dot_edge2_cases as d2
import geodesics_cases as gc
import geodesics_model as gm
import patches_cases as pc
import patches_model as pmod
import points_model as pm
import sweep_cases as sc
import sweep_model as sm

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _one(name, n_points, link):
    """The lists of a one-structure case: (case, link_offsets int64, idx, w float32, mask)."""
    c = d2.get(name)
    off, loff, ent, mask = gm.links(*c.cols[:4], c.ids, c.probe, n_points, F(link))
    return c, loff.astype(np.int64), ent["idx"].astype(np.int64), gm.weights(ent), mask


# ---- the constants and the table of runs -------------------------------------------------------------------------------------

def test_the_constants_of_the_cases_are_the_kernels():
    text = open(os.path.join(ROOT, "rustsasa_amd", "csrc", "device_types.h")).read()
    assert int(re.search(r"constexpr uint32_t kGdRounds = (\d+);", text).group(1)) == d2.GD_ROUNDS
    assert int(re.search(r"constexpr uint32_t kPsQueue = (\d+);", text).group(1)) == d2.PS_QUEUE == pc.PS_QUEUE
    assert d2.GD_ROUNDS in range(1, d2.ROW_MAX) and d2.GD_ROUNDS + 1 <= d2.ROW_MAX and 2 * d2.GD_ROUNDS + 1 <= d2.ROW_MAX
    assert d2.HUB_DISCS == (d2.PS_QUEUE, d2.PS_QUEUE + 1, 1200) and d2.TWO_FULL_POINTS - 1 == d2.PS_QUEUE + 1
    assert d2.ROWS_STRUCTURES > 2 * 256 and d2.ROWS_PERIOD == d2.ROW_MAX + 1


def test_the_runs_of_the_shared_sweep_s_cases():
    names = [n for n, _ in d2.LIST_RUNS]
    assert set(names) == set(sc.CASES) and d2.LIST_RUNS[:-1] == sc.runs() and d2.LIST_RUNS[-1] == ("margin_twelve", 100)
    assert all(run in d2.LIST_RUNS for run in d2.WEIGHT_RUNS)
    # the weights are observed on every case of several structures, on crowded_cells and on chain
    several = {n for n in names if len(d2.case(n).so) > 2}
    assert several == {"column_z", "margin_under", "margin_over", "margin_twelve", "margin_small_h", "half_link", "odd_beside_even"}
    assert {n for n, _ in d2.WEIGHT_RUNS} == several | {"crowded_cells", "chain"}
    assert d2.link_of("half_link", cc.FAR_POINTS) == sc.HALF_LINK == cc.H * F(0.5)
    # odd_beside_even: ball's link, not the 35 A that its radius of 64.5 asks for
    o = sc.get("odd_beside_even")
    assert 1.73 < d2.link_of("odd_beside_even", 100) == d2.ball_link() < 1.75 and 34.0 < cc.default_link(o.r, o.probe, 100) < 36.0
    for name in ("margin_under", "crowded_cells", "chain", "column_z"):
        c = sc.get(name)
        assert d2.link_of(name, sc.points_of(name)[0]) == cc.default_link(c.r, c.probe, sc.points_of(name)[0])
    # crowded_cells: link 0, ball's, its own, and at 65 points one whose reach is the whole grid
    c = sc.get("crowded_cells")
    l100, l65 = d2.crowded_links(100), d2.crowded_links(65)
    assert len(l100) == 3 and len(l65) == 4 and l100[0] == l65[0] == 0 and l100[1] == l65[1] == d2.ball_link()
    assert 11.3 < l100[2] < 11.5 and 14.0 < l65[2] < 14.2
    g = sm.grid(*c.cols[:4], c.probe)
    far = int(g.dims.max()) - 1                                 # the last shell any sweep of this grid can have
    assert l65[3] == F(4.0) * g.h and sm.s_end_of(l65[3], g.h, far, True) == far
    assert d2.CROSS_RUNS[:2] == [("half_link", cc.FAR_POINTS), ("crowded_cells", 65)] and len(d2.CROSS_RUNS) == 8
    assert d2.cross_link("crowded_cells", 65) == d2.ball_link() and d2.cross_link("half_link", cc.FAR_POINTS) == sc.HALF_LINK
    assert d2.finite_limit("margin_small_h") == pytest.approx(0.18) and d2.finite_limit("chain") == 6.0


def test_crowded_cells_stages_more_than_a_wave_of_atoms_in_one_run_step():
    """k_dot_link stages the atoms of a run step that own dots, 64 at a time: the step of the own cell (shell 0) of an atom
    in the ball holds more than 64 of them, so the loop over f0 goes round more than once with something to stage.  The
    masks are ball's and one free atom (test_sweep_cpu.py pins that identity)."""
    c, b = sc.get("crowded_cells"), dc.get("ball")
    free = np.append(pm.exposed_masks_batch(*b.cols, b.so, b.probe, 100, 8).any(axis=1), True)
    g = sm.grid(*c.cols[:4], c.probe)
    most, later = 0, 0
    for i in range(0, c.n_atoms - 1, 7):
        for s in (0, 1):
            for flat in sm.shell_steps(g, i, s)[0]:
                own = free[g.order[flat]]
                most = max(most, int(own.sum()))
                later = max(later, int(own[sm.WAVE:].sum()))
    assert most > sm.WAVE and later >= 1           # atoms that own dots beyond the first 64 of a step


def test_the_middle_seed_is_not_a_structure_s_first_dot():
    """A batch-wide dot number stored without, or with the wrong, first dot of the structure only shows where a seed's
    number within its structure differs from its number in the batch and from 0."""
    for name, n_points in (("half_link", cc.FAR_POINTS), ("margin_twelve", 100)):
        c = d2.case(name)
        off = gm.links_batch(*c.cols, c.so, c.probe, n_points, F(0.0))[0].astype(np.int64)
        seeds = np.flatnonzero(d2.middle_seeds(off, c.so))
        first = off[c.so.astype(np.int64)[:-1]]
        assert len(seeds) == len(c.so) - 1 >= 12 and (seeds > first).all() and (first[1:] > 0).all()
    c = d2.rows_batch()
    off = np.arange(c.n_atoms + 1)
    last = np.flatnonzero(d2.last_seeds(off, c.so))
    assert len(last) == 568 and np.array_equal(last, off[c.so.astype(np.int64)[1:]][np.diff(c.so.astype(np.int64)) > 0] - 1)


# ---- B: row(N) ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", range(1, d2.ROW_MAX + 1))
def test_row_is_a_path_of_unit_weights(n):
    c, loff, idx, w, mask = _one("row%d" % n, 1, d2.ROW_LINK)
    assert mask.shape == (n, 1) and mask.all() and len(w) == 2 * (n - 1) and (w == 1.0).all()
    assert np.diff(loff).tolist() == ([0] if n == 1 else [1] + [2] * (n - 2) + [1])
    line = np.arange(n, dtype=F)
    first, last = gc.one_seed(n, 0), gc.one_seed(n, n - 1)
    d = gm.dijkstra(loff, idx, w, first)
    assert d.tolist() == line.tolist() and not gm.sources_of(loff, idx, w, d, first).any()
    assert gm.hops(loff, idx, first).max() == n - 1              # n - 1 rounds settle it, one more finds nothing: n at most
    d = gm.dijkstra(loff, idx, w, last)
    assert d.tolist() == line[::-1].tolist() and (gm.sources_of(loff, idx, w, d, last) == n - 1).all()
    both = first | last
    d = gm.dijkstra(loff, idx, w, both)
    assert d.tolist() == np.minimum(line, line[::-1]).tolist()
    assert gm.sources_of(loff, idx, w, d, both).tolist() == [0 if v <= n - 1 - v else n - 1 for v in range(n)]
    limit = (n - 1) / 2
    d = gm.dijkstra(loff, idx, w, first, limit)
    assert d.tolist() == [float(v) if v <= limit else np.inf for v in range(n)]
    assert gm.sources_of(loff, idx, w, d, first).tolist() == [0 if v <= limit else NONE for v in range(n)]


# ---- C: hub, two_full, rows_batch -----------------------------------------------------------------------------------------------

def test_the_disc_and_exact_coordinates():
    xy = d2.disc_points()
    assert len(xy) == d2.HUB_LATTICE == 1257 and np.array_equal(xy, xy[np.lexsort((xy[:, 1], xy[:, 0]))])
    assert np.array_equal(xy * 8, np.round(xy * 8)) and (np.hypot(xy[:, 0], xy[:, 1]) <= 2.5).all()
    c = d2.hub(1200)
    assert c.n_atoms == 1202 and not c.z.any() and (c.r == 1).all() and c.probe == 1.0
    assert (c.x[0], c.y[0], c.x[1], c.y[1]) == (16.0, 0.0, 7.0, 0.0) and np.array_equal(np.stack([c.x[2:], c.y[2:]], -1), xy[:1200])


@pytest.mark.parametrize("n_disc", d2.HUB_DISCS)
def test_the_hub_s_second_step_lowers_exactly_the_disc(n_disc):
    c, loff, idx, w, mask = _one("hub%d" % n_disc, 1, d2.HUB_LINK)
    n = n_disc + 2
    L = np.diff(loff)
    assert mask.all() and len(loff) - 1 == n and L[0] == 1 and L[1] == n_disc + 1
    assert idx[loff[0]:loff[1]].tolist() == [1] and w[loff[0]:loff[1]].tolist() == [9.0]          # the hub, 9 away
    assert sorted(idx[loff[1]:loff[2]].tolist()) == [0] + list(range(2, n)) and w[loff[1]:loff[2]].max() <= 9.5
    d0 = np.hypot(c.x[2:].astype(np.float64) - 16.0, c.y[2:].astype(np.float64))
    assert d0.min() >= 13.5 and (L[2:] == n_disc).all()                                           # the disc: the hub and each other
    seen = []
    centres, cover, dist, src = pmod.sample(loff, idx, w, np.inf, None, lambda *a: seen.append(a))
    assert centres.tolist() == [0] and np.isinf(cover).all() and len(seen) == 1 and not src.any()
    k, c0, before, after = seen[0]
    assert c0 == 0 and np.isinf(before).all()
    # step 1 pushes along dot 0's list: the hub alone.  Step 2 pushes along the hub's: dot 0 stays 0, every disc dot falls
    # from +inf - and the hub's own value cannot fall meanwhile, for nothing but dot 0 and the disc could lower it
    hub_list, hub_w = idx[loff[1]:loff[2]], w[loff[1]:loff[2]]
    direct = np.full(n, np.inf, F)
    direct[hub_list] = F(9.0) + hub_w
    direct[0], direct[1] = 0.0, 9.0
    assert after[1] == 9.0 and np.isfinite(direct[2:]).all() and (after <= direct).all()
    # what the steps after the second still have to do: a few two-hop paths round below the direct one, so a pick that
    # stopped pushing once its queue had overflowed would leave wrong bits
    assert 1 <= (after < direct).sum() < n_disc // 8


@pytest.mark.parametrize("spacing,max_centres", [(3.0, None), (0.0, 40)])
def test_later_picks_on_the_hub_start_from_the_disc(spacing, max_centres):
    for n_disc in d2.HUB_DISCS[1:]:
        _, loff, idx, w, _ = _one("hub%d" % n_disc, 1, d2.HUB_LINK)
        first_steps = []

        def on_pick(k, c, before, after):
            mine = slice(loff[c], loff[c + 1])
            first_steps.append(int((w[mine] < before[idx[mine]]).sum()))

        centres = pmod.sample(loff, idx, w, spacing, max_centres, on_pick)[0]
        assert centres[:3].tolist() == [0, 2, 1] and len(centres) == (5 if max_centres is None else 40)
        # the second pick, a disc dot, lowers most of the disc in its first step: an overflow of the first step right after
        # the pick whose second step overflowed; the later picks lower few dots and queue them
        assert first_steps[0] == 1 and first_steps[1] > d2.PS_QUEUE // 2 and min(first_steps[2:]) < 64


def test_two_full_overflows_in_the_first_step_of_both_picks():
    c, loff, idx, w, mask = _one("two_full", d2.TWO_FULL_POINTS, d2.TWO_FULL_LINK)
    P = d2.TWO_FULL_POINTS
    assert mask.all() and len(loff) - 1 == 2 * P and (np.diff(loff) == P - 1).all()
    assert (idx[:loff[P]] < P).all() and (idx[loff[P]:] >= P).all()                 # no link between the atoms
    assert 6.3 < w.max() <= F(6.32) < d2.TWO_FULL_LINK < d2.TWO_FULL_APART - 6.4
    lowered = []

    def on_pick(k, ck, before, after):
        mine = slice(loff[ck], loff[ck + 1])
        lowered.append((ck, int((w[mine] < before[idx[mine]]).sum())))

    centres, cover, dist, src = pmod.sample(loff, idx, w, np.inf, None, on_pick)
    assert centres.tolist() == [0, P] and np.isinf(cover).all() and np.isfinite(dist).all()
    assert lowered == [(0, d2.PS_QUEUE + 1), (P, d2.PS_QUEUE + 1)]
    assert (src[:P] == 0).all() and (src[P:] == P).all()
    # as two structures: the same lists per atom, each with its own first pick
    b = d2.two_full_batch()
    assert len(b.so) == 3 and b.n_atoms == 2 and np.array_equal(b.x, c.x) and np.array_equal(b.r, c.r)


def test_rows_batch_and_its_four_centre_counts():
    c = d2.rows_batch()
    per = np.diff(c.so.astype(np.int64))
    assert len(per) == d2.ROWS_STRUCTURES == 600 and per.tolist() == [s % 19 for s in range(600)]
    assert c.n_atoms == 5356 and (per == 0).sum() == 32
    lists = gm.links_batch(*c.cols, c.so, c.probe, 1, d2.ROW_LINK)
    assert lists[3].all() and int(lists[0][-1]) == 5356 and len(lists[2]) == 2 * int(np.maximum(per - 1, 0).sum())
    for (spacing, max_centres), K in zip(d2.ROWS_RUNS, d2.ROWS_CENTRES):
        got = pmod.patches_batch(*c.cols, c.so, c.probe, 1, d2.ROW_LINK, spacing, max_centres, lists=lists)
        assert len(got[2]) == K == int(got[1][-1])
        k_s = np.diff(got[1].astype(np.int64))
        if spacing == 0.0:
            assert np.array_equal(k_s, per if max_centres is None else np.minimum(per, max_centres))
        elif np.isinf(spacing):
            assert np.array_equal(k_s, np.minimum(per, 1))
    assert d2.ROWS_CENTRES == (5356, 2602, 568, 1104)
    assert int(np.minimum(per, 2).sum()) == 1104                                # the bound of max_centres = 2 is its K here
    seeds = d2.last_seeds(lists[0], c.so)
    _, dist, src, _ = gm.geodesics_batch(*c.cols, c.so, c.probe, 1, d2.ROW_LINK, seeds, lists=lists)
    want = np.concatenate([np.arange(n)[::-1] for n in per]).astype(F)
    assert dist.tobytes() == want.tobytes() and np.array_equal(src, np.repeat(np.maximum(per - 1, 0), per))
