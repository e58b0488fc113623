"""k_atom_depth (depth.hip) and k_component_link (components.hip) against the exact CPU models on the cases of
sweep_cases.py, which sit at the edges of the sweep both kernels share (pinned by test_sweep_cpu.py from the emulation
alone): 24 shells through a grid 3 cells wide, winners in an inside row's low and high cell at large s, structures just
under and just over the 65536 h limit of the margins in one launch, a structure that stops early beside two that must
sweep everything, cells of a hundred atoms, a winner in a shell's rows past the first 64, a chain of 384 atoms against
the cell order.  No tolerances anywhere: minima of keys and graph components have no order."""
import functools

import numpy as np
import pytest

import component_cases as cc
import components_model as cm
import depth_cases as dc
import depth_model as dm
import point_edge_cases as pe
import points_model as pm
import sweep_cases as sc
import test_gpu_components as tgc
import test_gpu_depth as tgd

pytestmark = pytest.mark.gpu

F = np.float32
RUNS = sc.runs()
MARGIN_OUTPUTS = ("depth", "nearest", "free", "sasa", "labels")


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _masks(name, n_points):
    c = sc.get(name)
    return pm.exposed_masks_batch(*c.cols, c.so, c.probe, n_points, 8)


@pytest.fixture(scope="module", autouse=True)
def _all_masks():
    pe.pmap(lambda run: _masks(*run), RUNS)          # side by side, once


def _link(c, n_points):
    return cc.default_link(c.r, c.probe, n_points)


def _depth_model(name, n_points):
    c = sc.get(name)
    return dm.atom_depth_batch(*c.cols, c.so, c.probe, n_points, mask=_masks(name, n_points))


def _components_model(name, n_points, link):
    c = sc.get(name)
    return cm.components_batch(*c.cols, c.so, c.probe, n_points, link, mask=_masks(name, n_points))


# ---- every case against the models ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n_points", RUNS)
def test_depth_equals_the_model(ctx, name, n_points):
    c = sc.get(name)
    got = ctx.atom_depth_batch(*c.cols, c.so, c.probe, n_points)
    words, sasa = ctx.accessible_points_batch(*c.cols, c.so, c.probe, n_points)
    # free and sasa against the other point call first: a disagreement with the model below is then the masks' or the sweep's
    assert np.array_equal(got[2].astype(np.int64), pe.popcount(words)) and got[3].tobytes() == sasa.tobytes()
    tgd._check(got, _depth_model(name, n_points), c.r, c.probe, n_points)


@pytest.mark.parametrize("name,n_points", RUNS)
def test_components_equal_the_model(ctx, name, n_points):
    c = sc.get(name)
    link = sc.HALF_LINK if name == "half_link" else _link(c, n_points)
    got = ctx.surface_components_batch(*c.cols, c.so, c.probe, n_points, None if name != "half_link" else link)
    tgc._check(got, _components_model(name, n_points, link), c.r, c.probe, n_points)


@pytest.mark.parametrize("n_points", sc.CROWDED_POINTS)
def test_crowded_cells_at_link_zero_and_at_a_link_over_the_whole_grid(ctx, n_points):
    c = sc.get("crowded_cells")
    wide = F(4.0) * (F(c.probe) + c.r.max())
    for link in (F(0.0), wide):
        got = ctx.surface_components_batch(*c.cols, c.so, c.probe, n_points, link)
        tgc._check(got, _components_model("crowded_cells", n_points, link), c.r, c.probe, n_points)
    assert not got[1].any()                                      # the wide link: one component


def test_chain_three_times_on_one_context(ctx):
    c = sc.get("chain")
    first = ctx.surface_components_batch(*c.cols, c.so, c.probe, 100)
    assert not first[1].any() and len(first[1]) > 10000          # one component
    for _ in range(2):
        again = ctx.surface_components_batch(*c.cols, c.so, c.probe, 100)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


# ---- the margins' flag is per structure ----------------------------------------------------------------------------------------

def _both(ctx, c):
    """{output: [bytes per structure]} of the depth and the components call on a batch; labels per structure."""
    depth, nearest, free, sasa = ctx.atom_depth_batch(*c.cols, c.so, c.probe, 100)
    off, labels, free2, sasa2 = ctx.surface_components_batch(*c.cols, c.so, c.probe, 100)
    assert free.tobytes() == free2.tobytes() and sasa.tobytes() == sasa2.tobytes()
    out = {k: [] for k in MARGIN_OUTPUTS}
    for s in range(len(c.so) - 1):
        b, e = int(c.so[s]), int(c.so[s + 1])
        for k, a in zip(MARGIN_OUTPUTS[:4], (depth, nearest, free, sasa)):
            out[k].append(a[b:e].tobytes())
        out["labels"].append(labels[int(off[b]):int(off[e])].tobytes())
    return out


def test_margin_structures_alone_in_the_batch_of_twelve_and_beside_their_counterpart(ctx):
    twelve = _both(ctx, sc.get("margin_twelve"))
    for n in range(6):
        pair = _both(ctx, sc.margin_pair(n))
        for w, which in enumerate(("under", "over")):
            c = sc.get("margin_" + which)
            alone = _both(ctx, dc._case("alone", [c.part(n)[:4] + (None,)]))
            for k in MARGIN_OUTPUTS:
                assert alone[k][0] == twelve[k][2 * n + w], (n, which, k, "twelve")
                assert alone[k][0] == pair[k][w], (n, which, k, "pair")


def test_the_even_structure_beside_the_odd_ones_equals_ball_alone(ctx):
    o, b = sc.get("odd_beside_even"), dc.get("ball")
    n = b.n_atoms
    got = ctx.atom_depth_batch(*o.cols, o.so, o.probe, 100)
    alone = ctx.atom_depth(*b.cols, b.probe, 100)
    for k in range(4):
        assert got[k][:n].tobytes() == alone[k].tobytes(), k
    off, labels, _, _ = ctx.surface_components_batch(*o.cols, o.so, o.probe, 100)
    a_off, a_labels, _, _ = ctx.surface_components(*b.cols, b.probe, 100)
    assert np.array_equal(off[:n + 1], a_off) and np.array_equal(labels[:int(off[n])], a_labels)
