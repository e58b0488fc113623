"""The dot patches without a GPU: the model (patches_model.py) pinned to a hand table, to the incremental identity the
kernel rests on, to the component labels and to the guarantees of the header; the stop rule at its edges; every input of
patches_cases.py pinned to what it is named for; the host helpers against direct loops; the binding table; and the new
rules of entry_checks.h in a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import component_cases as cc
import components_model as cm
import depth_model as dm
import geodesics_cases as gc
import geodesics_model as gm
import patches_cases as pc
import patches_model as pmod

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF


def _one(name, n_points=100, link=None):
    """The lists of a one-structure case: (case, link_offsets int64, idx, w float32, dots (qx, qy, qz), mask)."""
    c = pc.get(name)
    link = cc.default_link(c.r, c.probe, n_points) if link is None else F(link)
    off, loff, ent, mask = gm.links(*c.cols[:4], c.ids, c.probe, n_points, link)
    q = dm.dots_of(*c.cols[:4], mask, c.probe, n_points)[1:]
    return c, loff.astype(np.int64), ent["idx"].astype(np.int64), gm.weights(ent), q, mask


# ---- 1: the model --------------------------------------------------------------------------------------------------------

def test_the_ladder_by_hand():
    c, loff, idx, w, q, mask = _one("ladder", 1, 1.0)
    assert mask.shape == (5, 1) and mask.all()                                 # all five points are accessible
    assert q[0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and not q[1].any() and (q[2] == 2.0).all()
    assert loff.tolist() == [0, 1, 3, 5, 7, 8] and (w == 1.0).all()
    centres, cover, dist, src = pmod.sample(loff, idx, w, 0.0)
    assert centres.tolist() == [0, 4, 2, 1, 3] and cover.tolist() == [np.inf, 4.0, 2.0, 1.0, 1.0]
    assert not dist.any() and src.tolist() == [0, 1, 2, 3, 4]
    centres, cover, dist, src = pmod.sample(loff, idx, w, 1.0)
    assert centres.tolist() == [0, 4, 2] and dist.tolist() == [0.0, 1.0, 0.0, 1.0, 0.0] and src.tolist() == [0, 0, 2, 2, 4]
    # link one ulp short: nothing is linked, every dot is its own centre, in order
    _, loff0, idx0, w0, _, _ = _one("ladder", 1, np.nextafter(F(1.0), F(0.0)))
    centres, cover, _, _ = pmod.sample(loff0, idx0, w0, 6.0)
    assert len(w0) == 0 and centres.tolist() == [0, 1, 2, 3, 4] and np.isinf(cover).all()


@pytest.mark.parametrize("name,spacing", [("cavity", 8.0), ("twins", 0.0), ("tiny", 1.5)])
def test_every_pick_is_the_minimum_with_one_more_single_source_run(name, spacing):
    """What the kernel rests on: dist after the pick of c equals min(dist before, single-source dist from c), bit for bit
    - so lowering from the previous values reaches the values of a run from scratch."""
    c = pc.get(name)
    off, loff, ent, _ = gm.links_batch(*c.cols, c.so, c.probe, 100, cc.default_link(c.r, c.probe, 100))
    w = gm.weights(ent)
    seen = []
    for s in range(len(c.so) - 1):
        b, e = int(off[int(c.so[s])]), int(off[int(c.so[s + 1])])
        if e == b:
            continue
        lo = loff[b:e + 1].astype(np.int64)
        sl = slice(int(lo[0]), int(lo[-1]))
        lo, idx, ws = lo - lo[0], ent["idx"][sl].astype(np.int64), w[sl]

        def on_pick(k, c_k, before, after):
            single = gm.dijkstra(lo, idx, ws, gc.one_seed(e - b, c_k))
            assert np.minimum(before, single).tobytes() == after.tobytes(), (name, s, k)
            assert after[c_k] == 0 and (after <= before).all()
            seen.append(k)

        pmod.sample(lo, idx, ws, spacing, None, on_pick)
    assert len(seen) >= (32 if name == "cavity" else 50)


@pytest.mark.parametrize("name,n_points,spacing", [("cavity", 100, 8.0), ("corner", 100, 3.0), ("twins", 100, 0.0),
                                                   ("dot_counts", gc.COUNT_POINTS, 3.0), ("tiny", 100, np.inf)])
def test_labels_cover_order_reach_and_separation(name, n_points, spacing):
    c = pc.get(name)
    link = cc.default_link(c.r, c.probe, n_points)
    lists = gm.links_batch(*c.cols, c.so, c.probe, n_points, link)
    off, c_off, centres, cover, dist, src, mask = pmod.patches_batch(*c.cols, c.so, c.probe, n_points, link, spacing, lists=lists)
    _, labels, _ = cm.components_batch(*c.cols, c.so, c.probe, n_points, link, mask=mask)
    w = gm.weights(lists[2])
    assert (dist <= F(spacing)).all() and (src != NONE).all()
    for s in range(len(c.so) - 1):
        b, e = int(off[int(c.so[s])]), int(off[int(c.so[s + 1])])
        cs, cv = centres[int(c_off[s]):int(c_off[s + 1])], cover[int(c_off[s]):int(c_off[s + 1])]
        lab = np.unique(labels[b:e])
        first = np.isinf(cv)
        assert np.array_equal(cs[first], lab) and first[:len(lab)].all() and not first[len(lab):].any()
        assert (cv[1:] <= cv[:-1]).all() and ((cv > F(spacing)) | first).all()   # (compared directly: inf - inf is NaN)
        assert len(np.unique(cs)) == len(cs) and np.array_equal(np.unique(src[b:e]), np.sort(cs)[np.isin(np.sort(cs), src[b:e])])
        if e == b or name == "cavity":
            continue
        lo = lists[1][b:e + 1].astype(np.int64)
        sl = slice(int(lo[0]), int(lo[-1]))
        for j, cj in enumerate(cs[:12]):                                       # any two centres lie more than spacing apart
            d = gm.dijkstra(lo - lo[0], lists[2]["idx"][sl].astype(np.int64), w[sl], gc.one_seed(e - b, int(cj)))
            later = cs[j + 1:]
            assert (d[later] > F(spacing)).all() and (d[later] >= cv[j + 1:]).all()
    if name == "cavity":
        assert len(centres) == 32 and np.isinf(cover[:2]).all() and np.isfinite(cover[2:]).all()   # two components
    if name == "dot_counts":
        assert mask.sum(axis=1)[c.info["first"]].tolist() == list(gc.COUNTS)
        # an atom's lone dot far from everything else is its own centre; atoms of 63, 64 and 65 dots are sampled
        assert np.diff(c_off.astype(np.int64)).min() >= 1
    if name == "tiny":
        assert np.diff(c_off.astype(np.int64)).tolist() == [1, 0, 1, 0, 1]     # empty structures between others


def test_the_stop_rule_at_its_edges():
    _, loff, idx, w, _, _ = _one("corner")
    n = len(loff) - 1
    centres, cover, dist, _ = pmod.sample(loff, idx, w, 3.0)
    assert len(centres) > 20 and np.isfinite(cover[1:]).all()
    # the picks do not depend on the spacing, only their number does: spacing exactly a cover value stops in front of that
    # pick (m <= spacing), one ulp below takes it and every pick of the same cover
    v = cover[12]
    at, below = pmod.sample(loff, idx, w, v), pmod.sample(loff, idx, w, np.nextafter(v, F(0.0)))
    assert len(at[0]) == int((cover > v).sum()) <= 12 and np.array_equal(at[0], centres[:len(at[0])])
    assert len(below[0]) == int((cover >= v).sum()) >= 13 and np.array_equal(below[0], centres[:len(below[0])])
    assert at[2].max() == v and below[2].max() < v
    # spacing +inf: one centre per component; -0.0 is 0; spacing 0 goes on until every dot is a centre or coincides with one
    one = pmod.sample(loff, idx, w, np.inf)
    assert len(one[0]) == 1 and one[0][0] == 0 and np.isinf(one[1][0]) and np.isfinite(one[2]).all()
    lad = _one("ladder", 1, 1.0)
    for max_centres, k in ((1, 1), (4, 4), (5, 5), (6, 5), (None, 5)):         # 1, D - 1, D, D + 1 of D = 5
        got = pmod.sample(*lad[1:4], 0.0, max_centres)
        assert got[0].tolist() == [0, 4, 2, 1, 3][:k]
        assert np.array_equal(got[2], np.array([[0, 1, 2, 3, 4], [0, 1, 2, 1, 0], [0, 1, 0, 1, 0], [0, 0, 0, 1, 0], [0] * 5][k - 1], F))
    assert pmod.sample(*lad[1:4], -0.0)[0].tolist() == [0, 4, 2, 1, 3]
    # max_centres cuts a component short: finite everywhere, but beyond the spacing; it cuts the components short: +inf stays
    cut = pmod.sample(loff, idx, w, 3.0, 5)
    assert np.array_equal(cut[0], centres[:5]) and cut[2].max() == cover[5] > 3.0
    _, cl, ci, cw, _, _ = _one("cavity")
    cut = pmod.sample(cl, ci, cw, 8.0, 1)
    assert np.isinf(cut[2]).any() and (cut[3][np.isinf(cut[2])] == NONE).all() and (cut[3][np.isfinite(cut[2])] == 0).all()
    assert n > 5


# ---- 2: every case is what it is named for ---------------------------------------------------------------------------------

def test_the_constants_of_the_cases_are_the_kernels():
    text = open(os.path.join(ROOT, "rustsasa_amd", "csrc", "device_types.h")).read()
    assert int(re.search(r"constexpr uint32_t kPsBlock = (\d+);", text).group(1)) == pc.PS_BLOCK
    assert int(re.search(r"constexpr uint32_t kPsQueue = (\d+);", text).group(1)) == pc.PS_QUEUE
    for edge in (pc.PS_BLOCK, pc.PS_QUEUE):
        assert {edge - 1, edge, edge + 1} <= set(pc.LONE_POINTS)
    assert {1, 2, 63, 64, 65, 255, 256, 257, 960} <= set(pc.LONE_POINTS)
    assert pc.PS_QUEUE + 1 in pc.FULL_POINTS and pc.PS_QUEUE + 2 in pc.FULL_POINTS and 960 in pc.FULL_POINTS


@pytest.mark.parametrize("n_points", [1, 2, 65, pc.PS_BLOCK + 1, 960])
def test_a_lone_atom_has_exactly_n_points_dots(n_points):
    _, loff, idx, w, _, mask = _one("lone", n_points)
    assert mask.all() and len(loff) - 1 == n_points
    centres, cover, dist, src = pmod.sample(loff, idx, w, 3.0)
    assert centres[0] == 0 and (dist <= 3.0).all() and (n_points < 3 or len(centres) > 1)


def test_a_full_link_lowers_every_other_dot_in_the_first_step():
    for n_points in (960, pc.PS_QUEUE + 2):
        _, loff, idx, w, _, _ = _one("lone", n_points, pc.FULL_LINK)
        assert (np.diff(loff) == n_points - 1).all()
        # after the first pick every other dot has its value from the centre's own list or lower: one step lowers them all
        first = gm.dijkstra(loff, idx, w, gc.one_seed(n_points, 0))
        assert np.isfinite(first).all() and (first[1:] <= w[:n_points - 1][np.argsort(idx[:n_points - 1])]).all()
    assert pc.PS_QUEUE + 2 - 1 > pc.PS_QUEUE >= 960 - 1                        # 960 fits the queue as built, 1026 does not


def test_twins_chain_and_mixed_are_what_they_are_named_for():
    # twins: coincident dots, zero weights, exact ties in the argmax
    _, loff, idx, w, _, _ = _one("twins")
    ties = []
    pmod.sample(loff, idx, w, 0.0, None, lambda k, c, before, after: ties.append(int((before == before.max()).sum())))
    assert (w == 0).sum() >= 180 and max(ties[1:]) >= 2
    centres, _, dist, src = pmod.sample(loff, idx, w, 0.0)
    assert len(centres) < len(dist) and not dist.any() and (src <= np.arange(len(src))).all() and (src != np.arange(len(src))).any()
    # chain: the first pick runs more than 200 steps
    _, loff, idx, w, _, _ = _one("chain")
    assert gm.hops(loff, idx, gc.one_seed(len(loff) - 1, 0)).max() >= 200
    # mixed: structures that end at different picks, empty ones among them
    c = pc.get("mixed")
    got = pmod.patches_batch(*c.cols, c.so, c.probe, 100, cc.default_link(c.r, c.probe, 100), 6.0)
    per = np.diff(got[1].astype(np.int64))
    assert len(c.so) - 1 == 8 and per[1] == per[3] == 0 and len(set(per.tolist())) >= 3 and per.max() > 7


def test_jcd_at_twelve_angstrom():
    c, loff, idx, w, _, _ = _one("jcd")
    assert c.n_atoms == 1052 and len(loff) - 1 == 7417 and len(w) == 59516
    centres, cover, dist, _ = pmod.sample(loff, idx, w, 12.0)
    assert len(centres) == 38 and (dist <= 12.0).all()


# ---- 3: the helpers, the binding table, the rules -----------------------------------------------------------------------------

def test_helpers_against_direct_loops():
    import rustsasa_amd
    c = pc.get("mixed")
    link = cc.default_link(c.r, c.probe, 100)
    for max_centres in (1, None):                                            # (1 leaves the void of cavity unreached)
        off, c_off, centres, cover, dist, src, _ = pmod.patches_batch(*c.cols, c.so, c.probe, 100, link, 6.0, max_centres)
        D, K, S = int(off[-1]), len(centres), len(c.so) - 1
        dso = [int(off[int(s)]) for s in c.so]
        # dot_seeds_from
        want = np.zeros(D, np.uint8)
        for s in range(S):
            for k in range(int(c_off[s]), int(c_off[s + 1])):
                want[dso[s] + int(centres[k])] = 1
        seeds = rustsasa_amd.dot_seeds_from(c_off, centres, off, c.so)
        assert seeds.dtype == np.uint8 and np.array_equal(seeds, want) and int(want.sum()) == K
        # ... and they reproduce dist and source in the model
        g = gm.geodesics_batch(*c.cols, c.so, c.probe, 100, link, seeds)
        assert g[1].tobytes() == dist.tobytes() and np.array_equal(g[2], src)
        # patch_index
        want = np.full(D, -1, np.int64)
        for s in range(S):
            mine = {int(centres[k]): k for k in range(int(c_off[s]), int(c_off[s + 1]))}
            for d in range(dso[s], dso[s + 1]):
                if src[d] != NONE:
                    want[d] = mine[int(src[d])]
        which = rustsasa_amd.patch_index(off, src, c_off, centres, c.so)
        assert which.dtype == np.int64 and np.array_equal(which, want)
        assert ((which < 0).any()) == (max_centres == 1) and np.array_equal(which < 0, np.isinf(dist))
        # patch_table
        R = (c.r + F(c.probe)).astype(np.float64)
        owner = np.repeat(np.arange(c.n_atoms), np.diff(off.astype(np.int64)))
        rows = rustsasa_amd.patch_table(off, src, c_off, centres, c.r, c.probe, 100, c.so)
        assert [a.dtype for a in rows] == [np.int64, np.uint32, np.int64, np.int64, np.float64] and all(len(a) == K for a in rows)
        for k in range(K):
            d = np.flatnonzero(want == k)
            area = 0.0
            for i in d:
                area += 4.0 * np.pi * R[owner[i]] ** 2 / 100
            s = int(np.searchsorted(c_off.astype(np.int64), k, side="right")) - 1
            assert rows[0][k] == s and rows[1][k] == centres[k] and rows[2][k] == len(d) and rows[3][k] == len(set(owner[d]))
            assert abs(rows[4][k] - area) <= 1e-9 * max(area, 1.0)
        reached = np.bincount(owner[want >= 0], minlength=c.n_atoms) * (4.0 * np.pi * R * R / 100)
        for s in range(S):
            assert abs(rows[4][rows[0] == s].sum() - reached[int(c.so[s]):int(c.so[s + 1])].sum()) < 1e-6
    # one structure without structure_offsets, and the errors
    lad = pmod.patches_batch(*pc.get("ladder").cols, pc.get("ladder").so, 1.0, 1, F(1.0), 1.0)
    assert rustsasa_amd.patch_index(lad[0], lad[5], lad[1], lad[2]).tolist() == [0, 0, 2, 2, 1]
    assert rustsasa_amd.dot_seeds_from(lad[1], lad[2], lad[0]).tolist() == [1, 0, 1, 0, 1]
    assert rustsasa_amd.patch_table(lad[0], lad[5], lad[1], lad[2], np.ones(5, F), 1.0, 1)[2].tolist() == [2, 1, 2]
    with pytest.raises(ValueError):
        rustsasa_amd.patch_index(lad[0], lad[5][:-1], lad[1], lad[2])
    with pytest.raises(ValueError):
        rustsasa_amd.patch_index(lad[0], lad[5], lad[1], np.array([0, 4, 9], np.uint32))
    with pytest.raises(ValueError):
        rustsasa_amd.patch_index(lad[0], np.array([0, 1, 2, 2, 4], np.uint32), lad[1], lad[2])      # dot 1 is no centre
    with pytest.raises(ValueError):
        rustsasa_amd.dot_seeds_from(np.array([0, 2], np.uint64), lad[2], lad[0])


def test_binding_table_and_the_documents():
    from rustsasa_amd import _capi
    import rustsasa_amd
    header = open(os.path.join(ROOT, "include", "rustsasa_amd.h")).read()
    assert "#define RSASA_ABI_VERSION 4" in header
    assert "rsasa_dot_patches, rsasa_dot_patches_batch; rsasa_context_patch_stats. */" in header
    for name, n_args in (("rsasa_dot_patches", 23), ("rsasa_dot_patches_batch", 24), ("rsasa_context_patch_stats", 2)):
        assert f"int {name}(" in header
        res, args = _capi.SYMBOLS[name]
        assert res is C.c_int and len(args) == n_args
    p = _capi.SYMBOLS["rsasa_dot_patches_batch"][1]
    assert p[10] is C.c_float and p[11] is C.c_float and p[12] is C.c_uint32        # link, spacing, max_centres
    assert p[18] is C.c_size_t and p[21] is C.c_size_t                              # centres_capacity, dots_capacity
    p = _capi.SYMBOLS["rsasa_dot_patches"][1]
    assert p[6] is C.c_size_t and p[9] is C.c_float and p[10] is C.c_float and p[11] is C.c_uint32 and p[17] is C.c_size_t
    lib = _capi.load()
    assert all(hasattr(lib, n) for n in ("rsasa_dot_patches", "rsasa_dot_patches_batch", "rsasa_context_patch_stats"))
    assert lib.rsasa_abi_version() == 4
    for name in ("dot_patches", "dot_patches_batch", "patch_stats"):
        assert callable(getattr(rustsasa_amd.Context, name))
    for name in ("patch_index", "patch_table", "dot_seeds_from"):
        assert name in rustsasa_amd.__all__ and callable(getattr(rustsasa_amd, name))
    docs = {"README": open(os.path.join(ROOT, "README.md")).read(), "DESIGN": open(os.path.join(ROOT, "DESIGN.md")).read(),
            "INTEGRATION": open(os.path.join(ROOT, "INTEGRATION.md")).read()}
    assert "WHERE TO PUT THE PATCHES" in docs["README"] and "WHERE TO PUT THE PATCHES" in header
    assert "## 5q. Dot patches" in docs["DESIGN"] and "rsasa_dot_patches" in docs["INTEGRATION"]
    for doc in docs.values():
        assert "dot_patches" in doc
    srcs = open(os.path.join(ROOT, "rustsasa_amd", "csrc", "Makefile")).read()
    assert " patches.hip " in srcs and "-ffp-contract=off" in srcs


def test_python_argument_checks_without_a_gpu():
    """The checks Context.dot_patches makes before it reaches the library, on a Context that has none (no call below gets
    as far as the C entry point: each must raise first)."""
    import rustsasa_amd
    ctx = object.__new__(rustsasa_amd.Context)              # no device, no handle, no library
    c = pc.get("tiny")
    one = lambda **kw: ctx.dot_patches(*c.part(2), c.probe, 100, **kw)                     # noqa: E731
    many = lambda **kw: ctx.dot_patches_batch(*c.cols, c.so, c.probe, 100, **kw)          # noqa: E731
    for call in (one, many):
        for spacing in (-1.0, float("nan"), -float("inf"), -1e-30):
            with pytest.raises(ValueError, match="spacing must be"):
                call(spacing=spacing)
        for max_centres in (0, -1, 2 ** 32):
            with pytest.raises(ValueError, match="max_centres must be"):
                call(max_centres=max_centres)
        with pytest.raises(ValueError):
            call(spacing="wide")
        for kw in ({}, {"spacing": 0.0}, {"spacing": -0.0}, {"spacing": float("inf"), "max_centres": 1}, {"max_centres": 2 ** 32 - 1}):
            with pytest.raises(AttributeError):             # the checks pass; the Context has no library to call
                call(**kw)
    with pytest.raises(ValueError, match="n_points"):
        ctx.dot_patches(*c.part(2), c.probe, 0)


def test_new_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "patch_checks_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "rustsasa_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "patch_checks_test.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "patch checks ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-2000:])


def test_the_bench_tool_records_the_resources_of_the_file_head():
    """tools/bench_patches.py writes its KERNELS table into profiles/patches_bench.json beside the times; the table, the
    one in the head of patches.hip and the committed record must be the same numbers, and none uses scratch."""
    import ast
    import json
    head = open(os.path.join(ROOT, "rustsasa_amd", "csrc", "patches.hip")).read().split("#include")[0]
    rows = re.findall(r"^//   (k_\w+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", head, re.M)
    want = {n: {"vgprs": int(v), "sgprs": int(s), "lds_bytes": int(lds), "scratch": int(sc)} for n, v, s, lds, sc in rows}
    assert sorted(want) == ["k_patch_init", "k_patch_pack", "k_patch_sample"] and all(r["scratch"] == 0 for r in want.values())
    tool = open(os.path.join(ROOT, "tools", "bench_patches.py")).read()
    table = ast.literal_eval(re.search(r"^KERNELS = (\{.*?\}\})$", tool, re.M | re.S).group(1))
    assert table == want
    record = json.load(open(os.path.join(ROOT, "profiles", "patches_bench.json")))
    assert record["kernels"] == want and [c["workload"] for c in record["cases"]] == ["proteome", "real_coords"]
    assert record["queue"] == pc.PS_QUEUE and record["workgroup"] == pc.PS_BLOCK
    for case in record["cases"]:
        assert all(v["loop_returns_the_same_centres_and_dist"] for v in case["host_loop"].values())
