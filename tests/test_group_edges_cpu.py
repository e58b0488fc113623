"""The inputs of the group-contact edge tests (group_edge_cases.py) pinned to the classes they are named for, from the
oracle's neighbour lists and the labels alone - no library output is read here - and groups_model.py against whole
runs of the oracle on the new cluster labellings: own prefixes and foreign runs longer than an LDS stage, which the
protein-length lists of test_groups_cpu.py never reach.  No GPU; every comparison is exact."""
import numpy as np
import pytest

import group_edge_cases as ge
import groups_model as gm
import nb_helpers as nh
import point_edge_cases as pe
import tail_cases as tl
import tie_cases as tc

STAGE = pe.PT_STAGE


def _cluster_classes(n, kind, shared_ids=False):
    cols, g, c0 = ge.cluster(n, kind, shared_ids)
    offs, ent = nh.oracle_csr(*cols, ge.PROBE)
    k = np.diff(offs.astype(np.int64))
    n_own, rows, runs = ge.list_classes(offs, ent, g)
    return cols, g, c0, k, n_own, rows, runs


@pytest.mark.parametrize("n", ge.CLUSTER_SIZES)
def test_cluster_lists_are_the_whole_cluster(n):
    cols, c0 = nh.tight_cluster(n, seed=n)
    k = np.diff(nh.oracle_csr(*cols, ge.PROBE)[0].astype(np.int64))
    assert k[c0:].min() == k[c0:].max() == n - 1 and k[:c0].max() < STAGE
    assert -(-(n - 1) // STAGE) == {258: 2, 514: 3, 769: 3}[n] and n - 1 > STAGE


@pytest.mark.parametrize("n", ge.CLUSTER_SIZES)
def test_class_one_label(n):
    _, _, c0, k, n_own, rows, _ = _cluster_classes(n, "one_label")
    assert np.all(n_own[c0:] == n - 1) and n - 1 in (257, 513, 768) and n - 1 > STAGE   # an own prefix of every stage
    assert not rows[c0:].any()


def test_class_head_against_rest():
    last_group = {}
    for n in ge.CLUSTER_SIZES:
        _, _, c0, k, n_own, rows, runs = _cluster_classes(n, "head_against_rest")
        # the head: no own entry, one foreign run that covers whole stages
        assert n_own[c0] == 0 and rows[c0] == 1 and runs[c0].tolist() == [n - 1] and n - 1 > STAGE
        # the rest: several stages of own entries, then one foreign entry, the last of the list
        assert np.all(n_own[c0 + 1:] == n - 2) and np.all(rows[c0 + 1:] == 1) and n - 2 >= STAGE
        assert all(runs[i].tolist() == [1] for i in range(c0 + 1, c0 + n))
        last = n - 2                                  # its position in the reordered list
        assert last == k[c0 + 1] - 1
        last_group[n] = (k[c0 + 1] % 4, last % STAGE)
    # the last group of four: one entry and three of padding (twice), and full
    assert [last_group[n][0] for n in ge.CLUSTER_SIZES] == [1, 1, 0]
    assert [last_group[n][1] for n in ge.CLUSTER_SIZES] == [0, 0, 255]    # the first and the last slot of a stage


def test_class_own_then_many():
    want_rows = {514: 214, 769: 469}
    assert [n for n, kind in ge.cluster_keys() if kind == "own_then_many"] == [514, 769]
    for n in (514, 769):
        _, g, c0, k, n_own, rows, runs = _cluster_classes(n, "own_then_many")
        block = slice(c0, c0 + ge.OWN_BLOCK)
        rest = slice(c0 + ge.OWN_BLOCK, c0 + n)
        assert np.all(n_own[block] == 299) and STAGE < 299 < 2 * STAGE          # ends inside the second stage
        assert np.all(rows[block] == want_rows[n]) and np.all(rows[rest] == want_rows[n])
        assert all(runs[i].tolist() == [1] * want_rows[n] for i in range(c0, c0 + ge.OWN_BLOCK))
        # from the others: the block's run of 300 comes first (its label is the smallest), then runs of one
        assert np.all(n_own[rest] == 0) and g[c0] < g[rest].min()
        assert all(runs[i].tolist() == [300] + [1] * (want_rows[n] - 1) for i in range(c0 + ge.OWN_BLOCK, c0 + n))
        own = g[rest].astype(np.int64)
        assert own.min() > 1 << 31 and len(set(own.tolist())) == len(own) and np.any(np.diff(own) < 0) \
            and np.any(np.diff(own) > 0)
    assert want_rows[514] < ge.ROW_REGS < want_rows[769]                        # both sides of the register rows


def test_class_two_long_runs():
    for n in ge.CLUSTER_SIZES:
        _, g, c0, k, n_own, rows, runs = _cluster_classes(n, "two_long_runs")
        half = (n - 1) // 2
        assert n_own[c0] == 0 and rows[c0] == 2 and runs[c0].tolist() == [half, n - 1 - half]
        assert g[c0] < g[c0 + 1] < g[c0 + n - 1]
        assert half % STAGE != 0 or n == 514          # the seam: inside a stage, or (n = 514) exactly between two
        # a B atom: its own half, then the head's run of one and the whole of C
        assert n_own[c0 + 1] == half - 1 and runs[c0 + 1].tolist() == [1, n - 1 - half]
        # a C atom: the head and the whole of B, both below its label
        assert n_own[c0 + n - 1] == n - 2 - half and runs[c0 + n - 1].tolist() == [1, half]
    half = (769 - 1) // 2
    assert half > STAGE and 769 - 1 - half > STAGE and 0 < half % STAGE           # each run longer than a stage


def test_cluster_point_classes():
    assert ge.W == 16 and ge.CLUSTER_POINTS == (100, 300)
    assert pe.nch(100) == 2 and 100 <= 2 * pe.WAVE                               # one pass
    assert pe.nch(300) == 4 and 4 * pe.WAVE < 300 <= 8 * pe.WAVE                 # two passes
    assert tc.n_fused(100, 16) == 96 and tc.n_fused(300, 16) == 288 > 4 * pe.WAVE  # a remainder in the last pass


def test_scan_size_classes():
    assert [nh.scan_chunk(n) for n in ge.SCAN_SIZES] == [512, 768]
    assert nh.scan_chunk(262144) == 256                                          # (the largest single-tile size)
    for n in ge.SCAN_SIZES:
        for kind in ge.SCAN_KINDS:
            x, y, z, r, ids, so, g = ge.scan_case(n, kind)
            assert len(x) == len(g) == n == int(so[-1]) and (len(so) == 2) == (kind == "single")
            assert g.max() == 2
    assert ge.SCAN_FULL[:2] == (ge.SCAN_SIZES[0], "batch")


def test_scan_row_counts_are_not_the_neighbour_counts():
    """What the second scan adds up at these sizes: with three labels an atom has 0, 1 or 2 rows (mostly 2: at probe 0
    nearly every atom still touches both other labels), another sequence than the neighbour counts that
    test_gpu_neighbor_edges.py scans at the same sizes, and every scan block holds rows, so the carry crosses every
    tile seam."""
    n = ge.SCAN_FULL[0]
    for kind in ge.SCAN_KINDS:
        x, y, z, r, ids, so, g = ge.scan_case(n, kind)
        offs, ent = nh.oracle_batch_csr(x, y, z, r, ids, so, ge.SCAN_PROBE)
        rows = np.diff(ge.row_offsets(offs, ent, g, ge.structure_base(so)).astype(np.int64))
        k = np.diff(offs.astype(np.int64))
        assert rows.max() == 2 and (rows <= k).all() and rows.sum() < k.sum() // 2
        assert (rows == 1).any() and ((rows == 0).any() or kind == "batch")
        per_block = np.add.reduceat(rows, np.arange(0, n, nh.scan_chunk(n)))
        assert len(per_block) == -(-n // 512) and (per_block[:-1] > 0).all()


def test_mixed_batch_classes():
    parts = ge.mixed_parts()
    sizes = [len(c[0]) for c, _ in parts]
    assert len(parts) == len(ge.MIXED_NAMES) == 9
    assert sizes[:3] == [0, 1, 2] and sizes[6] == 0
    # both binning routes
    assert sizes[5] == tl.LDS_MAX_ATOMS == min(len(tl._tail(k)) for k in range(3))
    assert sum(s >= tl.LDS_MAX_ATOMS for s in sizes) == 1 and sum(0 < s < tl.LDS_MAX_ATOMS for s in sizes) == 6
    for cols, g in parts:
        assert len(g) == len(cols[0]) and (len(g) == 0 or g.min() == 0)          # labels start at 0 everywhere
    assert parts[2][1].tolist() == [0, 1]
    (cat, g, so), (rcat, rg, rso) = ge.mixed_batch(), ge.mixed_batch(reverse=True)
    assert np.array_equal(np.diff(so.astype(np.int64)), sizes) and np.array_equal(np.diff(rso.astype(np.int64)), sizes[::-1])
    # the atom bases and the seams of the 4-wave workgroups move with the order
    assert sorted(set((so[:-1] % 4).tolist())) != [0] and (so[:-1] % 4).tolist() != (rso[:-1] % 4).tolist()[::-1]
    offs, ent = nh.oracle_batch_csr(*cat, so, ge.PROBE)
    k = np.diff(offs.astype(np.int64))
    per = [k[int(so[s]):int(so[s + 1])] for s in range(len(parts))]
    assert per[1].tolist() == [0] and per[2].tolist() == [1, 1]
    # lists longer than the neighbour staging (the 600-cluster), and none in the 300-cluster
    assert per[8].max() == 599 > ge.NB_STAGE and per[4].max() == 299 < ge.NB_STAGE
    assert int(np.sum(per[8] > ge.NB_STAGE)) == 400 and max(p.max() for p in per[:8] if len(p)) <= ge.NB_STAGE
    # entries removed by the id rule: against the lists without ids
    for s, n in ((4, 300), (8, 600)):
        b, e = int(so[s]), int(so[s + 1])
        cols = [c[b:e] for c in cat]
        with_ids = np.diff(nh.oracle_csr(*cols, ge.PROBE)[0].astype(np.int64))
        without = np.diff(nh.oracle_csr(*cols[:4], None, ge.PROBE)[0].astype(np.int64))
        assert np.array_equal(with_ids, per[s]) and int((without - with_ids).sum()) == (n // 3) * (n // 3 - 1)
        assert with_ids[-n:].min() == n - n // 3 and without[-n:].min() == n - 1
    # the head of each cluster shares its id with a third of the cluster: its one run is the shortened list
    n_own, rows, runs = ge.list_classes(offs, ent, g, ge.structure_base(so))
    c0 = int(so[9]) - 600
    assert n_own[c0] == 0 and runs[c0].tolist() == [400] and n_own[c0 + 1] == 400 and rows[c0 + 1] == 0
    assert n_own[c0 + 599] == 598 and runs[c0 + 599].tolist() == [1]


def test_tiny_batch_classes():
    cat, g, so = ge.tiny_batch()
    sizes = np.diff(so.astype(np.int64))
    assert len(sizes) == 3000 and sorted(set(sizes.tolist())) == [1, 2, 3, 4]
    offs, ent = nh.oracle_batch_csr(*cat, so, ge.PROBE)
    k = np.diff(offs.astype(np.int64))
    assert np.array_equal(k, np.repeat(sizes - 1, sizes))                        # every atom touches all the others
    rows = np.diff(ge.row_offsets(offs, ent, g, ge.structure_base(so)).astype(np.int64))
    assert rows.max() == 1 and np.array_equal(rows == 0, np.repeat(sizes == 1, sizes))


def test_id_cases_classes():
    n = 514
    for kind in ("head_against_rest", "one_label"):
        cols, g, c0, k, n_own, rows, runs = _cluster_classes(n, kind, shared_ids=True)
        plain = np.diff(nh.oracle_csr(*cols[:4], None, ge.PROBE)[0].astype(np.int64))
        short = k < plain
        assert short.sum() == n // 3 and np.array_equal(np.nonzero(short)[0], np.arange(c0, c0 + n // 3))
        assert k[short].min() == k[short].max() == n - n // 3 > STAGE            # shortened, and still two stages
        assert k[c0 + n // 3:].min() == n - 1
    _, _, c0, k, n_own, rows, runs = _cluster_classes(n, "head_against_rest", shared_ids=True)
    assert n_own[c0] == 0 and runs[c0].tolist() == [n - n // 3]                  # K and the run shrink
    assert n_own[c0 + 1] == n - n // 3 and rows[c0 + 1] == 0                     # the head is gone from these lists
    assert n_own[c0 + n - 1] == n - 2 and rows[c0 + n - 1] == 1


def test_threaded_batch_model_is_group_counts_batch():
    parts = [ge.mixed_parts()[k] for k in (0, 1, 2, 3, 6, 4)]
    cat, g, so = ge.pack(parts)
    want = gm.group_counts_batch(*cat, g, so, ge.PROBE, 100, 16)
    got = ge.batch_model(*cat, g, so, ge.PROBE, 100, 16, chunk=500)              # several tasks per structure
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    back = ge.join_models([ge.slice_model(got, so, s) for s in range(len(parts))])
    for a, b in zip(back, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)


# ---- the model against whole runs of the oracle -------------------------------------------------------------------

@pytest.mark.parametrize("kind", ge.CLUSTER_KINDS)
def test_model_against_the_oracle_on_long_runs(kind):
    """alone_check: the oracle on every group by itself (under one_label the own prefix of 257 entries);
    deletion_check: the oracle on the structure without each group in turn (the whole-stage run of head_against_rest
    goes with the rest's label, the last foreign entry with the head's).  Both are exact only where the smaller
    structure keeps the largest radius, so the radii are capped at the protein's largest and the head gets it: then
    no deletion is skipped and every named cluster group is compared alone.  The cluster's lists, and with them the
    classes, do not change: it sits inside 1.2 A.  own_then_many needs 514 atoms; the other labellings run at 258."""
    n = 514 if kind == "own_then_many" else 258
    cols, g, c0 = ge.cluster(n, kind)
    x, y, z, r, ids = cols
    cap = r[:c0].max()
    r = np.minimum(r, cap)
    r[c0] = cap
    cols = (x, y, z, r, ids)
    offs, ent = nh.oracle_csr(*cols, ge.PROBE)
    assert np.all(np.diff(offs.astype(np.int64))[c0:] == n - 1)
    n_own, rows, _ = ge.list_classes(offs, ent, g)
    assert np.array_equal(n_own[c0:], ge.list_classes(*nh.oracle_csr(*ge.cluster(n, kind)[0], ge.PROBE), g)[0][c0:])
    model = gm.group_counts(*cols, g, ge.PROBE, 100, ge.W, lists=(offs, ent))
    assert np.array_equal(np.diff(model[0].astype(np.int64)), rows)
    labels = np.unique(g)
    holds = [h for h in labels.tolist() if nh.fold_max(r[g == h]) == float(cap)]
    named = [h for h in (ge.LABEL_A, ge.LABEL_B, ge.LABEL_C) if (g == h).any()]
    assert named and set(named) <= set(holds)
    done, skipped = gm.alone_check(*cols, g, ge.PROBE, 100, ge.W, model)
    assert done == len(holds) and done + skipped == len(labels)
    done, skipped = gm.deletion_check(*cols, g, ge.PROBE, 100, ge.W, model)
    assert done == len(labels) and skipped == 0
    # the checks had something to find: cluster atoms lose points to their own group and to the others
    lost = model[4][c0:].astype(np.int64) - model[5][c0:].astype(np.int64)
    assert (lost > 0).any() if kind != "one_label" else (model[4][c0:] < 100).all()
