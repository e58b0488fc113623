#!/usr/bin/env python3
"""Wall time of rsasa_radial_counts_batch (host buffers in; 1 B of class per atom beside the columns) on the workloads of
tools/bench_hse.py - the headline proteome (bench_workloads.synthetic_proteome()) and real_coords (real_coords.py, tiled
to the proteome's size) - in three shapes, every atom centre and partner:

    counts_4x4     edges (6, 8, 10, 12), 4 classes, counts only: 64 B per atom come back
    pairs_4x4      the same with the pair tables only: 512 B per structure come back
    counts_1x1     one class, the one edge 13 A, counts only - beside rsasa_half_sphere_exposure_batch at 13 A without
                   directions on the same input as the yardstick: the same sweep without the histogram

    python tools/bench_radial.py [--reps 5] [--out profiles/radial_bench.json]

The four calls alternate (hse, counts_1x1, counts_4x4, pairs_4x4, hse, ...), each on preallocated pageable output
buffers, after one warm-up call each; a call's time is a host clock around the synchronous C call.  On the full workload
it checks the identities of the header: counts_1x1 equals up + down of the yardstick, the 4 x 4 table summed over classes
and bins equals up + down at 12 A, and the pair tables equal the sums of the 4 x 4 rows by structure and class (numpy,
uint64).  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/bench_radial.py
--kernels-only` (k_radial_counts, k_radial_pairs and k_sort_kinds next to k_half_sphere on the same input)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench_workloads as bw  # noqa: E402
import rustsasa_amd  # noqa: E402
from rustsasa_amd import _capi  # noqa: E402
from rustsasa_amd._capi import ptr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--probe", type=float, default=1.4)
ap.add_argument("--workloads", nargs="+", default=["proteome", "real_coords"])
ap.add_argument("--structures", type=int, default=None, help="proteome only: this many structures (default: the headline size)")
ap.add_argument("--kernels-only", action="store_true", help="one call of each kind per input (for rocprofv3), no timing")
ap.add_argument("--out", default=None, help="write the JSON result here too")
args = ap.parse_args()

EDGES = np.array([6.0, 8.0, 10.0, 12.0], np.float32)
ONE_EDGE = np.array([13.0], np.float32)
N_CLASSES = 4


def workload(name):
    if name == "proteome":
        return bw.synthetic_proteome(args.structures) if args.structures else bw.synthetic_proteome()
    import real_coords as rc
    return rc.tiled(rc.quality_set_batch(), bw.synthetic_proteome().n_atoms)


def group_sums(table, classes, so):
    """uint64[S, C, C, B]: the rows of `table` summed by (structure, class of the atom)."""
    n_struct = len(so) - 1
    out = np.zeros((n_struct, N_CLASSES) + table.shape[1:], np.uint64)
    starts = so[:-1].astype(np.int64)
    filled = np.diff(so.astype(np.int64)) > 0
    for a in range(N_CLASSES):
        rows = np.where((classes == a)[:, None, None], table, 0).astype(np.uint64)
        out[filled, a] = np.add.reduceat(rows, starts[filled], axis=0)
    return out


def main():
    ctx = rustsasa_amd.Context(0)
    lib = _capi.load()
    result = {"tool": "bench_radial", "probe": args.probe, "reps": args.reps, "edges": EDGES.tolist(), "n_classes": N_CLASSES,
              "one_edge": ONE_EDGE.tolist(), "cases": []}
    for wname in args.workloads:
        b = workload(wname)
        x, y, z, r = (np.ascontiguousarray(a, np.float32) for a in (b.x, b.y, b.z, b.radius))
        ids = np.ascontiguousarray(b.ids, np.uint64)
        so = np.ascontiguousarray(b.structure_offsets, np.uint32)
        S, N = len(so) - 1, b.n_atoms
        classes = np.random.default_rng(1).integers(0, N_CLASSES, N).astype(np.uint8)
        up, down = np.zeros(N, np.uint32), np.zeros(N, np.uint32)
        one = np.zeros((N, 1, 1), np.uint32)
        table = np.zeros((N, N_CLASSES, len(EDGES)), np.uint32)
        pairs = np.zeros((S, N_CLASSES, N_CLASSES, len(EDGES)), np.uint64)

        def radial(cl, n_classes, edges, counts, tables):
            t0 = time.perf_counter()
            rc = lib.rsasa_radial_counts_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S, args.probe, None,
                                               ptr(cl), n_classes, ptr(edges), len(edges), ptr(counts), ptr(tables))
            dt = (time.perf_counter() - t0) * 1e3
            _capi.check(rc, ctx._h)
            return dt

        def yardstick(cutoff=float(ONE_EDGE[0])):
            t0 = time.perf_counter()
            rc = lib.rsasa_half_sphere_exposure_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S, args.probe,
                                                      None, None, cutoff, ptr(up), ptr(down))
            dt = (time.perf_counter() - t0) * 1e3
            _capi.check(rc, ctx._h)
            return dt

        calls = {"hse_13": yardstick,
                 "counts_1x1": lambda: radial(None, 1, ONE_EDGE, one, None),
                 "counts_4x4": lambda: radial(classes, N_CLASSES, EDGES, table, None),
                 "pairs_4x4": lambda: radial(classes, N_CLASSES, EDGES, None, pairs)}
        for call in calls.values():  # warm-up: workspaces (and, with --kernels-only, the one launch of each kind)
            call()
        if args.kernels_only:
            print(json.dumps({"workload": wname, "atoms": N, "kernels_only": True, "order": list(calls)}), flush=True)
            continue
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, call in calls.items():
                times[k].append(call())
        contact13 = up.astype(np.int64) + down
        one_ok = bool(np.array_equal(one[:, 0, 0].astype(np.int64), contact13))
        yardstick(float(EDGES[-1]))
        sum_ok = bool(np.array_equal(table.sum(axis=(1, 2), dtype=np.int64), up.astype(np.int64) + down))
        pairs_ok = bool(np.array_equal(pairs, group_sums(table, classes, so)))
        med = {k: statistics.median(v) for k, v in times.items()}
        case = {"workload": wname, "structures": S, "atoms": N,
                "out_bytes": {"counts_1x1": int(one.nbytes), "counts_4x4": int(table.nbytes), "pairs_4x4": int(pairs.nbytes),
                              "hse_13": int(up.nbytes + down.nbytes)},
                "ms": {k: [round(t, 2) for t in v] for k, v in times.items()},
                "median_ms": {k: round(v, 2) for k, v in med.items()},
                "counts_1x1_to_hse_13": round(med["counts_1x1"] / med["hse_13"], 3),
                "counts_1x1_equals_up_plus_down_at_13": one_ok,
                "counts_4x4_summed_equals_up_plus_down_at_12": sum_ok,
                "pairs_4x4_equal_the_group_sums_of_counts_4x4": pairs_ok,
                "mean_partners_within_12": float(table.sum(dtype=np.uint64) / max(N, 1)),
                "mean_partners_within_13": float(contact13.mean()) if N else 0.0,
                "largest_pair_cell": int(pairs.max()) if S else 0}
        assert one_ok and sum_ok and pairs_ok, case
        print(json.dumps(case), flush=True)
        result["cases"].append(case)
    ctx.close()
    if args.out and not args.kernels_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}))


main()
