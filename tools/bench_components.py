#!/usr/bin/env python3
"""Wall time of rsasa_surface_components_batch (host buffers in; 8 B of dot offset per atom and 4 B of label per dot out,
and 4 B of count and 4 B of value per atom) beside rsasa_accessible_points_batch on the same input.  Both calls run the
same upload, grid, count, fill and point tests; the component call keeps the masks on the device, counts and scans them
and links the dots through the grid, so the difference of the two is the cost of search plus union (and the labels'
download against the masks').  Inputs: the workloads of tools/bench_points.py - the headline proteome
(bench_workloads.synthetic_proteome()) and real_coords (real_coords.py, tiled to the proteome's size) - at 100 and 960
points with the default link (rustsasa_amd.default_link of the batch).

    python tools/bench_components.py [--reps 5] [--out profiles/components_bench.json]

The two calls alternate (masks, components, masks, components, ...), each on preallocated pageable output buffers, after
one warm-up call each (the component call's warm-up sizes the label buffer); a call's time is a host clock around the
synchronous C call.  free is checked against the popcount of the masks and the offsets against its running sum; the
components are summarised (their number, the structures with more than one, the dots outside each structure's largest).
Nothing passes or fails on a time.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats --
python tools/bench_components.py --kernels-only` (k_component_link next to k_accessible_points on the same input)."""
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
ap.add_argument("--points", type=int, nargs="+", default=[100, 960])
ap.add_argument("--workloads", nargs="+", default=["proteome", "real_coords"])
ap.add_argument("--structures", type=int, default=None, help="proteome only: this many structures (default: the headline size)")
ap.add_argument("--kernels-only", action="store_true",
                help="one surface_components_batch and one accessible_points_batch per input (for rocprofv3), no timing")
ap.add_argument("--out", default=None, help="write the JSON result here too")
args = ap.parse_args()

ROWS = 65536  # atoms per block of the host-side popcount


def workload(name):
    if name == "proteome":
        return bw.synthetic_proteome(args.structures) if args.structures else bw.synthetic_proteome()
    import real_coords as rc
    return rc.tiled(rc.quality_set_batch(), bw.synthetic_proteome().n_atoms)


def main():
    ctx = rustsasa_amd.Context(0)
    lib = _capi.load()
    result = {"tool": "bench_components", "probe": args.probe, "reps": args.reps, "cases": []}
    for wname in args.workloads:
        b = workload(wname)
        x, y, z, r = (np.ascontiguousarray(a, np.float32) for a in (b.x, b.y, b.z, b.radius))
        ids = np.ascontiguousarray(b.ids, np.uint64)
        so = np.ascontiguousarray(b.structure_offsets, np.uint32)
        S, N = len(so) - 1, b.n_atoms
        if args.kernels_only:
            for n_points in args.points:
                ctx.surface_components_batch(x, y, z, r, ids, so, args.probe, n_points)
                ctx.accessible_points_batch(x, y, z, r, ids, so, args.probe, n_points)
            print(json.dumps({"workload": wname, "atoms": N, "kernels_only": True}), flush=True)
            continue
        sasa, free = np.zeros(N, np.float32), np.zeros(N, np.uint32)
        offsets = np.zeros(N + 1, np.uint64)
        for n_points in args.points:
            masks = np.zeros((N, (n_points + 31) // 32), np.uint32)
            link = float(rustsasa_amd.default_link(r, args.probe, n_points))
            buf = {"labels": None}

            def new():
                labels = buf["labels"]
                t0 = time.perf_counter()
                rc = lib.rsasa_surface_components_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S,
                                                        args.probe, n_points, link, ptr(offsets), ptr(labels),
                                                        0 if labels is None else labels.shape[0], ptr(free), ptr(sasa))
                dt = (time.perf_counter() - t0) * 1e3
                if labels is None and rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL:
                    return None
                _capi.check(rc, ctx._h)
                return dt

            def old():
                t0 = time.perf_counter()
                rc = lib.rsasa_accessible_points_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S,
                                                       args.probe, n_points, ptr(masks), ptr(sasa))
                dt = (time.perf_counter() - t0) * 1e3
                _capi.check(rc, ctx._h)
                return dt

            old()  # warm-up: workspaces, lattice
            new()  # sizing call
            buf["labels"] = labels = np.zeros(max(int(offsets[-1]), 1), np.uint32)
            new()
            t_new, t_old = [], []
            for _ in range(args.reps):
                t_old.append(old())
                t_new.append(new())
            popcount = np.zeros(N, np.int64)
            for blk in range(0, N, ROWS):
                popcount[blk:blk + ROWS] = np.unpackbits(masks[blk:blk + ROWS].view(np.uint8), axis=1).sum(axis=1)
            n_dots = int(offsets[-1])
            table = rustsasa_amd.component_table(offsets, labels[:n_dots], r, args.probe, n_points, so)
            per_structure = np.diff(table[0])
            first = table[0][:-1][per_structure > 0]
            case = {"workload": wname, "structures": S, "atoms": N, "n_points": n_points, "link": link, "dots": n_dots,
                    "mask_bytes": int(masks.nbytes), "label_bytes": 4 * n_dots, "offset_bytes": int(offsets.nbytes),
                    "surface_components_batch_ms": [round(t, 2) for t in t_new],
                    "surface_components_batch_median_ms": round(statistics.median(t_new), 2),
                    "accessible_points_batch_ms": [round(t, 2) for t in t_old],
                    "accessible_points_batch_median_ms": round(statistics.median(t_old), 2),
                    "search_and_union_median_ms": round(statistics.median(t_new) - statistics.median(t_old), 2),
                    "free_equals_popcount": bool(np.array_equal(free.astype(np.int64), popcount)),
                    "offsets_equal_cumsum": bool(np.array_equal(offsets[1:].astype(np.int64), np.cumsum(popcount))),
                    "components": int(len(table[1])),
                    "structures_with_several_components": int((per_structure > 1).sum()),
                    "dots_outside_the_largest_component": int(n_dots - table[2][first].sum())}
            assert case["free_equals_popcount"] and case["offsets_equal_cumsum"], case
            print(json.dumps(case), flush=True)
            result["cases"].append(case)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}))


main()
