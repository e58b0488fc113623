#!/usr/bin/env python3
"""Wall time of rsasa_atom_depth_batch (host buffers in; 8 B of key, 4 B of count and 4 B of value per atom out) beside
rsasa_accessible_points_batch on the same input.  Both calls run the same upload, grid, count, fill and point tests; the
depth call keeps the masks on the device, counts them and searches the grid for every atom's nearest accessible dot, so
the difference of the two is the cost of the search itself (less the masks' download, n_points / 8 bytes per atom, which
the depth call does not make).  Inputs: the workloads of tools/bench_points.py - the headline proteome
(bench_workloads.synthetic_proteome()) and real_coords (real_coords.py, tiled to the proteome's size) - at 100 and 960
points.

    python tools/bench_depth.py [--reps 5] [--out profiles/depth_bench.json]

The two calls alternate (masks, depth, masks, depth, ...), each on preallocated pageable output buffers, after one
warm-up call each; a call's time is a host clock around the synchronous C call.  free is checked against the popcount of
the masks; the depths are summarised (median, maximum, atoms with no accessible point).  Kernel times come from a
separate run under `rocprofv3 --kernel-trace --stats -- python tools/bench_depth.py --kernels-only` (k_atom_depth next to
k_accessible_points on the same input)."""
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
                help="one atom_depth_batch and one accessible_points_batch per input (for rocprofv3), no timing")
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
    result = {"tool": "bench_depth", "probe": args.probe, "reps": args.reps, "cases": []}
    for wname in args.workloads:
        b = workload(wname)
        x, y, z, r = (np.ascontiguousarray(a, np.float32) for a in (b.x, b.y, b.z, b.radius))
        ids = np.ascontiguousarray(b.ids, np.uint64)
        so = np.ascontiguousarray(b.structure_offsets, np.uint32)
        S, N = len(so) - 1, b.n_atoms
        if args.kernels_only:
            for n_points in args.points:
                ctx.atom_depth_batch(x, y, z, r, ids, so, args.probe, n_points)
                ctx.accessible_points_batch(x, y, z, r, ids, so, args.probe, n_points)
            print(json.dumps({"workload": wname, "atoms": N, "kernels_only": True}), flush=True)
            continue
        sasa = np.zeros(N, np.float32)
        depth, nearest, free = np.zeros(N, np.float32), np.zeros(N, np.uint32), np.zeros(N, np.uint32)
        for n_points in args.points:
            masks = np.zeros((N, (n_points + 31) // 32), np.uint32)

            def new():
                t0 = time.perf_counter()
                rc = lib.rsasa_atom_depth_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S, args.probe,
                                                n_points, ptr(depth), ptr(nearest), ptr(free), ptr(sasa))
                dt = (time.perf_counter() - t0) * 1e3
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
            new()
            t_new, t_old = [], []
            for _ in range(args.reps):
                t_old.append(old())
                t_new.append(new())
            popcount = np.zeros(N, np.int64)
            for blk in range(0, N, ROWS):
                popcount[blk:blk + ROWS] = np.unpackbits(masks[blk:blk + ROWS].view(np.uint8), axis=1).sum(axis=1)
            finite = np.isfinite(depth)
            case = {"workload": wname, "structures": S, "atoms": N, "n_points": n_points,
                    "mask_bytes": int(masks.nbytes), "depth_bytes": int(depth.nbytes + nearest.nbytes + free.nbytes),
                    "sasa_bytes": int(sasa.nbytes),
                    "atom_depth_batch_ms": [round(t, 2) for t in t_new],
                    "atom_depth_batch_median_ms": round(statistics.median(t_new), 2),
                    "accessible_points_batch_ms": [round(t, 2) for t in t_old],
                    "accessible_points_batch_median_ms": round(statistics.median(t_old), 2),
                    "search_cost_median_ms": round(statistics.median(t_new) - statistics.median(t_old), 2),
                    "free_equals_popcount": bool(np.array_equal(free.astype(np.int64), popcount)),
                    "atoms_without_accessible_point": int((free == 0).sum()),
                    "atoms_without_depth": int((~finite).sum()),
                    "median_depth": float(np.median(depth[finite])) if finite.any() else None,
                    "max_depth": float(depth[finite].max()) if finite.any() else None,
                    "nearest_is_self_fraction": float(np.mean(nearest == (np.arange(N) - np.repeat(so[:-1], np.diff(so)))))}
            assert case["free_equals_popcount"], case
            print(json.dumps(case), flush=True)
            result["cases"].append(case)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}))


main()
