#!/usr/bin/env python3
"""Wall time of rsasa_accessible_points_batch (host buffers in, bit masks and values out) against another build's
rsasa_precompute_neighbors_batch (host buffers in, CSR lists out) on the same inputs: both run the same upload, grid,
count and fill; the point call replaces the download of the lists (8 B per entry) with one kernel and a download of
n_points / 8 + 4 B per atom.  Inputs: the headline proteome workload (bench_workloads.synthetic_proteome()) and the
real_coords workload (real_coords.py, tiled to the proteome's size), at 100 and 960 points.

    python tools/bench_points.py --baseline-lib OTHER/librustsasa_amd.so [--reps 5] [--out profiles/points_bench.json]

The two calls alternate (baseline, new, baseline, new, ...), each on preallocated pageable output buffers, each in a
context of its own library.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_points.py --kernels-only` (k_accessible_points next to the
k_occlusion_mx* kernels of rsasa_calculate_sasa_batch on the same input)."""
import argparse
import ctypes as C
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
ap.add_argument("--baseline-lib", help="librustsasa_amd.so of the build to compare with (its precompute_neighbors_batch)")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--probe", type=float, default=1.4)
ap.add_argument("--points", type=int, nargs="+", default=[100, 960])
ap.add_argument("--workloads", nargs="+", default=["proteome", "real_coords"])
ap.add_argument("--kernels-only", action="store_true",
                help="one accessible_points_batch and one calculate_sasa_batch per input (for rocprofv3), no timing")
ap.add_argument("--out", default=None, help="write the JSON result here too")
args = ap.parse_args()


def workload(name):
    if name == "proteome":
        return bw.synthetic_proteome()
    import real_coords as rc
    return rc.tiled(rc.quality_set_batch(), bw.synthetic_proteome().n_atoms)


def main():
    ctx = rustsasa_amd.Context(0)
    lib = _capi.load()
    base_lib = base_ctx = None
    if args.baseline_lib and not args.kernels_only:
        base_lib = C.CDLL(os.path.abspath(args.baseline_lib))
        for name in ("rsasa_context_create", "rsasa_context_destroy", "rsasa_precompute_neighbors_batch"):
            fn = getattr(base_lib, name)
            fn.restype, fn.argtypes = _capi.SYMBOLS[name]
        h = C.c_void_p()
        _capi.check(base_lib.rsasa_context_create(0, C.byref(h)))
        base_ctx = h
    result = {"tool": "bench_points", "probe": args.probe, "reps": args.reps, "cases": []}
    for wname in args.workloads:
        b = workload(wname)
        x, y, z, r = (np.ascontiguousarray(a, np.float32) for a in (b.x, b.y, b.z, b.radius))
        ids = np.ascontiguousarray(b.ids, np.uint64)
        so = np.ascontiguousarray(b.structure_offsets, np.uint32)
        S, N = len(so) - 1, b.n_atoms
        if args.kernels_only:
            for n_points in args.points:
                ctx.accessible_points_batch(x, y, z, r, ids, so, args.probe, n_points)
                ctx.calculate_sasa_batch(x, y, z, r, ids, so, args.probe, n_points)
            print(json.dumps({"workload": wname, "atoms": N, "kernels_only": True}), flush=True)
            continue
        offsets = entries = None
        if base_lib is not None:
            offsets = np.zeros(N + 1, np.uint64)
            rc = base_lib.rsasa_precompute_neighbors_batch(base_ctx, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so),
                                                           S, args.probe, float("nan"), ptr(offsets), None, 0)
            assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL, rc
            entries = np.zeros(int(offsets[-1]), _capi.NEIGHBOR_DTYPE)
        sasa = np.zeros(N, np.float32)
        for n_points in args.points:
            masks = np.zeros((N, (n_points + 31) // 32), np.uint32)

            def new():
                t0 = time.perf_counter()
                rc = lib.rsasa_accessible_points_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S,
                                                       args.probe, n_points, ptr(masks), ptr(sasa))
                dt = (time.perf_counter() - t0) * 1e3
                _capi.check(rc, ctx._h)
                return dt

            def base():
                t0 = time.perf_counter()
                rc = base_lib.rsasa_precompute_neighbors_batch(base_ctx, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids),
                                                               ptr(so), S, args.probe, float("nan"), ptr(offsets),
                                                               ptr(entries), entries.shape[0])
                dt = (time.perf_counter() - t0) * 1e3
                assert rc == 0, rc
                return dt

            new()  # warm-up: workspaces, lattice
            if base_lib is not None:
                base()
            t_new, t_base = [], []
            for _ in range(args.reps):
                if base_lib is not None:
                    t_base.append(base())
                t_new.append(new())
            case = {"workload": wname, "structures": S, "atoms": N, "n_points": n_points,
                    "mask_bytes": int(masks.nbytes), "sasa_bytes": int(sasa.nbytes),
                    "accessible_points_batch_ms": [round(t, 2) for t in t_new],
                    "accessible_points_batch_median_ms": round(statistics.median(t_new), 2)}
            if base_lib is not None:
                case.update({"baseline_precompute_neighbors_batch_ms": [round(t, 2) for t in t_base],
                             "baseline_precompute_neighbors_batch_median_ms": round(statistics.median(t_base), 2),
                             "list_bytes": int(entries.nbytes + offsets.nbytes),
                             "new_not_slower": statistics.median(t_new) <= statistics.median(t_base)})
            print(json.dumps(case), flush=True)
            result["cases"].append(case)
    if base_lib is not None:
        base_lib.rsasa_context_destroy(base_ctx)
        result["bar1_met"] = all(c["new_not_slower"] for c in result["cases"])
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}))


main()
