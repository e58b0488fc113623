#!/usr/bin/env python3
"""Wall time of rsasa_exposure_vectors_batch (host buffers in; 12 B of vector, 4 B of count and 4 B of value per atom
out) against the way to the same vectors without it: rsasa_accessible_points_batch (bit masks and values out) and a
host-side sum of the lattice over the unpacked masks.  Both calls run the same upload, grid, count and fill and the same
point tests; the exposure call replaces the mask words by a reduction in the wave and downloads 16 B per atom where the
masks are n_points / 8.  Inputs: the workloads of tools/bench_points.py - the headline proteome
(bench_workloads.synthetic_proteome()) and real_coords (real_coords.py, tiled to the proteome's size) - at 100 and 960
points.

    python tools/bench_exposure.py [--reps 5] [--out profiles/exposure_bench.json]

The two calls alternate (masks, vectors, masks, vectors, ...), each on preallocated pageable output buffers, after one
warm-up call each; a call's time is a host clock around the synchronous C call.  The host-side sum (numpy: unpackbits,
then a float32 product with the lattice, 65 536 atoms at a time) is timed `--host-sum-reps` times (default once: it takes
seconds) and reported by itself; it is checked against the call's vectors to 1e-3 (it adds in another order).
Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_exposure.py --kernels-only` (k_exposure_vectors next to
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
ap.add_argument("--host-sum-reps", type=int, default=1)
ap.add_argument("--probe", type=float, default=1.4)
ap.add_argument("--points", type=int, nargs="+", default=[100, 960])
ap.add_argument("--workloads", nargs="+", default=["proteome", "real_coords"])
ap.add_argument("--structures", type=int, default=None, help="proteome only: this many structures (default: the headline size)")
ap.add_argument("--kernels-only", action="store_true",
                help="one exposure_vectors_batch and one accessible_points_batch per input (for rocprofv3), no timing")
ap.add_argument("--out", default=None, help="write the JSON result here too")
args = ap.parse_args()

ROWS = 65536  # atoms per block of the host-side sum


def workload(name):
    if name == "proteome":
        return bw.synthetic_proteome(args.structures) if args.structures else bw.synthetic_proteome()
    import real_coords as rc
    return rc.tiled(rc.quality_set_batch(), bw.synthetic_proteome().n_atoms)


def host_sum(masks, n_points, lattice):
    """float32[N, 3]: the lattice summed over the set bits of every row of `masks`, block by block."""
    out = np.empty((masks.shape[0], 3), np.float32)
    for b in range(0, masks.shape[0], ROWS):
        bits = np.unpackbits(masks[b:b + ROWS].view(np.uint8), axis=1, bitorder="little")[:, :n_points]
        out[b:b + ROWS] = bits.astype(np.float32) @ lattice
    return out


def main():
    ctx = rustsasa_amd.Context(0)
    lib = _capi.load()
    result = {"tool": "bench_exposure", "probe": args.probe, "reps": args.reps, "host_sum_reps": args.host_sum_reps,
              "cases": []}
    for wname in args.workloads:
        b = workload(wname)
        x, y, z, r = (np.ascontiguousarray(a, np.float32) for a in (b.x, b.y, b.z, b.radius))
        ids = np.ascontiguousarray(b.ids, np.uint64)
        so = np.ascontiguousarray(b.structure_offsets, np.uint32)
        S, N = len(so) - 1, b.n_atoms
        if args.kernels_only:
            for n_points in args.points:
                ctx.exposure_vectors_batch(x, y, z, r, ids, so, args.probe, n_points)
                ctx.accessible_points_batch(x, y, z, r, ids, so, args.probe, n_points)
            print(json.dumps({"workload": wname, "atoms": N, "kernels_only": True}), flush=True)
            continue
        sasa = np.zeros(N, np.float32)
        vectors, free = np.zeros((N, 3), np.float32), np.zeros(N, np.uint32)
        for n_points in args.points:
            masks = np.zeros((N, (n_points + 31) // 32), np.uint32)
            lattice = np.ascontiguousarray(np.stack(rustsasa_amd.sphere_points(n_points), axis=1))

            def new():
                t0 = time.perf_counter()
                rc = lib.rsasa_exposure_vectors_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S,
                                                      args.probe, n_points, ptr(vectors), ptr(free), ptr(sasa))
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
            t_sum = []
            for _ in range(args.host_sum_reps):
                t0 = time.perf_counter()
                summed = host_sum(masks, n_points, lattice)
                t_sum.append((time.perf_counter() - t0) * 1e3)
            case = {"workload": wname, "structures": S, "atoms": N, "n_points": n_points,
                    "mask_bytes": int(masks.nbytes), "vector_bytes": int(vectors.nbytes + free.nbytes),
                    "sasa_bytes": int(sasa.nbytes),
                    "exposure_vectors_batch_ms": [round(t, 2) for t in t_new],
                    "exposure_vectors_batch_median_ms": round(statistics.median(t_new), 2),
                    "accessible_points_batch_ms": [round(t, 2) for t in t_old],
                    "accessible_points_batch_median_ms": round(statistics.median(t_old), 2),
                    "new_not_slower_than_masks_call": statistics.median(t_new) <= statistics.median(t_old)}
            if t_sum:
                popcount = np.zeros(N, np.int64)
                for blk in range(0, N, ROWS):
                    popcount[blk:blk + ROWS] = np.unpackbits(masks[blk:blk + ROWS].view(np.uint8), axis=1).sum(axis=1)
                case.update({"host_sum_ms": [round(t, 1) for t in t_sum],
                             "masks_call_plus_host_sum_median_ms": round(statistics.median(t_old) + statistics.median(t_sum), 1),
                             "free_equals_popcount": bool(np.array_equal(free.astype(np.int64), popcount)),
                             "max_abs_vector_difference": float(np.max(np.abs(summed - vectors)))})
                assert case["free_equals_popcount"] and case["max_abs_vector_difference"] < 1e-3, case
            print(json.dumps(case), flush=True)
            result["cases"].append(case)
    ctx.close()
    if not args.kernels_only:
        result["new_not_slower_everywhere"] = all(c["new_not_slower_than_masks_call"] for c in result["cases"])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}))


main()
