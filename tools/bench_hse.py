#!/usr/bin/env python3
"""Wall time of rsasa_half_sphere_exposure_batch (host buffers in; 12 B of direction and 1 B of flags per atom beside the
columns, 8 B of counts per atom out) at cutoff 13 A, once with every atom centre and partner and once with one atom in
eight as both (the CA-like case: the others are skipped by the kernel and counted by nobody), beside
rsasa_atom_depth_batch at 100 points on the same input as the neighbouring yardstick - the other call that sweeps the
grid beyond the neighbour reach.  Inputs: the workloads of tools/bench_points.py - the headline proteome
(bench_workloads.synthetic_proteome()) and real_coords (real_coords.py, tiled to the proteome's size).

    python tools/bench_hse.py [--reps 5] [--out profiles/hse_bench.json]

The three calls alternate (depth, all, eighth, depth, ...), each on preallocated pageable output buffers, after one
warm-up call each; a call's time is a host clock around the synchronous C call.  The counts are summarised (mean and
largest contact number, the share that is `up`), and up + down is checked against a second call without directions.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/bench_hse.py
--kernels-only` (k_half_sphere and k_sort_flags next to k_atom_depth on the same input)."""
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
ap.add_argument("--cutoff", type=float, default=13.0)
ap.add_argument("--depth-points", type=int, default=100)
ap.add_argument("--workloads", nargs="+", default=["proteome", "real_coords"])
ap.add_argument("--structures", type=int, default=None, help="proteome only: this many structures (default: the headline size)")
ap.add_argument("--kernels-only", action="store_true",
                help="one call of each kind per input (for rocprofv3), no timing")
ap.add_argument("--out", default=None, help="write the JSON result here too")
args = ap.parse_args()


def workload(name):
    if name == "proteome":
        return bw.synthetic_proteome(args.structures) if args.structures else bw.synthetic_proteome()
    import real_coords as rc
    return rc.tiled(rc.quality_set_batch(), bw.synthetic_proteome().n_atoms)


def main():
    ctx = rustsasa_amd.Context(0)
    lib = _capi.load()
    result = {"tool": "bench_hse", "probe": args.probe, "cutoff": args.cutoff, "reps": args.reps,
              "depth_points": args.depth_points, "cases": []}
    for wname in args.workloads:
        b = workload(wname)
        x, y, z, r = (np.ascontiguousarray(a, np.float32) for a in (b.x, b.y, b.z, b.radius))
        ids = np.ascontiguousarray(b.ids, np.uint64)
        so = np.ascontiguousarray(b.structure_offsets, np.uint32)
        S, N = len(so) - 1, b.n_atoms
        rng = np.random.default_rng(1)
        dirs = rng.normal(size=(N, 3)).astype(np.float32)
        eighth = np.where(np.arange(N) % 8 == 0, 3, 0).astype(np.uint8)
        up, down = np.zeros(N, np.uint32), np.zeros(N, np.uint32)
        depth, nearest = np.zeros(N, np.float32), np.zeros(N, np.uint32)

        def hse(flags, with_dirs=True):
            t0 = time.perf_counter()
            rc = lib.rsasa_half_sphere_exposure_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S, args.probe,
                                                      ptr(dirs) if with_dirs else None, ptr(flags), args.cutoff, ptr(up),
                                                      ptr(down))
            dt = (time.perf_counter() - t0) * 1e3
            _capi.check(rc, ctx._h)
            return dt

        def yardstick():
            t0 = time.perf_counter()
            rc = lib.rsasa_atom_depth_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S, args.probe,
                                            args.depth_points, ptr(depth), ptr(nearest), None, None)
            dt = (time.perf_counter() - t0) * 1e3
            _capi.check(rc, ctx._h)
            return dt

        if args.kernels_only:
            yardstick()
            hse(None)
            hse(eighth)
            print(json.dumps({"workload": wname, "atoms": N, "kernels_only": True}), flush=True)
            continue
        yardstick()  # warm-up: workspaces, lattice
        hse(None)
        hse(eighth)
        t_depth, t_all, t_eighth = [], [], []
        for _ in range(args.reps):
            t_depth.append(yardstick())
            t_all.append(hse(None))
            t_eighth.append(hse(eighth))
        hse(None, with_dirs=False)
        contact = up.copy()
        hse(None)
        case = {"workload": wname, "structures": S, "atoms": N, "cutoff": args.cutoff,
                "in_bytes_beside_columns": int(dirs.nbytes + eighth.nbytes), "out_bytes": int(up.nbytes + down.nbytes),
                "hse_all_ms": [round(t, 2) for t in t_all], "hse_all_median_ms": round(statistics.median(t_all), 2),
                "hse_one_in_eight_ms": [round(t, 2) for t in t_eighth],
                "hse_one_in_eight_median_ms": round(statistics.median(t_eighth), 2),
                "atom_depth_batch_ms": [round(t, 2) for t in t_depth],
                "atom_depth_batch_median_ms": round(statistics.median(t_depth), 2),
                "up_plus_down_equals_contact_number": bool(np.array_equal(up + down, contact)),
                "mean_contact_number": float(contact.mean()), "max_contact_number": int(contact.max()),
                "up_share": float(up.sum() / max(int(contact.sum()), 1))}
        assert case["up_plus_down_equals_contact_number"], case
        print(json.dumps(case), flush=True)
        result["cases"].append(case)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}))


main()
