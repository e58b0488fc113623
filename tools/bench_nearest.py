#!/usr/bin/env python3
"""Wall time of rsasa_nearest_atoms_batch (host buffers in; 8 B of offsets per atom and 8 B per entry out) on the headline
proteome (bench_workloads.synthetic_proteome()), in two shapes:

    all_30       every atom centre and partner, k = 30, no cutoff (all-atom k-NN graphs)
    eighth_64    one atom in eight a centre, every atom a partner, k = 64, no cutoff (residue-level k-NN graphs)

beside the route a caller has without it: rsasa_atoms_within_batch on the same input and flags at a guessed cutoff of
8 A and of 13 A, whose lists the caller then cuts at k on the host (that cut is not timed).  Both are timed in the same
run on the same build.  For each cutoff the share of centres whose within-list is shorter than k says how many lists
the guess leaves short.  A within call whose entries would take more than --max-gb of host memory is sized only (its
count pass and scan run, and give the entries and the share; there is no fill to time).

    python tools/bench_nearest.py [--reps 3] [--out profiles/nearest_bench.json]

The calls alternate (within 8, within 13, nearest, ...), each on preallocated pageable output buffers, after one warm-up
call each; a call's time is a host clock around the synchronous C call.  The nearest lists are checked against the
within lists cut at k wherever the within list holds k entries or more.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_nearest.py --kernels-only` (k_nearest, k_nearest_gather next to
k_within_count, k_within_fill)."""
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
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--probe", type=float, default=1.4)
ap.add_argument("--structures", type=int, default=None, help="this many structures (default: the headline size)")
ap.add_argument("--shapes", nargs="+", default=["all_30", "eighth_64"])
ap.add_argument("--cutoffs", nargs="+", type=float, default=[8.0, 13.0])
ap.add_argument("--max-gb", type=float, default=12.0, help="a within call with more entries than this is sized, not filled")
ap.add_argument("--kernels-only", action="store_true", help="one call of each kind per shape (for rocprofv3), no timing")
ap.add_argument("--out", default=None, help="write the JSON result here too")
args = ap.parse_args()


def main():
    ctx = rustsasa_amd.Context(0)
    lib = _capi.load()
    b = bw.synthetic_proteome(args.structures) if args.structures else bw.synthetic_proteome()
    x, y, z, r = (np.ascontiguousarray(a, np.float32) for a in (b.x, b.y, b.z, b.radius))
    ids = np.ascontiguousarray(b.ids, np.uint64)
    so = np.ascontiguousarray(b.structure_offsets, np.uint32)
    S, N = len(so) - 1, b.n_atoms
    shapes = {"all_30": (None, 30), "eighth_64": (np.where(np.arange(N) % 8 == 0, 3, 1).astype(np.uint8), 64)}
    result = {"tool": "bench_nearest", "probe": args.probe, "reps": args.reps, "structures": S, "atoms": N, "cases": []}
    cols = (ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S, args.probe)
    for name in args.shapes:
        flags, k = shapes[name]
        centre = np.ones(N, bool) if flags is None else (flags & 2) != 0
        centres = int(centre.sum())

        def nearest(offsets, entries):
            t0 = time.perf_counter()
            rc = lib.rsasa_nearest_atoms_batch(ctx._h, *cols, ptr(flags), k, float("inf"), ptr(offsets), ptr(entries), len(entries))
            dt = (time.perf_counter() - t0) * 1e3
            _capi.check(rc, ctx._h)
            return dt

        def within(cutoff, offsets, entries):
            t0 = time.perf_counter()
            rc = lib.rsasa_atoms_within_batch(ctx._h, *cols, ptr(flags), cutoff, 0, ptr(offsets), ptr(entries),
                                              0 if entries is None else len(entries))
            return rc, (time.perf_counter() - t0) * 1e3

        nn_off = np.zeros(N + 1, np.uint64)
        nn_ent = np.zeros(centres * k, _capi.WITHIN_DTYPE)   # (zeros: the pages are touched before the clock runs)
        routes = []
        for cutoff in args.cutoffs:
            off = np.zeros(N + 1, np.uint64)
            rc, t_size = within(cutoff, off, None)           # the sizing call: grid, count pass and scan, no entries
            assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL, rc
            total = int(off[-1])
            lengths = np.diff(off.astype(np.int64))[centre]
            route = {"cutoff": cutoff, "entries": total, "out_bytes": int(total * 8 + off.nbytes),
                     "mean_list": float(total / max(centres, 1)), "sizing_call_ms": round(t_size, 2),
                     "share_of_centres_shorter_than_k": float(np.count_nonzero(lengths < k) / max(centres, 1)),
                     "filled": total * 8 <= args.max_gb * 1e9}
            route["buffers"] = (off, np.zeros(total, _capi.WITHIN_DTYPE) if route["filled"] else None)
            routes.append(route)

        def fill(route):
            rc, dt = within(route["cutoff"], *route["buffers"])
            _capi.check(rc, ctx._h)
            return dt

        for route in routes:                                 # warm-up: workspaces
            if route["filled"]:
                fill(route)
        nearest(nn_off, nn_ent)
        if args.kernels_only:
            print(json.dumps({"shape": name, "atoms": N, "k": k, "kernels_only": True}), flush=True)
            continue
        t_nn = []
        for route in routes:
            route["ms"] = []
        for _ in range(args.reps):
            for route in routes:
                if route["filled"]:
                    route["ms"].append(fill(route))
            t_nn.append(nearest(nn_off, nn_ent))
        total_nn = int(nn_off[-1])
        med_nn = statistics.median(t_nn)
        case = {"shape": name, "k": k, "centres": centres, "entries": total_nn, "out_bytes": int(total_nn * 8 + nn_off.nbytes),
                "nearest_atoms_batch_ms": [round(t, 2) for t in t_nn], "nearest_atoms_batch_median_ms": round(med_nn, 2),
                "entries_per_second": round(total_nn / (med_nn * 1e-3)), "atoms_within_batch": []}
        for route in routes:
            off, ent = route.pop("buffers")
            ms = route.pop("ms")
            if route["filled"]:
                # where the within list holds k entries or more, its first k are the nearest list
                w_len, n_len = np.diff(off.astype(np.int64)), np.diff(nn_off.astype(np.int64))
                full = np.flatnonzero(w_len >= k)[:: max(1, centres // 200000)]
                take = (off[full].astype(np.int64)[:, None] + np.arange(k)[None, :]).ravel()
                mine = (nn_off[full].astype(np.int64)[:, None] + np.arange(k)[None, :]).ravel()
                route["first_k_equal_nearest"] = bool(np.all(n_len[full] == k) and ent[take].tobytes() == nn_ent[mine].tobytes())
                route["lists_compared"] = int(len(full))
                assert route["first_k_equal_nearest"], route
                med = statistics.median(ms)
                route.update(atoms_within_batch_ms=[round(t, 2) for t in ms], atoms_within_batch_median_ms=round(med, 2),
                             nearest_over_within=round(med_nn / med, 3))
            case["atoms_within_batch"].append(route)
            del ent
        print(json.dumps(case), flush=True)
        result["cases"].append(case)
        del nn_ent, routes
    ctx.close()
    if args.out and not args.kernels_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}))


main()
