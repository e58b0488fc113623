#!/usr/bin/env python3
"""Wall time of rsasa_dot_enclosure_batch (host buffers in; 8 B per atom and 4 B per dot come back) on the workloads of
tools/bench_crowding.py - the headline proteome (bench_workloads.synthetic_proteome()) and real_coords (real_coords.py,
tiled to the proteome's size) - at 30 directions and reach 10 with every atom an obstacle, beside one yardstick on the
same input:

    crowding_10    rsasa_dot_crowding_batch with the single edge 10: it shares the whole front half (lists, masks,
                   popcounts, scan, sorted flags) and the reach, and tests every staged atom against every dot once

    python tools/bench_enclosure.py [--reps 5] [--out profiles/enclosure_bench.json]

The two calls alternate (crowding_10, enclosure, crowding_10, ...), each on preallocated pageable output buffers, after
one warm-up call each; a call's time is a host clock around the synchronous C call.  On the full workload it checks what
the header promises without a model: the dot offsets equal those of the crowding call, no bit at or above n_dirs is set,
and for a sample of structures the OR over a three-way split of the obstacle flags equals the words with all obstacles.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/bench_enclosure.py
--kernels-only` (k_dot_enclosure next to k_dot_crowding and k_accessible_points on the same input)."""
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
ap.add_argument("--points", type=int, default=100)
ap.add_argument("--dirs", type=int, default=30)
ap.add_argument("--reach", type=float, default=10.0)
ap.add_argument("--workloads", nargs="+", default=["proteome", "real_coords"])
ap.add_argument("--structures", type=int, default=None, help="proteome only: this many structures (default: the headline size)")
ap.add_argument("--witness", type=int, default=6, help="structures checked by the OR-split identity")
ap.add_argument("--kernels-only", action="store_true", help="one call of each kind per input (for rocprofv3), no timing")
ap.add_argument("--out", default=None, help="write the JSON result here too")
args = ap.parse_args()

EDGE = np.array([args.reach], np.float32)


def workload(name):
    if name == "proteome":
        return bw.synthetic_proteome(args.structures) if args.structures else bw.synthetic_proteome()
    import real_coords as rc
    return rc.tiled(rc.quality_set_batch(), bw.synthetic_proteome().n_atoms)


def split_witness(ctx, cols, so, picks, offsets, words):
    """Whether, in the structures `picks`, the OR over a split of the obstacles equals the words with all of them."""
    x, y, z, r, ids = cols
    ok = True
    rng = np.random.default_rng(5)
    for s in picks:
        b, e = int(so[s]), int(so[s + 1])
        if e == b:
            continue
        part = rng.integers(0, 3, e - b)
        got = 0
        for k in range(3):
            got = got | ctx.dot_enclosure(x[b:e], y[b:e], z[b:e], r[b:e], ids[b:e], args.probe, args.points, args.dirs, args.reach,
                                          (part == k).astype(np.uint8))[1]
        ok = ok and bool(np.array_equal(got, words[int(offsets[b]):int(offsets[e])]))
    return ok


def main():
    ctx = rustsasa_amd.Context(0)
    lib = _capi.load()
    result = {"tool": "bench_enclosure", "probe": args.probe, "n_points": args.points, "n_dirs": args.dirs, "reach": args.reach,
              "reps": args.reps, "cases": []}
    for wname in args.workloads:
        b = workload(wname)
        x, y, z, r = (np.ascontiguousarray(a, np.float32) for a in (b.x, b.y, b.z, b.radius))
        ids = np.ascontiguousarray(b.ids, np.uint64)
        so = np.ascontiguousarray(b.structure_offsets, np.uint32)
        S, N = len(so) - 1, b.n_atoms
        off_c, off_e = np.zeros(N + 1, np.uint64), np.zeros(N + 1, np.uint64)
        cols = (ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S, args.probe)
        # size the per-dot buffers once
        rc = lib.rsasa_dot_enclosure_batch(ctx._h, *cols, args.points, None, args.reach, args.dirs, ptr(off_e), None, 0, None, None)
        assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL or (rc == 0 and N == 0), rc
        D = int(off_e[-1])
        rows = np.zeros((D, 1), np.uint32)
        words = np.zeros(D, np.uint32)

        def timed(fn, *a):
            t0 = time.perf_counter()
            rc = fn(ctx._h, *cols, *a)
            dt = (time.perf_counter() - t0) * 1e3
            _capi.check(rc, ctx._h)
            return dt

        calls = {"crowding_10": lambda: timed(lib.rsasa_dot_crowding_batch, args.points, None, ptr(EDGE), 1, ptr(off_c), ptr(rows),
                                              D, None, None),
                 "enclosure": lambda: timed(lib.rsasa_dot_enclosure_batch, args.points, None, args.reach, args.dirs, ptr(off_e),
                                            ptr(words), D, None, None)}
        for call in calls.values():  # warm-up: workspaces (and, with --kernels-only, the one launch of each kind)
            call()
        if args.kernels_only:
            print(json.dumps({"workload": wname, "atoms": N, "dots": D, "kernels_only": True, "order": list(calls)}), flush=True)
            continue
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, call in calls.items():
                times[k].append(call())
        offsets_ok = bool(np.array_equal(off_c, off_e))
        high_ok = args.dirs == 32 or not bool((words >> np.uint32(args.dirs)).any())
        picks = np.random.default_rng(2).permutation(S)[:args.witness]
        split_ok = split_witness(ctx, (x, y, z, r, ids), so, picks, off_e, words)
        med = {k: statistics.median(v) for k, v in times.items()}
        frac = rustsasa_amd.enclosure_fraction(words, args.dirs)
        case = {"workload": wname, "structures": S, "atoms": N, "dots": D,
                "out_bytes": {"enclosure": int(words.nbytes + off_e.nbytes), "crowding_10": int(rows.nbytes + off_c.nbytes)},
                "ms": {k: [round(t, 2) for t in v] for k, v in times.items()},
                "median_ms": {k: round(v, 2) for k, v in med.items()},
                "enclosure_to_crowding_10": round(med["enclosure"] / med["crowding_10"], 3),
                "dot_offsets_equal_those_of_dot_crowding": offsets_ok, "no_bit_at_or_above_n_dirs": high_ok,
                "or_over_a_split_of_the_obstacles_equals_the_words": split_ok, "witness_structures": [int(s) for s in picks],
                "mean_atoms_within_reach_of_a_dot": float(rows.mean()) if D else 0.0,
                "dot_obstacle_pairs_within_reach": int(rows.sum(dtype=np.int64)),
                "blocked_fraction": {"min": float(frac.min()), "median": float(np.median(frac)), "max": float(frac.max()),
                                     "share_of_dots_at_or_above_0.8": float((frac >= 0.8).mean())} if D else {}}
        assert offsets_ok and high_ok and split_ok, case
        print(json.dumps(case), flush=True)
        result["cases"].append(case)
    ctx.close()
    if args.out and not args.kernels_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}))


main()
