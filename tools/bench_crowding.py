#!/usr/bin/env python3
"""Wall time of rsasa_dot_crowding_batch (host buffers in; 8 B per atom and 4 B per dot and bin come back) on the
workloads of tools/bench_radial.py - the headline proteome (bench_workloads.synthetic_proteome()) and real_coords
(real_coords.py, tiled to the proteome's size) - with edges (6, 8, 10) and every atom a partner, beside two yardsticks
on the same input:

    components     rsasa_surface_components_batch at the default link: it shares the masks, the popcounts and the scan
    hse_10         rsasa_half_sphere_exposure_batch at 10 A without directions: the same reach, per atom

    python tools/bench_crowding.py [--reps 5] [--out profiles/crowding_bench.json]

The three calls alternate (components, hse_10, crowding, components, ...), each on preallocated pageable output buffers,
after one warm-up call each; a call's time is a host clock around the synchronous C call.  On the full workload it checks
the identities of the header: the dot offsets equal those of the components call, and for a sample of structures the rows
equal rsasa_radial_counts_batch with the structure's dots appended as centre-only atoms of radius 0 (another kernel on
another grid).  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python
tools/bench_crowding.py --kernels-only` (k_dot_crowding next to k_accessible_points, k_component_link and k_half_sphere on
the same input)."""
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
ap.add_argument("--workloads", nargs="+", default=["proteome", "real_coords"])
ap.add_argument("--structures", type=int, default=None, help="proteome only: this many structures (default: the headline size)")
ap.add_argument("--witness", type=int, default=6, help="structures checked against the radial witness")
ap.add_argument("--kernels-only", action="store_true", help="one call of each kind per input (for rocprofv3), no timing")
ap.add_argument("--out", default=None, help="write the JSON result here too")
args = ap.parse_args()

EDGES = np.array([6.0, 8.0, 10.0], np.float32)


def workload(name):
    if name == "proteome":
        return bw.synthetic_proteome(args.structures) if args.structures else bw.synthetic_proteome()
    import real_coords as rc
    return rc.tiled(rc.quality_set_batch(), bw.synthetic_proteome().n_atoms)


def witness(ctx, cols, so, picks, offsets, rows):
    """Whether the rows of the structures `picks` equal the radial counts around their dots."""
    x, y, z, r, ids = cols
    ok = True
    for s in picks:
        b, e = int(so[s]), int(so[s + 1])
        if e == b:
            continue
        part = (x[b:e], y[b:e], z[b:e], r[b:e])
        _, q = ctx.surface_points(*part, ids[b:e], args.probe, args.points)
        n, d = e - b, len(q)
        cat = [np.concatenate([a, q[:, k]]) for k, a in enumerate(part[:3])] + [np.concatenate([part[3], np.zeros(d, np.float32)])]
        flags = np.concatenate([np.full(n, 1, np.uint8), np.full(d, 2, np.uint8)])
        table = ctx.radial_counts(*cat, None, args.probe, EDGES, None, 1, flags)
        ok = ok and d == int(offsets[e] - offsets[b]) and bool(np.array_equal(table[n:, 0, :], rows[int(offsets[b]):int(offsets[e])]))
    return ok


def main():
    ctx = rustsasa_amd.Context(0)
    lib = _capi.load()
    result = {"tool": "bench_crowding", "probe": args.probe, "n_points": args.points, "reps": args.reps,
              "edges": EDGES.tolist(), "cases": []}
    for wname in args.workloads:
        b = workload(wname)
        x, y, z, r = (np.ascontiguousarray(a, np.float32) for a in (b.x, b.y, b.z, b.radius))
        ids = np.ascontiguousarray(b.ids, np.uint64)
        so = np.ascontiguousarray(b.structure_offsets, np.uint32)
        S, N = len(so) - 1, b.n_atoms
        link = float(rustsasa_amd.default_link(r, args.probe, args.points))
        up, down = np.zeros(N, np.uint32), np.zeros(N, np.uint32)
        off_c, off_d = np.zeros(N + 1, np.uint64), np.zeros(N + 1, np.uint64)
        cols = (ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S, args.probe)
        # size the per-dot buffers once
        rc = lib.rsasa_dot_crowding_batch(ctx._h, *cols, args.points, None, ptr(EDGES), len(EDGES), ptr(off_d), None, 0, None, None)
        assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL or (rc == 0 and N == 0), rc
        D = int(off_d[-1])
        labels = np.zeros(D, np.uint32)
        rows = np.zeros((D, len(EDGES)), np.uint32)

        def timed(fn, *a):
            t0 = time.perf_counter()
            rc = fn(ctx._h, *cols, *a)
            dt = (time.perf_counter() - t0) * 1e3
            _capi.check(rc, ctx._h)
            return dt

        calls = {"components": lambda: timed(lib.rsasa_surface_components_batch, args.points, link, ptr(off_c), ptr(labels), D,
                                             None, None),
                 "hse_10": lambda: timed(lib.rsasa_half_sphere_exposure_batch, None, None, float(EDGES[-1]), ptr(up), ptr(down)),
                 "crowding": lambda: timed(lib.rsasa_dot_crowding_batch, args.points, None, ptr(EDGES), len(EDGES), ptr(off_d),
                                           ptr(rows), D, None, None)}
        for call in calls.values():  # warm-up: workspaces (and, with --kernels-only, the one launch of each kind)
            call()
        if args.kernels_only:
            print(json.dumps({"workload": wname, "atoms": N, "dots": D, "kernels_only": True, "order": list(calls)}), flush=True)
            continue
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, call in calls.items():
                times[k].append(call())
        offsets_ok = bool(np.array_equal(off_c, off_d))
        picks = np.random.default_rng(2).permutation(S)[:args.witness]
        witness_ok = witness(ctx, (x, y, z, r, ids), so, picks, off_d, rows)
        med = {k: statistics.median(v) for k, v in times.items()}
        within = rows.sum(axis=1, dtype=np.int64)
        case = {"workload": wname, "structures": S, "atoms": N, "dots": D,
                "out_bytes": {"crowding": int(rows.nbytes + off_d.nbytes), "components": int(labels.nbytes + off_c.nbytes),
                              "hse_10": int(up.nbytes + down.nbytes)},
                "ms": {k: [round(t, 2) for t in v] for k, v in times.items()},
                "median_ms": {k: round(v, 2) for k, v in med.items()},
                "crowding_to_components": round(med["crowding"] / med["components"], 3),
                "crowding_to_hse_10": round(med["crowding"] / med["hse_10"], 3),
                "dot_offsets_equal_those_of_surface_components": offsets_ok,
                "rows_equal_the_radial_witness": witness_ok, "witness_structures": [int(s) for s in picks],
                "mean_atoms_within_10_of_a_dot": float(within.mean()) if D else 0.0,
                "dot_partner_pairs_within_10": int(within.sum()),
                "mean_partners_within_10_of_an_atom": float((up.astype(np.int64) + down).mean()) if N else 0.0}
        assert offsets_ok and witness_ok, case
        print(json.dumps(case), flush=True)
        result["cases"].append(case)
    ctx.close()
    if args.out and not args.kernels_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}))


main()
