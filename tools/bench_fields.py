#!/usr/bin/env python3
"""Wall time of rsasa_dot_fields_batch (host buffers in; 8 B per atom and 8 B per dot and channel come back) on the
workloads of tools/bench_crowding.py - the headline proteome (bench_workloads.synthetic_proteome()) and real_coords
(real_coords.py, tiled to the proteome's size) - with the cutoff 10 and every atom a partner, beside its yardstick on the
same input in the same process:

    crowding_10    rsasa_dot_crowding_batch with the single edge (10.0,): the same frame, the same (dot, atom) pairs, 1 added

and three calls of the fields:

    step_1         one STEP channel of ones: what the frame change alone costs (the weight rows staged, 64-bit sums)
    inv_d_1        one INV_D channel of seeded charges: a square root and a division per hit
    four_kinds_4   four channels of the four kinds

    python tools/bench_fields.py [--reps 5] [--out profiles/fields_bench.json]

The four calls alternate (crowding_10, step_1, inv_d_1, four_kinds_4, crowding_10, ...), each on preallocated pageable
output buffers, after one warm-up call each; a call's time is a host clock around the synchronous C call.  On the full
workload it checks the identities of the header: the dot offsets equal those of the crowding call, and the STEP channel of
ones equals 2^24 times the crowding counts, row for row."""
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
ap.add_argument("--kernels-only", action="store_true", help="one call of each kind per input (for rocprofv3), no timing")
ap.add_argument("--out", default=None, help="write the JSON result here too")
args = ap.parse_args()

CUTOFF = 10.0
EDGE = np.array([CUTOFF], np.float32)


def workload(name):
    if name == "proteome":
        return bw.synthetic_proteome(args.structures) if args.structures else bw.synthetic_proteome()
    import real_coords as rc
    return rc.tiled(rc.quality_set_batch(), bw.synthetic_proteome().n_atoms)


def main():
    ctx = rustsasa_amd.Context(0)
    lib = _capi.load()
    result = {"tool": "bench_fields", "probe": args.probe, "n_points": args.points, "reps": args.reps, "cutoff": CUTOFF,
              "cases": []}
    for wname in args.workloads:
        b = workload(wname)
        x, y, z, r = (np.ascontiguousarray(a, np.float32) for a in (b.x, b.y, b.z, b.radius))
        ids = np.ascontiguousarray(b.ids, np.uint64)
        so = np.ascontiguousarray(b.structure_offsets, np.uint32)
        S, N = len(so) - 1, b.n_atoms
        rng = np.random.default_rng(6)
        ones = np.ones((N, 1), np.float32)
        charges = np.ascontiguousarray(rng.uniform(-1.0, 1.0, (N, 1)), np.float32)
        four = np.ascontiguousarray(rng.uniform(-1.0, 1.0, (N, 4)), np.float32)
        kinds = {"step_1": np.array([rustsasa_amd.FIELD_STEP], np.uint8), "inv_d_1": np.array([rustsasa_amd.FIELD_INV_D], np.uint8),
                 "four_kinds_4": np.array([rustsasa_amd.FIELD_STEP, rustsasa_amd.FIELD_INV_D, rustsasa_amd.FIELD_INV_D2,
                                           rustsasa_amd.FIELD_INV_1PD], np.uint8)}
        weights = {"step_1": ones, "inv_d_1": charges, "four_kinds_4": four}
        off_c = np.zeros(N + 1, np.uint64)
        off_f = {k: np.zeros(N + 1, np.uint64) for k in kinds}
        cols = (ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S, args.probe)
        # size the per-dot buffers once
        rc = lib.rsasa_dot_crowding_batch(ctx._h, *cols, args.points, None, ptr(EDGE), 1, ptr(off_c), None, 0, None, None)
        assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL or (rc == 0 and N == 0), rc
        D = int(off_c[-1])
        counts = np.zeros((D, 1), np.uint32)
        sums = {k: np.zeros((D, len(v)), np.int64) for k, v in kinds.items()}

        def timed(fn, *a):
            t0 = time.perf_counter()
            rc = fn(ctx._h, *cols, *a)
            dt = (time.perf_counter() - t0) * 1e3
            _capi.check(rc, ctx._h)
            return dt

        def fields(k):
            return lambda: timed(lib.rsasa_dot_fields_batch, args.points, None, ptr(weights[k]), ptr(kinds[k]), len(kinds[k]),
                                 CUTOFF, ptr(off_f[k]), ptr(sums[k]), D, None, None)

        calls = {"crowding_10": lambda: timed(lib.rsasa_dot_crowding_batch, args.points, None, ptr(EDGE), 1, ptr(off_c),
                                              ptr(counts), D, None, None)}
        calls.update({k: fields(k) for k in kinds})
        for call in calls.values():  # warm-up: workspaces (and, with --kernels-only, the one launch of each kind)
            call()
        if args.kernels_only:
            print(json.dumps({"workload": wname, "atoms": N, "dots": D, "kernels_only": True, "order": list(calls)}), flush=True)
            continue
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, call in calls.items():
                times[k].append(call())
        offsets_ok = all(bool(np.array_equal(off_c, o)) for o in off_f.values())
        witness_ok = bool(np.array_equal(sums["step_1"], counts.astype(np.int64) << 24))
        med = {k: statistics.median(v) for k, v in times.items()}
        values = rustsasa_amd.field_values(sums["four_kinds_4"])
        case = {"workload": wname, "structures": S, "atoms": N, "dots": D,
                "out_bytes": {"crowding_10": int(counts.nbytes + off_c.nbytes),
                              **{k: int(sums[k].nbytes + off_f[k].nbytes) for k in kinds}},
                "ms": {k: [round(t, 2) for t in v] for k, v in times.items()},
                "median_ms": {k: round(v, 2) for k, v in med.items()},
                "step_1_to_crowding_10": round(med["step_1"] / med["crowding_10"], 3),
                "inv_d_1_to_crowding_10": round(med["inv_d_1"] / med["crowding_10"], 3),
                "four_kinds_4_to_crowding_10": round(med["four_kinds_4"] / med["crowding_10"], 3),
                "dot_offsets_equal_those_of_dot_crowding": offsets_ok,
                "step_of_ones_equals_the_crowding_counts": witness_ok,
                "dot_partner_pairs_within_10": int(counts.sum(dtype=np.int64)),
                "mean_field_per_channel": [float(v) for v in values.mean(axis=0)] if D else []}
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
