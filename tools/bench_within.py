#!/usr/bin/env python3
"""Wall time and entries per second of rsasa_atoms_within_batch (host buffers in; 8 B of offsets per atom and 8 B per
entry out) on the headline proteome (bench_workloads.synthetic_proteome()), in the two shapes whose entries fit:

    all_8        every atom centre and partner, cutoff 8 A (heavy-atom contact maps, radius graphs)
    eighth_13    one atom in eight a centre, every atom a partner, cutoff 13 A (residue-level environments)

beside rsasa_half_sphere_exposure_batch on the same input, flags and cutoff without directions as the yardstick: it is
the count pass alone (the same sweep, no lists), so the ratio of the two says what the scan, the second sweep, the sort
and the 8 bytes per entry cost.

    python tools/bench_within.py [--reps 3] [--out profiles/within_bench.json]

The two calls alternate (hse, within, hse, ...), each on preallocated pageable output buffers sized by one sizing call,
after one warm-up call each; a call's time is a host clock around the synchronous C call.  The list lengths are checked
against the yardstick's up + down.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats --
python tools/bench_within.py --kernels-only` (k_within_count, k_within_fill, k_neighbor_rank_spill next to k_half_sphere)."""
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
ap.add_argument("--shapes", nargs="+", default=["all_8", "eighth_13"])
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
    shapes = {"all_8": (None, 8.0), "eighth_13": (np.where(np.arange(N) % 8 == 0, 3, 1).astype(np.uint8), 13.0)}
    result = {"tool": "bench_within", "probe": args.probe, "reps": args.reps, "structures": S, "atoms": N, "cases": []}
    up, down = np.zeros(N, np.uint32), np.zeros(N, np.uint32)
    offsets = np.zeros(N + 1, np.uint64)
    for name in args.shapes:
        flags, cutoff = shapes[name]

        def within(entries, cap):
            t0 = time.perf_counter()
            rc = lib.rsasa_atoms_within_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S, args.probe,
                                              ptr(flags), cutoff, 0, ptr(offsets), ptr(entries), cap)
            return rc, (time.perf_counter() - t0) * 1e3

        def yardstick():
            t0 = time.perf_counter()
            rc = lib.rsasa_half_sphere_exposure_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S, args.probe,
                                                      None, ptr(flags), cutoff, ptr(up), ptr(down))
            dt = (time.perf_counter() - t0) * 1e3
            _capi.check(rc, ctx._h)
            return dt

        rc, t_size = within(None, 0)     # the sizing call: grid, count pass and scan, no entries
        assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL, rc
        total = int(offsets[-1])
        entries = np.zeros(total, _capi.WITHIN_DTYPE)   # (zeros: the pages are touched before the clock runs)

        def fill():
            rc, dt = within(entries, total)
            _capi.check(rc, ctx._h)
            return dt

        yardstick()  # warm-up: workspaces
        fill()
        if args.kernels_only:
            print(json.dumps({"shape": name, "atoms": N, "entries": total, "kernels_only": True}), flush=True)
            continue
        t_hse, t_within = [], []
        for _ in range(args.reps):
            t_hse.append(yardstick())
            t_within.append(fill())
        lengths_ok = bool(np.array_equal(np.diff(offsets.astype(np.int64)), up.astype(np.int64) + down))
        k = np.diff(offsets.astype(np.int64))
        centres = N if flags is None else int(np.count_nonzero(flags & 2))
        med_w, med_h = statistics.median(t_within), statistics.median(t_hse)
        case = {"shape": name, "cutoff": cutoff, "centres": centres, "entries": total, "out_bytes": int(entries.nbytes + offsets.nbytes),
                "mean_list": float(total / max(centres, 1)), "max_list": int(k.max()),
                "lists_above_stage": int(np.count_nonzero(k > 1024)),
                "sizing_call_ms": round(t_size, 2),
                "atoms_within_batch_ms": [round(t, 2) for t in t_within], "atoms_within_batch_median_ms": round(med_w, 2),
                "half_sphere_exposure_batch_ms": [round(t, 2) for t in t_hse],
                "half_sphere_exposure_batch_median_ms": round(med_h, 2),
                "ratio_to_hse": round(med_w / med_h, 2),
                "entries_per_second": round(total / (med_w * 1e-3)),
                "list_lengths_equal_up_plus_down": lengths_ok}
        assert lengths_ok, case
        print(json.dumps(case), flush=True)
        result["cases"].append(case)
        del entries
    ctx.close()
    if args.out and not args.kernels_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}))


main()
