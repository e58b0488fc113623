#!/usr/bin/env python3
"""Wall time of rsasa_contact_owners_batch (host buffers in; lists, one count per entry and values out), without and
with out_owner (4 B per atom and point more, reserved, written and copied only when asked for), beside
rsasa_contact_points_batch of the same build on the same input: the same upload, grid, lists and downloads but for one
count per entry less, and a kernel of one sweep of the list per pass where k_contact_points makes two.  Inputs: the
workloads of tools/bench_points.py - the headline proteome (bench_workloads.synthetic_proteome()) and real_coords
(real_coords.py, tiled to the proteome's size) - at 100 and 960 points.

    python tools/bench_owners.py [--reps 5] [--out profiles/contact_owners_bench.json]

The calls alternate (contact_points, owners, owners with out_owner, contact_points, ...), each on preallocated
pageable output buffers, after one warm-up call each; a call's time is a host clock around the synchronous C call.
The leg with out_owner is left out (null) where the owner table would pass --owner-max-gib of host memory.  The
results are tied together before they are reported: the lists and values of the two families are equal, owned lies
between exclusive and covered, and owned and the owner table say the same.  Kernel times come from a separate run
under `rocprofv3 --kernel-trace --stats -- python tools/bench_owners.py --kernels-only` (k_contact_owners next to
k_contact_points on the same input)."""
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
ap.add_argument("--owner-max-gib", type=float, default=8.0, help="largest owner table (host memory) the third leg may take")
ap.add_argument("--kernels-only", action="store_true", help="one call of each kind per input (for rocprofv3), no timing")
ap.add_argument("--out", default=None, help="write the JSON result here too")
args = ap.parse_args()


def workload(name):
    if name == "proteome":
        return bw.synthetic_proteome(args.structures) if args.structures else bw.synthetic_proteome()
    import real_coords as rc
    return rc.tiled(rc.quality_set_batch(), bw.synthetic_proteome().n_atoms)


def median(ts):
    return round(statistics.median(ts), 2)


def main():
    ctx = rustsasa_amd.Context(0)
    lib = _capi.load()
    result = {"tool": "bench_owners", "probe": args.probe, "reps": args.reps, "cases": []}
    for wname in args.workloads:
        b = workload(wname)
        x, y, z, r = (np.ascontiguousarray(a, np.float32) for a in (b.x, b.y, b.z, b.radius))
        ids = np.ascontiguousarray(b.ids, np.uint64)
        so = np.ascontiguousarray(b.structure_offsets, np.uint32)
        S, N = len(so) - 1, b.n_atoms
        offsets = np.zeros(N + 1, np.uint64)
        rc = lib.rsasa_contact_owners_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S, args.probe, 100,
                                            ptr(offsets), None, None, 0, None, None)
        assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL, rc
        total = int(offsets[-1])
        entries, c_entries = np.zeros(total, _capi.NEIGHBOR_DTYPE), np.zeros(total, _capi.NEIGHBOR_DTYPE)
        owned, cov, exc = (np.zeros(total, np.uint32) for _ in range(3))
        sasa, c_sasa, c_offsets = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros(N + 1, np.uint64)
        for n_points in args.points:
            with_owner = N * n_points * 4 <= args.owner_max_gib * 2 ** 30
            owner = np.zeros((N, n_points), np.uint32) if with_owner else None

            def timed(f):
                t0 = time.perf_counter()
                rc = f()
                dt = (time.perf_counter() - t0) * 1e3
                _capi.check(rc, ctx._h)
                return dt

            def contact_points():
                return lib.rsasa_contact_points_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S,
                                                      args.probe, n_points, ptr(c_offsets), ptr(c_entries), ptr(cov),
                                                      ptr(exc), total, ptr(c_sasa))

            def owners(table=None):
                return lib.rsasa_contact_owners_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S,
                                                      args.probe, n_points, ptr(offsets), ptr(entries), ptr(owned), total,
                                                      ptr(table), ptr(sasa))
            calls = {"contact_points_batch": contact_points, "contact_owners_batch": owners}
            if with_owner:
                calls["contact_owners_batch_with_owner"] = lambda: owners(owner)
            for f in calls.values():  # warm-up: workspaces, lattice
                timed(f)
            if args.kernels_only:
                continue
            times = {k: [] for k in calls}
            for _ in range(args.reps):
                for k, f in calls.items():
                    times[k].append(timed(f))
            case = {"workload": wname, "structures": S, "atoms": N, "entries": total, "n_points": n_points,
                    "owner_table_bytes": int(N * n_points * 4)}
            for k in ("contact_points_batch", "contact_owners_batch", "contact_owners_batch_with_owner"):
                case[k + "_ms"] = [round(t, 2) for t in times[k]] if k in times else None
                case[k + "_median_ms"] = median(times[k]) if k in times else None
            base = statistics.median(times["contact_points_batch"])
            case["owners_over_contact_points"] = round(statistics.median(times["contact_owners_batch"]) / base, 3)
            case["owners_with_owner_over_contact_points"] = (
                round(statistics.median(times["contact_owners_batch_with_owner"]) / base, 3) if with_owner else None)
            case["lists_and_values_equal"] = bool(np.array_equal(offsets, c_offsets) and sasa.tobytes() == c_sasa.tobytes()
                                                  and entries.tobytes() == c_entries.tobytes())
            case["owned_between_exclusive_and_covered"] = bool(np.all(exc <= owned) and np.all(owned <= cov))
            case["owned_total"] = int(owned.sum(dtype=np.uint64))
            if with_owner:
                # per atom: the points the table gives away are the points its entries own
                per_atom = np.diff(np.concatenate([[0], np.cumsum(owned, dtype=np.int64)])[offsets.astype(np.int64)])
                case["owner_table_agrees_with_owned"] = bool(
                    np.array_equal(np.count_nonzero(owner != 0xFFFFFFFF, axis=1), per_atom))
                del per_atom
            for k in ("lists_and_values_equal", "owned_between_exclusive_and_covered", "owner_table_agrees_with_owned"):
                assert case.get(k, True), case
            print(json.dumps(case), flush=True)
            result["cases"].append(case)
            del owner
        print(json.dumps({"workload": wname, "atoms": N, "done": True}), flush=True)
        del entries, c_entries, owned, cov, exc
    ctx.close()
    if args.out and not args.kernels_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}))


main()
