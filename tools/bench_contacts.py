#!/usr/bin/env python3
"""Wall time of rsasa_contact_points_batch (host buffers in; lists, per-entry counts and values out) next to another
build's rsasa_precompute_neighbors_batch and rsasa_accessible_points_batch on the same inputs.  All three run the same
upload, grid, count and fill; the contact call adds a kernel and downloads 8 + 4 + 4 B per entry.  Inputs: the
headline proteome workload (bench_workloads.synthetic_proteome()) and the real_coords workload (real_coords.py, tiled
to the proteome's size), at 100 and 960 points.

    python tools/bench_contacts.py --baseline-lib OTHER/librustsasa_amd.so [--reps 5] [--out profiles/contacts_bench.json]

The calls alternate (baseline lists, baseline points, new, ...), each on preallocated pageable output buffers, each
library in a context of its own.  --host-route also times the way to the same counts without this call, on the
untiled quality set (real_coords.quality_set_batch(), 100 points): the baseline's precompute_neighbors_batch, then
tests/contacts_model.py on the host over up to 16 threads, one structure per task; the counts of the two routes are
compared.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_contacts.py --kernels-only` (k_contact_points next to
k_accessible_points on the same input)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench_workloads as bw  # noqa: E402
import rustsasa_amd  # noqa: E402
from rustsasa_amd import _capi  # noqa: E402
from rustsasa_amd._capi import ptr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--baseline-lib", help="librustsasa_amd.so of the build to compare with")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--probe", type=float, default=1.4)
ap.add_argument("--points", type=int, nargs="+", default=[100, 960])
ap.add_argument("--workloads", nargs="+", default=["proteome", "real_coords"])
ap.add_argument("--host-route", action="store_true", help="the quality-set comparison with the host model (needs --baseline-lib)")
ap.add_argument("--kernels-only", action="store_true",
                help="one contact_points_batch and one accessible_points_batch per input (for rocprofv3), no timing")
ap.add_argument("--out", default=None, help="write the JSON result here too")
args = ap.parse_args()


def workload(name):
    import real_coords as rc
    if name == "proteome":
        return bw.synthetic_proteome()
    if name == "quality_set":
        return rc.quality_set_batch()
    return rc.tiled(rc.quality_set_batch(), bw.synthetic_proteome().n_atoms)


def columns(b):
    x, y, z, r = (np.ascontiguousarray(a, np.float32) for a in (b.x, b.y, b.z, b.radius))
    return x, y, z, r, np.ascontiguousarray(b.ids, np.uint64), np.ascontiguousarray(b.structure_offsets, np.uint32)


def timed(f):
    t0 = time.perf_counter()
    rc = f()
    dt = (time.perf_counter() - t0) * 1e3
    assert rc == 0, rc
    return dt


def median(ts):
    return round(statistics.median(ts), 2)


class Baseline:
    def __init__(self, path):
        self.lib = C.CDLL(os.path.abspath(path))
        for name in ("rsasa_context_create", "rsasa_context_destroy", "rsasa_precompute_neighbors_batch",
                     "rsasa_accessible_points_batch"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _capi.SYMBOLS[name]
        h = C.c_void_p()
        _capi.check(self.lib.rsasa_context_create(0, C.byref(h)))
        self.h = h

    def lists(self, x, y, z, r, ids, so, offsets, entries, cap):
        return self.lib.rsasa_precompute_neighbors_batch(self.h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so),
                                                         len(so) - 1, args.probe, float("nan"), ptr(offsets),
                                                         ptr(entries), cap)

    def points(self, x, y, z, r, ids, so, n_points, masks, sasa):
        return self.lib.rsasa_accessible_points_batch(self.h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so),
                                                      len(so) - 1, args.probe, n_points, ptr(masks), ptr(sasa))

    def close(self):
        self.lib.rsasa_context_destroy(self.h)


def host_route(ctx, lib, base):
    """The quality set at 100 points: this call against the baseline's lists + the host model (the counts compared)."""
    import contacts_model as cm
    x, y, z, r, ids, so = columns(workload("quality_set"))
    N, n_points = len(x), 100
    offsets = np.zeros(N + 1, np.uint64)
    assert base.lists(x, y, z, r, ids, so, offsets, None, 0) == _capi.RSASA_ERR_BUFFER_TOO_SMALL
    total = int(offsets[-1])
    entries = np.zeros(total, _capi.NEIGHBOR_DTYPE)
    cov, exc, sasa = np.zeros(total, np.uint32), np.zeros(total, np.uint32), np.zeros(N, np.float32)

    def new():
        return lib.rsasa_contact_points_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), len(so) - 1,
                                              args.probe, n_points, ptr(offsets), ptr(entries), ptr(cov), ptr(exc),
                                              total, ptr(sasa))
    new()
    t_new = [timed(new) for _ in range(args.reps)]
    try:
        threads = max(1, min(16, len(os.sched_getaffinity(0))))
    except AttributeError:
        threads = max(1, min(16, os.cpu_count() or 1))
    b_off = np.zeros(N + 1, np.uint64)
    b_ent = np.zeros(total, _capi.NEIGHBOR_DTYPE)

    def one(s):
        b, e = int(so[s]), int(so[s + 1])
        lo, hi = int(b_off[b]), int(b_off[e])
        lists = (b_off[b:e + 1] - b_off[b], b_ent[lo:hi])
        _, _, c, xx = cm.contact_counts(x[b:e], y[b:e], z[b:e], r[b:e], ids[b:e], args.probe, n_points, 8, lists)
        return c, xx
    t0 = time.perf_counter()
    assert base.lists(x, y, z, r, ids, so, b_off, b_ent, total) == 0
    t_lists = (time.perf_counter() - t0) * 1e3
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(one, range(len(so) - 1)))
    t_route = (time.perf_counter() - t0) * 1e3
    same = (np.array_equal(np.concatenate([p[0] for p in parts]), cov)
            and np.array_equal(np.concatenate([p[1] for p in parts]), exc) and np.array_equal(b_off, offsets)
            and b_ent.tobytes() == entries.tobytes())
    return {"workload": "quality_set", "structures": len(so) - 1, "atoms": N, "entries": total, "n_points": n_points,
            "contact_points_batch_ms": [round(t, 2) for t in t_new], "contact_points_batch_median_ms": median(t_new),
            "host_route_ms": round(t_route, 1), "host_route_lists_ms": round(t_lists, 1), "host_route_threads": threads,
            "host_route_counts_equal": bool(same), "new_faster": statistics.median(t_new) < t_route}


def main():
    ctx = rustsasa_amd.Context(0)
    lib = _capi.load()
    base = Baseline(args.baseline_lib) if args.baseline_lib and not args.kernels_only else None
    result = {"tool": "bench_contacts", "probe": args.probe, "reps": args.reps, "cases": []}
    for wname in args.workloads:
        x, y, z, r, ids, so = columns(workload(wname))
        S, N = len(so) - 1, len(x)
        if args.kernels_only:
            for n_points in args.points:
                ctx.contact_points_batch(x, y, z, r, ids, so, args.probe, n_points)
                ctx.accessible_points_batch(x, y, z, r, ids, so, args.probe, n_points)
            print(json.dumps({"workload": wname, "atoms": N, "kernels_only": True}), flush=True)
            continue
        offsets = np.zeros(N + 1, np.uint64)
        rc = lib.rsasa_contact_points_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S, args.probe,
                                            100, ptr(offsets), None, None, None, 0, None)
        assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL, rc
        total = int(offsets[-1])
        entries = np.zeros(total, _capi.NEIGHBOR_DTYPE)
        cov, exc, sasa = np.zeros(total, np.uint32), np.zeros(total, np.uint32), np.zeros(N, np.float32)
        b_off, b_ent = np.zeros(N + 1, np.uint64), (np.zeros(total, _capi.NEIGHBOR_DTYPE) if base else None)
        b_sasa = np.zeros(N, np.float32)
        for n_points in args.points:
            masks = np.zeros((N, (n_points + 31) // 32), np.uint32) if base else None

            def new():
                return lib.rsasa_contact_points_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S,
                                                      args.probe, n_points, ptr(offsets), ptr(entries), ptr(cov),
                                                      ptr(exc), total, ptr(sasa))
            calls = {"contact_points_batch": new}
            if base:
                calls["baseline_precompute_neighbors_batch"] = lambda: base.lists(x, y, z, r, ids, so, b_off, b_ent, total)
                calls["baseline_accessible_points_batch"] = lambda: base.points(x, y, z, r, ids, so, n_points, masks, b_sasa)
            for f in calls.values():  # warm-up: workspaces, lattice
                f()
            times = {k: [] for k in calls}
            for _ in range(args.reps):
                for k in reversed(list(calls)):  # baselines first, then the new call
                    times[k].append(timed(calls[k]))
            case = {"workload": wname, "structures": S, "atoms": N, "entries": total, "n_points": n_points,
                    "output_bytes": int(offsets.nbytes + entries.nbytes + cov.nbytes + exc.nbytes + sasa.nbytes)}
            for k, ts in times.items():
                case[k + "_ms"] = [round(t, 2) for t in ts]
                case[k + "_median_ms"] = median(ts)
            if base:
                case["lists_equal"] = bool(np.array_equal(b_off, offsets) and b_ent.tobytes() == entries.tobytes())
                case["sasa_equal"] = bool(b_sasa.tobytes() == sasa.tobytes())
            print(json.dumps(case), flush=True)
            result["cases"].append(case)
        del entries, cov, exc, b_ent
    if base is not None and args.host_route:
        result["host_route"] = host_route(ctx, lib, base)
        print(json.dumps(result["host_route"]), flush=True)
    if base is not None:
        base.close()
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}))


main()
