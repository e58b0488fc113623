#!/usr/bin/env python3
"""Kernel and wall times of rsasa_group_contacts_batch next to rsasa_contact_points_batch (this build's, or another
build's through --lib) on one seeded input: a shard of the headline proteome workload
(bench_workloads.synthetic_proteome(), structures 0, k, 2k, ...; default k = 8, about 1.5 M atoms), labelled per
residue (its residue_offsets) or per chain (every structure cut into three runs of residues: the workload has no
chains of its own).

The calls are synchronous host calls (upload, grid, lists, kernels, download), so the KERNEL times are taken from the
GPU's own timestamps, one run per variant under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/residue -- python tools/bench_groups.py --call group --labels residue
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/chain   -- python tools/bench_groups.py --call group --labels chain
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/contact -- python tools/bench_groups.py --call contact --lib PARENT/librustsasa_amd.so
    python tools/bench_groups.py --collect profiles/groups_bench.json --commit PARENT_COMMIT \\
        residue=OUT/residue/..._kernel_stats.csv chain=... contact=... [NAME.wall=the JSON line a run printed]

Each run prints one JSON line with the median wall time of its call per point count.  --collect reads the kernel
statistics (k_group_order, k_group_points<NCH>, k_contact_points<NCH>; NCH = 2 at 100 points, 4 at 960) and writes the
per-call kernel times and their ratio to the contact kernel's."""
import argparse
import csv
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench_workloads as bw  # noqa: E402
from rustsasa_amd import _capi  # noqa: E402
from rustsasa_amd._capi import ptr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--call", choices=["group", "contact"], default="group")
ap.add_argument("--labels", choices=["residue", "chain"], default="residue")
ap.add_argument("--lib", help="librustsasa_amd.so of another build (contact only: the parent commit's)")
ap.add_argument("--shard", type=int, default=8, help="take structures 0, k, 2k, ... of the proteome")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--probe", type=float, default=1.4)
ap.add_argument("--points", type=int, nargs="+", default=[100, 960])
ap.add_argument("--collect", metavar="OUT.json", help="assemble NAME=kernel_stats.csv / NAME.wall=run.json into OUT.json")
ap.add_argument("--commit", default=None, help="--collect: the commit the contact figures were taken on")
ap.add_argument("inputs", nargs="*")
args = ap.parse_args()


def workload():
    b = bw.synthetic_proteome()
    return bw.shard(b, 0, args.shard) if args.shard > 1 else b


def group_labels(b, kind):
    ro = b.residue_offsets.astype(np.int64)
    residue = np.repeat(np.arange(len(ro) - 1, dtype=np.int64), np.diff(ro))
    if kind == "residue":
        return residue.astype(np.uint32)
    # three chains per structure: the structure's residues in three runs of equal length
    so = b.structure_offsets.astype(np.int64)
    first = np.repeat(residue[so[:-1]], np.diff(so))
    count = np.repeat(residue[so[1:] - 1] - residue[so[:-1]] + 1, np.diff(so))
    return ((residue - first) * 3 // count).astype(np.uint32)


def run():
    b = workload()
    x, y, z, r = (np.ascontiguousarray(a, np.float32) for a in (b.x, b.y, b.z, b.radius))
    ids = np.ascontiguousarray(b.ids, np.uint64)
    so = np.ascontiguousarray(b.structure_offsets, np.uint32)
    S, N = len(so) - 1, len(x)
    if args.lib:
        lib = C.CDLL(os.path.abspath(args.lib))
        for name in ("rsasa_context_create", "rsasa_context_destroy", "rsasa_contact_points_batch"):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = _capi.SYMBOLS[name]
    else:
        lib = _capi.load()
    h = C.c_void_p()
    _capi.check(lib.rsasa_context_create(0, C.byref(h)))
    offsets, sasa = np.zeros(N + 1, np.uint64), np.zeros(N, np.float32)
    if args.call == "group":
        assert not args.lib, "the group call is this build's"
        g = group_labels(b, args.labels)
        self_free, free = np.zeros(N, np.uint32), np.zeros(N, np.uint32)

        def call(bufs, cap, n_points):
            return lib.rsasa_group_contacts_batch(h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(g), ptr(so), S, args.probe,
                                                  n_points, ptr(offsets), *(ptr(a) for a in bufs), cap, ptr(self_free),
                                                  ptr(free), ptr(sasa))
        dtypes = (np.uint32, np.uint32, np.uint32)
    else:
        def call(bufs, cap, n_points):
            return lib.rsasa_contact_points_batch(h, ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S, args.probe,
                                                  n_points, ptr(offsets), *(ptr(a) for a in bufs), cap, ptr(sasa))
        dtypes = (_capi.NEIGHBOR_DTYPE, np.uint32, np.uint32)
    assert call((None, None, None), 0, 100) == _capi.RSASA_ERR_BUFFER_TOO_SMALL
    total = int(offsets[-1])
    bufs = [np.zeros(total, d) for d in dtypes]
    out = {"tool": "bench_groups", "call": args.call, "labels": args.labels if args.call == "group" else None,
           "lib": args.lib or "this build", "shard": args.shard, "structures": S, "atoms": N, "rows_or_entries": total,
           "probe": args.probe, "reps": args.reps, "wall_ms": {}}
    for n_points in args.points:
        assert call(bufs, total, n_points) == 0   # warm-up: workspaces, lattice
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            assert call(bufs, total, n_points) == 0
            ts.append((time.perf_counter() - t0) * 1e3)
        out["wall_ms"][str(n_points)] = round(statistics.median(ts), 2)
    lib.rsasa_context_destroy(h)
    print(json.dumps(out), flush=True)


KERNELS = re.compile(r"\b(k_group_order|k_group_points<\d>|k_contact_points<\d>)")


def collect():
    result = {"tool": "bench_groups", "contact_points_commit": args.commit, "kernel_us_per_call": {}, "wall": {}}
    for item in args.inputs:
        name, path = item.split("=", 1)
        if name.endswith(".wall"):
            result["wall"][name[:-5]] = json.loads(open(path).read().strip().splitlines()[-1])
            continue
        rows = {}
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                m = KERNELS.search(row["Name"])
                if m:
                    rows[m.group(1)] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 1),
                                        "min_us": round(int(row["MinNs"]) / 1e3, 1), "max_us": round(int(row["MaxNs"]) / 1e3, 1)}
        result["kernel_us_per_call"][name] = rows
    k = result["kernel_us_per_call"]
    if "contact" in k:
        ratios = {}
        for name in k:
            if name == "contact":
                continue
            for nch, points in (("2", "100"), ("4", "960")):
                ct = k["contact"].get(f"k_contact_points<{nch}>")
                gp = k[name].get(f"k_group_points<{nch}>")
                if ct and gp:
                    order = k[name]["k_group_order"]["average_us"]
                    ratios[f"{name}_{points}_points"] = {
                        "group_points_over_contact_points": round(gp["average_us"] / ct["average_us"], 3),
                        "with_group_order": round((gp["average_us"] + order) / ct["average_us"], 3)}
        result["ratio_to_contact_kernel"] = ratios
    os.makedirs(os.path.dirname(os.path.abspath(args.collect)), exist_ok=True)
    with open(args.collect, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result.get("ratio_to_contact_kernel", {})))


if args.collect:
    collect()
else:
    run()
