#!/usr/bin/env python3
"""Wall time of rsasa_dot_links_batch and rsasa_dot_geodesics_batch (host buffers in) on the workloads of
tools/bench_enclosure.py - the headline proteome (bench_workloads.synthetic_proteome()) and real_coords (real_coords.py,
tiled to the proteome's size) - at the default link, beside one yardstick on the same input:

    components     rsasa_surface_components_batch: the same prologue (lists, masks, popcounts, scan) and the same sweep
                   over the same reach, once over unordered pairs with a union-find where the list build goes twice over
                   ordered pairs (count, fill) - of the atoms its staging cut keeps - and sorts

and the geodesics in three shapes:

    patch_12       one seed per structure (its middle dot), limit 12 A, no sources
    depth          every dot whose enclosure fraction (rsasa_dot_enclosure_batch, 30 directions, reach 10) is below 0.5 a
                   seed, no limit, no sources: the pocket depth of every dot
    front          limit 0: the call without its relaxation (one round that finds nothing), which the two above are
                   reduced by to get the time per round

    python tools/bench_geodesics.py [--reps 3] [--out profiles/geodesics_bench.json]

The calls alternate, each on preallocated pageable output buffers, after one warm-up call each; a call's time is a host
clock around the synchronous C call.  On the full workload it checks what the header promises without a model: the dot
offsets equal those of the component call, every list is as long as the count pass said, and in the depth shape a dot has
a finite distance exactly when its component (the labels of the component call) holds a seed."""
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
ap.add_argument("--points", type=int, default=100)
ap.add_argument("--limit", type=float, default=12.0)
ap.add_argument("--workloads", nargs="+", default=["proteome", "real_coords"])
ap.add_argument("--structures", type=int, default=None, help="proteome only: this many structures (default: the headline size)")
ap.add_argument("--out", default=None, help="write the JSON result here too")
args = ap.parse_args()

# the compiler's report for geodesics.hip (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage)
KERNELS = {"k_dot_link<count>": {"vgprs": 91, "sgprs": 90, "lds_bytes": 17408, "scratch": 0},
           "k_dot_link<fill>": {"vgprs": 96, "sgprs": 96, "lds_bytes": 17408, "scratch": 0},
           "k_dot_link<weights>": {"vgprs": 94, "sgprs": 99, "lds_bytes": 17408, "scratch": 0},
           "k_link_sort": {"vgprs": 16, "sgprs": 18, "lds_bytes": 0, "scratch": 0},
           "k_geo_init": {"vgprs": 16, "sgprs": 26, "lds_bytes": 0, "scratch": 0},
           "k_geo_relax": {"vgprs": 14, "sgprs": 33, "lds_bytes": 0, "scratch": 0},
           "k_geo_restamp": {"vgprs": 4, "sgprs": 14, "lds_bytes": 0, "scratch": 0},
           "k_geo_source": {"vgprs": 16, "sgprs": 37, "lds_bytes": 0, "scratch": 0}}


def workload(name):
    if name == "proteome":
        return bw.synthetic_proteome(args.structures) if args.structures else bw.synthetic_proteome()
    import real_coords as rc
    return rc.tiled(rc.quality_set_batch(), bw.synthetic_proteome().n_atoms)


def main():
    ctx = rustsasa_amd.Context(0)
    lib = _capi.load()
    result = {"tool": "bench_geodesics", "probe": args.probe, "n_points": args.points, "limit": args.limit, "reps": args.reps,
              "kernels": KERNELS, "cases": []}
    for wname in args.workloads:
        b = workload(wname)
        x, y, z, r = (np.ascontiguousarray(a, np.float32) for a in (b.x, b.y, b.z, b.radius))
        ids = np.ascontiguousarray(b.ids, np.uint64)
        so = np.ascontiguousarray(b.structure_offsets, np.uint32)
        S, N = len(so) - 1, b.n_atoms
        link = float(rustsasa_amd.default_link(r, args.probe, args.points))
        cols = (ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S, args.probe, args.points)
        off_c, off_l, off_g = (np.zeros(N + 1, np.uint64) for _ in range(3))
        n_links = np.zeros(1, np.uint64)
        rc = lib.rsasa_dot_links_batch(ctx._h, *cols, link, ptr(off_l), ptr(n_links), None, 0, None, 0, None, None)
        assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL or (rc == 0 and N == 0), rc
        D, E = int(off_l[-1]), int(n_links[0])
        labels = np.zeros(D, np.uint32)
        loff, entries = np.zeros(D + 1, np.uint64), np.empty(E, _capi.WITHIN_DTYPE)
        dist = np.zeros(D, np.float32)
        # the seeds: the middle dot of every structure; the dots that dot_enclosure calls open
        s_off = rustsasa_amd.dot_structure_offsets(off_l, so)
        one = np.zeros(D, np.uint8)
        has = np.diff(s_off) > 0
        one[((s_off[:-1] + s_off[1:]) // 2)[has]] = 1
        words = ctx.dot_enclosure_batch(x, y, z, r, ids, so, args.probe, args.points, 30, 10.0)[1]
        open_dots = (rustsasa_amd.enclosure_fraction(words, 30) < 0.5).astype(np.uint8)
        del words
        seen = {}

        def timed(fn, *a):
            t0 = time.perf_counter()
            rc = fn(ctx._h, *cols, link, *a)
            dt = (time.perf_counter() - t0) * 1e3
            _capi.check(rc, ctx._h)
            return dt

        def geo(name, seeds, limit):
            dt = timed(lib.rsasa_dot_geodesics_batch, ptr(seeds), D, limit, ptr(off_g), ptr(dist), None, None, None)
            seen[name] = (ctx.geodesic_rounds()[0], int(np.isfinite(dist).sum()),
                          float(dist[np.isfinite(dist)].max()) if np.isfinite(dist).any() else 0.0)
            return dt

        calls = {"components": lambda: timed(lib.rsasa_surface_components_batch, ptr(off_c), ptr(labels), D, None, None),
                 "links": lambda: timed(lib.rsasa_dot_links_batch, ptr(off_l), ptr(n_links), ptr(loff), D, ptr(entries), E,
                                        None, None),
                 "front": lambda: geo("front", one, 0.0),
                 "patch_12": lambda: geo("patch_12", one, args.limit),
                 "depth": lambda: geo("depth", open_dots, float("inf"))}
        for call in calls.values():
            call()
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, call in calls.items():
                times[k].append(call())
        med = {k: statistics.median(v) for k, v in times.items()}
        # (after the last call dist holds the depth shape)
        base = np.repeat(s_off[:-1], np.diff(s_off))
        glabel = labels.astype(np.int64) + base
        seeded = np.zeros(D, bool)
        seeded[glabel[open_dots != 0]] = True
        reach_ok = bool(np.array_equal(np.isfinite(dist), seeded[glabel]))
        offsets_ok = bool(np.array_equal(off_c, off_l) and np.array_equal(off_c, off_g))
        lists_ok = bool(int(loff[-1]) == E and E % 2 == 0 and (np.diff(loff.astype(np.int64)) >= 0).all())
        lengths = np.diff(loff.astype(np.int64))
        per_round = {k: round((med[k] - med["front"]) / max(seen[k][0], 1), 4) for k in ("patch_12", "depth")}
        case = {"workload": wname, "structures": S, "atoms": N, "dots": D, "entries": E, "link": link,
                "entries_per_dot": {"mean": round(E / max(D, 1), 3), "max": int(lengths.max()) if D else 0},
                "out_bytes": {"links": int(off_l.nbytes + loff.nbytes + entries.nbytes), "geodesics": int(off_g.nbytes + dist.nbytes),
                              "components": int(off_c.nbytes + labels.nbytes)},
                "ms": {k: [round(t, 2) for t in v] for k, v in times.items()},
                "median_ms": {k: round(v, 2) for k, v in med.items()},
                "links_to_components": round(med["links"] / med["components"], 3),
                "geodesics_front_to_components": round(med["front"] / med["components"], 3),
                "rounds": {k: seen[k][0] for k in seen}, "dots_reached": {k: seen[k][1] for k in seen},
                "farthest": {k: round(seen[k][2], 3) for k in seen},
                "seeds": {"patch_12": int(one.sum()), "depth": int(open_dots.sum())},
                "ms_per_round": per_round,
                "dot_offsets_equal_those_of_surface_components": offsets_ok, "lists_as_long_as_counted": lists_ok,
                "finite_exactly_in_the_seeded_components": reach_ok}
        assert offsets_ok and lists_ok and reach_ok, case
        print(json.dumps(case), flush=True)
        result["cases"].append(case)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}))


main()
