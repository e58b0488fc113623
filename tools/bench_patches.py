#!/usr/bin/env python3
"""Wall time of rsasa_dot_patches_batch (host buffers in) on the workloads of tools/bench_geodesics.py - the headline
proteome (bench_workloads.synthetic_proteome()) and real_coords (real_coords.py, tiled to the proteome's size) - at the
default link and spacings of 12 A and 6 A, beside two yardsticks:

    front          rsasa_dot_geodesics_batch at limit 0 on the same input: grid, masks, dots and lists, and one round that
                   finds nothing - the front end the patches share, so the difference is the sampler (and, with sources,
                   the source phase)
    host loop      what a caller had before this call: rsasa_dot_geodesics_batch once per pick with all centres so far
                   as seeds, a numpy argmax per structure between the calls - every structure of the sub-batch picks in
                   the same call, which is the loop at its best.  On the first --loop-structures structures only (it would
                   not finish on the workload), against the new call on the SAME sub-batch; the two must return the same
                   centres and the same distances.

    python tools/bench_patches.py [--reps 3] [--out profiles/patches_bench.json]

The calls alternate, each on preallocated pageable output buffers, after one warm-up call each; a call's time is a host
clock around the synchronous C call.  On the full workload it checks what the header promises without a model: the covers
of every structure do not rise, every dist is <= spacing, every centre has dist 0 and itself as source, and the picks of
rsasa_context_patch_stats equal the centres returned."""
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
ap.add_argument("--spacings", type=float, nargs="+", default=[12.0, 6.0])
ap.add_argument("--workloads", nargs="+", default=["proteome", "real_coords"])
ap.add_argument("--structures", type=int, default=None, help="proteome only: this many structures (default: the headline size)")
ap.add_argument("--loop-structures", type=int, default=16, help="the sub-batch of the host loop")
ap.add_argument("--out", default=None, help="write the JSON result here too")
args = ap.parse_args()

# the compiler's report for patches.hip (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage)
KERNELS = {"k_patch_init": {"vgprs": 10, "sgprs": 16, "lds_bytes": 0, "scratch": 0},
           "k_patch_sample": {"vgprs": 42, "sgprs": 95, "lds_bytes": 8232, "scratch": 0},
           "k_patch_pack": {"vgprs": 11, "sgprs": 26, "lds_bytes": 0, "scratch": 0}}


def workload(name):
    if name == "proteome":
        return bw.synthetic_proteome(args.structures) if args.structures else bw.synthetic_proteome()
    import real_coords as rc
    return rc.tiled(rc.quality_set_batch(), bw.synthetic_proteome().n_atoms)


class Input:
    """The columns of structures [0, n_struct) of a batch, the link of the WHOLE batch, and the buffers of the calls."""

    def __init__(self, ctx, lib, b, link, n_struct=None):
        so = np.ascontiguousarray(b.structure_offsets, np.uint32)
        if n_struct is not None:
            so = so[:n_struct + 1].copy()
        n = int(so[-1])
        self.ctx, self.lib, self.so, self.S, self.N, self.link = ctx, lib, so, len(so) - 1, n, link
        self.x, self.y, self.z, self.r = (np.ascontiguousarray(a[:n], np.float32) for a in (b.x, b.y, b.z, b.radius))
        self.ids = np.ascontiguousarray(b.ids[:n], np.uint64)
        self.cols = (ptr(self.x), ptr(self.y), ptr(self.z), ptr(self.r), ptr(self.ids), ptr(so), self.S, args.probe, args.points)
        self.off, self.bound = np.zeros(n + 1, np.uint64), np.zeros(1, np.uint64)
        rc = lib.rsasa_dot_patches_batch(ctx._h, *self.cols, link, 6.0, 0xFFFFFFFF, ptr(self.off), ptr(self.bound), None, None,
                                         None, 0, None, None, 0, None, None)
        assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL or (rc == 0 and n == 0), rc
        self.D = D = int(self.off[-1])
        assert int(self.bound[0]) == D
        self.c_off = np.zeros(self.S + 1, np.uint64)
        self.centres, self.cover = np.zeros(D, np.uint32), np.zeros(D, np.float32)
        self.dist, self.source = np.zeros(D, np.float32), np.zeros(D, np.uint32)
        self.g_off, self.g_dist = np.zeros(n + 1, np.uint64), np.zeros(D, np.float32)
        self.s_off = rustsasa_amd.dot_structure_offsets(self.off, so)

    def timed(self, fn, *a):
        t0 = time.perf_counter()
        rc = fn(self.ctx._h, *self.cols, self.link, *a)
        dt = (time.perf_counter() - t0) * 1e3
        _capi.check(rc, self.ctx._h)
        return dt

    def patches(self, spacing, sources=True):
        return self.timed(self.lib.rsasa_dot_patches_batch, spacing, 0xFFFFFFFF, ptr(self.off), ptr(self.bound), ptr(self.c_off),
                          ptr(self.centres), ptr(self.cover), self.D, ptr(self.dist), ptr(self.source) if sources else None,
                          self.D, None, None)

    def geodesics(self, seeds, limit):
        return self.timed(self.lib.rsasa_dot_geodesics_batch, ptr(seeds), self.D, limit, ptr(self.g_off), ptr(self.g_dist),
                          None, None, None)

    def host_loop(self, spacing):
        """(ms, calls, centres per structure in pick order): dot_geodesics_batch once per round of picks."""
        spacing = np.float32(spacing)
        seeds = np.zeros(self.D, np.uint8)
        dist = np.full(self.D, np.inf, np.float32)
        picked = [[] for _ in range(self.S)]
        active = [s for s in range(self.S) if self.s_off[s + 1] > self.s_off[s]]
        calls = 0
        t0 = time.perf_counter()
        while True:
            still = []
            for s in active:
                seg = dist[self.s_off[s]:self.s_off[s + 1]]
                c = int(np.argmax(seg))
                if np.isfinite(seg[c]) and seg[c] <= spacing:
                    continue
                seeds[self.s_off[s] + c] = 1
                picked[s].append(c)
                still.append(s)
            active = still
            if not active:
                break
            self.geodesics(seeds, float("inf"))
            dist, self.g_dist = self.g_dist, dist
            calls += 1
        return (time.perf_counter() - t0) * 1e3, calls, picked, dist


def main():
    ctx = rustsasa_amd.Context(0)
    lib = _capi.load()
    result = {"tool": "bench_patches", "probe": args.probe, "n_points": args.points, "spacings": args.spacings, "reps": args.reps,
              "kernels": KERNELS, "queue": 1024, "workgroup": 256, "cases": []}
    for wname in args.workloads:
        b = workload(wname)
        link = float(rustsasa_amd.default_link(np.ascontiguousarray(b.radius, np.float32), args.probe, args.points))
        full = Input(ctx, lib, b, link)
        none = np.zeros(full.D, np.uint8)
        seen = {}

        def patch(inp, spacing, sources=True):
            dt = inp.patches(spacing, sources)
            seen[spacing] = ctx.patch_stats()
            return dt

        calls = {"front": lambda: full.geodesics(none, 0.0)}
        for sp in args.spacings:
            calls[f"patches_{sp:g}"] = lambda sp=sp: patch(full, sp)
            calls[f"patches_{sp:g}_no_source"] = lambda sp=sp: patch(full, sp, False)
        for call in calls.values():
            call()
        times = {k: [] for k in calls}
        checks = {}
        for _ in range(args.reps):
            for k, call in calls.items():
                times[k].append(call())
                if k.startswith("patches_") and not k.endswith("no_source") and k not in checks:
                    sp = np.float32(float(k.split("_")[1]))
                    K = int(full.c_off[-1])
                    base = np.repeat(full.s_off[:-1], np.diff(full.c_off.astype(np.int64)))
                    at = full.centres[:K].astype(np.int64) + base
                    cv = full.cover[:K]
                    first = np.zeros(K, bool)
                    first[full.c_off[:-1][np.diff(full.c_off.astype(np.int64)) > 0].astype(np.int64)] = True
                    checks[k] = {"centres": K, "picks": seen[float(sp)][0], "steps": seen[float(sp)][1], "overflows": seen[float(sp)][2],
                                 "covers_do_not_rise": bool((first[1:] | (cv[1:] <= cv[:-1])).all()),
                                 "every_dist_within_spacing": bool((full.dist <= sp).all()),
                                 "centres_are_their_own_source": bool((not full.dist[at].any()) and
                                                                      np.array_equal(full.source[at], full.centres[:K])),
                                 "farthest": round(float(full.dist.max()) if full.D else 0.0, 3)}
                    assert checks[k]["covers_do_not_rise"] and checks[k]["every_dist_within_spacing"], checks[k]
                    assert checks[k]["centres_are_their_own_source"] and checks[k]["picks"] == K, checks[k]
        med = {k: statistics.median(v) for k, v in times.items()}
        # ---- the host loop of the parent commit against the new call, on the same sub-batch
        sub = Input(ctx, lib, b, link, min(args.loop_structures, full.S))
        loops = {}
        for sp in args.spacings:
            sub.patches(sp, False)
            sub.geodesics(np.zeros(sub.D, np.uint8), 0.0)              # (a warm-up of the loop's call at this size)
            t_new, t_loop = [], []
            for _ in range(args.reps):
                t_new.append(sub.patches(sp, False))
                ms, n_calls, picked, dist = sub.host_loop(sp)
                t_loop.append(ms)
            got = [sub.centres[int(sub.c_off[s]):int(sub.c_off[s + 1])].tolist() for s in range(sub.S)]
            same = bool(got == picked and dist.tobytes() == sub.dist.tobytes())
            assert same, (wname, sp)
            loops[f"{sp:g}"] = {"structures": sub.S, "atoms": sub.N, "dots": sub.D, "centres": int(sub.c_off[-1]), "loop_calls": n_calls,
                                "new_ms": [round(t, 2) for t in t_new], "loop_ms": [round(t, 2) for t in t_loop],
                                "median_new_ms": round(statistics.median(t_new), 2),
                                "median_loop_ms": round(statistics.median(t_loop), 2),
                                "loop_to_new": round(statistics.median(t_loop) / statistics.median(t_new), 2),
                                "new_spread_ms": round(max(t_new) - min(t_new), 2), "loop_spread_ms": round(max(t_loop) - min(t_loop), 2),
                                "loop_returns_the_same_centres_and_dist": same}
        case = {"workload": wname, "structures": full.S, "atoms": full.N, "dots": full.D, "link": link,
                "ms": {k: [round(t, 2) for t in v] for k, v in times.items()},
                "median_ms": {k: round(v, 2) for k, v in med.items()},
                "sampler_ms": {f"{sp:g}": round(med[f"patches_{sp:g}_no_source"] - med["front"], 2) for sp in args.spacings},
                "source_phase_ms": {f"{sp:g}": round(med[f"patches_{sp:g}"] - med[f"patches_{sp:g}_no_source"], 2) for sp in args.spacings},
                "checks": checks, "host_loop": loops}
        print(json.dumps(case), flush=True)
        result["cases"].append(case)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}))


main()
