#!/usr/bin/env python3
"""Wall time of rsasa_dot_curvature_batch (host buffers in; 8 B per atom and 68 B per dot come back) on the workloads of
tools/bench_fields.py - the proteome (bench_workloads.synthetic_proteome) and real_coords (real_coords.py, tiled to the
same number of atoms) - at 100 points and the reaches 1.5, 3.0 and 6.0, beside its yardstick on the same input in the same
process:

    links      rsasa_dot_links_batch at link = reach: the parent's way to the same pairs - the same ordered-pair sweep
               twice (count, fill), a sort, and 8 B per entry back, which the caller then reduces on the host

    python tools/bench_curvature.py [--reps 3] [--structures 200] [--out profiles/curvature_bench.json]

The lists of the links grow with the cube of the reach - about 100 entries per dot at 6 A -, so the comparison runs on the
first --structures structures of the proteome (default 200: about 3.4 million dots, 2.7 GB of entries at 6 A) and on
real_coords tiled to as many atoms; --full adds the time of the curvature call alone on the headline proteome at 3 A.
The two calls alternate, each on preallocated pageable output buffers, after one warm-up call each; a call's time is a
host clock around the synchronous C call.  Per reach it checks the identities of the header:
    pairs    pairs[d] equals the length of dot d's list less its entries with d2 == 0 - on every dot; a dot where the two
             differ is re-evaluated here from the definition (numpy float32), and must have dropped exactly that many
             pairs by t2 == 0 or by a term beyond 2^24;
    frame    dot_offsets, free and sasa equal those of the links call, and sasa that of rsasa_calculate_sasa_batch."""
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
ap.add_argument("--reaches", type=float, nargs="+", default=[1.5, 3.0, 6.0])
ap.add_argument("--workloads", nargs="+", default=["proteome", "real_coords"])
ap.add_argument("--structures", type=int, default=200, help="structures of the proteome in the comparison")
ap.add_argument("--full", action="store_true", help="also time the curvature call alone on the headline proteome at 3 A")
ap.add_argument("--out", default=None, help="write the JSON result here too")
args = ap.parse_args()

F = np.float32


def workload(name, n_atoms=None):
    if name == "proteome":
        return bw.synthetic_proteome(args.structures)
    import real_coords as rc
    return rc.tiled(rc.quality_set_batch(), n_atoms)


def dropped_by_definition(b, so, masks, off, loff, ent, d, reach):
    """The pairs of dot d (batch-wide) that pass d2 <= reach^2 and d2 > 0 but not t2 > 0 or the bound of 2^24, from the
    definition in numpy float32 over the dots its list names."""
    s = np.stack([np.asarray(a, F) for a in rustsasa_amd.sphere_points(args.points)], -1)
    atom = int(np.searchsorted(off, d, side="right") - 1)
    first = int(off[int(so[np.searchsorted(so, atom, side="right") - 1])])      # the structure's first dot

    def dot(g):
        i = int(np.searchsorted(off, g, side="right") - 1)
        k = np.flatnonzero(masks[i])[g - int(off[i])]
        R = F(b.radius[i]) + F(args.probe)
        return np.array([F(b.x[i]) + R * s[k, 0], F(b.y[i]) + R * s[k, 1], F(b.z[i]) + R * s[k, 2]], F), s[k]

    qa, n = dot(d)
    dropped = 0
    for e in ent[int(loff[d]):int(loff[d + 1])]:
        if e["d2"] == 0:
            continue
        qb, _ = dot(first + int(e["idx"]))
        v = qb - qa
        with np.errstate(all="ignore"):
            h = (n[0] * v[0] + n[1] * v[1]) + n[2] * v[2]
            t = v - h * n
            t2 = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
            g = h / t2
            terms = np.array([e["d2"], h, t[0] * t[0] * g, t[1] * t[1] * g, t[2] * t[2] * g, (t[0] * t[1]) * g, (t[0] * t[2]) * g,
                              (t[1] * t[2]) * g], F)
            dropped += not (t2 > 0 and (np.abs(terms) <= F(2.0 ** 24)).all())
    return dropped


def main():
    ctx = rustsasa_amd.Context(0)
    lib = _capi.load()
    result = {"tool": "bench_curvature", "probe": args.probe, "n_points": args.points, "reps": args.reps, "cases": []}
    n_atoms = None
    for wname in args.workloads:
        b = workload(wname, n_atoms)
        n_atoms = b.n_atoms if n_atoms is None else n_atoms
        x, y, z, r = (np.ascontiguousarray(a, F) for a in (b.x, b.y, b.z, b.radius))
        ids = np.ascontiguousarray(b.ids, np.uint64)
        so = np.ascontiguousarray(b.structure_offsets, np.uint32)
        S, N = len(so) - 1, b.n_atoms
        cols = (ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), S, args.probe, args.points)
        atom_sasa, _ = ctx.calculate_sasa_batch(x, y, z, r, ids, so, args.probe, args.points)
        words, _ = ctx.accessible_points_batch(x, y, z, r, ids, so, args.probe, args.points)
        masks = rustsasa_amd.unpack_points(words, args.points)
        for reach in args.reaches:
            off_c, off_l = np.zeros(N + 1, np.uint64), np.zeros(N + 1, np.uint64)
            n_links = np.zeros(1, np.uint64)
            rc = lib.rsasa_dot_links_batch(ctx._h, *cols, reach, ptr(off_l), ptr(n_links), None, 0, None, 0, None, None)
            assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL, rc
            D, E = int(off_l[-1]), int(n_links[0])
            pairs, mom = np.zeros(D, np.uint32), np.zeros((D, 8), np.int64)
            loff, ent = np.zeros(D + 1, np.uint64), np.zeros(E, rustsasa_amd.WITHIN_DTYPE)
            free_c, free_l = np.zeros(N, np.uint32), np.zeros(N, np.uint32)
            sasa_c, sasa_l = np.zeros(N, F), np.zeros(N, F)

            def timed(fn, *a):
                t0 = time.perf_counter()
                rc = fn(ctx._h, *cols, reach, *a)
                dt = (time.perf_counter() - t0) * 1e3
                _capi.check(rc, ctx._h)
                return dt

            calls = {"curvature": lambda: timed(lib.rsasa_dot_curvature_batch, ptr(off_c), ptr(pairs), ptr(mom), D, ptr(free_c),
                                                ptr(sasa_c)),
                     "links": lambda: timed(lib.rsasa_dot_links_batch, ptr(off_l), ptr(n_links), ptr(loff), D, ptr(ent), E,
                                            ptr(free_l), ptr(sasa_l))}
            for call in calls.values():
                call()
            times = {k: [] for k in calls}
            for _ in range(args.reps):
                for k, call in calls.items():
                    times[k].append(call())
            lo = loff.astype(np.int64)
            zero = np.concatenate([[0], np.cumsum(ent["d2"] == 0)])
            length = np.diff(lo) - (zero[lo[1:]] - zero[lo[:-1]])
            differ = np.flatnonzero(pairs.astype(np.int64) != length)
            pairs_ok = bool((pairs[differ] < length[differ]).all()) and len(differ) <= 10000
            if pairs_ok:
                o64 = off_l.astype(np.int64)
                pairs_ok = all(dropped_by_definition(b, so.astype(np.int64), masks, o64, lo, ent, int(d), reach) ==
                               int(length[d]) - int(pairs[d]) for d in differ)
            frame_ok = bool(np.array_equal(off_c, off_l) and np.array_equal(free_c, free_l) and
                            sasa_c.tobytes() == sasa_l.tobytes() == np.ascontiguousarray(atom_sasa, F).tobytes())
            med = {k: statistics.median(v) for k, v in times.items()}
            mean = rustsasa_amd.curvature_values(pairs, mom)[0]
            case = {"workload": wname, "structures": S, "atoms": N, "dots": D, "reach": reach, "link_entries": E,
                    "out_bytes": {"curvature": int(off_c.nbytes + pairs.nbytes + mom.nbytes),
                                  "links": int(off_l.nbytes + loff.nbytes + ent.nbytes)},
                    "ms": {k: [round(t, 2) for t in v] for k, v in times.items()},
                    "median_ms": {k: round(v, 2) for k, v in med.items()},
                    "curvature_to_links": round(med["curvature"] / med["links"], 3),
                    "pairs_equal_the_link_lists_less_d2_zero_and_the_dropped": pairs_ok,
                    "dots_with_a_dropped_pair": int(len(differ)),
                    "offsets_free_and_sasa_equal_those_of_the_other_calls": frame_ok,
                    "pairs_per_dot": round(float(pairs.mean()), 2) if D else 0.0,
                    "dots_with_positive_mean_curvature": round(float((mean > 0).mean()), 4) if D else 0.0}
            assert pairs_ok and frame_ok, case
            print(json.dumps(case), flush=True)
            result["cases"].append(case)
            del ent, loff, mom, pairs
    if args.full:
        b = bw.synthetic_proteome()
        x, y, z, r = (np.ascontiguousarray(a, F) for a in (b.x, b.y, b.z, b.radius))
        ids, so = np.ascontiguousarray(b.ids, np.uint64), np.ascontiguousarray(b.structure_offsets, np.uint32)
        N = b.n_atoms
        cols = (ptr(x), ptr(y), ptr(z), ptr(r), ptr(ids), ptr(so), len(so) - 1, args.probe, args.points, 3.0)
        off = np.zeros(N + 1, np.uint64)
        rc = lib.rsasa_dot_curvature_batch(ctx._h, *cols, ptr(off), None, None, 0, None, None)
        assert rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL, rc
        D = int(off[-1])
        pairs, mom = np.zeros(D, np.uint32), np.zeros((D, 8), np.int64)
        ms = []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            _capi.check(lib.rsasa_dot_curvature_batch(ctx._h, *cols, ptr(off), ptr(pairs), ptr(mom), D, None, None), ctx._h)
            ms.append(round((time.perf_counter() - t0) * 1e3, 2))
        result["full_proteome"] = {"structures": len(so) - 1, "atoms": N, "dots": D, "reach": 3.0, "ms_after_warm_up": ms[1:],
                                   "median_ms": round(statistics.median(ms[1:]), 2), "out_bytes": int(off.nbytes + pairs.nbytes + mom.nbytes)}
        print(json.dumps(result["full_proteome"]), flush=True)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}))


main()
