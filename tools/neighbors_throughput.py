#!/usr/bin/env python3
"""Wall time of rsasa_precompute_neighbors_batch (host buffers in, CSR lists out) on a shard of the synthetic
proteome; prints one JSON line.  Default: a 1/8 shard (about 1.5 M atoms, 0.5 GB of entries); --shard 1 is the
whole proteome (about 4.1 GB of host output).  Kernel times come from a separate run of this tool under
`rocprofv3 --kernel-trace --stats -- python tools/neighbors_throughput.py` (k_neighbor_count, k_neighbor_fill)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench_workloads as bw  # noqa: E402
import rustsasa_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shard", type=int, default=8, help="take structures 0, k, 2k, ... of the proteome")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--probe", type=float, default=1.4)
args = ap.parse_args()

b = bw.synthetic_proteome()
if args.shard > 1:
    b = bw.shard(b, 0, args.shard)
with rustsasa_amd.Context(0) as ctx:
    offsets, entries = ctx.precompute_neighbors_batch(b.x, b.y, b.z, b.radius, b.ids, b.structure_offsets,
                                                      args.probe)  # (warm-up, and sizes the output)
    total = int(offsets[-1])
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        offsets, entries = ctx.precompute_neighbors_batch(b.x, b.y, b.z, b.radius, b.ids, b.structure_offsets,
                                                          args.probe)
        times.append((time.perf_counter() - t0) * 1e3)
print(json.dumps({"tool": "neighbors_throughput", "shard": args.shard, "structures": b.n_structures,
                  "atoms": b.n_atoms, "entries": total, "entry_bytes": total * 8,
                  "max_list": int(np.max(np.diff(offsets.astype(np.int64)))) if b.n_atoms else 0,
                  "wall_ms": [round(t, 2) for t in times], "wall_ms_min": round(min(times), 2)}))
