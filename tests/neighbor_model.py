"""A plain restatement of precompute_neighbors (reference src/lib.rs:69-84; SpatialGrid::new and
build_all_neighbor_lists, spatial_grid.rs:28-50, 195-465) in vectorised numpy float32, all pairs, no grid data
structure.  It shares no code with the oracle (oracle/sasa_oracle.c) or the engine (neighbors.hip), so a mistake the
two have in common shows up against it.

Atom j is in atom i's list when
  - j != i and id_j != id_i (spatial_grid.rs:314; no ids: all atoms distinct),
  - the cells of i and j are at most 2 apart along every axis (the half shell of search extent
    ceil(max_search / cell) = 2, spatial_grid.rs:47; cell coordinates ((pos - (min - cell)) * inv) as u32),
  - d^2 <= max_search^2 and d^2 <= (r_i + max_r + 2 probe)^2 (spatial_grid.rs:216-220, 307-335),
with d^2 = dx*dx + dy*dy + dz*dz in float32, not fused.  Each list is ordered by (d^2, idx), the engine's documented
order; threshold_squared = (r_j + probe)^2.  Plain helper module (not a conftest)."""
from __future__ import annotations

import numpy as np

F = np.float32
NEIGHBOR_DTYPE = np.dtype([("threshold_squared", "<f4"), ("idx", "<u4")])
CHUNK_PAIRS = 1 << 22  # pairs per block of rows


def fold_max(r) -> np.float32:
    """radii.fold(0.0, f32::max) (lib.rs:259-262): NaN radii are skipped."""
    r = np.asarray(r, F)
    r = r[~np.isnan(r)]
    return F(max(F(0.0), np.max(r, initial=F(0.0))))


def _as_u32(v: np.ndarray) -> np.ndarray:
    """Rust's saturating `f32 as u32`: NaN -> 0, below 0 -> 0, above u32::MAX -> u32::MAX."""
    v = np.asarray(v, np.float64)
    out = np.where(np.isnan(v), 0.0, np.clip(v, 0.0, 4294967295.0))
    return np.floor(out).astype(np.int64)


def grid_params(probe, max_radius):
    """(cell, 1 / cell, max_search^2) in float32 (lib.rs:76-80); ValueError where the engine reports RSASA_ERR_INVALID_ARGUMENT."""
    probe, m = F(probe), F(max_radius)
    cell = probe + m
    with np.errstate(divide="ignore", over="ignore"):
        inv = F(1.0) / cell
    if not (cell > 0 and np.isfinite(cell) and np.isfinite(inv)):
        raise ValueError("probe_radius + max_radius must be a positive finite number")
    ms = m + m + F(2.0) * probe
    with np.errstate(over="ignore"):  # (a huge max_radius: ms^2 = +inf, every pair of the block passes)
        return cell, inv, ms * ms


@np.errstate(over="ignore", invalid="ignore")
def neighbor_csr(x, y, z, r, ids=None, probe=1.4, max_radius=None, active_indices=None):
    """(offsets uint64[n + 1], entries NEIGHBOR_DTYPE) of the lists, n = len(active_indices) or all atoms.
    max_radius None or NaN: the fold maximum of the active radii.  With active_indices only those atoms are binned
    and bounded; lists are indexed by active position and idx is the original index."""
    x, y, z, r = (np.asarray(a, F) for a in (x, y, z, r))
    ids = None if ids is None else np.asarray(ids, np.uint64)
    act = np.arange(len(x), dtype=np.int64) if active_indices is None else np.asarray(active_indices, np.int64)
    x, y, z, r = x[act], y[act], z[act], r[act]
    if ids is not None:
        ids = ids[act]
    n = len(act)
    probe = F(probe)
    if max_radius is None or np.isnan(max_radius):
        max_radius = fold_max(r)
    cell, inv, ms2 = grid_params(probe, max_radius)
    m = F(max_radius)
    offsets = np.zeros(n + 1, np.uint64)
    if n == 0:
        return offsets, np.zeros(0, NEIGHBOR_DTYPE)
    # calculate_bounds (spatial_grid.rs:108-129): f32::min skips NaN
    mins = [F(np.nanmin(a) if not np.all(np.isnan(a)) else np.inf) - cell for a in (x, y, z)]
    cells = np.stack([_as_u32((a - mn) * inv) for a, mn in zip((x, y, z), mins)], axis=1)
    sr = r + m + F(2.0) * probe
    sr2 = sr * sr
    tj = r + probe
    thr = tj * tj
    rows_all, idx_all, d2_all = [], [], []
    step = max(1, CHUNK_PAIRS // n)
    for i0 in range(0, n, step):
        i1 = min(n, i0 + step)
        dx = x[i0:i1, None] - x[None, :]
        dy = y[i0:i1, None] - y[None, :]
        dz = z[i0:i1, None] - z[None, :]
        d2 = dx * dx + dy * dy + dz * dz
        assert d2.dtype == F
        ok = (d2 <= ms2) & (d2 <= sr2[i0:i1, None])
        ok &= np.all(np.abs(cells[i0:i1, None, :] - cells[None, :, :]) <= 2, axis=2)
        ok[np.arange(i1 - i0), np.arange(i0, i1)] = False
        if ids is not None:
            ok &= ids[i0:i1, None] != ids[None, :]
        ri, j = np.nonzero(ok)
        rows_all.append(ri + i0)
        idx_all.append(j)
        d2_all.append(d2[ri, j])
    rows = np.concatenate(rows_all)
    j = np.concatenate(idx_all)
    d2 = np.concatenate(d2_all)
    # (d^2 >= 0 and never NaN in a list: its bits order like the numbers, so (d^2, idx) is one 64-bit key)
    order = np.lexsort(((d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64), rows))
    rows, j = rows[order], j[order]
    offsets[1:] = np.cumsum(np.bincount(rows, minlength=n), dtype=np.uint64)
    ent = np.zeros(len(j), NEIGHBOR_DTYPE)
    ent["threshold_squared"] = thr[j]
    ent["idx"] = act[j]
    return offsets, ent
