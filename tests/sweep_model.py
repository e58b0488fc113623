"""The Chebyshev shell sweep of k_atom_depth (depth.hip) and k_component_link (components.hip), emulated in numpy: what
one wave does for one atom of one structure, step by step - NOT a second brute force.  The grid is tail_cases.grid_of /
depth_cases.grid_cells (pinned to the engine), the cell order a stable sort by cell index; the shells, their rows, the
rim rows' x-runs and the inside rows' two cells, the 64-row steps and the 64-atom staging batches are built as the
kernels build them; the stop rule, the margins test and the components reach are evaluated in float32 as written there.

The key held after a shell is the minimum of pair_keys()[i, seen]: depth_model.keys_of's expression (the header's
definition, numpy float32, nothing fused) reduced per owner atom instead of over all dots at once, so that a sweep costs
a table look-up per shell.  A minimum over a union is the minimum of the minima: the held key is keys_of restricted to
the atoms seen so far, bit for bit (test_sweep_cpu.py pins pair_keys().min(axis=1) == keys_of for every case).

The keyword switches exist only so that the CPU tests can show that a case bites; each is one way a kernel could be
wrong.  Plain helper module (not a conftest)."""
from dataclasses import dataclass

import numpy as np

import depth_cases as dc
import depth_model as dm
import tail_cases as tc

F = np.float32
NONE_KEY = dm.NONE_KEY
WAVE = 64          # kWave: rows per step, atoms per staging batch
_PAIRS = 1 << 22   # (target, dot) pairs evaluated at once


# ---- the margins -------------------------------------------------------------------------------------------------------

def odd_input(x, y, z, r):
    """StructGrid::odd_radii bit 0 as k_bounds sets it: a radius outside [0, 64] or NaN, a coordinate beyond 1e8 or
    non-finite."""
    x, y, z, r = (np.asarray(a, F) for a in (x, y, z, r))
    with np.errstate(invalid="ignore"):
        big = ~(np.fmax(np.fmax(np.abs(x), np.abs(y)), np.abs(z)) <= F(1e8))
        return bool((~((r >= F(0.0)) & (r <= F(64.0)))).any() or big.any() or np.isnan(x).any() or np.isnan(y).any()
                    or np.isnan(z).any())


def margin_sums(x, y, z, r, probe):
    """(float32[3], float32): fabsf(min) + (float)dim * h per axis and 65536 h, as sh_margins_hold forms them."""
    mn, _, dims = tc.grid_of(x, y, z, r, probe)
    h = F(probe) + np.max(r)
    a = np.array([np.abs(mn[k]) + F(dims[k]) * h for k in range(3)], F)
    return a, F(65536.0) * h


def margins_hold(x, y, z, r, probe):
    """sh_margins_hold (shell_sweep.h) restated in float32 for one structure (not empty)."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    if odd_input(x, y, z, r):
        return False
    h = F(probe) + np.max(r)
    a, limit = margin_sums(x, y, z, r, probe)
    with np.errstate(invalid="ignore"):
        return bool(F(probe) >= F(0.0) and h > F(0.0) and np.fmax(a[0], np.fmax(a[1], a[2])) <= limit)


# ---- the grid of one structure -----------------------------------------------------------------------------------------

@dataclass
class Grid:
    h: np.float32
    dims: np.ndarray     # int64[3]
    cells: np.ndarray    # int64[N, 3]: cell coordinates, input order
    order: np.ndarray    # int64[N]: cell-sorted position -> input index
    pos: np.ndarray      # int64[N]: input index -> cell-sorted position
    starts: np.ndarray   # int64[n_cells + 1]: first cell-sorted position of every cell

    def s_last(self, i):
        c = self.cells[i]
        return int(max(np.maximum(c, self.dims - 1 - c)))


def grid(x, y, z, r, probe):
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    h, dims, cells = dc.grid_cells(x, y, z, r, probe)
    mn, inv, _ = tc.grid_of(x, y, z, r, probe)
    idx = tc.cell_index(x, y, z, mn, inv, dims)
    assert np.array_equal(idx, cells[:, 0] + cells[:, 1] * dims[0] + cells[:, 2] * dims[0] * dims[1])
    order = np.argsort(idx, kind="stable")
    pos = np.empty_like(order)
    pos[order] = np.arange(len(order))
    n_cells = int(dims[0] * dims[1] * dims[2])
    starts = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n_cells))]).astype(np.int64)
    return Grid(h, np.asarray(dims, np.int64), cells, order, pos, starts)


def shell_steps(g, i, s, drop_lo=False, drop_hi=False, rows_first_step_only=False, atoms_first_step_only=False):
    """The cell-sorted positions that the wave of atom i reads in shell s, one array per 64-row step, in the order of
    the concatenated runs (lane l: row r0 + l; run a, then run b).  Returns (steps, longest run)."""
    cx, cy, cz = (int(v) for v in g.cells[i])
    dx, dy, dz = (int(v) for v in g.dims)
    y0, y1 = max(cy - s, 0), min(cy + s, dy - 1)
    z0, z1 = max(cz - s, 0), min(cz + s, dz - 1)
    ny = y1 - y0 + 1
    n_rows = ny * (z1 - z0 + 1)
    x0, x1 = max(cx - s, 0), min(cx + s, dx - 1)
    has_lo, has_hi = cx >= s, cx + s <= dx - 1
    rr = np.arange(n_rows, dtype=np.int64)
    yy, zz = y0 + rr % ny, z0 + rr // ny
    rim = np.maximum(np.abs(yy - cy), np.abs(zz - cz)) == s
    c_row = yy * dx + zz * dx * dy
    st = g.starts
    start_a, len_a = np.zeros(n_rows, np.int64), np.zeros(n_rows, np.int64)
    start_b, len_b = np.zeros(n_rows, np.int64), np.zeros(n_rows, np.int64)
    start_a[rim] = st[c_row[rim] + x0]
    len_a[rim] = st[c_row[rim] + x1 + 1] - st[c_row[rim] + x0]
    ins = ~rim
    if has_lo and not drop_lo:
        start_a[ins] = st[c_row[ins] + cx - s]
        len_a[ins] = st[c_row[ins] + cx - s + 1] - st[c_row[ins] + cx - s]
    if has_hi and not drop_hi:
        start_b[ins] = st[c_row[ins] + cx + s]
        len_b[ins] = st[c_row[ins] + cx + s + 1] - st[c_row[ins] + cx + s]
    steps = []
    for r0 in range(0, n_rows, WAVE):
        if rows_first_step_only and r0:
            break
        sl = slice(r0, min(r0 + WAVE, n_rows))
        run_start = np.stack([start_a[sl], start_b[sl]], -1).ravel()
        run_len = np.stack([len_a[sl], len_b[sl]], -1).ravel()
        excl = np.cumsum(run_len) - run_len
        total = int(run_len.sum())
        flat = np.repeat(run_start - excl, run_len) + np.arange(total)      # sh_pos of f = 0 .. total - 1
        if atoms_first_step_only:
            flat = flat[:WAVE]
        steps.append(flat)
    longest = int(max(len_a.max(initial=0), len_b.max(initial=0)))
    return steps, longest


# ---- keys ----------------------------------------------------------------------------------------------------------------

def pair_keys(x, y, z, r, mask, probe, n_points):
    """uint64[N, N]: entry (i, j) is the smallest key (bits(d2) << 32) | j of target i over the accessible dots of atom
    j alone, NONE_KEY where j has no dot whose d2 is no NaN - depth_model.keys_of's arithmetic, reduced per owner."""
    x, y, z = (np.ascontiguousarray(a, F) for a in (x, y, z))
    n = len(x)
    out = np.full((n, n), NONE_KEY, np.uint64)
    owner, qx, qy, qz = dm.dots_of(x, y, z, r, mask, probe, n_points)
    if len(owner) == 0:
        return out
    has, first = np.unique(owner, return_index=True)      # the dots are sorted by owner
    low = owner.astype(np.uint64)
    step = max(1, _PAIRS // len(owner))
    for a in range(0, n, step):
        t = slice(a, min(a + step, n))
        with np.errstate(invalid="ignore", over="ignore"):
            ddx, ddy, ddz = x[t, None] - qx[None, :], y[t, None] - qy[None, :], z[t, None] - qz[None, :]
            d2 = ddx * ddx + ddy * ddy + ddz * ddz
        assert d2.dtype == F
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low[None, :]
        key[np.isnan(d2)] = NONE_KEY
        out[t, has] = np.minimum.reduceat(key, first, axis=1)
    return out


# ---- the depth sweep -------------------------------------------------------------------------------------------------

@dataclass
class Sweep:
    """What sweep_depth returns per target atom.  The winner's place in the sweep - shell, rim / inside-low / inside-high,
    the faces the shell is clipped at - is position_class(grid, i, keys[i] & 0xFFFFFFFF); `found` is the shell the sweep
    itself met it in, which test_sweep_cpu.py requires to be that class's shell."""
    keys: np.ndarray      # uint64[N]
    stop: np.ndarray      # int64[N]: the shell the sweep stopped after
    by_rule: np.ndarray   # bool[N]: stopped by the stop rule (else: the shells covered the grid)
    found: np.ndarray     # int64[N]: the shell in which the held key was found, -1 without one
    longest_run: int      # atoms of the longest x-run any sweep read


def position_class(g, i, j):
    """Where atom j's cell lies in the sweep of atom i: (shell, kind, faces) - kind "rim" (a row on the rim of the
    shell's square: part of an x-run), "inside-low" / "inside-high" (the cell cx - s / cx + s of a row inside it); faces:
    the grid faces the shell is clipped at, as a sorted tuple of "x-", "x+", "y-", ..."""
    d = g.cells[j] - g.cells[i]
    s = int(np.abs(d).max())
    kind = "rim" if max(abs(int(d[1])), abs(int(d[2]))) == s else ("inside-low" if d[0] < 0 else "inside-high")
    c = g.cells[i]
    faces = [n + "-" for k, n in enumerate("xyz") if c[k] - s < 0] + [n + "+" for k, n in enumerate("xyz") if c[k] + s > g.dims[k] - 1]
    return s, kind, tuple(sorted(faces))


def sweep_depth(x, y, z, r, mask, probe, n_points, stop_shift=2, sample=None, margins=None, **switches):
    """The sweeps of the atoms `sample` (None: all) of ONE structure.  margins None: margins_hold of the structure."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    g = grid(x, y, z, r, probe)
    K = pair_keys(x, y, z, r, mask, probe, n_points)
    if margins is None:
        margins = margins_hold(x, y, z, r, probe)
    tgt = np.arange(len(x)) if sample is None else np.asarray(sample, np.int64)
    out = Sweep(np.full(len(tgt), NONE_KEY, np.uint64), np.zeros(len(tgt), np.int64), np.zeros(len(tgt), bool),
                np.full(len(tgt), -1, np.int64), 0)
    for n, i in enumerate(tgt):
        s_last = g.s_last(i)
        best, s = NONE_KEY, 0
        while True:
            steps, longest = shell_steps(g, i, s, **switches)
            out.longest_run = max(out.longest_run, longest)
            for flat in steps:
                if len(flat):
                    m = K[i, g.order[flat]].min()
                    if m < best:
                        best, out.found[n] = m, s
            if s >= s_last:               # the shells cover the grid
                break
            if margins and s >= max(stop_shift, 0) and best != NONE_KEY:
                lim = F(s - stop_shift) * g.h
                if np.uint32(best >> np.uint64(32)).view(F) <= lim * lim:
                    out.by_rule[n] = True
                    break
            s += 1
        out.keys[n], out.stop[n] = best, s
    return out, g


# ---- the components reach ------------------------------------------------------------------------------------------------

def s_end_of(link, h, s_last, margins, reach_shift=0):
    """The last shell k_component_link sweeps, computed as there (float32 t, ceilf, the correcting while)."""
    s_end = s_last
    if margins:
        t = F(link) / F(h) + F(2.5)
        if t < F(s_last):
            S = int(np.ceil(t))
            while (F(S) - F(2.5)) * F(h) < F(link):
                S += 1
            s_end = min(S, s_last)
    return max(s_end + reach_shift, 0)


def reach_pairs(x, y, z, r, probe, link, reach_shift=0, margins=None, **switches):
    """(set of (i, j), s_end int64[N], grid): the atom pairs (input indices) that the wave of atom i takes - j at or
    before i in the cell order, within s_end(i) shells, i itself included - for every atom i of ONE structure."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    g = grid(x, y, z, r, probe)
    if margins is None:
        margins = margins_hold(x, y, z, r, probe)
    pairs, ends = set(), np.zeros(len(x), np.int64)
    for i in range(len(x)):
        ends[i] = s_end_of(link, g.h, g.s_last(i), margins, reach_shift)
        p = g.pos[i]
        for s in range(int(ends[i]) + 1):
            for flat in shell_steps(g, i, s, **switches)[0]:
                for q in flat[flat <= p]:
                    pairs.add((i, int(g.order[q])))
    return pairs, ends, g


def edge_atom_pairs(g, edges, owner):
    """The model's edges (dot numbers) as the atom pairs (later in the cell order, the other) that must take them."""
    a, b = owner[edges[:, 0]], owner[edges[:, 1]]
    swap = g.pos[a] < g.pos[b]
    i, j = np.where(swap, b, a), np.where(swap, a, b)
    return set(zip(i.tolist(), j.tolist()))
