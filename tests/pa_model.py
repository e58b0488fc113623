"""The routing of the two per-atom occlusion kernels, k_occlusion_fast (rustsasa_amd/csrc/occlusion_fast.inc) and
k_occlusion_v3 (occlusion_v3.inc), emulated in numpy: the integers that decide what code an atom runs through - NOT a
second SASA oracle (values and K always come from oracle/pyoracle.py).

For a batch (columns, structure offsets, probe, n_points, lane count W, ids or None, forced kernel and atoms per wave)
and an order of the atoms inside a cell, launch() gives per atom (input order):

  T   the swept count: atoms in the cells [x0, x1] of the 25 x-rows of the atom's 5 x 5 x 5 block, self included.  The
      prologue (prologue_runs / the v3 prologue) is restated in float32 - fx, fy, fz, the cell, tol, thr, the row gaps -
      but b2 and the square root are taken in float64: the device's raw v_sqrt_f32 and the heuristic factors are not
      imitated to the bit.  `widen` moves every cull width by that much (relative, plus as many cells) so that the CPU
      test can show that no case depends on them;
  A   accepted atoms (q != p, d^2 <= sr^2 in float32, before the id rule) and K after the id rule;
  deferred   k_occlusion_fast's rule, T > 256 or K > 144.

Launch.fast(i) and Launch.v3(i) follow one atom through its kernel for the figures that depend on the order of the
flat positions (near counts, flush sizes, windows).  The grid is tail_cases.grid_of / cell_index, pinned to the engine.
The keyword switches swept_limit, cap, flush_at and window make the model wrong in one way each; they exist only so
that the CPU test can show that a case bites.

mx_model.launch has a K_all and an `order` parameter of the same kind; they are not reused.  K_all counts over the
whole 5 x 5 x 5 block, while A and K here must count over the cells the culled rows keep - a candidate that the culling
drops has to show as a K below the oracle's - and T, the runs and the flat positions need the same cell-sorted order
with a third, random, variant.  Both models take the grid from tail_cases and are pinned to the oracle's K.
Plain helper module (not a conftest)."""
from dataclasses import dataclass

import numpy as np

import tail_cases as tc
import tie_cases as ti

F = np.float32
FAST_CAP = 144          # kFastCap
FAST_MAX_SWEPT = 256    # kFastMaxSwept
FAST_MAX_REM = 4        # kFastMaxRem
FAST_APW = 10           # kFastAtomsPerWave
CAND_PAD = 16           # kCandPad
V3_APW = 8              # kMaxAtomsPerWave
LIST_CAP = 192          # kListCap
LIST_FLUSH = 128        # kListFlush
WINDOW = 256            # flat positions per marker window
NCH = 2                 # chunks of 64 points per group
NEAR_SCALE2 = F(1.5625)  # kNearScale2
MX_MIN_ATOMS = 32768    # kMxMinAtoms
ROWS = [(r % 5 - 2, r // 5 - 2) for r in range(25)]   # lane r -> (rdy, rdz)


def cdiv(a, b):
    return -(-a // b)


def uses_fast(n_atoms, n_points, W, kernel=None):
    """launch_occlusion: k_occlusion_fast takes the batch (kernel: RSASA_OCCLUSION_KERNEL or None)."""
    kv = 6 if kernel is None else int(kernel)
    n_rem = n_points - ti.n_fused(n_points, W)
    mx = kv >= 5 and n_rem <= FAST_MAX_REM and (kv == 5 or n_atoms >= MX_MIN_ATOMS)
    return kv >= 4 and not mx and cdiv(n_points, 64) <= 2 and n_rem <= FAST_MAX_REM


def launch_apw(n_atoms, fast, forced=None):
    """launch_occlusion's atoms per wave: the forced value or n_atoms / 32 768 (one at least), capped at
    4 kFastAtomsPerWave (fast; above 10 rounded down to a multiple of 10) or kMaxAtomsPerWave (v3)."""
    apw = int(forced) if forced else max(1, n_atoms // (256 * 4 * 8 * 4))
    apw = min(apw, 4 * FAST_APW if fast else V3_APW)
    if fast and apw > FAST_APW:
        apw -= apw % FAST_APW
    return apw


def remap(bid, n_blocks):
    """The XCD remap of a workgroup's number."""
    per = n_blocks // 8
    return (bid % 8) * per + bid // 8 if bid < per * 8 else bid


def waves(n_atoms, apw, fast):
    """[(first, behind, [groups of kFastAtomsPerWave])] of every wave that has atoms, in workgroup order."""
    n_blocks = cdiv(cdiv(n_atoms, apw), 4)
    out = []
    for blk in range(n_blocks):
        for w in range(4):
            b = (remap(blk, n_blocks) * 4 + w) * apw
            if b < n_atoms:
                e = min(b + apw, n_atoms)
                step = FAST_APW if fast else apw
                out.append((b, e, [(g, min(g + step, e)) for g in range(b, e, step)]))
    return out


def list_trips(n_atoms, n_deferred, hint=None):
    """(workgroups, grid-stride trips of the busiest wave) of the list-mode launch of k_occlusion_v3 (one atom per
    wave) for a deferred_hint (None: unknown)."""
    want = 1024 if hint is None else min(1024, max(16, cdiv(hint, 2)))
    n_blocks = min(cdiv(n_atoms, 4), want)
    return n_blocks, cdiv(n_deferred, n_blocks * 4) if n_blocks else 0


def rem_tiling(n_rem):
    """(rem_shift, rem_groups) of k_occlusion_v3's remainder points."""
    s = 0
    while (1 << s) < n_rem:
        s += 1
    s = max(s, 2)
    return s, 64 >> s


@dataclass
class Launch:
    n: int
    n_points: int
    W: int
    fast_kernel: bool
    apw: int
    n_blocks: int
    per: int
    order: np.ndarray      # cell-sorted position -> input index
    pos: np.ndarray        # input index -> cell-sorted position
    sid: np.ndarray        # input index -> structure
    cxyz: np.ndarray       # input index -> cell (x, y, z)
    x0: np.ndarray         # [n, 25] first swept cell of every row, -1 where the row is dropped
    x1: np.ndarray
    run_start: np.ndarray  # [n, 25] cell-sorted position of the run's first atom
    run_len: np.ndarray    # [n, 25]
    T: np.ndarray
    A: np.ndarray
    K: np.ndarray
    deferred: np.ndarray   # bool (k_occlusion_fast's rule, whatever kernel runs)
    cols: tuple
    ids: np.ndarray
    probe: np.float32
    max_r: np.ndarray      # per structure
    sw: dict

    @property
    def n_deferred(self):
        return int(self.deferred.sum()) if self.fast_kernel else 0

    @property
    def n_fused(self):
        return ti.n_fused(self.n_points, self.W)

    def swept_cells(self, i):
        """The (row, x0, x1) of the rows atom i sweeps."""
        return [(r, int(self.x0[i, r]), int(self.x1[i, r])) for r in range(25) if self.x0[i, r] >= 0]

    def runs(self, i):
        """The non-empty runs of atom i: (row, first flat position, length)."""
        out, f = [], 0
        for r in range(25):
            if self.run_len[i, r]:
                out.append((r, f, int(self.run_len[i, r])))
                f += int(self.run_len[i, r])
        return out

    def flat(self, i):
        """Input indices of the atoms at atom i's flat positions 0 .. T - 1."""
        parts = [self.order[self.run_start[i, r]:self.run_start[i, r] + self.run_len[i, r]] for r in range(25)
                 if self.run_len[i, r]]
        return np.concatenate(parts) if parts else np.zeros(0, np.int64)

    def _tests(self, i, q):
        """(d^2 <= sr^2 and q != i, other id, near) of atoms q for atom i, in the kernels' float32 expressions."""
        x, y, z, r = self.cols
        sr = r[i] + self.max_r[self.sid[i]] + F(2.0) * self.probe
        dx, dy, dz = x[i] - x[q], y[i] - y[q], z[i] - z[q]
        d2 = dx * dx + dy * dy + dz * dz
        Rr = r[i] + self.probe
        acc = (d2 <= sr * sr) & (q != i)
        other = np.ones(len(q), bool) if self.ids is None else self.ids[q] != self.ids[i]
        return acc, other, d2 < NEAR_SCALE2 * (Rr * Rr)

    def fast(self, i):
        """Atom i in k_occlusion_fast: the sweep's trips, the list, prep's passes and phase A / B's sizes."""
        T, K = int(self.T[i]), int(self.K[i])
        out = dict(T=T, K=K, A=int(self.A[i]), deferred=bool(self.deferred[i]), HALF1=self.n_fused <= 96,
                   n_rem=self.n_points - self.n_fused,
                   trips=[(s, s + 64 < T) for s in range(0, T, 128)])
        if out["deferred"]:
            return out
        q = self.flat(i)
        acc, other, near = self._tests(i, q)
        lst = (acc & other)
        first = np.flatnonzero(lst)[:64]
        nA = int(near[first].sum())
        nA4 = min(K, (nA + 3) & ~3)
        # phase A tests the slots below nA4 of the list as prep leaves it: the first pass's near ones, then its far ones
        cand = q[np.flatnonzero(lst)]
        head = np.concatenate([first[near[first]], first[~near[first]]])
        alive = self._survivors(i, q[head[:nA4]])
        S = int(alive.sum())
        nB = K - nA4
        form = "none" if S == 0 or nB == 0 else "tiles" if S <= 64 else "broadcast"
        G = 64 >> (3 if S <= 8 else 4 if S <= 16 else 5 if S <= 32 else 6)
        out.update(passes=cdiv(K, 64), nA=nA, nA4=nA4, nB=nB, pad=(K, K + CAND_PAD), S=S, form=form,
                   G=G if form == "tiles" else None, steps=cdiv(nB, G) if form == "tiles" else None, n_cand=len(cand),
                   S_second=int(alive[64:].sum()))
        return out

    def _survivors(self, i, cands):
        """Fused-rule points of atom i that none of the atoms `cands` occludes (lib.rs:129-146 in float32, the dot product
        fused): what phase A leaves to phase B - the one place where the model looks at points, because the tiling of
        phase B depends on their number."""
        x, y, z, r = self.cols
        sx, sy, sz = ti.sphere(self.n_points)
        nf = self.n_fused
        occ = np.zeros(nf, bool)
        Rr = r[i] + self.probe
        for j in cands:
            vx, vy, vz = x[i] - x[j], y[i] - y[j], z[i] - z[j]
            d2 = vx * vx + vy * vy + vz * vz
            tj = r[j] + self.probe
            limit = (tj * tj - d2 - Rr * Rr) / (F(2.0) * Rr)
            occ |= ti.fmaf_vec(sx[:nf], vx, ti.fmaf_vec(sy[:nf], vy, sz[:nf] * vz)) < limit
        return ~occ

    def v3(self, i):
        """Atom i in k_occlusion_v3: the flushes of one sweep (sizes, and the flat position each one falls at), the
        windows visited with the runs that start in each and the run that straddles its start, the chunk groups and
        whether each sweeps again, the remainder tiling and the id rule's hit in the first prep pass."""
        flush_at, window = self.sw["flush_at"], self.sw["window"]
        T = int(self.T[i])
        q = self.flat(i)
        acc, other, _ = self._tests(i, q)
        a = np.concatenate([acc, np.zeros(64, bool)])
        o = np.concatenate([other, np.ones(64, bool)])
        flushes, at, id_hit = [], [], False
        seg, n_list, taken = 0, 0, []
        while seg < T:
            round_end = min(T, (seg // window) * window + window)
            while seg < round_end and n_list <= flush_at:
                taken += (np.flatnonzero(a[seg:seg + 64]) + seg).tolist()
                n_list = len(taken)
                seg += 64
            if n_list <= flush_at and seg < T:
                continue
            if not flushes:
                id_hit = bool((~o[taken[:64]]).any())
            flushes.append(n_list)
            at.append(min(seg, T))
            n_list, taken = 0, []
        runs = self.runs(i)
        wins = []
        for w in range(cdiv(T, window)):
            lo = w * window
            starts = [r for r, f, n in runs if lo <= f < lo + window]
            straddle = [r for r, f, n in runs if f < lo < f + n]
            wins.append((w, starts, straddle[0] if straddle else None))
        n_chunks = cdiv(self.n_points, 64)
        n_groups = cdiv(n_chunks, NCH)
        single = len(flushes) == 1
        n_rem = self.n_points - self.n_fused
        shift, groups = rem_tiling(n_rem)
        return dict(T=T, A=int(self.A[i]), K=int(self.K[i]), flushes=flushes, flush_at=at, single_flush=single,
                    windows=wins, n_groups=n_groups, sweeps=1 if single else n_groups, n_rem=n_rem, rem_shift=shift,
                    rem_groups=groups, id_hit_first_pass=id_hit)


def launch(x, y, z, r, so, probe, n_points, W, ids=None, kernel=None, apw=None, order="asc", seed=0, widen=0.0,
           swept_limit=FAST_MAX_SWEPT, cap=FAST_CAP, flush_at=LIST_FLUSH, window=WINDOW):
    """The model of one launch.  order: the atoms of a cell by rising ("asc") or falling ("desc") input index, or in a
    seeded random order ("random").  widen: every cull width (wx, and the row test's b2) moved by this much - relative
    plus as many cells; negative narrows.  The last four keywords are the switches."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    so = np.asarray(so, np.int64)
    N = len(x)
    probe = F(probe)
    ids = None if ids is None else np.asarray(ids, np.uint64)
    fast = uses_fast(N, n_points, W, kernel)
    a_pw = launch_apw(N, fast, apw)
    order_l, max_rs = [], []
    sid = np.zeros(N, np.int64)
    cxyz = np.zeros((N, 3), np.int64)
    x0 = np.full((N, 25), -1, np.int64)
    x1 = np.full((N, 25), -1, np.int64)
    run_start = np.zeros((N, 25), np.int64)
    run_len = np.zeros((N, 25), np.int64)
    T = np.zeros(N, np.int64)
    A = np.zeros(N, np.int64)
    K = np.zeros(N, np.int64)
    rng = np.random.default_rng(seed)
    base = 0
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        n = e - b
        max_rs.append(F(np.max(r[b:e], initial=F(0.0))))
        if n == 0:
            continue
        sx, sy, sz, srr = x[b:e], y[b:e], z[b:e], r[b:e]
        mn, inv, dims = tc.grid_of(sx, sy, sz, srr, probe)
        dims = np.asarray(dims, np.int64)
        f = [(a - mn[k]) * inv for k, a in enumerate((sx, sy, sz))]            # float32: spatial_grid.rs:139-141
        c = [np.minimum(np.maximum(f[k], F(0.0)).astype(np.int64), dims[k] - 1) for k in range(3)]
        idx = c[0] + c[1] * dims[0] + c[2] * dims[0] * dims[1]
        assert np.array_equal(idx, tc.cell_index(sx, sy, sz, mn, inv, dims))
        key = {"asc": np.arange(n), "desc": -np.arange(n), "random": rng.permutation(n)}[order]
        o = np.lexsort((key, idx))
        n_cells = int(np.prod(dims))
        starts = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n_cells))]).astype(np.int64)
        sid[b:e] = s
        cxyz[b:e] = np.stack(c, -1)
        order_l.append(b + o)
        # the prologue: tol, sr, thr in float32; the gaps in float32; b2 and wx in float64
        tol = F(8.0) * F(1.1920929e-7) * F(dims.max()) + F(1e-5)
        sr = srr + max_rs[-1] + F(2.0) * probe
        srn = sr * inv
        thr = srn * srn * F(1.00001)
        uy, uz = f[1] - c[1].astype(F), f[2] - c[2].astype(F)
        for row, (rdy, rdz) in enumerate(ROWS):
            gy = F(rdy) - uy if rdy > 0 else (uy - F(rdy + 1) if rdy < 0 else np.zeros(n, F))
            gz = F(rdz) - uz if rdz > 0 else (uz - F(rdz + 1) if rdz < 0 else np.zeros(n, F))
            gy, gz = np.maximum(gy - tol, F(0.0)), np.maximum(gz - tol, F(0.0))
            b2 = thr.astype(np.float64) - gy.astype(np.float64) ** 2 - gz.astype(np.float64) ** 2
            b2 = b2 + widen * (thr.astype(np.float64) + 1.0)
            yy, zz = c[1] + rdy, c[2] + rdz
            ok = (yy >= 0) & (yy < dims[1]) & (zz >= 0) & (zz < dims[2]) & (b2 >= 0.0)
            wx = np.sqrt(np.maximum(b2, 0.0)) * 1.0001 * (1.0 + widen) + float(tol) + widen
            fx = f[0].astype(np.float64)
            lo = np.maximum(np.maximum(np.floor(fx - wx).astype(np.int64), c[0] - 2), 0)
            hi = np.minimum(np.minimum(np.floor(fx + wx).astype(np.int64), c[0] + 2), dims[0] - 1)
            ok &= hi >= lo
            c0 = np.where(ok, lo + yy * dims[0] + zz * dims[0] * dims[1], 0)
            first = starts[c0]
            length = np.where(ok, starts[np.where(ok, c0 + (hi - lo) + 1, 0)] - first, 0)
            x0[b:e, row] = np.where(ok, lo, -1)
            x1[b:e, row] = np.where(ok, hi, -1)
            run_start[b:e, row] = np.where(ok, base + first, 0)
            run_len[b:e, row] = length
        T[b:e] = run_len[b:e].sum(1)
        # accepted atoms among the swept ones: the pair tests of the whole structure at once
        dx, dy, dz = sx[:, None] - sx[None, :], sy[:, None] - sy[None, :], sz[:, None] - sz[None, :]
        d2 = dx * dx + dy * dy + dz * dz                                          # float32: spatial_grid.rs:321
        acc = (d2 <= (sr * sr)[:, None]) & ~np.eye(n, dtype=bool)
        ry, rz = c[1][None, :] - c[1][:, None], c[2][None, :] - c[2][:, None]
        inblock = (np.abs(ry) <= 2) & (np.abs(rz) <= 2)
        row_of = np.where(inblock, (rz + 2) * 5 + (ry + 2), 0)
        lo_ij = np.take_along_axis(x0[b:e], row_of, 1)
        hi_ij = np.take_along_axis(x1[b:e], row_of, 1)
        swept = inblock & (lo_ij >= 0) & (c[0][None, :] >= lo_ij) & (c[0][None, :] <= hi_ij)
        assert np.array_equal(swept.sum(1), T[b:e])
        A[b:e] = (swept & acc).sum(1)
        other = np.ones((n, n), bool) if ids is None else ids[b:e][:, None] != ids[b:e][None, :]
        K[b:e] = (swept & acc & other).sum(1)
        base += n
    order_a = np.concatenate(order_l) if order_l else np.zeros(0, np.int64)
    pos = np.empty(N, np.int64)
    pos[order_a] = np.arange(N)
    n_blocks = cdiv(cdiv(N, a_pw), 4) if N else 0
    return Launch(N, n_points, W, fast, a_pw, n_blocks, n_blocks // 8, order_a, pos, sid, cxyz, x0, x1, run_start,
                  run_len, T, A, K, (T > swept_limit) | (K > cap), (x, y, z, r), ids, probe, np.array(max_rs, F),
                  dict(flush_at=flush_at, window=window))
