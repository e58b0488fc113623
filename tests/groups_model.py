"""An exact CPU model of the group contacts (rsasa_group_contacts*): for each atom the hit matrix [K, n_points] of its
neighbour list against the lattice - the float32 expressions of contacts_model.py (tie_cases.fmaf_vec, oracle lists) -
and the unions the header defines over the entries of one label: self (the atom's own label), cov_h per foreign label
h; self_free = #!self, free = #(nothing hits), buried_h = #(cov_h & !self), only_h = #(cov_h & !self & no other
foreign label).  Rows per atom in ascending unsigned label order.  No tolerance anywhere.

The three oracle checks (alone_check, pair_check, deletion_check) tie the counts to whole runs of the oracle on
sub-structures; they are exact by construction only when the sub-structure's fold-max radius equals the whole
structure's (the candidate rule depends on it), so each returns how many cases it compared and how many it skipped.
Plain helper module (not a conftest)."""
import numpy as np

import nb_helpers as nh
import structio as sio
import tie_cases as tc
from oracle import pyoracle as po

F = np.float32
_BLOCK = 1 << 22  # entries x points evaluated at once (float64 temporaries of fmaf_vec: 32 MiB each)


def _labels(groups, n):
    g = np.ascontiguousarray(groups, dtype=np.uint32)
    assert g.shape == (n,)
    return g


def group_counts(x, y, z, r, ids, groups, probe, n_points, W, lists=None):
    """(offsets uint64[n + 1], partner uint32[rows], buried uint32[rows], only uint32[rows], self_free uint32[n],
    free uint32[n]) of one structure at lane count W.  `lists` (offsets, entries) defaults to the oracle's lists of
    calculate_sasa_internal; their order does not matter."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    n = len(x)
    g = _labels(groups, n)
    offs, ent = nh.oracle_csr(x, y, z, r, ids, probe) if lists is None else lists
    o = offs.astype(np.int64)
    sx, sy, sz = po.sphere_points(n_points)
    nf = tc.n_fused(n_points, W)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(o))
    j = ent["idx"].astype(np.int64)
    lab = g[j]
    probe = F(probe)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):   # (R = 0: a limit of +-inf or NaN, as on the GPU)
        vx, vy, vz = x[rows] - x[j], y[rows] - y[j], z[rows] - z[j]
        d2 = vx * vx + vy * vy + vz * vz
        R = r[rows] + probe
        R2 = R * R
        limit = (ent["threshold_squared"].astype(F) - d2 - R2) / (F(2.0) * R)
    assert limit.dtype == F
    self_free = np.full(n, n_points, np.uint32)
    free = np.full(n, n_points, np.uint32)
    n_rows = np.zeros(n, np.int64)
    partner, buried, only = [], [], []
    step = max(1, _BLOCK // max(n_points, 1))
    a = 0
    while a < n:
        # whole atoms, about `step` entries
        b = int(np.searchsorted(o, o[a] + step, side="right")) - 1
        b = min(max(b, a + 1), n)
        e0, e1 = int(o[a]), int(o[b])
        if e1 > e0:
            cv = [t[e0:e1, None] for t in (vx, vy, vz, limit)]
            parts = []
            with np.errstate(invalid="ignore", over="ignore"):
                if nf:
                    f = slice(0, nf)
                    dot = tc.fmaf_vec(sx[None, f], cv[0], tc.fmaf_vec(sy[None, f], cv[1], sz[None, f] * cv[2]))
                    parts.append(dot < cv[3])
                if nf < n_points:
                    u = slice(nf, n_points)
                    dot = sx[None, u] * cv[0] + sy[None, u] * cv[1] + sz[None, u] * cv[2]
                    assert dot.dtype == F
                    parts.append(dot <= cv[3])
            hit = np.concatenate(parts, axis=1) if len(parts) > 1 else parts[0]
            # the entries by (atom, label): one segment per label of an atom's list, its union of hits
            rw, lb = rows[e0:e1] - a, lab[e0:e1]
            order = np.lexsort((lb, rw))
            rw, lb, hit = rw[order], lb[order], hit[order]
            head = np.ones(len(rw), bool)
            head[1:] = (rw[1:] != rw[:-1]) | (lb[1:] != lb[:-1])
            starts = np.nonzero(head)[0]
            cov = np.logical_or.reduceat(hit, starts, axis=0)
            s_row, s_lab = rw[starts], lb[starts]
            own = s_lab == g[a + s_row]
            self_ = np.zeros((b - a, n_points), bool)
            self_[s_row[own]] = cov[own]            # (at most one own-label segment per atom)
            f_row, f_lab = s_row[~own], s_lab[~own]
            f_cov = cov[~own] & ~self_[f_row]
            n_groups = np.zeros((b - a, n_points), np.int32)   # foreign labels hitting each point self leaves free
            np.add.at(n_groups, f_row, f_cov.astype(np.int32))
            partner.append(f_lab)
            buried.append(f_cov.sum(axis=1))
            only.append((f_cov & (n_groups[f_row] == 1)).sum(axis=1))
            self_free[a:b] = n_points - self_.sum(axis=1)
            free[a:b] = n_points - (self_ | (n_groups > 0)).sum(axis=1)
            n_rows[a:b] = np.bincount(f_row, minlength=b - a)
        a = b
    out_offs = np.zeros(n + 1, np.uint64)
    out_offs[1:] = np.cumsum(n_rows)
    cat = lambda parts: np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)  # noqa: E731
    return out_offs, cat(partner), cat(buried), cat(only), self_free, free


def group_counts_batch(x, y, z, r, ids, groups, so, probe, n_points, W):
    """group_counts of every structure of a batch (one grid and one max radius each; labels are compared within a
    structure only), offsets batch-global."""
    groups = _labels(groups, len(x))
    offs, cols, per_atom, base = [np.zeros(1, np.uint64)], [[], [], []], [[], []], 0
    for s in range(len(so) - 1):
        b, e = int(so[s]), int(so[s + 1])
        if e == b:
            continue
        m = group_counts(x[b:e], y[b:e], z[b:e], r[b:e], None if ids is None else ids[b:e], groups[b:e], probe,
                         n_points, W)
        offs.append(m[0][1:] + np.uint64(base))
        base += int(m[0][-1])
        for k in range(3):
            cols[k].append(m[1 + k])
        per_atom[0].append(m[4])
        per_atom[1].append(m[5])
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint32)  # noqa: E731
    return (np.concatenate(offs),) + tuple(cat(c) for c in cols) + tuple(cat(c) for c in per_atom)


def rows_of(offs):
    """The atom of every row."""
    return np.repeat(np.arange(len(offs) - 1, dtype=np.int64), np.diff(offs.astype(np.int64)))


def row_lookup(model, h):
    """(buried_h int64[n], only_h int64[n]): each atom's row for label h, 0 where it has none."""
    offs, partner, buried, only = model[:4]
    n = len(offs) - 1
    atom = rows_of(offs)
    m = partner == np.uint32(h)
    bur, onl = np.zeros(n, np.int64), np.zeros(n, np.int64)
    bur[atom[m]] = buried[m]
    onl[atom[m]] = only[m]
    return bur, onl


# ---- fixtures with chain and residue labels ---------------------------------------------------------------------

def labelled_fixture(name):
    """(columns, chain uint32[n], residue uint32[n], chain names) of a structure file: its ATOM records with the vdW
    radii of structio (HETATM records go: waters and ions share their chain's letter).  Chains are numbered in order
    of first appearance, residues by (chain, number, insertion code) likewise."""
    atoms = [a for a in sio.read_structure(sio.data_path(name)) if not a.hetero and a.element in sio.VDW]
    cols = sio.soa_vdw(atoms)
    chains, residues = {}, {}
    chain = np.array([chains.setdefault(a.chain, len(chains)) for a in atoms], np.uint32)
    residue = np.array([residues.setdefault((a.chain, a.resseq, a.icode), len(residues)) for a in atoms], np.uint32)
    return cols, chain, residue, list(chains)


# ---- the model against whole runs of the oracle -----------------------------------------------------------------

def _sub(cols, ids, sel):
    return [np.ascontiguousarray(a[sel]) for a in cols], None if ids is None else np.ascontiguousarray(ids[sel])


def _oracle_points(cols, ids, sel, probe, n_points, W):
    (sx, sy, sz, sr), sid = _sub(cols, ids, sel)
    _, pts, _ = po.calculate_sasa_internal(sx, sy, sz, sr, sid, probe, n_points, W, return_details=True)
    return pts.astype(np.int64)


def alone_check(x, y, z, r, ids, groups, probe, n_points, W, model):
    """(i) The oracle on every group alone: its atoms' accessible points must equal self_free.  Returns (groups
    compared, groups skipped because their largest radius is not the structure's)."""
    g = _labels(groups, len(x))
    rmax = nh.fold_max(r)
    done = skipped = 0
    for h in np.unique(g).tolist():
        sel = g == h
        if nh.fold_max(r[sel]) != rmax:
            skipped += 1
            continue
        pts = _oracle_points((x, y, z, r), ids, sel, probe, n_points, W)
        assert np.array_equal(pts, model[4][sel].astype(np.int64)), h
        done += 1
    return done, skipped


def pair_check(x, y, z, r, ids, groups, probe, n_points, W, model):
    """(ii) The oracle on every ordered pair of groups A, B together: the atoms of A must have self_free - buried_B
    accessible points.  Returns (pairs compared, pairs skipped for the largest radius)."""
    g = _labels(groups, len(x))
    rmax = nh.fold_max(r)
    labels = np.unique(g).tolist()
    done = skipped = 0
    for ka, A in enumerate(labels):
        for B in labels[ka + 1:]:
            sel = (g == A) | (g == B)
            if nh.fold_max(r[sel]) != rmax:
                skipped += 2
                continue
            pts = _oracle_points((x, y, z, r), ids, sel, probe, n_points, W)
            sub_g = g[sel]
            for own, other in ((A, B), (B, A)):
                bur, _ = row_lookup(model, other)
                want = (model[4].astype(np.int64) - bur)[sel][sub_g == own]
                assert np.array_equal(pts[sub_g == own], want), (own, other)
                done += 1
    return done, skipped


def deletion_check(x, y, z, r, ids, groups, probe, n_points, W, model):
    """(iii) The oracle on the structure without group h, for every h: every remaining atom must have free + only_h
    accessible points.  Returns (groups compared, groups skipped for the largest radius)."""
    g = _labels(groups, len(x))
    rmax = nh.fold_max(r)
    done = skipped = 0
    for h in np.unique(g).tolist():
        keep = g != h
        if not keep.any() or nh.fold_max(r[keep]) != rmax:
            skipped += 1
            continue
        pts = _oracle_points((x, y, z, r), ids, keep, probe, n_points, W)
        _, onl = row_lookup(model, h)
        assert np.array_equal(pts, (model[5].astype(np.int64) + onl)[keep]), h
        done += 1
    return done, skipped
