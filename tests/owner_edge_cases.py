"""The inputs of the second pass over the contact owners (test_owner_edges_cpu.py, test_gpu_owner_edges.py): what the
first suite of k_contact_owners (points.hip) never gave it.

    the exact ties of tie_cases.py, grouped into batches: co_test writes out the two dots of pt_hit itself, and only a
    point with dot == limit can tell its copy of the two rules from the original - tie_margins counts the points that do;
    PASS_WINDOW_CASES: lists of more than one window of 256 entries at point counts of three and four passes, where
    owned[] is added to across passes window by window;
    the degenerate radius / probe batches of point_edge_cases.py that the contact counts run.

Plain helper module (not a conftest)."""
import functools

import numpy as np

import bench_workloads as bw
import nb_helpers as nh
import owner_cases as oc
import owners_model as om
import point_edge_cases as pe
import tie_cases as tc
from oracle import pyoracle as po

WS = (8, 16)


# ---- exact ties -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tie_groups():
    """{(probe, n_points, W): [tie_cases.Structure]}: every structure of every case, as test_tie_cases_contacts groups them."""
    groups = {}
    for case in tc.all_cases():
        groups.setdefault((case.probe, case.n_points, case.W), []).extend(case.structures)
    return groups


def tie_margins(st, probe, n_points, W):
    """What the model decides at dot == limit in one structure, as two counts:
    rem_zero    remainder points (p >= n_fused) whose owner has margin exactly 0.0: dot == limit hits under `<=`;
    fused_kept  fused points (p < n_fused) with an entry at dot == limit, which does not hit under `<`, that stay free
                or belong to a later entry."""
    cols = st.soa()
    offs, ent = nh.oracle_csr(*cols, probe)
    o = offs.astype(np.int64)
    terms = om.entry_terms(*cols[:4], probe, offs, ent)
    pts = po.sphere_points(n_points)
    nf = tc.n_fused(n_points, W)
    rem_zero = fused_kept = 0
    for i in range(st.n):
        e0, e1 = int(o[i]), int(o[i + 1])
        if e1 == e0:
            continue
        dot_f, dot_u = om.dots(terms, e0, e1, pts, nf, nf)
        limit = terms[7][e0:e1]
        hit, m = om.hits_and_margins(dot_f, dot_u, limit, nf, nf, n_points)
        owner = om.walk(hit, m, np.array([0]), np.array([e1 - e0]))[0]
        if nf < n_points:
            p = np.arange(nf, n_points)
            owned = owner[p] != om.FREE
            at = m[owner[p][owned].astype(np.int64), p[owned]]
            rem_zero += int((at == 0.0).sum())
        if nf:
            e, p = np.nonzero(dot_f[:, :nf] == limit[:, None])
            assert not hit[e, p].any()                                  # `<`: no hit at equality
            fused_kept += int(((owner[p] == om.FREE) | (owner[p].astype(np.int64) > e)).sum())
    return rem_zero, fused_kept


# ---- passes x windows -----------------------------------------------------------------------------------------------------

# (case of test_gpu_owners._named_case, n_points): K = 599 at 513 points - three passes over three windows; K = 257 at 960
# points - four passes over two windows
PASS_WINDOW_CASES = (("late_owner", 513), (258, 960))


def named_cols(name):
    """(cols, the cluster's first atom)."""
    return oc.late_owner() if name == "late_owner" else nh.tight_cluster(name, seed=name)


def passes(n_points):
    chunks = -(-n_points // pe.WAVE)
    return -(-chunks // pe.nch(n_points))


def windows(k):
    return -(-k // oc.PT_STAGE)


@functools.lru_cache(maxsize=None)
def pass_window_model(name, n_points):
    """owners_model.owners_ws of the case at both lane counts, computed once and left unchanged."""
    cols, _ = named_cols(name)
    return om.owners_ws(*cols, 1.4, n_points, WS)


# ---- degenerate radii and probes, in a batch -----------------------------------------------------------------------------------

DEGENERATE_BATCH = (100, 16)       # n_points, W: n_fused = 96, both rules
N_DEGENERATE = 10


@functools.lru_cache(maxsize=None)
def _ordinary():
    b = bw.synthetic_proteome(30, seed=8)
    return tuple(b.structure(0)), tuple(b.structure(4))


def degenerate_batch(k):
    """Setting k of point_edge_cases.degenerate_settings on 1jcd, between two ordinary structures: (columns, structure
    offsets, probe) - the batches test_gpu_point_edges.py gives the contact counts."""
    cols = nh.protor("1jcd.pdb")
    _, probe, r = pe.degenerate_settings(cols[3])[k]
    first, last = _ordinary()
    parts = [first, pe.with_radii(cols, r), last]
    so = np.zeros(len(parts) + 1, np.uint32)
    so[1:] = np.cumsum([len(p[0]) for p in parts])
    return [np.ascontiguousarray(np.concatenate([p[j] for p in parts])) for j in range(5)], so, probe


def degenerate_models():
    """{k: (owned, owner)} of every degenerate batch, on a few threads."""
    _ordinary()   # (built once, before the threads start)

    def one(k):
        cat, so, probe = degenerate_batch(k)
        return om.owners_batch(*cat, so, probe, *DEGENERATE_BATCH)
    return pe.pmap(one, range(N_DEGENERATE))
