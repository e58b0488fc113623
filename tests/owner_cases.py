"""The named inputs of the contact-owner tests (test_owners_cpu.py, test_gpu_owners.py), each with an assertion of
what it is named for: twins that tie on every point (dups, and dup_stage with the pair across the LDS stage boundary of
k_contact_owners) and clusters whose far atoms own points from positions behind the first and second stage
(late_owner).  Plain helper module (not a conftest)."""
import numpy as np

import nb_helpers as nh
import owners_model as om

PT_STAGE = 256  # list entries per LDS stage (kPtStage)


def _append(cols, src, first_id):
    """cols with copies of the atoms `src` appended (same coordinates and radius, new ids from first_id)."""
    x, y, z, r, ids = cols
    cat = lambda a: np.ascontiguousarray(np.concatenate([a, a[src]]))  # noqa: E731
    new_ids = np.arange(first_id, first_id + len(src), dtype=np.uint64)
    return cat(x), cat(y), cat(z), cat(r), np.ascontiguousarray(np.concatenate([ids, new_ids]))


# ---- dup_stage: a pair of twins at positions 255 and 256 of one list ----

DUP_STAGE_CLUSTER = (300, 17)  # (atoms, seed) of the tight cluster before the twin is added


def dup_stage():
    """(cols, centre, twin): a tight cluster in which the atom at position 255 of the list of the cluster's first atom
    (`centre`) is duplicated as the structure's last atom `twin`, so positions 255 and 256 of that list tie on every
    point: the last entry of the first stage and the first of the second."""
    n, seed = DUP_STAGE_CLUSTER
    cols, c0 = nh.tight_cluster(n, seed=seed)
    offs, ent = nh.oracle_csr(*cols, 1.4)
    j = int(ent["idx"][int(offs[c0]) + PT_STAGE - 1])
    out = _append(cols, np.array([j]), 2 * 10 ** 6)
    return out, c0, len(out[0]) - 1


def assert_dup_stage(cols, centre, twin, offs, ent):
    """offs, ent: the lists of cols.  Positions 255 and 256 of the centre's list are the original and its twin."""
    lo = int(offs[centre])
    assert int(offs[centre + 1]) - lo == DUP_STAGE_CLUSTER[0] > PT_STAGE + 1
    a, b = ent[lo + PT_STAGE - 1], ent[lo + PT_STAGE]
    assert int(b["idx"]) == twin and int(a["idx"]) < twin
    assert a["threshold_squared"] == b["threshold_squared"]
    assert all(c[int(a["idx"])] == c[twin] for c in cols[:4]) and cols[4][int(a["idx"])] != cols[4][twin]


# ---- dups: every 7th atom of a small protein twice ----

DUPS_PROTEIN = "1jcd.pdb"


def dups():
    """(cols, original, twins): DUPS_PROTEIN with every 7th atom duplicated behind the protein; original[k] is the atom
    twins[k] copies.  A twin follows its original in every list that holds both (the same d^2, a larger idx)."""
    cols = nh.protor(DUPS_PROTEIN)
    n = len(cols[0])
    src = np.arange(0, n, 7)
    out = _append(cols, src, 3 * 10 ** 6)
    assert len(np.unique(out[4])) == len(out[4])
    return out, src, n + np.arange(len(src))


def twin_entries(offs, ent, original, twins):
    """(e_orig, e_twin): the entries of the lists of atoms that are neither an original nor a twin which hold a twin,
    and the entries of the same lists that hold its original.  The pair sits at neighbouring positions."""
    o = offs.astype(np.int64)
    n = len(o) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(o))
    idx = ent["idx"].astype(np.int64)
    of_twin = np.full(n, -1, np.int64)
    of_twin[twins] = original
    involved = np.zeros(n, bool)
    involved[original] = involved[twins] = True
    e_twin = np.nonzero((of_twin[idx] >= 0) & ~involved[rows])[0]
    e_orig = e_twin - 1
    assert len(e_twin) > 1000
    assert np.array_equal(rows[e_orig], rows[e_twin]) and np.array_equal(idx[e_orig], of_twin[idx[e_twin]])
    return e_orig, e_twin


# ---- late_owner: owners behind the first and the second stage ----

LATE_OWNER = (600, 1)  # (atoms, seed) of nh.tight_cluster: K = 599, three stages


def late_owner():
    """(cols, c0): a tight cluster whose far atoms own the far side of every sphere."""
    return nh.tight_cluster(LATE_OWNER[0], seed=LATE_OWNER[1])


def assert_late_owner(owner, c0):
    """owner: the model's owner positions of late_owner() (any lane count).  Points are owned from the second and from
    the third stage, and from the first."""
    o = owner[c0:]
    o = o[o != om.FREE]
    assert (o < PT_STAGE).any() and ((o >= PT_STAGE) & (o < 2 * PT_STAGE)).any() and (o >= 2 * PT_STAGE).any()
