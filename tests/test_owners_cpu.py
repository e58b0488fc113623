"""Contact owners (rsasa_contact_owners*) as seen without a GPU: the exact CPU model of owners_model.py - the
yardstick the GPU tests compare with - checked against the float64 power distance it approximates, against the
identities that tie it to contacts_model.py, on exact ties and under permutation; owner_areas; the header, the
bindings and the exported symbols."""
import os
import re

import numpy as np
import pytest

import contacts_model as cm
import nb_helpers as nh
import owner_cases as oc
import owners_model as om
import point_edge_cases as pe
import tie_cases as tc
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rustsasa_amd.h")
FIXTURES = ["example.cif:vdw", "1jcd.pdb", "151L_H3.pdb"]
N_POINTS = (100, 101, 127, 960)
WS = (1, 4, 8, 16)
EPS = 2.0 ** -24


# ---- 1: the float32 margin against the float64 power distance ---------------------------------------------------

@pytest.mark.parametrize("name, probe, n_points", [("1jcd.pdb", 1.4, 100), ("1jcd.pdb", 3.0, 127), ("151L_H3.pdb", 1.4, 100)])
def test_margin_is_the_power_distance(name, probe, n_points):
    """With P = c_i + R s (R and threshold_squared taken as their float32 values), pw_j = |P - c_j|^2 - th_j and
    S = th + d^2 + R^2 + 2 R (|vx| + |vy| + |vz|): |2 R m - pw| <= 16 * 2^-24 * S for every hitting pair (16 counts the
    float32 operations from the coordinates to m), and the model's owner is the float64 argmin wherever the best pw
    beats the runner-up by more than 32 * 2^-24 * S, S the larger of the two entries' (each margin is within
    16 * 2^-24 * S of its pw, so a wider gap fixes the order)."""
    W = 8
    cols = nh.protor(name)
    x, y, z, r = (np.ascontiguousarray(a, np.float32) for a in cols[:4])
    offs, ent, owned, owner = om.owners(*cols, probe, n_points, W)
    o = offs.astype(np.int64)
    terms = om.entry_terms(x, y, z, r, probe, offs, ent)
    _, j, vx, vy, vz, d2, R, limit = terms
    pts = po.sphere_points(n_points)
    s64 = np.stack([p.astype(np.float64) for p in pts], axis=1)                    # [n_points, 3]
    c64 = np.stack([x, y, z], axis=1).astype(np.float64)
    th = ent["threshold_squared"].astype(np.float32).astype(np.float64)
    nf = tc.n_fused(n_points, W)
    worst, n_hit, n_decided, n_points_hit = 0.0, 0, 0, 0
    for i in range(len(x)):
        e0, e1 = int(o[i]), int(o[i + 1])
        if e1 == e0:
            continue
        hit, m = om.hits_and_margins(*om.dots(terms, e0, e1, pts, nf, nf), limit[e0:e1], nf, nf, n_points)
        Ri = float(R[e0])
        P = c64[i] + Ri * s64                                                      # [n_points, 3]
        d = P[None, :, :] - c64[j[e0:e1]][:, None, :]                              # [K, n_points, 3]
        pw = (d * d).sum(axis=2) - th[e0:e1, None]
        S = (th[e0:e1] + d2[e0:e1].astype(np.float64) + Ri * Ri
             + 2.0 * Ri * (np.abs(vx[e0:e1]) + np.abs(vy[e0:e1]) + np.abs(vz[e0:e1])).astype(np.float64))
        err = np.abs(2.0 * Ri * m.astype(np.float64) - pw) / S[:, None]
        if hit.any():
            worst = max(worst, float(err[hit].max()) / EPS)
        n_hit += int(hit.sum())
        # the float64 argmin over the hitting entries, and its lead over the runner-up
        pwh = np.where(hit, pw, np.inf)
        order = np.argsort(pwh, axis=0, kind="stable")
        best = order[0]
        cols_ = np.arange(n_points)
        with np.errstate(invalid="ignore"):  # (a free point: inf - inf, not `some`)
            lead = (pwh[order[1], cols_] - pwh[best, cols_]) if e1 - e0 > 1 else np.full(n_points, np.inf)
        some = hit.any(axis=0)
        second = order[1] if e1 - e0 > 1 else best
        decided = some & (lead > 32.0 * EPS * np.maximum(S[best], S[second]))
        assert np.array_equal(owner[i][decided], best[decided].astype(np.uint32)), i
        assert np.array_equal(owner[i] != om.FREE, some), i
        n_decided += int(decided.sum())
        n_points_hit += int(some.sum())
    print(f"{name} {probe} {n_points}: max |2Rm - pw| = {worst:.3f} * 2^-24 * S over {n_hit} hitting pairs; "
          f"{n_decided} of {n_points_hit} buried points decided by the float64 lead")
    assert worst <= 16.0
    assert n_hit > 100 * len(x) // 4 and n_decided > 0.99 * n_points_hit


# ---- 2: the identities that tie owned to covered, exclusive and the buried points -------------------------------

@pytest.fixture(scope="module")
def fixture_models():
    """{(fixture, n_points): (offsets, entries, {W: (owned, owner)}, {W: (covered, exclusive, buried)})}"""
    def one(key):
        name, n = key
        cols = pe.fixture(name)
        lists = nh.oracle_csr(*cols, 1.4)
        offs, ent, own = om.owners_ws(*cols, 1.4, n, WS, lists)
        _, _, cnt = cm.contact_counts_ws(*cols, 1.4, n, WS, lists)
        return offs, ent, own, cnt
    return pe.pmap(one, [(f, n) for f in FIXTURES for n in N_POINTS])


@pytest.mark.parametrize("n_points", N_POINTS)
@pytest.mark.parametrize("name", FIXTURES)
def test_identities_against_the_contact_model(fixture_models, name, n_points):
    offs, ent, own, cnt = fixture_models[(name, n_points)]
    o = offs.astype(np.int64)
    n = len(o) - 1
    k = np.diff(o)
    rows = np.repeat(np.arange(n), k)
    for W in WS:
        owned, owner = own[W]
        cov, exc, buried = cnt[W]
        s = np.zeros(n, np.int64)
        np.add.at(s, rows, owned.astype(np.int64))
        assert np.array_equal(s, buried)                                  # a partition of the buried points
        assert np.array_equal((owner != om.FREE).sum(axis=1), buried)
        assert np.all(exc <= owned) and np.all(owned <= cov)
        one = k[rows] == 1
        assert np.array_equal(owned[one], cov[one]) and np.array_equal(owned[one], exc[one])
        assert (owned < cov).any() and (exc < owned).any()
        # owner and owned say the same
        at, _ = np.nonzero(owner != om.FREE)
        again = np.bincount(o[at] + owner[owner != om.FREE].astype(np.int64), minlength=len(owned))
        assert np.array_equal(again, owned)


def test_one_entry_lists():
    """K = 1: owned = covered = exclusive (two atoms, and the pair inside a batch-like larger structure)."""
    f = lambda *a: np.array(a, np.float32)  # noqa: E731
    cols = (f(0, 2.5, 40, 42), f(0, 0, 0, 0.5), f(0, 0, 1, 0), f(1.7, 1.5, 1.9, 1.2), None)
    for n_points in (100, 101):
        for W in WS:
            offs, ent, owned, owner = om.owners(*cols, 1.4, n_points, W)
            _, _, cov, exc = cm.contact_counts(*cols, 1.4, n_points, W, lists=(offs, ent))
            assert np.diff(offs.astype(np.int64)).tolist() == [1, 1, 1, 1]
            assert np.array_equal(owned, cov) and np.array_equal(owned, exc) and (owned > 0).all()
            assert set(np.unique(owner).tolist()) == {0, om.FREE}


# ---- 3: exact ties ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_points, W", [(100, 8), (101, 16)])
def test_twins_the_earlier_owns(n_points, W):
    """dups: in every list that holds an atom and its copy, the copy (the later position) owns nothing although it
    covers what the original covers, and the original owns what it owns in the structure without the copies."""
    cols, original, twins = oc.dups()
    n0 = int(twins[0])
    lists = nh.oracle_csr(*cols, 1.4)
    offs, ent, owned, owner = om.owners(*cols, 1.4, n_points, W, lists)
    _, _, cov, _ = cm.contact_counts(*cols, 1.4, n_points, W, lists)
    e_orig, e_twin = oc.twin_entries(offs, ent, original, twins)
    assert not owned[e_twin].any() and np.array_equal(cov[e_twin], cov[e_orig]) and (cov[e_twin] > 0).sum() > 500
    assert (owned[e_orig] > 0).sum() > 100
    # without the copies: the lists of the atoms that have no copy lose the copies' entries and nothing else changes
    base = tuple(a[:n0] for a in cols)
    offs0, ent0, owned0, _ = om.owners(*base, 1.4, n_points, W)
    o, o0 = offs.astype(np.int64), offs0.astype(np.int64)
    plain = np.setdiff1d(np.arange(n0), original)
    for i in plain.tolist():
        keep = ent["idx"][o[i]:o[i + 1]] < n0
        assert np.array_equal(ent["idx"][o[i]:o[i + 1]][keep], ent0["idx"][o0[i]:o0[i + 1]])
        assert np.array_equal(owned[o[i]:o[i + 1]][keep], owned0[o0[i]:o0[i + 1]]), i
        assert not owned[o[i]:o[i + 1]][~keep].any()


def test_twins_across_the_stage_boundary():
    cols, centre, twin = oc.dup_stage()
    lists = nh.oracle_csr(*cols, 1.4)
    oc.assert_dup_stage(cols, centre, twin, *lists)
    for n_points, W in ((100, 8), (130, 16)):
        offs, ent, owned, owner = om.owners(*cols, 1.4, n_points, W, lists)
        _, _, cov, _ = cm.contact_counts(*cols, 1.4, n_points, W, lists)
        lo = int(offs[centre])
        assert owned[lo + oc.PT_STAGE] == 0 and cov[lo + oc.PT_STAGE] == cov[lo + oc.PT_STAGE - 1] > 0
        assert not (owner[centre] == oc.PT_STAGE).any()
        # the earlier twin owns what it owns without the later one
        base = tuple(a[:twin] for a in cols)
        offs0, ent0, owned0, owner0 = om.owners(*base, 1.4, n_points, W)
        lo0 = int(offs0[centre])
        assert owned[lo + oc.PT_STAGE - 1] == owned0[lo0 + oc.PT_STAGE - 1]
        shifted = np.where((owner0[centre] >= oc.PT_STAGE) & (owner0[centre] != om.FREE), owner0[centre] + 1, owner0[centre])
        assert np.array_equal(owner[centre], shifted)


def test_late_owner_case():
    cols, c0 = oc.late_owner()
    _, _, owned, owner = om.owners(*cols, 1.4, 100, 8)
    oc.assert_late_owner(owner, c0)


# ---- 4: permutation ---------------------------------------------------------------------------------------------

def _table(offs, ent, owned, name_of):
    o = offs.astype(np.int64)
    rows = np.repeat(np.arange(len(o) - 1), np.diff(o))
    return {(int(name_of[i]), int(name_of[j])): int(c) for i, j, c in zip(rows, ent["idx"].astype(np.int64), owned)}


def test_permuting_the_atoms_permutes_owned():
    cols = nh.protor("151L_H3.pdb")
    n = len(cols[0])
    xyz = np.stack(cols[:3], axis=1)
    assert len(np.unique(xyz, axis=0)) == n                               # duplicate-free
    want = _table(*om.owners(*cols, 1.4, 101, 8)[:3], np.arange(n))
    assert sum(want.values()) > 0
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(n)                 # new atom i is old atom perm[i]
        pc = tuple(np.ascontiguousarray(a[perm]) for a in cols)
        assert _table(*om.owners(*pc, 1.4, 101, 8)[:3], perm) == want


# ---- 5: owner_areas ---------------------------------------------------------------------------------------------

def test_owner_areas_against_a_direct_loop_and_additivity():
    from rustsasa_amd import contact_areas, owner_areas
    a, b = nh.protor("1jcd.pdb"), nh.protor("151L_H3.pdb")
    n_points, probe = 100, 1.4
    parts = [om.owners(*c, probe, n_points, 8) for c in (a, b)]
    so = np.array([0, len(a[0]), len(a[0]) + len(b[0])], np.uint32)
    n = int(so[-1])
    offs = np.concatenate([parts[0][0], parts[1][0][1:] + parts[0][0][-1]])
    ent = np.concatenate([parts[0][1], parts[1][1]])
    owned = np.concatenate([parts[0][2], parts[1][2]])
    owner = np.concatenate([parts[0][3], parts[1][3]])
    radius = np.concatenate([a[3], b[3]])
    labels = (np.arange(n) // 37 % 11 + 5).astype(np.uint32)              # labels shared by the two structures
    frm, to, area = owner_areas(offs, ent, owned, labels, radius, probe, n_points, structure_offsets=so)
    assert frm.dtype == np.uint32 and to.dtype == np.uint32 and area.dtype == np.float64
    key = frm.astype(np.uint64) << np.uint64(32) | to.astype(np.uint64)
    assert np.all(np.diff(key.astype(np.int64)) > 0) and (frm == to).any()
    per_entry = contact_areas(owned, offs, radius, probe, n_points)
    want, want_counts = {}, {}
    o = offs.astype(np.int64)
    for i in range(n):
        base = int(so[np.searchsorted(so[1:], i, side="right")])
        for e in range(int(o[i]), int(o[i + 1])):
            k = (int(labels[i]), int(labels[base + int(ent["idx"][e])]))
            want[k] = want.get(k, 0.0) + float(per_entry[e])
            want_counts[k] = want_counts.get(k, 0) + int(owned[e])
    assert sorted(want) == list(zip(frm.tolist(), to.tolist()))
    assert np.allclose(area, [want[k] for k in sorted(want)], rtol=1e-12, atol=0.0)
    # additivity, exact in counts: per label, owned by anybody + free = n_points per atom
    free = (owner == om.FREE).sum(axis=1)
    for lab in np.unique(labels).tolist():
        lost = sum(c for (f, _), c in want_counts.items() if f == lab)
        assert lost + int(free[labels == lab].sum()) == n_points * int((labels == lab).sum())
    # ... and in areas up to the float32 rounding of each term
    R = (radius + np.float32(probe)).astype(np.float64)
    full = 4.0 * np.pi * R * R
    for lab in np.unique(labels).tolist():
        sel = labels == lab
        sasa = float((full[sel] * free[sel] / n_points).sum())
        assert abs(area[frm == lab].sum() + sasa - full[sel].sum()) <= 1e-5 * full[sel].sum()
    # one structure without offsets; argument errors
    f1, t1, a1 = owner_areas(parts[0][0], parts[0][1], parts[0][2], labels[:so[1]], a[3], probe, n_points)
    assert a1.sum() == pytest.approx(float(contact_areas(parts[0][2], parts[0][0], a[3], probe, n_points).astype(np.float64).sum()))
    with pytest.raises(ValueError):
        owner_areas(offs, ent, owned, labels[:-1], radius, probe, n_points, structure_offsets=so)
    with pytest.raises(ValueError):
        owner_areas(offs, ent, owned, labels, radius, probe, n_points, structure_offsets=so[:2])
    with pytest.raises(ValueError):
        owner_areas(offs, ent[:-1], owned, labels, radius, probe, n_points, structure_offsets=so)
    with pytest.raises(ValueError):
        owner_areas(offs, ent, owned, labels.astype(np.float32), radius, probe, n_points, structure_offsets=so)


# ---- 6: header, bindings, symbols -------------------------------------------------------------------------------

def test_owner_symbols_header_and_abi():
    from rustsasa_amd import _capi
    lib = _capi.load()
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("rsasa_contact_owners", "rsasa_contact_owners_batch"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code)
        assert hasattr(lib, name)
        assert name in _capi.SYMBOLS
        assert getattr(lib, name).argtypes == _capi.SYMBOLS[name][1]
    one, many = _capi.SYMBOLS["rsasa_contact_owners"], _capi.SYMBOLS["rsasa_contact_owners_batch"]
    assert len(one[1]) == 15 and len(many[1]) == 16
    assert re.search(r"#define\s+RSASA_ABI_VERSION\s+4\b", text) and lib.rsasa_abi_version() == 4
    # the rule's numeric parts: the header, the README and the model's docstring state them in the same words
    # (compared without line breaks, comment stars and code quotes)
    flat = lambda s: re.sub(r"[\s*`]+", " ", s)  # noqa: E731
    readme = open(os.path.join(ROOT, "README.md")).read()
    for phrase in ("m(e, p) = fmaf(sx, vx, fmaf(sy, vy, sz*vz)) - limit for p < n_fused",
                   "m(e, p) = ((sx*vx + sy*vy) + sz*vz) - limit for later points",
                   "the same dot as the hit rule for that point, followed by one float32 subtraction, unfused",
                   "m(e, p) < m(owner, p)", "0xFFFFFFFF"):
        for where in (text, readme, om.__doc__):
            assert flat(phrase) in flat(where), phrase


class _NoCall:
    """Stands in for the library: any C call fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_argument_errors_raise_before_the_c_call():
    from rustsasa_amd import Context
    c = object.__new__(Context)
    c._lib = _NoCall()
    c._h = None
    x = np.zeros(5, np.float32)
    with pytest.raises(ValueError):
        c.contact_owners(x, x, x[:4], x)
    for n in (0, -3, 2.5):
        with pytest.raises(ValueError):
            c.contact_owners(x, x, x, x, n_points=n, points=True)
        with pytest.raises(ValueError):
            c.contact_owners_batch(x, x, x, x, None, [0, 5], n_points=n)
    with pytest.raises(ValueError):
        c.contact_owners_batch(x, x, x, x, None, [0, 2, 4])
