"""Surface components (rsasa_surface_components*) as seen without a GPU: the symbols and their documented signatures, the
Python side's checks, default_link, component_table and split_sasa, and the cases of depth_cases.py and
component_cases.py pinned to what they are named for, from the model (components_model.py) alone: a later edit of a
radius or a spacing cannot silently stop a case from testing what it tests."""
import os
import re

import numpy as np
import pytest

import component_cases as cc
import components_model as cm
import depth_cases as dc
import depth_model as dm

F = np.float32


def _link(c, n_points=100):
    return cc.default_link(c.r, c.probe, n_points)


# ---- the interface -------------------------------------------------------------------------------------------------

def _prototype(text, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, name
    return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]


def test_component_symbols_header_and_abi_version():
    from rustsasa_amd import _capi
    lib = _capi.load()
    for name in ("rsasa_surface_components", "rsasa_surface_components_batch"):
        assert hasattr(lib, name)
        assert name in _capi.SYMBOLS
        assert getattr(lib, name).argtypes == _capi.SYMBOLS[name][1]
    assert lib.rsasa_abi_version() == 4
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rustsasa_amd.h")
    with open(header) as f:
        text = f.read()
    cols = ["rsasa_context_t *ctx", "const float *x", "const float *y", "const float *z", "const float *radius",
            "const uint64_t *id"]
    outs = ["uint64_t *out_dot_offsets", "uint32_t *out_labels", "size_t labels_capacity", "uint32_t *out_free"]
    assert _prototype(text, "rsasa_surface_components") == cols + \
        ["size_t n_atoms", "float probe_radius", "size_t n_points", "float link"] + outs + ["float *out_sasa"]
    assert _prototype(text, "rsasa_surface_components_batch") == cols + \
        ["const uint32_t *structure_offsets", "size_t n_structures", "float probe_radius", "size_t n_points",
         "float link"] + outs + ["float *out_atom_sasa"]
    assert len(_capi.SYMBOLS["rsasa_surface_components"][1]) == 15
    assert len(_capi.SYMBOLS["rsasa_surface_components_batch"][1]) == 16
    for phrase in ("d2 <= link * link", "smallest dot number", "A NaN d2 links nothing", "one float32 product"):
        assert phrase in text, phrase


class _NoCall:
    """Stands in for the library: any C call fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_argument_errors_raise_before_the_c_call():
    import rustsasa_amd
    c = object.__new__(rustsasa_amd.Context)
    c._lib = _NoCall()
    c._h = None
    x = np.zeros(5, F)
    with pytest.raises(ValueError):
        c.surface_components(x, x, x[:4], x)
    with pytest.raises(ValueError):
        c.surface_components(x, x, x, x, ids=np.zeros(4, np.uint64))
    for n in (0, -3, 2.5):
        with pytest.raises(ValueError):
            c.surface_components(x, x, x, x, n_points=n)
        with pytest.raises(ValueError):
            c.surface_components_batch(x, x, x, x, None, [0, 5], n_points=n)
    with pytest.raises(ValueError):
        c.surface_components_batch(x, x, x, x, None, [0, 2, 4])            # offsets cover 4 of 5 atoms


def test_default_link_values():
    import rustsasa_amd
    got = rustsasa_amd.default_link(dc.RADII, 1.4, 100)
    assert isinstance(got, np.float32)
    assert got == F(1.5 * np.sqrt(4.0 * np.pi / 100) * (float(F(1.88)) + 1.4)) and abs(float(got) - 1.7441) < 5e-5
    assert got == cc.default_link(dc.RADII, 1.4, 100)
    # the largest FINITE radius, folded from 0
    odd = np.array([np.nan, -2.0, np.inf, 1.5], F)
    assert rustsasa_amd.default_link(odd, 1.0, 960) == F(1.5 * np.sqrt(4.0 * np.pi / 960) * 2.5)
    assert rustsasa_amd.default_link(np.array([-1.0, np.nan], F), 1.4, 100) == F(1.5 * np.sqrt(4.0 * np.pi / 100) * 1.4)
    assert rustsasa_amd.default_link(np.zeros(0, F), 1.4, 100) == F(1.5 * np.sqrt(4.0 * np.pi / 100) * 1.4)
    # it spans the largest nearest-dot gap of one sphere at both ends of the usual range
    for n_points in (100, 960):
        link = rustsasa_amd.default_link(dc.RADII, 1.4, n_points)
        one = (np.zeros(1, F),) * 3 + (np.array([1.88], F),)
        _, labels, _ = cm.components(*one, None, 1.4, n_points, link, mask=np.ones((1, n_points), bool))
        assert not labels.any()
    with pytest.raises(ValueError):
        rustsasa_amd.default_link(dc.RADII, 1.4, 0)


# ---- component_table and split_sasa ----------------------------------------------------------------------------------

def _direct_table(off, labels, r, probe, n_points, b_atom, e_atom):
    """One structure's table by a direct bincount, rows in label order."""
    off = off.astype(np.int64)
    b, e = int(off[b_atom]), int(off[e_atom])
    lab = labels[b:e].astype(np.int64)
    owner = np.repeat(np.arange(b_atom, e_atom), np.diff(off[b_atom:e_atom + 1]))
    R = (r + F(probe)).astype(np.float64)
    a = 4.0 * np.pi * (R * R) / n_points
    rep = np.unique(lab)
    dots = np.bincount(lab, minlength=max(e - b, 1))[rep]
    area = np.bincount(lab, weights=a[owner], minlength=max(e - b, 1))[rep]
    atoms = np.array([len(np.unique(owner[lab == v])) for v in rep], np.int64)
    return rep, dots, area, atoms, owner, a


def test_component_table_and_split_sasa_against_a_direct_bincount():
    import rustsasa_amd
    parts = [cc.get("cavity").part(0)[:4] + (None,), cc.get("tiny").part(4)[:4] + (None,),
             (np.zeros(0, F),) * 4 + (None,), cc.get("twins").part(0)[:4] + (None,)]
    c = dc._case("table", parts)
    link = F(0.9)                                        # below the dot spacing in places: many components of many sizes
    off, labels, mask = cm.components_batch(*c.cols, c.so, c.probe, 100, link)
    c_off, label, dots, area, atoms = rustsasa_amd.component_table(off, labels, c.r, c.probe, 100, c.so)
    assert c_off.dtype == np.int64 and label.dtype == np.uint32 and dots.dtype == np.int64
    assert area.dtype == np.float64 and atoms.dtype == np.int64
    assert c_off.shape == (5,) and c_off[0] == 0 and c_off[3] == c_off[2]          # the empty structure has no rows
    outer, cavity = rustsasa_amd.split_sasa(off, labels, c.r, c.probe, 100, c.so)
    assert outer.dtype == cavity.dtype == np.float64 and outer.shape == cavity.shape == (c.n_atoms,)
    for s in range(4):
        b_atom, e_atom = int(c.so[s]), int(c.so[s + 1])
        rep, w_dots, w_area, w_atoms, owner, a = _direct_table(off, labels, c.r, c.probe, 100, b_atom, e_atom)
        rows = slice(int(c_off[s]), int(c_off[s + 1]))
        assert len(rep) == c_off[s + 1] - c_off[s]
        if not len(rep):
            continue
        order = np.lexsort((rep, -w_area))                                         # area descending, ties to the smaller label
        assert np.array_equal(label[rows], rep[order]) and np.array_equal(dots[rows], w_dots[order])
        assert np.array_equal(area[rows], w_area[order]) and np.array_equal(atoms[rows], w_atoms[order])
        assert (np.diff(area[rows]) <= 0).all() and dots[rows].sum() == len(owner)
        lab = labels[int(off[b_atom]):int(off[e_atom])]
        first = lab == label[rows][0]
        assert np.array_equal(outer[b_atom:e_atom], np.bincount(owner[first] - b_atom, weights=a[owner[first]], minlength=e_atom - b_atom))
        assert np.array_equal(cavity[b_atom:e_atom], np.bincount(owner[~first] - b_atom, weights=a[owner[~first]], minlength=e_atom - b_atom))
    assert len(np.unique(dots)) > 3 and (atoms > 1).any() and (cavity > 0).any() and (outer > 0).any()
    # one structure without offsets; equal areas go to the smaller label
    p = cc.get("pole_tie")
    t = rustsasa_amd.component_table(np.array([0, 1, 2], np.uint64), np.array([0, 1], np.uint32), p.r, p.probe, 1)
    assert t[0].tolist() == [0, 2] and t[1].tolist() == [0, 1] and t[2].tolist() == [1, 1] and t[4].tolist() == [1, 1]
    assert t[3][0] == t[3][1] == 4.0 * np.pi * 4.0
    o, v = rustsasa_amd.split_sasa(np.array([0, 1, 2], np.uint64), np.array([0, 1], np.uint32), p.r, p.probe, 1)
    assert o.tolist() == [t[3][0], 0.0] and v.tolist() == [0.0, t[3][1]]
    for bad in (dict(dot_offsets=[0, 1]), dict(labels=[0]), dict(labels=[0, 2]), dict(structure_offsets=[0, 1])):
        args = dict(dot_offsets=np.array([0, 1, 2], np.uint64), labels=np.array([0, 1], np.uint32), radius=p.r,
                    probe_radius=1.0, n_points=1)
        args.update(bad)
        with pytest.raises(ValueError):
            rustsasa_amd.component_table(**args)


# ---- the cases -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cavity_model():
    c = dc.get("cavity")
    return cm.components(*c.cols, c.probe, 100, _link(c), with_edges=True)


def test_ball_is_one_component():
    c = dc.get("ball")
    off, labels, _ = cm.components(*c.cols, c.probe, 100, _link(c))
    assert len(labels) == 2391 and off[-1] == 2391 and not labels.any()


def test_cavity_is_the_outside_and_the_void(cavity_model):
    c = dc.get("cavity")
    off, labels, mask, edges, owner = cavity_model
    rep, n = cm.sizes(labels)
    assert n.tolist() == [2391, 34] and rep[0] == 0
    _, qx, qy, qz = dm.dots_of(*c.cols[:4], mask, c.probe, 100)
    d = np.linalg.norm(np.stack([qx, qy, qz], -1).astype(np.float64) - dc.VOID_CENTRE, axis=1)
    assert np.array_equal(np.flatnonzero(d <= dc.VOID_RADIUS), np.flatnonzero(labels == rep[1]))
    # the void shares no edge with the outside
    assert (labels[edges[:, 0]] == labels[edges[:, 1]]).all() and len(edges) > len(labels)


def test_twins_at_link_zero_hold_only_exact_ties():
    c = dc.get("twins")
    off, labels, mask, edges, owner = cm.components(*c.cols, c.probe, 100, 0.0, with_edges=True)
    assert len(labels) == 268 and len(np.unique(labels)) == 178 and len(edges) == 90
    _, qx, qy, qz = dm.dots_of(*c.cols[:4], mask, c.probe, 100)
    a, b = edges[:, 0], edges[:, 1]
    dx, dy, dz = qx[a] - qx[b], qy[a] - qy[b], qz[a] - qz[b]
    assert ((dx * dx + dy * dy + dz * dz) == 0).all()
    assert set(owner[a]) == {1} and set(owner[b]) == {2}          # the coinciding atoms' dots, pair by pair


def test_pole_tie_sits_on_the_tie():
    c = cc.get("pole_tie")
    mask = np.ones((2, 1), bool)
    _, qx, qy, qz = dm.dots_of(*c.cols[:4], mask, c.probe, 1)
    assert qx.tolist() == [0.0, 3.0] and qy.tolist() == [0.0, 0.0] and qz.tolist() == [2.0, 2.0]   # the exact +z pole
    off, labels, m = cm.components(*c.cols, c.probe, 1, F(3.0))
    assert m.all() and labels.tolist() == [0, 0]                  # d2 == link * link == 9
    assert cm.components(*c.cols, c.probe, 1, np.nextafter(F(3.0), F(0.0)))[1].tolist() == [0, 1]


def test_far_link_reaches_three_cells_and_not_beyond():
    pairs = cc.far_link_pairs()
    assert [(a, s) for a, s, _, _ in pairs] == cc.DIRECTIONS
    h = float(cc.H)
    near, far = cc.get("far_link"), cc.far_link(0.5)
    assert len(near.so) == 13 and near.n_atoms == 24
    for n, (axis, sign, base, dist) in enumerate(pairs):
        assert 2.0 * h + h - 0.25 <= dist < 2.0 * h + h               # just under 2 h + link
        for swap in (0, 1):
            s = 2 * n + swap
            part = near.part(s)
            assert cc._cell_gap(part, axis) == 3                      # cells that differ by 3 along the axis
            assert cc.cross_edges(part, cc.H) >= 1                    # and an edge between the two atoms
            assert np.sign(part[axis][1 - swap] - part[axis][swap]) == sign
            assert cc.cross_edges(far.part(s), cc.H) == 0             # 0.5 A further apart: none
    # the atoms do not occlude each other, so every point of both is a dot
    p = near.part(0)
    assert np.linalg.norm([p[k][0] - p[k][1] for k in range(3)]) > 2.0 * h


def test_multi_chunk_fills_2_2_3_and_15_chunks():
    c = cc.get("multi_chunk")
    assert [-(-n // 64) for n in cc.CHUNK_POINTS] == [2, 2, 3, 15]
    for n_points in cc.CHUNK_POINTS:
        off, labels, mask = cm.components_batch(*c.cols, c.so, c.probe, n_points, _link(c, n_points))
        assert mask[0].all() and mask[-1].all()                       # the lone atoms: every point
        free = mask[1:4].sum(axis=1)
        assert (free > 0).all() and (free < n_points).all()           # the cluster: part of every atom
        assert n_points == 65 or (mask[1:4, 64:].any(axis=1)).all()   # in more chunks than the first
        for s in range(3):
            b, e = int(off[c.so[s]]), int(off[c.so[s + 1]])
            assert not labels[b:e].any()                              # each structure is one component


def test_example_cif_with_vdw_radii_has_pockets():
    import rustsasa_amd
    c = cc.get("example_vdw")
    assert c.n_atoms == 2622
    off, labels, mask = cm.components(*c.cols, c.probe, 100, 2.0)
    rep, n = cm.sizes(labels)
    assert len(labels) == 16843 and len(rep) == 10 and n[0] == 16823 and n[1:].tolist() == [5, 4, 3, 2, 2, 1, 1, 1, 1]
    per_atom = [len(np.unique(labels[int(off[i]):int(off[i + 1])])) for i in range(c.n_atoms)]
    assert sum(k > 1 for k in per_atom) == 4                          # atoms that own dots of more than one component
    t = rustsasa_amd.component_table(off, labels, c.r, c.probe, 100)
    assert t[0].tolist() == [0, 10] and t[1][0] == 0 and t[2][0] == 16823
    outer, cavity = rustsasa_amd.split_sasa(off, labels, c.r, c.probe, 100)
    assert (cavity > 0).sum() == len(np.unique(np.repeat(np.arange(c.n_atoms), mask.sum(axis=1))[labels != 0]))


def test_a_permutation_of_the_atoms_maps_the_partition_onto_itself():
    c = dc.get("cavity")
    link = _link(c)
    off, labels, mask = cm.components(*c.cols, c.probe, 100, link)
    perm = np.random.default_rng(3).permutation(c.n_atoms)
    p_off, p_labels, p_mask = cm.components(*(a[perm] for a in c.cols), c.probe, 100, link)
    assert np.array_equal(p_mask, mask[perm])
    # dot (perm[i], k) of the original is dot (i, k) of the permuted input
    src = np.concatenate([np.arange(int(off[j]), int(off[j + 1])) for j in perm]).astype(np.int64)
    assert len(src) == len(labels)
    a, b = labels[src].astype(np.int64), p_labels.astype(np.int64)
    pairs = np.unique(np.stack([a, b], -1), axis=0)
    assert len(pairs) == len(np.unique(a)) == len(np.unique(b)) == 2      # a bijection between the two partitions
