"""Atom depth (rsasa_atom_depth*) as seen without a GPU: the symbols and their documented signatures, the Python side's
checks and residue_depth, the model (depth_model.py) against a lone sphere and against a float64 nearest-dot search over
surface_points(), and the cases of depth_cases.py pinned to the classes they are named for, from the model alone: a
later edit of a radius or a spacing cannot silently stop a case from testing what it tests."""
import os
import re

import numpy as np
import pytest

import depth_cases as dc
import depth_model as dm
import point_edge_cases as pe
import points_model as pm

F = np.float32
N_POINTS = 100


@pytest.fixture(scope="module")
def models():
    """{case: (depth, nearest, mask)} of the small cases at 100 points, W = 8, side by side."""
    return pe.pmap(lambda name: dm.atom_depth_batch(*dc.get(name).cols, dc.get(name).so, dc.get(name).probe, N_POINTS),
                   dc.SMALL)


# ---- the interface -------------------------------------------------------------------------------------------------

def _prototype(text, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, name
    return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]


def test_depth_symbols_header_and_abi_version():
    from rustsasa_amd import _capi
    lib = _capi.load()
    for name in ("rsasa_atom_depth", "rsasa_atom_depth_batch"):
        assert hasattr(lib, name)
        assert name in _capi.SYMBOLS
        assert getattr(lib, name).argtypes == _capi.SYMBOLS[name][1]
    assert lib.rsasa_abi_version() == 4
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rustsasa_amd.h")
    with open(header) as f:
        text = f.read()
    assert re.search(r"#define\s+RSASA_ABI_VERSION\s+4\b", text)
    cols = ["rsasa_context_t *ctx", "const float *x", "const float *y", "const float *z", "const float *radius",
            "const uint64_t *id"]
    outs = ["float *out_depth", "uint32_t *out_nearest", "uint32_t *out_free"]
    assert _prototype(text, "rsasa_atom_depth") == cols + ["size_t n_atoms", "float probe_radius", "size_t n_points"] + \
        outs + ["float *out_sasa"]
    assert _prototype(text, "rsasa_atom_depth_batch") == cols + \
        ["const uint32_t *structure_offsets", "size_t n_structures", "float probe_radius", "size_t n_points"] + outs + \
        ["float *out_atom_sasa"]
    assert len(_capi.SYMBOLS["rsasa_atom_depth"][1]) == 13 and len(_capi.SYMBOLS["rsasa_atom_depth_batch"][1]) == 14
    # the definition, the tie rule and the case without a dot are in the header
    for phrase in ("bits(d2) << 32", "smallest index", "0xFFFFFFFF", "+inf", "does not subtract"):
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
        c.atom_depth(x, x, x[:4], x)
    with pytest.raises(ValueError):
        c.atom_depth(x, x, x, x, ids=np.zeros(4, np.uint64))
    for n in (0, -3, 2.5):
        with pytest.raises(ValueError):
            c.atom_depth(x, x, x, x, n_points=n)
        with pytest.raises(ValueError):
            c.atom_depth_batch(x, x, x, x, None, [0, 5], n_points=n)
    with pytest.raises(ValueError):
        c.atom_depth_batch(x, x, x, x, None, [0, 2, 4])            # offsets cover 4 of 5 atoms


def test_residue_depth_on_a_hand_case():
    import rustsasa_amd
    d = np.array([1.0, 2.0, 4.0, 0.5, 3.5, np.inf], F)
    got = rustsasa_amd.residue_depth(d, [0, 2, 2, 5, 6])
    assert got.dtype == np.float64 and got.shape == (4,)
    assert got[0] == 1.5 and np.isnan(got[1]) and got[2] == (4.0 + 0.5 + 3.5) / 3.0 and got[3] == np.inf
    assert rustsasa_amd.residue_depth(d, [0]).shape == (0,)
    assert rustsasa_amd.residue_depth(d[:0], [0, 0]).tolist() != [0.0]     # (an empty residue is NaN, never 0)
    # float64 sums of float32 depths: 0.1f + 0.2f is not rounded to float32
    two = np.array([0.1, 0.2], F)
    assert rustsasa_amd.residue_depth(two, [0, 2])[0] == (float(two[0]) + float(two[1])) / 2.0
    for bad in ([0, 7], [2, 1], [0.0, 2.0]):
        with pytest.raises(ValueError):
            rustsasa_amd.residue_depth(d, bad)


# ---- the model -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_points", [1, 33, 100, 960])
def test_lone_sphere(n_points):
    """One atom: every point accessible, depth = sqrtf(min d2) over its own dots, within 2 ulp of R."""
    x, y, z, r = (np.array([v], F) for v in (11.25, -3.5, 7.125, 1.76))
    mask = np.ones((1, n_points), bool)
    keys = dm.keys_of(x, y, z, r, mask, 1.4, n_points)
    bits, depth, nearest = dm.split(keys)
    owner, qx, qy, qz = dm.dots_of(x, y, z, r, mask, 1.4, n_points)
    d2 = (x[0] - qx) * (x[0] - qx) + (y[0] - qy) * (y[0] - qy) + (z[0] - qz) * (z[0] - qz)
    assert d2.dtype == F and depth[0] == np.sqrt(d2.min()) and nearest[0] == 0 and bits[0] == dm.bits(d2.min())
    R = F(1.76) + F(1.4)
    # the dots lie on the sphere up to the rounding of coordinates of size 11 (ulp 2^-20 there, R's is 2^-22)
    assert abs(float(depth[0]) - float(R)) <= 2.0 * 2.0 ** -20
    assert abs(float(np.sqrt(F(R * R))) - float(R)) <= 2.0 * float(np.spacing(R))
    # at the origin nothing but the lattice's own rounding is left: within 2 ulp of R
    zero = np.zeros(1, F)
    d0 = dm.split(dm.keys_of(zero, zero, zero, r, mask, 1.4, n_points))[1][0]
    assert abs(float(d0) - float(R)) <= 2.0 * float(np.spacing(R))


def test_model_agrees_with_a_float64_search_over_surface_points(models):
    import rustsasa_amd
    c = dc.get("ball")
    depth, nearest, mask = models["ball"]
    atom, xyz = rustsasa_amd.surface_points(pm.pack(mask), *c.cols[:4], c.probe, N_POINTS)
    own, qx, qy, qz = dm.dots_of(*c.cols[:4], mask, c.probe, N_POINTS)
    assert np.array_equal(atom, own.astype(np.uint32)) and np.array_equal(xyz, np.stack([qx, qy, qz], -1))   # the same dots
    ctr = np.stack(c.cols[:3], -1).astype(np.float64)
    q = xyz.astype(np.float64)
    want = np.array([np.sqrt(((q - ctr[i]) ** 2).sum(axis=1).min()) for i in range(len(ctr))])
    assert np.all(np.abs(depth.astype(np.float64) - want) <= 1e-5 * want)
    # (the owner of the float64 minimum may differ at near ties; where the gap is clear it is the same atom)
    assert np.isfinite(depth).all() and (nearest < c.n_atoms).all()


def test_model_without_dots_and_with_nan():
    x = np.array([0.0, 1.0, np.nan], F)
    o = np.zeros(3, F)
    r = np.array([1.5, 1.5, 1.5], F)
    none = np.zeros((3, 10), bool)
    _, depth, nearest = dm.split(dm.keys_of(x, o, o, r, none, 1.4, 10))
    assert np.isinf(depth).all() and (nearest == 0xFFFFFFFF).all()
    some = none.copy()
    some[2] = True            # the NaN atom's dots have NaN d2: they count for nobody
    some[1, 3] = True
    _, depth, nearest = dm.split(dm.keys_of(x, o, o, r, some, 1.4, 10))
    assert nearest.tolist() == [1, 1, 0xFFFFFFFF] and np.isinf(depth[2]) and np.isfinite(depth[:2]).all()


# ---- the cases are what they are named for ---------------------------------------------------------------------------

def test_ball_and_cavity_hold_every_depth_class(models):
    """Depths in (0, 1], (1, 2], (2, 3] and above 3 cell sizes: sweeps that stop at shells 3, 4, 5 and later."""
    seen = np.zeros(4, np.int64)
    for name in ("ball", "cavity"):
        c = dc.get(name)
        h, dims, cells = dc.grid_cells(*c.cols[:4], c.probe)
        t = models[name][0] / h
        seen += np.histogram(t, [0.0, 1.0, 2.0, 3.0, np.inf])[0]
        assert 850 <= c.n_atoms <= 950
    assert (seen >= 20).all(), seen
    # the ball's deepest atoms are out of reach of the 5x5x5 block: more than 2 cells + a dot's radius away
    c = dc.get("ball")
    h, _, _ = dc.grid_cells(*c.cols[:4], c.probe)
    assert int((models["ball"][0] > 3.0 * h).sum()) >= 20
    assert not models["ball"][2][models["ball"][0] > 2.0 * h].any()       # and they have no point of their own


def test_cavity_holds_dots_that_are_the_nearest_of_their_surroundings(models):
    c = dc.get("cavity")
    depth, nearest, mask = models["cavity"]
    rim = c.info["rim"]
    xyz = np.stack(c.cols[:3], -1).astype(np.float64)
    assert np.linalg.norm(xyz - dc.VOID_CENTRE, axis=1).min() > dc.VOID_RADIUS
    assert 4.0 < np.linalg.norm(dc.VOID_CENTRE) < dc.BALL_RADIUS - 2.0 * dc.VOID_RADIUS + 1.0   # off centre, well inside
    wall = rim[mask[rim].any(axis=1)]
    assert len(wall) >= 5                                       # the void holds accessible dots
    served = np.flatnonzero(np.isin(nearest, wall))
    assert len(served) >= 10
    # ... and those atoms are nearer to the void's dots than the same atoms of the solid ball are to any dot
    others = np.setdiff1d(served, wall)
    assert len(others) >= 10 and not mask[others].any()
    # the outer surface is further: the dots of the atoms outside the rim
    outer = mask.copy()
    outer[rim] = False
    _, d_outer, _ = dm.split(dm.keys_of(*c.cols[:4], outer, c.probe, N_POINTS, sample=others))
    assert np.all(depth[others] < d_outer)


def test_twins_hold_exact_ties(models):
    c = dc.get("twins")
    depth, nearest, mask = models["twins"]
    assert np.array_equal(mask[1], mask[2]) and mask[1].any() and c.ids[1] == c.ids[2]
    assert not mask[0].any()                                    # the atom inside them is buried
    for i in range(c.n_atoms):
        k1 = dm.keys_of(*c.cols[:4], mask & (np.arange(4) == 1)[:, None], c.probe, N_POINTS, sample=[i])[0]
        k2 = dm.keys_of(*c.cols[:4], mask & (np.arange(4) == 2)[:, None], c.probe, N_POINTS, sample=[i])[0]
        assert k1 >> np.uint64(32) == k2 >> np.uint64(32)       # the same d2 bits from both twins
    assert nearest[0] == 1 and nearest[1] == 1 and nearest[2] == 1 and nearest[3] == 3
    assert dm.bits(depth)[1] == dm.bits(depth)[2]


def test_corner_sweeps_clip_at_every_face(models):
    """The grid reaches one cell below the smallest coordinate and two above the largest, so an atom's cell coordinate
    lies in [0, dim - 3]: the outermost layers an atom can be in are 0 / 1 and dim - 3.  Every atom of the case is in such
    a layer of some axis, some in three, and the shells of every sweep (at least 3, the stop rule's earliest) cross a face, and
    every one of the six faces is crossed by some sweep."""
    c = dc.get("corner")
    h, dims, cells = dc.grid_cells(*c.cols[:4], c.probe)
    assert (cells >= 0).all() and (cells <= dims - 3).all()
    low, high = cells <= 1, cells >= dims - 3
    assert (low | high).any(axis=1).all()
    assert int((low | high).all(axis=1).sum()) >= 8             # corner cells
    below, above = cells - 3 < 0, cells + 3 > dims - 1
    assert (below | above).any(axis=1).all() and below.any(axis=0).all() and above.any(axis=0).all()
    assert float(models["corner"][0].min()) > 0.0 and (models["corner"][0] <= 2.0 * h).all()


def test_tiny_and_overlap_batch(models):
    c = dc.get("tiny")
    assert np.diff(c.so.astype(np.int64)).tolist() == [1, 0, 2, 0, 3]
    depth, nearest, mask = models["tiny"]
    assert nearest[0] == 0 and mask[0].all()
    o = dc.get("overlap_batch")
    b = dc.get("ball")
    assert np.diff(o.so.astype(np.int64)).tolist() == [b.n_atoms, 1]
    assert models["overlap_batch"][0][:-1].tobytes() == models["ball"][0].tobytes()
    # had the lone atom's dots counted, the ball's centre would be a radius away from them
    lone_R = float(o.r[-1]) + o.probe
    centre = np.flatnonzero(np.linalg.norm(np.stack(b.cols[:3], -1), axis=1) < 1.0)
    assert len(centre) >= 1 and (models["ball"][0][centre] > 2.0 * lone_R).all()


def test_tail_case_layout():
    c = dc.get("tail")
    sizes = np.diff(c.so.astype(np.int64))
    assert sizes[-1] >= 65536 and (sizes[:-1] < 65536).all() and len(sizes) >= 4
