"""The order in which the neighbour-list and point-run entry points (rustsasa_amd/csrc/neighbors.cpp) give their
verdicts: every call here breaks two rules at once and must be answered with the earlier rule's message.  The order is
resolve_ctx, the structure offsets (batch forms), n_points (point families), the columns and required outputs, then the
family's own rules - k before cutoff for the nearest atoms; n_classes, n_bins, the edges, then the class bytes for the
radial counts; n_dirs before reach for the dot enclosure.  All 14 families, single and batch form, through the C ABI
(_capi) on one context.  No call passes its rules, so no kernel is launched."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 3
NAN = float("nan")
OFFSETS = "structure_offsets[0] must be 0"
POINTS = "n_points must be in [1, 2^31 - 1)"
NULL = "NULL argument"


@pytest.fixture(scope="module")
def ctx():
    import rustsasa_amd
    c = rustsasa_amd.Context(0)
    yield c
    c.close()


class Args:
    """The arguments of one call, by name; `tail` of a family turns them into the C argument list behind probe_radius."""

    def __init__(self):
        from rustsasa_amd._capi import ptr
        f32, u32, u64 = np.float32, np.uint32, np.uint64
        self.keep = dict(x=np.array([0.0, 1.5, 3.0], f32), y=np.zeros(N, f32), z=np.zeros(N, f32), r=np.full(N, 1.7, f32),
                         group=np.zeros(N, u32), so=np.array([0, N], u32), bad_so=np.array([1, 2], u32),
                         edges=np.array([4.0, 8.0], f32), falling=np.array([8.0, 4.0], f32),
                         classes=np.array([0, 1, 0], np.uint8), high_class=np.array([0, 2, 0], np.uint8),
                         active=np.array([0, 5], u32))
        self.outs = dict(o64=np.zeros(64, u64), f32a=np.zeros(4096, f32), **{"o32" + c: np.zeros(4096, u32) for c in "abcde"})
        p = {k: ptr(v) for k, v in {**self.keep, **self.outs}.items()}
        self.p = p
        self.v = dict(x=p["x"], y=p["y"], z=p["z"], r=p["r"], id=None, group=p["group"], so=p["so"], n_points=100,
                      link=1.0, cutoff=8.0, k=2, flags=None, dirs=None, classes=p["classes"], n_classes=2, edges=p["edges"],
                      n_bins=2, reach=10.0, n_dirs=30, active=None, n_active=0, out_offsets=p["o64"], out_a=p["o32a"],
                      out_b=p["o32b"], out_c=p["o32c"], out_d=p["o32d"], out_e=p["o32e"], out_f=p["f32a"], cap=16)

    def but(self, **changes):
        v = dict(self.v)
        for k, val in changes.items():
            v[k] = self.p[val] if isinstance(val, str) else val
        return v


# family: (symbol stem, point family?, the required outputs a NULL stands for, bad family argument or None,
#          the arguments behind probe_radius)
FAMILIES = {
    "neighbors": ("rsasa_precompute_neighbors", False, "out_offsets", None,
                  lambda v: (NAN, v["out_offsets"], v["out_a"], v["cap"])),
    "points": ("rsasa_accessible_points", True, "out_a", None, lambda v: (v["n_points"], v["out_a"], v["out_f"])),
    "exposure": ("rsasa_exposure_vectors", True, "out_f", None, lambda v: (v["n_points"], v["out_f"], v["out_a"], None)),
    "depth": ("rsasa_atom_depth", True, "out_f", None, lambda v: (v["n_points"], v["out_f"], v["out_a"], v["out_b"], None)),
    "components": ("rsasa_surface_components", True, "out_offsets", dict(link=NAN),
                   lambda v: (v["n_points"], v["link"], v["out_offsets"], v["out_a"], v["cap"], v["out_b"], None)),
    "crowding": ("rsasa_dot_crowding", True, "out_offsets", dict(n_bins=0),
                 lambda v: (v["n_points"], v["flags"], v["edges"], v["n_bins"], v["out_offsets"], v["out_a"], v["cap"],
                            v["out_b"], None)),
    "enclosure": ("rsasa_dot_enclosure", True, "out_offsets", dict(n_dirs=0),
                  lambda v: (v["n_points"], v["flags"], v["reach"], v["n_dirs"], v["out_offsets"], v["out_a"], v["cap"],
                             v["out_b"], None)),
    "hse": ("rsasa_half_sphere_exposure", False, "out_a", dict(cutoff=-1.0),
            lambda v: (v["dirs"], v["flags"], v["cutoff"], v["out_a"], v["out_b"])),
    "within": ("rsasa_atoms_within", False, "out_offsets", dict(cutoff=-1.0),
               lambda v: (v["flags"], v["cutoff"], 0, v["out_offsets"], v["out_a"], v["cap"])),
    "nearest": ("rsasa_nearest_atoms", False, "out_offsets", dict(k=0),
                lambda v: (v["flags"], v["k"], v["cutoff"], v["out_offsets"], v["out_a"], v["cap"])),
    "radial": ("rsasa_radial_counts", False, ("out_a", "out_offsets"), dict(n_classes=0),
               lambda v: (v["flags"], v["classes"], v["n_classes"], v["edges"], v["n_bins"], v["out_a"], v["out_offsets"])),
    "contacts": ("rsasa_contact_points", True, "out_offsets", None,
                 lambda v: (v["n_points"], v["out_offsets"], v["out_a"], v["out_b"], v["out_c"], v["cap"], None)),
    "owners": ("rsasa_contact_owners", True, "out_offsets", None,
               lambda v: (v["n_points"], v["out_offsets"], v["out_a"], v["out_b"], v["cap"], None, None)),
    "groups": ("rsasa_group_contacts", True, "out_offsets", None,
               lambda v: (v["n_points"], v["out_offsets"], v["out_a"], v["out_b"], v["out_c"], v["cap"], v["out_d"],
                          v["out_e"], None)),
}


def _call(lib, h, family, batch, v):
    stem, _, _, _, tail = FAMILIES[family]
    cols = (v["x"], v["y"], v["z"], v["r"], v["id"]) + ((v["group"],) if family == "groups" else ())
    if batch:
        return getattr(lib, stem + "_batch")(h, *cols, v["so"], 1, 1.4, *tail(v))
    if family == "neighbors":
        return getattr(lib, stem)(h, *cols, N, v["active"], v["n_active"], 1.4, *tail(v))
    return getattr(lib, stem)(h, *cols, N, 1.4, *tail(v))


def _null_output(family):
    out = FAMILIES[family][2]
    return {k: None for k in ((out,) if isinstance(out, str) else out)}


def _pairs(family, batch):
    """(what, changed arguments, the earlier rule's message) of every two-rule call of a family's form."""
    _, point, _, bad, _ = FAMILIES[family]
    out = _null_output(family)
    pairs = []
    if batch:
        if point:
            pairs.append(("offsets before n_points", dict(so="bad_so", n_points=0), OFFSETS))
        pairs.append(("offsets before a NULL output", dict(so="bad_so", **out), OFFSETS))
        if bad:
            pairs.append(("offsets before the family's rule", dict(so="bad_so", **bad), OFFSETS))
    if point:
        pairs.append(("n_points before a NULL column", dict(n_points=0, y=None), POINTS))
    if bad:
        pairs.append(("a NULL output before the family's rule", dict(**out, **bad), NULL))
    if family == "neighbors" and not batch:
        pairs.append(("a NULL output before the active indices", dict(active="active", n_active=2, **out), NULL))
    if family == "nearest":
        pairs.append(("k before cutoff", dict(k=0, cutoff=NAN), "k must be in [1, 256]"))
    if family == "enclosure":
        pairs.append(("n_dirs before reach", dict(n_dirs=0, reach=NAN), "n_dirs must be in [1, 32]"))
    if family == "radial":
        pairs.append(("n_classes before n_bins", dict(n_classes=0, n_bins=0), "n_classes must be in [1, 16]"))
        pairs.append(("edges before classes", dict(classes="high_class", edges="falling"), "edges must be non-decreasing"))
    return pairs


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_earlier_rule_answers(ctx, family, batch):
    from rustsasa_amd import _capi
    lib = _capi.load()
    args = Args()
    pairs = _pairs(family, batch)
    assert pairs, (family, batch)
    for what, changes, message in pairs:
        rc = _call(lib, ctx._h, family, batch, args.but(**changes))
        got = lib.rsasa_context_last_error(ctx._h).decode()
        assert rc == _capi.RSASA_ERR_INVALID_ARGUMENT and got == message, (family, batch, what, rc, got)
    assert not any(a.any() for a in args.outs.values())  # nothing was written


def test_every_family_and_form_is_covered():
    from rustsasa_amd import _capi
    stems = {FAMILIES[f][0] for f in FAMILIES}
    entry = {s for s in _capi.SYMBOLS if s in stems or (s.endswith("_batch") and s[:-6] in stems)}
    assert len(FAMILIES) == 14 and len(entry) == 28
