"""The inputs of the second dot-crowding / dot-enclosure suites (test_dot_edges_cpu.py, test_gpu_dot_edges.py), each named
for what it reaches in the frame that k_dot_crowding (crowding.hip) and k_dot_enclosure (enclosure.hip) share and no other
kernel has: the mask compacted into LDS by rank, 64 words a trip; passes of 128 dots; a pass of 32 dots or fewer spread
over P lanes with G = 64 / P groups that share the staged atoms out and meet again by shuffles; the stop rules at their
clamps; the enclosure's cuts at coordinates of 65536 h.  The CPU file pins every case to what it is named for from the
models alone, the GPU file compares the kernels with the models.  Plain helper module (not a conftest)."""
import functools

import numpy as np

import crowding_cases as cc
import depth_cases as dc
import enclosure_cases as ec
import enclosure_model as em
import points_model as pm
import sweep_cases as sc
import sweep_model as sm

F = np.float32
WAVE = sm.WAVE
PASS = cc.PASS      # kDcPass = kDePass
TWO = "two"         # a pass of more than 64 dots: two dots a lane


# ---- the classes of a pass -------------------------------------------------------------------------------------------------

LANES = (1, 2, 4, 8, 16, 32, 64, TWO)
CLASSES = tuple((later, P) for later in (False, True) for P in LANES)


def lanes_of(n_pass):
    """P of a pass of n_pass dots, as both kernels choose it: the power of two >= n_pass up to 32 dots, 64 lanes up to
    64 dots, two dots a lane beyond."""
    assert 1 <= n_pass <= PASS
    if n_pass > WAVE:
        return TWO
    if n_pass > WAVE // 2:
        return WAVE
    P = 1
    while P < n_pass:
        P <<= 1
    return P


def groups_of(P):
    return 1 if P == TWO else WAVE // P


def passes_of(n_free):
    """[(later pass?, P)] of the passes of an atom with n_free accessible points."""
    return [(lo > 0, lanes_of(min(int(n_free) - lo, PASS))) for lo in range(0, int(n_free), PASS)]


def pass_classes(free):
    """The set of (later pass?, P) over the atoms with the free counts `free`."""
    return {c for n in np.asarray(free).ravel() for c in passes_of(n)}


# ---- A: lattices past 2048 points --------------------------------------------------------------------------------------------

BIG = (("lone", 2049), ("pair", 2049), ("pair", 4097))   # 65 words: two trips, the second of one bit; 129 words: three
TRIP_POINTS = WAVE * 32                                  # the points of one trip over the mask's words


@functools.lru_cache(maxsize=None)
def big(name, n_points):
    return getattr(cc, name)(n_points)


# ---- B: every class of pass, with obstacles that make the split matter ------------------------------------------------------

SPLIT_POINTS = 200
SPLIT_OWNER = (np.array([3.25, -1.5, 7.75]), 1.5)       # R = 2.9
SPLIT_COVER_RADIUS = 3.0                                # R = 4.4 = h
SPLIT_FIRST = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65)
SPLIT_LATER = tuple(PASS + t for t in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65))
SPLIT_CLUSTERS = (3, 50, 70)
SPLIT_CUBE = 1.2
SPLIT_AWAY = 7.5        # the cluster's centre from the owner's, along the free cap's axis
SPLIT_EDGES = (4.0, 6.0, 9.0)
SPLIT_REACH = 10.0


def _cap_axis():
    from oracle import pyoracle as po
    s = np.stack([np.asarray(a, F) for a in po.sphere_points(SPLIT_POINTS)], -1).astype(np.float64)
    return s[-1] / np.linalg.norm(s[-1])


def _split_pair(d):
    """The owner and a larger atom d away from it, opposite the last lattice point (crowding_cases._cap_pair at 200
    points)."""
    c, r = SPLIT_OWNER
    return np.array([c, np.round(c - _cap_axis() * d, 3)]), np.array([r, SPLIT_COVER_RADIUS])


@functools.lru_cache(maxsize=None)
def split_distances():
    """{free count of the owner: a distance that gives it}, scanned on a grid of 0.002 A with the points model."""
    out = {}
    for d in np.arange(7.4, 1.0, -0.002):
        xyz, r = _split_pair(float(d))
        m = pm.exposed_masks(*(xyz[:, k].astype(F) for k in range(3)), r.astype(F), None, cc.PROBE, SPLIT_POINTS, 8)
        out.setdefault(int(m[0].sum()), float(d))
    return out


def _class_of_count(n):
    return passes_of(n)[-1]


@functools.lru_cache(maxsize=None)
def split_counts():
    """The owners' free counts: every target of SPLIT_FIRST and SPLIT_LATER, or where the scan skips it the nearest
    count it gives whose last pass has the same class."""
    have = split_distances()
    out = []
    for t in SPLIT_FIRST + SPLIT_LATER:
        same = [n for n in have if n and _class_of_count(n) == _class_of_count(t)]
        assert same, ("no count of the class of", t)
        out.append(min(same, key=lambda n: (abs(n - t), n)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def split(n_cluster):
    """One structure per count of split_counts(): the owner (atom 0, flagged), the cover (atom 1; flagged beside the
    clusters of 50 and 70, which it joins in one staging step - 51 and 64 + 7 -, not beside the cluster of 3) and a cluster
    of n_cluster flagged atoms packed into a cube of 1.2 A, SPLIT_AWAY out from the owner over its free cap - further
    than R_i + R_j from the owner, so it buries none of the owner's points, and within the reach and the edges of every
    dot of the cap.  Garbage in flag bits 1 to 7.  info: owners (batch indices), free (their counts)."""
    rng = np.random.default_rng(300 + n_cluster)
    dist = split_distances()
    axis = _cap_axis()
    parts, owners, at = [], [], 0
    for n in split_counts():
        xyz, r = _split_pair(dist[n])
        cube = np.round(SPLIT_OWNER[0] + axis * SPLIT_AWAY + rng.uniform(-SPLIT_CUBE / 2, SPLIT_CUBE / 2, (n_cluster, 3)), 3)
        parts.append((np.concatenate([xyz, cube]), np.concatenate([r, rng.choice(dc.RADII, n_cluster)])))
        owners.append(at)
        at += 2 + n_cluster
    flags = ((rng.integers(0, 128, at) << 1) | 1).astype(np.uint8)
    if n_cluster == SPLIT_CLUSTERS[0]:
        flags[np.asarray(owners) + 1] &= 0xFE
    c = cc._case("split_%d" % n_cluster, parts, n_points=SPLIT_POINTS, edges=SPLIT_EDGES, flags=flags,
                 info=dict(owners=owners, free=list(split_counts())))
    return c


def staged_batches(c, s, owner=0, drop_owner=False):
    """[n_staged] of every staging batch that the wave of atom `owner` of structure s of the case meets, shell by shell
    over the whole grid, step by step, 64 atoms of a step's runs at a time: the atoms with the partner bit (k_dot_crowding)
    and, with drop_owner, without the owner itself (k_dot_enclosure, whose staging cut must let every atom pass: see
    test_dot_edges_cpu.py).  Batches that stage nobody are left out, as the kernels leave them."""
    b, e = int(c.so[s]), int(c.so[s + 1])
    g = sm.grid(c.x[b:e], c.y[b:e], c.z[b:e], c.r[b:e], c.probe)
    fl = np.ones(e - b, np.uint8) if c.flags is None else c.flags[b:e]
    out = []
    for shell in range(g.s_last(owner) + 1):
        for flat in sm.shell_steps(g, owner, shell)[0]:
            for a in range(0, len(flat), WAVE):
                j = g.order[flat[a:a + WAVE]]
                keep = (fl[j] & 1) != 0
                if drop_owner:
                    keep &= j != owner
                if keep.any():
                    out.append(int(keep.sum()))
    return out


# ---- C: the stop rules at their boundaries -----------------------------------------------------------------------------------

REACH_SHELLS = (3, 4, 5, 6, 7)


def reach_of(h, shells):
    """A reach that k_dot_enclosure's rule admits after `shells` shells and not sooner: (shells - 2.5) h in float32."""
    return float(max(F(shells) - F(2.5), F(0.0)) * F(h))


def boundary_reaches(h=sc.H):
    """[(shells, on the boundary?, reach)]: reach_of(h, s) and the float above it for s = 3 .. 7."""
    out = []
    for s in REACH_SHELLS:
        L = reach_of(h, s)
        out += [(s, True, L), (s, False, float(np.nextafter(F(L), F(np.inf))))]
    return out


@functools.lru_cache(maxsize=None)
def boundary_case(reach):
    return ec.of_depth("cavity", n_points=20, reach=reach)


def rank_of(mask_row, k):
    """The rank of lattice point k among an atom's accessible points."""
    assert mask_row[k]
    return int(mask_row[:k].sum())


# ---- D: the cuts and the ties at coordinates of 65536 h ----------------------------------------------------------------------

MARGIN_MOVES = ((0, 1), (2, -1))      # (axis, sign): +x and -z


def moved_structures(c, axis, sign):
    """[(xyz float32 [n, 3], r)] of the structures of a case, each translated in float32 along the axis to just under
    the margins' limit (sweep_cases._edge_shift: one coordinate step further and sh_margins_hold fails)."""
    parts = []
    for s in range(len(c.so) - 1):
        b, e = int(c.so[s]), int(c.so[s + 1])
        xyz = np.stack([c.x[b:e], c.y[b:e], c.z[b:e]], -1)
        under, _ = sc._edge_shift(xyz, c.r[b:e], c.probe, axis, sign)
        parts.append((sc._moved(xyz, axis, sign, under), c.r[b:e]))
    return parts


MOVED = ("prefilter_edge", "last_shell", "last_shell_3")


@functools.lru_cache(maxsize=None)
def moved_enclosure(name, axis, sign):
    """enclosure_cases.prefilter_edge() / last_shell() / last_shell(3) on a grid translated to just under the margins'
    limit: coordinates of about 131072 = 65536 h, whose ulp is h / 128 or h / 256.  The ties are no longer exact - the
    model decides."""
    c = {"prefilter_edge": ec.prefilter_edge, "last_shell": ec.last_shell, "last_shell_3": lambda: ec.last_shell(3)}[name]()
    return ec._case("%s_moved_%s%s" % (name, "+" if sign > 0 else "-", "xyz"[axis]), moved_structures(c, axis, sign),
                    n_points=c.n_points, n_dirs=c.n_dirs, reach=c.reach, probe=c.probe, info=c.info)


@functools.lru_cache(maxsize=None)
def moved_tie(kind, axis, sign):
    """crowding_cases.tie("last") / tie("below") with the owner translated to just under the margins' limit and the
    partner and the edge rebuilt from the moved float32 dot, as tie_geometry builds them: the tie is exact again."""
    xyz, r, _, _ = cc.tie_geometry()
    h = float(F(cc.PROBE) + np.max(r))
    under, _ = sc._edge_shift(xyz, r, cc.PROBE, axis, sign)
    step = float(np.spacing(F(65536.0 * h)))
    for back in range(8):          # the rebuilt partner may lie a step further out than the translated one
        centre = sc._moved(xyz[:1], axis, sign, under - back * step)[0]
        xyz_m, r_m, _, e = cc.tie_geometry(centre=centre)
        if sm.margins_hold(*xyz_m.T, r_m, cc.PROBE):
            break
    else:
        raise AssertionError("no translation under the margins")
    edges = {"last": (3.2, float(e)), "below": (3.2, float(np.nextafter(e, F(0.0))))}[kind]
    return cc._case("tie_%s_moved_%s%s" % (kind, "+" if sign > 0 else "-", "xyz"[axis]), [(xyz_m, r_m)], n_points=cc.TIE_POINTS,
                    edges=edges, info=dict(owner=0, partner=1, dot=cc.TIE_DOT, centre=centre, back=back))


# ---- D: the case only the staging cut's absolute h / 64 keeps -----------------------------------------------------------------

ABS_SEEDS = tuple(range(500, 540))
ABS_SEED = 514        # the first of them that abs_search() finds (test_dot_edges_cpu.py pins it)
ABS_POINTS = 20
ABS_DIRS = 30


def abs_candidate(seed):
    """A seeded structure under the margins, at coordinates of 65536 h along z, whose reach is h / 2: an owner, an
    obstacle of the largest radius (R_j = h) straight above the owner's point 0 - which is (0, 0, 1), as is direction 0 -
    with its centre R_i + L + R_j and up to 0.007 h more from the owner's, and two bystanders that fix the grid.  There
    (L + R_i + R_j) 2^-10 is about 0.0024 h, and the rounding of the dot's z, half an ulp of 65536 h, up to h / 256."""
    rng = np.random.default_rng(seed)
    probe = 1.4
    r_max = F(rng.uniform(0.65, 1.1))
    h = F(probe) + r_max
    L = F(0.5) * h
    r_i = F(rng.uniform(0.3, float(r_max)))
    z0 = float(rng.uniform(131200.0, 65536.0 * float(h) - 60.0))
    ci = np.array([3.0, -2.0, z0], F)
    Ri = float(r_i + F(probe))
    gap = rng.uniform(0.0, 0.007) * float(h)
    cj = np.array([3.0, -2.0, float(ci[2]) + Ri + float(L) + float(h) + gap], F)
    low = np.array([3.0 + rng.uniform(-2, 2), -2.0 + rng.uniform(-2, 2), float(ci[2]) - 3.2 * float(h)], F)
    side = np.array([3.0 + 3.5 * float(h), -2.0, float(ci[2]) + rng.uniform(-1, 1)], F)
    xyz = np.stack([ci, cj, low, side])
    r = np.array([r_i, r_max, F(rng.uniform(0.3, float(r_max))), F(rng.uniform(0.3, float(r_max)))], F)
    return ec._case("abs_term_%d" % seed, [(xyz, r)], n_points=ABS_POINTS, n_dirs=ABS_DIRS, reach=float(L), probe=probe,
                    info=dict(owner=0, obstacle=1, seed=seed))


def abs_lost(c):
    """(words of the owner's dots from the model, from the emulated sweep, from the sweep without the h / 64) or None
    when the structure fails the margins."""
    x, y, z, r = c.x, c.y, c.z, c.r
    if not sm.margins_hold(x, y, z, r, c.probe):
        return None
    mask = ec.masks(c)
    off, words = em.blocked(x, y, z, r, mask, c.probe, c.n_points, c.n_dirs, c.reach)
    own = np.array([c.info["owner"]])
    want = words[int(off[own[0]]):int(off[own[0] + 1])]
    full = em.sweep_blocked(x, y, z, r, mask, c.probe, c.n_points, c.n_dirs, c.reach, None, own)[0][0]
    bare = em.sweep_blocked(x, y, z, r, mask, c.probe, c.n_points, c.n_dirs, c.reach, None, own, abs_term=False)[0][0]
    return want, full, bare


@functools.lru_cache(maxsize=None)
def abs_search():
    """The first seed of ABS_SEEDS whose structure loses a bit of the model without the h / 64, or None."""
    for seed in ABS_SEEDS:
        got = abs_lost(abs_candidate(seed))
        if got is not None and (got[0] & ~got[2]).any():
            return seed
    return None
