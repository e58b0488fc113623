"""The oracle at the edges of its decisions (CPU): exact dot == limit ties of the fused and the remainder rule,
patch rims, k_occlusion_mx's admission range, candidate cutoffs and colliding id folds (tests/tie_cases.py), against
an independent restatement of the reference's decision; and k_occlusion_mx's three-operation quotient against
IEEE division."""
import numpy as np
import pytest

import tie_cases as tc

WIDTHS = (1, 4, 8, 16)


@pytest.fixture(scope="module")
def cases():
    return tc.all_cases()


def test_generator_reaches_its_minimums():
    rep = tc.report()
    m = tc.MINIMUM
    assert rep["fused_ties"] >= m["fused_ties"], rep
    assert rep["remainder_ties"] >= m["remainder_ties"], rep
    assert rep["patch"] >= m["patch"], rep
    assert rep["cutoff"] >= m["cutoff"], rep
    assert rep["cutoff_exact"] >= m["cutoff_exact"], rep
    assert rep["fold"] >= m["fold"], rep
    assert rep["f16_subnormal_v"] >= m["f16_subnormal_v"], rep
    edges = [k for k in rep if k.startswith("range_")]
    assert len(edges) >= 10, edges
    for k in edges:
        assert rep[k] >= m["range_edge"], (k, rep[k])


# k_occlusion_mx's admission of the watched atom per edge: inside each bound, and one f32 step beyond it.  (No atom
# of a structure with a radius of 64 can be admitted: sr <= 64 would need r = probe = 0, and then R < 0.5.)
ADMITTED = {"probe0": True, "probe32": True, "probe32_plus": False, "R_half": True, "R_half_minus": False,
            "sr64": True, "sr64_plus": False, "radius64": False, "radius64_plus": False, "large_limit_diag": True}


def test_range_edges_sit_on_the_side_of_the_bound_they_name():
    fam = tc.generate()["range"]
    assert set(fam) == set(ADMITTED)
    for edge, lst in fam.items():
        for c in lst:
            for st in c.structures:
                assert tc.mx_admits(st, c.probe, 0) == ADMITTED[edge], (edge, c.meta)
    # the exact bounds themselves: probe 32 with radii 0 is sr = 64, R_half is R = 0.5, sr64 is sr = 64
    f32 = np.float32
    for c in fam["probe32"]:
        assert c.probe == 32.0 and not np.any(c.structures[0].r)
    for c in fam["R_half"]:
        assert c.structures[0].r[0] + f32(c.probe) == f32(0.5)
    for c in fam["sr64"]:
        st = c.structures[0]
        assert st.r[0] + np.max(st.r) + f32(2.0) * f32(c.probe) == f32(64.0)
    for c in fam["sr64_plus"]:
        st = c.structures[0]
        assert st.r[0] + np.max(st.r) + f32(2.0) * f32(c.probe) == tc.ulps(64.0, 1)


def test_cutoff_cases_sit_on_the_cutoff():
    """Exact cutoff cases: d^2 == sr^2 in f32 on the inside side, the neighbour a candidate there and not one f32
    step further out."""
    for c in tc.generate()["cutoff"]:
        if c.family != "cutoff" or not c.tie:
            continue
        st_in, st_out = c.structures[0], c.structures[1]
        assert 1 in tc.candidates(st_in, c.probe)[0] and 1 not in tc.candidates(st_out, c.probe)[0]


def test_ties_are_exact():
    """A tie case's flip side has dot == limit bit for bit (the model's own arithmetic), and its neighbour is a
    candidate of the atom."""
    fam = tc.generate()
    for c in fam["fused"] + fam["remainder"]:
        if not c.tie:
            continue
        assert c.meta["dot"] == c.meta["limit"], c.meta
        for st in c.structures[:2]:
            assert 1 in tc.candidates(st, c.probe)[0]


def test_oracle_matches_the_model_on_every_case(cases):
    """Exposed-point counts and neighbour counts K of every atom of every variant, at the case's lane count."""
    bad = []
    for c in cases:
        for v, st in enumerate(c.structures):
            m, mk = tc.model_counts(st, c.probe, c.n_points, c.W)
            _, p, k = tc.oracle_counts(st, c.probe, c.n_points, c.W)
            if not (np.array_equal(m, p) and np.array_equal(mk, k)):
                bad.append((c.family, c.edge or c.label, v, m.tolist(), p.tolist(), mk.tolist(), k.tolist()))
    assert not bad, (len(bad), bad[:5])


def test_oracle_matches_the_model_at_every_lane_count(cases):
    """The two sides of every flip with W = 1, 4, 8 and 16: which points take the remainder rule changes with W."""
    bad = []
    for c in cases:
        for st in c.structures[:2]:
            for W in WIDTHS:
                m, mk = tc.model_counts(st, c.probe, c.n_points, W)
                _, p, k = tc.oracle_counts(st, c.probe, c.n_points, W)
                if not (np.array_equal(m, p) and np.array_equal(mk, k)):
                    bad.append((c.family, c.edge or c.label, W, m.tolist(), p.tolist()))
    assert not bad, (len(bad), bad[:5])


def test_flip_changes_the_oracle_by_the_models_amount():
    """Across each tie the oracle's count of the watched atom drops, exactly as the model's does."""
    fam = tc.generate()
    for c in fam["fused"] + fam["remainder"] + fam["patch"]:
        lo, hi = c.structures[0], c.structures[1]
        m_lo, _ = tc.model_counts(lo, c.probe, c.n_points, c.W)
        m_hi, _ = tc.model_counts(hi, c.probe, c.n_points, c.W)
        p_lo = tc.oracle_counts(lo, c.probe, c.n_points, c.W)[1]
        p_hi = tc.oracle_counts(hi, c.probe, c.n_points, c.W)[1]
        assert m_lo[c.atom] > m_hi[c.atom], (c.family, c.meta)
        assert (p_lo[c.atom], p_hi[c.atom]) == (m_lo[c.atom], m_hi[c.atom]), (c.family, c.meta)


def test_fold_collisions_change_the_values():
    """Colliding folds are different ids: the oracle lets j occlude i; equal ids do not."""
    for c in tc.generate()["fold"]:
        hi, lo = c.meta["ids"]
        assert hi != lo and tc.fold_id(hi) == tc.fold_id(lo)
        vals = [tc.oracle_counts(st, c.probe, c.n_points, c.W)[0] for st in c.structures]
        assert vals[0][0] != vals[1][0]
        assert vals[0][0] == vals[2][0] == vals[3][0]


def test_vector_fmaf_is_the_libm_fmaf(cases):
    """The model's vectorised fmaf against the libm function on the operands of every tie point, and a seeded
    sample with operands of all magnitudes."""
    a, b, c = [], [], []
    for cs in cases:
        if "k" not in cs.meta:
            continue
        sx, sy, sz = tc.sphere(cs.n_points)
        k = cs.meta["k"]
        for st in cs.structures:
            vx, vy, vz, _ = tc.pair_terms(st.centre(0), st.r[0], st.centre(1), st.r[1], cs.probe)
            inner = sz[k] * vz
            a += [sy[k], sx[k]]
            b += [vy, vx]
            c += [inner, tc.fmaf(sy[k], vy, inner)]
    rng = np.random.default_rng(5)
    n = 20000
    a += list(rng.uniform(-1, 1, n).astype(np.float32))
    b += list((rng.uniform(-1, 1, n) * 2.0 ** rng.integers(-20, 7, n)).astype(np.float32))
    c += list((rng.uniform(-1, 1, n) * 2.0 ** rng.integers(-30, 7, n)).astype(np.float32))
    a, b, c = (np.array(t, np.float32) for t in (a, b, c))
    got = tc.fmaf_vec(a, b, c)
    want = np.array([tc.fmaf(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_three_operation_quotient_is_ieee_division(cases):
    """k_occlusion_mx's limit: over the numerator and divisor of every pair of every generated case, then a seeded
    sample of numerators (|a| in [2^-44, 2^16), both signs) against the divisors tools/check_division.c singles out -
    2R in [1, 128] with mantissas all ones, all zeros, one, all ones but one, protein radii plus probe, and random."""
    seen = set()
    for cs in cases:
        for st in cs.structures:
            for i in range(st.n):
                for j in tc.candidates(st, cs.probe)[i]:
                    p = np.float32(cs.probe)
                    R = st.r[i] + p
                    dx, dy, dz = st.x[i] - st.x[j], st.y[i] - st.y[j], st.z[i] - st.z[j]
                    d2 = dx * dx + dy * dy + dz * dz
                    tj = st.r[j] + p
                    num = tj * tj - d2 - R * R
                    seen.add((float(num), float(np.float32(2.0) * R)))
    assert len(seen) > 1000
    for num, d in seen:
        num, d = np.float32(num), np.float32(d)
        if not (np.float32(1.0) <= d <= np.float32(192.0)):
            continue  # (outside the range k_occlusion_mx admits: 2R in [1, 192])
        q = tc.quotient_3op(num, d)
        assert q == num / d or (q == 0 and num == 0), (num, d, q, num / d)
    rng = np.random.default_rng(88172645)
    ds = [np.float32(2.0) * (np.float32(r) + np.float32(1.4)) for r in (1.88, 1.61, 1.42, 1.64, 1.76, 1.46, 1.77)]
    ds.append(np.float32(1.0))
    for e in range(8):
        for m in (0x7FFFFF, 0, 0x7FFFFE, 1, int(rng.integers(0, 1 << 23)), int(rng.integers(0, 1 << 23))):
            ds.append(np.array([(127 + e) << 23 | m], np.uint32).view(np.float32)[0])
    n = 4000
    for d in ds:
        a = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(-44, 16, n) * rng.choice([-1, 1], n)).astype(np.float32)
        y = np.float32(1.0) / d
        q0 = a * y
        r = tc.fmaf_vec(-q0, np.full(n, d, np.float32), a)
        q = tc.fmaf_vec(r, np.full(n, y, np.float32), q0)
        assert np.array_equal(q, a / d), (d, a[q != a / d][:3])
