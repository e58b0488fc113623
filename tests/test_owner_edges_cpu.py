"""The cases of owner_edge_cases.py without a GPU: the exact ties of tie_cases.py do exercise co_test's own copy of the
two hit rules (the model owns remainder points at margin exactly 0.0 and leaves fused points at dot == limit to nobody or
to a later entry - if either count were zero, test_tie_cases_owners could not see the copy drift), the pass and window
counts of the lists that add to owned[] across passes, and the degenerate batches."""
import numpy as np

import nb_helpers as nh
import owner_cases as oc
import owner_edge_cases as oe
import point_edge_cases as pe
import tie_cases as tc


def test_the_tie_cases_sit_on_both_rules_of_the_owner_kernel():
    fam = tc.generate()
    def per_case(cases, which):                                         # the count of each tie case, summed over its structures
        return [sum(oe.tie_margins(s, c.probe, c.n_points, c.W)[which] for s in c.structures) for c in cases if c.tie]
    rem, fused = per_case(fam["remainder"], 0), per_case(fam["fused"], 1)
    rem_zero, fused_kept = sum(rem), sum(fused)
    print(f"remainder ties: {rem_zero} owned points at margin 0.0 in {len(rem)} cases; "
          f"fused ties: {fused_kept} points at dot == limit not taken by that entry in {len(fused)} cases")
    # `dotu < limit` on the remainder lanes would free (or hand on) every one of the first, `dot <= limit` on the fused
    # lanes would take every one of the second
    assert rem_zero >= tc.MINIMUM["remainder_ties"], "the remainder ties never own a point at margin 0: the copy is not exercised"
    assert fused_kept >= tc.MINIMUM["fused_ties"], "the fused ties never leave a point at dot == limit: the copy is not exercised"
    # ... and every tie case has such a point in one of its structures
    assert len(rem) >= tc.MINIMUM["remainder_ties"] and all(rem)
    assert len(fused) >= tc.MINIMUM["fused_ties"] and all(fused)


def test_the_tie_groups_are_those_of_the_contact_test():
    groups = oe.tie_groups()
    assert sum(len(v) for v in groups.values()) > 10000
    assert {W for _, _, W in groups} == {1, 4, 8, 16} and len(groups) > 40
    assert any(tc.n_fused(n, W) < n for _, n, W in groups) and any(n > 128 for _, n, _ in groups)   # both rules, both kernels


def test_pass_and_window_counts():
    assert oe.PASS_WINDOW_CASES == (("late_owner", 513), (258, 960))
    want = {("late_owner", 513): (599, 3, 3), (258, 960): (257, 4, 2)}
    for name, n_points in oe.PASS_WINDOW_CASES:
        cols, c0 = oe.named_cols(name)
        k = np.diff(nh.oracle_csr(*cols, 1.4)[0].astype(np.int64))
        K, n_pass, n_win = want[(name, n_points)]
        assert k[c0:].min() == k[c0:].max() == K and k[:c0].max() < oc.PT_STAGE
        assert pe.nch(n_points) == 4 and oc.PT_STAGE == pe.PT_STAGE == 256
        assert oe.passes(n_points) == n_pass == -(-(-(-n_points // 64)) // 4) and oe.windows(K) == n_win
    # the first suite's longest lists: one or two passes
    assert [oe.passes(n) for n in (100, 300)] == [1, 2] and oe.passes(256) == 1 and oe.passes(257) == 2
    assert tc.n_fused(513, 8) == 512 and tc.n_fused(513, 16) == 512     # the remainder point alone in the third pass
    assert tc.n_fused(960, 8) == tc.n_fused(960, 16) == 960


def test_degenerate_batches_are_those_of_the_contact_counts():
    labels = [s[0] for s in pe.degenerate_settings(nh.protor("1jcd.pdb")[3])]
    assert len(labels) == oe.N_DEGENERATE and {"negative", "R_zero_probe_0", "probe_33", "huge"} <= set(labels)
    for k in (0, 6):
        cat, so, probe = oe.degenerate_batch(k)
        n = len(nh.protor("1jcd.pdb")[0])
        assert len(so) == 4 and int(so[2] - so[1]) == n and int(so[-1]) == len(cat[0])
        assert probe == pe.degenerate_settings(cat[3][so[1]:so[2]])[k][1]
        assert np.array_equal(cat[3][so[1]:so[2]], pe.degenerate_settings(nh.protor("1jcd.pdb")[3])[k][2])
    assert tc.n_fused(*oe.DEGENERATE_BATCH) == 96
