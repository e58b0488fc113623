"""The models of the point-mask and contact-count edge tests against the oracle, on every input family that
test_gpu_point_edges.py adds (point_edge_cases.py): points_model's masks give the oracle's values byte for byte
(sasa_of of their popcounts == calculate_sasa_internal at the same lane count), and contacts_model's buried counts are
n_points minus those popcounts.  No GPU; every comparison is exact."""
import numpy as np
import pytest

import nb_helpers as nh
import point_edge_cases as pe
import points_model as pm
from oracle import pyoracle as po


def _check(cols, probe, n_points, Ws=pe.WS):
    x, y, z, r, ids = cols
    _, _, by_w = pe.models(cols, probe, n_points, Ws)
    for W in Ws:
        mask, cov, exc, buried = by_w[W]
        assert mask.shape == (len(x), n_points)
        k = mask.sum(axis=1).astype(np.int64)
        assert np.array_equal(pe.popcount(pm.pack(mask)), k)
        want = po.calculate_sasa_internal(x, y, z, r, ids, probe, n_points, W)
        assert pm.sasa_of(r, probe, k, n_points).tobytes() == want.tobytes(), (probe, n_points, W)
        assert np.array_equal(buried, n_points - k), (probe, n_points, W)
        assert np.all(exc <= cov)


def test_edge_point_classes():
    pe.assert_edge_point_classes()


def test_models_equal_oracle_at_edge_point_counts():
    cols = nh.protor("1jcd.pdb")
    pe.pmap(lambda n: _check(cols, 1.4, n), pe.EDGE_POINTS)


def test_models_equal_oracle_at_edge_point_counts_vdw_radii():
    cols = pe.fixture("example.cif:vdw")
    pe.pmap(lambda n: _check(cols, 1.4, n), (1, 33, 64, 130, 257, 271))


def test_models_equal_oracle_at_degenerate_radii_and_probes():
    cols = nh.protor("1jcd.pdb")
    settings = pe.degenerate_settings(cols[3])
    assert len(settings) == 10
    # R = r + probe is 0 in two settings (the model divides by zero there: numpy warns, the values are the oracle's)
    assert sum(bool(np.any(r + np.float32(p) == 0)) for _, p, r in settings) == 2
    assert sum(bool(np.any(r + np.float32(p) < 0)) for _, p, r in settings) >= 1
    assert sum(bool(np.any(r < 0)) for _, p, r in settings) >= 3

    def one(k):
        label, probe, r = settings[k]
        for n_points in (100, 271):
            _check(pe.with_radii(cols, r), probe, n_points)
    pe.pmap(one, range(len(settings)))


@pytest.mark.parametrize("n_points", [100, 300])
def test_models_equal_oracle_on_clusters(n_points):
    def one(n):
        cols, c0 = nh.tight_cluster(n, seed=n)
        offs, _ = nh.oracle_csr(*cols)
        k = np.diff(offs.astype(np.int64))
        assert k[c0:].min() == k[c0:].max() == n - 1 and k[:c0].max() < pe.PT_STAGE
        _check(cols, 1.4, n_points, (1, 16))
    sizes = pe.CLUSTER_SIZES if n_points == 100 else (5, 257, 513, 769)
    pe.pmap(one, sizes)


def test_models_equal_oracle_on_lists_of_nearly_every_atom():
    """probe 33, one radius of 70 and probe 42 on 1jcd: lists of four and five LDS stages (pe.full_list_cols)."""
    def one(setting):
        cols, probe = pe.full_list_cols(setting)
        offs, _ = nh.oracle_csr(*cols, probe)
        pe.assert_full_lists(setting, np.diff(offs.astype(np.int64)))
        _check(cols, probe, 100, (8,))
    pe.pmap(one, sorted(pe.FULL_LIST_SETTINGS))
