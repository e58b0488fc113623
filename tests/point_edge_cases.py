"""The inputs of the point-mask and contact-count edge tests (test_point_edges_cpu.py, test_gpu_point_edges.py): the
point counts around the chunks, words, passes and kernel instantiations of points.hip, the radius / probe settings off
the protein range, the cluster sizes around the list staging, and the two models run together.  The CPU file pins the
models to the oracle on these inputs; the GPU file compares the kernels with the models.  Plain helper module (not a
conftest)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import contacts_model as cm
import nb_helpers as nh
import points_model as pm
import structio as sio
import tie_cases as tc

WS = (1, 4, 8, 16)
WAVE = 64        # points per chunk (kWave)
PT_STAGE = 256   # list entries per LDS stage (kPtStage)
NCH_SPLIT = 128  # the launcher: NCH = 2 up to 2 * kWave points, NCH = 4 above

EDGE_POINTS = (1, 2, 3, 5, 7, 15, 16, 17, 31, 32, 33, 63, 64, 65, 67, 79, 96, 97, 128, 129, 130, 143, 192, 193, 255,
               256, 257, 259, 271, 320, 321, 512, 513)

CLUSTER_SIZES = (2, 3, 4, 5, 6, 256, 257, 258, 259, 260, 261, 512, 513, 514, 769)   # K = n - 1


def nch(n_points):
    return 2 if n_points <= NCH_SPLIT else 4


def assert_edge_point_classes():
    """The classes EDGE_POINTS must hold, by arithmetic (a later edit cannot silently lose one)."""
    nf = {(n, W): tc.n_fused(n, W) for n in EDGE_POINTS for W in WS}
    assert all(v == n - n % W for (n, W), v in nf.items())
    # every point a remainder point
    assert any(v == 0 for v in nf.values())
    # the remainder alone in a later chunk of the first pass
    assert any(0 < v < n and v % WAVE == 0 and n <= WAVE * nch(n) for (n, W), v in nf.items())
    # the remainder alone in the second pass of the NCH = 4 kernel: pass 1 REM = false, pass 2 REM = true
    assert any(v == 4 * WAVE < n for (n, W), v in nf.items())
    # one mask word, a dead second chunk, both sides of the launcher's split, dead chunks of four, one full pass and
    # the smallest second pass (one live chunk, one word of it), two full passes and one point more
    assert 1 in EDGE_POINTS and any(n < 32 for n in EDGE_POINTS) and 64 in EDGE_POINTS and 65 in EDGE_POINTS
    assert {128, 129, 192, 193, 256, 257, 512, 513} <= set(EDGE_POINTS)
    assert len({pm.words_of(n) for n in EDGE_POINTS}) >= 12


def threads():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(16, n))


def pmap(f, keys):
    """{key: f(key)} on at most 16 threads (numpy releases the interpreter lock in the large array operations)."""
    keys = list(keys)
    with ThreadPoolExecutor(threads()) as ex:
        return dict(zip(keys, ex.map(f, keys)))


def fixture(name):
    if name.endswith(":vdw"):
        return sio.soa_vdw(sio.read_structure(sio.data_path(name.split(":")[0])))
    return nh.protor(name)


def popcount(words):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1).sum(axis=1).astype(np.int64)


def models(cols, probe, n_points, Ws=WS):
    """(offsets, entries, {W: (mask bool[N, n_points], covered, exclusive, buried)}): points_model and contacts_model
    on one set of oracle lists."""
    lists = nh.oracle_csr(*cols, probe)
    masks = pm.exposed_masks_ws(*cols, probe, n_points, Ws, lists)
    offs, ent, by_w = cm.contact_counts_ws(*cols, probe, n_points, Ws, lists)
    return offs, ent, {W: (masks[W],) + by_w[W] for W in Ws}


def batch_models(x, y, z, r, ids, so, probe, n_points, W):
    """(mask bool[N, n_points], covered, exclusive) of every structure of a batch, aligned with
    nb_helpers.oracle_batch_csr."""
    mask = pm.exposed_masks_batch(x, y, z, r, ids, so, probe, n_points, W)
    cov, exc = cm.contact_counts_batch(x, y, z, r, ids, so, probe, n_points, W)
    return mask, cov, exc


def degenerate_settings(r, seed=8):
    """[(label, probe, radii)]: the radius / probe settings off the protein range, on a copy of the radii `r`."""
    rng = np.random.default_rng(seed)
    r = np.ascontiguousarray(r, np.float32)

    def some(vals, k=4):
        out = r.copy()
        idx = rng.choice(len(r), k * len(vals), replace=False)
        out[idx] = np.resize(np.array(vals, np.float32), idx.shape)
        return out
    return [("negative", 1.4, some((-1.0, -0.25))),
            ("one_70", 1.4, some((70.0,), 1)),
            ("zeros", 1.4, some((0.0,))),
            ("around_64", 1.4, some((63.5, 64.5))),
            ("R_zero_probe_0", 0.0, some((0.0,))),
            ("tiny", 0.05, (r * np.float32(0.2)).astype(np.float32)),
            ("probe_33", 33.0, r.copy()),
            ("huge", 2.0, (r * np.float32(12.0)).astype(np.float32)),
            ("R_zero_probe_1.4", 1.4, some((-1.4,))),
            ("negative_probe_0", 0.0, some((-0.5,)))]


def with_radii(cols, r):
    return cols[:3] + (r,) + cols[4:]


# (probe, the radius of atom 500) on 1jcd.  The structure is 85.1 A across: at probe 33 and with one radius of 70 the
# search radius r + max_r + 2 probe is about 70 / 75 A, so most lists hold every other atom (1 051 entries, four full
# stages and 27 entries) and the shortest still need four stages; at probe 42 it is above 85.2 A and every list does.
FULL_LIST_SETTINGS = {"probe_33": (33.0, None), "radius_70": (1.4, 70.0), "probe_42": (42.0, None)}


def full_list_cols(setting):
    probe, r70 = FULL_LIST_SETTINGS[setting]
    cols = nh.protor("1jcd.pdb")
    if r70 is not None:
        r = cols[3].copy()
        r[500] = r70
        cols = with_radii(cols, r)
    return cols, probe


def assert_full_lists(setting, k):
    """k: the list lengths.  Every list takes at least four stages, most (all at probe 42) hold every other atom: five
    stages, the last of 27 entries, K % 4 = 3."""
    n = len(k)
    assert n == 1052 and (n - 1) // PT_STAGE == 4 and (n - 1) % PT_STAGE == 27 and (n - 1) % 4 == 3
    assert int(k.max()) == n - 1 and int(k.min()) > 3 * PT_STAGE
    assert int(np.sum(k == n - 1)) >= (n if setting == "probe_42" else 750)
