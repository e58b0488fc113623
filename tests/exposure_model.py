"""An exact CPU model of the exposure vectors (rsasa_exposure_vectors*) and of the volume made from them
(rsasa_sas_volume).  The masks are those of points_model.exposed_masks*; the vectors are the float32 sums of the exposed
lattice points in the order the header fixes:

  - the lattice in chunks of 64 points, zero padded; a point's term is t = exposed ? s : +0.0 per component
  - within a chunk, for h = 32, 16, 8, 4, 2, 1: t[l] = t[l] + t[l + h] for l < h; the chunk's sum is t[0]
  - across chunks, ascending: E = chunk_0, then E = E + chunk_c

all in np.float32, so a comparison with the engine is one of bit patterns.  The volume is the double formula
V = sum (a / 3) (R k + (c - o) . E), a = 4 pi R^2 / n_points, in atom order.  Plain helper module (not a conftest)."""
import numpy as np

from oracle import pyoracle as po

F = np.float32
CHUNK = 64  # points per chunk (kWave)


def vectors_of(mask, n_points):
    """float32[N, 3] from bool[N, n_points]: the sums of the exposed points of po.sphere_points(n_points), in the
    interface's order."""
    mask = np.asarray(mask)
    assert mask.dtype == bool and mask.ndim == 2 and mask.shape[1] == n_points >= 1
    n = mask.shape[0]
    n_chunks = -(-n_points // CHUNK)
    padded = np.zeros((n, n_chunks * CHUNK), bool)
    padded[:, :n_points] = mask
    out = np.empty((n, 3), F)
    for k, s in enumerate(po.sphere_points(n_points)):
        sp = np.zeros(n_chunks * CHUNK, F)
        sp[:n_points] = s
        t = np.where(padded, sp[None, :], F(0)).reshape(n, n_chunks, CHUNK)
        assert t.dtype == F
        h = CHUNK // 2
        while h >= 1:
            t = t[:, :, :h] + t[:, :, h:2 * h]
            assert t.dtype == F
            h //= 2
        e = t[:, 0, 0].copy()
        for c in range(1, n_chunks):
            e = e + t[:, c, 0]
        assert e.dtype == F
        out[:, k] = e
    return out


def bits(a):
    """The bit patterns of a float32 array (what the comparisons with the engine compare)."""
    a = np.ascontiguousarray(a)
    assert a.dtype == F
    return a.view(np.uint32)


def _seq_sum(a):
    """The sum of a float64 array in index order (np.sum adds pairwise)."""
    a = np.asarray(a, np.float64)
    return float(np.cumsum(a)[-1]) if a.size else 0.0


def volume_of(x, y, z, r, vectors, free, probe, n_points, so=None, origins=None):
    """(volume float64[S], area float64[S]): the double formula of rsasa_sas_volume in plain numpy, atoms in order;
    atoms with a non-finite coordinate or radius are skipped; origins None: the mean centre of the counted atoms."""
    x, y, z, r = (np.ascontiguousarray(a, F) for a in (x, y, z, r))
    vectors = np.ascontiguousarray(vectors, F).reshape(len(x), 3)
    free = np.ascontiguousarray(free, np.uint32)
    so = np.array([0, len(x)], np.uint32) if so is None else np.asarray(so, np.uint32)
    vol, area = np.zeros(len(so) - 1), np.zeros(len(so) - 1)
    for s in range(len(so) - 1):
        i = np.arange(int(so[s]), int(so[s + 1]))
        i = i[np.isfinite(x[i]) & np.isfinite(y[i]) & np.isfinite(z[i]) & np.isfinite(r[i])]
        c = [a[i].astype(np.float64) for a in (x, y, z)]
        if origins is not None:
            o = [float(v) for v in np.asarray(origins, np.float64).reshape(-1, 3)[s]]
        elif len(i):
            o = [_seq_sum(a) / float(len(i)) for a in c]
        else:
            o = [0.0, 0.0, 0.0]
        with np.errstate(over="ignore"):
            R = (r[i] + F(probe)).astype(np.float64)   # the sum in float32, as the engine's R
        k = free[i].astype(np.float64)
        E = vectors[i].astype(np.float64)
        a = ((4.0 * np.pi) * (R * R)) / float(n_points)
        dot = (c[0] - o[0]) * E[:, 0] + (c[1] - o[1]) * E[:, 1] + (c[2] - o[2]) * E[:, 2]
        vol[s] = _seq_sum((a / 3.0) * (R * k + dot))
        area[s] = _seq_sum(a * k)
    return vol, area


def union_volume(R1, R2, d):
    """The volume of the union of two balls of radii R1, R2 whose centres are d apart (|R1 - R2| < d < R1 + R2):
    4/3 pi (R1^3 + R2^3) minus the lens."""
    assert abs(R1 - R2) < d < R1 + R2
    lens = np.pi * (R1 + R2 - d) ** 2 * (d * d + 2.0 * d * (R1 + R2) - 3.0 * (R1 - R2) ** 2) / (12.0 * d)
    return 4.0 / 3.0 * np.pi * (R1 ** 3 + R2 ** 3) - lens
