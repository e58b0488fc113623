"""The HIP kernels at the edges of their decisions (tests/tie_cases.py): exact dot == limit ties, the f16 filter's
margin band, patch rims, k_occlusion_mx's admission range, candidate cutoffs and colliding id folds.  Every atom
bit-equal to the oracle run with the same lane count, and the neighbour counts K equal where they are returned;
through every kernel route and entry point."""
import numpy as np
import pytest

import tie_cases as tc

pytestmark = pytest.mark.gpu

MX_MIN_ATOMS = 32768  # batches of at least this many atoms take k_occlusion_mx by default


class Group:
    """The cases' structures that share (W, probe, n_points), packed into one batch, with the oracle's answer."""

    def __init__(self, key, structures):
        self.W, self.probe, self.n_points = key
        self.structures = structures
        self.x, self.y, self.z, self.r, self.ids, self.so = tc.pack(structures)
        vals, ks = [], []
        for st in structures:
            v, _, k = tc.oracle_counts(st, self.probe, self.n_points, self.W)
            vals.append(v)
            ks.append(k)
        self.want = np.concatenate(vals)
        self.want_k = np.concatenate(ks)

    @property
    def n(self):
        return len(self.x)

    def tiled(self, min_atoms):
        """The batch repeated until it holds at least min_atoms atoms (structures are independent)."""
        reps = -(-min_atoms // self.n)
        so = np.concatenate([self.so[:-1] + np.uint32(k * self.n) for k in range(reps)] + [[reps * self.n]])
        t = lambda a: np.tile(a, reps)  # noqa: E731
        return (t(self.x), t(self.y), t(self.z), t(self.r), t(self.ids), so.astype(np.uint32),
                t(self.want), t(self.want_k))


@pytest.fixture(scope="module")
def groups():
    by = {}
    for c in tc.all_cases():
        by.setdefault((c.W, c.probe, c.n_points), []).extend(c.structures)
    return {k: Group(k, v) for k, v in sorted(by.items())}


def _device_run(ctx, x, y, z, r, ids, so, probe, n_points, want_k=True):
    """enqueue_device with the probe a parameter; returns (atom values, K or None)."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    n = len(x)
    out = torch.full((n,), -1.0, dtype=torch.float32, device=dev)
    k = torch.zeros(n, dtype=torch.int32, device=dev) if want_k else None
    torch.cuda.synchronize()
    ctx.enqueue_device(t(x), t(y), t(z), t(r), t(ids.view(np.int64)), so, out, None, None, k, probe, n_points,
                       stream=torch.cuda.current_stream().cuda_stream)
    ctx.wait()
    return out.cpu().numpy(), None if k is None else k.cpu().numpy().view(np.uint32)


def _key(W, probe, n_points):
    return (W, float(np.float32(probe)), n_points)


def _where(g, got):
    """(structure, atom) of the first few atoms that differ, for the failure message."""
    bad = np.flatnonzero(got != g.want)
    return [(int(np.searchsorted(g.so, b, side="right") - 1), int(b)) for b in bad[:5]]


def _by_width(groups):
    out = {}
    for key, g in groups.items():
        out.setdefault(g.W, []).append(g)
    return out


def test_default_dispatch_small_batches(groups):
    """Each group as one small batch (the per-atom kernels: fast or general): device-resident with K out, and from
    pageable host memory."""
    import rustsasa_amd
    for W, gs in _by_width(groups).items():
        with rustsasa_amd.Context(0, simd_width=W) as c:
            for g in gs:
                got, k = _device_run(c, g.x, g.y, g.z, g.r, g.ids, g.so, g.probe, g.n_points)
                assert np.array_equal(got, g.want), ("device", W, g.probe, g.n_points, _where(g, got))
                assert np.array_equal(k, g.want_k), ("K", W, g.probe, g.n_points)
                got, _ = c.calculate_sasa_batch(g.x, g.y, g.z, g.r, g.ids, g.so, g.probe, g.n_points)
                assert np.array_equal(got, g.want), ("host", W, g.probe, g.n_points, _where(g, got))


def test_default_dispatch_at_the_matrix_core_threshold(groups):
    """Each group repeated to at least 32 768 atoms: k_occlusion_mx by default (up to 1344 points with at most four
    remainder points; the others go to the general kernel) - NT = 4..8 tiles, the many-point kernel at 129 (4 waves),
    960 (8 waves), 1100 and 1344 (12 waves), every lane count."""
    import rustsasa_amd
    for W, gs in _by_width(groups).items():
        with rustsasa_amd.Context(0, simd_width=W) as c:
            for g in gs:
                x, y, z, r, ids, so, want, want_k = g.tiled(MX_MIN_ATOMS)
                got, k = _device_run(c, x, y, z, r, ids, so, g.probe, g.n_points)
                assert np.array_equal(got, want), (W, g.probe, g.n_points, int(np.sum(got != want)))
                assert np.array_equal(k, want_k), ("K", W, g.probe, g.n_points)


@pytest.mark.parametrize("kernel", ["0", "3", "4", "5"])
def test_kernel_variants_on_the_edges(kernel, groups, monkeypatch):
    """Every occlusion kernel forced (RSASA_OCCLUSION_KERNEL, a fresh context), every group, values and K."""
    import rustsasa_amd
    monkeypatch.setenv("RSASA_OCCLUSION_KERNEL", kernel)
    for W, gs in _by_width(groups).items():
        with rustsasa_amd.Context(0, simd_width=W) as c:
            for g in gs:
                got, k = _device_run(c, g.x, g.y, g.z, g.r, g.ids, g.so, g.probe, g.n_points)
                assert np.array_equal(got, g.want), (kernel, W, g.probe, g.n_points, _where(g, got))
                assert np.array_equal(k, g.want_k), ("K", kernel, W, g.probe, g.n_points)


def test_single_structure_calls(groups):
    """calculate_sasa_soa on single structures: every fifth structure of every group."""
    import rustsasa_amd
    for W, gs in _by_width(groups).items():
        with rustsasa_amd.Context(0, simd_width=W) as c:
            for g in gs:
                for s in range(0, len(g.structures), 5):
                    b, e = int(g.so[s]), int(g.so[s + 1])
                    got = c.calculate_sasa_soa(g.x[b:e], g.y[b:e], g.z[b:e], g.r[b:e], g.ids[b:e], g.probe, g.n_points)
                    assert np.array_equal(got, g.want[b:e]), (W, g.probe, g.n_points, s)


def test_pipelined_host_batches_with_folded_ids(groups, monkeypatch):
    """The 100-point, probe-1.4 cases of lane count 8 - fold collisions among them - repeated to 210 000 atoms and
    cut into sub-batches (RSASA_SUB_ATOMS): from pinned memory the host folds the ids to 32 bits (a structure whose
    folds collide keeps its ids, and the full ids are read where folds are equal), from pageable memory they travel
    whole."""
    import rustsasa_amd
    import torch
    g = groups[_key(8, 1.4, 100)]
    assert any(len(set(s.ids.tolist())) < s.n or len({tc.fold_id(int(i)) for i in s.ids}) < s.n for s in g.structures)
    x, y, z, r, ids, so, want, _ = g.tiled(210000)

    def pin(a):
        return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().numpy()

    monkeypatch.setenv("RSASA_SUB_ATOMS", "100000")
    with rustsasa_amd.Context(0) as c:
        got, _ = c.calculate_sasa_batch(*(pin(a) for a in (x, y, z, r, ids)), so, g.probe, 100)
        assert np.array_equal(got, want), ("pinned", int(np.sum(got != want)))
        got, _ = c.calculate_sasa_batch(x, y, z, r, ids, so, g.probe, 100)
        assert np.array_equal(got, want), ("pageable", int(np.sum(got != want)))


@pytest.mark.parametrize("apw", ["8", "23", "64"])
def test_mixed_id_verdicts_at_several_wave_widths(apw, groups, monkeypatch):
    """A batch in which a few structures keep their ids (an equal-id pair; a colliding-fold pair beside one) and the
    others do not, on k_occlusion_mx with RSASA_ATOMS_PER_WAVE = 8, 23 and 64 atoms per wave: the kernel's early
    return for structures of the other id verdict repeats the launch's block-to-atom mapping."""
    import rustsasa_amd
    monkeypatch.setenv("RSASA_OCCLUSION_KERNEL", "5")
    monkeypatch.setenv("RSASA_ATOMS_PER_WAVE", apw)
    fold = tc.generate()["fold"]
    plain = [st for c in tc.generate()["fused"] if (c.W, c.n_points) == (8, 100) for st in c.structures]
    assert len(plain) > 200
    # kept-id structures at the start, in the middle and at the end of the batch
    sts = [fold[0].structures[1]] + plain[:100] + [fold[1].structures[3]] + plain[100:] + [fold[2].structures[1],
                                                                                          fold[3].structures[3]]
    g = Group(_key(8, 1.4, 100), sts)
    with rustsasa_amd.Context(0) as c:
        got, k = _device_run(c, g.x, g.y, g.z, g.r, g.ids, g.so, g.probe, 100)
        assert np.array_equal(got, g.want), (apw, _where(g, got))
        assert np.array_equal(k, g.want_k), apw
