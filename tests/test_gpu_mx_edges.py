"""k_occlusion_mx at its integer limits (tests/mx_cases.py): group width, union size and narrowing, the first-chunk
rule, the candidate list's cap, spill and prep passes, the chunk-count loop bodies, phase B's forms, the survivor
list's flushes, blocks of atoms per wave, the persistent waves' pieces and the id bitmaps' word edges.

Almost every one of these branches has a correct fallback - the atom goes to k_occlusion_v3 - so values alone cannot
show an off-by-one in a limit.  Every run therefore asserts three things: each atom's value bit-equal to the oracle
at the same lane count, the candidate counts K equal to the oracle's, and timings()["n_deferred"] EQUAL to the count
the routing model (tests/mx_model.py) gives for that batch, block size and id verdict.  test_mx_cases_cpu.py pins the
cases to their edges and shows that the count does not depend on the order of the atoms inside a cell.

A batch in which some structure keeps its ids is run twice in its context: the first run may be run again by the host
(OcclusionChain::solo) and is checked on its values only; the second is a plain pair of launches and its count is
asserted too."""
import numpy as np
import pytest

import mx_cases as mc
import tie_cases as ti

pytestmark = pytest.mark.gpu

MX_MIN_ATOMS = 32768
_ORACLE = {}


def _want(c):
    """(values, K) of the oracle for a case or batch, every structure computed once per (W, probe, n_points)."""
    vals, ks = [], []
    for st in c.structures:
        key = (id(st), c.W, c.probe, c.n_points)
        if key not in _ORACLE:
            if st.n:
                v, _, k = ti.oracle_counts(st, c.probe, c.n_points, c.W)
            else:
                v, k = np.zeros(0, np.float32), np.zeros(0, np.uint32)
            _ORACLE[key] = (st, v, k)   # (the structure is kept: its id() stays its own)
        vals.append(_ORACLE[key][1])
        ks.append(_ORACLE[key][2])
    return np.concatenate(vals), np.concatenate(ks).astype(np.uint32)


def _device_run(ctx, c):
    """The batch from device memory with K out (as test_gpu_ties._device_run); (values, K, n_deferred)."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out = torch.full((c.n,), -1.0, dtype=torch.float32, device=dev)
    k = torch.zeros(c.n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.enqueue_device(t(c.x), t(c.y), t(c.z), t(c.r), t(c.ids.view(np.int64)), c.so, out, None, None, k, c.probe,
                       c.n_points, stream=torch.cuda.current_stream().cuda_stream)
    ctx.wait()
    return out.cpu().numpy(), k.cpu().numpy().view(np.uint32), int(ctx.timings()["n_deferred"])


def _check(ctx, c, apw, tag):
    """One batch on the device path: values, K and the deferred count against the oracle and the model."""
    want, want_k = _want(c)
    m = c.model(apw=apw)
    kept = sum(s.has_ids for s in m.structs)
    got, k, n_def = _device_run(ctx, c)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (tag, c.name, "values", bad[:5].tolist(), m.reason[bad[:5]].tolist())
    assert np.array_equal(k, want_k), (tag, c.name, "K", np.flatnonzero(k != want_k)[:5].tolist())
    if kept:
        # (the first run of a batch whose ids matter may have been run again by the host: values only; now the pair)
        got, k, n_def = _device_run(ctx, c)
        assert np.array_equal(got, want) and np.array_equal(k, want_k), (tag, c.name, "second run")
        assert ctx.ids_kept() == kept, (tag, c.name, ctx.ids_kept(), kept)
    print(f"{tag} {c.name}: atoms {c.n} apw {m.apw} deferred gpu {n_def} model {m.n_deferred}")
    assert n_def == m.n_deferred, (tag, c.name, "n_deferred", n_def, m.n_deferred)


def _context(monkeypatch, W, apw):
    import rustsasa_amd
    monkeypatch.setenv("RSASA_OCCLUSION_KERNEL", "5")
    if apw:
        monkeypatch.setenv("RSASA_ATOMS_PER_WAVE", str(apw))
    else:
        monkeypatch.delenv("RSASA_ATOMS_PER_WAVE", raising=False)
    ctx = rustsasa_amd.Context(0, simd_width=W)
    ctx.enable_timing(True)
    return ctx


FAMILIES = ["union", "first_chunk", "list", "shift", "phase_b", "many", "ids", "range"]


@pytest.mark.parametrize("family", FAMILIES)
def test_every_case_alone(family, monkeypatch):
    """Each case as a batch of its own, with the atoms per wave it is pinned at (64; 16 above 128 points): the edge it is
    named for is the one the launch meets.  A fresh context per lane count; the shift cases with and without ids."""
    cases = [c for c in mc.all_cases() if c.family == family]
    assert cases
    for W, apw in sorted({(c.W, c.apw) for c in cases}):
        with _context(monkeypatch, W, apw) as ctx:
            for c in cases:
                if (c.W, c.apw) == (W, apw):
                    _check(ctx, c, apw, family)


@pytest.mark.parametrize("apw", [8, 23, 64])
def test_blocks_of_atoms_per_wave(apw, monkeypatch):
    """RSASA_ATOMS_PER_WAVE = 8, 23 and 64: exactly one block, exactly four, 4 apw + 1 atoms (a last block of one atom)
    with an empty structure and structure boundaries inside a wave - and every case of the common (W, probe, n_points)
    in one batch, whose groups and cells the blocks' ends cut wherever they fall."""
    with _context(monkeypatch, 8, apw) as ctx:
        for c in mc.block_cases(apw):
            _check(ctx, c, apw, f"blocks{apw}")
        _check(ctx, mc.packed(mc.KEY), apw, f"blocks{apw}")


@pytest.mark.parametrize("key", mc.keys(), ids=str)
def test_packed_batches(key, monkeypatch):
    """All cases of one (W, probe, n_points) in one batch, and in the opposite order: the same groups meet other block
    boundaries (the model is evaluated for that batch).  With the launch's own atoms per wave (8 at this size) and with
    the kernel's largest."""
    W, _, n_points = key
    for apw in (0, 16 if n_points > 128 else 64):
        with _context(monkeypatch, W, apw) as ctx:
            for rev in (False, True):
                _check(ctx, mc.packed(key, rev), apw, f"packed apw {apw}")


@pytest.mark.parametrize("n_points,W", mc.MANY_POINTS)
def test_many_point_batches(n_points, W, monkeypatch):
    """More than 128 points (persistent waves, the patch loop's second trip at 65 patches, the survivors' list flushed
    never, once and several times, remainder points in the last tile): batches of fewer than eight workgroups, exactly
    eight and nine, wave blocks the pieces do not divide, an empty last piece (mx_cases.MANY_SIZES)."""
    with _context(monkeypatch, W, 16) as ctx:
        for n_atoms in mc.MANY_SIZES:
            _check(ctx, mc.many_point_batch(n_points, W, n_atoms), 16, "many")


@pytest.mark.parametrize("offset", mc.SEG_OFFSETS)
def test_id_bitmaps_at_their_word_edge(offset, monkeypatch):
    """One structure that keeps its ids at cell-sorted positions 1984 .. 2047 (bit 31 of the bitmaps' first word),
    2048 .. 2111 (bit 0 of the second) and 2016 .. 2079 (both), the others with rising ids: the default pair of launches,
    each workgroup looking its atoms up in BatchView::ids_seg."""
    with _context(monkeypatch, 8, 0) as ctx:
        _check(ctx, mc.seg_case(offset), 0, "ids_seg")


def test_default_dispatch_tiled(monkeypatch):
    """The packed batch of the common key repeated to at least 32 768 atoms, no kernel forced: k_occlusion_mx by default."""
    import rustsasa_amd
    monkeypatch.delenv("RSASA_OCCLUSION_KERNEL", raising=False)
    monkeypatch.delenv("RSASA_ATOMS_PER_WAVE", raising=False)
    c = mc.packed(mc.KEY)
    want, want_k = _want(c)
    reps = -(-MX_MIN_ATOMS // c.n)
    big = mc.Case("tiled", "packed", c.structures * reps)
    assert big.n >= MX_MIN_ATOMS
    with rustsasa_amd.Context(0, simd_width=8) as ctx:
        ctx.enable_timing(True)
        got, k, _ = _device_run(ctx, big)
    assert np.array_equal(got, np.tile(want, reps)), int((got != np.tile(want, reps)).sum())
    assert np.array_equal(k, np.tile(want_k, reps))


@pytest.mark.parametrize("overlap", ["0", "1"])
def test_host_memory_entry_point(overlap, monkeypatch):
    """The packed batches through calculate_sasa_batch from pageable host memory, and with RSASA_OVERLAP_TAIL=1: values
    only (the host path folds and checks the ids itself)."""
    import rustsasa_amd
    monkeypatch.setenv("RSASA_OCCLUSION_KERNEL", "5")
    monkeypatch.setenv("RSASA_OVERLAP_TAIL", overlap)
    for key in mc.keys():
        c = mc.packed(key)
        want, _ = _want(c)
        with rustsasa_amd.Context(0, simd_width=key[0]) as ctx:
            got, _ = ctx.calculate_sasa_batch(c.x, c.y, c.z, c.r, c.ids, c.so, c.probe, c.n_points)
        assert np.array_equal(got, want), (key, overlap, np.flatnonzero(got != want)[:5].tolist())
