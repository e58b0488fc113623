"""k_occlusion_fast and k_occlusion_v3 at their structural limits (tests/pa_cases.py): the 256 swept atoms and the 144
candidate records (with the padding behind them) of the fast kernel, its marker words, prep passes, near counts, phase
B's tilings and point counts; the general kernel's flush threshold, 256-position windows, chunk groups with the re-sweep
and the `done` exit, remainder tilings and id rule; blocks of atoms per wave, the XCD remap and the deferred list's
launch; and the row culling of both prologues in grids up to 4 000 cells long.

Almost every one of these branches has a correct fallback - a deferred atom goes to k_occlusion_v3, an extra flush only
costs time - so values alone cannot show an off-by-one in a limit.  Every fast run therefore asserts three things: each
atom's value bit-equal to the oracle at the same lane count, the candidate counts K equal to the oracle's, and
timings()["n_deferred"] EQUAL to the count the routing model (tests/pa_model.py) gives for that batch.  The general
kernel's flushes and windows cannot be observed: its cases are asserted on values and K (a dropped candidate shows as
a K that is too small, or a value that is too large), with K out and without - only the run without K can take the
`done` exit.  test_pa_cases_cpu.py pins every case to its edge and shows that nothing asserted here depends on the
culling's heuristic factors or on the order of the atoms inside a cell.  Outputs are filled with -1 before every run:
an atom that nobody writes shows up."""
import threading

import numpy as np
import pytest

import pa_cases as pc
import pa_model as pm
import tie_cases as ti

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _want(c):
    """(values, K) of the oracle for a case or batch, every structure computed once per (W, probe, n_points)."""
    vals, ks = [], []
    for st in c.structures:
        key = (id(st), c.key)
        if key not in _ORACLE:
            if st.n:
                v, _, k = ti.oracle_counts(st, c.probe, c.n_points, c.W)
            else:
                v, k = np.zeros(0, np.float32), np.zeros(0, np.uint32)
            _ORACLE[key] = (st, v, k)   # (the structure is kept: its id() stays its own)
        vals.append(_ORACLE[key][1])
        ks.append(_ORACLE[key][2])
    return np.concatenate(vals), np.concatenate(ks).astype(np.uint32)


def _device_run(ctx, c, want_k=True):
    """The batch from device memory; (values, K or None, n_deferred)."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out = torch.full((c.n,), -1.0, dtype=torch.float32, device=dev)
    k = torch.full((c.n,), -1, dtype=torch.int32, device=dev) if want_k else None
    torch.cuda.synchronize()
    ctx.enqueue_device(t(c.x), t(c.y), t(c.z), t(c.r), t(c.ids.view(np.int64)), c.so, out, None, None, k, c.probe,
                       c.n_points, stream=torch.cuda.current_stream().cuda_stream)
    ctx.wait()
    return out.cpu().numpy(), None if k is None else k.cpu().numpy().view(np.uint32), int(ctx.timings()["n_deferred"])


def _context(monkeypatch, W, kernel=None, apw=None, timing=True):
    import rustsasa_amd
    for name, v in (("RSASA_OCCLUSION_KERNEL", kernel), ("RSASA_ATOMS_PER_WAVE", apw)):
        if v:
            monkeypatch.setenv(name, str(v))
        else:
            monkeypatch.delenv(name, raising=False)
    ctx = rustsasa_amd.Context(0, simd_width=W)
    ctx.enable_timing(timing)
    return ctx


def _check(ctx, c, tag, kernel=None, apw=None, counts=True):
    """One batch on the device path with K out: values, K and the deferred count against the oracle and the model."""
    want, want_k = _want(c)
    got, k, n_def = _device_run(ctx, c)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (tag, c.name, "values", bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
    assert np.array_equal(k, want_k), (tag, c.name, "K", np.flatnonzero(k != want_k)[:5].tolist())
    if counts:
        m = c.model(kernel=kernel, apw=apw)
        print(f"{tag} {c.name}: atoms {c.n} apw {m.apw} deferred gpu {n_def} model {m.n_deferred}")
        assert n_def == m.n_deferred, (tag, c.name, "n_deferred", n_def, m.n_deferred)
    return n_def


def _check_without_k(ctx, c, tag):
    want, _ = _want(c)
    got, _, n_def = _device_run(ctx, c, want_k=False)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (tag, c.name, "values without K", bad[:5].tolist())
    return n_def


FAST_FAMILIES = ["swept", "list", "near", "survivors", "points"]
V3_FAMILIES = ["flush", "windows", "groups", "remainder", "ids"]


@pytest.mark.parametrize("family", FAST_FAMILIES)
def test_every_fast_case_alone(family, monkeypatch):
    """Each case as a batch of its own, no kernel forced (a small batch takes k_occlusion_fast), K out, timing on:
    values, K and the deferred count EQUAL to the model's.  A fresh context per lane count."""
    cases = [c for c in pc.all_cases() if c.family == family and c.kernel == "fast"]
    assert cases
    for W in sorted({c.W for c in cases}):
        with _context(monkeypatch, W) as ctx:
            for c in cases:
                if c.W == W:
                    _check(ctx, c, family)
                    _check_without_k(ctx, c, family)


@pytest.mark.parametrize("family", V3_FAMILIES)
def test_every_v3_case_alone(family, monkeypatch):
    """Each case as a batch of its own, with K out and without (only the second run can take the `done` exit): up to 128
    points under RSASA_OCCLUSION_KERNEL=3, above 128 points or with more than 4 remainder points with no kernel forced
    (k_occlusion_v3 by default there).  Direct mode: nothing is deferred."""
    cases = [c for c in pc.all_cases() if c.family == family and c.kernel == "v3"]
    assert cases
    for W, forced in sorted({(c.W, c.forced or "") for c in cases}):
        with _context(monkeypatch, W, forced or None) as ctx:
            for c in cases:
                if (c.W, c.forced or "") == (W, forced):
                    assert _check(ctx, c, family, kernel=c.forced) == 0
                    assert _check_without_k(ctx, c, family) == 0


@pytest.mark.parametrize("key", pc.keys("fast"), ids=str)
def test_packed_fast_batches(key, monkeypatch):
    """All fast cases of one (W, probe, n_points) in one batch, forward and reversed: the same atoms meet other waves and
    other neighbours in the deferred list.  At the launch's own atoms per wave with no kernel forced, and under
    RSASA_OCCLUSION_KERNEL=4 at every forced value of the waves family (64 is capped to 40, 25 rounded to 20).  The
    count is the model's for that batch."""
    W = key[0]
    with _context(monkeypatch, W) as ctx:
        for rev in (False, True):
            _check(ctx, pc.packed(key, rev), "packed")
    for apw in (1, 3, 10, 11, 25, 40, 64):
        with _context(monkeypatch, W, "4", apw) as ctx:
            for rev in (False, True):
                _check(ctx, pc.packed(key, rev, apw=apw), f"packed k4 apw {apw}", kernel="4", apw=apw)


@pytest.mark.parametrize("apw", [1, 7, 8, 9])
def test_packed_v3_batches(apw, monkeypatch):
    """The general kernel's cases of the common key in one batch under RSASA_OCCLUSION_KERNEL=3 with 1, 7, 8 and 9 (capped
    to 8) atoms per wave, forward and reversed, and the wave batches: atom counts around 4 apw with a structure
    boundary and an empty structure inside a wave."""
    key = (pc.KEY[0], float(np.float32(pc.KEY[1])), pc.KEY[2])
    with _context(monkeypatch, key[0], "3", apw) as ctx:
        for rev in (False, True):
            c = pc.packed(key, rev, kernel="v3", apw=apw)
            assert _check(ctx, c, f"packed v3 apw {apw}", kernel="3", apw=apw) == 0
            assert _check_without_k(ctx, c, "packed v3") == 0
        for c in pc.v3_wave_batches()[apw]:
            assert _check(ctx, c, f"v3waves{apw}", kernel="3", apw=apw) == 0
            assert _check_without_k(ctx, c, "v3waves") == 0


@pytest.mark.parametrize("apw", [1, 3, 10, 11, 25, 40, 64])
def test_fast_wave_batches(apw, monkeypatch):
    """RSASA_OCCLUSION_KERNEL=4 with forced atoms per wave: 4 apw k - 1, 4 apw k and 4 apw k + 1 atoms for k = 1 and 2, a
    structure boundary and an empty structure inside a group of 10, and the one deferred atom of a batch first, in the
    middle and last of its group of 10."""
    with _context(monkeypatch, 8, "4", apw) as ctx:
        for c in pc.fast_wave_batches()[apw]:
            _check(ctx, c, f"waves{apw}", kernel="4", apw=apw)


def test_block_counts_around_the_xcd_remap(monkeypatch):
    """n_blocks = 7, 8, 9, 16 and 17 at the launch's own one atom per wave: per = 0, 1, 1, 2, 2."""
    with _context(monkeypatch, 8) as ctx:
        for c in pc.block_count_cases():
            m = c.model()
            assert (m.n_blocks, m.per) == (c.expect["n_blocks"], c.expect["per"])
            _check(ctx, c, "blocks")


def test_the_deferred_lists_launch(monkeypatch):
    """One context, in this order: batches that defer 0, 65, 200, 0, 65 and 129 atoms - the list-mode launch of
    k_occlusion_v3 is sized by the count the batch before left (1 024 workgroups while nothing is known, then half the
    last count, 16 at least), so its waves make one trip or several over the list.  Values, K and the count after every
    batch; the model's trip count for the hint in force is printed (it cannot be observed)."""
    hint = None
    with _context(monkeypatch, 8) as ctx:
        for ns, nd in ((0, 0), (65, 0), (53, 1), (0, 0), (65, 0), (129, 0)):
            c = pc.deferring_batch(ns, nd)
            n_def = _check(ctx, c, "deferred list")
            print(f"  hint {hint}: workgroups, trips = {pm.list_trips(c.n, n_def, hint)}")
            hint = n_def


def _single_structure_fast_cases():
    return [c for c in pc.all_cases() if c.kernel == "fast" and len(c.structures) == 1]


def test_single_structure_routes():
    """Every fast case through calculate_sasa_soa and calculate_sasa_internal: the single-structure route, where
    k_occlusion_fast reports a deferred atom through the pinned flag and the host then launches the general kernel.
    Values only (timing would send the call down the general path)."""
    import rustsasa_amd
    cases = _single_structure_fast_cases()
    for W in sorted({c.W for c in cases}):
        with rustsasa_amd.Context(0, simd_width=W) as ctx:
            for c in cases:
                if c.W != W:
                    continue
                want, _ = _want(c)
                got = ctx.calculate_sasa_soa(c.x, c.y, c.z, c.r, c.ids, c.probe, c.n_points)
                assert np.array_equal(got, want), ("soa", c.name, np.flatnonzero(got != want)[:5].tolist())
                got = ctx.calculate_sasa_internal(rustsasa_amd.make_atoms(c.x, c.y, c.z, c.r, c.ids), c.probe, c.n_points)
                assert np.array_equal(got, want), ("internal", c.name, np.flatnonzero(got != want)[:5].tolist())


def test_host_batch_routes():
    """The packed batches through calculate_sasa_batch on a small-path context and on a general-path context (as
    test_gpu_host_paths._context makes them).  Values only."""
    from test_gpu_host_paths import _context as host_context
    small, general = host_context(True), host_context(False)
    try:
        key = (pc.KEY[0], float(np.float32(pc.KEY[1])), pc.KEY[2])
        for kernel in ("fast", "v3"):
            for rev in (False, True):
                c = pc.packed(key, rev, kernel=kernel)
                want, _ = _want(c)
                for name, ctx in (("small", small), ("general", general)):
                    got, _ = ctx.calculate_sasa_batch(c.x, c.y, c.z, c.r, c.ids, c.so, c.probe, c.n_points)
                    assert np.array_equal(got, want), (name, c.name, np.flatnonzero(got != want)[:5].tolist())
    finally:
        small.close()
        general.close()


def test_call_combining_with_deferred_atoms():
    """Eight host threads on one context with call combining on, each calling with the structures of a batch that defers
    more than 64 atoms (a structure of 147 deferred atoms among them): every call equals the oracle, and the counters
    show that at least one block merged calls."""
    import rustsasa_amd
    batch = pc.deferring_batch(8, 1)
    assert batch.model().n_deferred > 64
    jobs = []
    for st in batch.structures:
        c = pc.Case("one", "packed", [st])
        jobs.append((c, _want(c)[0], rustsasa_amd.make_atoms(c.x, c.y, c.z, c.r, c.ids)))
    n_threads, n_iter = 8, 12
    errors, done = [], []
    shared = rustsasa_amd.Context(0)
    shared.set_call_combining(0)
    b0, c0 = rustsasa_amd.Context.call_combining_stats(0)
    # the combiner merges the calls that arrive while its three lanes are busy: the eight threads call together
    together = threading.Barrier(n_threads)

    def work(tid):
        try:
            for it in range(n_iter):
                c, want, atoms = jobs[(tid + 3 * it) % len(jobs)]
                together.wait(timeout=60)
                if (tid + it) % 2:
                    got = shared.calculate_sasa_internal(atoms, c.probe, c.n_points)
                else:
                    got = shared.calculate_sasa_soa(c.x, c.y, c.z, c.r, c.ids, c.probe, c.n_points)
                if not np.array_equal(got, want):
                    errors.append((tid, it, int(np.sum(got != want))))
            done.append(tid)
        except Exception as e:  # noqa: BLE001
            errors.append((tid, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(n_threads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a combined call hangs"
    b1, c1 = rustsasa_amd.Context.call_combining_stats(0)
    shared.close()
    assert errors == [] and len(done) == n_threads, errors[:8]
    assert c1 - c0 == n_threads * n_iter
    assert b1 - b0 < c1 - c0, f"{c1 - c0} calls in {b1 - b0} batches: nothing was merged"


@pytest.mark.parametrize("kernel", ["3", "4", None])
def test_reach_cases(kernel, monkeypatch):
    """tie_cases' exact-cutoff pairs and cell-face atoms in grids about 256, 1 024 and 4 000 cells long along x, y and z,
    the pair at the low and at the high end: tol is up to 4e-3 cells and fx carries the rounding of a long grid.  Both
    prologues (RSASA_OCCLUSION_KERNEL = 3, 4 and unset), values and K: a culled candidate shows in both."""
    by_probe = {}
    for c in pc.reach_cases():
        by_probe.setdefault(c.key, []).extend(c.structures)
    with _context(monkeypatch, 8, kernel) as ctx:
        for key, sts in sorted(by_probe.items()):
            c = pc.Case(f"reach_{key}", "reach", sts, W=key[0], probe=key[1], n_points=key[2])
            _check(ctx, c, f"reach k{kernel}", counts=False)


def test_packed_key_past_the_matrix_core_threshold(monkeypatch):
    """The packed batch of the common key repeated past 32 768 atoms, no kernel forced: k_occlusion_mx takes it and hands
    atoms to k_occlusion_v3 in list mode, which then reads the caller's ids through sorted_orig (no sorted copy of the
    ids is kept for the matrix-core kernel).  The common key is the cases' own (8, 0.5, 100): their geometry is built on
    probe 0.5, which makes the cell 2.0 with an exact reciprocal, not on 1.4.  Every fast case and every case of the `ids`
    family is in the batch: the structures with an equal id keep their ids, and an atom that meets its own id fold
    among its candidates (the ids cases, list_150_ids) or has more than 128 candidates (the list cases) is handed over.
    Values and K only."""
    key = (pc.KEY[0], float(np.float32(pc.KEY[1])), pc.KEY[2])
    c = pc.packed(key)
    c = pc.Case("packed_with_ids", "packed", c.structures + [s for i in pc.id_cases() for s in i.structures])
    want, want_k = _want(c)
    reps = -(-pm.MX_MIN_ATOMS // c.n) + 1
    big = pc.Case("tiled", "packed", c.structures * reps)
    assert big.n > pm.MX_MIN_ATOMS
    with _context(monkeypatch, 8) as ctx:
        got, k, _ = _device_run(ctx, big)
    assert np.array_equal(got, np.tile(want, reps)), int((got != np.tile(want, reps)).sum())
    assert np.array_equal(k, np.tile(want_k, reps))
