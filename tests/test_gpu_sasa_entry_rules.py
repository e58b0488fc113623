"""The verdicts of the SASA entry points - rsasa_calculate_sasa_internal, _soa, _batch, _trajectory,
rsasa_host_batch_enqueue, rsasa_batch_enqueue and rsasa_segment_sums - on arguments that break their rules
(rustsasa_amd/csrc/sasa_checks.h): every row of the table breaks one rule, or two where the order matters, and is
answered with the status and the message of the first.  Through the C ABI (_capi) on one context, with three atoms.  No
call passes its rules, so no kernel is launched, nothing is reserved and no output is written; a valid call on the same
context equals the oracle afterwards.

Rows that reach for the pipelined path CLAIM millions of atoms in their structure offsets while the columns hold three:
the rules answer before anything reads them.

`was`: what the same row got before the rules were gathered in front, where that differs (None: the same answer)."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

N = 3
PROBE = 1.4
NAN, INF = float("nan"), float("inf")
BIG = 0xFFFFFFF0  # the first size that does not fit

POINTS = "n_points must be in [1, 2^24]"
PROBE_MSG = "probe_radius must be finite and >= 0"
SPAN = "structure_offsets must span [0, n_atoms]"
ORDER = "structure_offsets must be non-decreasing"
COLS = "coordinate / radius arrays are NULL"
RES_OUT = "out_residue_sasa is NULL"
NO_OUT = "no output requested"
RES_EXCEED = "residue_offsets exceed n_atoms"
RES_ORDER = "residue_offsets must be non-decreasing"
BATCH_BIG = "batch too large for 32-bit indices"
TRAJ_BIG = "trajectory too large for 32-bit indices"
BARE = None  # refused without a message: the context's last error stays what it was

COMPUTED = "computed the atoms from structure_offsets[0] on (RSASA_OK)"
NOT_RUN = "not run: sized its buffers by the offsets before it answered"


class World:
    """One context, the arrays every row points into, and the values of the default arguments by name."""

    def __init__(self):
        import torch
        import rustsasa_amd
        from rustsasa_amd._capi import ptr
        f32, u32 = np.float32, np.uint32
        self.ctx = rustsasa_amd.Context(0)
        # (three atoms at the front of eight: a rule that read past the three would still read the test's own memory)
        col = lambda *v: np.array(list(v) + [0.0] * 5, f32)[:N]  # noqa: E731
        x, y, z, r = col(0.0, 1.5, 3.0), col(0.0, 0.0, 0.0), col(0.0, 0.0, 0.0), col(1.7, 1.7, 1.7)
        ids = np.arange(N, dtype=np.uint64)
        self.cols = (x, y, z, r, ids)
        self.host = dict(x=x, y=y, z=z, r=r, id=ids, atoms=rustsasa_amd.make_atoms(x, y, z, r, ids),
                         xyz=np.ascontiguousarray(np.tile(np.stack([x, y, z], 1), (2, 1, 1))),
                         so=np.array([0, N], u32), so_first=np.array([1, N], u32), so_fall=np.array([0, 5, N], u32),
                         so_both=np.array([1, 5, N], u32), so_huge=np.array([0, BIG], u32),
                         piped_first=np.array([1, 3_000_000, 6_000_000], u32), piped_both=np.array([1, 6_000_000, 3_000_000], u32),
                         piped_wrap=np.array([0, 3_500_000, 3_000_000], u32),
                         ro=np.array([0, 2, N], u32), ro_past=np.array([0, 2, N + 1], u32), ro_fall=np.array([0, 2, 1, N], u32),
                         seg_fall=np.array([0, 3, 2, N], u32), values=np.ones(N, f32))
        self.outs = dict(out=np.zeros(2 * N, f32), out_res=np.zeros(2 * N, f32))
        dev = torch.device("cuda:0")
        self.dev = dict(d_x=torch.zeros(N, device=dev), d_ro=torch.zeros(2, dtype=torch.int32, device=dev))
        self.dev_outs = dict(d_out=torch.zeros(N, device=dev), d_out_res=torch.zeros(N, device=dev))
        self.p = {k: ptr(v) for k, v in {**self.host, **self.outs}.items()}
        self.p.update({k: v.data_ptr() for k, v in {**self.dev, **self.dev_outs}.items()})

    def unwritten(self):
        import torch
        torch.cuda.synchronize()
        return not any(a.any() for a in self.outs.values()) and not any(bool(t.any()) for t in self.dev_outs.values())


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.ctx.close()


# entry point -> (default arguments by name; str values name an array of World, the call from the resolved values)
def _device_batch(v):
    from rustsasa_amd._capi import DeviceBatch
    if v["batch"] is None:
        return None
    return C.byref(DeviceBatch(v["x"], v["y"], v["z"], v["r"], v["id"], v["so"], v["S"], v["n_atoms"], v["ro"], v["R"], v["out"], v["out_res"],
                               None))


_BATCH = (dict(x="x", y="y", z="z", r="r", id=None, so="so", S=1, probe=PROBE, n_points=100, out="out", ro=None, R=0, out_res=None),
          lambda v: (v["x"], v["y"], v["z"], v["r"], v["id"], v["so"], v["S"], v["probe"], v["n_points"], v["out"], v["ro"], v["R"],
                     v["out_res"]))
ENTRIES = {
    "rsasa_calculate_sasa_soa": (dict(x="x", y="y", z="z", r="r", id="id", n=N, probe=PROBE, n_points=100, out="out"),
                                 lambda v: (v["x"], v["y"], v["z"], v["r"], v["id"], v["n"], v["probe"], v["n_points"], v["out"])),
    "rsasa_calculate_sasa_internal": (dict(atoms="atoms", n=N, probe=PROBE, n_points=100, out="out"),
                                      lambda v: (v["atoms"], v["n"], v["probe"], v["n_points"], -1, v["out"])),
    "rsasa_calculate_sasa_batch": _BATCH,
    "rsasa_host_batch_enqueue": _BATCH,
    "rsasa_calculate_sasa_trajectory": (dict(xyz="xyz", frames=2, n=N, r="r", id=None, probe=PROBE, n_points=100, out="out", ro=None, R=0,
                                             out_res=None),
                                        lambda v: (v["xyz"], v["frames"], v["n"], v["r"], v["id"], v["probe"], v["n_points"], v["out"],
                                                   v["ro"], v["R"], v["out_res"])),
    "rsasa_batch_enqueue": (dict(batch=True, x="d_x", y="d_x", z="d_x", r="d_x", id=None, so="so", S=1, n_atoms=N, ro=None, R=0,
                                 out="d_out", out_res=None, probe=PROBE, n_points=100),
                            lambda v: (_device_batch(v), v["probe"], v["n_points"], None)),
    "rsasa_segment_sums": (dict(values="values", n_values=N, offsets="ro", n=2, out="out"),
                           lambda v: (v["values"], v["n_values"], v["offsets"], v["n"], v["out"])),
}

RES = dict(ro="ro", R=2, out_res="out_res")  # residue sums asked for, in order

# (entry point, what the row breaks, changed arguments, the message - BARE: none, "ok": RSASA_OK -, was)
ROWS = [
    # ---- one structure per call: two bare refusals, the columns, empty, n_points, probe
    ("rsasa_calculate_sasa_soa", "n_atoms does not fit", dict(n=BIG, x=None), BARE, None),
    ("rsasa_calculate_sasa_soa", "no out_sasa, no columns", dict(out=None, x=None), BARE, None),
    ("rsasa_calculate_sasa_soa", "columns before n_points", dict(z=None, n_points=0), COLS, None),
    ("rsasa_calculate_sasa_soa", "no atoms: n_points 0 is no error", dict(n=0, n_points=0, probe=NAN), "ok", None),
    ("rsasa_calculate_sasa_soa", "n_points 0 before probe", dict(n_points=0, probe=NAN), POINTS, None),
    ("rsasa_calculate_sasa_soa", "n_points 2^24 + 1", dict(n_points=2 ** 24 + 1), POINTS, None),
    ("rsasa_calculate_sasa_soa", "probe NaN", dict(probe=NAN), PROBE_MSG, None),
    ("rsasa_calculate_sasa_soa", "probe -1", dict(probe=-1.0), PROBE_MSG, None),
    ("rsasa_calculate_sasa_internal", "no atoms array", dict(atoms=None, n_points=0), BARE, None),
    ("rsasa_calculate_sasa_internal", "no out_sasa", dict(out=None, n_points=0), BARE, None),
    ("rsasa_calculate_sasa_internal", "n_atoms does not fit", dict(n=BIG), BARE, None),
    ("rsasa_calculate_sasa_internal", "no atoms: n_points 0 is no error", dict(n=0, n_points=0), "ok", None),
    ("rsasa_calculate_sasa_internal", "n_points 0 before probe", dict(n_points=0, probe=INF), POINTS, None),
    ("rsasa_calculate_sasa_internal", "probe +inf", dict(probe=INF), PROBE_MSG, None),
    # ---- a host batch, in the order of its twelve verdicts
    ("rsasa_calculate_sasa_batch", "offsets NULL before columns", dict(so=None, x=None), "structure_offsets is NULL", None),
    ("rsasa_calculate_sasa_batch", "columns before out_residue_sasa", dict(y=None, ro="ro", R=2), COLS, None),
    ("rsasa_calculate_sasa_batch", "out_residue_sasa before the residue offsets", dict(ro="ro_past", R=2), RES_OUT, None),
    ("rsasa_calculate_sasa_batch", "no output before n_points", dict(out=None, n_points=0), NO_OUT, None),
    ("rsasa_calculate_sasa_batch", "no structure: n_points 0 is no error", dict(S=0, n_points=0), "ok", None),
    ("rsasa_calculate_sasa_batch", "residue offsets past N before n_points", dict(RES, ro="ro_past", n_points=0), RES_EXCEED, None),
    ("rsasa_calculate_sasa_batch", "residue offsets fall before n_points", dict(RES, ro="ro_fall", R=3, n_points=0), RES_ORDER, None),
    ("rsasa_calculate_sasa_batch", "n_points 0 before probe", dict(n_points=0, probe=NAN), POINTS, None),
    ("rsasa_calculate_sasa_batch", "n_points 2^24 + 1", dict(n_points=2 ** 24 + 1), POINTS, None),
    ("rsasa_calculate_sasa_batch", "probe before the span", dict(probe=NAN, so="so_first"), PROBE_MSG, None),
    ("rsasa_calculate_sasa_batch", "probe -1", dict(probe=-1.0), PROBE_MSG, None),
    ("rsasa_calculate_sasa_batch", "0xFFFFFFF0 atoms claimed", dict(so="so_huge"), BATCH_BIG, NOT_RUN),
    ("rsasa_calculate_sasa_batch", "first offset not 0", dict(so="so_first"), SPAN, COMPUTED),
    ("rsasa_calculate_sasa_batch", "span before order", dict(so="so_both", S=2), SPAN, ORDER),
    ("rsasa_calculate_sasa_batch", "offsets fall", dict(so="so_fall", S=2), ORDER, None),
    ("rsasa_calculate_sasa_batch", "pipelined size: first offset not 0", dict(so="piped_first", S=2), SPAN, None),
    ("rsasa_calculate_sasa_batch", "pipelined size: span before order", dict(so="piped_both", S=2), SPAN, NOT_RUN + "; " + ORDER),
    ("rsasa_calculate_sasa_batch", "pipelined size: offsets fall and wrap", dict(so="piped_wrap", S=2), ORDER, NOT_RUN),
    # ---- a stream of host batches: the enqueue takes anything, the wait returns the worker's verdict
    ("rsasa_host_batch_enqueue", "n_points 0", dict(n_points=0), POINTS, None),
    # ---- a trajectory: its seven verdicts, then n_points and probe
    ("rsasa_calculate_sasa_trajectory", "no frame: everything else is not looked at", dict(frames=0, xyz=None, n_points=0), "ok", None),
    ("rsasa_calculate_sasa_trajectory", "xyz NULL before out_residue_sasa", dict(xyz=None, ro="ro", R=2), "xyz / radius are NULL", None),
    ("rsasa_calculate_sasa_trajectory", "out_residue_sasa before sizes", dict(ro="ro", R=2, frames=BIG), RES_OUT, None),
    ("rsasa_calculate_sasa_trajectory", "no output before sizes", dict(out=None, frames=BIG), NO_OUT, None),
    ("rsasa_calculate_sasa_trajectory", "sizes before the residue offsets", dict(RES, ro="ro_past", frames=BIG), TRAJ_BIG, None),
    ("rsasa_calculate_sasa_trajectory", "residue offsets past N before n_points", dict(RES, ro="ro_past", n_points=0), RES_EXCEED, None),
    ("rsasa_calculate_sasa_trajectory", "residue offsets fall before probe", dict(RES, ro="ro_fall", R=3, probe=NAN), RES_ORDER, None),
    ("rsasa_calculate_sasa_trajectory", "n_points 0 before probe", dict(n_points=0, probe=NAN), POINTS, None),
    ("rsasa_calculate_sasa_trajectory", "probe NaN", dict(probe=NAN), PROBE_MSG, None),
    # ---- a device batch: today's order
    ("rsasa_batch_enqueue", "no descriptor before n_points", dict(batch=None, n_points=0), "batch is NULL", None),
    ("rsasa_batch_enqueue", "n_points 0 before probe", dict(n_points=0, probe=NAN), POINTS, None),
    ("rsasa_batch_enqueue", "probe before sizes", dict(probe=NAN, n_atoms=BIG), PROBE_MSG, None),
    ("rsasa_batch_enqueue", "sizes before columns", dict(n_atoms=BIG, x=None), BATCH_BIG, None),
    ("rsasa_batch_enqueue", "columns before the offsets", dict(r=None, so=None), COLS, None),
    ("rsasa_batch_enqueue", "offsets NULL before out_residue_sasa", dict(so=None, ro="d_ro", R=1), "structure_offsets_host is NULL", None),
    ("rsasa_batch_enqueue", "first offset not 0", dict(so="so_first"), SPAN, None),
    ("rsasa_batch_enqueue", "last offset not n_atoms", dict(n_atoms=N + 1), SPAN, None),
    ("rsasa_batch_enqueue", "span before order", dict(so="so_both", S=2), SPAN, None),
    ("rsasa_batch_enqueue", "offsets fall", dict(so="so_fall", S=2), ORDER, None),
    ("rsasa_batch_enqueue", "atoms without structures before out_residue_sasa", dict(S=0, so=None, ro="d_ro", R=1), "atoms without structures", None),
    ("rsasa_batch_enqueue", "residue sums without their output", dict(ro="d_ro", R=1), RES_OUT, None),
    # ---- segment sums: its own rules
    ("rsasa_segment_sums", "no segment: nothing else is looked at", dict(n=0, offsets=None, out=None), "ok", None),
    ("rsasa_segment_sums", "offsets NULL", dict(offsets=None), "NULL argument", None),
    ("rsasa_segment_sums", "out NULL before the last offset", dict(out=None, offsets="ro_past"), "NULL argument", None),
    ("rsasa_segment_sums", "values NULL", dict(values=None), "NULL argument", None),
    ("rsasa_segment_sums", "last offset past n_values", dict(offsets="ro_past"), "offsets exceed n_values", None),
    ("rsasa_segment_sums", "n_values does not fit", dict(n_values=BIG), "offsets exceed n_values", None),
    ("rsasa_segment_sums", "past n_values before order", dict(offsets="seg_fall", n=3, n_values=2), "offsets exceed n_values", None),
    ("rsasa_segment_sums", "offsets fall", dict(offsets="seg_fall", n=3), "offsets must be non-decreasing", None),
]


def row_id(row):
    return f"{row[0][6:]}: {row[1]}"


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_the_first_rule_answers_and_nothing_is_written(world, row):
    from rustsasa_amd import _capi
    lib = _capi.load()
    entry, what, changes, message, _ = row
    defaults, call = ENTRIES[entry]
    v = {k: world.p[val] if isinstance(val, str) else val for k, val in {**defaults, **changes}.items()}
    h = world.ctx._h
    before = lib.rsasa_context_last_error(h).decode()
    rc = getattr(lib, entry)(h, *call(v))
    if entry == "rsasa_host_batch_enqueue":
        assert rc == _capi.RSASA_OK, (what, rc)
        rc = lib.rsasa_host_batch_wait(h)
    got = lib.rsasa_context_last_error(h).decode()
    if message == "ok":
        assert rc == _capi.RSASA_OK and got == before, (entry, what, rc, got)
    else:
        assert rc == _capi.RSASA_ERR_INVALID_ARGUMENT and got == (before if message is BARE else message), (entry, what, rc, got)
    assert world.unwritten(), (entry, what)


def test_a_valid_call_on_the_same_context_equals_the_oracle(world):
    x, y, z, r, ids = world.cols
    got = world.ctx.calculate_sasa_soa(x, y, z, r, ids, PROBE, 100)
    assert np.array_equal(got, po.calculate_sasa_internal(x, y, z, r, ids, PROBE, 100, 8))
    assert world.unwritten()


def test_every_sasa_entry_point_has_rows():
    from rustsasa_amd import _capi
    sasa = {s for s in _capi.SYMBOLS
            if s.startswith("rsasa_calculate_sasa_") or s in ("rsasa_batch_enqueue", "rsasa_host_batch_enqueue", "rsasa_segment_sums")}
    assert len(sasa) == 7 and sasa == set(ENTRIES) == {row[0] for row in ROWS}
    assert all(set(row[2]) <= set(ENTRIES[row[0]][0]) for row in ROWS)  # (a row changes arguments its entry point has)


def test_an_invalid_call_of_pipelined_size_reserves_nothing():
    """structure_offsets that claim 400 M atoms in two structures, with n_points = 0: the rule answers before plan() and
    stage() size the sub-batches' device buffers (2 slots x 5 arrays x 800 MB) by them.  96 MiB: the room
    test_host_stream_under_stress leaves for other tenants' noise."""
    import torch
    import rustsasa_amd
    from rustsasa_amd import _capi
    from rustsasa_amd._capi import ptr
    lib = _capi.load()
    f32 = np.float32
    x, y, z, r = np.array([0.0, 1.5, 3.0], f32), np.zeros(N, f32), np.zeros(N, f32), np.full(N, 1.7, f32)
    with rustsasa_amd.Context(0) as warm:  # (the runtime's own start-up allocations are not this test's)
        warm.calculate_sasa_soa(x, y, z, r, None, PROBE, 100)
    so = np.array([0, 200_000_000, 400_000_000], np.uint32)
    out = np.zeros(N, f32)  # pageable
    with rustsasa_amd.Context(0) as ctx:
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        rc = lib.rsasa_calculate_sasa_batch(ctx._h, ptr(x), ptr(y), ptr(z), ptr(r), None, ptr(so), 2, PROBE, 0, ptr(out), None, 0, None)
        got = lib.rsasa_context_last_error(ctx._h).decode()
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        print(f"free device memory {free0 >> 20} -> {free1 >> 20} MiB")
        assert rc == _capi.RSASA_ERR_INVALID_ARGUMENT and got == POINTS, (rc, got)
        assert free0 - free1 <= 96 * 2 ** 20, f"device memory {free0 >> 20} -> {free1 >> 20} MiB"
        assert not out.any()
