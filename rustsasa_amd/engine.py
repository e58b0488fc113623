"""Python host wrapper over the C ABI: one `Context` per GPU.

Mirrors the reference's free function `calculate_sasa_internal`
(src/lib.rs:249-254) and its directory-mode batching (src/main.rs:375,439).
All compute happens in the HIP library; this module only marshals buffers.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _capi
from ._capi import (ATOM_DTYPE, CROWD_MAX_BINS, CURV_COLUMNS, ENCLOSE_MAX_DIRS, FIELD_MAX_CHANNELS, NEAREST_MAX_K, NEIGHBOR_DTYPE, RADIAL_MAX_BINS,
                    RADIAL_MAX_CLASSES, WITHIN_CENTRE, WITHIN_DTYPE, WITHIN_PARTNER, DeviceBatch, RsasaError, Timings, check,
                    ptr)


def device_count() -> int:
    n = C.c_int(0)
    check(_capi.load().rsasa_device_count(C.byref(n)))
    return n.value


def sphere_points(n_points: int):
    """Golden-section-spiral lattice as uploaded to the GPU (src/lib.rs:43-66)."""
    x = np.empty(n_points, np.float32)
    y = np.empty(n_points, np.float32)
    z = np.empty(n_points, np.float32)
    check(_capi.load().rsasa_sphere_points(n_points, ptr(x), ptr(y), ptr(z)))
    return x, y, z


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _columns(x, y, z, radius, ids, n_expected=None):
    """The SoA columns as contiguous arrays of one common length (the C side sizes every copy from
    the offsets it is given, so a short column would be read past its end)."""
    x, y, z, radius = map(_f32, (x, y, z, radius))
    ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint64)
    n = x.shape[0]
    for name, a in (("x", x), ("y", y), ("z", z), ("radius", radius), ("ids", ids)):
        if a is not None and (a.ndim != 1 or a.shape[0] != n):
            raise ValueError(f"{name} must be a 1-D array of {n} entries (the length of x)")
    if n_expected is not None and n != n_expected:
        raise ValueError(f"the offsets cover {n_expected} atoms but the columns hold {n}")
    return x, y, z, radius, ids


def _offsets(name, off):
    off = np.ascontiguousarray(off, dtype=np.uint32)
    if off.ndim != 1 or off.shape[0] < 1:
        raise ValueError(f"{name} must be a 1-D array of at least one entry")
    return off


def _labels(groups, n):
    """Group labels as a contiguous uint32 array of n entries: integers in [0, 2^32) only (a float or a negative label
    would be another label after conversion)."""
    g = np.asarray(groups)
    if g.dtype.kind not in "ui":
        raise ValueError(f"groups must be an array of integer labels (uint32), not {g.dtype}")
    if g.ndim != 1 or g.shape[0] != n:
        raise ValueError(f"groups must be a 1-D array of {n} entries (one label per atom)")
    if g.dtype != np.uint32 and g.size and (int(g.min()) < 0 or int(g.max()) > 0xFFFFFFFF):
        raise ValueError("group labels must lie in [0, 2^32)")
    return np.ascontiguousarray(g, dtype=np.uint32)


def _flag_bytes(flags, n, name="flags"):
    """The flag bytes of half_sphere_exposure / atoms_within (or, under another name, the class bytes of radial_counts)
    as a contiguous uint8 array of n entries, or None."""
    if flags is None:
        return None
    f = np.asarray(flags)
    if f.dtype.kind not in "ui" or f.shape != (n,):
        raise ValueError(f"{name} must be a 1-D array of {n} integer entries (uint8, one per atom)")
    if f.dtype != np.uint8 and f.size and (int(f.min()) < 0 or int(f.max()) > 0xFF):
        raise ValueError(f"{name} must lie in [0, 256)")
    return np.ascontiguousarray(f, dtype=np.uint8)


def _out_buffer(name, buf, n):
    """A caller-provided output array (e.g. pinned host memory) or a fresh one."""
    if buf is None:
        return np.zeros(n, np.float32)
    if not (isinstance(buf, np.ndarray) and buf.dtype == np.float32 and buf.ndim == 1 and
            buf.shape[0] == n and buf.flags["C_CONTIGUOUS"] and buf.flags["WRITEABLE"]):
        raise ValueError(f"{name} must be a writeable contiguous float32 array of {n} entries")
    return buf


_SINGLE = object()  # in place of structure_offsets: the call goes to the single-structure entry point


class Context:
    """One GPU, one HIP stream, one growable HBM workspace (rsasa_context_t)."""

    def __init__(self, device: int = 0, simd_width: int = 8):
        self._lib = _capi.load()
        h = C.c_void_p()
        check(self._lib.rsasa_context_create(device, C.byref(h)))
        self._h = h
        self.device = device
        if simd_width != 8:
            self.set_simd_width(simd_width)
        self._keepalive = []  # buffers of the batches in flight, oldest first
        self._host_keepalive = []  # the same for host batches (host_batch_enqueue)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rsasa_context_destroy(self._h)  # (waits for queued host batches)
            self._h = None
            self._host_keepalive = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, status):
        check(status, self._h)

    def set_simd_width(self, w: int):
        self._check(self._lib.rsasa_context_set_simd_width(self._h, w))

    def set_call_combining(self, max_wait_us: int = 0):
        """rsasa_context_set_call_combining: per-structure calls of several host threads (ctypes releases the interpreter
        lock during a call) are merged into batch launches; max_wait_us < 0 switches it off."""
        self._check(self._lib.rsasa_context_set_call_combining(self._h, int(max_wait_us)))

    @staticmethod
    def call_combining_stats(device: int = 0):
        """(batches launched, calls merged into them) on `device` since the process started."""
        b, c = C.c_uint64(0), C.c_uint64(0)
        check(_capi.load().rsasa_call_combining_stats(device, C.byref(b), C.byref(c)), None)
        return int(b.value), int(c.value)

    # ---- single structure -------------------------------------------------
    def calculate_sasa_internal(self, atoms: np.ndarray, probe_radius: float = 1.4,
                                n_points: int = 100, threads: int = -1) -> np.ndarray:
        """Drop-in for calculate_sasa_internal(&[Atom], probe, n_points, threads)."""
        atoms = np.ascontiguousarray(atoms, dtype=ATOM_DTYPE)
        out = np.zeros(atoms.shape[0], np.float32)
        self._check(self._lib.rsasa_calculate_sasa_internal(
            self._h, ptr(atoms), atoms.shape[0], probe_radius, n_points, threads, ptr(out)))
        return out

    def calculate_sasa_soa(self, x, y, z, radius, ids=None, probe_radius: float = 1.4,
                           n_points: int = 100) -> np.ndarray:
        x, y, z, radius, ids = _columns(x, y, z, radius, ids)
        out = np.zeros(x.shape[0], np.float32)
        self._check(self._lib.rsasa_calculate_sasa_soa(
            self._h, ptr(x), ptr(y), ptr(z), ptr(radius), ptr(ids), x.shape[0], probe_radius,
            n_points, ptr(out)))
        return out

    # ---- many structures, host buffers -----------------------------------
    def calculate_sasa_batch(self, x, y, z, radius, ids, structure_offsets,
                             probe_radius: float = 1.4, n_points: int = 100,
                             residue_offsets=None, want_atoms: bool = True, atom_out=None,
                             res_out=None):
        """Host buffers in, host buffers out.  `atom_out` / `res_out` may be preallocated float32
        arrays (pinned host memory makes both copy directions asynchronous)."""
        so = _offsets("structure_offsets", structure_offsets)
        n_struct = so.shape[0] - 1
        x, y, z, radius, ids = _columns(x, y, z, radius, ids, int(so[-1]) if n_struct else 0)
        atom_out = _out_buffer("atom_out", atom_out, x.shape[0]) if want_atoms else None
        ro = None
        n_res = 0
        if residue_offsets is not None:
            ro = _offsets("residue_offsets", residue_offsets)
            n_res = ro.shape[0] - 1
            res_out = _out_buffer("res_out", res_out, n_res)
        else:
            res_out = None
        self._check(self._lib.rsasa_calculate_sasa_batch(
            self._h, ptr(x), ptr(y), ptr(z), ptr(radius), ptr(ids), ptr(so), n_struct,
            probe_radius, n_points, ptr(atom_out), ptr(ro), n_res, ptr(res_out)))
        return atom_out, res_out

    # ---- a stream of host batches ------------------------------------------
    def host_batch_enqueue(self, x, y, z, radius, ids, structure_offsets,
                           probe_radius: float = 1.4, n_points: int = 100,
                           residue_offsets=None, want_atoms: bool = True, atom_out=None,
                           res_out=None):
        """rsasa_host_batch_enqueue: as calculate_sasa_batch, but returns once the batch is queued; the results are
        in (atom_out, res_out) - returned here - after the host_batch_wait() that returns this batch.  All arrays
        are kept alive until then; do not touch them in between."""
        so = _offsets("structure_offsets", structure_offsets)
        n_struct = so.shape[0] - 1
        x, y, z, radius, ids = _columns(x, y, z, radius, ids, int(so[-1]) if n_struct else 0)
        atom_out = _out_buffer("atom_out", atom_out, x.shape[0]) if want_atoms else None
        ro = None
        n_res = 0
        if residue_offsets is not None:
            ro = _offsets("residue_offsets", residue_offsets)
            n_res = ro.shape[0] - 1
            res_out = _out_buffer("res_out", res_out, n_res)
        else:
            res_out = None
        self._check(self._lib.rsasa_host_batch_enqueue(
            self._h, ptr(x), ptr(y), ptr(z), ptr(radius), ptr(ids), ptr(so), n_struct,
            probe_radius, n_points, ptr(atom_out), ptr(ro), n_res, ptr(res_out)))
        self._host_keepalive.append((x, y, z, radius, ids, so, ro, atom_out, res_out))
        return atom_out, res_out

    def host_batch_wait(self):
        """Waits for the oldest enqueued host batch and raises its error, if any."""
        try:
            self._check(self._lib.rsasa_host_batch_wait(self._h))
        finally:
            if self._host_keepalive:
                self._host_keepalive.pop(0)

    def host_batch_wait_all(self):
        while self._host_keepalive:
            self.host_batch_wait()

    # ---- neighbour lists and the point runs behind them: one private body per foo / foo_batch pair ----
    def _entry(self, name, x, y, z, radius, ids, structure_offsets):
        """The checked columns of a call of family `name`, and its C entry point with the context and the columns bound:
        rsasa_<name> when structure_offsets is _SINGLE, else rsasa_<name>_batch.  The two signatures differ at one place
        only, behind the columns (and the arguments `before`, if any): (n_atoms, *single) there, (ptr(so), n_struct)
        here.  The other arguments follow."""
        if structure_offsets is _SINGLE:
            so = None
            x, y, z, radius, ids = _columns(x, y, z, radius, ids)
        else:
            so = _offsets("structure_offsets", structure_offsets)
            x, y, z, radius, ids = _columns(x, y, z, radius, ids, int(so[-1]) if so.shape[0] > 1 else 0)

        def call(*args, before=(), single=()):
            fn = getattr(self._lib, "rsasa_" + name + ("" if so is None else "_batch"))
            where = (x.shape[0], *single) if so is None else (ptr(so), so.shape[0] - 1)
            return fn(self._h, ptr(x), ptr(y), ptr(z), ptr(radius), ptr(ids), *before, *where, *args)
        return (x, y, z, radius, ids), call

    def _sized_call(self, call, n_lists: int, guess: int, *dtypes):
        """Runs `call(offsets, *columns, capacity)` with columns of `guess` entries each, and once more at the size the
        offsets give when that was too small; returns (offsets uint64[n_lists + 1], *columns cut to offsets[-1])."""
        offsets = np.zeros(n_lists + 1, np.uint64)
        cols = [np.empty(guess, dt) for dt in dtypes]
        rc = call(offsets, *cols, guess)
        if rc == _capi.RSASA_ERR_BUFFER_TOO_SMALL:
            cols = [np.empty(int(offsets[-1]), dt) for dt in dtypes]
            rc = call(offsets, *cols, cols[0].shape[0])
        self._check(rc)
        return (offsets,) + tuple(c[:int(offsets[-1])] for c in cols)

    # ---- neighbour lists (precompute_neighbors, reference src/lib.rs:69-84) --
    def _precompute_neighbors(self, x, y, z, radius, ids, probe_radius, max_radius, structure_offsets=_SINGLE,
                              active_indices=None):
        (x, *_), entry = self._entry("precompute_neighbors", x, y, z, radius, ids, structure_offsets)
        act = None
        if active_indices is not None:
            act = np.ascontiguousarray(active_indices, dtype=np.uint32)
            if act.ndim != 1:
                raise ValueError("active_indices must be a 1-D array")
        n_lists = x.shape[0] if act is None else act.shape[0]
        mr = float("nan") if max_radius is None else float(max_radius)

        def call(offsets, entries, cap):
            # (single: the active atoms follow n_atoms in rsasa_precompute_neighbors; the batch call has none)
            return entry(probe_radius, mr, ptr(offsets), ptr(entries), cap,
                         single=(ptr(act), 0 if act is None else act.shape[0]))
        return self._sized_call(call, n_lists, 64 * n_lists, NEIGHBOR_DTYPE)

    def precompute_neighbors(self, x, y, z, radius, ids=None, probe_radius: float = 1.4,
                             max_radius: Optional[float] = None, active_indices=None):
        """rsasa_precompute_neighbors: the lists of the active atoms (all atoms when active_indices is None) in CSR form,
        (offsets uint64[n_active + 1], entries NEIGHBOR_DTYPE[total]); each list sorted by (d^2, idx).  max_radius None:
        the largest active radius (NaN radii skipped)."""
        return self._precompute_neighbors(x, y, z, radius, ids, probe_radius, max_radius, active_indices=active_indices)

    def precompute_neighbors_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4,
                                   max_radius: Optional[float] = None):
        """rsasa_precompute_neighbors_batch: one grid per structure; (offsets uint64[n_atoms + 1] over the whole
        batch, entries NEIGHBOR_DTYPE[total]) with idx the index within the structure."""
        return self._precompute_neighbors(x, y, z, radius, ids, probe_radius, max_radius, structure_offsets)

    def neighbor_lists(self, x, y, z, radius, ids=None, probe_radius: float = 1.4,
                       max_radius: Optional[float] = None, active_indices=None):
        """precompute_neighbors as a list of per-atom NEIGHBOR_DTYPE arrays (one per active atom, like Vec<Vec<NeighborData>>)."""
        offsets, entries = self.precompute_neighbors(x, y, z, radius, ids, probe_radius, max_radius, active_indices)
        return [entries[int(offsets[i]):int(offsets[i + 1])] for i in range(offsets.shape[0] - 1)]

    # ---- accessible sphere points (the decisions behind each SASA value, reference src/lib.rs:96-223) ----
    def _accessible_points(self, x, y, z, radius, ids, probe_radius, n_points, structure_offsets=_SINGLE):
        n_points = _n_points(n_points)
        (x, *_), entry = self._entry("accessible_points", x, y, z, radius, ids, structure_offsets)
        words = np.zeros((x.shape[0], _words(n_points)), np.uint32)
        sasa = np.zeros(x.shape[0], np.float32)
        self._check(entry(probe_radius, n_points, ptr(words), ptr(sasa)))
        return words, sasa

    def accessible_points(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, n_points: int = 100):
        """rsasa_accessible_points: (words uint32[N, (n_points + 31) // 32], sasa float32[N]); bit p & 31 of word p >> 5 of
        row i is 1 when point p of sphere_points(n_points) is accessible on atom i.  sasa equals calculate_sasa_soa."""
        return self._accessible_points(x, y, z, radius, ids, probe_radius, n_points)

    def accessible_points_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4,
                                n_points: int = 100):
        """rsasa_accessible_points_batch: accessible_points of every structure (one grid each), rows in batch order."""
        return self._accessible_points(x, y, z, radius, ids, probe_radius, n_points, structure_offsets)

    # ---- exposure vectors (in which direction an atom is exposed: the sum of its accessible lattice points) ----
    def _exposure_vectors(self, x, y, z, radius, ids, probe_radius, n_points, structure_offsets=_SINGLE):
        n_points = _n_points(n_points)
        (x, *_), entry = self._entry("exposure_vectors", x, y, z, radius, ids, structure_offsets)
        vectors = np.zeros((x.shape[0], 3), np.float32)
        free = np.zeros(x.shape[0], np.uint32)
        sasa = np.zeros(x.shape[0], np.float32)
        self._check(entry(probe_radius, n_points, ptr(vectors), ptr(free), ptr(sasa)))
        return vectors, free, sasa

    def exposure_vectors(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, n_points: int = 100):
        """rsasa_exposure_vectors: (vectors float32[N, 3], free uint32[N], sasa float32[N]).  vectors[i] is the float32 sum
        of the points of sphere_points(n_points) that are accessible on atom i, in the fixed order the header gives (a
        tree over each chunk of 64 points, the chunks ascending); free[i] their number, the popcount of
        accessible_points; sasa equals calculate_sasa_soa.  vectors[i] / free[i] is the mean outward direction;
        sas_volume() turns vectors and free into the volume the accessible surface encloses."""
        return self._exposure_vectors(x, y, z, radius, ids, probe_radius, n_points)

    def exposure_vectors_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4,
                               n_points: int = 100):
        """rsasa_exposure_vectors_batch: exposure_vectors of every structure (one grid each), rows in batch order."""
        return self._exposure_vectors(x, y, z, radius, ids, probe_radius, n_points, structure_offsets)

    # ---- atom depth (how far under the accessible surface an atom lies: its nearest accessible dot) ----
    def _atom_depth(self, x, y, z, radius, ids, probe_radius, n_points, structure_offsets=_SINGLE):
        n_points = _n_points(n_points)
        (x, *_), entry = self._entry("atom_depth", x, y, z, radius, ids, structure_offsets)
        depth = np.zeros(x.shape[0], np.float32)
        nearest = np.zeros(x.shape[0], np.uint32)
        free = np.zeros(x.shape[0], np.uint32)
        sasa = np.zeros(x.shape[0], np.float32)
        self._check(entry(probe_radius, n_points, ptr(depth), ptr(nearest), ptr(free), ptr(sasa)))
        return depth, nearest, free, sasa

    def atom_depth(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, n_points: int = 100):
        """rsasa_atom_depth: (depth float32[N], nearest uint32[N], free uint32[N], sasa float32[N]).  depth[i] is the
        float32 distance from atom i's centre to the nearest dot of surface_points() of the structure's accessible
        points, evaluated as the header defines it (plain float32, so it can be checked bit for bit); nearest[i] the atom
        that owns that dot (ties: the smallest index); +inf and 0xFFFFFFFF where there is no such dot.  free[i] is the
        popcount of accessible_points, sasa equals calculate_sasa_soa.  depth - probe_radius estimates the distance to
        the molecular surface; residue_depth() averages depth over residues."""
        return self._atom_depth(x, y, z, radius, ids, probe_radius, n_points)

    def atom_depth_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4, n_points: int = 100):
        """rsasa_atom_depth_batch: atom_depth of every structure (one grid each, dots of other structures never count),
        rows in batch order; nearest holds indices within the atom's structure."""
        return self._atom_depth(x, y, z, radius, ids, probe_radius, n_points, structure_offsets)

    # ---- surface components (which connected piece of accessible surface a free point lies on) ----
    def _surface_components(self, x, y, z, radius, ids, probe_radius, n_points, link, structure_offsets=_SINGLE):
        n_points = _n_points(n_points)
        (x, _, _, radius, _), entry = self._entry("surface_components", x, y, z, radius, ids, structure_offsets)
        link = default_link(radius, probe_radius, n_points) if link is None else link
        free, sasa = np.zeros(x.shape[0], np.uint32), np.zeros(x.shape[0], np.float32)

        def call(offsets, labels, cap):
            return entry(probe_radius, n_points, link, ptr(offsets), ptr(labels), cap, ptr(free), ptr(sasa))
        return self._sized_call(call, x.shape[0], min(n_points, 32) * x.shape[0], np.uint32) + (free, sasa)

    def surface_components(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, n_points: int = 100, link=None):
        """rsasa_surface_components: (dot_offsets uint64[N + 1], labels uint32[dots], free uint32[N], sasa float32[N]).
        The accessible dots (surface_points' rows: atoms in order, each atom's points in lattice order) are numbered
        from 0; two dots no further apart than `link` (float32 d2 <= link * link) are linked, and labels[d] is the
        smallest dot number of d's connected component.  Atom i's dots are [dot_offsets[i], dot_offsets[i + 1]).
        link None: default_link(radius, probe_radius, n_points).  free is the popcount of accessible_points, sasa
        equals calculate_sasa_soa.  component_table() ranks the components, split_sasa() splits each atom's area into
        the largest component's and the rest."""
        return self._surface_components(x, y, z, radius, ids, probe_radius, n_points, link)

    def surface_components_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4,
                                 n_points: int = 100, link=None):
        """rsasa_surface_components_batch: surface_components of every structure (one grid each, dots of different
        structures are never linked).  dot_offsets runs over the whole batch; labels are dot numbers within the
        structure (subtract dot_offsets[structure_offsets[s]] from a position to get one).  link None: default_link of
        the whole batch's radii."""
        return self._surface_components(x, y, z, radius, ids, probe_radius, n_points, link, structure_offsets)

    # ---- dot links (the graph surface_components labels, as per-dot lists) ----
    def _dot_links(self, x, y, z, radius, ids, probe_radius, n_points, link, structure_offsets=_SINGLE):
        n_points = _n_points(n_points)
        (x, _, _, radius, _), entry = self._entry("dot_links", x, y, z, radius, ids, structure_offsets)
        link = default_link(radius, probe_radius, n_points) if link is None else link
        n = x.shape[0]
        free, sasa = np.zeros(n, np.uint32), np.zeros(n, np.float32)
        dot_offsets, n_links = np.zeros(n + 1, np.uint64), np.zeros(1, np.uint64)
        # the first guess: proteins have 4 to 7 accessible dots per atom at 100 points and 8.3 entries per dot at the
        # default link; the second call is sized by what the first one wrote
        dots_cap = min(n_points, 16) * n
        cap = 12 * dots_cap
        for _ in range(2):
            link_offsets, entries = np.zeros(dots_cap + 1, np.uint64), np.empty(cap, WITHIN_DTYPE)
            rc = entry(probe_radius, n_points, link, ptr(dot_offsets), ptr(n_links), ptr(link_offsets), dots_cap,
                       ptr(entries), cap, ptr(free), ptr(sasa))
            if rc != _capi.RSASA_ERR_BUFFER_TOO_SMALL:
                break
            dots_cap, cap = int(dot_offsets[-1]), int(n_links[0])
        self._check(rc)
        return dot_offsets, link_offsets[:int(dot_offsets[-1]) + 1], entries[:int(n_links[0])], free, sasa

    def dot_links(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, n_points: int = 100, link=None):
        """rsasa_dot_links: (dot_offsets uint64[N + 1], link_offsets uint64[D + 1], entries WITHIN_DTYPE[total],
        free uint32[N], sasa float32[N]).  Dots, numbering and the edge test are surface_components': the list of the dot
        at position d, entries[link_offsets[d]:link_offsets[d + 1]], holds every other dot b of its structure with
        float32 d2 <= link * link as (d2, idx = b's dot number within the structure), ascending by (d2, idx); the test
        is symmetric.  link None: default_link(radius, probe_radius, n_points).
        edge_index(link_offsets, entries, dot_structure_offsets(dot_offsets, structure_offsets)) gives the graph's
        int64[2, E]."""
        return self._dot_links(x, y, z, radius, ids, probe_radius, n_points, link)

    def dot_links_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4, n_points: int = 100,
                        link=None):
        """rsasa_dot_links_batch: dot_links of every structure (one grid each, dots of different structures are never
        linked); dot_offsets and link_offsets run over the whole batch, idx is the dot number within the structure."""
        return self._dot_links(x, y, z, radius, ids, probe_radius, n_points, link, structure_offsets)

    # ---- dot geodesics (the shortest distance along that graph from a set of seed dots) ----
    def _dot_geodesics(self, x, y, z, radius, ids, probe_radius, n_points, seeds, limit, link, sources,
                       structure_offsets=_SINGLE):
        n_points = _n_points(n_points)
        (x, _, _, radius, _), entry = self._entry("dot_geodesics", x, y, z, radius, ids, structure_offsets)
        link = default_link(radius, probe_radius, n_points) if link is None else link
        seeds = np.asarray(seeds)
        if seeds.dtype.kind not in "uib" or seeds.ndim != 1:
            raise ValueError("seeds must be a 1-D array of one byte per accessible dot (uint8, nonzero = seed)")
        seeds = np.ascontiguousarray(seeds != 0, dtype=np.uint8)
        limit = float("inf") if limit is None else float(limit)
        if not limit >= 0.0:
            raise ValueError("limit must be None (no limit), +inf or finite, and not negative")
        n, d = x.shape[0], seeds.shape[0]
        free, sasa = np.zeros(n, np.uint32), np.zeros(n, np.float32)
        dot_offsets = np.zeros(n + 1, np.uint64)
        dist = np.zeros(d, np.float32)
        source = np.zeros(d, np.uint32) if sources else None
        self._check(entry(probe_radius, n_points, link, ptr(seeds), d, limit, ptr(dot_offsets), ptr(dist), ptr(source),
                          ptr(free), ptr(sasa)))
        return (dot_offsets, dist, free, sasa) + ((source,) if sources else ())

    def dot_geodesics(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, n_points: int = 100, seeds=None,
                      limit=None, link=None, sources: bool = False):
        """rsasa_dot_geodesics: (dot_offsets uint64[N + 1], dist float32[D], free uint32[N], sasa float32[N]), and
        source uint32[D] behind them with sources=True.  seeds: uint8[D], one byte per accessible dot in the order of
        surface_points(), nonzero = seed (dot_seeds() marks all dots of given atoms); a wrong length raises with D in
        the message.  dist[v] is the minimum over the paths of dot_links' graph from any seed to v of the float32
        left-to-right sum of the edge weights sqrt(d2), over the paths no longer than `limit` (None: no limit); +inf
        where there is none, 0 at a seed.  Any relaxation order converges to these bits, so they can be checked for
        equality.  source[v] is the smallest seed dot number (within the structure) on a path that reaches every vertex
        at exactly its dist, 0xFFFFFFFF where dist is +inf.  link None: default_link(radius, probe_radius, n_points)."""
        return self._dot_geodesics(x, y, z, radius, ids, probe_radius, n_points, seeds, limit, link, sources)

    def dot_geodesics_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4, n_points: int = 100,
                            seeds=None, limit=None, link=None, sources: bool = False):
        """rsasa_dot_geodesics_batch: dot_geodesics of every structure (one grid each, no path crosses structures; all
        structures relax in the same launches); seeds, dist and source run over the dots of the whole batch."""
        return self._dot_geodesics(x, y, z, radius, ids, probe_radius, n_points, seeds, limit, link, sources,
                                   structure_offsets)

    def geodesic_rounds(self):
        """rsasa_context_geodesic_rounds: (rounds for dist, rounds for source) of this context's last dot_geodesics[_batch]
        call, the last round - which changed nothing - included.  A measurement: it varies with the GPU's schedule."""
        rounds = np.zeros(2, np.uint32)
        self._check(self._lib.rsasa_context_geodesic_rounds(self._h, ptr(rounds)))
        return int(rounds[0]), int(rounds[1])

    # ---- dot patches (geodesic farthest-point sampling: where to put the centres of surface patches) ----
    def _dot_patches(self, x, y, z, radius, ids, probe_radius, n_points, spacing, max_centres, link, sources,
                     structure_offsets=_SINGLE):
        n_points = _n_points(n_points)
        (x, _, _, radius, _), entry = self._entry("dot_patches", x, y, z, radius, ids, structure_offsets)
        link = default_link(radius, probe_radius, n_points) if link is None else link
        spacing = float(spacing)
        if not spacing >= 0.0:
            raise ValueError("spacing must be +inf or finite, and not negative")
        max_centres = 0xFFFFFFFF if max_centres is None else int(max_centres)
        if not 1 <= max_centres <= 0xFFFFFFFF:
            raise ValueError("max_centres must be None (no bound) or in [1, 2^32 - 1]")
        n = x.shape[0]
        n_struct = 1 if structure_offsets is _SINGLE else len(structure_offsets) - 1
        free, sasa = np.zeros(n, np.uint32), np.zeros(n, np.float32)
        dot_offsets, bound = np.zeros(n + 1, np.uint64), np.zeros(1, np.uint64)
        centre_offsets = np.zeros(n_struct + 1, np.uint64)
        # the first guess, as in dot_links; the second call is sized by what the first one wrote
        dots_cap = min(n_points, 16) * n
        cap = min(dots_cap, max_centres * n_struct)
        for _ in range(2):
            centres, cover = np.zeros(cap, np.uint32), np.zeros(cap, np.float32)
            dist = np.zeros(dots_cap, np.float32)
            source = np.zeros(dots_cap, np.uint32) if sources else None
            rc = entry(probe_radius, n_points, link, spacing, max_centres, ptr(dot_offsets), ptr(bound), ptr(centre_offsets),
                       ptr(centres), ptr(cover), cap, ptr(dist), ptr(source), dots_cap, ptr(free), ptr(sasa))
            if rc != _capi.RSASA_ERR_BUFFER_TOO_SMALL:
                break
            dots_cap, cap = int(dot_offsets[-1]), int(bound[0])
        self._check(rc)
        d, k = int(dot_offsets[-1]), int(centre_offsets[-1])
        return (dot_offsets, centre_offsets, centres[:k], cover[:k], dist[:d], source[:d] if sources else None, free, sasa)

    def dot_patches(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, n_points: int = 100, spacing: float = 6.0,
                    max_centres=None, link=None, sources: bool = True):
        """rsasa_dot_patches: (dot_offsets uint64[N + 1], centre_offsets uint64[2], centres uint32[K], cover float32[K],
        dist float32[D], source uint32[D] or None, free uint32[N], sasa float32[N]).  Geodesic farthest-point sampling
        of the accessible dots along dot_links' graph: the dot farthest from the centres so far (ties to the smallest
        dot number; a dot at +inf first) becomes the next centre, cover[k] being its distance then, until every dot
        lies within `spacing` of a centre (float32 compare; +inf: one centre per component) or the structure has
        max_centres centres (None: no bound).  dist is dot_geodesics' result for the seed set `centres` with no limit,
        source (sources=False: None) the smallest centre with a tight path - the patch of every dot.  centres and
        source are dot numbers within the structure.  link None: default_link(radius, probe_radius, n_points).
        patch_index() turns source into positions in `centres`, patch_table() sums the patches, dot_seeds_from()
        gives the seed bytes with which dot_geodesics reproduces dist and source."""
        return self._dot_patches(x, y, z, radius, ids, probe_radius, n_points, spacing, max_centres, link, sources)

    def dot_patches_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4, n_points: int = 100,
                          spacing: float = 6.0, max_centres=None, link=None, sources: bool = True):
        """rsasa_dot_patches_batch: dot_patches of every structure, each sampled on its own with max_centres centres at
        most, all in one launch; centre_offsets uint64[S + 1] is batch-global, dist and source run over the dots of the
        whole batch."""
        return self._dot_patches(x, y, z, radius, ids, probe_radius, n_points, spacing, max_centres, link, sources,
                                 structure_offsets)

    def patch_stats(self):
        """rsasa_context_patch_stats: (picks, relaxation steps summed over the structures, picks whose frontier outgrew
        the sampler's queue) of this context's last dot_patches[_batch] call.  A measurement: the last two vary with
        the GPU's schedule."""
        stats = np.zeros(3, np.uint64)
        self._check(self._lib.rsasa_context_patch_stats(self._h, ptr(stats)))
        return int(stats[0]), int(stats[1]), int(stats[2])

    # ---- dot crowding (how much protein lies around each accessible dot, by distance bin) ----
    def _dot_crowding(self, x, y, z, radius, ids, probe_radius, n_points, edges, flags, structure_offsets=_SINGLE):
        n_points = _n_points(n_points)
        (x, *_), entry = self._entry("dot_crowding", x, y, z, radius, ids, structure_offsets)
        n = x.shape[0]
        flags = _flag_bytes(flags, n)
        edges = _f32(edges)
        if edges.ndim != 1 or not 1 <= edges.shape[0] <= CROWD_MAX_BINS:
            raise ValueError(f"edges must be a 1-D array of 1 to {CROWD_MAX_BINS} radii")
        n_bins = edges.shape[0]
        free, sasa = np.zeros(n, np.uint32), np.zeros(n, np.float32)

        def call(offsets, counts, cap):
            return entry(probe_radius, n_points, ptr(flags), ptr(edges), n_bins, ptr(offsets), ptr(counts), cap,
                         ptr(free), ptr(sasa))
        # the first guess of the rows: proteins have 4 to 7 accessible dots per atom at 100 points
        return self._sized_call(call, n, min(n_points, 16) * n, np.dtype((np.uint32, (n_bins,)))) + (free, sasa)

    def dot_crowding(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, n_points: int = 100,
                     edges=(6.0, 8.0, 10.0), flags=None):
        """rsasa_dot_crowding: (dot_offsets uint64[N + 1], counts uint32[D, B], free uint32[N], sasa float32[N]).  The
        rows of counts are the accessible dots in the order of surface_points() and of surface_components' labels: atom
        i's dots are [dot_offsets[i], dot_offsets[i + 1]).  counts[d, b] is the number of atoms j with CROWD_PARTNER in
        flags[j] - the dot's own atom included - whose float32 d2 to the dot lies in bin b, the smallest b with
        d2 <= edges[b] * edges[b], evaluated as the header defines it (plain float32, so the counts can be checked for
        equality).  edges: 1 to CROWD_MAX_BINS radii, finite, not negative, non-decreasing.  flags None: every atom is a
        partner.  np.cumsum(counts, -1)[:, k] is the number of atoms within edges[k] of each dot; dot_means() averages a
        per-dot column over the atoms.  free is the popcount of accessible_points, sasa equals calculate_sasa_soa."""
        return self._dot_crowding(x, y, z, radius, ids, probe_radius, n_points, edges, flags)

    def dot_crowding_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4, n_points: int = 100,
                           edges=(6.0, 8.0, 10.0), flags=None):
        """rsasa_dot_crowding_batch: dot_crowding of every structure (one grid each, atoms of other structures never
        count); dot_offsets and the rows run over the whole batch."""
        return self._dot_crowding(x, y, z, radius, ids, probe_radius, n_points, edges, flags, structure_offsets)

    # ---- dot fields (weighted sums of atom properties around each accessible dot: potentials on the surface) ----
    def _dot_fields(self, x, y, z, radius, ids, probe_radius, n_points, weights, kinds, cutoff, flags, structure_offsets=_SINGLE):
        n_points = _n_points(n_points)
        (x, *_), entry = self._entry("dot_fields", x, y, z, radius, ids, structure_offsets)
        n = x.shape[0]
        flags = _flag_bytes(flags, n)
        if weights is None:
            raise ValueError("weights must be an array of one row per atom")
        weights = _f32(weights)
        if weights.ndim == 1:
            weights = np.ascontiguousarray(weights[:, None])
        if weights.ndim != 2 or weights.shape[0] != n or not 1 <= weights.shape[1] <= FIELD_MAX_CHANNELS:
            raise ValueError(f"weights must be an array of shape ({n},) or ({n}, C) with 1 <= C <= {FIELD_MAX_CHANNELS}")
        n_channels = weights.shape[1]
        k = np.full(n_channels, FIELD_INV_D, np.int64) if kinds is None else np.atleast_1d(np.asarray(kinds))
        if k.dtype.kind not in "ui" or k.shape != (n_channels,) or (k.size and (int(k.min()) < 0 or int(k.max()) > 0xFF)):
            raise ValueError(f"kinds must be {n_channels} integers (one FIELD_* kind per channel of weights)")
        k = np.ascontiguousarray(k, dtype=np.uint8)
        free, sasa = np.zeros(n, np.uint32), np.zeros(n, np.float32)

        def call(offsets, sums, cap):
            return entry(probe_radius, n_points, ptr(flags), ptr(weights), ptr(k), n_channels, cutoff, ptr(offsets), ptr(sums),
                         cap, ptr(free), ptr(sasa))
        return self._sized_call(call, n, min(n_points, 16) * n, np.dtype((np.int64, (n_channels,)))) + (free, sasa)

    def dot_fields(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, n_points: int = 100, weights=None, kinds=None,
                   cutoff: float = 10.0, flags=None):
        """rsasa_dot_fields: (dot_offsets uint64[N + 1], sums int64[D, C], free uint32[N], sasa float32[N]).  The rows of
        sums are the accessible dots in the order of surface_points() and of dot_crowding's rows.  sums[d, c] is the sum
        over the atoms j with FIELD_PARTNER in flags[j] - the dot's own atom included - whose float32 d2 to the dot is at
        most cutoff * cutoff, of rint(weights[j, c] * g * 2^24), where g is 1 (FIELD_STEP), 1 / d (FIELD_INV_D: Coulomb),
        1 / d2 (FIELD_INV_D2) or 1 / (1 + d) (FIELD_INV_1PD: the lipophilic potential) as kinds[c] says, evaluated as the
        header defines it in plain float32; a term that is NaN or above 2^24 in magnitude adds nothing.  The sums are
        integers and wrap, so they have no order and can be checked for equality; field_values() turns them into float64.
        weights: float32[N] (one channel) or [N, C] with C up to FIELD_MAX_CHANNELS; kinds None: every channel FIELD_INV_D;
        cutoff finite and not negative; flags None: every atom is a partner.  dot_means() averages a column over the
        atoms.  free is the popcount of accessible_points, sasa equals calculate_sasa_soa."""
        return self._dot_fields(x, y, z, radius, ids, probe_radius, n_points, weights, kinds, cutoff, flags)

    def dot_fields_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4, n_points: int = 100,
                         weights=None, kinds=None, cutoff: float = 10.0, flags=None):
        """rsasa_dot_fields_batch: dot_fields of every structure (one grid each, atoms of other structures never count);
        dot_offsets and the rows run over the whole batch."""
        return self._dot_fields(x, y, z, radius, ids, probe_radius, n_points, weights, kinds, cutoff, flags, structure_offsets)

    # ---- dot curvature (the moments of the dots around each accessible dot: mean and principal curvatures, shape index) ----
    def _dot_curvature(self, x, y, z, radius, ids, probe_radius, n_points, reach, structure_offsets=_SINGLE):
        n_points = _n_points(n_points)
        (x, *_), entry = self._entry("dot_curvature", x, y, z, radius, ids, structure_offsets)
        n = x.shape[0]
        free, sasa = np.zeros(n, np.uint32), np.zeros(n, np.float32)

        def call(offsets, pairs, moments, cap):
            return entry(probe_radius, n_points, reach, ptr(offsets), ptr(pairs), ptr(moments), cap, ptr(free), ptr(sasa))
        return self._sized_call(call, n, min(n_points, 16) * n, np.dtype(np.uint32), np.dtype((np.int64, (CURV_COLUMNS,)))) + (free, sasa)

    def dot_curvature(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, n_points: int = 100, reach: float = 3.0):
        """rsasa_dot_curvature: (dot_offsets uint64[N + 1], pairs uint32[D], moments int64[D, 8], free uint32[N], sasa
        float32[N]).  The rows are the accessible dots in the order of surface_points().  For dot a with normal n (its
        lattice point) and every other dot b of its structure with float32 d2 <= reach * reach, the header's plain float32
        h = n . (q_b - q_a), t = (q_b - q_a) - h n, g = h / |t|^2 give the terms d2, h and (t t^t) g (CURV_D2, CURV_H,
        CURV_XX .. CURV_YZ); a pair counts - 1 to pairs[a], rint(term * 2^24) to each column of moments[a] - iff d2 > 0,
        |t|^2 > 0 and every |term| <= 2^24, for all columns or for none.  The sums are integers and wrap, so rows can be
        checked for equality; curvature_values() turns them into mean, Gaussian and principal curvatures and the shape
        index.  The mean is robust at any density; the principal split wants about 50 pairs or more per dot (on a lone
        sphere at 100 points and reach 3, k1 R ranges over 1.02 .. 1.41), and dots at the rim of the accessible surface
        see a half-disc.  reach finite and not negative; 0 gives zero rows.  dot_means() averages a column over the
        atoms.  free is the popcount of accessible_points, sasa equals calculate_sasa_soa."""
        return self._dot_curvature(x, y, z, radius, ids, probe_radius, n_points, reach)

    def dot_curvature_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4, n_points: int = 100,
                            reach: float = 3.0):
        """rsasa_dot_curvature_batch: dot_curvature of every structure (one grid each, dots of different structures never
        pair); dot_offsets and the rows run over the whole batch."""
        return self._dot_curvature(x, y, z, radius, ids, probe_radius, n_points, reach, structure_offsets)

    # ---- dot enclosure (in which directions a probe leaving an accessible dot is stopped by protein) ----
    def _dot_enclosure(self, x, y, z, radius, ids, probe_radius, n_points, n_dirs, reach, flags, structure_offsets=_SINGLE):
        n_points = _n_points(n_points)
        (x, *_), entry = self._entry("dot_enclosure", x, y, z, radius, ids, structure_offsets)
        n = x.shape[0]
        flags = _flag_bytes(flags, n)
        n_dirs = int(n_dirs)
        if not 0 <= n_dirs < 2 ** 32:
            raise ValueError("n_dirs must fit an unsigned 32-bit integer")
        free, sasa = np.zeros(n, np.uint32), np.zeros(n, np.float32)

        def call(offsets, blocked, cap):
            return entry(probe_radius, n_points, ptr(flags), reach, n_dirs, ptr(offsets), ptr(blocked), cap, ptr(free), ptr(sasa))
        return self._sized_call(call, n, min(n_points, 16) * n, np.uint32) + (free, sasa)

    def dot_enclosure(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, n_points: int = 100, n_dirs: int = 30,
                      reach: float = 10.0, flags=None):
        """rsasa_dot_enclosure: (dot_offsets uint64[N + 1], blocked uint32[D], free uint32[N], sasa float32[N]).  The
        words of blocked are the accessible dots in the order of surface_points(), of surface_components' labels and of
        dot_crowding's rows.  Bit m of blocked[d] is set when a probe centre leaving dot d along direction m of
        sphere_points(n_dirs) meets, within `reach`, the expanded sphere (radius + probe_radius) of an atom j with
        ENCLOSE_PARTNER in flags[j], or enters the dot's own atom's; the float32 test is the header's, so the words can
        be checked for equality.  n_dirs: 1 to ENCLOSE_MAX_DIRS; reach finite and not negative; flags None: every atom
        is an obstacle.  enclosure_fraction() turns the words into the blocked share, escape_vectors() into the way
        out; dot_means() averages a fraction over the atoms.  free is the popcount of accessible_points, sasa equals
        calculate_sasa_soa."""
        return self._dot_enclosure(x, y, z, radius, ids, probe_radius, n_points, n_dirs, reach, flags)

    def dot_enclosure_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4, n_points: int = 100,
                            n_dirs: int = 30, reach: float = 10.0, flags=None):
        """rsasa_dot_enclosure_batch: dot_enclosure of every structure (one grid each, atoms of other structures stop
        nothing); dot_offsets and the words run over the whole batch."""
        return self._dot_enclosure(x, y, z, radius, ids, probe_radius, n_points, n_dirs, reach, flags, structure_offsets)

    # ---- half-sphere exposure (how many partners lie on either side of an atom, within a cutoff of several cells) ----
    def _half_sphere_exposure(self, x, y, z, radius, ids, probe_radius, dirs, flags, cutoff, structure_offsets=_SINGLE):
        (x, *_), entry = self._entry("half_sphere_exposure", x, y, z, radius, ids, structure_offsets)
        n = x.shape[0]
        if dirs is not None:
            dirs = _f32(dirs)
            if dirs.shape != (n, 3):
                raise ValueError(f"dirs must be an array of shape ({n}, 3) (one direction per atom)")
        flags = _flag_bytes(flags, n)
        up, down = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self._check(entry(probe_radius, ptr(dirs), ptr(flags), cutoff, ptr(up), ptr(down)))
        return up, down

    def half_sphere_exposure(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, dirs=None, flags=None,
                             cutoff: float = 13.0):
        """rsasa_half_sphere_exposure: (up uint32[N], down uint32[N]).  For every atom i with HSE_CENTRE in flags[i], the
        atoms j != i with HSE_PARTNER in flags[j] whose float32 d2 to i is at most cutoff * cutoff, evaluated as the
        header defines it (plain float32, so the counts can be checked for equality): up[i] counts those with
        (c_j - c_i) . dirs[i] >= 0, down[i] the others; atoms that are no centre get 0 / 0.  flags None: every atom is
        centre and partner; dirs None: down is zero and up is the contact number.  radius and probe_radius only fix
        the grid's cell size.  pseudo_cb_directions() gives the HSE-alpha directions of a CA trace."""
        return self._half_sphere_exposure(x, y, z, radius, ids, probe_radius, dirs, flags, cutoff)

    def half_sphere_exposure_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4, dirs=None,
                                   flags=None, cutoff: float = 13.0):
        """rsasa_half_sphere_exposure_batch: half_sphere_exposure of every structure (one grid each, atoms of other
        structures never count), rows in batch order."""
        return self._half_sphere_exposure(x, y, z, radius, ids, probe_radius, dirs, flags, cutoff, structure_offsets)

    # ---- atoms within a cutoff (the lists behind the half-sphere counts) ----
    def _atoms_within(self, x, y, z, radius, ids, probe_radius, flags, cutoff, upper_only, structure_offsets=_SINGLE):
        (x, *_), entry = self._entry("atoms_within", x, y, z, radius, ids, structure_offsets)
        n = x.shape[0]
        flags = _flag_bytes(flags, n)
        cutoff = float(cutoff)
        if not (cutoff >= 0.0) or np.isinf(cutoff):
            raise ValueError("cutoff must be finite and not negative")
        # the first guess of the entries: all-atom lists of proteins hold about 0.2 C^3 entries (19 at 4.5 A, 93 at 8 A,
        # 314 at 13 A), and no list is longer than the largest structure less one
        largest = n if structure_offsets is _SINGLE else int(np.diff(_offsets("structure_offsets", structure_offsets)).max(initial=0))
        n_centres = n if flags is None else int(np.count_nonzero(flags & WITHIN_CENTRE))
        per_list = int(min(max(largest - 1, 0), 0.25 * cutoff ** 3 + 16.0))
        upper = bool(upper_only)

        def call(offsets, entries, cap):
            return entry(probe_radius, ptr(flags), cutoff, int(upper), ptr(offsets), ptr(entries), cap)
        return self._sized_call(call, n, n_centres * per_list // (2 if upper else 1), WITHIN_DTYPE)

    def atoms_within(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, flags=None, cutoff: float = 8.0,
                     upper_only: bool = False):
        """rsasa_atoms_within: (offsets uint64[N + 1], entries WITHIN_DTYPE[total]).  The list of atom i,
        entries[offsets[i]:offsets[i + 1]], holds the atoms j != i with WITHIN_PARTNER in flags[j] whose float32 d2 to i
        is at most cutoff * cutoff (plain float32, as the header defines it), each as (d2, idx), ascending by (d2, idx);
        atoms without WITHIN_CENTRE in flags[i] have an empty list.  flags None: every atom is centre and partner.
        upper_only: only j > i (every pair once).  The list lengths are up + down of half_sphere_exposure.  radius and
        probe_radius only fix the grid's cell size.  edge_index() and closest_pairs() turn the lists into a graph's edges
        and into a contact map between groups of atoms."""
        return self._atoms_within(x, y, z, radius, ids, probe_radius, flags, cutoff, upper_only)

    def atoms_within_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4, flags=None,
                           cutoff: float = 8.0, upper_only: bool = False):
        """rsasa_atoms_within_batch: atoms_within of every structure (one grid each, no list crosses structures);
        offsets over the whole batch, idx the index within the structure."""
        return self._atoms_within(x, y, z, radius, ids, probe_radius, flags, cutoff, upper_only, structure_offsets)

    # ---- the k nearest atoms (the lists within a cutoff, cut at k; the reach follows the atom) ----
    def _nearest_atoms(self, x, y, z, radius, ids, probe_radius, k, flags, cutoff, structure_offsets=_SINGLE):
        (x, *_), entry = self._entry("nearest_atoms", x, y, z, radius, ids, structure_offsets)
        n = x.shape[0]
        flags = _flag_bytes(flags, n)
        if isinstance(k, (bool, float)) or int(k) != k or not 1 <= int(k) <= NEAREST_MAX_K:
            raise ValueError(f"k must be an integer in [1, {NEAREST_MAX_K}]")
        k = int(k)
        cutoff = float("inf") if cutoff is None else float(cutoff)
        if not cutoff >= 0.0:
            raise ValueError("cutoff must be None (no cutoff), +inf or finite, and not negative")
        n_centres = n if flags is None else int(np.count_nonzero(flags & WITHIN_CENTRE))
        cap = n_centres * k  # (always suffices: one call)
        offsets = np.zeros(n + 1, np.uint64)
        entries = np.empty(cap, WITHIN_DTYPE)
        self._check(entry(probe_radius, ptr(flags), k, cutoff, ptr(offsets), ptr(entries), cap))
        return offsets, entries[:int(offsets[-1])]

    def nearest_atoms(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, k: int = 16, flags=None, cutoff=None):
        """rsasa_nearest_atoms: (offsets uint64[N + 1], entries WITHIN_DTYPE[total]).  The list of atom i is the list
        atoms_within defines for it at the same flags and cutoff (upper_only off), cut at k: its first
        min(k, length) entries, ascending by (d2, idx) - the k nearest partners, those with the smaller idx where several
        share the k-th d2.  cutoff None: no cutoff (+inf), whatever the distance.  1 <= k <= NEAREST_MAX_K.  Atoms
        without WITHIN_CENTRE in flags[i] have an empty list; flags None: every atom is centre and partner.  radius and
        probe_radius only fix the grid's cell size.  edge_index() and closest_pairs() work on the result as on
        atoms_within's; nearest_table() gives the dense [N, k] form."""
        return self._nearest_atoms(x, y, z, radius, ids, probe_radius, k, flags, cutoff)

    def nearest_atoms_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4, k: int = 16,
                            flags=None, cutoff=None):
        """rsasa_nearest_atoms_batch: nearest_atoms of every structure (one grid each, no list crosses structures);
        offsets over the whole batch, idx the index within the structure."""
        return self._nearest_atoms(x, y, z, radius, ids, probe_radius, k, flags, cutoff, structure_offsets)

    # ---- radial counts (how many partners of which class in which distance bin; one sweep for every radius) ----
    def _radial_counts(self, x, y, z, radius, ids, probe_radius, edges, classes, n_classes, flags, pairs,
                       structure_offsets=_SINGLE):
        (x, *_), entry = self._entry("radial_counts", x, y, z, radius, ids, structure_offsets)
        n = x.shape[0]
        flags = _flag_bytes(flags, n)
        classes = _flag_bytes(classes, n, "classes")
        if n_classes is None:
            n_classes = 1 if classes is None or not classes.size else int(classes.max()) + 1
        if isinstance(n_classes, (bool, float)) or int(n_classes) != n_classes or not 1 <= int(n_classes) <= RADIAL_MAX_CLASSES:
            raise ValueError(f"n_classes must be an integer in [1, {RADIAL_MAX_CLASSES}]")
        n_classes = int(n_classes)
        edges = _f32(edges)
        if edges.ndim != 1 or not 1 <= edges.shape[0] <= RADIAL_MAX_BINS:
            raise ValueError(f"edges must be a 1-D array of 1 to {RADIAL_MAX_BINS} radii")
        if pairs not in (False, True, "only"):
            raise ValueError('pairs must be False, True or "only"')
        n_bins = edges.shape[0]
        n_struct = 1 if structure_offsets is _SINGLE else _offsets("structure_offsets", structure_offsets).shape[0] - 1
        counts = None if pairs == "only" else np.zeros((n, n_classes, n_bins), np.uint32)
        table = np.zeros((n_struct, n_classes, n_classes, n_bins), np.uint64) if pairs else None
        self._check(entry(probe_radius, ptr(flags), ptr(classes), n_classes, ptr(edges), n_bins, ptr(counts), ptr(table)))
        return table if pairs == "only" else (counts, table) if pairs else counts

    def radial_counts(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, edges=(6.0, 8.0, 10.0, 12.0),
                      classes=None, n_classes=None, flags=None, pairs=False):
        """rsasa_radial_counts: counts uint32[N, C, B].  counts[i, b, k] is the number of atoms j != i with RADIAL_PARTNER
        in flags[j] and classes[j] == b whose float32 d2 to i lies in bin k - the smallest k with d2 <= edges[k] *
        edges[k], evaluated as the header defines it (plain float32, so the counts can be checked for equality) - for
        every atom i with RADIAL_CENTRE in flags[i]; the other rows are zero.  edges: 1 to RADIAL_MAX_BINS radii, finite,
        not negative, non-decreasing.  classes: a byte per atom below n_classes (None: everybody is class 0); n_classes
        None: max(classes) + 1.  flags None: every atom is centre and partner.  pairs=True: (counts, table) with table
        uint64[1, C, C, B], table[0, a, b, k] the sum of counts[i, b, k] over the centres i of class a (the pair-distance
        histogram by class pair); pairs="only": the table alone, and no row crosses to the host.  np.cumsum(counts, -1)
        .sum(1)[:, k] is the contact number at edges[k]; radial_density() divides by the shells' volumes.  radius and
        probe_radius only fix the grid's cell size."""
        return self._radial_counts(x, y, z, radius, ids, probe_radius, edges, classes, n_classes, flags, pairs)

    def radial_counts_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4,
                            edges=(6.0, 8.0, 10.0, 12.0), classes=None, n_classes=None, flags=None, pairs=False):
        """rsasa_radial_counts_batch: radial_counts of every structure (one grid each, atoms of other structures never
        count), rows in batch order; the pair tables are uint64[S, C, C, B], one per structure."""
        return self._radial_counts(x, y, z, radius, ids, probe_radius, edges, classes, n_classes, flags, pairs,
                                   structure_offsets)

    # ---- contact counts (which neighbour buries which points, reference src/lib.rs:129-146,183-207) ----
    def _contact_points(self, x, y, z, radius, ids, probe_radius, n_points, structure_offsets=_SINGLE):
        n_points = _n_points(n_points)
        (x, *_), entry = self._entry("contact_points", x, y, z, radius, ids, structure_offsets)
        sasa = np.zeros(x.shape[0], np.float32)

        def call(offsets, entries, covered, exclusive, cap):
            return entry(probe_radius, n_points, ptr(offsets), ptr(entries), ptr(covered), ptr(exclusive), cap, ptr(sasa))
        return self._sized_call(call, x.shape[0], 64 * x.shape[0], NEIGHBOR_DTYPE, np.uint32, np.uint32) + (sasa,)

    def contact_points(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, n_points: int = 100):
        """rsasa_contact_points: (offsets uint64[N + 1], entries NEIGHBOR_DTYPE[total], covered uint32[total],
        exclusive uint32[total], sasa float32[N]).  offsets / entries are precompute_neighbors(max_radius=None); for
        entry e of atom i's list, covered[e] counts the points of sphere_points(n_points) on atom i that the entry
        occludes, exclusive[e] those that no other entry of the list occludes.  sasa equals calculate_sasa_soa;
        contact_areas() turns counts into A^2."""
        return self._contact_points(x, y, z, radius, ids, probe_radius, n_points)

    def contact_points_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4,
                             n_points: int = 100):
        """rsasa_contact_points_batch: contact_points of every structure (one grid each); offsets over the whole batch,
        idx the index within the structure."""
        return self._contact_points(x, y, z, radius, ids, probe_radius, n_points, structure_offsets)

    # ---- contact owners (every buried point given to one neighbour: an additive split of the buried points) ----
    def _contact_owners(self, x, y, z, radius, ids, probe_radius, n_points, points, structure_offsets=_SINGLE):
        n_points = _n_points(n_points)
        (x, *_), entry = self._entry("contact_owners", x, y, z, radius, ids, structure_offsets)
        sasa = np.zeros(x.shape[0], np.float32)
        owner = np.full((x.shape[0], n_points), 0xFFFFFFFF, np.uint32) if points else None

        def call(offsets, entries, owned, cap):
            return entry(probe_radius, n_points, ptr(offsets), ptr(entries), ptr(owned), cap, ptr(owner), ptr(sasa))
        out = self._sized_call(call, x.shape[0], 64 * x.shape[0], NEIGHBOR_DTYPE, np.uint32) + (sasa,)
        return out + (owner,) if points else out

    def contact_owners(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, n_points: int = 100,
                       points: bool = False):
        """rsasa_contact_owners: (offsets uint64[N + 1], entries NEIGHBOR_DTYPE[total], owned uint32[total],
        sasa float32[N]), and with points=True also owner uint32[N, n_points].  offsets / entries / sasa are those of
        contact_points.  Every point of sphere_points(n_points) on atom i that some entry of its list occludes belongs
        to ONE entry, the hitting entry with the smallest margin dot - limit in float32 (the power distance of the point
        to the neighbour's expanded sphere; the earlier list position on an exact tie): owned[e] counts the points entry
        e owns, so the owned counts of an atom add up to n_points minus its accessible points, and
        exclusive <= owned <= covered entry by entry.  owner[i, p] is the owner's position in atom i's list - the
        neighbour is entries[offsets[i] + owner[i, p]] - or 0xFFFFFFFF for an accessible point.  contact_areas() turns
        owned into A^2; owner_areas() sums it into an additive group x group table."""
        return self._contact_owners(x, y, z, radius, ids, probe_radius, n_points, points)

    def contact_owners_batch(self, x, y, z, radius, ids, structure_offsets, probe_radius: float = 1.4,
                             n_points: int = 100, points: bool = False):
        """rsasa_contact_owners_batch: contact_owners of every structure (one grid each); offsets over the whole batch,
        idx the index within the structure, owner rows in batch order."""
        return self._contact_owners(x, y, z, radius, ids, probe_radius, n_points, points, structure_offsets)

    # ---- group contacts (which partner group buries which points: unions of the same tests over a label's entries) ----
    def _group_contacts(self, x, y, z, radius, ids, groups, probe_radius, n_points, structure_offsets=_SINGLE):
        n_points = _n_points(n_points)
        (x, *_), entry = self._entry("group_contacts", x, y, z, radius, ids, structure_offsets)
        groups = _labels(groups, x.shape[0])
        self_free, free = np.zeros(x.shape[0], np.uint32), np.zeros(x.shape[0], np.uint32)
        sasa = np.zeros(x.shape[0], np.float32)

        def call(offsets, partner, buried, only, cap):
            # (before: the labels sit between the columns and n_atoms / structure_offsets in both signatures)
            return entry(probe_radius, n_points, ptr(offsets), ptr(partner), ptr(buried), ptr(only), cap, ptr(self_free),
                         ptr(free), ptr(sasa), before=(ptr(groups),))
        return self._sized_call(call, x.shape[0], 16 * x.shape[0], np.uint32, np.uint32, np.uint32) + (self_free, free, sasa)

    def group_contacts(self, x, y, z, radius, ids, groups, probe_radius: float = 1.4, n_points: int = 100):
        """rsasa_group_contacts: (offsets uint64[N + 1], partner_groups uint32[rows], buried uint32[rows],
        only uint32[rows], self_free uint32[N], free uint32[N], sasa float32[N]).  groups: a uint32 label per atom
        (chain, residue, ligand).  Atom i has one row per distinct foreign label in its neighbour list, ascending:
        buried = the points of sphere_points(n_points) on atom i that the label's atoms occlude among those atom i's own
        group leaves free (self_free of them), only = those no other foreign label occludes; free = the accessible
        points in the whole structure, sasa equals calculate_sasa_soa.  group_areas() sums rows into a group x group
        table of A^2."""
        return self._group_contacts(x, y, z, radius, ids, groups, probe_radius, n_points)

    def group_contacts_batch(self, x, y, z, radius, ids, groups, structure_offsets, probe_radius: float = 1.4,
                             n_points: int = 100):
        """rsasa_group_contacts_batch: group_contacts of every structure (one grid each), offsets over the whole batch;
        labels are compared within a structure only, so their values may be reused from one structure to the next."""
        return self._group_contacts(x, y, z, radius, ids, groups, probe_radius, n_points, structure_offsets)

    def surface_points(self, x, y, z, radius, ids=None, probe_radius: float = 1.4, n_points: int = 100):
        """The accessible points themselves: (atom_index uint32[M], xyz float32[M, 3]), see surface_points()."""
        words, _ = self.accessible_points(x, y, z, radius, ids, probe_radius, n_points)
        return surface_points(words, x, y, z, radius, probe_radius, n_points)

    # ---- MD trajectory: one topology, many frames --------------------------
    def calculate_sasa_trajectory(self, xyz, radius, ids=None, probe_radius: float = 1.4,
                                  n_points: int = 100, residue_offsets=None, want_atoms: bool = True):
        """xyz: [n_frames, n_atoms, 3] float32 (frame-major); returns ([F, N] atom values or None,
        [F, R] residue sums or None)."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        if xyz.ndim != 3 or xyz.shape[2] != 3:
            raise ValueError("xyz must have shape [n_frames, n_atoms, 3]")
        n_frames, n_atoms = xyz.shape[0], xyz.shape[1]
        radius = _f32(radius)
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint64)
        for name, a in (("radius", radius), ("ids", ids)):
            if a is not None and (a.ndim != 1 or a.shape[0] != n_atoms):
                raise ValueError(f"{name} must be a 1-D array of {n_atoms} entries")
        atom_out = np.zeros((n_frames, n_atoms), np.float32) if want_atoms else None
        ro = res_out = None
        n_res = 0
        if residue_offsets is not None:
            ro = np.ascontiguousarray(residue_offsets, dtype=np.uint32)
            n_res = ro.shape[0] - 1
            res_out = np.zeros((n_frames, n_res), np.float32)
        self._check(self._lib.rsasa_calculate_sasa_trajectory(
            self._h, ptr(xyz), n_frames, n_atoms, ptr(radius), ptr(ids), probe_radius, n_points,
            ptr(atom_out), ptr(ro), n_res, ptr(res_out)))
        return atom_out, res_out

    # ---- many structures, buffers already in HBM --------------------------
    def enqueue_device(self, x, y, z, radius, ids, structure_offsets_host: np.ndarray,
                       out_atom_sasa=None, residue_offsets=None, out_residue_sasa=None,
                       out_neighbor_counts=None, probe_radius: float = 1.4, n_points: int = 100,
                       stream: Optional[int] = None):
        """Enqueue one batch whose arrays are torch CUDA(=HIP) tensors.

        `stream` is a raw hipStream_t value (e.g. torch.cuda.current_stream().cuda_stream);
        None uses the context's own streams.  Up to two batches may be in flight (the library gives
        each its own workspace; a third enqueue first waits for the oldest): wait() waits for the
        OLDEST batch in flight, so enqueue(k + 1) followed by wait() returns batch k's results.
        """
        so = np.ascontiguousarray(structure_offsets_host, dtype=np.uint32)

        def dp(t):
            return None if t is None else t.data_ptr()

        b = DeviceBatch()
        b.x, b.y, b.z, b.radius = dp(x), dp(y), dp(z), dp(radius)
        b.id = dp(ids)
        b.structure_offsets_host = so.ctypes.data
        b.n_structures = so.shape[0] - 1
        b.n_atoms = int(x.shape[0])
        b.residue_offsets = dp(residue_offsets)
        b.n_residues = 0 if residue_offsets is None else int(residue_offsets.shape[0]) - 1
        b.out_atom_sasa = dp(out_atom_sasa)
        b.out_residue_sasa = dp(out_residue_sasa)
        b.out_neighbor_counts = dp(out_neighbor_counts)
        # The library may re-run a batch from its wait(): a batch's buffers stay alive until it has been
        # waited for.  With two batches already in flight rsasa_batch_enqueue waits for the oldest itself.
        keep = (so, x, y, z, radius, ids, residue_offsets, out_atom_sasa, out_residue_sasa,
                out_neighbor_counts)
        full = len(self._keepalive) >= 2
        try:
            self._check(self._lib.rsasa_batch_enqueue(self._h, C.byref(b), probe_radius, n_points,
                                                      C.c_void_p(stream) if stream else None))
        finally:
            if full:
                self._keepalive.pop(0)
        self._keepalive.append(keep)

    def wait(self):
        """Waits for the oldest batch in flight (no batch in flight: returns at once)."""
        try:
            self._check(self._lib.rsasa_batch_wait(self._h))
        finally:
            if self._keepalive:
                self._keepalive.pop(0)

    def wait_all(self):
        while self._keepalive:
            self.wait()

    # ---- measurement -------------------------------------------------------
    def enable_timing(self, enable: bool = True):
        self._check(self._lib.rsasa_context_enable_timing(self._h, 1 if enable else 0))

    def timings(self) -> dict:
        t = Timings()
        self._check(self._lib.rsasa_context_get_timings(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in Timings._fields_}

    def ids_kept(self) -> int:
        """Structures of the context's last checked (sub-)batch that kept their ids (rsasa_context_ids_kept)."""
        n = C.c_uint64(0)
        self._check(self._lib.rsasa_context_ids_kept(self._h, C.byref(n)))
        return int(n.value)

    def ids_dropped(self) -> int:
        """(Sub-)batches that ran without their ids because the ids of every structure increased strictly
        (rsasa_context_ids_dropped)."""
        n = C.c_uint64(0)
        self._check(self._lib.rsasa_context_ids_dropped(self._h, C.byref(n)))
        return int(n.value)


def _n_points(n_points) -> int:
    n = int(n_points)
    if n != n_points or n < 1:
        raise ValueError(f"n_points must be a positive integer, not {n_points!r}")
    return n


def _words(n_points: int) -> int:
    return (n_points + 31) // 32


def unpack_points(words, n_points: int) -> np.ndarray:
    """Masks of accessible_points as bool[N, n_points] (column p: point p of sphere_points(n_points))."""
    n_points = _n_points(n_points)
    words = np.ascontiguousarray(words, dtype="<u4")
    if words.ndim != 2 or words.shape[1] != _words(n_points):
        raise ValueError(f"words must have shape [N, {_words(n_points)}] for {n_points} points")
    bits = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")
    return bits[:, :n_points].astype(bool)


def surface_points(words, x, y, z, radius, probe_radius: float = 1.4, n_points: int = 100):
    """The accessible points of masks `words` (accessible_points of these columns): (atom_index uint32[M],
    xyz float32[M, 3]), atoms in order and each atom's points in lattice order.  A point is c + R * s in float32
    (no FMA), R = radius + probe_radius, s the point of sphere_points(n_points) - the reference's sphere
    (src/lib.rs:101, 43-66)."""
    mask = unpack_points(words, n_points)
    x, y, z, radius, _ = _columns(x, y, z, radius, None)
    if x.shape[0] != mask.shape[0]:
        raise ValueError(f"words has {mask.shape[0]} rows but the columns hold {x.shape[0]} atoms")
    atom, p = np.nonzero(mask)
    sx, sy, sz = sphere_points(n_points)
    R = radius[atom] + np.float32(probe_radius)
    xyz = np.empty((atom.shape[0], 3), np.float32)
    for k, (c, s) in enumerate(((x, sx), (y, sy), (z, sz))):
        xyz[:, k] = c[atom] + R * s[p]
    return atom.astype(np.uint32), xyz


def residue_depth(depth, residue_offsets):
    """Residue depth: the float64 mean of the atom depths (atom_depth[_batch]) of every residue, residue r being atoms
    [residue_offsets[r], residue_offsets[r + 1]); NaN for an empty residue.  Host arithmetic: each residue's depths are
    added in float64 in atom order and divided by their number (an atom at +inf makes its residue +inf)."""
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    ro = np.asarray(residue_offsets)
    if ro.dtype.kind not in "ui":
        raise ValueError(f"residue_offsets must be an array of integers, not {ro.dtype}")
    ro = ro.astype(np.int64)
    if depth.ndim != 1 or ro.ndim != 1 or ro.shape[0] < 1:
        raise ValueError("depth and residue_offsets must be 1-D arrays, residue_offsets of at least one entry")
    if ro[0] < 0 or (np.diff(ro) < 0).any() or ro[-1] > depth.shape[0]:
        raise ValueError("residue_offsets must be non-decreasing and stay within depth")
    out = np.full(ro.shape[0] - 1, np.nan, np.float64)
    for r in range(ro.shape[0] - 1):
        b, e = int(ro[r]), int(ro[r + 1])
        if e > b:
            total = 0.0
            for v in depth[b:e].astype(np.float64):
                total += float(v)
            out[r] = total / (e - b)
    return out


HSE_PARTNER = 1  # flag bits of half_sphere_exposure: the atom is counted / the atom gets a result
HSE_CENTRE = 2


RADIAL_PARTNER = 1  # flag bits of radial_counts (those of half_sphere_exposure)
RADIAL_CENTRE = 2


CROWD_PARTNER = 1  # flag bit of dot_crowding: the atom is counted


ENCLOSE_PARTNER = 1  # flag bit of dot_enclosure: the atom is an obstacle


FIELD_PARTNER = 1  # flag bit of dot_fields: the atom contributes
FIELD_STEP, FIELD_INV_D, FIELD_INV_D2, FIELD_INV_1PD = 0, 1, 2, 3  # the distance kernels of dot_fields: 1, 1 / d, 1 / d2, 1 / (1 + d)
FIELD_FRACTION_BITS = 24  # the sums of dot_fields are fixed point: value = sum * 2^-24


def field_values(sums) -> np.ndarray:
    """float64, the shape of sums: the fields of dot_fields[_batch] as numbers, sums * 2^-24 (exact up to 2^53)."""
    s = np.asarray(sums)
    if s.dtype != np.int64:
        raise ValueError("sums must be the int64 array dot_fields returns")
    return s.astype(np.float64) * 2.0 ** -FIELD_FRACTION_BITS


CURV_D2, CURV_H, CURV_XX, CURV_YY, CURV_ZZ, CURV_XY, CURV_XZ, CURV_YZ = range(8)  # the columns of dot_curvature's moments


def curvature_values(pairs, moments, directions=False, normals=None):
    """float64[D] each: (mean, gaussian, k1, k2, shape_index) of the rows dot_curvature[_batch] returns.
    mean = -2 Sum(h) / Sum(d2), the least-squares normal curvature (positive on convex surface).  The six moment columns
    give Taubin's tensor M = -2 Sum(h T T^t) / Sum(d2); its tangential eigenvalues m1 >= m2 follow from the trace and the
    Frobenius norm alone, (tr M +- sqrt(2 |M|_F^2 - tr^2)) / 2, and k1 = 3 m1 - m2 >= k2 = 3 m2 - m1 are the principal
    curvatures (k1 + k2 = 2 tr M); gaussian = k1 k2; shape_index = (2 / pi) atan2(k1 + k2, k1 - k2): +1 a convex cap, 0 a
    saddle, -1 a cup.  All NaN where pairs == 0 or Sum(d2) == 0.  The mean is robust at any density; the split of k1 and
    k2 wants about 50 pairs or more (see dot_curvature).
    directions=True: two more results, float64[D, 3] each - the unit principal directions of k1 and k2 (sign free).  With
    normals (float[D, 3]: the dots' outward normals, which are their lattice points - sphere_points(n_points)[k] of the
    accessible points in dot order, or (q - c) / (r + probe) from surface_points) the tensor is restricted to the plane
    orthogonal to each normal and numpy.linalg.eigh solves the 2 x 2 problem there: the directions are tangential
    whatever the curvatures.  Without them eigh runs on the 3 x 3 tensor and, of its three eigenvectors, the one whose
    eigenvalue is smallest in magnitude is taken for the normal (M n ~ 0): where m1 or m2 is itself near 0 - flat or
    parabolic dots - that choice is not determined, and a returned direction can be the normal; pass normals there."""
    p, s = np.asarray(pairs), np.asarray(moments)
    if s.dtype != np.int64 or s.ndim != 2 or s.shape[1] != CURV_COLUMNS or p.shape != s.shape[:1]:
        raise ValueError("pairs and moments must be the uint32[D] and int64[D, 8] arrays dot_curvature returns")
    ok = (p != 0) & (s[:, CURV_D2] != 0)
    v = s.astype(np.float64)          # (the scale 2^-24 cancels in every ratio)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(ok, -2.0 / v[:, CURV_D2], np.nan)
        mean = w * v[:, CURV_H]
        m = w[:, None] * v[:, CURV_XX:]
        tr = m[:, 0] + m[:, 1] + m[:, 2]
        fro2 = m[:, 0] ** 2 + m[:, 1] ** 2 + m[:, 2] ** 2 + 2.0 * (m[:, 3] ** 2 + m[:, 4] ** 2 + m[:, 5] ** 2)
        root = np.sqrt(np.maximum(2.0 * fro2 - tr * tr, 0.0))
        m1, m2 = (tr + root) / 2.0, (tr - root) / 2.0
        k1, k2 = 3.0 * m1 - m2, 3.0 * m2 - m1
        out = (mean, k1 * k2, k1, k2, (2.0 / np.pi) * np.arctan2(k1 + k2, k1 - k2))
    if not directions:
        return out
    d1, d2 = np.full((len(p), 3), np.nan), np.full((len(p), 3), np.nan)
    rows = np.flatnonzero(ok)
    if normals is not None:
        nrm = np.asarray(normals, np.float64)
        if nrm.shape != (len(p), 3):
            raise ValueError(f"normals must be an array of shape ({len(p)}, 3): one outward normal per dot")
    if len(rows):
        t = np.empty((len(rows), 3, 3))
        for (i, j), c in zip(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)), range(6)):
            t[:, i, j] = t[:, j, i] = m[rows, c]
        at = np.arange(len(rows))
        if normals is None:
            val, vec = np.linalg.eigh(t)                               # ascending eigenvalues, unit eigenvectors in columns
            normal = np.argmin(np.abs(val), axis=1)
            keep = np.array([[1, 2], [0, 2], [0, 1]])[normal]          # the other two, ascending: (m2, m1)
            d1[rows], d2[rows] = vec[at, :, keep[:, 1]], vec[at, :, keep[:, 0]]
        else:
            n = nrm[rows] / np.linalg.norm(nrm[rows], axis=1, keepdims=True)
            axis = np.eye(3)[np.argmin(np.abs(n), axis=1)]             # the coordinate axis least along the normal
            e1 = np.cross(n, axis)
            e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
            e2 = np.cross(n, e1)
            basis = np.stack([e1, e2], -1)                             # [rows, 3, 2]: an orthonormal basis of the tangent plane
            val, vec = np.linalg.eigh(np.swapaxes(basis, 1, 2) @ t @ basis)
            d1[rows] = (basis @ vec[:, :, 1:2])[:, :, 0]               # ascending: column 1 belongs to m1, column 0 to m2
            d2[rows] = (basis @ vec[:, :, 0:1])[:, :, 0]
    return out + (d1, d2)


def _blocked_bits(blocked, n_dirs):
    """bool[D, n_dirs]: the bits of dot_enclosure's words, checked."""
    b = np.asarray(blocked)
    n_dirs = int(n_dirs)
    if not 1 <= n_dirs <= ENCLOSE_MAX_DIRS:
        raise ValueError(f"n_dirs must lie in [1, {ENCLOSE_MAX_DIRS}]")
    if b.ndim != 1 or b.dtype != np.uint32:
        raise ValueError("blocked must be a 1-D uint32 array")
    if n_dirs < 32 and (b >> np.uint32(n_dirs)).any():
        raise ValueError("blocked has bits set at or above n_dirs")
    return ((b[:, None] >> np.arange(n_dirs, dtype=np.uint32)[None, :]) & np.uint32(1)).astype(bool)


def enclosure_fraction(blocked, n_dirs) -> np.ndarray:
    """float64[D]: the share of the n_dirs directions of dot_enclosure that are blocked, popcount / n_dirs - 0 on an open
    knob, 1 for a dot that is sealed in.  dot_means() averages it over the atoms."""
    return _blocked_bits(blocked, n_dirs).sum(axis=1).astype(np.float64) / int(n_dirs)


def escape_vectors(blocked, n_dirs) -> np.ndarray:
    """float64[D, 3]: for every dot the sum of the FREE directions of sphere_points(n_dirs) - the way out of a pocket;
    zero for a dot that is sealed in.  Summed in float64 in direction order on the host."""
    free = ~_blocked_bits(blocked, n_dirs)
    u = np.stack([np.asarray(a, np.float64) for a in sphere_points(int(n_dirs))], -1)
    out = np.zeros((free.shape[0], 3), np.float64)
    for m in range(int(n_dirs)):
        out[free[:, m]] += u[m]
    return out


def dot_means(dot_offsets, values) -> np.ndarray:
    """float64[N]: for every atom the mean of a per-dot column (dot_crowding's cumulative counts at one edge, say, or
    anything else with one entry per dot) over its dots [dot_offsets[i], dot_offsets[i + 1]), NaN for an atom without
    dots.  Summed in float64 in dot order on the host."""
    off = np.ascontiguousarray(dot_offsets, dtype=np.uint64).astype(np.int64)
    v = np.asarray(values)
    if off.ndim != 1 or off.shape[0] < 1 or off[0] != 0 or (np.diff(off) < 0).any():
        raise ValueError("dot_offsets must be non-decreasing from 0")
    if v.ndim != 1 or v.shape[0] != int(off[-1]):
        raise ValueError(f"values must be a 1-D array of dot_offsets[-1] = {int(off[-1])} entries")
    v = v.astype(np.float64)
    out = np.full(off.shape[0] - 1, np.nan, np.float64)
    for i in range(off.shape[0] - 1):
        b, e = int(off[i]), int(off[i + 1])
        if e > b:
            total = 0.0
            for x in v[b:e]:
                total += float(x)
            out[i] = total / (e - b)
    return out


def radial_density(counts, edges) -> np.ndarray:
    """The counts of radial_counts[_batch] (any array whose last axis runs over the bins) as number densities, float64
    of the same shape: every count divided by the volume of its shell, 4/3 pi (e_k^3 - e_(k-1)^3) with e_(-1) = 0.  An
    empty shell (equal edges, or a first edge of 0) gives NaN.  Host arithmetic in float64."""
    c = np.asarray(counts)
    e = np.asarray(edges, dtype=np.float64)
    if e.ndim != 1 or c.ndim < 1 or c.shape[-1] != e.shape[0]:
        raise ValueError("edges must be 1-D with one radius per bin of counts' last axis")
    if e.size and (not np.isfinite(e).all() or e[0] < 0 or (np.diff(e) < 0).any()):
        raise ValueError("edges must be finite, not negative and non-decreasing")
    volume = 4.0 / 3.0 * np.pi * np.diff(e ** 3, prepend=0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(volume > 0.0, c.astype(np.float64) / volume, np.nan)


def pseudo_cb_directions(ca_xyz, chain_offsets) -> np.ndarray:
    """The HSE-alpha directions of a CA trace, float32[N, 3]: for every CA that has both chain neighbours, the sum of
    the unit vectors from CA(i - 1) and from CA(i + 1) towards CA(i) (it points roughly where the side chain does).
    ca_xyz is [N, 3]; chain c is rows [chain_offsets[c], chain_offsets[c + 1]).  Chain ends (and chains of fewer than
    three atoms) get a zero vector, and so does the share of a neighbour that coincides with the atom.  Host
    arithmetic in float64, rounded once at the end."""
    ca = np.asarray(ca_xyz, dtype=np.float64)
    off = np.asarray(chain_offsets, dtype=np.int64)
    if ca.ndim != 2 or ca.shape[1] != 3:
        raise ValueError("ca_xyz must be an array of shape (N, 3)")
    if off.ndim != 1 or off.shape[0] < 1 or off[0] != 0 or off[-1] != ca.shape[0] or np.any(np.diff(off) < 0):
        raise ValueError("chain_offsets must be non-decreasing from 0 to N")
    n = ca.shape[0]
    out = np.zeros((n, 3), np.float64)
    interior = np.ones(n, bool)
    interior[off[:-1][off[:-1] < n]] = False  # (an empty chain's offset is its successor's first atom, or N)
    interior[off[1:][off[1:] > 0] - 1] = False
    i = np.flatnonzero(interior)
    for nb in (i - 1, i + 1):
        d = ca[i] - ca[nb]
        length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        ok = length > 0.0
        out[i[ok]] += d[ok] / length[ok, None]
    return out.astype(np.float32)


def _within_pairs(offsets, entries, structure_offsets):
    """(centre, partner) int64 batch-global atom indices of every entry of atoms_within[_batch]'s lists."""
    off = np.asarray(offsets).astype(np.int64)
    if off.ndim != 1 or off.shape[0] < 1 or off[0] != 0 or (np.diff(off) < 0).any():
        raise ValueError("offsets must be non-decreasing from 0")
    ent = np.asarray(entries)
    if ent.dtype != WITHIN_DTYPE or ent.ndim != 1 or ent.shape[0] != off[-1]:
        raise ValueError("entries must be a WITHIN_DTYPE array of offsets[-1] entries")
    n = off.shape[0] - 1
    centre = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    return centre, _structure_base(n, structure_offsets)[centre] + ent["idx"].astype(np.int64)


def _structure_base(n, structure_offsets):
    """int64[n]: the first atom of every atom's structure (zeros for structure_offsets None: one structure)."""
    base = np.zeros(n, np.int64)
    if structure_offsets is not None:
        so = np.asarray(structure_offsets).astype(np.int64)
        if so.ndim != 1 or so.shape[0] < 1 or so[0] != 0 or so[-1] != n or (np.diff(so) < 0).any():
            raise ValueError("structure_offsets must be non-decreasing from 0 to the number of atoms")
        base = so[np.searchsorted(so[1:], np.arange(n), side="right")] if n else base
    return base


def edge_index(offsets, entries, structure_offsets=None) -> np.ndarray:
    """The lists of atoms_within[_batch] as the edges of a graph, int64[2, E] in list order: row 0 the centre's
    batch-global atom index, row 1 the partner's (its structure's first atom plus idx).  entries["d2"] runs beside it."""
    return np.stack(_within_pairs(offsets, entries, structure_offsets))


def nearest_table(offsets, entries, k: int, structure_offsets=None):
    """The lists of nearest_atoms[_batch] as a dense table, (idx int64[N, k], d2 float32[N, k]): row i holds atom i's
    list in order, idx as batch-global atom indices (the structure's first atom plus idx), padded with -1, and d2 padded
    with +inf - the fixed fan-in form graph code wants.  A list longer than k raises."""
    centre, partner = _within_pairs(offsets, entries, structure_offsets)
    n = np.asarray(offsets).shape[0] - 1
    k = int(k)
    off = np.asarray(offsets).astype(np.int64)
    if k < 1 or (n and int(np.diff(off).max()) > k):
        raise ValueError("k must be at least 1 and no list may be longer than k")
    col = np.arange(len(centre), dtype=np.int64) - off[centre]
    idx = np.full((n, k), -1, np.int64)
    d2 = np.full((n, k), np.inf, np.float32)
    idx[centre, col] = partner
    d2[centre, col] = np.asarray(entries)["d2"]
    return idx, d2


def closest_pairs(offsets, entries, labels, structure_offsets=None):
    """(label_a int64[P], label_b int64[P], distance float32[P]): one row per ordered pair of different labels (centre's,
    partner's) that occurs in the lists of atoms_within[_batch], sorted by (label_a, label_b); distance is the float32
    square root of the smallest d2 between them.  labels holds an integer per atom of the batch - with the residue
    number per atom this is the residue contact map by closest atom.  (Labels are compared as they are: give the
    structures of a batch disjoint labels.)"""
    centre, partner = _within_pairs(offsets, entries, structure_offsets)
    lab = np.asarray(labels)
    if lab.dtype.kind not in "ui" or lab.shape != (np.asarray(offsets).shape[0] - 1,):
        raise ValueError("labels must be a 1-D array of one integer per atom")
    lab = lab.astype(np.int64)
    la, lb, d2 = lab[centre], lab[partner], np.asarray(entries)["d2"]
    keep = la != lb
    la, lb, d2 = la[keep], lb[keep], d2[keep]
    order = np.lexsort((d2, lb, la))
    la, lb, d2 = la[order], lb[order], d2[order]
    first = np.ones(la.shape[0], bool)
    first[1:] = (la[1:] != la[:-1]) | (lb[1:] != lb[:-1])
    return la[first], lb[first], np.sqrt(d2[first].astype(np.float32))


def default_link(radius, probe_radius: float = 1.4, n_points: int = 100) -> np.float32:
    """The link length surface_components uses when none is given: float32(1.5 * sqrt(4 pi / n_points) * (max_r + probe)),
    max_r the largest finite radius folded from 0, computed in float64 and rounded once.  sqrt(4 pi / n_points) * R is
    the side of the square that one dot's share of a sphere of radius R would fill; one and a half of that spans the
    largest gap between neighbouring dots of one sphere (1.42 A of 1.7441 A for ProtOr radii, probe 1.4 and 100 points)."""
    n_points = _n_points(n_points)
    r = np.asarray(radius, dtype=np.float32).astype(np.float64)
    r = r[np.isfinite(r)]
    max_r = max(0.0, float(r.max())) if r.size else 0.0
    return np.float32(1.5 * np.sqrt(4.0 * np.pi / n_points) * (max_r + float(probe_radius)))


def _dot_offsets(dot_offsets):
    off = np.ascontiguousarray(dot_offsets, dtype=np.uint64).astype(np.int64)
    if off.ndim != 1 or off.shape[0] < 1 or off[0] != 0 or (np.diff(off) < 0).any():
        raise ValueError("dot_offsets must be a 1-D array, non-decreasing from 0")
    return off


def dot_seeds(dot_offsets, atoms) -> np.ndarray:
    """uint8[D]: the seed bytes of dot_geodesics[_batch] that mark all dots of the given atoms (batch-global atom
    indices, or a boolean mask over the atoms); atom i's dots are [dot_offsets[i], dot_offsets[i + 1])."""
    off = _dot_offsets(dot_offsets)
    n = off.shape[0] - 1
    atoms = np.asarray(atoms)
    chosen = np.zeros(n, bool)
    if atoms.dtype == bool:
        if atoms.shape != (n,):
            raise ValueError(f"a mask of atoms must have {n} entries")
        chosen = atoms
    else:
        if atoms.size and (atoms.dtype.kind not in "ui" or int(atoms.min()) < 0 or int(atoms.max()) >= n):
            raise ValueError(f"atoms must be integer indices in [0, {n})")
        chosen[atoms.astype(np.int64).reshape(-1)] = True
    return np.repeat(chosen, np.diff(off)).astype(np.uint8)


def dot_structure_offsets(dot_offsets, structure_offsets=None) -> np.ndarray:
    """int64[S + 1]: where every structure's dots begin in the batch-wide dot order, dot_offsets[structure_offsets] - the
    structure_offsets to give edge_index() with the lists of dot_links[_batch].  None: one structure."""
    off = _dot_offsets(dot_offsets)
    if structure_offsets is None:
        return np.array([0, off[-1]], np.int64)
    so = _offsets("structure_offsets", structure_offsets).astype(np.int64)
    if so[0] != 0 or so[-1] != off.shape[0] - 1 or (np.diff(so) < 0).any():
        raise ValueError("structure_offsets must be non-decreasing from 0 to the number of atoms")
    return off[so]


def _dots(dot_offsets, labels, radius, probe_radius, n_points, structure_offsets):
    """The checked arguments of component_table / split_sasa: (dot offsets int64[N + 1], labels int64[D], structure
    offsets int64[S + 1], owner int64[D], dot area float64[D])."""
    n_points = _n_points(n_points)
    radius = _f32(radius)
    n = radius.shape[0]
    off = np.ascontiguousarray(dot_offsets, dtype=np.uint64).astype(np.int64)
    labels = np.ascontiguousarray(labels, dtype=np.uint32).astype(np.int64)
    if radius.ndim != 1 or off.ndim != 1 or off.shape[0] != n + 1:
        raise ValueError(f"dot_offsets must be a 1-D array of {n + 1} entries (one per atom, and the end)")
    sizes = np.diff(off)
    if off[0] != 0 or (sizes < 0).any():
        raise ValueError("dot_offsets must be non-decreasing from 0")
    if labels.ndim != 1 or labels.shape[0] != int(off[-1]):
        raise ValueError(f"labels must be a 1-D array of dot_offsets[-1] = {int(off[-1])} entries")
    so = np.array([0, n], np.int64) if structure_offsets is None else \
        _offsets("structure_offsets", structure_offsets).astype(np.int64)
    if (int(so[-1]) if so.shape[0] > 1 else 0) != n or so[0] != 0 or (np.diff(so) < 0).any():
        raise ValueError(f"structure_offsets must be non-decreasing from 0 to the {n} atoms of radius")
    owner = np.repeat(np.arange(n, dtype=np.int64), sizes)
    with np.errstate(invalid="ignore", over="ignore"):
        R = (radius + np.float32(probe_radius)).astype(np.float64)
        area = (4.0 * np.pi * (R * R) / n_points)[owner]
    return off, labels, so, owner, area


def component_table(dot_offsets, labels, radius, probe_radius: float = 1.4, n_points: int = 100, structure_offsets=None):
    """The components of surface_components[_batch] per structure, ranked: (component_offsets int64[S + 1],
    label uint32[C], dots int64[C], area float64[C], atoms int64[C]).  Structure s owns rows
    [component_offsets[s], component_offsets[s + 1]), sorted by area descending, ties to the smaller label; label is
    the component's representative dot (a dot number within the structure), dots its size, area the float64 sum of
    4 pi R^2 / n_points over its dots in dot order (R = radius + probe_radius in float32, of the dot's atom), atoms how
    many atoms own a dot of it.  structure_offsets None: one structure.  Host arithmetic (a bincount of the labels)."""
    off, labels, so, owner, area = _dots(dot_offsets, labels, radius, probe_radius, n_points, structure_offsets)
    n_struct = so.shape[0] - 1
    c_off = np.zeros(n_struct + 1, np.int64)
    cols = ([], [], [], [])
    for s in range(n_struct):
        b, e = int(off[so[s]]), int(off[so[s + 1]])
        lab = labels[b:e]
        if lab.size and int(lab.max()) >= e - b:
            raise ValueError(f"a label of structure {s} is no dot number of it")
        uniq = np.unique(lab)
        n_dots = np.bincount(lab, minlength=e - b)[uniq]
        a = np.bincount(lab, weights=area[b:e], minlength=e - b)[uniq]
        pairs = np.unique((lab << 32) | (owner[b:e] - so[s]))
        n_atoms = np.bincount(pairs >> 32, minlength=e - b)[uniq]
        order = np.lexsort((uniq, -a))
        for col, v in zip(cols, (uniq, n_dots, a, n_atoms)):
            col.append(v[order])
        c_off[s + 1] = c_off[s] + uniq.shape[0]
    cat = [np.concatenate(c) if c else np.zeros(0) for c in cols]
    return c_off, cat[0].astype(np.uint32), cat[1].astype(np.int64), cat[2].astype(np.float64), cat[3].astype(np.int64)


def split_sasa(dot_offsets, labels, radius, probe_radius: float = 1.4, n_points: int = 100, structure_offsets=None):
    """(outer float64[N], cavity float64[N]): every atom's accessible area split into the part that lies on its
    structure's first-ranked component of component_table (the largest by area) and the rest, each the float64 sum of
    4 pi R^2 / n_points over the atom's dots there.  Calling the largest component the outer surface is a convention
    for single-body structures (a protein with internal voids); a structure of several bodies has several outer
    surfaces, and its callers choose from component_table."""
    off, labels, so, owner, area = _dots(dot_offsets, labels, radius, probe_radius, n_points, structure_offsets)
    c_off, label = component_table(dot_offsets, labels, radius, probe_radius, n_points, structure_offsets)[:2]
    n = off.shape[0] - 1
    is_outer = np.zeros(labels.shape[0], bool)
    for s in range(so.shape[0] - 1):
        b, e = int(off[so[s]]), int(off[so[s + 1]])
        if e > b:
            is_outer[b:e] = labels[b:e] == int(label[c_off[s]])
    outer = np.bincount(owner[is_outer], weights=area[is_outer], minlength=n)
    cavity = np.bincount(owner[~is_outer], weights=area[~is_outer], minlength=n)
    return outer, cavity


def _patch_args(dot_offsets, centre_offsets, centres, structure_offsets):
    """The checked arguments of the patch helpers: (dot offsets int64[N + 1], first dot of every structure int64[S + 1],
    centre offsets int64[S + 1], centres int64[K])."""
    off = _dot_offsets(dot_offsets)
    s_off = dot_structure_offsets(dot_offsets, structure_offsets)
    c_off = np.ascontiguousarray(centre_offsets, dtype=np.uint64).astype(np.int64)
    centres = np.ascontiguousarray(centres, dtype=np.uint32).astype(np.int64)
    if c_off.ndim != 1 or c_off.shape != s_off.shape or c_off[0] != 0 or (np.diff(c_off) < 0).any():
        raise ValueError(f"centre_offsets must be a 1-D array of {s_off.shape[0]} entries, non-decreasing from 0")
    if centres.ndim != 1 or centres.shape[0] != int(c_off[-1]):
        raise ValueError(f"centres must be a 1-D array of centre_offsets[-1] = {int(c_off[-1])} entries")
    if (centres >= np.repeat(np.diff(s_off), np.diff(c_off))).any():
        raise ValueError("a centre is no dot number of its structure")
    return off, s_off, c_off, centres


def dot_seeds_from(centre_offsets, centres, dot_offsets, structure_offsets=None) -> np.ndarray:
    """uint8[D]: the seed bytes that mark the centres of dot_patches[_batch] - given to dot_geodesics[_batch] with no
    limit they reproduce its dist and source.  structure_offsets None: one structure."""
    off, s_off, c_off, centres = _patch_args(dot_offsets, centre_offsets, centres, structure_offsets)
    seeds = np.zeros(int(off[-1]), np.uint8)
    seeds[centres + np.repeat(s_off[:-1], np.diff(c_off))] = 1
    return seeds


def patch_index(dot_offsets, source, centre_offsets, centres, structure_offsets=None) -> np.ndarray:
    """int64[D]: for every dot the batch-global position in `centres` of its centre source[d] (dot_patches[_batch] with
    sources=True), -1 where source is 0xFFFFFFFF (a dot no centre reaches: max_centres cut the sampling short).
    np.bincount(patch_index, weights=values) sums per-dot values by patch.  structure_offsets None: one structure."""
    off, s_off, c_off, centres = _patch_args(dot_offsets, centre_offsets, centres, structure_offsets)
    source = np.ascontiguousarray(source, dtype=np.uint32).astype(np.int64)
    if source.ndim != 1 or source.shape[0] != int(off[-1]):
        raise ValueError(f"source must be a 1-D array of dot_offsets[-1] = {int(off[-1])} entries")
    base = np.repeat(s_off[:-1], np.diff(s_off))
    where = np.full(int(off[-1]) + 1, -1, np.int64)          # batch-wide dot -> position in centres; the last: no dot
    where[centres + np.repeat(s_off[:-1], np.diff(c_off))] = np.arange(centres.shape[0])
    none = source == 0xFFFFFFFF
    if (source[~none] >= (np.repeat(np.diff(s_off), np.diff(s_off)))[~none]).any():
        raise ValueError("a source is no dot number of its structure")
    out = where[np.where(none, int(off[-1]), source + base)]
    if (out[~none] < 0).any():
        raise ValueError("a source is no centre of its structure")
    return out


def patch_table(dot_offsets, source, centre_offsets, centres, radius, probe_radius: float = 1.4, n_points: int = 100,
                structure_offsets=None):
    """The patches of dot_patches[_batch], one row per centre in the order of `centres`: (structure int64[K],
    centre uint32[K], dots int64[K], atoms int64[K], area float64[K]) - the structure of the centre, its dot number,
    how many dots have it as their source, how many atoms own one of those, and the float64 sum of 4 pi R^2 / n_points
    over them in dot order (R = radius + probe_radius in float32, of the dot's atom; component_table's area).  The rows
    of a structure sum to the area of its reached dots.  structure_offsets None: one structure."""
    which = patch_index(dot_offsets, source, centre_offsets, centres, structure_offsets)
    off, _, so, owner, area = _dots(dot_offsets, np.zeros(which.shape[0], np.uint32), radius, probe_radius, n_points,
                                    structure_offsets)
    c_off = np.ascontiguousarray(centre_offsets, dtype=np.uint64).astype(np.int64)
    k = int(c_off[-1])
    hit = which >= 0
    dots = np.bincount(which[hit], minlength=k).astype(np.int64)
    a = np.bincount(which[hit], weights=area[hit], minlength=k).astype(np.float64)
    pairs = np.unique((which[hit] << 32) | owner[hit])
    atoms = np.bincount(pairs >> 32, minlength=k).astype(np.int64)
    structure = np.repeat(np.arange(so.shape[0] - 1, dtype=np.int64), np.diff(c_off))
    return structure, np.ascontiguousarray(centres, dtype=np.uint32), dots, atoms, a


def sas_volume(vectors, free, x, y, z, radius, probe_radius: float = 1.4, n_points: int = 100, structure_offsets=None,
               origins=None):
    """rsasa_sas_volume: (volume float64[S], area float64[S]) of the accessible surface of every structure from the
    vectors and counts of exposure_vectors[_batch] of these columns: V = sum (a / 3) (R k + (c - o) . E) and
    A = sum a k with a = 4 pi R^2 / n_points, R = radius + probe_radius (float32), in float64 and atom order on the host
    (no GPU).  structure_offsets None: one structure.  origins: float64[S, 3] or None for each structure's mean atom
    centre.  Atoms with a non-finite coordinate or radius are skipped."""
    n_points = _n_points(n_points)
    x, y, z, radius, _ = _columns(x, y, z, radius, None)
    n = x.shape[0]
    so = np.array([0, n], np.uint32) if structure_offsets is None else _offsets("structure_offsets", structure_offsets)
    n_struct = so.shape[0] - 1
    if (int(so[-1]) if n_struct else 0) != n:
        raise ValueError(f"the offsets cover {int(so[-1]) if n_struct else 0} atoms but the columns hold {n}")
    vectors = np.ascontiguousarray(vectors, dtype=np.float32)
    free = np.ascontiguousarray(free, dtype=np.uint32)
    if vectors.shape != (n, 3) or free.shape != (n,):
        raise ValueError(f"vectors must have shape [{n}, 3] and free [{n}]")
    if origins is not None:
        origins = np.ascontiguousarray(origins, dtype=np.float64)
        if origins.shape != (n_struct, 3):
            raise ValueError(f"origins must have shape [{n_struct}, 3]")
    volume, area = np.zeros(n_struct, np.float64), np.zeros(n_struct, np.float64)
    check(_capi.load().rsasa_sas_volume(ptr(x), ptr(y), ptr(z), ptr(radius), ptr(vectors), ptr(free), ptr(so), n_struct,
                                        probe_radius, n_points, ptr(origins), ptr(volume), ptr(area)))
    return volume, area


def contact_areas(counts, offsets, radius, probe_radius: float = 1.4, n_points: int = 100) -> np.ndarray:
    """Counts of contact_points (covered or exclusive) as areas, float32[total] in A^2: the reference's
    ((4 pi R^2) k) / n_points in float32 (src/lib.rs:220-222), k the count and R = radius + probe_radius of the atom
    whose list holds the entry (row i of `offsets`, radius[i])."""
    n_points = _n_points(n_points)
    radius = _f32(radius)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if radius.ndim != 1 or offsets.ndim != 1 or offsets.shape[0] != radius.shape[0] + 1:
        raise ValueError(f"offsets must be a 1-D array of {radius.shape[0] + 1} entries (one per atom, and the end)")
    sizes = np.diff(offsets.astype(np.int64))
    if offsets[0] != 0 or (sizes < 0).any():
        raise ValueError("offsets must be non-decreasing from 0")
    if counts.ndim != 1 or counts.shape[0] != int(offsets[-1]):
        raise ValueError(f"counts must be a 1-D array of offsets[-1] = {int(offsets[-1])} entries")
    R = radius[np.repeat(np.arange(radius.shape[0]), sizes)] + np.float32(probe_radius)
    with np.errstate(invalid="ignore"):
        return ((np.float32(4.0) * np.float32(np.pi)) * (R * R)) * counts.astype(np.float32) * \
            (np.float32(1.0) / np.float32(n_points))


def group_areas(offsets, partner_groups, counts, groups, radius, probe_radius: float = 1.4, n_points: int = 100):
    """Rows of group_contacts (buried or only) summed into a group x group table: (from_group uint32[P],
    to_group uint32[P], area float64[P]), one entry per distinct ordered pair that has a row, sorted by (from, to).
    area is the area of the atoms labelled `from` that group `to` takes: every row's area by contact_areas' float32
    expression (R of the atom that owns the row), summed in float64.  (A, B) and (B, A) are separate entries - the area
    of A buried by B and the area of B buried by A - and differ in general.  Labels are taken at face value: give a
    batch structure by structure unless its structures use different labels."""
    area = contact_areas(counts, offsets, radius, probe_radius, n_points)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    groups = _labels(groups, offsets.shape[0] - 1)
    partner = _labels(partner_groups, area.shape[0])
    owner = np.repeat(groups, np.diff(offsets.astype(np.int64)))
    key = (owner.astype(np.uint64) << np.uint64(32)) | partner.astype(np.uint64)
    pairs, inverse = np.unique(key, return_inverse=True)
    total = np.bincount(inverse.reshape(-1), weights=area.astype(np.float64), minlength=pairs.shape[0])
    return (pairs >> np.uint64(32)).astype(np.uint32), (pairs & np.uint64(0xFFFFFFFF)).astype(np.uint32), total


def owner_areas(offsets, entries, owned, labels, radius, probe_radius: float = 1.4, n_points: int = 100,
                structure_offsets=None):
    """The owned counts of contact_owners[_batch] summed into a label x label table: (from_label uint32[P],
    to_label uint32[P], area float64[P]), one entry per distinct ordered pair (label of the atom, label of the entry's
    neighbour) that has an entry, sorted by (from, to).  area is the area of the atoms labelled `from` that the atoms
    labelled `to` own: every entry's area by contact_areas' float32 expression (R of the atom whose list holds the
    entry), summed in float64.  from == to is included: the area lost inside a group.  labels: one integer label per
    atom, over the whole batch; structure_offsets (the batch form's) makes idx batch-global, None: one structure.
    The table is ADDITIVE: for every label A, the sum over B of area(A, B) plus A's SASA is the sum of 4 pi R^2 over
    A's atoms (up to the float32 rounding of each term), and in counts this holds exactly - the owned counts of
    A's atoms plus their accessible points are n_points per atom."""
    area = contact_areas(owned, offsets, radius, probe_radius, n_points)
    off = np.ascontiguousarray(offsets, dtype=np.uint64).astype(np.int64)
    n = off.shape[0] - 1
    labels = _labels(labels, n)
    ent = np.asarray(entries)
    if ent.dtype != NEIGHBOR_DTYPE or ent.ndim != 1 or ent.shape[0] != area.shape[0]:
        raise ValueError("entries must be a NEIGHBOR_DTYPE array of offsets[-1] entries")
    centre = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    partner = _structure_base(n, structure_offsets)[centre] + ent["idx"].astype(np.int64)
    if partner.size and int(partner.max()) >= n:
        raise ValueError("an entry's idx lies outside its structure: are the structure_offsets those of the call?")
    key = (labels[centre].astype(np.uint64) << np.uint64(32)) | labels[partner].astype(np.uint64)
    pairs, inverse = np.unique(key, return_inverse=True)
    total = np.bincount(inverse.reshape(-1), weights=area.astype(np.float64), minlength=pairs.shape[0])
    return (pairs >> np.uint64(32)).astype(np.uint32), (pairs & np.uint64(0xFFFFFFFF)).astype(np.uint32), total


def make_atoms(x, y, z, radius, ids) -> np.ndarray:
    """Packs SoA columns into rsasa_atom_t records."""
    a = np.zeros(len(x), ATOM_DTYPE)
    a["position"][:, 0] = x
    a["position"][:, 1] = y
    a["position"][:, 2] = z
    a["radius"] = radius
    a["id"] = ids
    return a


__all__ = ["Context", "RsasaError", "device_count", "sphere_points", "make_atoms", "unpack_points", "surface_points",
           "ENCLOSE_MAX_DIRS", "ENCLOSE_PARTNER", "enclosure_fraction", "escape_vectors",
           "contact_areas", "group_areas", "owner_areas", "sas_volume", "residue_depth", "default_link", "component_table", "split_sasa",
           "dot_seeds", "dot_structure_offsets",
           "ATOM_DTYPE", "NEIGHBOR_DTYPE"]
