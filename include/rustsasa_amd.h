/*
 * rustsasa_amd.h -- C ABI of the MI355X-native Shrake-Rupley SASA engine.
 *
 * This is the drop-in boundary for RustSASA's hot path.  The reference has no
 * FFI layer of its own; its seam is the free function
 *
 *     pub fn calculate_sasa_internal(atoms: &[Atom], probe_radius: f32,
 *                                    n_points: usize, threads: isize) -> Vec<f32>
 *                                                     (reference src/lib.rs:249-254)
 *
 * called from SASAOptions::<T>::process (reference src/options.rs:615-616).
 * Every entry point below cites the reference interface it replaces.  The
 * Rust-side binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every function
 * returns RSASA_OK (0) or a negative rsasa_status; nothing throws across the
 * boundary; all `out_*` buffers are caller-owned.  The library is built for
 * gfx950 only and has NO CPU fallback: without a usable HIP device every
 * compute entry point fails with RSASA_ERR_NO_DEVICE.
 */
#ifndef RUSTSASA_AMD_H
#define RUSTSASA_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: rsasa_batch_wait returns the OLDEST of up to two batches in flight (version 1 had one batch in flight, so
 * "the" batch); rsasa_batch_wait_all, rsasa_context_get_simd_width, rsasa_context_bind_thread added.
 * 3: rsasa_host_batch_enqueue / _wait / _wait_all (a stream of host batches), rsasa_context_clone_settings,
 *    rsasa_context_ids_dropped added;
 * 4: rsasa_context_set_call_combining, rsasa_call_combining_stats, rsasa_context_ids_kept added; rsasa_host_batch_enqueue with eight batches
 *    queued returns RSASA_ERR_QUEUE_FULL at once (it used to wait for the oldest batch and then fail);
 * nothing else changed, nothing removed.
 * Additive under 4 (callers detect them by symbol): rsasa_neighbor_t, rsasa_precompute_neighbors,
 * rsasa_precompute_neighbors_batch, RSASA_ERR_BUFFER_TOO_SMALL; rsasa_accessible_points,
 * rsasa_accessible_points_batch; rsasa_contact_points, rsasa_contact_points_batch; rsasa_group_contacts,
 * rsasa_group_contacts_batch; rsasa_exposure_vectors, rsasa_exposure_vectors_batch, rsasa_sas_volume;
 * rsasa_atom_depth, rsasa_atom_depth_batch; rsasa_surface_components, rsasa_surface_components_batch;
 * rsasa_half_sphere_exposure, rsasa_half_sphere_exposure_batch; rsasa_within_t, rsasa_atoms_within,
 * rsasa_atoms_within_batch; RSASA_NEAREST_MAX_K, rsasa_nearest_atoms, rsasa_nearest_atoms_batch;
 * RSASA_RADIAL_MAX_CLASSES, RSASA_RADIAL_MAX_BINS, rsasa_radial_counts, rsasa_radial_counts_batch;
 * rsasa_contact_owners, rsasa_contact_owners_batch; RSASA_CROWD_MAX_BINS, rsasa_dot_crowding,
 * rsasa_dot_crowding_batch; RSASA_ENCLOSE_MAX_DIRS, rsasa_dot_enclosure, rsasa_dot_enclosure_batch. */
/* Additive under 4 as well: rsasa_dot_links, rsasa_dot_links_batch; rsasa_dot_geodesics, rsasa_dot_geodesics_batch;
 * rsasa_context_geodesic_rounds. */
/* And: rsasa_dot_patches, rsasa_dot_patches_batch; rsasa_context_patch_stats. */
/* And: RSASA_FIELD_PARTNER, RSASA_FIELD_MAX_CHANNELS, RSASA_FIELD_STEP, RSASA_FIELD_INV_D, RSASA_FIELD_INV_D2,
 * RSASA_FIELD_INV_1PD, rsasa_dot_fields, rsasa_dot_fields_batch. */
/* And: RSASA_CURV_COLUMNS, RSASA_CURV_D2, RSASA_CURV_H, RSASA_CURV_XX, RSASA_CURV_YY, RSASA_CURV_ZZ, RSASA_CURV_XY,
 * RSASA_CURV_XZ, RSASA_CURV_YZ, rsasa_dot_curvature, rsasa_dot_curvature_batch. */
#define RSASA_ABI_VERSION 4

typedef enum rsasa_status {
    RSASA_OK = 0,
    RSASA_ERR_INVALID_ARGUMENT = -1, /* NULL where data is required, probe+max_radius <= 0, n_points == 0, ... */
    RSASA_ERR_NO_DEVICE = -2,        /* no HIP device / device index out of range */
    RSASA_ERR_HIP = -3,              /* a HIP runtime call failed; see rsasa_context_last_error */
    RSASA_ERR_OUT_OF_MEMORY = -4,
    RSASA_ERR_GRID_TOO_LARGE = -5,   /* a structure's cell grid exceeds 2^31 cells (coordinates too sparse) */
    RSASA_ERR_INTERNAL = -6,
    RSASA_ERR_QUEUE_FULL = -7,       /* rsasa_host_batch_enqueue: eight batches are queued and not yet waited for */
    RSASA_ERR_BUFFER_TOO_SMALL = -8  /* rsasa_precompute_neighbors*, rsasa_contact_points*, rsasa_contact_owners*: out_entries is NULL or holds
                                        fewer entries than out_offsets[n] (which has been written); rsasa_group_contacts*:
                                        the same for its row buffers; rsasa_surface_components*: for out_labels;
                                        rsasa_dot_crowding*: for out_counts; rsasa_dot_enclosure*: for out_blocked;
                                        rsasa_dot_fields*: for out_sums;
                                        rsasa_atoms_within*, rsasa_nearest_atoms*: for their out_entries;
                                        rsasa_dot_links*: for out_link_offsets and out_entries */
                                     /* rsasa_dot_patches*: for its centre and dot buffers (see there) */
} rsasa_status;

/* Mirrors `Atom` (reference src/structures/atomic.rs:13-24) without the
 * parent_id field, which the hot path never reads.  24 bytes, C layout. */
typedef struct rsasa_atom {
    float position[3];
    float radius;
    uint64_t id; /* atoms with equal id never occlude each other (src/lib.rs:124) */
} rsasa_atom_t;

typedef struct rsasa_context rsasa_context_t;

/* ---- library / device ------------------------------------------------- */
int rsasa_abi_version(void);
const char *rsasa_status_string(int status);
/* Number of HIP devices visible to this process (0 is a valid answer). */
int rsasa_device_count(int *out_count);

/* One context = one GPU + two launch streams with a growable HBM workspace
 * each (two batches in flight, see rsasa_batch_enqueue), copy streams of the
 * host-pointer entry points, and the cached sphere lattices.  Calls on one context are serialised by an internal
 * mutex; use one context per host thread (or per rayon worker) for
 * concurrency.  Replaces the reference's global rayon pool
 * (src/utils.rs:63-81) as the unit of parallel resources. */
int rsasa_context_create(int device, rsasa_context_t **out_ctx);
int rsasa_context_destroy(rsasa_context_t *ctx);
const char *rsasa_context_last_error(const rsasa_context_t *ctx);
/* The GPU index the context was created on (directory mode opens its second worker context there). */
int rsasa_context_get_device(const rsasa_context_t *ctx, int *out_device);

/* pulp lane count W the reference host would dispatch to (8 = AVX2+FMA
 * [default], 16 = AVX-512, 4 = NEON, 1 = scalar).  It only selects which of
 * the last (n_points mod W) sphere points use the reference's scalar
 * remainder rule -- unfused dot product and `<=` (src/lib.rs:163-218). */
int rsasa_context_set_simd_width(rsasa_context_t *ctx, int simd_width);
int rsasa_context_get_simd_width(rsasa_context_t *ctx, int *out_simd_width);

/* CALL COMBINING (ABI 4), for the reference's own call pattern left unchanged:
 * one rsasa_calculate_sasa_internal / rsasa_calculate_sasa_soa call per
 * structure from every worker thread (reference src/main.rs:375,439,
 * src/lib.rs:249-254).  With max_wait_us >= 0 the per-structure calls made
 * through this context - from any number of host threads, and together with
 * those of every other context of the same GPU that has it on - are merged into
 * batch launches: a caller that finds one of the GPU's two combining lanes free
 * leads a batch of every call queued at that moment with the same settings
 * (probe radius, point count, lane count W, ids passed or not; calls that
 * differ are never merged), every member copies its own atoms in and its own
 * values out.  While both lanes are busy the arriving calls queue up, so the
 * batches grow with the load and no timer is needed: max_wait_us = 0 is the
 * recommended setting; a positive value lets a leader hold its batch back up
 * to that long for as many calls as the previous batch had.  The values are
 * those of the call made alone, bit for bit (a batch is independent
 * structures).  A call the combiner does not take - more than 32 768 atoms,
 * non-finite input, anything the call alone would report as an error - runs
 * by itself and cannot fail its batch-mates; a device error fails every call
 * of the batch it hit with that status.  A context may be shared by all
 * threads or there may be one per thread.  max_wait_us < 0 switches it off
 * (the default). */
int rsasa_context_set_call_combining(rsasa_context_t *ctx, int max_wait_us);
/* Batches launched and calls merged into them on `device` since the process
 * started (either pointer may be NULL). */
int rsasa_call_combining_stats(int device, uint64_t *out_batches, uint64_t *out_calls);

/* Multi-socket hosts: binds the CALLING thread to the CPUs of the NUMA node the
 * context's GPU hangs off (sysfs numa_node / local_cpulist of its PCI address;
 * the context's own worker threads are bound the same way when they start).
 * A host program with one worker thread per GPU - the reference runs one rayon
 * worker per structure, src/main.rs:375 - calls this once at the top of each
 * worker, before it allocates the buffers it hands to the context.
 * *out_numa_node (nullable) receives the node, or -1 when the machine has one
 * node, hides its topology, or RSASA_NUMA=0 is set; then nothing is bound. */
int rsasa_context_bind_thread(rsasa_context_t *ctx, int *out_numa_node);

/* Copies every setting that changes how `src` computes - the pulp lane count
 * and the kernel tuning a process may have set - to `dst`: for programs that
 * run several contexts side by side (a second context on the same GPU, one
 * context per GPU) and want them to give the same values. */
int rsasa_context_clone_settings(rsasa_context_t *dst, rsasa_context_t *src);

/* Argument rules (every entry point of the hot path, rsasa_batch_enqueue and
 * rsasa_segment_sums).  A call is answered by the FIRST rule it breaks, in the
 * order listed for its entry point, with RSASA_ERR_INVALID_ARGUMENT and the
 * rule's message as the context's last error - before the context is locked,
 * a buffer reserved, a byte uploaded, an output written, or a column or
 * offset read for anything but a rule.  The rules:
 *   - n_points in [1, 2^24]; probe_radius finite and >= 0 (-0.0 is 0);
 *     n_points comes before probe_radius;
 *   - sizes (atoms, structures, residues, frames, values, segments) below
 *     0xFFFFFFF0;
 *   - structure offsets: not NULL, spanning [0, n_atoms] - the first entry is
 *     0 on EVERY path, and for a device batch the last is n_atoms -, then
 *     non-decreasing: the span comes before the order;
 *   - residue offsets: the last not past the atoms, then non-decreasing.
 * Order of the verdicts:
 *   rsasa_calculate_sasa_internal, _soa: n_atoms >= 0xFFFFFFF0 and a missing
 *     out_sasa (for _internal: or atoms) are refused without a message; columns
 *     NULL; n_atoms == 0 is RSASA_OK (whatever n_points is); n_points; probe.
 *   rsasa_calculate_sasa_batch (and, from rsasa_host_batch_wait, a batch of
 *     rsasa_host_batch_enqueue, which itself checks nothing): structure_offsets
 *     NULL; columns NULL; out_residue_sasa NULL; no output requested; no atoms
 *     and no residues is RSASA_OK; residue offsets; n_points; probe; sizes; the
 *     structure offsets' span; their order.
 *   rsasa_calculate_sasa_trajectory: no frames or no atoms is RSASA_OK; xyz /
 *     radius NULL; out_residue_sasa NULL; no output requested; sizes; residue
 *     offsets; n_points; probe.
 *   rsasa_batch_enqueue: batch NULL; n_points; probe; sizes; columns NULL;
 *     structure_offsets_host NULL; span; order; atoms without structures;
 *     out_residue_sasa NULL.
 *   rsasa_segment_sums: no segments is RSASA_OK; NULL argument; sizes and the
 *     last offset; the offsets' order.
 * The rules answer before device batches in flight on the context are waited
 * for: an invalid call does not report an earlier batch's deferred error - that
 * error stays with its batch for the next rsasa_batch_wait. */

/* ---- the hot path, one structure per call ------------------------------ */

/* Non-finite input (every entry point of the hot path, every kernel).
 * The reference checks nothing; what its arithmetic does with a NaN is
 * reproduced bit for bit: a NaN coordinate is skipped by the bounding box
 * (f32::min / max, spatial_grid.rs:113-121), lands in cell 0 (`as u32`,
 * :139-141) and fails every distance test (:321-335), so the atom is nobody's
 * neighbour, has no neighbours and keeps its whole sphere; a NaN radius makes
 * that atom's own value NaN (src/lib.rs:101-102,220-222) and is skipped by the
 * maximum radius (lib.rs:262).  Other atoms and the other structures of a
 * batch are not affected.  An INFINITE coordinate overflows the reference's
 * grid arithmetic (it panics): here the call - for a batch: the whole batch,
 * whose grids are placed by one scan - returns RSASA_ERR_GRID_TOO_LARGE and
 * the context stays usable.  probe_radius + largest radius not a positive
 * finite number - an infinite radius among them: an infinite cell size,
 * lib.rs:76 - returns RSASA_ERR_INVALID_ARGUMENT. */

/* Drop-in for calculate_sasa_internal (reference src/lib.rs:249-254).
 * `threads` is accepted for signature compatibility and ignored (the
 * reference uses it only to choose sequential vs rayon, src/lib.rs:278).
 * out_sasa[i] is the SASA of atoms[i] in A^2; n_atoms == 0 is valid. */
int rsasa_calculate_sasa_internal(rsasa_context_t *ctx, const rsasa_atom_t *atoms,
                                  size_t n_atoms, float probe_radius, size_t n_points,
                                  ptrdiff_t threads, float *out_sasa);

/* Same computation on struct-of-arrays input.  `id` may be NULL (all atoms
 * distinct). */
int rsasa_calculate_sasa_soa(rsasa_context_t *ctx, const float *x, const float *y,
                             const float *z, const float *radius, const uint64_t *id,
                             size_t n_atoms, float probe_radius, size_t n_points,
                             float *out_sasa);

/* ---- the hot path, many structures per call ---------------------------- */

/* Directory mode (reference src/main.rs:375,439): n_structures independent
 * structures concatenated into one SoA; structure s owns atoms
 * [structure_offsets[s], structure_offsets[s+1]).  Each structure gets its
 * own bounding box, cell grid and max radius exactly as a separate
 * calculate_sasa_internal call would.
 *
 * Optional ResidueLevel aggregation (reference src/options.rs:202-216,
 * src/utils.rs:14-22): residue k owns atoms
 * [residue_offsets[k], residue_offsets[k+1]) of the concatenated arrays and
 * out_residue_sasa[k] is their strictly sequential f32 sum.  Pass
 * residue_offsets = NULL / n_residues = 0 to skip.  out_atom_sasa may be NULL
 * when only residue values are wanted.  All pointers are HOST pointers. */
int rsasa_calculate_sasa_batch(rsasa_context_t *ctx, const float *x, const float *y,
                               const float *z, const float *radius, const uint64_t *id,
                               const uint32_t *structure_offsets, size_t n_structures,
                               float probe_radius, size_t n_points, float *out_atom_sasa,
                               const uint32_t *residue_offsets, size_t n_residues,
                               float *out_residue_sasa);

/* A STREAM of host batches (ABI 3): the same arguments and the same results as
 * rsasa_calculate_sasa_batch, but the call returns once the batch is queued.  A
 * rank that works through its share of a directory (reference
 * src/main.rs:375: files dealt to workers) enqueues batch k + 1 before it
 * waits for batch k: batch k + 1's first atoms cross the link while batch k's
 * last sub-batches compute and download, which one synchronous call after the
 * other cannot do (its first upload hides behind nothing, and nothing hides
 * its last kernels).  Two batches compute at a time - on two private contexts
 * on the caller's GPU, created by the first call (their workspaces and pinned
 * staging are sized like the caller's own would be, and live until
 * rsasa_context_destroy) - with the caller's settings at the time of the
 * enqueue; up to eight may be queued and not yet waited for: a ninth enqueue
 * does not block and does not take the batch - it returns RSASA_ERR_QUEUE_FULL
 * at once (nothing of the call's buffers is touched; call rsasa_host_batch_wait
 * and enqueue again).
 * rsasa_host_batch_wait() returns the OLDEST enqueued batch: it blocks until
 * that batch is complete and returns its status (the message is then the
 * context's last error); with nothing enqueued it returns RSASA_OK at once.
 * Several threads may enqueue and wait on one context at once: a waiting
 * thread takes the oldest batch no other thread is waiting for already.
 * Every buffer of a batch - inputs and outputs - belongs to the library from
 * the enqueue until the wait that returns the batch.  Pinned (page-locked)
 * host memory makes all copies asynchronous, as for the synchronous call.
 * The two worker contexts create their streams on hardware queues of their
 * own (the runtime otherwise multiplexes a process's streams onto four
 * queues, and two streams that share one run in order: nothing overlaps). */
int rsasa_host_batch_enqueue(rsasa_context_t *ctx, const float *x, const float *y,
                             const float *z, const float *radius, const uint64_t *id,
                             const uint32_t *structure_offsets, size_t n_structures,
                             float probe_radius, size_t n_points, float *out_atom_sasa,
                             const uint32_t *residue_offsets, size_t n_residues,
                             float *out_residue_sasa);
int rsasa_host_batch_wait(rsasa_context_t *ctx);
/* Waits for every enqueued host batch, oldest first; returns the first error. */
int rsasa_host_batch_wait_all(rsasa_context_t *ctx);

/* Device-resident form of the batch call: every pointer in the descriptor is
 * a DEVICE pointer on the context's GPU except structure_offsets_host, which
 * stays on the host (the launch geometry is derived from it).  The call only
 * enqueues work on `hip_stream` (a hipStream_t; NULL = one of the context's
 * own two streams) and returns.  Up to TWO batches may be in flight per
 * context, each in its own workspace (a third rsasa_batch_enqueue first
 * waits for the oldest): enqueueing batch k + 1 before waiting for batch k
 * keeps the GPU busy across the batch boundary - what a rank of a sharded
 * run does with its stream of batches (reference src/main.rs:375).
 * rsasa_batch_wait() waits for the OLDEST batch in flight, reports its
 * deferred errors and transparently re-runs it if the cell workspace had to
 * grow; with no batch in flight it returns RSASA_OK at once.  A batch's
 * buffers must stay valid until the rsasa_batch_wait that returns it. */
typedef struct rsasa_device_batch {
    const float *x, *y, *z, *radius;       /* [n_atoms] device */
    const uint64_t *id;                    /* [n_atoms] device, or NULL */
    const uint32_t *structure_offsets_host;/* [n_structures + 1] HOST */
    size_t n_structures;
    size_t n_atoms;
    const uint32_t *residue_offsets;       /* [n_residues + 1] device, or NULL */
    size_t n_residues;
    float *out_atom_sasa;                  /* [n_atoms] device, or NULL */
    float *out_residue_sasa;               /* [n_residues] device, or NULL */
    uint32_t *out_neighbor_counts;         /* [n_atoms] device, or NULL: per-atom
                                              candidate count K (the length of the
                                              reference's neighbour list,
                                              spatial_grid.rs:335-341) */
} rsasa_device_batch_t;

int rsasa_batch_enqueue(rsasa_context_t *ctx, const rsasa_device_batch_t *batch,
                        float probe_radius, size_t n_points, void *hip_stream);
int rsasa_batch_wait(rsasa_context_t *ctx);
/* Waits for EVERY batch in flight (oldest first) and returns the first error. */
int rsasa_batch_wait_all(rsasa_context_t *ctx);

/* MD-trajectory mode (the reference ecosystem's second workload: per-frame SASA of one
 * topology, README.md:98-149 / paper.md:45): n_frames frames of the same n_atoms atoms.
 * `xyz` is frame-major [n_frames][n_atoms][3] (HOST); radius / id / residue_offsets
 * ([n_residues + 1], offsets within one frame) are given once.  Every frame is an
 * independent structure (own bounding box, grid, max radius), exactly as n_frames separate
 * calculate_sasa_internal calls (src/lib.rs:249-254).  out_atom_sasa is [n_frames][n_atoms],
 * out_residue_sasa [n_frames][n_residues]; either may be NULL.  Only 12 bytes per atom and
 * frame cross PCIe. */
int rsasa_calculate_sasa_trajectory(rsasa_context_t *ctx, const float *xyz, size_t n_frames,
                                    size_t n_atoms, const float *radius, const uint64_t *id,
                                    float probe_radius, size_t n_points, float *out_atom_sasa,
                                    const uint32_t *residue_offsets, size_t n_residues,
                                    float *out_residue_sasa);

/* Strictly sequential f32 sums of contiguous segments of a host array, computed
 * on the GPU: out[k] = ((values[o[k]] + values[o[k]+1]) + ...) over
 * [offsets[k], offsets[k+1]).  This is the reference's simd_sum
 * (src/utils.rs:14-22) as used by the level aggregations
 * (src/options.rs:216,308,392,404). */
int rsasa_segment_sums(rsasa_context_t *ctx, const float *values, size_t n_values,
                       const uint32_t *offsets, size_t n_segments, float *out);

/* ---- neighbour lists ---------------------------------------------------- */

/* The reference's neighbour search as a product of its own:
 *
 *     pub fn precompute_neighbors(atoms: &[Atom], active_indices: &[usize],
 *                                 probe_radius: f32, max_radii: f32) -> Vec<Vec<NeighborData>>
 *                                                     (reference src/lib.rs:69-84)
 *
 * built by SpatialGrid::new / build_all_neighbor_lists and sorted by
 * sort_neighbors_by_distance (src/structures/spatial_grid.rs:28-50,195-465).
 * The lists are returned in CSR form: the list of active atom a is
 * out_entries[out_offsets[a] .. out_offsets[a + 1]).  Atom j is in atom i's
 * list exactly when j is active, j != i, id_j != id_i, d^2 <= (2 max_r + 2p)^2
 * and d^2 <= (r_i + max_r + 2p)^2, d^2 = dx*dx + dy*dy + dz*dz (not fused)
 * (spatial_grid.rs:300-341).  Entries hold the neighbour's ORIGINAL index and
 * threshold_squared = (r_j + p) * (r_j + p).
 *
 * Order: each list is sorted ascending by (d^2, idx), d^2 the centre-relative
 * key the reference sorts on (spatial_grid.rs:452-462) - one of the orders its
 * sort_unstable_by may give, and a deterministic one.
 *
 * max_radius is taken as given, as by the reference (grid cell size
 * probe + max_radius, both distance tests); NaN means fold(0, max) of the
 * active atoms' radii (lib.rs:259-262).  The "Non-finite input" paragraph
 * above holds: a NaN coordinate is nobody's neighbour and has an empty list; a
 * NaN radius gives that atom an empty list and a NaN threshold in the lists of
 * others; an infinite coordinate returns RSASA_ERR_GRID_TOO_LARGE.
 *
 * Sizing: out_offsets is always written (on success and on
 * RSASA_ERR_BUFFER_TOO_SMALL).  If out_entries is NULL or entries_capacity <
 * out_offsets[n], nothing else is written and RSASA_ERR_BUFFER_TOO_SMALL is
 * returned: call once to size, allocate, call again.
 *
 * Both calls are synchronous and run on the GPU in a workspace of their own
 * on the context's first stream: device batches in flight on the context
 * (rsasa_batch_enqueue) are neither waited for nor disturbed - they keep
 * their results and errors for rsasa_batch_wait - and streams of host
 * batches run on contexts of their own. */

/* NeighborData (reference src/structures/atomic.rs:5-10), repr(C), 8 bytes. */
typedef struct rsasa_neighbor {
    float threshold_squared;
    uint32_t idx;
} rsasa_neighbor_t;

/* precompute_neighbors (reference src/lib.rs:69-84) for one structure.
 * id: nullable (all atoms distinct).  active_indices: nullable (every atom,
 * in order); else n_active distinct indices below n_atoms (otherwise
 * RSASA_ERR_INVALID_ARGUMENT).  Only active atoms are binned and bounded
 * (spatial_grid.rs:52-90); lists are indexed by active position, idx is the
 * original index.  out_offsets: [n_active + 1]. */
int rsasa_precompute_neighbors(rsasa_context_t *ctx,
                               const float *x, const float *y, const float *z, const float *radius,
                               const uint64_t *id, size_t n_atoms,
                               const uint32_t *active_indices, size_t n_active,
                               float probe_radius, float max_radius,
                               uint64_t *out_offsets, rsasa_neighbor_t *out_entries,
                               size_t entries_capacity);

/* Directory-mode form: n_structures independent structures, one grid each
 * (as that many rsasa_precompute_neighbors calls without active_indices).
 * idx is the index WITHIN the structure; out_offsets is batch-global
 * [structure_offsets[n_structures] + 1].  A NaN max_radius is each
 * structure's own maximum. */
int rsasa_precompute_neighbors_batch(rsasa_context_t *ctx,
                                     const float *x, const float *y, const float *z, const float *radius,
                                     const uint64_t *id,
                                     const uint32_t *structure_offsets, size_t n_structures,
                                     float probe_radius, float max_radius,
                                     uint64_t *out_offsets, rsasa_neighbor_t *out_entries,
                                     size_t entries_capacity);

/* ---- accessible points -------------------------------------------------- */

/* WHICH sphere points of each atom are accessible: the decisions the SASA
 * value of an atom counts (AtomSasaKernel, reference src/lib.rs:96-223), one
 * bit per point - SAS dot surfaces, surface point clouds, directional
 * exposure, point-by-point checks of a value.
 *
 * Layout: words = (n_points + 31) / 32; atom i owns
 * out_masks[i * words .. (i + 1) * words).  Bit (p & 31) of word (p >> 5) is 1
 * exactly when lattice point p - in the order of rsasa_sphere_points
 * (lib.rs:43-66) - is accessible; the bits past n_points in the last word
 * are 0.
 *
 * Bit p is the reference's own decision for that point.  The candidates are
 * those of calculate_sasa_internal: the lists of rsasa_precompute_neighbors
 * with max_radius = fold(0, max) of the structure's radii (NaN radii skipped,
 * lib.rs:259-262), ids as there.  With v = centre - neighbour,
 * d^2 = vx*vx + vy*vy + vz*vz, R = radius + probe and
 * limit = (threshold_squared - d^2 - R*R) / (2 R) (the IEEE quotient,
 * lib.rs:129-136), a point p < n_points - n_points % W is occluded when some
 * entry gives fmaf(sx, vx, fmaf(sy, vy, sz*vz)) < limit (lib.rs:143-146), any
 * later point when some entry gives (sx*vx + sy*vy) + sz*vz <= limit
 * (lib.rs:185-186,206-207); W is the context's lane count
 * (rsasa_context_set_simd_width).  Both rules are ORs over the list, so the
 * list's order does not matter.  popcount of an atom's words is therefore the
 * reference's accessible-point count k, and out_sasa[i] (nullable) is
 * ((12.566371f * R*R) * (float)k) * (1.0f / (float)n_points) (lib.rs:220-222):
 * bit for bit the value of rsasa_calculate_sasa_batch on the same input.
 *
 * The "Non-finite input" paragraph above holds: an atom with a NaN coordinate
 * or a NaN radius has a mask of all ones (its out_sasa is NaN for a NaN
 * radius); an infinite coordinate returns RSASA_ERR_GRID_TOO_LARGE and the
 * context stays usable.  n_points == 0, probe_radius + largest radius not a
 * positive finite number, or structure_offsets that are not non-decreasing
 * from 0 return RSASA_ERR_INVALID_ARGUMENT.
 *
 * Like the neighbour calls, both are synchronous and run on the GPU in the
 * neighbour calls' workspace on the context's first stream: device batches in
 * flight (rsasa_batch_enqueue) are neither waited for nor disturbed.  Only the
 * masks (n_points / 8 bytes per atom, rounded up to whole words) and the
 * values cross the link; the lists stay on the device. */

/* One structure: n_atoms atoms, id nullable (all atoms distinct).
 * out_masks: [n_atoms * words]; out_sasa: [n_atoms] or NULL. */
int rsasa_accessible_points(rsasa_context_t *ctx,
                            const float *x, const float *y, const float *z, const float *radius,
                            const uint64_t *id, size_t n_atoms,
                            float probe_radius, size_t n_points,
                            uint32_t *out_masks, float *out_sasa);

/* Directory-mode form: n_structures independent structures concatenated as in
 * rsasa_calculate_sasa_batch (one grid and one max radius each).
 * out_masks: [structure_offsets[n_structures] * words]; out_atom_sasa:
 * [structure_offsets[n_structures]] or NULL. */
int rsasa_accessible_points_batch(rsasa_context_t *ctx,
                                  const float *x, const float *y, const float *z, const float *radius,
                                  const uint64_t *id,
                                  const uint32_t *structure_offsets, size_t n_structures,
                                  float probe_radius, size_t n_points,
                                  uint32_t *out_masks, float *out_atom_sasa);

/* ---- exposure vectors --------------------------------------------------- */

/* IN WHICH DIRECTION an atom is exposed, and the volume the accessible
 * surface encloses: per atom the vector sum of its exposed lattice points
 *
 *     E_i = sum over the exposed points p of s_p,
 *
 * s_p the unit lattice points of rsasa_sphere_points, exposed as
 * rsasa_accessible_points decides it (the same lists, the same two rules, W
 * the context's lane count).  E_i / k_i is the atom's mean outward direction
 * (summed over a residue: the side it is exposed on, as half-sphere-exposure
 * style descriptors need it); with the counts k_i the sums give the volume
 * inside the dot surface (rsasa_sas_volume below).
 *
 *   out_vectors[3 i + {0, 1, 2}] = E_i (x, y, z), float32;
 *   out_free[i]                  = k_i, the exposed count: the popcount of
 *                                  rsasa_accessible_points;
 *   out_sasa[i]                  (nullable) bit for bit
 *                                  rsasa_calculate_sasa_batch.
 *
 * The float32 summation order is part of the interface, so results can be
 * checked bit for bit.  The lattice is taken in chunks of 64 points (zero
 * padded); the term of a point is t = occluded ? +0.0f : s for each of the
 * three components, and the lanes past n_points are occluded.
 *   1. Within a chunk, with lanes l = 0..63: for h = 32, 16, 8, 4, 2, 1, set
 *      t[l] = t[l] + t[l + h] for l < h.  The chunk's sum is t[0].
 *   2. Across chunks, ascending c: E = chunk_0, then E = E + chunk_c.
 *   3. Only plain adds (no fused multiply-add, no reassociation).
 * An atom with no exposed point has E = (+0.0f, +0.0f, +0.0f).
 *
 * Non-finite input as rsasa_accessible_points: an atom with a NaN coordinate
 * or a NaN radius gets the full lattice sum (every point a term) and
 * out_free = n_points (its out_sasa is NaN for a NaN radius); an infinite
 * coordinate returns RSASA_ERR_GRID_TOO_LARGE and the context stays usable.
 * The argument errors are those of rsasa_accessible_points (n_points == 0,
 * probe_radius + largest radius not a positive finite number,
 * structure_offsets that are not non-decreasing from 0, NULL columns); in
 * addition out_vectors or out_free NULL where there are atoms returns
 * RSASA_ERR_INVALID_ARGUMENT.
 *
 * Synchronous, in the neighbour calls' workspace on the context's first
 * stream: device batches in flight (rsasa_batch_enqueue) are neither waited
 * for nor disturbed.  No masks are written or read anywhere: 16 bytes per atom
 * cross the link (and 4 for out_sasa); the lists stay on the device. */

/* One structure: n_atoms atoms, id nullable (all atoms distinct).
 * out_vectors: [n_atoms * 3]; out_free: [n_atoms]; out_sasa: [n_atoms] or
 * NULL. */
int rsasa_exposure_vectors(rsasa_context_t *ctx,
                           const float *x, const float *y, const float *z, const float *radius,
                           const uint64_t *id, size_t n_atoms,
                           float probe_radius, size_t n_points,
                           float *out_vectors, uint32_t *out_free, float *out_sasa);

/* Directory-mode form: n_structures independent structures concatenated as in
 * rsasa_calculate_sasa_batch (one grid and one max radius each).
 * out_vectors: [structure_offsets[n_structures] * 3]; out_free and
 * out_atom_sasa (nullable): [structure_offsets[n_structures]]. */
int rsasa_exposure_vectors_batch(rsasa_context_t *ctx,
                                 const float *x, const float *y, const float *z, const float *radius,
                                 const uint64_t *id,
                                 const uint32_t *structure_offsets, size_t n_structures,
                                 float probe_radius, size_t n_points,
                                 float *out_vectors, uint32_t *out_free, float *out_atom_sasa);

/* The volume the dot surface encloses, per structure, from the vectors and
 * counts above - the divergence theorem on the dots, the volume a
 * double-cubic-lattice SASA tool reports beside its area:
 *
 *     V = sum_i (a_i / 3) (R_i k_i + (c_i - o) . E_i),   A = sum_i a_i k_i,
 *
 * a_i = 4 pi R_i^2 / n_points, R_i = (double)(radius_i + probe_radius) with the
 * sum taken in float32 (the engine's R), k_i = free[i], c_i the centre, o the
 * structure's origin: origins[3 s ..] or, origins NULL, the mean centre of
 * the structure's counted atoms (accumulated in double in atom order).  V does
 * not depend on o for a closed surface; on the dots the choice changes it
 * within their discretisation error, and an origin inside the structure keeps
 * that small.  A host utility: no context, no GPU; computed in double, in atom
 * order.  Atoms with a non-finite coordinate or radius are skipped (no term,
 * not counted in the mean centre), so the results stay finite.  An empty
 * structure has volume 0 and area 0.
 * x, y, z, radius, free: [structure_offsets[n_structures]]; vectors: three per
 * atom; out_volume: [n_structures]; out_area: [n_structures] or NULL.
 * structure_offsets NULL or not non-decreasing from 0, n_points == 0, or a
 * NULL array where there are atoms (out_volume where there are structures)
 * return RSASA_ERR_INVALID_ARGUMENT. */
int rsasa_sas_volume(const float *x, const float *y, const float *z, const float *radius,
                     const float *vectors, const uint32_t *free,
                     const uint32_t *structure_offsets, size_t n_structures,
                     float probe_radius, size_t n_points,
                     const double *origins, double *out_volume, double *out_area);

/* ---- atom depth --------------------------------------------------------- */

/* HOW FAR UNDER THE SURFACE an atom lies: per atom the distance from its
 * centre to the nearest accessible dot of its own structure (atom depth,
 * Chakravarty & Varadarajan; averaged over a residue: residue depth).  The
 * other point calls are silent about the atoms with no accessible point; this
 * one tells them apart.
 *
 * Definition.  For a structure with atoms j at centre c_j and radius r_j, probe
 * p and lattice s = rsasa_sphere_points(n_points), let A_j be the accessible
 * points of j: exactly the mask of rsasa_accessible_points under the context's
 * current lane count W.  All arithmetic is float32, unfused, left to right:
 *
 *     R_j   = r_j + p
 *     q     = (c_j.x + R_j * s_k.x, c_j.y + R_j * s_k.y, c_j.z + R_j * s_k.z)
 *     dx    = c_i.x - q.x            (dy, dz alike)
 *     d2    = dx * dx + dy * dy + dz * dz
 *     key_i = min over j in the SAME structure, k in A_j, d2 not NaN,
 *             of ((uint64_t)bits(d2) << 32) | j
 *
 * q is the dot that surface_points() of the Python package lists for (j, k);
 * d2 >= +0, so its bits order like the numbers; j is the index within the
 * structure, as in the neighbour entries.  A minimum is exact and has no order,
 * so the results can be checked bit for bit.
 *
 *   out_depth[i]   = sqrtf(d2 of key_i): the correctly rounded float32 square
 *                    root, taken on the host;
 *   out_nearest[i] = the low word of key_i: the atom that owns the nearest
 *                    accessible dot.  Ties in d2 go to the smallest index.  For
 *                    an exposed atom it is usually i itself;
 *   an atom for which no accessible dot of its structure has a d2 that is not
 *   NaN gets out_depth = +inf and out_nearest = 0xFFFFFFFF;
 *   out_free[i]    (nullable) the exposed count: the popcount of
 *                    rsasa_accessible_points;
 *   out_sasa[i]    (nullable) bit for bit rsasa_calculate_sasa_batch.
 *
 * Dots of other structures of a batch never count.  The depth is measured to
 * the ACCESSIBLE surface (the surface the probe's centre traces); depth - p is
 * the usual estimate of the distance to the molecular surface, and the library
 * does not subtract it.
 *
 * Non-finite input as rsasa_exposure_vectors: a NaN coordinate or radius is
 * taken (the atom's own depth is then +inf / 0xFFFFFFFF, its dots have NaN d2
 * and count for nobody), an infinite coordinate returns
 * RSASA_ERR_GRID_TOO_LARGE and the context stays usable.  The argument errors
 * are those of rsasa_exposure_vectors (n_points == 0, probe_radius + largest
 * radius not a positive finite number, structure_offsets that are not
 * non-decreasing from 0, NULL columns); out_depth or out_nearest NULL where
 * there are atoms returns RSASA_ERR_INVALID_ARGUMENT.  No atoms: RSASA_OK.
 *
 * Synchronous, in the neighbour calls' workspace on the context's first
 * stream: device batches in flight are neither waited for nor disturbed.  The
 * masks stay on the device; 8 bytes per atom cross the link (and 4 each for
 * out_free and out_sasa). */

/* One structure: n_atoms atoms, id nullable (all atoms distinct).
 * out_depth, out_nearest: [n_atoms]; out_free, out_sasa: [n_atoms] or NULL. */
int rsasa_atom_depth(rsasa_context_t *ctx,
                     const float *x, const float *y, const float *z, const float *radius,
                     const uint64_t *id, size_t n_atoms,
                     float probe_radius, size_t n_points,
                     float *out_depth, uint32_t *out_nearest,
                     uint32_t *out_free, float *out_sasa);

/* Directory-mode form: n_structures independent structures concatenated as in
 * rsasa_calculate_sasa_batch (one grid and one max radius each; an empty
 * structure is legal).  out_depth, out_nearest:
 * [structure_offsets[n_structures]]; out_free, out_atom_sasa: the same or NULL.
 * out_nearest holds indices within the atom's structure. */
int rsasa_atom_depth_batch(rsasa_context_t *ctx,
                           const float *x, const float *y, const float *z, const float *radius,
                           const uint64_t *id,
                           const uint32_t *structure_offsets, size_t n_structures,
                           float probe_radius, size_t n_points,
                           float *out_depth, uint32_t *out_nearest,
                           uint32_t *out_free, float *out_atom_sasa);

/* ---- surface components ------------------------------------------------- */

/* WHICH SURFACE a free point belongs to: every accessible dot of a structure
 * labelled by the connected piece of accessible surface it lies on.  A dot on
 * the wall of an internal cavity counts in the SASA value, in rsasa_sas_volume
 * and in rsasa_atom_depth exactly like one that faces bulk solvent; the labels
 * tell them apart.  The result is per dot and not per atom: one atom can own
 * dots on two surfaces.
 *
 * Definition.  Take one structure, probe p, lattice
 * s = rsasa_sphere_points(n_points); A_j is the mask of rsasa_accessible_points
 * under the context's current lane count W.
 *
 *   Dots.   The dots of the structure are the pairs (j, k) with k in A_j,
 *           ordered by (j, k) ascending; a dot's number is its position in
 *           that order, starting at 0 for each structure.
 *   Place.  Float32, unfused, as in rsasa_atom_depth:
 *               R_j = r_j + p
 *               q   = (c_j.x + R_j * s_k.x, c_j.y + R_j * s_k.y, c_j.z + R_j * s_k.z)
 *   Edges.  Two different dots a, b of the same structure are linked when
 *               dx = q_a.x - q_b.x            (dy, dz alike)
 *               d2 = dx * dx + dy * dy + dz * dz
 *               d2 <= link * link             (one float32 product)
 *           A NaN d2 links nothing.  The test is symmetric, because negation
 *           is exact.  Atom ids play no part.
 *   Label.  A component is a connected component of that graph; a dot's label
 *           is the smallest dot number in its component.  A dot whose label
 *           equals its own number is its component's representative.
 *
 * A minimum over a set has no order, so the labels can be checked bit for bit
 * with no tolerance anywhere, whatever the schedule of the GPU.
 *
 *   out_dot_offsets  [n + 1], the exclusive scan of the free counts: atom i's
 *                    dots are [out_dot_offsets[i], out_dot_offsets[i + 1]).  In
 *                    the batch form it is batch-global, like out_offsets of the
 *                    neighbour calls.
 *   out_labels       out_labels[out_dot_offsets[i] .. out_dot_offsets[i + 1])
 *                    are the labels of atom i's accessible points, in ascending
 *                    point order.  Labels are relative to the structure:
 *                    subtract out_dot_offsets[structure_offsets[s]] from an
 *                    array position to get a dot number of structure s.
 *   out_free[i]      (nullable) the exposed count: the popcount of
 *                    rsasa_accessible_points;
 *   out_sasa[i]      (nullable) bit for bit rsasa_calculate_sasa_batch.
 *
 * Sizing, as the neighbour calls: out_dot_offsets is always written (on
 * success and on RSASA_ERR_BUFFER_TOO_SMALL).  If out_labels is NULL or
 * labels_capacity < out_dot_offsets[n], nothing else is written and
 * RSASA_ERR_BUFFER_TOO_SMALL is returned: call once to size, allocate, call
 * again.
 *
 * link must be finite and >= 0 (link = 0 links coinciding dots only); NaN, a
 * negative or an infinite link returns RSASA_ERR_INVALID_ARGUMENT, and so does
 * a batch with 2^32 or more dots.  The remaining argument errors and the
 * non-finite input rules are those of rsasa_atom_depth: a NaN coordinate or
 * radius is taken (the atom's mask is all ones, its dots have NaN positions, so
 * each is a component of its own), an infinite coordinate returns
 * RSASA_ERR_GRID_TOO_LARGE and the context stays usable.  No atoms: RSASA_OK
 * with out_dot_offsets[0] = 0.
 *
 * Synchronous, in the neighbour calls' workspace on the context's first
 * stream: device batches in flight are neither waited for nor disturbed.  The
 * masks and lists stay on the device; 8 bytes per atom and 4 per dot cross the
 * link (and 4 per atom each for out_free and out_sasa). */

/* One structure: n_atoms atoms, id nullable (all atoms distinct).
 * out_dot_offsets: [n_atoms + 1]; out_labels: [labels_capacity]; out_free,
 * out_sasa: [n_atoms] or NULL. */
int rsasa_surface_components(rsasa_context_t *ctx,
                             const float *x, const float *y, const float *z, const float *radius,
                             const uint64_t *id, size_t n_atoms,
                             float probe_radius, size_t n_points, float link,
                             uint64_t *out_dot_offsets,
                             uint32_t *out_labels, size_t labels_capacity,
                             uint32_t *out_free, float *out_sasa);

/* Directory-mode form: n_structures independent structures concatenated as in
 * rsasa_calculate_sasa_batch (one grid and one max radius each; an empty
 * structure is legal); dots of different structures are never linked.
 * out_dot_offsets is batch-global [structure_offsets[n_structures] + 1]. */
int rsasa_surface_components_batch(rsasa_context_t *ctx,
                                   const float *x, const float *y, const float *z, const float *radius,
                                   const uint64_t *id,
                                   const uint32_t *structure_offsets, size_t n_structures,
                                   float probe_radius, size_t n_points, float link,
                                   uint64_t *out_dot_offsets,
                                   uint32_t *out_labels, size_t labels_capacity,
                                   uint32_t *out_free, float *out_atom_sasa);

/* ---- dot crowding ------------------------------------------------------- */

/* HOW MUCH PROTEIN lies around each point of the accessible surface: per
 * accessible dot the number of partner atoms of its structure by distance bin -
 * the buriedness of a surface point that pocket finders and surface
 * fingerprints start from.  A dot in a groove or a pocket has many atoms within
 * 8 - 10 A, a dot on a knob has few, and one atom often owns both kinds: the
 * result is per dot, where rsasa_radial_counts is per atom.
 *
 * Definition.  Take one structure, probe p, lattice
 * s = rsasa_sphere_points(n_points); A_i is the mask of rsasa_accessible_points
 * under the context's current lane count.  Dots, their order and their
 * numbering are exactly those of rsasa_surface_components: the dots are the
 * pairs (i, k) with k in A_i, ordered by (i, k); out_dot_offsets is the
 * exclusive scan of the free counts, batch-global in the batch form.  Each atom
 * j has a flag byte f_j: bit 0 (RSASA_CROWD_PARTNER) - the atom is a partner, it
 * is counted; the other bits are ignored.  edges[0 .. n_bins) are the bins'
 * outer radii.  All arithmetic is float32, unfused, left to right:
 *
 *     R_i   = r_i + p
 *     q     = (c_i.x + R_i * s_k.x, c_i.y + R_i * s_k.y, c_i.z + R_i * s_k.z)     the dot (i, k)
 *     e2[b] = edges[b] * edges[b]        (may overflow to +inf, underflow to 0)
 *     dx = c_j.x - q.x                   (dy, dz alike)
 *     d2 = dx * dx + dy * dy + dz * dz
 *     j counts for the dot  iff  j is in the SAME structure, (f_j & 1),
 *                                d2 <= e2[n_bins - 1]
 *     bin = the smallest b with d2 <= e2[b]
 *     out_counts[dot][bin] += 1
 *
 * The dot's own atom i is an atom like any other: it counts if its partner bit
 * is set, in the bin where d2 (about R_i^2) falls.  flags == NULL: every atom is
 * a partner.  A NaN d2 counts nowhere - the dots of an atom with a NaN
 * coordinate or radius get all-zero rows, and such an atom counts for nobody.
 * Of several equal edges the first takes the pair and the others stay empty, as
 * in rsasa_radial_counts.  Atom ids play no part beyond the masks.  The counts
 * are integers and have no order, so they can be checked for equality.
 * Unlike the calls on the grid alone, radius and probe_radius matter here: they
 * place the dots.
 *
 *   out_dot_offsets  [n + 1], as rsasa_surface_components writes it;
 *   out_counts       [counts_capacity][n_bins], row-major: row d is dot d, the
 *                    rows line up one to one with out_labels of
 *                    rsasa_surface_components;
 *   out_free[i]      (nullable) the exposed count: the popcount of
 *                    rsasa_accessible_points;
 *   out_sasa[i]      (nullable) bit for bit rsasa_calculate_sasa_batch.
 *
 * Sizing, as rsasa_surface_components: out_dot_offsets is always written (on
 * success and on RSASA_ERR_BUFFER_TOO_SMALL).  If out_counts is NULL or
 * counts_capacity (in dots) < out_dot_offsets[n], nothing else is written and
 * RSASA_ERR_BUFFER_TOO_SMALL is returned: call once to size, allocate, call
 * again.  A batch with 2^32 or more dots returns RSASA_ERR_INVALID_ARGUMENT.
 *
 * n_bins must lie in [1, RSASA_CROWD_MAX_BINS]; every edge must be finite and
 * >= 0 (-0.0 is 0) and the edges non-decreasing (equal edges are allowed);
 * anything else, and NULL edges, returns RSASA_ERR_INVALID_ARGUMENT.  The
 * remaining argument errors and the non-finite input rules are those of
 * rsasa_atom_depth: a NaN coordinate or radius is taken, an infinite coordinate
 * returns RSASA_ERR_GRID_TOO_LARGE and the context stays usable.  No atoms:
 * RSASA_OK with out_dot_offsets[0] = 0.  The call holds 4 * n_bins bytes per dot
 * on the device; a failed reservation returns RSASA_ERR_OUT_OF_MEMORY and the
 * context stays usable.
 *
 * Synchronous, in the neighbour calls' workspace on the context's first
 * stream: device batches in flight are neither waited for nor disturbed.  The
 * masks and lists stay on the device; 8 bytes per atom and 4 * n_bins per dot
 * cross the link (and 4 per atom each for out_free and out_sasa). */
#define RSASA_CROWD_PARTNER 1
#define RSASA_CROWD_MAX_BINS 8

/* One structure: n_atoms atoms, id nullable (all atoms distinct).  flags:
 * [n_atoms] or NULL; edges: [n_bins]; out_dot_offsets: [n_atoms + 1];
 * out_counts: [counts_capacity][n_bins]; out_free, out_sasa: [n_atoms] or NULL. */
int rsasa_dot_crowding(rsasa_context_t *ctx,
                       const float *x, const float *y, const float *z, const float *radius,
                       const uint64_t *id, size_t n_atoms,
                       float probe_radius, size_t n_points,
                       const uint8_t *flags, const float *edges, uint32_t n_bins,
                       uint64_t *out_dot_offsets,
                       uint32_t *out_counts, size_t counts_capacity,
                       uint32_t *out_free, float *out_sasa);

/* Directory-mode form: n_structures independent structures concatenated as in
 * rsasa_calculate_sasa_batch (one grid and one max radius each; an empty
 * structure is legal); atoms of other structures never count.  flags runs over
 * structure_offsets[n_structures] atoms; out_dot_offsets is batch-global
 * [structure_offsets[n_structures] + 1]. */
int rsasa_dot_crowding_batch(rsasa_context_t *ctx,
                             const float *x, const float *y, const float *z, const float *radius,
                             const uint64_t *id,
                             const uint32_t *structure_offsets, size_t n_structures,
                             float probe_radius, size_t n_points,
                             const uint8_t *flags, const float *edges, uint32_t n_bins,
                             uint64_t *out_dot_offsets,
                             uint32_t *out_counts, size_t counts_capacity,
                             uint32_t *out_free, float *out_atom_sasa);

/* ---- dot fields --------------------------------------------------------- */

/* WHAT THE CHEMISTRY looks like from each point of the accessible surface: per
 * accessible dot and channel the sum, over the partner atoms of its structure
 * within a cutoff, of a per-atom weight times a distance kernel - the
 * electrostatic potential at the dot from the partial charges, the lipophilic
 * potential from per-atom hydropathy, or a plain sum of a property within a
 * radius: the columns that surface fingerprints, pocket scorers and interface
 * maps put beside the shape columns.  rsasa_dot_crowding visits the same (dot,
 * atom) pairs and adds 1; this adds weight * g(distance), up to
 * RSASA_FIELD_MAX_CHANNELS channels in one call.
 *
 * The result is a 64-bit fixed-point integer per dot and channel with 24
 * fraction bits.  A float sum would depend on the order in which the atoms are
 * met; an integer sum does not, so the result can be checked for equality.
 *
 * Definition.  The dots, their order, out_dot_offsets, out_free, out_sasa, the
 * masks and the flag byte are those of rsasa_dot_crowding: bit 0 of f_j
 * (RSASA_FIELD_PARTNER) - the atom is a partner; the other bits are ignored;
 * flags == NULL: every atom is a partner.  weights is float32[n][n_channels],
 * row-major, kinds is uint8[n_channels].  All arithmetic is float32, unfused,
 * left to right; division and square root are correctly rounded and
 * subnormals are kept:
 *
 *     R_i = r_i + p;   q = c_i + R_i * s_k  (per component)      the dot (i, k), as rsasa_dot_crowding
 *     c2  = cutoff * cutoff              (may overflow to +inf, underflow to 0)
 *     dx  = c_j.x - q.x                  (dy, dz alike)
 *     d2  = dx * dx + dy * dy + dz * dz;   d = sqrtf(d2)
 *     j counts for the dot  iff  j is in the SAME structure, (f_j & 1), d2 <= c2
 *     g[RSASA_FIELD_STEP    = 0] = 1.0f
 *     g[RSASA_FIELD_INV_D   = 1] = 1.0f / d              Coulomb
 *     g[RSASA_FIELD_INV_D2  = 2] = 1.0f / d2             Coulomb with a dielectric proportional to d
 *     g[RSASA_FIELD_INV_1PD = 3] = 1.0f / (1.0f + d)     Audry's lipophilic potential
 *     t = weights[j][c] * g[kinds[c]]
 *     if |t| <= 0x1p24f:  out_sums[dot][c] += rint(t * 2^24)
 *
 * rint rounds to nearest, ties to even; t * 2^24 is exact; the sum is an int64
 * in two's complement and wraps.  A term that is NaN or above 2^24 in magnitude
 * adds nothing: a NaN or infinite weight, and d2 == 0 under RSASA_FIELD_INV_D
 * and RSASA_FIELD_INV_D2 (g is +inf there; under RSASA_FIELD_INV_1PD g is 1 at
 * d == 0 and the term counts).  A NaN d2 counts nowhere, as in rsasa_dot_crowding.  The dot's own atom
 * is an atom like any other.  Every row is written, the all-zero ones included.
 * The value of a field is out_sums * 2^-24.
 *
 * 24 fraction bits match float32 at magnitude 1; with the 2^24 bound a term
 * takes at most 48 bits plus sign, so a sum can wrap only beyond 2^15 partners
 * at that bound - and is defined there too, because it wraps.
 *
 *   out_dot_offsets  [n + 1], as rsasa_dot_crowding writes it;
 *   out_sums         [sums_capacity][n_channels], row-major: row d is dot d,
 *                    lined up with the rows of rsasa_dot_crowding;
 *   out_free[i]      (nullable) the popcount of rsasa_accessible_points;
 *   out_sasa[i]      (nullable) bit for bit rsasa_calculate_sasa_batch.
 *
 * Sizing, as rsasa_dot_crowding: out_dot_offsets is always written (on success
 * and on RSASA_ERR_BUFFER_TOO_SMALL).  If out_sums is NULL or sums_capacity (in
 * dots) < out_dot_offsets[n], nothing else is written and
 * RSASA_ERR_BUFFER_TOO_SMALL is returned.  A batch with 2^32 or more dots
 * returns RSASA_ERR_INVALID_ARGUMENT.
 *
 * n_channels must lie in [1, RSASA_FIELD_MAX_CHANNELS], every kind must be one
 * of the four above, cutoff must be finite and >= 0 (-0.0 is 0); anything else,
 * NULL kinds, and NULL weights where there are atoms, returns
 * RSASA_ERR_INVALID_ARGUMENT.  The values of weights are not checked.  The
 * remaining argument errors, the non-finite input rules, empty input, the
 * workspace and the streams are those of rsasa_dot_crowding.  The call holds
 * 8 * n_channels bytes per dot (and 4 * n_channels per atom) on the device; 8
 * bytes per atom and 8 * n_channels per dot cross the link back. */
#define RSASA_FIELD_PARTNER 1
#define RSASA_FIELD_MAX_CHANNELS 4
#define RSASA_FIELD_STEP 0
#define RSASA_FIELD_INV_D 1
#define RSASA_FIELD_INV_D2 2
#define RSASA_FIELD_INV_1PD 3

/* One structure: n_atoms atoms, id nullable (all atoms distinct).  flags:
 * [n_atoms] or NULL; weights: [n_atoms][n_channels]; kinds: [n_channels];
 * out_dot_offsets: [n_atoms + 1]; out_sums: [sums_capacity][n_channels];
 * out_free, out_sasa: [n_atoms] or NULL. */
int rsasa_dot_fields(rsasa_context_t *ctx,
                     const float *x, const float *y, const float *z, const float *radius,
                     const uint64_t *id, size_t n_atoms,
                     float probe_radius, size_t n_points,
                     const uint8_t *flags, const float *weights, const uint8_t *kinds, uint32_t n_channels,
                     float cutoff,
                     uint64_t *out_dot_offsets,
                     int64_t *out_sums, size_t sums_capacity,
                     uint32_t *out_free, float *out_sasa);

/* Directory-mode form, as rsasa_dot_crowding_batch: atoms of other structures
 * never count; flags and weights run over structure_offsets[n_structures]
 * atoms; out_dot_offsets is batch-global. */
int rsasa_dot_fields_batch(rsasa_context_t *ctx,
                           const float *x, const float *y, const float *z, const float *radius,
                           const uint64_t *id,
                           const uint32_t *structure_offsets, size_t n_structures,
                           float probe_radius, size_t n_points,
                           const uint8_t *flags, const float *weights, const uint8_t *kinds, uint32_t n_channels,
                           float cutoff,
                           uint64_t *out_dot_offsets,
                           int64_t *out_sums, size_t sums_capacity,
                           uint32_t *out_free, float *out_atom_sasa);

/* ---- dot curvature ------------------------------------------------------ */

/* HOW THE SURFACE BENDS at each of its points: per accessible dot the moments
 * from which mean curvature, the two principal curvatures, Gaussian curvature
 * and the shape index follow - the shape columns that surface fingerprints
 * start from, beside which they put rsasa_dot_fields' chemistry.  The dots
 * within a reach of a dot are a sample of the surface around it; the call
 * reduces every such pair on the device to nine integers per dot instead of
 * listing the pairs (rsasa_dot_links at link = reach lists them).
 *
 * Definition.  The dots, their order, out_dot_offsets, out_free, out_sasa and
 * the masks are those of rsasa_surface_components and rsasa_dot_links.  Dot a is
 * point k of atom i; its outward normal is the lattice point itself, n = s_k,
 * the float32 values of rsasa_sphere_points(n_points)[k].  For every other dot
 * b of the SAME structure, all arithmetic float32, unfused, in the order
 * written; the division is correctly rounded and subnormals are kept:
 *
 *     R_i = r_i + p;   q_a = c_i + R_i * s_k  (per component)    the dot, as rsasa_dot_links
 *     reach2 = reach * reach           (may overflow to +inf, underflow to 0)
 *     dx = q_b.x - q_a.x               (dy, dz alike)
 *     d2 = dx * dx + dy * dy + dz * dz                           the bits of rsasa_dot_links' d2
 *     h  = (n.x * dx + n.y * dy) + n.z * dz                      height of b over a's tangent plane
 *     tx = dx - h * n.x                (ty, tz alike)            tangential part of the chord
 *     t2 = (tx * tx + ty * ty) + tz * tz
 *     g  = h / t2
 *     term[RSASA_CURV_D2 = 0] = d2
 *     term[RSASA_CURV_H  = 1] = h
 *     term[RSASA_CURV_XX = 2] = (tx * tx) * g        term[RSASA_CURV_XY = 5] = (tx * ty) * g
 *     term[RSASA_CURV_YY = 3] = (ty * ty) * g        term[RSASA_CURV_XZ = 6] = (tx * tz) * g
 *     term[RSASA_CURV_ZZ = 4] = (tz * tz) * g        term[RSASA_CURV_YZ = 7] = (ty * tz) * g
 *
 * The drop rule.  The pair (a, b) counts iff b != a, d2 <= reach2 (a NaN
 * fails), d2 > 0, t2 > 0, and every one of the eight terms has
 * |term| <= 0x1p24f (a NaN fails).  A pair counts for all columns or for
 * none: a coincident dot, a dot straight above or below a along its normal, a
 * dot of an atom with a NaN coordinate or radius, and a pair one of whose terms
 * leaves the fixed point's range add nothing anywhere.  A pair that counts adds
 * 1 to out_pairs[a] and rint(term[c] * 2^24) to out_moments[a][c]; rint rounds
 * to nearest, ties to even; term * 2^24 is exact.  The moments are int64 in
 * two's complement with 24 fraction bits - rsasa_dot_fields' fixed point -
 * and wrap.  Integer sums have no order, so the rows can be checked for
 * equality.  Every row is written, the all-zero ones included.
 *
 * What the sums mean.  On a sphere of radius rho every chord has
 * h = -d2 / (2 rho), so
 *     H = -2 * Sum(h) / Sum(d2)
 * is the least-squares normal curvature under the weights d2: positive on
 * convex surface, negative in seams and pockets; near-coincident dots carry
 * almost no weight and nothing is divided by d2.  With T = t / |t|,
 *     M = -2 * Sum(h T T^t) / Sum(d2)
 * - the six moment columns over the first - is Taubin's curvature tensor under
 * the same weights.  M n ~ 0 and tr M = H up to rounding; its two tangential
 * eigenvalues m1 >= m2 are (tr M +- sqrt(2 |M|_F^2 - (tr M)^2)) / 2 and give the
 * principal curvatures k1 = 3 m1 - m2, k2 = 3 m2 - m1: the caller needs neither
 * the normals nor an eigen-solver.
 *
 * The estimator's limits.  The mean is robust at any density: on a lone sphere
 * of radius R = 1.8 + 1.4 with coordinates of about 10, H * R stays within 5e-6
 * of 1 at 100 and at 960 points, at reach 1.5 and 3.0.  The principal split is
 * not that tight, because the golden-spiral neighbours of a dot are not
 * angularly uniform: on the same sphere at reach 3.0, k1 * R ranges over
 * 1.02 .. 1.41 at 100 points and over 1.00 .. 1.11 at 960.  The split wants
 * about 50 pairs or more per dot (there are about 20 at 100 points).  Dots at
 * the rim of the accessible surface see a half-disc of neighbours, which biases
 * both.  These are properties of the estimator, not of the implementation.
 *
 *   out_dot_offsets  [n + 1], as rsasa_surface_components writes it;
 *   out_pairs        [dots_capacity]: the pairs that count, per dot;
 *   out_moments      [dots_capacity][RSASA_CURV_COLUMNS], row-major: row d is
 *                    dot d, lined up with the rows of rsasa_dot_crowding;
 *   out_free[i]      (nullable) the popcount of rsasa_accessible_points;
 *   out_sasa[i]      (nullable) bit for bit rsasa_calculate_sasa_batch.
 *
 * Sizing takes two calls, as rsasa_dot_crowding: out_dot_offsets is always
 * written (on success and on RSASA_ERR_BUFFER_TOO_SMALL).  If out_pairs or
 * out_moments is NULL or dots_capacity < out_dot_offsets[n], nothing else is
 * written or computed and RSASA_ERR_BUFFER_TOO_SMALL is returned.  A batch
 * with 2^32 or more dots returns RSASA_ERR_INVALID_ARGUMENT.
 *
 * reach must be finite and >= 0 (-0.0 is 0); anything else returns
 * RSASA_ERR_INVALID_ARGUMENT.  reach == 0 is legal: no pair counts and every
 * row is zero.  The work grows with the cube of the reach (every dot of the
 * reach is tested against every dot of the atom), as in rsasa_dot_links.  The
 * remaining argument errors, the non-finite input rules, empty input, the
 * workspace and the streams are those of rsasa_surface_components.  The call
 * holds 68 bytes per dot on the device; 8 bytes per atom and 68 per dot cross
 * the link back. */
#define RSASA_CURV_COLUMNS 8
#define RSASA_CURV_D2 0
#define RSASA_CURV_H 1
#define RSASA_CURV_XX 2
#define RSASA_CURV_YY 3
#define RSASA_CURV_ZZ 4
#define RSASA_CURV_XY 5
#define RSASA_CURV_XZ 6
#define RSASA_CURV_YZ 7

/* One structure: n_atoms atoms, id nullable (all atoms distinct).
 * out_dot_offsets: [n_atoms + 1]; out_pairs: [dots_capacity]; out_moments:
 * [dots_capacity][8]; out_free, out_sasa: [n_atoms] or NULL. */
int rsasa_dot_curvature(rsasa_context_t *ctx,
                        const float *x, const float *y, const float *z, const float *radius,
                        const uint64_t *id, size_t n_atoms,
                        float probe_radius, size_t n_points,
                        float reach,
                        uint64_t *out_dot_offsets,
                        uint32_t *out_pairs, int64_t *out_moments, size_t dots_capacity,
                        uint32_t *out_free, float *out_sasa);

/* Directory-mode form, as rsasa_dot_crowding_batch: dots of different
 * structures never pair; out_dot_offsets is batch-global. */
int rsasa_dot_curvature_batch(rsasa_context_t *ctx,
                              const float *x, const float *y, const float *z, const float *radius,
                              const uint64_t *id,
                              const uint32_t *structure_offsets, size_t n_structures,
                              float probe_radius, size_t n_points,
                              float reach,
                              uint64_t *out_dot_offsets,
                              uint32_t *out_pairs, int64_t *out_moments, size_t dots_capacity,
                              uint32_t *out_free, float *out_atom_sasa);

/* ---- dot enclosure ------------------------------------------------------ */

/* HOW ENCLOSED each point of the accessible surface is: per accessible dot the
 * directions, of a fixed fan, in which a probe leaving the dot on a straight
 * path is stopped by protein within a given length - the buriedness that
 * pocket finders rank by.  A count of atoms by distance (rsasa_dot_crowding)
 * does not see direction: a dot on a flat face over a thick slab and a dot in a
 * narrow pocket have as many atoms within 10 A, but the first has a half-space
 * open and the second almost nothing.
 *
 * Definition.  Take one structure, probe p, lattice
 * s = rsasa_sphere_points(n_points) and directions
 * u = rsasa_sphere_points(n_dirs), 1 <= n_dirs <= RSASA_ENCLOSE_MAX_DIRS.  Dots,
 * their order and out_dot_offsets are exactly those of
 * rsasa_surface_components and rsasa_dot_crowding.  Each atom j has a flag byte
 * f_j: bit 0 (RSASA_ENCLOSE_PARTNER) - the atom is an obstacle; the other bits
 * are ignored; flags == NULL: every atom is an obstacle.  reach = L is the
 * length of a ray.  All arithmetic is float32, unfused, left to right.  For the
 * dot (i, k), direction m and an obstacle j != i (by atom index: a coincident
 * twin is an obstacle like any other) of the SAME structure:
 *
 *     R_i = r_i + p
 *     q   = (c_i.x + R_i * s_k.x, c_i.y + R_i * s_k.y, c_i.z + R_i * s_k.z)
 *     R_j = r_j + p;   R2 = R_j * R_j
 *     dx = c_j.x - q.x                          (dy, dz alike)
 *     d2 = dx * dx + dy * dy + dz * dz
 *     t  = dx * u_m.x + dy * u_m.y + dz * u_m.z
 *     j stops ray m  iff  t > 0  and
 *         ( t <= L  ?  d2 - t * t <= R2
 *                   :  ex = dx - L * u_m.x (ey, ez alike);
 *                      ex * ex + ey * ey + ez * ez <= R2 )
 *
 * In words: the segment q + t u_m, 0 <= t <= L, meets the expanded sphere of j -
 * its nearest point to c_j is the foot of the perpendicular or the far end.  The
 * ray is the path of a probe CENTRE, so the obstacle is the expanded sphere, the
 * one that defines the dots.  A sphere behind the start (t <= 0) stops nothing:
 * accessible dots lie outside every other expanded sphere.
 *
 * The own atom i is not put through this test (its dot lies on its own sphere
 * up to rounding).  It stops ray m iff it has the obstacle bit and
 *
 *     u_m.x * s_k.x + u_m.y * s_k.y + u_m.z * s_k.z < 0
 *
 * - the ray enters the sphere it starts on; a tangent ray is free; L plays no
 * part.
 *
 * out_blocked[dot] is a uint32: bit m is set iff the own-atom rule or some
 * obstacle stops ray m; bits >= n_dirs are 0.  The decisions are booleans OR-ed
 * over the obstacles, so the words have no order and can be checked for
 * equality.  A NaN anywhere fails its comparison and stops nothing:
 *   - a NaN obstacle (coordinate or radius) stops no ray;
 *   - the dots of an atom with a NaN coordinate or radius are stopped by no
 *     other atom, whatever t > 0 gives;
 *   - their own-atom bits stay as the lattice gives them (that rule reads only
 *     u_m and s_k).
 *
 *   out_dot_offsets  [n + 1], as rsasa_surface_components writes it;
 *   out_blocked      [blocked_capacity]: word d is dot d, lined up with
 *                    out_labels of rsasa_surface_components and the rows of
 *                    rsasa_dot_crowding;
 *   out_free[i]      (nullable) the popcount of rsasa_accessible_points;
 *   out_sasa[i]      (nullable) bit for bit rsasa_calculate_sasa_batch.
 *
 * Sizing, as rsasa_dot_crowding: out_dot_offsets is always written (on success
 * and on RSASA_ERR_BUFFER_TOO_SMALL).  If out_blocked is NULL or
 * blocked_capacity (in dots) < out_dot_offsets[n], nothing else is written and
 * RSASA_ERR_BUFFER_TOO_SMALL is returned: call once to size, allocate, call
 * again.  A batch with 2^32 or more dots returns RSASA_ERR_INVALID_ARGUMENT.
 *
 * n_dirs must lie in [1, RSASA_ENCLOSE_MAX_DIRS]; reach must be finite and >= 0
 * (-0.0 is 0); anything else returns RSASA_ERR_INVALID_ARGUMENT.  The remaining
 * argument errors and the non-finite input rules are those of rsasa_atom_depth.
 * No atoms: RSASA_OK with out_dot_offsets[0] = 0.  The call holds 4 bytes per dot
 * on the device; a failed reservation returns RSASA_ERR_OUT_OF_MEMORY and the
 * context stays usable.
 *
 * Synchronous, in the neighbour calls' workspace on the context's first
 * stream: device batches in flight are neither waited for nor disturbed.  8
 * bytes per atom and 4 per dot cross the link (and 4 per atom each for
 * out_free and out_sasa). */
#define RSASA_ENCLOSE_PARTNER 1
#define RSASA_ENCLOSE_MAX_DIRS 32

/* One structure: n_atoms atoms, id nullable (all atoms distinct).  flags:
 * [n_atoms] or NULL; out_dot_offsets: [n_atoms + 1]; out_blocked:
 * [blocked_capacity]; out_free, out_sasa: [n_atoms] or NULL. */
int rsasa_dot_enclosure(rsasa_context_t *ctx,
                        const float *x, const float *y, const float *z, const float *radius,
                        const uint64_t *id, size_t n_atoms,
                        float probe_radius, size_t n_points,
                        const uint8_t *flags, float reach, uint32_t n_dirs,
                        uint64_t *out_dot_offsets,
                        uint32_t *out_blocked, size_t blocked_capacity,
                        uint32_t *out_free, float *out_sasa);

/* Directory-mode form: n_structures independent structures concatenated as in
 * rsasa_calculate_sasa_batch (one grid each; an empty structure is legal);
 * atoms of other structures stop nothing.  flags runs over
 * structure_offsets[n_structures] atoms; out_dot_offsets is batch-global. */
int rsasa_dot_enclosure_batch(rsasa_context_t *ctx,
                              const float *x, const float *y, const float *z, const float *radius,
                              const uint64_t *id,
                              const uint32_t *structure_offsets, size_t n_structures,
                              float probe_radius, size_t n_points,
                              const uint8_t *flags, float reach, uint32_t n_dirs,
                              uint64_t *out_dot_offsets,
                              uint32_t *out_blocked, size_t blocked_capacity,
                              uint32_t *out_free, float *out_atom_sasa);

/* ---- half-sphere exposure ----------------------------------------------- */

/* HOW CROWDED the two sides of an atom are: per centre atom the number of
 * partner atoms of its own structure within a cutoff, split by the plane
 * through the centre that is normal to a direction the caller gives
 * (half-sphere exposure, Hamelryck: HSE-up and HSE-down; their sum is the
 * contact or coordination number).  The cutoff is 12-15 A in practice, four to
 * five times the reach of the neighbour lists; the cell grid is swept as far
 * as the cutoff needs.
 *
 * Definition.  For a structure, each atom i has centre c_i, a direction u_i
 * (3 float32 values of any length, zero allowed) and a flag byte f_i: bit 0
 * (RSASA_HSE_PARTNER) - the atom is a partner, it is counted; bit 1
 * (RSASA_HSE_CENTRE) - the atom is a centre, it gets a result; the other bits
 * are ignored.  C is the cutoff.  All arithmetic is float32, unfused, left to
 * right, as in rsasa_atom_depth:
 *
 *     c2   = C * C
 *     dx   = c_j.x - c_i.x                 (dy, dz alike)
 *     d2   = dx * dx + dy * dy + dz * dz
 *     side = dx * u_i.x + dy * u_i.y + dz * u_i.z
 *     j counts for i  iff  j != i, j in the SAME structure, (f_j & 1), d2 <= c2
 *     out_up[i]   = number of counting j with side >= 0
 *     out_down[i] = number of counting j with !(side >= 0)
 *
 * An atom without bit 1 gets out_up = out_down = 0.  flags == NULL: every atom
 * is both a centre and a partner.  dirs == NULL: side is taken as +0 for
 * everybody, so out_down is all zero and out_up is the contact number.  A NaN
 * coordinate makes d2 NaN: that atom counts for nobody and, as a centre, gets
 * 0 / 0.  A NaN component of u_i sends every partner of i to out_down.  A
 * coincident atom (d2 == 0, side == 0) counts as up.  c2 may overflow to +inf:
 * then every atom whose d2 is not NaN counts.  Atom ids play no part.  The
 * counts are integers and have no order, so they can be checked for equality.
 *
 * radius and probe_radius are taken, and checked by the rules of the other
 * calls (probe_radius + largest radius a positive finite number), only because
 * they fix the cell size of the grid; the result does not depend on them.
 *
 * cutoff must be finite and >= 0 (-0.0 is 0); NaN, a negative or an infinite
 * cutoff returns RSASA_ERR_INVALID_ARGUMENT, and so do NULL columns,
 * structure_offsets that are not non-decreasing from 0, and out_up or out_down
 * NULL where there are atoms.  An infinite coordinate returns
 * RSASA_ERR_GRID_TOO_LARGE and the context stays usable.  No atoms: RSASA_OK.
 *
 * Synchronous, in the neighbour calls' workspace on the context's first
 * stream: device batches in flight are neither waited for nor disturbed.  No
 * neighbour lists are built; 8 bytes per atom come back. */
#define RSASA_HSE_PARTNER 1
#define RSASA_HSE_CENTRE 2

/* One structure: n_atoms atoms, id nullable (it plays no part).  dirs: [3 * n_atoms]
 * (x, y, z per atom) or NULL; flags: [n_atoms] or NULL; out_up, out_down:
 * [n_atoms]. */
int rsasa_half_sphere_exposure(rsasa_context_t *ctx,
                               const float *x, const float *y, const float *z, const float *radius,
                               const uint64_t *id, size_t n_atoms,
                               float probe_radius,
                               const float *dirs, const uint8_t *flags, float cutoff,
                               uint32_t *out_up, uint32_t *out_down);

/* Directory-mode form: n_structures independent structures concatenated as in
 * rsasa_calculate_sasa_batch (one grid each; an empty structure is legal);
 * atoms of other structures never count.  dirs, flags, out_up, out_down run
 * over structure_offsets[n_structures] atoms. */
int rsasa_half_sphere_exposure_batch(rsasa_context_t *ctx,
                                     const float *x, const float *y, const float *z, const float *radius,
                                     const uint64_t *id,
                                     const uint32_t *structure_offsets, size_t n_structures,
                                     float probe_radius,
                                     const float *dirs, const uint8_t *flags, float cutoff,
                                     uint32_t *out_up, uint32_t *out_down);

/* ---- atoms within a cutoff ---------------------------------------------- */

/* WHO is within a cutoff of an atom: per centre atom the list of the partner
 * atoms of its own structure within a cutoff, each with its squared distance -
 * what rsasa_half_sphere_exposure counts, named.  Residue contact maps (closest
 * heavy atoms within 4.5 / 6 / 8 A), CA or CB contact maps at 8-10 A, contact
 * order, residue-interaction networks and the radius graphs of structure
 * networks start from these lists; the neighbour lists of
 * rsasa_precompute_neighbors stop at r_i + max_r + 2 probe (about 6.5 A).
 *
 * Definition.  For a structure, each atom i has centre c_i and a flag byte f_i:
 * bit 0 (RSASA_WITHIN_PARTNER) - the atom is a partner, it is listed; bit 1
 * (RSASA_WITHIN_CENTRE) - the atom is a centre, it gets a list; the other bits
 * are ignored (the bits of RSASA_HSE_PARTNER / RSASA_HSE_CENTRE).  C is the
 * cutoff.  All arithmetic is float32, unfused, left to right, exactly as in
 * rsasa_half_sphere_exposure:
 *
 *     c2 = C * C
 *     dx = c_j.x - c_i.x                 (dy, dz alike)
 *     d2 = dx * dx + dy * dy + dz * dz
 *     j is in i's list  iff  (f_i & 2), j != i, j in the SAME structure,
 *                            (f_j & 1), d2 <= c2,
 *                            and, when upper_only != 0, j > i
 *
 * Lists.  The list of atom i is out_entries[out_offsets[i] .. out_offsets[i+1]).
 * An atom without bit 1 has an empty list.  flags == NULL: every atom is both
 * a centre and a partner.  Each entry holds the float32 d2 of the definition
 * and idx, the partner's index within its structure (in the one-structure
 * call: its input index).
 *
 * Order.  Every list is ascending by (d2, idx) - the order of the 64-bit key
 * (bits(d2) << 32) | idx: d2 in a list is never NaN or negative, so its bits
 * order like the numbers; +inf can appear only when c2 overflows, and orders
 * last.  The result can therefore be compared byte for byte.
 *
 * Symmetry.  d2 is the same bit pattern in both directions (float subtraction
 * is exactly antisymmetric): with every flag 3 and upper_only == 0, j is in
 * i's list with d2 exactly when i is in j's with the same d2.
 *
 * Relation to the half-sphere exposure.  With upper_only == 0,
 * out_offsets[i+1] - out_offsets[i] equals out_up[i] + out_down[i] of
 * rsasa_half_sphere_exposure for the same flags and cutoff.
 *
 * A NaN coordinate makes d2 NaN: that atom is in nobody's list and, as a
 * centre, has an empty list.  c2 may overflow to +inf: then every partner whose
 * d2 is not NaN is listed.  Atom ids play no part.
 *
 * radius and probe_radius are taken, and checked by the rules of the other
 * calls (probe_radius + largest radius a positive finite number), only because
 * they fix the cell size of the grid; the result does not depend on them.
 *
 * cutoff must be finite and >= 0 (-0.0 is 0); NaN, a negative or an infinite
 * cutoff returns RSASA_ERR_INVALID_ARGUMENT, and so do NULL columns,
 * structure_offsets that are not non-decreasing from 0, and out_offsets NULL.
 * An infinite coordinate returns RSASA_ERR_GRID_TOO_LARGE and the context stays
 * usable.  No atoms: RSASA_OK with out_offsets[0] = 0.
 *
 * Sizing, as in rsasa_precompute_neighbors: out_offsets is always written (on
 * success and on RSASA_ERR_BUFFER_TOO_SMALL).  If out_entries is NULL or
 * entries_capacity < out_offsets[n], nothing else is written and
 * RSASA_ERR_BUFFER_TOO_SMALL is returned: call once to size, allocate, call
 * again - or pass a generous buffer (all-atom lists of proteins hold about
 * 0.2 C^3 entries each, C in A).  The entries take 8 bytes each on the device
 * as well; a failed reservation returns RSASA_ERR_OUT_OF_MEMORY and the context
 * stays usable.
 *
 * Synchronous, in the neighbour calls' workspace on the context's first
 * stream: device batches in flight are neither waited for nor disturbed.  No
 * neighbour lists are built. */
typedef struct rsasa_within {
    float d2;     /* squared distance to the centre, float32 as defined above */
    uint32_t idx; /* the partner's index within its structure */
} rsasa_within_t; /* 8 bytes */
#define RSASA_WITHIN_PARTNER 1
#define RSASA_WITHIN_CENTRE 2

/* One structure: n_atoms atoms, id nullable (it plays no part).  flags:
 * [n_atoms] or NULL; out_offsets: [n_atoms + 1]; out_entries:
 * [entries_capacity]. */
int rsasa_atoms_within(rsasa_context_t *ctx,
                       const float *x, const float *y, const float *z, const float *radius,
                       const uint64_t *id, size_t n_atoms,
                       float probe_radius,
                       const uint8_t *flags, float cutoff, int upper_only,
                       uint64_t *out_offsets,
                       rsasa_within_t *out_entries, size_t entries_capacity);

/* Directory-mode form: n_structures independent structures concatenated as in
 * rsasa_calculate_sasa_batch (one grid each; an empty structure is legal); no
 * list crosses structures.  flags runs over structure_offsets[n_structures]
 * atoms; out_offsets is batch-global [structure_offsets[n_structures] + 1]; idx
 * is the index within the partner's (= the centre's) structure. */
int rsasa_atoms_within_batch(rsasa_context_t *ctx,
                             const float *x, const float *y, const float *z, const float *radius,
                             const uint64_t *id,
                             const uint32_t *structure_offsets, size_t n_structures,
                             float probe_radius,
                             const uint8_t *flags, float cutoff, int upper_only,
                             uint64_t *out_offsets,
                             rsasa_within_t *out_entries, size_t entries_capacity);

/* ---- dot links ---------------------------------------------------------- */

/* WHICH DOTS are next to a dot on the accessible surface: the graph that
 * rsasa_surface_components labels, returned as per-dot lists in CSR form - the
 * edge list of a graph network over the surface points, as rsasa_atoms_within
 * is for atoms (declared here, behind rsasa_within_t, which its entries are).
 *
 * Definition.  Dots, their numbering, their positions q and the edge test are
 * exactly those of rsasa_surface_components (see there: Dots, Place, Edges).
 * The list of dot a holds every other dot b of its structure with float32
 * d2 <= link * link.  Each entry is an rsasa_within_t: that d2, and idx = b's dot
 * number within the structure.  Lists are ascending by the key
 * (bits(d2) << 32) | idx, so the result compares byte for byte.  The test is
 * symmetric: b is in a's list with the same d2 exactly when a is in b's.  A NaN
 * dot has an empty list and is in nobody's.
 *
 *   out_dot_offsets   [n + 1], as rsasa_surface_components writes it; D is
 *                     out_dot_offsets[n];
 *   out_n_links       the total number of entries, written whenever
 *                     out_dot_offsets is (0 if the call fails behind its
 *                     argument rules before it has counted them);
 *   out_link_offsets  [D + 1] (room for dots_capacity + 1): the list of the dot
 *                     at array position d (batch-global, as out_labels is
 *                     indexed) is out_entries[out_link_offsets[d] ..
 *                     out_link_offsets[d + 1]); 64-bit, batch-global;
 *   out_entries       [entries_capacity];
 *   out_free[i]       (nullable) the popcount of rsasa_accessible_points;
 *   out_sasa[i]       (nullable) bit for bit rsasa_calculate_sasa_batch.
 *
 * Sizing, in two calls: out_dot_offsets and *out_n_links are always written (on
 * success and on RSASA_ERR_BUFFER_TOO_SMALL).  If out_link_offsets or
 * out_entries is NULL, dots_capacity < D or entries_capacity < *out_n_links,
 * nothing else is written and RSASA_ERR_BUFFER_TOO_SMALL is returned: call once
 * to size, allocate, call again - or pass generous buffers (a protein at 100
 * points and the default link has about 6.4 dots per atom and 8.3 entries per
 * dot).  The entries take 8 bytes each on the device as well (twice: in sweep
 * order and sorted); a failed reservation returns RSASA_ERR_OUT_OF_MEMORY and
 * the context stays usable.  Cost: the lists are ordered by one GPU lane per dot
 * with L * L comparisons for a list of L entries - nothing at the 8 entries of a
 * protein at the default link, but quadratic: a link that joins every dot of a
 * sphere of tens of thousands of points to every other (lists of that length)
 * keeps the device busy for seconds.
 *
 * link must be finite and >= 0, as for rsasa_surface_components; out_dot_offsets
 * or out_n_links NULL returns RSASA_ERR_INVALID_ARGUMENT, and so does a batch
 * with 2^31 - 1 or more dots.  The remaining argument errors and the non-finite
 * input rules are those of rsasa_surface_components.  No atoms: RSASA_OK with
 * out_dot_offsets[0] = 0, *out_n_links = 0 and (if given) out_link_offsets[0] = 0.
 *
 * Synchronous, in the neighbour calls' workspace on the context's first
 * stream: device batches in flight are neither waited for nor disturbed. */

/* One structure: n_atoms atoms, id nullable (all atoms distinct). */
int rsasa_dot_links(rsasa_context_t *ctx,
                    const float *x, const float *y, const float *z, const float *radius,
                    const uint64_t *id, size_t n_atoms,
                    float probe_radius, size_t n_points, float link,
                    uint64_t *out_dot_offsets, uint64_t *out_n_links,
                    uint64_t *out_link_offsets, size_t dots_capacity,
                    rsasa_within_t *out_entries, size_t entries_capacity,
                    uint32_t *out_free, float *out_sasa);

/* Directory-mode form, as rsasa_surface_components_batch: dots of different
 * structures are never linked; out_dot_offsets and out_link_offsets are
 * batch-global, idx is the dot number within the structure. */
int rsasa_dot_links_batch(rsasa_context_t *ctx,
                          const float *x, const float *y, const float *z, const float *radius,
                          const uint64_t *id,
                          const uint32_t *structure_offsets, size_t n_structures,
                          float probe_radius, size_t n_points, float link,
                          uint64_t *out_dot_offsets, uint64_t *out_n_links,
                          uint64_t *out_link_offsets, size_t dots_capacity,
                          rsasa_within_t *out_entries, size_t entries_capacity,
                          uint32_t *out_free, float *out_atom_sasa);

/* ---- dot geodesics ------------------------------------------------------ */

/* HOW FAR ALONG THE SURFACE a dot lies from a set of seed dots: the shortest
 * distance along the graph of rsasa_dot_links.  The dots within 12 A in space
 * of a centre include the far wall of a cleft; the dots within 12 A along the
 * surface do not (surface patches); seeded from the open dots of
 * rsasa_dot_enclosure it is the depth of a pocket.
 *
 * Definition.  The graph is that of rsasa_dot_links at the same link.  seeds is
 * one byte per accessible dot, in array order (the order of out_labels of
 * rsasa_surface_components), nonzero = seed.  All arithmetic is float32 and
 * unfused.
 *
 *   The edge weight is w(a, b) = sqrtf(d2), correctly rounded: the sqrt that
 *   rsasa_atom_depth already exposes bit for bit.
 *   The length of a path v0 ... vk is the left-to-right sum ((0 + w1) + w2) + ...
 *   dist[v] is the minimum over all paths from any seed to v whose length, and
 *   hence every prefix, is <= limit; +inf where there is none.  A seed has dist 0.
 *
 * Float addition of a non-negative number is monotone and never decreases its
 * left operand.  So dist is also the unique least solution of
 *
 *     dist[v] = min(seed ? 0 : inf, min_u fl(dist[u] + w(u, v)))
 *                                      with values > limit replaced by inf
 *
 * and any relaxation order, in place or double buffered, atomic or not,
 * converges to these bits: (1) every value a relaxation ever stores is the
 * length of a real path from a seed, so it is never below the least solution;
 * (2) when no edge can lower anything the values solve the equation, and a
 * solution reached from above through a monotone map is the least one.  The
 * result can therefore be checked for equality, whatever the schedule of the GPU.
 *
 * out_source (nullable) is uint32: source[v] is the smallest seed dot number,
 * within the structure, from which a path to v exists on which every vertex is
 * reached at exactly its dist - the trivial path included, so a seed that
 * coincides with a smaller seed has that one as its source.  It is 0xFFFFFFFF
 * where dist is +inf.  Equivalently it is the least fixed point of
 *
 *     source[v] = min(seed ? v : none,
 *                     min over u with fl(dist[u] + w(u, v)) == dist[v] of source[u])
 *
 * computed in a second phase over the converged dist (packed with dist into one
 * 64-bit minimum it would depend on the schedule: two distances can round to the
 * same sum).  Such a tight path exists for every finite dist.
 *
 *   out_dot_offsets  [n + 1], as rsasa_surface_components writes it; D is
 *                    out_dot_offsets[n];
 *   out_dist         [n_seed_bytes]: dist of the dot at each array position;
 *   out_source       [n_seed_bytes] or NULL;
 *   out_free[i]      (nullable) the popcount of rsasa_accessible_points;
 *   out_sasa[i]      (nullable) bit for bit rsasa_calculate_sasa_batch.
 *
 * Sizing: the caller needs D to pass the seeds - from any earlier dot call on
 * the same input (rsasa_surface_components, rsasa_dot_links, rsasa_dot_enclosure).
 * out_dot_offsets is always written; if n_seed_bytes != D nothing else is and
 * RSASA_ERR_INVALID_ARGUMENT is returned with a message (rsasa_context_last_error)
 * that names both numbers.
 *
 * limit must be >= 0; +inf is allowed and means no limit (-0.0 is 0); NaN or a
 * negative limit returns RSASA_ERR_INVALID_ARGUMENT.  link as for
 * rsasa_dot_links, and so the bound of 2^31 - 1 dots, the remaining argument
 * errors and the non-finite input rules: the dots of an atom with a NaN
 * coordinate or radius have no edges - as seeds they have dist 0, otherwise
 * +inf.  seeds or out_dist NULL with D > 0 returns RSASA_ERR_INVALID_ARGUMENT.
 * No atoms: RSASA_OK with out_dot_offsets[0] = 0 (n_seed_bytes must be 0).  The
 * lists stay on the device, 8 bytes per entry; a failed reservation returns
 * RSASA_ERR_OUT_OF_MEMORY and the context stays usable.  A relaxation that has
 * not settled after as many rounds as there are dots is a logic error and
 * returns RSASA_ERR_INTERNAL.
 *
 * Synchronous, in the neighbour calls' workspace on the context's first
 * stream: device batches in flight are neither waited for nor disturbed. */

/* One structure: n_atoms atoms, id nullable (all atoms distinct). */
int rsasa_dot_geodesics(rsasa_context_t *ctx,
                        const float *x, const float *y, const float *z, const float *radius,
                        const uint64_t *id, size_t n_atoms,
                        float probe_radius, size_t n_points, float link,
                        const uint8_t *seeds, size_t n_seed_bytes, float limit,
                        uint64_t *out_dot_offsets,
                        float *out_dist, uint32_t *out_source,
                        uint32_t *out_free, float *out_sasa);

/* Directory-mode form, as rsasa_dot_links_batch: no path crosses structures,
 * all structures relax in the same launches; seeds, out_dist and out_source run
 * over the dots of the whole batch, out_source holds dot numbers within the
 * structure. */
int rsasa_dot_geodesics_batch(rsasa_context_t *ctx,
                              const float *x, const float *y, const float *z, const float *radius,
                              const uint64_t *id,
                              const uint32_t *structure_offsets, size_t n_structures,
                              float probe_radius, size_t n_points, float link,
                              const uint8_t *seeds, size_t n_seed_bytes, float limit,
                              uint64_t *out_dot_offsets,
                              float *out_dist, uint32_t *out_source,
                              uint32_t *out_free, float *out_atom_sasa);

/* A measurement, not part of any result: out_rounds[0 .. 2) get the rounds of
 * relaxation that the context's last rsasa_dot_geodesics* call ran for dist and
 * for source, the last round - which changed nothing - included; 0 / 0 before
 * the first such call, after one that failed and for a phase that did not run.
 * The counts depend on the GPU's schedule by a round or two; the results do
 * not. */
int rsasa_context_geodesic_rounds(rsasa_context_t *ctx, uint32_t *out_rounds);

/* ---- dot patches -------------------------------------------------------- */

/* WHERE TO PUT THE PATCHES: a set of centre dots that covers the accessible
 * surface evenly ALONG the surface - surface fingerprints, patch descriptors,
 * coarse-grained interface maps, one representative per 6 A of pocket wall.
 * Geodesic farthest-point sampling: repeatedly the dot farthest from the
 * centres chosen so far becomes a centre, until no dot lies further than
 * `spacing` from its nearest centre.  One call replaces a host loop of one
 * rsasa_dot_geodesics_batch call per centre.
 *
 * Definition.  Graph, dots, numbering, weights and path length are those of
 * rsasa_dot_geodesics at the same link; there is no limit.  Each structure,
 * with D_s dots numbered within the structure, is sampled on its own:
 *
 *   dist_0[v] = +inf for every dot.
 *   Before pick k let m = max_v dist_k[v].  Sampling stops when
 *   k == min(max_centres, D_s), or D_s is 0, or m is finite and m <= spacing
 *   (float32 compare).  A dot at +inf is therefore always picked, and
 *   spacing = +inf gives exactly one centre per connected component.
 *   Otherwise c_k is the dot with dist_k == m, the smallest dot number among
 *   equals, and cover[k] = m (+inf for the first centre of a component).
 *   dist_{k+1} is the rsasa_dot_geodesics solution with seeds {c_0 .. c_k} and
 *   no limit.
 *
 * dist_{k+1} is computed from dist_k: with dist[c_k] = 0 every stored value is
 * still the length of a real path from a seed, and a relaxation from there
 * reaches the least solution for the larger seed set from above - the same bits
 * as a relaxation from scratch (rsasa_dot_geodesics: why any order converges).
 * So the results can be checked for equality, whatever the schedule of the GPU.
 *
 * Consequences: cover[k + 1] <= cover[k] as floats; the centres with cover ==
 * +inf are exactly the distinct rsasa_surface_components labels of the structure,
 * ascending, and they come first; unless max_centres cut the sampling short
 * every dist <= spacing, and only then can a dot stay at +inf; any two centres
 * are more than spacing apart along the graph; a dot without edges - every dot
 * of an atom with a NaN coordinate or radius among them - is its own centre.
 *
 *   out_dot_offsets     [n + 1], as rsasa_surface_components writes it; D is
 *                       out_dot_offsets[n].  Always written;
 *   *out_centre_bound   B = sum over the structures of min(max_centres, D_s): the
 *                       most centres the call can return.  Always written;
 *   out_centre_offsets  [S + 1] (S = n_structures; [0, K] for one structure):
 *                       structure s owns the centres [out_centre_offsets[s],
 *                       out_centre_offsets[s + 1]); 64-bit, batch-global;
 *   out_centres         [centres_capacity]: the centres in pick order, dot
 *                       numbers within the structure;
 *   out_cover           [centres_capacity]: cover of each centre;
 *   out_dist            [dots_capacity]: the final dist of the dot at each array
 *                       position;
 *   out_source          [dots_capacity] or NULL: exactly rsasa_dot_geodesics'
 *                       source for the seed set `centres` - the smallest centre
 *                       dot number with a tight path, 0xFFFFFFFF where dist is
 *                       +inf: the patch a dot belongs to;
 *   out_free[i]         (nullable) the popcount of rsasa_accessible_points;
 *   out_sasa[i]         (nullable) bit for bit rsasa_calculate_sasa_batch.
 *
 * Sizing, in two calls: if out_centre_offsets, out_centres, out_cover or
 * out_dist is NULL, dots_capacity < D or centres_capacity < B, nothing beyond
 * out_dot_offsets and *out_centre_bound is written, no sampling runs and
 * RSASA_ERR_BUFFER_TOO_SMALL is returned: call once to size, allocate, call
 * again.  A capacity of D always suffices for the centres.
 *
 * spacing must be finite and >= 0, or +inf (-0.0 is 0); NaN or a negative value
 * returns RSASA_ERR_INVALID_ARGUMENT, and so does max_centres == 0 or
 * out_dot_offsets or out_centre_bound NULL.  link, the bound of 2^31 - 1 dots,
 * the remaining argument errors and the non-finite input rules are those of
 * rsasa_dot_links.  No atoms: RSASA_OK with out_dot_offsets[0] = 0,
 * *out_centre_bound = 0 and (if given) out_centre_offsets all 0.
 *
 * Cost.  One GPU workgroup samples one structure, all its picks in one launch:
 * a pick reads the structure's D_s distances once (the argmax) and then relaxes
 * only where the new centre lowers something, a frontier step at a time.  The
 * structures of a batch run side by side; ONE large structure is sampled by one
 * workgroup alone and takes as long as its picks times its dots.
 * A sampler that leaves one of its bounded loops is a logic error and returns
 * RSASA_ERR_INTERNAL.
 *
 * Synchronous, in the neighbour calls' workspace on the context's first
 * stream: device batches in flight are neither waited for nor disturbed. */

/* One structure: n_atoms atoms, id nullable (all atoms distinct). */
int rsasa_dot_patches(rsasa_context_t *ctx,
                      const float *x, const float *y, const float *z, const float *radius,
                      const uint64_t *id, size_t n_atoms,
                      float probe_radius, size_t n_points, float link,
                      float spacing, uint32_t max_centres,
                      uint64_t *out_dot_offsets, uint64_t *out_centre_bound,
                      uint64_t *out_centre_offsets,
                      uint32_t *out_centres, float *out_cover, size_t centres_capacity,
                      float *out_dist, uint32_t *out_source, size_t dots_capacity,
                      uint32_t *out_free, float *out_sasa);

/* Directory-mode form, as rsasa_dot_geodesics_batch: every structure is sampled
 * on its own, all of them in the same launch; out_dist and out_source run over
 * the dots of the whole batch, out_centres and out_source hold dot numbers
 * within the structure. */
int rsasa_dot_patches_batch(rsasa_context_t *ctx,
                            const float *x, const float *y, const float *z, const float *radius,
                            const uint64_t *id,
                            const uint32_t *structure_offsets, size_t n_structures,
                            float probe_radius, size_t n_points, float link,
                            float spacing, uint32_t max_centres,
                            uint64_t *out_dot_offsets, uint64_t *out_centre_bound,
                            uint64_t *out_centre_offsets,
                            uint32_t *out_centres, float *out_cover, size_t centres_capacity,
                            float *out_dist, uint32_t *out_source, size_t dots_capacity,
                            uint32_t *out_free, float *out_atom_sasa);

/* A measurement, not part of any result: out_stats[0 .. 3) get, for the
 * context's last rsasa_dot_patches* call, the picks (the centres returned), the
 * relaxation steps summed over the structures - the step of each pick that
 * lowered nothing included - and the picks whose frontier outgrew the sampler's
 * queue and finished on the slower scan.  0 / 0 / 0 before the first such call
 * and after one that failed or only sized.  The steps and overflows depend on
 * the GPU's schedule; the results do not. */
int rsasa_context_patch_stats(rsasa_context_t *ctx, uint64_t *out_stats);

/* ---- the k nearest atoms ------------------------------------------------ */

/* WHO are the k nearest atoms of an atom, whatever their distance: the k-NN
 * graphs of structure networks (a fixed fan-in per node: k = 16, 30, 48, 64 on
 * CA traces or on all atoms).  A cutoff guessed for rsasa_atoms_within returns
 * every entry inside it and still leaves surface atoms, termini and ligands
 * short; here the reach follows the atom.
 *
 * Definition.  Flags, d2, eligibility and order are exactly those of
 * rsasa_atoms_within with upper_only == 0.  Let W_i be the list
 * rsasa_atoms_within defines for centre i at the same flags and cutoff.  Then
 *
 *     the list of atom i is the first min(k, |W_i|) entries of W_i.
 *
 * Entries are rsasa_within_t: d2 float32, unfused, idx the index within the
 * structure, ascending by the key (bits(d2) << 32) | idx.  When several
 * partners share the k-th d2, those with the smaller idx are kept: the result
 * is unique and can be compared byte for byte.  An atom without
 * RSASA_WITHIN_CENTRE has an empty list.  A NaN coordinate puts the atom in
 * nobody's list and gives it an empty one.  A structure with fewer than k
 * eligible partners gives shorter lists (all of them: n - 1 entries when every
 * atom is a partner and there is no cutoff).
 *
 * cutoff: +inf means no cutoff (c2 = +inf: every partner whose d2 is not NaN
 * is eligible), and a finite cutoff whose square overflows behaves the same;
 * -0.0 is 0; NaN or a negative cutoff returns RSASA_ERR_INVALID_ARGUMENT.
 * k: 1 <= k <= RSASA_NEAREST_MAX_K, anything else returns
 * RSASA_ERR_INVALID_ARGUMENT, and so do NULL columns, structure_offsets that
 * are not non-decreasing from 0, and out_offsets NULL.  radius, probe_radius
 * and id are treated as in rsasa_atoms_within: they only fix the cell size.
 * An infinite coordinate returns RSASA_ERR_GRID_TOO_LARGE and the context stays
 * usable.  No atoms: RSASA_OK with out_offsets[0] = 0.
 *
 * Sizing, as in rsasa_atoms_within: out_offsets is always written (on success
 * and on RSASA_ERR_BUFFER_TOO_SMALL).  If out_entries is NULL or
 * entries_capacity < out_offsets[n], nothing else is written and
 * RSASA_ERR_BUFFER_TOO_SMALL is returned; the context stays usable.  A
 * capacity of (number of centres) * k always suffices, so one call is enough.
 * On the device the call takes 16 bytes per centre and k; a failed reservation
 * returns RSASA_ERR_OUT_OF_MEMORY and the context stays usable.
 *
 * Synchronous, in the neighbour calls' workspace on the context's first
 * stream: device batches in flight are neither waited for nor disturbed.  One
 * sweep of the grid per centre, which ends by what it has found: no neighbour
 * lists are built and no cutoff is guessed. */
#define RSASA_NEAREST_MAX_K 256

/* One structure: n_atoms atoms, id nullable (it plays no part).  flags:
 * [n_atoms] or NULL; out_offsets: [n_atoms + 1]; out_entries:
 * [entries_capacity]. */
int rsasa_nearest_atoms(rsasa_context_t *ctx,
                        const float *x, const float *y, const float *z, const float *radius,
                        const uint64_t *id, size_t n_atoms,
                        float probe_radius,
                        const uint8_t *flags, uint32_t k, float cutoff,
                        uint64_t *out_offsets,
                        rsasa_within_t *out_entries, size_t entries_capacity);

/* Directory-mode form, as rsasa_atoms_within_batch: no list crosses
 * structures; out_offsets is batch-global; idx is the index within the
 * structure. */
int rsasa_nearest_atoms_batch(rsasa_context_t *ctx,
                              const float *x, const float *y, const float *z, const float *radius,
                              const uint64_t *id,
                              const uint32_t *structure_offsets, size_t n_structures,
                              float probe_radius,
                              const uint8_t *flags, uint32_t k, float cutoff,
                              uint64_t *out_offsets,
                              rsasa_within_t *out_entries, size_t entries_capacity);

/* ---- radial counts ------------------------------------------------------ */

/* HOW MANY atoms OF WHICH KIND AT WHICH DISTANCE an atom has around it: per
 * centre atom the number of partner atoms of its own structure by the
 * partner's class and by distance bin - contact numbers at several radii in one
 * pass (6 / 8 / 10 / 12 A), element-pair or residue-type environment
 * fingerprints (counts of C / N / O / S partners within 12 A), the local
 * density profile - and, per structure, the same counts summed by the centre's
 * class: the pair-distance histogram by class pair, the numerator of a radial
 * distribution function.  One sweep of the grid per centre, as far as the last
 * edge needs; what rsasa_half_sphere_exposure counts at one radius, split.
 *
 * Definition.  For a structure, each atom i has centre c_i, a flag byte f_i:
 * bit 0 (RSASA_RADIAL_PARTNER) - the atom is a partner, it is counted; bit 1
 * (RSASA_RADIAL_CENTRE) - the atom is a centre, it gets a row; the other bits
 * are ignored (the bits of RSASA_HSE_PARTNER / RSASA_HSE_CENTRE) - and a class
 * byte classes[i] < n_classes.  edges[0 .. n_bins) are the bins' outer radii.
 * All arithmetic is float32, unfused, left to right, exactly as in
 * rsasa_half_sphere_exposure:
 *
 *     e2[k] = edges[k] * edges[k]        (may overflow to +inf, underflow to 0)
 *     dx = c_j.x - c_i.x                 (dy, dz alike)
 *     d2 = dx * dx + dy * dy + dz * dz
 *     j counts for i  iff  j != i, j in the SAME structure, (f_j & 1), (f_i & 2),
 *                          d2 <= e2[n_bins - 1]
 *     bin(i, j) = the smallest k with d2 <= e2[k]
 *     out_counts[i][classes[j]][bin(i, j)] += 1
 *     out_pairs[s][a][b][k] = sum over the centres i of structure s with
 *                             classes[i] == a of out_counts[i][b][k]
 *
 * Bin k therefore holds the partners with e2[k - 1] < d2 <= e2[k] (bin 0: d2 <=
 * e2[0]).  An atom without bit 1 gets an all-zero row and adds nothing to
 * out_pairs.  flags == NULL: every atom is both a centre and a partner.
 * classes == NULL: every atom is class 0.  A NaN coordinate makes d2 NaN: a NaN
 * d2 counts nowhere, and that atom, as a centre, gets a zero row.  Of several
 * equal edges the first takes the pair and the others stay empty; with
 * edges[0] == 0, bin 0 holds exactly the coincident atoms.  e2[n_bins - 1] may
 * overflow to +inf: then every partner whose d2 is not NaN is counted.  Atom
 * ids play no part.  The counts are integers and have no order, so they can be
 * checked for equality.
 *
 * The cumulative identity.  For every k, the sum of out_counts[i][b][k'] over
 * every class b and every k' <= k equals out_up[i] + out_down[i] of
 * rsasa_half_sphere_exposure at the same flags and cutoff = edges[k]; the sum
 * over one class b alone equals that count when the partner bit is cleared on
 * the atoms of the other classes.
 *
 * Symmetry.  With flags == NULL, out_pairs[s][a][b][k] == out_pairs[s][b][a][k]:
 * d2 is the same bit pattern in both directions.  Otherwise the two are
 * separate entries (centres of class a around which partners of class b lie,
 * and the reverse).  A pair of two centres of one class is counted from both
 * ends: out_pairs[s][a][a][k] is twice the number of unordered pairs.
 *
 * radius and probe_radius are taken, and checked by the rules of the other
 * calls (probe_radius + largest radius a positive finite number), only because
 * they fix the cell size of the grid; the result does not depend on them.
 *
 * n_classes must lie in [1, RSASA_RADIAL_MAX_CLASSES] and n_bins in
 * [1, RSASA_RADIAL_MAX_BINS]; every edge must be finite and >= 0 (-0.0 is 0) and
 * the edges non-decreasing (equal edges are allowed); every class byte, on any
 * atom, centre or partner or neither, must be below n_classes - the host reads
 * them all before anything is launched.  Anything else returns
 * RSASA_ERR_INVALID_ARGUMENT, and so do NULL edges, NULL columns,
 * structure_offsets that are not non-decreasing from 0, and, where there are
 * atoms, out_counts and out_pairs both NULL (either one may be NULL: it is
 * then not written).  An infinite coordinate returns RSASA_ERR_GRID_TOO_LARGE and
 * the context stays usable.  No atoms: RSASA_OK, and out_pairs, when given, is
 * zeroed for the (empty) structures.
 *
 * Device memory.  The call holds the dense [N][n_classes][n_bins] uint32 table
 * on the device - 4 * n_classes * n_bins bytes per atom, 2 KiB at the bounds -
 * even when only out_pairs is asked for: the pair tables are summed from its
 * rows.  A failed reservation returns RSASA_ERR_OUT_OF_MEMORY and the context
 * stays usable.
 *
 * Synchronous, in the neighbour calls' workspace on the context's first
 * stream: device batches in flight are neither waited for nor disturbed.  No
 * neighbour lists are built; 4 * n_classes * n_bins bytes per atom come back,
 * or, with out_counts NULL, 8 * n_classes^2 * n_bins bytes per structure. */
#define RSASA_RADIAL_PARTNER 1
#define RSASA_RADIAL_CENTRE 2
#define RSASA_RADIAL_MAX_CLASSES 16
#define RSASA_RADIAL_MAX_BINS 32

/* One structure: n_atoms atoms, id nullable (it plays no part).  flags, classes:
 * [n_atoms] or NULL; edges: [n_bins]; out_counts: [n_atoms][n_classes][n_bins],
 * row-major, or NULL; out_pairs: [n_classes][n_classes][n_bins] or NULL. */
int rsasa_radial_counts(rsasa_context_t *ctx,
                        const float *x, const float *y, const float *z, const float *radius,
                        const uint64_t *id, size_t n_atoms,
                        float probe_radius,
                        const uint8_t *flags, const uint8_t *classes, uint32_t n_classes,
                        const float *edges, uint32_t n_bins,
                        uint32_t *out_counts, uint64_t *out_pairs);

/* Directory-mode form: n_structures independent structures concatenated as in
 * rsasa_calculate_sasa_batch (one grid each; an empty structure is legal, its
 * table is zero); atoms of other structures never count.  flags, classes and
 * out_counts run over structure_offsets[n_structures] atoms; out_pairs is
 * [n_structures][n_classes][n_classes][n_bins]. */
int rsasa_radial_counts_batch(rsasa_context_t *ctx,
                              const float *x, const float *y, const float *z, const float *radius,
                              const uint64_t *id,
                              const uint32_t *structure_offsets, size_t n_structures,
                              float probe_radius,
                              const uint8_t *flags, const uint8_t *classes, uint32_t n_classes,
                              const float *edges, uint32_t n_bins,
                              uint32_t *out_counts, uint64_t *out_pairs);

/* ---- contact counts ----------------------------------------------------- */

/* WHICH neighbour buries which part of an atom: per entry of each atom's
 * neighbour list, how many of the atom's sphere points it occludes - contact
 * surfaces between atoms, residues or chains, the atoms of a partner that bury
 * a residue, the area an atom regains when one neighbour goes.
 *
 * The lists are those of calculate_sasa_internal: out_offsets and out_entries
 * are byte for byte what rsasa_precompute_neighbors[_batch] returns with
 * max_radius = NaN (each list sorted by (d^2, idx); in the batch form idx is
 * the index within the structure).  For atom i, entry e of its list and
 * lattice point p, hit(e, p) is the test rsasa_accessible_points documents:
 * fmaf(sx, vx, fmaf(sy, vy, sz*vz)) < limit for p < n_fused, and
 * (sx*vx + sy*vy) + sz*vz <= limit after that, with
 * n_fused = n_points - n_points % W (W the context's lane count).
 *   out_covered[e]   = #{p : hit(e, p)}: the points e occludes, whatever the
 *                      other entries do;
 *   out_exclusive[e] = #{p : hit(e, p) and hit(e', p) for no other entry e'}:
 *                      the points only e occludes.
 * Both are uint32, aligned with out_entries, and do not depend on the list's
 * order; entries with out_covered == 0 are kept.  out_sasa[i] (nullable) is bit
 * for bit rsasa_calculate_sasa_batch: k = n_points - #{p : some hit} is n_points
 * minus the popcount of rsasa_accessible_points.  A count k is an area of
 * ((12.566371f * (R*R)) * (float)k) * (1.0f / (float)n_points) square
 * angstroms, R = radius + probe of the atom that owns the list (lib.rs:220-222);
 * out_exclusive[e] as an area is what atom i's SASA grows by when atom idx is
 * deleted from the structure, as long as the deletion leaves the structure's
 * largest radius unchanged.
 *
 * Sizing, as the neighbour calls: out_offsets is always written (on success
 * and on RSASA_ERR_BUFFER_TOO_SMALL).  If out_entries, out_covered or
 * out_exclusive is NULL, or entries_capacity < out_offsets[n], nothing else is
 * written and RSASA_ERR_BUFFER_TOO_SMALL is returned: call once to size,
 * allocate, call again.
 *
 * Everything else is as rsasa_accessible_points*: the argument errors; the
 * "Non-finite input" paragraph (a NaN coordinate: an empty list, nobody's
 * neighbour; a NaN radius: an empty list and a NaN threshold in the lists of
 * others, so counts of 0 there; an infinite coordinate:
 * RSASA_ERR_GRID_TOO_LARGE, the context stays usable); synchronous, in the
 * neighbour calls' workspace on the context's first stream, so device batches
 * in flight (rsasa_batch_enqueue) are neither waited for nor disturbed.  The
 * lists stay on the device between the neighbour search and the counts. */

/* One structure: n_atoms atoms, id nullable (all atoms distinct).
 * out_offsets: [n_atoms + 1]; out_entries, out_covered, out_exclusive:
 * [entries_capacity]; out_sasa: [n_atoms] or NULL. */
int rsasa_contact_points(rsasa_context_t *ctx,
                         const float *x, const float *y, const float *z, const float *radius,
                         const uint64_t *id, size_t n_atoms,
                         float probe_radius, size_t n_points,
                         uint64_t *out_offsets, rsasa_neighbor_t *out_entries,
                         uint32_t *out_covered, uint32_t *out_exclusive, size_t entries_capacity,
                         float *out_sasa);

/* Directory-mode form: n_structures independent structures concatenated as in
 * rsasa_calculate_sasa_batch (one grid and one max radius each); out_offsets
 * is batch-global [structure_offsets[n_structures] + 1]. */
int rsasa_contact_points_batch(rsasa_context_t *ctx,
                               const float *x, const float *y, const float *z, const float *radius,
                               const uint64_t *id,
                               const uint32_t *structure_offsets, size_t n_structures,
                               float probe_radius, size_t n_points,
                               uint64_t *out_offsets, rsasa_neighbor_t *out_entries,
                               uint32_t *out_covered, uint32_t *out_exclusive, size_t entries_capacity,
                               float *out_atom_sasa);

/* ---- contact owners ----------------------------------------------------- */

/* A PARTITION of an atom's buried points among its neighbours: every point
 * some entry of the list hits goes to exactly one entry, so the counts of an
 * atom's entries add up to what the atom lost - the atom x atom (and, summed,
 * residue x residue or chain x chain) table of buried area whose rows are
 * additive.  out_covered counts a point once for every entry that hits it and
 * out_exclusive drops every point two entries hit; out_owned lies between.
 *
 * Lists, hit(e, p), n_fused, out_sasa, sizing, argument errors, non-finite
 * input, stream and workspace are all as rsasa_contact_points*.  For atom i,
 * position e of its list (sorted by (d^2, idx)) and lattice point p, with
 * (sx, sy, sz) the point, (vx, vy, vz) = centre_i - centre_idx and
 * limit = (threshold_squared - d^2 - R*R) / (2*R) as the hit rule uses them,
 * the margin is
 *   m(e, p) = fmaf(sx, vx, fmaf(sy, vy, sz*vz)) - limit    for p < n_fused,
 *   m(e, p) = ((sx*vx + sy*vy) + sz*vz) - limit            for later points:
 * the same dot as the hit rule for that point, followed by one float32
 * subtraction, unfused.  In exact arithmetic 2*R*m is |P - c_idx|^2 -
 * threshold_squared with P = c_i + R*s: the power distance of the point to the
 * neighbour's expanded sphere, negative where the entry hits.
 *   owner(p) is found by walking the list in order: entry e takes the point if
 *   hit(e, p) and either nobody owns it yet or m(e, p) < m(owner, p).
 * Without NaN this is the hitting entry with the smallest (m, e): the buried
 * part of the sphere is cut by the radical planes of the neighbours (the power
 * diagram).  The earlier position wins an exact tie; -0 and +0 tie; a NaN limit
 * never hits and so never owns; a free point has owner 0xFFFFFFFF.
 *   out_owned[e] = #{p : owner(p) = e}, uint32, aligned with out_entries;
 *                  entries that own nothing are kept.
 * Hence, exactly, for every atom: the sum of out_owned over its entries is
 * n_points - popcount(rsasa_accessible_points);
 * out_exclusive[e] <= out_owned[e] <= out_covered[e]; and all three are equal
 * for a list of one entry.  Counts are areas by the expression given for
 * rsasa_contact_points.
 *
 * out_owner (nullable): uint32[n_atoms * n_points], row i in input order, the
 * owner position of every point of atom i; the neighbour is
 * out_entries[out_offsets[i] + owner].  It is the dot-level contact map:
 * together with rsasa_sphere_points it colours every buried dot by partner.
 * When it is NULL no device memory is reserved for it.  It is written only on
 * RSASA_OK.
 *
 * Sizing: if out_entries or out_owned is NULL, or entries_capacity <
 * out_offsets[n], out_offsets is written, nothing else, and
 * RSASA_ERR_BUFFER_TOO_SMALL is returned. */

/* One structure: n_atoms atoms, id nullable (all atoms distinct).
 * out_offsets: [n_atoms + 1]; out_entries, out_owned: [entries_capacity];
 * out_owner: [n_atoms * n_points] or NULL; out_sasa: [n_atoms] or NULL. */
int rsasa_contact_owners(rsasa_context_t *ctx,
                         const float *x, const float *y, const float *z, const float *radius,
                         const uint64_t *id, size_t n_atoms,
                         float probe_radius, size_t n_points,
                         uint64_t *out_offsets, rsasa_neighbor_t *out_entries,
                         uint32_t *out_owned, size_t entries_capacity,
                         uint32_t *out_owner, float *out_sasa);

/* Directory-mode form: n_structures independent structures concatenated as in
 * rsasa_calculate_sasa_batch (one grid and one max radius each); out_offsets
 * is batch-global [structure_offsets[n_structures] + 1], out_owner rows in
 * batch order. */
int rsasa_contact_owners_batch(rsasa_context_t *ctx,
                               const float *x, const float *y, const float *z, const float *radius,
                               const uint64_t *id,
                               const uint32_t *structure_offsets, size_t n_structures,
                               float probe_radius, size_t n_points,
                               uint64_t *out_offsets, rsasa_neighbor_t *out_entries,
                               uint32_t *out_owned, size_t entries_capacity,
                               uint32_t *out_owner, float *out_atom_sasa);

/* ---- group contacts ----------------------------------------------------- */

/* WHICH partner buries which part of an atom, above the level of single
 * atoms: every atom carries a uint32 group label (chain, residue, ligand,
 * anything), and per atom and partner group the call counts the points the
 * partner takes - buried surface on complex formation per atom, residue or
 * chain, the chain x chain or residue x residue interface matrix, what an atom
 * regains when a ligand or a chain is removed.  The area one group buries is a
 * UNION over its atoms: sums of rsasa_contact_points' per-entry counts over a
 * group count every point twice that two of its atoms hit.
 *
 * For atom i, L(i) is its list as rsasa_contact_points uses it (max_radius =
 * NaN), g(.) are the labels - compared within one structure only - and
 * hit(e, p) is the test rsasa_accessible_points documents (the fused rule for
 * p < n_fused, the remainder rule after it, W the context's lane count).
 *   self(p)          = some entry e of L(i) with g(idx_e) == g(i) has hit(e, p);
 *   out_self_free[i] = #{p : !self(p)}: the accessible points of atom i with
 *                      only its own group present (n_points if no entry shares
 *                      its label);
 *   out_free[i]      = #{p : no entry hits p}: the popcount of
 *                      rsasa_accessible_points;
 *   out_sasa[i]      (nullable) bit for bit rsasa_calculate_sasa_batch.
 * Atom i has one row per DISTINCT FOREIGN label h among the entries of L(i), in
 * ascending unsigned order of h, in CSR form: its rows are
 * [out_offsets[i], out_offsets[i + 1]), out_groups[row] = h.  With
 * cov_h(p) = some entry labelled h has hit(e, p):
 *   out_buried[row]  = #{p : cov_h(p) && !self(p)}: what group h alone takes
 *                      from atom i of the isolated group g(i) - the pairwise
 *                      interface, A+B against A;
 *   out_only[row]    = #{p : cov_h(p) && !self(p) && cov_h'(p) for no other
 *                      foreign h'}: what atom i regains in the whole structure
 *                      when group h is deleted.
 * Rows whose counts are 0 are kept (a neighbour with a NaN radius, a candidate
 * that hits nothing).  Nothing depends on the list's order.  Counts are areas
 * by the expression given for rsasa_contact_points, R that of atom i.  As
 * there, the statements about isolated groups and deletions are exact as long
 * as the smaller structure has the whole structure's largest radius (the
 * candidate rule depends on it).
 *
 * Sizing, as the neighbour and contact calls: out_offsets is always written (on
 * success and on RSASA_ERR_BUFFER_TOO_SMALL).  If out_groups, out_buried or
 * out_only is NULL, or rows_capacity < out_offsets[n], nothing else is written
 * and RSASA_ERR_BUFFER_TOO_SMALL is returned: call once to size, allocate,
 * call again.  group, out_self_free and out_free are required where there are
 * atoms: NULL returns RSASA_ERR_INVALID_ARGUMENT.
 *
 * Everything else is as rsasa_contact_points*: the argument errors; non-finite
 * input (a NaN coordinate: no rows, n_points everywhere; a NaN radius: the
 * same, and rows of 0 in the lists of others; an infinite coordinate:
 * RSASA_ERR_GRID_TOO_LARGE, the context stays usable); synchronous, in the
 * neighbour calls' workspace on the context's first stream, so device batches
 * in flight are neither waited for nor disturbed.  The lists stay on the
 * device; only the labels go up and the rows and per-atom counts come down. */

/* One structure: n_atoms atoms, id nullable (all atoms distinct).
 * group: [n_atoms]; out_offsets: [n_atoms + 1]; out_groups, out_buried,
 * out_only: [rows_capacity]; out_self_free, out_free: [n_atoms]; out_sasa:
 * [n_atoms] or NULL. */
int rsasa_group_contacts(rsasa_context_t *ctx,
                         const float *x, const float *y, const float *z, const float *radius,
                         const uint64_t *id, const uint32_t *group, size_t n_atoms,
                         float probe_radius, size_t n_points,
                         uint64_t *out_offsets, uint32_t *out_groups,
                         uint32_t *out_buried, uint32_t *out_only, size_t rows_capacity,
                         uint32_t *out_self_free, uint32_t *out_free, float *out_sasa);

/* Directory-mode form: n_structures independent structures concatenated as in
 * rsasa_calculate_sasa_batch (one grid and one max radius each); out_offsets
 * is batch-global [structure_offsets[n_structures] + 1].  Labels never match
 * across structures: lists never cross them. */
int rsasa_group_contacts_batch(rsasa_context_t *ctx,
                               const float *x, const float *y, const float *z, const float *radius,
                               const uint64_t *id, const uint32_t *group,
                               const uint32_t *structure_offsets, size_t n_structures,
                               float probe_radius, size_t n_points,
                               uint64_t *out_offsets, uint32_t *out_groups,
                               uint32_t *out_buried, uint32_t *out_only, size_t rows_capacity,
                               uint32_t *out_self_free, uint32_t *out_free, float *out_atom_sasa);

/* ---- measurement ------------------------------------------------------- */

/* When enabled, every rsasa_batch_enqueue brackets its kernels with HIP
 * events on the launch stream; the elapsed times of the most recent
 * completed batch are returned by rsasa_context_get_timings. */
typedef struct rsasa_timings {
    float grid_build_ms;   /* bounds + binning + scan + scatter kernels */
    float occlusion_ms;    /* the occlusion kernels alone (fast kernel + general kernel over deferred atoms) */
    float aggregate_ms;    /* residue sums */
    float total_ms;        /* first kernel start -> last kernel end */
    uint64_t n_cells;      /* total grid cells of the batch */
    uint64_t n_atoms;
    uint64_t n_deferred;   /* atoms the fast occlusion kernel left to the general one */
} rsasa_timings_t;

int rsasa_context_enable_timing(rsasa_context_t *ctx, int enable);
int rsasa_context_get_timings(rsasa_context_t *ctx, rsasa_timings_t *out);

/* Ids only matter where two atoms of one structure share one (a neighbour with
 * the atom's own id is skipped: reference src/lib.rs:127).  Large batches are
 * checked, and when the ids of every structure are all different the batch,
 * or the sub-batch of a pipelined host call, runs as one WITHOUT ids: the
 * same values, no id traffic, the id-less kernels (4 % faster).  Ids that
 * increase strictly within every structure (atom serials, indices) are found
 * by one comparison per atom, on the device or by the host's coding threads;
 * 64-bit ids in no order (hashes) that are on the device go through a hash
 * table per structure (up to 55 296 atoms per structure); ids the host has
 * folded to 32 bits (a pipelined host call's pinned ids) through the same
 * tables on their folds.  The verdict is each STRUCTURE's: one with two equal
 * ids (a file whose serial numbers repeat), or one nobody could check, keeps
 * its ids and runs in the kernels' instantiation with ids, the others of the
 * same batch without (ABI 4; a single such structure used to put the whole
 * batch on the slower path).  rsasa_context_ids_dropped counts the
 * (sub-)batches of the context, its stream of host batches included, in which
 * NO structure kept its ids; rsasa_context_ids_kept gives the number of
 * structures that kept theirs in the context's last checked (sub-)batch. */
int rsasa_context_ids_dropped(rsasa_context_t *ctx, uint64_t *out_batches);
int rsasa_context_ids_kept(rsasa_context_t *ctx, uint64_t *out_structures);

/* ---- utilities --------------------------------------------------------- */

/* The golden-section-spiral lattice the engine uploads to the GPU
 * (reference src/lib.rs:43-66), computed on the host with libm. */
int rsasa_sphere_points(size_t n_points, float *out_x, float *out_y, float *out_z);

#ifdef __cplusplus
}
#endif
#endif /* RUSTSASA_AMD_H */
