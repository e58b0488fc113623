// Host side of the neighbour-list entry points (rsasa_precompute_neighbors / _batch, include/rustsasa_amd.h): the
// batch's grid is built by the SASA path's kernels in a workspace of the context's own (rsasa_context::nb_ws), then
// neighbors.hip counts, scans and fills the lists.  The accessible-point entry points (rsasa_accessible_points /
// _batch) run the same stages and hand the lists, still on the device, to points.hip; so do the exposure vectors
// (rsasa_exposure_vectors*), the contact counts (rsasa_contact_points*) and the group contacts (rsasa_group_contacts*);
// the atom depths (rsasa_atom_depth*) run the point masks and hand them and the grid to depth.hip, the surface
// components (rsasa_surface_components*) hand the same to components.hip.
// rsasa_sas_volume is plain host arithmetic on what the exposure vectors return.  Host code only.
#include "engine_internal.h"

#include <cmath>
#include <cstring>

namespace {

using namespace rsasa;

struct NbHost {  // the pinned block the device's verdicts come back in
    BatchStatus status;
    NbInfo info;
    uint64_t last_offset;  // offsets[N], when the caller wants no host copy of the offsets
};

// The upload, the grid and the counts of a run over columns already in host memory: S structures, N >= 1 atoms.
// idx_map (host, nullable): input atom -> the index written to the entries.  out_offsets (nullable): [N + 1], the
// offsets are copied there.  On RSASA_OK `a` describes the device lists (everything but their entries) and `info` their
// sizes.  The caller holds the context's mutex and has made its device current.
int nb_count(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id,
             const uint32_t *so, size_t S, size_t N, const uint32_t *idx_map, float probe, float max_r,
             uint64_t *out_offsets, NbArgs &a, NbInfo &info)
{
    int rc;
    rsasa_context::Workspace &W = ctx->nb_ws;
    hipStream_t st = ctx->stream;

    const SegmentCount sc = count_segments(so, S);
    std::vector<Segment> segs(sc.n_seg);
    write_segments(so, S, segs.data(), nullptr);
    const bool has_tail = sc.has_tail;
    const bool has_id = id != nullptr;
    if (!ctx->nb_host.p) RS_HIP(ctx, ctx->nb_host.regrow(sizeof(NbHost)));
    NbHost *h = static_cast<NbHost *>(ctx->nb_host.p);

    if ((rc = reserve(ctx, ctx->nb_x, N * 4)) || (rc = reserve(ctx, ctx->nb_y, N * 4)) || (rc = reserve(ctx, ctx->nb_z, N * 4)) ||
        (rc = reserve(ctx, ctx->nb_r, N * 4)) || (has_id && (rc = reserve(ctx, ctx->nb_id, N * 8))) ||
        (idx_map && (rc = reserve(ctx, ctx->nb_map, N * 4))))
        return rc;
    RS_HIP(ctx, hipMemcpyAsync(ctx->nb_x.p, x, N * 4, hipMemcpyHostToDevice, st));
    RS_HIP(ctx, hipMemcpyAsync(ctx->nb_y.p, y, N * 4, hipMemcpyHostToDevice, st));
    RS_HIP(ctx, hipMemcpyAsync(ctx->nb_z.p, z, N * 4, hipMemcpyHostToDevice, st));
    RS_HIP(ctx, hipMemcpyAsync(ctx->nb_r.p, r, N * 4, hipMemcpyHostToDevice, st));
    if (has_id) RS_HIP(ctx, hipMemcpyAsync(ctx->nb_id.p, id, N * 8, hipMemcpyHostToDevice, st));
    if (idx_map) RS_HIP(ctx, hipMemcpyAsync(ctx->nb_map.p, idx_map, N * 4, hipMemcpyHostToDevice, st));

    // ---- the grid (without the id check: every id takes part), grown until the cells fit
    BatchView v{};
    for (int attempt = 0;; attempt++) {
        if ((rc = W.reserve_grid(ctx, N, S, segs.size(), ctx->nb_cell_capacity, has_tail, has_id))) return rc;
        if (!segs.empty())
            RS_HIP(ctx, hipMemcpyAsync(W.segments.p, segs.data(), segs.size() * sizeof(Segment), hipMemcpyHostToDevice, st));
        v = BatchView{};
        v.x = (const float *)ctx->nb_x.p; v.y = (const float *)ctx->nb_y.p; v.z = (const float *)ctx->nb_z.p;
        v.radius = (const float *)ctx->nb_r.p;
        v.id = has_id ? (const uint64_t *)ctx->nb_id.p : nullptr;
        v.n_atoms = (uint32_t)N; v.n_structures = (uint32_t)S; v.n_segments = (uint32_t)segs.size();
        v.probe = probe;
        v.max_r_override = max_r;
        W.grid_view(v);
        launch_grid_prepare(v, st);
        launch_sort_lds(v, st);
        if (has_tail) launch_sort_tail(v, st);
        RS_HIP(ctx, hipMemcpyAsync(&h->status, W.status.p, sizeof(BatchStatus), hipMemcpyDeviceToHost, st));
        RS_HIP(ctx, hipGetLastError());
        RS_HIP(ctx, hipStreamSynchronize(st));
        if ((rc = grid_verdict(ctx, h->status, attempt, ctx->nb_cell_capacity)) == RSASA_OK) break;
        if (rc != kGridAgain) return rc;
    }

    // ---- counts, offsets
    a = NbArgs{};
    a.b = v;
    if ((rc = reserve(ctx, ctx->nb_counts, N * 4)) || (rc = reserve(ctx, ctx->nb_offsets, (N + 1) * 8)) ||
        (rc = reserve(ctx, ctx->nb_parts, 4 * 1024 * 8)) || (rc = reserve(ctx, ctx->nb_info, sizeof(NbInfo))))
        return rc;
    a.counts = (uint32_t *)ctx->nb_counts.p;
    a.offsets = (unsigned long long *)ctx->nb_offsets.p;
    a.parts = (unsigned long long *)ctx->nb_parts.p;
    a.info = (NbInfo *)ctx->nb_info.p;
    a.idx_map = idx_map ? (const uint32_t *)ctx->nb_map.p : nullptr;
    RS_HIP(ctx, hipMemsetAsync(a.info, 0, sizeof(NbInfo), st));
    launch_neighbor_count(a, st);
    RS_HIP(ctx, hipMemcpyAsync(&h->info, a.info, sizeof(NbInfo), hipMemcpyDeviceToHost, st));
    if (out_offsets) RS_HIP(ctx, hipMemcpyAsync(out_offsets, a.offsets, (N + 1) * 8, hipMemcpyDeviceToHost, st));
    else RS_HIP(ctx, hipMemcpyAsync(&h->last_offset, a.offsets + N, 8, hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, hipStreamSynchronize(st));
    info = h->info;
    if (info.total != (out_offsets ? out_offsets[N] : h->last_offset))
        return fail(ctx, RSASA_ERR_INTERNAL, "neighbour offsets disagree with their total");
    return RSASA_OK;
}

// The entries of the lists nb_count sized (info.total >= 1), sorted, in a.out on the device.
int nb_fill(rsasa_context *ctx, NbArgs &a, const NbInfo &info)
{
    int rc;
    hipStream_t st = ctx->stream;
    NbHost *h = static_cast<NbHost *>(ctx->nb_host.p);
    if ((rc = reserve(ctx, ctx->nb_entries, info.total * 8)) ||
        (info.spill_atoms && ((rc = reserve(ctx, ctx->nb_spill, info.spill_entries * sizeof(NbKey))) ||
                              (rc = reserve(ctx, ctx->nb_recs, info.spill_atoms * sizeof(NbSpillRec))))))
        return rc;
    a.out = (uint2 *)ctx->nb_entries.p;
    a.spill = info.spill_atoms ? (NbKey *)ctx->nb_spill.p : nullptr;
    a.spill_recs = info.spill_atoms ? (NbSpillRec *)ctx->nb_recs.p : nullptr;
    launch_neighbor_fill(a, info.spill_atoms, st);
    RS_HIP(ctx, hipMemcpyAsync(&h->info, a.info, sizeof(NbInfo), hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, hipStreamSynchronize(st));
    if (h->info.mismatch || h->info.spill_cursor != info.spill_entries || h->info.spill_recs != info.spill_atoms)
        return fail(ctx, RSASA_ERR_INTERNAL, "the neighbour fill pass disagrees with its count pass");
    return RSASA_OK;
}

// One neighbour-list run: S structures, N atoms (see nb_count).
int nb_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id,
           const uint32_t *so, size_t S, size_t N, const uint32_t *idx_map, float probe, float max_r,
           uint64_t *out_offsets, rsasa_neighbor_t *out_entries, size_t cap)
{
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    int rc;
    if (N == 0) {
        out_offsets[0] = 0;
        return RSASA_OK;
    }
    NbArgs a{};
    NbInfo info{};
    if ((rc = nb_count(ctx, x, y, z, r, id, so, S, N, idx_map, probe, max_r, out_offsets, a, info))) return rc;
    if (!out_entries || cap < info.total)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "out_entries holds fewer entries than out_offsets[n]");
    if (info.total == 0) return RSASA_OK;
    if ((rc = nb_fill(ctx, a, info))) return rc;
    RS_HIP(ctx, hipMemcpyAsync(out_entries, a.out, info.total * 8, hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RSASA_OK;
}

// ---- accessible points (rsasa_accessible_points*) ----

// The lattice in the reference's order (lib.rs:43-66) on the device: x | y | z, each zero padded to whole 64s.
int pt_lattice(rsasa_context *ctx, size_t n_points, size_t &padded)
{
    padded = (n_points + 63) / 64 * 64;
    if (ctx->pt_lattice_points == n_points) return RSASA_OK;
    int rc;
    ctx->pt_lattice_points = 0;
    if ((rc = reserve(ctx, ctx->pt_lattice, 3 * padded * sizeof(float)))) return rc;
    std::vector<float> h(3 * padded, 0.0f);
    generate_sphere_points(n_points, h.data(), h.data() + padded, h.data() + 2 * padded);
    RS_HIP(ctx, hipMemcpyAsync(ctx->pt_lattice.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->pt_lattice_points = n_points;
    return RSASA_OK;
}

// One run of the point tests: the lists of nb_count / nb_fill with max_r = NaN - the lists calculate_sasa_internal
// builds (lib.rs:259-267) - stay on the device and k_accessible_points turns them into masks.
int pt_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id,
           const uint32_t *so, size_t S, size_t N, float probe, size_t n_points, uint32_t *out_masks, float *out_sasa)
{
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    int rc;
    if (N == 0) return RSASA_OK;
    const size_t words = (n_points + 31) / 32;
    size_t padded = 0;
    if ((rc = pt_lattice(ctx, n_points, padded))) return rc;
    NbArgs a{};
    NbInfo info{};
    if ((rc = nb_count(ctx, x, y, z, r, id, so, S, N, nullptr, probe, __builtin_nanf(""), nullptr, a, info))) return rc;
    if (info.total && (rc = nb_fill(ctx, a, info))) return rc;
    if ((rc = reserve(ctx, ctx->pt_masks, N * words * 4)) || (out_sasa && (rc = reserve(ctx, ctx->pt_sasa, N * 4)))) return rc;
    PtArgs pa{};
    pa.b = a.b;
    pa.offsets = a.offsets;
    pa.entries = (const uint2 *)ctx->nb_entries.p;  // (not read when every list is empty)
    const float *lat = (const float *)ctx->pt_lattice.p;
    pa.lx = lat; pa.ly = lat + padded; pa.lz = lat + 2 * padded;
    pa.n_points = (uint32_t)n_points;
    pa.n_fused = (uint32_t)(n_points - n_points % (size_t)ctx->simd_width);
    pa.words = (uint32_t)words;
    pa.masks = (uint32_t *)ctx->pt_masks.p;
    pa.sasa = out_sasa ? (float *)ctx->pt_sasa.p : nullptr;
    hipStream_t st = ctx->stream;
    launch_accessible_points(pa, st);
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, hipMemcpyAsync(out_masks, pa.masks, N * words * 4, hipMemcpyDeviceToHost, st));
    if (out_sasa) RS_HIP(ctx, hipMemcpyAsync(out_sasa, pa.sasa, N * 4, hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    return RSASA_OK;
}

// ---- exposure vectors (rsasa_exposure_vectors*) ----

// One run of the exposure vectors: the lists of pt_run stay on the device and k_exposure_vectors turns them into the sum
// of each atom's exposed lattice points and their number; 16 bytes per atom come back (and 4 for the value, if asked).
int ex_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id,
           const uint32_t *so, size_t S, size_t N, float probe, size_t n_points, float *out_vectors, uint32_t *out_free,
           float *out_sasa)
{
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    int rc;
    if (N == 0) return RSASA_OK;
    size_t padded = 0;
    if ((rc = pt_lattice(ctx, n_points, padded))) return rc;
    NbArgs a{};
    NbInfo info{};
    if ((rc = nb_count(ctx, x, y, z, r, id, so, S, N, nullptr, probe, __builtin_nanf(""), nullptr, a, info))) return rc;
    if (info.total && (rc = nb_fill(ctx, a, info))) return rc;
    if ((rc = reserve(ctx, ctx->ex_vectors, N * 12)) || (rc = reserve(ctx, ctx->ex_free, N * 4)) ||
        (out_sasa && (rc = reserve(ctx, ctx->pt_sasa, N * 4))))
        return rc;
    ExArgs e{};
    e.p.b = a.b;
    e.p.offsets = a.offsets;
    e.p.entries = (const uint2 *)ctx->nb_entries.p;  // (not read when every list is empty)
    const float *lat = (const float *)ctx->pt_lattice.p;
    e.p.lx = lat; e.p.ly = lat + padded; e.p.lz = lat + 2 * padded;
    e.p.n_points = (uint32_t)n_points;
    e.p.n_fused = (uint32_t)(n_points - n_points % (size_t)ctx->simd_width);
    e.p.sasa = out_sasa ? (float *)ctx->pt_sasa.p : nullptr;
    e.vectors = (float *)ctx->ex_vectors.p;
    e.free = (uint32_t *)ctx->ex_free.p;
    hipStream_t st = ctx->stream;
    launch_exposure_vectors(e, st);
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, hipMemcpyAsync(out_vectors, e.vectors, N * 12, hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipMemcpyAsync(out_free, e.free, N * 4, hipMemcpyDeviceToHost, st));
    if (out_sasa) RS_HIP(ctx, hipMemcpyAsync(out_sasa, e.p.sasa, N * 4, hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    return RSASA_OK;
}

// ---- atom depth (rsasa_atom_depth*) ----

// One run of the atom depths: pt_run's stages up to the masks, which stay on the device (pt_masks); k_depth_free counts
// them and k_atom_depth searches the grid for every atom's nearest accessible dot.  8 bytes per atom come back (and 4
// each for the counts and the values, if asked); the square root of the key's d2 is taken here (sqrtf: correctly rounded).
int dp_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id,
           const uint32_t *so, size_t S, size_t N, float probe, size_t n_points, float *out_depth, uint32_t *out_nearest,
           uint32_t *out_free, float *out_sasa)
{
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    int rc;
    if (N == 0) return RSASA_OK;
    const size_t words = (n_points + 31) / 32;
    size_t padded = 0;
    if ((rc = pt_lattice(ctx, n_points, padded))) return rc;
    NbArgs a{};
    NbInfo info{};
    if ((rc = nb_count(ctx, x, y, z, r, id, so, S, N, nullptr, probe, __builtin_nanf(""), nullptr, a, info))) return rc;
    if (info.total && (rc = nb_fill(ctx, a, info))) return rc;
    if ((rc = reserve(ctx, ctx->pt_masks, N * words * 4)) || (rc = reserve(ctx, ctx->dp_keys, N * 8)) ||
        (rc = reserve(ctx, ctx->dp_free, N * 4)) || (out_sasa && (rc = reserve(ctx, ctx->pt_sasa, N * 4))))
        return rc;
    DpArgs d{};
    d.p.b = a.b;
    d.p.offsets = a.offsets;
    d.p.entries = (const uint2 *)ctx->nb_entries.p;  // (not read when every list is empty)
    const float *lat = (const float *)ctx->pt_lattice.p;
    d.p.lx = lat; d.p.ly = lat + padded; d.p.lz = lat + 2 * padded;
    d.p.n_points = (uint32_t)n_points;
    d.p.n_fused = (uint32_t)(n_points - n_points % (size_t)ctx->simd_width);
    d.p.words = (uint32_t)words;
    d.p.masks = (uint32_t *)ctx->pt_masks.p;
    d.p.sasa = out_sasa ? (float *)ctx->pt_sasa.p : nullptr;
    d.free = (uint32_t *)ctx->dp_free.p;
    d.keys = (unsigned long long *)ctx->dp_keys.p;
    hipStream_t st = ctx->stream;
    launch_accessible_points(d.p, st);
    launch_atom_depth(d, st);
    RS_HIP(ctx, hipGetLastError());
    std::vector<uint64_t> keys(N);
    RS_HIP(ctx, hipMemcpyAsync(keys.data(), d.keys, N * 8, hipMemcpyDeviceToHost, st));
    if (out_free) RS_HIP(ctx, hipMemcpyAsync(out_free, d.free, N * 4, hipMemcpyDeviceToHost, st));
    if (out_sasa) RS_HIP(ctx, hipMemcpyAsync(out_sasa, d.p.sasa, N * 4, hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    for (size_t i = 0; i < N; i++) {
        const uint64_t k = keys[i];
        const uint32_t hi = (uint32_t)(k >> 32);
        float d2;
        std::memcpy(&d2, &hi, 4);
        out_depth[i] = k == ~0ull ? __builtin_inff() : sqrtf(d2);
        out_nearest[i] = (uint32_t)k;
    }
    return RSASA_OK;
}

// ---- surface components (rsasa_surface_components*) ----

// One run of the surface components: dp_run's stages up to the masks, which stay on the device (pt_masks);
// k_component_free counts them, the scan of the neighbour counts turns the counts into out_offsets, the caller's label
// buffer is checked against out_offsets[N] as nb_run checks its entries, and the union-find kernels label the dots.
// 8 bytes per atom and 4 per dot come back (and 4 per atom each for the counts and the values, if asked).
int cc_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id,
           const uint32_t *so, size_t S, size_t N, float probe, size_t n_points, float link, uint64_t *out_offsets,
           uint32_t *out_labels, size_t cap, uint32_t *out_free, float *out_sasa)
{
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    int rc;
    if (N == 0) {
        out_offsets[0] = 0;
        return RSASA_OK;
    }
    const size_t words = (n_points + 31) / 32;
    size_t padded = 0;
    if ((rc = pt_lattice(ctx, n_points, padded))) return rc;
    NbArgs a{};
    NbInfo info{};
    if ((rc = nb_count(ctx, x, y, z, r, id, so, S, N, nullptr, probe, __builtin_nanf(""), nullptr, a, info))) return rc;
    if (info.total && (rc = nb_fill(ctx, a, info))) return rc;
    if ((rc = reserve(ctx, ctx->pt_masks, N * words * 4)) || (rc = reserve(ctx, ctx->dp_free, N * 4)) ||
        (rc = reserve(ctx, ctx->cc_offsets, (N + 1) * 8)) || (out_sasa && (rc = reserve(ctx, ctx->pt_sasa, N * 4))))
        return rc;
    CcArgs c{};
    c.p.b = a.b;
    c.p.offsets = a.offsets;
    c.p.entries = (const uint2 *)ctx->nb_entries.p;  // (not read when every list is empty)
    const float *lat = (const float *)ctx->pt_lattice.p;
    c.p.lx = lat; c.p.ly = lat + padded; c.p.lz = lat + 2 * padded;
    c.p.n_points = (uint32_t)n_points;
    c.p.n_fused = (uint32_t)(n_points - n_points % (size_t)ctx->simd_width);
    c.p.words = (uint32_t)words;
    c.p.masks = (uint32_t *)ctx->pt_masks.p;
    c.p.sasa = out_sasa ? (float *)ctx->pt_sasa.p : nullptr;
    c.free = (uint32_t *)ctx->dp_free.p;
    c.dot_offsets = (const unsigned long long *)ctx->cc_offsets.p;
    c.link = link;
    c.link2 = link * link;
    hipStream_t st = ctx->stream;
    launch_accessible_points(c.p, st);
    launch_component_free(c, st);
    NbArgs scan = a;  // (the neighbour run has read its parts and its info)
    scan.counts = c.free;
    scan.offsets = (unsigned long long *)ctx->cc_offsets.p;
    launch_neighbor_scan(scan, st);
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, hipMemcpyAsync(out_offsets, c.dot_offsets, (N + 1) * 8, hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    const uint64_t n_dots = out_offsets[N];
    if (n_dots >= 0x100000000ull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "2^32 or more accessible dots");
    if (!out_labels || cap < n_dots)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "out_labels is NULL or holds fewer labels than out_dot_offsets[n]");
    if (n_dots) {
        if ((rc = reserve(ctx, ctx->cc_parent, n_dots * 4)) || (rc = reserve(ctx, ctx->cc_labels, n_dots * 4))) return rc;
        c.n_dots = n_dots;
        c.parent = (uint32_t *)ctx->cc_parent.p;
        c.labels = (uint32_t *)ctx->cc_labels.p;
        launch_components(c, st);
        RS_HIP(ctx, hipGetLastError());
        RS_HIP(ctx, hipMemcpyAsync(out_labels, c.labels, n_dots * 4, hipMemcpyDeviceToHost, st));
    }
    if (out_free) RS_HIP(ctx, hipMemcpyAsync(out_free, c.free, N * 4, hipMemcpyDeviceToHost, st));
    if (out_sasa) RS_HIP(ctx, hipMemcpyAsync(out_sasa, c.p.sasa, N * 4, hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    return RSASA_OK;
}

// ---- contact counts (rsasa_contact_points*) ----

// One run of the contact counts: the lists of pt_run, sized and copied out as by nb_run, and k_contact_points' counts
// of every entry beside them.
int ct_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id,
           const uint32_t *so, size_t S, size_t N, float probe, size_t n_points, uint64_t *out_offsets,
           rsasa_neighbor_t *out_entries, uint32_t *out_covered, uint32_t *out_exclusive, size_t cap, float *out_sasa)
{
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    int rc;
    if (N == 0) {
        out_offsets[0] = 0;
        return RSASA_OK;
    }
    NbArgs a{};
    NbInfo info{};
    if ((rc = nb_count(ctx, x, y, z, r, id, so, S, N, nullptr, probe, __builtin_nanf(""), out_offsets, a, info))) return rc;
    if (!out_entries || !out_covered || !out_exclusive || cap < info.total)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "an entry buffer is NULL or holds fewer entries than out_offsets[n]");
    if (info.total && ((rc = nb_fill(ctx, a, info)) || (rc = reserve(ctx, ctx->ct_covered, info.total * 4)) ||
                       (rc = reserve(ctx, ctx->ct_exclusive, info.total * 4))))
        return rc;
    size_t padded = 0;
    if ((rc = pt_lattice(ctx, n_points, padded)) || (out_sasa && (rc = reserve(ctx, ctx->pt_sasa, N * 4)))) return rc;
    CtArgs c{};
    c.p.b = a.b;
    c.p.offsets = a.offsets;
    c.p.entries = (const uint2 *)ctx->nb_entries.p;  // (none of these three is read when every list is empty)
    c.covered = (uint32_t *)ctx->ct_covered.p;
    c.exclusive = (uint32_t *)ctx->ct_exclusive.p;
    const float *lat = (const float *)ctx->pt_lattice.p;
    c.p.lx = lat; c.p.ly = lat + padded; c.p.lz = lat + 2 * padded;
    c.p.n_points = (uint32_t)n_points;
    c.p.n_fused = (uint32_t)(n_points - n_points % (size_t)ctx->simd_width);
    c.p.sasa = out_sasa ? (float *)ctx->pt_sasa.p : nullptr;
    hipStream_t st = ctx->stream;
    launch_contact_points(c, st);
    RS_HIP(ctx, hipGetLastError());
    if (info.total) {
        RS_HIP(ctx, hipMemcpyAsync(out_entries, c.p.entries, info.total * 8, hipMemcpyDeviceToHost, st));
        RS_HIP(ctx, hipMemcpyAsync(out_covered, c.covered, info.total * 4, hipMemcpyDeviceToHost, st));
        RS_HIP(ctx, hipMemcpyAsync(out_exclusive, c.exclusive, info.total * 4, hipMemcpyDeviceToHost, st));
    }
    if (out_sasa) RS_HIP(ctx, hipMemcpyAsync(out_sasa, c.p.sasa, N * 4, hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    return RSASA_OK;
}

// The argument checks of rsasa_accessible_points*, and out_offsets.
int ct_check(rsasa_context *ctx, size_t N, const float *x, const float *y, const float *z, const float *radius,
             size_t n_points, const uint64_t *out_offsets)
{
    if (!out_offsets || (N && (!x || !y || !z || !radius))) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_points == 0 || n_points >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "n_points must be in [1, 2^31 - 1)");
    if (N >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 atoms");
    return RSASA_OK;
}

// ct_check, and the link length: finite and not negative.
int cc_check(rsasa_context *ctx, size_t N, const float *x, const float *y, const float *z, const float *radius,
             size_t n_points, float link, const uint64_t *out_offsets)
{
    int rc;
    if ((rc = ct_check(ctx, N, x, y, z, radius, n_points, out_offsets))) return rc;
    if (!(link >= 0.0f) || std::isinf(link)) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "link must be finite and not negative");
    return RSASA_OK;
}

// ---- group contacts (rsasa_group_contacts*) ----

// One run of the group contacts: the lists of pt_run stay on the device; k_group_order puts each in label order and
// counts its rows, the scan of the neighbour counts turns those into out_offsets, the caller's row buffers are checked
// against out_offsets[N] as nb_run checks its entries, and k_group_points fills the rows.
int gp_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id,
           const uint32_t *group, const uint32_t *so, size_t S, size_t N, float probe, size_t n_points, uint64_t *out_offsets,
           uint32_t *out_groups, uint32_t *out_buried, uint32_t *out_only, size_t cap, uint32_t *out_self_free,
           uint32_t *out_free, float *out_sasa)
{
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    int rc;
    if (N == 0) {
        out_offsets[0] = 0;
        return RSASA_OK;
    }
    hipStream_t st = ctx->stream;
    NbArgs a{};
    NbInfo info{};
    if ((rc = nb_count(ctx, x, y, z, r, id, so, S, N, nullptr, probe, __builtin_nanf(""), nullptr, a, info))) return rc;
    if (info.total && ((rc = nb_fill(ctx, a, info)) || (rc = reserve(ctx, ctx->gp_sorted, info.total * 8)) ||
                       (rc = reserve(ctx, ctx->gp_sorted_group, info.total * 4))))
        return rc;
    if ((rc = reserve(ctx, ctx->gp_group, N * 4)) || (rc = reserve(ctx, ctx->gp_own, N * 4)) ||
        (rc = reserve(ctx, ctx->gp_nrows, N * 4)) || (rc = reserve(ctx, ctx->gp_offsets, (N + 1) * 8)))
        return rc;
    RS_HIP(ctx, hipMemcpyAsync(ctx->gp_group.p, group, N * 4, hipMemcpyHostToDevice, st));
    GpArgs g{};
    g.p.b = a.b;
    g.p.offsets = a.offsets;
    g.p.entries = (const uint2 *)ctx->nb_entries.p;  // (neither the lists nor their copies are read when every list is empty)
    g.group = (const uint32_t *)ctx->gp_group.p;
    g.sorted = (uint2 *)ctx->gp_sorted.p;
    g.sorted_group = (uint32_t *)ctx->gp_sorted_group.p;
    g.n_own = (uint32_t *)ctx->gp_own.p;
    g.n_rows = (uint32_t *)ctx->gp_nrows.p;
    g.row_offsets = (const unsigned long long *)ctx->gp_offsets.p;
    launch_group_order(g, st);
    NbArgs scan = a;  // (the neighbour run has read its parts and its info)
    scan.counts = g.n_rows;
    scan.offsets = (unsigned long long *)ctx->gp_offsets.p;
    launch_neighbor_scan(scan, st);
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, hipMemcpyAsync(out_offsets, g.row_offsets, (N + 1) * 8, hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    const uint64_t n_rows = out_offsets[N];
    if (!out_groups || !out_buried || !out_only || cap < n_rows)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "a row buffer is NULL or holds fewer rows than out_offsets[n]");
    size_t padded = 0;
    if ((n_rows && ((rc = reserve(ctx, ctx->gp_groups, n_rows * 4)) || (rc = reserve(ctx, ctx->gp_buried, n_rows * 4)) ||
                    (rc = reserve(ctx, ctx->gp_only, n_rows * 4)))) ||
        (rc = reserve(ctx, ctx->gp_self_free, N * 4)) || (rc = reserve(ctx, ctx->gp_free, N * 4)) ||
        (rc = pt_lattice(ctx, n_points, padded)) || (out_sasa && (rc = reserve(ctx, ctx->pt_sasa, N * 4))))
        return rc;
    g.groups = (uint32_t *)ctx->gp_groups.p;
    g.buried = (uint32_t *)ctx->gp_buried.p;
    g.only = (uint32_t *)ctx->gp_only.p;
    g.self_free = (uint32_t *)ctx->gp_self_free.p;
    g.free = (uint32_t *)ctx->gp_free.p;
    const float *lat = (const float *)ctx->pt_lattice.p;
    g.p.lx = lat; g.p.ly = lat + padded; g.p.lz = lat + 2 * padded;
    g.p.n_points = (uint32_t)n_points;
    g.p.n_fused = (uint32_t)(n_points - n_points % (size_t)ctx->simd_width);
    g.p.sasa = out_sasa ? (float *)ctx->pt_sasa.p : nullptr;
    launch_group_points(g, st);
    RS_HIP(ctx, hipGetLastError());
    if (n_rows) {
        RS_HIP(ctx, hipMemcpyAsync(out_groups, g.groups, n_rows * 4, hipMemcpyDeviceToHost, st));
        RS_HIP(ctx, hipMemcpyAsync(out_buried, g.buried, n_rows * 4, hipMemcpyDeviceToHost, st));
        RS_HIP(ctx, hipMemcpyAsync(out_only, g.only, n_rows * 4, hipMemcpyDeviceToHost, st));
    }
    RS_HIP(ctx, hipMemcpyAsync(out_self_free, g.self_free, N * 4, hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipMemcpyAsync(out_free, g.free, N * 4, hipMemcpyDeviceToHost, st));
    if (out_sasa) RS_HIP(ctx, hipMemcpyAsync(out_sasa, g.p.sasa, N * 4, hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    return RSASA_OK;
}

// ct_check, and the arrays every atom has an entry of.
int gp_check(rsasa_context *ctx, size_t N, const float *x, const float *y, const float *z, const float *radius,
             const uint32_t *group, size_t n_points, const uint64_t *out_offsets, const uint32_t *out_self_free,
             const uint32_t *out_free)
{
    int rc;
    if ((rc = ct_check(ctx, N, x, y, z, radius, n_points, out_offsets))) return rc;
    if (N && (!group || !out_self_free || !out_free)) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    return RSASA_OK;
}

}  // namespace

extern "C" {

int rsasa_precompute_neighbors(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                               const uint64_t *id, size_t n_atoms, const uint32_t *active_indices, size_t n_active,
                               float probe_radius, float max_radius, uint64_t *out_offsets, rsasa_neighbor_t *out_entries,
                               size_t entries_capacity)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    const size_t n = active_indices ? n_active : n_atoms;
    if (!out_offsets || (n_atoms && (!x || !y || !z || !radius)) || (n_active && !active_indices))
        return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_atoms >= 0x7FFFFFFFull || n >= 0x7FFFFFFFull)
        return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 atoms");
    if (!active_indices) {
        const uint32_t so[2] = {0u, (uint32_t)n_atoms};
        return nb_run(ctx, x, y, z, radius, id, so, 1, n_atoms, nullptr, probe_radius, max_radius, out_offsets, out_entries,
                      entries_capacity);
    }
    // only the active atoms are binned and bounded (spatial_grid.rs:52-90, calculate_bounds): gather them, map idx back
    std::vector<uint8_t> seen(n_atoms, 0);
    std::vector<float> gx(n), gy(n), gz(n), gr(n);
    std::vector<uint64_t> gid(id ? n : 0);
    for (size_t k = 0; k < n; k++) {
        const uint32_t i = active_indices[k];
        if (i >= n_atoms || seen[i]) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "active_indices must be distinct and below n_atoms");
        seen[i] = 1;
        gx[k] = x[i]; gy[k] = y[i]; gz[k] = z[i]; gr[k] = radius[i];
        if (id) gid[k] = id[i];
    }
    const uint32_t so[2] = {0u, (uint32_t)n};
    return nb_run(ctx, gx.data(), gy.data(), gz.data(), gr.data(), id ? gid.data() : nullptr, so, 1, n, active_indices,
                  probe_radius, max_radius, out_offsets, out_entries, entries_capacity);
}

int rsasa_precompute_neighbors_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                                     const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                                     float probe_radius, float max_radius, uint64_t *out_offsets, rsasa_neighbor_t *out_entries,
                                     size_t entries_capacity)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (!structure_offsets || !out_offsets) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_structures >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "too many structures");
    for (size_t s = 0; s < n_structures; s++)
        if (structure_offsets[s] > structure_offsets[s + 1])
            return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "structure_offsets must be non-decreasing");
    const size_t N = n_structures ? structure_offsets[n_structures] : 0;
    if (n_structures && structure_offsets[0] != 0) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "structure_offsets[0] must be 0");
    if (N >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 atoms");
    if (N && (!x || !y || !z || !radius)) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    return nb_run(ctx, x, y, z, radius, id, structure_offsets, n_structures, N, nullptr, probe_radius, max_radius, out_offsets,
                  out_entries, entries_capacity);
}

int rsasa_accessible_points(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                            const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, uint32_t *out_masks,
                            float *out_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (n_atoms && (!x || !y || !z || !radius || !out_masks)) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_points == 0 || n_points >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "n_points must be in [1, 2^31 - 1)");
    if (n_atoms >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 atoms");
    const uint32_t so[2] = {0u, (uint32_t)n_atoms};
    return pt_run(ctx, x, y, z, radius, id, so, 1, n_atoms, probe_radius, n_points, out_masks, out_sasa);
}

int rsasa_accessible_points_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                                  const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                                  float probe_radius, size_t n_points, uint32_t *out_masks, float *out_atom_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (!structure_offsets) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_points == 0 || n_points >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "n_points must be in [1, 2^31 - 1)");
    if (n_structures >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "too many structures");
    for (size_t s = 0; s < n_structures; s++)
        if (structure_offsets[s] > structure_offsets[s + 1])
            return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "structure_offsets must be non-decreasing");
    const size_t N = n_structures ? structure_offsets[n_structures] : 0;
    if (n_structures && structure_offsets[0] != 0) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "structure_offsets[0] must be 0");
    if (N >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 atoms");
    if (N && (!x || !y || !z || !radius || !out_masks)) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    return pt_run(ctx, x, y, z, radius, id, structure_offsets, n_structures, N, probe_radius, n_points, out_masks, out_atom_sasa);
}

int rsasa_exposure_vectors(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                           const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, float *out_vectors,
                           uint32_t *out_free, float *out_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (n_atoms && (!x || !y || !z || !radius || !out_vectors || !out_free)) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_points == 0 || n_points >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "n_points must be in [1, 2^31 - 1)");
    if (n_atoms >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 atoms");
    const uint32_t so[2] = {0u, (uint32_t)n_atoms};
    return ex_run(ctx, x, y, z, radius, id, so, 1, n_atoms, probe_radius, n_points, out_vectors, out_free, out_sasa);
}

int rsasa_exposure_vectors_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                                 const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                                 float probe_radius, size_t n_points, float *out_vectors, uint32_t *out_free,
                                 float *out_atom_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (!structure_offsets) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_points == 0 || n_points >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "n_points must be in [1, 2^31 - 1)");
    if (n_structures >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "too many structures");
    for (size_t s = 0; s < n_structures; s++)
        if (structure_offsets[s] > structure_offsets[s + 1])
            return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "structure_offsets must be non-decreasing");
    const size_t N = n_structures ? structure_offsets[n_structures] : 0;
    if (n_structures && structure_offsets[0] != 0) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "structure_offsets[0] must be 0");
    if (N >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 atoms");
    if (N && (!x || !y || !z || !radius || !out_vectors || !out_free)) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    return ex_run(ctx, x, y, z, radius, id, structure_offsets, n_structures, N, probe_radius, n_points, out_vectors, out_free,
                  out_atom_sasa);
}

int rsasa_atom_depth(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                     const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, float *out_depth,
                     uint32_t *out_nearest, uint32_t *out_free, float *out_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (n_atoms && (!x || !y || !z || !radius || !out_depth || !out_nearest)) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_points == 0 || n_points >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "n_points must be in [1, 2^31 - 1)");
    if (n_atoms >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 atoms");
    const uint32_t so[2] = {0u, (uint32_t)n_atoms};
    return dp_run(ctx, x, y, z, radius, id, so, 1, n_atoms, probe_radius, n_points, out_depth, out_nearest, out_free, out_sasa);
}

int rsasa_atom_depth_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                           const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                           size_t n_points, float *out_depth, uint32_t *out_nearest, uint32_t *out_free, float *out_atom_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (!structure_offsets) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_points == 0 || n_points >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "n_points must be in [1, 2^31 - 1)");
    if (n_structures >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "too many structures");
    for (size_t s = 0; s < n_structures; s++)
        if (structure_offsets[s] > structure_offsets[s + 1])
            return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "structure_offsets must be non-decreasing");
    const size_t N = n_structures ? structure_offsets[n_structures] : 0;
    if (n_structures && structure_offsets[0] != 0) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "structure_offsets[0] must be 0");
    if (N >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 atoms");
    if (N && (!x || !y || !z || !radius || !out_depth || !out_nearest)) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    return dp_run(ctx, x, y, z, radius, id, structure_offsets, n_structures, N, probe_radius, n_points, out_depth, out_nearest,
                  out_free, out_atom_sasa);
}

int rsasa_surface_components(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                             const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, float link,
                             uint64_t *out_dot_offsets, uint32_t *out_labels, size_t labels_capacity, uint32_t *out_free,
                             float *out_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if ((rc = cc_check(ctx, n_atoms, x, y, z, radius, n_points, link, out_dot_offsets))) return rc;
    const uint32_t so[2] = {0u, (uint32_t)n_atoms};
    return cc_run(ctx, x, y, z, radius, id, so, 1, n_atoms, probe_radius, n_points, link, out_dot_offsets, out_labels,
                  labels_capacity, out_free, out_sasa);
}

int rsasa_surface_components_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                                   const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                                   float probe_radius, size_t n_points, float link, uint64_t *out_dot_offsets,
                                   uint32_t *out_labels, size_t labels_capacity, uint32_t *out_free, float *out_atom_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (!structure_offsets) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_structures >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "too many structures");
    for (size_t s = 0; s < n_structures; s++)
        if (structure_offsets[s] > structure_offsets[s + 1])
            return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "structure_offsets must be non-decreasing");
    const size_t N = n_structures ? structure_offsets[n_structures] : 0;
    if (n_structures && structure_offsets[0] != 0) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "structure_offsets[0] must be 0");
    if ((rc = cc_check(ctx, N, x, y, z, radius, n_points, link, out_dot_offsets))) return rc;
    return cc_run(ctx, x, y, z, radius, id, structure_offsets, n_structures, N, probe_radius, n_points, link, out_dot_offsets,
                  out_labels, labels_capacity, out_free, out_atom_sasa);
}

// No context, no device: double arithmetic in atom order on the host.
int rsasa_sas_volume(const float *x, const float *y, const float *z, const float *radius, const float *vectors,
                     const uint32_t *free_points, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                     size_t n_points, const double *origins, double *out_volume, double *out_area)
{
    if (!structure_offsets || n_points == 0 || (n_structures && !out_volume)) return RSASA_ERR_INVALID_ARGUMENT;
    if (n_structures && structure_offsets[0] != 0) return RSASA_ERR_INVALID_ARGUMENT;
    for (size_t s = 0; s < n_structures; s++)
        if (structure_offsets[s] > structure_offsets[s + 1]) return RSASA_ERR_INVALID_ARGUMENT;
    const size_t N = n_structures ? structure_offsets[n_structures] : 0;
    if (N && (!x || !y || !z || !radius || !vectors || !free_points)) return RSASA_ERR_INVALID_ARGUMENT;
    const double four_pi = 4.0 * 3.14159265358979323846;
    for (size_t s = 0; s < n_structures; s++) {
        const size_t b = structure_offsets[s], e = structure_offsets[s + 1];
        auto counted = [&](size_t i) { return std::isfinite(x[i]) && std::isfinite(y[i]) && std::isfinite(z[i]) && std::isfinite(radius[i]); };
        double ox = 0.0, oy = 0.0, oz = 0.0;
        if (origins) {
            ox = origins[3 * s]; oy = origins[3 * s + 1]; oz = origins[3 * s + 2];
        } else {
            size_t n = 0;
            for (size_t i = b; i < e; i++)
                if (counted(i)) { ox += (double)x[i]; oy += (double)y[i]; oz += (double)z[i]; n++; }
            if (n) { ox /= (double)n; oy /= (double)n; oz /= (double)n; }
        }
        double vol = 0.0, area = 0.0;
        for (size_t i = b; i < e; i++) {
            if (!counted(i)) continue;
            const float Rf = radius[i] + probe_radius;  // lib.rs:101, in float32
            const double R = (double)Rf, k = (double)free_points[i];
            const double a = (four_pi * (R * R)) / (double)n_points;
            const double dot = ((double)x[i] - ox) * (double)vectors[3 * i] + ((double)y[i] - oy) * (double)vectors[3 * i + 1] +
                               ((double)z[i] - oz) * (double)vectors[3 * i + 2];
            vol += (a / 3.0) * (R * k + dot);
            area += a * k;
        }
        out_volume[s] = vol;
        if (out_area) out_area[s] = area;
    }
    return RSASA_OK;
}

int rsasa_contact_points(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                         const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, uint64_t *out_offsets,
                         rsasa_neighbor_t *out_entries, uint32_t *out_covered, uint32_t *out_exclusive,
                         size_t entries_capacity, float *out_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if ((rc = ct_check(ctx, n_atoms, x, y, z, radius, n_points, out_offsets))) return rc;
    const uint32_t so[2] = {0u, (uint32_t)n_atoms};
    return ct_run(ctx, x, y, z, radius, id, so, 1, n_atoms, probe_radius, n_points, out_offsets, out_entries, out_covered,
                  out_exclusive, entries_capacity, out_sasa);
}

int rsasa_contact_points_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                               const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                               float probe_radius, size_t n_points, uint64_t *out_offsets, rsasa_neighbor_t *out_entries,
                               uint32_t *out_covered, uint32_t *out_exclusive, size_t entries_capacity,
                               float *out_atom_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (!structure_offsets) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_structures >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "too many structures");
    for (size_t s = 0; s < n_structures; s++)
        if (structure_offsets[s] > structure_offsets[s + 1])
            return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "structure_offsets must be non-decreasing");
    const size_t N = n_structures ? structure_offsets[n_structures] : 0;
    if (n_structures && structure_offsets[0] != 0) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "structure_offsets[0] must be 0");
    if ((rc = ct_check(ctx, N, x, y, z, radius, n_points, out_offsets))) return rc;
    return ct_run(ctx, x, y, z, radius, id, structure_offsets, n_structures, N, probe_radius, n_points, out_offsets,
                  out_entries, out_covered, out_exclusive, entries_capacity, out_atom_sasa);
}

int rsasa_group_contacts(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                         const uint64_t *id, const uint32_t *group, size_t n_atoms, float probe_radius, size_t n_points,
                         uint64_t *out_offsets, uint32_t *out_groups, uint32_t *out_buried, uint32_t *out_only,
                         size_t rows_capacity, uint32_t *out_self_free, uint32_t *out_free, float *out_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if ((rc = gp_check(ctx, n_atoms, x, y, z, radius, group, n_points, out_offsets, out_self_free, out_free))) return rc;
    const uint32_t so[2] = {0u, (uint32_t)n_atoms};
    return gp_run(ctx, x, y, z, radius, id, group, so, 1, n_atoms, probe_radius, n_points, out_offsets, out_groups, out_buried,
                  out_only, rows_capacity, out_self_free, out_free, out_sasa);
}

int rsasa_group_contacts_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                               const uint64_t *id, const uint32_t *group, const uint32_t *structure_offsets,
                               size_t n_structures, float probe_radius, size_t n_points, uint64_t *out_offsets,
                               uint32_t *out_groups, uint32_t *out_buried, uint32_t *out_only, size_t rows_capacity,
                               uint32_t *out_self_free, uint32_t *out_free, float *out_atom_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (!structure_offsets) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_structures >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "too many structures");
    for (size_t s = 0; s < n_structures; s++)
        if (structure_offsets[s] > structure_offsets[s + 1])
            return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "structure_offsets must be non-decreasing");
    const size_t N = n_structures ? structure_offsets[n_structures] : 0;
    if (n_structures && structure_offsets[0] != 0) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "structure_offsets[0] must be 0");
    if ((rc = gp_check(ctx, N, x, y, z, radius, group, n_points, out_offsets, out_self_free, out_free))) return rc;
    return gp_run(ctx, x, y, z, radius, id, group, structure_offsets, n_structures, N, probe_radius, n_points, out_offsets,
                  out_groups, out_buried, out_only, rows_capacity, out_self_free, out_free, out_atom_sasa);
}

}  // extern "C"
