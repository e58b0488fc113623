// Host side of the neighbour-list entry points (rsasa_precompute_neighbors / _batch, include/rustsasa_amd.h) and of the
// point runs built on them: accessible points, exposure vectors, atom depth, surface components, dot crowding, contact
// counts, contact owners and group contacts; and of the half-sphere exposure, the lists within a cutoff, the k nearest atoms and the radial counts,
// which need the grid alone.  The batch's grid is built by the SASA path's kernels in a workspace of the context's own (rsasa_context::nb_ws;
// nb_grid, and hs_grid for the runs on the grid alone), then neighbors.hip counts, scans and fills the lists (nb_count,
// nb_fill).  A point run keeps the lists on the device: every family shares one prologue (pt_count, pt_prepare: lists
// with the SASA path's cutoff, lattice, PtArgs) and adds its own kernels of points.hip, depth.hip or components.hip and
// its own downloads.  Every entry point is: resolve_ctx, the argument rules of entry_checks.h, a Cols, the family's run
// function.
// rsasa_sas_volume is plain host arithmetic on what the exposure vectors return.  Host code only.
#include "engine_internal.h"
#include "entry_checks.h"

#include <cmath>
#include <cstring>

namespace {

using namespace rsasa;

#define RS_ARGS(ctx, rule)                                                               \
    do {                                                                                 \
        if (const char *msg_ = (rule)) return fail((ctx), RSASA_ERR_INVALID_ARGUMENT, msg_); \
    } while (0)

struct NbHost {  // the pinned block the device's verdicts come back in
    BatchStatus status;
    NbInfo info;
    uint64_t last_offset;  // offsets[N], when the caller wants no host copy of the offsets
};

// The upload and the grid of a run over columns already in host memory: c.N >= 1 atoms.  idx_map (host, nullable) is
// uploaded beside the columns (RunScratch::map).  On RSASA_OK `v` describes the binned batch.  The caller holds the
// context's mutex and has made its device current.
int nb_grid(rsasa_context *ctx, const Cols &c, const uint32_t *idx_map, float probe, float max_r, BatchView &v)
{
    int rc;
    rsasa_context::Workspace &W = ctx->nb_ws;
    rsasa_context::RunScratch &R = ctx->run;
    hipStream_t st = ctx->stream;
    const size_t N = c.N;

    const SegmentCount sc = count_segments(c.so, c.S);
    std::vector<Segment> segs(sc.n_seg);
    write_segments(c.so, c.S, segs.data(), nullptr);
    const bool has_tail = sc.has_tail;
    const bool has_id = c.id != nullptr;
    if (!ctx->nb_host.p) RS_HIP(ctx, ctx->nb_host.regrow(sizeof(NbHost)));
    NbHost *h = static_cast<NbHost *>(ctx->nb_host.p);

    if ((rc = reserve(ctx, R.x, N * 4)) || (rc = reserve(ctx, R.y, N * 4)) || (rc = reserve(ctx, R.z, N * 4)) ||
        (rc = reserve(ctx, R.r, N * 4)) || (has_id && (rc = reserve(ctx, R.id, N * 8))) ||
        (idx_map && (rc = reserve(ctx, R.map, N * 4))))
        return rc;
    RS_HIP(ctx, hipMemcpyAsync(R.x.p, c.x, N * 4, hipMemcpyHostToDevice, st));
    RS_HIP(ctx, hipMemcpyAsync(R.y.p, c.y, N * 4, hipMemcpyHostToDevice, st));
    RS_HIP(ctx, hipMemcpyAsync(R.z.p, c.z, N * 4, hipMemcpyHostToDevice, st));
    RS_HIP(ctx, hipMemcpyAsync(R.r.p, c.r, N * 4, hipMemcpyHostToDevice, st));
    if (has_id) RS_HIP(ctx, hipMemcpyAsync(R.id.p, c.id, N * 8, hipMemcpyHostToDevice, st));
    if (idx_map) RS_HIP(ctx, hipMemcpyAsync(R.map.p, idx_map, N * 4, hipMemcpyHostToDevice, st));

    // ---- the grid (without the id check: every id takes part), grown until the cells fit
    for (int attempt = 0;; attempt++) {
        if ((rc = W.reserve_grid(ctx, N, c.S, segs.size(), ctx->nb_cell_capacity, has_tail, has_id))) return rc;
        if (!segs.empty())
            RS_HIP(ctx, hipMemcpyAsync(W.segments.p, segs.data(), segs.size() * sizeof(Segment), hipMemcpyHostToDevice, st));
        v = BatchView{};
        v.x = (const float *)R.x.p; v.y = (const float *)R.y.p; v.z = (const float *)R.z.p;
        v.radius = (const float *)R.r.p;
        v.id = has_id ? (const uint64_t *)R.id.p : nullptr;
        v.n_atoms = (uint32_t)N; v.n_structures = (uint32_t)c.S; v.n_segments = (uint32_t)segs.size();
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
    return RSASA_OK;
}

// The buffers a count pass and its scan write (counts, offsets, parts, a cleared NbInfo) for the N atoms of a.b, and
// the length above which the run's fill kernel takes a list for long.
int nb_scan_buffers(rsasa_context *ctx, size_t N, uint32_t stage, NbArgs &a)
{
    int rc;
    rsasa_context::RunScratch &R = ctx->run;
    if ((rc = reserve(ctx, R.counts, N * 4)) || (rc = reserve(ctx, R.offsets, (N + 1) * 8)) ||
        (rc = reserve(ctx, R.parts, 4 * 1024 * 8)) || (rc = reserve(ctx, R.info, sizeof(NbInfo))))
        return rc;
    a.counts = (uint32_t *)R.counts.p;
    a.offsets = (unsigned long long *)R.offsets.p;
    a.parts = (unsigned long long *)R.parts.p;
    a.info = (NbInfo *)R.info.p;
    a.stage = stage;
    RS_HIP(ctx, hipMemsetAsync(a.info, 0, sizeof(NbInfo), ctx->stream));
    return RSASA_OK;
}

// What a queued count pass and scan found: waits for them; `info` gets the lists' sizes and out_offsets (nullable:
// [N + 1]) the offsets.
int nb_sizes(rsasa_context *ctx, const NbArgs &a, size_t N, uint64_t *out_offsets, NbInfo &info)
{
    hipStream_t st = ctx->stream;
    NbHost *h = static_cast<NbHost *>(ctx->nb_host.p);
    RS_HIP(ctx, hipMemcpyAsync(&h->info, a.info, sizeof(NbInfo), hipMemcpyDeviceToHost, st));
    if (out_offsets) RS_HIP(ctx, hipMemcpyAsync(out_offsets, a.offsets, (N + 1) * 8, hipMemcpyDeviceToHost, st));
    else RS_HIP(ctx, hipMemcpyAsync(&h->last_offset, a.offsets + N, 8, hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, hipStreamSynchronize(st));
    info = h->info;
    if (info.total != (out_offsets ? out_offsets[N] : h->last_offset))
        return fail(ctx, RSASA_ERR_INTERNAL, "list offsets disagree with their total");
    return RSASA_OK;
}

// nb_grid, and the counts of the lists on that grid.  idx_map: input atom -> the index written to the entries.
// out_offsets (nullable): [N + 1], the offsets are copied there.  On RSASA_OK `a` describes the device lists (everything
// but their entries) and `info` their sizes.
int nb_count(rsasa_context *ctx, const Cols &c, const uint32_t *idx_map, float probe, float max_r, uint64_t *out_offsets,
             NbArgs &a, NbInfo &info)
{
    int rc;
    a = NbArgs{};
    if ((rc = nb_grid(ctx, c, idx_map, probe, max_r, a.b)) || (rc = nb_scan_buffers(ctx, c.N, neighbor_stage_capacity(), a)))
        return rc;
    a.idx_map = idx_map ? (const uint32_t *)ctx->run.map.p : nullptr;
    launch_neighbor_count(a, ctx->stream);
    return nb_sizes(ctx, a, c.N, out_offsets, info);
}

// The entries of the lists a count pass sized (info.total >= 1), sorted, in a.out on the device: reserves them and the
// long lists' scratch, runs `launch(info.spill_atoms)` - the family's fill kernels over `a` - and checks that the fill
// pass agreed with the count pass.
template <class Launch>
int nb_fill_by(rsasa_context *ctx, NbArgs &a, const NbInfo &info, Launch launch)
{
    int rc;
    rsasa_context::RunScratch &R = ctx->run;
    hipStream_t st = ctx->stream;
    NbHost *h = static_cast<NbHost *>(ctx->nb_host.p);
    if ((rc = reserve(ctx, R.entries, info.total * 8)) ||
        (info.spill_atoms && ((rc = reserve(ctx, R.spill, info.spill_entries * sizeof(NbKey))) ||
                              (rc = reserve(ctx, R.recs, info.spill_atoms * sizeof(NbSpillRec))))))
        return rc;
    a.out = (uint2 *)R.entries.p;
    a.spill = info.spill_atoms ? (NbKey *)R.spill.p : nullptr;
    a.spill_recs = info.spill_atoms ? (NbSpillRec *)R.recs.p : nullptr;
    launch(info.spill_atoms);
    RS_HIP(ctx, hipMemcpyAsync(&h->info, a.info, sizeof(NbInfo), hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, hipStreamSynchronize(st));
    if (h->info.mismatch || h->info.spill_cursor != info.spill_entries || h->info.spill_recs != info.spill_atoms)
        return fail(ctx, RSASA_ERR_INTERNAL, "the fill pass of the lists disagrees with its count pass");
    return RSASA_OK;
}

// The entries of the lists nb_count sized (info.total >= 1).
int nb_fill(rsasa_context *ctx, NbArgs &a, const NbInfo &info)
{
    return nb_fill_by(ctx, a, info, [&](uint64_t spill_atoms) { launch_neighbor_fill(a, spill_atoms, ctx->stream); });
}

// Queues the copy of `bytes` from the device into a host array that the caller may have left out.
hipError_t download(void *out, const void *from, size_t bytes, hipStream_t st)
{
    return out ? hipMemcpyAsync(out, from, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
}

// One neighbour-list run (see nb_count).
int nb_run(rsasa_context *ctx, const Cols &c, const uint32_t *idx_map, float probe, float max_r, uint64_t *out_offsets,
           rsasa_neighbor_t *out_entries, size_t cap)
{
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    int rc;
    if (c.N == 0) {
        out_offsets[0] = 0;
        return RSASA_OK;
    }
    NbArgs a{};
    NbInfo info{};
    if ((rc = nb_count(ctx, c, idx_map, probe, max_r, out_offsets, a, info))) return rc;
    if (!out_entries || cap < info.total)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "out_entries holds fewer entries than out_offsets[n]");
    if (info.total == 0) return RSASA_OK;
    if ((rc = nb_fill(ctx, a, info))) return rc;
    RS_HIP(ctx, hipMemcpyAsync(out_entries, a.out, info.total * 8, hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RSASA_OK;
}

// ---- the point runs: what the six families share ----

// The lattice in the reference's order (lib.rs:43-66) on the device: x | y | z, each zero padded to whole 64s.
// (Made once per point count: the copy and the wait happen in the first call at that count only.)
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

struct Lists {  // the device lists of a point run: nb_count's description and sizes
    NbArgs a{};
    NbInfo info{};
};

// The prologue's count step (c.N >= 1): the lists calculate_sasa_internal builds (lib.rs:259-267) - nb_count with
// max_r = NaN - sized on the device; out_offsets (nullable) as in nb_count.  A family that sizes a caller's buffer by
// l.info.total answers RSASA_ERR_BUFFER_TOO_SMALL between this step and the next.
int pt_count(rsasa_context *ctx, const Cols &c, float probe, uint64_t *out_offsets, Lists &l)
{
    return nb_count(ctx, c, nullptr, probe, __builtin_nanf(""), out_offsets, l.a, l.info);
}

// The prologue's fill-and-prepare step: the lists' entries (no fill when every list is empty: `entries` is then null or
// stale, and no kernel reads it), the lattice, and the masks and values if the family wants them; `p` is then what every
// point kernel takes.  The masks and values stay on the device (RunScratch::masks, ::sasa) for the family to use.
int pt_prepare(rsasa_context *ctx, Lists &l, size_t n_points, bool masks, bool sasa, PtArgs &p)
{
    int rc;
    rsasa_context::RunScratch &R = ctx->run;
    const size_t N = l.a.b.n_atoms, words = (n_points + 31) / 32;
    size_t padded = 0;
    if ((l.info.total && (rc = nb_fill(ctx, l.a, l.info))) || (rc = pt_lattice(ctx, n_points, padded)) ||
        (masks && (rc = reserve(ctx, R.masks, N * words * 4))) || (sasa && (rc = reserve(ctx, R.sasa, N * 4))))
        return rc;
    p = PtArgs{};
    p.b = l.a.b;
    p.offsets = l.a.offsets;
    p.entries = (const uint2 *)R.entries.p;
    const float *lat = (const float *)ctx->pt_lattice.p;
    p.lx = lat; p.ly = lat + padded; p.lz = lat + 2 * padded;
    p.n_points = (uint32_t)n_points;
    p.n_fused = (uint32_t)(n_points - n_points % (size_t)ctx->simd_width);
    if (masks) {
        p.words = (uint32_t)words;
        p.masks = (uint32_t *)R.masks.p;
    }
    p.sasa = sasa ? (float *)R.sasa.p : nullptr;
    return RSASA_OK;
}

// ---- accessible points (rsasa_accessible_points*) ----

// One run of the point tests: k_accessible_points turns the lists into masks.
int pt_run(rsasa_context *ctx, const Cols &c, float probe, size_t n_points, uint32_t *out_masks, float *out_sasa)
{
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    if (c.N == 0) return RSASA_OK;
    int rc;
    Lists l;
    PtArgs p{};
    if ((rc = pt_count(ctx, c, probe, nullptr, l)) || (rc = pt_prepare(ctx, l, n_points, true, out_sasa != nullptr, p))) return rc;
    hipStream_t st = ctx->stream;
    launch_accessible_points(p, st);
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, download(out_masks, p.masks, c.N * p.words * 4, st));
    RS_HIP(ctx, download(out_sasa, p.sasa, c.N * 4, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    return RSASA_OK;
}

// ---- exposure vectors (rsasa_exposure_vectors*) ----

// One run of the exposure vectors: k_exposure_vectors turns the lists into the sum of each atom's exposed lattice points
// and their number; 16 bytes per atom come back (and 4 for the value, if asked).
int ex_run(rsasa_context *ctx, const Cols &c, float probe, size_t n_points, float *out_vectors, uint32_t *out_free,
           float *out_sasa)
{
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    if (c.N == 0) return RSASA_OK;
    int rc;
    rsasa_context::RunScratch &R = ctx->run;
    Lists l;
    ExArgs e{};
    if ((rc = pt_count(ctx, c, probe, nullptr, l)) || (rc = pt_prepare(ctx, l, n_points, false, out_sasa != nullptr, e.p)) ||
        (rc = reserve(ctx, R.vectors, c.N * 12)) || (rc = reserve(ctx, R.free, c.N * 4)))
        return rc;
    e.vectors = (float *)R.vectors.p;
    e.free = (uint32_t *)R.free.p;
    hipStream_t st = ctx->stream;
    launch_exposure_vectors(e, st);
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, download(out_vectors, e.vectors, c.N * 12, st));
    RS_HIP(ctx, download(out_free, e.free, c.N * 4, st));
    RS_HIP(ctx, download(out_sasa, e.p.sasa, c.N * 4, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    return RSASA_OK;
}

// ---- atom depth (rsasa_atom_depth*) ----

// One run of the atom depths: pt_run's masks stay on the device; k_mask_free counts them and k_atom_depth searches the
// grid for every atom's nearest accessible dot.  8 bytes per atom come back (and 4 each for the counts and the values,
// if asked); the square root of the key's d2 is taken here (sqrtf: correctly rounded).
int dp_run(rsasa_context *ctx, const Cols &c, float probe, size_t n_points, float *out_depth, uint32_t *out_nearest,
           uint32_t *out_free, float *out_sasa)
{
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    if (c.N == 0) return RSASA_OK;
    int rc;
    rsasa_context::RunScratch &R = ctx->run;
    Lists l;
    DpArgs d{};
    if ((rc = pt_count(ctx, c, probe, nullptr, l)) || (rc = pt_prepare(ctx, l, n_points, true, out_sasa != nullptr, d.p)) ||
        (rc = reserve(ctx, R.keys, c.N * 8)) || (rc = reserve(ctx, R.free, c.N * 4)))
        return rc;
    d.free = (uint32_t *)R.free.p;
    d.keys = (unsigned long long *)R.keys.p;
    hipStream_t st = ctx->stream;
    launch_accessible_points(d.p, st);
    launch_mask_free(d.p, d.free, st);
    launch_atom_depth(d, st);
    RS_HIP(ctx, hipGetLastError());
    std::vector<uint64_t> keys(c.N);
    RS_HIP(ctx, download(keys.data(), d.keys, c.N * 8, st));
    RS_HIP(ctx, download(out_free, d.free, c.N * 4, st));
    RS_HIP(ctx, download(out_sasa, d.p.sasa, c.N * 4, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    for (size_t i = 0; i < c.N; i++) {
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

// One run of the surface components: pt_run's masks stay on the device; k_mask_free counts them, the scan of the
// neighbour counts turns the counts into out_offsets, the caller's label buffer is checked against out_offsets[N] as
// nb_run checks its entries, and the union-find kernels label the dots.  8 bytes per atom and 4 per dot come back (and
// 4 per atom each for the counts and the values, if asked).
int cc_run(rsasa_context *ctx, const Cols &c, float probe, size_t n_points, float link, uint64_t *out_offsets,
           uint32_t *out_labels, size_t cap, uint32_t *out_free, float *out_sasa)
{
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    if (c.N == 0) {
        out_offsets[0] = 0;
        return RSASA_OK;
    }
    int rc;
    rsasa_context::RunScratch &R = ctx->run;
    Lists l;
    CcArgs cc{};
    if ((rc = pt_count(ctx, c, probe, nullptr, l)) || (rc = pt_prepare(ctx, l, n_points, true, out_sasa != nullptr, cc.p)) ||
        (rc = reserve(ctx, R.free, c.N * 4)) || (rc = reserve(ctx, R.row_offsets, (c.N + 1) * 8)))
        return rc;
    cc.free = (uint32_t *)R.free.p;
    cc.dot_offsets = (const unsigned long long *)R.row_offsets.p;
    cc.link = link;
    cc.link2 = link * link;
    hipStream_t st = ctx->stream;
    launch_accessible_points(cc.p, st);
    launch_mask_free(cc.p, cc.free, st);
    NbArgs scan = l.a;  // (the neighbour run has read its parts and its info)
    scan.counts = cc.free;
    scan.offsets = (unsigned long long *)R.row_offsets.p;
    launch_neighbor_scan(scan, st);
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, download(out_offsets, cc.dot_offsets, (c.N + 1) * 8, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    const uint64_t n_dots = out_offsets[c.N];
    if (n_dots >= 0x100000000ull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "2^32 or more accessible dots");
    if (!out_labels || cap < n_dots)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "out_labels is NULL or holds fewer labels than out_dot_offsets[n]");
    if (n_dots) {
        if ((rc = reserve(ctx, R.parent, n_dots * 4)) || (rc = reserve(ctx, R.labels, n_dots * 4))) return rc;
        cc.n_dots = n_dots;
        cc.parent = (uint32_t *)R.parent.p;
        cc.labels = (uint32_t *)R.labels.p;
        launch_components(cc, st);
        RS_HIP(ctx, hipGetLastError());
        RS_HIP(ctx, download(out_labels, cc.labels, n_dots * 4, st));
    }
    RS_HIP(ctx, download(out_free, cc.free, c.N * 4, st));
    RS_HIP(ctx, download(out_sasa, cc.p.sasa, c.N * 4, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    return RSASA_OK;
}

// ---- dot crowding (rsasa_dot_crowding*) ----

// One run of the dot crowding: cc_run's front half - the masks stay on the device, k_mask_free counts them, the scan of
// the neighbour counts turns the counts into out_offsets, the caller's buffer is checked against out_offsets[N] - with
// the flag bytes uploaded beside it (flags: host, [N], nullable) and sorted by k_sort_flags; then k_dot_crowding fills a
// row of n_bins counts per dot.  8 bytes per atom and 4 * n_bins per dot come back (and 4 per atom each for the counts
// and the values, if asked).  check_crowding has passed.
int dc_run(rsasa_context *ctx, const Cols &c, float probe, size_t n_points, const uint8_t *flags, const float *edges,
           uint32_t n_bins, uint64_t *out_offsets, uint32_t *out_counts, size_t cap, uint32_t *out_free, float *out_sasa)
{
    static_assert(kCrowdMaxBins == RSASA_CROWD_MAX_BINS, "the header's bound is the kernel's bound");
    static_assert(sizeof(DcArgs::e2) == kCrowdMaxBins * sizeof(float), "an edge per bin");
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    if (c.N == 0) {
        out_offsets[0] = 0;
        return RSASA_OK;
    }
    int rc;
    rsasa_context::RunScratch &R = ctx->run;
    Lists l;
    DcArgs dc{};
    if ((rc = pt_count(ctx, c, probe, nullptr, l)) || (rc = pt_prepare(ctx, l, n_points, true, out_sasa != nullptr, dc.p)) ||
        (rc = reserve(ctx, R.free, c.N * 4)) || (rc = reserve(ctx, R.row_offsets, (c.N + 1) * 8)) ||
        (flags && (rc = reserve(ctx, R.flags, c.N))) || (rc = reserve(ctx, R.sorted_flags, c.N)))
        return rc;
    hipStream_t st = ctx->stream;
    if (flags) RS_HIP(ctx, hipMemcpyAsync(R.flags.p, flags, c.N, hipMemcpyHostToDevice, st));
    HsArgs h{};
    h.b = dc.p.b;
    h.flags = flags ? (const uint8_t *)R.flags.p : nullptr;
    h.sorted_flags = (uint8_t *)R.sorted_flags.p;
    dc.free = (uint32_t *)R.free.p;
    dc.dot_offsets = (const unsigned long long *)R.row_offsets.p;
    dc.sorted_flags = h.sorted_flags;
    dc.n_bins = n_bins;
    for (uint32_t k = 0; k < kCrowdMaxBins; k++) {
        const float e = edges[k < n_bins ? k : n_bins - 1u];
        dc.e2[k] = e * e;
    }
    launch_accessible_points(dc.p, st);
    launch_mask_free(dc.p, dc.free, st);
    NbArgs scan = l.a;  // (the neighbour run has read its parts and its info)
    scan.counts = dc.free;
    scan.offsets = (unsigned long long *)R.row_offsets.p;
    launch_neighbor_scan(scan, st);
    launch_sort_flags(h, st);
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, download(out_offsets, dc.dot_offsets, (c.N + 1) * 8, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    const uint64_t n_dots = out_offsets[c.N];
    if (n_dots >= 0x100000000ull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "2^32 or more accessible dots");
    if (!out_counts || cap < n_dots)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "out_counts is NULL or holds fewer rows than out_dot_offsets[n]");
    if (n_dots) {
        if ((rc = reserve(ctx, R.crowd, n_dots * n_bins * 4))) return rc;
        dc.counts = (uint32_t *)R.crowd.p;
        launch_dot_crowding(dc, st);
        RS_HIP(ctx, hipGetLastError());
        RS_HIP(ctx, download(out_counts, dc.counts, n_dots * n_bins * 4, st));
    }
    RS_HIP(ctx, download(out_free, dc.free, c.N * 4, st));
    RS_HIP(ctx, download(out_sasa, dc.p.sasa, c.N * 4, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    return RSASA_OK;
}

// ---- contact counts (rsasa_contact_points*) ----

// One run of the contact counts: the lists, sized and copied out as by nb_run, and k_contact_points' counts of every
// entry beside them.
int ct_run(rsasa_context *ctx, const Cols &c, float probe, size_t n_points, uint64_t *out_offsets,
           rsasa_neighbor_t *out_entries, uint32_t *out_covered, uint32_t *out_exclusive, size_t cap, float *out_sasa)
{
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    if (c.N == 0) {
        out_offsets[0] = 0;
        return RSASA_OK;
    }
    int rc;
    rsasa_context::RunScratch &R = ctx->run;
    Lists l;
    CtArgs ct{};
    if ((rc = pt_count(ctx, c, probe, out_offsets, l))) return rc;
    const size_t total = l.info.total;
    if (!out_entries || !out_covered || !out_exclusive || cap < total)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "an entry buffer is NULL or holds fewer entries than out_offsets[n]");
    if ((rc = pt_prepare(ctx, l, n_points, false, out_sasa != nullptr, ct.p)) ||
        (total && ((rc = reserve(ctx, R.covered, total * 4)) || (rc = reserve(ctx, R.exclusive, total * 4)))))
        return rc;
    ct.covered = (uint32_t *)R.covered.p;  // (like the entries, not read when every list is empty)
    ct.exclusive = (uint32_t *)R.exclusive.p;
    hipStream_t st = ctx->stream;
    launch_contact_points(ct, st);
    RS_HIP(ctx, hipGetLastError());
    if (total) {
        RS_HIP(ctx, download(out_entries, ct.p.entries, total * 8, st));
        RS_HIP(ctx, download(out_covered, ct.covered, total * 4, st));
        RS_HIP(ctx, download(out_exclusive, ct.exclusive, total * 4, st));
    }
    RS_HIP(ctx, download(out_sasa, ct.p.sasa, c.N * 4, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    return RSASA_OK;
}

// ---- contact owners (rsasa_contact_owners*) ----

// One run of the contact owners: the lists, sized and copied out as by ct_run, and k_contact_owners' count of every
// entry beside them; the owner of every point too when the caller asks for it (no device memory for it otherwise).
int co_run(rsasa_context *ctx, const Cols &c, float probe, size_t n_points, uint64_t *out_offsets,
           rsasa_neighbor_t *out_entries, uint32_t *out_owned, size_t cap, uint32_t *out_owner, float *out_sasa)
{
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    if (c.N == 0) {
        out_offsets[0] = 0;
        return RSASA_OK;
    }
    int rc;
    rsasa_context::RunScratch &R = ctx->run;
    Lists l;
    CoArgs co{};
    if ((rc = pt_count(ctx, c, probe, out_offsets, l))) return rc;
    const size_t total = l.info.total;
    if (!out_entries || !out_owned || cap < total)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "an entry buffer is NULL or holds fewer entries than out_offsets[n]");
    if ((rc = pt_prepare(ctx, l, n_points, false, out_sasa != nullptr, co.p)) ||
        (total && (rc = reserve(ctx, R.owned, total * 4))) || (out_owner && (rc = reserve(ctx, R.owner, c.N * n_points * 4))))
        return rc;
    co.owned = (uint32_t *)R.owned.p;  // (like the entries, not read when every list is empty)
    co.owner = out_owner ? (uint32_t *)R.owner.p : nullptr;
    hipStream_t st = ctx->stream;
    launch_contact_owners(co, st);
    RS_HIP(ctx, hipGetLastError());
    if (total) {
        RS_HIP(ctx, download(out_entries, co.p.entries, total * 8, st));
        RS_HIP(ctx, download(out_owned, co.owned, total * 4, st));
    }
    RS_HIP(ctx, download(out_owner, co.owner, c.N * n_points * 4, st));
    RS_HIP(ctx, download(out_sasa, co.p.sasa, c.N * 4, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    return RSASA_OK;
}

// ---- group contacts (rsasa_group_contacts*) ----

// One run of the group contacts: k_group_order puts each list in label order and counts its rows, the scan of the
// neighbour counts turns those into out_offsets, the caller's row buffers are checked against out_offsets[N] as nb_run
// checks its entries, and k_group_points fills the rows.
int gp_run(rsasa_context *ctx, const Cols &c, const uint32_t *group, float probe, size_t n_points, uint64_t *out_offsets,
           uint32_t *out_groups, uint32_t *out_buried, uint32_t *out_only, size_t cap, uint32_t *out_self_free,
           uint32_t *out_free, float *out_sasa)
{
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    if (c.N == 0) {
        out_offsets[0] = 0;
        return RSASA_OK;
    }
    int rc;
    rsasa_context::RunScratch &R = ctx->run;
    hipStream_t st = ctx->stream;
    const size_t N = c.N;
    Lists l;
    GpArgs g{};
    if ((rc = pt_count(ctx, c, probe, nullptr, l)) || (rc = pt_prepare(ctx, l, n_points, false, out_sasa != nullptr, g.p)) ||
        (l.info.total && ((rc = reserve(ctx, R.sorted, l.info.total * 8)) || (rc = reserve(ctx, R.sorted_group, l.info.total * 4)))) ||
        (rc = reserve(ctx, R.group, N * 4)) || (rc = reserve(ctx, R.own, N * 4)) || (rc = reserve(ctx, R.nrows, N * 4)) ||
        (rc = reserve(ctx, R.row_offsets, (N + 1) * 8)))
        return rc;
    RS_HIP(ctx, hipMemcpyAsync(R.group.p, group, N * 4, hipMemcpyHostToDevice, st));
    g.group = (const uint32_t *)R.group.p;
    g.sorted = (uint2 *)R.sorted.p;  // (like the entries, the lists' copies are not read when every list is empty)
    g.sorted_group = (uint32_t *)R.sorted_group.p;
    g.n_own = (uint32_t *)R.own.p;
    g.n_rows = (uint32_t *)R.nrows.p;
    g.row_offsets = (const unsigned long long *)R.row_offsets.p;
    launch_group_order(g, st);
    NbArgs scan = l.a;  // (the neighbour run has read its parts and its info)
    scan.counts = g.n_rows;
    scan.offsets = (unsigned long long *)R.row_offsets.p;
    launch_neighbor_scan(scan, st);
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, download(out_offsets, g.row_offsets, (N + 1) * 8, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    const uint64_t n_rows = out_offsets[N];
    if (!out_groups || !out_buried || !out_only || cap < n_rows)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "a row buffer is NULL or holds fewer rows than out_offsets[n]");
    if ((n_rows && ((rc = reserve(ctx, R.groups, n_rows * 4)) || (rc = reserve(ctx, R.buried, n_rows * 4)) ||
                    (rc = reserve(ctx, R.only, n_rows * 4)))) ||
        (rc = reserve(ctx, R.self_free, N * 4)) || (rc = reserve(ctx, R.free, N * 4)))
        return rc;
    g.groups = (uint32_t *)R.groups.p;
    g.buried = (uint32_t *)R.buried.p;
    g.only = (uint32_t *)R.only.p;
    g.self_free = (uint32_t *)R.self_free.p;
    g.free = (uint32_t *)R.free.p;
    launch_group_points(g, st);
    RS_HIP(ctx, hipGetLastError());
    if (n_rows) {
        RS_HIP(ctx, download(out_groups, g.groups, n_rows * 4, st));
        RS_HIP(ctx, download(out_buried, g.buried, n_rows * 4, st));
        RS_HIP(ctx, download(out_only, g.only, n_rows * 4, st));
    }
    RS_HIP(ctx, download(out_self_free, g.self_free, N * 4, st));
    RS_HIP(ctx, download(out_free, g.free, N * 4, st));
    RS_HIP(ctx, download(out_sasa, g.p.sasa, N * 4, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    return RSASA_OK;
}

// ---- half-sphere exposure (rsasa_half_sphere_exposure*) and atoms within a cutoff (rsasa_atoms_within*) ----

// The opening of a run on the grid alone: the grid into h.b (nb_grid with every structure's own largest radius:
// max_r = NaN), then the flag bytes (flags: host, [N], nullable) beside it: uploaded, with room for their cell-sorted copy;
// k_sort_flags (launch_half_sphere, launch_sort_flags) then writes h.sorted_flags.
int hs_grid(rsasa_context *ctx, const Cols &c, const uint32_t *idx_map, float probe, const uint8_t *flags, HsArgs &h)
{
    int rc;
    rsasa_context::RunScratch &R = ctx->run;
    const size_t N = c.N;
    if ((rc = nb_grid(ctx, c, idx_map, probe, __builtin_nanf(""), h.b)) || (flags && (rc = reserve(ctx, R.flags, N))) ||
        (rc = reserve(ctx, R.sorted_flags, N)))
        return rc;
    if (flags) RS_HIP(ctx, hipMemcpyAsync(R.flags.p, flags, N, hipMemcpyHostToDevice, ctx->stream));
    h.flags = flags ? (const uint8_t *)R.flags.p : nullptr;
    h.sorted_flags = (uint8_t *)R.sorted_flags.p;
    return RSASA_OK;
}

// One run of the half-sphere counts: the grid alone (hs_grid: no counting pass, no lists) with the flags, the directions
// beside them (their buffer is reserved behind the flags', which hs_grid reserves), k_sort_flags and k_half_sphere; 8 bytes
// per atom come back.
int hs_run(rsasa_context *ctx, const Cols &c, float probe, const float *dirs, const uint8_t *flags, float cutoff,
           uint32_t *out_up, uint32_t *out_down)
{
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    if (c.N == 0) return RSASA_OK;
    int rc;
    rsasa_context::RunScratch &R = ctx->run;
    hipStream_t st = ctx->stream;
    const size_t N = c.N;
    HsArgs h{};
    if ((rc = hs_grid(ctx, c, nullptr, probe, flags, h)) || (dirs && (rc = reserve(ctx, R.dirs, N * 12))) ||
        (rc = reserve(ctx, R.up, N * 4)) || (rc = reserve(ctx, R.down, N * 4)))
        return rc;
    if (dirs) RS_HIP(ctx, hipMemcpyAsync(R.dirs.p, dirs, N * 12, hipMemcpyHostToDevice, st));
    h.dirs = dirs ? (const float *)R.dirs.p : nullptr;
    h.cutoff = cutoff;
    h.up = (uint32_t *)R.up.p;
    h.down = (uint32_t *)R.down.p;
    launch_half_sphere(h, st);
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, download(out_up, h.up, N * 4, st));
    RS_HIP(ctx, download(out_down, h.down, N * 4, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    return RSASA_OK;
}

// One run of the lists within a cutoff: the grid alone and the flags as in hs_run, k_within_count and the neighbour
// runs' scan, the sizing rule of nb_run, then k_within_fill (and the ranking of the long lists) and 8 bytes per entry back.
int wn_run(rsasa_context *ctx, const Cols &c, float probe, const uint8_t *flags, float cutoff, int upper_only,
           uint64_t *out_offsets, rsasa_within_t *out_entries, size_t cap)
{
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    if (c.N == 0) {
        out_offsets[0] = 0;
        return RSASA_OK;
    }
    int rc;
    hipStream_t st = ctx->stream;
    HsArgs h{};
    WnArgs w{};
    NbInfo info{};
    if ((rc = hs_grid(ctx, c, nullptr, probe, flags, h))) return rc;
    w.n.b = h.b;
    if ((rc = nb_scan_buffers(ctx, c.N, within_stage_capacity(), w.n))) return rc;
    w.sorted_flags = h.sorted_flags;
    w.cutoff = cutoff;
    w.upper_only = upper_only ? 1u : 0u;
    launch_sort_flags(h, st);
    launch_within_count(w, st);
    if ((rc = nb_sizes(ctx, w.n, c.N, out_offsets, info))) return rc;
    if (!out_entries || cap < info.total)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "out_entries is NULL or holds fewer entries than out_offsets[n]");
    if (info.total == 0) return RSASA_OK;
    if ((rc = nb_fill_by(ctx, w.n, info, [&](uint64_t spill_atoms) { launch_within_fill(w, spill_atoms, st); }))) return rc;
    RS_HIP(ctx, hipMemcpyAsync(out_entries, w.n.out, info.total * 8, hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    return RSASA_OK;
}

// One run of the k nearest atoms: the grid alone and the flags as in wn_run, with the centres' ranks (a host prefix over
// the flag bytes: which row a centre's keys go to) uploaded beside the columns; k_nearest sweeps once and leaves rows and
// counts, the neighbour runs' scan and the sizing rule of nb_run follow, then k_nearest_gather and 8 bytes per entry back.
int nn_run(rsasa_context *ctx, const Cols &c, float probe, const uint8_t *flags, uint32_t k, float cutoff,
           uint64_t *out_offsets, rsasa_within_t *out_entries, size_t cap)
{
    static_assert(kNearestMaxK == RSASA_NEAREST_MAX_K, "the header's bound is the kernels' bound");
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    if (c.N == 0) {
        out_offsets[0] = 0;
        return RSASA_OK;
    }
    int rc;
    rsasa_context::RunScratch &R = ctx->run;
    hipStream_t st = ctx->stream;
    NbHost *nh;
    HsArgs h{};
    NnArgs nn{};
    NbInfo info{};
    std::vector<uint32_t> rank;
    size_t rows = c.N;
    if (flags) {
        rank.resize(c.N);
        rows = 0;
        for (size_t i = 0; i < c.N; i++) {
            rank[i] = (uint32_t)rows;
            rows += (flags[i] >> 1) & 1u;
        }
    }
    if ((rc = hs_grid(ctx, c, flags ? rank.data() : nullptr, probe, flags, h)) || (rc = reserve(ctx, R.rows, rows * k * 8)))
        return rc;
    nn.w.n.b = h.b;
    if ((rc = nb_scan_buffers(ctx, c.N, k, nn.w.n))) return rc;  // (stage = k: no list is longer)
    nn.w.sorted_flags = h.sorted_flags;
    nn.w.cutoff = cutoff;
    nn.w.upper_only = 0u;
    nn.k = k;
    nn.rank = flags ? (const uint32_t *)R.map.p : nullptr;
    nn.rows = (unsigned long long *)R.rows.p;
    launch_sort_flags(h, st);
    launch_nearest(nn, st);
    if ((rc = nb_sizes(ctx, nn.w.n, c.N, out_offsets, info))) return rc;
    if (!out_entries || cap < info.total)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "out_entries is NULL or holds fewer entries than out_offsets[n]");
    if (info.total == 0) return RSASA_OK;
    if (info.max_k > k || info.spill_atoms) return fail(ctx, RSASA_ERR_INTERNAL, "a list of the k nearest atoms is longer than k");
    if ((rc = reserve(ctx, R.entries, info.total * 8))) return rc;
    nn.w.n.out = (uint2 *)R.entries.p;
    launch_nearest_gather(nn, st);
    nh = static_cast<NbHost *>(ctx->nb_host.p);
    RS_HIP(ctx, hipMemcpyAsync(&nh->info, nn.w.n.info, sizeof(NbInfo), hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipMemcpyAsync(out_entries, nn.w.n.out, info.total * 8, hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, hipStreamSynchronize(st));
    if (nh->info.mismatch) return fail(ctx, RSASA_ERR_INTERNAL, "the rows of the k nearest atoms disagree with their counts");
    return RSASA_OK;
}

// One run of the radial counts: the grid alone and the flags as in hs_run, the class bytes and the structures' offsets
// beside them, the dense table of rows ([N][n_classes][n_bins] uint32: held on the device even when only the pair
// tables are asked for - k_radial_pairs sums its rows) and, when asked for, the pair tables, zeroed on the stream;
// k_sort_kinds, k_radial_counts and k_radial_pairs; what was asked for comes back.  check_radial and check_classes have
// passed.
int rd_run(rsasa_context *ctx, const Cols &c, float probe, const uint8_t *flags, const uint8_t *classes, uint32_t n_classes,
           const float *edges, uint32_t n_bins, uint32_t *out_counts, uint64_t *out_pairs)
{
    static_assert(kRadialMaxClasses == RSASA_RADIAL_MAX_CLASSES && kRadialMaxBins == RSASA_RADIAL_MAX_BINS,
                  "the header's bounds are the kernels' bounds");
    static_assert(sizeof(RdArgs::e2) == kRadialMaxBins * sizeof(float), "an edge per bin");
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    const size_t N = c.N, cells = (size_t)n_classes * n_bins, pair_bytes = c.S * n_classes * cells * 8;
    if (N == 0) {
        if (out_pairs) std::memset(out_pairs, 0, pair_bytes);
        return RSASA_OK;
    }
    int rc;
    rsasa_context::RunScratch &R = ctx->run;
    hipStream_t st = ctx->stream;
    HsArgs h{};
    RdArgs r{};
    if ((rc = hs_grid(ctx, c, nullptr, probe, flags, h)) || (classes && (rc = reserve(ctx, R.classes, N))) ||
        (rc = reserve(ctx, R.so, (c.S + 1) * 4)) || (rc = reserve(ctx, R.table, N * cells * 4)) ||
        (out_pairs && (rc = reserve(ctx, R.pairs, pair_bytes))))
        return rc;
    if (classes) RS_HIP(ctx, hipMemcpyAsync(R.classes.p, classes, N, hipMemcpyHostToDevice, st));
    RS_HIP(ctx, hipMemcpyAsync(R.so.p, c.so, (c.S + 1) * 4, hipMemcpyHostToDevice, st));
    if (out_pairs) RS_HIP(ctx, hipMemsetAsync(R.pairs.p, 0, pair_bytes, st));
    r.b = h.b;
    r.flags = h.flags;
    r.classes = classes ? (const uint8_t *)R.classes.p : nullptr;
    r.sorted_kinds = h.sorted_flags;
    r.so = (const uint32_t *)R.so.p;
    r.n_classes = n_classes;
    r.n_bins = n_bins;
    for (uint32_t k = 0; k < n_bins; k++) r.e2[k] = edges[k] * edges[k];
    r.table = (uint32_t *)R.table.p;
    r.pairs = out_pairs ? (unsigned long long *)R.pairs.p : nullptr;
    launch_radial(r, st);
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, download(out_counts, r.table, N * cells * 4, st));
    RS_HIP(ctx, download(out_pairs, r.pairs, pair_bytes, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
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
    RS_ARGS(ctx, check_columns(n_atoms, x, y, z, radius, out_offsets && (!n_active || active_indices)));
    if (n >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 atoms");
    if (!active_indices)
        return nb_run(ctx, Cols(x, y, z, radius, id, n_atoms), nullptr, probe_radius, max_radius, out_offsets, out_entries,
                      entries_capacity);
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
    return nb_run(ctx, Cols(gx.data(), gy.data(), gz.data(), gr.data(), id ? gid.data() : nullptr, n), active_indices,
                  probe_radius, max_radius, out_offsets, out_entries, entries_capacity);
}

int rsasa_precompute_neighbors_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                                     const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                                     float probe_radius, float max_radius, uint64_t *out_offsets, rsasa_neighbor_t *out_entries,
                                     size_t entries_capacity)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    size_t N;
    RS_ARGS(ctx, check_offsets(structure_offsets, n_structures, N));
    RS_ARGS(ctx, check_columns(N, x, y, z, radius, out_offsets));
    return nb_run(ctx, Cols(x, y, z, radius, id, structure_offsets, n_structures, N), nullptr, probe_radius, max_radius,
                  out_offsets, out_entries, entries_capacity);
}

int rsasa_accessible_points(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                            const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, uint32_t *out_masks,
                            float *out_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    RS_ARGS(ctx, check_points(n_atoms, x, y, z, radius, !n_atoms || out_masks, n_points));
    return pt_run(ctx, Cols(x, y, z, radius, id, n_atoms), probe_radius, n_points, out_masks, out_sasa);
}

int rsasa_accessible_points_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                                  const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                                  float probe_radius, size_t n_points, uint32_t *out_masks, float *out_atom_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    size_t N;
    RS_ARGS(ctx, check_offsets(structure_offsets, n_structures, N));
    RS_ARGS(ctx, check_points(N, x, y, z, radius, !N || out_masks, n_points));
    return pt_run(ctx, Cols(x, y, z, radius, id, structure_offsets, n_structures, N), probe_radius, n_points, out_masks,
                  out_atom_sasa);
}

int rsasa_exposure_vectors(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                           const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, float *out_vectors,
                           uint32_t *out_free, float *out_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    RS_ARGS(ctx, check_points(n_atoms, x, y, z, radius, !n_atoms || (out_vectors && out_free), n_points));
    return ex_run(ctx, Cols(x, y, z, radius, id, n_atoms), probe_radius, n_points, out_vectors, out_free, out_sasa);
}

int rsasa_exposure_vectors_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                                 const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                                 float probe_radius, size_t n_points, float *out_vectors, uint32_t *out_free,
                                 float *out_atom_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    size_t N;
    RS_ARGS(ctx, check_offsets(structure_offsets, n_structures, N));
    RS_ARGS(ctx, check_points(N, x, y, z, radius, !N || (out_vectors && out_free), n_points));
    return ex_run(ctx, Cols(x, y, z, radius, id, structure_offsets, n_structures, N), probe_radius, n_points, out_vectors,
                  out_free, out_atom_sasa);
}

int rsasa_atom_depth(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                     const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, float *out_depth,
                     uint32_t *out_nearest, uint32_t *out_free, float *out_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    RS_ARGS(ctx, check_points(n_atoms, x, y, z, radius, !n_atoms || (out_depth && out_nearest), n_points));
    return dp_run(ctx, Cols(x, y, z, radius, id, n_atoms), probe_radius, n_points, out_depth, out_nearest, out_free, out_sasa);
}

int rsasa_atom_depth_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                           const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                           size_t n_points, float *out_depth, uint32_t *out_nearest, uint32_t *out_free, float *out_atom_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    size_t N;
    RS_ARGS(ctx, check_offsets(structure_offsets, n_structures, N));
    RS_ARGS(ctx, check_points(N, x, y, z, radius, !N || (out_depth && out_nearest), n_points));
    return dp_run(ctx, Cols(x, y, z, radius, id, structure_offsets, n_structures, N), probe_radius, n_points, out_depth,
                  out_nearest, out_free, out_atom_sasa);
}

int rsasa_surface_components(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                             const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, float link,
                             uint64_t *out_dot_offsets, uint32_t *out_labels, size_t labels_capacity, uint32_t *out_free,
                             float *out_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    RS_ARGS(ctx, check_points(n_atoms, x, y, z, radius, out_dot_offsets, n_points));
    RS_ARGS(ctx, check_link(link));
    return cc_run(ctx, Cols(x, y, z, radius, id, n_atoms), probe_radius, n_points, link, out_dot_offsets, out_labels,
                  labels_capacity, out_free, out_sasa);
}

int rsasa_surface_components_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                                   const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                                   float probe_radius, size_t n_points, float link, uint64_t *out_dot_offsets,
                                   uint32_t *out_labels, size_t labels_capacity, uint32_t *out_free, float *out_atom_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    size_t N;
    RS_ARGS(ctx, check_offsets(structure_offsets, n_structures, N));
    RS_ARGS(ctx, check_points(N, x, y, z, radius, out_dot_offsets, n_points));
    RS_ARGS(ctx, check_link(link));
    return cc_run(ctx, Cols(x, y, z, radius, id, structure_offsets, n_structures, N), probe_radius, n_points, link,
                  out_dot_offsets, out_labels, labels_capacity, out_free, out_atom_sasa);
}

int rsasa_dot_crowding(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                       const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, const uint8_t *flags,
                       const float *edges, uint32_t n_bins, uint64_t *out_dot_offsets, uint32_t *out_counts,
                       size_t counts_capacity, uint32_t *out_free, float *out_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    RS_ARGS(ctx, check_points(n_atoms, x, y, z, radius, out_dot_offsets, n_points));
    RS_ARGS(ctx, check_crowding(edges, n_bins));
    return dc_run(ctx, Cols(x, y, z, radius, id, n_atoms), probe_radius, n_points, flags, edges, n_bins, out_dot_offsets,
                  out_counts, counts_capacity, out_free, out_sasa);
}

int rsasa_dot_crowding_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                             const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                             size_t n_points, const uint8_t *flags, const float *edges, uint32_t n_bins,
                             uint64_t *out_dot_offsets, uint32_t *out_counts, size_t counts_capacity, uint32_t *out_free,
                             float *out_atom_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    size_t N;
    RS_ARGS(ctx, check_offsets(structure_offsets, n_structures, N));
    RS_ARGS(ctx, check_points(N, x, y, z, radius, out_dot_offsets, n_points));
    RS_ARGS(ctx, check_crowding(edges, n_bins));
    return dc_run(ctx, Cols(x, y, z, radius, id, structure_offsets, n_structures, N), probe_radius, n_points, flags, edges,
                  n_bins, out_dot_offsets, out_counts, counts_capacity, out_free, out_atom_sasa);
}

int rsasa_half_sphere_exposure(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                               const uint64_t *id, size_t n_atoms, float probe_radius, const float *dirs, const uint8_t *flags,
                               float cutoff, uint32_t *out_up, uint32_t *out_down)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    RS_ARGS(ctx, check_columns(n_atoms, x, y, z, radius, !n_atoms || (out_up && out_down)));
    RS_ARGS(ctx, check_cutoff(cutoff));
    return hs_run(ctx, Cols(x, y, z, radius, id, n_atoms), probe_radius, dirs, flags, cutoff, out_up, out_down);
}

int rsasa_half_sphere_exposure_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                                     const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                                     float probe_radius, const float *dirs, const uint8_t *flags, float cutoff,
                                     uint32_t *out_up, uint32_t *out_down)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    size_t N;
    RS_ARGS(ctx, check_offsets(structure_offsets, n_structures, N));
    RS_ARGS(ctx, check_columns(N, x, y, z, radius, !N || (out_up && out_down)));
    RS_ARGS(ctx, check_cutoff(cutoff));
    return hs_run(ctx, Cols(x, y, z, radius, id, structure_offsets, n_structures, N), probe_radius, dirs, flags, cutoff,
                  out_up, out_down);
}

int rsasa_atoms_within(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                       const uint64_t *id, size_t n_atoms, float probe_radius, const uint8_t *flags, float cutoff,
                       int upper_only, uint64_t *out_offsets, rsasa_within_t *out_entries, size_t entries_capacity)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    RS_ARGS(ctx, check_columns(n_atoms, x, y, z, radius, out_offsets));
    RS_ARGS(ctx, check_cutoff(cutoff));
    return wn_run(ctx, Cols(x, y, z, radius, id, n_atoms), probe_radius, flags, cutoff, upper_only, out_offsets, out_entries,
                  entries_capacity);
}

int rsasa_atoms_within_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                             const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                             const uint8_t *flags, float cutoff, int upper_only, uint64_t *out_offsets,
                             rsasa_within_t *out_entries, size_t entries_capacity)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    size_t N;
    RS_ARGS(ctx, check_offsets(structure_offsets, n_structures, N));
    RS_ARGS(ctx, check_columns(N, x, y, z, radius, out_offsets));
    RS_ARGS(ctx, check_cutoff(cutoff));
    return wn_run(ctx, Cols(x, y, z, radius, id, structure_offsets, n_structures, N), probe_radius, flags, cutoff,
                  upper_only, out_offsets, out_entries, entries_capacity);
}

int rsasa_nearest_atoms(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                        const uint64_t *id, size_t n_atoms, float probe_radius, const uint8_t *flags, uint32_t k, float cutoff,
                        uint64_t *out_offsets, rsasa_within_t *out_entries, size_t entries_capacity)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    RS_ARGS(ctx, check_columns(n_atoms, x, y, z, radius, out_offsets));
    RS_ARGS(ctx, check_nearest_k(k));
    RS_ARGS(ctx, check_nearest_cutoff(cutoff));
    return nn_run(ctx, Cols(x, y, z, radius, id, n_atoms), probe_radius, flags, k, cutoff, out_offsets, out_entries,
                  entries_capacity);
}

int rsasa_nearest_atoms_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                              const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                              const uint8_t *flags, uint32_t k, float cutoff, uint64_t *out_offsets,
                              rsasa_within_t *out_entries, size_t entries_capacity)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    size_t N;
    RS_ARGS(ctx, check_offsets(structure_offsets, n_structures, N));
    RS_ARGS(ctx, check_columns(N, x, y, z, radius, out_offsets));
    RS_ARGS(ctx, check_nearest_k(k));
    RS_ARGS(ctx, check_nearest_cutoff(cutoff));
    return nn_run(ctx, Cols(x, y, z, radius, id, structure_offsets, n_structures, N), probe_radius, flags, k, cutoff,
                  out_offsets, out_entries, entries_capacity);
}

int rsasa_radial_counts(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                        const uint64_t *id, size_t n_atoms, float probe_radius, const uint8_t *flags, const uint8_t *classes,
                        uint32_t n_classes, const float *edges, uint32_t n_bins, uint32_t *out_counts, uint64_t *out_pairs)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    RS_ARGS(ctx, check_columns(n_atoms, x, y, z, radius, !n_atoms || out_counts || out_pairs));
    RS_ARGS(ctx, check_radial(edges, n_bins, n_classes));
    RS_ARGS(ctx, check_classes(classes, n_atoms, n_classes));
    return rd_run(ctx, Cols(x, y, z, radius, id, n_atoms), probe_radius, flags, classes, n_classes, edges, n_bins, out_counts,
                  out_pairs);
}

int rsasa_radial_counts_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                              const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                              const uint8_t *flags, const uint8_t *classes, uint32_t n_classes, const float *edges,
                              uint32_t n_bins, uint32_t *out_counts, uint64_t *out_pairs)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    size_t N;
    RS_ARGS(ctx, check_offsets(structure_offsets, n_structures, N));
    RS_ARGS(ctx, check_columns(N, x, y, z, radius, !N || out_counts || out_pairs));
    RS_ARGS(ctx, check_radial(edges, n_bins, n_classes));
    RS_ARGS(ctx, check_classes(classes, N, n_classes));
    return rd_run(ctx, Cols(x, y, z, radius, id, structure_offsets, n_structures, N), probe_radius, flags, classes, n_classes,
                  edges, n_bins, out_counts, out_pairs);
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
    RS_ARGS(ctx, check_points(n_atoms, x, y, z, radius, out_offsets, n_points));
    return ct_run(ctx, Cols(x, y, z, radius, id, n_atoms), probe_radius, n_points, out_offsets, out_entries, out_covered,
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
    size_t N;
    RS_ARGS(ctx, check_offsets(structure_offsets, n_structures, N));
    RS_ARGS(ctx, check_points(N, x, y, z, radius, out_offsets, n_points));
    return ct_run(ctx, Cols(x, y, z, radius, id, structure_offsets, n_structures, N), probe_radius, n_points, out_offsets,
                  out_entries, out_covered, out_exclusive, entries_capacity, out_atom_sasa);
}

int rsasa_contact_owners(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                         const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, uint64_t *out_offsets,
                         rsasa_neighbor_t *out_entries, uint32_t *out_owned, size_t entries_capacity, uint32_t *out_owner,
                         float *out_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    RS_ARGS(ctx, check_points(n_atoms, x, y, z, radius, out_offsets, n_points));
    return co_run(ctx, Cols(x, y, z, radius, id, n_atoms), probe_radius, n_points, out_offsets, out_entries, out_owned,
                  entries_capacity, out_owner, out_sasa);
}

int rsasa_contact_owners_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                               const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                               float probe_radius, size_t n_points, uint64_t *out_offsets, rsasa_neighbor_t *out_entries,
                               uint32_t *out_owned, size_t entries_capacity, uint32_t *out_owner, float *out_atom_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    size_t N;
    RS_ARGS(ctx, check_offsets(structure_offsets, n_structures, N));
    RS_ARGS(ctx, check_points(N, x, y, z, radius, out_offsets, n_points));
    return co_run(ctx, Cols(x, y, z, radius, id, structure_offsets, n_structures, N), probe_radius, n_points, out_offsets,
                  out_entries, out_owned, entries_capacity, out_owner, out_atom_sasa);
}

int rsasa_group_contacts(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                         const uint64_t *id, const uint32_t *group, size_t n_atoms, float probe_radius, size_t n_points,
                         uint64_t *out_offsets, uint32_t *out_groups, uint32_t *out_buried, uint32_t *out_only,
                         size_t rows_capacity, uint32_t *out_self_free, uint32_t *out_free, float *out_sasa)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    RS_ARGS(ctx, check_points(n_atoms, x, y, z, radius, out_offsets && (!n_atoms || (group && out_self_free && out_free)),
                              n_points));
    return gp_run(ctx, Cols(x, y, z, radius, id, n_atoms), group, probe_radius, n_points, out_offsets, out_groups, out_buried,
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
    size_t N;
    RS_ARGS(ctx, check_offsets(structure_offsets, n_structures, N));
    RS_ARGS(ctx, check_points(N, x, y, z, radius, out_offsets && (!N || (group && out_self_free && out_free)), n_points));
    return gp_run(ctx, Cols(x, y, z, radius, id, structure_offsets, n_structures, N), group, probe_radius, n_points,
                  out_offsets, out_groups, out_buried, out_only, rows_capacity, out_self_free, out_free, out_atom_sasa);
}

}  // extern "C"
