// Host side of the nineteen families that run on a grid of the context's own (rsasa_context::nb_ws), each a single /
// batch pair of include/rustsasa_amd.h: the neighbour lists (rsasa_precompute_neighbors*); the point runs built on
// them - accessible points, exposure vectors, atom depth, surface components, dot links, dot geodesics, dot patches, dot crowding,
// dot fields, dot curvature, dot enclosure, contact counts, contact owners, group contacts; and the runs on the grid alone - half-sphere exposure, atoms within a cutoff, the k nearest
// atoms, radial counts.  The grid is built by the SASA path's kernels (nb_grid, and hs_grid for the runs on the grid
// alone), then neighbors.hip counts, scans and fills the lists (nb_count, nb_fill).  A point run keeps the lists on the
// device: every family shares one prologue (pt_count, pt_prepare: lists with the SASA path's cutoff, lattice, PtArgs) and
// adds its own kernels of points.hip, depth.hip, components.hip, geodesics.hip, patches.hip, crowding.hip, fields.hip, curvature.hip or enclosure.hip and its
// own downloads.
// Every family is one function (*_run) behind its two entry points, which only forward to it: the single form as
// Form::one(n_atoms), the batch form as Form::many(structure_offsets, n_structures).  The function opens with the rules
// - entry_open: the context, N and the Cols (entry_checks.h: Cols::fix), n_points, the columns; then the family's own -
// and goes on under a Run, the frame that holds the context's mutex and device and hands out the scratch.  Only the
// neighbour lists have the two apart (nb_entry, nb_run): the single form may run on a gathered copy of its columns.
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

// The opening of every family's function, in the order of the verdicts: the context; N and the Cols (the offsets rule
// of a batch); n_points (point families; null: the family has none); the columns.  always: the arrays the call cannot
// do without whatever N is; per_atom: those with an entry per atom, which may all be NULL when N is 0, as the columns may.
int entry_open(rsasa_context *&ctx, Cols &c, const Form &f, const size_t *n_points, bool always, bool per_atom)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    RS_ARGS(ctx, c.fix(f));
    const bool rest = always && (!c.N || per_atom);
    RS_ARGS(ctx, n_points ? check_points(c.N, c.x, c.y, c.z, c.r, rest, *n_points)
                          : check_columns(c.N, c.x, c.y, c.z, c.r, rest));
    return RSASA_OK;
}

// The frame of a run function: for its lifetime the calling thread holds the context's mutex and the context's device is
// current.  open() is the first step of every run.  R is the scratch of these calls (rsasa_context::RunScratch) and st
// the stream they queue on.
struct Run {
    std::lock_guard<std::recursive_mutex> lk;
    DeviceGuard dev;
    rsasa_context *const ctx;
    rsasa_context::RunScratch &R;
    const hipStream_t st;
    int rc = RSASA_OK;
    explicit Run(rsasa_context *c) : lk(c->mu), dev(c->device), ctx(c), R(c->run), st(c->stream) {}
    // Whether the run goes on.  If not, rc is its answer: the device could not be made current, or there is no atom - then
    // out_offsets (null: the family has none) describes N = 0 lists.
    bool open(size_t N, uint64_t *out_offsets = nullptr)
    {
        if (dev.err != hipSuccess) rc = fail(ctx, RSASA_ERR_HIP, "hipSetDevice", dev.err);
        else if (N == 0 && out_offsets) out_offsets[0] = 0;
        return rc == RSASA_OK && N != 0;
    }
    // `bytes` of b (contents are not kept; none asked for: b stays as it is), and where they are.
    template <class T>
    int reserve(DeviceBuffer &b, size_t bytes, T *&p)
    {
        const int verdict = rsasa::reserve(ctx, b, bytes);
        p = (T *)b.p;
        return verdict;
    }
    // Queues the copy of `bytes` from a host array that the caller may have left out into b; p: where they are on the
    // device, or null.
    template <class T>
    int upload(DeviceBuffer &b, const T *host, size_t bytes, const T *&p)
    {
        p = nullptr;
        if (!host) return RSASA_OK;
        if (int verdict = reserve(b, bytes, p)) return verdict;
        RS_HIP(ctx, hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, st));
        return RSASA_OK;
    }
};

// Queues the copy of `bytes` from the device into a host array that the caller may have left out.
hipError_t download(void *out, const void *from, size_t bytes, hipStream_t st)
{
    return out ? hipMemcpyAsync(out, from, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
}

struct NbHost {  // the pinned block the device's verdicts come back in
    BatchStatus status;
    NbInfo info;
    uint64_t last_offset;  // offsets[N], when the caller wants no host copy of the offsets
};

// The upload and the grid of a run over columns already in host memory: c.N >= 1 atoms.  idx_map (host, nullable) is
// uploaded beside the columns (RunScratch::map).  On RSASA_OK `v` describes the binned batch.
int nb_grid(Run &f, const Cols &c, const uint32_t *idx_map, float probe, float max_r, BatchView &v)
{
    int rc;
    rsasa_context *ctx = f.ctx;
    rsasa_context::Workspace &W = ctx->nb_ws;
    const size_t N = c.N;

    const SegmentCount sc = count_segments(c.so, c.S);
    std::vector<Segment> segs(sc.n_seg);
    write_segments(c.so, c.S, segs.data(), nullptr);
    const bool has_tail = sc.has_tail;
    const bool has_id = c.id != nullptr;
    if (!ctx->nb_host.p) RS_HIP(ctx, ctx->nb_host.regrow(sizeof(NbHost)));
    NbHost *h = static_cast<NbHost *>(ctx->nb_host.p);

    const float *x, *y, *z, *r;
    const uint64_t *id;
    const uint32_t *map;  // (who reads it takes it from RunScratch::map)
    if ((rc = f.upload(f.R.x, c.x, N * 4, x)) || (rc = f.upload(f.R.y, c.y, N * 4, y)) || (rc = f.upload(f.R.z, c.z, N * 4, z)) ||
        (rc = f.upload(f.R.r, c.r, N * 4, r)) || (rc = f.upload(f.R.id, c.id, N * 8, id)) ||
        (rc = f.upload(f.R.map, idx_map, N * 4, map)))
        return rc;

    // ---- the grid (without the id check: every id takes part), grown until the cells fit
    for (int attempt = 0;; attempt++) {
        if ((rc = W.reserve_grid(ctx, N, c.S, segs.size(), ctx->nb_cell_capacity, has_tail, has_id))) return rc;
        if (!segs.empty())
            RS_HIP(ctx, hipMemcpyAsync(W.segments.p, segs.data(), segs.size() * sizeof(Segment), hipMemcpyHostToDevice, f.st));
        v = BatchView{};
        v.x = x; v.y = y; v.z = z;
        v.radius = r;
        v.id = id;
        v.n_atoms = (uint32_t)N; v.n_structures = (uint32_t)c.S; v.n_segments = (uint32_t)segs.size();
        v.probe = probe;
        v.max_r_override = max_r;
        W.grid_view(v);
        launch_grid_prepare(v, f.st);
        launch_sort_lds(v, f.st);
        if (has_tail) launch_sort_tail(v, f.st);
        RS_HIP(ctx, hipMemcpyAsync(&h->status, W.status.p, sizeof(BatchStatus), hipMemcpyDeviceToHost, f.st));
        RS_HIP(ctx, hipGetLastError());
        RS_HIP(ctx, hipStreamSynchronize(f.st));
        if ((rc = grid_verdict(ctx, h->status, attempt, ctx->nb_cell_capacity)) == RSASA_OK) break;
        if (rc != kGridAgain) return rc;
    }
    return RSASA_OK;
}

// The buffers a count pass and its scan write (counts, offsets, parts, a cleared NbInfo) for the N atoms of a.b, and
// the length above which the run's fill kernel takes a list for long.
int nb_scan_buffers(Run &f, size_t N, uint32_t stage, NbArgs &a)
{
    int rc;
    if ((rc = f.reserve(f.R.counts, N * 4, a.counts)) || (rc = f.reserve(f.R.offsets, (N + 1) * 8, a.offsets)) ||
        (rc = f.reserve(f.R.parts, 4 * 1024 * 8, a.parts)) || (rc = f.reserve(f.R.info, sizeof(NbInfo), a.info)))
        return rc;
    a.stage = stage;
    RS_HIP(f.ctx, hipMemsetAsync(a.info, 0, sizeof(NbInfo), f.st));
    return RSASA_OK;
}

// What a queued count pass and scan found: waits for them; `info` gets the lists' sizes and out_offsets (nullable:
// [N + 1]) the offsets.
int nb_sizes(Run &f, const NbArgs &a, size_t N, uint64_t *out_offsets, NbInfo &info)
{
    NbHost *h = static_cast<NbHost *>(f.ctx->nb_host.p);
    RS_HIP(f.ctx, hipMemcpyAsync(&h->info, a.info, sizeof(NbInfo), hipMemcpyDeviceToHost, f.st));
    if (out_offsets) RS_HIP(f.ctx, hipMemcpyAsync(out_offsets, a.offsets, (N + 1) * 8, hipMemcpyDeviceToHost, f.st));
    else RS_HIP(f.ctx, hipMemcpyAsync(&h->last_offset, a.offsets + N, 8, hipMemcpyDeviceToHost, f.st));
    RS_HIP(f.ctx, hipGetLastError());
    RS_HIP(f.ctx, hipStreamSynchronize(f.st));
    info = h->info;
    if (info.total != (out_offsets ? out_offsets[N] : h->last_offset))
        return fail(f.ctx, RSASA_ERR_INTERNAL, "list offsets disagree with their total");
    return RSASA_OK;
}

// nb_grid, and the counts of the lists on that grid.  idx_map: input atom -> the index written to the entries.
// out_offsets (nullable): [N + 1], the offsets are copied there.  On RSASA_OK `a` describes the device lists (everything
// but their entries) and `info` their sizes.
int nb_count(Run &f, const Cols &c, const uint32_t *idx_map, float probe, float max_r, uint64_t *out_offsets, NbArgs &a,
             NbInfo &info)
{
    int rc;
    a = NbArgs{};
    if ((rc = nb_grid(f, c, idx_map, probe, max_r, a.b)) || (rc = nb_scan_buffers(f, c.N, neighbor_stage_capacity(), a)))
        return rc;
    a.idx_map = idx_map ? (const uint32_t *)f.R.map.p : nullptr;
    launch_neighbor_count(a, f.st);
    return nb_sizes(f, a, c.N, out_offsets, info);
}

// The entries of the lists a count pass sized (info.total >= 1), sorted, in a.out on the device: reserves them and the
// long lists' scratch, runs `launch(info.spill_atoms)` - the family's fill kernels over `a` - and checks that the fill
// pass agreed with the count pass.
template <class Launch>
int nb_fill_by(Run &f, NbArgs &a, const NbInfo &info, Launch launch)
{
    int rc;
    NbHost *h = static_cast<NbHost *>(f.ctx->nb_host.p);
    if ((rc = f.reserve(f.R.entries, info.total * 8, a.out)) ||
        (info.spill_atoms && ((rc = f.reserve(f.R.spill, info.spill_entries * sizeof(NbKey), a.spill)) ||
                              (rc = f.reserve(f.R.recs, info.spill_atoms * sizeof(NbSpillRec), a.spill_recs)))))
        return rc;
    launch(info.spill_atoms);
    RS_HIP(f.ctx, hipMemcpyAsync(&h->info, a.info, sizeof(NbInfo), hipMemcpyDeviceToHost, f.st));
    RS_HIP(f.ctx, hipGetLastError());
    RS_HIP(f.ctx, hipStreamSynchronize(f.st));
    if (h->info.mismatch || h->info.spill_cursor != info.spill_entries || h->info.spill_recs != info.spill_atoms)
        return fail(f.ctx, RSASA_ERR_INTERNAL, "the fill pass of the lists disagrees with its count pass");
    return RSASA_OK;
}

// The entries of the lists nb_count sized (info.total >= 1).
int nb_fill(Run &f, NbArgs &a, const NbInfo &info)
{
    return nb_fill_by(f, a, info, [&](uint64_t spill_atoms) { launch_neighbor_fill(a, spill_atoms, f.st); });
}

// The end of a run that hands sized lists back, once the caller has their offsets: out_entries (cap entries) is
// checked against info.total - too_small is the family's message - then, unless every list is empty, nb_fill_by fills
// the lists and 8 bytes per entry come back.
template <class Launch>
int nb_entries_out(Run &f, NbArgs &a, const NbInfo &info, void *out_entries, size_t cap, const char *too_small, Launch launch)
{
    if (!out_entries || cap < info.total) return fail(f.ctx, RSASA_ERR_BUFFER_TOO_SMALL, too_small);
    if (info.total == 0) return RSASA_OK;
    if (int rc = nb_fill_by(f, a, info, launch)) return rc;
    RS_HIP(f.ctx, hipMemcpyAsync(out_entries, a.out, info.total * 8, hipMemcpyDeviceToHost, f.st));
    RS_HIP(f.ctx, hipStreamSynchronize(f.st));
    return RSASA_OK;
}

// ---- the neighbour lists (rsasa_precompute_neighbors*) ----

// One neighbour-list run (see nb_count).
int nb_run(rsasa_context *ctx, const Cols &c, const uint32_t *idx_map, float probe, float max_r, uint64_t *out_offsets,
           rsasa_neighbor_t *out_entries, size_t cap)
{
    Run f(ctx);
    if (!f.open(c.N, out_offsets)) return f.rc;
    int rc;
    NbArgs a{};
    NbInfo info{};
    if ((rc = nb_count(f, c, idx_map, probe, max_r, out_offsets, a, info))) return rc;
    return nb_entries_out(f, a, info, out_entries, cap, "out_entries holds fewer entries than out_offsets[n]",
                          [&](uint64_t spill_atoms) { launch_neighbor_fill(a, spill_atoms, f.st); });
}

// The single form's own: with active_indices only those atoms are binned and bounded (spatial_grid.rs:52-90,
// calculate_bounds): they are gathered, and idx maps back.  (A batch has none: active is null and n_active 0.)
int nb_entry(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form f,
             const uint32_t *active, size_t n_active, float probe, float max_r, uint64_t *out_offsets,
             rsasa_neighbor_t *out_entries, size_t cap)
{
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, f, nullptr, out_offsets && (!n_active || active), true)) return rc;
    if (!active) return nb_run(ctx, c, nullptr, probe, max_r, out_offsets, out_entries, cap);
    const size_t n = n_active;
    if (n >= 0x7FFFFFFFull) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 atoms");
    std::vector<uint8_t> seen(c.N, 0);
    std::vector<float> gx(n), gy(n), gz(n), gr(n);
    std::vector<uint64_t> gid(id ? n : 0);
    for (size_t k = 0; k < n; k++) {
        const uint32_t i = active[k];
        if (i >= c.N || seen[i]) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "active_indices must be distinct and below n_atoms");
        seen[i] = 1;
        gx[k] = x[i]; gy[k] = y[i]; gz[k] = z[i]; gr[k] = r[i];
        if (id) gid[k] = id[i];
    }
    Cols g(gx.data(), gy.data(), gz.data(), gr.data(), id ? gid.data() : nullptr);
    g.fix(Form::one(n));
    return nb_run(ctx, g, active, probe, max_r, out_offsets, out_entries, cap);
}

// ---- the point runs: what the eight families share ----

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
int pt_count(Run &f, const Cols &c, float probe, uint64_t *out_offsets, Lists &l)
{
    return nb_count(f, c, nullptr, probe, __builtin_nanf(""), out_offsets, l.a, l.info);
}

// The prologue's fill-and-prepare step: the lists' entries (no fill when every list is empty: `entries` is then null or
// stale, and no kernel reads it), the lattice, and the masks and values if the family wants them; `p` is then what every
// point kernel takes.  The masks and values stay on the device (RunScratch::masks, ::sasa) for the family to use.
int pt_prepare(Run &f, Lists &l, size_t n_points, bool masks, bool sasa, PtArgs &p)
{
    int rc;
    const size_t N = l.a.b.n_atoms, words = (n_points + 31) / 32;
    size_t padded = 0;
    p = PtArgs{};
    if ((l.info.total && (rc = nb_fill(f, l.a, l.info))) || (rc = pt_lattice(f.ctx, n_points, padded)) ||
        (masks && (rc = f.reserve(f.R.masks, N * words * 4, p.masks))) || (sasa && (rc = f.reserve(f.R.sasa, N * 4, p.sasa))))
        return rc;
    p.b = l.a.b;
    p.offsets = l.a.offsets;
    p.entries = (const uint2 *)f.R.entries.p;
    const float *lat = (const float *)f.ctx->pt_lattice.p;
    p.lx = lat; p.ly = lat + padded; p.lz = lat + 2 * padded;
    p.n_points = (uint32_t)n_points;
    p.n_fused = (uint32_t)(n_points - n_points % (size_t)f.ctx->simd_width);
    if (masks) p.words = (uint32_t)words;
    return RSASA_OK;
}

// Rows by scan: the neighbour runs' scan turns per-atom counts into RunScratch::row_offsets, which the caller has
// reserved for l's N + 1 entries (the neighbour run has read its parts and its info); the offsets are copied to the
// caller, and after the wait `total` is out_offsets[N], against which the family checks the caller's capacity.
// sort (nullable): flag bytes for k_sort_flags to order behind the scan.
int pt_rows(Run &f, const Lists &l, uint32_t *counts, const HsArgs *sort, uint64_t *out_offsets, uint64_t &total)
{
    const size_t N = l.a.b.n_atoms;
    NbArgs scan = l.a;
    scan.counts = counts;
    scan.offsets = (unsigned long long *)f.R.row_offsets.p;
    launch_neighbor_scan(scan, f.st);
    if (sort) launch_sort_flags(*sort, f.st);
    RS_HIP(f.ctx, hipGetLastError());
    RS_HIP(f.ctx, download(out_offsets, scan.offsets, (N + 1) * 8, f.st));
    RS_HIP(f.ctx, hipStreamSynchronize(f.st));
    total = out_offsets[N];
    return RSASA_OK;
}

// The accessible dots of a run whose masks pt_prepare has made room for: k_accessible_points writes the masks,
// k_mask_free counts them into `free`, and pt_rows turns the counts into dot offsets.  A dot's number is 32 bits in
// every kernel that follows.
int pt_dots(Run &f, const Lists &l, const PtArgs &p, uint32_t *free, const HsArgs *sort, uint64_t *out_offsets, uint64_t &n_dots)
{
    launch_accessible_points(p, f.st);
    launch_mask_free(p, free, f.st);
    if (int rc = pt_rows(f, l, free, sort, out_offsets, n_dots)) return rc;
    if (n_dots >= 0x100000000ull) return fail(f.ctx, RSASA_ERR_INVALID_ARGUMENT, "2^32 or more accessible dots");
    return RSASA_OK;
}

// ---- accessible points (rsasa_accessible_points*) ----

// One run of the point tests: k_accessible_points turns the lists into masks.
int pt_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form form,
           float probe, size_t n_points, uint32_t *out_masks, float *out_sasa)
{
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, &n_points, true, out_masks)) return rc;
    Run f(ctx);
    if (!f.open(c.N)) return f.rc;
    int rc;
    Lists l;
    PtArgs p{};
    if ((rc = pt_count(f, c, probe, nullptr, l)) || (rc = pt_prepare(f, l, n_points, true, out_sasa != nullptr, p))) return rc;
    launch_accessible_points(p, f.st);
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, download(out_masks, p.masks, c.N * p.words * 4, f.st));
    RS_HIP(ctx, download(out_sasa, p.sasa, c.N * 4, f.st));
    RS_HIP(ctx, hipStreamSynchronize(f.st));
    return RSASA_OK;
}

// ---- exposure vectors (rsasa_exposure_vectors*) ----

// One run of the exposure vectors: k_exposure_vectors turns the lists into the sum of each atom's exposed lattice points
// and their number; 16 bytes per atom come back (and 4 for the value, if asked).
int ex_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form form,
           float probe, size_t n_points, float *out_vectors, uint32_t *out_free, float *out_sasa)
{
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, &n_points, true, out_vectors && out_free)) return rc;
    Run f(ctx);
    if (!f.open(c.N)) return f.rc;
    int rc;
    Lists l;
    ExArgs e{};
    if ((rc = pt_count(f, c, probe, nullptr, l)) || (rc = pt_prepare(f, l, n_points, false, out_sasa != nullptr, e.p)) ||
        (rc = f.reserve(f.R.vectors, c.N * 12, e.vectors)) || (rc = f.reserve(f.R.free, c.N * 4, e.free)))
        return rc;
    launch_exposure_vectors(e, f.st);
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, download(out_vectors, e.vectors, c.N * 12, f.st));
    RS_HIP(ctx, download(out_free, e.free, c.N * 4, f.st));
    RS_HIP(ctx, download(out_sasa, e.p.sasa, c.N * 4, f.st));
    RS_HIP(ctx, hipStreamSynchronize(f.st));
    return RSASA_OK;
}

// ---- atom depth (rsasa_atom_depth*) ----

// One run of the atom depths: pt_run's masks stay on the device; k_mask_free counts them and k_atom_depth searches the
// grid for every atom's nearest accessible dot.  8 bytes per atom come back (and 4 each for the counts and the values,
// if asked); the square root of the key's d2 is taken here (sqrtf: correctly rounded).
int dp_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form form,
           float probe, size_t n_points, float *out_depth, uint32_t *out_nearest, uint32_t *out_free, float *out_sasa)
{
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, &n_points, true, out_depth && out_nearest)) return rc;
    Run f(ctx);
    if (!f.open(c.N)) return f.rc;
    int rc;
    Lists l;
    DpArgs d{};
    if ((rc = pt_count(f, c, probe, nullptr, l)) || (rc = pt_prepare(f, l, n_points, true, out_sasa != nullptr, d.p)) ||
        (rc = f.reserve(f.R.keys, c.N * 8, d.keys)) || (rc = f.reserve(f.R.free, c.N * 4, d.free)))
        return rc;
    launch_accessible_points(d.p, f.st);
    launch_mask_free(d.p, d.free, f.st);
    launch_atom_depth(d, f.st);
    RS_HIP(ctx, hipGetLastError());
    std::vector<uint64_t> keys(c.N);
    RS_HIP(ctx, download(keys.data(), d.keys, c.N * 8, f.st));
    RS_HIP(ctx, download(out_free, d.free, c.N * 4, f.st));
    RS_HIP(ctx, download(out_sasa, d.p.sasa, c.N * 4, f.st));
    RS_HIP(ctx, hipStreamSynchronize(f.st));
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

// One run of the surface components: pt_run's masks stay on the device and become dot offsets (pt_dots), the caller's
// label buffer is checked against out_offsets[N] as nb_run checks its entries, and the union-find kernels label the
// dots.  8 bytes per atom and 4 per dot come back (and 4 per atom each for the counts and the values, if asked).
int cc_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form form,
           float probe, size_t n_points, float link, uint64_t *out_offsets, uint32_t *out_labels, size_t cap,
           uint32_t *out_free, float *out_sasa)
{
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, &n_points, out_offsets, true)) return rc;
    RS_ARGS(ctx, check_link(link));
    Run f(ctx);
    if (!f.open(c.N, out_offsets)) return f.rc;
    int rc;
    Lists l;
    CcArgs cc{};
    if ((rc = pt_count(f, c, probe, nullptr, l)) || (rc = pt_prepare(f, l, n_points, true, out_sasa != nullptr, cc.p)) ||
        (rc = f.reserve(f.R.free, c.N * 4, cc.free)) || (rc = f.reserve(f.R.row_offsets, (c.N + 1) * 8, cc.dot_offsets)))
        return rc;
    cc.link = link;
    cc.link2 = link * link;
    uint64_t n_dots;
    if ((rc = pt_dots(f, l, cc.p, cc.free, nullptr, out_offsets, n_dots))) return rc;
    if (!out_labels || cap < n_dots)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "out_labels is NULL or holds fewer labels than out_dot_offsets[n]");
    if (n_dots) {
        if ((rc = f.reserve(f.R.parent, n_dots * 4, cc.parent)) || (rc = f.reserve(f.R.labels, n_dots * 4, cc.labels))) return rc;
        cc.n_dots = n_dots;
        launch_components(cc, f.st);
        RS_HIP(ctx, hipGetLastError());
        RS_HIP(ctx, download(out_labels, cc.labels, n_dots * 4, f.st));
    }
    RS_HIP(ctx, download(out_free, cc.free, c.N * 4, f.st));
    RS_HIP(ctx, download(out_sasa, cc.p.sasa, c.N * 4, f.st));
    RS_HIP(ctx, hipStreamSynchronize(f.st));
    return RSASA_OK;
}

// ---- dot links and dot geodesics (rsasa_dot_links*, rsasa_dot_geodesics*) ----

// The opening both share, cc_run's: pt_run's masks stay on the device and become dot offsets (pt_dots), which the
// caller gets; gd.c then describes the n_dots dots, under check_dot_total.
int gd_dots(Run &f, const Cols &c, float probe, size_t n_points, float link, bool sasa, uint64_t *out_offsets, Lists &l,
            GdArgs &gd, uint64_t &n_dots)
{
    int rc;
    CcArgs &cc = gd.c;
    if ((rc = pt_count(f, c, probe, nullptr, l)) || (rc = pt_prepare(f, l, n_points, true, sasa, cc.p)) ||
        (rc = f.reserve(f.R.free, c.N * 4, cc.free)) || (rc = f.reserve(f.R.row_offsets, (c.N + 1) * 8, cc.dot_offsets)))
        return rc;
    cc.link = link;
    cc.link2 = link * link;
    if ((rc = pt_dots(f, l, cc.p, cc.free, nullptr, out_offsets, n_dots))) return rc;
    RS_ARGS(f.ctx, check_dot_total(n_dots));
    cc.n_dots = n_dots;
    return RSASA_OK;
}

// The lengths of the lists of n_dots >= 1 dots and their offsets by the neighbour runs' scan (whose parts and info the
// neighbour run has read); waits, and `total` is link_offsets[n_dots].  The cursors of the fill pass are zeroed too.
int gd_count(Run &f, const Lists &l, GdArgs &gd, uint64_t &total)
{
    int rc;
    const uint64_t n_dots = gd.c.n_dots;
    NbArgs scan = l.a;
    if ((rc = f.reserve(f.R.link_counts, n_dots * 4, gd.counts)) || (rc = f.reserve(f.R.link_cursor, n_dots * 4, gd.cursor)) ||
        (rc = f.reserve(f.R.link_offsets, (n_dots + 1) * 8, scan.offsets)))
        return rc;
    RS_HIP(f.ctx, hipMemsetAsync(gd.counts, 0, n_dots * 4, f.st));
    RS_HIP(f.ctx, hipMemsetAsync(gd.cursor, 0, n_dots * 4, f.st));
    launch_dot_link_count(gd, f.st);
    scan.b.n_atoms = (uint32_t)n_dots;  // (the scan's items are the dots)
    scan.counts = gd.counts;
    scan.stage = 0xFFFFFFFFu;  // (no list is long: the fill stages nothing)
    launch_neighbor_scan(scan, f.st);
    gd.link_offsets = scan.offsets;
    gd.info = scan.info;
    NbHost *h = static_cast<NbHost *>(f.ctx->nb_host.p);
    RS_HIP(f.ctx, hipMemcpyAsync(&h->info, gd.info, sizeof(NbInfo), hipMemcpyDeviceToHost, f.st));
    RS_HIP(f.ctx, hipGetLastError());
    RS_HIP(f.ctx, hipStreamSynchronize(f.st));
    total = h->info.total;
    return RSASA_OK;
}

// One run of the dot links: the dots as in cc_run, the lists' lengths and offsets (gd_count); *out_n_links is written,
// the caller's buffers are checked against the two totals, then k_dot_link fills and k_link_sort orders the lists.  8
// bytes per atom, 8 per dot and 8 per entry come back (and 4 per atom each for the counts and the values, if asked).
int dl_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form form,
           float probe, size_t n_points, float link, uint64_t *out_offsets, uint64_t *out_n_links, uint64_t *out_link_offsets,
           size_t dots_cap, rsasa_within_t *out_entries, size_t cap, uint32_t *out_free, float *out_sasa)
{
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, &n_points, out_offsets && out_n_links, true)) return rc;
    RS_ARGS(ctx, check_link(link));
    *out_n_links = 0;  // (what a call that fails behind its rules leaves there, with or without the dot offsets)
    Run f(ctx);
    if (!f.open(c.N, out_offsets)) {
        if (f.rc == RSASA_OK && out_link_offsets) out_link_offsets[0] = 0;  // (no atom: no dot, no entry)
        return f.rc;
    }
    int rc;
    Lists l;
    GdArgs gd{};
    uint64_t n_dots, total = 0;
    if ((rc = gd_dots(f, c, probe, n_points, link, out_sasa != nullptr, out_offsets, l, gd, n_dots)) ||
        (n_dots && (rc = gd_count(f, l, gd, total))))
        return rc;
    *out_n_links = total;
    if (!out_link_offsets || dots_cap < n_dots || !out_entries || cap < total)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL,
                    "out_link_offsets or out_entries is NULL or holds fewer dots than out_dot_offsets[n] or fewer entries than "
                    "*out_n_links");
    if (!n_dots) out_link_offsets[0] = 0;
    if (total) {
        if ((rc = f.reserve(f.R.link_raw, total * 8, gd.raw)) || (rc = f.reserve(f.R.link_out, total * 8, gd.out))) return rc;
        launch_dot_link_fill(gd, false, f.st);
        NbHost *h = static_cast<NbHost *>(ctx->nb_host.p);
        RS_HIP(ctx, hipMemcpyAsync(&h->info, gd.info, sizeof(NbInfo), hipMemcpyDeviceToHost, f.st));
        RS_HIP(ctx, hipGetLastError());
        RS_HIP(ctx, hipStreamSynchronize(f.st));
        if (h->info.mismatch) return fail(ctx, RSASA_ERR_INTERNAL, "the fill pass of the dot links disagrees with its count pass");
        RS_HIP(ctx, download(out_entries, gd.out, total * 8, f.st));
    }
    if (n_dots) RS_HIP(ctx, download(out_link_offsets, gd.link_offsets, (n_dots + 1) * 8, f.st));
    RS_HIP(ctx, download(out_free, gd.c.free, c.N * 4, f.st));
    RS_HIP(ctx, download(out_sasa, gd.c.p.sasa, c.N * 4, f.st));
    RS_HIP(ctx, hipStreamSynchronize(f.st));
    return RSASA_OK;
}

// A phase of the geodesics over gd's n_dots >= 1 dots, whose start is queued: groups of kGdRounds rounds of the
// relaxation (source false) or of the source phase until one of them lowers nothing; n: the rounds run, that one
// included.  More rounds than there are dots (and one) is RSASA_ERR_INTERNAL.
int gd_phase(Run &f, const GdArgs &gd, bool source, uint32_t &n)
{
    rsasa_context *ctx = f.ctx;
    NbHost *h = static_cast<NbHost *>(ctx->nb_host.p);
    uint32_t flags[kGdRounds];
    for (uint64_t first = 2;; first += kGdRounds) {
        if (first > gd.c.n_dots + 3)
            return fail(ctx, RSASA_ERR_INTERNAL, "the dot geodesics did not settle within as many rounds as there are dots");
        RS_HIP(ctx, hipMemsetAsync(gd.flags, 0, sizeof flags, f.st));
        launch_geodesic_rounds(gd, source, (uint32_t)first, f.st);
        RS_HIP(ctx, hipMemcpyAsync(flags, gd.flags, sizeof flags, hipMemcpyDeviceToHost, f.st));
        RS_HIP(ctx, hipMemcpyAsync(&h->info, gd.info, sizeof(NbInfo), hipMemcpyDeviceToHost, f.st));
        RS_HIP(ctx, hipGetLastError());
        RS_HIP(ctx, hipStreamSynchronize(f.st));
        if (h->info.mismatch)
            return fail(ctx, RSASA_ERR_INTERNAL, "the fill pass of the dot links disagrees with its count pass");
        for (uint32_t k = 0; k < kGdRounds; k++)
            if (!flags[k]) {
                n = (uint32_t)(first - 2) + k + 1u;
                return RSASA_OK;
            }
    }
}

// One run of the dot geodesics: the dots and the lists' offsets as in dl_run, the seed bytes checked against the dots;
// the lists are filled as weights and stay on the device unsorted, k_geo_init turns the seeds into dist, and the rounds
// of k_geo_relax run kGdRounds at a time until one lowers nothing; then, if asked, the rounds of k_geo_source.  More
// rounds than there are dots (and one) is RSASA_ERR_INTERNAL.  8 bytes per atom and 4 per dot come back (4 more per dot
// for the sources, 4 per atom each for the counts and the values, if asked); the rounds run stay with the context
// (rsasa_context::gd_rounds, rsasa_context_geodesic_rounds).
int dg_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form form,
           float probe, size_t n_points, float link, const uint8_t *seeds, size_t n_seed_bytes, float limit,
           uint64_t *out_offsets, float *out_dist, uint32_t *out_source, uint32_t *out_free, float *out_sasa)
{
    static_assert(sizeof(GdArgs) <= 4096, "kernel arguments");
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, &n_points, out_offsets, true)) return rc;
    RS_ARGS(ctx, check_link(link));
    RS_ARGS(ctx, check_geodesic_limit(limit));
    char why[96];
    uint32_t n_rounds[2] = {0u, 0u};
    Run f(ctx);
    ctx->gd_rounds[0] = ctx->gd_rounds[1] = 0u;  // (under the mutex the frame holds)
    if (!f.open(c.N, out_offsets)) {
        if (f.rc == RSASA_OK) RS_ARGS(ctx, check_seed_bytes(seeds, n_seed_bytes, 0, why));
        return f.rc;
    }
    int rc;
    Lists l;
    GdArgs gd{};
    uint64_t n_dots, total = 0;
    if ((rc = gd_dots(f, c, probe, n_points, link, out_sasa != nullptr, out_offsets, l, gd, n_dots))) return rc;
    RS_ARGS(ctx, check_seed_bytes(seeds, n_seed_bytes, n_dots, why));
    if (n_dots && !out_dist) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_dots) {
        if ((rc = gd_count(f, l, gd, total)) || (total && (rc = f.reserve(f.R.link_raw, total * 8, gd.raw))) ||
            (rc = f.upload(f.R.gd_seeds, seeds, n_dots, gd.seeds)) || (rc = f.reserve(f.R.gd_dist, n_dots * 4, gd.dist)) ||
            (rc = f.reserve(f.R.gd_stamp, n_dots * 4, gd.stamp)) ||
            (out_source && (rc = f.reserve(f.R.gd_source, n_dots * 4, gd.source))) ||
            (rc = f.reserve(f.R.gd_flags, kGdRounds * 4, gd.flags)))
            return rc;
        gd.limit = limit + 0.0f;  // (-0.0 is 0)
        if (total) launch_dot_link_fill(gd, true, f.st);
        launch_geodesic_init(gd, f.st);
        if ((rc = gd_phase(f, gd, false, n_rounds[0]))) return rc;
        if (out_source) {
            launch_geodesic_restamp(gd, f.st);
            if ((rc = gd_phase(f, gd, true, n_rounds[1]))) return rc;
        }
        RS_HIP(ctx, download(out_dist, gd.dist, n_dots * 4, f.st));
        RS_HIP(ctx, download(out_source, gd.source, n_dots * 4, f.st));
    }
    ctx->gd_rounds[0] = n_rounds[0];
    ctx->gd_rounds[1] = n_rounds[1];
    RS_HIP(ctx, download(out_free, gd.c.free, c.N * 4, f.st));
    RS_HIP(ctx, download(out_sasa, gd.c.p.sasa, c.N * 4, f.st));
    RS_HIP(ctx, hipStreamSynchronize(f.st));
    return RSASA_OK;
}

// ---- dot patches (rsasa_dot_patches*) ----

// One run of the dot patches: the dots and the weighted lists as in dg_run; *out_bound and the caller's buffers are
// checked against the dots (check_patch_room) before anything is sampled.  k_patch_sample then makes every structure's
// picks in one launch - one wait, no polling - and, if asked, the source phase of the geodesics runs from the centres it
// marked.  The centres are packed on the device (k_patch_pack) once the host has scanned their counts.  8 bytes per atom, 4
// per dot, 4 per structure and 8 per centre come back (4 more per dot for the sources, 4 per atom each for the counts and the values, if asked);
// the sampler's sums stay with the context (rsasa_context::ps_stats, rsasa_context_patch_stats).
int ps_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form form,
           float probe, size_t n_points, float link, float spacing, uint32_t max_centres, uint64_t *out_offsets,
           uint64_t *out_bound, uint64_t *out_centre_offsets, uint32_t *out_centres, float *out_cover, size_t centres_cap,
           float *out_dist, uint32_t *out_source, size_t dots_cap, uint32_t *out_free, float *out_sasa)
{
    static_assert(sizeof(PsArgs) <= 4096, "kernel arguments");
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, &n_points, out_offsets && out_bound, true)) return rc;
    RS_ARGS(ctx, check_link(link));
    RS_ARGS(ctx, check_patch_spacing(spacing));
    RS_ARGS(ctx, check_patch_max_centres(max_centres));
    *out_bound = 0;
    Run f(ctx);
    ctx->ps_stats[0] = ctx->ps_stats[1] = ctx->ps_stats[2] = 0u;  // (under the mutex the frame holds)
    if (!f.open(c.N, out_offsets)) {
        if (f.rc == RSASA_OK && out_centre_offsets) std::fill(out_centre_offsets, out_centre_offsets + c.S + 1, 0ull);  // (no atom: no centre)
        return f.rc;
    }
    int rc;
    Lists l;
    PsArgs ps{};
    GdArgs &gd = ps.g;
    uint64_t n_dots, total = 0;
    if ((rc = gd_dots(f, c, probe, n_points, link, out_sasa != nullptr, out_offsets, l, gd, n_dots))) return rc;
    std::vector<uint64_t> slots(c.S + 1);
    const uint64_t bound = patch_centre_bound(out_offsets, c.so, c.S, max_centres, slots.data());
    *out_bound = bound;
    if (const char *msg = check_patch_room(out_centre_offsets, out_centres, out_cover, out_dist, dots_cap, n_dots, centres_cap, bound))
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, msg);
    std::fill(out_centre_offsets, out_centre_offsets + c.S + 1, 0ull);
    PsStats stats{};
    if (n_dots) {
        const unsigned long long *slot_offsets;
        if ((rc = gd_count(f, l, gd, total)) || (total && (rc = f.reserve(f.R.link_raw, total * 8, gd.raw))) ||
            (rc = f.reserve(f.R.gd_dist, n_dots * 4, gd.dist)) || (rc = f.reserve(f.R.gd_stamp, n_dots * 4, gd.stamp)) ||
            (out_source && (rc = f.reserve(f.R.gd_source, n_dots * 4, gd.source))) ||
            (rc = f.reserve(f.R.gd_flags, kGdRounds * 4, gd.flags)) || (rc = f.upload(f.R.so, c.so, (c.S + 1) * 4, ps.so)) ||
            (rc = f.upload(f.R.ps_slots, (const unsigned long long *)slots.data(), (c.S + 1) * 8, slot_offsets)) ||
            (rc = f.reserve(f.R.ps_counts, c.S * 4, ps.n_centres)) || (rc = f.reserve(f.R.ps_centres, bound * 4, ps.centres)) ||
            (rc = f.reserve(f.R.ps_cover, bound * 4, ps.cover)) || (rc = f.reserve(f.R.ps_stats, sizeof(PsStats), ps.stats)))
            return rc;
        ps.slot_offsets = slot_offsets;
        ps.n_structures = (uint32_t)c.S;
        ps.spacing = spacing + 0.0f;  // (-0.0 is 0)
        ps.max_centres = max_centres;
        gd.limit = __builtin_inff();
        RS_HIP(ctx, hipMemsetAsync(ps.stats, 0, sizeof(PsStats), f.st));
        if (total) launch_dot_link_fill(gd, true, f.st);
        launch_patch_sample(ps, f.st);
        NbHost *h = static_cast<NbHost *>(ctx->nb_host.p);
        std::vector<uint32_t> counts(c.S);
        RS_HIP(ctx, hipMemcpyAsync(&stats, ps.stats, sizeof(PsStats), hipMemcpyDeviceToHost, f.st));
        RS_HIP(ctx, hipMemcpyAsync(&h->info, gd.info, sizeof(NbInfo), hipMemcpyDeviceToHost, f.st));
        RS_HIP(ctx, hipMemcpyAsync(counts.data(), ps.n_centres, c.S * 4, hipMemcpyDeviceToHost, f.st));
        RS_HIP(ctx, hipGetLastError());
        RS_HIP(ctx, hipStreamSynchronize(f.st));
        if (h->info.mismatch) return fail(ctx, RSASA_ERR_INTERNAL, "the fill pass of the dot links disagrees with its count pass");
        if (stats.error) return fail(ctx, RSASA_ERR_INTERNAL, "the dot patches of a structure left a bounded loop of the sampler");
        for (size_t s = 0; s < c.S; s++) {
            if (counts[s] > slots[s + 1] - slots[s])
                return fail(ctx, RSASA_ERR_INTERNAL, "a structure of the dot patches has more centres than its bound");
            out_centre_offsets[s + 1] = out_centre_offsets[s] + counts[s];
        }
        // the centres without the unused room of the bound: K entries come back, packed on the device
        const uint64_t n_centres = out_centre_offsets[c.S];
        const unsigned long long *centre_offsets;
        if ((rc = f.upload(f.R.ps_offsets, (const unsigned long long *)out_centre_offsets, (c.S + 1) * 8, centre_offsets)) ||
            (rc = f.reserve(f.R.ps_packed, n_centres * 8, ps.packed_centres)))
            return rc;
        ps.centre_offsets = centre_offsets;
        ps.packed_cover = ps.packed_centres + n_centres;
        launch_patch_pack(ps, f.st);
        RS_HIP(ctx, hipGetLastError());
        RS_HIP(ctx, download(out_centres, ps.packed_centres, n_centres * 4, f.st));
        RS_HIP(ctx, download(out_cover, ps.packed_cover, n_centres * 4, f.st));
        if (out_source) {
            uint32_t n_rounds = 0;
            launch_geodesic_restamp(gd, f.st);
            if ((rc = gd_phase(f, gd, true, n_rounds))) return rc;
        }
        RS_HIP(ctx, download(out_dist, gd.dist, n_dots * 4, f.st));
        RS_HIP(ctx, download(out_source, gd.source, n_dots * 4, f.st));
    }
    RS_HIP(ctx, download(out_free, gd.c.free, c.N * 4, f.st));
    RS_HIP(ctx, download(out_sasa, gd.c.p.sasa, c.N * 4, f.st));
    RS_HIP(ctx, hipStreamSynchronize(f.st));
    ctx->ps_stats[0] = stats.picks;
    ctx->ps_stats[1] = stats.steps;
    ctx->ps_stats[2] = stats.overflows;
    return RSASA_OK;
}

// ---- dot crowding (rsasa_dot_crowding*) ----

// The flag bytes of a run (flags: host, [N], nullable) for k_sort_flags: uploaded, with room for their cell-sorted copy.
// The caller points h.b at the grid.
int hs_flags(Run &f, size_t N, const uint8_t *flags, HsArgs &h)
{
    if (int rc = f.upload(f.R.flags, flags, N, h.flags)) return rc;
    return f.reserve(f.R.sorted_flags, N, h.sorted_flags);
}

// One run of the dot crowding: the dots as in cc_run, with the flag bytes beside them (hs_flags) and sorted by
// k_sort_flags behind the scan; the caller's buffer is checked against out_offsets[N], then k_dot_crowding fills a row of
// n_bins counts per dot.  8 bytes per atom and 4 * n_bins per dot come back (and 4 per atom each for the counts and the
// values, if asked).  check_crowding has passed.
int dc_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form form,
           float probe, size_t n_points, const uint8_t *flags, const float *edges, uint32_t n_bins, uint64_t *out_offsets,
           uint32_t *out_counts, size_t cap, uint32_t *out_free, float *out_sasa)
{
    static_assert(kCrowdMaxBins == RSASA_CROWD_MAX_BINS, "the header's bound is the kernel's bound");
    static_assert(sizeof(DcArgs::e2) == kCrowdMaxBins * sizeof(float), "an edge per bin");
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, &n_points, out_offsets, true)) return rc;
    RS_ARGS(ctx, check_crowding(edges, n_bins));
    Run f(ctx);
    if (!f.open(c.N, out_offsets)) return f.rc;
    int rc;
    Lists l;
    DcArgs dc{};
    HsArgs h{};
    if ((rc = pt_count(f, c, probe, nullptr, l)) || (rc = pt_prepare(f, l, n_points, true, out_sasa != nullptr, dc.p)) ||
        (rc = f.reserve(f.R.free, c.N * 4, dc.free)) || (rc = f.reserve(f.R.row_offsets, (c.N + 1) * 8, dc.dot_offsets)) ||
        (rc = hs_flags(f, c.N, flags, h)))
        return rc;
    h.b = dc.p.b;
    dc.sorted_flags = h.sorted_flags;
    dc.n_bins = n_bins;
    for (uint32_t k = 0; k < kCrowdMaxBins; k++) {
        const float e = edges[k < n_bins ? k : n_bins - 1u];
        dc.e2[k] = e * e;
    }
    uint64_t n_dots;
    if ((rc = pt_dots(f, l, dc.p, dc.free, &h, out_offsets, n_dots))) return rc;
    if (!out_counts || cap < n_dots)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "out_counts is NULL or holds fewer rows than out_dot_offsets[n]");
    if (n_dots) {
        if ((rc = f.reserve(f.R.crowd, n_dots * n_bins * 4, dc.counts))) return rc;
        launch_dot_crowding(dc, f.st);
        RS_HIP(ctx, hipGetLastError());
        RS_HIP(ctx, download(out_counts, dc.counts, n_dots * n_bins * 4, f.st));
    }
    RS_HIP(ctx, download(out_free, dc.free, c.N * 4, f.st));
    RS_HIP(ctx, download(out_sasa, dc.p.sasa, c.N * 4, f.st));
    RS_HIP(ctx, hipStreamSynchronize(f.st));
    return RSASA_OK;
}

// ---- dot fields (rsasa_dot_fields*) ----

// One run of the dot fields: dc_run's dots and sorted flags, with the weight rows uploaded beside them in input order;
// the caller's buffer is checked against out_offsets[N], then k_dot_fields fills a row of n_channels sums per dot.  8
// bytes per atom and 8 * n_channels per dot come back (and 4 per atom each for the counts and the values, if asked).
int fd_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form form,
           float probe, size_t n_points, const uint8_t *flags, const float *weights, const uint8_t *kinds, uint32_t n_channels,
           float cutoff, uint64_t *out_offsets, int64_t *out_sums, size_t cap, uint32_t *out_free, float *out_sasa)
{
    static_assert(kFieldMaxChannels == RSASA_FIELD_MAX_CHANNELS && kFieldMaxChannels == kFieldChannels,
                  "the header's bound is the kernel's bound");
    static_assert(RSASA_FIELD_STEP == 0 && RSASA_FIELD_INV_D == 1 && RSASA_FIELD_INV_D2 == 2 && RSASA_FIELD_INV_1PD == 3 &&
                      kFieldKinds == 4, "the kinds as k_dot_fields reads them");
    static_assert(sizeof(long long) == sizeof(int64_t), "a sum is 64 bits");
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, &n_points, out_offsets, weights != nullptr)) return rc;
    RS_ARGS(ctx, check_fields(kinds, n_channels, cutoff));
    Run f(ctx);
    if (!f.open(c.N, out_offsets)) return f.rc;
    int rc;
    Lists l;
    FdArgs fd{};
    HsArgs h{};
    if ((rc = pt_count(f, c, probe, nullptr, l)) || (rc = pt_prepare(f, l, n_points, true, out_sasa != nullptr, fd.p)) ||
        (rc = f.reserve(f.R.free, c.N * 4, fd.free)) || (rc = f.reserve(f.R.row_offsets, (c.N + 1) * 8, fd.dot_offsets)) ||
        (rc = hs_flags(f, c.N, flags, h)) || (rc = f.upload(f.R.field_w, weights, c.N * n_channels * 4, fd.weights)))
        return rc;
    h.b = fd.p.b;
    fd.sorted_flags = h.sorted_flags;
    fd.n_channels = n_channels;
    for (uint32_t k = 0; k < n_channels; k++) {
        fd.kinds[k] = kinds[k];
        fd.need |= 1u << kinds[k];
    }
    const float cut = cutoff + 0.0f;  // (-0.0 is 0)
    fd.c2 = cut * cut;
    uint64_t n_dots;
    if ((rc = pt_dots(f, l, fd.p, fd.free, &h, out_offsets, n_dots))) return rc;
    if (!out_sums || cap < n_dots)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "out_sums is NULL or holds fewer rows than out_dot_offsets[n]");
    if (n_dots) {
        if ((rc = f.reserve(f.R.fields, n_dots * n_channels * 8, fd.sums))) return rc;
        launch_dot_fields(fd, f.st);
        RS_HIP(ctx, hipGetLastError());
        RS_HIP(ctx, download(out_sums, fd.sums, n_dots * n_channels * 8, f.st));
    }
    RS_HIP(ctx, download(out_free, fd.free, c.N * 4, f.st));
    RS_HIP(ctx, download(out_sasa, fd.p.sasa, c.N * 4, f.st));
    RS_HIP(ctx, hipStreamSynchronize(f.st));
    return RSASA_OK;
}

// ---- dot curvature (rsasa_dot_curvature*) ----

// One run of the dot curvature: the dots as in cc_run with the reach as their link; the caller's two buffers are checked
// against out_offsets[N], both device buffers are zeroed (k_dot_curvature adds to its rows), then the kernel fills a pair
// count and a row of eight sums per dot.  8 bytes per atom and 68 per dot come back (and 4 per atom each for the counts
// and the values, if asked).
int cv_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form form,
           float probe, size_t n_points, float reach, uint64_t *out_offsets, uint32_t *out_pairs, int64_t *out_moments, size_t cap,
           uint32_t *out_free, float *out_sasa)
{
    static_assert(RSASA_CURV_D2 == 0 && RSASA_CURV_H == 1 && RSASA_CURV_XX == 2 && RSASA_CURV_YY == 3 && RSASA_CURV_ZZ == 4 &&
                      RSASA_CURV_XY == 5 && RSASA_CURV_XZ == 6 && RSASA_CURV_YZ == 7 && RSASA_CURV_COLUMNS == kCurvColumns,
                  "the columns as k_dot_curvature writes them");
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "a sum is 64 bits");
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, &n_points, out_offsets, true)) return rc;
    RS_ARGS(ctx, check_curvature(reach));
    Run f(ctx);
    if (!f.open(c.N, out_offsets)) return f.rc;
    int rc;
    Lists l;
    CvArgs cv{};
    CcArgs &cc = cv.c;
    if ((rc = pt_count(f, c, probe, nullptr, l)) || (rc = pt_prepare(f, l, n_points, true, out_sasa != nullptr, cc.p)) ||
        (rc = f.reserve(f.R.free, c.N * 4, cc.free)) || (rc = f.reserve(f.R.row_offsets, (c.N + 1) * 8, cc.dot_offsets)))
        return rc;
    cc.link = reach + 0.0f;  // (-0.0 is 0)
    cc.link2 = cc.link * cc.link;
    uint64_t n_dots;
    if ((rc = pt_dots(f, l, cc.p, cc.free, nullptr, out_offsets, n_dots))) return rc;
    if (!out_pairs || !out_moments || cap < n_dots)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL,
                    "out_pairs or out_moments is NULL or holds fewer dots than out_dot_offsets[n]");
    if (n_dots) {
        if ((rc = f.reserve(f.R.curv_pairs, n_dots * 4, cv.pairs)) ||
            (rc = f.reserve(f.R.curv_moments, n_dots * kCurvColumns * 8, cv.moments)))
            return rc;
        cc.n_dots = n_dots;
        RS_HIP(ctx, hipMemsetAsync(cv.pairs, 0, n_dots * 4, f.st));
        RS_HIP(ctx, hipMemsetAsync(cv.moments, 0, n_dots * kCurvColumns * 8, f.st));
        launch_dot_curvature(cv, f.st);
        RS_HIP(ctx, hipGetLastError());
        RS_HIP(ctx, download(out_pairs, cv.pairs, n_dots * 4, f.st));
        RS_HIP(ctx, download(out_moments, cv.moments, n_dots * kCurvColumns * 8, f.st));
    }
    RS_HIP(ctx, download(out_free, cc.free, c.N * 4, f.st));
    RS_HIP(ctx, download(out_sasa, cc.p.sasa, c.N * 4, f.st));
    RS_HIP(ctx, hipStreamSynchronize(f.st));
    return RSASA_OK;
}

// ---- dot enclosure (rsasa_dot_enclosure*) ----

// One run of the dot enclosure: dc_run's dots and sorted flags; the fan of n_dirs directions is computed here
// (generate_sphere_points, what rsasa_sphere_points returns) and travels in the kernel's arguments with the reach, its
// square and the rays' far ends reach * u_m; the caller's buffer is checked against out_offsets[N], then k_dot_enclosure
// fills a word per dot.  8 bytes per atom and 4 per dot come back (and 4 per atom each for the counts and the values,
// if asked).
int de_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form form,
           float probe, size_t n_points, const uint8_t *flags, float reach, uint32_t n_dirs, uint64_t *out_offsets,
           uint32_t *out_blocked, size_t cap, uint32_t *out_free, float *out_sasa)
{
    static_assert(kEncloseMaxDirs == RSASA_ENCLOSE_MAX_DIRS, "the header's bound is the kernel's bound");
    static_assert(kEncloseMaxDirs == kEncloseDirs && kEncloseDirs == 32, "a direction per bit of a dot's word");
    static_assert(sizeof(DeArgs::dir) == kEncloseMaxDirs * 32, "32 bytes per direction");
    static_assert(sizeof(DeArgs) <= 4096, "kernel arguments");
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, &n_points, out_offsets, true)) return rc;
    RS_ARGS(ctx, check_enclosure(reach, n_dirs));
    Run f(ctx);
    if (!f.open(c.N, out_offsets)) return f.rc;
    int rc;
    Lists l;
    DeArgs de{};
    HsArgs h{};
    if ((rc = pt_count(f, c, probe, nullptr, l)) || (rc = pt_prepare(f, l, n_points, true, out_sasa != nullptr, de.p)) ||
        (rc = f.reserve(f.R.free, c.N * 4, de.free)) || (rc = f.reserve(f.R.row_offsets, (c.N + 1) * 8, de.dot_offsets)) ||
        (rc = hs_flags(f, c.N, flags, h)))
        return rc;
    h.b = de.p.b;
    de.sorted_flags = h.sorted_flags;
    de.n_dirs = n_dirs;
    de.reach = reach + 0.0f;  // (-0.0 is 0)
    de.reach2 = de.reach * de.reach;
    float ux[kEncloseMaxDirs], uy[kEncloseMaxDirs], uz[kEncloseMaxDirs];
    generate_sphere_points(n_dirs, ux, uy, uz);
    for (uint32_t m = 0; m < n_dirs; m++)
        de.dir[m] = DeDir{ux[m], uy[m], uz[m], 0.0f, de.reach * ux[m], de.reach * uy[m], de.reach * uz[m], 0.0f};
    uint64_t n_dots;
    if ((rc = pt_dots(f, l, de.p, de.free, &h, out_offsets, n_dots))) return rc;
    if (!out_blocked || cap < n_dots)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "out_blocked is NULL or holds fewer words than out_dot_offsets[n]");
    if (n_dots) {
        if ((rc = f.reserve(f.R.enclose, n_dots * 4, de.blocked))) return rc;
        launch_dot_enclosure(de, f.st);
        RS_HIP(ctx, hipGetLastError());
        RS_HIP(ctx, download(out_blocked, de.blocked, n_dots * 4, f.st));
    }
    RS_HIP(ctx, download(out_free, de.free, c.N * 4, f.st));
    RS_HIP(ctx, download(out_sasa, de.p.sasa, c.N * 4, f.st));
    RS_HIP(ctx, hipStreamSynchronize(f.st));
    return RSASA_OK;
}

// ---- contact counts (rsasa_contact_points*) ----

// One run of the contact counts: the lists, sized and copied out as by nb_run, and k_contact_points' counts of every
// entry beside them (like the entries, not read when every list is empty).
int ct_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form form,
           float probe, size_t n_points, uint64_t *out_offsets, rsasa_neighbor_t *out_entries, uint32_t *out_covered,
           uint32_t *out_exclusive, size_t cap, float *out_sasa)
{
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, &n_points, out_offsets, true)) return rc;
    Run f(ctx);
    if (!f.open(c.N, out_offsets)) return f.rc;
    int rc;
    Lists l;
    CtArgs ct{};
    if ((rc = pt_count(f, c, probe, out_offsets, l))) return rc;
    const size_t total = l.info.total;
    if (!out_entries || !out_covered || !out_exclusive || cap < total)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "an entry buffer is NULL or holds fewer entries than out_offsets[n]");
    if ((rc = pt_prepare(f, l, n_points, false, out_sasa != nullptr, ct.p)) ||
        (rc = f.reserve(f.R.covered, total * 4, ct.covered)) || (rc = f.reserve(f.R.exclusive, total * 4, ct.exclusive)))
        return rc;
    launch_contact_points(ct, f.st);
    RS_HIP(ctx, hipGetLastError());
    if (total) {
        RS_HIP(ctx, download(out_entries, ct.p.entries, total * 8, f.st));
        RS_HIP(ctx, download(out_covered, ct.covered, total * 4, f.st));
        RS_HIP(ctx, download(out_exclusive, ct.exclusive, total * 4, f.st));
    }
    RS_HIP(ctx, download(out_sasa, ct.p.sasa, c.N * 4, f.st));
    RS_HIP(ctx, hipStreamSynchronize(f.st));
    return RSASA_OK;
}

// ---- contact owners (rsasa_contact_owners*) ----

// One run of the contact owners: the lists, sized and copied out as by ct_run, and k_contact_owners' count of every
// entry beside them; the owner of every point too when the caller asks for it (no device memory for it otherwise).
int co_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form form,
           float probe, size_t n_points, uint64_t *out_offsets, rsasa_neighbor_t *out_entries, uint32_t *out_owned,
           size_t cap, uint32_t *out_owner, float *out_sasa)
{
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, &n_points, out_offsets, true)) return rc;
    Run f(ctx);
    if (!f.open(c.N, out_offsets)) return f.rc;
    int rc;
    Lists l;
    CoArgs co{};
    if ((rc = pt_count(f, c, probe, out_offsets, l))) return rc;
    const size_t total = l.info.total;
    if (!out_entries || !out_owned || cap < total)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "an entry buffer is NULL or holds fewer entries than out_offsets[n]");
    if ((rc = pt_prepare(f, l, n_points, false, out_sasa != nullptr, co.p)) || (rc = f.reserve(f.R.owned, total * 4, co.owned)) ||
        (out_owner && (rc = f.reserve(f.R.owner, c.N * n_points * 4, co.owner))))
        return rc;
    launch_contact_owners(co, f.st);
    RS_HIP(ctx, hipGetLastError());
    if (total) {
        RS_HIP(ctx, download(out_entries, co.p.entries, total * 8, f.st));
        RS_HIP(ctx, download(out_owned, co.owned, total * 4, f.st));
    }
    RS_HIP(ctx, download(out_owner, co.owner, c.N * n_points * 4, f.st));
    RS_HIP(ctx, download(out_sasa, co.p.sasa, c.N * 4, f.st));
    RS_HIP(ctx, hipStreamSynchronize(f.st));
    return RSASA_OK;
}

// ---- group contacts (rsasa_group_contacts*) ----

// One run of the group contacts: k_group_order puts each list in label order and counts its rows, the rows' offsets come
// by scan (pt_rows), the caller's row buffers are checked against out_offsets[N] as nb_run checks its
// entries, and k_group_points fills the rows.  (Like the entries, the lists' copies and the rows are not read when there
// are none.)
int gp_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id,
           const uint32_t *group, Form form, float probe, size_t n_points, uint64_t *out_offsets, uint32_t *out_groups,
           uint32_t *out_buried, uint32_t *out_only, size_t cap, uint32_t *out_self_free, uint32_t *out_free,
           float *out_sasa)
{
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, &n_points, out_offsets, group && out_self_free && out_free)) return rc;
    Run f(ctx);
    if (!f.open(c.N, out_offsets)) return f.rc;
    int rc;
    rsasa_context::RunScratch &R = f.R;
    const size_t N = c.N;
    Lists l;
    GpArgs g{};
    if ((rc = pt_count(f, c, probe, nullptr, l)) || (rc = pt_prepare(f, l, n_points, false, out_sasa != nullptr, g.p)) ||
        (rc = f.reserve(R.sorted, l.info.total * 8, g.sorted)) || (rc = f.reserve(R.sorted_group, l.info.total * 4, g.sorted_group)) ||
        (rc = f.upload(R.group, group, N * 4, g.group)) || (rc = f.reserve(R.own, N * 4, g.n_own)) ||
        (rc = f.reserve(R.nrows, N * 4, g.n_rows)) || (rc = f.reserve(R.row_offsets, (N + 1) * 8, g.row_offsets)))
        return rc;
    uint64_t n_rows;
    launch_group_order(g, f.st);
    if ((rc = pt_rows(f, l, g.n_rows, nullptr, out_offsets, n_rows))) return rc;
    if (!out_groups || !out_buried || !out_only || cap < n_rows)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "a row buffer is NULL or holds fewer rows than out_offsets[n]");
    if ((rc = f.reserve(R.groups, n_rows * 4, g.groups)) || (rc = f.reserve(R.buried, n_rows * 4, g.buried)) ||
        (rc = f.reserve(R.only, n_rows * 4, g.only)) || (rc = f.reserve(R.self_free, N * 4, g.self_free)) ||
        (rc = f.reserve(R.free, N * 4, g.free)))
        return rc;
    launch_group_points(g, f.st);
    RS_HIP(ctx, hipGetLastError());
    if (n_rows) {
        RS_HIP(ctx, download(out_groups, g.groups, n_rows * 4, f.st));
        RS_HIP(ctx, download(out_buried, g.buried, n_rows * 4, f.st));
        RS_HIP(ctx, download(out_only, g.only, n_rows * 4, f.st));
    }
    RS_HIP(ctx, download(out_self_free, g.self_free, N * 4, f.st));
    RS_HIP(ctx, download(out_free, g.free, N * 4, f.st));
    RS_HIP(ctx, download(out_sasa, g.p.sasa, N * 4, f.st));
    RS_HIP(ctx, hipStreamSynchronize(f.st));
    return RSASA_OK;
}

// ---- the runs on the grid alone: half-sphere exposure (rsasa_half_sphere_exposure*), atoms within a cutoff
// (rsasa_atoms_within*), the k nearest atoms (rsasa_nearest_atoms*), radial counts (rsasa_radial_counts*) ----

// The opening of a run on the grid alone: the grid into h.b (nb_grid with every structure's own largest radius:
// max_r = NaN), then the flag bytes beside it (hs_flags); k_sort_flags (launch_half_sphere, launch_sort_flags) then
// writes h.sorted_flags.
int hs_grid(Run &f, const Cols &c, const uint32_t *idx_map, float probe, const uint8_t *flags, HsArgs &h)
{
    if (int rc = nb_grid(f, c, idx_map, probe, __builtin_nanf(""), h.b)) return rc;
    return hs_flags(f, c.N, flags, h);
}

// One run of the half-sphere counts: the grid alone (hs_grid: no counting pass, no lists) with the flags, the directions
// beside them, k_sort_flags and k_half_sphere; 8 bytes per atom come back.
int hs_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form form,
           float probe, const float *dirs, const uint8_t *flags, float cutoff, uint32_t *out_up, uint32_t *out_down)
{
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, nullptr, true, out_up && out_down)) return rc;
    RS_ARGS(ctx, check_cutoff(cutoff));
    Run f(ctx);
    if (!f.open(c.N)) return f.rc;
    int rc;
    const size_t N = c.N;
    HsArgs h{};
    if ((rc = hs_grid(f, c, nullptr, probe, flags, h)) || (rc = f.upload(f.R.dirs, dirs, N * 12, h.dirs)) ||
        (rc = f.reserve(f.R.up, N * 4, h.up)) || (rc = f.reserve(f.R.down, N * 4, h.down)))
        return rc;
    h.cutoff = cutoff;
    launch_half_sphere(h, f.st);
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, download(out_up, h.up, N * 4, f.st));
    RS_HIP(ctx, download(out_down, h.down, N * 4, f.st));
    RS_HIP(ctx, hipStreamSynchronize(f.st));
    return RSASA_OK;
}

// One run of the lists within a cutoff: the grid alone and the flags as in hs_run, k_within_count and the neighbour
// runs' scan, then the end of nb_run (nb_entries_out) with k_within_fill (and the ranking of the long lists).
int wn_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form form,
           float probe, const uint8_t *flags, float cutoff, int upper_only, uint64_t *out_offsets,
           rsasa_within_t *out_entries, size_t cap)
{
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, nullptr, out_offsets, true)) return rc;
    RS_ARGS(ctx, check_cutoff(cutoff));
    Run f(ctx);
    if (!f.open(c.N, out_offsets)) return f.rc;
    int rc;
    HsArgs h{};
    WnArgs w{};
    NbInfo info{};
    if ((rc = hs_grid(f, c, nullptr, probe, flags, h))) return rc;
    w.n.b = h.b;
    if ((rc = nb_scan_buffers(f, c.N, within_stage_capacity(), w.n))) return rc;
    w.sorted_flags = h.sorted_flags;
    w.cutoff = cutoff;
    w.upper_only = upper_only ? 1u : 0u;
    launch_sort_flags(h, f.st);
    launch_within_count(w, f.st);
    if ((rc = nb_sizes(f, w.n, c.N, out_offsets, info))) return rc;
    return nb_entries_out(f, w.n, info, out_entries, cap, "out_entries is NULL or holds fewer entries than out_offsets[n]",
                          [&](uint64_t spill_atoms) { launch_within_fill(w, spill_atoms, f.st); });
}

// One run of the k nearest atoms: the grid alone and the flags as in wn_run, with the centres' ranks (a host prefix over
// the flag bytes: which row a centre's keys go to) uploaded beside the columns; k_nearest sweeps once and leaves rows and
// counts, the neighbour runs' scan and the sizing rule of nb_run follow, then k_nearest_gather and 8 bytes per entry
// back.  (Its end is its own: no fill pass, and the gather's verdict comes back with the entries, in one wait.)
int nn_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form form,
           float probe, const uint8_t *flags, uint32_t k, float cutoff, uint64_t *out_offsets, rsasa_within_t *out_entries,
           size_t cap)
{
    static_assert(kNearestMaxK == RSASA_NEAREST_MAX_K, "the header's bound is the kernels' bound");
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, nullptr, out_offsets, true)) return rc;
    RS_ARGS(ctx, check_nearest_k(k));
    RS_ARGS(ctx, check_nearest_cutoff(cutoff));
    Run f(ctx);
    if (!f.open(c.N, out_offsets)) return f.rc;
    int rc;
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
    if ((rc = hs_grid(f, c, flags ? rank.data() : nullptr, probe, flags, h)) || (rc = f.reserve(f.R.rows, rows * k * 8, nn.rows)))
        return rc;
    nn.w.n.b = h.b;
    if ((rc = nb_scan_buffers(f, c.N, k, nn.w.n))) return rc;  // (stage = k: no list is longer)
    nn.w.sorted_flags = h.sorted_flags;
    nn.w.cutoff = cutoff;
    nn.w.upper_only = 0u;
    nn.k = k;
    nn.rank = flags ? (const uint32_t *)f.R.map.p : nullptr;
    launch_sort_flags(h, f.st);
    launch_nearest(nn, f.st);
    if ((rc = nb_sizes(f, nn.w.n, c.N, out_offsets, info))) return rc;
    if (!out_entries || cap < info.total)
        return fail(ctx, RSASA_ERR_BUFFER_TOO_SMALL, "out_entries is NULL or holds fewer entries than out_offsets[n]");
    if (info.total == 0) return RSASA_OK;
    if (info.max_k > k || info.spill_atoms) return fail(ctx, RSASA_ERR_INTERNAL, "a list of the k nearest atoms is longer than k");
    if ((rc = f.reserve(f.R.entries, info.total * 8, nn.w.n.out))) return rc;
    launch_nearest_gather(nn, f.st);
    NbHost *nh = static_cast<NbHost *>(ctx->nb_host.p);
    RS_HIP(ctx, hipMemcpyAsync(&nh->info, nn.w.n.info, sizeof(NbInfo), hipMemcpyDeviceToHost, f.st));
    RS_HIP(ctx, hipMemcpyAsync(out_entries, nn.w.n.out, info.total * 8, hipMemcpyDeviceToHost, f.st));
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, hipStreamSynchronize(f.st));
    if (nh->info.mismatch) return fail(ctx, RSASA_ERR_INTERNAL, "the rows of the k nearest atoms disagree with their counts");
    return RSASA_OK;
}

// One run of the radial counts: the grid alone and the flags as in hs_run, the class bytes and the structures' offsets
// beside them, the dense table of rows ([N][n_classes][n_bins] uint32: held on the device even when only the pair
// tables are asked for - k_radial_pairs sums its rows) and, when asked for, the pair tables, zeroed on the stream;
// k_sort_kinds, k_radial_counts and k_radial_pairs; what was asked for comes back.  check_radial and check_classes have
// passed.
int rd_run(rsasa_context *ctx, const float *x, const float *y, const float *z, const float *r, const uint64_t *id, Form form,
           float probe, const uint8_t *flags, const uint8_t *classes, uint32_t n_classes, const float *edges,
           uint32_t n_bins, uint32_t *out_counts, uint64_t *out_pairs)
{
    static_assert(kRadialMaxClasses == RSASA_RADIAL_MAX_CLASSES && kRadialMaxBins == RSASA_RADIAL_MAX_BINS,
                  "the header's bounds are the kernels' bounds");
    static_assert(sizeof(RdArgs::e2) == kRadialMaxBins * sizeof(float), "an edge per bin");
    Cols c(x, y, z, r, id);
    if (int rc = entry_open(ctx, c, form, nullptr, true, out_counts || out_pairs)) return rc;
    RS_ARGS(ctx, check_radial(edges, n_bins, n_classes));
    RS_ARGS(ctx, check_classes(classes, c.N, n_classes));
    const size_t N = c.N, cells = (size_t)n_classes * n_bins, pair_bytes = c.S * n_classes * cells * 8;
    Run f(ctx);
    if (!f.open(N)) {
        if (f.rc == RSASA_OK && out_pairs) std::memset(out_pairs, 0, pair_bytes);  // (no atom: no pair)
        return f.rc;
    }
    int rc;
    HsArgs h{};
    RdArgs rd{};
    if ((rc = hs_grid(f, c, nullptr, probe, flags, h)) || (rc = f.upload(f.R.classes, classes, N, rd.classes)) ||
        (rc = f.upload(f.R.so, c.so, (c.S + 1) * 4, rd.so)) || (rc = f.reserve(f.R.table, N * cells * 4, rd.table)) ||
        (out_pairs && (rc = f.reserve(f.R.pairs, pair_bytes, rd.pairs))))
        return rc;
    if (out_pairs) RS_HIP(ctx, hipMemsetAsync(rd.pairs, 0, pair_bytes, f.st));
    rd.b = h.b;
    rd.flags = h.flags;
    rd.sorted_kinds = h.sorted_flags;
    rd.n_classes = n_classes;
    rd.n_bins = n_bins;
    for (uint32_t k = 0; k < n_bins; k++) rd.e2[k] = edges[k] * edges[k];
    launch_radial(rd, f.st);
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, download(out_counts, rd.table, N * cells * 4, f.st));
    RS_HIP(ctx, download(out_pairs, rd.pairs, pair_bytes, f.st));
    RS_HIP(ctx, hipStreamSynchronize(f.st));
    return RSASA_OK;
}

}  // namespace

extern "C" {  // (every pair forwards to its family's function: see the head of the file)

int rsasa_precompute_neighbors(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                               const uint64_t *id, size_t n_atoms, const uint32_t *active_indices, size_t n_active,
                               float probe_radius, float max_radius, uint64_t *out_offsets, rsasa_neighbor_t *out_entries,
                               size_t entries_capacity)
{
    return nb_entry(ctx, x, y, z, radius, id, Form::one(n_atoms), active_indices, n_active, probe_radius, max_radius,
                    out_offsets, out_entries, entries_capacity);
}

int rsasa_precompute_neighbors_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                                     const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                                     float probe_radius, float max_radius, uint64_t *out_offsets, rsasa_neighbor_t *out_entries,
                                     size_t entries_capacity)
{
    return nb_entry(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), nullptr, 0, probe_radius, max_radius,
                    out_offsets, out_entries, entries_capacity);
}

int rsasa_accessible_points(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                            const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, uint32_t *out_masks,
                            float *out_sasa)
{
    return pt_run(ctx, x, y, z, radius, id, Form::one(n_atoms), probe_radius, n_points, out_masks, out_sasa);
}

int rsasa_accessible_points_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                                  const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                                  float probe_radius, size_t n_points, uint32_t *out_masks, float *out_atom_sasa)
{
    return pt_run(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), probe_radius, n_points, out_masks,
                    out_atom_sasa);
}

int rsasa_exposure_vectors(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                           const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, float *out_vectors,
                           uint32_t *out_free, float *out_sasa)
{
    return ex_run(ctx, x, y, z, radius, id, Form::one(n_atoms), probe_radius, n_points, out_vectors, out_free, out_sasa);
}

int rsasa_exposure_vectors_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                                 const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                                 float probe_radius, size_t n_points, float *out_vectors, uint32_t *out_free,
                                 float *out_atom_sasa)
{
    return ex_run(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), probe_radius, n_points, out_vectors,
                    out_free, out_atom_sasa);
}

int rsasa_atom_depth(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                     const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, float *out_depth,
                     uint32_t *out_nearest, uint32_t *out_free, float *out_sasa)
{
    return dp_run(ctx, x, y, z, radius, id, Form::one(n_atoms), probe_radius, n_points, out_depth, out_nearest, out_free,
                    out_sasa);
}

int rsasa_atom_depth_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                           const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                           size_t n_points, float *out_depth, uint32_t *out_nearest, uint32_t *out_free, float *out_atom_sasa)
{
    return dp_run(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), probe_radius, n_points, out_depth,
                    out_nearest, out_free, out_atom_sasa);
}

int rsasa_surface_components(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                             const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, float link,
                             uint64_t *out_dot_offsets, uint32_t *out_labels, size_t labels_capacity, uint32_t *out_free,
                             float *out_sasa)
{
    return cc_run(ctx, x, y, z, radius, id, Form::one(n_atoms), probe_radius, n_points, link, out_dot_offsets, out_labels,
                    labels_capacity, out_free, out_sasa);
}

int rsasa_surface_components_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                                   const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                                   float probe_radius, size_t n_points, float link, uint64_t *out_dot_offsets,
                                   uint32_t *out_labels, size_t labels_capacity, uint32_t *out_free, float *out_atom_sasa)
{
    return cc_run(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), probe_radius, n_points, link,
                    out_dot_offsets, out_labels, labels_capacity, out_free, out_atom_sasa);
}

int rsasa_dot_links(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                    const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, float link,
                    uint64_t *out_dot_offsets, uint64_t *out_n_links, uint64_t *out_link_offsets, size_t dots_capacity,
                    rsasa_within_t *out_entries, size_t entries_capacity, uint32_t *out_free, float *out_sasa)
{
    return dl_run(ctx, x, y, z, radius, id, Form::one(n_atoms), probe_radius, n_points, link, out_dot_offsets, out_n_links,
                    out_link_offsets, dots_capacity, out_entries, entries_capacity, out_free, out_sasa);
}

int rsasa_dot_links_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                          const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                          size_t n_points, float link, uint64_t *out_dot_offsets, uint64_t *out_n_links,
                          uint64_t *out_link_offsets, size_t dots_capacity, rsasa_within_t *out_entries,
                          size_t entries_capacity, uint32_t *out_free, float *out_atom_sasa)
{
    return dl_run(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), probe_radius, n_points, link,
                    out_dot_offsets, out_n_links, out_link_offsets, dots_capacity, out_entries, entries_capacity, out_free,
                    out_atom_sasa);
}

int rsasa_dot_geodesics(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                        const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, float link,
                        const uint8_t *seeds, size_t n_seed_bytes, float limit, uint64_t *out_dot_offsets, float *out_dist,
                        uint32_t *out_source, uint32_t *out_free, float *out_sasa)
{
    return dg_run(ctx, x, y, z, radius, id, Form::one(n_atoms), probe_radius, n_points, link, seeds, n_seed_bytes, limit,
                    out_dot_offsets, out_dist, out_source, out_free, out_sasa);
}

int rsasa_dot_geodesics_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                              const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                              size_t n_points, float link, const uint8_t *seeds, size_t n_seed_bytes, float limit,
                              uint64_t *out_dot_offsets, float *out_dist, uint32_t *out_source, uint32_t *out_free,
                              float *out_atom_sasa)
{
    return dg_run(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), probe_radius, n_points, link, seeds,
                    n_seed_bytes, limit, out_dot_offsets, out_dist, out_source, out_free, out_atom_sasa);
}

int rsasa_context_geodesic_rounds(rsasa_context_t *ctx, uint32_t *out_rounds)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (!out_rounds) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "out_rounds is NULL");
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    out_rounds[0] = ctx->gd_rounds[0];
    out_rounds[1] = ctx->gd_rounds[1];
    return RSASA_OK;
}

int rsasa_dot_patches(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                      const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, float link, float spacing,
                      uint32_t max_centres, uint64_t *out_dot_offsets, uint64_t *out_centre_bound,
                      uint64_t *out_centre_offsets, uint32_t *out_centres, float *out_cover, size_t centres_capacity,
                      float *out_dist, uint32_t *out_source, size_t dots_capacity, uint32_t *out_free, float *out_sasa)
{
    return ps_run(ctx, x, y, z, radius, id, Form::one(n_atoms), probe_radius, n_points, link, spacing, max_centres,
                    out_dot_offsets, out_centre_bound, out_centre_offsets, out_centres, out_cover, centres_capacity, out_dist,
                    out_source, dots_capacity, out_free, out_sasa);
}

int rsasa_dot_patches_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                            const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                            size_t n_points, float link, float spacing, uint32_t max_centres, uint64_t *out_dot_offsets,
                            uint64_t *out_centre_bound, uint64_t *out_centre_offsets, uint32_t *out_centres, float *out_cover,
                            size_t centres_capacity, float *out_dist, uint32_t *out_source, size_t dots_capacity,
                            uint32_t *out_free, float *out_atom_sasa)
{
    return ps_run(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), probe_radius, n_points, link, spacing,
                    max_centres, out_dot_offsets, out_centre_bound, out_centre_offsets, out_centres, out_cover, centres_capacity,
                    out_dist, out_source, dots_capacity, out_free, out_atom_sasa);
}

int rsasa_context_patch_stats(rsasa_context_t *ctx, uint64_t *out_stats)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (!out_stats) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "out_stats is NULL");
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    for (int k = 0; k < 3; k++) out_stats[k] = ctx->ps_stats[k];
    return RSASA_OK;
}

int rsasa_dot_crowding(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                       const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, const uint8_t *flags,
                       const float *edges, uint32_t n_bins, uint64_t *out_dot_offsets, uint32_t *out_counts,
                       size_t counts_capacity, uint32_t *out_free, float *out_sasa)
{
    return dc_run(ctx, x, y, z, radius, id, Form::one(n_atoms), probe_radius, n_points, flags, edges, n_bins, out_dot_offsets,
                    out_counts, counts_capacity, out_free, out_sasa);
}

int rsasa_dot_crowding_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                             const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                             size_t n_points, const uint8_t *flags, const float *edges, uint32_t n_bins,
                             uint64_t *out_dot_offsets, uint32_t *out_counts, size_t counts_capacity, uint32_t *out_free,
                             float *out_atom_sasa)
{
    return dc_run(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), probe_radius, n_points, flags, edges,
                    n_bins, out_dot_offsets, out_counts, counts_capacity, out_free, out_atom_sasa);
}

int rsasa_dot_fields(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                     const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, const uint8_t *flags,
                     const float *weights, const uint8_t *kinds, uint32_t n_channels, float cutoff, uint64_t *out_dot_offsets,
                     int64_t *out_sums, size_t sums_capacity, uint32_t *out_free, float *out_sasa)
{
    return fd_run(ctx, x, y, z, radius, id, Form::one(n_atoms), probe_radius, n_points, flags, weights, kinds, n_channels,
                    cutoff, out_dot_offsets, out_sums, sums_capacity, out_free, out_sasa);
}

int rsasa_dot_fields_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                           const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                           size_t n_points, const uint8_t *flags, const float *weights, const uint8_t *kinds,
                           uint32_t n_channels, float cutoff, uint64_t *out_dot_offsets, int64_t *out_sums,
                           size_t sums_capacity, uint32_t *out_free, float *out_atom_sasa)
{
    return fd_run(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), probe_radius, n_points, flags, weights,
                    kinds, n_channels, cutoff, out_dot_offsets, out_sums, sums_capacity, out_free, out_atom_sasa);
}

int rsasa_dot_curvature(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                        const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, float reach,
                        uint64_t *out_dot_offsets, uint32_t *out_pairs, int64_t *out_moments, size_t dots_capacity,
                        uint32_t *out_free, float *out_sasa)
{
    return cv_run(ctx, x, y, z, radius, id, Form::one(n_atoms), probe_radius, n_points, reach, out_dot_offsets, out_pairs,
                  out_moments, dots_capacity, out_free, out_sasa);
}

int rsasa_dot_curvature_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                              const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                              size_t n_points, float reach, uint64_t *out_dot_offsets, uint32_t *out_pairs,
                              int64_t *out_moments, size_t dots_capacity, uint32_t *out_free, float *out_atom_sasa)
{
    return cv_run(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), probe_radius, n_points, reach,
                  out_dot_offsets, out_pairs, out_moments, dots_capacity, out_free, out_atom_sasa);
}

int rsasa_dot_enclosure(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                        const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, const uint8_t *flags,
                        float reach, uint32_t n_dirs, uint64_t *out_dot_offsets, uint32_t *out_blocked,
                        size_t blocked_capacity, uint32_t *out_free, float *out_sasa)
{
    return de_run(ctx, x, y, z, radius, id, Form::one(n_atoms), probe_radius, n_points, flags, reach, n_dirs, out_dot_offsets,
                    out_blocked, blocked_capacity, out_free, out_sasa);
}

int rsasa_dot_enclosure_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                              const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                              size_t n_points, const uint8_t *flags, float reach, uint32_t n_dirs,
                              uint64_t *out_dot_offsets, uint32_t *out_blocked, size_t blocked_capacity, uint32_t *out_free,
                              float *out_atom_sasa)
{
    return de_run(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), probe_radius, n_points, flags, reach,
                    n_dirs, out_dot_offsets, out_blocked, blocked_capacity, out_free, out_atom_sasa);
}

int rsasa_half_sphere_exposure(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                               const uint64_t *id, size_t n_atoms, float probe_radius, const float *dirs, const uint8_t *flags,
                               float cutoff, uint32_t *out_up, uint32_t *out_down)
{
    return hs_run(ctx, x, y, z, radius, id, Form::one(n_atoms), probe_radius, dirs, flags, cutoff, out_up, out_down);
}

int rsasa_half_sphere_exposure_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                                     const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                                     float probe_radius, const float *dirs, const uint8_t *flags, float cutoff,
                                     uint32_t *out_up, uint32_t *out_down)
{
    return hs_run(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), probe_radius, dirs, flags, cutoff,
                    out_up, out_down);
}

int rsasa_atoms_within(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                       const uint64_t *id, size_t n_atoms, float probe_radius, const uint8_t *flags, float cutoff,
                       int upper_only, uint64_t *out_offsets, rsasa_within_t *out_entries, size_t entries_capacity)
{
    return wn_run(ctx, x, y, z, radius, id, Form::one(n_atoms), probe_radius, flags, cutoff, upper_only, out_offsets,
                    out_entries, entries_capacity);
}

int rsasa_atoms_within_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                             const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                             const uint8_t *flags, float cutoff, int upper_only, uint64_t *out_offsets,
                             rsasa_within_t *out_entries, size_t entries_capacity)
{
    return wn_run(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), probe_radius, flags, cutoff,
                    upper_only, out_offsets, out_entries, entries_capacity);
}

int rsasa_nearest_atoms(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                        const uint64_t *id, size_t n_atoms, float probe_radius, const uint8_t *flags, uint32_t k, float cutoff,
                        uint64_t *out_offsets, rsasa_within_t *out_entries, size_t entries_capacity)
{
    return nn_run(ctx, x, y, z, radius, id, Form::one(n_atoms), probe_radius, flags, k, cutoff, out_offsets, out_entries,
                    entries_capacity);
}

int rsasa_nearest_atoms_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                              const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                              const uint8_t *flags, uint32_t k, float cutoff, uint64_t *out_offsets,
                              rsasa_within_t *out_entries, size_t entries_capacity)
{
    return nn_run(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), probe_radius, flags, k, cutoff,
                    out_offsets, out_entries, entries_capacity);
}

int rsasa_radial_counts(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                        const uint64_t *id, size_t n_atoms, float probe_radius, const uint8_t *flags, const uint8_t *classes,
                        uint32_t n_classes, const float *edges, uint32_t n_bins, uint32_t *out_counts, uint64_t *out_pairs)
{
    return rd_run(ctx, x, y, z, radius, id, Form::one(n_atoms), probe_radius, flags, classes, n_classes, edges, n_bins,
                    out_counts, out_pairs);
}

int rsasa_radial_counts_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                              const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures, float probe_radius,
                              const uint8_t *flags, const uint8_t *classes, uint32_t n_classes, const float *edges,
                              uint32_t n_bins, uint32_t *out_counts, uint64_t *out_pairs)
{
    return rd_run(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), probe_radius, flags, classes,
                    n_classes, edges, n_bins, out_counts, out_pairs);
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
    return ct_run(ctx, x, y, z, radius, id, Form::one(n_atoms), probe_radius, n_points, out_offsets, out_entries, out_covered,
                    out_exclusive, entries_capacity, out_sasa);
}

int rsasa_contact_points_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                               const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                               float probe_radius, size_t n_points, uint64_t *out_offsets, rsasa_neighbor_t *out_entries,
                               uint32_t *out_covered, uint32_t *out_exclusive, size_t entries_capacity,
                               float *out_atom_sasa)
{
    return ct_run(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), probe_radius, n_points, out_offsets,
                    out_entries, out_covered, out_exclusive, entries_capacity, out_atom_sasa);
}

int rsasa_contact_owners(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                         const uint64_t *id, size_t n_atoms, float probe_radius, size_t n_points, uint64_t *out_offsets,
                         rsasa_neighbor_t *out_entries, uint32_t *out_owned, size_t entries_capacity, uint32_t *out_owner,
                         float *out_sasa)
{
    return co_run(ctx, x, y, z, radius, id, Form::one(n_atoms), probe_radius, n_points, out_offsets, out_entries, out_owned,
                    entries_capacity, out_owner, out_sasa);
}

int rsasa_contact_owners_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                               const uint64_t *id, const uint32_t *structure_offsets, size_t n_structures,
                               float probe_radius, size_t n_points, uint64_t *out_offsets, rsasa_neighbor_t *out_entries,
                               uint32_t *out_owned, size_t entries_capacity, uint32_t *out_owner, float *out_atom_sasa)
{
    return co_run(ctx, x, y, z, radius, id, Form::many(structure_offsets, n_structures), probe_radius, n_points, out_offsets,
                    out_entries, out_owned, entries_capacity, out_owner, out_atom_sasa);
}

int rsasa_group_contacts(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                         const uint64_t *id, const uint32_t *group, size_t n_atoms, float probe_radius, size_t n_points,
                         uint64_t *out_offsets, uint32_t *out_groups, uint32_t *out_buried, uint32_t *out_only,
                         size_t rows_capacity, uint32_t *out_self_free, uint32_t *out_free, float *out_sasa)
{
    return gp_run(ctx, x, y, z, radius, id, group, Form::one(n_atoms), probe_radius, n_points, out_offsets, out_groups,
                    out_buried, out_only, rows_capacity, out_self_free, out_free, out_sasa);
}

int rsasa_group_contacts_batch(rsasa_context_t *ctx, const float *x, const float *y, const float *z, const float *radius,
                               const uint64_t *id, const uint32_t *group, const uint32_t *structure_offsets,
                               size_t n_structures, float probe_radius, size_t n_points, uint64_t *out_offsets,
                               uint32_t *out_groups, uint32_t *out_buried, uint32_t *out_only, size_t rows_capacity,
                               uint32_t *out_self_free, uint32_t *out_free, float *out_atom_sasa)
{
    return gp_run(ctx, x, y, z, radius, id, group, Form::many(structure_offsets, n_structures), probe_radius, n_points,
                    out_offsets, out_groups, out_buried, out_only, rows_capacity, out_self_free, out_free, out_atom_sasa);
}

}  // extern "C"
