// C ABI of the engine (include/rustsasa_amd.h): contexts, HBM workspace,
// sphere lattice cache, batch enqueue / wait.  Host code only; the kernels
// live in kernels.hip.  There is no CPU compute path in this library.
#include "engine_internal.h"
#include "sasa_checks.h"

namespace rsasa {

// The library's measurement switches (kernel choice, sub-batch sizes, copy experiments: INTEGRATION.md 7) are read only
// when the process sets RSASA_TUNING=1: a production program's numerics path does not depend on stray environment
// variables.  (RSASA_NUMA=0, which only says where threads may run, is read regardless.)
const char *tuning_env(const char *name)
{
    static const bool on = [] { const char *v = std::getenv("RSASA_TUNING"); return v && std::atoi(v) != 0; }();
    return on ? std::getenv(name) : nullptr;
}

// Golden-section spiral (reference src/lib.rs:43-66, constants
// src/utils/consts.rs:18-19), f32 at every step, libm transcendentals.
// Computed on the host and uploaded: the occlusion decision is integer valued,
// so the table must be bit-identical to what the reference's host would use.
void generate_sphere_points(size_t n, float *x, float *y, float *z)
{
    const float pi = 3.14159274101257324219f;
    const float angle_increment = (2.0f * pi) * 1.618034f;
    const float inv_n = 1.0f / (float)n;
    for (size_t i = 0; i < n; i++) {
        const float fi = (float)i;
        const float t = fi * inv_n;
        const float inclination = acosf(1.0f - 2.0f * t);
        const float azimuth = angle_increment * fi;
        const float si = sinf(inclination);
        x[i] = si * cosf(azimuth);
        y[i] = si * sinf(azimuth);
        z[i] = cosf(inclination);
    }
}

// ---- sphere points in patches (point counts above 128 only) ----
// Every kernel only COUNTS points, so the order of the points that share a rule is free.  With many points the
// matrix-core kernel first tests whole patches of 16 points against the nearest candidates (one candidate whose
// cap holds the patch kills all 16: occlusion_mx.inc); for that the fused-rule points [0, n_fused) are reordered so
// that every aligned run of 16 is a compact patch of the sphere (recursive bisection along the widest axis, left
// halves in multiples of 16).  The remainder points keep their places behind them.
static void bisect_points(std::vector<uint32_t> &idx, size_t lo, size_t hi, const float *x, const float *y, const float *z)
{
    const size_t n = hi - lo;
    if (n <= 16) return;
    float mn[3] = {2.f, 2.f, 2.f}, mx[3] = {-2.f, -2.f, -2.f};
    for (size_t i = lo; i < hi; i++) {
        const float c[3] = {x[idx[i]], y[idx[i]], z[idx[i]]};
        for (int k = 0; k < 3; k++) { mn[k] = std::min(mn[k], c[k]); mx[k] = std::max(mx[k], c[k]); }
    }
    int ax = 0;
    for (int k = 1; k < 3; k++)
        if (mx[k] - mn[k] > mx[ax] - mn[ax]) ax = k;
    const float *c = ax == 0 ? x : ax == 1 ? y : z;
    std::sort(idx.begin() + (long)lo, idx.begin() + (long)hi,
              [c](uint32_t a, uint32_t b) { return c[a] != c[b] ? c[a] < c[b] : a < b; });
    const size_t left = ((n + 15) / 16 / 2) * 16;
    bisect_points(idx, lo, lo + left, x, y, z);
    bisect_points(idx, lo + left, hi, x, y, z);
}

static uint16_t f16_bits(_Float16 h)
{
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}
// smallest f16 >= v (v finite, non-negative, below the f16 range's end)
static uint16_t f16_round_up(float v)
{
    _Float16 h = (_Float16)v;
    uint16_t u = f16_bits(h);
    if ((float)h < v) u++;  // next representable value (positive numbers: the bit pattern is monotone)
    return u;
}

NodeCpus device_node_cpus(int device)
{
    NodeCpus nc;
    CPU_ZERO(&nc.set);
    if (const char *v = std::getenv("RSASA_NUMA"))
        if (std::atoi(v) == 0) return nc;
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf) - 1, device) != hipSuccess) {
        (void)hipGetLastError();
        return nc;
    }
    for (char *c = bdf; *c; c++) *c = (char)std::tolower((unsigned char)*c);
    const std::string base = std::string("/sys/bus/pci/devices/") + bdf;
    FILE *f = std::fopen((base + "/numa_node").c_str(), "r");
    if (!f) return nc;
    int node = -1;
    const int got = std::fscanf(f, "%d", &node);
    std::fclose(f);
    if (got != 1 || node < 0) return nc;
    f = std::fopen((base + "/local_cpulist").c_str(), "r");
    if (!f) return nc;
    char buf[4096] = {0};
    const bool ok = std::fgets(buf, sizeof(buf), f) != nullptr;
    std::fclose(f);
    if (!ok) return nc;
    int n_set = 0;
    for (char *q = buf; *q;) {  // "0-31,64-95"
        char *end = nullptr;
        const long lo = std::strtol(q, &end, 10);
        if (end == q) break;
        long hi = lo;
        q = end;
        if (*q == '-') {
            hi = std::strtol(q + 1, &end, 10);
            q = end;
        }
        for (long c = lo; c <= hi && c < CPU_SETSIZE; c++) { CPU_SET((int)c, &nc.set); n_set++; }
        while (*q == ',' || *q == ' ' || *q == '\n') q++;
    }
    nc.node = node;
    nc.valid = n_set > 0;
    return nc;
}

// Binds a thread to `nc` (intersected with what the thread may run on); false when there is nothing to do.
bool bind_thread_to(pthread_t th, const NodeCpus &nc)
{
    if (!nc.valid) return false;
    cpu_set_t cur, want;
    if (pthread_getaffinity_np(th, sizeof(cur), &cur) != 0) return false;
    CPU_AND(&want, &cur, &nc.set);
    if (CPU_COUNT(&want) == 0) return false;
    return pthread_setaffinity_np(th, sizeof(want), &want) == 0;
}

}  // namespace rsasa

namespace rsasa {

int fail(rsasa_context *ctx, int code, const char *what, hipError_t e)
{
    if (ctx) {
        // several threads may share a context (host/files_mode.cpp runs two workers on one): the message
        // is written and read under the context's (recursive) mutex
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        ctx->last_error = what;
        if (e != hipSuccess) {
            ctx->last_error += ": ";
            ctx->last_error += hipGetErrorString(e);
        }
    }
    return code;
}

LinkTurn g_link[64];

// Grows `b` to at least `bytes` (contents are NOT preserved).  The caller has
// already drained the stream if the buffer may be in use.
int reserve(rsasa_context *ctx, DeviceBuffer &b, size_t bytes)
{
    if (bytes <= b.cap) return RSASA_OK;
    if (b.p) {
        // the buffer may be read by work on any of the context's streams (two launch streams, a caller's stream of a
        // batch in flight, the copy streams of the pipelined host path): drain them all, not only the first
        RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->stream2) RS_HIP(ctx, hipStreamSynchronize(ctx->stream2));
        if (ctx->side_stream) RS_HIP(ctx, hipStreamSynchronize(ctx->side_stream));
        if (ctx->copy_stream) RS_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
        if (ctx->d2h_stream) RS_HIP(ctx, hipStreamSynchronize(ctx->d2h_stream));
        for (const Pending &pd : ctx->pending)
            if (pd.active && pd.stream && pd.stream != ctx->stream && pd.stream != ctx->stream2) RS_HIP(ctx, hipStreamSynchronize(pd.stream));
        RS_HIP(ctx, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    size_t want = bytes + bytes / 4 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        want = bytes;
        e = hipMalloc(&b.p, want);
    }
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(ctx, RSASA_ERR_OUT_OF_MEMORY, "hipMalloc(workspace)", e);
    }
    b.cap = want;
    return RSASA_OK;
}

void release(DeviceBuffer &b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

int get_lattice(rsasa_context *ctx, size_t n_points, Lattice *out)
{
    const auto key = std::make_pair(n_points, ctx->simd_width);
    auto it = ctx->lattices.find(key);
    if (it == ctx->lattices.end()) {
        // the cache holds the few point counts a program uses; a sweep over many counts must not
        // pin 28 bytes per point per count forever
        size_t cached_bytes = 0;
        for (const auto &kv : ctx->lattices) cached_bytes += 7 * sizeof(float) * (size_t)kv.second.padded + 16 * (size_t)kv.second.n_patches + 1536;
        if (ctx->lattices.size() >= 16 || cached_bytes > (64u << 20)) {
            RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
            for (const Pending &pd : ctx->pending)
                if (pd.active && pd.stream != ctx->stream) RS_HIP(ctx, hipStreamSynchronize(pd.stream));
            for (auto &kv : ctx->lattices)
                if (kv.second.d) (void)hipFree(kv.second.d);
            ctx->lattices.clear();
        }
        const uint32_t padded = (uint32_t)((n_points + 63) / 64 * 64);
        const uint32_t n_patches = n_points > 128 ? (uint32_t)((n_points + 15) / 16) : 0u;
        const uint32_t patches_padded = (n_patches + 63u) / 64u * 64u;
        const uint32_t tab_at = 7 * padded + 4 * patches_padded;
        std::vector<float> h((size_t)tab_at + mx_tab_floats((uint32_t)n_points), 0.0f);  // x | y | z | (x, y, z, 0) records | patches | mx_tab
        generate_sphere_points(n_points, h.data(), h.data() + padded, h.data() + 2 * (size_t)padded);
        if (n_patches) {
            // compact patches: permute the fused-rule points (see bisect_points), then one table entry per patch:
            // (cz, cy | cx, -1 | eps, 0 | 0, 0) as f16 - centre c (unit, rounded to nearest) and eps >= the largest
            // distance from c to a point of the patch (+ the centre's rounding), rounded up
            const size_t n_fused = n_points - n_points % (size_t)ctx->simd_width;
            std::vector<uint32_t> idx(n_fused);
            for (size_t i = 0; i < n_fused; i++) idx[i] = (uint32_t)i;
            float *px = h.data(), *py = h.data() + padded, *pz = h.data() + 2 * (size_t)padded;
            bisect_points(idx, 0, n_fused, px, py, pz);
            std::vector<float> t(3 * n_fused);
            for (size_t i = 0; i < n_fused; i++) { t[3 * i] = px[idx[i]]; t[3 * i + 1] = py[idx[i]]; t[3 * i + 2] = pz[idx[i]]; }
            for (size_t i = 0; i < n_fused; i++) { px[i] = t[3 * i]; py[i] = t[3 * i + 1]; pz[i] = t[3 * i + 2]; }
            uint16_t *pt = reinterpret_cast<uint16_t *>(h.data() + 7 * (size_t)padded);
            for (uint32_t k = 0; k < n_patches; k++) {
                const size_t b = 16 * (size_t)k, e = std::min(b + 16, n_points);
                double c[3] = {0, 0, 0};
                for (size_t i = b; i < e; i++) { c[0] += px[i]; c[1] += py[i]; c[2] += pz[i]; }
                const double len = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
                _Float16 c16[3];
                for (int q = 0; q < 3; q++) c16[q] = (_Float16)(float)(len > 0 ? c[q] / len : (q == 2 ? 1.0 : 0.0));
                double eps = 0;  // against the centre the kernel will actually use (the f16 one)
                for (size_t i = b; i < e; i++) {
                    const double dx = px[i] - (double)(float)c16[0], dy = py[i] - (double)(float)c16[1], dz = pz[i] - (double)(float)c16[2];
                    eps = std::max(eps, std::sqrt(dx * dx + dy * dy + dz * dz));
                }
                uint16_t *en = pt + 8 * (size_t)k;
                en[0] = f16_bits(c16[2]); en[1] = f16_bits(c16[1]); en[2] = f16_bits(c16[0]); en[3] = f16_bits((_Float16)-1.0f);
                en[4] = f16_round_up((float)(eps * 1.001 + 1e-4)); en[5] = en[6] = en[7] = 0;
            }
            // (entries of patches that do not exist: centre 0, -1 -> 0, eps 0: all zero, never looked at)
        }
        for (size_t i = 0; i < n_points; i++) {
            float *r4 = h.data() + 3 * (size_t)padded + 4 * i;
            r4[0] = h[i];
            r4[1] = h[padded + i];
            r4[2] = h[2 * (size_t)padded + i];
        }
        if (n_points <= 128) {
            // the matrix-core kernel's operand tables (device_types.h mx_tab_floats)
            const uint32_t np = 16u * mx_tab_tiles((uint32_t)n_points), nps = np + 16u;
            float *t = h.data() + tab_at;
            uint16_t *t16 = reinterpret_cast<uint16_t *>(t + 4 * (size_t)nps);
            for (size_t i = 0; i < n_points; i++) {
                const float px = h[i], py = h[padded + i], pz = h[2 * (size_t)padded + i];
                t[i] = pz; t[nps + i] = py; t[2 * (size_t)nps + i] = px; t[3 * (size_t)nps + i] = -1.0f;
                t16[4 * i] = f16_bits((_Float16)pz); t16[4 * i + 1] = f16_bits((_Float16)py);
                t16[4 * i + 2] = f16_bits((_Float16)px); t16[4 * i + 3] = f16_bits((_Float16)-1.0f);
            }
        }
        LatticeEntry e;
        e.padded = padded;
        e.n_patches = n_patches;
        e.mx_tab_at = n_points <= 128 ? tab_at : 0u;
        RS_HIP(ctx, hipMalloc((void **)&e.d, h.size() * sizeof(float)));
        hipError_t err = hipMemcpy(e.d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
        if (err != hipSuccess) {
            (void)hipFree(e.d);
            return fail(ctx, RSASA_ERR_HIP, "hipMemcpy(lattice)", err);
        }
        it = ctx->lattices.emplace(key, e).first;
    }
    out->x = it->second.d;
    out->y = it->second.d + it->second.padded;
    out->z = it->second.d + 2 * (size_t)it->second.padded;
    out->xyz4 = (const float4 *)(it->second.d + 3 * (size_t)it->second.padded);
    out->patches = it->second.n_patches ? (const uint4 *)(it->second.d + 7 * (size_t)it->second.padded) : nullptr;
    out->n_patches = it->second.n_patches;
    out->mx_tab = it->second.mx_tab_at ? it->second.d + it->second.mx_tab_at : nullptr;
    out->n_points = (uint32_t)n_points;
    out->n_fused = (uint32_t)(n_points - n_points % (size_t)ctx->simd_width);
    return RSASA_OK;
}

// Enqueues the whole pipeline for the batch `pd` on its stream, using host slot `hs`.
// The streams beside the launch stream are created on first use.  The runtime multiplexes a
// process's streams onto a few hardware queues in creation order: a context that only serves
// per-structure calls should hold ONE stream, or the launch streams of several contexts (one per host
// thread) all land on the same queue and their kernels run one after the other.
//
// own_queues (the worker contexts of a stream of host batches): a stream created with a CU mask gets a hardware queue
// of its own instead of one from the shared pool, and a mask of every CU restricts nothing.  Streams that share a
// queue run their packets in order - the barrier that makes one worker's kernels wait for its upload would hold the
// other worker's kernels behind it, and the stream of batches would not overlap (measured: 6.6 ms per proteome batch
// on pooled queues that collide, 4.4 on queues of their own).
hipError_t new_stream(rsasa_context *ctx, hipStream_t *out, int level)
{
    if (ctx->own_queues >= level) {
        int n_cu = 0;
        uint32_t mask[16] = {};
        if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device) == hipSuccess && n_cu > 0 && n_cu <= 512) {
            for (int c = 0; c < n_cu; c++) mask[c / 32] |= 1u << (c % 32);
            // (such a stream is a BLOCKING one: work on the process's legacy default stream and work on it wait for each
            // other - ordering a caller may not expect, never a wrong result)
            if (hipExtStreamCreateWithCUMask(out, (uint32_t)(n_cu + 31) / 32, mask) == hipSuccess) return hipSuccess;
            (void)hipGetLastError();  // (a device that does not take the mask: a pooled queue then)
        }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}

int ensure_side_stream(rsasa_context *ctx)
{
    if (!ctx->side_stream) RS_HIP(ctx, new_stream(ctx, &ctx->side_stream.h, 2));
    return RSASA_OK;
}

int ensure_copy_streams(rsasa_context *ctx)
{
    if (!ctx->copy_stream) RS_HIP(ctx, new_stream(ctx, &ctx->copy_stream.h, 1));
    if (!ctx->d2h_stream) RS_HIP(ctx, new_stream(ctx, &ctx->d2h_stream.h, 1));
    return RSASA_OK;
}

SegmentCount count_segments(const uint32_t *so, size_t S)
{
    SegmentCount c;
    for (size_t s = 0; s < S; s++) {
        const uint32_t n = so[s + 1] - so[s];
        c.n_seg += (n + kSegmentAtoms - 1) / kSegmentAtoms;
        c.n_large += n > kIdAtomsSmall && n <= kIdAtomsLarge;
        c.has_tail |= n >= kLdsMaxAtoms;
    }
    return c;
}

void write_segments(const uint32_t *so, size_t S, Segment *out, uint32_t *large)
{
    for (size_t s = 0; s < S; s++) {
        const uint32_t b = so[s], e = so[s + 1];
        if (large && e - b > kIdAtomsSmall && e - b <= kIdAtomsLarge) *large++ = (uint32_t)s;
        for (uint32_t a = b; a < e; a += kSegmentAtoms)
            *out++ = Segment{(uint32_t)s, a, std::min(e, a + kSegmentAtoms), a != b ? 1u : 0u};
    }
}

}  // namespace rsasa

int rsasa_context::Workspace::reserve_sorted(rsasa_context *ctx, size_t N, size_t cell_words, bool with_id)
{
    int rc;
    has_id = with_id;
    if ((rc = reserve(ctx, sid_sorted, std::max<size_t>(N, 1) * 4))) return rc;
    if ((rc = reserve(ctx, rank_of, std::max<size_t>(N, 1) * 4))) return rc;
    if ((rc = reserve(ctx, cells, cell_words * 4))) return rc;
    if ((rc = reserve(ctx, sorted_xyzr, std::max<size_t>(N, 1) * 16))) return rc;
    if ((rc = reserve(ctx, sorted_orig, std::max<size_t>(N, 1) * 4))) return rc;
    if (has_id && (rc = reserve(ctx, sorted_id32, std::max<size_t>(N, 1) * 4))) return rc;
    return RSASA_OK;
}

void rsasa_context::Workspace::sorted_view(BatchView &v) const
{
    v.sid_sorted = (uint32_t *)sid_sorted.p;
    v.cell_of = (uint32_t *)cell_of.p;  // (reserved by reserve_grid for a batch with a tail: batch-wide binning only)
    v.rank_of = (uint32_t *)rank_of.p;
    v.cells = (uint32_t *)cells.p;
    v.sorted_xyzr = (float4 *)sorted_xyzr.p;
    v.sorted_orig = (uint32_t *)sorted_orig.p;
    v.sorted_id32 = has_id ? (uint32_t *)sorted_id32.p : nullptr;
}

int rsasa_context::Workspace::reserve_grid(rsasa_context *ctx, size_t N, size_t S, size_t n_seg_all, uint64_t &capacity, bool has_tail,
                                           bool with_id)
{
    int rc;
    if (capacity == 0) capacity = std::max<uint64_t>(1u << 16, 20ull * N + 512ull * S);
    capacity = std::min<uint64_t>(capacity, 0xFFFFFFF0ull);
    cell_capacity = capacity;
    // one k_sort_window workgroup per window of kWindowCells 16-bit cell entries (two per entry of the cell
    // array), at most one partly filled window per structure: whatever fits the cell array fits this list
    window_capacity = (uint32_t)std::min<uint64_t>(2 * cell_capacity / kWindowCells + S + 1, 0x7FFFFFFFull);
    if ((rc = reserve(ctx, segments, std::max<size_t>(n_seg_all, 1) * sizeof(Segment)))) return rc;
    if ((rc = reserve(ctx, acc, std::max<size_t>(S, 1) * sizeof(StructAcc)))) return rc;
    if ((rc = reserve(ctx, grids, std::max<size_t>(S, 1) * sizeof(StructGrid)))) return rc;
    if ((rc = reserve(ctx, grid_sums, (std::max<size_t>(S, 1) + 255) / 256 * 32))) return rc;
    if (has_tail && (rc = reserve(ctx, cell_of, std::max<size_t>(N, 1) * 4))) return rc;  // (batch-wide binning only)
    if ((rc = reserve(ctx, windows, (size_t)window_capacity * sizeof(uint4)))) return rc;
    if ((rc = reserve(ctx, scan_sums, kScanBlocks * 4))) return rc;
    if ((rc = reserve(ctx, status, sizeof(BatchStatus)))) return rc;
    // + 1 end marker, + 3: k_zero_cells / k_scan_* access whole 16-byte vectors up to the end marker
    return reserve_sorted(ctx, N, (size_t)(cell_capacity + 1 + 3), with_id);
}

void rsasa_context::Workspace::grid_view(BatchView &v) const
{
    sorted_view(v);
    v.segments = (const Segment *)segments.p;
    v.acc = (StructAcc *)acc.p;
    v.grids = (StructGrid *)grids.p;
    v.grid_sums = (GridSums *)grid_sums.p;
    v.cell_capacity = cell_capacity;
    v.windows = (uint4 *)windows.p;
    v.window_capacity = window_capacity;
    v.scan_block_sums = (uint32_t *)scan_sums.p;
    v.status = (BatchStatus *)status.p;
}

int rsasa_context::Workspace::reserve_occlusion(rsasa_context *ctx, const Lattice &lat, size_t N, bool with_id, bool bitmaps,
                                                bool own_values)
{
    int rc;
    // (the matrix-core kernel works on the id folds: no sorted copy of the 64-bit ids then)
    keep_ids = with_id && !occlusion_uses_mx(ctx->tuning, lat, (uint32_t)N);
    id_bitmaps = bitmaps;
    ids_seg_words = bitmaps ? (uint32_t)((N + 2047) / 2048) : 0u;  // (BatchView::ids_seg: a bit per 64 atoms, two bitmaps)
    own_atom_sasa = own_values;
    if ((rc = reserve(ctx, deferred_list, std::max<size_t>(N, 1) * 4))) return rc;
    if ((rc = reserve(ctx, claim, kClaimBytes))) return rc;
    if (id_bitmaps && (rc = reserve(ctx, ids_seg, 2 * (size_t)ids_seg_words * 4 + 16))) return rc;
    if (keep_ids && (rc = reserve(ctx, sorted_id, std::max<size_t>(N, 1) * 8))) return rc;
    if (own_atom_sasa && (rc = reserve(ctx, atom_sasa, std::max<size_t>(N, 1) * 4))) return rc;
    return RSASA_OK;
}

void rsasa_context::Workspace::occlusion_view(BatchView &v) const
{
    v.deferred_list = (uint32_t *)deferred_list.p;
    v.claim = (uint32_t *)claim.p;
    v.ids_seg = id_bitmaps ? (uint32_t *)ids_seg.p : nullptr;
    v.ids_seg_words = ids_seg_words;
    v.sorted_id = keep_ids ? (uint64_t *)sorted_id.p : nullptr;
    if (own_atom_sasa) v.atom_sasa = (float *)atom_sasa.p;
}

namespace rsasa {

int grid_input_error(rsasa_context *ctx, const BatchStatus &stt)
{
    if (stt.grid_too_large)
        return fail(ctx, RSASA_ERR_GRID_TOO_LARGE, "a structure's cell grid exceeds 2^31 cells (coordinates too sparse)");
    if (stt.bad_input)
        return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "probe_radius + max radius must be a positive finite number");
    return RSASA_OK;
}

// the cell array was too small for a batch that needs total_cells: a larger one, three times at the most
int grid_grow(rsasa_context *ctx, uint64_t total_cells, int attempts, uint64_t &cell_capacity)
{
    if (total_cells >= 0xFFFFFFF0ull || attempts >= 3)
        return fail(ctx, RSASA_ERR_GRID_TOO_LARGE, "batch needs more than 2^32 grid cells; split it");
    cell_capacity = total_cells + total_cells / 8 + 1024;
    return kGridAgain;
}

int grid_verdict(rsasa_context *ctx, const BatchStatus &stt, int attempts, uint64_t &cell_capacity)
{
    if (const int rc = grid_input_error(ctx, stt)) return rc;
    return stt.overflow ? grid_grow(ctx, stt.total_cells, attempts, cell_capacity) : RSASA_OK;
}

int enqueue_batch(rsasa_context *ctx, const Pending &pd, rsasa_context::HostSlot &hs)
{
    rsasa_context::Workspace &W = ctx->ws[pd.ws];
    const rsasa_device_batch_t &bt = pd.batch;
    const size_t N = bt.n_atoms, S = bt.n_structures, R = bt.n_residues;
    hipStream_t st = pd.stream;

    Lattice lat;
    int rc = get_lattice(ctx, pd.n_points, &lat);
    if (rc) return rc;

    const SegmentCount sc = count_segments(bt.structure_offsets_host, S);
    const size_t n_seg = sc.n_seg, n_large = sc.n_large;
    const bool has_tail = sc.has_tail;
    // (behind the segments, in the same upload: the large-id structures' numbers, four per segment-sized entry)
    const size_t n_seg_all = n_seg + (n_large + 3) / 4;
    if (n_seg_all * sizeof(Segment) > hs.h_segments.cap) {
        if (hs.h_segments.p) RS_HIP(ctx, hipStreamSynchronize(pd.stream));
        RS_HIP(ctx, hs.h_segments.regrow((n_seg_all + n_seg_all / 2 + 64) * sizeof(Segment)));
    }
    Segment *h_segments = static_cast<Segment *>(hs.h_segments.p);
    write_segments(bt.structure_offsets_host, S, h_segments, reinterpret_cast<uint32_t *>(h_segments + n_seg));

    const bool has_id = bt.id != nullptr;  // (with pd.id32 set, bt.id is the general kernel's device-accessible copy)
    if ((rc = W.reserve_grid(ctx, N, S, n_seg_all, ctx->cell_capacity, has_tail, has_id))) return rc;
    if ((rc = W.reserve_occlusion(ctx, lat, N, has_id, has_id, !bt.out_atom_sasa))) return rc;
    const bool keep_ids = W.keep_ids;
    if (keep_ids && pd.id32) return fail(ctx, RSASA_ERR_INTERNAL, "folded ids on a batch the per-atom kernels take");

    if (n_seg_all)
        RS_HIP(ctx, hipMemcpyAsync(W.segments.p, h_segments, n_seg_all * sizeof(Segment),
                                   hipMemcpyHostToDevice, st));

    BatchView v{};
    v.x = bt.x; v.y = bt.y; v.z = bt.z; v.radius = bt.radius; v.id = bt.id;
    v.id32 = pd.id32;
    // ids that are all different within their structure change nothing: checked on the device (BatchView::ids_check)
    // unless the host has looked already (pd.ids_needed_known: the host paths check before they upload)
    // (host-folded ids are checked as well: folds that differ are ids that differ, and a structure with two equal folds
    // simply keeps its ids)
    v.ids_check = (has_id && !pd.ids_needed_known && !keep_ids && !tuning_env("RSASA_NO_ID_CHECK")) ? 1u : 0u;
    hs.ids_check = v.ids_check != 0u;
    v.large_sids = reinterpret_cast<const uint32_t *>((const Segment *)W.segments.p + n_seg);
    v.n_large = (uint32_t)n_large;
    v.ids_tables = ctx->ids_unordered_hint ? 1u : 0u;
    v.radius8 = pd.radius8;
    v.radius_table = pd.radius_table;
    v.residue_offsets = bt.residue_offsets;
    v.n_atoms = (uint32_t)N; v.n_structures = (uint32_t)S; v.n_residues = (uint32_t)R;
    v.n_segments = (uint32_t)n_seg;
    v.probe = pd.probe;
    v.atom_sasa = bt.out_atom_sasa;
    W.grid_view(v);
    W.occlusion_view(v);
    v.residue_sasa = (R && bt.residue_offsets) ? bt.out_residue_sasa : nullptr;
    v.neighbor_counts = bt.out_neighbor_counts;

    // Launch stream: grids -> LDS binning -> occlusion of the LDS-binned structures -> (join) ->
    // occlusion of the tail -> sums.  Side stream (forked after the LDS binning): the tail's
    // batch-wide binning, which is bandwidth bound and runs next to the compute-bound occlusion kernel.
    if (ctx->timing) RS_HIP(ctx, hipEventRecord(W.ev[0], st));
    launch_grid_prepare(v, st);
    // Two batches in flight: this one's grid build is enqueued beside the other one's occlusion kernel (it gets the CUs
    // when that kernel's workgroups retire: the kernel leaves a CU no room), its occlusion kernel behind it.
    rsasa_context::Workspace &other = ctx->ws[pd.ws ^ 1];
    const bool chain = other.occ_recorded && !tuning_env("RSASA_FREE_OVERLAP");
    const bool overlap = ctx->overlap_tail && has_tail;
    if (overlap && (rc = ensure_side_stream(ctx))) return rc;
    if (overlap) {
        launch_sort_lds(v, st);
        // fork here, not before the LDS binning: two bandwidth-bound phases gain nothing from
        // running side by side, the occlusion kernel (compute bound) hides the tail's binning
        RS_HIP(ctx, hipEventRecord(ctx->ev_fork, st));
        RS_HIP(ctx, hipStreamWaitEvent(ctx->side_stream, ctx->ev_fork, 0));
        launch_sort_tail(v, ctx->side_stream);
        RS_HIP(ctx, hipEventRecord(ctx->ev_join, ctx->side_stream));
        if (ctx->timing) RS_HIP(ctx, hipEventRecord(W.ev[1], st));
        if (chain) RS_HIP(ctx, hipStreamWaitEvent(st, other.ev_occ, 0));
        if (ctx->timing) RS_HIP(ctx, hipEventRecord(W.ev[2], st));
        launch_occlusion(v, lat, ctx->tuning, kOccHead, st);
        RS_HIP(ctx, hipStreamWaitEvent(st, ctx->ev_join, 0));
        launch_occlusion(v, lat, ctx->tuning, kOccRest, st);
    } else {
        launch_sort_lds(v, st);
        if (has_tail) launch_sort_tail(v, st);
        if (ctx->timing) RS_HIP(ctx, hipEventRecord(W.ev[1], st));
        // (the wait for the other batch's occlusion kernel, the timing event and this batch's "occlusion kernel has ended"
        // event sit around the launch that does the work: OcclusionChain)
        OcclusionChain oc;
        oc.wait = chain ? other.ev_occ : nullptr;
        oc.start = ctx->timing ? W.ev[2] : nullptr;
        oc.done = W.ev_occ;
        oc.expect_ids_dropped = ctx->ids_drop_hint;
        oc.solo = pd.solo_ok && v.ids_check != 0u;
        launch_occlusion(v, lat, ctx->tuning, kOccAll, st, &oc);
    }
    if (overlap) RS_HIP(ctx, hipEventRecord(W.ev_occ, st));
    W.occ_recorded = true;
    if (ctx->timing) RS_HIP(ctx, hipEventRecord(W.ev[3], st));
    launch_residue_sums(v, st);
    if (ctx->timing) RS_HIP(ctx, hipEventRecord(W.ev[4], st));
    RS_HIP(ctx, hipMemcpyAsync(hs.h_status.p, W.status.p, sizeof(BatchStatus),
                               hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipGetLastError());
    return RSASA_OK;
}

// Waits for the batch in `pd` (re-running it if the cell array had to grow) and reports its deferred errors.
int wait_one(rsasa_context *ctx, Pending &pd)
{
    if (!pd.active) return RSASA_OK;
    rsasa_context::Workspace &W = ctx->ws[pd.ws];
    for (;;) {
        hipError_t e = hipStreamSynchronize(pd.stream);
        if (e != hipSuccess) {
            pd.active = false;
            return fail(ctx, RSASA_ERR_HIP, "hipStreamSynchronize", e);
        }
        const BatchStatus stt = ctx->slot[pd.ws].status();
        int rc = grid_verdict(ctx, stt, pd.attempts, ctx->cell_capacity);
        // the batch's one occlusion launch was the id-less instantiation and the ids do matter (OcclusionChain::solo):
        // nothing was computed
        const bool solo_missed = rc == RSASA_OK && ctx->slot[pd.ws].ids_check && (stt.ids_unordered & 2u) != 0u;
        if (rc == kGridAgain) {
            pd.attempts++;  // the cell array was too small for this batch: it has grown, run again
        } else if (solo_missed && pd.solo_ok) {
            // the batch runs again with its ids, as a launch pair (the check runs with it).  Only the solo launch raises
            // the bit: once per batch, whatever the cell array's attempts
            ctx->ids_drop_hint = false;
            ctx->ids_unordered_hint = (stt.ids_unordered & 1u) != 0u;
            pd.solo_ok = false;  // (every structure in the instantiation that is its own)
        } else {
            if (solo_missed) {
                rc = fail(ctx, RSASA_ERR_INTERNAL, "a launch pair reports the id-less launch's verdict");
            } else if (rc == RSASA_OK) {
                ctx->tuning.deferred_hint = stt.deferred;  // (sizes the next batch's launch over its deferred list)
                if (ctx->slot[pd.ws].ids_check) {
                    ctx->ids_drop_hint = !stt.ids_needed;
                    ctx->ids_unordered_hint = (stt.ids_unordered & 1u) != 0u;
                    ctx->ids_kept_structures.store(stt.ids_needed, std::memory_order_relaxed);
                    if (!stt.ids_needed) ctx->ids_dropped.fetch_add(1, std::memory_order_relaxed);
                }
                if (ctx->timing) {
                    float g = 0, o = 0, a = 0, t = 0;
                    (void)hipEventElapsedTime(&g, W.ev[0], W.ev[1]);
                    (void)hipEventElapsedTime(&o, W.ev[2], W.ev[3]);
                    (void)hipEventElapsedTime(&a, W.ev[3], W.ev[4]);
                    (void)hipEventElapsedTime(&t, W.ev[0], W.ev[4]);
                    ctx->timings = rsasa_timings_t{g, o, a, t, stt.grid_cells, pd.batch.n_atoms, stt.deferred};
                    ctx->timings_valid = true;
                }
            }
            pd.active = false;
            return rc;
        }
        if ((rc = enqueue_batch(ctx, pd, ctx->slot[pd.ws]))) {
            pd.active = false;
            return rc;
        }
    }
}

// The oldest batch in flight (rsasa_batch_wait), or every one (entry points that need the whole context).
int wait_oldest(rsasa_context *ctx)
{
    if (ctx->n_pending == 0) return RSASA_OK;
    const int rc = wait_one(ctx, ctx->pending[ctx->head]);
    ctx->head ^= 1;
    ctx->n_pending--;
    return rc;
}

int wait_pending(rsasa_context *ctx)
{
    int first = RSASA_OK;
    while (ctx->n_pending) {
        const int rc = wait_one(ctx, ctx->pending[ctx->head]);
        if (rc && !first) first = rc;
        ctx->head ^= 1;
        ctx->n_pending--;
    }
    return first;
}

rsasa_context *g_default_ctx = nullptr;
std::mutex g_default_mu;

int resolve_ctx(rsasa_context *&ctx)
{
    if (ctx) return RSASA_OK;
    std::lock_guard<std::mutex> lk(g_default_mu);
    if (!g_default_ctx) {
        int rc = rsasa_context_create(0, &g_default_ctx);
        if (rc) return rc;
    }
    ctx = g_default_ctx;
    return RSASA_OK;
}

}  // namespace rsasa

extern "C" {

int rsasa_abi_version(void) { return RSASA_ABI_VERSION; }

const char *rsasa_status_string(int status)
{
    switch (status) {
    case RSASA_OK: return "ok";
    case RSASA_ERR_INVALID_ARGUMENT: return "invalid argument";
    case RSASA_ERR_NO_DEVICE: return "no usable HIP device (this library has no CPU fallback)";
    case RSASA_ERR_HIP: return "HIP runtime error";
    case RSASA_ERR_OUT_OF_MEMORY: return "out of device memory";
    case RSASA_ERR_GRID_TOO_LARGE: return "cell grid too large";
    case RSASA_ERR_INTERNAL: return "internal error";
    case RSASA_ERR_QUEUE_FULL: return "host batch queue full";
    case RSASA_ERR_BUFFER_TOO_SMALL: return "output buffer too small (the offsets give the size needed)";
    default: return "unknown status";
    }
}

int rsasa_device_count(int *out_count)
{
    if (!out_count) return RSASA_ERR_INVALID_ARGUMENT;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        n = 0;
    }
    *out_count = n;
    return RSASA_OK;
}


int rsasa_context_create(int device, rsasa_context_t **out_ctx)
{
    return context_create(device, 0, out_ctx);
}

}  // extern "C"

int rsasa::context_create(int device, int own_queues, rsasa_context_t **out_ctx)
{
    if (!out_ctx) return RSASA_ERR_INVALID_ARGUMENT;
    *out_ctx = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return RSASA_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) return RSASA_ERR_NO_DEVICE;
    rsasa_context *ctx = new (std::nothrow) rsasa_context();
    if (!ctx) return RSASA_ERR_OUT_OF_MEMORY;
    ctx->device = device;
    ctx->own_queues = own_queues;
    ctx->node = device_node_cpus(device);
    DeviceGuard guard(device);
    hipError_t e = guard.err;
    if (e == hipSuccess) e = new_stream(ctx, &ctx->stream.h, 2);
    for (int w = 0; w < rsasa_context::kInFlight; w++) {
        for (int i = 0; i < 5 && e == hipSuccess; i++) e = hipEventCreate(&ctx->ws[w].ev[i].h);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ws[w].ev_occ.h, hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_fork.h, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_join.h, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_link.h, hipEventDisableTiming);
    for (int i = 0; i < rsasa_context::kSlots && e == hipSuccess; i++) e = hipEventCreateWithFlags(&ctx->ev_copy[i].h, hipEventDisableTiming);
    for (int i = 0; i < rsasa_context::kSlots && e == hipSuccess; i++) e = hipEventCreateWithFlags(&ctx->ev_d2h[i].h, hipEventDisableTiming);
    for (int i = 0; i < rsasa_context::kSlots && e == hipSuccess; i++) {
        e = ctx->slot[i].h_status.regrow(sizeof(BatchStatus));
        if (e == hipSuccess) std::memset(ctx->slot[i].h_status.p, 0, sizeof(BatchStatus));
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_done[i].h, hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        rsasa_context_destroy(ctx);
        return RSASA_ERR_HIP;
    }
    if (const char *v = tuning_env("RSASA_OCCLUSION_KERNEL")) ctx->tuning.kernel_version = std::atoi(v);
    if (const char *v = tuning_env("RSASA_ATOMS_PER_WAVE")) ctx->tuning.atoms_per_wave = (uint32_t)std::atoi(v);
    if (const char *v = tuning_env("RSASA_OVERLAP_TAIL")) ctx->overlap_tail = std::atoi(v) != 0;
    if (const char *v = tuning_env("RSASA_SMALL_PATH")) ctx->small_path = std::atoi(v) != 0;
    *out_ctx = ctx;
    return RSASA_OK;
}

extern "C" {

int rsasa_context_destroy(rsasa_context_t *ctx)
{
    if (!ctx) return RSASA_OK;
    if (HostStream *hs = ctx->host_stream) {
        // queued host batches finish (their buffers are the caller's: it has been told to wait for them), then the workers go
        {
            std::unique_lock<std::mutex> lk(hs->mu);
            hs->cv_done.wait(lk, [&] { for (auto &j : hs->jobs) if (!j->done) return false; return true; });
            hs->quit = true;
        }
        hs->cv_work.notify_all();
        for (auto &t : hs->th)
            if (t.joinable()) t.join();
        for (rsasa_context *sc : hs->sub) rsasa_context_destroy(sc);
        delete hs;
        ctx->host_stream = nullptr;
    }
    DeviceGuard guard(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
    if (ctx->d2h_stream) (void)hipStreamSynchronize(ctx->d2h_stream);
    if (ctx->device >= 0 && ctx->device < 64) {
        std::lock_guard<std::mutex> lk(g_link[ctx->device].mu);
        if (g_link[ctx->device].owner == ctx) { g_link[ctx->device].last = nullptr; g_link[ctx->device].owner = nullptr; }
    }
    for (auto &kv : ctx->lattices)
        if (kv.second.d) (void)hipFree(kv.second.d);
    // (the coding pool is the device's, shared by its contexts: it stays.  Everything else is the members' own to free,
    // here, while the guard keeps the context's device current)
    delete ctx;
    return RSASA_OK;
}

const char *rsasa_context_last_error(const rsasa_context_t *ctx)
{
    if (!ctx) return "";
    // a copy per calling thread, taken under the lock: another thread's failure cannot change
    // (or free) the string while this one reads it; valid until this thread's next call
    static thread_local std::string copy;
    rsasa_context *c = const_cast<rsasa_context *>(ctx);
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    copy = c->last_error;
    return copy.c_str();
}

int rsasa_context_get_device(const rsasa_context_t *ctx, int *out_device)
{
    if (!ctx || !out_device) return RSASA_ERR_INVALID_ARGUMENT;
    *out_device = ctx->device;
    return RSASA_OK;
}

int rsasa_context_set_simd_width(rsasa_context_t *ctx, int w)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (w != 1 && w != 4 && w != 8 && w != 16)
        return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "simd_width must be 1, 4, 8 or 16");
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ctx->simd_width = w;
    return RSASA_OK;
}

int rsasa_context_get_simd_width(rsasa_context_t *ctx, int *out_simd_width)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (!out_simd_width) return RSASA_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    *out_simd_width = ctx->simd_width;
    return RSASA_OK;
}

int rsasa_context_bind_thread(rsasa_context_t *ctx, int *out_numa_node)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (out_numa_node) *out_numa_node = ctx->node.valid ? ctx->node.node : -1;
    (void)bind_thread_to(pthread_self(), ctx->node);
    return RSASA_OK;
}

int rsasa_context_enable_timing(rsasa_context_t *ctx, int enable)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // a batch enqueued under the other setting has (or lacks) its events: finish what is in flight first
    if (ctx->n_pending && (ctx->timing != (enable != 0))) {
        RS_DEVICE(ctx);
        if ((rc = wait_pending(ctx))) return rc;
    }
    ctx->timing = enable != 0;
    ctx->timings_valid = false;
    return RSASA_OK;
}

int rsasa_context_get_timings(rsasa_context_t *ctx, rsasa_timings_t *out)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (!out) return RSASA_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!ctx->timings_valid)
        return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "no timed batch has completed");
    *out = ctx->timings;
    return RSASA_OK;
}

int rsasa_context_ids_kept(rsasa_context_t *ctx, uint64_t *out_structures)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (!out_structures) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, "out_structures is NULL");
    *out_structures = ctx->ids_kept_structures.load(std::memory_order_relaxed);
    return RSASA_OK;
}

int rsasa_context_ids_dropped(rsasa_context_t *ctx, uint64_t *out_batches)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (!out_batches) return RSASA_ERR_INVALID_ARGUMENT;
    uint64_t n = ctx->ids_dropped.load(std::memory_order_relaxed);
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (ctx->host_stream)  // (the stream's batches run on its workers' contexts)
        for (int w = 0; w < ctx->host_stream->n_workers; w++)
            if (ctx->host_stream->sub[w]) n += ctx->host_stream->sub[w]->ids_dropped.load(std::memory_order_relaxed);
    *out_batches = n;
    return RSASA_OK;
}

int rsasa_batch_enqueue(rsasa_context_t *ctx, const rsasa_device_batch_t *batch,
                        float probe_radius, size_t n_points, void *hip_stream)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    if (const char *msg = check_device_batch(batch, probe_radius, n_points)) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, msg);
    return enqueue_checked(ctx, *batch, probe_radius, n_points, hip_stream);
}

}  // extern "C"

// rsasa_batch_enqueue behind its rule.  `batch` has passed check_device_batch with this probe and n_points, or was built
// from arguments that passed their entry point's rule (a host batch of one sub-batch, a trajectory's chunk of frames):
// nothing here looks again.
int rsasa::enqueue_checked(rsasa_context *ctx, const rsasa_device_batch_t &batch, float probe_radius, size_t n_points, void *hip_stream)
{
    int rc;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    // Up to two batches in flight, each in its own workspace; a third waits for the oldest one.
    while (ctx->n_pending >= rsasa_context::kInFlight)
        if ((rc = wait_oldest(ctx))) return rc;
    const int w = ctx->n_pending ? ctx->pending[ctx->head].ws ^ 1 : 0;
    if (w == 1 && !hip_stream && !ctx->stream2)
        RS_HIP(ctx, new_stream(ctx, &ctx->stream2.h, 2));
    Pending &pd = ctx->pending[ctx->head ^ (ctx->n_pending ? 1 : 0)];
    pd = Pending{};
    pd.batch = batch;
    pd.probe = probe_radius;
    pd.n_points = n_points;
    pd.stream = hip_stream ? (hipStream_t)hip_stream : (w ? ctx->stream2 : ctx->stream);
    pd.ws = w;
    pd.solo_ok = true;  // (rsasa_batch_wait runs a batch again when the id-less launch was the wrong guess: wait_one)
    rc = enqueue_batch(ctx, pd, ctx->slot[w]);
    pd.active = (rc == RSASA_OK);
    if (pd.active) ctx->n_pending++;
    return rc;
}

extern "C" {

int rsasa_batch_wait(rsasa_context_t *ctx)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    return wait_oldest(ctx);
}

int rsasa_batch_wait_all(rsasa_context_t *ctx)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    return wait_pending(ctx);
}

int rsasa_context_clone_settings(rsasa_context_t *dst, rsasa_context_t *src)
{
    int rc = resolve_ctx(src);
    if (rc) return rc;
    if (!dst || dst == src) return dst ? RSASA_OK : RSASA_ERR_INVALID_ARGUMENT;
    int simd = 8;
    bool small = true, overlap = false;
    OcclusionTuning tune;
    {
        std::lock_guard<std::recursive_mutex> lk(src->mu);
        simd = src->simd_width; small = src->small_path; overlap = src->overlap_tail; tune = src->tuning;
    }
    std::lock_guard<std::recursive_mutex> lk(dst->mu);
    tune.deferred_hint = dst->tuning.deferred_hint;  // (a measurement of dst's own batches, not a setting)
    dst->simd_width = simd; dst->small_path = small; dst->overlap_tail = overlap; dst->tuning = tune;
    return RSASA_OK;
}

int rsasa_segment_sums(rsasa_context_t *ctx, const float *values, size_t n_values,
                       const uint32_t *offsets, size_t n_segments, float *out)
{
    int rc = resolve_ctx(ctx);
    if (rc) return rc;
    bool empty;
    if (const char *msg = check_segments(values, n_values, offsets, n_segments, out, empty)) return fail(ctx, RSASA_ERR_INVALID_ARGUMENT, msg);
    if (empty) return RSASA_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    RS_DEVICE(ctx);
    if (ctx->n_pending && (rc = wait_pending(ctx))) return rc;
    if ((rc = reserve(ctx, ctx->ws[0].atom_sasa, std::max<size_t>(n_values, 1) * 4))) return rc;
    if ((rc = reserve(ctx, ctx->in_res, (n_segments + 1) * 4))) return rc;
    if ((rc = reserve(ctx, ctx->out_res, n_segments * 4))) return rc;
    if ((rc = reserve(ctx, ctx->ws[0].status, sizeof(BatchStatus)))) return rc;
    hipStream_t st = ctx->stream;
    RS_HIP(ctx, hipMemsetAsync(ctx->ws[0].status.p, 0, sizeof(BatchStatus), st));
    if (n_values)
        RS_HIP(ctx, hipMemcpyAsync(ctx->ws[0].atom_sasa.p, values, n_values * 4, hipMemcpyHostToDevice, st));
    RS_HIP(ctx, hipMemcpyAsync(ctx->in_res.p, offsets, (n_segments + 1) * 4, hipMemcpyHostToDevice, st));
    BatchView v{};
    v.residue_offsets = (const uint32_t *)ctx->in_res.p;
    v.n_residues = (uint32_t)n_segments;
    v.status = (BatchStatus *)ctx->ws[0].status.p;
    v.atom_sasa = (float *)ctx->ws[0].atom_sasa.p;
    v.residue_sasa = (float *)ctx->out_res.p;
    launch_residue_sums(v, st);
    RS_HIP(ctx, hipMemcpyAsync(out, ctx->out_res.p, n_segments * 4, hipMemcpyDeviceToHost, st));
    RS_HIP(ctx, hipStreamSynchronize(st));
    return RSASA_OK;
}

int rsasa_sphere_points(size_t n_points, float *out_x, float *out_y, float *out_z)
{
    if (!n_points || !out_x || !out_y || !out_z) return RSASA_ERR_INVALID_ARGUMENT;
    generate_sphere_points(n_points, out_x, out_y, out_z);
    return RSASA_OK;
}

}  // extern "C"
