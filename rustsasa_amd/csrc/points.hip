// Accessible-point kernel (rsasa_accessible_points*, gfx950 only): which sphere points of each atom the reference finds
// exposed (AtomSasaKernel::with_simd, reference src/lib.rs:96-223), as bit masks, from the neighbour lists that
// neighbors.hip built in HBM (k_neighbor_count / k_nb_scan_* / k_neighbor_fill with max_r = NaN: the SASA path's lists).
//
//   k_accessible_points   one wave per cell-sorted atom; lanes over 64-point chunks of the lattice (reference order,
//                         zero padded), NCH chunks per pass; the atom's list is staged in LDS as (vx, vy, vz, limit),
//                         kPtStage entries at a time, and every lane tests its points against each staged entry.  A
//                         pass stops once its ballot of still-exposed lanes is empty.  Each chunk's exposed ballot is
//                         two 32-bit words of the mask.
//   k_contact_points      (rsasa_contact_points*) the same layout, no early exit: per entry of the list, the points it
//                         hits (covered) and those it alone hits (exclusive), from two sweeps of the list per pass.
//   k_contact_owners      (rsasa_contact_owners*) the same layout, one sweep per pass: every buried point goes to the
//                         entry with the smallest margin dot - limit (owned per entry, the owner position per point).
//   k_group_order         (rsasa_group_contacts*) one wave per atom: its list again with the entries of its own group
//                         (label) first and the others by (label, position), each entry ranked by counting the keys
//                         below its own; the number of distinct foreign labels is the atom's row count.
//   k_group_points        the layout of k_contact_points over the reordered list, one sweep per pass: the own-group
//                         entries give `self`, every run of one foreign label an OR whose ballots are the row's buried
//                         count; a point remembers the first row that hit it, which gives the rows' `only` counts.
//   k_exposure_vectors    (rsasa_exposure_vectors*) the layout, staging, tests and early exit of k_accessible_points; no
//                         masks: per atom the float32 sum of its exposed lattice points, in a fixed order (a tree over
//                         the lanes of a chunk, then the chunks ascending), and their number.
//   k_mask_free           one thread per atom: the popcount of its mask (free[], input order), for the kernels that start
//                         from the masks of a finished run (depth.hip, components.hip).
//
// The five point kernels share one frame, written once below: the atom and its list (pt_atom), the list staged in LDS
// (pt_stage: once by pt_stage_first when it fits one stage, else by pt_restage in every sweep, which holds the fences),
// the lattice points of a pass (pt_load_points, pt_pass_begin), the two hit rules (pt_hit) and the value (pt_sasa).
//
// Points [0, n_fused) take the fused rule - mul_add(sx, vx, mul_add(sy, vy, sz * vz)) < limit (lib.rs:143-146) -, the
// rest the remainder rule - plain products, `<=` (lib.rs:185-186,206-207).  Both rules are ORs over the list, so the
// list's order (and the reference's early exits and cached neighbour) do not change a bit.
// Compiled with -ffp-contract=off: d^2 and the remainder dot product are not fused, as in the reference.
#include "device_utils.h"

namespace rsasa {
namespace {

constexpr uint32_t kPtStage = 256;  // list entries a wave holds in LDS (4 KiB; lists are ~44 long at probe 1.4)

// One wave's atom: cell-sorted atom p as input row `row` of the batch, its structure's first row, and its list in `entries`.
struct PtAtom {
    uint32_t row, base;
    float4 me;                // (x, y, z, radius)
    float R2, twoR;
    unsigned long long off;   // the list is entries[off .. off + K)
    uint32_t K;
    const uint2 *ent;
    bool one_stage;           // the whole list fits s_ent: staged once, before the passes
};

__device__ __forceinline__ PtAtom pt_atom(const PtArgs &a, const uint2 *entries, uint32_t p)
{
    const BatchView &b = a.b;
    PtAtom t;
    t.row = b.sorted_orig[p];
    t.base = b.grids[b.sid_sorted[p]].atom_begin;
    t.me = make_float4(b.x[t.row], b.y[t.row], b.z[t.row], b.radius[t.row]);
    const float R = t.me.w + b.probe;  // lib.rs:101
    t.R2 = R * R;                      // lib.rs:102
    t.twoR = 2.0f * R;                 // lib.rs:136
    t.off = a.offsets[t.row];
    t.K = (uint32_t)(a.offsets[t.row + 1] - t.off);
    t.ent = entries + t.off;
    t.one_stage = t.K <= kPtStage;
    return t;
}

__device__ __forceinline__ uint32_t pt_pad4(uint32_t n) { return (n + 3u) & ~3u; }

// Entries [s0, s0 + n) of the atom's list -> s_ent as (vx, vy, vz, limit) (lib.rs:129-136), lanes in parallel, then
// up to 3 entries (0, 0, 0, -inf) up to a multiple of 4: no point of the lattice is occluded by one (dot = 0, 0 < -inf
// and 0 <= -inf are false), so the test loop reads whole groups of four.
__device__ __forceinline__ void pt_stage(const PtArgs &a, const PtAtom &t, uint32_t s0, uint32_t n, float4 *s_ent)
{
    const BatchView &b = a.b;
    const uint32_t n4 = pt_pad4(n);
    for (uint32_t e = lane_id(); e < n4; e += kWave) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, -__builtin_inff());
        if (e < n) {
            const uint2 en = t.ent[s0 + e];
            const uint32_t j = t.base + en.y;                             // idx is the index within the structure
            const float vx = t.me.x - b.x[j], vy = t.me.y - b.y[j], vz = t.me.z - b.z[j];  // lib.rs:129-131
            const float d2 = vx * vx + vy * vy + vz * vz;                 // lib.rs:132
            const float th = __uint_as_float(en.x);                       // threshold_squared, spatial_grid.rs:336-339
            v = make_float4(vx, vy, vz, (th - d2 - t.R2) / t.twoR);       // lib.rs:136
        }
        s_ent[e] = v;
    }
}

// A list of one stage is staged here, before the passes; `stage(s0, n)` writes entries [s0, s0 + n) to the wave's LDS.
template <typename Stage>
__device__ __forceinline__ void pt_stage_first(const PtAtom &t, Stage stage)
{
    if (t.one_stage && t.K) {
        stage(0u, t.K);
        wave_lds_fence();
    }
}

// A sweep of the list is `for (s0 = 0; s0 < t.K; s0 += kPtStage)` over pt_restage: after it entries [s0, s0 + n), n
// returned, are in the wave's LDS.  A list of more than one stage is staged again in every sweep, between two fences;
// one that pt_stage_first staged is left alone.  (A loop in the kernel, not a function that takes the sweep's body: with
// the body in a lambda k_group_points keeps its flags in scalar registers and spills them.)
template <typename Stage>
__device__ __forceinline__ uint32_t pt_restage(const PtAtom &t, uint32_t s0, Stage stage)
{
    const uint32_t n = min(kPtStage, t.K - s0);
    if (!t.one_stage) {
        wave_lds_fence();  // (every lane is done with the previous stage)
        stage(s0, n);
        wave_lds_fence();
    }
    return n;
}

// The lattice points of one pass, NCH chunks of 64, one point of each chunk per lane.
template <int NCH>
struct PtPass {
    float sx[NCH], sy[NCH], sz[NCH];
    bool live[NCH];  // a point of the lattice: not a lane past the last point (or a chunk past the last)
    bool rem[NCH];   // the point takes the remainder rule
};

// The points of chunks [cb, cb + NCH) -> nx, ny, nz; zeros for the chunks past the last (the lattice arrays are zero
// padded to whole chunks).
template <int NCH>
__device__ __forceinline__ void pt_load_points(const PtArgs &a, uint32_t cb, uint32_t n_chunks, float (&nx)[NCH],
                                               float (&ny)[NCH], float (&nz)[NCH])
{
    const uint32_t lane = lane_id();
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const uint32_t nc = cb + c;
        const bool in = nc < n_chunks;
        nx[c] = in ? a.lx[nc * kWave + lane] : 0.0f;
        ny[c] = in ? a.ly[nc * kWave + lane] : 0.0f;
        nz[c] = in ? a.lz[nc * kWave + lane] : 0.0f;
    }
}

// The pass over chunks [c0, c0 + NCH) takes the points in nx, ny, nz (pt_load_points, before the first pass); those of
// the next pass are loaded there while it runs.  Returns any_rem: some live point of the pass takes the remainder rule
// (the same in every lane).
template <int NCH>
__device__ __forceinline__ bool pt_pass_begin(const PtArgs &a, uint32_t c0, uint32_t n_chunks, float (&nx)[NCH],
                                              float (&ny)[NCH], float (&nz)[NCH], PtPass<NCH> &ps)
{
    const uint32_t lane = lane_id();
    bool any_rem = false;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        ps.sx[c] = nx[c]; ps.sy[c] = ny[c]; ps.sz[c] = nz[c];
        const uint32_t pi = (c0 + c) * kWave + lane;
        ps.live[c] = pi < a.n_points;
        ps.rem[c] = pi >= a.n_fused;
        any_rem = any_rem || (ps.rem[c] && ps.live[c]);
    }
    pt_load_points(a, c0 + NCH, n_chunks, nx, ny, nz);
    return ballot64(any_rem) != 0ull;
}

// Whether staged entry e = (vx, vy, vz, limit) hits the point (sx, sy, sz); REM: the points with `rem` take the
// remainder rule.
template <bool REM>
__device__ __forceinline__ bool pt_hit(float sx, float sy, float sz, bool rem, const float4 e)
{
    // lib.rs:143-146: mul_add(sx, vx, mul_add(sy, vy, sz * vz)) < limit
    bool hit = __builtin_fmaf(sx, e.x, __builtin_fmaf(sy, e.y, sz * e.z)) < e.w;
    if (REM) {
        // lib.rs:185-186,206-207: plain products, `<=`
        const float dotu = sx * e.x + sy * e.y + sz * e.z;
        hit = rem ? dotu <= e.w : hit;
    }
    return hit;
}

// lib.rs:220-222
__device__ __forceinline__ float pt_sasa(float R2, uint32_t exposed, uint32_t n_points)
{
    return ((4.0f * 3.14159274101257324219f) * R2) * (float)exposed * (1.0f / (float)n_points);
}

// Staged entries [0, n) (n a multiple of 4) against the NCH chunks of a pass; REM: some lane of the pass takes the
// remainder rule.  Returns true once every point of the pass is occluded (lib.rs:149-152).
template <int NCH, bool REM>
__device__ __forceinline__ bool pt_test(const float4 *s_ent, uint32_t n, const PtPass<NCH> &ps, bool (&occ)[NCH])
{
    for (uint32_t k = 0; k < n; k += 4) {
        float4 e[4];
#pragma unroll
        for (int u = 0; u < 4; u++) e[u] = s_ent[k + u];  // (the four LDS reads in flight together)
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const bool hit = pt_hit<REM>(ps.sx[c], ps.sy[c], ps.sz[c], ps.rem[c], e[u]);
                occ[c] = occ[c] || hit;
            }
        }
        bool all = true;
#pragma unroll
        for (int c = 0; c < NCH; c++) all = all && occ[c];
        if (ballot64(!all) == 0ull) return true;
    }
    return false;
}

// One pass of the early-exit kernels: occ[c] of every point of the pass after the whole list, or after the part of it
// that occluded them all.  The lanes past the last point (and the chunks past the last) start occluded: never exposed.
template <int NCH, typename Stage>
__device__ __forceinline__ void pt_pass_occluded(const PtAtom &t, Stage stage, const float4 *s_ent, const PtPass<NCH> &ps,
                                                 bool any_rem, bool (&occ)[NCH])
{
#pragma unroll
    for (int c = 0; c < NCH; c++) occ[c] = !ps.live[c];
    for (uint32_t s0 = 0; s0 < t.K; s0 += kPtStage) {
        const uint32_t n4 = pt_pad4(pt_restage(t, s0, stage));
        if (any_rem ? pt_test<NCH, true>(s_ent, n4, ps, occ) : pt_test<NCH, false>(s_ent, n4, ps, occ)) break;
    }
}

// NCH chunks of 64 points per pass: every staged entry is read once for all of them.
template <int NCH>
__global__ __launch_bounds__(256) void k_accessible_points(PtArgs a)
{
    __shared__ float4 s_ent[4][kPtStage];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= a.b.n_atoms) return;
    const PtAtom t = pt_atom(a, a.entries, p);
    const auto stage = [&](uint32_t s0, uint32_t n) __attribute__((always_inline)) { pt_stage(a, t, s0, n, s_ent[w]); };
    pt_stage_first(t, stage);

    const uint32_t n_chunks = (a.n_points + kWave - 1) / kWave;
    float nx[NCH], ny[NCH], nz[NCH];
    pt_load_points(a, 0u, n_chunks, nx, ny, nz);
    uint32_t exposed = 0;
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += NCH) {
        PtPass<NCH> ps;
        bool occ[NCH];
        const bool any_rem = pt_pass_begin(a, c0, n_chunks, nx, ny, nz, ps);
        pt_pass_occluded(t, stage, s_ent[w], ps, any_rem, occ);
        // the pass's exposed ballots: lanes 0 .. 2 NCH - 1 write its 2 NCH words at once
        uint32_t word = 0;
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const unsigned long long m = ballot64(!occ[c]);
            exposed += (uint32_t)__popcll(m);
            if (lane == 2u * c) word = (uint32_t)m;
            if (lane == 2u * c + 1u) word = (uint32_t)(m >> 32);
        }
        const uint32_t wi = 2u * c0 + lane;
        if (lane < 2u * NCH && wi < a.words) a.masks[(size_t)t.row * a.words + wi] = word;
    }
    if (lane == 0 && a.sasa) a.sasa[t.row] = pt_sasa(t.R2, exposed, a.n_points);
}

__global__ __launch_bounds__(256) void k_mask_free(PtArgs a, uint32_t *free)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.b.n_atoms) return;
    const uint32_t *m = a.masks + (size_t)i * a.words;
    uint32_t n = 0;
    for (uint32_t w = 0; w < a.words; w++) n += (uint32_t)__popc(m[w]);
    free[i] = n;
}

// ---- contact counts (rsasa_contact_points*) ----

// Staged entries [0, n) (n a multiple of 4) against the NCH chunks of a pass: entry k's hits on the points `gate`
// admits are counted into s_cnt[k].  FIRST (the first sweep): every hit also marks its point hit once, or twice once
// it was hit before.
template <int NCH, bool REM, bool FIRST>
__device__ __forceinline__ void ct_test(const float4 *s_ent, uint32_t n, const PtPass<NCH> &ps, const bool (&gate)[NCH],
                                        bool (&once)[NCH], bool (&twice)[NCH], uint32_t *s_cnt)
{
    const uint32_t lane = lane_id();
    for (uint32_t k = 0; k < n; k += 4) {
        float4 e[4];
#pragma unroll
        for (int u = 0; u < 4; u++) e[u] = s_ent[k + u];
        uint32_t cnt[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            cnt[u] = 0;
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                bool hit = pt_hit<REM>(ps.sx[c], ps.sy[c], ps.sz[c], ps.rem[c], e[u]);
                hit = hit && gate[c];
                if (FIRST) {
                    twice[c] = twice[c] || (once[c] && hit);
                    once[c] = once[c] || hit;
                }
                cnt[u] += (uint32_t)__popcll(ballot64(hit));
            }
        }
        // lanes 0 .. 3 write the group's four counts at once
        const uint32_t mine = lane == 0 ? cnt[0] : lane == 1 ? cnt[1] : lane == 2 ? cnt[2] : cnt[3];
        if (lane < 4u) s_cnt[k + lane] = mine;
    }
}

// One sweep of the whole list for the chunks of a pass: entry e's count goes to dst[e], added to what the earlier
// passes left there when `add`.
template <int NCH, bool FIRST, typename Stage>
__device__ __forceinline__ void ct_sweep(const PtAtom &t, Stage stage, const float4 *s_ent, uint32_t *s_cnt, uint32_t *dst,
                                         bool add, const PtPass<NCH> &ps, bool any_rem, const bool (&gate)[NCH],
                                         bool (&once)[NCH], bool (&twice)[NCH])
{
    for (uint32_t s0 = 0; s0 < t.K; s0 += kPtStage) {
        const uint32_t n = pt_restage(t, s0, stage);
        if (any_rem) ct_test<NCH, true, FIRST>(s_ent, pt_pad4(n), ps, gate, once, twice, s_cnt);
        else ct_test<NCH, false, FIRST>(s_ent, pt_pad4(n), ps, gate, once, twice, s_cnt);
        wave_lds_fence();
        // coalesced; lane l owns entries l, l + 64, ... in every pass, so what it adds to is its own earlier write
        for (uint32_t e = lane_id(); e < n; e += kWave) dst[s0 + e] = s_cnt[e] + (add ? dst[s0 + e] : 0u);
        wave_lds_fence();  // (every lane has read the counts before the next sweep writes them)
    }
}

// The frame of k_accessible_points (one wave per cell-sorted atom, lanes over NCH chunks of 64 points per pass, the
// list staged in LDS by pt_stage), without its early exit.  Per pass, sweep 1 counts each entry's hits (covered) and
// leaves every lane knowing which of its points one entry hits and which more than one; sweep 2 goes over the list
// again and counts each entry's hits on the points hit once (exclusive).
template <int NCH>
__global__ __launch_bounds__(256) void k_contact_points(CtArgs ct)
{
    const PtArgs &a = ct.p;
    __shared__ float4 s_ent[4][kPtStage];
    __shared__ uint32_t s_cnt[4][kPtStage];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= a.b.n_atoms) return;
    const PtAtom t = pt_atom(a, a.entries, p);
    const auto stage = [&](uint32_t s0, uint32_t n) __attribute__((always_inline)) { pt_stage(a, t, s0, n, s_ent[w]); };
    pt_stage_first(t, stage);

    // an empty list: no counts, every point exposed
    const uint32_t n_chunks = t.K ? (a.n_points + kWave - 1) / kWave : 0u;
    float nx[NCH], ny[NCH], nz[NCH];
    pt_load_points(a, 0u, n_chunks, nx, ny, nz);
    uint32_t exposed = t.K ? 0u : a.n_points;
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += NCH) {
        PtPass<NCH> ps;
        bool once[NCH], twice[NCH], solo[NCH];
        const bool any_rem = pt_pass_begin(a, c0, n_chunks, nx, ny, nz, ps);
#pragma unroll
        for (int c = 0; c < NCH; c++) once[c] = twice[c] = false;
        ct_sweep<NCH, true>(t, stage, s_ent[w], s_cnt[w], ct.covered + t.off, c0 != 0, ps, any_rem, ps.live, once, twice);
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            solo[c] = once[c] && !twice[c];
            exposed += (uint32_t)__popcll(ballot64(ps.live[c] && !once[c]));
        }
        ct_sweep<NCH, false>(t, stage, s_ent[w], s_cnt[w], ct.exclusive + t.off, c0 != 0, ps, any_rem, solo, once, twice);
    }
    if (lane == 0 && a.sasa) a.sasa[t.row] = pt_sasa(t.R2, exposed, a.n_points);
}

// ---- contact owners (rsasa_contact_owners*) ----

constexpr uint32_t kCoFree = 0xFFFFFFFFu;  // the owner of a point no entry hits

// Staged entries [0, n) (n a multiple of 4) - positions s0, s0 + 1, ... of the list - against the NCH chunks of a pass.
// The margin of entry e at a point is the dot product its hit rule compares, minus the limit (one float32 subtraction,
// not fused: -ffp-contract=off); a hitting entry takes the point when nobody owns it yet or its margin is below the
// owner's, so of equal margins the earlier position keeps it.  The pad entries (limit -inf) and a NaN limit never hit;
// `live` keeps the lanes past the last point (dot 0, which hits under a positive limit) from owning.
template <int NCH, bool REM>
__device__ __forceinline__ void co_test(const float4 *s_ent, uint32_t n, uint32_t s0, const PtPass<NCH> &ps,
                                        float (&best_m)[NCH], uint32_t (&best_e)[NCH])
{
    for (uint32_t k = 0; k < n; k += 4) {
        float4 e[4];
#pragma unroll
        for (int u = 0; u < 4; u++) e[u] = s_ent[k + u];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t pos = s0 + k + u;  // (the same in every lane)
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                // pt_hit's two dots
                float dot = __builtin_fmaf(ps.sx[c], e[u].x, __builtin_fmaf(ps.sy[c], e[u].y, ps.sz[c] * e[u].z));
                bool hit = dot < e[u].w;
                if (REM) {
                    const float dotu = ps.sx[c] * e[u].x + ps.sy[c] * e[u].y + ps.sz[c] * e[u].z;
                    hit = ps.rem[c] ? dotu <= e[u].w : hit;
                    dot = ps.rem[c] ? dotu : dot;
                }
                const float m = dot - e[u].w;
                const bool take = hit && ps.live[c] && (best_e[c] == kCoFree || m < best_m[c]);
                best_m[c] = take ? m : best_m[c];
                best_e[c] = take ? pos : best_e[c];
            }
        }
    }
}

// The frame of k_contact_points, one sweep of the list per pass: every lane carries the smallest margin and its
// position (best_m, best_e) of each of its points across the whole list, stages included.  After the sweep each lane
// adds 1 to its owners' cells of s_cnt (LDS atomics), one window of kPtStage positions at a time, and the window is
// added to owned[] as ct_sweep adds its counts across passes.  owner[] (nullable) gets every point's owner position.
template <int NCH>
__global__ __launch_bounds__(256) void k_contact_owners(CoArgs co)
{
    const PtArgs &a = co.p;
    __shared__ float4 s_ent[4][kPtStage];
    __shared__ uint32_t s_cnt[4][kPtStage];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= a.b.n_atoms) return;
    const PtAtom t = pt_atom(a, a.entries, p);
    const auto stage = [&](uint32_t s0, uint32_t n) __attribute__((always_inline)) { pt_stage(a, t, s0, n, s_ent[w]); };
    pt_stage_first(t, stage);
    uint32_t *owned = co.owned + t.off;
    uint32_t *owner = co.owner ? co.owner + (size_t)t.row * a.n_points : nullptr;

    // an empty list: no counts, no sweep, every point free
    const uint32_t n_chunks = t.K ? (a.n_points + kWave - 1) / kWave : 0u;
    if (!t.K && owner)
        for (uint32_t pi = lane; pi < a.n_points; pi += kWave) owner[pi] = kCoFree;
    float nx[NCH], ny[NCH], nz[NCH];
    pt_load_points(a, 0u, n_chunks, nx, ny, nz);
    uint32_t exposed = t.K ? 0u : a.n_points;
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += NCH) {
        PtPass<NCH> ps;
        float best_m[NCH];
        uint32_t best_e[NCH];
        const bool any_rem = pt_pass_begin(a, c0, n_chunks, nx, ny, nz, ps);
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            best_m[c] = __builtin_inff();
            best_e[c] = kCoFree;
        }
        for (uint32_t s0 = 0; s0 < t.K; s0 += kPtStage) {
            const uint32_t n4 = pt_pad4(pt_restage(t, s0, stage));
            if (any_rem) co_test<NCH, true>(s_ent[w], n4, s0, ps, best_m, best_e);
            else co_test<NCH, false>(s_ent[w], n4, s0, ps, best_m, best_e);
        }
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            exposed += (uint32_t)__popcll(ballot64(ps.live[c] && best_e[c] == kCoFree));
            const uint32_t pi = (c0 + c) * kWave + lane;
            if (owner && pi < a.n_points) owner[pi] = best_e[c];  // coalesced
        }
        for (uint32_t s0 = 0; s0 < t.K; s0 += kPtStage) {
            const uint32_t n = min(kPtStage, t.K - s0);
            for (uint32_t e = lane; e < n; e += kWave) s_cnt[w][e] = 0u;
            wave_lds_fence();
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const uint32_t rel = best_e[c] - s0;  // (a free point: kCoFree - s0 >= 2^32 - 2^31 > n)
                if (rel < n) atomicAdd(&s_cnt[w][rel], 1u);
            }
            wave_lds_fence();
            // lane l owns entries l, l + 64, ... in every pass, so what it adds to is its own earlier write
            for (uint32_t e = lane; e < n; e += kWave) owned[s0 + e] = s_cnt[w][e] + (c0 != 0 ? owned[s0 + e] : 0u);
            wave_lds_fence();  // (every lane has read the counts before the next window clears them)
        }
    }
    if (lane == 0 && a.sasa) a.sasa[t.row] = pt_sasa(t.R2, exposed, a.n_points);
}

// ---- group contacts (rsasa_group_contacts*) ----

// The sort key of entry e (its position in the list, below 2^31) with label `lab` in the list of an atom labelled `mine`:
// own-group entries first, then ascending unsigned label, then position.  No two entries of a list share a key.
__device__ __forceinline__ unsigned long long gp_key(uint32_t lab, uint32_t mine, uint32_t e)
{
    const unsigned long long cls = lab == mine ? 0ull : (1ull << 32) | lab;
    return (cls << 31) | e;
}

// One wave per cell-sorted atom.  Lane l takes entries l, l + 64, ... of the list; an entry's place in the new order is
// the number of keys below its own, counted against the keys of the whole list, which pass through LDS kPtStage at a
// time (any list length; K^2 / 64 steps per lane).  A foreign entry with no key of its label below it starts a row.
__global__ __launch_bounds__(256) void k_group_order(GpArgs g)
{
    const PtArgs &a = g.p;
    __shared__ unsigned long long s_key[4][kPtStage];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= a.b.n_atoms) return;
    const PtAtom t = pt_atom(a, a.entries, p);  // (its list; the centre and the radius stay unread)
    const uint32_t mine = g.group[t.row];
    uint32_t n_own = 0, n_rows = 0;
    for (uint32_t eb = 0; eb < t.K; eb += kWave) {
        const uint32_t e = eb + lane;
        const bool valid = e < t.K;
        const uint2 en = valid ? t.ent[e] : make_uint2(0u, 0u);
        const uint32_t lab = valid ? g.group[t.base + en.y] : mine;  // idx is the index within the structure
        const unsigned long long first = gp_key(lab, mine, 0u), key = first | e;
        uint32_t rank = 0, before_label = 0;
        for (uint32_t t0 = 0; t0 < t.K; t0 += kPtStage) {
            const uint32_t n = min(kPtStage, t.K - t0);
            if (t.K > kPtStage || eb == 0) {  // (not one stage; written out: !t.one_stage costs the loop an instruction)
                wave_lds_fence();  // (every lane is done with the previous keys)
                for (uint32_t k = lane; k < n; k += kWave) s_key[w][k] = gp_key(g.group[t.base + t.ent[t0 + k].y], mine, t0 + k);
                wave_lds_fence();
            }
            for (uint32_t k = 0; k < n; k++) {
                const unsigned long long o = s_key[w][k];  // (the same address in every lane: a broadcast)
                rank += o < key ? 1u : 0u;
                before_label += o < first ? 1u : 0u;
            }
        }
        const bool own = valid && lab == mine;
        n_own += (uint32_t)__popcll(ballot64(own));
        n_rows += (uint32_t)__popcll(ballot64(valid && !own && rank == before_label));
        if (valid) {
            g.sorted[t.off + rank] = en;
            g.sorted_group[t.off + rank] = lab;
        }
    }
    if (lane == 0) {
        g.n_own[t.row] = n_own;
        g.n_rows[t.row] = n_rows;
    }
}

constexpr uint32_t kGpOwn = 0, kGpInRun = 1, kGpRunEnd = 2;  // a staged entry: of the atom's own group / foreign / the last of its label
constexpr uint32_t kGpRowRegs = 4;  // rows [0, 64 kGpRowRegs) of an atom are counted in registers: row r in lane r % 64

// Entries [s0, s0 + n) of the reordered list -> s_run as (kind, label), padded like pt_stage's to a multiple of 4 with
// foreign entries inside a run (they hit nothing).
__device__ __forceinline__ void gp_stage_runs(const uint32_t *lab, uint32_t s0, uint32_t n, uint32_t K, uint32_t n_own,
                                              uint2 *s_run)
{
    const uint32_t n4 = pt_pad4(n);
    for (uint32_t e = lane_id(); e < n4; e += kWave) {
        uint2 v = make_uint2(kGpInRun, 0u);
        if (e < n) {
            const uint32_t q = s0 + e, l = lab[q];
            const bool last = q + 1u == K || lab[q + 1u] != l;
            v = make_uint2(q < n_own ? kGpOwn : last ? kGpRunEnd : kGpInRun, l);
        }
        s_run[e] = v;
    }
}

// Row r of the atom gains `cnt` (the same in every lane): in acc, lane r % 64's register r / 64; behind those registers
// in dst[r] itself, which lane 0 alone writes and adds to (`add`: an earlier pass has written it).
__device__ __forceinline__ void gp_row_add(uint32_t (&acc)[kGpRowRegs], uint32_t *dst, uint32_t r, uint32_t cnt, bool add)
{
    const uint32_t lane = lane_id();
    if (r < kGpRowRegs * kWave) {
        const bool mine = lane == (r & (kWave - 1u));
#pragma unroll
        for (uint32_t j = 0; j < kGpRowRegs; j++) acc[j] += mine && j == r / kWave ? cnt : 0u;
    } else if (lane == 0) {
        dst[r] = cnt + (add ? dst[r] : 0u);
    }
}

struct GpRows {  // the rows of one atom
    uint32_t *groups, *buried, *only;
    uint32_t n;
};

// Staged entries [0, n) (n a multiple of 4) of the reordered list against the NCH chunks of a pass.  An own-group
// entry's hits go to self; a foreign entry's hits on live points that self has left free go to cov, and the last entry
// of a label closes row r: cov's ballots are its buried count, and every point keeps whether one row or more than one
// has hit it and which row was the first.
template <int NCH, bool REM>
__device__ __forceinline__ void gp_test(const float4 *s_ent, const uint2 *s_run, uint32_t n, const PtPass<NCH> &ps,
                                        bool (&self)[NCH], bool (&cov)[NCH], bool (&once)[NCH], bool (&twice)[NCH],
                                        uint32_t (&first_row)[NCH], uint32_t &r, uint32_t (&acc)[kGpRowRegs],
                                        const GpRows &rows, bool first_pass)
{
    for (uint32_t k = 0; k < n; k += 4) {
        float4 e[4];
        uint2 run[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { e[u] = s_ent[k + u]; run[u] = s_run[k + u]; }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            // (the same in every lane: a branch of the wave)
            const uint32_t kind = (uint32_t)__builtin_amdgcn_readfirstlane((int)run[u].x);
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const bool hit = pt_hit<REM>(ps.sx[c], ps.sy[c], ps.sz[c], ps.rem[c], e[u]);
                // (both updates, masked by the kind: a choice between two destinations would put them in scratch)
                self[c] = self[c] || (hit && kind == kGpOwn);
                cov[c] = cov[c] || (hit && kind != kGpOwn && ps.live[c] && !self[c]);
            }
            if (kind == kGpRunEnd) {
                uint32_t cnt = 0;
#pragma unroll
                for (int c = 0; c < NCH; c++) {
                    cnt += (uint32_t)__popcll(ballot64(cov[c]));
                    twice[c] = twice[c] || (once[c] && cov[c]);
                    first_row[c] = cov[c] && !once[c] ? r : first_row[c];
                    once[c] = once[c] || cov[c];
                    cov[c] = false;
                }
                gp_row_add(acc, rows.buried, r, cnt, !first_pass);
                if (first_pass && lane_id() == 0) rows.groups[r] = run[u].y;
                r++;
            }
        }
    }
}

// The frame of k_contact_points over the list k_group_order left (own group first, then one run per foreign label, so
// the rows come out in ascending label order), one sweep per pass and no early exit.  After the sweep of a pass a
// point hit by exactly one row belongs to that row's `only` count.
template <int NCH>
__global__ __launch_bounds__(256) void k_group_points(GpArgs g)
{
    const PtArgs &a = g.p;
    __shared__ float4 s_ent[4][kPtStage];
    __shared__ uint2 s_run[4][kPtStage];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= a.b.n_atoms) return;
    const PtAtom t = pt_atom(a, g.sorted, p);
    const uint32_t *lab = g.sorted_group + t.off;
    const uint32_t n_own = g.n_own[t.row];
    const unsigned long long r0 = g.row_offsets[t.row];
    const GpRows rows = {g.groups + r0, g.buried + r0, g.only + r0, (uint32_t)(g.row_offsets[t.row + 1] - r0)};
    const auto stage = [&](uint32_t s0, uint32_t n) __attribute__((always_inline)) {
        pt_stage(a, t, s0, n, s_ent[w]);
        gp_stage_runs(lab, s0, n, t.K, n_own, s_run[w]);
    };
    pt_stage_first(t, stage);

    // an empty list: no rows, every point free
    const uint32_t n_chunks = t.K ? (a.n_points + kWave - 1) / kWave : 0u;
    float nx[NCH], ny[NCH], nz[NCH];
    pt_load_points(a, 0u, n_chunks, nx, ny, nz);
    uint32_t self_free = t.K ? 0u : a.n_points, exposed = self_free;
    uint32_t acc_b[kGpRowRegs], acc_o[kGpRowRegs];
#pragma unroll
    for (uint32_t j = 0; j < kGpRowRegs; j++) acc_b[j] = acc_o[j] = 0u;
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += NCH) {
        PtPass<NCH> ps;
        bool self[NCH], cov[NCH], once[NCH], twice[NCH];
        uint32_t first_row[NCH];
        const bool any_rem = pt_pass_begin(a, c0, n_chunks, nx, ny, nz, ps);
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            self[c] = cov[c] = once[c] = twice[c] = false;
            first_row[c] = 0u;
        }
        uint32_t r = 0;
        for (uint32_t s0 = 0; s0 < t.K; s0 += kPtStage) {
            const uint32_t n4 = pt_pad4(pt_restage(t, s0, stage));
            if (any_rem) gp_test<NCH, true>(s_ent[w], s_run[w], n4, ps, self, cov, once, twice, first_row, r, acc_b, rows, c0 == 0);
            else gp_test<NCH, false>(s_ent[w], s_run[w], n4, ps, self, cov, once, twice, first_row, r, acc_b, rows, c0 == 0);
        }
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            self_free += (uint32_t)__popcll(ballot64(ps.live[c] && !self[c]));
            exposed += (uint32_t)__popcll(ballot64(ps.live[c] && !self[c] && !once[c]));
        }
        for (uint32_t rr = 0; rr < rows.n; rr++) {
            uint32_t cnt = 0;
#pragma unroll
            for (int c = 0; c < NCH; c++) cnt += (uint32_t)__popcll(ballot64(once[c] && !twice[c] && first_row[c] == rr));
            gp_row_add(acc_o, rows.only, rr, cnt, c0 != 0);
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < kGpRowRegs; j++) {
        const uint32_t rr = j * kWave + lane;
        if (rr < rows.n) {
            rows.buried[rr] = acc_b[j];
            rows.only[rr] = acc_o[j];
        }
    }
    if (lane == 0) {
        g.self_free[t.row] = self_free;
        g.free[t.row] = exposed;
        if (a.sasa) a.sasa[t.row] = pt_sasa(t.R2, exposed, a.n_points);
    }
}

// ---- exposure vectors (rsasa_exposure_vectors*) ----

// The sum of t over the chunk's 64 lanes in the interface's order: for h = 32, 16, 8, 4, 2, 1, t[l] = t[l] + t[l + h]
// for l < h; the chunk's sum is t[0].  Lane l < h of the xor butterfly adds exactly t[l] + t[l + h] (the lanes above h
// compute sums nobody reads), so lane 0 ends with that tree.  Plain float32 adds (-ffp-contract=off, no fast-math).
__device__ __forceinline__ float ex_chunk_sum(float t)
{
#pragma unroll
    for (int h = kWave / 2; h >= 1; h >>= 1) t = t + __shfl_xor(t, h, kWave);
    return t;
}

// The frame, tests and early exit of k_accessible_points (pt_pass_occluded), no masks.  After a pass every lane holds
// occ[c] of its point of chunk c; its term is occ ? +0.0f : s per component (the lattice is zero padded and the lanes
// past n_points are occ).  A chunk sums its terms by ex_chunk_sum, the chunks are added in ascending order:
// E = chunk_0, then E = E + chunk_c.  A chunk with no exposed lane has 64 terms +0.0f, whose tree is +0.0f: that is
// added without the shuffles.  Lane 0 writes the three sums, the exposed count and the value.
template <int NCH>
__global__ __launch_bounds__(256) void k_exposure_vectors(ExArgs ex)
{
    const PtArgs &a = ex.p;
    __shared__ float4 s_ent[4][kPtStage];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= a.b.n_atoms) return;
    const PtAtom t = pt_atom(a, a.entries, p);
    const auto stage = [&](uint32_t s0, uint32_t n) __attribute__((always_inline)) { pt_stage(a, t, s0, n, s_ent[w]); };
    pt_stage_first(t, stage);

    const uint32_t n_chunks = (a.n_points + kWave - 1) / kWave;
    float nx[NCH], ny[NCH], nz[NCH];
    pt_load_points(a, 0u, n_chunks, nx, ny, nz);
    uint32_t exposed = 0;
    float ex_x = 0.0f, ex_y = 0.0f, ex_z = 0.0f;  // (E = chunk_0 overwrites them)
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += NCH) {
        PtPass<NCH> ps;
        bool occ[NCH];
        const bool any_rem = pt_pass_begin(a, c0, n_chunks, nx, ny, nz, ps);
        pt_pass_occluded(t, stage, s_ent[w], ps, any_rem, occ);
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            if (c0 + c >= n_chunks) break;  // (the same in every lane) the chunks past the last are no terms of the sum
            const unsigned long long m = ballot64(!occ[c]);
            exposed += (uint32_t)__popcll(m);
            float cx = 0.0f, cy = 0.0f, cz = 0.0f;
            if (m != 0ull) {  // (the same in every lane)
                cx = ex_chunk_sum(occ[c] ? 0.0f : ps.sx[c]);
                cy = ex_chunk_sum(occ[c] ? 0.0f : ps.sy[c]);
                cz = ex_chunk_sum(occ[c] ? 0.0f : ps.sz[c]);
            }
            const bool first = c0 + c == 0u;
            ex_x = first ? cx : ex_x + cx;
            ex_y = first ? cy : ex_y + cy;
            ex_z = first ? cz : ex_z + cz;
        }
    }
    if (lane == 0) {
        ex.vectors[(size_t)t.row * 3 + 0] = ex_x;
        ex.vectors[(size_t)t.row * 3 + 1] = ex_y;
        ex.vectors[(size_t)t.row * 3 + 2] = ex_z;
        ex.free[t.row] = exposed;
        if (a.sasa) a.sasa[t.row] = pt_sasa(t.R2, exposed, a.n_points);
    }
}

// One wave per atom, four to a workgroup: the kernel of two chunks per pass while the lattice fits one pass of it.
template <typename Args>
void pt_launch(void (*k2)(Args), void (*k4)(Args), const PtArgs &p, const Args &args, hipStream_t stream)
{
    const uint32_t n = p.b.n_atoms;
    if (!n) return;
    hipLaunchKernelGGL(p.n_points <= 2u * kWave ? k2 : k4, dim3(cdiv(n, 4)), dim3(256), 0, stream, args);
}

}  // namespace

// masks[] (and sasa[], if set) of every atom of the binned batch
void launch_accessible_points(const PtArgs &a, hipStream_t stream)
{
    pt_launch(k_accessible_points<2>, k_accessible_points<4>, a, a, stream);
}

// free[] of every atom from the masks of a finished point run
void launch_mask_free(const PtArgs &a, uint32_t *free, hipStream_t stream)
{
    const uint32_t n = a.b.n_atoms;
    if (!n) return;
    hipLaunchKernelGGL(k_mask_free, dim3(cdiv(n, 256)), dim3(256), 0, stream, a, free);
}

// covered[] and exclusive[] (and p.sasa[], if set) of every atom of the binned batch
void launch_contact_points(const CtArgs &c, hipStream_t stream)
{
    pt_launch(k_contact_points<2>, k_contact_points<4>, c.p, c, stream);
}

// owned[] (and owner[] and p.sasa[], if set) of every atom of the binned batch
void launch_contact_owners(const CoArgs &c, hipStream_t stream)
{
    pt_launch(k_contact_owners<2>, k_contact_owners<4>, c.p, c, stream);
}

// sorted[], sorted_group[], n_own[] and n_rows[] of every atom of the binned batch
void launch_group_order(const GpArgs &g, hipStream_t stream)
{
    const uint32_t n = g.p.b.n_atoms;
    if (!n) return;
    hipLaunchKernelGGL(k_group_order, dim3(cdiv(n, 4)), dim3(256), 0, stream, g);
}

// groups[], buried[] and only[] of every row, self_free[] and free[] (and p.sasa[], if set) of every atom
void launch_group_points(const GpArgs &g, hipStream_t stream)
{
    pt_launch(k_group_points<2>, k_group_points<4>, g.p, g, stream);
}

// vectors[] and free[] (and p.sasa[], if set) of every atom of the binned batch
void launch_exposure_vectors(const ExArgs &e, hipStream_t stream)
{
    pt_launch(k_exposure_vectors<2>, k_exposure_vectors<4>, e.p, e, stream);
}

}  // namespace rsasa
