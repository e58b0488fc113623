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
//   k_group_order         (rsasa_group_contacts*) one wave per atom: its list again with the entries of its own group
//                         (label) first and the others by (label, position), each entry ranked by counting the keys
//                         below its own; the number of distinct foreign labels is the atom's row count.
//   k_group_points        the layout of k_contact_points over the reordered list, one sweep per pass: the own-group
//                         entries give `self`, every run of one foreign label an OR whose ballots are the row's buried
//                         count; a point remembers the first row that hit it, which gives the rows' `only` counts.
//   k_exposure_vectors    (rsasa_exposure_vectors*) the layout, staging, tests and early exit of k_accessible_points; no
//                         masks: per atom the float32 sum of its exposed lattice points, in a fixed order (a tree over
//                         the lanes of a chunk, then the chunks ascending), and their number.
//
// Points [0, n_fused) take the fused rule - mul_add(sx, vx, mul_add(sy, vy, sz * vz)) < limit (lib.rs:143-146) -, the
// rest the remainder rule - plain products, `<=` (lib.rs:185-186,206-207).  Both rules are ORs over the list, so the
// list's order (and the reference's early exits and cached neighbour) do not change a bit.
// Compiled with -ffp-contract=off: d^2 and the remainder dot product are not fused, as in the reference.
#include "device_utils.h"

namespace rsasa {
namespace {

constexpr uint32_t kPtStage = 256;  // list entries a wave holds in LDS (4 KiB; lists are ~44 long at probe 1.4)

// Entries [s0, s0 + n) of the atom's list -> s_ent as (vx, vy, vz, limit) (lib.rs:129-136), lanes in parallel, then
// up to 3 entries (0, 0, 0, -inf) up to a multiple of 4: no point of the lattice is occluded by one (dot = 0, 0 < -inf
// and 0 <= -inf are false), so the test loop reads whole groups of four.
__device__ __forceinline__ void pt_stage(const PtArgs &a, const uint2 *ent, uint32_t s0, uint32_t n, uint32_t base,
                                         const float4 me, float R2, float twoR, float4 *s_ent)
{
    const BatchView &b = a.b;
    const uint32_t n4 = (n + 3u) & ~3u;
    for (uint32_t e = lane_id(); e < n4; e += kWave) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, -__builtin_inff());
        if (e < n) {
            const uint2 en = ent[s0 + e];
            const uint32_t j = base + en.y;                               // idx is the index within the structure
            const float vx = me.x - b.x[j], vy = me.y - b.y[j], vz = me.z - b.z[j];  // lib.rs:129-131
            const float d2 = vx * vx + vy * vy + vz * vz;                 // lib.rs:132
            const float t = __uint_as_float(en.x);                        // threshold_squared, spatial_grid.rs:336-339
            v = make_float4(vx, vy, vz, (t - d2 - R2) / twoR);            // lib.rs:136
        }
        s_ent[e] = v;
    }
}

// Staged entries [0, n) (n a multiple of 4) against the NCH chunks of a pass; REM: some lane of the pass takes the
// remainder rule (rem[c]).  Returns true once every point of the pass is occluded (lib.rs:149-152).
template <int NCH, bool REM>
__device__ __forceinline__ bool pt_test(const float4 *s_ent, uint32_t n, const float (&sx)[NCH], const float (&sy)[NCH],
                                        const float (&sz)[NCH], const bool (&rem)[NCH], bool (&occ)[NCH])
{
    for (uint32_t k = 0; k < n; k += 4) {
        float4 e[4];
#pragma unroll
        for (int u = 0; u < 4; u++) e[u] = s_ent[k + u];  // (the four LDS reads in flight together)
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                // lib.rs:143-146: mul_add(sx, vx, mul_add(sy, vy, sz * vz)) < limit
                bool hit = __builtin_fmaf(sx[c], e[u].x, __builtin_fmaf(sy[c], e[u].y, sz[c] * e[u].z)) < e[u].w;
                if (REM) {
                    // lib.rs:185-186,206-207: plain products, `<=`
                    const float dotu = sx[c] * e[u].x + sy[c] * e[u].y + sz[c] * e[u].z;
                    hit = rem[c] ? dotu <= e[u].w : hit;
                }
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

// NCH chunks of 64 points per pass: every staged entry is read once for all of them.
template <int NCH>
__global__ __launch_bounds__(256) void k_accessible_points(PtArgs a)
{
    const BatchView &b = a.b;
    __shared__ float4 s_ent[4][kPtStage];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= b.n_atoms) return;
    const uint32_t row = b.sorted_orig[p];
    const uint32_t base = b.grids[b.sid_sorted[p]].atom_begin;
    const float4 me = make_float4(b.x[row], b.y[row], b.z[row], b.radius[row]);
    const float R = me.w + b.probe;  // lib.rs:101
    const float R2 = R * R;          // lib.rs:102
    const float twoR = 2.0f * R;     // lib.rs:136
    const unsigned long long off = a.offsets[row];
    const uint32_t K = (uint32_t)(a.offsets[row + 1] - off);
    const uint2 *ent = a.entries + off;
    const bool one_stage = K <= kPtStage;
    if (one_stage && K) {
        pt_stage(a, ent, 0, K, base, me, R2, twoR, s_ent[w]);
        wave_lds_fence();
    }

    const uint32_t n_chunks = (a.n_points + kWave - 1) / kWave;
    // the points of the next pass are loaded while this one runs (the lattice arrays are zero padded to whole chunks)
    float nx[NCH], ny[NCH], nz[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const uint32_t pi = (uint32_t)c * kWave + lane;
        const bool in = (uint32_t)c < n_chunks;
        nx[c] = in ? a.lx[pi] : 0.0f;
        ny[c] = in ? a.ly[pi] : 0.0f;
        nz[c] = in ? a.lz[pi] : 0.0f;
    }
    uint32_t exposed = 0;
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += NCH) {
        float sx[NCH], sy[NCH], sz[NCH];
        bool occ[NCH], rem[NCH];
        bool any_rem = false;
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            sx[c] = nx[c]; sy[c] = ny[c]; sz[c] = nz[c];
            const uint32_t pi = (c0 + c) * kWave + lane;
            occ[c] = pi >= a.n_points;  // lanes past the last point (and chunks past the last): never exposed
            rem[c] = pi >= a.n_fused;
            any_rem = any_rem || (rem[c] && !occ[c]);
            const uint32_t nc = c0 + NCH + c;
            const bool in = nc < n_chunks;
            nx[c] = in ? a.lx[nc * kWave + lane] : 0.0f;
            ny[c] = in ? a.ly[nc * kWave + lane] : 0.0f;
            nz[c] = in ? a.lz[nc * kWave + lane] : 0.0f;
        }
        any_rem = ballot64(any_rem) != 0ull;
        for (uint32_t s0 = 0; s0 < K; s0 += kPtStage) {
            const uint32_t n = min(kPtStage, K - s0);
            if (!one_stage) {
                wave_lds_fence();  // (every lane is done with the previous stage)
                pt_stage(a, ent, s0, n, base, me, R2, twoR, s_ent[w]);
                wave_lds_fence();
            }
            const uint32_t n4 = (n + 3u) & ~3u;
            if (any_rem ? pt_test<NCH, true>(s_ent[w], n4, sx, sy, sz, rem, occ)
                        : pt_test<NCH, false>(s_ent[w], n4, sx, sy, sz, rem, occ))
                break;
        }
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
        if (lane < 2u * NCH && wi < a.words) a.masks[(size_t)row * a.words + wi] = word;
    }
    if (lane == 0 && a.sasa)  // lib.rs:220-222
        a.sasa[row] = ((4.0f * 3.14159274101257324219f) * R2) * (float)exposed * (1.0f / (float)a.n_points);
}

// ---- contact counts (rsasa_contact_points*) ----

// Staged entries [0, n) (n a multiple of 4) against the NCH chunks of a pass: entry k's hits on the points `gate`
// admits are counted into s_cnt[k].  FIRST (the first sweep): every hit also marks its point hit once, or twice once
// it was hit before.
template <int NCH, bool REM, bool FIRST>
__device__ __forceinline__ void ct_test(const float4 *s_ent, uint32_t n, const float (&sx)[NCH], const float (&sy)[NCH],
                                        const float (&sz)[NCH], const bool (&rem)[NCH], const bool (&gate)[NCH],
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
                // the tests of pt_test (lib.rs:143-146; lib.rs:185-186,206-207)
                bool hit = __builtin_fmaf(sx[c], e[u].x, __builtin_fmaf(sy[c], e[u].y, sz[c] * e[u].z)) < e[u].w;
                if (REM) {
                    const float dotu = sx[c] * e[u].x + sy[c] * e[u].y + sz[c] * e[u].z;
                    hit = rem[c] ? dotu <= e[u].w : hit;
                }
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

// One sweep of the whole list (kPtStage entries at a time) for the chunks of a pass: entry e's count goes to dst[e],
// added to what the earlier passes left there when `add`.
template <int NCH, bool FIRST>
__device__ __forceinline__ void ct_sweep(const PtArgs &a, const uint2 *ent, uint32_t K, bool one_stage, uint32_t base,
                                         const float4 me, float R2, float twoR, float4 *s_ent, uint32_t *s_cnt,
                                         uint32_t *dst, bool add, bool any_rem, const float (&sx)[NCH],
                                         const float (&sy)[NCH], const float (&sz)[NCH], const bool (&rem)[NCH],
                                         const bool (&gate)[NCH], bool (&once)[NCH], bool (&twice)[NCH])
{
    for (uint32_t s0 = 0; s0 < K; s0 += kPtStage) {
        const uint32_t n = min(kPtStage, K - s0);
        if (!one_stage) {
            wave_lds_fence();  // (every lane is done with the previous stage)
            pt_stage(a, ent, s0, n, base, me, R2, twoR, s_ent);
            wave_lds_fence();
        }
        const uint32_t n4 = (n + 3u) & ~3u;
        if (any_rem) ct_test<NCH, true, FIRST>(s_ent, n4, sx, sy, sz, rem, gate, once, twice, s_cnt);
        else ct_test<NCH, false, FIRST>(s_ent, n4, sx, sy, sz, rem, gate, once, twice, s_cnt);
        wave_lds_fence();
        // coalesced; lane l owns entries l, l + 64, ... in every pass, so what it adds to is its own earlier write
        for (uint32_t e = lane_id(); e < n; e += kWave) dst[s0 + e] = s_cnt[e] + (add ? dst[s0 + e] : 0u);
        wave_lds_fence();  // (every lane has read the counts before the next sweep writes them)
    }
}

// The layout of k_accessible_points (one wave per cell-sorted atom, lanes over NCH chunks of 64 points per pass, the
// list staged in LDS by pt_stage), without its early exit.  Per pass, sweep 1 counts each entry's hits (covered) and
// leaves every lane knowing which of its points one entry hits and which more than one; sweep 2 goes over the list
// again and counts each entry's hits on the points hit once (exclusive).
template <int NCH>
__global__ __launch_bounds__(256) void k_contact_points(CtArgs ct)
{
    const PtArgs &a = ct.p;
    const BatchView &b = a.b;
    __shared__ float4 s_ent[4][kPtStage];
    __shared__ uint32_t s_cnt[4][kPtStage];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= b.n_atoms) return;
    const uint32_t row = b.sorted_orig[p];
    const uint32_t base = b.grids[b.sid_sorted[p]].atom_begin;
    const float4 me = make_float4(b.x[row], b.y[row], b.z[row], b.radius[row]);
    const float R = me.w + b.probe;  // lib.rs:101
    const float R2 = R * R;          // lib.rs:102
    const float twoR = 2.0f * R;     // lib.rs:136
    const unsigned long long off = a.offsets[row];
    const uint32_t K = (uint32_t)(a.offsets[row + 1] - off);
    const uint2 *ent = a.entries + off;
    const bool one_stage = K <= kPtStage;
    if (one_stage && K) {
        pt_stage(a, ent, 0, K, base, me, R2, twoR, s_ent[w]);
        wave_lds_fence();
    }

    // an empty list: no counts, every point exposed
    const uint32_t n_chunks = K ? (a.n_points + kWave - 1) / kWave : 0u;
    float nx[NCH], ny[NCH], nz[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const uint32_t pi = (uint32_t)c * kWave + lane;
        const bool in = (uint32_t)c < n_chunks;
        nx[c] = in ? a.lx[pi] : 0.0f;
        ny[c] = in ? a.ly[pi] : 0.0f;
        nz[c] = in ? a.lz[pi] : 0.0f;
    }
    uint32_t exposed = K ? 0u : a.n_points;
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += NCH) {
        float sx[NCH], sy[NCH], sz[NCH];
        bool live[NCH], rem[NCH], once[NCH], twice[NCH], solo[NCH];
        bool any_rem = false;
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            sx[c] = nx[c]; sy[c] = ny[c]; sz[c] = nz[c];
            const uint32_t pi = (c0 + c) * kWave + lane;
            live[c] = pi < a.n_points;  // lanes past the last point (and chunks past the last): never counted
            rem[c] = pi >= a.n_fused;
            any_rem = any_rem || (rem[c] && live[c]);
            once[c] = twice[c] = false;
            const uint32_t nc = c0 + NCH + c;
            const bool in = nc < n_chunks;
            nx[c] = in ? a.lx[nc * kWave + lane] : 0.0f;
            ny[c] = in ? a.ly[nc * kWave + lane] : 0.0f;
            nz[c] = in ? a.lz[nc * kWave + lane] : 0.0f;
        }
        any_rem = ballot64(any_rem) != 0ull;
        ct_sweep<NCH, true>(a, ent, K, one_stage, base, me, R2, twoR, s_ent[w], s_cnt[w], ct.covered + off, c0 != 0,
                            any_rem, sx, sy, sz, rem, live, once, twice);
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            solo[c] = once[c] && !twice[c];
            exposed += (uint32_t)__popcll(ballot64(live[c] && !once[c]));
        }
        ct_sweep<NCH, false>(a, ent, K, one_stage, base, me, R2, twoR, s_ent[w], s_cnt[w], ct.exclusive + off, c0 != 0,
                             any_rem, sx, sy, sz, rem, solo, once, twice);
    }
    if (lane == 0 && a.sasa)  // lib.rs:220-222, as k_accessible_points
        a.sasa[row] = ((4.0f * 3.14159274101257324219f) * R2) * (float)exposed * (1.0f / (float)a.n_points);
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
    const BatchView &b = a.b;
    __shared__ unsigned long long s_key[4][kPtStage];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= b.n_atoms) return;
    const uint32_t row = b.sorted_orig[p];
    const uint32_t base = b.grids[b.sid_sorted[p]].atom_begin;
    const unsigned long long off = a.offsets[row];
    const uint32_t K = (uint32_t)(a.offsets[row + 1] - off);
    const uint2 *ent = a.entries + off;
    const uint32_t mine = g.group[row];
    const bool one_stage = K <= kPtStage;
    uint32_t n_own = 0, n_rows = 0;
    for (uint32_t eb = 0; eb < K; eb += kWave) {
        const uint32_t e = eb + lane;
        const bool valid = e < K;
        const uint2 en = valid ? ent[e] : make_uint2(0u, 0u);
        const uint32_t lab = valid ? g.group[base + en.y] : mine;  // idx is the index within the structure
        const unsigned long long first = gp_key(lab, mine, 0u), key = first | e;
        uint32_t rank = 0, before_label = 0;
        for (uint32_t t0 = 0; t0 < K; t0 += kPtStage) {
            const uint32_t n = min(kPtStage, K - t0);
            if (!one_stage || eb == 0) {
                wave_lds_fence();  // (every lane is done with the previous keys)
                for (uint32_t k = lane; k < n; k += kWave) s_key[w][k] = gp_key(g.group[base + ent[t0 + k].y], mine, t0 + k);
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
            g.sorted[off + rank] = en;
            g.sorted_group[off + rank] = lab;
        }
    }
    if (lane == 0) {
        g.n_own[row] = n_own;
        g.n_rows[row] = n_rows;
    }
}

constexpr uint32_t kGpOwn = 0, kGpInRun = 1, kGpRunEnd = 2;  // a staged entry: of the atom's own group / foreign / the last of its label
constexpr uint32_t kGpRowRegs = 4;  // rows [0, 64 kGpRowRegs) of an atom are counted in registers: row r in lane r % 64

// Entries [s0, s0 + n) of the reordered list -> s_run as (kind, label), padded like pt_stage's to a multiple of 4 with
// foreign entries inside a run (they hit nothing).
__device__ __forceinline__ void gp_stage_runs(const uint32_t *lab, uint32_t s0, uint32_t n, uint32_t K, uint32_t n_own,
                                              uint2 *s_run)
{
    const uint32_t n4 = (n + 3u) & ~3u;
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

// Staged entries [0, n) (n a multiple of 4) of the reordered list against the NCH chunks of a pass, with the tests of
// pt_test.  An own-group entry's hits go to self; a foreign entry's hits on live points that self has left free go to
// cov, and the last entry of a label closes row r: cov's ballots are its buried count, and every point keeps whether
// one row or more than one has hit it and which row was the first.
template <int NCH, bool REM>
__device__ __forceinline__ void gp_test(const float4 *s_ent, const uint2 *s_run, uint32_t n, const float (&sx)[NCH],
                                        const float (&sy)[NCH], const float (&sz)[NCH], const bool (&rem)[NCH],
                                        const bool (&live)[NCH], bool (&self)[NCH], bool (&cov)[NCH], bool (&once)[NCH],
                                        bool (&twice)[NCH], uint32_t (&first_row)[NCH], uint32_t &r,
                                        uint32_t (&acc)[kGpRowRegs], const GpRows &rows, bool first_pass)
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
                bool hit = __builtin_fmaf(sx[c], e[u].x, __builtin_fmaf(sy[c], e[u].y, sz[c] * e[u].z)) < e[u].w;
                if (REM) {
                    const float dotu = sx[c] * e[u].x + sy[c] * e[u].y + sz[c] * e[u].z;
                    hit = rem[c] ? dotu <= e[u].w : hit;
                }
                // (both updates, masked by the kind: a choice between two destinations would put them in scratch)
                self[c] = self[c] || (hit && kind == kGpOwn);
                cov[c] = cov[c] || (hit && kind != kGpOwn && live[c] && !self[c]);
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

// The layout of k_contact_points over the list k_group_order left (own group first, then one run per foreign label, so
// the rows come out in ascending label order), one sweep per pass and no early exit.  After the sweep of a pass a
// point hit by exactly one row belongs to that row's `only` count.
template <int NCH>
__global__ __launch_bounds__(256) void k_group_points(GpArgs g)
{
    const PtArgs &a = g.p;
    const BatchView &b = a.b;
    __shared__ float4 s_ent[4][kPtStage];
    __shared__ uint2 s_run[4][kPtStage];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= b.n_atoms) return;
    const uint32_t row = b.sorted_orig[p];
    const uint32_t base = b.grids[b.sid_sorted[p]].atom_begin;
    const float4 me = make_float4(b.x[row], b.y[row], b.z[row], b.radius[row]);
    const float R = me.w + b.probe;  // lib.rs:101
    const float R2 = R * R;          // lib.rs:102
    const float twoR = 2.0f * R;     // lib.rs:136
    const unsigned long long off = a.offsets[row];
    const uint32_t K = (uint32_t)(a.offsets[row + 1] - off);
    const uint2 *ent = g.sorted + off;
    const uint32_t *lab = g.sorted_group + off;
    const uint32_t n_own = g.n_own[row];
    const unsigned long long r0 = g.row_offsets[row];
    const GpRows rows = {g.groups + r0, g.buried + r0, g.only + r0, (uint32_t)(g.row_offsets[row + 1] - r0)};
    const bool one_stage = K <= kPtStage;
    if (one_stage && K) {
        pt_stage(a, ent, 0, K, base, me, R2, twoR, s_ent[w]);
        gp_stage_runs(lab, 0, K, K, n_own, s_run[w]);
        wave_lds_fence();
    }

    // an empty list: no rows, every point free
    const uint32_t n_chunks = K ? (a.n_points + kWave - 1) / kWave : 0u;
    float nx[NCH], ny[NCH], nz[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const uint32_t pi = (uint32_t)c * kWave + lane;
        const bool in = (uint32_t)c < n_chunks;
        nx[c] = in ? a.lx[pi] : 0.0f;
        ny[c] = in ? a.ly[pi] : 0.0f;
        nz[c] = in ? a.lz[pi] : 0.0f;
    }
    uint32_t self_free = K ? 0u : a.n_points, exposed = self_free;
    uint32_t acc_b[kGpRowRegs], acc_o[kGpRowRegs];
#pragma unroll
    for (uint32_t j = 0; j < kGpRowRegs; j++) acc_b[j] = acc_o[j] = 0u;
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += NCH) {
        float sx[NCH], sy[NCH], sz[NCH];
        bool live[NCH], rem[NCH], self[NCH], cov[NCH], once[NCH], twice[NCH];
        uint32_t first_row[NCH];
        bool any_rem = false;
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            sx[c] = nx[c]; sy[c] = ny[c]; sz[c] = nz[c];
            const uint32_t pi = (c0 + c) * kWave + lane;
            live[c] = pi < a.n_points;  // lanes past the last point (and chunks past the last): never counted
            rem[c] = pi >= a.n_fused;
            any_rem = any_rem || (rem[c] && live[c]);
            self[c] = cov[c] = once[c] = twice[c] = false;
            first_row[c] = 0u;
            const uint32_t nc = c0 + NCH + c;
            const bool in = nc < n_chunks;
            nx[c] = in ? a.lx[nc * kWave + lane] : 0.0f;
            ny[c] = in ? a.ly[nc * kWave + lane] : 0.0f;
            nz[c] = in ? a.lz[nc * kWave + lane] : 0.0f;
        }
        any_rem = ballot64(any_rem) != 0ull;
        uint32_t r = 0;
        for (uint32_t s0 = 0; s0 < K; s0 += kPtStage) {
            const uint32_t n = min(kPtStage, K - s0);
            if (!one_stage) {
                wave_lds_fence();  // (every lane is done with the previous stage)
                pt_stage(a, ent, s0, n, base, me, R2, twoR, s_ent[w]);
                gp_stage_runs(lab, s0, n, K, n_own, s_run[w]);
                wave_lds_fence();
            }
            const uint32_t n4 = (n + 3u) & ~3u;
            if (any_rem) gp_test<NCH, true>(s_ent[w], s_run[w], n4, sx, sy, sz, rem, live, self, cov, once, twice, first_row, r,
                                            acc_b, rows, c0 == 0);
            else gp_test<NCH, false>(s_ent[w], s_run[w], n4, sx, sy, sz, rem, live, self, cov, once, twice, first_row, r,
                                     acc_b, rows, c0 == 0);
        }
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            self_free += (uint32_t)__popcll(ballot64(live[c] && !self[c]));
            exposed += (uint32_t)__popcll(ballot64(live[c] && !self[c] && !once[c]));
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
        g.self_free[row] = self_free;
        g.free[row] = exposed;
        if (a.sasa)  // lib.rs:220-222, as k_accessible_points
            a.sasa[row] = ((4.0f * 3.14159274101257324219f) * R2) * (float)exposed * (1.0f / (float)a.n_points);
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

// The layout of k_accessible_points (one wave per cell-sorted atom, lanes over NCH chunks of 64 points per pass, the list
// staged by pt_stage and tested by pt_test with its early exit), no masks.  After a pass every lane holds occ[c] of its
// point of chunk c; its term is occ ? +0.0f : s per component (the lattice is zero padded and the lanes past n_points
// are occ).  A chunk sums its terms by ex_chunk_sum, the chunks are added in ascending order: E = chunk_0, then
// E = E + chunk_c.  A chunk with no exposed lane has 64 terms +0.0f, whose tree is +0.0f: that is added without the
// shuffles.  Lane 0 writes the three sums, the exposed count and the value.
template <int NCH>
__global__ __launch_bounds__(256) void k_exposure_vectors(ExArgs ex)
{
    const PtArgs &a = ex.p;
    const BatchView &b = a.b;
    __shared__ float4 s_ent[4][kPtStage];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= b.n_atoms) return;
    const uint32_t row = b.sorted_orig[p];
    const uint32_t base = b.grids[b.sid_sorted[p]].atom_begin;
    const float4 me = make_float4(b.x[row], b.y[row], b.z[row], b.radius[row]);
    const float R = me.w + b.probe;  // lib.rs:101
    const float R2 = R * R;          // lib.rs:102
    const float twoR = 2.0f * R;     // lib.rs:136
    const unsigned long long off = a.offsets[row];
    const uint32_t K = (uint32_t)(a.offsets[row + 1] - off);
    const uint2 *ent = a.entries + off;
    const bool one_stage = K <= kPtStage;
    if (one_stage && K) {
        pt_stage(a, ent, 0, K, base, me, R2, twoR, s_ent[w]);
        wave_lds_fence();
    }

    const uint32_t n_chunks = (a.n_points + kWave - 1) / kWave;
    // the points of the next pass are loaded while this one runs (the lattice arrays are zero padded to whole chunks)
    float nx[NCH], ny[NCH], nz[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const uint32_t pi = (uint32_t)c * kWave + lane;
        const bool in = (uint32_t)c < n_chunks;
        nx[c] = in ? a.lx[pi] : 0.0f;
        ny[c] = in ? a.ly[pi] : 0.0f;
        nz[c] = in ? a.lz[pi] : 0.0f;
    }
    uint32_t exposed = 0;
    float ex_x = 0.0f, ex_y = 0.0f, ex_z = 0.0f;  // (E = chunk_0 overwrites them)
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += NCH) {
        float sx[NCH], sy[NCH], sz[NCH];
        bool occ[NCH], rem[NCH];
        bool any_rem = false;
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            sx[c] = nx[c]; sy[c] = ny[c]; sz[c] = nz[c];
            const uint32_t pi = (c0 + c) * kWave + lane;
            occ[c] = pi >= a.n_points;  // lanes past the last point (and chunks past the last): never exposed
            rem[c] = pi >= a.n_fused;
            any_rem = any_rem || (rem[c] && !occ[c]);
            const uint32_t nc = c0 + NCH + c;
            const bool in = nc < n_chunks;
            nx[c] = in ? a.lx[nc * kWave + lane] : 0.0f;
            ny[c] = in ? a.ly[nc * kWave + lane] : 0.0f;
            nz[c] = in ? a.lz[nc * kWave + lane] : 0.0f;
        }
        any_rem = ballot64(any_rem) != 0ull;
        for (uint32_t s0 = 0; s0 < K; s0 += kPtStage) {
            const uint32_t n = min(kPtStage, K - s0);
            if (!one_stage) {
                wave_lds_fence();  // (every lane is done with the previous stage)
                pt_stage(a, ent, s0, n, base, me, R2, twoR, s_ent[w]);
                wave_lds_fence();
            }
            const uint32_t n4 = (n + 3u) & ~3u;
            if (any_rem ? pt_test<NCH, true>(s_ent[w], n4, sx, sy, sz, rem, occ)
                        : pt_test<NCH, false>(s_ent[w], n4, sx, sy, sz, rem, occ))
                break;
        }
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            if (c0 + c >= n_chunks) break;  // (the same in every lane) the chunks past the last are no terms of the sum
            const unsigned long long m = ballot64(!occ[c]);
            exposed += (uint32_t)__popcll(m);
            float cx = 0.0f, cy = 0.0f, cz = 0.0f;
            if (m != 0ull) {  // (the same in every lane)
                cx = ex_chunk_sum(occ[c] ? 0.0f : sx[c]);
                cy = ex_chunk_sum(occ[c] ? 0.0f : sy[c]);
                cz = ex_chunk_sum(occ[c] ? 0.0f : sz[c]);
            }
            const bool first = c0 + c == 0u;
            ex_x = first ? cx : ex_x + cx;
            ex_y = first ? cy : ex_y + cy;
            ex_z = first ? cz : ex_z + cz;
        }
    }
    if (lane == 0) {
        ex.vectors[(size_t)row * 3 + 0] = ex_x;
        ex.vectors[(size_t)row * 3 + 1] = ex_y;
        ex.vectors[(size_t)row * 3 + 2] = ex_z;
        ex.free[row] = exposed;
        if (a.sasa)  // lib.rs:220-222, as k_accessible_points
            a.sasa[row] = ((4.0f * 3.14159274101257324219f) * R2) * (float)exposed * (1.0f / (float)a.n_points);
    }
}

}  // namespace

// masks[] (and sasa[], if set) of every atom of the binned batch
void launch_accessible_points(const PtArgs &a, hipStream_t stream)
{
    const uint32_t n = a.b.n_atoms;
    if (!n) return;
    if (a.n_points <= 2u * kWave) hipLaunchKernelGGL(k_accessible_points<2>, dim3(cdiv(n, 4)), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_accessible_points<4>, dim3(cdiv(n, 4)), dim3(256), 0, stream, a);
}

// covered[] and exclusive[] (and p.sasa[], if set) of every atom of the binned batch
void launch_contact_points(const CtArgs &c, hipStream_t stream)
{
    const uint32_t n = c.p.b.n_atoms;
    if (!n) return;
    if (c.p.n_points <= 2u * kWave) hipLaunchKernelGGL(k_contact_points<2>, dim3(cdiv(n, 4)), dim3(256), 0, stream, c);
    else hipLaunchKernelGGL(k_contact_points<4>, dim3(cdiv(n, 4)), dim3(256), 0, stream, c);
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
    const uint32_t n = g.p.b.n_atoms;
    if (!n) return;
    if (g.p.n_points <= 2u * kWave) hipLaunchKernelGGL(k_group_points<2>, dim3(cdiv(n, 4)), dim3(256), 0, stream, g);
    else hipLaunchKernelGGL(k_group_points<4>, dim3(cdiv(n, 4)), dim3(256), 0, stream, g);
}

// vectors[] and free[] (and p.sasa[], if set) of every atom of the binned batch
void launch_exposure_vectors(const ExArgs &e, hipStream_t stream)
{
    const uint32_t n = e.p.b.n_atoms;
    if (!n) return;
    if (e.p.n_points <= 2u * kWave) hipLaunchKernelGGL(k_exposure_vectors<2>, dim3(cdiv(n, 4)), dim3(256), 0, stream, e);
    else hipLaunchKernelGGL(k_exposure_vectors<4>, dim3(cdiv(n, 4)), dim3(256), 0, stream, e);
}

}  // namespace rsasa
