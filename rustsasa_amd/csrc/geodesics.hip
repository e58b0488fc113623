// Dot-graph kernels (rsasa_dot_links*, rsasa_dot_geodesics*, gfx950 only): the graph that rsasa_surface_components*
// builds and throws away - two accessible dots of a structure are linked when their float32 d2 <= link * link - kept as
// per-dot lists, and the shortest float32 distance along it from a set of seed dots.  Dots, numbering, q and the edge
// test are those of components.hip; the definitions: include/rustsasa_amd.h.
//
//   k_dot_link<kCount>    the sweep and the reach of k_component_link (see there: its proof that no linked
//                         pair lies beyond shell S does not depend on which pairs a wave keeps), one wave per cell-sorted
//                         atom i with free != 0, but over ORDERED pairs: every atom of the reach with free != 0 that passes
//                         the staging cut below is staged, whether it stands before or after i.  A lane holds one dot of
//                         i per chunk of 64 points and counts the dots b != a with d2 <= link * link into counts[a].
//   (launch_neighbor_scan)  counts -> link_offsets[n_dots + 1], 64 bits, batch-global.
//   k_dot_link<kFill>     the same sweep; the lane writes (d2 bits, b's dot number within the structure) at
//                         link_offsets[a] + cursor[a]++ - only below link_offsets[a + 1]: every write is bounded by the count.
//   k_dot_link<kWeights>  the fill of the geodesics: (bits of sqrtf(d2), b's batch-wide dot number); no sort follows.
//   k_link_sort           one lane per dot: a list is ranked by the key (d2 bits << 32) | idx - the keys of a list are
//                         distinct, idx being - from the unsorted copy into the caller's order.  No staging: a list of any
//                         length takes the same path, L * L comparisons (L = 8 on average, 26 at most on a protein at the
//                         default link; quadratic, and serial in the lane: the header says so).  A cursor that differs from the count raises NbInfo::mismatch, as k_within_fill
//                         does, and the host answers RSASA_ERR_INTERNAL.
//
// The staging cut.  The reach S covers (2 S + 1)^3 cells, a few hundred atoms at the default link, of which only those
// within R_i + R_j + link of i can hold a linked dot.  In a structure that passes sh_margins_hold, and for link <= 65536 h,
// k_dot_link stages atom j only if the float32 |c_j - c_i|^2 <= (R_i + R_j + link + h)^2.  Nothing is lost: a dot lies
// within R of its centre, so two dots with exact distance t have centres no further apart than R_i + R_j + t; the
// float32 d2 <= link * link bounds t by link plus the roundings of q and d - a few h / 128 each, the coordinates being at
// most 65536 h - and of d2 and link * link - a few 2^-24 of link, under h / 64 for link <= 65536 h; the cut's own
// arithmetic errs by as little.  All of that is below h / 8; the cut leaves a whole h.  A NaN anywhere fails the test,
// and such an atom's dots link nothing.  Without the margins, or with a longer link, every atom of the reach is staged.
// (k_component_link has no such cut and stays as it is.)
// k_dot_link writes the loops of sh_sweep (shell_sweep.h: the driver and its contract) out as k_component_link does, and
// follows a change there and in k_component_link: the two bodies are the same text but for the staged atoms, the lane's
// state, what an accepted pair does and what the lane stores.  One function template for both, the four differences as
// inline members of a policy struct, was built and timed on the MI355X (profiles/dot_pairs_ab.txt): the same registers
// and LDS, k_component_link 5 % and the count 11 % faster, but of the fill and the weights one was always slower than
// here (2 to 3 %, or 0.4 % against a run-to-run range of 0.1 %), whichever place the policy's per-wave set-up took.
//
// Ordered pairs or atomics.  k_component_link takes every unordered pair of atoms once; lists need both directions.  With
// unordered pairs the dot of the staged atom would get its entry from a lane that does not own it: a global atomic per
// accepted pair on the count AND on the cursor of the fill, and the order of a list would depend on the schedule before
// the sort.  With ordered pairs the sweep does twice the distance tests (dots are formed once per wave and tested in 64
// lanes, 8.3 accepted of several thousand tested per dot), but count and cursor belong to one lane: plain loads and stores,
// no atomic anywhere in the build.  Chosen by this reasoning, NOT by measurement: the unordered variant was not written.
//
// The relaxation.  dist[] holds float32 bits; every value is >= +0, so the bits order like the numbers and a minimum is
// an unsigned atomicMin.  Round t (t = 2, 3, ...): a dot u with stamp[u] >= t - 1 - its value fell in the previous round
// or already in this one - reads dist[u] and pushes nd = dist[u] + w (one float32 addition) to every neighbour v with
// nd <= limit and nd < dist[v]; a push that lowers dist[v] sets stamp[v] = t and the round's flag.  Invariant between
// rounds: an edge (u, v) with fl(dist[u] + w) <= limit and below dist[v] has stamp[u] >= t - 1 (whoever lowered dist[u]
// stamped it in that round, after which u pushes what it then reads or is lowered and stamped again).  A round that
// lowers nothing therefore leaves the least solution of
//     dist[v] = min(seed ? 0 : inf, min_u fl(dist[u] + w(u, v))), values above limit replaced by inf:
// every value ever stored is the length of a real path from a seed (so >= the least solution), and addition of a
// non-negative float32 is monotone (so the fixed point reached from above is the least one) - whatever the schedule.
// Every pending dot pushes in every round, so round t has settled all paths of t - 1 hops: at most n_dots rounds and one
// more that finds nothing; the host reads the flags every kGdRounds rounds and gives up (RSASA_ERR_INTERNAL) past that.
// source[] is a second phase over the converged dist[]: source[v] = min(seed ? v : none, min over u with
// fl(dist[u] + w) == dist[v] finite of source[u]), the same push with an unsigned minimum.  (Packed into one 64-bit
// minimum with dist it would not be monotone: two distances can round to the same sum.)
// Plain 32-bit vector loads and stores and relaxed agent-scope atomics; nothing else.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   kernel                 VGPRs  SGPRs  LDS (bytes)  scratch
//   k_dot_link<kCount>        91     90        17408        0
//   k_dot_link<kFill>         96     96        17408        0
//   k_dot_link<kWeights>      94     99        17408        0     (k_component_link: the same LDS; five waves per SIMD each)
//   k_link_sort               16     18            0        0
//   k_geo_init                16     26            0        0
//   k_geo_relax               14     33            0        0
//   k_geo_restamp              4     14            0        0
//   k_geo_source              16     37            0        0
// Compiled with -ffp-contract=off: q, d2 and dist + w are not fused (the definition is the model's plain float32
// arithmetic); sqrtf is the correctly rounded one (the compiler's default for HIP), the host's bit for bit.
#include "shell_sweep.h"

namespace rsasa {
namespace {

enum : int { kCount = 0, kFill = 1, kWeights = 2 };

constexpr uint32_t kInfBits = 0x7F800000u;
constexpr uint32_t kNoSource = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t gd_load(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void gd_store(uint32_t *p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int MODE>
__global__ __launch_bounds__(256) void k_dot_link(GdArgs gd)
{
    const CcArgs &c = gd.c;
    const PtArgs &a = c.p;
    const BatchView &b = a.b;
    __shared__ uint32_t s_excl[4][kShRuns], s_start[4][kShRuns];
    __shared__ float4 s_atom[4][kWave];   // (c_j, R_j) of the staged atoms
    __shared__ uint2 s_who[4][kWave];     // (input row, its first dot)
    __shared__ uint2 s_bits[4][kWave];    // their mask words of the current chunk
    __shared__ uint32_t s_dot0[4][kWave];  // their first dot of the current chunk
    __shared__ float4 s_lat[4][kWave];    // the lattice points of the current chunk
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= b.n_atoms) return;
    const uint32_t me_orig = b.sorted_orig[p];
    if (c.free[me_orig] == 0u) return;  // (the same in every lane; the kernel has no workgroup barrier)
    const StructGrid g = b.grids[b.sid_sorted[p]];
    const float4 me = b.sorted_xyzr[p];
    const float me_R = me.w + b.probe;
    const uint32_t me_dot0 = (uint32_t)c.dot_offsets[me_orig];
    const uint32_t base = MODE == kFill ? (uint32_t)c.dot_offsets[g.atom_begin] : 0u;  // the structure's first dot
    const uint32_t *me_mask = a.masks + (size_t)me_orig * a.words;
    const ShCell cell = sh_cell(g, me);
    uint32_t s_end = cell.s_last;  // the last shell of the reach (k_component_link's)
    if (sh_margins_hold(g, b.probe)) {
        const float t = c.link / g.cell_size + 2.5f;
        if (t < (float)cell.s_last) {
            uint32_t S = (uint32_t)ceilf(t);
            while (((float)S - 2.5f) * g.cell_size < c.link) S++;
            s_end = min(S, cell.s_last);
        }
    }
    const uint32_t n_chunks = (a.n_points + kWave - 1) / kWave;
    // The staging cut (see the head of the file): where the margins hold and link is no more than 65536 h, an atom whose
    // centre lies further from i's than R_i + R_j + link + h has no dot linked to a dot of i.
    const bool cut = sh_margins_hold(g, b.probe) && c.link <= 65536.0f * g.cell_size;
    const float cut_base = me_R + c.link + g.cell_size;

    for (uint32_t s = 0; s <= s_end; s++) {
        const ShShell shell = sh_shell(g, cell, s);
        for (unsigned long long r0 = 0; r0 < shell.n_rows; r0 += kWave) {
            const uint32_t total = sh_step_runs(b, g, cell, shell, s, r0, s_excl[w], s_start[w]);
            for (uint32_t f0 = 0; f0 < total; f0 += kWave) {
                // ---- lanes over the atoms of the runs: those with accessible points are staged, i itself among them
                const uint32_t f = f0 + lane;
                bool keep = false;
                uint32_t q = 0, orig = 0;
                if (f < total) {
                    q = sh_pos(s_excl[w], s_start[w], f);
                    orig = b.sorted_orig[q];
                    keep = c.free[orig] != 0u;
                    if (keep && cut) {
                        const float4 o = b.sorted_xyzr[q];
                        const float ex = o.x - me.x, ey = o.y - me.y, ez = o.z - me.z;
                        const float lim = cut_base + (o.w + b.probe);
                        keep = ex * ex + ey * ey + ez * ez <= lim * lim;  // (a NaN fails: its dots link nothing)
                    }
                }
                const unsigned long long m = ballot64(keep);
                if (m == 0ull) continue;  // (the same in every lane)
                const uint32_t n_staged = (uint32_t)__popcll(m);
                const uint32_t slot = mbcnt64(m);
                wave_lds_fence();  // (every lane is done with the previous atoms)
                if (keep) {
                    const float4 o = b.sorted_xyzr[q];
                    s_atom[w][slot] = make_float4(o.x, o.y, o.z, o.w + b.probe);  // R_j = r_j + p
                    s_who[w][slot] = make_uint2(orig, (uint32_t)c.dot_offsets[orig]);
                }
                wave_lds_fence();
                // ---- i's own dots, 64 points at a time
                uint32_t me_seen = 0;  // i's dots in the chunks before this one
                for (uint32_t co = 0; co < n_chunks; co++) {
                    const uint32_t pi = co * kWave + lane;
                    const uint32_t o0 = 2u * co, o1 = 2u * co + 1u;
                    const uint32_t own = lane < 32u ? (o0 < a.words ? me_mask[o0] : 0u) : (o1 < a.words ? me_mask[o1] : 0u);
                    const bool mine = pi < a.n_points && ((own >> (lane & 31u)) & 1u);
                    const unsigned long long mm = ballot64(mine);
                    const uint32_t my_dot = me_dot0 + me_seen + mbcnt64(mm);  // this lane's dot (if `mine`)
                    me_seen += (uint32_t)__popcll(mm);
                    if (mm == 0ull) continue;
                    const float ax = me.x + me_R * a.lx[pi], ay = me.y + me_R * a.ly[pi], az = me.z + me_R * a.lz[pi];
                    // the lane's count so far, or its cursor and the bounds of its segment: its own, nobody else's
                    uint32_t k = 0, len = 0;
                    unsigned long long off = 0;
                    if (mine) {
                        if (MODE == kCount) {
                            k = gd.counts[my_dot];
                        } else {
                            k = gd.cursor[my_dot];
                            off = gd.link_offsets[my_dot];
                            len = (uint32_t)(gd.link_offsets[my_dot + 1u] - off);
                        }
                    }
                    // ---- against the staged atoms' dots, 64 points at a time
                    uint32_t seen = 0;  // lane k: the dots of staged atom k in the chunks before this one
                    uint2 bits = make_uint2(0u, 0u);
                    for (uint32_t cj = 0; cj < n_chunks; cj++) {
                        const uint32_t pj = cj * kWave + lane;
                        wave_lds_fence();  // (every lane is done with the previous chunk's words and points)
                        s_lat[w][lane] = make_float4(a.lx[pj], a.ly[pj], a.lz[pj], 0.0f);  // (zero padded to whole chunks)
                        if (lane < n_staged) {
                            seen += (uint32_t)(__popc(bits.x) + __popc(bits.y));
                            const uint32_t *mw = a.masks + (size_t)s_who[w][lane].x * a.words;
                            const uint32_t w0 = 2u * cj, w1 = 2u * cj + 1u;
                            bits = make_uint2(w0 < a.words ? mw[w0] : 0u, w1 < a.words ? mw[w1] : 0u);
                            const uint32_t left = a.n_points - cj * kWave;  // (>= 1) the points of this chunk and after
                            if (left < 32u) bits.x &= (1u << left) - 1u;
                            if (left <= 32u) bits.y = 0u;
                            else if (left < 64u) bits.y &= (1u << (left - 32u)) - 1u;
                            s_bits[w][lane] = bits;
                            s_dot0[w][lane] = s_who[w][lane].y + seen;
                        }
                        wave_lds_fence();
                        for (uint32_t j = 0; j < n_staged; j++) {
                            const uint2 kb = s_bits[w][j];  // (the same address in every lane: a broadcast)
                            unsigned long long jm = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)kb.y) << 32) |
                                                    (uint32_t)__builtin_amdgcn_readfirstlane((int)kb.x);
                            if (jm == 0ull) continue;
                            const float4 o = s_atom[w][j];
                            uint32_t dot = s_dot0[w][j];
                            for (; jm; jm &= jm - 1ull, dot++) {
                                const float4 sp = s_lat[w][__builtin_ctzll(jm)];
                                const float bx = o.x + o.w * sp.x, by = o.y + o.w * sp.y, bz = o.z + o.w * sp.z;
                                const float dx = ax - bx, dy = ay - by, dz = az - bz;
                                const float d2 = dx * dx + dy * dy + dz * dz;
                                if (mine && d2 <= c.link2 && dot != my_dot) {
                                    if (MODE != kCount && k < len)
                                        gd.raw[off + k] = MODE == kFill ? make_uint2(__float_as_uint(d2), dot - base)
                                                                        : make_uint2(__float_as_uint(sqrtf(d2)), dot);
                                    k++;
                                }
                            }
                        }
                    }
                    if (mine) {
                        if (MODE == kCount) gd.counts[my_dot] = k;
                        else gd.cursor[my_dot] = k;
                    }
                }
            }
        }
    }
}

// One lane per dot: its list from raw[] to out[] by rank (see the head of the file).
__global__ __launch_bounds__(256) void k_link_sort(GdArgs gd)
{
    const unsigned long long d = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (d >= gd.c.n_dots) return;
    const unsigned long long off = gd.link_offsets[d];
    const uint32_t len = (uint32_t)(gd.link_offsets[d + 1ull] - off);
    const uint32_t k = gd.cursor[d];
    if (k != len) atomicOr(&gd.info->mismatch, 1ull);
    const uint32_t n = min(k, len);
    for (uint32_t i = 0; i < n; i++) {
        const uint2 e = gd.raw[off + i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; j++) {
            const uint2 o = gd.raw[off + j];
            rank += (o.x < e.x || (o.x == e.x && o.y < e.y)) ? 1u : 0u;
        }
        gd.out[off + rank] = e;
    }
}

// One wave per atom: dist, stamp and source of its dots from the seed bytes; the fill's cursors are checked here.
__global__ __launch_bounds__(256) void k_geo_init(GdArgs gd)
{
    const CcArgs &c = gd.c;
    const BatchView &b = c.p.b;
    const uint32_t p = blockIdx.x * 4u + threadIdx.x / kWave;
    if (p >= b.n_atoms) return;
    const uint32_t orig = b.sorted_orig[p];
    const uint32_t base = (uint32_t)c.dot_offsets[b.grids[b.sid_sorted[p]].atom_begin];  // the structure's first dot
    const uint32_t d1 = (uint32_t)c.dot_offsets[orig + 1u];
    for (uint32_t d = (uint32_t)c.dot_offsets[orig] + lane_id(); d < d1; d += kWave) {
        if (gd.cursor[d] != (uint32_t)(gd.link_offsets[d + 1u] - gd.link_offsets[d])) atomicOr(&gd.info->mismatch, 1ull);
        const bool seed = gd.seeds[d] != 0;
        gd.dist[d] = seed ? 0u : kInfBits;
        gd.stamp[d] = seed ? 1u : 0u;
        if (gd.source) gd.source[d] = seed ? d - base : kNoSource;
    }
}

// Round `round` (>= 2) of the relaxation (see the head of the file); flag: this round's word of GdArgs::flags.
__global__ __launch_bounds__(256) void k_geo_relax(GdArgs gd, uint32_t round, uint32_t *flag)
{
    const unsigned long long u = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (u >= gd.c.n_dots) return;
    if (gd_load(gd.stamp + u) < round - 1u) return;
    const float du = __uint_as_float(gd_load(gd.dist + u));
    const unsigned long long e0 = gd.link_offsets[u], e1 = gd.link_offsets[u + 1ull];
    bool changed = false;
    for (unsigned long long e = e0; e < e1; e++) {
        const uint2 en = gd.raw[e];
        const float nd = du + __uint_as_float(en.x);
        if (!(nd <= gd.limit) || en.y >= gd.c.n_dots) continue;  // (an entry a failed fill left unwritten names no dot)
        const uint32_t nb = __float_as_uint(nd);
        if (nb < gd_load(gd.dist + en.y) && nb < atomicMin(gd.dist + en.y, nb)) {
            gd_store(gd.stamp + en.y, round);
            changed = true;
        }
    }
    if (changed) gd_store(flag, 1u);
}

// The dots that have a source start the second phase: stamp = 1 (rounds count from 2 again).
__global__ __launch_bounds__(256) void k_geo_restamp(GdArgs gd)
{
    const unsigned long long d = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (d < gd.c.n_dots) gd.stamp[d] = gd.source[d] != kNoSource ? 1u : 0u;
}

// Round `round` of the source phase: the smallest source travels along the tight edges of the converged dist[].
__global__ __launch_bounds__(256) void k_geo_source(GdArgs gd, uint32_t round, uint32_t *flag)
{
    const unsigned long long u = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (u >= gd.c.n_dots) return;
    if (gd_load(gd.stamp + u) < round - 1u) return;
    const uint32_t su = gd_load(gd.source + u);
    if (su == kNoSource) return;
    const float du = __uint_as_float(gd.dist[u]);
    const unsigned long long e0 = gd.link_offsets[u], e1 = gd.link_offsets[u + 1ull];
    bool changed = false;
    for (unsigned long long e = e0; e < e1; e++) {
        const uint2 en = gd.raw[e];
        const uint32_t nb = __float_as_uint(du + __uint_as_float(en.x));
        if (nb == kInfBits || en.y >= gd.c.n_dots || nb != gd.dist[en.y]) continue;  // (no NaN: du and w are no NaN and not both infinite of unlike sign)
        if (su < gd_load(gd.source + en.y) && su < atomicMin(gd.source + en.y, su)) {
            gd_store(gd.stamp + en.y, round);
            changed = true;
        }
    }
    if (changed) gd_store(flag, 1u);
}

}  // namespace

// counts[] of the n_dots (>= 1, < 2^31) dots that c.dot_offsets counts; the caller has zeroed them
void launch_dot_link_count(const GdArgs &gd, hipStream_t stream)
{
    const uint32_t n = gd.c.p.b.n_atoms;
    if (!n || !gd.c.n_dots) return;
    hipLaunchKernelGGL(k_dot_link<kCount>, dim3(cdiv(n, 4)), dim3(256), 0, stream, gd);
}

// The lists behind link_offsets (total >= 1), the caller having zeroed cursor[]: sorted into out[] with idx within the
// structure and d2 (weights false), or left in raw[] in sweep order with batch-wide idx and sqrtf(d2) (weights true)
void launch_dot_link_fill(const GdArgs &gd, bool weights, hipStream_t stream)
{
    const uint32_t n = gd.c.p.b.n_atoms;
    if (!n || !gd.c.n_dots) return;
    if (weights) {
        hipLaunchKernelGGL(k_dot_link<kWeights>, dim3(cdiv(n, 4)), dim3(256), 0, stream, gd);
        return;
    }
    hipLaunchKernelGGL(k_dot_link<kFill>, dim3(cdiv(n, 4)), dim3(256), 0, stream, gd);
    hipLaunchKernelGGL(k_link_sort, dim3((uint32_t)((gd.c.n_dots + 255ull) / 256ull)), dim3(256), 0, stream, gd);
}

void launch_geodesic_init(const GdArgs &gd, hipStream_t stream)
{
    const uint32_t n = gd.c.p.b.n_atoms;
    if (!n || !gd.c.n_dots) return;
    hipLaunchKernelGGL(k_geo_init, dim3(cdiv(n, 4)), dim3(256), 0, stream, gd);
}

void launch_geodesic_restamp(const GdArgs &gd, hipStream_t stream)
{
    if (!gd.c.n_dots) return;
    hipLaunchKernelGGL(k_geo_restamp, dim3((uint32_t)((gd.c.n_dots + 255ull) / 256ull)), dim3(256), 0, stream, gd);
}

// kGdRounds rounds, the first of them round `first` (>= 2), of the relaxation (source false) or of the source phase;
// round first + k leaves its verdict in gd.flags[k], which the caller has zeroed
void launch_geodesic_rounds(const GdArgs &gd, bool source, uint32_t first, hipStream_t stream)
{
    if (!gd.c.n_dots) return;
    const dim3 grid((uint32_t)((gd.c.n_dots + 255ull) / 256ull));
    for (uint32_t k = 0; k < kGdRounds; k++) {
        if (source) hipLaunchKernelGGL(k_geo_source, grid, dim3(256), 0, stream, gd, first + k, gd.flags + k);
        else hipLaunchKernelGGL(k_geo_relax, grid, dim3(256), 0, stream, gd, first + k, gd.flags + k);
    }
}

}  // namespace rsasa
