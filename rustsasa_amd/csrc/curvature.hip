// Dot-curvature kernel (rsasa_dot_curvature*, gfx950 only): for every accessible dot a the number of dots b of its own
// structure within a reach, and eight sums over them - d2, the height h of b over a's tangent plane, and the six distinct
// entries of h * T T^t (T the unit tangential part of the chord) - as 64-bit fixed-point integers with 24 fraction bits,
// dot_fields' fixed point.  From them the host forms the least-squares mean curvature and Taubin's curvature tensor
// without normals or an eigen-solver; the definition, the drop rule and the estimator's limits: include/rustsasa_amd.h.
//
//   k_dot_curvature  k_dot_link's frame (geodesics.hip) with `reach` in place of `link`: one wave per cell-sorted atom i
//                    with free != 0, the ORDERED-pair sweep (every atom of the reach that has dots and passes the staging
//                    cut is staged, i itself among them), the reach S of k_component_link and the staging cut
//                    |c_j - c_i|^2 <= (R_i + R_j + reach + h)^2 under the same two conditions (margins hold, reach <=
//                    65536 h).  The proofs there ("The staging cut" in geodesics.hip, the reach in components.hip) speak
//                    only of d2 against the squared length and of nothing a lane does behind the hit test: they carry over
//                    unchanged - no dot pair with d2 <= reach * reach is left out, and one that ties with it is seen.
//                    What is new.  A lane that owns dot a = (i, k) also holds its normal n = s_k, the lattice point
//                    itself.  Behind the hit test d2 <= reach2 && b != a it computes, in plain float32,
//                        h = (n.x*dx + n.y*dy) + n.z*dz;  t = d - h n;  t2 = (tx*tx + ty*ty) + tz*tz;  g = h / t2
//                    - one correctly rounded division per accepted pair - and the eight terms; the pair counts iff d2 > 0,
//                    t2 > 0 and every |term| <= 2^24 (a NaN fails), for all nine columns or for none.  A term is converted
//                    as in fields.hip: term * 2^24 is exact, v_rndne rounds it to nearest even, and the add is an UNSIGNED
//                    64-bit add, so that the wrap is defined.
//                    The accumulators.  pairs and the eight sums are the lane's own state, loaded from and stored to its
//                    own row per staging round and chunk of own dots, as k_dot_link does with its count: the host zeroes
//                    both buffers first, so every row is written, the all-zero ones too.  A row has one owner - the lane
//                    that holds the dot, in the one wave of its atom: plain vector loads and stores, no atomic anywhere.
//                    The other choice - the sums in registers across the whole sweep, the loop over the chunks of own dots
//                    hoisted outside it - repeats the run tables and the staging once per chunk (two at 100 points, 15 at
//                    960) to save 17 dwords of load and store per lane and staging round, a few dozen rounds against
//                    thousands of pair tests: chosen by this reasoning, NOT by measurement; the hoisted variant was not
//                    written.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   kernel            VGPRs  SGPRs  LDS (bytes)  scratch
//   k_dot_curvature     122    102        17408        0     (k_dot_link's LDS; four waves per SIMD where k_dot_link, at 91
//                                                          to 96 VGPRs, runs five: the 17 accumulator registers, the
//                                                          normal and the terms' temporaries cost the fifth wave)
// Measured: DESIGN 5s.
// Compiled with -ffp-contract=off: q, d2, h, t, t2 and the terms are not fused (the definition is the model's plain
// float32); the division is the correctly rounded one (the compiler's default for HIP), subnormals are kept.
#include "shell_sweep.h"

namespace rsasa {
namespace {

// |term| <= 2^24 (a NaN fails)
__device__ __forceinline__ bool cv_fits(float t) { return fabsf(t) <= 0x1p24f; }

// rint(term * 2^24) of a term that fits, as the 64 bits an unsigned add takes
__device__ __forceinline__ unsigned long long cv_fixed(float t) { return (unsigned long long)__float2ll_rn(t * 0x1p24f); }

__global__ __launch_bounds__(256) void k_dot_curvature(CvArgs cv)
{
    const CcArgs &c = cv.c;
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
    const uint32_t *me_mask = a.masks + (size_t)me_orig * a.words;
    const ShCell cell = sh_cell(g, me);
    uint32_t s_end = cell.s_last;  // the last shell of the reach (k_component_link's, c.link being the reach)
    if (sh_margins_hold(g, b.probe)) {
        const float t = c.link / g.cell_size + 2.5f;
        if (t < (float)cell.s_last) {
            uint32_t S = (uint32_t)ceilf(t);
            while (((float)S - 2.5f) * g.cell_size < c.link) S++;
            s_end = min(S, cell.s_last);
        }
    }
    const uint32_t n_chunks = (a.n_points + kWave - 1) / kWave;
    // The staging cut (k_dot_link's: see the head of geodesics.hip)
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
                        keep = ex * ex + ey * ey + ez * ez <= lim * lim;  // (a NaN fails: its dots pair with nobody)
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
                    const float nx = a.lx[pi], ny = a.ly[pi], nz = a.lz[pi];  // the dot's normal: its lattice point
                    const float ax = me.x + me_R * nx, ay = me.y + me_R * ny, az = me.z + me_R * nz;
                    // the lane's row so far: its own, nobody else's
                    uint32_t n_pairs = 0;
                    unsigned long long sum[kCurvColumns];
#pragma unroll
                    for (uint32_t col = 0; col < kCurvColumns; col++) sum[col] = 0ull;
                    unsigned long long *row = cv.moments + (size_t)my_dot * kCurvColumns;
                    if (mine) {
                        n_pairs = cv.pairs[my_dot];
#pragma unroll
                        for (uint32_t col = 0; col < kCurvColumns; col++) sum[col] = row[col];
                    }
                    // ---- against the staged atoms' dots, 64 points at a time
                    uint32_t seen = 0;  // lane l: the dots of staged atom l in the chunks before this one
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
                                const float dx = bx - ax, dy = by - ay, dz = bz - az;
                                const float d2 = dx * dx + dy * dy + dz * dz;
                                if (mine && d2 <= c.link2 && dot != my_dot) {
                                    const float h = (nx * dx + ny * dy) + nz * dz;
                                    const float tx = dx - h * nx, ty = dy - h * ny, tz = dz - h * nz;
                                    const float xx = tx * tx, yy = ty * ty, zz = tz * tz;
                                    const float t2 = (xx + yy) + zz;
                                    if (d2 > 0.0f && t2 > 0.0f) {
                                        const float gq = h / t2;
                                        const float e2 = xx * gq, e3 = yy * gq, e4 = zz * gq;
                                        const float e5 = (tx * ty) * gq, e6 = (tx * tz) * gq, e7 = (ty * tz) * gq;
                                        if (cv_fits(d2) && cv_fits(h) && cv_fits(e2) && cv_fits(e3) && cv_fits(e4) &&
                                            cv_fits(e5) && cv_fits(e6) && cv_fits(e7)) {
                                            n_pairs++;
                                            sum[0] += cv_fixed(d2);
                                            sum[1] += cv_fixed(h);
                                            sum[2] += cv_fixed(e2);
                                            sum[3] += cv_fixed(e3);
                                            sum[4] += cv_fixed(e4);
                                            sum[5] += cv_fixed(e5);
                                            sum[6] += cv_fixed(e6);
                                            sum[7] += cv_fixed(e7);
                                        }
                                    }
                                }
                            }
                        }
                    }
                    if (mine) {
                        cv.pairs[my_dot] = n_pairs;
#pragma unroll
                        for (uint32_t col = 0; col < kCurvColumns; col++) row[col] = sum[col];
                    }
                }
            }
        }
    }
}

}  // namespace

// pairs[] and moments[][8] of the n_dots (>= 1, < 2^32) dots that cv.c.dot_offsets counts; the caller has zeroed both
void launch_dot_curvature(const CvArgs &cv, hipStream_t stream)
{
    const uint32_t n = cv.c.p.b.n_atoms;
    if (!n || !cv.c.n_dots) return;
    hipLaunchKernelGGL(k_dot_curvature, dim3(cdiv(n, 4)), dim3(256), 0, stream, cv);
}

}  // namespace rsasa
