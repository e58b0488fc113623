// Dot-enclosure kernel (rsasa_dot_enclosure*, gfx950 only): for every accessible dot the directions of a fixed fan in
// which a probe centre leaving the dot on a straight path is stopped by an obstacle atom of its own structure within
// the reach L - one bit per direction -, from the cell grid of a finished point run (the masks of k_accessible_points,
// their popcounts free[], the scan of those, the flags in cell-sorted order: what k_dot_crowding starts from).
//
//   k_dot_enclosure  k_dot_crowding's frame (crowding.hip), run by sh_sweep (shell_sweep.h): one wave per cell-sorted atom
//                    i, four waves per workgroup; a wave whose atom has no accessible point leaves at once.  LANES OWN
//                    DOTS, kDePass = 128 to a pass, compacted from the mask into LDS by rank; a lane holds its dots as
//                    q = c_i + R_i * s_k, R_i = r_i + p, float32, unfused.  A pass of more than 32 dots gives lane l the
//                    dots l and 64 + l; a pass of n <= 32 dots is spread over P lanes, P the power of two >= n, and the
//                    G = 64 / P groups of lanes hold the same dots and take the staged obstacles g, g + G, ... in turn.
//                    A lane keeps ONE uint32 per dot, bit m: ray m is stopped.  It starts as the own-atom rule,
//                    u_m . s_k < 0 for an owner with the obstacle bit (from s_k alone, once per dot); the owner itself is
//                    dropped at staging by its cell-sorted position.  The sweep's `visit`: lanes go over the atoms of a
//                    step's runs, 64 at a time; the obstacles that pass the staging cut (below) are compacted into LDS
//                    as (c_j, R2_j = R_j * R_j) with the lane cut's square beside them; then every lane evaluates, for
//                    each of its dots, dx = c_j.x - q.x, d2 = dx*dx + dy*dy + dz*dz and - where d2 passes the lane cut -
//                    the header's test for m = 0 .. n_dirs - 1,
//                        t = dx*u.x + dy*u.y + dz*u.z;   t > 0  and  (t <= L ? d2 - t*t : |d - L u|^2) <= R2_j,
//                    both arms computed and one selected (no branch inside the loop); u_m and L * u_m are read from the
//                    kernel's arguments with the loop's counter, which is the same in every lane: scalar loads of 32
//                    bytes.  A NaN fails its comparison and sets no bit.  After the sweep the groups' words are OR-ed
//                    over the lanes that hold the same dot (log2 G shuffles) and a lane of group 0 writes its dots'
//                    words: the wave alone owns the rows [dot_offsets[i], dot_offsets[i + 1]), so plain stores, and
//                    every word is written, the zero ones too (the buffer holds an earlier call's data).
//
// Notation for the proofs: eps = 2^-24; a float32 sum, difference or product is the exact one times (1 + d), |d| <= eps,
// unless it underflows, which costs at most 2^-149 absolute.  d = (dx, dy, dz) is the COMPUTED vector of the definition.
// |u_m| <= 1 + 2^-20: a lattice point's components are products of float32 libm sines and cosines of one angle pair.
//
// (A) A stopped ray has |d| <= (L + |R_j|)(1 + 2^-20).  Arm t <= L: the float32 value of d2 - t*t is <= R2, so
//     d2 <= R2 (1 + 2 eps) + fl(t*t) (1 + eps), and 0 < t <= L as float32 numbers gives fl(t*t) <= L^2 (1 + eps): the
//     computed t is never compared with the exact projection, so the cancellation in the dot product plays no part.
//     d2 >= |d|^2 (1 - eps)^3.  Together |d|^2 <= (L^2 + R_j^2)(1 + 7 eps) <= (L + |R_j|)^2 (1 + 7 eps).  Arm t > L:
//     e = fl(d - fl(L u)) has |e|^2 (1 - eps)^3 <= fl(e2) <= R2 <= R_j^2 (1 + eps), and d = e / (1 + b) + L u (1 + a)
//     per component with |a|, |b| <= eps, so |d| <= |e| (1 + 2 eps) + L |u| (1 + eps) <= (|R_j| + L)(1 + 2^-20).
//     Only relative roundings: both bounds hold up to the underflows' 2^-149, which the 1e-30 guards below keep 2^50
//     times under the slack.
//
// The stop rule.  In a structure that passes sh_margins_hold every 0 <= R_j <= h, and an atom j not seen after shell s
// has, along some axis, |dx| > (s - 1.25) h for every dot of i - crowding.hip, "The stop rule", which rests on
// shell_sweep.h, "What an unseen atom implies"; dx is the same float32 difference here.  So |d| > (s - 1.25) h.  The
// sweep stops after shell s >= 3 when
//     L * L <= lim2,  lim = (float(s) - 2.5f) * h,  lim2 = lim * lim,  and lim2 >= 1e-30
// (float(s) - 2.5f is exact): fl(L*L) >= L^2 (1 - eps) and lim2 <= ((s - 2.5) h)^2 (1 + eps)^3 give L <= (s - 2.5) h
// (1 + 2^-22), and with R_j <= h, by (A), a stopping j has |d| <= (s - 1.5) h (1 + 2^-19).  (s - 1.5)(1 + 2^-19) <
// s - 1.25 for s < 2^17, and s < dim <= 65536 under the margins' |min| + dim h <= 65536 h: no unseen atom stops a ray
// of any dot of i.  The cell between 1.5 and 2.5 is R_j - forgetting it passes every natural structure tried and loses rays
// on tests/enclosure_cases.py last_shell() -, the quarter cell between 1.25 and 1.5 pays for the roundings, as in
// crowding.hip; it did not have to be widened.  s >= 3 keeps lim positive; lim2 >= 1e-30 keeps the squares normal (an L
// whose square underflows is below 1e-19 and lim above 1e-15).  Without the margins, or when the rule is never met
// (L * L = +inf), the sweep ends when the shells cover the grid (ShCell::s_last), which is always exact.  For L = 10 and
// h = 3.28 the rule is met after shell 6.
//
// The prefilter, two cuts, both only under the margins (elsewhere R_j may be negative and R2_j is still its square) and
// both with the factor k = 1 + 2^-10 (exact in float32):
//   the lane cut    d2 <= cut2_j = fl(fl(fl(L + R_j) * k)^2), tested per (dot, obstacle) around the loop over m when
//                   cut2_j >= 1e-30; cut2_j is +inf otherwise (a NaN d2 still fails it, and stops nothing).  By (A) a
//                   stopping j has d2 <= |d|^2 (1 + eps)^3 <= (L + R_j)^2 (1 + 2^-18) and cut2_j >= (L + R_j)^2 k^2
//                   (1 - eps)^5 > (L + R_j)^2 (1 + 2^-10): no stopping pair is cut.
//   the staging cut |c_j - c_i|^2 (float32, the differences first) <= fl((fl(fl(fl(L + R_i) + R_j) * k) + h / 64)^2), used
//                   when that square is >= 1e-30 (a NaN square: not used).  c_j - c_i = (c_j - q) + (q - c_i): the first
//                   is d up to (1 + eps); a component of q - c_i is R_i s_k (1 + eps) plus the rounding of the sum, half
//                   an ulp of q, and |q| <= 65537 h has an ulp of h / 64 at most: |q - c_i| <= R_i (1 + 2^-20) + sqrt(3)
//                   h / 128.  So a stopping j has |c_j - c_i| <= (L + R_i + R_j)(1 + 2^-19) + 0.0136 h, the float32
//                   square of it at most (1 + 2^-21) times the exact one, and the bound's is at least ((L + R_i + R_j)
//                   (1 + 2^-10) + 0.0156 h)^2 (1 - eps)^8: no stopping atom is dropped.  The h / 64 is an ABSOLUTE term:
//                   with coordinates of 65536 h the relative slack alone would not cover the rounding of q.
//   A NaN c_i or c_j fails the staging cut, and by the definition stops nothing and is stopped by nothing.
//
// Resources (compiler's report): 101 VGPRs, 106 SGPRs (6 spilled to a VGPR's lanes), 11 264 bytes of LDS (4 x 1 KiB of run
// tables, 4 x 1 KiB of staged obstacles, 4 x 256 bytes of lane cuts, 4 x 512 bytes of point numbers), 4 waves per SIMD; no
// scratch.  The loop over m compiles to scalar loads from the kernel arguments and packed float32 multiplies and adds, two
// directions to an instruction, none fused.
// Measured (one MI355X, single runs): the proteome at 100 points, 30 directions and reach 10 in 644 ms, where
// k_dot_crowding with the one edge 10 takes 88.6 ms on the same input.  Both cuts were built together: there is no figure
// for either alone.
// Compiled with -ffp-contract=off: nothing is fused (the definition is the model's plain float32 arithmetic).
#include "shell_sweep.h"

namespace rsasa {
namespace {

constexpr uint32_t kDeDots = 2;                // dots a lane holds in one pass
constexpr uint32_t kDePass = kDeDots * kWave;  // dots of one pass
constexpr float kDeSlack = 1.0009765625f;      // 1 + 2^-10

__global__ __launch_bounds__(256) void k_dot_enclosure(DeArgs d)
{
    const PtArgs &a = d.p;
    const BatchView &b = a.b;
    __shared__ uint32_t s_excl[4][kShRuns], s_start[4][kShRuns];
    __shared__ float4 s_atom[4][kWave];    // (c_j, R2_j) of the staged obstacles
    __shared__ float s_cut[4][kWave];      // their lane cuts, squared
    __shared__ uint32_t s_pt[4][kDePass];  // the pass's accessible points, by rank
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= b.n_atoms) return;
    const uint32_t orig = b.sorted_orig[p];
    const uint32_t n_free = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.free[orig]);  // (the same in every lane)
    if (n_free == 0u) return;  // (the same in every lane)
    const unsigned long long first_row = d.dot_offsets[orig];
    const ShFrame fr = sh_frame(b, p);
    const float4 me = fr.me;
    const float R = me.w + b.probe;
    const uint32_t n_dirs = d.n_dirs;
    const float L = d.reach, LL = d.reach2;
    const float h = fr.g.cell_size;
    const float LR = L + R, h64 = h * 0.015625f;
    const bool own = (d.sorted_flags[p] & 1u) != 0u;  // (the same in every lane)
    const uint32_t *mw = a.masks + (size_t)orig * a.words;

    for (uint32_t lo = 0; lo < n_free; lo += kDePass) {
        const uint32_t n_pass = min(n_free - lo, kDePass);
        // ---- the points of ranks [lo, lo + n_pass) into s_pt: lanes over the mask's words, 64 at a time
        wave_lds_fence();  // (every lane is done with the previous pass's points)
        uint32_t before = 0;  // set bits of the words already walked
        for (uint32_t w0 = 0; w0 < a.words && before < lo + n_pass; w0 += kWave) {
            const uint32_t wi = w0 + lane;
            uint32_t word = wi < a.words ? mw[wi] : 0u;
            const uint32_t pc = (uint32_t)__popc(word);
            const uint32_t incl = wave_incl_scan(pc);
            uint32_t rank = before + incl - pc;
            if (rank + pc > lo && rank < lo + n_pass) {
                while (word) {
                    const uint32_t bit = (uint32_t)__ffs(word) - 1u;
                    word &= word - 1u;
                    if (rank >= lo && rank < lo + n_pass) s_pt[w][rank - lo] = wi * 32u + bit;
                    rank++;
                }
            }
            before += wave_bcast(incl, kWave - 1);
        }
        wave_lds_fence();
        // ---- lanes to dots, as in k_dot_crowding: P lanes and G groups for a pass of 32 dots or fewer, else two dots a lane
        uint32_t P = kWave;
        if (n_pass <= kWave / 2) {
            P = 1u;
            while (P < n_pass) P <<= 1;
        }
        const uint32_t lg = (uint32_t)__ffs(P) - 1u, G = kWave >> lg, g = lane >> lg, r0 = lane & (P - 1u);
        const bool two = n_pass > kWave;  // (the same in every lane)
        float qx[kDeDots], qy[kDeDots], qz[kDeDots];
        uint32_t blk[kDeDots];
#pragma unroll
        for (uint32_t t = 0; t < kDeDots; t++) {
            const uint32_t r = t ? kWave + lane : r0;
            const uint32_t pi = r < n_pass ? s_pt[w][r] : 0u;  // (a lane without a dot computes point 0's and writes nothing)
            const float sx = a.lx[pi], sy = a.ly[pi], sz = a.lz[pi];
            qx[t] = me.x + R * sx;
            qy[t] = me.y + R * sy;
            qz[t] = me.z + R * sz;
            // the own atom: ray m enters the sphere it starts on (every group sets the same bits)
            uint32_t bits = 0u;
            if (own) {
                for (uint32_t m = 0; m < n_dirs; m++) {
                    const DeDir u = d.dir[m];
                    bits |= (u.ux * sx + u.uy * sy + u.uz * sz < 0.0f ? 1u : 0u) << m;
                }
            }
            blk[t] = bits;
        }

        sh_sweep(
            b, fr, s_excl[w], s_start[w],
            [&](bool in, uint32_t q) {
                // ---- lanes over the atoms of the runs: the obstacles that can reach a dot of i are staged
                bool keep = in && q != p && (d.sorted_flags[q] & 1u) != 0u;
                float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                float cut2 = __builtin_inff();
                if (keep) {
                    o = b.sorted_xyzr[q];
                    const float Rj = o.w + b.probe;
                    if (fr.margins) {
                        const float ddx = o.x - me.x, ddy = o.y - me.y, ddz = o.z - me.z;
                        const float dd2 = ddx * ddx + ddy * ddy + ddz * ddz;
                        const float far = (LR + Rj) * kDeSlack + h64, far2 = far * far;
                        if (far2 >= 1e-30f) keep = dd2 <= far2;
                        const float near = (L + Rj) * kDeSlack, near2 = near * near;
                        if (near2 >= 1e-30f) cut2 = near2;
                    }
                    o.w = Rj * Rj;
                }
                const unsigned long long m64 = ballot64(keep);
                if (m64 == 0ull) return;  // (the same in every lane)
                const uint32_t n_staged = (uint32_t)__popcll(m64);
                const uint32_t slot = mbcnt64(m64);
                wave_lds_fence();  // (every lane is done with the previous atoms)
                if (keep) {
                    s_atom[w][slot] = o;
                    s_cut[w][slot] = cut2;
                }
                wave_lds_fence();
                // ---- lanes over their dots
                for (uint32_t k = g; k < n_staged; k += G) {
                    const float4 c = s_atom[w][k];  // (the same address in every lane of a group: G broadcasts)
                    const float c2 = s_cut[w][k];
#pragma unroll
                    for (uint32_t t = 0; t < kDeDots; t++) {
                        if (t == 0u || two) {
                            const float dx = c.x - qx[t], dy = c.y - qy[t], dz = c.z - qz[t];
                            const float d2 = dx * dx + dy * dy + dz * dz;
                            if (d2 <= c2) {
                                uint32_t bits = 0u;
                                for (uint32_t m = 0; m < n_dirs; m++) {
                                    const DeDir u = d.dir[m];  // (the same in every lane: a scalar load)
                                    const float tt = dx * u.ux + dy * u.uy + dz * u.uz;
                                    const float perp = d2 - tt * tt;
                                    const float ex = dx - u.lx, ey = dy - u.ly, ez = dz - u.lz;
                                    const float e2 = ex * ex + ey * ey + ez * ez;
                                    const float v = tt <= L ? perp : e2;
                                    bits |= (tt > 0.0f && v <= c.w ? 1u : 0u) << m;
                                }
                                blk[t] |= bits;
                            }
                        }
                    }
                }
            },
            [&](uint32_t s, bool) {
                if (fr.margins && s >= 3u) {
                    const float lim = ((float)s - 2.5f) * h;
                    const float lim2 = lim * lim;
                    if (LL <= lim2 && lim2 >= 1e-30f) return true;
                }
                return false;
            });

        // ---- the groups' words meet (every lane is here: the sweep ends for the whole wave at once), then the words of
        // the pass from the lanes of group 0
        for (uint32_t m = P; m < kWave; m <<= 1) blk[0] |= (uint32_t)__shfl_xor((int)blk[0], (int)m, kWave);
#pragma unroll
        for (uint32_t t = 0; t < kDeDots; t++) {
            const uint32_t r = t ? kWave + lane : r0;
            if (r < n_pass && (t ? two : g == 0u)) d.blocked[first_row + lo + r] = blk[t];
        }
    }
}

}  // namespace

// The word of every accessible dot from the masks of a finished point run, their popcounts (launch_mask_free), the scan
// of those (DeArgs::dot_offsets) and the flags in cell-sorted order (launch_sort_flags).
void launch_dot_enclosure(const DeArgs &d, hipStream_t stream)
{
    const uint32_t n = d.p.b.n_atoms;
    if (!n) return;
    hipLaunchKernelGGL(k_dot_enclosure, dim3(cdiv(n, 4)), dim3(256), 0, stream, d);
}

}  // namespace rsasa
