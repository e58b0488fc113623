// Dot-crowding kernel (rsasa_dot_crowding*, gfx950 only): for every accessible dot the partner atoms of its own structure
// by distance bin, from the cell grid of a finished point run (the masks of k_accessible_points, still on the device,
// their popcounts free[] from k_mask_free, points.hip, and the exclusive scan of those, the dots' rows).
//
//   k_dot_crowding  one wave per cell-sorted atom i, four waves per workgroup, run by sh_sweep (shell_sweep.h: the driver
//                   and its contract); a wave whose atom has no accessible point leaves at once.  LANES OWN DOTS: the
//                   atom's mask is compacted (a popcount per word, a scan over the wave, the set bits' point numbers
//                   into LDS by rank), kDcPass = 128 dots to a pass, and a lane holds its dots as q = c_i + R_i * s_k
//                   with R_i = r_i + p - float32, unfused, the definition of include/rustsasa_amd.h.  A pass of more
//                   than 32 dots gives lane l the dots of rank l and 64 + l (the second one skipped, wave-uniformly, in a
//                   pass of 64 or fewer).  A pass of n <= 32 dots - nearly every atom at 100 points - would leave
//                   most lanes without a dot: it is spread over P lanes, P the power of two >= n, and the G = 64 / P
//                   groups of lanes hold the same dots and share the partners out (below).  An atom with more than 128
//                   dots is swept once per pass (at 100 points no atom is; a lone atom at 960 points takes eight).
//                   The sweep's `visit`: lanes go over the atoms of a step's runs, 64 at a time, and those with the
//                   partner bit (one byte at the cell-sorted position, k_sort_flags of hse.hip) are compacted into LDS
//                   as c_j; then group g goes over the staged atoms g, g + G, ... - one address per group, G
//                   broadcasts of 16 bytes in consecutive banks -, evaluates dx = c_j.x - q.x;
//                   d2 = dx*dx + dy*dy + dz*dz for each of its dots and adds (d2 <= e2[b]) to a CUMULATIVE counter per
//                   edge, in registers.  After the sweep the groups' counters are added up over the lanes that hold the
//                   same dot (log2 G shuffles per counter; integers: the order does not matter) and a lane of group 0
//                   writes its dots' rows as the differences of neighbouring counters: a NaN d2 passes no test and
//                   counts nowhere; of equal edges the first takes the pair (the later differences are 0).  The rows of
//                   atom i are [dot_offsets[i], dot_offsets[i + 1]) and the wave alone owns them: no atomics, and every
//                   row is written, the all-zero ones too (the buffer holds an earlier call's data).
//                   Two instantiations, NB = 4 and NB = 8 counters per dot (n_bins <= 4, n_bins <= 8); the host pads
//                   e2[n_bins .. 8) with the last edge, so the spare counters repeat the last one and are not written.
//
// The stop rule.  In a structure that passes sh_margins_hold an atom j not seen after shell s differs from i, along some
// axis, by D = |x_j - x_i| > (s - 1/8) h in exact arithmetic, h = StructGrid::cell_size (shell_sweep.h, "What an unseen
// atom implies").  A dot of i is q = c_i + R_i * s_k with 0 <= R_i <= h and |s_k.x| <= 1: along that axis it lies within
// h of c_i, up to the roundings of the product and the sum, and dx = x_j - q.x carries one more - each at most h / 128
// under the margins, a handful of them, far below the h / 8 set aside.  So |dx| > (s - 1.25) h, and the float32 d2 is no
// smaller than the float32 square of dx (the other terms are not negative and rounding is monotone, as in
// cutoff_sweep.h): d2 > ((s - 1.25) h)^2 (1 - 2^-24)^3 as long as the square does not underflow.  The sweep stops after
// shell s >= 2 when
//     e2[n_bins - 1] <= lim2,  lim = (float(s) - 1.5f) * h,  lim2 = lim * lim,  and lim2 >= 1e-30
// (float(s) - 1.5f is exact; two roundings): lim2 <= ((s - 1.5) h)^2 (1 + 2^-24)^3, and ((s - 1.25) / (s - 1.5))^2 >
// 1 + 1 / (2 s) > 1 + 2^-19 for s < 2^18, far above the six roundings' 1 + 2^-21: every unseen d2 is strictly above
// lim2 >= e2[n_bins - 1], so no unseen atom counts for any dot of i, and one that ties with the last edge has been seen.
// The quarter cell between 1.25 and 1.5 pays for the roundings, as in depth.hip; s >= 2 keeps lim positive (at s = 1 the
// square of -h / 2 would pass for a bound); lim2 >= 1e-30 keeps the squares in the normal range.  Without the margins,
// or when the rule is never met (e2 = +inf), the sweep ends when the shells cover the grid (ShCell::s_last), which is
// always exact.  For edges up to 10 and h = 3.28 the rule is met after shell 5.
// No prefilter on |c_j - c_i| was built: every staged partner is tested against every dot of the pass.
// Resources (compiler's report): k_dot_crowding<4> 105 VGPRs, k_dot_crowding<8> 124 VGPRs, each 10 240 bytes of LDS (4 x 1
// KiB of run tables, 4 x 1 KiB of staged atoms, 4 x 512 bytes of point numbers), 4 waves per SIMD; no scratch.
// Measured: the proteome at edges 6 / 8 / 10 in 88.6 ms; with every lane holding a dot of its own and no
// groups - the first build - 247.9 ms.
// Compiled with -ffp-contract=off: q and d2 are not fused (the definition is the model's plain float32 arithmetic).
#include "shell_sweep.h"

namespace rsasa {
namespace {

constexpr uint32_t kDcDots = 2;                // dots a lane holds in one pass
constexpr uint32_t kDcPass = kDcDots * kWave;  // dots of one pass

template <uint32_t NB>
__global__ __launch_bounds__(256) void k_dot_crowding(DcArgs d)
{
    const PtArgs &a = d.p;
    const BatchView &b = a.b;
    __shared__ uint32_t s_excl[4][kShRuns], s_start[4][kShRuns];
    __shared__ float4 s_atom[4][kWave];    // c_j of the staged partners
    __shared__ uint32_t s_pt[4][kDcPass];  // the pass's accessible points, by rank
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
    const uint32_t n_bins = d.n_bins;
    const float c2 = d.e2[n_bins - 1u];
    float e2[NB];
#pragma unroll
    for (uint32_t k = 0; k < NB; k++) e2[k] = d.e2[k];
    const uint32_t *mw = a.masks + (size_t)orig * a.words;

    for (uint32_t lo = 0; lo < n_free; lo += kDcPass) {
        const uint32_t n_pass = min(n_free - lo, kDcPass);
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
        // ---- lanes to dots: a pass of 32 dots or fewer is spread over P = the power of two >= n_pass lanes, and the
        // 64 / P groups of lanes take the staged atoms in turn (group g the atoms g, g + G, ...); a larger pass gives
        // lane l the dots l and 64 + l, and every lane takes every staged atom
        uint32_t P = kWave;
        if (n_pass <= kWave / 2) {
            P = 1u;
            while (P < n_pass) P <<= 1;
        }
        const uint32_t lg = (uint32_t)__ffs(P) - 1u, G = kWave >> lg, g = lane >> lg, r0 = lane & (P - 1u);
        const bool two = n_pass > kWave;  // (the same in every lane)
        float qx[kDcDots], qy[kDcDots], qz[kDcDots];
        uint32_t cnt[kDcDots][NB];
#pragma unroll
        for (uint32_t t = 0; t < kDcDots; t++) {
            const uint32_t r = t ? kWave + lane : r0;
            const uint32_t pi = r < n_pass ? s_pt[w][r] : 0u;  // (a lane without a dot computes point 0's and writes nothing)
            qx[t] = me.x + R * a.lx[pi];
            qy[t] = me.y + R * a.ly[pi];
            qz[t] = me.z + R * a.lz[pi];
#pragma unroll
            for (uint32_t k = 0; k < NB; k++) cnt[t][k] = 0u;
        }

        sh_sweep(
            b, fr, s_excl[w], s_start[w],
            [&](bool in, uint32_t q) {
                // ---- lanes over the atoms of the runs: the partners are staged
                const bool keep = in && (d.sorted_flags[q] & 1u) != 0u;
                const unsigned long long m = ballot64(keep);
                if (m == 0ull) return;  // (the same in every lane)
                const uint32_t n_staged = (uint32_t)__popcll(m);
                const uint32_t slot = mbcnt64(m);
                wave_lds_fence();  // (every lane is done with the previous atoms)
                if (keep) s_atom[w][slot] = b.sorted_xyzr[q];
                wave_lds_fence();
                // ---- lanes over their dots
                for (uint32_t k = g; k < n_staged; k += G) {
                    const float4 o = s_atom[w][k];  // (the same address in every lane of a group: G broadcasts)
#pragma unroll
                    for (uint32_t t = 0; t < kDcDots; t++) {
                        if (t == 0u || two) {
                            const float dx = o.x - qx[t], dy = o.y - qy[t], dz = o.z - qz[t];
                            const float d2 = dx * dx + dy * dy + dz * dz;
#pragma unroll
                            for (uint32_t e = 0; e < NB; e++) cnt[t][e] += d2 <= e2[e] ? 1u : 0u;
                        }
                    }
                }
            },
            [&](uint32_t s, bool) {
                if (fr.margins && s >= 2u) {
                    const float lim = ((float)s - 1.5f) * fr.g.cell_size;
                    const float lim2 = lim * lim;
                    if (c2 <= lim2 && lim2 >= 1e-30f) return true;
                }
                return false;
            });

        // ---- the groups' counters meet (every lane is here: the sweep ends for the whole wave at once), then the rows
        // of the pass: the cumulative counters of the lanes of group 0, differenced
        for (uint32_t m = P; m < kWave; m <<= 1) {
#pragma unroll
            for (uint32_t k = 0; k < NB; k++) cnt[0][k] += (uint32_t)__shfl_xor((int)cnt[0][k], (int)m, kWave);
        }
#pragma unroll
        for (uint32_t t = 0; t < kDcDots; t++) {
            const uint32_t r = t ? kWave + lane : r0;
            if (r < n_pass && (t ? two : g == 0u)) {
                uint32_t *row = d.counts + (size_t)(first_row + lo + r) * n_bins;
#pragma unroll
                for (uint32_t k = 0; k < NB; k++)
                    if (k < n_bins) row[k] = k ? cnt[t][k] - cnt[t][k - 1u] : cnt[t][0];
            }
        }
    }
}

}  // namespace

// The row of every accessible dot from the masks of a finished point run, their popcounts (launch_mask_free), the scan
// of those (DcArgs::dot_offsets) and the flags in cell-sorted order (launch_sort_flags).
void launch_dot_crowding(const DcArgs &d, hipStream_t stream)
{
    const uint32_t n = d.p.b.n_atoms;
    if (!n) return;
    if (d.n_bins <= 4u) hipLaunchKernelGGL(k_dot_crowding<4>, dim3(cdiv(n, 4)), dim3(256), 0, stream, d);
    else hipLaunchKernelGGL(k_dot_crowding<8>, dim3(cdiv(n, 4)), dim3(256), 0, stream, d);
}

}  // namespace rsasa
