// Dot-fields kernel (rsasa_dot_fields*, gfx950 only): for every accessible dot and up to four channels the sum, over the
// partner atoms of its own structure within a cutoff, of a per-atom weight times a distance kernel - the electrostatic or
// lipophilic potential at the dot, or a plain sum of a property - as a 64-bit fixed-point integer with 24 fraction bits.
// It starts from what k_dot_crowding starts from: the cell grid of a finished point run, the masks of
// k_accessible_points, their popcounts free[] and the scan of those.
//
//   k_dot_fields  k_dot_crowding's frame (crowding.hip) unchanged, run by sh_sweep (shell_sweep.h): one wave per
//                 cell-sorted atom i, four waves per workgroup; the atom's mask compacted into s_pt, kFdPass = 128 dots to
//                 a pass, two dots per lane; a pass of n <= 32 dots spread over P lanes, P the power of two >= n, the
//                 G = 64 / P groups of lanes holding the same dots and sharing the staged partners out.  The dots are
//                 q = c_i + R_i * s_k with R_i = r_i + p - float32, unfused, the definition of include/rustsasa_amd.h.
//                 What is new.  At staging a partner's weight row is fetched through sorted_orig[q] (the weights are in
//                 input order) and put into LDS beside its c_j: one float4 per staged atom, the channels the call does
//                 not have as 0.  Per (dot, partner) pair dx = c_j.x - q.x; d2 = dx*dx + dy*dy + dz*dz and the hit test
//                 d2 <= c2 come first; behind it only the factors g that some channel's kind needs are computed -
//                 `need`, a bit per kind, is a kernel argument and the same in every lane, and channels of one kind
//                 share the factor -: d = sqrtf(d2), 1.0f / d, 1.0f / d2, 1.0f / (1.0f + d), correctly rounded
//                 (v_div_scale / v_div_fmas / v_div_fixup and the refined square root: the build flags give nothing
//                 faster).  Then per channel one multiply t = w * g, one guarded conversion - |t| <= 2^24, which a NaN
//                 fails; t * 2^24 is exact and v_rndne_f32 rounds it to nearest even - and one 64-bit UNSIGNED add, so
//                 that the wrap is defined.  The accumulators stay in registers, 2 dots x NC channels x 2 VGPRs.  After
//                 the sweep the groups' partial sums meet by __shfl_xor on both halves (integers: the order does not
//                 matter) and the lanes of group 0 write their rows.  The rows of atom i are [dot_offsets[i],
//                 dot_offsets[i + 1]) and the wave alone owns them: no atomics, and every row is written, the all-zero
//                 ones too (the buffer holds an earlier call's data).
//                 Three instantiations, NC = 1, 2 and 4 accumulators per dot (three channels run as four, the fourth
//                 with weight 0 and never written).
//
// The stop rule is k_dot_crowding's with c2 = cutoff * cutoff in place of the last squared edge: after shell s >= 2 when
//     c2 <= lim2,  lim = (float(s) - 1.5f) * h,  lim2 = lim * lim,  and lim2 >= 1e-30.
// The proof in crowding.hip ("The stop rule") carries over word for word - it speaks of the dots of i, of d2 and of the
// largest squared radius that counts, and nothing else of this kernel enters it: every unseen d2 is strictly above
// lim2 >= c2, so no unseen atom passes the hit test for any dot of i, and one that ties with the cutoff has been seen.
// Resources (compiler's report): k_dot_fields<1> 89 VGPRs, k_dot_fields<2> 95 VGPRs (5 waves per SIMD each),
// k_dot_fields<4> 105 VGPRs (4 waves per SIMD) - the instantiation by channel count buys the one- and two-channel calls
// a wave -, each 14 336 bytes of LDS (4 x 1 KiB of run tables, 4 x 1 KiB of staged atoms, 4 x 1 KiB of staged weight
// rows, 4 x 512 bytes of point numbers); no scratch.
// Measured: DESIGN 5r.
// Compiled with -ffp-contract=off: q, d2, 1.0f + d and w * g are not fused (the definition is the model's plain float32).
#include "shell_sweep.h"

namespace rsasa {
namespace {

constexpr uint32_t kFdDots = 2;                // dots a lane holds in one pass
constexpr uint32_t kFdPass = kFdDots * kWave;  // dots of one pass

template <uint32_t NC>
__global__ __launch_bounds__(256) void k_dot_fields(FdArgs d)
{
    const PtArgs &a = d.p;
    const BatchView &b = a.b;
    __shared__ uint32_t s_excl[4][kShRuns], s_start[4][kShRuns];
    __shared__ float4 s_atom[4][kWave];    // c_j of the staged partners
    __shared__ float4 s_wt[4][kWave];      // their weight rows, channels [n_channels .. 4) as 0
    __shared__ uint32_t s_pt[4][kFdPass];  // the pass's accessible points, by rank
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
    const uint32_t n_ch = d.n_channels, need = d.need;  // (kernel arguments: the same in every lane)
    const float c2 = d.c2;
    uint32_t kind[NC];
#pragma unroll
    for (uint32_t c = 0; c < NC; c++) kind[c] = d.kinds[c];
    const uint32_t *mw = a.masks + (size_t)orig * a.words;

    for (uint32_t lo = 0; lo < n_free; lo += kFdPass) {
        const uint32_t n_pass = min(n_free - lo, kFdPass);
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
        // ---- lanes to dots, as in k_dot_crowding: P lanes and G groups for a pass of 32 dots or fewer, else two dots a
        // lane and every lane takes every staged atom
        uint32_t P = kWave;
        if (n_pass <= kWave / 2) {
            P = 1u;
            while (P < n_pass) P <<= 1;
        }
        const uint32_t lg = (uint32_t)__ffs(P) - 1u, G = kWave >> lg, g = lane >> lg, r0 = lane & (P - 1u);
        const bool two = n_pass > kWave;  // (the same in every lane)
        float qx[kFdDots], qy[kFdDots], qz[kFdDots];
        unsigned long long sum[kFdDots][NC];
#pragma unroll
        for (uint32_t t = 0; t < kFdDots; t++) {
            const uint32_t r = t ? kWave + lane : r0;
            const uint32_t pi = r < n_pass ? s_pt[w][r] : 0u;  // (a lane without a dot computes point 0's and writes nothing)
            qx[t] = me.x + R * a.lx[pi];
            qy[t] = me.y + R * a.ly[pi];
            qz[t] = me.z + R * a.lz[pi];
#pragma unroll
            for (uint32_t c = 0; c < NC; c++) sum[t][c] = 0ull;
        }

        sh_sweep(
            b, fr, s_excl[w], s_start[w],
            [&](bool in, uint32_t q) {
                // ---- lanes over the atoms of the runs: the partners are staged, each with its weight row
                const bool keep = in && (d.sorted_flags[q] & 1u) != 0u;
                const unsigned long long m = ballot64(keep);
                if (m == 0ull) return;  // (the same in every lane)
                const uint32_t n_staged = (uint32_t)__popcll(m);
                const uint32_t slot = mbcnt64(m);
                wave_lds_fence();  // (every lane is done with the previous atoms)
                if (keep) {
                    s_atom[w][slot] = b.sorted_xyzr[q];
                    const float *row = d.weights + (size_t)b.sorted_orig[q] * n_ch;
                    float4 wt = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (n_ch == 4u) wt = *(const float4 *)row;  // (rows of 16 bytes in a buffer of the allocator's alignment)
                    else {
                        wt.x = row[0];
                        if (n_ch >= 2u) wt.y = row[1];
                        if (n_ch >= 3u) wt.z = row[2];
                    }
                    s_wt[w][slot] = wt;
                }
                wave_lds_fence();
                // ---- lanes over their dots
                for (uint32_t k = g; k < n_staged; k += G) {
                    const float4 o = s_atom[w][k];  // (the same address in every lane of a group: G broadcasts)
                    const float4 wt = s_wt[w][k];
                    const float wc[4] = {wt.x, wt.y, wt.z, wt.w};
#pragma unroll
                    for (uint32_t t = 0; t < kFdDots; t++) {
                        if (t == 0u || two) {
                            const float dx = o.x - qx[t], dy = o.y - qy[t], dz = o.z - qz[t];
                            const float d2 = dx * dx + dy * dy + dz * dz;
                            if (d2 <= c2) {  // (a NaN d2 fails)
                                float dd = 0.0f, g1 = 0.0f, g2 = 0.0f, g3 = 0.0f;
                                if (need & 0xAu) dd = sqrtf(d2);
                                if (need & 0x2u) g1 = 1.0f / dd;
                                if (need & 0x4u) g2 = 1.0f / d2;
                                if (need & 0x8u) g3 = 1.0f / (1.0f + dd);
#pragma unroll
                                for (uint32_t c = 0; c < NC; c++) {
                                    const float gk = kind[c] == 0u ? 1.0f : kind[c] == 1u ? g1 : kind[c] == 2u ? g2 : g3;
                                    const float term = wc[c] * gk;
                                    if (fabsf(term) <= 0x1p24f)  // (a NaN fails; term * 2^24 is exact)
                                        sum[t][c] += (unsigned long long)__float2ll_rn(term * 0x1p24f);
                                }
                            }
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

        // ---- the groups' sums meet (every lane is here: the sweep ends for the whole wave at once), then the rows of the
        // pass from the lanes of group 0
        for (uint32_t m = P; m < kWave; m <<= 1) {
#pragma unroll
            for (uint32_t c = 0; c < NC; c++) {
                const uint32_t lo32 = (uint32_t)__shfl_xor((int)(uint32_t)sum[0][c], (int)m, kWave);
                const uint32_t hi32 = (uint32_t)__shfl_xor((int)(uint32_t)(sum[0][c] >> 32), (int)m, kWave);
                sum[0][c] += ((unsigned long long)hi32 << 32) | lo32;
            }
        }
#pragma unroll
        for (uint32_t t = 0; t < kFdDots; t++) {
            const uint32_t r = t ? kWave + lane : r0;
            if (r < n_pass && (t ? two : g == 0u)) {
                long long *row = d.sums + (size_t)(first_row + lo + r) * n_ch;
#pragma unroll
                for (uint32_t c = 0; c < NC; c++)
                    if (c < n_ch) row[c] = (long long)sum[t][c];
            }
        }
    }
}

}  // namespace

// The row of every accessible dot from the masks of a finished point run, their popcounts (launch_mask_free), the scan
// of those (FdArgs::dot_offsets), the flags in cell-sorted order (launch_sort_flags) and the weights in input order.
void launch_dot_fields(const FdArgs &d, hipStream_t stream)
{
    const uint32_t n = d.p.b.n_atoms;
    if (!n) return;
    if (d.n_channels == 1u) hipLaunchKernelGGL(k_dot_fields<1>, dim3(cdiv(n, 4)), dim3(256), 0, stream, d);
    else if (d.n_channels == 2u) hipLaunchKernelGGL(k_dot_fields<2>, dim3(cdiv(n, 4)), dim3(256), 0, stream, d);
    else hipLaunchKernelGGL(k_dot_fields<4>, dim3(cdiv(n, 4)), dim3(256), 0, stream, d);
}

}  // namespace rsasa
