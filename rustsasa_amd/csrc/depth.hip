// Atom-depth kernel (rsasa_atom_depth*, gfx950 only): for every atom the nearest accessible dot of its own structure,
// from the cell grid of a finished point run (the masks of k_accessible_points, still on the device, and their popcounts
// free[] from k_mask_free, points.hip).
//
//   k_atom_depth    one wave per cell-sorted atom i, over the shell sweep of shell_sweep.h.  Lanes go first over the atoms
//                   of a step's runs, 64 at a time, and read free[] (4 bytes): the atoms with free != 0 are compacted into
//                   LDS as (c_j, R_j) and (row, j).  Then lanes go over the points in chunks of 64: per chunk the two mask
//                   words of every staged atom are fetched to LDS at once, and every lane with its bit set evaluates the
//                   definition (include/rustsasa_amd.h) - R = r + p; q = c_j + R * s_k; d = c_i - q;
//                   d2 = dx*dx + dy*dy + dz*dz, float32, unfused, left to right - and keeps the smallest key
//                   (bits(d2) << 32) | j of those whose d2 is no NaN.  After every shell the lanes' minima are reduced
//                   over the wave.
//
// The stop rule.  In a structure that passes sh_margins_hold an atom j not seen after shell s differs from i by more than
// (s - 1/8) h along some axis, h = StructGrid::cell_size (shell_sweep.h, "What an unseen atom implies").  Every dot of j
// lies within R_j <= h of c_j, and q and d carry a few roundings of at most h / 128 each, so the float32 d2 of any dot of
// an unseen atom is above ((s - 1.25) h)^2.  The sweep stops after shell s when best_d2 <= ((s - 2) h)^2 (one float32
// product and square: rounding far below the 0.75 h between the two bounds): every unseen key is strictly larger than the
// one held, ties included.  Without the margins the sweep ends when the shells cover the grid, which is always exact.
// No per-candidate bound (|c_i - c_j| - R_j) and no per-cell summary of the dots were built: see DESIGN 5g.
// The kernel takes its atom from sh_frame and writes the loops of sh_sweep (shell_sweep.h: the driver and its contract)
// out, and must follow a change there by hand: run by the driver it measured 3.6 to 4.7 % slower at the same registers
// (profiles/sweep_driver_ab.txt).
// Resources (compiler's report): k_atom_depth 79 VGPRs, 12 288 bytes of LDS, 6 waves per SIMD; no scratch.
// Compiled with -ffp-contract=off: q and d2 are not fused (the definition is the model's plain float32 arithmetic).
#include "shell_sweep.h"

namespace rsasa {
namespace {

__device__ __forceinline__ unsigned long long dp_wave_min(unsigned long long v)
{
#pragma unroll
    for (int h = kWave / 2; h >= 1; h >>= 1) {
        const unsigned long long o = __shfl_xor(v, h, kWave);
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_atom_depth(DpArgs d)
{
    const PtArgs &a = d.p;
    const BatchView &b = a.b;
    __shared__ uint32_t s_excl[4][kShRuns], s_start[4][kShRuns];
    __shared__ float4 s_atom[4][kWave];  // (c_j, R_j) of the staged atoms
    __shared__ uint2 s_who[4][kWave];    // (input row, index within the structure)
    __shared__ uint2 s_bits[4][kWave];   // their mask words of the current chunk
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= b.n_atoms) return;
    const ShFrame fr = sh_frame(b, p);
    const float4 me = fr.me;
    const uint32_t n_chunks = (a.n_points + kWave - 1) / kWave;

    unsigned long long best = ~0ull;  // this lane's smallest key; after a shell, the wave's
    for (uint32_t s = 0;; s++) {
        const ShShell shell = sh_shell(fr.g, fr.cell, s);
        for (unsigned long long r0 = 0; r0 < shell.n_rows; r0 += kWave) {
            const uint32_t total = sh_step_runs(b, fr.g, fr.cell, shell, s, r0, s_excl[w], s_start[w]);
            for (uint32_t f0 = 0; f0 < total; f0 += kWave) {
                // ---- lanes over the atoms of the runs: those with accessible points are staged
                const uint32_t f = f0 + lane;
                bool keep = false;
                uint32_t q = 0, orig = 0;
                if (f < total) {
                    q = sh_pos(s_excl[w], s_start[w], f);
                    orig = b.sorted_orig[q];
                    keep = d.free[orig] != 0u;
                }
                const uint32_t n_staged = sh_stage(b, keep, q, make_uint2(orig, orig - fr.g.atom_begin), s_atom[w], s_who[w]);
                if (n_staged == 0u) continue;  // (the same in every lane)
                // ---- lanes over the points, 64 at a time
                for (uint32_t c = 0; c < n_chunks; c++) {
                    const uint32_t pi = c * kWave + lane;
                    const float sx = a.lx[pi], sy = a.ly[pi], sz = a.lz[pi];  // (zero padded to whole chunks)
                    if (c) wave_lds_fence();  // (every lane is done with the previous chunk's words)
                    if (lane < n_staged) {
                        const uint32_t *mw = a.masks + (size_t)s_who[w][lane].x * a.words;
                        const uint32_t w0 = 2u * c, w1 = 2u * c + 1u;
                        s_bits[w][lane] = make_uint2(w0 < a.words ? mw[w0] : 0u, w1 < a.words ? mw[w1] : 0u);
                    }
                    wave_lds_fence();
                    const bool live = pi < a.n_points;
                    for (uint32_t k = 0; k < n_staged; k++) {
                        const uint2 bits = s_bits[w][k];  // (the same address in every lane: a broadcast)
                        if ((bits.x | bits.y) == 0u) continue;
                        const uint32_t word = lane < 32u ? bits.x : bits.y;
                        if (live && ((word >> (lane & 31u)) & 1u)) {
                            const float4 o = s_atom[w][k];
                            const float qx = o.x + o.w * sx, qy = o.y + o.w * sy, qz = o.z + o.w * sz;
                            const float dx = me.x - qx, dy = me.y - qy, dz = me.z - qz;
                            const float d2 = dx * dx + dy * dy + dz * dz;
                            const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | s_who[w][k].y;
                            if (d2 == d2 && key < best) best = key;
                        }
                    }
                }
            }
        }
        best = dp_wave_min(best);
        if (s >= fr.cell.s_last) break;  // the shells cover the grid
        if (fr.margins && s >= 2u && best != ~0ull) {
            const float lim = (float)(s - 2u) * fr.g.cell_size;
            if (__uint_as_float((uint32_t)(best >> 32)) <= lim * lim) break;
        }
    }
    if (lane == 0) d.keys[b.sorted_orig[p]] = best;
}

}  // namespace

// keys[] of every atom from the masks of a finished point run and their popcounts free[] (launch_mask_free)
void launch_atom_depth(const DpArgs &d, hipStream_t stream)
{
    const uint32_t n = d.p.b.n_atoms;
    if (!n) return;
    hipLaunchKernelGGL(k_atom_depth, dim3(cdiv(n, 4)), dim3(256), 0, stream, d);
}

}  // namespace rsasa
