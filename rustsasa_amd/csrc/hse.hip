// Half-sphere exposure kernels (rsasa_half_sphere_exposure*, gfx950 only): for every centre the partners of its own
// structure within a cutoff several cells long, split by the side of the plane through the centre that is normal to the
// centre's direction.  They need the cell grid of a binned batch and nothing else: no neighbour lists, no lattice.
//
//   k_sort_flags    one thread per cell-sorted position: the atom's flag byte, gathered once through sorted_orig (3 where
//                   the caller gave no flags).  k_half_sphere then reads a partner's bit at the position it reads the
//                   partner's coordinates from.  Gathered in the sweep instead, the compile listing shows the byte load
//                   behind an s_waitcnt vmcnt(0) for the sorted_orig load in every trip of the inner loop - two memory
//                   latencies in a row where the copy issues its byte load and its coordinate load together -, at the same
//                   66 VGPRs, and a null `flags` is a branch there.
//   k_half_sphere   one wave per cell-sorted atom i, run by sh_sweep (shell_sweep.h: the driver and its contract); a wave
//                   whose atom is no centre writes 0 / 0 and returns.  Its `visit`: each lane with an atom reads
//                   sorted_xyzr[q] and the flag byte and evaluates the definition (include/rustsasa_amd.h) -
//                   dx = c_j.x - c_i.x; d2 = dx*dx + dy*dy + dz*dz; side = dx*u.x + dy*u.y + dz*u.z, float32, unfused, left
//                   to right; j counts iff q != p, bit 0, d2 <= c2 - and the wave adds the popcounts of the ballots of
//                   (counts, side >= 0) and (counts, !(side >= 0)).  Nothing but the sweep's run tables is in LDS: an atom is
//                   read by one lane, once, and used for ten operations, so a staged copy would be written and read back
//                   for nothing (k_atom_depth stages because every staged atom meets every point of the lattice).
//
// The reach.  Its `after` is sh_cutoff_reached: the sweep stops after shell s >= 1 once c2 <= ((s - 1/2) h)^2, or when the
// shells cover the grid: the rule, and the proof that no unseen atom can count, ties included, are in cutoff_sweep.h
// (within.hip sweeps by the same rule).
// Resources (compiler's report): k_half_sphere 66 VGPRs, 4 096 bytes of LDS, 7 waves per SIMD; no scratch.
// Compiled with -ffp-contract=off: d2 and side are not fused (the definition is the model's plain float32 arithmetic).
#include "cutoff_sweep.h"

namespace rsasa {
namespace {

__global__ __launch_bounds__(256) void k_sort_flags(HsArgs a)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.b.n_atoms) return;
    a.sorted_flags[p] = a.flags ? a.flags[a.b.sorted_orig[p]] : (uint8_t)3u;
}

__global__ __launch_bounds__(256) void k_half_sphere(HsArgs a)
{
    const BatchView &b = a.b;
    __shared__ uint32_t s_excl[4][kShRuns], s_start[4][kShRuns];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= b.n_atoms) return;
    const uint32_t orig = b.sorted_orig[p];
    if ((a.sorted_flags[p] & 2u) == 0u) {  // no centre (the same in every lane)
        if (lane == 0) {
            a.up[orig] = 0u;
            a.down[orig] = 0u;
        }
        return;
    }
    const ShFrame fr = sh_frame(b, p);
    const float4 me = fr.me;
    const bool has_dirs = a.dirs != nullptr;
    float ux = 0.0f, uy = 0.0f, uz = 0.0f;
    if (has_dirs) {
        ux = a.dirs[3u * (size_t)orig];
        uy = a.dirs[3u * (size_t)orig + 1u];
        uz = a.dirs[3u * (size_t)orig + 2u];
    }
    const float c2 = a.cutoff * a.cutoff;

    uint32_t up = 0, down = 0;
    sh_sweep(
        b, fr, s_excl[w], s_start[w],
        [&](bool in, uint32_t q) {
            bool counts = false, above = false;
            if (in) {
                const float4 o = b.sorted_xyzr[q];
                const uint32_t fl = a.sorted_flags[q];
                const float dx = o.x - me.x, dy = o.y - me.y, dz = o.z - me.z;
                const float d2 = dx * dx + dy * dy + dz * dz;
                const float side = has_dirs ? dx * ux + dy * uy + dz * uz : 0.0f;
                counts = q != p && (fl & 1u) != 0u && d2 <= c2;
                above = side >= 0.0f;
            }
            up += (uint32_t)__popcll(ballot64(counts && above));
            down += (uint32_t)__popcll(ballot64(counts && !above));
        },
        [&](uint32_t s, bool) { return sh_cutoff_reached(fr.margins, s, fr.g.cell_size, c2); });
    if (lane == 0) {
        a.up[orig] = up;
        a.down[orig] = down;
    }
}

}  // namespace

// sorted_flags[] of every atom (h.b, h.flags, h.sorted_flags: nothing else of `h` is read)
void launch_sort_flags(const HsArgs &h, hipStream_t stream)
{
    const uint32_t n = h.b.n_atoms;
    if (!n) return;
    hipLaunchKernelGGL(k_sort_flags, dim3(cdiv(n, 256)), dim3(256), 0, stream, h);
}

// sorted_flags[], then up[] and down[] of every atom, on the grid of a binned batch
void launch_half_sphere(const HsArgs &h, hipStream_t stream)
{
    const uint32_t n = h.b.n_atoms;
    if (!n) return;
    launch_sort_flags(h, stream);
    hipLaunchKernelGGL(k_half_sphere, dim3(cdiv(n, 4)), dim3(256), 0, stream, h);
}

}  // namespace rsasa
