// Radial count kernels (rsasa_radial_counts*, gfx950 only): for every centre the partners of its own structure by class
// and distance bin, and per structure the sums of those rows by the centre's class.  Like hse.hip they need the cell grid
// of a binned batch and nothing else.
//
//   k_sort_kinds     one thread per cell-sorted position: (class << 2) | (flags & 3), gathered once through sorted_orig
//                    (flags 3 where the caller gave none, class 0 where the caller gave none), into the buffer
//                    k_sort_flags fills for the other sweeps.  k_radial_counts then reads one byte per partner at the
//                    position it reads the coordinates from (hse.hip says what the gather costs inside the sweep).
//   k_radial_counts  one wave per cell-sorted atom i, four waves per workgroup, run by sh_sweep (shell_sweep.h: the driver
//                    and its contract); a wave whose atom is no centre writes a zero row and returns before the sweep.
//                    Its `visit`: each lane with an atom reads sorted_xyzr[q] and the kind byte and evaluates the
//                    definition (include/rustsasa_amd.h) - dx = c_j.x - c_i.x; d2 = dx*dx + dy*dy + dz*dz, float32,
//                    unfused, left to right; j counts iff q != p, bit 0, d2 <= e2[n_bins - 1] -, finds the smallest k
//                    with d2 <= e2[k] and adds 1 to cell class * n_bins + k of the wave's histogram in LDS.  Integer
//                    LDS atomics: the row does not depend on the order of the adds, and 64 lanes adding to one cell in
//                    one instruction (a crowded cell of one class in one bin) are serialised by the LDS, not lost.
//                    After the sweep the lanes stride the row and write it to the table (coalesced, input order).
//   k_radial_pairs   only when the pair tables are asked for: the exact uint64 sums of the table's rows by (structure,
//                    class of the centre).  A workgroup takes kRdChunk consecutive atoms of the input order - which is
//                    the structures' order - and ONE class of the centre (blockIdx.y): it walks the structures its atoms
//                    span, and within one structure thread (sub, c) adds cell c of the rows of its sub-group's atoms
//                    of that class into a 64-bit register (a cell is below 2^31 and a structure's cell can pass
//                    2^32, so nothing narrower would do); at the structure's end the sub-groups meet in 64-bit LDS
//                    cells and the first n_classes * n_bins threads issue one global 64-bit add each - at most one per
//                    (workgroup, structure, cell), none where the sum is zero.  Every row is read by exactly one
//                    workgroup (the one of its class).  No float anywhere.  The host zeroes the tables on the stream.
//
// The bin.  A branch-free binary search over the wave's LDS copy of the squared edges, padded with +inf to the power of
// two P >= n_bins: log2(P) dependent ds_read_b32, each with one compare and one select - none at one bin, 2 at four
// bins, 5 at 32.  Acceptance (d2 <= e2[n_bins - 1]) has already bounded the answer by P - 1, so no last step is needed;
// equal edges: `e2[k] < d2` moves right only past edges strictly below d2, so the first of several equal edges takes the
// pair.  The alternative - counting the k with e2[k] < d2 against uniform values - is n_bins - 1 LDS reads (or scalar
// loads, each with its own wait in the inner loop) and as many compare-and-add pairs per atom: the same at four bins,
// six times the instructions at 32; it was not kept.  The search stands in the listing as a loop of a uniform trip count
// inside the lanes that count.
//
// The reach.  Its `after` is sh_cutoff_reached with c2 = e2[n_bins - 1]: acceptance is d2 <= c2, and the bin only
// partitions what was accepted (cutoff_sweep.h).
// Resources (compiler's report): k_radial_counts 72 VGPRs, 12 800 bytes of LDS (4 x 1 KiB of run tables, 4 x 2 KiB of
// histogram, 4 x 128 bytes of edges), 7 waves per SIMD; no scratch.  The 7 is asked for (amdgpu_waves_per_eu): left to
// itself the compiler takes 80 VGPRs, 6 waves per SIMD, no scratch either, and on the proteome at one class and one bin
// that build ran 43.1 ms where this one runs 39.4 ms and k_half_sphere (66 VGPRs, 7 waves) 37.7 ms.  k_radial_pairs 18
// VGPRs, 4 096 bytes of LDS, 8 waves per SIMD; k_sort_kinds 6 VGPRs; no scratch.
// Compiled with -ffp-contract=off: d2 is not fused (the definition is the model's plain float32 arithmetic).
#include "cutoff_sweep.h"
#include "entry_checks.h"

namespace rsasa {
namespace {

constexpr uint32_t kRdCells = kRadialMaxClasses * kRadialMaxBins;  // the widest row: 512 cells, 2 KiB per wave
constexpr uint32_t kRdChunk = 1024;                                // atoms of one k_radial_pairs workgroup
constexpr uint32_t kRdThreads = 256;
static_assert(kRdCells <= 2u * kRdThreads, "a thread of k_radial_pairs holds at most two cells of a row");

__global__ __launch_bounds__(256) void k_sort_kinds(RdArgs a)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.b.n_atoms) return;
    const uint32_t orig = a.b.sorted_orig[p];
    const uint32_t fl = a.flags ? (uint32_t)a.flags[orig] & 3u : 3u;
    const uint32_t cls = a.classes ? (uint32_t)a.classes[orig] : 0u;
    a.sorted_kinds[p] = (uint8_t)((cls << 2) | fl);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 7))) void k_radial_counts(RdArgs a)
{
    const BatchView &b = a.b;
    __shared__ uint32_t s_excl[4][kShRuns], s_start[4][kShRuns];
    __shared__ uint32_t s_hist[4][kRdCells];
    __shared__ float s_e2[4][kRadialMaxBins];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= b.n_atoms) return;
    const uint32_t orig = b.sorted_orig[p];
    const uint32_t n_bins = a.n_bins, cells = a.n_classes * n_bins;  // cells <= kRdCells (check_radial)
    uint32_t *row = a.table + (size_t)orig * cells;
    if ((a.sorted_kinds[p] & 2u) == 0u) {  // no centre (the same in every lane)
        for (uint32_t c = lane; c < cells; c += kWave) row[c] = 0u;
        return;
    }
    uint32_t *hist = s_hist[w];
    float *e2 = s_e2[w];
    for (uint32_t c = lane; c < cells; c += kWave) hist[c] = 0u;
    if (lane < kRadialMaxBins) e2[lane] = lane < n_bins ? a.e2[lane] : __builtin_inff();
    wave_lds_fence();
    const ShFrame fr = sh_frame(b, p);
    const float4 me = fr.me;
    const float c2 = a.e2[n_bins - 1u];
    uint32_t half = 1u;  // the power of two P >= n_bins, halved: the search's first step
    while (2u * half < n_bins) half <<= 1;
    if (n_bins == 1u) half = 0u;

    sh_sweep(
        b, fr, s_excl[w], s_start[w],
        [&](bool in, uint32_t q) {
            if (in) {
                const float4 o = b.sorted_xyzr[q];
                const uint32_t kind = a.sorted_kinds[q];
                const float dx = o.x - me.x, dy = o.y - me.y, dz = o.z - me.z;
                const float d2 = dx * dx + dy * dy + dz * dz;
                if (q != p && (kind & 1u) != 0u && d2 <= c2) {
                    uint32_t k = 0u;
                    for (uint32_t step = half; step > 0u; step >>= 1)
                        if (e2[k + step - 1u] < d2) k += step;
                    __hip_atomic_fetch_add(&hist[(kind >> 2) * n_bins + k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        },
        [&](uint32_t s, bool) { return sh_cutoff_reached(fr.margins, s, fr.g.cell_size, c2); });
    wave_lds_fence();  // (every lane's adds are in the histogram)
    for (uint32_t c = lane; c < cells; c += kWave) row[c] = hist[c];
}

// The structure that holds atom i: the s with so[s] <= i < so[s + 1] (so: [n_structures + 1], non-decreasing from 0;
// i < so[n_structures]).
__device__ __forceinline__ uint32_t rd_structure_of(const uint32_t *so, uint32_t n_structures, uint32_t i)
{
    uint32_t lo = 0u, hi = n_structures;  // so[lo] <= i < so[hi] throughout
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (so[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kRdThreads) void k_radial_pairs(RdArgs a)
{
    __shared__ unsigned long long s_acc[kRdCells];
    const uint32_t t = threadIdx.x;
    const uint32_t cells = a.n_classes * a.n_bins;
    const uint32_t cls = blockIdx.y;  // the class of the centres this workgroup sums
    const uint32_t n = a.b.n_atoms;
    const uint32_t i0 = blockIdx.x * kRdChunk, i1 = min(i0 + kRdChunk, n);
    // threads as (sub, c): c a cell of the row, sub-groups take the atoms in turn; a row of more than 256 cells gives
    // every thread a second cell, c + 256
    uint32_t width = 1u;
    while (width < cells && width < kRdThreads) width <<= 1;
    const uint32_t n_sub = kRdThreads / width, sub = t / width, c = t % width;
    const bool has0 = c < cells, has1 = c + kRdThreads < cells;
    for (uint32_t k = t; k < cells; k += kRdThreads) s_acc[k] = 0ull;
    __syncthreads();
    for (uint32_t s = rd_structure_of(a.so, a.b.n_structures, i0); s < a.b.n_structures; s++) {
        const uint32_t sb = a.so[s], se = a.so[s + 1u];
        if (sb >= i1) break;
        const uint32_t lo = max(sb, i0), hi = min(se, i1);
        if (lo >= hi) continue;  // an empty structure, or one that ends at i0 (the same in every thread)
        unsigned long long sum0 = 0ull, sum1 = 0ull;
        for (uint32_t i = lo + sub; i < hi; i += n_sub) {
            if ((a.classes ? (uint32_t)a.classes[i] : 0u) != cls) continue;
            const uint32_t *row = a.table + (size_t)i * cells;
            if (has0) sum0 += row[c];
            if (has1) sum1 += row[c + kRdThreads];
        }
        if (sum0) atomicAdd(&s_acc[c], sum0);
        if (sum1) atomicAdd(&s_acc[c + kRdThreads], sum1);
        __syncthreads();
        unsigned long long *dst = a.pairs + ((size_t)s * a.n_classes + cls) * cells;
        for (uint32_t k = t; k < cells; k += kRdThreads) {
            const unsigned long long v = s_acc[k];
            if (v) {
                atomicAdd(&dst[k], v);
                s_acc[k] = 0ull;
            }
        }
        __syncthreads();
    }
}

}  // namespace

// sorted_kinds[], then the table's row of every atom, on the grid of a binned batch; with r.pairs, the sums of the rows
// added to the pair tables, which the caller has zeroed on the stream.
void launch_radial(const RdArgs &r, hipStream_t stream)
{
    const uint32_t n = r.b.n_atoms;
    if (!n) return;
    hipLaunchKernelGGL(k_sort_kinds, dim3(cdiv(n, 256)), dim3(256), 0, stream, r);
    hipLaunchKernelGGL(k_radial_counts, dim3(cdiv(n, 4)), dim3(256), 0, stream, r);
    if (r.pairs) hipLaunchKernelGGL(k_radial_pairs, dim3(cdiv(n, kRdChunk), r.n_classes), dim3(kRdThreads), 0, stream, r);
}

}  // namespace rsasa
