// Atom-depth kernels (rsasa_atom_depth*, gfx950 only): for every atom the nearest accessible dot of its own structure,
// from the cell grid of a finished point run (the masks of k_accessible_points, still on the device).
//
//   k_depth_free    one thread per atom: the popcount of its mask (free[], input order).
//   k_atom_depth    one wave per cell-sorted atom i.  The cells of its structure's grid are swept in Chebyshev shells
//                   s = 0, 1, 2, ... around its own cell: shell s is the cells at distance exactly s, cut into x-runs of
//                   cell starts as nb_runs cuts the 5x5x5 block - a row (y, z) on the rim of the shell's square gives
//                   the whole run [cx - s, cx + s], a row inside it the two cells cx - s and cx + s -, 64 rows at a time,
//                   both cell-start encodings (StructGrid::in_lds).  Lanes go first over the atoms of the runs, 64 at a
//                   time, and read free[] (4 bytes): the atoms with free != 0 are compacted into LDS as (c_j, R_j) and
//                   (row, j).  Then lanes go over the points in chunks of 64: per chunk the two mask words of every staged
//                   atom are fetched to LDS at once, and every lane with its bit set evaluates the definition
//                   (include/rustsasa_amd.h) - R = r + p; q = c_j + R * s_k; d = c_i - q; d2 = dx*dx + dy*dy + dz*dz, float32,
//                   unfused, left to right - and keeps the smallest key (bits(d2) << 32) | j of those whose d2 is no NaN.
//                   After every shell the lanes' minima are reduced over the wave.
//
// The stop rule.  Let h = StructGrid::cell_size = probe + max_r.  After shell s every atom j not yet seen has a cell
// coordinate that differs from i's by more than s along some axis.  A cell coordinate is floor(t'), t' the float32 value
// of (x - min) * inv_cell, except where the clamp to dim - 1 lowered it; following the cases (i clamped: no larger
// coordinate exists; j clamped: its coordinate is the largest, so it is not below i's) |t'_j - t'_i| > s.  The sweep stops
// early only in a structure that passes dp_margins_hold: no odd radius or coordinate (every 0 <= R_j <= h, R_j and h
// being the same rounded sum of a radius and the probe), probe >= 0, and every |coordinate| <= 65536 h.  There a
// coordinate's ulp is at most h / 128 and t' < 2^18, so t' is within 1/16 of the exact (x - min) / h, and
// |x_j - x_i| > (s - 1/8) h.  Every dot of j lies within R_j <= h of c_j, and q and d carry a few roundings of at most
// h / 128 each, so the float32 d2 of any dot of an unseen atom is above ((s - 1.25) h)^2.  The sweep stops after shell s
// when best_d2 <= ((s - 2) h)^2 (one float32 product and square: rounding far below the 0.75 h between the two bounds):
// every unseen key is strictly larger than the one held, ties included.  Without the margins the sweep ends when the
// shells cover the grid, which is always exact.
// No per-candidate bound (|c_i - c_j| - R_j) and no per-cell summary of the dots were built: see DESIGN 5g.
// Compiled with -ffp-contract=off: q and d2 are not fused (the definition is the model's plain float32 arithmetic).
#include "device_utils.h"

namespace rsasa {
namespace {

constexpr uint32_t kDpRuns = 128;  // x-runs of one step: two per row, 64 rows

__global__ __launch_bounds__(256) void k_depth_free(DpArgs d)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= d.p.b.n_atoms) return;
    const uint32_t *m = d.p.masks + (size_t)i * d.p.words;
    uint32_t n = 0;
    for (uint32_t w = 0; w < d.p.words; w++) n += (uint32_t)__popc(m[w]);
    d.free[i] = n;
}

// Whether the stop rule's margins hold in this structure (see the head of the file).  NaN bounds fail every comparison.
__device__ __forceinline__ bool dp_margins_hold(const StructGrid &g, float probe)
{
    const float h = g.cell_size;
    const float ax = fabsf(g.min_x) + (float)g.dim_x * h, ay = fabsf(g.min_y) + (float)g.dim_y * h,
                az = fabsf(g.min_z) + (float)g.dim_z * h;
    return (g.odd_radii & 1u) == 0u && probe >= 0.0f && h > 0.0f && fmaxf(ax, fmaxf(ay, az)) <= 65536.0f * h;
}

// Flat position f of the concatenated runs -> cell-sorted position (nb_pos over kDpRuns entries).
__device__ __forceinline__ uint32_t dp_pos(const uint32_t *s_excl, const uint32_t *s_start, uint32_t f)
{
    uint32_t lo = 0;
#pragma unroll
    for (int step = kDpRuns / 2; step > 0; step >>= 1)
        if (s_excl[lo + step] <= f) lo += step;
    return s_start[lo] + (f - s_excl[lo]);
}

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
    __shared__ uint32_t s_excl[4][kDpRuns], s_start[4][kDpRuns];
    __shared__ float4 s_atom[4][kWave];  // (c_j, R_j) of the staged atoms
    __shared__ uint2 s_who[4][kWave];    // (input row, index within the structure)
    __shared__ uint2 s_bits[4][kWave];   // their mask words of the current chunk
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= b.n_atoms) return;
    const StructGrid g = b.grids[b.sid_sorted[p]];
    const float4 me = b.sorted_xyzr[p];
    const bool rel16 = g.in_lds != 0u;
    const uint32_t pos_base = rel16 ? g.sorted_base : 0u;
    uint32_t cx, cy, cz;
    cell_coords(g, me.x, me.y, me.z, cx, cy, cz);
    // the last shell that holds a cell of the grid
    const uint32_t s_last = max(max(max(cx, g.dim_x - 1u - cx), max(cy, g.dim_y - 1u - cy)), max(cz, g.dim_z - 1u - cz));
    const bool margins = dp_margins_hold(g, b.probe);
    const uint32_t n_chunks = (a.n_points + kWave - 1) / kWave;

    unsigned long long best = ~0ull;  // this lane's smallest key; after a shell, the wave's
    for (uint32_t s = 0;; s++) {
        // the rows (y, z) of the shell's square that lie in the grid
        const uint32_t y0 = cy >= s ? cy - s : 0u, y1 = min(cy + s, g.dim_y - 1u);
        const uint32_t z0 = cz >= s ? cz - s : 0u, z1 = min(cz + s, g.dim_z - 1u);
        const uint32_t ny = y1 - y0 + 1u;
        const unsigned long long n_rows = (unsigned long long)ny * (z1 - z0 + 1u);
        const uint32_t x0 = cx >= s ? cx - s : 0u, x1 = min(cx + s, g.dim_x - 1u);
        const bool has_lo = cx >= s, has_hi = cx + s <= g.dim_x - 1u;  // the cells cx - s, cx + s exist
        for (unsigned long long r0 = 0; r0 < n_rows; r0 += kWave) {
            // ---- this step's runs: lane l takes row r0 + l
            uint32_t len_a = 0, len_b = 0, start_a = 0, start_b = 0;
            const unsigned long long rr = r0 + lane;
            if (rr < n_rows) {
                const uint32_t yy = y0 + (uint32_t)(rr % ny), zz = z0 + (uint32_t)(rr / ny);
                const uint32_t dy = yy > cy ? yy - cy : cy - yy, dz = zz > cz ? zz - cz : cz - zz;
                const uint32_t c_row = g.cell_base + yy * g.dim_x + zz * g.dim_x * g.dim_y;
                if (max(dy, dz) == s) {  // on the rim: every cell of [x0, x1] is at distance s
                    uint32_t f0, f1;
                    load_cell_start2(b.cells, c_row + x0, c_row + x1 + 1u, rel16, f0, f1);
                    start_a = pos_base + f0;
                    len_a = f1 - f0;
                } else {  // inside (s >= 1): the two cells at |dx| = s
                    if (has_lo) {
                        uint32_t f0, f1;
                        load_cell_start2(b.cells, c_row + cx - s, c_row + cx - s + 1u, rel16, f0, f1);
                        start_a = pos_base + f0;
                        len_a = f1 - f0;
                    }
                    if (has_hi) {
                        uint32_t f0, f1;
                        load_cell_start2(b.cells, c_row + cx + s, c_row + cx + s + 1u, rel16, f0, f1);
                        start_b = pos_base + f0;
                        len_b = f1 - f0;
                    }
                }
            }
            const uint32_t incl = wave_incl_scan(len_a + len_b);
            wave_lds_fence();  // (every lane is done with the previous step's runs)
            s_excl[w][2u * lane] = incl - len_a - len_b;
            s_excl[w][2u * lane + 1u] = incl - len_b;
            s_start[w][2u * lane] = start_a;
            s_start[w][2u * lane + 1u] = start_b;
            wave_lds_fence();
            // (an empty run shares its prefix with the next one; dp_pos then lands on the last run of that prefix, which
            // is the one that holds the position)
            const uint32_t total = wave_bcast(incl, kWave - 1);

            for (uint32_t f0 = 0; f0 < total; f0 += kWave) {
                // ---- lanes over the atoms of the runs: those with accessible points are staged
                const uint32_t f = f0 + lane;
                bool keep = false;
                uint32_t q = 0, orig = 0;
                if (f < total) {
                    q = dp_pos(s_excl[w], s_start[w], f);
                    orig = b.sorted_orig[q];
                    keep = d.free[orig] != 0u;
                }
                const unsigned long long m = ballot64(keep);
                if (m == 0ull) continue;  // (the same in every lane)
                const uint32_t n_staged = (uint32_t)__popcll(m);
                const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                wave_lds_fence();  // (every lane is done with the previous atoms)
                if (keep) {
                    const float4 o = b.sorted_xyzr[q];
                    s_atom[w][slot] = make_float4(o.x, o.y, o.z, o.w + b.probe);  // R_j = r_j + p
                    s_who[w][slot] = make_uint2(orig, orig - g.atom_begin);
                }
                wave_lds_fence();
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
        if (s >= s_last) break;  // the shells cover the grid
        if (margins && s >= 2u && best != ~0ull) {
            const float lim = (float)(s - 2u) * g.cell_size;
            if (__uint_as_float((uint32_t)(best >> 32)) <= lim * lim) break;
        }
    }
    if (lane == 0) d.keys[b.sorted_orig[p]] = best;
}

}  // namespace

// free[] of every atom from the masks of a finished point run, then keys[]
void launch_atom_depth(const DpArgs &d, hipStream_t stream)
{
    const uint32_t n = d.p.b.n_atoms;
    if (!n) return;
    hipLaunchKernelGGL(k_depth_free, dim3(cdiv(n, 256)), dim3(256), 0, stream, d);
    hipLaunchKernelGGL(k_atom_depth, dim3(cdiv(n, 4)), dim3(256), 0, stream, d);
}

}  // namespace rsasa
