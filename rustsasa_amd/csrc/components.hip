// Surface-component kernels (rsasa_surface_components*, gfx950 only): the accessible dots of every structure labelled by
// the connected component of the graph that links two dots no further apart than `link`, from the masks and the cell
// grid of a finished point run (k_accessible_points, still on the device).  The definition: include/rustsasa_amd.h.
//
//   k_component_free     one thread per atom: the popcount of its mask (free[], input order); the host scans it into the
//                        dot offsets (launch_neighbor_scan), so dot (j, k) has the batch-wide index offsets[j] + rank of k.
//   k_component_init     parent[d] = d for every dot.
//   k_component_link     one wave per cell-sorted atom i with free != 0.  The cells of its structure's grid are swept in
//                        Chebyshev shells around its own cell exactly as k_atom_depth sweeps them (depth.hip: x-runs of cell
//                        starts, 64 rows at a time, both cell-start encodings), but over the fixed reach below.  Lanes go
//                        first over the atoms of the runs and read free[] (4 bytes): the atoms with free != 0 that stand
//                        at or before i in the cell order - every unordered pair of atoms is taken once, i with itself
//                        included - are compacted into LDS.  Then, per chunk of 64 of i's own points (a lane holds the dot
//                        of its point if the bit is set) and per chunk of 64 of the staged atoms' points (mask words and
//                        lattice chunk in LDS), every dot of every staged atom is formed once for the wave, each lane
//                        evaluates the edge test - dx = q_a.x - q_b.x, ...; d2 = dx*dx + dy*dy + dz*dz; d2 <= link * link;
//                        float32, unfused, left to right; a NaN d2 fails - and on an edge unites the two dots.
//   k_component_flatten  one wave per atom: label[d] = root of d - first dot index of d's structure.
//
// The union-find.  parent[] only ever changes in two ways: a root r (parent[r] == r) is hung under a smaller root by
// atomicCAS(&parent[r], r, smaller), and a non-root's parent is replaced by one of its ancestors (path halving).  So every
// non-root has parent < self for good, a tree's root is its smallest dot, and the trees only merge.  A union finds both
// roots, returns if they are equal (every link followed was a real one, so the two dots are in one tree), and else hangs
// the larger under the smaller; a CAS that fails returns the larger one's real parent, and the union goes on from there
// with a strictly smaller pair.  A parent read that is out of date is a value that parent[] once held: still an ancestor
// (or the dot itself, which the CAS then refuses).  After the kernel every edge has its two dots in one tree, trees never
// cross components, and so each component is one tree whose root is its smallest dot, whatever the schedule.
// Plain 32-bit global atomics (relaxed, agent scope) and vector loads and stores; nothing else.
//
// The reach.  Let h = StructGrid::cell_size.  In a structure that passes the margins of k_atom_depth's stop rule (no odd
// radius or coordinate, probe >= 0, every |coordinate| <= 65536 h: the same test, restated here) an atom j not seen
// after shell s differs from i by more than (s - 1/8) h along some axis (depth.hip, "The stop rule").  Every dot lies
// within R <= h of its centre and the roundings of q and d are a few h / 128, so the float32 d2 of a dot of i and a dot of
// an unseen atom is above ((s - 2.25) h)^2.  The sweep covers the shells 0 .. S, S the smallest integer with
// (S - 2.5) h >= link: a quarter cell more than link * link (one float32 product) can reach, S = 3 for link <= h / 2, S = 4
// up to 1.5 h.  Where the margins do not hold, or S reaches the last shell that holds a cell of the grid, the whole grid
// is swept, which is exact for any input.
// Compiled with -ffp-contract=off: q and d2 are not fused (the definition is the model's plain float32 arithmetic).
#include "device_utils.h"

namespace rsasa {
namespace {

constexpr uint32_t kCcRuns = 128;  // x-runs of one step: two per row, 64 rows

__global__ __launch_bounds__(256) void k_component_free(CcArgs c)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= c.p.b.n_atoms) return;
    const uint32_t *m = c.p.masks + (size_t)i * c.p.words;
    uint32_t n = 0;
    for (uint32_t w = 0; w < c.p.words; w++) n += (uint32_t)__popc(m[w]);
    c.free[i] = n;
}

__global__ __launch_bounds__(256) void k_component_init(CcArgs c)
{
    const unsigned long long d = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (d < c.n_dots) c.parent[d] = (uint32_t)d;
}

// The margins of k_atom_depth's stop rule (dp_margins_hold, depth.hip).  NaN bounds fail every comparison.
__device__ __forceinline__ bool cc_margins_hold(const StructGrid &g, float probe)
{
    const float h = g.cell_size;
    const float ax = fabsf(g.min_x) + (float)g.dim_x * h, ay = fabsf(g.min_y) + (float)g.dim_y * h,
                az = fabsf(g.min_z) + (float)g.dim_z * h;
    return (g.odd_radii & 1u) == 0u && probe >= 0.0f && h > 0.0f && fmaxf(ax, fmaxf(ay, az)) <= 65536.0f * h;
}

// Flat position f of the concatenated runs -> cell-sorted position (as dp_pos, depth.hip).
__device__ __forceinline__ uint32_t cc_pos(const uint32_t *s_excl, const uint32_t *s_start, uint32_t f)
{
    uint32_t lo = 0;
#pragma unroll
    for (int step = kCcRuns / 2; step > 0; step >>= 1)
        if (s_excl[lo + step] <= f) lo += step;
    return s_start[lo] + (f - s_excl[lo]);
}

__device__ __forceinline__ uint32_t cc_load(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's tree as far as this thread can see (see the head of the file), halving the path on the way.
__device__ __forceinline__ uint32_t cc_find(uint32_t *parent, uint32_t x)
{
    uint32_t cur = cc_load(parent + x);
    if (cur < x) {
        uint32_t prev = x, next;
        while ((next = cc_load(parent + cur)) < cur) {
            __hip_atomic_store(parent + prev, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (prev is no root: no CAS takes it)
            prev = cur;
            cur = next;
        }
    }
    return cur;
}

// Unites the trees of a and b; returns the root both then hang under.  The larger of the pair falls with every round.
__device__ __forceinline__ uint32_t cc_union(uint32_t *parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return a;
        const uint32_t hi = max(a, b), lo = min(a, b);
        const uint32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return lo;
        a = old;  // hi's real parent, below hi
        b = lo;
    }
}

__global__ __launch_bounds__(256) void k_component_link(CcArgs c)
{
    const PtArgs &a = c.p;
    const BatchView &b = a.b;
    __shared__ uint32_t s_excl[4][kCcRuns], s_start[4][kCcRuns];
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
    const bool rel16 = g.in_lds != 0u;
    const uint32_t pos_base = rel16 ? g.sorted_base : 0u;
    uint32_t cx, cy, cz;
    cell_coords(g, me.x, me.y, me.z, cx, cy, cz);
    // the last shell that holds a cell of the grid, and the last one of the reach
    const uint32_t s_last = max(max(max(cx, g.dim_x - 1u - cx), max(cy, g.dim_y - 1u - cy)), max(cz, g.dim_z - 1u - cz));
    uint32_t s_end = s_last;
    if (cc_margins_hold(g, b.probe)) {
        const float t = c.link / g.cell_size + 2.5f;
        if (t < (float)s_last) {
            uint32_t S = (uint32_t)ceilf(t);
            while (((float)S - 2.5f) * g.cell_size < c.link) S++;
            s_end = min(S, s_last);
        }
    }
    const uint32_t n_chunks = (a.n_points + kWave - 1) / kWave;

    for (uint32_t s = 0; s <= s_end; s++) {
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
            // (an empty run shares its prefix with the next one; cc_pos then lands on the last run of that prefix, which
            // is the one that holds the position)
            const uint32_t total = wave_bcast(incl, kWave - 1);

            for (uint32_t f0 = 0; f0 < total; f0 += kWave) {
                // ---- lanes over the atoms of the runs: those with accessible points, at or before i, are staged
                const uint32_t f = f0 + lane;
                bool keep = false;
                uint32_t q = 0, orig = 0;
                if (f < total) {
                    q = cc_pos(s_excl[w], s_start[w], f);
                    if (q <= p) {
                        orig = b.sorted_orig[q];
                        keep = c.free[orig] != 0u;
                    }
                }
                const unsigned long long m = ballot64(keep);
                if (m == 0ull) continue;  // (the same in every lane)
                const uint32_t n_staged = (uint32_t)__popcll(m);
                const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
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
                    const uint32_t me_rank =
                        __builtin_amdgcn_mbcnt_hi((uint32_t)(mm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mm, 0u));
                    uint32_t root = me_dot0 + me_seen + me_rank;  // this lane's dot, later any dot above it in its tree
                    me_seen += (uint32_t)__popcll(mm);
                    if (mm == 0ull) continue;
                    const float ax = me.x + me_R * a.lx[pi], ay = me.y + me_R * a.ly[pi], az = me.z + me_R * a.lz[pi];
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
                        for (uint32_t k = 0; k < n_staged; k++) {
                            const uint2 kb = s_bits[w][k];  // (the same address in every lane: a broadcast)
                            unsigned long long jm = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)kb.y) << 32) |
                                                    (uint32_t)__builtin_amdgcn_readfirstlane((int)kb.x);
                            if (jm == 0ull) continue;
                            const float4 o = s_atom[w][k];
                            uint32_t dot = s_dot0[w][k];
                            for (; jm; jm &= jm - 1ull, dot++) {
                                const float4 sp = s_lat[w][__builtin_ctzll(jm)];
                                const float bx = o.x + o.w * sp.x, by = o.y + o.w * sp.y, bz = o.z + o.w * sp.z;
                                const float dx = ax - bx, dy = ay - by, dz = az - bz;
                                const float d2 = dx * dx + dy * dy + dz * dz;
                                if (mine && d2 <= c.link2) root = cc_union(c.parent, root, dot);
                            }
                        }
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_component_flatten(CcArgs c)
{
    const BatchView &b = c.p.b;
    const uint32_t p = blockIdx.x * 4u + threadIdx.x / kWave;
    if (p >= b.n_atoms) return;
    const uint32_t orig = b.sorted_orig[p];
    const uint32_t base = (uint32_t)c.dot_offsets[b.grids[b.sid_sorted[p]].atom_begin];  // the structure's first dot
    const uint32_t d1 = (uint32_t)c.dot_offsets[orig + 1u];
    for (uint32_t d = (uint32_t)c.dot_offsets[orig] + lane_id(); d < d1; d += kWave) c.labels[d] = cc_find(c.parent, d) - base;
}

}  // namespace

// free[] of every atom from the masks of a finished point run
void launch_component_free(const CcArgs &c, hipStream_t stream)
{
    const uint32_t n = c.p.b.n_atoms;
    if (!n) return;
    hipLaunchKernelGGL(k_component_free, dim3(cdiv(n, 256)), dim3(256), 0, stream, c);
}

// parent[] and labels[] of the n_dots (>= 1, < 2^32) dots that dot_offsets counts
void launch_components(const CcArgs &c, hipStream_t stream)
{
    const uint32_t n = c.p.b.n_atoms;
    if (!n || !c.n_dots) return;
    hipLaunchKernelGGL(k_component_init, dim3((uint32_t)((c.n_dots + 255ull) / 256ull)), dim3(256), 0, stream, c);
    hipLaunchKernelGGL(k_component_link, dim3(cdiv(n, 4)), dim3(256), 0, stream, c);
    hipLaunchKernelGGL(k_component_flatten, dim3(cdiv(n, 4)), dim3(256), 0, stream, c);
}

}  // namespace rsasa
