// Surface-component kernels (rsasa_surface_components*, gfx950 only): the accessible dots of every structure labelled by
// the connected component of the graph that links two dots no further apart than `link`, from the masks and the cell
// grid of a finished point run (k_accessible_points, still on the device).  The definition: include/rustsasa_amd.h.
//
// The popcounts of the masks (free[], input order) come from k_mask_free (points.hip); the host scans them into the dot
// offsets (launch_neighbor_scan), so dot (j, k) has the batch-wide index offsets[j] + rank of k.
//
//   k_component_init     parent[d] = d for every dot.
//   k_component_link     one wave per cell-sorted atom i with free != 0, over the shell sweep of shell_sweep.h (the one
//                        k_atom_depth runs), but over the fixed reach below.  Lanes go first over the atoms of a step's
//                        runs and read free[] (4 bytes): the atoms with free != 0 that stand
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
// The reach.  In a structure that passes sh_margins_hold an atom j not seen after shell s differs from i by more than
// (s - 1/8) h along some axis, h = StructGrid::cell_size (shell_sweep.h, "What an unseen atom implies").  Every dot lies
// within R <= h of its centre and the roundings of q and d are a few h / 128, so the float32 d2 of a dot of i and a dot of
// an unseen atom is above ((s - 2.25) h)^2.  The sweep covers the shells 0 .. S, S the smallest integer with
// (S - 2.5) h >= link: a quarter cell more than link * link (one float32 product) can reach, S = 3 for link <= h / 2, S = 4
// up to 1.5 h.  Where the margins do not hold, or S reaches the last shell that holds a cell of the grid, the whole grid
// is swept, which is exact for any input.
// k_component_link writes the loops of sh_sweep (shell_sweep.h: the driver and its contract) out, and must follow a change
// there by hand: run by the driver it measured 9 % slower at the same registers (profiles/sweep_driver_ab.txt).
// Compiled with -ffp-contract=off: q and d2 are not fused (the definition is the model's plain float32 arithmetic).
#include "shell_sweep.h"

namespace rsasa {
namespace {

__global__ __launch_bounds__(256) void k_component_init(CcArgs c)
{
    const unsigned long long d = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (d < c.n_dots) c.parent[d] = (uint32_t)d;
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
    uint32_t s_end = cell.s_last;  // the last shell of the reach
    if (sh_margins_hold(g, b.probe)) {
        const float t = c.link / g.cell_size + 2.5f;
        if (t < (float)cell.s_last) {
            uint32_t S = (uint32_t)ceilf(t);
            while (((float)S - 2.5f) * g.cell_size < c.link) S++;
            s_end = min(S, cell.s_last);
        }
    }
    const uint32_t n_chunks = (a.n_points + kWave - 1) / kWave;

    for (uint32_t s = 0; s <= s_end; s++) {
        const ShShell shell = sh_shell(g, cell, s);
        for (unsigned long long r0 = 0; r0 < shell.n_rows; r0 += kWave) {
            const uint32_t total = sh_step_runs(b, g, cell, shell, s, r0, s_excl[w], s_start[w]);
            for (uint32_t f0 = 0; f0 < total; f0 += kWave) {
                // ---- lanes over the atoms of the runs: those with accessible points, at or before i, are staged
                const uint32_t f = f0 + lane;
                bool keep = false;
                uint32_t q = 0, orig = 0;
                if (f < total) {
                    q = sh_pos(s_excl[w], s_start[w], f);
                    if (q <= p) {
                        orig = b.sorted_orig[q];
                        keep = c.free[orig] != 0u;
                    }
                }
                // (sh_stage, written out: with the first dot read in front of the call the kernel measured 4 % slower)
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
                    const uint32_t me_rank = mbcnt64(mm);
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
