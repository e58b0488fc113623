// The shell sweep of the wave-per-atom kernels that search the grid beyond the neighbour reach (device only, gfx950
// only): its frame (sh_frame), its driver (sh_sweep) and the steps the driver is made of.  Ten kernels sweep this way,
// each with its own work per batch of atoms (the driver's `visit`) and its own stop rule (its `after`).
// Run by sh_sweep:
//   k_half_sphere (hse.hip)            sh_cutoff_reached(c2) of cutoff_sweep.h
//   k_nearest (nearest.hip)            the same, or the k-th smallest staged d2 in place of c2 (nn_kth_reached)
//   k_radial_counts (radial.hip)       sh_cutoff_reached(the last squared edge)
//   k_dot_crowding (crowding.hip)      the last squared edge <= ((s - 1.5) h)^2, s >= 2: the partners are counted around
//                                      the dots of i, which lie up to h from c_i (written out it was not timed)
//   k_dot_enclosure (enclosure.hip)    reach^2 <= ((s - 2.5) h)^2, s >= 3: rays from the dots of i, up to h from c_i, are
//                                      stopped by spheres of up to h around the atoms (written out it was not timed)
// With the driver's three loops written out, because run by sh_sweep they measured slower on the MI355X at the same
// registers, LDS and (within a few) instructions - the table is profiles/sweep_driver_ab.txt; their instruction streams
// are the ones they had before the driver existed.  A change to sh_sweep is made in these four places too:
//   wn_sweep of k_within_count and k_within_fill (within.hip)   sh_cutoff_reached(c2); the fill 1.1 to 1.2 % slower
//   k_atom_depth (depth.hip)           best_d2 <= ((s - 2) h)^2, after reducing `best` over the wave; 3.6 to 4.7 % slower
//   k_component_link (components.hip)  a fixed reach, shells 0 .. s_end, computed before the sweep; 9 % slower.  It does
//                                      not take sh_frame either: with the frame alone its listing changes (936
//                                      instructions for 932), and that build was not timed.
//   k_dot_link (geodesics.hip)         k_component_link's loops and reach.  The three instantiations were not run through
//                                      the driver (the 9 % are the components kernel's); sharing one written-out body
//                                      with k_component_link was timed, and the fill or the weights came out slower
//                                      (profiles/dot_pairs_ab.txt), so the body stands twice.
// One wave per cell-sorted atom i.  The cells of its structure's grid are swept in Chebyshev shells s = 0, 1, 2, ... around
// its own cell: shell s is the cells at distance exactly s, cut into x-runs of cell starts as nb_runs cuts the 5x5x5 block
// - a row (y, z) on the rim of the shell's square gives the whole run [cx - s, cx + s], a row inside it the two cells
// cx - s and cx + s -, 64 rows at a time (sh_step_runs), both cell-start encodings (StructGrid::in_lds).  Lanes then go
// over the atoms of the runs, 64 at a time (sh_pos), and the atoms a kernel keeps it may compact into LDS (sh_stage;
// k_component_link writes that one step out, see there).
//
// The driver's contract.  sh_sweep holds the three loops (shells, steps of 64 rows, batches of 64 atoms), and every proof
// in cutoff_sweep.h, depth.hip and components.hip rests on them being exactly this, in sh_sweep and in the three copies:
//   - every cell of the shells 0 .. s has been visited before `after` is asked about s;
//   - "the shells cover the grid" (s >= ShCell::s_last) is tested before the kernel's own rule and ends the sweep whatever
//     that rule says; sh_sweep hands it to `after` as `last`, so a rule that costs something returns at once when it is set;
//   - every lane of the wave reaches every ballot: `visit` and `after` are called by all 64 lanes, lanes without an atom
//     included (`in` false), and no lane leaves the loops before the others.
//
// What an unseen atom implies.  Let h = StructGrid::cell_size = probe + max_r.  After shell s every atom j not yet seen
// has a cell coordinate that differs from i's by more than s along some axis.  A cell coordinate is floor(t'), t' the
// float32 value of (x - min) * inv_cell, except where the clamp to dim - 1 lowered it; following the cases (i clamped: no
// larger coordinate exists; j clamped: its coordinate is the largest, so it is not below i's) |t'_j - t'_i| > s.  In a
// structure that passes sh_margins_hold - no odd radius or coordinate (every 0 <= R_j <= h, R_j and h being the same
// rounded sum of a radius and the probe), probe >= 0, and every |coordinate| <= 65536 h - a coordinate's ulp is at most
// h / 128 and t' < 2^18, so t' is within 1/16 of the exact (x - min) / h, and |x_j - x_i| > (s - 1/8) h.  Every dot of j
// lies within R_j <= h of c_j, and a dot q = c_j + R_j * s_k and a difference of two points carry a few roundings of at
// most h / 128 each.  The stop rules of the ten kernels follow from this; without the margins every one of them sweeps
// until the shells cover the grid (ShCell::s_last), which is always exact.
#pragma once
#include "device_utils.h"

namespace rsasa {
namespace {

constexpr uint32_t kShRuns = 128;  // x-runs of one step: two per row, 64 rows

// Whether the margins hold in this structure (see the head of the file).  NaN bounds fail every comparison.
__device__ __forceinline__ bool sh_margins_hold(const StructGrid &g, float probe)
{
    const float h = g.cell_size;
    const float ax = fabsf(g.min_x) + (float)g.dim_x * h, ay = fabsf(g.min_y) + (float)g.dim_y * h,
                az = fabsf(g.min_z) + (float)g.dim_z * h;
    return (g.odd_radii & 1u) == 0u && probe >= 0.0f && h > 0.0f && fmaxf(ax, fmaxf(ay, az)) <= 65536.0f * h;
}

// Flat position f of the concatenated runs -> cell-sorted position (nb_pos over kShRuns entries).
__device__ __forceinline__ uint32_t sh_pos(const uint32_t *s_excl, const uint32_t *s_start, uint32_t f)
{
    uint32_t lo = 0;
#pragma unroll
    for (int step = kShRuns / 2; step > 0; step >>= 1)
        if (s_excl[lo + step] <= f) lo += step;
    return s_start[lo] + (f - s_excl[lo]);
}

struct ShCell {  // the cell of the wave's atom
    uint32_t cx, cy, cz;
    uint32_t s_last;    // the last shell that holds a cell of the grid
    bool rel16;         // the structure's cell starts are 16-bit, relative to pos_base
    uint32_t pos_base;
};

__device__ __forceinline__ ShCell sh_cell(const StructGrid &g, const float4 me)
{
    ShCell c;
    c.rel16 = g.in_lds != 0u;
    c.pos_base = c.rel16 ? g.sorted_base : 0u;
    cell_coords(g, me.x, me.y, me.z, c.cx, c.cy, c.cz);
    c.s_last = max(max(max(c.cx, g.dim_x - 1u - c.cx), max(c.cy, g.dim_y - 1u - c.cy)), max(c.cz, g.dim_z - 1u - c.cz));
    return c;
}

struct ShShell {  // shell s: the rows (y, z) of its square that lie in the grid, row r = (y0 + r % ny, z0 + r / ny)
    uint32_t y0, z0, ny;
    unsigned long long n_rows;
    uint32_t x0, x1;      // the x-run of a row on the rim
    bool has_lo, has_hi;  // the cells cx - s, cx + s exist
};

__device__ __forceinline__ ShShell sh_shell(const StructGrid &g, const ShCell &c, uint32_t s)
{
    ShShell sh;
    const uint32_t y1 = min(c.cy + s, g.dim_y - 1u), z1 = min(c.cz + s, g.dim_z - 1u);
    sh.y0 = c.cy >= s ? c.cy - s : 0u;
    sh.z0 = c.cz >= s ? c.cz - s : 0u;
    sh.ny = y1 - sh.y0 + 1u;
    sh.n_rows = (unsigned long long)sh.ny * (z1 - sh.z0 + 1u);
    sh.x0 = c.cx >= s ? c.cx - s : 0u;
    sh.x1 = min(c.cx + s, g.dim_x - 1u);
    sh.has_lo = c.cx >= s;
    sh.has_hi = c.cx + s <= g.dim_x - 1u;
    return sh;
}

// One step of shell s: lane l turns row r0 + l into its x-runs, and the wave's 128 runs go to s_excl (the exclusive
// prefix sums of their lengths) and s_start (their first cell-sorted positions).  Returns the atoms of the step.  (An empty
// run shares its prefix with the next one; sh_pos then lands on the last run of that prefix, which is the one that holds
// the position.)
__device__ __forceinline__ uint32_t sh_step_runs(const BatchView &b, const StructGrid &g, const ShCell &c, const ShShell &sh,
                                                 uint32_t s, unsigned long long r0, uint32_t *s_excl, uint32_t *s_start)
{
    const uint32_t lane = lane_id();
    uint32_t len_a = 0, len_b = 0, start_a = 0, start_b = 0;
    const unsigned long long rr = r0 + lane;
    if (rr < sh.n_rows) {
        const uint32_t yy = sh.y0 + (uint32_t)(rr % sh.ny), zz = sh.z0 + (uint32_t)(rr / sh.ny);
        const uint32_t dy = yy > c.cy ? yy - c.cy : c.cy - yy, dz = zz > c.cz ? zz - c.cz : c.cz - zz;
        const uint32_t c_row = g.cell_base + yy * g.dim_x + zz * g.dim_x * g.dim_y;
        if (max(dy, dz) == s) {  // on the rim: every cell of [x0, x1] is at distance s
            uint32_t f0, f1;
            load_cell_start2(b.cells, c_row + sh.x0, c_row + sh.x1 + 1u, c.rel16, f0, f1);
            start_a = c.pos_base + f0;
            len_a = f1 - f0;
        } else {  // inside (s >= 1): the two cells at |dx| = s
            if (sh.has_lo) {
                uint32_t f0, f1;
                load_cell_start2(b.cells, c_row + c.cx - s, c_row + c.cx - s + 1u, c.rel16, f0, f1);
                start_a = c.pos_base + f0;
                len_a = f1 - f0;
            }
            if (sh.has_hi) {
                uint32_t f0, f1;
                load_cell_start2(b.cells, c_row + c.cx + s, c_row + c.cx + s + 1u, c.rel16, f0, f1);
                start_b = c.pos_base + f0;
                len_b = f1 - f0;
            }
        }
    }
    const uint32_t incl = wave_incl_scan(len_a + len_b);
    wave_lds_fence();  // (every lane is done with the previous step's runs)
    s_excl[2u * lane] = incl - len_a - len_b;
    s_excl[2u * lane + 1u] = incl - len_b;
    s_start[2u * lane] = start_a;
    s_start[2u * lane + 1u] = start_b;
    wave_lds_fence();
    return wave_bcast(incl, kWave - 1);
}

// The lanes with `keep` (their atom at cell-sorted position q) are compacted into LDS in lane order: s_atom gets
// (c_j, R_j = r_j + probe), s_who the caller's pair.  Returns the number staged (the same in every lane); 0: nothing was
// written.
__device__ __forceinline__ uint32_t sh_stage(const BatchView &b, bool keep, uint32_t q, uint2 who, float4 *s_atom, uint2 *s_who)
{
    const unsigned long long m = ballot64(keep);
    if (m == 0ull) return 0u;
    const uint32_t n_staged = (uint32_t)__popcll(m);
    const uint32_t slot = mbcnt64(m);
    wave_lds_fence();  // (every lane is done with the previous atoms)
    if (keep) {
        const float4 o = b.sorted_xyzr[q];
        s_atom[slot] = make_float4(o.x, o.y, o.z, o.w + b.probe);
        s_who[slot] = who;
    }
    wave_lds_fence();
    return n_staged;
}

struct ShFrame {  // what every sweep kernel holds of the wave's atom before the sweep
    uint32_t p;    // its cell-sorted position
    StructGrid g;  // its structure's grid
    float4 me;     // (c_i, r_i)
    ShCell cell;
    bool margins;  // sh_margins_hold
};

__device__ __forceinline__ ShFrame sh_frame(const BatchView &b, uint32_t p)
{
    ShFrame fr;
    fr.p = p;
    fr.g = b.grids[b.sid_sorted[p]];
    fr.me = b.sorted_xyzr[p];
    fr.cell = sh_cell(fr.g, fr.me);
    fr.margins = sh_margins_hold(fr.g, b.probe);
    return fr;
}

// THE sweep (the contract: the head of the file).  visit(in, q): every lane, once per batch of 64 flat positions of a
// step's runs; `in`: the lane has an atom, q its cell-sorted position (else 0).  after(s, last): every lane, once per
// shell, after all of its steps; last = s >= s_last; the sweep ends when `last` is set or `after` returns true.
// s_excl, s_start: the wave's run tables (LDS, kShRuns entries each).
template <class Visit, class After>
__device__ __forceinline__ void sh_sweep(const BatchView &b, const ShFrame &fr, uint32_t *s_excl, uint32_t *s_start,
                                         Visit visit, After after)
{
    const uint32_t lane = lane_id();
    for (uint32_t s = 0;; s++) {
        const ShShell shell = sh_shell(fr.g, fr.cell, s);
        for (unsigned long long r0 = 0; r0 < shell.n_rows; r0 += kWave) {
            const uint32_t total = sh_step_runs(b, fr.g, fr.cell, shell, s, r0, s_excl, s_start);
            for (uint32_t f0 = 0; f0 < total; f0 += kWave) {
                const uint32_t f = f0 + lane;
                const bool in = f < total;
                visit(in, in ? sh_pos(s_excl, s_start, f) : 0u);
            }
        }
        const bool last = s >= fr.cell.s_last;  // the shells cover the grid
        if (after(s, last) || last) break;
    }
}

}  // namespace
}  // namespace rsasa
