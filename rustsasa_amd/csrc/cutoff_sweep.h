// The stop rule of a shell sweep (sh_sweep of shell_sweep.h) that accepts an atom by d2 <= c2: shared by k_half_sphere
// (hse.hip), by k_within_count / k_within_fill (within.hip) and by k_nearest (nearest.hip), which hand it to the driver
// as their `after` and all evaluate, for the wave's atom i at c_i and an atom j at c_j,
//     dx = c_j.x - c_i.x (dy, dz alike);  d2 = dx*dx + dy*dy + dz*dz      float32, unfused, left to right
// and take j only if d2 <= c2 (whatever else they ask of j only removes atoms).  Device only, gfx950 only.
// k_radial_counts (radial.hip) is covered too: its acceptance is d2 <= c2 with c2 the last squared edge, e2[n_bins - 1].
// The bin it then finds only partitions what was accepted, so nothing below depends on it.
//
// The reach.  In a structure that passes sh_margins_hold an atom j not seen after shell s >= 1 has, along some axis,
// D = |x_j - x_i| > (s - 1/8) h in exact arithmetic, h = StructGrid::cell_size (shell_sweep.h, "What an unseen atom
// implies").  Its float32 d2 is no smaller than the float32 square of that axis' difference: the terms are not negative,
// and a rounded sum of a float a and a number b >= 0 is at least a (rounding is monotone, a is a float), which holds for
// both additions wherever the axis' term stands.  The difference carries one rounding and its square one more, so
//     d2 >= D^2 (1 - 2^-24)^3 > ((s - 1/8) h)^2 (1 - 2^-24)^3
// as long as the square does not underflow.  The sweep stops after shell s >= 1 when
//     c2 <= lim2,  lim = (float(s) - 0.5f) * h,  lim2 = lim * lim,  and lim2 >= 1e-30
// (float(s) - 0.5f is exact, s < 2^18 under the margins; two roundings): lim2 <= ((s - 1/2) h)^2 (1 + 2^-24)^3, and
// ((s - 1/8) / (s - 1/2))^2 > 1 + 3 / (4 s) > 1 + 2^-19, far above the six roundings' 1 + 2^-21, so every unseen d2 is
// strictly above lim2 >= c2: no unseen atom is accepted, and one with d2 == c2 has been seen.  lim2 >= 1e-30 keeps D^2 in
// the normal range, where the roundings are relative.  (NaN d2 is accepted for nobody, seen or not; c2 = +inf never meets
// the rule.)  Without the margins, or when the rule is never met, the caller's sweep ends when the shells cover the grid
// (ShCell::s_last), which is always exact.  For cutoff 13 and h = 3.3 the rule is met after shell 5.
//
// A bound found on the way.  k_nearest (nearest.hip) wants the k smallest keys (bits(d2) << 32) | idx among the atoms with
// d2 <= c2 and calls the rule with b2 = min(c2, the k-th smallest d2 it holds once it holds k, else +inf) in place of c2.
// The proof carries over word for word, being about one number compared with lim2: every unseen d2 is strictly above
// lim2 >= b2.  If b2 = c2 no unseen atom is eligible; otherwise k held keys have d2 <= b2 < every unseen d2, so an unseen
// atom cannot displace any of them, not even on a tie of d2 (where idx would decide).  The k-th smallest held d2 only falls
// as the sweep goes on, and "the k-th smallest is at most lim2" is "at least k held d2 are at most lim2", which needs
// no sort.  Without the margins the rule is never met and the whole grid is swept.
#pragma once
#include "shell_sweep.h"

namespace rsasa {
namespace {

// Whether the sweep may stop after shell s: margins = sh_margins_hold of the structure, h its cell size, c2 = C * C.
__device__ __forceinline__ bool sh_cutoff_reached(bool margins, uint32_t s, float h, float c2)
{
    if (margins && s >= 1u) {
        const float lim = ((float)s - 0.5f) * h;
        const float lim2 = lim * lim;
        if (c2 <= lim2 && lim2 >= 1e-30f) return true;
    }
    return false;
}

}  // namespace
}  // namespace rsasa
