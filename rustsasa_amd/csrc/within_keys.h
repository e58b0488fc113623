// What the kernels that list atoms by distance share - k_within_count / k_within_fill (within.hip) and k_nearest
// (nearest.hip): the ONE acceptance rule of a centre and a candidate (wn_accept: include/rustsasa_amd.h,
// rsasa_atoms_within) and the sort of a wave's staged 64-bit keys (float bits of d2) << 32 | idx in LDS (wn_sort).
// d2 >= 0 and never NaN in a list, so the key's bits order like (d2, idx), and the key IS the entry (rsasa_within_t: d2
// in the low address, idx behind it).  Device only, gfx950 only.
#pragma once
#include "cutoff_sweep.h"

namespace rsasa {
namespace {

struct WnAtom {  // what the rule needs of the wave's atom beside its frame (ShFrame): its input index and the run's rule
    uint32_t orig;
    float c2;
    bool upper;
};

// THE acceptance rule (include/rustsasa_amd.h, rsasa_atoms_within), used by every pass: the atom at cell-sorted
// position q is in the list of the wave's atom when it is another atom, a partner, d2 <= c2 and, under upper_only, its
// input index is the larger one (atoms of one structure: the same order as their indices within it).  orig_q: q's
// input index when `want_orig` (the passes that write entries, and every pass under upper_only), else 0.
__device__ __forceinline__ bool wn_accept(const WnArgs &a, const ShFrame &fr, const WnAtom &at, uint32_t q, bool want_orig,
                                          float &d2, uint32_t &orig_q)
{
    const BatchView &b = a.n.b;
    const float4 o = b.sorted_xyzr[q];
    const uint32_t fl = a.sorted_flags[q];
    orig_q = want_orig ? b.sorted_orig[q] : 0u;
    const float dx = o.x - fr.me.x, dy = o.y - fr.me.y, dz = o.z - fr.me.z;
    d2 = dx * dx + dy * dy + dz * dz;
    return q != fr.p && (fl & 1u) != 0u && d2 <= at.c2 && (!at.upper || orig_q > at.orig);
}

// The wave's n keys in s_key, ascending: padded with all-ones keys to P, the power of two at or above n (s_key holds at
// least P keys), and sorted by the bitonic network of log2 P (log2 P + 1) / 2 stages of P / 2 compare-exchanges (see the
// head of within.hip).  One wave; the keys of the caller's earlier writes need no fence of the caller's.
__device__ __forceinline__ void wn_sort(unsigned long long *s_key, uint32_t n)
{
    const uint32_t lane = lane_id();
    uint32_t P = 2;
    while (P < n) P <<= 1;
    for (uint32_t i = n + lane; i < P; i += kWave) s_key[i] = ~0ull;
    for (uint32_t size = 2; size <= P; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            wave_lds_fence();
            for (uint32_t t = lane; t < P / 2u; t += kWave) {
                const uint32_t i = ((t & ~(stride - 1u)) << 1) | (t & (stride - 1u)), j = i | stride;
                const unsigned long long x = s_key[i], y = s_key[j];
                if ((x > y) == ((i & size) == 0u)) {  // ascending where bit `size` of i is clear (always, in the last merge)
                    s_key[i] = y;
                    s_key[j] = x;
                }
            }
        }
    }
    wave_lds_fence();
}

}  // namespace
}  // namespace rsasa
