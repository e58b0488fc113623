// The-k-nearest-atoms kernels (rsasa_nearest_atoms*, gfx950 only): for every centre the first k entries of the list
// rsasa_atoms_within defines for it at the same flags and cutoff (upper_only off) - the k partners of its own structure
// with the smallest keys (float bits of d2) << 32 | idx, whatever their distance when the cutoff is +inf.  They need the
// cell grid of a binned batch and the flag bytes in cell-sorted order (k_sort_flags of hse.hip), as within.hip does.
//
//   k_nearest          one wave per cell-sorted atom i, four per workgroup, run by sh_sweep (shell_sweep.h: the driver
//                      and its contract); a wave whose atom is no centre writes count 0 and returns.  Its `visit`:
//                      each lane evaluates wn_accept (within_keys.h: THE rule of rsasa_atoms_within, `upper` off) and
//                      the accepted candidates are staged as keys in the wave's LDS staging (compacted first when the
//                      next 64 might not fit); its `after`: the stop rule below.  At the end the staging is sorted once
//                      (wn_sort) and the first min(k, held) keys go to the centre's row of stride k in device scratch,
//                      the row's length to counts[input atom].
//   the scan           launch_neighbor_scan (neighbors.hip) turns the counts into offsets and NbInfo; NbArgs::stage = k,
//                      so no list counts as long.  The host sizes the caller's buffer from them as every list call does.
//   k_nearest_gather   one wave per input atom: the row's counts[atom] keys -> out[offsets[atom] ..), 64 consecutive
//                      entries per store.  Every write is bounded by the count, by k and by the offsets; a count above
//                      k sets NbInfo::mismatch, which the host answers with RSASA_ERR_INTERNAL.
//
// One sweep, no count pass: the reach is not known before the sweep, and a row of k keys per centre bounds what a
// centre can write, so the sizes come out of the same pass as the entries.
//
// Rows are per centre, not per atom.  With flags == NULL the row is the input atom.  Otherwise it is the centre's rank:
// the number of centres before it in input order, made by a HOST prefix over the flag bytes and uploaded beside the
// columns (the host reads the flags anyway to size the rows; RunScratch::map, as idx_map of the neighbour runs) - one
// atom in eight a centre takes an eighth of the scratch.
//
// The stop rule.  Let b2 = min(c2, the k-th smallest staged d2 once at least k keys are held, else +inf).  After shell s
// the sweep stops when the shells cover the grid (the driver's `last`: nothing is counted then) or
// sh_cutoff_reached(margins, s, h, b2) holds: by the proof in cutoff_sweep.h every unseen atom has d2 strictly above
// lim2 >= b2, so it is outside the cutoff or cannot displace any of the k held keys, not even on a tie of d2.  No sort is
// needed for it: "the k-th smallest d2 meets the rule" is "at least k staged keys meet it" (the rule is monotone in its
// c2), one counting pass over the staging with a ballot (nn_kth_reached), run only when c2 itself does not meet the rule
// and at least k keys are held.
//
// Staging that survives any density.  kNnStage = 1024 keys per wave, the figure of within.hip and for its reason: 8 KiB
// per wave, 36 KiB per workgroup with the sweep's run tables, four workgroups = 16 waves per CU.  When the next batch of
// 64 candidates might not fit (held + 64 > kNnStage) the staging is sorted, its first k keys are kept, and from then on
// a candidate whose key is above the k-th is rejected (it can never be among the k smallest: the k-th only falls).  With
// k <= 256 a compaction frees at least 1024 - 256 - 64 = 704 slots, so the sweep always goes on: a cell of 2 000
// coincident atoms or a ball of 1 026 costs a few sorts, no global scratch for keys and no quadratic ranking.  After a
// compaction the staging holds the k smallest keys seen and every later candidate not above their k-th, so the k
// smallest keys of the staging stay the k smallest of everything seen.
//
// Resources (compiler's report): k_nearest 83 VGPRs, 36 864 bytes of LDS, 4 waves per SIMD = 16 per CU (the LDS sets
// it); k_nearest_gather 14 VGPRs, no LDS, 8 waves per SIMD; no scratch in either.
// Compiled with -ffp-contract=off: d2 is not fused (the definition is the model's plain float32 arithmetic).
#include "entry_checks.h"
#include "within_keys.h"

namespace rsasa {
namespace {

constexpr uint32_t kNnStage = 1024;  // keys a wave stages in LDS between compactions
static_assert(kNearestMaxK + 2u * kWave <= kNnStage, "a compaction must leave room for the next batches of 64");

// Whether at least k of the wave's `held` staged keys have a d2 that meets the stop rule after shell s: then so does the
// k-th smallest.  The same answer in every lane.
__device__ __forceinline__ bool nn_kth_reached(const unsigned long long *s_key, uint32_t held, uint32_t k, bool margins,
                                               uint32_t s, float h)
{
    const uint32_t lane = lane_id();
    wave_lds_fence();  // (the keys other lanes staged)
    uint32_t n = 0;
    for (uint32_t i0 = 0; i0 < held; i0 += kWave) {
        const uint32_t i = i0 + lane;
        const bool in = i < held && sh_cutoff_reached(margins, s, h, __uint_as_float((uint32_t)(s_key[i] >> 32)));
        n += (uint32_t)__popcll(ballot64(in));
        if (n >= k) return true;
    }
    return false;
}

__global__ __launch_bounds__(256) void k_nearest(NnArgs a)
{
    const WnArgs &wa = a.w;
    const BatchView &b = wa.n.b;
    __shared__ uint32_t s_excl[4][kShRuns], s_start[4][kShRuns];
    __shared__ unsigned long long s_key[4][kNnStage];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= b.n_atoms) return;
    const uint32_t orig = b.sorted_orig[p];
    if ((wa.sorted_flags[p] & 2u) == 0u) {  // no centre (the same in every lane)
        if (lane == 0) wa.n.counts[orig] = 0u;
        return;
    }
    const ShFrame fr = sh_frame(b, p);
    WnAtom at;
    at.orig = orig;
    at.c2 = wa.cutoff * wa.cutoff;
    at.upper = false;
    const uint32_t k = a.k;
    unsigned long long *key = s_key[w];

    uint32_t held = 0;                  // keys in the staging
    unsigned long long bound = ~0ull;   // the k-th key at the last compaction: a key above it is no candidate
    sh_sweep(
        b, fr, s_excl[w], s_start[w],
        [&](bool in, uint32_t q) {
            if (held + kWave > kNnStage) {  // the next 64 might not fit: keep the k smallest (held > k here)
                wn_sort(key, held);
                held = k;
                bound = key[k - 1u];
            }
            bool acc = false;
            float d2 = 0.0f;
            uint32_t orig_q = 0;
            if (in) acc = wn_accept(wa, fr, at, q, true, d2, orig_q);
            const unsigned long long cand = ((unsigned long long)__float_as_uint(d2) << 32) | (orig_q - fr.g.atom_begin);
            acc = acc && cand <= bound;
            const unsigned long long m = ballot64(acc);
            if (acc) key[held + mbcnt64(m)] = cand;
            held += (uint32_t)__popcll(m);
        },
        [&](uint32_t s, bool last) {
            if (last) return true;  // (no count over the staging after the last shell)
            if (sh_cutoff_reached(fr.margins, s, fr.g.cell_size, at.c2)) return true;
            return fr.margins && s >= 1u && held >= k && nn_kth_reached(key, held, k, fr.margins, s, fr.g.cell_size);
        });
    wn_sort(key, held);
    const uint32_t n = min(held, k);
    unsigned long long *row = a.rows + (unsigned long long)(a.rank ? a.rank[orig] : orig) * k;
    for (uint32_t i = lane; i < n; i += kWave) row[i] = key[i];
    if (lane == 0) wa.n.counts[orig] = n;
}

__global__ __launch_bounds__(256) void k_nearest_gather(NnArgs a)
{
    const NbArgs &nb = a.w.n;
    const uint32_t lane = lane_id();
    const uint32_t i = blockIdx.x * 4u + threadIdx.x / kWave;
    if (i >= nb.b.n_atoms) return;
    const uint32_t count = nb.counts[i];
    if (count == 0u) return;  // (no centre, or nobody to list)
    const unsigned long long off = nb.offsets[i];
    const unsigned long long room = nb.offsets[i + 1] - off;
    if ((count > a.k || count != room) && lane == 0) atomicOr(&nb.info->mismatch, 1ull);
    const uint32_t n = (uint32_t)min((unsigned long long)min(count, a.k), room);
    const unsigned long long *row = a.rows + (unsigned long long)(a.rank ? a.rank[i] : i) * a.k;
    for (uint32_t j = lane; j < n; j += kWave) {
        const unsigned long long key = row[j];
        nb.out[off + j] = make_uint2((uint32_t)(key >> 32), (uint32_t)key);
    }
}

}  // namespace

// the rows and counts[] of every input atom, then offsets[] and NbInfo, on the grid of a binned batch with sorted flags
void launch_nearest(const NnArgs &a, hipStream_t stream)
{
    const uint32_t n = a.w.n.b.n_atoms;
    if (!n) return;
    hipLaunchKernelGGL(k_nearest, dim3(cdiv(n, 4)), dim3(256), 0, stream, a);
    launch_neighbor_scan(a.w.n, stream);
}

// the entries (out[]) from the rows
void launch_nearest_gather(const NnArgs &a, hipStream_t stream)
{
    const uint32_t n = a.w.n.b.n_atoms;
    if (!n) return;
    hipLaunchKernelGGL(k_nearest_gather, dim3(cdiv(n, 4)), dim3(256), 0, stream, a);
}

}  // namespace rsasa
