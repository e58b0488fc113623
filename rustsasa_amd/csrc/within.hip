// Atoms-within-a-cutoff kernels (rsasa_atoms_within*, gfx950 only): for every centre the LIST of the partners of its own
// structure within a cutoff several cells long - what k_half_sphere (hse.hip) counts, named.  They need the cell grid of a
// binned batch and the flag bytes in cell-sorted order (k_sort_flags of hse.hip), no neighbour lists and no lattice.
//
//   k_within_count   one wave per cell-sorted atom i over the shell sweep of shell_sweep.h; a wave whose atom is no centre
//                    writes 0 and returns.  Lanes go over the atoms of a step's runs, 64 at a time, and the wave adds the
//                    popcounts of the ballots of wn_accept -> counts[input atom].  The scan of neighbors.hip
//                    (launch_neighbor_scan) then gives offsets and NbInfo, with NbArgs::stage = kWnStage as the length
//                    above which a list is counted as long.
//   k_within_fill    the same sweep again (wn_sweep<true>); accepted candidates are staged in LDS as the 64-bit keys
//                    (float bits of d2) << 32 | idx - d2 >= 0 and never NaN in a list, so the bits order like the numbers,
//                    and the key IS the entry (rsasa_within_t: d2 in the low address, idx behind it) -, sorted there by a
//                    bitonic network, and written to out[offset ..) in order, 64 consecutive entries per store.
//   long lists       a list longer than kWnStage (a dense cluster, coincident atoms, a cutoff that covers the structure)
//                    goes to global scratch as NbKey records with thr = d2 and is ranked by k_neighbor_rank_spill
//                    (neighbors.hip: one workgroup per list, 256-key tiles, any length; it writes (bits of thr, idx),
//                    which here is the entry).  Its cost is quadratic in the length; it is the route of the exception.
//
// The count and the fill pass run ONE function, wn_sweep, whose decisions come from ONE rule, wn_accept (within_keys.h,
// with the sort wn_sort: k_nearest of nearest.hip shares both), and which stops by ONE stop rule, sh_cutoff_reached
// (cutoff_sweep.h: the proof that no unseen atom can be accepted carries over from k_half_sphere unchanged, the
// acceptance having the same d2 <= c2; upper_only only removes entries).  A fill that accepted another number than the
// count sets NbInfo::mismatch and the host answers RSASA_ERR_INTERNAL; every write is bounded by the count regardless.
// wn_sweep takes its atom from sh_frame and writes the loops of sh_sweep (shell_sweep.h: the driver and its contract)
// out, and must follow a change there by hand: run by the driver k_within_fill measured 1.1 to 1.2 % slower
// (profiles/sweep_driver_ab.txt).
//
// The staging and the sort.  All-atom lists of proteins are 80-160 long at 8 A, 250-560 at 13 A and 330-810 at 15 A
// (mean - maximum of the fixtures; large proteins sit near the maxima).  kWnStage = 1024 keys per wave holds every one
// of them: 8 KiB per wave, 36 KiB per workgroup of four waves with the sweep's run tables, which leaves four workgroups =
// 16 waves resident per CU (160 KiB of LDS; the registers would allow more) - enough to cover the sweep's load
// latencies, where 2048 keys would leave 8.  k_neighbor_fill ranks by counting: K^2 / 64 compares per lane, 6 000 at
// K = 600, more than the sweep that found the entries.  Here the list is padded with all-ones keys to P, the power of two
// at or above its length (so a list of 90 sorts 128 keys, not 1024), and sorted by the bitonic network of
// log2 P (log2 P + 1) / 2 stages of P / 2 compare-exchanges: 8 per lane and stage at P = 1024, 440 in all, 180 at
// P = 512, 21 at P = 128.  A compare-exchange is two 8-byte LDS reads and, when it swaps, two writes; the wave runs the
// stages in lockstep with a wave-level fence between them (no workgroup barrier: the four waves sort four lists).  Keys
// are distinct (idx is), so the network's instability cannot show.
//
// Resources (compiler's report): k_within_count 64 VGPRs, 4 096 bytes of LDS, 8 waves per SIMD; k_within_fill 83 VGPRs,
// 36 864 bytes of LDS, 4 waves per SIMD = 16 per CU (the LDS sets it); no scratch in either.
// Compiled with -ffp-contract=off: d2 is not fused (the definition is the model's plain float32 arithmetic).
#include "within_keys.h"

namespace rsasa {
namespace {

constexpr uint32_t kWnStage = 1024;  // keys a wave stages and sorts in LDS; longer lists go through global scratch

// THE sweep of the centre at cell-sorted position p (input index orig), used by both passes; returns the number of
// atoms accepted (the same in every lane).  FILL: the accepted atoms' keys go, in the order the sweep meets them, to
// slots 0 .. K - 1 of s_key (LDS) or, when `spill`, of g_key (global); an atom past slot K - 1 is counted and not written.
template <bool FILL>
__device__ __forceinline__ uint32_t wn_sweep(const WnArgs &a, uint32_t p, uint32_t orig, uint32_t *s_excl, uint32_t *s_start,
                                             uint32_t K, bool spill, unsigned long long *s_key, NbKey *g_key)
{
    const BatchView &b = a.n.b;
    const uint32_t lane = lane_id();
    const ShFrame fr = sh_frame(b, p);
    WnAtom at;
    at.orig = orig;
    at.c2 = a.cutoff * a.cutoff;
    at.upper = a.upper_only != 0u;
    const bool want_orig = FILL || at.upper;

    uint32_t k = 0;
    for (uint32_t s = 0;; s++) {
        const ShShell shell = sh_shell(fr.g, fr.cell, s);
        for (unsigned long long r0 = 0; r0 < shell.n_rows; r0 += kWave) {
            const uint32_t total = sh_step_runs(b, fr.g, fr.cell, shell, s, r0, s_excl, s_start);
            for (uint32_t f0 = 0; f0 < total; f0 += kWave) {
                const uint32_t f = f0 + lane;
                bool acc = false;
                float d2 = 0.0f;
                uint32_t orig_q = 0;
                if (f < total) acc = wn_accept(a, fr, at, sh_pos(s_excl, s_start, f), want_orig, d2, orig_q);
                const unsigned long long m = ballot64(acc);
                if (FILL) {
                    const uint32_t slot = k + mbcnt64(m);
                    if (acc && slot < K) {
                        const unsigned long long key =
                            ((unsigned long long)__float_as_uint(d2) << 32) | (orig_q - fr.g.atom_begin);
                        if (spill) {
                            NbKey e;
                            e.key = key;
                            e.thr = d2;  // (k_neighbor_rank_spill writes thr's bits in front of idx)
                            e.pad = 0;
                            g_key[slot] = e;
                        } else {
                            s_key[slot] = key;
                        }
                    }
                }
                k += (uint32_t)__popcll(m);
            }
        }
        if (s >= fr.cell.s_last) break;  // the shells cover the grid
        if (sh_cutoff_reached(fr.margins, s, fr.g.cell_size, at.c2)) break;
    }
    return k;
}

__global__ __launch_bounds__(256) void k_within_count(WnArgs a)
{
    const BatchView &b = a.n.b;
    __shared__ uint32_t s_excl[4][kShRuns], s_start[4][kShRuns];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= b.n_atoms) return;
    const uint32_t orig = b.sorted_orig[p];
    if ((a.sorted_flags[p] & 2u) == 0u) {  // no centre (the same in every lane)
        if (lane == 0) a.n.counts[orig] = 0u;
        return;
    }
    const uint32_t k = wn_sweep<false>(a, p, orig, s_excl[w], s_start[w], 0u, false, nullptr, nullptr);
    if (lane == 0) a.n.counts[orig] = k;
}

__global__ __launch_bounds__(256) void k_within_fill(WnArgs a)
{
    const BatchView &b = a.n.b;
    __shared__ uint32_t s_excl[4][kShRuns], s_start[4][kShRuns];
    __shared__ unsigned long long s_key[4][kWnStage];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= b.n_atoms) return;
    const uint32_t orig = b.sorted_orig[p];
    const unsigned long long off = a.n.offsets[orig];
    const uint32_t K = (uint32_t)(a.n.offsets[orig + 1] - off);
    if (K == 0) return;  // (no centre, or nobody within the cutoff)
    const bool spill = K > kWnStage;
    unsigned long long sbase = 0;
    if (spill) {
        if (lane == 0) {
            sbase = atomicAdd(&a.n.info->spill_cursor, (unsigned long long)K);
            const unsigned long long r = atomicAdd(&a.n.info->spill_recs, 1ull);
            NbSpillRec rec;
            rec.off = off;
            rec.base = sbase;
            rec.k = K;
            rec.pad = 0;
            a.n.spill_recs[r] = rec;
        }
        sbase = __shfl(sbase, 0, kWave);
    }
    const uint32_t k = wn_sweep<true>(a, p, orig, s_excl[w], s_start[w], K, spill, s_key[w], spill ? a.n.spill + sbase : nullptr);
    if (k != K && lane == 0) atomicOr(&a.n.info->mismatch, 1ull);
    if (spill) return;
    const uint32_t n = min(k, K);
    wn_sort(s_key[w], n);
    for (uint32_t i = lane; i < n; i += kWave) {
        const unsigned long long key = s_key[w][i];
        a.n.out[off + i] = make_uint2((uint32_t)(key >> 32), (uint32_t)key);
    }
}

}  // namespace

// counts[] of every input atom, then offsets[] and NbInfo, on the grid of a binned batch with sorted flags
void launch_within_count(const WnArgs &w, hipStream_t stream)
{
    const uint32_t n = w.n.b.n_atoms;
    if (!n) return;
    hipLaunchKernelGGL(k_within_count, dim3(cdiv(n, 4)), dim3(256), 0, stream, w);
    launch_neighbor_scan(w.n, stream);
}

// the entries (out[]); `spill_atoms` lists are longer than the LDS staging (NbInfo::spill_atoms)
void launch_within_fill(const WnArgs &w, uint64_t spill_atoms, hipStream_t stream)
{
    const uint32_t n = w.n.b.n_atoms;
    if (!n) return;
    hipLaunchKernelGGL(k_within_fill, dim3(cdiv(n, 4)), dim3(256), 0, stream, w);
    launch_neighbor_rank_spill(w.n, spill_atoms, stream);
}

uint32_t within_stage_capacity() { return kWnStage; }

}  // namespace rsasa
