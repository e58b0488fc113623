// Dot-patch kernels (rsasa_dot_patches*, gfx950 only): geodesic farthest-point sampling of every structure's accessible
// dots along the graph of geodesics.hip - repeatedly the dot farthest from the centres chosen so far becomes a centre.
// The lists are those of k_dot_link<kWeights> (bits of sqrtf(d2), batch-wide dot), dist and stamp those of the geodesics;
// the definition: include/rustsasa_amd.h.
//
//   k_patch_init     one lane per dot: dist = +inf, stamp = 0, source = none; the fill's cursors are checked here, as
//                    k_geo_init checks them.
//   k_patch_sample   ONE workgroup of kPsBlock lanes per structure runs all picks of that structure in one launch:
//       pick         an argmax over the structure's dist with the key (bits(dist) << 32) | ~dot, the maximum wins: every
//                    value is >= +0, so the bits order like the numbers, and of equal values the smallest dot has the
//                    largest key.  Lanes stride over the dots, a wave reduces by shuffles, the four waves through LDS.
//                    Sampling stops when the structure has its min(max_centres, D_s) centres or the maximum m is finite
//                    and m <= spacing (float32 compare); otherwise the dot is centre k, cover[k] = m, dist = 0.
//       relaxation   starts from the dist of the previous pick - exact, see below - with the new centre alone in an LDS
//                    queue.  A step: the dots lowered in the previous step (the queue, kPsFan lanes a dot over its list)
//                    push fl(dist[u] + w) to their neighbours with the unsigned atomicMin of k_geo_relax; a push that
//                    lowers dist[v] stamps v with the step's number, and the first to stamp v in a step appends it to
//                    the next queue.  A pick ends with the step that lowers nothing.
//       overflow     a step that lowers more than kPsQueue dots cannot queue them all: the rest of that pick runs on the
//                    stamps alone, k_geo_relax's rule - in step t every dot with stamp >= t - 1 pushes, one lane a dot
//                    over all D_s dots.  Counted (PsStats::overflows); the next pick queues again.
//   k_patch_pack     one workgroup per structure moves its centres and covers from their room of the bound
//                    (min(max_centres, D_s) slots) to where the host's scan of the counts puts them: K entries come
//                    back, not the whole bound.
//   (k_geo_restamp, k_geo_source of geodesics.hip then spread source from the centres, which k_patch_sample marked.)
//
// Why the previous dist is a valid start.  After the picks S the array holds the least solution for the seeds S.  With
// dist[c] = 0 every stored value is still the length of a real path from a seed of S + {c}, so no value lies below the
// least solution for S + {c}; the only edges that can lower anything leave c, which is queued, and from then on the
// invariant of geodesics.hip holds: an edge (u, v) with fl(dist[u] + w) < dist[v] has u in the queue (or stamped in the
// previous step).  A step that lowers nothing leaves a solution reached from above through a monotone map: the least
// one, bit for bit what a relaxation from scratch with all the seeds gives, whatever the schedule.
//
// Visibility.  A structure's dist and stamp are read and written by its one workgroup only, through relaxed agent-scope
// atomic loads, stores and read-modify-writes: they are served by the L2 of the workgroup's XCD, never by the CU's L1
// (which an atomic of another wave does not refresh), and ps_sync() - every wave drains its memory operations, then the barrier - orders the waves' accesses between steps.  The
// lists, offsets and cleared arrays come from earlier launches; the outputs are read by later ones or by the host.
// Every loop is bounded: a pick takes at most D_s + 1 steps (a path has fewer edges than there are dots, and one step finds
// nothing), a structure at most min(max_centres, D_s) picks, the step numbers stay below 2^32; a structure that exceeds a
// bound raises PsStats::error and leaves, and the host answers RSASA_ERR_INTERNAL.  One launch, one wait, no polling.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   kernel                 VGPRs  SGPRs  LDS (bytes)  scratch
//   k_patch_init              10     16            0        0
//   k_patch_sample            42     95         8232        0     (2 x 4 KiB of queue; eight workgroups of four waves per CU)
//   k_patch_pack              11     26            0        0
// Compiled with -ffp-contract=off (dist + w is one float32 addition, as in geodesics.hip).
#include "device_utils.h"

namespace rsasa {
namespace {

constexpr uint32_t kInfBits = 0x7F800000u;
constexpr uint32_t kNoSource = 0xFFFFFFFFu;
constexpr uint32_t kPsFan = 8;          // lanes that share the list of one queued dot
constexpr uint32_t kPsStepMax = 0xFFFFFFF0u;  // the step numbers (stamps) stay below this

__device__ __forceinline__ uint32_t ps_load(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void ps_store(uint32_t *p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t ps_exchange(uint32_t *p, uint32_t v)
{
    return __hip_atomic_exchange(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_patch_init(PsArgs ps)
{
    const GdArgs &gd = ps.g;
    const unsigned long long d = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (d >= gd.c.n_dots) return;
    if (gd.cursor[d] != (uint32_t)(gd.link_offsets[d + 1ull] - gd.link_offsets[d])) atomicOr(&gd.info->mismatch, 1ull);
    gd.dist[d] = kInfBits;
    gd.stamp[d] = 0u;
    if (gd.source) gd.source[d] = kNoSource;
}

// The pushes of dot u (batch-wide) in step `step`: this lane takes entries first, first + stride, ... of u's list.  A
// dot it lowers is stamped; the first stamp of the step counts the dot into *n_next and, while there is room, queues its
// number within the structure.  Targets outside the structure [base, base + n) name no dot of it (an entry that a
// failed fill left unwritten) and are skipped.
__device__ __forceinline__ void ps_push(const GdArgs &gd, uint32_t u, uint32_t first, uint32_t stride, uint32_t base, uint32_t n,
                                        uint32_t step, uint32_t *q_next, uint32_t *n_next)
{
    const float du = __uint_as_float(ps_load(gd.dist + u));
    const unsigned long long e1 = gd.link_offsets[u + 1u];
    for (unsigned long long e = gd.link_offsets[u] + first; e < e1; e += stride) {
        const uint2 en = gd.raw[e];
        const uint32_t v = en.y - base;
        if (v >= n) continue;
        const uint32_t nb = __float_as_uint(du + __uint_as_float(en.x));
        if (nb < ps_load(gd.dist + en.y) && nb < atomicMin(gd.dist + en.y, nb)) {
            if (ps_exchange(gd.stamp + en.y, step) != step) {
                const uint32_t at = atomicAdd(n_next, 1u);
                if (at < kPsQueue) q_next[at] = v;
            }
        }
    }
}

// The barrier between two phases of a workgroup: every wave first waits for its own loads, stores and atomics to be
// acknowledged, so what it did to dist, stamp and the outputs is done before another wave goes on.
__device__ __forceinline__ void ps_sync()
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

__global__ __launch_bounds__(kPsBlock) void k_patch_sample(PsArgs ps)
{
    const GdArgs &gd = ps.g;
    __shared__ uint32_t s_queue[2][kPsQueue];    // the dots (numbers within the structure) lowered in the previous / this step
    __shared__ uint32_t s_count[2];              // how many each step lowered: may exceed kPsQueue, the queue then holds the first
    __shared__ unsigned long long s_best[kPsBlock / kWave];
    const uint32_t s = blockIdx.x, tid = threadIdx.x, lane = lane_id(), w = tid / kWave;
    if (s >= ps.n_structures) return;
    const uint32_t base = (uint32_t)gd.c.dot_offsets[ps.so[s]];            // the structure's first dot
    const uint32_t n = (uint32_t)gd.c.dot_offsets[ps.so[s + 1u]] - base;   // D_s
    const uint32_t k_max = min(ps.max_centres, n);
    const unsigned long long slot = ps.slot_offsets[s];
    uint32_t step = 0, k = 0;                    // the same in every lane, as is all control flow below
    unsigned long long n_steps = 0, n_over = 0;
    bool lost = false;

    for (; k < k_max; k++) {
        // ---- the farthest dot
        unsigned long long key = 0ull;
        for (uint32_t v = tid; v < n; v += kPsBlock)
            key = max(key, ((unsigned long long)ps_load(gd.dist + base + v) << 32) | (uint32_t)~v);
        for (int h = kWave / 2; h >= 1; h >>= 1) {
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), h, kWave);
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, h, kWave);
            key = max(key, ((unsigned long long)hi << 32) | lo);
        }
        if (lane == 0u) s_best[w] = key;
        ps_sync();
#pragma unroll
        for (uint32_t i = 0; i < kPsBlock / kWave; i++) key = max(key, s_best[i]);
        const uint32_t m = (uint32_t)(key >> 32), c = ~(uint32_t)key;
        if (m != kInfBits && __uint_as_float(m) <= ps.spacing) break;
        if (c >= n || step >= kPsStepMax) {  // (c: no value is a NaN or negative, so the key of a dot of the structure won)
            lost = true;
            break;
        }
        step++;
        if (tid == 0u) {
            ps.centres[slot + k] = c;
            ps.cover[slot + k] = m;
            if (gd.source) gd.source[base + c] = c;
            ps_exchange(gd.dist + base + c, 0u);
            ps_store(gd.stamp + base + c, step);
            s_queue[0][0] = c;
            s_count[0] = 1u;
            s_count[1] = 0u;
        }
        // ---- the relaxation from the new centre
        uint32_t cur = 0, steps = 0;
        bool scan = false;
        ps_sync();
        for (;;) {
            const uint32_t qn = s_count[cur];
            if (qn == 0u) break;             // the last step lowered nothing
            if (qn > kPsQueue && !scan) {
                scan = true;
                n_over++;
            }
            if (++steps > n + 1u || step >= kPsStepMax) {
                lost = true;
                break;
            }
            step++;
            if (scan) {
                for (uint32_t u = tid; u < n; u += kPsBlock)
                    if (ps_load(gd.stamp + base + u) >= step - 1u)
                        ps_push(gd, base + u, 0u, 1u, base, n, step, s_queue[cur ^ 1u], &s_count[cur ^ 1u]);
            } else {
                for (uint32_t i = tid / kPsFan; i < qn; i += kPsBlock / kPsFan)
                    ps_push(gd, base + s_queue[cur][i], tid % kPsFan, kPsFan, base, n, step, s_queue[cur ^ 1u], &s_count[cur ^ 1u]);
            }
            ps_sync();                 // (every lane has read s_count[cur] and pushed)
            if (tid == 0u) s_count[cur] = 0u;
            cur ^= 1u;
            ps_sync();
        }
        n_steps += steps;
        if (lost) break;
    }
    if (tid == 0u) {
        ps.n_centres[s] = k;
        atomicAdd(&ps.stats->picks, (unsigned long long)k);
        atomicAdd(&ps.stats->steps, n_steps);
        atomicAdd(&ps.stats->overflows, n_over);
        if (lost) atomicOr(&ps.stats->error, 1ull);
    }
}

// One workgroup per structure: its centres and covers from their room of the bound to their place in the packed arrays.
__global__ __launch_bounds__(256) void k_patch_pack(PsArgs ps)
{
    const uint32_t s = blockIdx.x;
    if (s >= ps.n_structures) return;
    const unsigned long long from = ps.slot_offsets[s], to = ps.centre_offsets[s];
    const unsigned long long room = ps.slot_offsets[s + 1u] - from;
    const unsigned long long k_end = min((unsigned long long)ps.n_centres[s], min(room, ps.centre_offsets[s + 1u] - to));
    for (unsigned long long k = threadIdx.x; k < k_end; k += 256ull) {
        ps.packed_centres[to + k] = ps.centres[from + k];
        ps.packed_cover[to + k] = ps.cover[from + k];
    }
}

}  // namespace

void launch_patch_sample(const PsArgs &ps, hipStream_t stream)
{
    if (!ps.g.c.n_dots || !ps.n_structures) return;
    hipLaunchKernelGGL(k_patch_init, dim3((uint32_t)((ps.g.c.n_dots + 255ull) / 256ull)), dim3(256), 0, stream, ps);
    hipLaunchKernelGGL(k_patch_sample, dim3(ps.n_structures), dim3(kPsBlock), 0, stream, ps);
}

void launch_patch_pack(const PsArgs &ps, hipStream_t stream)
{
    if (!ps.n_structures) return;
    hipLaunchKernelGGL(k_patch_pack, dim3(ps.n_structures), dim3(256), 0, stream, ps);
}

}  // namespace rsasa
