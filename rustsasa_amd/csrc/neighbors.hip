// Neighbour-list kernels (rsasa_precompute_neighbors*, gfx950 only): the lists of precompute_neighbors
// (reference src/lib.rs:69-84; SpatialGrid::build_all_neighbor_lists, spatial_grid.rs:195-465) from the cell grid the
// SASA path builds (launch_grid_prepare / launch_sort_lds / launch_sort_tail, with BatchView::max_r_override).
//
//   k_neighbor_count       one wave per cell-sorted atom: sweep of the 25 x-runs of its 5x5x5 cell block (as in
//                          occlusion_v0.inc), lanes over candidates, ballot popcount -> counts[input atom]
//   k_nb_scan_*            64-bit exclusive scan of the counts -> offsets; totals, the longest list and the lists
//                          too long for the LDS staging -> NbInfo (the host sizes its buffers from it)
//   k_neighbor_fill        the same sweep again; accepted candidates are staged as 64-bit keys
//                          (float bits of d^2) << 32 | idx - d^2 >= 0 and never NaN in a list, so the bits order like
//                          the numbers - and each lane writes its entries at out[offset + rank], rank = number of
//                          smaller keys: the list comes out sorted by (d^2, idx) without a sort pass
//   k_neighbor_rank_spill  lists longer than the staging (clusters of coincident atoms): keys in global scratch,
//                          one workgroup per list
//
// The count and the fill pass take their decisions from ONE function (nb_accept): a list the fill pass saw longer
// than its count would run into its neighbour's entries (every write is bounded by the count regardless).
// Compiled with -ffp-contract=off: d^2 = dx*dx + dy*dy + dz*dz is not fused, as in the reference.
#include "device_utils.h"

#include <algorithm>

namespace rsasa {
namespace {

constexpr uint32_t kNbStage = 512;       // keys a wave stages in LDS (lists are ~44 long at probe 1.4)
constexpr uint32_t kNbScanBlocks = 1024;  // workgroups of the count scan

// The 25 x-runs of cells around the atom at cell-sorted position p (search extent 2, spatial_grid.rs:47), their
// exclusive prefix sums and starts in s_excl / s_start (32 entries, one wave); returns the candidates in all runs.
__device__ __forceinline__ uint32_t nb_runs(const BatchView &b, const StructGrid &g, const float4 me, uint32_t *s_excl,
                                            uint32_t *s_start)
{
    const uint32_t lane = lane_id();
    uint32_t cx, cy, cz;
    cell_coords(g, me.x, me.y, me.z, cx, cy, cz);
    uint32_t run_start = 0, run_len = 0;
    if (lane < 25) {
        const int yy = (int)cy + (int)(lane % 5u) - 2;
        const int zz = (int)cz + (int)(lane / 5u) - 2;
        if (yy >= 0 && yy < (int)g.dim_y && zz >= 0 && zz < (int)g.dim_z) {
            const uint32_t x0 = cx >= 2u ? cx - 2u : 0u;
            const uint32_t x1 = min(cx + 2u, g.dim_x - 1u);
            const uint32_t c0 = g.cell_base + x0 + (uint32_t)yy * g.dim_x + (uint32_t)zz * g.dim_x * g.dim_y;
            const bool rel16 = g.in_lds != 0u;
            const uint32_t first = load_cell_start(b.cells, c0, rel16);
            run_len = load_cell_start(b.cells, c0 + (x1 - x0) + 1u, rel16) - first;
            run_start = (rel16 ? g.sorted_base : 0u) + first;
        }
    }
    const uint32_t run_incl = wave_incl_scan(run_len);
    if (lane < 32) {
        s_excl[lane] = lane < 25 ? run_incl - run_len : 0xFFFFFFFFu;
        s_start[lane] = run_start;
    }
    wave_lds_fence();
    return wave_bcast(run_incl, 31);
}

// Flat position f of the concatenated runs -> cell-sorted position.
__device__ __forceinline__ uint32_t nb_pos(const uint32_t *s_excl, const uint32_t *s_start, uint32_t f)
{
    uint32_t lo = 0;
#pragma unroll
    for (int step = 16; step > 0; step >>= 1)
        if (s_excl[lo + step] <= f) lo += step;
    return s_start[lo] + (f - s_excl[lo]);
}

// One atom's side of the rule.
struct NbAtom {
    float4 me;
    float ms2;       // max_search_radius^2 (spatial_grid.rs:219-220)
    float sr2;       // (r_i + max_r + 2p)^2 (spatial_grid.rs:307-308)
    uint32_t id32;
    uint64_t id;
};

template <bool HAS_ID>
__device__ __forceinline__ NbAtom nb_atom(const BatchView &b, const StructGrid &g, uint32_t p)
{
    NbAtom at;
    at.me = b.sorted_xyzr[p];
    const float ms = g.max_r + g.max_r + 2.0f * b.probe;   // spatial_grid.rs:219
    at.ms2 = ms * ms;                                      // spatial_grid.rs:220
    const float sr = at.me.w + g.max_r + 2.0f * b.probe;   // spatial_grid.rs:307
    at.sr2 = sr * sr;                                      // spatial_grid.rs:308
    at.id32 = 0;
    at.id = 0;
    if (HAS_ID) {
        at.id32 = b.sorted_id32[p];
        at.id = b.id[b.sorted_orig[p]];
    }
    return at;
}

// THE acceptance rule (spatial_grid.rs:300-341), used by both passes: candidate q is in the list of atom p when it is
// another atom, its id differs (equal 32-bit folds are decided on the 64-bit ids), and d^2 passes both distance tests.
// d2 is the reference's sort key as well (spatial_grid.rs:452-462: centre minus neighbour, squared).
template <bool HAS_ID>
__device__ __forceinline__ bool nb_accept(const BatchView &b, const NbAtom &at, uint32_t p, uint32_t q, const float4 o,
                                          float &d2)
{
    const float dx = at.me.x - o.x, dy = at.me.y - o.y, dz = at.me.z - o.z;
    d2 = dx * dx + dy * dy + dz * dz;                         // spatial_grid.rs:321
    bool ok = q != p && d2 <= at.ms2 && d2 <= at.sr2;        // spatial_grid.rs:324-335
    if (HAS_ID && ok && b.sorted_id32[q] == at.id32) ok = b.id[b.sorted_orig[q]] != at.id;  // spatial_grid.rs:314
    return ok;
}

template <bool HAS_ID>
__global__ __launch_bounds__(256) void k_neighbor_count(NbArgs a)
{
    const BatchView &b = a.b;
    __shared__ uint32_t s_excl[4][32], s_start[4][32];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= b.n_atoms) return;
    const StructGrid g = b.grids[b.sid_sorted[p]];
    const NbAtom at = nb_atom<HAS_ID>(b, g, p);
    const uint32_t total = nb_runs(b, g, at.me, s_excl[w], s_start[w]);
    uint32_t k = 0;
    for (uint32_t base = 0; base < total; base += kWave) {
        const uint32_t f = base + lane;
        bool acc = false;
        if (f < total) {
            const uint32_t q = nb_pos(s_excl[w], s_start[w], f);
            float d2;
            acc = nb_accept<HAS_ID>(b, at, p, q, b.sorted_xyzr[q], d2);
        }
        k += (uint32_t)__popcll(ballot64(acc));
    }
    if (lane == 0) a.counts[b.sorted_orig[p]] = k;
}

// ---- 64-bit exclusive scan of the counts (the pattern of k_scan_reduce / k_scan_block_sums / k_scan_apply) ----

__device__ __forceinline__ void nb_scan_range(uint32_t n, uint32_t &begin, uint32_t &end)
{
    uint32_t chunk = (n + kNbScanBlocks - 1) / kNbScanBlocks;
    chunk = (chunk + 255u) & ~255u;
    const unsigned long long b0 = (unsigned long long)blockIdx.x * chunk;
    begin = (uint32_t)min(b0, (unsigned long long)n);
    end = (uint32_t)min(b0 + chunk, (unsigned long long)n);
}

// sum, max, and the sum and number of the counts above the run's staging, NbArgs::stage (parts[4 * block ..])
__global__ __launch_bounds__(256) void k_nb_scan_reduce(NbArgs a)
{
    __shared__ unsigned long long smem[4][4];
    uint32_t begin, end;
    nb_scan_range(a.b.n_atoms, begin, end);
    unsigned long long sum = 0, mx = 0, se = 0, sn = 0;
    for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
        const uint32_t c = a.counts[i];
        sum += c;
        mx = max(mx, (unsigned long long)c);
        if (c > a.stage) { se += c; sn++; }
    }
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        sum += __shfl_xor(sum, d, kWave);
        mx = max(mx, __shfl_xor(mx, d, kWave));
        se += __shfl_xor(se, d, kWave);
        sn += __shfl_xor(sn, d, kWave);
    }
    const uint32_t w = threadIdx.x / kWave;
    if (lane_id() == 0) { smem[w][0] = sum; smem[w][1] = mx; smem[w][2] = se; smem[w][3] = sn; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const uint32_t k = threadIdx.x;
        unsigned long long v = smem[0][k];
        for (int i = 1; i < 4; i++) v = k == 1 ? max(v, smem[i][k]) : v + smem[i][k];
        a.parts[4 * blockIdx.x + k] = v;
    }
}

// one workgroup of kNbScanBlocks threads: the parts' sums become exclusive prefixes; totals -> NbInfo, offsets[n]
__global__ __launch_bounds__(kNbScanBlocks) void k_nb_scan_parts(NbArgs a)
{
    constexpr int NW = kNbScanBlocks / kWave;
    __shared__ unsigned long long s_sum[NW], s_max[NW], s_se[NW], s_sn[NW];
    const uint32_t t = threadIdx.x, w = t / kWave, lane = lane_id();
    const unsigned long long v = a.parts[4 * t], vmax = a.parts[4 * t + 1];
    unsigned long long se = a.parts[4 * t + 2], sn = a.parts[4 * t + 3], mx = vmax;
    const unsigned long long inc = wave_incl_scan(v);
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        mx = max(mx, __shfl_xor(mx, d, kWave));
        se += __shfl_xor(se, d, kWave);
        sn += __shfl_xor(sn, d, kWave);
    }
    if (lane == kWave - 1) s_sum[w] = inc;
    if (lane == 0) { s_max[w] = mx; s_se[w] = se; s_sn[w] = sn; }
    __syncthreads();
    unsigned long long before = 0, total = 0, gmax = 0, gse = 0, gsn = 0;
    for (int i = 0; i < NW; i++) {
        if ((uint32_t)i < w) before += s_sum[i];
        total += s_sum[i];
        gmax = max(gmax, s_max[i]);
        gse += s_se[i];
        gsn += s_sn[i];
    }
    a.parts[4 * t] = before + inc - v;
    if (t == 0) {
        a.info->total = total;
        a.info->max_k = gmax;
        a.info->spill_entries = gse;
        a.info->spill_atoms = gsn;
        a.offsets[a.b.n_atoms] = total;
    }
}

__global__ __launch_bounds__(256) void k_nb_scan_apply(NbArgs a)
{
    __shared__ unsigned long long smem[4];
    uint32_t begin, end;
    nb_scan_range(a.b.n_atoms, begin, end);
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    unsigned long long running = a.parts[4 * blockIdx.x];
    for (uint32_t tile = begin; tile < end; tile += 256) {
        const uint32_t i = tile + threadIdx.x;
        const unsigned long long v = i < end ? a.counts[i] : 0ull;
        const unsigned long long inc = wave_incl_scan(v);
        __syncthreads();
        if (lane == kWave - 1) smem[w] = inc;
        __syncthreads();
        unsigned long long before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if ((uint32_t)k < w) before += smem[k];
            total += smem[k];
        }
        if (i < end) a.offsets[i] = running + before + inc - v;
        running += total;
    }
}

// ---- fill ----

template <bool HAS_ID>
__global__ __launch_bounds__(256) void k_neighbor_fill(NbArgs a)
{
    const BatchView &b = a.b;
    __shared__ uint32_t s_excl[4][32], s_start[4][32];
    __shared__ unsigned long long s_key[4][kNbStage];
    __shared__ float s_thr[4][kNbStage];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + w;
    if (p >= b.n_atoms) return;
    const uint32_t row = b.sorted_orig[p];
    const unsigned long long off = a.offsets[row];
    const uint32_t K = (uint32_t)(a.offsets[row + 1] - off);
    if (K == 0) return;
    const bool spill = K > kNbStage;
    unsigned long long sbase = 0;
    if (spill) {
        if (lane == 0) {
            sbase = atomicAdd(&a.info->spill_cursor, (unsigned long long)K);
            const unsigned long long r = atomicAdd(&a.info->spill_recs, 1ull);
            NbSpillRec rec;
            rec.off = off;
            rec.base = sbase;
            rec.k = K;
            rec.pad = 0;
            a.spill_recs[r] = rec;
        }
        sbase = __shfl(sbase, 0, kWave);
    }
    const StructGrid g = b.grids[b.sid_sorted[p]];
    const NbAtom at = nb_atom<HAS_ID>(b, g, p);
    const uint32_t total = nb_runs(b, g, at.me, s_excl[w], s_start[w]);
    const float probe = b.probe;
    uint32_t k = 0;
    for (uint32_t base = 0; base < total; base += kWave) {
        const uint32_t f = base + lane;
        bool acc = false;
        unsigned long long key = 0;
        float thr = 0.0f;
        if (f < total) {
            const uint32_t q = nb_pos(s_excl[w], s_start[w], f);
            const float4 o = b.sorted_xyzr[q];
            float d2;
            acc = nb_accept<HAS_ID>(b, at, p, q, o, d2);
            if (acc) {
                const uint32_t orig = b.sorted_orig[q];
                const uint32_t idx = a.idx_map ? a.idx_map[orig] : orig - g.atom_begin;
                key = ((unsigned long long)__float_as_uint(d2) << 32) | idx;
                const float tj = o.w + probe;  // spatial_grid.rs:336
                thr = tj * tj;                 // spatial_grid.rs:339
            }
        }
        const unsigned long long m = ballot64(acc);
        const uint32_t slot = k + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (acc && slot < K) {
            if (spill) {
                NbKey e;
                e.key = key;
                e.thr = thr;
                e.pad = 0;
                a.spill[sbase + slot] = e;
            } else {
                s_key[w][slot] = key;
                s_thr[w][slot] = thr;
            }
        }
        k += (uint32_t)__popcll(m);
    }
    if (k != K && lane == 0) atomicOr(&a.info->mismatch, 1ull);
    if (spill) return;
    wave_lds_fence();
    const uint32_t n = min(k, K);
    for (uint32_t i = lane; i < n; i += kWave) {
        const unsigned long long key = s_key[w][i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; j++) rank += s_key[w][j] < key ? 1u : 0u;
        a.out[off + rank] = make_uint2(__float_as_uint(s_thr[w][i]), (uint32_t)key);
    }
}

// The long lists: one workgroup per list, the keys compared in tiles of 256 staged in LDS.
__global__ __launch_bounds__(256) void k_neighbor_rank_spill(NbArgs a, uint32_t n_recs)
{
    __shared__ unsigned long long tile[256];
    for (uint32_t r = blockIdx.x; r < n_recs; r += gridDim.x) {
        const NbSpillRec rec = a.spill_recs[r];
        for (uint32_t i0 = 0; i0 < rec.k; i0 += 256) {
            const uint32_t i = i0 + threadIdx.x;
            NbKey e;
            e.key = 0;
            e.thr = 0.0f;
            if (i < rec.k) e = a.spill[rec.base + i];
            uint32_t rank = 0;
            for (uint32_t j0 = 0; j0 < rec.k; j0 += 256) {
                __syncthreads();
                tile[threadIdx.x] = j0 + threadIdx.x < rec.k ? a.spill[rec.base + j0 + threadIdx.x].key : ~0ull;
                __syncthreads();
                const uint32_t nj = min(256u, rec.k - j0);
                for (uint32_t j = 0; j < nj; j++) rank += tile[j] < e.key ? 1u : 0u;
            }
            if (i < rec.k) a.out[rec.off + rank] = make_uint2(__float_as_uint(e.thr), (uint32_t)e.key);
        }
        __syncthreads();
    }
}

}  // namespace

// counts[] of every input atom, then offsets[] and NbInfo (total, longest list, the long lists' totals)
void launch_neighbor_count(const NbArgs &a, hipStream_t stream)
{
    const uint32_t n = a.b.n_atoms;
    if (!n) return;
    if (a.b.sorted_id32) hipLaunchKernelGGL(k_neighbor_count<true>, dim3(cdiv(n, 4)), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_neighbor_count<false>, dim3(cdiv(n, 4)), dim3(256), 0, stream, a);
    launch_neighbor_scan(a, stream);
}

// offsets[] and NbInfo of counts[] that are already there (the group rows of rsasa_group_contacts* too)
void launch_neighbor_scan(const NbArgs &a, hipStream_t stream)
{
    if (!a.b.n_atoms) return;
    hipLaunchKernelGGL(k_nb_scan_reduce, dim3(kNbScanBlocks), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_nb_scan_parts, dim3(1), dim3(kNbScanBlocks), 0, stream, a);
    hipLaunchKernelGGL(k_nb_scan_apply, dim3(kNbScanBlocks), dim3(256), 0, stream, a);
}

// the entries (out[]); `spill_atoms` lists are longer than the LDS staging (NbInfo::spill_atoms)
void launch_neighbor_fill(const NbArgs &a, uint64_t spill_atoms, hipStream_t stream)
{
    const uint32_t n = a.b.n_atoms;
    if (!n) return;
    if (a.b.sorted_id32) hipLaunchKernelGGL(k_neighbor_fill<true>, dim3(cdiv(n, 4)), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_neighbor_fill<false>, dim3(cdiv(n, 4)), dim3(256), 0, stream, a);
    launch_neighbor_rank_spill(a, spill_atoms, stream);
}

// the entries of the `spill_atoms` lists whose keys the fill kernel left in a.spill (k_within_fill of within.hip too: the
// ranking writes (float bits of NbKey::thr, idx), and that run stores d^2 as thr)
void launch_neighbor_rank_spill(const NbArgs &a, uint64_t spill_atoms, hipStream_t stream)
{
    if (spill_atoms)
        hipLaunchKernelGGL(k_neighbor_rank_spill, dim3((uint32_t)std::min<uint64_t>(spill_atoms, 4096)), dim3(256), 0, stream, a,
                           (uint32_t)spill_atoms);
}

uint32_t neighbor_stage_capacity() { return kNbStage; }

}  // namespace rsasa
