// The general occlusion kernel (k_occlusion_v3): it decides the atoms the other kernels defer,
// and every atom when they do not apply (more points or remainder points than they take, or
// RSASA_OCCLUSION_KERNEL=3).  The stages are described at the top of occlusion.hip.  It is bound
// by VALU + SALU issue (~1.15 ns per wave-instruction and SIMD, tools/microbench_issue.hip), so
// the design choices below are about instruction count:
//   * a dense prologue computes the culled runs of all the wave's atoms, 64 (atom, run) pairs
//     per pass; the per-atom prefix sum uses DPP, not LDS permutes;
//   * the sweep only tests distances and appends the accepted atom's INDEX (4-byte LDS store,
//     exec-masked: LDS stores cost by active lane); the prep pass (lane = candidate) re-gathers
//     the atom, applies the id rule, computes (v, limit) and writes the near-first list once;
//   * survivors are compacted as point indices and re-read from the lattice (float4 records).

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp_zero(uint32_t src)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)src, CTRL, ROW_MASK, 0xf, true);
}

// inclusive prefix sum over lanes 0..31 (each 16-lane row, then row 0 -> row 1)
__device__ __forceinline__ uint32_t scan_lanes32(uint32_t v)
{
    v += dpp_zero<0x111>(v);       // row_shr:1
    v += dpp_zero<0x112>(v);       // row_shr:2
    v += dpp_zero<0x114>(v);       // row_shr:4
    v += dpp_zero<0x118>(v);       // row_shr:8
    v += dpp_zero<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
    return v;
}

constexpr bool kFlatSweep = true;          // flat lane->atom map over the runs (false: 16-atom segments)
constexpr int kSegCap = 64;               // segment-table entries per round
constexpr int kSegLanes = 16;             // atoms per sweep segment (64 / kSegLanes segments per iteration)
constexpr int kSegShift = 4;
constexpr int kMaxAtomsPerWave = 8;        // atoms one wave prepares in its prologue
constexpr int kListCap = 192;              // queued candidate indices per wave
constexpr int kListFlush = kListCap - 64;  // flush once more than this many are queued
constexpr float kNearScale2 = 1.5625f;  // near: d^2 < (1.25 (r_i + p))^2 -- heuristic split only

// Only what the kernel reads: a small argument block keeps the SGPR file free of spills.
struct OccArgs3 {
    const float4 *sorted_xyzr;
    const uint32_t *cells, *sid, *sorted_orig;  // sid: structure of the atom at a cell-sorted position
    const StructGrid *grids;
    const uint64_t *sorted_id;   // null when the batch keeps no sorted copy of the ids (see BatchView::sorted_id):
    const uint64_t *ids_in;      // the id of the atom at position q is then ids_in[sorted_orig[q]]
    const uint32_t *sorted_id32;
    const BatchStatus *status;
    const float *lat_x, *lat_y, *lat_z;
    const float4 *lat4;
    const uint4 *patches;  // Lattice::patches (k_occlusion_mx with more than 128 points)
    float *atom_sasa;
    uint32_t *neighbor_counts;
    uint32_t n_atoms, n_points, n_fused, n_blocks, atoms_per_wave;
    float probe;
    // deferred atoms: written by k_occlusion_fast, consumed by k_occlusion_v3 in list mode
    // (work_list != nullptr: the wave's atoms are work_list[i], i < *work_count, grid-stride)
    uint32_t *work_list_out, *work_count_out;
    const uint32_t *work_list, *work_count;
    uint32_t part;  // OcclusionPart (k_occlusion_fast): all atoms / below / from BatchStatus::tail_atom_base
    uint32_t *defer_flag;  // nullable, pinned host memory: set to 1 by a wave that defers an atom (BatchView::defer_flag)
    uint32_t *claim;       // k_occlusion_mx: this launch's eight block counters (BatchStatus::claim)
    const float *mx_tab;   // k_occlusion_mx, at most 128 points: Lattice::mx_tab
    uint32_t ids_check;    // BatchView::ids_check (k_occlusion_mx): the launch is one of a pair, with and without ids, and
                           // every structure is computed by the one that is its own (the general kernel reads the
                           // caller's ids for its few atoms either way: different ids change nothing)
    const uint32_t *ids_seg;  // BatchView::ids_seg (nullable) and its word count
    uint32_t ids_seg_words;
};

inline OccArgs3 make_args3(const OccArgs &a)
{
    return OccArgs3{a.b.sorted_xyzr, a.b.cells, a.b.sid_sorted, a.b.sorted_orig, a.b.grids, a.b.sorted_id, a.b.id, a.b.sorted_id32,
                    a.b.status, a.lat.x, a.lat.y, a.lat.z, a.lat.xyz4, a.lat.patches, a.b.atom_sasa,
                    a.b.neighbor_counts, a.b.n_atoms, a.lat.n_points, a.lat.n_fused, a.n_blocks,
                    a.atoms_per_wave, a.b.probe, nullptr, nullptr, nullptr, nullptr, 0u, nullptr, nullptr, a.lat.mx_tab, a.b.ids_check,
                    a.b.ids_check ? a.b.ids_seg : nullptr, a.b.ids_seg_words};
}

template <int NCH, bool HAS_ID>
__global__ __launch_bounds__(256) void k_occlusion_v3(OccArgs3 a)
{
    if (batch_aborted(a.status)) return;
    __shared__ float4 s_cand[4][kListCap + 16];  // (vx, vy, vz, limit), near candidates first; +16 padding
    __shared__ uint32_t s_list[4][kListCap + 64];  // accepted atom indices (+ 64 parking slots)
    __shared__ uint2 s_seg[4][kFlatSweep ? 1 : kSegCap + 64 / kSegLanes];
    __shared__ int s_delta[4][32];      // flat sweep: per non-empty run, start - exclusive prefix
    __shared__ uint32_t s_mask[4][8];   // flat sweep: run-start markers of a 256-position window
    __shared__ uint32_t s_pts[4][64];
    __shared__ uint2 s_runs[4][kMaxAtomsPerWave][25];  // (start, length) of every atom's culled x-runs
    __shared__ float s_sr[4][kMaxAtomsPerWave];         // r_i + max_r + 2p per atom

    const float4 *__restrict__ sorted_xyzr = a.sorted_xyzr;
    const uint32_t *__restrict__ cells = a.cells;
    const uint32_t *__restrict__ sid = a.sid;  // (prologue only)
    const StructGrid *__restrict__ grids = a.grids;
    const uint64_t *__restrict__ sorted_id = a.sorted_id;
    const float4 *__restrict__ lat4 = a.lat4;
    const uint32_t n_atoms = a.n_atoms;

    const uint32_t lane = lane_id();
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t bid = blockIdx.x;
    {
        const uint32_t per = a.n_blocks / 8u;
        if (bid < per * 8u) bid = (bid % 8u) * per + bid / 8u;
    }
    const uint32_t apw = a.atoms_per_wave;
    const uint32_t *__restrict__ work_list = a.work_list;
    const bool list_mode = work_list != nullptr;
    if (list_mode) bid = blockIdx.x;
    const uint32_t n_work = list_mode ? *a.work_count : n_atoms;
    uint32_t p_begin = (bid * 4u + w) * apw;
    if (p_begin >= n_work) return;

    const float probe = a.probe;
    const uint32_t n_points = a.n_points;
    const uint32_t n_fused = a.n_fused;
    const uint32_t n_rem = n_points - n_fused;  // < 16
    const uint32_t n_chunks = (n_points + kWave - 1) / kWave;
    const bool counting = a.neighbor_counts != nullptr;
    const float neg_inf = __int_as_float(0xFF800000);

    // ---- per-wave constants -------------------------------------------------
    float sx[NCH], sy[NCH], sz[NCH];
    unsigned long long invalid[NCH];
    auto load_group = [&](uint32_t ch0) {
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const uint32_t pi = (ch0 + c) * kWave + lane;  // lattice arrays are zero padded
            const bool in_range = (ch0 + c) < n_chunks;
            sx[c] = in_range ? a.lat_x[pi] : 0.0f;
            sy[c] = in_range ? a.lat_y[pi] : 0.0f;
            sz[c] = in_range ? a.lat_z[pi] : 0.0f;
            invalid[c] = __ballot(!(in_range && pi < n_fused));
        }
    };
    const bool single_group = n_chunks <= (uint32_t)NCH;
    if (single_group) load_group(0);

    // remainder points: lanes tiled as (point = lane % P, candidate group = lane / P)
    uint32_t rem_shift = 0;
    while ((1u << rem_shift) < n_rem) rem_shift++;
    rem_shift = max(rem_shift, 2u);  // at most 16 candidate groups, so tiles stay inside the padded list
    const uint32_t rem_pt = lane & ((1u << rem_shift) - 1u);
    const uint32_t rem_grp = lane >> rem_shift;
    const uint32_t rem_groups = 64u >> rem_shift;
    float4 rp = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rem_pt < n_rem) rp = lat4[n_fused + rem_pt];
    const unsigned long long rem_low = n_rem ? ((1ull << n_rem) - 1ull) : 0ull;

    const uint32_t seg_sub = lane & (uint32_t)(kSegLanes - 1), seg_grp = lane >> kSegShift;
    const uint32_t dummy_slot = (uint32_t)kListCap + lane;  // where rejected lanes park their store

  for (;;) {  // one pass in direct mode; grid-stride over the deferred list in list mode
    const uint32_t p_end = min(p_begin + apw, n_work);
    // ---- prologue: the culled x-runs of ALL the wave's atoms, 64 (atom, run) pairs per pass ----
    // -- 1. Every atom owns the 25 x-runs of the 5x5x5 cell block around its cell.  With u = f - c
    // the fractional position inside the cell, the gap to row c + d is d - u (d > 0), u - d - 1
    // (d < 0) or 0; a run whose gap exceeds the search radius is dropped, the others are
    // trimmed to the cells that can hold an atom within reach.
    {
        const uint32_t n_mine = p_end - p_begin;
        for (uint32_t idx = lane; idx < n_mine * 25u; idx += 64u) {
            const uint32_t at = (idx * 5243u) >> 17;  // idx / 25 for idx < 2^14
            const uint32_t r = idx - at * 25u;
            const int rdz = (int)((r * 13u) >> 6) - 2;  // r / 5 - 2 for r < 25
            const int rdy = (int)r - (rdz + 2) * 5 - 2;
            const uint32_t pa = list_mode ? work_list[p_begin + at] : p_begin + at;
            const float4 m = sorted_xyzr[pa];
            const StructGrid g = grids[sid[pa]];
            // rounding of f = (x - min) * inv in cell units grows with the grid extent
            const float tol = 8.0f * 1.1920929e-7f * (float)max(max(g.dim_x, g.dim_y), g.dim_z) + 1e-5f;
            const float sr = m.w + g.max_r + 2.0f * probe;  // spatial_grid.rs:307
            const float fx = (m.x - g.min_x) * g.inv_cell;  // spatial_grid.rs:139-141
            const float fy = (m.y - g.min_y) * g.inv_cell;
            const float fz = (m.z - g.min_z) * g.inv_cell;
            const int cx = (int)min((uint32_t)fmaxf(fx, 0.0f), g.dim_x - 1u);
            const int cy = (int)min((uint32_t)fmaxf(fy, 0.0f), g.dim_y - 1u);
            const int cz = (int)min((uint32_t)fmaxf(fz, 0.0f), g.dim_z - 1u);
            const float srn = sr * g.inv_cell;
            const float thr = srn * srn * 1.00001f;
            const float uy = fy - (float)cy, uz = fz - (float)cz;
            float gy = rdy > 0 ? (float)rdy - uy : (rdy < 0 ? uy - (float)(rdy + 1) : 0.0f);
            float gz = rdz > 0 ? (float)rdz - uz : (rdz < 0 ? uz - (float)(rdz + 1) : 0.0f);
            gy = fmaxf(gy - tol, 0.0f);
            gz = fmaxf(gz - tol, 0.0f);
            const float b2 = __builtin_fmaf(-gy, gy, __builtin_fmaf(-gz, gz, thr));
            const uint32_t yy = (uint32_t)(cy + rdy), zz = (uint32_t)(cz + rdz);
            uint32_t run_start = 0, run_len = 0;
            if (yy < g.dim_y && zz < g.dim_z && b2 >= 0.0f) {
                // cells of the row that can hold an atom within sqrt(b2) (+ tol) of fx
                const float wx = __builtin_amdgcn_sqrtf(b2) * 1.0001f + tol;  // raw v_sqrt_f32: heuristic bound only
                const int x0 = max(max((int)floorf(fx - wx), cx - 2), 0);
                const int x1 = min(min((int)floorf(fx + wx), cx + 2), (int)g.dim_x - 1);
                const uint32_t c0 = g.cell_base + (uint32_t)x0 + yy * g.dim_x + zz * g.dim_x * g.dim_y;
                const bool rel16 = g.in_lds != 0u;
                const uint32_t first = load_cell_start(cells, c0, rel16);
                run_len = load_cell_start(cells, c0 + (uint32_t)(x1 - x0) + 1u, rel16) - first;
                run_start = (rel16 ? g.sorted_base : 0u) + first;
            }
            s_runs[w][at][r] = make_uint2(run_start, run_len);
            if (r == 0u) s_sr[w][at] = sr;
        }
        wave_lds_fence();
    }

    for (uint32_t pi = p_begin; pi < p_end; pi++) {
        const uint32_t at = pi - p_begin;
        const uint32_t p = list_mode ? work_list[pi] : pi;
        const float4 me = sorted_xyzr[p];
        const float R = me.w + probe;                    // lib.rs:101
        const float R2 = R * R;                          // lib.rs:102
        const float twoR = 2.0f * R;                     // lib.rs:136
        const float sr = s_sr[w][at];                    // spatial_grid.rs:307
        const float sr2 = sr * sr;                       // spatial_grid.rs:308
        const float near2 = kNearScale2 * R2;
        unsigned long long my_id = 0;
        if (HAS_ID) my_id = sorted_id ? sorted_id[p] : a.ids_in[a.sorted_orig[p]];
        uint32_t run_start = 0, run_len = 0;
        if (lane < 25u) {
            const uint2 rr = s_runs[w][at][lane];
            run_start = rr.x;
            run_len = rr.y;
        }
        // Sweep units: 16-atom segments of the runs, or (flat sweep) the atoms themselves, in
        // which case seg_excl is the flat position of the run's first atom and n_seg_total = T.
        const uint32_t nseg = kFlatSweep ? run_len : (run_len + (uint32_t)(kSegLanes - 1)) >> kSegShift;
        const uint32_t seg_incl = scan_lanes32(nseg);
        const uint32_t n_seg_total = (uint32_t)__builtin_amdgcn_readlane((int)seg_incl, 31);
        const uint32_t seg_excl = seg_incl - nseg;
        const bool run_ne = run_len > 0u;
        if (kFlatSweep) {
            const unsigned long long ne_mask = __ballot(run_ne);
            if (run_ne) s_delta[w][mbcnt64(ne_mask)] = (int)run_start - (int)seg_excl;
        }
        uint32_t mword = 0, base_rank = 0;  // flat sweep: marker words (lanes 0..7), runs started so far

        float accessible = 0.0f;
        uint32_t k_total = 0;
        bool all_groups = false;

        for (uint32_t ch0 = 0; ch0 < n_chunks; ch0 += NCH) {
            if (!single_group) load_group(ch0);
            unsigned long long occ[NCH];
#pragma unroll
            for (int c = 0; c < NCH; c++) occ[c] = invalid[c];
            unsigned long long rem_mask = 0ull;
            const bool do_rem = (ch0 == 0) && (n_rem != 0);

            uint32_t n_list = 0;
            bool done = false, flushed = false, counted = false;
            float acc_fused = 0.0f;
            uint32_t seg_i = 0;  // next segment (over all table rounds)
            bool exhausted = n_seg_total == 0u;

            while (!exhausted && !done) {
                if (kFlatSweep) {
                    if ((seg_i & 255u) == 0u) {
                        // markers of the run starts inside flat positions [seg_i, seg_i + 256)
                        wave_lds_fence();
                        if (lane < 8u) s_mask[w][lane] = 0u;
                        wave_lds_fence();
                        if (run_ne && (seg_excl - seg_i) < 256u)
                            atomicOr(&s_mask[w][(seg_excl - seg_i) >> 5], 1u << ((seg_excl - seg_i) & 31u));
                        wave_lds_fence();
                        mword = lane < 8u ? s_mask[w][lane] : 0u;
                        base_rank = (uint32_t)__popcll(__ballot(run_ne && seg_excl < seg_i));
                    }
                    const uint32_t round_end = min(n_seg_total, (seg_i & ~255u) + 256u);
                    // -- 2. sweep 64 atoms of the flattened runs per iteration: distance rule only.
                    // Lanes past the end look at the atom itself, which the q != p test rejects.
                    while (seg_i < round_end && n_list <= (uint32_t)kListFlush) {
                        const int win2 = (int)((seg_i >> 5) & 6u);
                        const unsigned long long mask64 =
                            (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)mword, win2) |
                            ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)mword, win2 + 1) << 32);
                        // run that holds flat position f: (runs started at or before f) - 1
                        const uint32_t rnk = base_rank + (uint32_t)(mask64 & 1ull) + mbcnt64(mask64 >> 1) - 1u;
                        base_rank += (uint32_t)__popcll(mask64);
                        const uint32_t f = seg_i + lane;
                        uint32_t q = p;
                        if (f < n_seg_total) q = (uint32_t)((int)f + s_delta[w][rnk]);
                        const float4 o = sorted_xyzr[q];
                        const float dx = me.x - o.x, dy = me.y - o.y, dz = me.z - o.z;
                        const float d2 = dx * dx + dy * dy + dz * dz;          // spatial_grid.rs:321
                        const bool accept = (q != p) && (d2 <= sr2);            // spatial_grid.rs:335
                        const unsigned long long m = __ballot(accept);
                        s_list[w][accept ? n_list + mbcnt64(m) : dummy_slot] = q;
                        n_list += (uint32_t)__popcll(m);
                        seg_i += 64u;
                    }
                } else {
                if ((seg_i & (uint32_t)(kSegCap - 1)) == 0u) {
                        // (re)fill the segment table for the round that starts at seg_i
                        wave_lds_fence();
                        const uint32_t n_round = min(n_seg_total - seg_i, (uint32_t)kSegCap);
                        for (uint32_t j = 0; j < nseg; j++) {
                            const uint32_t idx = seg_excl + j - seg_i;  // wraps for other rounds
                            if (idx < (uint32_t)kSegCap)
                                s_seg[w][idx] = make_uint2(run_start + (uint32_t)kSegLanes * j, min((uint32_t)kSegLanes, run_len - (uint32_t)kSegLanes * j));
                        }
                        if (lane < (uint32_t)(64 / kSegLanes)) s_seg[w][n_round + lane] = make_uint2(0u, 0u);
                        wave_lds_fence();
                    }
                    const uint32_t round_end = min(n_seg_total, (seg_i & ~(uint32_t)(kSegCap - 1)) + (uint32_t)kSegCap);
                    // -- 2. sweep four segments (16 lanes each) per iteration: distance rule only.
                    // Lanes past the end of their segment look at the atom itself, which the
                    // q != p test rejects, so the loop body is branch free.
                    while (seg_i < round_end && n_list <= (uint32_t)kListFlush) {
                        const uint2 sg = s_seg[w][(seg_i & (uint32_t)(kSegCap - 1)) + seg_grp];
                        const uint32_t q = seg_sub < sg.y ? sg.x + seg_sub : p;
                        const float4 o = sorted_xyzr[q];
                        const float dx = me.x - o.x, dy = me.y - o.y, dz = me.z - o.z;
                        const float d2 = dx * dx + dy * dy + dz * dz;          // spatial_grid.rs:321
                        const bool accept = (q != p) && (d2 <= sr2);            // spatial_grid.rs:335
                        const unsigned long long m = __ballot(accept);
                        s_list[w][accept ? n_list + mbcnt64(m) : dummy_slot] = q;
                        n_list += (uint32_t)__popcll(m);
                        seg_i += (uint32_t)(64 / kSegLanes);
                    }
                }
                exhausted = seg_i >= n_seg_total;
                if (n_list <= (uint32_t)kListFlush && !exhausted) continue;
                const bool last = exhausted;
                {
                    // ---- flush: decide points against the queued candidates ----
                    const uint32_t K = n_list;
                    wave_lds_fence();
                    // -- 3. prep (lane = candidate): id rule, v, limit; the first pass puts the
                    //       near candidates first
                    uint32_t nA = 0;
                    for (uint32_t k0 = 0; k0 < K; k0 += 64u) {
                        const uint32_t k = k0 + lane;
                        const bool live = k < K;
                        const uint32_t q = s_list[w][live ? k : 0u];
                        const float4 o = sorted_xyzr[q];
                        float4 e;
                        e.x = me.x - o.x; e.y = me.y - o.y; e.z = me.z - o.z;  // lib.rs:129-131
                        const float d2 = e.x * e.x + e.y * e.y + e.z * e.z;    // lib.rs:132-133
                        const float tj = o.w + probe;                          // spatial_grid.rs:336
                        const float t = tj * tj;                               // spatial_grid.rs:339
                        e.w = (t - d2 - R2) / twoR;                            // lib.rs:136
                        bool keep = live;
                        if (HAS_ID) keep = live && ((sorted_id ? sorted_id[q] : a.ids_in[a.sorted_orig[q]]) != my_id);  // spatial_grid.rs:314, lib.rs:124
                        if (!keep) e.w = neg_inf;                              // never occludes
                        const unsigned long long mK = __ballot(keep);
                        if (ch0 == 0) k_total += (uint32_t)__popcll(mK);
                        uint32_t slot = k;
                        if (k0 == 0) {
                            const unsigned long long mN = __ballot(keep && d2 < near2);
                            const unsigned long long mAll = __ballot(live);
                            nA = (uint32_t)__popcll(mN);
                            slot = ((mN >> lane) & 1ull) ? mbcnt64(mN) : nA + mbcnt64(mAll & ~mN);
                        }
                        if (live) s_cand[w][slot] = e;
                    }
                    if (lane < 16u) s_cand[w][K + lane] = make_float4(0.f, 0.f, 0.f, neg_inf);  // tile padding
                    wave_lds_fence();
                    // -- remainder points, scalar rule (lib.rs:185-186,206-207): plain products, `<=`
                    if (do_rem) {
                        // candidate slots past K hold limit = -inf, so whole steps run unchecked
                        unsigned long long mm = 0ull;
                        const float4 *cp = &s_cand[w][rem_grp];
                        const uint32_t steps = (K + rem_groups - 1u) >> (6u - rem_shift);
                        for (uint32_t st = 0; st < steps; st++) {
                            const float4 cd = *cp;
                            cp += rem_groups;
                            mm |= __ballot((rp.x * cd.x + rp.y * cd.y + rp.z * cd.z) <= cd.w);
                        }
                        // OR together the lanes that hold the same point (lane % P)
                        mm |= mm >> 32;
                        if (rem_shift < 5u) mm |= mm >> 16;
                        if (rem_shift < 4u) mm |= mm >> 8;
                        if (rem_shift < 3u) mm |= mm >> 4;
                        if (rem_shift < 2u) mm |= mm >> 2;
                        if (rem_shift < 1u) mm |= mm >> 1;
                        rem_mask |= mm & rem_low;
                    }
                    // When the whole candidate list is resident (the usual case: one flush), every
                    // chunk group is decided here, so the sweep runs once per atom whatever n_points
                    // is.  Otherwise only the current group is updated and its masks persist.
                    const bool single_flush = last && !flushed;
                    const uint32_t nB = K - nA;
                    uint32_t g0 = ch0;
                    do {
                        if (g0 != ch0) {
                            load_group(g0);
#pragma unroll
                            for (int c = 0; c < NCH; c++) occ[c] = invalid[c];
                        }
                        // -- 4. phase A: near candidates against all fused-rule points (lane = point),
                        // four per trip (slots past nA hold far candidates or -inf padding: harmless).
                        // Each lane keeps max(limit - dot): positive iff some candidate occludes the
                        // point - exactly `dot < limit` in IEEE arithmetic with denormals preserved
                        // (see occlusion_fast.inc).
                        {
                            float mA[NCH];
#pragma unroll
                            for (int c = 0; c < NCH; c++) mA[c] = neg_inf;
                            for (uint32_t k = 0; k < nA; k += 4u) {
                                const float4 c0 = s_cand[w][k], c1 = s_cand[w][k + 1u], c2 = s_cand[w][k + 2u], c3 = s_cand[w][k + 3u];
#pragma unroll
                                for (int c = 0; c < NCH; c++) {
                                    // lib.rs:143-146: mul_add(sx, vx, mul_add(sy, vy, sz * vz)) < limit
                                    const float a0 = c0.w - __builtin_fmaf(sx[c], c0.x, __builtin_fmaf(sy[c], c0.y, sz[c] * c0.z));
                                    const float a1 = c1.w - __builtin_fmaf(sx[c], c1.x, __builtin_fmaf(sy[c], c1.y, sz[c] * c1.z));
                                    const float a2 = c2.w - __builtin_fmaf(sx[c], c2.x, __builtin_fmaf(sy[c], c2.y, sz[c] * c2.z));
                                    const float a3 = c3.w - __builtin_fmaf(sx[c], c3.x, __builtin_fmaf(sy[c], c3.y, sz[c] * c3.z));
                                    mA[c] = fmaxf(fmaxf(mA[c], a0), a1);
                                    mA[c] = fmaxf(fmaxf(mA[c], a2), a3);
                                }
                            }
#pragma unroll
                            for (int c = 0; c < NCH; c++) occ[c] |= __builtin_amdgcn_ballot_w64(mA[c] > 0.0f);
                        }
                        // -- 5. phase B: far candidates against the survivors
                        uint32_t S = 0;
#pragma unroll
                        for (int c = 0; c < NCH; c++) S += (uint32_t)__popcll(~occ[c]);
                        if (single_flush && (S == 0u || nB == 0u)) {
                            acc_fused += (float)S;
                        } else if (single_flush && S <= 64u) {
                            // compact the survivors' point indices through LDS
                            uint32_t base = 0;
#pragma unroll
                            for (int c = 0; c < NCH; c++) {
                                const unsigned long long sv = ~occ[c];
                                if ((sv >> lane) & 1ull)
                                    s_pts[w][base + mbcnt64(sv)] = (uint32_t)c * 64u + lane;  // index inside the group
                                base += (uint32_t)__popcll(sv);
                            }
                            wave_lds_fence();
                            // lanes tiled as (survivor = lane % P, candidate group = lane / P)
                            const uint32_t ps = S <= 8u ? 3u : (S <= 16u ? 4u : (S <= 32u ? 5u : 6u));
                            const uint32_t G = 64u >> ps;
                            const uint32_t pt = lane & ((1u << ps) - 1u);
                            const uint32_t grp = lane >> ps;
                            // the survivor's coordinates come from the lattice registers of the lane
                            // that owns the point (ds_bpermute, no memory round trip)
                            float4 pv = make_float4(0.f, 0.f, 0.f, 0.f);
                            {
                                const uint32_t idx = pt < S ? s_pts[w][pt] : 0u;
                                const int src = (int)((idx & 63u) << 2);
                                float px = 0.f, py = 0.f, pz = 0.f;
#pragma unroll
                                for (int c = 0; c < NCH; c++) {
                                    const float qx = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(sx[c])));
                                    const float qy = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(sy[c])));
                                    const float qz = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(sz[c])));
                                    if ((idx >> 6) == (uint32_t)c) { px = qx; py = qy; pz = qz; }
                                }
                                if (pt < S) pv = make_float4(px, py, pz, 0.f);
                            }
                            // candidate slots past K hold limit = -inf (written by the prep pass),
                            // so whole steps can run without a tail test; two steps per trip
                            // (2 G - 1 <= 15 padding entries)
                            float mx = neg_inf;
                            const float4 *cp = &s_cand[w][nA + grp];
                            const uint32_t steps = (nB + G - 1u) >> (6u - ps);
                            for (uint32_t st = 0; st < steps; st += 2u) {
                                const float4 cd = cp[0], ce = cp[G];
                                cp += 2u * G;
                                const float t0 = cd.w - __builtin_fmaf(pv.x, cd.x, __builtin_fmaf(pv.y, cd.y, pv.z * cd.z));
                                const float t1 = ce.w - __builtin_fmaf(pv.x, ce.x, __builtin_fmaf(pv.y, ce.y, pv.z * ce.z));
                                mx = fmaxf(fmaxf(mx, t0), t1);
                            }
                            unsigned long long mm = __builtin_amdgcn_ballot_w64(mx > 0.0f);
                            for (uint32_t sh = 1u << ps; sh < 64u; sh <<= 1) mm |= mm >> sh;
                            const unsigned long long low = S >= 64u ? ~0ull : ((1ull << S) - 1ull);
                            acc_fused += (float)(S - (uint32_t)__popcll(mm & low));
                            wave_lds_fence();
                        } else {
                            // far candidates broadcast against all points of the group, masks exact
                            {
                                float mB[NCH];
#pragma unroll
                                for (int c = 0; c < NCH; c++) mB[c] = neg_inf;
                                for (uint32_t k = nA; k < K; k += 2u) {  // slot K is -inf padding
                                    const float4 cd = s_cand[w][k], ce = s_cand[w][k + 1u];
#pragma unroll
                                    for (int c = 0; c < NCH; c++) {
                                        const float t0 = cd.w - __builtin_fmaf(sx[c], cd.x, __builtin_fmaf(sy[c], cd.y, sz[c] * cd.z));
                                        const float t1 = ce.w - __builtin_fmaf(sx[c], ce.x, __builtin_fmaf(sy[c], ce.y, sz[c] * ce.z));
                                        mB[c] = fmaxf(fmaxf(mB[c], t0), t1);
                                    }
                                }
#pragma unroll
                                for (int c = 0; c < NCH; c++) occ[c] |= __builtin_amdgcn_ballot_w64(mB[c] > 0.0f);
                            }
                            if (single_flush) {
#pragma unroll
                                for (int c = 0; c < NCH; c++) acc_fused += (float)__popcll(~occ[c]);  // lib.rs:156-159
                            }
                        }
                        g0 += NCH;
                    } while (single_flush && g0 < n_chunks);
                    if (single_flush) {
                        counted = true;
                        all_groups = true;
                    } else {
                        flushed = true;
                        if (!counting) {
                            unsigned long long all = ~0ull;
#pragma unroll
                            for (int c = 0; c < NCH; c++) all &= occ[c];
                            done = (all == ~0ull) && (!do_rem || rem_mask == rem_low);  // lib.rs:149-152
                        }
                    }
                    wave_lds_fence();
                    n_list = 0;
                }
            }
            if (!counted) {
#pragma unroll
                for (int c = 0; c < NCH; c++) acc_fused += (float)__popcll(~occ[c]);  // lib.rs:156-159
            }
            accessible += acc_fused;
            if (do_rem) accessible += (float)(n_rem - (uint32_t)__popcll(rem_mask));  // lib.rs:215-217
            if (all_groups) break;
        }

        if (lane == 0) {
            const uint32_t orig = a.sorted_orig[p];
            const float surface_area = (4.0f * 3.14159274101257324219f) * R2;  // 4.0 * PI * r2, lib.rs:220
            const float inv_n = 1.0f / (float)n_points;                        // lib.rs:221
            a.atom_sasa[orig] = surface_area * accessible * inv_n;             // lib.rs:222
            if (counting) a.neighbor_counts[orig] = k_total;
        }
        wave_lds_fence();
    }
    if (!list_mode) break;
    p_begin += gridDim.x * 4u * apw;
    if (p_begin >= n_work) break;
  }
}
