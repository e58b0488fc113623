// k_occlusion_fast: the straight-line version of k_occlusion_v3 for the common case
//   * n_points <= 128 (two 64-point chunks held in registers for the whole wave),
//   * at most 4 remainder points (kept in SGPRs, tested inside the prep pass),
//   * an atom whose culled runs hold at most 256 atoms and whose candidate list fits the LDS
//     list (kFastCap); any other atom is appended to the batch's deferred list and handled by
//     k_occlusion_v3 in list mode right after this kernel.
// Same stages and the same f32 expressions as k_occlusion_v3 (see occlusion.hip); what is gone
// is the bookkeeping of the general kernel (chunk groups, repeated flushes, early-out flags),
// which cost scalar instructions and SGPR spills on every atom.  A wave works through its atoms
// one after the other, so the kernel is also built for a short per-atom dependency chain and a
// full CU: <= 72 VGPRs and 20 KB of LDS (7-8 waves per SIMD), the next atom's record prefetched,
// both sweep gathers of an atom in flight together, accepted candidates kept as LDS records (no
// second gather), survivors' coordinates fetched by ds_bpermute instead of from memory.
//
// Point tests accumulate max(limit_j - dot_j) and read "occluded" off as max > 0.  In IEEE
// binary32 with gradual underflow (the kernels run with float_denorm_mode_32 = 3, i.e.
// denormals preserved) limit - dot > 0 holds exactly when dot < limit, so this is the
// reference's comparison (lib.rs:146), not an approximation; -inf limits (padding, id rule)
// give -inf and NaN never appears for finite input.

constexpr int kFastCap = 144;              // candidate records per wave (LDS: 8 workgroups per CU)
constexpr uint32_t kFastMaxSwept = 256;    // atoms in the culled runs (one run-start mask window)
constexpr uint32_t kFastMaxRem = 4;        // remainder points held in SGPRs
constexpr int kFastAtomsPerWave = 10;      // 250 (atom, run) pairs fill four prologue passes
constexpr int kTileSteps = 2;                 // phase-B tile steps (LDS reads in flight) per trip: 2 or 4 (no difference measured)
constexpr int kCandPad = 8 * kTileSteps;      // -inf records behind the candidate list (tile over-read)


__device__ __forceinline__ float uniform_f(float v)
{
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// The culled x-runs of the wave's atoms (same rule as k_occlusion_v3's prologue), in two steps so
// that per-atom work is not repeated in all 25 run lanes: (1) lane = atom: position in cell units,
// cell, thresholds -> a 16-word record in `scratch` (the candidate buffer, idle at this point);
// (2) lane = (atom, run) pair, 64 pairs per pass: gap to the run's row, trimmed x range, the run's
// first atom and length from the cell table.
__device__ __forceinline__ void prologue_runs(const OccArgs3 &a, uint32_t first, uint32_t n_mine, float probe,
                                              float4 *scratch, uint2 (*runs)[25], float *srs)
{
    const uint32_t lane = lane_id();
    if (lane < n_mine) {
        const uint32_t pa = first + lane;
        const float4 m = a.sorted_xyzr[pa];
        const StructGrid g = a.grids[a.sid[pa]];
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
        const uint32_t dim_xy = g.dim_x * g.dim_y;
        float4 *rec = scratch + 4u * lane;
        rec[0] = make_float4(fx, fy - (float)cy, fz - (float)cz, srn * srn * 1.00001f);
        rec[1] = make_float4(tol, __int_as_float(cx), __int_as_float(cy), __int_as_float(cz));
        rec[2] = make_float4(__uint_as_float(g.dim_x), __uint_as_float(g.dim_y), __uint_as_float(g.dim_z),
                             __uint_as_float(g.cell_base + (uint32_t)cy * g.dim_x + (uint32_t)cz * dim_xy));
        // .y: what a cell entry is relative to (16-bit entries, LDS-binned structure), or all ones (32-bit absolute entries)
        rec[3] = make_float4(__uint_as_float(dim_xy), __uint_as_float(g.in_lds ? g.sorted_base : 0xFFFFFFFFu), 0.f, 0.f);
        srs[lane] = sr;
    }
    wave_lds_fence();
    for (uint32_t idx = lane; idx < n_mine * 25u; idx += 64u) {
        const uint32_t at = (idx * 5243u) >> 17;  // idx / 25 for idx < 2^14
        const uint32_t r = idx - at * 25u;
        const int rdz = (int)((r * 13u) >> 6) - 2;  // r / 5 - 2 for r < 25
        const int rdy = (int)r - (rdz + 2) * 5 - 2;
        const float4 *rec = scratch + 4u * at;
        const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
        const float fx = r0.x, uy = r0.y, uz = r0.z, thr = r0.w, tol = r1.x;
        const int cx = __float_as_int(r1.y), cy = __float_as_int(r1.z), cz = __float_as_int(r1.w);
        const uint32_t dim_x = __float_as_uint(r2.x), dim_y = __float_as_uint(r2.y), dim_z = __float_as_uint(r2.z);
        // With u = f - c the fractional position inside the cell, the gap to row c + d is d - u
        // (d > 0), u - d - 1 (d < 0) or 0; a run whose gap exceeds the search radius is dropped,
        // the others are trimmed to the cells that can hold an atom within reach.
        float gy = rdy > 0 ? (float)rdy - uy : (rdy < 0 ? uy - (float)(rdy + 1) : 0.0f);
        float gz = rdz > 0 ? (float)rdz - uz : (rdz < 0 ? uz - (float)(rdz + 1) : 0.0f);
        gy = fmaxf(gy - tol, 0.0f);
        gz = fmaxf(gz - tol, 0.0f);
        const float b2 = __builtin_fmaf(-gy, gy, __builtin_fmaf(-gz, gz, thr));
        const uint32_t yy = (uint32_t)(cy + rdy), zz = (uint32_t)(cz + rdz);
        uint32_t run_start = 0, run_len = 0;
        if (yy < dim_y && zz < dim_z && b2 >= 0.0f) {
            const float wx = __builtin_amdgcn_sqrtf(b2) * 1.0001f + tol;  // heuristic bound only
            const int x0 = max(max((int)floorf(fx - wx), cx - 2), 0);
            const int x1 = min(min((int)floorf(fx + wx), cx + 2), (int)dim_x - 1);
            const float4 r3 = rec[3];
            const uint32_t dim_xy = __float_as_uint(r3.x), rel_base = __float_as_uint(r3.y);
            const bool rel16 = rel_base != 0xFFFFFFFFu;
            const uint32_t c0 = __float_as_uint(r2.w) + (uint32_t)(rdy * (int)dim_x) + (uint32_t)(rdz * (int)dim_xy) + (uint32_t)x0;
            const uint32_t first = load_cell_start(a.cells, c0, rel16);
            run_len = load_cell_start(a.cells, c0 + (uint32_t)(x1 - x0) + 1u, rel16) - first;
            run_start = (rel16 ? rel_base : 0u) + first;
        }
        runs[at][r] = make_uint2(run_start, run_len);
    }
    wave_lds_fence();
}

template <bool HAS_ID, bool HAS_REM, bool HALF1>
__global__ __launch_bounds__(256) void k_occlusion_fast(OccArgs3 a)
{
    if (batch_aborted(a.status)) return;
    __shared__ float4 s_cand[4][kFastCap + kCandPad];  // sweep: accepted atoms (x, y, z, r); after prep: (vx, vy, vz, limit), near first; +16 padding
    __shared__ int s_delta[4][32];               // per non-empty run: start - exclusive prefix
    __shared__ uint32_t s_mask[4][8];            // run-start markers of the 256 flat positions
    __shared__ uint32_t s_pts[4][64];
    __shared__ uint2 s_runs[4][kFastAtomsPerWave][25];
    __shared__ float s_sr[4][kFastAtomsPerWave];

    const float4 *__restrict__ sorted_xyzr = a.sorted_xyzr;
    const uint64_t *__restrict__ sorted_id = a.sorted_id;
    const float4 *__restrict__ lat4 = a.lat4;
    const uint32_t n_atoms = a.n_atoms;

    const uint32_t lane = lane_id();
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // The launch covers the cell-sorted positions [lo, hi): all of them, or the part below / from
    // BatchStatus::tail_atom_base while the tail is still being binned on another stream.  Only
    // the first ceil((hi - lo) / (4 apw)) workgroups have work; they are dealt round-robin to the
    // XCDs by the hardware, and the remap gives each XCD a contiguous piece of [lo, hi).
    const uint32_t apw = a.atoms_per_wave;
    uint32_t lo = 0, hi = n_atoms;
    if (a.part == kOccHead) hi = min(hi, a.status->tail_atom_base);
    else if (a.part == kOccRest) lo = min(hi, a.status->tail_atom_base);
    const uint32_t n_blocks = (hi - lo + 4u * apw - 1u) / (4u * apw);
    uint32_t bid = blockIdx.x;
    if (bid >= n_blocks) return;
    {
        const uint32_t per = n_blocks / 8u;
        if (bid < per * 8u) bid = (bid % 8u) * per + bid / 8u;
    }
    const uint32_t w_begin = lo + (bid * 4u + w) * apw;
    if (w_begin >= hi) return;
    const uint32_t w_end = min(w_begin + apw, hi);

    const float probe = a.probe;
    const uint32_t n_points = a.n_points;  // <= 128
    const uint32_t n_fused = a.n_fused;
    const uint32_t n_rem = HAS_REM ? n_points - n_fused : 0u;  // <= kFastMaxRem
    const bool counting = a.neighbor_counts != nullptr;
    const float neg_inf = __int_as_float(0xFF800000);

    // ---- per-wave constants: the lattice (lane = point) and the remainder points (uniform) ----
    float sx[2], sy[2], sz[2], m_init[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        // lattice arrays are zero padded to 64s.  HALF1 (at most 96 fused points): both halves of the
        // second chunk hold points 64..95, so that one instruction tests them against TWO candidates.
        const uint32_t pi = (HALF1 && c == 1) ? 64u + (lane & 31u) : (uint32_t)c * kWave + lane;
        const bool in_range = pi < ((n_points + 63u) & ~63u);
        sx[c] = in_range ? a.lat_x[pi] : 0.0f;
        sy[c] = in_range ? a.lat_y[pi] : 0.0f;
        sz[c] = in_range ? a.lat_z[pi] : 0.0f;
        m_init[c] = pi < n_fused ? neg_inf : 1.0f;  // points outside the fused rule start "occluded"
    }
    // unused remainder slots hold NaN: `NaN <= limit` is false, so they never report a hit
    float rx[kFastMaxRem], ry[kFastMaxRem], rz[kFastMaxRem];
#pragma unroll
    for (uint32_t r = 0; r < kFastMaxRem; r++) {
        const float nan = __int_as_float(0x7FC00000);
        float4 q = make_float4(nan, nan, nan, 0.f);
        if (HAS_REM && r < n_rem) q = lat4[n_fused + r];
        rx[r] = uniform_f(q.x);
        ry[r] = uniform_f(q.y);
        rz[r] = uniform_f(q.z);
    }

  // the wave's atoms in groups of kFastAtomsPerWave: one dense prologue and one write-out per group
  for (uint32_t p_begin = w_begin; p_begin < w_end; p_begin += (uint32_t)kFastAtomsPerWave) {
    const uint32_t p_end = min(p_begin + (uint32_t)kFastAtomsPerWave, w_end);
    prologue_runs(a, p_begin, p_end - p_begin, probe, s_cand[w], s_runs[w], s_sr[w]);

    // lane `at` collects atom p_begin + at's result: exposed points | candidates << 8 (or "deferred")
    constexpr uint32_t kDeferred = 0xFFFFFFFFu;
    uint32_t my_result = kDeferred;

    // the next atom's record is requested one atom ahead: a wave's atoms are processed one after
    // the other, so every global round trip on that chain costs throughput
    float4 me_next = sorted_xyzr[p_begin];
    unsigned long long id_next = 0;
    if (HAS_ID) id_next = sorted_id[p_begin];
    for (uint32_t p = p_begin; p < p_end; p++) {
        const uint32_t at = p - p_begin;
        const float4 me = me_next;
        const unsigned long long my_id = id_next;
        if (p + 1u < p_end) {
            me_next = sorted_xyzr[p + 1u];
            if (HAS_ID) id_next = sorted_id[p + 1u];
        }
        const float R = me.w + probe;   // lib.rs:101
        const float R2 = R * R;         // lib.rs:102
        const float twoR = 2.0f * R;    // lib.rs:136
        const float sr = s_sr[w][at];   // spatial_grid.rs:307
        const float sr2 = sr * sr;      // spatial_grid.rs:308
        const float near2 = kNearScale2 * R2;
        uint32_t run_start = 0, run_len = 0;
        if (lane < 25u) {
            const uint2 rr = s_runs[w][at][lane];
            run_start = rr.x;
            run_len = rr.y;
        }
        // -- 1. flat positions of the concatenated runs
        const uint32_t incl = scan_lanes32(run_len);
        const uint32_t T = (uint32_t)__builtin_amdgcn_readlane((int)incl, 31);
        const uint32_t excl = incl - run_len;
        const bool run_ne = run_len > 0u;
        bool defer = T > kFastMaxSwept;
        uint32_t K = 0;
        if (!defer) {
            // Run r > 0 (of the non-empty ones) is marked at flat position start - 1, so the run
            // holding position f is (marks below f): one mbcnt, no special case for position 0.
            const unsigned long long ne_mask = ballot64(run_ne);
            if (lane < 8u) s_mask[w][lane] = 0u;
            if (run_ne) s_delta[w][mbcnt64(ne_mask)] = (int)run_start - (int)excl;
            wave_lds_fence();
            if (run_ne && excl != 0u) atomicOr(&s_mask[w][(excl - 1u) >> 5], 1u << ((excl - 1u) & 31u));
            wave_lds_fence();
            const uint32_t mword = lane < 8u ? s_mask[w][lane] : 0u;
            // -- 2. sweep 64 flat positions per iteration, two iterations' gathers in flight: the
            // candidate rule and the id rule; accepted atoms' records go to the wave's LDS list.
            // Lanes past the end land behind the last run (index clamped), f < T rejects them.
            uint32_t base_rank = 0;
            auto flat_atom = [&](uint32_t seg_i) -> uint32_t {
                const int win2 = (int)(seg_i >> 5);
                const unsigned long long mask64 =
                    (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)mword, win2) |
                    ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)mword, win2 + 1) << 32);
                const uint32_t rnk = base_rank + mbcnt64(mask64);
                base_rank += (uint32_t)__popcll(mask64);
                return min((uint32_t)((int)(seg_i + lane) + s_delta[w][rnk]), n_atoms - 1u);
            };
            auto test_and_append = [&](uint32_t seg_i, uint32_t q, const float4 &o, unsigned long long oid) {
                const float dx = me.x - o.x, dy = me.y - o.y, dz = me.z - o.z;
                const float d2 = dx * dx + dy * dy + dz * dz;                          // spatial_grid.rs:321
                bool accept = (seg_i + lane < T) & (q != p) & (d2 <= sr2);              // spatial_grid.rs:335
                if (HAS_ID) accept = accept & (oid != my_id);                           // spatial_grid.rs:314, lib.rs:124
                const unsigned long long m = ballot64(accept);
                const uint32_t slot = K + mbcnt64(m);
                if (accept & (slot < (uint32_t)kFastCap)) s_cand[w][slot] = o;
                K += (uint32_t)__popcll(m);
            };
            for (uint32_t seg_i = 0; seg_i < T; seg_i += 128u) {
                const bool two = seg_i + 64u < T;
                const uint32_t qa = flat_atom(seg_i);
                const float4 oa = sorted_xyzr[qa];
                unsigned long long ia = 0, ib = 0;
                if (HAS_ID) ia = sorted_id[qa];
                uint32_t qb = qa;
                float4 ob = oa;
                if (two) {
                    qb = flat_atom(seg_i + 64u);
                    ob = sorted_xyzr[qb];
                    if (HAS_ID) ib = sorted_id[qb];
                }
                test_and_append(seg_i, qa, oa, ia);
                if (two) test_and_append(seg_i + 64u, qb, ob, ib);
            }
            defer = K > (uint32_t)kFastCap;  // more candidates than the LDS records hold
        }
        if (defer) {  // (my_result stays "deferred" for this atom)
            if (lane == 0) {
                a.work_list_out[atomicAdd(a.work_count_out, 1u)] = p;
                if (a.defer_flag) *a.defer_flag = 1u;
            }
            wave_lds_fence();
            continue;
        }
        wave_lds_fence();

        // -- 3. prep (lane = candidate), in place: (x, y, z, r) -> (v, limit); the first pass puts
        //       the near candidates first (a permutation inside the pass's 64 slots: every lane has
        //       read its record before any lane writes).  Remainder points (scalar rule,
        //       lib.rs:185-186,206-207: plain products, `<=`) are uniform values tested here
        //       against every candidate.
        uint32_t nA = 0;
        const uint32_t k_total = K;
        unsigned long long rem_hit[kFastMaxRem] = {0ull, 0ull, 0ull, 0ull};
        for (uint32_t k0 = 0; k0 < K; k0 += 64u) {
            const uint32_t k = k0 + lane;
            const bool live = k < K;
            const float4 o = s_cand[w][live ? k : 0u];
            float4 e;
            e.x = me.x - o.x; e.y = me.y - o.y; e.z = me.z - o.z;  // lib.rs:129-131
            const float d2 = e.x * e.x + e.y * e.y + e.z * e.z;    // lib.rs:132-133
            const float tj = o.w + probe;                          // spatial_grid.rs:336
            const float t = tj * tj;                               // spatial_grid.rs:339
            e.w = (t - d2 - R2) / twoR;                            // lib.rs:136
            if (!live) e.w = neg_inf;                              // never occludes
            uint32_t slot = k;
            if (k0 == 0) {
                // live lanes are 0..K-1 here, so a far lane has k - (near lanes before it) far
                // lanes before it
                const bool near = live & (d2 < near2);
                const unsigned long long mN = ballot64(near);
                const uint32_t before = mbcnt64(mN);
                nA = (uint32_t)__popcll(mN);
                slot = near ? before : nA + k - before;
            }
            if (live) s_cand[w][slot] = e;
            if (HAS_REM) {
#pragma unroll
                for (uint32_t r = 0; r < kFastMaxRem; r++)
                    rem_hit[r] |= ballot64((rx[r] * e.x + ry[r] * e.y + rz[r] * e.z) <= e.w);
            }
        }
        if (lane < (uint32_t)kCandPad) s_cand[w][K + lane] = make_float4(0.f, 0.f, 0.f, neg_inf);  // tile padding
        wave_lds_fence();

        // -- 4. phase A: near candidates against all fused-rule points (lane = point), four
        // candidates per trip.  Slots past nA hold far candidates or padding: testing them early
        // is harmless (the result is an OR over all candidates).
        float m0 = m_init[0], m1 = m_init[1];
        const uint32_t nA4 = min(K, (nA + 3u) & ~3u);
        const uint32_t hi = lane >> 5;
        for (uint32_t k = 0; k < nA; k += 4u) {
            const float4 c0 = s_cand[w][k], c1 = s_cand[w][k + 1u], c2 = s_cand[w][k + 2u], c3 = s_cand[w][k + 3u];
            // HALF1: lanes 0..31 take candidates k and k + 2, lanes 32..63 take k + 1 and k + 3
            const float4 p0 = HALF1 ? s_cand[w][k + hi] : c0, p1 = HALF1 ? s_cand[w][k + 2u + hi] : c1;
            // lib.rs:143-146: mul_add(sx, vx, mul_add(sy, vy, sz * vz)) < limit
            const float a0 = c0.w - __builtin_fmaf(sx[0], c0.x, __builtin_fmaf(sy[0], c0.y, sz[0] * c0.z));
            const float a1 = c1.w - __builtin_fmaf(sx[0], c1.x, __builtin_fmaf(sy[0], c1.y, sz[0] * c1.z));
            const float a2 = c2.w - __builtin_fmaf(sx[0], c2.x, __builtin_fmaf(sy[0], c2.y, sz[0] * c2.z));
            const float a3 = c3.w - __builtin_fmaf(sx[0], c3.x, __builtin_fmaf(sy[0], c3.y, sz[0] * c3.z));
            m0 = fmaxf(fmaxf(m0, a0), a1);
            m0 = fmaxf(fmaxf(m0, a2), a3);
            const float b0 = p0.w - __builtin_fmaf(sx[1], p0.x, __builtin_fmaf(sy[1], p0.y, sz[1] * p0.z));
            const float b1 = p1.w - __builtin_fmaf(sx[1], p1.x, __builtin_fmaf(sy[1], p1.y, sz[1] * p1.z));
            m1 = fmaxf(fmaxf(m1, b0), b1);
            if (!HALF1) {
                const float b2 = c2.w - __builtin_fmaf(sx[1], c2.x, __builtin_fmaf(sy[1], c2.y, sz[1] * c2.z));
                const float b3 = c3.w - __builtin_fmaf(sx[1], c3.x, __builtin_fmaf(sy[1], c3.y, sz[1] * c3.z));
                m1 = fmaxf(fmaxf(m1, b2), b3);
            }
        }
        // survivors of the second chunk: with HALF1 a point is occluded if either half saw an occluder
        auto survivors1 = [&](float m) -> unsigned long long {
            const unsigned long long o = ballot64(m > 0.0f);
            return HALF1 ? ~(o | (o >> 32)) & 0xFFFFFFFFull : ~o;
        };
        const unsigned long long sv0 = ballot64(!(m0 > 0.0f)), sv1 = survivors1(m1);

        // -- 5. phase B: far candidates against the survivors
        const uint32_t S0 = (uint32_t)__popcll(sv0);
        const uint32_t S = S0 + (uint32_t)__popcll(sv1);
        const uint32_t nB = K - nA4;
        uint32_t exposed = S;
        if (S != 0u && nB != 0u) {
            if (S <= 64u) {
                // compact the survivors' point indices through LDS
                if ((sv0 >> lane) & 1ull) s_pts[w][mbcnt64(sv0)] = lane;
                if ((sv1 >> lane) & 1ull) s_pts[w][S0 + mbcnt64(sv1)] = 64u + lane;
                wave_lds_fence();
                // lanes tiled as (survivor = lane % P, candidate group = lane / P)
                const uint32_t ps = S <= 8u ? 3u : (S <= 16u ? 4u : (S <= 32u ? 5u : 6u));
                const uint32_t G = 64u >> ps;
                const uint32_t pt = lane & ((1u << ps) - 1u);
                const uint32_t grp = lane >> ps;
                // the survivor's coordinates come from the lattice registers of the lane that owns the
                // point (ds_bpermute: no memory round trip)
                float4 pv = make_float4(0.f, 0.f, 0.f, 0.f);
                {
                    const uint32_t idx = pt < S ? s_pts[w][pt] : 0u;
                    const int src = (int)((idx & 63u) << 2);
                    const bool second = idx >= 64u;
                    const float x0 = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(sx[0])));
                    const float y0 = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(sy[0])));
                    const float z0 = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(sz[0])));
                    const float x1 = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(sx[1])));
                    const float y1 = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(sy[1])));
                    const float z1 = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(sz[1])));
                    if (pt < S) pv = make_float4(second ? x1 : x0, second ? y1 : y0, second ? z1 : z0, 0.f);
                }
                // candidate slots past K hold limit = -inf, so whole steps run without a tail test
                // (kTileSteps steps per trip - the LDS round trip, not the arithmetic, sets the pace;
                // the padding covers the extra steps: kTileSteps * G - 1 <= kCandPad - 1)
                float mx = neg_inf;
                const float4 *cp = &s_cand[w][nA4 + grp];
                const uint32_t steps = (nB + G - 1u) >> (6u - ps);
                for (uint32_t st = 0; st < steps; st += (uint32_t)kTileSteps) {
                    float4 cd[kTileSteps];
#pragma unroll
                    for (int u = 0; u < kTileSteps; u++) cd[u] = cp[(uint32_t)u * G];
                    cp += (uint32_t)kTileSteps * G;
                    float t[kTileSteps];
#pragma unroll
                    for (int u = 0; u < kTileSteps; u++)
                        t[u] = cd[u].w - __builtin_fmaf(pv.x, cd[u].x, __builtin_fmaf(pv.y, cd[u].y, pv.z * cd[u].z));
#pragma unroll
                    for (int u = 0; u < kTileSteps; u += 2) mx = fmaxf(fmaxf(mx, t[u]), t[u + 1]);
                }
                unsigned long long mm = ballot64(mx > 0.0f);
                for (uint32_t sh = 1u << ps; sh < 64u; sh <<= 1) mm |= mm >> sh;
                const unsigned long long low = S >= 64u ? ~0ull : ((1ull << S) - 1ull);
                exposed = S - (uint32_t)__popcll(mm & low);
            } else {
                // many survivors (few near candidates): broadcast the far candidates
                for (uint32_t k = nA4; k < K; k++) {
                    const float4 cd = s_cand[w][k];
                    m0 = fmaxf(m0, cd.w - __builtin_fmaf(sx[0], cd.x, __builtin_fmaf(sy[0], cd.y, sz[0] * cd.z)));
                    m1 = fmaxf(m1, cd.w - __builtin_fmaf(sx[1], cd.x, __builtin_fmaf(sy[1], cd.y, sz[1] * cd.z)));
                }
                exposed = (uint32_t)__popcll(ballot64(!(m0 > 0.0f))) + (uint32_t)__popcll(survivors1(m1));
            }
        }
        uint32_t rem_exposed = n_rem;                                          // lib.rs:215-217
        if (HAS_REM) {
#pragma unroll
            for (uint32_t r = 0; r < kFastMaxRem; r++)
                rem_exposed -= min((uint32_t)__popcll(rem_hit[r]), 1u);
        }
        if (lane == at) my_result = (exposed + rem_exposed) | ((counting ? k_total : 0u) << 8);       // lib.rs:156-159
        wave_lds_fence();
    }

    // ---- results of the wave's atoms, one lane each ----
    if (my_result != kDeferred) {
        const uint32_t p = p_begin + lane;
        const uint32_t orig = a.sorted_orig[p];
        const float R = sorted_xyzr[p].w + probe;                          // lib.rs:101
        const float surface_area = (4.0f * 3.14159274101257324219f) * (R * R);  // 4.0 * PI * r2, lib.rs:220
        const float inv_n = 1.0f / (float)n_points;                        // lib.rs:221
        const float accessible = (float)(my_result & 0xFFu);
        a.atom_sasa[orig] = surface_area * accessible * inv_n;             // lib.rs:222
        if (counting) a.neighbor_counts[orig] = my_result >> 8;
    }
  }
}
