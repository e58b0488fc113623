// k_occlusion_mx: group-union candidate search + point tests on the matrix instructions.
//
// What bounds this kernel on gfx950 (DESIGN.md 6a, measured in round 5 with observed residency, stage ablation and stamps):
// no single unit - the vector ALU + matrix pipe are 0.70 busy, the CU's one scalar unit 0.66 (a scalar instruction costs a
// SIMD a quarter of it: 4.2 cycles; a vector one 2.2, a compare that writes an SGPR pair 4.1), the LDS pipe 0.51 - and a wave
// spends most of its time on dependent latency: LDS round trips in a row, the filter instruction and what hangs on its
// result.  The kernel is therefore organised around few instructions per atom of EVERY kind and short dependent chains on
// the per-atom path: LDS stores go to dummy slots instead of being masked out, loops over tiles are unrolled on ranges, rare
// cases share one branch.  And around little state: whatever has to live through the atom loops - the next group's
// prefetched cell starts, a persistent wave's block bookkeeping - measured dearer than the latency it was meant to hide
// (DESIGN.md 7).  Shortening the work at the price of a longer chain does not pay either (the early way out for buried
// atoms, tools/experiments/round5_early_exit.patch: +2.5 %).
//
//   * A wave takes up to 64 consecutive cell-sorted atoms (lane = atom: cells, group boundaries, the
//     per-atom constants), and keeps their records in LDS (broadcast reads per atom later).  Atoms of the
//     same cell row (same structure, same y/z cell) whose x cells fall in the same aligned block of
//     2^shift cells (8 at most; fewer where the structure fills its grid densely) form a GROUP (about 5 atoms on protein input).  A group shares ONE union of swept
//     atoms - the 25 x-runs of the 5x5x5 block, widened to the group's x extent, the group's own row
//     first - gathered once into registers (lane = union slot, up to 4 x 64 slots).  Each atom then
//     tests lane = union slot with its own position as a uniform operand: no per-atom run tables, no
//     per-atom flat map, no gathers on the per-atom chain.  The candidate RULE is the reference's
//     (d^2 <= (r_i + max_r + 2p)^2, spatial_grid.rs:307-335), evaluated exactly on every union slot, so
//     the candidate SET is the reference's.
//   * The id rule (spatial_grid.rs:314, lib.rs:124) is applied on 32-bit folds of the ids; an atom
//     that meets an equal fold among its accepted candidates is left to the general kernel, which
//     compares the full ids.
//   * PREP (lane = candidate) turns the accepted records (x, y, z, r) into operand records
//     (vz, vy, vx, limit), near candidates first; the first 16 also as the f16 operand of the filter.
//     limit = (t - d2 - R2) / 2R is the IEEE quotient, computed in three operations from the divisor's
//     correctly rounded reciprocal (see prep).
//   * PHASE A, a one-sided filter on v_mfma_f32_16x16x4_4b_f16 (four independent 16 x 16 x 4 products per
//     instruction: tile 0 against 64 points): tile 0 against all points in two instructions.  The f16 limit is
//     lowered by more than every rounding can add to dot - limit, so a negative result proves
//     dot < limit (lib.rs:146) - see prep.  With at most 128 points a lane's two point operands never change: they
//     stay in registers for the wave's lifetime.
//   * PHASE B, exact: the points the filter left alive, 16 per instruction, against EVERY tile on
//     v_mfma_f32_16x16x4_f32.  With A = a candidate tile, B = 16 points as (z, y, x, -1) and C = 0 the
//     result is, bit for bit, fma(-1, limit, fma(sx, vx, fma(sy, vy, fma(sz, vz, 0)))) = dot - limit in
//     the reference's operation order (MI355X guide: the f32 MFMA is a k-ordered fmaf chain, C/D never
//     flush; checked on hardware by tools/microbench_mfma.hip).  dot < limit holds exactly when that
//     difference is a negative non-zero number, which is read off the bit patterns with unsigned maxima.
//   * The remainder points (the last N mod W, lib.rs:163-218: plain products, `<=`) are columns of phase A like
//     the others, but the ones the filter leaves alive never join the survivors' list: they get an exact pass of
//     their own on the vector ALU (phase_b_rem: the reference's own expression, lane = (point, candidate)).  Nothing
//     of this kernel's decisions is taken with a tolerance.
//
// Atoms this kernel cannot take (union of more than 256 atoms even for a single cell, more than
// kMxCap candidates, equal id folds, radii outside the range the f16 operands and the error bounds
// assume) go to the batch's deferred list ->
// k_occlusion_v3.

#define MX_MIN_WAVES 7   // waves per SIMD the register allocation must allow (<= 72 VGPRs; also selects the
                         // MFMA form that writes VGPRs directly: no accumulator-register copies)
constexpr int kMxCap = 128;               // candidate records per wave (8 tiles of 16)
constexpr uint32_t kMxUnion = 256;        // union slots: 4 register sets of 64
// (the instantiations without ids hold a fifth set, 320 slots, where the id folds' registers are free: two-cell groups in a
// dense medium, fewer narrowed groups elsewhere - see NS below)
constexpr uint32_t kMxMinAtoms = 32768;   // batches below this size go to the per-atom kernels (lower latency per call;
                                          // measured crossover: 16 k atoms 0.024 / 0.027 ms, 36 k 0.041 / 0.040, 129 k 0.094 / 0.080)
constexpr uint32_t kMxMaxPoints = 1344;   // points the kernel takes (11 groups of 128: 33 KB of LDS for the two operand tables)
constexpr uint32_t kMxAtoms = 64;         // most atoms per wave (lane = atom); small batches give a wave fewer (OccArgs3::atoms_per_wave)
constexpr uint32_t kMxAtomsMulti = 16;    // the same with more than 128 points (an atom is a microsecond of work there; less LDS per wave)
#define MX_MAX_SGPR 96   // 256-thread workgroups per CU = floor(800 / (ceil(sgpr / 16) * 16 + 16)): 96 -> 7, 80 -> 8
constexpr float kMxNearScale2 = 1.8f;     // near: d^2 < 1.8 (r_i + p)^2 - these fill tile 0, the only one phase A takes (heuristic split only;
                                          // 1.4 +4.0 %, 1.6 +1.3 %, 2.0 +1.5 %, 2.4 +10 %)
constexpr uint32_t kMxXShift = 3;         // a group's atoms share cx >> shift (aligned blocks of at most 2^kMxXShift cells along x)

typedef float mx_f4 __attribute__((ext_vector_type(4)));
typedef float mx_f16v __attribute__((ext_vector_type(16)));
typedef _Float16 mx_h4 __attribute__((ext_vector_type(4)));
typedef __fp16 mx_h2 __attribute__((ext_vector_type(2)));

// Two f32 -> packed f16, rounded towards zero (v_cvt_pkrtz_f16_f32).
__device__ __forceinline__ uint32_t pack_f16_rtz(float lo, float hi)
{
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(lo, hi));
}

__device__ __forceinline__ uint32_t max3u(uint32_t a, uint32_t b, uint32_t c) { return max(max(a, b), c); }

// true for the bit pattern of a negative, non-zero, non-NaN f32 (unsigned compare)
__device__ __forceinline__ bool is_negative_bits(uint32_t u) { return (u - 0x80000001u) <= 0x7F7FFFFFu; }
// the same in one instruction where the pattern cannot be a NaN's: the filter's and the patch test's results of columns that
// exist (a padding candidate, limit -inf, against a real point gives +inf; only padding against a padding column - a zero
// point, a zero patch - gives inf x 0 = NaN, and those columns are masked out by every caller)
__device__ __forceinline__ bool is_negative_no_nan(uint32_t u) { return u > 0x80000000u; }

__device__ __forceinline__ float readlane_f(float v, uint32_t l)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)l));
}
__device__ __forceinline__ uint32_t readlane_u(uint32_t v, uint32_t l)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l);
}

// ---- wave-uniform values kept on the vector ALU ----
// The compiler moves whatever it can prove uniform to the scalar unit, which is the busiest unit of this
// kernel.  These helpers hide the uniformity: their results live in vector registers.
__device__ __forceinline__ uint32_t vgpr_u(uint32_t s)  // a vector-register copy of a uniform value
{
    uint32_t r;
    asm("v_mov_b32 %0, %1" : "=v"(r) : "s"(s));
    return r;
}
__device__ __forceinline__ uint32_t vadd_u(uint32_t v, uint32_t c)  // v + c on the vector ALU
{
    uint32_t r;
    asm("v_add_u32 %0, %1, %2" : "=v"(r) : "v"(v), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t vbcnt64(unsigned long long m, uint32_t acc)  // acc + popcount(m)
{
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "s"((uint32_t)m), "v"(acc));
    asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(r) : "s"((uint32_t)(m >> 32)));
    return r;
}
// lane l: bit l of m ? if1 : if0
__device__ __forceinline__ uint32_t vsel(unsigned long long m, uint32_t if0, uint32_t if1)
{
    uint32_t r;
    asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(r) : "v"(if0), "v"(if1), "s"(m));
    return r;
}
__device__ __forceinline__ float vsel_f(unsigned long long m, float if0, float if1)
{
    return __uint_as_float(vsel(m, __float_as_uint(if0), __float_as_uint(if1)));
}
// lane l: bit l of m ? v : 0xFFFFFFFF
__device__ __forceinline__ uint32_t vsel_or_ones(unsigned long long m, uint32_t v)
{
    uint32_t r;
    asm("v_cndmask_b32 %0, -1, %1, %2" : "=v"(r) : "v"(v), "s"(m));
    return r;
}
// number of set bits of m below this lane, plus add
__device__ __forceinline__ uint32_t mbcnt64_add(unsigned long long m, uint32_t add)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, add));
}

// MULTI: more than 128 sphere points.  The points are taken in groups of NT tiles: phase A
// per group with the group's operands re-read from LDS, survivors of all groups collected in one
// list that phase B works off 16 at a time.  NT is 8 then and NP the padded point count.
//
// NW waves per workgroup: they share the point tables (24 bytes per point) and nothing else.  With
// many points the tables limit how many workgroups fit a CU's LDS; larger workgroups then keep more
// waves resident (launch_occlusion picks NW).
// Persistent waves (see the kernel): with many points a workgroup's start - 24 KB of point tables at 960 points - is
// paid per 8 x 16 atoms otherwise, and the waves' uneven ends leave slots empty: - 9.5 % on 1M atoms x 960 points.  At
// 100 points the start is cheap and the loop-carried state costs the atom loops registers: + 2 %, so those launches
// keep one block of atoms per wave.
// Wave priorities (s_setprio): a wave that is waiting for memory - its block's atoms at the start, the cell starts and
// the union's records in a group's prologue, the result stores at the end - issues ahead of the waves that are in their
// atom loops, which have instructions to spare: - 0.8 % (measured one by one: group prologue - 0.6 %, start and end
// - 0.2 %; raising the point tests or the sweep instead: + 0.5 % / + 0.7 %).
constexpr int kMxPrioGroup = 2;
constexpr int kMxPrioStart = 3;
constexpr int kMxPrioEnd = 3;
// Phase A's two point operands (launches with at most 128 points) do not depend on the atom: a lane keeps its 2 x 8 bytes
// in registers for the wave's lifetime instead of fetching them from the LDS table for every atom (two reads and one LDS
// round trip in front of the second matrix instruction): -0.9 % (only the first: no gain; both fetched per atom, but beside the
// candidates: +1.5 %).
constexpr bool mx_persistent(bool multi) { return multi; }  // (persistent waves at 100 points too: +2.7 %, tools/experiments)

template <int NT, bool HAS_ID, bool HAS_REM, bool MULTI, int NW>
__global__ __launch_bounds__(64 * NW, NW >= 8 ? 6 : MX_MIN_WAVES)  /* 8 or 12 waves per workgroup: LDS keeps 6 waves per SIMD or fewer */ __attribute__((amdgpu_num_sgpr(MX_MAX_SGPR))) void k_occlusion_mx(OccArgs3 a)
{
    if (batch_aborted(a.status)) return;
    // OccArgs3::ids_check: the launch is one of a pair, with and without ids, and every STRUCTURE is one instantiation's -
    // the id-less one's unless the grid build found that its ids matter (StructGrid::odd_radii bit 1: two equal ids, or ids
    // nobody could check).  The instantiation with ids returns at once when no structure is its; the id-less one launched
    // alone (2: OcclusionChain::solo) tells the host when some structure is not its own: the batch is run again as a pair.
    if (a.ids_check) {
        const bool some_keep_ids = a.status->ids_needed != 0u;
        if (HAS_ID && !some_keep_ids) return;
        if (!HAS_ID && a.ids_check == 2u && some_keep_ids) {
            if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(const_cast<uint32_t *>(&a.status->ids_unordered), 2u);
            return;
        }
        // A workgroup whose atoms hold nothing of this instantiation's returns here, before it has fetched anything else
        // (BatchView::ids_seg: a bit per 64 cell-sorted atoms and kind of structure; the same words for every thread).  With
        // one structure of a batch keeping its ids, the instantiation with ids is 46 000 such workgroups and a few that work.
        if (!mx_persistent(MULTI) && a.ids_seg && some_keep_ids && a.part == kOccAll) {
            uint32_t bid = blockIdx.x;
            const uint32_t per = gridDim.x / 8u;
            if (bid < per * 8u) bid = (bid % 8u) * per + bid / 8u;  // (the block -> atoms mapping below)
            const uint32_t first = bid * (uint32_t)NW * a.atoms_per_wave;
            if (first >= a.n_atoms) return;
            const uint32_t last = min(a.n_atoms, first + (uint32_t)NW * a.atoms_per_wave) - 1u;
            const uint32_t *bits = a.ids_seg + (HAS_ID ? 0u : a.ids_seg_words);
            const uint32_t s0 = first >> 6, s1 = last >> 6;
            uint32_t any = 0u;
            for (uint32_t wd = s0 >> 5; wd <= (s1 >> 5); wd++) {
                const uint32_t lo_b = max(s0, wd << 5) & 31u, hi_b = min(s1, (wd << 5) + 31u) & 31u;
                any |= bits[wd] & (0xFFFFFFFFu >> (31u - hi_b)) & (0xFFFFFFFFu << lo_b);
            }
            if (!any) return;
        }
    }
    // points as matrix operands, component major: (z | y | x | -1) x NPS floats; NPS = NP + 16: the 16 entries
    // behind the points are zero (a column that nothing occludes: padding of phase B's last round)
    extern __shared__ float s_lat[];
    // Per wave, contiguous: the candidate list (sweep: accepted (x, y, z, r) records; after prep: operand records
    // (vz, vy, vx, limit)), the f16 operand of the filter and the survivors' point indices.  The sweep stores
    // EVERY lane's record: lanes that did not accept theirs write dummy slot kMxCap + lane, i.e. into the two
    // small arrays, which are dead during the sweep.
    // survivors (MULTI: up to 192, flushed to phase B before a group of 128 points could overflow them; else up to 128)
    // + padding of the last round (64) + dummy entries of the other lanes (64).  MULTI workgroups have 8 or 12 waves
    // and share a large point table: every byte per wave counts against the workgroups a CU holds (53.8 KB per
    // workgroup of 8 waves at 960 points left two on a CU instead of three: 1.37 against 1.16 ms on config 5).
    constexpr uint32_t kSurvivors = MULTI ? 192u : 128u;
    constexpr uint32_t kPts = MULTI ? kSurvivors + 128u : 448u;
    constexpr uint32_t kDummyPts = kSurvivors + 64u;
    struct __attribute__((aligned(16))) WaveLists {
        float4 cand[kMxCap];
        uint2 c16[16];       // tile 0 as f16 (vz, vy | vx, limit - margin); prep's other lanes store behind it, into
        uint2 vn16[MULTI ? 16 : 0];  // MULTI: tile 0's (|v| rounded up, 0 | 0, 0) as f16: k = 4..7 of the patch test; spare entries likewise
        uint16_t pts[kPts];  // the survivors' point indices (dead at that time)
    };
    constexpr uint32_t kSpillEnd = sizeof(WaveLists) / sizeof(float4);  // the sweep's stores stay below this record
    static_assert(kSpillEnd >= kMxCap + 48u && kSpillEnd <= kMxCap + 64u, "room for a chunk's worth of list overflow");
    __shared__ WaveLists s_wl[NW];
    __shared__ int s_delta[NW][32];             // per non-empty run: start - exclusive prefix
    // union slots of this instantiation: 4 register sets of 64 - or 5 without ids, where the id folds' registers are free:
    // a group of TWO cells of a dense medium (1.8 atoms per cell: 150 cells around it, 264 atoms) then shares one union, and
    // the group work is paid per 3.5 atoms instead of 1.8 (1 M atoms in one structure: 0.390 against 0.433 ms at 100 points,
    // 0.704 against 0.728 at 960); in sparse structures fewer groups are narrowed (the proteome: -0.7 %)
    constexpr int NS = HAS_ID ? 4 : 5;
    // Without ids the record's id word is free: it carries sr^2, and the record's last float R = r + probe instead of r - what
    // the atom loop would otherwise compute from r in all 64 lanes alike, per atom (four vector instructions fewer per atom:
    // 3.076 -> 3.043 ms over twelve interleaved rounds).  The same operations on the same operands, made where lane = atom.
    constexpr bool kHoist = !HAS_ID;
    constexpr uint32_t kUnion = 64u * (uint32_t)NS;
    __shared__ uint32_t s_mask[NW][2 * NS];     // run-start markers of the union's flat positions
    __shared__ __attribute__((aligned(16))) uint32_t s_blk[NW][8];  // where the wave's blocks of atoms are (see "persistent waves")
    constexpr uint32_t kWaveAtoms = MULTI ? kMxAtomsMulti : kMxAtoms;  // (the launch keeps atoms_per_wave within it)
    __shared__ float4 s_atom[NW][kWaveAtoms];   // the wave's atoms (x, y, z, r): broadcast reads per atom instead of
    __shared__ uint2 s_aux[NW][kWaveAtoms];     // readlanes; (id fold, 1 / (2 (r + probe)) correctly rounded)

    const float4 *__restrict__ sorted_xyzr = a.sorted_xyzr;
    const uint32_t *__restrict__ sorted_id32 = a.sorted_id32;
    const uint32_t *__restrict__ cells = a.cells;
    const uint32_t n_atoms = a.n_atoms;
    const uint32_t lane = lane_id();
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t n_points = a.n_points;  // <= 128 unless MULTI
    const uint32_t n_fused = a.n_fused;    // points [n_fused, n_points): the remainder rule (at most kFastMaxRem)
    const uint32_t NP = MULTI ? (n_points + 15u) & ~15u : (uint32_t)NT * 16u;  // points covered by the tiles
    const uint32_t NPS = NP + 16u;       // stride of the f32 table
    const float probe = a.probe;
    const float neg_inf = __int_as_float(0xFF800000);
    const float nan_f = __int_as_float(0x7FC00000);

    WaveLists &wl = s_wl[w];
    // the lists start out as finite numbers (prep reads records beyond the list's end as padding)
    for (uint32_t i = lane; i < sizeof(WaveLists) / 16u; i += 64u) reinterpret_cast<float4 *>(&wl)[i] = make_float4(0.f, 0.f, 0.f, 0.f);

    // the same points as f16 operands of the filter, (z, y | x, -1) per point, behind the f32 table
    uint2 *s_pt16 = reinterpret_cast<uint2 *>(s_lat + 4u * NPS);
    auto lat_ld = [&](const uint32_t off) -> float { return s_lat[off]; };   // f32 table: component k of point i at k NPS + i
    auto pt16_ld = [&](const uint32_t i) -> uint2 { return s_pt16[i]; };
    // MULTI: behind them the patch table (Lattice::patches: one 16-byte entry per tile of 16 points, padded to whole
    // blocks of 64 entries) and one zero entry
    const uint32_t n_patches = MULTI ? (n_points + 15u) >> 4 : 0u;
    const uint32_t n_patches_pad = (n_patches + 63u) & ~63u;
    uint4 *s_patch = reinterpret_cast<uint4 *>(s_pt16 + NP);
    if (MULTI) {
        for (uint32_t i = threadIdx.x; i < n_patches_pad; i += 64u * NW) s_patch[i] = a.patches[i];
        if (threadIdx.x == 0) s_patch[n_patches_pad] = make_uint4(0u, 0u, 0u, 0u);
    }
    // ---- lattice as matrix operand: s_lat[k * NPS + i] = component k of point i ----
    for (uint32_t i = threadIdx.x; i < NPS; i += 64u * NW) {
        const bool live = i < n_points;
        const float4 q = live ? a.lat4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        s_lat[i] = q.z;
        s_lat[NPS + i] = q.y;
        s_lat[2 * NPS + i] = q.x;
        s_lat[3 * NPS + i] = live ? -1.0f : 0.0f;
        const mx_h4 h = {(_Float16)q.z, (_Float16)q.y, (_Float16)q.x, (_Float16)(live ? -1.0f : 0.0f)};  // round to nearest
        if (i < NP) s_pt16[i] = __builtin_bit_cast(uint2, h);
    }
    __syncthreads();

    // The launch covers the cell-sorted positions [lo, hi) (see k_occlusion_fast); each XCD gets a
    // contiguous piece.
    uint32_t lo = 0, hi = n_atoms;
    if (a.part == kOccHead) hi = min(hi, a.status->tail_atom_base);
    else if (a.part == kOccRest) lo = min(hi, a.status->tail_atom_base);
    const uint32_t apw = a.atoms_per_wave;  // <= kMxAtoms
    // ---- per-wave constants ----
    // after the fold of phase A lane l of register R1 holds point pidx1, of R2 point pidx1 + 64
    // (rows of 16 lanes = tiles {0, 2, 1, 3} and {4, 6, 5, 7}; NT < 8: the rows of the missing tiles repeat others)
    const uint32_t row = lane >> 4;
    const uint32_t pidx1 = 16u * (((row & 1u) << 1) | (row >> 1)) + (lane & 15u);
    const unsigned long long ok1 = ballot64(pidx1 < n_points);
    const unsigned long long ok2 = ballot64(pidx1 + 64u < n_points);  // (that also drops the repeated rows)
    // lanes of r1 / r2 that hold a remainder point (at most 128 points; MULTI looks at the point indices)
    // (NT >= 7: more than 96 points, so n_fused = n_points - n_points % W >= 82 with W <= 16: no remainder point among the first 64)
    const unsigned long long rem1 = HAS_REM && !MULTI && NT < 7 ? ballot64(pidx1 >= n_fused && pidx1 < n_points) : 0ull;
    const unsigned long long rem2 = HAS_REM && !MULTI ? ballot64(pidx1 + 64u >= n_fused && pidx1 + 64u < n_points) : 0ull;
    // The remainder points (at most kFastMaxRem = 4, lib.rs:163-218: plain products, `<=`) are columns of the filter like the
    // others, but a surviving one never joins the survivors' list - those points get a pass of their own on the vector ALU
    // with the reference's own expression (phase_b_rem), exact, so nothing of this kernel's decisions on them is left to a
    // certainty band or to the general kernel.  (Round 6: with the remainder points in the matrix rounds - four or eight
    // tiles with the band's minimum for every atom that had one alive - 100 points with 4 remainder points ran 5 % SLOWER
    // than 104 points with none: 3.42 against 3.25 ms; 1 M atoms x 964 points 9 % slower than x 960.)
    constexpr bool kRemApart = HAS_REM;  // (more than 128 points as well: the filter's trips pick the remainder points out, below)
    constexpr bool kPhaseBAtOnce = !MULTI;
    const unsigned long long okf1 = kRemApart ? ok1 & ~rem1 : ok1, okf2 = kRemApart ? ok2 & ~rem2 : ok2;  // the fused-rule points
    // row of the 5x5 block this lane looks up in a group's prologue (lanes 0..24), the group's own row (12) in lane 0:
    // its atoms - the group's among them - then come first in the union
    // The rows come CENTRE-OUT (by dy^2 + dz^2: the own row, its 4 neighbours, the 4 diagonal ones, ...; five bits per row,
    // twelve rows per constant) and the sweep takes the union's chunks in that order, so the list's first candidates are the
    // atom's row and the rows around it: what fills tile 0 behind the near candidates - an atom has about a dozen of those - is
    // then likely to occlude something.  (Round 6: with the rows in index order and the chunks swept from the last one down the
    // fillers came from the farthest rows: 3.291 -> 3.245 ms, -1.4 %, for nothing per atom.)
    const uint32_t rrow = lane < 12u ? (uint32_t)(0x72852820d16acecull >> (5u * lane)) & 31u
                          : lane < 24u ? (uint32_t)(0xa1017acde928c36ull >> (5u * (lane - 12u))) & 31u : lane == 24u ? 24u : 0u;
    const int rdz = (int)((rrow * 13u) >> 6) - 2;  // row / 5 - 2
    const int rdy = (int)rrow - (rdz + 2) * 5 - 2;
    // LDS addresses that depend on the lane only
    float *const candf = reinterpret_cast<float *>(&wl.cand[0]);
    const float *const a_tile = candf + (lane & 15u) * 4u + (lane >> 4);  // matrix operand A: component l >> 4 of record l & 15 of tile 0
    // filter operand: the candidates, in lanes 0..15 (block 0 of the four-block instruction).  MULTI: the same register
    // is the candidate operand of the patch test on the K = 16 instruction: k = 0..3 in lanes 0..15, k = 4..7 (|v|, 0, 0, 0)
    // in lanes 16..31, zeros above
    const uint2 *const a_c16 = !MULTI || lane < 16u ? &wl.c16[lane & 15u]
                               : lane < 32u ? &wl.vn16[lane & 15u] : reinterpret_cast<const uint2 *>(&s_patch[n_patches_pad]);
    uint2 *const c16_all = &wl.c16[0];                                      // (80 entries: 16 + the spare ones)
    const uint32_t lat_lane = (lane >> 4) * NPS;                            // matrix operand B: component l >> 4 of a point (offset into the f32 table)

    const uint2 pt_lo = pt16_ld(lane);
    const uint2 pt_hi = pt16_ld(64u + min(lane, 16u * (uint32_t)((NT > 4 ? NT : 5) - 4) - 16u + (lane & 15u)));
    // ---- persistent waves: every wave works through blocks of apw consecutive atoms until none is left ----
    // A workgroup's registers and LDS are held until its last wave ends; with a fixed share of atoms per wave, three of
    // four waves ended early and their slots stayed empty.  Here the range is cut into eight pieces, one per XCD (its
    // workgroups work through a contiguous piece, which their L2 sees once); a wave's first block is the one its
    // position in the launch gives it, the later ones it claims from its piece's counter, which starts behind the
    // first blocks.  All waves of an XCD end within one block's time of each other.  (No stealing from other pieces: at
    // the end of a launch some seven thousand waves would come by every counter, and that many atomics on one address
    // take longer than a block of atoms - measured: + 0.3 ms.)
    // What a wave needs to find its next block lives in LDS (s_blk), not in scalar registers: carried around the atom
    // loops they were spilled to vector-register lanes there (42 v_readlane / 15 v_writelane against 15 / 0) and the
    // launches with 100 points lost 3.5 %.
    constexpr bool kPersist = mx_persistent(MULTI);
    {
        const uint32_t n_wblocks = (hi - lo + apw - 1u) / apw;
        if (kPersist) {
            const uint32_t n_pieces = min(8u, gridDim.x);  // (a launch of fewer than eight workgroups: a piece each)
            const uint32_t per_piece = (n_wblocks + n_pieces - 1u) / n_pieces;
            const uint32_t piece = blockIdx.x % n_pieces;
            const uint32_t piece_first = min(piece * per_piece, n_wblocks);
            const unsigned long long cl = (unsigned long long)(a.claim + piece * kClaimStride);
            if (lane == 0) {
                s_blk[w][0] = lo + piece_first * apw;                                        // first atom of the piece
                s_blk[w][1] = min(per_piece, n_wblocks - piece_first);                       // its blocks
                s_blk[w][2] = ((gridDim.x - piece + n_pieces - 1u) / n_pieces) * NW;         // of them assigned by position: one per wave of the piece's workgroups
                s_blk[w][3] = (blockIdx.x / n_pieces) * NW + w;                              // this wave's (next) block
                s_blk[w][4] = (uint32_t)cl; s_blk[w][5] = (uint32_t)(cl >> 32);              // the piece's counter
                s_blk[w][6] = hi; s_blk[w][7] = apw;
            }
        } else if (lane == 0) {
            // one block per wave, one workgroup per NW blocks; each XCD gets a contiguous piece of the range
            uint32_t bid = blockIdx.x;
            const uint32_t per = gridDim.x / 8u;
            if (bid < per * 8u) bid = (bid % 8u) * per + bid / 8u;
            s_blk[w][0] = lo; s_blk[w][1] = n_wblocks; s_blk[w][3] = bid * NW + w; s_blk[w][6] = hi; s_blk[w][7] = apw;
        }
        wave_lds_fence();
    }
    for (;; ) {
    uint32_t w_begin, n_mine, hi_b;
    {
        const uint4 q0 = *reinterpret_cast<const uint4 *>(&s_blk[w][0]);
        const uint2 q1 = *reinterpret_cast<const uint2 *>(&s_blk[w][6]);
        const uint32_t in_piece = (uint32_t)__builtin_amdgcn_readfirstlane((int)q0.w);
        if (in_piece >= (uint32_t)__builtin_amdgcn_readfirstlane((int)q0.y)) break;
        const uint32_t apw_b = (uint32_t)__builtin_amdgcn_readfirstlane((int)q1.y);
        hi_b = (uint32_t)__builtin_amdgcn_readfirstlane((int)q1.x);
        w_begin = (uint32_t)__builtin_amdgcn_readfirstlane((int)q0.x) + in_piece * apw_b;
        n_mine = min(apw_b, hi_b - w_begin);
    }
    __builtin_amdgcn_s_setprio(kMxPrioStart);

    // ---- the wave's atoms, lane = atom ----
    const uint32_t pa = min(w_begin + lane, hi_b - 1u);
    const float4 mine = sorted_xyzr[pa];
    // (persistent waves: the pointers that only a block's start and end use are fetched from the kernel's argument
    // segment there, every time - held in scalar registers through the atom loops they were spilled)
    typedef const OccArgs3 __attribute__((address_space(4))) *ArgSegment;
    ArgSegment ka = (ArgSegment)__builtin_amdgcn_kernarg_segment_ptr();
    if (kPersist) asm volatile("" : "+s"(ka));
    const uint32_t my_sid = (kPersist ? ka->sid : a.sid)[pa];
    uint32_t my_id32 = 0;
    if (HAS_ID) my_id32 = sorted_id32[pa];
    uint32_t cx, cy, cz, my_shift;
    unsigned long long ok_atoms;
    {
        const StructGrid g = a.grids[my_sid];
        cell_coords(g, mine.x, mine.y, mine.z, cx, cy, cz);  // spatial_grid.rs:133-143
        my_shift = min((g.odd_radii >> 8) & 3u, kMxXShift);   // the structure's group width (device_types.h grid_group_shift)
        if (NS == 5 && my_shift == 0u && (float)g.n_atoms < 1.95f * (float)g.n_cells) my_shift = 1u;  // (320 slots hold two cells' union)
        // What the straight-line code relies on (f16 operands that hold every vector and limit, the three-step
        // quotient's tested range, the remainder rule's error bound): probe in [0, 32], 2R in [1, 192],
        // sr = r + max_r + 2 probe <= 64 and every radius of the structure in [0, 64] (the grid build's
        // odd_radii flag), hence |v| <= sr, 0 <= t, d2, R2 <= sr^2 and |limit| <= sr^2 / R < 2^13.  Anything
        // else (negative or NaN radii, huge spheres) goes to the general kernel.
        const float myR = mine.w + probe;
        const float my_sr = mine.w + g.max_r + 2.0f * probe;
        // ... and grids of at most 1024 cells per axis (the three cell coordinates share a register, below)
        // (the largest of the three: their bitwise OR passes 1024 as soon as one axis has exactly 1024 cells and another has
        // any, which left every atom of such a grid to the general kernel - tests/mx_cases.py range_dim_1024)
        ok_atoms = ballot64(myR >= 0.5f && my_sr <= 64.0f && probe >= 0.0f && probe <= 32.0f && (g.odd_radii & 1u) == 0u &&
                            max3u(g.dim_x, g.dim_y, g.dim_z) <= 1024u);
        if (lane < kWaveAtoms) {
            s_atom[w][lane] = kHoist ? make_float4(mine.x, mine.y, mine.z, myR) : mine;
            s_aux[w][lane] = make_uint2(kHoist ? __float_as_uint(my_sr * my_sr) : my_id32, __float_as_uint(1.0f / (2.0f * myR)));  // IEEE division: the correctly rounded reciprocal
        }
    }
    // the next block is claimed now and looked at when this one is done (an atomic on a counter that all waves of the
    // XCD share takes a few microseconds to come back)
    uint32_t next_claim = 0;
    if (kPersist && lane == 0)
        next_claim = atomicAdd(reinterpret_cast<uint32_t *>((unsigned long long)s_blk[w][4] | ((unsigned long long)s_blk[w][5] << 32)), 1u);
    // group starts: first atom, or (structure, y cell, z cell, block of x cells) differs from the atom before
    unsigned long long starts;
    uint32_t cxyz;  // cx | cy << 10 | cz << 20: what a group's prologue reads of its atoms (one register through the atom loops
                    // instead of three; larger coordinates are cut - such atoms are not ok_atoms and their groups are deferred)
    {
        cxyz = (cx & 1023u) | ((cy & 1023u) << 10) | ((cz & 1023u) << 20);
        const uint32_t bx = cx >> my_shift;
        const uint32_t p_sid = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)my_sid, 0x138, 0xf, 0xf, false);  // wave_shr:1
        const uint32_t p_cy = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cy, 0x138, 0xf, 0xf, false);
        const uint32_t p_cz = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cz, 0x138, 0xf, 0xf, false);
        const uint32_t p_bx = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)bx, 0x138, 0xf, 0xf, false);
        starts = ballot64(lane == 0u || p_sid != my_sid || p_cy != cy || p_cz != cz || p_bx != bx);
    }
    __builtin_amdgcn_s_setprio(0);
    wave_lds_fence();  // the atoms' LDS records are read from here on
    const unsigned long long mine_mask = n_mine >= 64u ? ~0ull : ((1ull << n_mine) - 1ull);

    constexpr uint32_t kDeferred = 0xFFFFFFFFu;
    uint32_t my_result = kDeferred;  // lane `at`: exposed points | candidates << 16

    const mx_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const mx_f16v zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    uint32_t g0 = 0;
    uint32_t cur_sid = 0xFFFFFFFFu;
    // grid of the current structure (uniform; reloaded when a group belongs to another structure)
    uint32_t dim_x = 1, dim_y = 1, dim_z = 1, cell_base = 0, rel_base = 0;
    bool rel16 = false;  // the structure's cell entries: 16-bit, relative to rel_base (else 32-bit absolute)
    float max_r = 0.f;
    bool not_mine = false;  // the current structure belongs to the other instantiation of the pair (its ids matter / do not)
    while (g0 < n_mine) {
        // ---- the group [g0, g1): until the next group start, narrowed if its union is too large ----
        uint32_t g1;
        {
            const unsigned long long later = starts & mine_mask & ~((2ull << g0) - 1ull);
            g1 = later ? (uint32_t)__builtin_ctzll(later) : n_mine;
        }
        const uint32_t sid_g = readlane_u(my_sid, g0);
        if (sid_g != cur_sid) {
            const StructGrid g = a.grids[sid_g];
            dim_x = (uint32_t)__builtin_amdgcn_readfirstlane((int)g.dim_x);
            dim_y = (uint32_t)__builtin_amdgcn_readfirstlane((int)g.dim_y);
            dim_z = (uint32_t)__builtin_amdgcn_readfirstlane((int)g.dim_z);
            cell_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)g.cell_base);
            rel16 = __builtin_amdgcn_readfirstlane((int)g.in_lds) != 0;
            rel_base = rel16 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)g.sorted_base) : 0u;
            max_r = uniform_f(g.max_r);
            not_mine = a.ids_check != 0u && (((uint32_t)__builtin_amdgcn_readfirstlane((int)g.odd_radii) >> 1) & 1u) != (HAS_ID ? 1u : 0u);
            cur_sid = sid_g;
        }
        if (not_mine) {  // (its atoms' results stay "deferred": nothing is stored for them here)
            // (persistent waves: the block's first group is where the next block's claim is put down - below, behind the
            // gathers that hide its latency; a first group that is skipped puts it down here)
            if (kPersist && g0 == 0u && lane == 0u) s_blk[w][3] = s_blk[w][2] + next_claim;
            g0 = g1;
            continue;
        }
        const uint32_t gxyz = readlane_u(cxyz, g0);
        const uint32_t gcy = (gxyz >> 10) & 1023u, gcz = gxyz >> 20;
        const uint32_t cx_first = gxyz & 1023u;
        __builtin_amdgcn_s_setprio(kMxPrioGroup);
        uint32_t U, run_start, excl, n_chunk;
        for (;;) {
            const uint32_t cx_last = readlane_u(cxyz, g1 - 1u) & 1023u;
            const uint32_t x_lo = cx_first >= 2u ? cx_first - 2u : 0u;
            const uint32_t x_hi = min(cx_last + 2u, dim_x - 1u);
            // the 25 x-runs (lane = row of the 5x5 block): cells [x_lo, x_hi] of row (gcy + dy, gcz + dz)
            const uint32_t yy = gcy + (uint32_t)rdy, zz = gcz + (uint32_t)rdz;
            uint32_t run_len = 0;
            run_start = 0;
            if (lane < 25u && yy < dim_y && zz < dim_z) {
                const uint32_t c0 = cell_base + (zz * dim_y + yy) * dim_x + x_lo;
                uint32_t first, behind;
                load_cell_start2(cells, c0, c0 + (x_hi - x_lo) + 1u, rel16, first, behind);
                run_len = behind - first;
                run_start = rel_base + first;
            }
            const uint32_t incl = scan_lanes32(run_len);
            U = readlane_u(incl, 31);
            excl = incl - run_len;
            if (U <= kUnion || cx_last == cx_first) {
                // flat positions -> atoms: run r > 0 (of the non-empty ones) is marked one position
                // before its start, so the run of position f is (marks below f)
                const bool run_ne = run_len > 0u;
                const unsigned long long ne_mask = ballot64(run_ne);
                if (lane < 2u * (uint32_t)NS) s_mask[w][lane] = 0u;
                if (run_ne) s_delta[w][mbcnt64(ne_mask)] = (int)run_start - (int)excl;
                wave_lds_fence();
                if (run_ne && excl != 0u && excl <= kUnion) atomicOr(&s_mask[w][(excl - 1u) >> 5], 1u << ((excl - 1u) & 31u));
                wave_lds_fence();
                break;
            }
            // too many atoms around these cells: keep the lower half of the group's x cells
            const uint32_t mid = (cx_first + cx_last) >> 1;
            const unsigned long long other = ballot64((cxyz & 1023u) > mid) & ~((1ull << g0) - 1ull) & mine_mask;
            g1 = (uint32_t)__builtin_ctzll(other);
        }
        n_chunk = (min(U, kUnion) + 63u) >> 6;
        // the group's own row is the first run (lane 0): position of atom g0 inside the union
        const uint32_t self0 = w_begin + g0 - readlane_u(run_start, 0);

        // ---- the union in registers: lane = slot of chunk c ----
        float4 un[NS];
        uint32_t uid[NS];
        {
            const uint32_t mword = lane < 2u * (uint32_t)NS ? s_mask[w][lane] : 0u;
            uint32_t base_rank = 0;
#pragma unroll
            for (int c = 0; c < NS; c++) {
                // (a chunk that is not swept is never read, and of the slots past the union's end only x - NaN: never
                // accepted - and the id fold are: no instruction spent on the rest)
                asm volatile("" : "=v"(un[c].x), "=v"(un[c].y), "=v"(un[c].z), "=v"(un[c].w), "=v"(uid[c]));
                if ((uint32_t)c < n_chunk) {
                    const unsigned long long mask64 =
                        (unsigned long long)readlane_u(mword, 2u * (uint32_t)c) |
                        ((unsigned long long)readlane_u(mword, 2u * (uint32_t)c + 1u) << 32);
                    const uint32_t rnk = base_rank + mbcnt64(mask64);
                    base_rank += (uint32_t)__popcll(mask64);
                    const uint32_t f = 64u * (uint32_t)c + lane;
                    un[c].x = nan_f;
                    uid[c] = 0u;  // (an atom whose own fold is 0 meets it here and goes to the general kernel: correct, rare)
                    if (f < U) {
                        const uint32_t q = (uint32_t)((int)f + s_delta[w][rnk]);
                        un[c] = sorted_xyzr[q];
                        if (HAS_ID) uid[c] = sorted_id32[q];
                    }
                }
            }
        }
        __builtin_amdgcn_s_setprio(0);
        // (the claim has come back by now - it is older than the gathers above -, and no register has to carry it
        // through the atom loops)
        if (kPersist && g0 == 0u && lane == 0u) s_blk[w][3] = s_blk[w][2] + next_claim;
        // The general kernel takes the whole group when a single cell has more than 256 atoms around it, when a
        // radius is out of range (ok_atoms), or when the group's atoms do not all sit in the union's first
        // chunk (the sweep excludes an atom from its own list there and nowhere else).
        if (U > kUnion || (~ok_atoms & ((2ull << (g1 - 1u)) - (1ull << g0))) != 0ull || self0 + (g1 - g0) > 64u) {
            if (lane >= g0 && lane < g1) a.work_list_out[atomicAdd(a.work_count_out, 1u)] = w_begin + lane;
            g0 = g1;
            continue;
        }

        // ---- the group's atoms, one after the other ----
        // The loop exists once per chunk count of the union (the count is the group's): no test of it in front of every
        // chunk of every atom, and the compiler schedules the chunks of a sweep as one block (-1.8 % / -1.2 % on the two
        // bench workloads for 2.2 times the code, against one loop that reads the count at run time).
        auto atoms_of_group = [&](auto n_chunk_tag) {
        constexpr uint32_t NCH = decltype(n_chunk_tag)::value;  // 0: not specialised (the count is read at run time)
        uint32_t at_v = vgpr_u(g0);       // the atom's index in the wave and its position in the union (chunk 0),
        // lane l is the atom's own slot of chunk 0 when l == self0 + (at - g0): l - self0 + g0 == at, the left side made once per group
        const uint32_t self_v = lane - vgpr_u(self0) + vgpr_u(g0);
        for (uint32_t at = g0; at < g1; at++, at_v = vadd_u(at_v, 1u)) {
            const float4 me = s_atom[w][at_v];  // (one address in all lanes: broadcast reads)
            const uint2 aux = s_aux[w][at_v];
            const float mx = me.x, my = me.y, mz = me.z, mr = me.w;
            const uint32_t mid = aux.x;
            const float inv2R = __uint_as_float(aux.y);   // 1.0 / (2.0 * R), correctly rounded (lane = atom prologue)
            const float R = kHoist ? mr : mr + probe;   // lib.rs:101 (kHoist: the record holds r + probe)
            const float R2 = R * R;                     // lib.rs:102
            const float twoR = 2.0f * R;                // lib.rs:136
            const float sr = kHoist ? 0.f : mr + max_r + 2.0f * probe; // spatial_grid.rs:307
            const float sr2 = kHoist ? __uint_as_float(aux.x) : sr * sr;  // spatial_grid.rs:308 (kHoist: the same product, from the record)
            const float near2 = kMxNearScale2 * R2;
            // -- sweep: the candidate rule on every union slot, the chunks in the union's order (the own row and the rows
            // around it first: see rrow; the order of candidates is free)
            uint32_t K = 0;
            uint32_t id_min = 0xFFFFFFFFu;  // per lane: min over its slots of (id fold xor own fold); 0 = an equal fold in the union
            auto sweep_chunk = [&](const float4 &o, uint32_t oid, const int c) {
                const float dx = mx - o.x, dy = my - o.y, dz = mz - o.z;
                const float d2 = dx * dx + dy * dy + dz * dz;                 // spatial_grid.rs:321
                // spatial_grid.rs:335; the atom itself always sits in chunk 0
                const unsigned long long m = c == 0 ? ballot64(d2 <= sr2) & ballot64(self_v != at) : ballot64(d2 <= sr2);
                // equal id folds (spatial_grid.rs:314, lib.rs:124: same atom) are decided on the full ids elsewhere: ANY slot
                // of the union with the atom's fold - accepted or not, its own slot excepted - sends it there
                if (HAS_ID) id_min = min(id_min, c == 0 ? vsel_or_ones(ballot64(self_v != at), oid ^ mid) : oid ^ mid);
                // a list longer than the buffer spills into the lists behind it (dead during the sweep) and ends
                // on the struct's last record: such an atom is deferred
                if (c == 0 ? (d2 <= sr2) & (self_v != at) : d2 <= sr2) {
                    if ((uint32_t)(c + 1) * 64u > kSpillEnd) wl.cand[min(mbcnt64_add(m, K), kSpillEnd - 1u)] = o;  // (at most 64 c accepted before chunk c)
                    else (&wl.cand[K])[mbcnt64(m)] = o;  // (the list's end as a scalar base: no copy of K into a vector register)
                }
                K += (uint32_t)__popcll(m);
            };
            sweep_chunk(un[0], uid[0], 0);
            if (NCH ? NCH > 1u : n_chunk > 1u) sweep_chunk(un[1], uid[1], 1);
            if (NCH ? NCH > 2u : n_chunk > 2u) sweep_chunk(un[2], uid[2], 2);
            if (NCH ? NCH > 3u : n_chunk > 3u) sweep_chunk(un[3], uid[3], 3);
            if constexpr (NS == 5) {
                if (NCH ? NCH > 4u : n_chunk > 4u) sweep_chunk(un[4], uid[4], 4);
            }
            // the rare cases: no candidate at all (every point exposed), more candidates than the list holds or an equal
            // id fold (the general kernel takes the atom: my_result of lane `at` stays "deferred")
            if (K - 1u >= (uint32_t)kMxCap || (HAS_ID && ballot64(id_min == 0u) != 0ull)) {
                if (K == 0u && !(HAS_ID && ballot64(id_min == 0u) != 0ull)) {
                    if (lane == at) my_result = n_points;  // lib.rs:156-159 with an empty list (K = 0 in the upper half)
                } else if (lane == 0) {
                    a.work_list_out[atomicAdd(a.work_count_out, 1u)] = w_begin + at;
                }
                wave_lds_fence();
                continue;
            }
            wave_lds_fence();

            // -- prep (lane = candidate), in place: record (x, y, z, r) -> operand record (vz, vy, vx, limit).
            // Lanes beyond the list read whatever the buffer holds (finite numbers) and get limit -inf.
            auto prep_pass = [&](const uint32_t k0, const bool first) {
                const uint32_t k = k0 + lane;
                const unsigned long long live = ballot64(k < K);
                const float4 o = wl.cand[k];
                float4 e;  // (z, y, x, limit): the k order of the matrix operand
                e.z = mx - o.x; e.y = my - o.y; e.x = mz - o.z;       // lib.rs:129-131
                const float d2 = e.z * e.z + e.y * e.y + e.x * e.x;   // lib.rs:132-133
                const float tj = o.w + probe;                         // spatial_grid.rs:336
                const float t = tj * tj;                              // spatial_grid.rs:339
                // lib.rs:136: (t - d2 - R2) / twoR, the IEEE quotient in three operations: with y the correctly
                // rounded reciprocal of the divisor, q0 = RN(a y), r = a - q0 d (exact in an fma) and RN(q0 + r y)
                // is the correctly rounded a / d (Markstein; tools/check_division.c compares all numerators of the
                // range this kernel admits against `/` for random and worst-case divisors; -0 / d gives +0, which
                // no comparison distinguishes)
                const float num = t - d2 - R2;
                const float q0 = num * inv2R;
                const float rr = __builtin_fmaf(-q0, twoR, num);
                e.w = vsel_f(live, neg_inf, __builtin_fmaf(rr, inv2R, q0));  // padding: a finite vector, limit -inf: never occludes
                uint32_t slot = k;
                if (first) {
                    // near candidates (strong occluders) first; a permutation inside this pass's slots
                    // (padding lanes come after every near lane: they keep slot k)
                    const unsigned long long mN = ballot64(d2 < near2) & live;
                    const uint32_t before = mbcnt64_add(mN, 0u);
                    slot = vsel(mN, (uint32_t)__popcll(mN) + k - before, before);
                }
                wave_lds_fence();  // every lane has read its record before any lane writes
                wl.cand[slot] = e;
                if (first) {
                    // Tile 0 once more as the f16 operand of the filter (phase A).  The filter may only kill
                    // a point the exact test kills too: its limit is lowered by more than every rounding
                    // can add to dot - limit.  s (rounded to nearest) and v (towards zero) are off by at
                    // most 2^-11 and 2^-10 of their size, the products of f16 values are exact in f32 and
                    // |s_k| <= 1: |dot16 - dot| <= 0.8 * 2^-9 (|vx| + |vy| + |vz|); 3e-4 covers operands an
                    // f16 pipeline may flush and the few ulps between the fused and the plain dot product (the
                    // remainder points' rule).  The limit itself is rounded DOWN (2^-9 of its size covers
                    // the conversion's 2^-10 in either direction).  f16 holds every operand: |v| <= sr <= 64 and
                    // |limit| < 2^13 for the atoms that get here (ok_atoms).  Slots 16 and up land in
                    // the array's spare entries (at most two lanes per entry).
                    const float m3 = fabsf(e.x) + fabsf(e.y) + fabsf(e.z);
                    float lim = e.w - __builtin_fmaf(m3, 0x1.8p-9f, 3e-4f);
                    lim = __builtin_fmaf(-0x1p-9f, fabsf(lim), lim);
                    c16_all[min(slot, 16u + lane)] = make_uint2(pack_f16_rtz(e.x, e.y), pack_f16_rtz(e.z, lim));
                    // MULTI: |v| rounded up (the square root is good to an ulp, the conversion rounds towards zero by at
                    // most 2^-10 of the value: 1.002 covers both) for the patch test; written after the line above,
                    // whose spare entries overlap this array's first 16
                    if (MULTI) (&wl.vn16[0])[min(slot, 16u + lane)] = make_uint2(pack_f16_rtz(1.002f * __builtin_sqrtf(d2), 0.f), 0u);
                }
            };
            prep_pass(0u, true);
            if (K > 64u) prep_pass(64u, false);
            wave_lds_fence();

            // -- point tests.
            // PHASE A, a filter on the f16 matrix instruction: tile 0 against all points (the remainder points
            // are columns like the others).  D = dot16 - limit16 < 0 proves dot < limit (see prep): such points
            // are dead.  PHASE B, exact: the others, 16 per instruction, against every tile with
            // v_mfma_f32_16x16x4_f32, whose result is bit for bit the reference's dot - limit for the
            // fused-rule points; the remainder points' plain-product rule is evaluated as written (phase_b_rem).
            const uint32_t n_tiles = (K + 15u) >> 4;
            uint32_t exposed = 0u;
            {
                uint32_t n_sv = 0;
                unsigned long long rem_left = 0ull;  // (at most 128 points) the remainder points' lanes of r1 | r2 that the filter left alive
                uint32_t rem_alive4 = 0u;            // (more points) bit q: remainder point n_fused + q is alive after the filter
                // PHASE B for a handful of survivors (at most SW = 4 or 8, none of them a remainder point), on the vector
                // ALU: lane = (survivor l & (SW - 1), candidate l >> log2 SW of a pass of 64 / SW candidates), the
                // reference's fused chain and `<` (lib.rs:143-146) per pair.  A matrix round costs the same for 1 or 16
                // survivors (about 45 cycles per candidate tile); this costs 6 instructions per pass.
                auto phase_b_small = [&](const uint32_t sw_log2) {
                    const uint32_t SW = 1u << sw_log2, CPP = 64u >> sw_log2;
                    wl.pts[n_sv + lane] = (uint16_t)NP;  // (lanes of survivors that do not exist read the zero point; masked out below)
                    wave_lds_fence();
                    uint32_t ln = lane;
                    asm volatile("" : "+v"(ln));  // (addresses derived here, not kept in registers across the kernel: they would spill)
                    const uint32_t idx = (uint32_t)wl.pts[ln & (SW - 1u)];
                    const float pz = lat_ld(idx), py = lat_ld(NPS + idx), px = lat_ld(2u * NPS + idx);
                    const float4 *cp = &wl.cand[ln >> sw_log2];
                    unsigned long long km = 0ull;
                    // two passes per trip, their records read up front (prep wrote whole passes of 64 records: the ones
                    // past the list's end have limit -inf)
                    for (uint32_t k0 = 0; k0 < K; k0 += 2u * CPP, cp += 2u * CPP) {
                        float4 e[2];  // (vz, vy, vx, limit)
#pragma unroll
                        for (int q = 0; q < 2; q++) e[q] = cp[(uint32_t)q * CPP];
#pragma unroll
                        for (int q = 0; q < 2; q++) {
                            const float dot = __builtin_fmaf(px, e[q].z, __builtin_fmaf(py, e[q].y, pz * e[q].x));  // lib.rs:143-144
                            km |= ballot64(dot < e[q].w);                                                          // lib.rs:146
                        }
                    }
                    uint32_t k32 = (uint32_t)km | (uint32_t)(km >> 32);
                    k32 |= k32 >> 16;
                    k32 |= k32 >> 8;
                    if (sw_log2 == 2u) k32 |= k32 >> 4;
                    exposed += n_sv - (uint32_t)__popc(k32 & ((1u << n_sv) - 1u));
                    n_sv = 0;
                    wave_lds_fence();
                };
                auto phase_b = [&]() {
                    if (n_sv <= 4u) { phase_b_small(2u); return; }
                    if (n_sv <= 8u) { phase_b_small(3u); return; }
                    // the last round's spare columns: a point with all components zero (dot - limit = +0: never occluded)
                    wl.pts[n_sv + lane] = (uint16_t)NP;
                    wave_lds_fence();
                    uint32_t killed = 0;
                    for (uint32_t s0 = 0; s0 < n_sv; s0 += 16u) {
                        const uint32_t idx = (uint32_t)wl.pts[s0 + (lane & 15u)];
                        const float bv = lat_ld(lat_lane + idx);  // B operand: component l >> 4 of survivor j
                        uint32_t acc = 0u;  // unsigned maximum of the bit patterns of dot - limit: > 0x80000000 iff one is negative
                        // (prep wrote whole passes of 64 records, padding included)
                        const float *ap = a_tile;  // A operand: component l >> 4 of candidate l & 15 of a tile
                        for (uint32_t ct = 0; ct < n_tiles; ct++, ap += 64) {
                            const mx_f4 d = __builtin_amdgcn_mfma_f32_16x16x4f32(*ap, bv, zero4, 0, 0, 0);
                            acc = max3u(acc, __float_as_uint(d[0]), __float_as_uint(d[1]));
                            acc = max3u(acc, __float_as_uint(d[2]), __float_as_uint(d[3]));
                        }
                        const unsigned long long km = ballot64(is_negative_bits(acc));
                        uint32_t k16 = (uint32_t)km | (uint32_t)(km >> 32);
                        k16 |= k16 >> 16;
                        killed += (uint32_t)__popc(k16 & 0xFFFFu);
                    }
                    exposed += n_sv - killed;
                    n_sv = 0;
                    wave_lds_fence();
                };
                // The remainder points that the filter left alive (bit q of `alive`: point n_fused + q), exact: lane = (point
                // l & 3, candidate l >> 2 of a pass of 16), plain products and `<=` as lib.rs:185-186,206-207 write them
                // (the reference's `current_nb` only changes the order of the tests).  Two passes per trip, like the small
                // phase B; prep wrote whole passes of 64 records, the ones past the list's end with limit -inf.
                auto phase_b_rem = [&](const uint32_t alive) {
                    uint32_t ln = lane;
                    asm volatile("" : "+v"(ln));  // (addresses derived here, not kept in registers across the kernel: they would spill)
                    const uint32_t idx = n_fused + (ln & 3u);  // (behind the last point: zero entries of the table - their lanes' verdicts are masked out)
                    const float pz = lat_ld(idx), py = lat_ld(NPS + idx), px = lat_ld(2u * NPS + idx);
                    const float4 *cp = &wl.cand[ln >> 2];
                    unsigned long long km = 0ull;
                    for (uint32_t k0 = 0; k0 < K; k0 += 32u, cp += 32u) {
                        float4 e[2];  // (vz, vy, vx, limit)
#pragma unroll
                        for (int q = 0; q < 2; q++) e[q] = cp[(uint32_t)q * 16u];
#pragma unroll
                        for (int q = 0; q < 2; q++) {
                            const float dot = px * e[q].z + py * e[q].y + pz * e[q].x;  // lib.rs:185,206
                            km |= ballot64(dot <= e[q].w);                              // lib.rs:186,207
                        }
                    }
                    uint32_t k32 = (uint32_t)km | (uint32_t)(km >> 32);
                    k32 |= k32 >> 16;
                    k32 |= k32 >> 8;
                    k32 |= k32 >> 4;
                    exposed += (uint32_t)__popc(alive & ~k32 & 15u);
                };
                // the candidates' f16 operand lives in lanes 0..15 = block 0 of the instruction, which broadcasts it to
                // its other three blocks (what lanes 16..63 hold is not looked at)
                const uint2 av16 = *a_c16;
                // mu: per lane (point l & 15 of tile t, candidates 4 (l >> 4) .. + 3) the unsigned maximum of the
                // bit patterns of D; then maxima over the four candidate quarters (lanes l, l ^ 16, l ^ 32,
                // l ^ 48): rows of 16 lanes = tiles 0, 2, 1, 3 of the four
                auto fold4 = [&](uint32_t (&mu)[4], const int nt) -> uint32_t {
                    if (nt == 3) mu[3] = mu[2];
                    const auto swa = __builtin_amdgcn_permlane32_swap(mu[0], mu[1], false, false);
                    const uint32_t ca = max(swa[0], swa[1]);  // lanes 0..31: tile 0, lanes 32..63: tile 1
                    uint32_t cb = ca;
                    if (nt > 2) {
                        const auto swb = __builtin_amdgcn_permlane32_swap(mu[2], mu[3], false, false);
                        cb = max(swb[0], swb[1]);
                    }
                    const auto sw = __builtin_amdgcn_permlane16_swap(ca, cb, false, false);
                    return max(sw[0], sw[1]);  // rows: tiles 0, 2, 1, 3 (nt == 2: 0, 0, 1, 1; nt == 3: 0, 2, 1, 2)
                };
                // ONE v_mfma_f32_16x16x4_4b_f16: four independent 16 x 16 x 4 products, block b = the 16 candidates
                // (block 0's operand broadcast, cbsz:2) against the 16 points the lanes 16 b .. 16 b + 15 supply;
                // result registers 4 b .. 4 b + 3 are block b's (tools/check_mfma4b.hip)
                auto filter4 = [&](const uint2 bt4, const int nt) -> uint32_t {
                    uint32_t mu[4];
                    const mx_f16v d16 = __builtin_amdgcn_mfma_f32_16x16x4f16(__builtin_bit_cast(mx_h4, av16), __builtin_bit_cast(mx_h4, bt4), zero16, 2, 0, 0);
#pragma unroll
                    for (int t = 0; t < nt; t++)
                        mu[t] = max3u(max(__float_as_uint(d16[4 * t]), __float_as_uint(d16[4 * t + 1])), __float_as_uint(d16[4 * t + 2]), __float_as_uint(d16[4 * t + 3]));
                    return fold4(mu, nt);
                };
                if (MULTI) {
                    // PATCH TEST.  The points come in compact patches of 16 (one per tile; context.cpp bisect_points) with
                    // a centre c and a radius eps: every point s of the patch has s . v <= c . v + eps |v|.  A candidate of
                    // tile 0 with c . v + eps |v| < limit therefore occludes the whole tile, and the tile is not looked at
                    // again.  As a matrix product: candidates (vz, vy, vx, limit', |v|) x patches (cz, cy, cx, -1, eps)
                    // on v_mfma_f32_16x16x16_f16 (K = 16, five of them used), limit' being the filter's lowered limit: its
                    // margin covers c16 . v16 against c . v exactly as it does for a point (|c_k| <= 1, c rounded to nearest,
                    // prep); |v| and eps are rounded up.  D < 0 proves the tile dead, remainder points included (real
                    // s . v below the limit by more than the margin makes the plain-product `<=` true as well).
                    wave_lds_fence();  // (av16 is in registers: the c16 / vn16 entries now hold the list of live tiles)
                    uint8_t *const tiles = reinterpret_cast<uint8_t *>(&wl.c16[0]);  // [0, 96): live tiles; [128, 192): other lanes' stores
                    uint32_t n_live = 0;
                    uint32_t ln = lane;
                    asm volatile("" : "+v"(ln));  // (addresses derived from here on are not kept in registers across the kernel: they would spill)
                    const uint32_t l15 = ln & 15u, lrow = ln >> 4;
                    for (uint32_t pb = 0; pb < n_patches; pb += 64u) {
                        uint32_t mu[4];
#pragma unroll
                        for (int t = 0; t < 4; t++) {
                            const uint4 pe = s_patch[pb + 16u * (uint32_t)t + l15];
                            const uint2 bop = lrow == 1u ? make_uint2(pe.z, pe.w) : make_uint2(pe.x, pe.y);  // (k >= 8: times zero)
                            const mx_f4 d = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(mx_h4, av16), __builtin_bit_cast(mx_h4, bop), zero4, 0, 0, 0);
                            mu[t] = max3u(max(__float_as_uint(d[0]), __float_as_uint(d[1])), __float_as_uint(d[2]), __float_as_uint(d[3]));
                        }
                        const uint32_t rp = fold4(mu, 4);  // lane l: patch pb + pidx1
                        const unsigned long long live = ballot64(!is_negative_no_nan(rp) && pb + pidx1 < n_patches);
                        tiles[vsel(live, 128u + ln, mbcnt64_add(live, n_live))] = (uint8_t)(pb + pidx1);
                        n_live += (uint32_t)__popcll(live);
                    }
                    wave_lds_fence();
                    // FILTER on the live tiles, eight per trip (two instructions of four tiles)
                    const uint32_t rowt = ((lrow & 1u) << 1) | (lrow >> 1);  // the tile of the four whose points the fold leaves in this lane's row
                    for (uint32_t t0 = 0; t0 < n_live; t0 += 8u) {
                        // (list entries past the end repeat the last tile; their lanes are masked out below)
                        const uint32_t tb1 = (uint32_t)tiles[min(t0 + lrow, n_live - 1u)], tb2 = (uint32_t)tiles[min(t0 + 4u + lrow, n_live - 1u)];
                        const uint32_t tr1 = (uint32_t)tiles[min(t0 + rowt, n_live - 1u)], tr2 = (uint32_t)tiles[min(t0 + 4u + rowt, n_live - 1u)];
                        const uint32_t r1 = filter4(s_pt16[16u * tb1 + l15], 4);
                        const uint32_t r2 = filter4(s_pt16[16u * tb2 + l15], 4);
                        const uint32_t p1 = 16u * tr1 + l15, p2 = 16u * tr2 + l15;
                        unsigned long long sv1 = ballot64(!is_negative_no_nan(r1) && t0 + rowt < n_live && p1 < n_points);
                        unsigned long long sv2 = ballot64(!is_negative_no_nan(r2) && t0 + 4u + rowt < n_live && p2 < n_points);
                        if (HAS_REM) {
                            // the remainder points (behind the fused-rule points: the last tile's, at most four) never join the
                            // list; the ones alive are noted for their own exact pass
                            const unsigned long long f1 = ballot64(p1 < n_fused), f2 = ballot64(p2 < n_fused);
                            if (((sv1 & ~f1) | (sv2 & ~f2)) != 0ull) {
#pragma unroll
                                for (uint32_t q = 0; q < kFastMaxRem; q++)
                                    if (((sv1 & ballot64(p1 == n_fused + q)) | (sv2 & ballot64(p2 == n_fused + q))) != 0ull) rem_alive4 |= 1u << q;
                            }
                            sv1 &= f1;
                            sv2 &= f2;
                        }
                        const uint32_t S1 = (uint32_t)__popcll(sv1), S = S1 + (uint32_t)__popcll(sv2);
                        if (S != 0u) {
                            wl.pts[vsel(sv1, kDummyPts + ln, mbcnt64_add(sv1, n_sv))] = (uint16_t)p1;
                            wl.pts[vsel(sv2, kDummyPts + ln, mbcnt64_add(sv2, n_sv + S1))] = (uint16_t)p2;
                            n_sv += S;
                            if (n_sv > kSurvivors - 128u) phase_b();  // room for the next trip's survivors
                        }
                    }
                }
                for (uint32_t pg = 0; !MULTI && pg < 1u; pg++) {
                    // mu: per lane (point l & 15 of tile t, candidates 4 (l >> 4) .. + 3) the unsigned maximum of the
                    // bit patterns of D; then maxima over the four candidate quarters (lanes l, l ^ 16, l ^ 32,
                    // l ^ 48): lane l of r1 holds point pidx1, of r2 point pidx1 + 64.  Two halves of four tiles
                    // (one instruction, 16 result registers each).
                    // tiles t0 .. t0 + nt - 1 (nt = 2, 3 or 4): lane l supplies point 16 (t0 + (l >> 4)) + (l & 15), the lanes of
                    // a tile that does not exist repeat the last one
                    // (both point operands sit in registers for the wave's lifetime: pt_lo, pt_hi)
                    const uint32_t r1 = filter4(pt_lo, 4);
                    const uint32_t r2 = filter4(pt_hi, NT - 4);
                    const unsigned long long a1 = ballot64(!is_negative_no_nan(r1)), a2 = ballot64(!is_negative_no_nan(r2));  // (masked below: okf1 / okf2, rem1 / rem2)
                    const unsigned long long sv1 = a1 & okf1, sv2 = a2 & okf2;
                    const uint32_t S1 = (uint32_t)__popcll(sv1), S = S1 + (uint32_t)__popcll(sv2);
                    if (kRemApart) rem_left = (NT < 7 ? a1 & rem1 : 0ull) | (a2 & rem2);
                    if (S != 0u) {
                        // survivors append their point index; the other lanes store to dummy entries behind the list
                        // (pidx1 + 64 is computed here: kept in a register of its own it was spilled, and reloaded per atom)
                        uint32_t p1 = kPersist ? lane : pidx1;
                        asm volatile("" : "+v"(p1));
                        if (kPersist) p1 = (p1 & 15u) | ((p1 & 16u) << 1) | ((p1 >> 1) & 16u);  // (= pidx1, from the lane: a register less)
                        wl.pts[vsel(sv1, kDummyPts + lane, mbcnt64_add(sv1, 0u))] = (uint16_t)p1;
                        wl.pts[vsel(sv2, kDummyPts + lane, mbcnt64_add(sv2, S1))] = (uint16_t)(p1 + 64u);
                        n_sv += S;
                        if (kPhaseBAtOnce) phase_b();  // (one test of S for the stores and the exact tests)
                    }
                }
                if (!kPhaseBAtOnce && n_sv != 0u) phase_b();
                if (kRemApart && MULTI && rem_alive4 != 0u) phase_b_rem(rem_alive4);
                if (kRemApart && !MULTI && rem_left != 0ull) {
                    // lane of point n_fused in r1 / r2 (rows of 16 lanes = tiles 0, 2, 1, 3): the remainder points follow it,
                    // inside one row (n_fused is a multiple of the lane count W <= 16, and there are fewer than W of them - at most 4)
                    const uint32_t pf = n_fused & 63u, t = pf >> 4;
                    phase_b_rem((uint32_t)(rem_left >> (16u * (((t & 1u) << 1) | (t >> 1)) + (pf & 15u))));
                }
            }
            if (lane == at) my_result = exposed | (K << 16);  // lib.rs:156-159,215-217 (K: only read when counts are asked for)
            wave_lds_fence();
        }
        };
        if (n_chunk == 3u) atoms_of_group(std::integral_constant<uint32_t, 3u>{});
        else if (NS == 5 && n_chunk == 5u) atoms_of_group(std::integral_constant<uint32_t, 5u>{});
        else if (n_chunk == 4u) atoms_of_group(std::integral_constant<uint32_t, 4u>{});
        else if (n_chunk == 2u) atoms_of_group(std::integral_constant<uint32_t, 2u>{});
        else atoms_of_group(std::integral_constant<uint32_t, 1u>{});
        g0 = g1;
    }

    __builtin_amdgcn_s_setprio(kMxPrioEnd);
    // ---- results of the wave's atoms, one lane each ----
    if (lane < n_mine && my_result != kDeferred) {
        if (kPersist) asm volatile("" : "+s"(ka));
        const uint32_t pa_e = min(w_begin + lane, s_blk[w][6] - 1u);  // (= pa: computed again, a register less through the block)
        const uint32_t orig = (kPersist ? ka->sorted_orig : a.sorted_orig)[pa_e];
        uint32_t *const counts = kPersist ? ka->neighbor_counts : a.neighbor_counts;
        const float R = kHoist ? s_atom[w][lane].w : s_atom[w][lane].w + probe;  // lib.rs:101
        const float surface_area = (4.0f * 3.14159274101257324219f) * (R * R);  // 4.0 * PI * r2, lib.rs:220
        const float inv_n = 1.0f / (float)n_points;                             // lib.rs:221
        const float accessible = (float)(my_result & 0xFFFFu);
        (kPersist ? ka->atom_sasa : a.atom_sasa)[orig] = surface_area * accessible * inv_n;  // lib.rs:222
        if (counts) counts[orig] = my_result >> 16;
    }
    __builtin_amdgcn_s_setprio(0);
    wave_lds_fence();  // (the next block's atoms overwrite s_atom)
    if (!kPersist) break;
    }  // next block
}
