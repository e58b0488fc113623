// The argument rules of the neighbour-list and point-run entry points (neighbors.cpp), and the one description of their
// input.  Plain host C++: no HIP, no context, nothing is written but N and the Cols.  A rule returns the message of the
// first thing it finds wrong, or null when the arguments stand; the entry points turn a message into
// RSASA_ERR_INVALID_ARGUMENT.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace rsasa {

// The shape of structure_offsets[0 .. n_structures]: non-decreasing from 0 to N, fewer than 2^31 - 1 atoms.
inline const char *check_offsets(const uint32_t *so, size_t n_structures, size_t &N)
{
    N = 0;
    if (!so) return "NULL argument";
    if (n_structures >= 0x7FFFFFFFull) return "too many structures";
    for (size_t s = 0; s < n_structures; s++)
        if (so[s] > so[s + 1]) return "structure_offsets must be non-decreasing";
    if (n_structures && so[0] != 0) return "structure_offsets[0] must be 0";
    if (n_structures) N = so[n_structures];
    if (N >= 0x7FFFFFFFull) return "more than 2^31 - 1 atoms";
    return nullptr;
}

// How an entry point names its atoms: a single structure of n atoms, or n structures by the caller's structure_offsets.
struct Form {
    bool batch;
    const uint32_t *so;  // batch: structure_offsets[0 .. n]
    size_t n;
    static Form one(size_t n_atoms) { return {false, nullptr, n_atoms}; }
    static Form many(const uint32_t *so, size_t n_structures) { return {true, so, n_structures}; }
};

// The columns of a run in host memory: S structures, N atoms, structure s being atoms [so[s], so[s + 1]).  Empty (S = N
// = 0, no offsets) until fix() has passed.
struct Cols {
    const float *x, *y, *z, *r;
    const uint64_t *id;  // nullable
    const uint32_t *so = nullptr;
    size_t S = 0, N = 0;
    uint32_t one[2] = {0u, 0u};  // `so` of a single structure
    Cols(const float *x, const float *y, const float *z, const float *r, const uint64_t *id) : x(x), y(y), z(z), r(r), id(id) {}
    Cols(const Cols &) = delete;  // (so may point into the object)
    Cols &operator=(const Cols &) = delete;
    // Fixes N and the structures.  A single structure owns its offsets {0, n} and has no rule of its own; a batch points
    // at the caller's, under check_offsets: on its message the Cols stays empty.
    const char *fix(const Form &f)
    {
        if (!f.batch) {
            one[1] = (uint32_t)f.n;
            so = one; S = 1; N = f.n;
            return nullptr;
        }
        const char *msg = check_offsets(f.so, f.n, N);
        if (msg) N = 0;
        else { so = f.so; S = f.n; }
        return msg;
    }
};

// The columns of N atoms.  rest: whatever else the call cannot do without is there - the caller's own test of the arrays
// it needs always and of those that have an entry per atom (which may all be NULL when N is 0, as the columns may).
inline const char *check_columns(size_t N, const float *x, const float *y, const float *z, const float *r, bool rest)
{
    if (!rest || (N && (!x || !y || !z || !r))) return "NULL argument";
    if (N >= 0x7FFFFFFFull) return "more than 2^31 - 1 atoms";
    return nullptr;
}

// check_columns, and the size of the lattice.
inline const char *check_points(size_t N, const float *x, const float *y, const float *z, const float *r, bool rest,
                                size_t n_points)
{
    if (n_points == 0 || n_points >= 0x7FFFFFFFull) return "n_points must be in [1, 2^31 - 1)";
    return check_columns(N, x, y, z, r, rest);
}

// The link length of the surface components: finite and not negative (-0.0 is 0).
inline const char *check_link(float link)
{
    if (!(link >= 0.0f) || std::isinf(link)) return "link must be finite and not negative";
    return nullptr;
}

// The limit of the dot geodesics: +inf (no limit) or finite, and not negative (-0.0 is 0).
inline const char *check_geodesic_limit(float limit)
{
    if (!(limit >= 0.0f)) return "limit must be +inf or finite, and not negative";
    return nullptr;
}

// The dots of the dot links and geodesics: their scan and their 32-bit round counter take fewer than 2^31 - 1.
inline const char *check_dot_total(uint64_t n_dots)
{
    if (n_dots >= 0x7FFFFFFFull) return "2^31 - 1 or more accessible dots";
    return nullptr;
}

// The seed bytes of the dot geodesics against the D dots the call found: one byte per dot, NULL only where D is 0.
// why: room for the message that names both numbers (a caller who guessed reads D there).
inline const char *check_seed_bytes(const uint8_t *seeds, size_t n_seed_bytes, uint64_t n_dots, char (&why)[96])
{
    if (n_seed_bytes != n_dots) {
        std::snprintf(why, sizeof why, "n_seed_bytes is %llu but the structures have %llu accessible dots",
                      (unsigned long long)n_seed_bytes, (unsigned long long)n_dots);
        return why;
    }
    if (n_dots && !seeds) return "NULL argument";
    return nullptr;
}

// The spacing of the dot patches: +inf (one centre per component) or finite, and not negative (-0.0 is 0).
inline const char *check_patch_spacing(float spacing)
{
    if (!(spacing >= 0.0f)) return "spacing must be +inf or finite, and not negative";
    return nullptr;
}

// The most centres a structure of the dot patches gets: at least one.
inline const char *check_patch_max_centres(uint32_t max_centres)
{
    if (max_centres < 1u) return "max_centres must be at least 1";
    return nullptr;
}

// The room the centres of the dot patches can take: slots[s] (S + 1 entries, nullable) becomes the exclusive scan of
// min(max_centres, D_s) over the S structures, D_s being the dots of structure s - dot_offsets (N + 1 entries) at its
// first atom so[s] and behind its last; returns the total B.
inline uint64_t patch_centre_bound(const uint64_t *dot_offsets, const uint32_t *so, size_t S, uint32_t max_centres, uint64_t *slots)
{
    uint64_t B = 0;
    for (size_t s = 0; s < S; s++) {
        if (slots) slots[s] = B;
        const uint64_t D = dot_offsets[so[s + 1]] - dot_offsets[so[s]];
        B += D < max_centres ? D : (uint64_t)max_centres;
    }
    if (slots) slots[S] = B;
    return B;
}

// The caller's buffers of the dot patches against the D dots and the bound B the call found: all four are needed, with
// room for D dots and B centres.  The message stands for RSASA_ERR_BUFFER_TOO_SMALL.
inline const char *check_patch_room(const void *centre_offsets, const void *centres, const void *cover, const void *dist,
                                    size_t dots_capacity, uint64_t D, size_t centres_capacity, uint64_t B)
{
    if (!centre_offsets || !centres || !cover || !dist) return "out_centre_offsets, out_centres, out_cover or out_dist is NULL";
    if (dots_capacity < D) return "out_dist holds fewer dots than out_dot_offsets[n]";
    if (centres_capacity < B) return "out_centres and out_cover hold fewer centres than *out_centre_bound";
    return nullptr;
}

// The cutoff of the half-sphere exposure: finite and not negative (-0.0 is 0).
inline const char *check_cutoff(float cutoff)
{
    if (!(cutoff >= 0.0f) || std::isinf(cutoff)) return "cutoff must be finite and not negative";
    return nullptr;
}

// The cutoff of the k nearest atoms: check_cutoff with +inf allowed (no cutoff).
inline const char *check_nearest_cutoff(float cutoff)
{
    if (!(cutoff >= 0.0f)) return "cutoff must be +inf or finite, and not negative";
    return nullptr;
}

// The k of the k nearest atoms: 1 .. RSASA_NEAREST_MAX_K, the most keys a compaction of k_nearest's staging keeps.
constexpr uint32_t kNearestMaxK = 256;
inline const char *check_nearest_k(uint32_t k)
{
    if (k < 1u || k > kNearestMaxK) return "k must be in [1, 256]";
    return nullptr;
}

// The bins and classes of the radial counts: 1 .. RSASA_RADIAL_MAX_BINS edges, each finite and not negative (-0.0 is
// 0), non-decreasing (equal edges are allowed), and 1 .. RSASA_RADIAL_MAX_CLASSES classes - a row of k_radial_counts'
// histogram is n_classes * n_bins cells of LDS.
constexpr uint32_t kRadialMaxClasses = 16, kRadialMaxBins = 32;
// The edges themselves, n_bins of them (the caller has bounded n_bins): what check_radial and check_crowding share.
inline const char *check_edges(const float *edges, uint32_t n_bins)
{
    if (!edges) return "NULL argument";
    for (uint32_t k = 0; k < n_bins; k++) {
        if (!(edges[k] >= 0.0f) || std::isinf(edges[k])) return "edges must be finite and not negative";
        if (k && edges[k] < edges[k - 1u]) return "edges must be non-decreasing";
    }
    return nullptr;
}
inline const char *check_radial(const float *edges, uint32_t n_bins, uint32_t n_classes)
{
    if (n_classes < 1u || n_classes > kRadialMaxClasses) return "n_classes must be in [1, 16]";
    if (n_bins < 1u || n_bins > kRadialMaxBins) return "n_bins must be in [1, 32]";
    return check_edges(edges, n_bins);
}

// The bins of the dot crowding: 1 .. RSASA_CROWD_MAX_BINS edges under the rules of check_radial's - a dot's counters
// are registers of k_dot_crowding.
constexpr uint32_t kCrowdMaxBins = 8;
inline const char *check_crowding(const float *edges, uint32_t n_bins)
{
    if (n_bins < 1u || n_bins > kCrowdMaxBins) return "n_bins must be in [1, 8]";
    return check_edges(edges, n_bins);
}

// The channels of the dot fields: 1 .. RSASA_FIELD_MAX_CHANNELS kinds, each one of RSASA_FIELD_STEP .. _INV_1PD - a
// dot's accumulators are registers of k_dot_fields - and a cutoff that is finite and not negative (-0.0 is 0).  The
// weights' values have no rule.
constexpr uint32_t kFieldMaxChannels = 4, kFieldKinds = 4;
inline const char *check_fields(const uint8_t *kinds, uint32_t n_channels, float cutoff)
{
    if (n_channels < 1u || n_channels > kFieldMaxChannels) return "n_channels must be in [1, 4]";
    if (!kinds) return "NULL argument";
    for (uint32_t c = 0; c < n_channels; c++)
        if (kinds[c] >= kFieldKinds) return "kinds must be RSASA_FIELD_STEP, _INV_D, _INV_D2 or _INV_1PD";
    if (!(cutoff >= 0.0f) || std::isinf(cutoff)) return "cutoff must be finite and not negative";
    return nullptr;
}

// The reach of the dot curvature: finite and not negative (-0.0 is 0; 0 is legal and gives zero rows).
inline const char *check_curvature(float reach)
{
    if (!(reach >= 0.0f) || std::isinf(reach)) return "reach must be finite and not negative";
    return nullptr;
}

// The fan of the dot enclosure: 1 .. RSASA_ENCLOSE_MAX_DIRS directions - a dot's word of k_dot_enclosure has a bit for
// each - and a reach that is finite and not negative (-0.0 is 0).
constexpr uint32_t kEncloseMaxDirs = 32;
inline const char *check_enclosure(float reach, uint32_t n_dirs)
{
    if (n_dirs < 1u || n_dirs > kEncloseMaxDirs) return "n_dirs must be in [1, 32]";
    if (!(reach >= 0.0f) || std::isinf(reach)) return "reach must be finite and not negative";
    return nullptr;
}

// The class bytes of N atoms (nullable: every atom is class 0): every one below n_classes, on any atom.
inline const char *check_classes(const uint8_t *classes, size_t N, uint32_t n_classes)
{
    if (!classes) return nullptr;
    for (size_t i = 0; i < N; i++)
        if (classes[i] >= n_classes) return "classes must lie below n_classes";
    return nullptr;
}

}  // namespace rsasa
