// The argument and sizing rules of the dot-patch entry points (check_patch_spacing, check_patch_max_centres,
// patch_centre_bound, check_patch_room, rustsasa_amd/csrc/entry_checks.h) against the verdicts the header documents,
// with check_geodesic_limit beside the spacing on the same values: a spacing is a length that may be +inf, as a limit
// may.  Stand-alone: host compiler, no HIP, built with -fsanitize=address,undefined by tests/test_patches_cpu.py.
// Prints "patch checks ok" and returns 0 when every verdict is the listed one.
#include "entry_checks.h"

#include <cfloat>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace rsasa;

static int failures = 0;

static void expect(const char *what, const char *msg, const char *want)
{
    const bool good = want ? msg != nullptr && std::strcmp(msg, want) == 0 : msg == nullptr;
    if (!good) {
        std::printf("FAIL %s: expected %s, got %s\n", what, want ? want : "OK", msg ? msg : "OK");
        failures++;
    }
}

static void expect_eq(const char *what, uint64_t got, uint64_t want)
{
    if (got != want) {
        std::printf("FAIL %s: expected %llu, got %llu\n", what, (unsigned long long)want, (unsigned long long)got);
        failures++;
    }
}

// A spacing; check_geodesic_limit agrees on whether the length stands.
static void spacing(const char *what, float s, const char *want)
{
    expect(what, check_patch_spacing(s), want);
    if ((check_geodesic_limit(s) == nullptr) != (want == nullptr)) {
        std::printf("FAIL %s: check_geodesic_limit disagrees\n", what);
        failures++;
    }
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const char *bad = "spacing must be +inf or finite, and not negative";

    spacing("NaN", nan, bad);
    spacing("-NaN", -nan, bad);
    spacing("-inf", -inf, bad);
    spacing("-1", -1.0f, bad);
    spacing("-FLT_MIN", -FLT_MIN, bad);
    spacing("the smallest negative subnormal", -std::numeric_limits<float>::denorm_min(), bad);
    spacing("-0.0", -0.0f, nullptr);
    spacing("0", 0.0f, nullptr);
    spacing("the smallest subnormal", std::numeric_limits<float>::denorm_min(), nullptr);
    spacing("6", 6.0f, nullptr);
    spacing("FLT_MAX", FLT_MAX, nullptr);
    spacing("+inf", inf, nullptr);

    expect("no centre", check_patch_max_centres(0u), "max_centres must be at least 1");
    expect("one centre", check_patch_max_centres(1u), nullptr);
    expect("no bound", check_patch_max_centres(0xFFFFFFFFu), nullptr);

    // the bound: five structures of 3, 0 (no atom), 0 (an atom without dots), 10 and 1 dots
    const uint64_t dot_offsets[] = {0, 2, 3, 3, 3, 8, 13, 14};   // seven atoms
    const uint32_t so[] = {0, 2, 2, 3, 6, 7};
    std::vector<uint64_t> slots(6, 77);
    expect_eq("max_centres 1", patch_centre_bound(dot_offsets, so, 5, 1u, slots.data()), 3);
    expect_eq("slots[1] at 1", slots[1], 1);
    expect_eq("slots[3] at 1", slots[3], 1);
    expect_eq("slots[5] at 1", slots[5], 3);
    expect_eq("max_centres 4", patch_centre_bound(dot_offsets, so, 5, 4u, slots.data()), 3 + 0 + 0 + 4 + 1);
    expect_eq("slots[4] at 4", slots[4], 7);
    expect_eq("max_centres 10", patch_centre_bound(dot_offsets, so, 5, 10u, slots.data()), 14);
    expect_eq("no bound equals the dots", patch_centre_bound(dot_offsets, so, 5, 0xFFFFFFFFu, nullptr), 14);
    expect_eq("no structure", patch_centre_bound(dot_offsets, so, 0, 7u, slots.data()), 0);
    expect_eq("slots[0] of none", slots[0], 0);
    // dots beyond 32 bits do not wrap the bound
    const uint64_t big[] = {0, 0x200000000ull};
    const uint32_t one[] = {0, 1};
    expect_eq("a structure of 2^33 dots", patch_centre_bound(big, one, 1, 0xFFFFFFFFu, nullptr), 0xFFFFFFFFull);

    // the room: all four buffers, D dots, B centres
    int x;
    const char *null = "out_centre_offsets, out_centres, out_cover or out_dist is NULL";
    const char *dots = "out_dist holds fewer dots than out_dot_offsets[n]";
    const char *centres = "out_centres and out_cover hold fewer centres than *out_centre_bound";
    expect("room", check_patch_room(&x, &x, &x, &x, 14, 14, 8, 8), nullptr);
    expect("more room", check_patch_room(&x, &x, &x, &x, 15, 14, 14, 8), nullptr);
    expect("nothing to hold", check_patch_room(&x, &x, &x, &x, 0, 0, 0, 0), nullptr);
    expect("no offsets", check_patch_room(nullptr, &x, &x, &x, 14, 14, 8, 8), null);
    expect("no centres", check_patch_room(&x, nullptr, &x, &x, 14, 14, 8, 8), null);
    expect("no cover", check_patch_room(&x, &x, nullptr, &x, 14, 14, 8, 8), null);
    expect("no dist", check_patch_room(&x, &x, &x, nullptr, 14, 14, 8, 8), null);
    expect("NULL even where nothing is to hold", check_patch_room(&x, &x, &x, nullptr, 0, 0, 0, 0), null);
    expect("one dot short", check_patch_room(&x, &x, &x, &x, 13, 14, 8, 8), dots);
    expect("one centre short", check_patch_room(&x, &x, &x, &x, 14, 14, 7, 8), centres);
    expect("both short: the dots are named", check_patch_room(&x, &x, &x, &x, 0, 14, 0, 8), dots);
    expect("a capacity of D suffices for the centres", check_patch_room(&x, &x, &x, &x, 14, 14, 14, 14), nullptr);

    if (failures) return 1;
    std::printf("patch checks ok\n");
    return 0;
}
