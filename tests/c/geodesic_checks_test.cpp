// The argument rules of the dot-link and dot-geodesic entry points (check_geodesic_limit, check_dot_total,
// check_seed_bytes, rustsasa_amd/csrc/entry_checks.h) against the verdicts the header documents, with check_link and
// check_nearest_cutoff beside them on the same values: the link is the components' and a limit is a length that may be
// +inf, as the cutoff of the k nearest atoms may.  Stand-alone: host compiler, no HIP, built with
// -fsanitize=address,undefined by tests/test_geodesics_cpu.py.  Prints "geodesic checks ok" and returns 0 when every
// verdict is the listed one.
#include "entry_checks.h"

#include <cfloat>
#include <cstdio>
#include <cstring>
#include <limits>

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

// A limit; check_nearest_cutoff agrees on whether the length stands, and check_link too unless it is +inf.
static void limit(const char *what, float L, const char *want)
{
    expect(what, check_geodesic_limit(L), want);
    if ((check_nearest_cutoff(L) == nullptr) != (want == nullptr)) {
        std::printf("FAIL %s: check_nearest_cutoff disagrees\n", what);
        failures++;
    }
    if (!std::isinf(L) && (check_link(L) == nullptr) != (want == nullptr)) {
        std::printf("FAIL %s: check_link disagrees\n", what);
        failures++;
    }
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const char *bad = "limit must be +inf or finite, and not negative";

    limit("NaN", nan, bad);
    limit("-NaN", -nan, bad);
    limit("-inf", -inf, bad);
    limit("-1", -1.0f, bad);
    limit("-FLT_MIN", -FLT_MIN, bad);
    limit("the smallest negative subnormal", -std::numeric_limits<float>::denorm_min(), bad);
    limit("-0.0", -0.0f, nullptr);
    limit("0", 0.0f, nullptr);
    limit("the smallest subnormal", std::numeric_limits<float>::denorm_min(), nullptr);
    limit("12", 12.0f, nullptr);
    limit("FLT_MAX", FLT_MAX, nullptr);
    limit("+inf", inf, nullptr);
    expect("an infinite link", check_link(inf), "link must be finite and not negative");

    // the dots: 2^31 - 2 stand, 2^31 - 1 and more do not
    const char *many = "2^31 - 1 or more accessible dots";
    expect("no dot", check_dot_total(0), nullptr);
    expect("2^31 - 2 dots", check_dot_total(0x7FFFFFFEull), nullptr);
    expect("2^31 - 1 dots", check_dot_total(0x7FFFFFFFull), many);
    expect("2^32 - 1 dots", check_dot_total(0xFFFFFFFFull), many);
    expect("2^63 dots", check_dot_total(1ull << 63), many);

    // the seed bytes: one per dot; the message names both numbers; NULL only where there is no dot
    char why[96];
    const uint8_t seeds[4] = {0, 1, 0, 255};
    expect("4 bytes for 4 dots", check_seed_bytes(seeds, 4, 4, why), nullptr);
    expect("no byte for no dot", check_seed_bytes(nullptr, 0, 0, why), nullptr);
    expect("an array for no dot", check_seed_bytes(seeds, 0, 0, why), nullptr);
    expect("NULL for 4 dots", check_seed_bytes(nullptr, 4, 4, why), "NULL argument");
    expect("3 bytes for 4 dots", check_seed_bytes(seeds, 3, 4, why), "n_seed_bytes is 3 but the structures have 4 accessible dots");
    expect("5 bytes for 4 dots", check_seed_bytes(seeds, 5, 4, why), "n_seed_bytes is 5 but the structures have 4 accessible dots");
    expect("NULL and the wrong number", check_seed_bytes(nullptr, 0, 4, why), "n_seed_bytes is 0 but the structures have 4 accessible dots");
    expect("the largest numbers fit the message",
           check_seed_bytes(seeds, (size_t)0xFFFFFFFFFFFFFFFFull, 0x7FFFFFFEull, why),
           "n_seed_bytes is 18446744073709551615 but the structures have 2147483646 accessible dots");
    if (std::strlen(why) >= sizeof why) {
        std::printf("FAIL the message overran its room\n");
        failures++;
    }

    if (failures) return 1;
    std::printf("geodesic checks ok\n");
    return 0;
}
