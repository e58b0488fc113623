// The k and cutoff rules of the k-nearest-atoms entry points (check_nearest_k, check_nearest_cutoff,
// rustsasa_amd/csrc/entry_checks.h) against the verdicts the header documents.  Stand-alone: host compiler, no HIP, built
// with -fsanitize=address,undefined by tests/test_nearest_cpu.py.  Prints "nearest checks ok" and returns 0 when every
// verdict is the listed one.
#include "entry_checks.h"

#include <cfloat>
#include <cstdio>
#include <cstring>
#include <limits>

using namespace rsasa;

static int failures = 0;

static void expect(const char *rule, const char *what, const char *msg, bool ok, const char *want)
{
    const bool good = ok ? msg == nullptr : msg != nullptr && std::strcmp(msg, want) == 0;
    if (!good) {
        std::printf("FAIL %s %s: expected %s, got %s\n", rule, what, ok ? "OK" : want, msg ? msg : "OK");
        failures++;
    }
}

static void expect_k(const char *what, uint32_t k, bool ok) { expect("k", what, check_nearest_k(k), ok, "k must be in [1, 256]"); }

static void expect_cutoff(const char *what, float cutoff, bool ok)
{
    expect("cutoff", what, check_nearest_cutoff(cutoff), ok, "cutoff must be +inf or finite, and not negative");
}

int main()
{
    static_assert(kNearestMaxK == 256, "RSASA_NEAREST_MAX_K");
    expect_k("0", 0u, false);
    expect_k("1", 1u, true);
    expect_k("16", 16u, true);
    expect_k("256", 256u, true);
    expect_k("257", 257u, false);
    expect_k("2^32 - 1", 0xFFFFFFFFu, false);

    expect_cutoff("+0", 0.0f, true);
    expect_cutoff("-0.0", -0.0f, true);
    expect_cutoff("+inf", std::numeric_limits<float>::infinity(), true);
    expect_cutoff("NaN", std::numeric_limits<float>::quiet_NaN(), false);
    expect_cutoff("-1", -1.0f, false);
    expect_cutoff("-inf", -std::numeric_limits<float>::infinity(), false);
    expect_cutoff("-FLT_MIN", -FLT_MIN, false);
    expect_cutoff("the smallest subnormal", std::numeric_limits<float>::denorm_min(), true);
    expect_cutoff("8", 8.0f, true);
    expect_cutoff("FLT_MAX", FLT_MAX, true);
    // check_cutoff itself still refuses +inf: the two rules differ there and nowhere else
    if (check_cutoff(std::numeric_limits<float>::infinity()) == nullptr || check_cutoff(FLT_MAX) != nullptr) {
        std::printf("FAIL check_cutoff changed\n");
        failures++;
    }

    if (failures) return 1;
    std::printf("nearest checks ok\n");
    return 0;
}
