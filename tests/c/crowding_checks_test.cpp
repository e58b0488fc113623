// The bin rules of the dot-crowding entry points (check_crowding, rustsasa_amd/csrc/entry_checks.h) against the verdicts
// the header documents, and check_radial beside it on the same edges: the two share the edge rules.  Stand-alone: host
// compiler, no HIP, built with -fsanitize=address,undefined by tests/test_crowding_cpu.py; the arrays live on the heap at
// their exact sizes, so a rule that read past n_bins edges would be reported.  Prints "crowding checks ok" and returns 0
// when every verdict is the listed one.
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

static const char *crowding(const std::vector<float> &edges)
{
    std::vector<float> exact(edges);  // (a heap block of exactly n_bins floats)
    exact.shrink_to_fit();
    return check_crowding(exact.data(), (uint32_t)exact.size());
}

// The verdict on the edges themselves is the one check_radial gives (one class).
static void both(const char *what, const std::vector<float> &edges, const char *want)
{
    std::vector<float> exact(edges);
    exact.shrink_to_fit();
    expect(what, check_crowding(exact.data(), (uint32_t)exact.size()), want);
    expect(what, check_radial(exact.data(), (uint32_t)exact.size(), 1u), want);
}

int main()
{
    static_assert(kCrowdMaxBins == 8, "RSASA_CROWD_MAX_BINS");
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const char *bins = "n_bins must be in [1, 8]";
    const char *finite = "edges must be finite and not negative", *order = "edges must be non-decreasing";
    const float one = 1.0f;

    // the number of bins: 0 and 9 are refused, 1 and 8 stand
    expect("0 bins", check_crowding(&one, 0u), bins);
    expect("1 bin", crowding({6.0f}), nullptr);
    expect("8 bins", crowding(std::vector<float>(8, 5.0f)), nullptr);
    expect("9 bins", crowding(std::vector<float>(9, 5.0f)), bins);
    expect("2^32 - 1 bins", check_crowding(&one, 0xFFFFFFFFu), bins);
    // the edges' values
    both("NaN edge", {6.0f, nan, 8.0f}, finite);
    both("NaN last edge", {6.0f, nan}, finite);
    both("negative edge", {-1.0f, 8.0f}, finite);
    both("-FLT_MIN", {-FLT_MIN}, finite);
    both("+inf edge", {6.0f, inf}, finite);
    both("-inf edge", {-inf, 6.0f}, finite);
    both("-0.0", {-0.0f, 6.0f}, nullptr);
    both("-0.0 after +0", {0.0f, -0.0f, 0.0f}, nullptr);
    both("FLT_MAX (its square overflows)", {6.0f, FLT_MAX}, nullptr);
    both("1e-30 (its square underflows)", {1e-30f, 6.0f}, nullptr);
    both("the smallest subnormal", {std::numeric_limits<float>::denorm_min()}, nullptr);
    // their order
    both("a decreasing pair", {6.0f, 8.0f, 7.5f, 12.0f}, order);
    both("a decreasing last pair", {6.0f, 5.0f}, order);
    both("equal edges", {6.0f, 6.0f, 8.0f, 8.0f}, nullptr);
    both("(6, 8, 10)", {6.0f, 8.0f, 10.0f}, nullptr);
    // NULL edges
    expect("NULL edges", check_crowding(nullptr, 4u), "NULL argument");
    expect("NULL edges, 0 bins", check_crowding(nullptr, 0u), bins);

    if (failures) return 1;
    std::printf("crowding checks ok\n");
    return 0;
}
