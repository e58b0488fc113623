// The bin, class and class-byte rules of the radial-count entry points (check_radial, check_classes,
// rustsasa_amd/csrc/entry_checks.h) against the verdicts the header documents.  Stand-alone: host compiler, no HIP, built
// with -fsanitize=address,undefined by tests/test_radial_cpu.py; the arrays live on the heap at their exact sizes, so a
// rule that read past n_bins edges or N class bytes would be reported.  Prints "radial checks ok" and returns 0 when every
// verdict is the listed one.
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

static const char *radial(const std::vector<float> &edges, uint32_t n_classes)
{
    std::vector<float> exact(edges);  // (a heap block of exactly n_bins floats)
    exact.shrink_to_fit();
    return check_radial(exact.data(), (uint32_t)exact.size(), n_classes);
}

int main()
{
    static_assert(kRadialMaxClasses == 16 && kRadialMaxBins == 32, "RSASA_RADIAL_MAX_CLASSES, RSASA_RADIAL_MAX_BINS");
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const char *bins = "n_bins must be in [1, 32]", *classes = "n_classes must be in [1, 16]";
    const char *finite = "edges must be finite and not negative", *order = "edges must be non-decreasing";
    const float one = 1.0f;

    // the number of bins: 0 and 33 are refused, 1 and 32 stand
    expect("0 bins", check_radial(&one, 0u, 1u), bins);
    expect("1 bin", radial({6.0f}, 1u), nullptr);
    expect("32 bins", radial(std::vector<float>(32, 5.0f), 1u), nullptr);
    expect("33 bins", radial(std::vector<float>(33, 5.0f), 1u), bins);
    // the number of classes: 0 and 17 are refused, 1 and 16 stand
    expect("0 classes", radial({6.0f}, 0u), classes);
    expect("16 classes", radial({6.0f}, 16u), nullptr);
    expect("17 classes", radial({6.0f}, 17u), classes);
    expect("2^32 - 1 classes", radial({6.0f}, 0xFFFFFFFFu), classes);
    // the edges' values
    expect("NaN edge", radial({6.0f, nan, 8.0f}, 4u), finite);
    expect("NaN last edge", radial({6.0f, nan}, 4u), finite);
    expect("negative edge", radial({-1.0f, 8.0f}, 4u), finite);
    expect("-FLT_MIN", radial({-FLT_MIN}, 4u), finite);
    expect("+inf edge", radial({6.0f, inf}, 4u), finite);
    expect("-inf edge", radial({-inf, 6.0f}, 4u), finite);
    expect("-0.0", radial({-0.0f, 6.0f}, 4u), nullptr);
    expect("-0.0 after +0", radial({0.0f, -0.0f, 0.0f}, 4u), nullptr);
    expect("FLT_MAX (its square overflows)", radial({6.0f, FLT_MAX}, 4u), nullptr);
    expect("1e-30 (its square underflows)", radial({1e-30f, 6.0f}, 4u), nullptr);
    expect("the smallest subnormal", radial({std::numeric_limits<float>::denorm_min()}, 1u), nullptr);
    // their order
    expect("a decreasing pair", radial({6.0f, 8.0f, 7.5f, 12.0f}, 4u), order);
    expect("a decreasing last pair", radial({6.0f, 5.0f}, 4u), order);
    expect("equal edges", radial({6.0f, 6.0f, 8.0f, 8.0f}, 4u), nullptr);
    expect("(6, 8, 10, 12)", radial({6.0f, 8.0f, 10.0f, 12.0f}, 4u), nullptr);
    // NULL edges
    expect("NULL edges", check_radial(nullptr, 4u, 4u), "NULL argument");
    expect("NULL edges, 0 bins", check_radial(nullptr, 0u, 4u), bins);

    // the class bytes: every one below n_classes, on any atom; NULL is class 0 for everybody
    const char *below = "classes must lie below n_classes";
    std::vector<uint8_t> cl{0, 1, 2, 3, 3, 0};
    cl.shrink_to_fit();
    expect("classes below 4", check_classes(cl.data(), cl.size(), 4u), nullptr);
    expect("a class byte equal to n_classes", check_classes(cl.data(), cl.size(), 3u), below);
    cl.back() = 4;
    expect("the last byte equal to n_classes", check_classes(cl.data(), cl.size(), 4u), below);
    expect("without the last atom", check_classes(cl.data(), cl.size() - 1, 4u), nullptr);
    cl.back() = 255;
    expect("255 with 16 classes", check_classes(cl.data(), cl.size(), 16u), below);
    expect("NULL classes", check_classes(nullptr, 6, 1u), nullptr);
    expect("no atoms", check_classes(cl.data(), 0, 1u), nullptr);

    if (failures) return 1;
    std::printf("radial checks ok\n");
    return 0;
}
