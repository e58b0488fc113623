// The reach rule of the dot-curvature entry points (check_curvature, rustsasa_amd/csrc/entry_checks.h) against the verdicts
// the header documents.  Stand-alone: host compiler, no HIP, built with -fsanitize=address,undefined by
// tests/test_curvature_cpu.py.  Prints "curvature checks ok" and returns 0 when every verdict is the listed one.
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

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const char *reach = "reach must be finite and not negative";

    expect("NaN", check_curvature(nan), reach);
    expect("-NaN", check_curvature(-nan), reach);
    expect("negative", check_curvature(-1.0f), reach);
    expect("-FLT_MIN", check_curvature(-FLT_MIN), reach);
    expect("minus the smallest subnormal", check_curvature(-std::numeric_limits<float>::denorm_min()), reach);
    expect("+inf", check_curvature(inf), reach);
    expect("-inf", check_curvature(-inf), reach);
    expect("-0.0", check_curvature(-0.0f), nullptr);
    expect("0 (legal: zero rows)", check_curvature(0.0f), nullptr);
    expect("the default", check_curvature(3.0f), nullptr);
    expect("FLT_MAX (its square overflows)", check_curvature(FLT_MAX), nullptr);
    expect("1e-30 (its square underflows)", check_curvature(1e-30f), nullptr);
    expect("the smallest subnormal", check_curvature(std::numeric_limits<float>::denorm_min()), nullptr);
    // the rule sits beside those it resembles and changes none of them
    expect("check_link", check_link(nan), "link must be finite and not negative");
    expect("check_enclosure", check_enclosure(nan, 4u), reach);
    expect("check_dot_total", check_dot_total(0x7FFFFFFFull), "2^31 - 1 or more accessible dots");

    if (failures) return 1;
    std::printf("curvature checks ok\n");
    return 0;
}
