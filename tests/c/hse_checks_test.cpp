// The cutoff rule of the half-sphere exposure entry points (check_cutoff, rustsasa_amd/csrc/entry_checks.h) against the
// verdicts the header documents.  Stand-alone: host compiler, no HIP, built with -fsanitize=address,undefined by
// tests/test_hse_cpu.py.  Prints "hse checks ok" and returns 0 when every verdict is the listed one.
#include "entry_checks.h"

#include <cfloat>
#include <cstdio>
#include <cstring>
#include <limits>

using namespace rsasa;

static int failures = 0;

static void expect(const char *what, float cutoff, bool ok)
{
    const char *want = "cutoff must be finite and not negative";
    const char *msg = check_cutoff(cutoff);
    const bool good = ok ? msg == nullptr : msg != nullptr && std::strcmp(msg, want) == 0;
    if (!good) {
        std::printf("FAIL cutoff %s: expected %s, got %s\n", what, ok ? "OK" : want, msg ? msg : "OK");
        failures++;
    }
}

int main()
{
    expect("NaN", std::numeric_limits<float>::quiet_NaN(), false);
    expect("+inf", std::numeric_limits<float>::infinity(), false);
    expect("-inf", -std::numeric_limits<float>::infinity(), false);
    expect("-1", -1.0f, false);
    expect("-FLT_MIN", -FLT_MIN, false);
    expect("-0.0", -0.0f, true);
    expect("0", 0.0f, true);
    expect("the smallest subnormal", std::numeric_limits<float>::denorm_min(), true);
    expect("13", 13.0f, true);
    expect("FLT_MAX", FLT_MAX, true);

    if (failures) return 1;
    std::printf("hse checks ok\n");
    return 0;
}
