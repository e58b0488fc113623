// The argument rule of the dot-enclosure entry points (check_enclosure, rustsasa_amd/csrc/entry_checks.h) against the
// verdicts the header documents, with check_cutoff and check_link beside it on the same values: a reach is a length like
// theirs.  Stand-alone: host compiler, no HIP, built with -fsanitize=address,undefined by tests/test_enclosure_cpu.py.
// Prints "enclosure checks ok" and returns 0 when every verdict is the listed one.
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

// A reach under every legal number of directions; check_cutoff and check_link agree on whether the length stands.
static void reach(const char *what, float L, const char *want)
{
    for (uint32_t n = 1; n <= kEncloseMaxDirs; n++) expect(what, check_enclosure(L, n), want);
    if ((check_cutoff(L) == nullptr) != (want == nullptr) || (check_link(L) == nullptr) != (want == nullptr)) {
        std::printf("FAIL %s: check_cutoff / check_link disagree\n", what);
        failures++;
    }
}

int main()
{
    static_assert(kEncloseMaxDirs == 32, "RSASA_ENCLOSE_MAX_DIRS");
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const char *dirs = "n_dirs must be in [1, 32]", *finite = "reach must be finite and not negative";

    // the number of directions: 0 and 33 are refused, 1 and 32 stand; it is looked at first
    expect("0 directions", check_enclosure(10.0f, 0u), dirs);
    expect("1 direction", check_enclosure(10.0f, 1u), nullptr);
    expect("32 directions", check_enclosure(10.0f, 32u), nullptr);
    expect("33 directions", check_enclosure(10.0f, 33u), dirs);
    expect("2^32 - 1 directions", check_enclosure(10.0f, 0xFFFFFFFFu), dirs);
    expect("0 directions and a NaN reach", check_enclosure(nan, 0u), dirs);
    // the reach
    reach("NaN", nan, finite);
    reach("-NaN", -nan, finite);
    reach("+inf", inf, finite);
    reach("-inf", -inf, finite);
    reach("-1", -1.0f, finite);
    reach("-FLT_MIN", -FLT_MIN, finite);
    reach("the smallest negative subnormal", -std::numeric_limits<float>::denorm_min(), finite);
    reach("-0.0", -0.0f, nullptr);
    reach("0", 0.0f, nullptr);
    reach("the smallest subnormal", std::numeric_limits<float>::denorm_min(), nullptr);
    reach("1e-30 (its square underflows)", 1e-30f, nullptr);
    reach("10", 10.0f, nullptr);
    reach("FLT_MAX (its square overflows)", FLT_MAX, nullptr);

    if (failures) return 1;
    std::printf("enclosure checks ok\n");
    return 0;
}
