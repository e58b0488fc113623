// The channel and cutoff rules of the dot-fields entry points (check_fields, rustsasa_amd/csrc/entry_checks.h) against the
// verdicts the header documents.  Stand-alone: host compiler, no HIP, built with -fsanitize=address,undefined by
// tests/test_fields_cpu.py; the kinds live on the heap at their exact size, so a rule that read past n_channels kinds
// would be reported.  Prints "fields checks ok" and returns 0 when every verdict is the listed one.
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

static const char *fields(const std::vector<uint8_t> &kinds, float cutoff)
{
    std::vector<uint8_t> exact(kinds);  // (a heap block of exactly n_channels bytes)
    exact.shrink_to_fit();
    return check_fields(exact.data(), (uint32_t)exact.size(), cutoff);
}

int main()
{
    static_assert(kFieldMaxChannels == 4, "RSASA_FIELD_MAX_CHANNELS");
    static_assert(kFieldKinds == 4, "RSASA_FIELD_STEP .. RSASA_FIELD_INV_1PD");
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const char *channels = "n_channels must be in [1, 4]";
    const char *kind = "kinds must be RSASA_FIELD_STEP, _INV_D, _INV_D2 or _INV_1PD";
    const char *cutoff = "cutoff must be finite and not negative";
    const uint8_t one = 1;

    // the number of channels: 0 and 5 are refused (before the kinds are read), 1 and 4 stand
    expect("0 channels", check_fields(&one, 0u, 10.0f), channels);
    expect("1 channel", fields({1}, 10.0f), nullptr);
    expect("4 channels", fields({0, 1, 2, 3}, 10.0f), nullptr);
    expect("5 channels", check_fields(&one, 5u, 10.0f), channels);
    expect("2^32 - 1 channels", check_fields(&one, 0xFFFFFFFFu, 10.0f), channels);
    // the kinds
    for (uint8_t k = 0; k < 4; k++) expect("every kind alone", fields({k}, 10.0f), nullptr);
    expect("kinds repeated", fields({2, 2, 2, 2}, 10.0f), nullptr);
    expect("kind 4", fields({4}, 10.0f), kind);
    expect("kind 4 last", fields({0, 1, 2, 4}, 10.0f), kind);
    expect("kind 255", fields({0, 255}, 10.0f), kind);
    expect("NULL kinds", check_fields(nullptr, 2u, 10.0f), "NULL argument");
    expect("NULL kinds, 0 channels", check_fields(nullptr, 0u, 10.0f), channels);
    // the cutoff
    expect("NaN cutoff", fields({1}, nan), cutoff);
    expect("negative cutoff", fields({1}, -1.0f), cutoff);
    expect("-FLT_MIN", fields({1}, -FLT_MIN), cutoff);
    expect("+inf cutoff", fields({1}, inf), cutoff);
    expect("-inf cutoff", fields({1}, -inf), cutoff);
    expect("-0.0", fields({1}, -0.0f), nullptr);
    expect("0", fields({1}, 0.0f), nullptr);
    expect("FLT_MAX (its square overflows)", fields({1}, FLT_MAX), nullptr);
    expect("1e-30 (its square underflows)", fields({1}, 1e-30f), nullptr);
    expect("the smallest subnormal", fields({1}, std::numeric_limits<float>::denorm_min()), nullptr);
    // the order of the verdicts: channels, kinds, cutoff
    expect("a bad kind and a bad cutoff", fields({9}, nan), kind);
    expect("no channel and a bad cutoff", check_fields(&one, 0u, nan), channels);

    if (failures) return 1;
    std::printf("fields checks ok\n");
    return 0;
}
