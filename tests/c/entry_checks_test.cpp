// The argument rules of the neighbour-list and point-run entry points (rustsasa_amd/csrc/entry_checks.h) against the
// verdicts the entry points have always given.  Stand-alone: host compiler, no HIP, built with
// -fsanitize=address,undefined by tests/test_entry_checks_cpu.py, so a rule that reads an offset it should not have read
// ends the program.  Prints "entry checks ok" and returns 0 when every verdict is the listed one.
#include "entry_checks.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace rsasa;

static int failures = 0;

static void expect(const char *what, const char *msg, bool ok, const char *want_msg = nullptr)
{
    const bool good = ok ? msg == nullptr : msg != nullptr && (!want_msg || std::strcmp(msg, want_msg) == 0);
    if (!good) {
        std::printf("FAIL %s: %s, got %s\n", what, ok ? "expected OK" : want_msg ? want_msg : "expected a refusal", msg ? msg : "OK");
        failures++;
    }
}

static void offsets(const char *what, std::vector<uint32_t> so, size_t n_structures, bool ok, size_t want_N = 0,
                    const char *want_msg = nullptr)
{
    // (a heap copy of exactly the entries given: one read past it is the sanitizer's)
    size_t N = 12345;
    const char *msg = check_offsets(so.data(), n_structures, N);
    expect(what, msg, ok, want_msg);
    if (ok && N != want_N) {
        std::printf("FAIL %s: N = %zu, expected %zu\n", what, N, want_N);
        failures++;
    }
}

int main()
{
    // ---- structure_offsets
    offsets("no structure, {0}", {0}, 0, true, 0);
    offsets("{0, 0, 0}", {0, 0, 0}, 2, true, 0);
    offsets("{1, 2}", {1, 2}, 1, false, 0, "structure_offsets[0] must be 0");
    offsets("{0, 5, 4}", {0, 5, 4}, 2, false, 0, "structure_offsets must be non-decreasing");
    offsets("{0, 2^31 - 2}", {0, 0x7FFFFFFEu}, 1, true, 0x7FFFFFFEu);
    offsets("{0, 2^31 - 1}", {0, 0x7FFFFFFFu}, 1, false, 0, "more than 2^31 - 1 atoms");
    offsets("2^31 - 1 structures, one entry", {0}, 0x7FFFFFFFu, false, 0, "too many structures");
    {
        size_t N = 0;
        expect("NULL offsets", check_offsets(nullptr, 1, N), false, "NULL argument");
        expect("NULL offsets, no structure", check_offsets(nullptr, 0, N), false, "NULL argument");
    }

    // ---- the columns, N and n_points
    const float col[1] = {0.0f};
    expect("n_points 0", check_points(1, col, col, col, col, true, 0), false, "n_points must be in [1, 2^31 - 1)");
    expect("n_points 2^31 - 1", check_points(1, col, col, col, col, true, 0x7FFFFFFFull), false, "n_points must be in [1, 2^31 - 1)");
    expect("n_points 1", check_points(1, col, col, col, col, true, 1), true);
    expect("n_points 2^31 - 2", check_points(1, col, col, col, col, true, 0x7FFFFFFEull), true);
    expect("NULL x, one atom", check_points(1, nullptr, col, col, col, true, 100), false, "NULL argument");
    expect("NULL y, one atom", check_points(1, col, nullptr, col, col, true, 100), false, "NULL argument");
    expect("NULL z, one atom", check_points(1, col, col, nullptr, col, true, 100), false, "NULL argument");
    expect("NULL radius, one atom", check_points(1, col, col, col, nullptr, true, 100), false, "NULL argument");
    expect("NULL columns, no atom", check_points(0, nullptr, nullptr, nullptr, nullptr, true, 100), true);
    expect("NULL columns, no atom, no n_points", check_columns(0, nullptr, nullptr, nullptr, nullptr, true), true);
    expect("a missing output, no atom", check_points(0, nullptr, nullptr, nullptr, nullptr, false, 100), false, "NULL argument");
    expect("2^31 - 2 atoms", check_columns(0x7FFFFFFEull, col, col, col, col, true), true);
    expect("2^31 - 1 atoms", check_columns(0x7FFFFFFFull, col, col, col, col, true), false, "more than 2^31 - 1 atoms");

    // ---- the link length
    expect("link -0.0", check_link(-0.0f), true);
    expect("link 0", check_link(0.0f), true);
    expect("link 1.5", check_link(1.5f), true);
    expect("link NaN", check_link(std::numeric_limits<float>::quiet_NaN()), false, "link must be finite and not negative");
    expect("link -1", check_link(-1.0f), false, "link must be finite and not negative");
    expect("link +inf", check_link(std::numeric_limits<float>::infinity()), false, "link must be finite and not negative");

    // ---- the input's description: a single structure owns its offsets
    {
        Cols one(col, col, col, col, nullptr);
        const char *msg = one.fix(Form::one(7));
        if (msg || one.S != 1 || one.N != 7 || one.so != one.one || one.so[0] != 0 || one.so[1] != 7) {
            std::printf("FAIL Cols of a single structure\n");
            failures++;
        }
        // (heap arrays of exactly the entries given, as in offsets(): one read past them is the sanitizer's)
        const std::vector<uint32_t> so = {0, 3, 7};
        Cols many(col, col, col, col, nullptr);
        msg = many.fix(Form::many(so.data(), 2));
        if (msg || many.S != 2 || many.N != 7 || many.so != so.data()) {
            std::printf("FAIL Cols of structure_offsets\n");
            failures++;
        }
        const std::vector<uint32_t> falling = {0, 5, 4};
        Cols bad(col, col, col, col, nullptr);
        bad.N = 12345;
        expect("Cols of falling offsets", bad.fix(Form::many(falling.data(), 2)), false, "structure_offsets must be non-decreasing");
        if (bad.N != 0) {
            std::printf("FAIL Cols of falling offsets: N = %zu, expected 0\n", bad.N);
            failures++;
        }
        const std::vector<uint32_t> first = {0};
        Cols none(col, col, col, col, nullptr);
        none.N = 12345;
        msg = none.fix(Form::many(first.data(), 0));
        if (msg || none.S != 0 || none.N != 0 || none.so != first.data()) {
            std::printf("FAIL Cols of no structure\n");
            failures++;
        }
    }

    if (failures) return 1;
    std::printf("entry checks ok\n");
    return 0;
}
