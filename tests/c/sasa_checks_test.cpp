// The argument rules of the SASA entry points (rustsasa_amd/csrc/sasa_checks.h) at both sides of every bound, and the
// order inside every composite rule.  Stand-alone: host compiler, no HIP, built with -fsanitize=address,undefined by
// tests/test_sasa_checks_cpu.py, so a rule that reads an offset or a column it should not have read ends the program.
// Prints "sasa checks ok" and returns 0 when every verdict is the listed one.
#include "sasa_checks.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace rsasa;

static int failures = 0;

// msg against the message wanted (null: the rule passes)
static void expect(const char *what, const char *msg, const char *want)
{
    const bool good = want ? msg != nullptr && std::strcmp(msg, want) == 0 : msg == nullptr;
    if (!good) {
        std::printf("FAIL %s: expected %s, got %s\n", what, want ? want : "OK", msg ? msg : "OK");
        failures++;
    }
}

static void expect_empty(const char *what, bool empty, bool want)
{
    if (empty != want) {
        std::printf("FAIL %s: empty = %d, expected %d\n", what, (int)empty, (int)want);
        failures++;
    }
}

static const char *const POINTS = "n_points must be in [1, 2^24]";
static const char *const PROBE = "probe_radius must be finite and >= 0";
static const char *const SPAN = "structure_offsets must span [0, n_atoms]";
static const char *const ORDER = "structure_offsets must be non-decreasing";
static const char *const SO_NULL = "structure_offsets is NULL";
static const char *const COLS = "coordinate / radius arrays are NULL";
static const char *const RES_OUT = "out_residue_sasa is NULL";
static const char *const NO_OUT = "no output requested";
static const char *const RES_EXCEED = "residue_offsets exceed n_atoms";
static const char *const RES_ORDER = "residue_offsets must be non-decreasing";
static const char *const BATCH_BIG = "batch too large for 32-bit indices";

// (heap copies of exactly the entries given: one read past them is the sanitizer's)
using U32 = std::vector<uint32_t>;
using F32 = std::vector<float>;

static const float NaN = std::numeric_limits<float>::quiet_NaN(), Inf = std::numeric_limits<float>::infinity();

// a host batch of three-element columns with these offsets and everything else in order
static const char *host_batch(const U32 &so, size_t S, float probe = 1.4f, size_t n_points = 100, bool *empty_out = nullptr)
{
    const F32 c(3, 0.0f);
    F32 out(3, 0.0f);
    bool empty;
    const char *msg = check_host_batch(c.data(), c.data(), c.data(), c.data(), so.data(), S, probe, n_points, out.data(), nullptr, 0, nullptr, empty);
    if (empty_out) *empty_out = empty;
    return msg;
}

int main()
{
    // ---- the sphere: n_points in [1, 2^24], a probe that is finite and not negative
    expect("n_points 0", check_sphere(0, 1.4f), POINTS);
    expect("n_points 1", check_sphere(1, 1.4f), nullptr);
    expect("n_points 2^24", check_sphere(size_t(1) << 24, 1.4f), nullptr);
    expect("n_points 2^24 + 1", check_sphere((size_t(1) << 24) + 1, 1.4f), POINTS);
    expect("probe -0.0", check_sphere(100, -0.0f), nullptr);
    expect("probe 0", check_sphere(100, 0.0f), nullptr);
    expect("probe NaN", check_sphere(100, NaN), PROBE);
    expect("probe +inf", check_sphere(100, Inf), PROBE);
    expect("probe -1", check_sphere(100, -1.0f), PROBE);
    expect("n_points before probe", check_sphere(0, NaN), POINTS);

    // ---- sizes, as numbers
    if (!sasa_size_fits(0xFFFFFFEFull) || sasa_size_fits(0xFFFFFFF0ull) || !sasa_size_fits(0)) {
        std::printf("FAIL sasa_size_fits at 0xFFFFFFEF / 0xFFFFFFF0\n");
        failures++;
    }

    // ---- a host batch's structure offsets
    expect("offsets NULL", check_host_offsets(nullptr, 2), SO_NULL);
    expect("offsets NULL, no structure (the empty form)", check_host_offsets(nullptr, 0), nullptr);
    expect("offsets {0}, no structure", check_host_offsets(U32{0}.data(), 0), nullptr);
    expect("offsets {7}, no structure: not read", check_host_offsets(U32{7}.data(), 0), nullptr);
    expect("offsets {0, 3}", check_host_offsets(U32{0, 3}.data(), 1), nullptr);
    expect("offsets {0, 0, 3, 3}", check_host_offsets(U32{0, 0, 3, 3}.data(), 3), nullptr);
    expect("offsets {1, 3}", check_host_offsets(U32{1, 3}.data(), 1), SPAN);
    expect("offsets {0, 5, 3}", check_host_offsets(U32{0, 5, 3}.data(), 2), ORDER);
    expect("offsets {0, 3 500 000, 3 000 000}", check_host_offsets(U32{0, 3500000, 3000000}.data(), 2), ORDER);
    expect("offsets {1, 6 000 000, 3 000 000}: span before order", check_host_offsets(U32{1, 6000000, 3000000}.data(), 2), SPAN);

    // ---- a device batch's offsets: the span is against n_atoms at both ends
    expect("span {0, 3} of 3 atoms", check_span(U32{0, 3}.data(), 1, 3), nullptr);
    expect("span {0, 3} of 4 atoms", check_span(U32{0, 3}.data(), 1, 4), SPAN);
    expect("span {0, 5, 3} of 3 atoms", check_span(U32{0, 5, 3}.data(), 2, 3), ORDER);

    // ---- residue offsets against N
    expect("residues {0, 2, 3} of 3", check_residue_offsets(U32{0, 2, 3}.data(), 2, 3), nullptr);
    expect("residues {1, 2} of 3 (a part of the atoms)", check_residue_offsets(U32{1, 2}.data(), 1, 3), nullptr);
    expect("residues one past N", check_residue_offsets(U32{0, 2, 4}.data(), 2, 3), RES_EXCEED);
    expect("residues, a falling pair", check_residue_offsets(U32{0, 2, 1, 3}.data(), 3, 3), RES_ORDER);
    expect("residues, exceed before order", check_residue_offsets(U32{0, 9, 4}.data(), 2, 3), RES_EXCEED);

    // ---- rsasa_calculate_sasa_batch, in the order of its verdicts
    {
        const F32 c(3, 0.0f);
        F32 out(3, 0.0f);
        const float *p = c.data();
        const U32 so{0, 3}, ro{0, 2, 3}, ro_past{0, 2, 4}, ro_fall{0, 2, 1, 3}, so_bad{1, 3};
        bool empty = true;
        expect("batch: in order", check_host_batch(p, p, p, p, so.data(), 1, 1.4f, 100, out.data(), ro.data(), 2, out.data(), empty), nullptr);
        expect_empty("batch: in order", empty, false);
        expect("batch: offsets NULL before columns", check_host_batch(nullptr, p, p, p, nullptr, 1, NaN, 0, nullptr, nullptr, 0, nullptr, empty), SO_NULL);
        expect("batch: columns before out_residue_sasa", check_host_batch(p, nullptr, p, p, so.data(), 1, 1.4f, 100, out.data(), ro.data(), 2, nullptr, empty), COLS);
        expect("batch: out_residue_sasa before residue offsets", check_host_batch(p, p, p, p, so.data(), 1, 1.4f, 100, nullptr, ro_past.data(), 2, nullptr, empty), RES_OUT);
        expect("batch: no output before n_points", check_host_batch(p, p, p, p, so.data(), 1, 1.4f, 0, nullptr, nullptr, 0, nullptr, empty), NO_OUT);
        expect("batch: no structure, n_points 0", check_host_batch(nullptr, nullptr, nullptr, nullptr, nullptr, 0, NaN, 0, nullptr, nullptr, 0, nullptr, empty), nullptr);
        expect_empty("batch: no structure", empty, true);
        expect("batch: no atoms, n_points 0", check_host_batch(nullptr, nullptr, nullptr, nullptr, U32{0, 0}.data(), 1, 1.4f, 0, nullptr, nullptr, 0, nullptr, empty), nullptr);
        expect_empty("batch: no atoms", empty, true);
        expect("batch: residues exceed before n_points", check_host_batch(p, p, p, p, so.data(), 1, 1.4f, 0, out.data(), ro_past.data(), 2, out.data(), empty), RES_EXCEED);
        expect("batch: residues fall before n_points", check_host_batch(p, p, p, p, so.data(), 1, 1.4f, 0, out.data(), ro_fall.data(), 3, out.data(), empty), RES_ORDER);
        expect("batch: n_points before probe", check_host_batch(p, p, p, p, so.data(), 1, NaN, 0, out.data(), nullptr, 0, nullptr, empty), POINTS);
        expect("batch: probe before the span", check_host_batch(p, p, p, p, so_bad.data(), 1, NaN, 100, out.data(), nullptr, 0, nullptr, empty), PROBE);
        expect("batch: 0xFFFFFFF0 atoms (claimed) before the span", check_host_batch(p, p, p, p, U32{1, 0xFFFFFFF0u}.data(), 1, 1.4f, 100, out.data(), nullptr, 0, nullptr, empty), BATCH_BIG);
        expect("batch: 0xFFFFFFEF atoms (claimed)", check_host_batch(p, p, p, p, U32{0, 0xFFFFFFEFu}.data(), 1, 1.4f, 100, out.data(), nullptr, 0, nullptr, empty), nullptr);
        expect_empty("batch: 0xFFFFFFEF atoms", empty, false);
        expect("batch: 0xFFFFFFF0 residues without offsets are not asked for", check_host_batch(p, p, p, p, so.data(), 1, 1.4f, 100, out.data(), nullptr, 0xFFFFFFF0ull, nullptr, empty), nullptr);
    }
    expect("batch {1, 3}", host_batch({1, 3}, 1), SPAN);
    expect("batch {0, 5, 3}", host_batch({0, 5, 3}, 2), ORDER);
    expect("batch {0, 3 500 000, 3 000 000}", host_batch({0, 3500000, 3000000}, 2), ORDER);
    expect("batch {1, 6 000 000, 3 000 000}", host_batch({1, 6000000, 3000000}, 2), SPAN);
    expect("batch {0, 200 000 000, 400 000 000}, n_points 0", host_batch({0, 200000000, 400000000}, 2, 1.4f, 0), POINTS);
    expect("batch n_points 2^24 + 1", host_batch({0, 3}, 1, 1.4f, (size_t(1) << 24) + 1), POINTS);
    expect("batch n_points 2^24", host_batch({0, 3}, 1, 1.4f, size_t(1) << 24), nullptr);
    expect("batch probe -0.0", host_batch({0, 3}, 1, -0.0f), nullptr);

    // ---- rsasa_calculate_sasa_soa / _internal
    {
        bool empty = true;
        expect("call: in order", check_structure_call(true, 3, 1.4f, 100, empty), nullptr);
        expect_empty("call: in order", empty, false);
        expect("call: columns before n_points", check_structure_call(false, 3, NaN, 0, empty), COLS);
        expect("call: no atoms, no columns, n_points 0", check_structure_call(false, 0, NaN, 0, empty), nullptr);
        expect_empty("call: no atoms", empty, true);
        expect("call: n_points 0", check_structure_call(true, 3, 1.4f, 0, empty), POINTS);
        expect("call: n_points before probe", check_structure_call(true, 3, -1.0f, 0, empty), POINTS);
        expect("call: probe NaN", check_structure_call(true, 3, NaN, 100, empty), PROBE);
    }

    // ---- rsasa_calculate_sasa_trajectory
    {
        const F32 xyz(18, 0.0f), r(3, 1.7f);
        F32 out(6, 0.0f);
        const U32 ro{0, 2, 3}, ro_past{0, 2, 4}, ro_fall{0, 2, 1, 3};
        const char *const BIG = "trajectory too large for 32-bit indices";
        bool empty = true;
        expect("trajectory: in order", check_trajectory(xyz.data(), 2, 3, r.data(), 1.4f, 100, out.data(), ro.data(), 2, out.data(), empty), nullptr);
        expect_empty("trajectory: in order", empty, false);
        expect("trajectory: no frame, everything else wrong", check_trajectory(nullptr, 0, 3, nullptr, NaN, 0, nullptr, nullptr, 0, nullptr, empty), nullptr);
        expect_empty("trajectory: no frame", empty, true);
        expect("trajectory: no atom", check_trajectory(nullptr, 2, 0, nullptr, NaN, 0, nullptr, nullptr, 0, nullptr, empty), nullptr);
        expect_empty("trajectory: no atom", empty, true);
        expect("trajectory: xyz NULL before out_residue_sasa", check_trajectory(nullptr, 2, 3, r.data(), 1.4f, 100, out.data(), ro.data(), 2, nullptr, empty), "xyz / radius are NULL");
        expect("trajectory: radius NULL", check_trajectory(xyz.data(), 2, 3, nullptr, 1.4f, 100, out.data(), nullptr, 0, nullptr, empty), "xyz / radius are NULL");
        expect("trajectory: out_residue_sasa before sizes", check_trajectory(xyz.data(), 0xFFFFFFF0ull, 3, r.data(), 1.4f, 100, out.data(), ro.data(), 2, nullptr, empty), RES_OUT);
        expect("trajectory: no output before sizes", check_trajectory(xyz.data(), 0xFFFFFFF0ull, 3, r.data(), 1.4f, 100, nullptr, nullptr, 0, nullptr, empty), NO_OUT);
        expect("trajectory: 0xFFFFFFF0 frames before n_points", check_trajectory(xyz.data(), 0xFFFFFFF0ull, 3, r.data(), 1.4f, 0, out.data(), nullptr, 0, nullptr, empty), BIG);
        expect("trajectory: 0xFFFFFFEF frames (claimed)", check_trajectory(xyz.data(), 0xFFFFFFEFull, 3, r.data(), 1.4f, 100, out.data(), nullptr, 0, nullptr, empty), nullptr);
        expect("trajectory: 0xFFFFFFF0 atoms before the residue offsets", check_trajectory(xyz.data(), 2, 0xFFFFFFF0ull, r.data(), 1.4f, 100, out.data(), ro_fall.data(), 3, out.data(), empty), BIG);
        expect("trajectory: 0xFFFFFFF0 residues, no offsets", check_trajectory(xyz.data(), 2, 3, r.data(), 1.4f, 100, out.data(), nullptr, 0xFFFFFFF0ull, nullptr, empty), BIG);
        expect("trajectory: residues exceed before n_points", check_trajectory(xyz.data(), 2, 3, r.data(), 1.4f, 0, out.data(), ro_past.data(), 2, out.data(), empty), RES_EXCEED);
        expect("trajectory: residues fall before probe", check_trajectory(xyz.data(), 2, 3, r.data(), NaN, 100, out.data(), ro_fall.data(), 3, out.data(), empty), RES_ORDER);
        expect("trajectory: n_points before probe", check_trajectory(xyz.data(), 2, 3, r.data(), NaN, 0, out.data(), nullptr, 0, nullptr, empty), POINTS);
        expect("trajectory: probe +inf", check_trajectory(xyz.data(), 2, 3, r.data(), Inf, 100, out.data(), nullptr, 0, nullptr, empty), PROBE);
    }

    // ---- rsasa_batch_enqueue's descriptor (the device pointers are only compared with NULL)
    {
        const F32 dev(1, 0.0f);
        const U32 so{0, 3}, so_bad{1, 3}, so_fall{0, 5, 3}, ro(1, 0u);
        rsasa_device_batch_t good{};
        good.x = good.y = good.z = good.radius = dev.data();
        good.structure_offsets_host = so.data();
        good.n_structures = 1;
        good.n_atoms = 3;
        F32 out(1, 0.0f);
        good.out_atom_sasa = out.data();
        rsasa_device_batch_t b = good;
        expect("device: in order", check_device_batch(&good, 1.4f, 100), nullptr);
        expect("device: NULL before n_points", check_device_batch(nullptr, NaN, 0), "batch is NULL");
        expect("device: n_points before probe", check_device_batch(&good, NaN, 0), POINTS);
        b.n_atoms = 0xFFFFFFF0ull;
        expect("device: probe before sizes", check_device_batch(&b, NaN, 100), PROBE);
        b.x = nullptr;
        expect("device: 0xFFFFFFF0 atoms before columns", check_device_batch(&b, 1.4f, 100), BATCH_BIG);
        b.n_atoms = 0xFFFFFFEFull;
        expect("device: 0xFFFFFFEF atoms: the columns' turn", check_device_batch(&b, 1.4f, 100), COLS);
        b = good; b.n_structures = 0xFFFFFFF0ull;
        expect("device: 0xFFFFFFF0 structures", check_device_batch(&b, 1.4f, 100), BATCH_BIG);
        b = good; b.n_residues = 0xFFFFFFF0ull;
        expect("device: 0xFFFFFFF0 residues", check_device_batch(&b, 1.4f, 100), BATCH_BIG);
        b = good; b.radius = nullptr; b.structure_offsets_host = nullptr;
        expect("device: columns before the offsets", check_device_batch(&b, 1.4f, 100), COLS);
        b = good; b.structure_offsets_host = nullptr; b.n_residues = 1; b.residue_offsets = ro.data();
        expect("device: offsets NULL before out_residue_sasa", check_device_batch(&b, 1.4f, 100), "structure_offsets_host is NULL");
        b = good; b.structure_offsets_host = so_bad.data();
        expect("device: {1, 3}", check_device_batch(&b, 1.4f, 100), SPAN);
        b = good; b.n_atoms = 4;
        expect("device: {0, 3} of 4 atoms", check_device_batch(&b, 1.4f, 100), SPAN);
        b = good; b.structure_offsets_host = so_fall.data(); b.n_structures = 2;
        expect("device: {0, 5, 3}", check_device_batch(&b, 1.4f, 100), ORDER);
        b = good; b.structure_offsets_host = nullptr; b.n_structures = 0; b.n_residues = 1; b.residue_offsets = ro.data();
        expect("device: atoms without structures before out_residue_sasa", check_device_batch(&b, 1.4f, 100), "atoms without structures");
        b = good; b.n_residues = 1; b.residue_offsets = ro.data();
        expect("device: residue sums without their output", check_device_batch(&b, 1.4f, 100), RES_OUT);
        b.residue_offsets = nullptr;
        expect("device: residues without offsets are not asked for", check_device_batch(&b, 1.4f, 100), nullptr);
        rsasa_device_batch_t none{};
        expect("device: an empty batch", check_device_batch(&none, 1.4f, 100), nullptr);
    }

    // ---- rsasa_segment_sums
    {
        const F32 v(3, 1.0f);
        F32 out(2, 0.0f);
        const U32 o{0, 2, 3}, past{0, 2, 4}, fall{0, 3, 2, 3};
        bool empty = true;
        expect("segments: in order", check_segments(v.data(), 3, o.data(), 2, out.data(), empty), nullptr);
        expect_empty("segments: in order", empty, false);
        expect("segments: none, everything else NULL", check_segments(nullptr, 3, nullptr, 0, nullptr, empty), nullptr);
        expect_empty("segments: none", empty, true);
        expect("segments: offsets NULL", check_segments(v.data(), 3, nullptr, 2, out.data(), empty), "NULL argument");
        expect("segments: out NULL before the last offset", check_segments(v.data(), 3, past.data(), 2, nullptr, empty), "NULL argument");
        expect("segments: values NULL", check_segments(nullptr, 3, o.data(), 2, out.data(), empty), "NULL argument");
        expect("segments: no values, none needed", check_segments(nullptr, 0, U32{0, 0}.data(), 1, out.data(), empty), nullptr);
        expect("segments: one past n_values", check_segments(v.data(), 3, past.data(), 2, out.data(), empty), "offsets exceed n_values");
        expect("segments: 0xFFFFFFF0 values (claimed)", check_segments(v.data(), 0xFFFFFFF0ull, o.data(), 2, out.data(), empty), "offsets exceed n_values");
        expect("segments: 0xFFFFFFEF values (claimed)", check_segments(v.data(), 0xFFFFFFEFull, o.data(), 2, out.data(), empty), nullptr);
        expect("segments: 0xFFFFFFF0 segments: the offsets are not read", check_segments(v.data(), 3, o.data(), 0xFFFFFFF0ull, out.data(), empty), "offsets exceed n_values");
        expect("segments: a falling pair", check_segments(v.data(), 3, fall.data(), 3, out.data(), empty), "offsets must be non-decreasing");
        expect("segments: exceed before order", check_segments(v.data(), 2, fall.data(), 3, out.data(), empty), "offsets exceed n_values");
    }

    if (failures) return 1;
    std::printf("sasa checks ok\n");
    return 0;
}
