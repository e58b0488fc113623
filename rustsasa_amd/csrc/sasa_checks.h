// The argument rules of the SASA entry points - rsasa_calculate_sasa_internal, _soa, _batch, _trajectory,
// rsasa_batch_enqueue and rsasa_segment_sums; rsasa_host_batch_enqueue hands its arguments to a worker's
// rsasa_calculate_sasa_batch, whose verdict the wait returns.  Plain host C++ in the manner of entry_checks.h: no HIP, no
// context, nothing is written but a rule's `empty`.  A rule returns the message of the first thing it finds wrong, or null
// when the arguments stand; the entry points turn a message into RSASA_ERR_INVALID_ARGUMENT.  `empty`: the arguments
// stand and there is nothing to compute (RSASA_OK at once).
//
// Every entry point opens with its rule: behind resolve_ctx, before the context's mutex is taken, a buffer reserved, a
// byte uploaded, or a column or offset read for anything but a rule.  Nothing behind the opening looks again - the small
// path, the call combiner, the pipelined path and the enqueue of a checked batch (enqueue_checked) assume what is written
// here.
//
// The bounds are this path's own and NOT those of the neighbour families (entry_checks.h): n_points in [1, 2^24], sizes
// below 0xFFFFFFF0, a probe that is finite and not negative (-0.0 is 0).
//
// Two decisions.  (1) Where the paths used to disagree, rsasa_batch_enqueue's answer holds: the span of the structure
// offsets comes before their order, and a first offset other than 0 is refused on every path (a host batch of one
// sub-batch used to compute the atoms from structure_offsets[0] on and leave the ones in front unwritten).  (2) The
// rules answer before the device batches in flight are waited for: a call that is itself invalid no longer reports an
// earlier batch's deferred error first - that error stays with its batch for the next wait.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/rustsasa_amd.h"

namespace rsasa {

constexpr size_t kSasaMaxPoints = size_t(1) << 24;
inline bool sasa_size_fits(size_t n) { return n < 0xFFFFFFF0ull; }  // 32-bit indices, with room for the kernels' padding

// offsets[0 .. n] fall somewhere.  (Branch-free: vectorised; a proteome batch has a million and a half residue offsets.)
inline bool any_falling(const uint32_t *offsets, size_t n)
{
    uint32_t falling = 0;
    for (size_t k = 0; k < n; k++) falling |= (uint32_t)(offsets[k] > offsets[k + 1]);
    return falling != 0;
}

// The lattice and the probe: n_points, then probe_radius.
inline const char *check_sphere(size_t n_points, float probe)
{
    if (n_points == 0 || n_points > kSasaMaxPoints) return "n_points must be in [1, 2^24]";
    if (!(probe >= 0.0f) || !std::isfinite(probe)) return "probe_radius must be finite and >= 0";
    return nullptr;
}

// The structure offsets of a host batch, structure_offsets[0 .. n_structures] (their last entry IS the batch's atom
// count): there, the first entry 0, non-decreasing.  check_host_offsets_there is the first of the three by itself - what
// rsasa_calculate_sasa_batch has to know before it can read N.
inline const char *check_host_offsets_there(const uint32_t *so, size_t n_structures)
{
    if (n_structures && !so) return "structure_offsets is NULL";
    return nullptr;
}
inline const char *check_span(const uint32_t *so, size_t n_structures, size_t n_atoms)
{
    if (n_structures && (so[0] != 0 || so[n_structures] != n_atoms)) return "structure_offsets must span [0, n_atoms]";
    if (any_falling(so, n_structures)) return "structure_offsets must be non-decreasing";
    return nullptr;
}
inline const char *check_host_offsets(const uint32_t *so, size_t n_structures)
{
    if (const char *msg = check_host_offsets_there(so, n_structures)) return msg;
    return check_span(so, n_structures, n_structures ? so[n_structures] : 0);
}

// Residue offsets[0 .. n_residues] against the N atoms they index: none past N, non-decreasing.
inline const char *check_residue_offsets(const uint32_t *ro, size_t n_residues, size_t N)
{
    if (ro[n_residues] > N) return "residue_offsets exceed n_atoms";
    if (any_falling(ro, n_residues)) return "residue_offsets must be non-decreasing";
    return nullptr;
}

inline bool columns_there(const float *x, const float *y, const float *z, const float *r) { return x && y && z && r; }

// rsasa_calculate_sasa_batch: the offsets are there; columns; outputs; empty; the residue offsets; the sphere; sizes; the
// offsets' span and order.
inline const char *check_host_batch(const float *x, const float *y, const float *z, const float *r, const uint32_t *so,
                                    size_t n_structures, float probe, size_t n_points, const float *out_atom,
                                    const uint32_t *ro, size_t n_residues, const float *out_res, bool &empty)
{
    empty = false;
    const char *msg = check_host_offsets_there(so, n_structures);
    if (msg) return msg;
    const size_t N = n_structures ? so[n_structures] : 0;
    const bool want_res = ro && n_residues;
    if (N && !columns_there(x, y, z, r)) return "coordinate / radius arrays are NULL";
    if (want_res && !out_res) return "out_residue_sasa is NULL";
    if (N && !out_atom && !want_res) return "no output requested";
    if (N == 0 && !want_res) {  // empty input -> empty output (tests/sanity.rs:149-157)
        empty = true;
        return nullptr;
    }
    if (want_res && (msg = check_residue_offsets(ro, n_residues, N))) return msg;
    if ((msg = check_sphere(n_points, probe))) return msg;
    // (n_residues without offsets asks for nothing and is not looked at, as ever)
    if (!sasa_size_fits(N) || !sasa_size_fits(n_structures) || (want_res && !sasa_size_fits(n_residues))) return "batch too large for 32-bit indices";
    return check_span(so, n_structures, N);
}

// rsasa_calculate_sasa_soa and _internal, behind their two bare refusals (n_atoms does not fit, no out_sasa): the
// columns (or records: columns = they are there), empty, the sphere.  n_points = 0 with no atoms is therefore no error.
inline const char *check_structure_call(bool columns, size_t n_atoms, float probe, size_t n_points, bool &empty)
{
    empty = false;
    if (n_atoms && !columns) return "coordinate / radius arrays are NULL";
    if (n_atoms == 0) {  // empty input -> empty output (tests/sanity.rs:149-157)
        empty = true;
        return nullptr;
    }
    return check_sphere(n_points, probe);
}

// rsasa_calculate_sasa_trajectory: empty; inputs; outputs; sizes; the residue offsets of one frame; the sphere.
inline const char *check_trajectory(const float *xyz, size_t n_frames, size_t n_atoms, const float *radius, float probe,
                                    size_t n_points, const float *out_atom, const uint32_t *ro, size_t n_residues,
                                    const float *out_res, bool &empty)
{
    empty = n_frames == 0 || n_atoms == 0;
    if (empty) return nullptr;
    const bool want_res = ro && n_residues;
    if (!xyz || !radius) return "xyz / radius are NULL";
    if (want_res && !out_res) return "out_residue_sasa is NULL";
    if (!out_atom && !want_res) return "no output requested";
    if (!sasa_size_fits(n_atoms) || !sasa_size_fits(n_frames) || !sasa_size_fits(n_residues)) return "trajectory too large for 32-bit indices";
    if (want_res)
        if (const char *msg = check_residue_offsets(ro, n_residues, n_atoms)) return msg;
    return check_sphere(n_points, probe);
}

// rsasa_batch_enqueue's descriptor: there; the sphere; sizes; columns; the host's structure offsets - there, their span,
// their order; atoms need structures; residue sums need their output.
inline const char *check_device_batch(const rsasa_device_batch_t *b, float probe, size_t n_points)
{
    if (!b) return "batch is NULL";
    if (const char *msg = check_sphere(n_points, probe)) return msg;
    if (!sasa_size_fits(b->n_atoms) || !sasa_size_fits(b->n_structures) || !sasa_size_fits(b->n_residues)) return "batch too large for 32-bit indices";
    if (b->n_atoms && !columns_there(b->x, b->y, b->z, b->radius)) return "coordinate / radius arrays are NULL";
    if (b->n_structures && !b->structure_offsets_host) return "structure_offsets_host is NULL";
    if (const char *msg = check_span(b->structure_offsets_host, b->n_structures, b->n_atoms)) return msg;
    if (!b->n_structures && b->n_atoms) return "atoms without structures";
    if (b->n_residues && b->residue_offsets && !b->out_residue_sasa) return "out_residue_sasa is NULL";
    return nullptr;
}

// rsasa_segment_sums: empty; the arrays; sizes and the last offset; the offsets' order.
inline const char *check_segments(const float *values, size_t n_values, const uint32_t *offsets, size_t n_segments,
                                  const float *out, bool &empty)
{
    empty = n_segments == 0;
    if (empty) return nullptr;
    if (!offsets || !out || (n_values && !values)) return "NULL argument";
    if (!sasa_size_fits(n_values) || !sasa_size_fits(n_segments) || offsets[n_segments] > n_values) return "offsets exceed n_values";
    if (any_falling(offsets, n_segments)) return "offsets must be non-decreasing";
    return nullptr;
}

}  // namespace rsasa
