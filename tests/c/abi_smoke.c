/* Plain C99 consumer of include/rustsasa_amd.h: the header must compile as C and the
 * library must link and behave without any C++/HIP types on the caller's side.
 * Exit code 0 = ok on a GPU host, 0 with "no device" printed on a GPU-less host. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rustsasa_amd.h"

int main(void)
{
    if (rsasa_abi_version() != RSASA_ABI_VERSION) return 10;
    if (sizeof(rsasa_atom_t) != 24) return 11;
    int n_dev = -1;
    if (rsasa_device_count(&n_dev) != RSASA_OK) return 12;
    float sx[100], sy[100], sz[100];
    if (rsasa_sphere_points(100, sx, sy, sz) != RSASA_OK || sz[0] != 1.0f) return 13;

    rsasa_context_t *ctx = NULL;
    int rc = rsasa_context_create(0, &ctx);
    if (n_dev == 0) {
        if (rc != RSASA_ERR_NO_DEVICE || ctx != NULL) return 14;
        printf("no device: %s\n", rsasa_status_string(rc));
        return 0;
    }
    if (rc != RSASA_OK) return 15;

    /* two overlapping spheres (reference tests/sanity.rs:64-85) + one far away */
    rsasa_atom_t atoms[3];
    memset(atoms, 0, sizeof atoms);
    atoms[0].radius = atoms[1].radius = atoms[2].radius = 2.0f;
    atoms[1].position[0] = 4.0f;
    atoms[2].position[0] = 40.0f;
    atoms[0].id = 1; atoms[1].id = 2; atoms[2].id = 3;
    float out[3] = {-1.f, -1.f, -1.f};
    rc = rsasa_calculate_sasa_internal(ctx, atoms, 3, 1.4f, 5000, -1, out);
    if (rc != RSASA_OK) { printf("%s\n", rsasa_context_last_error(ctx)); return 16; }
    const double pi = 3.14159265358979323846, r = 3.4;
    const double full = 4 * pi * r * r, exposed = full - 2 * pi * r * (r - 2.0);
    if (out[0] < exposed * 0.99 || out[0] > exposed * 1.01) return 17;
    if (out[1] < exposed * 0.99 || out[1] > exposed * 1.01) return 18;
    if (out[2] < full * 0.999 || out[2] > full * 1.001) return 19;
    /* ABI 2: lane count round trip, NUMA binding of the calling thread (node -1: nothing to bind), wait-all with
     * nothing in flight */
    int w = 0, node = -2;
    if (rsasa_context_set_simd_width(ctx, 4) != RSASA_OK || rsasa_context_get_simd_width(ctx, &w) != RSASA_OK || w != 4) return 23;
    if (rsasa_context_set_simd_width(ctx, 3) != RSASA_ERR_INVALID_ARGUMENT) return 24;
    if (rsasa_context_set_simd_width(ctx, 8) != RSASA_OK) return 25;
    if (rsasa_context_bind_thread(ctx, &node) != RSASA_OK || node < -1) return 26;
    if (rsasa_batch_wait_all(ctx) != RSASA_OK || rsasa_batch_wait(ctx) != RSASA_OK) return 27;
    /* ABI 3: a second context with the first one's settings; a stream of host batches: two queued, waited for in order,
     * a wait with nothing queued returns at once */
    {
        rsasa_context_t *other = NULL;
        int w2 = 0;
        if (rsasa_context_create(0, &other) != RSASA_OK) return 28;
        if (rsasa_context_set_simd_width(ctx, 16) != RSASA_OK || rsasa_context_clone_settings(other, ctx) != RSASA_OK ||
            rsasa_context_get_simd_width(other, &w2) != RSASA_OK || w2 != 16) return 29;
        if (rsasa_context_set_simd_width(ctx, 8) != RSASA_OK || rsasa_context_destroy(other) != RSASA_OK) return 30;
        float x[3] = {0.f, 4.f, 40.f}, y[3] = {0.f, 0.f, 0.f}, z[3] = {0.f, 0.f, 0.f}, rad[3] = {2.f, 2.f, 2.f};
        uint32_t so[2] = {0u, 3u};
        float a1[3] = {-1.f, -1.f, -1.f}, a2[3] = {-1.f, -1.f, -1.f};
        if (rsasa_host_batch_wait(ctx) != RSASA_OK) return 31;
        if (rsasa_host_batch_enqueue(ctx, x, y, z, rad, NULL, so, 1, 1.4f, 5000, a1, NULL, 0, NULL) != RSASA_OK) return 32;
        if (rsasa_host_batch_enqueue(ctx, x, y, z, rad, NULL, so, 1, 1.4f, 5000, a2, NULL, 0, NULL) != RSASA_OK) return 33;
        if (rsasa_host_batch_wait(ctx) != RSASA_OK || a1[0] != out[0] || a1[2] != out[2]) return 34;
        if (rsasa_host_batch_wait_all(ctx) != RSASA_OK || a2[1] != out[1]) return 35;
        uint64_t dropped = 99;
        if (rsasa_context_ids_dropped(ctx, &dropped) != RSASA_OK || dropped != 0) return 36;  /* (small batches are not checked) */
    }
    /* additive under ABI 4: neighbour lists, accessible points, contact counts and group contacts on the same three
     * spheres (labels 0, 1, 0), each sized first (RSASA_ERR_BUFFER_TOO_SMALL and the offsets), then filled */
    {
        float x[3] = {0.f, 4.f, 40.f}, y[3] = {0.f, 0.f, 0.f}, z[3] = {0.f, 0.f, 0.f}, rad[3] = {2.f, 2.f, 2.f};
        uint64_t id[3] = {1u, 2u, 3u};
        uint32_t group[3] = {0u, 1u, 0u}, so[2] = {0u, 3u};
        const size_t n_points = 5000, words = (5000 + 31) / 32;
        /* neighbour lists: {1}, {0}, {} */
        uint64_t offs[4] = {9u, 9u, 9u, 9u};
        rsasa_neighbor_t ent[2];
        const float no_override = NAN;   /* max_radius: the structure's own largest radius */
        if (rsasa_precompute_neighbors(ctx, x, y, z, rad, id, 3, NULL, 0, 1.4f, no_override, offs, NULL, 0) != RSASA_ERR_BUFFER_TOO_SMALL) return 40;
        if (offs[0] != 0 || offs[1] != 1 || offs[2] != 2 || offs[3] != 2) return 41;
        if (rsasa_precompute_neighbors(ctx, x, y, z, rad, id, 3, NULL, 0, 1.4f, no_override, offs, ent, 2) != RSASA_OK) return 42;
        if (offs[3] != 2 || ent[0].idx != 1 || ent[1].idx != 0) return 43;
        offs[1] = offs[2] = offs[3] = 9u;
        if (rsasa_precompute_neighbors_batch(ctx, x, y, z, rad, id, so, 1, 1.4f, no_override, offs, NULL, 0) != RSASA_ERR_BUFFER_TOO_SMALL) return 44;
        if (offs[0] != 0 || offs[1] != 1 || offs[2] != 2 || offs[3] != 2) return 45;
        if (rsasa_precompute_neighbors_batch(ctx, x, y, z, rad, id, so, 1, 1.4f, no_override, offs, ent, 2) != RSASA_OK) return 46;
        if (ent[0].idx != 1 || ent[1].idx != 0 || ent[0].threshold_squared != ent[1].threshold_squared) return 47;
        /* accessible points (nothing to size): popcount * area per point == out[], bit for bit */
        uint32_t *masks = (uint32_t *)calloc(3 * words, sizeof(uint32_t));
        float psasa[3] = {-1.f, -1.f, -1.f};
        size_t free_pts[3] = {0, 0, 0};
        if (!masks) return 48;
        if (rsasa_accessible_points(ctx, x, y, z, rad, id, 3, 1.4f, n_points, masks, psasa) != RSASA_OK) return 49;
        for (size_t i = 0; i < 3; i++) {
            for (size_t wd = 0; wd < words; wd++)
                for (uint32_t m = masks[i * words + wd]; m; m &= m - 1) free_pts[i]++;
            const float R = rad[i] + 1.4f;
            const float area = ((12.566371f * (R * R)) * (float)free_pts[i]) * (1.0f / (float)n_points);
            if (area != out[i] || psasa[i] != out[i]) return 50;
        }
        if (free_pts[2] != n_points || free_pts[0] == 0 || free_pts[0] >= n_points || free_pts[1] == 0 || free_pts[1] >= n_points) return 51;
        if (masks[2 * words + words - 1] != 0xFFu) return 52;   /* 5000 = 156 * 32 + 8: the padding bits are 0 */
        memset(masks, 0, 3 * words * sizeof(uint32_t));
        if (rsasa_accessible_points_batch(ctx, x, y, z, rad, id, so, 1, 1.4f, n_points, masks, NULL) != RSASA_OK) return 53;
        if (masks[2 * words] != 0xFFFFFFFFu || masks[2 * words + words - 1] != 0xFFu) return 54;
        free(masks);
        /* contact counts: one entry per list, so covered == exclusive == the buried points */
        uint32_t cov[2] = {7u, 7u}, exc[2] = {7u, 7u};
        float csasa[3] = {-1.f, -1.f, -1.f};
        offs[1] = offs[2] = offs[3] = 9u;
        if (rsasa_contact_points(ctx, x, y, z, rad, id, 3, 1.4f, n_points, offs, NULL, NULL, NULL, 0, NULL) != RSASA_ERR_BUFFER_TOO_SMALL) return 55;
        if (offs[0] != 0 || offs[1] != 1 || offs[2] != 2 || offs[3] != 2 || cov[0] != 7u) return 56;
        if (rsasa_contact_points(ctx, x, y, z, rad, id, 3, 1.4f, n_points, offs, ent, cov, exc, 2, csasa) != RSASA_OK) return 57;
        if (ent[0].idx != 1 || ent[1].idx != 0) return 58;
        for (size_t e = 0; e < 2; e++)
            if (cov[e] != exc[e] || cov[e] != n_points - free_pts[e]) return 59;
        if (csasa[0] != out[0] || csasa[1] != out[1] || csasa[2] != out[2]) return 60;
        cov[0] = exc[0] = 7u;
        if (rsasa_contact_points_batch(ctx, x, y, z, rad, id, so, 1, 1.4f, n_points, offs, ent, cov, exc, 1, NULL) != RSASA_ERR_BUFFER_TOO_SMALL) return 61;
        if (cov[0] != 7u || exc[0] != 7u || offs[3] != 2) return 62;
        if (rsasa_contact_points_batch(ctx, x, y, z, rad, id, so, 1, 1.4f, n_points, offs, ent, cov, exc, 2, NULL) != RSASA_OK) return 63;
        if (cov[0] != n_points - free_pts[0] || exc[1] != cov[1]) return 64;
        /* group contacts: atom 0 has one row (partner 1), atom 1 one row (partner 0), atom 2 none */
        uint32_t partner[2] = {7u, 7u}, buried[2] = {7u, 7u}, only[2] = {7u, 7u}, self_free[3] = {7u, 7u, 7u}, gfree[3] = {7u, 7u, 7u};
        float gsasa[3] = {-1.f, -1.f, -1.f};
        offs[1] = offs[2] = offs[3] = 9u;
        if (rsasa_group_contacts(ctx, x, y, z, rad, id, group, 3, 1.4f, n_points, offs, NULL, NULL, NULL, 0, self_free, gfree, NULL) != RSASA_ERR_BUFFER_TOO_SMALL) return 65;
        if (offs[0] != 0 || offs[1] != 1 || offs[2] != 2 || offs[3] != 2 || self_free[0] != 7u || gfree[2] != 7u) return 66;
        if (rsasa_group_contacts(ctx, x, y, z, rad, id, group, 3, 1.4f, n_points, offs, partner, buried, only, 2, self_free, gfree, gsasa) != RSASA_OK) return 67;
        if (offs[0] != 0 || offs[1] != 1 || offs[2] != 2 || offs[3] != 2) return 68;
        if (partner[0] != 1 || self_free[0] != 5000 || buried[0] != only[0] || buried[0] != self_free[0] - gfree[0]) return 69;
        if (partner[1] != 0 || self_free[1] != 5000 || buried[1] != only[1] || buried[1] != cov[1]) return 70;
        if (gfree[0] != free_pts[0] || gfree[2] != 5000 || self_free[2] != 5000) return 71;
        if (gsasa[0] != out[0] || gsasa[1] != out[1] || gsasa[2] != out[2]) return 72;
        partner[0] = buried[0] = only[0] = 7u;
        if (rsasa_group_contacts_batch(ctx, x, y, z, rad, id, group, so, 1, 1.4f, n_points, offs, partner, buried, only, 1, self_free, gfree, NULL) != RSASA_ERR_BUFFER_TOO_SMALL) return 73;
        if (partner[0] != 7u || buried[0] != 7u || offs[3] != 2) return 74;
        if (rsasa_group_contacts_batch(ctx, x, y, z, rad, id, group, so, 1, 1.4f, n_points, offs, partner, buried, only, 2, self_free, gfree, NULL) != RSASA_OK) return 75;
        if (partner[0] != 1 || partner[1] != 0 || buried[0] != cov[0] || only[1] != cov[1] || gfree[1] != free_pts[1]) return 76;
        /* all one label: no rows at all */
        group[1] = 0u;
        if (rsasa_group_contacts(ctx, x, y, z, rad, id, group, 3, 1.4f, n_points, offs, partner, buried, only, 2, self_free, gfree, NULL) != RSASA_OK) return 77;
        if (offs[3] != 0 || self_free[0] != gfree[0] || gfree[0] != free_pts[0]) return 78;
    }
    /* empty input is valid and touches nothing */
    if (rsasa_calculate_sasa_internal(ctx, NULL, 0, 1.4f, 100, 1, NULL) != RSASA_OK) return 20;
    /* invalid arguments are reported, not crashed on */
    if (rsasa_calculate_sasa_internal(ctx, atoms, 3, 1.4f, 0, 1, out) != RSASA_ERR_INVALID_ARGUMENT) return 21;
    if (rsasa_context_destroy(ctx) != RSASA_OK) return 22;
    printf("abi ok: %.3f %.3f %.3f\n", out[0], out[1], out[2]);
    return 0;
}
