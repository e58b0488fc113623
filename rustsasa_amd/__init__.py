"""MI355X-native Shrake-Rupley SASA engine behind RustSASA's hot-path API.

The compute lives in rustsasa_amd/lib/librustsasa_amd.so (HIP, gfx950 only,
built from rustsasa_amd/csrc).  Importing this package does not load the
library; the first call does, and raises if it is missing or no GPU is usable.
"""
from .engine import (ATOM_DTYPE, CROWD_MAX_BINS, CROWD_PARTNER, CURV_COLUMNS, CURV_D2, CURV_H, CURV_XX, CURV_XY,
                     CURV_XZ, CURV_YY, CURV_YZ, CURV_ZZ, ENCLOSE_MAX_DIRS, ENCLOSE_PARTNER, FIELD_INV_1PD, FIELD_INV_D,
                     FIELD_INV_D2, FIELD_MAX_CHANNELS, FIELD_PARTNER, FIELD_STEP, HSE_CENTRE,
                     HSE_PARTNER, NEAREST_MAX_K, NEIGHBOR_DTYPE, RADIAL_CENTRE, RADIAL_MAX_BINS, RADIAL_MAX_CLASSES,
                     RADIAL_PARTNER, WITHIN_CENTRE, WITHIN_DTYPE, WITHIN_PARTNER, Context, RsasaError, closest_pairs,
                     component_table, contact_areas, curvature_values, default_link, device_count, dot_means, dot_seeds,
                     dot_seeds_from, dot_structure_offsets, edge_index,
                     enclosure_fraction, escape_vectors, field_values, group_areas, make_atoms, nearest_table, owner_areas,
                     patch_index, patch_table, pseudo_cb_directions, radial_density, residue_depth, sas_volume, sphere_points, split_sasa,
                     surface_points, unpack_points)

__all__ = ["ATOM_DTYPE", "CROWD_MAX_BINS", "CROWD_PARTNER", "CURV_COLUMNS", "CURV_D2", "CURV_H", "CURV_XX", "CURV_XY",
           "CURV_XZ", "CURV_YY", "CURV_YZ", "CURV_ZZ", "ENCLOSE_MAX_DIRS", "ENCLOSE_PARTNER", "FIELD_INV_1PD", "FIELD_INV_D",
           "FIELD_INV_D2", "FIELD_MAX_CHANNELS", "FIELD_PARTNER", "FIELD_STEP", "HSE_CENTRE",
           "HSE_PARTNER", "NEAREST_MAX_K", "NEIGHBOR_DTYPE", "RADIAL_CENTRE", "RADIAL_MAX_BINS", "RADIAL_MAX_CLASSES",
           "RADIAL_PARTNER", "WITHIN_CENTRE", "WITHIN_DTYPE", "WITHIN_PARTNER", "Context", "RsasaError",
           "closest_pairs", "component_table", "contact_areas", "curvature_values", "default_link", "device_count", "dot_means",
           "dot_seeds", "dot_seeds_from", "dot_structure_offsets", "edge_index", "enclosure_fraction", "escape_vectors", "field_values", "group_areas",
           "make_atoms", "nearest_table", "owner_areas", "patch_index", "patch_table", "pseudo_cb_directions", "radial_density", "residue_depth",
           "sas_volume", "sphere_points", "split_sasa", "surface_points", "unpack_points"]
