// Shared host/device plain-data types of the SASA engine (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rsasa {

// Per-structure uniform cell grid, restating SpatialGrid::new
// (reference src/structures/spatial_grid.rs:28-50).  64 bytes.
struct StructGrid {
    float min_x, min_y, min_z;     // bounding-box minimum minus cell_size (spatial_grid.rs:124-127)
    float inv_cell;                // 1.0 / cell_size                      (spatial_grid.rs:36)
    uint32_t dim_x, dim_y, dim_z;  // ceil(extent * inv_cell) + 1          (spatial_grid.rs:39-43)
    uint32_t cell_base;            // first cell of this structure in the batch-wide cell array: index of a 16-bit
                                   // entry when in_lds (multiple of 8), of a 32-bit entry otherwise
    float max_r;                   // fold(0.0, max) of the radii           (lib.rs:259-262)
    float cell_size;               // probe + max_r                        (lib.rs:76)
    uint32_t n_cells;
    uint32_t atom_begin;           // first atom of the structure in input order
    uint32_t n_atoms;
    uint32_t sorted_base;          // first position of the structure in the cell-sorted arrays
    uint32_t in_lds;               // 1: binned by k_sort_window (fewer than 65536 atoms; 16-bit cell starts relative
                                   // to sorted_base), 0: by the batch-wide kernels (32-bit absolute cell starts)
    uint32_t odd_radii;            // bit 0: some radius of the structure lies outside [0, 64] or is NaN, or some coordinate is
                                   // NaN, infinite or beyond 1e8 (the matrix-core occlusion kernel leaves such structures
                                   // to the general kernel: its padding records must be finite vectors);
                                   // bit 1 (BatchView::ids_check): the structure keeps its ids - two of them are equal, or nobody
                                   // could check (k_bounds, k_ids_distinct); bit 2: its ids are in no order (k_bounds);
                                   // bits 8..9: log2 of the x-cell block its atom groups share (grid_group_shift)
};
static_assert(sizeof(StructGrid) == 64, "StructGrid layout");

// Order-preserving integer images of the running min/max, combined with
// integer atomics by the bounds kernel.
struct StructAcc {
    int min_x, min_y, min_z;
    int max_x, max_y, max_z;
    int max_r;
    uint32_t n_atoms;      // atoms of the structure (sum over its bounds workgroups)
    uint32_t first_atom;   // smallest atom index of the structure
    int odd_radii;         // bit 0: a radius outside [0, 64] or NaN, a coordinate non-finite or beyond 1e8; bits 1, 2: the ids' verdict
                           // (see StructGrid::odd_radii)
};

// A contiguous slice of one structure handled by one bounds workgroup.
struct Segment {
    uint32_t sid;
    uint32_t begin;
    uint32_t end;
    uint32_t continues;  // 1: atom begin - 1 belongs to the same structure (k_bounds' id check looks across the seam)
};

// Deferred status of a batch, written on device, copied to pinned host memory.
// k_occlusion_mx's waves claim blocks of atoms from one counter per XCD piece of the launch's range; every counter has
// a 128-byte line to itself (all of them in one line made every claim of the GPU queue up behind one address), and
// the launch over the tail structures has its own set.
constexpr uint32_t kClaimStride = 32;                       // uint32 entries between two counters
constexpr uint32_t kClaimBytes = 2u * 8u * kClaimStride * 4u;

struct BatchStatus {
    uint32_t overflow;        // total cells exceed the workspace capacity: re-run after growing
    uint32_t grid_too_large;  // some structure needs more than 2^31 cells
    uint32_t bad_input;       // probe + max_r <= 0 or non-finite bounds
    uint32_t deferred;        // atoms k_occlusion_fast left to the general kernel (BatchView::deferred_list)
    uint64_t total_cells;     // 32-bit entries of the batch-wide cell array in use (the 16-bit cell starts of the
                              // LDS-binned structures first, two per entry, then the tail's)
    uint64_t tail_cell_begin; // first entry of the structures binned by the batch-wide kernels (multiple of 1024)
    uint32_t tail_atom_base;  // their first position in the cell-sorted arrays (= atoms of the LDS-binned structures)
    uint32_t n_windows;       // entries of BatchView::windows (work list of k_sort_window)
    uint64_t grid_cells;      // cells of all grids (statistic)
    uint32_t ids_needed;      // BatchView::ids_check: the structures that keep their ids (StructGrid::odd_radii bit 1).  0 = the ids of
                              // every structure are all different, so "another atom with my id" never happens - the batch
                              // runs as one without ids; otherwise each structure runs in the instantiation that is its own
    uint32_t ids_unordered;   // bit 0, the same: some id does not rise above its predecessor's (k_bounds); k_ids_distinct then looks
                              // for equal ids structure by structure.  Bit 1: the one occlusion launch of the batch was the id-less
                              // instantiation and the ids turned out to matter (OcclusionChain::solo): nothing was computed
};
static_assert(sizeof(BatchStatus) == 56, "BatchStatus layout");

struct Lattice {
    const float *x, *y, *z;  // device SoA, padded with zeros to a multiple of 64 entries
    const float4 *xyz4;      // the same points as (x, y, z, 0) records
    const uint4 *patches;    // point counts above 128: one entry per aligned run of 16 points, f16 (cz, cy | cx, -1 | eps, 0 | 0, 0)
    const float *mx_tab;     // at most 128 points: the matrix-core kernel's operand tables (mx_tab_floats(): context.cpp get_lattice);
                             // single-wave workgroups read them from here (L1 / L2 hits), not from a per-workgroup LDS copy
    uint32_t n_patches;      // (see context.cpp bisect_points, occlusion_mx.inc); else null / 0
    uint32_t n_points;
    uint32_t n_fused;        // points [0, n_fused) use the fused-FMA `<` rule (lib.rs:143-146);
                             // the rest the scalar remainder rule (lib.rs:185-186,206-207)
};

// Lattice::mx_tab (point counts up to 128): NT = 6, 7 or 8 tiles of 16 points cover them (the kernel's template
// argument); NPS = 16 NT + 16.  Floats [0, 4 NPS): the points component major, (z | y | x | -1) x NPS, entries
// behind the last point zero (among them the 16 behind the tiles: a column that nothing occludes); then 16 NT
// entries of 8 bytes: the same points as f16 (z, y | x, -1), rounded to nearest, zero behind the last point.
inline uint32_t mx_tab_tiles(uint32_t n_points) { return n_points <= 96u ? 6u : n_points <= 112u ? 7u : 8u; }
inline uint32_t mx_tab_floats(uint32_t n_points) { return n_points > 128u ? 0u : 4u * (16u * mx_tab_tiles(n_points) + 16u) + 2u * 16u * mx_tab_tiles(n_points); }

// Running sums of the grid placement scan: (cells, atoms) of the LDS-binned / tail structures.
struct GridSums {
    unsigned long long cells_s, cells_l, atoms_s, atoms_l;
};

// Everything a batch run needs on the device.  All pointers are device pointers.
struct BatchView {
    // inputs
    const float *x, *y, *z, *radius;
    const uint64_t *id;  // may be null
    const uint32_t *id32;  // nullable: the ids already folded to 32 bits (fold_id) by the host, in input order.  When set,
                           // the binning kernels read these instead of `id`, no sorted copy of the 64-bit ids is kept, and
                           // `id` (device-accessible, possibly mapped host memory) is only read by the general occlusion
                           // kernel for the few atoms whose folds collide
    const uint8_t *radius8;  // nullable (pipelined host path): the radii as one-byte codes into `radius_table`, read instead of
    const float *radius_table;  // `radius` (a batch has few distinct radii: 1 byte per atom crosses the link, not 4)
    const uint32_t *residue_offsets;
    uint32_t n_atoms, n_structures, n_residues, n_segments;
    float probe;
    // Ids only matter where two atoms of a structure share one (lib.rs:127: a neighbour with the atom's own id is
    // skipped).  1: k_bounds also checks that the ids of every structure increase strictly (what atom serials and indices
    // do); where they do not (hashes), k_ids_distinct puts that structure's ids (or the host's 32-bit folds of them) through
    // a hash table in LDS.  The verdict is each STRUCTURE's (StructGrid::odd_radii bit 1): one whose ids are all different
    // is computed as one WITHOUT ids - no id loads, no sorted copies, the occlusion kernel's id-less instantiation (4 %
    // faster) - with identical results; BatchStatus::ids_needed counts the others.  Set for batches with ids that the
    // matrix-core kernel takes.
    uint32_t ids_check;
    const uint32_t *large_sids;    // k_ids_distinct: the structures of more than kIdAtomsSmall (and at most kIdAtomsLarge) atoms
    uint32_t n_large;
    uint32_t ids_tables;           // the k_ids_distinct launches are part of this batch (the context's last checked batch had
                                   // ids in no order); 0: they are not - their workgroups wait for LDS even to return -, and
                                   // ids that do not rise simply stay in play for this batch
    // workspace
    const Segment *segments;
    StructAcc *acc;
    StructGrid *grids;
    uint32_t *sid_sorted;         // structure of the atom at cell-sorted position p
    uint32_t *cell_of, *rank_of;  // binning only.  Batch-wide route: cell index / arrival rank inside the cell;
                                  // k_sort_window: rank_of = sorted position of the atoms a workgroup's registers do not hold
    uint32_t *deferred_list;      // atoms k_occlusion_fast left to the general kernel (BatchStatus::deferred entries)
    uint32_t *claim;              // k_occlusion_mx: block counters of its persistent waves, kClaimBytes (launch_occlusion zeroes them)
    uint32_t *ids_seg;            // BatchView::ids_check: two bitmaps of ids_seg_words words, a bit per 64 cell-sorted atoms - "an atom of a
    uint32_t ids_seg_words;       // structure that keeps its ids is among them" and "... of one that does not" (k_ids_segments): a workgroup of
                                  // k_occlusion_mx whose atoms hold nothing of its instantiation's returns before it has fetched anything else
    uint32_t *cells;              // cell starts (cell_capacity + 1 entries of 32 bits; see StructGrid::cell_base)
    uint64_t cell_capacity;
    uint4 *windows;               // (structure, window, first atom, atoms) of every k_sort_window workgroup
    uint32_t window_capacity;     // entries of `windows` = workgroups launched (the surplus exits)
    uint32_t *scan_block_sums;
    GridSums *grid_sums;   // per 256 structures: (cells, atoms) x (LDS-binned, tail), 4 x u64
    float4 *sorted_xyzr;          // cell-sorted (x, y, z, radius)
    uint32_t *sorted_orig;        // cell-sorted position -> input index
    uint64_t *sorted_id;          // cell-sorted ids (only when id != null; null too when the matrix-core kernel takes
                                  // the batch: it works on the folds, and the general kernel fetches the few ids it
                                  // needs through sorted_orig)
    uint32_t *sorted_id32;        // the same folded to 32 bits (fold_id): different folds => different ids
    BatchStatus *status;
    // outputs
    float *atom_sasa;             // never null (workspace buffer when the caller passed none)
    float *residue_sasa;          // may be null
    uint32_t *neighbor_counts;    // may be null
    // Nullable, pinned host memory (the one-structure call): k_occlusion_fast sets it to 1 when it leaves an
    // atom to the general kernel, and launch_occlusion then does NOT launch that kernel - the caller looks at
    // the flag after the stream has drained and calls launch_occlusion_deferred if it is set (it rarely is).
    uint32_t *defer_flag;
    // rsasa_precompute_neighbors*: the max_radius the caller gave (precompute_neighbors takes it as given, reference
    // src/lib.rs:69-84): make_grid builds every structure's grid and search radii from it instead of StructAcc::max_r.
    // NaN (the default): no override - the SASA path never sets it.
    float max_r_override = __builtin_nanf("");
};

// ---- neighbour lists (neighbors.hip, rsasa_precompute_neighbors*) ----
// What the host reads back after the count and scan kernels, and the cursors of the fill kernel.
struct NbInfo {
    unsigned long long total;          // entries of all lists (offsets[n])
    unsigned long long max_k;          // the longest list
    unsigned long long spill_entries;  // entries of the lists longer than the fill kernel's LDS staging
    unsigned long long spill_atoms;    // number of such lists
    unsigned long long spill_cursor;   // k_neighbor_fill: entries of NbArgs::spill handed out
    unsigned long long spill_recs;     // k_neighbor_fill: records of NbArgs::spill_recs written
    unsigned long long mismatch;       // nonzero: the fill pass accepted a different number of candidates than the count pass
    unsigned long long pad;
};
static_assert(sizeof(NbInfo) == 64, "NbInfo layout");
struct NbKey {                 // a staged candidate of a long list: (float bits of d^2) << 32 | idx, and its threshold
    unsigned long long key;
    float thr;
    uint32_t pad;
};
struct NbSpillRec {            // a long list: its entries at out[off ..), its keys at spill[base ..), k of them
    unsigned long long off, base;
    uint32_t k, pad;
};
struct NbArgs {
    BatchView b;
    uint32_t *counts;                // [n_atoms] list length of input atom i
    unsigned long long *offsets;     // [n_atoms + 1] exclusive scan of counts
    unsigned long long *parts;       // scan: 4 entries per workgroup of the scan
    NbInfo *info;
    const uint32_t *idx_map;         // nullable: input atom -> the index written to the entries (active_indices);
                                     // null: the index within the structure
    uint2 *out;                      // (threshold_squared bits, idx) = rsasa_neighbor_t
    NbKey *spill;
    NbSpillRec *spill_recs;
    uint32_t stage;                  // the keys the run's fill kernel stages per list: the scan counts the longer lists into
                                     // NbInfo::spill_entries / spill_atoms (neighbor_stage_capacity, within_stage_capacity)
};

// ---- accessible points (points.hip, rsasa_accessible_points*) ----
// The lists of a finished neighbour run (NbArgs: offsets, out) tested against the lattice, bits out.
struct PtArgs {
    BatchView b;                        // the binned batch of the neighbour run (input columns, grids, sorted order)
    const unsigned long long *offsets;  // [n_atoms + 1] NbArgs::offsets
    const uint2 *entries;               // NbArgs::out: (threshold_squared bits, idx within the structure)
    const float *lx, *ly, *lz;          // the lattice in the reference's order (lib.rs:43-66), zero padded to whole 64s
    uint32_t n_points, n_fused, words;  // words = (n_points + 31) / 32 per atom
    uint32_t *masks;                    // [n_atoms][words], input order: bit p & 31 of word p >> 5 = point p exposed
    float *sasa;                        // [n_atoms] or null: ((4 pi R^2) popcount) / n_points (lib.rs:220-222)
};

// ---- exposure vectors (points.hip, rsasa_exposure_vectors*) ----
// The same lists and lattice (p.masks and p.words unused): per atom the sum of its exposed lattice points and their number.
struct ExArgs {
    PtArgs p;                           // p.sasa: [n_atoms] or null, ((4 pi R^2) k) / n_points with k = free
    float *vectors;                     // [n_atoms][3], input order: the float32 sum of the exposed points of the unit lattice,
                                        // a tree over the 64 lanes of a chunk, then the chunks ascending (k_exposure_vectors)
    uint32_t *free;                     // [n_atoms] the exposed points: the popcount of PtArgs::masks
};

// ---- atom depth (depth.hip, rsasa_atom_depth*) ----
// A finished point run (p.masks written, in input order) and the grid it ran on: per atom the smallest key over the
// accessible dots of its structure.
struct DpArgs {
    PtArgs p;                           // p.masks, p.words: the masks k_accessible_points wrote; p.sasa as there
    uint32_t *free;                     // [n_atoms] the exposed points: the popcount of the atom's mask (k_mask_free)
    unsigned long long *keys;           // [n_atoms], input order: min of (float bits of d2) << 32 | index within the structure of
                                        // the dot's owner, over the accessible dots of the atom's structure whose d2 is no NaN
                                        // (the definition: include/rustsasa_amd.h); all ones where there is none
};

// ---- surface components (components.hip, rsasa_surface_components*) ----
// A finished point run (p.masks written, in input order) and the grid it ran on: the accessible dots numbered through the
// batch in (atom, point) order and, per dot, the smallest dot of its connected component.
struct CcArgs {
    PtArgs p;                           // p.masks, p.words: the masks k_accessible_points wrote; p.sasa as there
    uint32_t *free;                     // [n_atoms] the exposed points: the popcount of the atom's mask (k_mask_free)
    const unsigned long long *dot_offsets;  // [n_atoms + 1] exclusive scan of free: atom i's dots are [dot_offsets[i], dot_offsets[i + 1])
    unsigned long long n_dots;          // dot_offsets[n_atoms], below 2^32
    uint32_t *parent;                   // [n_dots] the union-find forest: parent <= self, a root is the smallest dot of its tree
    uint32_t *labels;                   // [n_dots] the root of the dot's tree minus the first dot of its structure
    float link, link2;                  // two dots are linked when d2 <= link2 = link * link (one float32 product)
};

// ---- dot links and dot geodesics (geodesics.hip, rsasa_dot_links*, rsasa_dot_geodesics*) ----
// The dots and the edge test of CcArgs (c.parent and c.labels unused): per dot the list of the dots linked to it, and the
// shortest float32 path length along those lists from a set of seed dots.
constexpr uint32_t kGdRounds = 8;       // rounds of the relaxation between two looks of the host at the flags
struct GdArgs {
    CcArgs c;                           // c.p.masks, c.free, c.dot_offsets, c.n_dots (here below 2^31), c.link, c.link2
    uint32_t *counts;                   // [n_dots] the length of every dot's list (k_dot_link<kCount>; zeroed by the caller)
    uint32_t *cursor;                   // [n_dots] the entries the fill pass accepted per dot (zeroed by the caller)
    const unsigned long long *link_offsets;  // [n_dots + 1] exclusive scan of counts, batch-global
    uint2 *raw;                         // [link_offsets[n_dots]] the lists in sweep order: (d2 bits, idx within the structure)
                                        // for the links, (bits of sqrtf(d2), batch-wide dot) for the geodesics
    uint2 *out;                         // links only: the lists ascending by (d2 bits << 32) | idx = rsasa_within_t
    NbInfo *info;                       // mismatch: a cursor differs from its count
    const uint8_t *seeds;               // geodesics: [n_dots], nonzero = seed
    float limit;                        // a path longer than this is none (+inf: no limit)
    uint32_t *dist;                     // [n_dots] float32 bits (all >= +0: they order like the numbers); +inf = unreached
    uint32_t *stamp;                    // [n_dots] the last round in which the dot's value fell
    uint32_t *source;                   // [n_dots] or null: the smallest seed (dot number within the structure) on a tight path
    uint32_t *flags;                    // [kGdRounds] nonzero: that round of the current group lowered a value
};

// ---- dot curvature (curvature.hip, rsasa_dot_curvature*) ----
// The dots and the hit test of CcArgs with the reach as its link (c.parent and c.labels unused): per dot the number of
// dots of its structure within the reach and eight fixed-point sums over them.
constexpr uint32_t kCurvColumns = 8;    // RSASA_CURV_D2 .. RSASA_CURV_YZ: the columns of a row of moments
struct CvArgs {
    CcArgs c;                           // c.p.masks, c.free, c.dot_offsets, c.n_dots; c.link = reach, c.link2 = reach * reach
    uint32_t *pairs;                    // [n_dots] the pairs that count per dot (zeroed by the caller)
    unsigned long long *moments;        // [n_dots][kCurvColumns] the wrapping sums, 24 fraction bits (zeroed by the caller)
};

// ---- dot patches (patches.hip, rsasa_dot_patches*) ----
// The lists of the geodesics (g.raw as weights) and their dist, stamp and source: per structure the farthest-point
// sample of its dots along the graph, one workgroup of k_patch_sample per structure.
constexpr uint32_t kPsBlock = 256;      // lanes of a k_patch_sample workgroup
constexpr uint32_t kPsQueue = 1024;     // dots a frontier queue in LDS holds; a longer frontier falls back to the stamp scan
struct PsStats {                        // what k_patch_sample adds up over the structures of a call
    unsigned long long picks, steps, overflows;
    unsigned long long error;           // nonzero: a structure left one of its bounded loops (a logic error)
};
struct PsArgs {
    GdArgs g;                           // g.c (dots), g.link_offsets, g.raw, g.cursor, g.info, g.dist, g.stamp, g.source (nullable)
    const uint32_t *so;                 // [n_structures + 1] the structures' offsets in input order
    uint32_t n_structures;
    float spacing;                      // sampling stops when the farthest dot is finite and <= spacing (+inf: one centre a component)
    uint32_t max_centres;               // >= 1
    const unsigned long long *slot_offsets;  // [n_structures + 1] exclusive scan of min(max_centres, D_s): a structure's room
    uint32_t *centres;                  // [slot_offsets[n_structures]] the centres in pick order, dot numbers within the structure
    uint32_t *cover;                    // the same room: float32 bits of the farthest distance before each pick
    uint32_t *n_centres;                // [n_structures] the picks of each structure
    PsStats *stats;                     // zeroed by the caller
    // k_patch_pack, once the host has scanned n_centres: the centres and covers without the unused room between structures
    const unsigned long long *centre_offsets;  // [n_structures + 1] exclusive scan of n_centres
    uint32_t *packed_centres, *packed_cover;    // [centre_offsets[n_structures]]
};

// ---- dot crowding (crowding.hip, rsasa_dot_crowding*) ----
// A finished point run (p.masks written, in input order), the grid it ran on and a flag byte per atom: the accessible
// dots numbered as CcArgs numbers them and, per dot, the partner atoms of its structure by distance bin.
struct DcArgs {
    PtArgs p;                           // p.masks, p.words: the masks k_accessible_points wrote; p.sasa as there
    uint32_t *free;                     // [n_atoms] the exposed points: the popcount of the atom's mask (k_mask_free)
    const unsigned long long *dot_offsets;  // [n_atoms + 1] exclusive scan of free: atom i's rows are [dot_offsets[i], dot_offsets[i + 1])
    const uint8_t *sorted_flags;        // [n_atoms] HsArgs::sorted_flags (k_sort_flags): bit 0 - the atom is a partner
    uint32_t n_bins;                    // 1 .. kCrowdMaxBins (entry_checks.h)
    float e2[8];                        // the squared edges, edges[k] * edges[k] (one float32 product), non-decreasing;
                                        // [n_bins .. 8) repeat the last one
    uint32_t *counts;                   // [dot_offsets[n_atoms]][n_bins]: every row is written
};

// ---- dot fields (fields.hip, rsasa_dot_fields*) ----
// What DcArgs describes, with a row of weights per atom: per dot and channel the fixed-point sum of weight times a
// distance kernel over the partner atoms of its structure within the cutoff.
constexpr uint32_t kFieldChannels = 4;  // the channels of a call at most: a dot's accumulators are registers of k_dot_fields
struct FdArgs {
    PtArgs p;                           // p.masks, p.words: the masks k_accessible_points wrote; p.sasa as there
    uint32_t *free;                     // [n_atoms] the exposed points: the popcount of the atom's mask (k_mask_free)
    const unsigned long long *dot_offsets;  // [n_atoms + 1] exclusive scan of free: atom i's rows are [dot_offsets[i], dot_offsets[i + 1])
    const uint8_t *sorted_flags;        // [n_atoms] HsArgs::sorted_flags (k_sort_flags): bit 0 - the atom is a partner
    const float *weights;               // [n_atoms][n_channels], input order (read through sorted_orig)
    uint32_t n_channels;                // 1 .. kFieldChannels
    uint32_t kinds[kFieldChannels];     // the channels' kinds (RSASA_FIELD_*); [n_channels .. 4) are 0
    uint32_t need;                      // bit k: some channel has kind k
    float c2;                           // cutoff * cutoff (one float32 product; may overflow to +inf, underflow to 0)
    long long *sums;                    // [dot_offsets[n_atoms]][n_channels]: every row is written
};

// ---- dot enclosure (enclosure.hip, rsasa_dot_enclosure*) ----
// A finished point run (p.masks written, in input order), the grid it ran on and a flag byte per atom: the accessible
// dots numbered as CcArgs numbers them and, per dot, the directions of a fixed fan in which the probe is stopped.
constexpr uint32_t kEncloseDirs = 32;   // the directions of the fan at most: a bit each of a dot's word
struct DeDir {                          // direction m of the fan, as the kernel reads it (32 bytes, one scalar load)
    float ux, uy, uz, pad0;             // u_m of generate_sphere_points(n_dirs)
    float lx, ly, lz, pad1;             // reach * u_m, per component (one float32 product each): the ray's far end
};
struct DeArgs {
    PtArgs p;                           // p.masks, p.words: the masks k_accessible_points wrote; p.sasa as there
    uint32_t *free;                     // [n_atoms] the exposed points: the popcount of the atom's mask (k_mask_free)
    const unsigned long long *dot_offsets;  // [n_atoms + 1] exclusive scan of free: atom i's dots are [dot_offsets[i], dot_offsets[i + 1])
    const uint8_t *sorted_flags;        // [n_atoms] HsArgs::sorted_flags (k_sort_flags): bit 0 - the atom is an obstacle
    uint32_t n_dirs;                    // 1 .. kEncloseDirs
    float reach, reach2;                // L and L * L (one float32 product; may overflow to +inf, underflow to 0)
    DeDir dir[kEncloseDirs];            // [n_dirs .. 32) are zero and never read
    uint32_t *blocked;                  // [dot_offsets[n_atoms]]: every word is written
};

// ---- half-sphere exposure (hse.hip, rsasa_half_sphere_exposure*) ----
// A binned batch (no neighbour lists) with a direction and a flag byte per atom: per centre the partners of its own
// structure within the cutoff, split by the side of the plane through the centre that is normal to its direction.
struct HsArgs {
    BatchView b;                        // the binned batch: grids, cell starts, sorted order
    const float *dirs;                  // [n_atoms][3], input order, or null: every partner counts as `up`
    const uint8_t *flags;               // [n_atoms], input order, or null: every atom is centre and partner
    uint8_t *sorted_flags;              // [n_atoms] the flags in cell-sorted order (k_sort_flags; all 3 where flags is null)
    float cutoff;                       // a partner counts when d2 <= cutoff * cutoff (one float32 product)
    uint32_t *up, *down;                // [n_atoms], input order (the definition: include/rustsasa_amd.h)
};

// ---- atoms within a cutoff (within.hip, rsasa_atoms_within*) ----
// A binned batch (no neighbour lists) with a flag byte per atom in cell-sorted order: per centre the list of the partners
// of its own structure within the cutoff, as entries (float bits of d2, idx) sorted by (d2, idx).
struct WnArgs {
    NbArgs n;                           // the binned batch; counts, offsets, parts, info as in a neighbour run (idx_map null);
                                        // out: the entries (d2 bits, idx within the structure) = rsasa_within_t; spill (thr =
                                        // d2) and spill_recs for the lists longer than the staging, as k_neighbor_fill uses them
    const uint8_t *sorted_flags;        // [n_atoms] HsArgs::sorted_flags (k_sort_flags)
    float cutoff;                       // a partner is listed when d2 <= cutoff * cutoff (one float32 product)
    uint32_t upper_only;                // nonzero: only partners with a larger index than the centre's
};

// ---- the k nearest atoms (nearest.hip, rsasa_nearest_atoms*) ----
// The same batch, flags and rule (w.upper_only 0; w.cutoff may be +inf): per centre the first k entries of the list
// WnArgs defines.  k_nearest writes them to a row of stride k and the row's length to w.n.counts; the neighbour runs'
// scan and k_nearest_gather then make w.n.offsets and w.n.out (no spill: w.n.stage = k).
struct NnArgs {
    WnArgs w;
    uint32_t k;                         // 1 .. kNearestMaxK (entry_checks.h)
    const uint32_t *rank;               // [n_atoms], input order, or null: the row of a centre - the number of centres
                                        // before it (a host prefix over the flag bytes); null: the row is the atom
    unsigned long long *rows;           // [rows][k] the keys (d2 bits) << 32 | idx of each centre, ascending
};

// ---- radial counts (radial.hip, rsasa_radial_counts*) ----
// A binned batch (no neighbour lists) with a flag byte and a class byte per atom and a list of distance bins: per centre
// the partners of its own structure by (class, bin), and per structure the sums of those rows by the centre's class.
struct RdArgs {
    BatchView b;                        // the binned batch: grids, cell starts, sorted order
    const uint8_t *flags;               // [n_atoms], input order, or null: every atom is centre and partner
    const uint8_t *classes;             // [n_atoms], input order, or null: every atom is class 0; every byte < n_classes
    uint8_t *sorted_kinds;              // [n_atoms] (class << 2) | (flags & 3) in cell-sorted order (k_sort_kinds)
    const uint32_t *so;                 // [n_structures + 1] the structures' offsets in input order (k_radial_pairs)
    uint32_t n_classes, n_bins;         // 1 .. kRadialMaxClasses, 1 .. kRadialMaxBins (entry_checks.h)
    float e2[32];                       // [n_bins] the squared edges, edges[k] * edges[k] (one float32 product), non-decreasing
    uint32_t *table;                    // [n_atoms][n_classes][n_bins], input order: every row is written
    unsigned long long *pairs;          // [n_structures][n_classes][n_classes][n_bins] or null; zeroed by the caller
};

// ---- contact counts (points.hip, rsasa_contact_points*) ----
// The same lists and lattice (p.masks unused), per-entry counts out, aligned with NbArgs::out.
struct CtArgs {
    PtArgs p;                           // p.sasa: [n_atoms] or null, ((4 pi R^2) k) / n_points with k the points no entry hits
    uint32_t *covered;                  // [offsets[n_atoms]]: points of the atom the entry hits
    uint32_t *exclusive;                // [offsets[n_atoms]]: points of the atom the entry hits and no other entry of the list does
};

// ---- contact owners (points.hip, rsasa_contact_owners*) ----
// The same lists and lattice (p.masks unused): every point some entry hits goes to ONE entry, the hitting entry with the
// smallest margin dot - limit (the earlier position on a tie).
struct CoArgs {
    PtArgs p;                           // p.sasa: [n_atoms] or null, as CtArgs
    uint32_t *owned;                    // [offsets[n_atoms]]: points of the atom the entry owns
    uint32_t *owner;                    // [n_atoms][n_points] or null, input order: the owner's position in the atom's
                                        // list, 0xFFFFFFFF for a point no entry hits
};

// ---- group contacts (points.hip, rsasa_group_contacts*) ----
// The same lists and lattice (p.masks unused) and a label per atom: k_group_order reorders every list by label and counts
// its rows (one per distinct foreign label), the host scans the counts into row_offsets, k_group_points fills the rows.
struct GpArgs {
    PtArgs p;                           // p.sasa: [n_atoms] or null, as CtArgs
    const uint32_t *group;              // [n_atoms] the labels, input order
    uint2 *sorted;                      // [offsets[n_atoms]] every list again: its own-group entries first, then the others
                                        // by (label, position in the list)
    uint32_t *sorted_group;             // [offsets[n_atoms]] the labels of those entries
    uint32_t *n_own;                    // [n_atoms] own-group entries of the list
    uint32_t *n_rows;                   // [n_atoms] distinct foreign labels of the list
    const unsigned long long *row_offsets;  // [n_atoms + 1] exclusive scan of n_rows
    uint32_t *groups, *buried, *only;   // [row_offsets[n_atoms]] a row's label, and the points of the atom its own group leaves
                                        // free that the label hits / that it alone among the foreign labels hits
    uint32_t *self_free, *free;         // [n_atoms] points no own-group entry hits / no entry hits
};

// Grid and status of a one-structure batch, computed by the host and handed to k_sort_window<true> as
// kernel arguments.
struct SingleJob {
    StructGrid grid;
    BatchStatus status;
};

// Occlusion kernel selection (RSASA_OCCLUSION_KERNEL / RSASA_ATOMS_PER_WAVE, read once per
// context; for A/B measurements -- every version computes identical results).
struct OcclusionTuning {
    int kernel_version = 6;       // 0 = all-pairs reference kernel, 3 = general culled-sweep kernel for every atom,
                                  // 4 = straight-line per-atom kernel, 5 = group-union sweep + matrix-core point
                                  // tests (4 and 5 leave the atoms they cannot take to the general kernel),
                                  // 6 = 5 for batches of 32 768 atoms or more, 4 below
    uint32_t atoms_per_wave = 0;  // 0 = choose from the batch size
    uint32_t deferred_hint = 0xFFFFFFFFu;  // atoms the context's last completed batch left to the general kernel (unknown at
                                           // first): sizes the launch that works off the next batch's deferred list - a grid-stride
                                           // loop, so any size is correct; 1 024 workgroups that find an empty list cost 20 us
};

// Launchers implemented in kernels.hip / occlusion.hip.  Each only enqueues on `stream`.
void launch_grid_prepare(const BatchView &b, hipStream_t stream);
void launch_sort_lds(const BatchView &b, hipStream_t stream);
void launch_sort_single(const BatchView &b, const SingleJob &job, hipStream_t stream);
void launch_sort_tail(const BatchView &b, hipStream_t stream);
// Which atoms (cell-sorted positions) an occlusion launch covers: the tail's binning may still be
// running on another stream while the LDS-binned structures are processed.
enum OcclusionPart : uint32_t {
    kOccAll = 0,   // every atom (both binning routes are complete)
    kOccHead = 1,  // positions below BatchStatus::tail_atom_base (LDS-binned structures); may launch nothing
    kOccRest = 2,  // whatever kOccHead did not launch, plus the deferred atoms
};
// Two batches in flight: a batch's occlusion kernel starts when the other batch's has ended, and "has ended" is an event
// recorded right behind THAT kernel - not behind the launches that follow it (the instantiation the id check does not ask
// for, which returns at once, and the general kernel over the deferred list: 25 us that the next occlusion kernel then
// does not wait for).  launch_occlusion waits for `wait` in front of the launch that does the work, records `start` (timing,
// nullable) there and `done` behind it.  With BatchView::ids_check the host does not know which instantiation will work:
// `expect_ids_dropped` (what the context's last batch did) puts the other one FIRST, in front of the wait, where it runs
// beside the neighbour's kernel for nothing; a wrong guess only loses the ordering for that batch.
// `solo` (callers that can run a batch again: rsasa_batch_wait): when the ids are expected to be dropped only the id-less
// instantiation is launched; should the device find that the ids do matter, that launch does nothing but raise bit 1 of
// BatchStatus::ids_unordered, and the caller runs the batch again with its ids (once, at a change of the id pattern -
// against an empty launch of 45 000 workgroups in front of every batch's working kernel: 15 us of every step).
struct OcclusionChain {
    hipEvent_t wait = nullptr, start = nullptr, done = nullptr;
    bool expect_ids_dropped = true;
    bool solo = false;
};
void launch_occlusion(const BatchView &b, const Lattice &lat, const OcclusionTuning &tune,
                      OcclusionPart part, hipStream_t stream, const OcclusionChain *chain = nullptr);
// Whether launch_occlusion gives a batch of n_atoms atoms to the matrix-core kernel.
bool occlusion_uses_mx(const OcclusionTuning &tune, const Lattice &lat, uint32_t n_atoms);
// The general kernel over the atoms the straight-line kernel deferred (see BatchView::defer_flag).
void launch_occlusion_deferred(const BatchView &b, const Lattice &lat, hipStream_t stream);
void launch_residue_sums(const BatchView &b, hipStream_t stream);
// Neighbour lists (neighbors.hip) on a binned batch: counts, offsets and NbInfo; then the entries.
void launch_neighbor_count(const NbArgs &a, hipStream_t stream);
void launch_neighbor_fill(const NbArgs &a, uint64_t spill_atoms, hipStream_t stream);
// The point masks (points.hip) from those lists.
void launch_accessible_points(const PtArgs &a, hipStream_t stream);
// The exposed-point sums and counts (points.hip) from those lists.
void launch_exposure_vectors(const ExArgs &e, hipStream_t stream);
// The exposed-point counts (points.hip) from the masks launch_accessible_points wrote: free[n_atoms], input order.
void launch_mask_free(const PtArgs &a, uint32_t *free, hipStream_t stream);
// The nearest-dot keys (depth.hip) from those masks and counts (DpArgs::free).
void launch_atom_depth(const DpArgs &d, hipStream_t stream);
// The component labels of the dots (components.hip) from those masks and counts, with CcArgs::dot_offsets.
void launch_components(const CcArgs &c, hipStream_t stream);
// The dot graph (geodesics.hip) from those masks and counts, with GdArgs::c.dot_offsets: the lists' lengths; then, with
// link_offsets, the lists themselves (sorted, or as weights for the relaxation); the relaxation's start, its rounds
// (kGdRounds per call, verdicts in GdArgs::flags) and the start of its source phase.
void launch_dot_link_count(const GdArgs &gd, hipStream_t stream);
void launch_dot_link_fill(const GdArgs &gd, bool weights, hipStream_t stream);
void launch_geodesic_init(const GdArgs &gd, hipStream_t stream);
void launch_geodesic_rounds(const GdArgs &gd, bool source, uint32_t first, hipStream_t stream);
void launch_geodesic_restamp(const GdArgs &gd, hipStream_t stream);
// The farthest-point sample (patches.hip) on the weighted lists of the geodesics: dist, stamp and source cleared (and the
// fill's cursors checked), then every structure's picks in one launch.
void launch_patch_sample(const PsArgs &ps, hipStream_t stream);
// The centres and covers of the sample moved together (patches.hip): ps.centre_offsets -> ps.packed_centres, ps.packed_cover.
void launch_patch_pack(const PsArgs &ps, hipStream_t stream);
// The pair counts and moments of the dots (curvature.hip) from those masks and counts; the caller has zeroed both.
void launch_dot_curvature(const CvArgs &cv, hipStream_t stream);
// The rows of the dots (crowding.hip) from those masks and counts, with DcArgs::dot_offsets and ::sorted_flags.
void launch_dot_crowding(const DcArgs &d, hipStream_t stream);
// The fixed-point sums of the dots (fields.hip) from the same, with FdArgs::weights in input order.
void launch_dot_fields(const FdArgs &d, hipStream_t stream);
// The blocked directions of the dots (enclosure.hip) from those masks and counts, with DeArgs::dot_offsets and ::sorted_flags.
void launch_dot_enclosure(const DeArgs &d, hipStream_t stream);
// The half-sphere counts (hse.hip) on a binned batch: the flags in cell-sorted order, then up[] and down[].
void launch_half_sphere(const HsArgs &h, hipStream_t stream);
// The keys k_neighbor_fill / k_within_fill stage per list in LDS: what NbArgs::stage is set to for their runs.
uint32_t neighbor_stage_capacity();
uint32_t within_stage_capacity();
// The flags in cell-sorted order alone (hse.hip): h.b, h.flags -> h.sorted_flags.
void launch_sort_flags(const HsArgs &h, hipStream_t stream);
// The lists of the atoms within a cutoff (within.hip) on a binned batch with sorted flags: counts, offsets and NbInfo
// (with NbArgs::stage = within_stage_capacity()); then the entries.
void launch_within_count(const WnArgs &w, hipStream_t stream);
void launch_within_fill(const WnArgs &w, uint64_t spill_atoms, hipStream_t stream);
// The k nearest atoms (nearest.hip) on a binned batch with sorted flags: the rows, counts, offsets and NbInfo; then the
// entries gathered from the rows (a count above k sets NbInfo::mismatch).
void launch_nearest(const NnArgs &a, hipStream_t stream);
void launch_nearest_gather(const NnArgs &a, hipStream_t stream);
// The radial counts (radial.hip) on a binned batch: the kinds in cell-sorted order, every row of r.table and, with
// r.pairs, the rows' sums added to the pair tables.
void launch_radial(const RdArgs &r, hipStream_t stream);
// The ranking of the long lists by itself (neighbors.hip): a.spill, a.spill_recs -> a.out, one workgroup per list.
void launch_neighbor_rank_spill(const NbArgs &a, uint64_t spill_atoms, hipStream_t stream);
// The per-entry point counts (points.hip) from those lists.
void launch_contact_points(const CtArgs &c, hipStream_t stream);
void launch_contact_owners(const CoArgs &c, hipStream_t stream);
// The 64-bit exclusive scan of the count pass by itself (neighbors.hip): a.counts -> a.offsets[0 .. n_atoms], totals -> a.info.
void launch_neighbor_scan(const NbArgs &a, hipStream_t stream);
// Group contacts (points.hip): the lists in label order and their row counts; then, with GpArgs::row_offsets, the rows.
void launch_group_order(const GpArgs &g, hipStream_t stream);
void launch_group_points(const GpArgs &g, hipStream_t stream);
// Pinned 24-byte atom records (x, y, z, r, id) -> device columns, and `hdr_bytes` of header beside them (combine.cpp).
void launch_unpack_atoms(const void *records, uint32_t n_atoms, float *x, float *y, float *z, float *r, uint64_t *id,
                         const void *hdr_src, void *hdr_dst, uint32_t hdr_bytes, hipStream_t stream);
void launch_expand_frames(const float *xyz, const float *radius, const uint64_t *id,
                          const uint32_t *res_off, uint32_t n_atoms, uint32_t n_frames, uint32_t res_stride,
                          float *x, float *y, float *z, float *r, uint64_t *id_out,
                          uint32_t *res_out, hipStream_t stream);

constexpr uint32_t kSegmentAtoms = 4096;  // atoms per bounds workgroup
constexpr uint32_t kScanBlocks = 1024;    // workgroups of the cell scan
constexpr uint32_t kWindowCells = 36864;  // cells one k_sort_window workgroup bins (16-bit counters, 72 KiB: two per CU)
// k_ids_distinct (BatchView::ids_check): a table of 8 192 slots in LDS for structures of up to 4 096 atoms (32 KB: several
// workgroups per CU), one of 36 864 for up to 27 648 (144 KB, one workgroup per such structure)
// (the large table's entries are 16 bits wide - an atom's number within its structure, below 65 536 -: twice the slots in the
// same 144 KB, which takes structures of up to 55 296 atoms; round 5's 32-bit entries stopped at 27 648, and the reference's own
// quality set holds a complex of 32 500)
constexpr uint32_t kIdSlotsSmall = 8192, kIdAtomsSmall = 4096, kIdSlotsLarge = 73728, kIdAtomsLarge = 55296;
constexpr uint32_t kLdsMaxAtoms = 65536;  // structures with fewer atoms are binned in LDS (16-bit positions)

// 16-bit entries a structure of n_cells cells takes in the cell array: its cells, the end marker,
// padding to whole 16-byte vectors.
// k_occlusion_mx groups atoms of one cell row whose x cells fall in the same aligned block of 2^shift cells; the group
// shares the union of the 25 x-runs around it, (2^shift + 4) cells long, which must hold at most 256 atoms or the group
// is narrowed (and the runs looked up again).  Where atoms fill their grid - 1.5 per cell in a dense medium - a block
// of 8 cells never fits: start from the width that does.  (A heuristic: it changes the kernel's speed, not its results.)
__host__ __device__ inline uint32_t grid_group_shift(uint32_t n_atoms, uint32_t n_cells)
{
    const float per_cell = (float)n_atoms / (float)(n_cells ? n_cells : 1u);
    return per_cell >= 1.0f ? 0u : per_cell >= 0.6f ? 1u : per_cell >= 0.3f ? 2u : 3u;
}
__host__ __device__ constexpr uint32_t lds_cell_slots(uint32_t n_cells) { return (n_cells + 1u + 7u) & ~7u; }
__host__ __device__ constexpr uint32_t grid_windows(uint32_t n_cells) { return (n_cells + kWindowCells - 1u) / kWindowCells; }

}  // namespace rsasa
