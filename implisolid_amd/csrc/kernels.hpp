// kernels.hpp -- launch-side declarations of the MI355X kernels (all on one HIP stream).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdexcept>
#include <string>

#include "grid.hpp"
#include "host.hpp"
#include "mc_types.hpp"
#include "program.hpp"

namespace impli {

GridDesc make_grid(int R, const float box[6], int cz0, int cz1, int cz_emit);

void build_case_table(CaseInfo out[256]);
// the vertex pass's word per case (mc_device.hpp case_word), stored behind the table (mc_types.hpp case_words)
void build_case_words(const CaseInfo cases[256], uint32_t out[256]);

// K1: field at the slab's stored samples
void launch_eval_field(const Program* d_prog, int depth, const float* d_rabbit, const GridDesc& g, float* d_field,
                       hipStream_t s);
// direct evaluation at arbitrary points (implicit values / gradients)
BrickGrid brick_grid(const GridDesc& g);
// K1a: interval pass -- per-brick CSG pruning modes and sign class (coarse boxes, then the bricks
// of mixed coarse boxes)
BrickGrid coarse_grid(const GridDesc& g);
// JIT-compiled interval kernels for the shape (jit.hpp); null members -> interpreter
struct JitIntervalKernels {
    hipFunction_t coarse = nullptr, refine = nullptr;
};
void launch_brick_modes(const Program* d_prog, int depth, const float* d_rabbit, float2 tab_range, const GridDesc& g,
                        uint64_t* d_cmodes, uint8_t* d_ccls, uint32_t* d_clist, uint32_t* d_counters, uint64_t* d_modes,
                        uint8_t* d_cls, hipStream_t s, const JitIntervalKernels* jit = nullptr,
                        hipEvent_t after_coarse = nullptr /* recorded between the two kernels (timing) */);
// K1b: neighbour rule -> fill[b], the list of bricks to evaluate, constant sign bits of the rest
void launch_brick_fill(const GridDesc& g, const uint8_t* d_ccls, const uint64_t* d_cmodes, const uint8_t* d_cls,
                       const uint64_t* d_modes, int sign_fill, uint8_t* d_fill, uint32_t* d_list, uint64_t* d_lmodes,
                       uint32_t* d_count, void* d_signs, uint32_t* d_umark, uint32_t mark_id, hipStream_t s);
// K1c (interpreter): the listed bricks; the JIT variant is TreeJit::launch_bricks (jit.hpp)
constexpr int kEvalBlock = 256;   // lanes per block of the brick eval kernels
// whole waves (a partial wave would share the next block's brick index), within __launch_bounds__
static_assert(kEvalBlock % 64 == 0 && kEvalBlock <= 256, "kEvalBlock: whole waves, at most 256 lanes");
unsigned eval_bricks_grid(const GridDesc& g);
void launch_eval_bricks_interp(const Program* d_prog, int depth, const float* d_rabbit, const GridDesc& g,
                               const uint64_t* d_modes, const uint32_t* d_list, const uint32_t* d_count,
                               float* d_field, void* d_signs, const ClaimCtx& cc, hipStream_t s);
// sign bitmap of a fully written field (unpruned path)
void launch_signs_from_field(const GridDesc& g, const float* d_field, uint64_t* d_signs, hipStream_t s);
void launch_eval_points(const Program* d_prog, int depth, const float* d_rabbit, const float* d_xyz, int64_t n,
                        float* d_f, float* d_grad /* nullable: values only */, hipStream_t s);
// per-vertex normals -g / |g| at n points (ob02.hip k_vertex_normals, the interpreter form of
// ob02_device.hpp vertex_normals_body); d_counters (nullable): a slab's counter block, whose emitted
// vertex count then bounds the pass (n: the capacity the grid covers); *d_problems += the -42 rows
void launch_vertex_normals(const Program* d_prog, int depth, const float* d_rabbit, const float* d_pts, int64_t n,
                           const uint32_t* d_counters, float* d_normals, unsigned long long* d_problems, hipStream_t s);
// diagnostics: glibc sinf (0) / atanf (1) / atan2f (2) restatements on device operands
void launch_libm_probe(int which, const float* d_a, const float* d_b, int64_t n, float* d_out, hipStream_t s);
void launch_cos_probe(const double* d_a, int64_t n, double* d_out, hipStream_t s);
// diagnostics: the interval evaluator on n boxes, one thread per box (jit_fn: a tree module's
// impli_debug_iv instead of the interpreter), and the pruned point interpreter with a modes word per point
void launch_iv_probe(const Program* d_prog, int depth, const float* d_rabbit, float2 tab_range, const float* d_boxes,
                     const uint64_t* d_modes_in /* nullable */, int64_t n, float* d_iv, uint64_t* d_modes_out,
                     hipStream_t s, hipFunction_t jit_fn = nullptr);
void launch_eval_modes_probe(const Program* d_prog, int depth, const float* d_rabbit, const float* d_xyz,
                             const uint64_t* d_modes, int64_t n, float* d_f, hipStream_t s);

// The bounds descent (implisolid_bounds; DESIGN "Bounds of the solid"): levels 3 .. depth of the
// search box's 2^depth-cell edge table, one launch per level on s, no host synchronisation between
// them.  The device state: count[l] = mixed boxes listed at level l (the next launch's items are
// read from it), the running bounds as order-preserving keys of the edge floats {min x, max x, min
// y, max y, min z, max z} (no contribution: min keys all ones), an overflow flag (a list was full:
// the result is void, rerun with longer lists) and the work counters.
struct BoundsState {
    uint32_t count[12];
    uint32_t key[6];
    uint32_t overflow, pad;
    unsigned long long evaluated, skipped;
};
constexpr uint32_t kBoundsMaxList = 1u << 27;   // boxes of level 9: the longest list any descent needs
// order-preserving key of a float (no NaN): a < b  <=>  key(a) < key(b)
__host__ __device__ inline uint32_t bounds_key(uint32_t float_bits) {
    return (float_bits & 0x80000000u) ? ~float_bits : (float_bits | 0x80000000u);
}
__host__ __device__ inline uint32_t bounds_key_bits(uint32_t key) {
    return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
}
// d_edges: 3 (2^depth + 1) floats (host.hpp bounds_edges); d_box / d_modes: the two alternating
// lists of `cap` entries each (box index x | y << 10 | z << 20 at its level, its modes word)
void launch_bounds_levels(const Program* d_prog, int prog_depth, const float* d_rabbit, float2 tab_range,
                          const float* d_edges, int depth, uint32_t* const d_box[2], uint64_t* const d_modes[2],
                          uint32_t cap, BoundsState* d_state, hipStream_t s);

// Mass properties (implisolid_mass; DESIGN "Mass properties of the solid", mass.hip): the ten integer
// moments of the solid cells' indices and the solid cells per z layer, all launches on s with no host
// synchronisation between them.  The device state: count[l] = mixed boxes listed at level l (the last
// level's, depth - 2, is the leaf list's length; the counts keep counting past the capacity), the
// overflow flag (a list was full: the result is void, rerun with longer lists), the work counters and
// the moments.
struct MassState {
    uint32_t count[12];
    uint32_t overflow, pad;
    unsigned long long bounded, whole_cells;   // boxes bounded; cells counted whole from solid boxes
    unsigned long long moments[10];            // n, Si, Sj, Sk, Sii, Sjj, Skk, Sij, Sjk, Sik
};
// d_edges: 3 (2^depth + 1) floats (host.hpp bounds_edges); d_mids: 3 2^depth floats (host.hpp
// mass_mids); d_layers: 2^depth counters; d_box / d_modes: the two alternating lists of `cap` entries
// each, as launch_bounds_levels takes them (not read when prune is false: every leaf is evaluated
// with modes word 0).  State and layer counts are zeroed by the first launch.
void launch_mass(const Program* d_prog, int prog_depth, const float* d_tab, float2 tab_range, const float* d_edges,
                 const float* d_mids, int depth, bool prune, uint32_t* const d_box[2], uint64_t* const d_modes[2],
                 uint32_t cap, MassState* d_state, unsigned long long* d_layers, hipStream_t s);

// the interpreter's stack class for a program of this depth (eval.hip: 12 slots at least, see there)
int eval_depth(int depth);
// exclusive scan of n uint32 into out[0 .. n], out[n] = the total (ob02.hip's scan kernels); sums:
// scratch of n / 4096 + 2 words; zero_in leaves in[] zeroed
void launch_scan_u32(uint32_t* in, uint32_t* out, int64_t n, uint32_t* sums, bool zero_in, hipStream_t s);

// Slicing (implisolid_slice; DESIGN "Slices of the solid"): the marching-squares contours of the
// planes z[l] on an R-cell grid of xs x ys (host.hpp slice_coords), in tiles of kSliceTile cells.
// One chunk = `n` consecutive (layer, tile) items from global item `first` (item = layer * tiles per
// layer + ty * ntx + tx); all launches on s, no host synchronisation inside a function.
struct SliceGrid {
    int R, ntx;          // cells and tiles per axis
    uint32_t tpl;        // tiles per layer = ntx^2
};
struct SliceState {      // zeroed before classify
    uint32_t n_listed, pad;
    unsigned long long samples;   // samples the listed tiles hold
};
constexpr int kSliceSide = kSliceTile + 1, kSliceSamples = kSliceSide * kSliceSide;
constexpr uint32_t kSliceMaxChunk = 1u << 20;   // items per chunk: 512 segments each stay below 2^32
// classify: one thread per item; prune: bound the tile's box with the interval interpreter and list
// only mixed tiles (with their modes words), else list every tile with modes word 0.  list / lmodes:
// n entries (chunk-local item indices, in any order)
void launch_slice_classify(const Program* d_prog, int prog_depth, const float* d_tab, float2 tab_range, const float* d_xs,
                           const float* d_ys, const float* d_z, SliceGrid g, int64_t first, uint32_t n, bool prune,
                           uint32_t* d_list, uint64_t* d_lmodes, SliceState* d_state, hipStream_t s);
// march: one block per listed tile; its samples into d_samples[slot][kSliceSamples], its segment
// count into d_counts[item] (zeroed by the caller: unlisted tiles hold 0)
void launch_slice_march(const Program* d_prog, int prog_depth, const float* d_tab, const float* d_xs, const float* d_ys,
                        const float* d_z, SliceGrid g, int64_t first, uint32_t n_listed, const uint32_t* d_list,
                        const uint64_t* d_lmodes, float* d_samples, uint32_t* d_counts, hipStream_t s);
// emit: one block per listed tile; segments {x0, y0, x1, y1} and keys {start, end} at
// d_offsets[item] (the exclusive scan of d_counts) + the cell's prefix inside the tile; total: the
// chunk's segment count (nothing is written at or past it)
void launch_slice_emit(const float* d_xs, const float* d_ys, SliceGrid g, int64_t first, uint32_t n_listed,
                       const uint32_t* d_list, const float* d_samples, const uint32_t* d_offsets, uint32_t total,
                       float* d_xy, uint32_t* d_keys, hipStream_t s);
// out[k] = d_offsets[k * tpl] for k <= n_layers: the chunk's per-layer offsets and its total
void launch_slice_layer_offsets(const uint32_t* d_offsets, uint32_t tpl, uint32_t n_layers, uint32_t* d_out, hipStream_t s);

// Layer images (implisolid_raster; DESIGN "Layer images of the solid", raster.hip): the coverage bytes
// of the planes z[l] on a W x H-pixel grid with s x s samples per pixel (host.hpp raster_coords), in
// tiles of kRasterTile pixels.  One chunk = `n` consecutive (layer, tile) items from global item `first`
// (item = layer * tiles per layer + ty * ntx + tx); all launches on s, no host synchronisation inside a
// function.  The chunk's device image holds H rows of `pitch` = 16 ntx bytes per layer, so every tile
// row is 16 aligned bytes; the caller zeroes it (tiles outside the solid are never written).
struct RasterGrid {
    int W, H, s;         // pixels per axis, samples per pixel and axis
    int ntx, nty;        // tiles per axis
    uint32_t tpl;        // tiles per layer = ntx nty
    uint32_t pitch;      // bytes per image row = 16 ntx
};
struct RasterState {     // zeroed before classify
    uint32_t n_eval, n_fill;      // the two lists' lengths
    unsigned long long samples;   // samples the listed tiles evaluate
};
constexpr uint32_t kRasterMaxChunk = 1u << 20;   // items per chunk: the image stays at or below 256 MiB
// classify: one thread per item; prune: bound the tile's box with the interval interpreter, append
// solid tiles to d_fill and mixed ones (with their modes words) to d_list / d_lmodes, else append
// every tile to d_list with modes word 0.  The lists hold n entries each (chunk-local item indices,
// in any order)
void launch_raster_classify(const Program* d_prog, int prog_depth, const float* d_tab, float2 tab_range, const float* d_mx,
                            const float* d_my, const float* d_z, RasterGrid g, int64_t first, uint32_t n, bool prune,
                            uint32_t* d_list, uint64_t* d_lmodes, uint32_t* d_fill, RasterState* d_state, hipStream_t s);
// eval: one block per listed tile, one pixel per lane; its 256 coverage bytes into d_img (not written
// when null) and their sum onto d_sums[layer].  l0: the chunk's first layer (the image's row 0)
void launch_raster_eval(const Program* d_prog, int prog_depth, const float* d_tab, const float* d_mx, const float* d_my,
                        const float* d_z, RasterGrid g, int64_t first, int l0, uint32_t n_listed, const uint32_t* d_list,
                        const uint64_t* d_lmodes, uint8_t* d_img, unsigned long long* d_sums, hipStream_t s);
// fill: sixteen solid tiles per block; s^2 in every pixel of the tile, nx ny s^2 onto d_sums[layer]
void launch_raster_fill(RasterGrid g, int64_t first, int l0, uint32_t n_fill, const uint32_t* d_fill, uint8_t* d_img,
                        unsigned long long* d_sums, hipStream_t s);

// What every layer pass takes: a chunk's image as launch_raster_eval and launch_raster_fill left it, n_layers x
// H rows of `pitch` bytes with the padding columns zero.  A pass with parameters of its own derives its grid.
struct LayerGrid {
    int W, H;            // pixels per axis
    uint32_t pitch;      // bytes per image row
    int threshold;       // solid: cov >= threshold
};
constexpr uint64_t kLayerMaxPixels = 1ull << 28;   // what one launch takes: a chunk is never less than one layer
// what every layer pass relies on; the passes add their own conditions.  what: the refusal's text behind "<who>: ",
// for the passes that tell a bad grid from a bad chunk
inline void check_layer_chunk(const LayerGrid& g, uint32_t n_layers, const char* who, const char* what = "chunk out of range") {
    if (g.W < 1 || g.H < 1 || g.W > kRasterMaxSide || g.H > kRasterMaxSide || g.pitch < (uint32_t)g.W || g.pitch % 16u != 0u ||
        n_layers < 1u || (uint64_t)n_layers * (uint64_t)g.H * (uint64_t)g.W > kLayerMaxPixels)
        throw std::runtime_error(std::string(who) + ": " + what);
}

// Islands of the layers (implisolid_islands; DESIGN "Islands of the layers", islands.hip): the connected
// components of the solid pixels (cov >= threshold) of a chunk's image, as launch_raster_eval and
// launch_raster_fill left it (n_layers x H rows of `pitch` bytes, padding columns zero).  d_lab: int32
// [n_layers][H][W], the pixel's component seed (the smallest py W + px of the component) or -1 where it is
// not solid.  The launches go on s in the order tiles, merge, rows, scan of d_counts (launch_scan_u32),
// roots, tally; only the chunk's per-layer offsets (every H-th entry of the scan and its last) are read
// back, between the scan and roots, to size the records.
struct IslandGrid : LayerGrid {
    int ntx, nty;        // label tiles per axis
    int connectivity;
};
struct IslandState {     // zeroed before the first chunk; the chunks add to it
    unsigned long long solid;     // solid pixels
};
constexpr int kIslandTileW = 64, kIslandTileH = 32;   // pixels per label tile
constexpr uint32_t kIslandMaxChunk = 1u << 18;   // (layer, raster tile) pairs per chunk: 2^26 pixels, a 256 MiB label array
IslandGrid island_grid(const LayerGrid& g, int connectivity);
// tiles: one block per tile; the tile-local components, labelled with their smallest index, into d_lab (every
// pixel is written), the solid pixels onto d_state->solid
void launch_island_tiles(IslandGrid g, uint32_t n_layers, const uint8_t* d_img, int32_t* d_lab, IslandState* d_state, hipStream_t s);
// merge: one lane per tile-border pixel; afterwards label == own index exactly at the seeds
void launch_island_merge(IslandGrid g, uint32_t n_layers, int32_t* d_lab, hipStream_t s);
// rows: d_counts[layer * H + py] = the seeds in the row
void launch_island_rows(IslandGrid g, uint32_t n_layers, const int32_t* d_lab, uint32_t* d_counts, hipStream_t s);
// roots: the records {seed, 0, 0, INT_MAX, seed / W, -1, -1, l0 + layer} in (layer, seed) order; d_offsets: the
// exclusive scan of d_counts, total: its last entry (nothing is written at or past it)
void launch_island_roots(IslandGrid g, uint32_t n_layers, int l0, const int32_t* d_lab, const uint32_t* d_offsets, uint32_t total,
                         int32_t* d_rec, hipStream_t s);
// tally: every label pointed at its seed; area, below and the extent added to the records.  d_layer_off:
// n_layers + 1 record offsets; below of the chunk's first layer reads d_carry (the image of layer l0 - 1, one
// layer of the same pitch; not read when l0 == 0: every pixel of layer 0 counts as supported)
void launch_island_tally(IslandGrid g, uint32_t n_layers, int l0, const uint8_t* d_img, const uint8_t* d_carry, int32_t* d_lab,
                         const uint32_t* d_layer_off, int32_t* d_rec, hipStream_t s);

// Pixel distance field of the layers (implisolid_layer_distance; DESIGN "Distance field of the layers",
// distance.hip): the exact squared Euclidean distance of every pixel of a chunk's image (as launch_raster_eval
// and launch_raster_fill left it) to the nearest pixel of the other class (solid: cov >= threshold), signed
// by the pixel's own class.  d_dist: int32 [n_layers][H][W].  d_rec: four u64 per layer of the call {solid,
// key, unsupported, unused}, zeroed before the first chunk; key = (D2 << 32) | (0xFFFFFFFF - index) of the
// widest solid pixel, 0 when the layer has none.  The launches go on s in the order columns, rows, unsupported.
constexpr int kDistNone = 1 << 30;                // no pixel of the other class in the layer
constexpr int kDistFar = 32768;                   // the column pass's "none in this column": kDistFar^2 == kDistNone
constexpr uint32_t kDistMaxChunk = 1u << 18;      // (layer, raster tile) pairs per chunk, as kIslandMaxChunk
// columns: one lane per (layer, column); d_dist = the signed vertical distance to the nearest pixel of the
// other class in the column (+ solid, - empty), magnitude kDistFar where the column holds none
void launch_distance_columns(LayerGrid g, uint32_t n_layers, const uint8_t* d_img, int32_t* d_dist, hipStream_t s);
// rows: one block per (layer, row); d_dist = +-D2 in place, the layer's solid pixels and widest key onto d_rec
// (layer l0 + ll of the call)
void launch_distance_rows(LayerGrid g, uint32_t n_layers, int l0, int32_t* d_dist, unsigned long long* d_rec, hipStream_t s);
// unsupported: the solid pixels of every layer but the call's first whose pixel in the distance layer below is
// < -reach2, onto d_rec.  Below the chunk's first layer lies d_carry (the last distance layer of the chunk
// before, H x W; not read when l0 == 0)
void launch_distance_unsupported(LayerGrid g, uint32_t n_layers, int l0, int64_t reach2, const int32_t* d_dist, const int32_t* d_carry,
                                 unsigned long long* d_rec, hipStream_t s);

// Hollowed layers (implisolid_layer_hollow; DESIGN "Hollowing the layer stack", hollow.hip): the window pass over
// the distance fields of the layers within reach.  The images (as launch_raster_eval and launch_raster_fill left
// them, H rows of `pitch` bytes, pitch a multiple of 16) and the distance fields (int32 [H][W], as
// launch_distance_rows left them) live in two rings of `ring` layers, layer m of the call in slot m % ring; ring ==
// n_layers, or ring > 2 reach (a voxel's window never meets itself).
struct HollowGrid : LayerGrid {
    int n_layers;        // of the call
    int reach, ends;     // layers within reach on either side; bit 0 / 1: the layers in front of / behind the call are empty
    uint32_t ring;       // layers in either ring
};
constexpr uint32_t kHollowMaxChunk = 1u << 18;    // (layer, raster tile) pairs per chunk, as kDistMaxChunk
constexpr int kHollowMaxReach = 1024;
constexpr uint64_t kHollowMaxWindow = 1ull << 20; // (2 reach + 1) x tiles per layer: the carried window stays at or below 1 GiB
// window: output layers [l0, l0 + n_out), every layer within reach of them inside the call in its slot of both
// rings.  d_wall2: reach + 1 thresholds in [0, 2^30).  d_out (nullable): uint8 [n_out][H][W], 0 for a core voxel and
// the coverage byte otherwise.  d_rec: two u64 per layer of the call {solid, core}, zeroed before the first batch
void launch_hollow_window(HollowGrid g, int l0, uint32_t n_out, const uint8_t* d_img, const int32_t* d_dist, const int32_t* d_wall2,
                          uint8_t* d_out, unsigned long long* d_rec, hipStream_t s);

// Support tips under the layer stack (implisolid_layer_supports; DESIGN "Support tips under the layer stack",
// supports.hip): one tip per non-empty cell of a square grid over each layer's unsupported pixels (dist > 0 and
// the pixel of the distance layer below < -reach2), and the layer each tip's column lands on.  The distances are
// launch_distance_rows' (int32 [n_layers][H][W]), the image launch_raster_eval's and launch_raster_fill's
// (n_layers x H rows of `pitch` bytes, pitch a multiple of 16, padding columns zero).  The chunk's table holds
// per (layer, cell) an 8-byte key (dist << 32) | (0xFFFFFFFF - p) of the cell's tip, 0 for a cell without one,
// and a 4-byte load; both zeroed before the cell pass.  Per chunk the launches go on s in the order cells,
// count, scan of d_counts (launch_scan_u32), launch_slice_layer_offsets with tpl = ncx ncy, emit, top; only
// the chunk's per-layer offsets are read back, between the scan and emit, to size the records.
struct SupportGrid : LayerGrid {
    int cell;            // the side of a cell in pixels
    uint32_t ncx, ncy;   // cells per axis: ceil(W / cell), ceil(H / cell)
};
constexpr uint32_t kSupportMaxChunk = 1u << 18;   // (layer, raster tile) pairs per chunk, as kDistMaxChunk
constexpr int kSupportMaxCell = 16384;
SupportGrid support_grid(const LayerGrid& g, int cell);
// cells: every unsupported pixel's key and count onto its cell of the table, each layer's unsupported pixels
// onto d_unsupported[l0 + layer].  Below the chunk's first layer lies d_carry (the last distance layer of the
// chunk before, H x W; not read when l0 == 0: the call's first layer has no unsupported pixel)
void launch_support_cells(SupportGrid g, uint32_t n_layers, int l0, int64_t reach2, const int32_t* d_dist, const int32_t* d_carry,
                          unsigned long long* d_keys, uint32_t* d_loads, unsigned long long* d_unsupported, hipStream_t s);
// count: d_counts[layer * ncx ncy + c] = the cell has a tip
void launch_support_count(SupportGrid g, uint32_t n_layers, const unsigned long long* d_keys, uint32_t* d_counts, hipStream_t s);
// emit: the records {p, depth, foot, load} in (layer, cell) order; d_offsets: the exclusive scan of d_counts,
// total: its last entry (nothing is written at or past it).  foot: the highest layer below the tip's own
// whose pixel p is solid, from the chunk's image down to its first layer, then d_top[p] (the same over the
// layers in front of the chunk, -1 for none; null when l0 == 0).  *d_bad: raised where a record contradicts
// its cell
void launch_support_emit(SupportGrid g, uint32_t n_layers, int l0, const unsigned long long* d_keys, const uint32_t* d_loads,
                         const uint32_t* d_offsets, uint32_t total, const uint8_t* d_img, const int32_t* d_top, int32_t* d_rec,
                         uint32_t* d_bad, hipStream_t s);
// top: d_top[p] raised to the highest solid layer of the chunk at p; l0 == 0 starts from -1 without reading it
void launch_support_top(SupportGrid g, uint32_t n_layers, int l0, const uint8_t* d_img, int32_t* d_top, hipStream_t s);

// Run-length layer images (implisolid_layer_runs; DESIGN "Run-length layer images", runs.hip): the runs of
// every layer's row-major stream p = py W + px over the real pixels of a chunk's image (as launch_raster_eval
// and launch_raster_fill left it: n_layers x H rows of `pitch` bytes, pitch a multiple of 16).  A pixel's value
// is its coverage byte (threshold 0) or cov >= threshold as 0 / 1; a run starts at p = 0 and wherever the value
// differs from the stream's pixel before, across row ends too.  The launches go on s in the order count, scan of
// d_counts (launch_scan_u32), launch_slice_layer_offsets with tpl = H, emit; only the chunk's per-layer offsets
// are read back, between the scan and emit, to size the records.
constexpr uint32_t kRunMaxChunk = 1u << 20;       // (layer, raster tile) pairs per chunk, as kRasterMaxChunk: a 256 MiB image
// count: d_counts[layer * H + py] = the runs that start in the row
void launch_run_count(LayerGrid g, uint32_t n_layers, const uint8_t* d_img, uint32_t* d_counts, hipStream_t s);
// emit: per run its start (p within its layer) and value, in (layer, start) order; d_offsets: the exclusive scan
// of d_counts, total: its last entry (nothing is written at or past it)
void launch_run_emit(LayerGrid g, uint32_t n_layers, const uint8_t* d_img, const uint32_t* d_offsets, uint32_t total,
                     uint32_t* d_start, uint8_t* d_value, hipStream_t s);

// Bodies of the layer stack (implisolid_layer_bodies; DESIGN "Bodies of the layer stack", bodies.hip): the
// connected components of the target voxels (target 1: cov >= threshold, 0: cov < threshold) through the whole
// stack under 6- or 26-adjacency, as a union-find over the stack's row runs.  The stack-wide arrays hold every
// chunk's runs: d_runs {x0, x1} int32 pairs, d_parent one int32 a run, d_rowoff one uint32 per image row of the
// stack + 1 (row l H + py holds runs [d_rowoff[row], d_rowoff[row + 1])).  Per chunk the launches go on s in the
// order count, scan of d_counts (launch_scan_u32), launch_slice_layer_offsets with tpl = H, emit, link; only the
// chunk's per-layer offsets are read back, between the scan and emit, to size the arrays.  Behind the last chunk:
// root_rows over the stack's rows, the scan of its counts, roots, tally.
struct BodyGrid : LayerGrid {
    int target, connectivity;
};
struct BodyState {       // zeroed before the first chunk; the chunks add to it
    unsigned long long voxels;    // target voxels
};
constexpr uint32_t kBodyMaxChunk = 1u << 20;      // (layer, raster tile) pairs per chunk, as kRasterMaxChunk: a 256 MiB image
constexpr uint64_t kBodyMaxRows = 1ull << 30;     // image rows of a stack: 65536 layers of 16384 rows
// count: d_counts[layer * H + py] = the row's target runs; the chunk's target voxels onto d_state->voxels
void launch_body_count(BodyGrid g, uint32_t n_layers, const uint8_t* d_img, uint32_t* d_counts, BodyState* d_state, hipStream_t s);
// emit: the chunk's `total` runs behind the `base` runs of the chunks before (base + total < 2^31): {x0, x1},
// parent = own index, and the rows' offsets; d_offsets: the exclusive scan of d_counts.  l0: the chunk's first layer
void launch_body_emit(BodyGrid g, uint32_t n_layers, int l0, const uint8_t* d_img, const uint32_t* d_offsets, uint32_t base,
                      uint32_t total, int32_t* d_runs, int32_t* d_parent, uint32_t* d_rowoff, hipStream_t s);
// link: every run of the chunk united with the adjacent runs of the row above it in its layer and of the layer
// below (the chunk's own, or for its first layer the last of the chunk before, from the same arrays)
void launch_body_link(BodyGrid g, uint32_t n_layers, int l0, const int32_t* d_runs, const uint32_t* d_rowoff, int32_t* d_parent,
                      hipStream_t s);
// root_rows: d_counts[row] = the row's roots, over the `rows` = layers x H rows of the stack
void launch_body_root_rows(BodyGrid g, uint32_t rows, const uint32_t* d_rowoff, const int32_t* d_parent, uint32_t* d_counts,
                           hipStream_t s);
// roots: d_ord[root run] = its ordinal, and the records {seed, 0, MAX, MAX, l0, -1, -1, -1} in seed order; d_offsets:
// the exclusive scan of d_counts, total: its last entry (nothing is written at or past it)
void launch_body_roots(BodyGrid g, uint32_t rows, const int32_t* d_runs, const uint32_t* d_rowoff, const int32_t* d_parent,
                       const uint32_t* d_offsets, uint32_t total, uint32_t* d_ord, long long* d_rec, hipStream_t s);
// tally: every run's length and extent added to its body's record; d_out (nullable): {start, length, body} per run
void launch_body_tally(BodyGrid g, uint32_t rows, const int32_t* d_runs, const uint32_t* d_rowoff, int32_t* d_parent,
                       const uint32_t* d_ord, uint32_t n_bodies, long long* d_rec, int32_t* d_out, hipStream_t s);

// Suction cups of the layer stack (implisolid_layer_cups; DESIGN "Suction cups of the layer stack", cups.hip): per
// layer l the empty voxels of layer l whose pocket of the prefix 0 .. l (the bodies of the empty class of layers
// 0 .. l) holds no voxel of the image frame.  The runs, their union-find and the rows' offsets are the bodies'
// with target 0, except that the caller numbers the stack's runs from 1 (launch_body_emit's base is 1 + the runs
// of the chunks before) and keeps d_parent[0] = 0: run 0 is the outside.  Stack-wide beside them, one entry a run:
// d_rootat int32, d_cup int32, d_first uint32 (zeroed; the finish keeps the heads' ordinals there).  Per chunk the
// launches go on s in the order body count, scan, body emit, frame; then per layer body link of that layer, mark,
// head, with no host synchronisation between layers.  Behind the last chunk: rows over the stack's rows, the scans
// of its two counts (launch_slice_layer_offsets with tpl = H gives cup_offsets and run_offsets), heads, tally.
struct CupState {        // zeroed before the first chunk
    unsigned long long cupped;    // the voxels of the cupped runs, counted by launch_cup_rows
};
// frame: parent = 0 for every run of the chunk that holds a frame voxel; behind emit, before any link of the chunk
void launch_cup_frame(BodyGrid g, uint32_t n_layers, int l0, const int32_t* d_runs, const uint32_t* d_rowoff, int32_t* d_parent,
                      hipStream_t s);
// mark: over one layer's runs [lo, hi), all linked: d_rootat[run] = its root, and the layer's smallest run of
// every closed root onto d_first[root] (as lo + hi - 1 - run, by maximum)
void launch_cup_mark(uint32_t lo, uint32_t hi, int32_t* d_parent, int32_t* d_rootat, uint32_t* d_first, hipStream_t s);
// head: d_cup[run] = the smallest run of the layer with the same closed root, or -1 where the root is 0
void launch_cup_head(uint32_t lo, uint32_t hi, const int32_t* d_rootat, const uint32_t* d_first, int32_t* d_cup, hipStream_t s);
// rows: per image row of the stack its heads (d_cup[run] == run) and its cupped runs (d_cup[run] >= 0); their
// voxels onto d_state->cupped
void launch_cup_rows(BodyGrid g, uint32_t rows, const int32_t* d_runs, const uint32_t* d_rowoff, const int32_t* d_cup,
                     uint32_t* d_head_counts, uint32_t* d_run_counts, CupState* d_state, hipStream_t s);
// heads: d_ord[head run] = its ordinal, and the records {seed, 0, MAX, MAX, -1, -1, pocket} in (layer, seed) order;
// d_offsets: the exclusive scan of d_head_counts, total: its last entry (nothing is written at or past it)
void launch_cup_heads(BodyGrid g, uint32_t rows, const int32_t* d_runs, const uint32_t* d_rowoff, const int32_t* d_cup,
                      const int32_t* d_rootat, const uint32_t* d_offsets, uint32_t total, uint32_t* d_ord, long long* d_rec,
                      hipStream_t s);
// tally: every cupped run's length and extent added to its cup's record; end: 1 + the stack's runs; d_out
// (nullable): {start, length, cup} per cupped run at d_offsets, the exclusive scan of d_run_counts, n_out: its last entry
void launch_cup_tally(BodyGrid g, uint32_t rows, uint32_t end, const int32_t* d_runs, const uint32_t* d_rowoff, const int32_t* d_cup,
                      const uint32_t* d_ord, uint32_t n_cups, long long* d_rec, const uint32_t* d_offsets, uint32_t n_out,
                      int32_t* d_out, hipStream_t s);

// Rays against the solid (implisolid_raycast; DESIGN "Rays against the solid", raycast.hip): per ray the
// first solid sample of the table d_ts (host.hpp ray_params, N + 1 floats), the bisection inside its
// bracket and the normal there.  One chunk = n rays (3 n floats of origins and directions each); both
// launches on s, no host synchronisation between them.
struct RayState {        // zeroed before the first chunk; the chunks add to it
    unsigned long long skipped, evaluated;   // segments proved outside / evaluated, up to each ray's hit segment
    unsigned long long hits, inside;         // rays with hit >= 0 / hit == 0
};
constexpr uint32_t kRayMaxChunk = 1u << 20;   // rays per chunk: 64 MiB of device scratch
// march: one wave per ray; prune: bound every segment of kRaySegment steps with the interval
// interpreter, skip the ones proved outside and evaluate the others with their modes words, else
// evaluate every segment with modes word 0, up to the first solid sample.  Per ray: d_hit (its index,
// or -1), d_hmodes (the hit segment's modes word), d_fhit (F there) and d_work (segments skipped |
// evaluated << 16)
void launch_ray_march(const Program* d_prog, int prog_depth, const float* d_tab, float2 tab_range, const float* d_ts,
                      const float* d_org, const float* d_dir, uint32_t n, int N, bool prune, int32_t* d_hit,
                      uint64_t* d_hmodes, float* d_fhit, uint32_t* d_work, hipStream_t s);
// finish: one lane per ray; B bisection rounds for hit >= 1, the normal (launch_vertex_normals' rule;
// d_normals nullable) for hit >= 0, d_t / d_f, and the work figures onto *d_state
void launch_ray_finish(const Program* d_prog, int prog_depth, const float* d_tab, const float* d_ts, const float* d_org,
                       const float* d_dir, uint32_t n, int N, int B, const int32_t* d_hit, const uint64_t* d_hmodes,
                       const float* d_fhit, const uint32_t* d_work, float* d_t, float* d_f, float* d_normals,
                       RayState* d_state, hipStream_t s);

// Solid spans along rays (implisolid_ray_spans; DESIGN "Solid spans along rays", rayspans.hip): per ray
// every maximal run of solid samples of the table d_ts, with both ends refined.  One chunk = n rays; the
// launches go on s in the order march, scan of d_counts (launch_scan_u32), tally, emit, refine; only the
// chunk's span total (the scan's last entry) is read back between tally and emit, to size the outputs.
struct SpanState {       // zeroed before the first chunk; the chunks add to it
    unsigned long long outside, solid;       // segments proved outside / proved solid
    unsigned long long spans, rays, inside;  // spans; rays with a span; rays whose first span has k_in == 0
};
// the chunk's (ray, segment) words: 64 MiB of device scratch.  A ray of nseg segments holds at most
// 32 nseg + 1 spans, so a chunk's spans stay below 2^28 + 2^20 and the 32-bit scan cannot wrap
constexpr uint64_t kSpanMaxWords = 1ull << 23;
// march: one wave per ray over the whole ray.  d_words[r * nseg + j]: segment j's solidity word (bit i =
// sample 64 j + 1 + i; 0 for a segment proved outside, its samples' mask for one proved solid); d_counts:
// the ray's spans; d_info: segments proved outside | proved solid << 12 | sample 0 solid << 31
void launch_span_march(const Program* d_prog, int prog_depth, const float* d_tab, float2 tab_range, const float* d_ts,
                       const float* d_org, const float* d_dir, uint32_t n, int N, bool prune, uint64_t* d_words,
                       uint32_t* d_counts, uint32_t* d_info, hipStream_t s);
// tally: the chunk's work figures added to *d_state
void launch_span_tally(uint32_t n, const uint32_t* d_counts, const uint32_t* d_info, SpanState* d_state, hipStream_t s);
// emit: d_offsets = the exclusive scan of d_counts (n + 1 entries); d_k[2 i], d_k[2 i + 1] = span i's
// {k_in, k_out}, d_ray_of[i] = its ray (chunk-local), rays in order and a ray's spans in increasing k_in
void launch_span_emit(uint32_t n, int N, const uint64_t* d_words, const uint32_t* d_info, const uint32_t* d_offsets,
                      int32_t* d_k, uint32_t* d_ray_of, hipStream_t s);
// refine: one lane per span end; d_t, d_f: 2 n_spans floats {in, out}; d_normals (nullable): 6 n_spans
void launch_span_refine(const Program* d_prog, int prog_depth, const float* d_tab, float2 tab_range, const float* d_ts,
                        const float* d_org, const float* d_dir, int N, int B, bool prune, uint32_t n_spans, const int32_t* d_k,
                        const uint32_t* d_ray_of, float* d_t, float* d_f, float* d_normals, hipStream_t s);

// the min / max pyramid of one sdf_3d table inside an object's table arena (host.hpp SdfTable: the
// padded table at tab_off, level L at lvl_off[L]); one launch per level, in order on s
void launch_sdf3d_pyramid(float* d_arena, uint32_t tab_off, int sx, int sy, int sz, uint32_t level0, int n_levels,
                          const uint32_t* lvl_off, hipStream_t s);

// K2 (count per group) and K2b (group bases + flat list of non-empty units)
void launch_mc_count(const CaseInfo* d_cases, const GridDesc& g, const MCBuffers& b, hipStream_t s);
void launch_mc_scan(const GridDesc& g, const MCBuffers& b, hipStream_t s);
// K3 and K4
void launch_mc_verts(const CaseInfo* d_cases, const GridDesc& g, const MCBuffers& b, hipStream_t s);
void launch_mc_faces(const CaseInfo* d_cases, const GridDesc& g, const MCBuffers& b, hipStream_t s);

// One object's device state for the merged launches of an object stream (BASELINE config 5): every
// stage of eval + MC runs once for all objects, block row y = object y (same grid for all objects,
// each with its own node program, buffers and counters; the interpreter kernels, since every
// object has its own tree).
struct ObjArgs {
    const Program* prog;
    uint64_t* cmodes;
    uint8_t* ccls;
    uint32_t* clist;
    uint64_t* modes;
    uint8_t* cls;
    uint8_t* fill;
    uint32_t* blist;
    uint64_t* lmodes;
    uint32_t* umark;
    uint32_t mark_id;
    float* field;
    void* signs;
    uint32_t* counters;
    uint32_t* claimed;   // the merged eval's claimed candidates, appended at counters[kClaimedWord]
    MCBuffers mc;
    // a stream that computes normals (launch_batch_vertex_normals), else null: 3 floats per vertex,
    // sized like mc.verts, and the object's count of -42 rows (counters + kNormalProblemsWord)
    float* normals;
    unsigned long long* nproblems;
};
// eval (interval passes, fill, listed bricks) and MC (count, scan, vertices, faces) of n objects;
// blocks per object are capped for the grid-stride kernels (small grids: most blocks would idle)
// Node-stack capacity: 9 slots for objects of depth <= 9 (the smallest capacity the compiler
// still indexes through VGPR index mode rather than select chains; the eval then runs four waves
// per SIMD, 128 VGPRs and a small spill), else the interpreter's 12 or 16
// every object's counter block (kCounterWords words) into d_out[n][kCounterWords]
void launch_gather_counters(const ObjArgs* d_objs, int n, uint32_t* d_out, hipStream_t s);
// device byte ranges to clear, one block each (an object stream's fresh engines' resets in one
// launch instead of a memset call per buffer); p 16-byte aligned, n <= kZeroPieceBytes
struct ZeroPiece { uint64_t p; uint32_t n, pad; };
constexpr uint32_t kZeroPieceBytes = 1u << 16;
void launch_zero_pieces(const ZeroPiece* d_pieces, int n, hipStream_t s);
void launch_batch_eval(const ObjArgs* d_objs, int n, int depth, int vdepth, const float* d_rabbit, float2 tab_range, const GridDesc& g,
                       int sign_fill, hipStream_t s);
constexpr int kBatchShallowDepth = 9;
// merged object streams: the shallow class as this many pipelines on separate streams (abi.hip;
// the deep class is always one more).  Config 5: 2 / 3 / 4 pipelines 0.58 / 0.64 / 0.85 ms against
// 0.545 for one (profiles/r04x_*): concurrent merged kernels contend more than they overlap.
constexpr int kBatchGroups = 1;
void launch_batch_mc(const ObjArgs* d_objs, int n, const CaseInfo* d_cases, const GridDesc& g, hipStream_t s);
// the normals (launch_vertex_normals' rule) of the vertices every one of the n objects emitted, into
// rows[k].normals, the -42 rows counted in *rows[k].nproblems: one launch behind launch_batch_mc;
// depth: the deepest program's (the stack classes of launch_batch_eval)
void launch_batch_vertex_normals(const ObjArgs* rows, int n, int depth, const float* d_rabbit, hipStream_t s);

}  // namespace impli
