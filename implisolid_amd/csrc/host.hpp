// host.hpp -- host side of the drop-in boundary: mc-settings parser, MP5 factory, matrix inverse.
#pragma once
#include <string>
#include <vector>

#include "json.hpp"
#include "program.hpp"

namespace impli {

// polygoniser_settings.hpp:8-85 mc_settings
struct MCSettings {
    float box[6] = {-1, 1, -1, 1, -1, 1};   // xmin, xmax, ymin, ymax, zmin, zmax
    int resolution = 28;
    bool ignore_root_matrix = false;
    int overall_repeats = 1;
    int vresampl_iters = 0;
    float vresampl_c = 1.0f;
    bool qem = false;
    bool projection = false;
    bool subdiv = true;
    float post_subdiv_noise = 0.01f;
    bool normals = false;   // additive: "normals.enabled", per-vertex normals with the mesh (no reference key)
    // additive: "fit_box": {"enabled", "depth", "margin"} -- build_geometry fits its sampling box to
    // the solid's interval bounds inside `box` (bounds_edges / fit_box below; no reference key)
    bool fit_box = false;
    int fit_depth = 3;      // levels of the bounds descent; default ceil(log2(resolution)) in [3, 10]
    int fit_margin = 2;     // cells of the fitted grid between the bounds and the box wall
};

// Errors the reference reports with abort() / clog.  The C ABI decides what to do with them
// (abort-compatible by default, see abi.cpp).
struct InputError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// parse_mc_properties_json (polygoniser_settings.hpp:147-305).  Throws InputError where the
// reference sets needs_abort.
MCSettings parse_mc_settings(const char* json_text);

// The edge table of the bounds descent (implisolid_bounds): N = 2^depth cells per axis of the search
// box {xmin, xmax, ymin, ymax, zmin, zmax}; per axis edge[k] = lo + (float)k * ((hi - lo) / (float)N)
// for k < N, each operation rounded to float on its own, and edge[N] = hi.  edges: 3 (N + 1) floats,
// x then y then z.  Throws InputError for a depth outside [3, 10] or a box that is not finite with
// lo < hi on every axis.
constexpr int kBoundsMinDepth = 3, kBoundsMaxDepth = 10;
void bounds_edges(const float search[6], int depth, float* edges);
// The sampling box for `bounds` inside the settings box `search`: per axis, in double,
// w = (b1 - b0) / (resolution - 2 margin), lo = max(s0, b0 - margin w), hi = min(s1, b1 + margin w),
// rounded to float.  False if resolution - 2 margin < 1 or margin < 0.
bool fit_box(const float search[6], const float bounds[6], int resolution, int margin, float out[6]);

// The sample points of the mass pass (implisolid_mass): per axis mid[k] = edge[k] + 0.5f * (edge[k + 1] -
// edge[k]) over bounds_edges' table, every operation rounded to float on its own; mids: 3 N floats, x
// then y then z.  Throws InputError as bounds_edges does, and when some edge[k] <= mid[k] <= edge[k + 1]
// fails (a cell's sample must lie inside every interval box that contains the cell).
void mass_mids(const float box[6], int depth, float* mids);
// Volume, centre of mass and inertia about it from the ten integer moments [n, Si, Sj, Sk, Sii, Sjj,
// Skk, Sij, Sjk, Sik] (include/implisolid.h implisolid_mass_physical states the arithmetic): out =
// [volume, cx, cy, cz, Ixx, Iyy, Izz, Ixy, Iyz, Ixz].  False and zeros when n == 0; throws InputError
// for a bad depth or box.
bool mass_physical(const float box[6], int depth, const uint64_t moments[10], double out[10]);

// The sample coordinates of a slice (implisolid_slice): R cells per axis of rect {xmin, xmax, ymin,
// ymax}; xs[i] = xmin + (float)i * ((xmax - xmin) / (float)R) for i < R, each operation rounded to float
// on its own, xs[R] = xmax, and ys the same way.  xs, ys: R + 1 floats each.  Throws InputError for a
// resolution outside [1, 4096] or a rect that is not finite with min < max on both axes.
constexpr int kSliceMaxResolution = 4096, kSliceMaxLayers = 65536;
constexpr int kSliceTile = 16;   // cells per tile side: part of the ABI (it fixes the segments' order)
void slice_coords(const float rect[4], int resolution, float* xs, float* ys);
// The sample coordinates of a raster (implisolid_raster): width x height pixels of rect, s = supersample
// sub-cells per pixel and axis.  The W s + 1 sub-cell edges follow slice_coords' formula with W s cells;
// mx[k] = edge[k] + 0.5f * (edge[k + 1] - edge[k]) as mass_mids has it, my the same over H s.  mx: W s
// floats, my: H s floats.  Throws InputError for a width or height outside [1, 16384], a supersample
// other than 1, 2, 4, a rect that is not finite with min < max, or a sample outside its sub-cell.
constexpr int kRasterMaxSide = 16384, kRasterMaxLayers = 65536;
constexpr int kRasterTile = 16;   // pixels per tile side
void raster_coords(const float rect[4], int width, int height, int supersample, float* mx, float* my);
// The sample parameters of a ray cast (implisolid_raycast): ts[k] = t0 + (float)k * ((t1 - t0) /
// (float)steps) for k < steps, each operation rounded to float on its own, ts[steps] = t1; steps + 1
// floats, shared by all rays.  Throws InputError for steps outside [1, 65536], a range that is not finite
// with t0 < t1, or a table that is not non-decreasing (ts[steps - 1] > t1: what puts every sample of a
// segment between the segment's end samples).
constexpr int kRayMaxSteps = 65536, kRayMaxBisect = 32;
constexpr int64_t kRayMaxRays = (int64_t)1 << 24;
constexpr int kRaySegment = 64;   // steps per segment: the unit of the pruning and of the stats
void ray_params(float t0, float t1, int steps, float* ts);
// Chains one layer's segments {start key, end key} into polylines by exact key matching
// (implisolid_slice_loops): order = a permutation of the segment indices, every polyline's segments
// consecutive; open chains first (by first segment), then closed loops, each from its lowest-indexed
// segment (by that index).  loop_offsets: polylines + 1 entries; closed: one flag per polyline.
// Returns the number of polylines, or -1 if a key starts two segments or ends two.
int64_t slice_loops(const uint32_t* keys, int64_t n_segments, int64_t* order, int64_t* loop_offsets, uint8_t* closed);

// The caller-supplied SDF tables of an object's sdf_3d nodes (sdf_3d.hpp:73-102: read from the node
// itself).  They travel beside the Program, whose NT_SDF3D parameter rows (program.hpp SdfParam)
// hold each table's place in the object's device table arena:
//   [0, kArenaRabbitFloats)   the rabbit section, as every object without sdf_3d reads it
//   per node                  the table, zero-padded to `padded` floats, then its min / max pyramid
//                             (float2 entries; built on the device, engine.hip TableArena)
// Level 0 has one entry per flat index b < level0 = sx + sy sx + sz sx sy + 1 (cube_iv's block
// table: min / max of the eight reads from b); level L >= 1 is a dense (s >> L) + 1 grid per axis
// whose entry combines 2 x 2 x 2 entries of level L - 1.
struct SdfTable {
    uint32_t sx, sy, sz;
    uint32_t padded;                  // floats of the zero-padded table: every index a read can reach
    uint32_t level0;                  // entries of level 0
    uint32_t n_levels;
    uint32_t tab_off;                 // arena offsets, in floats
    uint32_t lvl_off[kSdfMaxLevels];
    size_t data_off;                  // the padded table's start in ObjectTables::data
};
struct ObjectTables {
    std::vector<SdfTable> nodes;
    std::vector<float> data;          // the nodes' padded tables, one after the other
    size_t arena_floats = 0;          // the whole arena, rabbit section included
    bool empty() const { return nodes.empty(); }
    bool same(const ObjectTables& o) const;   // layout and table contents, bit for bit
};

// object_factory (object_factory.hpp:56-758) -> node program.  Throws InputError for unknown or
// unsupported node types (the reference abort()s on unknown ones, :731-734).  tables receives the
// object's sdf_3d tables; a caller that passes none cannot take a shape with such a node (InputError).
Program compile_mp5(const char* shape_json, bool ignore_root_matrix, ObjectTables* tables = nullptr);
Program compile_mp5(const Json& shape, bool ignore_root_matrix, ObjectTables* tables = nullptr);

// Z-slab decomposition of the cell layers 1 .. res-3 (res = R + 5) over nranks: rank r owns
// layers [z0, z1) and recomputes `halo` (0 or 1) layer below z0 (owner rule).
struct SlabRange { int z0, z1, halo; };
SlabRange slab_partition(int R, int rank, int nranks);
// the slab of cell layers [z0, z1); throws if its cells overflow the kernels' 32-bit cell ids
SlabRange slab_range(int R, int z0, int z1);

// glibc rand() / srand() restated (stdlib/random_r.c, TYPE_3: additive feedback
// x_n = x_{n-3} + x_{n-31} mod 2^32, output x_n >> 1; state seeded by the 16807 LCG, 310 outputs
// discarded).  randomize_verts (basic_functions.hpp:551-557) draws from the process-global rand() of
// the native reference build; the library keeps one process-global generator in that state (never
// seeded = srand(1), implisolid_srand to reseed), advanced only by subdivision.
//
// The state is kept as the window of the last 31 terms, so that n draws can be skipped (or handed
// to GPU lanes) with the polynomial z^n mod P(z), P = z^31 - z^28 - 1 over Z/2^32:
//   x_{m+n+j} = sum_i c_i x_{m+i+j}  where  z^n = sum_i c_i z^i  (mod P).
class GlibcRand {
public:
    explicit GlibcRand(unsigned seed = 1) { seed_(seed); }
    void seed_(unsigned seed);
    int32_t next();
    void fill(uint32_t* out, int64_t n) { for (int64_t i = 0; i < n; ++i) out[i] = (uint32_t)next(); }
    // x_m .. x_{m+60}: the window (oldest first) extended by 30 terms; draw k of the future is
    // produced from x_{m+k} and x_{m+k+28}
    void extended_window(uint32_t out[61]) const;
    void skip(uint64_t n);
private:
    uint32_t r_[31];
    int head_ = 0;   // r_[head_] is the oldest term x_{n-31}
};
GlibcRand& process_rand();

// z^n mod (z^31 - z^28 - 1), coefficients mod 2^32
void rand_jump_poly(uint64_t n, uint32_t c[31]);
void rand_poly_mulmod(const uint32_t a[31], const uint32_t b[31], uint32_t out[31]);

// basic_functions.hpp:77-128 invert_matrix (ublas LU on a float 4x4 with last row 0,0,0,1)
bool invert_matrix12(const float in[12], float out[12]);

}  // namespace impli
