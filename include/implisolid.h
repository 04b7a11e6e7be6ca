/*
 * implisolid.h -- C ABI of the MI355X-native implicit-surface polygoniser.
 *
 * Drop-in replacement for the extern "C" interface of ImpliSolid's mcc2.cpp.  Every declaration
 * below names the reference declaration it replaces (/root/reference/js_iteration_2/mcc2.cpp,
 * declarations :88-134, definitions as cited).  Signatures, argument meaning, ownership and error
 * behaviour are the reference's; the work runs on the GPU (HIP, gfx950).
 *
 * MP5 node families: the reference factory's primitives and CSG nodes, and "sdf_3d" with its table
 * in the node (size_x/y/z in [2, 512], at most 2^22 entries, grid_size, origin_x/y/z, "sdf"; at most
 * 8 per object): sampled trilinearly like the rabbit ("icube"), reads past the table return 0, the
 * gradient is the analytic in-cell gradient.  Rejected: "rawjscode", an "sdf_3d" without its table
 * fields, and any "sdf_3d" in implisolid_batch_create.
 *
 * Thread-safety: like the reference, one global geometry slot and one direct-eval slot; not
 * reentrant.  build_geometry returns after the result is host resident.
 */
#ifndef IMPLISOLID_H
#define IMPLISOLID_H

#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- mesh API ------------------------------------------------------------------------------ */
/* mcc2.cpp:89 / :446-464  polygonise the MP5 shape with the given mc_settings JSON.  Refuses (with
   a message) while a previous result is active: call finish_geometry() first (:316-319). */
void build_geometry(const char* shape_parameters_json, const char* mc_parameters_json);
/* mcc2.cpp:90 (declared, body commented out at :296-302): build_geometry + worker call specs
   ({"progressCallback_id", "call_id", "shape_id"}, worker_call_specs.hpp:28-40; each -1 when
   absent).  Progress updates carry those ids (see implisolid_set_progress_callback). */
void build_geometry_u(const char* shape_parameters_json, const char* mc_parameters_json, const char* call_specs);
/* Additive: the progress hook of build_geometry / build_geometry_u -- the reference's
   polygonizer::send_mesh_back_to_client (polygonizer_algorithm_ob02.hpp:180-220), which posts the
   current mesh to wwapi.send_progress_update (js/worker_api.js:399-416) after marching cubes
   (mcc2.cpp:351), after each repeat's vertex resampling (:372) and after each centroid projection
   (:390).  The callback runs synchronously on the calling thread with the intermediate mesh
   (library-owned, valid during the call; get_v_ptr / get_f_ptr / get_v_size / get_f_size read the
   same mesh meanwhile) and the call specs' ids (-1 for plain build_geometry).  NULL unregisters. */
typedef void (*implisolid_progress_callback)(const float* verts, int n_verts, const int32_t* faces, int n_faces,
                                             int progress_callback_id, int shape_id, int call_id, void* user);
void implisolid_set_progress_callback(implisolid_progress_callback cb, void* user);
/* mcc2.cpp:91 / :470-473  vertex count */
int get_v_size(void);
/* mcc2.cpp:92 / :466-469  face count */
int get_f_size(void);
/* mcc2.cpp:93 / :496-511  copy 3*fcount int32 vertex indices */
void get_f(int* f_out, int fcount);
/* mcc2.cpp:94 / :474-492  copy 3*vcount float32 coordinates */
void get_v(float* v_out, int vcount);
/* mcc2.cpp:95 / :540-552  release the slot (buffers stay valid until the next build) */
void finish_geometry(void);
/* mcc2.cpp:96 / :521-525  library-owned int32 triplets */
void* get_f_ptr(void);
/* mcc2.cpp:97 / :515-519  library-owned float32 xyz */
void* get_v_ptr(void);
/* Additive: per-vertex surface normals with the mesh, from the same build.  The mc_settings key
   "normals": {"enabled": 1} (an int, read like projection.enabled: true / false are not ints and
   leave the default 0; the reference ignores the key) makes build_geometry evaluate the implicit
   gradient at the final vertices -- after the last step of the OB02 loop, or at the marching-cubes
   vertices when nothing refines them -- and apply what calculate_implicit_gradients(true) applies,
   mcc2.cpp:852-871: norm = sqrt(x x + y y + z z); n = g * (norm > 0.0001 ? -1 / norm : -42).  This
   replaces the reference front end's second round trip (implisolid_main.js:335-368 and :583-622:
   set_object, set_x with fewer than 50000 points, calculate_implicit_gradients, get_gradients_ptr;
   its author's note at :551 asks for "the normals in the same request").  Names as the reference
   names get_v_*:
     get_n_size  the vertex count if the last build computed normals, else 0
     get_n_ptr   library-owned float32 xyz per vertex, valid like get_v_ptr's until the next build;
                 NULL when the size is 0
     get_n       copy 3*vcount floats
   A build without the key exposes nothing, also directly after one that had normals.  Intermediate
   meshes carry no normals: inside a progress callback get_n_size() is 0; the final mesh has them.
   With implisolid_set_devices each slab's device computes the normals of the vertices it emitted
   (after a refinement: the device the loop ran on).  The object stream (implisolid_batch_*) honours
   the key too: implisolid_batch_download_normals.  implisolid_normals_stats: out = [normals computed, rows that took the -42 branch] of the
   last build; 0, or -1 with implisolid_last_error(). */
int get_n_size(void);
void* get_n_ptr(void);
void get_n(float* n_out, int vcount);
int implisolid_normals_stats(int64_t out[2]);

/* ---- direct evaluation API ------------------------------------------------------------------ */
/* mcc2.cpp:106 / :726-741  returns 1, or 0 if an object is already set */
int set_object(const char* shape_parameters_json, bool ignore_root_matrix);
/* mcc2.cpp:107 / :743-763 */
bool unset_object(int id);
/* mcc2.cpp:109 / :765-799  0 <= n < 50000 points, float32 xyz */
bool set_x(void* verts, int n);
/* mcc2.cpp:110 / :800-812 */
void unset_x(void);
/* mcc2.cpp:112 / :815-822 */
void calculate_implicit_values(void);
/* mcc2.cpp:113 / :827-829 */
void* get_values_ptr(void);
/* mcc2.cpp:114 / :830-832 */
int get_values_size(void);
/* mcc2.cpp:116 / :834-889  with normalize_and_invert: g <- -g/|g| (factor -42 if |g| <= 1e-4) */
void calculate_implicit_gradients(bool normalize_and_invert);
/* mcc2.cpp:117 / :890-903 */
void* get_gradients_ptr(void);
/* mcc2.cpp:118 / :904-911  = 3n */
int get_gradients_size(void);

/* ---- misc ------------------------------------------------------------------------------------ */
/* mcc2.cpp:122 / :203-209  debug point sets (pre/post_resampling_vertices, pre/post_p_centroids,
   pre/post_qem_verts); NULL if absent */
void* get_pointset_ptr(char* id);
/* mcc2.cpp:123 / :210-215 */
int get_pointset_size(char* id);
/* mcc2.cpp:126 / :574-617  build information */
void about(void);

/* ---- additive API (not in the reference) ---------------------------------------------------- */
/* last error message of this thread's calls ("" if none) */
const char* implisolid_last_error(void);
/* 0 (default): abort() where the reference aborts (bad settings, unknown MP5 type);
   1: print the same message, record it in implisolid_last_error() and return */
void implisolid_set_error_mode(int mode);

/* Additive: per-brick interval pruning of the field evaluation (process-wide; environment
 * IMPLISOLID_PRUNE=<level> sets the initial level).  0 off; 1 CSG operands proven irrelevant over a
 * brick are skipped (field bit-identical); 2 (default) additionally fills bricks that are
 * sign-definite together with their face neighbours with +-1 (only their sign is ever read, so
 * the mesh is bit-identical). */
void implisolid_set_pruning(int level);

/* Additive, host only: the library's process-global glibc rand() generator, which the subdivision
 * noise draws from (randomize_verts, basic_functions.hpp:551-557, calls the C library's rand()).
 * It starts in glibc's unseeded state (srand(1)); implisolid_srand/implisolid_rand behave as
 * srand/rand; implisolid_rand_skip(n) discards n draws (jump-ahead, O(log n)). */
void implisolid_srand(unsigned seed);
int implisolid_rand(void);
void implisolid_rand_skip(uint64_t n);

/* Additive, host only: the parsed mc-settings (polygoniser_settings.hpp:147-305 semantics).
 * ints = resolution, ignore_root_matrix, overall_repeats, vresampl.iters, projection, qem, subdiv;
 * floats = vresampl.c, debug.post_subdiv_noise.  0, or -1 with implisolid_last_error() set where
 * the reference would abort() (error mode 0 aborts, as the reference). */
int implisolid_parse_settings(const char* mc_json, float box[6], int32_t ints[7], float floats[2]);

/* Additive, host only: Z-slab decomposition used by the slab API -- rank owns cell layers
 * [out[0], out[1]) and recomputes out[2] (0/1) halo layers below. */
int implisolid_slab_partition(int R, int rank, int nranks, int32_t out[3]);
/* Additive: balanced Z-slab cuts (nranks + 1 cell-layer boundaries, cuts[0] = 1, cuts[nranks] =
 * R + 3; rank r owns layers [cuts[r], cuts[r+1])).  Runs the interval pass of the whole grid once
 * on the current HIP device and splits the estimated work (listed bricks per layer) evenly; every
 * rank computing it gets the same cuts, so no exchange is needed (blocking). */
int implisolid_slab_balance(const char* shape_json, const char* mc_json, int nranks, int32_t* cuts);
/* host only: the same split from per-sample-layer listed-brick counts of the whole grid
 * (n_layers = R + 3) and the bricks per layer */
int implisolid_cuts_from_layer_work(const int64_t* listed, int n_layers, int64_t bricks_per_layer, int R, int nranks,
                                    int32_t* cuts);
/* Additive: the devices build_geometry uses for marching cubes (HIP ordinals; n <= 0 or NULL: the
 * current device only).  With n > 1 the grid is split into n balanced Z-slabs, slab r on device
 * ids[r] (a device may repeat), the slabs' meshes are concatenated in rank order on the host --
 * byte-identical to one device -- and the OB02 steps run on ids[0]. */
int implisolid_set_devices(const int32_t* ids, int n);
/* Additive diagnostics of the OB02 steps (polygonizer_algorithm_ob02.hpp:74-157 keeps per-step
 * timers, timer.hpp:33-75).  With profiling on, build_geometry drains its stream at every stage
 * boundary and sums each stage's wall time, and counts the projection's implicit evaluations (off
 * by default: the stages then overlap and nothing is counted).  last_build_stats (blocking) returns
 * [bisections that hit the 200-round cap (F8e), projection evaluations (profiled builds),
 *  last average edge length, ms of: topology, vertex resampling, edge-length fold, projection, QEM,
 *  subdivision, result fetch (profiled builds), faces, vertices, OB02 passes that ran the JIT point
 *  module] of the last build. */
void implisolid_ob02_profile(int on);
int implisolid_last_build_stats(double out[13]);
/* evaluate n >= 0 points (no 50k limit) of the current set_object(); grad may be NULL */
int implisolid_eval_points(const float* xyz, int64_t n, float* f_out, float* grad_out);
/* Additive: the normals of n >= 0 points of the current set_object() (no 50k limit), by the kernel
   build_geometry's "normals" key runs: out receives 3n floats, -g / |g| per mcc2.cpp:852-871 (-42 g
   where |g| <= 0.0001, or is not a number); *problems (may be NULL) the number of such rows.
   calculate_implicit_gradients keeps its own host loop.  0, or -1 with implisolid_last_error(). */
int implisolid_eval_normals(const float* xyz, int64_t n, float* out, int64_t* problems);
/* Additive, diagnostics: the device restatements of glibc 2.35 sinf (which 0: out = sinf(a)),
   atanf (1) and atan2f (2: out = atan2f(a, b)) that the screw family calls (screw.hpp:20-36,
   std::sin / std::atan2 on floats), on n host operands; 0 or -1 with implisolid_last_error() */
int implisolid_debug_libm(int which, const float* a, const float* b, int64_t n, float* out);
/* Additive, diagnostics: the device restatement of glibc 2.35's double cos (x86_64 FMA variant) that
   the screw gradient calls (screw.hpp:178-180, cos(M_PI * (...))), on n host doubles; 0 or -1 */
int implisolid_debug_cos(const double* a, int64_t n, double* out);
/* Additive, diagnostics: the edge-length fold of the projection (compute_average_edge_length,
   centroids_projection.cpp:70-82: s = 0; s += e[k] in order, float) on n host terms, computed as
   build_geometry computes it -- the chunk table and the device walk; *sum_out = s, *table_chunks
   (may be NULL) = chunks the walk took from the table.  0, or -1 with implisolid_last_error(). */
int implisolid_debug_fold(const float* terms, int64_t n, float* sum_out, int64_t* table_chunks);
/* Additive, diagnostics (never called by build_geometry or the slab pipeline): the interval evaluator
   that prunes CSG operands per brick, on n caller-given world-space boxes {xlo, xhi, ylo, yhi, zlo,
   zhi} of the MP5 tree, one thread per box.  variant 0: the interpreter (eval_iv); 1: the tree
   shape's hipRTC module (tree_iv, matrices read from memory); 2: the object's baked module (matrices
   as literals) -- 1 and 2 compile the module first if need be.  modes_in (may be NULL: nothing
   pruned) holds per box the modes word of an enclosing box; iv_out receives {lo, hi} of the root and
   modes_out the 2-bit decision per CSG node (0 both operands, 1 left only, 2 right only; nodes past
   the 32nd are never pruned).  0, or -1 with implisolid_last_error(). */
int implisolid_debug_intervals(const char* shape_json, int ignore_root_matrix, int variant, const float* boxes,
                               const uint64_t* modes_in, int64_t n, float* iv_out, uint64_t* modes_out);
/* Additive, diagnostics: the pruned point interpreter (eval_f_pruned) at n points, each with its own
   modes word (as implisolid_debug_intervals returns them for a box holding the point); 0 or -1 */
int implisolid_debug_eval_modes(const char* shape_json, int ignore_root_matrix, const float* xyz, const uint64_t* modes,
                                int64_t n, float* f_out);

/* Additive: the axis-aligned bounds of the solid inside a search box, from the interval evaluator (no
 * reference counterpart: the front end guesses boxes from node matrices, boundingbox_utils.js:63-196).
 *   search  {xmin, xmax, ymin, ymax, zmin, zmax}, the order implisolid_parse_settings returns a box
 *   depth   in [3, 10]: the box is cut into N = 2^depth cells per axis by the edge table of
 *           implisolid_bounds_edges; level l (3 .. depth) has 2^l boxes per axis, box i spanning
 *           edge[i << (depth - l)] .. edge[(i + 1) << (depth - l)]
 * The 512 boxes of level 3 are bounded with modes word 0, a child with its parent's returned modes
 * word (implisolid_debug_intervals' modes_in).  A box whose bound is hi < 0 is dropped; one with
 * lo >= 0 contributes its extent and is not cut further; any other (a NaN bound included) is cut
 * into its eight children, or at level `depth` contributes its extent.  out = the per-axis min / max
 * over the contributions: deterministic, never inside the solid's true extent, and at most the
 * interval bounds' slack plus one cell of level `depth` outside it.  An unbounded primitive
 * (half_plane, inf_screw, a lid) yields `search` on the axes where it is unbounded.
 *   returns 1 and out = the bounds; 0 when the solid is empty in `search` (out = search); -1 with
 *           implisolid_last_error() for a depth outside [3, 10], a box that is not finite with
 *           min < max on every axis, or an unsupported node
 *   stats   (may be NULL) [boxes bounded, boxes skipped because they lay inside the bounds found so
 *           far (they cannot extend them; only the work depends on it), longest list of boxes cut at
 *           one level, reruns after a list overflowed]
 * One kernel launch per level on the library's stream, one read-back at the end.  The lists start at
 * IMPLISOLID_BOUNDS_LIST boxes (environment, read at each call; default 8 N^2, at most 2^21) and
 * grow when a level overflows them, after which the descent runs again. */
int implisolid_bounds(const char* shape_json, int ignore_root_matrix, const float search[6], int depth, float out[6],
                      int64_t stats[4]);
/* host only (no GPU): the edge table, 3 (N + 1) floats, x then y then z.  Per axis
 * edge[k] = lo + (float)k * ((hi - lo) / (float)N) for k < N, every operation rounded to float on its
 * own (no fused multiply-add), and edge[N] = hi.  0, or -1 (depth, box) */
int implisolid_bounds_edges(const float search[6], int depth, float* edges);
/* host only: the sampling box that puts `bounds` on `resolution - 2 margin` cells with `margin` cells
 * around them, clipped to the settings box `search`.  Per axis, in double:
 * w = (b1 - b0) / (resolution - 2 margin), lo = max(s0, b0 - margin w), hi = min(s1, b1 + margin w),
 * then rounded to float.  0, or -1 if resolution - 2 margin < 1 or margin < 0 */
int implisolid_fit_box(const float search[6], const float bounds[6], int resolution, int margin, float out[6]);
/* The mc-settings key "fit_box": {"enabled": 1, "depth": d, "margin": m} (ints, read as
 * "projection.enabled" is; true / false are no ints and leave it off).  build_geometry and
 * build_geometry_u then take the settings box as the search box: they find the bounds on the
 * build's device (ids[0] under implisolid_set_devices), replace the box by implisolid_fit_box's
 * and run unchanged on it (marching cubes, the OB02 loop, normals, progress callbacks).  The fitted
 * box never leaves the settings box, which stays the caller's clip region; an empty solid keeps
 * the box as given.  depth defaults to ceil(log2(resolution)) clamped to [3, 10], margin to 2.
 * Without the key nothing changes.  implisolid_slab_create* and implisolid_batch_create refuse an
 * enabled key (their grids are the caller's, or shared by all objects).
 *   parse_fit_box  host only: out = {enabled, depth, margin} as a build would read them; 0 or -1
 *   last_fit_box   1 and out = the box the last build used if it was fitted, else 0 */
int implisolid_parse_fit_box(const char* mc_json, int32_t out[3]);
int implisolid_last_fit_box(float out[6]);
/* diagnostics: with enable != 0 the following implisolid_bounds calls (and fitted builds) time their
 * level launches with HIP events; returns the last such figure in milliseconds (-1: none yet) */
double implisolid_debug_bounds_ms(int enable);

/* Additive: the solid's closed outlines on the planes z = z[l], by marching squares on the GPU (no
 * reference counterpart; a slicer's input).
 *   rect        {xmin, xmax, ymin, ymax}, finite with min < max
 *   resolution  R in [1, 4096] cells per axis; the samples are xs[0 .. R] x ys[0 .. R] of
 *               implisolid_slice_coords
 *   z           n_layers in [1, 65536] finite plane heights, in the caller's order (they may repeat and
 *               need not be sorted)
 * F[l][j][i] is implisolid_eval_points' value at (xs[i], ys[j], z[l]); a sample is solid iff !(F < 0)
 * (marching cubes' rule; a NaN counts as solid).  Cell (i, j), i, j < R, has the corners c0 = (i, j),
 * c1 = (i + 1, j), c2 = (i + 1, j + 1), c3 = (i, j + 1); case bit k is set iff ck is solid.  With
 * W = R + 1 its edges and their keys are
 *   e0 bottom c0-c1  2 (j W + i)          e1 right c1-c2  2 (j W + i + 1) + 1
 *   e2 top    c3-c2  2 ((j + 1) W + i)    e3 left  c0-c3  2 (j W + i) + 1
 * (even: an x-edge, odd: a y-edge, each named after its lower sample).  Segments are directed with the
 * solid on their left (x right, y up):
 *   case 1 e0>e3   2 e1>e0   4 e2>e1   8 e3>e2   3 e1>e3   6 e2>e0   5 e0>e3 then e2>e1
 *       14 e3>e0  13 e0>e1  11 e1>e2   7 e2>e3  12 e3>e1   9 e0>e2  10 e1>e0 then e3>e2
 * (0 and 15: none; the saddles 5 and 10 always cut their two solid corners off separately).  An
 * endpoint lies on its edge, interpolated from the edge's lower sample a to its higher sample b:
 * mu = (0.f - a) / (b - a); on an x-edge at (i, j) x = xs[i] + mu * (xs[i + 1] - xs[i]), y = ys[j]; on a
 * y-edge x = xs[i], y = ys[j] + mu * (ys[j + 1] - ys[j]); every operation rounded to float on its own.
 * Where a or b is not finite the endpoint is what these formulas give under IEEE arithmetic, with no special
 * case: a NaN mu (a or b NaN, or both infinite) gives a NaN coordinate, a finite a beside an infinite b gives
 * mu = +-0 and the lower sample's coordinate.  The keys do not depend on mu, so such contours still chain.
 * Both cells that share an edge compute the same bits, so a contour's segments chain by key.
 * Order: by layer, then by tile of 16 x 16 cells row-major (ty, tx), then by cell row-major inside
 * the tile (j, i), then the table's order.  The tile size is part of the interface.
 *   returns        S, the number of segments, or -1 with implisolid_last_error(): a bad rect,
 *                  resolution, n_layers or z, an unsupported node, or a total that reaches 2^31
 *   layer_offsets  n_layers + 1 entries: layer l's segments are [layer_offsets[l], layer_offsets[l + 1])
 *   stats          (may be NULL) [(layer, tile) pairs, tiles evaluated, samples evaluated, chunks]
 * The result stays in one library-owned slot, in host memory, until the next implisolid_slice call:
 *   slice_copy     copies it: xy = 4 S floats {x_start, y_start, x_end, y_end}, keys = 2 S words
 *                  {start key, end key}; 0, or -1 when there is no result
 * At implisolid_set_pruning level >= 1 each (layer, tile) is first bounded by the interval evaluator
 * over the box of its end samples and {z, z}: a tile that is all solid or all empty is skipped, the
 * others evaluate their samples with the bound's modes word (bit-identical values); at level 0 every
 * tile is evaluated.  Only the work differs.  Layers are processed in chunks of at most
 * IMPLISOLID_SLICE_CHUNK tiles (environment, read at each call; default and maximum 2^20, at least one
 * layer's tiles), which bounds the device scratch. */
int64_t implisolid_slice(const char* shape_json, int ignore_root_matrix, const float rect[4], int resolution,
                         const float* z, int n_layers, int64_t* layer_offsets, int64_t stats[4]);
int implisolid_slice_copy(float* xy, uint32_t* keys);
/* host only (no GPU): the sample coordinates, R + 1 floats each.  xs[i] = xmin + (float)i * ((xmax -
 * xmin) / (float)R) for i < R, every operation rounded to float on its own, xs[R] = xmax; ys likewise.
 * 0, or -1 (resolution, rect) */
int implisolid_slice_coords(const float rect[4], int resolution, float* xs, float* ys);
/* host only: chains ONE layer's keys (pass the layer's sub-array, 2 n_segments words) into polylines
 * by exact key matching.  order (n_segments entries) is a permutation of the segment indices in which
 * each polyline's segments are consecutive and every segment's end key is the next one's start key;
 * polyline p is order[loop_offsets[p] .. loop_offsets[p + 1]) and closed[p] says whether its last
 * segment ends where its first starts (loop_offsets: n_segments + 1 entries, closed: n_segments).
 * Open chains come first: each starts at a key no segment ends on (the contour meets the rect there),
 * in the order of their first segments.  Closed loops follow, each from its lowest-indexed segment, in
 * the order of those.  Returns the number of polylines, or -1 if a key starts two segments or ends
 * two (implisolid_slice never produces that). */
int64_t implisolid_slice_loops(const uint32_t* keys, int64_t n_segments, int64_t* order, int64_t* loop_offsets,
                               uint8_t* closed);

/* Additive: volume, centre of mass and inertia of the solid inside a box, integrated on the GPU over
 * the solid itself (no mesh, no reference counterpart).
 *   box    {xmin, xmax, ymin, ymax, zmin, zmax}, finite with min < max
 *   depth  in [3, 10]: N = 2^depth cells per axis; the cell edges are exactly those of
 *          implisolid_bounds_edges(box, depth)
 * The sample point of cell k on an axis is mid[k] = edge[k] + 0.5f * (edge[k + 1] - edge[k]), every
 * operation rounded to float on its own (implisolid_mass_mids: computed once on the host and uploaded,
 * the kernels only index the table; the host refuses a box for which some edge[k] <= mid[k] <=
 * edge[k + 1] fails, so a cell's sample lies inside every interval box that contains the cell).
 * Cell (i, j, k) is solid iff !(F < 0), F being implisolid_eval_points' value at (midx[i], midy[j],
 * midz[k]): marching cubes' rule, -0.0 and NaN are solid.  The result is ten unsigned 64-bit sums over
 * the solid cells,
 *   moments = [n, sum i, sum j, sum k, sum i^2, sum j^2, sum k^2, sum i j, sum j k, sum i k],
 * and layer_cells[k] (N entries, may be NULL) = the solid cells with z index k; their sum is n.  All are
 * integers: they do not depend on the order of summation, the pruning level or the list sizes (at
 * depth 10 the largest is about 3.6e14).
 *   returns 1 when n > 0, 0 when the box holds no solid cell, -1 with implisolid_last_error() for a
 *           depth outside [3, 10], a box side that is not finite with min < max (nothing is
 *           launched), or an unsupported node
 *   stats   (may be NULL) [boxes bounded by the interval evaluator, cells counted whole from boxes
 *           the bound proved solid, samples evaluated, reruns after a list overflowed]
 * At implisolid_set_pruning level >= 1 the boxes of level min(3, depth - 2) (2^level per axis, modes
 * word 0) are bounded over their edge extent; an outside box (hi < 0) is dropped, a solid one
 * (lo >= 0) adds the closed-form sums of its index range, a mixed one (a NaN bound included) is cut
 * into its eight children, which are bounded with its modes word, down to level depth - 2, whose
 * mixed boxes (4 x 4 x 4 cells) are evaluated sample by sample with their modes word (bit-identical
 * values).  At level 0 nothing is bounded and every sample is evaluated.  Only the work differs.  One
 * device, the interpreter kernels; the lists start at IMPLISOLID_MASS_LIST boxes (environment, read at
 * each call; default and clamp as IMPLISOLID_BOUNDS_LIST) and grow when a level overflows them, after
 * which everything runs again. */
int implisolid_mass(const char* shape_json, int ignore_root_matrix, const float box[6], int depth, uint64_t moments[10],
                    int64_t* layer_cells, int64_t stats[4]);
/* host only (no GPU): the sample table, 3 N floats, rows x, y, z.  0, or -1 (depth, box, or a sample
 * that left its cell) */
int implisolid_mass_mids(const float box[6], int depth, float* mids);
/* host only: the physical quantities of the union of the solid cells as cuboids, unit density, in
 * double from the integers and the box: out = [volume, cx, cy, cz, Ixx, Iyy, Izz, Ixy, Iyz, Ixz], the
 * inertia about the centre of mass.  Per axis d_a = ((double)hi_a - (double)lo_a) / N;
 *   cell = (dx * dy) * dz, volume = (double)n * cell,
 *   centre_a = lo_a + ((double)S_a / (double)n + 0.5) * d_a,
 *   c_ab = n S_ab - S_a S_b exactly, in a signed 128-bit integer (a cross term can be negative), converted
 *   to double once, mu_ab = ((volume * d_a) * d_b) * ((double)c_ab / ((double)n * (double)n) +
 *   (a == b ? 1.0 / 12.0 : 0.0)),
 *   Ixx = mu_yy + mu_zz, Iyy = mu_xx + mu_zz, Izz = mu_xx + mu_yy, Ixy = -mu_xy, Iyz = -mu_yz,
 *   Ixz = -mu_xz (no fused multiply-add).  The area of layer k is layer_cells[k] * dx * dy.
 * Returns 1, 0 with out all zero when n == 0 ("empty"), -1 (depth, box) */
int implisolid_mass_physical(const float box[6], int depth, const uint64_t moments[10], double out[10]);

/* Additive: the solid's layers as coverage images on the GPU, what a masked-resin printer exposes (no
 * reference counterpart).
 *   rect        {xmin, xmax, ymin, ymax}, finite with min < max
 *   width, height  W, H in [1, 16384] pixels
 *   supersample    s in {1, 2, 4}: sub-samples per axis per pixel
 *   z           n_layers in [1, 65536] finite plane heights, in the caller's order (they may repeat and
 *               need not be sorted)
 * Sub-cell edges: ex[0 .. W s] follows implisolid_slice_coords' formula with W s cells, ex[k] = xmin +
 * (float)k * ((xmax - xmin) / (float)(W s)) for k < W s, every operation rounded to float on its own,
 * ex[W s] = xmax; ey the same with H s.  Samples: mx[k] = ex[k] + 0.5f * (ex[k + 1] - ex[k]), my likewise
 * (implisolid_mass_mids' rule; implisolid_raster_coords: computed once on the host and uploaded, the
 * kernels only index the tables; the host refuses a rect for which some ex[k] <= mx[k] <= ex[k + 1]
 * fails).  Coverage: cov[l][py][px] = the number of (a, b) in [0, s)^2 with !(F < 0), F being
 * implisolid_eval_points' value at (mx[px s + a], my[py s + b], z[l]): marching cubes' rule, -0.0 and
 * NaN are solid.  It is a byte in 0 .. s^2; row py = 0 is the row at ymin (y up).  layer_sum[l] = the
 * sum of cov[l] (n_layers entries); the layer's area is layer_sum * pixel area / s^2.  Everything is an
 * integer: no result depends on the pruning level, the order of the tile lists or of the atomics, or
 * the chunking.  With W = H = 2^depth and s = 1 on a box's x, y sides and z = implisolid_mass_mids' z
 * row, layer_sum equals implisolid_mass' layer_cells.
 *   cov      the caller's host buffer of n_layers * H * W bytes, rows tightly packed, written chunk by
 *            chunk (there is no library-owned result slot); may be NULL: only sums and stats
 *   stats    (may be NULL) [(layer, tile) pairs, tiles evaluated, tiles filled whole, samples
 *            evaluated, chunks]
 *   returns  0, or -1 with implisolid_last_error(): a bad rect, width, height, supersample, n_layers
 *            or z, or an unsupported node; all checked before anything is launched
 * Tiles are 16 x 16 pixels.  At implisolid_set_pruning level >= 1 each (layer, tile) is first bounded by
 * the interval evaluator over the box of its first and last samples and {z, z}: an outside tile is
 * left zero, a solid one (lo >= 0) is filled with s^2 without evaluating a sample, the others (a NaN
 * bound included) evaluate their samples with the bound's modes word (bit-identical values); at
 * level 0 every tile is evaluated.  Only the work differs.  Layers are processed in chunks of whole
 * layers of at most IMPLISOLID_RASTER_CHUNK (layer, tile) pairs (environment, read at each call;
 * default and maximum 2^20, at least one layer's tiles), which bounds the device image and the two
 * pinned staging slots the chunks pass through.  One device, the interpreter kernels. */
int implisolid_raster(const char* shape_json, int ignore_root_matrix, const float rect[4], int width, int height,
                      int supersample, const float* z, int n_layers, uint8_t* cov, int64_t* layer_sum, int64_t stats[5]);
/* host only (no GPU): the sample tables, mx = W s floats, my = H s floats.  0, or -1 (width, height,
 * supersample, rect, or a sample that left its sub-cell) */
int implisolid_raster_coords(const float rect[4], int width, int height, int supersample, float* mx, float* my);

/* Additive: the islands of the layers on the GPU -- the connected regions of every layer image and how
 * much of each rests on the layer below, what a resin slicer looks for first (no reference counterpart).
 * Arguments, limits and refusals are implisolid_raster's: shape_json, ignore_root_matrix, rect, width,
 * height, supersample s in {1, 2, 4}, z, n_layers; further
 *   threshold     in [1, s^2]
 *   connectivity  4 or 8
 * cov[l][py][px] is exactly implisolid_raster's: the same sample tables, the same rule !(F < 0), -0.0 and
 * NaN solid.  A pixel is solid iff cov >= threshold.  Two solid pixels of one layer are adjacent if they
 * differ by one step in x or in y (connectivity 4), or by at most one step in each (connectivity 8);
 * adjacency holds inside the image only.  A component is a class of the transitive closure of adjacency.
 * Layers are taken in the caller's order: the layer "below" layer l is entry l - 1 of z, whatever the
 * heights are (repeated and unsorted planes are legal, as for implisolid_raster).
 * One record per component, eight int32 {seed, area, below, x0, y0, x1, y1, layer}:
 *   seed            the smallest py * W + px among the component's pixels
 *   area            its pixel count
 *   below           the number of its pixels that are solid at the same (px, py) in layer l - 1; for l = 0
 *                   (on the build plate) below = area
 *   x0, y0, x1, y1  the inclusive pixel bounding box
 * An island is a component with below == 0.
 *   comp_offsets  n_layers + 1 entries: layer l's records are [comp_offsets[l], comp_offsets[l + 1]), in
 *                 increasing seed
 *   labels        (may be NULL: none) int32 [n_layers][H][W], the caller's host buffer: the pixel's component
 *                 seed, or -1 where the pixel is not solid
 *   stats         (may be NULL) implisolid_raster's five figures, then the components, the islands and the
 *                 solid pixels
 *   returns       the total number of components C, or -1 with implisolid_last_error(): implisolid_raster's
 *                 refusals, a bad threshold or connectivity, or 2^31 components or more; bad input is refused
 *                 before anything is compiled or reaches a device
 * The records stay in one library-owned host slot until the next implisolid_islands call; a failed call
 * empties the slot.  implisolid_islands_copy copies them out (8 C int32): 0, or -1 when there is nothing to
 * copy or comps is NULL with C > 0.
 * Everything is an integer: no result depends on the pruning level, the chunking, the order in which atomics
 * land or the launch geometry.  The image never leaves the device: per chunk only the records
 * come down, and the labels when asked for.  Layers are processed in chunks of whole layers of at most
 * IMPLISOLID_ISLANDS_CHUNK (layer, 16 x 16 tile) pairs (environment, read at each call; default and maximum
 * 2^18, at least one layer's tiles): 2^26 pixels, a 64 MiB image and a 256 MiB label array.  One device, the
 * interpreter kernels. */
int64_t implisolid_islands(const char* shape_json, int ignore_root_matrix, const float rect[4], int width, int height,
                           int supersample, const float* z, int n_layers, int threshold, int connectivity,
                           int64_t* comp_offsets, int32_t* labels, int64_t stats[8]);
int implisolid_islands_copy(int32_t* comps);
/* diagnostics: with enable != 0 the following implisolid_islands calls time their kernels with HIP events;
 * ms (may be NULL) = the last timed call's {raster passes, tile pass, merge pass, seed rows and scan, records
 * and tally} milliseconds summed over its chunks, -1 before any.  Returns 0 */
int implisolid_debug_islands_ms(int enable, double ms[5]);

/* Additive: the pixel distance field of the layers on the GPU -- the exact squared Euclidean distance
 * transform of every layer image, what XY compensation, wall thickness and overhang checks threshold (no
 * reference counterpart).  Arguments, limits and refusals are implisolid_islands': shape_json,
 * ignore_root_matrix, rect, width, height in [1, 16384], supersample s in {1, 2, 4}, z, n_layers, threshold
 * in [1, s^2]; further
 *   reach2        in [0, 2^30): the squared self-supporting reach, in pixels
 * cov[l][py][px] is exactly implisolid_raster's.  A pixel is solid iff cov >= threshold.  Only the pixels of
 * the image exist: there is no implicit border of either class.
 * For pixel p of layer l let O be the pixels of layer l whose solidity differs from p's:
 *   D2(p) = min over q in O of (px - qx)^2 + (py - qy)^2, and NONE = 2^30 when O is empty (the largest real
 *           value, 2 * 16383^2, is below it)
 *   dist[l][py][px] = +D2 for a solid pixel, -D2 for an empty one
 * so dist is never 0, dist > 0 is exactly the solid mask and |dist| >= 1.
 *   dist       (may be NULL: only the records come down) int32 [n_layers][H][W], the caller's host buffer
 *   layer_rec  four int64 per layer {solid, widest, widest_at, unsupported}:
 *     solid        the layer's solid pixels
 *     widest       the largest D2 over the solid pixels: 0 when there are none, NONE for an all-solid layer;
 *                  the squared radius, in pixels, of the largest inscribed disc, up to pixel sampling
 *     widest_at    the smallest py * W + px that attains it, -1 when there is none
 *     unsupported  for l >= 1 the solid pixels of layer l with dist[l - 1] < -reach2 at the same (px, py): the
 *                  pixel is empty below and no solid pixel of the layer below lies within sqrt(reach2)
 *                  pixels; 0 for l = 0.  "Below" is entry l - 1 of z, as for implisolid_islands; an empty
 *                  layer below makes every solid pixel unsupported.  reach2 = 0 counts the pixels with
 *                  nothing straight below
 *   stats      (may be NULL) implisolid_raster's five figures, then the solid pixels, the unsupported pixels
 *              and the layers whose widest is NONE
 *   returns    0, or -1 with implisolid_last_error(): implisolid_raster's refusals, a bad threshold or reach2,
 *              or layer_rec NULL; bad input is refused before anything is compiled or reaches a device
 * There is no library-owned slot.  Everything is an integer: no result depends on the pruning level, the
 * chunking, the order in which atomics land or the launch geometry.  The image never leaves the device.
 * Layers are processed in chunks of whole layers of at most IMPLISOLID_DISTANCE_CHUNK (layer, 16 x 16 tile)
 * pairs (environment, read at each call; default and maximum 2^18, at least one layer's tiles): 2^26 pixels,
 * a 64 MiB image and a 256 MiB distance array; the last distance layer of a chunk stays on the device for the
 * first layer of the next.  One device, the interpreter kernels. */
int implisolid_layer_distance(const char* shape_json, int ignore_root_matrix, const float rect[4], int width, int height,
                              int supersample, const float* z, int n_layers, int threshold, int64_t reach2,
                              int32_t* dist, int64_t* layer_rec, int64_t stats[8]);
/* diagnostics: with enable != 0 the following implisolid_layer_distance calls time their kernels with HIP
 * events; ms (may be NULL) = the last timed call's {raster passes, column pass, row pass and records}
 * milliseconds summed over its chunks, -1 before any.  Returns 0 */
int implisolid_debug_layer_distance_ms(int enable, double ms[3]);

/* Additive: the layer stack hollowed to a shell of a given wall on the GPU -- the exact 3D erosion of the solid
 * voxels by a structuring element given layer by layer, what a resin slicer's hollowing does, without a mesh and
 * without downloading a distance field (no reference counterpart).  Arguments, limits, refusals and their order
 * are implisolid_layer_distance's: shape_json, ignore_root_matrix, rect, width, height in [1, 16384], supersample
 * s in {1, 2, 4}, z, n_layers, threshold in [1, s^2]; further, refused in this order,
 *   reach         in [0, 1024]: the layers on either side that a voxel looks at.  (2 reach + 1) times the 16 x 16
 *                 tiles of a layer must not exceed 2^20: the window of layers a voxel looks at stays on the device
 *   wall2         required, reach + 1 entries, each in [0, 2^30), non-increasing: wall2[j] is the squared in-plane
 *                 radius, in pixels, of the structuring element at a layer offset of +-j.  The library knows no z
 *                 metric: layers are neighbours by their position in z, as everywhere else (repeated and unsorted
 *                 planes are legal); implisolid_hollow_wall2 makes the table of an ellipsoid from a wall and a
 *                 layer pitch in pixels
 *   ends          in {0, 1, 2, 3}.  Bit 0: the layers in front of entry 0 of z count as empty, so a skin of the
 *                 wall's thickness forms on the build plate; bit 1: the layers behind the last entry count as
 *                 empty.  A clear bit means those layers do not exist, and the shell stays open there
 * cov[l][py][px] is exactly implisolid_raster's and dist[l][py][px] exactly implisolid_layer_distance's.  A voxel
 * (l, py, px) is solid iff cov >= threshold.  Only the pixels of the image exist in the plane.  A voxel is core
 * iff for every j in [-reach, reach], with m = l + j,
 *   0 <= m < n_layers   dist[m][py][px] > wall2[|j|]
 *   m < 0               bit 0 of ends is clear
 *   m >= n_layers       bit 1 of ends is clear
 * Equivalently: no empty voxel (m, qy, qx), the virtual empty layers of ends included, has |m - l| <= reach and
 * (qx - px)^2 + (qy - py)^2 <= wall2[|m - l|].  j = 0 makes every core voxel solid, at a squared distance of more
 * than wall2[0] from every empty pixel of its own layer.  A layer of one class has dist = +-NONE (2^30): an
 * all-solid layer passes every threshold and an empty one fails every one.  Because only the image's pixels
 * exist, a rect without an empty margin around the solid leaves no skin at the image's sides: the solid is cut
 * open there, exactly as dist sees no other class beyond the border.
 *   out        (may be NULL: only the records come down) uint8 [n_layers][H][W], the caller's host buffer: 0 for
 *              a core voxel, cov for every other.  The shell keeps its grey levels: out is the printable image
 *   layer_rec  required, two int64 per layer {solid, core}: the layer's solid voxels and its core voxels
 *   stats      (may be NULL) implisolid_raster's five figures, then the solid voxels, the core voxels and the
 *              number of layers whose distance transform was computed (n_layers: none is computed twice)
 *   returns    0, or -1 with implisolid_last_error(): implisolid_layer_distance's refusals, a bad reach, wall2 or
 *              ends, or wall2 or layer_rec NULL; bad input is refused before anything is compiled or reaches a
 *              device, and a refused call writes nothing
 * There is no library-owned slot.  Everything is an integer: no result depends on the pruning level, the
 * chunking, the order in which atomics land or the launch geometry; before returning the library checks core <=
 * solid for every layer and the solid counts against the distance pass's.  Neither the images nor the distance
 * fields leave the device.  Layers stream through in chunks of whole layers of at most IMPLISOLID_HOLLOW_CHUNK
 * (layer, 16 x 16 tile) pairs (environment, read at each call; default and maximum 2^18, at least one layer's
 * tiles).  A layer's output needs the layers up to reach ahead, so output lags input by reach layers: a ring of
 * chunk + 2 reach distance layers (4 bytes a pixel) and as many image layers is carried on the device between
 * chunks, and no layer is rastered or transformed twice.  One device, the interpreter kernels. */
int implisolid_layer_hollow(const char* shape_json, int ignore_root_matrix, const float rect[4], int width, int height,
                            int supersample, const float* z, int n_layers, int threshold,
                            const int64_t* wall2, int reach, int ends,
                            uint8_t* out, int64_t* layer_rec, int64_t stats[8]);
/* host only, no GPU: the table of the digital ellipsoid with in-plane radius wall_px pixels over layers pitch_px
 * pixels apart.  Returns R, the largest j >= 0 with (j pitch) (j pitch) <= wall wall, and fills wall2[j] = (int64)
 * floor(wall wall - (j pitch) (j pitch)) for j <= R; the arithmetic is in doubles, each product and the
 * difference rounded on its own, no fused multiply-add.  (3, 1) gives {9, 8, 5, 0}, (2.5, 2) gives {6, 2}.
 * Returns -1 with implisolid_last_error(), nothing written, for a non-finite or negative wall, a non-finite
 * pitch or pitch <= 0, wall wall >= 2^30, R > 1024, or R + 1 > cap (wall2 NULL counts as cap 0) */
int implisolid_hollow_wall2(double wall_px, double pitch_px, int64_t* wall2, int cap);
/* diagnostics: with enable != 0 the following implisolid_layer_hollow calls time their kernels with HIP events;
 * ms (may be NULL) = the last timed call's {raster passes, copy into the ring and column pass, row pass, window
 * pass} milliseconds summed over its chunks, -1 before any.  Returns 0 */
int implisolid_debug_layer_hollow_ms(int enable, double ms[4]);

/* Additive: support tips under the layer stack on the GPU -- where a resin slicer's supports touch the model and
 * where each support's column lands, without downloading a distance field (no reference counterpart).  One tip per
 * non-empty cell of a square grid laid over each layer's unsupported pixels.  Arguments, limits, refusals and their
 * order are implisolid_layer_distance's: shape_json, ignore_root_matrix, rect, width, height in [1, 16384],
 * supersample s in {1, 2, 4}, z, n_layers, threshold in [1, s^2], reach2 in [0, 2^30); shape_json, rect or z NULL
 * is refused first.  Further, refused in this order,
 *   cell          in [1, 16384]: the side of the placement grid in pixels
 *   tip_offsets   required, n_layers + 1 int64
 *   layer_rec     required, two int64 per layer
 * cov[l][py][px] is exactly implisolid_raster's and dist[l][py][px] exactly implisolid_layer_distance's.
 * Unsupported pixels: for l >= 1, U_l = { p : dist[l][p] > 0 and dist[l - 1][p] < -reach2 }; U_0 is empty, layer 0
 * rests on the plate.  This is implisolid_layer_distance's unsupported, pixel for pixel.  "Below" is entry l - 1 of
 * z, as everywhere else: repeated and unsorted planes are legal.
 * Cells: ncx = ceil(W / cell), ncy = ceil(H / cell); the cell of p = (px, py) is c = (py / cell) ncx + px / cell
 * (integer divisions).  The last cells of a row or column may be partial; a cell larger than both sides gives one.
 * Tips: every (l, c) with a pixel of U_l in c yields one tip, the pixel of U_l in c with the largest dist[l][p]
 * -- the pixel deepest inside its own layer, on an island's first layer its middle and not its rim --, among equals
 * the smallest p = py W + px.
 *   tips        (implisolid_layer_supports_copy) four int32 per tip {p, depth, foot, load}:
 *     p           the tip's pixel, py W + px
 *     depth       dist[l][p], which may be NONE = 2^30
 *     foot        the largest m < l with cov[m][p] >= threshold: the layer of the model the support's column
 *                 stands on; -1 when there is none and the column reaches the plate.  Layer l - 1 is empty at p
 *                 (that made p unsupported): foot <= l - 2
 *     load        the pixels of U_l in the cell: the unsupported pixels this tip stands for
 *                 in order of layer, and within a layer of increasing c
 *   tip_offsets layer l's tips are [tip_offsets[l], tip_offsets[l + 1])
 *   layer_rec   per layer {unsupported = |U_l|, tips}
 *   stats       (may be NULL) implisolid_raster's five figures, then the unsupported pixels, the tips and the tips
 *               with foot == -1
 *   returns     the number of tips, or -1 with implisolid_last_error(): the refusals above, or 2^31 tips or more
 *               (found at run time); bad input is refused before anything is compiled or reaches a device, and a
 *               refused call writes nothing
 * cell = 1 lists the unsupported pixels themselves, each with its foot: the compact form of the overhang mask.
 * The tips stay in a library-owned slot until the next implisolid_layer_supports call, which empties it whether it
 * succeeds or not; implisolid_layer_supports_copy copies them out (tips may be NULL when there are none) and
 * returns 0, or -1 when there is no result.  Everything is an integer: no result depends on the pruning level, the
 * chunking, the order in which atomics land or the launch geometry; before returning the library checks that every
 * layer's loads add up to its unsupported pixels, tips <= unsupported <= solid, and that every tip lies in the
 * cell whose turn it is.  Neither the images nor the distance fields leave the device.  Layers go through in
 * chunks of whole layers of at most IMPLISOLID_SUPPORTS_CHUNK (layer, 16 x 16 tile) pairs (environment, read at
 * each call; default and maximum 2^18, at least one layer's tiles).  Device memory besides the image: 4 bytes a
 * pixel of a chunk plus one carried layer for the distances; 12 bytes per cell of a chunk for the table of keys
 * and loads, and 8 for its counts and offsets; where there is more than one chunk, 4 bytes a pixel for `top`,
 * the highest solid layer of every pixel in front of the chunk, from which the feet below a chunk are read.
 * One device, the interpreter kernels. */
int64_t implisolid_layer_supports(const char* shape_json, int ignore_root_matrix, const float rect[4], int width, int height,
                                  int supersample, const float* z, int n_layers, int threshold, int64_t reach2, int cell,
                                  int64_t* tip_offsets, int64_t* layer_rec, int64_t stats[8]);
int implisolid_layer_supports_copy(int32_t* tips);
/* diagnostics: with enable != 0 the following implisolid_layer_supports calls time their kernels with HIP events;
 * ms (may be NULL) = the last timed call's {raster passes, column and row passes, cell pass, count, scan, emit
 * and top passes} milliseconds summed over its chunks, -1 before any.  Returns 0 */
int implisolid_debug_layer_supports_ms(int enable, double ms[4]);

/* Additive: the layer images as run-length streams on the GPU -- what a resin printer's file formats store
 * and what a slicer finally hands over, without downloading a pixel (no reference counterpart).  Arguments,
 * limits and refusals are implisolid_raster's, in the same order: shape_json, ignore_root_matrix, rect, width,
 * height in [1, 16384], supersample s in {1, 2, 4}, z, n_layers; further
 *   threshold     0, or in [1, s^2]; anything else is refused
 * cov[l][py][px] is exactly implisolid_raster's: the same sample tables, the same rule !(F < 0), -0.0 and NaN
 * solid.  The pixel's value v is
 *   threshold == 0        the grey mode: v = cov, a byte in 0 .. s^2
 *   threshold in [1, s^2] the binary mode: v = (cov >= threshold) ? 1 : 0
 * A layer is the stream of its W H pixels in row-major order, p = py * W + px for p in [0, W H): the W pixels of
 * row 0 (the row at ymin), then those of row 1, and so on; nothing stands between a row's last pixel and the
 * next row's first.  A run starts at p = 0 and at every p > 0 with v[p] != v[p - 1]; it ends in front of the
 * next start, or at W H.  Runs therefore cross row ends (the pixel before (0, py) is (W - 1, py - 1)), runs of
 * value 0 are listed like any other, the runs partition the layer, and every layer has at least one run.  Runs
 * never cross layers.  Layers are taken in the caller's order (repeated and unsorted planes are legal).
 * One record per run:
 *   start   uint32, the run's first p (W H <= 2^28)
 *   value   uint8, its v
 * in increasing start.  A run's length is the next run's start minus its own, or W H - start for the last run
 * of its layer.
 *   run_offsets  n_layers + 1 entries: layer l's runs are [run_offsets[l], run_offsets[l + 1])
 *   layer_sum    implisolid_raster's: the sum of cov[l] (n_layers entries; required).  In the grey mode it
 *                equals the sum of value * length over the layer's runs
 *   stats        (may be NULL) implisolid_raster's five figures, then the runs and the runs with value != 0
 *   returns      the total number of runs, or -1 with implisolid_last_error(): implisolid_raster's refusals, a
 *                bad threshold, run_offsets or layer_sum NULL, or 2^31 runs or more; bad input is refused
 *                before anything is compiled or reaches a device
 * The runs stay in one library-owned host slot until the next implisolid_layer_runs call; a failed call empties
 * the slot.  implisolid_layer_runs_copy copies them out (start: that many uint32, value: that many bytes): 0,
 * or -1 when there is nothing to copy or a pointer is NULL.
 * Everything is an integer: no result depends on the pruning level, the chunking or the launch geometry, and
 * there is no atomic on the way from the image to the runs.  The image never leaves the device: per chunk only
 * the runs come down, through two pinned staging slots; before returning the library checks that every layer's
 * first start is 0, that its starts increase strictly below W H and, in the grey mode, that the runs add up to
 * layer_sum.  Layers are processed in chunks of whole layers of at most IMPLISOLID_RUNS_CHUNK (layer, 16 x 16
 * tile) pairs (environment, read at each call; default and maximum 2^20, at least one layer's tiles): 2^28
 * pixels, a 256 MiB image, and 5 bytes of device and staging memory per run of the chunk.  One device, the
 * interpreter kernels. */
int64_t implisolid_layer_runs(const char* shape_json, int ignore_root_matrix, const float rect[4], int width, int height,
                              int supersample, const float* z, int n_layers, int threshold, int64_t* run_offsets,
                              int64_t* layer_sum, int64_t stats[7]);
int implisolid_layer_runs_copy(uint32_t* start, uint8_t* value);
/* diagnostics: with enable != 0 the following implisolid_layer_runs calls time their kernels with HIP events;
 * ms (may be NULL) = the last timed call's {raster passes, count pass and scan, emit pass} milliseconds summed
 * over its chunks, -1 before any.  Returns 0 */
int implisolid_debug_layer_runs_ms(int enable, double ms[3]);

/* Additive: the bodies of the layer stack on the GPU -- the connected components of the voxels through the
 * whole stack: whether the solid is one piece, which parts float, and which empty regions are sealed on all
 * sides and would trap resin (no reference counterpart).  Arguments, limits, refusals and their order are
 * implisolid_islands': shape_json, ignore_root_matrix, rect, width, height in [1, 16384], supersample s in
 * {1, 2, 4}, z, n_layers, threshold in [1, s^2]; further
 *   target        1: the solid voxels (cov >= threshold); 0: the empty ones (cov < threshold); anything else is
 *                 refused
 *   connectivity  6 or 26; anything else is refused
 *   want_runs     0 or 1; anything else is refused
 * cov[l][py][px] is exactly implisolid_raster's.  A voxel is (l, py, px), l being the position in the caller's z
 * list: the neighbours of layer l are entries l - 1 and l + 1 of z, whatever the heights are (repeated and
 * unsorted planes are legal, as everywhere else).  Two target voxels are adjacent if they differ by one step in
 * exactly one of px, py, l (connectivity 6), or by at most one step in each and are not equal (connectivity
 * 26).  Adjacency holds inside the stack only: there is no implicit border of either class.  A body is a class
 * of the transitive closure of adjacency.  Restricted to one layer, connectivity 6 is implisolid_islands' 4 and
 * connectivity 26 its 8.
 * The key of a voxel is l * W * H + py * W + px, an int64.  One record per body, eight int64 {seed, volume, x0,
 * y0, l0, x1, y1, l1}:
 *   seed                     the smallest key among the body's voxels: the seed lies in layer l0
 *   volume                   its voxel count
 *   x0, y0, l0, x1, y1, l1   the inclusive bounding box
 * in increasing seed.  With target 0 a body that touches no face of the stack (x0 > 0, y0 > 0, l0 > 0, x1 < W -
 * 1, y1 < H - 1, l1 < n_layers - 1) is an enclosed void; with target 1 a body with l0 > 0 starts in mid-air.
 * The row runs are the compact form of the label image: a row run is a maximal sequence of target voxels
 * within one image row, so row runs never cross a row end (unlike implisolid_layer_runs' stream runs).  With
 * want_runs one record per row run is kept, three int32 {start = py * W + x0, length, body}, body being the
 * index of its body's record; the runs come layer by layer, within a layer in increasing start.
 *   run_offsets  n_layers + 1 entries, required, always filled: layer l's row runs are [run_offsets[l],
 *                run_offsets[l + 1])
 *   stats        (may be NULL) implisolid_raster's five figures, then the row runs, the bodies and the target
 *                voxels
 *   returns      the number of bodies B, or -1 with implisolid_last_error(): implisolid_raster's refusals, a bad
 *                threshold, target, connectivity or want_runs, or run_offsets NULL -- all refused before
 *                anything is compiled or reaches a device --, or at run time a stack that reaches 2^31 row runs
 *                or 2^31 bodies
 * The records, and the runs when asked for, stay in one library-owned host slot until the next
 * implisolid_layer_bodies call; a failed call empties the slot.  implisolid_layer_bodies_copy copies them out
 * (bodies: 8 B int64; runs: 3 int32 per row run, may be NULL when the call did not ask for runs): 0, or -1 when
 * there is nothing to copy or a needed pointer is NULL.
 * Everything is an integer: no result depends on the pruning level, the chunking, the order in which atomics
 * land or the launch geometry; before returning the library checks that the volumes add up to the target voxels
 * counted from the images.  The labelling is a union-find over the row runs of the whole stack, not a voxel
 * array: the image never leaves the device, the only per-pixel memory is a chunk's image, and the stack-wide
 * device memory is 16 bytes per row run (28 with want_runs), 12 per image row and 64 per body.  Layers are
 * processed in chunks of whole layers of at most IMPLISOLID_BODIES_CHUNK (layer, 16 x 16 tile) pairs
 * (environment, read at each call; default and maximum 2^20, at least one layer's tiles): 2^28 pixels, a 256 MiB
 * image; no image is carried between chunks.  One device, the interpreter kernels. */
int64_t implisolid_layer_bodies(const char* shape_json, int ignore_root_matrix, const float rect[4], int width, int height,
                                int supersample, const float* z, int n_layers, int threshold, int target, int connectivity,
                                int want_runs, int64_t* run_offsets, int64_t stats[8]);
int implisolid_layer_bodies_copy(int64_t* bodies, int32_t* runs);
/* diagnostics: with enable != 0 the following implisolid_layer_bodies calls time their kernels with HIP events;
 * ms (may be NULL) = the last timed call's {raster passes, row-run count + scan + emit, link, finish}
 * milliseconds summed over its chunks, -1 before any.  Returns 0 */
int implisolid_debug_layer_bodies_ms(int enable, double ms[4]);

/* Additive: the suction cups of the layer stack on the GPU -- per layer the empty regions that seal against the
 * film when that layer is cured, because their pocket has no way out through the part as printed so far (no
 * reference counterpart).  Arguments, limits, refusals and their order are implisolid_layer_bodies' without
 * target: shape_json, ignore_root_matrix, rect, width, height in [1, 16384], supersample s in {1, 2, 4}, z,
 * n_layers, threshold in [1, s^2]; further
 *   connectivity  6 or 26, of the empty voxels; anything else is refused.  6 is the dual of 26 for the solid
 *   want_runs     0 or 1; anything else is refused
 * cov[l][py][px] is exactly implisolid_raster's.  A voxel (l, py, px) is empty iff cov[l][py][px] < threshold; l
 * is the position in the caller's z list, and that order is the print order.  Two empty voxels are adjacent as
 * implisolid_layer_bodies' target voxels are.  The prefix P_l is layers 0 .. l.  A frame voxel has px in {0, W -
 * 1} or py in {0, H - 1}.  The plate below layer 0 and the film above layer l are closed: neither is outside (a
 * caller whose model does not start on the plate puts an empty plane first).  A pocket of P_l is a class of the
 * transitive closure of adjacency among the empty voxels of P_l, paths inside P_l only; it is open if it holds a
 * frame voxel and closed otherwise.  A cup of layer l is the set of the layer-l voxels of one closed pocket of P_l
 * that has a voxel in layer l: one record per cup, even where the cup is several separate regions of the layer
 * that join further down.  Seven int64 {seed, area, x0, y0, x1, y1, pocket}:
 *   seed              the smallest py * W + px of the cup's voxels (all in layer l)
 *   area              their count
 *   x0, y0, x1, y1    their inclusive bounding box
 *   pocket            the smallest key l' * W * H + py * W + px of the whole pocket in P_l: pocket / (W * H) is the
 *                     layer where the pocket begins, and the value stays the same from layer to layer until the
 *                     pocket merges with one that has a smaller key
 * layer by layer, in increasing seed within a layer.  With want_runs the row runs of empty voxels (maximal within
 * one image row) that lie in a cup are kept, three int32 {start = py * W + x0, length, cup}, cup being the index
 * of the run's record in the whole array; a run lies in one pocket, so it is cupped whole or not at all.  The runs
 * come layer by layer, within a layer in increasing start.
 *   cup_offsets  n_layers + 1 entries, required, always filled: layer l's cups are [cup_offsets[l],
 *                cup_offsets[l + 1])
 *   run_offsets  n_layers + 1 entries, may be NULL iff want_runs == 0; filled when given: layer l's cupped runs
 *                are [run_offsets[l], run_offsets[l + 1])
 *   stats        (may be NULL) implisolid_raster's five figures, then the empty row runs of the stack, the cups and
 *                the cupped voxels (the sum of area)
 *   returns      the number of cups, or -1 with implisolid_last_error(): implisolid_raster's refusals, a bad
 *                threshold, connectivity or want_runs, or a needed pointer NULL -- all refused before anything is
 *                compiled or reaches a device --, or at run time a stack that reaches 2^31 row runs or 2^31 cups
 * The records, and the runs when asked for, stay in one library-owned host slot until the next
 * implisolid_layer_cups call; a failed call empties the slot.  implisolid_layer_cups_copy copies them out (cups: 7
 * int64 per cup; runs: 3 int32 per cupped run, may be NULL when the call did not ask for runs): 0, or -1 when
 * there is nothing to copy or a needed pointer is NULL.
 * Everything is an integer: no result depends on the pruning level, the chunking, the order in which atomics
 * land or the launch geometry; before returning the library checks that the areas add up to the cupped voxels
 * counted on the device.  The volume of a pocket is left out on purpose.  One union-find over the empty row runs
 * of the whole stack answers every prefix: joins only add up as layers arrive, and the pockets are read off
 * behind each layer's joins.  Stack-wide device memory is 24 bytes per empty row run, 20 per image row, 56 per cup
 * and 12 per cupped run with want_runs; the only per-pixel memory is a chunk's image.  Layers are processed in
 * chunks of whole layers of at most IMPLISOLID_CUPS_CHUNK (layer, 16 x 16 tile) pairs (environment, read at each
 * call; default and maximum 2^20, at least one layer's tiles).  One device, the interpreter kernels. */
int64_t implisolid_layer_cups(const char* shape_json, int ignore_root_matrix, const float rect[4], int width, int height,
                              int supersample, const float* z, int n_layers, int threshold, int connectivity, int want_runs,
                              int64_t* cup_offsets, int64_t* run_offsets, int64_t stats[8]);
int implisolid_layer_cups_copy(int64_t* cups, int32_t* runs);
/* diagnostics: with enable != 0 the following implisolid_layer_cups calls time their kernels with HIP events;
 * ms (may be NULL) = the last timed call's {raster passes, row-run count + scan + emit + frame, the layers' link +
 * mark + head, finish} milliseconds summed over its chunks, -1 before any.  Returns 0 */
int implisolid_debug_layer_cups_ms(int enable, double ms[4]);

/* Additive: rays cast at the solid on the GPU -- per ray the first hit, its distance, the field value
 * and the normal there (no reference counterpart: the reference front end ray-casts the mesh).
 *   origins, dirs  3 n floats each, n in [0, 2^24], every float finite.  A direction need not have unit
 *                  length; an all-zero direction is legal (every sample is then the origin)
 *   t0, t1         finite, t0 < t1
 *   steps          N in [1, 65536]
 *   bisect         B in [0, 32]
 * Sample parameters (implisolid_ray_params: computed once on the host and uploaded, the kernels only
 * index the table): ts[k] = t0 + (float)k * ((t1 - t0) / (float)N) for k < N, every operation rounded to
 * float on its own, ts[N] = t1; N + 1 floats shared by all rays.  The host refuses a range for which ts
 * is not non-decreasing (only ts[N - 1] > t1 can violate it).
 * Points: p(t) = (ox + t * dx, oy + t * dy, oz + t * dz), every operation rounded to float on its own, no
 * fused multiply-add.  F(t) is implisolid_eval_points' value at p(t); a sample is solid iff !(F < 0):
 * marching cubes' rule, -0.0 and NaN are solid.
 * Per ray, with k the smallest index in 0 .. N whose sample ts[k] is solid:
 *   no such k   hit = -1, t = t1, f = 0, normal = (0, 0, 0)
 *   k = 0       (the ray starts inside) hit = 0, t = ts[0], f = F(ts[0]); no bisection
 *   k >= 1      hit = k; from a = ts[k - 1], b = ts[k], fb = F(b), B rounds of m = a + 0.5f * (b - a),
 *               fm = F(m), if !(fm < 0) then b = m, fb = fm, else a = m; then t = b, f = fb: the returned
 *               point is always on the solid side (a round with m == a or m == b ends the rounds: every
 *               later one would repeat it)
 *   normal      (normals != NULL, hit >= 0) exactly implisolid_eval_normals' row at p(t) (mcc2.cpp:852-871):
 *               -g / |g|, and -42 g where |g| <= 0.0001 or is not a number
 *   hit, t, f   n entries each; normals 3 n floats, may be NULL
 *   stats       (may be NULL) [segments = n * ceil(N / 64), segments proved outside and skipped,
 *               segments evaluated -- both counted only up to and including each ray's hit segment --,
 *               rays with hit >= 0, rays with hit == 0, chunks]
 *   returns     0, or -1 with implisolid_last_error(): a bad n, range, steps or bisect, a non-finite origin
 *               or direction, or an unsupported node; all checked before anything is launched.  n = 0
 *               returns 0 without a launch.
 * A ray is cut into segments of 64 steps; segment j spans the samples 64 j .. min(64 j + 64, N), both ends
 * included, so a bracket [ts[k - 1], ts[k]] always lies inside one segment (the hit segment of k >= 1 is
 * (k - 1) / 64, that of k = 0 is 0).  Rounded multiplication and addition are monotone and ts is
 * non-decreasing, so every coordinate of every p(t) with t in the segment -- the bisection's midpoints
 * included -- lies between the coordinates of the segment's two end points.  At implisolid_set_pruning
 * level >= 1 the box of the two end points is bounded by the interval evaluator: hi < 0 proves every
 * sample of the segment outside and the segment is skipped; any other bound (lo >= 0 and NaN bounds
 * included) has the segment's samples, and a bracket found in it, evaluated with the bound's modes word
 * (bit-identical values).  At level 0 nothing is bounded and every sample up to the hit is evaluated.
 * t * d may overflow: origins, directions and ts are finite, p(t) need not be, and F at a point with an
 * infinite coordinate is still implisolid_eval_points' value (NaN, which is solid, wherever a zero matrix
 * entry multiplies the infinity).  A segment with an end point that is not finite is never proved outside:
 * it counts as evaluated, with modes word 0.
 * Segments after the hit segment are not evaluated.  Only the work differs: no result depends on the
 * pruning level, the chunking or the order of any atomic.  Rays are processed in chunks of at most
 * IMPLISOLID_RAY_CHUNK rays (environment, read at each call; default and maximum 2^20, minimum 1), which
 * bounds the device scratch.  One device, the interpreter kernels. */
int implisolid_raycast(const char* shape_json, int ignore_root_matrix, const float* origins, const float* dirs, int64_t n,
                       float t0, float t1, int steps, int bisect, int32_t* hit, float* t, float* f, float* normals,
                       int64_t stats[6]);
/* host only (no GPU): the sample parameters, steps + 1 floats.  0, or -1 (steps, the range, or a table
 * that is not non-decreasing) */
int implisolid_ray_params(float t0, float t1, int steps, float* ts);
/* diagnostics: with enable != 0 the following implisolid_raycast calls time their two kernels with HIP
 * events (a stream synchronisation per chunk); ms (may be NULL) = the last timed call's {march, finish}
 * milliseconds summed over its chunks, -1 before any.  Returns 0 */
int implisolid_debug_raycast_ms(int enable, double ms[2]);

/* Additive: every solid span along each ray on the GPU -- entries, exits, the field and the normals at
 * both (wall thickness along a direction, X-ray previews, dexels, picking through a part).
 * Arguments, limits and checks are implisolid_raycast's: n in [0, 2^24], finite origins and directions,
 * ts = implisolid_ray_params(t0, t1, steps), bisect B in [0, 32], everything checked before a launch;
 * n = 0 returns 0 without a launch.  p(t), F(t) and "solid iff !(F < 0)" are implisolid_raycast's, points
 * that are not finite included.  Let s[k] be the solidity of sample k, k = 0 .. N.
 * A span is a maximal run of consecutive solid samples k_in .. k_out - 1: k_in in 0 .. N, k_out in
 * 1 .. N + 1, and k_out = N + 1 means that the ray ends inside.  Per span:
 *   entry, k_in == 0      t_in = ts[0], f_in = F(ts[0])
 *   entry otherwise       implisolid_raycast's bisection on [ts[k_in - 1], ts[k_in]]: t_in = b, f_in = fb
 *   exit, k_out == N + 1  t_out = ts[N], f_out = F(ts[N])
 *   exit otherwise        the mirror: a = ts[k_out - 1], fa = F(a), b = ts[k_out]; B rounds of
 *                         m = a + 0.5f * (b - a) (a round with m == a or m == b ends the rounds), fm = F(m),
 *                         if !(fm < 0) then a = m, fa = fm, else b = m; then t_out = a, f_out = fa
 * Both returned ends are solid points and t_in <= t_out.  f_in and f_out are field values, also where a
 * proof (below) made every sample of the segment unnecessary.  Normals (want_normals != 0):
 * implisolid_eval_normals' row at p(t_in) and at p(t_out).
 *   span_offsets  n + 1 entries: ray r's spans are [span_offsets[r], span_offsets[r + 1]), in increasing k_in
 *   stats         (may be NULL) [segments = n * ceil(N / 64), segments proved outside, segments proved
 *                 solid, segments evaluated, spans, rays with at least one span, rays whose first span has
 *                 k_in == 0, chunks].  The whole ray is walked: entries 1 + 2 + 3 equal entry 0.  At
 *                 pruning level 0 entries 1 and 2 are 0
 *   returns       S = span_offsets[n], or -1 with implisolid_last_error() (what implisolid_raycast refuses,
 *                 or a total that reaches 2^31)
 * The result stays in one library-owned host slot until the next implisolid_ray_spans call (a failed one
 * empties it), like implisolid_slice's.
 * At implisolid_set_pruning level >= 1 the box of a segment's two end points is bounded as in
 * implisolid_raycast: hi < 0 proves the segment outside, lo >= 0 proves it solid; in both cases none of its
 * samples is evaluated and it holds no crossing (the box holds every sample of the segment, both end samples
 * included).  Any other bound -- NaN bounds, and every segment with an end point that is not finite (modes
 * word 0) -- has the segment evaluated with the bound's modes word.  Neighbouring segments share their
 * boundary sample, so no crossing falls between segments.  No result depends on the pruning level, the
 * chunking or any atomic's order.
 * Rays go in chunks of at most IMPLISOLID_SPAN_CHUNK rays (environment, read at each call; default and
 * maximum 2^20, minimum 1), cut further so that chunk * ceil(N / 64) stays within 2^23 segment words (64 MiB
 * of device scratch); offsets are global across chunks.  One device, the interpreter kernels. */
int64_t implisolid_ray_spans(const char* shape_json, int ignore_root_matrix, const float* origins, const float* dirs,
                             int64_t n, float t0, float t1, int steps, int bisect, int want_normals,
                             int64_t* span_offsets, int64_t stats[8]);
/* the last implisolid_ray_spans result: k = 2 S ints {k_in, k_out}; t, f = 2 S floats each {in, out};
 * normals = 6 S floats {in, out} x {x, y, z}, or NULL.  Returns 0, or -1: no result, or normals asked for
 * that the call did not compute */
int implisolid_ray_spans_copy(int32_t* k, float* t, float* f, float* normals);
/* diagnostics, as implisolid_debug_raycast_ms: ms (may be NULL) = the last timed call's {march, scan +
 * tally + emit, refine} milliseconds summed over its chunks, -1 before any.  Returns 0 */
int implisolid_debug_ray_spans_ms(int enable, double ms[3]);

/* host-only: compile an MP5 tree to the node program; info = {n_instr, depth, n_mats, 0};
   mats_out receives n_mats inverse matrices (12 floats each, up to 256) */
/* Additive, host only (no GPU): generate and hipRTC-compile the tree kernel for this shape.
 * Returns the code-object size (> 0), or -1 with implisolid_last_error(); optionally copies the
 * generated source (NUL-terminated, truncated to capacity) and the compile time in seconds. */
int64_t implisolid_jit_compile(const char* shape_json, char* source_out, int64_t capacity, double* seconds);
/* the same for the shape's point module (the OB02 passes and direct evaluation over straight-line
 * tree code; used by build_geometry's OB02 steps and implisolid_eval_points once loaded) */
int64_t implisolid_jit_compile_points(const char* shape_json, char* source_out, int64_t capacity, double* seconds);
int implisolid_program_info(const char* shape_json, int ignore_root_matrix, int32_t info[4], float* mats_out);

/* Device-resident slab pipeline (benchmarks / multi-GPU Z-slab runs).  A slab engine owns the
   device buffers of one Z-slab of one object on the current HIP device.  `stream` is a
   hipStream_t (may be NULL).  The launches (eval, count, emit*, copy_*) are stream-ordered and do
   not block; implisolid_slab_counts, _download, _stats* and _kernel_times* block on their stream;
   the setup calls (create*, set_offsets) synchronise the device, since the buffers they reset or
   write may still be read by kernels of an earlier call on another stream. */
typedef struct implisolid_slab implisolid_slab;
implisolid_slab* implisolid_slab_create(const char* shape_json, const char* mc_json, int rank, int nranks);
/* async device-to-device copy of the slab's emitted mesh (nv vertices, nf faces, as counted) into
 * caller-owned device buffers on the slab's device (the multi-process output gather) */
int implisolid_slab_copy_mesh(implisolid_slab* s, float* d_verts, int32_t* d_faces, int64_t nv, int64_t nf, void* stream);
/* the slab of cell layers [z0, z1) (e.g. from implisolid_slab_balance); a halo layer below if z0 > 1 */
implisolid_slab* implisolid_slab_create_range(const char* shape_json, const char* mc_json, int z0, int z1);
void implisolid_slab_destroy(implisolid_slab* s);
int implisolid_slab_eval(implisolid_slab* s, void* stream);            /* field (K1) */
int implisolid_slab_count(implisolid_slab* s, void* stream);           /* counts + scan (K2) */
/* d_offsets: device uint32[2] = this slab's {vertex, face} offset in the global numbering, or NULL
   for the host-set offsets (implisolid_slab_set_offsets, default 0) */
int implisolid_slab_emit(implisolid_slab* s, const uint32_t* d_offsets, void* stream);
/* emit in two halves, so that the count all-gather can overlap the vertex pass: verts needs no
   offsets (slab-local ids); faces takes d_offsets as above, or d_gathered = every rank's
   copy_counts (device uint32[nranks][4], rank order) and this slab's rank, from which it forms
   its vertex offset on the device */
int implisolid_slab_emit_verts(implisolid_slab* s, void* stream);
int implisolid_slab_emit_faces(implisolid_slab* s, const uint32_t* d_offsets, const uint32_t* d_gathered, int rank,
                               void* stream);
/* device uint32[16]: [2] owned verts incl. halo, [3] faces, [4] active cells, [5] halo verts */
const uint32_t* implisolid_slab_counters(implisolid_slab* s);
/* blocking: out[0] = vertices, out[1] = faces of this slab, out[2] = overflow flag; grows the
   output buffers when needed (then emit again) */
int implisolid_slab_counts(implisolid_slab* s, void* stream, uint32_t out[3]);
int implisolid_slab_grid(implisolid_slab* s, int32_t out[8]);
/* async device copy of counters[2..5] (owned verts incl. halo, faces, active cells, halo verts)
   into d_dst (uint32[4]) on `stream` -- for device-side all-gathers */
int implisolid_slab_copy_counts(implisolid_slab* s, uint32_t* d_dst, void* stream);
int implisolid_slab_set_offsets(implisolid_slab* s, uint32_t voff, uint32_t foff);
/* blocking copy of the slab's emitted vertices (3*V floats) and faces (3*F ints, global ids) */
int implisolid_slab_download(implisolid_slab* s, float* verts, int32_t* faces, void* stream);   /* R, res, cz0, cz1, cz_emit, fz0, fz1, depth */
/* Additive: the normals (mcc2.cpp:852-871, as get_n_ptr's) of the vertices the slab emitted, the rows
   implisolid_slab_download returns.  emit_normals is stream-ordered after emit / emit_verts (the
   vertex count is read on the device); slab_normals is the device array (valid after emit_normals,
   until the slab's buffers grow); download_normals blocks and copies 3*V floats. */
int implisolid_slab_emit_normals(implisolid_slab* s, void* stream);
float* implisolid_slab_normals(implisolid_slab* s);
int implisolid_slab_download_normals(implisolid_slab* s, float* out, void* stream);
float* implisolid_slab_verts(implisolid_slab* s);     /* device pointers */
int32_t* implisolid_slab_faces(implisolid_slab* s);
float* implisolid_slab_field(implisolid_slab* s);
/* blocking copy of the slab's stored field samples (n*n*layers floats, x fastest, converted from
 * the device's brick-major storage); with out == NULL returns the sample count only.
 * implisolid_slab_field's device pointer is brick-major (8x8x2-sample bricks, x fastest inside). */
int64_t implisolid_slab_read_field(implisolid_slab* s, float* out, int64_t capacity);
/* per-kernel HIP-event timing (stream-ordered, no synchronisation) of the following eval /
 * count / emit calls; kernel_times blocks and returns milliseconds of the last timed calls for
 * [brick pass, field eval, MC count, unit scan, vertex emission, face emission] */
int implisolid_slab_set_timing(implisolid_slab* s, int on);
/* after count: [units, non-empty units, owned vertices (incl. halo), triangles, active cells,
 * halo-owned vertices, cells, mixed coarse boxes of the last eval] (blocking) */
int implisolid_slab_stats(implisolid_slab* s, int64_t out[8]);
/* the same figures, then [halo-owned vertices as the vertex pass reads them (counter word 1, must
 * equal [5]), unit parts, small units (the vertex pass takes them two to a wave), heavy units'
 * parts, the vertex pass's wave work items]: writes min(n, 13) values and returns how many exist
 * (13), or -1 */
int implisolid_slab_stats_n(implisolid_slab* s, int64_t* out, int n);
/* the tree kernels the slab's last eval ran: 0 the interpreter, 1 the shape's JIT module, 2 the
 * object's baked JIT module */
int implisolid_slab_used_jit(implisolid_slab* s);
/* process-wide tree-kernel JIT mode for objects set from now on (environment IMPLISOLID_JIT):
 *   0 off (interpreter kernels only), 1 sync (hipRTC compiles before the first eval of a new shape),
 *   2 async (default: compilation runs on background threads, evals use the interpreter kernels
 *   until the module is loaded -- a never-seen shape pays no compile latency).  Compiled code
 *   objects are kept in a disk cache (IMPLISOLID_JIT_CACHE).  Results are bit-identical in every mode. */
void implisolid_set_jit(int mode);
/* tree modules with the object's matrices baked in as literals (IMPLISOLID_JIT_BAKE): 0 never (one
 * module per tree shape, matrices read from memory), 1 every object (one module per object), 2
 * (default) hot objects: an engine that evaluates the same object 4 times requests its baked module
 * (in the background in async mode) and switches to it once loaded.  Bit-identical in every mode. */
void implisolid_set_jit_bake(int mode);
/* block until all scheduled tree-kernel compilations have finished */
void implisolid_jit_wait(void);
/* [mode, bake, modules compiled, modules read from the disk cache], total compile seconds */
void implisolid_jit_stats(int32_t out[4], double* compile_seconds);
/* bound on the loaded tree modules (IMPLISOLID_JIT_MAX_MODULES, default 1024, at least 8): past it
 * the least recently requested modules no engine holds are unloaded (a later request recompiles or
 * reads the disk cache).  Unloads happen at trim points -- set_object and implisolid_jit_wait, where
 * the device is synchronised anyway -- so between them the loaded modules may exceed the bound; a
 * request evicts on its own only once the cache is 4x over it (4 n modules is the hard bound).
 * Replaces nothing in mcc2.cpp: the reference interprets its trees. */
void implisolid_set_jit_max_modules(int n);
/* [modules resident, bound, modules unloaded so far] */
void implisolid_jit_modules(int32_t out[3]);
int implisolid_slab_kernel_times(implisolid_slab* s, float ms[6]);
/* the same timing per kernel: [coarse interval pass, brick refine, brick fill, field eval, MC count,
 * unit scan, vertex emission (k_mc_cells), face emission (k_mc_faces)] */
int implisolid_slab_kernel_times_each(implisolid_slab* s, float ms[8]);
/* blocking copy of the slab's sample signs (1: value < 0), n*n*layers bytes, x fastest; with
 * out == NULL returns the count.  At pruning level 2 sign-filled bricks keep no field values, so
 * this (not the field) is the complete sign information marching cubes uses. */
int64_t implisolid_slab_read_signs(implisolid_slab* s, uint8_t* out, int64_t capacity);
/* bricks of the last slab eval: out = [bricks, mixed-sign bricks, sign-filled bricks] (blocking);
 * sign-filled = no value computed (claimed neighbour candidates, which were evaluated, excluded) */
int implisolid_slab_brick_stats(implisolid_slab* s, int64_t out[3]);
/* the per-brick fill bytes of the last slab eval (blocking; diagnostics and tests): bits 0-1 the
 * brick's sign class (0 mixed, 1 positive, 2 negative), bits 4-5 its fill class (0: listed and
 * evaluated), 0x08 a claim candidate, 0x80 claimed and evaluated by a mixed neighbour's wave.
 * dims = bricks per axis (x fastest).  Returns the brick count; out may be null. */
int64_t implisolid_slab_read_fill(implisolid_slab* s, uint8_t* out, int64_t capacity, int32_t dims[3]);

/* Object stream (BASELINE config 5): n objects polygonised with the same mc settings, each with
 * its own buffers.  create runs each object once to size its outputs, then:
 *   n_streams <= 0 (merged): run() launches every stage of eval + MC once for all objects (block row
 *     y = object y; the interpreter kernels, no per-object compilation);
 *   n_streams >= 1: compiles every tree kernel (parallel hipRTC), captures each object's eval +
 *     count + emit in a hipGraph (direct launches when capture is unavailable, or with
 *     IMPLISOLID_NO_GRAPH=1), and run() replays them round-robin over n_streams streams joined back
 *     into `stream`.
 * run is async on `stream`; counts and download block.  info = {objects, streams, graphs (1/0),
 * merged (1/0)} and the JIT compile seconds. */
/* With the mc settings' "normals": {"enabled": 1} (read as build_geometry reads it) every run() also
 * computes each object's per-vertex normals (mcc2.cpp:852-871, as get_n_ptr's), stream-ordered behind
 * its face pass with no host round trip: merged, one more launch per depth class for all objects;
 * per object, one more kernel at the end of its graph (or of its direct launches).  Without the key
 * run() enqueues what it always did and no normals buffer exists.
 *   has_normals       1 if the batch was created with the key, else 0
 *   download_normals  blocking, synchronises like download: copies 3 * n_verts floats, the rows of
 *                     download's vertices; *problems (may be NULL) = that object's rows that took the
 *                     -42 branch in the last run.  -1 with implisolid_last_error() for a bad index and
 *                     for a batch created without the key (no normals exist: an error, not an empty
 *                     result). */
typedef struct implisolid_batch implisolid_batch;
implisolid_batch* implisolid_batch_create(const char* const* shapes, int n, const char* mc_json, int n_streams);
int implisolid_batch_run(implisolid_batch* b, void* stream);
int implisolid_batch_info(implisolid_batch* b, int32_t out[4], double* jit_seconds);
int implisolid_batch_counts(implisolid_batch* b, int i, uint32_t out[3]);
int implisolid_batch_download(implisolid_batch* b, int i, float* verts, int32_t* faces);
int implisolid_batch_has_normals(implisolid_batch* b);
int implisolid_batch_download_normals(implisolid_batch* b, int i, float* normals_out, int64_t* problems);
void implisolid_batch_destroy(implisolid_batch* b);

/* The OB02 loop (polygonizer steps 1-3, polygonizer_algorithm_ob02.hpp:74-157) on one Z-slab shard of
 * a multi-GPU build: every rank loads the whole MC mesh (device pointers on the current device) and
 * owns the vertices [v0, v1) of its slab.  resample / project (+ QEM per the mc settings) update only
 * the owned vertices, evaluating the faces that touch them (and their edge neighbours for the
 * resampling weights); the edge-length fold runs over every face on every rank.  After each step
 * that moves vertices, the caller exchanges the owned ranges: get_verts copies the current
 * vertices (3 nv floats) into a device buffer, set_verts takes them back.  Every call blocks;
 * ranges = [v0, v1, work faces f0, f1, centroid faces f0, f1].  Results are byte-identical to the
 * single-device loop.  0, or -1 with implisolid_last_error(). */
typedef struct implisolid_ob02 implisolid_ob02;
implisolid_ob02* implisolid_ob02_create(const char* shape_json, const char* mc_json);
void implisolid_ob02_destroy(implisolid_ob02* h);
int implisolid_ob02_load(implisolid_ob02* h, const float* d_verts, int64_t nv, const int32_t* d_faces, int64_t nf, int64_t v0,
                         int64_t v1);
int implisolid_ob02_resample(implisolid_ob02* h);
int implisolid_ob02_project(implisolid_ob02* h);
int implisolid_ob02_subdivide(implisolid_ob02* h, float amplitude);
int implisolid_ob02_counts(implisolid_ob02* h, int64_t out[2]);
int implisolid_ob02_ranges(implisolid_ob02* h, int64_t out[6]);
int implisolid_ob02_get_verts(implisolid_ob02* h, float* d_dst);
int implisolid_ob02_set_verts(implisolid_ob02* h, const float* d_src);
int implisolid_ob02_download(implisolid_ob02* h, float* verts, int32_t* faces);
/* Stream-ordered form of the same loop (distributed.ob02_sharded): no host synchronisation per step.
 *   attach: like load, ordered after `after_stream` by an event (no device synchronisation), and
 *     d_verts (3 nv floats, the caller's, kept alive until destroy or the next attach/load) becomes
 *     the working vertex array itself: the steps update it in place and the caller's exchange
 *     writes the other ranks' ranges into it.  Two small read-backs size the shard's ranges.
 *   stream: the handle's HIP stream; the caller enqueues its collectives on it (and orders its
 *     own streams after it).
 *   resample_async / project_async: the steps, enqueued on that stream.
 *   unpack: after an all-gather of every rank's owned range into equal rows (row r = rank r's
 *     3 (voff[r+1] - voff[r]) floats at d_rows + r row_len; voff: host int64[world + 1]), one kernel
 *     on the stream copies every row but `self` into the vertex array.
 *   halo: [h0, h1), the vertices the next resampling reads (those of the faces whose centroids its
 *     weights use): between a QEM and a resampling only they must be exchanged; the edge-length
 *     fold of a projection reads every vertex. */
int implisolid_ob02_attach(implisolid_ob02* h, float* d_verts, int64_t nv, const int32_t* d_faces, int64_t nf, int64_t v0,
                           int64_t v1, void* after_stream);
void* implisolid_ob02_stream(implisolid_ob02* h);
int implisolid_ob02_resample_async(implisolid_ob02* h);
int implisolid_ob02_project_async(implisolid_ob02* h);
int implisolid_ob02_unpack(implisolid_ob02* h, const float* d_rows, int64_t row_len, const int64_t* voff, int world, int self);
int implisolid_ob02_halo(implisolid_ob02* h, int64_t out[2]);

#ifdef __cplusplus
}
#endif
#endif
