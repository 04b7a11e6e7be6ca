// abi_queries.hip -- the field queries of the C ABI: the interval probes, bounds, slices, layer images and
// their islands, distance fields, hollowed shells, support tips, run-length streams and bodies, rays and mass properties.  Each entry validates its request, compiles
// the shape (QueryShape), puts it on the device and runs its passes; the scaffolding is abi_common.hpp's.
// The seven layer queries share their request (LayerRequest) and the passes that make a chunk's image
// (LayerImages): each reads as what it does with the image.  The two ray queries share ray_request.  Slice,
// islands, supports, runs, bodies and ray spans place their records with abi_common.hpp's CountedOutput and keep them in a
// ResultSlot; the timed queries keep their figures in a PassTimer.
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "../../include/implisolid.h"
#include "abi_common.hpp"

using namespace impli;
using namespace impli::cabi;

// ---- the interval probes ----------------------------------------------------------------------------
namespace {
struct JitHold {   // a tree module compiled before the launch (sync mode for the request), held for the scope
    TreeJit::Slot* slot = nullptr;
    ~JitHold() { TreeJit::instance().release(slot); }
    void request(const Program& p, bool baked, hipStream_t s) {
        TreeJit& J = TreeJit::instance();
        struct Restore {
            TreeJit& J;
            int mode;
            ~Restore() { J.set_mode(mode); }
        } restore{J, J.mode()};
        J.set_mode(TreeJit::kSync);
        slot = J.request(p, TreeJit::kBricks, baked, s);
    }
};
}  // namespace

extern "C" {

int implisolid_debug_intervals(const char* shape_json, int ignore_root_matrix, int variant, const float* boxes,
                               const uint64_t* modes_in, int64_t n, float* iv_out, uint64_t* modes_out) {
    if (!shape_json || variant < 0 || variant > 2 || n < 0 || (n && (!boxes || !iv_out || !modes_out))) {
        report("implisolid_debug_intervals: bad arguments", false);
        return -1;
    }
    if (n == 0) return 0;
    JitHold jit;   // outlives the guard: released after its tail has drained the device
    return guard_device([&] {
        QueryShape q(shape_json, ignore_root_matrix);
        q.upload();
        Engine& E = *q.E;
        hipStream_t s = q.s;
        hipFunction_t fn = nullptr;
        if (variant) {   // the shape module (1) or the object's baked module (2)
            jit.request(q.prog, variant == 2, s);
            if (!jit.slot || !jit.slot->ready.load(std::memory_order_acquire) || !jit.slot->k.debug_iv)
                throw std::runtime_error("implisolid_debug_intervals: the tree module did not compile");
            fn = jit.slot->k.debug_iv;
        }
        DevBuf& db = E.scratch(0);
        DevBuf& dm = E.scratch(1);
        DevBuf& dout = E.scratch(2);
        db.reserve((size_t)n * 24);
        dm.reserve((size_t)n * 16);   // modes_in, then modes_out
        dout.reserve((size_t)n * 8);
        uint64_t* d_mi = modes_in ? dm.as<uint64_t>() : nullptr;
        uint64_t* d_mo = dm.as<uint64_t>() + n;
        IMPLI_HIP(hipMemcpyAsync(db.p, boxes, (size_t)n * 24, hipMemcpyHostToDevice, s));
        if (modes_in) IMPLI_HIP(hipMemcpyAsync(d_mi, modes_in, (size_t)n * 8, hipMemcpyHostToDevice, s));
        launch_iv_probe(q.d_prog, q.max_depth, q.d_tab, E.tab_range(), db.as<float>(), d_mi, n, dout.as<float>(), d_mo, s, fn);
        IMPLI_HIP(hipGetLastError());
        IMPLI_HIP(hipMemcpyAsync(iv_out, dout.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
        IMPLI_HIP(hipMemcpyAsync(modes_out, d_mo, (size_t)n * 8, hipMemcpyDeviceToHost, s));
        IMPLI_HIP(hipStreamSynchronize(s));
        return 0;
    });
}

int implisolid_debug_eval_modes(const char* shape_json, int ignore_root_matrix, const float* xyz, const uint64_t* modes,
                                int64_t n, float* f_out) {
    if (!shape_json || n < 0 || (n && (!xyz || !modes || !f_out))) {
        report("implisolid_debug_eval_modes: bad arguments", false);
        return -1;
    }
    if (n == 0) return 0;
    return guard_device([&] {
        QueryShape q(shape_json, ignore_root_matrix);
        q.upload();
        Engine& E = *q.E;
        hipStream_t s = q.s;
        DevBuf& dx = E.scratch(0);
        DevBuf& dm = E.scratch(1);
        DevBuf& df = E.scratch(2);
        dx.reserve((size_t)n * 12);
        dm.reserve((size_t)n * 8);
        df.reserve((size_t)n * 4);
        IMPLI_HIP(hipMemcpyAsync(dx.p, xyz, (size_t)n * 12, hipMemcpyHostToDevice, s));
        IMPLI_HIP(hipMemcpyAsync(dm.p, modes, (size_t)n * 8, hipMemcpyHostToDevice, s));
        launch_eval_modes_probe(q.d_prog, q.max_depth, q.d_tab, dx.as<float>(), dm.as<uint64_t>(), n, df.as<float>(), s);
        IMPLI_HIP(hipGetLastError());
        IMPLI_HIP(hipMemcpyAsync(f_out, df.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        IMPLI_HIP(hipStreamSynchronize(s));
        return 0;
    });
}

}  // extern "C"

// ---- bounds of the solid (implisolid_bounds, the "fit_box" settings key) ------------------------
// The descent of eval.hip's k_bounds_level on the current device: E lends its scratch buffers (10:
// state and edge table, 11-14: the two lists), d_prog / d_tab are the object's program and tables
// there.  The only read-back is the state block, after the last level; a raised overflow flag voids
// the run, the lists grow and the descent runs again.  Returns whether the solid has bounds in
// `search` (else out = search); stats (nullable): boxes bounded, boxes skipped as inside the running
// bounds, longest list, reruns after overflow.
namespace {
PassTimer<1> g_bounds_timer;   // implisolid_debug_bounds_ms: HIP events around the level launches
}  // namespace

bool impli::cabi::compute_bounds(Engine& E, hipStream_t s, const Program* d_prog, int prog_depth, const float* d_tab,
                                const float search[6], int depth, float out[6], int64_t stats[4]) {
    const int N = 1 << depth;
    std::vector<float> edges((size_t)3 * (N + 1));
    bounds_edges(search, depth, edges.data());   // validates depth and box (InputError)
    DevBuf& dst = E.scratch(10);
    dst.reserve(kStateBytes + edges.size() * sizeof(float));
    BoundsState* d_state = dst.as<BoundsState>();
    float* d_edges = behind_state<BoundsState>(dst);
    IMPLI_HIP(hipMemcpyAsync(d_edges, edges.data(), edges.size() * sizeof(float), hipMemcpyHostToDevice, s));
    uint32_t cap = list_capacity("IMPLISOLID_BOUNDS_LIST", depth);
    int64_t reruns = 0;
    BoundsState h{};
    Timed<1, 2> tm(g_bounds_timer, false);   // the last descent's figure is assigned, not added up
    for (;;) {
        uint32_t* d_box[2];
        uint64_t* d_modes[2];
        for (int k = 0; k < 2; ++k) {
            E.scratch(11 + k).reserve((size_t)cap * sizeof(uint32_t));
            E.scratch(13 + k).reserve((size_t)cap * sizeof(uint64_t));
            d_box[k] = E.scratch(11 + k).as<uint32_t>();
            d_modes[k] = E.scratch(13 + k).as<uint64_t>();
        }
        tm.mark(0, s);
        launch_bounds_levels(d_prog, prog_depth, d_tab, E.tab_range(), d_edges, depth, d_box, d_modes, cap, d_state, s);
        IMPLI_HIP(hipGetLastError());
        tm.mark(1, s);
        IMPLI_HIP(hipMemcpyAsync(&h, d_state, sizeof h, hipMemcpyDeviceToHost, s));
        IMPLI_HIP(hipStreamSynchronize(s));
        if (!h.overflow) break;
        cap = grown_capacity("bounds", cap, h.count, kBoundsMinDepth, depth);
        ++reruns;
    }
    if (tm) g_bounds_timer.ms[0] = tm.elapsed(tm.ev[0], tm.ev[1]);
    const bool found = h.key[0] != 0xffffffffu;
    for (int a = 0; a < 6; ++a) {
        const uint32_t bits = bounds_key_bits(h.key[a]);
        float f;
        std::memcpy(&f, &bits, sizeof f);
        out[a] = found ? f : search[a];
    }
    if (stats) {
        stats[0] = (int64_t)h.evaluated;
        stats[1] = (int64_t)h.skipped;
        stats[2] = 0;
        for (int l = kBoundsMinDepth; l < depth; ++l) stats[2] = std::max<int64_t>(stats[2], h.count[l]);
        stats[3] = reruns;
    }
    return found;
}

extern "C" {

int implisolid_bounds(const char* shape_json, int ignore_root_matrix, const float search[6], int depth, float out[6],
                      int64_t stats[4]) {
    last_error().clear();
    if (!shape_json || !search || !out) {
        report("implisolid_bounds: bad arguments", false);
        return -1;
    }
    return guard_device([&] {
        // depth and box first: bad input is refused before anything reaches the device
        if (depth < kBoundsMinDepth || depth > kBoundsMaxDepth) throw InputError("implisolid_bounds: depth must be in [3, 10]");
        {
            std::vector<float> probe((size_t)3 * ((1 << depth) + 1));
            bounds_edges(search, depth, probe.data());
        }
        QueryShape q(shape_json, ignore_root_matrix);
        q.upload();
        return compute_bounds(*q.E, q.s, q.d_prog, q.max_depth, q.d_tab, search, depth, out, stats) ? 1 : 0;
    });
}

double implisolid_debug_bounds_ms(int enable) {
    g_bounds_timer.on = enable != 0;
    return g_bounds_timer.ms[0];
}

int implisolid_bounds_edges(const float search[6], int depth, float* edges) {
    return guard_host([&] {
        if (!search || !edges) throw InputError("implisolid_bounds_edges: bad arguments");
        bounds_edges(search, depth, edges);
        return 0;
    });
}

int implisolid_fit_box(const float search[6], const float bounds[6], int resolution, int margin, float out[6]) {
    return guard_host([&] {
        if (!search || !bounds || !out || !fit_box(search, bounds, resolution, margin, out))
            throw InputError("implisolid_fit_box: resolution - 2 margin must be >= 1 (margin >= 0)");
        return 0;
    });
}

}  // extern "C"

// ---- slices of the solid (implisolid_slice) ------------------------------------------------------
// Layers go through slice.hip's passes in chunks of whole layers, at most kSliceMaxChunk (layer, tile)
// items each: classify, a read-back of the list's length (it sizes the sample scratch and the march
// and emit grids), march, scan, a read-back of the chunk's per-layer offsets and total (they size
// the output), emit, and the copy into the host slot at the running offset.  E lends its scratch.
namespace {
struct SliceSlot : ResultSlot {  // the last slice's result
    PinnedVec<float> xy;
    PinnedVec<uint32_t> keys;
};
SliceSlot g_slice;

int64_t slice_layers(const QueryShape& q, int R, const std::vector<float>& xs, const std::vector<float>& ys, const float* z,
                     int n_layers, int64_t* layer_offsets, int64_t stats[4]) {
    Engine& E = *q.E;
    hipStream_t s = q.s;
    SliceGrid g;
    g.R = R;
    g.ntx = (R + kSliceTile - 1) / kSliceTile;
    g.tpl = (uint32_t)g.ntx * (uint32_t)g.ntx;
    const uint32_t chunk_layers = cabi::chunk_layers("IMPLISOLID_SLICE_CHUNK", kSliceMaxChunk, g.tpl, n_layers);
    const uint32_t cap = chunk_layers * g.tpl;   // items per chunk, <= kSliceMaxChunk (tpl <= 2^16)
    const bool prune = Engine::pruning() >= 1;
    const size_t W = (size_t)R + 1;
    // every reserve before any pointer is taken: a DevBuf that grows moves
    E.scratch(10).reserve(kStateBytes + (2 * W + (size_t)n_layers) * sizeof(float));
    E.scratch(11).reserve((size_t)cap * sizeof(uint32_t));                        // list
    E.scratch(12).reserve((size_t)cap * sizeof(uint32_t));                        // counts
    E.scratch(13).reserve((size_t)cap * sizeof(uint64_t));                        // the listed tiles' modes
    SliceState* d_state = E.scratch(10).as<SliceState>();
    float* d_xs = behind_state<SliceState>(E.scratch(10));
    float* d_ys = d_xs + W;
    float* d_z = d_ys + W;
    uint32_t* d_list = E.scratch(11).as<uint32_t>();
    uint32_t* d_counts = E.scratch(12).as<uint32_t>();
    uint64_t* d_lmodes = E.scratch(13).as<uint64_t>();
    CountedOutput segments(E.scratch(14), cap, g.tpl, d_counts);   // a tile's segments, a layer's offset
    IMPLI_HIP(hipMemcpyAsync(d_xs, xs.data(), W * sizeof(float), hipMemcpyHostToDevice, s));
    IMPLI_HIP(hipMemcpyAsync(d_ys, ys.data(), W * sizeof(float), hipMemcpyHostToDevice, s));
    IMPLI_HIP(hipMemcpyAsync(d_z, z, (size_t)n_layers * sizeof(float), hipMemcpyHostToDevice, s));
    g_slice.xy.resize(0);
    g_slice.keys.resize(0);
    int64_t total = 0, listed = 0, samples = 0, chunks = 0;
    for (int l0 = 0; l0 < n_layers; l0 += (int)chunk_layers, ++chunks) {
        const uint32_t nl = (uint32_t)std::min<int64_t>(chunk_layers, n_layers - l0);
        const uint32_t n = nl * g.tpl;
        const int64_t first = (int64_t)l0 * g.tpl;
        IMPLI_HIP(hipMemsetAsync(d_state, 0, sizeof(SliceState), s));
        IMPLI_HIP(hipMemsetAsync(d_counts, 0, (size_t)n * sizeof(uint32_t), s));
        launch_slice_classify(q.d_prog, q.max_depth, q.d_tab, E.tab_range(), d_xs, d_ys, d_z, g, first, n, prune, d_list, d_lmodes,
                              d_state, s);
        IMPLI_HIP(hipGetLastError());
        SliceState h{};
        IMPLI_HIP(hipMemcpyAsync(&h, d_state, sizeof h, hipMemcpyDeviceToHost, s));
        IMPLI_HIP(hipStreamSynchronize(s));
        if (h.n_listed > n) throw HipError("slice: the tile list overran its chunk");
        listed += h.n_listed;
        samples += (int64_t)h.samples;
        uint32_t chunk_total = 0;
        if (h.n_listed) {
            E.scratch(15).reserve((size_t)h.n_listed * kSliceSamples * sizeof(float));
            float* d_samples = E.scratch(15).as<float>();
            launch_slice_march(q.d_prog, q.max_depth, q.d_tab, d_xs, d_ys, d_z, g, first, h.n_listed, d_list, d_lmodes, d_samples,
                               d_counts, s);
            chunk_total = segments.place(nl, s, total, "implisolid_slice: the slice reaches 2^31 segments", layer_offsets + l0);
            if (chunk_total) {
                E.scratch(0).reserve((size_t)chunk_total * 4 * sizeof(float));
                E.scratch(1).reserve((size_t)chunk_total * 2 * sizeof(uint32_t));
                launch_slice_emit(d_xs, d_ys, g, first, h.n_listed, d_list, d_samples, segments.d_offsets, chunk_total,
                                  E.scratch(0).as<float>(), E.scratch(1).as<uint32_t>(), s);
                IMPLI_HIP(hipGetLastError());
                g_slice.xy.resize((size_t)(total + chunk_total) * 4);
                g_slice.keys.resize((size_t)(total + chunk_total) * 2);
                IMPLI_HIP(hipMemcpyAsync(g_slice.xy.data() + 4 * total, E.scratch(0).p, (size_t)chunk_total * 4 * sizeof(float),
                                         hipMemcpyDeviceToHost, s));
                IMPLI_HIP(hipMemcpyAsync(g_slice.keys.data() + 2 * total, E.scratch(1).p,
                                         (size_t)chunk_total * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
                IMPLI_HIP(hipStreamSynchronize(s));
            }
        } else {
            std::fill(layer_offsets + l0, layer_offsets + l0 + nl, total);   // nothing listed: no scan, no segments
        }
        total += chunk_total;
    }
    layer_offsets[n_layers] = total;
    if (stats) {
        stats[0] = (int64_t)n_layers * g.tpl;
        stats[1] = listed;
        stats[2] = samples;
        stats[3] = chunks;
    }
    return total;
}
}  // namespace

extern "C" {

int64_t implisolid_slice(const char* shape_json, int ignore_root_matrix, const float rect[4], int resolution, const float* z,
                         int n_layers, int64_t* layer_offsets, int64_t stats[4]) {
    last_error().clear();
    g_slice.reset();
    if (!shape_json || !rect || !z || !layer_offsets) {
        report("implisolid_slice: bad arguments", false);
        return -1;
    }
    return guard_device([&]() -> int64_t {
        // the request first: bad input is refused before anything reaches the device
        if (n_layers < 1 || n_layers > kSliceMaxLayers) throw InputError("implisolid_slice: n_layers must be in [1, 65536]");
        for (int l = 0; l < n_layers; ++l)
            if (!std::isfinite(z[l])) throw InputError("implisolid_slice: every z must be finite");
        if (resolution < 1 || resolution > kSliceMaxResolution) throw InputError("slice: resolution must be in [1, 4096]");
        std::vector<float> xs((size_t)resolution + 1), ys((size_t)resolution + 1);
        slice_coords(rect, resolution, xs.data(), ys.data());
        QueryShape q(shape_json, ignore_root_matrix);
        q.upload();
        return g_slice.publish(slice_layers(q, resolution, xs, ys, z, n_layers, layer_offsets, stats));
    });
}

int implisolid_slice_copy(float* xy, uint32_t* keys) {
    if (g_slice.refuses_copy("slice", "slice", g_slice.n == 0 || (xy && keys))) return -1;
    if (g_slice.n > 0) {
        std::memcpy(xy, g_slice.xy.data(), (size_t)g_slice.n * 4 * sizeof(float));
        std::memcpy(keys, g_slice.keys.data(), (size_t)g_slice.n * 2 * sizeof(uint32_t));
    }
    return 0;
}

int implisolid_slice_coords(const float rect[4], int resolution, float* xs, float* ys) {
    return guard_host([&] {
        if (!rect || !xs || !ys) throw InputError("implisolid_slice_coords: bad arguments");
        slice_coords(rect, resolution, xs, ys);
        return 0;
    });
}

int64_t implisolid_slice_loops(const uint32_t* keys, int64_t n_segments, int64_t* order, int64_t* loop_offsets,
                               uint8_t* closed) {
    return guard_host([&]() -> int64_t {
        if (n_segments < 0 || !loop_offsets || (n_segments > 0 && (!keys || !order || !closed)))
            throw InputError("implisolid_slice_loops: bad arguments");
        const int64_t loops = slice_loops(keys, n_segments, order, loop_offsets, closed);
        if (loops < 0) report("implisolid_slice_loops: a key starts two segments or ends two", false);
        return loops;
    });
}

}  // extern "C"

// ---- what the layer queries share: the request and the image (raster, islands, layer distance, hollow, supports, runs, bodies) ------
namespace {
// The request of implisolid_<entry>, refused in this order: n_layers, z, width / height, supersample, threshold
// (an entry without one passes 1, which every supersample admits).  The entry's own checks follow, then
// sample(): the rect, which fills mx and my.
struct LayerRequest {
    const float* rect;
    int W, H, ss;
    const float* z;
    int n_layers;
    std::vector<float> mx, my;
    LayerRequest(const std::string& entry, const float* rect, int width, int height, int supersample, const float* z, int n_layers,
                 int threshold = 1)
        : rect(rect), W(width), H(height), ss(supersample), z(z), n_layers(n_layers) {
        const std::string who = "implisolid_" + entry + ": ";
        if (n_layers < 1 || n_layers > kRasterMaxLayers) throw InputError(who + "n_layers must be in [1, 65536]");
        for (int l = 0; l < n_layers; ++l)
            if (!std::isfinite(z[l])) throw InputError(who + "every z must be finite");
        if (W < 1 || W > kRasterMaxSide || H < 1 || H > kRasterMaxSide) throw InputError(who + "width and height must be in [1, 16384]");
        if (ss != 1 && ss != 2 && ss != 4) throw InputError(who + "supersample must be 1, 2 or 4");
        if (threshold < 1 || threshold > ss * ss) throw InputError(who + "threshold must be in [1, supersample^2]");
    }
    void sample() {
        mx.resize((size_t)W * ss);
        my.resize((size_t)H * ss);
        raster_coords(rect, W, H, ss, mx.data(), my.data());
    }
};

// The layers' images, chunk by chunk.  Layers go through raster.hip's passes in chunks of whole layers, at most
// max_items (layer, tile) items each (chunk_env may lower that).  next() enqueues a chunk's head: the state
// block and the image zeroed, classify, a read-back of the two lists' lengths (they size the grids), evaluate,
// fill.  It leaves layers [l0, l0 + nl) in d_img, H rows of g.pitch bytes each, and their sums added to d_sums.
// E lends its scratch: 10 the state block with mx, my and z behind it, 11 the evaluate list, 12 the fill list,
// 13 the listed tiles' modes, 9 the layer sums, 15 the chunk's image.  Every reserve before any pointer is
// taken (a DevBuf that grows moves): these are made here, and a query reserves only buffers of its own.
struct LayerImages {
    const QueryShape& q;
    const LayerRequest& r;
    const char* who;                 // the query's name in the overrun message
    RasterGrid g;
    uint32_t chunk_layers;
    size_t layer_img, layer_px;      // a layer's bytes in d_img, its pixels
    RasterState* d_state;
    float *d_mx, *d_my, *d_z;
    uint32_t *d_list, *d_fill;
    uint64_t* d_lmodes;
    unsigned long long* d_sums;
    uint8_t* d_img;                  // null where no image is wanted (raster with cov == NULL)
    int l0 = 0;                      // the chunk next() has enqueued
    uint32_t nl = 0;
    int64_t evaluated = 0, filled = 0, samples = 0, chunks = 0;
    EventSet<4> ev;                  // with timing: around classify, and around evaluate + fill

    LayerImages(const QueryShape& q, const LayerRequest& r, const char* who, const char* chunk_env, uint64_t max_items,
                bool want_img, bool timing)
        : q(q), r(r), who(who) {
        Engine& E = *q.E;
        g.W = r.W;
        g.H = r.H;
        g.s = r.ss;
        g.ntx = (r.W + kRasterTile - 1) / kRasterTile;
        g.nty = (r.H + kRasterTile - 1) / kRasterTile;
        g.tpl = (uint32_t)g.ntx * (uint32_t)g.nty;   // <= 2^20
        g.pitch = (uint32_t)(kRasterTile * g.ntx);
        chunk_layers = cabi::chunk_layers(chunk_env, max_items, g.tpl, r.n_layers);
        const uint32_t cap = chunk_layers * g.tpl;   // items per chunk: <= max_items, or one layer's
        const size_t n_layers = (size_t)r.n_layers;
        layer_img = (size_t)r.H * g.pitch;
        layer_px = (size_t)r.H * (size_t)r.W;
        E.scratch(10).reserve(kStateBytes + (r.mx.size() + r.my.size() + n_layers) * sizeof(float));
        E.scratch(11).reserve((size_t)cap * sizeof(uint32_t));
        E.scratch(12).reserve((size_t)cap * sizeof(uint32_t));
        E.scratch(13).reserve((size_t)cap * sizeof(uint64_t));
        E.scratch(9).reserve(n_layers * sizeof(uint64_t));
        if (want_img) E.scratch(15).reserve((size_t)chunk_layers * layer_img);
        d_state = E.scratch(10).as<RasterState>();
        d_mx = behind_state<RasterState>(E.scratch(10));
        d_my = d_mx + r.mx.size();
        d_z = d_my + r.my.size();
        d_list = E.scratch(11).as<uint32_t>();
        d_fill = E.scratch(12).as<uint32_t>();
        d_lmodes = E.scratch(13).as<uint64_t>();
        d_sums = E.scratch(9).as<unsigned long long>();
        d_img = want_img ? E.scratch(15).as<uint8_t>() : nullptr;
        IMPLI_HIP(hipMemcpyAsync(d_mx, r.mx.data(), r.mx.size() * sizeof(float), hipMemcpyHostToDevice, q.s));
        IMPLI_HIP(hipMemcpyAsync(d_my, r.my.data(), r.my.size() * sizeof(float), hipMemcpyHostToDevice, q.s));
        IMPLI_HIP(hipMemcpyAsync(d_z, r.z, n_layers * sizeof(float), hipMemcpyHostToDevice, q.s));
        IMPLI_HIP(hipMemsetAsync(d_sums, 0, n_layers * sizeof(uint64_t), q.s));
        if (timing) ev.create();
    }

    // The next chunk's head, enqueued; false after the last.  It synchronises the stream once, at the read-back:
    // whatever the query enqueued for the chunk before has finished when it returns.
    bool next() {
        l0 += (int)nl;
        if (l0 >= r.n_layers) return false;
        nl = (uint32_t)std::min<int64_t>(chunk_layers, r.n_layers - l0);
        const uint32_t n = nl * g.tpl;
        const int64_t first = (int64_t)l0 * g.tpl;
        hipStream_t s = q.s;
        IMPLI_HIP(hipMemsetAsync(d_state, 0, sizeof(RasterState), s));
        if (d_img) IMPLI_HIP(hipMemsetAsync(d_img, 0, (size_t)nl * layer_img, s));   // ordered behind the last chunk's copies
        if (ev[0]) IMPLI_HIP(hipEventRecord(ev[0], s));
        launch_raster_classify(q.d_prog, q.max_depth, q.d_tab, q.E->tab_range(), d_mx, d_my, d_z, g, first, n,
                               Engine::pruning() >= 1, d_list, d_lmodes, d_fill, d_state, s);
        if (ev[1]) IMPLI_HIP(hipEventRecord(ev[1], s));
        IMPLI_HIP(hipGetLastError());
        RasterState h{};
        IMPLI_HIP(hipMemcpyAsync(&h, d_state, sizeof h, hipMemcpyDeviceToHost, s));
        IMPLI_HIP(hipStreamSynchronize(s));
        if (h.n_eval > n || h.n_fill > n || (uint64_t)h.n_eval + h.n_fill > n)
            throw HipError(std::string(who) + ": a tile list overran its chunk");
        evaluated += h.n_eval;
        filled += h.n_fill;
        samples += (int64_t)h.samples;
        if (ev[2]) IMPLI_HIP(hipEventRecord(ev[2], s));
        launch_raster_eval(q.d_prog, q.max_depth, q.d_tab, d_mx, d_my, d_z, g, first, l0, h.n_eval, d_list, d_lmodes, d_img, d_sums, s);
        launch_raster_fill(g, first, l0, h.n_fill, d_fill, d_img, d_sums, s);
        if (ev[3]) IMPLI_HIP(hipEventRecord(ev[3], s));
        ++chunks;
        return true;
    }
    // with timing, after a synchronisation behind the chunk's fill: the ms of its raster passes
    float raster_ms() const {
        float a = 0.f, b = 0.f;
        IMPLI_HIP(hipEventElapsedTime(&a, ev[0], ev[1]));
        IMPLI_HIP(hipEventElapsedTime(&b, ev[2], ev[3]));
        return a + b;
    }
    // stats[0..4] of every layer query: pairs, tiles evaluated, tiles filled, samples, chunks
    void stats(int64_t* out) const {
        const int64_t v[5] = {(int64_t)r.n_layers * g.tpl, evaluated, filled, samples, chunks};
        std::copy(v, v + 5, out);
    }
};
}  // namespace

// ---- layer images of the solid (implisolid_raster) -------------------------------------------------
// Per chunk, behind LayerImages' head: the pitched copy of the chunk's image into a pinned staging slot, with
// the chunk's layer sums behind it.  There are two slots: the host copies a chunk from its slot into the
// caller's buffer while the device works on the next one.
namespace {
struct RasterStage {             // the staging slots, kept until exit (grow-only)
    PinnedVec<uint8_t> img[2];
    PinnedVec<int64_t> sums;
};
RasterStage g_raster;

void raster_layers(const QueryShape& q, const LayerRequest& r, uint8_t* cov, int64_t* layer_sum, int64_t stats[5]) {
    hipStream_t s = q.s;
    LayerImages im(q, r, "raster", "IMPLISOLID_RASTER_CHUNK", kRasterMaxChunk, cov != nullptr, false);
    const size_t layer_out = im.layer_px;
    g_raster.sums.resize((size_t)r.n_layers);
    if (cov)
        for (int k = 0; k < (r.n_layers > (int)im.chunk_layers ? 2 : 1); ++k) g_raster.img[k].resize((size_t)im.chunk_layers * layer_out);
    // the chunk whose image is on its way into a staging slot, not yet in cov
    int pend_l0 = 0;
    uint32_t pend_nl = 0;
    auto drain = [&](int slot) {   // after a synchronisation that covers the pending copy
        if (pend_nl) std::memcpy(cov + (size_t)pend_l0 * layer_out, g_raster.img[slot].data(), (size_t)pend_nl * layer_out);
        pend_nl = 0;
    };
    while (im.next()) {   // its synchronisation: the last chunk's image has landed in the other slot
        const int l0 = im.l0, slot = (int)((im.chunks - 1) & 1);
        const uint32_t nl = im.nl;
        IMPLI_HIP(hipGetLastError());
        if (cov) {
            uint8_t* dst = g_raster.img[slot].data();
            if (im.g.pitch == (uint32_t)r.W)
                IMPLI_HIP(hipMemcpyAsync(dst, im.d_img, (size_t)nl * layer_out, hipMemcpyDeviceToHost, s));
            else
                IMPLI_HIP(hipMemcpy2DAsync(dst, (size_t)r.W, im.d_img, (size_t)im.g.pitch, (size_t)r.W, (size_t)nl * (size_t)r.H,
                                           hipMemcpyDeviceToHost, s));
        }
        IMPLI_HIP(hipMemcpyAsync(g_raster.sums.data() + l0, im.d_sums + l0, (size_t)nl * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        if (cov) {
            drain(slot ^ 1);   // the chunk before this one, while the device works on this one
            pend_l0 = l0;
            pend_nl = nl;
        }
    }
    IMPLI_HIP(hipStreamSynchronize(s));
    if (cov) drain((int)((im.chunks - 1) & 1));
    for (int l = 0; l < r.n_layers; ++l) layer_sum[l] = g_raster.sums.data()[l];
    if (stats) im.stats(stats);
}
}  // namespace

extern "C" {

int implisolid_raster(const char* shape_json, int ignore_root_matrix, const float rect[4], int width, int height, int supersample,
                      const float* z, int n_layers, uint8_t* cov, int64_t* layer_sum, int64_t stats[5]) {
    last_error().clear();
    if (!shape_json || !rect || !z || !layer_sum) {
        report("implisolid_raster: bad arguments", false);
        return -1;
    }
    return guard_device([&] {
        // the request first: bad input is refused before anything is compiled or reaches the device
        LayerRequest r("raster", rect, width, height, supersample, z, n_layers);
        r.sample();
        QueryShape q(shape_json, ignore_root_matrix);
        q.upload();
        raster_layers(q, r, cov, layer_sum, stats);
        return 0;
    });
}

int implisolid_raster_coords(const float rect[4], int width, int height, int supersample, float* mx, float* my) {
    return guard_host([&] {
        if (!rect || !mx || !my) throw InputError("implisolid_raster_coords: bad arguments");
        raster_coords(rect, width, height, supersample, mx, my);
        return 0;
    });
}

}  // extern "C"

// ---- islands of the layers (implisolid_islands) -------------------------------------------------------
// Per chunk, behind LayerImages' head, islands.hip's passes: tiles, merge, rows, the scan, a read-back of the
// chunk's per-layer record offsets (their last entry sizes the records), roots, tally, and the copies of the
// records into the host slot and of the labels, when asked for, into the caller's array.  The image stays on
// the device: the last layer of a chunk is copied to a carry buffer for the first layer of the next.  Scratch
// of its own: 14 the counted output over the rows, 0 the labels, 1 the records, 2 the carried layer.
namespace {
struct IslandSlot : ResultSlot {   // the last call's records
    PinnedVec<int32_t> comps;
};
IslandSlot g_islands;
PassTimer<5> g_island_timer;     // implisolid_debug_islands_ms: HIP events around the launches

int64_t island_layers(const QueryShape& q, const LayerRequest& r, int threshold, int connectivity, int64_t* comp_offsets,
                      int32_t* labels, int64_t stats[8]) {
    Engine& E = *q.E;
    hipStream_t s = q.s;
    const int H = r.H, n_layers = r.n_layers;
    LayerImages im(q, r, "islands", "IMPLISOLID_ISLANDS_CHUNK", kIslandMaxChunk, true, g_island_timer.on);
    const IslandGrid ig = island_grid(r.W, H, im.g.pitch, threshold, connectivity);
    const uint32_t chunk_layers = im.chunk_layers;
    const size_t layer_img = im.layer_img, layer_px = im.layer_px;
    // every reserve before any pointer is taken (the records' buffer, sized per chunk, holds nothing else)
    CountedOutput comps(E.scratch(14), (size_t)chunk_layers * (size_t)H, (uint32_t)H);   // a row's seeds, a layer's offset
    E.scratch(0).reserve((size_t)chunk_layers * layer_px * sizeof(int32_t));   // labels
    if (n_layers > (int)chunk_layers) E.scratch(2).reserve(layer_img);     // the carried layer
    static_assert(sizeof(RasterState) + sizeof(IslandState) <= kStateBytes, "both states share the state block");
    IslandState* d_istate = reinterpret_cast<IslandState*>(im.d_state + 1);
    uint8_t* d_img = im.d_img;
    int32_t* d_lab = E.scratch(0).as<int32_t>();
    uint8_t* d_carry = n_layers > (int)chunk_layers ? E.scratch(2).as<uint8_t>() : nullptr;
    IMPLI_HIP(hipMemsetAsync(d_istate, 0, sizeof(IslandState), s));
    g_islands.comps.resize(0);
    Timed<5, 5> tm(g_island_timer);   // behind im.ev[3], the end of the raster passes: tiles, merge, rows + scan; around roots + tally
    int64_t total = 0;
    while (im.next()) {
        const int l0 = im.l0;
        const uint32_t nl = im.nl;
        launch_island_tiles(ig, nl, d_img, d_lab, d_istate, s);
        tm.mark(0, s);
        launch_island_merge(ig, nl, d_lab, s);
        tm.mark(1, s);
        launch_island_rows(ig, nl, d_lab, comps.d_counts, s);
        const uint32_t cc = comps.place(nl, s, total, "implisolid_islands: the result reaches 2^31 components", comp_offsets + l0,
                                        [&] { tm.mark(2, s); });   // the chunk's components
        if (cc) {
            E.scratch(1).reserve((size_t)cc * 8 * sizeof(int32_t));
            int32_t* d_rec = E.scratch(1).as<int32_t>();
            tm.mark(3, s);
            launch_island_roots(ig, nl, l0, d_lab, comps.d_offsets, cc, d_rec, s);
            launch_island_tally(ig, nl, l0, d_img, d_carry, d_lab, comps.d_groups, d_rec, s);
            tm.mark(4, s);
            IMPLI_HIP(hipGetLastError());
            g_islands.comps.resize((size_t)(total + cc) * 8);
            IMPLI_HIP(hipMemcpyAsync(g_islands.comps.data() + 8 * (size_t)total, d_rec, (size_t)cc * 8 * sizeof(int32_t),
                                     hipMemcpyDeviceToHost, s));
        }
        // without a component no pixel is solid: the tile pass has written -1 everywhere
        if (labels)
            IMPLI_HIP(hipMemcpyAsync(labels + (size_t)l0 * layer_px, d_lab, (size_t)nl * layer_px * sizeof(int32_t),
                                     hipMemcpyDeviceToHost, s));
        if (l0 + (int)nl < n_layers)
            IMPLI_HIP(hipMemcpyAsync(d_carry, d_img + (size_t)(nl - 1) * layer_img, layer_img, hipMemcpyDeviceToDevice, s));
        IMPLI_HIP(hipStreamSynchronize(s));   // the next chunk's launches write the buffers these copies read
        if (tm) {
            tm.add(0, im.raster_ms());
            tm.add(1, im.ev[3], tm.ev[0]);
            tm.add(2, tm.ev[0], tm.ev[1]);
            tm.add(3, tm.ev[1], tm.ev[2]);
            if (cc) tm.add(4, tm.ev[3], tm.ev[4]);
        }
        total += cc;
    }
    comp_offsets[n_layers] = total;
    IslandState hi{};
    IMPLI_HIP(hipMemcpyAsync(&hi, d_istate, sizeof hi, hipMemcpyDeviceToHost, s));
    IMPLI_HIP(hipStreamSynchronize(s));
    int64_t islands = 0, area = 0;
    for (int64_t c = 0; c < total; ++c) {
        const int32_t* rec = g_islands.comps.data() + 8 * (size_t)c;
        islands += rec[2] == 0;
        area += rec[1];
    }
    if (area != (int64_t)hi.solid) throw HipError("islands: the records' areas and the solid pixels disagree");
    if (stats) {
        im.stats(stats);
        stats[5] = total;
        stats[6] = islands;
        stats[7] = (int64_t)hi.solid;
    }
    return total;
}
}  // namespace

extern "C" {

int64_t implisolid_islands(const char* shape_json, int ignore_root_matrix, const float rect[4], int width, int height,
                           int supersample, const float* z, int n_layers, int threshold, int connectivity, int64_t* comp_offsets,
                           int32_t* labels, int64_t stats[8]) {
    last_error().clear();
    g_islands.reset();
    if (!shape_json || !rect || !z || !comp_offsets) {
        report("implisolid_islands: bad arguments", false);
        return -1;
    }
    return guard_device([&]() -> int64_t {
        // the request first: bad input is refused before anything is compiled or reaches the device
        LayerRequest r("islands", rect, width, height, supersample, z, n_layers, threshold);
        if (connectivity != 4 && connectivity != 8) throw InputError("implisolid_islands: connectivity must be 4 or 8");
        r.sample();
        QueryShape q(shape_json, ignore_root_matrix);
        q.upload();
        return g_islands.publish(island_layers(q, r, threshold, connectivity, comp_offsets, labels, stats));
    });
}

int implisolid_islands_copy(int32_t* comps) {
    if (g_islands.refuses_copy("islands", "records", g_islands.n == 0 || comps)) return -1;
    if (g_islands.n > 0) std::memcpy(comps, g_islands.comps.data(), (size_t)g_islands.n * 8 * sizeof(int32_t));
    return 0;
}

int implisolid_debug_islands_ms(int enable, double ms[5]) {
    return g_island_timer.entry(enable, ms);
}

}  // extern "C"

// ---- pixel distance field of the layers (implisolid_layer_distance) --------------------------------------
// Per chunk, behind LayerImages' head, distance.hip's passes: columns, rows, unsupported, and the copy of the
// distances, when asked for, into the caller's array.  The image stays on the device; the last distance layer
// of a chunk is copied to a carry buffer for the first layer of the next.  The records add up on the device
// over the chunks and come down once.  Scratch of its own: 0 the distances, 1 the records, 2 the carried layer.
namespace {
PassTimer<3> g_dist_timer;       // implisolid_debug_layer_distance_ms: HIP events around the launches

void distance_layers(const QueryShape& q, const LayerRequest& r, int threshold, int64_t reach2, int32_t* dist, int64_t* layer_rec,
                     int64_t stats[8]) {
    Engine& E = *q.E;
    hipStream_t s = q.s;
    const int n_layers = r.n_layers;
    LayerImages im(q, r, "distance", "IMPLISOLID_DISTANCE_CHUNK", kDistMaxChunk, true, g_dist_timer.on);
    const DistGrid dg = dist_grid(r.W, r.H, im.g.pitch, threshold);
    const uint32_t chunk_layers = im.chunk_layers;
    const size_t layer_px = im.layer_px;
    // every reserve before any pointer is taken
    E.scratch(0).reserve((size_t)chunk_layers * layer_px * sizeof(int32_t));   // distances
    E.scratch(1).reserve((size_t)n_layers * 4 * sizeof(uint64_t));         // records
    if (n_layers > (int)chunk_layers) E.scratch(2).reserve(layer_px * sizeof(int32_t));   // the carried layer
    int32_t* d_dist = E.scratch(0).as<int32_t>();
    unsigned long long* d_rec = E.scratch(1).as<unsigned long long>();
    int32_t* d_carry = n_layers > (int)chunk_layers ? E.scratch(2).as<int32_t>() : nullptr;
    IMPLI_HIP(hipMemsetAsync(d_rec, 0, (size_t)n_layers * 4 * sizeof(uint64_t), s));
    Timed<3, 2> tm(g_dist_timer);   // behind im.ev[3], the end of the raster passes: columns, rows + unsupported
    while (im.next()) {
        const int l0 = im.l0;
        const uint32_t nl = im.nl;
        launch_distance_columns(dg, nl, im.d_img, d_dist, s);
        tm.mark(0, s);
        launch_distance_rows(dg, nl, l0, d_dist, d_rec, s);
        launch_distance_unsupported(dg, nl, l0, reach2, d_dist, d_carry, d_rec, s);
        tm.mark(1, s);
        IMPLI_HIP(hipGetLastError());
        if (dist)
            IMPLI_HIP(hipMemcpyAsync(dist + (size_t)l0 * layer_px, d_dist, (size_t)nl * layer_px * sizeof(int32_t),
                                     hipMemcpyDeviceToHost, s));
        if (l0 + (int)nl < n_layers)
            IMPLI_HIP(hipMemcpyAsync(d_carry, d_dist + (size_t)(nl - 1) * layer_px, layer_px * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        IMPLI_HIP(hipStreamSynchronize(s));   // the next chunk's launches write the buffers these copies read
        if (tm) {
            tm.add(0, im.raster_ms());
            tm.add(1, im.ev[3], tm.ev[0]);
            tm.add(2, tm.ev[0], tm.ev[1]);
        }
    }
    std::vector<unsigned long long> rec((size_t)n_layers * 4);
    IMPLI_HIP(hipMemcpyAsync(rec.data(), d_rec, rec.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    IMPLI_HIP(hipStreamSynchronize(s));
    int64_t solid = 0, unsupported = 0, whole = 0;
    for (int l = 0; l < n_layers; ++l) {
        const unsigned long long* in = rec.data() + 4 * (size_t)l;
        if ((in[0] == 0) != (in[1] == 0) || in[2] > in[0]) throw HipError("distance: a layer's record contradicts itself");
        int64_t* o = layer_rec + 4 * (size_t)l;
        o[0] = (int64_t)in[0];
        o[1] = (int64_t)(in[1] >> 32);
        o[2] = in[1] ? (int64_t)(0xFFFFFFFFull - (in[1] & 0xFFFFFFFFull)) : -1;
        o[3] = (int64_t)in[2];
        solid += o[0];
        unsupported += o[3];
        whole += o[1] == (int64_t)kDistNone;
    }
    if (stats) {
        im.stats(stats);
        stats[5] = solid;
        stats[6] = unsupported;
        stats[7] = whole;
    }
}
}  // namespace

extern "C" {

int implisolid_layer_distance(const char* shape_json, int ignore_root_matrix, const float rect[4], int width, int height,
                              int supersample, const float* z, int n_layers, int threshold, int64_t reach2, int32_t* dist,
                              int64_t* layer_rec, int64_t stats[8]) {
    last_error().clear();
    if (!shape_json || !rect || !z || !layer_rec) {
        report("implisolid_layer_distance: bad arguments", false);
        return -1;
    }
    return guard_device([&] {
        // the request first: bad input is refused before anything is compiled or reaches the device
        LayerRequest r("layer_distance", rect, width, height, supersample, z, n_layers, threshold);
        if (reach2 < 0 || reach2 >= (int64_t)kDistNone) throw InputError("implisolid_layer_distance: reach2 must be in [0, 2^30)");
        r.sample();
        QueryShape q(shape_json, ignore_root_matrix);
        q.upload();
        distance_layers(q, r, threshold, reach2, dist, layer_rec, stats);
        return 0;
    });
}

int implisolid_debug_layer_distance_ms(int enable, double ms[3]) {
    return g_dist_timer.entry(enable, ms);
}

}  // extern "C"

// ---- hollowed layers (implisolid_layer_hollow) ----------------------------------------------------------------
// Per chunk, behind LayerImages' head: the chunk's image copied into the image ring, distance.hip's column and row
// passes into the distance ring (a chunk that wraps round the ring's end goes in two runs of consecutive slots),
// then hollow.hip's window pass over the layers whose window is complete -- output lags input by reach layers -- in
// batches of at most a chunk's layers, each copied into the caller's array.  Both rings hold chunk + 2 reach layers
// (or the whole call, if that is fewer): the window of the oldest layer not yet emitted and a whole new chunk.  No
// layer is rastered or transformed twice.  The records add up on the device and come down once.  Scratch of its
// own: 0 the distance ring, 1 the records, 2 the threshold table, 3 the image ring, 4 a batch of out, 5 the row
// pass's records (their solid counts are checked against the window pass's).
namespace {
PassTimer<4> g_hollow_timer;     // implisolid_debug_layer_hollow_ms: HIP events around the launches

void hollow_layers(const QueryShape& q, const LayerRequest& r, int threshold, const int64_t* wall2, int reach, int ends, uint8_t* out,
                   int64_t* layer_rec, int64_t stats[8]) {
    Engine& E = *q.E;
    hipStream_t s = q.s;
    const int n_layers = r.n_layers;
    LayerImages im(q, r, "hollow", "IMPLISOLID_HOLLOW_CHUNK", kHollowMaxChunk, true, g_hollow_timer.on);
    const uint32_t chunk_layers = im.chunk_layers;
    const uint32_t ring = (uint32_t)std::min<uint64_t>((uint64_t)chunk_layers + 2u * (uint64_t)reach, (uint64_t)n_layers);
    const size_t layer_px = im.layer_px, layer_img = im.layer_img;
    const DistGrid dg = dist_grid(r.W, r.H, im.g.pitch, threshold);
    HollowGrid hg;
    hg.W = r.W;
    hg.H = r.H;
    hg.pitch = im.g.pitch;
    hg.threshold = threshold;
    hg.n_layers = n_layers;
    hg.reach = reach;
    hg.ends = ends;
    hg.ring = ring;
    // every reserve before any pointer is taken
    E.scratch(0).reserve((size_t)ring * layer_px * sizeof(int32_t));
    E.scratch(1).reserve((size_t)n_layers * 2 * sizeof(uint64_t));
    E.scratch(2).reserve((size_t)(reach + 1) * sizeof(int32_t));
    E.scratch(3).reserve((size_t)ring * layer_img);
    if (out) E.scratch(4).reserve((size_t)chunk_layers * layer_px);
    E.scratch(5).reserve((size_t)n_layers * 4 * sizeof(uint64_t));
    int32_t* d_dist = E.scratch(0).as<int32_t>();
    unsigned long long* d_rec = E.scratch(1).as<unsigned long long>();
    int32_t* d_wall2 = E.scratch(2).as<int32_t>();
    uint8_t* d_ring = E.scratch(3).as<uint8_t>();
    uint8_t* d_out = out ? E.scratch(4).as<uint8_t>() : nullptr;
    unsigned long long* d_drec = E.scratch(5).as<unsigned long long>();
    std::vector<int32_t> w32(wall2, wall2 + reach + 1);   // each in [0, 2^30): the entry checked
    IMPLI_HIP(hipMemcpyAsync(d_wall2, w32.data(), w32.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    IMPLI_HIP(hipMemsetAsync(d_rec, 0, (size_t)n_layers * 2 * sizeof(uint64_t), s));
    IMPLI_HIP(hipMemsetAsync(d_drec, 0, (size_t)n_layers * 4 * sizeof(uint64_t), s));
    Timed<4, 4> tm(g_hollow_timer);   // behind im.ev[3]: the ring copy + columns, rows; around each window launch
    int emitted = 0;                  // output layers [0, emitted) are done
    int64_t transformed = 0;
    auto emit = [&](int upto) {
        while (emitted < upto) {
            const uint32_t nb = (uint32_t)std::min<int64_t>(chunk_layers, upto - emitted);
            tm.mark(2, s);
            launch_hollow_window(hg, emitted, nb, d_ring, d_dist, d_wall2, d_out, d_rec, s);
            tm.mark(3, s);
            IMPLI_HIP(hipGetLastError());
            if (out)   // the next batch's launch is ordered behind this copy
                IMPLI_HIP(hipMemcpyAsync(out + (size_t)emitted * layer_px, d_out, (size_t)nb * layer_px, hipMemcpyDeviceToHost, s));
            if (tm) {
                IMPLI_HIP(hipStreamSynchronize(s));
                tm.add(3, tm.ev[2], tm.ev[3]);
            }
            emitted += (int)nb;
        }
    };
    while (im.next()) {
        const int l0 = im.l0;
        const uint32_t nl = im.nl;
        // the chunk's runs of consecutive slots: two where it wraps round the ring's end
        struct Run {
            uint32_t first, slot, n;
        } runs[2];
        int n_runs = 0;
        for (uint32_t done = 0; done < nl; ++n_runs) {
            const uint32_t slot = (uint32_t)(l0 + (int)done) % ring;
            runs[n_runs] = {done, slot, std::min(nl - done, ring - slot)};   // nl <= ring: at most two
            done += runs[n_runs].n;
        }
        for (int k = 0; k < n_runs; ++k) {
            const Run& u = runs[k];
            IMPLI_HIP(hipMemcpyAsync(d_ring + (size_t)u.slot * layer_img, im.d_img + (size_t)u.first * layer_img, (size_t)u.n * layer_img,
                                     hipMemcpyDeviceToDevice, s));
            launch_distance_columns(dg, u.n, d_ring + (size_t)u.slot * layer_img, d_dist + (size_t)u.slot * layer_px, s);
        }
        tm.mark(0, s);
        for (int k = 0; k < n_runs; ++k)
            launch_distance_rows(dg, runs[k].n, l0 + (int)runs[k].first, d_dist + (size_t)runs[k].slot * layer_px, d_drec, s);
        tm.mark(1, s);
        IMPLI_HIP(hipGetLastError());
        transformed += nl;
        if (tm) {
            IMPLI_HIP(hipStreamSynchronize(s));
            tm.add(0, im.raster_ms());
            tm.add(1, im.ev[3], tm.ev[0]);
            tm.add(2, tm.ev[0], tm.ev[1]);
        }
        const int fed = l0 + (int)nl;   // layers [0, fed) are in the rings, the last ring of them still there
        emit(fed == n_layers ? n_layers : std::max(0, fed - reach));
    }
    std::vector<unsigned long long> rec((size_t)n_layers * 2), drec((size_t)n_layers * 4);
    IMPLI_HIP(hipMemcpyAsync(rec.data(), d_rec, rec.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    IMPLI_HIP(hipMemcpyAsync(drec.data(), d_drec, drec.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    IMPLI_HIP(hipStreamSynchronize(s));
    if (emitted != n_layers || transformed != (int64_t)n_layers) throw HipError("hollow: a layer was left out");
    int64_t solid = 0, core = 0;
    for (int l = 0; l < n_layers; ++l) {
        const unsigned long long* in = rec.data() + 2 * (size_t)l;
        if (in[1] > in[0] || in[0] != drec[4 * (size_t)l]) throw HipError("hollow: a layer's record contradicts itself");
        layer_rec[2 * (size_t)l] = (int64_t)in[0];
        layer_rec[2 * (size_t)l + 1] = (int64_t)in[1];
        solid += (int64_t)in[0];
        core += (int64_t)in[1];
    }
    if (stats) {
        im.stats(stats);
        stats[5] = solid;
        stats[6] = core;
        stats[7] = transformed;
    }
}
}  // namespace

extern "C" {

int implisolid_layer_hollow(const char* shape_json, int ignore_root_matrix, const float rect[4], int width, int height,
                            int supersample, const float* z, int n_layers, int threshold, const int64_t* wall2, int reach, int ends,
                            uint8_t* out, int64_t* layer_rec, int64_t stats[8]) {
    last_error().clear();
    if (!shape_json || !rect || !z || !wall2 || !layer_rec) {
        report("implisolid_layer_hollow: bad arguments", false);
        return -1;
    }
    return guard_device([&] {
        // the request first: bad input is refused before anything is compiled or reaches the device
        LayerRequest r("layer_hollow", rect, width, height, supersample, z, n_layers, threshold);
        if (reach < 0 || reach > kHollowMaxReach) throw InputError("implisolid_layer_hollow: reach must be in [0, 1024]");
        const uint64_t tpl = (uint64_t)((width + kRasterTile - 1) / kRasterTile) * (uint64_t)((height + kRasterTile - 1) / kRasterTile);
        if ((2ull * (uint64_t)reach + 1ull) * tpl > kHollowMaxWindow)
            throw InputError("implisolid_layer_hollow: (2 reach + 1) layers must hold at most 2^20 tiles");
        for (int j = 0; j <= reach; ++j)
            if (wall2[j] < 0 || wall2[j] >= (int64_t)kDistNone || (j && wall2[j] > wall2[j - 1]))
                throw InputError("implisolid_layer_hollow: wall2 must be in [0, 2^30) and non-increasing");
        if (ends < 0 || ends > 3) throw InputError("implisolid_layer_hollow: ends must be in [0, 3]");
        r.sample();
        QueryShape q(shape_json, ignore_root_matrix);
        q.upload();
        hollow_layers(q, r, threshold, wall2, reach, ends, out, layer_rec, stats);
        return 0;
    });
}

int implisolid_hollow_wall2(double wall_px, double pitch_px, int64_t* wall2, int cap) {
    return guard_host([&] {
        if (!std::isfinite(wall_px) || wall_px < 0.0 || !std::isfinite(pitch_px) || pitch_px <= 0.0)
            throw InputError("implisolid_hollow_wall2: wall must be finite and >= 0, pitch finite and > 0");
        const double w2 = wall_px * wall_px;
        if (!(w2 < (double)kDistNone)) throw InputError("implisolid_hollow_wall2: wall^2 must be below 2^30");
        int R = 0;   // the largest j with (j pitch)^2 <= wall^2: the squares do not decrease with j
        while (R <= kHollowMaxReach) {
            const double h = (double)(R + 1) * pitch_px;
            if (!(h * h <= w2)) break;
            ++R;
        }
        if (R > kHollowMaxReach) throw InputError("implisolid_hollow_wall2: the wall reaches more than 1024 layers");
        if (!wall2 || R + 1 > cap) throw InputError("implisolid_hollow_wall2: wall2 holds fewer than reach + 1 entries");
        for (int j = 0; j <= R; ++j) {
            const double h = (double)j * pitch_px;
            wall2[j] = (int64_t)std::floor(w2 - h * h);
        }
        return R;
    });
}

int implisolid_debug_layer_hollow_ms(int enable, double ms[4]) {
    return g_hollow_timer.entry(enable, ms);
}

}  // extern "C"

// ---- support tips under the layer stack (implisolid_layer_supports) -------------------------------------------
// Per chunk, behind LayerImages' head: distance.hip's column and row passes, then supports.hip's: the cell pass
// into the chunk's zeroed table, count, the scan, a read-back of the chunk's per-layer tip offsets (their last
// entry sizes the records), emit, and, where a chunk follows, the top pass; then the copy of the records into a
// pinned staging slot.  There are two slots: the host appends a chunk from its slot to the result slot while the
// device works on the next one.  The image and the distances stay on the device: the last distance layer of a
// chunk is copied to a carry buffer for the first layer of the next, and `top` carries the highest solid layer
// of every pixel in front of the chunk.  The per-layer unsupported counts add up on the device and come down
// once.  Scratch of its own: 14 the counted output over the cells, 0 the distances, 1 the layers' unsupported
// counts with the row pass's records and the bad flag behind them, 2 the carried layer, 3 the table, 4 the
// chunk's records, 5 top.
namespace {
struct SupportSlot : ResultSlot {   // the last call's tips
    PinnedVec<int32_t> tips;
};
SupportSlot g_supports;
struct SupportStage {               // the staging slots, kept until exit (grow-only)
    PinnedVec<int32_t> tips[2];
};
SupportStage g_support_stage;
PassTimer<4> g_support_timer;       // implisolid_debug_layer_supports_ms: HIP events around the launches

int64_t support_layers(const QueryShape& q, const LayerRequest& r, int threshold, int64_t reach2, int cell, int64_t* tip_offsets,
                       int64_t* layer_rec, int64_t stats[8]) {
    Engine& E = *q.E;
    hipStream_t s = q.s;
    const int n_layers = r.n_layers;
    LayerImages im(q, r, "supports", "IMPLISOLID_SUPPORTS_CHUNK", kSupportMaxChunk, true, g_support_timer.on);
    const DistGrid dg = dist_grid(r.W, r.H, im.g.pitch, threshold);
    const SupportGrid sg = support_grid(r.W, r.H, im.g.pitch, threshold, cell);
    const uint32_t chunk_layers = im.chunk_layers, ncc = sg.ncx * sg.ncy;   // ncc <= the layer's pixels
    const size_t layer_px = im.layer_px, table = (size_t)chunk_layers * ncc;
    const bool chunked = n_layers > (int)chunk_layers;
    // every reserve before any pointer is taken (the records' buffer, sized per chunk, holds nothing else)
    CountedOutput tips(E.scratch(14), table, ncc);   // a cell's tip, a layer's offset
    E.scratch(0).reserve((size_t)chunk_layers * layer_px * sizeof(int32_t));          // distances
    E.scratch(1).reserve((size_t)n_layers * 5 * sizeof(uint64_t) + sizeof(uint64_t)); // unsupported; the row pass's records; bad
    if (chunked) E.scratch(2).reserve(layer_px * sizeof(int32_t));                    // the carried layer
    E.scratch(3).reserve(table * (sizeof(uint64_t) + sizeof(uint32_t)));              // keys, then loads
    if (chunked) E.scratch(5).reserve(layer_px * sizeof(int32_t));                    // top
    int32_t* d_dist = E.scratch(0).as<int32_t>();
    unsigned long long* d_unsup = E.scratch(1).as<unsigned long long>();
    unsigned long long* d_drec = d_unsup + n_layers;
    uint32_t* d_bad = reinterpret_cast<uint32_t*>(d_drec + 4 * (size_t)n_layers);
    int32_t* d_carry = chunked ? E.scratch(2).as<int32_t>() : nullptr;
    unsigned long long* d_keys = E.scratch(3).as<unsigned long long>();
    uint32_t* d_loads = reinterpret_cast<uint32_t*>(d_keys + table);
    int32_t* d_top = chunked ? E.scratch(5).as<int32_t>() : nullptr;
    IMPLI_HIP(hipMemsetAsync(d_unsup, 0, (size_t)n_layers * 5 * sizeof(uint64_t) + sizeof(uint64_t), s));
    g_supports.tips.resize(0);
    Timed<4, 5> tm(g_support_timer);   // behind im.ev[3]: columns + rows, cells, count + scan; around emit + top
    int64_t total = 0;
    // the chunk whose records are on their way into a staging slot, not yet in the result slot
    uint32_t pend = 0;
    auto drain = [&](int slot) {   // after a synchronisation that covers the pending copy
        if (pend) {
            const size_t at = g_supports.tips.size();
            g_supports.tips.resize(at + 4 * (size_t)pend);
            std::memcpy(g_supports.tips.data() + at, g_support_stage.tips[slot].data(), (size_t)pend * 4 * sizeof(int32_t));
        }
        pend = 0;
    };
    while (im.next()) {   // its synchronisation: the last chunk's records have landed in the other slot
        const int l0 = im.l0, slot = (int)((im.chunks - 1) & 1);
        const uint32_t nl = im.nl;
        const bool more = l0 + (int)nl < n_layers;
        launch_distance_columns(dg, nl, im.d_img, d_dist, s);
        launch_distance_rows(dg, nl, l0, d_dist, d_drec, s);
        tm.mark(0, s);
        IMPLI_HIP(hipMemsetAsync(d_keys, 0, (size_t)nl * ncc * sizeof(uint64_t), s));
        IMPLI_HIP(hipMemsetAsync(d_loads, 0, (size_t)nl * ncc * sizeof(uint32_t), s));
        launch_support_cells(sg, nl, l0, reach2, d_dist, d_carry, d_keys, d_loads, d_unsup, s);
        tm.mark(1, s);
        launch_support_count(sg, nl, d_keys, tips.d_counts, s);
        const uint32_t cc = tips.place(nl, s, total, "implisolid_layer_supports: the result reaches 2^31 tips", tip_offsets + l0,
                                       [&] { tm.mark(2, s); });   // the chunk's tips
        int32_t* d_rec = nullptr;
        if (cc) {
            E.scratch(4).reserve((size_t)cc * 4 * sizeof(int32_t));
            d_rec = E.scratch(4).as<int32_t>();
        }
        tm.mark(3, s);
        if (cc) launch_support_emit(sg, nl, l0, d_keys, d_loads, tips.d_offsets, cc, im.d_img, d_top, d_rec, d_bad, s);
        if (more) launch_support_top(sg, nl, l0, im.d_img, d_top, s);
        tm.mark(4, s);
        if (cc) {
            g_support_stage.tips[slot].resize(0);   // nothing of the chunk before last is kept
            g_support_stage.tips[slot].resize((size_t)cc * 4);
            IMPLI_HIP(hipMemcpyAsync(g_support_stage.tips[slot].data(), d_rec, (size_t)cc * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        if (more)
            IMPLI_HIP(hipMemcpyAsync(d_carry, d_dist + (size_t)(nl - 1) * layer_px, layer_px * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        IMPLI_HIP(hipGetLastError());
        drain(slot ^ 1);   // the chunk before this one, while the device works on this one
        pend = cc;
        total += cc;
        if (tm) {   // only a timed call synchronises here
            IMPLI_HIP(hipStreamSynchronize(s));
            tm.add(0, im.raster_ms());
            tm.add(1, im.ev[3], tm.ev[0]);
            tm.add(2, tm.ev[0], tm.ev[1]);
            tm.add(3, tm.ev[1], tm.ev[2]);
            tm.add(3, tm.ev[3], tm.ev[4]);
        }
    }
    std::vector<unsigned long long> unsup((size_t)n_layers * 5);   // the row pass's records behind the counts
    uint32_t bad = 0;
    IMPLI_HIP(hipMemcpyAsync(unsup.data(), d_unsup, unsup.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    IMPLI_HIP(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
    IMPLI_HIP(hipStreamSynchronize(s));
    drain((int)((im.chunks - 1) & 1));
    tip_offsets[n_layers] = total;
    if (bad) throw HipError("supports: a tip lies outside its cell");
    // the records against their definition
    int64_t unsupported = 0, plate = 0;
    for (int l = 0; l < n_layers; ++l) {
        const int32_t* rec = g_supports.tips.data() + 4 * (size_t)tip_offsets[l];
        const int64_t n = tip_offsets[l + 1] - tip_offsets[l];
        int64_t load = 0, last_cell = -1;
        for (int64_t k = 0; k < n; ++k) {
            const int32_t* t = rec + 4 * k;
            const int64_t p = t[0];
            if (p < 0 || p >= (int64_t)layer_px || t[3] < 1 || t[1] < 1 || t[2] < -1 || t[2] > l - 2)
                throw HipError("supports: a tip's record contradicts itself");
            const int64_t c = (p / r.W / cell) * (int64_t)sg.ncx + (p % r.W) / cell;
            if (c <= last_cell) throw HipError("supports: a tip lies outside the cell whose turn it is");
            last_cell = c;
            load += t[3];
            plate += t[2] == -1;
        }
        if (load != (int64_t)unsup[(size_t)l] || n > (int64_t)unsup[(size_t)l] || unsup[(size_t)l] > unsup[(size_t)n_layers + 4 * (size_t)l])
            throw HipError("supports: a layer's loads and its unsupported pixels disagree");
        layer_rec[2 * (size_t)l] = (int64_t)unsup[(size_t)l];
        layer_rec[2 * (size_t)l + 1] = n;
        unsupported += (int64_t)unsup[(size_t)l];
    }
    if (stats) {
        im.stats(stats);
        stats[5] = unsupported;
        stats[6] = total;
        stats[7] = plate;
    }
    return total;
}
}  // namespace

extern "C" {

int64_t implisolid_layer_supports(const char* shape_json, int ignore_root_matrix, const float rect[4], int width, int height,
                                  int supersample, const float* z, int n_layers, int threshold, int64_t reach2, int cell,
                                  int64_t* tip_offsets, int64_t* layer_rec, int64_t stats[8]) {
    last_error().clear();
    g_supports.reset();
    if (!shape_json || !rect || !z) {
        report("implisolid_layer_supports: bad arguments", false);
        return -1;
    }
    return guard_device([&]() -> int64_t {
        // the request first: bad input is refused before anything is compiled or reaches the device
        LayerRequest r("layer_supports", rect, width, height, supersample, z, n_layers, threshold);
        if (reach2 < 0 || reach2 >= (int64_t)kDistNone) throw InputError("implisolid_layer_supports: reach2 must be in [0, 2^30)");
        if (cell < 1 || cell > kSupportMaxCell) throw InputError("implisolid_layer_supports: cell must be in [1, 16384]");
        if (!tip_offsets || !layer_rec) throw InputError("implisolid_layer_supports: tip_offsets and layer_rec are required");
        r.sample();
        QueryShape q(shape_json, ignore_root_matrix);
        q.upload();
        return g_supports.publish(support_layers(q, r, threshold, reach2, cell, tip_offsets, layer_rec, stats));
    });
}

int implisolid_layer_supports_copy(int32_t* tips) {
    if (g_supports.refuses_copy("layer_supports", "tips", g_supports.n == 0 || tips)) return -1;
    if (g_supports.n > 0) std::memcpy(tips, g_supports.tips.data(), (size_t)g_supports.n * 4 * sizeof(int32_t));
    return 0;
}

int implisolid_debug_layer_supports_ms(int enable, double ms[4]) {
    return g_support_timer.entry(enable, ms);
}

}  // extern "C"

// ---- run-length layer images (implisolid_layer_runs) ---------------------------------------------------------
// Per chunk, behind LayerImages' head, runs.hip's passes: count, the scan, a read-back of the chunk's per-layer
// run offsets (their last entry sizes the records), emit, and the copy of the records into a pinned staging
// slot.  There are two slots: the host appends a chunk from its slot to the result slot while the device works
// on the next one.  The image stays on the device; runs never cross layers, so nothing is carried between
// chunks.  Scratch of its own: 14 the counted output over the rows, 0 the starts, 1 the values.
namespace {
struct RunSlot : ResultSlot {    // the last call's runs
    PinnedVec<uint32_t> start;
    PinnedVec<uint8_t> value;
};
RunSlot g_runs;
struct RunStage {                // the staging slots, kept until exit (grow-only)
    PinnedVec<uint32_t> start[2];
    PinnedVec<uint8_t> value[2];
    PinnedVec<int64_t> sums;
};
RunStage g_run_stage;
PassTimer<3> g_run_timer;        // implisolid_debug_layer_runs_ms: HIP events around the launches

int64_t run_layers(const QueryShape& q, const LayerRequest& r, int threshold, int64_t* run_offsets, int64_t* layer_sum,
                   int64_t stats[7]) {
    Engine& E = *q.E;
    hipStream_t s = q.s;
    const int H = r.H, n_layers = r.n_layers;
    LayerImages im(q, r, "runs", "IMPLISOLID_RUNS_CHUNK", kRunMaxChunk, true, g_run_timer.on);
    const RunGrid rg = run_grid(r.W, H, im.g.pitch, threshold);
    // the records' buffers, sized per chunk, hold nothing else
    CountedOutput runs(E.scratch(14), (size_t)im.chunk_layers * (size_t)H, (uint32_t)H);   // a row's runs, a layer's offset
    g_runs.start.resize(0);
    g_runs.value.resize(0);
    g_run_stage.sums.resize((size_t)n_layers);
    Timed<3, 3> tm(g_run_timer);   // behind im.ev[3], the end of the raster passes: count + scan; around emit
    int64_t total = 0;
    // the chunk whose records are on their way into a staging slot, not yet in the result slot
    uint32_t pend = 0;
    auto drain = [&](int slot) {   // after a synchronisation that covers the pending copy
        if (pend) {
            const size_t at = g_runs.start.size();
            g_runs.start.resize(at + pend);
            g_runs.value.resize(at + pend);
            std::memcpy(g_runs.start.data() + at, g_run_stage.start[slot].data(), (size_t)pend * sizeof(uint32_t));
            std::memcpy(g_runs.value.data() + at, g_run_stage.value[slot].data(), (size_t)pend);
        }
        pend = 0;
    };
    while (im.next()) {   // its synchronisation: the last chunk's records have landed in the other slot
        const int l0 = im.l0, slot = (int)((im.chunks - 1) & 1);
        const uint32_t nl = im.nl;
        launch_run_count(rg, nl, im.d_img, runs.d_counts, s);
        const uint32_t cc = runs.place(nl, s, total, "implisolid_layer_runs: the result reaches 2^31 runs", run_offsets + l0,
                                       [&] { tm.mark(0, s); });   // the chunk's runs: one a layer at least
        if (cc < nl) throw HipError("runs: a layer without a run");
        E.scratch(0).reserve((size_t)cc * sizeof(uint32_t));
        E.scratch(1).reserve((size_t)cc);
        uint32_t* d_start = E.scratch(0).as<uint32_t>();
        uint8_t* d_value = E.scratch(1).as<uint8_t>();
        tm.mark(1, s);
        launch_run_emit(rg, nl, im.d_img, runs.d_offsets, cc, d_start, d_value, s);
        tm.mark(2, s);
        IMPLI_HIP(hipGetLastError());
        g_run_stage.start[slot].resize(0);   // nothing of the chunk before last is kept
        g_run_stage.value[slot].resize(0);
        g_run_stage.start[slot].resize(cc);
        g_run_stage.value[slot].resize(cc);
        IMPLI_HIP(hipMemcpyAsync(g_run_stage.start[slot].data(), d_start, (size_t)cc * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        IMPLI_HIP(hipMemcpyAsync(g_run_stage.value[slot].data(), d_value, (size_t)cc, hipMemcpyDeviceToHost, s));
        IMPLI_HIP(hipMemcpyAsync(g_run_stage.sums.data() + l0, im.d_sums + l0, (size_t)nl * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        drain(slot ^ 1);   // the chunk before this one, while the device works on this one
        pend = cc;
        total += cc;
        if (tm) {   // only a timed call synchronises here
            IMPLI_HIP(hipStreamSynchronize(s));
            tm.add(0, im.raster_ms());
            tm.add(1, im.ev[3], tm.ev[0]);
            tm.add(2, tm.ev[1], tm.ev[2]);
        }
    }
    IMPLI_HIP(hipStreamSynchronize(s));
    drain((int)((im.chunks - 1) & 1));
    run_offsets[n_layers] = total;
    // the records against their definition, and in grey mode against the device's sums
    const int64_t layer_px = (int64_t)im.layer_px;
    int64_t lit = 0;
    for (int l = 0; l < n_layers; ++l) {
        layer_sum[l] = g_run_stage.sums.data()[l];
        const uint32_t* st = g_runs.start.data() + run_offsets[l];
        const uint8_t* va = g_runs.value.data() + run_offsets[l];
        const int64_t n = run_offsets[l + 1] - run_offsets[l];
        if (n < 1 || st[0] != 0u) throw HipError("runs: a layer's first run does not start at pixel 0");
        int64_t sum = 0;
        for (int64_t k = 0; k < n; ++k) {
            const int64_t end = k + 1 < n ? (int64_t)st[k + 1] : layer_px;
            if (end <= (int64_t)st[k] || end > layer_px) throw HipError("runs: a layer's starts do not increase inside the layer");
            sum += (int64_t)va[k] * (end - (int64_t)st[k]);
            lit += va[k] != 0;
        }
        if (threshold == 0 && sum != layer_sum[l]) throw HipError("runs: the runs' coverage and the layer's sum disagree");
    }
    if (stats) {
        im.stats(stats);
        stats[5] = total;
        stats[6] = lit;
    }
    return total;
}
}  // namespace

extern "C" {

int64_t implisolid_layer_runs(const char* shape_json, int ignore_root_matrix, const float rect[4], int width, int height,
                              int supersample, const float* z, int n_layers, int threshold, int64_t* run_offsets,
                              int64_t* layer_sum, int64_t stats[7]) {
    last_error().clear();
    g_runs.reset();
    if (!shape_json || !rect || !z || !run_offsets || !layer_sum) {
        report("implisolid_layer_runs: bad arguments", false);
        return -1;
    }
    return guard_device([&]() -> int64_t {
        // the request first: bad input is refused before anything is compiled or reaches the device
        LayerRequest r("layer_runs", rect, width, height, supersample, z, n_layers);
        if (threshold < 0 || threshold > supersample * supersample)
            throw InputError("implisolid_layer_runs: threshold must be 0 (grey) or in [1, supersample^2]");
        r.sample();
        QueryShape q(shape_json, ignore_root_matrix);
        q.upload();
        return g_runs.publish(run_layers(q, r, threshold, run_offsets, layer_sum, stats));
    });
}

int implisolid_layer_runs_copy(uint32_t* start, uint8_t* value) {
    if (g_runs.refuses_copy("layer_runs", "runs", start && value)) return -1;   // a result has a run a layer: never empty
    std::memcpy(start, g_runs.start.data(), (size_t)g_runs.n * sizeof(uint32_t));
    std::memcpy(value, g_runs.value.data(), (size_t)g_runs.n);
    return 0;
}

int implisolid_debug_layer_runs_ms(int enable, double ms[3]) {
    return g_run_timer.entry(enable, ms);
}

}  // extern "C"

// ---- bodies of the layer stack (implisolid_layer_bodies) ------------------------------------------------------
// Per chunk, behind LayerImages' head, bodies.hip's passes: count, the scan, a read-back of the chunk's per-layer
// run offsets (their last entry sizes the stack's arrays), emit, link.  The image stays on the device and nothing
// of it is carried: the runs, their union-find and the rows' offsets live in stack-wide arrays that grow with
// the chunks, and a chunk's first layer links to the runs of the layer below there.  Behind the last chunk the
// finish passes: the roots per row, their scan, the records, the tally; then the records, and the runs when asked
// for, come down into the result slot.  Scratch of its own: 14 the counted output over a chunk's rows, 0 the
// runs, 1 the union-find, 2 the rows' offsets, 3 the counted output over the stack's rows, 4 the roots' ordinals,
// 5 the records, 6 the run records.
namespace {
struct BodySlot : ResultSlot {   // the last call's records, and its runs when it asked for them
    PinnedVec<int64_t> bodies;
    PinnedVec<int32_t> runs;
    int64_t n_runs = -1;         // < 0: the call did not ask for runs
};
BodySlot g_bodies;
PassTimer<4> g_body_timer;       // implisolid_debug_layer_bodies_ms: HIP events around the launches

// A stack-wide array grown to `want` bytes with its first `keep` bytes kept: DevBuf::reserve hands out another
// block and drops the old one's contents, so the new block is filled from the old one before that is released.
void grow_keeping(DevBuf& b, size_t keep, size_t want, hipStream_t s) {
    if (b.p && want <= b.bytes) return;
    DevBuf grown;
    grown.reserve(std::max(want, b.bytes + b.bytes / 2));
    try {
        if (keep) IMPLI_HIP(hipMemcpyAsync(grown.p, b.p, keep, hipMemcpyDeviceToDevice, s));
        IMPLI_HIP(hipStreamSynchronize(s));   // nothing in flight reads or writes the old block
    } catch (...) {
        grown.release();
        throw;
    }
    std::swap(b, grown);
    grown.release();
}

int64_t body_layers(const QueryShape& q, const LayerRequest& r, int threshold, int target, int connectivity, bool want_runs,
                    int64_t* run_offsets, int64_t stats[8]) {
    Engine& E = *q.E;
    hipStream_t s = q.s;
    const int H = r.H, n_layers = r.n_layers;
    LayerImages im(q, r, "bodies", "IMPLISOLID_BODIES_CHUNK", kBodyMaxChunk, true, g_body_timer.on);
    const BodyGrid bg = body_grid(r.W, H, im.g.pitch, threshold, target, connectivity);
    const size_t rows = (size_t)n_layers * (size_t)H;   // <= 2^30
    // every reserve before any pointer is taken; the runs' arrays grow in the loop and are addressed through their DevBuf
    CountedOutput placed(E.scratch(14), (size_t)im.chunk_layers * (size_t)H, (uint32_t)H);   // a row's runs, a layer's offset
    CountedOutput roots(E.scratch(3), rows, (uint32_t)rows);                                 // a row's roots; one group, the stack
    E.scratch(2).reserve((rows + 1) * sizeof(uint32_t));
    DevBuf& b_runs = E.scratch(0);
    DevBuf& b_parent = E.scratch(1);
    uint32_t* d_rowoff = E.scratch(2).as<uint32_t>();
    static_assert(sizeof(RasterState) + sizeof(BodyState) <= kStateBytes, "both states share the state block");
    BodyState* d_bstate = reinterpret_cast<BodyState*>(im.d_state + 1);
    IMPLI_HIP(hipMemsetAsync(d_bstate, 0, sizeof(BodyState), s));
    g_bodies.bodies.resize(0);
    g_bodies.runs.resize(0);
    Timed<4, 4> tm(g_body_timer);   // behind im.ev[3], the end of the raster passes: count + scan + emit, link; around the finish
    int64_t total = 0;
    while (im.next()) {
        const int l0 = im.l0;
        const uint32_t nl = im.nl;
        launch_body_count(bg, nl, im.d_img, placed.d_counts, d_bstate, s);
        const uint32_t cc = placed.place(nl, s, total, "implisolid_layer_bodies: the stack reaches 2^31 row runs", run_offsets + l0);
        grow_keeping(b_runs, (size_t)total * 2 * sizeof(int32_t), (size_t)(total + cc + 1) * 2 * sizeof(int32_t), s);
        grow_keeping(b_parent, (size_t)total * sizeof(int32_t), (size_t)(total + cc + 1) * sizeof(int32_t), s);
        launch_body_emit(bg, nl, l0, im.d_img, placed.d_offsets, (uint32_t)total, cc, b_runs.as<int32_t>(), b_parent.as<int32_t>(),
                         d_rowoff, s);
        tm.mark(0, s);
        launch_body_link(bg, nl, l0, b_runs.as<int32_t>(), d_rowoff, b_parent.as<int32_t>(), s);
        tm.mark(1, s);
        IMPLI_HIP(hipGetLastError());
        total += cc;
        if (tm) {   // only a timed call synchronises here
            IMPLI_HIP(hipStreamSynchronize(s));
            tm.add(0, im.raster_ms());
            tm.add(1, im.ev[3], tm.ev[0]);
            tm.add(2, tm.ev[0], tm.ev[1]);
        }
    }
    run_offsets[n_layers] = total;
    // the finish: the roots in run order are the bodies in seed order
    tm.mark(2, s);
    launch_body_root_rows(bg, (uint32_t)rows, d_rowoff, b_parent.as<int32_t>(), roots.d_counts, s);
    int64_t first = 0;
    const uint32_t B = roots.place(1, s, 0, "implisolid_layer_bodies: the stack reaches 2^31 bodies", &first);
    if ((int64_t)B > total) throw HipError("bodies: more roots than runs");
    E.scratch(4).reserve((size_t)(total + 1) * sizeof(uint32_t));
    E.scratch(5).reserve((size_t)(B + 1u) * 8 * sizeof(int64_t));
    if (want_runs) E.scratch(6).reserve((size_t)(total + 1) * 3 * sizeof(int32_t));
    long long* d_rec = E.scratch(5).as<long long>();
    int32_t* d_out = want_runs ? E.scratch(6).as<int32_t>() : nullptr;
    launch_body_roots(bg, (uint32_t)rows, b_runs.as<int32_t>(), d_rowoff, b_parent.as<int32_t>(), roots.d_offsets, B,
                      E.scratch(4).as<uint32_t>(), d_rec, s);
    launch_body_tally(bg, (uint32_t)rows, b_runs.as<int32_t>(), d_rowoff, b_parent.as<int32_t>(), E.scratch(4).as<uint32_t>(), B, d_rec,
                      d_out, s);
    tm.mark(3, s);
    IMPLI_HIP(hipGetLastError());
    g_bodies.bodies.resize((size_t)B * 8);
    if (B) IMPLI_HIP(hipMemcpyAsync(g_bodies.bodies.data(), d_rec, (size_t)B * 8 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (want_runs) {
        g_bodies.runs.resize((size_t)total * 3);
        if (total) IMPLI_HIP(hipMemcpyAsync(g_bodies.runs.data(), d_out, (size_t)total * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    BodyState hb{};
    IMPLI_HIP(hipMemcpyAsync(&hb, d_bstate, sizeof hb, hipMemcpyDeviceToHost, s));
    IMPLI_HIP(hipStreamSynchronize(s));
    if (tm) tm.add(3, tm.ev[2], tm.ev[3]);
    int64_t volume = 0;
    for (uint32_t b = 0; b < B; ++b) volume += g_bodies.bodies.data()[8 * (size_t)b + 1];
    if (volume != (int64_t)hb.voxels) throw HipError("bodies: the records' volumes and the target voxels disagree");
    g_bodies.n_runs = want_runs ? total : -1;
    if (stats) {
        im.stats(stats);
        stats[5] = total;
        stats[6] = (int64_t)B;
        stats[7] = (int64_t)hb.voxels;
    }
    return (int64_t)B;
}
}  // namespace

extern "C" {

int64_t implisolid_layer_bodies(const char* shape_json, int ignore_root_matrix, const float rect[4], int width, int height,
                                int supersample, const float* z, int n_layers, int threshold, int target, int connectivity,
                                int want_runs, int64_t* run_offsets, int64_t stats[8]) {
    last_error().clear();
    g_bodies.reset();
    g_bodies.n_runs = -1;
    if (!shape_json || !rect || !z || !run_offsets) {
        report("implisolid_layer_bodies: bad arguments", false);
        return -1;
    }
    return guard_device([&]() -> int64_t {
        // the request first: bad input is refused before anything is compiled or reaches the device
        LayerRequest r("layer_bodies", rect, width, height, supersample, z, n_layers, threshold);
        if (target != 0 && target != 1) throw InputError("implisolid_layer_bodies: target must be 0 (empty) or 1 (solid)");
        if (connectivity != 6 && connectivity != 26) throw InputError("implisolid_layer_bodies: connectivity must be 6 or 26");
        if (want_runs != 0 && want_runs != 1) throw InputError("implisolid_layer_bodies: want_runs must be 0 or 1");
        r.sample();
        QueryShape q(shape_json, ignore_root_matrix);
        q.upload();
        return g_bodies.publish(body_layers(q, r, threshold, target, connectivity, want_runs != 0, run_offsets, stats));
    });
}

int implisolid_layer_bodies_copy(int64_t* bodies, int32_t* runs) {
    if (g_bodies.refuses_copy("layer_bodies", "bodies", (g_bodies.n == 0 || bodies) && (g_bodies.n_runs <= 0 || runs))) return -1;
    if (g_bodies.n > 0) std::memcpy(bodies, g_bodies.bodies.data(), (size_t)g_bodies.n * 8 * sizeof(int64_t));
    if (g_bodies.n_runs > 0) std::memcpy(runs, g_bodies.runs.data(), (size_t)g_bodies.n_runs * 3 * sizeof(int32_t));
    return 0;
}

int implisolid_debug_layer_bodies_ms(int enable, double ms[4]) {
    return g_body_timer.entry(enable, ms);
}

}  // extern "C"

// ---- rays against the solid (implisolid_raycast) -----------------------------------------------------
// Rays go through raycast.hip's two passes in chunks of at most kRayMaxChunk rays: the chunk's origins
// and directions uploaded, march, finish, and the results copied into the caller's arrays.  The work
// figures add up on the device over the chunks and are read back once.  E lends its scratch.
namespace {
// The request implisolid_raycast and implisolid_ray_spans share, refused in this order: n, bisect, steps, the
// range (ray_params), the origins and directions.  Returns the sample parameters.
std::vector<float> ray_request(const std::string& entry, const float* origins, const float* dirs, int64_t n, float t0, float t1,
                               int steps, int bisect) {
    const std::string who = "implisolid_" + entry + ": ";
    if (n < 0 || n > kRayMaxRays) throw InputError(who + "n must be in [0, 2^24]");
    if (bisect < 0 || bisect > kRayMaxBisect) throw InputError(who + "bisect must be in [0, 32]");
    if (steps < 1 || steps > kRayMaxSteps) throw InputError(who + "steps must be in [1, 65536]");
    std::vector<float> ts((size_t)steps + 1);
    ray_params(t0, t1, steps, ts.data());
    for (int64_t i = 0; i < 3 * n; ++i)
        if (!std::isfinite(origins[i]) || !std::isfinite(dirs[i])) throw InputError(who + "every origin and direction must be finite");
    return ts;
}

PassTimer<2> g_ray_timer;        // implisolid_debug_raycast_ms: HIP events around the two launches

void cast_rays(const QueryShape& q, const std::vector<float>& ts, const float* origins, const float* dirs, int64_t n, int bisect,
               int32_t* hit, float* t, float* f, float* normals, int64_t stats[6]) {
    Engine& E = *q.E;
    hipStream_t s = q.s;
    const int N = (int)ts.size() - 1;
    const uint32_t cap = (uint32_t)std::min<int64_t>((int64_t)env_limit("IMPLISOLID_RAY_CHUNK", kRayMaxChunk, kRayMaxChunk), n);
    const bool prune = Engine::pruning() >= 1;
    // every reserve before any pointer is taken: a DevBuf that grows moves
    E.scratch(10).reserve(kStateBytes + ts.size() * sizeof(float));
    E.scratch(11).reserve((size_t)cap * 6 * sizeof(float));                // origins, directions
    E.scratch(12).reserve((size_t)cap * 3 * sizeof(uint32_t));             // hit, F(ts[hit]), work
    E.scratch(13).reserve((size_t)cap * sizeof(uint64_t));                 // the hit segments' modes
    E.scratch(9).reserve((size_t)cap * 2 * sizeof(float));                 // t, f
    if (normals) E.scratch(15).reserve((size_t)cap * 3 * sizeof(float));
    RayState* d_state = E.scratch(10).as<RayState>();
    float* d_ts = behind_state<RayState>(E.scratch(10));
    float* d_org = E.scratch(11).as<float>();
    float* d_dir = d_org + (size_t)cap * 3;
    int32_t* d_hit = E.scratch(12).as<int32_t>();
    float* d_fhit = reinterpret_cast<float*>(d_hit + cap);
    uint32_t* d_work = reinterpret_cast<uint32_t*>(d_hit + 2 * (size_t)cap);
    uint64_t* d_hmodes = E.scratch(13).as<uint64_t>();
    float* d_t = E.scratch(9).as<float>();
    float* d_f = d_t + cap;
    float* d_n = normals ? E.scratch(15).as<float>() : nullptr;
    IMPLI_HIP(hipMemsetAsync(d_state, 0, sizeof(RayState), s));
    IMPLI_HIP(hipMemcpyAsync(d_ts, ts.data(), ts.size() * sizeof(float), hipMemcpyHostToDevice, s));
    Timed<2, 3> tm(g_ray_timer);
    int64_t chunks = 0;
    for (int64_t first = 0; first < n; first += cap, ++chunks) {
        const uint32_t nc = (uint32_t)std::min<int64_t>(cap, n - first);
        IMPLI_HIP(hipMemcpyAsync(d_org, origins + 3 * first, (size_t)nc * 12, hipMemcpyHostToDevice, s));
        IMPLI_HIP(hipMemcpyAsync(d_dir, dirs + 3 * first, (size_t)nc * 12, hipMemcpyHostToDevice, s));
        tm.mark(0, s);
        launch_ray_march(q.d_prog, q.max_depth, q.d_tab, E.tab_range(), d_ts, d_org, d_dir, nc, N, prune, d_hit, d_hmodes, d_fhit,
                         d_work, s);
        tm.mark(1, s);
        launch_ray_finish(q.d_prog, q.max_depth, q.d_tab, d_ts, d_org, d_dir, nc, N, bisect, d_hit, d_hmodes, d_fhit, d_work, d_t,
                          d_f, d_n, d_state, s);
        tm.mark(2, s);
        IMPLI_HIP(hipGetLastError());
        IMPLI_HIP(hipMemcpyAsync(hit + first, d_hit, (size_t)nc * 4, hipMemcpyDeviceToHost, s));
        IMPLI_HIP(hipMemcpyAsync(t + first, d_t, (size_t)nc * 4, hipMemcpyDeviceToHost, s));
        IMPLI_HIP(hipMemcpyAsync(f + first, d_f, (size_t)nc * 4, hipMemcpyDeviceToHost, s));
        if (normals) IMPLI_HIP(hipMemcpyAsync(normals + 3 * first, d_n, (size_t)nc * 12, hipMemcpyDeviceToHost, s));
        if (tm) {   // only a timed call synchronises here
            IMPLI_HIP(hipStreamSynchronize(s));
            tm.add(0, tm.ev[0], tm.ev[1]);
            tm.add(1, tm.ev[1], tm.ev[2]);
        }
    }
    RayState h{};
    IMPLI_HIP(hipMemcpyAsync(&h, d_state, sizeof h, hipMemcpyDeviceToHost, s));
    IMPLI_HIP(hipStreamSynchronize(s));
    if (stats) {
        stats[0] = n * (int64_t)((N + kRaySegment - 1) / kRaySegment);
        stats[1] = (int64_t)h.skipped;
        stats[2] = (int64_t)h.evaluated;
        stats[3] = (int64_t)h.hits;
        stats[4] = (int64_t)h.inside;
        stats[5] = chunks;
    }
}
}  // namespace

extern "C" {

int implisolid_raycast(const char* shape_json, int ignore_root_matrix, const float* origins, const float* dirs, int64_t n,
                       float t0, float t1, int steps, int bisect, int32_t* hit, float* t, float* f, float* normals,
                       int64_t stats[6]) {
    last_error().clear();
    if (!shape_json || (n > 0 && (!origins || !dirs || !hit || !t || !f))) {
        report("implisolid_raycast: bad arguments", false);
        return -1;
    }
    return guard_device([&] {
        // the request first: bad input is refused before anything is compiled or reaches the device
        const std::vector<float> ts = ray_request("raycast", origins, dirs, n, t0, t1, steps, bisect);
        QueryShape q(shape_json, ignore_root_matrix);   // no rays: a bad shape is still reported
        if (stats) std::fill(stats, stats + 6, (int64_t)0);
        if (n == 0) return 0;                           // ... and nothing creates the engine or a stream
        q.upload();
        cast_rays(q, ts, origins, dirs, n, bisect, hit, t, f, normals, stats);
        return 0;
    });
}

int implisolid_ray_params(float t0, float t1, int steps, float* ts) {
    return guard_host([&] {
        if (!ts) throw InputError("implisolid_ray_params: bad arguments");
        ray_params(t0, t1, steps, ts);
        return 0;
    });
}

int implisolid_debug_raycast_ms(int enable, double ms[2]) {
    return g_ray_timer.entry(enable, ms);
}

}  // extern "C"

// ---- solid spans along rays (implisolid_ray_spans) -----------------------------------------------------
// Rays go through rayspans.hip's passes in chunks: at most IMPLISOLID_SPAN_CHUNK rays, and at most
// kSpanMaxWords (ray, segment) words.  Per chunk: the origins and directions uploaded, march, the scan of
// the per-ray counts, tally, a read-back of the chunk's offsets (their last entry sizes the outputs), emit,
// refine, and the copies into the host slot at the running offset.  E lends its scratch.
namespace {
struct SpanSlot : ResultSlot {   // the last call's result
    PinnedVec<int32_t> k;
    PinnedVec<float> t, f, normals;
    bool has_normals = false;
};
SpanSlot g_spans;
PassTimer<3> g_span_timer;       // implisolid_debug_ray_spans_ms: HIP events around the launches

int64_t span_rays(const QueryShape& q, const std::vector<float>& ts, const float* origins, const float* dirs, int64_t n, int bisect,
                  bool want_normals, int64_t* span_offsets, int64_t stats[8]) {
    Engine& E = *q.E;
    hipStream_t s = q.s;
    const int N = (int)ts.size() - 1;
    const uint64_t nseg = (uint64_t)((N + kRaySegment - 1) / kRaySegment);
    const uint64_t by_env = env_limit("IMPLISOLID_SPAN_CHUNK", kRayMaxChunk, kRayMaxChunk);
    const uint32_t cap = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(by_env, kSpanMaxWords / nseg), (uint64_t)n);   // nseg <= 1024: >= 1
    const bool prune = Engine::pruning() >= 1;
    // every reserve before any pointer is taken: a DevBuf that grows moves
    E.scratch(10).reserve(kStateBytes + ts.size() * sizeof(float));
    E.scratch(11).reserve((size_t)cap * 6 * sizeof(float));                         // origins, directions
    E.scratch(12).reserve((size_t)cap * nseg * sizeof(uint64_t));                   // the solidity words
    E.scratch(13).reserve((size_t)cap * 2 * sizeof(uint32_t));                      // counts, info
    SpanState* d_state = E.scratch(10).as<SpanState>();
    float* d_ts = behind_state<SpanState>(E.scratch(10));
    float* d_org = E.scratch(11).as<float>();
    float* d_dir = d_org + (size_t)cap * 3;
    uint64_t* d_words = E.scratch(12).as<uint64_t>();
    uint32_t* d_counts = E.scratch(13).as<uint32_t>();
    uint32_t* d_info = d_counts + cap;
    CountedOutput spans(E.scratch(14), cap, 0, d_counts);   // a ray's spans, and its own offset
    IMPLI_HIP(hipMemsetAsync(d_state, 0, sizeof(SpanState), s));
    IMPLI_HIP(hipMemcpyAsync(d_ts, ts.data(), ts.size() * sizeof(float), hipMemcpyHostToDevice, s));
    g_spans.k.resize(0);
    g_spans.t.resize(0);
    g_spans.f.resize(0);
    g_spans.normals.resize(0);
    Timed<3, 6> tm(g_span_timer);
    int64_t total = 0, chunks = 0;
    for (int64_t first = 0; first < n; first += cap, ++chunks) {
        const uint32_t nc = (uint32_t)std::min<int64_t>(cap, n - first);
        IMPLI_HIP(hipMemcpyAsync(d_org, origins + 3 * first, (size_t)nc * 12, hipMemcpyHostToDevice, s));
        IMPLI_HIP(hipMemcpyAsync(d_dir, dirs + 3 * first, (size_t)nc * 12, hipMemcpyHostToDevice, s));
        tm.mark(0, s);
        launch_span_march(q.d_prog, q.max_depth, q.d_tab, E.tab_range(), d_ts, d_org, d_dir, nc, N, prune, d_words, d_counts, d_info, s);
        tm.mark(1, s);
        const uint32_t sc = spans.place(nc, s, total, "implisolid_ray_spans: the result reaches 2^31 spans", span_offsets + first, [&] {
            launch_span_tally(nc, d_counts, d_info, d_state, s);
            tm.mark(2, s);
        });   // the chunk's spans
        if (sc) {
            E.scratch(9).reserve((size_t)sc * 3 * sizeof(uint32_t));    // {k_in, k_out}, then the spans' rays
            E.scratch(15).reserve((size_t)sc * 4 * sizeof(float));      // t, f
            if (want_normals) E.scratch(0).reserve((size_t)sc * 6 * sizeof(float));
            int32_t* d_k = E.scratch(9).as<int32_t>();
            uint32_t* d_ray_of = reinterpret_cast<uint32_t*>(d_k + 2 * (size_t)sc);
            float* d_t = E.scratch(15).as<float>();
            float* d_f = d_t + 2 * (size_t)sc;
            float* d_n = want_normals ? E.scratch(0).as<float>() : nullptr;
            tm.mark(3, s);
            launch_span_emit(nc, N, d_words, d_info, spans.d_offsets, d_k, d_ray_of, s);
            tm.mark(4, s);
            launch_span_refine(q.d_prog, q.max_depth, q.d_tab, E.tab_range(), d_ts, d_org, d_dir, N, bisect, prune, sc, d_k, d_ray_of,
                               d_t, d_f, d_n, s);
            tm.mark(5, s);
            IMPLI_HIP(hipGetLastError());
            const size_t at = (size_t)total, upto = (size_t)(total + sc);
            g_spans.k.resize(upto * 2);
            g_spans.t.resize(upto * 2);
            g_spans.f.resize(upto * 2);
            if (want_normals) g_spans.normals.resize(upto * 6);
            IMPLI_HIP(hipMemcpyAsync(g_spans.k.data() + 2 * at, d_k, (size_t)sc * 8, hipMemcpyDeviceToHost, s));
            IMPLI_HIP(hipMemcpyAsync(g_spans.t.data() + 2 * at, d_t, (size_t)sc * 8, hipMemcpyDeviceToHost, s));
            IMPLI_HIP(hipMemcpyAsync(g_spans.f.data() + 2 * at, d_f, (size_t)sc * 8, hipMemcpyDeviceToHost, s));
            if (want_normals) IMPLI_HIP(hipMemcpyAsync(g_spans.normals.data() + 6 * at, d_n, (size_t)sc * 24, hipMemcpyDeviceToHost, s));
            IMPLI_HIP(hipStreamSynchronize(s));   // the next chunk's launches write the buffers these copies read
        }
        if (tm) {
            tm.add(0, tm.ev[0], tm.ev[1]);
            tm.add(1, tm.ev[1], tm.ev[2]);   // scan and tally
            if (sc) {
                tm.add(1, tm.ev[3], tm.ev[4]);   // ... then emit
                tm.add(2, tm.ev[4], tm.ev[5]);
            }
        }
        total += sc;
    }
    span_offsets[n] = total;
    SpanState h{};
    IMPLI_HIP(hipMemcpyAsync(&h, d_state, sizeof h, hipMemcpyDeviceToHost, s));
    IMPLI_HIP(hipStreamSynchronize(s));
    if ((int64_t)h.spans != total) throw HipError("ray_spans: the tally and the scan disagree");
    if (stats) {
        stats[0] = n * (int64_t)nseg;
        stats[1] = (int64_t)h.outside;
        stats[2] = (int64_t)h.solid;
        stats[3] = stats[0] - stats[1] - stats[2];   // the whole ray is walked
        stats[4] = total;
        stats[5] = (int64_t)h.rays;
        stats[6] = (int64_t)h.inside;
        stats[7] = chunks;
    }
    return total;
}
}  // namespace

extern "C" {

int64_t implisolid_ray_spans(const char* shape_json, int ignore_root_matrix, const float* origins, const float* dirs, int64_t n,
                             float t0, float t1, int steps, int bisect, int want_normals, int64_t* span_offsets,
                             int64_t stats[8]) {
    last_error().clear();
    g_spans.reset();
    if (!shape_json || !span_offsets || (n > 0 && (!origins || !dirs))) {
        report("implisolid_ray_spans: bad arguments", false);
        return -1;
    }
    return guard_device([&]() -> int64_t {
        // the request first: bad input is refused before anything is compiled or reaches the device
        const std::vector<float> ts = ray_request("ray_spans", origins, dirs, n, t0, t1, steps, bisect);
        QueryShape q(shape_json, ignore_root_matrix);   // no rays: a bad shape is still reported
        if (stats) std::fill(stats, stats + 8, (int64_t)0);
        g_spans.has_normals = want_normals != 0;
        if (n == 0) {                                   // ... and nothing creates the engine or a stream
            span_offsets[0] = 0;
            return g_spans.publish(0);
        }
        q.upload();
        return g_spans.publish(span_rays(q, ts, origins, dirs, n, bisect, want_normals != 0, span_offsets, stats));
    });
}

int implisolid_ray_spans_copy(int32_t* k, float* t, float* f, float* normals) {
    if (g_spans.n >= 0 && normals && !g_spans.has_normals) {   // ahead of the pointers; behind "no spans to copy"
        report("implisolid_ray_spans_copy: the call computed no normals (want_normals was 0)", false);
        return -1;
    }
    if (g_spans.refuses_copy("ray_spans", "spans", g_spans.n == 0 || (k && t && f))) return -1;
    if (g_spans.n > 0) {
        const size_t S = (size_t)g_spans.n;
        std::memcpy(k, g_spans.k.data(), S * 2 * sizeof(int32_t));
        std::memcpy(t, g_spans.t.data(), S * 2 * sizeof(float));
        std::memcpy(f, g_spans.f.data(), S * 2 * sizeof(float));
        if (normals) std::memcpy(normals, g_spans.normals.data(), S * 6 * sizeof(float));
    }
    return 0;
}

int implisolid_debug_ray_spans_ms(int enable, double ms[3]) {
    return g_span_timer.entry(enable, ms);
}

}  // extern "C"

// ---- mass properties of the solid (implisolid_mass) ----------------------------------------------
// mass.hip's passes on the current device: E lends its scratch buffers (10: state block, layer counts,
// edge and sample tables; 11-14: the two lists, as compute_bounds takes them).  The only read-back is
// the state block with the layer counts behind it, after the last launch; a raised overflow flag voids
// the run, the lists grow and everything runs again (the first launch zeroes the sums).
namespace {
bool compute_mass(const QueryShape& q, const float box[6], int depth, uint64_t moments[10], int64_t* layer_cells, int64_t stats[4]) {
    Engine& E = *q.E;
    hipStream_t s = q.s;
    const int N = 1 << depth, last = depth - 2, first = std::min(3, last);
    std::vector<float> tables((size_t)3 * (N + 1) + (size_t)3 * N);
    bounds_edges(box, depth, tables.data());                    // validates depth and box (InputError)
    mass_mids(box, depth, tables.data() + 3 * (N + 1));
    const bool prune = Engine::pruning() >= 1;
    const size_t head = kStateBytes + (size_t)N * sizeof(uint64_t);   // what is read back
    uint32_t cap = list_capacity("IMPLISOLID_MASS_LIST", depth);
    int64_t reruns = 0;
    std::vector<uint64_t> h(head / sizeof(uint64_t));
    MassState hs{};
    for (bool uploaded = false;;) {
        // every reserve before any pointer is taken: a DevBuf that grows moves
        E.scratch(10).reserve(head + tables.size() * sizeof(float));
        uint32_t* d_box[2] = {nullptr, nullptr};
        uint64_t* d_modes[2] = {nullptr, nullptr};
        if (prune) {
            for (int k = 0; k < 2; ++k) {
                E.scratch(11 + k).reserve((size_t)cap * sizeof(uint32_t));
                E.scratch(13 + k).reserve((size_t)cap * sizeof(uint64_t));
                d_box[k] = E.scratch(11 + k).as<uint32_t>();
                d_modes[k] = E.scratch(13 + k).as<uint64_t>();
            }
        }
        MassState* d_state = E.scratch(10).as<MassState>();
        unsigned long long* d_layers = behind_state<MassState, unsigned long long>(E.scratch(10));
        float* d_edges = reinterpret_cast<float*>(d_layers + N);
        float* d_mids = d_edges + 3 * (N + 1);
        if (!uploaded) {
            IMPLI_HIP(hipMemcpyAsync(d_edges, tables.data(), tables.size() * sizeof(float), hipMemcpyHostToDevice, s));
            uploaded = true;
        }
        launch_mass(q.d_prog, q.max_depth, q.d_tab, E.tab_range(), d_edges, d_mids, depth, prune, d_box, d_modes, cap, d_state,
                    d_layers, s);
        IMPLI_HIP(hipGetLastError());
        IMPLI_HIP(hipMemcpyAsync(h.data(), d_state, head, hipMemcpyDeviceToHost, s));
        IMPLI_HIP(hipStreamSynchronize(s));
        std::memcpy(&hs, h.data(), sizeof hs);
        if (!hs.overflow) break;
        cap = grown_capacity("mass", cap, hs.count, first, last + 1);
        ++reruns;
    }
    for (int k = 0; k < 10; ++k) moments[k] = hs.moments[k];
    if (layer_cells)
        for (int k = 0; k < N; ++k) layer_cells[k] = (int64_t)h[kStateBytes / sizeof(uint64_t) + (size_t)k];
    if (stats) {
        stats[0] = (int64_t)hs.bounded;
        stats[1] = (int64_t)hs.whole_cells;
        stats[2] = prune ? 64 * (int64_t)hs.count[last] : (int64_t)1 << (3 * depth);
        stats[3] = reruns;
    }
    return hs.moments[0] != 0;
}
}  // namespace

extern "C" {

int implisolid_mass(const char* shape_json, int ignore_root_matrix, const float box[6], int depth, uint64_t moments[10],
                    int64_t* layer_cells, int64_t stats[4]) {
    last_error().clear();
    if (!shape_json || !box || !moments) {
        report("implisolid_mass: bad arguments", false);
        return -1;
    }
    return guard_device([&] {
        // depth and box first: bad input is refused before anything reaches the device
        if (depth < kBoundsMinDepth || depth > kBoundsMaxDepth) throw InputError("implisolid_mass: depth must be in [3, 10]");
        {
            std::vector<float> probe((size_t)3 * (1 << depth));
            mass_mids(box, depth, probe.data());
        }
        QueryShape q(shape_json, ignore_root_matrix);
        q.upload();
        return compute_mass(q, box, depth, moments, layer_cells, stats) ? 1 : 0;
    });
}

int implisolid_mass_mids(const float box[6], int depth, float* mids) {
    return guard_host([&] {
        if (!box || !mids) throw InputError("implisolid_mass_mids: bad arguments");
        mass_mids(box, depth, mids);
        return 0;
    });
}

int implisolid_mass_physical(const float box[6], int depth, const uint64_t moments[10], double out[10]) {
    return guard_host([&] {
        if (!box || !moments || !out) throw InputError("implisolid_mass_physical: bad arguments");
        return mass_physical(box, depth, moments, out) ? 1 : 0;
    });
}

}  // extern "C"
