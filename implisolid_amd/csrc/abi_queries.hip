// abi_queries.hip -- the field queries of the C ABI: the interval probes, bounds, slices, rays and mass properties
// (the layer queries are abi_layers.hip's).  Each entry validates its request, compiles the shape (QueryShape), puts
// it on the device and runs its passes; the scaffolding is abi_common.hpp's.  The two ray queries share
// ray_request.  Slice and ray spans place their records with abi_common.hpp's CountedOutput and keep them in a
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
