// abi_layers.hip -- the layer queries of the C ABI: layer images and their islands, distance fields, hollowed
// shells, support tips, run-length streams, bodies and suction cups.  The eight share their entry (layer_entry), their request
// (LayerRequest) and the passes that make a chunk's image (LayerImages): each reads as what it does with the
// image.  The scaffolding is abi_common.hpp's: islands, supports, runs, bodies and cups place their records with
// CountedOutput and keep them in a ResultSlot; raster, supports and runs bring theirs down through StagingSlots;
// islands, distance and supports hand a CarriedLayer from chunk to chunk; the timed queries keep their figures
// in a PassTimer.
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../../include/implisolid.h"
#include "abi_common.hpp"

using namespace impli;
using namespace impli::cabi;

// ---- what the layer queries share: the request and the image (raster, islands, layer distance, hollow, supports, runs, bodies, cups) ------
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
    // what the layer passes take of the image
    LayerGrid grid(int threshold) const { return {g.W, g.H, g.pitch, threshold}; }
    bool chunked() const { return r.n_layers > (int)chunk_layers; }
    bool more() const { return l0 + (int)nl < r.n_layers; }   // a chunk follows the one in hand
};

// The body of implisolid_<entry>, which has reset its result slot if it has one.  Refused in this order: null
// pointers (have_pointers: the entry's own required ones), the LayerRequest checks, checks() -- the entry's own
// --, the rect, the shape.  Bad input is refused before anything is compiled or reaches the device.
template <class Checks, class Run>
auto layer_entry(const char* entry, bool have_pointers, const char* shape_json, int ignore_root_matrix, const float* rect, int width,
                 int height, int supersample, const float* z, int n_layers, int threshold, Checks&& checks, Run&& run)
    -> decltype(run(std::declval<const QueryShape&>(), std::declval<const LayerRequest&>())) {
    last_error().clear();
    if (!have_pointers || !shape_json || !rect || !z) {
        report(std::string("implisolid_") + entry + ": bad arguments", false);
        return -1;
    }
    return guard_device([&] {
        LayerRequest r(entry, rect, width, height, supersample, z, n_layers, threshold);
        checks();
        r.sample();
        QueryShape q(shape_json, ignore_root_matrix);
        q.upload();
        return run(q, r);
    });
}
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
    StagingSlots stage([&](int slot, size_t l0, uint32_t nl) {   // layers [l0, l0 + nl) into cov
        std::memcpy(cov + l0 * layer_out, g_raster.img[slot].data(), (size_t)nl * layer_out);
    });
    while (im.next()) {   // its synchronisation: the last chunk's image has landed in the other slot
        const int l0 = im.l0, slot = stage.begin();
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
        if (cov) stage.staged((size_t)l0, nl);   // the chunk before this one, while the device works on this one
    }
    IMPLI_HIP(hipStreamSynchronize(s));
    stage.finish();
    for (int l = 0; l < r.n_layers; ++l) layer_sum[l] = g_raster.sums.data()[l];
    if (stats) im.stats(stats);
}
}  // namespace

extern "C" {

int implisolid_raster(const char* shape_json, int ignore_root_matrix, const float rect[4], int width, int height, int supersample,
                      const float* z, int n_layers, uint8_t* cov, int64_t* layer_sum, int64_t stats[5]) {
    return layer_entry("raster", layer_sum, shape_json, ignore_root_matrix, rect, width, height, supersample, z, n_layers, 1, [] {},
                       [&](const QueryShape& q, const LayerRequest& r) {
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
    const IslandGrid ig = island_grid(im.grid(threshold), connectivity);
    const uint32_t chunk_layers = im.chunk_layers;
    const size_t layer_img = im.layer_img, layer_px = im.layer_px;
    // every reserve before any pointer is taken (the records' buffer, sized per chunk, holds nothing else)
    CountedOutput comps(E.scratch(14), (size_t)chunk_layers * (size_t)H, (uint32_t)H);   // a row's seeds, a layer's offset
    E.scratch(0).reserve((size_t)chunk_layers * layer_px * sizeof(int32_t));   // labels
    CarriedLayer<uint8_t> carry(E.scratch(2), layer_img, im.chunked());
    static_assert(sizeof(RasterState) + sizeof(IslandState) <= kStateBytes, "both states share the state block");
    IslandState* d_istate = reinterpret_cast<IslandState*>(im.d_state + 1);
    uint8_t* d_img = im.d_img;
    int32_t* d_lab = E.scratch(0).as<int32_t>();
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
            launch_island_tally(ig, nl, l0, d_img, carry.d, d_lab, comps.d_groups, d_rec, s);
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
        carry.keep(d_img + (size_t)(nl - 1) * layer_img, im.more(), s);
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
    g_islands.reset();
    return layer_entry(
        "islands", comp_offsets, shape_json, ignore_root_matrix, rect, width, height, supersample, z, n_layers, threshold,
        [&] {
            if (connectivity != 4 && connectivity != 8) throw InputError("implisolid_islands: connectivity must be 4 or 8");
        },
        [&](const QueryShape& q, const LayerRequest& r) {
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
    const LayerGrid dg = im.grid(threshold);
    const uint32_t chunk_layers = im.chunk_layers;
    const size_t layer_px = im.layer_px;
    // every reserve before any pointer is taken
    E.scratch(0).reserve((size_t)chunk_layers * layer_px * sizeof(int32_t));   // distances
    E.scratch(1).reserve((size_t)n_layers * 4 * sizeof(uint64_t));         // records
    CarriedLayer<int32_t> carry(E.scratch(2), layer_px, im.chunked());
    int32_t* d_dist = E.scratch(0).as<int32_t>();
    unsigned long long* d_rec = E.scratch(1).as<unsigned long long>();
    IMPLI_HIP(hipMemsetAsync(d_rec, 0, (size_t)n_layers * 4 * sizeof(uint64_t), s));
    Timed<3, 2> tm(g_dist_timer);   // behind im.ev[3], the end of the raster passes: columns, rows + unsupported
    while (im.next()) {
        const int l0 = im.l0;
        const uint32_t nl = im.nl;
        launch_distance_columns(dg, nl, im.d_img, d_dist, s);
        tm.mark(0, s);
        launch_distance_rows(dg, nl, l0, d_dist, d_rec, s);
        launch_distance_unsupported(dg, nl, l0, reach2, d_dist, carry.d, d_rec, s);
        tm.mark(1, s);
        IMPLI_HIP(hipGetLastError());
        if (dist)
            IMPLI_HIP(hipMemcpyAsync(dist + (size_t)l0 * layer_px, d_dist, (size_t)nl * layer_px * sizeof(int32_t),
                                     hipMemcpyDeviceToHost, s));
        carry.keep(d_dist + (size_t)(nl - 1) * layer_px, im.more(), s);
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
    return layer_entry(
        "layer_distance", layer_rec, shape_json, ignore_root_matrix, rect, width, height, supersample, z, n_layers, threshold,
        [&] {
            if (reach2 < 0 || reach2 >= (int64_t)kDistNone) throw InputError("implisolid_layer_distance: reach2 must be in [0, 2^30)");
        },
        [&](const QueryShape& q, const LayerRequest& r) {
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
    const LayerGrid dg = im.grid(threshold);
    const HollowGrid hg{dg, n_layers, reach, ends, ring};
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
    return layer_entry(
        "layer_hollow", wall2 && layer_rec, shape_json, ignore_root_matrix, rect, width, height, supersample, z, n_layers, threshold,
        [&] {
            if (reach < 0 || reach > kHollowMaxReach) throw InputError("implisolid_layer_hollow: reach must be in [0, 1024]");
            const uint64_t tpl = (uint64_t)((width + kRasterTile - 1) / kRasterTile) * (uint64_t)((height + kRasterTile - 1) / kRasterTile);
            if ((2ull * (uint64_t)reach + 1ull) * tpl > kHollowMaxWindow)
                throw InputError("implisolid_layer_hollow: (2 reach + 1) layers must hold at most 2^20 tiles");
            for (int j = 0; j <= reach; ++j)
                if (wall2[j] < 0 || wall2[j] >= (int64_t)kDistNone || (j && wall2[j] > wall2[j - 1]))
                    throw InputError("implisolid_layer_hollow: wall2 must be in [0, 2^30) and non-increasing");
            if (ends < 0 || ends > 3) throw InputError("implisolid_layer_hollow: ends must be in [0, 3]");
        },
        [&](const QueryShape& q, const LayerRequest& r) {
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
    const LayerGrid dg = im.grid(threshold);
    const SupportGrid sg = support_grid(dg, cell);
    const uint32_t chunk_layers = im.chunk_layers, ncc = sg.ncx * sg.ncy;   // ncc <= the layer's pixels
    const size_t layer_px = im.layer_px, table = (size_t)chunk_layers * ncc;
    const bool chunked = im.chunked();
    // every reserve before any pointer is taken (the records' buffer, sized per chunk, holds nothing else)
    CountedOutput tips(E.scratch(14), table, ncc);   // a cell's tip, a layer's offset
    E.scratch(0).reserve((size_t)chunk_layers * layer_px * sizeof(int32_t));          // distances
    E.scratch(1).reserve((size_t)n_layers * 5 * sizeof(uint64_t) + sizeof(uint64_t)); // unsupported; the row pass's records; bad
    CarriedLayer<int32_t> carry(E.scratch(2), layer_px, chunked);
    E.scratch(3).reserve(table * (sizeof(uint64_t) + sizeof(uint32_t)));              // keys, then loads
    if (chunked) E.scratch(5).reserve(layer_px * sizeof(int32_t));                    // top
    int32_t* d_dist = E.scratch(0).as<int32_t>();
    unsigned long long* d_unsup = E.scratch(1).as<unsigned long long>();
    unsigned long long* d_drec = d_unsup + n_layers;
    uint32_t* d_bad = reinterpret_cast<uint32_t*>(d_drec + 4 * (size_t)n_layers);
    unsigned long long* d_keys = E.scratch(3).as<unsigned long long>();
    uint32_t* d_loads = reinterpret_cast<uint32_t*>(d_keys + table);
    int32_t* d_top = chunked ? E.scratch(5).as<int32_t>() : nullptr;
    IMPLI_HIP(hipMemsetAsync(d_unsup, 0, (size_t)n_layers * 5 * sizeof(uint64_t) + sizeof(uint64_t), s));
    g_supports.tips.resize(0);
    Timed<4, 5> tm(g_support_timer);   // behind im.ev[3]: columns + rows, cells, count + scan; around emit + top
    int64_t total = 0;
    StagingSlots stage([&](int slot, size_t at, uint32_t n) {   // tips [at, at + n) of the result
        g_supports.tips.resize(4 * (at + n));
        std::memcpy(g_supports.tips.data() + 4 * at, g_support_stage.tips[slot].data(), (size_t)n * 4 * sizeof(int32_t));
    });
    while (im.next()) {   // its synchronisation: the last chunk's records have landed in the other slot
        const int l0 = im.l0, slot = stage.begin();
        const uint32_t nl = im.nl;
        const bool more = im.more();
        launch_distance_columns(dg, nl, im.d_img, d_dist, s);
        launch_distance_rows(dg, nl, l0, d_dist, d_drec, s);
        tm.mark(0, s);
        IMPLI_HIP(hipMemsetAsync(d_keys, 0, (size_t)nl * ncc * sizeof(uint64_t), s));
        IMPLI_HIP(hipMemsetAsync(d_loads, 0, (size_t)nl * ncc * sizeof(uint32_t), s));
        launch_support_cells(sg, nl, l0, reach2, d_dist, carry.d, d_keys, d_loads, d_unsup, s);
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
            restage(g_support_stage.tips[slot], (size_t)cc * 4);
            IMPLI_HIP(hipMemcpyAsync(g_support_stage.tips[slot].data(), d_rec, (size_t)cc * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        carry.keep(d_dist + (size_t)(nl - 1) * layer_px, more, s);
        IMPLI_HIP(hipGetLastError());
        stage.staged((size_t)total, cc);   // the chunk before this one, while the device works on this one
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
    stage.finish();
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
    g_supports.reset();
    return layer_entry(
        "layer_supports", true, shape_json, ignore_root_matrix, rect, width, height, supersample, z, n_layers, threshold,
        [&] {
            if (reach2 < 0 || reach2 >= (int64_t)kDistNone) throw InputError("implisolid_layer_supports: reach2 must be in [0, 2^30)");
            if (cell < 1 || cell > kSupportMaxCell) throw InputError("implisolid_layer_supports: cell must be in [1, 16384]");
            if (!tip_offsets || !layer_rec) throw InputError("implisolid_layer_supports: tip_offsets and layer_rec are required");
        },
        [&](const QueryShape& q, const LayerRequest& r) {
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
    const LayerGrid rg = im.grid(threshold);
    // the records' buffers, sized per chunk, hold nothing else
    CountedOutput runs(E.scratch(14), (size_t)im.chunk_layers * (size_t)H, (uint32_t)H);   // a row's runs, a layer's offset
    g_runs.start.resize(0);
    g_runs.value.resize(0);
    g_run_stage.sums.resize((size_t)n_layers);
    Timed<3, 3> tm(g_run_timer);   // behind im.ev[3], the end of the raster passes: count + scan; around emit
    int64_t total = 0;
    StagingSlots stage([&](int slot, size_t at, uint32_t n) {   // runs [at, at + n) of the result
        g_runs.start.resize(at + n);
        g_runs.value.resize(at + n);
        std::memcpy(g_runs.start.data() + at, g_run_stage.start[slot].data(), (size_t)n * sizeof(uint32_t));
        std::memcpy(g_runs.value.data() + at, g_run_stage.value[slot].data(), (size_t)n);
    });
    while (im.next()) {   // its synchronisation: the last chunk's records have landed in the other slot
        const int l0 = im.l0, slot = stage.begin();
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
        restage(g_run_stage.start[slot], cc);
        restage(g_run_stage.value[slot], cc);
        IMPLI_HIP(hipMemcpyAsync(g_run_stage.start[slot].data(), d_start, (size_t)cc * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        IMPLI_HIP(hipMemcpyAsync(g_run_stage.value[slot].data(), d_value, (size_t)cc, hipMemcpyDeviceToHost, s));
        IMPLI_HIP(hipMemcpyAsync(g_run_stage.sums.data() + l0, im.d_sums + l0, (size_t)nl * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        stage.staged((size_t)total, cc);   // the chunk before this one, while the device works on this one
        total += cc;
        if (tm) {   // only a timed call synchronises here
            IMPLI_HIP(hipStreamSynchronize(s));
            tm.add(0, im.raster_ms());
            tm.add(1, im.ev[3], tm.ev[0]);
            tm.add(2, tm.ev[1], tm.ev[2]);
        }
    }
    IMPLI_HIP(hipStreamSynchronize(s));
    stage.finish();
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
    g_runs.reset();
    return layer_entry(
        "layer_runs", run_offsets && layer_sum, shape_json, ignore_root_matrix, rect, width, height, supersample, z, n_layers, 1,
        [&] {
            if (threshold < 0 || threshold > supersample * supersample)
                throw InputError("implisolid_layer_runs: threshold must be 0 (grey) or in [1, supersample^2]");
        },
        [&](const QueryShape& q, const LayerRequest& r) { return g_runs.publish(run_layers(q, r, threshold, run_offsets, layer_sum, stats)); });
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
    const BodyGrid bg{im.grid(threshold), target, connectivity};
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
    g_bodies.reset();
    g_bodies.n_runs = -1;
    return layer_entry(
        "layer_bodies", run_offsets, shape_json, ignore_root_matrix, rect, width, height, supersample, z, n_layers, threshold,
        [&] {
            if (target != 0 && target != 1) throw InputError("implisolid_layer_bodies: target must be 0 (empty) or 1 (solid)");
            if (connectivity != 6 && connectivity != 26) throw InputError("implisolid_layer_bodies: connectivity must be 6 or 26");
            if (want_runs != 0 && want_runs != 1) throw InputError("implisolid_layer_bodies: want_runs must be 0 or 1");
        },
        [&](const QueryShape& q, const LayerRequest& r) {
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

// ---- suction cups of the layer stack (implisolid_layer_cups) ---------------------------------------------------
// Per chunk, behind LayerImages' head, bodies.hip's count, the scan, a read-back of the chunk's per-layer run
// offsets, bodies.hip's emit with the runs numbered from 1 (run 0 is the outside), cups.hip's frame; then for
// every layer of the chunk bodies.hip's link of that one layer and cups.hip's mark and head, enqueued back to
// back: the host knows every layer's runs from the read-back and waits for none of them.  The stack-wide arrays
// grow with the chunks as the bodies' do.  Behind the last chunk the finish passes: the heads and the cupped runs
// per row, their scans (per-layer offsets: cup_offsets and run_offsets), the records, the tally; then the
// records, and the cupped runs when asked for, come down into the result slot.  Scratch of its own: 14 the counted
// output over a chunk's rows, 0 the runs, 1 the union-find, 2 the rows' offsets, 3 the counted output of the heads
// over the stack's rows, 4 rootat, 5 cup, 6 first (the heads' ordinals in the finish), 7 the counted output of the
// cupped runs, 8 the records with the run records behind them.
namespace {
struct CupSlot : ResultSlot {    // the last call's records, and its cupped runs when it asked for them
    PinnedVec<int64_t> cups;
    PinnedVec<int32_t> runs;
    int64_t n_runs = -1;         // < 0: the call did not ask for runs
};
CupSlot g_cups;
PassTimer<4> g_cup_timer;        // implisolid_debug_layer_cups_ms: HIP events around the launches

int64_t cup_layers(const QueryShape& q, const LayerRequest& r, int threshold, int connectivity, bool want_runs, int64_t* cup_offsets,
                   int64_t* run_offsets, int64_t stats[8]) {
    Engine& E = *q.E;
    hipStream_t s = q.s;
    const int H = r.H, n_layers = r.n_layers;
    LayerImages im(q, r, "cups", "IMPLISOLID_CUPS_CHUNK", kBodyMaxChunk, true, g_cup_timer.on);
    const BodyGrid bg{im.grid(threshold), 0, connectivity};
    const size_t rows = (size_t)n_layers * (size_t)H;   // <= 2^30
    // every reserve before any pointer is taken; the runs' arrays grow in the loop and are addressed through their DevBuf
    CountedOutput placed(E.scratch(14), (size_t)im.chunk_layers * (size_t)H, (uint32_t)H);   // a row's runs, a layer's offset
    CountedOutput heads(E.scratch(3), rows, (uint32_t)H);                                    // a row's heads, a layer's offset
    CountedOutput kept(E.scratch(7), rows, (uint32_t)H);                                     // a row's cupped runs, a layer's offset
    E.scratch(2).reserve((rows + 1) * sizeof(uint32_t));
    DevBuf& b_runs = E.scratch(0);
    DevBuf& b_parent = E.scratch(1);
    DevBuf& b_rootat = E.scratch(4);
    DevBuf& b_cup = E.scratch(5);
    DevBuf& b_first = E.scratch(6);
    uint32_t* d_rowoff = E.scratch(2).as<uint32_t>();
    static_assert(sizeof(RasterState) + sizeof(BodyState) + sizeof(CupState) <= kStateBytes, "the three states share the state block");
    BodyState* d_bstate = reinterpret_cast<BodyState*>(im.d_state + 1);
    CupState* d_cstate = reinterpret_cast<CupState*>(d_bstate + 1);
    IMPLI_HIP(hipMemsetAsync(d_bstate, 0, sizeof(BodyState) + sizeof(CupState), s));
    g_cups.cups.resize(0);
    g_cups.runs.resize(0);
    Timed<4, 4> tm(g_cup_timer);   // behind im.ev[3], the end of the raster passes: count + scan + emit + frame, the layers' loop; around the finish
    std::vector<int64_t> at((size_t)n_layers + 1);   // layer l's empty row runs are [at[l], at[l + 1]), run 1 + k of the arrays being run k
    int64_t total = 0;
    while (im.next()) {
        const int l0 = im.l0;
        const uint32_t nl = im.nl;
        launch_body_count(bg, nl, im.d_img, placed.d_counts, d_bstate, s);
        const char* limit = "implisolid_layer_cups: the stack reaches 2^31 row runs";
        const uint32_t cc = placed.place(nl, s, total, limit, at.data() + l0);
        if (total + (int64_t)cc + 1 >= ((int64_t)1 << 31)) throw InputError(limit);   // run 0 takes an index too
        // entries 0 .. total + cc, and one to spare; entry 0 is the outside, so the first chunk has nothing to keep
        const size_t have = total ? (size_t)total + 1 : 0, want = (size_t)total + cc + 2;
        grow_keeping(b_runs, have * 2 * sizeof(int32_t), want * 2 * sizeof(int32_t), s);
        for (DevBuf* b : {&b_parent, &b_rootat, &b_cup, &b_first}) grow_keeping(*b, have * sizeof(int32_t), want * sizeof(int32_t), s);
        if (!total) IMPLI_HIP(hipMemsetAsync(b_parent.p, 0, sizeof(int32_t), s));   // parent[0] = 0
        IMPLI_HIP(hipMemsetAsync(b_first.as<uint32_t>() + total + 1, 0, (size_t)cc * sizeof(uint32_t), s));
        launch_body_emit(bg, nl, l0, im.d_img, placed.d_offsets, (uint32_t)total + 1u, cc, b_runs.as<int32_t>(), b_parent.as<int32_t>(),
                         d_rowoff, s);
        launch_cup_frame(bg, nl, l0, b_runs.as<int32_t>(), d_rowoff, b_parent.as<int32_t>(), s);
        tm.mark(0, s);
        for (uint32_t k = 0; k < nl; ++k) {   // nothing here waits for the device
            const uint32_t lo = 1u + (uint32_t)at[(size_t)l0 + k], hi = 1u + (uint32_t)(k + 1u < nl ? at[(size_t)l0 + k + 1] : total + cc);
            if (lo == hi) continue;   // a layer without an empty voxel
            launch_body_link(bg, 1, l0 + (int)k, b_runs.as<int32_t>(), d_rowoff, b_parent.as<int32_t>(), s);
            launch_cup_mark(lo, hi, b_parent.as<int32_t>(), b_rootat.as<int32_t>(), b_first.as<uint32_t>(), s);
            launch_cup_head(lo, hi, b_rootat.as<int32_t>(), b_first.as<uint32_t>(), b_cup.as<int32_t>(), s);
        }
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
    at[(size_t)n_layers] = total;
    // the finish: the heads in run order are the cups in (layer, seed) order
    tm.mark(2, s);
    launch_cup_rows(bg, (uint32_t)rows, b_runs.as<int32_t>(), d_rowoff, b_cup.as<int32_t>(), heads.d_counts, kept.d_counts, d_cstate, s);
    const uint32_t C = heads.place((uint32_t)n_layers, s, 0, "implisolid_layer_cups: the stack reaches 2^31 cups", cup_offsets);
    cup_offsets[n_layers] = C;
    std::vector<int64_t> own(run_offsets ? 0 : (size_t)n_layers + 1);
    int64_t* ro = run_offsets ? run_offsets : own.data();
    const uint32_t K = kept.place((uint32_t)n_layers, s, 0, "implisolid_layer_cups: the stack reaches 2^31 row runs", ro);
    ro[n_layers] = K;
    if ((int64_t)C > (int64_t)K || (int64_t)K > total) throw HipError("cups: more cups than cupped runs, or more of those than runs");
    const size_t rec_bytes = (size_t)(C + 1u) * 7 * sizeof(int64_t);
    E.scratch(8).reserve(rec_bytes + (want_runs ? (size_t)(K + 1u) * 3 * sizeof(int32_t) : 0));
    long long* d_rec = E.scratch(8).as<long long>();
    int32_t* d_out = want_runs ? reinterpret_cast<int32_t*>(E.scratch(8).as<char>() + rec_bytes) : nullptr;
    launch_cup_heads(bg, (uint32_t)rows, b_runs.as<int32_t>(), d_rowoff, b_cup.as<int32_t>(), b_rootat.as<int32_t>(), heads.d_offsets, C,
                     b_first.as<uint32_t>(), d_rec, s);
    launch_cup_tally(bg, (uint32_t)rows, (uint32_t)total + 1u, b_runs.as<int32_t>(), d_rowoff, b_cup.as<int32_t>(), b_first.as<uint32_t>(), C,
                     d_rec, kept.d_offsets, K, d_out, s);
    tm.mark(3, s);
    IMPLI_HIP(hipGetLastError());
    g_cups.cups.resize((size_t)C * 7);
    if (C) IMPLI_HIP(hipMemcpyAsync(g_cups.cups.data(), d_rec, (size_t)C * 7 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (want_runs) {
        g_cups.runs.resize((size_t)K * 3);
        if (K) IMPLI_HIP(hipMemcpyAsync(g_cups.runs.data(), d_out, (size_t)K * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    CupState hc{};
    IMPLI_HIP(hipMemcpyAsync(&hc, d_cstate, sizeof hc, hipMemcpyDeviceToHost, s));
    IMPLI_HIP(hipStreamSynchronize(s));
    if (tm) tm.add(3, tm.ev[2], tm.ev[3]);
    int64_t area = 0;
    for (uint32_t c = 0; c < C; ++c) area += g_cups.cups.data()[7 * (size_t)c + 1];
    if (area != (int64_t)hc.cupped) throw HipError("cups: the records' areas and the cupped voxels disagree");
    g_cups.n_runs = want_runs ? (int64_t)K : -1;
    if (stats) {
        im.stats(stats);
        stats[5] = total;
        stats[6] = (int64_t)C;
        stats[7] = (int64_t)hc.cupped;
    }
    return (int64_t)C;
}
}  // namespace

extern "C" {

int64_t implisolid_layer_cups(const char* shape_json, int ignore_root_matrix, const float rect[4], int width, int height,
                              int supersample, const float* z, int n_layers, int threshold, int connectivity, int want_runs,
                              int64_t* cup_offsets, int64_t* run_offsets, int64_t stats[8]) {
    g_cups.reset();
    g_cups.n_runs = -1;
    return layer_entry(
        "layer_cups", cup_offsets && (run_offsets || want_runs == 0), shape_json, ignore_root_matrix, rect, width, height, supersample, z,
        n_layers, threshold,
        [&] {
            if (connectivity != 6 && connectivity != 26) throw InputError("implisolid_layer_cups: connectivity must be 6 or 26");
            if (want_runs != 0 && want_runs != 1) throw InputError("implisolid_layer_cups: want_runs must be 0 or 1");
        },
        [&](const QueryShape& q, const LayerRequest& r) {
            return g_cups.publish(cup_layers(q, r, threshold, connectivity, want_runs != 0, cup_offsets, run_offsets, stats));
        });
}

int implisolid_layer_cups_copy(int64_t* cups, int32_t* runs) {
    if (g_cups.refuses_copy("layer_cups", "cups", (g_cups.n == 0 || cups) && (g_cups.n_runs <= 0 || runs))) return -1;
    if (g_cups.n > 0) std::memcpy(cups, g_cups.cups.data(), (size_t)g_cups.n * 7 * sizeof(int64_t));
    if (g_cups.n_runs > 0) std::memcpy(runs, g_cups.runs.data(), (size_t)g_cups.n_runs * 3 * sizeof(int32_t));
    return 0;
}

int implisolid_debug_layer_cups_ms(int enable, double ms[4]) {
    return g_cup_timer.entry(enable, ms);
}

}  // extern "C"
