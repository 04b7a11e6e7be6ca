// abi_common.hpp -- what the files behind the C ABI share (abi.hip, abi_queries.hip, abi_layers.hip).  Internal: not
// installed, not part of include/.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>

#include "engine.hpp"

namespace impli {
namespace cabi {

// ---- one definition each, in abi.hip ---------------------------------------------------------------
// sets the thread's last error and prints it; aborts where the reference does (error mode 0)
void report(const std::string& msg, bool reference_aborts);
std::string& last_error();      // the thread's last error (implisolid_last_error)
Engine& engine();               // the process's engine, created at the first call
hipStream_t abi_stream();       // and its stream

// The descent of eval.hip's k_bounds_level (abi_queries.hip); the "fit_box" settings key runs it too.
bool compute_bounds(Engine& E, hipStream_t s, const Program* d_prog, int prog_depth, const float* d_tab,
                    const float search[6], int depth, float out[6], int64_t stats[4]);

// Host results in pinned memory (D2H at full PCIe rate, where pageable memory goes through the
// driver's staging copies) that resize() does not zero (a vector zero-filled 13 MB per 512^3 build
// before the copy overwrote it).  Grow-only; kept until exit.
template <class T>
struct PinnedVec {
    T* p = nullptr;
    size_t n = 0, cap = 0;
    size_t size() const { return n; }
    T* data() { return p; }
    const T* data() const { return p; }
    void resize(size_t m) {
        if (m > cap) {
            const size_t nc = std::max(m, cap + cap / 2);
            T* q = nullptr;
            if (hipHostMalloc((void**)&q, nc * sizeof(T), hipHostMallocDefault) != hipSuccess || !q)
                throw HipError("host mesh: pinned allocation failed");
            if (n) std::memcpy(q, p, n * sizeof(T));
            if (p) (void)hipHostFree(p);
            p = q;
            cap = nc;
        }
        n = m;
    }
};

// ---- the catch tail of an extern "C" entry -----------------------------------------------------------
// Both run the body and return its value; an exception is reported and becomes -1.
// A device entry: an InputError is the caller's mistake, which the reference answers by aborting;
// anything else may have left work in flight, which is drained before the entry returns.
template <class Body>
auto guard_device(Body&& body) -> decltype(body()) {
    try {
        return body();
    } catch (const InputError& e) {
        report(e.what(), true);
    } catch (const std::exception& e) {
        (void)hipDeviceSynchronize();
        report(e.what(), false);
    }
    return -1;
}
// A host-only entry (no counterpart in the reference: nothing aborts).  Clears the last error first.
template <class Body>
auto guard_host(Body&& body) -> decltype(body()) {
    last_error().clear();
    try {
        return body();
    } catch (const std::exception& e) {
        report(e.what(), false);
    }
    return -1;
}

// ---- a query's shape ---------------------------------------------------------------------------------
// Compiled on the host by the constructor (InputError for a bad shape), put on the current device by
// upload(): the shape's own sdf_3d tables (the engine's rabbit section first either way) and its own
// copy of the program -- the engine's object, if any, is left alone.  Freed on every path.
struct QueryShape {
    ObjectTables tabs;
    Program prog;
    Engine* E = nullptr;
    hipStream_t s = nullptr;
    const float* d_tab = nullptr;
    const Program* d_prog = nullptr;
    int max_depth;
    QueryShape(const char* shape_json, int ignore_root_matrix)
        : prog(compile_mp5(shape_json, ignore_root_matrix != 0, &tabs)), max_depth(prog.max_depth) {}
    QueryShape(const QueryShape&) = delete;
    ~QueryShape() { prog_buf_.release(); }
    void upload() {
        E = &engine();
        s = abi_stream();
        d_tab = arena_.set(tabs, E->d_rabbit());
        prog_buf_.reserve(sizeof(Program));
        IMPLI_HIP(hipMemcpy(prog_buf_.p, &prog, sizeof(Program), hipMemcpyHostToDevice));
        d_prog = prog_buf_.as<Program>();
    }
private:
    TableArena arena_;
    DevBuf prog_buf_;
};

// ---- limits the environment may replace ----------------------------------------------------------------
// A value > 0 replaces the default; the result is clamped to the maximum.  Read at every call: the
// tests force several chunks and the rerun paths this way.
inline uint64_t env_limit(const char* name, uint64_t dflt, uint64_t max) {
    if (const char* e = std::getenv(name)) {
        const long long v = std::atoll(e);
        if (v > 0) dflt = (uint64_t)v;
    }
    return std::min(dflt, max);
}
// whole layers per chunk, from at most max_items (layer, tile) items per chunk
inline uint32_t chunk_layers(const char* name, uint64_t max_items, uint32_t tiles_per_layer, int n_layers) {
    const uint64_t items = env_limit(name, max_items, max_items);
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(items / tiles_per_layer, 1), (uint64_t)n_layers);
}
// the two box lists of a descent to `depth`: 8 N^2 boxes by default (a surface crossing the whole box
// lists about 6 N^2 at the last level)
inline uint32_t list_capacity(const char* name, int depth) {
    return (uint32_t)env_limit(name, std::min<uint64_t>(std::max<uint64_t>(8ull << (2 * depth), 4096), 1ull << 21), kBoundsMaxList);
}
// ... and after a run that overflowed them: twice as many, and at least the longest list seen in
// count[lo, hi) (the counts kept counting past the capacity)
inline uint32_t grown_capacity(const char* who, uint32_t cap, const uint32_t* count, int lo, int hi) {
    if (cap >= kBoundsMaxList) throw HipError(std::string(who) + ": list overflow at the largest capacity");
    uint64_t want = 2ull * cap;
    for (int l = lo; l < hi; ++l) want = std::max<uint64_t>(want, count[l]);
    return (uint32_t)std::min<uint64_t>(want, kBoundsMaxList);
}

// ---- HIP events for the debug timers: created on request, destroyed with the scope -----------------------
template <int N>
struct EventSet {
    hipEvent_t e[N] = {};
    EventSet() = default;
    EventSet(const EventSet&) = delete;
    ~EventSet() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    void create() {
        for (hipEvent_t& x : e) IMPLI_HIP(hipEventCreate(&x));
    }
    hipEvent_t operator[](int k) const { return e[k]; }   // null unless created
};

// What follows to the state block is the queries' own host scaffolding: in an unnamed namespace, so that none of
// it adds to the library's exported symbols.
namespace {

// ---- a query's pass timer (implisolid_debug_<query>_ms) ---------------------------------------------------
// The contract: the figures are -1 before any timed call; a timed call zeroes them at its start and adds each
// chunk's intervals; an untimed call leaves the last timed call's figures; the switch is read at the start of
// a call.  PassTimer is the query's global: the switch and the N figures.  Timed is a call's own: its E events,
// null in an untimed call, where mark() does nothing and the call, tested as a bool, skips its add()s.
template <int N>
struct PassTimer {
    bool on = false;
    double ms[N];
    PassTimer() { std::fill(ms, ms + N, -1.0); }
    int entry(int enable, double* out) {   // the debug entry: sets the switch, copies the last figures out
        on = enable != 0;
        if (out) std::copy(ms, ms + N, out);
        return 0;
    }
};
template <int N, int E>
struct Timed {
    PassTimer<N>& t;
    EventSet<E> ev;
    explicit Timed(PassTimer<N>& t, bool zero = true) : t(t) {
        if (!t.on) return;
        ev.create();
        if (zero) std::fill(t.ms, t.ms + N, 0.0);
    }
    explicit operator bool() const { return ev[0] != nullptr; }
    void mark(int k, hipStream_t s) {
        if (ev[k]) IMPLI_HIP(hipEventRecord(ev[k], s));
    }
    static float elapsed(hipEvent_t a, hipEvent_t b) {   // both recorded, and the stream synchronised behind b
        float ms = 0.f;
        IMPLI_HIP(hipEventElapsedTime(&ms, a, b));
        return ms;
    }
    void add(int k, hipEvent_t a, hipEvent_t b) { t.ms[k] += elapsed(a, b); }
    void add(int k, float ms) { t.ms[k] += ms; }
};

// ---- a counted output: per-item counts -> offsets -> records ------------------------------------------------
// A chunk's items (tiles, rows, rays) each count their records; the exclusive scan of the counts places them,
// and the host needs the offset of every group of `stride` items (a layer's tiles or rows) and the chunk's
// total, which sizes the records.  stride 0: every item is a group of its own (a ray), and the offsets are read
// back as they are, with no gather.  The constructor carves the scan's buffers for at most cap items out of b,
// which holds nothing else: the counts unless the query keeps them elsewhere, cap + 1 offsets, launch_scan_u32's
// sums, and with a stride the group offsets.
struct CountedOutput {
    uint32_t *d_counts, *d_offsets, *d_sums, *d_groups;
    uint32_t stride;
    std::vector<uint32_t> off;   // the chunk's group offsets and its total, read back

    CountedOutput(DevBuf& b, size_t cap, uint32_t stride, uint32_t* counts_elsewhere = nullptr) : stride(stride) {
        const size_t counts = counts_elsewhere ? 0 : cap, sums = cap / 4096 + 2, groups = stride ? cap / stride + 1 : 0;
        b.reserve((counts + cap + 1 + sums + groups) * sizeof(uint32_t));
        d_counts = counts_elsewhere ? counts_elsewhere : b.as<uint32_t>();
        d_offsets = b.as<uint32_t>() + counts;
        d_sums = d_offsets + cap + 1;
        d_groups = stride ? d_sums + sums : d_offsets;
        off.resize(stride ? groups : cap + 1);
    }

    // Behind the launch that filled d_counts for `groups` groups: enqueues the scan (and the gather of every
    // stride-th offset, with a stride), then behind() -- what the query enqueues ahead of the read-back --, reads the group
    // offsets back and synchronises the stream.  A result of total + the chunk's records >= 2^31 is refused with
    // `limit`; else out[k] = total + the offset of group k, and the chunk's records are returned.
    template <class Behind>
    uint32_t place(uint32_t groups, hipStream_t s, int64_t total, const char* limit, int64_t* out, Behind&& behind) {
        launch_scan_u32(d_counts, d_offsets, (int64_t)groups * (stride ? stride : 1), d_sums, false, s);
        if (stride) launch_slice_layer_offsets(d_offsets, stride, groups, d_groups, s);
        behind();
        IMPLI_HIP(hipGetLastError());
        IMPLI_HIP(hipMemcpyAsync(off.data(), d_groups, ((size_t)groups + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        IMPLI_HIP(hipStreamSynchronize(s));
        const uint32_t* h = off.data();   // a local: the loop below runs over a million rays
        const uint32_t records = h[groups];
        if (total + (int64_t)records >= ((int64_t)1 << 31)) throw InputError(limit);
        for (uint32_t k = 0; k < groups; ++k) out[k] = total + h[k];
        return records;
    }
    uint32_t place(uint32_t groups, hipStream_t s, int64_t total, const char* limit, int64_t* out) {
        return place(groups, s, total, limit, out, [] {});
    }
};

// ---- the result slot of a query whose records the caller fetches with implisolid_<entry>_copy ----------------
// n < 0: none.  The entry resets the slot before anything else -- whatever happens, the previous result is gone
// -- and publishes the count behind the last pass.  A query's slot adds its pinned arrays.
struct ResultSlot {
    int64_t n = -1;
    void reset() { n = -1; }
    int64_t publish(int64_t count) { return n = count; }
    // The head of implisolid_<entry>_copy: clears the last error; true, with the refusal reported, where there
    // is no result or the caller's pointers do not serve (have_pointers: as the entry requires them).
    bool refuses_copy(const std::string& entry, const char* noun, bool have_pointers) const {
        last_error().clear();
        if (n >= 0 && have_pointers) return false;
        const std::string who = "implisolid_" + entry;
        report(n < 0 ? who + "_copy: no " + noun + " to copy (the last " + who + " failed, or none ran)" : who + "_copy: bad arguments",
               false);
        return true;
    }
};

// ---- two staging slots for a chunked query's records ----------------------------------------------------------
// A chunk's records come down into one of two pinned staging slots, and the host moves them on to the result while
// the device works on the next chunk.  The order: begin() at the head of a chunk, behind a synchronisation (the
// chunk before has landed in the other slot), gives the chunk's slot; staged(at, n), behind the chunk's copies
// into that slot, moves the chunk before out of the other slot and notes this one: n items for position `at` of
// the result; finish(), behind the call's last synchronisation, moves the last chunk.  move(slot, at, n) is the
// query's: what to move and where from.  No call of these synchronises.  The staging arrays are the query's,
// grow-only and kept until exit; restage() sizes one for a chunk with nothing of an earlier chunk kept.
template <class Move>
struct StagingSlots {
    Move move;
    int slot = 1;        // of the chunk in hand
    size_t at = 0;
    uint32_t n = 0;      // the chunk on its way into a slot, not yet in the result; 0: none
    explicit StagingSlots(Move m) : move(m) {}
    int begin() { return slot ^= 1; }
    void staged(size_t at_, uint32_t n_) {
        flush(slot ^ 1);
        at = at_;
        n = n_;
    }
    void finish() { flush(slot); }
private:
    void flush(int from) {
        if (n) move(from, at, n);
        n = 0;
    }
};
template <class T>
void restage(PinnedVec<T>& v, size_t n) {
    v.resize(0);
    v.resize(n);
}

// ---- the layer a chunk leaves for the next ---------------------------------------------------------------------
// The first layer of a chunk reads the layer below it, the last of the chunk before: n items of b, reserved only
// where the call has more than one chunk (d is null otherwise: the first chunk reads none).
template <class T>
struct CarriedLayer {
    T* d = nullptr;
    size_t n;
    CarriedLayer(DevBuf& b, size_t n, bool chunked) : n(n) {
        if (!chunked) return;
        b.reserve(n * sizeof(T));
        d = b.as<T>();
    }
    // behind the chunk's passes: its last layer, where a chunk follows
    void keep(const T* d_last, bool more, hipStream_t s) {
        if (more) IMPLI_HIP(hipMemcpyAsync(d, d_last, n * sizeof(T), hipMemcpyDeviceToDevice, s));
    }
};

}  // namespace

// ---- the state block of a query's passes ------------------------------------------------------------------
// kStateBytes at the head of a scratch buffer hold the passes' State; the query's tables follow
constexpr size_t kStateBytes = 256;
template <class State, class T = float>
T* behind_state(const DevBuf& b) {
    static_assert(sizeof(State) <= kStateBytes, "the tables follow the state block");
    return reinterpret_cast<T*>(b.as<char>() + kStateBytes);
}

}  // namespace cabi
}  // namespace impli
