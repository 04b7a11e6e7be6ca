// abi_common.hpp -- what the files behind the C ABI share (abi.hip, abi_queries.hip).  Internal: not
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
