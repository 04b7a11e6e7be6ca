// unionfind_device.hpp -- the lock-free union-find of the labelling kernels (islands.hip, bodies.hip): an int
// array in which every entry holds the index of a member of its own class that is not larger than its own;
// following entries ends at a root (entry == own index), the smallest index of the class once all joins are in.
// Every loop is bounded by the input: a find walks strictly decreasing indices, and in a union the larger of
// the two indices strictly decreases from round to round (see unite()), so both end after at most `index`
// steps.  Internal linkage: every file that includes this has its own copies, inlined into its kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace impli {

namespace {

// ---- union-find, the smaller index is the parent --------------------------------------------------------
// LDS flavour: volatile reads (another lane's atomicMin must be seen)
__device__ __forceinline__ int find_lds(const volatile int* L, int x) {
    int p;
    while ((p = L[x]) != x) x = p;   // p < x: strictly decreasing
    return x;
}
// global flavour: relaxed device-scope loads, not served from a stale cache line
__device__ __forceinline__ int find_glb(int* L, int x) {
    int p;
    while ((p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != x) x = p;
    return x;
}
// Joins the classes of a and b.  With a > b both roots, atomicMin(&L[a], b) returns a when a was still a
// root: done.  Otherwise another lane has pointed a at old < a in the meantime and L[a] is now min(old, b),
// a member of the class either way; what remains is to join old and b, both < a: the larger index of the
// pair has strictly decreased, which bounds the rounds.
template <bool LDS>
__device__ __forceinline__ void unite(int* L, int a, int b) {
    for (;;) {
        a = LDS ? find_lds(L, a) : find_glb(L, a);
        b = LDS ? find_lds(L, b) : find_glb(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&L[a], b);
        if (old == a) return;
        a = old;
    }
}

}  // namespace

}  // namespace impli
