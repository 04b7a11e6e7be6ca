// layer_device.hpp -- what the kernels of the layer passes share (islands.hip, distance.hip, hollow.hip,
// supports.hip, runs.hip, bodies.hip, cups.hip): sums, maxima and ranks over a wave of 64 lanes, a block's sum of its
// four waves' values, the four neighbouring pixels a lane takes, the solid bits of a dword of coverage bytes, and
// the one-way minimum and maximum onto a record's field.
// Device-only, and no part of the JIT's headers.  Internal linkage: every file that includes this has its own
// copies, inlined into its kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"   // LayerGrid

namespace impli {

namespace {

typedef unsigned long long u64;

// ---- over the wave ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}
// a 64-bit value from another lane, as two 32-bit halves
__device__ __forceinline__ u64 shfl_xor64(u64 v, int d) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_up64(u64 v, int d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u64 o = shfl_xor64(v, d);
        v = o > v ? o : v;
    }
    return v;
}
// the set bits of the four ballots of bits 0 .. 3 of `bits` in the lanes below this one, and in `all` in every lane
__device__ __forceinline__ uint32_t ranks_below(uint32_t bits, uint32_t& all) {
    uint32_t below = 0;
    all = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const u64 m = __ballot((bits >> k) & 1u);
        below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, below));
        all += (uint32_t)__popcll(m);
    }
    return below;
}

// ---- over a block of four waves ----------------------------------------------------------------------------
// A value per wave, summed over the block, in two halves around a __syncthreads() of the caller's: wave_put
// leaves the wave's value (its lane 0's) in s[wave], four words of the caller's LDS; behind the barrier block_sum
// adds them, for the one thread that lands the result (or for all).
__device__ __forceinline__ void wave_put(uint32_t* s, uint32_t v) {
    const int t = threadIdx.x;
    if ((t & 63) == 0) s[t >> 6] = v;
}
__device__ __forceinline__ uint32_t block_sum(const uint32_t* s) { return s[0] + s[1] + s[2] + s[3]; }

// ---- four neighbouring pixels per lane ---------------------------------------------------------------------
// A layer's pixels in groups of four of one row, x4 .. x4 + 3 with x4 a multiple of 4, kGroups to a block: group
// b kGroups + t of the layer goes to thread t of the layer's block b.  Where W is a multiple of 4 a group is 16
// aligned bytes of an int32 [H][W] layer (kVec), and in any case four aligned bytes of the image.
constexpr uint32_t kGroups = 256;   // one per lane
struct PixelGroup {
    bool active;        // the group lies in the layer; y, x4, nv and at are 0 where it does not
    uint32_t y, x4;
    uint32_t nv;        // the group's pixels inside the row
    size_t at;          // the group in an [H][W] layer: y W + x4
};
__device__ __forceinline__ PixelGroup pixel_group(int Wi, int Hi, uint32_t b, int t) {
    const uint32_t W = (uint32_t)Wi, gpr = (W + 3u) / 4u;        // groups per row
    const uint32_t gi = b * kGroups + (uint32_t)t;
    PixelGroup p;
    p.active = gi < gpr * (uint32_t)Hi;                          // <= 2^26
    p.y = p.active ? gi / gpr : 0u;
    p.x4 = p.active ? (gi % gpr) * 4u : 0u;
    p.nv = p.active ? (W - p.x4 < 4u ? W - p.x4 : 4u) : 0u;
    p.at = (size_t)p.y * W + p.x4;
    return p;
}
// the blocks that cover one layer's groups
constexpr uint32_t groups_blocks(const LayerGrid& g) {
    const uint32_t gpr = ((uint32_t)g.W + 3u) / 4u;
    return (gpr * (uint32_t)g.H + kGroups - 1u) / kGroups;   // <= 2^18
}
// the int32 of an active group at p into v: kVec reads the four together, else the nv inside the row one by one
// and the others keep what v held.  The caller guards: the vector load is unconditional
template <bool kVec>
__device__ __forceinline__ void load4(const int32_t* p, uint32_t nv, int (&v)[4]) {
    if (kVec) {
        const int4 a = *reinterpret_cast<const int4*>(p);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
            if (i < nv) v[i] = p[i];
    }
}

// ---- coverage bytes ------------------------------------------------------------------------------------------
// the dword of four coverage bytes at p (4-byte aligned: the pitch is a multiple of 16), 0 where `in` is false
__device__ __forceinline__ uint32_t cov_load4(const uint8_t* p, bool in) {
    return in ? *reinterpret_cast<const uint32_t*>(p) : 0u;
}
// byte i of cov4 is solid; and bit i of the result: byte i is
__device__ __forceinline__ bool cov_solid(uint32_t cov4, uint32_t i, int threshold) {
    return (int)((cov4 >> (8u * i)) & 0xffu) >= threshold;
}
__device__ __forceinline__ uint32_t cov_solid4(uint32_t cov4, int threshold) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) s |= (uint32_t)cov_solid(cov4, i, threshold) << i;
    return s;
}

// ---- records that waves add to ----------------------------------------------------------------------------------
// min and max onto a record's field.  Both only ever move one way, so a field that already holds a value at
// least as small (as large) stays as it is whatever lands later, and the atomic is left out: a body's extent
// settles after a few runs, and the thousands that follow would queue up on its record for nothing.
__device__ __forceinline__ void rec_min(long long* p, long long v) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v) __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void rec_max(long long* p, long long v) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

}  // namespace impli
