// ray_device.hpp -- what the ray kernels share (raycast.hip, rayspans.hip): a ray's points, the field at
// them under a segment's modes word, and the wave helpers of the marches (device).
#pragma once
#include "ifunc_device.hpp"
#include "ifunc_interval.hpp"

namespace impli {
namespace ray {

using namespace dev;

struct RayAt {
    float ox, oy, oz, dx, dy, dz;
};
__device__ __forceinline__ RayAt ray_at(const float* __restrict__ o, const float* __restrict__ d, size_t r) {
    return RayAt{o[3 * r], o[3 * r + 1], o[3 * r + 2], d[3 * r], d[3 * r + 1], d[3 * r + 2]};
}
// p(t): every operation rounded on its own (-ffp-contract=off)
__device__ __forceinline__ V3 ray_point(const RayAt& r, float t) {
    const float ax = t * r.dx, ay = t * r.dy, az = t * r.dz;
    return V3{r.ox + ax, r.oy + ay, r.oz + az};
}
__device__ __forceinline__ Iv span(float a, float b) { return a < b ? Iv{a, b} : Iv{b, a}; }
__device__ __forceinline__ bool finite3(const V3& p) { return fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY && fabsf(p.z) < INFINITY; }

// F at a point of a ray under the segment's modes word.  eval_f_pruned evaluates an XF_DIAG matrix as
// m_dd v + m_d3, the full row's value at finite points only (program.hpp XformPattern); at a point with an
// infinite coordinate the field is eval_f's, the full rows' (implisolid_eval_points' value there), and no
// modes word applies
template <int D>
__device__ __forceinline__ float ray_field(const Program* __restrict__ prog, const float* __restrict__ tab, uint64_t m,
                                           const V3& p) {
    if (!finite3(p)) return eval_f<D>(prog, tab, p.x, p.y, p.z);
    return eval_f_pruned<D>(prog, tab, m, p.x, p.y, p.z);
}

// lane q's 64-bit value in every lane, as a scalar
__device__ __forceinline__ uint64_t wave_bcast(uint64_t v, int q) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, q, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), q, 64);
    return ((uint64_t)__builtin_amdgcn_readfirstlane(hi) << 32) | (uint64_t)__builtin_amdgcn_readfirstlane(lo);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

}  // namespace ray
}  // namespace impli
