// raycast.hip -- rays against the solid on gfx950 (implisolid_raycast): per ray the first of the N + 1
// samples ts[k] of its line p(t) = o + t d that is solid (!(F < 0)), then B bisection rounds inside the
// bracket [ts[k - 1], ts[k]] and the normal at the returned point.  The sample table ts is computed on
// the host (host.hpp ray_params) and only indexed here.
//
// k_ray_march  : one wave per ray, four rays per block.  A ray is cut into segments of 64 steps
//                (segment j = samples 64 j .. min(64 j + 64, N), both ends included).  With pruning, lane
//                i of a batch bounds segment j0 + i: rounded multiplication and addition are monotone
//                and ts is non-decreasing, so every coordinate of every p(t) with t in the segment lies
//                between those of its two end points, and the interval interpreter over that box bounds
//                every sample and every bisection midpoint of the segment.  hi < 0 proves the segment
//                outside.  One ballot marks the others; the wave walks them in order, broadcasts the
//                segment's modes word (wave-uniform skips in eval_f_pruned) and evaluates the samples
//                64 j + 1 + lane, for segment 0 sample 0 on lane 0 first.  The lowest solid lane is the
//                hit and ends the walk.  Without pruning every segment is walked with modes word 0.
//                Per ray: hit, the hit segment's modes word, F(ts[hit]) and the work done.
//                t * d may overflow the float range (o, d and ts are finite, p(t) need not be).  The
//                bound speaks of finite boxes only, so a segment with an end point that is not finite is
//                never proved outside and is walked with modes word 0; its points that are not finite
//                take the field of the full matrix rows (ray_field), where 0 * inf = NaN is solid.
// k_ray_finish : one lane per ray.  hit >= 1 bisects with its segment's modes word; hit >= 0 takes the
//                normal from vertex_normal_at, the rule of launch_vertex_normals; t, f and the normal
//                are written; the work figures of the wave's rays are summed and added with one atomic
//                per wave and counter.
// No result depends on the pruning level, the chunks or the order of any atomic.
#include <stdexcept>

#include "ifunc_device.hpp"
#include "ifunc_interval.hpp"
#include "ob02_device.hpp"
#include "ray_device.hpp"
#include "kernels.hpp"

namespace impli {

using namespace dev;
using namespace ray;   // RayAt, ray_point, span, finite3, ray_field, wave_bcast, wave_sum

namespace {

typedef unsigned long long u64;
constexpr int kSeg = kRaySegment;
static_assert(kSeg == 64, "one sample of a segment per lane");

template <int D>
__global__ __launch_bounds__(256) void k_ray_march(const Program* __restrict__ prog, const float* __restrict__ tab,
                                                    float2 tab_range, const float* __restrict__ ts,
                                                    const float* __restrict__ org, const float* __restrict__ dir, uint32_t n,
                                                    int N, int prune, int32_t* __restrict__ hit,
                                                    uint64_t* __restrict__ hmodes, float* __restrict__ fhit,
                                                    uint32_t* __restrict__ work) {
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t r = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (r >= n) return;   // the whole wave: nothing below crosses waves
    const RayAt ray = ray_at(org, dir, r);
    const int nseg = (N + kSeg - 1) / kSeg;
    int k_hit = -1;
    uint64_t m_hit = 0;
    float f_hit = 0.f;
    uint32_t skipped = 0, evaluated = 0;
    for (int j0 = 0; j0 < nseg && k_hit < 0; j0 += 64) {
        const int seg = j0 + lane;
        const bool valid = seg < nseg;
        uint64_t m = 0;
        bool outside = false;
        if (prune && valid) {
            // ts[kSeg seg] and ts[min(kSeg seg + kSeg, N)]: indices within 0 .. N
            const int k1 = min(kSeg * seg + kSeg, N);
            const V3 a = ray_point(ray, ts[kSeg * seg]), b = ray_point(ray, ts[k1]);
            const Iv iv = eval_iv<D>(prog, tab, tab_range, Box{span(a.x, b.x), span(a.y, b.y), span(a.z, b.z)}, 0ull, m);
            const bool fin = finite3(a) && finite3(b);   // then every point between them is finite
            outside = fin && iv.hi < 0.f;                // a NaN bound proves nothing
            if (!fin) m = 0;
        }
        const uint64_t skipm = (uint64_t)__ballot(valid && outside);
        uint64_t live = (uint64_t)__ballot(valid && !outside);
        uint64_t before = ~0ull;   // the batch's segments up to the hit segment
        while (live && k_hit < 0) {
            const int q = __builtin_ctzll((u64)live);
            live &= live - 1ull;
            ++evaluated;
            const uint64_t mq = wave_bcast(m, q);
            const int sg = j0 + q;
            // segment 0 holds sample 0 as well: lane 0 takes it in a pass of its own
            for (int pass = sg == 0 ? 0 : 1; pass < 2 && k_hit < 0; ++pass) {
                const int k = pass == 0 ? 0 : kSeg * sg + 1 + lane;
                const bool has = pass == 0 ? lane == 0 : k <= N;
                float f = -1.f;
                if (has) {
                    const V3 p = ray_point(ray, ts[k]);
                    f = ray_field<D>(prog, tab, mq, p);
                }
                const uint64_t hm = (uint64_t)__ballot(has && !(f < 0.f));   // marching cubes' rule: -0.0 and NaN are solid
                if (hm) {
                    const int L = __builtin_ctzll((u64)hm);
                    k_hit = __shfl(k, L, 64);
                    f_hit = __shfl(f, L, 64);
                    m_hit = mq;
                    before = (1ull << q) - 1ull;
                }
            }
        }
        skipped += (uint32_t)__popcll((u64)(skipm & before));
    }
    if (lane == 0) {
        hit[r] = k_hit;
        hmodes[r] = m_hit;
        fhit[r] = f_hit;
        work[r] = skipped | (evaluated << 16);   // at most 1024 segments a ray
    }
}

template <int D>
__global__ __launch_bounds__(256) void k_ray_finish(const Program* __restrict__ prog, const float* __restrict__ tab,
                                                     const float* __restrict__ ts, const float* __restrict__ org,
                                                     const float* __restrict__ dir, uint32_t n, int N, int B,
                                                     const int32_t* __restrict__ hit, const uint64_t* __restrict__ hmodes,
                                                     const float* __restrict__ fhit, const uint32_t* __restrict__ work,
                                                     float* __restrict__ t_out, float* __restrict__ f_out,
                                                     float* __restrict__ normals, RayState* __restrict__ st) {
    // whole waves run to the end (the sums cover the wave)
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t c_skip = 0, c_eval = 0, c_hit = 0, c_in = 0;
    if (i < n) {
        const int h = hit[i];
        const uint32_t wk = work[i];
        c_skip = wk & 0xffffu;
        c_eval = wk >> 16;
        c_hit = h >= 0 ? 1u : 0u;
        c_in = h == 0 ? 1u : 0u;
        float t = ts[N], f = 0.f;
        V3 nrm{0.f, 0.f, 0.f};
        if (h >= 0) {
            const RayAt ray = ray_at(org, dir, i);
            t = ts[h];
            f = fhit[i];
            if (h >= 1) {
                const uint64_t m = hmodes[i];
                float a = ts[h - 1];
                for (int round = 0; round < B; ++round) {
                    const float mid = a + 0.5f * (t - a);
                    if (mid == a || mid == t) break;   // every later round repeats this one
                    const V3 p = ray_point(ray, mid);
                    const float fm = ray_field<D>(prog, tab, m, p);
                    if (!(fm < 0.f)) {
                        t = mid;
                        f = fm;
                    } else {
                        a = mid;
                    }
                }
            }
            if (normals) {
                const V3 p = ray_point(ray, t);
                (void)ob::vertex_normal_at(ob::InterpPt<D>{prog, tab}, p.x, p.y, p.z, nrm);
            }
        }
        t_out[i] = t;
        f_out[i] = f;
        if (normals) {
            normals[3 * (size_t)i] = nrm.x;
            normals[3 * (size_t)i + 1] = nrm.y;
            normals[3 * (size_t)i + 2] = nrm.z;
        }
    }
    c_skip = wave_sum(c_skip);
    c_eval = wave_sum(c_eval);
    c_hit = wave_sum(c_hit);
    c_in = wave_sum(c_in);
    if ((threadIdx.x & 63u) == 0u) {
        if (c_skip) atomicAdd(&st->skipped, (u64)c_skip);
        if (c_eval) atomicAdd(&st->evaluated, (u64)c_eval);
        if (c_hit) atomicAdd(&st->hits, (u64)c_hit);
        if (c_in) atomicAdd(&st->inside, (u64)c_in);
    }
}

void check_chunk(uint32_t n, int N, int B) {
    if (n < 1u || n > kRayMaxChunk) throw std::runtime_error("raycast: chunk size out of range");
    if (N < 1 || N > kRayMaxSteps || B < 0 || B > kRayMaxBisect) throw std::runtime_error("raycast: steps or bisect out of range");
}

}  // namespace

void launch_ray_march(const Program* d_prog, int prog_depth, const float* d_tab, float2 tab_range, const float* d_ts,
                      const float* d_org, const float* d_dir, uint32_t n, int N, bool prune, int32_t* d_hit,
                      uint64_t* d_hmodes, float* d_fhit, uint32_t* d_work, hipStream_t s) {
    check_chunk(n, N, 0);
    const unsigned blocks = (n + 3u) / 4u;
    const int D = eval_depth(prog_depth), p = prune ? 1 : 0;
#define IMPLI_RAY_MARCH(DD) \
    k_ray_march<DD><<<blocks, 256, 0, s>>>(d_prog, d_tab, tab_range, d_ts, d_org, d_dir, n, N, p, d_hit, d_hmodes, d_fhit, d_work)
    if (D <= 4) IMPLI_RAY_MARCH(4);
    else if (D <= 8) IMPLI_RAY_MARCH(8);
    else if (D <= 12) IMPLI_RAY_MARCH(12);
    else IMPLI_RAY_MARCH(16);
#undef IMPLI_RAY_MARCH
}

void launch_ray_finish(const Program* d_prog, int prog_depth, const float* d_tab, const float* d_ts, const float* d_org,
                       const float* d_dir, uint32_t n, int N, int B, const int32_t* d_hit, const uint64_t* d_hmodes,
                       const float* d_fhit, const uint32_t* d_work, float* d_t, float* d_f, float* d_normals,
                       RayState* d_state, hipStream_t s) {
    check_chunk(n, N, B);
    const unsigned blocks = (n + 255u) / 256u;
    const int D = eval_depth(prog_depth);
#define IMPLI_RAY_FINISH(DD) \
    k_ray_finish<DD><<<blocks, 256, 0, s>>>(d_prog, d_tab, d_ts, d_org, d_dir, n, N, B, d_hit, d_hmodes, d_fhit, d_work, d_t, d_f, d_normals, d_state)
    if (D <= 4) IMPLI_RAY_FINISH(4);
    else if (D <= 8) IMPLI_RAY_FINISH(8);
    else if (D <= 12) IMPLI_RAY_FINISH(12);
    else IMPLI_RAY_FINISH(16);
#undef IMPLI_RAY_FINISH
}

}  // namespace impli
