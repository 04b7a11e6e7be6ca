// slice.hip -- per-layer contours of the solid on gfx950 (implisolid_slice): marching squares on the
// planes z = z[l] over an R x R-cell grid, in tiles of 16 x 16 cells.
//
// k_slice_classify : one thread per (layer, tile).  With pruning the tile's box (its end samples in x
//                    and y, {z, z}) is bounded by the interval interpreter: a sign-definite tile holds
//                    only case-0 or case-15 cells and is dropped, a mixed one (a NaN bound included)
//                    is listed with the modes word the bound returned.  Without pruning every tile is
//                    listed with modes word 0.  The append costs one atomic per wave; the list's
//                    order is arbitrary and nothing downstream depends on it.
// k_slice_march    : one block of 320 lanes per listed tile: lane t < 289 evaluates sample (t % 17,
//                    t / 17) of the tile (eval_f_pruned with the tile's modes word: bit-identical to
//                    eval_f inside the box), stores it in LDS and in the tile's slot of the sample
//                    scratch; then one cell per lane (t < 256) looks up its case, and the block's
//                    segment count goes to counts[layer, tile] -- dense, zero for unlisted tiles.
//                    Border samples are evaluated by both tiles that share them: same operands, same
//                    bits.
// (scan)           : ob02.hip's exclusive scan of the dense counts: the tile offsets.
// k_slice_emit     : one block of 256 lanes per listed tile: the stored samples back into LDS, the
//                    cell's case, a block prefix of the cells' segment counts in cell row-major order,
//                    and the segments and keys at tile offset + prefix.  Positions come from the scan
//                    and the prefix alone.
#include <stdexcept>

#include "ifunc_device.hpp"
#include "ifunc_interval.hpp"
#include "brick_modes.hpp"
#include "kernels.hpp"

namespace impli {

using namespace dev;

namespace {

constexpr int kT = kSliceTile, kS = kSliceSide;
constexpr int kMarchBlock = 320;   // five waves: 289 samples, one each
static_assert(kMarchBlock >= kSliceSamples && kMarchBlock % 64 == 0 && kT * kT == 256, "one sample and one cell per lane");

// Segments per case, packed: count | start0 << 2 | end0 << 4 | start1 << 6 | end1 << 8 (edges e0
// bottom, e1 right, e2 top, e3 left; solid on the left of start -> end; the saddles 5 and 10 cut their
// two solid corners off separately)
__host__ __device__ constexpr uint32_t seg1(int a, int b) { return 1u | (uint32_t)a << 2 | (uint32_t)b << 4; }
__host__ __device__ constexpr uint32_t seg2(int a, int b, int c, int d) {
    return 2u | (uint32_t)a << 2 | (uint32_t)b << 4 | (uint32_t)c << 6 | (uint32_t)d << 8;
}
// (a table in constant memory: a function-local array indexed by the case was built on the stack)
__constant__ const uint32_t kCaseSegments[16] = {0u,         seg1(0, 3), seg1(1, 0), seg1(1, 3), seg1(2, 1), seg2(0, 3, 2, 1),
                                                 seg1(2, 0), seg1(2, 3), seg1(3, 2), seg1(0, 2), seg2(1, 0, 3, 2), seg1(1, 2),
                                                 seg1(3, 1), seg1(0, 1), seg1(3, 0), 0u};
__device__ __forceinline__ uint32_t case_segments(uint32_t c) { return kCaseSegments[c]; }

struct TileAt {
    int l, tx, ty, nx, ny;   // layer, tile, its cells per axis (16, fewer at the border)
};
__device__ __forceinline__ TileAt tile_at(const SliceGrid& g, int64_t item) {
    TileAt t;
    t.l = (int)(item / g.tpl);
    const uint32_t k = (uint32_t)(item % g.tpl);
    t.ty = (int)(k / (uint32_t)g.ntx);
    t.tx = (int)(k % (uint32_t)g.ntx);
    t.nx = min(kT, g.R - kT * t.tx);
    t.ny = min(kT, g.R - kT * t.ty);
    return t;
}

// a cell's corner samples from the tile's in LDS (named members: an array indexed by the edge number
// went to scratch), and its case: bit k set iff corner k is solid, !(f < 0)
struct Corners { float f0, f1, f2, f3; };
__device__ __forceinline__ Corners cell_corners(const float* s_f, int ci, int cj) {
    return Corners{s_f[cj * kS + ci], s_f[cj * kS + ci + 1], s_f[(cj + 1) * kS + ci + 1], s_f[(cj + 1) * kS + ci]};
}
__device__ __forceinline__ uint32_t cell_case(const Corners& c) {
    return (c.f0 < 0.f ? 0u : 1u) | (c.f1 < 0.f ? 0u : 2u) | (c.f2 < 0.f ? 0u : 4u) | (c.f3 < 0.f ? 0u : 8u);
}

template <int D>
__global__ __launch_bounds__(256) void k_slice_classify(const Program* __restrict__ prog, const float* __restrict__ tab,
                                                         float2 tab_range, const float* __restrict__ xs,
                                                         const float* __restrict__ ys, const float* __restrict__ z,
                                                         SliceGrid g, int64_t first, uint32_t n, int prune,
                                                         uint32_t* __restrict__ list, uint64_t* __restrict__ lmodes,
                                                         SliceState* __restrict__ st) {
    // whole waves run to the end (the append's ballot covers the wave)
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool live = i < n;
    const TileAt t = tile_at(g, first + (live ? i : 0u));
    bool push = live;
    uint64_t m = 0;
    if (live && prune) {
        // the tile's samples lie between its end samples: xs, ys are monotone in the index
        const float zl = z[t.l];
        const Box b{Iv{xs[kT * t.tx], xs[kT * t.tx + t.nx]}, Iv{ys[kT * t.ty], ys[kT * t.ty + t.ny]}, Iv{zl, zl}};
        push = sign_class(eval_iv<D>(prog, tab, tab_range, b, 0ull, m)) == kBrickMixed;
    }
    const uint64_t pm = __ballot(push);
    if (!pm) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&st->n_listed, (uint32_t)__popcll((unsigned long long)pm));
    base = (uint32_t)__shfl((int)base, 0, 64);
    const uint32_t at = base + (uint32_t)__popcll((unsigned long long)(pm & ((1ull << lane) - 1ull)));
    if (push && at < n) {   // at < n always: every item is appended at most once
        list[at] = i;
        lmodes[at] = m;
    }
    uint32_t ns = push ? (uint32_t)((t.nx + 1) * (t.ny + 1)) : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ns += (uint32_t)__shfl_xor((int)ns, o, 64);
    if (lane == 0) atomicAdd(&st->samples, (unsigned long long)ns);
}

template <int D>
__global__ __launch_bounds__(kMarchBlock) void k_slice_march(const Program* __restrict__ prog,
                                                             const float* __restrict__ tab,
                                                             const float* __restrict__ xs, const float* __restrict__ ys,
                                                             const float* __restrict__ z, SliceGrid g, int64_t first,
                                                             const uint32_t* __restrict__ list,
                                                             const uint64_t* __restrict__ lmodes,
                                                             float* __restrict__ samples, uint32_t* __restrict__ counts) {
    __shared__ float s_f[kMarchBlock];
    __shared__ uint32_t s_w[kMarchBlock / 64];
    const int t = threadIdx.x;
    const uint32_t item = list[blockIdx.x];
    const TileAt at = tile_at(g, first + item);
    // the tile's modes word is block-uniform: uniform skips, scalar instruction fetch
    const uint64_t m64 = lmodes[blockIdx.x];
    const uint64_t m = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(m64 >> 32)) << 32) |
                       (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)m64);
    const int si = t % kS, sj = t / kS;
    float f = 0.f;
    if (t < kSliceSamples && si <= at.nx && sj <= at.ny)
        f = eval_f_pruned<D>(prog, tab, m, xs[kT * at.tx + si], ys[kT * at.ty + sj], z[at.l]);
    s_f[t] = f;
    if (t < kSliceSamples) samples[(size_t)blockIdx.x * kSliceSamples + t] = f;
    __syncthreads();
    uint32_t cnt = 0;
    if (t < kT * kT && (t & (kT - 1)) < at.nx && (t >> 4) < at.ny) {
        cnt = case_segments(cell_case(cell_corners(s_f, t & (kT - 1), t >> 4))) & 3u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, o, 64);
    if ((t & 63) == 0) s_w[t >> 6] = cnt;
    __syncthreads();
    if (t == 0) counts[item] = s_w[0] + s_w[1] + s_w[2] + s_w[3];   // the fifth wave holds no cell
}

// the point on edge E of cell (gi, gj), interpolated from the edge's lower sample a to its higher b.
// E is a compile-time constant: the emit kernel computes the cell's four edge points and selects by
// compare (corner values or points selected by a run-time edge number were built on the stack)
struct EdgePoint { float x, y; uint32_t key; };
template <int E>
__device__ __forceinline__ EdgePoint edge_point(int gi, int gj, uint32_t W, const Corners& c,
                                                const float* __restrict__ xs, const float* __restrict__ ys) {
    const int i = gi + (E == 1 ? 1 : 0), j = gj + (E == 2 ? 1 : 0);   // the edge's lower sample
    const float a = (E == 0 || E == 3) ? c.f0 : (E == 1 ? c.f1 : c.f3);
    const float b = E == 0 ? c.f1 : (E == 3 ? c.f3 : c.f2);
    const float mu = (0.f - a) / (b - a);
    EdgePoint p;
    p.key = 2u * ((uint32_t)j * W + (uint32_t)i) + (uint32_t)(E & 1);
    if (E & 1) {
        const float y0 = ys[j];
        p.x = xs[i];
        p.y = y0 + mu * (ys[j + 1] - y0);
    } else {
        const float x0 = xs[i];
        p.x = x0 + mu * (xs[i + 1] - x0);
        p.y = ys[j];
    }
    return p;
}
__device__ __forceinline__ EdgePoint pick(uint32_t e, const EdgePoint& p0, const EdgePoint& p1, const EdgePoint& p2,
                                          const EdgePoint& p3) {
    EdgePoint r = p0;
    if (e == 1u) r = p1;
    if (e == 2u) r = p2;
    if (e == 3u) r = p3;
    return r;
}

__global__ __launch_bounds__(256) void k_slice_emit(const float* __restrict__ xs, const float* __restrict__ ys,
                                                    SliceGrid g, int64_t first, const uint32_t* __restrict__ list,
                                                    const float* __restrict__ samples,
                                                    const uint32_t* __restrict__ offsets, uint32_t total,
                                                    float4* __restrict__ xy, uint2* __restrict__ keys) {
    __shared__ float s_f[kSliceSamples];
    __shared__ uint32_t s_w[4];
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const uint32_t item = list[blockIdx.x];
    const TileAt at = tile_at(g, first + item);
    const float* src = samples + (size_t)blockIdx.x * kSliceSamples;
    s_f[t] = src[t];
    if (t + 256 < kSliceSamples) s_f[t + 256] = src[t + 256];
    __syncthreads();
    const int ci = t & (kT - 1), cj = t >> 4;
    const Corners f = cell_corners(s_f, ci, cj);   // within the staged 17 x 17 for every lane
    uint32_t segs = 0;
    if (ci < at.nx && cj < at.ny) segs = case_segments(cell_case(f));
    const uint32_t cnt = segs & 3u;
    // exclusive prefix over the block in lane order = cell row-major order
    uint32_t v = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)v, o, 64);
        if (lane >= o) v += y;
    }
    if (lane == 63) s_w[wid] = v;
    __syncthreads();
    uint32_t pre = v - cnt;
    for (int w = 0; w < 4; ++w) pre += (w < wid) ? s_w[w] : 0u;
    const uint32_t base = offsets[item] + pre;
    const uint32_t W = (uint32_t)g.R + 1u;
    const int gi = kT * at.tx + ci, gj = kT * at.ty + cj;
    if (cnt == 0u) return;
    // gi + 1, gj + 1 <= R for a live cell: the coordinate reads stay inside xs, ys
    const EdgePoint p0 = edge_point<0>(gi, gj, W, f, xs, ys), p1 = edge_point<1>(gi, gj, W, f, xs, ys),
                    p2 = edge_point<2>(gi, gj, W, f, xs, ys), p3 = edge_point<3>(gi, gj, W, f, xs, ys);
    for (uint32_t k = 0; k < cnt; ++k) {
        const uint32_t pair = (segs >> (2u + 4u * k)) & 15u;
        const EdgePoint a = pick(pair & 3u, p0, p1, p2, p3), b = pick(pair >> 2, p0, p1, p2, p3);
        if (base + k < total) {   // always, when the counts came from these samples
            xy[base + k] = float4{a.x, a.y, b.x, b.y};
            keys[base + k] = uint2{a.key, b.key};
        }
    }
}

__global__ __launch_bounds__(256) void k_slice_layer_offsets(const uint32_t* __restrict__ offsets, uint32_t tpl,
                                                             uint32_t n_layers, uint32_t* __restrict__ out) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k <= n_layers) out[k] = offsets[(size_t)k * tpl];
}

}  // namespace

void launch_slice_classify(const Program* d_prog, int prog_depth, const float* d_tab, float2 tab_range, const float* d_xs,
                           const float* d_ys, const float* d_z, SliceGrid g, int64_t first, uint32_t n, bool prune,
                           uint32_t* d_list, uint64_t* d_lmodes, SliceState* d_state, hipStream_t s) {
    if (n < 1u || n > kSliceMaxChunk) throw std::runtime_error("slice: chunk size out of range");
    const unsigned blocks = (n + 255u) / 256u;
    const int D = eval_depth(prog_depth), p = prune ? 1 : 0;
#define IMPLI_SLICE_CLASSIFY(DD) \
    k_slice_classify<DD><<<blocks, 256, 0, s>>>(d_prog, d_tab, tab_range, d_xs, d_ys, d_z, g, first, n, p, d_list, d_lmodes, d_state)
    if (D <= 4) IMPLI_SLICE_CLASSIFY(4);
    else if (D <= 8) IMPLI_SLICE_CLASSIFY(8);
    else if (D <= 12) IMPLI_SLICE_CLASSIFY(12);
    else IMPLI_SLICE_CLASSIFY(16);
#undef IMPLI_SLICE_CLASSIFY
}

void launch_slice_march(const Program* d_prog, int prog_depth, const float* d_tab, const float* d_xs, const float* d_ys,
                        const float* d_z, SliceGrid g, int64_t first, uint32_t n_listed, const uint32_t* d_list,
                        const uint64_t* d_lmodes, float* d_samples, uint32_t* d_counts, hipStream_t s) {
    if (n_listed == 0u) return;
    if (n_listed > kSliceMaxChunk) throw std::runtime_error("slice: list longer than a chunk");
    const int D = eval_depth(prog_depth);
#define IMPLI_SLICE_MARCH(DD) \
    k_slice_march<DD><<<n_listed, kMarchBlock, 0, s>>>(d_prog, d_tab, d_xs, d_ys, d_z, g, first, d_list, d_lmodes, d_samples, d_counts)
    if (D <= 4) IMPLI_SLICE_MARCH(4);
    else if (D <= 8) IMPLI_SLICE_MARCH(8);
    else if (D <= 12) IMPLI_SLICE_MARCH(12);
    else IMPLI_SLICE_MARCH(16);
#undef IMPLI_SLICE_MARCH
}

void launch_slice_emit(const float* d_xs, const float* d_ys, SliceGrid g, int64_t first, uint32_t n_listed,
                       const uint32_t* d_list, const float* d_samples, const uint32_t* d_offsets, uint32_t total,
                       float* d_xy, uint32_t* d_keys, hipStream_t s) {
    if (n_listed == 0u || total == 0u) return;
    k_slice_emit<<<n_listed, 256, 0, s>>>(d_xs, d_ys, g, first, d_list, d_samples, d_offsets, total,
                                          reinterpret_cast<float4*>(d_xy), reinterpret_cast<uint2*>(d_keys));
}

void launch_slice_layer_offsets(const uint32_t* d_offsets, uint32_t tpl, uint32_t n_layers, uint32_t* d_out, hipStream_t s) {
    k_slice_layer_offsets<<<(n_layers + 1u + 255u) / 256u, 256, 0, s>>>(d_offsets, tpl, n_layers, d_out);
}

}  // namespace impli
