// mass.hip -- volume, centre of mass and inertia of the solid on gfx950 (implisolid_mass): the ten
// integer moments [n, Si, Sj, Sk, Sii, Sjj, Skk, Sij, Sjk, Sik] of the solid cells' indices on the
// N = 2^depth grid of the box's edge table, and the solid cells per z layer.
//
// k_mass_init   : zeroes the state block and the layer counts (every run, a rerun included).
// k_mass_level  : one launch per level l = min(3, depth - 2) .. depth - 2, one thread per box of the
//                 level (box i spans the cells [i << (depth - l), (i + 1) << (depth - l)) per axis): the
//                 level's first boxes with modes word 0, else the eight children of every mixed box the
//                 level above listed, bounded by the interval interpreter over the box's edge extent
//                 from the parent's modes word.  An outside box (hi < 0) is dropped.  A solid one
//                 (lo >= 0) is not cut: every sample in it is solid (edge[k] <= mid[k] <= edge[k + 1]),
//                 so its thread adds the closed-form sums of its index range.  A mixed one (a NaN bound
//                 included) is appended to the level's list: one ballot, one prefix, one atomic per
//                 wave; an entry past the capacity is not written and raises the overflow flag.  The
//                 last level's list is the leaf list: boxes of 4 x 4 x 4 cells.
// k_mass_leaves : one wave per listed leaf, one lane per cell (lane = li + 4 lj + 16 lk): the sample's
//                 value from eval_f_pruned with the leaf's modes word (bit-identical to eval_f inside
//                 the box), solid iff !(f < 0).  The wave reduces the lanes' local sums (packed, every
//                 one below 2^10), lane 0 widens them to the global index sums in 64 bits and adds
//                 them to the block's accumulators in LDS; the block walks the list grid-stride and
//                 issues one set of ten 64-bit atomics at its end.  The layer counts take one
//                 no-return atomic per z layer of the leaf.  Without a list (pruning level 0) the wave's
//                 item is the leaf's own index and the modes word 0.
// All sums are integers: the result does not depend on arrival order, the pruning level or the lists.
#include <algorithm>
#include <stdexcept>

#include "ifunc_device.hpp"
#include "ifunc_interval.hpp"
#include "brick_modes.hpp"
#include "kernels.hpp"

namespace impli {

using namespace dev;

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ u64 sum1(u64 a, u64 b) {   // sum of i, a <= i < b
    return (a + b - 1ull) * (b - a) / 2ull;
}
__device__ __forceinline__ u64 sq_below(u64 m) {      // sum of i^2, i < m
    return m == 0ull ? 0ull : (m - 1ull) * m * (2ull * m - 1ull) / 6ull;
}

// the block's accumulators: the ten moments, then (descent) the cells counted whole
constexpr int kAcc = 11;
__device__ __forceinline__ void acc_clear(u64* s_acc) {
    if (threadIdx.x < kAcc) s_acc[threadIdx.x] = 0ull;
    __syncthreads();
}
__device__ __forceinline__ void acc_flush(const u64* s_acc, MassState* __restrict__ st) {
    __syncthreads();
    const int t = threadIdx.x;
    if (t < kAcc) {
        const u64 v = s_acc[t];
        if (v) atomicAdd(t < 10 ? &st->moments[t] : &st->whole_cells, v);
    }
}

__global__ __launch_bounds__(256) void k_mass_init(MassState* __restrict__ st, u64* __restrict__ layers, int N) {
    const int t = threadIdx.x;
    if (t < 12) st->count[t] = 0u;
    if (t < 10) st->moments[t] = 0ull;
    if (t == 0) {
        st->overflow = 0u;
        st->pad = 0u;
        st->bounded = 0ull;
        st->whole_cells = 0ull;
    }
    for (int k = t; k < N; k += 256) layers[k] = 0ull;
}

template <int D>
__global__ __launch_bounds__(256) void k_mass_level(const Program* __restrict__ prog, const float* __restrict__ tab,
                                                     float2 tab_range, const float* __restrict__ edges, int depth,
                                                     int level, int first, const uint32_t* __restrict__ pbox,
                                                     const uint64_t* __restrict__ pmodes, uint32_t* __restrict__ obox,
                                                     uint64_t* __restrict__ omodes, uint32_t cap,
                                                     MassState* __restrict__ st, u64* __restrict__ layers) {
    __shared__ u64 s_acc[kAcc];
    acc_clear(s_acc);
    const int N = 1 << depth, sh = depth - level;
    const bool top = level == first;
    // cap <= kBoundsMaxList = 2^27: eight children per listed parent stay below 2^32
    const uint32_t total = top ? 1u << (3 * level) : min(st->count[level - 1], cap) * 8u;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t n_eval = 0;   // wave-uniform
    // whole waves iterate (the append's ballot covers the wave)
    for (uint32_t i0 = blockIdx.x * 256u + (threadIdx.x & ~63u); i0 < total; i0 += gridDim.x * 256u) {
        const uint32_t i = i0 + lane;
        const bool live = i < total;
        const uint32_t j = live ? i : 0u;
        uint32_t ix, iy, iz;
        uint64_t m_in = 0;
        if (top) {
            const uint32_t mask = (1u << level) - 1u;
            ix = j & mask; iy = (j >> level) & mask; iz = j >> (2 * level);
        } else {
            const uint32_t p = pbox[j >> 3];
            m_in = pmodes[j >> 3];
            ix = 2u * (p & 1023u) + (j & 1u);
            iy = 2u * ((p >> 10) & 1023u) + ((j >> 1) & 1u);
            iz = 2u * (p >> 20) + ((j >> 2) & 1u);
        }
        // ix + 1 <= 2^level: the edge indices stay within [0, N]
        const float* ey = edges + (N + 1);
        const float* ez = ey + (N + 1);
        uint8_t c = kBrickNeg;
        uint64_t m = 0;
        if (live) {
            const Box b{Iv{edges[ix << sh], edges[(ix + 1u) << sh]}, Iv{ey[iy << sh], ey[(iy + 1u) << sh]},
                        Iv{ez[iz << sh], ez[(iz + 1u) << sh]}};
            c = sign_class(eval_iv<D>(prog, tab, tab_range, b, m_in, m));
        }
        if (live && c == kBrickPos) {
            // the closed-form sums of the index range: every factor is 64 bits wide before it is multiplied
            const u64 w = 1ull << sh;
            const u64 a0 = (u64)ix << sh, b0 = (u64)iy << sh, c0 = (u64)iz << sh;
            const u64 sx = sum1(a0, a0 + w), sy = sum1(b0, b0 + w), sz = sum1(c0, c0 + w);
            const u64 qx = sq_below(a0 + w) - sq_below(a0), qy = sq_below(b0 + w) - sq_below(b0),
                      qz = sq_below(c0 + w) - sq_below(c0);
            const u64 ww = w * w;
            atomicAdd(&s_acc[0], ww * w);
            atomicAdd(&s_acc[1], ww * sx);
            atomicAdd(&s_acc[2], ww * sy);
            atomicAdd(&s_acc[3], ww * sz);
            atomicAdd(&s_acc[4], ww * qx);
            atomicAdd(&s_acc[5], ww * qy);
            atomicAdd(&s_acc[6], ww * qz);
            atomicAdd(&s_acc[7], w * sx * sy);
            atomicAdd(&s_acc[8], w * sy * sz);
            atomicAdd(&s_acc[9], w * sx * sz);
            atomicAdd(&s_acc[10], ww * w);
            // c0 + w <= N: the layer indices stay within [0, N)
            for (u64 k = c0; k < c0 + w; ++k) atomicAdd(&layers[k], ww);
        }
        const bool push = live && c == kBrickMixed;
        const uint64_t pm = __ballot(push);
        if (pm) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&st->count[level], (uint32_t)__popcll((unsigned long long)pm));
            base = (uint32_t)__shfl((int)base, 0, 64);
            const uint32_t at = base + (uint32_t)__popcll((unsigned long long)(pm & ((1ull << lane) - 1ull)));
            if (push) {
                if (at < cap) {
                    obox[at] = ix | (iy << 10) | (iz << 20);
                    omodes[at] = m;
                } else {
                    st->overflow = 1u;
                }
            }
        }
        n_eval += (uint32_t)__popcll((unsigned long long)__ballot(live));
    }
    if (lane == 0 && n_eval) atomicAdd(&st->bounded, (u64)n_eval);
    acc_flush(s_acc, st);
}

template <int D>
__global__ __launch_bounds__(256) void k_mass_leaves(const Program* __restrict__ prog, const float* __restrict__ tab,
                                                      const float* __restrict__ mids, int depth,
                                                      const uint32_t* __restrict__ list,
                                                      const uint64_t* __restrict__ lmodes, uint32_t cap,
                                                      MassState* __restrict__ st, u64* __restrict__ layers) {
    __shared__ u64 s_acc[kAcc];
    acc_clear(s_acc);
    const int N = 1 << depth, lb = depth - 2;   // lb: bits of a leaf index per axis
    const uint32_t total = list ? min(st->count[lb], cap) : 1u << (3 * lb);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t li = lane & 3u, lj = (lane >> 2) & 3u, lk = lane >> 4;
    const float* my = mids + N;
    const float* mz = my + N;
    for (uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6); w < total; w += gridDim.x * 4u) {
        // the leaf and its modes word are wave-uniform: uniform skips, scalar instruction fetch
        uint32_t p;
        uint64_t m = 0;
        if (list) {
            p = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[w]);
            const uint64_t m64 = lmodes[w];
            m = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(m64 >> 32)) << 32) |
                (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)m64);
        } else {
            const uint32_t wu = (uint32_t)__builtin_amdgcn_readfirstlane((int)w), mask = (1u << lb) - 1u;
            p = (wu & mask) | (((wu >> lb) & mask) << 10) | ((wu >> (2 * lb)) << 20);
        }
        // a leaf index is below 2^lb = N / 4: the cell indices stay within [0, N)
        const uint32_t i0 = 4u * (p & 1023u), j0 = 4u * ((p >> 10) & 1023u), k0 = 4u * (p >> 20);
        const float f = eval_f_pruned<D>(prog, tab, m, mids[i0 + li], my[j0 + lj], mz[k0 + lk]);
        const bool solid = !(f < 0.f);   // marching cubes' rule: -0.0 and NaN are solid
        const uint64_t sm = __ballot(solid);
        if (!sm) continue;
        // the lanes' local sums, three fields of 10 bits per word (each sum is at most 64 * 9 = 576)
        uint32_t a = 0, b = 0, c = 0, d = 0;
        if (solid) {
            a = 1u | (li << 10) | (lj << 20);
            b = lk | ((li * li) << 10) | ((lj * lj) << 20);
            c = (lk * lk) | ((li * lj) << 10) | ((lj * lk) << 20);
            d = li * lk;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a += (uint32_t)__shfl_xor((int)a, o, 64);
            b += (uint32_t)__shfl_xor((int)b, o, 64);
            c += (uint32_t)__shfl_xor((int)c, o, 64);
            d += (uint32_t)__shfl_xor((int)d, o, 64);
        }
        if (lane == 0) {
            const u64 n = a & 1023u, si = (a >> 10) & 1023u, sj = a >> 20;
            const u64 sk = b & 1023u, sii = (b >> 10) & 1023u, sjj = b >> 20;
            const u64 skk = c & 1023u, sij = (c >> 10) & 1023u, sjk = c >> 20, sik = d;
            const u64 x = i0, y = j0, z = k0;
            atomicAdd(&s_acc[0], n);
            atomicAdd(&s_acc[1], n * x + si);
            atomicAdd(&s_acc[2], n * y + sj);
            atomicAdd(&s_acc[3], n * z + sk);
            atomicAdd(&s_acc[4], n * x * x + 2ull * x * si + sii);
            atomicAdd(&s_acc[5], n * y * y + 2ull * y * sj + sjj);
            atomicAdd(&s_acc[6], n * z * z + 2ull * z * sk + skk);
            atomicAdd(&s_acc[7], n * x * y + x * sj + y * si + sij);
            atomicAdd(&s_acc[8], n * y * z + y * sk + z * sj + sjk);
            atomicAdd(&s_acc[9], n * x * z + x * sk + z * si + sik);
        }
        if (lane < 4u) {
            const u64 nl = (u64)__popcll((unsigned long long)((sm >> (16u * lane)) & 0xffffull));
            if (nl) atomicAdd(&layers[k0 + lane], nl);   // the result is not used: a no-return atomic
        }
    }
    acc_flush(s_acc, st);
}

}  // namespace

void launch_mass(const Program* d_prog, int prog_depth, const float* d_tab, float2 tab_range, const float* d_edges,
                 const float* d_mids, int depth, bool prune, uint32_t* const d_box[2], uint64_t* const d_modes[2],
                 uint32_t cap, MassState* d_state, unsigned long long* d_layers, hipStream_t s) {
    if (depth < kBoundsMinDepth || depth > kBoundsMaxDepth) throw std::runtime_error("mass: depth must be in [3, 10]");
    if (cap < 1u || cap > kBoundsMaxList) throw std::runtime_error("mass: list capacity out of range");
    const int D = eval_depth(prog_depth);
    const int N = 1 << depth, last = depth - 2, first = std::min(3, last);
    k_mass_init<<<1, 256, 0, s>>>(d_state, d_layers, N);
    const uint32_t* list = nullptr;
    const uint64_t* lmodes = nullptr;
    uint64_t leaves = 1ull << (3 * last);
    if (prune) {
        for (int l = first; l <= last; ++l) {
            // the level holds at most 8^l boxes, and at most eight per listed parent
            const uint64_t most = l == first ? 1ull << (3 * l) : std::min<uint64_t>(1ull << (3 * l), 8ull * cap);
            const unsigned blocks = (unsigned)std::min<uint64_t>((most + 255) / 256, 1024);
            const uint32_t* pb = d_box[(l - 1) & 1];
            const uint64_t* pmo = d_modes[(l - 1) & 1];
            uint32_t* ob = d_box[l & 1];
            uint64_t* om = d_modes[l & 1];
#define IMPLI_MASS_LEVEL(DD) \
    k_mass_level<DD><<<blocks, 256, 0, s>>>(d_prog, d_tab, tab_range, d_edges, depth, l, first, pb, pmo, ob, om, cap, d_state, d_layers)
            if (D <= 4) IMPLI_MASS_LEVEL(4);
            else if (D <= 8) IMPLI_MASS_LEVEL(8);
            else if (D <= 12) IMPLI_MASS_LEVEL(12);
            else IMPLI_MASS_LEVEL(16);
#undef IMPLI_MASS_LEVEL
        }
        list = d_box[last & 1];
        lmodes = d_modes[last & 1];
        leaves = std::min<uint64_t>(leaves, cap);
    }
    // one wave per leaf, four per block, the grid capped: a block walks the list grid-stride
    const unsigned blocks = (unsigned)std::min<uint64_t>((leaves + 3) / 4, 1024);
#define IMPLI_MASS_LEAVES(DD) \
    k_mass_leaves<DD><<<blocks, 256, 0, s>>>(d_prog, d_tab, d_mids, depth, list, lmodes, cap, d_state, d_layers)
    if (D <= 4) IMPLI_MASS_LEAVES(4);
    else if (D <= 8) IMPLI_MASS_LEAVES(8);
    else if (D <= 12) IMPLI_MASS_LEAVES(12);
    else IMPLI_MASS_LEAVES(16);
#undef IMPLI_MASS_LEAVES
}

}  // namespace impli
