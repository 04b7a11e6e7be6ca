// raster.hip -- per-layer coverage images of the solid on gfx950 (implisolid_raster): on the planes
// z = z[l], the number of solid samples among the s x s of every pixel of a W x H grid, in tiles of
// 16 x 16 pixels.  The chunk's device image has a row pitch of 16 ntx bytes: every tile row is 16
// aligned bytes, stored by one lane as one uint4.
//
// k_raster_classify : one thread per (layer, tile).  With pruning the box of the tile's first and last
//                     samples in x and y (the sample tables are monotone) and {z, z} is bounded by the
//                     interval interpreter: an outside tile is left alone (the image was zeroed), a
//                     solid one (lo >= 0) goes to the fill list, a mixed one (a NaN bound included) to
//                     the evaluate list with the modes word the bound returned.  Without pruning every
//                     tile goes to the evaluate list with modes word 0.  An append costs one ballot,
//                     one prefix and one atomic per wave and list; the lists' order is arbitrary and
//                     nothing downstream depends on it.
// k_raster_eval     : one block of 256 lanes per listed tile, one pixel per lane: its s^2 samples from
//                     eval_f_pruned with the tile's modes word (bit-identical to eval_f inside the box),
//                     solid iff !(f < 0).  The 256 counts are gathered in LDS as bytes, 16 lanes store
//                     one image row of the tile each (padding columns as zeros), and the block's sum
//                     goes onto the layer's with one 64-bit atomic.
// k_raster_fill     : sixteen solid tiles per block, one tile row per lane: s^2 in the tile's nx
//                     pixels of the row, zeros in its padding; the tile's nx ny s^2 goes onto its
//                     layer's sum, tiles of one layer that lie side by side in the block merged first.
//                     No interpreter here: the kernel needs a handful of registers.
// All results are integers: they do not depend on the lists' order, the pruning level or the chunks.
#include <stdexcept>

#include "ifunc_device.hpp"
#include "ifunc_interval.hpp"
#include "brick_modes.hpp"
#include "kernels.hpp"

namespace impli {

using namespace dev;

namespace {

typedef unsigned long long u64;
constexpr int kT = kRasterTile;
constexpr int kFillTiles = 16;   // tiles per block of the fill kernel: one lane per tile row
static_assert(kT == 16 && kT * kT == 256 && kFillTiles * kT == 256, "one pixel, or one tile row, per lane; 16-byte tile rows");

struct TileAt {
    int l, tx, ty, nx, ny;   // layer, tile, its pixels per axis (16, fewer at the border)
};
__device__ __forceinline__ TileAt tile_at(const RasterGrid& g, int64_t item) {
    TileAt t;
    t.l = (int)(item / g.tpl);
    const uint32_t k = (uint32_t)(item % g.tpl);
    t.ty = (int)(k / (uint32_t)g.ntx);
    t.tx = (int)(k % (uint32_t)g.ntx);
    t.nx = min(kT, g.W - kT * t.tx);
    t.ny = min(kT, g.H - kT * t.ty);
    return t;
}
// the 16 bytes of tile row `row` in the chunk's image: row < t.ny, so the image row is below H
__device__ __forceinline__ uint4* tile_row(uint8_t* img, const RasterGrid& g, const TileAt& t, int l0, int row) {
    const size_t r = (size_t)(t.l - l0) * (size_t)g.H + (size_t)(kT * t.ty + row);
    return reinterpret_cast<uint4*>(img + r * g.pitch + (size_t)(kT * t.tx));
}

// one wave's append of its lanes with `push` set: the lane's position in the list
__device__ __forceinline__ uint32_t wave_append(bool push, uint32_t lane, uint32_t* counter) {
    const uint64_t pm = __ballot(push);
    if (!pm) return 0u;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(counter, (uint32_t)__popcll((unsigned long long)pm));
    base = (uint32_t)__shfl((int)base, 0, 64);
    return base + (uint32_t)__popcll((unsigned long long)(pm & ((1ull << lane) - 1ull)));
}

template <int D>
__global__ __launch_bounds__(256) void k_raster_classify(const Program* __restrict__ prog, const float* __restrict__ tab,
                                                          float2 tab_range, const float* __restrict__ mx,
                                                          const float* __restrict__ my, const float* __restrict__ z,
                                                          RasterGrid g, int64_t first, uint32_t n, int prune,
                                                          uint32_t* __restrict__ list, uint64_t* __restrict__ lmodes,
                                                          uint32_t* __restrict__ fill, RasterState* __restrict__ st) {
    // whole waves run to the end (the appends' ballots cover the wave)
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool live = i < n;
    const TileAt t = tile_at(g, first + (live ? i : 0u));
    uint8_t c = kBrickMixed;
    uint64_t m = 0;
    if (live && prune) {
        // the tile's samples lie between its first and last ones: mx, my are monotone in the index.
        // The last sample's index is s (16 tx + nx) - 1 <= W s - 1
        const float zl = z[t.l];
        const int i0 = g.s * kT * t.tx, j0 = g.s * kT * t.ty;
        const Box b{Iv{mx[i0], mx[i0 + g.s * t.nx - 1]}, Iv{my[j0], my[j0 + g.s * t.ny - 1]}, Iv{zl, zl}};
        c = sign_class(eval_iv<D>(prog, tab, tab_range, b, 0ull, m));
    }
    const bool ev = live && c == kBrickMixed, fl = live && c == kBrickPos;
    const uint32_t ae = wave_append(ev, lane, &st->n_eval);
    if (ev && ae < n) {   // ae < n always: every item is appended at most once
        list[ae] = i;
        lmodes[ae] = m;
    }
    const uint32_t af = wave_append(fl, lane, &st->n_fill);
    if (fl && af < n) fill[af] = i;
    uint32_t ns = ev ? (uint32_t)(t.nx * t.ny * g.s * g.s) : 0u;   // at most 4096 a lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ns += (uint32_t)__shfl_xor((int)ns, o, 64);
    if (lane == 0 && ns) atomicAdd(&st->samples, (u64)ns);
}

template <int D>
__global__ __launch_bounds__(256) void k_raster_eval(const Program* __restrict__ prog, const float* __restrict__ tab,
                                                      const float* __restrict__ mx, const float* __restrict__ my,
                                                      const float* __restrict__ z, RasterGrid g, int64_t first, int l0,
                                                      const uint32_t* __restrict__ list,
                                                      const uint64_t* __restrict__ lmodes, uint8_t* __restrict__ img,
                                                      u64* __restrict__ sums) {
    __shared__ __attribute__((aligned(16))) uint8_t s_c[kT * kT];
    __shared__ uint32_t s_w[4];
    const int t = threadIdx.x;
    const TileAt at = tile_at(g, first + list[blockIdx.x]);
    // the tile's modes word is block-uniform: uniform skips, scalar instruction fetch.  The lane read returns an
    // int: the low half goes through uint32_t, or its bit 31 (CSG node 15 pruned to its right operand) would be
    // extended over the high half and give the nodes 16 .. 31 a mode that no interpreter knows
    const uint64_t m64 = lmodes[blockIdx.x];
    const uint64_t m = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m64 >> 32)) << 32) |
                       (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m64);
    const int px = t & (kT - 1), py = t >> 4;
    uint32_t cov = 0;
    if (px < at.nx && py < at.ny) {
        // the pixel's samples: indices s (16 tx + px) + a < W s, s (16 ty + py) + b < H s
        const float zl = z[at.l];
        const float* sx = mx + g.s * (kT * at.tx + px);
        const float* sy = my + g.s * (kT * at.ty + py);
        const int ss = g.s * g.s, sm = g.s - 1, sh = g.s >> 1;   // s in {1, 2, 4}: log2 s = s >> 1
        for (int k = 0; k < ss; ++k) {
            const float f = eval_f_pruned<D>(prog, tab, m, sx[k & sm], sy[k >> sh], zl);
            cov += (f < 0.f) ? 0u : 1u;   // marching cubes' rule: -0.0 and NaN are solid
        }
    }
    s_c[t] = (uint8_t)cov;
    uint32_t sum = cov;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += (uint32_t)__shfl_xor((int)sum, o, 64);
    if ((t & 63) == 0) s_w[t >> 6] = sum;
    __syncthreads();
    if (img && t < at.ny) *tile_row(img, g, at, l0, t) = reinterpret_cast<const uint4*>(s_c)[t];
    if (t == 0) {
        const uint32_t total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        if (total) atomicAdd(&sums[at.l], (u64)total);   // the result is not used: a no-return atomic
    }
}

__global__ __launch_bounds__(256) void k_raster_fill(RasterGrid g, int64_t first, int l0, uint32_t n_fill,
                                                     const uint32_t* __restrict__ fill, uint8_t* __restrict__ img,
                                                     u64* __restrict__ sums) {
    __shared__ int s_l[kFillTiles];
    __shared__ uint32_t s_n[kFillTiles];
    const int t = threadIdx.x, slot = t >> 4, row = t & (kT - 1);
    const uint32_t k = blockIdx.x * (uint32_t)kFillTiles + (uint32_t)slot;
    const bool live = k < n_fill;
    const TileAt at = tile_at(g, first + (live ? fill[k] : 0u));
    if (row == 0) {
        s_l[slot] = live ? at.l : -1;
        s_n[slot] = live ? (uint32_t)(at.nx * at.ny * g.s * g.s) : 0u;
    }
    if (live && img && row < at.ny) {
        // byte p of the row holds s^2 for p < nx, zero in the padding
        const uint32_t v = (uint32_t)(g.s * g.s) * 0x01010101u;
        const int nx = at.nx;
        uint4 w;
        w.x = nx >= 4 ? v : v & ((1u << (8 * nx)) - 1u);
        w.y = nx >= 8 ? v : (nx > 4 ? v & ((1u << (8 * (nx - 4))) - 1u) : 0u);
        w.z = nx >= 12 ? v : (nx > 8 ? v & ((1u << (8 * (nx - 8))) - 1u) : 0u);
        w.w = nx >= 16 ? v : (nx > 12 ? v & ((1u << (8 * (nx - 12))) - 1u) : 0u);
        *tile_row(img, g, at, l0, row) = w;
    }
    __syncthreads();
    if (t == 0) {
        // runs of one layer merge into one atomic: the list is close to item order, so a block's
        // tiles mostly share a layer
        int cur = s_l[0];
        u64 acc = s_n[0];
        for (int q = 1; q < kFillTiles; ++q) {
            const int l = s_l[q];
            if (l != cur) {
                if (cur >= 0 && acc) atomicAdd(&sums[cur], acc);
                cur = l;
                acc = 0ull;
            }
            acc += s_n[q];
        }
        if (cur >= 0 && acc) atomicAdd(&sums[cur], acc);
    }
}

}  // namespace

void launch_raster_classify(const Program* d_prog, int prog_depth, const float* d_tab, float2 tab_range, const float* d_mx,
                            const float* d_my, const float* d_z, RasterGrid g, int64_t first, uint32_t n, bool prune,
                            uint32_t* d_list, uint64_t* d_lmodes, uint32_t* d_fill, RasterState* d_state, hipStream_t s) {
    if (n < 1u || n > kRasterMaxChunk) throw std::runtime_error("raster: chunk size out of range");
    const unsigned blocks = (n + 255u) / 256u;
    const int D = eval_depth(prog_depth), p = prune ? 1 : 0;
#define IMPLI_RASTER_CLASSIFY(DD) \
    k_raster_classify<DD><<<blocks, 256, 0, s>>>(d_prog, d_tab, tab_range, d_mx, d_my, d_z, g, first, n, p, d_list, d_lmodes, d_fill, d_state)
    if (D <= 4) IMPLI_RASTER_CLASSIFY(4);
    else if (D <= 8) IMPLI_RASTER_CLASSIFY(8);
    else if (D <= 12) IMPLI_RASTER_CLASSIFY(12);
    else IMPLI_RASTER_CLASSIFY(16);
#undef IMPLI_RASTER_CLASSIFY
}

void launch_raster_eval(const Program* d_prog, int prog_depth, const float* d_tab, const float* d_mx, const float* d_my,
                        const float* d_z, RasterGrid g, int64_t first, int l0, uint32_t n_listed, const uint32_t* d_list,
                        const uint64_t* d_lmodes, uint8_t* d_img, unsigned long long* d_sums, hipStream_t s) {
    if (n_listed == 0u) return;
    if (n_listed > kRasterMaxChunk) throw std::runtime_error("raster: list longer than a chunk");
    const int D = eval_depth(prog_depth);
#define IMPLI_RASTER_EVAL(DD) \
    k_raster_eval<DD><<<n_listed, 256, 0, s>>>(d_prog, d_tab, d_mx, d_my, d_z, g, first, l0, d_list, d_lmodes, d_img, d_sums)
    if (D <= 4) IMPLI_RASTER_EVAL(4);
    else if (D <= 8) IMPLI_RASTER_EVAL(8);
    else if (D <= 12) IMPLI_RASTER_EVAL(12);
    else IMPLI_RASTER_EVAL(16);
#undef IMPLI_RASTER_EVAL
}

void launch_raster_fill(RasterGrid g, int64_t first, int l0, uint32_t n_fill, const uint32_t* d_fill, uint8_t* d_img,
                        unsigned long long* d_sums, hipStream_t s) {
    if (n_fill == 0u) return;
    if (n_fill > kRasterMaxChunk) throw std::runtime_error("raster: fill list longer than a chunk");
    k_raster_fill<<<(n_fill + kFillTiles - 1u) / kFillTiles, 256, 0, s>>>(g, first, l0, n_fill, d_fill, d_img, d_sums);
}

}  // namespace impli
