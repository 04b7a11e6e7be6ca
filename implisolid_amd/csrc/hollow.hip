// hollow.hip -- the window pass of implisolid_layer_hollow on gfx950: the exact 3D erosion of the layer stack by
// the structuring element wall2, as thresholds on the layers' own 2D squared distance fields (distance.hip).
// Voxel (l, py, px) is core iff dist[m][py][px] > wall2[|m - l|] in every layer m of the call within reach of l,
// and no layer within reach lies outside the call on a side whose bit of `ends` is set (such a layer is empty:
// its pixel straight above or below is at in-plane distance 0 <= wall2).  out = 0 for a core voxel, cov for
// every other; per layer the solid and the core voxels.
//
// The images and the distance fields live in two rings of `ring` layers: layer m of the call in slot m % ring,
// the image as raster.hip left it (H rows of `pitch` = 16 ntx bytes), the field as int32 [H][W].
//
// k_hollow_window : one block of 256 lanes per 1024 pixels of one output layer; a lane takes four neighbouring
//                   pixels of one row, x4 .. x4 + 3 with x4 a multiple of 4: one aligned 4-byte load of the image
//                   (pitch is a multiple of 16) and, where W is a multiple of 4, one aligned 16-byte load per
//                   distance layer and one 4-byte store of out; otherwise per-pixel loads and stores under the
//                   same mapping.  A lane none of whose pixels is solid, or none still core, loads no distance
//                   (with 16-byte loads a lane reads its four pixels together, per-pixel loads skip the empty
//                   ones).  The offsets go 0, +1, -1, +2, -2, ...: the largest thresholds first, which fail
//                   first.  They are taken four at a time: the four layers' loads are issued before the first
//                   compare, and the wave leaves the loop at a vote that none of its lanes is still core.  A step
//                   whose layer lies outside the call, or past the loop's end in the last group of four, tests
//                   the pixel's own layer against a threshold <= wall2[0] again, which changes nothing: the
//                   loop has no branch but the vote.  Layer index, slot and threshold are the same across the
//                   block: they sit in scalar registers and the table is read through the scalar cache.  The
//                   counts are summed over the wave, then over the block in LDS, and land with one atomicAdd
//                   per counter per block that found any.
// No block waits for another; the loop is bounded by 2 reach + 1.  Everything is an integer and the atomics are
// sums: the results depend on no order.
#include <stdexcept>

#include "kernels.hpp"
#include "layer_device.hpp"

namespace impli {

namespace {

constexpr int kAhead = 4;              // distance layers in flight before the first compare

template <bool kVec>
__global__ __launch_bounds__(256) void k_hollow_window(HollowGrid g, uint32_t blocks_per_layer, int l0,
                                                       const uint8_t* __restrict__ img, const int32_t* __restrict__ dist,
                                                       const int32_t* __restrict__ wall2, uint8_t* __restrict__ out,
                                                       u64* __restrict__ rec) {
    __shared__ uint32_t s_solid[4], s_core[4];
    const int t = threadIdx.x;
    const uint32_t ll = blockIdx.x / blocks_per_layer, b = blockIdx.x % blocks_per_layer;
    const int l = l0 + (int)ll;                                  // block-uniform
    const PixelGroup pg = pixel_group(g.W, g.H, b, t);
    const size_t px = (size_t)(uint32_t)g.W * (size_t)g.H, layer_img = (size_t)g.H * g.pitch;
    const size_t at = pg.at;                                     // the group in a distance layer and in out
    const uint32_t slot_l = (uint32_t)l % g.ring;

    const uint32_t cov4 = cov_load4(img + (size_t)slot_l * layer_img + (size_t)pg.y * g.pitch + pg.x4, pg.active);
    uint32_t solid = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
        if (i < pg.nv && cov_solid(cov4, i, g.threshold)) solid |= 1u << i;

    // a layer within reach outside the call, on a side that counts as empty: no voxel of this layer is core
    const bool skinned = ((g.ends & 1) && l < g.reach) || ((g.ends & 2) && l + g.reach >= g.n_layers);
    uint32_t core = skinned ? 0u : solid;
    const int steps = 2 * g.reach + 1;
    for (int k0 = 0; k0 < steps; k0 += kAhead) {
        if (!__any(core != 0u)) break;
        int d[kAhead][4] = {}, w[kAhead];
        const int32_t* p[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const int k = k0 + u, j = (k + 1) >> 1, m = (k & 1) ? l + j : l - j;
            const bool there = k < steps && m >= 0 && m < g.n_layers;
            // j <= reach < ring where the ring is shorter than the call: one wrap at the most; else slot m == m
            uint32_t slot = slot_l;
            if (there) {
                const int sl = (k & 1) ? (int)slot_l + j : (int)slot_l - j;
                slot = (uint32_t)(sl < 0 ? sl + (int)g.ring : sl >= (int)g.ring ? sl - (int)g.ring : sl);
            }
            w[u] = wall2[there ? j : 0];
            p[u] = dist + (size_t)slot * px + at;
        }
        if (kVec) {
            if (core) {
#pragma unroll
                for (int u = 0; u < kAhead; ++u) load4<true>(p[u], 4u, d[u]);
            }
        } else {   // pixel by pixel, each pixel's kAhead layers together: the shared load goes layer by layer
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if ((core >> i) & 1u) {   // a core pixel is solid: inside the row
#pragma unroll
                    for (int u = 0; u < kAhead; ++u) d[u][i] = p[u][i];
                }
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (!(d[u][i] > w[u])) core &= ~(1u << i);
    }

    if (out && pg.active) {
        uint32_t v = cov4;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
            if ((core >> i) & 1u) v &= ~(0xffu << (8u * i));
        uint8_t* o = out + (size_t)ll * px + at;
        if (kVec) {
            *reinterpret_cast<uint32_t*>(o) = v;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i)
                if (i < pg.nv) o[i] = (uint8_t)(v >> (8u * i));
        }
    }

    const uint32_t n_solid = wave_sum((uint32_t)__popc(solid)), n_core = wave_sum((uint32_t)__popc(core));
    if ((t & 63) == 0) {   // both counts under one branch: two wave_put() are two
        s_solid[t >> 6] = n_solid;
        s_core[t >> 6] = n_core;
    }
    __syncthreads();
    if (t == 0) {
        const uint32_t ts = block_sum(s_solid), tc = block_sum(s_core);
        if (ts) atomicAdd(rec + 2 * (size_t)l, (u64)ts);
        if (tc) atomicAdd(rec + 2 * (size_t)l + 1, (u64)tc);
    }
}

}  // namespace

void launch_hollow_window(HollowGrid g, int l0, uint32_t n_out, const uint8_t* d_img, const int32_t* d_dist, const int32_t* d_wall2,
                          uint8_t* d_out, unsigned long long* d_rec, hipStream_t s) {
    check_layer_chunk(g, 1u, "hollow", "grid out of range");
    if (g.threshold < 1 || g.n_layers < 1 || g.reach < 0 || g.reach > kHollowMaxReach || g.ends < 0 || g.ends > 3 || g.ring < 1u ||
        g.ring > (uint32_t)g.n_layers || (g.ring < (uint32_t)g.n_layers && g.ring <= 2u * (uint32_t)g.reach))   // a window fits the ring
        throw std::runtime_error("hollow: grid out of range");
    check_layer_chunk(g, n_out, "hollow", "batch out of range");   // n_out >= 1, and the batch's pixels
    if (l0 < 0 || (uint64_t)l0 + n_out > (uint64_t)g.n_layers || n_out > g.ring) throw std::runtime_error("hollow: batch out of range");
    const uint32_t bpl = groups_blocks(g);
    if (g.W % 4 == 0)
        k_hollow_window<true><<<n_out * bpl, 256, 0, s>>>(g, bpl, l0, d_img, d_dist, d_wall2, d_out, d_rec);
    else
        k_hollow_window<false><<<n_out * bpl, 256, 0, s>>>(g, bpl, l0, d_img, d_dist, d_wall2, d_out, d_rec);
}

}  // namespace impli
