// supports.hip -- the passes of implisolid_layer_supports on gfx950: one support tip per non-empty cell of a square
// grid laid over each layer's unsupported pixels, and the layer of the model each tip's column lands on.  A pixel p
// of layer l >= 1 is unsupported iff dist[l][p] > 0 and dist[l - 1][p] < -reach2 (distance.hip's fields); its cell
// is c = (py / cell) ncx + px / cell; a cell's tip is its unsupported pixel of the largest dist, the smallest p
// among equals: the largest key (dist << 32) | (0xFFFFFFFF - p), the form of the row pass's widest key.
//
// The chunk's table holds one 8-byte key and one 4-byte load per (layer, cell), zeroed before the cell pass.
//
// k_support_cells : one block of 256 lanes per 1024 pixels of one layer; a lane takes four neighbouring pixels of
//                   one row, x4 .. x4 + 3 with x4 a multiple of 4: where W is a multiple of 4 one aligned 16-byte
//                   load of the layer and one of the layer below (the carried layer under the chunk's first),
//                   otherwise per-pixel loads under the same mapping.  A lane whose pixels lie in one cell folds
//                   them into one (cell, key, count); the lanes of a wave run through the pixels in order, so the
//                   lanes of one cell in one row are neighbours: a segmented scan over the wave (the heads of the
//                   runs of equal cells from one vote, six shuffle steps of key max and count sum) leaves each
//                   run's result on its last lane, which lands it with one atomicMax and one atomicAdd.  A wave
//                   without an unsupported pixel skips the scan.  A lane whose pixels lie in more than one cell
//                   (a cell side that is no multiple of 4) lands its own runs itself and stands between the runs
//                   of its neighbours.  The layer's unsupported pixels are summed over the wave, then over the
//                   block in LDS: one atomicAdd per block that found any.  The call's first layer does nothing.
// k_support_count : one lane per (layer, cell): counts = key != 0, for the scan.
// k_support_emit  : one lane per (layer, cell) with a tip: the record {p, depth, foot, load} at the cell's offset.
//                   foot: down the chunk's image from the layer two below the tip's (the layer below is empty at p:
//                   that made p unsupported) to the chunk's first, four layers' bytes in flight ahead of the
//                   compares; below that top[p], the highest solid layer at p in front of the chunk.  A record
//                   outside the image, outside its cell or past the total raises *bad instead of writing.
// k_support_top   : one lane per four neighbouring pixels: top raised to the chunk's highest solid layer, the
//                   layers in ascending order, one aligned 4-byte load of the image per layer (pitch is a multiple
//                   of 16), four in flight.
// No kernel waits for another block; the loops are bounded by the chunk's layers.  Everything is an integer and the
// atomics are sums and maxima: the results depend on no order.
#include <stdexcept>

#include "kernels.hpp"
#include "layer_device.hpp"

namespace impli {

namespace {

constexpr uint32_t kNoCell = 0xFFFFFFFFu;  // a lane that takes no part in the wave's runs
constexpr int kAhead = 4;                  // image layers in flight in the foot walk and the top pass

__device__ __forceinline__ u64 tip_key(int dist, uint32_t p) { return ((u64)(uint32_t)dist << 32) | (u64)(0xFFFFFFFFu - p); }

template <bool kVec>
__global__ __launch_bounds__(256) void k_support_cells(SupportGrid g, uint32_t blocks_per_layer, int l0, int reach2,
                                                       const int32_t* __restrict__ dist, const int32_t* __restrict__ carry,
                                                       u64* __restrict__ keys, uint32_t* __restrict__ loads, u64* __restrict__ unsupported) {
    __shared__ uint32_t s_cnt[4];
    const int t = threadIdx.x, lane = t & 63;
    const uint32_t ll = blockIdx.x / blocks_per_layer, b = blockIdx.x % blocks_per_layer;
    if (ll == 0u && l0 == 0) return;   // the call's first layer rests on the plate: block-uniform
    const PixelGroup pg = pixel_group(g.W, g.H, b, t);
    const bool active = pg.active;
    const uint32_t W = (uint32_t)g.W, y = pg.y, x4 = pg.x4, nv = pg.nv;
    const size_t px = (size_t)W * (size_t)g.H, at = pg.at;
    const int32_t* mine = dist + (size_t)ll * px + at;
    const int32_t* below = ll ? mine - px : carry + at;

    int dm[4] = {}, db[4] = {};
    if (kVec) {
        if (active) {
            load4<true>(mine, 4u, dm);
            load4<true>(below, 4u, db);
        }
    } else {   // pixel by pixel, both layers of a pixel together: the shared load goes layer by layer
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
            if (i < nv) {
                dm[i] = mine[i];
                db[i] = below[i];
            }
    }
    uint32_t un = 0;   // the group's unsupported pixels
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
        if (i < nv && dm[i] > 0 && db[i] < -reach2) un |= 1u << i;

    const uint32_t cell = (uint32_t)g.cell, ncc = g.ncx * g.ncy;
    const uint32_t row_cell = (y / cell) * g.ncx, cf = x4 / cell, cl = (x4 + (nv ? nv - 1u : 0u)) / cell;
    u64* kd = keys + (size_t)ll * ncc;
    uint32_t* ld = loads + (size_t)ll * ncc;
    const uint32_t p0 = y * W + x4;   // < 2^28
    uint32_t id = kNoCell, cnt = 0;
    u64 key = 0;
    if (cf == cl) {
        if (active) id = row_cell + cf;   // < ncc
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
            if ((un >> i) & 1u) {
                const u64 k = tip_key(dm[i], p0 + i);
                key = k > key ? k : key;
                ++cnt;
            }
    } else if (un) {   // the group's own runs of equal cells
        uint32_t c_run = cf, n_run = 0;
        u64 k_run = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
            if (i < nv) {
                const uint32_t c = (x4 + i) / cell;   // < ncx
                if (c != c_run) {
                    if (n_run) {
                        atomicMax(kd + row_cell + c_run, k_run);
                        atomicAdd(ld + row_cell + c_run, n_run);
                    }
                    c_run = c, n_run = 0, k_run = 0;
                }
                if ((un >> i) & 1u) {
                    const u64 k = tip_key(dm[i], p0 + i);
                    k_run = k > k_run ? k : k_run;
                    ++n_run;
                }
            }
        if (n_run) {
            atomicMax(kd + row_cell + c_run, k_run);
            atomicAdd(ld + row_cell + c_run, n_run);
        }
    }

    if (__any(cnt != 0u)) {
        // the runs of equal cells along the wave: start = the first lane of this lane's run
        const uint32_t before = (uint32_t)__shfl_up((int)id, 1, 64);
        const u64 heads = __ballot(lane == 0 || before != id);   // bit 0 is set
        const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
#pragma unroll
        for (int d = 1; d <= 32; d <<= 1) {
            const uint32_t oc = (uint32_t)__shfl_up((int)cnt, d, 64);
            const u64 ok = shfl_up64(key, d);
            if (lane - d >= start) {
                cnt += oc;
                key = ok > key ? ok : key;
            }
        }
        const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
        if (tail && cnt) {   // cnt != 0: a run of real cells, id < ncc
            atomicMax(kd + id, key);
            atomicAdd(ld + id, cnt);
        }
    }

    wave_put(s_cnt, wave_sum((uint32_t)__popc(un)));
    __syncthreads();
    if (t == 0) {
        const uint32_t total = block_sum(s_cnt);
        if (total) atomicAdd(unsupported + (size_t)((uint32_t)l0 + ll), (u64)total);
    }
}

__global__ __launch_bounds__(256) void k_support_count(uint32_t n, const u64* __restrict__ keys, uint32_t* __restrict__ counts) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) counts[i] = keys[i] != 0ull;
}

__global__ __launch_bounds__(256) void k_support_emit(SupportGrid g, uint32_t n, int l0, const u64* __restrict__ keys,
                                                      const uint32_t* __restrict__ loads, const uint32_t* __restrict__ offsets,
                                                      uint32_t total, const uint8_t* __restrict__ img, const int32_t* __restrict__ top,
                                                      int4* __restrict__ rec, uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const u64 key = keys[i];
    if (!key) return;
    const uint32_t ncc = g.ncx * g.ncy, ll = i / ncc, c = i % ncc, off = offsets[i];
    const uint32_t W = (uint32_t)g.W, cell = (uint32_t)g.cell;
    const uint32_t p = 0xFFFFFFFFu - (uint32_t)key;
    const uint32_t py = p / W, x = p % W;
    if (off >= total || py >= (uint32_t)g.H || (py / cell) * g.ncx + x / cell != c) {
        atomicOr(bad, 1u);
        return;
    }
    const size_t layer_img = (size_t)g.H * g.pitch;
    const uint8_t* col = img + (size_t)py * g.pitch + x;   // the pixel in the chunk's first layer
    int foot = -1;
    for (int m0 = (int)ll - 2; m0 >= 0 && foot < 0; m0 -= kAhead) {   // at most the chunk's layers
        int v[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) v[u] = m0 - u >= 0 ? (int)col[(size_t)(m0 - u) * layer_img] : 0;
#pragma unroll
        for (int u = 0; u < kAhead; ++u)
            if (foot < 0 && v[u] >= g.threshold) foot = l0 + m0 - u;   // threshold >= 1: a layer not read is not solid
    }
    if (foot < 0 && top) foot = top[p];
    rec[off] = make_int4((int)p, (int)(uint32_t)(key >> 32), foot, (int)loads[i]);
}

template <bool kVec>
__global__ __launch_bounds__(256) void k_support_top(SupportGrid g, uint32_t n_layers, int l0, const uint8_t* __restrict__ img,
                                                     int32_t* __restrict__ top) {
    const PixelGroup pg = pixel_group(g.W, g.H, blockIdx.x, (int)threadIdx.x);
    if (!pg.active) return;
    const uint32_t nv = pg.nv;
    int32_t* tp = top + pg.at;
    int v[4] = {-1, -1, -1, -1};
    if (l0 > 0) load4<kVec>(tp, nv, v);
    const size_t layer_img = (size_t)g.H * g.pitch;
    const uint8_t* q = img + (size_t)pg.y * g.pitch + pg.x4;   // x4 + 4 <= pitch: the padding columns are zero, never solid
    for (uint32_t m0 = 0; m0 < n_layers; m0 += kAhead) {
        uint32_t w[kAhead];
#pragma unroll
        for (uint32_t u = 0; u < kAhead; ++u) w[u] = cov_load4(q + (size_t)(m0 + u) * layer_img, m0 + u < n_layers);
#pragma unroll
        for (uint32_t u = 0; u < kAhead; ++u) {
            const uint32_t solid = cov_solid4(w[u], g.threshold);
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i)
                if ((solid >> i) & 1u) v[i] = l0 + (int)(m0 + u);
        }
    }
    if (kVec) {
        *reinterpret_cast<int4*>(tp) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
            if (i < nv) tp[i] = v[i];
    }
}

void check(const SupportGrid& g, uint32_t n_layers) {
    check_layer_chunk(g, n_layers, "supports");
    if (g.threshold < 1 || g.cell < 1 || g.cell > kSupportMaxCell || g.ncx != ((uint32_t)g.W + (uint32_t)g.cell - 1u) / (uint32_t)g.cell ||
        g.ncy != ((uint32_t)g.H + (uint32_t)g.cell - 1u) / (uint32_t)g.cell)
        throw std::runtime_error("supports: chunk out of range");
}

}  // namespace

SupportGrid support_grid(const LayerGrid& g, int cell) {
    return {g, cell, cell >= 1 ? (uint32_t)((g.W + cell - 1) / cell) : 0u, cell >= 1 ? (uint32_t)((g.H + cell - 1) / cell) : 0u};
}

void launch_support_cells(SupportGrid g, uint32_t n_layers, int l0, int64_t reach2, const int32_t* d_dist, const int32_t* d_carry,
                          unsigned long long* d_keys, uint32_t* d_loads, unsigned long long* d_unsupported, hipStream_t s) {
    check(g, n_layers);
    if (reach2 < 0 || reach2 >= (int64_t)kDistNone) throw std::runtime_error("supports: reach2 out of range");
    if (l0 < 0 || (l0 > 0 && !d_carry)) throw std::runtime_error("supports: a later chunk needs the carried layer");
    if (l0 == 0 && n_layers == 1u) return;   // the call's first layer has nothing below
    const uint32_t bpl = groups_blocks(g);
    if (g.W % 4 == 0)
        k_support_cells<true><<<n_layers * bpl, 256, 0, s>>>(g, bpl, l0, (int)reach2, d_dist, d_carry, d_keys, d_loads, d_unsupported);
    else
        k_support_cells<false><<<n_layers * bpl, 256, 0, s>>>(g, bpl, l0, (int)reach2, d_dist, d_carry, d_keys, d_loads, d_unsupported);
}

void launch_support_count(SupportGrid g, uint32_t n_layers, const unsigned long long* d_keys, uint32_t* d_counts, hipStream_t s) {
    check(g, n_layers);
    const uint32_t n = n_layers * g.ncx * g.ncy;   // <= the chunk's pixels <= 2^28
    k_support_count<<<(n + 255u) / 256u, 256, 0, s>>>(n, d_keys, d_counts);
}

void launch_support_emit(SupportGrid g, uint32_t n_layers, int l0, const unsigned long long* d_keys, const uint32_t* d_loads,
                         const uint32_t* d_offsets, uint32_t total, const uint8_t* d_img, const int32_t* d_top, int32_t* d_rec,
                         uint32_t* d_bad, hipStream_t s) {
    check(g, n_layers);
    if (l0 < 0 || (l0 > 0 && !d_top)) throw std::runtime_error("supports: a later chunk needs the carried tops");
    if (total == 0u) return;
    const uint32_t n = n_layers * g.ncx * g.ncy;
    k_support_emit<<<(n + 255u) / 256u, 256, 0, s>>>(g, n, l0, d_keys, d_loads, d_offsets, total, d_img, l0 > 0 ? d_top : nullptr,
                                                     reinterpret_cast<int4*>(d_rec), d_bad);
}

void launch_support_top(SupportGrid g, uint32_t n_layers, int l0, const uint8_t* d_img, int32_t* d_top, hipStream_t s) {
    check(g, n_layers);
    if (l0 < 0 || !d_top) throw std::runtime_error("supports: no array of tops");
    if (g.W % 4 == 0)
        k_support_top<true><<<groups_blocks(g), 256, 0, s>>>(g, n_layers, l0, d_img, d_top);
    else
        k_support_top<false><<<groups_blocks(g), 256, 0, s>>>(g, n_layers, l0, d_img, d_top);
}

}  // namespace impli
