// distance.hip -- the pixel distance field of the layer images on gfx950 (implisolid_layer_distance): per
// pixel the exact squared Euclidean distance D2 to the nearest pixel of the layer whose solidity (cov >=
// threshold) differs from its own, +D2 for a solid pixel and -D2 for an empty one, kDistNone = 2^30 where
// the layer holds one class only; and per layer the solid pixels, the widest solid pixel and the pixels
// that nothing of the layer below supports.  The chunk's image is raster.hip's (row pitch 16 ntx bytes);
// the distance array is int32 [layer][H][W].
//
// k_distance_columns     : one lane per (layer, column), neighbouring lanes on neighbouring bytes.  A sweep
//                          down stores the distance to the nearest pixel of the other class above (1 at a
//                          change of class, the one above plus 1 otherwise, kDistFar = 32768 while there is
//                          none); a sweep up takes the smaller of it and the same from below and stores the
//                          signed column distance c in place.  kDistFar^2 == kDistNone: the sentinel needs
//                          no special case afterwards.  Rows are read eight at a time ahead of the dependent
//                          chain.
// k_distance_rows        : one block of 256 lanes per (layer, row).  The row's c go into LDS as 16 bits each
//                          (bit 15 the class, bits 0 .. 14 the magnitude, 0 for kDistFar: a real magnitude
//                          is in [1, 16383]), 2 W bytes of dynamic LDS: the widest row, 16384 pixels, takes
//                          32 KiB, under the 64 KiB a block gets without asking, and a 2048-pixel row 4 KiB,
//                          which leaves the occupancy to the wave limit.  A row of one
//                          class whose columns all hold kDistFar is a layer of one class: +-kDistNone,
//                          without a search.  Otherwise a pixel starts from best = c^2 and walks outwards
//                          k = 1, 2, ... while k^2 < best and a neighbour is left on either side, taking
//                          best = min(best, k^2 + g(x +- k)^2) with g the neighbour column's distance to
//                          the pixel's opposite class: 0 where the neighbour is of the other class itself,
//                          its |c| otherwise.  A column farther than sqrt(best) cannot improve best, so
//                          this is exact; the loop ends after at most W - 1 steps.  The results replace
//                          the row's c (every c is in LDS before the first store).  The row's solid pixels
//                          and its largest key (D2 << 32) | (0xFFFFFFFF - index) over the solid pixels go
//                          onto the layer's record with one atomicAdd and one atomicMax per block.
// k_distance_unsupported : four pixels per lane: the solid pixels (dist > 0) whose pixel in the distance layer
//                          below is < -reach2, one atomicAdd per block that found any.
// No kernel waits for another block and every loop is bounded by the input.  Everything is an integer and
// the atomics are sums and maxima: the results depend on no order.
#include <stdexcept>

#include "kernels.hpp"
#include "layer_device.hpp"

namespace impli {

namespace {

constexpr int kBatch = 8;   // rows a column lane reads ahead

__global__ __launch_bounds__(256) void k_distance_columns(LayerGrid g, uint32_t n_cols, const uint8_t* __restrict__ img,
                                                          int32_t* __restrict__ dist) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cols) return;
    const uint32_t ll = i / (uint32_t)g.W, x = i % (uint32_t)g.W;
    const int H = g.H;
    const size_t W = (size_t)g.W, pitch = g.pitch;
    const uint8_t* im = img + (size_t)ll * (size_t)H * pitch + x;   // x < W <= pitch
    int32_t* d = dist + (size_t)ll * (size_t)H * W + x;
    // down: the nearest pixel of the other class above
    int run = kDistFar;
    bool prev = false;
    for (int y0 = 0; y0 < H; y0 += kBatch) {
        bool s[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) s[j] = y0 + j < H && (int)im[(size_t)(y0 + j) * pitch] >= g.threshold;
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const int y = y0 + j;
            if (y < H) {
                if (y > 0 && s[j] != prev) run = 1;
                else if (run != kDistFar) ++run;   // <= y < kDistFar
                prev = s[j];
                d[(size_t)y * W] = run;
            }
        }
    }
    // up: the same from below, the smaller of the two, signed
    run = kDistFar;
    for (int y1 = H - 1; y1 >= 0; y1 -= kBatch) {
        bool s[kBatch];
        int up[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const int y = y1 - j;
            s[j] = y >= 0 && (int)im[(size_t)(y >= 0 ? y : 0) * pitch] >= g.threshold;
            up[j] = y >= 0 ? d[(size_t)y * W] : kDistFar;
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const int y = y1 - j;
            if (y >= 0) {
                if (y < H - 1 && s[j] != prev) run = 1;
                else if (run != kDistFar) ++run;
                prev = s[j];
                const int m = run < up[j] ? run : up[j];
                d[(size_t)y * W] = s[j] ? m : -m;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_distance_rows(LayerGrid g, int l0, int32_t* __restrict__ dist, u64* __restrict__ rec) {
    extern __shared__ uint16_t s_c[];   // the row: 2 W bytes, rounded up to 16 (the static arrays below take 64)
    __shared__ uint32_t s_real[4], s_solid[4];
    __shared__ u64 s_key[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int W = g.W;
    const uint32_t R = blockIdx.x, ll = R / (uint32_t)g.H, py = R % (uint32_t)g.H;
    int32_t* row = dist + (size_t)R * (size_t)W;
    bool real = false;
    uint32_t solid = 0;
    for (int x = t; x < W; x += 256) {
        const int c = row[x];
        const int m = c < 0 ? -c : c;
        s_c[x] = (uint16_t)((c > 0 ? 0x8000 : 0) | (m == kDistFar ? 0 : m));
        real |= m != kDistFar;
        solid += c > 0;
    }
    real = __any(real);
    solid = wave_sum(solid);
    // Not wave_put(): two of them compile to two branches and move the search loop below by 20 bytes, and with that
    // placement layer_distance, layer_hollow and layer_supports each took 3 % longer as a whole call (config 4's tree,
    // 2048 x 2048 x 64 on an MI355X: 63.9 against 62.0 ms for layer_distance, five calls each with a spread of 0.3 ms).
    // As written the kernel is byte for byte the one from before the helpers.
    if (lane == 0) {
        s_real[wv] = real;
        s_solid[wv] = solid;
    }
    __syncthreads();   // every c of the row is in LDS: the stores below overwrite them
    const uint32_t n_solid = block_sum(s_solid);
    const bool one_class = !(s_real[0] | s_real[1] | s_real[2] | s_real[3]) && (n_solid == 0u || n_solid == (uint32_t)W);
    u64 key = 0;
    for (int x = t; x < W; x += 256) {
        const uint32_t v = s_c[x], cls = v >> 15;
        int best = kDistNone;
        if (!one_class) {
            const int c = (v & 0x7fffu) ? (int)(v & 0x7fffu) : kDistFar;
            best = c * c;
            for (int k = 1; k * k < best && (k <= x || x + k < W); ++k) {   // k < W <= 16384
                const int kk = k * k;
                if (k <= x) {
                    const uint32_t u = s_c[x - k];
                    const int gd = (u >> 15) != cls ? 0 : (u & 0x7fffu) ? (int)(u & 0x7fffu) : kDistFar;
                    const int cand = kk + gd * gd;   // < 2^28 + 2^30
                    best = cand < best ? cand : best;
                }
                if (x + k < W) {
                    const uint32_t u = s_c[x + k];
                    const int gd = (u >> 15) != cls ? 0 : (u & 0x7fffu) ? (int)(u & 0x7fffu) : kDistFar;
                    const int cand = kk + gd * gd;
                    best = cand < best ? cand : best;
                }
            }
        }
        row[x] = cls ? best : -best;
        if (cls) {
            const u64 mine = ((u64)(uint32_t)best << 32) | (u64)(0xFFFFFFFFu - (py * (uint32_t)W + (uint32_t)x));
            key = mine > key ? mine : key;
        }
    }
    key = wave_max(key);
    if (lane == 0) s_key[wv] = key;
    __syncthreads();
    if (t == 0 && n_solid) {
        for (int k = 1; k < 4; ++k) key = s_key[k] > key ? s_key[k] : key;
        u64* r = rec + 4 * (size_t)((uint32_t)l0 + ll);
        atomicAdd(r, (u64)n_solid);
        atomicMax(r + 1, key);
    }
}

constexpr uint32_t kPerBlock = 1024;   // pixels per block of k_distance_unsupported

__global__ __launch_bounds__(256) void k_distance_unsupported(LayerGrid g, uint32_t blocks_per_layer, int l0, int reach2,
                                                              const int32_t* __restrict__ dist, const int32_t* __restrict__ carry,
                                                              u64* __restrict__ rec) {
    __shared__ uint32_t s_cnt[4];
    const int t = threadIdx.x;
    const uint32_t ll = blockIdx.x / blocks_per_layer, b = blockIdx.x % blocks_per_layer;
    if (ll == 0u && l0 == 0) return;   // the call's first layer: block-uniform
    const uint32_t px = (uint32_t)g.W * (uint32_t)g.H;   // <= 2^28
    const int32_t* mine = dist + (size_t)ll * px;
    const int32_t* below = ll ? mine - px : carry;
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t p = b * kPerBlock + (uint32_t)j * 256u + (uint32_t)t;
        if (p < px && mine[p] > 0) cnt += below[p] < -reach2;
    }
    wave_put(s_cnt, wave_sum(cnt));
    __syncthreads();
    if (t == 0) {
        const uint32_t total = block_sum(s_cnt);
        if (total) atomicAdd(rec + 4 * (size_t)((uint32_t)l0 + ll) + 2, (u64)total);
    }
}

}  // namespace

void launch_distance_columns(LayerGrid g, uint32_t n_layers, const uint8_t* d_img, int32_t* d_dist, hipStream_t s) {
    check_layer_chunk(g, n_layers, "distance");
    const uint32_t n_cols = n_layers * (uint32_t)g.W;   // <= 2^28
    k_distance_columns<<<(n_cols + 255u) / 256u, 256, 0, s>>>(g, n_cols, d_img, d_dist);
}

void launch_distance_rows(LayerGrid g, uint32_t n_layers, int l0, int32_t* d_dist, unsigned long long* d_rec, hipStream_t s) {
    check_layer_chunk(g, n_layers, "distance");
    const size_t lds = ((size_t)g.W * sizeof(uint16_t) + 15u) & ~(size_t)15u;   // <= 32 KiB: W <= kRasterMaxSide (check)
    k_distance_rows<<<n_layers * (uint32_t)g.H, 256, lds, s>>>(g, l0, d_dist, d_rec);   // <= 2^28 blocks
}

void launch_distance_unsupported(LayerGrid g, uint32_t n_layers, int l0, int64_t reach2, const int32_t* d_dist, const int32_t* d_carry,
                                 unsigned long long* d_rec, hipStream_t s) {
    check_layer_chunk(g, n_layers, "distance");
    if (reach2 < 0 || reach2 >= (int64_t)kDistNone) throw std::runtime_error("distance: reach2 out of range");
    if (l0 > 0 && !d_carry) throw std::runtime_error("distance: a later chunk needs the carried layer");
    if (l0 == 0 && n_layers == 1u) return;   // the call's first layer has nothing below
    const uint32_t bpl = ((uint32_t)g.W * (uint32_t)g.H + kPerBlock - 1u) / kPerBlock;
    k_distance_unsupported<<<n_layers * bpl, 256, 0, s>>>(g, bpl, l0, (int)reach2, d_dist, d_carry, d_rec);   // <= 2^18 + 2^16 blocks
}

}  // namespace impli
