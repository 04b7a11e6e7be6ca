// islands.hip -- connected components of the layer images on gfx950 (implisolid_islands): per layer the
// classes of the solid pixels (cov >= threshold) under 4- or 8-adjacency, each labelled with its smallest
// linear pixel index py W + px (its seed), and one record {seed, area, below, x0, y0, x1, y1, layer} per
// component.  The chunk's image is raster.hip's (row pitch 16 ntx bytes, padding columns zero); the label
// array is int32 [layer][H][W], -1 where the pixel is not solid.  A label is always the index of a pixel of
// the same component that is not larger than the pixel's own: following labels ends at a root (label ==
// own index), and after the merge pass the root is the seed.
//
// k_island_tiles  : one block of 256 lanes per tile of 64 x 32 pixels.  One ballot of cov >= threshold is a
//                   row's solidity word; a pixel starts at the first pixel of its run (bit tricks on the
//                   word, no memory).  Runs of neighbouring rows are joined in LDS by a lock-free union-find
//                   (atomicMin, the smaller index wins): for every shift d of the upper word (0; +-1 under
//                   connectivity 8) the pairs M = Wb & (Wa shifted by d), of which only M & ~(M << 1) are
//                   joined -- the pair one pixel to the left joins the same two runs -- and a diagonal
//                   pair only where the pixel straight above is empty.  The tile's labels are then pointed
//                   at their roots and stored as global indices; the tile's solid pixels go onto the state's
//                   count with one atomic.
// k_island_merge  : one lane per pixel of a tile border (the first row of every tile row but the first,
//                   the first column of every tile column but the first), the same joins across the
//                   border on the global label array, corners and diagonals included.
// k_island_rows   : one wave per image row: its roots (label == own index), by ballot.
// k_island_roots  : one wave per image row: the row's roots in pixel order behind the row's offset (the
//                   exclusive scan of the counts), which is increasing-seed order; the record is initialised
//                   {seed, 0, 0, INT_MAX, seed / W, -1, -1, layer}.
// k_island_tally  : one wave per 64 pixels of a row.  The first lane of every run finds the run's root
//                   (the others take it by a shuffle), every lane stores it as its label; the run's first
//                   lane finds the record by bisection over the layer's seeds and adds the run's length, its
//                   pixels that are solid in the layer below, and its extent: five atomics per run.
// No kernel waits for another block.  Every loop is bounded by the input: a find walks strictly decreasing
// indices, and in a union the larger of the two indices strictly decreases from round to round (see
// unite()), so both end after at most `index` steps; the bisection takes at most 32.
// Everything is an integer: the results depend on no order of the atomics.
#include <climits>
#include <stdexcept>

#include "kernels.hpp"
#include "layer_device.hpp"
#include "unionfind_device.hpp"   // find_lds, find_glb, unite<>

namespace impli {

namespace {

constexpr int kTW = kIslandTileW, kTH = kIslandTileH;
static_assert(kTW == 64, "one ballot is one tile row");
static_assert(kTH % 4 == 0, "the four waves of a block share the rows evenly");

// the first lane of the run of `w` that holds `lane` (bit `lane` of w is set)
__device__ __forceinline__ int run_start(uint64_t w, int lane) {
    const uint64_t gaps = ~w & ((1ull << lane) - 1ull);
    return gaps ? 64 - __clzll((long long)gaps) : 0;
}

__global__ __launch_bounds__(256) void k_island_tiles(IslandGrid g, const uint8_t* __restrict__ img, int32_t* __restrict__ lab,
                                                      IslandState* __restrict__ st) {
    __shared__ uint64_t s_word[kTH];
    __shared__ int s_lab[kTH * kTW];
    __shared__ uint32_t s_cnt[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint32_t tpl = (uint32_t)g.ntx * (uint32_t)g.nty;
    const uint32_t ll = blockIdx.x / tpl, k = blockIdx.x % tpl;
    const int ty = (int)(k / (uint32_t)g.ntx), tx = (int)(k % (uint32_t)g.ntx);
    const int px = tx * kTW + lane;
    const uint8_t* im = img + (size_t)ll * (size_t)g.H * g.pitch;
    int32_t* out = lab + (size_t)ll * (size_t)g.H * (size_t)g.W;
    uint32_t cnt = 0;
    for (int r = wv; r < kTH; r += 4) {
        const int py = ty * kTH + r;
        bool solid = false;
        if (py < g.H && px < g.W) solid = (int)im[(size_t)py * g.pitch + (size_t)px] >= g.threshold;   // px < W <= pitch
        const uint64_t w = __ballot(solid);
        if (lane == 0) s_word[r] = w;
        s_lab[r * kTW + lane] = solid ? r * kTW + run_start(w, lane) : -1;
        cnt += (uint32_t)__popcll((u64)w);
    }
    wave_put(s_cnt, cnt);
    __syncthreads();
    for (int r = wv; r < kTH; r += 4) {
        if (r == 0) continue;
        const uint64_t wb = s_word[r], wa = s_word[r - 1];
        const int me = r * kTW + lane, up = me - kTW;
        uint64_t m = wb & wa;
        if (((m & ~(m << 1)) >> lane) & 1ull) unite<true>(s_lab, me, up);
        if (g.connectivity == 8) {
            m = wb & (wa >> 1);   // bit x: pixel x below, pixel x + 1 above
            if (((m & ~(m << 1) & ~wa) >> lane) & 1ull) unite<true>(s_lab, me, up + 1);
            m = wb & (wa << 1);   // bit x: pixel x below, pixel x - 1 above
            if (((m & ~(m << 1) & ~wa) >> lane) & 1ull) unite<true>(s_lab, me, up - 1);
        }
    }
    __syncthreads();
    for (int r = wv; r < kTH; r += 4) {
        const int py = ty * kTH + r;
        const int v = s_lab[r * kTW + lane];
        int o = -1;
        if (v >= 0) {
            const int root = find_lds(s_lab, v);
            o = (ty * kTH + (root >> 6)) * g.W + tx * kTW + (root & 63);   // a pixel of the image: < W H <= 2^28
        }
        if (py < g.H && px < g.W) out[(size_t)py * (size_t)g.W + (size_t)px] = o;
    }
    if (t == 0) {
        const uint32_t total = block_sum(s_cnt);
        if (total) atomicAdd(&st->solid, (u64)total);
    }
}

__global__ __launch_bounds__(256) void k_island_merge(IslandGrid g, uint32_t n_layers, uint32_t per_layer, int32_t* __restrict__ lab) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)n_layers * per_layer) return;
    const uint32_t ll = (uint32_t)(i / per_layer);
    uint32_t j = (uint32_t)(i % per_layer);
    const int W = g.W, H = g.H;
    int32_t* L = lab + (size_t)ll * (size_t)H * (size_t)W;
    auto solid = [&](int x, int y) {   // labels of solid pixels stay >= 0, the others stay -1
        return x >= 0 && x < W && y >= 0 && y < H && __hip_atomic_load(&L[y * W + x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0;
    };
    const uint32_t n_rows = (uint32_t)(g.nty - 1) * (uint32_t)W;
    if (j < n_rows) {
        // pixel x of the first row of tile row j / W + 1, against the row above: the tile pass's rule
        const int yb = (int)(j / (uint32_t)W + 1u) * kTH, ya = yb - 1, x = (int)(j % (uint32_t)W);
        if (!solid(x, yb)) return;
        const bool left = solid(x - 1, yb), above = solid(x, ya);
        if (above && !(left && solid(x - 1, ya))) unite<false>(L, yb * W + x, ya * W + x);
        if (g.connectivity == 8 && !above) {
            // (x, ya) is empty: nothing to the left joins the runs of (x, yb) and (x + 1, ya)
            if (solid(x + 1, ya)) unite<false>(L, yb * W + x, ya * W + x + 1);
            if (solid(x - 1, ya) && !(left && solid(x - 2, ya))) unite<false>(L, yb * W + x, ya * W + x - 1);
        }
    } else {
        // row y at the seam in front of tile column j / H + 1: the pixel left of it against the ones right of it
        j -= n_rows;
        const int xr = (int)(j / (uint32_t)H + 1u) * kTW, xl = xr - 1, y = (int)(j % (uint32_t)H);
        if (!solid(xl, y)) return;
        const bool right = solid(xr, y);
        if (right) unite<false>(L, y * W + xr, y * W + xl);
        if (g.connectivity == 8 && !right) {
            // a diagonal pair is joined through (xr, y) or (xl, y +- 1) where one of them is solid
            if (solid(xr, y + 1) && !solid(xl, y + 1)) unite<false>(L, (y + 1) * W + xr, y * W + xl);
            if (solid(xr, y - 1) && !solid(xl, y - 1)) unite<false>(L, y * W + xl, (y - 1) * W + xr);
        }
    }
}

__global__ __launch_bounds__(256) void k_island_rows(IslandGrid g, uint32_t rows, const int32_t* __restrict__ lab,
                                                     uint32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const uint32_t R = blockIdx.x * 4u + (threadIdx.x >> 6);   // wave-uniform
    if (R >= rows) return;
    const int py = (int)(R % (uint32_t)g.H);
    const int32_t* row = lab + (size_t)R * (size_t)g.W;
    uint32_t cnt = 0;
    for (int x0 = 0; x0 < g.W; x0 += 64) {
        const int px = x0 + lane;
        const bool root = px < g.W && row[px] == py * g.W + px;
        cnt += (uint32_t)__popcll((u64)__ballot(root));
    }
    if (lane == 0) counts[R] = cnt;
}

__global__ __launch_bounds__(256) void k_island_roots(IslandGrid g, uint32_t rows, int l0, const int32_t* __restrict__ lab,
                                                      const uint32_t* __restrict__ offsets, uint32_t total, int32_t* __restrict__ rec) {
    const int lane = threadIdx.x & 63;
    const uint32_t R = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (R >= rows) return;
    const int py = (int)(R % (uint32_t)g.H), layer = l0 + (int)(R / (uint32_t)g.H);
    const int32_t* row = lab + (size_t)R * (size_t)g.W;
    uint32_t base = offsets[R];
    for (int x0 = 0; x0 < g.W; x0 += 64) {
        const int px = x0 + lane;
        const bool root = px < g.W && row[px] == py * g.W + px;
        const uint64_t m = __ballot(root);
        const uint32_t at = base + (uint32_t)__popcll((u64)(m & ((1ull << lane) - 1ull)));
        if (root && at < total) {   // at < total always: the scan counted these roots
            int4* r = reinterpret_cast<int4*>(rec + 8 * (size_t)at);
            r[0] = make_int4(py * g.W + px, 0, 0, INT_MAX);
            r[1] = make_int4(py, -1, -1, layer);   // the seed is the smallest index: its row is y0
        }
        base += (uint32_t)__popcll((u64)m);
    }
}

__global__ __launch_bounds__(256) void k_island_tally(IslandGrid g, uint32_t n_waves, int l0, const uint8_t* __restrict__ img,
                                                      const uint8_t* __restrict__ carry, int32_t* __restrict__ lab,
                                                      const uint32_t* __restrict__ layer_off, int32_t* __restrict__ rec) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (wave >= n_waves) return;
    const uint32_t nsx = (uint32_t)(g.W + 63) / 64u;
    const uint32_t R = wave / nsx, ll = R / (uint32_t)g.H;
    const int py = (int)(R % (uint32_t)g.H), px = (int)(wave % nsx) * 64 + lane;
    const size_t layer_img = (size_t)g.H * g.pitch;
    int32_t* L = lab + (size_t)ll * (size_t)g.H * (size_t)g.W;
    const bool in = px < g.W;
    const int v = in ? L[py * g.W + px] : -1;
    const bool solid = v >= 0;
    // the layer below: the chunk's image one layer up, the carried image for the chunk's first layer, and
    // for layer 0 of the stack the build plate, which supports every pixel
    const uint8_t* below = ll ? img + (size_t)(ll - 1u) * layer_img : carry;
    bool held = solid;
    if (solid && (ll || l0)) held = (int)below[(size_t)py * g.pitch + (size_t)px] >= g.threshold;
    const uint64_t w = __ballot(solid), wh = __ballot(held);
    const int start = solid ? run_start(w, lane) : lane;
    const bool first = solid && start == lane;
    int root = -1;
    if (first) root = find_glb(L, v);
    root = __shfl(root, start, 64);
    if (solid && root != v) __hip_atomic_store(&L[py * g.W + px], root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!first) return;
    const uint64_t rest = ~(w >> lane);   // its lowest set bit ends the run
    const int len = rest ? __ffsll((long long)rest) - 1 : 64;
    const uint64_t mask = (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << lane;
    const int held_n = __popcll((u64)(wh & mask));
    uint32_t lo = layer_off[ll], hi = layer_off[ll + 1u];
    const uint32_t end = hi;
    while (lo < hi) {   // at most 32 rounds
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (rec[8 * (size_t)mid] < root) lo = mid + 1u;
        else hi = mid;
    }
    if (lo >= end) return;   // never: the root has a record
    int32_t* r = rec + 8 * (size_t)lo;
    atomicAdd(r + 1, len);
    if (held_n) atomicAdd(r + 2, held_n);
    atomicMin(r + 3, px);
    atomicMax(r + 5, px + len - 1);
    atomicMax(r + 6, py);
}

void check(const IslandGrid& g, uint32_t n_layers) {
    check_layer_chunk(g, n_layers, "islands");
    if (g.ntx != (g.W + kTW - 1) / kTW || g.nty != (g.H + kTH - 1) / kTH) throw std::runtime_error("islands: chunk out of range");
}

}  // namespace

IslandGrid island_grid(const LayerGrid& g, int connectivity) {
    return {g, (g.W + kTW - 1) / kTW, (g.H + kTH - 1) / kTH, connectivity};
}

void launch_island_tiles(IslandGrid g, uint32_t n_layers, const uint8_t* d_img, int32_t* d_lab, IslandState* d_state, hipStream_t s) {
    check(g, n_layers);
    const uint32_t blocks = n_layers * (uint32_t)g.ntx * (uint32_t)g.nty;   // <= 2^26 / 64 + borders
    k_island_tiles<<<blocks, 256, 0, s>>>(g, d_img, d_lab, d_state);
}

void launch_island_merge(IslandGrid g, uint32_t n_layers, int32_t* d_lab, hipStream_t s) {
    check(g, n_layers);
    const uint32_t per_layer = (uint32_t)(g.nty - 1) * (uint32_t)g.W + (uint32_t)(g.ntx - 1) * (uint32_t)g.H;
    const uint64_t n = (uint64_t)n_layers * per_layer;   // < pixels / 32 + pixels / 64
    if (n == 0) return;
    k_island_merge<<<(unsigned)((n + 255u) / 256u), 256, 0, s>>>(g, n_layers, per_layer, d_lab);
}

void launch_island_rows(IslandGrid g, uint32_t n_layers, const int32_t* d_lab, uint32_t* d_counts, hipStream_t s) {
    check(g, n_layers);
    const uint32_t rows = n_layers * (uint32_t)g.H;
    k_island_rows<<<(rows + 3u) / 4u, 256, 0, s>>>(g, rows, d_lab, d_counts);
}

void launch_island_roots(IslandGrid g, uint32_t n_layers, int l0, const int32_t* d_lab, const uint32_t* d_offsets, uint32_t total,
                         int32_t* d_rec, hipStream_t s) {
    check(g, n_layers);
    if (total == 0u) return;
    const uint32_t rows = n_layers * (uint32_t)g.H;
    k_island_roots<<<(rows + 3u) / 4u, 256, 0, s>>>(g, rows, l0, d_lab, d_offsets, total, d_rec);
}

void launch_island_tally(IslandGrid g, uint32_t n_layers, int l0, const uint8_t* d_img, const uint8_t* d_carry, int32_t* d_lab,
                         const uint32_t* d_layer_off, int32_t* d_rec, hipStream_t s) {
    check(g, n_layers);
    if (l0 > 0 && !d_carry) throw std::runtime_error("islands: a later chunk needs the carried image");
    const uint32_t n_waves = n_layers * (uint32_t)g.H * ((uint32_t)(g.W + 63) / 64u);   // <= 2^26 / 64 + 2^26 / W borders
    k_island_tally<<<(n_waves + 3u) / 4u, 256, 0, s>>>(g, n_waves, l0, d_img, d_carry, d_lab, d_layer_off, d_rec);
}

}  // namespace impli
